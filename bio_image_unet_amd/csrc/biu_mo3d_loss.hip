// The five criteria of the 3-D multi-output trainer (multi_output_unet3d/losses.py) on the tensor the model returned for a head, fp32
// contiguous [N, C, D, H, W], which the criteria treat as LOGITS (p = sigmoid(x)); all heads of a step as one autograd node:
//   biu_mo3d_loss_fwd     one launch per head, one pass over (x, t): per-block partial sums, BIU_MO3D_SLOTS floats per row, rows kept per
//                         sample so that Dice (per sample) and Tversky (whole tensor) follow from one layout; no float atomics
//   biu_mo3d_loss_finish  one one-block launch per step: merges every head's rows in a fixed order (fp64), evaluates every criterion and
//                         the weighted total into `saved`
//   biu_mo3d_loss_coef    one one-block launch: d total (device scalar) -> four coefficients per (head, sample)
//   biu_mo3d_loss_bwd     one launch per head: dx = c0 (p - t) + (c1 + c2 t) p (1 - p) + ct (sign(x[z] - x[z-1]) - sign(x[z+1] - x[z]))
// Slots of a partial row: 0 sum BCEWithLogits, 1 sum p, 2 sum t, 3 sum p t, 4 sum |x[z+1] - x[z]| (the temporal kind only).
// The temporal term is the L1 between neighbouring z-planes of x (not of p).  Within a sample the element i = ((c D + z) H + y) W + x has
// z = (i / (H W)) % D and its z-neighbour at i + H W; a pair exists for z < D - 1, so none crosses a channel or a sample.  The neighbour
// plane is re-read through L2 (another block of the same launch streams it at about the same time); no LDS staging.
#include "biu_common.h"

namespace {
enum { K_BCEDICE = 0, K_TVERSKY = 1, K_LCTVERSKY = 2, K_TEMPORAL = 3, K_COUNT = 4 };
constexpr int NS = BIU_MO3D_SLOTS, NACC = 5, HDR = BIU_MO3D_SAVED_HEADER;

struct Args {
    const float* x;
    const float* t;
    const float* coef;      // bwd: [n][4]
    float* out;             // fwd: partial [n][rows][NS]; bwd: dx
    i64 per, hw;            // elements per sample (C D H W) and per z-plane (H W)
    int d, pre_act, narrow; // narrow: per < 2^31, so the z index takes 32-bit divisions
};

template <int V> struct Vec { float v[V]; };
template <int V> __device__ __forceinline__ Vec<V> ldv(const float* p) {
    Vec<V> r;
    if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
    } else {
        r.v[0] = p[0];
    }
    return r;
}
template <int V> __device__ __forceinline__ void stv(float* p, const Vec<V>& a) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]);
    else p[0] = a.v[0];
}
__device__ __forceinline__ float sgn(float x) { return (float)(x > 0.f) - (float)(x < 0.f); }
// the head activation once more (validation, forward only): codes of engine._ACT_CODE
__device__ __forceinline__ float pre(float x, int act) {
    return act == 1 ? 1.f / (1.f + expf(-x)) : (act == 2 ? tanhf(x) : (act == 3 ? fmaxf(x, 0.f) : x));
}
__device__ __forceinline__ int z_of(const Args& a, i64 i) {
    return a.narrow ? (int)(((unsigned)i / (unsigned)a.hw) % (unsigned)a.d) : (int)((i / a.hw) % a.d);
}

// grid (rows, n): block (b, s) strides over sample s; V == 4 only where per % 4 == 0 (and H W % 4 == 0 for the temporal kind), so a
// vector never straddles a sample or a z-plane
template <bool BCE, bool TEMP, int V> __global__ __launch_bounds__(256) void k_mo3d_fwd(const Args a) {
    const i64 base = (i64)blockIdx.y * a.per;
    const float* x = a.x + base;
    const float* t = a.t + base;
    float s[NACC] = {0.f, 0.f, 0.f, 0.f, 0.f};
    const i64 units = a.per / V;
    for (i64 u = (i64)blockIdx.x * 256 + threadIdx.x; u < units; u += (i64)gridDim.x * 256) {
        const i64 i = u * V;
        Vec<V> xv = ldv<V>(x + i);
        const Vec<V> tv = ldv<V>(t + i);
        if (a.pre_act) {
#pragma unroll
            for (int j = 0; j < V; ++j) xv.v[j] = pre(xv.v[j], a.pre_act);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float l = xv.v[j], y = tv.v[j];
            // The pass is bound by the vector ALU, not by HBM, with log1pf and two IEEE divisions per element.  e is in (0, 1], so
            // log(1 + e) through the hardware log differs from log1pf by the rounding of 1 + e (6e-8 absolute against terms of order 1),
            // and the hardware reciprocal is within one ulp; both errors average out in the sums.  The backward pass keeps the divisions:
            // it runs at the memory rate and its error stays in every element.
            const float e = __expf(-fabsf(l)), r = __builtin_amdgcn_rcpf(1.f + e);
            if constexpr (BCE) s[0] += fmaxf(l, 0.f) - l * y + __logf(1.f + e);      // BCEWithLogits, the stable form
            const float p = l >= 0.f ? r : e * r;
            s[1] += p;
            s[2] += y;
            s[3] += p * y;
        }
        if constexpr (TEMP) {
            if (z_of(a, i) < a.d - 1) {
                const Vec<V> nv = ldv<V>(x + i + a.hw);
#pragma unroll
                for (int j = 0; j < V; ++j) s[4] += fabsf(pre(nv.v[j], a.pre_act) - xv.v[j]);
            }
        }
    }
    __shared__ float red[4][NS];      // a row per wave; the five readers below touch consecutive words
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
        const float v = wave_sum(s[k]);
        if (lane == 0) red[wid][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        const int k = threadIdx.x;
        const float v = k < NACC ? (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]) : 0.f;
        a.out[((i64)blockIdx.y * gridDim.x + blockIdx.x) * NS + k] = v;
    }
}

template <bool TEMP, int V> __global__ __launch_bounds__(256) void k_mo3d_bwd(const Args a) {
    const i64 base = (i64)blockIdx.y * a.per;
    const float* x = a.x + base;
    const float* t = a.t + base;
    float* dx = a.out + base;
    const float* c = a.coef + (i64)blockIdx.y * 4;
    const float c0 = c[0], c1 = c[1], c2 = c[2], ct = c[3];
    const i64 units = a.per / V;
    for (i64 u = (i64)blockIdx.x * 256 + threadIdx.x; u < units; u += (i64)gridDim.x * 256) {
        const i64 i = u * V;
        const Vec<V> xv = ldv<V>(x + i), tv = ldv<V>(t + i);
        Vec<V> g;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float l = xv.v[j], y = tv.v[j];
            const float e = __expf(-fabsf(l));
            const float p = l >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
            g.v[j] = c0 * (p - y) + (c1 + c2 * y) * p * (1.f - p);
        }
        if constexpr (TEMP) {
            const int z = z_of(a, i);
            if (z > 0) {
                const Vec<V> pv = ldv<V>(x + i - a.hw);
#pragma unroll
                for (int j = 0; j < V; ++j) g.v[j] += ct * sgn(xv.v[j] - pv.v[j]);
            }
            if (z < a.d - 1) {
                const Vec<V> nv = ldv<V>(x + i + a.hw);
#pragma unroll
                for (int j = 0; j < V; ++j) g.v[j] -= ct * sgn(nv.v[j] - xv.v[j]);
            }
        }
        stv<V>(dx + i, g);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the scalar part: saved = { total, loss of term 0 .. nterms - 1, 0 ..., then from HDR a row of NS floats per (term, sample):
//                            the merged sums of the five slots, 0 x 3 }
// ---------------------------------------------------------------------------------------------------------------------------------
struct Whole { double bce, ps, ts, tp, dice, tdiff; };
__device__ __forceinline__ Whole whole_of(const float* s, int n) {      // fixed order over the samples
    Whole w = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < n; ++i) {
        const float* r = s + (i64)i * NS;
        w.bce += (double)r[0]; w.ps += (double)r[1]; w.ts += (double)r[2]; w.tp += (double)r[3]; w.tdiff += (double)r[4];
        w.dice += 2.0 * ((double)r[3] + 1.0) / ((double)r[1] + (double)r[2] + 1.0);
    }
    return w;
}
__device__ __forceinline__ double tversky(const biu_mo3d_term& t, const Whole& w, double* den) {
    *den = w.tp + (double)t.p0 * (w.ps - w.tp) + (double)t.p1 * (w.ts - w.tp) + (double)t.p2;
    return (w.tp + (double)t.p2) / *den;
}

__global__ __launch_bounds__(1024) void k_mo3d_finish(const biu_mo3d_term* __restrict__ terms, int nterms, const float* __restrict__ ws,
                                                      float* __restrict__ saved) {
    // The table goes to LDS once and the (term, sample, slot) sums of all terms are one flat list of work, so the global round trips of
    // the terms overlap instead of queueing up behind each other: this launch is a chain of latencies, not of arithmetic.
    __shared__ biu_mo3d_term tm[BIU_MO3D_MAX_TERMS];
    __shared__ int first[BIU_MO3D_MAX_TERMS + 1];      // first saved row of a term
    __shared__ float lossf[BIU_MO3D_MAX_TERMS];
    if ((int)threadIdx.x < nterms) tm[threadIdx.x] = terms[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        int r = 0;
        for (int t = 0; t < nterms; ++t) { first[t] = r; r += tm[t].n > 0 ? (int)tm[t].n : 0; }
        first[nterms] = r;
    }
    __syncthreads();
    // one wave per sum, lanes stride over the rows, fixed-order butterfly in fp64
    const int lane = threadIdx.x & 63, nwaves = (int)(blockDim.x >> 6), items = first[nterms] * NS;
    for (int idx = threadIdx.x >> 6; idx < items; idx += nwaves) {
        const int row = idx / NS, k = idx % NS;
        int t = 0;
        while (row >= first[t + 1]) ++t;
        const int i = row - first[t], rows = tm[t].rows;
        const float* part = ws + tm[t].partial_off;
        double s = 0.0;
        if (k < NACC)
            for (int b = lane; b < rows; b += 64) s += (double)part[((i64)i * rows + b) * NS + k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if (lane == 0) saved[HDR + (i64)row * NS + k] = (float)s;
    }
    __syncthreads();
    if ((int)threadIdx.x < nterms) {
        const biu_mo3d_term t = tm[threadIdx.x];
        const Whole w = whole_of(saved + HDR + (i64)first[threadIdx.x] * NS, (int)t.n);
        const double M = (double)t.n * (double)t.per_sample;
        double loss, den;
        switch (t.kind) {
            case K_BCEDICE: loss = (double)t.p0 * (w.bce / M) + (double)t.p1 * (1.0 - w.dice / (double)t.n); break;
            case K_TVERSKY: loss = 1.0 - tversky(t, w, &den); break;
            case K_LCTVERSKY: loss = log(cosh(1.0 - tversky(t, w, &den))); break;
            default:      // an empty slice (D = 1): l1_loss gives nan, whatever its weight
                loss = (double)t.p0 * (w.bce / M + 1.0 - w.dice / (double)t.n) + (t.pairs > 0 ? (double)t.p1 * (w.tdiff / (double)t.pairs) : (double)NAN);
                break;
        }
        saved[1 + threadIdx.x] = lossf[threadIdx.x] = (float)loss;
    } else if ((int)threadIdx.x < HDR - 1) {
        saved[1 + threadIdx.x] = 0.f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int i = 0; i < nterms; ++i) total += (double)tm[i].weight * (double)lossf[i];
        saved[0] = (float)total;
    }
}

__global__ __launch_bounds__(256) void k_mo3d_coef(const biu_mo3d_term* __restrict__ terms, int nterms, const float* __restrict__ g,
                                                   const float* __restrict__ saved, float* __restrict__ coef) {
    i64 row0 = 0;
    for (int ti = 0; ti < nterms; ++ti) {
        const biu_mo3d_term t = terms[ti];
        const int n = (int)t.n;
        const float* s = saved + HDR + row0 * NS;
        const double gw = (double)g[0] * (double)t.weight, M = (double)t.n * (double)t.per_sample;
        double c0 = 0.0, c1 = 0.0, c2 = 0.0, ct = 0.0, dw = 0.0;
        if (t.kind == K_TVERSKY || t.kind == K_LCTVERSKY) {
            double den;
            const Whole w = whole_of(s, n);
            const double tv = tversky(t, w, &den), tps = w.tp + (double)t.p2;
            const double outer = -gw * (t.kind == K_LCTVERSKY ? tanh(1.0 - tv) : 1.0);          // d loss / d Tversky
            c1 = outer * (-tps * (double)t.p0 / (den * den));
            c2 = outer * (1.0 / den - tps * (1.0 - (double)t.p0 - (double)t.p1) / (den * den));
        } else if (t.kind == K_BCEDICE) {
            c0 = gw * (double)t.p0 / M;
            dw = gw * (double)t.p1 / (double)t.n;
        } else {
            c0 = gw * (double)t.p0 / M;
            dw = gw * (double)t.p0 / (double)t.n;
            ct = t.pairs > 0 ? gw * (double)t.p1 / (double)t.pairs : 0.0;
        }
        for (int i = threadIdx.x; i < n; i += 256) {
            const float* r = s + (i64)i * NS;
            double a1 = c1, a2 = c2;
            if (dw != 0.0) {      // 1 - mean_n 2 (I_n + 1) / (P_n + T_n + 1), per sample
                const double den = (double)r[1] + (double)r[2] + 1.0;
                a1 = dw * 2.0 * ((double)r[3] + 1.0) / (den * den);
                a2 = -dw * 2.0 / den;
            }
            float* c = coef + (row0 + i) * 4;
            c[0] = (float)c0; c[1] = (float)a1; c[2] = (float)a2; c[3] = (float)ct;
        }
        row0 += n;
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int fill_args(const char* who, Args& a, int kind, const float* x, const float* target, int n, int c, int d, int h, int w) {
    BIU_REQUIRE(kind >= 0 && kind < K_COUNT, BIU_ERR_UNSUPPORTED, "%s: unknown kind %d", who, kind);
    BIU_REQUIRE(x && target && n > 0 && n <= 65535 && c > 0 && d > 0 && h > 0 && w > 0, BIU_ERR_SHAPE, "%s: bad arguments", who);
    a.x = x; a.t = target; a.coef = nullptr; a.out = nullptr;
    a.hw = (i64)h * w;
    a.per = (i64)c * d * a.hw;
    a.d = d;
    a.pre_act = 0;
    a.narrow = a.per < ((i64)1 << 31) ? 1 : 0;
    return BIU_OK;
}
bool vec4_ok(const Args& a, int kind) {
    return aligned16(a.x) && aligned16(a.t) && aligned16(a.out) && a.per % 4 == 0 && (kind != K_TEMPORAL || a.hw % 4 == 0);
}
}  // namespace

extern "C" int biu_mo3d_loss_blocks(long long numel) {
    long long b = (numel + 4095) / 4096;
    return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

extern "C" int biu_mo3d_loss_fwd(int kind, int pre_act, const float* x, const float* target, int n, int c, int d, int h, int w, float* partial,
                                 biu_stream stream) {
    Args a;
    const int rc = fill_args("mo3d_loss_fwd", a, kind, x, target, n, c, d, h, w);
    if (rc != BIU_OK) return rc;
    BIU_REQUIRE(partial, BIU_ERR_SHAPE, "mo3d_loss_fwd: no partial buffer");
    BIU_REQUIRE(pre_act >= 0 && pre_act <= 3, BIU_ERR_UNSUPPORTED, "mo3d_loss_fwd: unknown activation code %d", pre_act);
    a.out = partial;
    a.pre_act = pre_act;
    const dim3 grid(biu_mo3d_loss_blocks((long long)n * a.per), n);
    hipStream_t st = (hipStream_t)stream;
    const bool v4 = vec4_ok(a, kind), bce = kind == K_BCEDICE || kind == K_TEMPORAL;
    if (kind == K_TEMPORAL) {
        if (v4) hipLaunchKernelGGL((k_mo3d_fwd<true, true, 4>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_mo3d_fwd<true, true, 1>), grid, dim3(256), 0, st, a);
    } else if (bce) {
        if (v4) hipLaunchKernelGGL((k_mo3d_fwd<true, false, 4>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_mo3d_fwd<true, false, 1>), grid, dim3(256), 0, st, a);
    } else {
        if (v4) hipLaunchKernelGGL((k_mo3d_fwd<false, false, 4>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_mo3d_fwd<false, false, 1>), grid, dim3(256), 0, st, a);
    }
    BIU_CHECK_LAUNCH("mo3d_loss_fwd");
    return BIU_OK;
}

extern "C" int biu_mo3d_loss_bwd(int kind, const float* x, const float* target, int n, int c, int d, int h, int w, const float* coef, float* dx,
                                 biu_stream stream) {
    Args a;
    const int rc = fill_args("mo3d_loss_bwd", a, kind, x, target, n, c, d, h, w);
    if (rc != BIU_OK) return rc;
    BIU_REQUIRE(coef && dx, BIU_ERR_SHAPE, "mo3d_loss_bwd: bad arguments");
    a.coef = coef;
    a.out = dx;
    const bool v4 = vec4_ok(a, kind);
    const dim3 grid(grid_for(a.per / (v4 ? 4 : 1), 256, 2048), n);
    hipStream_t st = (hipStream_t)stream;
    if (kind == K_TEMPORAL) {
        if (v4) hipLaunchKernelGGL((k_mo3d_bwd<true, 4>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_mo3d_bwd<true, 1>), grid, dim3(256), 0, st, a);
    } else {
        if (v4) hipLaunchKernelGGL((k_mo3d_bwd<false, 4>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_mo3d_bwd<false, 1>), grid, dim3(256), 0, st, a);
    }
    BIU_CHECK_LAUNCH("mo3d_loss_bwd");
    return BIU_OK;
}

extern "C" int biu_mo3d_loss_finish(const biu_mo3d_term* terms, int nterms, const float* workspace, float* saved, biu_stream stream) {
    BIU_REQUIRE(terms && workspace && saved && nterms >= 1 && nterms <= BIU_MO3D_MAX_TERMS, BIU_ERR_SHAPE, "mo3d_loss_finish: bad arguments");
    hipLaunchKernelGGL(k_mo3d_finish, dim3(1), dim3(1024), 0, (hipStream_t)stream, terms, nterms, workspace, saved);
    BIU_CHECK_LAUNCH("mo3d_loss_finish");
    return BIU_OK;
}

extern "C" int biu_mo3d_loss_coef(const biu_mo3d_term* terms, int nterms, const float* g, const float* saved, float* coef, biu_stream stream) {
    BIU_REQUIRE(terms && g && saved && coef && nterms >= 1 && nterms <= BIU_MO3D_MAX_TERMS, BIU_ERR_SHAPE, "mo3d_loss_coef: bad arguments");
    hipLaunchKernelGGL(k_mo3d_coef, dim3(1), dim3(256), 0, (hipStream_t)stream, terms, nterms, g, saved, coef);
    BIU_CHECK_LAUNCH("mo3d_loss_coef");
    return BIU_OK;
}
