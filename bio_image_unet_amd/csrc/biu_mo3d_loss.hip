// The segmentation criteria on fp32 contiguous LOGITS (p = sigmoid(x)), one implementation for the single-head criteria of
// bio_image_unet_amd/losses.py (any rank, seen as [N, per]) and the five of the 3-D multi-output trainer (multi_output_unet3d/losses.py,
// [N, C, D, H, W]); all terms of a step are one autograd node:
//   biu_mo3d_loss_fwd       one launch per head, one pass over (x, t): per-block partial sums, NS floats per row, rows kept per sample so
//                           that Dice (per sample) and Tversky (whole tensor) follow from one layout; no float atomics
//   biu_pair_smooth_l1_fwd  the K_PAIRSL1 term's pass over x: one row per block, the block's sum in slot 0
//   biu_mo3d_loss_finish    one one-block launch per step: merges every term's rows in a fixed order (fp64), evaluates every criterion and
//                           the weighted total into `saved`
//   biu_mo3d_loss_coef      one one-block launch: d total (device scalar) -> four coefficients per (term, sample)
//   biu_mo3d_loss_bwd       one launch per head: dx = c0 (p - t) + (c1 + c2 t) p (1 - p) + ct (sign(x[z] - x[z-1]) - sign(x[z+1] - x[z]))
//   biu_pair_smooth_l1_bwd  dx (+)= c0 d sum SmoothL1 / dx, c0 read from the K_PAIRSL1 term's coefficient row
// Kinds and the (p0, p1, p2) of their biu_mo3d_term:
//   K_BCEDICE    (alpha, beta, s)     alpha mean BCEWithLogits + beta (1 - mean_n 2 (PT_n + s) / (P_n + T_n + s))
//   K_TVERSKY    (alpha, beta, s)     1 - Tv, Tv = (TP + s) / (TP + alpha FP + beta FN + s) over the whole tensor
//   K_LCTVERSKY  (alpha, beta, s)     log cosh(1 - Tv)
//   K_TEMPORAL   (w0, w1, -)          w0 BCEDice(1, 1) with s = 1 + w1 sum |x[z+1] - x[z]| / pairs; nan when pairs == 0
//   K_PAIRSL1    (-, -, -)            sum SmoothL1(x[i + per] - x[i]) / pairs between neighbouring BATCH entries, pairs = (N - 1) per; a
//                                     term with n = 1 and rows = biu_pair_smooth_l1_blocks(pairs), it has no fwd / bwd launch of its own kind
// Slots of a partial row: 0 sum BCEWithLogits (K_PAIRSL1: sum SmoothL1), 1 sum p, 2 sum t, 3 sum p t, 4 sum |x[z+1] - x[z]| (K_TEMPORAL),
// 5..7 zero.
// saved = { total, loss of term 0 .. nterms - 1, 0 ... up to HDR, then a row of NS floats per (term, sample) in table order: the merged
// slots }; coef = { c0, c1, c2, ct } per (term, sample) in the same order.
// The temporal term is the L1 between neighbouring z-planes of x (not of p).  Within a sample the element i = ((c D + z) H + y) W + x has
// z = (i / (H W)) % D and its z-neighbour at i + H W; a pair exists for z < D - 1, so none crosses a channel or a sample.  The neighbour
// plane is re-read through L2 (another block of the same launch streams it at about the same time); no LDS staging.
#include "biu_common.h"

namespace {
enum { K_BCEDICE = 0, K_TVERSKY = 1, K_LCTVERSKY = 2, K_TEMPORAL = 3, K_COUNT = 4 /* kinds of _fwd / _bwd */, K_PAIRSL1 = BIU_MO3D_PAIR_SL1 };
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

// SmoothL1 (beta = 1, mean) between neighbouring BATCH entries of the logits -- the 3-D trainer's "time" term
// nn.SmoothL1Loss()(y_logits[1:], y_logits[:-1]) (unet3d/train.py:140-145).  d_i = l[i+1] - l[i] for i < (n-1)*per_sample.
__device__ __forceinline__ float sl1(float d) { const float a = fabsf(d); return a < 1.f ? 0.5f * d * d : a - 0.5f; }
__device__ __forceinline__ float dsl1(float d) { return d > 1.f ? 1.f : (d < -1.f ? -1.f : d); }
__global__ __launch_bounds__(256) void k_pair_sl1_fwd(const float* __restrict__ lg, i64 per_sample, i64 pairs, float* __restrict__ partial) {
    float s = 0.f;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += (i64)gridDim.x * blockDim.x) s += sl1(lg[i + per_sample] - lg[i]);
    __shared__ float red[16];
    const float r = block_sum(s, red);
    if (threadIdx.x == 0) {
        float* row = partial + (i64)blockIdx.x * NS;
        row[0] = r;
#pragma unroll
        for (int k = 1; k < NS; ++k) row[k] = 0.f;
    }
}
// dl[j] (+)= c * (h'(l[j] - l[j - P]) [j >= P]  -  h'(l[j + P] - l[j]) [j < pairs]),  c = upstream gradient * weight / pairs
__global__ __launch_bounds__(256) void k_pair_sl1_bwd(const float* __restrict__ lg, i64 per_sample, i64 total, const float* __restrict__ coef,
                                                      float* __restrict__ dl, int accumulate) {
    const float c = coef[0];
    const i64 pairs = total - per_sample;
    for (i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (i64)gridDim.x * blockDim.x) {
        const float x = lg[j];
        float g = 0.f;
        if (j >= per_sample) g += dsl1(x - lg[j - per_sample]);
        if (j < pairs) g -= dsl1(lg[j + per_sample] - x);
        g *= c;
        dl[j] = accumulate ? dl[j] + g : g;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the scalar part: saved = { total, loss of term 0 .. nterms - 1, 0 ..., then from HDR a row of NS floats per (term, sample):
//                            the merged sums of the five slots, 0 x 3 }
// `sm` is the Dice smooth: p2 of a K_BCEDICE term, 1 for K_TEMPORAL.
// ---------------------------------------------------------------------------------------------------------------------------------
struct Whole { double bce, ps, ts, tp, dice, tdiff; };
__device__ __forceinline__ double dice_smooth(const biu_mo3d_term& t) { return t.kind == K_BCEDICE ? (double)t.p2 : 1.0; }
__device__ __forceinline__ Whole whole_of(const float* s, int n, double sm) {      // fixed order over the samples
    Whole w = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < n; ++i) {
        const float* r = s + (i64)i * NS;
        w.bce += (double)r[0]; w.ps += (double)r[1]; w.ts += (double)r[2]; w.tp += (double)r[3]; w.tdiff += (double)r[4];
        w.dice += 2.0 * ((double)r[3] + sm) / ((double)r[1] + (double)r[2] + sm);
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
        const Whole w = whole_of(saved + HDR + (i64)first[threadIdx.x] * NS, (int)t.n, dice_smooth(t));
        const double M = (double)t.n * (double)t.per_sample;
        double loss, den;
        switch (t.kind) {
            case K_BCEDICE: loss = (double)t.p0 * (w.bce / M) + (double)t.p1 * (1.0 - w.dice / (double)t.n); break;
            case K_TVERSKY: loss = 1.0 - tversky(t, w, &den); break;
            case K_LCTVERSKY: loss = log(cosh(1.0 - tversky(t, w, &den))); break;
            case K_PAIRSL1: loss = w.bce / (double)t.pairs; break;
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
        const double sm = dice_smooth(t);
        double c0 = 0.0, c1 = 0.0, c2 = 0.0, ct = 0.0, dw = 0.0;
        if (t.kind == K_TVERSKY || t.kind == K_LCTVERSKY) {
            double den;
            const Whole w = whole_of(s, n, 1.0);
            const double tv = tversky(t, w, &den), tps = w.tp + (double)t.p2;
            const double outer = -gw * (t.kind == K_LCTVERSKY ? tanh(1.0 - tv) : 1.0);          // d loss / d Tversky
            c1 = outer * (-tps * (double)t.p0 / (den * den));
            c2 = outer * (1.0 / den - tps * (1.0 - (double)t.p0 - (double)t.p1) / (den * den));
        } else if (t.kind == K_BCEDICE) {
            c0 = gw * (double)t.p0 / M;
            dw = gw * (double)t.p1 / (double)t.n;
        } else if (t.kind == K_PAIRSL1) {
            c0 = gw / (double)t.pairs;
        } else {
            c0 = gw * (double)t.p0 / M;
            dw = gw * (double)t.p0 / (double)t.n;
            ct = t.pairs > 0 ? gw * (double)t.p1 / (double)t.pairs : 0.0;
        }
        for (int i = threadIdx.x; i < n; i += 256) {
            const float* r = s + (i64)i * NS;
            double a1 = c1, a2 = c2;
            if (dw != 0.0) {      // 1 - mean_n 2 (I_n + s) / (P_n + T_n + s), per sample
                const double den = (double)r[1] + (double)r[2] + sm;
                a1 = dw * 2.0 * ((double)r[3] + sm) / (den * den);
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

extern "C" int biu_pair_smooth_l1_blocks(long long pairs) {
    long long b = (pairs + 256 * 8 - 1) / (256 * 8);
    return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}
extern "C" int biu_pair_smooth_l1_fwd(const float* logits, int n, long long per_sample, float* partial, biu_stream stream) {
    BIU_REQUIRE(logits && partial && n > 1 && per_sample > 0, BIU_ERR_SHAPE, "pair_smooth_l1_fwd: needs at least two batch entries");
    const i64 pairs = (i64)(n - 1) * per_sample;
    hipLaunchKernelGGL(k_pair_sl1_fwd, dim3(biu_pair_smooth_l1_blocks(pairs)), dim3(256), 0, (hipStream_t)stream, logits, (i64)per_sample, pairs, partial);
    BIU_CHECK_LAUNCH("pair_smooth_l1_fwd");
    return BIU_OK;
}
extern "C" int biu_pair_smooth_l1_bwd(const float* logits, int n, long long per_sample, const float* coef, float* dlogits, int accumulate,
                                      biu_stream stream) {
    BIU_REQUIRE(logits && coef && dlogits && n > 1 && per_sample > 0, BIU_ERR_SHAPE, "pair_smooth_l1_bwd: bad arguments");
    const i64 total = (i64)n * per_sample;
    hipLaunchKernelGGL(k_pair_sl1_bwd, dim3(grid_for(total, 256, 4096)), dim3(256), 0, (hipStream_t)stream, logits, (i64)per_sample, total, coef,
                       dlogits, accumulate);
    BIU_CHECK_LAUNCH("pair_smooth_l1_bwd");
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
