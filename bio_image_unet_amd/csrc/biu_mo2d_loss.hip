// The ten criteria of the 2-D multi-output trainer (multi_output_unet/losses.py) on ACTIVATED head outputs, fp32 contiguous [N, C, H, W],
// fused per head over its deep-supervision levels (multi_output_unet/train.py:157-181):
//   biu_mo2d_loss_fwd     one launch per head: the target is read once, up to four prediction tensors against it; per-block partial sums,
//                         BIU_MO2D_SLOTS floats per (level, block); no float atomics, so a step repeats bit for bit
//   biu_mo2d_loss_finish  one one-block launch per step: merges every head's partials in a fixed order (fp64), evaluates every criterion
//                         and the weighted total into `saved`
//   biu_mo2d_loss_coef    one one-block launch: d total (device scalar) -> four coefficients per (head, level)
//   biu_mo2d_loss_bwd     one launch per head: d total / d pred for all its levels; the torch.gradient terms gather their +-2 stencil
// e = pred - target; G_y, G_x = torch.gradient along H and W (central differences, one-sided at the edges).
//
// Slots of a (level, block) partial row, by kind:
//   BCEDice / Tversky / logcoshTversky : 0 sum bce, 1 sum p, 2 sum t, 3 sum p t, 4 #pred outside [0, 1], 5 #target outside [0, 1]
//   MSE / MAE / Huber                  : 0 sum of the per-element loss
//   DistanceGradient / Weighted...     : 0 sum e~^2, 1 sum |e~|, 2 sum (G_y e~)^2, 3 sum (G_x e~)^2        (e~ = w e, w from the target)
//   WeightedVectorField                : 0 sum (w e)^2, 1 sum |w e|, 2 sum_pixels (w (|p|^2 - |t|^2))^2
// The +-2 halo of the backward stencil is re-read through L1 / L2 (five row loads per element): a head tensor is at most a few MB,
// the rows a block touches are contiguous and shared with its neighbours, and LDS staging would add a barrier per tile for no traffic saved.
#include "biu_common.h"

namespace {
enum { K_BCEDICE = 0, K_TVERSKY = 1, K_LCTVERSKY = 2, K_MSE = 3, K_MAE = 4, K_HUBER = 5, K_DGRAD = 6, K_WDGRAD = 7, K_WVF = 8, K_COUNT = 9 };
enum { G_PROB = 0, G_REG = 1, G_STENCIL = 2, G_VEC = 3 };
constexpr int NS = BIU_MO2D_SLOTS, NL = BIU_MO2D_MAX_LEVELS, NACC = 6;

struct HeadArgs {
    const float* pred[NL];
    float* dpred[NL];
    const float* target;
    const float* coef;      // bwd: [nlev][4]
    float* partial;         // fwd: [nlev][nb][NS]
    int nlev, kind, n, c, h, w;
    float pa, pb;           // Huber: delta; weighted kinds: weight where the target is set / elsewhere
    i64 total;
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
template <int V> __device__ __forceinline__ Vec<V> zerov() {
    Vec<V> r;
#pragma unroll
    for (int j = 0; j < V; ++j) r.v[j] = 0.f;
    return r;
}
__device__ __forceinline__ float sgn(float x) { return (float)(x > 0.f) - (float)(x < 0.f); }
__device__ __forceinline__ float wof(const HeadArgs& a, float t) { return a.kind == K_WDGRAD ? (t > 0.f ? a.pa : a.pb) : 1.f; }

// ---------------------------------------------------------------------------------------------------------------------------------
// forward: V consecutive elements from flat index `idx` (for the stencil / vector-field kinds V consecutive columns of one row)
// ---------------------------------------------------------------------------------------------------------------------------------
template <int GRP, int V> __device__ __forceinline__ void fwd_unit(const HeadArgs& a, i64 idx, float (&acc)[NL][NACC]) {
    if constexpr (GRP == G_PROB) {
        const Vec<V> t = ldv<V>(a.target + idx);
        float st = 0.f, ot = 0.f;
#pragma unroll
        for (int j = 0; j < V; ++j) { st += t.v[j]; ot += (t.v[j] >= 0.f && t.v[j] <= 1.f) ? 0.f : 1.f; }
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if (l >= a.nlev) break;
            const Vec<V> p = ldv<V>(a.pred[l] + idx);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float x = p.v[j], y = t.v[j];
                if (a.kind == K_BCEDICE)      // nn.BCELoss: both logs clamped at -100 (accurate logf / log1pf: the tolerance near p -> 1 needs them)
                    acc[l][0] += (y - 1.f) * fmaxf(log1pf(-x), -100.f) - y * fmaxf(logf(x), -100.f);
                acc[l][1] += x;
                acc[l][3] += x * y;
                acc[l][4] += (x >= 0.f && x <= 1.f) ? 0.f : 1.f;
            }
            acc[l][2] += st;
            acc[l][5] += ot;
        }
    } else if constexpr (GRP == G_REG) {
        const Vec<V> t = ldv<V>(a.target + idx);
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if (l >= a.nlev) break;
            const Vec<V> p = ldv<V>(a.pred[l] + idx);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float e = p.v[j] - t.v[j], d = fabsf(e);
                acc[l][0] += a.kind == K_MSE ? e * e : (a.kind == K_MAE ? d : (d < a.pa ? 0.5f * d * d : a.pa * (d - 0.5f * a.pa)));
            }
        }
    } else if constexpr (GRP == G_STENCIL) {
        const int W = a.w, H = a.h;
        const int x0 = (int)(idx % W), y = (int)((idx / W) % H);
        const i64 up = y > 0 ? idx - W : idx, dn = y < H - 1 ? idx + W : idx;
        const i64 lf = x0 > 0 ? idx - 1 : idx, rt = x0 + V < W ? idx + V : idx + V - 1;
        const float sy = (y == 0 || y == H - 1) ? 1.f : 0.5f;
        const Vec<V> tc = ldv<V>(a.target + idx), tu = ldv<V>(a.target + up), td = ldv<V>(a.target + dn);
        const float tl = a.target[lf], tr = a.target[rt];
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if (l >= a.nlev) break;
            const float* p = a.pred[l];
            const Vec<V> pc = ldv<V>(p + idx), pu = ldv<V>(p + up), pd = ldv<V>(p + dn);
            float er[V + 2];
            er[0] = wof(a, tl) * (p[lf] - tl);
            er[V + 1] = wof(a, tr) * (p[rt] - tr);
#pragma unroll
            for (int j = 0; j < V; ++j) er[j + 1] = wof(a, tc.v[j]) * (pc.v[j] - tc.v[j]);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float e = er[j + 1];
                const float gy = sy * (wof(a, td.v[j]) * (pd.v[j] - td.v[j]) - wof(a, tu.v[j]) * (pu.v[j] - tu.v[j]));
                const int x = x0 + j;
                const float gx = ((x == 0 || x == W - 1) ? 1.f : 0.5f) * (er[j + 2] - er[j]);
                acc[l][0] += e * e;
                acc[l][1] += fabsf(e);
                acc[l][2] += gy * gy;
                acc[l][3] += gx * gx;
            }
        }
    } else {      // G_VEC: idx runs over the N*H*W pixels; the two components are H*W apart
        const i64 hw = (i64)a.h * a.w;
        const i64 o0 = (idx / hw) * 2 * hw + idx % hw, o1 = o0 + hw;
        const Vec<V> t0 = ldv<V>(a.target + o0), t1 = ldv<V>(a.target + o1);
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if (l >= a.nlev) break;
            const Vec<V> p0 = ldv<V>(a.pred[l] + o0), p1 = ldv<V>(a.pred[l] + o1);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float w = (t0.v[j] == 0.f && t1.v[j] == 0.f) ? a.pb : a.pa;
                const float u0 = w * (p0.v[j] - t0.v[j]), u1 = w * (p1.v[j] - t1.v[j]);
                const float m = w * (p0.v[j] * p0.v[j] + p1.v[j] * p1.v[j]) - w * (t0.v[j] * t0.v[j] + t1.v[j] * t1.v[j]);
                acc[l][0] += u0 * u0 + u1 * u1;
                acc[l][1] += fabsf(u0) + fabsf(u1);
                acc[l][2] += m * m;
            }
        }
    }
}

template <int GRP, int V> __global__ __launch_bounds__(256) void k_mo2d_fwd(const HeadArgs a) {
    float acc[NL][NACC];
#pragma unroll
    for (int l = 0; l < NL; ++l)
#pragma unroll
        for (int k = 0; k < NACC; ++k) acc[l][k] = 0.f;
    const i64 span = GRP == G_VEC ? a.total / 2 : a.total;       // the vector-field kind walks pixels
    const i64 units = span / V;
    for (i64 u = (i64)blockIdx.x * 256 + threadIdx.x; u < units; u += (i64)gridDim.x * 256) fwd_unit<GRP, V>(a, u * V, acc);
    if constexpr (V == 4 && (GRP == G_PROB || GRP == G_REG)) {      // scalar tail of a flat tensor whose length is no multiple of 4
        const i64 done = units * 4;
        if (blockIdx.x == 0 && (i64)threadIdx.x < span - done) fwd_unit<GRP, 1>(a, done + threadIdx.x, acc);
    }
    __shared__ float red[4][NL * NACC];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int l = 0; l < NL; ++l)
#pragma unroll
        for (int k = 0; k < NACC; ++k) {
            const float v = wave_sum(acc[l][k]);
            if (lane == 0) red[wid][l * NACC + k] = v;
        }
    __syncthreads();
    if (threadIdx.x < NL * NACC) {
        const int l = threadIdx.x / NACC, k = threadIdx.x % NACC;
        if (l < a.nlev)
            a.partial[((i64)l * gridDim.x + blockIdx.x) * NS + k] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------------------------------------
// One term of (G^T G e)_i along an axis of extent n >= 2: row j = i + DJ of G (torch.gradient), v[k] = e[i + k - 2].
template <int DJ> __device__ __forceinline__ float gtg_term(const float* v, int i, int n) {
    const int j = i + DJ;
    if (j < 0 || j >= n) return 0.f;
    if (j == 0) return (DJ == 0 ? -1.f : (DJ == -1 ? 1.f : 0.f)) * (v[3 + DJ] - v[2 + DJ]);
    if (j == n - 1) return (DJ == 0 ? 1.f : (DJ == 1 ? -1.f : 0.f)) * (v[2 + DJ] - v[1 + DJ]);
    return (DJ == -1 ? 0.25f : (DJ == 1 ? -0.25f : 0.f)) * (v[3 + DJ] - v[1 + DJ]);
}
__device__ __forceinline__ float gtg(const float* v, int i, int n) { return gtg_term<-1>(v, i, n) + gtg_term<0>(v, i, n) + gtg_term<1>(v, i, n); }

template <int GRP, int V> __device__ __forceinline__ void bwd_unit(const HeadArgs& a, i64 idx) {
    if constexpr (GRP == G_PROB) {
        const Vec<V> t = ldv<V>(a.target + idx);
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if (l >= a.nlev) break;
            const float c0 = a.coef[l * 4], c1 = a.coef[l * 4 + 1], c2 = a.coef[l * 4 + 2];
            const Vec<V> p = ldv<V>(a.pred[l] + idx);
            Vec<V> g;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float x = p.v[j], y = t.v[j];
                float d = fmaf(c2, y, c1);
                if (a.kind == K_BCEDICE) d += c0 * (x - y) / fmaxf((1.f - x) * x, 1e-12f);      // PyTorch's binary_cross_entropy backward
                g.v[j] = d;
            }
            stv<V>(a.dpred[l] + idx, g);
        }
    } else if constexpr (GRP == G_REG) {
        const Vec<V> t = ldv<V>(a.target + idx);
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if (l >= a.nlev) break;
            const float c0 = a.coef[l * 4];
            const Vec<V> p = ldv<V>(a.pred[l] + idx);
            Vec<V> g;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float e = p.v[j] - t.v[j];
                g.v[j] = c0 * (a.kind == K_MSE ? e : (a.kind == K_MAE ? sgn(e) : (fabsf(e) < a.pa ? e : a.pa * sgn(e))));
            }
            stv<V>(a.dpred[l] + idx, g);
        }
    } else if constexpr (GRP == G_STENCIL) {
        const int W = a.w, H = a.h;
        const int x0 = (int)(idx % W), y = (int)((idx / W) % H);
        Vec<V> tr[5], wr[5];
        bool vr[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            vr[k] = y + k - 2 >= 0 && y + k - 2 < H;
            tr[k] = vr[k] ? ldv<V>(a.target + idx + (i64)(k - 2) * W) : zerov<V>();
#pragma unroll
            for (int j = 0; j < V; ++j) wr[k].v[j] = wof(a, tr[k].v[j]);
        }
        // the two columns on either side of the unit, row y
        const int xs[4] = {x0 - 2, x0 - 1, x0 + V, x0 + V + 1};
        float ts[4], ws[4];
        bool vs[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            vs[k] = xs[k] >= 0 && xs[k] < W;
            ts[k] = vs[k] ? a.target[idx + (xs[k] - x0)] : 0.f;
            ws[k] = wof(a, ts[k]);
        }
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if (l >= a.nlev) break;
            const float c0 = a.coef[l * 4], c1 = a.coef[l * 4 + 1], c2 = a.coef[l * 4 + 2];
            const float* p = a.pred[l];
            Vec<V> e[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const Vec<V> q = vr[k] ? ldv<V>(p + idx + (i64)(k - 2) * W) : zerov<V>();
#pragma unroll
                for (int j = 0; j < V; ++j) e[k].v[j] = wr[k].v[j] * (q.v[j] - tr[k].v[j]);
            }
            float er[V + 4];
#pragma unroll
            for (int k = 0; k < 4; ++k) er[k < 2 ? k : V + k] = vs[k] ? ws[k] * (p[idx + (xs[k] - x0)] - ts[k]) : 0.f;
#pragma unroll
            for (int j = 0; j < V; ++j) er[j + 2] = e[2].v[j];
            Vec<V> g;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float col[5] = {e[0].v[j], e[1].v[j], e[2].v[j], e[3].v[j], e[4].v[j]};
                const float ec = e[2].v[j];
                const float s = gtg(col, y, H) + gtg(er + j, x0 + j, W);
                g.v[j] = wr[2].v[j] * (c0 * ec + c1 * sgn(ec) + c2 * s);
            }
            stv<V>(a.dpred[l] + idx, g);
        }
    } else {
        const i64 hw = (i64)a.h * a.w;
        const i64 o0 = (idx / hw) * 2 * hw + idx % hw, o1 = o0 + hw;
        const Vec<V> t0 = ldv<V>(a.target + o0), t1 = ldv<V>(a.target + o1);
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if (l >= a.nlev) break;
            const float c0 = a.coef[l * 4], c1 = a.coef[l * 4 + 1], c2 = a.coef[l * 4 + 2];
            const Vec<V> p0 = ldv<V>(a.pred[l] + o0), p1 = ldv<V>(a.pred[l] + o1);
            Vec<V> g0, g1;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float w = (t0.v[j] == 0.f && t1.v[j] == 0.f) ? a.pb : a.pa;
                const float u0 = w * (p0.v[j] - t0.v[j]), u1 = w * (p1.v[j] - t1.v[j]);
                const float m = w * (p0.v[j] * p0.v[j] + p1.v[j] * p1.v[j]) - w * (t0.v[j] * t0.v[j] + t1.v[j] * t1.v[j]);
                const float cm = c2 * m * w;
                g0.v[j] = w * (c0 * u0 + c1 * sgn(u0)) + cm * p0.v[j];
                g1.v[j] = w * (c0 * u1 + c1 * sgn(u1)) + cm * p1.v[j];
            }
            stv<V>(a.dpred[l] + o0, g0);
            stv<V>(a.dpred[l] + o1, g1);
        }
    }
}

template <int GRP, int V> __global__ __launch_bounds__(256) void k_mo2d_bwd(const HeadArgs a) {
    const i64 span = GRP == G_VEC ? a.total / 2 : a.total;
    const i64 units = span / V;
    for (i64 u = (i64)blockIdx.x * 256 + threadIdx.x; u < units; u += (i64)gridDim.x * 256) bwd_unit<GRP, V>(a, u * V);
    if constexpr (V == 4 && (GRP == G_PROB || GRP == G_REG)) {
        const i64 done = units * 4;
        if (blockIdx.x == 0 && (i64)threadIdx.x < span - done) bwd_unit<GRP, 1>(a, done + threadIdx.x);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the scalar part: saved = { total, #pred out of range, #target out of range, 0 x 5, then per term { loss, sums[6], 0 } }
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double tversky(const biu_mo2d_term& t, const float* s, double* den) {
    const double tp = s[3], fp = (double)s[1] - tp, fn = (double)s[2] - tp;
    *den = tp + (double)t.p0 * fp + (double)t.p1 * fn + (double)t.p2;
    return (tp + (double)t.p2) / *den;
}
__global__ __launch_bounds__(1024) void k_mo2d_finish(const biu_mo2d_term* __restrict__ terms, int nterms, const float* __restrict__ ws,
                                                     float* __restrict__ saved) {
    // one wave per (term, slot) sum, lanes stride over the per-block partials, fixed-order butterfly in fp64
    for (int idx = threadIdx.x >> 6; idx < nterms * NACC; idx += (int)(blockDim.x >> 6)) {
        const int t = idx / NACC, k = idx % NACC, lane = threadIdx.x & 63;
        const float* part = ws + terms[t].partial_off;
        double s = 0.0;
        for (int b = lane; b < terms[t].nb; b += 64) s += (double)part[(i64)b * NS + k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if (lane == 0) saved[8 + t * 8 + 1 + k] = (float)s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double total = 0.0, op = 0.0, ot = 0.0;
    for (int i = 0; i < nterms; ++i) {
        const biu_mo2d_term t = terms[i];
        const float* s = saved + 8 + i * 8 + 1;
        const double M = (double)t.numel;
        double loss = 0.0, den;
        switch (t.kind) {
            case K_BCEDICE:
                loss = (double)t.p0 * ((double)s[0] / M) + (double)t.p1 * (1.0 - (2.0 * (double)s[3] + 1e-5) / ((double)s[1] + (double)s[2] + 1e-5));
                op += (double)s[4];
                ot += (double)s[5];
                break;
            case K_TVERSKY: loss = 1.0 - tversky(t, s, &den); break;
            case K_LCTVERSKY: loss = log(cosh(1.0 - tversky(t, s, &den))); break;
            case K_MSE: case K_MAE: case K_HUBER: loss = (double)s[0] / M; break;
            case K_DGRAD: loss = (double)s[0] / M + (double)t.p0 * ((double)s[2] / M + (double)s[3] / M); break;
            case K_WDGRAD: loss = (double)s[0] / M + (double)s[1] / M + (double)t.p0 * ((double)s[2] / M + (double)s[3] / M); break;
            default: loss = (double)s[0] / M + (double)s[1] / M + (double)t.p1 * ((double)s[2] / (double)t.pixels); break;
        }
        saved[8 + i * 8] = (float)loss;
        saved[8 + i * 8 + 7] = 0.f;
        total += (double)t.weight * loss;
    }
    saved[0] = (float)total;
    saved[1] = (float)op;
    saved[2] = (float)ot;
    for (int k = 3; k < 8; ++k) saved[k] = 0.f;
}

__global__ __launch_bounds__(64) void k_mo2d_coef(const biu_mo2d_term* __restrict__ terms, int nterms, const float* __restrict__ g,
                                                  const float* __restrict__ saved, float* __restrict__ coef) {
    const int i = threadIdx.x;
    if (i >= nterms) return;
    const biu_mo2d_term t = terms[i];
    const float* s = saved + 8 + i * 8 + 1;
    const double gw = (double)g[0] * (double)t.weight, M = (double)t.numel;
    double c0 = 0.0, c1 = 0.0, c2 = 0.0;
    switch (t.kind) {
        case K_BCEDICE: {
            const double den = (double)s[1] + (double)s[2] + 1e-5;
            c0 = gw * (double)t.p0 / M;
            c1 = gw * (double)t.p1 * (2.0 * (double)s[3] + 1e-5) / (den * den);
            c2 = -gw * (double)t.p1 * 2.0 / den;
            break;
        }
        case K_TVERSKY: case K_LCTVERSKY: {
            double den;
            const double tv = tversky(t, s, &den), tps = (double)s[3] + (double)t.p2;
            const double outer = -gw * (t.kind == K_LCTVERSKY ? tanh(1.0 - tv) : 1.0);         // d loss / d Tversky
            c1 = outer * (-tps * (double)t.p0 / (den * den));
            c2 = outer * (1.0 / den - tps * (1.0 - (double)t.p0 - (double)t.p1) / (den * den));
            break;
        }
        case K_MSE: c0 = 2.0 * gw / M; break;
        case K_MAE: case K_HUBER: c0 = gw / M; break;
        case K_DGRAD: c0 = 2.0 * gw / M; c2 = 2.0 * (double)t.p0 * gw / M; break;
        case K_WDGRAD: c0 = 2.0 * gw / M; c1 = gw / M; c2 = 2.0 * (double)t.p0 * gw / M; break;
        default: c0 = 2.0 * gw / M; c1 = gw / M; c2 = 4.0 * (double)t.p1 * gw / (double)t.pixels; break;
    }
    coef[i * 4] = (float)c0; coef[i * 4 + 1] = (float)c1; coef[i * 4 + 2] = (float)c2; coef[i * 4 + 3] = 0.f;
}

int group_of(int kind) { return kind <= K_LCTVERSKY ? G_PROB : (kind <= K_HUBER ? G_REG : (kind <= K_WDGRAD ? G_STENCIL : G_VEC)); }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// shared argument checks; (ea, eb): what the per-element arithmetic of a kind needs (include/biu.h)
int fill_args(const char* who, HeadArgs& a, int kind, float ea, float eb, const float* const* pred, int nlev, const float* target, int n, int c,
              int h, int w) {
    BIU_REQUIRE(kind >= 0 && kind < K_COUNT, BIU_ERR_UNSUPPORTED, "%s: unknown kind %d", who, kind);
    BIU_REQUIRE(pred && target && nlev >= 1 && nlev <= NL && n > 0 && c > 0 && h > 0 && w > 0, BIU_ERR_SHAPE, "%s: bad arguments", who);
    BIU_REQUIRE(group_of(kind) != G_STENCIL || (h >= 2 && w >= 2), BIU_ERR_SHAPE,
                "%s: torch.gradient expects each dimension size to be at least edge_order+1 (H = %d, W = %d)", who, h, w);
    BIU_REQUIRE(kind != K_WVF || c == 2, BIU_ERR_SHAPE, "%s: the vector-field criterion takes two channels, got %d", who, c);
    for (int l = 0; l < NL; ++l) {
        a.pred[l] = l < nlev ? pred[l] : nullptr;
        a.dpred[l] = nullptr;
        BIU_REQUIRE(l >= nlev || pred[l], BIU_ERR_SHAPE, "%s: prediction %d is null", who, l);
    }
    a.target = target; a.coef = nullptr; a.partial = nullptr;
    a.nlev = nlev; a.kind = kind; a.n = n; a.c = c; a.h = h; a.w = w;
    a.total = (i64)n * c * h * w;
    a.pa = ea;
    a.pb = eb;
    return BIU_OK;
}
// 16-byte accesses where the addresses allow: aligned bases, and rows (stencil) / planes (vector field) that are multiples of four
bool vec4_ok(const HeadArgs& a, bool bwd) {
    bool ok = aligned16(a.target);
    for (int l = 0; l < a.nlev; ++l) ok = ok && aligned16(a.pred[l]) && (!bwd || aligned16(a.dpred[l]));
    const int g = group_of(a.kind);
    if (g == G_STENCIL) ok = ok && a.w % 4 == 0;
    if (g == G_VEC) ok = ok && ((i64)a.h * a.w) % 4 == 0;
    return ok;
}
}  // namespace

#define MO2D_LAUNCH(KERNEL, grid, st, a, v4)                                                                                          \
    do {                                                                                                                              \
        switch (group_of((a).kind) * 2 + ((v4) ? 1 : 0)) {                                                                            \
            case 0: hipLaunchKernelGGL((KERNEL<G_PROB, 1>), dim3(grid), dim3(256), 0, st, a); break;                                  \
            case 1: hipLaunchKernelGGL((KERNEL<G_PROB, 4>), dim3(grid), dim3(256), 0, st, a); break;                                  \
            case 2: hipLaunchKernelGGL((KERNEL<G_REG, 1>), dim3(grid), dim3(256), 0, st, a); break;                                   \
            case 3: hipLaunchKernelGGL((KERNEL<G_REG, 4>), dim3(grid), dim3(256), 0, st, a); break;                                   \
            case 4: hipLaunchKernelGGL((KERNEL<G_STENCIL, 1>), dim3(grid), dim3(256), 0, st, a); break;                               \
            case 5: hipLaunchKernelGGL((KERNEL<G_STENCIL, 4>), dim3(grid), dim3(256), 0, st, a); break;                               \
            case 6: hipLaunchKernelGGL((KERNEL<G_VEC, 1>), dim3(grid), dim3(256), 0, st, a); break;                                   \
            default: hipLaunchKernelGGL((KERNEL<G_VEC, 4>), dim3(grid), dim3(256), 0, st, a); break;                                  \
        }                                                                                                                             \
    } while (0)

extern "C" int biu_mo2d_loss_blocks(long long numel) {
    long long b = (numel + 1023) / 1024;
    return (int)(b < 1 ? 1 : (b > 256 ? 256 : b));
}

extern "C" int biu_mo2d_loss_fwd(int kind, float ea, float eb, const float* const* pred, int nlev, const float* target, int n, int c, int h,
                                 int w, float* partial, biu_stream stream) {
    HeadArgs a;
    const int rc = fill_args("mo2d_loss_fwd", a, kind, ea, eb, pred, nlev, target, n, c, h, w);
    if (rc != BIU_OK) return rc;
    BIU_REQUIRE(partial, BIU_ERR_SHAPE, "mo2d_loss_fwd: no partial buffer");
    a.partial = partial;
    const int grid = biu_mo2d_loss_blocks(a.total);
    MO2D_LAUNCH(k_mo2d_fwd, grid, (hipStream_t)stream, a, vec4_ok(a, false));
    BIU_CHECK_LAUNCH("mo2d_loss_fwd");
    return BIU_OK;
}

extern "C" int biu_mo2d_loss_bwd(int kind, float ea, float eb, const float* const* pred, int nlev, const float* target, int n, int c, int h,
                                 int w, const float* coef, float* const* dpred, biu_stream stream) {
    HeadArgs a;
    const int rc = fill_args("mo2d_loss_bwd", a, kind, ea, eb, pred, nlev, target, n, c, h, w);
    if (rc != BIU_OK) return rc;
    BIU_REQUIRE(coef && dpred, BIU_ERR_SHAPE, "mo2d_loss_bwd: bad arguments");
    for (int l = 0; l < nlev; ++l) {
        BIU_REQUIRE(dpred[l], BIU_ERR_SHAPE, "mo2d_loss_bwd: gradient %d is null", l);
        a.dpred[l] = dpred[l];
    }
    a.coef = coef;
    const int grid = grid_for(a.total, 1024, 1024);
    MO2D_LAUNCH(k_mo2d_bwd, grid, (hipStream_t)stream, a, vec4_ok(a, true));
    BIU_CHECK_LAUNCH("mo2d_loss_bwd");
    return BIU_OK;
}

extern "C" int biu_mo2d_loss_finish(const biu_mo2d_term* terms, int nterms, const float* workspace, float* saved, biu_stream stream) {
    BIU_REQUIRE(terms && workspace && saved && nterms >= 1 && nterms <= BIU_MO2D_MAX_TERMS, BIU_ERR_SHAPE, "mo2d_loss_finish: bad arguments");
    hipLaunchKernelGGL(k_mo2d_finish, dim3(1), dim3(nterms * NACC > 16 ? 1024 : 256), 0, (hipStream_t)stream, terms, nterms, workspace, saved);
    BIU_CHECK_LAUNCH("mo2d_loss_finish");
    return BIU_OK;
}

extern "C" int biu_mo2d_loss_coef(const biu_mo2d_term* terms, int nterms, const float* g, const float* saved, float* coef, biu_stream stream) {
    BIU_REQUIRE(terms && g && saved && coef && nterms >= 1 && nterms <= BIU_MO2D_MAX_TERMS, BIU_ERR_SHAPE, "mo2d_loss_coef: bad arguments");
    hipLaunchKernelGGL(k_mo2d_coef, dim3(1), dim3(64), 0, (hipStream_t)stream, terms, nterms, g, saved, coef);
    BIU_CHECK_LAUNCH("mo2d_loss_coef");
    return BIU_OK;
}
