// The front of the Predict pipelines on the device: the percentile clip and rescale every reference Predict runs in numpy before it
// tiles (unet/predict.py:122-181, unet3d/predict.py:97-150, siam_unet/predict.py:98-170, multi_output_unet/predict.py:129-181,
// multi_output_unet3d/predict.py:99-160), restated as three stages that never leave the stream:
//
//   biu_order_stats   exact order statistics by radix select: an order-preserving 32-bit key (integers widened; float32 with the sign
//                     flip, so negatives, -0.0 < +0.0 and denormals sort as IEEE orders them, NaN after everything like np.sort), one
//                     8-bit digit per pass from the top.  A pass is a histogram kernel (LDS bins, integer LDS atomics, flushed with
//                     integer global atomics: integer sums do not depend on arrival order, so the result is deterministic -- there
//                     is no float atomic in this file) and a pick kernel that scans the bins for every (segment, rank) and leaves the
//                     narrowed prefix and the remaining rank in device memory for the next pass.  No host round trip between passes.
//   biu_prep_finalize numpy's linear percentile on the selected neighbours and the scalars of each family's formula, fp64.
//   biu_prep_tiles    clip, rescale and tile gather fused: reads the raw stack, writes the patch batch the network reads.
//
// Arithmetic on pixel values is fp64 in the host's operation order with one rounding per operation.  hipcc contracts a + b * c into an
// FMA by default, which changes the last bit of the percentile (x_k + d * g) and of the inverted output (top - a * top), so
// contraction is switched off for this whole file:
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "biu_common.h"
#include "biu_internal.h"

namespace {
constexpr int TPB = 256;
constexpr int MAXR = 8;          // ranks per segment
constexpr int BINS = 256;        // 8-bit digits: 8 KB of LDS for the 8 prefix groups of a pass
static_assert(BINS == TPB, "the pass-0 flush takes one digit per thread");

template <int E> struct ElemOf;
template <> struct ElemOf<BIU_ELEM_U8> { typedef uint8_t type; static constexpr int bits = 8; };
template <> struct ElemOf<BIU_ELEM_U16> { typedef uint16_t type; static constexpr int bits = 16; };
template <> struct ElemOf<BIU_ELEM_I16> { typedef int16_t type; static constexpr int bits = 16; };
template <> struct ElemOf<BIU_ELEM_F32> { typedef uint32_t type; static constexpr int bits = 32; };      // raw bits

__host__ __device__ inline int key_bits(int elem) { return elem == BIU_ELEM_U8 ? 8 : (elem == BIU_ELEM_F32 ? 32 : 16); }
__host__ __device__ inline int elem_bytes(int elem) { return elem == BIU_ELEM_U8 ? 1 : (elem == BIU_ELEM_F32 ? 4 : 2); }

__device__ inline bool f32_is_nan(uint32_t b) { return (b & 0x7fffffffu) > 0x7f800000u; }

template <int E>
__device__ inline uint32_t key_of(typename ElemOf<E>::type v) {
    if constexpr (E == BIU_ELEM_I16) return (uint32_t)((int)v + 32768);
    else if constexpr (E == BIU_ELEM_F32) return f32_is_nan(v) ? 0xffffffffu : ((v & 0x80000000u) ? ~v : (v | 0x80000000u));
    else return (uint32_t)v;
}
__device__ inline double value_of_key(int elem, uint32_t key) {
    if (elem == BIU_ELEM_I16) return (double)((int)key - 32768);
    if (elem == BIU_ELEM_F32) return (double)__uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
    return (double)key;
}

// Selection state in the caller's workspace.  hist: [S][R][BINS] (group g of a segment uses row g); the rest: [S][R] / [S].
struct SelState {
    uint32_t* hist;
    unsigned long long* rem;     // rank still to go inside the prefix
    uint32_t* prefix;            // key digits fixed so far, per (segment, rank)
    uint32_t* group;             // rank -> histogram row of its prefix (ranks sharing a prefix share a row)
    uint32_t* gprefix;           // row -> prefix
    uint32_t* ngroups;           // rows in use, per segment
};

// One pass' histogram: grid (blocks per segment, S).  Pass 0 has one row (no prefix yet), kept in eight interleaved copies (lane & 7) because
// the top digit of an image is the same for most of a wave; later passes one row per distinct prefix.
// 16-byte loads over the aligned body of the segment, block 0 takes the (< 16 element) head and tail one element per thread.
template <int E>
__global__ __launch_bounds__(TPB) void k_sel_hist(const unsigned char* __restrict__ x, i64 n, i64 stride, int R, int pass, int shift,
                                                  SelState st, unsigned long long* __restrict__ nan_count) {
    typedef typename ElemOf<E>::type T;
    constexpr int PER = 16 / (int)sizeof(T);
    __shared__ uint32_t lh[MAXR * BINS];
    __shared__ uint32_t lp[MAXR];
    __shared__ uint32_t lnan;
    const int tid = threadIdx.x, s = blockIdx.y;
    const int G = pass == 0 ? 1 : min((int)st.ngroups[s], R);
    for (int i = tid; i < (pass == 0 ? MAXR : G) * BINS; i += TPB) lh[i] = 0;
    if (tid < G) lp[tid] = pass == 0 ? 0u : st.gprefix[(i64)s * R + tid];
    if (tid == 0) lnan = 0;
    __syncthreads();

    const T* seg = (const T*)x + (i64)s * stride;
    i64 head = (i64)((16 - ((uintptr_t)seg & 15)) & 15) / (i64)sizeof(T);
    if (head > n) head = n;
    const i64 nv = (n - head) / PER;
    const i64 tail0 = head + nv * PER;
    uint32_t nans = 0;
    // Neighbouring pixels of an image mostly share their upper digits: a thread merges a run of elements that fall into the same bin into
    // one LDS atomic (same-address atomics of a wave serialise, so the top-digit pass of a smooth image is bound by them otherwise).
    constexpr uint32_t NONE = 0xffffffffu;
    uint32_t run_bin = NONE, run_len = 0;
    uint32_t pf[MAXR];                                       // the prefixes in registers (block-uniform): a compare per slot and element
#pragma unroll
    for (int k = 0; k < MAXR; ++k) pf[k] = k < G ? lp[k] : NONE;
    auto flush = [&]() {
        if (run_bin != NONE) atomicAdd(&lh[run_bin], run_len);
    };
    auto put = [&](T v) {
        if constexpr (E == BIU_ELEM_F32) nans += f32_is_nan(v) ? 1u : 0u;
        const uint32_t key = key_of<E>(v);
        uint32_t bin = (key >> shift) & (BINS - 1);
        if (pass == 0) {
            bin = bin * MAXR + (tid & (MAXR - 1));           // eight copies of the one row, a digit's copies in neighbouring banks
        } else {
            const uint32_t hi = key >> (shift + 8);          // < 2^24: never equals an unused slot
            int g = -1;
#pragma unroll
            for (int k = 0; k < MAXR; ++k) g = pf[k] == hi ? k : g;
            bin = g >= 0 ? g * BINS + bin : NONE;            // outside every prefix still in play: counted nowhere
        }
        if (bin == run_bin) { ++run_len; return; }
        flush();
        run_bin = bin;
        run_len = 1;
    };
    const uint4* body = (const uint4*)(seg + head);
    for (i64 v = (i64)blockIdx.x * TPB + tid; v < nv; v += (i64)gridDim.x * TPB) {
        union { uint4 q; T e[PER]; } u;
        u.q = body[v];
#pragma unroll
        for (int j = 0; j < PER; ++j) put(u.e[j]);
    }
    if (blockIdx.x == 0) {
        if (tid < head) put(seg[tid]);
        if (tail0 + tid < n) put(seg[tail0 + tid]);
    }
    flush();
    if (E == BIU_ELEM_F32 && pass == 0 && nans) atomicAdd(&lnan, nans);
    __syncthreads();
    uint32_t* gh = st.hist + (i64)s * R * BINS;
    if (pass == 0) {
        uint32_t c = 0;                                      // TPB == BINS: one digit per thread
        for (int k = 0; k < MAXR; ++k) c += lh[tid * MAXR + k];
        if (c) atomicAdd(&gh[tid], c);
    } else {
        for (int i = tid; i < G * BINS; i += TPB)
            if (lh[i]) atomicAdd(&gh[i], lh[i]);
    }
    if (E == BIU_ELEM_F32 && pass == 0 && tid == 0 && lnan) atomicAdd(nan_count, (unsigned long long)lnan);
}

struct Ranks { unsigned long long r[MAXR]; };

// One wave per segment.  For every rank: each lane takes four bins of the rank's histogram row, a wave scan finds the lane and then the bin
// that holds the rank (a serial walk over 256 bins in global memory costs a load latency per bin); the digit goes onto the prefix, what is
// left of the rank is kept.  Then lane 0 either regroups the prefixes for the next pass or, after the last digit, turns the complete keys
// back into values, and the wave clears the segment's rows for the next pass.
__global__ __launch_bounds__(64) void k_sel_pick(int R, int pass, int last, int elem, Ranks ranks, SelState st, double* __restrict__ out) {
    __shared__ uint32_t sp[MAXR];
    const int s = blockIdx.x, lane = threadIdx.x;
    const i64 base = (i64)s * R;
    for (int r = 0; r < R; ++r) {
        const uint32_t g = pass == 0 ? 0u : st.group[base + r];
        const unsigned long long rem = pass == 0 ? ranks.r[r] : st.rem[base + r];
        const uint4 c = ((const uint4*)(st.hist + (base + g) * BINS))[lane];
        const unsigned long long mine = (unsigned long long)c.x + c.y + c.z + c.w;
        unsigned long long inc = mine;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long t = __shfl_up(inc, d, 64);
            if (lane >= d) inc += t;
        }
        unsigned long long cum = inc - mine;
        const bool here = cum <= rem && rem < inc;
        const bool any = __ballot(here) != 0ull;                       // (a rank beyond the counted elements cannot happen: last bin then)
        if (here || (!any && lane == 63)) {
            uint32_t b = 4 * lane;
            if (rem >= cum + c.x) { cum += c.x; ++b;
                if (rem >= cum + c.y) { cum += c.y; ++b;
                    if (rem >= cum + c.z) { cum += c.z; ++b; } } }
            const uint32_t p = pass == 0 ? b : ((st.prefix[base + r] << 8) | b);
            st.rem[base + r] = rem - cum;
            st.prefix[base + r] = p;
            sp[r] = p;
        }
    }
    __syncthreads();
    for (int r = 0; r < R; ++r) ((uint4*)(st.hist + (base + r) * BINS))[lane] = make_uint4(0, 0, 0, 0);
    if (lane != 0) return;
    if (last) {
        for (int r = 0; r < R; ++r) out[base + r] = value_of_key(elem, sp[r]);
        return;
    }
    uint32_t ng = 0;
    for (int r = 0; r < R; ++r) {
        uint32_t g = 0;
        while (g < ng && st.gprefix[base + g] != sp[r]) ++g;
        if (g == ng) st.gprefix[base + ng++] = sp[r];
        st.group[base + r] = g;
    }
    st.ngroups[s] = ng;
}

// np.percentile(..., method='linear') of a sorted sample from its two neighbours: vi = q/100 * (n - 1), k = floor(vi), g = vi - k,
// x_k + (x_k1 - x_k) * g, and from the other end when g >= 0.5 (numpy's _lerp).  The caller selected x_k1 = x_k when vi >= n - 1.
__device__ inline double pct_linear(double xk, double xk1, double q, i64 n) {
    const double vi = (double)(n - 1) * (q / 100.0);
    const double g = vi - floor(vi);
    const double d = xk1 - xk;
    return g >= 0.5 ? xk1 - d * (1.0 - g) : xk + d * g;
}
__device__ inline double clipd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }      // np.clip: minimum(maximum(v, lo), hi)

// stats [U][6]: minimum, maximum, x_k and x_k+1 of the lower percentile, x_k and x_k+1 of the upper.  scalars [U][4]: lo, hi, sub, den
// with out = (clip(v, lo, hi) - sub) / den.
__global__ void k_prep_finalize(const double* __restrict__ stats, int U, i64 n, double q_lo, double q_hi, int family,
                                double* __restrict__ scal) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= U) return;
    const double* t = stats + (i64)u * 6;
    const double lo = pct_linear(t[2], t[3], q_lo, n), hi = pct_linear(t[4], t[5], q_hi, n);
    const double cmin = clipd(t[0], lo, hi);                 // min(clip(a)) = clip(min(a)): clip is monotone
    const double crange = clipd(t[1], lo, hi) - cmin;        // max(clip(a) - cmin)  = clip(max(a)) - cmin: so is a rounded subtraction
    double sub, den;
    if (family == BIU_PREP_MINMAX) { sub = cmin; den = crange; }
    else if (family == BIU_PREP_MINMAX_EPS) { sub = cmin; den = crange + 1e-8; }
    else { sub = lo; den = (hi - lo) + 1e-8; }
    double* o = scal + (i64)u * 4;
    o[0] = lo; o[1] = hi; o[2] = sub; o[3] = den;
}

struct TileGeo {
    int Z, D, H, W;          // planes in the source, planes per volume (z reflects inside its own volume), plane extent
    int td, th, tw;          // tile extent
    int N, U;                // tiles, units
    int pad_zero, out_f32, invert;
};
// numpy 'reflect' (no edge repeat): period 2 (n - 1), folded as often as it takes; n = 1 -> 0
__device__ inline int reflect_idx(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}
template <int E>
__device__ inline double load_px(const void* src, i64 off) {
    if constexpr (E == BIU_ELEM_F32) return (double)((const float*)src)[off];
    else return (double)((const typename ElemOf<E>::type*)src)[off];
}
// One thread per 16 output bytes along x (16 uint8 or 4 float32 pixels): one 16-byte store where the row allows it, element stores for a
// narrow last chunk or rows that do not keep the alignment.
template <int E, typename O>
__global__ __launch_bounds__(TPB) void k_prep_tiles(const void* __restrict__ src, const int* __restrict__ origins,
                                                    const double* __restrict__ scal, TileGeo g, O* __restrict__ out) {
    constexpr int CH = 16 / (int)sizeof(O);
    const int chunks = (g.tw + CH - 1) / CH;
    const i64 rows = (i64)g.N * g.td * g.th;
    const i64 total = rows * chunks;
    const bool vec_ok = g.tw % CH == 0 && ((uintptr_t)out & 15) == 0;
    for (i64 i = (i64)blockIdx.x * TPB + threadIdx.x; i < total; i += (i64)gridDim.x * TPB) {
        const int c = (int)(i % chunks);
        const i64 row = i / chunks;
        const int y = (int)(row % g.th);
        const int z = (int)((row / g.th) % g.td);
        const int t = (int)(row / ((i64)g.th * g.td));
        const int unit = origins[t * 4 + 0], z0 = origins[t * 4 + 1], y0 = origins[t * 4 + 2], x0 = origins[t * 4 + 3];
        const int x_beg = c * CH, cnt = min(CH, g.tw - x_beg);
        O vals[CH];
        bool live = unit >= 0 && unit < g.U && z0 >= 0 && z0 < g.Z && y0 >= 0 && x0 >= 0 && y0 < (1 << 30) && x0 < (1 << 30);   // else zeros
        int sz = 0, sy = 0;
        if (live) {
            const int vbase = z0 / g.D * g.D, zl = z0 - vbase + z, yy = y0 + y;
            if (g.pad_zero) live = zl < g.D && yy < g.H;
            sz = vbase + (g.pad_zero ? zl : reflect_idx(zl, g.D));
            sy = g.pad_zero ? yy : reflect_idx(yy, g.H);
        }
        double lo = 0, hi = 0, sub = 0, den = 1;
        if (live) { const double* q = scal + (i64)unit * 4; lo = q[0]; hi = q[1]; sub = q[2]; den = q[3]; }
        const i64 rowoff = ((i64)sz * g.H + sy) * g.W;
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int xx = x0 + x_beg + j;
            O o = (O)0;
            if (live && j < cnt && !(g.pad_zero && xx >= g.W)) {
                const int sx = g.pad_zero ? xx : reflect_idx(xx, g.W);
                double a = clipd(load_px<E>(src, rowoff + sx), lo, hi);
                a = a - sub;
                a = a / den;
                if constexpr (sizeof(O) == 1) {
                    a = a * 255.0;
                    if (g.invert) a = 255.0 - a;
                    o = (O)(int)a;                           // astype('uint8') of a value in [0, 255]: truncation
                } else {
                    o = (O)a;                                // the one rounding to float32
                }
            }
            vals[j] = o;
        }
        O* dst = out + row * g.tw + x_beg;
        if (vec_ok) {
            union { uint4 q; O e[CH]; } u;
#pragma unroll
            for (int j = 0; j < CH; ++j) u.e[j] = vals[j];
            *(uint4*)dst = u.q;
        } else {
#pragma unroll
            for (int j = 0; j < CH; ++j)
                if (j < cnt) dst[j] = vals[j];
        }
    }
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline bool valid_elem(int e) { return e == BIU_ELEM_U8 || e == BIU_ELEM_U16 || e == BIU_ELEM_I16 || e == BIU_ELEM_F32; }
}  // namespace

extern "C" size_t biu_order_stats_workspace(long long segments, int nranks) {
    if (segments < 1 || nranks < 1 || nranks > MAXR) return 0;
    const size_t sr = (size_t)segments * nranks;
    return align256(sr * BINS * 4) + align256(sr * 8) + 3 * align256(sr * 4) + align256((size_t)segments * 4) + 256;
}

extern "C" int biu_order_stats(const void* x, int elem, long long segments, long long n, long long stride, const long long* ranks, int nranks,
                               double* out, long long* nan_count, void* workspace, size_t workspace_bytes, biu_stream stream) {
    BIU_REQUIRE(x && ranks && out && nan_count && workspace, BIU_ERR_SHAPE, "order_stats: null argument");
    BIU_REQUIRE(valid_elem(elem), BIU_ERR_UNSUPPORTED, "order_stats: element type %d is not uint8, uint16, int16 or float32", elem);
    BIU_REQUIRE(segments >= 1 && segments <= 65535 && n >= 1 && n <= (1LL << 31) && stride >= 0 && nranks >= 1 && nranks <= MAXR, BIU_ERR_SHAPE,
                "order_stats: need 1 <= segments <= 65535, 1 <= n <= 2^31, stride >= 0, 1 <= ranks <= %d", MAXR);
    BIU_REQUIRE(((uintptr_t)x % elem_bytes(elem)) == 0 && ((uintptr_t)workspace & 255) == 0, BIU_ERR_ALIGN, "order_stats: misaligned pointer");
    BIU_REQUIRE(workspace_bytes >= biu_order_stats_workspace(segments, nranks), BIU_ERR_WORKSPACE, "order_stats: workspace too small");
    Ranks rk{};
    for (int r = 0; r < nranks; ++r) {
        BIU_REQUIRE(ranks[r] >= 0 && ranks[r] < n, BIU_ERR_SHAPE, "order_stats: rank %lld outside [0, %lld)", ranks[r], n);
        rk.r[r] = (unsigned long long)ranks[r];
    }
    const int S = (int)segments, R = nranks;
    const size_t sr = (size_t)S * R;
    unsigned char* w = (unsigned char*)workspace;
    SelState st;
    st.hist = (uint32_t*)w;             w += align256(sr * BINS * 4);
    st.rem = (unsigned long long*)w;    w += align256(sr * 8);
    st.prefix = (uint32_t*)w;           w += align256(sr * 4);
    st.group = (uint32_t*)w;            w += align256(sr * 4);
    st.gprefix = (uint32_t*)w;          w += align256(sr * 4);
    st.ngroups = (uint32_t*)w;
    hipStream_t hs = (hipStream_t)stream;
    if (hipMemsetAsync(nan_count, 0, sizeof(long long), hs) != hipSuccess || hipMemsetAsync(st.hist, 0, sr * BINS * 4, hs) != hipSuccess)
        return biu_fail(BIU_ERR_LAUNCH, "order_stats: memset failed");               // (the pick kernel clears the bins between passes)
    const int per = 16 / elem_bytes(elem);
    i64 bps = (n / per + (i64)TPB * 4 - 1) / ((i64)TPB * 4);              // about four vectors per thread
    const i64 cap = 2048 / S > 1 ? 2048 / S : 1;
    bps = bps < 1 ? 1 : (bps > cap ? cap : bps);
    const int passes = key_bits(elem) / 8;
    for (int p = 0; p < passes; ++p) {
        const int shift = key_bits(elem) - 8 * (p + 1);
        const dim3 grid((unsigned)bps, (unsigned)S);
        unsigned long long* nc = (unsigned long long*)nan_count;
        const unsigned char* xb = (const unsigned char*)x;
        switch (elem) {
            case BIU_ELEM_U8: hipLaunchKernelGGL(k_sel_hist<BIU_ELEM_U8>, grid, dim3(TPB), 0, hs, xb, (i64)n, (i64)stride, R, p, shift, st, nc); break;
            case BIU_ELEM_U16: hipLaunchKernelGGL(k_sel_hist<BIU_ELEM_U16>, grid, dim3(TPB), 0, hs, xb, (i64)n, (i64)stride, R, p, shift, st, nc); break;
            case BIU_ELEM_I16: hipLaunchKernelGGL(k_sel_hist<BIU_ELEM_I16>, grid, dim3(TPB), 0, hs, xb, (i64)n, (i64)stride, R, p, shift, st, nc); break;
            default: hipLaunchKernelGGL(k_sel_hist<BIU_ELEM_F32>, grid, dim3(TPB), 0, hs, xb, (i64)n, (i64)stride, R, p, shift, st, nc); break;
        }
        BIU_CHECK_LAUNCH("order_stats histogram");
        hipLaunchKernelGGL(k_sel_pick, dim3(S), dim3(64), 0, hs, R, p, (int)(p == passes - 1), elem, rk, st, out);
        BIU_CHECK_LAUNCH("order_stats pick");
    }
    return BIU_OK;
}

extern "C" int biu_prep_finalize(const double* stats, int units, long long n, double q_lo, double q_hi, int family, double* scalars,
                                 biu_stream stream) {
    BIU_REQUIRE(stats && scalars && units >= 1 && n >= 1, BIU_ERR_SHAPE, "prep_finalize: bad arguments");
    BIU_REQUIRE(q_lo >= 0. && q_lo <= 100. && q_hi >= 0. && q_hi <= 100., BIU_ERR_SHAPE, "prep_finalize: percentiles must be in [0, 100]");
    BIU_REQUIRE(family == BIU_PREP_MINMAX || family == BIU_PREP_MINMAX_EPS || family == BIU_PREP_LOHI_EPS, BIU_ERR_UNSUPPORTED,
                "prep_finalize: unknown family %d", family);
    hipLaunchKernelGGL(k_prep_finalize, dim3((units + 63) / 64), dim3(64), 0, (hipStream_t)stream, stats, units, (i64)n, q_lo, q_hi, family, scalars);
    BIU_CHECK_LAUNCH("prep_finalize");
    return BIU_OK;
}

extern "C" int biu_prep_tiles(const void* src, int elem, int planes, int depth, int height, int width, const int* origins, int ntiles, int td,
                              int th, int tw, const double* scalars, int units, int pad_zero, int out_f32, int invert, void* out,
                              biu_stream stream) {
    BIU_REQUIRE(src && origins && scalars && out, BIU_ERR_SHAPE, "prep_tiles: null argument");
    BIU_REQUIRE(valid_elem(elem), BIU_ERR_UNSUPPORTED, "prep_tiles: element type %d is not uint8, uint16, int16 or float32", elem);
    BIU_REQUIRE(planes >= 1 && depth >= 1 && planes % depth == 0 && height >= 1 && width >= 1 && ntiles >= 1 && td >= 1 && th >= 1 && tw >= 1 &&
                    td <= (1 << 24) && th <= (1 << 24) && tw <= (1 << 24) && units >= 1, BIU_ERR_SHAPE, "prep_tiles: bad extents");
    BIU_REQUIRE((long long)ntiles * 4 <= 0x7fffffffLL && (long long)planes * height * width > 0, BIU_ERR_SHAPE, "prep_tiles: too many tiles");
    BIU_REQUIRE(((uintptr_t)src % elem_bytes(elem)) == 0 && ((uintptr_t)out & (out_f32 ? 3 : 0)) == 0, BIU_ERR_ALIGN, "prep_tiles: misaligned pointer");
    const TileGeo g{planes, depth, height, width, td, th, tw, ntiles, units, pad_zero ? 1 : 0, out_f32 ? 1 : 0, invert ? 1 : 0};
    const int ch = out_f32 ? 4 : 16;
    const int grid = grid_for((i64)ntiles * td * th * ((tw + ch - 1) / ch), TPB, 8192);
    hipStream_t hs = (hipStream_t)stream;
#define BIU_PREP_LAUNCH(E)                                                                                                             \
    do {                                                                                                                               \
        if (out_f32) hipLaunchKernelGGL((k_prep_tiles<E, float>), dim3(grid), dim3(TPB), 0, hs, src, origins, scalars, g, (float*)out); \
        else hipLaunchKernelGGL((k_prep_tiles<E, uint8_t>), dim3(grid), dim3(TPB), 0, hs, src, origins, scalars, g, (uint8_t*)out);    \
    } while (0)
    switch (elem) {
        case BIU_ELEM_U8: BIU_PREP_LAUNCH(BIU_ELEM_U8); break;
        case BIU_ELEM_U16: BIU_PREP_LAUNCH(BIU_ELEM_U16); break;
        case BIU_ELEM_I16: BIU_PREP_LAUNCH(BIU_ELEM_I16); break;
        default: BIU_PREP_LAUNCH(BIU_ELEM_F32); break;
    }
#undef BIU_PREP_LAUNCH
    BIU_CHECK_LAUNCH("prep_tiles");
    return BIU_OK;
}
