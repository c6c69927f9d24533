// Cubic-spline resampling of rotated scalar targets (MASK fields) of the 2-D multi-output family: what the reference computes with
// scipy.ndimage.rotate(order=3, mode='grid-wrap') and then clips back into the target's own range (multi_output_unet/data.py:213-242).
// The sibling of biu_augment_f32.hip, which gathers these fields bilinearly; same records (biu_augf_params), same fp64 map, indices WRAP.
// The contract is in include/biu.h.  Three launches per field, all of them skipped by samples whose record has no BIU_AUGF_ROT:
//
//   k_spline_range     : one block of 1024 lanes per sample: lo = min, hi = max of the loaded values over all planes (a block reduction: no
//                        atomics, nothing to clear first, the result does not depend on any order); 16-byte loads where the field allows
//   k_spline_prefilter : one block per 64 x 64 tile of one (sample, plane).  With 'grid-wrap' scipy's cubic prefilter is the cyclic convolution
//                        c[k] = sum_j sqrt(3) z^|j| s[(k - j) mod n], z = sqrt(3) - 2, separable; |z|^j decays geometrically, so the sum is cut
//                        at |j| <= R = BIU_SPLINE_R and becomes tile-local: tile + halo of R into LDS through the wrap (which may go round a
//                        small field several times), 2R + 1 taps along x, then along y, symmetric taps added before the multiply, from the
//                        outermost inwards (smallest terms first).
//   k_spline_gather    : k_augf_point's structure (a lane owns 4 consecutive pixels of a row, one 16-byte store).  Rotating samples: fp64
//                        coordinate and fraction, four cubic B-spline weights per axis evaluated in fp64 and rounded once to fp32, 4 x 4
//                        coefficients summed in fp32 (rows first), then the clip.  Other samples: biu_augment_f32's nearest gather from src.
// No atomics, no scratch.
#include <hip/hip_runtime.h>

#include "biu_common.h"
#include "biu_augment_stages.h"

namespace {
using biu_augment_stages::overlap;
using biu_augment_stages::source_of;
using biu_augment_stages::wrap;

constexpr int TPB = 256;
constexpr int RANGE_TPB = 1024;                 // the range kernel's one block per sample
constexpr int GROUP = 4;                        // pixels per lane: one 16-byte store
constexpr int TILE = 64;                        // the prefilter's output tile is TILE x TILE
constexpr int R = BIU_SPLINE_R;                 // taps |j| <= R per axis
constexpr int IN = TILE + 2 * R;                // 96 rows / columns of loaded source; a row is 384 B, 16-byte aligned

// sqrt(3) z^d, d = 0 .. 16, z = sqrt(3) - 2: the fp64 values rounded once (signs alternate)
__constant__ float TAPS[R + 1] = {1.7320507764816284f, -0.4641016125679016f, 0.12435565143823624f, -0.03332099691033363f, 0.008928334340453148f,
                                  -0.002392339985817671f, 0.0006410255446098745f, -0.0001717622799333185f, 4.6023564209463075e-05f, -1.2331976904533803e-05f,
                                  3.3043431812984636e-06f, -8.853961048771453e-07f, 2.3724116715584387e-07f, -6.356857795708493e-08f, 1.7033150001566355e-08f,
                                  -4.564018496466815e-09f, 1.22292509452393e-09f};
static_assert(R == 16, "TAPS holds sqrt(3) z^d for d = 0 .. 16");

struct Launch {
    const void* src;
    const float* coef;         // gather: the prefilter's output
    const float* range;        // gather: [n][2]
    float* dst;                // range: [n][2]; prefilter: coef; gather: the augmented field
    const biu_augf_params* params;
    int u8;                    // src holds bytes
    int n, planes, h, w;
};

__device__ __forceinline__ float load(const Launch& L, int i) {
    return L.u8 ? (float)static_cast<const uint8_t*>(L.src)[i] / 255.0f : static_cast<const float*>(L.src)[i];
}

// grid = n; one block of RANGE_TPB lanes walks the sample's field, 16 bytes per lane and step where the field allows it (a single block has
// only its own loads in flight to hide the memory latency with)
__global__ __launch_bounds__(RANGE_TPB) void k_spline_range(Launch L, int vec) {
    __shared__ float s_lo[RANGE_TPB / 64], s_hi[RANGE_TPB / 64];
    const int s = blockIdx.x, field = L.planes * L.h * L.w;
    if (!(L.params[s].flags & BIU_AUGF_ROT)) return;
    float lo = INFINITY, hi = -INFINITY;                       // fminf / fmaxf pass a NaN by: "NaN aside"
    if (vec) {                                                 // field % 16 == 0 (bytes) or % 4 == 0 (floats), src 16-byte aligned
        const int per = L.u8 ? 16 : 4, groups = field / per;
        const uint4* q = reinterpret_cast<const uint4*>(static_cast<const char*>(L.src) + (size_t)s * field * (L.u8 ? 1 : 4));
#pragma unroll 4
        for (int i = threadIdx.x; i < groups; i += RANGE_TPB) {
            const uint4 v = q[i];
            const uint32_t word[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (L.u8) {                                    // min and max of the bytes; widened once at the end (the widening is monotonic)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float f = (float)((word[j] >> (8 * k)) & 255u);
                        lo = fminf(lo, f);
                        hi = fmaxf(hi, f);
                    }
                } else {
                    lo = fminf(lo, __uint_as_float(word[j]));
                    hi = fmaxf(hi, __uint_as_float(word[j]));
                }
            }
        }
        if (L.u8) {
            lo /= 255.0f;
            hi /= 255.0f;
        }
    } else {
#pragma unroll 4
        for (int i = threadIdx.x; i < field; i += RANGE_TPB) {
            const float v = load(L, s * field + i);
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_down(lo, o, 64));
        hi = fmaxf(hi, __shfl_down(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        s_lo[threadIdx.x >> 6] = lo;
        s_hi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < RANGE_TPB / 64; ++i) {
            lo = fminf(lo, s_lo[i]);
            hi = fmaxf(hi, s_hi[i]);
        }
        L.dst[2 * s] = lo;
        L.dst[2 * s + 1] = hi;
    }
}

// grid = n * planes * tiles_y * tiles_x
__global__ __launch_bounds__(TPB) void k_spline_prefilter(Launch L, int tiles_x, int tiles_y) {
    __shared__ __attribute__((aligned(16))) float s_in[IN * IN];             // 36 864 B
    __shared__ __attribute__((aligned(16))) float s_h[IN * TILE];            // 24 576 B
    int b = blockIdx.x;
    const int tx0 = (b % tiles_x) * TILE;
    b /= tiles_x;
    const int ty0 = (b % tiles_y) * TILE;
    b /= tiles_y;
    const int p = b % L.planes, s = b / L.planes;
    if (!(L.params[s].flags & BIU_AUGF_ROT)) return;
    const int hw = L.h * L.w, base = (s * L.planes + p) * hw;
    // 1. tile + halo; the index wraps as often as the field is smaller than the halo
    for (int i = threadIdx.x; i < IN * IN; i += TPB) {
        const int ly = i / IN, lx = i - ly * IN;
        s_in[i] = load(L, base + wrap(ty0 - R + ly, L.h) * L.w + wrap(tx0 - R + lx, L.w));
    }
    __syncthreads();
    // 2. along x; a wave covers one row of 64 sums, its lanes read consecutive floats (no bank conflict)
    for (int i = threadIdx.x; i < IN * TILE; i += TPB) {
        const int ly = i / TILE, lx = i % TILE;
        const float* c = &s_in[ly * IN + lx + R];
        float a = 0.f;
#pragma unroll
        for (int d = R; d > 0; --d) a = fmaf(TAPS[d], c[-d] + c[d], a);
        s_h[i] = fmaf(TAPS[0], c[0], a);
    }
    __syncthreads();
    // 3. along y, four pixels per lane (16-byte LDS reads of consecutive lanes), store
    float* out = L.dst + base;
    const bool vec4 = (L.w & 3) == 0 && ((uintptr_t)L.dst % 16) == 0;
    for (int i = threadIdx.x; i < TILE * TILE / 4; i += TPB) {
        const int ly = i / (TILE / 4), lx = (i % (TILE / 4)) * 4;
        const int y = ty0 + ly, x0 = tx0 + lx;
        if (y >= L.h || x0 >= L.w) continue;
        const float* c = &s_h[(ly + R) * TILE + lx];
        float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int d = R; d > 0; --d) {
            const float4 q = *reinterpret_cast<const float4*>(c - d * TILE), r = *reinterpret_cast<const float4*>(c + d * TILE);
            a[0] = fmaf(TAPS[d], q.x + r.x, a[0]);
            a[1] = fmaf(TAPS[d], q.y + r.y, a[1]);
            a[2] = fmaf(TAPS[d], q.z + r.z, a[2]);
            a[3] = fmaf(TAPS[d], q.w + r.w, a[3]);
        }
        const float4 q = *reinterpret_cast<const float4*>(c);
        a[0] = fmaf(TAPS[0], q.x, a[0]);
        a[1] = fmaf(TAPS[0], q.y, a[1]);
        a[2] = fmaf(TAPS[0], q.z, a[2]);
        a[3] = fmaf(TAPS[0], q.w, a[3]);
        if (vec4) *reinterpret_cast<float4*>(out + y * L.w + x0) = float4{a[0], a[1], a[2], a[3]};
        else {
            const int cnt = min(4, L.w - x0);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) out[y * L.w + x0 + j] = a[j];
        }
    }
}

// cubic B-spline weights of the taps floor(c) - 1 .. floor(c) + 2 at the fraction t, fp64, rounded once
__device__ __forceinline__ void weights(double t, float w[4]) {
    const double u = 1.0 - t;
    w[0] = (float)(u * u * u / 6.0);
    w[1] = (float)((4.0 + t * t * (3.0 * t - 6.0)) / 6.0);
    w[2] = (float)((1.0 + t * (3.0 + t * (3.0 - 3.0 * t))) / 6.0);
    w[3] = (float)(t * t * t / 6.0);
}

// one output pixel of plane p of sample s (base = first element of the sample's field)
__device__ __forceinline__ float pixel(const Launch& L, const biu_augf_params& P, int s, int base, int p, int hw, int x, int y) {
    double sx, sy;
    source_of(P, x, y, sx, sy);
    if (!(P.flags & BIU_AUGF_ROT))         // biu_augment_f32's MASK gather
        return load(L, base + p * hw + wrap((int)floor(sy + 0.5), L.h) * L.w + wrap((int)floor(sx + 0.5), L.w));
    const double x0f = floor(sx), y0f = floor(sy);
    float wx[4], wy[4];
    weights(sx - x0f, wx);
    weights(sy - y0f, wy);
    int xi[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) xi[j] = wrap((int)x0f - 1 + j, L.w);
    const float* c = L.coef + base + p * hw;
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float* row = c + wrap((int)y0f - 1 + i, L.h) * L.w;
        float a = wx[0] * row[xi[0]];
        a = fmaf(wx[1], row[xi[1]], a);
        a = fmaf(wx[2], row[xi[2]], a);
        a = fmaf(wx[3], row[xi[3]], a);
        v = fmaf(wy[i], a, v);
    }
    const float lo = L.range[2 * s], hi = L.range[2 * s + 1];
    if (lo >= 0.f && hi <= 1.f) v = fminf(fmaxf(v, lo), hi);
    return v;
}

// ROWS: w % 4 == 0 and dst 16-byte aligned, a lane's 4 pixels lie in one row of one plane; otherwise every pixel finds its own place
template <bool ROWS>
__global__ __launch_bounds__(TPB) void k_spline_gather(Launch L, int total) {
    const int hw = L.h * L.w, field = L.planes * hw;
    const int groups = (total + GROUP - 1) / GROUP;
    for (int g = blockIdx.x * TPB + threadIdx.x; g < groups; g += gridDim.x * TPB) {
        const int e0 = g * GROUP;
        if (ROWS) {
            const int s = e0 / field, inf = e0 - s * field;          // sample, index inside its field
            const int p = inf / hw, inp = inf - p * hw;
            const int y = inp / L.w, x0 = inp - y * L.w;
            const biu_augf_params P = L.params[s];
            float4 o;
            o.x = pixel(L, P, s, s * field, p, hw, x0, y);
            o.y = pixel(L, P, s, s * field, p, hw, x0 + 1, y);
            o.z = pixel(L, P, s, s * field, p, hw, x0 + 2, y);
            o.w = pixel(L, P, s, s * field, p, hw, x0 + 3, y);
            *reinterpret_cast<float4*>(L.dst + e0) = o;
        } else {
            for (int j = 0; j < GROUP && e0 + j < total; ++j) {
                const int e = e0 + j;
                const int s = e / field, inf = e - s * field;
                const int p = inf / hw, inp = inf - p * hw;
                const int y = inp / L.w, x = inp - y * L.w;
                const biu_augf_params P = L.params[s];
                L.dst[e] = pixel(L, P, s, s * field, p, hw, x, y);
            }
        }
    }
}
}  // namespace

extern "C" int biu_spline_prefilter_f32(const void* src, int src_is_u8, float* coef, float* range, int n, int planes, int h, int w,
                                        const biu_augf_params* params, biu_stream stream) {
    BIU_REQUIRE(src && coef && range && params && n > 0 && planes > 0 && h > 0 && w > 0, BIU_ERR_SHAPE, "spline_prefilter_f32: bad arguments");
    BIU_REQUIRE((i64)n * planes * h * w < ((i64)1 << 31) - GROUP, BIU_ERR_SHAPE, "spline_prefilter_f32: the batch field has 2^31 elements or more");
    BIU_REQUIRE(((uintptr_t)coef % 4) == 0 && ((uintptr_t)range % 4) == 0 && (src_is_u8 || ((uintptr_t)src % 4) == 0), BIU_ERR_SHAPE,
                "spline_prefilter_f32: unaligned float pointer");
    const int total = n * planes * h * w;
    const i64 src_bytes = (i64)total * (src_is_u8 ? 1 : 4), coef_bytes = (i64)total * 4, range_bytes = (i64)n * 8;
    BIU_REQUIRE(!overlap(src, src_bytes, coef, coef_bytes) && !overlap(src, src_bytes, range, range_bytes) && !overlap(coef, coef_bytes, range, range_bytes),
                BIU_ERR_SHAPE, "spline_prefilter_f32: src, coef and range must not overlap");
    const int tx = (w + TILE - 1) / TILE, ty = (h + TILE - 1) / TILE;
    BIU_REQUIRE((i64)n * planes * tx * ty < ((i64)1 << 31), BIU_ERR_SHAPE, "spline_prefilter_f32: too many tiles");
    hipStream_t st = (hipStream_t)stream;
    Launch L{src, nullptr, nullptr, range, params, src_is_u8 != 0, n, planes, h, w};
    const int field = planes * h * w;
    const int vec = field % (src_is_u8 ? 16 : 4) == 0 && ((uintptr_t)src % 16) == 0;         // every sample's field starts 16-byte aligned
    hipLaunchKernelGGL(k_spline_range, dim3(n), dim3(RANGE_TPB), 0, st, L, vec);
    L.dst = coef;
    hipLaunchKernelGGL(k_spline_prefilter, dim3(n * planes * tx * ty), dim3(TPB), 0, st, L, tx, ty);
    BIU_CHECK_LAUNCH("spline_prefilter_f32");
    return BIU_OK;
}

extern "C" int biu_augment_f32_cubic(const void* src, int src_is_u8, const float* coef, const float* range, float* dst, int n, int planes, int h,
                                     int w, const biu_augf_params* params, biu_stream stream) {
    BIU_REQUIRE(src && coef && range && dst && params && n > 0 && planes > 0 && h > 0 && w > 0, BIU_ERR_SHAPE, "augment_f32_cubic: bad arguments");
    BIU_REQUIRE((i64)n * planes * h * w < ((i64)1 << 31) - GROUP, BIU_ERR_SHAPE, "augment_f32_cubic: the batch field has 2^31 elements or more");
    BIU_REQUIRE(((uintptr_t)dst % 4) == 0 && ((uintptr_t)coef % 4) == 0 && ((uintptr_t)range % 4) == 0 && (src_is_u8 || ((uintptr_t)src % 4) == 0),
                BIU_ERR_SHAPE, "augment_f32_cubic: unaligned float pointer");
    const int total = n * planes * h * w;
    const i64 src_bytes = (i64)total * (src_is_u8 ? 1 : 4), f_bytes = (i64)total * 4, range_bytes = (i64)n * 8;
    BIU_REQUIRE(!overlap(dst, f_bytes, src, src_bytes) && !overlap(dst, f_bytes, coef, f_bytes) && !overlap(dst, f_bytes, range, range_bytes),
                BIU_ERR_SHAPE, "augment_f32_cubic: dst must not overlap src, coef or range");
    const Launch L{src, coef, range, dst, params, src_is_u8 != 0, n, planes, h, w};
    const int grid = grid_for((total + GROUP - 1) / GROUP, TPB, 4096);
    hipStream_t st = (hipStream_t)stream;
    if (w % GROUP == 0 && ((uintptr_t)dst % 16) == 0) hipLaunchKernelGGL(k_spline_gather<true>, dim3(grid), dim3(TPB), 0, st, L, total);
    else hipLaunchKernelGGL(k_spline_gather<false>, dim3(grid), dim3(TPB), 0, st, L, total);
    BIU_CHECK_LAUNCH("augment_f32_cubic");
    return BIU_OK;
}
