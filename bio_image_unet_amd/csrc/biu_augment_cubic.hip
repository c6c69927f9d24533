// Cubic-spline resampling of rotated scalar targets (MASK fields) of the 2-D multi-output family: what the reference computes with
// scipy.ndimage.rotate(order=3, mode='grid-wrap') and then clips back into the target's own range (multi_output_unet/data.py:213-242).
// The sibling of biu_augment_f32.hip, which gathers these fields bilinearly; same records (biu_augf_params), same fp64 map, indices WRAP.
// The contract is in include/biu.h.  Three kernels:
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
//                        coefficients summed in fp32 (rows first), then the clip.  Other samples: the nearest gather from src.
//
// One kernel body each, as in biu_augment_f32.hip; the SOURCE of a sample is a compile-time policy:
//   Tiles : biu_spline_prefilter_f32 + biu_augment_f32_cubic, per batch.  Sample s is tile s of a batch [n, planes, h, w]; coefficients and range
//           are scratch of the batch, written for the samples whose record has BIU_AUGF_ROT and read back by the gather of the same batch.
//   Arena : biu_spline_prefilter_items (once per store) + biu_augment_f32_crop_cubic (per batch).  An item of an arena of whole images
//           (feed.ImageStore.to_device) is named by a biu_augf_source record: a 64-bit element offset and its own (h, w), in which every index
//           wraps.  The tables have the arena's layout.  NaN means "no label": the value spline runs through the zero-filled item, a second
//           one through isnan(item) as 0 / 1 (only for items that hold a NaN), and the gather renders nan_to_val where that one reaches 0.5.
//           The table kernels get one item per launch, its record by value; the gather reads one record per sample from the device and
//           validates it: a sample whose source does not lie inside the arena is rendered as nan_to_val, nothing outside the arena is read.
// Index math inside a sample is 32-bit (planes * h * w < 2^31 - 4); an item's base is added to the pointers as a 64-bit offset.
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
static_assert(sizeof(biu_spline_item) == 16, "one 16-byte load per item");

// What the Tiles kernels read comes first (biu_augment_f32.hip's rule).
struct Launch {
    const void* src;           // Tiles: the batch; Arena: the arena
    const float* coef;         // gather: the value coefficients
    const float* range;        // Tiles gather: [n][2]; Arena: biu_spline_item records (gather: the table; indicator prefilter: the item's own)
    float* dst;                // range: what it writes; prefilter: the coefficients (Arena: that arena); gather: the augmented field
    const biu_augf_params* params;
    int u8;                    // src holds bytes
    int n, planes, h, w;       // Tiles: the batch; Arena gather: the OUTPUT [n, planes, h, w]
    // Arena only
    const float* ind;          // gather: the indicator coefficients, or null
    const biu_augf_source* sources;        // gather: one record per sample; null in the table kernels, which read `one`
    const int32_t* item_index; // gather: the row of a sample's item in the table
    biu_augf_source one;       // table kernels: the launch's item
    unsigned long long arena_elems;
    int n_items;
    float nan_to_val;
};

// one sample's source: `off` elements behind src / coef / ind / (the table kernels') dst lies the arena item (Tiles: 0), `first` elements
// further the sample (Arena: 0); !ok: the record does not describe a part of the arena
struct Item {
    size_t off;
    int first, h, w, hw;
    bool ok;
};

struct Tiles {
    static constexpr bool ARENA = false;
    static __device__ __forceinline__ Item item_of(const Launch& L, int s) {
        const int hw = L.h * L.w;
        return Item{0, s * L.planes * hw, L.h, L.w, hw, true};
    }
    static __device__ __forceinline__ void range_of(const Launch& L, int s, float& lo, float& hi, bool& nan) {
        lo = L.range[2 * s];
        hi = L.range[2 * s + 1];
        nan = false;
    }
};
struct Arena {
    static constexpr bool ARENA = true;
    static __device__ __forceinline__ Item item_of(const Launch& L, int s) {
        const biu_augf_source S = L.sources ? L.sources[s] : L.one;
        Item it;
        it.first = 0;
        it.h = S.h;
        it.w = S.w;
        const i64 elems = (i64)L.planes * (i64)S.h * (i64)S.w;
        it.ok = S.h > 0 && S.w > 0 && elems < ((i64)1 << 31) - GROUP && S.offset <= L.arena_elems && (unsigned long long)elems <= L.arena_elems - S.offset;
        if (L.item_index) it.ok = it.ok && (unsigned)L.item_index[s] < (unsigned)L.n_items;
        it.hw = it.ok ? S.h * S.w : 0;
        it.off = it.ok ? (size_t)S.offset : 0;
        return it;
    }
    // the item's row of the table (it.ok holds)
    static __device__ __forceinline__ void range_of(const Launch& L, int s, float& lo, float& hi, bool& nan) {
        const biu_spline_item T = reinterpret_cast<const biu_spline_item*>(L.range)[L.item_index ? L.item_index[s] : 0];
        lo = T.lo;
        hi = T.hi;
        nan = T.has_nan != 0;
    }
};

// element i of the sample's source, a byte scaled to [0, 1] or a float
__device__ __forceinline__ float load(const Launch& L, const Item& it, int i) {
    return L.u8 ? (float)(static_cast<const uint8_t*>(L.src) + it.off)[i] / 255.0f : (static_cast<const float*>(L.src) + it.off)[i];
}

// grid = n (Arena: 1, the launch's item); one block of RANGE_TPB lanes walks the sample's field, 16 bytes per lane and step where the field
// allows it (a single block has only its own loads in flight to hide the memory latency with).  Arena: the item's biu_spline_item.
template <class S>
__global__ __launch_bounds__(RANGE_TPB) void k_spline_range(Launch L, int vec) {
    __shared__ float s_lo[RANGE_TPB / 64], s_hi[RANGE_TPB / 64];
    const int s = blockIdx.x;
    if (!S::ARENA) {
        if (!(L.params[s].flags & BIU_AUGF_ROT)) return;
    }
    const Item it = S::item_of(L, s);
    if (S::ARENA && !it.ok) return;
    const int field = L.planes * it.hw;
    float lo = INFINITY, hi = -INFINITY;                       // fminf / fmaxf pass a NaN by: "NaN aside"
    int nan = 0;                                               // Arena: some float of the item is NaN
    if (vec) {                                                 // field % 16 == 0 (bytes) or % 4 == 0 (floats), the sample 16-byte aligned
        const int per = L.u8 ? 16 : 4, groups = field / per;
        const uint4* q = reinterpret_cast<const uint4*>(static_cast<const char*>(L.src) + (it.off + (size_t)it.first) * (L.u8 ? 1 : 4));
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
                    const float f = __uint_as_float(word[j]);
                    lo = fminf(lo, f);
                    hi = fmaxf(hi, f);
                    if (S::ARENA) nan |= f != f;
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
            const float v = load(L, it, it.first + i);
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
            if (S::ARENA) nan |= v != v;
        }
    }
    if (S::ARENA) nan = __syncthreads_or(nan);
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
        if (S::ARENA) {
            *reinterpret_cast<biu_spline_item*>(L.dst) = biu_spline_item{lo, hi, nan ? 1u : 0u, 0u};
        } else {
            L.dst[2 * s] = lo;
            L.dst[2 * s + 1] = hi;
        }
    }
}

// grid = n * planes * tiles_y * tiles_x (Arena: the launch's item, n = 1).  IND (Arena): the spline through isnan(item) as 0 / 1 instead of
// the one through the zero-filled item; an item whose table row says "no NaN" is left alone
template <class S, bool IND>
__global__ __launch_bounds__(TPB) void k_spline_prefilter(Launch L, int tiles_x, int tiles_y) {
    __shared__ __attribute__((aligned(16))) float s_in[IN * IN];             // 36 864 B
    __shared__ __attribute__((aligned(16))) float s_h[IN * TILE];            // 24 576 B
    int b = blockIdx.x;
    const int tx0 = (b % tiles_x) * TILE;
    b /= tiles_x;
    const int ty0 = (b % tiles_y) * TILE;
    b /= tiles_y;
    const int p = b % L.planes, s = b / L.planes;
    if (!S::ARENA) {
        if (!(L.params[s].flags & BIU_AUGF_ROT)) return;
    }
    const Item it = S::item_of(L, s);
    if (S::ARENA) {
        if (!it.ok) return;
        if (IND) {
            float lo, hi;
            bool nan;
            S::range_of(L, s, lo, hi, nan);
            if (!nan) return;
        }
    }
    const int base = it.first + p * it.hw;
    // 1. tile + halo; the index wraps as often as the field is smaller than the halo
    for (int i = threadIdx.x; i < IN * IN; i += TPB) {
        const int ly = i / IN, lx = i - ly * IN;
        float v = load(L, it, base + wrap(ty0 - R + ly, it.h) * it.w + wrap(tx0 - R + lx, it.w));
        if (S::ARENA) v = IND ? (v != v ? 1.f : 0.f) : (v != v ? 0.f : v);
        s_in[i] = v;
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
    float* out = L.dst + it.off + base;
    const bool vec4 = (it.w & 3) == 0 && ((uintptr_t)(L.dst + it.off) % 16) == 0;
    for (int i = threadIdx.x; i < TILE * TILE / 4; i += TPB) {
        const int ly = i / (TILE / 4), lx = (i % (TILE / 4)) * 4;
        const int y = ty0 + ly, x0 = tx0 + lx;
        if (y >= it.h || x0 >= it.w) continue;
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
        if (vec4) *reinterpret_cast<float4*>(out + y * it.w + x0) = float4{a[0], a[1], a[2], a[3]};
        else {
            const int cnt = min(4, it.w - x0);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) out[y * it.w + x0 + j] = a[j];
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

// 4 x 4 coefficients of the plane at c, rows first
__device__ __forceinline__ float spline_sum(const float* c, const Item& it, const int (&xi)[4], int y0, const float (&wx)[4], const float (&wy)[4]) {
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float* row = c + wrap(y0 - 1 + i, it.h) * it.w;
        float a = wx[0] * row[xi[0]];
        a = fmaf(wx[1], row[xi[1]], a);
        a = fmaf(wx[2], row[xi[2]], a);
        a = fmaf(wx[3], row[xi[3]], a);
        v = fmaf(wy[i], a, v);
    }
    return v;
}

// one output pixel of plane p of sample s
template <class S>
__device__ __forceinline__ float pixel(const Launch& L, const biu_augf_params& P, const Item& it, int s, int p, int x, int y) {
    if (S::ARENA && !it.ok) return L.nan_to_val;
    double sx, sy;
    source_of(P, x, y, sx, sy);
    const int plane0 = it.first + p * it.hw;
    if (!(P.flags & BIU_AUGF_ROT)) {       // the MASK gather of biu_augment_f32 (Arena: of biu_augment_f32_crop, NaN -> nan_to_val)
        const float v = load(L, it, plane0 + wrap((int)floor(sy + 0.5), it.h) * it.w + wrap((int)floor(sx + 0.5), it.w));
        return S::ARENA && v != v ? L.nan_to_val : v;
    }
    const double x0f = floor(sx), y0f = floor(sy);
    float wx[4], wy[4];
    weights(sx - x0f, wx);
    weights(sy - y0f, wy);
    int xi[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) xi[j] = wrap((int)x0f - 1 + j, it.w);
    float v = spline_sum(L.coef + it.off + plane0, it, xi, (int)y0f, wx, wy);
    float lo, hi;
    bool nan;
    S::range_of(L, s, lo, hi, nan);
    if (S::ARENA && nan && L.ind) {        // the weight of "no label" at this point; an all-NaN item gives 1 up to rounding
        if (spline_sum(L.ind + it.off + plane0, it, xi, (int)y0f, wx, wy) >= 0.5f) return L.nan_to_val;
    }
    if (lo >= 0.f && hi <= 1.f) v = fminf(fmaxf(v, lo), hi);
    return v;
}

// ROWS: w % 4 == 0 and dst 16-byte aligned, a lane's 4 pixels lie in one row of one plane; otherwise every pixel finds its own place
template <class S, bool ROWS>
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
            const Item it = S::item_of(L, s);
            float4 o;
            o.x = pixel<S>(L, P, it, s, p, x0, y);
            o.y = pixel<S>(L, P, it, s, p, x0 + 1, y);
            o.z = pixel<S>(L, P, it, s, p, x0 + 2, y);
            o.w = pixel<S>(L, P, it, s, p, x0 + 3, y);
            *reinterpret_cast<float4*>(L.dst + e0) = o;
        } else {
            for (int j = 0; j < GROUP && e0 + j < total; ++j) {
                const int e = e0 + j;
                const int s = e / field, inf = e - s * field;
                const int p = inf / hw, inp = inf - p * hw;
                const int y = inp / L.w, x = inp - y * L.w;
                const biu_augf_params P = L.params[s];
                const Item it = S::item_of(L, s);
                L.dst[e] = pixel<S>(L, P, it, s, p, x, y);
            }
        }
    }
}

template <class S>
void launch_gather(const Launch& L, int total, hipStream_t st) {
    const int grid = grid_for((total + GROUP - 1) / GROUP, TPB, 4096);
    if (L.w % GROUP == 0 && ((uintptr_t)L.dst % 16) == 0) hipLaunchKernelGGL((k_spline_gather<S, true>), dim3(grid), dim3(TPB), 0, st, L, total);
    else hipLaunchKernelGGL((k_spline_gather<S, false>), dim3(grid), dim3(TPB), 0, st, L, total);
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
    Launch L{src, nullptr, nullptr, range, params, src_is_u8 != 0, n, planes, h, w, nullptr, nullptr, nullptr, biu_augf_source{0, 0, 0}, 0, 0, 0.f};
    const int field = planes * h * w;
    const int vec = field % (src_is_u8 ? 16 : 4) == 0 && ((uintptr_t)src % 16) == 0;         // every sample's field starts 16-byte aligned
    hipLaunchKernelGGL(k_spline_range<Tiles>, dim3(n), dim3(RANGE_TPB), 0, st, L, vec);
    L.dst = coef;
    hipLaunchKernelGGL((k_spline_prefilter<Tiles, false>), dim3(n * planes * tx * ty), dim3(TPB), 0, st, L, tx, ty);
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
    const Launch L{src, coef, range, dst, params, src_is_u8 != 0, n, planes, h, w, nullptr, nullptr, nullptr, biu_augf_source{0, 0, 0}, 0, 0, 0.f};
    launch_gather<Tiles>(L, total, (hipStream_t)stream);
    BIU_CHECK_LAUNCH("augment_f32_cubic");
    return BIU_OK;
}

extern "C" int biu_spline_prefilter_items(const void* arena, int arena_is_u8, unsigned long long arena_elems, float* coef, float* indicator,
                                          biu_spline_item* table, int n_items, int planes, const biu_augf_source* items, biu_stream stream) {
    BIU_REQUIRE(arena && table && items && (coef || indicator) && arena_elems > 0 && n_items > 0 && planes > 0, BIU_ERR_SHAPE,
                "spline_prefilter_items: bad arguments");
    BIU_REQUIRE(arena_elems < (1ull << 62), BIU_ERR_SHAPE, "spline_prefilter_items: arena_elems out of range");
    BIU_REQUIRE(((uintptr_t)coef % 4) == 0 && ((uintptr_t)indicator % 4) == 0 && ((uintptr_t)table % 16) == 0 && (arena_is_u8 || ((uintptr_t)arena % 4) == 0),
                BIU_ERR_SHAPE, "spline_prefilter_items: unaligned pointer (floats 4 bytes, the table 16)");
    const unsigned long long arena_bytes = arena_elems * (arena_is_u8 ? 1ull : 4ull), f_bytes = arena_elems * 4ull;
    const unsigned long long table_bytes = (unsigned long long)n_items * sizeof(biu_spline_item);
    BIU_REQUIRE(!(coef && (overlap(coef, f_bytes, arena, arena_bytes) || overlap(coef, f_bytes, table, table_bytes))) &&
                !(indicator && (overlap(indicator, f_bytes, arena, arena_bytes) || overlap(indicator, f_bytes, table, table_bytes))) &&
                !(coef && indicator && overlap(coef, f_bytes, indicator, f_bytes)) && !overlap(table, table_bytes, arena, arena_bytes),
                BIU_ERR_SHAPE, "spline_prefilter_items: the arena, coef, indicator and the table must not overlap");
    for (int i = 0; i < n_items; ++i) {            // every item before the first launch
        const biu_augf_source S = items[i];
        const i64 elems = (i64)planes * (i64)S.h * (i64)S.w;
        BIU_REQUIRE(S.h > 0 && S.w > 0 && elems < ((i64)1 << 31) - GROUP && S.offset <= arena_elems && (unsigned long long)elems <= arena_elems - S.offset,
                    BIU_ERR_SHAPE, "spline_prefilter_items: item %d (offset %llu, %d x %d x %d) does not lie inside the arena of %llu elements", i,
                    (unsigned long long)S.offset, planes, S.h, S.w, arena_elems);
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t esize = arena_is_u8 ? 1 : 4;
    for (int i = 0; i < n_items; ++i) {
        const biu_augf_source S = items[i];
        Launch L{arena, nullptr, reinterpret_cast<const float*>(table + i), reinterpret_cast<float*>(table + i), nullptr, arena_is_u8 != 0,
                 1, planes, S.h, S.w, nullptr, nullptr, nullptr, S, arena_elems, n_items, 0.f};
        const int field = planes * S.h * S.w;
        const int vec = field % (arena_is_u8 ? 16 : 4) == 0 && (((uintptr_t)arena + S.offset * esize) % 16) == 0;
        hipLaunchKernelGGL(k_spline_range<Arena>, dim3(1), dim3(RANGE_TPB), 0, st, L, vec);
        const int tx = (S.w + TILE - 1) / TILE, ty = (S.h + TILE - 1) / TILE;          // planes tx ty <= field < 2^31
        if (coef) {
            L.dst = coef;
            hipLaunchKernelGGL((k_spline_prefilter<Arena, false>), dim3(planes * tx * ty), dim3(TPB), 0, st, L, tx, ty);
        }
        if (indicator && !arena_is_u8) {           // bytes hold no NaN
            L.dst = indicator;
            hipLaunchKernelGGL((k_spline_prefilter<Arena, true>), dim3(planes * tx * ty), dim3(TPB), 0, st, L, tx, ty);
        }
    }
    BIU_CHECK_LAUNCH("spline_prefilter_items");
    return BIU_OK;
}

extern "C" int biu_augment_f32_crop_cubic(const void* arena, int arena_is_u8, unsigned long long arena_elems, const float* coef, const float* indicator,
                                          const biu_spline_item* table, int n_items, const int32_t* item_index, float* dst, int n, int planes, int th,
                                          int tw, const biu_augf_params* params, const biu_augf_source* sources, float nan_to_val, biu_stream stream) {
    BIU_REQUIRE(arena && coef && table && item_index && dst && params && sources && arena_elems > 0 && n_items > 0 && n > 0 && planes > 0 && th > 0 && tw > 0,
                BIU_ERR_SHAPE, "augment_f32_crop_cubic: bad arguments");
    BIU_REQUIRE((i64)n * planes * th * tw < ((i64)1 << 31) - GROUP, BIU_ERR_SHAPE, "augment_f32_crop_cubic: the output has 2^31 elements or more");
    BIU_REQUIRE(arena_elems < (1ull << 62), BIU_ERR_SHAPE, "augment_f32_crop_cubic: arena_elems out of range");
    BIU_REQUIRE(((uintptr_t)dst % 4) == 0 && ((uintptr_t)coef % 4) == 0 && ((uintptr_t)indicator % 4) == 0 && ((uintptr_t)item_index % 4) == 0 &&
                ((uintptr_t)table % 16) == 0 && (arena_is_u8 || ((uintptr_t)arena % 4) == 0), BIU_ERR_SHAPE,
                "augment_f32_crop_cubic: unaligned pointer (floats and indices 4 bytes, the table 16)");
    BIU_REQUIRE(((uintptr_t)params % 8) == 0 && ((uintptr_t)sources % 8) == 0, BIU_ERR_SHAPE, "augment_f32_crop_cubic: unaligned record pointer");
    BIU_REQUIRE(nan_to_val == nan_to_val, BIU_ERR_SHAPE, "augment_f32_crop_cubic: nan_to_val is NaN");
    const unsigned long long arena_bytes = arena_elems * (arena_is_u8 ? 1ull : 4ull), f_bytes = arena_elems * 4ull;
    const unsigned long long dst_bytes = (unsigned long long)n * planes * th * tw * 4ull, table_bytes = (unsigned long long)n_items * sizeof(biu_spline_item);
    const unsigned long long par_bytes = (unsigned long long)n * sizeof(biu_augf_params), src_bytes = (unsigned long long)n * sizeof(biu_augf_source);
    BIU_REQUIRE(!overlap(dst, dst_bytes, arena, arena_bytes) && !overlap(dst, dst_bytes, coef, f_bytes) && !(indicator && overlap(dst, dst_bytes, indicator, f_bytes)) &&
                !overlap(dst, dst_bytes, table, table_bytes) && !overlap(dst, dst_bytes, item_index, (unsigned long long)n * 4ull) &&
                !overlap(dst, dst_bytes, params, par_bytes) && !overlap(dst, dst_bytes, sources, src_bytes),
                BIU_ERR_SHAPE, "augment_f32_crop_cubic: dst must not overlap the arena, the tables or the records");
    const Launch L{arena, coef, reinterpret_cast<const float*>(table), dst, params, arena_is_u8 != 0, n, planes, th, tw, indicator, sources, item_index,
                   biu_augf_source{0, 0, 0}, arena_elems, n_items, nan_to_val};
    launch_gather<Arena>(L, n * planes * th * tw, (hipStream_t)stream);
    BIU_CHECK_LAUNCH("augment_f32_crop_cubic");
    return BIU_OK;
}
