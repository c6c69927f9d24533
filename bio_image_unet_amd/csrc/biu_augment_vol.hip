// On-the-fly training augmentation of float VOLUMES on the device: the 3-D multi-output family's pipeline (multi_output_unet3d/data.py:152-230,
// which the reference runs offline through albumentations).  The third sibling, next to biu_augment.hip and biu_augment_f32.hip; one launch
// per field:
//
//   IMAGE  : bilinear gather -> [brightness/contrast] -> [k x k box blur of that result] -> [shot noise] -> [Gauss noise]
//   MASK   : nearest gather; nothing else
//   VECTOR : channel pairs (cos phi, sin phi), a whole volume apart: nearest gather of both at one source voxel, then the pair is rotated
//
// ONE fp64 2x3 in-plane map per sample, the same for every z-plane of every channel; borders reflect (101) or are constant 0, nothing wraps.
// The contract is in include/biu.h; the records are biu_augf_params, the noise stream is biu_augment_f32's.
//
// Two entry points, one kernel body.  What they differ in is the SOURCE of a sample, a compile-time policy of every kernel and helper:
//   Tiles : biu_augment_vol_f32.  Sample s is tile s of a batch [n, channels, d, h, w]; its extent is the launch's, uniform over the launch,
//           and output plane u reads input plane u.
//   Arena : biu_augment_vol_f32_crop (ShiftScaleRotate of the whole volume, then RandomCrop3D(dim_out)).  Sample s names its item in an arena
//           of whole volumes (feed.VolumeStore.to_device; biu_augv_source: element offset, d, h, w, first z-plane), m maps an OUTPUT pixel to
//           a coordinate in that item's (h, w) plane, the output extent (d, h, w) is not the item's, and output plane (c, z) reads plane
//           (c, z0 + z) of the item.  The record is validated per sample: a sample whose source does not describe a part of the arena that
//           holds the crop's z-planes is rendered as nan_to_val, the kernel never reads outside [arena, arena + arena_elems).  NaN in a
//           target means "no label": dst never holds NaN.
// Everything else is written once, so a crop of a whole item equals the tile launch's output bit for bit (include/biu.h, "equivalence law").
// Index math inside a sample is 32-bit (the launch refuses 2^31 output elements or more; channels * d * h * w < 2^31 - 4 is the store's guard
// for an item, checked again per sample here); an item's base is added to the arena pointer as a 64-bit offset.
//
// These fields are three orders of magnitude larger than the 2-D ones (one f32 field of a 128 x 256 x 256 sample is 32 MiB), so the work is
// cut along what the map does NOT depend on ("Volumes"; what that reaches is measured in profiles/r10_augment_vol.txt):
//   k_augv_point : a lane owns 4 consecutive pixels of one row (1 where rows are no multiple of 4) and computes their source coordinates, tap
//                  offsets and fp64 weights ONCE, then walks a chunk of the channels x depth planes with them: per voxel what is left is the
//                  loads, the interpolation and one 16-byte store.
//   k_augv_tile  : some sample of the batch blurs: a block owns a 64 x 64 tile and a chunk of planes.  A blurring sample's block fills LDS with
//                  BC(gather) of the tile plus a halo of k/2 <= 7 -- halo pixels outside the plane are the reflect-101 of the OUTPUT plane
//                  (cv2.blur on the patch), not more gathered volume -- sums k along x, then k along y; the other samples' blocks walk their
//                  planes as the point kernel does.
// No atomics, no scratch.
#include <hip/hip_runtime.h>

#include "biu_common.h"
#include "biu_augment_stages.h"

namespace {
using namespace biu_augment_stages;

constexpr int MAX_CHUNK = 16;                   // planes a lane walks with one set of taps, at most

// How a launch is cut, planned from the shape of what it WRITES, so biu_augment_vol_chunk answers for both entry points.
// Planes per lane (per block of the tile kernel): as many as MAX_CHUNK, halved while the launch would have fewer than 2048 blocks, 8 for
// each of the 256 compute units.  That figure is a guess at what hides the tail of the last wave of blocks; it has not been measured
// against other values.
struct Plan {
    bool tile, rows;
    int units, tx, ty, chunk, nchunks;
};
Plan plan_of(int n, int channels, int depth, int h, int w, int kind, int max_blur_k, bool aligned16) {
    Plan p;
    p.tile = kind == BIU_AUGF_IMAGE && max_blur_k > 1;
    p.rows = w % 4 == 0 && aligned16;
    p.units = kind == BIU_AUGF_VECTOR ? channels / 2 * depth : channels * depth;
    p.tx = (w + TILE - 1) / TILE;
    p.ty = (h + TILE - 1) / TILE;
    const i64 work = p.tile ? (i64)n * p.tx * p.ty : (i64)n * (p.rows ? h * (w / 4) : h * w);      // blocks, or lanes, per chunk
    const i64 want = p.tile ? 2048 : (i64)2048 * TPB;
    int c = MAX_CHUNK;
    while (c > 1 && work * ((p.units + c - 1) / c) < want) c >>= 1;
    p.chunk = p.units < c ? p.units : c;
    p.nchunks = (p.units + p.chunk - 1) / p.chunk;
    return p;
}

struct Launch {
    const void* src;           // Tiles: the batch; Arena: the arena
    float* dst;
    const biu_augf_params* params;
    const biu_augv_source* sources;        // Arena only, as are arena_elems and nan_to_val
    unsigned long long arena_elems;
    int u8;                    // src holds bytes
    int constant;              // border: taps outside the item's plane read 0
    int n, channels, units;    // units: OUTPUT planes a lane may walk (channels x d; VECTOR: pairs x d)
    int d, h, w;               // the OUTPUT: [n, channels, d, h, w]
    int chunk, nchunks;        // planes per lane / block, and how many such chunks cover `units`
    float nan_to_val;
    uint32_t k0, k1;           // Philox key: the 64-bit seed
    uint32_t epoch, c3;        // counter words 2 and 3 (c3 = field_id * 16, the stage id is added)
};

// one sample's item: element `first` behind `base` is its first, (d, h, w) its extent, z0 the z-plane output plane 0 reads; !ok: the source
// record does not describe a part of the arena that holds the crop
struct Item {
    const void* base;
    int first, d, h, w, hw, z0;
    bool ok;
};

struct Tiles {
    static constexpr bool VALIDATED = false, NAN_RULE = false;
    static __device__ __forceinline__ Item item_of(const Launch& L, int s) {
        const int hw = L.h * L.w;
        return Item{L.src, s * L.channels * L.d * hw, L.d, L.h, L.w, hw, 0, true};
    }
    // the item's plane that output plane u = (c, z) of an IMAGE or MASK field reads
    static __device__ __forceinline__ int plane_of(const Launch&, const Item&, int u) { return u; }
};
struct Arena {
    static constexpr bool VALIDATED = true, NAN_RULE = true;
    static __device__ __forceinline__ Item item_of(const Launch& L, int s) {
        const biu_augv_source S = L.sources[s];
        Item it;
        it.first = 0;
        it.d = S.d;
        it.h = S.h;
        it.w = S.w;
        it.z0 = S.z0;
        // no product below leaves 64 bits: d h < 2^62, and only a volume below 2^31 voxels is multiplied by the channels
        const i64 dh = (i64)S.d * (i64)S.h, lim = (i64)1 << 31;
        const bool fits = S.d > 0 && S.h > 0 && S.w > 0 && dh < lim && dh * (i64)S.w < lim;
        const i64 elems = fits ? (i64)L.channels * (dh * (i64)S.w) : lim;
        it.ok = fits && elems < lim - 4 && S.z0 >= 0 && (i64)S.z0 + L.d <= (i64)S.d && S.offset <= L.arena_elems &&
                (unsigned long long)elems <= L.arena_elems - S.offset;
        it.hw = it.ok ? S.h * S.w : 0;
        it.base = L.u8 ? (const void*)(static_cast<const uint8_t*>(L.src) + S.offset) : (const void*)(static_cast<const float*>(L.src) + S.offset);
        return it;
    }
    static __device__ __forceinline__ int plane_of(const Launch& L, const Item& it, int u) {
        const int c = u / L.d, z = u - c * L.d;
        return c * it.d + it.z0 + z;
    }
};

// the border rule: index inside 0 .. n - 1, or -1 for a tap that reads 0
__device__ __forceinline__ int border(const Launch& L, int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;
    return L.constant ? -1 : reflect(i, n);
}
__device__ __forceinline__ int offset_of(const Launch& L, const Item& it, int ix, int iy) {
    const int bx = border(L, ix, it.w), by = border(L, iy, it.h);
    return (bx | by) < 0 ? -1 : by * it.w + bx;
}
__device__ __forceinline__ float tap(const Launch& L, const Item& it, int base, int off) { return off < 0 ? 0.f : load(it.base, L.u8, base + off); }
// product and sum rounded one after the other: the fp32 formula, not a fused multiply-add
__device__ __forceinline__ float bc(const biu_augf_params& P, float v) {
#pragma clang fp contract(off)
    const float m = v * P.alpha;
    return clip01(m + P.beta);
}
// (c, s) -> (c cos_t + s sin_t, s cos_t - c sin_t) with the roundings written out: the first product of each sum is fused, the second rounded
__device__ __forceinline__ void rotate(const biu_augf_params& P, float a, float b, float& c, float& sn) {
#pragma clang fp contract(off)
    const float bs = b * P.sin_t, as = a * P.sin_t;
    c = fmaf(a, P.cos_t, bs);
    sn = fmaf(b, P.cos_t, -as);
}

// what a lane keeps of one output pixel while it walks the planes
struct Taps {
    int o00, o01, o10, o11;    // offsets inside a plane of the item, -1: reads 0 (nearest: o00 alone)
    double ax, ay;
};
template <bool BILINEAR>
__device__ __forceinline__ Taps taps_of(const Launch& L, const Item& it, const biu_augf_params& P, int x, int y) {
    double sx, sy;
    source_of(P, x, y, sx, sy);
    Taps t;
    if (BILINEAR) {
        const double x0f = floor(sx), y0f = floor(sy);
        const int x0 = (int)x0f, y0 = (int)y0f;
        t.ax = sx - x0f;
        t.ay = sy - y0f;
        t.o00 = offset_of(L, it, x0, y0);
        t.o01 = offset_of(L, it, x0 + 1, y0);
        t.o10 = offset_of(L, it, x0, y0 + 1);
        t.o11 = offset_of(L, it, x0 + 1, y0 + 1);
    } else {
        t.o00 = offset_of(L, it, (int)floor(sx + 0.5), (int)floor(sy + 0.5));
        t.o01 = t.o10 = t.o11 = -1;
        t.ax = t.ay = 0.0;
    }
    return t;
}
__device__ __forceinline__ float bilinear(const Launch& L, const Item& it, const Taps& t, int base) {
    const double v00 = (double)tap(L, it, base, t.o00), v01 = (double)tap(L, it, base, t.o01);
    const double v10 = (double)tap(L, it, base, t.o10), v11 = (double)tap(L, it, base, t.o11);
    const double top = fma(t.ax, v01 - v00, v00), bot = fma(t.ax, v11 - v10, v10);
    return (float)fma(t.ay, bot - top, top);
}

// PX output pixels (x0 .. x0 + cnt - 1, y) of sample s through the OUTPUT planes u0 .. u1 - 1; no blur here
template <class S, int KIND, int PX>
__device__ __forceinline__ void walk(const Launch& L, const biu_augf_params& P, const Item& it, int s, int x0, int y, int u0, int u1, int cnt, bool vec) {
    const int hw = L.h * L.w;
    const int inp = y * L.w + x0;
    float* out = L.dst + s * (L.channels * L.d * hw) + inp;
    if (S::VALIDATED && !it.ok) {
        float v[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) v[j] = L.nan_to_val;
        if (KIND == BIU_AUGF_VECTOR) {
            for (int u = u0; u < u1; ++u) {
                const int j2 = u / L.d, z = u - j2 * L.d;
                store<PX>(out + (2 * j2 * L.d + z) * hw, v, cnt, vec);
                store<PX>(out + ((2 * j2 + 1) * L.d + z) * hw, v, cnt, vec);
            }
        } else {
            for (int u = u0; u < u1; ++u) store<PX>(out + u * hw, v, cnt, vec);
        }
        return;
    }
    Taps t[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) t[j] = taps_of<KIND == BIU_AUGF_IMAGE>(L, it, P, x0 + j, y);
    if (KIND == BIU_AUGF_VECTOR) {
        const int pair_in = it.d * it.hw, pair_out = L.d * hw;
        for (int u = u0; u < u1; ++u) {
            const int j2 = u / L.d, z = u - j2 * L.d;
            const int base = it.first + (2 * j2 * it.d + it.z0 + z) * it.hw;     // the cos plane; the sin plane is `pair_in` further
            float c[PX], sn[PX];
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const float a = tap(L, it, base, t[j].o00), b = tap(L, it, base + pair_in, t[j].o00);
                rotate(P, a, b, c[j], sn[j]);
                if (S::NAN_RULE && (a != a || b != b)) c[j] = sn[j] = L.nan_to_val;      // no label in either plane: no label in both
            }
            float* o = out + (2 * j2 * L.d + z) * hw;
            store<PX>(o, c, cnt, vec);
            store<PX>(o + pair_out, sn, cnt, vec);
        }
    } else {
        const bool noisy = KIND == BIU_AUGF_IMAGE && (P.flags & (BIU_AUGF_SHOT | BIU_AUGF_GAUSS)) != 0;
        const bool has_bc = KIND == BIU_AUGF_IMAGE && (P.flags & BIU_AUGF_BC) != 0;
        for (int u = u0; u < u1; ++u) {
            const int base = it.first + S::plane_of(L, it, u) * it.hw;
            float v[PX];
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                if (KIND == BIU_AUGF_IMAGE) {
                    v[j] = bilinear(L, it, t[j], base);
                    if (has_bc) v[j] = bc(P, v[j]);
                    if (noisy && j < cnt) v[j] = shot_gauss(L, P, v[j], (uint32_t)(u * hw + inp + j));
                } else {
                    v[j] = tap(L, it, base, t[j].o00);
                    if (S::NAN_RULE && v[j] != v[j]) v[j] = L.nan_to_val;
                }
            }
            store<PX>(out + u * hw, v, cnt, vec);
        }
    }
}

// grid covers n x nchunks x (pixel groups of an output plane); PX = 4: w % 4 == 0 and dst is 16-byte aligned, a lane's pixels lie in one row
template <class S, int KIND, int PX>
__global__ __launch_bounds__(TPB) void k_augv_point(Launch L, int groups_per_plane, int total) {
    const int g = blockIdx.x * TPB + threadIdx.x;
    if (g >= total) return;
    const int lp = g % groups_per_plane, rest = g / groups_per_plane;
    const int ch = rest % L.nchunks, s = rest / L.nchunks;
    const int gw = L.w / PX;                                   // groups per row
    const int y = lp / gw, x0 = (lp - y * gw) * PX;
    const biu_augf_params P = L.params[s];
    walk<S, KIND, PX>(L, P, S::item_of(L, s), s, x0, y, ch * L.chunk, min((ch + 1) * L.chunk, L.units), PX, PX == 4);
}

// IMAGE fields of a batch in which at least one sample blurs; grid = n * nchunks * tiles_y * tiles_x
template <class S>
__global__ __launch_bounds__(TPB) void k_augv_tile(Launch L, int tiles_x, int tiles_y) {
    __shared__ __attribute__((aligned(16))) float s_in[IN_MAX * IN_PITCH];     // 24 960 B
    __shared__ __attribute__((aligned(16))) float s_h[IN_MAX * TILE];          // 19 968 B
    int b = blockIdx.x;
    const int tx0 = (b % tiles_x) * TILE;
    b /= tiles_x;
    const int ty0 = (b % tiles_y) * TILE;
    b /= tiles_y;
    const int ch = b % L.nchunks, s = b / L.nchunks;
    const int u0 = ch * L.chunk, u1 = min(u0 + L.chunk, L.units);
    const int hw = L.h * L.w, field = L.units * hw;
    const biu_augf_params P = L.params[s];
    const Item it = S::item_of(L, s);
    const bool vec4 = (L.w & 3) == 0 && ((uintptr_t)L.dst % 16) == 0;

    if (!(P.flags & BIU_AUGF_BLUR) || (S::VALIDATED && !it.ok)) {
        // this sample does not blur: a lane owns 4 consecutive pixels, 16 lanes one 256-byte row segment, and walks the planes
        for (int i = threadIdx.x; i < TILE * TILE / 4; i += TPB) {
            const int y = ty0 + i / (TILE / 4), x0 = tx0 + (i % (TILE / 4)) * 4;
            if (y >= L.h || x0 >= L.w) continue;
            walk<S, BIU_AUGF_IMAGE, 4>(L, P, it, s, x0, y, u0, u1, min(4, L.w - x0), vec4);
        }
        return;
    }
    const int k = min((int)P.blur_k | 1, BIU_AUG_MAX_BLUR), r = k >> 1;      // odd, <= 15: the halo fits the LDS tile whatever the record holds
    const int iw = TILE + 2 * r, ih = TILE + 2 * r;
    const bool has_bc = (P.flags & BIU_AUGF_BC) != 0, noisy = (P.flags & (BIU_AUGF_SHOT | BIU_AUGF_GAUSS)) != 0;
    for (int u = u0; u < u1; ++u) {
        const int base = it.first + S::plane_of(L, it, u) * it.hw;
        // 1. BC(gather) of the tile plus halo; an LDS pixel outside the OUTPUT plane is its reflect-101 (cv2.blur's border)
        for (int i = threadIdx.x; i < ih * iw; i += TPB) {
            const int ly = i / iw, lx = i - ly * iw;
            const Taps t = taps_of<true>(L, it, P, reflect(tx0 - r + lx, L.w), reflect(ty0 - r + ly, L.h));
            const float v = bilinear(L, it, t, base);
            s_in[ly * IN_PITCH + lx] = has_bc ? bc(P, v) : v;
        }
        __syncthreads();
        // 2. and 3. the box sums and the mean, then the noise stages
        blur_sums(s_in, s_h, k, tx0, ty0, L.h, L.w, L.dst + s * field + u * hw, vec4,
                  [&](float v, int x, int y) { return noisy ? shot_gauss(L, P, v, (uint32_t)(u * hw + y * L.w + x)) : v; });
    }
}

template <class S, int KIND>
void launch_point(const Launch& L, bool rows, hipStream_t st) {
    const int gpp = rows ? L.h * (L.w / 4) : L.h * L.w;
    const int total = L.n * L.nchunks * gpp;                    // at most the elements of the output: below 2^31
    const int grid = total / TPB + (total % TPB != 0);          // not (total + TPB - 1) / TPB, which leaves int just below 2^31
    if (rows) hipLaunchKernelGGL((k_augv_point<S, KIND, 4>), dim3(grid), dim3(TPB), 0, st, L, gpp, total);
    else hipLaunchKernelGGL((k_augv_point<S, KIND, 1>), dim3(grid), dim3(TPB), 0, st, L, gpp, total);
}

bool dims_ok(int n, int channels, int depth, int h, int w, int kind, int max_blur_k) {
    return n > 0 && channels > 0 && depth > 0 && h > 0 && w > 0 && (double)n * channels * depth * h * w < 2147483648.0 &&
           (kind == BIU_AUGF_IMAGE || kind == BIU_AUGF_MASK || (kind == BIU_AUGF_VECTOR && channels % 2 == 0)) && max_blur_k >= 0 &&
           max_blur_k <= BIU_AUG_MAX_BLUR;
}

// The checks both entry points make, in two parts because biu_augment_vol_f32_crop has checks of its own between them; `name` is the entry
// point's, for the message.
int check_field(const char* name, const void* src, int src_is_u8, const float* dst, int channels, int kind, int border) {
    BIU_REQUIRE(kind == BIU_AUGF_IMAGE || kind == BIU_AUGF_MASK || kind == BIU_AUGF_VECTOR, BIU_ERR_UNSUPPORTED, "%s: unknown kind %d", name, kind);
    BIU_REQUIRE(border == BIU_AUGV_REFLECT || border == BIU_AUGV_CONSTANT, BIU_ERR_UNSUPPORTED, "%s: unknown border %d", name, border);
    BIU_REQUIRE(kind != BIU_AUGF_VECTOR || channels % 2 == 0, BIU_ERR_SHAPE, "%s: a vector field has (c, s) channel pairs, got %d channels", name, channels);
    BIU_REQUIRE(((uintptr_t)dst % 4) == 0 && (src_is_u8 || ((uintptr_t)src % 4) == 0), BIU_ERR_SHAPE, "%s: unaligned float pointer", name);
    return BIU_OK;
}
int check_stages(const char* name, int max_blur_k, unsigned field_id) {
    BIU_REQUIRE(max_blur_k >= 0 && max_blur_k <= BIU_AUG_MAX_BLUR, BIU_ERR_UNSUPPORTED, "%s: blur kernel %d exceeds %d", name, max_blur_k, BIU_AUG_MAX_BLUR);
    BIU_REQUIRE(field_id < (1u << 28), BIU_ERR_SHAPE, "%s: field_id needs 28 bits at most", name);
    return BIU_OK;
}

// the launch of either entry point, all arguments checked; L's units, chunk and nchunks are filled in here, from the plan
template <class S>
int launch(const char* name, Launch L, int kind, int max_blur_k, biu_stream stream) {
    const Plan p = plan_of(L.n, L.channels, L.d, L.h, L.w, kind, max_blur_k, ((uintptr_t)L.dst % 16) == 0);
    L.units = p.units;
    L.chunk = p.chunk;
    L.nchunks = p.nchunks;
    hipStream_t st = (hipStream_t)stream;
    if (p.tile) hipLaunchKernelGGL(k_augv_tile<S>, dim3(L.n * p.nchunks * p.tx * p.ty), dim3(TPB), 0, st, L, p.tx, p.ty);
    else if (kind == BIU_AUGF_IMAGE) launch_point<S, BIU_AUGF_IMAGE>(L, p.rows, st);
    else if (kind == BIU_AUGF_MASK) launch_point<S, BIU_AUGF_MASK>(L, p.rows, st);
    else launch_point<S, BIU_AUGF_VECTOR>(L, p.rows, st);
    BIU_CHECK_LAUNCH(name);
    return BIU_OK;
}
}  // namespace

extern "C" int biu_augment_vol_chunk(int n, int channels, int depth, int h, int w, int kind, int max_blur_k, int dst_aligned16) {
    if (!dims_ok(n, channels, depth, h, w, kind, max_blur_k)) return 0;
    return plan_of(n, channels, depth, h, w, kind, max_blur_k, dst_aligned16 != 0).chunk;
}

extern "C" int biu_augment_vol_f32(const void* src, int src_is_u8, float* dst, int n, int channels, int depth, int h, int w, int kind, int border,
                                   const biu_augf_params* params, int max_blur_k, unsigned long long seed, unsigned epoch, unsigned field_id,
                                   biu_stream stream) {
    BIU_REQUIRE(src && dst && params && src != (const void*)dst && n > 0 && channels > 0 && depth > 0 && h > 0 && w > 0, BIU_ERR_SHAPE,
                "augment_vol_f32: bad arguments");
    BIU_REQUIRE((double)n * channels * depth * h * w < 2147483648.0, BIU_ERR_SHAPE, "augment_vol_f32: the batch field has 2^31 elements or more");
    if (int rc = check_field("augment_vol_f32", src, src_is_u8, dst, channels, kind, border)) return rc;
    if (int rc = check_stages("augment_vol_f32", max_blur_k, field_id)) return rc;
    const Launch L{src, dst, params, nullptr, 0, src_is_u8 != 0, border == BIU_AUGV_CONSTANT, n, channels, 0, depth, h, w, 0, 0, 0.f, (uint32_t)seed,
                   (uint32_t)(seed >> 32), epoch, field_id << 4};
    return launch<Tiles>("augment_vol_f32", L, kind, max_blur_k, stream);
}

extern "C" int biu_augment_vol_f32_crop(const void* arena, int arena_is_u8, unsigned long long arena_elems, float* dst, int n, int channels, int td,
                                        int th, int tw, int kind, int border, const biu_augf_params* params, const biu_augv_source* sources,
                                        float nan_to_val, int max_blur_k, unsigned long long seed, unsigned epoch, unsigned field_id,
                                        biu_stream stream) {
    BIU_REQUIRE(arena && dst && params && sources && arena_elems > 0 && n > 0 && channels > 0 && td > 0 && th > 0 && tw > 0, BIU_ERR_SHAPE,
                "augment_vol_f32_crop: bad arguments");
    BIU_REQUIRE((double)n * channels * td * th * tw < 2147483648.0, BIU_ERR_SHAPE, "augment_vol_f32_crop: the output has 2^31 elements or more");
    BIU_REQUIRE(arena_elems < (1ull << 62), BIU_ERR_SHAPE, "augment_vol_f32_crop: arena_elems out of range");
    if (int rc = check_field("augment_vol_f32_crop", arena, arena_is_u8, dst, channels, kind, border)) return rc;
    BIU_REQUIRE(((uintptr_t)params % 8) == 0 && ((uintptr_t)sources % 8) == 0, BIU_ERR_SHAPE, "augment_vol_f32_crop: unaligned record pointer");
    BIU_REQUIRE(nan_to_val == nan_to_val, BIU_ERR_SHAPE, "augment_vol_f32_crop: nan_to_val is NaN");
    const unsigned long long arena_bytes = arena_elems * (arena_is_u8 ? 1ull : 4ull), dst_bytes = (unsigned long long)n * channels * td * th * tw * 4ull;
    const unsigned long long par_bytes = (unsigned long long)n * sizeof(biu_augf_params), src_bytes = (unsigned long long)n * sizeof(biu_augv_source);
    BIU_REQUIRE(!overlap(dst, dst_bytes, arena, arena_bytes) && !overlap(dst, dst_bytes, params, par_bytes) && !overlap(dst, dst_bytes, sources, src_bytes),
                BIU_ERR_SHAPE, "augment_vol_f32_crop: dst must not overlap the arena or the records");
    if (int rc = check_stages("augment_vol_f32_crop", max_blur_k, field_id)) return rc;
    const Launch L{arena, dst, params, sources, arena_elems, arena_is_u8 != 0, border == BIU_AUGV_CONSTANT, n, channels, 0, td, th, tw, 0, 0, nan_to_val,
                   (uint32_t)seed, (uint32_t)(seed >> 32), epoch, field_id << 4};
    return launch<Arena>("augment_vol_f32_crop", L, kind, max_blur_k, stream);
}
