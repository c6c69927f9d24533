// On-the-fly training augmentation of float fields on the device: the 2-D multi-output family's pipeline (multi_output_unet/data.py:187-311,
// which the reference runs offline through scipy.ndimage.rotate and albumentations).  The sibling of biu_augment.hip; one launch per field:
//
//   IMAGE  : nearest gather -> [k x k box blur] -> [shot noise] -> [Gauss noise] -> [brightness/contrast]
//   MASK   : bilinear gather under an arbitrary-angle rotation, nearest otherwise; nothing else
//   VECTOR : plane pairs (cos phi, sin phi): nearest gather of both planes at one source pixel, then the pair is rotated by the record's angle
//
// ONE fp64 2x3 map per sample (rotation, scale and crop offset composed on the host), indices WRAP.  The contract is in include/biu.h; the
// per-sample records (biu_augf_params) are drawn on the host, per-pixel noise is Philox4x32-10 with the counter
// (element / 2, dataset index, epoch, field-and-stage id), so a batch is a pure function of (seed, epoch, dataset indices).
//
// Two entry points, one kernel body.  What they differ in is the SOURCE of a sample, a compile-time policy of every kernel and helper:
//   Tiles : biu_augment_f32.  Sample s is tile s of a batch [n, planes, h, w]; its extent is the launch's, uniform over the launch.
//   Arena : biu_augment_f32_crop.  Sample s names its item in an arena of whole images (feed.ImageStore.to_device; biu_augf_source: element
//           offset, h, w), m maps an OUTPUT pixel to a coordinate in that item, and every index wraps in the item's own (h, w), however often
//           a small item needs it.  The record is validated per sample: a sample whose source does not lie inside the arena is rendered as
//           nan_to_val, the kernel never reads outside [arena, arena + arena_elems).  NaN in a target means "no label": dst never holds NaN
//           (include/biu.h states the rule per kind).
// Index math inside a sample is 32-bit (planes * h * w < 2^31 - 4: the launch's guard for Tiles, the store's for Arena and checked again per
// sample here); an item's base is added to the arena pointer as a 64-bit offset.
//
// Two kernels ("On-device augmentation" and "Whole-image stores"):
//   k_augf_point : every MASK / VECTOR field, and IMAGE fields of a batch in which no sample blurs: the chain is per pixel; a lane owns 4
//                  consecutive pixels of a row and stores them as one 16-byte vector.
//   k_augf_tile  : some sample blurs: a block owns a 64 x 64 output tile of one (sample, plane).  A blurring sample's block gathers the tile
//                  plus a halo of k/2 <= 7 into LDS (78 x 80 floats; the halo continues the affine map: the reference blurs before it
//                  crops), sums k floats along x into a second LDS array (78 x 64), then k row sums along y; the other samples' blocks run
//                  the per-pixel chain on their tile.  44 928 B of LDS per block, three blocks per CU, whatever the source.
// The noise stages call the accurate library functions (logf, exp2f, cospif ...), not the bare v_log_f32 / v_exp_f32 / v_cos_f32: the result
// is a float the loss reads, not a byte, and these launches are latency-bound.  No atomics, no scratch.
#include <hip/hip_runtime.h>

#include "biu_common.h"
#include "biu_augment_stages.h"

namespace {
using namespace biu_augment_stages;

constexpr int GROUP = 4;                        // pixels per lane: one 16-byte store

// What the Tiles kernels read comes first.  Where the Arena's fields stand moves single cases of the Tiles launches by up to 4 % either way
// (the scalar loads of the record are cut differently); this order measured best (profiles/r13_augment_merge.txt).
struct Launch {
    const void* src;           // Tiles: the batch; Arena: the arena
    float* dst;
    const biu_augf_params* params;
    int u8;                    // src holds bytes
    int n, planes, h, w;       // the OUTPUT: [n, planes, h, w]
    uint32_t k0, k1;           // Philox key: the 64-bit seed
    uint32_t epoch, c3;        // counter words 2 and 3 (c3 = field_id * 16, the stage id is added)
    const biu_augf_source* sources;        // Arena only, as are arena_elems and nan_to_val
    unsigned long long arena_elems;
    float nan_to_val;
};

// one sample's item: element `first` behind `base` is its first, (h, w) its extent; !ok: the source record does not describe a part of the arena
struct Item {
    const void* base;
    int first, h, w, hw;
    bool ok;
};

struct Tiles {
    static constexpr bool VALIDATED = false, NAN_RULE = false;
    // the launch's expression `s cos_t - c sin_t` had its first product fused where a lane stores 4 pixels of a row and both rounded where
    // every pixel finds its own place; rotate() keeps either
    static constexpr bool FUSED_ROWS = true;
    static __device__ __forceinline__ Item item_of(const Launch& L, int s) {
        const int hw = L.h * L.w;
        return Item{L.src, s * L.planes * hw, L.h, L.w, hw, true};
    }
};
struct Arena {
    static constexpr bool VALIDATED = true, NAN_RULE = true, FUSED_ROWS = false;
    static __device__ __forceinline__ Item item_of(const Launch& L, int s) {
        const biu_augf_source S = L.sources[s];
        Item it;
        it.first = 0;
        it.h = S.h;
        it.w = S.w;
        const i64 elems = (i64)L.planes * (i64)S.h * (i64)S.w;
        it.ok = S.h > 0 && S.w > 0 && elems < ((i64)1 << 31) - GROUP && S.offset <= L.arena_elems && (unsigned long long)elems <= L.arena_elems - S.offset;
        it.hw = it.ok ? S.h * S.w : 0;
        it.base = L.u8 ? (const void*)(static_cast<const uint8_t*>(L.src) + S.offset) : (const void*)(static_cast<const float*>(L.src) + S.offset);
        return it;
    }
};

// index of the nearest item pixel inside its plane
__device__ __forceinline__ int nearest_of(const Item& it, const biu_augf_params& P, int x, int y) {
    double sx, sy;
    source_of(P, x, y, sx, sy);
    return wrap((int)floor(sy + 0.5), it.h) * it.w + wrap((int)floor(sx + 0.5), it.w);
}
// bilinear MASK gather in the plane that starts at element plane0.  NAN_RULE: NaN taps read 0; the fp64 weight they carry decides between
// nan_to_val and the interpolated value
template <bool NAN_RULE>
__device__ __forceinline__ float bilinear(const Launch& L, const Item& it, const biu_augf_params& P, int plane0, int x, int y) {
    double sx, sy;
    source_of(P, x, y, sx, sy);
    const double x0f = floor(sx), y0f = floor(sy);
    const double ax = sx - x0f, ay = sy - y0f;
    const int x0 = wrap((int)x0f, it.w), x1 = wrap((int)x0f + 1, it.w);
    const int y0 = wrap((int)y0f, it.h), y1 = wrap((int)y0f + 1, it.h);
    float t00 = load(it.base, L.u8, plane0 + y0 * it.w + x0), t01 = load(it.base, L.u8, plane0 + y0 * it.w + x1);
    float t10 = load(it.base, L.u8, plane0 + y1 * it.w + x0), t11 = load(it.base, L.u8, plane0 + y1 * it.w + x1);
    if (NAN_RULE) {
        double w_nan = 0.0;
        if (t00 != t00) { w_nan += (1.0 - ax) * (1.0 - ay); t00 = 0.f; }
        if (t01 != t01) { w_nan += ax * (1.0 - ay); t01 = 0.f; }
        if (t10 != t10) { w_nan += (1.0 - ax) * ay; t10 = 0.f; }
        if (t11 != t11) { w_nan += ax * ay; t11 = 0.f; }
        if (w_nan >= 0.5) return L.nan_to_val;
    }
    const double v00 = (double)t00, v01 = (double)t01, v10 = (double)t10, v11 = (double)t11;
    const double top = fma(ax, v01 - v00, v00), bot = fma(ax, v11 - v10, v10);
    return (float)fma(ay, bot - top, top);
}

// plane `odd` of the pair (c, s) rotated: c cos_t + s sin_t, or s cos_t - c sin_t.  The roundings are written out; FUSED: the cos_t product
// is fused into the sum, otherwise both products are rounded (Tiles::FUSED_ROWS).
template <bool FUSED>
__device__ __forceinline__ float rotate(const biu_augf_params& P, float c, float s, bool odd) {
#pragma clang fp contract(off)
    const float a = odd ? s : c, b = odd ? -(c * P.sin_t) : s * P.sin_t;
    if (FUSED) return fmaf(a, P.cos_t, b);
    const float m = a * P.cos_t;
    return m + b;
}

// the intensity stages behind the blur; `elem` = index of the pixel inside its sample's output field
__device__ __forceinline__ float stages(const Launch& L, const biu_augf_params& P, float v, uint32_t elem) {
    v = shot_gauss(L, P, v, elem);                                              // shared with biu_augment_vol.hip
    if (P.flags & BIU_AUGF_BC) v = clip01(fmaf(v, P.alpha, P.beta));            // one rounding
    return v;
}

// one output pixel (x, y) of plane p of a sample; blur is the tile kernel's business
template <class S, int KIND, bool FUSED = false>
__device__ __forceinline__ float pixel(const Launch& L, const biu_augf_params& P, const Item& it, int p, int x, int y) {
    if (S::VALIDATED && !it.ok) return L.nan_to_val;
    if (KIND == BIU_AUGF_VECTOR) {
        const int q = it.first + (p & ~1) * it.hw + nearest_of(it, P, x, y);
        const float c = load(it.base, L.u8, q), s = load(it.base, L.u8, q + it.hw);
        if (S::NAN_RULE && (c != c || s != s)) return L.nan_to_val;
        return rotate<FUSED>(P, c, s, p & 1);
    }
    if (KIND == BIU_AUGF_MASK) {
        if (P.flags & BIU_AUGF_ROT) return bilinear<S::NAN_RULE>(L, it, P, it.first + p * it.hw, x, y);
        const float v = load(it.base, L.u8, it.first + p * it.hw + nearest_of(it, P, x, y));
        return S::NAN_RULE && v != v ? L.nan_to_val : v;
    }
    float v = load(it.base, L.u8, it.first + p * it.hw + nearest_of(it, P, x, y));
    if (P.flags & (BIU_AUGF_SHOT | BIU_AUGF_GAUSS | BIU_AUGF_BC)) v = stages(L, P, v, (uint32_t)(p * (L.h * L.w) + y * L.w + x));
    return v;
}

// ROWS: w % 4 == 0 and dst 16-byte aligned, a lane's 4 pixels lie in one row of one plane; otherwise every pixel finds its own place
template <class S, int KIND, bool ROWS>
__global__ __launch_bounds__(TPB) void k_augf_point(Launch L, int total) {
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
            o.x = pixel<S, KIND, S::FUSED_ROWS>(L, P, it, p, x0, y);
            o.y = pixel<S, KIND, S::FUSED_ROWS>(L, P, it, p, x0 + 1, y);
            o.z = pixel<S, KIND, S::FUSED_ROWS>(L, P, it, p, x0 + 2, y);
            o.w = pixel<S, KIND, S::FUSED_ROWS>(L, P, it, p, x0 + 3, y);
            *reinterpret_cast<float4*>(L.dst + e0) = o;
        } else {
            for (int j = 0; j < GROUP && e0 + j < total; ++j) {
                const int e = e0 + j;
                const int s = e / field, inf = e - s * field;
                const int p = inf / hw, inp = inf - p * hw;
                const int y = inp / L.w, x = inp - y * L.w;
                const biu_augf_params P = L.params[s];
                const Item it = S::item_of(L, s);
                L.dst[e] = pixel<S, KIND>(L, P, it, p, x, y);
            }
        }
    }
}

// IMAGE fields of a batch in which at least one sample blurs; grid = n * planes * tiles_y * tiles_x
template <class S>
__global__ __launch_bounds__(TPB) void k_augf_tile(Launch L, int tiles_x, int tiles_y) {
    __shared__ __attribute__((aligned(16))) float s_in[IN_MAX * IN_PITCH];     // 24 960 B
    __shared__ __attribute__((aligned(16))) float s_h[IN_MAX * TILE];          // 19 968 B
    int b = blockIdx.x;
    const int tx0 = (b % tiles_x) * TILE;
    b /= tiles_x;
    const int ty0 = (b % tiles_y) * TILE;
    b /= tiles_y;
    const int p = b % L.planes, s = b / L.planes;
    const int hw = L.h * L.w, field = L.planes * hw;
    const biu_augf_params P = L.params[s];
    const Item it = S::item_of(L, s);
    float* out = L.dst + (size_t)s * field + (size_t)p * hw;
    const bool vec4 = (L.w & 3) == 0 && ((uintptr_t)L.dst % 16) == 0;

    if (!(P.flags & BIU_AUGF_BLUR) || (S::VALIDATED && !it.ok)) {
        // per-pixel chain on this tile: a lane owns 4 consecutive pixels, 16 lanes one 256-byte row segment
        for (int i = threadIdx.x; i < TILE * TILE / 4; i += TPB) {
            const int y = ty0 + i / (TILE / 4), x0 = tx0 + (i % (TILE / 4)) * 4;
            if (y >= L.h || x0 >= L.w) continue;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            const int cnt = min(4, L.w - x0);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) v[j] = pixel<S, BIU_AUGF_IMAGE>(L, P, it, p, x0 + j, y);
            store<4>(out + y * L.w + x0, v, cnt, vec4);
        }
        return;
    }
    const int k = min((int)P.blur_k | 1, BIU_AUG_MAX_BLUR), r = k >> 1;      // odd, <= 15: the halo fits the LDS tile whatever the record holds
    const int iw = TILE + 2 * r, ih = TILE + 2 * r;
    // 1. the gathered image, tile + halo; output coordinates outside the tile continue the affine map, the item index wraps
    for (int i = threadIdx.x; i < ih * iw; i += TPB) {
        const int ly = i / iw, lx = i - ly * iw;
        s_in[ly * IN_PITCH + lx] = load(it.base, L.u8, it.first + p * it.hw + nearest_of(it, P, tx0 - r + lx, ty0 - r + ly));
    }
    __syncthreads();
    // 2. and 3. the box sums and the mean, then the other stages
    blur_sums(s_in, s_h, k, tx0, ty0, L.h, L.w, out, vec4, [&](float v, int x, int y) {
        return (P.flags & (BIU_AUGF_SHOT | BIU_AUGF_GAUSS | BIU_AUGF_BC)) ? stages(L, P, v, (uint32_t)((p * L.h + y) * L.w + x)) : v;
    });
}

template <class S, int KIND>
void launch_point(const Launch& L, int total, bool rows, hipStream_t st) {
    const int grid = grid_for((total + GROUP - 1) / GROUP, TPB, 4096);
    if (rows) hipLaunchKernelGGL((k_augf_point<S, KIND, true>), dim3(grid), dim3(TPB), 0, st, L, total);
    else hipLaunchKernelGGL((k_augf_point<S, KIND, false>), dim3(grid), dim3(TPB), 0, st, L, total);
}

// The checks both entry points make, in two parts because biu_augment_f32_crop has checks of its own between them; `name` is the entry
// point's, for the message.
int check_field(const char* name, const void* src, int src_is_u8, const float* dst, int planes, int kind) {
    BIU_REQUIRE(kind == BIU_AUGF_IMAGE || kind == BIU_AUGF_MASK || kind == BIU_AUGF_VECTOR, BIU_ERR_UNSUPPORTED, "%s: unknown kind %d", name, kind);
    BIU_REQUIRE(kind != BIU_AUGF_VECTOR || planes % 2 == 0, BIU_ERR_SHAPE, "%s: a vector field has (c, s) plane pairs, got %d planes", name, planes);
    BIU_REQUIRE(((uintptr_t)dst % 4) == 0 && (src_is_u8 || ((uintptr_t)src % 4) == 0), BIU_ERR_SHAPE, "%s: unaligned float pointer", name);
    return BIU_OK;
}
int check_stages(const char* name, int max_blur_k, unsigned field_id) {
    BIU_REQUIRE(max_blur_k >= 0 && max_blur_k <= BIU_AUG_MAX_BLUR, BIU_ERR_UNSUPPORTED, "%s: blur kernel %d exceeds %d", name, max_blur_k, BIU_AUG_MAX_BLUR);
    BIU_REQUIRE(field_id < (1u << 28), BIU_ERR_SHAPE, "%s: field_id needs 28 bits at most", name);
    return BIU_OK;
}

// the launch of either entry point, all arguments checked
template <class S>
int launch(const char* name, const Launch& L, int kind, int max_blur_k, biu_stream stream) {
    const int total = L.n * L.planes * L.h * L.w;
    hipStream_t st = (hipStream_t)stream;
    if (kind == BIU_AUGF_IMAGE && max_blur_k > 1) {
        const int tx = (L.w + TILE - 1) / TILE, ty = (L.h + TILE - 1) / TILE;
        BIU_REQUIRE((i64)L.n * L.planes * tx * ty < ((i64)1 << 31), BIU_ERR_SHAPE, "%s: too many tiles", name);
        hipLaunchKernelGGL(k_augf_tile<S>, dim3(L.n * L.planes * tx * ty), dim3(TPB), 0, st, L, tx, ty);
    } else {
        const bool rows = L.w % GROUP == 0 && ((uintptr_t)L.dst % 16) == 0;
        if (kind == BIU_AUGF_IMAGE) launch_point<S, BIU_AUGF_IMAGE>(L, total, rows, st);
        else if (kind == BIU_AUGF_MASK) launch_point<S, BIU_AUGF_MASK>(L, total, rows, st);
        else launch_point<S, BIU_AUGF_VECTOR>(L, total, rows, st);
    }
    BIU_CHECK_LAUNCH(name);
    return BIU_OK;
}
}  // namespace

extern "C" int biu_augment_f32(const void* src, int src_is_u8, float* dst, int n, int planes, int h, int w, int kind, const biu_augf_params* params,
                               int max_blur_k, unsigned long long seed, unsigned epoch, unsigned field_id, biu_stream stream) {
    BIU_REQUIRE(src && dst && params && src != (const void*)dst && n > 0 && planes > 0 && h > 0 && w > 0, BIU_ERR_SHAPE, "augment_f32: bad arguments");
    BIU_REQUIRE((i64)n * planes * h * w < ((i64)1 << 31) - GROUP, BIU_ERR_SHAPE, "augment_f32: the batch field has 2^31 elements or more");
    if (int rc = check_field("augment_f32", src, src_is_u8, dst, planes, kind)) return rc;
    if (int rc = check_stages("augment_f32", max_blur_k, field_id)) return rc;
    const Launch L{src, dst, params, src_is_u8 != 0, n, planes, h, w, (uint32_t)seed, (uint32_t)(seed >> 32), epoch, field_id << 4, nullptr, 0, 0.f};
    return launch<Tiles>("augment_f32", L, kind, max_blur_k, stream);
}

extern "C" int biu_augment_f32_crop(const void* arena, int arena_is_u8, unsigned long long arena_elems, float* dst, int n, int planes, int th, int tw,
                                    int kind, const biu_augf_params* params, const biu_augf_source* sources, float nan_to_val, int max_blur_k,
                                    unsigned long long seed, unsigned epoch, unsigned field_id, biu_stream stream) {
    BIU_REQUIRE(arena && dst && params && sources && arena_elems > 0 && n > 0 && planes > 0 && th > 0 && tw > 0, BIU_ERR_SHAPE,
                "augment_f32_crop: bad arguments");
    BIU_REQUIRE((i64)n * planes * th * tw < ((i64)1 << 31) - GROUP, BIU_ERR_SHAPE, "augment_f32_crop: the output has 2^31 elements or more");
    BIU_REQUIRE(arena_elems < (1ull << 62), BIU_ERR_SHAPE, "augment_f32_crop: arena_elems out of range");
    if (int rc = check_field("augment_f32_crop", arena, arena_is_u8, dst, planes, kind)) return rc;
    BIU_REQUIRE(((uintptr_t)params % 8) == 0 && ((uintptr_t)sources % 8) == 0, BIU_ERR_SHAPE, "augment_f32_crop: unaligned record pointer");
    BIU_REQUIRE(nan_to_val == nan_to_val, BIU_ERR_SHAPE, "augment_f32_crop: nan_to_val is NaN");
    const unsigned long long arena_bytes = arena_elems * (arena_is_u8 ? 1ull : 4ull), dst_bytes = (unsigned long long)n * planes * th * tw * 4ull;
    const unsigned long long par_bytes = (unsigned long long)n * sizeof(biu_augf_params), src_bytes = (unsigned long long)n * sizeof(biu_augf_source);
    BIU_REQUIRE(!overlap(dst, dst_bytes, arena, arena_bytes) && !overlap(dst, dst_bytes, params, par_bytes) && !overlap(dst, dst_bytes, sources, src_bytes),
                BIU_ERR_SHAPE, "augment_f32_crop: dst must not overlap the arena or the records");
    if (int rc = check_stages("augment_f32_crop", max_blur_k, field_id)) return rc;
    const Launch L{arena, dst, params, arena_is_u8 != 0, n, planes, th, tw, (uint32_t)seed, (uint32_t)(seed >> 32), epoch, field_id << 4,
                   sources, arena_elems, nan_to_val};
    return launch<Arena>("augment_f32_crop", L, kind, max_blur_k, stream);
}
