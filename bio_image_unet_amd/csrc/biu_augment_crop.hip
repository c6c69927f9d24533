// Crop augmentation of whole items on the device: the 2-D multi-output family's pipeline (multi_output_unet/data.py:187-311) rendered straight
// from an arena of whole images (feed.ImageStore.to_device), one launch per field and batch.  The sibling of biu_augment_f32.hip: the record
// (biu_augf_params), the kinds, the stages, the samplers and the Philox counter are that file's; what differs is the source.  Every sample
// names its item in the arena (biu_augf_source: element offset, h, w), m maps an OUTPUT TILE pixel to a coordinate in that item, and every
// index wraps in the item's own (h, w), however often a small item needs it.  NaN in a target means "no label": dst never holds NaN
// (include/biu.h states the rule per kind).
//
// Index math inside an item is 32-bit (planes * h * w < 2^31 - 4 is the store's guard, and checked again per sample here); the item base is
// added to the arena pointer as a 64-bit offset.  A sample whose source does not lie inside the arena is rendered as nan_to_val: the kernel
// never reads outside [arena, arena + arena_elems).
//
// Two kernels, the plan of biu_augment_f32.hip ("Whole-image stores"):
//   k_augc_point : MASK / VECTOR fields, and IMAGE fields of a batch in which no sample blurs; a lane owns 4 consecutive pixels of a row.
//   k_augc_tile  : some sample blurs: a block owns a 64 x 64 output tile of one (sample, plane); tile + halo of k/2 <= 7 gathered through the
//                  same map and wrap into LDS (78 x 80 floats), k sums along x into a second LDS array (78 x 64), then k along y.
//                  44 928 B of LDS per block, three blocks per CU: k_augf_tile's plan unchanged, because the work per block is the same.
// No atomics, no scratch.
#include <hip/hip_runtime.h>

#include "biu_common.h"
#include "biu_augment_stages.h"

namespace {
using biu_augment_stages::clip01;
using biu_augment_stages::shot_gauss;
using biu_augment_stages::source_of;

constexpr int TPB = 256;
constexpr int GROUP = 4;                        // pixels per lane: one 16-byte store
constexpr int TILE = 64;
constexpr int RMAX = BIU_AUG_MAX_BLUR / 2;      // 7
constexpr int IN_MAX = TILE + 2 * RMAX;         // 78
constexpr int IN_PITCH = 80;

struct Launch {
    const void* arena;
    float* dst;
    const biu_augf_params* params;
    const biu_augf_source* sources;
    unsigned long long arena_elems;
    int u8;                    // the arena holds bytes
    int n, planes, th, tw;
    float nan_to_val;
    uint32_t k0, k1;           // Philox key: the 64-bit seed
    uint32_t epoch, c3;        // counter words 2 and 3 (c3 = field_id * 16, the stage id is added)
};

// one sample's item: its first element and its extent; !ok: the source record does not describe a part of the arena
struct Item {
    const void* base;
    int h, w, hw;
    bool ok;
};

__device__ __forceinline__ Item item_of(const Launch& L, int s) {
    const biu_augf_source S = L.sources[s];
    Item it;
    it.h = S.h;
    it.w = S.w;
    const i64 elems = (i64)L.planes * (i64)S.h * (i64)S.w;
    it.ok = S.h > 0 && S.w > 0 && elems < ((i64)1 << 31) - GROUP && S.offset <= L.arena_elems && (unsigned long long)elems <= L.arena_elems - S.offset;
    it.hw = it.ok ? S.h * S.w : 0;
    it.base = L.u8 ? (const void*)(static_cast<const uint8_t*>(L.arena) + S.offset) : (const void*)(static_cast<const float*>(L.arena) + S.offset);
    return it;
}
__device__ __forceinline__ float load(const Launch& L, const Item& it, int i) {
    return L.u8 ? (float)static_cast<const uint8_t*>(it.base)[i] / 255.0f : static_cast<const float*>(it.base)[i];
}
__device__ __forceinline__ int wrap(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;
    i %= n;
    return i < 0 ? i + n : i;
}
// index of the nearest item pixel inside its plane
__device__ __forceinline__ int nearest_of(const Item& it, const biu_augf_params& P, int x, int y) {
    double sx, sy;
    source_of(P, x, y, sx, sy);
    return wrap((int)floor(sy + 0.5), it.h) * it.w + wrap((int)floor(sx + 0.5), it.w);
}
// bilinear MASK gather: NaN taps read 0; the fp64 weight they carry decides between nan_to_val and the interpolated value
__device__ __forceinline__ float bilinear_nan(const Launch& L, const Item& it, const biu_augf_params& P, int plane0, int x, int y) {
    double sx, sy;
    source_of(P, x, y, sx, sy);
    const double x0f = floor(sx), y0f = floor(sy);
    const double ax = sx - x0f, ay = sy - y0f;
    const int x0 = wrap((int)x0f, it.w), x1 = wrap((int)x0f + 1, it.w);
    const int y0 = wrap((int)y0f, it.h), y1 = wrap((int)y0f + 1, it.h);
    float t00 = load(L, it, plane0 + y0 * it.w + x0), t01 = load(L, it, plane0 + y0 * it.w + x1);
    float t10 = load(L, it, plane0 + y1 * it.w + x0), t11 = load(L, it, plane0 + y1 * it.w + x1);
    double w_nan = 0.0;
    if (t00 != t00) { w_nan += (1.0 - ax) * (1.0 - ay); t00 = 0.f; }
    if (t01 != t01) { w_nan += ax * (1.0 - ay); t01 = 0.f; }
    if (t10 != t10) { w_nan += (1.0 - ax) * ay; t10 = 0.f; }
    if (t11 != t11) { w_nan += ax * ay; t11 = 0.f; }
    if (w_nan >= 0.5) return L.nan_to_val;
    const double v00 = (double)t00, v01 = (double)t01, v10 = (double)t10, v11 = (double)t11;
    const double top = fma(ax, v01 - v00, v00), bot = fma(ax, v11 - v10, v10);
    return (float)fma(ay, bot - top, top);
}

// the intensity stages behind the blur; `elem` = index of the pixel inside the output tile's field
__device__ __forceinline__ float stages(const Launch& L, const biu_augf_params& P, float v, uint32_t elem) {
    v = shot_gauss(L, P, v, elem);
    if (P.flags & BIU_AUGF_BC) v = clip01(v * P.alpha + P.beta);
    return v;
}

// one output pixel (x, y) of plane p of a sample; blur is the tile kernel's business
template <int KIND>
__device__ __forceinline__ float pixel(const Launch& L, const biu_augf_params& P, const Item& it, int p, int x, int y) {
    if (!it.ok) return L.nan_to_val;
    if (KIND == BIU_AUGF_VECTOR) {
        const int i = nearest_of(it, P, x, y), q = (p & ~1) * it.hw;
        const float c = load(L, it, q + i), s = load(L, it, q + it.hw + i);
        if (c != c || s != s) return L.nan_to_val;
        return (p & 1) ? s * P.cos_t - c * P.sin_t : c * P.cos_t + s * P.sin_t;
    }
    if (KIND == BIU_AUGF_MASK) {
        if (P.flags & BIU_AUGF_ROT) return bilinear_nan(L, it, P, p * it.hw, x, y);
        const float v = load(L, it, p * it.hw + nearest_of(it, P, x, y));
        return v != v ? L.nan_to_val : v;
    }
    float v = load(L, it, p * it.hw + nearest_of(it, P, x, y));
    if (P.flags & (BIU_AUGF_SHOT | BIU_AUGF_GAUSS | BIU_AUGF_BC)) v = stages(L, P, v, (uint32_t)((p * L.th + y) * L.tw + x));
    return v;
}

// ROWS: tw % 4 == 0 and dst 16-byte aligned, a lane's 4 pixels lie in one row of one plane; otherwise every pixel finds its own place
template <int KIND, bool ROWS>
__global__ __launch_bounds__(TPB) void k_augc_point(Launch L, int total) {
    const int thw = L.th * L.tw, field = L.planes * thw;
    const int groups = (total + GROUP - 1) / GROUP;
    for (int g = blockIdx.x * TPB + threadIdx.x; g < groups; g += gridDim.x * TPB) {
        const int e0 = g * GROUP;
        if (ROWS) {
            const int s = e0 / field, inf = e0 - s * field;
            const int p = inf / thw, inp = inf - p * thw;
            const int y = inp / L.tw, x0 = inp - y * L.tw;
            const biu_augf_params P = L.params[s];
            const Item it = item_of(L, s);
            float4 o;
            o.x = pixel<KIND>(L, P, it, p, x0, y);
            o.y = pixel<KIND>(L, P, it, p, x0 + 1, y);
            o.z = pixel<KIND>(L, P, it, p, x0 + 2, y);
            o.w = pixel<KIND>(L, P, it, p, x0 + 3, y);
            *reinterpret_cast<float4*>(L.dst + e0) = o;
        } else {
            for (int j = 0; j < GROUP && e0 + j < total; ++j) {
                const int e = e0 + j;
                const int s = e / field, inf = e - s * field;
                const int p = inf / thw, inp = inf - p * thw;
                const int y = inp / L.tw, x = inp - y * L.tw;
                const biu_augf_params P = L.params[s];
                const Item it = item_of(L, s);
                L.dst[e] = pixel<KIND>(L, P, it, p, x, y);
            }
        }
    }
}

// IMAGE fields of a batch in which at least one sample blurs; grid = n * planes * tiles_y * tiles_x
__global__ __launch_bounds__(TPB) void k_augc_tile(Launch L, int tiles_x, int tiles_y) {
    __shared__ __attribute__((aligned(16))) float s_in[IN_MAX * IN_PITCH];     // 24 960 B
    __shared__ __attribute__((aligned(16))) float s_h[IN_MAX * TILE];          // 19 968 B
    int b = blockIdx.x;
    const int tx0 = (b % tiles_x) * TILE;
    b /= tiles_x;
    const int ty0 = (b % tiles_y) * TILE;
    b /= tiles_y;
    const int p = b % L.planes, s = b / L.planes;
    const int thw = L.th * L.tw, field = L.planes * thw;
    const biu_augf_params P = L.params[s];
    const Item it = item_of(L, s);
    float* out = L.dst + (size_t)s * field + (size_t)p * thw;
    const bool vec4 = (L.tw & 3) == 0 && ((uintptr_t)L.dst % 16) == 0;

    if (!(P.flags & BIU_AUGF_BLUR) || !it.ok) {
        // per-pixel chain on this tile: a lane owns 4 consecutive pixels, 16 lanes one 256-byte row segment
        for (int i = threadIdx.x; i < TILE * TILE / 4; i += TPB) {
            const int y = ty0 + i / (TILE / 4), x0 = tx0 + (i % (TILE / 4)) * 4;
            if (y >= L.th || x0 >= L.tw) continue;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            const int cnt = min(4, L.tw - x0);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) v[j] = pixel<BIU_AUGF_IMAGE>(L, P, it, p, x0 + j, y);
            if (vec4) *reinterpret_cast<float4*>(out + y * L.tw + x0) = float4{v[0], v[1], v[2], v[3]};
            else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < cnt) out[y * L.tw + x0 + j] = v[j];
            }
        }
        return;
    }
    const int k = min((int)P.blur_k | 1, BIU_AUG_MAX_BLUR), r = k >> 1;      // odd, <= 15: the halo fits the LDS tile whatever the record holds
    const int iw = TILE + 2 * r, ih = TILE + 2 * r;
    // 1. the gathered image, tile + halo; output coordinates outside the tile continue the affine map, the item index wraps
    for (int i = threadIdx.x; i < ih * iw; i += TPB) {
        const int ly = i / iw, lx = i - ly * iw;
        s_in[ly * IN_PITCH + lx] = load(L, it, p * it.hw + nearest_of(it, P, tx0 - r + lx, ty0 - r + ly));
    }
    __syncthreads();
    // 2. sums of k floats along x; a wave covers one row of 64 sums, its lanes read consecutive floats (no bank conflict)
    for (int i = threadIdx.x; i < ih * TILE; i += TPB) {
        const int ly = i / TILE, lx = i % TILE;
        float a = 0.f;
        for (int d = 0; d < k; ++d) a += s_in[ly * IN_PITCH + lx + d];
        s_h[i] = a;
    }
    __syncthreads();
    // 3. sums of k row sums along y, four pixels per lane (16-byte LDS reads of consecutive lanes), mean, the other stages, store
    const float inv = 1.f / (float)(k * k);
    for (int i = threadIdx.x; i < TILE * TILE / 4; i += TPB) {
        const int ly = i / (TILE / 4), lx = (i % (TILE / 4)) * 4;
        const int y = ty0 + ly, x0 = tx0 + lx;
        if (y >= L.th || x0 >= L.tw) continue;
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        for (int d = 0; d < k; ++d) {
            const float4 q = *reinterpret_cast<const float4*>(&s_h[(ly + d) * TILE + lx]);
            a[0] += q.x; a[1] += q.y; a[2] += q.z; a[3] += q.w;
        }
        const int cnt = min(4, L.tw - x0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a[j] *= inv;
            if (j < cnt && (P.flags & (BIU_AUGF_SHOT | BIU_AUGF_GAUSS | BIU_AUGF_BC)))
                a[j] = stages(L, P, a[j], (uint32_t)((p * L.th + y) * L.tw + x0 + j));
        }
        if (vec4) *reinterpret_cast<float4*>(out + y * L.tw + x0) = float4{a[0], a[1], a[2], a[3]};
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) out[y * L.tw + x0 + j] = a[j];
        }
    }
}

template <int KIND>
void launch_point(const Launch& L, int total, bool rows, hipStream_t st) {
    const int grid = grid_for((total + GROUP - 1) / GROUP, TPB, 4096);
    if (rows) hipLaunchKernelGGL((k_augc_point<KIND, true>), dim3(grid), dim3(TPB), 0, st, L, total);
    else hipLaunchKernelGGL((k_augc_point<KIND, false>), dim3(grid), dim3(TPB), 0, st, L, total);
}

// do [a, a + na) and [b, b + nb) share a byte
bool overlap(const void* a, unsigned long long na, const void* b, unsigned long long nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}
}  // namespace

extern "C" int biu_augment_f32_crop(const void* arena, int arena_is_u8, unsigned long long arena_elems, float* dst, int n, int planes, int th, int tw,
                                    int kind, const biu_augf_params* params, const biu_augf_source* sources, float nan_to_val, int max_blur_k,
                                    unsigned long long seed, unsigned epoch, unsigned field_id, biu_stream stream) {
    BIU_REQUIRE(arena && dst && params && sources && arena_elems > 0 && n > 0 && planes > 0 && th > 0 && tw > 0, BIU_ERR_SHAPE,
                "augment_f32_crop: bad arguments");
    BIU_REQUIRE((i64)n * planes * th * tw < ((i64)1 << 31) - GROUP, BIU_ERR_SHAPE, "augment_f32_crop: the output has 2^31 elements or more");
    BIU_REQUIRE(arena_elems < (1ull << 62), BIU_ERR_SHAPE, "augment_f32_crop: arena_elems out of range");
    BIU_REQUIRE(kind == BIU_AUGF_IMAGE || kind == BIU_AUGF_MASK || kind == BIU_AUGF_VECTOR, BIU_ERR_UNSUPPORTED, "augment_f32_crop: unknown kind %d", kind);
    BIU_REQUIRE(kind != BIU_AUGF_VECTOR || planes % 2 == 0, BIU_ERR_SHAPE, "augment_f32_crop: a vector field has (c, s) plane pairs, got %d planes", planes);
    BIU_REQUIRE(((uintptr_t)dst % 4) == 0 && (arena_is_u8 || ((uintptr_t)arena % 4) == 0), BIU_ERR_SHAPE, "augment_f32_crop: unaligned float pointer");
    BIU_REQUIRE(((uintptr_t)params % 8) == 0 && ((uintptr_t)sources % 8) == 0, BIU_ERR_SHAPE, "augment_f32_crop: unaligned record pointer");
    BIU_REQUIRE(nan_to_val == nan_to_val, BIU_ERR_SHAPE, "augment_f32_crop: nan_to_val is NaN");
    const unsigned long long arena_bytes = arena_elems * (arena_is_u8 ? 1ull : 4ull), dst_bytes = (unsigned long long)n * planes * th * tw * 4ull;
    const unsigned long long par_bytes = (unsigned long long)n * sizeof(biu_augf_params), src_bytes = (unsigned long long)n * sizeof(biu_augf_source);
    BIU_REQUIRE(!overlap(dst, dst_bytes, arena, arena_bytes) && !overlap(dst, dst_bytes, params, par_bytes) && !overlap(dst, dst_bytes, sources, src_bytes),
                BIU_ERR_SHAPE, "augment_f32_crop: dst must not overlap the arena or the records");
    BIU_REQUIRE(max_blur_k >= 0 && max_blur_k <= BIU_AUG_MAX_BLUR, BIU_ERR_UNSUPPORTED, "augment_f32_crop: blur kernel %d exceeds %d", max_blur_k,
                BIU_AUG_MAX_BLUR);
    BIU_REQUIRE(field_id < (1u << 28), BIU_ERR_SHAPE, "augment_f32_crop: field_id needs 28 bits at most");
    const Launch L{arena, dst, params, sources, arena_elems, arena_is_u8 != 0, n, planes, th, tw, nan_to_val,
                   (uint32_t)seed, (uint32_t)(seed >> 32), epoch, field_id << 4};
    const int total = n * planes * th * tw;
    hipStream_t st = (hipStream_t)stream;
    if (kind == BIU_AUGF_IMAGE && max_blur_k > 1) {
        const int tx = (tw + TILE - 1) / TILE, ty = (th + TILE - 1) / TILE;
        BIU_REQUIRE((i64)n * planes * tx * ty < ((i64)1 << 31), BIU_ERR_SHAPE, "augment_f32_crop: too many tiles");
        hipLaunchKernelGGL(k_augc_tile, dim3(n * planes * tx * ty), dim3(TPB), 0, st, L, tx, ty);
    } else {
        const bool rows = tw % GROUP == 0 && ((uintptr_t)dst % 16) == 0;
        if (kind == BIU_AUGF_IMAGE) launch_point<BIU_AUGF_IMAGE>(L, total, rows, st);
        else if (kind == BIU_AUGF_MASK) launch_point<BIU_AUGF_MASK>(L, total, rows, st);
        else launch_point<BIU_AUGF_VECTOR>(L, total, rows, st);
    }
    BIU_CHECK_LAUNCH("augment_f32_crop");
    return BIU_OK;
}
