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
// Two kernels ("On-device augmentation"):
//   k_augf_point : every MASK / VECTOR field, and IMAGE fields of a batch in which no sample blurs: the chain is per pixel; a lane owns 4
//                  consecutive pixels of a row and stores them as one 16-byte vector.
//   k_augf_tile  : some sample blurs: a block owns a 64 x 64 output tile of one (sample, plane).  A blurring sample's block gathers the tile
//                  plus a halo of k/2 <= 7 into LDS (the halo continues the affine map: the reference blurs before it crops), sums k floats
//                  along x, then k row sums along y; the other samples' blocks run the per-pixel chain on their tile.
// The noise stages call the accurate library functions (logf, exp2f, cospif ...), not the bare v_log_f32 / v_exp_f32 / v_cos_f32: the result
// is a float the loss reads, not a byte, and these launches are latency-bound.  No atomics, no scratch.
#include <hip/hip_runtime.h>

#include "biu_common.h"
#include "biu_augment_stages.h"

namespace {
using biu_augment_stages::clip01;
using biu_augment_stages::shot_gauss;
using biu_augment_stages::source_of;

constexpr int TPB = 256;
constexpr int GROUP = 4;                        // pixels per lane: one 16-byte store
constexpr int TILE = 64;                        // the tile kernel's output tile is TILE x TILE
constexpr int RMAX = BIU_AUG_MAX_BLUR / 2;      // 7
constexpr int IN_MAX = TILE + 2 * RMAX;         // 78 rows / columns of gathered image
constexpr int IN_PITCH = 80;

struct Launch {
    const void* src;
    float* dst;
    const biu_augf_params* params;
    int u8;                    // src holds bytes
    int n, planes, h, w;
    uint32_t k0, k1;           // Philox key: the 64-bit seed
    uint32_t epoch, c3;        // counter words 2 and 3 (c3 = field_id * 16, the stage id is added)
};

__device__ __forceinline__ float load(const Launch& L, int i) {
    return L.u8 ? (float)static_cast<const uint8_t*>(L.src)[i] / 255.0f : static_cast<const float*>(L.src)[i];
}
__device__ __forceinline__ int wrap(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;
    i %= n;
    return i < 0 ? i + n : i;
}
// index of the nearest source pixel inside its plane
__device__ __forceinline__ int nearest_of(const Launch& L, const biu_augf_params& P, int x, int y) {
    double sx, sy;
    source_of(P, x, y, sx, sy);
    return wrap((int)floor(sy + 0.5), L.h) * L.w + wrap((int)floor(sx + 0.5), L.w);
}
__device__ __forceinline__ float bilinear(const Launch& L, const biu_augf_params& P, int base, int x, int y) {
    double sx, sy;
    source_of(P, x, y, sx, sy);
    const double x0f = floor(sx), y0f = floor(sy);
    const double ax = sx - x0f, ay = sy - y0f;
    const int x0 = wrap((int)x0f, L.w), x1 = wrap((int)x0f + 1, L.w);
    const int y0 = wrap((int)y0f, L.h), y1 = wrap((int)y0f + 1, L.h);
    const double v00 = (double)load(L, base + y0 * L.w + x0), v01 = (double)load(L, base + y0 * L.w + x1);
    const double v10 = (double)load(L, base + y1 * L.w + x0), v11 = (double)load(L, base + y1 * L.w + x1);
    const double top = fma(ax, v01 - v00, v00), bot = fma(ax, v11 - v10, v10);
    return (float)fma(ay, bot - top, top);
}

// the intensity stages behind the blur; `elem` = index of the pixel inside its sample's field
__device__ __forceinline__ float stages(const Launch& L, const biu_augf_params& P, float v, uint32_t elem) {
    v = shot_gauss(L, P, v, elem);                                              // shared with biu_augment_vol.hip
    if (P.flags & BIU_AUGF_BC) v = clip01(v * P.alpha + P.beta);
    return v;
}

// one output pixel of plane p of sample s (base = first element of the sample's field); blur is the tile kernel's business
template <int KIND>
__device__ __forceinline__ float pixel(const Launch& L, const biu_augf_params& P, int base, int p, int hw, int x, int y) {
    if (KIND == BIU_AUGF_VECTOR) {
        const int i = nearest_of(L, P, x, y), q = base + (p & ~1) * hw;
        const float c = load(L, q + i), s = load(L, q + hw + i);
        return (p & 1) ? s * P.cos_t - c * P.sin_t : c * P.cos_t + s * P.sin_t;
    }
    if (KIND == BIU_AUGF_MASK) {
        if (P.flags & BIU_AUGF_ROT) return bilinear(L, P, base + p * hw, x, y);
        return load(L, base + p * hw + nearest_of(L, P, x, y));
    }
    float v = load(L, base + p * hw + nearest_of(L, P, x, y));
    if (P.flags & (BIU_AUGF_SHOT | BIU_AUGF_GAUSS | BIU_AUGF_BC)) v = stages(L, P, v, (uint32_t)(p * hw + y * L.w + x));
    return v;
}

// ROWS: w % 4 == 0 and dst 16-byte aligned, a lane's 4 pixels lie in one row of one plane; otherwise every pixel finds its own place
template <int KIND, bool ROWS>
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
            float4 o;
            o.x = pixel<KIND>(L, P, s * field, p, hw, x0, y);
            o.y = pixel<KIND>(L, P, s * field, p, hw, x0 + 1, y);
            o.z = pixel<KIND>(L, P, s * field, p, hw, x0 + 2, y);
            o.w = pixel<KIND>(L, P, s * field, p, hw, x0 + 3, y);
            *reinterpret_cast<float4*>(L.dst + e0) = o;
        } else {
            for (int j = 0; j < GROUP && e0 + j < total; ++j) {
                const int e = e0 + j;
                const int s = e / field, inf = e - s * field;
                const int p = inf / hw, inp = inf - p * hw;
                const int y = inp / L.w, x = inp - y * L.w;
                const biu_augf_params P = L.params[s];
                L.dst[e] = pixel<KIND>(L, P, s * field, p, hw, x, y);
            }
        }
    }
}

// IMAGE fields of a batch in which at least one sample blurs; grid = n * planes * tiles_y * tiles_x
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
    float* out = L.dst + (size_t)s * field + (size_t)p * hw;
    const bool vec4 = (L.w & 3) == 0 && ((uintptr_t)L.dst % 16) == 0;

    if (!(P.flags & BIU_AUGF_BLUR)) {
        // per-pixel chain on this tile: a lane owns 4 consecutive pixels, 16 lanes one 256-byte row segment
        for (int i = threadIdx.x; i < TILE * TILE / 4; i += TPB) {
            const int y = ty0 + i / (TILE / 4), x0 = tx0 + (i % (TILE / 4)) * 4;
            if (y >= L.h || x0 >= L.w) continue;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            const int cnt = min(4, L.w - x0);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) v[j] = pixel<BIU_AUGF_IMAGE>(L, P, s * field, p, hw, x0 + j, y);
            if (vec4) *reinterpret_cast<float4*>(out + y * L.w + x0) = float4{v[0], v[1], v[2], v[3]};
            else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < cnt) out[y * L.w + x0 + j] = v[j];
            }
        }
        return;
    }
    const int k = min((int)P.blur_k | 1, BIU_AUG_MAX_BLUR), r = k >> 1;      // odd, <= 15: the halo fits the LDS tile whatever the record holds
    const int iw = TILE + 2 * r, ih = TILE + 2 * r;
    // 1. the gathered image, tile + halo; output coordinates outside the tile continue the affine map, the source index wraps
    for (int i = threadIdx.x; i < ih * iw; i += TPB) {
        const int ly = i / iw, lx = i - ly * iw;
        s_in[ly * IN_PITCH + lx] = load(L, s * field + p * hw + nearest_of(L, P, tx0 - r + lx, ty0 - r + ly));
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
        if (y >= L.h || x0 >= L.w) continue;
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        for (int d = 0; d < k; ++d) {
            const float4 q = *reinterpret_cast<const float4*>(&s_h[(ly + d) * TILE + lx]);
            a[0] += q.x; a[1] += q.y; a[2] += q.z; a[3] += q.w;
        }
        const int cnt = min(4, L.w - x0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a[j] *= inv;
            if (j < cnt && (P.flags & (BIU_AUGF_SHOT | BIU_AUGF_GAUSS | BIU_AUGF_BC))) a[j] = stages(L, P, a[j], (uint32_t)(p * hw + y * L.w + x0 + j));
        }
        if (vec4) *reinterpret_cast<float4*>(out + y * L.w + x0) = float4{a[0], a[1], a[2], a[3]};
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) out[y * L.w + x0 + j] = a[j];
        }
    }
}

template <int KIND>
void launch_point(const Launch& L, int total, bool rows, hipStream_t st) {
    const int grid = grid_for((total + GROUP - 1) / GROUP, TPB, 4096);
    if (rows) hipLaunchKernelGGL((k_augf_point<KIND, true>), dim3(grid), dim3(TPB), 0, st, L, total);
    else hipLaunchKernelGGL((k_augf_point<KIND, false>), dim3(grid), dim3(TPB), 0, st, L, total);
}
}  // namespace

extern "C" int biu_augment_f32(const void* src, int src_is_u8, float* dst, int n, int planes, int h, int w, int kind, const biu_augf_params* params,
                               int max_blur_k, unsigned long long seed, unsigned epoch, unsigned field_id, biu_stream stream) {
    BIU_REQUIRE(src && dst && params && src != (const void*)dst && n > 0 && planes > 0 && h > 0 && w > 0, BIU_ERR_SHAPE, "augment_f32: bad arguments");
    BIU_REQUIRE((i64)n * planes * h * w < ((i64)1 << 31) - GROUP, BIU_ERR_SHAPE, "augment_f32: the batch field has 2^31 elements or more");
    BIU_REQUIRE(kind == BIU_AUGF_IMAGE || kind == BIU_AUGF_MASK || kind == BIU_AUGF_VECTOR, BIU_ERR_UNSUPPORTED, "augment_f32: unknown kind %d", kind);
    BIU_REQUIRE(kind != BIU_AUGF_VECTOR || planes % 2 == 0, BIU_ERR_SHAPE, "augment_f32: a vector field has (c, s) plane pairs, got %d planes", planes);
    BIU_REQUIRE(((uintptr_t)dst % 4) == 0 && (src_is_u8 || ((uintptr_t)src % 4) == 0), BIU_ERR_SHAPE, "augment_f32: unaligned float pointer");
    BIU_REQUIRE(max_blur_k >= 0 && max_blur_k <= BIU_AUG_MAX_BLUR, BIU_ERR_UNSUPPORTED, "augment_f32: blur kernel %d exceeds %d", max_blur_k,
                BIU_AUG_MAX_BLUR);
    BIU_REQUIRE(field_id < (1u << 28), BIU_ERR_SHAPE, "augment_f32: field_id needs 28 bits at most");
    const Launch L{src, dst, params, src_is_u8 != 0, n, planes, h, w, (uint32_t)seed, (uint32_t)(seed >> 32), epoch, field_id << 4};
    const int total = n * planes * h * w;
    hipStream_t st = (hipStream_t)stream;
    if (kind == BIU_AUGF_IMAGE && max_blur_k > 1) {
        const int tx = (w + TILE - 1) / TILE, ty = (h + TILE - 1) / TILE;
        BIU_REQUIRE((i64)n * planes * tx * ty < ((i64)1 << 31), BIU_ERR_SHAPE, "augment_f32: too many tiles");
        hipLaunchKernelGGL(k_augf_tile, dim3(n * planes * tx * ty), dim3(TPB), 0, st, L, tx, ty);
    } else {
        const bool rows = w % GROUP == 0 && ((uintptr_t)dst % 16) == 0;
        if (kind == BIU_AUGF_IMAGE) launch_point<BIU_AUGF_IMAGE>(L, total, rows, st);
        else if (kind == BIU_AUGF_MASK) launch_point<BIU_AUGF_MASK>(L, total, rows, st);
        else launch_point<BIU_AUGF_VECTOR>(L, total, rows, st);
    }
    BIU_CHECK_LAUNCH("augment_f32");
    return BIU_OK;
}
