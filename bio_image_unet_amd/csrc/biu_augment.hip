// On-the-fly training augmentation of uint8 tile batches on the device (the pipelines of unet/data.py:217-245, siam_unet/data.py:236-243,
// unet3d/data.py:209-239, which the reference runs offline through albumentations).  One launch per field per batch:
//
//   gather (rot90 and shift/scale/rotate composed into ONE inverse 2x3 map; bilinear for images, nearest for masks; reflect-101)
//   -> [gauss_noise] -> brightness_contrast -> [k x k box blur] -> [mult_noise]          (images only; masks stop after the gather)
//
// with the value clipped to [0, 255] and rounded to nearest-even after every stage, as a uint8 pipeline does.  The per-sample parameters
// (biu_aug_params) are drawn on the host; per-pixel noise is Philox4x32-10 keyed by the seed with the counter
// (element group, dataset index, epoch, field-and-stage id), so a batch is a pure function of (seed, epoch, dataset indices).
//
// Two kernels ("On-device augmentation"):
//   k_aug_point : no sample of the batch blurs (and every mask): the chain is per pixel; a lane owns 16 consecutive pixels of the flattened
//                 batch and stores them as one 16-byte vector.
//   k_aug_tile  : some sample blurs: a block owns a 64 x 64 output tile of one (sample, plane).  A blurring sample's block writes the exact
//                 uint8 intermediate for the tile plus a halo of k/2 <= 7 into LDS, sums k bytes along x into uint16 row sums, then k row sums
//                 along y (separable: 2k LDS reads per pixel, not k^2); the other samples' blocks run the per-pixel chain on their tile.
// The gather reads the source bytes through the vector cache (fields are 64 KiB - 8 MiB, L2-resident); there are no atomics and no scratch.
#include <hip/hip_runtime.h>

#include "biu_common.h"
#include "biu_philox.h"

namespace {
constexpr int TPB = 256;
constexpr int GROUP = 16;                      // pixels per lane in the point kernel: one 16-byte store
constexpr int TILE = 64;                        // the tile kernel's output tile is TILE x TILE
constexpr int RMAX = BIU_AUG_MAX_BLUR / 2;      // 7
constexpr int IN_MAX = TILE + 2 * RMAX;         // 78 rows / columns of intermediate
constexpr int IN_PITCH = 80;

using biu_philox::U4;
using biu_philox::philox4x32_10;      // biu_philox.h: shared with biu_augment_f32.hip
using biu_philox::uniform24;
using biu_philox::word_of;

// reflect without repeating the edge: ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ...
__device__ __forceinline__ int reflect101(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}
// a source coordinate as an index-safe number whatever the parameter record holds (NaN -> the lower bound)
__device__ __forceinline__ double safe_coord(double v) { return fmin(fmax(v, -1.0e6), 1.0e6); }
__device__ __forceinline__ float quant8(float v) { return rintf(fminf(fmaxf(v, 0.f), 255.f)); }     // clip, round to nearest-even

struct Launch {
    const uint8_t* src;
    uint8_t* dst;
    const biu_aug_params* params;
    int n, planes, h, w;
    int order;                 // BIU_AUG_ORDER_UNET | BIU_AUG_ORDER_SIAM
    uint32_t k0, k1;           // Philox key: the 64-bit seed
    uint32_t epoch, c3;        // counter words 2 and 3 (c3 = field_id * 16, the stage id is added)
};
struct NoiseCache {           // one Philox block serves 4 (mult_noise) or 2 (gauss_noise) neighbouring elements
    uint32_t ctr;
    bool valid;
    U4 r;
};
__device__ __forceinline__ const U4& noise_block(const Launch& L, const biu_aug_params& P, uint32_t ctr, uint32_t stage, NoiseCache& nc) {
    if (!nc.valid || nc.ctr != ctr) {
        nc.r = philox4x32_10(U4{ctr, P.index, L.epoch, L.c3 + stage}, L.k0, L.k1);
        nc.ctr = ctr;
        nc.valid = true;
    }
    return nc.r;
}

template <bool MASK>
__device__ __forceinline__ float gather(const uint8_t* __restrict__ pl, int h, int w, const biu_aug_params& P, int x, int y) {
    // fp64 coordinates and weights (include/biu.h): 12 double operations per pixel next to four byte loads
    const double fx = (double)x, fy = (double)y;
    const double sx = safe_coord(fma(P.m[0], fx, fma(P.m[1], fy, P.m[2])));
    const double sy = safe_coord(fma(P.m[3], fx, fma(P.m[4], fy, P.m[5])));
    if (MASK) return (float)pl[reflect101((int)rint(sy), h) * w + reflect101((int)rint(sx), w)];
    const double x0f = floor(sx), y0f = floor(sy);
    const double ax = sx - x0f, ay = sy - y0f;
    const int x0 = reflect101((int)x0f, w), x1 = reflect101((int)x0f + 1, w);
    const int y0 = reflect101((int)y0f, h), y1 = reflect101((int)y0f + 1, h);
    const double v00 = (double)pl[y0 * w + x0], v01 = (double)pl[y0 * w + x1];
    const double v10 = (double)pl[y1 * w + x0], v11 = (double)pl[y1 * w + x1];
    const double top = fma(ax, v01 - v00, v00), bot = fma(ax, v11 - v10, v10);
    return (float)rint(fmin(fmax(fma(ay, bot - top, top), 0.0), 255.0));
}

// image stages in front of the blur; `elem` = index of the pixel inside its sample's field
__device__ __forceinline__ float stages_pre(const Launch& L, const biu_aug_params& P, float v, uint32_t elem, NoiseCache& nc) {
    if (L.order == BIU_AUG_ORDER_SIAM && (P.flags & BIU_AUG_GAUSS)) {
        const U4& r = noise_block(L, P, elem >> 1, BIU_AUG_STAGE_GAUSS, nc);
        const int o = (int)(elem & 1u) * 2;
        const float u1 = uniform24(word_of(r, o)), u2 = uniform24(word_of(r, o + 1));
        const float g = P.noise_a * sqrtf(-2.f * __logf(1.f - u1)) * __builtin_amdgcn_cosf(u2);     // v_cos_f32 takes revolutions: cos(2 pi u2)
        v = quant8(v + g);
    }
    if (P.flags & BIU_AUG_BC) v = quant8(fmaf(v, P.alpha, P.beta));
    return v;
}
// ... and behind it
__device__ __forceinline__ float stages_post(const Launch& L, const biu_aug_params& P, float v, uint32_t elem, NoiseCache& nc) {
    if (L.order == BIU_AUG_ORDER_UNET && (P.flags & BIU_AUG_MULT)) {
        const U4& r = noise_block(L, P, elem >> 2, BIU_AUG_STAGE_MULT, nc);
        v = quant8(v * fmaf(uniform24(word_of(r, (int)(elem & 3u))), P.noise_b, P.noise_a));
    }
    return v;
}
template <bool MASK>
__device__ __forceinline__ uint32_t pixel(const Launch& L, const biu_aug_params& P, const uint8_t* __restrict__ pl, int x, int y, uint32_t elem,
                                          NoiseCache& nc) {
    float v = gather<MASK>(pl, L.h, L.w, P, x, y);
    if (!MASK && (P.flags & (BIU_AUG_BC | BIU_AUG_MULT | BIU_AUG_GAUSS))) v = stages_post(L, P, stages_pre(L, P, v, elem, nc), elem, nc);
    return (uint32_t)v;
}

// ROWS: w % 16 == 0, a lane's 16 pixels lie in one row of one plane; otherwise every pixel finds its own place
template <bool MASK, bool ROWS>
__global__ __launch_bounds__(TPB) void k_aug_point(Launch L, int total) {
    const int hw = L.h * L.w, field = L.planes * hw;
    const int groups = (total + GROUP - 1) / GROUP;
    for (int g = blockIdx.x * TPB + threadIdx.x; g < groups; g += gridDim.x * TPB) {
        const int e0 = g * GROUP;
        uint32_t out[GROUP / 4] = {0, 0, 0, 0};
        NoiseCache nc{0, false, U4{0, 0, 0, 0}};
        if (ROWS) {
            const int s = e0 / field, inf = e0 - s * field;          // sample, index inside its field
            const int p = inf / hw, inp = inf - p * hw;
            const int y = inp / L.w, x0 = inp - y * L.w;
            const biu_aug_params P = L.params[s];
            const uint8_t* pl = L.src + (size_t)s * field + (size_t)p * hw;
#pragma unroll
            for (int j = 0; j < GROUP; ++j) out[j >> 2] |= pixel<MASK>(L, P, pl, x0 + j, y, (uint32_t)(inf + j), nc) << (8 * (j & 3));
            *reinterpret_cast<uint4*>(L.dst + e0) = uint4{out[0], out[1], out[2], out[3]};
        } else {
            for (int j = 0; j < GROUP && e0 + j < total; ++j) {
                const int e = e0 + j;
                const int s = e / field, inf = e - s * field;
                const int p = inf / hw, inp = inf - p * hw;
                const int y = inp / L.w, x = inp - y * L.w;
                const biu_aug_params P = L.params[s];
                L.dst[e] = (uint8_t)pixel<MASK>(L, P, L.src + (size_t)s * field + (size_t)p * hw, x, y, (uint32_t)inf, nc);
            }
        }
    }
}

// images of a batch in which at least one sample blurs; grid = n * planes * tiles_y * tiles_x
__global__ __launch_bounds__(TPB) void k_aug_tile(Launch L, int tiles_x, int tiles_y) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[IN_MAX * IN_PITCH];
    __shared__ __attribute__((aligned(16))) uint16_t s_h[IN_MAX * TILE];
    int b = blockIdx.x;
    const int tx0 = (b % tiles_x) * TILE;
    b /= tiles_x;
    const int ty0 = (b % tiles_y) * TILE;
    b /= tiles_y;
    const int p = b % L.planes, s = b / L.planes;
    const int hw = L.h * L.w, field = L.planes * hw;
    const biu_aug_params P = L.params[s];
    const uint8_t* pl = L.src + (size_t)s * field + (size_t)p * hw;
    uint8_t* out = L.dst + (size_t)s * field + (size_t)p * hw;
    const bool vec4 = (L.w & 3) == 0;
    NoiseCache nc{0, false, U4{0, 0, 0, 0}};

    if (!(P.flags & BIU_AUG_BLUR) || L.order != BIU_AUG_ORDER_UNET) {
        // per-pixel chain on this tile: a lane owns 4 consecutive pixels, 16 lanes one 64-byte row segment
        for (int i = threadIdx.x; i < TILE * TILE / 4; i += TPB) {
            const int y = ty0 + i / (TILE / 4), x0 = tx0 + (i % (TILE / 4)) * 4;
            if (y >= L.h || x0 >= L.w) continue;
            uint32_t v4 = 0;
            const int cnt = min(4, L.w - x0);
            for (int j = 0; j < cnt; ++j) v4 |= pixel<false>(L, P, pl, x0 + j, y, (uint32_t)(p * hw + y * L.w + x0 + j), nc) << (8 * j);
            if (vec4) *reinterpret_cast<uint32_t*>(out + y * L.w + x0) = v4;
            else for (int j = 0; j < cnt; ++j) out[y * L.w + x0 + j] = (uint8_t)(v4 >> (8 * j));
        }
        return;
    }
    const int k = min((int)P.blur_k | 1, BIU_AUG_MAX_BLUR), r = k >> 1;      // odd, <= 15: the halo fits the LDS tile whatever the record holds
    const int iw = TILE + 2 * r, ih = TILE + 2 * r;
    // 1. the uint8 intermediate in front of the blur, tile + halo; outside the image it is the reflected intermediate (reflect-101 border)
    for (int i = threadIdx.x; i < ih * iw; i += TPB) {
        const int ly = i / iw, lx = i - ly * iw;
        const int oy = reflect101(ty0 - r + ly, L.h), ox = reflect101(tx0 - r + lx, L.w);
        const float v = stages_pre(L, P, gather<false>(pl, L.h, L.w, P, ox, oy), (uint32_t)(p * hw + oy * L.w + ox), nc);
        s_in[ly * IN_PITCH + lx] = (uint8_t)v;
    }
    __syncthreads();
    // 2. sums of k bytes along x; a wave covers one row of 64 sums, its lanes read consecutive bytes (no bank conflict)
    for (int i = threadIdx.x; i < ih * TILE; i += TPB) {
        const int ly = i / TILE, lx = i % TILE;
        uint32_t a = 0;
        for (int d = 0; d < k; ++d) a += s_in[ly * IN_PITCH + lx + d];
        s_h[i] = (uint16_t)a;                       // <= 15 * 255
    }
    __syncthreads();
    // 3. sums of k row sums along y, four pixels per lane (8-byte LDS reads of consecutive lanes: no bank conflict), mean, mult_noise, store
    const float inv = 1.f / (float)(k * k);          // sum / k^2 is never within 1 / (2 k^2) of a tie (k odd): the product rounds as the quotient does
    for (int i = threadIdx.x; i < TILE * TILE / 4; i += TPB) {
        const int ly = i / (TILE / 4), lx = (i % (TILE / 4)) * 4;
        const int y = ty0 + ly, x0 = tx0 + lx;
        if (y >= L.h || x0 >= L.w) continue;
        uint32_t a[4] = {0, 0, 0, 0};
        for (int d = 0; d < k; ++d) {
            const uint2 q = *reinterpret_cast<const uint2*>(&s_h[(ly + d) * TILE + lx]);
            a[0] += q.x & 0xffffu; a[1] += q.x >> 16; a[2] += q.y & 0xffffu; a[3] += q.y >> 16;
        }
        uint32_t v4 = 0;
        const int cnt = min(4, L.w - x0);
        for (int j = 0; j < cnt; ++j) {
            const float v = stages_post(L, P, rintf((float)a[j] * inv), (uint32_t)(p * hw + y * L.w + x0 + j), nc);
            v4 |= (uint32_t)v << (8 * j);
        }
        if (vec4) *reinterpret_cast<uint32_t*>(out + y * L.w + x0) = v4;
        else for (int j = 0; j < cnt; ++j) out[y * L.w + x0 + j] = (uint8_t)(v4 >> (8 * j));
    }
}

__global__ void k_philox_u32(uint32_t* __restrict__ out, i64 blocks, uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < blocks; i += (i64)gridDim.x * blockDim.x) {
        const U4 r = philox4x32_10(U4{c0 + (uint32_t)i, c1, c2, c3}, k0, k1);
        *reinterpret_cast<uint4*>(out + 4 * i) = uint4{r.x, r.y, r.z, r.w};
    }
}
}  // namespace

extern "C" int biu_augment_u8(const uint8_t* src, uint8_t* dst, int n, int planes, int h, int w, int is_mask, const biu_aug_params* params,
                              int stage_order, int max_blur_k, unsigned long long seed, unsigned epoch, unsigned field_id, biu_stream stream) {
    BIU_REQUIRE(src && dst && params && src != dst && n > 0 && planes > 0 && h > 0 && w > 0, BIU_ERR_SHAPE, "augment_u8: bad arguments");
    BIU_REQUIRE((i64)n * planes * h * w < ((i64)1 << 31) - GROUP, BIU_ERR_SHAPE, "augment_u8: the batch field has 2^31 elements or more");
    BIU_REQUIRE(stage_order == BIU_AUG_ORDER_UNET || stage_order == BIU_AUG_ORDER_SIAM, BIU_ERR_UNSUPPORTED, "augment_u8: unknown stage order %d",
                stage_order);
    BIU_REQUIRE(max_blur_k >= 0 && max_blur_k <= BIU_AUG_MAX_BLUR, BIU_ERR_UNSUPPORTED, "augment_u8: blur kernel %d exceeds %d", max_blur_k,
                BIU_AUG_MAX_BLUR);
    BIU_REQUIRE(max_blur_k == 0 || stage_order == BIU_AUG_ORDER_UNET, BIU_ERR_UNSUPPORTED, "augment_u8: only the unet stage order has a blur");
    BIU_REQUIRE(field_id < (1u << 28), BIU_ERR_SHAPE, "augment_u8: field_id needs 28 bits at most");
    const Launch L{src, dst, params, n, planes, h, w, stage_order, (uint32_t)seed, (uint32_t)(seed >> 32), epoch, field_id << 4};
    const int total = n * planes * h * w;
    hipStream_t st = (hipStream_t)stream;
    if (!is_mask && max_blur_k > 1) {
        const int tx = (w + TILE - 1) / TILE, ty = (h + TILE - 1) / TILE;
        BIU_REQUIRE((i64)n * planes * tx * ty < ((i64)1 << 31), BIU_ERR_SHAPE, "augment_u8: too many tiles");
        hipLaunchKernelGGL(k_aug_tile, dim3(n * planes * tx * ty), dim3(TPB), 0, st, L, tx, ty);
    } else {
        const bool rows = w % GROUP == 0 && ((uintptr_t)dst % 16) == 0;
        const int grid = grid_for((total + GROUP - 1) / GROUP, TPB, 4096);
        if (is_mask) {
            if (rows) hipLaunchKernelGGL((k_aug_point<true, true>), dim3(grid), dim3(TPB), 0, st, L, total);
            else hipLaunchKernelGGL((k_aug_point<true, false>), dim3(grid), dim3(TPB), 0, st, L, total);
        } else {
            if (rows) hipLaunchKernelGGL((k_aug_point<false, true>), dim3(grid), dim3(TPB), 0, st, L, total);
            else hipLaunchKernelGGL((k_aug_point<false, false>), dim3(grid), dim3(TPB), 0, st, L, total);
        }
    }
    BIU_CHECK_LAUNCH("augment_u8");
    return BIU_OK;
}

extern "C" int biu_philox_u32(uint32_t* out, long long blocks, unsigned long long seed, unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                              biu_stream stream) {
    BIU_REQUIRE(out && blocks > 0 && ((uintptr_t)out % 16) == 0, BIU_ERR_SHAPE, "philox_u32: bad arguments");
    hipLaunchKernelGGL(k_philox_u32, dim3(grid_for(blocks, TPB, 4096)), dim3(TPB), 0, (hipStream_t)stream, out, (i64)blocks, (uint32_t)seed,
                       (uint32_t)(seed >> 32), c0, c1, c2, c3);
    BIU_CHECK_LAUNCH("philox_u32");
    return BIU_OK;
}
