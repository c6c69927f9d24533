// On-the-fly training augmentation of float VOLUMES on the device: the 3-D multi-output family's pipeline (multi_output_unet3d/data.py:152-178,
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
// These fields are three orders of magnitude larger than the 2-D ones (one f32 field of a 128 x 256 x 256 sample is 32 MiB), so the work is
// cut along what the map does NOT depend on ("Volumes"; what that reaches is measured in profiles/r10_augment_vol.txt):
//   k_augv_point : a lane owns 4 consecutive pixels of one row (1 where rows are no multiple of 4) and computes their source coordinates, tap
//                  offsets and fp64 weights ONCE, then walks a chunk of the channels x depth planes with them: per voxel what is left is the
//                  loads, the interpolation and one 16-byte store.
//   k_augv_tile  : some sample of the batch blurs: a block owns a 64 x 64 tile and a chunk of planes.  A blurring sample's block fills LDS with
//                  BC(gather) of the tile plus a halo of k/2 <= 7 -- halo pixels outside the plane are the reflect-101 of the OUTPUT plane --
//                  sums k along x, then k along y; the other samples' blocks walk their planes as the point kernel does.
// No atomics, no scratch, 32-bit index math (the launch refuses 2^31 elements or more).
#include <hip/hip_runtime.h>

#include "biu_common.h"
#include "biu_augment_stages.h"
#include "biu_augment_vol_plan.h"

namespace {
using biu_augment_vol_plan::Plan;
using biu_augment_vol_plan::plan_of;
using biu_augment_vol_plan::TILE;
using biu_augment_vol_plan::TPB;
using biu_augment_stages::clip01;
using biu_augment_stages::shot_gauss;
using biu_augment_stages::source_of;

constexpr int RMAX = BIU_AUG_MAX_BLUR / 2;      // 7
constexpr int IN_MAX = TILE + 2 * RMAX;         // 78 rows / columns of BC(gather)
constexpr int IN_PITCH = 80;

struct Launch {
    const void* src;
    float* dst;
    const biu_augf_params* params;
    int u8;                    // src holds bytes
    int constant;              // border: taps outside the plane read 0
    int n, units, h, w;        // units: planes a lane may walk (channels x depth; VECTOR: pairs x depth)
    int depth;                 // VECTOR: the two planes of a pair are depth * h * w apart
    int chunk, nchunks;        // planes per lane / block, and how many such chunks cover `units`
    uint32_t k0, k1;           // Philox key: the 64-bit seed
    uint32_t epoch, c3;        // counter words 2 and 3 (c3 = field_id * 16, the stage id is added)
};

__device__ __forceinline__ float load(const Launch& L, int i) {
    return L.u8 ? (float)static_cast<const uint8_t*>(L.src)[i] / 255.0f : static_cast<const float*>(L.src)[i];
}
// reflect-101 at any distance from the image: d c b | a b c d | c b a
__device__ __forceinline__ int reflect(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}
// the border rule: index inside 0 .. n - 1, or -1 for a tap that reads 0
__device__ __forceinline__ int border(const Launch& L, int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;
    return L.constant ? -1 : reflect(i, n);
}
__device__ __forceinline__ int offset_of(const Launch& L, int ix, int iy) {
    const int bx = border(L, ix, L.w), by = border(L, iy, L.h);
    return (bx | by) < 0 ? -1 : by * L.w + bx;
}
__device__ __forceinline__ float tap(const Launch& L, int base, int off) { return off < 0 ? 0.f : load(L, base + off); }
// product and sum rounded one after the other: the fp32 formula, not a fused multiply-add
__device__ __forceinline__ float bc(const biu_augf_params& P, float v) {
#pragma clang fp contract(off)
    const float m = v * P.alpha;
    return clip01(m + P.beta);
}

// what a lane keeps of one output pixel while it walks the planes
struct Taps {
    int o00, o01, o10, o11;    // offsets inside a plane, -1: reads 0 (nearest: o00 alone)
    double ax, ay;
};
template <bool BILINEAR>
__device__ __forceinline__ Taps taps_of(const Launch& L, const biu_augf_params& P, int x, int y) {
    double sx, sy;
    source_of(P, x, y, sx, sy);
    Taps t;
    if (BILINEAR) {
        const double x0f = floor(sx), y0f = floor(sy);
        const int x0 = (int)x0f, y0 = (int)y0f;
        t.ax = sx - x0f;
        t.ay = sy - y0f;
        t.o00 = offset_of(L, x0, y0);
        t.o01 = offset_of(L, x0 + 1, y0);
        t.o10 = offset_of(L, x0, y0 + 1);
        t.o11 = offset_of(L, x0 + 1, y0 + 1);
    } else {
        t.o00 = offset_of(L, (int)floor(sx + 0.5), (int)floor(sy + 0.5));
        t.o01 = t.o10 = t.o11 = -1;
        t.ax = t.ay = 0.0;
    }
    return t;
}
__device__ __forceinline__ float bilinear(const Launch& L, const Taps& t, int base) {
    const double v00 = (double)tap(L, base, t.o00), v01 = (double)tap(L, base, t.o01);
    const double v10 = (double)tap(L, base, t.o10), v11 = (double)tap(L, base, t.o11);
    const double top = fma(t.ax, v01 - v00, v00), bot = fma(t.ax, v11 - v10, v10);
    return (float)fma(t.ay, bot - top, top);
}

template <int PX>
__device__ __forceinline__ void store(float* p, const float (&v)[PX], int cnt, bool vec) {
    if (PX == 4 && vec) {
        *reinterpret_cast<float4*>(p) = float4{v[0], v[PX > 1 ? 1 : 0], v[PX > 2 ? 2 : 0], v[PX > 3 ? 3 : 0]};
    } else {
#pragma unroll
        for (int j = 0; j < PX; ++j)
            if (j < cnt) p[j] = v[j];
    }
}

// PX pixels (x0 .. x0 + cnt - 1, y) of sample s through the planes u0 .. u1 - 1; no blur here.  field = elements of one sample.
template <int KIND, int PX>
__device__ __forceinline__ void walk(const Launch& L, const biu_augf_params& P, int s, int x0, int y, int u0, int u1, int cnt, bool vec) {
    const int hw = L.h * L.w;
    Taps t[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) t[j] = taps_of<KIND == BIU_AUGF_IMAGE>(L, P, x0 + j, y);
    const int inp = y * L.w + x0;
    if (KIND == BIU_AUGF_VECTOR) {
        const int pair = L.depth * hw, field = 2 * L.units * hw;
        for (int u = u0; u < u1; ++u) {
            const int j2 = u / L.depth, z = u - j2 * L.depth;
            const int base = s * field + (2 * j2 * L.depth + z) * hw;        // the cos plane; the sin plane is `pair` further
            float c[PX], sn[PX];
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const float a = tap(L, base, t[j].o00), b = tap(L, base + pair, t[j].o00);
                c[j] = a * P.cos_t + b * P.sin_t;
                sn[j] = b * P.cos_t - a * P.sin_t;
            }
            store<PX>(L.dst + base + inp, c, cnt, vec);
            store<PX>(L.dst + base + pair + inp, sn, cnt, vec);
        }
    } else {
        const int field = L.units * hw;
        const bool noisy = KIND == BIU_AUGF_IMAGE && (P.flags & (BIU_AUGF_SHOT | BIU_AUGF_GAUSS)) != 0;
        const bool has_bc = KIND == BIU_AUGF_IMAGE && (P.flags & BIU_AUGF_BC) != 0;
        for (int u = u0; u < u1; ++u) {
            const int base = s * field + u * hw;
            float v[PX];
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                if (KIND == BIU_AUGF_IMAGE) {
                    v[j] = bilinear(L, t[j], base);
                    if (has_bc) v[j] = bc(P, v[j]);
                    if (noisy && j < cnt) v[j] = shot_gauss(L, P, v[j], (uint32_t)(u * hw + inp + j));
                } else {
                    v[j] = tap(L, base, t[j].o00);
                }
            }
            store<PX>(L.dst + base + inp, v, cnt, vec);
        }
    }
}

// grid covers n x nchunks x (pixel groups of a plane); PX = 4: w % 4 == 0 and dst is 16-byte aligned, a lane's pixels lie in one row
template <int KIND, int PX>
__global__ __launch_bounds__(TPB) void k_augv_point(Launch L, int groups_per_plane, int total) {
    const int g = blockIdx.x * TPB + threadIdx.x;
    if (g >= total) return;
    const int lp = g % groups_per_plane, rest = g / groups_per_plane;
    const int ch = rest % L.nchunks, s = rest / L.nchunks;
    const int gw = L.w / PX;                                   // groups per row
    const int y = lp / gw, x0 = (lp - y * gw) * PX;
    const biu_augf_params P = L.params[s];
    walk<KIND, PX>(L, P, s, x0, y, ch * L.chunk, min((ch + 1) * L.chunk, L.units), PX, PX == 4);
}

// IMAGE fields of a batch in which at least one sample blurs; grid = n * nchunks * tiles_y * tiles_x
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
    const bool vec4 = (L.w & 3) == 0 && ((uintptr_t)L.dst % 16) == 0;

    if (!(P.flags & BIU_AUGF_BLUR)) {
        // this sample does not blur: a lane owns 4 consecutive pixels, 16 lanes one 256-byte row segment, and walks the planes
        for (int i = threadIdx.x; i < TILE * TILE / 4; i += TPB) {
            const int y = ty0 + i / (TILE / 4), x0 = tx0 + (i % (TILE / 4)) * 4;
            if (y >= L.h || x0 >= L.w) continue;
            walk<BIU_AUGF_IMAGE, 4>(L, P, s, x0, y, u0, u1, min(4, L.w - x0), vec4);
        }
        return;
    }
    const int k = min((int)P.blur_k | 1, BIU_AUG_MAX_BLUR), r = k >> 1;      // odd, <= 15: the halo fits the LDS tile whatever the record holds
    const int iw = TILE + 2 * r, ih = TILE + 2 * r;
    const bool has_bc = (P.flags & BIU_AUGF_BC) != 0, noisy = (P.flags & (BIU_AUGF_SHOT | BIU_AUGF_GAUSS)) != 0;
    const float inv = 1.f / (float)(k * k);
    for (int u = u0; u < u1; ++u) {
        const int base = s * field + u * hw;
        // 1. BC(gather) of the tile plus halo; an LDS pixel outside the plane is the reflect-101 of the output plane (cv2.blur's border)
        for (int i = threadIdx.x; i < ih * iw; i += TPB) {
            const int ly = i / iw, lx = i - ly * iw;
            const Taps t = taps_of<true>(L, P, reflect(tx0 - r + lx, L.w), reflect(ty0 - r + ly, L.h));
            const float v = bilinear(L, t, base);
            s_in[ly * IN_PITCH + lx] = has_bc ? bc(P, v) : v;
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
        // 3. sums of k row sums along y, four pixels per lane (16-byte LDS reads of consecutive lanes), mean, the noise stages, store
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
                if (noisy && j < cnt) a[j] = shot_gauss(L, P, a[j], (uint32_t)(u * hw + y * L.w + x0 + j));
            }
            store<4>(L.dst + base + y * L.w + x0, a, cnt, vec4);
        }
        // the next plane's step 1 writes s_in, which no lane reads after the barrier behind step 2; its step 2 writes s_h only behind the
        // barrier that follows step 1, by when every lane has left this step 3
    }
}

template <int KIND>
void launch_point(const Launch& L, bool rows, hipStream_t st) {
    const int gpp = rows ? L.h * (L.w / 4) : L.h * L.w;
    const int total = L.n * L.nchunks * gpp;                    // at most the elements of the batch field: below 2^31
    const int grid = total / TPB + (total % TPB != 0);          // not (total + TPB - 1) / TPB, which leaves int just below 2^31
    if (rows) hipLaunchKernelGGL((k_augv_point<KIND, 4>), dim3(grid), dim3(TPB), 0, st, L, gpp, total);
    else hipLaunchKernelGGL((k_augv_point<KIND, 1>), dim3(grid), dim3(TPB), 0, st, L, gpp, total);
}

// How a launch is cut is decided in one place for the launch, for biu_augment_vol_chunk and for biu_augment_vol_f32_crop:
// biu_augment_vol_plan.h.
bool dims_ok(int n, int channels, int depth, int h, int w, int kind, int max_blur_k) {
    return n > 0 && channels > 0 && depth > 0 && h > 0 && w > 0 && (double)n * channels * depth * h * w < 2147483648.0 &&
           (kind == BIU_AUGF_IMAGE || kind == BIU_AUGF_MASK || (kind == BIU_AUGF_VECTOR && channels % 2 == 0)) && max_blur_k >= 0 &&
           max_blur_k <= BIU_AUG_MAX_BLUR;
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
    BIU_REQUIRE(kind == BIU_AUGF_IMAGE || kind == BIU_AUGF_MASK || kind == BIU_AUGF_VECTOR, BIU_ERR_UNSUPPORTED, "augment_vol_f32: unknown kind %d", kind);
    BIU_REQUIRE(border == BIU_AUGV_REFLECT || border == BIU_AUGV_CONSTANT, BIU_ERR_UNSUPPORTED, "augment_vol_f32: unknown border %d", border);
    BIU_REQUIRE(kind != BIU_AUGF_VECTOR || channels % 2 == 0, BIU_ERR_SHAPE, "augment_vol_f32: a vector field has (c, s) channel pairs, got %d channels",
                channels);
    BIU_REQUIRE(((uintptr_t)dst % 4) == 0 && (src_is_u8 || ((uintptr_t)src % 4) == 0), BIU_ERR_SHAPE, "augment_vol_f32: unaligned float pointer");
    BIU_REQUIRE(max_blur_k >= 0 && max_blur_k <= BIU_AUG_MAX_BLUR, BIU_ERR_UNSUPPORTED, "augment_vol_f32: blur kernel %d exceeds %d", max_blur_k,
                BIU_AUG_MAX_BLUR);
    BIU_REQUIRE(field_id < (1u << 28), BIU_ERR_SHAPE, "augment_vol_f32: field_id needs 28 bits at most");
    const Plan p = plan_of(n, channels, depth, h, w, kind, max_blur_k, ((uintptr_t)dst % 16) == 0);
    const Launch L{src, dst, params, src_is_u8 != 0, border == BIU_AUGV_CONSTANT, n, p.units, h, w, depth, p.chunk, p.nchunks, (uint32_t)seed,
                   (uint32_t)(seed >> 32), epoch, field_id << 4};
    hipStream_t st = (hipStream_t)stream;
    if (p.tile) hipLaunchKernelGGL(k_augv_tile, dim3(n * p.nchunks * p.tx * p.ty), dim3(TPB), 0, st, L, p.tx, p.ty);
    else if (kind == BIU_AUGF_IMAGE) launch_point<BIU_AUGF_IMAGE>(L, p.rows, st);
    else if (kind == BIU_AUGF_MASK) launch_point<BIU_AUGF_MASK>(L, p.rows, st);
    else launch_point<BIU_AUGF_VECTOR>(L, p.rows, st);
    BIU_CHECK_LAUNCH("augment_vol_f32");
    return BIU_OK;
}
