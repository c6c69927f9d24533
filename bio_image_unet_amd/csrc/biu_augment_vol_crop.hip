// Crop augmentation of whole volumes on the device: the 3-D multi-output family's pipeline (multi_output_unet3d/data.py:152-230:
// ShiftScaleRotate of the whole volume, then RandomCrop3D(dim_out)) rendered straight from an arena of whole volumes
// (feed.VolumeStore.to_device), one launch per field and batch.  The sibling of biu_augment_vol.hip: the record (biu_augf_params), the kinds,
// the stages, the samplers, the Philox counter, the borders and the arithmetic are that file's, so that a crop of a whole item equals that
// kernel's output bit for bit (include/biu.h, "equivalence law").  What differs is the source: every sample names its item in the arena
// (biu_augv_source: element offset, d, h, w, first z-plane), m maps an OUTPUT TILE pixel to a coordinate in that item's (h, w) plane, the
// output extent (td, th, tw) is not the item's, and NaN in a target means "no label": dst never holds NaN.
//
// Index math inside an item is 32-bit (channels * d * h * w < 2^31 - 4 is the store's guard, and checked again per sample here); the item
// base is added to the arena pointer as a 64-bit offset.  A sample whose source does not describe a part of the arena that holds the crop's
// z-planes is rendered as nan_to_val: the kernel never reads outside [arena, arena + arena_elems).
//
// The two kernels and the cut of a launch are biu_augment_vol.hip's (biu_augment_vol_plan.h, planned from the OUTPUT shape):
//   k_augvc_point : a lane owns 4 consecutive output pixels of one row (1 where rows are no multiple of 4), computes their taps in the item's
//                   plane once and walks a chunk of the channels x td output planes with them.
//   k_augvc_tile  : some sample blurs: a block owns a 64 x 64 output tile and a chunk of planes.  Halo pixels outside the OUTPUT tile extent
//                   th x tw are its reflect-101 (cv2.blur on the cropped patch), not more gathered volume.
// The helpers below restate biu_augment_vol.hip's on purpose, line by line, with the item's extent where that file has the launch's.
// No atomics, no scratch.
#include <hip/hip_runtime.h>

#include "biu_common.h"
#include "biu_augment_stages.h"
#include "biu_augment_vol_plan.h"

namespace {
using biu_augment_stages::clip01;
using biu_augment_stages::shot_gauss;
using biu_augment_stages::source_of;
using biu_augment_vol_plan::Plan;
using biu_augment_vol_plan::plan_of;
using biu_augment_vol_plan::TILE;
using biu_augment_vol_plan::TPB;

constexpr int RMAX = BIU_AUG_MAX_BLUR / 2;      // 7
constexpr int IN_MAX = TILE + 2 * RMAX;         // 78 rows / columns of BC(gather)
constexpr int IN_PITCH = 80;

struct Launch {
    const void* arena;
    float* dst;
    const biu_augf_params* params;
    const biu_augv_source* sources;
    unsigned long long arena_elems;
    int u8;                    // the arena holds bytes
    int constant;              // border: taps outside the item's plane read 0
    int n, channels, units;    // units: OUTPUT planes a lane may walk (channels x td; VECTOR: pairs x td)
    int td, th, tw;
    int chunk, nchunks;        // planes per lane / block, and how many such chunks cover `units`
    float nan_to_val;
    uint32_t k0, k1;           // Philox key: the 64-bit seed
    uint32_t epoch, c3;        // counter words 2 and 3 (c3 = field_id * 16, the stage id is added)
};

// one sample's item: its first element, its extent and the crop's first z-plane; !ok: the source record does not describe a part of the
// arena that holds the crop
struct Item {
    const void* base;
    int d, h, w, hw, z0;
    bool ok;
};
__device__ __forceinline__ Item item_of(const Launch& L, int s) {
    const biu_augv_source S = L.sources[s];
    Item it;
    it.d = S.d;
    it.h = S.h;
    it.w = S.w;
    it.z0 = S.z0;
    // no product below leaves 64 bits: d h < 2^62, and only a volume below 2^31 voxels is multiplied by the channels
    const i64 dh = (i64)S.d * (i64)S.h, lim = (i64)1 << 31;
    const bool fits = S.d > 0 && S.h > 0 && S.w > 0 && dh < lim && dh * (i64)S.w < lim;
    const i64 elems = fits ? (i64)L.channels * (dh * (i64)S.w) : lim;
    it.ok = fits && elems < lim - 4 && S.z0 >= 0 && (i64)S.z0 + L.td <= (i64)S.d && S.offset <= L.arena_elems &&
            (unsigned long long)elems <= L.arena_elems - S.offset;
    it.hw = it.ok ? S.h * S.w : 0;
    it.base = L.u8 ? (const void*)(static_cast<const uint8_t*>(L.arena) + S.offset) : (const void*)(static_cast<const float*>(L.arena) + S.offset);
    return it;
}
__device__ __forceinline__ float load(const Launch& L, const Item& it, int i) {
    return L.u8 ? (float)static_cast<const uint8_t*>(it.base)[i] / 255.0f : static_cast<const float*>(it.base)[i];
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
__device__ __forceinline__ int offset_of(const Launch& L, const Item& it, int ix, int iy) {
    const int bx = border(L, ix, it.w), by = border(L, iy, it.h);
    return (bx | by) < 0 ? -1 : by * it.w + bx;
}
__device__ __forceinline__ float tap(const Launch& L, const Item& it, int base, int off) { return off < 0 ? 0.f : load(L, it, base + off); }
// product and sum rounded one after the other: the fp32 formula, not a fused multiply-add
__device__ __forceinline__ float bc(const biu_augf_params& P, float v) {
#pragma clang fp contract(off)
    const float m = v * P.alpha;
    return clip01(m + P.beta);
}

// (c, s) -> (c cos_t + s sin_t, s cos_t - c sin_t), written out with the roundings biu_augment_vol.hip's expression gets from the compiler's
// contraction (the first product of each sum is fused, the second rounded), so that the equivalence law holds bit for bit whatever else
// surrounds the expression here; tests/test_gpu_augment_vol_crop.py holds the two kernels to each other.
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

// PX output pixels (x0 .. x0 + cnt - 1, y) of sample s through the OUTPUT planes u0 .. u1 - 1; no blur here.  An output plane u = (c, z)
// reads plane (c, z0 + z) of the item.
template <int KIND, int PX>
__device__ __forceinline__ void walk(const Launch& L, const biu_augf_params& P, const Item& it, int s, int x0, int y, int u0, int u1, int cnt, bool vec) {
    const int thw = L.th * L.tw;
    const int inp = y * L.tw + x0;
    const int field = (KIND == BIU_AUGF_VECTOR ? 2 : 1) * L.units * thw;         // elements of one output sample
    float* out = L.dst + s * field + inp;
    if (!it.ok) {
        float v[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) v[j] = L.nan_to_val;
        if (KIND == BIU_AUGF_VECTOR) {
            for (int u = u0; u < u1; ++u) {
                const int j2 = u / L.td, z = u - j2 * L.td;
                store<PX>(out + (2 * j2 * L.td + z) * thw, v, cnt, vec);
                store<PX>(out + ((2 * j2 + 1) * L.td + z) * thw, v, cnt, vec);
            }
        } else {
            for (int u = u0; u < u1; ++u) store<PX>(out + u * thw, v, cnt, vec);
        }
        return;
    }
    Taps t[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) t[j] = taps_of<KIND == BIU_AUGF_IMAGE>(L, it, P, x0 + j, y);
    if (KIND == BIU_AUGF_VECTOR) {
        const int pair_in = it.d * it.hw, pair_out = L.td * thw;
        for (int u = u0; u < u1; ++u) {
            const int j2 = u / L.td, z = u - j2 * L.td;
            const int base = (2 * j2 * it.d + it.z0 + z) * it.hw;                // the cos plane; the sin plane is `pair_in` further
            float c[PX], sn[PX];
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const float a = tap(L, it, base, t[j].o00), b = tap(L, it, base + pair_in, t[j].o00);
                rotate(P, a, b, c[j], sn[j]);
                if (a != a || b != b) c[j] = sn[j] = L.nan_to_val;               // no label in either plane: no label in both
            }
            float* o = out + (2 * j2 * L.td + z) * thw;
            store<PX>(o, c, cnt, vec);
            store<PX>(o + pair_out, sn, cnt, vec);
        }
    } else {
        const bool noisy = KIND == BIU_AUGF_IMAGE && (P.flags & (BIU_AUGF_SHOT | BIU_AUGF_GAUSS)) != 0;
        const bool has_bc = KIND == BIU_AUGF_IMAGE && (P.flags & BIU_AUGF_BC) != 0;
        for (int u = u0; u < u1; ++u) {
            const int c = u / L.td, z = u - c * L.td;
            const int base = (c * it.d + it.z0 + z) * it.hw;
            float v[PX];
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                if (KIND == BIU_AUGF_IMAGE) {
                    v[j] = bilinear(L, it, t[j], base);
                    if (has_bc) v[j] = bc(P, v[j]);
                    if (noisy && j < cnt) v[j] = shot_gauss(L, P, v[j], (uint32_t)(u * thw + inp + j));
                } else {
                    v[j] = tap(L, it, base, t[j].o00);
                    if (v[j] != v[j]) v[j] = L.nan_to_val;
                }
            }
            store<PX>(out + u * thw, v, cnt, vec);
        }
    }
}

// grid covers n x nchunks x (pixel groups of an output plane); PX = 4: tw % 4 == 0 and dst is 16-byte aligned, a lane's pixels lie in one row
template <int KIND, int PX>
__global__ __launch_bounds__(TPB) void k_augvc_point(Launch L, int groups_per_plane, int total) {
    const int g = blockIdx.x * TPB + threadIdx.x;
    if (g >= total) return;
    const int lp = g % groups_per_plane, rest = g / groups_per_plane;
    const int ch = rest % L.nchunks, s = rest / L.nchunks;
    const int gw = L.tw / PX;                                  // groups per row
    const int y = lp / gw, x0 = (lp - y * gw) * PX;
    const biu_augf_params P = L.params[s];
    const Item it = item_of(L, s);
    walk<KIND, PX>(L, P, it, s, x0, y, ch * L.chunk, min((ch + 1) * L.chunk, L.units), PX, PX == 4);
}

// IMAGE fields of a batch in which at least one sample blurs; grid = n * nchunks * tiles_y * tiles_x
__global__ __launch_bounds__(TPB) void k_augvc_tile(Launch L, int tiles_x, int tiles_y) {
    __shared__ __attribute__((aligned(16))) float s_in[IN_MAX * IN_PITCH];     // 24 960 B
    __shared__ __attribute__((aligned(16))) float s_h[IN_MAX * TILE];          // 19 968 B
    int b = blockIdx.x;
    const int tx0 = (b % tiles_x) * TILE;
    b /= tiles_x;
    const int ty0 = (b % tiles_y) * TILE;
    b /= tiles_y;
    const int ch = b % L.nchunks, s = b / L.nchunks;
    const int u0 = ch * L.chunk, u1 = min(u0 + L.chunk, L.units);
    const int thw = L.th * L.tw, field = L.units * thw;
    const biu_augf_params P = L.params[s];
    const Item it = item_of(L, s);
    const bool vec4 = (L.tw & 3) == 0 && ((uintptr_t)L.dst % 16) == 0;

    if (!(P.flags & BIU_AUGF_BLUR) || !it.ok) {
        // this sample does not blur: a lane owns 4 consecutive pixels, 16 lanes one 256-byte row segment, and walks the planes
        for (int i = threadIdx.x; i < TILE * TILE / 4; i += TPB) {
            const int y = ty0 + i / (TILE / 4), x0 = tx0 + (i % (TILE / 4)) * 4;
            if (y >= L.th || x0 >= L.tw) continue;
            walk<BIU_AUGF_IMAGE, 4>(L, P, it, s, x0, y, u0, u1, min(4, L.tw - x0), vec4);
        }
        return;
    }
    const int k = min((int)P.blur_k | 1, BIU_AUG_MAX_BLUR), r = k >> 1;      // odd, <= 15: the halo fits the LDS tile whatever the record holds
    const int iw = TILE + 2 * r, ih = TILE + 2 * r;
    const bool has_bc = (P.flags & BIU_AUGF_BC) != 0, noisy = (P.flags & (BIU_AUGF_SHOT | BIU_AUGF_GAUSS)) != 0;
    const float inv = 1.f / (float)(k * k);
    for (int u = u0; u < u1; ++u) {
        const int c = u / L.td, z = u - c * L.td;
        const int base = (c * it.d + it.z0 + z) * it.hw;
        float* out = L.dst + s * field + u * thw;
        // 1. BC(gather) of the tile plus halo; an LDS pixel outside the OUTPUT tile extent is its reflect-101 (cv2.blur on the cropped patch)
        for (int i = threadIdx.x; i < ih * iw; i += TPB) {
            const int ly = i / iw, lx = i - ly * iw;
            const Taps t = taps_of<true>(L, it, P, reflect(tx0 - r + lx, L.tw), reflect(ty0 - r + ly, L.th));
            const float v = bilinear(L, it, t, base);
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
                if (noisy && j < cnt) a[j] = shot_gauss(L, P, a[j], (uint32_t)(u * thw + y * L.tw + x0 + j));
            }
            store<4>(out + y * L.tw + x0, a, cnt, vec4);
        }
        // the next plane's step 1 writes s_in, which no lane reads after the barrier behind step 2; its step 2 writes s_h only behind the
        // barrier that follows step 1, by when every lane has left this step 3
    }
}

template <int KIND>
void launch_point(const Launch& L, bool rows, hipStream_t st) {
    const int gpp = rows ? L.th * (L.tw / 4) : L.th * L.tw;
    const int total = L.n * L.nchunks * gpp;                    // at most the elements of the output: below 2^31
    const int grid = total / TPB + (total % TPB != 0);
    if (rows) hipLaunchKernelGGL((k_augvc_point<KIND, 4>), dim3(grid), dim3(TPB), 0, st, L, gpp, total);
    else hipLaunchKernelGGL((k_augvc_point<KIND, 1>), dim3(grid), dim3(TPB), 0, st, L, gpp, total);
}

// do [a, a + na) and [b, b + nb) share a byte
bool overlap(const void* a, unsigned long long na, const void* b, unsigned long long nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}
}  // namespace

extern "C" int biu_augment_vol_f32_crop(const void* arena, int arena_is_u8, unsigned long long arena_elems, float* dst, int n, int channels, int td,
                                        int th, int tw, int kind, int border, const biu_augf_params* params, const biu_augv_source* sources,
                                        float nan_to_val, int max_blur_k, unsigned long long seed, unsigned epoch, unsigned field_id,
                                        biu_stream stream) {
    BIU_REQUIRE(arena && dst && params && sources && arena_elems > 0 && n > 0 && channels > 0 && td > 0 && th > 0 && tw > 0, BIU_ERR_SHAPE,
                "augment_vol_f32_crop: bad arguments");
    BIU_REQUIRE((double)n * channels * td * th * tw < 2147483648.0, BIU_ERR_SHAPE, "augment_vol_f32_crop: the output has 2^31 elements or more");
    BIU_REQUIRE(arena_elems < (1ull << 62), BIU_ERR_SHAPE, "augment_vol_f32_crop: arena_elems out of range");
    BIU_REQUIRE(kind == BIU_AUGF_IMAGE || kind == BIU_AUGF_MASK || kind == BIU_AUGF_VECTOR, BIU_ERR_UNSUPPORTED, "augment_vol_f32_crop: unknown kind %d",
                kind);
    BIU_REQUIRE(border == BIU_AUGV_REFLECT || border == BIU_AUGV_CONSTANT, BIU_ERR_UNSUPPORTED, "augment_vol_f32_crop: unknown border %d", border);
    BIU_REQUIRE(kind != BIU_AUGF_VECTOR || channels % 2 == 0, BIU_ERR_SHAPE,
                "augment_vol_f32_crop: a vector field has (c, s) channel pairs, got %d channels", channels);
    BIU_REQUIRE(((uintptr_t)dst % 4) == 0 && (arena_is_u8 || ((uintptr_t)arena % 4) == 0), BIU_ERR_SHAPE, "augment_vol_f32_crop: unaligned float pointer");
    BIU_REQUIRE(((uintptr_t)params % 8) == 0 && ((uintptr_t)sources % 8) == 0, BIU_ERR_SHAPE, "augment_vol_f32_crop: unaligned record pointer");
    BIU_REQUIRE(nan_to_val == nan_to_val, BIU_ERR_SHAPE, "augment_vol_f32_crop: nan_to_val is NaN");
    const unsigned long long arena_bytes = arena_elems * (arena_is_u8 ? 1ull : 4ull), dst_bytes = (unsigned long long)n * channels * td * th * tw * 4ull;
    const unsigned long long par_bytes = (unsigned long long)n * sizeof(biu_augf_params), src_bytes = (unsigned long long)n * sizeof(biu_augv_source);
    BIU_REQUIRE(!overlap(dst, dst_bytes, arena, arena_bytes) && !overlap(dst, dst_bytes, params, par_bytes) && !overlap(dst, dst_bytes, sources, src_bytes),
                BIU_ERR_SHAPE, "augment_vol_f32_crop: dst must not overlap the arena or the records");
    BIU_REQUIRE(max_blur_k >= 0 && max_blur_k <= BIU_AUG_MAX_BLUR, BIU_ERR_UNSUPPORTED, "augment_vol_f32_crop: blur kernel %d exceeds %d", max_blur_k,
                BIU_AUG_MAX_BLUR);
    BIU_REQUIRE(field_id < (1u << 28), BIU_ERR_SHAPE, "augment_vol_f32_crop: field_id needs 28 bits at most");
    const Plan p = plan_of(n, channels, td, th, tw, kind, max_blur_k, ((uintptr_t)dst % 16) == 0);
    const Launch L{arena, dst, params, sources, arena_elems, arena_is_u8 != 0, border == BIU_AUGV_CONSTANT, n, channels, p.units, td, th, tw,
                   p.chunk, p.nchunks, nan_to_val, (uint32_t)seed, (uint32_t)(seed >> 32), epoch, field_id << 4};
    hipStream_t st = (hipStream_t)stream;
    if (p.tile) hipLaunchKernelGGL(k_augvc_tile, dim3(n * p.nchunks * p.tx * p.ty), dim3(TPB), 0, st, L, p.tx, p.ty);
    else if (kind == BIU_AUGF_IMAGE) launch_point<BIU_AUGF_IMAGE>(L, p.rows, st);
    else if (kind == BIU_AUGF_MASK) launch_point<BIU_AUGF_MASK>(L, p.rows, st);
    else launch_point<BIU_AUGF_VECTOR>(L, p.rows, st);
    BIU_CHECK_LAUNCH("augment_vol_f32_crop");
    return BIU_OK;
}
