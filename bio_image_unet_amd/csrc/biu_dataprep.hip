// Training data preparation on the device: what is left of the reference's DataProcess (unet/data.py:124-215, unet3d/data.py:116-207,
// siam_unet/data.py:126-233) once augmentation runs on the fly -- the mask edit and the mask half of the tile split.  The image half
// (percentile normalisation to bytes and its tile gather) is biu_prep.hip.
//
//   biu_lut_u8          every pointwise step of the mask edit as one 256-entry table
//   biu_morph_u8        grey erosion / dilation, disk(r <= 7) or square(w <= 15), scipy.ndimage's 'reflect' border and even-footprint rule
//   biu_thin_step_u8    one sub-iteration of Zhang-Suen thinning through a 256-entry neighbourhood table; counts what it cleared
//   biu_tile_gather_u8  tiles of a uint8 stack with numpy 'reflect' beyond the far end, optional 255 - v
//
// Everything is integer arithmetic on bytes: there is no rounding anywhere, the tests compare with array_equal.
//
// Layout shared by the two stencil kernels: a block of 256 threads owns a tile of 32 rows x 128 columns.  The tile and its halo sit in LDS
// as rows of dwords; the column halo is a fixed 8 bytes (morphology) or 4 bytes (thinning) on either side so that the lane's own four
// pixels are one aligned dword.  Lane (lx, ly) = (tid & 31, tid >> 5) computes the four pixels of dword lx in rows 4 ly .. 4 ly + 3: the
// 32 lanes of a wave half read 32 consecutive dwords of one LDS row -- consecutive banks, no conflict -- and an input row loaded once
// serves all four output rows.  Rows reach the plane as one dword store per lane where the width keeps dwords aligned, else as bytes.
#include <hip/hip_runtime.h>

#include "biu_common.h"
#include "biu_internal.h"

namespace {
constexpr int TPB = 256;
constexpr int TW = 128, TH = 32;                 // tile of a block
constexpr int MAXR = 7;                          // largest footprint offset on either side
constexpr int M_PADB = 8;                        // morphology: bytes of column halo on either side (>= MAXR, a multiple of 4)
constexpr int M_STRIDE = (TW + 2 * M_PADB) / 4;  // 36 dwords per LDS row
constexpr int M_ROWS = TH + 2 * MAXR;            // 46
constexpr int T_STRIDE = (TW + 8) / 4;           // thinning: 4 bytes of halo on either side, 34 dwords
constexpr int T_ROWS = TH + 2;

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

// scipy.ndimage mode='reflect' (numpy 'symmetric'): the edge pixel repeated, period 2 n, folded as often as it takes
__device__ inline int reflect_edge(int i, int n) {
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}
// numpy 'reflect' (no edge repeat), the rule of biu_prep_tiles
__device__ inline int reflect_idx(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

__global__ __launch_bounds__(TPB) void k_lut_u8(const uint8_t* __restrict__ src, const uint8_t* __restrict__ lut, uint8_t* __restrict__ dst, i64 n) {
    __shared__ uint8_t tab[256];
    tab[threadIdx.x] = lut[threadIdx.x];         // TPB == 256
    __syncthreads();
    const bool vec = ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0;
    const i64 nv = vec ? n / 16 : 0;
    const i64 t0 = (i64)blockIdx.x * TPB + threadIdx.x, step = (i64)gridDim.x * TPB;
    for (i64 v = t0; v < nv; v += step) {
        union { uint4 q; uint8_t e[16]; } u;
        u.q = ((const uint4*)src)[v];
#pragma unroll
        for (int j = 0; j < 16; ++j) u.e[j] = tab[u.e[j]];
        ((uint4*)dst)[v] = u.q;
    }
    for (i64 i = nv * 16 + t0; i < n; i += step) dst[i] = tab[src[i]];
}

// Footprint: rows dy in [-up, down]; row dy spans dx in [-l, r] with l and r the nibbles (dy + 7) of lbits and rbits.
struct Foot {
    unsigned long long lbits, rbits;
    int up, down;
};

template <int OP>   // 0: minimum, 1: maximum
__global__ __launch_bounds__(TPB) void k_morph_u8(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W, Foot f) {
    __shared__ uint32_t tile[M_ROWS * M_STRIDE];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const uint8_t* sp = src + (i64)blockIdx.z * H * W;
    uint8_t* dp = dst + (i64)blockIdx.z * H * W;
    const bool aligned = (W & 3) == 0 && (((uintptr_t)src) & 3) == 0;
    const int rows = TH + f.up + f.down;         // LDS row j holds plane row y0 - up + j; dword c holds columns x0 - 8 + 4 c ..
    for (int i = tid; i < rows * M_STRIDE; i += TPB) {
        const int j = i / M_STRIDE, c = i - j * M_STRIDE;
        const int gy = reflect_edge(y0 - f.up + j, H), gx = x0 - M_PADB + 4 * c;
        const uint8_t* row = sp + (i64)gy * W;
        uint32_t v;
        if (aligned && gx >= 0 && gx + 3 < W) {
            v = *(const uint32_t*)(row + gx);
        } else {
            v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) v |= (uint32_t)row[reflect_edge(gx + b, W)] << (8 * b);
        }
        tile[i] = v;
    }
    __syncthreads();

    const int lx = tid & 31, ly = tid >> 5;
    const uint32_t init = OP == 0 ? 0x00ff00ffu : 0u;
    uint32_t ev[4], od[4];                       // bytes 0, 2 and bytes 1, 3 of the four output pixels, one 16-bit field each
#pragma unroll
    for (int o = 0; o < 4; ++o) ev[o] = od[o] = init;
    auto fold = [](uint32_t a, uint32_t b) -> uint32_t {
        const us2 x = __builtin_bit_cast(us2, a), y = __builtin_bit_cast(us2, b);
        return __builtin_bit_cast(uint32_t, OP == 0 ? __builtin_elementwise_min(x, y) : __builtin_elementwise_max(x, y));
    };
    for (int rr = 0; rr < 4 + f.up + f.down; ++rr) {        // input row 4 ly - up + rr of the tile
        const uint32_t* w = tile + (4 * ly + rr) * M_STRIDE + lx;      // bytes: columns 4 lx - 8 .. 4 lx + 11 of the lane's pixels 0 .. 3
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
        uint32_t mask[4];                        // per output row: bit (dx + 7) = offset dx of footprint row dy = rr - up - o
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int dy = rr - f.up - o;
            mask[o] = 0;
            if (dy >= -f.up && dy <= f.down) {
                const int l = (int)((f.lbits >> (4 * (dy + 7))) & 15), r = (int)((f.rbits >> (4 * (dy + 7))) & 15);
                mask[o] = ((1u << (l + r + 1)) - 1u) << (7 - l);
            }
        }
        const uint32_t any = mask[0] | mask[1] | mask[2] | mask[3];
#pragma unroll
        for (int dx = -MAXR; dx <= MAXR; ++dx) {
            if (!((any >> (dx + 7)) & 1u)) continue;        // block-uniform
            constexpr int base = M_PADB;                     // byte of pixel 0 inside w0..w4
            const int k = (base + dx) >> 2, s = (base + dx) & 3;
            const uint32_t lo = k == 0 ? w0 : k == 1 ? w1 : k == 2 ? w2 : w3;
            const uint32_t hi = k == 0 ? w1 : k == 1 ? w2 : k == 2 ? w3 : w4;
            const uint32_t u = s == 0 ? lo : __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)s);       // pixels 0..3 shifted by dx
            const uint32_t e = u & 0x00ff00ffu, q = (u >> 8) & 0x00ff00ffu;
#pragma unroll
            for (int o = 0; o < 4; ++o)
                if ((mask[o] >> (dx + 7)) & 1u) { ev[o] = fold(ev[o], e); od[o] = fold(od[o], q); }
        }
    }
    const int x = x0 + 4 * lx;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int y = y0 + 4 * ly + o;
        if (y >= H || x >= W) continue;
        const uint32_t v = ev[o] | (od[o] << 8);
        uint8_t* out = dp + (i64)y * W + x;
        if ((W & 3) == 0 && (((uintptr_t)dst) & 3) == 0) {
            *(uint32_t*)out = v;
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (x + b < W) out[b] = (uint8_t)(v >> (8 * b));
        }
    }
}

__device__ inline uint32_t nonzero_bytes(uint32_t w) {       // 1 in every byte that is not 0
    return ((w | ((w & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u;
}

__global__ __launch_bounds__(TPB) void k_thin_step_u8(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W, int sub,
                                                      const uint8_t* __restrict__ table, unsigned long long* __restrict__ cleared) {
    __shared__ uint32_t tile[T_ROWS * T_STRIDE];
    __shared__ uint8_t tab[256];
    __shared__ uint32_t count;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const uint8_t* sp = src + (i64)blockIdx.z * H * W;
    uint8_t* dp = dst + (i64)blockIdx.z * H * W;
    const bool aligned = (W & 3) == 0 && (((uintptr_t)src) & 3) == 0;
    tab[tid] = table[tid];                       // TPB == 256
    if (tid == 0) count = 0;
    for (int i = tid; i < T_ROWS * T_STRIDE; i += TPB) {    // LDS row j holds plane row y0 - 1 + j; dword c holds columns x0 - 4 + 4 c ..
        const int j = i / T_STRIDE, c = i - j * T_STRIDE;
        const int gy = y0 - 1 + j, gx = x0 - 4 + 4 * c;
        uint32_t v = 0;                          // outside the plane: 0
        if (gy >= 0 && gy < H) {
            const uint8_t* row = sp + (i64)gy * W;
            if (aligned && gx >= 0 && gx + 3 < W) {
                v = *(const uint32_t*)(row + gx);
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (gx + b >= 0 && gx + b < W) v |= (uint32_t)row[gx + b] << (8 * b);
            }
        }
        tile[i] = nonzero_bytes(v);
    }
    __syncthreads();

    const int lx = tid & 31, ly = tid >> 5;
    // strip of a row: byte k = column 4 lx - 1 + k of the lane's pixels, k = 0 .. 5 (left neighbour, the four pixels, right neighbour)
    auto strip = [&](int j) -> unsigned long long {
        const uint32_t* w = tile + j * T_STRIDE + lx;
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
        return (unsigned long long)__builtin_amdgcn_alignbyte(w1, w0, 3u) | ((unsigned long long)__builtin_amdgcn_alignbyte(w2, w1, 3u) << 32);
    };
    unsigned long long up = strip(4 * ly), mid = strip(4 * ly + 1);
    uint32_t gone = 0;
    const int x = x0 + 4 * lx;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const unsigned long long down = strip(4 * ly + o + 2);
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t p = (uint32_t)(mid >> (8 * (b + 1))) & 1u;
            // P2 = N, P3 = NE, P4 = E, P5 = SE, P6 = S, P7 = SW, P8 = W, P9 = NW in bits 0 .. 7
            const uint32_t code = ((uint32_t)(up >> (8 * (b + 1))) & 1u) | (((uint32_t)(up >> (8 * (b + 2))) & 1u) << 1) |
                                  (((uint32_t)(mid >> (8 * (b + 2))) & 1u) << 2) | (((uint32_t)(down >> (8 * (b + 2))) & 1u) << 3) |
                                  (((uint32_t)(down >> (8 * (b + 1))) & 1u) << 4) | (((uint32_t)(down >> (8 * b)) & 1u) << 5) |
                                  (((uint32_t)(mid >> (8 * b)) & 1u) << 6) | (((uint32_t)(up >> (8 * b)) & 1u) << 7);
            const uint32_t clr = p & (((uint32_t)tab[code] >> sub) & 1u);
            const int y = y0 + 4 * ly + o;
            gone += (y < H && x + b < W) ? clr : 0u;         // (outside the plane p is 0 anyway)
            v |= (p & ~clr) << (8 * b);
        }
        const int y = y0 + 4 * ly + o;
        if (y < H && x < W) {
            uint8_t* out = dp + (i64)y * W + x;
            if ((W & 3) == 0 && (((uintptr_t)dst) & 3) == 0) {
                *(uint32_t*)out = v;
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (x + b < W) out[b] = (uint8_t)(v >> (8 * b));
            }
        }
        up = mid;
        mid = down;
    }
    if (gone) atomicAdd(&count, gone);
    __syncthreads();
    if (tid == 0 && count) atomicAdd(cleared, (unsigned long long)count);
}

struct GatherGeo {
    int Z, D, H, W;          // planes in the source, planes per volume (z reflects inside its own volume), plane extent
    int td, th, tw, N;       // tile extent, tiles
    int invert;
};
// One thread per 16 output bytes along x, as k_prep_tiles: one 16-byte store where the row allows it.
__global__ __launch_bounds__(TPB) void k_tile_gather_u8(const uint8_t* __restrict__ src, const int* __restrict__ origins, GatherGeo g,
                                                        uint8_t* __restrict__ out) {
    constexpr int CH = 16;
    const int chunks = (g.tw + CH - 1) / CH;
    const i64 rows = (i64)g.N * g.td * g.th;
    const i64 total = rows * chunks;
    const bool vec_ok = g.tw % CH == 0 && ((uintptr_t)out & 15) == 0;
    const uint8_t flip = g.invert ? 0xff : 0x00;             // 255 - v == v ^ 255 on bytes
    for (i64 i = (i64)blockIdx.x * TPB + threadIdx.x; i < total; i += (i64)gridDim.x * TPB) {
        const int c = (int)(i % chunks);
        const i64 row = i / chunks;
        const int y = (int)(row % g.th);
        const int z = (int)((row / g.th) % g.td);
        const int t = (int)(row / ((i64)g.th * g.td));
        const int z0 = origins[t * 4 + 1], y0 = origins[t * 4 + 2], x0 = origins[t * 4 + 3];
        const int x_beg = c * CH, cnt = min(CH, g.tw - x_beg);
        const bool live = z0 >= 0 && z0 < g.Z && y0 >= 0 && x0 >= 0 && y0 < (1 << 30) && x0 < (1 << 30);      // else zeros
        union { uint4 q; uint8_t e[CH]; } u;
        u.q = make_uint4(0, 0, 0, 0);
        if (live) {
            const int vbase = z0 / g.D * g.D;
            const int sz = vbase + reflect_idx(z0 - vbase + z, g.D), sy = reflect_idx(y0 + y, g.H);
            const uint8_t* srow = src + ((i64)sz * g.H + sy) * g.W;
            const int xx = x0 + x_beg;
            if (cnt == CH && xx + CH <= g.W) {
                __builtin_memcpy(&u.q, srow + xx, CH);
            } else {
#pragma unroll
                for (int j = 0; j < CH; ++j)
                    if (j < cnt) u.e[j] = srow[reflect_idx(xx + j, g.W)];
            }
#pragma unroll
            for (int j = 0; j < CH; ++j) u.e[j] ^= flip;
        }
        uint8_t* dstp = out + row * g.tw + x_beg;
        if (vec_ok) {
            *(uint4*)dstp = u.q;
        } else {
#pragma unroll
            for (int j = 0; j < CH; ++j)
                if (j < cnt) dstp[j] = u.e[j];
        }
    }
}

inline bool plane_args_ok(int planes, int height, int width) {
    return planes >= 1 && planes <= 65535 && height >= 1 && width >= 1 && (height + TH - 1) / TH <= 65535 &&
           (long long)planes * height * width <= (1LL << 40);
}
}  // namespace

extern "C" int biu_lut_u8(const uint8_t* src, const uint8_t* lut, uint8_t* dst, long long n, biu_stream stream) {
    BIU_REQUIRE(src && lut && dst && n >= 1, BIU_ERR_SHAPE, "lut_u8: bad arguments");
    hipLaunchKernelGGL(k_lut_u8, dim3(grid_for((n + 15) / 16, TPB, 8192)), dim3(TPB), 0, (hipStream_t)stream, src, lut, dst, (i64)n);
    BIU_CHECK_LAUNCH("lut_u8");
    return BIU_OK;
}

extern "C" int biu_morph_u8(const uint8_t* src, uint8_t* dst, int planes, int height, int width, int op, int footprint, int size,
                            biu_stream stream) {
    BIU_REQUIRE(src && dst && src != dst, BIU_ERR_SHAPE, "morph_u8: null or aliased argument");
    BIU_REQUIRE(plane_args_ok(planes, height, width), BIU_ERR_SHAPE, "morph_u8: need 1 <= planes <= 65535 and a plane of at least 1 x 1");
    BIU_REQUIRE(op == BIU_MORPH_ERODE || op == BIU_MORPH_DILATE, BIU_ERR_UNSUPPORTED, "morph_u8: unknown operation %d", op);
    Foot f{0, 0, 0, 0};
    if (footprint == BIU_FOOT_DISK) {
        BIU_REQUIRE(size >= 1 && size <= MAXR, BIU_ERR_UNSUPPORTED, "morph_u8: disk(%d) is not supported (1 <= r <= %d)", size, MAXR);
        f.up = f.down = size;
        for (int dy = -size; dy <= size; ++dy) {
            int h = 0;
            while ((h + 1) * (h + 1) + dy * dy <= size * size) ++h;
            f.lbits |= (unsigned long long)h << (4 * (dy + 7));
            f.rbits |= (unsigned long long)h << (4 * (dy + 7));
        }
    } else if (footprint == BIU_FOOT_SQUARE) {
        BIU_REQUIRE(size >= 1 && size <= 2 * MAXR + 1, BIU_ERR_UNSUPPORTED, "morph_u8: square(%d) is not supported (1 <= w <= %d)", size,
                    2 * MAXR + 1);
        const int h = size / 2;
        int lo = h, hi = h;                                  // offsets [-lo, hi] per axis
        if (size % 2 == 0) {                                 // scipy.ndimage: erosion [-w/2, w/2 - 1], dilation [-(w/2 - 1), w/2]
            if (op == BIU_MORPH_ERODE) hi = h - 1;
            else lo = h - 1;
        }
        f.up = lo;
        f.down = hi;
        for (int dy = -lo; dy <= hi; ++dy) {
            f.lbits |= (unsigned long long)lo << (4 * (dy + 7));
            f.rbits |= (unsigned long long)hi << (4 * (dy + 7));
        }
    } else {
        return biu_fail(BIU_ERR_UNSUPPORTED, "morph_u8: unknown footprint %d", footprint);
    }
    const dim3 grid((unsigned)((width + TW - 1) / TW), (unsigned)((height + TH - 1) / TH), (unsigned)planes);
    if (op == BIU_MORPH_ERODE) hipLaunchKernelGGL(k_morph_u8<0>, grid, dim3(TPB), 0, (hipStream_t)stream, src, dst, height, width, f);
    else hipLaunchKernelGGL(k_morph_u8<1>, grid, dim3(TPB), 0, (hipStream_t)stream, src, dst, height, width, f);
    BIU_CHECK_LAUNCH("morph_u8");
    return BIU_OK;
}

extern "C" int biu_thin_step_u8(const uint8_t* src, uint8_t* dst, int planes, int height, int width, int sub, const uint8_t* table,
                                unsigned long long* cleared, biu_stream stream) {
    BIU_REQUIRE(src && dst && src != dst && table && cleared, BIU_ERR_SHAPE, "thin_step_u8: null or aliased argument");
    BIU_REQUIRE(plane_args_ok(planes, height, width), BIU_ERR_SHAPE, "thin_step_u8: need 1 <= planes <= 65535 and a plane of at least 1 x 1");
    BIU_REQUIRE(sub == 0 || sub == 1, BIU_ERR_SHAPE, "thin_step_u8: sub-iteration %d is not 0 or 1", sub);
    BIU_REQUIRE(((uintptr_t)cleared & 7) == 0, BIU_ERR_ALIGN, "thin_step_u8: misaligned counter");
    const dim3 grid((unsigned)((width + TW - 1) / TW), (unsigned)((height + TH - 1) / TH), (unsigned)planes);
    hipLaunchKernelGGL(k_thin_step_u8, grid, dim3(TPB), 0, (hipStream_t)stream, src, dst, height, width, sub, table, cleared);
    BIU_CHECK_LAUNCH("thin_step_u8");
    return BIU_OK;
}

extern "C" int biu_tile_gather_u8(const uint8_t* src, int planes, int depth, int height, int width, const int* origins, int ntiles, int td,
                                  int th, int tw, int invert, uint8_t* out, biu_stream stream) {
    BIU_REQUIRE(src && origins && out, BIU_ERR_SHAPE, "tile_gather_u8: null argument");
    BIU_REQUIRE(planes >= 1 && depth >= 1 && planes % depth == 0 && height >= 1 && width >= 1 && ntiles >= 1 && td >= 1 && th >= 1 && tw >= 1 &&
                    td <= (1 << 24) && th <= (1 << 24) && tw <= (1 << 24), BIU_ERR_SHAPE, "tile_gather_u8: bad extents");
    BIU_REQUIRE((long long)ntiles * 4 <= 0x7fffffffLL, BIU_ERR_SHAPE, "tile_gather_u8: too many tiles");
    const GatherGeo g{planes, depth, height, width, td, th, tw, ntiles, invert ? 1 : 0};
    const int grid = grid_for((i64)ntiles * td * th * ((tw + 15) / 16), TPB, 8192);
    hipLaunchKernelGGL(k_tile_gather_u8, dim3(grid), dim3(TPB), 0, (hipStream_t)stream, src, origins, g, out);
    BIU_CHECK_LAUNCH("tile_gather_u8");
    return BIU_OK;
}
