// What biu_augment_f32.hip (float fields) and biu_augment_vol.hip (float volumes) must compute alike, kept once: the fp64 source coordinate of
// an output pixel, and the shot and Gauss noise stages with their samplers and their Philox counter.  The contract of both kernels says the
// noise of the one is exactly the noise of the other (include/biu.h); tests/augment_f32_oracle.py restates it for both.
// `Launch` is either file's launch record; read here are its Philox key (k0, k1) and its counter words 2 and 3 (epoch, c3).
// Below the stages: what the two families (and biu_augment_cubic.hip) share although their gather, border rule, stage order and BC rounding
// differ by contract -- the u8/f32 load, wrap and reflect, the 4-pixel store, the box blur behind its gather, the host's overlap test.
#pragma once
#include "biu_common.h"
#include "biu_philox.h"

namespace biu_augment_stages {
// a source coordinate as an index-safe number whatever the parameter record holds (NaN -> the lower bound)
__device__ __forceinline__ double safe_coord(double v) { return fmin(fmax(v, -1.0e6), 1.0e6); }
__device__ __forceinline__ float clip01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

__device__ __forceinline__ void source_of(const biu_augf_params& P, int x, int y, double& sx, double& sy) {
    const double fx = (double)x, fy = (double)y;
    sx = safe_coord(fma(P.m[0], fx, fma(P.m[1], fy, P.m[2])));
    sy = safe_coord(fma(P.m[3], fx, fma(P.m[4], fy, P.m[5])));
}

// two uniforms of element `elem` for one noise stage; two neighbouring elements share a Philox block
template <class Launch>
__device__ __forceinline__ void uniforms(const Launch& L, const biu_augf_params& P, uint32_t elem, uint32_t stage, float& u1, float& u2) {
    using namespace biu_philox;
    const U4 r = philox4x32_10(U4{elem >> 1, P.index, L.epoch, L.c3 + stage}, L.k0, L.k1);
    const int o = (int)(elem & 1u) * 2;
    u1 = uniform24(word_of(r, o));
    u2 = uniform24(word_of(r, o + 1));
}
__device__ __forceinline__ float normal(float u1, float u2) { return sqrtf(-2.f * logf(1.f - u1)) * cospif(2.f * u2); }

__device__ __forceinline__ float poisson(float lambda, float u1, float u2) {
    if (lambda < 32.f) {
        float p = expf(-lambda), cdf = p;
        int k = 0;
        while (u1 >= cdf && k < BIU_AUGF_POISSON_CAP && ((float)k < lambda || p > 2.3283064365386963e-10f)) {
            ++k;
            p *= lambda / (float)k;
            cdf += p;
        }
        return (float)k;
    }
    return fmaxf(0.f, floorf(lambda + sqrtf(lambda) * normal(u1, u2) + 0.5f));
}

// [shot noise] -> [Gauss noise] of one value; `elem` = index of the element inside its sample's field
template <class Launch>
__device__ __forceinline__ float shot_gauss(const Launch& L, const biu_augf_params& P, float v, uint32_t elem) {
    if (P.flags & BIU_AUGF_SHOT) {
        float u1, u2;
        uniforms(L, P, elem, BIU_AUGF_STAGE_SHOT, u1, u2);
        const float lin = exp2f(2.2f * log2f(v));                           // v = 0 -> 0
        const float cnt = poisson(lin / P.shot_s, u1, u2);
        v = exp2f(log2f(clip01(cnt * P.shot_s)) / 2.2f);
    }
    if (P.flags & BIU_AUGF_GAUSS) {
        float u1, u2;
        uniforms(L, P, elem, BIU_AUGF_STAGE_GAUSS, u1, u2);
        v = clip01(v + P.gauss_sigma * normal(u1, u2));
    }
    return v;
}

// ---- what the float augmenters share beside the stages: the source element, the index rules, the 16-byte store, the box blur's sums --------
// element i behind `base`, a byte scaled to [0, 1] or a float
__device__ __forceinline__ float load(const void* base, int u8, int i) {
    return u8 ? (float)static_cast<const uint8_t*>(base)[i] / 255.0f : static_cast<const float*>(base)[i];
}
__device__ __forceinline__ int wrap(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;
    i %= n;
    return i < 0 ? i + n : i;
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
// the first cnt of PX consecutive pixels; vec: all four as one 16-byte vector
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

// The k x k box blur of a TILE x TILE output tile by a block of TPB lanes.  Its caller gathers the tile plus a halo of k / 2 <= RMAX into
// s_in (rows of IN_PITCH floats) and passes a barrier; blur_sums does the rest:
//   2. sums of k floats along x into s_h; a wave covers one row of 64 sums, its lanes read consecutive floats (no bank conflict)
//   3. sums of k row sums along y, four pixels per lane (16-byte LDS reads of consecutive lanes), times 1 / k^2, then epilogue(v, x, y) on
//      every pixel inside the h x w plane that starts at `out`, and the store.
// A caller that blurs plane after plane needs no barrier of its own between two calls: its next gather writes s_in, which no lane reads after
// the barrier behind step 2, and the next step 2 writes s_h only behind the barrier that follows that gather, by when every lane has left
// this step 3.
constexpr int TPB = 256;
constexpr int TILE = 64;
constexpr int RMAX = BIU_AUG_MAX_BLUR / 2;      // 7
constexpr int IN_MAX = TILE + 2 * RMAX;         // 78 rows / columns of gathered image
constexpr int IN_PITCH = 80;

template <class Epilogue>
__device__ __forceinline__ void blur_sums(const float* s_in, float* s_h, int k, int tx0, int ty0, int h, int w, float* out, bool vec4, Epilogue epilogue) {
    const int ih = TILE + 2 * (k >> 1);
    for (int i = threadIdx.x; i < ih * TILE; i += TPB) {
        const int ly = i / TILE, lx = i % TILE;
        float a = 0.f;
        for (int d = 0; d < k; ++d) a += s_in[ly * IN_PITCH + lx + d];
        s_h[i] = a;
    }
    __syncthreads();
    const float inv = 1.f / (float)(k * k);
    for (int i = threadIdx.x; i < TILE * TILE / 4; i += TPB) {
        const int ly = i / (TILE / 4), lx = (i % (TILE / 4)) * 4;
        const int y = ty0 + ly, x0 = tx0 + lx;
        if (y >= h || x0 >= w) continue;
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        for (int d = 0; d < k; ++d) {
            const float4 q = *reinterpret_cast<const float4*>(&s_h[(ly + d) * TILE + lx]);
            a[0] += q.x; a[1] += q.y; a[2] += q.z; a[3] += q.w;
        }
        const int cnt = min(4, w - x0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a[j] *= inv;
            if (j < cnt) a[j] = epilogue(a[j], x0 + j, y);
        }
        store<4>(out + y * w + x0, a, cnt, vec4);
    }
}

// host: do [a, a + na) and [b, b + nb) share a byte
inline bool overlap(const void* a, unsigned long long na, const void* b, unsigned long long nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}
}  // namespace biu_augment_stages
