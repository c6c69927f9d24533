// What biu_augment_f32.hip (float fields) and biu_augment_vol.hip (float volumes) must compute alike, kept once: the fp64 source coordinate of
// an output pixel, and the shot and Gauss noise stages with their samplers and their Philox counter.  The contract of both kernels says the
// noise of the one is exactly the noise of the other (include/biu.h); tests/augment_f32_oracle.py restates it for both.
// `Launch` is either file's launch record; read here are its Philox key (k0, k1) and its counter words 2 and 3 (epoch, c3).
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
}  // namespace biu_augment_stages
