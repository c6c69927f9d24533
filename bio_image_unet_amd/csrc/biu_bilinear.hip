// Bilinear x2 up-sampling, align_corners = True -- nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True) in front of
// every decoder node of the nested U-Net++ [multi_output_unet/multi_output_nested_unet.py:73].  2-D, channels-last, bandwidth-bound:
//   * a thread owns one pixel (fine in the forward, coarse in the backward) and walks its channels 16 bytes at a time, so the taps
//     and weights are computed once per pixel and reused for all its channels; the `tpp` threads of a pixel read one row contiguously;
//   * a scalar tail takes the channels past the last whole vector; slices that are not 16-byte addressable run the G = 1 form;
//   * fp32 accumulation for both storage types; the backward is the gather form of the adjoint (no atomics: bit-reproducible).
#include <hip/hip_runtime.h>

#include "biu_common.h"
#include "biu_internal.h"

namespace {

constexpr int TPB = 256;

// PyTorch's taps (area_pixel_compute_scale / _source_index with align_corners = True, fp32):
//   scale = (n_in - 1) / (n_out - 1) (0 when n_out == 1), src = scale * o, i0 = (int)src, i1 = i0 + (i0 < n_in - 1), l1 = src - i0
struct Tap { int i0, i1; float l0, l1; };
__device__ __forceinline__ Tap tap_ac(int o, int n_in, float scale) {
    const float src = scale * (float)o;
    int i0 = (int)src;
    i0 = i0 < n_in - 1 ? i0 : n_in - 1;
    const float l1 = src - (float)i0;
    return Tap{i0, i0 + (i0 < n_in - 1 ? 1 : 0), 1.f - l1, l1};
}
__host__ __device__ __forceinline__ float scale_ac(int n_in, int n_out) {
    return n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f;
}
// weight of coarse index i in the tap of fine index o (both taps count when they coincide)
__device__ __forceinline__ float tap_weight(int o, int i, int n_in, float scale) {
    const Tap t = tap_ac(o, n_in, scale);
    return (t.i0 == i ? t.l0 : 0.f) + (t.i1 == i ? t.l1 : 0.f);
}

// pixel and lane of flat thread index t (tpp = 1 << lg): 32-bit divisions whenever the launch fits them (`small`, uniform per launch)
__device__ __forceinline__ void pix_of(i64 t, int lg, int w, int h, bool small, i64& pix, int& lane, int& x, int& y, int& n) {
    lane = (int)(t & ((1 << lg) - 1));
    pix = t >> lg;
    if (small) {
        const unsigned p = (unsigned)pix, r = p / (unsigned)w;
        x = (int)(p - r * (unsigned)w);
        y = (int)(r % (unsigned)h);
        n = (int)(r / (unsigned)h);
    } else {
        const i64 r = pix / w;
        x = (int)(pix - r * w);
        y = (int)(r % h);
        n = (int)(r / h);
    }
}

// the transform vectors of channels [c0, c0 + G): 16-byte loads when XV (all three vectors 16-byte aligned), identity where absent
template <int G, bool XV>
__device__ __forceinline__ void ld_xf(const DXf& xf, int c0, float* s, float* b, float* l) {
#pragma unroll
    for (int k = 0; k < G; ++k) { s[k] = 1.f; b[k] = 0.f; l[k] = 1.f; }
    const float* src[3] = {xf.scale, xf.shift, xf.slope};
    float* dst[3] = {s, b, l};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        if (!src[q]) continue;
        if constexpr (XV && G % 4 == 0) {
#pragma unroll
            for (int k = 0; k < G; k += 4) {
                const float4 v = *(const float4*)(src[q] + c0 + k);
                dst[q][k] = v.x; dst[q][k + 1] = v.y; dst[q][k + 2] = v.z; dst[q][k + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < G; ++k) dst[q][k] = src[q][c0 + k];
        }
    }
}
__device__ __forceinline__ float xf_v(float v, float s, float b, float l) {      // xf_apply with the channel's constants in registers
    const float t = fmaf(s, v, b);
    return t > 0.f ? t : l * t;
}

template <typename T, int G>
__device__ __forceinline__ void ld_vec(const T* p, float* v) {
    if constexpr (G == 1) {
        v[0] = to_f(p[0]);
    } else {
        const Pack<T, G> q = *(const Pack<T, G>*)p;
#pragma unroll
        for (int k = 0; k < G; ++k) v[k] = to_f(q.v[k]);
    }
}
template <typename T, int G>
__device__ __forceinline__ void st_vec(T* p, const float* v) {
    if constexpr (G == 1) {
        p[0] = from_f<T>(v[0]);
    } else {
        Pack<T, G> q;
#pragma unroll
        for (int k = 0; k < G; ++k) q.v[k] = from_f<T>(v[k]);
        *(Pack<T, G>*)p = q;
    }
}

// out[n, Y, X, :] = ly0 (lx0 T(x[i0y, i0x]) + lx1 T(x[i0y, i1x])) + ly1 (lx0 T(x[i1y, i0x]) + lx1 T(x[i1y, i1x]))  (PyTorch's order)
template <typename T, int G, bool XV>
__global__ __launch_bounds__(TPB) void k_bilinear_up_fwd(DAct x, DXf xf, DAct out, int lg, float sh, float sw) {
    const int C = out.c, nvec = (C + G - 1) / G, tpp = 1 << lg;
    const i64 total = (i64)out.n * out.h * out.w * tpp;
    const bool small = total < (1LL << 31);
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (i64)gridDim.x * blockDim.x) {
        i64 pix;
        int lane, X, Y, n;
        pix_of(t, lg, out.w, out.h, small, pix, lane, X, Y, n);
        const Tap ty = tap_ac(Y, x.h, sh), tx = tap_ac(X, x.w, sw);
        const i64 rowy0 = ((i64)n * x.h + ty.i0) * x.w, rowy1 = ((i64)n * x.h + ty.i1) * x.w;
        const T* p00 = (const T*)x.p + (rowy0 + tx.i0) * x.pitch;
        const T* p01 = (const T*)x.p + (rowy0 + tx.i1) * x.pitch;
        const T* p10 = (const T*)x.p + (rowy1 + tx.i0) * x.pitch;
        const T* p11 = (const T*)x.p + (rowy1 + tx.i1) * x.pitch;
        T* po = (T*)out.p + pix * out.pitch;
        for (int v = lane; v < nvec; v += tpp) {
            const int c0 = v * G;
            if (c0 + G <= C) {
                float a[G], b[G], c[G], d[G], o[G];
                ld_vec<T, G>(p00 + c0, a);
                ld_vec<T, G>(p01 + c0, b);
                ld_vec<T, G>(p10 + c0, c);
                ld_vec<T, G>(p11 + c0, d);
                float s[G], sb[G], sl[G];
                ld_xf<G, XV>(xf, c0, s, sb, sl);
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    const float top = tx.l0 * xf_v(a[k], s[k], sb[k], sl[k]) + tx.l1 * xf_v(b[k], s[k], sb[k], sl[k]);
                    const float bot = tx.l0 * xf_v(c[k], s[k], sb[k], sl[k]) + tx.l1 * xf_v(d[k], s[k], sb[k], sl[k]);
                    o[k] = ty.l0 * top + ty.l1 * bot;
                }
                st_vec<T, G>(po + c0, o);
            } else {
                for (int ch = c0; ch < C; ++ch) {       // scalar tail: C % G channels
                    const float top = tx.l0 * xf_apply(xf, ch, to_f(p00[ch])) + tx.l1 * xf_apply(xf, ch, to_f(p01[ch]));
                    const float bot = tx.l0 * xf_apply(xf, ch, to_f(p10[ch])) + tx.l1 * xf_apply(xf, ch, to_f(p11[ch]));
                    po[ch] = from_f<T>(ty.l0 * top + ty.l1 * bot);
                }
            }
        }
    }
}

// dx[n, y, x, :] (+)= sum over the fine pixels (Y, X) whose taps touch (y, x) of wy(Y) wx(X) dout[n, Y, X, :].  The touching fine
// indices of one axis form a contiguous run inside [2i - 2, 2i + 3] (scale = (n - 1) / (2n - 1) < 1/2 bounds the spread), found once
// per coarse pixel; the weights along a run are recomputed from the same tap function as the forward's (a few ALU ops per 16-byte load).
__device__ __forceinline__ void touch_run(int i, int n_in, int n_out, float scale, int& lo, int& hi) {
    lo = 1;
    hi = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int o = 2 * i - 2 + k;
        if (o >= 0 && o < n_out && tap_weight(o, i, n_in, scale) != 0.f) {
            if (lo > hi) lo = o;
            hi = o;
        }
    }
}

template <typename T, int G>
__global__ __launch_bounds__(TPB) void k_bilinear_up_bwd(DAct dout, DAct dx, int lg, float sh, float sw, int accumulate) {
    const int C = dx.c, nvec = (C + G - 1) / G, tpp = 1 << lg;
    const i64 total = (i64)dx.n * dx.h * dx.w * tpp;
    const bool small = total < (1LL << 31);
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (i64)gridDim.x * blockDim.x) {
        i64 pix;
        int lane, xx, y, n;
        pix_of(t, lg, dx.w, dx.h, small, pix, lane, xx, y, n);
        int ylo, yhi, xlo, xhi;
        touch_run(y, dx.h, dout.h, sh, ylo, yhi);
        touch_run(xx, dx.w, dout.w, sw, xlo, xhi);
        T* pd = (T*)dx.p + pix * dx.pitch;
        for (int v = lane; v < nvec; v += tpp) {
            const int c0 = v * G;
            const int g = c0 + G <= C ? G : C - c0;
            float acc[G];
#pragma unroll
            for (int k = 0; k < G; ++k) acc[k] = 0.f;
            for (int oy = ylo; oy <= yhi; ++oy) {
                const float wyv = tap_weight(oy, y, dx.h, sh);
                const T* row = (const T*)dout.p + ((i64)n * dout.h + oy) * dout.w * dout.pitch + c0;
                for (int ox = xlo; ox <= xhi; ++ox) {
                    const float wgt = wyv * tap_weight(ox, xx, dx.w, sw);
                    const T* src = row + (i64)ox * dout.pitch;
                    float gv[G];
                    if (g == G) {
                        ld_vec<T, G>(src, gv);
                    } else {
#pragma unroll
                        for (int k = 0; k < G; ++k) gv[k] = k < g ? to_f(src[k]) : 0.f;
                    }
#pragma unroll
                    for (int k = 0; k < G; ++k) acc[k] = fmaf(wgt, gv[k], acc[k]);
                }
            }
            if (g == G) {
                if (accumulate) {
                    float old[G];
                    ld_vec<T, G>(pd + c0, old);
#pragma unroll
                    for (int k = 0; k < G; ++k) acc[k] += old[k];
                }
                st_vec<T, G>(pd + c0, acc);
            } else {
                for (int k = 0; k < g; ++k) {            // scalar tail
                    const float o = accumulate ? to_f(pd[c0 + k]) : 0.f;
                    pd[c0 + k] = from_f<T>(acc[k] + o);
                }
            }
        }
    }
}

// log2 of the threads per pixel: enough to cover the row's vectors in one pass, up to a wave
int lg_threads_per_pixel(int nvec) {
    int lg = 0;
    while ((1 << lg) < nvec && lg < 6) ++lg;
    return lg;
}

int check_pair(const biu_act* lo, const biu_act* hi, const char* who) {
    BIU_REQUIRE(valid_act(lo) && valid_act(hi), BIU_ERR_SHAPE, "%s: bad tensor", who);
    BIU_REQUIRE(lo->d == 1 && hi->d == 1, BIU_ERR_SHAPE, "%s: 2-D tensors only (d == 1)", who);
    BIU_REQUIRE(lo->n == hi->n && lo->c == hi->c && hi->h == 2 * lo->h && hi->w == 2 * lo->w, BIU_ERR_SHAPE,
                "%s: expected (h, w) = 2x of the coarse tensor and equal n, c", who);
    return BIU_OK;
}

template <typename T, int G, bool XV>
void launch_fwd(const biu_act* x, const biu_xform* xf, const biu_act* out, hipStream_t st) {
    const int lg = lg_threads_per_pixel((out->c + G - 1) / G);
    hipLaunchKernelGGL((k_bilinear_up_fwd<T, G, XV>), dim3(grid_for(nvox(out) << lg, TPB, 1 << 16)), dim3(TPB), 0, st, dact(x), dxf(xf), dact(out),
                       lg, scale_ac(x->h, out->h), scale_ac(x->w, out->w));
}
template <typename T, int G>
void launch_bwd(const biu_act* dout, const biu_act* dx, int accumulate, hipStream_t st) {
    const int lg = lg_threads_per_pixel((dx->c + G - 1) / G);
    hipLaunchKernelGGL((k_bilinear_up_bwd<T, G>), dim3(grid_for(nvox(dx) << lg, TPB, 1 << 16)), dim3(TPB), 0, st, dact(dout), dact(dx), lg,
                       scale_ac(dx->h, dout->h), scale_ac(dx->w, dout->w), accumulate);
}
// the transform vectors can be read 16 bytes at a time (absent vectors count as aligned)
bool xf16(const biu_xform* xf) {
    return !xf || ((uintptr_t)xf->scale % 16 == 0 && (uintptr_t)xf->shift % 16 == 0 && (uintptr_t)xf->slope % 16 == 0);
}

// 16-byte vectors when both slices' rows and base pointers are 16-byte aligned (the channel count itself may leave a tail)
bool vec16(const biu_act* a, const biu_act* b, int dtype) {
    const size_t es = dsize(dtype);
    return (a->pitch * es) % 16 == 0 && (b->pitch * es) % 16 == 0 && (uintptr_t)a->p % 16 == 0 && (uintptr_t)b->p % 16 == 0;
}

}  // namespace

extern "C" int biu_bilinear_up_fwd(const biu_act* x, const biu_xform* xf, const biu_act* out, int dtype, biu_stream stream) {
    const int rc = check_pair(x, out, "bilinear_up_fwd");
    if (rc != BIU_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool v = vec16(x, out, dtype);
    const bool xv = xf16(xf);
    if (dtype == BIU_BF16) {
        v ? (xv ? launch_fwd<bf16_t, 8, true>(x, xf, out, st) : launch_fwd<bf16_t, 8, false>(x, xf, out, st)) : launch_fwd<bf16_t, 1, false>(x, xf, out, st);
    } else if (dtype == BIU_F32) {
        v ? (xv ? launch_fwd<float, 4, true>(x, xf, out, st) : launch_fwd<float, 4, false>(x, xf, out, st)) : launch_fwd<float, 1, false>(x, xf, out, st);
    } else {
        return biu_fail(BIU_ERR_UNSUPPORTED, "unknown dtype %d", dtype);
    }
    BIU_CHECK_LAUNCH("bilinear_up_fwd");
    return BIU_OK;
}

extern "C" int biu_bilinear_up_bwd(const biu_act* dout, const biu_act* dx, int accumulate, int dtype, biu_stream stream) {
    const int rc = check_pair(dx, dout, "bilinear_up_bwd");
    if (rc != BIU_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool v = vec16(dx, dout, dtype);
    if (dtype == BIU_BF16) {
        v ? launch_bwd<bf16_t, 8>(dout, dx, accumulate, st) : launch_bwd<bf16_t, 1>(dout, dx, accumulate, st);
    } else if (dtype == BIU_F32) {
        v ? launch_bwd<float, 4>(dout, dx, accumulate, st) : launch_bwd<float, 1>(dout, dx, accumulate, st);
    } else {
        return biu_fail(BIU_ERR_UNSUPPORTED, "unknown dtype %d", dtype);
    }
    BIU_CHECK_LAUNCH("bilinear_up_bwd");
    return BIU_OK;
}
