/*
 * biu.h -- C ABI of the MI355X-native U-Net hot path (libbiu_hip.so).
 *
 * The reference (danihae/bio-image-unet) has no FFI: its seam is class injection of an nn.Module whose
 * forward/backward dispatch to torch.nn primitives.  Each entry point below replaces one of
 * those primitive call sites with a hand-written gfx950 kernel; the citation on every declaration names the
 * reference line whose arithmetic it takes over.  Paths are relative to /root/reference/bio_image_unet.
 *
 * Conventions
 *   - Activations live in HBM channels-last: element (n,d,h,w,c) of a biu_act is at
 *         p + (((n*D + d)*H + h)*W + w) * pitch + c          (2-D tensors use D = 1)
 *     `pitch` >= c lets several tensors share one buffer as channel slices, which is how the
 *     skip-concat (unet/unet.py:62-67) costs zero bytes: producers write straight into their slice.
 *   - dtype: BIU_F32 or BIU_BF16 for activations / activation gradients.  Parameters, parameter
 *     gradients and all BatchNorm vectors are always fp32.
 *   - A biu_xform is the per-channel epilogue of the *producer* applied by the *consumer* while loading:
 *         T(v) = max(t, slope[c]*t),  t = scale[c]*v + shift[c]        (0 <= slope <= 1)
 *     i.e. BatchNorm-affine followed by LeakyReLU.  NULL members mean scale=1 / shift=0 / slope=1.
 *     Spatial zero padding is applied AFTER T (padding pads the activated tensor).
 *   - Every function only enqueues work on `stream`; no allocation, no host synchronisation.  Outputs and
 *     workspaces are caller-owned (PyTorch's caching allocator in practice).
 *   - Return value: 0 = BIU_OK, otherwise a negative biu_status; biu_last_error() gives a message.
 *     Nothing throws across this boundary.
 */
#ifndef BIU_H
#define BIU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* biu_stream;          /* hipStream_t */

enum { BIU_F32 = 0, BIU_BF16 = 1 };

typedef enum {
    BIU_OK = 0,
    BIU_ERR_SHAPE = -1,            /* operand shapes inconsistent with each other             */
    BIU_ERR_UNSUPPORTED = -2,      /* valid request that no kernel covers                     */
    BIU_ERR_ALIGN = -3,            /* pointer / pitch alignment requirement violated          */
    BIU_ERR_WORKSPACE = -4,        /* workspace too small                                     */
    BIU_ERR_LAUNCH = -5            /* hipLaunchKernel reported an error                       */
} biu_status;

typedef struct {
    void*   p;                     /* first element of channel 0 of the slice                 */
    int32_t n, d, h, w;            /* batch and spatial extent                                */
    int32_t c;                     /* channels in this slice                                  */
    int32_t pitch;                 /* elements between consecutive voxels                     */
} biu_act;

typedef struct {
    const float* scale;
    const float* shift;
    const float* slope;
} biu_xform;

const char* biu_last_error(void);
int  biu_version(void);

/* How fp32 tensors are multiplied by the 2-D 3x3 convolution and ConvTranspose kernels (forward, data gradient, weight gradient).
 *   2 "bf16x6" (default): every operand is split hi + mid + lo in bf16 while it is staged (24 significant bits: the split is exact up to
 *                2^-24), a product is the six terms of order >= 2^-16 -- hi*hi' + hi*mid' + mid*hi' + mid*mid' + hi*lo' + lo*hi' -- on the
 *                bf16 matrix pipe with fp32 accumulation: <= 2^-22 relative per product (what is dropped is <= 2^-23; summing the six terms in
 *                the pipe's fp32 accumulator adds the rest: measured on single products worst 2^-22.6, median 2^-25.3, against 2^-24 / 2^-25.5
 *                of the fp32 MFMA's own rounding to nearest -- tests/test_gpu_fp32_product_probes.py), i.e. fp32-grade, at
 *                2.7 x the matrix-pipe rate of the fp32 MFMA.  Tensors, accumulators and every other kernel stay fp32.
 *   0 "exact"  : v_mfma_f32_32x32x2_f32 -- IEEE fp32 products, fp32 accumulation.
 *   1 "bf16x3" : hi + lo, three terms: <= 2^-15 relative per product (32 x tighter than the TF32 products torch.backends.cudnn
 *                .allow_tf32 = True -- the reference's default on Ampere and later -- uses), twice the rate of mode 2.
 * Process-wide; must be chosen before the first fp32 convolution or weight packing call (the packed weights differ), else BIU_ERR_UNSUPPORTED.
 * BIU_FP32_PRODUCTS=exact|bf16x3|bf16x6 in the environment selects the mode when this function was never called.
 * Replaces: torch.backends.cudnn.allow_tf32 / torch.set_float32_matmul_precision as used around unet/train.py:70-139. */
int  biu_set_fp32_products(int mode);

/* The same choice for the fp32 3-D kernels (kd = 2 | 3): 3x3x3 convolution (forward, data gradient, weight gradient, the fused BatchNorm and
 * two-source forms), ConvTranspose3d k2 s2 and the skip half of the folded decoder level (biu_foldt_*).  Modes as above, but the default is
 * 0 "exact"; 1 "bf16x3" and 2 "bf16x6" are opt-in; the folded up-sampling kernels (biu_upconv_*, both halves of biu_foldt_*) follow it too.
 * Stay exact: launches with fewer than 16 or a non-multiple of 16 reduction channels, 3x3x3 launches wider than LDS allows (more than 1328
 * reduction channels at bf16x6, 3056 at bf16x3), and the ConvTranspose3d data gradient.
 * Latched on its own, independently of biu_set_fp32_products: fixed by the first 3-D fp32 convolution, weight packing or packed-size /
 * workspace query (the packed weights differ), after which another mode is refused with BIU_ERR_UNSUPPORTED.
 * BIU_FP32_PRODUCTS_3D=exact|bf16x3|bf16x6 in the environment selects the mode when this function was never called. */
int  biu_set_fp32_products_3d(int mode);

/* ------------------------------------------------------------------------------------------------
 * 3x3 / 3x3x3 "same" convolution, stride 1, padding = dilation            [K1, K2 of SURVEY 2b]
 * replaces nn.Conv2d / nn.Conv3d inside the conv block: unet/unet.py:56, unet3d/unet3d.py:54,
 * siam_unet/siam_unet.py:61, multi_output_unet3d/multi_output_unet3d.py:86-87
 * ---------------------------------------------------------------------------------------------- */

/* Weight packing for the MFMA implicit-GEMM kernels.  `kind`: 0 = forward operand, 1 = data-gradient
 * operand (spatially flipped, Cin<->Cout swapped).  w is the PyTorch tensor (Cout,Cin,kd,kh,kw) fp32,
 * kd = 1 for 2-D.  biu_conv_packed_bytes returns 0 when the shape is served by the direct kernels and
 * no packing is needed. */
size_t biu_conv_packed_bytes(int kind, int cin, int cout, int kd, int kh, int kw, int dilation, int dtype);
int    biu_conv_pack(int kind, const float* w, int cin, int cout, int kd, int kh, int kw, int dtype,
                     void* packed, biu_stream stream);

/* All packings of a network in one launch.  jobs is DEVICE memory (n entries); each job packs one weight tensor exactly as
 * biu_conv_pack (transposed = 0: PyTorch (Cout, Cin, kd, kh, kw)) or biu_convt_pack (transposed = 1: (Cin, Cout, [2,] 2, 2),
 * kd = 1 | 2) would into `packed` (sized by the matching *_packed_bytes query).                                          */
typedef struct biu_pack_job {
    const void* w;
    void* packed;
    int32_t transposed, kind, cin, cout, kd, kh, kw, reserved;
} biu_pack_job;
int biu_pack_batch(const biu_pack_job* jobs, int n, int dtype, biu_stream stream);

/* Split workspace (caller-owned, like every other byte the library touches).  An fp32 3x3(x3) launch whose bricks x channel
 * tiles would fill under half of the CUs (U-Net bottlenecks) splits its INPUT channels over workgroups: every split writes a
 * partial result into its slice of `ws`, a second kernel sums the slices into the output.  biu_conv_split_workspace returns the
 * bytes such a launch writing y (and y1: the second output of a two-tensor data gradient, else NULL) from `cin` input channels
 * needs; 0 = that launch is never split.  The calls below that take (ws, ws_bytes) split only when ws_bytes covers the query;
 * with ws == NULL (or too small) they run the same arithmetic unsplit.  The library keeps no scratch of its own: nothing is
 * allocated, cached or freed behind the caller's back, so a launch captured in a hipGraph refers to caller memory only.       */
size_t biu_conv_split_workspace(int cin, const biu_act* y, const biu_act* y1, int kd, int kh, int kw, int dilation, int dtype);

/* y = conv(T(x), w) + bias.  w: PyTorch layout fp32; packed: result of biu_conv_pack(kind 0), or NULL
 * when biu_conv_packed_bytes() returned 0 for this shape.  ws: biu_conv_split_workspace(x->c, y, NULL, ...) bytes or NULL.  */
int biu_conv_fwd(const biu_act* x, const biu_xform* xf, const float* w, const void* packed,
                 const float* bias, int kd, int kh, int kw, int dilation,
                 const biu_act* y, void* ws, size_t ws_bytes, int dtype, biu_stream stream);

/* Same, and additionally emits the BatchNorm statistics partials of y: float[nblk][cout][2] = (sum, sum of squares)
 * per block.  On the MFMA path they come out of the convolution's own epilogue (no extra pass over y); otherwise a
 * separate reduction runs.  bn_partial must hold biu_conv_fwd_stats_floats(y, kd) floats; *bn_nblk receives nblk.      */
size_t biu_conv_fwd_stats_floats(const biu_act* y, int kd);
int biu_conv_fwd_stats(const biu_act* x, const biu_xform* xf, const float* w, const void* packed,
                       const float* bias, int kd, int kh, int kw, int dilation, const biu_act* y,
                       float* bn_partial, size_t bn_partial_floats, int* bn_nblk, void* ws, size_t ws_bytes, int dtype,
                       biu_stream stream);

/* dx = conv_transpose_of_the_above(dy): dx[v,ci] = sum_{tap,co} dy[v - off(tap), co] * w[co,ci,tap].
 * packed: result of biu_conv_pack(kind 1) or NULL.  accumulate != 0 adds into dx.
 * ws: biu_conv_split_workspace(dy->c, dx, NULL, ...) bytes or NULL.                                      */
int biu_conv_bwd_data(const biu_act* dy, const float* w, const void* packed,
                      int kd, int kh, int kw, int dilation,
                      const biu_act* dx, int accumulate, void* ws, size_t ws_bytes, int dtype, biu_stream stream);

/* Data gradient that also emits the BatchNorm-backward partial sums (biu_bn_bwd_reduce's output) of the conv block that
 * PRODUCED the tensor whose gradient dx is: y_up is that block's raw conv output, (scale, shift, slope, mean, invstd) its
 * transform / saved statistics.  Use only when this call writes the complete gradient of that tensor.  `partial` holds
 * biu_bwd_data_bnred_floats(dx, kd, transposed) floats; *nblk receives the number of partial rows.                    */
size_t biu_bwd_data_bnred_floats(const biu_act* dx, int kd, int transposed);
int biu_conv_bwd_data_bnred(const biu_act* dy, const float* w, const void* packed, int kd, int kh, int kw, int dilation,
                            const biu_act* dx, const biu_act* y_up, const float* scale, const float* shift,
                            const float* slope, const float* mean, const float* invstd, float* partial,
                            size_t partial_floats, int* nblk, void* ws, size_t ws_bytes, int dtype, biu_stream stream);
int biu_convt_bwd_data_bnred(const biu_act* dy, const float* w, const void* packed, int kd, const biu_act* dx,
                             const biu_act* y_up, const float* scale, const float* shift, const float* slope,
                             const float* mean, const float* invstd, float* partial, size_t partial_floats, int* nblk,
                             int dtype, biu_stream stream);

/* dw[co,ci,tap] = sum_v T(x)[v + off(tap), ci] * dy[v, co]  (PyTorch layout fp32, overwritten);
 * dbias[co] = sum_v dy[v,co] (may be NULL).  ws: biu_conv_bwd_weight_workspace() bytes.                 */
size_t biu_conv_bwd_weight_workspace(int cin, int cout, int kd, int kh, int kw, int dtype);
/* First layers: 1 to 4 input channels, 3x3(x3), dilation 1, 8 | cout (bf16 with 16 | cout runs on the matrix cores, K = cin x taps).
 * biu_conv_first_ok: 1 if a first-layer kernel serves this layer (host arithmetic on the descriptors, no device call);
 * biu_conv_first_workspace: weight-gradient scratch enough for either of its kernels.  biu_conv_bwd_weight_workspace() is 0 for 2..4 input
 * channels, so a caller sizes ws by the larger of the two; with less, these layers take the any-shape kernel.                          */
int biu_conv_first_ok(const biu_act* x, const biu_act* y, int kd, int kh, int kw, int dilation, int dtype);
size_t biu_conv_first_workspace(int cin, int cout, int kd, int dtype);
int biu_conv_bwd_weight(const biu_act* x, const biu_xform* xf, const biu_act* dy,
                        int kd, int kh, int kw, int dilation,
                        float* dw, float* dbias, void* ws, size_t ws_bytes, int dtype, biu_stream stream);

/* Weight gradient with the BatchNorm+LeakyReLU backward of the conv's own output fused into its tile loader:
 * on entry `da` = d loss / d a (a = T(y)); on return it holds d loss / d y (what biu_bn_bwd_apply would write), and
 * dw is the weight gradient w.r.t. that dy.  coefA/B/C come from biu_bn_bwd_finalize.  (The conv bias gradient is
 * identically zero in front of a train-mode BatchNorm and is not produced.)                                          */
int biu_conv_bwd_weight_bn(const biu_act* x, const biu_xform* xf, const biu_act* da, const biu_act* y,
                           const float* scale, const float* shift, const float* slope, const float* coefA,
                           const float* coefB, const float* coefC, int kd, int kh, int kw, int dilation,
                           float* dw, void* ws, size_t ws_bytes, int dtype, biu_stream stream);
/* The block in front of a ONE-channel 1x1 head, when that head is the block's only reader: the head's data gradient
 * da[v][c] = bf16(dlogits[v] * w_head[c]) need not be stored by biu_head_bwd_bnred (dx = NULL) and loaded back here -- the loader
 * rebuilds it from dlogits (fp32 [N,1,D,H,W]) and w_head[C] with the head kernel's own product and rounding.  `dy` is only
 * written (d loss / d y, as biu_conv_bwd_weight_bn leaves it in `da`).  Served: bf16, 3x3x3, 16 output channels, the
 * rolling-window form of the weight gradient; biu_conv_bwd_weight_bn_rank1_ok says (1 / 0), and the call returns
 * BIU_ERR_UNSUPPORTED without launching where it says 0.                                                                      */
int biu_conv_bwd_weight_bn_rank1_ok(const biu_act* x, const biu_act* dy, const biu_act* y, int head_cout, int kd, int kh, int kw,
                                    int dilation, int dtype);
int biu_conv_bwd_weight_bn_rank1(const biu_act* x, const biu_xform* xf, const float* dlogits, const float* w_head, int head_cout,
                                 const biu_act* dy, const biu_act* y, const float* scale, const float* shift, const float* slope,
                                 const float* coefA, const float* coefB, const float* coefC, int kd, int kh, int kw, int dilation,
                                 float* dw, void* ws, size_t ws_bytes, int dtype, biu_stream stream);

/* ------------------------------------------------------------------------------------------------
 * BatchNorm (training: batch statistics) + LeakyReLU(0.1)                          [K3, K4]
 * replaces nn.BatchNorm2d/3d + nn.LeakyReLU: unet/unet.py:57-58, unet3d/unet3d.py:55-56
 * ---------------------------------------------------------------------------------------------- */
#define BIU_BN_MAX_PARTIALS 1024
/* partial: float[nblk][c][2]; returns nblk actually written through *nblk_out (<= BIU_BN_MAX_PARTIALS). */
int biu_bn_stats(const biu_act* y, float* partial, int* nblk_out, int dtype, biu_stream stream);

/* Training-mode finalize: mean/biased var from the partials (fp64 merge), running stats updated with the
 * unbiased variance and `momentum`, and the consumer transform (scale, shift) = (g*r, b - mean*g*r).
 * save_mean / save_invstd are kept for the backward pass.                                                */
int biu_bn_finalize(const float* partial, int nblk, int c, double count,
                    const float* gamma, const float* beta, float* running_mean, float* running_var,
                    float momentum, float eps, float* scale, float* shift,
                    float* save_mean, float* save_invstd, biu_stream stream);

/* Eval-mode transform from the running statistics.                                                       */
int biu_bn_eval_affine(int c, const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, float* scale, float* shift, biu_stream stream);

/* out = T(x) (materialises BatchNorm-affine + LeakyReLU; also plain dtype-preserving copies).            */
int biu_xform_apply(const biu_act* x, const biu_xform* xf, const biu_act* out, int dtype, biu_stream stream);

/* Backward of a = T(y), T = lrelu_slope(scale*y+shift) with scale/shift from batch statistics.
 *   reduce:   partial[nblk][c][2] = (sum dz, sum dz*yhat),  dz = da * T'(.)
 *   finalize: dgamma, dbeta and the three vectors of   dy = A*dz + B*y + C
 *   apply:    dy (may alias da)                                                                           */
int biu_bn_bwd_reduce(const biu_act* da, const biu_act* y, const float* scale, const float* shift,
                      const float* slope, const float* save_mean, const float* save_invstd,
                      float* partial, int* nblk_out, int dtype, biu_stream stream);
int biu_bn_bwd_finalize(const float* partial, int nblk, int c, double count,
                        const float* scale, const float* save_mean, const float* save_invstd,
                        float* dgamma, float* dbeta, float* coefA, float* coefB, float* coefC,
                        biu_stream stream);
/* The same for a BatchNorm in EVAL mode (running statistics are constants: model.eval(); loss.backward(), the frozen-BatchNorm
 * fine-tuning the reference's plain nn.BatchNorm allows, unet/unet.py:54-60).  `partial` from biu_bn_bwd_reduce called with
 * save_mean = running_mean and save_invstd = 1 / sqrt(running_var + eps):  dgamma = sum dz*yhat, dbeta = sum dz, dy = scale * dz, i.e.
 * (A, B, C) = (scale, 0, 0), and the conv bias gradient dbias = sum_v dy = scale * sum dz is no longer zero (dbias may be NULL).          */
int biu_bn_bwd_finalize_eval(const float* partial, int nblk, int c, const float* scale,
                             float* dgamma, float* dbeta, float* dbias, float* coefA, float* coefB, float* coefC,
                             biu_stream stream);
int biu_bn_bwd_apply(const biu_act* da, const biu_act* y, const float* scale, const float* shift,
                     const float* slope, const float* coefA, const float* coefB, const float* coefC,
                     const biu_act* dy, int dtype, biu_stream stream);

/* ------------------------------------------------------------------------------------------------
 * 2x2 / 2x2x2 max-pool, stride 2                                                        [K6]
 * replaces nn.MaxPool2d/3d: unet/unet.py:22-31, unet3d/unet3d.py:26-32
 * bwd routes the gradient to the FIRST maximum in (d,h,w) scan order (PyTorch tie rule).
 * nearest: F.interpolate(scale 0.5 / 2, 'nearest'), multi_output_unet3d.py:112-156     [K11]
 * ---------------------------------------------------------------------------------------------- */
int biu_maxpool_fwd(const biu_act* x, const biu_xform* xf, const biu_act* out, int dtype, biu_stream stream);
int biu_maxpool_bwd(const biu_act* x, const biu_xform* xf, const biu_act* dout, const biu_act* dx,
                    int accumulate, int dtype, biu_stream stream);
/* biu_maxpool_bwd that also emits biu_bn_bwd_reduce's partial sums for the conv block that produced x (xf = that block's
 * BatchNorm transform, mean / invstd its saved statistics).  Use when this call completes the gradient of x.
 * partial holds >= BIU_BN_MAX_PARTIALS * C * 2 floats (more lets the kernel use more workgroups); *nblk = rows written. */
int biu_maxpool_bwd_bnred(const biu_act* x, const biu_xform* xf, const biu_act* dout, const biu_act* dx, int accumulate,
                          const float* mean, const float* invstd, float* partial, size_t partial_floats, int* nblk,
                          int dtype, biu_stream stream);
int biu_nearest_down_fwd(const biu_act* x, const biu_xform* xf, const biu_act* out, int dtype, biu_stream stream);
int biu_nearest_down_bwd(const biu_act* dout, const biu_act* dx, int accumulate, int dtype, biu_stream stream);
int biu_nearest_up_fwd(const biu_act* x, const biu_xform* xf, const biu_act* out, int dtype, biu_stream stream);
int biu_nearest_up_bwd(const biu_act* dout, const biu_act* dx, int accumulate, int dtype, biu_stream stream);

/* Nearest-neighbour up-sampling (x2 per axis) FOLDED into the 3x3x3 convolution behind it -- forward only.
 * replaces F.interpolate(scale_factor=2, mode='nearest') + self.upN_conv's nn.Conv3d:
 * multi_output_unet3d/multi_output_unet3d.py:138-139,147-148,156-157 (conv3d block: :86-87).
 *   y[2v + p] = bias + sum_{t in {0,1}^3} W'[p][t] . T(x)[v + t - 1 + p]      p = output parity per axis, x = the coarse tensor (D,H,W),
 *   W'[p][t] = the sum of the conv's taps that read the same coarse voxel (8 x 8 tap groups instead of 27 taps: 0.30 x the FLOPs),
 * identical to the convolution of the up-sampled tensor up to fp32 summation order (coarse zero padding = fine zero padding).
 * y is (2D, 2H, 2W).  biu_upconv_bwd_data is the matching data gradient straight onto the coarse tensor (replaces biu_conv_bwd_data +
 * biu_nearest_up_bwd):   dx[u] (+)= sum_p sum_{s in {0,1}^3} W'[p][1 - s]^T . dy[2 (u - p + s) + p].
 * biu_upconv_bwd_weight_bn is the weight gradient, with the block's BatchNorm+LeakyReLU backward in its loader exactly as
 * biu_conv_bwd_weight_bn has it (da -> dy in place; y = NULL: da already is dy): per parity class
 *   G[p][t] = sum_v dy[2v + p] (x) T(x)[v + t - 1 + p],   dw[k] = sum_p G[p][t_p(k)]   (t_p(k): the coarse tap fine tap k reads under parity p);
 * with all three the up-sampled tensor is never materialised (no biu_nearest_up_fwd / _bwd).
 * biu_upconv_ok: shapes / channels the folded kernels serve (else: up-sample + biu_conv_*).  biu_upconv_pack folds and packs
 * w (Cout, Cin, 3, 3, 3) fp32 into `packed` (biu_upconv_packed_bytes; kind 0 = forward image, 1 = data-gradient image).
 * bn_partial may be NULL (no statistics); with it, *bn_nblk partial rows of [Cout][2] (sum, sum of squares) are written, as
 * biu_conv_fwd_stats does (biu_upconv_fwd_stats_floats sizes the buffer). */
int    biu_upconv_ok(const biu_act* x, const biu_act* y, int dtype);
size_t biu_upconv_packed_bytes(int kind, int cin, int cout, int dtype);
int    biu_upconv_pack(int kind, const float* w, int cin, int cout, int dtype, void* packed, biu_stream stream);
int    biu_upconv_bwd_data(const biu_act* dy, const void* packed, const biu_act* dx, int accumulate, int dtype, biu_stream stream);
size_t biu_upconv_bwd_weight_workspace(int cin, int cout, int dtype);
int    biu_upconv_bwd_weight_bn(const biu_act* x, const biu_xform* xf, const biu_act* da, const biu_act* y, const float* scale,
                                const float* shift, const float* slope, const float* coefA, const float* coefB, const float* coefC,
                                float* dw, void* ws, size_t ws_bytes, int dtype, biu_stream stream);
size_t biu_upconv_fwd_stats_floats(const biu_act* x, const biu_act* y);
int    biu_upconv_fwd(const biu_act* x, const biu_xform* xf, const void* packed, const float* bias, const biu_act* y,
                      float* bn_partial, size_t bn_partial_floats, int* bn_nblk, int dtype, biu_stream stream);

/* ------------------------------------------------------------------------------------------------
 * ConvTranspose k=2, stride=2 (non-overlapping)                                         [K7]
 * replaces nn.ConvTranspose2d/3d: unet/unet.py:38-47, unet3d/unet3d.py:40-42
 * w: PyTorch layout (Cin, Cout, kd, 2, 2) fp32 with kd = 2 (3-D) or 1 (2-D).
 * ---------------------------------------------------------------------------------------------- */
/* d loss / d logits of one head from the caller's gradients w.r.t. its logits and / or its activated output (act as in
 * biu_head_fwd; multi_output_unet3d.py:97-104), written to channels [dst_c0, dst_c0 + ch) of a fp32 [n, dst_channels, spatial]
 * tensor -- the stacked operand of one biu_head_bwd over all heads that share a trunk.                                    */
int biu_head_dlogits(const float* g_logits, const float* g_act, const float* activated, int act, int n, int ch, long long spatial,
                     float* dst, int dst_channels, int dst_c0, biu_stream stream);

/* The criteria of the 2-D multi-output trainer (multi_output_unet/losses.py) on ACTIVATED head outputs: pred / target fp32 contiguous
 * [n, c, h, w] as the head kernel emits them; one head with its nlev <= BIU_MO2D_MAX_LEVELS deep-supervision predictions per launch
 * (multi_output_unet/train.py:157-181: the levels share a target).  e = pred - target, M = n c h w, G_y / G_x = torch.gradient along h / w.
 *   kind                          (p0, p1, p2)                    value
 *   0 BCEDiceLoss                 (bce_weight, dice_weight, -)    p0 mean(-t max(log p, -100) - (1-t) max(log(1-p), -100)) + p1 (1 - (2 sum pt + 1e-5) / (sum p + sum t + 1e-5))
 *   1 TverskyLoss, 2 logcosh...   (alpha, beta, smooth)           1 - Tv | log cosh(1 - Tv),  Tv = (TP + s) / (TP + alpha FP + beta FN + s) on probabilities
 *   3 MSELoss  4 MAELoss  5 HuberLoss (delta, -, -)               mean e^2 | mean |e| | mean(|e| < delta ? e^2 / 2 : delta (|e| - delta / 2))
 *   6 DistanceGradientLoss        (alpha, -, -)                   mean e^2 + alpha (mean (G_y e)^2 + mean (G_x e)^2)
 *   7 WeightedDistanceGradient... (alpha, beta, -)                w = t > 0 ? beta : 1 - beta, e~ = w e: mean e~^2 + mean |e~| + alpha (mean (G_y e~)^2 + mean (G_x e~)^2)
 *   8 WeightedVectorFieldLoss     (beta, magnitude_weight, -)     c == 2; w = (t0 != 0 or t1 != 0) ? beta : 1 - beta:
 *                                                                 mean (w e)^2 + mean |w e| + p1 mean_{n h w} (w (p0^2 + p1^2) - w (t0^2 + t1^2))^2
 * biu_mo2d_loss_fwd:    partial[nlev][biu_mo2d_loss_blocks(M)][BIU_MO2D_SLOTS] per-block sums (no atomics: bit-reproducible).  Kinds 6, 7
 *                       refuse h < 2 or w < 2 (BIU_ERR_SHAPE), as torch.gradient does; kind 8 refuses c != 2.
 * biu_mo2d_loss_finish: ONE one-block launch for all heads and levels of a step.  terms (device array, nterms <= BIU_MO2D_MAX_TERMS) name
 *                       each (head, level): its partial rows (offset in floats into `workspace`), kind, parameters and weight
 *                       (supervision weight x head weight) ->
 *                       saved[8 + 8 nterms] = { sum_t weight_t loss_t, #pred outside [0, 1], #target outside [0, 1] (kind 0 terms), 0 x 5,
 *                                               then per term { loss_t, merged sums[6], 0 } }.
 * biu_mo2d_loss_coef:   g = d / d total (device scalar) -> coef[nterms][4].
 * biu_mo2d_loss_bwd:    dpred[l] = d total / d pred[l] for the nlev levels of one head from its coef rows (coef + 4 * first term); the
 *                       torch.gradient kinds gather G^T G e (a +-2 stencil per axis with its edge rows / columns), no atomics.
 * (ea, eb): what the per-element arithmetic needs -- kind 5: (delta, 0); kinds 7, 8: (beta, 1 - beta) as the caller rounds them, i.e. the
 * weight where the target is set and elsewhere; ignored by the other kinds.
 * pred / dpred: host arrays of nlev device pointers.  16-byte accesses when every pointer is 16-byte aligned (and w % 4 == 0 for kinds
 * 6, 7, h w % 4 == 0 for kind 8), with a scalar tail for the flat kinds; scalar accesses otherwise.                                    */
#define BIU_MO2D_MAX_LEVELS 4
#define BIU_MO2D_MAX_TERMS 32
#define BIU_MO2D_SLOTS 8
typedef struct biu_mo2d_term {
    int kind, nb;               /* nb: rows of this term's partial (biu_mo2d_loss_blocks)          */
    long long partial_off;      /* floats, into the workspace handed to biu_mo2d_loss_finish       */
    long long numel, pixels;    /* n c h w and n h w                                               */
    float p0, p1, p2, weight;
} biu_mo2d_term;
int biu_mo2d_loss_blocks(long long numel);
int biu_mo2d_loss_fwd(int kind, float ea, float eb, const float* const* pred, int nlev, const float* target, int n, int c, int h, int w,
                      float* partial, biu_stream stream);
int biu_mo2d_loss_finish(const biu_mo2d_term* terms, int nterms, const float* workspace, float* saved, biu_stream stream);
int biu_mo2d_loss_coef(const biu_mo2d_term* terms, int nterms, const float* g, const float* saved, float* coef, biu_stream stream);
int biu_mo2d_loss_bwd(int kind, float ea, float eb, const float* const* pred, int nlev, const float* target, int n, int c, int h, int w,
                      const float* coef, float* const* dpred, biu_stream stream);

/* The segmentation criteria on logits (p = sigmoid(x)): the single-head criteria of losses.py (unet/losses.py:78-239, any rank, passed as
 * [n, c, 1, 1, rest]) and those of the 3-D multi-output trainer (multi_output_unet3d/losses.py).  x / target fp32 contiguous
 * [n, c, d, h, w]; only per = c d h w matters to kinds 0..2.  M = n per, sums over one sample carry _n.
 *   kind                    (p0, p1, p2)            value
 *   0 BCEDiceLoss           (alpha, beta, smooth)   p0 mean BCEWithLogits(x, t) + p1 (1 - mean_n 2 (sum_n p t + s) / (sum_n p + sum_n t + s))
 *   1 TverskyLoss           (alpha, beta, smooth)   1 - Tv,  Tv = (TP + s) / (TP + alpha FP + beta FN + s) over the whole tensor
 *   2 logcoshTverskyLoss    (alpha, beta, smooth)   log cosh(1 - Tv)
 *   3 BCEDiceTemporalLoss   (w0, w1, -)             p0 BCEDice(1, 1) (s = 1) + p1 mean |x[:, :, 1:] - x[:, :, :-1]| over
 *                                                   pairs = n c (d - 1) h w; nan when d == 1 (l1_loss over an empty slice)
 *   4 pair SmoothL1         (-, -, -)               sum SmoothL1(x[1:] - x[:-1]) / pairs between neighbouring BATCH entries, the "time" term
 *                                                   of the 3-D trainer (unet3d/train.py:140-145): a table term only (n = 1, rows =
 *                                                   biu_pair_smooth_l1_blocks(pairs), pairs = (N - 1) per), refused by _fwd / _bwd
 * biu_mo3d_loss_blocks: rows = the partial rows PER SAMPLE for a tensor of numel elements.
 * biu_mo3d_loss_fwd:    partial[n][rows][BIU_MO3D_SLOTS] per-block sums { BCE, p, t, p t, |x[z+1] - x[z]| (kind 3), 0 x 3 }, no atomics:
 *                       bit-reproducible.  pre_act (0 none, 1 sigmoid, 2 tanh, 3 relu) is applied to x before everything else -- the
 *                       validation pass of the reference, forward only.
 * biu_pair_smooth_l1_fwd: partial[biu_pair_smooth_l1_blocks(pairs)][BIU_MO3D_SLOTS], the block's sum of SmoothL1 in slot 0, 0 x 7.
 * biu_mo3d_loss_finish: ONE one-block launch for all terms of a step.  terms (device array, nterms <= BIU_MO3D_MAX_TERMS) name each one:
 *                       its partial rows (offset in floats into `workspace`), kind, extents, parameters and weight ->
 *                       saved[BIU_MO3D_SAVED_HEADER + BIU_MO3D_SLOTS sum_terms n] = { sum_t weight_t loss_t, loss_0 .. loss_{nterms-1}, 0 ..,
 *                       then per (term, sample) in table order the merged row }.
 * biu_mo3d_loss_coef:   g = d / d total (device scalar) -> coef[sum_terms n][4] = { c0, c1, c2, ct } per (term, sample), table order;
 *                       kind 4: c0 = g weight / pairs.
 * biu_mo3d_loss_bwd:    dx = c0 (p - t) + (c1 + c2 t) p (1 - p) + ct (sign(x[z] - x[z-1]) - sign(x[z+1] - x[z])) for one head from its coef
 *                       rows (coef + 4 * samples of the terms before it); the missing neighbour's term is dropped at z = 0 and z = d - 1,
 *                       sign(0) = 0.  Takes x as given: a pre-activation under autograd is the caller's.
 * biu_pair_smooth_l1_bwd: dlogits (+)= coef[0] * d sum SmoothL1 / d logits, coef = the kind-4 term's row of biu_mo3d_loss_coef.
 * 16-byte accesses when every pointer is 16-byte aligned and c d h w % 4 == 0 (kind 3: h w % 4 == 0 too); scalar accesses otherwise.
 * n <= 65535 (one grid row per sample).                                                                                               */
#define BIU_MO3D_PAIR_SL1 4
#define BIU_MO3D_MAX_TERMS 16
#define BIU_MO3D_SLOTS 8
#define BIU_MO3D_SAVED_HEADER 32
typedef struct biu_mo3d_term {
    int kind, rows;             /* rows: partial rows per sample (biu_mo3d_loss_blocks)            */
    long long partial_off;      /* floats, into the workspace handed to biu_mo3d_loss_finish       */
    long long n, per_sample;    /* samples, and c d h w                                            */
    long long pairs;            /* n c (d - 1) h w; kind 4: (N - 1) per                            */
    float p0, p1, p2, weight;
} biu_mo3d_term;
int biu_mo3d_loss_blocks(long long numel);
int biu_mo3d_loss_fwd(int kind, int pre_act, const float* x, const float* target, int n, int c, int d, int h, int w, float* partial,
                      biu_stream stream);
int biu_mo3d_loss_finish(const biu_mo3d_term* terms, int nterms, const float* workspace, float* saved, biu_stream stream);
int biu_mo3d_loss_coef(const biu_mo3d_term* terms, int nterms, const float* g, const float* saved, float* coef, biu_stream stream);
int biu_mo3d_loss_bwd(int kind, const float* x, const float* target, int n, int c, int d, int h, int w, const float* coef, float* dx,
                      biu_stream stream);
int biu_pair_smooth_l1_blocks(long long pairs);
int biu_pair_smooth_l1_fwd(const float* logits, int n, long long per_sample, float* partial, biu_stream stream);
int biu_pair_smooth_l1_bwd(const float* logits, int n, long long per_sample, const float* coef, float* dlogits, int accumulate,
                           biu_stream stream);

/* Trilinear x2 up-sampling, align_corners = False (F.interpolate(scale_factor=2, mode='trilinear'),
 * unet3d/unet3d.py:82,89,96): out = interp(T(x)); depth is doubled when out->d == 2 * x->d, kept when equal.
 * bwd: dx (+)= adjoint(dout).                                                                                        */
int biu_trilinear_up_fwd(const biu_act* x, const biu_xform* xf, const biu_act* out, int dtype, biu_stream stream);
int biu_trilinear_up_bwd(const biu_act* dout, const biu_act* dx, int accumulate, int dtype, biu_stream stream);

/* Bilinear x2 up-sampling, align_corners = True (nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True),
 * multi_output_unet/multi_output_nested_unet.py:73): out = interp(T(x)); 2-D only (d == 1); out->h == 2 x->h, out->w == 2 x->w.
 * Taps as PyTorch's, in fp32: scale = (n_in - 1) / (n_out - 1) (0 when n_out == 1), src = scale * o, i0 = (int)src,
 * i1 = i0 + (i0 < n_in - 1), l1 = src - i0.  Both tensors may be pitched channel slices.
 * bwd: dx (+)= adjoint(dout), gather form (no atomics: bit-reproducible).                                              */
int biu_bilinear_up_fwd(const biu_act* x, const biu_xform* xf, const biu_act* out, int dtype, biu_stream stream);
int biu_bilinear_up_bwd(const biu_act* dout, const biu_act* dx, int accumulate, int dtype, biu_stream stream);

/* Depth-wise cross-correlation of two equal 2-D maps, padding='same' (Siam_UNet.depthwise_xcorr,
 * siam_unet/siam_unet.py:75-83): out[n,y,x,c] = sum_ij T(cur)[n,y+i-ph,x+j-pw,c] * T(prev)[n,i,j,c], ph=(H-1)/2, pw=(W-1)/2.
 * bwd needs identity transforms (materialised operands): dcur, dprev (+)= gradients.                                  */
int biu_xcorr_fwd(const biu_act* cur, const biu_xform* xc, const biu_act* prev, const biu_xform* xp, const biu_act* out,
                  int dtype, biu_stream stream);
int biu_xcorr_bwd(const biu_act* cur, const biu_xform* xc, const biu_act* prev, const biu_xform* xp, const biu_act* dout,
                  const biu_act* dcur, const biu_act* dprev, int accumulate, int dtype, biu_stream stream);

/* The same conv block on a channel CONCATENATION (x0 | x1) whose two parts stay in separate dense buffers -- the decoder's
 * torch.cat (unet/unet.py:62-67, unet3d/unet3d.py:60-61) without a concat buffer.  w / packed / dw have Cin = x0->c + x1->c in
 * that order.  Only shapes the MFMA kernels serve: biu_conv_cat_ok returns 1 when all three calls will succeed (channel counts
 * that are multiples of 32 -- x0's of 64 when the total is an even number of 32-tiles --, dilation 1, aligned dense rows).
 * fwd: bn_partial may be NULL (no statistics).  bwd_weight: y == NULL gives the plain weight gradient (da is dy), otherwise the
 * BatchNorm backward is fused exactly as in biu_conv_bwd_weight_bn.  bwd_data writes dx0 and dx1 (each with its own
 * accumulate flag).  (ws, ws_bytes) of fwd / bwd_data: biu_conv_split_workspace(x0->c + x1->c, y, NULL, ...) resp.
 * (dy->c, dx0, dx1, ...) bytes, or NULL.                                                                                  */
int biu_conv_cat_ok(const biu_act* x0, const biu_act* x1, const biu_act* y, int kd, int kh, int kw, int dilation, int dtype);
int biu_conv_fwd_cat(const biu_act* x0, const biu_xform* xf0, const biu_act* x1, const biu_xform* xf1, const float* w,
                     const void* packed, const float* bias, int kd, int kh, int kw, int dilation, const biu_act* y,
                     float* bn_partial, size_t bn_partial_floats, int* bn_nblk, void* ws, size_t ws_bytes, int dtype,
                     biu_stream stream);
int biu_conv_bwd_data_cat(const biu_act* dy, const float* w, const void* packed, int kd, int kh, int kw, int dilation,
                          const biu_act* dx0, int accumulate0, const biu_act* dx1, int accumulate1, void* ws, size_t ws_bytes,
                          int dtype, biu_stream stream);
int biu_conv_bwd_weight_cat(const biu_act* x0, const biu_xform* xf0, const biu_act* x1, const biu_xform* xf1,
                            const biu_act* da, const biu_act* y, const float* scale, const float* shift, const float* slope,
                            const float* coefA, const float* coefB, const float* coefC, int kd, int kh, int kw, int dilation,
                            float* dw, void* ws, size_t ws_bytes, int dtype, biu_stream stream);

/* MFMA operand packing, as for the 3x3 kernels.  kind 0 = forward operand, 1 = data-gradient operand.          */
size_t biu_convt_packed_bytes(int kind, int cin, int cout, int kd, int dtype);
int    biu_convt_pack(int kind, const float* w, int cin, int cout, int kd, int dtype, void* packed, biu_stream stream);
/* y[2v + a, co] = bias[co] + sum_ci T(x)[v, ci] * w[ci, co, a]                                                 */
int biu_convt_fwd(const biu_act* x, const biu_xform* xf, const float* w, const void* packed, const float* bias,
                  int kd, const biu_act* y, int dtype, biu_stream stream);
/* dx[v, ci] (+)= sum_{a, co} dy[2v + a, co] * w[ci, co, a]                                                      */
int biu_convt_bwd_data(const biu_act* dy, const float* w, const void* packed, int kd, const biu_act* dx,
                       int accumulate, int dtype, biu_stream stream);
/* dw[ci, co, a] = sum_v T(x)[v, ci] * dy[2v + a, co]; dbias[co] = sum dy (may be NULL)                          */
size_t biu_convt_bwd_weight_workspace(int cin, int cout, int kd, int dtype);
int biu_convt_bwd_weight(const biu_act* x, const biu_xform* xf, const biu_act* dy, int kd, float* dw, float* dbias,
                         void* ws, size_t ws_bytes, int dtype, biu_stream stream);

/* ConvTranspose(k2, s2) + concat + 3x3x3 convolution of a decoder level as ONE op, the up half folded onto the coarse tensor.
 * replaces self.upN (nn.ConvTranspose3d) + torch.cat + the first conv of the decode block: unet3d/unet3d.py:40-42,84-90
 * (multi_output_unet3d/multi_output_unet3d.py with use_interpolation=False likewise); no non-linearity sits between the two.
 *   y = conv(concat(convT(T(x_low)) + b_T, T(skip))) + b_conv
 *     = conv_skip(T(skip)) + b_conv + sum_{taps k inside} Wb[k] + sum_{t in {0,1}^3} W'[p][t] . T(x_low)[v + t - 1 + p]        at y[2v + p],
 *   W'[p][t][ci][co] = sum_{k in class(p,t)} sum_c W_conv[co][c][k] W_T[ci][c][q(p,k)],  Wb[k][co] = sum_c W_conv[co][c][k] b_T[c]:
 * the same function of the four parameter tensors (the up-sampled tensor is not materialised, 8 x 8 instead of 27 taps on its channels).
 * w_conv (Cout, cup + cskip, 3,3,3) with the concat order (up | skip); w_t (Cin_low, cup, 2,2,2); packed: biu_foldt_packed_bytes, refreshed
 * by biu_foldt_pack whenever one of the four tensors changes.  biu_foldt_ok: the kernels serve the level and it is large enough to pay for the
 * weight-space work of every step (3 x 216 small GEMMs of Cout x cup x Cin_low; BIU_FOLDT=always in the environment drops the size test).  bn_partial as in biu_upconv_fwd (biu_foldt_fwd_stats_floats). */
int    biu_foldt_ok(const biu_act* x_low, const biu_act* skip, const biu_act* y, int dtype);
size_t biu_foldt_packed_bytes(int cin_low, int cskip, int cout, int dtype);
int    biu_foldt_pack(const float* w_conv, const float* b_conv, const float* w_t, const float* b_t, int cin_low, int cup, int cskip, int cout,
                      int dtype, void* packed, biu_stream stream);
size_t biu_foldt_fwd_stats_floats(const biu_act* x_low, const biu_act* y);
/* which form biu_foldt_fwd takes: 0 = brick kernels (the skip half + biases stored, the border shell corrected, the fold accumulated on top);
 * 1 = rolling-window kernels for 64 -> 32 | 32-channel levels (the fold + border-state bias stored first, the skip half accumulated onto it and
 * rounded once).  Same function; the storage roundings of the intermediate differ (a bit-level checker needs to know: tests/insitu.py). */
int    biu_foldt_fwd_form(const biu_act* x_low, const biu_act* skip, const biu_act* y, int dtype);
int    biu_foldt_fwd(const biu_act* x_low, const biu_xform* xf_low, const biu_act* skip, const biu_xform* xf_skip, const void* packed,
                     const biu_act* y, float* bn_partial, size_t bn_partial_floats, int* bn_nblk, int dtype, biu_stream stream);
/* backward of the same op.  biu_foldt_bwd_data: d skip (the conv's data gradient restricted to the skip channels) and d x_low (the composed fold
 * transposed: replaces biu_conv_bwd_data_cat's up half + biu_convt_bwd_data); y_low != NULL additionally emits the BatchNorm-backward sums of
 * x_low's producer as biu_convt_bwd_data_bnred does (acc_low must be 0; biu_foldt_bwd_data_bnred_floats sizes `partial`).
 * biu_foldt_bwd_weight_bn: BatchNorm+LeakyReLU backward of the block in the loader (da -> dy in place; y = NULL: da already is dy), then
 *   dw_conv (Cout, cup + cskip, 27) in full, dw_t (Cin_low, cup, 8) and db_t (cup; may be NULL) by the chain rule from
 *   G[p][t] = sum_v dy[2v + p] (x) T(x_low)[v + t - 1 + p]:  dw_conv[.., c < cup, k] = sum_p W_T[., c, q(p,k)] . G[p][t_p(k)] + b_T[c] S_k,
 *   dw_t[ci, c, q] = sum_{(p,k): q(p,k) = q} W_conv[., c, k] . G[p][t_p(k)][., ci],  db_t[c] = sum_k W_conv[., c, k] . S_k with S_k the sum of dy over
 *   the voxels whose tap k stays inside the tensor = dy_sum - (border sums).  dy_sum (Cout floats) = sum_v dy per channel; NULL = identically
 *   zero, which holds behind a train-mode BatchNorm only: a plain dy (y = NULL) or an eval-mode BatchNorm (coefB = coefC = 0, see
 *   biu_bn_bwd_finalize_eval) must pass it (BIU_ERR_UNSUPPORTED otherwise when the ConvT has a bias). */
size_t biu_foldt_bwd_data_bnred_floats(const biu_act* dx_low);
int    biu_foldt_bwd_data(const biu_act* dy, const void* packed, const biu_act* dx_low, int acc_low, const biu_act* dskip, int acc_skip,
                          const biu_act* y_low, const float* scale, const float* shift, const float* slope, const float* mean,
                          const float* invstd, float* partial, size_t partial_floats, int* nblk, void* ws, size_t ws_bytes, int dtype,
                          biu_stream stream);
size_t biu_foldt_bwd_weight_workspace(int cin_low, int cskip, int cout, int dtype);
int    biu_foldt_bwd_weight_bn(const biu_act* x_low, const biu_xform* xf_low, const biu_act* skip, const biu_xform* xf_skip, const biu_act* da,
                               const biu_act* y, const float* scale, const float* shift, const float* slope, const float* coefA,
                               const float* coefB, const float* coefC, const float* dy_sum, const float* w_conv, const float* w_t, const float* b_t,
                               int cup, float* dw_conv, float* dw_t, float* db_t, void* ws, size_t ws_bytes, int dtype, biu_stream stream);
/* the same call in parts, for a caller that overlaps everything only the optimizer waits for with the rest of its backward.  `phases` is a
 * mask: 1 = the skip half (da -> dy in place by the fused BatchNorm backward, the skip slice of dw_conv); 4 = G on the finished dy into ws;
 * 2 = the border sums of dy and the chain rule on the tables (the up slice of dw_conv, dw_t, db_t).  Parts 4 and 2 read dy (= da after part
 * 1), x_low, ws, dy_sum and the parameters: they may be enqueued on ANOTHER stream once part 1 is complete there (the caller orders them
 * with an event, part 4 before part 2, and leaves dy and ws alone in between; reading dy meanwhile is fine); 7 = biu_foldt_bwd_weight_bn. */
int    biu_foldt_bwd_weight_bn_phase(const biu_act* x_low, const biu_xform* xf_low, const biu_act* skip, const biu_xform* xf_skip, const biu_act* da,
                                     const biu_act* y, const float* scale, const float* shift, const float* slope, const float* coefA,
                                     const float* coefB, const float* coefC, const float* dy_sum, const float* w_conv, const float* w_t,
                                     const float* b_t, int cup, float* dw_conv, float* dw_t, float* db_t, void* ws, size_t ws_bytes, int dtype,
                                     int phases, biu_stream stream);

/* ------------------------------------------------------------------------------------------------
 * 1x1(x1) head + activation                                                             [K9]
 * replaces final Conv + torch.sigmoid: unet/unet.py:51,103-104, unet3d/unet3d.py:50,98-99,
 * multi_output_unet3d.py:80-82,164-168.  Outputs are fp32 NCDHW (what the caller's loss consumes).
 * act: 0 none, 1 sigmoid, 2 tanh, 3 relu.  logits / activated may each be NULL.
 * ---------------------------------------------------------------------------------------------- */
int biu_head_fwd(const biu_act* x, const biu_xform* xf, const float* w, const float* bias, int cout,
                 int act, float* logits, float* activated, int dtype, biu_stream stream);
/* dlogits: fp32 NCDHW.  dx = W^T dlogits (activation-gradient layout); dw (cout,cin), dbias (cout) fp32,
 * overwritten; each of dx / dw / dbias may be NULL.  ws: biu_head_bwd_workspace(cin) bytes (for dw).      */
size_t biu_head_bwd_workspace(int cin);
int biu_head_bwd(const biu_act* x, const biu_xform* xf, const float* w, int cout, const float* dlogits,
                 const biu_act* dx, float* dw, float* dbias, void* ws, size_t ws_bytes, int dtype,
                 biu_stream stream);
/* biu_head_bwd that also emits biu_bn_bwd_reduce's partial sums of the conv block that produced x (xf = its BatchNorm transform,
 * mean / invstd its saved statistics); valid when the head is x's only reader.  partial: >= BIU_BN_MAX_PARTIALS * C * 2 floats.
 * dx = NULL (C <= 32, cout <= 2, 16-byte rows): dx is not stored, dw / dbias / partial are bit for bit what the storing call
 * gives (the sums are taken from the value rounded to the storage type) -- for biu_conv_bwd_weight_bn_rank1.                  */
int biu_head_bwd_bnred(const biu_act* x, const biu_xform* xf, const float* w, int cout, const float* dlogits, const biu_act* dx,
                       float* dw, float* dbias, void* ws, size_t ws_bytes, const float* mean, const float* invstd,
                       float* partial, size_t partial_floats, int* nblk, int dtype, biu_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Element-wise helpers on activation slices
 * ---------------------------------------------------------------------------------------------- */
/* out = max(T1(a), T2(b))  -- Siam 'max' join, siam_unet/siam_unet.py:117; bwd: the winner takes dout, an exact tie
 * splits it evenly (torch.maximum's backward).                                                              */
int biu_max_join_fwd(const biu_act* a, const biu_xform* xa, const biu_act* b, const biu_xform* xb,
                     const biu_act* out, int dtype, biu_stream stream);
int biu_max_join_bwd(const biu_act* a, const biu_xform* xa, const biu_act* b, const biu_xform* xb,
                     const biu_act* dout, const biu_act* da, const biu_act* db, int accumulate,
                     int dtype, biu_stream stream);
/* dst (+)= src, both activation slices of equal shape.                                                   */
int biu_act_add(const biu_act* src, const biu_act* dst, int accumulate, int dtype, biu_stream stream);
/* NC[D]HW fp32 <-> channels-last activation (network input / gradient at the module boundary).           */
int biu_from_nchw(const float* src, const biu_act* dst, int dtype, biu_stream stream);
int biu_to_nchw(const biu_act* src, const biu_xform* xf, float* dst, int dtype, biu_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Attention gate of AttentionUnet (unet/attention_unet.py:112-181; the 1x1 conv + BatchNorm stages are biu_conv_* calls
 * with kernel size 1 and slope 1):
 *   add_relu: out = relu(T(a) + T(b))                               (:177, psi = self.relu(g1 + x1))
 *             bwd: da, db (+)= dout where the stored out > 0
 *   gate:     out[v, c] = T(e)[v, c] * sigmoid(T(psi)[v, 0])         (:178-179, psi has ONE channel)
 *             bwd: de[v, c] (+)= dout[v, c] * s ;  dpsi[v] = s (1 - s) * sum_c dout[v, c] * T(e)[v, c]   (gradient w.r.t. T(psi));
 *             de may be NULL.
 * ---------------------------------------------------------------------------------------------- */
int biu_add_relu_fwd(const biu_act* a, const biu_xform* xa, const biu_act* b, const biu_xform* xb, const biu_act* out, int dtype,
                     biu_stream stream);
int biu_add_relu_bwd(const biu_act* out, const biu_act* dout, const biu_act* da, const biu_act* db, int accumulate, int dtype,
                     biu_stream stream);
int biu_gate_fwd(const biu_act* e, const biu_xform* xe, const biu_act* psi, const biu_xform* xpsi, const biu_act* out, int dtype,
                 biu_stream stream);
int biu_gate_bwd(const biu_act* e, const biu_xform* xe, const biu_act* psi, const biu_xform* xpsi, const biu_act* dout,
                 const biu_act* de, int accumulate_e, const biu_act* dpsi, int dtype, biu_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Data formats either side of the network, kept on the device
 *   biu_from_nchw_u8 : uint8 NC[D]HW batch / divisor -> channels-last activation; replaces `batch / 255` + `.to(device)` of float32
 *                      (unet/data.py:253-266 items, unet/predict.py:192-196 patches): a quarter of the H2D bytes, no float copy.
 *                      The fp32 value is the correctly rounded quotient (float)byte / divisor, `tile.astype('float32') / 255` bit for
 *                      bit -- the value the augmentation kernels and TileStore.__getitem__ give too; byte * (1/255) is not (126 codes
 *                      differ in the last bit).  bf16 storage rounds that quotient to nearest even.  divisor > 0.
 *   biu_u8_to_f32    : uint8 / divisor -> fp32, the same quotient (targets: masks are stored 0 / 255, and 255 / 255 is exactly 1)
 *   biu_quantize_u8  : (p * scale) truncated to uint8 -- `(res * 255).astype('uint8')`, unet/predict.py:200
 *   biu_stitch_add   : one patch [channels, pd, ph, pw] (uint8 or fp32) times an optional weight [pd, ph, pw] added into (set != 0:
 *                      written over) acc [channels, D, H, W] / wsum [D, H, W] at origin (z0, y0, x0); 2-D: D = pd = 1
 *   biu_stitch_finish: out = acc / wsum where wsum > 0 else 0 (fp32: the ramp blend of multi_output_unet3d/predict.py:300-303), or
 *                      floor(sum_layers acc / sum_layers wsum) as uint8 (the nan-mean of overlapping uint8 tiles cast to uint8,
 *                      unet/predict.py:204-229; `layers` = 3 reproduces unet3d/predict.py:173-195)
 * ---------------------------------------------------------------------------------------------- */
int biu_from_nchw_u8(const uint8_t* src, float divisor, const biu_act* dst, int dtype, biu_stream stream);
int biu_u8_to_f32(const uint8_t* src, float divisor, float* dst, long long n, biu_stream stream);
int biu_quantize_u8(const float* src, float scale, uint8_t* dst, long long n, biu_stream stream);
int biu_stitch_add(const void* patch, int patch_is_u8, const float* weight, int channels, int pd, int ph, int pw, float* acc, float* wsum,
                   int D, int H, int W, int z0, int y0, int x0, int set, biu_stream stream);
int biu_stitch_finish(const float* acc, const float* wsum, int layers, int channels, long long spatial, void* out, int out_is_u8,
                      biu_stream stream);

/* ------------------------------------------------------------------------------------------------
 * The front of the Predict pipelines: percentile clip, rescale and tiling of the raw stack on the device (the numpy stage of
 * unet/predict.py:122-181, unet3d/predict.py:97-150, siam_unet/predict.py:98-170, multi_output_unet/predict.py:129-181,
 * multi_output_unet3d/predict.py:99-160).  Everything is enqueued on `stream`; nothing synchronises.
 *
 *   biu_order_stats  : exact order statistics.  x holds `segments` runs of n elements of type `elem`, run s starting at element
 *                      s * stride (stride = n: the array cut into equal parts; stride < n: overlapping windows, as the frame pairs of
 *                      the Siamese predictor).  out[s * nranks + r] = the value at 0-based position ranks[r] of run s in sorted order,
 *                      as fp64 (ranks is a host array, the same for every run; nranks <= 8).  float32 sorts as np.sort does: IEEE order
 *                      (-0.0 and +0.0 compare equal to the caller), NaN last.  *nan_count (device) = NaN elements met, summed over
 *                      the runs; 0 for integer input.  Radix select on an order-preserving 32-bit key, 8 bits per pass, integer
 *                      atomics only: the result is deterministic.  workspace: biu_order_stats_workspace(segments, nranks) bytes of
 *                      device memory, 256-byte aligned.  n <= 2^31, segments <= 65535.
 *   biu_prep_finalize: stats [units][6] = minimum, maximum, x_k, x_k+1 of the lower percentile, x_k, x_k+1 of the upper (k =
 *                      floor(q/100 * (n - 1)), and k + 1 replaced by k where q/100 * (n - 1) >= n - 1) -> scalars [units][4] = lo, hi, sub,
 *                      den.  lo / hi restate np.percentile(method='linear') in fp64 bit for bit; the fused kernel then computes
 *                      (clip(v, lo, hi) - sub) / den:
 *                        BIU_PREP_MINMAX      sub = min(clip), den = max(clip) - min(clip)           (unet, unet3d, siam_unet, multi_output_unet)
 *                        BIU_PREP_MINMAX_EPS  the same with den + 1e-8                               (multi_output_unet3d 'single')
 *                        BIU_PREP_LOHI_EPS    sub = lo, den = hi - lo + 1e-8                         (multi_output_unet3d 'first' / 'all')
 *   biu_prep_tiles   : src [planes][height][width] of type `elem`; origins (device) = ntiles records (unit, z0, y0, x0); tile t is
 *                      out[t][td][th][tw] read from planes z0.., rows y0.., columns x0.. and normalised with scalars[unit].  `depth`
 *                      divides planes: a tile stays inside the block of `depth` planes that holds z0 (2-D stacks: depth = td = 1).
 *                      Beyond the source, pad_zero = 0 reflects as numpy 'reflect' does (no edge repeat, period 2 (n - 1), repeatedly),
 *                      pad_zero != 0 writes 0.  out_f32 = 0: uint8, `(a * 255)` (`255 - a * 255` with invert) truncated; out_f32 != 0:
 *                      float32, rounded once from fp64.  Pixel arithmetic is fp64, one rounding per operation, never contracted.
 * ---------------------------------------------------------------------------------------------- */
enum { BIU_ELEM_U8 = 0, BIU_ELEM_U16 = 1, BIU_ELEM_I16 = 2, BIU_ELEM_F32 = 3 };
enum { BIU_PREP_MINMAX = 0, BIU_PREP_MINMAX_EPS = 1, BIU_PREP_LOHI_EPS = 2 };
size_t biu_order_stats_workspace(long long segments, int nranks);
int biu_order_stats(const void* x, int elem, long long segments, long long n, long long stride, const long long* ranks, int nranks,
                    double* out, long long* nan_count, void* workspace, size_t workspace_bytes, biu_stream stream);
int biu_prep_finalize(const double* stats, int units, long long n, double q_lo, double q_hi, int family, double* scalars,
                      biu_stream stream);
int biu_prep_tiles(const void* src, int elem, int planes, int depth, int height, int width, const int* origins, int ntiles, int td, int th,
                   int tw, const double* scalars, int units, int pad_zero, int out_f32, int invert, void* out, biu_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Training data preparation: the mask edit and the mask half of the tile split of the reference's DataProcess (unet/data.py:124-215,
 * unet3d/data.py:116-207, siam_unet/data.py:126-233) on uint8 planes [planes][height][width], contiguous.  Everything is integer-exact,
 * enqueued on `stream`, and the caller owns all memory.  src and dst must not overlap (biu_lut_u8 excepted: it may run in place).
 *
 *   biu_lut_u8         : dst[i] = lut[src[i]] -- every pointwise step of the mask edit (binarise, threshold, invert, x 255) or a chain of
 *                        them as one 256-entry table (device memory).
 *   biu_morph_u8       : grey erosion (op = BIU_MORPH_ERODE, minimum) or dilation (BIU_MORPH_DILATE, maximum) per plane.  Footprints:
 *                        BIU_FOOT_DISK, size = r in 1..7: {(dy, dx): dy^2 + dx^2 <= r^2}; BIU_FOOT_SQUARE, size = w in 1..15: per axis the
 *                        offsets [-(w/2), w/2] for odd w, and for even w scipy.ndimage's convention: erosion [-w/2, w/2 - 1], dilation
 *                        [-(w/2 - 1), w/2].  Border: scipy's mode='reflect' (the edge pixel repeated: -1 -> 0, -2 -> 1, n -> n - 1),
 *                        applied literally.  Larger footprints are refused (BIU_ERR_UNSUPPORTED).
 *   biu_thin_step_u8   : one sub-iteration (sub = 0 | 1) of Zhang-Suen thinning: src holds 0 / 1 bytes (nonzero counts as set), pixels
 *                        outside a plane are 0, every pixel is judged on src, dst is written in full (0 / 1).  table (device, 256 bytes):
 *                        entry n = neighbourhood code with bit 0 = P2 (north), then clockwise P3 (NE) .. P9 (NW) in bits 1..7; bit `sub`
 *                        of the entry set = a set pixel with this neighbourhood is cleared in that sub-iteration.  *cleared (device) is
 *                        incremented by the number of pixels the launch cleared (integer atomic; the caller zeroes it).
 *   biu_tile_gather_u8 : the mask twin of biu_prep_tiles: origins (device) = ntiles records (ignored, z0, y0, x0); tile t is
 *                        out[t][td][th][tw] read from planes z0.., rows y0.., columns x0.. inside the block of `depth` planes that holds
 *                        z0, reflecting beyond the source as numpy 'reflect' does; invert != 0 writes 255 - v.
 * ---------------------------------------------------------------------------------------------- */
enum { BIU_MORPH_ERODE = 0, BIU_MORPH_DILATE = 1 };
enum { BIU_FOOT_DISK = 0, BIU_FOOT_SQUARE = 1 };
int biu_lut_u8(const uint8_t* src, const uint8_t* lut, uint8_t* dst, long long n, biu_stream stream);
int biu_morph_u8(const uint8_t* src, uint8_t* dst, int planes, int height, int width, int op, int footprint, int size, biu_stream stream);
int biu_thin_step_u8(const uint8_t* src, uint8_t* dst, int planes, int height, int width, int sub, const uint8_t* table,
                     unsigned long long* cleared, biu_stream stream);
int biu_tile_gather_u8(const uint8_t* src, int planes, int depth, int height, int width, const int* origins, int ntiles, int td, int th,
                       int tw, int invert, uint8_t* out, biu_stream stream);

/* ------------------------------------------------------------------------------------------------
 * On-the-fly training augmentation of uint8 tile batches (the albumentations pipelines of unet/data.py:217-245,
 * siam_unet/data.py:236-243, unet3d/data.py:209-239, which the reference runs offline)
 *
 * One record per sample, drawn on the host, shared by every field of the sample.  `m` is the INVERSE map of the composed rot90 and
 * shift/scale/rotate: output pixel x, y samples the source at sx = m[0] x + m[1] y + m[2], sy = m[3] x + m[4] y + m[5] (bilinear for
 * images, nearest for masks, reflect-101 outside).  It is double precision and so is the kernel's coordinate and interpolation arithmetic:
 * in fp32 the coordinate error (1e-5 pixel at 256^2) moves 0.07 % of a noise image's pixels across a rounding tie, and a later stage with a
 * gain above 1 (alpha, mult_noise) turns that grey level into two; in fp64 the gather agrees with a float64 restatement.
 * The kernel reads flags, blur_k, index, m, alpha, beta, noise_a, noise_b; the rest documents the draw (rot_k, angle in degrees, scale,
 * dx, dy as fractions of the tile).
 *   BIU_AUG_BC    : v * alpha + beta                        (beta on the 0..255 scale)
 *   BIU_AUG_BLUR  : blur_k x blur_k box mean, reflect-101  (odd, <= BIU_AUG_MAX_BLUR; stage order UNET only)
 *   BIU_AUG_MULT  : v * (noise_a + noise_b * u)             (stage order UNET)
 *   BIU_AUG_GAUSS : v + noise_a * N(0, 1)                   (stage order SIAM; Box-Muller)
 * Stage order UNET: gather, BC, BLUR, MULT.  SIAM (also the 3-D recipe, planes as channels): gather, GAUSS, BC.  The value is clipped to
 * [0, 255] and rounded to nearest-even after every stage.  Masks (is_mask != 0) stop after the gather.
 * Noise: Philox4x32-10, key = seed, counter = (element / 4 for MULT, element / 2 for GAUSS, params.index, epoch, field_id * 16 + stage)
 * with element = the pixel's index inside its sample's [planes, h, w] field; a MULT pixel takes word element % 4, a GAUSS pixel words
 * 2 (element % 2) and the next; uniform = (word >> 8) * 2^-24.
 *
 * biu_augment_u8: src, dst [n, planes, h, w] uint8 on the device, dst != src; params: n records on the device; max_blur_k: the largest
 *                 blur_k among the records whose BIU_AUG_BLUR is set (0: none -- the per-pixel kernel runs and a set bit is ignored).
 * biu_philox_u32: out[4 i .. 4 i + 3] = Philox4x32-10(counter = (c0 + i, c1, c2, c3), key = seed), i < blocks -- the raw stream.
 * ---------------------------------------------------------------------------------------------- */
#define BIU_AUG_GATE 1u   /* the sample passed the pipeline gate (informational) */
#define BIU_AUG_SSR 2u    /* shift/scale/rotate drawn (informational: it is part of m) */
#define BIU_AUG_BC 4u
#define BIU_AUG_BLUR 8u
#define BIU_AUG_MULT 16u
#define BIU_AUG_GAUSS 32u
#define BIU_AUG_ORDER_UNET 0
#define BIU_AUG_ORDER_SIAM 1
#define BIU_AUG_STAGE_MULT 1u
#define BIU_AUG_STAGE_GAUSS 2u
#define BIU_AUG_MAX_BLUR 15
typedef struct biu_aug_params {
    uint32_t flags, rot_k, blur_k, index;
    double m[6];
    float alpha, beta, noise_a, noise_b;
    float angle, scale, dx, dy;
} biu_aug_params;             /* 96 bytes */
int biu_augment_u8(const uint8_t* src, uint8_t* dst, int n, int planes, int h, int w, int is_mask, const biu_aug_params* params,
                   int stage_order, int max_blur_k, unsigned long long seed, unsigned epoch, unsigned field_id, biu_stream stream);
int biu_philox_u32(uint32_t* out, long long blocks, unsigned long long seed, unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                   biu_stream stream);

/* ------------------------------------------------------------------------------------------------
 * On-the-fly training augmentation of float fields: the 2-D multi-output family (multi_output_unet/data.py:187-311, which the
 * reference runs offline through scipy.ndimage.rotate and albumentations).  One launch per field per batch.
 *
 * src [n, planes, h, w]: float32, or uint8 (src_is_u8 != 0) widened on load as (float)byte / 255.0f (correctly rounded, the value
 * TileStore.__getitem__ yields).  dst: float32 of the same shape, never src.  One record per sample, drawn on the host:
 *   m : output pixel (x, y) samples the source at (m0 x + m1 y + m2, m3 x + m4 y + m5); fp64 coordinates and weights as for the uint8
 *       kernel.  Indices WRAP (scipy's mode='grid-wrap', cv2.BORDER_WRAP): i mod n.  Nearest is floor(c + 0.5).
 * kind:
 *   BIU_AUGF_IMAGE  : nearest gather, then BLUR -> SHOT -> GAUSS -> BC, each when its flag is set, in fp32
 *   BIU_AUGF_MASK   : any scalar target.  Bilinear gather when BIU_AUGF_ROT is set (an arbitrary-angle rotation), nearest otherwise;
 *                     nothing else
 *   BIU_AUGF_VECTOR : planes even; plane pairs (c, s) = (cos phi, sin phi).  Both planes are gathered nearest at the same source pixel
 *                     and the pair is rotated with the record's rotation t: (c cos_t + s sin_t, s cos_t - c sin_t).  The host writes exact
 *                     0 / +-1 for quarter turns, so those are sign-and-swap, bit for bit.
 * Stages (IMAGE):
 *   BIU_AUGF_BLUR  : blur_k x blur_k box mean (odd, <= BIU_AUG_MAX_BLUR) of the GATHERED image: the halo continues the affine map (and
 *                    wraps in the source); fp32 sums, first k along x, then k along y, times 1 / k^2
 *   BIU_AUGF_SHOT  : lin = v^2.2, lambda = lin / shot_s, n ~ Poisson(lambda), v = clip(n shot_s, 0, 1)^(1 / 2.2).
 *                    lambda < 32: inversion with ONE uniform u: p = exp(-lambda), cdf = p, n = 0;
 *                      while (u >= cdf && n < BIU_AUGF_POISSON_CAP && (n < lambda || p > 2^-32)) { ++n; p *= lambda / n; cdf += p; }
 *                    otherwise n = max(0, floor(lambda + sqrt(lambda) z + 0.5)), z one Box-Muller normal
 *   BIU_AUGF_GAUSS : v = clip(v + gauss_sigma z, 0, 1)
 *   BIU_AUGF_BC    : v = clip(v alpha + beta, 0, 1)
 * Per-pixel randomness as for the uint8 kernel: Philox4x32-10, key = seed, counter = (element / 2, index, epoch, field_id * 16 + stage)
 * with stage BIU_AUGF_STAGE_SHOT | BIU_AUGF_STAGE_GAUSS; element % 2 picks words (0, 1) or (2, 3): u1, u2 = (word >> 8) * 2^-24,
 * z = sqrt(-2 ln(1 - u1)) cos(2 pi u2); the inversion uses u1.
 * The kernel reads flags, blur_k, index, m, cos_t .. gauss_sigma; rot_k, angle (degrees), scale and dx, dy (whole pixels) document the draw.
 * max_blur_k: the largest blur_k among the records whose BIU_AUGF_BLUR is set (0: none -- the per-pixel kernel runs, a set bit is ignored).
 * ---------------------------------------------------------------------------------------------- */
#define BIU_AUGF_IMAGE 0
#define BIU_AUGF_MASK 1
#define BIU_AUGF_VECTOR 2
#define BIU_AUGF_ROT 1u     /* an arbitrary-angle rotation is part of m: MASK fields are gathered bilinearly */
#define BIU_AUGF_SCALE 2u   /* informational: scale and crop offset are part of m */
#define BIU_AUGF_BLUR 4u
#define BIU_AUGF_SHOT 8u
#define BIU_AUGF_GAUSS 16u
#define BIU_AUGF_BC 32u
#define BIU_AUGF_STAGE_SHOT 3u
#define BIU_AUGF_STAGE_GAUSS 4u
#define BIU_AUGF_POISSON_CAP 128
typedef struct biu_augf_params {
    uint32_t flags, rot_k, blur_k, index;
    double m[6];
    float cos_t, sin_t, alpha, beta, shot_s, gauss_sigma;
    float angle, scale, dx, dy;
} biu_augf_params;            /* 104 bytes */
int biu_augment_f32(const void* src, int src_is_u8, float* dst, int n, int planes, int h, int w, int kind, const biu_augf_params* params,
                    int max_blur_k, unsigned long long seed, unsigned epoch, unsigned field_id, biu_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Cubic-spline resampling of MASK fields under an arbitrary-angle rotation: what the reference computes with
 * scipy.ndimage.rotate(order=3, mode='grid-wrap') followed by its clip (multi_output_unet/data.py:213-242).  Opt-in; two calls replace
 * the one biu_augment_f32(kind = BIU_AUGF_MASK) call of a field.  src, n, planes, h, w, params: as for biu_augment_f32.
 *
 * biu_spline_prefilter_f32, for every sample whose record has BIU_AUGF_ROT (the others' coef and range are left unspecified):
 *   coef [n, planes, h, w] : coefficients of the periodic cubic B-spline through the loaded values s, per plane, separable, x then y:
 *                              c[k] = sum over |j| <= BIU_SPLINE_R of sqrt(3) z^|j| s[(k - j) mod len],   z = sqrt(3) - 2
 *                            the exact prefilter of 'grid-wrap' is the same sum over all integers j; the dropped tail is at most
 *                            2 sqrt(3) |z|^(R + 1) / (1 - |z|) = 9.0e-10 of max |s| per axis at R = 16, below 2^-26.  fp32 taps (the fp64
 *                            values rounded once) and fp32 sums: s[k - j] + s[k + j] is formed first, terms are added from |j| = R inwards.
 *   range [n, 2]           : lo = min, hi = max of the sample's loaded values over all planes (NaN aside), exact
 * biu_augment_f32_cubic writes dst [n, planes, h, w], never src, coef or range:
 *   records with BIU_AUGF_ROT : at the fp64 source coordinate (sx, sy) of m, x0 = floor(sx), t = sx - x0, the taps x0 - 1 .. x0 + 2 carry
 *                            the weights (1 - t)^3 / 6, (3 t^3 - 6 t^2 + 4) / 6, (-3 t^3 + 3 t^2 + 3 t + 1) / 6, t^3 / 6, evaluated in fp64 and
 *                            rounded once to fp32; likewise in y; v = sum of 4 x 4 coefficients (every index wraps) in fp32, rows first.
 *                            Then the reference's clip: v = min(max(v, lo), hi) if lo >= 0 and hi <= 1, no clip otherwise.
 *   other records          : biu_augment_f32's MASK output (nearest gather from src), bit for bit; coef and range are not read.
 * Three launches (range, prefilter, gather) on `stream`; no atomics, nothing cleared beforehand.  Null pointers, buffers that overlap
 * (src, coef, range among each other; dst with any of them), unaligned float pointers, non-positive extents and 2^31 elements or more
 * return a status and launch nothing.
 * ---------------------------------------------------------------------------------------------- */
#define BIU_SPLINE_R 16      /* the prefilter's taps reach |j| <= 16 per axis */
int biu_spline_prefilter_f32(const void* src, int src_is_u8, float* coef, float* range, int n, int planes, int h, int w,
                             const biu_augf_params* params, biu_stream stream);
int biu_augment_f32_cubic(const void* src, int src_is_u8, const float* coef, const float* range, float* dst, int n, int planes, int h, int w,
                          const biu_augf_params* params, biu_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Crop augmentation of whole items: biu_augment_f32 with the source in an arena of whole images (feed.ImageStore.to_device) instead of
 * a batch of stored tiles.  One launch per field per batch renders dst [n, planes, th, tw] (float32) straight from the arena.
 *
 * arena: arena_elems elements, float32 or uint8 (arena_is_u8 != 0, widened as (float)byte / 255.0f); the items of one field one after
 * the other, each [planes, h_i, w_i].  sources[s] names sample s's item: its element offset in THIS field's arena and its extent.
 * params[s] is biu_augf_params unchanged; m maps an output-tile pixel (x, y) to a coordinate in the ITEM, and every index wraps in the
 * item's own (h, w), however often a small item needs it.  Index math inside an item is 32-bit (planes h w < 2^31 - 4), the offset 64-bit.
 * A sample whose source does not lie inside the arena (or breaks the 32-bit bound) is rendered as nan_to_val; nothing outside the arena is read.
 *
 * Kinds, stages, samplers and the Philox counter are biu_augment_f32's; the element of the noise counter is the pixel's index inside the
 * output tile's field, (p th + y) tw + x.  The blur halo is more gathered item through the same map and wrap.
 *
 * NaN in a MASK or VECTOR item means "no label"; dst never holds NaN (nan_to_val itself must not be NaN):
 *   MASK, nearest    : a NaN source pixel gives nan_to_val
 *   VECTOR           : if either plane of the pair is NaN at the source pixel, both outputs are nan_to_val and no rotation is applied
 *   MASK, bilinear   : the four taps are read with NaN replaced by 0; w_nan = the sum of the fp64 weights (1 - ax)(1 - ay), ax (1 - ay),
 *                      (1 - ax) ay, ax ay of the NaN taps; the output is nan_to_val if w_nan >= 0.5, else the interpolated value of the
 *                      zero-filled taps (the reference's rotate_array at order = 1: scipy rounds the rotated uint8 NaN mask half up before
 *                      its > 0.5 test)
 *   IMAGE            : finite by the store's contract; NaN is not special-cased
 *
 * Equivalence law.  For items whose (h, w) equals (th, tw), the output equals biu_augment_f32 on the batch of those items for the same
 * records bit for bit, for every kind, on NaN-free data.  One exception: where tw % 4 == 0 and dst is 16-byte aligned, biu_augment_f32
 * rotates a VECTOR pair with the cos_t product fused into the sum, and this entry point rounds both products as biu_augment_f32 does on
 * its other path; under an arbitrary angle (cos_t, sin_t not in {0, 1, -1}) the two then differ by that one rounding.
 *
 * Null pointers, dst overlapping the arena or the records, unaligned float or record pointers, non-positive extents, field_id >= 2^28,
 * an output of 2^31 - 4 elements or more and a NaN nan_to_val return a status and launch nothing.  No atomics, no scratch.
 * ---------------------------------------------------------------------------------------------- */
typedef struct biu_augf_source {
    uint64_t offset;          /* element offset of the item in this field's arena */
    int32_t h, w;             /* the item's extent */
} biu_augf_source;            /* 16 bytes */
int biu_augment_f32_crop(const void* arena, int arena_is_u8, unsigned long long arena_elems, float* dst, int n, int planes, int th, int tw,
                         int kind, const biu_augf_params* params, const biu_augf_source* sources, float nan_to_val, int max_blur_k,
                         unsigned long long seed, unsigned epoch, unsigned field_id, biu_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Cubic-spline resampling of the MASK fields of whole items: biu_spline_prefilter_f32 + biu_augment_f32_cubic with the source in an arena
 * (above), and with the reference's exact semantics (rotate_array at order = 3, multi_output_unet/data.py:213-242): the periodic spline of
 * the whole item, the clip range of the whole item, and NaN carried through the rotation.  What depends on the item alone -- coefficients,
 * range, "holds a NaN" -- is computed once per store (biu_spline_prefilter_items) and read by every batch (biu_augment_f32_crop_cubic).
 *
 * biu_spline_prefilter_items: the tables of n_items items of ONE field's arena (arena, arena_is_u8, arena_elems, planes: as above).
 *   items     : n_items biu_augf_source records IN HOST MEMORY (the others are device pointers): each item's element offset and extent.
 *               Every item is checked before the first launch: one that does not lie inside the arena, or has planes h w >= 2^31 - 4,
 *               returns a status and nothing is launched.
 *   table     : n_items biu_spline_item on the device, 16-byte aligned; always written:
 *                 lo, hi  : min and max of the item's loaded values over all planes, NaN aside, exact (bytes: the min and max of the bytes,
 *                           divided by 255.0f once); an item that holds nothing but NaN gives lo = +inf, hi = -inf
 *                 has_nan : 1 if some element of the item is NaN, else 0 (a byte arena: always 0)
 *   coef      : arena_elems floats with the arena's layout and offsets (or null: not computed): per item and plane the coefficients of
 *               the periodic cubic B-spline through the loaded values with NaN read as 0 -- biu_spline_prefilter_f32's definition (cut at
 *               BIU_SPLINE_R, fp32 taps, symmetric pairs added first, outermost first, x then y); indices wrap in the item's own (h, w), as
 *               often as a small item needs.  Elements of the arena that belong to no item are not written.
 *   indicator : the same spline through isnan(item) as 0 / 1 (or null: not computed).  Written only for the items whose has_nan is 1; the
 *               others' elements are left as they are and are never read by the gather.  A caller reads the table after a first call with
 *               indicator = null and needs no indicator arena at all if no item holds a NaN.  At least one of coef and indicator is given.
 * Up to three launches per item on `stream` (range, value prefilter, indicator prefilter); no atomics, nothing cleared beforehand.
 *
 * biu_augment_f32_crop_cubic renders dst [n, planes, th, tw] of one MASK field; params, sources, nan_to_val and the validation of a
 * sample's source are biu_augment_f32_crop's.  item_index [n] (device, int32) names the row of each sample's item in `table`; a sample
 * whose index is outside 0 .. n_items - 1 is rendered as nan_to_val, as is one whose source does not lie inside the arena.
 *   records without BIU_AUGF_ROT : biu_augment_f32_crop's MASK output bit for bit (nearest gather from the arena, NaN -> nan_to_val);
 *                                  coef, indicator and the table are not read.
 *   records with BIU_AUGF_ROT    : biu_augment_f32_cubic's gather at the crop's one affine map m: fp64 coordinate and fraction, the four
 *                                  B-spline weights per axis in fp64 rounded once, v = the sum of 4 x 4 wrapped coefficients in fp32, rows
 *                                  first.  If the item's has_nan is set and indicator is not null, w_nan = the same sum over the indicator
 *                                  coefficients, and the output is nan_to_val if w_nan >= 0.5 (scipy rounds the rotated uint8 NaN mask half
 *                                  up before the reference's > 0.5 test).  Otherwise the output is v, clipped to the item's [lo, hi] iff
 *                                  lo >= 0 and hi <= 1.
 * dst never holds NaN; an item of nothing but NaN renders nan_to_val everywhere (its indicator coefficients sum to 1).
 * Equivalence law: NaN-free items of exactly (th, tw) with the same record bytes give biu_augment_f32_cubic's bytes.
 *
 * Both: null pointers (but a null coef or indicator where it is optional), buffers that overlap (the arena, coef, indicator and the table
 * among each other; dst with any input), unaligned pointers, non-positive extents, an output of 2^31 - 4 elements or more and a NaN
 * nan_to_val return a status and launch nothing.
 * ---------------------------------------------------------------------------------------------- */
typedef struct biu_spline_item {
    float lo, hi;             /* the item's value range over all planes, NaN aside */
    uint32_t has_nan;         /* 1: some element is NaN */
    uint32_t reserved;        /* written as 0 */
} biu_spline_item;            /* 16 bytes */
int biu_spline_prefilter_items(const void* arena, int arena_is_u8, unsigned long long arena_elems, float* coef, float* indicator,
                               biu_spline_item* table, int n_items, int planes, const biu_augf_source* items, biu_stream stream);
int biu_augment_f32_crop_cubic(const void* arena, int arena_is_u8, unsigned long long arena_elems, const float* coef, const float* indicator,
                               const biu_spline_item* table, int n_items, const int32_t* item_index, float* dst, int n, int planes, int th,
                               int tw, const biu_augf_params* params, const biu_augf_source* sources, float nan_to_val, biu_stream stream);

/* ------------------------------------------------------------------------------------------------
 * On-the-fly training augmentation of float volumes: the 3-D multi-output family (multi_output_unet3d/data.py:152-178, which the
 * reference runs offline through albumentations).  One launch per field per batch; the records are biu_augf_params unchanged.
 *
 * src [n, channels, depth, h, w]: float32, or uint8 (src_is_u8 != 0) widened on load as (float)byte / 255.0f.  dst: float32 of the same
 * shape, never src.  Every z-plane of every channel gets the record's in-plane map m (any m; fp64 coordinates and weights).  Nothing
 * wraps; `border` says what lies outside a plane:
 *   BIU_AUGV_REFLECT  : reflect-101 (d c b | a b c d | c b a) at any distance from the image
 *   BIU_AUGV_CONSTANT : taps outside the image read 0 and keep their bilinear weight
 * kind:
 *   BIU_AUGF_IMAGE  : bilinear gather, then BC -> BLUR -> SHOT -> GAUSS, each when its flag is set, in fp32:
 *                       BC    : v = clip(v alpha + beta, 0, 1), product and sum rounded one after the other
 *                       BLUR  : blur_k x blur_k box mean (odd, <= BIU_AUG_MAX_BLUR) of BC(gather).  Pixels outside the plane are the
 *                               reflect-101 of that OUTPUT plane whatever `border` says (cv2.blur's default border); fp32 sums, first k
 *                               along x, then k along y, times 1 / k^2
 *                       SHOT, GAUSS : biu_augment_f32's arithmetic, samplers, stage ids and Philox counter; the element is the voxel's
 *                               index inside the sample's channels x depth x h x w field
 *   BIU_AUGF_MASK   : any scalar target: nearest gather floor(c + 0.5), nothing else
 *   BIU_AUGF_VECTOR : channels even; the pair (c, s) is channels (2j, 2j + 1), depth x h x w apart.  Both are gathered nearest at one
 *                     source voxel, then (c cos_t + s sin_t, s cos_t - c sin_t)
 * The kernel reads flags (BLUR | SHOT | GAUSS | BC), blur_k, index, m, cos_t, sin_t, alpha, beta, shot_s and gauss_sigma.
 * max_blur_k: as for biu_augment_f32.  2^31 elements or more, field_id >= 2^28 and every other argument error return a status and launch nothing.
 * ---------------------------------------------------------------------------------------------- */
#define BIU_AUGV_REFLECT 0   /* reflect-101: d c b | a b c d | c b a, any distance from the image */
#define BIU_AUGV_CONSTANT 1  /* taps outside the image read 0 and keep their bilinear weight */
int biu_augment_vol_f32(const void* src, int src_is_u8, float* dst, int n, int channels, int depth, int h, int w,
                        int kind, int border, const biu_augf_params* params, int max_blur_k,
                        unsigned long long seed, unsigned epoch, unsigned field_id, biu_stream stream);
/* How that launch would be cut, without launching: the planes (VECTOR: pairs of planes) a lane walks with one set of taps, or, with
 * max_blur_k > 1, a block of the blurring path walks; 1 .. 16, the last chunk of a field may be shorter.  dst_aligned16: dst % 16 == 0.
 * 0 for dimensions, a kind or a max_blur_k the launch refuses.  For tests and tools, so that they can say which loop a shape ran. */
int biu_augment_vol_chunk(int n, int channels, int depth, int h, int w, int kind, int max_blur_k, int dst_aligned16);

/* ------------------------------------------------------------------------------------------------
 * Crop augmentation of whole volumes: biu_augment_vol_f32 with the source in an arena of whole volumes (feed.VolumeStore.to_device)
 * instead of a batch of stored tiles: the reference's ShiftScaleRotate of the whole volume followed by RandomCrop3D(dim_out)
 * (multi_output_unet3d/data.py:152-230).  One launch per field per batch renders dst [n, channels, td, th, tw] (float32).
 *
 * arena: arena_elems elements, float32 or uint8 (arena_is_u8 != 0, widened as (float)byte / 255.0f); the items of one field one after
 * the other, each [channels, d_i, h_i, w_i].  sources[s] names sample s's item -- its element offset in THIS field's arena and its
 * extent -- and the first z-plane z0 of the crop.  params[s] is biu_augf_params unchanged.
 *
 * Gather.  Output voxel (c, z, y, x) of sample s reads plane (c, z0 + z) of the item at the in-plane coordinate m (x, y, 1): m is the
 * fp64 2x3 map from TILE pixel to ITEM pixel, i.e. the whole-plane shift-scale-rotate map about the centre of the item's (h, w) plane
 * (augment._matrix's sign) composed with the crop origin (ox, oy) (augment.vol_crop_matrix).  Nothing wraps; `border` (BIU_AUGV_REFLECT /
 * BIU_AUGV_CONSTANT) applies in the ITEM's (h, w), exactly as in biu_augment_vol_f32.  z is never resampled.
 *
 * Kinds, stages, samplers, stage ids and the Philox counter are biu_augment_vol_f32's: IMAGE is bilinear in fp64, then BC (product and sum
 * rounded one after the other) -> BLUR -> SHOT -> GAUSS; the blur's halo is the reflect-101 of the OUTPUT tile th x tw (cv2.blur on the
 * cropped patch), and the noise element is the voxel's index inside the OUTPUT sample's field, ((c td + z) th + y) tw + x.  MASK is
 * nearest.  VECTOR takes channel pairs (2j, 2j + 1), a whole item volume d h w apart, gathers both nearest at one voxel, then rotates by
 * (cos_t, sin_t).
 *
 * NaN in a MASK or VECTOR item means "no label"; dst never holds NaN (nan_to_val itself must not be NaN):
 *   MASK    : a NaN source voxel gives nan_to_val
 *   VECTOR  : if either plane of the pair is NaN at the source voxel, both outputs are nan_to_val and no rotation is applied
 *   IMAGE   : finite by the store's contract; NaN is not special-cased
 * A constant-border tap outside the plane reads 0, as in biu_augment_vol_f32, not nan_to_val.
 *
 * Equivalence law.  For an item whose (d, h, w) equals (td, th, tw), with z0 = 0 and origin (0, 0), the output equals biu_augment_vol_f32 on
 * that item for the same record bit for bit, for every kind and border, on NaN-free data.
 *
 * Safety.  The item base is a 64-bit offset, index math inside an item is 32-bit.  Per sample the kernel checks d, h, w > 0,
 * channels d h w < 2^31 - 4, 0 <= z0, z0 + td <= d and that the item lies inside [arena, arena + arena_elems); a sample that fails is
 * rendered as nan_to_val, and nothing outside the arena is ever read.  Null pointers, dst overlapping the arena or the records,
 * unaligned float, record or source pointers, non-positive extents, an unknown kind or border, odd VECTOR channels,
 * max_blur_k > BIU_AUG_MAX_BLUR, field_id >= 2^28, an output of 2^31 elements or more and a NaN nan_to_val return a status and launch
 * nothing.  No atomics, no scratch.
 *
 * The launch is cut as biu_augment_vol_f32 is, from the OUTPUT shape: biu_augment_vol_chunk(n, channels, td, th, tw, kind, max_blur_k,
 * dst_aligned16) answers for this launch too.
 * ---------------------------------------------------------------------------------------------- */
typedef struct biu_augv_source {
    uint64_t offset;          /* element offset of the item [channels, d, h, w] in this field's arena */
    int32_t d, h, w;          /* the item's extent */
    int32_t z0;               /* first z-plane of the crop */
} biu_augv_source;            /* 24 bytes */
int biu_augment_vol_f32_crop(const void* arena, int arena_is_u8, unsigned long long arena_elems, float* dst,
                             int n, int channels, int td, int th, int tw, int kind, int border,
                             const biu_augf_params* params, const biu_augv_source* sources, float nan_to_val,
                             int max_blur_k, unsigned long long seed, unsigned epoch, unsigned field_id, biu_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Fused multi-tensor Adam                                                              [K14]
 * replaces torch.optim.Adam(lr) step: unet/train.py:102,139 (betas 0.9/0.999, eps 1e-8, no decay).
 * One launch updates `n` parameter tensors; ptrs are device arrays of device pointers.
 * ---------------------------------------------------------------------------------------------- */
int biu_adam_step(int n, float* const* params, const float* const* grads, float* const* exp_avg,
                  float* const* exp_avg_sq, const int64_t* numel, float lr, float beta1, float beta2,
                  float eps, int step, float grad_scale, biu_stream stream);

/* The same update with its scalars in device memory, for a step captured in a hipGraph (bio_image_unet_amd/graph.py): the graph holds
 * biu_adam_step_hyper, and biu_adam_set_hyper -- launched in front of every replay, arguments by value -- writes
 * hyper[6] = {lr, beta1, beta2, eps, grad_scale, step} for the step being replayed (ReduceLROnPlateau of unet/train.py:103 keeps working). */
int biu_adam_set_hyper(float* hyper, float lr, float beta1, float beta2, float eps, int step, float grad_scale, biu_stream stream);
int biu_adam_step_hyper(int n, float* const* params, const float* const* grads, float* const* exp_avg,
                        float* const* exp_avg_sq, const int64_t* numel, const float* hyper, biu_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Gradient-norm clipping over a table of fp32 tensors                                     [K14b]
 * replaces torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0): multi_output_unet3d/train.py:201.
 *   total = sqrt(sum_i |g_i|^2), coef = min(1, max_norm / (total + 1e-6)), g_i *= coef in place (three launches, sums in a fixed order).
 * grads / numel: device arrays as for biu_adam_step; scratch: biu_grad_clip_scratch_floats(n) floats of device memory;
 * total_norm: one device float receiving the norm before clipping, or NULL.
 * ---------------------------------------------------------------------------------------------- */
size_t biu_grad_clip_scratch_floats(int n);
int biu_grad_clip(int n, float* const* grads, const int64_t* numel, float max_norm, float* scratch, size_t scratch_floats, float* total_norm,
                  biu_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* BIU_H */
