/*
 * faoctasr.h -- C ABI of the MI355X (gfx950) kernels behind the frequency-aware OCTA
 * super-resolution train step.
 *
 * The reference has no native code: its hot path (train.py:166-269) runs stock ATen
 * ops from Python.  These entry points are what a binding for that path would bind,
 * one per ATen op class the path executes.  Conventions:
 *   - every tensor is a raw DEVICE pointer to contiguous fp32 NCHW data owned by the caller;
 *   - `stream` is a hipStream_t passed as void*; kernels are only enqueued: no allocation,
 *     no synchronisation, no host read-back (safe under hipGraph capture);
 *   - workspaces are caller-provided (sizes from the *_workspace_floats queries);
 *   - return 0 on success, negative on error; faoctasr_last_error() gives the thread-local text.
 * Each function cites the reference call site(s) it stands in for (paths under /root/reference).
 */
#ifndef FAOCTASR_H
#define FAOCTASR_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void* faoctasr_stream_t;

enum { FAOCTASR_ACT_NONE = 0, FAOCTASR_ACT_RELU = 1, FAOCTASR_ACT_LRELU = 2, FAOCTASR_ACT_TANH = 3 };
enum { FAOCTASR_OK = 0, FAOCTASR_EINVAL = -1, FAOCTASR_EUNSUPPORTED = -2, FAOCTASR_EHIP = -3 };

int faoctasr_version(void);
const char* faoctasr_last_error(void);
/* diagnostics (bench.py's per-family roofline): the kernel family the calling thread's last convolution-type call went to:
 * 1 flat implicit GEMM, 2 LDS-patch implicit GEMM, 3 Winograd F(2x2,3x3), 4 bf16x3 split, 5 M=1 head (VALU), 6 narrow-map GEMM,
 * 7 stem input gradient (1..4 input channels, VALU), 8 narrow-map f16x2 GEMM (precision 3); 11 flat weight gradient, 12 LDS-patch weight gradient, 13 stride-1 / 4x4
 * stride-2 weight gradient (wgrad_s1), 14 M=1 weight gradient, 15 bf16x3 weight gradient (wgrad_x3), 16 stem weight gradient (VALU) */
int faoctasr_last_route(void);

/* ---- convolution family (implicit GEMM on f32 MFMA) --------------------------------------
 * nn.Conv2d forward: model.py:102,109,117,122 (discriminator), 242-244,250,258,275-277,286
 * (stems/skip), 412-414,438 (ResnetBlock, head), 451,458,473 (ResnetGenerator), 494,499.
 * y[N,M,OH,OW] = act(conv(x[N,C,IH,IW], w[M,C,KH,KW]) + bias); OH=(IH+2*pad-KH)/stride+1.
 * reflect!=0 folds nn.ReflectionPad2d(pad) (model.py:450,472) into the gather.          */
int faoctasr_conv2d_fwd(const float* x, const float* w, const float* bias, float* y,
                        int N, int C, int IH, int IW, int M, int KH, int KW, int stride, int pad,
                        int reflect, int act, float slope, float* wpack, int wpack_state, int precision,
                        faoctasr_stream_t stream);
/* Packed-weight images for the LDS-patch kernel.  Every gather-type call (conv2d_fwd/dgrad,
 * conv_transpose2d_fwd/dgrad) takes an optional caller-owned buffer `wpack` of
 * faoctasr_conv_wpack_floats(kind, C, M, KH, KW, stride, pad) floats (kind 0..3 in that order; C, M
 * as in the matching call) and `wpack_state`: 0 = none (flat im2col kernel), 1 = pack `w` into it
 * now, 2 = it already holds this `w` (valid until the weights change).
 * `precision`: 0 = exact fp32 on v_mfma_f32_32x32x2_f32 (Winograd F(2x2,3x3) on the dense stride-1 3x3 layers), 1 = the same
 * without Winograd, 3 = "f16x2" (below: faoctasr_conv_set_scales); 2 = "bf16x3": operands split hi/lo into bf16, three
 * v_mfma_f32_32x32x16_bf16 per product, fp32 accumulate (fp32-parity, ~5x the MFMA rate; needs a wpack buffer and
 * C >= 16, width >= 24 -- other shapes silently use the fp32 kernels).  The packed image depends on `precision` and on
 * whether the map is wide enough for the split kernel, so keep one buffer per (weights, precision, input size).
 * OR-ing FAOCTASR_CONV_NO_SPLIT_K into `precision` of a gather call keeps the whole reduction of an output element in one
 * block: no fp32 atomics, a bit-reproducible result, at the price of under-filled grids on narrow maps (the kernels otherwise
 * split K across blocks when a layer has fewer blocks than the chip has CUs).                                          */
#define FAOCTASR_CONV_NO_SPLIT_K 0x100
long faoctasr_conv_wpack_floats(int kind, int C, int M, int KH, int KW, int stride, int pad, int precision);
/* Batched packing: all packed-weight images of a step in ONE launch (csrc/conv_pack.hip).  Each convolution call of
 * train.py:166-269 re-reads weights the optimizer has just changed (train.py:239,268), i.e. ~240 images per step;
 * packed one by one they are ~240 tiny dependent launches.  faoctasr_conv_pack_job writes, into a HOST slot of
 * FAOCTASR_PACK_JOB_BYTES, the job that the gather call `kind` (0 conv2d_fwd, 1 conv2d_dgrad, 2 conv_transpose2d_fwd,
 * 3 conv_transpose2d_dgrad) with exactly these arguments and wpack_state 1 would launch; it returns the job's block
 * count (0: that call uses no packed image -- skip the slot; < 0: error).  `block_base` is the sum of the block counts
 * of the jobs before it.  The caller copies the slots, contiguous, to device memory once and calls
 * faoctasr_conv_pack_run(table, njobs, total_blocks, stream) after every weight update; the matching gather calls then
 * pass wpack_state 2.  `w` / `wpack` addresses are baked into the job.                                              */
#define FAOCTASR_PACK_JOB_BYTES 1024
long faoctasr_conv_pack_job(void* job_host, long block_base, int kind, const float* w, float* wpack,
                            int N, int C, int IH, int IW, int M, int KH, int KW, int stride, int pad,
                            int reflect, int out_pad, int precision);
int faoctasr_conv_pack_run(const void* jobs_dev, int njobs, long nblocks, faoctasr_stream_t stream);
/* precision 3 ("f16x2") tables only, BEFORE faoctasr_conv_pack_run on the same stream: the absmax slots of every job's weight
 * tensor (8 blocks per job, one partial maximum each, in the last 8 words of the job's image).                          */
int faoctasr_conv_pack_scales(const void* jobs_dev, int njobs, faoctasr_stream_t stream);
/* ---- precision 3, "f16x2": fp32-exact-class contraction at the 16-bit matrix-core rate ------------------------------
 * Every fp32 operand is split into hi = f16(x s), lo = f16(x s - hi) (22 significant bits) and a product is accumulated in
 * fp32 as hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16; s is the power of two that puts the operand tensor's largest
 * magnitude in [2^14, 2^15) and is divided out of the accumulators.  Measured against fp64 the result is at or below the
 * error of the exact-f32 MFMA kernels (csrc/split16.h, profiles/r04_split_precision_error.log), at ~5x their rate.
 * The largest magnitude of an ACTIVATION operand travels as its fp32 bit pattern in a caller-owned "absmax slot" of
 * FAOCTASR_ABSMAX_SLOT_WORDS device words (512 bytes; 8 of them are used, one per 64-byte line, so that the producers' atomics
 * do not queue on one address; a reader takes their maximum): zero the slot, then faoctasr_absmax_bits(x, n, slot) (atomicMax:
 * several calls may fold several tensors into one slot).  The slots of the next convolution-type call of the calling thread are handed over with
 * faoctasr_conv_set_scales(a, b): gather calls (conv2d_fwd / dgrad, conv_transpose2d_fwd / dgrad) read `a` = the slot of their
 * gathered tensor (x, resp. dy); weight-gradient calls read `a` = slot of x and `b` = slot of dy.  The call consumes them
 * (a precision-3 call without slots fails with FAOCTASR_EINVAL); the weights' own slot lives in the packed image.  Shapes
 * the split kernels do not take (maps narrower than 24, fewer than 16 channels) silently run on the exact-f32 kernels. */
#define FAOCTASR_ABSMAX_SLOT_WORDS 128
int faoctasr_absmax_bits(const float* x, long n, unsigned* slot, faoctasr_stream_t stream);
/* The producer's side of the same slot: the NEXT faoctasr_batchnorm_train_fwd (its y) / faoctasr_batchnorm_train_bwd (its dx) /
 * faoctasr_cat2_act_fwd (its y) call of the calling thread folds the largest magnitude of its output into `slot` (zeroed by the caller) in its own store loop, so
 * the convolution that reads that tensor needs no separate faoctasr_absmax_bits pass over it.  Map sizes (H*W) that are not a
 * multiple of 4 are refused (FAOCTASR_EUNSUPPORTED): use faoctasr_absmax_bits there.                                       */
int faoctasr_out_absmax(unsigned* slot);
int faoctasr_conv_set_scales(const unsigned* slot_a, const unsigned* slot_b);
/* Which slots the precision-3 form of a call reads: bit 0 = slot a, bit 1 = slot b, 0 = none (the shape runs on an exact-f32
 * kernel).  kind 0..3 as faoctasr_conv_pack_job (conv2d_fwd, conv2d_dgrad, conv_transpose2d_fwd, conv_transpose2d_dgrad),
 * 4 = conv2d_wgrad, 5 = conv_transpose2d_wgrad; the other arguments exactly as that call receives them.                      */
int faoctasr_conv_needs_scales(int kind, int N, int C, int IH, int IW, int M, int KH, int KW, int stride, int pad,
                               int reflect, int out_pad);
/* Two-pass weight-gradient reduction (precisions 2 and 3, the shapes the split kernels take): with a caller-owned, 16-byte aligned
 * workspace of faoctasr_conv_wgrad_workspace_floats(C, M, KH, KW, stride) floats handed over for the NEXT weight-gradient call of the
 * calling thread, every pixel range of the kernel stores its partial dW there (plain stores) and a second kernel adds them to dw
 * in a fixed order -- instead of one fp32 atomic per partial and element.  Faster (the atomics were 29 us of a 67 us launch on the
 * 256 -> 256 3x3 layer) and, with a step's weight gradients on one stream, bit-reproducible.  Without a workspace (or one that is
 * too small) the call accumulates with atomics as before.  The workspace is only used between the call's two launches: calls on
 * the same stream may share it.                                                                                            */
int faoctasr_conv_set_workspace(float* workspace, long nfloats);
/* The same hand-over for the NEXT gather call (conv2d_fwd / dgrad, conv_transpose2d_fwd / dgrad) at precision 3 whose route is the
 * f16x2 narrow-map kernel: with a workspace of faoctasr_conv_gather_workspace_floats(...) floats (kind 0..3 and the call's arguments as
 * faoctasr_conv_needs_scales) a small grid splits its reduction, every slice stores its partial there and a second kernel sums them in
 * a fixed order and applies bias, activation and residual -- no atomics, bit-reproducible.  Without one the grid is not split.      */
long faoctasr_conv_gather_workspace_floats(int kind, int N, int C, int IH, int IW, int M, int KH, int KW, int stride, int pad,
                                           int reflect, int out_pad);
/* y = gather(...) + residual for the NEXT gather call (conv2d_fwd / dgrad, conv_transpose2d_fwd / dgrad) of the calling thread;
 * `residual` has the output's shape.  x + conv_block(x) (model.py:420,505) sends two gradients to x -- the skip's and the first
 * convolution's input gradient -- and autograd adds them with an elementwise kernel (66 per train step); handing the skip's gradient
 * to that input-gradient call adds it in the split kernels' epilogue instead (other routes: one in-place pass after the kernel). */
int faoctasr_conv_set_residual(const float* residual);
long faoctasr_conv_wgrad_workspace_floats(int C, int M, int KH, int KW, int stride);
/* aten::convolution_backward, input gradient.  dx[N,C,IH,IW] from dy[N,M,OH,OW].  With
 * reflect!=0 dx is the gradient w.r.t. the PADDED input [N,C,IH+2p,IW+2p] (fold it with
 * faoctasr_reflect_pad_bwd).                                                              */
int faoctasr_conv2d_dgrad(const float* dy, const float* w, float* dx,
                          int N, int C, int IH, int IW, int M, int KH, int KW, int stride, int pad,
                          float* wpack, int wpack_state, int precision, faoctasr_stream_t stream);
/* aten::convolution_backward, weight gradient.  dw[M,C,KH,KW] is overwritten, or added to
 * when accumulate != 0 (the gradient arena is zeroed once per step instead).  precision as above: 2 = bf16x3 (hi/lo-split dY
 * and X on v_mfma_f32_32x32x16_bf16) for the stride-1 3x3 (pad 1) and 7x7 (pad 3, reflection or zero padding) layers and the
 * stride-2 3x3 / 4x4 (pad 1) layers, with C, M multiples of 64, an output width that is a multiple of 32 and an even output
 * height (the transposed convolution's weight gradient takes the stride-2 form with x and dy swapped); other shapes silently
 * use the fp32 kernels.  faoctasr_last_route() tells which (15 = bf16x3).                    */
int faoctasr_conv2d_wgrad(const float* x, const float* dy, float* dw,
                          int N, int C, int IH, int IW, int M, int KH, int KW, int stride, int pad,
                          int reflect, int accumulate, int precision, faoctasr_stream_t stream);
/* nn.ConvTranspose2d forward: model.py:431 (4x4 s2 p1), 469 (3x3 s2 p1 output_padding 1).
 * x[N,C,IH,IW], w[C,M,KH,KW], y[N,M,OH,OW], OH=(IH-1)*stride-2*pad+KH+out_pad.          */
int faoctasr_conv_transpose2d_fwd(const float* x, const float* w, const float* bias, float* y,
                                  int N, int C, int IH, int IW, int M, int KH, int KW, int stride, int pad,
                                  int out_pad, int act, float slope, float* wpack, int wpack_state, int precision,
                                  faoctasr_stream_t stream);
int faoctasr_conv_transpose2d_dgrad(const float* dy, const float* w, float* dx,
                                    int N, int C, int IH, int IW, int M, int KH, int KW, int stride, int pad,
                                    int out_pad, float* wpack, int wpack_state, int precision, faoctasr_stream_t stream);
int faoctasr_conv_transpose2d_wgrad(const float* x, const float* dy, float* dw,
                                    int N, int C, int IH, int IW, int M, int KH, int KW, int stride, int pad,
                                    int out_pad, int accumulate, int precision, faoctasr_stream_t stream);
/* gradient of nn.ReflectionPad2d(p): dx[NC,H,W] += fold of dxp[NC,H+2p,W+2p] (dx overwritten) */
int faoctasr_reflect_pad_bwd(const float* dxp, float* dx, int NC, int H, int W, int p, faoctasr_stream_t stream);
/* per-channel sum over (N,HW): conv bias gradient.  db[C] overwritten (or added to).      */
int faoctasr_channel_sum(const float* dy, float* db, int N, int C, int HW, int accumulate, faoctasr_stream_t stream);

/* ---- BatchNorm2d (training mode) + fused activation / residual ----------------------------
 * nn.BatchNorm2d calls: model.py:110,118 (D), 244-245,251 (stems/skip), 412-414,431 (shallowNet),
 * 452,459,470 (ResnetGenerator), 494,499 (ResidualBlock).  Batch statistics over (N,H,W),
 * biased variance for normalisation, unbiased for running_var, momentum/eps as given.
 * y = act(gamma*xhat + beta + residual)   (residual may be NULL).
 * workspace: faoctasr_bn_workspace_floats(C) floats.                                       */
long faoctasr_bn_workspace_floats(int C);
int faoctasr_batchnorm_train_fwd(const float* x, const float* gamma, const float* beta, const float* residual,
                                 float* y, float* save_mean, float* save_invstd,
                                 float* running_mean, float* running_var,
                                 int N, int C, int HW, float eps, float momentum, int act, float slope,
                                 float* workspace, faoctasr_stream_t stream);
/* dx overwritten; dgamma[C], dbeta[C] overwritten or (accumulate_affine != 0) added to; y is
 * the saved forward output (activation mask); the residual gradient dy*act'(y) is written to
 * dres when dres != NULL.  y may be NULL for act NONE / RELU / LRELU when the forward had NO residual: the mask is then taken
 * from the recomputed pre-activation x*gamma*invstd + (beta - mean*gamma*invstd) (the forward's own expression), which saves
 * one tensor read per pass; `beta` is only read in that case.                                */
int faoctasr_batchnorm_train_bwd(const float* x, const float* dy, const float* y, const float* gamma, const float* beta,
                                 const float* save_mean, const float* save_invstd,
                                 float* dx, float* dgamma, float* dbeta, float* dres,
                                 int N, int C, int HW, int act, float slope, int accumulate_affine,
                                 float* workspace, faoctasr_stream_t stream);
/* nn.BatchNorm2d in eval mode (running statistics): the inference path, utils.py:186,221 `model.eval()`.
 * y = act(gamma*(x-running_mean)/sqrt(running_var+eps)+beta); the backward gives dx only (statistics are constants). */
int faoctasr_batchnorm_eval_fwd(const float* x, const float* gamma, const float* beta, const float* running_mean,
                                const float* running_var, float* y, int N, int C, int HW, float eps, int act, float slope,
                                faoctasr_stream_t stream);
int faoctasr_batchnorm_eval_bwd(const float* dy, const float* y, const float* gamma, const float* running_var, float* dx,
                                int N, int C, int HW, float eps, int act, float slope, faoctasr_stream_t stream);
/* InstanceNorm2d (named by north_star; not on the reference's path): per-(n,c) statistics;
 * save_mean/save_invstd have N*C entries, workspace faoctasr_bn_workspace_floats(N*C) floats. */
int faoctasr_instancenorm_fwd(const float* x, const float* gamma, const float* beta, float* y,
                              float* save_mean, float* save_invstd, int N, int C, int HW, float eps,
                              int act, float slope, float* workspace, faoctasr_stream_t stream);
int faoctasr_instancenorm_bwd(const float* x, const float* dy, const float* y, const float* gamma, const float* beta,
                              const float* save_mean, const float* save_invstd, float* dx,
                              float* dgamma, float* dbeta, int N, int C, int HW, int act, float slope,
                              float* workspace, faoctasr_stream_t stream);

/* ---- pointwise / data movement ----------------------------------------------------------- */
/* nn.ReLU / nn.LeakyReLU(0.2) / nn.Tanh (model.py:102,111,119,243,249,254,413,431,438,...) */
int faoctasr_act_fwd(const float* x, float* y, long n, int act, float slope, faoctasr_stream_t stream);
/* dx = dy * act'(y) with y the activation OUTPUT */
int faoctasr_act_bwd(const float* dy, const float* y, float* dx, long n, int act, float slope, faoctasr_stream_t stream);
/* torch.cat([a,b],1) followed by an optional activation (model.py:266,268,298 + 249,431) */
int faoctasr_cat2_act_fwd(const float* a, const float* b, float* y, int N, int Ca, int Cb, int HW,
                          int act, float slope, faoctasr_stream_t stream);
int faoctasr_cat2_act_bwd(const float* dy, const float* y, float* da, float* db, int N, int Ca, int Cb, int HW,
                          int act, float slope, faoctasr_stream_t stream);
/* y = alpha*a + beta*b (residual add x + conv_block(x): model.py:420,505) */
int faoctasr_axpby(const float* a, const float* b, float* y, long n, float alpha, float beta, faoctasr_stream_t stream);

/* ---- Haar DWT / IDWT, mode 'reflect', even H and W ----------------------------------------
 * DWTForward.forward transform2d.py:44-74 -> AFB2D lowlevel.py:312-365; DWTInverse.forward
 * transform2d.py:111-148 -> SFB2D lowlevel.py:647-694.  One level per call.
 * x[NC,H,W] -> ll[NC,H/2,W/2], hi[NC,3,H/2,W/2] (band order LH,HL,HH).                     */
int faoctasr_haar_dwt2d_fwd(const float* x, float* ll, float* hi, long NC, int H, int W, faoctasr_stream_t stream);
/* AFB2D.backward lowlevel.py:349-365 (= synthesis): dx[NC,H,W] from dll, dhi (either may be NULL = zeros) */
int faoctasr_haar_dwt2d_bwd(const float* dll, const float* dhi, float* dx, long NC, int H, int W, faoctasr_stream_t stream);
/* fused discriminator front ends: model.py:166-179 (D_A: LL only) and model.py:222-235
 * (D_B: cat(LH,HL,HH)*0.5+0.5, x[N,1,H,W] -> y[N,3,H/2,W/2]); mode 0 = LL, 1 = cat-normalised */
int faoctasr_haar_dfront_fwd(const float* x, float* y, int N, int H, int W, int mode, faoctasr_stream_t stream);
int faoctasr_haar_dfront_bwd(const float* dy, float* dx, int N, int H, int W, int mode, faoctasr_stream_t stream);

/* ---- FFT Gaussian frequency split as circulant GEMMs ---------------------------------------
 * utils.high_pass / utils.low_pass (utils.py:71-117) as called at train.py:173-175,189-191,
 * 197-199,211-213.  The shifted Gaussian mask is separable, so ifft2(mask*fft2(x)) = Ch x Cw^T
 * with real symmetric circulant matrices built once per (n, radius) (faoctasr_circulant_lowpass).
 * Batched row-major SGEMM on f32 MFMA: for b in [0,batch): C_b = A_b(MxK) * B_b(KxN).
 * batch <= 65535 and M <= 65535 * 64 (the grid's z and y extents); beyond either: FAOCTASR_EUNSUPPORTED, nothing launched. */
int faoctasr_sgemm_batched(const float* A, const float* B, float* C, int M, int N, int K,
                           int lda, int ldb, int ldc, long strideA, long strideB, long strideC, int batch,
                           faoctasr_stream_t stream);
/* The filter cache entry for one (n, radius): out[n*n] = the real symmetric circulant of the centred Gaussian mask of
 * utils.py:71-80 (guais_low_pass; the high-pass mask is 1 - it), built in double precision on the device.  SURVEY 8b asks
 * for an immutable (H,W,r)-keyed cache behind a create/destroy handle; because this ABI never allocates, the entry is a
 * caller-owned buffer instead: build it once per (n, radius, device) with this call and keep it as long as needed.    */
int faoctasr_circulant_lowpass(float* out, int n, float radius, faoctasr_stream_t stream);
/* hf = (|x - low_hp| + x)/2, lf = -|low_lp|  (train.py:173-175) */
int faoctasr_freq_mix_fwd(const float* x, const float* low_hp, const float* low_lp, float* hf, float* lf,
                          long n, faoctasr_stream_t stream);
/* s_hp = 0.5*g_hf*sign(x-low_hp), s_lp = -g_lf*sign(low_lp), dx_direct = 0.5*g_hf + s_hp
 * (the caller then subtracts Ch s_hp Cw and adds Ch s_lp Cw)                                */
int faoctasr_freq_mix_bwd(const float* x, const float* low_hp, const float* low_lp, const float* g_hf, const float* g_lf,
                          float* s_hp, float* s_lp, float* dx_direct, long n, faoctasr_stream_t stream);

/* ---- SSIM (ssim.py:17-37), fused separable 11-tap Gaussian window, zero padding -------------
 * per-image sums of the ssim map are written to sums[N] (mean = sums/(C*H*W)).              */
int faoctasr_ssim_fwd(const float* a, const float* b, float* sums, int N, int C, int H, int W, faoctasr_stream_t stream);
/* da, db (either may be NULL) = g[n or 0] * d(sum of map)/d(a|b); gscale multiplies, g is a device scalar
 * array of length gN (1 = shared) */
int faoctasr_ssim_bwd(const float* a, const float* b, const float* g, int gN, float gscale, float* da, float* db,
                      int N, int C, int H, int W, faoctasr_stream_t stream);

/* ---- spectral phase-consistency loss (model.py:36-58; train.py:28,94) -------------------------
 * loss_b = -cos(a_x, a_y), a = flatten(m * log|fft2(.)|) over (C,H,W) of sample b, m[u,v] = 1 - exp(-0.5 d^2 / radius^2) with d
 * the distance of bin (u,v) from the zero frequency (the reference's fftshift permutes both operands of the dot product alike
 * and is dropped).  The reference reads sample 0 only (its train.py runs batch 1); here the loss is evaluated per sample and
 * loss_mean is the batch mean -- identical at N = 1.  A bin whose amplitude is exactly zero gives log 0 = -inf and a NaN
 * loss, as in the reference: there is no clamp and no epsilon.  The DFT runs as real GEMMs on v_mfma_f32_32x32x2_f32 with
 * cos / sin tables (csrc/spectral.hip); the operands are always exact fp32, whatever the convolutions' precision.
 * DFT tables for one n, built once per (n, device) in double on the device into a caller-owned buffer of 4*n*n floats:
 * [C_n | S_n] (n rows of 2n) followed by [C_n ; S_n] (2n rows of n), C_n[k,l] = cos(2 pi kl/n), S_n[k,l] = sin(2 pi kl/n). */
int faoctasr_dft_tables(float* out, int n, faoctasr_stream_t stream);
/* workspace of one forward / backward pair (model.py:36-58): per-sample sums, per-block partial sums, the spectrum planes the
 * backward reads (Re, -Im: 8 bytes per pixel of x and of y) and the row-pass buffer; -1 on a bad shape */
long faoctasr_phase_loss_workspace_floats(int N, int C, int H, int W);
/* model.py:36-58 forward for x, y[N,C,H,W] (H, W >= 2, even or odd): loss_per_sample[N], loss_mean[1].  Enqueues the row pass
 * (faoctasr_sgemm_batched), the fused column pass + log-amplitude + partial sums, and a fixed-order finishing reduction
 * (no float atomics: bit-reproducible).  tabH, tabW: faoctasr_dft_tables of H and of W.  `workspace` (8-byte aligned) must
 * stay untouched until the matching backward has run. */
int faoctasr_phase_loss_fwd(const float* x, const float* y, const float* tabH, const float* tabW, float radius,
                            float* loss_per_sample, float* loss_mean, float* workspace, int N, int C, int H, int W,
                            faoctasr_stream_t stream);
/* model.py:36-58 backward: dx, dy[N,C,H,W] (either may be NULL) = g[0] * d loss_mean / d(x|y), g a device scalar; reads the
 * workspace the forward of the same arguments filled (and reuses its row-pass buffer). */
int faoctasr_phase_loss_bwd(const float* g, const float* tabH, const float* tabW, float radius, float* dx, float* dy,
                            float* workspace, int N, int C, int H, int W, faoctasr_stream_t stream);

/* ---- focal frequency loss (Jiang, Dai, Wu, Loy, ICCV 2021; not part of the reference) ----------
 * D = fft2(x, ortho) - fft2(y, ortho) per (n, c) plane, q = |D|^2, w = phi(q) / phi(M) with phi(q) = q^(alpha/2) or, with
 * log_matrix, log(q^(alpha/2) + 1), and M the maximum of q over the plane (batch_matrix: over the whole batch); w is a constant
 * for the gradient and a plane (batch) with M = 0 has w = 0.  L = mean over n, c, u, v of w q.  The DFT is linear, so one
 * transform of x - y serves both images, and sum w q = (sum phi(q) q) / phi(M) makes the forward one pass (csrc/spectral.hip).
 * Always exact fp32; no atomics, every sum in a fixed order: bit-reproducible.  tabH, tabW: faoctasr_dft_tables of H and of W.
 * workspace of one forward or one backward (per-plane sums, per-block partials, the row-pass buffer; free again once the call has
 * run on its stream); -1 on a bad shape */
long faoctasr_ffl_workspace_floats(int N, int C, int H, int W);
/* forward for x, y[N,C,H,W] (H, W >= 2, even or odd), alpha finite and >= 0: loss[1].  Enqueues the row pass of x and y
 * (faoctasr_sgemm_batched), the fused column pass of their difference + weight + partial sums, and a single-block finish.
 * planes (may be NULL: no backward will follow and the spectrum is not stored): N*C*(2*H*W + 1) floats that the backward reads --
 * Re and -Im of D per plane, then 1 / phi(M) per plane.  `workspace` must be 8-byte aligned. */
int faoctasr_ffl_fwd(const float* x, const float* y, const float* tabH, const float* tabW, float alpha, int log_matrix,
                     int batch_matrix, float* loss, float* planes, float* workspace, int N, int C, int H, int W,
                     faoctasr_stream_t stream);
/* backward: dx, dy[N,C,H,W] (either may be NULL) = g[0] * dL/d(x|y), g a device scalar, from the `planes` a forward with the same
 * alpha and log_matrix filled.  One column pass and one row pass whichever sides are wanted; dy is the exact negation of dx. */
int faoctasr_ffl_bwd(const float* g, const float* planes, const float* tabH, const float* tabW, float alpha, int log_matrix,
                     float* dx, float* dy, float* workspace, int N, int C, int H, int W, faoctasr_stream_t stream);

/* ---- spectral-profile loss (after Durall, Keuper, Keuper, CVPR 2020; not part of the reference) ----------
 * q = |fft2(x)|^2 / (HW) per plane; A[k] = the mean of q over the ring bin(u,v) = floor(M sqrt(u_c^2/H^2 + v_c^2/W^2)) = k of centred
 * frequencies, M = min(H, W), K = 1 + floor(M sqrt((H/2)^2/H^2 + (W/2)^2/W^2)) bins; a = log(A + eps).  The loss is the mean over
 * n, c and k >= k_min of (a_x - a_y)^2 or, with batch_profile, the mean over k >= k_min of the squared difference of the batch means
 * of a (phase-blind and translation-invariant, so meaningful between unpaired images).  2 <= H, W <= 1024.
 * Only the half spectrum (columns v < Wh = W/2 + 1) is transformed.  The caller owns every table (nothing is allocated here):
 *   tabH     faoctasr_dft_tables of H
 *   halfW    [C_W[:, :Wh] | S_W[:, :Wh]] (W rows of 2 Wh) followed by [C_W[:, :Wh]^T ; S_W[:, :Wh]^T] (2 Wh rows of W)
 *   csr_off  K + 1 offsets into csr_idx;  csr_idx  the H*Wh flat half-plane positions sorted by (bin, position)
 *   cnt      K counts of FULL-plane positions per bin;  binmap  int16 H x Wh, the bin of every half-plane position
 * Wh == W with tables of the full plane is accepted too (every column then counts once): a measuring switch.
 * Always exact fp32; no atomics, every sum in a fixed order: bit-reproducible, and L(x, y) == L(y, x) bit for bit.
 * workspace of one forward or one backward for `sides` (1: the profile, 2: the loss) images; -1 on a bad shape */
long faoctasr_sprof_workspace_floats(int sides, int N, int C, int H, int W, int Wh, int K);
/* the profile A[N*C][K] of x[N,C,H,W].  save (may be NULL: no backward will follow): N*C*2*H*Wh floats, Re and -Im per plane. */
int faoctasr_sprof_profile_fwd(const float* x, const float* tabH, const float* halfW, const int* csr_off, const int* csr_idx,
                               const int* cnt, float* A, float* save, float* workspace, int N, int C, int H, int W, int Wh, int K,
                               faoctasr_stream_t stream);
/* the loss of x, y[N,C,H,W]: loss[1], loss_per_image[N] (per_image, which excludes batch_profile; else may be NULL), and both
 * profiles A[2][N*C][K].  eps finite and > 0, 0 <= k_min < K.  save_x, save_y (each may be NULL: that side gets no gradient):
 * N*C*(2*H*Wh + K) floats, the planes and then dL/dA / cnt_k, which a single-block finish writes with the loss. */
int faoctasr_sprof_loss_fwd(const float* x, const float* y, const float* tabH, const float* halfW, const int* csr_off,
                            const int* csr_idx, const int* cnt, double eps, int k_min, int batch_profile, int per_image, float* loss,
                            float* loss_per_image, float* A, float* save_x, float* save_y, float* workspace, int N, int C, int H, int W,
                            int Wh, int K, faoctasr_stream_t stream);
/* backward of either: dx, dy[N,C,H,W] (either may be NULL; a side needs its save buffer).  The loss: g a device scalar, or with
 * g_per_image N of them, and gA NULL.  The profile: gA[N*C][K] the cotangent of A, g, save_y and dy NULL. */
int faoctasr_sprof_bwd(const float* g, int g_per_image, const float* gA, const float* save_x, const float* save_y, const float* tabH,
                       const float* halfW, const short* binmap, const int* cnt, float* dx, float* dy, float* workspace, int N, int C,
                       int H, int W, int Wh, int K, faoctasr_stream_t stream);

/* ---- Fourier ring correlation (Saxton & Baumeister 1982, van Heel & Schatz 2005; not part of the reference) ----
 * With F = fft2(x), G = fft2(y) per plane and the rings, tables and limits of the spectral profile above, the ring MEANS
 *   Nk = mean Re(F conj G) / (HW),  Xk = mean |F|^2 / (HW),  Yk = mean |G|^2 / (HW),   r_k = Nk / sqrt(Xk Yk + eps) in double.
 * The index of an image is the mean of r_k over c and k_min <= k <= k_max; the curve is r_k at every ring.  Xk and Yk are the
 * spectral profiles of x and y bit for bit.  A ring with Xk Yk = 0 has r_k = 0 and finite gradients.  Always exact fp32; no
 * atomics, every sum in a fixed order: bit-reproducible, and frc(x, y) == frc(y, x) bit for bit with swapped gradients.
 * workspace of one forward or one backward; -1 on a bad shape */
long faoctasr_frc_workspace_floats(int N, int C, int H, int W, int Wh, int K);
/* index[1] (the batch mean), index_per_image[N] (needed with per_image, else may be NULL; always each sample's own mean),
 * curve[N*C][K], rings[3][N*C][K] (Nk, Xk, Yk).  eps finite and > 0, 0 <= k_min <= k_max <= K - 1.  save (may be NULL: no backward
 * will follow): N*C*(4*H*Wh + 3*K) floats, Re and -Im of x and of y and then the coefficient tables d index / d (Nk, Xk, Yk) / cnt_k
 * (per_image: of each sample's own mean), which the single-block finish writes with the index. */
int faoctasr_frc_fwd(const float* x, const float* y, const float* tabH, const float* halfW, const int* csr_off, const int* csr_idx,
                     const int* cnt, double eps, int k_min, int k_max, int per_image, float* index, float* index_per_image, float* curve,
                     float* rings, float* save, float* workspace, int N, int C, int H, int W, int Wh, int K, faoctasr_stream_t stream);
/* dx, dy[N,C,H,W] (either may be NULL; one side still reads both saved spectra).  g a device scalar, or with g_per_image N of them. */
int faoctasr_frc_bwd(const float* g, int g_per_image, const float* save, const float* tabH, const float* halfW, const short* binmap,
                     float* dx, float* dy, float* workspace, int N, int C, int H, int W, int Wh, int K, faoctasr_stream_t stream);

/* ---- phase-correlation registration and the Fourier shift (Kuglin & Hines 1975; Guizar-Sicairos et al. 2008; not in the reference) ----
 * a, b[N,C,H,W] fp32, the tables and limits of the spectral-profile loss (Wh = W/2 + 1; binmap: the int16 ring of every half-plane
 * position).  F = fft2(a), G = fft2(b), R = G conj(F) / (HW), Rn = R / sqrt(|R|^2 + eps) (normalize) or R, zero in every ring above
 * k_max; surface[N,H,W] = sum_c Re ifft2(Rn), whose peak lies at d when b(p) = a(p - d).  The coarse peak is the first maximum in
 * row-major order among |d_y| <= max_shift_y, |d_x| <= max_shift_x (positions > H/2, > W/2 wrap negative); with upsample U > 1 the
 * inverse transform is evaluated on T x T points, T = ceil(1.5 U), at the offsets (j - T/2) / U around it, and the first maximum
 * there wins.  shift[N][2] = (d_y, d_x), peak[N] = the winning value over C.  Nothing waits for the host, nothing is allocated, every sum
 * has a fixed order: capturable and bit-reproducible.
 * workspace of one call; -1 on a bad shape or upsample outside 1..100 */
long faoctasr_pcorr_workspace_floats(int N, int C, int H, int W, int Wh, int K, int upsample);
/* shift and peak NULL: only the surface is computed (surface must be given); surface NULL: it stays in the workspace.
 * eps finite and >= 0, 0 <= k_max <= K - 1, upsample 1..100, 0 <= max_shift_y <= H/2, 0 <= max_shift_x <= W/2. */
int faoctasr_pcorr_fwd(const float* a, const float* b, const float* tabH, const float* halfW, const short* binmap, double eps, int k_max,
                       int normalize, int upsample, int max_shift_y, int max_shift_x, float* shift, float* peak, float* surface,
                       float* workspace, int N, int C, int H, int W, int Wh, int K, faoctasr_stream_t stream);
/* out[N,C,H,W] = Re ifft2(fft2(x) exp(-2 pi i (f_u d_y + f_v d_x))), (d_y, d_x) = sign * shift[n], shift[N][2] on the device, f of
 * numpy.fft.fftfreq: the content moves by +d.  sign is 1 or -1; the transpose of the operator is the call with the other sign. */
long faoctasr_fourier_shift_workspace_floats(int N, int C, int H, int W);
int faoctasr_fourier_shift(const float* x, const float* shift, float sign, const float* tabH, const float* halfW, float* out,
                           float* workspace, int N, int C, int H, int W, faoctasr_stream_t stream);

/* ---- differentiable mutual information (Gaussian Parzen windows; not part of the reference) ----
 * Per (n, c) plane of n_pix = H*W pixels, with K = bins, d = (hi - lo) / K, centres c_k = lo + (k + 1/2) d, sigma = sigma_ratio d:
 * Wa[p,k] = softmax_k(-(x_p - c_k)^2 / (2 sigma^2)) (evaluated stably: any finite x, in the range or not), Wb likewise from y,
 * P = Wa^T Wb / n_pix, pa / pb its row / column sums, H(q) = -sum q log(q + eps); the plane's score is MI = Ha + Hb - Hab or,
 * with `normalized`, NMI = (Ha + Hb) / Hab.  out[0] = the mean over all planes, or with `per_image` out[n] = the mean over c.
 * Nothing of size pixels x bins is stored: the weights are formed in registers / LDS, contracted on the exact-f32 MFMA and
 * recomputed in the backward (csrc/mi.hip).  No atomics, every sum in a fixed order: bit-reproducible, and swapping x and y gives
 * the same score and the swapped gradients bit for bit.  2 <= bins <= 64, N*C <= 65535, hi > lo, sigma_ratio > 0, eps > 0.
 * workspace of one forward (per-plane scores in double, one K x K partial per 2048 pixels; free again once the call has run on
 * its stream; 8-byte aligned); -1 on a bad shape */
long faoctasr_mi_workspace_floats(int N, int C, int H, int W, int bins);
/* forward for x, y[N,C,H,W]: out[1] or, with per_image, out[N].  table (may be NULL: no backward will follow and nothing is
 * saved): N*C*bins*bins floats, dS/dP per plane with the 1 / (planes * n_pix * sigma^2) factor of the mean folded in (per_image:
 * 1 / (C * n_pix * sigma^2)).  Three launches: histogram partials, per-plane entropies, means. */
int faoctasr_mi_fwd(const float* x, const float* y, float* out, float* table, float* workspace, int N, int C, int H, int W,
                    int bins, float lo, float hi, float sigma_ratio, float eps, int normalized, int per_image,
                    faoctasr_stream_t stream);
/* backward: dx, dy[N,C,H,W] (either may be NULL) = g * dS/d(x|y) from x, y and the `table` a forward with the same parameters
 * filled; g a device scalar, or with per_image N device floats, multiplied in last.  One pass over the pixels. */
int faoctasr_mi_bwd(const float* g, const float* x, const float* y, const float* table, float* dx, float* dy, int N, int C,
                    int H, int W, int bins, float lo, float hi, float sigma_ratio, int per_image, faoctasr_stream_t stream);

/* ---- total-variation loss (model.py:17-33; train.py:98,178) ------------------------------------
 * L = weight * 2 * (S_h / count_h + S_w / count_w) / B for x[B,C,H,W] (H, W >= 2), S_h = sum (x[.,.,i+1,j] - x[.,.,i,j])^2,
 * S_w = sum (x[.,.,i,j+1] - x[.,.,i,j])^2, count_h = C (H-1) W, count_w = C H (W-1)  (csrc/tv.hip).  float4 loads when W % 4 == 0
 * and the pointers are 16-byte aligned, a scalar path otherwise.  Always exact fp32, whatever the convolutions' precision.
 * workspace of one forward (two partial sums per block; free again once the forward has run on its stream); -1 on a bad shape */
long faoctasr_tv_loss_workspace_floats(int B, int C, int H, int W);
/* out[0] = L (overwritten).  One pass over x with S_h and S_w kept apart, per-block partials in `workspace`, then a single-block
 * kernel that adds them in a fixed order in double and applies the divisors (no atomics: bit-reproducible). */
int faoctasr_tv_loss_fwd(const float* x, float* out, float* workspace, int B, int C, int H, int W, float weight,
                         faoctasr_stream_t stream);
/* dx[B,C,H,W] (overwritten) = g[0] * dL/dx, g a device scalar: one stencil kernel, reads x only. */
int faoctasr_tv_loss_bwd(const float* x, const float* g, float* dx, int B, int C, int H, int W, float weight,
                         faoctasr_stream_t stream);

/* ---- general filter-bank 2-D DWT / IDWT, one level per call (csrc/dwt.hip) ----------------------
 * pytorch_wavelets dwt/lowlevel.py:91-172 (afb1d), 226-271 (sfb1d), 312-365 (AFB2D), 647-694 (SFB2D).  The taps are HOST
 * pointers, read during the call and passed to the kernel by value (nothing is allocated or copied: the launch is capturable):
 * a lowpass / highpass pair of L_h taps filtering along H and one of L_w taps along W, each L even and 2 <= L <= 16.  Analysis
 * taps are given as the correlation kernels the reference registers (the decomposition taps reversed), synthesis taps as
 * given.  mode: 0 zero, 1 symmetric, 2 periodization, 4 reflect, 6 periodic (lowlevel.py:274-290).  FAOCTASR_EINVAL for an odd
 * or out-of-range L, an unknown mode, a side below the minimum, or a crop outside the result.
 * Analysis: x[NC,H,W] -> ll[NC,OH,OW], hi[NC,3,OH,OW] (band order LH, HL, HH), O = (N + 1) / 2 for periodization and
 * (N + L - 1) / 2 otherwise; H >= L_h / 2 + 1 and W >= L_w / 2 + 1.  Also SFB2D.backward (with the synthesis taps). */
int faoctasr_dwt2d_analysis(const float* x, float* ll, float* hi, long NC, int H, int W, const float* lo_h, const float* hi_h,
                            int L_h, const float* lo_w, const float* hi_w, int L_w, int mode, faoctasr_stream_t stream);
/* Synthesis: ll[NC,nh,nw], hi[NC,3,nh,nw] (either may be NULL = zeros) -> y[NC,out_h,out_w], the top-left crop of the
 * (2 n - L + 2)-sided (periodization: 2 n) result; n >= L / 2 (periodization: 2 n >= L / 2).  Also AFB2D.backward (with the
 * analysis taps and the crop to the input's size). */
int faoctasr_dwt2d_synthesis(const float* ll, const float* hi, float* y, long NC, int nh, int nw, int out_h, int out_w,
                             const float* lo_h, const float* hi_h, int L_h, const float* lo_w, const float* hi_w, int L_w,
                             int mode, faoctasr_stream_t stream);

/* ---- 1-D filter-bank DWT / IDWT over rows, all levels of a row in one launch (csrc/dwt1d.hip) ----
 * pytorch_wavelets dwt/transform1d.py:7-115 (DWT1DForward / DWT1DInverse), dwt/lowlevel.py:368-424 (AFB1D), 697-743 (SFB1D).  One
 * lowpass / highpass pair of L taps, L even and 2 <= L <= 16, as HOST pointers read during the call and passed to the kernel by
 * value, like the host arrays of per-level pointers and lengths (nothing is allocated or copied: the launch is capturable);
 * analysis taps as the correlation kernels the reference registers (the decomposition taps reversed), synthesis taps as given;
 * modes as for the 2-D bank; 1 <= J <= 8 levels.  The rows of the strided operand: row r starts (r / inner) * outer_stride +
 * (r % inner) * row_stride elements in, samples contiguous (an (N, C, n) tensor: inner = C).  fused = 1: one launch runs all J
 * levels of a row in LDS, rows of at most faoctasr_dwt1d_fused_max() samples; fused = 0: the tiled launch, any length, J = 1
 * only (one call per level).  Both give the same bits.  FAOCTASR_EINVAL for anything outside these. */
long faoctasr_dwt1d_fused_max(void);
/* Analysis: NC rows of n samples -> lo[NC, n_J], hi[j][NC, n_(j+1)] for j = 0 .. J-1 (hi: a host array of J device pointers),
 * per level out[i] = sum_k h[k] xe[2 i + k - base], n_(j+1) = (m + 1) / 2 for periodization and (m + L - 1) / 2 otherwise, m the
 * level's input length.  in_lens (NULL: every level reads what the one before produced; level 0 reads n): J host ints, the
 * length level j is to read -- what its source holds, or ONE more: the extra sample is a zero appended before the extension.
 * Every level's input has at least 2 samples.  Also SFB1D.backward (with the synthesis taps). */
int faoctasr_dwt1d_analysis(const float* x, long x_inner, long x_outer_stride, long x_row_stride, float* lo, float* const* hi,
                            long NC, int n, const int* in_lens, int J, const float* h0, const float* h1, int L, int mode,
                            int fused, faoctasr_stream_t stream);
/* Synthesis: lo (NC strided rows, the first counts[J-1] samples of each are read), hi[j][NC, counts[j]] (a host array of J
 * device pointers, a NULL entry = zeros), counts: J host ints, the coefficient count of level j (0 = finest) -> y[NC, out_len].
 * From the coarsest level to the finest; level j's result (2 c - L + 2 samples, periodization 2 c) is cropped to counts[j-1],
 * the finest level's to out_len; a crop longer than the result is an error, as is a count below L / 2 (periodization: below
 * (L + 3) / 4).  Also AFB1D.backward (with the analysis taps, the crops being the levels' input lengths). */
int faoctasr_dwt1d_synthesis(const float* lo, long lo_inner, long lo_outer_stride, long lo_row_stride, const float* const* hi,
                             float* y, long NC, const int* counts, int J, int out_len, const float* g0, const float* g1, int L,
                             int mode, int fused, faoctasr_stream_t stream);

/* ---- stationary (undecimated, a-trous) 2-D wavelet transform, one level per call (csrc/swt.hip) --
 * pytorch_wavelets dwt/lowlevel.py:175-223 (afb1d_atrous), 475-521 (afb2d_atrous); transform2d.py:151-212 (SWTForward).  The taps
 * are HOST pointers, read during the call and passed to the kernel by value (the launch is capturable), in WAVELET order
 * (dec_lo / dec_hi, not the reversed buffers the modules register): a pair of L_h taps filtering along H and one of L_w taps
 * along W, each L even and 2 <= L <= 16.  dilation = 2^level: 1, 2, 4 or 8.  mode: 0 zero, 1 symmetric, 4 reflect, 6 periodic.
 * H >= L_h dilation / 2 + 1 and W >= L_w dilation / 2 + 1 (the extension then folds at most once a side).  FAOCTASR_EINVAL for a
 * tap count, mode, dilation, plane stride or side outside these.
 * Analysis: NC planes of x (H x W, x_plane_stride elements apart: level j + 1 reads band 0 of level j's output in place) ->
 * y[NC,4,H,W], per axis out[i] = sum_k h[k] xe[i - k dilation + L dilation / 2], W first, then H, the result times `scale`;
 * bands (W lo, H lo), (W lo, H hi), (W hi, H lo), (W hi, H hi).  Also the periodic inverse's backward (reversed rec taps, 1/4). */
int faoctasr_swt2d_analysis(const float* x, long x_plane_stride, float* y, long NC, int H, int W, const float* lo_h,
                            const float* hi_h, int L_h, const float* lo_w, const float* hi_w, int L_w, int dilation, int mode,
                            float scale, faoctasr_stream_t stream);
/* Adjoint: c[NC,4,H,W] -> NC planes of dx (dx_plane_stride elements apart), `scale` times the exact transpose of the analysis
 * in every mode, as a fixed-order gather (no atomics).  With the reversed rec taps, mode 6 and scale 1/4 it is one level of the
 * periodic inverse: y[m] = 1/2 sum_k g0[k] lo[(m - k d + (L/2 - 1) d) mod N] + g1[k] hi[same] per axis, H first.
 * band0 (NULL: none): NC planes, band0_plane_stride elements apart, that are added to band 0 of c as it is read
 * (band0_replaces = 0: the backward chains the coarser level's gradient into a level's cotangent) or read instead of it
 * (band0_replaces = 1: the inverse chains the coarser level's result into a level's coefficients) -- neither copies c. */
int faoctasr_swt2d_adjoint(const float* c, float* dx, long dx_plane_stride, const float* band0, long band0_plane_stride,
                           int band0_replaces, long NC, int H, int W, const float* lo_h,
                           const float* hi_h, int L_h, const float* lo_w, const float* hi_w, int L_w, int dilation, int mode,
                           float scale, faoctasr_stream_t stream);

/* ---- dual-tree complex wavelet transform, one level per call (csrc/dtcwt.hip) --------------------
 * pytorch_wavelets dtcwt/transform_funcs.py (fwd_j1, fwd_j2plus, inv_j1, inv_j2plus), dtcwt/lowlevel.py.  The taps are HOST
 * pointers, read during the call and passed to the kernel by value (the launch is capturable), in the order the modules register
 * them (prep_filt: the taps reversed).  Level 1: a lowpass of L0 and a highpass of L1 taps, each odd and 3..19; mode 1 is the
 * symmetric extension, every other mode pads with zeros.  Levels >= 2: the four q-shift filters of one even length m, 4..20,
 * always symmetric.  Operands of N x C planes.  The lowpass INPUT of a call is strided: plane (n, c) starts n * sn + c * sc
 * elements in, rows are sr elements apart, columns contiguous.  The bandpass tensor -- six complex orientations (15, 45, 75,
 * 105, 135, 165 degrees) of half the lowpass resolution -- is addressed through the element strides of its n, c, orientation,
 * row, column and re/im axes, so any layout or view is read and written in place; hi_vec2 = 1 (only where hi_si == 1, every
 * other stride is even and the base is 8-byte aligned) stores each (re, im) pair as one 8-byte word.  Outputs ll and y are
 * contiguous.  FAOCTASR_EINVAL for a tap count, size or null pointer outside these.
 * fwd_j1: x [H, W], H and W even -> ll [H, W] and hi [H/2, W/2]; either output may be NULL (not computed / not stored).  Also the
 *   backward of inv_j1 (on the synthesis taps).
 * fwd_j2: x [H, W], multiples of 4 -> ll [H/2, W/2], hi [H/4, W/4]; either may be NULL.  Also the backward of inv_j2 (on the
 *   synthesis taps with a and b swapped).
 * inv_j1: ll [H, W], hi [H/2, W/2] -> y [H, W]; ll or hi may be NULL (zeros; its path is not computed).  Also the backward of
 *   fwd_j1 (on the analysis taps).
 * inv_j2: ll [H/2, W/2], hi [H/4, W/4] -> y [H, W], multiples of 4; ll or hi may be NULL.  Also the backward of fwd_j2 (on the
 *   analysis taps with a and b swapped).
 * The optional third filter: the rotationally symmetric three-filter banks (near_sym_b_bp / qshift_b_bp; fwd_j1_rot, fwd_j2plus_rot,
 * inv_j1_rot, inv_j2plus_rot) filter the diagonal band hh by a bandpass filter of its own on both axes -- forward
 * hh = col(row(x, h2), h2); inverse y = row(col(hl, g0), g1) + row(col(lh, g1) + col(ll, g0), g0) + row(col(hh, g2), g2).  Level 1:
 * h2 / g2 of L2 taps, odd and 3..19 like the other two and of its own length; NULL with L2 = 0 is the two-filter bank.  Levels >= 2: a
 * third pair (h2a, h2b) of the same even length m, used as the highpass pair is (and swapped with the other two in a backward); both
 * NULL is the two-filter bank, one NULL is FAOCTASR_EINVAL.  Every other argument, rule and error code is the same in both forms; a
 * forward call with a third filter needs hi (the lowpass alone has none: pass a NULL third filter, else FAOCTASR_EINVAL). */
int faoctasr_dtcwt_fwd_j1(const float* x, long x_sn, long x_sc, long x_sr, float* ll, float* hi, long hi_sn, long hi_sc,
                          long hi_so, long hi_sr, long hi_sw, long hi_si, int hi_vec2, long N, int C, int H, int W,
                          const float* h0, int L0, const float* h1, int L1, const float* h2, int L2, int mode,
                          faoctasr_stream_t stream);
int faoctasr_dtcwt_fwd_j2(const float* x, long x_sn, long x_sc, long x_sr, float* ll, float* hi, long hi_sn, long hi_sc,
                          long hi_so, long hi_sr, long hi_sw, long hi_si, int hi_vec2, long N, int C, int H, int W,
                          const float* h0a, const float* h0b, const float* h1a, const float* h1b, const float* h2a,
                          const float* h2b, int m, faoctasr_stream_t stream);
int faoctasr_dtcwt_inv_j1(const float* ll, long ll_sn, long ll_sc, long ll_sr, const float* hi, long hi_sn, long hi_sc,
                          long hi_so, long hi_sr, long hi_sw, long hi_si, float* y, long N, int C, int H, int W,
                          const float* g0, int L0, const float* g1, int L1, const float* g2, int L2, int mode,
                          faoctasr_stream_t stream);
int faoctasr_dtcwt_inv_j2(const float* ll, long ll_sn, long ll_sc, long ll_sr, const float* hi, long hi_sn, long hi_sc,
                          long hi_so, long hi_sr, long hi_sw, long hi_si, float* y, long N, int C, int H, int W,
                          const float* g0a, const float* g0b, const float* g1a, const float* g1b, const float* g2a,
                          const float* g2b, int m, faoctasr_stream_t stream);

/* ---- DTCWT scattering layers (csrc/scat.hip) ------------------------------------------------------
 * pytorch_wavelets scatternet/lowlevel.py (ScatLayerj1_f, ScatLayerj2_f): one dual-tree level, the smoothed magnitude
 * sqrt(re^2 + im^2 + bias^2) - bias of its six orientations and the 2x2 mean of its lowpass, in one launch each way.  Taps, modes
 * and size rules are those of the dtcwt calls above; bias2 is bias * bias, computed by the caller in double and rounded.
 * Addresses are in elements and rows are contiguous: x takes (n, c, row) strides; low / dlow (n, c) strides; mag / dmag
 * (n, orientation, c) strides, so a call writes into (reads from) slices of a layer's output (cotangent); phase is a contiguous
 * (N, 6, C, H', W', 2) tensor of unit phasors (re / r, im / r); dx is contiguous (N, C, H, W).
 * fwd_j1: x [H, W] -> low [H/2, W/2] (pool = 1: the mean) or [H, W] (pool = 0: the lowpass itself), mag and phase [H/2, W/2].
 * fwd_j2: x [H, W], multiples of 4 -> low, mag, phase [H/4, W/4].
 * phase == NULL: no phasors are stored (a forward without a backward).  colour = 1 (C must be 3): one magnitude per orientation
 *   over the three channels, sqrt(sum_c (re_c^2 + im_c^2) + bias^2) - bias (mag_sc is not used), phasors per channel.
 * bwd_j1, bwd_j2: the adjoints, on the SAME analysis taps as the forward call (bwd_j2 swaps trees a and b itself): dlow of the
 *   forward's low shape, dmag and phase of its mag and phase shapes -> dx [H, W].  The colour form is dmag_sc = 0.
 * The optional third filter (ScatLayerj1_rot_f, ScatLayerj2_rot_f) is that of the dtcwt calls above, NULL for a two-filter bank;
 * bwd_* takes the forward's analysis taps, the third included. */
int faoctasr_scat_fwd_j1(const float* x, long x_sn, long x_sc, long x_sr, float* low, long low_sn, long low_sc, int pool,
                         float* mag, long mag_sn, long mag_so, long mag_sc, float* phase, int colour, float bias, float bias2,
                         long N, int C, int H, int W, const float* h0, int L0, const float* h1, int L1, const float* h2, int L2,
                         int mode, faoctasr_stream_t stream);
int faoctasr_scat_fwd_j2(const float* x, long x_sn, long x_sc, long x_sr, float* low, long low_sn, long low_sc, float* mag,
                         long mag_sn, long mag_so, long mag_sc, float* phase, int colour, float bias, float bias2, long N, int C,
                         int H, int W, const float* h0a, const float* h0b, const float* h1a, const float* h1b, const float* h2a,
                         const float* h2b, int m, faoctasr_stream_t stream);
int faoctasr_scat_bwd_j1(const float* dlow, long dlow_sn, long dlow_sc, int pool, const float* dmag, long dmag_sn, long dmag_so,
                         long dmag_sc, const float* phase, float* dx, long N, int C, int H, int W, const float* h0, int L0,
                         const float* h1, int L1, const float* h2, int L2, int mode, faoctasr_stream_t stream);
int faoctasr_scat_bwd_j2(const float* dlow, long dlow_sn, long dlow_sc, const float* dmag, long dmag_sn, long dmag_so, long dmag_sc,
                         const float* phase, float* dx, long N, int C, int H, int W, const float* h0a, const float* h0b,
                         const float* h1a, const float* h1b, const float* h2a, const float* h2b, int m, faoctasr_stream_t stream);

/* ---- DTCWT magnitude loss (csrc/dtcwt_loss.hip) -----------------------------------------------------
 * L(x, y) = sum_j w_j * mean over (n, c, orientation, row, column) of | r_j(x) - r_j(y) |,  r = sqrt(re^2 + im^2 + bias^2), over the
 * bandpass coefficients of the dtcwt calls above; no lowpass term.  Taps, modes, size rules, strides of x and y ((n, c, row), unit
 * columns) and error codes are theirs; bias2 = bias * bias > 0.
 * fwd_j1 / fwd_j2: one level of BOTH images in one launch (a block runs its tile of x, then of y, through the same LDS).  Writes
 *   part[0, blocks): one partial sum of |r_x - r_y| per block, blocks = faoctasr_dtcwt_loss_workspace_floats(N, C, H, W, level1)
 *     with the H, W of that launch (level1 = 1 for fwd_j1, 0 for fwd_j2; -1 on a bad shape);
 *   llx, lly: each image's lowpass for the next level, contiguous [H, W] (fwd_j1) or [H/2, W/2] (fwd_j2); NULL: not stored;
 *   gx, gy: the cotangent bands sign(r_x - r_y) * z_x / r_x * scale and -sign(r_x - r_y) * z_y / r_y * scale, sign(0) = 0, as
 *     contiguous (N, C, 6, h, w, 2) tensors; NULL: not computed.  scale = w_j / count_j.  dtcwt_inv_j2 / dtcwt_inv_j1 on the
 *     analysis taps (a and b swapped at levels >= 2) carry them to dL/dx and dL/dy.
 * final: out[0] = sum_j level_scale[j] * (sum of the level_floats[j] partials of level j), the levels' partials one after the
 *   other in `workspace`; level_floats and level_scale are HOST arrays of `levels` (<= 16) entries, read during the call.  Fixed
 *   order, in double: bit-reproducible. */
long faoctasr_dtcwt_loss_workspace_floats(long N, int C, int H, int W, int level1);
int faoctasr_dtcwt_loss_fwd_j1(const float* x, long x_sn, long x_sc, long x_sr, const float* y, long y_sn, long y_sc, long y_sr,
                               float* llx, float* lly, float* gx, float* gy, float* part, float scale, float bias2, long N, int C,
                               int H, int W, const float* h0, int L0, const float* h1, int L1, int mode, faoctasr_stream_t stream);
int faoctasr_dtcwt_loss_fwd_j2(const float* x, long x_sn, long x_sc, long x_sr, const float* y, long y_sn, long y_sc, long y_sr,
                               float* llx, float* lly, float* gx, float* gy, float* part, float scale, float bias2, long N, int C,
                               int H, int W, const float* h0a, const float* h0b, const float* h1a, const float* h1b, int m,
                               faoctasr_stream_t stream);
int faoctasr_dtcwt_loss_final(const float* workspace, const long* level_floats, const double* level_scale, int levels, float* out,
                              faoctasr_stream_t stream);

/* ---- complex-wavelet structural similarity (csrc/cwssim.hip) ------------------------------------------
 * cx, cy: two complex bands of one level, contiguous (planes, h, w, 2), planes = N * C * 6; a win x win box window (1 <= win <= 11,
 * h, w >= win) at each of the (h - win + 1) x (w - win + 1) valid positions p:
 *   z_p = sum_W cx conj(cy),  E_p = sum_W |cx|^2 + sum_W |cy|^2,  S_p = (2 |z_p| + K) / (E_p + K),  K > 0.
 * index: part[0, blocks) gets one partial sum of S_p per block, blocks = faoctasr_cwssim_workspace_floats(planes, h, w, win) (-1 on
 *   a bad shape), plane-major.  map_a (planes, h - win + 1, w - win + 1, 2) and map_b (planes, h - win + 1, w - win + 1), both or
 *   neither NULL: a_p z_p / |z_p| (0 where z_p = 0) and b_p, a_p = 2 / (E_p + K), b_p = 2 S_p / (E_p + K).
 * final: out_image[n] = the mean of S_p over image n (planes / N planes each), out_mean[0] = the mean of those; added in double in
 *   a fixed order.  planes, h, w, win as given to index.
 * grad: with A_q, B_q the sums of map_a, map_b over the windows that contain q,
 *   gx_q = (cy_q A_q - cx_q B_q) gscale[n] / count,  gy_q = (cx_q conj(A_q) - cy_q B_q) gscale[n] / count,
 *   count = (planes / N) (h - win + 1) (w - win + 1), gscale a DEVICE array of N floats (the upstream gradient per image); gx or gy
 *   may be NULL (not computed), not both.
 * For cx == cy S_p is exactly 1 and both gradients exactly 0; swapping cx and cy leaves every S_p bit for bit and swaps gx, gy. */
long faoctasr_cwssim_workspace_floats(long planes, int h, int w, int win);
int faoctasr_cwssim_index(const float* cx, const float* cy, float* map_a, float* map_b, float* part, long planes, int h, int w, int win,
                          float K, faoctasr_stream_t stream);
int faoctasr_cwssim_grad(const float* cx, const float* cy, const float* map_a, const float* map_b, float* gx, float* gy,
                         const float* gscale, long N, long planes, int h, int w, int win, faoctasr_stream_t stream);
int faoctasr_cwssim_final(const float* part, long N, long planes, int h, int w, int win, float* out_image, float* out_mean,
                          faoctasr_stream_t stream);

/* ---- multi-scale SSIM (csrc/msssim.hip) -----------------------------------------------------------------
 * a, b: scale `scale` (0-based) of a pair whose scale 0 is (planes, H, W), planes = N * C: contiguous (planes, H >> scale, W >> scale);
 * scale j + 1 is the 2 x 2 mean of scale j (floor).  1 <= levels <= 5 scales, none empty.  Moments as faoctasr_ssim_fwd (11-tap
 * sigma-1.5 Gaussian, zero padding 5):  cs_p = (2 s12 + C2) / (s11 + s22 + C2),  l_p = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1).
 * scale_fwd: one partial sum per block of cs_p (of l_p cs_p at scale levels - 1) into this scale's part of the workspace of
 *   faoctasr_msssim_workspace_floats(planes, H, W, levels) floats (-1 on a bad shape); no atomics.  pa, pb (planes, H >> (scale + 1),
 *   W >> (scale + 1)) get the next scale of both images; both NULL at the last scale and only there.
 * final: F_j[n] = the mean of scale j's map over image n, MS[n] = prod_j max(F_j[n], 0)^weights[j] (weights: HOST array of `levels`
 *   positive doubles), out_image[n] = MS[n], out_mean[0] = their mean; added in double in a fixed order.  coef (levels, N), may be
 *   NULL: w_j MS[n] / F_j[n] / (C h_j w_j), 0 for an image with a factor <= 0, times 1 / N when average != 0.
 * scale_bwd: da, db (either may be NULL, not both) = coef[scale][n] g[n or 0] d(sum of scale's map)/d(a|b) + the adjoint of the
 *   pooling applied to dca, dcb, the gradients of scale + 1 (NULL at the last scale; required for a side that is written elsewhere).
 *   g is a DEVICE array of gN floats (1 = shared, or N).  Run from scale levels - 1 down to 0; scale 0 writes the input gradients.
 * For a == b MS is exactly 1 and both gradients exactly 0; swapping a and b leaves MS bit for bit and swaps the gradients. */
long faoctasr_msssim_workspace_floats(long planes, int H, int W, int levels);
int faoctasr_msssim_scale_fwd(const float* a, const float* b, float* pa, float* pb, float* workspace, long planes, int H, int W, int levels,
                              int scale, float C1, float C2, faoctasr_stream_t stream);
int faoctasr_msssim_final(const float* workspace, long N, long C, int H, int W, int levels, const double* weights, int average,
                          float* out_image, float* out_mean, float* coef, faoctasr_stream_t stream);
int faoctasr_msssim_scale_bwd(const float* a, const float* b, const float* coef, const float* g, int gN, const float* dca, const float* dcb,
                              float* da, float* db, long N, long C, int H, int W, int levels, int scale, float C1, float C2,
                              faoctasr_stream_t stream);

/* ---- HaarPSI (csrc/haarpsi.hip) -----------------------------------------------------------------
 * x, y: contiguous (planes, H, W), planes = N * C, H, W >= 2; every plane a grey image.  u = (x - lo) 255 / (hi - lo), hi > lo; u2 its 2 x 2
 * mean at every second pixel (samples beyond the image 0, divisor 4), (H + 1) / 2 by (W + 1) / 2; g^o_k, o in {v, h}, k = 1, 2, 3, the Haar
 * coefficients of u2 on 2^k x 2^k windows (2^-k times the difference of the two half-window sums; window rows i - 2^(k-1) + 1 ..
 * i + 2^(k-1), u2 zero outside the map); a_k = |g^o_k(x)|, b_k = |g^o_k(y)|:
 *   S_o = 1/2 sum_{k = 1, 2} (2 a_k b_k + c) / (a_k^2 + b_k^2 + c),  W_o = max(a_3, b_3),  c > 0, alpha > 0,
 *   r[n] = sum_{ch, o, p} sigmoid(alpha S_o) W_o / sum W_o,  HaarPSI[n] = (log(r / (1 - r)) / alpha)^2, 1 where sum W_o == 0.
 * index: one partial of sum (sigmoid(alpha) - sigmoid(alpha S_o)) W_o and one of sum W_o per block into the workspace of
 *   faoctasr_haarpsi_workspace_floats(planes, H, W) floats (-1 on a bad shape); no atomics.
 * final: adds an image's partials in double in a fixed order; out_image[n] = HaarPSI[n], out_mean[0] = their mean.  fac (2, N), may be
 *   NULL: fac[0][n] = dHaarPSI[n]/dr / sum W_o (times 1 / N when average != 0; 0 where sum W_o == 0), fac[1][n] = sigmoid(alpha) - r[n].
 * grad: dx, dy (either may be NULL, not both) = fac[0][n] g[n or 0] d(r[n] sum W_o)/d(x|y) at fixed sum W_o and r taken from fac[1],
 *   which is g dHaarPSI/d(x|y); g is a DEVICE array of gN floats (1 = shared, or N).  d|g|/dg = sign(g), sign(0) = 0; in max(a_3, b_3)
 *   the gradient goes to the larger side, at equality to x.
 * For x == y HaarPSI is exactly 1 and both gradients exactly 0; swapping x and y leaves it bit for bit and swaps the gradients. */
long faoctasr_haarpsi_workspace_floats(long planes, int H, int W);
int faoctasr_haarpsi_index(const float* x, const float* y, float* workspace, long planes, int H, int W, float lo, float hi, float c, float alpha,
                           faoctasr_stream_t stream);
int faoctasr_haarpsi_final(const float* workspace, long N, long C, int H, int W, double alpha, int average, float* out_image, float* out_mean,
                           float* fac, faoctasr_stream_t stream);
int faoctasr_haarpsi_grad(const float* x, const float* y, const float* fac, const float* g, int gN, float* dx, float* dy, long N, long C, int H,
                          int W, float lo, float hi, float c, float alpha, faoctasr_stream_t stream);

/* ---- local normalised cross-correlation (csrc/lncc.hip) -----------------------------------------------
 * a, b: contiguous (planes, H, W), planes = N * C.  win odd in 3..15, n = win^2, eps > 0; box(t)_p the sum of t over the win x win window
 * centred on p, samples beyond the image 0 (the window may be larger than the image):
 *   u = box(a b) - box(a) box(b) / n,  va = box(a a) - box(a)^2 / n,  vb = box(b b) - box(b)^2 / n,
 *   cc_p = u^2 / (va vb + eps),  LNCC[n] = the mean of cc_p over c, y, x.
 * index: one partial sum of cc_p per block into the workspace of faoctasr_lncc_workspace_floats(planes, H, W) floats (-1 on a bad
 *   shape); no atomics.
 * final: adds an image's partials in double in a fixed order; out_image[n] = LNCC[n], out_mean[0] = their mean.  fac (N), may be NULL:
 *   fac[n] = 1 / (C H W), times 1 / N when average != 0.
 * grad: da, db (either may be NULL, not both) = fac[n] g[n or 0] d(sum cc_p)/d(a|b), which is g dLNCC/d(a|b); g is a DEVICE array of
 *   gN floats (1 = shared, or N).  Nothing is clamped.
 * Swapping a and b leaves LNCC bit for bit and swaps the gradients; halving g halves them bit for bit. */
long faoctasr_lncc_workspace_floats(long planes, int H, int W);
int faoctasr_lncc_index(const float* a, const float* b, float* workspace, long planes, int H, int W, int win, float eps,
                        faoctasr_stream_t stream);
int faoctasr_lncc_final(const float* workspace, long N, long C, int H, int W, int average, float* out_image, float* out_mean, float* fac,
                        faoctasr_stream_t stream);
int faoctasr_lncc_grad(const float* a, const float* b, const float* fac, const float* g, int gN, float* da, float* db, long N, long C, int H,
                       int W, int win, float eps, faoctasr_stream_t stream);

/* ---- GMSD and multi-scale GMSD (csrc/gmsd.hip) --------------------------------------------------------
 * a, b: contiguous (planes, H, W), planes = N * C, independent grey planes pooled inside an image.  u = (x - lo) / (hi - lo), hi > lo;
 * pool(t) = avg_pool2d(t, 2), floor pooling.  Prewitt gradients, zero padding 1, the size of their input:
 *   gx_p = (1/3) sum_{dy = -1..1} (t[y + dy][x - 1] - t[y + dy][x + 1]), gy_p the same on the other axis, m_p = sqrt(gx_p^2 + gy_p^2), no epsilon;
 *   g_p = (2 ma_p mb_p + c) / (ma_p^2 + mb_p^2 + c), c > 0;  V[n] = the population variance of g_p over the channels and positions of image n.
 * pooled != 0 (scales = 1, sides at least 2): GMSD[n] = sqrt(V[n]) on pool(u_a), pool(u_b), staged straight from a, b.
 * pooled == 0: MS-GMSD[n] = sqrt(sum_j w_j V_j[n]) over 1 <= scales <= 5; scale 0 is the mapped input, scale j + 1 = pool(scale j), of
 *   (H >> j) x (W >> j); sides at least 2^(scales - 1).  Both are distortions: 0 for identical images.
 * index, once per scale: a, b are that scale's pair (the inputs themselves at scale 0 and in the pooled form); writes one partial sum of
 *   d_p = 1 - g_p and one of d_p^2 per block into the scale's part of the workspace of faoctasr_gmsd_workspace_floats(planes, H, W, scales,
 *   pooled) floats (-1 on a bad shape); no atomics.  next_a, next_b (both or neither; not in the pooled form, not at the last scale) take
 *   the pair of scale + 1.  workspace NULL (a scale of weight 0): only pools.
 * final: weights is a HOST array of `scales` doubles, each finite and >= 0, not all zero (pooled: {1}); adds the partials in double in a
 *   fixed order, skipping scales of weight 0; out_image[n] the score, out_mean[0] their mean.  table (2, scales, N), may be NULL:
 *   table[0][j][n] = mean of d_p, table[1][j][n] = w_j / (score[n] P_j), P_j = C h_j w_j, times 1 / N when average != 0, 0 where score[n] == 0.
 * grad, once per scale, coarsest first: da, db (either may be NULL, not both) of that scale's size (of H x W in the pooled form) =
 *   g[n or 0] d score[n] / d (a | b) of this scale's term plus 0.25 dca / dcb [y >> 1][x >> 1], the gradient of scale + 1 (NULL at the last
 *   scale and in the pooled form); g is a DEVICE array of gN floats (1 = shared, or N).  Where m_p == 0 that image's direction is (0, 0);
 *   where score[n] == 0 the gradient is exactly zero.
 * Swapping a and b leaves the score bit for bit and swaps the gradients; halving g halves them bit for bit. */
long faoctasr_gmsd_workspace_floats(long planes, int H, int W, int scales, int pooled);
int faoctasr_gmsd_index(const float* a, const float* b, float* next_a, float* next_b, float* workspace, long planes, int H, int W, int scales,
                        int scale, int pooled, float lo, float hi, float c, faoctasr_stream_t stream);
int faoctasr_gmsd_final(const float* workspace, long N, long C, int H, int W, int scales, int pooled, const double* weights, int average,
                        float* out_image, float* out_mean, float* table, faoctasr_stream_t stream);
int faoctasr_gmsd_grad(const float* a, const float* b, const float* table, const float* g, int gN, const float* dca, const float* dcb, float* da,
                       float* db, long N, long C, int H, int W, int scales, int scale, int pooled, float lo, float hi, float c,
                       faoctasr_stream_t stream);

/* ---- Hessian vesselness and the vessel Dice index (csrc/vessel.hip) --------------------------------------
 * x, y: contiguous (N, C, H, W), channels independent grey planes pooled inside an image, any sides >= 1.  u = (x - lo) / (hi - lo), hi > lo.
 * sigmas, weights: HOST arrays of `scales` doubles (1..3), read during the call; the taps are computed from them in double and passed to
 *   the kernel by value (nothing is allocated or copied: the launch is capturable).  Every sigma in [0.5, 3], every weight positive and
 *   finite; the caller drops scales of weight 0 and normalises the rest to sum 1.  Per scale R = int(3 sigma + 0.5), t = -R..R,
 *   g = exp(-t^2 / (2 sigma^2)) / sum, g1 = -t / sigma^2 g, g2 = (t^2 / sigma^4 - 1 / sigma^2) g;
 *   a = sigma^2 (g2 along W, g along H) * u, b = sigma^2 (g1, g1) * u, d = sigma^2 (g along W, g2 along H) * u: true convolutions, zero padding;
 *   bright == 0 negates a, b, d.  m = (a + d) / 2, h = (a - d) / 2, r = sqrt(h^2 + b^2), kappa = r - m, mu = m + r,
 *   E1 = mu^2 / (2 beta^2 kappa^2), E2 = (mu^2 + kappa^2) / (2 c^2), V = exp(-E1) (1 - exp(-E2)) where kappa > 0 and E1 < 87, else exactly 0;
 *   Rsp = sum_s w_s V_s;  S[n] = (2 mean(A B) + eps) / (mean(A^2) + mean(B^2) + eps) with A = Rsp(x), B = Rsp(y).
 * index: with y, writes one partial each of A B, A^2, B^2 per block into the workspace of faoctasr_vessel_workspace_floats(N, C, H, W)
 *   floats (-1 on a bad shape; 8-byte aligned) and, given map_x and map_y (both or neither), the two response maps the backward reads.
 *   With y NULL (and no workspace, no map_y) it writes the response map of x into map_x: the vesselness filter.
 * final: adds the partials in double in a fixed order, a wave per image; out_image[N]; out_mean (may be NULL) the batch mean; table (may
 *   be NULL) [2][N]: S and 1 / (P D), P = C H W, D the denominator (times 1 / N with `average`).
 * grad: with a table, the index's gradient: g is a DEVICE array of gN floats (1 = shared, or N); a NULL dx or dy skips that side.  With
 *   table NULL (and y, the maps and dy NULL) the filter's: g is the upstream map, the size of x.
 * Swapping x and y leaves the score bit for bit and swaps the gradients; halving g halves them bit for bit.  No atomics. */
long faoctasr_vessel_workspace_floats(long N, long C, int H, int W);
int faoctasr_vessel_index(const float* x, const float* y, float* map_x, float* map_y, float* workspace, long N, long C, int H, int W,
                          const double* sigmas, const double* weights, int scales, float beta, float c, float lo, float hi, int bright,
                          faoctasr_stream_t stream);
int faoctasr_vessel_final(float* workspace, long N, long C, int H, int W, double eps, int average, float* out_image, float* out_mean,
                          float* table, faoctasr_stream_t stream);
int faoctasr_vessel_grad(const float* x, const float* y, const float* map_x, const float* map_y, const float* table, const float* g, int gN,
                         float* dx, float* dy, long N, long C, int H, int W, const double* sigmas, const double* weights, int scales,
                         float beta, float c, float lo, float hi, int bright, faoctasr_stream_t stream);

/* ---- visual information fidelity, pixel domain (VIFp; csrc/vif.hip) ---------------------------------------
 * x (the image under test), r (the reference): contiguous (N, C, H, W), H, W >= 41, channels independent grey planes pooled inside an
 * image.  u = (t - lo) * 255 / (hi - lo), hi > lo; EPS = 1e-8; sigma_n_sq finite and > 0.  Scale s = 0..3: K_s = 2^(4-s) + 1,
 *   w_s[k] = exp(-(k - (K_s-1)/2)^2 / (2 (K_s/5)^2)) / sum (computed in double during the call, passed to the kernel by value: nothing is
 *   allocated or copied, every launch is capturable); W_s * t the separable VALID convolution; at s > 0 x_s = (W_s * x_{s-1})[::2, ::2], r_s
 *   likewise.  mx = W_s*x_s, mr = W_s*r_s, sxx = relu(W_s*(x_s x_s) - mx^2), srr = relu(W_s*(r_s r_s) - mr^2), sxr = W_s*(x_s r_s) - mx mr,
 *   g = sxr / (srr + EPS), sv = sxx - g sxr, then in this order: srr < EPS: g = 0, sv = sxx, srr = 0; sxx < EPS: g = 0, sv = 0;
 *   g < 0: sv = sxx, g = 0; sv <= EPS: sv = EPS.  num_s[n] = sum log10(1 + g^2 srr / (sv + sigma_n_sq)), den_s[n] = sum log10(1 + srr / sigma_n_sq);
 *   V[n] = (sum_s num_s + EPS) / (sum_s den_s + EPS).  V(x, r) is NOT V(r, x).
 * H, W are always the sides of scale 0; the sides of scale s + 1 are (side_s - K_{s+1} + 2) / 2.
 * scale_fwd, once per scale in any order after the scale's pair exists: x, r are the pair of that scale (scale 0: the inputs, mapped
 *   inside); writes one partial of num and one of den per block into the workspace of faoctasr_vif_workspace_floats(N, C, H, W) floats
 *   (-1 on a bad shape) and, at scales 0..2, the pair of the next scale into next_x, next_r (NULL at scale 3).
 * final: adds an image's partials in double in a fixed order, a wave per image; out_image[N]; out_mean (may be NULL) the batch mean,
 *   from the same launch; table (may be NULL) [2][N]: 1 / ((den + EPS) ln 10) and V / ((den + EPS) ln 10), times 1 / N with `average`.
 * scale_bwd, once per scale, coarsest first: x, r the pair of that scale, g a DEVICE array of gN floats (1 = shared, or N), dnext_x /
 *   dnext_r the gradients scale + 1 wrote (NULL at scale 3); writes the gradient with respect to that scale's pair, at scale 0 that of
 *   the inputs.  A NULL dx or dr skips that side (its dnext is then NULL too).
 * Halving g halves the gradients bit for bit; one side's gradient has the same bits with or without the other.  No atomics. */
long faoctasr_vif_workspace_floats(long N, long C, int H, int W);
int faoctasr_vif_scale_fwd(const float* x, const float* r, float* next_x, float* next_r, float* workspace, long N, long C, int H, int W,
                           int scale, float lo, float hi, float sigma_n_sq, faoctasr_stream_t stream);
int faoctasr_vif_final(const float* workspace, long N, long C, int H, int W, int average, float* out_image, float* out_mean, float* table,
                       faoctasr_stream_t stream);
int faoctasr_vif_scale_bwd(const float* x, const float* r, const float* table, const float* g, int gN, const float* dnext_x,
                           const float* dnext_r, float* dx, float* dr, long N, long C, int H, int W, int scale, float lo, float hi,
                           float sigma_n_sq, faoctasr_stream_t stream);

/* ---- soft-clDice: soft skeletons and the centre-line Dice (csrc/cldice.hip) -------------------------------
 * x, y: contiguous (N, C, H, W), channels independent grey planes pooled inside an image, any sides >= 1, finite values.
 *   u = (x - lo) / (hi - lo), hi > lo; bright == 0 uses (hi - x) / (hi - lo).  iters = K in 1..10.
 *   E(I)[q] = min of I over the cross {up, left, q, right, down}, D(I)[q] = max over the 3 x 3 square, positions outside the image left out;
 *   I_0 = u, I_{k+1} = E(I_k), O_k = D(I_{k+1}), delta_k = relu(I_k - O_k), k = 0..K; s_0 = delta_0, s_k = s_{k-1} + relu(delta_k - s_{k-1} delta_k);
 *   skel(u) = s_K.  Tprec = (sum skel(x) u_y + smooth) / (sum skel(x) + smooth), Tsens = (sum skel(y) u_x + smooth) / (sum skel(y) + smooth), sums
 *   over the channels and positions of image n, a ratio of denominator 0 taken as 0; S[n] = 2 Tprec Tsens / (Tprec + Tsens), 0 where that
 *   denominator is 0.
 * Records (written only where asked, read by grad): per side rec [K + 1][N][C][H][W] floats, the coefficient c_k that turns the skeleton's
 *   cotangent at q into that of delta_k at q, and sel [K + 1][N][C][H][W] bytes: bits 0-2 the arg-min of q's cross in I_k (up, left, centre,
 *   right, down = 0..4), bits 3-6 the arg-max of q's square in I_{k+1} (3 (dy + 1) + (dx + 1) = 0..8), each the FIRST position in that
 *   order whose value equals the result: the tie rule, a valid subgradient, which on plateaus differs from a framework's pooling backward.
 * index: with y, writes one partial each of sum skel(x) u_y, sum skel(x), sum skel(y) u_x, sum skel(y) per block into the workspace of
 *   faoctasr_cldice_workspace_floats(N, C, H, W) floats (-1 on a bad shape; 8-byte aligned); skel_x, skel_y (each may be NULL) take the
 *   skeleton maps, rec_x / sel_x and rec_y / sel_y (each pair or NULL) the records.  With y NULL (and no workspace, skel_y, rec_y, sel_y) it
 *   writes the skeleton map of x into skel_x and, given rec_x / sel_x, its records: the soft-skeleton filter.
 * final: adds the partials in double in a fixed order, a wave per image; out_image[N]; out_mean (may be NULL) the batch mean, from the
 *   same call; table (may be NULL) [4][N]: dS / d(each of the four sums, in the order above), times 1 / N with `average`.
 * grad: with a table, the index's gradient: g is a DEVICE array of gN floats (1 = shared, or N); dx needs rec_x, sel_x and skel_y, dy needs
 *   rec_y, sel_y and skel_x; a NULL dx or dy skips that side and leaves the other side's bits.  With table NULL (and y, dy, rec_y, sel_y
 *   NULL) the filter's: g is the upstream map, the size of x.  The kernel routes cotangents by the records alone, level K down to 0, in
 *   gather form: it does not repeat the forward's arithmetic.
 * Swapping x and y leaves the score bit for bit and swaps the gradients; halving g halves them bit for bit.  No atomics. */
long faoctasr_cldice_workspace_floats(long N, long C, int H, int W);
int faoctasr_cldice_index(const float* x, const float* y, float* skel_x, float* skel_y, float* rec_x, unsigned char* sel_x, float* rec_y,
                          unsigned char* sel_y, float* workspace, long N, long C, int H, int W, int iters, float lo, float hi, int bright,
                          faoctasr_stream_t stream);
int faoctasr_cldice_final(float* workspace, long N, long C, int H, int W, double smooth, int average, float* out_image, float* out_mean,
                          float* table, faoctasr_stream_t stream);
int faoctasr_cldice_grad(const float* x, const float* y, const float* rec_x, const unsigned char* sel_x, const float* rec_y,
                         const unsigned char* sel_y, const float* skel_x, const float* skel_y, const float* table, const float* g, int gN,
                         float* dx, float* dy, long N, long C, int H, int W, int iters, float lo, float hi, int bright,
                         faoctasr_stream_t stream);

/* ---- losses (train.py:91-99) -----------------------------------------------------------------
 * kind 0: sum (a-b)^2 (MSELoss), 1: sum |a-b| (L1Loss), 2: BCEWithLogits(input=a, target=b) sum.
 * out[0] = scale * sum (overwritten); workspace: faoctasr_loss_workspace_floats() floats.  */
long faoctasr_loss_workspace_floats(void);
int faoctasr_loss_fwd(const float* a, const float* b, float* out, long n, int kind, float scale, float* workspace,
                      faoctasr_stream_t stream);
/* gradient wrt `wrt` (0 = a, 1 = b): d = g[0]*scale * dloss/d(...) ; g is a device scalar */
int faoctasr_loss_bwd(const float* a, const float* b, const float* g, float* d, long n, int kind, float scale, int wrt,
                      faoctasr_stream_t stream);
/* discriminator head model.py:158-164: out[n] = wa*mean(a[n,:]) + wb*mean(b[n,:]) */
int faoctasr_mean_mix_fwd(const float* a, const float* b, float* out, int N, int La, int Lb, float wa, float wb,
                          faoctasr_stream_t stream);
int faoctasr_mean_mix_bwd(const float* g, float* da, float* db, int N, int La, int Lb, float wa, float wb,
                          faoctasr_stream_t stream);

/* ---- optimizer: torch.optim.AdamW step (train.py:102-103,239,269) over one flat arena -------- */
int faoctasr_adamw_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                        float eps, float weight_decay, int step, float grad_scale, faoctasr_stream_t stream);
/* The same update with the scalars in DEVICE memory (for a hipGraph-captured step, SURVEY 8f-1: the graph replays with each
 * step's own values): hyper[8] = {lr, beta1, beta2, eps, weight_decay, lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t), grad_scale}. */
int faoctasr_adamw_step_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, faoctasr_stream_t stream);

/* ---- input pipeline: the tensor transforms of train.py:129-140 fused into one pass ---------------------------
 * img [N,H,W] uint8 grayscale (what Image.open(..).convert('L') + ToTensor hold before the /255), tops/lefts [N] device ints =
 * the RandomCrop offsets (drawn by the caller), out [N,1,out_size,out_size] fp32:
 *   out = (resize(crop(img)/255) - mean) / std,  resize = torch bicubic (align_corners false, A = -0.75) when out_size != crop
 * transforms_A = crop 128 -> 256 bicubic; transforms_B = crop 256, no resize (the Normalize/RandomCrop order there commutes). */
int faoctasr_prep_crop_resize(const unsigned char* img, const int* tops, const int* lefts, float* out, int N, int H, int W,
                              int crop, int out_size, float mean, float std, faoctasr_stream_t stream);

/* ---- data-parallel gradient exchange over RCCL ---------------------------------------------------------
 * The reference has no distributed code; a DDP wrap of its loop would all-reduce after loss_G.backward() (train.py:238) and
 * after the discriminator backwards (train.py:255,267).  Here that is ONE in-place SUM all-reduce per flat gradient arena,
 * enqueued on the caller's stream (capturable in a hipGraph); the 1/world average is folded into adamw_step's grad_scale.
 * librccl is bound at run time (dlopen; the copy already in the process when there is one) -- single-GPU hosts never load it.
 * comm handles: rank 0 fills a 128-byte id (ncclUniqueId) and ships it to the other ranks by any host channel; every rank
 * then calls comm_create with the device it will use current.  These three calls are the only ones that create state.  */
int faoctasr_comm_unique_id(void* id128);
int faoctasr_comm_create(void** comm, int nranks, int rank, const void* id128);
int faoctasr_comm_destroy(void* comm);
int faoctasr_comm_size(void* comm);                 /* number of ranks (> 0) or a negative error */
/* dtype: 0 = fp32 (the only arena type) */
int faoctasr_grad_allreduce(float* bucket, long count, int dtype, void* comm, faoctasr_stream_t stream);
/* identical replicas at start: rank `root`'s parameter arena / BatchNorm buffers to everyone, in place */
int faoctasr_param_broadcast(float* buf, long count, int root, void* comm, faoctasr_stream_t stream);

/* ---- evaluation path: utils.py:182-242 `eval` / `eval_6m` ------------------------------------------------------
 * The four skimage metrics of utils.py:209-212 on device images: y, gt [N][H][W] fp32; out [N][4] doubles = {PSNR
 * (peak_signal_noise_ratio, data_range), SSIM (structural_similarity defaults: 7x7 uniform window, sample covariance, map cropped
 * by 3), MSE, NMI (normalized_mutual_information: joint bins x bins histogram over each image's [min, max], numpy.histogram2d
 * bin semantics)}.  data_range = 2, bins = 100 reproduce the reference.  workspace: faoctasr_eval_workspace_bytes(N, bins) bytes.
 * Every sum has a fixed order (no floating-point atomics): two calls on the same images give the same bits. */
long faoctasr_eval_workspace_bytes(int N, int bins);
int faoctasr_eval_metrics(const float* y, const float* gt, double* out, void* workspace, int N, int H, int W, float data_range, int bins,
                          faoctasr_stream_t stream);
/* `model.eval()` (utils.py:186,221) makes every BatchNorm2d a per-channel affine map; folded into the preceding convolution:
 * w_folded = w * gamma / sqrt(running_var + eps) per output channel m, bias_folded = (bias - running_mean) * that + beta.
 * w is [M][K] (Conv2d; transposed = 0) or [K0][M][K] (ConvTranspose2d weight [C][M][kh*kw]; transposed = 1).            */
int faoctasr_bn_fold(const float* w, const float* bias, const float* gamma, const float* beta, const float* running_mean,
                     const float* running_var, float eps, float* w_folded, float* bias_folded, int M, long K, int transposed, long K0,
                     faoctasr_stream_t stream);

/* ---- utility ---------------------------------------------------------------------------------- */
int faoctasr_fill(float* p, long n, float value, faoctasr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FAOCTASR_H */
