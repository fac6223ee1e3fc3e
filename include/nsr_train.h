/* nsr_train.h — C ABI of the TRAINING step through the NeRF-SR render path.
 *
 * Same conventions as nsr.h: raw DEVICE pointers, caller-owned memory, work enqueued on the caller's HIP
 * stream, int status returns, no global mutable state.  The reference interface replaced here is
 * NeRFDownXModel.optimize_parameters (models/nerf_downX_model.py:398-408):
 *     forward()  [train mode: randomized sampling, density noise]   -> nsr_train_loss_and_grads
 *     comp_low_res_output() + calculate_losses() + loss_tot.backward()  -> nsr_train_loss_and_grads
 *     optimizer.step()  [torch.optim.Adam, :201-204]                 -> nsr_adam_step
 * Weights, gradients and Adam moments are the 24 tensors of VanillaMLP.state_dict() in nn.Linear layout
 * (see NSR_N_STATE_TENSORS in nsr.h), handed over as HOST arrays of 24 DEVICE pointers, so a binding can
 * pass `p.data_ptr()` / `p.grad.data_ptr()` of the reference's own parameters.
 *
 * Arithmetic: fp32 storage and accumulation throughout, like the reference.  precision = NSR_FP32: every contraction on
 * v_mfma_f32_32x32x2_f32, layer by layer.  precision = NSR_F16X3: the network as two fused chain launches per pass
 * (DESIGN 7.1): forward pass and input gradients on split-fp16 v_mfma_f32_32x32x16_f16 with fp32-grade products (hi/lo
 * operands, three MFMAs per product; gradients scaled by exact powers of two per point); the WEIGHT gradients contract
 * the chain's fp16 `hi` operands (activation and input gradient rounded to 11 bits, one MFMA per product, fp32
 * accumulation over the sample points: a gradient tensor moves by < 1e-4 of its norm, less than fp32-vs-fp64 of the
 * reference's own arithmetic).  precision = NSR_F16X3_GEMM: layer-by-layer GEMMs, forward products split-fp16, every
 * gradient on the fp32 MFMA (round 1's design; the chain path's A/B partner).
 */
#ifndef NSR_TRAIN_H_
#define NSR_TRAIN_H_

#include "nsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A third `precision` value, valid for the training entry points only (nsr_precision in nsr.h holds the others). */
#define NSR_F16X3_GEMM 18
/* The chain path with the arithmetic of its BACKWARD chain (the input gradients dz_{l-1} = W_l^T dz_l) named explicitly
 * (round 6; forward pass and weight gradients as under NSR_F16X3 in all three):
 *   NSR_F16X3_BWD3: W_hi g_hi + W_hi g_lo + W_lo g_hi, three MFMAs per product, fp32-grade (rounds 2-5's arithmetic);
 *   NSR_F16X3_BWD2: W_hi g_hi + W_lo g_hi: the gradient entering a layer is its fp16 `hi` alone (11 bits, scaled per point by a
 *                   power of two), the weights keep their 22 bits;
 *   NSR_F16X3_BWD1: W_hi g_hi: one MFMA per product, both operands rounded to 11 bits;
 *   NSR_F16X3_BWDM: mixed -- two terms (as _BWD2) on the six layers nearest the output (dir_encoding, xyz_encoding_final,
 *                   xyz_encoding_8 .. _5), one (as _BWD1) on the three below (xyz_encoding_4 .. _2), whose rounding passes
 *                   through the fewest further layers.
 * NSR_F16X3 selects the cheapest of them whose gradients stay inside the bounds of tests/test_gpu_train.py (every gradient
 * tensor within 2e-3 of its norm of the fp64 oracle, 5e-4 on the heads, a 200-step Adam trajectory no further from the fp32
 * run than another fp32-grade implementation is; the whole gradient within 2e-4 of the fp32-gradient path at 393,216 sample
 * points): NSR_F16X3_BWDM as of NSR_VERSION 131 (measured 4.0e-4 / 7e-5 on the heads / whole gradient 1.0e-4; NSR_VERSION 130:
 * NSR_F16X3_BWD2, 2.0e-4 / 7e-5 / 1.8e-5).  NSR_F16X3_BWD1 is a stated FAST path: it holds the per-tensor bounds (measured
 * 6.6e-4 / 2.2e-4 on the heads) and the trajectory bound, not the whole-gradient one (3.1e-4) -- measured: DESIGN.md 7.1. */
#define NSR_F16X3_BWD3 19
#define NSR_F16X3_BWD2 20
#define NSR_F16X3_BWD1 21
#define NSR_F16X3_BWDM 22
/* NSR_F16X3_GEMM with its BACKWARD products on the split-fp16 MFMA too (opt-in; 23 stays unknown).  It is accepted wherever
 * NSR_F16X3_GEMM is (nsr_train_loss_and_grads[_var], nsr_train_forward / _backward, nsr_train_arch_* with their _e / _r forms,
 * every size function) and refused wherever that is (e.g. nsr_train_backward_r with g_rays: NSR_ERR_UNSUPPORTED).
 *   Forward: NSR_F16X3_GEMM's -- the same launches, the same bits, the same saved-state format and size.
 *   Backward: every product of the layer-by-layer network -- the input gradients, the weight gradients, the products onto the
 *   encoded-position / encoded-direction columns of nsr_train_arch_backward_r -- runs on v_mfma_f32_32x32x16_f16 with three
 *   terms (lo hi + hi lo + hi hi, small terms first, fp32 accumulation: products exact to ~2^-21) instead of
 *   v_mfma_f32_32x32x2_f32.  Everything that is not a product (bias sums, reductions, encodings' and compositing backward,
 *   --stop_grad, Adam) is what it is under NSR_F16X3_GEMM; the colour and density heads' bias gradients have its bits.
 *   Range: gradients are brought into fp16's range by exact powers of two, removed again before the store.  An input gradient
 *   scales every ROW (sample point) of the incoming gradient by its own power of two (row max -> [2^13, 2^14)): a row of the
 *   result depends on that row, its mask row and the weights only -- not on the batch, the ray chunk or its neighbours -- so
 *   the rows of g_rays stay bit-identical across ray_chunk and batch order.  A weight gradient (a contraction over the
 *   points) scales the matrix by one power of two from its largest magnitude, kept in a device word by integer maximum.
 *   Zero rows / matrices and NaN use 1; non-finite values pass through.  No float atomics: identical calls, identical bits;
 *   scaling the upstream gradients by a power of two scales every gradient by exactly it.
 *   Workspace: NSR_F16X3_GEMM's layout with a tail behind it (the transposed split copies of the weights the input gradients
 *   read, re-made by every call that runs a backward, and 64 range words); the size functions include it for this value only.
 * The backward takes its arithmetic from the precision recorded in the saved header. */
#define NSR_F16X3_GEMM_BWD 24

/* Workspace for one pass over `ray_chunk` rays (activations of one network, gradient buffers, padded weight copies,
 * split-K partials; for NSR_F16X3 the activation / gradient panels, ~24 KB per sample point in all).  0 on invalid
 * arguments. */
size_t nsr_train_workspace_bytes(int64_t ray_chunk, int n_coarse, int n_importance);
/* The same for the path `precision` selects (what nsr_train_loss_and_grads checks): NSR_F16X3 -> the chain path's 2-byte
 * panels, sign words and weight streams without the per-layer activation / gradient matrices of the GEMM path (~11 KB per
 * sample point); NSR_FP32 / NSR_F16X3_GEMM -> the GEMM path's buffers without the panels (~13 KB).
 * nsr_train_workspace_bytes is the union: sufficient whatever runs.  Both depend on their arguments only.
 * Behind its first 64 bytes (the sticky status block, nsr_train_status below) a workspace is scratch for every entry point of
 * this header: its contents on entry do not matter and are unspecified on return. */
size_t nsr_train_workspace_bytes_for(int precision, int64_t ray_chunk, int n_coarse, int n_importance);

/* Losses and d(loss_tot)/d(weights) of one batch.
 *   loss_tot = lambda_coarse * mse(mean_s2(coarse rgb), target) + lambda_fine * mse(mean_s2(fine rgb), target)
 *   (calculate_losses, nerf_downX_model.py:355-362; nn.MSELoss(reduction='mean'), criterions.py:7-15).
 * rays (R, ray_stride) LR-pixel-major with s2 sub-rays per LR pixel (s2 = 1: the vanilla `nerf` model);
 * target_lr (R / s2, 3).
 * Random draws are INPUTS (the reference draws them with torch.rand_like / torch.randn_like / torch.rand,
 * models/utils.py:37-41, 72-73, 199-212): u_coarse (R, Nc), u_fine (R, Ni) uniform in [0, 1); noise_coarse
 * (R, Nc), noise_fine (R, Nc + Ni) standard normal, scaled by noise_std.  NULL selects the deterministic
 * branch of the corresponding stage (randomized = False / noise off).
 * g_coarse / g_fine: 24 gradient tensors each, OVERWRITTEN.
 * precision: NSR_FP32 = every product on the fp32 MFMA; NSR_F16X3 = the chain kernels (forward and input gradients on the
 * split-fp16 MFMA, exact to ~2^-21, the inference path's scheme; weight gradients on one fp16 MFMA per product);
 * NSR_F16X3_GEMM = round 1's variant: per-layer GEMMs, forward products split-fp16, gradients on the fp32 MFMA.  The
 * path is a function of this argument alone: no environment variable, no process state.
 * ray_chunk: rays per pass (bounds the workspace; multiple of s2; 0 = R); gradients and losses of the passes
 * are accumulated, the result does not depend on the chunking beyond fp32 summation order.  Every pass -- the
 * shorter last one included -- must hold a multiple of 32 sample points in both networks
 * (rays_in_pass * n_coarse and rays_in_pass * (n_coarse + n_importance) divisible by 32: the weight-gradient
 * GEMM contracts over the points in K tiles of 32); otherwise NSR_ERR_UNSUPPORTED is returned before anything
 * is enqueued (outputs and gradients untouched).  All of the reference's scripts (64 + 64 samples) satisfy it
 * for any ray count.
 * render_flags (`white_bkgd` until NSR_VERSION 120): a word of options like the render path's (include/nsr.h): NSR_WHITE_BKGD and NSR_SIGMA_SOFTPLUS as there
 * (the backward pass carries sigmoid(sigma - 1) instead of [sigma > 0]), and the colour head's two, which the render
 * path keeps in the packed network: NSR_TRAIN_GAMMA_CORRECT = --gamma_correct while training (render_rays returns
 * pow(rgb, 1 / 2.2) per sample, nerf_downX_model.py:271-276; the colours are corrected between the network and the
 * compositor and the backward pass carries the slope y (1 - y^2.2) / 2.2 of the corrected sigmoid);
 * NSR_TRAIN_COLOR_NONE = --color_activation none (models/networks.py:173-180; slope 1); NSR_TRAIN_STOP_GRAD =
 * --stop_grad true (models/networks.py:218-219: the colour branch's input is detached -- xyz_encoding_final gets zero
 * gradients, the trunk the density head's alone).  Gamma and none together are
 * NSR_ERR_UNSUPPORTED (the power of an unbounded head is NaN for every negative value); any other bit NSR_ERR_INVALID_ARG.
 * outs: the 8 forward outputs in nsr_forward_rays order (entries may be NULL except the two comp_rgbs).
 * lr_coarse / lr_fine: (R / s2, 3) s2-means (comp_low_res_output, :326-348); losses: DEVICE float[2] =
 * { lambda_coarse * mse_coarse, lambda_fine * mse_fine }. */
#define NSR_TRAIN_GAMMA_CORRECT 4
#define NSR_TRAIN_COLOR_NONE 8
#define NSR_TRAIN_STOP_GRAD 16
int nsr_train_loss_and_grads(const float* const* w_coarse, const float* const* w_fine, float* const* g_coarse,
                             float* const* g_fine, const float* rays, int ray_stride, int64_t R, int s2,
                             const float* target_lr, int n_coarse, int n_importance, int render_flags, int lindisp,
                             const float* u_coarse, const float* u_fine, const float* noise_coarse,
                             const float* noise_fine, float noise_std, float lambda_coarse, float lambda_fine,
                             int precision, int64_t ray_chunk, float* const* outs, float* lr_coarse, float* lr_fine, float* losses,
                             void* workspace, size_t workspace_bytes, void* stream);

/* The optional variance losses of comp_low_res_output / calculate_losses (nerf_downX_model.py:332-336, 349-353, 374-378;
 * options --use_var_loss / --use_depth_var_loss, :107-112):
 *   loss_tot += lambda_coarse_var * sum_{LR pixels, channels} var_{s2 sub-rays}(coarse rgb) + lambda_fine_var * (fine rgb)
 *   loss_tot += lambda_coarse_depth_var * sum_{LR pixels} var_{s2 sub-rays}(coarse depth / far) + lambda_fine_depth_var * (fine)
 * with torch.var's default (unbiased: divisor s2 - 1) and `far` = the reference's self.far (:284: the far bound of the batch's
 * first ray).  A lambda of 0 switches its term off.  s2 must be >= 2 when any lambda is non-zero (the variance of one sub-ray
 * is 0 / 0: the reference would train on NaN) -- NSR_ERR_INVALID_ARG otherwise. */
typedef struct nsr_train_var_losses {
  float lambda_coarse_var, lambda_fine_var;
  float lambda_coarse_depth_var, lambda_fine_depth_var;
  float far;
} nsr_train_var_losses;
/* nsr_train_loss_and_grads with those terms in the loss and in the gradients.  var_losses (may be NULL): DEVICE float[4] =
 * { lambda_coarse_var * var_c, lambda_fine_var * var_f, lambda_coarse_depth_var * dvar_c, lambda_fine_depth_var * dvar_f },
 * the reference's loss_out_{coarse,fine}_var / loss_{coarse,fine}_depth_var times their lambdas.  Every other argument as above. */
int nsr_train_loss_and_grads_var(const float* const* w_coarse, const float* const* w_fine, float* const* g_coarse,
                                 float* const* g_fine, const float* rays, int ray_stride, int64_t R, int s2,
                                 const float* target_lr, int n_coarse, int n_importance, int render_flags, int lindisp,
                                 const float* u_coarse, const float* u_fine, const float* noise_coarse,
                                 const float* noise_fine, float noise_std, float lambda_coarse, float lambda_fine,
                                 int precision, int64_t ray_chunk, float* const* outs, float* lr_coarse, float* lr_fine, float* losses,
                                 void* workspace, size_t workspace_bytes, void* stream, const nsr_train_var_losses* var,
                                 float* var_losses);

/* The same training step as a FORWARD / BACKWARD pair, for a loss the caller writes (torch autograd: nerf_sr_amd/train.py
 * forward_rays_train; the reference's calculate_losses, regularize_patch, --sisr_path / --with_ref terms, gradient clipping).
 * nsr_train_forward is the first half of nsr_train_loss_and_grads: train-mode forward_rays (:280-313) with the same draws,
 * render_flags, precisions, ray strides, `ray_chunk` and 32-point rule, the same kernels and the same outputs bit for bit
 * (outs[0] and outs[4] required, the other six may be NULL); no target, no s2, no loss.  Every argument is checked before
 * anything is enqueued.  It ORs the same NSR_FLAG_* bits into the workspace's sticky status block (nsr_train_status).
 * What the backward needs stays in the caller's `saved` buffer (>= nsr_train_saved_bytes, 256-byte aligned; one per forward
 * call that is still to be differentiated -- the workspace is scratch and may be shared by any number of them): a header with
 * the run's parameters and the network's descriptor (nsr_arch below; the default network's here), the backward weight streams of
 * both networks (NSR_F16X3*), and per ray chunk and network the (rgb, sigma) of every sample point, its depth z, and the forward
 * activations -- the chain kernels' 2-byte panels and sign words (NSR_F16X3*) or the per-layer fp32 matrices (NSR_FP32,
 * NSR_F16X3_GEMM).  The format is one for nsr_train_forward and nsr_train_arch_forward; it is opaque and belongs to the
 * library build that wrote it.  At the bench's training batch (2,048 rays,
 * 64 + 64 samples = 393,216 sample points, one chunk): 2.13 GB under NSR_F16X3 (5.4 KB per sample point; the two weight streams
 * are 6 MB of it), 3.99 GB under NSR_FP32 (10.1 KB per point).
 * nsr_train_saved_bytes: 0 on invalid arguments (R <= 0 included); depends on its arguments only.
 *
 * nsr_train_backward: d(loss)/d(weights) of both networks from the upstream gradients g_outs[8] (DEVICE pointers in the outs
 * order: (R, 3) (R) (R) (R, Nc) coarse, the same with Nc + Ni columns fine; any entry NULL = zero).  The fine pass samples from
 * the DETACHED coarse weights (:302): the coarse `weights` gradient reaches the coarse network only.  g_coarse / g_fine are
 * OVERWRITTEN, chunk by chunk in the fused step's order, so that given the upstream gradient the fused step computes
 * internally the result is bit-identical to nsr_train_loss_and_grads.  R, the sample counts, render_flags, precision and
 * ray_chunk are read back from `saved` (the call waits for the stream to read the header: at the bench's batch the GPU idles
 * ~30 us in front of the backward, and the call cannot be captured into a graph): a buffer that no forward call
 * wrote -- or one that nsr_train_arch_forward wrote for another network than the default -- is NSR_ERR_INVALID_ARG, one smaller
 * than its header says NSR_ERR_WORKSPACE; the workspace must be large enough for that run (nsr_train_workspace_bytes_for).  The weights must be the forward call's (the GEMM path re-reads them).  `saved`
 * is not modified: a second backward of the same forward is allowed and gives the same gradients. */
size_t nsr_train_saved_bytes(int precision, int64_t R, int n_coarse, int n_importance, int64_t ray_chunk);
int nsr_train_forward(const float* const* w_coarse, const float* const* w_fine, const float* rays, int ray_stride, int64_t R,
                      int n_coarse, int n_importance, int render_flags, int lindisp, const float* u_coarse, const float* u_fine,
                      const float* noise_coarse, const float* noise_fine, float noise_std, int precision, int64_t ray_chunk,
                      float* const* outs, void* workspace, size_t workspace_bytes, void* saved, size_t saved_bytes, void* stream);
int nsr_train_backward(const float* const* w_coarse, const float* const* w_fine, const float* const* g_outs,
                       float* const* g_coarse, float* const* g_fine, void* workspace, size_t workspace_bytes,
                       const void* saved, size_t saved_bytes, void* stream);

/* Numerics status of the training step (the reference drops into pdb on NaN colours, nerf_downX_model.py:273-274; a
 * replacement reports instead).  The FIRST 64 BYTES of the workspace are a sticky status block: with NSR_F16X3 every
 * nsr_train_loss_and_grads ORs NSR_FLAG_WEIGHT_RANGE (a weight of the iteration's re-pack is non-finite or |w| >= 1023.75:
 * the split-fp16 stream cannot carry it), NSR_FLAG_INPUT_RANGE / NSR_FLAG_ACTIVATION_RANGE (a raw coordinate or a hidden
 * activation left the fp16 operand range: products degrade to 11 bits) and NSR_FLAG_OUTPUT_NONFINITE into its first word,
 * exactly as the inference entry points do into a packed network's tail (nsr.h).  Nothing is synchronised by the step.
 * nsr_train_status_reset zeroes the block (call it once when the workspace is allocated: the step never clears it);
 * nsr_train_status copies the word to the host (waits for the stream) and optionally clears it.  NSR_FP32 and
 * NSR_F16X3_GEMM raise nothing (the word stays as nsr_train_status_reset left it). */
int nsr_train_status_reset(void* workspace, void* stream);
int nsr_train_status(void* workspace, int clear, unsigned* flags_out, void* stream);

/* torch.optim.Adam (no weight decay, no amsgrad) on the 24 tensors of one network, in place:
 *   m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;
 *   w -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)        (step counts from 1). */
int nsr_adam_step(float* const* w, const float* const* g, float* const* m, float* const* v, int step, float lr,
                  float beta1, float beta2, float eps, void* stream);

/* ---- Training a network of any architecture the reference's flags describe (--D --W --skips --deg_pos --deg_dir --no_dir;
 * models/networks.py:124-169, models/nerf_model.py:53-57).  The entry points above run the default network (8 x 256, skip at
 * layer 4, degrees 10 / 4); the ones below take a descriptor.  There is ONE layer-by-layer network (csrc/nsr_train_gemm.hip), a
 * function of the descriptor: under NSR_FP32 / NSR_F16X3_GEMM the entry points above are the ones below with the descriptor
 * {8, 256, 1u << 4, 10, 4, 0}, bit for bit (the chain precisions exist for that network only, through the entry points above).
 *
 * State tensors: 2 D + 8, in the order of the reference module's state_dict() (nerf_sr_amd.weights.arch_spec):
 *   xyz_encoding_{i+1}.0.weight (W, fan_in) / .bias (W) for i = 0 .. D-1, fan_in = 3 + 6 deg_pos for layer 0,
 *   W + 3 + 6 deg_pos for a skip layer (input cat([pe, h])), W otherwise; xyz_encoding_final (W, W) / (W);
 *   dir_encoding.0 (W / 2, W + 3 + 6 deg_dir) / (W / 2) -- (W / 2, W) under no_dir --; sigma (1, W) / (1); rgb.0 (3, W / 2) / (3)
 *   (dim_rgb is 3: the compositor renders three colours).
 * Limits: 1 <= D <= 16, even W with 2 <= W <= 512, 0 <= deg_pos, deg_dir <= 16 (what nsr_posenc accepts).  A descriptor
 * beyond them (D > 16, W > 512, a degree > 16) is NSR_ERR_UNSUPPORTED; a malformed one (D < 1, W < 2 or odd, a negative
 * degree, a skip bit at 0 or at >= D, no_dir other than 0 / 1, a NULL descriptor) NSR_ERR_INVALID_ARG. */
typedef struct nsr_arch {
  int D, W;
  unsigned skips;      /* bit i (1 <= i < D): layer i sees cat([pe, h]) */
  int deg_pos, deg_dir;
  int no_dir;
} nsr_arch;
#define NSR_ARCH_MAX_D 16
#define NSR_ARCH_MAX_W 512
#define NSR_ARCH_MAX_DEG 16
/* 2 D + 8, or the error code (< 0) of the descriptor */
int nsr_arch_n_tensors(const nsr_arch* arch);
/* elements of state tensor t; 0 on an invalid descriptor or index */
int64_t nsr_arch_tensor_numel(const nsr_arch* arch, int t);
/* Sizes of the workspace and of the saved state of the pair below; they depend on their arguments only.  0 on invalid
 * arguments: a descriptor, precision or sample counts the pair rejects, ray_chunk <= 0 (workspace), R <= 0 or a chunking that
 * breaks the 32-point rule (saved state; the workspace size is a function of ray_chunk alone and does not know R).  Per sample point the saved state keeps, in
 * floats, n_x (Kx + Wp) + (D - n_x) Wp + (Wp + Dp) + Hp + 6 with Kx = r32(3 + 6 deg_pos), Wp = r32(W), Hp = r32(W / 2),
 * Dp = r32(3 + 6 deg_dir) (0 under no_dir), r32 = rounded up to 32, n_x = max(1, number of skips): every trunk layer's
 * output, the encoded position once per skip layer (in front of that layer's input, so cat([pe, h]) is a column range),
 * the colour branch's input [final | dir pe], its hidden layer, (rgb, sigma), the noisy sigma and z. */
size_t nsr_train_arch_workspace_bytes(const nsr_arch* arch, int precision, int64_t ray_chunk, int n_coarse, int n_importance);
size_t nsr_train_arch_saved_bytes(const nsr_arch* arch, int precision, int64_t R, int n_coarse, int n_importance, int64_t ray_chunk);
/* nsr_train_forward / nsr_train_backward for the network `arch` describes: the same arguments with the same meaning
 * (outputs, draws, render_flags with NSR_TRAIN_STOP_GRAD, lindisp, ray strides, ray_chunk, the 32-point rule; all eight
 * upstream gradients, NULL = zero; coarse weights detached for the fine pass; everything checked before anything is
 * enqueued), weight and gradient arrays of nsr_arch_n_tensors DEVICE pointers.  precision: NSR_FP32 or NSR_F16X3_GEMM
 * (forward products split-fp16, every gradient on the fp32 MFMA); the chain precisions are NSR_ERR_UNSUPPORTED.  The saved
 * header records the descriptor: a backward with another descriptor, a buffer no forward wrote or a damaged header is
 * NSR_ERR_INVALID_ARG, a buffer shorter than its header says NSR_ERR_WORKSPACE.  The weights must be the forward call's.
 * Weight matrices must be 16-byte aligned (a trunk layer whose shape needs no padding is the GEMMs' operand where the caller
 * holds it): NSR_ERR_INVALID_ARG otherwise, before anything is enqueued.  The same holds for nsr_train_loss_and_grads[_var],
 * nsr_train_forward and nsr_train_backward under NSR_FP32 / NSR_F16X3_GEMM.
 * Weight gradients are reduced in a fixed order (no atomics): two identical calls give identical bits. */
int nsr_train_arch_forward(const nsr_arch* arch, const float* const* w_coarse, const float* const* w_fine, const float* rays,
                           int ray_stride, int64_t R, int n_coarse, int n_importance, int render_flags, int lindisp,
                           const float* u_coarse, const float* u_fine, const float* noise_coarse, const float* noise_fine,
                           float noise_std, int precision, int64_t ray_chunk, float* const* outs, void* workspace,
                           size_t workspace_bytes, void* saved, size_t saved_bytes, void* stream);
int nsr_train_arch_backward(const nsr_arch* arch, const float* const* w_coarse, const float* const* w_fine,
                            const float* const* g_outs, float* const* g_coarse, float* const* g_fine, void* workspace,
                            size_t workspace_bytes, const void* saved, size_t saved_bytes, void* stream);
/* nsr_adam_step over n tensors of numel[i] elements each (HOST array), the same arithmetic; 1 <= n <= 2 NSR_ARCH_MAX_D + 8. */
int nsr_adam_step_n(int n, const int64_t* numel, float* const* w, const float* const* g, float* const* m, float* const* v,
                    int step, float lr, float beta1, float beta2, float eps, void* stream);

/* ---- Fused inference of a non-default architecture under split-fp16 (csrc/nsr_mlp_arch_f16.hip; opt-in: ops.GenericMLP(fused=True)).
 * ONE launch takes encoded rows x (P, in_xyz + in_dir; in_xyz = 3 + 6 deg_pos, in_dir = 3 + 6 deg_dir) to out (P, 4) = [rgb, sigma],
 * or, under NSR_ARCH_FUSED_SIGMA_ONLY, x (P, >= in_xyz) to out (P, 1) = sigma; no activation leaves the chip between two layers.
 * The arithmetic is nsr_linear_f16x3's, layer by layer (weights pre-split as RNE_f16(64 w) / RNE_f16(64 w - hi), every layer's
 * input split into fp16 (hi, lo), three v_mfma_f32_32x32x16_f16 per product, fp32 accumulation, bias and activation), in another
 * summation order.  A row's output bits depend on that row and the weights only.
 * Supported set -- narrower than the layer-by-layer limits above: 1 <= D <= 8, even W with 2 <= W <= 256, any skip set inside
 * 1 .. D-1, 0 <= deg_pos <= 10, 0 <= deg_dir <= 4, no_dir 0 / 1.  A descriptor beyond it is NSR_ERR_UNSUPPORTED (packed_bytes: 0),
 * a malformed one NSR_ERR_INVALID_ARG (0), both before anything is enqueued.
 *   nsr_arch_fused_pack     splits and re-lays the 2 D + 8 state tensors (DEVICE pointers, state_dict order) once into `packed`
 *                           (nsr_arch_fused_packed_bytes, 16-byte aligned).  A non-finite weight or bias, or |w| >= 1023.75 (2^6 w
 *                           leaves fp16), ORs NSR_FLAG_WEIGHT_RANGE into *status; the blob is written all the same.
 *   nsr_arch_fused_forward  flags: NSR_ARCH_FUSED_SIGMA_ONLY | NSR_ARCH_FUSED_COLOR_NONE (--color_activation none); any other bit
 *                           is NSR_ERR_INVALID_ARG.  ldx / ldo: row strides in floats.  P >= 0, any value (a tail tile forms no
 *                           out-of-range address).  ORs the sticky NSR_FLAG_INPUT_RANGE (a non-finite input or |x| > 65504),
 *                           NSR_FLAG_ACTIVATION_RANGE (a hidden activation >= 65520) and NSR_FLAG_OUTPUT_NONFINITE into *status
 *                           (a DEVICE word the caller owns and clears; NULL: not reported).  `packed` must be what
 *                           nsr_arch_fused_pack wrote for the same descriptor.
 *   nsr_arch_fused_render_rays  the same launch on rays and depths, the encodings computed in the kernel: rays (R, ray_stride),
 *                           stride 8 [o, d, near, far] (the direction that is encoded is d; 16-byte aligned) or 11 (the encoded
 *                           direction in columns 8:11), z (R, n_samples) -> out (R n_samples, ldo) = [rgb, sigma] per sample point
 *                           (sigma alone under NSR_ARCH_FUSED_SIGMA_ONLY).  Point k of ray r is o + z[r, k] d (separate multiply and
 *                           add, as nsr_sample_along_rays writes it); its encodings are nsr_posenc's values, so the output and the
 *                           status bits are those of nsr_arch_fused_forward on the rows cat([posenc(points), posenc(direction)
 *                           repeated]), bit for bit, without those rows ever being written.  Any n_samples >= 1, any R >= 0 (R == 0:
 *                           NSR_OK, nothing enqueued).  NSR_ERR_INVALID_ARG, before anything is enqueued: another flag bit, a stride
 *                           other than 8 or 11, misaligned rays at stride 8, n_samples <= 0, R < 0, a NULL packed / rays / z / out,
 *                           ldo < 4 (< 1 under sigma-only), more than 2^31 - 1 tiles of 128 points.  flags, packed, status: as above. */
#define NSR_ARCH_FUSED_SIGMA_ONLY 1
#define NSR_ARCH_FUSED_COLOR_NONE 2
#define NSR_ARCH_FUSED_MAX_D 8
#define NSR_ARCH_FUSED_MAX_W 256
#define NSR_ARCH_FUSED_MAX_DEG_POS 10
#define NSR_ARCH_FUSED_MAX_DEG_DIR 4
size_t nsr_arch_fused_packed_bytes(const nsr_arch* arch);
int nsr_arch_fused_pack(const nsr_arch* arch, const float* const* w, void* packed, unsigned* status, void* stream);
int nsr_arch_fused_forward(const nsr_arch* arch, const void* packed, const float* x, int64_t ldx, int64_t P, int flags, float* out,
                           int64_t ldo, unsigned* status, void* stream);
int nsr_arch_fused_render_rays(const nsr_arch* arch, const void* packed, const float* rays, int ray_stride, const float* z, int64_t R,
                               int n_samples, int flags, float* out, int64_t ldo, unsigned* status, void* stream);

/* ---- The embedding's options --no_xyz / --no_logscale (models/embedding.py:17-18) on the descriptor routes.  The option word
 * `embed` (NSR_EMBED_NO_XYZ | NSR_EMBED_LINEAR_FREQS, include/nsr.h: nsr_posenc_e, nsr_posenc_freqs) is an extra argument
 * behind the descriptor; struct nsr_arch keeps its layout.  Every entry point above that takes a descriptor IS its `_e` form
 * called with embed = 0: one implementation, the same bits.
 *   Widths.    Under NSR_EMBED_NO_XYZ in_xyz = 6 deg_pos and in_dir = 6 deg_dir everywhere a size derives from the descriptor:
 *              the state tensors (layer 0, the skip layers, dir_encoding), the K padding, workspace, saved state and packed
 *              stream.  nsr_arch_n_tensors does not depend on the word.
 *   Refusals.  NSR_ERR_INVALID_ARG (sizes: 0) before anything is enqueued: an unknown bit; NO_XYZ with deg_pos == 0; NO_XYZ with
 *              deg_dir == 0 unless no_dir -- a layer without input columns, which the reference cannot build either.
 *   Training.  The encoder writes the word's columns, sin / cos (nsr_sincos) of band * x from the table of nsr_posenc_freqs (the
 *              largest band is 2^(deg-1) under both tables).  The saved header records the word next to the descriptor: a
 *              backward with another word is NSR_ERR_INVALID_ARG.  The weight gradients do not differentiate through the encoding;
 *              nsr_train_arch_backward_r below does, for the gradient with respect to the rays.
 *   Fused.     nsr_arch_fused_forward_e takes rows of the narrower widths (what nsr_posenc_e writes).  nsr_arch_fused_render_rays_e
 *              computes them in the kernel by nsr_posenc_e's expression: output and status word are bit-identical to the rows
 *              entry on nsr_posenc_e's rows under every word.  NSR_FLAG_INPUT_RANGE tests the columns the network sees: under
 *              NO_XYZ a large raw coordinate is not one of them. */
#ifndef NSR_EMBED_NO_XYZ
#define NSR_EMBED_NO_XYZ 1u       /* --no_xyz */
#define NSR_EMBED_LINEAR_FREQS 2u /* --no_logscale */
#endif
int64_t nsr_arch_tensor_numel_e(const nsr_arch* arch, unsigned embed, int t);
size_t nsr_train_arch_workspace_bytes_e(const nsr_arch* arch, unsigned embed, int precision, int64_t ray_chunk, int n_coarse,
                                        int n_importance);
size_t nsr_train_arch_saved_bytes_e(const nsr_arch* arch, unsigned embed, int precision, int64_t R, int n_coarse, int n_importance,
                                    int64_t ray_chunk);
int nsr_train_arch_forward_e(const nsr_arch* arch, unsigned embed, const float* const* w_coarse, const float* const* w_fine,
                             const float* rays, int ray_stride, int64_t R, int n_coarse, int n_importance, int render_flags,
                             int lindisp, const float* u_coarse, const float* u_fine, const float* noise_coarse,
                             const float* noise_fine, float noise_std, int precision, int64_t ray_chunk, float* const* outs,
                             void* workspace, size_t workspace_bytes, void* saved, size_t saved_bytes, void* stream);
int nsr_train_arch_backward_e(const nsr_arch* arch, unsigned embed, const float* const* w_coarse, const float* const* w_fine,
                              const float* const* g_outs, float* const* g_coarse, float* const* g_fine, void* workspace,
                              size_t workspace_bytes, const void* saved, size_t saved_bytes, void* stream);
size_t nsr_arch_fused_packed_bytes_e(const nsr_arch* arch, unsigned embed);
int nsr_arch_fused_pack_e(const nsr_arch* arch, unsigned embed, const float* const* w, void* packed, unsigned* status, void* stream);
int nsr_arch_fused_forward_e(const nsr_arch* arch, unsigned embed, const void* packed, const float* x, int64_t ldx, int64_t P,
                             int flags, float* out, int64_t ldo, unsigned* status, void* stream);
int nsr_arch_fused_render_rays_e(const nsr_arch* arch, unsigned embed, const void* packed, const float* rays, int ray_stride,
                                 const float* z, int64_t R, int n_samples, int flags, float* out, int64_t ldo, unsigned* status,
                                 void* stream);

/* ---- The gradient with respect to the RAYS on the layer-by-layer pair (pose refinement, anything that produces rays).
 * nsr_train_arch_backward_r with g_rays == NULL IS nsr_train_arch_backward_e: the same launches, the same bits, the same
 * workspace.  With g_rays (R, g_ray_stride) it also OVERWRITES that matrix with d(loss) / d(rays) of the forward call's rays:
 *   a sample point is x = o + z d; the encoded direction is v = d at stride 8, columns 8:11 at stride 11.  As in the reference
 *   (models/nerf_downX_model.py:280-313) the depths z do not depend on o or d: the fine depths come from the DETACHED coarse
 *   weights and from near / far only.
 *   g_x[p]  = the positional encoding's backward at point p, from the gradients of the encoded columns of layer 0 and of every
 *             skip layer: identity columns pass through (none under NSR_EMBED_NO_XYZ), band f contributes
 *             f (cos(f x) g_sin - sin(f x) g_cos) with the sin / cos the forward saved and f of nsr_posenc_freqs' table;
 *   columns 0:3 = sum_k g_x[r, k];   columns 3:6 = sum_k z[r, k] g_x[r, k], plus at stride 8 the direction encoding's backward of
 *   sum_k g_dirpe[r, k]; at stride 11 that term goes to columns 8:11.  No direction term under no_dir, and none under
 *   NSR_TRAIN_STOP_GRAD (dir_encoding's whole input is detached, models/networks.py:218-219).  Coarse part first, fine part added.
 *   Columns 6:8 (near, far) get EXACT ZEROS: the gradient with respect to near / far needs the resampler's backward and is not
 *   computed.
 * Every reduction has a fixed order (no float atomics): a ray's row depends on that ray, its draws and the weights only, and
 * not on ray_chunk; two identical calls give identical bits.  g_ray_stride must be the forward call's ray stride (the saved
 * header records it); a mismatch, or a saved state of a chain precision, is NSR_ERR_INVALID_ARG before anything is enqueued
 * (g_rays untouched).  The workspace must hold nsr_train_arch_workspace_bytes_r (>= the _e figure: one (P, r32(in_xyz)) matrix
 * per layer that reads the encoded position, one (P, r32(in_dir)), one (P, 3)), else NSR_ERR_WORKSPACE.  The input gradients
 * onto the encoded columns run on the fp32 MFMA under both precisions, like every other gradient. */
size_t nsr_train_arch_workspace_bytes_r(const nsr_arch* arch, unsigned embed, int precision, int64_t ray_chunk, int n_coarse,
                                        int n_importance);
int nsr_train_arch_backward_r(const nsr_arch* arch, unsigned embed, const float* const* w_coarse, const float* const* w_fine,
                              const float* const* g_outs, float* const* g_coarse, float* const* g_fine, float* g_rays,
                              int g_ray_stride, void* workspace, size_t workspace_bytes, const void* saved, size_t saved_bytes,
                              void* stream);

/* ---- The same gradient on the CHAIN pair (nsr_train_forward / nsr_train_backward under NSR_F16X3 and its _BWD* variants; the
 * default network).  After the backward chain the gradient panels hold the masked pre-activation gradients of trunk layer 1, of
 * the skip layer and of dir_encoding as fp16 `hi` operands; csrc/nsr_train_raygrad_f16.hip multiplies them by the weight columns
 * of the encoded position / direction (split fp16: W_hi g + W_lo g on v_mfma_f32_32x32x16_f16, fp32 accumulation, the point's
 * power of two applied once per panel), runs the encodings' backward in registers on sin / cos RECOMPUTED from `rays` and the
 * saved depths by the forward's own expression, and sums per ray in double: the row layout, the exact zeros of columns 6:8, the
 * stop_grad rule, "coarse part first, fine part added" and the fixed reduction order are those of nsr_train_arch_backward_r above.
 *   nsr_train_backward_r with g_rays == NULL and flags == 0 IS nsr_train_backward: the same launches, the same bits, the
 *   workspace need of nsr_train_workspace_bytes_for (whatever the saved state's precision).
 *   With g_rays (R, g_ray_stride) it also OVERWRITES that matrix.  `rays` must be the forward call's rays, as the weights must be
 *   its weights; ray_stride and g_ray_stride must both equal the stride in the saved header, else NSR_ERR_INVALID_ARG.  The
 *   workspace must hold nsr_train_workspace_bytes_r (>= the _for figure: two (P, 3) matrices and 144 KiB of packed weight
 *   columns per network), else NSR_ERR_WORKSPACE.  Both are returned before anything is enqueued.
 *   A saved state of NSR_FP32 / NSR_F16X3_GEMM, or of a non-default descriptor, with g_rays or a flag is NSR_ERR_UNSUPPORTED:
 *   those have nsr_train_arch_backward_r.
 *   NSR_BACKWARD_NO_WEIGHT_GRADS (a frozen field): the weight-gradient launch and its finishing launches are not enqueued;
 *   g_coarse / g_fine may be NULL and are not touched; everything else, g_rays included, has the same bits.  The flag without
 *   g_rays is NSR_ERR_INVALID_ARG (nothing to compute), as is any other bit.
 * The saved-state format and nsr_train_saved_bytes are unchanged; the workspace stays pure scratch behind its status block. */
#define NSR_BACKWARD_NO_WEIGHT_GRADS 1u
size_t nsr_train_workspace_bytes_r(int precision, int64_t ray_chunk, int n_coarse, int n_importance);
int nsr_train_backward_r(const float* const* w_coarse, const float* const* w_fine, const float* rays, int ray_stride,
                         const float* const* g_outs, float* const* g_coarse, float* const* g_fine, float* g_rays, int g_ray_stride,
                         unsigned flags, void* workspace, size_t workspace_bytes, const void* saved, size_t saved_bytes, void* stream);

/* One nn.Linear (+ activation) on the training GEMM, exposed for testing the kernel on its own:
 *   y (P, N) = act(x (P, K) · w (N, K)^T + b),  act: 0 none, 1 relu, 2 sigmoid;  y_t (N, P) optional transpose.
 * K % 32 == 0, ldx % 4 == 0, ldw % 4 == 0, 16-byte aligned pointers (the training step pads its operands). */
int nsr_linear(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* b, int act, float* y,
               int64_t ldy, float* y_t, int64_t ldyt, int64_t P, int K, int N, void* stream);

/* The same nn.Linear on the split-fp16 MFMA (round 6: what a NON-default network architecture runs on layer by layer under
 * precision f16x3, ops.GenericMLP): three v_mfma_f32_32x32x16_f16 per product, x split into (hi, lo) fp16 halves on its way
 * to LDS, the weights pre-split ONCE by nsr_split_weights -- w_hi / w_lo (n halves each) = RNE_f16(64 w) and RNE_f16(64 w - hi);
 * the factor is undone in the epilogue -- products exact to ~2^-21, fp32 accumulation, fp32 in and out.  Same shape rules as
 * nsr_linear (K % 32 == 0, ldx % 4 == 0) plus ldw % 8 == 0 and 16-byte aligned w_hi / w_lo; no transposed output. */
int nsr_split_weights(const float* w, int64_t n, void* w_hi, void* w_lo, void* stream);
int nsr_linear_f16x3(const float* x, int64_t ldx, const void* w_hi, const void* w_lo, int64_t ldw, const float* b, int act,
                     float* y, int64_t ldy, int64_t P, int K, int N, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NSR_TRAIN_H_ */
