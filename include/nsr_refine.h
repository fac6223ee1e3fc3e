/* nsr_refine.h — C ABI of the refinement network's forward pass.
 *
 * Replaces MaxPoolingModel.forward(x_synth, list_x_candi) in eval mode (models/networks.py:735-990: the
 * Model_VNPCAT encoder on the synthesised patch and on each of its R reference patches, a max over the references
 * at every scale, the Model_VNPCAT decoder), as refine_model.py:99 calls it (`self.netRefine(sr_patch, ref_patches)`).
 * fp32 in / fp32 out; every 3x3 convolution runs as a GEMM (NSR_FP32: im2col + the fp32-MFMA GEMM of the training step,
 * nsr_gemm.hip; NSR_F16X3: the split-fp16 GEMM with implicit im2col on pre-split fp16 (hi, lo) activation planes) with
 * bias / ReLU / tanh in its epilogue; BatchNorm (eval: running statistics, eps 1e-5) is folded into the packed
 * weights; activations are NHWC so that channel concatenations and nearest-neighbour upsampling cost nothing
 * (GEMM outputs land directly in the concatenated buffers, the upsampling is an index map of the next im2col).
 *
 * Weights: the float tensors of MaxPoolingModel.state_dict() in state_dict order WITHOUT the 17 int64
 * `num_batches_tracked` entries: per layer weight (Cout, Cin, 3, 3), bias (Cout) and, for layers followed by a
 * BatchNorm2d, its weight, bias, running_mean, running_var.  Layer order (NSR_REFINE_N_LAYERS = 19):
 *   E.conv1 (no BN), E.conv2 .. E.conv7, D.conv1, D.conv2, D.conv2_up, D.conv3, D.conv4, D.conv4_up, D.conv5, D.conv6,
 *   D.conv6_up, D.conv7, D.conv8, D.conv9 (no BN)        ->  NSR_REFINE_N_TENSORS = 2 * 19 + 4 * 17 = 106.
 */
#ifndef NSR_REFINE_H_
#define NSR_REFINE_H_

#include "nsr.h"

#define NSR_REFINE_N_LAYERS 19
#define NSR_REFINE_N_TENSORS 106

#ifdef __cplusplus
extern "C" {
#endif

/* precision: NSR_FP32 (explicit im2col + fp32-MFMA GEMM) or NSR_F16X3 (split-fp16 MFMA, products exact to ~2^-21, with
 * implicit im2col: no col matrix is materialised); 0 / NSR_ERR_UNSUPPORTED for anything else.
 * The blob holds, per layer, the folded weights (row-major, K = tap-major), the folded bias and -- for the layers the
 * LDS-patch convolution kernel can take -- a second, fragment-ordered copy of the weights; its size is
 * whatever this function returns, the layout is private to the library.
 * Non-finite values travel as in torch: ReLU keeps NaN, the max over the reference patches propagates it, tanh(NaN) = NaN --
 * a NaN input pixel comes out as NaN over its receptive field, nothing is masked (there is no status word on this path). */
size_t nsr_refine_packed_bytes(int precision);
/* tensors: HOST array of NSR_REFINE_N_TENSORS DEVICE pointers (order above); packed: DEVICE, 16-byte aligned */
int nsr_refine_pack_weights(const float* const* tensors, void* packed, int precision, void* stream);

/* H and W multiples of 8 (three stride-2 levels); 0 on invalid arguments.  The plain form is the NSR_FP32 size (the larger
 * one: that mode materialises im2col matrices); `_for` gives the size a precision actually needs (NSR_F16X3: activations
 * + 128 bytes per input pixel for the first layer -- its input staged as pre-split 16-channel planes when the patch is whole
 * 16 x 16 blocks, a 32-column im2col matrix otherwise --, ~21 MB per 64 x 64 patch set with 8 references).
 * The workspace is scratch: its contents on entry do not matter and are unspecified on return (one buffer may serve calls of
 * any shapes and precisions, one at a time per stream); a size depends on the function's arguments only. */
size_t nsr_refine_workspace_bytes(int B, int R, int H, int W);
size_t nsr_refine_workspace_bytes_for(int precision, int B, int R, int H, int W);
/* x_synth (B, 3, H, W), x_candi (B, R, 3, H, W), out (B, 3, H, W): NCHW fp32 DEVICE (the reference's tensors) */
int nsr_refine_forward(const void* packed, int precision, const float* x_synth, const float* x_candi, int B, int R, int H,
                       int W, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- `--not_use_ref` (MaxPoolingModel with Model_VNPCAT_Decoder_NoPooling, networks.py:866-945, 958-969): the encoder
 * runs on the synthesised patch only and the decoder's concatenations carry no F_max_i channels, i.e. D.conv1, D.conv3,
 * D.conv5, D.conv7 have 512 / 1024 / 512 / 256 input channels.  Same 106 tensors in the same order (four of them with
 * those shapes), its own packed blob; workspace: nsr_refine_workspace_bytes_for(precision, B, 1, H, W). */
size_t nsr_refine_packed_bytes_noref(int precision);
int nsr_refine_pack_weights_noref(const float* const* tensors, void* packed, int precision, void* stream);
int nsr_refine_forward_noref(const void* packed, int precision, const float* x_synth, int B, int H, int W, float* out,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ---- training (MaxPoolingModel in .train(), models/refine_model.py:84-175): fp32 forward / backward pair over the
 * RAW (unfolded) tensors, with the reference patches (--not_use_ref is not trainable here).  BatchNorm2d normalises with
 * the batch statistics of the call (biased variance, eps 1e-5); the encoder runs on the B synthesised and on the B R
 * reference patches with the same weights, each call on ITS OWN statistics, its weight gradients are the sum over both.
 * Parameters (NSR_REFINE_N_PARAMS = 72): per layer weight, bias and, with a BatchNorm, its weight, bias -- the order
 * above without the running statistics.  `running`: HOST array of the 34 running_mean / running_var DEVICE pointers in
 * layer order, updated in place with `momentum` (running_var from the UNBIASED variance; the encoder's twice per
 * forward: synthesised call, then reference call), or NULL to leave them alone.
 * The 17 convolution biases in front of a BatchNorm are cancelled by its mean subtraction: their gradients are DEFINED
 * as exact zeros and not computed (the reference's fp32 autograd leaves ~1e-7 of rounding noise there).
 * Shapes: H, W multiples of 8 (NSR_ERR_UNSUPPORTED otherwise), B >= 1, 1 <= R <= 255, B H W / 64 >= 2 (a BatchNorm needs
 * two values per channel; NSR_ERR_INVALID_ARG).  `img_chunk`: images whose im2col matrix is live at once (<= 0: the
 * library picks, at most 1 GiB); it bounds the workspace, never the batch statistics, and the outputs do not depend on
 * it bit for bit (the weight gradients' summation order does).
 * `saved` (256-byte aligned) carries the run from the forward to its backward: a header (magic, B, R, H, W, img_chunk),
 * the inputs, at most the pre-activation and the output of every layer, the per-layer mean / 1 / std and the winner
 * indices of the four maxima: (787 R + 2398) H W floats + 232 H W bytes per patch set -- 143 MB for R = 8 at 64 x 64.
 * The backward does not modify it: a second backward gives the same bits.  A buffer no forward wrote is
 * NSR_ERR_INVALID_ARG, one shorter than its header says NSR_ERR_WORKSPACE.  The backward reads the header back (it waits
 * for the stream); everything is validated before anything is enqueued.  Every reduction runs in a fixed order without
 * float atomics: identical calls give identical bits.  No gradient with respect to the images; no status word
 * (non-finite values travel as in torch).
 * `workspace` (256-byte aligned) is scratch in both calls: its contents on entry do not matter and are unspecified on return,
 * nothing travels in it from a forward to its backward (one buffer may serve any number of pending forwards, of any shapes);
 * `saved` need not be initialised before the forward. */
#define NSR_REFINE_N_PARAMS 72
size_t nsr_refine_train_workspace_bytes(int B, int R, int H, int W, int img_chunk);
size_t nsr_refine_train_saved_bytes(int B, int R, int H, int W);
/* tensors: the NSR_REFINE_N_TENSORS of nsr_refine_pack_weights, raw; x_synth (B, 3, H, W), x_candi (B, R, 3, H, W),
 * out (B, 3, H, W) */
int nsr_refine_train_forward(const float* const* tensors, float* const* running, float momentum, const float* x_synth,
                             const float* x_candi, int B, int R, int H, int W, int img_chunk, float* out, void* workspace,
                             size_t workspace_bytes, void* saved, size_t saved_bytes, void* stream);
/* g_out (B, 3, H, W) = dL/d out; grads: HOST array of NSR_REFINE_N_PARAMS DEVICE pointers, OVERWRITTEN */
int nsr_refine_train_backward(const float* const* tensors, const float* g_out, float* const* grads, void* workspace,
                              size_t workspace_bytes, const void* saved, size_t saved_bytes, void* stream);

/* The same pair with the arithmetic of the convolutions as an argument.  precision = NSR_FP32: the pair above, bit for bit (the
 * two entry points above are calls of these).  precision = NSR_F16X3 ("f16x3_mixed" in the Python layer): the forward
 * convolutions of layers 1 .. 18 and the input gradients of the stride-1 layers (with and without the x2 upsample) run on the
 * split-fp16 MFMA (three terms per product, products exact to ~2^-21, fp32 accumulation) and gather the 3 x 3 window on the
 * fly -- no im2col, split-K or dcol matrix; E.conv1's forward (K = 32), the stride-2 layers' input gradients, BatchNorm, the
 * max over the references, the per-channel gradients and ALL weight gradients stay fp32 as above.  Any other value is
 * NSR_ERR_UNSUPPORTED, returned before anything else is looked at.
 * The saved state and the two size queries do not depend on the precision: a backward of either precision runs on the
 * saved state of a forward of either (the header records the forward's, nothing requires it to match).  At NSR_F16X3 the
 * outputs do not depend on img_chunk bit for bit either, and identical calls give identical bits: the range of the gradient
 * operand is tracked with an integer maximum, not a float atomic. */
int nsr_refine_train_forward_p(int precision, const float* const* tensors, float* const* running, float momentum,
                               const float* x_synth, const float* x_candi, int B, int R, int H, int W, int img_chunk, float* out,
                               void* workspace, size_t workspace_bytes, void* saved, size_t saved_bytes, void* stream);
int nsr_refine_train_backward_p(int precision, const float* const* tensors, const float* g_out, float* const* grads,
                                void* workspace, size_t workspace_bytes, const void* saved, size_t saved_bytes, void* stream);
/* The backward with the route of the WEIGHT gradients as a second, independent argument.  weight_grad = NSR_FP32: im2col + the
 * fp32-MFMA GEMM, split-K -- nsr_refine_train_backward_p, bit for bit (which is this call with NSR_FP32).  weight_grad =
 * NSR_F16X3 ("f16x3" in the Python layer): the weight gradient of every layer but E.conv1 (cin 3, K = 27: fp32 as before) is
 * one implicit GEMM per site on the split-fp16 MFMA -- dZ and the gathered input both split to fp16 (hi, lo) while they are
 * staged, three terms per product, fp32 accumulation, dZ scaled by a power of two from its tracked range; no col matrix.  The
 * pixels of a site are cut into slices whose length is a function of the layer's shape alone and whose partial sums are added
 * in slice order: no float atomics, identical calls give identical bits, and these weight gradients do not depend on
 * img_chunk.  A power of two applied to g_out comes out of every gradient exactly.  Every other output (gamma, beta, biases,
 * E.conv1's weight, the input gradients the backward passes on) is what `precision` alone makes it.  Any other weight_grad is
 * NSR_ERR_UNSUPPORTED, returned before anything else -- `precision` included -- is looked at; everything else is validated as in
 * nsr_refine_train_backward_p.  The workspace and saved-state sizes do not depend on it. */
int nsr_refine_train_backward_w(int precision, int weight_grad, const float* const* tensors, const float* g_out, float* const* grads,
                                void* workspace, size_t workspace_bytes, const void* saved, size_t saved_bytes, void* stream);

/* ---- patch tiler / stitcher around the network (the 'test' path of data/llff_refine_dataset.py:303-340 and
 * models/refine_model.py:205-216): an SR image is cut into `patch` x `patch` tiles on a grid (x outer, y inner, starts
 * clamped to size - patch); each tile gets `n_ref` reference patches whose top-left corners are the first `n_ref`
 * in-image warp targets locs[y][x] (nsr_depth_warp / `{i}_locs.npz`) of the tile's pixels scanned x outer / y inner,
 * clamped likewise; missing ones are the SR tile itself (ref start -1); predictions are pasted back in tile order.
 * n = ceil(W / patch) * ceil(H / patch) tiles.  All pointers DEVICE. */
int nsr_refine_tile(const double* locs, int H, int W, int patch, int n_ref, int* starts, int* ref_starts, void* stream);
int nsr_refine_gather(const float* sr_img, const float* ref_img, int H, int W, int patch, int n_ref, const int* starts,
                      const int* ref_starts, int n, float* sr_patch, float* ref_patches, void* stream);
int nsr_refine_stitch(const float* patches, const int* starts, int n, int patch, int H, int W, float* image, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NSR_REFINE_H_ */
