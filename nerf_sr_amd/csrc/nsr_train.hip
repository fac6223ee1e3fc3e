// Training step through the render path: include/nsr_train.h.
//
// Replaces NeRFDownXModel.optimize_parameters (models/nerf_downX_model.py:398-408): train-mode forward_rays
// (:280-313), the s^2 means (:326-348), the two MSE losses (:355-362), autograd's backward through the
// compositing and both MLPs, and torch.optim.Adam (:201-204).
//
// A call is a loop over (chunk of rays, network) passes, each with a forward half (pass_forward: sampling, the network,
// density noise, compositing) and a backward half (pass_backward: compositing backward, input and weight gradients).
// nsr_train_loss_and_grads runs the two halves of a pass back to back with the loss kernels in between, on the buffers of
// the workspace (Work, nsr_train_work.h).  nsr_train_forward / nsr_train_backward run them in two calls: what a backward
// half reads (Kept) then lies per pass in the caller's `saved` buffer.  The three drivers share their opening (check_args,
// open_work) and the loop (for_each_pass).
//
// The network itself has two implementations, selected by the precision argument:
//   CHAIN path (NSR_F16X3 and its _BWD* variants; the default network only): the network is a per-point chain.  Its forward
//   pass is the inference kernel (nsr_mlp_f16.hip, TRAIN) that additionally keeps every layer's activation as the fp16 operand
//   it makes anyway; the input gradients are one launch of the backward chain (nsr_train_chain.hip), which keeps its fp16
//   operands likewise.  Both write 2-byte "panels" in 1 KiB units (nsr_f16x3_core.h) that the weight gradients are computed
//   from (nsr_train_wgrad.hip, chain_weight_grads).
//   LAYER-BY-LAYER network (NSR_FP32, NSR_F16X3_GEMM, NSR_F16X3_GEMM_BWD): nsr_train_gemm.hip, a function of an architecture descriptor.
// and two families of entry points over the SAME drivers: nsr_train_* run the default network (the descriptor
// {8, 256, skips {4}, 10, 4, 0} on the layer-by-layer precisions), nsr_train_arch_* the network of the caller's descriptor
// (layer-by-layer precisions only).  One saved-state header and layout serves both; it records the descriptor.
// Per-ray stages (sampling, compositing, resampling) are the inference kernels (nsr_rays.hip / nsr_render.hip); the
// compositing backward is a one-wave-per-ray kernel like its forward.  The kernels both paths use, and Adam, are here.
#include <initializer_list>
#include "nsr_train_chain.h"
#include "nsr_train_work.h"
#include "../../include/nsr_train.h"

using namespace nsr;

namespace {

// N1: sigma + noise * std (models/utils.py:199-212); noise == nullptr copies
__global__ void sigma_noise_kernel(const float* __restrict__ sigma, int sigma_stride, const float* __restrict__ noise,
                                   float std_, int64_t P, float* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const float s = sigma[p * sigma_stride];
  out[p] = noise ? __fadd_rn(s, __fmul_rn(noise[p], std_)) : s;
}

// A1 + MSE: one thread per LR pixel.  lr = mean over the s2 sub-rays; loss partial per block; gC = dL/d(comp rgb)
// of every sub-ray = 2 lambda (lr - target) / (3 N_lr_total) / s2.
// Optional variance losses of the same function (comp_low_res_output, models/nerf_downX_model.py:332-336, 349-353; added to
// loss_tot at :374-378): lambda_var * SUM over the LR pixels and channels of torch.var (unbiased: / (s2 - 1)) of the s2 sub-ray
// colours, and lambda_dvar * SUM over the LR pixels of torch.var of the s2 sub-ray depths / far.  Their gradients join gC
// (2 lambda_var (x_k - mean) / (s2 - 1)) and form a per-ray depth gradient g_depth (2 lambda_dvar (d_k / far - mean) /
// ((s2 - 1) far)) that the compositing backward adds through depth = sum_k w_k z_k.
// block_sums: [0, nblk) squared errors, [nblk, 2 nblk) colour variances, [2 nblk, 3 nblk) depth variances.
__global__ void __launch_bounds__(256) lr_loss_kernel(const float* __restrict__ comp, const float* __restrict__ target,
                                                      int64_t n_lr, int s2, double scale, float lambda,
                                                      float* __restrict__ lr_out, float* __restrict__ g_comp,
                                                      double* __restrict__ block_sums, float lambda_var, float lambda_dvar,
                                                      float far, const float* __restrict__ depth, float* __restrict__ g_depth) {
  __shared__ double red[3][256];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double sq = 0.0, var_rgb = 0.0, var_d = 0.0;
  if (i < n_lr) {
    for (int c = 0; c < 3; ++c) {
      float acc = 0.0f;
      for (int k = 0; k < s2; ++k) acc = __fadd_rn(acc, comp[(i * s2 + k) * 3 + c]);
      const float lr = __fdiv_rn(acc, (float)s2);
      lr_out[i * 3 + c] = lr;
      const float d = __fsub_rn(lr, target[i * 3 + c]);
      sq += (double)d * (double)d;
      const float gc = (float)(2.0 * (double)lambda * (double)d * scale / (double)s2);
      if (lambda_var != 0.0f) {       // wave-uniform
        double ss = 0.0;
        for (int k = 0; k < s2; ++k) {
          const double e = (double)comp[(i * s2 + k) * 3 + c] - (double)lr;
          ss += e * e;
          g_comp[(i * s2 + k) * 3 + c] = gc + (float)(2.0 * (double)lambda_var * e / (double)(s2 - 1));
        }
        var_rgb += ss / (double)(s2 - 1);
      } else {
        for (int k = 0; k < s2; ++k) g_comp[(i * s2 + k) * 3 + c] = gc;
      }
    }
    if (g_depth) {
      if (lambda_dvar != 0.0f) {
        double m = 0.0;
        for (int k = 0; k < s2; ++k) m += (double)__fdiv_rn(depth[i * s2 + k], far);
        m /= (double)s2;
        double ss = 0.0;
        for (int k = 0; k < s2; ++k) {
          const double e = (double)__fdiv_rn(depth[i * s2 + k], far) - m;
          ss += e * e;
          g_depth[i * s2 + k] = (float)(2.0 * (double)lambda_dvar * e / ((double)(s2 - 1) * (double)far));
        }
        var_d = ss / (double)(s2 - 1);
      } else {
        for (int k = 0; k < s2; ++k) g_depth[i * s2 + k] = 0.0f;
      }
    }
  }
  red[0][threadIdx.x] = sq;
  red[1][threadIdx.x] = var_rgb;
  red[2][threadIdx.x] = var_d;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int q = 0; q < 3; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x < 3) block_sums[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = red[threadIdx.x][0];
}
// losses[slot] = lambda * scale * (sum of squared errors over the passes so far)   (single thread block: deterministic order);
// var_losses (optional): [slot] = lambda_var * sum of the colour variances, [2 + slot] = lambda_dvar * sum of the depth variances
__global__ void __launch_bounds__(256) loss_finish_kernel(const double* __restrict__ block_sums, int n, double scale,
                                                          float lambda, float* __restrict__ losses, int slot,
                                                          double* __restrict__ carry, float lambda_var, float lambda_dvar,
                                                          float* __restrict__ var_losses) {
  __shared__ double red[3][256];
  for (int q = 0; q < 3; ++q) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += block_sums[(int64_t)q * n + i];
    red[q][threadIdx.x] = s;
  }
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int q = 0; q < 3; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    carry[slot] += red[0][0];                                       // sum of squared errors over the passes so far
    losses[slot] = (float)((double)lambda * carry[slot] * scale);   // scale = 1 / (3 N_lr)
    carry[2 + slot] += red[1][0];
    carry[4 + slot] += red[2][0];
    if (var_losses) {
      var_losses[slot] = (float)((double)lambda_var * carry[2 + slot]);
      var_losses[2 + slot] = (float)((double)lambda_dvar * carry[4 + slot]);
    }
  }
}

// --gamma_correct while training: the per-sample colours of a pass (rgb4: (P, 4), columns 0..2) become pow(rgb, 1 / 2.2)
__global__ void __launch_bounds__(256) gamma_points_kernel(float* __restrict__ rgb4, int64_t P) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  float4 v = reinterpret_cast<float4*>(rgb4)[p];
  v.x = nsr_gamma(v.x); v.y = nsr_gamma(v.y); v.z = nsr_gamma(v.z);
  reinterpret_cast<float4*>(rgb4)[p] = v;
}
// g d(colour) / d(pre-activation) of the colour head from the colour y it produced: the slope is y (1 - y) for the sigmoid
// and y (1 - y^2.2) / 2.2 for the gamma-corrected sigmoid y = s^(1 / 2.2).  (The plain form keeps rounds 2-4's operation
// order, (g y) (1 - y): training trajectories are compared bit for bit across builds.)
// head: 0 = sigmoid, 1 = gamma-corrected sigmoid, 2 = none (--color_activation none: slope 1)
__device__ __forceinline__ float colour_head_bwd(float g, float y, int head) {
  if (head == 2) return g;
  return head == 1 ? g * y * (1.0f - powf(y, 2.2f)) * (1.0f / 2.2f) : g * y * (1.0f - y);
}

// Backward of V1 (models/rendering.py:75-111) w.r.t. the point colours and densities, given dL/d(comp rgb).
//   w_k = alpha_k T_k, T_k = prod_{j<k} f_j, f_j = 1 - alpha_j + 1e-10, alpha_k = 1 - exp(-delta_k relu(sigma_k))
//   gw_k = gC . rgb_k (- sum(gC) with a white background: comp += 1 - sum_k w_k) (+ g_depth z_k: depth = sum_k w_k z_k, when a
//   depth-variance loss is on)
//   dL/dalpha_k = gw_k T_k - (sum_{i>k} gw_i w_i) / f_k
//   dL/dsigma_k = dL/dalpha_k * delta_k exp(-delta_k relu(sigma_k)) * [sigma_k > 0];   dL/drgb_k = gC w_k
// and through the sigmoid of the colour head: d(rgb_pre) = d(rgb) * rgb (1 - rgb); under --gamma_correct the colours held
// are y = s^(1/2.2), s = sigmoid(pre), and dy/d(pre) = s^(1/2.2 - 1) s (1 - s) / 2.2 = y (1 - y^2.2) / 2.2.
// `white`: the training entry points' option word (include/nsr_train.h).  NSR_SIGMA_SOFTPLUS: density log(1 + exp(sigma - 1)),
// whose slope sigmoid(sigma - 1) replaces [sigma > 0]; NSR_TRAIN_COLOR_NONE: no colour activation, slope 1.
// Output: one float4 per point, d4[p] = (d_rgb_pre 0..2, d_sigma).  gmax (may be null): the backward chain's ten gmax words,
// cleared here.  bias_part (may be null): per ray, the sums of the four values over its points.
// FULL (nsr_train_backward: upstream gradients of every output): gw_k also takes + g_opacity (opacity = sum_k w_k) and
// + g_weights[k]; either pointer may be null.  The fused step's instantiations (FULL = false) do not contain the two terms.
template <int K, bool FULL>
__global__ void __launch_bounds__(256) composite_bwd_kernel(const float* __restrict__ rgb4, const float* __restrict__ sigma,
                                                            const float* __restrict__ z, const float* __restrict__ g_comp,
                                                            int64_t R, int N, int white,
                                                            float* __restrict__ d4, unsigned* __restrict__ gmax,
                                                            const float* __restrict__ g_depth, float* __restrict__ bias_part,
                                                            const float* __restrict__ g_opacity, const float* __restrict__ g_weights) {
  const int lane = threadIdx.x & 63;
  // the chain path's gmax words are cleared here -- the kernel that runs right in front of the chain -- instead of by a memset
  // launch of their own (round 6)
  if (gmax && blockIdx.x == 0 && threadIdx.x < 10) gmax[threadIdx.x] = 0u;
  const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (r >= R) return;
  const int64_t base = r * N;
  const float gc0 = g_comp[r * 3 + 0], gc1 = g_comp[r * 3 + 1], gc2 = g_comp[r * 3 + 2];
  const float gd = g_depth ? g_depth[r] : 0.0f;
  const int head = (white & NSR_TRAIN_GAMMA_CORRECT) ? 1 : ((white & NSR_TRAIN_COLOR_NONE) ? 2 : 0);
  const bool softplus = (white & NSR_SIGMA_SOFTPLUS) != 0;
  float zk[K], sg[K], c0[K], c1[K], c2[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const int k = lane * K + i;
    const int64_t p = base + (k < N ? k : N - 1);
    zk[i] = z[p];
    sg[i] = sigma[p];
    c0[i] = rgb4[p * 4 + 0];
    c1[i] = rgb4[p * 4 + 1];
    c2[i] = rgb4[p * 4 + 2];
  }
  const float z_next_lane = __shfl_down(zk[0], 1, 64);
  float alpha[K], ex[K], dl[K], ff[K];
  double pl[K];
  double run = 1.0;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const int k = lane * K + i;
    const float zn = (i + 1 < K) ? zk[(i + 1 < K) ? i + 1 : i] : z_next_lane;
    const float delta = (k >= N - 1) ? 1e10f : __fsub_rn(zn, zk[i]);
    const float e = expf(__fmul_rn(-delta, softplus ? nsr_softplus_density(sg[i]) : fmaxf(sg[i], 0.0f)));
    float a = __fsub_rn(1.0f, e);
    if (k >= N) a = 0.0f;
    alpha[i] = a;
    ex[i] = e;
    dl[i] = delta;
    const float f = (k < N) ? __fadd_rn(__fsub_rn(1.0f, a), 1e-10f) : 1.0f;
    ff[i] = f;
    run *= (double)f;
    pl[i] = run;
  }
  const double incl = wave_scan_mul_d(run, lane);
  double excl = __shfl_up(incl, 1, 64);
  if (lane == 0) excl = 1.0;
  // weights, gw, and the inclusive prefix of gw_i w_i (suffix = total - prefix)
  float T[K], w[K], gw[K];
  double pre[K];
  double acc = 0.0;
  const float white_term = (white & NSR_WHITE_BKGD) ? __fadd_rn(__fadd_rn(gc0, gc1), gc2) : 0.0f;

#pragma unroll
  for (int i = 0; i < K; ++i) {
    const int k = lane * K + i;
    const double t_d = (i == 0) ? excl : excl * pl[(i > 0) ? i - 1 : 0];
    T[i] = (k == 0) ? 1.0f : (float)t_d;
    w[i] = __fmul_rn(alpha[i], T[i]);
    gw[i] = gc0 * c0[i] + gc1 * c1[i] + gc2 * c2[i] - white_term;
    if (g_depth) gw[i] += gd * zk[i];
    if (FULL) {
      if (g_opacity) gw[i] += g_opacity[r];
      if (g_weights && k < N) gw[i] += g_weights[base + k];
    }
    if (k < N) acc += (double)gw[i] * (double)w[i];
    pre[i] = acc;
  }
  const double lane_incl = wave_scan_add_d(acc, lane);
  const double total = __shfl(lane_incl, 63, 64);
  const double lane_excl = lane_incl - acc;
  float bs0 = 0.0f, bs1 = 0.0f, bs2 = 0.0f, bs3 = 0.0f;     // this ray's sums of the four values = its share of the
                                                            // colour head's and the density head's bias gradients
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const int k = lane * K + i;
    if (k >= N) continue;
    const int64_t p = base + k;
    const double suffix = total - (lane_excl + pre[i]);             // sum_{i' > k} gw w
    const float d_alpha = (float)((double)gw[i] * (double)T[i] - suffix / (double)ff[i]);
    float d_sigma;
    if (softplus) d_sigma = d_alpha * dl[i] * ex[i] * (1.0f / (1.0f + expf(1.0f - sg[i])));      // d log(1 + e^(x - 1)) / dx = sigmoid(x - 1)
    else d_sigma = (sg[i] > 0.0f) ? d_alpha * dl[i] * ex[i] : 0.0f;
    const float dr0 = colour_head_bwd(gc0 * w[i], c0[i], head);
    const float dr1 = colour_head_bwd(gc1 * w[i], c1[i], head);
    const float dr2 = colour_head_bwd(gc2 * w[i], c2[i], head);
    reinterpret_cast<float4*>(d4)[p] = make_float4(dr0, dr1, dr2, d_sigma);
    bs0 += dr0; bs1 += dr1; bs2 += dr2; bs3 += d_sigma;
  }
  if (bias_part) {      // one float4 per ray; finish_jobs_kernel (kind 2) sums the rays in double
    bs0 = wave_sum(bs0); bs1 = wave_sum(bs1); bs2 = wave_sum(bs2); bs3 = wave_sum(bs3);
    if (lane == 0) reinterpret_cast<float4*>(bias_part)[r] = make_float4(bs0, bs1, bs2, bs3);
  }
}

// torch.optim.Adam over n tensors in one launch (adam_update: nsr_train_work.h)
struct AdamN {
  float* w[kMaxT];
  const float* g[kMaxT];
  float* m[kMaxT];
  float* v[kMaxT];
  int64_t n[kMaxT];
};
__global__ void __launch_bounds__(256) adam_n_kernel(AdamN a, float beta1, float beta2, float eps, float step_size, float bc2_sqrt) {
  const int t = blockIdx.y;
  const int64_t n = a.n[t];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    adam_update(a.g[t], a.m[t], a.v[t], a.w[t], i, beta1, beta2, eps, step_size, bc2_sqrt);
}

// ---- host side: carving the workspace ---------------------------------------------------------------------------------
// the kept state of a pass over P sample points (nsr_train_work.h): THE list of its buffers, for the workspace and for a
// pass region of the saved state alike
// net: the layer-by-layer network whose activations are kept (null: none); chain_path: the chain kernels' panels
Kept carve_kept(Carver& a, int64_t P, const Shape* net, bool chain_path) {
  Kept q{};
  if (net) carve_net_kept(a, *net, P, q);
  q.rgb = a.take(P * 4);   q.sig = a.take(P);   q.z = a.take(P);
  q.zpan = reinterpret_cast<char*>(a.take(nsr_f16x3_train_panel_bytes(P) / 4, chain_path));
  q.sgn = reinterpret_cast<unsigned*>(a.take(nsr_f16x3_train_sign_words(P), chain_path));
  return q;
}

// net (+ split: its split-fp16 weight halves) and / or the chain path: the buffers of what may run.  Both
// (nsr_train_workspace_bytes): sufficient whatever runs; the chain path alone holds no per-layer activation / gradient
// matrices (11 KB per sample point less)
// ray_grad: behind everything else (the layout in front of them is the same with and without), the three matrices of the
// gradient with respect to the rays
// bwd (NSR_F16X3_GEMM_BWD): behind the ray-gradient matrices, the transposed split halves of both packs and the range words
int64_t work_floats(int64_t chunk, int nc, int ni, const Shape* net, bool split, bool chain_path, Work* w, float* base,
                    bool ray_grad = false, bool bwd = false) {
  const int64_t nf = nc + ni, P = chunk * nf;
  Carver a{base};
  Work tmp;
  Work& k = w ? *w : tmp;
  k.status = reinterpret_cast<unsigned*>(a.take(16));      // offset 0 whatever the path: nsr_train_status reads it blind
  k.kept = carve_kept(a, P, net, chain_path);
  k.d4 = a.take(P * 4);
  if (net) {
    const Shape& S = *net;
    k.g0 = a.take(P * (S.Wp + 32));   k.g1 = a.take(P * (S.Wp + 32));
    k.drgb = a.take(P * 32);
    k.col_tiles = a.take((P / 128 + 1) * S.Wp + 2 * 64 * S.Wp + 64);   // per-tile column sums + 64 slices of doubles
    k.partial = a.take(kMaxSplits * S.part_stride);                    // also scratch of the small bias sums
    for (int n = 0; n < 2; ++n) k.pack[n] = carve_pack(a, S, split);
  }
  k.z_c = a.take(chunk * nc);   k.w_c = a.take(chunk * nc);
  k.g_comp = a.take(chunk * 3);
  k.scratch_out = a.take(chunk * (nf + 8));
  k.block_sums = reinterpret_cast<double*>(a.take(2 * 3 * (chunk / 256 + 2)));
  k.carry = reinterpret_cast<double*>(a.take(16));
  k.g_depth = a.take(chunk);
  // chain path: every second pass of a network waits for one launch; sized by the split-K factor of the larger pass
  const int64_t sp_max = n_splits(P);
  k.bias_part = a.take(chunk * 4, chain_path);
  k.slots = a.take(kChainSlots * sp_max * 256 * 256, chain_path);
  k.dpan = reinterpret_cast<char*>(a.take(nsr_f16x3_train_panel_bytes(P) / 4, chain_path));
  k.row_part = a.take(kChainRowSlots * sp_max * 256, chain_path);
  k.gmax = reinterpret_cast<unsigned*>(a.take(64, chain_path));
  k.pscale = a.take(10 * ((P + 127) / 128) * 128, chain_path);
  for (int n = 0; n < 2; ++n) {
    k.stream_f[n] = a.take((int64_t)(nsr_f16x3_packed_bytes() / 4), chain_path);
    k.stream_b[n] = a.take((int64_t)(nsr_chain_bwd_packed_bytes() / 4), chain_path);
  }
  const bool rg = ray_grad && net;
  const bool rgc = ray_grad && chain_path && !net;   // nsr_train_backward_r: per point (P, 3) + (P, 3), the packed columns
  k.gpe = a.take(rg ? net->n_pe() * P * net->Kx : 0, rg);
  k.gdir = a.take(rg ? P * net->Dp : P * 3, (rg && net->Dp > 0) || rgc);
  k.gx = a.take(P * 3, rg || rgc);
  for (int n = 0; n < 2; ++n) k.rgw[n] = a.take(kRayGradImageFloats, rgc);
  const bool tail = bwd && net;
  if (tail)
    for (int n = 0; n < 2; ++n) carve_pack_t(a, *net, k.pack[n]);
  k.range = reinterpret_cast<unsigned*>(a.take(kRangeWords, tail));
  return a.off;
}

// which implementation a precision value selects (include/nsr_train.h): the chain kernels or the layer-by-layer GEMMs
bool chain_selected(int precision) {
  return precision == NSR_F16X3 || precision == NSR_F16X3_BWD3 || precision == NSR_F16X3_BWD2 || precision == NSR_F16X3_BWD1 ||
         precision == NSR_F16X3_BWDM;
}
// MFMAs per product of the backward chain (include/nsr_train.h; NSR_F16X3 = the default, kDefaultBwdTerms)
constexpr int kDefaultBwdTerms = 12;   // NSR_F16X3_BWDM
int chain_bwd_terms(int precision) {
  return precision == NSR_F16X3_BWD3 ? 3 : (precision == NSR_F16X3_BWD2 ? 2 : (precision == NSR_F16X3_BWD1 ? 1 : (precision == NSR_F16X3_BWDM ? 12 : kDefaultBwdTerms)));
}
bool bwd_selected(int precision) { return precision == NSR_F16X3_GEMM_BWD; }   // ... and its gradient products split-fp16 too
bool train_precision_ok(int precision) {
  return precision == NSR_FP32 || chain_selected(precision) || precision == NSR_F16X3_GEMM || bwd_selected(precision);
}
// split-fp16 forward products of the layer-by-layer network
bool split_selected(int precision) { return precision == NSR_F16X3_GEMM || bwd_selected(precision); }

using CompositeBwdFn = decltype(&composite_bwd_kernel<1, false>);
template <bool FULL> CompositeBwdFn composite_bwd_for(int K) {   // K: samples per lane
  switch (K) {
    case 1: return composite_bwd_kernel<1, FULL>;
    case 2: return composite_bwd_kernel<2, FULL>;
    case 3: return composite_bwd_kernel<3, FULL>;
    case 4: return composite_bwd_kernel<4, FULL>;
    default: return nullptr;
  }
}

}  // namespace

// ---- the launchers of the kernels above (nsr_train_work.h): what the passes below call, and what the unit tests reach
// through tests/csrc/nsr_test_hooks_heads.hip
namespace nsr {

// (P, 4) rows into d4 from the pass's rgb / sig / z; gmax, bias_part: the chain path's, else null.  g_opacity / g_weights
// (the backward entry points only): non-null selects the FULL instantiation
int composite_bwd(hipStream_t st, const float* rgb, const float* sig, const float* z, const float* g_comp, int64_t R, int N, int white,
                  float* d4, unsigned* gmax, float* bias_part, const float* g_depth, const float* g_opacity, const float* g_weights) {
  const int K = (N + 63) / 64;
  const CompositeBwdFn fn = (g_opacity || g_weights) ? composite_bwd_for<true>(K) : composite_bwd_for<false>(K);
  if (!fn) return NSR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(fn, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, rgb, sig, z, g_comp, R, N, white, d4, gmax, g_depth,
                     bias_part, g_opacity, g_weights);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

int sigma_noise(hipStream_t st, const float* sigma, int sigma_stride, const float* noise, float std_, int64_t P, float* out) {
  hipLaunchKernelGGL(sigma_noise_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, sigma, sigma_stride, noise, std_, P, out);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

int gamma_points(hipStream_t st, float* rgb4, int64_t P) {
  hipLaunchKernelGGL(gamma_points_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, rgb4, P);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

int lr_loss(hipStream_t st, const float* comp, const float* target, int64_t n_lr, int s2, double scale, float lambda, float* lr_out,
            float* g_comp, double* block_sums, float lambda_var, float lambda_dvar, float far, const float* depth, float* g_depth) {
  const int nblk = (int)((n_lr + 255) / 256);
  hipLaunchKernelGGL(lr_loss_kernel, dim3(nblk), dim3(256), 0, st, comp, target, n_lr, s2, scale, lambda, lr_out, g_comp, block_sums,
                     lambda_var, lambda_dvar, far, depth, g_depth);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

int loss_finish(hipStream_t st, const double* block_sums, int n, double scale, float lambda, float* losses, int slot, double* carry,
                float lambda_var, float lambda_dvar, float* var_losses) {
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, st, block_sums, n, scale, lambda, losses, slot, carry, lambda_var,
                     lambda_dvar, var_losses);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

}  // namespace nsr

namespace {

// ---- the opening the drivers share ---------------------------------------------------------------------------------------
// the shape rules: sample counts and precision (NSR_ERR_UNSUPPORTED), R and the chunk multiples of s2
// (NSR_ERR_INVALID_ARG), a multiple of 32 points per pass in both networks (NSR_ERR_UNSUPPORTED).  ray_chunk <= 0 or > R
// becomes R.  gemm_only: the layer-by-layer precisions alone (nsr_train_arch_*)
int check_shape(int64_t R, int s2, int n_coarse, int n_importance, int precision, int64_t& ray_chunk, bool gemm_only) {
  if (n_coarse < 2 || n_importance < 1 || n_coarse + n_importance > 256) return NSR_ERR_UNSUPPORTED;
  if (!train_precision_ok(precision) || (gemm_only && chain_selected(precision))) return NSR_ERR_UNSUPPORTED;
  if (R % s2 != 0) return NSR_ERR_INVALID_ARG;
  if (ray_chunk <= 0 || ray_chunk > R) ray_chunk = R;
  if (ray_chunk % s2 != 0) return NSR_ERR_INVALID_ARG;
  // the split-K weight-gradient GEMM contracts over the chunk's sample points in K tiles of 32: every chunk,
  // the shorter last one included, must hold a multiple of 32 points in both passes -- checked BEFORE anything
  // is enqueued, so a rejected call leaves outputs and gradients untouched
  for (int64_t r0 = 0; r0 < R; r0 += ray_chunk) {
    const int64_t rc = (R - r0 < ray_chunk) ? R - r0 : ray_chunk;
    if ((rc * n_coarse) % 32 != 0 || (rc * (n_coarse + n_importance)) % 32 != 0) return NSR_ERR_UNSUPPORTED;
  }
  return NSR_OK;
}
// the option word (include/nsr_train.h): the renderer's two bits + the colour head's two + stop_grad
constexpr int kTrainOpts = NSR_WHITE_BKGD | NSR_SIGMA_SOFTPLUS | NSR_TRAIN_GAMMA_CORRECT | NSR_TRAIN_COLOR_NONE | NSR_TRAIN_STOP_GRAD;
int check_flags(int flags) {
  if ((flags & ~kTrainOpts) != 0) return NSR_ERR_INVALID_ARG;
  // pow(x, 1 / 2.2) of an unbounded head: NaN for every negative value
  if ((flags & NSR_TRAIN_GAMMA_CORRECT) && (flags & NSR_TRAIN_COLOR_NONE)) return NSR_ERR_UNSUPPORTED;
  return NSR_OK;
}


// Everything that is checked before a call enqueues, in the ONE order that decides which status a call with two mistakes
// returns.  c: shape and options of the call (c->chunk is resolved; s2 = 1 without a loss), or null for the backward, whose
// shape comes out of the saved header afterwards.  NSR_OK with c->R == 0 means: nothing to do, the rest was not looked at.
int check_args(const Need& need, Run* c, int s2) {
  for (const void* p : need.always)
    if (!p) return NSR_ERR_INVALID_ARG;
  if (c) {
    if (c->R < 0 || s2 <= 0 || !nsr_ray_stride_ok(c->ray_stride)) return NSR_ERR_INVALID_ARG;
    NSR_TRY(check_shape(c->R, s2, c->nc, c->ni, c->precision, c->chunk, need.gemm_only));
  }
  for (const float* const* tensors : need.state)
    for (int i = 0; i < need.n_state; ++i)
      if (!tensors[i]) return NSR_ERR_INVALID_ARG;
  if (c && c->R == 0) return NSR_OK;
  if (need.outs && (!need.outs[0] || !need.outs[4])) return NSR_ERR_INVALID_ARG;
  for (const void* p : need.with_rays)
    if (!p) return NSR_ERR_INVALID_ARG;
  for (const void* p : need.aligned)
    if ((reinterpret_cast<uintptr_t>(p) & 255) != 0) return NSR_ERR_INVALID_ARG;
  return c ? check_flags(c->flags) : NSR_OK;
}
// the workspace of a checked call: which implementation runs (c.net: the descriptor's shapes, already made), the weights
// usable where they lie, large enough, then carved.  The nsr_train_* family always sizes the split halves
// (nsr_train_workspace_bytes_for: one size for both layer-by-layer precisions), nsr_train_arch_* sizes by precision
int open_work(Run& c, const float* const* w_coarse, const float* const* w_fine, bool by_precision, void* workspace,
              size_t workspace_bytes, Work& k, bool ray_grad = false) {
  c.chain = chain_selected(c.precision);
  const Shape* net = c.chain ? nullptr : &c.net;
  if (net) {
    NSR_TRY(check_alignment(*net, w_coarse));
    NSR_TRY(check_alignment(*net, w_fine));
  }
  const bool split = !by_precision || split_selected(c.precision);
  const bool bwd = bwd_selected(c.precision);
  if (workspace_bytes < (size_t)work_floats(c.chunk, c.nc, c.ni, net, split, c.chain, nullptr, nullptr, ray_grad, bwd) * sizeof(float))
    return NSR_ERR_WORKSPACE;
  work_floats(c.chunk, c.nc, c.ni, net, split, c.chain, &k, static_cast<float*>(workspace), ray_grad, bwd);
  return NSR_OK;
}

// the weights of both networks in the form the path's kernels read, once per call
// with_backward: the call also runs the backward half (the fused step; nsr_train_forward's launches are the forward's alone)
int prepare_call(hipStream_t st, const Work& k, const float* const* w_coarse, const float* const* w_fine, const Run& c,
                 void* stream, bool with_backward = true) {
  if (c.chain) {
    // the weights are re-packed every iteration: a run whose weights drift beyond what the split-fp16 stream carries
    // (|w| >= 1023.75, or NaN) raises NSR_FLAG_WEIGHT_RANGE in the step's status word, like nsr_pack_weights does.
    // Round 6: both networks per launch (6 launches -> 3), and the backward pack also clears the loss carries and writes
    // word 1 of the status block = the colour-head option word the TRAIN instantiation of the forward kernel reads (the
    // blob tail's layout, nsr_common.h; written every call, so a workspace that was never reset cannot switch an option on)
    NSR_TRY(nsr_check_weights_range2(w_coarse, w_fine, NSR_F16X3, k.status, stream));
    NSR_TRY(nsr_f16x3_pack2(w_coarse, k.stream_f[0], w_fine, k.stream_f[1], stream));
    NSR_TRY(nsr_chain_bwd_pack2(w_coarse, k.stream_b[0], w_fine, k.stream_b[1], (c.flags & NSR_TRAIN_STOP_GRAD) != 0,
                                chain_bwd_terms(c.precision), k.carry, 8, k.status + 1,
                                (c.flags & NSR_TRAIN_COLOR_NONE) ? kOptColorNone : 0u, stream));
  } else {
    NSR_TRY(prepare_weights(st, c.net, w_coarse, k.pack[0], split_selected(c.precision)));
    NSR_TRY(prepare_weights(st, c.net, w_fine, k.pack[1], split_selected(c.precision)));
    if (with_backward && bwd_selected(c.precision)) {
      NSR_TRY(prepare_weights_t(st, c.net, w_coarse, k.pack[0]));
      NSR_TRY(prepare_weights_t(st, c.net, w_fine, k.pack[1]));
    }
    if (hipMemsetAsync(k.carry, 0, 8 * sizeof(double), st) != hipSuccess) return NSR_ERR_LAUNCH;
  }
  return NSR_OK;
}

// ---- the passes of a call ----------------------------------------------------------------------------------------------
// stratified samples (coarse) or inverse-CDF samples from the detached coarse weights w_c over z_c (fine) into z
int pass_sample(const Run& c, const Pass& q, const float* rays, const float* u, const float* z_c, const float* w_c, float* z,
                     void* stream) {
  const float* rays_c = rays + q.r0 * c.ray_stride;
  if (q.net == 0) return nsr_sample_along_rays(rays_c, c.ray_stride, q.rc, c.nc, c.lindisp, rows_of(u, q, c.nc), z, nullptr, stream);
  return nsr_resample_along_rays(rays_c, c.ray_stride, z_c, w_c, q.rc, c.nc, c.ni, rows_of(u, q, c.ni), z, nullptr, stream);
}
// from the raw densities in column 3 of the (P, 4) colours the network left: density noise into sig, --gamma_correct,
// compositing
int pass_finish(hipStream_t st, const Run& c, const Pass& q, const float* noise, float* rgb4, float* sig, const float* z, float* comp,
                float* depth, float* opac, float* wts, void* stream) {
  NSR_TRY(sigma_noise(st, rgb4 + 3, 4, c.noise_std > 0.0f ? rows_of(noise, q, q.N) : nullptr, c.noise_std, q.P, sig));
  if (c.flags & NSR_TRAIN_GAMMA_CORRECT)     // render_rays: out_rgbs = pow(out_rgbs, 1 / 2.2) per sample, in training too (nerf_downX_model.py:271-276)
    NSR_TRY(gamma_points(st, rgb4, q.P));
  return nsr_composite(rgb4, 4, sig, 1, z, q.rc, q.N, c.flags & (NSR_WHITE_BKGD | NSR_SIGMA_SOFTPLUS), comp, depth, opac, wts, stream);
}
// forward half of pass q: sampling into z, the network (what its backward reads stays in k.kept), density noise,
// --gamma_correct, compositing.
// rays / u / noise: the call's whole arrays; w_c / comp / depth / opac / wts: this pass's rows (all but comp may be null)
int pass_forward(hipStream_t st, const Work& k, const Run& c, const Pass& q, const float* const* w, const float* rays,
                 const float* u, const float* noise, const float* z_c, const float* w_c, float* z, float* comp, float* depth,
                 float* opac, float* wts, void* stream) {
  const Kept& s = k.kept;
  const float* rays_c = rays + q.r0 * c.ray_stride;
  NSR_TRY(pass_sample(c, q, rays, u, z_c, w_c, z, stream));
  if (c.chain) {   // the chain path encodes inside its forward kernel
    NSR_TRY(nsr_f16x3_train_forward(k.stream_f[q.net], rays_c, c.ray_stride, z, q.rc, q.N, s.rgb, s.zpan, s.sgn, k.status, stream));
  } else {
    NSR_TRY(net_forward(st, c.net, rays_c, c.ray_stride, z, q.N, w, k.pack[q.net], s, q.P, split_selected(c.precision),
                        (c.flags & NSR_TRAIN_COLOR_NONE) != 0));
  }
  return pass_finish(st, c, q, noise, s.rgb, s.sig, z, comp, depth, opac, wts, stream);
}

// backward half of the same pass, from the upstream gradients of its outputs (this pass's rows; g_comp required, the others
// may be null): compositing backward, then the chain kernels or the layer-by-layer network.  g: the network's gradient
// tensors, overwritten or accumulated (q.acc)
int pass_backward(hipStream_t st, const Work& k, const Run& c, const Pass& q, const float* const* w, const float* z,
                  const float* g_comp, const float* g_depth, const float* g_opacity, const float* g_weights, float* const* g,
                  void* stream, const RayGrad* rg = nullptr, bool weight_grads = true) {
  NSR_TRY(composite_bwd(st, k.kept.rgb, k.kept.sig, z, g_comp, q.rc, q.N, c.flags, k.d4, c.chain ? k.gmax : nullptr,
                        c.chain ? k.bias_part : nullptr, g_depth, g_opacity, g_weights));
  if (c.chain) {
    NSR_TRY(nsr_chain_bwd(k.stream_b[q.net], k.kept.sgn, k.dpan, k.d4, 4, k.d4 + 3, 4, q.P, k.gmax, k.pscale,
                          chain_bwd_terms(c.precision), 1, stream));
    if (rg)   // the panels hold what the ray gradient needs: three products with the columns the chain does not multiply by
      NSR_TRY(raygrad_f16(st, k.rgw[q.net], k.dpan, k.pscale, rg->in, c.ray_stride, rg->z, rg->rays, rg->N,
                          (c.flags & NSR_TRAIN_STOP_GRAD) != 0, k.gx, k.gdir, rg->rows, rg->acc));
    return weight_grads ? chain_weight_grads(st, k, q.P, q.rc, g, q.acc) : NSR_OK;
  }
  return net_backward(st, c.net, w, k.pack[q.net], k, q.P, g, q.acc, (c.flags & NSR_TRAIN_STOP_GRAD) != 0, rg);
}

// ---- saved state of a forward call (include/nsr_train.h) --------------------------------------------------------------
// [header: 256 bytes][chain path: backward weight streams of both networks][chunk 0: coarse pass, fine pass][chunk 1: ...]
// A pass region holds the pass's Kept: what pass_backward reads besides the weights.  Every region is sized for a full chunk.
constexpr uint64_t kSavedMagic = 0x32564153525343ull;   // "CSRSAV2": format of this header and layout
constexpr int64_t kSavedHeaderFloats = 64;
struct SavedHeader {
  uint64_t magic, floats;   // floats: the layout's total, checked against the arguments read back
  int64_t R, chunk;
  int nc, ni, flags, precision;
  nsr_arch arch;            // the network the forward ran (the default descriptor under a chain precision)
  unsigned embed;           // ... and the embedding's option word it ran with (include/nsr.h)
  int ray_stride;           // the forward call's ray stride: what a gradient with respect to the rays must be laid out for
};
static_assert(sizeof(SavedHeader) <= kSavedHeaderFloats * 4 && sizeof(SavedHeader) % 4 == 0, "header");
struct SavedLayout {
  int64_t stream, pass_c, pass_f, n_chunks, total;   // floats
};
int64_t kept_floats(int64_t P, const Shape* net, bool chain) {
  Carver a{nullptr};
  carve_kept(a, P, net, chain);
  return a.off;
}
SavedLayout saved_layout(const Shape& net, int precision, int64_t R, int nc, int ni, int64_t chunk) {
  const bool chain = chain_selected(precision);
  SavedLayout L;
  L.stream = chain ? align64((int64_t)(nsr_chain_bwd_packed_bytes() / 4)) : 0;
  L.pass_c = kept_floats(chunk * nc, chain ? nullptr : &net, chain);
  L.pass_f = kept_floats(chunk * (nc + ni), chain ? nullptr : &net, chain);
  L.n_chunks = (R + chunk - 1) / chunk;
  L.total = kSavedHeaderFloats + 2 * L.stream + L.n_chunks * (L.pass_c + L.pass_f);
  return L;
}
float* saved_stream(float* base, const SavedLayout& L, int net) { return base + kSavedHeaderFloats + net * L.stream; }
Kept saved_kept(float* base, const SavedLayout& L, const Run& c, const Pass& q) {
  Carver a{base + kSavedHeaderFloats + 2 * L.stream + q.ci * (L.pass_c + L.pass_f) + (q.net ? L.pass_c : 0)};
  return carve_kept(a, c.chunk * q.N, c.chain ? nullptr : &c.net, c.chain);
}
// the header is written on the stream (the call enqueues, it does not wait) and read back by the backward call
__global__ void saved_header_kernel(SavedHeader h, unsigned* __restrict__ dst) {
  const unsigned* src = reinterpret_cast<const unsigned*>(&h);
  const int i = threadIdx.x;
  if (i < (int)(sizeof(SavedHeader) / 4)) dst[i] = src[i];
}
bool same_arch(const nsr_arch& a, const nsr_arch& b) {
  return a.D == b.D && a.W == b.W && a.skips == b.skips && a.deg_pos == b.deg_pos && a.deg_dir == b.deg_dir && a.no_dir == b.no_dir;
}
bool sizes_ok(int64_t ray_chunk, int nc, int ni) { return ray_chunk > 0 && nc >= 2 && ni >= 1 && nc + ni <= 256; }

// ---- the forward / backward pair: nsr_train_* with the default descriptor and every precision, nsr_train_arch_* with the
// caller's descriptor and the layer-by-layer precisions only (by_arch) -------------------------------------------------------
size_t saved_bytes_of(const nsr_arch* arch, unsigned embed, bool by_arch, int precision, int64_t R, int nc, int ni, int64_t ray_chunk) {
  Shape S;
  if (make_shape(arch, S, embed) != NSR_OK) return 0;
  if (R <= 0 || check_shape(R, 1, nc, ni, precision, ray_chunk, by_arch) != NSR_OK) return 0;
  return (size_t)saved_layout(S, precision, R, nc, ni, ray_chunk).total * sizeof(float);
}

int train_forward(const nsr_arch* arch, unsigned embed, bool by_arch, const float* const* w_coarse, const float* const* w_fine, const float* rays,
                  int ray_stride, int64_t R, int n_coarse, int n_importance, int render_flags, int lindisp, const float* u_coarse,
                  const float* u_fine, const float* noise_coarse, const float* noise_fine, float noise_std, int precision,
                  int64_t ray_chunk, float* const* outs, void* workspace, size_t workspace_bytes, void* saved, size_t saved_bytes,
                  void* stream) {
  Run c{};
  NSR_TRY(make_shape(arch, c.net, embed));
  c.R = R; c.chunk = ray_chunk; c.nc = n_coarse; c.ni = n_importance; c.flags = render_flags; c.precision = precision;
  c.lindisp = lindisp; c.ray_stride = ray_stride; c.noise_std = noise_std;
  NSR_TRY(check_args({{w_coarse, w_fine, outs}, {w_coarse, w_fine}, outs, {rays, workspace, saved}, {workspace, saved},
                      c.net.n_tensors(), by_arch}, &c, 1));
  if (R == 0) return NSR_OK;
  Work k;
  NSR_TRY(open_work(c, w_coarse, w_fine, by_arch, workspace, workspace_bytes, k));
  const SavedLayout L = saved_layout(c.net, precision, R, n_coarse, n_importance, c.chunk);
  if (saved_bytes < (size_t)L.total * sizeof(float)) return NSR_ERR_WORKSPACE;
  hipStream_t st = nsr_stream(stream);
  float* sv = static_cast<float*>(saved);
  if (c.chain)   // the backward weight streams are packed into the saved state: the backward call uses them as they are
    for (int n = 0; n < 2; ++n) k.stream_b[n] = saved_stream(sv, L, n);
  const SavedHeader h{kSavedMagic, (uint64_t)L.total, R, c.chunk, n_coarse, n_importance, render_flags, precision, c.net.arch, embed, ray_stride};
  hipLaunchKernelGGL(saved_header_kernel, dim3(1), dim3(64), 0, st, h, reinterpret_cast<unsigned*>(sv));
  NSR_CHECK_LAUNCH();
  NSR_TRY(prepare_call(st, k, w_coarse, w_fine, c, stream, false));
  const float* z_c = nullptr;   // the coarse pass's samples of the chunk at hand
  return for_each_pass(c, [&](const Pass& q) -> int {
    k.kept = saved_kept(sv, L, c, q);
    if (q.net == 0) z_c = k.kept.z;
    float* const* o = outs + 4 * q.net;
    return pass_forward(st, k, c, q, q.net ? w_fine : w_coarse, rays, q.net ? u_fine : u_coarse,
                        q.net ? noise_fine : noise_coarse, z_c, rows_of(outs[3], q, c.nc, k.w_c), k.kept.z, o[0] + q.r0 * 3,
                        rows_of(o[1], q, 1), rows_of(o[2], q, 1), rows_of(o[3], q, q.N, q.net ? nullptr : k.w_c), stream);
  });
}

// nsr_train_backward_r: the forward call's rays and the call's option word (null: every other backward entry point)
struct ChainRays {
  const float* rays;
  int ray_stride;
  unsigned flags;
};
int train_backward(const nsr_arch* arch, unsigned embed, bool by_arch, const float* const* w_coarse, const float* const* w_fine,
                   const float* const* g_outs, float* const* g_coarse, float* const* g_fine, void* workspace, size_t workspace_bytes,
                   const void* saved, size_t saved_bytes, void* stream, float* g_rays = nullptr, int g_ray_stride = 0,
                   const ChainRays* cr = nullptr) {
  Run c{};   // no sampling in this half: lindisp and noise_std stay unused
  if (g_rays && !nsr_ray_stride_ok(g_ray_stride)) return NSR_ERR_INVALID_ARG;
  const bool weight_grads = !(cr && (cr->flags & NSR_BACKWARD_NO_WEIGHT_GRADS));
  const bool chain_r = cr && (g_rays || cr->flags != 0u);   // what only a chain precision's saved state can serve
  if (cr) {
    if ((cr->flags & ~NSR_BACKWARD_NO_WEIGHT_GRADS) != 0u || (!weight_grads && !g_rays)) return NSR_ERR_INVALID_ARG;
    if (g_rays && (!cr->rays || cr->ray_stride != g_ray_stride)) return NSR_ERR_INVALID_ARG;
  }
  NSR_TRY(make_shape(arch, c.net, embed));
  if (weight_grads) {
    NSR_TRY(check_args({{w_coarse, w_fine, g_outs, g_coarse, g_fine, workspace, saved}, {w_coarse, w_fine, g_coarse, g_fine},
                        nullptr, {}, {workspace, saved}, c.net.n_tensors(), by_arch}, nullptr, 1));
  } else {   // no gradient tensor is written: the two arrays may be null
    NSR_TRY(check_args({{w_coarse, w_fine, g_outs, workspace, saved}, {w_coarse, w_fine}, nullptr, {}, {workspace, saved},
                        c.net.n_tensors(), by_arch}, nullptr, 1));
  }
  if (saved_bytes < (size_t)kSavedHeaderFloats * sizeof(float)) return NSR_ERR_WORKSPACE;
  // the run's parameters, read back from the header the forward call wrote (waits for the stream)
  hipStream_t st = nsr_stream(stream);
  SavedHeader h{};
  if (hipMemcpyAsync(&h, saved, sizeof(h), hipMemcpyDeviceToHost, st) != hipSuccess) return NSR_ERR_LAUNCH;
  if (hipStreamSynchronize(st) != hipSuccess) return NSR_ERR_LAUNCH;
  if (h.magic != kSavedMagic) return NSR_ERR_INVALID_ARG;
  if (h.floats > saved_bytes / sizeof(float)) return NSR_ERR_WORKSPACE;   // the header says the state is larger than the buffer
  if (!same_arch(h.arch, c.net.arch) || h.embed != embed)   // the forward ran another network
    return chain_r ? NSR_ERR_UNSUPPORTED : NSR_ERR_INVALID_ARG;
  // bounds before anything loops over them (a damaged header may hold anything): every ray and every chunk takes at least
  // 64 floats of the layout, so neither count can exceed what the buffer holds
  if (h.R <= 0 || h.chunk <= 0 || h.chunk > h.R || (uint64_t)h.R > h.floats / 64 ||
      (uint64_t)((h.R + h.chunk - 1) / h.chunk) > h.floats / 64)
    return NSR_ERR_INVALID_ARG;
  c.R = h.R; c.chunk = h.chunk; c.nc = h.nc; c.ni = h.ni; c.flags = h.flags; c.precision = h.precision;
  if (check_shape(c.R, 1, c.nc, c.ni, c.precision, c.chunk, by_arch) != NSR_OK || c.chunk != h.chunk || check_flags(c.flags) != NSR_OK)
    return NSR_ERR_INVALID_ARG;
  const SavedLayout L = saved_layout(c.net, c.precision, c.R, c.nc, c.ni, c.chunk);
  if ((uint64_t)L.total != h.floats) return NSR_ERR_INVALID_ARG;
  if (chain_r && !chain_selected(c.precision)) return NSR_ERR_UNSUPPORTED;   // those have nsr_train_arch_backward_r
  if (g_rays && (h.ray_stride != g_ray_stride || (chain_selected(c.precision) && !chain_r)))
    return NSR_ERR_INVALID_ARG;   // laid out for another stride
  c.ray_stride = h.ray_stride;
  Work k;
  NSR_TRY(open_work(c, w_coarse, w_fine, by_arch, workspace, workspace_bytes, k, g_rays != nullptr));
  float* sv = const_cast<float*>(static_cast<const float*>(saved));   // read only
  if (c.chain) {
    for (int n = 0; n < 2; ++n) k.stream_b[n] = saved_stream(sv, L, n);
    if (g_rays) NSR_TRY(raygrad_f16_pack(st, w_coarse, k.rgw[0], w_fine, k.rgw[1]));
  } else {   // the padded weight copies the backward products read (no forward halves: NSR_FP32 / NSR_F16X3_GEMM run every
             // gradient on the fp32 MFMA), and under NSR_F16X3_GEMM_BWD their transposed split halves
    NSR_TRY(prepare_weights(st, c.net, w_coarse, k.pack[0], false));
    NSR_TRY(prepare_weights(st, c.net, w_fine, k.pack[1], false));
    if (bwd_selected(c.precision)) {
      NSR_TRY(prepare_weights_t(st, c.net, w_coarse, k.pack[0]));
      NSR_TRY(prepare_weights_t(st, c.net, w_fine, k.pack[1]));
    }
  }
  // the fused step's order of passes: the first chunk overwrites the gradients, later chunks accumulate
  return for_each_pass(c, [&](const Pass& q) -> int {
    k.kept = saved_kept(sv, L, c, q);
    const float* const* go = g_outs + 4 * q.net;
    if (!go[0] && hipMemsetAsync(k.g_comp, 0, (size_t)q.rc * 3 * sizeof(float), st) != hipSuccess) return NSR_ERR_LAUNCH;
    // the chunk's rows of the ray gradient: the coarse pass writes them, the fine pass adds its part
    const RayGrad rg{rows_of(g_rays, q, g_ray_stride), g_ray_stride, q.rc, q.N, k.kept.z, q.net,
                     cr && cr->rays ? cr->rays + q.r0 * c.ray_stride : nullptr};
    return pass_backward(st, k, c, q, q.net ? w_fine : w_coarse, k.kept.z, rows_of(go[0], q, 3, k.g_comp), rows_of(go[1], q, 1),
                         rows_of(go[2], q, 1), rows_of(go[3], q, q.N), q.net ? g_fine : g_coarse, stream, g_rays ? &rg : nullptr,
                         weight_grads);
  });
}

}  // namespace

extern "C" size_t nsr_train_workspace_bytes_for(int precision, int64_t ray_chunk, int n_coarse, int n_importance) {
  Shape S;
  if (!sizes_ok(ray_chunk, n_coarse, n_importance) || !train_precision_ok(precision) || make_shape(&kDefaultArch, S) != NSR_OK) return 0;
  const bool chain = chain_selected(precision);
  return (size_t)work_floats(ray_chunk, n_coarse, n_importance, chain ? nullptr : &S, true, chain, nullptr, nullptr, false,
                             bwd_selected(precision)) * sizeof(float);
}

extern "C" size_t nsr_train_workspace_bytes(int64_t ray_chunk, int n_coarse, int n_importance) {
  Shape S;
  if (!sizes_ok(ray_chunk, n_coarse, n_importance) || make_shape(&kDefaultArch, S) != NSR_OK) return 0;
  return (size_t)work_floats(ray_chunk, n_coarse, n_importance, &S, true, true, nullptr, nullptr, false, true) * sizeof(float);
}

extern "C" size_t nsr_train_arch_workspace_bytes(const nsr_arch* arch, int precision, int64_t ray_chunk, int n_coarse,
                                                 int n_importance) {
  return nsr_train_arch_workspace_bytes_e(arch, 0u, precision, ray_chunk, n_coarse, n_importance);
}
extern "C" size_t nsr_train_arch_workspace_bytes_e(const nsr_arch* arch, unsigned embed, int precision, int64_t ray_chunk,
                                                   int n_coarse, int n_importance) {
  Shape S;
  if (make_shape(arch, S, embed) != NSR_OK || !sizes_ok(ray_chunk, n_coarse, n_importance) || !train_precision_ok(precision) ||
      chain_selected(precision))
    return 0;
  return (size_t)work_floats(ray_chunk, n_coarse, n_importance, &S, split_selected(precision), false, nullptr, nullptr, false,
                             bwd_selected(precision)) * sizeof(float);
}

extern "C" size_t nsr_train_arch_workspace_bytes_r(const nsr_arch* arch, unsigned embed, int precision, int64_t ray_chunk,
                                                   int n_coarse, int n_importance) {
  Shape S;
  if (make_shape(arch, S, embed) != NSR_OK || !sizes_ok(ray_chunk, n_coarse, n_importance) || !train_precision_ok(precision) ||
      chain_selected(precision))
    return 0;
  return (size_t)work_floats(ray_chunk, n_coarse, n_importance, &S, split_selected(precision), false, nullptr, nullptr, true,
                             bwd_selected(precision)) * sizeof(float);
}

extern "C" int nsr_arch_n_tensors(const nsr_arch* arch) {
  Shape S;
  const int rc = make_shape(arch, S);
  return rc != NSR_OK ? rc : S.n_tensors();
}

extern "C" int64_t nsr_arch_tensor_numel(const nsr_arch* arch, int t) { return nsr_arch_tensor_numel_e(arch, 0u, t); }
extern "C" int64_t nsr_arch_tensor_numel_e(const nsr_arch* arch, unsigned embed, int t) {
  Shape S;
  if (make_shape(arch, S, embed) != NSR_OK) return 0;
  return tensor_numel_of(S, t);
}

extern "C" int nsr_train_loss_and_grads_var(const float* const* w_coarse, const float* const* w_fine, float* const* g_coarse,
                                            float* const* g_fine, const float* rays, int ray_stride, int64_t R, int s2,
                                            const float* target_lr, int n_coarse, int n_importance, int white_bkgd, int lindisp,
                                            const float* u_coarse, const float* u_fine, const float* noise_coarse,
                                            const float* noise_fine, float noise_std, float lambda_coarse, float lambda_fine,
                                            int precision, int64_t ray_chunk, float* const* outs, float* lr_coarse, float* lr_fine,
                                            float* losses, void* workspace, size_t workspace_bytes, void* stream,
                                            const nsr_train_var_losses* var, float* var_losses) {
  if (!var) return NSR_ERR_INVALID_ARG;
  const bool rgb_var = var->lambda_coarse_var != 0.0f || var->lambda_fine_var != 0.0f;
  const bool depth_var = var->lambda_coarse_depth_var != 0.0f || var->lambda_fine_depth_var != 0.0f;
  // torch.var over ONE sub-ray is 0 / 0 (the reference would train on NaN); a depth variance needs the divisor
  if ((rgb_var || depth_var) && s2 < 2) return NSR_ERR_INVALID_ARG;
  if (depth_var && !(var->far > 0.0f)) return NSR_ERR_INVALID_ARG;
  Run c{};
  c.R = R; c.chunk = ray_chunk; c.nc = n_coarse; c.ni = n_importance; c.flags = white_bkgd; c.precision = precision;
  c.lindisp = lindisp; c.ray_stride = ray_stride; c.noise_std = noise_std;
  NSR_TRY(make_shape(&kDefaultArch, c.net));
  NSR_TRY(check_args({{w_coarse, w_fine, g_coarse, g_fine, outs}, {w_coarse, w_fine, g_coarse, g_fine}, outs,
                      {rays, target_lr, lr_coarse, lr_fine, losses, workspace}, {workspace}}, &c, s2));
  if (R == 0) return NSR_OK;
  Work k;
  NSR_TRY(open_work(c, w_coarse, w_fine, false, workspace, workspace_bytes, k));
  hipStream_t st = nsr_stream(stream);
  const double mse_scale = 1.0 / (3.0 * (double)(R / s2));
  NSR_TRY(prepare_call(st, k, w_coarse, w_fine, c, stream));
  return for_each_pass(c, [&](const Pass& q) -> int {
    const int net = q.net;
    const float* const* w = net ? w_fine : w_coarse;
    float* const* o = outs + 4 * net;
    float* z = net ? k.kept.z : k.z_c;
    float* comp = o[0] + q.r0 * 3;
    float* depth = rows_of(o[1], q, 1, depth_var ? k.scratch_out : nullptr);   // the depth-variance loss reads it
    NSR_TRY(pass_forward(st, k, c, q, w, rays, net ? u_fine : u_coarse, net ? noise_fine : noise_coarse, k.z_c,
                         rows_of(outs[3], q, c.nc, k.w_c), z, comp, depth, rows_of(o[2], q, 1),
                         rows_of(o[3], q, q.N, net ? nullptr : k.w_c), stream));
    // s^2 mean, loss, dL/d(comp)
    const int64_t lr0 = q.r0 / s2, n_lr = q.rc / s2;
    const float lambda = net ? lambda_fine : lambda_coarse;
    const int nblk = (int)((n_lr + 255) / 256);
    const float l_var = net ? var->lambda_fine_var : var->lambda_coarse_var;
    const float l_dvar = net ? var->lambda_fine_depth_var : var->lambda_coarse_depth_var;
    NSR_TRY(lr_loss(st, comp, target_lr + lr0 * 3, n_lr, s2, mse_scale, lambda, (net ? lr_fine : lr_coarse) + lr0 * 3, k.g_comp,
                    k.block_sums, l_var, l_dvar, var->far, depth_var ? depth : nullptr, depth_var ? k.g_depth : nullptr));
    NSR_TRY(loss_finish(st, k.block_sums, nblk, mse_scale, lambda, losses, net, k.carry, l_var, l_dvar, var_losses));
    return pass_backward(st, k, c, q, w, z, k.g_comp, depth_var ? k.g_depth : nullptr, nullptr, nullptr,
                         net ? g_fine : g_coarse, stream);
  });
}

// the step without the variance losses: every lambda 0, and a `far` that is never read
extern "C" int nsr_train_loss_and_grads(const float* const* w_coarse, const float* const* w_fine, float* const* g_coarse,
                                        float* const* g_fine, const float* rays, int ray_stride, int64_t R, int s2,
                                        const float* target_lr, int n_coarse, int n_importance, int white_bkgd, int lindisp,
                                        const float* u_coarse, const float* u_fine, const float* noise_coarse, const float* noise_fine,
                                        float noise_std, float lambda_coarse, float lambda_fine, int precision, int64_t ray_chunk,
                                        float* const* outs, float* lr_coarse, float* lr_fine, float* losses, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  static const nsr_train_var_losses none = {0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
  return nsr_train_loss_and_grads_var(w_coarse, w_fine, g_coarse, g_fine, rays, ray_stride, R, s2, target_lr, n_coarse, n_importance,
                                      white_bkgd, lindisp, u_coarse, u_fine, noise_coarse, noise_fine, noise_std, lambda_coarse,
                                      lambda_fine, precision, ray_chunk, outs, lr_coarse, lr_fine, losses, workspace, workspace_bytes,
                                      stream, &none, nullptr);
}

extern "C" size_t nsr_train_saved_bytes(int precision, int64_t R, int n_coarse, int n_importance, int64_t ray_chunk) {
  return saved_bytes_of(&kDefaultArch, 0u, false, precision, R, n_coarse, n_importance, ray_chunk);
}
extern "C" size_t nsr_train_arch_saved_bytes(const nsr_arch* arch, int precision, int64_t R, int n_coarse, int n_importance,
                                             int64_t ray_chunk) {
  return saved_bytes_of(arch, 0u, true, precision, R, n_coarse, n_importance, ray_chunk);
}
extern "C" size_t nsr_train_arch_saved_bytes_e(const nsr_arch* arch, unsigned embed, int precision, int64_t R, int n_coarse,
                                               int n_importance, int64_t ray_chunk) {
  return saved_bytes_of(arch, embed, true, precision, R, n_coarse, n_importance, ray_chunk);
}

extern "C" int nsr_train_forward(const float* const* w_coarse, const float* const* w_fine, const float* rays, int ray_stride,
                                 int64_t R, int n_coarse, int n_importance, int render_flags, int lindisp,
                                 const float* u_coarse, const float* u_fine, const float* noise_coarse, const float* noise_fine,
                                 float noise_std, int precision, int64_t ray_chunk, float* const* outs, void* workspace,
                                 size_t workspace_bytes, void* saved, size_t saved_bytes, void* stream) {
  return train_forward(&kDefaultArch, 0u, false, w_coarse, w_fine, rays, ray_stride, R, n_coarse, n_importance, render_flags, lindisp,
                       u_coarse, u_fine, noise_coarse, noise_fine, noise_std, precision, ray_chunk, outs, workspace, workspace_bytes,
                       saved, saved_bytes, stream);
}
extern "C" int nsr_train_arch_forward(const nsr_arch* arch, const float* const* w_coarse, const float* const* w_fine,
                                      const float* rays, int ray_stride, int64_t R, int n_coarse, int n_importance, int render_flags,
                                      int lindisp, const float* u_coarse, const float* u_fine, const float* noise_coarse,
                                      const float* noise_fine, float noise_std, int precision, int64_t ray_chunk, float* const* outs,
                                      void* workspace, size_t workspace_bytes, void* saved, size_t saved_bytes, void* stream) {
  return nsr_train_arch_forward_e(arch, 0u, w_coarse, w_fine, rays, ray_stride, R, n_coarse, n_importance, render_flags, lindisp,
                                  u_coarse, u_fine, noise_coarse, noise_fine, noise_std, precision, ray_chunk, outs, workspace,
                                  workspace_bytes, saved, saved_bytes, stream);
}
extern "C" int nsr_train_arch_forward_e(const nsr_arch* arch, unsigned embed, const float* const* w_coarse, const float* const* w_fine,
                                        const float* rays, int ray_stride, int64_t R, int n_coarse, int n_importance, int render_flags,
                                        int lindisp, const float* u_coarse, const float* u_fine, const float* noise_coarse,
                                        const float* noise_fine, float noise_std, int precision, int64_t ray_chunk, float* const* outs,
                                        void* workspace, size_t workspace_bytes, void* saved, size_t saved_bytes, void* stream) {
  return train_forward(arch, embed, true, w_coarse, w_fine, rays, ray_stride, R, n_coarse, n_importance, render_flags, lindisp, u_coarse,
                       u_fine, noise_coarse, noise_fine, noise_std, precision, ray_chunk, outs, workspace, workspace_bytes, saved,
                       saved_bytes, stream);
}

extern "C" int nsr_train_backward(const float* const* w_coarse, const float* const* w_fine, const float* const* g_outs,
                                  float* const* g_coarse, float* const* g_fine, void* workspace, size_t workspace_bytes,
                                  const void* saved, size_t saved_bytes, void* stream) {
  return train_backward(&kDefaultArch, 0u, false, w_coarse, w_fine, g_outs, g_coarse, g_fine, workspace, workspace_bytes, saved,
                        saved_bytes, stream);
}
extern "C" int nsr_train_arch_backward(const nsr_arch* arch, const float* const* w_coarse, const float* const* w_fine,
                                       const float* const* g_outs, float* const* g_coarse, float* const* g_fine, void* workspace,
                                       size_t workspace_bytes, const void* saved, size_t saved_bytes, void* stream) {
  return nsr_train_arch_backward_e(arch, 0u, w_coarse, w_fine, g_outs, g_coarse, g_fine, workspace, workspace_bytes, saved,
                                   saved_bytes, stream);
}
extern "C" int nsr_train_arch_backward_e(const nsr_arch* arch, unsigned embed, const float* const* w_coarse,
                                         const float* const* w_fine, const float* const* g_outs, float* const* g_coarse,
                                         float* const* g_fine, void* workspace, size_t workspace_bytes, const void* saved,
                                         size_t saved_bytes, void* stream) {
  return train_backward(arch, embed, true, w_coarse, w_fine, g_outs, g_coarse, g_fine, workspace, workspace_bytes, saved, saved_bytes,
                        stream);
}

extern "C" int nsr_train_arch_backward_r(const nsr_arch* arch, unsigned embed, const float* const* w_coarse,
                                         const float* const* w_fine, const float* const* g_outs, float* const* g_coarse,
                                         float* const* g_fine, float* g_rays, int g_ray_stride, void* workspace, size_t workspace_bytes,
                                         const void* saved, size_t saved_bytes, void* stream) {
  return train_backward(arch, embed, true, w_coarse, w_fine, g_outs, g_coarse, g_fine, workspace, workspace_bytes, saved, saved_bytes,
                        stream, g_rays, g_ray_stride);
}

extern "C" size_t nsr_train_workspace_bytes_r(int precision, int64_t ray_chunk, int n_coarse, int n_importance) {
  Shape S;
  if (!sizes_ok(ray_chunk, n_coarse, n_importance) || !train_precision_ok(precision) || make_shape(&kDefaultArch, S) != NSR_OK) return 0;
  const bool chain = chain_selected(precision);
  return (size_t)work_floats(ray_chunk, n_coarse, n_importance, chain ? nullptr : &S, true, chain, nullptr, nullptr, chain,
                             bwd_selected(precision)) * sizeof(float);
}

extern "C" int nsr_train_backward_r(const float* const* w_coarse, const float* const* w_fine, const float* rays, int ray_stride,
                                    const float* const* g_outs, float* const* g_coarse, float* const* g_fine, float* g_rays,
                                    int g_ray_stride, unsigned flags, void* workspace, size_t workspace_bytes, const void* saved,
                                    size_t saved_bytes, void* stream) {
  const ChainRays cr{rays, ray_stride, flags};
  return train_backward(&kDefaultArch, 0u, false, w_coarse, w_fine, g_outs, g_coarse, g_fine, workspace, workspace_bytes, saved,
                        saved_bytes, stream, g_rays, g_ray_stride, &cr);
}

extern "C" int nsr_train_status_reset(void* workspace, void* stream) {
  if (!workspace) return NSR_ERR_INVALID_ARG;
  if (hipMemsetAsync(workspace, 0, 64, nsr_stream(stream)) != hipSuccess) return NSR_ERR_LAUNCH;
  return NSR_OK;
}

extern "C" int nsr_train_status(void* workspace, int clear, unsigned* flags_out, void* stream) {
  if (!workspace || !flags_out) return NSR_ERR_INVALID_ARG;
  hipStream_t st = nsr_stream(stream);
  unsigned host = 0;
  if (hipMemcpyAsync(&host, workspace, sizeof(unsigned), hipMemcpyDeviceToHost, st) != hipSuccess) return NSR_ERR_LAUNCH;
  if (clear && hipMemsetAsync(workspace, 0, sizeof(unsigned), st) != hipSuccess) return NSR_ERR_LAUNCH;
  if (hipStreamSynchronize(st) != hipSuccess) return NSR_ERR_LAUNCH;
  *flags_out = host;
  return NSR_OK;
}

extern "C" int nsr_adam_step_n(int n, const int64_t* numel, float* const* w, const float* const* g, float* const* m, float* const* v,
                               int step, float lr, float beta1, float beta2, float eps, void* stream) {
  if (n < 1 || n > kMaxT || !numel || !w || !g || !m || !v || step < 1) return NSR_ERR_INVALID_ARG;
  AdamN a{};
  for (int i = 0; i < n; ++i) {
    if (!w[i] || !g[i] || !m[i] || !v[i] || numel[i] < 0) return NSR_ERR_INVALID_ARG;
    a.w[i] = w[i]; a.g[i] = g[i]; a.m[i] = m[i]; a.v[i] = v[i]; a.n[i] = numel[i];
  }
  // bias corrections in double like Python's floats, then one rounding to fp32
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  const float step_size = (float)((double)lr / bc1), bc2_sqrt = (float)sqrt(bc2);
  hipLaunchKernelGGL(adam_n_kernel, dim3(64, n), dim3(256), 0, nsr_stream(stream), a, beta1, beta2, eps, step_size, bc2_sqrt);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

// the 24 tensors of the default network
extern "C" int nsr_adam_step(float* const* w, const float* const* g, float* const* m, float* const* v, int step, float lr,
                             float beta1, float beta2, float eps, void* stream) {
  Shape S;
  NSR_TRY(make_shape(&kDefaultArch, S));
  int64_t numel[NSR_N_STATE_TENSORS];
  for (int t = 0; t < NSR_N_STATE_TENSORS; ++t) numel[t] = tensor_numel_of(S, t);
  return nsr_adam_step_n(NSR_N_STATE_TENSORS, numel, w, g, m, v, step, lr, beta1, beta2, eps, stream);
}
