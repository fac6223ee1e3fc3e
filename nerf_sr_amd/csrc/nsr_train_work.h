// What the units of the training step share (internal; nsr_train.hip, nsr_train_gemm.hip, nsr_train_wgrad.hip): the padded
// layer shapes, the workspace of a call (Work), its validated arguments (Run), the host functions that cross a unit boundary.
#pragma once
#include <initializer_list>
#include "nsr_common.h"

namespace nsr {

constexpr int kW = 256, kPe = 64, kX5 = 320, kGs = 288, kDirOut = 128, kRgbPad = 32;
constexpr int kSigmaCol = 256, kDeCol = 260;     // columns of the [g | sigma | 0 0 0 | de27 | 0] buffer
#ifndef NSR_MAX_SPLITS
#define NSR_MAX_SPLITS 256   // one workgroup per CU.  Same box, 2,048-ray step: 128 -> 6.15 ms, 256 -> 5.30 ms, 512 -> 5.60 ms
#endif
constexpr int kMaxSplits = NSR_MAX_SPLITS;
constexpr int64_t kPartialFloats = (int64_t)kGs * kX5;   // >= every padded weight-gradient shape
constexpr int kChainSlots = 14, kChainRowSlots = 12;     // chain path: partial sums of a network's 14 weight-gradient
                                                        // products and of its bias row sums, all alive until ONE finishing launch

// state_dict indices (nsr.h): layer i (1..8) weight = 2 (i - 1), bias = 2 (i - 1) + 1
constexpr int kFinalW = 16, kFinalB = 17, kDirW = 18, kDirB = 19, kSigmaW = 20, kSigmaB = 21, kRgbW = 22, kRgbB = 23;
__host__ __device__ static constexpr int64_t tensor_numel(int t) {
  switch (t) {
    case 0: return 256 * 63;
    case 8: return 256 * 319;
    case kFinalW: return 256 * 256;
    case kDirW: return 128 * 283;
    case kDirB: return 128;
    case kSigmaW: return 256;
    case kSigmaB: return 1;
    case kRgbW: return 3 * 128;
    case kRgbB: return 3;
    default: return (t & 1) ? 256 : 256 * 256;
  }
}

static inline int64_t align64(int64_t n) { return (n + 63) & ~(int64_t)63; }   // floats -> 256-byte granules
// split-K factor of the weight gradients: 2 row tiles x splits workgroups should cover the 256 CUs at least once
static inline int n_splits(int64_t P) {
  const int64_t s = (P + 511) / 512;
  return (int)(s < 1 ? 1 : (s > kMaxSplits ? kMaxSplits : s));
}

#define NSR_TRY(expr)            \
  do {                           \
    const int rc_ = (expr);      \
    if (rc_ != NSR_OK) return rc_; \
  } while (0)

// GEMM path: zero-padded copies of the weights whose shapes are not MFMA friendly (floats, one block)
struct WeightPack {
  float *w1p, *w5p, *w9p, *wdirp, *wrgbp, *b9p, *brgbp;
  unsigned short* split;   // NSR_F16X3: (hi, lo) fp16 halves of the twelve forward weight matrices (kSplit* below)
};
// forward weight matrices in split-fp16 form: index, rows, K
constexpr int kSplitRows[12] = {256, 256, 256, 256, 256, 256, 256, 256, 256, 32, 128, 32};
constexpr int kSplitK[12] = {64, 256, 256, 256, 320, 256, 256, 256, 256, 256, 288, 128};
static constexpr int64_t split_offset(int e) { return e == 0 ? 0 : split_offset(e - 1) + 2 * (int64_t)kSplitRows[e - 1] * kSplitK[e - 1]; }
constexpr int64_t kSplitHalves = split_offset(11) + 2 * (int64_t)kSplitRows[11] * kSplitK[11];

// What the forward half of a pass over P sample points leaves for its backward half (all row-major).  The fused step keeps
// it in the workspace; nsr_train_forward keeps one per pass in the caller's `saved` buffer (nsr_train.hip, kept_floats).
struct Kept {
  float *x5, *h[9], *gs, *cc;   // GEMM path: [pe64 | h4], h1..h8 (h[0], h[4] unused), [g | sigma | de], dir_encoding's output
  float *rgb, *sig, *z;         // both paths: (P, 4) colours (+ raw sigma on the chain path), noisy sigma, sample depths
  char* zpan;                   // chain path: activation panels of the forward pass (2 bytes per value, nsr_f16x3_core.h)
  unsigned* sgn;                //             and its sign panels
};

struct Work {   // the workspace of a call, sized for P_max = chunk * (Nc + Ni) sample points
  unsigned* status; // sticky NSR_FLAG_* word of the training step (include/nsr_train.h): ALWAYS the first bytes of the workspace
  Kept kept;        // of the pass at hand (sized for a fine pass; kept.z is the fine pass's z)
  float *g0, *g1, *drgb, *col_tiles;
  float* d4;        // chain path: (P, 4) = d(rgb_pre) 0..2, d(sigma) of every sample point (composite_bwd_kernel COMPACT)
  float* bias_part; // chain path: (rays, 4) per-ray sums of d4: the bias gradients of the colour and density heads before their finish
  float *z_c, *w_c, *comp, *g_comp, *partial, *scratch_out;
  double *block_sums, *carry;
  float* g_depth;   // per ray: d(loss) / d(depth) of the depth-variance loss (zeros when it is off)
  WeightPack pack[2];
  // chain path: gradient panels of the backward chain, the two weight streams per network, per-slice row sums and partial
  // tiles of the weight-gradient products
  char* dpan;
  float *row_part, *slots;
  float *stream_f[2], *stream_b[2];
  float* pscale;    // per gradient panel and point: stored value x pscale = true gradient (written by the backward chain)
  unsigned* gmax;   // float bits of the largest magnitude in each gradient panel (written by the backward chain)
};

struct Run {   // the validated arguments of one call
  int64_t R, chunk;
  int nc, ni, flags, precision, lindisp, ray_stride;
  float noise_std;
  bool chain;
};

// one element of torch.optim.Adam: torch/optim/adam.py (_single_tensor_adam) operation order, fp32
__device__ __forceinline__ void adam_update(const float* gp, float* mp, float* vp, float* wp, int64_t i, float beta1, float beta2,
                                            float eps, float step_size, float bc2_sqrt) {
  const float g = gp[i];
  const float m = __fadd_rn(__fmul_rn(mp[i], beta1), __fmul_rn(g, 1.0f - beta1));
  const float v = __fadd_rn(__fmul_rn(vp[i], beta2), __fmul_rn(__fmul_rn(g, g), 1.0f - beta2));   // addcmul: (g*g)*value
  mp[i] = m;
  vp[i] = v;
  const float denom = __fadd_rn(__fdiv_rn(sqrtf(v), bc2_sqrt), eps);
  wp[i] = __fsub_rn(wp[i], __fmul_rn(step_size, __fdiv_rn(m, denom)));
}

struct Carver {   // hands out consecutive 256-byte granules of `base` (null: only counts them)
  float* base;
  int64_t off = 0;
  float* take(int64_t n, bool on = true) {
    if (!on) return nullptr;
    float* p = base ? base + off : nullptr;
    off += align64(n);
    return p;
  }
};

// ---- the passes of a call ----------------------------------------------------------------------------------------------
struct Pass {
  int net, N;               // 0 = coarse, 1 = fine; its samples per ray
  int64_t P, r0, rc, ci;    // sample points; first ray and rays of the chunk; index of the chunk
  int acc;                  // gradients: the first chunk overwrites them, later chunks accumulate
};
// chunk by chunk, coarse then fine
template <class F> int for_each_pass(const Run& c, F&& body) {
  for (int64_t r0 = 0, ci = 0; r0 < c.R; r0 += c.chunk, ++ci) {
    const int64_t rc = (c.R - r0 < c.chunk) ? c.R - r0 : c.chunk;
    for (int net = 0; net < 2; ++net) {
      const int N = net ? c.nc + c.ni : c.nc;
      NSR_TRY(body(Pass{net, N, rc * N, r0, rc, ci, r0 > 0}));
    }
  }
  return NSR_OK;
}
// the pass's rows of a per-ray array of the whole call (`width` values per ray); null: `fallback`
template <class T, class U = T> T* rows_of(T* p, const Pass& q, int64_t width, U* fallback = nullptr) {
  return p ? p + q.r0 * width : fallback;
}

struct Need {   // the pointers a driver requires of its caller
  std::initializer_list<const void*> always;          // whatever R is
  std::initializer_list<const float* const*> state;   // arrays of n_state tensors, every one of them set
  float* const* outs;                                 // not null: its two colour outputs [0], [4], when there are rays
  std::initializer_list<const void*> with_rays;       // when there are rays
  std::initializer_list<const void*> aligned;         // on 256 bytes
  int n_state = 24;                                   // NSR_N_STATE_TENSORS, or 2 D + 8 of an architecture descriptor
  bool gemm_only = false;                             // the chain precisions are NSR_ERR_UNSUPPORTED (nsr_train_arch.hip)
};

// ---- nsr_train.hip: what its drivers share with those of nsr_train_arch.hip
NSR_INTERNAL int check_shape(int64_t R, int s2, int n_coarse, int n_importance, int precision, int64_t& ray_chunk, bool gemm_only = false);
NSR_INTERNAL int check_flags(int flags);
NSR_INTERNAL int check_args(const Need& need, Run* c, int s2);
NSR_INTERNAL int pass_sample(const Run& c, const Pass& q, const float* rays, const float* u, const float* z_c, const float* w_c, float* z,
                             void* stream);
NSR_INTERNAL int pass_finish(hipStream_t st, const Run& c, const Pass& q, const float* sigma_raw, int sigma_stride, const float* noise,
                             float* rgb4, float* sig, const float* z, float* comp, float* depth, float* opac, float* wts, void* stream);
// reads k.kept.rgb / k.kept.sig; compact: (P, 4) rows into k.d4 (k.gmax, k.bias_part may be null), else k.drgb / k.g1
NSR_INTERNAL int composite_bwd(hipStream_t st, const Work& k, const float* z, const float* g_comp, int64_t R, int N, int white, bool compact,
                               const float* g_depth, const float* g_opacity, const float* g_weights);

// ---- nsr_train_gemm.hip: the layer-by-layer path.  precision: NSR_FP32 or NSR_F16X3 (split-fp16 forward products)
NSR_INTERNAL int prepare_weights(hipStream_t st, const float* const* w, const WeightPack& q, int precision);
// E1 + cast_rays of the P = rays x N sample points into s.x5 / s.gs, then M1 forward with everything kept for the backward pass
NSR_INTERNAL int net_forward(hipStream_t st, const float* rays, int ray_stride, const float* z, int N, const float* const* w,
                             const WeightPack& q, const Kept& s, int64_t P, int precision, int color_none);
// backward of M1: d_rgb_pre in k.drgb (P, 32), d_sigma in column 256 of k.g1 (P, 288)
NSR_INTERNAL int net_backward(hipStream_t st, const float* const* w, const WeightPack& q, const Work& k, int64_t P, float* const* g,
                              int acc, int stop_grad);
// the host wrappers of its kernels (one linear layer's three products, the deterministic reductions behind them)
NSR_INTERNAL int place(hipStream_t st, float* dst, int dst_ld, int r0, int c0, const float* src, int src_ld, int rows, int cols,
                       int col0, int transpose);
NSR_INTERNAL int lin_fwd_at(hipStream_t st, const float* x, int64_t ldx, int K, const float* w, int ldw, const float* b, int act,
                            float* y, int64_t ldy, int64_t P, int N, int n_valid, const unsigned short* hi, const unsigned short* lo,
                            int ldh);
NSR_INTERNAL int lin_dgrad(hipStream_t st, const Work& k, const float* dy, int64_t lddy, int K, const float* w, int ldw,
                           const float* mask, int64_t ldm, float* dx, int64_t lddx, int64_t P, int N, float* bias_grad, int acc,
                           int n_bias = 0);
NSR_INTERNAL int lin_wgrad(hipStream_t st, const float* dy, int64_t lddy, int M, const float* x, int64_t ldx, int N, int64_t P,
                           float* partial, int splits, int64_t stride = kPartialFloats);
NSR_INTERNAL int reduce_place(hipStream_t st, float* dst, int dst_ld, int dc0, int rows, int cols, const float* partial, int splits,
                              int p_ld, int pr0, int pc0, int accumulate, float scale = 1.0f, int64_t stride = kPartialFloats);
NSR_INTERNAL int colsum(hipStream_t st, const float* src, int64_t ld, int64_t P, int col0, int cols, float* dst, int accumulate,
                        float* scratch);
// ---- nsr_train_wgrad.hip: weight and bias gradients of the chain path from the panels
NSR_INTERNAL int chain_weight_grads(hipStream_t st, const Work& k, int64_t P, int64_t n_rays, float* const* g, int acc);

}  // namespace nsr
