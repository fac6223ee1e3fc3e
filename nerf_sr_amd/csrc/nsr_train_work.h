// What the units of the training step share (internal; nsr_train.hip, nsr_train_gemm.hip, nsr_train_wgrad.hip): the shapes of
// the layer-by-layer network (Shape), what a pass keeps (Kept), the workspace of a call (Work), its validated arguments (Run),
// the host functions that cross a unit boundary.
#pragma once
#include <initializer_list>
#include "nsr_common.h"
#include "nsr_embed.h"
#include "../../include/nsr_train.h"

namespace nsr {

constexpr int kW = 256, kPe = 64, kDirOut = 128;   // the default network's padded widths (the chain path is laid out for them)
#ifndef NSR_MAX_SPLITS
#define NSR_MAX_SPLITS 256   // one workgroup per CU.  Same box, 2,048-ray step: 128 -> 6.15 ms, 256 -> 5.30 ms, 512 -> 5.60 ms
#endif
constexpr int kMaxSplits = NSR_MAX_SPLITS;
constexpr int kChainSlots = 14, kChainRowSlots = 12;     // chain path: partial sums of a network's 14 weight-gradient
                                                        // products and of its bias row sums, all alive until ONE finishing launch

// state_dict indices of the default network (nsr.h): layer i (1..8) weight = 2 (i - 1), bias = 2 (i - 1) + 1
constexpr int kFinalW = 16, kFinalB = 17, kDirW = 18, kDirB = 19, kSigmaW = 20, kSigmaB = 21, kRgbW = 22, kRgbB = 23;

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

// ---- the layer-by-layer network (nsr_train_gemm.hip): everything is a function of the descriptor at run time -----------
// Layout of a pass over P sample points, r32 = rounded up to 32 (the K tile of the GEMM kernels; padding columns hold zeros
// and meet zero weight columns):
//   Kx = r32(in_xyz), Wp = r32(W), Hp = r32(W / 2), Dp = r32(in_dir) (0 under no_dir); in_xyz = 3 + 6 deg_pos, in_dir =
//   3 + 6 deg_dir, without the 3 under NSR_EMBED_NO_XYZ of the embedding's option word (include/nsr.h)
//   x[j]  (P, Kx + Wp)   one per skip layer: [pe | h of the layer below]: cat([pe, h]) is the buffer itself; layer 0 reads
//                        columns 0 .. Kx of x[0].  A network without skips has one (P, Kx) buffer.
//   h[l]  (P, Wp)        output of trunk layer l, unless layer l + 1 is a skip layer (then it lies in that layer's x)
//   ci    (P, Wp + Dp)   the colour branch's input [xyz_encoding_final | dir pe]
//   cc    (P, Hp)        dir_encoding's output;  rgb (P, 4) = colours + raw sigma
constexpr int kMaxD = NSR_ARCH_MAX_D, kMaxT = 2 * NSR_ARCH_MAX_D + 8;
constexpr nsr_arch kDefaultArch = {8, 256, 1u << 4, 10, 4, 0};
struct Shape {
  int D, W, H, in_xyz, in_dir, Kx, Wp, Hp, Dp, Ci, Xs, ldx, n_x, no_dir;
  unsigned skips;
  int x_of[kMaxD];        // the x buffer that is layer l's input (layer 0 and skip layers), else -1
  int64_t part_stride;    // floats of one split-K slice: >= every padded weight-gradient shape
  nsr_arch arch;
  unsigned embed;          // the embedding's option word, and the bands of the two encodings (nsr_posenc_freqs)
  NsrBands bands_pos, bands_dir;
  bool skip(int l) const { return l > 0 && ((skips >> l) & 1u); }
  int n_tensors() const { return 2 * D + 8; }
  int n_pe() const { return 1 + __builtin_popcount(skips); }                      // layers that read the encoded position
  int kin(int l) const { return l == 0 ? Kx : (skip(l) ? Xs : Wp); }             // padded fan-in of trunk layer l
  int fan_in(int l) const { return l == 0 ? in_xyz : (skip(l) ? in_xyz + W : W); }
  int dir_in() const { return W + (no_dir ? 0 : in_dir); }
  // indices into the state tensors
  int final_w() const { return 2 * D; }
  int dir_w() const { return 2 * D + 2; }
  int sigma_w() const { return 2 * D + 4; }
  int rgb_w() const { return 2 * D + 6; }
};

// Zero-padded copies of the weights whose shapes are not the GEMM's (one block, zeroed per call), and the (hi, lo) fp16
// halves of the forward matrices.  A trunk layer whose shape needs no padding is read where the caller holds it.
constexpr int kFinalE = kMaxD, kSigmaE = kMaxD + 1, kDirE = kMaxD + 2, kRgbE = kMaxD + 3, kNumE = kMaxD + 4;
struct Pack {
  float* first;
  int64_t floats;
  float* wl[kMaxD];
  float* bl[kMaxD];
  float *w9, *b9, *wdir, *bdir, *wrgb, *brgb;
  unsigned short* hi[kNumE];
  // NSR_F16X3_GEMM_BWD only (else null): the TRANSPOSED split halves the input-gradient products read (nsr_train_bwd_f16.hip),
  // hi then lo, each (fan-in x fan-out) with the fan-out contiguous: trunk layer l (kin(l) x Wp), kFinalE = the stacked
  // xyz_encoding_final + sigma layer (Wp x (Wp + 32)), kDirE (Ci x Hp), kRgbE (Hp x 32); kSigmaE is not used
  unsigned short* ht[kNumE];
};

// What the forward half of a pass over P sample points leaves for its backward half (all row-major).  The fused step keeps
// it in the workspace; nsr_train_forward keeps one per pass in the caller's `saved` buffer (nsr_train.hip, carve_kept).
struct Kept {
  float* x[kMaxD];              // layer-by-layer network: the layout above
  float* h[kMaxD];              //   null: the layer's output lies in the x buffer of the skip layer above it
  float *ci, *cc;
  float *rgb, *sig, *z;         // both paths: (P, 4) colours + raw sigma, noisy sigma, sample depths
  char* zpan;                   // chain path: activation panels of the forward pass (2 bytes per value, nsr_f16x3_core.h)
  unsigned* sgn;                //             and its sign panels
};

struct Work {   // the workspace of a call, sized for P_max = chunk * (Nc + Ni) sample points
  unsigned* status; // sticky NSR_FLAG_* word of the training step (include/nsr_train.h): ALWAYS the first bytes of the workspace
  Kept kept;        // of the pass at hand (sized for a fine pass; kept.z is the fine pass's z)
  float* d4;        // (P, 4) = d(rgb_pre) 0..2, d(sigma) of every sample point (composite_bwd)
  // layer-by-layer network: the two alternating gradient matrices (P, Wp + 32), [d rgb_pre | 0] (P, 32), per-tile column sums
  // of a dgrad product, split-K slices of a weight gradient, the padded weights of both networks
  float *g0, *g1, *drgb, *col_tiles, *partial;
  Pack pack[2];
  float* bias_part; // chain path: (rays, 4) per-ray sums of d4: the bias gradients of the colour and density heads before their finish
  float *z_c, *w_c, *g_comp, *scratch_out;
  double *block_sums, *carry;
  float* g_depth;   // per ray: d(loss) / d(depth) of the depth-variance loss (zeros when it is off)
  // chain path: gradient panels of the backward chain, the two weight streams per network, per-slice row sums and partial
  // tiles of the weight-gradient products
  char* dpan;
  float *row_part, *slots;
  float *stream_f[2], *stream_b[2];
  float* pscale;    // per gradient panel and point: stored value x pscale = true gradient (written by the backward chain)
  unsigned* gmax;   // float bits of the largest magnitude in each gradient panel (written by the backward chain)
  // the gradient with respect to the rays (nsr_train_arch_backward_r; null otherwise): the gradients of the encoded position's
  // columns, n_pe() matrices (P, Kx) -- layer 0's, then each skip layer's --, of the encoded direction's columns (P, Dp), and
  // d(loss) / d(sample point) (P, 3)
  float *gpe, *gdir, *gx;
  // chain path, nsr_train_backward_r with g_rays (null otherwise): gx (P, 3) and gdir (P, 3) = per point d(loss) / d(x) and the
  // back-propagated direction term, and per network the packed weight columns of raygrad_f16 (kRayGradPieces KiB)
  float* rgw[2];
  // NSR_F16X3_GEMM_BWD (null otherwise; behind everything else, with the packs' transposed halves): kRangeWords words, cleared by
  // net_backward, each the float bits of the largest magnitude of one gradient matrix (the weight gradients' range)
  unsigned* range;
};
constexpr int kRangeWords = 64;
// the pass's rows of d(loss) / d(rays) for net_backward: `rays` rays of N samples at depths z; acc: added to (the fine pass)
struct RayGrad {
  float* rows;
  int stride;
  int64_t rays;
  int N;
  const float* z;
  int acc;
  const float* in = nullptr;   // chain path: the pass's rows of the forward call's rays (the encodings are recomputed from them)
};

struct Run {   // the validated arguments of one call
  int64_t R, chunk;
  int nc, ni, flags, precision, lindisp, ray_stride;
  float noise_std;
  bool chain;   // which implementation the precision selects: the chain kernels, or the layer-by-layer network `net`
  Shape net;
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
  bool gemm_only = false;                             // the chain precisions are NSR_ERR_UNSUPPORTED (nsr_train_arch_*)
};

// ---- nsr_train_gemm.hip: the layer-by-layer network
// malformed descriptor -> NSR_ERR_INVALID_ARG, beyond the stated limits -> NSR_ERR_UNSUPPORTED (include/nsr_train.h)
// embed: an unknown bit, or NO_XYZ on an encoding of degree 0 that the network reads -> NSR_ERR_INVALID_ARG
NSR_INTERNAL int make_shape(const nsr_arch* a, Shape& S, unsigned embed = 0u);
NSR_INTERNAL int64_t tensor_numel_of(const Shape& S, int t);
NSR_INTERNAL void carve_net_kept(Carver& a, const Shape& S, int64_t P, Kept& q);   // x, h, ci, cc
NSR_INTERNAL Pack carve_pack(Carver& a, const Shape& S, bool split);
// NSR_F16X3_GEMM_BWD: the pack's transposed split halves (Pack::ht), and their preparation once per call (after prepare_weights)
NSR_INTERNAL void carve_pack_t(Carver& a, const Shape& S, Pack& q);
NSR_INTERNAL int prepare_weights_t(hipStream_t st, const Shape& S, const float* const* w, const Pack& q);
// a trunk layer without a padded copy is the GEMMs' operand where the caller holds it: 16-byte aligned, else NSR_ERR_INVALID_ARG
NSR_INTERNAL int check_alignment(const Shape& S, const float* const* w);
// split: also the (hi, lo) fp16 halves of the forward matrices (NSR_F16X3_GEMM; the pack must have been carved with them)
NSR_INTERNAL int prepare_weights(hipStream_t st, const Shape& S, const float* const* w, const Pack& q, bool split);
// the encoder with run-time degree: row p of each of the n_dst (<= kMaxD) destinations, row stride ld floats (a multiple of 4,
// >= 4 n_groups; rows 16-byte aligned), gets columns [0, 4 n_groups) = [x, sin(2^0 x), cos(2^0 x), ..., 2^(deg - 1) | zeros] with
// x = the sample point o + z d of ray p / N (view_dir: the ray's encoded view direction; z is then not read); embed / bands:
// the option word's column map and band table (no identity columns under NO_XYZ, sin / cos of bands.f[k] * x under LINEAR_FREQS)
NSR_INTERNAL int encode_arch(hipStream_t st, const float* rays, int ray_stride, const float* z, int64_t P, int N, int deg,
                             int view_dir, float* const* dst_rows, int n_dst, int64_t ld, int n_groups, unsigned embed = 0u,
                             const NsrBands* bands = nullptr);   // bands: read under LINEAR_FREQS only
// E1 + cast_rays of the P = rays x N sample points, then the network with everything kept for the backward pass; the raw
// density goes to column 3 of s.rgb.  split: the forward products on the pack's split-fp16 halves
NSR_INTERNAL int net_forward(hipStream_t st, const Shape& S, const float* rays, int ray_stride, const float* z, int N,
                             const float* const* w, const Pack& q, const Kept& s, int64_t P, bool split, int color_none);
// backward of the network from k.d4 (composite_bwd's rows); g: its 2 D + 8 gradient tensors
// rg (null: none): also the pass's rows of d(loss) / d(rays), through k.gpe / k.gdir / k.gx
NSR_INTERNAL int net_backward(hipStream_t st, const Shape& S, const float* const* w, const Pack& q, const Work& k, int64_t P,
                              float* const* g, int acc, int stop_grad, const RayGrad* rg = nullptr);
// ---- nsr_train_bwd_f16.hip: the gradient products on the split-fp16 MFMA (three terms, small terms first, fp32 accumulation)
// hi[c * rows + r] = fp16(v), lo[c * rows + r] = fp16(v - hi), v = 2^6 w[r * ldw + c]: the transposed split copy of (rows x cols)
NSR_INTERNAL int split_f16_t(hipStream_t st, const float* w, int rows, int cols, int ldw, unsigned short* hi, unsigned short* lo);
// *word = max(*word, float bits of the largest |src[p * ld + col0 + c]|, p < P, c < cols): integer atomicMax on the bit patterns
NSR_INTERNAL int absmax_bits(hipStream_t st, const float* src, int64_t ld, int64_t P, int col0, int cols, unsigned* word);
// dx (P, N) = (dy (P, K) wt^T) * [mask > 0] with wt (N, K) the transposed split halves (row stride ldwt halves, a multiple of
// 8); K, N multiples of 32, lddy a multiple of 4 (else NSR_ERR_UNSUPPORTED), any P >= 1.  mask (row stride ldm), col_tiles
// ((ceil(P / 128), N): per-128-row-tile column sums of dx, what tile_sums reads) and out_max (raised to the float bits of the
// largest |dx|) may be null.  dy is scaled PER ROW: a row of dx depends on that row of dy, its mask row and the weights only
NSR_INTERNAL int dgrad_f16x3(hipStream_t st, const float* dy, int64_t lddy, int K, const unsigned short* wt_hi,
                             const unsigned short* wt_lo, int ldwt, const float* mask, int64_t ldm, float* dx, int64_t lddx, int64_t P,
                             int N, float* col_tiles, unsigned* out_max);
// partial[z] (M x N, row stride N, at partial + z * stride) = sum over the points p of slice z of dy[p][0 : M) x[p][0 : N)^T;
// slice z = points [z L, min((z + 1) L, P)), L = bwd_f16_slice_len(P, splits) (a slice behind P writes zeros); M, N multiples
// of 32, lddy, ldx of 4.  *max_bits: float bits of a bound of max |dy| (device memory): ONE power of two for the matrix
NSR_INTERNAL int64_t bwd_f16_slice_len(int64_t P, int splits);
NSR_INTERNAL int wgrad_f16x3(hipStream_t st, const float* dy, int64_t lddy, int M, const float* x, int64_t ldx, int N, int64_t P,
                             const unsigned* max_bits, float* partial, int splits, int64_t stride);
// ---- nsr_train_gemm.hip: the two kernels of the gradient with respect to the rays
// backward of encode_arch's row: g_x (P, 3) = d(loss) / d(x) from the gradients of the encoded columns, summed over the n_src
// (1 .. kMaxD) sources src[j] (P, ld_src; ld_src a multiple of 4, rows 16-byte aligned; columns [0, 4 n_groups) are read,
// n_groups <= 32) in the order given, and the encoded rows `enc` (row stride ld_enc) the forward kept: an identity column
// passes through (none under NO_XYZ), band f gives f (cos(f x) g_sin - sin(f x) g_cos) with the kept sin / cos and f =
// 2^k, or bands->f[k] under LINEAR_FREQS.  Sums in double, in a fixed order
NSR_INTERNAL int encode_bwd(hipStream_t st, const float* const* src, int n_src, int64_t ld_src, const float* enc, int64_t ld_enc,
                            int64_t P, int deg, int n_groups, unsigned embed, const NsrBands* bands, float* g_x);
// one wavefront per ray: row r of g_rays (R, stride 8 | 11) (+)= [sum_k g_x[r, k] | sum_k z[r, k] g_x[r, k] | 0 0 | -] over
// the ray's N samples; g_dir (R N, ld_dir; may be null): the gradients of the encoded direction's columns, whose column sums
// go through the direction encoding's backward once per ray (dir_enc: the kept encoded direction, row stride ld_enc; the row
// of the ray's first sample is read) into columns 3:6 at stride 8, columns 8:11 at stride 11.  acc: add to the row
NSR_INTERNAL int ray_grad(hipStream_t st, const float* g_x, const float* z, int64_t R, int N, const float* g_dir, int64_t ld_dir,
                          const float* dir_enc, int64_t ld_enc, int deg_dir, unsigned embed, const NsrBands* bands, float* g_rays,
                          int stride, int acc);
// ---- nsr_train_raygrad_f16.hip: the gradient with respect to the rays on the chain path, from the backward chain's panels
constexpr int kRayGradPieces = 144;                     // 1 KiB pieces of one network's packed columns: 64 + 64 + 16
constexpr int64_t kRayGradImageFloats = kRayGradPieces * 256;
// 64 w of xyz_encoding_1.weight, xyz_encoding_5.weight[:, 0:63] and dir_encoding.0.weight[:, 256:283] of both networks, split into
// fp16 (hi, lo) and laid out as the MFMA A fragments of raygrad_f16 (one launch; img_*: kRayGradImageFloats floats, 16-byte aligned)
NSR_INTERNAL int raygrad_f16_pack(hipStream_t st, const float* const* w_coarse, float* img_coarse, const float* const* w_fine,
                                  float* img_fine);
// one pass, after nsr_chain_bwd has filled dpan / pscale for its P = R N points (a multiple of 32, else NSR_ERR_UNSUPPORTED):
// g_pe = dz_1 W_1 + dz_5 W_5[:, 0:63] and g_de = dz_dir W_dir[:, 256:] on the fp16 MFMA (W_hi g + W_lo g, pscale behind each
// panel's partial sum), the encodings' backward in registers on sin / cos recomputed from rays (R, ray_stride) and z (R, N) by
// the forward's expression -> g_x (P, 3), g_dv (P, 3) (scratch), then ray_grad: row r of g_rays (R, ray_stride) (+)= [sum_k g_x |
// sum_k z g_x (+ sum_k g_dv at stride 8) | 0 0 | sum_k g_dv at stride 11].  stop_grad: no direction term (exact zeros)
NSR_INTERNAL int raygrad_f16(hipStream_t st, const float* img, const char* dpan, const float* pscale, const float* rays,
                             int ray_stride, const float* z, int64_t R, int N, int stop_grad, float* g_x, float* g_dv, float* g_rays,
                             int acc);
// ---- nsr_train_gemm.hip: the launchers of the reduction and placement kernels behind the layer-by-layer products
// dst[(r0 + i) * dst_ld + c0 + j] = src[i * src_ld + col0 + j], i < rows, j < cols (transpose: dst[(r0 + j) * dst_ld + c0 + i]):
// a copy of bits
NSR_INTERNAL int place(hipStream_t st, float* dst, int dst_ld, int r0, int c0, const float* src, int src_ld, int rows, int cols,
                       int col0, int transpose);
// d4 (P, 4) = (d rgb_pre 0..2, d sigma) -> drgb (P, 32) = [d rgb_pre | 0], gsig[p * ldg + 0 .. 32) = [d sigma | 0]
NSR_INTERNAL int scatter_heads(hipStream_t st, const float* d4, int64_t P, float* drgb, float* gsig, int64_t ldg);
// bias_grad[c] (+)= sum over the n_tiles rows of col_tiles (n_tiles, N) of column c, c < n_bias (0: N), summed in double;
// scratch: 64 * N doubles behind the n_tiles * N tile sums
NSR_INTERNAL int tile_sums(hipStream_t st, float* col_tiles, int64_t n_tiles, int N, int n_bias, float* bias_grad, int acc);
// dst[i * dst_ld + dc0 + j] (+)= scale * sum_z partial[z * stride + (pr0 + i) * p_ld + pc0 + j], i < rows, j < cols, z < splits;
// summed in double, rows * cols < 2^31
NSR_INTERNAL int reduce_place(hipStream_t st, float* dst, int dst_ld, int dc0, int rows, int cols, const float* partial,
                              int splits, int p_ld, int pr0, int pc0, int accumulate, float scale, int64_t stride);
// dst[c] (+)= sum over the P rows of src[r * ld + col0 + c], c < cols <= 4 (more: NSR_ERR_INVALID_ARG), summed in double;
// `scratch`: >= 256 * 4 doubles (the split-K partial buffer is free between two weight gradients)
NSR_INTERNAL int colsum(hipStream_t st, const float* src, int64_t ld, int64_t P, int col0, int cols, float* dst, int accumulate,
                        float* scratch);
// ---- nsr_train.hip: the launchers of the kernels between the rendered colours and the network's backward
// compositing backward: (P, 4) rows d4 = (d rgb_pre 0..2, d sigma) of R rays x N samples (N <= 256, else NSR_ERR_UNSUPPORTED);
// `white`: the training option word; gmax (10 words, cleared), bias_part (R, 4), g_depth (R), g_opacity (R), g_weights (R, N)
// may be null; g_opacity or g_weights non-null selects the FULL instantiation
NSR_INTERNAL int composite_bwd(hipStream_t st, const float* rgb, const float* sig, const float* z, const float* g_comp, int64_t R,
                               int N, int white, float* d4, unsigned* gmax, float* bias_part, const float* g_depth,
                               const float* g_opacity, const float* g_weights);
// out[p] = sigma[p * sigma_stride] + noise[p] * std (noise null: a copy)
NSR_INTERNAL int sigma_noise(hipStream_t st, const float* sigma, int sigma_stride, const float* noise, float std_, int64_t P,
                             float* out);
// columns 0..2 of the (P, 4) rows become pow(c, 1 / 2.2)
NSR_INTERNAL int gamma_points(hipStream_t st, float* rgb4, int64_t P);
// s2 mean of the n_lr x s2 composited colours, loss partials of ceil(n_lr / 256) blocks into block_sums [q * nblk + block],
// dL/d(comp) per sub-ray and (g_depth non-null) dL/d(depth)
NSR_INTERNAL int lr_loss(hipStream_t st, const float* comp, const float* target, int64_t n_lr, int s2, double scale, float lambda,
                         float* lr_out, float* g_comp, double* block_sums, float lambda_var, float lambda_dvar, float far,
                         const float* depth, float* g_depth);
// carry[slot], [2 + slot], [4 + slot] += the three sums of n block partials; losses[slot] (and var_losses, may be null) from them
NSR_INTERNAL int loss_finish(hipStream_t st, const double* block_sums, int n, double scale, float lambda, float* losses, int slot,
                             double* carry, float lambda_var, float lambda_dvar, float* var_losses);
// ---- nsr_train_wgrad.hip: weight and bias gradients of the chain path from the panels
// reads k.dpan, k.kept.zpan (both zero-padded to 128 points), k.gmax, k.pscale, k.d4, k.bias_part; scratch: k.slots, k.row_part
NSR_INTERNAL int chain_weight_grads(hipStream_t st, const Work& k, int64_t P, int64_t n_rays, float* const* g, int acc);
// a head's weight gradient as a stream over one R-row forward panel: partial[z * NW * R + c * R + row] = sum over the points p of
// slice z of w[p * w_stride + c] * panel[p][row], c < NW.  (R, NW) = (128, 3) or (256, 1), else NSR_ERR_UNSUPPORTED.  *slices
// = min(max(P / 32, 1), 1024) slices of ceil(P / 32 / slices) point groups each; a slice behind the last group writes zeros
NSR_INTERNAL int panel_wsums(hipStream_t st, int R, int NW, const char* panel, int64_t P, const float* w, int w_stride,
                             float* partial, int* slices);
// One second pass of the chain path's gradients (finish_jobs_kernel), sums in double:
//   kind 0: dst[i * dst_ld + dc0 + j] (+)= scale * sum_z partial[z * stride + i * p_ld + col(j)], i < rows, j < cols, z < splits;
//           col = enc_panel_row(enc_rows, .): 0 identity, 1 / 2 the panel row of column j of the encoded position / direction
//   kind 1: dst[i] (+)= scale * sum_z partial[z * rows + i], i < rows (cols = 1)
//   kind 2: dst[i] (+)= sum_z partial[z * stride + i], i < rows <= 4
struct FinishJob {
  float* dst;
  const float* partial;
  int64_t stride;
  int kind, dst_ld, dc0, rows, cols, splits, p_ld, accumulate, enc_rows;
  float scale;
};
constexpr int kMaxFinishJobs = 32;
// n jobs (1 .. kMaxFinishJobs, else NSR_ERR_INVALID_ARG) in ONE launch.  NSR_ERR_UNSUPPORTED before anything is launched where a
// job exceeds its 65,536 threads: kind 0, and kind 1 with splits <= 64, need rows * cols <= 65,536; kind 2 rows <= 4
NSR_INTERNAL int finish_jobs(hipStream_t st, const FinishJob* jobs, int n);

}  // namespace nsr
