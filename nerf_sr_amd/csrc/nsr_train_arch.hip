// Train-mode forward / backward pair for a network of ANY architecture the reference's flags describe (include/nsr_train.h,
// nsr_arch: --D --W --skips --deg_pos --deg_dir --no_dir), layer by layer on the GEMM path's kernels.
//
// Everything here is a function of the descriptor at run time: the padded shapes (Shape), the kept state of a pass and the
// workspace (carve_kept / work_floats: one list for the workspace and for a pass region of the saved buffer), the padded
// weight copies and their split-fp16 halves (Pack), the drivers over the D trunk layers (net_forward / net_backward).  The
// three products of a linear layer, the deterministic reductions behind them and the per-ray stages (sampling, density
// noise, gamma, compositing and its backward) are the default path's own host functions (nsr_train_work.h): this unit adds
// an encoder with run-time degrees, the scatter of the compositing backward's (P, 4) rows into the two head layouts, and Adam
// over n tensors.
//
// Layout of a pass over P sample points, r32 = rounded up to 32 (the K tile of the GEMM kernels; padding columns hold zeros
// and meet zero weight columns):
//   Kx = r32(3 + 6 deg_pos), Wp = r32(W), Hp = r32(W / 2), Dp = r32(3 + 6 deg_dir) (0 under no_dir)
//   x[j]  (P, Kx + Wp)   one per skip layer: [pe | h of the layer below]: cat([pe, h]) is the buffer itself; layer 0 reads
//                        columns 0 .. Kx of x[0].  A network without skips has one (P, Kx) buffer.
//   h[l]  (P, Wp)        output of trunk layer l, unless layer l + 1 is a skip layer (then it lies in that layer's x)
//   ci    (P, Wp + Dp)   the colour branch's input [xyz_encoding_final | dir pe]
//   cc    (P, Hp)        dir_encoding's output;  rgb (P, 4) = colours + raw sigma;  sig (P) noisy sigma;  z (P)
// Backward: the density head is stacked under xyz_encoding_final as one (Wp + 32)-row layer, so the gradient of the trunk's
// last activation is one product over [d final | d sigma 0 .. 0]; the colour head is 32 rows.
#include "nsr_gemm.h"
#include "nsr_train_work.h"
#include "../../include/nsr_train.h"

using namespace nsr;

namespace {

constexpr int kMaxD = NSR_ARCH_MAX_D, kMaxT = 2 * NSR_ARCH_MAX_D + 8;
inline int r32(int n) { return (n + 31) & ~31; }

struct Shape {
  int D, W, H, in_xyz, in_dir, Kx, Wp, Hp, Dp, Ci, Xs, ldx, n_x, no_dir;
  unsigned skips;
  int x_of[kMaxD];        // the x buffer that is layer l's input (layer 0 and skip layers), else -1
  int64_t part_stride;    // floats of one split-K slice: >= every padded weight-gradient shape
  nsr_arch arch;
  bool skip(int l) const { return l > 0 && ((skips >> l) & 1u); }
  int n_tensors() const { return 2 * D + 8; }
  int kin(int l) const { return l == 0 ? Kx : (skip(l) ? Xs : Wp); }             // padded fan-in of trunk layer l
  int fan_in(int l) const { return l == 0 ? in_xyz : (skip(l) ? in_xyz + W : W); }
  int dir_in() const { return W + (no_dir ? 0 : in_dir); }
  // indices into the state tensors
  int final_w() const { return 2 * D; }
  int dir_w() const { return 2 * D + 2; }
  int sigma_w() const { return 2 * D + 4; }
  int rgb_w() const { return 2 * D + 6; }
};

// malformed -> NSR_ERR_INVALID_ARG, beyond the stated limits -> NSR_ERR_UNSUPPORTED (include/nsr_train.h)
int make_shape(const nsr_arch* a, Shape& S) {
  if (!a) return NSR_ERR_INVALID_ARG;
  if (a->D < 1 || a->W < 2 || (a->W & 1) || a->deg_pos < 0 || a->deg_dir < 0 || (a->no_dir != 0 && a->no_dir != 1))
    return NSR_ERR_INVALID_ARG;
  if ((a->skips & 1u) || (a->D < 32 && (a->skips >> a->D) != 0u)) return NSR_ERR_INVALID_ARG;
  if (a->D > NSR_ARCH_MAX_D || a->W > NSR_ARCH_MAX_W || a->deg_pos > NSR_ARCH_MAX_DEG || a->deg_dir > NSR_ARCH_MAX_DEG)
    return NSR_ERR_UNSUPPORTED;
  S.arch = *a;
  S.D = a->D; S.W = a->W; S.H = a->W / 2; S.skips = a->skips; S.no_dir = a->no_dir;
  S.in_xyz = 3 + 6 * a->deg_pos; S.in_dir = 3 + 6 * a->deg_dir;
  S.Kx = r32(S.in_xyz); S.Wp = r32(S.W); S.Hp = r32(S.H); S.Dp = a->no_dir ? 0 : r32(S.in_dir);
  S.Ci = S.Wp + S.Dp; S.Xs = S.Kx + S.Wp;
  int ns = 0;
  for (int l = 0; l < S.D; ++l) {
    S.x_of[l] = -1;
    if (S.skip(l)) S.x_of[l] = ns++;
  }
  S.x_of[0] = 0;
  S.n_x = ns > 0 ? ns : 1;
  S.ldx = ns > 0 ? S.Xs : S.Kx;
  int kin_max = S.Kx > S.Wp ? S.Kx : S.Wp;
  if (ns > 0) kin_max = S.Xs;
  int64_t m = (int64_t)S.Wp * kin_max;
  if ((int64_t)S.Hp * S.Ci > m) m = (int64_t)S.Hp * S.Ci;
  if (32 * (int64_t)S.Wp > m) m = 32 * (int64_t)S.Wp;
  S.part_stride = align64(m);
  return NSR_OK;
}
int64_t tensor_numel_of(const Shape& S, int t) {
  if (t < 0 || t >= S.n_tensors()) return 0;
  if (t < 2 * S.D) return (t & 1) ? S.W : (int64_t)S.W * S.fan_in(t / 2);
  switch (t - 2 * S.D) {
    case 0: return (int64_t)S.W * S.W;
    case 1: return S.W;
    case 2: return (int64_t)S.H * S.dir_in();
    case 3: return S.H;
    case 4: return S.W;
    case 5: return 1;
    case 6: return 3 * (int64_t)S.H;
    default: return 3;
  }
}

// E1 + cast_rays with run-time degree: one thread per (sample point, 4 columns) writes dst[p][4 g .. 4 g + 4) of
//   [x, sin(2^0 x), cos(2^0 x), sin(2^1 x), ...  | zeros up to 4 n_groups]      (x: the point o + z d, or the view direction)
// with nsr_sincos on the ldexpf frequencies, the values of encode_train_kernel (nsr_train_gemm.hip)
// The row is computed once and written to every destination (one x buffer per skip layer; all with row stride ld).
struct EncodeDst {
  float* p[kMaxD];
  int n;
};
__global__ void __launch_bounds__(256) encode_arch_kernel(const float* __restrict__ rays, int stride, const float* __restrict__ z,
                                                          int64_t P, int N, int deg, int view_dir, EncodeDst dst, int64_t ld,
                                                          int n_groups) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t p = idx / n_groups;
  const int g = (int)(idx % n_groups);
  if (p >= P) return;
  const NsrRay q = nsr_load_ray(rays, p / N, stride);
  float x[3];
  if (view_dir) {
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = q.v[c];
  } else {
    const float zk = z[p];
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = __fadd_rn(q.o[c], __fmul_rn(zk, q.d[c]));   // cast_rays, models/utils.py:5-14
  }
  const int n_valid = 3 + 6 * deg;
  float out[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = 4 * g + e;
    float v = 0.0f;
    if (c < 3) {
      v = c == 0 ? x[0] : (c == 1 ? x[1] : x[2]);
    } else if (c < n_valid) {
      const int f = (c - 3) / 6, r = (c - 3) % 6, comp = r % 3;
      const float xc = comp == 0 ? x[0] : (comp == 1 ? x[1] : x[2]);
      float sn, cs;
      nsr_sincos(ldexpf(xc, f), sn, cs);
      v = r < 3 ? sn : cs;
    }
    out[e] = v;
  }
  for (int j = 0; j < dst.n; ++j)
    *reinterpret_cast<float4*>(dst.p[j] + p * ld + 4 * g) = make_float4(out[0], out[1], out[2], out[3]);
}

// the compositing backward's compact rows d4[p] = (d rgb_pre 0..2, d sigma) into the layouts the two heads' products read:
// drgb (P, 32) = [d rgb_pre | 0], gsig[p * ldg + 0 .. 32) = [d sigma | 0].  One thread per (point, float4).
__global__ void __launch_bounds__(256) scatter_heads_kernel(const float4* __restrict__ d4, int64_t P, float* __restrict__ drgb,
                                                            float* __restrict__ gsig, int64_t ldg) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t p = idx >> 3;
  const int j = (int)(idx & 7);
  if (p >= P) return;
  float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
  if (j == 0) {
    const float4 v = d4[p];
    a = make_float4(v.x, v.y, v.z, 0.0f);
    b.x = v.w;
  }
  reinterpret_cast<float4*>(drgb + p * 32)[j] = a;
  reinterpret_cast<float4*>(gsig + p * ldg)[j] = b;
}

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

// ---- kept state, weight copies, workspace: one list each, functions of the descriptor --------------------------------
struct AKept {
  float* x[kMaxD];
  float* h[kMaxD];   // null: the layer's output lies in the x buffer of the skip layer above it
  float *ci, *cc, *rgb, *sig, *z;
};
AKept carve_kept(Carver& a, const Shape& S, int64_t P) {
  AKept q{};
  for (int j = 0; j < S.n_x; ++j) q.x[j] = a.take(P * S.ldx);
  for (int l = 0; l < S.D; ++l) q.h[l] = (l + 1 < S.D && S.skip(l + 1)) ? nullptr : a.take(P * S.Wp);
  q.ci = a.take(P * S.Ci);   q.cc = a.take(P * S.Hp);
  q.rgb = a.take(P * 4);   q.sig = a.take(P);   q.z = a.take(P);
  return q;
}
struct Mat { float* p; int64_t ld; };
Mat out_of(const Shape& S, const AKept& s, int l) {
  if (s.h[l]) return {s.h[l], S.Wp};
  return {s.x[S.x_of[l + 1]] + S.Kx, S.Xs};
}
Mat in_of(const Shape& S, const AKept& s, int l) {
  if (l == 0) return {s.x[0], S.ldx};
  if (S.skip(l)) return {s.x[S.x_of[l]], S.Xs};
  return out_of(S, s, l - 1);
}

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
};
Pack carve_pack(Carver& a, const Shape& S, bool split) {
  Pack q{};
  const int64_t off0 = a.off;
  q.first = a.take(0);
  for (int l = 0; l < S.D; ++l) {
    const bool pad = l == 0 || S.skip(l) || S.W != S.Wp;
    q.wl[l] = a.take((int64_t)S.Wp * S.kin(l), pad);
    q.bl[l] = a.take(S.Wp, S.W != S.Wp);
  }
  q.w9 = a.take((int64_t)(S.Wp + 32) * S.Wp);   q.b9 = a.take(S.Wp + 32);
  q.wdir = a.take((int64_t)S.Hp * S.Ci);        q.bdir = a.take(S.Hp, S.H != S.Hp);
  q.wrgb = a.take(32 * (int64_t)S.Hp);          q.brgb = a.take(32);
  q.floats = a.off - off0;
  if (split) {
    for (int l = 0; l < S.D; ++l) q.hi[l] = reinterpret_cast<unsigned short*>(a.take((int64_t)S.Wp * S.kin(l)));
    q.hi[kFinalE] = reinterpret_cast<unsigned short*>(a.take((int64_t)S.Wp * S.Wp));
    q.hi[kSigmaE] = reinterpret_cast<unsigned short*>(a.take(32 * (int64_t)S.Wp));
    q.hi[kDirE] = reinterpret_cast<unsigned short*>(a.take((int64_t)S.Hp * S.Ci));
    q.hi[kRgbE] = reinterpret_cast<unsigned short*>(a.take(32 * (int64_t)S.Hp));
  }
  return q;
}
struct Lin {   // a trunk layer's forward operand: weights with row stride ldw (the padded copy, or the caller's tensor), bias
  const float* w;
  int ldw;
  const float* b;
};
Lin trunk_lin(const Shape& S, const Pack& q, const float* const* w, int l) {
  return {q.wl[l] ? q.wl[l] : w[2 * l], q.wl[l] ? S.kin(l) : S.W, q.bl[l] ? q.bl[l] : w[2 * l + 1]};
}

struct AWork {
  unsigned* status;   // not written by this unit: reserves the block nsr_train_status reads at the start of any workspace
  AKept kept;
  float *g0, *g1, *drgb, *d4, *col_tiles, *z_c, *w_c, *g_comp, *partial;
  Pack pack[2];
};
int64_t work_floats(const Shape& S, bool split, int64_t chunk, int nc, int ni, AWork* w, float* base) {
  const int64_t P = chunk * (nc + ni);
  Carver a{base};
  AWork tmp;
  AWork& k = w ? *w : tmp;
  k.status = reinterpret_cast<unsigned*>(a.take(16));
  k.kept = carve_kept(a, S, P);
  k.g0 = a.take(P * (S.Wp + 32));   k.g1 = a.take(P * (S.Wp + 32));
  k.drgb = a.take(P * 32);   k.d4 = a.take(P * 4);
  k.col_tiles = a.take((P / 128 + 1) * S.Wp + 2 * 64 * S.Wp + 64);   // per-tile column sums + 64 slices of doubles
  k.z_c = a.take(chunk * nc);   k.w_c = a.take(chunk * nc);
  k.g_comp = a.take(chunk * 3);
  k.partial = a.take(kMaxSplits * S.part_stride);                    // also scratch of the small bias sums
  for (int n = 0; n < 2; ++n) k.pack[n] = carve_pack(a, S, split);
  return a.off;
}

int prepare_weights(hipStream_t st, const Shape& S, const float* const* w, const Pack& q, bool split) {
  if (hipMemsetAsync(q.first, 0, (size_t)q.floats * sizeof(float), st) != hipSuccess) return NSR_ERR_LAUNCH;
  for (int l = 0; l < S.D; ++l) {
    if (q.wl[l]) {
      const int fi = S.fan_in(l), kin = S.kin(l);
      if (S.skip(l)) {
        NSR_TRY(place(st, q.wl[l], kin, 0, 0, w[2 * l], fi, S.W, S.in_xyz, 0, 0));
        NSR_TRY(place(st, q.wl[l], kin, 0, S.Kx, w[2 * l], fi, S.W, S.W, S.in_xyz, 0));
      } else {
        NSR_TRY(place(st, q.wl[l], kin, 0, 0, w[2 * l], fi, S.W, fi, 0, 0));
      }
    }
    if (q.bl[l]) NSR_TRY(place(st, q.bl[l], S.Wp, 0, 0, w[2 * l + 1], S.W, 1, S.W, 0, 0));
  }
  const int F = S.final_w();
  NSR_TRY(place(st, q.w9, S.Wp, 0, 0, w[F], S.W, S.W, S.W, 0, 0));
  NSR_TRY(place(st, q.w9, S.Wp, S.Wp, 0, w[S.sigma_w()], S.W, 1, S.W, 0, 0));
  NSR_TRY(place(st, q.b9, S.Wp + 32, 0, 0, w[F + 1], S.W, 1, S.W, 0, 0));
  NSR_TRY(place(st, q.b9, S.Wp + 32, 0, S.Wp, w[S.sigma_w() + 1], 1, 1, 1, 0, 0));
  NSR_TRY(place(st, q.wdir, S.Ci, 0, 0, w[S.dir_w()], S.dir_in(), S.H, S.W, 0, 0));
  if (!S.no_dir) NSR_TRY(place(st, q.wdir, S.Ci, 0, S.Wp, w[S.dir_w()], S.dir_in(), S.H, S.in_dir, S.W, 0));
  if (q.bdir) NSR_TRY(place(st, q.bdir, S.Hp, 0, 0, w[S.dir_w() + 1], S.H, 1, S.H, 0, 0));
  NSR_TRY(place(st, q.wrgb, S.Hp, 0, 0, w[S.rgb_w()], S.H, 3, S.H, 0, 0));
  NSR_TRY(place(st, q.brgb, 32, 0, 0, w[S.rgb_w() + 1], 3, 1, 3, 0, 0));
  if (split) {
    for (int l = 0; l < S.D; ++l) {
      const int64_t n = (int64_t)S.Wp * S.kin(l);
      NSR_TRY(split_f16(trunk_lin(S, q, w, l).w, n, q.hi[l], q.hi[l] + n, st));
    }
    const int64_t nf = (int64_t)S.Wp * S.Wp, ns = 32 * (int64_t)S.Wp, nd = (int64_t)S.Hp * S.Ci, nr = 32 * (int64_t)S.Hp;
    NSR_TRY(split_f16(q.w9, nf, q.hi[kFinalE], q.hi[kFinalE] + nf, st));
    NSR_TRY(split_f16(q.w9 + nf, ns, q.hi[kSigmaE], q.hi[kSigmaE] + ns, st));
    NSR_TRY(split_f16(q.wdir, nd, q.hi[kDirE], q.hi[kDirE] + nd, st));
    NSR_TRY(split_f16(q.wrgb, nr, q.hi[kRgbE], q.hi[kRgbE] + nr, st));
  }
  return NSR_OK;
}

// one forward layer: x (P, K) -> y (P, N), entry e of the pack's split halves when they exist
int fwd(hipStream_t st, const Pack& q, int e, const float* x, int64_t ldx, int K, const float* w, int ldw, const float* b, int act,
        float* y, int64_t ldy, int64_t P, int N, int n_valid) {
  const unsigned short* hi = q.hi[e];
  return lin_fwd_at(st, x, ldx, K, w, ldw, b, act, y, ldy, P, N, n_valid, hi, hi ? hi + (int64_t)N * K : nullptr, K);
}

// E1 + cast_rays of the P = rays x N sample points, then the network with everything kept for the backward pass
int net_forward(hipStream_t st, const Shape& S, const float* rays, int ray_stride, const float* z, int N, const float* const* w,
                const Pack& q, const AKept& s, int64_t P, int color_none) {
  {
    EncodeDst dst{};
    for (int j = 0; j < S.n_x; ++j) dst.p[j] = s.x[j];
    dst.n = S.n_x;
    const int64_t n = P * (S.Kx / 4);
    hipLaunchKernelGGL(encode_arch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, rays, ray_stride, z, P, N,
                       S.arch.deg_pos, 0, dst, (int64_t)S.ldx, S.Kx / 4);
    NSR_CHECK_LAUNCH();
  }
  if (!S.no_dir) {
    const int64_t n = P * (S.Dp / 4);
    EncodeDst dst{};
    dst.p[0] = s.ci + S.Wp;
    dst.n = 1;
    hipLaunchKernelGGL(encode_arch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, rays, ray_stride, z, P, N,
                       S.arch.deg_dir, 1, dst, (int64_t)S.Ci, S.Dp / 4);
    NSR_CHECK_LAUNCH();
  }
  for (int l = 0; l < S.D; ++l) {
    const Mat x = in_of(S, s, l), y = out_of(S, s, l);
    const Lin a = trunk_lin(S, q, w, l);
    NSR_TRY(fwd(st, q, l, x.p, x.ld, S.kin(l), a.w, a.ldw, a.b, kActRelu, y.p, y.ld, P, S.Wp, S.Wp));
  }
  const Mat hD = out_of(S, s, S.D - 1);
  // xyz_encoding_final into the colour branch's input, the density head (stacked under it in w9) into column 3 of rgb
  NSR_TRY(fwd(st, q, kFinalE, hD.p, hD.ld, S.Wp, q.w9, S.Wp, q.b9, kActNone, s.ci, S.Ci, P, S.Wp, S.Wp));
  NSR_TRY(fwd(st, q, kSigmaE, hD.p, hD.ld, S.Wp, q.w9 + (int64_t)S.Wp * S.Wp, S.Wp, q.b9 + S.Wp, kActNone, s.rgb + 3, 4, P, 32, 1));
  NSR_TRY(fwd(st, q, kDirE, s.ci, S.Ci, S.Ci, q.wdir, S.Ci, q.bdir ? q.bdir : w[S.dir_w() + 1], kActRelu, s.cc, S.Hp, P, S.Hp, S.Hp));
  NSR_TRY(fwd(st, q, kRgbE, s.cc, S.Hp, S.Hp, q.wrgb, S.Hp, q.brgb, color_none ? kActNone : kActSigmoid, s.rgb, 4, P, 32, 3));
  return NSR_OK;
}

// backward of the network from k.d4 (composite_bwd's compact rows); g: its 2 D + 8 gradient tensors
int net_backward(hipStream_t st, const Shape& S, const float* const* w, const Pack& q, const AWork& k, const Work& kw, int64_t P,
                 float* const* g, int acc, int stop_grad) {
  const AKept& s = k.kept;
  const int sp = n_splits(P);
  const int64_t ps = S.part_stride;
  float* part = k.partial;
  const int ldg = S.Wp + 32;
  hipLaunchKernelGGL(scatter_heads_kernel, dim3((unsigned)((P * 8 + 255) / 256)), dim3(256), 0, st,
                     reinterpret_cast<const float4*>(k.d4), P, k.drgb, k.g1 + S.Wp, (int64_t)ldg);
  NSR_CHECK_LAUNCH();
  // rgb head
  NSR_TRY(lin_wgrad(st, k.drgb, 32, 32, s.cc, S.Hp, S.Hp, P, part, sp, ps));
  NSR_TRY(reduce_place(st, g[S.rgb_w()], S.H, 0, 3, S.H, part, sp, S.Hp, 0, 0, acc, 1.0f, ps));
  NSR_TRY(colsum(st, k.drgb, 32, P, 0, 3, g[S.rgb_w() + 1], acc, part));
  NSR_TRY(lin_dgrad(st, kw, k.drgb, 32, 32, q.wrgb, S.Hp, s.cc, S.Hp, k.g0, S.Hp, P, S.Hp, g[S.dir_w() + 1], acc, S.H));
  // dir_encoding: its input is [final | dir pe]
  NSR_TRY(lin_wgrad(st, k.g0, S.Hp, S.Hp, s.ci, S.Ci, S.Ci, P, part, sp, ps));
  NSR_TRY(reduce_place(st, g[S.dir_w()], S.dir_in(), 0, S.H, S.W, part, sp, S.Ci, 0, 0, acc, 1.0f, ps));
  if (!S.no_dir) NSR_TRY(reduce_place(st, g[S.dir_w()], S.dir_in(), S.W, S.H, S.in_dir, part, sp, S.Ci, 0, S.Wp, acc, 1.0f, ps));
  const int F = S.final_w();
  if (stop_grad) {   // --stop_grad (models/networks.py:218-219): dir_encoding's input is detached, d final = 0
    if (hipMemset2DAsync(k.g1, (size_t)ldg * sizeof(float), 0, (size_t)S.Wp * sizeof(float), (size_t)P, st) != hipSuccess) return NSR_ERR_LAUNCH;
    if (!acc && hipMemsetAsync(g[F + 1], 0, (size_t)S.W * sizeof(float), st) != hipSuccess) return NSR_ERR_LAUNCH;
  } else {
    NSR_TRY(lin_dgrad(st, kw, k.g0, S.Hp, S.Hp, q.wdir, S.Ci, nullptr, 0, k.g1, ldg, P, S.Wp, g[F + 1], acc, S.W));
  }
  // xyz_encoding_final + sigma: the (Wp + 32)-row layer over the trunk's last activation
  const Mat hD = out_of(S, s, S.D - 1);
  NSR_TRY(lin_wgrad(st, k.g1, ldg, S.Wp, hD.p, hD.ld, S.Wp, P, part, sp, ps));
  NSR_TRY(reduce_place(st, g[F], S.W, 0, S.W, S.W, part, sp, S.Wp, 0, 0, acc, 1.0f, ps));
  NSR_TRY(lin_wgrad(st, k.g1 + S.Wp, ldg, 32, hD.p, hD.ld, S.Wp, P, part, sp, ps));
  NSR_TRY(reduce_place(st, g[S.sigma_w()], S.W, 0, 1, S.W, part, sp, S.Wp, 0, 0, acc, 1.0f, ps));
  NSR_TRY(colsum(st, k.g1, ldg, P, S.Wp, 1, g[S.sigma_w() + 1], acc, part));
  NSR_TRY(lin_dgrad(st, kw, k.g1, ldg, ldg, q.w9, S.Wp, hD.p, hD.ld, k.g0, S.Wp, P, S.Wp, g[2 * (S.D - 1) + 1], acc, S.W));
  // trunk, top down; the gradient of a layer's pre-activation alternates between the two buffers
  const float* dy = k.g0;
  float* nx = k.g1;
  for (int l = S.D - 1; l >= 0; --l) {
    const Mat x = in_of(S, s, l);
    const int kin = S.kin(l), fi = S.fan_in(l);
    NSR_TRY(lin_wgrad(st, dy, S.Wp, S.Wp, x.p, x.ld, kin, P, part, sp, ps));
    float* gw = g[2 * l];
    if (S.skip(l)) {   // [pe | h] columns of the padded product -> the nn.Linear columns
      NSR_TRY(reduce_place(st, gw, fi, 0, S.W, S.in_xyz, part, sp, kin, 0, 0, acc, 1.0f, ps));
      NSR_TRY(reduce_place(st, gw, fi, S.in_xyz, S.W, S.W, part, sp, kin, 0, S.Kx, acc, 1.0f, ps));
    } else {
      NSR_TRY(reduce_place(st, gw, fi, 0, S.W, fi, part, sp, kin, 0, 0, acc, 1.0f, ps));
    }
    if (l == 0) break;
    // the layer's input h is the ReLU output of layer l - 1: its mask, and that layer's bias gradient
    const Mat m = out_of(S, s, l - 1);
    const Lin a = trunk_lin(S, q, w, l);
    NSR_TRY(lin_dgrad(st, kw, dy, S.Wp, S.Wp, a.w + (S.skip(l) ? S.Kx : 0), a.ldw, m.p, m.ld, nx, S.Wp, P, S.Wp, g[2 * (l - 1) + 1],
                      acc, S.W));
    const float* t0 = dy; dy = nx; nx = const_cast<float*>(t0);
  }
  return NSR_OK;
}

// a trunk layer without a padded copy is the GEMMs' operand where the caller holds it: 16-byte aligned (include/nsr_train.h)
int check_alignment(const Shape& S, const float* const* w) {
  for (int l = 1; l < S.D; ++l)
    if (!S.skip(l) && S.W == S.Wp && (reinterpret_cast<uintptr_t>(w[2 * l]) & 15) != 0) return NSR_ERR_INVALID_ARG;
  return NSR_OK;
}

// ---- the call layer ------------------------------------------------------------------------------------------------------
bool split_selected(int precision) { return precision == NSR_F16X3_GEMM; }
bool sizes_ok(int64_t ray_chunk, int nc, int ni, int precision) {
  return ray_chunk > 0 && nc >= 2 && ni >= 1 && nc + ni <= 256 && (precision == NSR_FP32 || precision == NSR_F16X3_GEMM);
}

// [header: 256 bytes][chunk 0: coarse pass, fine pass][chunk 1: ...], every region sized for a full chunk
constexpr uint64_t kArchSavedMagic = 0x41564153525343ull;   // "CSRSAVA"
constexpr int64_t kHeaderFloats = 64;
struct ArchSavedHeader {
  uint64_t magic, floats;
  int64_t R, chunk;
  int nc, ni, flags, precision;
  nsr_arch arch;
};
static_assert(sizeof(ArchSavedHeader) <= kHeaderFloats * 4 && sizeof(ArchSavedHeader) % 4 == 0, "header");
struct SavedLayout { int64_t pass_c, pass_f, n_chunks, total; };
int64_t kept_floats(const Shape& S, int64_t P) {
  Carver a{nullptr};
  carve_kept(a, S, P);
  return a.off;
}
SavedLayout saved_layout(const Shape& S, int64_t R, int nc, int ni, int64_t chunk) {
  SavedLayout L;
  L.pass_c = kept_floats(S, chunk * nc);
  L.pass_f = kept_floats(S, chunk * (nc + ni));
  L.n_chunks = (R + chunk - 1) / chunk;
  L.total = kHeaderFloats + L.n_chunks * (L.pass_c + L.pass_f);
  return L;
}
AKept saved_kept(float* base, const SavedLayout& L, const Shape& S, const Run& c, const Pass& q) {
  Carver a{base + kHeaderFloats + q.ci * (L.pass_c + L.pass_f) + (q.net ? L.pass_c : 0)};
  return carve_kept(a, S, c.chunk * q.N);
}
__global__ void arch_header_kernel(ArchSavedHeader h, unsigned* __restrict__ dst) {
  const unsigned* src = reinterpret_cast<const unsigned*>(&h);
  const int i = threadIdx.x;
  if (i < (int)(sizeof(ArchSavedHeader) / 4)) dst[i] = src[i];
}
bool same_arch(const nsr_arch& a, const nsr_arch& b) {
  return a.D == b.D && a.W == b.W && a.skips == b.skips && a.deg_pos == b.deg_pos && a.deg_dir == b.deg_dir && a.no_dir == b.no_dir;
}
// the default path's Work as far as its shared host functions read it (composite_bwd, lin_dgrad)
Work shared_view(const AWork& k) {
  Work v{};
  v.kept.rgb = k.kept.rgb;   v.kept.sig = k.kept.sig;
  v.d4 = k.d4;   v.col_tiles = k.col_tiles;
  return v;
}

}  // namespace

extern "C" int nsr_arch_n_tensors(const nsr_arch* arch) {
  Shape S;
  const int rc = make_shape(arch, S);
  return rc != NSR_OK ? rc : S.n_tensors();
}

extern "C" int64_t nsr_arch_tensor_numel(const nsr_arch* arch, int t) {
  Shape S;
  if (make_shape(arch, S) != NSR_OK) return 0;
  return tensor_numel_of(S, t);
}

extern "C" size_t nsr_train_arch_workspace_bytes(const nsr_arch* arch, int precision, int64_t ray_chunk, int n_coarse,
                                                 int n_importance) {
  Shape S;
  if (make_shape(arch, S) != NSR_OK || !sizes_ok(ray_chunk, n_coarse, n_importance, precision)) return 0;
  return (size_t)work_floats(S, split_selected(precision), ray_chunk, n_coarse, n_importance, nullptr, nullptr) * sizeof(float);
}

extern "C" size_t nsr_train_arch_saved_bytes(const nsr_arch* arch, int precision, int64_t R, int n_coarse, int n_importance,
                                             int64_t ray_chunk) {
  Shape S;
  if (make_shape(arch, S) != NSR_OK) return 0;
  if (R <= 0 || check_shape(R, 1, n_coarse, n_importance, precision, ray_chunk, true) != NSR_OK) return 0;
  return (size_t)saved_layout(S, R, n_coarse, n_importance, ray_chunk).total * sizeof(float);
}

extern "C" int nsr_train_arch_forward(const nsr_arch* arch, const float* const* w_coarse, const float* const* w_fine,
                                      const float* rays, int ray_stride, int64_t R, int n_coarse, int n_importance, int render_flags,
                                      int lindisp, const float* u_coarse, const float* u_fine, const float* noise_coarse,
                                      const float* noise_fine, float noise_std, int precision, int64_t ray_chunk, float* const* outs,
                                      void* workspace, size_t workspace_bytes, void* saved, size_t saved_bytes, void* stream) {
  Shape S;
  NSR_TRY(make_shape(arch, S));
  Run c{};
  c.R = R; c.chunk = ray_chunk; c.nc = n_coarse; c.ni = n_importance; c.flags = render_flags; c.precision = precision;
  c.lindisp = lindisp; c.ray_stride = ray_stride; c.noise_std = noise_std;
  NSR_TRY(check_args({{w_coarse, w_fine, outs}, {w_coarse, w_fine}, outs, {rays, workspace, saved}, {workspace, saved},
                      S.n_tensors(), true}, &c, 1));
  if (R == 0) return NSR_OK;
  NSR_TRY(check_alignment(S, w_coarse));
  NSR_TRY(check_alignment(S, w_fine));
  const bool split = split_selected(precision);
  if (workspace_bytes < (size_t)work_floats(S, split, c.chunk, c.nc, c.ni, nullptr, nullptr) * sizeof(float)) return NSR_ERR_WORKSPACE;
  AWork k;
  work_floats(S, split, c.chunk, c.nc, c.ni, &k, static_cast<float*>(workspace));
  const SavedLayout L = saved_layout(S, R, n_coarse, n_importance, c.chunk);
  if (saved_bytes < (size_t)L.total * sizeof(float)) return NSR_ERR_WORKSPACE;
  hipStream_t st = nsr_stream(stream);
  float* sv = static_cast<float*>(saved);
  const ArchSavedHeader h{kArchSavedMagic, (uint64_t)L.total, R, c.chunk, n_coarse, n_importance, render_flags, precision, *arch};
  hipLaunchKernelGGL(arch_header_kernel, dim3(1), dim3(64), 0, st, h, reinterpret_cast<unsigned*>(sv));
  NSR_CHECK_LAUNCH();
  NSR_TRY(prepare_weights(st, S, w_coarse, k.pack[0], split));
  NSR_TRY(prepare_weights(st, S, w_fine, k.pack[1], split));
  const float* z_c = nullptr;   // the coarse pass's samples of the chunk at hand
  return for_each_pass(c, [&](const Pass& q) -> int {
    k.kept = saved_kept(sv, L, S, c, q);
    const AKept& s = k.kept;
    if (q.net == 0) z_c = s.z;
    float* const* o = outs + 4 * q.net;
    NSR_TRY(pass_sample(c, q, rays, q.net ? u_fine : u_coarse, z_c, rows_of(outs[3], q, c.nc, k.w_c), s.z, stream));
    NSR_TRY(net_forward(st, S, rays + q.r0 * c.ray_stride, c.ray_stride, s.z, q.N, q.net ? w_fine : w_coarse, k.pack[q.net], s, q.P,
                        (c.flags & NSR_TRAIN_COLOR_NONE) != 0));
    return pass_finish(st, c, q, s.rgb + 3, 4, q.net ? noise_fine : noise_coarse, s.rgb, s.sig, s.z, o[0] + q.r0 * 3,
                       rows_of(o[1], q, 1), rows_of(o[2], q, 1), rows_of(o[3], q, q.N, q.net ? nullptr : k.w_c), stream);
  });
}

extern "C" int nsr_train_arch_backward(const nsr_arch* arch, const float* const* w_coarse, const float* const* w_fine,
                                       const float* const* g_outs, float* const* g_coarse, float* const* g_fine, void* workspace,
                                       size_t workspace_bytes, const void* saved, size_t saved_bytes, void* stream) {
  Shape S;
  NSR_TRY(make_shape(arch, S));
  NSR_TRY(check_args({{w_coarse, w_fine, g_outs, g_coarse, g_fine, workspace, saved}, {w_coarse, w_fine, g_coarse, g_fine},
                      nullptr, {}, {workspace, saved}, S.n_tensors(), true}, nullptr, 1));
  NSR_TRY(check_alignment(S, w_coarse));
  NSR_TRY(check_alignment(S, w_fine));
  if (saved_bytes < (size_t)kHeaderFloats * sizeof(float)) return NSR_ERR_WORKSPACE;
  // the run's parameters, read back from the header the forward call wrote (waits for the stream)
  hipStream_t st = nsr_stream(stream);
  ArchSavedHeader h{};
  if (hipMemcpyAsync(&h, saved, sizeof(h), hipMemcpyDeviceToHost, st) != hipSuccess) return NSR_ERR_LAUNCH;
  if (hipStreamSynchronize(st) != hipSuccess) return NSR_ERR_LAUNCH;
  if (h.magic != kArchSavedMagic) return NSR_ERR_INVALID_ARG;
  if (h.floats > saved_bytes / sizeof(float)) return NSR_ERR_WORKSPACE;   // the header says the state is larger than the buffer
  if (!same_arch(h.arch, *arch)) return NSR_ERR_INVALID_ARG;              // the forward ran another network
  // bounds before anything loops over them (a damaged header may hold anything)
  if (h.R <= 0 || h.chunk <= 0 || h.chunk > h.R || (uint64_t)h.R > h.floats / 64 ||
      (uint64_t)((h.R + h.chunk - 1) / h.chunk) > h.floats / 64)
    return NSR_ERR_INVALID_ARG;
  Run c{};   // no sampling in this half: lindisp, ray_stride and noise_std stay unused
  c.R = h.R; c.chunk = h.chunk; c.nc = h.nc; c.ni = h.ni; c.flags = h.flags; c.precision = h.precision;
  if (check_shape(c.R, 1, c.nc, c.ni, c.precision, c.chunk, true) != NSR_OK || c.chunk != h.chunk || check_flags(c.flags) != NSR_OK)
    return NSR_ERR_INVALID_ARG;
  const SavedLayout L = saved_layout(S, c.R, c.nc, c.ni, c.chunk);
  if ((uint64_t)L.total != h.floats) return NSR_ERR_INVALID_ARG;
  const bool split = split_selected(c.precision);
  if (workspace_bytes < (size_t)work_floats(S, split, c.chunk, c.nc, c.ni, nullptr, nullptr) * sizeof(float)) return NSR_ERR_WORKSPACE;
  AWork k;
  work_floats(S, split, c.chunk, c.nc, c.ni, &k, static_cast<float*>(workspace));
  float* sv = const_cast<float*>(static_cast<const float*>(saved));   // read only
  // the padded weight copies the backward products read (no split halves: every gradient runs on the fp32 MFMA)
  NSR_TRY(prepare_weights(st, S, w_coarse, k.pack[0], false));
  NSR_TRY(prepare_weights(st, S, w_fine, k.pack[1], false));
  return for_each_pass(c, [&](const Pass& q) -> int {
    k.kept = saved_kept(sv, L, S, c, q);
    const Work kw = shared_view(k);
    const float* const* go = g_outs + 4 * q.net;
    if (!go[0] && hipMemsetAsync(k.g_comp, 0, (size_t)q.rc * 3 * sizeof(float), st) != hipSuccess) return NSR_ERR_LAUNCH;
    NSR_TRY(composite_bwd(st, kw, k.kept.z, rows_of(go[0], q, 3, k.g_comp), q.rc, q.N, c.flags, true, rows_of(go[1], q, 1),
                          rows_of(go[2], q, 1), rows_of(go[3], q, q.N)));
    return net_backward(st, S, q.net ? w_fine : w_coarse, k.pack[q.net], k, kw, q.P, q.net ? g_fine : g_coarse, q.acc,
                        (c.flags & NSR_TRAIN_STOP_GRAD) != 0);
  });
}

extern "C" int nsr_adam_step_n(int n, const int64_t* numel, float* const* w, const float* const* g, float* const* m, float* const* v,
                               int step, float lr, float beta1, float beta2, float eps, void* stream) {
  if (n < 1 || n > kMaxT || !numel || !w || !g || !m || !v || step < 1) return NSR_ERR_INVALID_ARG;
  AdamN a{};
  for (int i = 0; i < n; ++i) {
    if (!w[i] || !g[i] || !m[i] || !v[i] || numel[i] < 0) return NSR_ERR_INVALID_ARG;
    a.w[i] = w[i]; a.g[i] = g[i]; a.m[i] = m[i]; a.v[i] = v[i]; a.n[i] = numel[i];
  }
  // bias corrections in double like Python's floats, then one rounding to fp32 (nsr_adam_step)
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  const float step_size = (float)((double)lr / bc1), bc2_sqrt = (float)sqrt(bc2);
  hipLaunchKernelGGL(adam_n_kernel, dim3(64, n), dim3(256), 0, nsr_stream(stream), a, beta1, beta2, eps, step_size, bc2_sqrt);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
