// The gradient with respect to the rays on the CHAIN path (nsr_train_backward_r, include/nsr_train.h): what the backward
// chain leaves behind is enough.  After nsr_chain_bwd the gradient panel set holds the masked pre-activation gradients as fp16
// `hi` operands in the chain's own MFMA B-operand layout (nsr_f16x3_core.h "Training panels"): panel 0 = dz of trunk layer 1,
// panel 4 = dz of the skip layer 5, panel 9 = dz of dir_encoding, stored value x pscale[panel][point] = true value.  The
// gradients of the encoded columns are three small products with weight columns the chain never multiplies by,
//     g_pe (P, 63) = dz_1 W_1 + dz_5 W_5[:, 0:63]          g_de (P, 27) = dz_dir W_dir[:, 256:283]
// evaluated TRANSPOSED like every chain product (nsr_mlp_layout.h): A = the weight columns (output row i = an encoded
// column), B = a panel unit loaded as it lies (unit u of block nb IS k-step 2 nb + u; lane (m, h) finds its 16 bytes in slot
// (2m + h) ^ 8u), v_mfma_f32_32x32x16_f16, two terms per product (W_hi g + W_lo g: the panels carry g_hi only), fp32
// accumulation, the point's power of two applied once per panel behind the panel's partial sum.
//
// Output rows are ordered so that the D fragment of lane (m, h) holds the gradients of exactly the encoded values
// encode_point<1> (nsr_mlp_encode.h) gives that lane: register r of output block b = encoding register t = 16 b + r, column
// pecol(t, h) / dircol(t, h).  The encoding's backward then runs in registers on sin / cos recomputed by the forward's own
// expression -- identity columns pass through, band k adds 2^k (g_sin cos - g_cos sin), sums in double -- the two lane halves
// of a point meet in one shuffle, and the kernel stores per point d(loss) / d(x) (P, 3) and the back-propagated direction
// term (P, 3).  The per-ray sums are ray_grad's (nsr_train_gemm.hip; one wavefront per ray, double, fixed order), fed the
// direction term as three identity columns (degree 0).  No float atomics anywhere: a ray's row depends on that ray only.
//
// Weights: a pack launch per backward call splits 64 w of the three column ranges into fp16 (hi, lo) and lays them out as the
// A fragments of the k-steps, 144 pieces of 1 KiB per network (64 + 64 + 16).  A workgroup of four waves takes 128 points, a
// wave 32; it stages ONE part at a time in LDS (at most 64 KiB), so that two workgroups share a CU.
#include "nsr_mlp_encode.h"
#include "nsr_panels.h"
#include "nsr_train_work.h"

using namespace nsr;

namespace {

typedef unsigned rg_u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 rg_h8 __attribute__((ext_vector_type(8)));
typedef float rg_f32x16 __attribute__((ext_vector_type(16)));

constexpr float kRgScale = 64.0f, kRgInvScale = 1.0f / 64.0f;   // the weights enter as 64 w: their lo halves stay normal fp16
constexpr int kRgParts = 3;

// part 0: xyz_encoding_1.weight (256, 63) x panel 0;  1: xyz_encoding_5.weight[:, 0:63] (256, 319) x panel 4;
// 2: dir_encoding.0.weight[:, 256:283] (128, 283) x panel 9
__host__ __device__ constexpr int rg_panel(int part) { return part == 0 ? 0 : (part == 1 ? 4 : 9); }
__host__ __device__ constexpr int rg_steps(int part) { return part < 2 ? 16 : 8; }       // 16-deep k-steps
__host__ __device__ constexpr int rg_blocks(int part) { return part < 2 ? 2 : 1; }       // 32-row output blocks
__host__ __device__ constexpr int rg_pieces(int part) { return 2 * rg_steps(part) * rg_blocks(part); }
__host__ __device__ constexpr int rg_piece0(int part) { return part == 0 ? 0 : (part == 1 ? 64 : 128); }
static_assert(rg_piece0(2) + rg_pieces(2) == kRayGradPieces, "144 pieces per network");

// piece ((s * blocks + b) * 2 + part_hl) of a part: lane (i, h), half j = 64 W[act_feature(8 s + j, h)][column of row i of
// block b]; row i = (r & 3) + 8 (r >> 2) + 4 hh is register r of lane half hh in the D fragment
struct RgPackArgs {
  const float* w[2][kRgParts];
  unsigned* img[2];
};
__global__ void __launch_bounds__(256) raygrad_pack_kernel(RgPackArgs a) {
  const int piece = blockIdx.x, net = blockIdx.y;
  const int part = piece < 64 ? 0 : (piece < 128 ? 1 : 2);
  const int q = piece - rg_piece0(part);
  const int hl = q & 1;
  const int b = part < 2 ? (q >> 1) & 1 : 0;
  const int s = part < 2 ? q >> 2 : q >> 1;
  const int lane = threadIdx.x >> 2, word = threadIdx.x & 3;
  const int i = lane & 31, h = lane >> 5;
  const int hh = (i >> 2) & 1, r = (i & 3) + 4 * (i >> 3);
  const int col = part < 2 ? pecol(16 * b + r, hh) : dircol(r, hh);
  const int ld = part == 0 ? kPosCh : (part == 1 ? kPosCh + kWidth : kWidth + kDirCh);
  const int col0 = part == 2 ? kWidth : 0;
  float v[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int f = act_feature(8 * s + 2 * word + e, h);
    v[e] = col == kPad ? 0.0f : __fmul_rn(kRgScale, a.w[net][part][(int64_t)f * ld + col0 + col]);
  }
  _Float16 h0 = (_Float16)v[0], h1 = (_Float16)v[1];
  if (hl) {
    h0 = (_Float16)(v[0] - (float)h0);
    h1 = (_Float16)(v[1] - (float)h1);
  }
  a.img[net][(int64_t)piece * 256 + threadIdx.x] =
      (unsigned)__builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
}

template <int PART>
__device__ __forceinline__ void rg_part(const rg_u32x4* __restrict__ img, rg_u32x4* lds, const char* __restrict__ dpan,
                                        const float* __restrict__ pscale, int64_t n_groups, int64_t group, bool live, int m, int h,
                                        int lane, rg_f32x16* acc) {
  constexpr int panel = rg_panel(PART), steps = rg_steps(PART), nblk = rg_blocks(PART), pieces = rg_pieces(PART);
  __syncthreads();   // the part before this one has been read by every wave
  for (int i = threadIdx.x; i < pieces * 64; i += 256) lds[i] = img[rg_piece0(PART) * 64 + i];
  __syncthreads();
  if (!live) return;
  const char* blk0 = dpan + panel_offset_bytes(n_groups, panel) + group * panel_rows(panel) * kPanelRowBytes;
  rg_f32x16 p[nblk];
#pragma unroll
  for (int b = 0; b < nblk; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) p[b][r] = 0.0f;
#pragma unroll
  for (int s = 0; s < steps; ++s) {
    const int u = s & 1;
    // unit u of block s >> 1 as it lies: slot (2m + h) ^ 8u
    const rg_u32x4 g = *reinterpret_cast<const rg_u32x4*>(blk0 + s * 1024 + 16 * ((2 * m + h) ^ (8 * u)));
#pragma unroll
    for (int b = 0; b < nblk; ++b) {
      const rg_u32x4 ah = lds[((s * nblk + b) * 2 + 0) * 64 + lane], al = lds[((s * nblk + b) * 2 + 1) * 64 + lane];
      p[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(rg_h8, ah), __builtin_bit_cast(rg_h8, g), p[b], 0, 0, 0);
      p[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(rg_h8, al), __builtin_bit_cast(rg_h8, g), p[b], 0, 0, 0);
    }
  }
  // stored value x pscale = true gradient, and the weights were 64 w: two powers of two, exact
  const float ps = __fmul_rn(pscale[(int64_t)panel * n_groups * 32 + group * 32 + m], kRgInvScale);
#pragma unroll
  for (int b = 0; b < nblk; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = __fadd_rn(acc[b][r], __fmul_rn(p[b][r], ps));
}

// grid: ceil(P / 128) workgroups of 256 threads; P a multiple of 32 (a wave's point group is whole or absent)
__global__ void __launch_bounds__(256) raygrad_f16_kernel(const rg_u32x4* __restrict__ img, const char* __restrict__ dpan,
                                                          const float* __restrict__ pscale, const float* __restrict__ rays,
                                                          int ray_stride, const float* __restrict__ z, int64_t P, int N, int dir_term,
                                                          float* __restrict__ g_x, float* __restrict__ g_dv) {
  __shared__ rg_u32x4 lds[64 * 64];   // one part's A fragments: at most 64 pieces of 1 KiB
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = lane & 31, h = lane >> 5;
  const int64_t n_groups = (P + 127) / 128 * 4;
  const int64_t group = (int64_t)blockIdx.x * 4 + wave;
  const bool live = group * 32 < P;
  rg_f32x16 acc[3];   // g_pe registers 0..15, 16..31; g_de registers 0..15
#pragma unroll
  for (int b = 0; b < 3; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = 0.0f;
  rg_part<0>(img, lds, dpan, pscale, n_groups, group, live, m, h, lane, acc);
  rg_part<1>(img, lds, dpan, pscale, n_groups, group, live, m, h, lane, acc);
  if (dir_term) rg_part<2>(img, lds, dpan, pscale, n_groups, group, live, m, h, lane, acc + 2);   // grid-uniform
  if (!live) return;

  // the encoding's backward on the forward's own sin / cos
  const int64_t pc = group * 32 + m;
  float pe[32], de[16];
  encode_point<1>(rays, z, pc, N, ray_stride, h, pe, de);
  double gx[3], dv[3];
  gx[0] = h ? 0.0 : (double)acc[0][0];
  gx[1] = h ? 0.0 : (double)acc[0][1];
  gx[2] = h ? (double)acc[0][0] : 0.0;
#pragma unroll
  for (int f = 0; f < 5; ++f) {
    const double band = (double)(1u << (5 * h + f));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int ts = 2 + 6 * f + c, tc = ts + 3;
      const float gs = ts < 16 ? acc[0][ts & 15] : acc[1][ts & 15], gc = tc < 16 ? acc[0][tc & 15] : acc[1][tc & 15];
      gx[c] += band * ((double)gs * (double)pe[tc] - (double)gc * (double)pe[ts]);
    }
  }
  dv[0] = h ? 0.0 : (double)acc[2][0];
  dv[1] = h ? 0.0 : (double)acc[2][1];
  dv[2] = h ? (double)acc[2][0] : 0.0;
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const double band = (double)(1u << (2 * h + f));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int ts = 2 + 6 * f + c, tc = ts + 3;
      dv[c] += band * ((double)acc[2][ts] * (double)de[tc] - (double)acc[2][tc] * (double)de[ts]);
    }
  }
  // the point's other lane half holds the other bands: one addition, the same bits in both halves
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    gx[c] += __shfl_xor(gx[c], 32, 64);
    dv[c] += __shfl_xor(dv[c], 32, 64);
  }
  if (h == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) g_x[pc * 3 + c] = (float)gx[c];
  } else if (dir_term) {
#pragma unroll
    for (int c = 0; c < 3; ++c) g_dv[pc * 3 + c] = (float)dv[c];
  }
}

}  // namespace

int nsr::raygrad_f16_pack(hipStream_t st, const float* const* w_coarse, float* img_coarse, const float* const* w_fine,
                          float* img_fine) {
  if (!w_coarse || !w_fine || !img_coarse || !img_fine) return NSR_ERR_INVALID_ARG;
  RgPackArgs a{};
  const float* const* w[2] = {w_coarse, w_fine};
  for (int n = 0; n < 2; ++n) {
    a.w[n][0] = w[n][0];        // xyz_encoding_1.weight
    a.w[n][1] = w[n][8];        // xyz_encoding_5.weight
    a.w[n][2] = w[n][kDirW];    // dir_encoding.0.weight
    for (int p = 0; p < kRgParts; ++p)
      if (!a.w[n][p]) return NSR_ERR_INVALID_ARG;
  }
  a.img[0] = reinterpret_cast<unsigned*>(img_coarse);
  a.img[1] = reinterpret_cast<unsigned*>(img_fine);
  hipLaunchKernelGGL(raygrad_pack_kernel, dim3(kRayGradPieces, 2), dim3(256), 0, st, a);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

int nsr::raygrad_f16(hipStream_t st, const float* img, const char* dpan, const float* pscale, const float* rays, int ray_stride,
                     const float* z, int64_t R, int N, int stop_grad, float* g_x, float* g_dv, float* g_rays, int acc) {
  if (!img || !dpan || !pscale || !rays || !z || !g_x || !g_dv || !g_rays || !nsr_ray_stride_ok(ray_stride) || N < 1 || R < 0)
    return NSR_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(img) & 15) != 0 || (reinterpret_cast<uintptr_t>(dpan) & 15) != 0) return NSR_ERR_INVALID_ARG;
  const int64_t P = R * N;
  if (P % 32 != 0 || (P + 127) / 128 > 0x7fffffff) return NSR_ERR_UNSUPPORTED;
  if (R == 0) return NSR_OK;
  const int dir_term = stop_grad ? 0 : 1;
  hipLaunchKernelGGL(raygrad_f16_kernel, dim3((unsigned)((P + 127) / 128)), dim3(256), 0, st, reinterpret_cast<const rg_u32x4*>(img),
                     dpan, pscale, rays, ray_stride, z, P, N, dir_term, g_x, g_dv);
  NSR_CHECK_LAUNCH();
  // the direction term arrives back-propagated: three identity columns of a degree-0 encoding, whose kept row is never read
  return ray_grad(st, g_x, z, R, N, dir_term ? g_dv : nullptr, 3, g_dv, 3, 0, 0u, nullptr, g_rays, ray_stride, acc);
}
