// Input gradient of a stride-1 3 x 3 / pad 1 convolution of the refinement network's train-mode pair on the split-fp16 MFMA
// (include/nsr_refine.h: nsr_refine_train_backward_p at NSR_F16X3), without the dcol matrix:
//
//   dX[(img, y, x)][c] = sum over taps (ky, kx) and outputs n of dZ[(img, y + 1 - ky, x + 1 - kx)][n] W[n][c][ky][kx]
//
// is itself a 3 x 3 / pad 1 convolution of dZ (np columns, dense) with the flipped, transposed weight: under tap t' = (ty, tx)
// it reads dZ at (y + ty - 1, x + tx - 1), so t' = (2 - ky, 2 - kx).  refine_flip_pack_kernel writes that operand once per
// site, B'[c][t' np + n] = 2^6 W[n][c][ky][kx] as (hi, lo) fp16 halves (nsr_gemm.h: kSplitScale); refine_dgrad_kernel is the
// staged split-fp16 GEMM of nsr_gemm_f16.hip (128 x 128 tile, four waves of 64 x 64, K tiles of 32, fp32 A split while it is
// staged, v_mfma_f32_32x32x16_f16 x 3 per product, small terms first) with the gather fixed to stride 1 and ONE addition:
//
// the RANGE of A.  dZ is of order 1e-6 and below at the reference's batch: split into fp16 as it is, its hi half is subnormal
// and its lo half is gone.  The kernels that write dZ leave the float bits of max |dZ| in a device word (integer atomicMax on
// the bit pattern: order-independent); this kernel derives a power of two from it in its prologue (max |dZ| -> [2^13, 2^14),
// the convention of nsr_wgrad_f16.hip), multiplies A by it while staging (exact) and removes it, with the weights' 2^6, in
// the epilogue.  max = 0 (or NaN) -> scale 1: zeros give zeros, non-finite values travel through the fp16 halves as they are.
//
// A kernel of its own, not a template flag of gemm_f16x3_kernel: the instantiations the eval path launches stay what they are.
#include "nsr_refine_train_work.h"
#include "nsr_gemm.h"
#include "nsr_gemm_epilogue.h"

namespace nsr {
namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kTM = 128, kTN = 128, kTK = 32, kLd = kTK + 8;     // LDS rows padded by 8 halves (nsr_gemm_f16.hip)
constexpr int kArr = kTM * kLd;

struct DgradArgs {
  const float* dz; int np;                 // (n_img H W, np), dense; np % 32 == 0
  const unsigned short *Bh, *Bl;           // (cin, 9 np) halves each
  float* dst; int64_t ld; int cin;         // rows (img, y, x), row stride ld floats, cin columns written; cin % 128 == 0
  int n_img, H, W;
  const unsigned* max_bits;
};

// staging row of a thread: eight lanes take rows {r, r + 4} (nsr_gemm_f16.hip, stage_row<4>)
__device__ __forceinline__ int stage_row4(int tid) {
  const int g8 = tid >> 3;
  return (g8 >> 2) * 8 + (g8 & 3) + 4 * ((tid >> 2) & 1);
}

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
refine_dgrad_kernel(DgradArgs a, int n_col_tiles) {
  __shared__ __attribute__((aligned(16))) _Float16 lds[4 * kArr];      // A hi | A lo | B hi | B lo
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1, li = lane & 31, h = lane >> 5;
  const int64_t bid = blockIdx.x;
  const int64_t m0 = (bid / n_col_tiles) * kTM;
  const int n0 = (int)(bid % n_col_tiles) * kTN;
  const int K = 9 * a.np, n_tiles = K / kTK;
  const int64_t per = (int64_t)a.H * a.W, M = (int64_t)a.n_img * per;

  // the range of A: a power of two that takes max |dZ| into [2^13, 2^14), and what removes it and the weights' 2^6
  const float amax = __uint_as_float(*a.max_bits);
  int eS = 13 - ((int)((__float_as_uint(amax) >> 23) & 255u) - 127);
  eS = eS < -100 ? -100 : (eS > 100 ? 100 : eS);
  if (!(amax > 0.0f)) eS = 0;
  const float scale = __uint_as_float((unsigned)(127 + eS) << 23);
  const float unscale = __uint_as_float((unsigned)(127 - 6 - eS) << 23);

  f32x16 acc[2][2];
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[bi][bj][r] = 0.0f;

  // ---- staging assignment.  A: 4 x (row = (tid >> 3) + 32 i, float4 column tid & 7); B: 2 x 2 x (row = stage_row4 + 64 i,
  // 8-half chunk tid & 3)
  const int c4 = tid & 7, c8 = tid & 3, ar0 = tid >> 3, br0 = stage_row4(tid);
  int img[4], oy[4], ox[4];
  int64_t arow[4];                                       // element offset of the source pixel under the tap at hand; -1: padding
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int64_t m = m0 + ar0 + 32 * i;
    m = m < M ? m : M - 1;                               // rows past M: computed on the last row, never stored
    const int64_t pix = m % per;
    img[i] = (int)(m / per);
    oy[i] = (int)(pix / a.W);
    ox[i] = (int)(pix % a.W);
    arow[i] = 0;
  }
  const unsigned short* bh_row[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) bh_row[i] = a.Bh + (int64_t)(n0 + br0 + 64 * i) * K;     // n0 + 127 < cin: whole column tiles
  const int64_t b_lo = a.Bl - a.Bh;
  f32x4 sa[4];
  u32x4 sbh[2], sbl[2];
  auto load = [&](int t) {
    const int k0 = t * kTK, cbase = k0 % a.np;
    if (cbase == 0) {                                    // the K tile enters the next tap (a tile never straddles one)
      const int tap = k0 / a.np, ty = tap / 3, tx = tap % 3;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int iy = oy[i] + ty - 1, ix = ox[i] + tx - 1;
        arow[i] = (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) ? (((int64_t)img[i] * a.H + iy) * a.W + ix) * a.np : -1;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      sa[i] = arow[i] >= 0 ? *reinterpret_cast<const f32x4*>(a.dz + arow[i] + cbase + 4 * c4) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const unsigned short* q = bh_row[i] + k0 + 8 * c8;
      sbh[i] = *reinterpret_cast<const u32x4*>(q);
      sbl[i] = *reinterpret_cast<const u32x4*>(q + b_lo);
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int off = (ar0 + 32 * i) * kLd + 4 * c4;
      h4 hi, lo;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v = sa[i][e] * scale;
        const _Float16 x = (_Float16)v;
        hi[e] = x;
        lo[e] = (_Float16)(v - (float)x);
      }
      *reinterpret_cast<h4*>(lds + off) = hi;
      *reinterpret_cast<h4*>(lds + kArr + off) = lo;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int off = (br0 + 64 * i) * kLd + 8 * c8;
      *reinterpret_cast<u32x4*>(lds + 2 * kArr + off) = sbh[i];
      *reinterpret_cast<u32x4*>(lds + 3 * kArr + off) = sbl[i];
    }
  };

  load(0);
  for (int t = 0; t < n_tiles; ++t) {
    store();
    __syncthreads();
    if (t + 1 < n_tiles) load(t + 1);
    const _Float16* ap = lds + (64 * wm + li) * kLd + 8 * h;
    const _Float16* bp = lds + 2 * kArr + (64 * wn + li) * kLd + 8 * h;
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < kTK / 16; ++s) {
      h8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        ah[b] = *reinterpret_cast<const h8*>(ap + 32 * b * kLd + 16 * s);
        al[b] = *reinterpret_cast<const h8*>(ap + kArr + 32 * b * kLd + 16 * s);
        bh[b] = *reinterpret_cast<const h8*>(bp + 32 * b * kLd + 16 * s);
        bl[b] = *reinterpret_cast<const h8*>(bp + kArr + 32 * b * kLd + 16 * s);
      }
#pragma unroll
      for (int bj = 0; bj < 2; ++bj)
#pragma unroll
        for (int bi = 0; bi < 2; ++bi) {
          acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[bi], bh[bj], acc[bi][bj], 0, 0, 0);   // small terms first
          acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[bi], bl[bj], acc[bi][bj], 0, 0, 0);
          acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[bi], bh[bj], acc[bi][bj], 0, 0, 0);
        }
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
  }
  // lane (column li, half h) of block (bi, bj) holds rows 8 (r >> 2) + 4 h + (r & 3) (nsr_gemm_epilogue.h)
#pragma unroll
  for (int bj = 0; bj < 2; ++bj) {
    const int n = n0 + 64 * wn + 32 * bj + li;
#pragma unroll
    for (int bi = 0; bi < 2; ++bi) {
      const int64_t mb = m0 + 64 * wm + 32 * bi + 4 * h;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t m = mb + 8 * (r >> 2) + (r & 3);
        if (m < M) a.dst[m * a.ld + n] = acc[bi][bj][r] * unscale;
      }
    }
  }
}

// B'[c][((2 - ky) * 3 + (2 - kx)) np + n] = 2^6 W[n][c][ky][kx] (W: the reference's (cout, cin, 3, 3)), zero for n >= cout:
// hi halves (cin x 9 np), then lo halves
__global__ void __launch_bounds__(256) refine_flip_pack_kernel(const float* __restrict__ w, int cin, int cout, int np,
                                                               unsigned short* __restrict__ dst) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nw = (int64_t)cin * 9 * np;
  if (idx >= nw) return;
  const int c = (int)(idx / (9 * np)), k = (int)(idx % (9 * np)), n = k % np, tap = 8 - k / np;
  const float v = n < cout ? kSplitScale * w[((int64_t)n * cin + c) * 9 + tap] : 0.0f;
  const _Float16 hi = (_Float16)v;
  const _Float16 lo = (_Float16)(v - (float)hi);
  dst[idx] = __builtin_bit_cast(unsigned short, hi);
  dst[nw + idx] = __builtin_bit_cast(unsigned short, lo);
}

// The nearest x2 upsample backwards, gather form: source pixel (img, sy, sx), channel quad c sums the 2 x 2 block of
// src (n_img, 2 Hs, 2 Ws, C dense) it was copied to, in the fixed order ((0, 0) + (0, 1)) + (1, 0)) + (1, 1), and stores
// the sum at dst[(img, sy, sx)][c] (row stride ld)
__global__ void __launch_bounds__(256) refine_fold2x2_kernel(const float* __restrict__ src, int C, int n_img, int Hs, int Ws,
                                                             float* __restrict__ dst, int64_t ld) {
  const int q = C / 4;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)n_img * Hs * Ws * q) return;
  const int c = (int)(idx % q) * 4;
  const int64_t px = idx / q;
  const int sx = (int)(px % Ws), sy = (int)((px / Ws) % Hs);
  const int64_t img = px / ((int64_t)Ws * Hs);
  const float* p = src + (((img * 2 * Hs + 2 * sy) * 2 * Ws) + 2 * sx) * C + c;
  const int64_t down = (int64_t)2 * Ws * C;
  const float4 t00 = *reinterpret_cast<const float4*>(p), t01 = *reinterpret_cast<const float4*>(p + C);
  const float4 t10 = *reinterpret_cast<const float4*>(p + down), t11 = *reinterpret_cast<const float4*>(p + down + C);
  *reinterpret_cast<float4*>(dst + px * ld + c) = make_float4(((t00.x + t01.x) + t10.x) + t11.x, ((t00.y + t01.y) + t10.y) + t11.y,
                                                              ((t00.z + t01.z) + t10.z) + t11.z, ((t00.w + t01.w) + t10.w) + t11.w);
}

inline dim3 blocks(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

int refine_flip_pack(hipStream_t st, const float* w, int cin, int cout, int np, unsigned short* dst) {
  hipLaunchKernelGGL(refine_flip_pack_kernel, blocks((int64_t)cin * 9 * np), dim3(256), 0, st, w, cin, cout, np, dst);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

int refine_dgrad_f16x3(hipStream_t st, const float* dz, int np, const unsigned short* packed, int cin, int n_img, int H, int W,
                       const unsigned* max_bits, float* dst, int64_t ld) {
  if ((cin % kTN) != 0 || (np % kTK) != 0) return NSR_ERR_UNSUPPORTED;
  DgradArgs a{};
  a.dz = dz; a.np = np; a.Bh = packed; a.Bl = packed + (int64_t)cin * 9 * np; a.dst = dst; a.ld = ld; a.cin = cin;
  a.n_img = n_img; a.H = H; a.W = W; a.max_bits = max_bits;
  const int64_t M = (int64_t)n_img * H * W, row_tiles = (M + kTM - 1) / kTM;
  const int n_col_tiles = cin / kTN;
  if (row_tiles * n_col_tiles >= ((int64_t)1 << 31)) return NSR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(refine_dgrad_kernel, dim3((unsigned)(row_tiles * n_col_tiles)), dim3(256), 0, st, a, n_col_tiles);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

int refine_fold2x2(hipStream_t st, const float* src, int C, int n_img, int Hs, int Ws, float* dst, int64_t ld) {
  hipLaunchKernelGGL(refine_fold2x2_kernel, blocks((int64_t)n_img * Hs * Ws * (C / 4)), dim3(256), 0, st, src, C, n_img, Hs, Ws, dst, ld);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

int refine_conv_f16x3(hipStream_t st, const float* src, int64_t lds, int cin, int n_img, int Hs, int Ws, int stride, int up,
                      const float* packed, int np, int cout, int act, float* dst, int64_t ld) {
  const int Hin = up ? 2 * Hs : Hs, Win = up ? 2 * Ws : Ws, Ho = (Hin - 1) / stride + 1, Wo = (Win - 1) / stride + 1;
  const int64_t kp = (int64_t)9 * cin;
  GemmF16Args a{};
  a.g.A = src; a.g.lda = lds; a.g.C = dst; a.g.ldc = ld; a.g.bias = packed + (int64_t)np * kp;
  a.g.M = (int64_t)n_img * Ho * Wo; a.g.N = np; a.g.K = kp; a.g.n_valid = cout; a.g.act = act; a.g.splits = 1;
  a.g.acc_scale = kSplitInvScale;
  a.Bh = reinterpret_cast<const unsigned short*>(packed);
  a.Bl = a.Bh + (int64_t)np * kp;
  a.ldbh = kp;
  a.conv = ConvGather{cin, Hs, Ws, Ho, Wo, stride, up};
  if (gemm_f16x3_route(a) != kRouteStagedF32A) return NSR_ERR_UNSUPPORTED;     // cin % 32 == 0: the one route of fp32 A
  return gemm_f16x3(a, st);
}

}  // namespace nsr
