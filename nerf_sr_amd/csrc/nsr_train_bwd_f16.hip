// The gradient products of the layer-by-layer training network on the split-fp16 MFMA (precision NSR_F16X3_GEMM_BWD,
// include/nsr_train.h; nsr_train_gemm.hip's lin_dgrad / lin_wgrad launch them when the pack holds the transposed halves):
// refine_dgrad_kernel (nsr_refine_dgrad_f16.hip) and refine_wgrad_kernel (nsr_refine_wgrad_f16.hip) in their plain-matrix
// form.  Every product is three v_mfma_f32_32x32x16_f16 per k step, small terms first (lo hi, hi lo, hi hi), fp32 accumulation:
// products exact to ~2^-21.  Kernels of their own, not template flags of gemm_f16x3_kernel: the instantiations the forward and
// the eval path launch stay what they are.
//
// INPUT GRADIENT  dx (P, N) = (dy (P, K) w[:, 0 : N]) * [mask > 0], w (K rows) in the nn.Linear layout.  The weight operand is a
// transposed split copy wt (N rows of K halves, hi and lo, pre-scaled by 2^6: kSplitScale) that prepare_weights_t makes once
// per call (split_f16_t), so the kernel is the staged GEMM of nsr_gemm_f16.hip: 128 x 128 tile, four waves of 64 x 64, K tiles
// of 32, fp32 A split into (hi, lo) while it is staged.
//   RANGE of dy: gradients are of order 1e-6 and below and differ by orders of magnitude from point to point.  The scale is
//   PER ROW: the workgroup scans its 128 rows of dy over the K columns it reads (integer max on the bit pattern of |v|), and a
//   row's power of two takes its own max into [2^13, 2^14) (nsr_wgrad_f16.hip's convention; clamped to 2^+-100; max = 0 or NaN
//   -> 1; non-finite values travel through the halves as they are).  It is applied while staging and removed per row in the
//   epilogue together with the 2^-6, both exact; the contraction runs along the row, so the factor leaves the sum exactly.
//   PROMISE: a row of dx depends on that row of dy, its mask row and the weights only -- not on P, not on its tile mates, not
//   on ray_chunk.  (The k order of a row's accumulation is fixed by K alone; nothing is shared between rows but the weights.)
//   The epilogue keeps lin_dgrad's contract: the optional mask with its own row stride, the optional per-row-tile column sums
//   (128-row tiles, the layout tile_sums reads), any P >= 1 (rows past P are computed on the last row and never stored).  It
//   may also raise a device word with the float bits of the largest |dx| written (integer atomicMax: order-independent) --
//   the range word of the weight gradient that reads dx as its dy.
//
// WEIGHT GRADIENT  partial[z] (M x N) = sum over the points p of slice z of dy[p][0 : M) x[p][0 : N)^T, both operands row-major
// fp32 with their own row strides.  One workgroup owns a 128 x 128 tile and one slice; per K tile of 32 points both operands are
// split into fp16 (hi, lo) while staged.  Both are contraction-major in memory ([point][feature]); the MFMA wants a lane's eight
// k values (points) side by side, so a thread loads a 4-point x 4-feature block (four float4 of consecutive points), transposes
// it in registers and stores four 8-byte pieces into [feature][32 + 8 pad] planes -- the input gradient's LDS layout, read by the
// same plain 16-byte fragment loads (refine_wgrad_kernel transposes in the LDS read instead, ds_read_b64_tr_b16; this unit has
// no need of nsr_lds_dma.h).  The contraction runs over the points, so the scale of dy is ONE power of two per matrix, from the float
// bits of the matrix's largest |dy| in a device word (max -> [2^13, 2^14), same rules), applied while staging, removed in the
// epilogue.  Slices: bwd_f16_slice_len(P, splits) points each, a function of P alone (splits = n_splits(P)); every slice is
// written (an empty one as zeros), in lin_wgrad's (M x N, ld N) layout at partial + z * stride; reduce_place adds them in
// order.  No float atomics anywhere: two identical calls give identical bits.
#include "nsr_train_work.h"
#include "nsr_gemm.h"
#include "nsr_gemm_epilogue.h"

namespace nsr {
namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kTM = 128, kTN = 128, kTK = 32;

// the power-of-two exponent that takes a magnitude with float bits `bits` into [2^13, 2^14)
__device__ __forceinline__ int range_exp(unsigned bits) {
  const float amax = __uint_as_float(bits);
  int eS = 13 - ((int)((bits >> 23) & 255u) - 127);
  eS = eS < -100 ? -100 : (eS > 100 ? 100 : eS);
  if (!(amax > 0.0f)) eS = 0;                              // zero or NaN
  return eS;
}
__device__ __forceinline__ float pow2f(int e) { return __uint_as_float((unsigned)(127 + e) << 23); }
__device__ __forceinline__ unsigned abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }
__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }

// ---- input gradient ------------------------------------------------------------------------------------------------------
constexpr int kLd = kTK + 8;                 // LDS rows padded by 8 halves (nsr_gemm_f16.hip)
constexpr int kArr = kTM * kLd;

struct DgArgs {
  const float* dy; int64_t lddy; int K;        // (P, K), K % 32 == 0
  const unsigned short *Bh, *Bl; int ldb;      // (N, K) halves each, row stride ldb
  const float* mask; int64_t ldm;
  float* dx; int64_t lddx;
  int64_t P; int N;                            // N % 32 == 0
  float* col_tiles;                            // may be null: (ceil(P / 128), N)
  unsigned* out_max;                           // may be null
};

// staging row of a thread: eight lanes take rows {r, r + 4} (nsr_gemm_f16.hip, stage_row<4>)
__device__ __forceinline__ int stage_row4(int tid) {
  const int g8 = tid >> 3;
  return (g8 >> 2) * 8 + (g8 & 3) + 4 * ((tid >> 2) & 1);
}

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) train_dgrad_kernel(DgArgs a, int n_col_tiles) {
  __shared__ __attribute__((aligned(16))) _Float16 lds[4 * kArr];      // A hi | A lo | B hi | B lo
  __shared__ float row_un[kTM];                                        // per row: what removes its scale and the weights' 2^6
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1, li = lane & 31, h = lane >> 5;
  const int64_t bid = blockIdx.x;
  const int64_t m0 = (bid / n_col_tiles) * kTM;
  const int n0 = (int)(bid % n_col_tiles) * kTN;
  const int n_tiles = a.K / kTK;

  // ---- staging assignment.  A: 4 x (row = (tid >> 3) + 32 i, float4 column tid & 7); B: 2 x (row = stage_row4 + 64 i,
  // 8-half chunk tid & 3)
  const int c4 = tid & 7, c8 = tid & 3, ar0 = tid >> 3, br0 = stage_row4(tid);
  const float* arow[4];
  float scale[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int64_t m = m0 + ar0 + 32 * i;
    m = m < a.P ? m : a.P - 1;                             // rows past P: computed on the last row, never stored
    arow[i] = a.dy + m * a.lddy + 4 * c4;
  }
  // the range of each row: the eight lanes of a row scan its K columns; integer max of the bit patterns of |v|
  {
    unsigned mx[4] = {0u, 0u, 0u, 0u};
    for (int t = 0; t < n_tiles; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(arow[i] + t * kTK);
        mx[i] = umax(umax(mx[i], umax(abs_bits(v[0]), abs_bits(v[1]))), umax(abs_bits(v[2]), abs_bits(v[3])));
      }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) mx[i] = umax(mx[i], (unsigned)__shfl_xor((int)mx[i], o, 64));
      const int eS = range_exp(mx[i]);
      scale[i] = pow2f(eS);
      if (c4 == 0) row_un[ar0 + 32 * i] = pow2f(-6 - eS);
    }
  }
  // column blocks of 32 past N: not multiplied, not stored (wave-uniform)
  bool col_on[2];
#pragma unroll
  for (int bj = 0; bj < 2; ++bj) col_on[bj] = n0 + 64 * wn + 32 * bj < a.N;

  f32x16 acc[2][2];
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[bi][bj][r] = 0.0f;

  const unsigned short* bh_row[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int n = n0 + br0 + 64 * i;
    n = n < a.N ? n : a.N - 1;                             // rows past N: read in range, their columns are never stored
    bh_row[i] = a.Bh + (int64_t)n * a.ldb + 8 * c8;
  }
  const int64_t b_lo = a.Bl - a.Bh;
  f32x4 sa[4];
  u32x4 sbh[2], sbl[2];
  auto load = [&](int t) {
    const int k0 = t * kTK;
#pragma unroll
    for (int i = 0; i < 4; ++i) sa[i] = *reinterpret_cast<const f32x4*>(arow[i] + k0);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const unsigned short* q = bh_row[i] + k0;
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
        const float v = sa[i][e] * scale[i];
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
      for (int bj = 0; bj < 2; ++bj) {
        if (!col_on[bj]) continue;
#pragma unroll
        for (int bi = 0; bi < 2; ++bi) {
          acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[bi], bh[bj], acc[bi][bj], 0, 0, 0);   // small terms first
          acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[bi], bl[bj], acc[bi][bj], 0, 0, 0);
          acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[bi], bh[bj], acc[bi][bj], 0, 0, 0);
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
  }
  // lane (column li, half h) of block (bi, bj) holds rows 8 (r >> 2) + 4 h + (r & 3) (nsr_gemm_epilogue.h)
  float csum[2] = {0.0f, 0.0f};
  unsigned omax = 0u;
#pragma unroll
  for (int bj = 0; bj < 2; ++bj) {
    const int n = n0 + 64 * wn + 32 * bj + li;
    if (!col_on[bj]) continue;
#pragma unroll
    for (int bi = 0; bi < 2; ++bi) {
      const int rb = 64 * wm + 32 * bi + 4 * h;
      const int64_t mb = m0 + rb;
      float mk[16];
      if (a.mask) {                                        // all 16 loads in flight before the first use
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int64_t m = mb + 8 * (r >> 2) + (r & 3);
          m = m < a.P ? m : a.P - 1;
          mk[r] = a.mask[m * a.ldm + n];
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ro = 8 * (r >> 2) + (r & 3);
        const int64_t m = mb + ro;
        float x = acc[bi][bj][r] * row_un[rb + ro];
        if (a.mask) x = mk[r] > 0.0f ? x : 0.0f;
        if (m < a.P) {
          a.dx[m * a.lddx + n] = x;
          csum[bj] += x;
          omax = umax(omax, abs_bits(x));
        }
      }
    }
  }
  if (a.col_tiles) {   // column sums of this 128-row tile: halves by shuffle, the two row-waves through LDS (gemm_epilogue)
    float* red = reinterpret_cast<float*>(lds);            // the K loop is over (its last statement is a barrier)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      const float s = csum[bj] + __shfl_xor(csum[bj], 32, 64);
      if (h == 0) red[wm * kTN + 64 * wn + 32 * bj + li] = s;
    }
    __syncthreads();
    if (tid < kTN && n0 + tid < a.N) a.col_tiles[(m0 / kTM) * a.N + n0 + tid] = red[tid] + red[kTN + tid];
  }
  if (a.out_max) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) omax = umax(omax, (unsigned)__shfl_xor((int)omax, o, 64));
    if (lane == 0 && omax != 0u) atomicMax(a.out_max, omax);
  }
}

// ---- weight gradient -----------------------------------------------------------------------------------------------------
constexpr int kPlane = kTM * kLd;            // halves per plane [feature][32 points + 8 pad]: dy hi | dy lo | x hi | x lo

struct WgArgs {
  const float* dy; int64_t lddy; int M;        // (P, M), M % 32 == 0
  const float* x; int64_t ldx; int N;          // (P, N), N % 32 == 0
  int64_t P, slice_len;
  const unsigned* max_bits;
  float* part; int64_t stride;                 // slice z: part + z stride, (M, N) with row stride N
};

// grid: x = column tile (128 columns of x), y = row tile (128 columns of dy), z = slice
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) train_wgrad_kernel(WgArgs a) {
  __shared__ __attribute__((aligned(16))) _Float16 lds[4 * kPlane];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1, li = lane & 31, h = lane >> 5;
  const int c0 = (int)blockIdx.x * kTN, n0 = (int)blockIdx.y * kTM;
  const int64_t k0 = (int64_t)blockIdx.z * a.slice_len;
  const int64_t k1 = k0 + a.slice_len < a.P ? k0 + a.slice_len : a.P;
  const int n_tiles = k1 > k0 ? (int)((k1 - k0 + kTK - 1) / kTK) : 0;       // a slice behind the last point writes zeros

  // the range of dy: a power of two that takes the matrix's max |dy| into [2^13, 2^14), and what removes it
  const int eS = range_exp(*a.max_bits);
  const float scale = pow2f(eS), unscale = pow2f(-eS);

  // 32 x 32 blocks past M / N: not multiplied, not stored (wave-uniform)
  bool row_on[2], col_on[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    row_on[b] = n0 + 64 * wm + 32 * b < a.M;
    col_on[b] = c0 + 64 * wn + 32 * b < a.N;
  }

  f32x16 acc[2][2];
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[bi][bj][r] = 0.0f;

  // ---- staging assignment, both operands: the 4 x 4 block of points 4 (tid & 7) + i of the K tile, float4 column tid >> 3.
  // Eight neighbouring lanes take eight point blocks of one column group: their 8-byte LDS stores fill 64 contiguous bytes of a
  // row (rows of 80 B: a half-wave's four column groups start 16 banks apart), and a global load covers 128 B per point row
  const int c4 = tid >> 3, pr0 = tid & 7;
  const bool dy_col = n0 + 4 * c4 < a.M, x_col = c0 + 4 * c4 < a.N;       // the tile's columns past the matrix: zeros
  f32x4 sz[4], sx[4];
  auto load = [&](int t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t k = k0 + (int64_t)t * kTK + 4 * pr0 + i;
      sz[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      sx[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      if (k < k1) {                                        // points past the slice: zeros in both operands
        if (dy_col) sz[i] = *reinterpret_cast<const f32x4*>(a.dy + k * a.lddy + n0 + 4 * c4);
        if (x_col) sx[i] = *reinterpret_cast<const f32x4*>(a.x + k * a.ldx + c0 + 4 * c4);
      }
    }
  };
  auto store = [&]() {   // feature 4 c4 + e, points 4 pr0 .. 4 pr0 + 3: the block transposed in registers
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int off = (4 * c4 + e) * kLd + 4 * pr0;
      h4 zh, zl, xh, xl;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float v = sz[i][e] * scale;
        const _Float16 p = (_Float16)v;
        zh[i] = p;
        zl[i] = (_Float16)(v - (float)p);
        const float u = sx[i][e];
        const _Float16 q = (_Float16)u;
        xh[i] = q;
        xl[i] = (_Float16)(u - (float)q);
      }
      *reinterpret_cast<h4*>(lds + off) = zh;
      *reinterpret_cast<h4*>(lds + kPlane + off) = zl;
      *reinterpret_cast<h4*>(lds + 2 * kPlane + off) = xh;
      *reinterpret_cast<h4*>(lds + 3 * kPlane + off) = xl;
    }
  };
  // lane (li, h) of a wave reads row li of its blocks, points 16 s + 8 h .. + 7 (the input gradient's fragment loads)
  const _Float16* ap = lds + (64 * wm + li) * kLd + 8 * h;
  const _Float16* bp = lds + 2 * kPlane + (64 * wn + li) * kLd + 8 * h;

  if (n_tiles > 0) load(0);
  for (int t = 0; t < n_tiles; ++t) {
    store();
    __syncthreads();
    if (t + 1 < n_tiles) load(t + 1);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < kTK / 16; ++s) {
      h8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        ah[b] = *reinterpret_cast<const h8*>(ap + 32 * b * kLd + 16 * s);
        al[b] = *reinterpret_cast<const h8*>(ap + kPlane + 32 * b * kLd + 16 * s);
        bh[b] = *reinterpret_cast<const h8*>(bp + 32 * b * kLd + 16 * s);
        bl[b] = *reinterpret_cast<const h8*>(bp + kPlane + 32 * b * kLd + 16 * s);
      }
#pragma unroll
      for (int bj = 0; bj < 2; ++bj)
#pragma unroll
        for (int bi = 0; bi < 2; ++bi) {
          if (!row_on[bi] || !col_on[bj]) continue;
          acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[bi], bh[bj], acc[bi][bj], 0, 0, 0);   // small terms first
          acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[bi], bl[bj], acc[bi][bj], 0, 0, 0);
          acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[bi], bh[bj], acc[bi][bj], 0, 0, 0);
        }
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
  }
  // lane (column li, half h) of block (bi, bj) holds rows 8 (r >> 2) + 4 h + (r & 3) (nsr_gemm_epilogue.h)
  float* C = a.part + (int64_t)blockIdx.z * a.stride;
#pragma unroll
  for (int bj = 0; bj < 2; ++bj) {
    const int c = c0 + 64 * wn + 32 * bj + li;
    if (!col_on[bj]) continue;
#pragma unroll
    for (int bi = 0; bi < 2; ++bi) {
      if (!row_on[bi]) continue;
      const int nb = n0 + 64 * wm + 32 * bi + 4 * h;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = nb + 8 * (r >> 2) + (r & 3);
        C[(int64_t)n * a.N + c] = acc[bi][bj][r] * unscale;
      }
    }
  }
}

// ---- the operands' helpers ------------------------------------------------------------------------------------------------
// hi[c * rows + r] = fp16(v), lo[...] = fp16(v - hi), v = 2^6 w[r * ldw + c]: the transposed split copy of a (rows x cols) matrix.
// One workgroup per 32 x 32 tile, through LDS (33 floats per row): the reads run along a row of w, the stores along a row of the
// copy, both contiguous; thread (tx = tid & 31, ty = tid >> 5) takes four of the tile's elements each way
__global__ void __launch_bounds__(256) split_f16_t_kernel(const float* __restrict__ w, int rows, int cols, int ldw,
                                                          unsigned short* __restrict__ hi, unsigned short* __restrict__ lo) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int r0 = (int)blockIdx.y * 32, c0 = (int)blockIdx.x * 32;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + ty + 8 * i, c = c0 + tx;
    tile[ty + 8 * i][tx] = (r < rows && c < cols) ? w[(int64_t)r * ldw + c] : 0.0f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + ty + 8 * i, r = r0 + tx;
    if (c >= cols || r >= rows) continue;
    const float v = kSplitScale * tile[tx][ty + 8 * i];
    const _Float16 x = (_Float16)v;
    const _Float16 y = (_Float16)(v - (float)x);
    const int64_t idx = (int64_t)c * rows + r;
    hi[idx] = __builtin_bit_cast(unsigned short, x);
    lo[idx] = __builtin_bit_cast(unsigned short, y);
  }
}

// *word = max(*word, float bits of the largest |src[p * ld + col0 + c]|, p < P, c < cols): integer max, order-independent
constexpr int kAbsBlocks = 256;
__global__ void __launch_bounds__(256) absmax_bits_kernel(const float* __restrict__ src, int64_t ld, int64_t P, int col0, int cols,
                                                          unsigned* __restrict__ word) {
  unsigned m = 0u;
  const int64_t n = P * cols;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)kAbsBlocks * 256)
    m = umax(m, abs_bits(src[(i / cols) * ld + col0 + (int)(i % cols)]));
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) m = umax(m, (unsigned)__shfl_xor((int)m, o, 64));
  if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(word, m);
}

}  // namespace

int split_f16_t(hipStream_t st, const float* w, int rows, int cols, int ldw, unsigned short* hi, unsigned short* lo) {
  const int64_t n = (int64_t)rows * cols;
  if (n == 0) return NSR_OK;
  hipLaunchKernelGGL(split_f16_t_kernel, dim3((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32)), dim3(256), 0, st, w, rows, cols,
                     ldw, hi, lo);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

int absmax_bits(hipStream_t st, const float* src, int64_t ld, int64_t P, int col0, int cols, unsigned* word) {
  if (P <= 0 || cols <= 0) return NSR_OK;
  hipLaunchKernelGGL(absmax_bits_kernel, dim3(kAbsBlocks), dim3(256), 0, st, src, ld, P, col0, cols, word);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

int dgrad_f16x3(hipStream_t st, const float* dy, int64_t lddy, int K, const unsigned short* wt_hi, const unsigned short* wt_lo,
                int ldwt, const float* mask, int64_t ldm, float* dx, int64_t lddx, int64_t P, int N, float* col_tiles,
                unsigned* out_max) {
  if (K < kTK || (K % kTK) != 0 || N < 32 || (N % 32) != 0 || (ldwt % 8) != 0 || (lddy % 4) != 0) return NSR_ERR_UNSUPPORTED;
  if (P <= 0) return NSR_OK;
  DgArgs a{};
  a.dy = dy; a.lddy = lddy; a.K = K; a.Bh = wt_hi; a.Bl = wt_lo; a.ldb = ldwt; a.mask = mask; a.ldm = ldm;
  a.dx = dx; a.lddx = lddx; a.P = P; a.N = N; a.col_tiles = col_tiles; a.out_max = out_max;
  const int64_t row_tiles = (P + kTM - 1) / kTM;
  const int n_col_tiles = (N + kTN - 1) / kTN;
  if (row_tiles * n_col_tiles >= ((int64_t)1 << 31)) return NSR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(train_dgrad_kernel, dim3((unsigned)(row_tiles * n_col_tiles)), dim3(256), 0, st, a, n_col_tiles);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

int64_t bwd_f16_slice_len(int64_t P, int splits) {
  const int64_t groups = (P + kTK - 1) / kTK;
  return (groups + splits - 1) / splits * kTK;
}

int wgrad_f16x3(hipStream_t st, const float* dy, int64_t lddy, int M, const float* x, int64_t ldx, int N, int64_t P,
                const unsigned* max_bits, float* partial, int splits, int64_t stride) {
  if (M < 32 || (M % 32) != 0 || N < 32 || (N % 32) != 0 || (lddy % 4) != 0 || (ldx % 4) != 0 || splits < 1 || splits > 65535 ||
      !max_bits)
    return NSR_ERR_UNSUPPORTED;
  if (P <= 0) return NSR_OK;
  WgArgs a{};
  a.dy = dy; a.lddy = lddy; a.M = M; a.x = x; a.ldx = ldx; a.N = N; a.P = P; a.slice_len = bwd_f16_slice_len(P, splits);
  a.max_bits = max_bits; a.part = partial; a.stride = stride;
  hipLaunchKernelGGL(train_wgrad_kernel, dim3((unsigned)((N + kTN - 1) / kTN), (unsigned)((M + kTM - 1) / kTM), (unsigned)splits),
                     dim3(256), 0, st, a);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

}  // namespace nsr
