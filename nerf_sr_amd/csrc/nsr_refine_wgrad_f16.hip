// Weight gradient of a 3 x 3 / pad 1 convolution of the refinement network's train-mode pair on the split-fp16 MFMA, without
// the col matrix (include/nsr_refine.h: nsr_refine_train_backward_w, weight_grad = NSR_F16X3):
//
//   dW[n][c][ky][kx] = sum over the output pixels (b, y, x) of dZ[(b, y, x)][n] X[(b, s y + ky - 1, s x + kx - 1)][c]
//
// (zero padding; X read through the nearest x2 upsample where the site has one) is a GEMM with M = cout, N = 9 cin (tap-major)
// and K = the output pixels of the call, BOTH operands contraction-major: dZ is (pixels x np) and X is NHWC.  One workgroup
// owns a 128 (cout) x 128 (one tap, 128 input channels) tile of dW and one SLICE of the pixels.  Per K tile of 32 pixels it
// stages the 32 dZ rows and the 32 tap-shifted input rows (the gather of nsr_gemm_f16.hip's ConvGather, restated for one tap)
// as fp16 (hi, lo) planes [pixel][128 + 32 pad], split from fp32 on the way (refine_dgrad_kernel's staging), and feeds
// v_mfma_f32_32x32x16_f16 through ds_read_b64_tr_b16 (tr16, nsr_lds_dma.h): a 16-lane group reads a block of 4 pixels x 16
// channels and lane i receives channel i of the 4 pixels, i.e. its half of an operand's k run.  Three MFMAs per product,
// small terms first (lo hi, hi lo, hi hi): the forward's and refine_dgrad_kernel's arithmetic.
//
// LDS rows of 160 halves (320 B): the four pixel rows of a transposed read start 64 B apart modulo the 256-B bank row, and the
// two 16-lane groups of a 32-lane half take 2 x 32 B side by side in each: 32 pieces on 32 distinct bank pairs.
//
// Range of dZ: the power of two 2^(13 - exponent(max |dZ|)) from the site's range word (refine_dgrad_kernel's derivation:
// clamped, max = 0 or NaN -> 1, non-finite values travel through the halves as they are), applied while staging and removed
// in the epilogue, both exact: scaling g_out by 2^k scales every weight gradient by exactly 2^k.
//
// Slices: refine_wgrad_slice_len() is a function of the SHAPE (cin, cout, pixels of the call) alone -- not of the CU count, not
// of img_chunk -- so identical calls give identical bits and the result does not depend on img_chunk.  Every workgroup writes
// its fp32 partial tile to the partial buffer (slice-major, rows x 9 cin, tap-major: what wgrad_reduce_kernel reads); the
// slices are added in order by refine_wgrad_reduce.  No float atomics.  Where the partial buffer cannot hold all slices, the
// site runs in passes of as many slices as fit (a function of the shape and the buffer size, which is a constant of the pair).
#include "nsr_refine_train_work.h"
#include "nsr_gemm.h"
#include "nsr_gemm_epilogue.h"
#include "nsr_lds_dma.h"

namespace nsr {
namespace {

using namespace dma;

constexpr int kTM = 128, kTN = 128, kTK = 32;
constexpr int kRow = kTM + 32;               // halves per LDS row (see the header)
constexpr int kPlane = kTK * kRow;           // halves per plane: dZ hi | dZ lo | X hi | X lo

struct WgArgs {
  const float* dz; int np, cout;           // (pixels, np) dense; rows n < cout of the product are stored
  const float* src; int64_t ld; int cin;   // NHWC source, row stride ld floats, channels [0, cin); cin % 128 == 0
  int n_img, Hs, Ws, Ho, Wo, stride, up;
  const unsigned* max_bits;
  float* part; int64_t slice_stride;       // partial of slice z (of this launch): part + z slice_stride, (rows, 9 cin)
  int64_t k_begin, slice_len, K;           // this launch's first pixel, pixels per slice, pixels of the call
};

// grid: x = column tile (tap, 128 input channels), y = row tile (128 outputs), z = slice
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) refine_wgrad_kernel(WgArgs a) {
  __shared__ __attribute__((aligned(16))) _Float16 lds[4 * kPlane];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1, li = lane & 31, h = lane >> 5;
  const int c_tiles = a.cin / kTN;
  const int tap = (int)blockIdx.x / c_tiles, c0 = ((int)blockIdx.x % c_tiles) * kTN, n0 = (int)blockIdx.y * kTM;
  const int ty = tap / 3, tx = tap % 3;
  const int64_t k0 = a.k_begin + (int64_t)blockIdx.z * a.slice_len;
  const int64_t k1 = k0 + a.slice_len < a.K ? k0 + a.slice_len : a.K;
  const int n_tiles = (int)((k1 - k0 + kTK - 1) / kTK);
  const int Hin = a.up ? 2 * a.Hs : a.Hs, Win = a.up ? 2 * a.Ws : a.Ws;
  const int64_t per = (int64_t)a.Ho * a.Wo;

  // the range of dZ: a power of two that takes max |dZ| into [2^13, 2^14), and what removes it (refine_dgrad_kernel)
  const float amax = __uint_as_float(*a.max_bits);
  int eS = 13 - ((int)((__float_as_uint(amax) >> 23) & 255u) - 127);
  eS = eS < -100 ? -100 : (eS > 100 ? 100 : eS);
  if (!(amax > 0.0f)) eS = 0;
  const float scale = __uint_as_float((unsigned)(127 + eS) << 23);
  const float unscale = __uint_as_float((unsigned)(127 - eS) << 23);

  f32x16 acc[2][2];
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[bi][bj][r] = 0.0f;

  // ---- staging assignment, both operands: 4 x (pixel row (tid >> 5) + 8 i of the K tile, float4 column tid & 31)
  const int c4 = tid & 31, pr0 = tid >> 5;
  const bool dz_col = n0 + 4 * c4 < a.np;            // dZ has np columns (np % 32 == 0): the tile's others are zero
  f32x4 sz[4], sx[4];
  auto load = [&](int t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t k = k0 + (int64_t)t * kTK + pr0 + 8 * i;
      sz[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      sx[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      if (k < k1) {                                  // pixels past the slice: zeros in both operands
        if (dz_col) sz[i] = *reinterpret_cast<const f32x4*>(a.dz + k * a.np + n0 + 4 * c4);
        const int64_t img = k / per, pix = k % per;
        const int oy = (int)(pix / a.Wo), ox = (int)(pix % a.Wo);
        const int iy = oy * a.stride + ty - 1, ix = ox * a.stride + tx - 1;
        if (iy >= 0 && iy < Hin && ix >= 0 && ix < Win) {
          const int sy = a.up ? iy >> 1 : iy, sxx = a.up ? ix >> 1 : ix;
          sx[i] = *reinterpret_cast<const f32x4*>(a.src + ((img * a.Hs + sy) * a.Ws + sxx) * a.ld + c0 + 4 * c4);
        }
      }
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int off = (pr0 + 8 * i) * kRow + 4 * c4;
      h4 zh, zl, xh, xl;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v = sz[i][e] * scale;
        const _Float16 p = (_Float16)v;
        zh[e] = p;
        zl[e] = (_Float16)(v - (float)p);
        const float u = sx[i][e];
        const _Float16 q = (_Float16)u;
        xh[e] = q;
        xl[e] = (_Float16)(u - (float)q);
      }
      *reinterpret_cast<h4*>(lds + off) = zh;
      *reinterpret_cast<h4*>(lds + kPlane + off) = zl;
      *reinterpret_cast<h4*>(lds + 2 * kPlane + off) = xh;
      *reinterpret_cast<h4*>(lds + 3 * kPlane + off) = xl;
    }
  };

  // ---- this lane's address for the transposing reads: its 16-lane group (columns 16 (g4 & 1) .., k half g4 >> 1 = h) reads
  // the block of pixels 16 s + 8 h + 4 t .. + 3; lane 4 q + p supplies pixel row q, columns 4 p .. 4 p + 3
  const int i16 = lane & 15, g4 = lane >> 4;
  const unsigned lds0 = lds_addr(lds);
  const unsigned rd = lds0 + 2u * (unsigned)((8 * h + (i16 >> 2)) * kRow + 16 * (g4 & 1) + 4 * (i16 & 3));
  const unsigned rd_a = rd + 2u * (unsigned)(64 * wm), rd_b = rd + 2u * (unsigned)(2 * kPlane + 64 * wn);
  auto frag = [&](unsigned base, int s) {            // rows 16 s + 8 h + 0 .. 7 of this lane's column
    const h4 lo4 = tr16(base + 2u * (unsigned)(16 * s * kRow)), hi4 = tr16(base + 2u * (unsigned)((16 * s + 4) * kRow));
    return __builtin_shufflevector(lo4, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
  };

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
        ah[b] = frag(rd_a + 2u * (unsigned)(32 * b), s);
        al[b] = frag(rd_a + 2u * (unsigned)(kPlane + 32 * b), s);
        bh[b] = frag(rd_b + 2u * (unsigned)(32 * b), s);
        bl[b] = frag(rd_b + 2u * (unsigned)(kPlane + 32 * b), s);
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
  // lane (column li, half h) of block (bi, bj) holds rows 8 (r >> 2) + 4 h + (r & 3) (nsr_gemm_epilogue.h); rows >= cout
  // (D.conv9: 3 of 128) are not stored
  float* C = a.part + (int64_t)blockIdx.z * a.slice_stride + (int64_t)tap * a.cin + c0;
  const int64_t kp = (int64_t)9 * a.cin;
#pragma unroll
  for (int bj = 0; bj < 2; ++bj) {
    const int c = 64 * wn + 32 * bj + li;
#pragma unroll
    for (int bi = 0; bi < 2; ++bi) {
      const int nb = n0 + 64 * wm + 32 * bi + 4 * h;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = nb + 8 * (r >> 2) + (r & 3);
        if (n < a.cout) C[n * kp + c] = acc[bi][bj][r] * unscale;
      }
    }
  }
}

}  // namespace

int64_t refine_wgrad_slice_len(int cin, int cout, int64_t K) {
  const int64_t tiles = (int64_t)9 * (cin / kTN) * ((cout + kTM - 1) / kTM);
  const int64_t want = (2048 + tiles - 1) / tiles;                     // about 2048 workgroups per site
  int64_t len = ((K + want - 1) / want + kTK - 1) / kTK * kTK;
  return len < 256 ? 256 : (len > 4096 ? 4096 : len);                  // 8 .. 128 K tiles per accumulation chain
}

int refine_wgrad_f16x3(hipStream_t st, const float* dz, int np, int cout, const float* src, int64_t ld, int cin, int n_img, int Hs,
                       int Ws, int stride, int up, const unsigned* max_bits, float* part, int64_t part_floats, int acc, float* g,
                       int64_t slice_len) {
  if ((cin % kTN) != 0 || (np % 32) != 0 || cout < 1 || cout > np || (stride != 1 && stride != 2)) return NSR_ERR_UNSUPPORTED;
  const int Hin = up ? 2 * Hs : Hs, Win = up ? 2 * Ws : Ws;
  WgArgs a{};
  a.dz = dz; a.np = np; a.cout = cout; a.src = src; a.ld = ld; a.cin = cin;
  a.n_img = n_img; a.Hs = Hs; a.Ws = Ws; a.Ho = (Hin - 1) / stride + 1; a.Wo = (Win - 1) / stride + 1; a.stride = stride; a.up = up;
  a.max_bits = max_bits; a.part = part;
  a.K = (int64_t)n_img * a.Ho * a.Wo;
  if (slice_len <= 0) slice_len = refine_wgrad_slice_len(cin, cout, a.K);
  if (slice_len % kTK) return NSR_ERR_UNSUPPORTED;
  a.slice_len = slice_len;
  const int kp = 9 * cin;
  a.slice_stride = (int64_t)cout * kp;
  const int64_t n_slices = (a.K + slice_len - 1) / slice_len;
  int64_t per_pass = part_floats / a.slice_stride;
  if (per_pass < 1) return NSR_ERR_WORKSPACE;
  per_pass = per_pass > 65535 ? 65535 : per_pass;                      // gridDim.z
  const dim3 tiles((unsigned)(9 * (cin / kTN)), (unsigned)((cout + kTM - 1) / kTM));
  for (int64_t z0 = 0; z0 < n_slices; z0 += per_pass) {
    const int64_t nz = n_slices - z0 < per_pass ? n_slices - z0 : per_pass;
    a.k_begin = z0 * slice_len;
    hipLaunchKernelGGL(refine_wgrad_kernel, dim3(tiles.x, tiles.y, (unsigned)nz), dim3(256), 0, st, a);
    NSR_CHECK_LAUNCH();
    const int rc = refine_wgrad_reduce(st, part, (int)nz, a.slice_stride, kp, cin, cout, (acc || z0 > 0) ? 1 : 0, g);
    if (rc != NSR_OK) return rc;
  }
  return NSR_OK;
}

}  // namespace nsr
