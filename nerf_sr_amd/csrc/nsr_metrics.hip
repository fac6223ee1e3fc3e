// Evaluation metrics (include/nsr_metrics.h; reference: models/criterions.py:190-284 SSIM, :27-36 PSNR).
//
// SSIM: one workgroup per 32 x 32 output tile of one (image, channel) plane.  Both input tiles with their halo are staged
// once in LDS -- halo indices are reflected THERE, not per tap -- next to a double copy of the window table; a thread owns
// 4 vertically adjacent outputs of one column and walks the kh + 3 input rows under them once per window column, so one
// pair of LDS reads and one set of products (x, y, x^2, y^2, xy, formed in double) feeds up to 4 outputs; the tap index of
// each is wave-uniform (scalar branch, broadcast read of the weight).  Lanes of a wave read consecutive dwords: no bank
// conflicts.  All sums are double.  Per-tile sums go to the workspace and a second kernel adds each image's in a fixed order:
// no atomics, so a frame's result does not depend on the batch around it.
//
// PSNR: the same two stages over fixed 4096-element blocks of every segment.
#include <math.h>
#include "nsr_common.h"
#include "../../include/nsr_metrics.h"

namespace {

constexpr int kTile = 32;           // output tile edge
constexpr int kRows = 4;            // outputs per thread (rows); 256 threads = 32 columns x 8 groups of 4 rows
constexpr int kThreads = 256;
constexpr size_t kMaxLds = 64 * 1024;
constexpr int kPsnrPerThread = 16;
constexpr int kPsnrBlock = kThreads * kPsnrPerThread;    // 4096 elements per block

static_assert(kTile * (kTile / kRows) == kThreads, "one thread per column and row group of the tile");

// torch's reflect padding (no edge repeat); rows of a ragged tile beyond the padded image are clamped: staged, never used
__device__ __forceinline__ int reflect_index(int g, int n) {
  if (g < 0) g = -g;
  if (g >= n) g = 2 * (n - 1) - g;
  return min(max(g, 0), n - 1);
}

// sum of one double per thread over the 256 threads, in a fixed order; valid in thread 0
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();       // red may be reused
  return s;
}

__global__ void __launch_bounds__(kThreads) ssim_tile_kernel(const float* __restrict__ X, const float* __restrict__ Y, int C, int H, int W,
                                                             int64_t sb, int64_t sc, int64_t sh, int64_t sw,
                                                             const float* __restrict__ window, int kh, int kw, double c1, double c2,
                                                             int tiles_x, int tiles_y, double* __restrict__ partial,
                                                             float* __restrict__ map) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ double red[kThreads / 64];
  const int tw = kTile + kw - 1, th = kTile + kh - 1;
  double* wd = reinterpret_cast<double*>(smem);
  float* xs = reinterpret_cast<float*>(wd + kh * kw);
  float* ys = xs + th * tw;

  const int tid = threadIdx.x;
  const int tile_x = (int)(blockIdx.x % (unsigned)tiles_x);
  const unsigned rest = blockIdx.x / (unsigned)tiles_x;
  const int tile_y = (int)(rest % (unsigned)tiles_y);
  const int64_t plane = rest / (unsigned)tiles_y;          // b * C + c
  const int64_t b = plane / C, c = plane % C;
  const float* xp = X + b * sb + c * sc;
  const float* yp = Y + b * sb + c * sc;
  const int gx0 = tile_x * kTile - (kw - 1) / 2, gy0 = tile_y * kTile - (kh - 1) / 2;

  for (int i = tid; i < kh * kw; i += kThreads) wd[i] = (double)window[i];
  for (int i = tid; i < th * tw; i += kThreads) {
    const int ly = i / tw, lx = i - ly * tw;
    const int64_t off = (int64_t)reflect_index(gy0 + ly, H) * sh + (int64_t)reflect_index(gx0 + lx, W) * sw;
    xs[i] = xp[off];
    ys[i] = yp[off];
  }
  __syncthreads();

  const int tx = tid & (kTile - 1), tg = tid / kTile;
  double acc[kRows][5];
#pragma unroll
  for (int q = 0; q < kRows; ++q)
#pragma unroll
    for (int m = 0; m < 5; ++m) acc[q][m] = 0.0;

  for (int j = 0; j < kw; ++j) {
    const float* xc = xs + tg * kRows * tw + tx + j;
    const float* yc = ys + tg * kRows * tw + tx + j;
    for (int rr = 0; rr < kRows + kh - 1; ++rr) {          // input row of the tile under this thread's 4 outputs
      const double x = (double)xc[rr * tw], y = (double)yc[rr * tw];
      const double xx = x * x, yy = y * y, xy = x * y;
#pragma unroll
      for (int q = 0; q < kRows; ++q) {
        const int i = rr - q;                              // window row this input row is to output q: wave-uniform
        if (i >= 0 && i < kh) {
          const double w = wd[i * kw + j];
          acc[q][0] = fma(w, x, acc[q][0]);
          acc[q][1] = fma(w, y, acc[q][1]);
          acc[q][2] = fma(w, xx, acc[q][2]);
          acc[q][3] = fma(w, yy, acc[q][3]);
          acc[q][4] = fma(w, xy, acc[q][4]);
        }
      }
    }
  }

  double sum = 0.0;
  const int gx = tile_x * kTile + tx;
#pragma unroll
  for (int q = 0; q < kRows; ++q) {
    const int gy = tile_y * kTile + tg * kRows + q;
    if (gx < W && gy < H) {
      const double mu_x = acc[q][0], mu_y = acc[q][1];
      const double mxx = mu_x * mu_x, myy = mu_y * mu_y, mxy = mu_x * mu_y;
      const double sxx = acc[q][2] - mxx, syy = acc[q][3] - myy, sxy = acc[q][4] - mxy;
      const double a1 = 2.0 * mxy + c1, a2 = 2.0 * sxy + c2;
      const double b1 = mxx + myy + c1, b2 = sxx + syy + c2;
      const double v = (a1 * a2) / (b1 * b2);
      sum += v;
      if (map) map[(plane * H + gy) * W + gx] = (float)v;
    }
  }
  const double s = block_sum_d(sum, red);
  if (tid == 0) partial[blockIdx.x] = s;
}

// out[b] = (sum of the image's per-tile sums, fixed order) / count
__global__ void __launch_bounds__(kThreads) ssim_finish_kernel(const double* __restrict__ partial, int64_t per_image, double count,
                                                               double* __restrict__ out) {
  __shared__ double red[kThreads / 64];
  const double* p = partial + (int64_t)blockIdx.x * per_image;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < per_image; i += kThreads) s += p[i];
  s = block_sum_d(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s / count;
}

__global__ void __launch_bounds__(kThreads) psnr_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                                                                const uint8_t* __restrict__ mask, int mask_group,
                                                                unsigned blocks_per_seg, double* __restrict__ partial) {
  __shared__ double red[kThreads / 64];
  const int64_t seg = blockIdx.x / blocks_per_seg;
  const int64_t start = (int64_t)(blockIdx.x % blocks_per_seg) * kPsnrBlock;
  const float* ap = a + seg * n;
  const float* bp = b + seg * n;
  const uint8_t* mp = mask ? mask + seg * (n / mask_group) : nullptr;
  double s = 0.0, cnt = 0.0;
#pragma unroll 4
  for (int k = 0; k < kPsnrPerThread; ++k) {
    const int64_t i = start + (int64_t)k * kThreads + threadIdx.x;
    if (i < n && (!mp || mp[i / mask_group])) {
      const double d = (double)ap[i] - (double)bp[i];
      s = fma(d, d, s);
      cnt += 1.0;
    }
  }
  s = block_sum_d(s, red);
  cnt = block_sum_d(cnt, red);
  if (threadIdx.x == 0) {
    partial[2 * (int64_t)blockIdx.x] = s;
    partial[2 * (int64_t)blockIdx.x + 1] = cnt;
  }
}

__global__ void __launch_bounds__(kThreads) psnr_finish_kernel(const double* __restrict__ partial, unsigned blocks_per_seg,
                                                               double* __restrict__ mse, double* __restrict__ psnr) {
  __shared__ double red[kThreads / 64];
  const double* p = partial + 2 * (int64_t)blockIdx.x * blocks_per_seg;
  double s = 0.0, cnt = 0.0;
  for (unsigned i = threadIdx.x; i < blocks_per_seg; i += kThreads) {
    s += p[2 * (int64_t)i];
    cnt += p[2 * (int64_t)i + 1];
  }
  s = block_sum_d(s, red);
  cnt = block_sum_d(cnt, red);
  if (threadIdx.x == 0) {
    const double m = s / cnt;                    // 0 / 0: NaN, torch.mean of an empty selection
    if (mse) mse[blockIdx.x] = m;
    if (psnr) psnr[blockIdx.x] = -10.0 * log10(m);
  }
}

int64_t ssim_tiles(int n) { return ((int64_t)n + kTile - 1) / kTile; }
int64_t psnr_blocks(int64_t n) { return n == 0 ? 1 : (n + kPsnrBlock - 1) / kPsnrBlock; }

}  // namespace

extern "C" size_t nsr_ssim_workspace_bytes(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)B * (size_t)C * (size_t)(ssim_tiles(H) * ssim_tiles(W)) * sizeof(double);
}

extern "C" int nsr_ssim(const float* output, const float* target, int B, int C, int H, int W, int layout, const float* window,
                        int kh, int kw, double c1, double c2, double* ssim, float* ssim_map, void* workspace,
                        size_t workspace_bytes, void* stream) {
  if (B < 0 || C <= 0 || H <= 0 || W <= 0) return NSR_ERR_INVALID_ARG;
  if (layout != NSR_LAYOUT_BCHW && layout != NSR_LAYOUT_BHWC) return NSR_ERR_INVALID_ARG;
  if (kh <= 0 || kw <= 0 || kh % 2 == 0 || kw % 2 == 0) return NSR_ERR_INVALID_ARG;
  if ((kh - 1) / 2 >= H || (kw - 1) / 2 >= W) return NSR_ERR_INVALID_ARG;            // torch's reflect condition
  if (B == 0) return NSR_OK;
  if (!output || !target || !window || !ssim || !workspace) return NSR_ERR_INVALID_ARG;
  const size_t lds = (size_t)kh * kw * sizeof(double) + 2 * (size_t)(kTile + kh - 1) * (size_t)(kTile + kw - 1) * sizeof(float);
  if (lds > kMaxLds) return NSR_ERR_UNSUPPORTED;
  const int64_t tiles_x = ssim_tiles(W), tiles_y = ssim_tiles(H);
  const int64_t per_image = (int64_t)C * tiles_y * tiles_x;
  if (per_image * B > 0x7fffffffLL) return NSR_ERR_UNSUPPORTED;
  if (workspace_bytes < nsr_ssim_workspace_bytes(B, C, H, W)) return NSR_ERR_WORKSPACE;
  int64_t sb, sc, sh, sw;
  if (layout == NSR_LAYOUT_BCHW) {
    sw = 1; sh = W; sc = (int64_t)H * W; sb = sc * C;
  } else {
    sc = 1; sw = C; sh = (int64_t)W * C; sb = sh * H;
  }
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)(per_image * B)), dim3(kThreads), lds, nsr_stream(stream), output, target, C, H, W,
                     sb, sc, sh, sw, window, kh, kw, c1, c2, (int)tiles_x, (int)tiles_y, partial, ssim_map);
  NSR_CHECK_LAUNCH();
  hipLaunchKernelGGL(ssim_finish_kernel, dim3((unsigned)B), dim3(kThreads), 0, nsr_stream(stream), partial, per_image,
                     (double)C * (double)H * (double)W, ssim);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

extern "C" size_t nsr_psnr_workspace_bytes(int n_seg, int64_t n) {
  if (n_seg <= 0 || n < 0) return 0;
  return (size_t)n_seg * (size_t)psnr_blocks(n) * 2 * sizeof(double);
}

extern "C" int nsr_psnr(const float* a, const float* b, int n_seg, int64_t n, const uint8_t* mask, int mask_group, double* mse,
                        double* psnr, void* workspace, size_t workspace_bytes, void* stream) {
  if (n_seg < 0 || n < 0) return NSR_ERR_INVALID_ARG;
  if (mask && (mask_group <= 0 || n % mask_group != 0)) return NSR_ERR_INVALID_ARG;
  if (n_seg == 0) return NSR_OK;
  if ((n > 0 && (!a || !b)) || (!mse && !psnr) || !workspace) return NSR_ERR_INVALID_ARG;
  const int64_t bps = psnr_blocks(n);
  if (bps * n_seg > 0x7fffffffLL) return NSR_ERR_UNSUPPORTED;
  if (workspace_bytes < nsr_psnr_workspace_bytes(n_seg, n)) return NSR_ERR_WORKSPACE;
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(psnr_partial_kernel, dim3((unsigned)(bps * n_seg)), dim3(kThreads), 0, nsr_stream(stream), a, b, n, mask,
                     mask ? mask_group : 1, (unsigned)bps, partial);
  NSR_CHECK_LAUNCH();
  hipLaunchKernelGGL(psnr_finish_kernel, dim3((unsigned)n_seg), dim3(kThreads), 0, nsr_stream(stream), partial, (unsigned)bps, mse, psnr);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
