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
// SSIM backward: one launch, one workgroup per 16 x 32 tile of INPUT pixels; the window sums of the tile +- pad are recomputed
// in double, their derivatives kept as four double maps in LDS and gathered per pixel over the pixel's reflect-padding aliases
// (ssim_backward_kernel below).  No workspace, no atomics.
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

// ---- SSIM backward.  One workgroup per kBwdTileH x kBwdTileW tile of INPUT pixels of one plane, three phases:
//   stage         x, y over the tile +- 2 pad (indices reflected here), the window as double between kBwdWinPad zero rows;
//   coefficients  the five window sums of every output in the tile +- pad, and from them G dS/dm1, G dS/dm2, G dS/dm3 (= dm4),
//                 G dS/dm5 as four double maps in LDS (zero where the image has no output) -- a thread owns kBwdCoefRows
//                 vertically adjacent outputs of one column and shares the staged reads among them, as the forward does.  The
//                 window is staged between zero rows, so an input row that is no tap of an output multiplies a zero weight
//                 (acc + 0 x is acc, bit for bit) and the inner loop has no branch: its seven LDS reads issue together;
//   gather        a thread owns kBwdRows vertically adjacent pixels of one column and sums window x map over the outputs that
//                 read the pixel itself (tap index wave-uniform, a half-wave reads 32 consecutive doubles of a map row: all 64
//                 banks of an 8-byte LDS read once), then over the outputs that read it through the reflect padding (its
//                 aliases: border pixels only, per-lane loops).  Every output an alias reaches lies within +- pad of the pixel,
//                 so the maps of the tile +- pad are all a tile needs: nothing is exchanged between workgroups, no atomics,
//                 and the order of a pixel's sum depends on its coordinates alone.
constexpr int kBwdTileW = 32, kBwdTileH = 16;
constexpr int kBwdRows = 2;         // pixels per thread in the gather: 32 columns x 8 groups of 2 rows
constexpr int kBwdCoefRows = 5;     // outputs per thread in the coefficient phase: 11 x 11 window -> 42 columns x 6 groups = 252 threads
constexpr int kBwdWinPad = kBwdCoefRows - 1;   // zero rows above and below the staged window: a tap index -4 .. kh + 3 needs no branch
constexpr int kNoAlias = -(1 << 30);

static_assert(kBwdTileW * (kBwdTileH / kBwdRows) == kThreads, "one thread per column and row group of the tile");
static_assert(kBwdRows <= kBwdCoefRows, "the gather's tap index stays inside the zero rows of the window");

size_t ssim_backward_lds(int kh, int kw) {
  const size_t stage = (size_t)(kBwdTileH + 2 * (kh - 1)) * (size_t)(kBwdTileW + 2 * (kw - 1));
  const size_t coef = (size_t)(kBwdTileH + kh - 1) * (size_t)(kBwdTileW + kw - 1);
  return (size_t)(kh + 2 * kBwdWinPad) * kw * sizeof(double) + 4 * coef * sizeof(double) + 2 * stage * sizeof(float);
}

// kDx / kDy: which gradient is wanted.  The map of the other one's dS/dm is neither written nor gathered; every quantity that
// is computed goes through the same operations in the same order in all three instantiations.
template <bool kDx, bool kDy>
__global__ void __launch_bounds__(kThreads) ssim_backward_kernel(const float* __restrict__ X, const float* __restrict__ Y, int C, int H, int W,
                                                                 int64_t sb, int64_t sc, int64_t sh, int64_t sw,
                                                                 const float* __restrict__ window, int kh, int kw, double c1, double c2,
                                                                 int tiles_x, int tiles_y, double count, const float* __restrict__ g_ssim,
                                                                 const float* __restrict__ g_map, float* __restrict__ GX,
                                                                 float* __restrict__ GY) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int ph = (kh - 1) / 2, pw = (kw - 1) / 2;
  const int stage_h = kBwdTileH + 4 * ph, stage_w = kBwdTileW + 4 * pw;
  const int coef_h = kBwdTileH + 2 * ph, coef_w = kBwdTileW + 2 * pw;
  const int coef_n = coef_h * coef_w;
  double* wz = reinterpret_cast<double*>(smem);              // the window between kBwdWinPad zero rows
  double* wd = wz + kBwdWinPad * kw;                          // tap (i, j) at wd[i * kw + j], -kBwdWinPad <= i < kh + kBwdWinPad
  double* cm = wz + (kh + 2 * kBwdWinPad) * kw;               // maps of G dS/dm1, dm2, dm3, dm5
  float* xs = reinterpret_cast<float*>(cm + 4 * coef_n);
  float* ys = xs + stage_h * stage_w;

  const int tid = threadIdx.x;
  const int tile_x = (int)(blockIdx.x % (unsigned)tiles_x);
  const unsigned rest = blockIdx.x / (unsigned)tiles_x;
  const int tile_y = (int)(rest % (unsigned)tiles_y);
  const int64_t plane = rest / (unsigned)tiles_y;          // b * C + c
  const int64_t b = plane / C, c = plane % C;
  const float* xp = X + b * sb + c * sc;
  const float* yp = Y + b * sb + c * sc;
  const int ty0 = tile_y * kBwdTileH, tx0 = tile_x * kBwdTileW;

  // ---- stage
  for (int i = tid; i < (kh + 2 * kBwdWinPad) * kw; i += kThreads) {
    const int k = i - kBwdWinPad * kw;
    wz[i] = k >= 0 && k < kh * kw ? (double)window[k] : 0.0;
  }
#pragma unroll 4
  for (int i = tid; i < stage_h * stage_w; i += kThreads) {
    const int ly = i / stage_w, lx = i - ly * stage_w;
    const int64_t off = (int64_t)reflect_index(ty0 - 2 * ph + ly, H) * sh + (int64_t)reflect_index(tx0 - 2 * pw + lx, W) * sw;
    xs[i] = xp[off];
    ys[i] = yp[off];
  }
  __syncthreads();

  // ---- coefficients
  const double g_mean = g_ssim ? (double)g_ssim[b] / count : 0.0;
  const float* gm = g_map ? g_map + plane * H * W : nullptr;
  const int groups = (coef_h + kBwdCoefRows - 1) / kBwdCoefRows;
  for (int item = tid; item < groups * coef_w; item += kThreads) {
    const int grp = item / coef_w, cc = item - grp * coef_w;
    const int cr0 = grp * kBwdCoefRows;
    double acc[kBwdCoefRows][5];
#pragma unroll
    for (int q = 0; q < kBwdCoefRows; ++q)
#pragma unroll
      for (int m = 0; m < 5; ++m) acc[q][m] = 0.0;
    for (int j = 0; j < kw; ++j) {
#pragma unroll 3
      for (int rr = 0; rr < kBwdCoefRows + kh - 1; ++rr) {
        // staged row under this thread's outputs; the last group's rows beyond the staged tile are clamped: read, never used
        const int o = min(cr0 + rr, stage_h - 1) * stage_w + cc + j;
        const double x = (double)xs[o], y = (double)ys[o];
        const double xx = x * x, yy = y * y, xy = x * y;
#pragma unroll
        for (int q = 0; q < kBwdCoefRows; ++q) {
          const double w = wd[(rr - q) * kw + j];          // window row rr - q: wave-uniform; a zero row where it is no tap
          acc[q][0] = fma(w, x, acc[q][0]);
          acc[q][1] = fma(w, y, acc[q][1]);
          acc[q][2] = fma(w, xx, acc[q][2]);
          acc[q][3] = fma(w, yy, acc[q][3]);
          acc[q][4] = fma(w, xy, acc[q][4]);
        }
      }
    }
    const int gx = tx0 - pw + cc;
#pragma unroll
    for (int q = 0; q < kBwdCoefRows; ++q) {
      const int cr = cr0 + q, gy = ty0 - ph + cr;
      if (cr >= coef_h) continue;
      double px = 0.0, py = 0.0, qv = 0.0, rv = 0.0;
      if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
        const double mu_x = acc[q][0], mu_y = acc[q][1];
        const double mxx = mu_x * mu_x, myy = mu_y * mu_y, mxy = mu_x * mu_y;
        const double sxx = acc[q][2] - mxx, syy = acc[q][3] - myy, sxy = acc[q][4] - mxy;
        const double a1 = 2.0 * mxy + c1, a2 = 2.0 * sxy + c2;
        const double b1 = mxx + myy + c1, b2 = sxx + syy + c2;
        const double d = b1 * b2;
        const double s = (a1 * a2) / d;
        const double g = gm ? g_mean + (double)gm[(int64_t)gy * W + gx] : g_mean;
        const double t1 = (a2 - a1) / d, t2 = s * (1.0 / b1 - 1.0 / b2);
        px = g * (2.0 * mu_y * t1 - 2.0 * mu_x * t2);
        py = g * (2.0 * mu_x * t1 - 2.0 * mu_y * t2);
        qv = g * (-s / b2);
        rv = g * (2.0 * a1 / d);
      }
      const int o = cr * coef_w + cc;
      if (kDx) cm[o] = px;
      if (kDy) cm[coef_n + o] = py;
      cm[2 * coef_n + o] = qv;
      cm[3 * coef_n + o] = rv;
    }
  }
  __syncthreads();

  // ---- gather
  const int tx = tid & (kBwdTileW - 1), r0 = (tid / kBwdTileW) * kBwdRows;
  double u[kBwdRows], uy[kBwdRows], v[kBwdRows], z[kBwdRows];
#pragma unroll
  for (int t = 0; t < kBwdRows; ++t) u[t] = uy[t] = v[t] = z[t] = 0.0;
  // the pixel itself: output (r + dr, c + dc) reads it through tap (ph - dr, pw - dc); map row r0 + rr is output row r0 + rr - ph
  for (int jj = 0; jj < kw; ++jj) {
    const double* mc = cm + r0 * coef_w + tx + jj;
    const int kc = kw - 1 - jj;
    for (int rr = 0; rr < kBwdRows + kh - 1; ++rr) {
      const int o = rr * coef_w;
      const double ma = kDx ? mc[o] : 0.0, mb = kDy ? mc[coef_n + o] : 0.0, mq = mc[2 * coef_n + o], mr = mc[3 * coef_n + o];
#pragma unroll
      for (int t = 0; t < kBwdRows; ++t) {
        const double w = wd[(t + kh - 1 - rr) * kw + kc];  // window row -1 .. kh: wave-uniform; a zero row where it is no tap
        if (kDx) u[t] = fma(w, ma, u[t]);
        if (kDy) uy[t] = fma(w, mb, uy[t]);
        v[t] = fma(w, mq, v[t]);
        z[t] = fma(w, mr, z[t]);
      }
    }
  }
  const int gj = tx0 + tx;
#pragma unroll
  for (int t = 0; t < kBwdRows; ++t) {
    const int gi = ty0 + r0 + t;
    if (gi >= H || gj >= W) continue;
    // the padded positions that reflect onto the pixel: itself, -i for 1 <= i <= pad, 2 (n - 1) - i for n - 1 - pad <= i <= n - 2
    const int prow[3] = {gi, (gi >= 1 && gi <= ph) ? -gi : kNoAlias, (gi >= H - 1 - ph && gi <= H - 2) ? 2 * (H - 1) - gi : kNoAlias};
    const int pcol[3] = {gj, (gj >= 1 && gj <= pw) ? -gj : kNoAlias, (gj >= W - 1 - pw && gj <= W - 2) ? 2 * (W - 1) - gj : kNoAlias};
    for (int ar = 0; ar < 3; ++ar) {
      for (int ac = 0; ac < 3; ++ac) {
        if ((ar == 0 && ac == 0) || prow[ar] == kNoAlias || pcol[ac] == kNoAlias) continue;
        // taps whose output (p + pad - k) exists; those outputs lie within +- pad of the pixel: inside the maps
        const int top = prow[ar] + ph, left = pcol[ac] + pw;
        const int kr_lo = max(0, top - (H - 1)), kr_hi = min(kh - 1, top);
        const int kc_lo = max(0, left - (W - 1)), kc_hi = min(kw - 1, left);
        for (int kr = kr_lo; kr <= kr_hi; ++kr) {
          const int ro = (top - kr - (ty0 - ph)) * coef_w - (tx0 - pw);
          for (int kc = kc_lo; kc <= kc_hi; ++kc) {
            const double w = wd[kr * kw + kc];
            const int o = ro + left - kc;
            if (kDx) u[t] = fma(w, cm[o], u[t]);
            if (kDy) uy[t] = fma(w, cm[coef_n + o], uy[t]);
            v[t] = fma(w, cm[2 * coef_n + o], v[t]);
            z[t] = fma(w, cm[3 * coef_n + o], z[t]);
          }
        }
      }
    }
    const int so = (r0 + t + 2 * ph) * stage_w + tx + 2 * pw;
    const double xi = (double)xs[so], yi = (double)ys[so];
    const int64_t off = b * sb + c * sc + (int64_t)gi * sh + (int64_t)gj * sw;
    if (kDx) GX[off] = (float)(u[t] + 2.0 * xi * v[t] + yi * z[t]);
    if (kDy) GY[off] = (float)(uy[t] + 2.0 * yi * v[t] + xi * z[t]);
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

extern "C" int nsr_ssim_backward(const float* output, const float* target, int B, int C, int H, int W, int layout,
                                 const float* window, int kh, int kw, double c1, double c2, const float* g_ssim, const float* g_map,
                                 float* grad_output, float* grad_target, void* stream) {
  if (B < 0 || C <= 0 || H <= 0 || W <= 0) return NSR_ERR_INVALID_ARG;
  if (layout != NSR_LAYOUT_BCHW && layout != NSR_LAYOUT_BHWC) return NSR_ERR_INVALID_ARG;
  if (kh <= 0 || kw <= 0 || kh % 2 == 0 || kw % 2 == 0) return NSR_ERR_INVALID_ARG;
  if ((kh - 1) / 2 >= H || (kw - 1) / 2 >= W) return NSR_ERR_INVALID_ARG;            // torch's reflect condition
  if (B == 0) return NSR_OK;
  if (!output || !target || !window) return NSR_ERR_INVALID_ARG;
  if ((!g_ssim && !g_map) || (!grad_output && !grad_target)) return NSR_ERR_INVALID_ARG;
  const size_t lds = ssim_backward_lds(kh, kw);
  if (lds > kMaxLds) return NSR_ERR_UNSUPPORTED;
  const int64_t tiles_x = ((int64_t)W + kBwdTileW - 1) / kBwdTileW, tiles_y = ((int64_t)H + kBwdTileH - 1) / kBwdTileH;
  const int64_t blocks = (int64_t)B * C * tiles_y * tiles_x;
  if (blocks > 0x7fffffffLL) return NSR_ERR_UNSUPPORTED;
  int64_t sb, sc, sh, sw;
  if (layout == NSR_LAYOUT_BCHW) {
    sw = 1; sh = W; sc = (int64_t)H * W; sb = sc * C;
  } else {
    sc = 1; sw = C; sh = (int64_t)W * C; sb = sh * H;
  }
  const double count = (double)C * (double)H * (double)W;
  auto kernel = grad_output && grad_target ? ssim_backward_kernel<true, true>
                : grad_output              ? ssim_backward_kernel<true, false>
                                           : ssim_backward_kernel<false, true>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kThreads), lds, nsr_stream(stream), output, target, C, H, W, sb, sc, sh, sw,
                     window, kh, kw, c1, c2, (int)tiles_x, (int)tiles_y, count, g_ssim, g_map, grad_output, grad_target);
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
