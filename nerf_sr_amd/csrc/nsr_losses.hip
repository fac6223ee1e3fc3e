// Image-space regularisers (include/nsr_losses.h; reference: models/criterions.py:56-69 TVLoss, :71-101 GradientLoss, :103-115
// LaplacianLoss, :118-137 BilateralLaplacianLoss).
//
// One core for the three families: a workgroup owns a 32 x 32 tile of one image plane (a thread: one column, 4 rows, the
// thread layout of the SSIM kernels), planes are addressed by (plane, row, column) strides so that (H, W, C), (B, C, H, W) and
// (N, H, W) are the same kernel, and the tile with its halo is staged once in LDS as fp32 (zeros outside the image: staged,
// never used -- every use is guarded by the global index).
//
// Forward: every stencil is evaluated by the thread that owns its first / centre element, in double and in the reference's
// operand order; a workgroup's sums go to the workspace (partial[k * n_blocks + block], k = the reference's k-th sum) and one
// finishing launch adds them in a fixed order, divides each by its own count and combines them as the reference does.
// Backward: gather form -- every input element adds up the stencils it belongs to, in double; one rounding, at the store.
// The patches these losses see are small: the launches are launch-bound, nothing here trades exactness for speed.
#include <math.h>
#include "nsr_common.h"
#include "../../include/nsr_losses.h"

namespace {

constexpr int kTile = 32;           // tile edge
constexpr int kRows = 4;            // elements per thread (rows); 256 threads = 32 columns x 8 groups of 4 rows
constexpr int kThreads = 256;
constexpr int kFwdDiff = kTile + 1;     // staged edge, forward TV / gradient: one element right and down
constexpr int kHalo1 = kTile + 2;       // one element all round: forward Laplacian, backward TV / gradient, the coefficient maps
constexpr int kHalo2 = kTile + 4;       // two elements all round: backward Laplacian
constexpr size_t kLapBwdLds = 4 * kHalo1 * kHalo1 * sizeof(double) + kHalo2 * kHalo2 * sizeof(float);

static_assert(kTile * (kTile / kRows) == kThreads, "one thread per column and row group of the tile");
static_assert(kLapBwdLds <= 64 * 1024, "the Laplacian backward's maps fit in LDS");

struct TileAt {
  int x0, y0;          // first column / row of the tile
  int64_t plane;
};

__device__ __forceinline__ TileAt tile_of_block(int tiles_x, int tiles_y) {
  TileAt t;
  t.x0 = (int)(blockIdx.x % (unsigned)tiles_x) * kTile;
  const unsigned rest = blockIdx.x / (unsigned)tiles_x;
  t.y0 = (int)(rest % (unsigned)tiles_y) * kTile;
  t.plane = rest / (unsigned)tiles_y;
  return t;
}

// dst (edge x edge) = the plane's elements from (y0, x0) on; 0 outside the image
__device__ __forceinline__ void stage_tile(float* __restrict__ dst, const float* __restrict__ plane, int H, int W, int64_t sh,
                                           int64_t sw, int y0, int x0, int edge) {
  for (int i = threadIdx.x; i < edge * edge; i += kThreads) {
    const int ly = i / edge, lx = i - ly * edge;
    const int gy = y0 + ly, gx = x0 + lx;
    dst[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? plane[(int64_t)gy * sh + (int64_t)gx * sw] : 0.0f;
  }
}

// sum of one double per thread over the 256 threads, in a fixed order
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();       // red may be reused
  return s;
}

// torch's sgn of a real: sign(0) = 0 (the derivative torch.abs back-propagates)
__device__ __forceinline__ double sign0(double v) { return (double)((v > 0.0) - (v < 0.0)); }

// local offset (in a staged map of `edge` columns) of the direction e of the k-th Laplacian stencil: column, row, main
// diagonal, anti-diagonal.  The reference's first operand is p - e, its second p + e (L4: inputs[2:, :-2] + inputs[:-2, 2:]).
__device__ __forceinline__ int lap_dy(int k) { return k == 0 ? 0 : (k == 3 ? -1 : 1); }
__device__ __forceinline__ bool lap_centre_valid(int k, int gy, int gx, int H, int W) {
  if (gy < 0 || gy >= H || gx < 0 || gx >= W) return false;
  const bool col = gx >= 1 && gx <= W - 2, row = gy >= 1 && gy <= H - 2;
  return k == 0 ? col : (k == 1 ? row : (col && row));
}

// exp(-sum_c |guide[p - e] + guide[p + e] - 2 guide[p]| / gamma) of one stencil; `centre`: the pixel's first channel
__device__ __forceinline__ double guide_weight(const float* __restrict__ centre, int64_t e, int C, double gamma) {
  double s = 0.0;
  for (int c = 0; c < C; ++c) s += fabs(((double)centre[c - e] + (double)centre[c + e]) - 2.0 * (double)centre[c]);
  return exp(-s / gamma);
}

enum { kTV = NSR_LOSS_TV, kGradient = NSR_LOSS_GRADIENT };

// ---- forward, TV and gradient: differences to the right and down neighbour.  partial[0]: the reference's first sum (TV: over
// rows, h_tv; gradient: dx), partial[1]: its second.
template <int kKind>
__global__ void __launch_bounds__(kThreads) diff_forward_kernel(const float* __restrict__ A, const float* __restrict__ Bv, int H, int W,
                                                                int64_t sp, int64_t sh, int64_t sw, int tiles_x, int tiles_y,
                                                                int64_t n_blocks, double* __restrict__ partial) {
  __shared__ float as[kFwdDiff * kFwdDiff];
  __shared__ float bs[kKind == kGradient ? kFwdDiff * kFwdDiff : 1];
  __shared__ double red[kThreads / 64];
  const TileAt t = tile_of_block(tiles_x, tiles_y);
  stage_tile(as, A + t.plane * sp, H, W, sh, sw, t.y0, t.x0, kFwdDiff);
  if (kKind == kGradient) stage_tile(bs, Bv + t.plane * sp, H, W, sh, sw, t.y0, t.x0, kFwdDiff);
  __syncthreads();

  const int tx = threadIdx.x & (kTile - 1), tg = threadIdx.x / kTile;
  const int gx = t.x0 + tx;
  double s_rows = 0.0, s_cols = 0.0;         // differences along rows (down) / along columns (right)
#pragma unroll
  for (int q = 0; q < kRows; ++q) {
    const int ly = tg * kRows + q, gy = t.y0 + ly, l = ly * kFwdDiff + tx;
    if (gx < W && gy < H) {
      if (gy + 1 < H) {
        double d = (double)as[l + kFwdDiff] - (double)as[l];
        if (kKind == kGradient) d = fabs(d - ((double)bs[l + kFwdDiff] - (double)bs[l]));
        s_rows += kKind == kTV ? d * d : d;
      }
      if (gx + 1 < W) {
        double d = (double)as[l + 1] - (double)as[l];
        if (kKind == kGradient) d = fabs(d - ((double)bs[l + 1] - (double)bs[l]));
        s_cols += kKind == kTV ? d * d : d;
      }
    }
  }
  // TVLoss: h_tv (rows) first; GradientLoss: dx (columns) first
  const double first = block_sum_d(kKind == kTV ? s_rows : s_cols, red);
  const double second = block_sum_d(kKind == kTV ? s_cols : s_rows, red);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = first;
    partial[n_blocks + blockIdx.x] = second;
  }
}

// ---- forward, Laplacian: the four second differences centred on the thread's elements; partial[k]: sum of |w t| of L(k+1)
template <bool kGuide>
__global__ void __launch_bounds__(kThreads) lap_forward_kernel(const float* __restrict__ D, const float* __restrict__ G, int H, int W, int C,
                                                               double gamma, int tiles_x, int tiles_y, int64_t n_blocks,
                                                               double* __restrict__ partial) {
  __shared__ float ds[kHalo1 * kHalo1];
  __shared__ double red[kThreads / 64];
  const TileAt t = tile_of_block(tiles_x, tiles_y);
  stage_tile(ds, D + t.plane * (int64_t)H * W, H, W, W, 1, t.y0 - 1, t.x0 - 1, kHalo1);
  __syncthreads();

  const int tx = threadIdx.x & (kTile - 1), tg = threadIdx.x / kTile;
  const int gx = t.x0 + tx;
  const float* gimg = kGuide ? G + t.plane * (int64_t)H * W * C : nullptr;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < kRows; ++q) {
    const int ly = tg * kRows + q, gy = t.y0 + ly, l = (ly + 1) * kHalo1 + tx + 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (lap_centre_valid(k, gy, gx, H, W)) {
        const int dy = lap_dy(k), dx = k == 1 ? 0 : 1;
        const int e = dy * kHalo1 + dx;
        double v = ((double)ds[l - e] + (double)ds[l + e]) - 2.0 * (double)ds[l];
        if (kGuide) v = guide_weight(gimg + ((int64_t)gy * W + gx) * C, ((int64_t)dy * W + dx) * C, C, gamma) * v;
        s[k] += fabs(v);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double v = block_sum_d(s[k], red);
    if (threadIdx.x == 0) partial[k * n_blocks + blockIdx.x] = v;
  }
}

struct Counts {
  double n[4];
};

// loss = scale * ((S_0 / n_0 + S_1 / n_1) + ...): each S_k the sum of its n_blocks partials in a fixed order
__global__ void __launch_bounds__(kThreads) loss_finish_kernel(const double* __restrict__ partial, int64_t n_blocks, int n_sums, Counts cnt,
                                                               double scale, double* __restrict__ out) {
  __shared__ double red[kThreads / 64];
  double total = 0.0;
  for (int k = 0; k < n_sums; ++k) {
    const double* p = partial + k * n_blocks;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n_blocks; i += kThreads) s += p[i];
    s = block_sum_d(s, red);
    total = k == 0 ? s / cnt.n[0] : total + s / cnt.n[k];
  }
  if (threadIdx.x == 0) out[0] = total * scale;
}

// ---- backward, TV and gradient.  An element belongs to the difference it starts (coefficient -1) and to the one its left / upper
// neighbour starts (+1), along rows and along columns: up to four contributions.
//   TV:        d/dx of d^2 = 2 d;   grad = g (sum_rows / n_rows + sum_cols / n_cols)
//   gradient:  d/da of |da - db| = sign(da - db), sign(0) = 0;  grad_a = (g / 2 / n) sum,  grad_b = -grad_a
template <int kKind>
__global__ void __launch_bounds__(kThreads) diff_backward_kernel(const float* __restrict__ A, const float* __restrict__ Bv, int H, int W,
                                                                 int64_t sp, int64_t sh, int64_t sw, int tiles_x, int tiles_y,
                                                                 double n_first, double n_second, const float* __restrict__ g,
                                                                 float* __restrict__ grad_a, float* __restrict__ grad_b) {
  __shared__ float as[kHalo1 * kHalo1];
  __shared__ float bs[kKind == kGradient ? kHalo1 * kHalo1 : 1];
  const TileAt t = tile_of_block(tiles_x, tiles_y);
  stage_tile(as, A + t.plane * sp, H, W, sh, sw, t.y0 - 1, t.x0 - 1, kHalo1);
  if (kKind == kGradient) stage_tile(bs, Bv + t.plane * sp, H, W, sh, sw, t.y0 - 1, t.x0 - 1, kHalo1);
  __syncthreads();

  const int tx = threadIdx.x & (kTile - 1), tg = threadIdx.x / kTile;
  const int gx = t.x0 + tx;
  const double up = (double)g[0];
  // the difference from local element `from` to `from + step`, as the forward forms it
  auto diff = [&](int from, int step) -> double {
    const double d = (double)as[from + step] - (double)as[from];
    if (kKind == kTV) return 2.0 * d;
    return sign0(d - ((double)bs[from + step] - (double)bs[from]));
  };
#pragma unroll
  for (int q = 0; q < kRows; ++q) {
    const int ly = tg * kRows + q, gy = t.y0 + ly, l = (ly + 1) * kHalo1 + tx + 1;
    if (gx < W && gy < H) {
      double s_rows = 0.0, s_cols = 0.0;
      if (gy > 0) s_rows += diff(l - kHalo1, kHalo1);
      if (gy + 1 < H) s_rows -= diff(l, kHalo1);
      if (gx > 0) s_cols += diff(l - 1, 1);
      if (gx + 1 < W) s_cols -= diff(l, 1);
      const int64_t o = t.plane * sp + (int64_t)gy * sh + (int64_t)gx * sw;
      if (kKind == kTV) {
        grad_a[o] = (float)((up / n_first) * s_rows + (up / n_second) * s_cols);     // n_first: (H-1) W C, the row differences
      } else {
        const double v = ((up * 0.5) / n_first) * (s_cols + s_rows);                 // both means over B C H W
        if (grad_a) grad_a[o] = (float)v;
        if (grad_b) grad_b[o] = (float)(-v);
      }
    }
  }
}

// ---- backward, Laplacian.  Phase 1: d over the tile +- 2.  Phase 2: for every stencil centred in the tile +- 1 and each of the
// four directions, coef = sign(w t) w (0 where the centre is outside the direction's index set): 4 maps of 34 x 34 doubles.
// Phase 3: an element p gathers, per direction, s_k = -2 coef[p] + coef[p - e] + coef[p + e] (it is the centre of the stencil at
// p, the `p + e` end of the one centred at p - e and the `p - e` end of the one centred at p + e); grad = g / 4 sum_k s_k / n_k.
template <bool kGuide>
__global__ void __launch_bounds__(kThreads) lap_backward_kernel(const float* __restrict__ D, const float* __restrict__ G, int H, int W, int C,
                                                                double gamma, int tiles_x, int tiles_y, double den,
                                                                const float* __restrict__ g, float* __restrict__ grad) {
  extern __shared__ __align__(16) unsigned char smem[];
  double* coef = reinterpret_cast<double*>(smem);                        // [4][kHalo1 * kHalo1]
  float* ds = reinterpret_cast<float*>(coef + 4 * kHalo1 * kHalo1);      // [kHalo2 * kHalo2]
  const TileAt t = tile_of_block(tiles_x, tiles_y);
  const int64_t plane_off = t.plane * (int64_t)H * W;
  stage_tile(ds, D + plane_off, H, W, W, 1, t.y0 - 2, t.x0 - 2, kHalo2);
  __syncthreads();

  const float* gimg = kGuide ? G + plane_off * C : nullptr;
  for (int i = threadIdx.x; i < kHalo1 * kHalo1; i += kThreads) {
    const int cy = i / kHalo1, cx = i - cy * kHalo1;
    const int gy = t.y0 - 1 + cy, gx = t.x0 - 1 + cx;
    const int l = (cy + 1) * kHalo2 + cx + 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      double c = 0.0;
      if (lap_centre_valid(k, gy, gx, H, W)) {
        const int dy = lap_dy(k), dx = k == 1 ? 0 : 1;
        const int e = dy * kHalo2 + dx;
        const double v = ((double)ds[l - e] + (double)ds[l + e]) - 2.0 * (double)ds[l];
        const double w = kGuide ? guide_weight(gimg + ((int64_t)gy * W + gx) * C, ((int64_t)dy * W + dx) * C, C, gamma) : 1.0;
        c = sign0(w * v) * w;
      }
      coef[k * kHalo1 * kHalo1 + i] = c;
    }
  }
  __syncthreads();

  const int tx = threadIdx.x & (kTile - 1), tg = threadIdx.x / kTile;
  const int gx = t.x0 + tx;
  // sum_k s_k / n_k over the common denominator N H W (H-2) (W-2): n_0 = N H (W-2), n_1 = N (H-2) W, n_2 = n_3 = N (H-2) (W-2).
  // Without a guide the s_k are small integers and the numerator is exact, so contributions that cancel across directions
  // (3 / n_2 against 4 / n_0 at 8 x 8) give an exact 0 and not the rounding residue of four separate quotients.
  const double up = (double)g[0] * 0.25;
  const double m0 = (double)(H - 2) * (double)W, m1 = (double)H * (double)(W - 2), m2 = (double)H * (double)W;
#pragma unroll
  for (int q = 0; q < kRows; ++q) {
    const int ly = tg * kRows + q, gy = t.y0 + ly, l = (ly + 1) * kHalo1 + tx + 1;
    if (gx < W && gy < H) {
      double s[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double* ck = coef + k * kHalo1 * kHalo1;
        const int e = lap_dy(k) * kHalo1 + (k == 1 ? 0 : 1);
        s[k] = (ck[l - e] + ck[l + e]) - 2.0 * ck[l];
      }
      const double num = (s[0] * m0 + s[1] * m1) + (s[2] + s[3]) * m2;
      grad[plane_off + (int64_t)gy * W + gx] = (float)(up * num / den);
    }
  }
}

int64_t tiles(int n) { return ((int64_t)n + kTile - 1) / kTile; }

// number of workgroups of `planes` planes of H x W; 0 when the grid would not fit
int64_t grid_blocks(int64_t planes, int H, int W) {
  const int64_t per_plane = tiles(H) * tiles(W);
  if (planes > 0x7fffffffLL / per_plane) return 0;
  return planes * per_plane;
}

bool lap_args_ok(const float* guide, int N, int H, int W, int C, double gamma) {
  return N > 0 && H >= 3 && W >= 3 && gamma > 0.0 && (!guide || C > 0);
}

Counts lap_counts(int N, int H, int W) {
  Counts c;
  c.n[0] = (double)N * (double)H * (double)(W - 2);
  c.n[1] = (double)N * (double)(H - 2) * (double)W;
  c.n[2] = c.n[3] = (double)N * (double)(H - 2) * (double)(W - 2);
  return c;
}

}  // namespace

extern "C" size_t nsr_loss_workspace_bytes(int kind, int64_t n_img, int C, int H, int W) {
  if (n_img <= 0 || H <= 0 || W <= 0) return 0;
  int64_t planes, sums;
  if (kind == NSR_LOSS_TV) {
    if (C <= 0 || H < 2 || W < 2) return 0;
    planes = n_img * C;
    sums = 2;
  } else if (kind == NSR_LOSS_GRADIENT) {
    if (C <= 0) return 0;
    planes = n_img * C;
    sums = 2;
  } else if (kind == NSR_LOSS_LAPLACIAN) {
    if (H < 3 || W < 3) return 0;
    planes = n_img;
    sums = 4;
  } else {
    return 0;
  }
  return (size_t)planes * (size_t)(tiles(H) * tiles(W)) * (size_t)sums * sizeof(double);
}

extern "C" int nsr_tv_loss(const float* x, int H, int W, int C, double* loss, void* workspace, size_t workspace_bytes, void* stream) {
  if (H < 2 || W < 2 || C <= 0) return NSR_ERR_INVALID_ARG;
  if (!x || !loss || !workspace) return NSR_ERR_INVALID_ARG;
  const int64_t blocks = grid_blocks(C, H, W);
  if (blocks == 0) return NSR_ERR_UNSUPPORTED;
  if (workspace_bytes < nsr_loss_workspace_bytes(NSR_LOSS_TV, 1, C, H, W)) return NSR_ERR_WORKSPACE;
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(diff_forward_kernel<kTV>, dim3((unsigned)blocks), dim3(kThreads), 0, nsr_stream(stream), x, (const float*)nullptr, H,
                     W, (int64_t)1, (int64_t)W * C, (int64_t)C, (int)tiles(W), (int)tiles(H), blocks, partial);
  NSR_CHECK_LAUNCH();
  Counts cnt = {{(double)(H - 1) * (double)W * (double)C, (double)H * (double)(W - 1) * (double)C, 1.0, 1.0}};
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(kThreads), 0, nsr_stream(stream), partial, blocks, 2, cnt, 1.0, loss);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

extern "C" int nsr_tv_loss_backward(const float* x, int H, int W, int C, const float* g, float* grad_x, void* stream) {
  if (H < 2 || W < 2 || C <= 0) return NSR_ERR_INVALID_ARG;
  if (!x || !g || !grad_x) return NSR_ERR_INVALID_ARG;
  const int64_t blocks = grid_blocks(C, H, W);
  if (blocks == 0) return NSR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(diff_backward_kernel<kTV>, dim3((unsigned)blocks), dim3(kThreads), 0, nsr_stream(stream), x, (const float*)nullptr, H,
                     W, (int64_t)1, (int64_t)W * C, (int64_t)C, (int)tiles(W), (int)tiles(H), (double)(H - 1) * (double)W * (double)C,
                     (double)H * (double)(W - 1) * (double)C, g, grad_x, (float*)nullptr);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

extern "C" int nsr_gradient_loss(const float* a, const float* b, int B, int C, int H, int W, double* loss, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return NSR_ERR_INVALID_ARG;
  if (!a || !b || !loss || !workspace) return NSR_ERR_INVALID_ARG;
  const int64_t blocks = grid_blocks((int64_t)B * C, H, W);
  if (blocks == 0) return NSR_ERR_UNSUPPORTED;
  if (workspace_bytes < nsr_loss_workspace_bytes(NSR_LOSS_GRADIENT, B, C, H, W)) return NSR_ERR_WORKSPACE;
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(diff_forward_kernel<kGradient>, dim3((unsigned)blocks), dim3(kThreads), 0, nsr_stream(stream), a, b, H, W,
                     (int64_t)H * W, (int64_t)W, (int64_t)1, (int)tiles(W), (int)tiles(H), blocks, partial);
  NSR_CHECK_LAUNCH();
  const double n = (double)B * (double)C * (double)H * (double)W;
  Counts cnt = {{n, n, 1.0, 1.0}};
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(kThreads), 0, nsr_stream(stream), partial, blocks, 2, cnt, 0.5, loss);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

extern "C" int nsr_gradient_loss_backward(const float* a, const float* b, int B, int C, int H, int W, const float* g, float* grad_a,
                                          float* grad_b, void* stream) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return NSR_ERR_INVALID_ARG;
  if (!a || !b || !g || (!grad_a && !grad_b)) return NSR_ERR_INVALID_ARG;
  const int64_t blocks = grid_blocks((int64_t)B * C, H, W);
  if (blocks == 0) return NSR_ERR_UNSUPPORTED;
  const double n = (double)B * (double)C * (double)H * (double)W;
  hipLaunchKernelGGL(diff_backward_kernel<kGradient>, dim3((unsigned)blocks), dim3(kThreads), 0, nsr_stream(stream), a, b, H, W,
                     (int64_t)H * W, (int64_t)W, (int64_t)1, (int)tiles(W), (int)tiles(H), n, n, g, grad_a, grad_b);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

extern "C" int nsr_laplacian_loss(const float* d, const float* guide, int N, int H, int W, int C, double gamma, double* loss,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  if (!lap_args_ok(guide, N, H, W, C, gamma)) return NSR_ERR_INVALID_ARG;
  if (!d || !loss || !workspace) return NSR_ERR_INVALID_ARG;
  const int64_t blocks = grid_blocks(N, H, W);
  if (blocks == 0) return NSR_ERR_UNSUPPORTED;
  if (workspace_bytes < nsr_loss_workspace_bytes(NSR_LOSS_LAPLACIAN, N, 1, H, W)) return NSR_ERR_WORKSPACE;
  double* partial = static_cast<double*>(workspace);
  auto kernel = guide ? lap_forward_kernel<true> : lap_forward_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kThreads), 0, nsr_stream(stream), d, guide, H, W, C, gamma, (int)tiles(W),
                     (int)tiles(H), blocks, partial);
  NSR_CHECK_LAUNCH();
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(kThreads), 0, nsr_stream(stream), partial, blocks, 4, lap_counts(N, H, W), 0.25,
                     loss);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

extern "C" int nsr_laplacian_loss_backward(const float* d, const float* guide, int N, int H, int W, int C, double gamma, const float* g,
                                           float* grad_d, void* stream) {
  if (!lap_args_ok(guide, N, H, W, C, gamma)) return NSR_ERR_INVALID_ARG;
  if (!d || !g || !grad_d) return NSR_ERR_INVALID_ARG;
  const int64_t blocks = grid_blocks(N, H, W);
  if (blocks == 0) return NSR_ERR_UNSUPPORTED;
  auto kernel = guide ? lap_backward_kernel<true> : lap_backward_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kThreads), kLapBwdLds, nsr_stream(stream), d, guide, H, W, C, gamma,
                     (int)tiles(W), (int)tiles(H), (double)N * (double)H * (double)W * (double)(H - 2) * (double)(W - 2), g, grad_d);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
