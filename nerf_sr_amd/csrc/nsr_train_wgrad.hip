// Weight and bias gradients of the chain path of the training step (nsr_train.hip calls chain_weight_grads once per pass).
//
// The forward kernel (nsr_mlp_f16.hip, TRAIN) and the backward chain (nsr_train_chain.hip) leave every layer's activations
// and input gradients as 2-byte panels (nsr_f16x3_core.h, nsr_panels.h).  The twelve panel x panel products of a network are
// ONE launch of the fp16-MFMA kernel (nsr_wgrad_f16.hip, which also sums the bias gradients); the 1- and 3-row heads are
// streams over one panel (panel_wsums_kernel); every second pass -- reduce the partial tiles, scatter into the nn.Linear
// shapes -- is one more launch (finish_jobs_kernel).
#include "nsr_gemm.h"
#include "nsr_panels.h"
#include "nsr_train_work.h"

using namespace nsr;

namespace {

// sums over the points of  w[p][c] * panel[p][row]  for c < NW weights per point -- the weight gradients of the 1- and
// 3-row heads (sigma over h8 = forward panel 7, rgb over dir_encoding's output = forward panel 9), whose "GEMM" is a stream
// over one 2-byte panel:  partial[z][c * R + row] = sum over slice z.  The run of a point group is R / 16 units of 1 KiB
// (nsr_f16x3_core.h): 16-byte slot sl of unit U holds, for point m = ((sl ^ 8 (U & 1)) >> 1) and lane half h = sl & 1,
// the features 32 (U >> 1) + 16 (U & 1) + 4 h + {0..3} and + 8 + {0..3}.  Thread t owns slot t & 63 of the units
// (t >> 6) + 4 i: its eight features are the same for every point group, its point is m.
template <int R, int NW>
__global__ void __launch_bounds__(256) panel_wsums_kernel(const char* __restrict__ panel, int64_t P, const float* __restrict__ w,
                                                          int w_stride, int64_t groups_per_slice, float* __restrict__ partial) {
  constexpr int NI = R / 64;               // units per thread and point group
  typedef _Float16 h8v __attribute__((ext_vector_type(8)));
  const int tid = threadIdx.x, sl = tid & 63, u0 = tid >> 6, z = blockIdx.x;
  const int64_t n_groups = P / 32;
  const int64_t g0 = (int64_t)z * groups_per_slice;
  const int64_t g1 = (g0 + groups_per_slice < n_groups) ? g0 + groups_per_slice : n_groups;
  float acc[NI][8][NW];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int c = 0; c < NW; ++c) acc[i][e][c] = 0.0f;
  for (int64_t g = g0; g < g1; ++g) {
    const char* run = panel + g * (int64_t)(R * 64);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int U = u0 + 4 * i;
      const int m = (sl ^ (8 * (U & 1))) >> 1;
      const h8v v = __builtin_nontemporal_load(reinterpret_cast<const h8v*>(run + U * 1024 + sl * 16));
      float wk[NW];
#pragma unroll
      for (int c = 0; c < NW; ++c) wk[c] = w[(g * 32 + m) * w_stride + c];
#pragma unroll
      for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int c = 0; c < NW; ++c) acc[i][e][c] = fmaf((float)v[e], wk[c], acc[i][e][c]);
    }
  }
  // the 32 points of a (unit, lane half) are the slots of one parity: sum over slot bits 1..5
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int U = u0 + 4 * i, h = sl & 1;
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int c = 0; c < NW; ++c) {
        float s = acc[i][e][c];
#pragma unroll
        for (int o = 2; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
        const int row = 32 * (U >> 1) + 16 * (U & 1) + 8 * (e >> 2) + 4 * h + (e & 3);
        if ((sl >> 1) == 0) partial[(int64_t)z * (NW * R) + c * R + row] = s;
      }
  }
}

// enc_rows: the partial's columns are rows of an encoding panel (nsr_f16x3_core.h, enc_row): 1 = the encoded position,
// column j of the 63 is register t of lane half h with pecol(t, h) == j; 2 = the encoded direction, dircol(t, h) == j
__device__ __forceinline__ int enc_panel_row(int enc_rows, int j) {
  if (enc_rows == 0) return j;
  const int per = enc_rows == 1 ? 30 : 12;           // columns per lane half behind the three raw coordinates
  const int t = j < 2 ? j : (j == 2 ? 0 : (j - 3) % per + 2), h = j < 2 ? 0 : (j == 2 ? 1 : (j - 3) / per);
  return enc_row(t, h);
}
// All second passes of one network's weight / bias gradients in ONE launch (chain path): blockIdx.y = job.
//   kind 0: dst[i * dst_ld + dc0 + j] (+)= scale * sum_z partial[z * stride + i * p_ld + col(j)]   (reduce_place_kernel)
//   kind 1: dst[i] (+)= sum_z partial[z * rows + i]                                                 (rowsum_finish_kernel)
//   kind 2: dst[i] (+)= sum_z partial[z * stride + i], i < rows <= 4, `splits` up to thousands (one partial per ray: the
//           bias gradients of the two heads, composite_bwd_kernel): one wavefront per element, lanes stride over z
// Twenty-odd launches of a few microseconds of work each (one wave of latency-bound workgroups) became the tail of
// the step once the GEMMs before them had shrunk; together they keep the memory system busy.
// (FinishJob, kMaxFinishJobs: nsr_train_work.h.)  One job's threads are the 256 x 256 of its grid row: kinds 0 and 1 (up to 64
// slices) own one element each, so rows * cols <= 65,536 (finish_jobs checks it).
struct FinishJobs {
  FinishJob j[kMaxFinishJobs];
  int n;
};
__global__ void __launch_bounds__(256) finish_jobs_kernel(FinishJobs jobs) {
  const FinishJob& q = jobs.j[blockIdx.y];
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (q.kind == 2) {
    const int e = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (blockIdx.x != 0 || e >= q.rows) return;       // wave-uniform
    double s = 0.0;
    for (int z = lane; z < q.splits; z += 64) s += (double)q.partial[(int64_t)z * q.stride + e];
    s = wave_sum_d(s);
    if (lane == 0) q.dst[e] = (q.accumulate ? q.dst[e] : 0.0f) + (float)s;
    return;
  }
  if (q.kind == 1 && q.splits > 64) {
    // many slices (the head streams: 1,024, round 6): one wavefront per element, lanes stride over the slices -- a thread
    // that walks them alone is a chain of a hundred dependent round trips
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    for (int i = e; i < q.rows; i += 4 * gridDim.x) {      // wave-uniform
      double s = 0.0;
      for (int z = lane; z < q.splits; z += 64) s += (double)q.partial[(int64_t)z * q.rows + i];
      s = wave_sum_d(s);
      if (lane == 0) q.dst[i] = (q.accumulate ? q.dst[i] : 0.0f) + (float)(s * (double)q.scale);
    }
    return;
  }
  if (idx >= q.rows * q.cols) return;
  const float* src;
  int64_t stride;
  float* d;
  if (q.kind == 0) {
    const int i = idx / q.cols, j = idx % q.cols;
    const int js = enc_panel_row(q.enc_rows, j);
    src = q.partial + (int64_t)i * q.p_ld + js;
    stride = q.stride;
    d = q.dst + (int64_t)i * q.dst_ld + q.dc0 + j;
  } else {
    src = q.partial + idx;
    stride = q.rows;
    d = q.dst + idx;
  }
  // Eight loads in flight per thread (round 6; four until then): the kernel is latency-bound -- ~21 partial tiles per
  // product, 26 blocks per CU of which 8 are resident, every round a trip to L2 / HBM (38 us per call for 29 MB).  The
  // association of the sum is fixed (eight chains, then a tree): bit-reproducible run to run.
  double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int zc = 0;
  for (; zc + 8 <= q.splits; zc += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(int64_t)(zc + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] += (double)v[u];
  }
  {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = (zc + u < q.splits) ? src[(int64_t)(zc + u) * stride] : 0.0f;
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] += (double)v[u];
  }
  const double sum = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  *d = (q.accumulate ? *d : 0.0f) + (float)(sum * (double)q.scale);
}
}  // namespace

// the slice plan of a head stream: 4 slices per CU (round 6).  With one 256-thread workgroup per CU (rounds 3-5: `sp` slices) a
// CU had 4-16 KiB of loads in flight and the streams ran at 1.5-2.3 TB/s (28 + 21 us coarse, 44 + 31 us fine: 4 % of the step)
int nsr::panel_wsums(hipStream_t st, int R, int NW, const char* panel, int64_t P, const float* w, int w_stride, float* partial,
                     int* slices) {
  if (!((R == 128 && NW == 3) || (R == 256 && NW == 1))) return NSR_ERR_UNSUPPORTED;
  const int64_t n_pg = P / 32;
  const int hs = (int)(n_pg < 1024 ? (n_pg < 1 ? 1 : n_pg) : 1024);
  const int64_t per = (n_pg + hs - 1) / hs;
  if (R == 128) hipLaunchKernelGGL((panel_wsums_kernel<128, 3>), dim3(hs), dim3(256), 0, st, panel, P, w, w_stride, per, partial);
  else hipLaunchKernelGGL((panel_wsums_kernel<256, 1>), dim3(hs), dim3(256), 0, st, panel, P, w, w_stride, per, partial);
  NSR_CHECK_LAUNCH();
  *slices = hs;
  return NSR_OK;
}

// nothing is launched unless every job fits the kernel: a job beyond its grid row would be cut off silently
int nsr::finish_jobs(hipStream_t st, const FinishJob* j, int n) {
  if (!j || n < 1 || n > kMaxFinishJobs) return NSR_ERR_INVALID_ARG;
  FinishJobs jobs{};
  for (int i = 0; i < n; ++i) {
    const FinishJob& q = j[i];
    if (q.kind < 0 || q.kind > 2 || !q.dst || !q.partial || q.rows < 0 || q.cols < 0 || q.splits < 0) return NSR_ERR_INVALID_ARG;
    if (q.kind == 2 ? q.rows > 4 : ((q.kind == 0 || q.splits <= 64) && (int64_t)q.rows * q.cols > 65536)) return NSR_ERR_UNSUPPORTED;
    jobs.j[i] = q;
  }
  jobs.n = n;
  hipLaunchKernelGGL(finish_jobs_kernel, dim3(256, n), dim3(256), 0, st, jobs);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

// zpan = the forward activations, dpan = the input gradients at each point's power-of-two scale (k.pscale); d_rgb_pre and
// d_sigma in k.d4 (P, 4).  ~256 workgroups share the products' point groups by bytes: a 256 x 256 product ends up with ~21
// partial tiles instead of the 256 a launch of its own needed to fill the chip -- 12 x fewer partial sums to write, and for
// finish_jobs_kernel to read back.
int nsr::chain_weight_grads(hipStream_t st, const Work& k, int64_t P, int64_t n_rays, float* const* g, int acc) {
  const int sp = n_splits(P);   // the workspace's slots are sized for the largest pass (work_floats): at least this one's
  constexpr int64_t kTile = (int64_t)256 * 256;
  const int64_t n_groups = ((P + 127) / 128) * 4;
  auto panel = [&](char* set, int p) { return set + panel_offset_bytes(n_groups, p); };
  struct { FinishJob j[kMaxFinishJobs]; int n; } jobs{};
  WgradJobs wj{};
  int fin_tiles[kMaxWgradJobs], fin_rows[kMaxWgradJobs];   // the finish jobs of product p's partial tiles / row sums (-1: none)
  bool overflow = false;
  // a second pass, executed by finish_jobs_kernel at the end; returns its index
  auto finish = [&](int kind, float* dst, int rows, int cols, const float* partial, int splits, int64_t stride) {
    FinishJob& q = jobs.j[jobs.n];
    q.kind = kind; q.dst = dst; q.rows = rows; q.cols = cols; q.partial = partial; q.splits = splits; q.stride = stride;
    q.accumulate = acc; q.scale = 1.0f;
    return jobs.n++;
  };
  // product of gradient panel a with forward panel b, an entry of the job table, and the second pass that places its tiles
  // (rows x cols at dst[:, dc0:]; enc_rows: enc_panel_row).  Slots are handed out after the plan.  Returns the product's index
  auto product = [&](int a_panel, int b_panel, float* dst, int dst_ld, int dc0, int rows, int cols, int p_ld, int enc_rows) {
    overflow |= wj.n == kMaxWgradJobs;
    const int pj = overflow ? wj.n - 1 : wj.n++;
    WgradArgs& w = wj.j[pj].w;
    w.A = panel(k.dpan, a_panel); w.M = panel_rows(a_panel); w.a_gbytes = (int64_t)kPanelRowBytes * w.M;
    w.B = panel(k.kept.zpan, b_panel); w.N = panel_rows(b_panel); w.b_gbytes = (int64_t)kPanelRowBytes * w.N;
    w.a_max_bits = k.gmax + a_panel;
    w.a_pscale = k.pscale + (int64_t)a_panel * n_groups * 32;
    w.split_stride = kTile;
    w.partial = k.slots;                       // placeholder (validated non-null); the real slots after the plan
    fin_tiles[pj] = finish(0, dst, rows, cols, nullptr, 0, kTile);
    fin_rows[pj] = -1;
    FinishJob& q = jobs.j[fin_tiles[pj]];
    q.dst_ld = dst_ld; q.dc0 = dc0; q.p_ld = p_ld; q.enc_rows = enc_rows;
    return pj;
  };
  // product pj also sums the rows of its gradient panel: the bias gradient (`rows` values)
  auto bias = [&](int pj, float* dst, int rows) {
    wj.j[pj].w.row_sums = k.row_part;          // placeholder, like `partial`
    fin_rows[pj] = finish(1, dst, rows, 1, nullptr, 0, 0);
  };
  // the two head streams (panel_wsums): the slot the partials go to holds sp x 256 x 256 floats, a slice writes 384 or 256
  int hs = 0;
  // rgb head: d_rgb_pre^T relu(zcc), a stream over the panel; its bias from the per-ray partials of composite_bwd_kernel
  float* part = k.slots;
  NSR_TRY(panel_wsums(st, 128, 3, panel(k.kept.zpan, 9), P, k.d4, 4, part, &hs));
  finish(1, g[kRgbW], 3 * 128, 1, part, hs, 0);
  finish(2, g[kRgbB], 3, 1, k.bias_part, (int)n_rays, 4);
  // dir_encoding: dzc^T [g | de]
  bias(product(9, 8, g[kDirW], 283, 0, 128, 256, kW, 0), g[kDirB], kDirOut);
  product(9, 11, g[kDirW], 283, 256, 128, 27, kPe, 2);
  // xyz_encoding_final: dg^T relu(z8); sigma: d_sigma^T relu(z8)
  bias(product(8, 7, g[kFinalW], 256, 0, 256, 256, kW, 0), g[kFinalB], kW);
  part = k.slots + sp * kTile;
  NSR_TRY(panel_wsums(st, 256, 1, panel(k.kept.zpan, 7), P, k.d4 + 3, 4, part, &hs));
  finish(1, g[kSigmaW], 256, 1, part, hs, 0);
  finish(2, g[kSigmaB], 1, 1, k.bias_part + 3, (int)n_rays, 4);
  // trunk layers 8..1: dz_L^T (input of layer L); layers 1 and 5 read the encoded position (panel 10, 64 rows in register order)
  for (int L = 8; L >= 1; --L) {
    float* gw = g[2 * (L - 1)];
    int pj = -1;
    if (L > 1) pj = product(L - 1, L - 2, gw, L == 5 ? 319 : 256, L == 5 ? 63 : 0, 256, 256, kW, 0);
    if (L == 1 || L == 5) {
      const int pe = product(L - 1, 10, gw, L == 1 ? 63 : 319, 0, 256, 63, kPe, 1);
      if (L == 1) pj = pe;
    }
    bias(pj, g[2 * (L - 1) + 1], kW);
  }
  if (overflow) return NSR_ERR_LAUNCH;   // cannot happen: twelve products, and 26 second passes <= kMaxFinishJobs
  // as many workgroups as there are CUs -- fewer for a small pass, so that the partial tiles fit the slots the
  // workspace holds and a workgroup always has a few point groups to sweep
  const int want = 10 * (sp - 1);
  const int n_wg = wgrad_jobs_plan(wj, P, want < 1 ? 1 : (want > 256 ? 256 : want));
  float* next_big = k.slots + 2 * sp * kTile;                       // behind the two head slots taken above
  float* next_row = k.row_part;
  for (int p = 0; p < wj.n; ++p) {
    WgradJob& q = wj.j[p];
    FinishJob& tiles = jobs.j[fin_tiles[p]];
    tiles.partial = q.w.partial = next_big;
    tiles.splits = q.n_slots;
    next_big += q.n_slots * kTile;
    if (fin_rows[p] < 0) continue;
    FinishJob& sums = jobs.j[fin_rows[p]];
    sums.partial = q.w.row_sums = next_row;
    sums.splits = q.n_slots;
    next_row += (int64_t)q.n_slots * q.w.M;
  }
  if (next_big > k.slots + kChainSlots * sp * kTile || next_row > k.row_part + (int64_t)kChainRowSlots * sp * 256)
    return NSR_ERR_WORKSPACE;   // cannot happen (see `want`)
  NSR_TRY(wgrad_jobs_f16(wj, n_wg, st));
  return finish_jobs(st, jobs.j, jobs.n);
}
