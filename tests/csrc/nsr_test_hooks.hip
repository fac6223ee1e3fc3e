// Test hooks (tests/hooks.py): default-visibility C wrappers over the library-internal matrix kernels, linked together with the
// UNCHANGED product objects into a second shared object (nerf_sr_amd/build.py build_test_hooks -> ab/libnsr_testhooks.so).
// Not part of libnsr.so; nothing here is declared in include/.  The wrappers marshal arguments and do no arithmetic.  The
// one kernel, pack_panel_kernel, is a WRITER of the 2-byte training panels: it follows the layout documented in
// nsr_f16x3_core.h ("Training panels") with the product's own helpers (unit_voff, kPanelRowBytes) and knows nothing of how
// nsr_wgrad_f16.hip reads a panel back -- the tests thereby pin the pair "documented writer layout <-> reader".
#include <stddef.h>
#include "nsr_gemm.h"
#include "nsr_f16x3_core.h"
#include "nsr_train_work.h"

#define NSR_TEST_API extern "C" __attribute__((visibility("default")))

using namespace nsr;

NSR_TEST_API int nsr_test_gemm(const GemmArgs* g, void* stream) {
  if (!g) return NSR_ERR_INVALID_ARG;
  return gemm(*g, nsr_stream(stream));
}

NSR_TEST_API int nsr_test_gemm_f16x3(const GemmF16Args* a, void* stream) {
  if (!a) return NSR_ERR_INVALID_ARG;
  return gemm_f16x3(*a, nsr_stream(stream));
}

NSR_TEST_API int nsr_test_wgrad_plan(WgradJobs* jobs, int64_t P, int n_wg) {
  if (!jobs) return NSR_ERR_INVALID_ARG;
  return wgrad_jobs_plan(*jobs, P, n_wg);
}

NSR_TEST_API int nsr_test_wgrad_jobs(const WgradJobs* jobs, int n_wg, void* stream) {
  if (!jobs) return NSR_ERR_INVALID_ARG;
  return wgrad_jobs_f16(*jobs, n_wg, nsr_stream(stream));
}

// sizeof / offsetof of the argument structs, in declaration order, so that the ctypes mirrors are checked and not trusted:
// which = 0 GemmArgs, 1 GemmF16Args, 2 WgradArgs, 3 WgradJob, 4 WgradJobs, 5 ConvGather, 6 FinishJob (nsr_train_work.h).  out[0] = sizeof, out[1..] = the
// offsets; returns the number of entries (written up to cap), -1 for an unknown struct.
NSR_TEST_API int nsr_test_layout(int which, int64_t* out, int cap) {
  int64_t v[32];
  int n = 0;
#define NSR_SZ(T) v[n++] = (int64_t)sizeof(T)
#define NSR_OFF(T, f) v[n++] = (int64_t)offsetof(T, f)
  switch (which) {
    case 0:
      NSR_SZ(GemmArgs);
      NSR_OFF(GemmArgs, A); NSR_OFF(GemmArgs, lda); NSR_OFF(GemmArgs, a_kmajor);
      NSR_OFF(GemmArgs, B); NSR_OFF(GemmArgs, ldb); NSR_OFF(GemmArgs, b_kmajor);
      NSR_OFF(GemmArgs, C); NSR_OFF(GemmArgs, ldc); NSR_OFF(GemmArgs, Ct); NSR_OFF(GemmArgs, ldct);
      NSR_OFF(GemmArgs, bias); NSR_OFF(GemmArgs, mask); NSR_OFF(GemmArgs, ldm);
      NSR_OFF(GemmArgs, M); NSR_OFF(GemmArgs, N); NSR_OFF(GemmArgs, K);
      NSR_OFF(GemmArgs, n_valid); NSR_OFF(GemmArgs, act); NSR_OFF(GemmArgs, splits); NSR_OFF(GemmArgs, split_stride);
      NSR_OFF(GemmArgs, col_sums); NSR_OFF(GemmArgs, acc_scale);
      break;
    case 1:
      NSR_SZ(GemmF16Args);
      NSR_OFF(GemmF16Args, g); NSR_OFF(GemmF16Args, Bh); NSR_OFF(GemmF16Args, Bl); NSR_OFF(GemmF16Args, ldbh);
      NSR_OFF(GemmF16Args, conv); NSR_OFF(GemmF16Args, Ah); NSR_OFF(GemmF16Args, a_plane); NSR_OFF(GemmF16Args, Ch);
      NSR_OFF(GemmF16Args, c_plane); NSR_OFF(GemmF16Args, group); NSR_OFF(GemmF16Args, Mh); NSR_OFF(GemmF16Args, m_plane);
      NSR_OFF(GemmF16Args, ldm); NSR_OFF(GemmF16Args, Bs);
      break;
    case 2:
      NSR_SZ(WgradArgs);
      NSR_OFF(WgradArgs, A); NSR_OFF(WgradArgs, a_gbytes); NSR_OFF(WgradArgs, M);
      NSR_OFF(WgradArgs, B); NSR_OFF(WgradArgs, b_gbytes); NSR_OFF(WgradArgs, N);
      NSR_OFF(WgradArgs, a_max_bits); NSR_OFF(WgradArgs, a_pscale); NSR_OFF(WgradArgs, partial);
      NSR_OFF(WgradArgs, split_stride); NSR_OFF(WgradArgs, row_sums);
      break;
    case 3:
      NSR_SZ(WgradJob);
      NSR_OFF(WgradJob, w); NSR_OFF(WgradJob, cost0); NSR_OFF(WgradJob, cost); NSR_OFF(WgradJob, w_first); NSR_OFF(WgradJob, n_slots);
      break;
    case 4:
      NSR_SZ(WgradJobs);
      NSR_OFF(WgradJobs, j); NSR_OFF(WgradJobs, n); NSR_OFF(WgradJobs, n_groups); NSR_OFF(WgradJobs, total_cost);
      NSR_OFF(WgradJobs, per_wg);
      v[n++] = kMaxWgradJobs;
      break;
    case 5:
      NSR_SZ(ConvGather);
      NSR_OFF(ConvGather, cin); NSR_OFF(ConvGather, Hs); NSR_OFF(ConvGather, Ws); NSR_OFF(ConvGather, Ho); NSR_OFF(ConvGather, Wo);
      NSR_OFF(ConvGather, stride); NSR_OFF(ConvGather, up);
      break;
    case 6:
      NSR_SZ(FinishJob);
      NSR_OFF(FinishJob, dst); NSR_OFF(FinishJob, partial); NSR_OFF(FinishJob, stride); NSR_OFF(FinishJob, kind);
      NSR_OFF(FinishJob, dst_ld); NSR_OFF(FinishJob, dc0); NSR_OFF(FinishJob, rows); NSR_OFF(FinishJob, cols);
      NSR_OFF(FinishJob, splits); NSR_OFF(FinishJob, p_ld); NSR_OFF(FinishJob, accumulate); NSR_OFF(FinishJob, enc_rows);
      NSR_OFF(FinishJob, scale);
      break;
    default:
      return -1;
  }
#undef NSR_SZ
#undef NSR_OFF
  for (int i = 0; i < n && i < cap; ++i) out[i] = v[i];
  return n;
}

namespace {

// One thread = one lane (m, h) of one unit: the 16 bytes that lane of a chain kernel stores (unit_store).  src is a plain
// row-major (P, ld) matrix of fp16 bit patterns, row = point, column = panel row (feature); the panel's point group g starts
// at g * gbytes, its 32-row block blk 32 * blk * kPanelRowBytes further on, unit u another KiB on.
__global__ void pack_panel_kernel(const unsigned short* __restrict__ src, int64_t ld, int64_t n_groups, int rows, char* panel,
                                  int64_t gbytes) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t units = n_groups * (rows / 16);
  if (t >= units * 64) return;
  const int lane = (int)(t & 63), m = lane & 31, h = lane >> 5;
  const int64_t unit = t >> 6, g = unit / (rows / 16);
  const int ub = (int)(unit % (rows / 16)), blk = ub >> 1, u = ub & 1;
  const unsigned short* p = src + (32 * g + m) * ld + 32 * blk + 16 * u + 4 * h;   // features 16u + 4h + {0..3}, then + 8
  u32x4 v;
  v[0] = (unsigned)p[0] | ((unsigned)p[1] << 16);
  v[1] = (unsigned)p[2] | ((unsigned)p[3] << 16);
  v[2] = (unsigned)p[8] | ((unsigned)p[9] << 16);
  v[3] = (unsigned)p[10] | ((unsigned)p[11] << 16);
  char* dst = panel + g * gbytes + (int64_t)32 * blk * kPanelRowBytes + 1024 * u + unit_voff(m, h, u);
  *reinterpret_cast<u32x4*>(dst) = v;
}

}  // namespace

// (P, rows) fp16 matrix, row stride ld halves -> panel rows [0, rows) of the point groups [0, P / 32) of a panel whose groups
// lie gbytes apart (>= 64 rows: a slice of a taller panel); P % 32 == 0, rows % 32 == 0
NSR_TEST_API int nsr_test_pack_panel(const void* src, int64_t ld, int64_t P, int rows, void* panel, int64_t gbytes, void* stream) {
  if (!src || !panel || P < 0 || (P % 32) || rows <= 0 || (rows % 32) || ld < rows) return NSR_ERR_INVALID_ARG;
  if (gbytes < (int64_t)rows * kPanelRowBytes || (gbytes % 1024) || (reinterpret_cast<uintptr_t>(panel) & 15)) return NSR_ERR_INVALID_ARG;
  if (P == 0) return NSR_OK;
  const int64_t threads = (P / 32) * (rows / 16) * 64;
  hipLaunchKernelGGL(pack_panel_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, nsr_stream(stream),
                     static_cast<const unsigned short*>(src), ld, P / 32, rows, static_cast<char*>(panel), gbytes);
  if (hipGetLastError() != hipSuccess) return NSR_ERR_LAUNCH;
  return NSR_OK;
}
