// What the eval forward (nsr_refine.hip) and the train-mode pair (nsr_refine_train.hip) of the refinement network share:
// the layer table, the tap-major weight re-layout and the explicit im2col of a 3x3 / pad 1 convolution.
#pragma once
#include "nsr_common.h"
#include "nsr_gemm.h"
#include "../../include/nsr_refine.h"

namespace {

using nsr::kActRelu;
using nsr::kActTanh;
using nsr::kSplitScale;

struct Layer {
  int cin, cout, stride, bn, up, act;
};
// forward order = state_dict order (E.conv1..7, D.conv1, 2, 2_up, 3, 4, 4_up, 5, 6, 6_up, 7, 8, 9).
// Variant 0: Model_VNPCAT_Decoder (decoder inputs [.. | F_synth_i | F_max_i]); variant 1: --not_use_ref,
// Model_VNPCAT_Decoder_NoPooling (networks.py:866-945: the same layers without the F_max_i channels, i.e. D.conv1,
// D.conv3, D.conv5 and D.conv7 take 512 / 1024 / 512 / 256 input channels).
constexpr Layer kLayersV[2][NSR_REFINE_N_LAYERS] = {{
    {3, 128, 1, 0, 0, kActRelu},    {128, 128, 1, 1, 0, kActRelu}, {128, 256, 2, 1, 0, kActRelu},
    {256, 256, 1, 1, 0, kActRelu},  {256, 512, 2, 1, 0, kActRelu}, {512, 512, 1, 1, 0, kActRelu},
    {512, 512, 2, 1, 0, kActRelu},
    {1024, 512, 1, 1, 0, kActRelu}, {512, 512, 1, 1, 0, kActRelu}, {512, 512, 1, 1, 1, kActRelu},
    {1536, 512, 1, 1, 0, kActRelu}, {512, 512, 1, 1, 0, kActRelu}, {512, 256, 1, 1, 1, kActRelu},
    {768, 256, 1, 1, 0, kActRelu},  {256, 256, 1, 1, 0, kActRelu}, {256, 128, 1, 1, 1, kActRelu},
    {384, 128, 1, 1, 0, kActRelu},  {128, 128, 1, 1, 0, kActRelu}, {128, 3, 1, 0, 0, kActTanh},
}, {
    {3, 128, 1, 0, 0, kActRelu},    {128, 128, 1, 1, 0, kActRelu}, {128, 256, 2, 1, 0, kActRelu},
    {256, 256, 1, 1, 0, kActRelu},  {256, 512, 2, 1, 0, kActRelu}, {512, 512, 1, 1, 0, kActRelu},
    {512, 512, 2, 1, 0, kActRelu},
    {512, 512, 1, 1, 0, kActRelu},  {512, 512, 1, 1, 0, kActRelu}, {512, 512, 1, 1, 1, kActRelu},
    {1024, 512, 1, 1, 0, kActRelu}, {512, 512, 1, 1, 0, kActRelu}, {512, 256, 1, 1, 1, kActRelu},
    {512, 256, 1, 1, 0, kActRelu},  {256, 256, 1, 1, 0, kActRelu}, {256, 128, 1, 1, 1, kActRelu},
    {256, 128, 1, 1, 0, kActRelu},  {128, 128, 1, 1, 0, kActRelu}, {128, 3, 1, 0, 0, kActTanh},
}};
constexpr int pad32(int n) { return (n + 31) & ~31; }

constexpr float kBnEps = 1e-5f;   // nn.BatchNorm2d default

// W'[n][(ky * 3 + kx) * cin + c] = s_n * W[n][c][ky][kx],  b'[n] = (b[n] - mean[n]) * s_n + beta[n],
// s_n = gamma[n] / sqrt(var[n] + eps)  (1 and the plain bias without a BatchNorm); padding rows / columns are zero
__global__ void pack_conv_kernel(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ gamma,
                                 const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ var,
                                 int cin, int cout, int kp, int np, int f16x3, float* __restrict__ dst) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nw = (int64_t)np * kp;
  if (idx >= nw + np) return;
  if (idx < nw) {
    const int n = (int)(idx / kp), k = (int)(idx % kp);
    float v = 0.0f;
    if (n < cout && k < 9 * cin) {
      const int tap = k / cin, c = k % cin;
      const float s = gamma ? __fdiv_rn(gamma[n], sqrtf(__fadd_rn(var[n], kBnEps))) : 1.0f;
      v = __fmul_rn(s, w[((int64_t)n * cin + c) * 9 + tap]);
    }
    if (f16x3) {   // [hi halves (np x kp)] [lo halves (np x kp)] [bias]: the same number of bytes as the fp32 layout
      v *= kSplitScale;   // see nsr_gemm.h: keeps the lo half clear of fp16's subnormal floor; undone by acc_scale
      const _Float16 hi = (_Float16)v;
      const _Float16 lo = (_Float16)(v - (float)hi);
      unsigned short* d16 = reinterpret_cast<unsigned short*>(dst);
      d16[idx] = __builtin_bit_cast(unsigned short, hi);
      d16[nw + idx] = __builtin_bit_cast(unsigned short, lo);
    } else {
      dst[idx] = v;
    }
  } else {
    const int n = (int)(idx - nw);
    float v = 0.0f;
    if (n < cout) {
      if (gamma) {
        const float s = __fdiv_rn(gamma[n], sqrtf(__fadd_rn(var[n], kBnEps)));
        v = __fadd_rn(__fmul_rn(__fsub_rn(b[n], mean[n]), s), beta[n]);
      } else {
        v = b[n];
      }
    }
    dst[idx] = v;
  }
}

// im2col of a 3x3 / pad 1 convolution.  Source: NHWC with row stride `ld` (channels [0, cin) of a possibly wider
// buffer), or NCHW (first layer: the reference's input tensor); `up`: the source is read through a nearest x2 upsample.
// col (M, kp), M = n_img * Ho * Wo; one thread per (row, tap, channel quad)
template <bool NCHW>
__global__ void __launch_bounds__(256) im2col_kernel(const float* __restrict__ src, int64_t ld, int cin, int n_img, int Hs,
                                                     int Ws, int stride, int up, int Ho, int Wo, int kp,
                                                     float* __restrict__ col) {
  const int q_per_row = kp / 4;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)n_img * Ho * Wo * q_per_row;
  if (idx >= total) return;
  const int64_t m = idx / q_per_row;
  const int k0 = (int)(idx % q_per_row) * 4;
  const int ox = (int)(m % Wo), oy = (int)((m / Wo) % Ho), img = (int)(m / ((int64_t)Wo * Ho));
  const int Hin = up ? 2 * Hs : Hs, Win = up ? 2 * Ws : Ws;     // extent the convolution sees
  float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (!NCHW && (cin & 3) == 0) {
    if (k0 < 9 * cin) {
      const int tap = k0 / cin, c = k0 % cin;
      const int iy = oy * stride + tap / 3 - 1, ix = ox * stride + tap % 3 - 1;
      if (iy >= 0 && iy < Hin && ix >= 0 && ix < Win) {
        const int sy = up ? iy >> 1 : iy, sx = up ? ix >> 1 : ix;
        const float4 t = *reinterpret_cast<const float4*>(src + (((int64_t)img * Hs + sy) * Ws + sx) * ld + c);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = k0 + e;
      if (k >= 9 * cin) continue;
      const int tap = k / cin, c = k % cin;
      const int iy = oy * stride + tap / 3 - 1, ix = ox * stride + tap % 3 - 1;
      if (iy < 0 || iy >= Hin || ix < 0 || ix >= Win) continue;
      const int sy = up ? iy >> 1 : iy, sx = up ? ix >> 1 : ix;
      v[e] = NCHW ? src[(((int64_t)img * cin + c) * Hs + sy) * Ws + sx]
                  : src[(((int64_t)img * Hs + sy) * Ws + sx) * ld + c];
    }
  }
  *reinterpret_cast<float4*>(col + m * kp + k0) = make_float4(v[0], v[1], v[2], v[3]);
}

}  // namespace
