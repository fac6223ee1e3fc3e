// R1-R4 per pixel: the one ray of HR pixel (px, py) -- camera-space direction, rotation into the world frame,
// normalisation, optional NDC projection -- shared by gen_rays_kernel (nsr_rays.hip: one pose, passed by value) and
// rayset_batch_kernel (nsr_data.hip: poses in device memory).  fp32 arithmetic in the reference's operation order
// (models/utils.py:98-196); both units are compiled with -ffp-contract=off, and every operation below is an explicit
// round-to-nearest intrinsic or an fma the reference's matmul performs as well, so the two kernels agree bit for bit.
#pragma once
#include "nsr_common.h"

// option word of nsr_gen_rays_opt / struct nsr_rayset (include/nsr_data.h)
constexpr unsigned kRayNoPixelCentres = 1u, kRayUnifiedDir = 2u;

struct NsrRayCam {
  int H, W, s, ndc;
  float focal, half_w, half_h;   // W/2, H/2 as fp32
  float ndc_ax, ndc_ay;          // -1/(W/(2f)), -1/(H/(2f)) evaluated in double on the host
  float near_, far_;
  float pix_off;                 // 0.5, or 0 under --use_pixel_centers false
  int unified;                   // --unified_dir: the camera-space direction is the LR pixel's (llff_downX_dataset.py:274-276)
  float u_focal, u_half_w, u_half_h;   // focal // s, (W // s) / 2, (H // s) / 2
};

// host: fills everything but the options' fields from the arguments of nsr_gen_rays*; returns false on a bad argument
static inline bool nsr_ray_cam(NsrRayCam& a, int H, int W, double focal, int s, int ndc, float near_, float far_,
                               unsigned options) {
  if (H <= 0 || W <= 0 || s <= 0 || !(focal > 0.0) || H % s != 0 || W % s != 0) return false;
  if (options & ~(kRayNoPixelCentres | kRayUnifiedDir)) return false;
  a.H = H; a.W = W; a.s = s; a.ndc = ndc;
  a.focal = (float)focal;
  a.half_w = (float)(W / 2.0);
  a.half_h = (float)(H / 2.0);
  a.ndc_ax = (float)(-1.0 / (W / (2.0 * focal)));
  a.ndc_ay = (float)(-1.0 / (H / (2.0 * focal)));
  a.near_ = near_; a.far_ = far_;
  a.pix_off = (options & kRayNoPixelCentres) ? 0.0f : 0.5f;
  a.unified = (options & kRayUnifiedDir) ? 1 : 0;
  const double uf = floor(focal / s);      // Python's float // int
  a.u_focal = (float)uf;
  a.u_half_w = (float)((W / s) / 2.0);
  a.u_half_h = (float)((H / s) / 2.0);
  if (a.unified && !(uf > 0.0)) return false;
  return true;
}

// c2w: 12 floats, row-major (3, 4).  out0 = (o.x, o.y, o.z, d.x), out1 = (d.y, d.z, near, far): one ray row.
__device__ __forceinline__ void nsr_raygen_pixel(const NsrRayCam& a, const float* c2w, int px, int py, float4& out0,
                                                 float4& out1) {
  // camera-space direction through the pixel centre (of the LR pixel under --unified_dir)
  float cx, cy;
  if (a.unified) {
    cx = __fdiv_rn(__fsub_rn(__fadd_rn((float)(px / a.s), a.pix_off), a.u_half_w), a.u_focal);
    cy = -__fdiv_rn(__fsub_rn(__fadd_rn((float)(py / a.s), a.pix_off), a.u_half_h), a.u_focal);
  } else {
    cx = __fdiv_rn(__fsub_rn(__fadd_rn((float)px, a.pix_off), a.half_w), a.focal);
    cy = -__fdiv_rn(__fsub_rn(__fadd_rn((float)py, a.pix_off), a.half_h), a.focal);
  }
  const float cz = -1.0f;
  // rotate into the world frame, normalise
  float d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
    d[k] = fmaf(cz, c2w[4 * k + 2], fmaf(cy, c2w[4 * k + 1], __fmul_rn(cx, c2w[4 * k + 0])));
  const float nrm = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(d[0], d[0]), __fmul_rn(d[1], d[1])), __fmul_rn(d[2], d[2])));
  d[0] = __fdiv_rn(d[0], nrm); d[1] = __fdiv_rn(d[1], nrm); d[2] = __fdiv_rn(d[2], nrm);
  float o[3] = {c2w[3], c2w[7], c2w[11]};
  float nr = a.near_, fr = a.far_;
  if (a.ndc) {
    // shift the origin to the near plane (near = 1.0), then project
    const float t = __fdiv_rn(-__fadd_rn(1.0f, o[2]), d[2]);
    o[0] = __fadd_rn(o[0], __fmul_rn(t, d[0]));
    o[1] = __fadd_rn(o[1], __fmul_rn(t, d[1]));
    o[2] = __fadd_rn(o[2], __fmul_rn(t, d[2]));
    const float ox_oz = __fdiv_rn(o[0], o[2]);
    const float oy_oz = __fdiv_rn(o[1], o[2]);
    const float o0 = __fmul_rn(a.ndc_ax, ox_oz);
    const float o1 = __fmul_rn(a.ndc_ay, oy_oz);
    const float o2 = __fadd_rn(1.0f, __fdiv_rn(2.0f, o[2]));
    const float d0 = __fmul_rn(a.ndc_ax, __fsub_rn(__fdiv_rn(d[0], d[2]), ox_oz));
    const float d1 = __fmul_rn(a.ndc_ay, __fsub_rn(__fdiv_rn(d[1], d[2]), oy_oz));
    const float d2 = __fsub_rn(1.0f, o2);
    o[0] = o0; o[1] = o1; o[2] = o2;
    d[0] = d0; d[1] = d1; d[2] = d2;
    nr = 0.0f; fr = 1.0f;
  }
  out0 = make_float4(o[0], o[1], o[2], d[0]);
  out1 = make_float4(d[1], d[2], nr, fr);
}
