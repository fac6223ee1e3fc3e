// The host-only unit of the public ABI (include/nsr.h); no kernel is defined here.
//   * The precision dispatcher of the inference MLP: packing, the blob's status and option words, nsr_mlp_forward,
//     nsr_render_rays and the fused render + composite entry points.  It owns the argument checks and picks the family;
//     the launchers are the fp32, split-fp16 and 16-bit units' (nsr_mlp_units.h).
//   * D3: the fused forward_rays driver (models/nerf_downX_model.py:280-324, eval mode) — one enqueue sequence for the
//     WHOLE ray batch: no ray_chunk / point_chunk slicing (288 GB of HBM hold every intermediate of a full image), no host
//     synchronisation (the reference syncs twice per 4096-ray chunk, nerf_downX_model.py:273,284).
#include <math.h>
#include "nsr_mlp_units.h"

extern "C" int nsr_version(void) { return NSR_VERSION; }

extern "C" const char* nsr_status_string(int status) {
  switch (status) {
    case NSR_OK: return "ok";
    case NSR_ERR_INVALID_ARG: return "invalid argument (null / negative size / misaligned pointer)";
    case NSR_ERR_UNSUPPORTED: return "configuration outside the built path (sample count, degree or precision)";
    case NSR_ERR_LAUNCH: return "HIP kernel launch failed";
    case NSR_ERR_WORKSPACE: return "workspace too small";
    case NSR_ERR_RANGE: return "a weight is non-finite or outside the operand range of the precision (use NSR_FP32)";
    default: return "unknown nsr status";
  }
}

// ---------------------------------------------------------------------------
// the precision dispatcher: argument checks in the order include/nsr.h's statuses depend on, then the family's launcher
// ---------------------------------------------------------------------------
static inline bool precision_built(int precision) {
  return precision == NSR_FP32 || precision == NSR_F16X3 || precision == NSR_BF16 || precision == NSR_F16;
}
static inline bool precision_h1(int precision) { return precision == NSR_BF16 || precision == NSR_F16; }

NSR_INTERNAL size_t nsr_payload_bytes(int precision) {
  if (precision == NSR_FP32) return nsr_fp32_packed_bytes();
  if (precision == NSR_F16X3) return nsr_f16x3_packed_bytes();
  if (precision_h1(precision)) return nsr_h1_packed_bytes();
  return 0;
}

extern "C" size_t nsr_packed_weights_bytes(int precision) {
  const size_t payload = nsr_payload_bytes(precision);
  return payload ? nsr_blob_tail_offset(payload) + kBlobTailBytes : 0;
}

extern "C" int nsr_pack_weights_async(const float* const* w, void* packed_dev, int precision, void* stream) {
  if (!w || !packed_dev) return NSR_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(packed_dev) & 15) != 0) return NSR_ERR_INVALID_ARG;
  if (!precision_built(precision)) return NSR_ERR_UNSUPPORTED;
  for (int i = 0; i < NSR_N_STATE_TENSORS; ++i)
    if (!w[i]) return NSR_ERR_INVALID_ARG;
  unsigned* tail = nsr_blob_tail(packed_dev, precision);
  if (hipMemsetAsync(tail, 0, kBlobTailBytes, nsr_stream(stream)) != hipSuccess) return NSR_ERR_LAUNCH;
  // range check of the 24 tensors into the cleared tail (include/nsr.h, nsr_pack_weights)
  const int rc = nsr_check_weights_range(w, precision, tail, stream);
  if (rc != NSR_OK) return rc;
  // (folds xyz_encoding_final into dir_encoding first; the folded matrix is range-checked like the 24 tensors)
  if (precision == NSR_F16X3) return nsr_f16x3_pack(w, packed_dev, nsr_weight_limit(precision), tail, stream);
  if (precision_h1(precision)) return nsr_h1_pack(precision == NSR_BF16, w, packed_dev, stream);
  return nsr_fp32_pack(w, packed_dev, stream);
}

extern "C" int nsr_weights_status(const void* packed_dev, int precision, int clear, unsigned* flags_out, void* stream) {
  if (!packed_dev || !flags_out) return NSR_ERR_INVALID_ARG;
  if (!precision_built(precision)) return NSR_ERR_UNSUPPORTED;
  unsigned* tail = nsr_blob_tail(packed_dev, precision);
  hipStream_t st = nsr_stream(stream);
  unsigned host = 0;
  if (hipMemcpyAsync(&host, tail, sizeof(unsigned), hipMemcpyDeviceToHost, st) != hipSuccess) return NSR_ERR_LAUNCH;
  if (clear && hipMemsetAsync(tail, 0, sizeof(unsigned), st) != hipSuccess) return NSR_ERR_LAUNCH;
  if (hipStreamSynchronize(st) != hipSuccess) return NSR_ERR_LAUNCH;
  *flags_out = host;
  return NSR_OK;
}

extern "C" int nsr_pack_weights(const float* const* w, void* packed_dev, int precision, void* stream) {
  const int rc = nsr_pack_weights_async(w, packed_dev, precision, stream);
  if (rc != NSR_OK) return rc;
  unsigned flags = 0;
  const int rs = nsr_weights_status(packed_dev, precision, 0, &flags, stream);
  if (rs != NSR_OK) return rs;
  return (flags & NSR_FLAG_WEIGHT_RANGE) ? NSR_ERR_RANGE : NSR_OK;
}

extern "C" int nsr_weights_set_options(void* packed_dev, int precision, unsigned options, void* stream) {
  static_assert(kOptGamma == NSR_OPT_GAMMA && kOptColorNone == NSR_OPT_COLOR_NONE, "option bits of include/nsr.h");
  if (!packed_dev || (options & ~(NSR_OPT_GAMMA | NSR_OPT_COLOR_NONE)) != 0u) return NSR_ERR_INVALID_ARG;
  if (!precision_built(precision)) return NSR_ERR_UNSUPPORTED;
  unsigned* tail = nsr_blob_tail(packed_dev, precision);
  if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(tail + 1), (int)options, 1, nsr_stream(stream)) != hipSuccess)
    return NSR_ERR_LAUNCH;
  return NSR_OK;
}
extern "C" int nsr_weights_set_gamma(void* packed_dev, int precision, int enable, void* stream) {
  return nsr_weights_set_options(packed_dev, precision, enable ? NSR_OPT_GAMMA : 0u, stream);
}

extern "C" int nsr_mlp_forward(const void* packed_dev, int precision, const float* x, int64_t P, int sigma_only,
                               float* out, void* stream) {
  if (P < 0 || !packed_dev) return NSR_ERR_INVALID_ARG;
  if (!precision_built(precision)) return NSR_ERR_UNSUPPORTED;
  if (P == 0) return NSR_OK;   // empty batch: nothing to read or write (pointers may be null)
  if (!x || !out) return NSR_ERR_INVALID_ARG;
  if (!sigma_only && (reinterpret_cast<uintptr_t>(out) & 15) != 0) return NSR_ERR_INVALID_ARG;
  unsigned* tail = nsr_blob_tail(packed_dev, precision);
  if (precision == NSR_F16X3) return nsr_f16x3_mlp_forward(packed_dev, x, P, sigma_only, out, tail, stream);
  if (precision_h1(precision)) return nsr_h1_mlp_forward(precision == NSR_BF16, packed_dev, x, P, sigma_only, out, tail, stream);
  return nsr_fp32_mlp_forward(packed_dev, x, P, sigma_only, out, tail, stream);
}

extern "C" int nsr_render_rays(const void* packed_dev, int precision, const float* rays, int ray_stride, const float* z,
                               int64_t R, int n_samples, float* out, void* stream) {
  if (!packed_dev || R < 0 || n_samples <= 0 || !nsr_ray_stride_ok(ray_stride)) return NSR_ERR_INVALID_ARG;
  if (!precision_built(precision)) return NSR_ERR_UNSUPPORTED;
  if (R == 0) return NSR_OK;
  if (!rays || !z || !out) return NSR_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(out) & 15) != 0 || (ray_stride == 8 && (reinterpret_cast<uintptr_t>(rays) & 15) != 0))
    return NSR_ERR_INVALID_ARG;
  unsigned* tail = nsr_blob_tail(packed_dev, precision);
  if (precision == NSR_F16X3) return nsr_f16x3_render_rays(packed_dev, rays, ray_stride, z, R, n_samples, out, tail, stream);
  if (precision_h1(precision))
    return nsr_h1_render_rays(precision == NSR_BF16, packed_dev, rays, ray_stride, z, R, n_samples, out, tail, stream);
  return nsr_fp32_render_rays(packed_dev, rays, ray_stride, z, R, n_samples, out, tail, stream);
}

/* D2 + V1 in one launch, see include/nsr.h: the one body of both entry points below.  ert_tau / cut: early ray termination
 * of the split-fp16 kernel (0 / null: off), already checked by the caller */
static int render_rays_composited(const void* packed_dev, int precision, const float* rays, int ray_stride, const float* z,
                                  int64_t R, int n_samples, int white_bkgd, float* raw, float* comp_rgb, float* depth,
                                  float* opacity, float* weights, float ert_tau, unsigned* cut, void* stream) {
  if (!packed_dev || R < 0 || n_samples <= 0 || !nsr_ray_stride_ok(ray_stride) || (white_bkgd & ~(NSR_WHITE_BKGD | NSR_SIGMA_SOFTPLUS)) != 0)
    return NSR_ERR_INVALID_ARG;
  if (!precision_built(precision)) return NSR_ERR_UNSUPPORTED;
  if (!nsr_fused_samples(precision, n_samples)) return NSR_ERR_UNSUPPORTED;
  if (R == 0) return NSR_OK;
  if (!rays || !z) return NSR_ERR_INVALID_ARG;
  if ((raw && (reinterpret_cast<uintptr_t>(raw) & 15) != 0) || (ray_stride == 8 && (reinterpret_cast<uintptr_t>(rays) & 15) != 0))
    return NSR_ERR_INVALID_ARG;
  NsrCompOut co{comp_rgb, depth, opacity, weights, white_bkgd};
  co.ert_tau = ert_tau;
  co.cut = cut;
  unsigned* tail = nsr_blob_tail(packed_dev, precision);
  if (precision == NSR_F16X3) return nsr_f16x3_render_composite(packed_dev, rays, ray_stride, z, R, n_samples, raw, &co, tail, stream);
  return nsr_fp32_render_composite(packed_dev, rays, ray_stride, z, R, n_samples, raw, &co, tail, stream);
}

extern "C" int nsr_render_rays_composited(const void* packed_dev, int precision, const float* rays, int ray_stride, const float* z,
                                          int64_t R, int n_samples, int white_bkgd, float* raw, float* comp_rgb, float* depth,
                                          float* opacity, float* weights, void* stream) {
  return render_rays_composited(packed_dev, precision, rays, ray_stride, z, R, n_samples, white_bkgd, raw, comp_rgb, depth, opacity,
                                weights, 0.0f, nullptr, stream);
}

/* the same launch with early ray termination (split-fp16 kernel only), see include/nsr.h */
extern "C" int nsr_render_rays_composited_ert(const void* packed_dev, int precision, const float* rays, int ray_stride, const float* z,
                                              int64_t R, int n_samples, int render_flags, float early_stop, float* comp_rgb,
                                              float* depth, float* opacity, float* weights, unsigned* windows_cut, void* stream) {
  const int rc = nsr_ert_check(early_stop, precision, n_samples, render_flags);
  if (rc != NSR_OK) return rc;
  const bool on = early_stop > 0.0f;
  return render_rays_composited(packed_dev, precision, rays, ray_stride, z, R, n_samples, render_flags, nullptr, comp_rgb, depth, opacity,
                                weights, on ? (float)(-log((double)early_stop)) : 0.0f,      // -ln eps in double, rounded once
                                on ? windows_cut : nullptr, stream);
}

/* the density-only pass of the same launch (split-fp16 kernel only), see include/nsr.h */
extern "C" int nsr_render_rays_density(const void* packed_dev, int precision, const float* rays, int ray_stride, const float* z,
                                       int64_t R, int n_samples, int render_flags, float* depth, float* opacity, float* weights,
                                       void* stream) {
  if (!packed_dev || R < 0 || n_samples <= 0 || !nsr_ray_stride_ok(ray_stride) || (render_flags & ~(NSR_WHITE_BKGD | NSR_SIGMA_SOFTPLUS)) != 0)
    return NSR_ERR_INVALID_ARG;
  if (!precision_built(precision)) return NSR_ERR_UNSUPPORTED;
  if (precision != NSR_F16X3 || !nsr_fused_samples(precision, n_samples)) return NSR_ERR_UNSUPPORTED;
  if (R == 0) return NSR_OK;
  if (!rays || !z) return NSR_ERR_INVALID_ARG;
  if (ray_stride == 8 && (reinterpret_cast<uintptr_t>(rays) & 15) != 0) return NSR_ERR_INVALID_ARG;
  NsrCompOut co{nullptr, depth, opacity, weights, render_flags};
  return nsr_f16x3_render_density(packed_dev, rays, ray_stride, z, R, n_samples, &co, nsr_blob_tail(packed_dev, precision), stream);
}

// ---------------------------------------------------------------------------
// D3: forward_rays
// ---------------------------------------------------------------------------
static inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// workspace carve: z_coarse (R,Nc) | w_coarse (R,Nc) | z_fine (R,Nf) | [unfused route only: raw_coarse (R,Nc,4) | raw_fine (R,Nf,4)]
extern "C" size_t nsr_forward_rays_workspace_bytes_for(int precision, int64_t R, int n_coarse, int n_importance) {
  if (R < 0 || n_coarse <= 0 || n_importance < 0) return 0;
  const size_t r = (size_t)R, nc = (size_t)n_coarse, nf = (size_t)(n_coarse + n_importance);
  size_t total = align256(r * nc * 4) + align256(r * nc * 4);
  if (!nsr_fused_samples(precision, n_coarse)) total += align256(r * nc * 16);
  if (n_importance > 0) {
    total += align256(r * nf * 4);
    if (!nsr_fused_samples(precision, n_coarse + n_importance)) total += align256(r * nf * 16);
  }
  return total;
}
// precision-agnostic upper bound (the unfused route of any precision)
extern "C" size_t nsr_forward_rays_workspace_bytes(int64_t R, int n_coarse, int n_importance) {
  return nsr_forward_rays_workspace_bytes_for(-1, R, n_coarse, n_importance);
}

extern "C" int nsr_event_create(void** event_out) {
  if (!event_out) return NSR_ERR_INVALID_ARG;
  hipEvent_t ev;
  if (hipEventCreate(&ev) != hipSuccess) return NSR_ERR_LAUNCH;
  *event_out = ev;
  return NSR_OK;
}
extern "C" int nsr_event_destroy(void* event) {
  if (!event) return NSR_ERR_INVALID_ARG;
  return hipEventDestroy(static_cast<hipEvent_t>(event)) == hipSuccess ? NSR_OK : NSR_ERR_LAUNCH;
}
extern "C" int nsr_event_elapsed_ms(void* start, void* stop, float* ms_out) {
  if (!start || !stop || !ms_out) return NSR_ERR_INVALID_ARG;
  if (hipEventSynchronize(static_cast<hipEvent_t>(stop)) != hipSuccess) return NSR_ERR_LAUNCH;
  return hipEventElapsedTime(ms_out, static_cast<hipEvent_t>(start), static_cast<hipEvent_t>(stop)) == hipSuccess
             ? NSR_OK : NSR_ERR_LAUNCH;
}

extern "C" int nsr_forward_rays(const void* packed_coarse, const void* packed_fine, int precision, const float* rays,
                                int ray_stride, int64_t R, int n_coarse, int n_importance, int white_bkgd, int lindisp,
                                float* const* outs, void* workspace, size_t workspace_bytes, void* stream) {
  return nsr_forward_rays_profiled(packed_coarse, packed_fine, precision, rays, ray_stride, R, n_coarse, n_importance,
                                   white_bkgd, lindisp, outs, workspace, workspace_bytes, stream, nullptr);
}

extern "C" int nsr_forward_rays_profiled(const void* packed_coarse, const void* packed_fine, int precision,
                                         const float* rays, int ray_stride, int64_t R, int n_coarse, int n_importance,
                                         int white_bkgd, int lindisp, float* const* outs, void* workspace,
                                         size_t workspace_bytes, void* stream, void* const* events) {
  return nsr_forward_rays_ert(packed_coarse, packed_fine, precision, rays, ray_stride, R, n_coarse, n_importance, white_bkgd, lindisp,
                              outs, workspace, workspace_bytes, stream, events, 0.0f, nullptr);
}

static int forward_rays(bool density_coarse, const void* packed_coarse, const void* packed_fine, int precision, const float* rays,
                        int ray_stride, int64_t R, int n_coarse, int n_importance, int white_bkgd, int lindisp,
                        float* const* outs, void* workspace, size_t workspace_bytes, void* stream,
                        void* const* events, float early_stop, unsigned* windows_cut);

// early_stop > 0: the LAST network pass (the fine one, or the coarse one when n_importance == 0) is launched with early ray
// termination; the coarse pass that feeds the resampler never is (include/nsr.h)
extern "C" int nsr_forward_rays_ert(const void* packed_coarse, const void* packed_fine, int precision, const float* rays,
                                    int ray_stride, int64_t R, int n_coarse, int n_importance, int white_bkgd, int lindisp,
                                    float* const* outs, void* workspace, size_t workspace_bytes, void* stream,
                                    void* const* events, float early_stop, unsigned* windows_cut) {
  return forward_rays(false, packed_coarse, packed_fine, precision, rays, ray_stride, R, n_coarse, n_importance, white_bkgd, lindisp,
                      outs, workspace, workspace_bytes, stream, events, early_stop, windows_cut);
}

// test-time mode (include/nsr.h): the coarse pass feeds the resampler only and runs the density-only launch; its colour does
// not exist, so outs[0] must be null and a fine pass is required.  The fine pass is nsr_forward_rays_ert's.
extern "C" int nsr_forward_rays_density_coarse(const void* packed_coarse, const void* packed_fine, int precision, const float* rays,
                                               int ray_stride, int64_t R, int n_coarse, int n_importance, int white_bkgd,
                                               int lindisp, float* const* outs, void* workspace, size_t workspace_bytes,
                                               void* stream, void* const* events, float early_stop, unsigned* windows_cut) {
  if (!outs || outs[0] || n_importance <= 0) return NSR_ERR_INVALID_ARG;
  if (precision != NSR_F16X3 || !nsr_fused_samples(precision, n_coarse)) return NSR_ERR_UNSUPPORTED;
  return forward_rays(true, packed_coarse, packed_fine, precision, rays, ray_stride, R, n_coarse, n_importance, white_bkgd, lindisp,
                      outs, workspace, workspace_bytes, stream, events, early_stop, windows_cut);
}

// the one body of the entry points above.  density_coarse: checked by the caller (split fp16, a fused coarse sample count, a
// fine pass, no coarse colour)
static int forward_rays(bool density_coarse, const void* packed_coarse, const void* packed_fine, int precision, const float* rays,
                        int ray_stride, int64_t R, int n_coarse, int n_importance, int white_bkgd, int lindisp,
                        float* const* outs, void* workspace, size_t workspace_bytes, void* stream,
                        void* const* events, float early_stop, unsigned* windows_cut) {
  {
    const int erc = nsr_ert_check(early_stop, precision, n_importance > 0 ? n_coarse + n_importance : n_coarse, white_bkgd);
    if (erc != NSR_OK) return erc;
  }
  // one pass: network + compositing in one launch, cut short if it is the last pass and the option is on
  auto composited = [&](bool last, const void* packed, const float* z, int n, float* c, float* d, float* o, float* w) {
    return (last && early_stop > 0.0f)
               ? nsr_render_rays_composited_ert(packed, precision, rays, ray_stride, z, R, n, white_bkgd, early_stop, c, d, o, w,
                                                windows_cut, stream)
               : nsr_render_rays_composited(packed, precision, rays, ray_stride, z, R, n, white_bkgd, nullptr, c, d, o, w, stream);
  };
  hipStream_t st = nsr_stream(stream);
  auto mark = [&](int i) {
    if (events && events[i]) (void)hipEventRecord(static_cast<hipEvent_t>(events[i]), st);
  };
  if (!packed_coarse || !outs || R < 0 || n_coarse <= 0 || n_importance < 0 || (white_bkgd & ~(NSR_WHITE_BKGD | NSR_SIGMA_SOFTPLUS)) != 0)
    return NSR_ERR_INVALID_ARG;
  if (n_importance > 0 && !packed_fine) return NSR_ERR_INVALID_ARG;
  if (workspace_bytes < nsr_forward_rays_workspace_bytes_for(precision, R, n_coarse, n_importance)) return NSR_ERR_WORKSPACE;
  if (R == 0) return NSR_OK;
  if (!rays || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 255) != 0) return NSR_ERR_INVALID_ARG;
  const size_t r = (size_t)R, nc = (size_t)n_coarse, nf = (size_t)(n_coarse + n_importance);
  char* ws = static_cast<char*>(workspace);
  float* z_c = reinterpret_cast<float*>(ws);   ws += align256(r * nc * 4);
  float* w_c_ws = reinterpret_cast<float*>(ws); ws += align256(r * nc * 4);
  float* raw_c = nullptr;
  float* z_f = nullptr;
  float* raw_f = nullptr;
  if (!nsr_fused_samples(precision, n_coarse)) { raw_c = reinterpret_cast<float*>(ws); ws += align256(r * nc * 16); }
  if (n_importance > 0) {
    z_f = reinterpret_cast<float*>(ws);   ws += align256(r * nf * 4);
    if (!nsr_fused_samples(precision, n_coarse + n_importance)) { raw_f = reinterpret_cast<float*>(ws); ws += align256(r * nf * 16); }
  }
  int rc;
  // S1: coarse depths
  rc = nsr_sample_along_rays(rays, ray_stride, R, n_coarse, lindisp, nullptr, z_c, nullptr, stream);
  if (rc != NSR_OK) return rc;
  // D2+M1+V1: coarse network at every sample, composited by the same launch when the tile shape allows it (64 or 128
  // samples per ray, contract-grade precisions): the (R, N, 4) network output then never goes to HBM.  The coarse weights
  // are needed by the resampler even if the caller does not want them.
  float* w_c = outs[3] ? outs[3] : w_c_ws;
  mark(0);
  rc = density_coarse ? nsr_render_rays_density(packed_coarse, precision, rays, ray_stride, z_c, R, n_coarse, white_bkgd, outs[1], outs[2],
                                                w_c, stream)
                      : composited(n_importance == 0, packed_coarse, z_c, n_coarse, outs[0], outs[1], outs[2], w_c);
  if (rc == NSR_ERR_UNSUPPORTED) {   // other sample counts / the single-operand fast paths: network, then compositor
    rc = nsr_render_rays(packed_coarse, precision, rays, ray_stride, z_c, R, n_coarse, raw_c, stream);
    mark(1);
    if (rc != NSR_OK) return rc;
    rc = nsr_composite(raw_c, 4, raw_c + 3, 4, z_c, R, n_coarse, white_bkgd, outs[0], outs[1], outs[2], w_c, stream);
  } else {
    mark(1);
  }
  if (rc != NSR_OK) return rc;
  if (n_importance == 0) return NSR_OK;
  // S2: importance resampling + merge
  rc = nsr_resample_along_rays(rays, ray_stride, z_c, w_c, R, n_coarse, n_importance, nullptr, z_f, nullptr, stream);
  if (rc != NSR_OK) return rc;
  // fine network + compositing
  mark(2);
  rc = composited(true, packed_fine, z_f, n_coarse + n_importance, outs[4], outs[5], outs[6], outs[7]);
  if (rc != NSR_ERR_UNSUPPORTED) {
    mark(3);
    return rc;
  }
  rc = nsr_render_rays(packed_fine, precision, rays, ray_stride, z_f, R, n_coarse + n_importance, raw_f, stream);
  mark(3);
  if (rc != NSR_OK) return rc;
  rc = nsr_composite(raw_f, 4, raw_f + 3, 4, z_f, R, n_coarse + n_importance, white_bkgd, outs[4], outs[5], outs[6],
                     outs[7], stream);
  return rc;
}
