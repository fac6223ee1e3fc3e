// The embedding's option word (include/nsr.h: NSR_EMBED_NO_XYZ, NSR_EMBED_LINEAR_FREQS) as the encoders share it: the
// column count of an encoding, the checks of the word, and the band table a kernel receives by value (nsr_posenc_freqs is
// the only place it is computed).
#pragma once
#include "nsr_common.h"

constexpr unsigned kEmbedBits = NSR_EMBED_NO_XYZ | NSR_EMBED_LINEAR_FREQS;
constexpr int kEmbedMaxDeg = 16;

struct NsrBands {
  float f[kEmbedMaxDeg];
};

// columns of the encoding of a 3-vector: [x |] sin, cos of every band
static inline int nsr_embed_cols(int deg, unsigned embed) { return ((embed & NSR_EMBED_NO_XYZ) ? 0 : 3) + 6 * deg; }
// first column of the bands = number of identity columns
__host__ __device__ static inline int nsr_embed_first(unsigned embed) { return (embed & NSR_EMBED_NO_XYZ) ? 0 : 3; }

// the word of a network with these degrees: an unknown bit, or --no_xyz on an encoding of degree 0 that the network reads
// (the layer would have no input columns; the reference cannot build it either)
static inline int nsr_embed_check_net(unsigned embed, int deg_pos, int deg_dir, int no_dir) {
  if ((embed & ~kEmbedBits) != 0u) return NSR_ERR_INVALID_ARG;
  if ((embed & NSR_EMBED_NO_XYZ) && (deg_pos == 0 || (deg_dir == 0 && !no_dir))) return NSR_ERR_INVALID_ARG;
  return NSR_OK;
}

static inline int nsr_bands(int deg, unsigned embed, NsrBands& b) {
  for (int i = 0; i < kEmbedMaxDeg; ++i) b.f[i] = 0.0f;
  return nsr_posenc_freqs(deg, embed, b.f);
}

// argument of band k of the encoders: under the log-scale bands the exact ldexpf of nsr_posenc (the code path of embed = 0),
// under the linear ones ONE fp32 multiply `freq * x` as in the reference (no contraction)
__device__ __forceinline__ float nsr_band_arg(float x, int k, const NsrBands& bands, unsigned embed) {
  return (embed & NSR_EMBED_LINEAR_FREQS) ? __fmul_rn(bands.f[k], x) : ldexpf(x, k);
}
