// Fused split-fp16 ("f16x3") forward of a NON-default network architecture (include/nsr_train.h: nsr_arch_fused_*): one
// launch takes the encoded rows x (P, in_xyz + in_dir) to (rgb, sigma); no activation leaves the CU between two layers.
//
// Arithmetic: that of nsr_linear_f16x3, layer by layer -- weights pre-split once as RNE_f16(64 w) / RNE_f16(64 w - hi), each
// layer's input split into fp16 (hi, lo), three v_mfma_f32_32x32x16_f16 per product (lo*hi, hi*lo, hi*hi), fp32
// accumulation from zero, epilogue fmaf(acc, 1/64, bias) -> activation in fp32 -- in another summation order.
//
// Layout: the network is evaluated transposed, Out^T (features x points) = W (features x K) * In^T (K x points).  A wave owns
// 32 points; the weights are the MFMA A operand, the activations the B operand.  The D fragment of a 32-feature output block
// -- lane (m = lane & 31, h = lane >> 5) holds, for point m, features (r & 3) + 8 (r >> 2) + 4 h in register r -- is, after
// the re-split, the B operand of the next layer's two k-steps over that block: registers 8 s .. 8 s + 7 are k-step s, whose
// element j is therefore feature
//     kmap(s, h, j) = 16 s + 8 (j >> 2) + 4 h + (j & 3)
// of the block.  The pack kernel lays every weight fragment out in that k order, and the encoded inputs are loaded from x in
// the same order, so ONE map serves every layer.  No transpose, no LDS trip for an activation.
//
// Weight stream: 1 KiB pieces (64 lanes x 16 B, the A fragment of one k-step and part).  One CHUNK = one 32-feature output
// block of one layer: for every 32-column input block, in the order [encoded position | hidden | encoded direction], the
// pieces (s = 0 hi, s = 0 lo, s = 1 hi, s = 1 lo), then one piece whose first 32 words are the block's fp32 biases.
// cat([pe, h]) of a skip layer and cat([final, dir_pe]) are K ranges of the chunk, never copies.  Chunk order: trunk layers
// 0 .. D-1, sigma, xyz_encoding_final, dir_encoding, rgb.  A workgroup is four waves = 128 points sharing the chunks through a
// two-slot LDS ring: while chunk j is consumed, every wave's LDS-DMA of its quarter of chunk j+1 is in flight; one
// (wait for the own DMA, barrier) per chunk publishes j+1 and frees the slot of j.
//
// Input modes (template parameter MODE, as encode_point<MODE> of nsr_mlp_encode.h): 0 reads the encoded rows x; 1
// (nsr_arch_fused_render_rays) takes rays (R, 8 | 11) and z (R, n_samples) -- point p is sample p % n_samples of ray
// p / n_samples, a tile may straddle rays -- forms o + z d and computes, in registers, exactly the encoded columns the lane
// would have loaded in mode 0, by the expression of the stand-alone encoder (nsr_posenc), so both modes feed the same bits to
// the same network code.  2 is mode 1 under a non-zero embedding option word (include/nsr.h: no identity columns, linear bands
// from the table in the arguments), by the expression nsr_posenc_e has for that word; the host selects it, so the launch of
// embed = 0 is the instantiation it always was.  Mode 0 sees the word only as the narrower widths in_xyz / in_dir.
#include "nsr_f16x3_core.h"
#include "nsr_embed.h"
#include "../../include/nsr_train.h"

namespace {

constexpr int kFusedMaxD = NSR_ARCH_FUSED_MAX_D, kFusedMaxW = NSR_ARCH_FUSED_MAX_W;
constexpr int kFusedMaxDegPos = NSR_ARCH_FUSED_MAX_DEG_POS, kFusedMaxDegDir = NSR_ARCH_FUSED_MAX_DEG_DIR;
constexpr int kFusedTile = 128;        // points per workgroup

struct FusedShape {
  int D, W, H, in_xyz, in_dir, no_dir;
  unsigned skips;
  int NB, HB, KXB;        // 32-feature blocks of W, of W / 2, of the encoded position
  bool skip(int l) const { return l > 0 && ((skips >> l) & 1u) != 0u; }
  int trunk_kb(int l) const { return l == 0 ? KXB : (skip(l) ? KXB + NB : NB); }
};
constexpr int chunk_pieces(int kb) { return 4 * kb + 1; }

int fused_shape(const nsr_arch* a, unsigned embed, FusedShape& S) {
  if (!a) return NSR_ERR_INVALID_ARG;
  if (a->D < 1 || a->W < 2 || (a->W & 1) || a->deg_pos < 0 || a->deg_dir < 0 || (a->no_dir != 0 && a->no_dir != 1))
    return NSR_ERR_INVALID_ARG;
  if ((a->skips & 1u) || (a->D < 32 && (a->skips >> a->D) != 0u)) return NSR_ERR_INVALID_ARG;
  if (a->D > kFusedMaxD || a->W > kFusedMaxW || a->deg_pos > kFusedMaxDegPos || a->deg_dir > kFusedMaxDegDir)
    return NSR_ERR_UNSUPPORTED;
  S.D = a->D; S.W = a->W; S.H = a->W / 2; S.skips = a->skips; S.no_dir = a->no_dir;
  const int rc = nsr_embed_check_net(embed, a->deg_pos, a->deg_dir, a->no_dir);
  if (rc != NSR_OK) return rc;
  S.in_xyz = nsr_embed_cols(a->deg_pos, embed); S.in_dir = nsr_embed_cols(a->deg_dir, embed);
  S.NB = (S.W + 31) / 32; S.HB = (S.H + 31) / 32; S.KXB = (S.in_xyz + 31) / 32;
  return NSR_OK;
}

int64_t fused_total_pieces(const FusedShape& S) {
  int64_t n = 0;
  for (int l = 0; l < S.D; ++l) n += (int64_t)S.NB * chunk_pieces(S.trunk_kb(l));
  n += chunk_pieces(S.NB);                                  // sigma
  n += (int64_t)S.NB * chunk_pieces(S.NB);                  // xyz_encoding_final
  n += (int64_t)S.HB * chunk_pieces(S.NB + (S.no_dir ? 0 : 1));   // dir_encoding
  n += chunk_pieces(S.HB);                                  // rgb
  return n;
}

// ---------------------------------------------------------------------------------------------------------------------
// pack: one launch per stage (= weight tensor), one thread per 32-bit word of the stage's chunks
// ---------------------------------------------------------------------------------------------------------------------
struct PackStage {
  const float* w;
  const float* b;
  int n_valid;       // rows of w
  int ldw;           // columns of w
  int nob;           // 32-row output blocks = chunks
  int nk[3];         // 32-column input blocks of the sources [encoded position | hidden | encoded direction]
  int col0[3];       // first column of w of each source
  int kvalid[3];     // columns of each source that exist (the rest of its last block is zero)
  int64_t piece0;    // first piece of the stage
};

__global__ void __launch_bounds__(256) arch_fused_pack_kernel(PackStage s, unsigned* __restrict__ out, float limit,
                                                              unsigned* __restrict__ status) {
  const int cp = chunk_pieces(s.nk[0] + s.nk[1] + s.nk[2]);
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)s.nob * cp * 256) return;
  const int piece = (int)(idx >> 8), word = (int)(idx & 255);
  const int ob = piece / cp, local = piece % cp;
  unsigned v = 0u;
  bool bad = false;
  if (local == cp - 1) {                                   // the chunk's biases: fp32, unscaled (the epilogue's fmaf operand)
    if (word < 32) {
      const int n = 32 * ob + word;
      const float f = n < s.n_valid ? s.b[n] : 0.0f;
      bad = !nsr_finite(f);
      v = __float_as_uint(f);
    }
  } else {
    int kb = local >> 2, src = 0;
    const int st = (local >> 1) & 1, part = local & 1;
    if (kb >= s.nk[0]) { kb -= s.nk[0]; src = 1; }
    if (src == 1 && kb >= s.nk[1]) { kb -= s.nk[1]; src = 2; }
    const int lane = word >> 2, jj = word & 3;
    const int n = 32 * ob + (lane & 31), h = lane >> 5;
    float f[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int j = 2 * jj + e;
      const int kk = 32 * kb + 16 * st + 8 * (j >> 2) + 4 * h + (j & 3);
      f[e] = (n < s.n_valid && kk < s.kvalid[src]) ? s.w[(int64_t)n * s.ldw + s.col0[src] + kk] : 0.0f;
      bad |= !(fabsf(f[e]) <= limit);                      // also true for NaN
    }
    v = pack_hl(kWScale * f[0], kWScale * f[1], part);
  }
  out[s.piece0 * 256 + idx] = v;
  if (bad && status) atomicOr(status, NSR_FLAG_WEIGHT_RANGE);
}

// ---------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------
struct FusedArgs {
  const char* stream;
  const float* x;
  int64_t ldx, P;
  float* out;
  int64_t ldo;
  unsigned* status;
  int D;
  unsigned skips;
  int in_xyz, in_dir, kxb, no_dir, sigma_only, color_none;
  const float* rays;      // MODE 1: (R, ray_stride) ray records and (R, n_samples) depths instead of x; P = R * n_samples
  const float* z;
  int ray_stride, n_samples;
  unsigned embed;         // MODE 2: the embedding's option word and the bands of the two encodings
  NsrBands bands_pos, bands_dir;
};

template <int N>
struct Act {            // a layer's input as MFMA B fragments: block, k-step -> 8 fp16 (hi) + 8 fp16 (lo)
  u32x4 hi[N][2], lo[N][2];
};

struct Ring {
  const char* cur;      // first byte of the chunk being consumed (wave-uniform)
  int cur_pieces;
  unsigned slot_cur, slot_next;
  int wave;
  unsigned lane_off;
};
// this wave's quarter of the chunk behind the current one -> the other slot
__device__ __forceinline__ void ring_fetch_next(const Ring& r, int next_pieces) {
  const char* src = r.cur + (size_t)r.cur_pieces * 1024u;
  for (int p = r.wave; p < next_pieces; p += 4) glds16_asm<0>(src + (size_t)p * 1024u, r.lane_off, r.slot_next + (unsigned)p * 1024u);
}
// publish the next chunk: every wave's pieces have landed and every wave has left the current one
__device__ __forceinline__ void ring_advance(Ring& r, int next_pieces) {
  dma_drain();
  __syncthreads();
  r.cur += (size_t)r.cur_pieces * 1024u;
  r.cur_pieces = next_pieces;
  const unsigned t = r.slot_cur;
  r.slot_cur = r.slot_next;
  r.slot_next = t;
}

// NSTEP consecutive k-steps of one output block.  a_addr: LDS byte address (+ lane * 16) of the first k-step's hi piece; k-step s
// reads the pieces 2 s (hi) and 2 s + 1 (lo) behind it.  The A fragments are fetched kAhead k-steps ahead of the MFMAs that use
// them (order pinned by sched_barrier: left to itself hipcc serialises every read behind a full lgkmcnt(0) wait here).
// b(s, hi, lo): the activation operands of k-step s.
constexpr int kAhead = 2;
template <int NSTEP, class BOf>
__device__ __forceinline__ void seg_mma(f32x16& acc, unsigned a_addr, BOf&& b) {
  const u32x4* a = lds_vec(a_addr);
  u32x4 ah[NSTEP], al[NSTEP];
#pragma unroll
  for (int s = 0; s < kAhead && s < NSTEP; ++s) {
    ah[s] = a[(2 * s) * 64];
    al[s] = a[(2 * s + 1) * 64];
  }
#pragma unroll
  for (int s = 0; s < NSTEP; ++s) {
    if (s + kAhead < NSTEP) {
      ah[s + kAhead] = a[(2 * (s + kAhead)) * 64];
      al[s + kAhead] = a[(2 * (s + kAhead) + 1) * 64];
    }
    u32x4 bh, bl;
    b(s, bh, bl);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(as_h8(al[s]), as_h8(bh), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(as_h8(ah[s]), as_h8(bl), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(as_h8(ah[s]), as_h8(bh), acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// the products of one chunk: n_pe (0..2) blocks of the encoded position, n_h (0 or NH) hidden blocks, the encoded direction
template <int NH>
__device__ __forceinline__ void chunk_mma(f32x16& acc, unsigned addr, int n_pe, int n_h, bool with_dir, const Act<2>& pe,
                                          const Act<NH>& hin, const Act<1>& de) {
  auto b_pe = [&](int s, u32x4& bh, u32x4& bl) { bh = pe.hi[s >> 1][s & 1]; bl = pe.lo[s >> 1][s & 1]; };
  if (n_pe == 2) seg_mma<4>(acc, addr, b_pe);
  else if (n_pe == 1) seg_mma<2>(acc, addr, b_pe);
  addr += (unsigned)n_pe * 4096u;
  if (n_h > 0) {
    seg_mma<2 * NH>(acc, addr, [&](int s, u32x4& bh, u32x4& bl) { bh = hin.hi[s >> 1][s & 1]; bl = hin.lo[s >> 1][s & 1]; });
    addr += (unsigned)NH * 4096u;
  }
  if (with_dir) seg_mma<2>(acc, addr, [&](int s, u32x4& bh, u32x4& bl) { bh = de.hi[0][s]; bl = de.lo[0][s]; });
}

// the layered epilogue: undo the weights' 2^6, add the bias, activate -- in fp32.  amax: largest magnitude that will be split
__device__ __forceinline__ void bias_act(f32x16& acc, unsigned bias_addr, int h, bool relu, float& amax) {
  const f32x4* b = reinterpret_cast<const f32x4*>(lds_vec(bias_addr + 16u * (unsigned)h));
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 b4 = b[2 * q];                     // biases of rows 8 q + 4 h .. + 3
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = fmaf(acc[4 * q + i], kWInvScale, b4[i]);
      if (relu) v = nsr_relu_nan(v);
      acc[4 * q + i] = v;
      amax = fmaxf(amax, fabsf(v));
    }
  }
}

// split2 of nsr_f16x3_core.h on two-element vectors: the same round-to-nearest conversions, which gfx950 has in packed form
// (v_cvt_pk_f16_f32), so a pair costs six instructions instead of eleven -- the re-split is the kernel's largest VALU item
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split2_pk(float x0, float x1, unsigned& hi, unsigned& lo) {
  const f32x2 x = {x0, x1};
  const h2 h = __builtin_convertvector(x, h2);
  const h2 l = __builtin_convertvector(x - __builtin_convertvector(h, f32x2), h2);
  hi = __builtin_bit_cast(unsigned, h);
  lo = __builtin_bit_cast(unsigned, l);
}

__device__ __forceinline__ void split_block(const f32x16& v, u32x4 (&hi)[2], u32x4 (&lo)[2]) {
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      unsigned a, b;
      split2_pk(v[8 * s + 2 * jj], v[8 * s + 2 * jj + 1], a, b);
      hi[s][jj] = a;
      lo[s][jj] = b;
    }
}

// 32 columns [col0 + 32 kb, ...) of this lane's row in the k order of the fragments; columns >= n_cols are zero
__device__ __forceinline__ void load_block(const float* __restrict__ row, int kb, int n_cols, int h, u32x4 (&hi)[2], u32x4 (&lo)[2],
                                           bool& ok) {
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int c = 32 * kb + 16 * s + 8 * (jj >> 1) + 4 * h + 2 * (jj & 1);      // kmap(s, h, 2 jj); 2 jj + 1 is the next column
      const float f0 = c < n_cols ? row[c] : 0.0f;
      const float f1 = c + 1 < n_cols ? row[c + 1] : 0.0f;
      ok = ok && fabsf(f0) <= 65504.0f && fabsf(f1) <= 65504.0f;                    // false for NaN
      unsigned a, b;
      split2_pk(f0, f1, a, b);
      hi[s][jj] = a;
      lo[s][jj] = b;
    }
}

// MODE 1: column c of [v, sin(2^0 v), cos(2^0 v), sin(2^1 v), ...] for the 3-vector v.  This is posenc_kernel's expression
// (nsr_rays.hip: sinf / cosf of the exact ldexpf argument, NOT nsr_sincos, whose values differ from it in the last bits): the
// row route feeds the network what that kernel wrote, and the two routes promise the same bits.  Both functions are
// evaluated and one is selected: the halves of a wave hold columns 4 apart, which mix sines and cosines, and the two share
// their argument reduction.
__device__ __forceinline__ float encoded_column(float v0, float v1, float v2, int c) {
  const int u = c < 3 ? c : c - 3;
  const int f = u / 6, r = u - 6 * f, comp = r < 3 ? r : r - 3;
  const float x = comp == 0 ? v0 : (comp == 1 ? v1 : v2);
  if (c < 3) return x;
  const float arg = ldexpf(x, f);                      // 2^f * x, exact
  const float sn = sinf(arg), cs = cosf(arg);
  return r < 3 ? sn : cs;
}

// MODE 2: the same under the option word `embed` -- nsr_posenc_e's expression.  c0 (the column of lane half 0) is wave-uniform and
// so are the two bands a pair of halves can need: they are read with uniform indices and selected by h.
__device__ __forceinline__ float encoded_column_e(float v0, float v1, float v2, int c0, int h, unsigned embed, const NsrBands& bands) {
  const int first = nsr_embed_first(embed), c = c0 + 4 * h;
  const int u = c < first ? c : c - first;
  const int f = u / 6, r = u - 6 * f, comp = r < 3 ? r : r - 3;
  const float x = comp == 0 ? v0 : (comp == 1 ? v1 : v2);
  if (c < first) return x;
  const int u0 = c0 < first ? 0 : c0 - first;
  const int f0 = min(u0 / 6, kEmbedMaxDeg - 1), f1 = min((u0 + 4) / 6, kEmbedMaxDeg - 1);
  const float band = h ? bands.f[f1] : bands.f[f0];
  const float arg = (embed & NSR_EMBED_LINEAR_FREQS) ? __fmul_rn(band, x) : ldexpf(x, f);
  const float sn = sinf(arg), cs = cosf(arg);
  return r < 3 ? sn : cs;
}

// load_block without the row: the same 32 columns of the encoding of v, in the same registers, under the same range test
template <int MODE>
__device__ __forceinline__ void encode_block(float v0, float v1, float v2, int kb, int n_cols, int h, u32x4 (&hi)[2], u32x4 (&lo)[2],
                                             bool& ok, unsigned embed, const NsrBands& bands) {
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int c0 = 32 * kb + 16 * s + 8 * (jj >> 1) + 2 * (jj & 1);                // the column of lane half 0: wave-uniform
      const int c = c0 + 4 * h;
      float f0 = 0.0f, f1 = 0.0f;
      if (c0 < n_cols) {                               // a pair past the encoding in both halves costs nothing
        if (MODE == 2) {
          f0 = c < n_cols ? encoded_column_e(v0, v1, v2, c0, h, embed, bands) : 0.0f;
          f1 = c + 1 < n_cols ? encoded_column_e(v0, v1, v2, c0 + 1, h, embed, bands) : 0.0f;
        } else {
          f0 = c < n_cols ? encoded_column(v0, v1, v2, c) : 0.0f;
          f1 = c + 1 < n_cols ? encoded_column(v0, v1, v2, c + 1) : 0.0f;
        }
      }
      ok = ok && fabsf(f0) <= 65504.0f && fabsf(f1) <= 65504.0f;                    // false for NaN
      unsigned a, b;
      split2_pk(f0, f1, a, b);
      hi[s][jj] = a;
      lo[s][jj] = b;
    }
}

template <int NB, int MODE>
__global__ void __launch_bounds__(256) arch_fused_kernel(FusedArgs a) {
  constexpr int HB = (NB + 1) / 2;
  constexpr int kSlot = chunk_pieces(NB + 2) * 1024;
  __shared__ __attribute__((aligned(1024))) unsigned char ring_mem[2 * kSlot];

  const int tid = threadIdx.x, lane = tid & 63, m = lane & 31, h = lane >> 5;
  Ring ring;
  ring.wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  ring.lane_off = 16u * (unsigned)lane;
  ring.slot_next = lds_addr(ring_mem);               // chunk 0 goes here ...
  ring.slot_cur = lds_addr(ring_mem) + kSlot;
  ring.cur = a.stream;
  ring.cur_pieces = 0;
  ring_fetch_next(ring, chunk_pieces(a.kxb));        // ... while the inputs are loaded

  const int64_t p = (int64_t)blockIdx.x * kFusedTile + 32 * ring.wave + m;
  const bool valid = p < a.P;
  unsigned flags = 0u;
  Act<2> pe;
  Act<1> de;
  if (MODE == 0) {
    const float* xr = a.x + (valid ? p : a.P - 1) * a.ldx;      // a tail lane re-reads the last row; its results are dropped
    bool ok = true;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) load_block(xr, kb, a.in_xyz, h, pe.hi[kb], pe.lo[kb], ok);
    const bool with_dir = !a.sigma_only && !a.no_dir;
    load_block(xr + a.in_xyz, 0, with_dir ? a.in_dir : 0, h, de.hi[0], de.lo[0], ok);
    if (!ok) flags |= NSR_FLAG_INPUT_RANGE;
  } else {
    const int64_t pc = valid ? p : a.P - 1;                     // a tail lane re-reads the last point (its ray and its z)
    const NsrRay rq = nsr_load_ray(a.rays, pc / a.n_samples, a.ray_stride);
    const float zk = a.z[pc];
    // cast_rays with a separate multiply and add, as sample_kernel / resample_kernel write the points of the row route
    const float v0 = __fadd_rn(rq.o[0], __fmul_rn(zk, rq.d[0])), v1 = __fadd_rn(rq.o[1], __fmul_rn(zk, rq.d[1])),
                v2 = __fadd_rn(rq.o[2], __fmul_rn(zk, rq.d[2]));
    bool ok = true;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) encode_block<MODE>(v0, v1, v2, kb, a.in_xyz, h, pe.hi[kb], pe.lo[kb], ok, a.embed, a.bands_pos);
    const bool with_dir = !a.sigma_only && !a.no_dir;
    encode_block<MODE>(rq.v[0], rq.v[1], rq.v[2], 0, with_dir ? a.in_dir : 0, h, de.hi[0], de.lo[0], ok, a.embed,
                       a.bands_dir);   // the direction that is ENCODED
    if (!ok) flags |= NSR_FLAG_INPUT_RANGE;
  }
  ring_advance(ring, chunk_pieces(a.kxb));

  Act<NB> hin;
#pragma unroll
  for (int kb = 0; kb < NB; ++kb)
#pragma unroll
    for (int s = 0; s < 2; ++s) hin.hi[kb][s] = hin.lo[kb][s] = u32x4{0u, 0u, 0u, 0u};
  f32x16 acc[NB];
  float amax = 0.0f, sigma = 0.0f, unused = 0.0f;
  const int dir_pieces = chunk_pieces(NB + (a.no_dir ? 0 : 1));

  // stages 0 .. D-1: the trunk; stage D: sigma (one chunk, read from the last trunk layer), then xyz_encoding_final
  for (int l = 0; l <= a.D; ++l) {
    const bool last = l == a.D;
    const int n_pe = (l == 0 || ((a.skips >> l) & 1u)) && !last ? a.kxb : 0;
    const int n_h = l == 0 ? 0 : NB;
    const int mine = ring.cur_pieces;
    int after;                                       // pieces of the first chunk of the next stage
    if (last) after = dir_pieces;
    else if (l + 1 == a.D) after = chunk_pieces(NB);
    else after = chunk_pieces(((a.skips >> (l + 1)) & 1u) ? a.kxb + NB : NB);
    if (last) {
      ring_fetch_next(ring, a.sigma_only ? 0 : mine);
      f32x16 sg = {};
      chunk_mma<NB>(sg, ring.slot_cur + ring.lane_off, 0, NB, false, pe, hin, de);
      bias_act(sg, ring.slot_cur + (unsigned)(mine - 1) * 1024u, h, false, unused);
      sigma = sg[0];                                 // row 0: lanes of half 0
      if (a.sigma_only) break;
      ring_advance(ring, mine);
    }
#pragma unroll
    for (int ob = 0; ob < NB; ++ob) {
      const int next = ob + 1 < NB ? mine : after;
      ring_fetch_next(ring, next);
      acc[ob] = f32x16{};
      chunk_mma<NB>(acc[ob], ring.slot_cur + ring.lane_off, n_pe, n_h, false, pe, hin, de);
      bias_act(acc[ob], ring.slot_cur + (unsigned)(mine - 1) * 1024u, h, !last, amax);
      ring_advance(ring, next);
    }
#pragma unroll
    for (int ob = 0; ob < NB; ++ob) split_block(acc[ob], hin.hi[ob], hin.lo[ob]);
  }

  if (a.sigma_only) {
    if (!nsr_finite(sigma)) flags |= NSR_FLAG_OUTPUT_NONFINITE;
    if (amax >= 65520.0f) flags |= NSR_FLAG_ACTIVATION_RANGE;
    if (valid) {
      if (h == 0) a.out[p * a.ldo] = sigma;
      if (flags != 0u && a.status) atomicOr(a.status, flags);
    }
    return;
  }

  // dir_encoding: relu(W [final | dir pe] + b), W / 2 features
  Act<HB> cin;
  {
    f32x16 c[HB];
    const int mine = ring.cur_pieces;
#pragma unroll
    for (int ob = 0; ob < HB; ++ob) {
      const int next = ob + 1 < HB ? mine : chunk_pieces(HB);
      ring_fetch_next(ring, next);
      c[ob] = f32x16{};
      chunk_mma<NB>(c[ob], ring.slot_cur + ring.lane_off, 0, NB, !a.no_dir, pe, hin, de);
      bias_act(c[ob], ring.slot_cur + (unsigned)(mine - 1) * 1024u, h, true, amax);
      ring_advance(ring, next);
    }
#pragma unroll
    for (int ob = 0; ob < HB; ++ob) split_block(c[ob], cin.hi[ob], cin.lo[ob]);
  }
  // rgb: rows 0..2 of one block
  f32x16 o = {};
  chunk_mma<HB>(o, ring.slot_cur + ring.lane_off, 0, HB, false, pe, cin, de);
  bias_act(o, ring.slot_cur + (unsigned)(ring.cur_pieces - 1) * 1024u, h, false, unused);
  const unsigned opts = a.color_none ? kOptColorNone : 0u;
  const float r = nsr_colour_activation(o[0], opts), g = nsr_colour_activation(o[1], opts), b = nsr_colour_activation(o[2], opts);
  if (h == 0 && !(nsr_finite(r) && nsr_finite(g) && nsr_finite(b) && nsr_finite(sigma))) flags |= NSR_FLAG_OUTPUT_NONFINITE;
  if (amax >= 65520.0f) flags |= NSR_FLAG_ACTIVATION_RANGE;
  if (valid) {
    if (h == 0) {
      float* dst = a.out + p * a.ldo;
      dst[0] = r; dst[1] = g; dst[2] = b; dst[3] = sigma;
    }
    if (flags != 0u && a.status) atomicOr(a.status, flags);
  }
}

template <int MODE>
void launch_fused(int NB, const FusedArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)((a.P + kFusedTile - 1) / kFusedTile)), block(256);
  switch (NB) {
    case 1: hipLaunchKernelGGL((arch_fused_kernel<1, MODE>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((arch_fused_kernel<2, MODE>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((arch_fused_kernel<3, MODE>), grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL((arch_fused_kernel<4, MODE>), grid, block, 0, st, a); break;
    case 5: hipLaunchKernelGGL((arch_fused_kernel<5, MODE>), grid, block, 0, st, a); break;
    case 6: hipLaunchKernelGGL((arch_fused_kernel<6, MODE>), grid, block, 0, st, a); break;
    case 7: hipLaunchKernelGGL((arch_fused_kernel<7, MODE>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((arch_fused_kernel<8, MODE>), grid, block, 0, st, a); break;
  }
}

}  // namespace

extern "C" size_t nsr_arch_fused_packed_bytes(const nsr_arch* arch) { return nsr_arch_fused_packed_bytes_e(arch, 0u); }
extern "C" size_t nsr_arch_fused_packed_bytes_e(const nsr_arch* arch, unsigned embed) {
  FusedShape S;
  if (fused_shape(arch, embed, S) != NSR_OK) return 0;
  return (size_t)fused_total_pieces(S) * 1024u;
}

extern "C" int nsr_arch_fused_pack(const nsr_arch* arch, const float* const* w, void* packed, unsigned* status, void* stream) {
  return nsr_arch_fused_pack_e(arch, 0u, w, packed, status, stream);
}
extern "C" int nsr_arch_fused_pack_e(const nsr_arch* arch, unsigned embed, const float* const* w, void* packed, unsigned* status,
                                     void* stream) {
  FusedShape S;
  const int rc = fused_shape(arch, embed, S);
  if (rc != NSR_OK) return rc;
  if (!w || !packed || (reinterpret_cast<uintptr_t>(packed) & 15) != 0) return NSR_ERR_INVALID_ARG;
  const int nt = 2 * S.D + 8;
  for (int t = 0; t < nt; ++t)
    if (!w[t]) return NSR_ERR_INVALID_ARG;
  hipStream_t st = nsr_stream(stream);
  const float limit = 65519.996f / kWScale;        // 2^6 w must stay finite in fp16 (nsr_pack_weights under NSR_F16X3)
  int64_t piece0 = 0;
  auto stage = [&](int t, int n_valid, int nob, int nk_pe, int nk_h, int h_col0, int h_valid, int nk_d) -> int {
    PackStage s;
    s.w = w[t]; s.b = w[t + 1];
    s.n_valid = n_valid; s.nob = nob;
    s.nk[0] = nk_pe; s.col0[0] = 0; s.kvalid[0] = S.in_xyz;
    s.nk[1] = nk_h; s.col0[1] = h_col0; s.kvalid[1] = h_valid;
    s.nk[2] = nk_d; s.col0[2] = h_col0 + h_valid; s.kvalid[2] = S.in_dir;
    s.ldw = (nk_pe ? S.in_xyz : 0) + (nk_h ? h_valid : 0) + (nk_d ? S.in_dir : 0);
    s.piece0 = piece0;
    const int64_t words = (int64_t)nob * chunk_pieces(nk_pe + nk_h + nk_d) * 256;
    hipLaunchKernelGGL(arch_fused_pack_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, s,
                       static_cast<unsigned*>(packed), limit, status);
    NSR_CHECK_LAUNCH();
    piece0 += words / 256;
    return NSR_OK;
  };
  for (int l = 0; l < S.D; ++l) {
    const bool pe = l == 0 || S.skip(l);
    const int e = stage(2 * l, S.W, S.NB, pe ? S.KXB : 0, l == 0 ? 0 : S.NB, pe ? S.in_xyz : 0, S.W, 0);
    if (e != NSR_OK) return e;
  }
  const int t0 = 2 * S.D;      // final, dir_encoding, sigma, rgb (state_dict order); stream order: sigma, final, dir, rgb
  int e = stage(t0 + 4, 1, 1, 0, S.NB, 0, S.W, 0);
  if (e == NSR_OK) e = stage(t0, S.W, S.NB, 0, S.NB, 0, S.W, 0);
  if (e == NSR_OK) e = stage(t0 + 2, S.H, S.HB, 0, S.NB, 0, S.W, S.no_dir ? 0 : 1);
  if (e == NSR_OK) e = stage(t0 + 6, 3, 1, 0, S.HB, 0, S.H, 0);
  return e;
}

extern "C" int nsr_arch_fused_forward(const nsr_arch* arch, const void* packed, const float* x, int64_t ldx, int64_t P, int flags,
                                      float* out, int64_t ldo, unsigned* status, void* stream) {
  return nsr_arch_fused_forward_e(arch, 0u, packed, x, ldx, P, flags, out, ldo, status, stream);
}
extern "C" int nsr_arch_fused_forward_e(const nsr_arch* arch, unsigned embed, const void* packed, const float* x, int64_t ldx, int64_t P,
                                        int flags, float* out, int64_t ldo, unsigned* status, void* stream) {
  FusedShape S;
  const int rc = fused_shape(arch, embed, S);
  if (rc != NSR_OK) return rc;
  if ((flags & ~(NSR_ARCH_FUSED_SIGMA_ONLY | NSR_ARCH_FUSED_COLOR_NONE)) != 0) return NSR_ERR_INVALID_ARG;
  const bool sigma_only = (flags & NSR_ARCH_FUSED_SIGMA_ONLY) != 0;
  const int n_in = S.in_xyz + ((sigma_only || S.no_dir) ? 0 : S.in_dir);
  if (!packed || (reinterpret_cast<uintptr_t>(packed) & 15) != 0 || !x || !out || P < 0 || ldx < n_in || ldo < (sigma_only ? 1 : 4))
    return NSR_ERR_INVALID_ARG;
  if ((P + kFusedTile - 1) / kFusedTile > 0x7fffffffLL) return NSR_ERR_INVALID_ARG;
  if (P == 0) return NSR_OK;
  FusedArgs a;
  a.stream = static_cast<const char*>(packed);
  a.x = x; a.ldx = ldx; a.P = P; a.out = out; a.ldo = ldo; a.status = status;
  a.D = S.D; a.skips = S.skips; a.in_xyz = S.in_xyz; a.in_dir = S.in_dir; a.kxb = S.KXB; a.no_dir = S.no_dir;
  a.sigma_only = sigma_only ? 1 : 0;
  a.color_none = (flags & NSR_ARCH_FUSED_COLOR_NONE) ? 1 : 0;
  a.rays = nullptr; a.z = nullptr; a.ray_stride = 0; a.n_samples = 0;
  a.embed = embed; a.bands_pos = NsrBands{}; a.bands_dir = NsrBands{};   // the rows carry the word: only the widths differ
  launch_fused<0>(S.NB, a, nsr_stream(stream));
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

extern "C" int nsr_arch_fused_render_rays(const nsr_arch* arch, const void* packed, const float* rays, int ray_stride, const float* z,
                                          int64_t R, int n_samples, int flags, float* out, int64_t ldo, unsigned* status,
                                          void* stream) {
  return nsr_arch_fused_render_rays_e(arch, 0u, packed, rays, ray_stride, z, R, n_samples, flags, out, ldo, status, stream);
}
extern "C" int nsr_arch_fused_render_rays_e(const nsr_arch* arch, unsigned embed, const void* packed, const float* rays, int ray_stride,
                                            const float* z, int64_t R, int n_samples, int flags, float* out, int64_t ldo,
                                            unsigned* status, void* stream) {
  FusedShape S;
  const int rc = fused_shape(arch, embed, S);
  if (rc != NSR_OK) return rc;
  if ((flags & ~(NSR_ARCH_FUSED_SIGMA_ONLY | NSR_ARCH_FUSED_COLOR_NONE)) != 0) return NSR_ERR_INVALID_ARG;
  const bool sigma_only = (flags & NSR_ARCH_FUSED_SIGMA_ONLY) != 0;
  if (!nsr_ray_stride_ok(ray_stride) || n_samples <= 0 || R < 0) return NSR_ERR_INVALID_ARG;
  if (!packed || (reinterpret_cast<uintptr_t>(packed) & 15) != 0 || !rays || !z || !out || ldo < (sigma_only ? 1 : 4))
    return NSR_ERR_INVALID_ARG;
  if (ray_stride == 8 && (reinterpret_cast<uintptr_t>(rays) & 15) != 0) return NSR_ERR_INVALID_ARG;      // nsr_load_ray's float4 loads
  if (R > (0x7fffffffLL * kFusedTile) / n_samples) return NSR_ERR_INVALID_ARG;      // more than 2^31 - 1 tiles (and no overflow below)
  if (R == 0) return NSR_OK;
  FusedArgs a;
  a.stream = static_cast<const char*>(packed);
  a.x = nullptr; a.ldx = 0; a.P = R * n_samples; a.out = out; a.ldo = ldo; a.status = status;
  a.D = S.D; a.skips = S.skips; a.in_xyz = S.in_xyz; a.in_dir = S.in_dir; a.kxb = S.KXB; a.no_dir = S.no_dir;
  a.sigma_only = sigma_only ? 1 : 0;
  a.color_none = (flags & NSR_ARCH_FUSED_COLOR_NONE) ? 1 : 0;
  a.rays = rays; a.z = z; a.ray_stride = ray_stride; a.n_samples = n_samples;
  a.embed = embed;
  if (nsr_bands(arch->deg_pos, embed, a.bands_pos) != NSR_OK || nsr_bands(arch->deg_dir, embed, a.bands_dir) != NSR_OK)
    return NSR_ERR_INVALID_ARG;
  if (embed != 0u) launch_fused<2>(S.NB, a, nsr_stream(stream));   // embed = 0 keeps the instantiation it always had
  else launch_fused<1>(S.NB, a, nsr_stream(stream));
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
