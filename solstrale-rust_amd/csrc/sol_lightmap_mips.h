// sol_lightmap_mips.h -- the rule of the lightmap mip chain, the trilinear lookup and the level of detail of a hit (sol_lightmap_mips,
// sol_lightmap_sample_lod, sol_lightmap_lod, include/solstrale_hip.h), operation by operation. The kernels of sol_lightmap_mips.hip
// only fetch, call this text and store. Compiled with -ffp-contract=off: every expression is the plain fp32 sequence it spells, `/` and sqrtf are
// correctly rounded, so that tests/lightmap_mips_ref.py can restate the rule in numpy float32 and compare the words. No fmaxf, no fminf, no fused
// multiply-add: every clamp is a comparison; finiteness is the exponent field (lf_finite).
//
//   layout        level 0 is the caller's W x H atlas. W_l = (W_{l-1} + 1) / 2, H_l likewise (a ceiling; 1 stays 1). The full count is the first
//                 l + 1 at which W_l == H_l == 1. The chain holds levels 1 .. levels - 1 packed in this order, level l at row
//                 sum_{k=1}^{l-1} W_k * H_k; rows have level 0's stride; the cover plane has one byte per row, 0 covered, 255 not.
//   reduction     texel (i, j) of level l + 1 looks at (2i, 2j), (2i + 1, 2j), (2i, 2j + 1), (2i + 1, 2j + 1) of level l in this order; the taps
//                 inside level l and live count c; a channel is ((0 + x_a) + x_b ..) / (float)c over the live taps in tap order; the words behind
//                 the channels are the first live tap's. One channel not finite, or c == 0: a zero row with cover 255.
//   lookup        x = ((u * (float)W) * 2^-l) - 0.5f against the level's own W_l, H_l; everything else is sol_lightmap_sample.h's.
//   lod           sol_lightmap.h's lm_setup judges the triangle and gives the texel-space area; see lml_lod below for the order of operations.
#pragma once
#include "sol_lightmap.h"
#include "sol_lightmap_sample.h"
#include "sol_launch.h"  // LmmLayout, lmm_layout: the layout rule, shared with the host

#define SOL_LMM_UNCOVERED 255u

// ---- reduction ----
// 2^-l as an exact constant, l = 0 .. 14
DEV float lmm_inv_pow2(uint32_t l) { return __uint_as_float((127u - l) << 23); }

// one channel of a destination texel: the live taps added in tap order onto 0, divided by their count
DEV float lmm_mean(uint32_t live, float x0, float x1, float x2, float x3, float fc) {
  float sum = 0.0f;
  if (live & 1u) sum = sum + x0;
  if (live & 2u) sum = sum + x1;
  if (live & 4u) sum = sum + x2;
  if (live & 8u) sum = sum + x3;
  return sum / fc;
}

// One destination texel (i, j) from its four taps, `live` the mask of the live ones. Src answers word(i, j, w) for a live tap; the row is written
// through Dst::put(w, bits); returns the cover byte. The words are produced in order and stored as they come; a row with a channel that is not
// finite is written again as zeros by the same lane.
template <typename Src, typename Dst>
DEV uint32_t lmm_reduce(const Src& S, uint32_t live, uint32_t i, uint32_t j, uint32_t channels, uint32_t stride_words, Dst& D) {
  if (live == 0u) {
    for (uint32_t w = 0; w < stride_words; ++w) D.put(w, 0u);
    return SOL_LMM_UNCOVERED;
  }
  const float fc = (float)__builtin_popcount(live);
  const uint32_t first = (uint32_t)__builtin_ctz(live);
  bool finite = true;
  for (uint32_t w = 0; w < stride_words; ++w) {
    if (w < channels) {
      float x[4];
#pragma unroll
      for (uint32_t k = 0; k < 4u; ++k) x[k] = (live & (1u << k)) ? __uint_as_float(S.word(2u * i + (k & 1u), 2u * j + (k >> 1), w)) : 0.0f;
      const float m = lmm_mean(live, x[0], x[1], x[2], x[3], fc);
      finite = finite && lf_finite(m);
      D.put(w, __float_as_uint(m));
    } else {
      D.put(w, S.word(2u * i + (first & 1u), 2u * j + (first >> 1), w));
    }
  }
  if (finite) return 0u;
  for (uint32_t w = 0; w < stride_words; ++w) D.put(w, 0u);
  return SOL_LMM_UNCOVERED;
}

// ---- the trilinear lookup ----
// lod[i] as the rule reads it: 0 unless > 0 (NaN reads as 0), levels - 1 when at least that
DEV float lml_clamp(float lod, uint32_t levels) {
  const float top = (float)(levels - 1u);
  float x = lod > 0.0f ? lod : 0.0f;
  if (x >= top) x = top;
  return x;
}
// The taps of a row over level l >= 1 (level 0 is ls_taps itself): ls_taps' bilinear branch with x = ((u * (float)W) * 2^-l) - 0.5f tested
// against the level's own size.
DEV LsTaps lml_taps(float u, float v, uint32_t W, uint32_t H, uint32_t l, uint32_t Wl, uint32_t Hl) {
  LsTaps t = {0, 0, 0.0f, 0.0f, 0u};
  const float s = lmm_inv_pow2(l);
  const float x = ((u * (float)W) * s) - 0.5f, y = ((v * (float)H) * s) - 0.5f;
  if (!(x >= -1.0f && x < (float)Wl && y >= -1.0f && y < (float)Hl)) return t;
  const float xf = floorf(x), yf = floorf(y);
  t.i0 = (int)xf; t.j0 = (int)yf;
  t.fx = x - xf; t.fy = y - yf;
  t.n = 4u;
  return t;
}
// the blend of two levels' answers, f in (0, 1): 1 - f is rounded once by the caller
DEV float lml_blend(float a, float b, float g, float f) { return (a * g) + (b * f); }

// ---- the level of detail of a hit ----
// the piecewise-linear logarithm from the bits of a positive normal number
DEV float lml_plog2(float q) {
  const uint32_t bits = __float_as_uint(q);
  return (float)((int)(bits >> 23) - 127) + (float)(bits & 0x7FFFFFu) * 1.1920928955078125e-07f;  // 2^-23
}
// uv: the triangle's 6 UV words, pos: its 9 vertex words, D: the ray's direction (finite, judged by the caller), t: the hit's distance (finite, > 0, judged by the caller).
DEV float lml_lod(const float* uv, const float* pos, float dx, float dy, float dz, float t, uint32_t W, uint32_t H, float spread, float bias) {
  LmTri T;
  if (!lm_setup(uv, pos, nullptr, (float)W, (float)H, T)) return 0.0f;  // a word not finite, no texel-space area, no world area
  const f3 v0 = mk3(pos[0], pos[1], pos[2]), v1 = mk3(pos[3], pos[4], pos[5]), v2 = mk3(pos[6], pos[7], pos[8]);
  const f3 N = cross3(v1 - v0, v2 - v0), D = mk3(dx, dy, dz);
  const float nn = len2(N), dd = len2(D), dn = dot3(D, N);
  float c2 = (dn * dn) / (dd * nn);
  if (!(c2 >= 0.015625f)) c2 = 0.015625f;  // a cosine floor of 1/8 (also for a direction without length: NaN)
  const float r = spread * t;
  const float q = ((r * r) * (T.area2 / sol_sqrt(nn))) / c2;
  float lambda = bias;
  if (q > 1.0f) lambda = bias + (0.5f * lml_plog2(q));
  return lambda > 0.0f ? lambda : 0.0f;
}
