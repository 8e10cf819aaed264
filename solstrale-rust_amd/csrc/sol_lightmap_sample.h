// sol_lightmap_sample.h -- the rule of the lightmap lookup (sol_lightmap_coords, sol_lightmap_sample, include/solstrale_hip.h),
// operation by operation. The kernels of sol_lightmap_sample.hip only fetch, call this text and store. Compiled with -ffp-contract=off: every
// expression is the plain fp32 sequence it spells and `/` is correctly rounded, so that tests/lightmap_sample_ref.py can restate the rule in numpy
// float32 and compare the words. No fmaxf, no fminf: every clamp is a comparison; finiteness is the exponent field (lf_finite).
//
//   surface row   a SolTexel: (triangle, b1, b2, flags) - the weights of the triangle's second and third corner; flags != 0: usable.
//   coords        A triangle hit's (u, v) weigh the two edges of the triangle's fp32 RECORD, and that record starts at the vertex opposite the
//                 longest edge (sol_triangle_rotation, include/solstrale_hip.h): it is the description's (v0, v0v1, v0v2) only for rotation 0.
//                 The caller's table therefore carries the rotation k in the two top bits of an entry, entry = triangle | k << 30, and
//                   k = 0: b1 = u,            b2 = v
//                   k = 1: b1 = (1 - u) - v,  b2 = u
//                   k = 2: b1 = v,            b2 = (1 - u) - v
//                 (record k starts at corner k and goes round in the triangle's own order). An entry of SOL_TEXEL_NONE, or one with k = 3, is a
//                 primitive without lightmap. The parts of a pre-split triangle are copies of one record: they answer the original's (u, v).
//   atlas         sol_lightmap.h's: texel (i, j) has its centre at ((float)i + 0.5f, (float)j + 0.5f), row j = 0 is v = 0, index j * W + i.
//   associations  b0 = (1 - b1) - b2; an interpolated word is ((a0 * b0) + (a1 * b1)) + (a2 * b2); x = (u * (float)W) - 0.5f; a tap weight is
//                 ONE product of two of fx, 1 - fx, fy, 1 - fy; sum = ((0 + (w_a * x_a)) + (w_b * x_b)) .. and wsum = ((0 + w_a) + w_b) .. over
//                 the live taps in tap order; the squared distance of the chart guard is lf_dot(E, E) of E = P_tap - P, compared with the one
//                 product r * r.
//   chart guard   protects against an OWNED texel of a neighbouring chart. A tap that only the dilation filled has no point row and stays live
//                 untested, and so does an owned tap whose position words are not finite: a gutter narrower than the dilation still mixes charts.
#pragma once
#include "sol_lightmap_filter.h"

#define SOL_LS_NONE 0xFFFFFFFFu
#define SOL_LS_ROTATION_SHIFT 30u
#define SOL_LS_TRIANGLE_MASK 0x3FFFFFFFu

// ---- sol_lightmap_coords ----
// The surface row of one hit; entry: the caller's table at the hit's dfs_index (read only when `listed`: a triangle hit whose dfs_index the table holds).
struct LsRow {
  uint32_t triangle;
  float b1, b2;
  uint32_t flags;
};
DEV LsRow ls_coords(bool listed, uint32_t entry, float u, float v) {
  const uint32_t k = entry >> SOL_LS_ROTATION_SHIFT;
  if (!listed || k == 3u) return LsRow{SOL_LS_NONE, 0.0f, 0.0f, 0u};
  const float w = (1.0f - u) - v;
  return LsRow{entry & SOL_LS_TRIANGLE_MASK, k == 0u ? u : k == 1u ? w : v, k == 0u ? v : k == 1u ? u : w, 1u};
}

// ---- sol_lightmap_sample ----
DEV float ls_lerp3(float a0, float a1, float a2, float b0, float b1, float b2) { return ((a0 * b0) + (a1 * b1)) + (a2 * b2); }

// The taps of a row: up to four texels (i[t], j[t]) with weight w[t], in tap order; n = 0: the lookup leaves the atlas altogether. A tap may
// still lie outside (ls_tap_inside). Nothing is converted to an integer before the comparisons have bounded it.
struct LsTaps {
  int i0, j0;
  float fx, fy;
  uint32_t n;  // 4 bilinear, 1 nearest, 0 none
};
DEV LsTaps ls_taps(float u, float v, uint32_t W, uint32_t H, bool nearest) {
  const float fw = (float)W, fh = (float)H;
  LsTaps t = {0, 0, 0.0f, 0.0f, 0u};
  if (nearest) {
    const float x = u * fw, y = v * fh;
    if (!(x >= 0.0f && x < fw && y >= 0.0f && y < fh)) return t;
    t.i0 = (int)floorf(x); t.j0 = (int)floorf(y); t.n = 1u;
    return t;
  }
  const float x = (u * fw) - 0.5f, y = (v * fh) - 0.5f;
  if (!(x >= -1.0f && x < fw && y >= -1.0f && y < fh)) return t;
  const float xf = floorf(x), yf = floorf(y);
  t.i0 = (int)xf; t.j0 = (int)yf;
  t.fx = x - xf; t.fy = y - yf;  // (float)i0 is xf exactly
  t.n = 4u;
  return t;
}
DEV int ls_tap_i(const LsTaps& t, uint32_t k) { return t.i0 + (int)(k & 1u); }
DEV int ls_tap_j(const LsTaps& t, uint32_t k) { return t.j0 + (int)(k >> 1); }
DEV bool ls_tap_inside(int i, int j, uint32_t W, uint32_t H) { return i >= 0 && j >= 0 && i < (int)W && j < (int)H; }
DEV float ls_tap_weight(const LsTaps& t, uint32_t k) {
  const float wx = (k & 1u) ? t.fx : 1.0f - t.fx, wy = (k >> 1) ? t.fy : 1.0f - t.fy;
  return wx * wy;
}
// covered: the dilation's plane where there is one, else ownership
DEV bool ls_covered(bool have_pass_of, uint32_t pass_of, uint32_t tap_triangle) { return have_pass_of ? pass_of != 255u : tap_triangle != SOL_LS_NONE; }
// The chart guard of one tap: P the shaded point, Q the tap's stored position. false: the tap is an owned texel of another place.
DEV bool ls_guard(uint32_t tap_flags, float qx, float qy, float qz, float px, float py, float pz, float r2) {
  if (tap_flags == 0u || !(lf_finite(qx) && lf_finite(qy) && lf_finite(qz))) return true;
  const float ex = qx - px, ey = qy - py, ez = qz - pz;
  return lf_dot(ex, ey, ez, ex, ey, ez) <= r2;
}
