// sol_lightmap.h -- the rule of the lightmap rasteriser (sol_lightmap_points, include/solstrale_hip.h), operation by operation.
// Both passes of sol_lightmap.hip call this one text: the claim pass decides with lm_classify which texels a triangle claims, the emit pass
// evaluates lm_classify's edge functions again for the owner and writes the row with lm_row. Compiled with -ffp-contract=off: every expression
// is the plain fp32 sequence it spells, `/` and sqrtf are correctly rounded (sol_math.h), so that tests/lightmap_ref.py can restate the rule in
// numpy float32 and compare the words.
//
//   texel space   a UV corner is (u * (float)W, v * (float)H); texel (i, j) is the square [i, i + 1] x [j, j + 1] with its centre at
//                 ((float)i + 0.5f, (float)j + 0.5f); row j = 0 is v = 0.
//   candidates    a triangle claims only among the texels whose closed square overlaps its closed texel-space bounding box:
//                 (float)i <= max x && (float)(i + 1) >= min x, and the same in y (lm_range: the same set as integer bounds).
//   edges         edge(Q, R, P) = (Rx - Qx) * (Py - Qy) - (Ry - Qy) * (Px - Qx), always evaluated with (Q, R) in lexicographic order (x, then
//                 y) and negated when the triangle's own order is the other one: two triangles compute the same number for a shared edge.
//                 e0 = edge(B, C, P), e1 = edge(C, A, P), e2 = edge(A, B, P); all three and area2 are negated when area2 < 0.
#pragma once
#include "sol_math.h"
#include "sol_ray.h"

#define SOL_LM_EMPTY 0xFFFFFFFFu
#define SOL_LM_CONSERVATIVE_BIT 0x80000000u

// a finite fp32 number that is not zero and not subnormal
DEV bool lm_normal(float x) {
  const uint32_t e = __float_as_uint(x) & 0x7F800000u;
  return e != 0u && e != 0x7F800000u;
}

// A triangle as both passes see it: its corners in texel space and its doubled signed area, made positive (`flip`: it was negative).
struct LmTri {
  float ax, ay, bx, by, cx, cy, area2;
  bool flip;
};

// The triangle of 6 UV words, 9 position words and (or null) 9 normal words; false: the triangle is skipped - a word that is not finite, a
// texel-space area that is zero or not finite, or a geometric normal whose squared length is not a finite, normal number.
DEV bool lm_setup(const float* uv, const float* pos, const float* nrm, float W, float H, LmTri& t) {
  bool finite = true;
  for (int k = 0; k < 6; ++k) finite = finite && query_finite(uv[k]);
  for (int k = 0; k < 9; ++k) finite = finite && query_finite(pos[k]);
  if (nrm)
    for (int k = 0; k < 9; ++k) finite = finite && query_finite(nrm[k]);
  if (!finite) return false;
  t.ax = uv[0] * W; t.ay = uv[1] * H;
  t.bx = uv[2] * W; t.by = uv[3] * H;
  t.cx = uv[4] * W; t.cy = uv[5] * H;
  const float area2 = (t.bx - t.ax) * (t.cy - t.ay) - (t.by - t.ay) * (t.cx - t.ax);
  if (area2 == 0.0f || !query_finite(area2)) return false;
  t.flip = area2 < 0.0f;
  t.area2 = t.flip ? -area2 : area2;
  const f3 v0 = mk3(pos[0], pos[1], pos[2]), v1 = mk3(pos[3], pos[4], pos[5]), v2 = mk3(pos[6], pos[7], pos[8]);
  return lm_normal(len2(cross3(v1 - v0, v2 - v0)));
}

// The candidates of `t` in a W x H atlas as inclusive integer bounds; false: none. ceilf / floorf are exact, and a bound beyond 2^24 is far
// outside every atlas (W, H <= 16384) before and after the rounding of `- 1.0f`.
DEV bool lm_range(const LmTri& t, uint32_t W, uint32_t H, uint32_t& i0, uint32_t& i1, uint32_t& j0, uint32_t& j1) {
  const float xmin = fminf(fminf(t.ax, t.bx), t.cx), xmax = fmaxf(fmaxf(t.ax, t.bx), t.cx);
  const float ymin = fminf(fminf(t.ay, t.by), t.cy), ymax = fmaxf(fmaxf(t.ay, t.by), t.cy);
  const float lo_x = fmaxf(ceilf(xmin) - 1.0f, 0.0f), hi_x = fminf(floorf(xmax), (float)(W - 1u));
  const float lo_y = fmaxf(ceilf(ymin) - 1.0f, 0.0f), hi_y = fminf(floorf(ymax), (float)(H - 1u));
  if (!(lo_x <= hi_x && lo_y <= hi_y)) return false;
  i0 = (uint32_t)lo_x; i1 = (uint32_t)hi_x; j0 = (uint32_t)lo_y; j1 = (uint32_t)hi_y;
  return true;
}

// edge(Q, R, P) in the lexicographic order of (Q, R)
DEV float lm_edge(float qx, float qy, float rx, float ry, float px, float py) {
  if (qx < rx || (qx == rx && qy <= ry)) return (rx - qx) * (py - qy) - (ry - qy) * (px - qx);
  return -((qx - rx) * (py - ry) - (qy - ry) * (px - rx));
}
DEV void lm_edges(const LmTri& t, float px, float py, float& e0, float& e1, float& e2) {
  e0 = lm_edge(t.bx, t.by, t.cx, t.cy, px, py);
  e1 = lm_edge(t.cx, t.cy, t.ax, t.ay, px, py);
  e2 = lm_edge(t.ax, t.ay, t.bx, t.by, px, py);
  if (t.flip) { e0 = -e0; e1 = -e1; e2 = -e2; }
}

// What `t` claims of its candidate texel (i, j): 1 the centre is inside (every edge >= 0 there); 2 (only with `conservative`) it is not, but
// for each edge some corner of the texel square has the edge >= 0 - "the maximum over the four corners is >= 0", said so that a NaN decides
// nothing; 0 nothing.
DEV uint32_t lm_classify(const LmTri& t, uint32_t i, uint32_t j, bool conservative) {
  float e0, e1, e2;
  lm_edges(t, (float)i + 0.5f, (float)j + 0.5f, e0, e1, e2);
  if (e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f) return 1u;
  if (!conservative) return 0u;
  bool in0 = false, in1 = false, in2 = false;
  for (uint32_t c = 0; c < 4u; ++c) {
    lm_edges(t, (float)(i + (c & 1u)), (float)(j + (c >> 1)), e0, e1, e2);
    in0 = in0 || e0 >= 0.0f; in1 = in1 || e1 >= 0.0f; in2 = in2 || e2 >= 0.0f;
  }
  return in0 && in1 && in2 ? 2u : 0u;
}
// the 32-bit key of a claim: one atomicMin per claim makes the lowest index among the centre claims win, then the lowest conservative-only one
DEV uint32_t lm_key(uint32_t triangle, uint32_t claim) { return triangle | (claim == 2u ? SOL_LM_CONSERVATIVE_BIT : 0u); }

// The point row and the barycentrics of texel (i, j), owned by `t` with claim `claim` (1 or 2): row = (position, tmin, normal, tmax).
DEV void lm_row(const LmTri& t, const float* pos, const float* nrm, uint32_t i, uint32_t j, uint32_t claim, float tmin, float tmax, float* row,
                float& b1_out, float& b2_out) {
  float e0, e1, e2;
  lm_edges(t, (float)i + 0.5f, (float)j + 0.5f, e0, e1, e2);
  float b1 = e1 / t.area2, b2 = e2 / t.area2;
  float b0 = (1.0f - b1) - b2;
  if (claim == 2u) {  // the centre is outside: the nearest weights that are not negative, renormalised
    const float c0 = b0 > 0.0f ? b0 : 0.0f, c1 = b1 > 0.0f ? b1 : 0.0f, c2 = b2 > 0.0f ? b2 : 0.0f;
    const float s = (c0 + c1) + c2;
    b1 = c1 / s; b2 = c2 / s;
    b0 = (1.0f - b1) - b2;
  }
  const f3 v0 = mk3(pos[0], pos[1], pos[2]), v1 = mk3(pos[3], pos[4], pos[5]), v2 = mk3(pos[6], pos[7], pos[8]);
  const f3 p = ((v0 * b0) + (v1 * b1)) + (v2 * b2);
  f3 n = cross3(v1 - v0, v2 - v0);
  if (nrm) {
    const f3 m = ((mk3(nrm[0], nrm[1], nrm[2]) * b0) + (mk3(nrm[3], nrm[4], nrm[5]) * b1)) + (mk3(nrm[6], nrm[7], nrm[8]) * b2);
    if (lm_normal(len2(m))) n = m;
  }
  n = unit3(n);
  row[0] = p.x; row[1] = p.y; row[2] = p.z; row[3] = tmin;
  row[4] = n.x; row[5] = n.y; row[6] = n.z; row[7] = tmax;
  b1_out = b1; b2_out = b2;
}

// ---- border dilation (sol_lightmap_dilate) ----
// The neighbours of a texel in the order their values are added: (di, dj) of neighbour k.
DEV int lm_di(uint32_t k) { return (int)((0x21020210u >> (4u * k)) & 3u) - 1; }  // -1 0 1 -1 1 -1 0 1
DEV int lm_dj(uint32_t k) { return k < 3u ? -1 : k < 5u ? 0 : 1; }
