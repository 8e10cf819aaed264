// sol_lightmap_unwrap.h -- the rule of the lightmap unwrap (sol_lightmap_unwrap, include/solstrale_hip.h), operation by operation.
// The kernels of sol_lightmap_unwrap.hip only fetch, call this text and store. Compiled with -ffp-contract=off: every expression is the plain
// fp32 sequence it spells, `/` and sqrtf are correctly rounded (sol_math.h), so that tests/lightmap_unwrap_ref.py can restate the rule in numpy
// float32 and compare the words. The edge key, its hash and the union-find are sol_lightmap_charts.h's, called, not restated.
//
//   triangle    live: its nine words finite and n = cross(v1 - v0, v2 - v0) with lm_normal(dot(n, n)) (sol_lightmap.h). Its class is 2 a + s:
//               a the index of the largest |n_k|, the lowest on a tie, s = 1 when n_a < 0. Its unit normal is n / sqrt(dot(n, n)), a division
//               per component. A dead triangle gets SOL_LC_NONE and six +0 UV words.
//   join        two live triangles are joined when they share an edge - lc_edge_key over the positions alone (the UV words zero), equal word
//               for word; the hash only sorts candidates together -, have the same class and dot(unit_a, unit_b) >= crease_cos. Every pair of a
//               run of equal keys is judged: the predicate is not transitive, so a fin of three triangles on one edge is three pairs. Charts
//               are the connected components; their ids are dense and in mesh order (the flatten, flag and scan of sol_lightmap_charts.hip).
//   projection  a corner projects to the coordinates ((a + 1) % 3, (a + 2) % 3) of its position, each (p * texels_per_unit) + 0.0f (so that
//               -0 is +0: equal numbers have equal bits).
//   extent      per chart and axis the minimum and the maximum of its corners: integer atomics on lu_ordered, an image of the float that
//               keeps its order. With f = floorf(min) and e = (floorf(max) + 1.0f) - f, the content rectangle is e + 2 texels wide: one guard
//               texel on each side of the e the corners span, because a conservative claim (sol_lightmap.h: closed squares) of a corner that
//               sits on a whole texel line also takes the texel beyond that line. An e that is not in [1, 32765] makes the content 32767.
//   rectangle   content + gutter each way: the gutter follows the content (to the right and above).
//   packing     the rectangles sorted by height descending, then width descending, then chart id ascending (one 64-bit key), walked in that
//               order: a rectangle joins the current shelf while x + w <= width, otherwise it opens the next shelf at x = 0, y += the height
//               of the shelf it leaves; a shelf is as high as its first rectangle, and its first rectangle sits in it whatever its width.
//               The walk stops once y, after a shelf was added to it, is beyond SOL_LIGHTMAP_MAX_SIZE. used_height is that y,
//               used_width the widest shelf walked. overflow bit 0: a rectangle wider than the atlas; bit 1: used_height > height.
//   uv          u = ((x - f_x) + (float)(rect_x + 1)) / (float)width, v = ((y - f_y) + (float)(rect_y + 1)) / (float)height: a corner's
//               UV depends on its position and its chart's placement alone. On overflow every UV word is +0 and every label SOL_LC_NONE.
//
// Self-overlap: the join rule keeps a chart one-to-one in projection locally (a fold flips the class), but a connected surface that passes
// over itself along its axis - a spiral ramp - lands on itself in the atlas. That is not detected; a larger crease_cos cuts such charts apart.
#pragma once
#include "sol_lightmap_charts.h"

#define SOL_LU_MAX_CONTENT 32767u  // the content extent of a chart whose corners span more than 32765 texels (or nothing finite)
#define SOL_LU_MAX_SHELVES 8192u   // (a shelf is at least 3 texels high and the walk ends beyond 16384: at most 5463)

// What the triangle of 9 position words is: its unit normal and its class, or dead.
struct LuTri {
  float ux, uy, uz;
  uint32_t cls;  // 2 a + s, or SOL_LC_NONE
};
DEV LuTri lu_triangle(const float* pos) {
  LuTri T = {0.0f, 0.0f, 0.0f, SOL_LC_NONE};
  bool finite = true;
#pragma unroll
  for (uint32_t k = 0; k < 9u; ++k) finite = finite && lf_finite(pos[k]);
  if (!finite) return T;
  const f3 v0 = mk3(pos[0], pos[1], pos[2]), v1 = mk3(pos[3], pos[4], pos[5]), v2 = mk3(pos[6], pos[7], pos[8]);
  const f3 n = cross3(v1 - v0, v2 - v0);
  const float d = len2(n);
  if (!lm_normal(d)) return T;
  const float ax = fabsf(n.x), ay = fabsf(n.y), az = fabsf(n.z);
  uint32_t a = 0u;
  float best = ax, na = n.x;
  if (ay > best) { a = 1u; best = ay; na = n.y; }
  if (az > best) { a = 2u; na = n.z; }
  const float l = sol_sqrt(d);
  T.ux = n.x / l; T.uy = n.y / l; T.uz = n.z / l;
  T.cls = 2u * a + (na < 0.0f ? 1u : 0u);
  return T;
}
// the join predicate beyond the shared edge
DEV bool lu_join(const LuTri& A, const LuTri& B, float crease_cos) {
  return A.cls == B.cls && (A.ux * B.ux + A.uy * B.uy + A.uz * B.uz) >= crease_cos;
}
// the key of edge e over the positions alone: lc_edge_key with the UV words zero
DEV LcKey lu_edge_key(const float* pos, uint32_t e) {
  const float zero[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  return lc_edge_key(zero, pos, e);
}

// corner c of a triangle of class cls, projected: (x, y) in texels
DEV void lu_project(const float* pos, uint32_t c, uint32_t cls, float texels_per_unit, float& x, float& y) {
  const uint32_t a = cls >> 1, i = a == 2u ? 0u : a + 1u, j = a == 0u ? 2u : a - 1u;
  x = (pos[3u * c + i] * texels_per_unit) + 0.0f;
  y = (pos[3u * c + j] * texels_per_unit) + 0.0f;
}
// an unsigned image of a float that keeps the order of the numbers (no NaN arrives here: finite * finite), and back
DEV uint32_t lu_ordered(float x) {
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
DEV float lu_unordered(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

// the content extent of an axis from its minimum and maximum; f: floorf(lo), the texel line the chart starts at
DEV uint32_t lu_content(float lo, float hi, float& f) {
  f = floorf(lo);
  const float e = (floorf(hi) + 1.0f) - f;
  return (e >= 1.0f && e <= 32765.0f) ? (uint32_t)e + 2u : SOL_LU_MAX_CONTENT;
}
// the sort key of chart `id` with the rectangle (w, h), both below 2^16, id below 2^30: height descending, width descending, id ascending
DEV uint64_t lu_sort_key(uint32_t w, uint32_t h, uint32_t id) {
  return ((uint64_t)(0xFFFFu - h) << 46) | ((uint64_t)(0xFFFFu - w) << 30) | (uint64_t)id;
}
DEV uint32_t lu_key_w(uint64_t k) { return 0xFFFFu - (uint32_t)((k >> 30) & 0xFFFFu); }
DEV uint32_t lu_key_h(uint64_t k) { return 0xFFFFu - (uint32_t)((k >> 46) & 0xFFFFu); }
DEV uint32_t lu_key_id(uint64_t k) { return (uint32_t)(k & 0x3FFFFFFFu); }
// one UV word: x the projected coordinate, f the chart's floorf(min), at the rectangle's place, n the atlas extent
DEV float lu_uv(float x, float f, uint32_t at, uint32_t n) { return ((x - f) + (float)(at + 1u)) / (float)n; }
