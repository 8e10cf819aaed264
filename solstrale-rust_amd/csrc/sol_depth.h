// sol_depth.h -- the rule of the directional distance moments (sol_visibility_oct, sol_volume_build_depth, sol_volume_sample_depth;
// include/solstrale_hip.h), operation by operation. The kernels of sol_depth.hip call this one text. Compiled with
// -ffp-contract=off: every expression is the plain fp32 sequence it spells, `/` and sqrtf are correctly rounded (sol_math.h), so that
// tests/depth_ref.py can restate the rule in numpy float32 and compare the words. dot3 / len2 (sol_math.h) are ((x * x) + (y * y)) + (z * z);
// vol_pos(x) (sol_volume.h) is x > 0 ? x : 0; sgn(x) is x >= 0 ? 1 : -1; |x| clears the sign bit. R is the map's res, (float)R exact.
//
//   map       R x R texels per point or probe, texel (i, j) at row j * R + i, stored without a gutter.
//   decode    u = ((((float)i + 0.5f) / (float)R) * 2) - 1, v likewise from j;  z = (1 - |u|) - |v|;
//             where z < 0: (x, y) = ((1 - |v|) * sgn(u), (1 - |u|) * sgn(v)), else (x, y) = (u, v);  T = (x, y, z) / sqrtf(dot((x, y, z), (x, y, z))).
//   lobe      c = vol_pos(dot(T, d)) with d the sample's direction as drawn; then c = c * c, sharpness_log2 times.
//   sample    HIT (distance t):  w = w + c;  ct = c * t;  wt = wt + ct;  wt2 = wt2 + (ct * t).   MISS:  w = w + c;  w_open = w_open + c.
//             A sample whose made ray is invalid adds nothing. Each sum in chunks of 16 samples counted from first_sample, a chunk from 0 in
//             sample order, the chunks in order onto 0 (sol_radiance's association).
//   build     s = w_open * radius;  mean = (wt + s) / w;  mean2 = (wt2 + (s * radius)) / w.  A texel whose w is not > 0, or one of whose four
//             sums is not finite, is (radius, radius * radius): open as far as the radius.
//   encode    of D with d = sqrtf(dot(D, D)) > 0:  s = (|Dx| + |Dy|) + |Dz|;  px = Dx / s;  py = Dy / s;
//             where Dz < 0: (px, py) = ((1 - |py|) * sgn(px), (1 - |px|) * sgn(py)), both from the unfolded pair;
//             u = (px * 0.5f) + 0.5f, v likewise;  tx = (u * (float)R) - 0.5f;  tx = tx > -0.5f ? tx : -0.5f (a NaN gives -0.5f);
//             tx = tx < (float)R - 0.5f ? tx : (float)R - 0.5f;  i0 = (int)floorf(tx), in [-1, R - 1];  a = tx - floorf(tx);  ty, j0, b likewise.
//   fold      neighbour (i, j), i in [-1, R], j in [-1, R]:  oi = i < 0 || i >= R, oj likewise;  ci = i clamped to [0, R - 1], cj likewise;
//             where oi: cj = (R - 1) - cj;  where oj: ci = (R - 1) - ci.  Beyond one edge the other index is mirrored, beyond a corner both:
//             the octahedron's edge rule. The texel is row cj * R + ci.
//   bilinear  w00 = (1 - a) * (1 - b), w10 = a * (1 - b), w01 = (1 - a) * b, w11 = a * b over the texels (i0, j0), (i0 + 1, j0), (i0, j0 + 1),
//             (i0 + 1, j0 + 1), each folded;  m = ((m00 * w00) + (m10 * w10)) + ((m01 * w01) + (m11 * w11)) for mean and for mean2.
//   sample    sol_volume.h's corner with one change: under SOL_VOLUME_CHEBYSHEV a valid probe at P takes mean, mean2 from its map at the encode
//             of D = q - P where d > 0 - the probe then counts as one with moments, whatever its own bit says -, and has no moments where d is
//             not > 0. Without the flag the map is not read.
#pragma once
#include "sol_volume.h"

#define SOL_OCT_MAX_RES 16
#define SOL_OCT_MAX_SHARPNESS 6u

DEV float oct_sgn(float x) { return x >= 0.0f ? 1.0f : -1.0f; }

// the unit direction of texel (i, j) of an R x R map
DEV f3 oct_texel_direction(uint32_t i, uint32_t j, uint32_t R) {
  const float fr = (float)R;
  const float u = ((((float)i + 0.5f) / fr) * 2.0f) - 1.0f;
  const float v = ((((float)j + 0.5f) / fr) * 2.0f) - 1.0f;
  const float z = (1.0f - fabsf(u)) - fabsf(v);
  float x = u, y = v;
  if (z < 0.0f) {
    x = (1.0f - fabsf(v)) * oct_sgn(u);
    y = (1.0f - fabsf(u)) * oct_sgn(v);
  }
  const f3 t = mk3(x, y, z);
  return t / sqrtf(len2(t));
}

// the lobe weight of a sample's direction in a texel
DEV float oct_lobe(f3 T, f3 d, uint32_t sharpness_log2) {
  float c = vol_pos(dot3(T, d));
  for (uint32_t k = 0; k < sharpness_log2; ++k) c = c * c;
  return c;
}

// What the gather kernel leaves for a sample that did not hit: a hit's word is its distance, a finite number.
#define SOL_DEPTH_MISS 0x7F800000u  // +inf: the ray missed
#define SOL_DEPTH_NONE 0x7FC00000u  // a quiet NaN: no ray was made
// One texel's four sums of a chunk (w, w_open, wt, wt2) and one sample's word.
DEV void oct_add_sample(float (&sum)[4], float c, uint32_t word) {
  if (word == SOL_DEPTH_NONE) return;
  sum[0] = sum[0] + c;
  if (word == SOL_DEPTH_MISS) {
    sum[1] = sum[1] + c;
  } else {
    const float t = __uint_as_float(word);
    const float ct = c * t;
    sum[2] = sum[2] + ct;
    sum[3] = sum[3] + (ct * t);
  }
}

// (mean, mean2) of a texel's four sums
DEV void oct_build(const float (&sum)[4], float radius, float& mean, float& mean2) {
  const bool ok = sum[0] > 0.0f && query_finite(sum[0]) && query_finite(sum[1]) && query_finite(sum[2]) && query_finite(sum[3]);
  if (!ok) {
    mean = radius;
    mean2 = radius * radius;
    return;
  }
  const float s = sum[1] * radius;
  mean = (sum[2] + s) / sum[0];
  mean2 = (sum[3] + (s * radius)) / sum[0];
}

// one axis of the encode: the texel coordinate of u in [0, 1], clamped; the lower neighbour (-1 .. R - 1) and the fraction
DEV void oct_axis(float p, uint32_t R, int& i0, float& a) {
  const float hi = (float)R - 0.5f;
  const float u = (p * 0.5f) + 0.5f;
  float tx = (u * (float)R) - 0.5f;
  tx = tx > -0.5f ? tx : -0.5f;
  tx = tx < hi ? tx : hi;
  const float fl = floorf(tx);
  i0 = (int)fl;
  a = tx - fl;
}
// the row of neighbour (i, j), folded at the map's edges
DEV uint32_t oct_fold(int i, int j, uint32_t R) {
  const int top = (int)R - 1;
  const bool oi = i < 0 || i > top, oj = j < 0 || j > top;
  int ci = i < 0 ? 0 : i > top ? top : i;
  int cj = j < 0 ? 0 : j > top ? top : j;
  if (oi) cj = top - cj;
  if (oj) ci = top - ci;
  return (uint32_t)cj * R + (uint32_t)ci;
}
// The four texels and weights of direction D (not zero): rows[k], wts[k] for k = 00, 10, 01, 11.
DEV void oct_lookup(f3 D, uint32_t R, uint32_t (&rows)[4], float (&wts)[4]) {
  const float s = (fabsf(D.x) + fabsf(D.y)) + fabsf(D.z);
  float px = D.x / s, py = D.y / s;
  if (D.z < 0.0f) {
    const float fx = (1.0f - fabsf(py)) * oct_sgn(px);
    const float fy = (1.0f - fabsf(px)) * oct_sgn(py);
    px = fx;
    py = fy;
  }
  int i0, j0;
  float a, b;
  oct_axis(px, R, i0, a);
  oct_axis(py, R, j0, b);
  rows[0] = oct_fold(i0, j0, R);
  rows[1] = oct_fold(i0 + 1, j0, R);
  rows[2] = oct_fold(i0, j0 + 1, R);
  rows[3] = oct_fold(i0 + 1, j0 + 1, R);
  wts[0] = (1.0f - a) * (1.0f - b);
  wts[1] = a * (1.0f - b);
  wts[2] = (1.0f - a) * b;
  wts[3] = a * b;
}
DEV float oct_bilinear(const float (&m)[4], const float (&wts)[4]) { return ((m[0] * wts[0]) + (m[1] * wts[1])) + ((m[2] * wts[2]) + (m[3] * wts[3])); }
