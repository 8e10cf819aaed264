// sol_triangle.h -- Triangle::new_with_tex_coords (src/hittable/triangle.rs:53-96) in f64, written ONCE for the host and the device: the CPU entry
// point sol_triangle_from_vertices and the records kernel of sol_scene_set_triangles (sol_geometry.hip) run these lines, in the
// operation order of the host mirror (host/solstrale_host.cpp, Triangle::new_with_tex_coords), so that a moved triangle's record is bit for bit
// what a creation from the moved description holds. Compiled with -ffp-contract=off on both sides: every operation below is one IEEE operation.
// Also here: the casts of a SolTriangle to the fp32 device records (DTri in the rotated frame or in the reference's, DTriShade), which creation
// (sol_create.cpp) and the kernel share, and the needle predicate of sol_scene_has_needles for one triangle.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/solstrale_hip.h"
#include "sol_types.h"

#define SOL_TRI_PAD_DELTA 0.0001  // PAD_DELTA (src/geo/mod.rs:11)

// A NaN the arithmetic below makes (a zero-area triangle's normal is 0 / 0; equal texture coordinates give r = 1 / 0 and tangents 0 x inf) is
// the DEFAULT NaN of the processor that made it: sign bit set on x86-64, clear on the GPU. Records are compared byte for byte with those a host
// made, so the device hands out the host's pattern. (Inputs are finite - a move refuses others -, so no NaN payload is ever propagated.)
SOL_HD inline double sol_host_nan(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return x != x ? __longlong_as_double((long long)0xFFF8000000000000ull) : x;
#else
  return x;
#endif
}

// Fills v0, v0v1, v0v2, normal, tangent, bi_tangent, area, uv0..2 and bbox of `t` from the three vertices v = (v0, v1, v2) and uv = (uv0, uv1,
// uv2); material and dfs_index are not touched.
SOL_HD inline void sol_triangle_new(const double v[9], const float uv[6], SolTriangle* t) {
  const double *p0 = v, *p1 = v + 3, *p2 = v + 6;
  // b_box = Aabb::new_from_3_points(v0, v1, v2).pad_if_needed()  (geo/mod.rs:106-150)
  for (int a = 0; a < 3; ++a) {
    double lo = fmin(fmin(p0[a], p1[a]), p2[a]), hi = fmax(fmax(p0[a], p1[a]), p2[a]);
    if (!(hi - lo >= SOL_TRI_PAD_DELTA)) { lo = lo - SOL_TRI_PAD_DELTA / 2.; hi = hi + SOL_TRI_PAD_DELTA / 2.; }  // Interval::expand
    t->bbox.v[2 * a] = lo; t->bbox.v[2 * a + 1] = hi;
  }
  double e1[3], e2[3];
  for (int a = 0; a < 3; ++a) { e1[a] = p1[a] - p0[a]; e2[a] = p2[a] - p0[a]; }
  const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  for (int a = 0; a < 3; ++a) t->normal[a] = sol_host_nan(n[a] / len);
  t->area = len / 2.;
  // the tangents: Uv arithmetic in f32 (geo/mod.rs:15-20), the rest in f64
  const float d1u = uv[2] - uv[0], d1v = uv[3] - uv[1], d2u = uv[4] - uv[0], d2v = uv[5] - uv[1];
  const float r = 1.0f / (d1u * d2v - d1v * d2u);
  double tg[3], bt[3];
  for (int a = 0; a < 3; ++a) {
    tg[a] = (e1[a] * (double)d2v - e2[a] * (double)d1v) * (double)r;
    bt[a] = (e2[a] * (double)d1u - e1[a] * (double)d2u) * (double)r;
  }
  const double tl = sqrt(tg[0] * tg[0] + tg[1] * tg[1] + tg[2] * tg[2]), bl = sqrt(bt[0] * bt[0] + bt[1] * bt[1] + bt[2] * bt[2]);
  for (int a = 0; a < 3; ++a) {
    t->tangent[a] = sol_host_nan(tg[a] / tl); t->bi_tangent[a] = sol_host_nan(bt[a] / bl);
    t->v0[a] = p0[a]; t->v0v1[a] = e1[a]; t->v0v2[a] = e2[a];
  }
  t->uv0[0] = uv[0]; t->uv0[1] = uv[1]; t->uv1[0] = uv[2]; t->uv1[1] = uv[3]; t->uv2[0] = uv[4]; t->uv2[1] = uv[5];
}

// sol_scene_has_needles (include/solstrale_hip.h) for one triangle: the same expressions.
SOL_HD inline bool sol_triangle_is_needle(const SolTriangle* t) {
  const double a[3] = {t->v0v1[0], t->v0v1[1], t->v0v1[2]}, b[3] = {t->v0v2[0], t->v0v2[1], t->v0v2[2]};
  const double c[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  double l2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
  const double lb = b[0] * b[0] + b[1] * b[1] + b[2] * b[2], lc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
  if (lb > l2) l2 = lb;
  if (lc > l2) l2 = lc;
  return !(l2 < 2.0 * SOL_NEEDLE_ASPECT * t->area);
}

// sol_triangle_rotation / sol_triangle_rotated of the header, callable from device code (static inline C functions are host functions to hipcc).
SOL_HD inline int sol_tri_rotation(const SolTriangle* t) {
  const double a[3] = {t->v0v1[0], t->v0v1[1], t->v0v1[2]}, b[3] = {t->v0v2[0], t->v0v2[1], t->v0v2[2]};
  const double c[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const double l01 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2], l02 = b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
  const double l12 = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
  int k = 0;
  double best = l12;
  if (l02 > best) { best = l02; k = 1; }
  if (l01 > best) { k = 2; }
  return k;
}
SOL_HD inline void sol_tri_rotated(const SolTriangle* t, int k, double v0[3], double e1[3], double e2[3], int uv_of[3]) {
  for (int i = 0; i < 3; ++i) {
    const double p0 = t->v0[i], a = t->v0v1[i], b = t->v0v2[i];
    if (k == 1) { v0[i] = p0 + a; e1[i] = b - a; e2[i] = -a; }
    else if (k == 2) { v0[i] = p0 + b; e1[i] = -b; e2[i] = a - b; }
    else { v0[i] = p0; e1[i] = a; e2[i] = b; }
  }
  uv_of[0] = k % 3; uv_of[1] = (k + 1) % 3; uv_of[2] = (k + 2) % 3;
}

// A triangle's fp32 intersect record: starts at the vertex opposite the longest edge (fp32 arithmetic contract, solstrale_hip.h
// sol_triangle_rotation; the oracle's float instantiation makes the same choice); `reference_order`: as the reference lists the vertices -
// the frame a triangle LIGHT is sampled in (DevScene::light_tri). uv_of = which of {uv0, uv1, uv2} belongs to the record's three vertices.
SOL_HD inline void sol_tri_cast(const SolTriangle* t, bool reference_order, DTri* o, int uv_of[3]) {
  double v0[3], e1[3], e2[3];
  sol_tri_rotated(t, reference_order ? 0 : sol_tri_rotation(t), v0, e1, e2, uv_of);
  o->v0x = (float)v0[0]; o->v0y = (float)v0[1]; o->v0z = (float)v0[2];
  o->e1x = (float)e1[0]; o->e1y = (float)e1[1]; o->e1z = (float)e1[2];
  o->e2x = (float)e2[0]; o->e2y = (float)e2[1]; o->e2z = (float)e2[2];
  o->dfs = t->dfs_index; o->mat = t->material; o->area = (float)t->area;
}
// ... and its shading record, the texture coordinates in the order of the record's vertices
SOL_HD inline void sol_tri_cast_shade(const SolTriangle* t, const int uo[3], DTriShade* s) {
  // (selects between values, not an array indexed at run time: that would put the triangle into scratch memory on the device)
  const float u[3] = {t->uv0[0], t->uv1[0], t->uv2[0]}, v[3] = {t->uv0[1], t->uv1[1], t->uv2[1]};
  auto pick = [&](int j, int c) { return c == 0 ? (j == 0 ? u[0] : j == 1 ? u[1] : u[2]) : (j == 0 ? v[0] : j == 1 ? v[1] : v[2]); };
  s->nx = (float)t->normal[0]; s->ny = (float)t->normal[1]; s->nz = (float)t->normal[2]; s->mat = t->material;
  s->tx = (float)t->tangent[0]; s->ty = (float)t->tangent[1]; s->tz = (float)t->tangent[2];
  s->bx = (float)t->bi_tangent[0]; s->by = (float)t->bi_tangent[1]; s->bz = (float)t->bi_tangent[2];
  s->u0 = pick(uo[0], 0); s->v0 = pick(uo[0], 1); s->u1 = pick(uo[1], 0); s->v1 = pick(uo[1], 1); s->u2 = pick(uo[2], 0); s->v2 = pick(uo[2], 1);
}
