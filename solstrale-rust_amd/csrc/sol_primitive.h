// sol_primitive.h -- Sphere::new (src/hittable/sphere.rs:25-36) and Quad::new without a transformer (src/hittable/quad.rs:34-66) in f64, written
// ONCE for the host and the device: the CPU entry points sol_sphere_from_center / sol_quad_from_corner and the records kernels of
// sol_scene_set_primitives (sol_geometry.hip) run these lines, in the operation order of the host mirror (host/solstrale_host.cpp,
// Sphere::create and Quad::create), so that a moved primitive's record is bit for bit what a creation from the moved description holds. Compiled
// with -ffp-contract=off on both sides: every operation below is one IEEE operation. Also here: the casts of a SolSphere / SolQuad to the fp32
// device records, which creation (sol_create.cpp, cast_primitives) and the kernels share.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/solstrale_hip.h"
#include "sol_triangle.h"  // SOL_TRI_PAD_DELTA, sol_host_nan
#include "sol_types.h"

// Fills center, radius and bbox of `s`; material and dfs_index are not touched. The box is Aabb::new_from_2_points(center - r, center + r): min and
// max per axis, so a negative radius gives the box of its magnitude.
SOL_HD inline void sol_sphere_new(const double c[3], double radius, SolSphere* s) {
  for (int a = 0; a < 3; ++a) {
    const double p = c[a] - radius, q = c[a] + radius;
    s->center[a] = c[a];
    s->bbox.v[2 * a] = fmin(p, q); s->bbox.v[2 * a + 1] = fmax(p, q);
  }
  s->radius = radius;
}

// Fills q, u, v, normal, d, w, area and bbox of `o`; material and dfs_index are not touched. A quad with u parallel to v has n = 0: normal and w
// are 0 / 0, d is a product with them - the host's NaN pattern on both sides (sol_host_nan, sol_triangle.h).
SOL_HD inline void sol_quad_new(const double q[3], const double u[3], const double v[3], SolQuad* o) {
  // b_box = Aabb::default().combine(2 points(q, q + u)).combine(2 points(q, q + v)).combine(2 points(q, q + u + v)).pad_if_needed()
  for (int a = 0; a < 3; ++a) {
    const double pu = q[a] + u[a], pv = q[a] + v[a], puv = pu + v[a];
    double lo = __builtin_huge_val(), hi = -__builtin_huge_val();  // EMPTY_INTERVAL
    lo = fmin(lo, fmin(q[a], pu)); hi = fmax(hi, fmax(q[a], pu));
    lo = fmin(lo, fmin(q[a], pv)); hi = fmax(hi, fmax(q[a], pv));
    lo = fmin(lo, fmin(q[a], puv)); hi = fmax(hi, fmax(q[a], puv));
    if (!(hi - lo >= SOL_TRI_PAD_DELTA)) { lo = lo - SOL_TRI_PAD_DELTA / 2.; hi = hi + SOL_TRI_PAD_DELTA / 2.; }  // Interval::expand
    o->bbox.v[2 * a] = lo; o->bbox.v[2 * a + 1] = hi;
  }
  const double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
  const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
  const double len = sqrt(nn);
  for (int a = 0; a < 3; ++a) {
    o->q[a] = q[a]; o->u[a] = u[a]; o->v[a] = v[a];
    o->normal[a] = sol_host_nan(n[a] / len);
    o->w[a] = sol_host_nan(n[a] / nn);
  }
  o->d = sol_host_nan(o->normal[0] * q[0] + o->normal[1] * q[1] + o->normal[2] * q[2]);
  o->area = len;
}

// The fp32 device records (sol_types.h) of a description's sphere and quad: plain casts.
SOL_HD inline void sol_sphere_cast(const SolSphere* s, DSphere* o) {
  o->cx = (float)s->center[0]; o->cy = (float)s->center[1]; o->cz = (float)s->center[2];
  o->radius = fabsf((float)s->radius);  // |r|: the reference uses r^2 and a min/max box only (sphere.rs:26-28,68), the fp32 rules of sol_trace.h / sol_shade.h use r itself
  o->dfs = s->dfs_index; o->mat = s->material; o->pad0 = o->pad1 = 0;
}
SOL_HD inline void sol_quad_cast(const SolQuad* q, DQuad* o) {
  o->nx = (float)q->normal[0]; o->ny = (float)q->normal[1]; o->nz = (float)q->normal[2]; o->d = (float)q->d;
  o->qx = (float)q->q[0]; o->qy = (float)q->q[1]; o->qz = (float)q->q[2]; o->dfs = q->dfs_index;
  o->wx = (float)q->w[0]; o->wy = (float)q->w[1]; o->wz = (float)q->w[2]; o->mat = q->material;
  o->ux = (float)q->u[0]; o->uy = (float)q->u[1]; o->uz = (float)q->u[2]; o->area = (float)q->area;
  o->vx = (float)q->v[0]; o->vy = (float)q->v[1]; o->vz = (float)q->v[2]; o->pad = 0.f;
}
