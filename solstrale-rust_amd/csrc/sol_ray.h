// sol_ray.h -- what the kernels that take the caller's own rays share (sol_query.hip, sol_radiance.hip): the validity rule of a SolRay
// (include/solstrale_hip.h), decided per ray by the kernel itself before any search, and the direction an irradiance query draws at a point.
#pragma once
#include "sol_math.h"
#include "sol_shade.h"

// finite: neither an infinity nor a NaN
DEV bool query_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
// a = (origin, tmin), b = (direction, tmax). Valid: every component finite (tmax may be +inf), a direction that is not zero, 0 <= tmin <= tmax
// (a NaN tmax fails the last comparison, -inf the one before).
DEV bool query_ray_valid(float4 a, float4 b) {
  const bool finite = query_finite(a.x) && query_finite(a.y) && query_finite(a.z) && query_finite(a.w) && query_finite(b.x) &&
                      query_finite(b.y) && query_finite(b.z);
  const bool dir = b.x != 0.0f || b.y != 0.0f || b.z != 0.0f;
  return finite && dir && a.w >= 0.0f && a.w <= b.w;
}

// What a finished search (t.cur == REF_DONE) of a caller's ray answers - one text for sol_query_kernel and sol_visibility_kernel. `settled`
// runs when t.h is the answer (no primitive in it: a miss). It does not (STRICT, scenes with needle triangles) when the closest hit was a
// triangle the consistency rule refuses: `t` is then set up to search the same ray again behind it, up to the ray's own upper end `tmax` -
// `left` counts the searches a ray may still start, 63 at its first (closest_hit's guard: 64 searches in all); when they are used up the
// ray misses. (A callable, not a returned flag: with the flag the STRICT instances of sol_query_kernel come out with other registers.)
template <bool STRICT, class F>
DEV void query_when_settled(const DevScene& S, const Stack& st, Trav& t, float tmax, uint32_t& left, F&& settled) {
  if (STRICT && SOL_REF_KIND(t.h.ref) != SOL_REF_NONE && !trav_accept_or_restart(S, t, st)) {
    t.h.t = tmax;  // (trav_accept_or_restart starts over with an open interval: the query's own upper end again)
    if (left != 0u) { left--; return; }
    t.cur = REF_DONE;  // (the search state holds no hit after the restart: a miss)
  }
  settled();
}
// The occlusion early-out, after each step of a lane that took it (`act`): a search that holds an accepted primitive is done - in a scene
// with needles only when that primitive is not a triangle (a triangle must pass the consistency rule first: its lane runs the bounded
// closest search to the end, and a sphere or a quad inside the interval stays a hit whatever the rule refuses).
template <bool STRICT>
DEV void query_occluded_done(Trav& t, bool act) {
  if (act) {
    const uint32_t kind = SOL_REF_KIND(t.h.ref);
    if (kind != SOL_REF_NONE && (!STRICT || kind != SOL_REF_TRIANGLE)) t.cur = REF_DONE;
  }
}

// The direction of one irradiance path (sol_irradiance), drawn from the path's own generator, which goes on from where this
// leaves it. COSINE: CosinePdf::generate (pdf.rs:58-71) about the point's normal - the two draws a Lambertian vertex makes in scatter
// (sol_shade.h); the normal need not be unit length (onb_new divides by it). SPHERE: random_unit_vector (vec3.rs:395), three draws per
// rejection round. One text for sol_radiance_kernel<.., GATHER> and sol_irradiance_rays_kernel: their bits agree because they are these operations.
DEV f3 irradiance_direction(uint32_t mode, f3 normal, Rng& rng) {
  if (mode == (uint32_t)SOL_IRRADIANCE_SPHERE) return unit3(random_in_unit_sphere(rng));
  return onb_local(onb_new(normal), random_cosine_direction(rng));
}
