// sol_ray.h -- what the kernels that take the caller's own rays share (sol_query.hip, sol_radiance.hip): the validity rule of a SolRay
// (include/solstrale_hip.h), decided per ray by the kernel itself before any search.
#pragma once
#include "sol_math.h"

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
