// sol_camera.h -- what scene creation (sol_create.cpp) and a camera move of a live scene (sol_camera.cpp, sol_camera.hip) share:
// the cast of a camera description to the device record, and (sol_proof.h) the background-block proof with its per-camera scalars.
#pragma once
#include <cstdint>

#include "../../include/solstrale_hip.h"
#include "sol_proof.h"
#include "sol_types.h"

inline DCamera cast_camera(const SolCamera& c) {
  return DCamera{(float)c.origin[0], (float)c.origin[1], (float)c.origin[2],
                 (float)c.lower_left_corner[0], (float)c.lower_left_corner[1], (float)c.lower_left_corner[2],
                 (float)c.horizontal[0], (float)c.horizontal[1], (float)c.horizontal[2],
                 (float)c.vertical[0], (float)c.vertical[1], (float)c.vertical[2],
                 (float)c.u[0], (float)c.u[1], (float)c.u[2], (float)c.v[0], (float)c.v[1], (float)c.v[2],
                 (float)c.lens_radius};
}
