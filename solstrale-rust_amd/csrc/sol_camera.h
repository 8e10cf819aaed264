// sol_camera.h -- what scene creation (sol_create.cpp) and a camera move of a live scene (sol_camera.cpp, sol_camera.hip) share:
// the cast of a camera description to the device record, and the per-camera scalars of the background-block proof - computed on the host in
// f64, read by the host proof (find_background_blocks) and passed by value to its device twin (sol_background_proof_kernel).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/solstrale_hip.h"
#include "sol_types.h"

inline DCamera cast_camera(const SolCamera& c) {
  return DCamera{(float)c.origin[0], (float)c.origin[1], (float)c.origin[2],
                 (float)c.lower_left_corner[0], (float)c.lower_left_corner[1], (float)c.lower_left_corner[2],
                 (float)c.horizontal[0], (float)c.horizontal[1], (float)c.horizontal[2],
                 (float)c.vertical[0], (float)c.vertical[1], (float)c.vertical[2],
                 (float)c.u[0], (float)c.u[1], (float)c.u[2], (float)c.v[0], (float)c.v[1], (float)c.v[2],
                 (float)c.lens_radius};
}

// The proof's view of one camera (the comment at find_background_blocks, sol_create.cpp, has the argument). lens: corners of the square
// around the lens disc (one point, the eye, for a pinhole: n_lens = 1), lens_wide: of the larger square the candidate planes are built from.
struct SolProofCamera {
  double org[3], ll[3], hh[3], vv[3];
  double lens[4][3], lens_wide[4][3];
  double norm_max, rounding_px, grow;  // fp32 rounding of generate_path in focal-plane pixels; grow = 1 + rounding_px pixels of margin
  double margin;                       // every child box is widened by this much (64 box pads)
  int n_lens;
  uint32_t width, height, bx_n, by_n;
};
// false: the proof is not attempted for this camera (a frame below 2x2, a lens radius that is negative or not finite, a rounding bound of
// three pixels or more) and no block is a background block.
inline bool sol_proof_camera(const DCamera& cam, uint32_t width, uint32_t height, double margin, SolProofCamera& p) {
  p.width = width; p.height = height; p.margin = margin;
  p.bx_n = (width + SOL_TILE - 1) / SOL_TILE; p.by_n = (height + SOL_TILE - 1) / SOL_TILE;
  if (width < 2 || height < 2 || !(cam.lens_radius >= 0.0f) || !std::isfinite(cam.lens_radius)) return false;
  const double org[3] = {cam.ox, cam.oy, cam.oz}, ll[3] = {cam.llx, cam.lly, cam.llz}, hh[3] = {cam.hx, cam.hy, cam.hz}, vv[3] = {cam.vx, cam.vy, cam.vz};
  const double lu[3] = {cam.ux, cam.uy, cam.uz}, lw[3] = {cam.wx, cam.wy, cam.wz};
  for (int a = 0; a < 3; ++a) { p.org[a] = org[a]; p.ll[a] = ll[a]; p.hh[a] = hh[a]; p.vv[a] = vv[a]; }
  p.n_lens = cam.lens_radius > 0.0f ? 4 : 1;
  for (int k = 0; k < 4; ++k) {
    const double sx = (k == 0 || k == 3) ? -1. : 1., sy = k < 2 ? -1. : 1., r = (double)cam.lens_radius * 1.0001, rw = (double)cam.lens_radius * 1.05;
    for (int a = 0; a < 3; ++a) {
      p.lens[k][a] = org[a] + (lu[a] * sx + lw[a] * sy) * r;
      p.lens_wide[k][a] = org[a] + (lu[a] * sx + lw[a] * sy) * rw;
    }
  }
  // generate_path forms T and the direction T - L in fp32: each component errs by a few ulps of the largest term. In pixels of the
  // focal plane that is 10^-4 for an ordinary camera; a camera a million units from the origin with a narrow field of view is another
  // matter - the margin grows with it, and beyond three pixels the proof is not attempted.
  auto amax = [](const double v[3]) { return std::max(std::fabs(v[0]), std::max(std::fabs(v[1]), std::fabs(v[2]))); };
  auto dot = [](const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
  p.norm_max = std::max(amax(ll) + amax(hh) + amax(vv), amax(org)) + (double)cam.lens_radius * 2.;
  const double pixel = std::min(std::sqrt(dot(hh, hh)) / (double)(width - 1), std::sqrt(dot(vv, vv)) / (double)(height - 1));
  p.rounding_px = pixel > 0. ? 8.0 * 1.1920929e-7 * p.norm_max / pixel : 1e300;
  p.grow = 1.0 + p.rounding_px;
  return p.rounding_px < 3.0;
}
