// sol_proof.h -- the background-block proof, written ONCE for the host and the device: scene creation and the diagnostic sol_background_blocks
// (sol_create.cpp) run sol_block_is_background over a host WideLayout, a camera move of a live scene (sol_camera.hip) runs it in a
// kernel over the tree on the device. Both are compiled with -ffp-contract=off and every operation below is one IEEE operation in f64 (sqrt
// is correctly rounded on both sides), so both flag the same blocks of the same tree because they run the same lines.
//
// Background blocks (include/solstrale_hip.h, SolSceneInfo::background_blocks): the 8x8 pixel blocks of which it can be PROVED that
// every camera ray of every pixel, whatever the jitter and the lens sample, sees nothing - so that every sample is the background
// colour and none has to be generated. A ray of the block (generate_path; Camera::get_ray, src/camera.rs:77-89) leaves a point L of
// the lens - the eye, or eye + lens_radius * (x u + y w) with (x, y) in the unit disc - towards a point T of the focal plane's
// rectangle of the block's pixels. Both sets are bounded by quadrilaterals (the lens disc's square; the rectangle widened by a whole
// pixel on every side plus a bound on the fp32 rounding of generate_path, ordinarily 10^-4 of a pixel). For a plane normal n all those rays lie in the half
// space n . x <= a with a = max n . L as soon as b = max n . (T - L) <= 0, both maxima taken over the corners (n . (T - L) is linear in
// T and in L): candidate normals come from the rectangle's edges and the lens corners (and the viewing direction, for what lies behind
// the camera), built from slightly LARGER quadrilaterals so that the check b <= 0 on the real ones holds with room to spare, and a
// candidate that fails the check is simply not used. The ray set so bounded walks the DEVICE tree as the kernel decodes it, every
// child box inflated by `margin` (64 box pads: the kernel's and the oracle's fp32 slab tests err by about one); a box is passed
// only when a valid plane has the whole box on its outer side. A block whose rays reach no primitive's (leaf) box is a background
// block: for each of its rays the kernel would find every leaf box missed - the quantised leaf boxes contain the primitives' own
// padded boxes, which the reference tree of the oracle tests -, so no primitive test would run on either side.
// Conservative in every step (a block near a silhouette is traced like any other); images never depend on it.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "sol_types.h"
#include "sol_wide.h"

// The proof's view of one camera: computed on the host in f64, once per camera. lens: corners of the square around the lens disc (one point,
// the eye, for a pinhole: n_lens = 1), lens_wide: of the larger square the candidate planes are built from.
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

struct SolProofV3 { double x, y, z; };
SOL_HD inline double sol_proof_dot(const SolProofV3& a, const SolProofV3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
SOL_HD inline SolProofV3 sol_proof_cross(const SolProofV3& a, const SolProofV3& b) { return SolProofV3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
SOL_HD inline SolProofV3 sol_proof_sub(const SolProofV3& a, const SolProofV3& b) { return SolProofV3{a.x - b.x, a.y - b.y, a.z - b.z}; }
SOL_HD inline SolProofV3 sol_proof_vec(const double v[3]) { return SolProofV3{v[0], v[1], v[2]}; }
SOL_HD inline double sol_proof_max(double a, double b) { return a < b ? b : a; }  // (selects, operand for operand the same on both sides: no library call)
SOL_HD inline double sol_proof_min(double a, double b) { return b < a ? b : a; }

#define SOL_PROOF_MAX_VISITS 4096u  // a walk that visits more nodes gives up: the block is traced

// Does every camera ray of block (bx, by) provably see nothing of the tree `wides` (n_wide nodes from the root 0, exponents over emin)?
// NL: corners of the lens (1: a pinhole, the eye; 4: the square around the lens disc) - C.n_lens, as a constant: the candidate planes (5 or
// 17) live in registers on the device, the loops over them unrolled. They keep their places, candidate p valid if bit p of `valid` is set (the
// `outside` test asks whether ANY valid plane has the box on its outer side).
// The walk is depth-first, a node's inner children from the highest slot down. `stack` - anything with uint32_t& operator[](uint32_t) - has
// ONE entry per level: the node's first inner child (24 bits) and the set of its inner children still to visit (7 bits); a tree of n levels
// needs n - 1 entries. A walk that would need more than stack_cap, like one that runs into SOL_PROOF_MAX_VISITS or leaves the node array,
// ends as "reached": the block is traced, never flagged.
template <int NL, class Stack>
SOL_HD inline bool sol_block_is_background(const DWide* wides, uint32_t n_wide, uint32_t emin, const SolProofCamera& C, uint32_t bx, uint32_t by,
                                           Stack stack, uint32_t stack_cap) {
  constexpr int NP = 4 * NL + 1;
  const uint32_t width = C.width, height = C.height;
  const uint32_t x0 = bx * SOL_TILE, x1 = x0 + SOL_TILE < width ? x0 + SOL_TILE : width, y0 = by * SOL_TILE, y1 = y0 + SOL_TILE < height ? y0 + SOL_TILE : height;
  const SolProofV3 org = sol_proof_vec(C.org), ll = sol_proof_vec(C.ll), hh = sol_proof_vec(C.hh), vv = sol_proof_vec(C.vv);
  // generate_path: u = (px + r) / (W - 1), v = ((H - 1 - py) + r) / (H - 1), r in [0, 1); `grow` pixels of margin on every side
  SolProofV3 T[4], Tw[4];
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const double grow = w == 0 ? C.grow : C.grow + 1.0;
    const double u0 = ((double)x0 - grow) / (double)(width - 1), u1 = ((double)x1 + grow) / (double)(width - 1);
    const double v0 = ((double)height - (double)y1 - grow) / (double)(height - 1), v1 = ((double)height - (double)y0 + grow) / (double)(height - 1);
    const double cu[4] = {u0, u1, u1, u0}, cv[4] = {v0, v0, v1, v1};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const SolProofV3 t{ll.x + hh.x * cu[k] + vv.x * cv[k], ll.y + hh.y * cu[k] + vv.y * cv[k], ll.z + hh.z * cu[k] + vv.z * cv[k]};
      if (w == 0) T[k] = t; else Tw[k] = t;
    }
  }
  SolProofV3 pn[NP];
  double pa[NP];
  uint32_t valid = 0;
  // keeps the candidate n (pointing AWAY from the rays) if every ray of the block provably stays in n . x <= a
  auto offer = [&](int p, SolProofV3 n) {
    pn[p] = n; pa[p] = 0.;
    const double len = sqrt(sol_proof_dot(n, n));
    if (!(len > 0.) || !(len < __builtin_huge_val())) return;
    double a = -1e300, b = -1e300;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const SolProofV3 Lj = sol_proof_vec(C.lens[j]);
      a = sol_proof_max(a, sol_proof_dot(n, Lj));
#pragma unroll
      for (int k = 0; k < 4; ++k) b = sol_proof_max(b, sol_proof_dot(n, sol_proof_sub(T[k], Lj)));
    }
    if (b <= 0.) { pa[p] = a; valid |= 1u << p; }
  };
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const SolProofV3 Lj = NL == 1 ? org : sol_proof_vec(C.lens_wide[j]);
      SolProofV3 n = sol_proof_cross(sol_proof_sub(Tw[(k + 1) & 3], Tw[k]), sol_proof_sub(Tw[k], Lj));
      if (sol_proof_dot(n, sol_proof_sub(Tw[(k + 2) & 3], Lj)) > 0.) n = SolProofV3{-n.x, -n.y, -n.z};  // the rectangle's far side is inside
      offer(k * NL + j, n);
    }
  {
    const SolProofV3 c{T[0].x + T[1].x + T[2].x + T[3].x - 4. * org.x, T[0].y + T[1].y + T[2].y + T[3].y - 4. * org.y, T[0].z + T[1].z + T[2].z + T[3].z - 4. * org.z};
    offer(NP - 1, SolProofV3{-c.x, -c.y, -c.z});  // what lies behind the camera
  }
  if (valid == 0) return false;
  const double margin = C.margin;
  uint32_t visits = 0, sp = 0, ni = 0;
  for (;;) {
    if (ni >= n_wide || ++visits > SOL_PROOF_MAX_VISITS) return false;
    const DWide w = wides[ni];
    const float origin[3] = {w.ox, w.oy, w.oz};
    const uint32_t imask = sol_wide_imask(w.meta), lmask = sol_wide_lmask(w.meta);
    float scale[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) scale[a] = sol_wide_scale(w.meta, a, emin);
    bool reached = false;
    uint32_t pending = 0;  // bit r: the r-th inner child (node base_inner + r) is to be visited
#pragma unroll
    for (int sl = 0; sl < SOL_WIDE_CHILDREN; ++sl) {
      if (reached || !(((imask | lmask) >> sl) & 1u)) continue;
      double lo[3], hi[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        lo[a] = (double)sol_wide_decode(origin[a], sol_wide_lo_byte(w.q, a, sl), scale[a]) - margin;
        hi[a] = (double)sol_wide_decode(origin[a], sol_wide_hi_byte(w.q, a, sl), scale[a]) + margin;
      }
      if (!(lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2])) { reached = true; continue; }  // (not a box: trace)
      // the least value of n . p over the box: > a = the whole box on the outer side of a valid plane
      bool outside = false;
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const double m = sol_proof_min(pn[p].x * lo[0], pn[p].x * hi[0]) + sol_proof_min(pn[p].y * lo[1], pn[p].y * hi[1]) + sol_proof_min(pn[p].z * lo[2], pn[p].z * hi[2]);
        outside = outside || (((valid >> p) & 1u) && m > pa[p]);
      }
      if (outside) continue;
      if ((lmask >> sl) & 1u) { reached = true; continue; }
      pending |= 1u << sol_wide_rank(imask, sl);
    }
    if (reached) return false;
    if (pending) {
      if (sp >= stack_cap) return false;
      stack[sp] = sol_wide_base_inner(w.q) | (pending << 24);
      ++sp;
    }
    if (sp == 0) return true;
    const uint32_t e = stack[sp - 1];
    const uint32_t r = 31u - (uint32_t)__builtin_clz(e >> 24);  // the highest slot first (an entry on the stack has a child left: e >> 24 != 0)
    ni = (e & 0x00FFFFFFu) + r;
    const uint32_t rest = e & ~(1u << (24 + r));
    if (rest >> 24) stack[sp - 1] = rest; else --sp;
  }
}
