// sol_lightmap_sh.h -- the rule of the directional lightmap (sol_lightmap_sh, sol_lightmap_normals, include/solstrale_hip.h),
// operation by operation. The kernels of sol_lightmap_sh.hip only fetch, exchange, call this text and store. Compiled with -ffp-contract=off:
// every expression is the plain fp32 sequence it spells, `/` and sqrtf are correctly rounded, so that tests/lightmap_sh_ref.py can restate the
// rule in numpy float32 and compare the words. Every clamp is a comparison; finiteness is the exponent field (lf_finite).
//
//   lookup        sol_lightmap_sample's, word for word, with channels = 27: row validity, atlas coordinates, taps, coverage, chart guard and
//                 nearest mode are sol_lightmap_sample.h's functions, called, not restated. A tap is live only when its 27 value words are
//                 finite; word 27 of a row (SolSh9::samples) is never read for a value and never judged. L[w] = sum / wsum with
//                 sum = ((0 + (w_a * x_a)) + (w_b * x_b)) .. over the live taps in tap order (lsh_word); nearest: the one tap's words.
//   evaluation    n = the row's normal as it comes, not normalised; Y_k(n) = sh9_basis (sol_sh.h); B_k = A_k * Y_k, one product, A the fp32
//                 roundings of pi (k = 0), 2 pi / 3 (k = 1..3), pi / 4 (k = 4..8) (lsh_lobe); t_k = B_k * L[3k + ch];
//                 E = ((0 + t_0) + t_1) .. + t_8 in k order; E = E * scale; with the clamp E = E > 0 ? E : 0 (lsh_finish): NaN becomes 0.
//   bad normals   a word of n that is not finite, or ((n.x * n.x) + (n.y * n.y)) + (n.z * n.z) not a finite, non-zero, non-subnormal number
//                 (lm_normal of sol_lightmap.h): four zero words (lsh_normal_ok).
//   normals       sol_lightmap_normals follows lm_row of sol_lightmap.h: b0 = (1 - b1) - b2; g = cross3(v1 - v0, v2 - v0); with vertex normals
//                 m = ((n0 * b0) + (n1 * b1)) + (n2 * b2) replaces g when lm_normal(len2(m)); zeros unless lm_normal(len2(.)) of the vector
//                 that would be normalised; then unit3 (lsh_surface_normal).
#pragma once
#include "sol_lightmap.h"
#include "sol_lightmap_sample.h"
#include "sol_sh.h"

#define SOL_LSH_CHANNELS 27u
#define SOL_LSH_A0 3.14159274f   // fl(pi)
#define SOL_LSH_A1 2.09439516f   // fl(2 pi / 3)
#define SOL_LSH_A2 0.785398185f  // fl(pi / 4)

// one interpolated coefficient: x[k] the word of tap k, w[k] its weight, over the taps of `live` in tap order
DEV float lsh_word(uint32_t live, const float (&w)[4], float x0, float x1, float x2, float x3, float wsum) {
  float sum = 0.0f;
  if (live & 1u) sum = sum + (w[0] * x0);
  if (live & 2u) sum = sum + (w[1] * x1);
  if (live & 4u) sum = sum + (w[2] * x2);
  if (live & 8u) sum = sum + (w[3] * x3);
  return sum / wsum;
}

DEV bool lsh_normal_ok(float nx, float ny, float nz) {
  if (!(lf_finite(nx) && lf_finite(ny) && lf_finite(nz))) return false;
  return lm_normal(lf_dot(nx, ny, nz, nx, ny, nz));
}

// B_k = A_l(k) * Y_k(n): the cosine lobe's zonal factor times the basis, one product each
DEV void lsh_lobe(float nx, float ny, float nz, float (&B)[9]) {
  float Y[9];
  sh9_basis(mk3(nx, ny, nz), Y);
  B[0] = SOL_LSH_A0 * Y[0];
#pragma unroll
  for (int k = 1; k < 4; ++k) B[k] = SOL_LSH_A1 * Y[k];
#pragma unroll
  for (int k = 4; k < 9; ++k) B[k] = SOL_LSH_A2 * Y[k];
}

// the nine products t_k of one channel, added in k order, scaled, clamped
DEV float lsh_finish(const float (&t)[9], float scale, bool clamp) {
  float E = 0.0f;
#pragma unroll
  for (int k = 0; k < 9; ++k) E = E + t[k];
  E = E * scale;
  if (clamp) E = E > 0.0f ? E : 0.0f;
  return E;
}

// ---- sol_lightmap_normals ----
// The unit normal of a surface row from the triangle's 9 position words and (or null) 9 normal words; false: there is none (zeros).
DEV bool lsh_surface_normal(const float (&pos)[9], const float* nrm, float b1, float b2, f3& out) {
  const float b0 = (1.0f - b1) - b2;
  const f3 v0 = mk3(pos[0], pos[1], pos[2]), v1 = mk3(pos[3], pos[4], pos[5]), v2 = mk3(pos[6], pos[7], pos[8]);
  f3 n = cross3(v1 - v0, v2 - v0);
  if (nrm) {
    const f3 m = ((mk3(nrm[0], nrm[1], nrm[2]) * b0) + (mk3(nrm[3], nrm[4], nrm[5]) * b1)) + (mk3(nrm[6], nrm[7], nrm[8]) * b2);
    if (lm_normal(len2(m))) n = m;
  }
  if (!lm_normal(len2(n))) return false;
  out = unit3(n);
  return true;
}
