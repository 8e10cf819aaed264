// sol_volume.h -- the rule of the irradiance volume (sol_volume_points, sol_volume_build, sol_volume_sample; include/solstrale_hip.h),
// operation by operation. The three kernels of sol_volume.hip call this one text. Compiled with -ffp-contract=off: every expression is the plain
// fp32 sequence it spells, `/` and sqrtf are correctly rounded (sol_math.h), so that tests/volume_ref.py can restate the rule in numpy float32
// and compare the words. dot3 / len2 (sol_math.h) are ((x * x) + (y * y)) + (z * z); vol_pos(x) is x > 0 ? x : 0 - a NaN and -0 give +0.
//
//   grid      probe (i, j, k) is row (k * ny + j) * nx + i; its position per axis is o + ((float)i * s), and o itself on an axis with one probe
//             (s is not read there). vol_probe_position is what the points kernel writes and what the sampler measures distances from.
//   build     invalid (32 zero words): sh.samples == 0 or one of the 27 sums not finite. Else e[k][c] = ((c[k][c] * K4PI) / (float)samples) * A[l(k)],
//             the SPHERE estimator of sol_irradiance_sh with the cosine lobe folded in; flags bit 0. Moments (flags bit 1) with a visibility row
//             whose samples != 0 and whose t_sum, t2_sum are finite, and a finite radius > 0:
//               mean  = (t_sum  + ((float)open * radius)) / (float)samples
//               mean2 = (t2_sum + (((float)open * radius) * radius)) / (float)samples
//   sample    invalid row (four zero words): one of the six position or normal words not finite, or N.N not a finite, normal number.
//             n = N / sqrtf(N.N); q = p + (n * normal_bias) per component; Y = sh9_basis(n) (sol_sh.h).
//             per axis: count == 1: g = 0; else g = (q - o) / s, g = g > 0 ? g : 0, g = g < (float)(count - 1) ? g : (float)(count - 1);
//                       i0 = min((int)floorf(g), max(count - 2, 0)); f = g - (float)i0.
//             corners in the order dz, dy, dx ascending (corner c = dz * 4 + dy * 2 + dx), w_axis = d ? f : (1 - f), w = ((wx * wy) * wz):
//               w == 0: skipped, the probe is not loaded;  probe flags bit 0 clear: skipped;
//               SOL_VOLUME_BACKFACE   D = P - p; l2 = D.D; where l2 > 0: c = (D.n) / sqrtf(l2); b = (c + 1) * 0.5; w = w * ((b * b) + 0.2f)
//               SOL_VOLUME_CHEBYSHEV  where the probe has moments: D' = P - q; d = sqrtf(D'.D'); where d > mean: v = vol_pos(mean2 - (mean * mean));
//                                     t = d - mean; den = v + (t * t); where den > 0: h = v / den; w = w * ((h * h) * h)
//               !(w > 0): skipped (a NaN too);  else samples += 1;
//               E[c] = 0, then E[c] = E[c] + (e[k][c] * Y[k]) for k = 0..8, then E[c] = vol_pos(E[c]);  sum[c] = sum[c] + (w * E[c]); wsum = wsum + w
//             out = (sum[0] / wsum, sum[1] / wsum, sum[2] / wsum, samples); samples == 0 (then wsum == 0): four zero words.
#pragma once
#include "sol_math.h"
#include "sol_ray.h"
#include "sol_sh.h"

#define SOL_VOL_K4PI 12.566370614359172f  // the fp32 rounding of 4 pi
#define SOL_VOL_A0 3.141592653589793f     // pi
#define SOL_VOL_A1 2.0943951023931953f    // 2 pi / 3
#define SOL_VOL_A2 0.7853981633974483f    // pi / 4
#define SOL_VOL_VALID 1u
#define SOL_VOL_MOMENTS 2u
#define SOL_VOL_BACKFACE 1u   // SOL_VOLUME_BACKFACE
#define SOL_VOL_CHEBYSHEV 2u  // SOL_VOLUME_CHEBYSHEV

// The grid as the kernels take it (SolVolumeGrid without its size word).
struct VolGrid {
  uint32_t n[3];
  float o[3], s[3];
  uint32_t flags;
  float normal_bias;
};

DEV float vol_pos(float x) { return x > 0.0f ? x : 0.0f; }
// a finite fp32 number that is not zero and not subnormal
DEV bool vol_normal(float x) {
  const uint32_t e = __float_as_uint(x) & 0x7F800000u;
  return e != 0u && e != 0x7F800000u;
}
DEV float vol_axis_position(const VolGrid& G, int a, uint32_t i) { return G.n[a] == 1u ? G.o[a] : G.o[a] + ((float)i * G.s[a]); }
DEV f3 vol_probe_position(const VolGrid& G, uint32_t i, uint32_t j, uint32_t k) {
  return mk3(vol_axis_position(G, 0, i), vol_axis_position(G, 1, j), vol_axis_position(G, 2, k));
}
DEV float vol_zonal(int k) { return k == 0 ? SOL_VOL_A0 : k < 4 ? SOL_VOL_A1 : SOL_VOL_A2; }

// One probe from an SolSh9 row (28 words) and a SolVisibility row (8 words; eight zero words where there is none: no samples, no moments): 32 words out.
DEV void vol_build(const uint32_t* sh, const uint32_t* vis, float radius, uint32_t (&out)[32]) {
  for (int w = 0; w < 32; ++w) out[w] = 0u;
  const uint32_t samples = sh[27];
  bool ok = samples != 0u;
  for (int w = 0; w < 27; ++w) ok = ok && query_finite(__uint_as_float(sh[w]));
  if (!ok) return;
  const float fs = (float)samples;
  for (int k = 0; k < 9; ++k)
    for (int c = 0; c < 3; ++c) out[k * 3 + c] = __float_as_uint(((__uint_as_float(sh[k * 3 + c]) * SOL_VOL_K4PI) / fs) * vol_zonal(k));
  uint32_t flags = SOL_VOL_VALID;
  if (vis[7] != 0u && query_finite(__uint_as_float(vis[4])) && query_finite(__uint_as_float(vis[5])) && query_finite(radius) && radius > 0.0f) {
    const float open = (float)vis[3], vs = (float)vis[7];
    out[27] = __float_as_uint((__uint_as_float(vis[4]) + (open * radius)) / vs);
    out[28] = __float_as_uint((__uint_as_float(vis[5]) + ((open * radius) * radius)) / vs);
    flags |= SOL_VOL_MOMENTS;
  }
  out[29] = flags;
  out[30] = samples;
}

// What a sample knows of its point before it looks at a probe.
struct VolPoint {
  f3 p, n, q;
  float Y[9];
  uint32_t i0[3];
  float f[3];
};
// false: the row is invalid
DEV bool vol_setup(const VolGrid& G, sol_v4f r0, sol_v4f r1, VolPoint& P) {
  const f3 N = mk3(r1.x, r1.y, r1.z);
  if (!(query_finite(r0.x) && query_finite(r0.y) && query_finite(r0.z) && query_finite(N.x) && query_finite(N.y) && query_finite(N.z))) return false;
  const float nn = len2(N);
  if (!vol_normal(nn)) return false;
  P.p = mk3(r0.x, r0.y, r0.z);
  P.n = N / sqrtf(nn);
  P.q = P.p + (P.n * G.normal_bias);
  sh9_basis(P.n, P.Y);
  const float q[3] = {P.q.x, P.q.y, P.q.z};
  for (int a = 0; a < 3; ++a) {
    float g = 0.0f;
    if (G.n[a] != 1u) {
      const float hi = (float)(G.n[a] - 1u);
      g = (q[a] - G.o[a]) / G.s[a];
      g = g > 0.0f ? g : 0.0f;
      g = g < hi ? g : hi;
    }
    const int top = G.n[a] >= 2u ? (int)(G.n[a] - 2u) : 0;
    const int fl = (int)floorf(g);
    const int i0 = fl < top ? fl : top;
    P.i0[a] = (uint32_t)i0;
    P.f[a] = g - (float)i0;
  }
  return true;
}
// the trilinear weight of corner c = dz * 4 + dy * 2 + dx
DEV float vol_trilinear(const VolPoint& P, uint32_t c) {
  const float wx = (c & 1u) ? P.f[0] : (1.0f - P.f[0]);
  const float wy = (c & 2u) ? P.f[1] : (1.0f - P.f[1]);
  const float wz = (c & 4u) ? P.f[2] : (1.0f - P.f[2]);
  return (wx * wy) * wz;
}
// One corner whose trilinear weight `w` is not zero and whose probe words are `e` (valid or not), the probe at `at`, added to the sums.
DEV void vol_corner(const VolGrid& G, const VolPoint& P, float w, f3 at, const uint32_t (&e)[32], float (&sum)[3], float& wsum, uint32_t& samples) {
  if (!(e[29] & SOL_VOL_VALID)) return;
  if (G.flags & SOL_VOL_BACKFACE) {
    const f3 D = at - P.p;
    const float l2 = len2(D);
    if (l2 > 0.0f) {
      const float c = dot3(D, P.n) / sqrtf(l2);
      const float b = (c + 1.0f) * 0.5f;
      w = w * ((b * b) + 0.2f);
    }
  }
  if ((G.flags & SOL_VOL_CHEBYSHEV) && (e[29] & SOL_VOL_MOMENTS)) {
    const float mean = __uint_as_float(e[27]), mean2 = __uint_as_float(e[28]);
    const float d = sqrtf(len2(at - P.q));
    if (d > mean) {
      const float v = vol_pos(mean2 - (mean * mean));
      const float t = d - mean;
      const float den = v + (t * t);
      if (den > 0.0f) {
        const float h = v / den;
        w = w * ((h * h) * h);
      }
    }
  }
  if (!(w > 0.0f)) return;
  samples += 1u;
  for (int c = 0; c < 3; ++c) {
    float E = 0.0f;
    for (int k = 0; k < 9; ++k) E = E + (__uint_as_float(e[k * 3 + c]) * P.Y[k]);
    sum[c] = sum[c] + (w * vol_pos(E));
  }
  wsum = wsum + w;
}
