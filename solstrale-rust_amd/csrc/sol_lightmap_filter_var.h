// sol_lightmap_filter_var.h -- the rule of the variance-guided lightmap filter (sol_lightmap_filter_var, include/solstrale_hip.h),
// operation by operation. Both pass shapes of sol_lightmap_filter_var.hip call this one text, so that they answer the same words. Compiled with
// -ffp-contract=off: every expression is the plain fp32 sequence it spells and `/` is correctly rounded, so that tests/lightmap_filter_var_ref.py
// can restate the rule in numpy float32 and compare the words. No expf, no powf, no sqrtf, no fmaxf: every clamp is a comparison.
//
//   live      triangle != SOL_TEXEL_NONE, the six position and normal words finite, samples >= 2, the six sums finite (lf_finite).
//   taps      k, E, w_d, w_pl and c are sol_lightmap_filter.h's, by inclusion: lfv_geometry calls lf_weight with a value factor that is switched
//             off - two equal values give D = 0 and w_v = 1 / (1 + (0 / 1)) = 1, both at compile time -, so that what it returns is
//             (((k * w_d) * w_pl) * c) * 1 on the bits; (sigma_position * f)^2 and (sigma_plane * f)^2 are lf_pass_of's.
//   the associations the header leaves open are fixed here: N and M are the conversions (float)samples and (float)(samples - 1u); x * x is formed
//   before the subtraction; sigma_value * sigma_value is one product, formed before the product with V; wsum * wsum and w * w are one product each,
//   formed before the division / the product with v_q; 1 + x is 1.0f + x; the three quotients vb[j] / gs are formed before they are added.
#pragma once
#include "sol_lightmap_filter.h"

// h3[d + 1] of the prefilter (1/4, 1/2, 1/4)
DEV float lfv_h3(int d) { return d == 0 ? 0.5f : 0.25f; }

// Prepare: the mean and the variance of the mean of one channel from its two sums.
DEV float lfv_mean(float sum, float N) { return sum / N; }
DEV float lfv_variance(float sum2, float x, float N, float M) { return lf_pos((sum2 / N) - (x * x)) / M; }

// What a pass derives from the configuration.
struct LfvPass {
  LfPass geometry;  // ss, sps and the normal power; its value factor is off
  float svs;        // sigma_value^2
  float variance_floor;
};
DEV LfvPass lfv_pass_of(float sigma_position, float sigma_plane, float sigma_value, float variance_floor, uint32_t normal_power_log2, uint32_t step) {
  const LfPass g = lf_pass_of(sigma_position, sigma_plane, 1.0f, 1.0f, normal_power_log2, 1u, step);
  return LfvPass{LfPass{g.ss, g.sps, 1.0f, 1.0f, normal_power_log2, 1u}, sigma_value * sigma_value, variance_floor};
}

// One tap of the variance prefilter
DEV void lfv_prefilter_add(float g, float v0, float v1, float v2, float& vb0, float& vb1, float& vb2, float& gs) {
  vb0 = vb0 + (g * v0);
  vb1 = vb1 + (g * v1);
  vb2 = vb2 + (g * v2);
  gs = gs + g;
}
// den of the value factor from the prefilter's sums
DEV float lfv_den(float vb0, float vb1, float vb2, float gs, const LfvPass& c) {
  const float V = (((vb0 / gs) + (vb1 / gs)) + (vb2 / gs)) + c.variance_floor;
  return c.svs * V;
}

// ((k * w_d) * w_pl) * c of a tap q that is not the centre p
DEV float lfv_geometry(float k, float ppx, float ppy, float ppz, float npx, float npy, float npz, float pqx, float pqy, float pqz, float nqx, float nqy,
                       float nqz, const LfvPass& c) {
  return lf_weight(k, ppx, ppy, ppz, npx, npy, npz, pqx, pqy, pqz, nqx, nqy, nqz, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, c.geometry);
}

// The weight of a tap that is not the centre: its geometry factors times the value factor of the two means under the centre's `den`.
DEV float lfv_weight(float geometry, float xp0, float xp1, float xp2, float xq0, float xq1, float xq2, float den) {
  float D = 0.0f;
  {
    const float dv = xp0 - xq0;
    D = D + (dv * dv);
  }
  {
    const float dv = xp1 - xq1;
    D = D + (dv * dv);
  }
  {
    const float dv = xp2 - xq2;
    D = D + (dv * dv);
  }
  float w_v = 1.0f / (1.0f + (D / den));
  w_v = w_v * w_v;
  return geometry * w_v;
}
