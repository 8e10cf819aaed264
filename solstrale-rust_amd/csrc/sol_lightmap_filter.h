// sol_lightmap_filter.h -- the rule of the lightmap filter (sol_lightmap_filter, include/solstrale_hip.h), operation by operation.
// Both pass shapes of sol_lightmap_filter.hip - taps from global memory, taps from a tile staged in LDS - call this one text, so that they answer
// the same words. Compiled with -ffp-contract=off: every expression is the plain fp32 sequence it spells and `/` is correctly rounded, so that
// tests/lightmap_filter_ref.py can restate the rule in numpy float32 and compare the words. No expf, no powf, no fmaxf: every clamp is a comparison.
//
//   live      triangle != SOL_TEXEL_NONE, the six position and normal words finite, the `channels` value words finite (lf_finite: the exponent
//             field is not all ones).
//   tap order dj outer, di inner, both from -2 to 2; k = lf_h(di) * lf_h(dj), exact.
//   the associations the header leaves open are fixed here: s * s, sp * sp and sv * sv are one product each of the rounded s = sigma_position * f,
//   sp = sigma_plane * f, sv = sigma_value / f (lf_pass_of); d * d and dv * dv are formed before the division / the addition; 1 + x is 1.0f + x.
#pragma once
#include "sol_math.h"

#define SOL_LF_TEXEL_NONE 0xFFFFFFFFu

DEV bool lf_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
DEV float lf_pos(float x) { return x > 0.0f ? x : 0.0f; }
DEV float lf_dot(float ax, float ay, float az, float bx, float by, float bz) { return ((ax * bx) + (ay * by)) + (az * bz); }
// h[d + 2] of the B3 spline (1/16, 1/4, 3/8, 1/4, 1/16)
DEV float lf_h(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

// What a pass derives from the configuration: the squared widths of its three factors.
struct LfPass {
  float ss, sps, svs;    // (sigma_position * f)^2, (sigma_plane * f)^2, (sigma_value / f)^2
  float value_scale;
  uint32_t normal_power_log2, m;  // m = min(channels, 3)
};
DEV LfPass lf_pass_of(float sigma_position, float sigma_plane, float sigma_value, float value_scale, uint32_t normal_power_log2, uint32_t channels,
                      uint32_t step) {
  const float f = (float)step;
  const float s = sigma_position * f, sp = sigma_plane * f, sv = sigma_value / f;
  return LfPass{s * s, sp * sp, sv * sv, value_scale, normal_power_log2, channels < 3u ? channels : 3u};
}

// a / (1 + a) of a value: where the value factor compares two texels
DEV float lf_tone(float x, float value_scale) {
  const float a = lf_pos(x * value_scale);
  return a / (1.0f + a);
}

// The weight of a tap q that is not the centre p. P, N: the stored position and normal; tp: the centre's three toned values (lf_tone of x_p[0..2],
// of which the first c.m are read); xq: the tap's first three values of the pass's input.
DEV float lf_weight(float k, float ppx, float ppy, float ppz, float npx, float npy, float npz, float pqx, float pqy, float pqz, float nqx, float nqy,
                    float nqz, float tp0, float tp1, float tp2, float xq0, float xq1, float xq2, const LfPass& c) {
  const float ex = pqx - ppx, ey = pqy - ppy, ez = pqz - ppz;
  const float l2 = lf_dot(ex, ey, ez, ex, ey, ez);
  const float w_d = 1.0f / (1.0f + (l2 / c.ss));
  const float d = lf_dot(npx, npy, npz, ex, ey, ez);
  const float w_pl = 1.0f / (1.0f + ((d * d) / c.sps));
  float cn = lf_pos(lf_dot(npx, npy, npz, nqx, nqy, nqz));
  for (uint32_t r = 0; r < c.normal_power_log2; ++r) cn = cn * cn;
  float D = 0.0f;
  {
    const float dv = tp0 - lf_tone(xq0, c.value_scale);
    D = D + (dv * dv);
  }
  if (c.m > 1u) {
    const float dv = tp1 - lf_tone(xq1, c.value_scale);
    D = D + (dv * dv);
  }
  if (c.m > 2u) {
    const float dv = tp2 - lf_tone(xq2, c.value_scale);
    D = D + (dv * dv);
  }
  float w_v = 1.0f / (1.0f + (D / c.svs));
  w_v = w_v * w_v;
  return (((k * w_d) * w_pl) * cn) * w_v;
}
