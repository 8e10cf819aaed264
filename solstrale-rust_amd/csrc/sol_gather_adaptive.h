// sol_gather_adaptive.h -- the stop rule of the adaptive irradiance gathers (sol_irradiance_adaptive, include/solstrale_hip.h),
// operation by operation: what sol_gather_judge_kernel (sol_gather_adaptive.hip) applies to every active row after a round. Compiled with
// -ffp-contract=off: every expression is the plain fp32 sequence it spells and `/` is correctly rounded, so that tests/irradiance_adaptive_ref.py
// can restate the rule in numpy float32 and compare the count maps. No sqrtf: the relative standard error is compared squared.
//
//   the estimators are sol_lightmap_filter_var.h's Prepare by inclusion: x = sum / N, v = pos((sum2 / N) - (x * x)) / M with N = (float)count and
//   M = (float)(count - 1u) - the variance the filter starts from is the variance the gather stopped on.
//   the associations the header leaves open are fixed here: t = threshold * max(x, floor) is one product of the chosen operand, the clamp a
//   comparison (a NaN x cannot reach it: the sums are finite); t * t is one product, formed before the comparison v <= t * t.
//   the first condition that holds names the reason: a row with a sum that is not finite is neither converged nor capped.
#pragma once
#include "sol_lightmap_filter_var.h"

enum { SOL_GA_ACTIVE = 0, SOL_GA_BROKEN = 1, SOL_GA_CAPPED = 2, SOL_GA_CONVERGED = 3 };

// One channel of condition 3: the variance of the mean against the squared tolerance.
DEV bool ga_channel_converged(float sum, float sum2, float N, float M, float threshold, float floor) {
  const float x = lfv_mean(sum, N);
  const float v = lfv_variance(sum2, x, N, M);
  const float t = threshold * (x > floor ? x : floor);
  return v <= t * t;
}

// What becomes of a valid active row that holds `count` samples (>= 1) after a round.
DEV uint32_t ga_judge(uint32_t count, uint32_t max_samples, uint32_t min_samples, float threshold, float floor, float s0, float s1, float s2, float q0, float q1,
                      float q2) {
  if (!(lf_finite(s0) && lf_finite(s1) && lf_finite(s2) && lf_finite(q0) && lf_finite(q1) && lf_finite(q2))) return SOL_GA_BROKEN;
  if (count == max_samples) return SOL_GA_CAPPED;
  if (!(threshold > 0.0f) || count < min_samples || count < 2u) return SOL_GA_ACTIVE;
  const float N = (float)count, M = (float)(count - 1u);
  const bool all = ga_channel_converged(s0, q0, N, M, threshold, floor) && ga_channel_converged(s1, q1, N, M, threshold, floor) &&
                   ga_channel_converged(s2, q2, N, M, threshold, floor);
  return all ? SOL_GA_CONVERGED : SOL_GA_ACTIVE;
}
