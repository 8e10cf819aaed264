// sol_gather.cpp -- the checks every gather family shares and the per-sample colour launches (sol_gather.h).
#include "sol_gather.h"

#include <cstddef>

static_assert(sizeof(SolIrradianceConfig) == sizeof(SolRadianceConfig) && offsetof(SolIrradianceConfig, samples) == offsetof(SolRadianceConfig, samples) &&
              offsetof(SolIrradianceConfig, first_sample) == offsetof(SolRadianceConfig, first_sample) &&
              offsetof(SolIrradianceConfig, first_draw) == offsetof(SolRadianceConfig, first_draw) && offsetof(SolIrradianceConfig, seed) == offsetof(SolRadianceConfig, seed) &&
              offsetof(SolIrradianceConfig, key_base) == offsetof(SolRadianceConfig, key_base) && offsetof(SolIrradianceConfig, mode) == offsetof(SolRadianceConfig, reserved),
              "SolIrradianceConfig is SolRadianceConfig with `mode` in the place of `reserved`");
static_assert(sizeof(SolSh9) == 7 * sizeof(SolRadiance) && sizeof(SolMoments) == 2 * sizeof(SolRadiance) && sizeof(SolVisibility) == 2 * sizeof(SolRadiance) &&
              sizeof(SolOctTexel) == sizeof(SolRadiance), "every family's answer is whole dwordx4 rows of the radiance queries' buffers");

int sol_radiance_config_check(const char* fn, SolRadianceKind kind, size_t n, const SolRadianceConfig* cfg) {
  const char* rec = kind == SOL_KIND_RADIANCE ? "SolRadianceConfig" : "SolIrradianceConfig";
  if (!cfg) return sol_fail(SOL_EINVAL, "%s: null configuration", fn);
  if (cfg->size != sizeof(SolRadianceConfig)) return sol_fail(SOL_EINVAL, "%s: %s.size is %u, not %zu", fn, rec, cfg->size, sizeof(SolRadianceConfig));
  if (kind == SOL_KIND_RADIANCE && cfg->reserved != 0u) return sol_fail(SOL_EINVAL, "%s: SolRadianceConfig.reserved must be 0", fn);
  if (cfg->samples == 0u) return sol_fail(SOL_EINVAL, "%s: %s.samples is 0", fn, rec);
  if (kind == SOL_KIND_IRRADIANCE_RAYS && cfg->samples != 1u)
    return sol_fail(SOL_EINVAL, "%s: %s.samples is %u: the rays of one sample (first_sample) per call", fn, rec, cfg->samples);
  if ((uint64_t)cfg->first_sample + cfg->samples > 0xFFFFFFF0ull) return sol_fail(SOL_EINVAL, "%s: first_sample + samples goes beyond 2^32 - 16", fn);
  if (n > SOL_GATHER_MAX_POINTS) return sol_fail(SOL_EINVAL, "%s: %zu %s in one call (at most 2^31)", fn, n, kind == SOL_KIND_RADIANCE ? "rays" : "points");
  if (kind != SOL_KIND_RADIANCE && cfg->reserved != (uint32_t)SOL_IRRADIANCE_COSINE && cfg->reserved != (uint32_t)SOL_IRRADIANCE_SPHERE)
    return sol_fail(SOL_EINVAL, "%s: unknown mode %u (SOL_IRRADIANCE_COSINE or SOL_IRRADIANCE_SPHERE)", fn, cfg->reserved);
  return SOL_OK;
}

int sol_query_mode_check(const char* fn, int mode) {
  if (mode != SOL_QUERY_CLOSEST && mode != SOL_QUERY_OCCLUDED) return sol_fail(SOL_EINVAL, "%s: unknown mode %d (SOL_QUERY_CLOSEST or SOL_QUERY_OCCLUDED)", fn, mode);
  return SOL_OK;
}

int sol_query_medium_check(const SolScene* s, const char* fn) {
  if (s->has_medium)
    return sol_fail(SOL_EINVAL, "%s: the scene has a constant medium - its hits are random draws keyed by a path, which a query ray does not have", fn);
  return SOL_OK;
}

int sol_irradiance_each_launch(SolScene* s, const void* points_dev, const void* keys_dev, size_t n, const SolRadianceConfig& cfg, uint32_t key_base, void* out_dev,
                               bool moments, bool carry, uint32_t total_samples) {
  const SolEstimator est = sol_estimator(s, s->S, false);  // what a render would run now
  const SolGatherPlan plan{sol_radiance_blocks_per_cu(true, true, s->strict_triangles, est.env, est.lt), 0u, 1u, moments ? sizeof(SolMoments) : sizeof(SolSh9), cfg.reserved};
  return sol_gather_launch(s, plan, points_dev, keys_dev, n, cfg, key_base, out_dev, [&](const SolGatherWindow& w) -> int {
    HIP_TRY(sol_launch_radiance(s->mirror.dev.get(), w.P, true, true, w.may_spill, s->strict_triangles, est.env, est.lt, w.points, w.keys, nullptr, s->rad_partial.get(),
                                s->rad_work.get(), s->rad_spill.get(), w.grid, s->stream));
    if (moments)
      HIP_TRY(sol_launch_moments_project(w.P, w.points, s->rad_partial.get(), w.out, w.samples, carry ? total_samples : cfg.samples, carry || !w.first, s->stream));
    else
      HIP_TRY(sol_launch_sh_project(w.P, w.points, w.keys, s->rad_partial.get(), w.out, w.samples, cfg.samples, !w.first, s->stream));
    return SOL_OK;
  });
}
