// sol_depth.cpp -- sol_visibility_oct, sol_volume_build_depth and sol_volume_sample_depth (include/solstrale_hip.h): the directional
// distance moments of an irradiance volume (kernels: sol_depth.hip; the rule: sol_depth.h). The gather is a visibility gather: it shares the
// radiance queries' scratch and staging (SolScene::rad_*) and their launch plan; build and sample trace nothing and stage through
// SolScene::vol_stage (SolStaged, sol_stage.h). Every refusal is decided before the device is looked for.
#include <algorithm>
#include <cmath>

#include "sol_bake_checks.h"
#include "sol_gather.h"
#include "sol_stage.h"

namespace {
constexpr size_t DEPTH_STAGE_TEXELS = (size_t)1 << 24;  // the gather's host route stages at most this many SolOctTexel rows at a time (256 MiB)

int oct_config_check(const char* fn, const SolOctConfig* c) {
  if (!c) return sol_fail(SOL_EINVAL, "%s: null SolOctConfig", fn);
  if (c->size != sizeof(SolOctConfig)) return sol_fail(SOL_EINVAL, "%s: SolOctConfig.size is %u, not %zu", fn, c->size, sizeof(SolOctConfig));
  if (c->res != 4u && c->res != 8u && c->res != 16u) return sol_fail(SOL_EINVAL, "%s: SolOctConfig.res is %u (4, 8 or 16)", fn, c->res);
  if (c->sharpness_log2 > 6u) return sol_fail(SOL_EINVAL, "%s: SolOctConfig.sharpness_log2 is %u (0 to 6)", fn, c->sharpness_log2);
  if (c->reserved != 0u) return sol_fail(SOL_EINVAL, "%s: SolOctConfig.reserved must be 0", fn);
  return SOL_OK;
}
// sol_visibility's order with the SolOctConfig directly after the SolIrradianceConfig. *go = false: nothing to do (n == 0).
int gather_check(const SolScene* s, const char* fn, const void* points, size_t n, const SolRadianceConfig* cfg, const SolOctConfig* oct, const void* out, bool* go) {
  *go = false;
  if (!s) return sol_fail(SOL_EINVAL, "%s: null scene", fn);
  if (const int rc = sol_radiance_config_check(fn, SOL_KIND_IRRADIANCE, n, cfg)) return rc;
  if (const int rc = oct_config_check(fn, oct)) return rc;
  if (n == 0) return SOL_OK;
  if (const int rc = sol_query_medium_check(s, fn)) return rc;
  if (!points || !out) return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !points ? "point" : "output");
  *go = true;
  return SOL_OK;
}
int build_check(bool have_scene, const char* fn, const SolVolumeGrid* g, const void* oct, const SolOctConfig* c, float radius, const void* out) {
  if (const int rc = sol_volume_grid_check(have_scene, fn, g)) return rc;
  if (const int rc = oct_config_check(fn, c)) return rc;
  if (!(std::isfinite(radius) && radius > 0.0f)) return sol_fail(SOL_EINVAL, "%s: radius %g (finite and > 0)", fn, (double)radius);
  if (!oct || !out) return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !oct ? "SolOctTexel" : "output");
  return SOL_OK;
}
int sample_check(bool have_scene, const char* fn, const SolVolumeGrid* g, const void* probes, const void* depth, const SolOctConfig* c, const void* points, size_t n,
                 const void* out) {
  if (const int rc = sol_volume_grid_check(have_scene, fn, g)) return rc;
  if (const int rc = oct_config_check(fn, c)) return rc;
  if (const int rc = sol_rows_check(fn, n, "points")) return rc;
  if (n > 0 && (!probes || !depth || !points || !out))
    return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !probes ? "probe" : !depth ? "depth" : !points ? "point" : "output");
  return SOL_OK;
}
size_t probes_of(const SolVolumeGrid& g) { return (size_t)g.nx * g.ny * g.nz; }

// n <= 2^31 points (and keys, or null) in device memory, n * res * res SolOctTexel out: per sample, one word each - four to a row of the partial buffer.
int gather_launch(SolScene* s, const void* points_dev, const void* keys_dev, size_t n, const SolRadianceConfig& cfg, uint32_t key_base, const SolOctConfig& oct,
                  void* out_dev) {
  const SolGatherPlan plan{sol_depth_each_blocks_per_cu(s->strict_triangles), 0u, 4u, (size_t)oct.res * oct.res * sizeof(SolOctTexel), cfg.reserved};
  return sol_gather_launch(s, plan, points_dev, keys_dev, n, cfg, key_base, out_dev, [&](const SolGatherWindow& w) -> int {
    HIP_TRY(sol_launch_depth_each(s->mirror.dev.get(), w.P, w.may_spill, s->strict_triangles, w.points, w.keys, s->rad_partial.get(), s->rad_work.get(),
                                  s->rad_spill.get(), w.grid, s->stream));
    HIP_TRY(sol_launch_depth_project(w.P, s->depth_project_plain, oct.res, oct.sharpness_log2, w.points, w.keys, s->rad_partial.get(), w.out, w.samples, !w.first,
                                     s->stream));
    return SOL_OK;
  });
}

int build_launch(SolScene* s, size_t n_texels, const void* oct, float radius, void* depth) {
  HIP_TRY(sol_launch_depth_build((uint64_t)n_texels, oct, radius, depth, s->stream));
  return SOL_OK;
}
int sample_launch(SolScene* s, const SolVolumeGrid& g, const void* probes, const void* depth, uint32_t res, const void* points, size_t n, void* out) {
  HIP_TRY(sol_launch_volume_sample_depth(g, probes, depth, res, points, (uint32_t)n, out, s->stream));
  return SOL_OK;
}
}  // namespace

extern "C" {

int sol_visibility_oct_dev(SolScene* s, const void* points_dev, const void* keys_dev, size_t n, const SolIrradianceConfig* config, const SolOctConfig* oct,
                           void* out_dev) {
  return sol_gather_entry(
      s, config, [&](const SolRadianceConfig* c, bool* go) { return gather_check(s, "sol_visibility_oct_dev", points_dev, n, c, oct, out_dev, go); },
      [&](const SolRadianceConfig& cfg) { return gather_launch(s, points_dev, keys_dev, n, cfg, cfg.key_base, *oct, out_dev); });
}

int sol_visibility_oct(SolScene* s, const SolRay* points, const SolRayKey* keys, size_t n, const SolIrradianceConfig* config, const SolOctConfig* oct,
                       SolOctTexel* out) {
  return sol_gather_entry(
      s, config, [&](const SolRadianceConfig* c, bool* go) { return gather_check(s, "sol_visibility_oct", points, n, c, oct, out, go); },
      [&](const SolRadianceConfig& cfg) {
        const size_t texels = (size_t)oct->res * oct->res;  // (the answers' staging holds the res x res rows of a point's map)
        return sol_gather_stage(s, points, keys, n, std::max<size_t>(1, DEPTH_STAGE_TEXELS / texels), out, texels * sizeof(SolOctTexel), cfg.key_base,
                                [&](const void* p, const void* k, size_t m, uint32_t key_base, void* o) { return gather_launch(s, p, k, m, cfg, key_base, *oct, o); });
      });
}

int sol_volume_build_depth_dev(SolScene* s, const SolVolumeGrid* grid, const void* oct_dev, const SolOctConfig* oct, float radius, void* depth_out_dev) {
  int rc;
  if ((rc = build_check(s != nullptr, "sol_volume_build_depth_dev", grid, oct_dev, oct, radius, depth_out_dev)) || (rc = sol_device_enter(s))) return rc;
  return build_launch(s, probes_of(*grid) * oct->res * oct->res, oct_dev, radius, depth_out_dev);
}

int sol_volume_build_depth(SolScene* s, const SolVolumeGrid* grid, const SolOctTexel* oct_rows, const SolOctConfig* oct, float radius, SolDepthTexel* depth_out) {
  int rc;
  if ((rc = build_check(s != nullptr, "sol_volume_build_depth", grid, oct_rows, oct, radius, depth_out)) || (rc = sol_device_enter(s))) return rc;
  const size_t n = probes_of(*grid) * oct->res * oct->res;
  SolStaged st(s->stream, s->vol_stage);
  const int oc = st.in(oct_rows, n * sizeof(SolOctTexel)), o = st.out(depth_out, n * sizeof(SolDepthTexel));
  if ((rc = st.upload()) || (rc = build_launch(s, n, st[oc], radius, st[o]))) return rc;
  return st.finish();
}

int sol_volume_sample_depth_dev(SolScene* s, const SolVolumeGrid* grid, const void* probes_dev, const void* depth_dev, const SolOctConfig* oct, const void* points_dev,
                                size_t n, void* out_dev) {
  int rc;
  if ((rc = sample_check(s != nullptr, "sol_volume_sample_depth_dev", grid, probes_dev, depth_dev, oct, points_dev, n, out_dev)) || n == 0 ||
      (rc = sol_device_enter(s)))
    return rc;
  return sample_launch(s, *grid, probes_dev, depth_dev, oct->res, points_dev, n, out_dev);
}

int sol_volume_sample_depth(SolScene* s, const SolVolumeGrid* grid, const SolProbe* probes, const SolDepthTexel* depth, const SolOctConfig* oct, const SolRay* points,
                            size_t n, SolRadiance* out) {
  int rc;
  if ((rc = sample_check(s != nullptr, "sol_volume_sample_depth", grid, probes, depth, oct, points, n, out)) || n == 0 || (rc = sol_device_enter(s))) return rc;
  const size_t np = probes_of(*grid), nt = np * oct->res * oct->res;
  SolStaged st(s->stream, s->vol_stage);
  const int pr = st.in(probes, np * sizeof(SolProbe)), d = st.in(depth, nt * sizeof(SolDepthTexel)), p = st.in(points, n * sizeof(SolRay));
  const int o = st.out(out, n * sizeof(SolRadiance));
  if ((rc = st.upload()) || (rc = sample_launch(s, *grid, st[pr], st[d], oct->res, st[p], n, st[o]))) return rc;
  return st.finish();
}

}  // extern "C"
