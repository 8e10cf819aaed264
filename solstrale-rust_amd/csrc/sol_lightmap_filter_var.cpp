// sol_lightmap_filter_var.cpp -- sol_lightmap_filter_var (include/solstrale_hip.h): a baked atlas filtered on the device under the
// guidance of its own per-texel variance (kernels: sol_lightmap_filter_var.hip; the rule: sol_lightmap_filter_var.h). The handle supplies the
// device, the stream and the scratch - sol_lightmap_filter's: SolScene::lf_guide, and lf_planes holding the two sides' mean and variance planes
// (both calls write all they read of them first); lm_stage for the host route, laid out by SolStaged (sol_stage.h) -; the scene itself is not
// read: nothing is traced. Every refusal is decided before the device is looked for (sol_device_enter), by a function that gets the arguments and
// not the handle; the sentences other families share are sol_bake_checks.h's, their order is this file's.
#include <cmath>

#include "sol_bake_checks.h"
#include "sol_stage.h"

namespace {
int filter_var_check(bool have_scene, const char* fn, const SolLightmapFilterVarConfig* c, const void* points, const void* texels, const void* moments,
                     const void* out, const void* variance_out) {
  if (!have_scene || !c) return sol_fail(SOL_EINVAL, "%s: null %s", fn, !have_scene ? "scene" : "configuration");
  if (const int rc = sol_config_head_check(fn, "SolLightmapFilterVarConfig", *c)) return rc;
  if (const int rc = sol_atlas_check(fn, c->width, c->height)) return rc;
  if (c->iterations < 1 || c->iterations > 8) return sol_fail(SOL_EINVAL, "%s: %u iterations (1 .. 8)", fn, c->iterations);
  if (c->normal_power_log2 > 7) return sol_fail(SOL_EINVAL, "%s: normal_power_log2 %u (0 .. 7)", fn, c->normal_power_log2);
  const float sigma[3] = {c->sigma_position, c->sigma_plane, c->sigma_value};
  const char* const sigma_name[3] = {"sigma_position", "sigma_plane", "sigma_value"};
  for (int k = 0; k < 3; ++k)
    if (!(sigma[k] >= 1e-6f)) return sol_fail(SOL_EINVAL, "%s: %s %g (at least 1e-6, not NaN; +inf switches the factor off)", fn, sigma_name[k], (double)sigma[k]);
  if (!(std::isfinite(c->variance_floor) && c->variance_floor > 0.0f))
    return sol_fail(SOL_EINVAL, "%s: variance_floor %g (finite, > 0)", fn, (double)c->variance_floor);
  if (!points || !texels || !moments || !out)
    return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !points ? "point" : !texels ? "texel" : !moments ? "moments" : "output");
  if (out == moments) return sol_fail(SOL_EINVAL, "%s: out may not be moments", fn);
  if (variance_out && (variance_out == moments || variance_out == out))
    return sol_fail(SOL_EINVAL, "%s: variance_out may not be %s", fn, variance_out == moments ? "moments" : "out");
  return SOL_OK;
}

// One stream-ordered sequence: prepare, then `iterations` passes that ping-pong between the two sides; the last one writes the caller's rows.
int filter_var_launch(SolScene* s, const SolLightmapFilterVarConfig& c, const void* points, const void* texels, const void* moments, void* out, void* variance_out) {
  int rc;
  const size_t wh = (size_t)c.width * c.height;
  if ((rc = s->lf_guide.reserve(s->stream, 2 * wh)) || (rc = s->lf_planes.reserve(s->stream, 4 * wh))) return rc;
  float4* const base = s->lf_planes.get();
  float4* side_x[2] = {base, base + 2 * wh};
  float4* side_v[2] = {base + wh, base + 3 * wh};
  HIP_TRY(sol_launch_lightmap_filter_var_prepare(texels, points, moments, (uint32_t)wh, s->lf_guide.get(), side_x[0], side_v[0], out, variance_out, s->stream));
  for (uint32_t i = 0; i < c.iterations; ++i)
    HIP_TRY(sol_launch_lightmap_filter_var_pass(c, i, s->lf_staged, s->lf_guide.get(), side_x[i & 1], side_v[i & 1], side_x[(i + 1) & 1], side_v[(i + 1) & 1], out,
                                                variance_out, s->stream));
  return SOL_OK;
}

}  // namespace

extern "C" {

int sol_lightmap_filter_var_dev(SolScene* s, const SolLightmapFilterVarConfig* config, const void* points_dev, const void* texels_dev, const void* moments_dev,
                                void* out_dev, void* variance_out_dev) {
  int rc;
  if ((rc = filter_var_check(s != nullptr, "sol_lightmap_filter_var_dev", config, points_dev, texels_dev, moments_dev, out_dev, variance_out_dev)) ||
      (rc = sol_device_enter(s)))
    return rc;
  return filter_var_launch(s, *config, points_dev, texels_dev, moments_dev, out_dev, variance_out_dev);
}

int sol_lightmap_filter_var(SolScene* s, const SolLightmapFilterVarConfig* config, const SolRay* points, const SolTexel* texels, const SolMoments* moments,
                            SolRadiance* out, float* variance_out) {
  int rc;
  if ((rc = filter_var_check(s != nullptr, "sol_lightmap_filter_var", config, points, texels, moments, out, variance_out)) || (rc = sol_device_enter(s))) return rc;
  const size_t wh = (size_t)config->width * config->height;
  SolStaged st(s->stream, s->lm_stage);
  const int p = st.in(points, wh * sizeof(SolRay)), t = st.in(texels, wh * sizeof(SolTexel)), m = st.in(moments, wh * sizeof(SolMoments));
  const int o = st.out(out, wh * sizeof(SolRadiance)), v = st.out_opt(variance_out, wh * 16);  // (no variance plane asked for: none written)
  if ((rc = st.upload()) || (rc = filter_var_launch(s, *config, st[p], st[t], st[m], st[o], st[v]))) return rc;
  return st.finish();
}

}  // extern "C"
