// sol_lightmap_filter.cpp -- sol_lightmap_filter (include/solstrale_hip.h): a baked atlas filtered on the device between the gather
// and the dilation (kernels: sol_lightmap_filter.hip; the rule: sol_lightmap_filter.h). The handle supplies the device, the stream and the scratch
// (SolScene::lf_guide, lf_planes; lm_stage for the host route, laid out by SolStaged, sol_stage.h); the scene itself is not read: nothing is
// traced. Every refusal is decided before the device is looked for (sol_device_enter), by a function that gets the arguments and not the handle;
// the sentences other families share are sol_bake_checks.h's, their order is this file's.
#include <cmath>

#include "sol_bake_checks.h"
#include "sol_stage.h"

namespace {
int filter_check(bool have_scene, const char* fn, const SolLightmapFilterConfig* c, const void* points, const void* texels, const void* values, const void* out) {
  if (!have_scene || !c) return sol_fail(SOL_EINVAL, "%s: null %s", fn, !have_scene ? "scene" : "configuration");
  if (const int rc = sol_config_head_check(fn, "SolLightmapFilterConfig", *c)) return rc;
  if (const int rc = sol_atlas_check(fn, c->width, c->height)) return rc;
  if (c->iterations < 1 || c->iterations > 8) return sol_fail(SOL_EINVAL, "%s: %u iterations (1 .. 8)", fn, c->iterations);
  if (c->normal_power_log2 > 7) return sol_fail(SOL_EINVAL, "%s: normal_power_log2 %u (0 .. 7)", fn, c->normal_power_log2);
  const float sigma[3] = {c->sigma_position, c->sigma_plane, c->sigma_value};
  const char* const sigma_name[3] = {"sigma_position", "sigma_plane", "sigma_value"};
  for (int k = 0; k < 3; ++k)
    if (!(sigma[k] >= 1e-6f)) return sol_fail(SOL_EINVAL, "%s: %s %g (at least 1e-6, not NaN; +inf switches the factor off)", fn, sigma_name[k], (double)sigma[k]);
  if (!(std::isfinite(c->value_scale) && c->value_scale > 0.0f)) return sol_fail(SOL_EINVAL, "%s: value_scale %g (finite, > 0)", fn, (double)c->value_scale);
  if (const int rc = sol_channels_check(fn, c->channels, c->stride_bytes)) return rc;
  if (!points || !texels || !values || !out)
    return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !points ? "point" : !texels ? "texel" : !values ? "value" : "output");
  if (out == values) return sol_fail(SOL_EINVAL, "%s: out may not be values", fn);
  return SOL_OK;
}

// One stream-ordered sequence: prepare, then `iterations` passes that ping-pong between the two planes; the last one writes the caller's rows.
int filter_launch(SolScene* s, const SolLightmapFilterConfig& c, const void* points, const void* texels, const void* values, void* out) {
  int rc;
  const size_t wh = (size_t)c.width * c.height, groups = (c.channels + 3u) / 4u;
  if ((rc = s->lf_guide.reserve(s->stream, 2 * wh)) || (rc = s->lf_planes.reserve(s->stream, 2 * groups * wh))) return rc;
  float4* plane[2] = {s->lf_planes.get(), s->lf_planes.get() + groups * wh};
  HIP_TRY(sol_launch_lightmap_filter_prepare(texels, points, values, (uint32_t)wh, c.channels, c.stride_bytes / 4, s->lf_guide.get(), plane[0], out, s->stream));
  for (uint32_t i = 0; i < c.iterations; ++i)
    HIP_TRY(sol_launch_lightmap_filter_pass(c, i, s->lf_staged, s->lf_fold, s->lf_guide.get(), plane[i & 1], plane[(i + 1) & 1], out, s->stream));
  return SOL_OK;
}

}  // namespace

extern "C" {

int sol_lightmap_filter_dev(SolScene* s, const SolLightmapFilterConfig* config, const void* points_dev, const void* texels_dev, const void* values_dev,
                            void* out_dev) {
  int rc;
  if ((rc = filter_check(s != nullptr, "sol_lightmap_filter_dev", config, points_dev, texels_dev, values_dev, out_dev)) || (rc = sol_device_enter(s))) return rc;
  return filter_launch(s, *config, points_dev, texels_dev, values_dev, out_dev);
}

int sol_lightmap_filter(SolScene* s, const SolLightmapFilterConfig* config, const SolRay* points, const SolTexel* texels, const void* values, void* out) {
  int rc;
  if ((rc = filter_check(s != nullptr, "sol_lightmap_filter", config, points, texels, values, out)) || (rc = sol_device_enter(s))) return rc;
  const size_t wh = (size_t)config->width * config->height, row = config->stride_bytes;
  SolStaged st(s->stream, s->lm_stage);
  const int p = st.in(points, wh * sizeof(SolRay)), t = st.in(texels, wh * sizeof(SolTexel)), v = st.in(values, wh * row), o = st.out(out, wh * row);
  if ((rc = st.upload()) || (rc = filter_launch(s, *config, st[p], st[t], st[v], st[o]))) return rc;
  return st.finish();
}

}  // extern "C"
