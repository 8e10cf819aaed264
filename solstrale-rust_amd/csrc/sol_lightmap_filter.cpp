// sol_lightmap_filter.cpp -- sol_lightmap_filter (include/solstrale_hip.h): a baked atlas filtered on the device between the gather
// and the dilation (kernels: sol_lightmap_filter.hip; the rule: sol_lightmap_filter.h). The handle supplies the device, the stream and the scratch
// (SolScene::lf_guide, lf_planes; lm_stage for the host route); the scene itself is not read: nothing is traced. Every refusal is decided before the
// device is looked for, by a function that gets the arguments and not the handle.
#include <cmath>

#include "sol_scene.h"

namespace {
int filter_check(bool have_scene, const char* fn, const SolLightmapFilterConfig* c, const void* points, const void* texels, const void* values, const void* out) {
  if (!have_scene || !c) return sol_fail(SOL_EINVAL, "%s: null %s", fn, !have_scene ? "scene" : "configuration");
  if (c->size != sizeof(SolLightmapFilterConfig))
    return sol_fail(SOL_EINVAL, "%s: SolLightmapFilterConfig.size %u (expected %zu)", fn, c->size, sizeof(SolLightmapFilterConfig));
  for (uint32_t r : c->reserved)
    if (r) return sol_fail(SOL_EINVAL, "%s: SolLightmapFilterConfig.reserved must be 0", fn);
  if (c->width == 0 || c->height == 0 || c->width > SOL_LIGHTMAP_MAX_SIZE || c->height > SOL_LIGHTMAP_MAX_SIZE)
    return sol_fail(SOL_EINVAL, "%s: an atlas of %u x %u texels (1 .. %u each way)", fn, c->width, c->height, SOL_LIGHTMAP_MAX_SIZE);
  if (c->iterations < 1 || c->iterations > 8) return sol_fail(SOL_EINVAL, "%s: %u iterations (1 .. 8)", fn, c->iterations);
  if (c->normal_power_log2 > 7) return sol_fail(SOL_EINVAL, "%s: normal_power_log2 %u (0 .. 7)", fn, c->normal_power_log2);
  const float sigma[3] = {c->sigma_position, c->sigma_plane, c->sigma_value};
  const char* const sigma_name[3] = {"sigma_position", "sigma_plane", "sigma_value"};
  for (int k = 0; k < 3; ++k)
    if (!(sigma[k] >= 1e-6f)) return sol_fail(SOL_EINVAL, "%s: %s %g (at least 1e-6, not NaN; +inf switches the factor off)", fn, sigma_name[k], (double)sigma[k]);
  if (!(std::isfinite(c->value_scale) && c->value_scale > 0.0f)) return sol_fail(SOL_EINVAL, "%s: value_scale %g (finite, > 0)", fn, (double)c->value_scale);
  if (c->channels == 0 || c->channels > 32) return sol_fail(SOL_EINVAL, "%s: %u channels (1 .. 32)", fn, c->channels);
  if (c->stride_bytes % 4 != 0 || c->stride_bytes / 4 < c->channels)
    return sol_fail(SOL_EINVAL, "%s: a stride of %u bytes (a multiple of 4, at least 4 x %u channels)", fn, c->stride_bytes, c->channels);
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
  if ((rc = filter_check(s != nullptr, "sol_lightmap_filter_dev", config, points_dev, texels_dev, values_dev, out_dev)) || (rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  return filter_launch(s, *config, points_dev, texels_dev, values_dev, out_dev);
}

int sol_lightmap_filter(SolScene* s, const SolLightmapFilterConfig* config, const SolRay* points, const SolTexel* texels, const void* values, void* out) {
  int rc;
  if ((rc = filter_check(s != nullptr, "sol_lightmap_filter", config, points, texels, values, out)) || (rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const size_t wh = (size_t)config->width * config->height, row = config->stride_bytes;
  SolStage st;
  const size_t at_p = st.add(wh * sizeof(SolRay)), at_t = st.add(wh * sizeof(SolTexel)), at_v = st.add(wh * row), at_o = st.add(wh * row);
  if ((rc = s->lm_stage.reserve(s->stream, st.total))) return rc;
  char* base = s->lm_stage.get();
  HIP_TRY(hipMemcpyAsync(base + at_p, points, wh * sizeof(SolRay), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(base + at_t, texels, wh * sizeof(SolTexel), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(base + at_v, values, wh * row, hipMemcpyHostToDevice, s->stream));
  if ((rc = filter_launch(s, *config, base + at_p, base + at_t, base + at_v, base + at_o))) return rc;
  HIP_TRY(hipMemcpyAsync(out, base + at_o, wh * row, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}

}  // extern "C"
