// sol_lightmap_charts.cpp -- sol_lightmap_charts, sol_lightmap_dilate_charts, sol_lightmap_sample_charts and sol_lightmap_chart_levels
// (include/solstrale_hip.h): UV islands labelled on the device, the dilation and the lookup that keep them apart, and the count of
// mip levels before two of them meet (kernels: sol_lightmap_charts.hip; the rule: sol_lightmap_charts.h). The handle supplies the device, the
// stream, the scratch (SolScene::lm_owner) and the staging of the host routes (SolScene::lm_stage through SolStaged, sol_stage.h); the scene
// itself is not read: nothing is traced. Every refusal is decided before the device is looked for, from the arguments alone - the checks below
// (their shared sentences: sol_bake_checks.h; the 2^30 triangles are this family's own) are not given the handle's contents, only whether there
// is one.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "sol_bake_checks.h"
#include "sol_stage.h"

namespace {
constexpr size_t LC_MAX_TRIANGLES = SOL_LIGHTMAP_CHARTS_MAX_TRIANGLES;

// SOL_LIGHTMAP_CHARTS=collide: the edge hash masked to 4 bits, the tested worst case of the match (the same labels)
bool charts_collide() {
  const char* e = std::getenv("SOL_LIGHTMAP_CHARTS");
  return e && std::strcmp(e, "collide") == 0;
}

int charts_check(bool have_scene, const char* fn, const void* uvs, size_t n, const void* chart_of, const void* n_charts) {
  if (!have_scene) return sol_fail(SOL_EINVAL, "%s: null scene", fn);
  if (n > LC_MAX_TRIANGLES) return sol_fail(SOL_EINVAL, "%s: %zu triangles in one call (at most 2^30)", fn, n);
  if (n > 0 && (!uvs || !chart_of)) return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !uvs ? "UV" : "label output");
  if (!n_charts) return sol_fail(SOL_EINVAL, "%s: null chart count pointer", fn);
  return SOL_OK;
}

// The labelling over n triangles; its scratch is sized here. (n == 0, the device route only: the launch writes *n_charts = 0.)
int charts_launch(SolScene* s, const void* uvs, const void* vertices, size_t n_triangles, void* chart_of, void* n_charts) {
  int rc;
  const uint32_t n = (uint32_t)n_triangles;
  LcScratch S{};
  S.words = 1;
  if (n) HIP_TRY(sol_lightmap_charts_scratch(n, S));
  if ((rc = s->lm_owner.reserve(s->stream, S.words))) return rc;
  HIP_TRY(sol_launch_lightmap_charts(uvs, vertices, n, charts_collide(), S, s->lm_owner.get(), chart_of, n_charts, s->stream));
  return SOL_OK;
}

int dilate_check(bool have_scene, const char* fn, const void* texels, uint32_t width, uint32_t height, const void* values, uint32_t channels,
                 uint32_t stride_bytes, uint32_t passes, const void* chart_of, size_t n_triangles, const void* out, const void* pass_of, const void* plane) {
  int rc;
  if (!have_scene) return sol_fail(SOL_EINVAL, "%s: null scene", fn);
  if (!texels || !values || !out || !pass_of || !plane)
    return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !texels ? "texel" : !values ? "value" : !out ? "output" : !pass_of ? "pass_of output" : "plane output");
  if ((rc = sol_atlas_check(fn, width, height)) || (rc = sol_channels_check(fn, channels, stride_bytes))) return rc;
  if (passes > 254) return sol_fail(SOL_EINVAL, "%s: %u passes (at most 254)", fn, passes);
  if (out == values) return sol_fail(SOL_EINVAL, "%s: out may not be values", fn);
  if (n_triangles > 0 && !chart_of) return sol_fail(SOL_EINVAL, "%s: null chart_of_triangle pointer", fn);
  if (n_triangles > LC_MAX_TRIANGLES) return sol_fail(SOL_EINVAL, "%s: %zu triangles in one call (at most 2^30)", fn, n_triangles);
  return SOL_OK;
}

// The coverage planes ping-pong in the words of the scratch, as sol_lightmap_dilate's; the last one written is pass_of.
int dilate_launch(SolScene* s, const void* texels, uint32_t width, uint32_t height, const void* values, uint32_t channels, uint32_t stride_bytes, uint32_t passes,
                  const void* chart_of, size_t n_triangles, void* out, void* pass_of, void* plane) {
  int rc;
  const size_t wh = (size_t)width * height;
  if ((rc = s->lm_owner.reserve(s->stream, (2 * wh + 3) / 4))) return rc;
  uint8_t* cover[2] = {(uint8_t*)s->lm_owner.get(), (uint8_t*)s->lm_owner.get() + wh};
  HIP_TRY(sol_launch_lightmap_dilate_charts_begin(texels, (uint32_t)wh, values, stride_bytes / 4, chart_of, (uint32_t)n_triangles, out, cover[0], plane, s->stream));
  for (uint32_t k = 1; k <= passes; ++k)
    HIP_TRY(sol_launch_lightmap_dilate_charts_pass(width, height, channels, stride_bytes / 4, k, out, cover[(k - 1) & 1], cover[k & 1], plane, s->stream));
  HIP_TRY(hipMemcpyAsync(pass_of, cover[passes & 1], wh, hipMemcpyDeviceToDevice, s->stream));
  return SOL_OK;
}

int sample_check(bool have_scene, const char* fn, const SolLightmapSampleConfig* c, const void* uvs, size_t n_triangles, const void* texels, const void* values,
                 const void* chart_of, const void* plane, const void* coords, size_t n, const void* out) {
  int rc;
  if (!have_scene || !c) return sol_fail(SOL_EINVAL, "%s: null %s", fn, !have_scene ? "scene" : "configuration");
  if ((rc = sol_config_head_check(fn, "SolLightmapSampleConfig", *c, c->flags, SOL_LIGHTMAP_SAMPLE_NEAREST))) return rc;
  if ((rc = sol_atlas_check(fn, c->width, c->height)) || (rc = sol_channels_check(fn, c->channels, c->stride_bytes))) return rc;
  if (!(std::isinf(c->chart_radius) && c->chart_radius > 0.0f))
    return sol_fail(SOL_EINVAL, "%s: chart_radius %g (+inf: the guard is the chart id)", fn, (double)c->chart_radius);
  if (n_triangles > LC_MAX_TRIANGLES) return sol_fail(SOL_EINVAL, "%s: %zu triangles in one call (at most 2^30)", fn, n_triangles);
  if ((rc = sol_rows_check(fn, n, "rows"))) return rc;
  if ((n_triangles > 0 && (!uvs || !chart_of)) || !texels || !values || !plane || !coords || !out)
    return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn,
                    (n_triangles > 0 && !uvs)        ? "UV"
                    : (n_triangles > 0 && !chart_of) ? "chart_of_triangle"
                    : !texels                        ? "texel"
                    : !values                        ? "value"
                    : !plane                         ? "plane"
                    : !coords                        ? "coordinate"
                                                     : "output");
  if (out == values || out == coords) return sol_fail(SOL_EINVAL, "%s: out may not be %s", fn, out == values ? "values" : "coords");
  return SOL_OK;
}

int sample_launch(SolScene* s, const SolLightmapSampleConfig& c, const void* uvs, size_t n_triangles, const void* texels, const void* pass_of, const void* values,
                  const void* chart_of, const void* plane, const void* coords, size_t n, void* out) {
  HIP_TRY(sol_launch_lightmap_sample_charts(c, (uint32_t)n_triangles, uvs, texels, pass_of, values, chart_of, plane, coords, (uint32_t)n, out, s->stream));
  return SOL_OK;
}

int levels_check(bool have_scene, const char* fn, const void* plane, uint32_t width, uint32_t height, const void* levels, const void* mixed_texels,
                 const void* mixed_windows) {
  int rc;
  if (!have_scene) return sol_fail(SOL_EINVAL, "%s: null scene", fn);
  if ((rc = sol_atlas_check(fn, width, height))) return rc;
  if (!plane || !levels || !mixed_texels || !mixed_windows)
    return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !plane ? "plane" : !levels ? "levels" : !mixed_texels ? "mixed_texels" : "mixed_windows");
  return SOL_OK;
}

// The plane reduced level by level in the scratch (L = lmm_layout(width, height, 0): L.rows words and a counter).
int levels_launch(SolScene* s, const LmmLayout& L, const void* plane, const void* pass_of, void* levels, void* mixed_texels, void* mixed_windows) {
  int rc;
  if ((rc = s->lm_owner.reserve(s->stream, (size_t)L.rows + 1))) return rc;
  HIP_TRY(sol_launch_lightmap_chart_levels(L, plane, pass_of, s->lm_owner.get(), levels, mixed_texels, mixed_windows, s->stream));
  return SOL_OK;
}

}  // namespace

extern "C" {

int sol_lightmap_charts_dev(SolScene* s, const void* uvs_dev, const void* vertices_dev, size_t n_triangles, void* chart_of_triangle_out_dev,
                            void* n_charts_out_dev) {
  int rc;
  if ((rc = charts_check(s != nullptr, "sol_lightmap_charts_dev", uvs_dev, n_triangles, chart_of_triangle_out_dev, n_charts_out_dev)) || (rc = sol_device_enter(s)))
    return rc;
  return charts_launch(s, uvs_dev, vertices_dev, n_triangles, chart_of_triangle_out_dev, n_charts_out_dev);
}

int sol_lightmap_charts(SolScene* s, const float* uvs, const float* vertices, size_t n_triangles, uint32_t* chart_of_triangle_out, uint32_t* n_charts_out) {
  int rc;
  if ((rc = charts_check(s != nullptr, "sol_lightmap_charts", uvs, n_triangles, chart_of_triangle_out, n_charts_out))) return rc;
  if (n_triangles == 0) {
    *n_charts_out = 0;
    return SOL_OK;
  }
  if ((rc = sol_device_enter(s))) return rc;
  const size_t nt = n_triangles;
  SolStaged st(s->stream, s->lm_stage);
  const int uv = st.in(uvs, nt * 6 * sizeof(float)), vx = st.in_opt(vertices, nt * 9 * sizeof(float));
  const int c = st.out(chart_of_triangle_out, nt * sizeof(uint32_t)), n = st.out(n_charts_out, sizeof(uint32_t));
  if ((rc = st.upload()) || (rc = charts_launch(s, st[uv], st[vx], nt, st[c], st[n]))) return rc;
  return st.finish();
}

int sol_lightmap_dilate_charts_dev(SolScene* s, const void* texels_dev, uint32_t width, uint32_t height, const void* values_dev, uint32_t channels,
                                   uint32_t stride_bytes, uint32_t passes, const void* chart_of_triangle_dev, size_t n_triangles, void* out_dev,
                                   void* pass_of_out_dev, void* chart_plane_out_dev) {
  int rc;
  if ((rc = dilate_check(s != nullptr, "sol_lightmap_dilate_charts_dev", texels_dev, width, height, values_dev, channels, stride_bytes, passes,
                         chart_of_triangle_dev, n_triangles, out_dev, pass_of_out_dev, chart_plane_out_dev)) ||
      (rc = sol_device_enter(s)))
    return rc;
  return dilate_launch(s, texels_dev, width, height, values_dev, channels, stride_bytes, passes, chart_of_triangle_dev, n_triangles, out_dev, pass_of_out_dev,
                       chart_plane_out_dev);
}

int sol_lightmap_dilate_charts(SolScene* s, const SolTexel* texels, uint32_t width, uint32_t height, const void* values, uint32_t channels,
                               uint32_t stride_bytes, uint32_t passes, const uint32_t* chart_of_triangle, size_t n_triangles, void* out, uint8_t* pass_of_out,
                               uint32_t* chart_plane_out) {
  int rc;
  if ((rc = dilate_check(s != nullptr, "sol_lightmap_dilate_charts", texels, width, height, values, channels, stride_bytes, passes, chart_of_triangle,
                         n_triangles, out, pass_of_out, chart_plane_out)) ||
      (rc = sol_device_enter(s)))
    return rc;
  const size_t wh = (size_t)width * height, nt = n_triangles;
  SolStaged st(s->stream, s->lm_stage);
  const int t = st.in(texels, wh * sizeof(SolTexel)), v = st.in(values, wh * stride_bytes), c = st.in(chart_of_triangle, nt * sizeof(uint32_t));
  const int o = st.out(out, wh * stride_bytes), p = st.out(pass_of_out, wh), pl = st.out(chart_plane_out, wh * sizeof(uint32_t));
  if ((rc = st.upload()) || (rc = dilate_launch(s, st[t], width, height, st[v], channels, stride_bytes, passes, st[c], nt, st[o], st[p], st[pl]))) return rc;
  return st.finish();
}

int sol_lightmap_sample_charts_dev(SolScene* s, const SolLightmapSampleConfig* config, const void* uvs_dev, size_t n_triangles, const void* texels_dev,
                                   const void* pass_of_dev, const void* values_dev, const void* chart_of_triangle_dev, const void* chart_plane_dev,
                                   const void* coords_dev, size_t n, void* out_dev) {
  int rc;
  if ((rc = sample_check(s != nullptr, "sol_lightmap_sample_charts_dev", config, uvs_dev, n_triangles, texels_dev, values_dev, chart_of_triangle_dev,
                         chart_plane_dev, coords_dev, n, out_dev)) ||
      n == 0 || (rc = sol_device_enter(s)))
    return rc;
  return sample_launch(s, *config, uvs_dev, n_triangles, texels_dev, pass_of_dev, values_dev, chart_of_triangle_dev, chart_plane_dev, coords_dev, n, out_dev);
}

int sol_lightmap_sample_charts(SolScene* s, const SolLightmapSampleConfig* config, const float* uvs, size_t n_triangles, const SolTexel* texels,
                               const uint8_t* pass_of, const void* values, const uint32_t* chart_of_triangle, const uint32_t* chart_plane, const SolTexel* coords,
                               size_t n, void* out) {
  int rc;
  if ((rc = sample_check(s != nullptr, "sol_lightmap_sample_charts", config, uvs, n_triangles, texels, values, chart_of_triangle, chart_plane, coords, n, out)) ||
      n == 0 || (rc = sol_device_enter(s)))
    return rc;
  const size_t wh = (size_t)config->width * config->height, row = config->stride_bytes, out_row = ((size_t)config->channels + 1) * 4, nt = n_triangles;
  SolStaged st(s->stream, s->lm_stage);
  const int uv = st.in(uvs, nt * 6 * sizeof(float)), t = st.in(texels, wh * sizeof(SolTexel)), pass = st.in_opt(pass_of, wh), v = st.in(values, wh * row);
  const int ch = st.in(chart_of_triangle, nt * sizeof(uint32_t)), pl = st.in(chart_plane, wh * sizeof(uint32_t)), c = st.in(coords, n * sizeof(SolTexel));
  const int o = st.out(out, n * out_row);
  if ((rc = st.upload()) || (rc = sample_launch(s, *config, st[uv], nt, st[t], st[pass], st[v], st[ch], st[pl], st[c], n, st[o]))) return rc;
  return st.finish();
}

int sol_lightmap_chart_levels_dev(SolScene* s, const void* chart_plane_dev, const void* pass_of_dev, uint32_t width, uint32_t height, void* levels_out_dev,
                                  void* mixed_texels_out_dev, void* mixed_windows_out_dev) {
  int rc;
  if ((rc = levels_check(s != nullptr, "sol_lightmap_chart_levels_dev", chart_plane_dev, width, height, levels_out_dev, mixed_texels_out_dev,
                         mixed_windows_out_dev)) ||
      (rc = sol_device_enter(s)))
    return rc;
  return levels_launch(s, lmm_layout(width, height, 0), chart_plane_dev, pass_of_dev, levels_out_dev, mixed_texels_out_dev, mixed_windows_out_dev);
}

int sol_lightmap_chart_levels(SolScene* s, const uint32_t* chart_plane, const uint8_t* pass_of, uint32_t width, uint32_t height, uint32_t* levels_out,
                              uint32_t* mixed_texels_out, uint32_t* mixed_windows_out) {
  int rc;
  if ((rc = levels_check(s != nullptr, "sol_lightmap_chart_levels", chart_plane, width, height, levels_out, mixed_texels_out, mixed_windows_out))) return rc;
  const LmmLayout L = lmm_layout(width, height, 0);
  if (L.full == 1) {  // a 1 x 1 plane: level 0 alone, and level 0 is not judged
    *levels_out = 1;
    std::memset(mixed_texels_out, 0, SOL_LIGHTMAP_MAX_LEVELS * sizeof(uint32_t));
    std::memset(mixed_windows_out, 0, SOL_LIGHTMAP_MAX_LEVELS * sizeof(uint32_t));
    return SOL_OK;
  }
  if ((rc = sol_device_enter(s))) return rc;
  const size_t wh = (size_t)width * height, counts = SOL_LIGHTMAP_MAX_LEVELS * sizeof(uint32_t);
  SolStaged st(s->stream, s->lm_stage);
  const int pl = st.in(chart_plane, wh * sizeof(uint32_t)), p = st.in_opt(pass_of, wh);
  const int l = st.out(levels_out, sizeof(uint32_t)), mt = st.out(mixed_texels_out, counts), mw = st.out(mixed_windows_out, counts);
  if ((rc = st.upload()) || (rc = levels_launch(s, L, st[pl], st[p], st[l], st[mt], st[mw]))) return rc;
  return st.finish();
}

}  // extern "C"
