// sol_lightmap_sample.cpp -- sol_lightmap_coords and sol_lightmap_sample (include/solstrale_hip.h): closest hits turned into surface
// rows, and a baked atlas looked up at surface rows (kernels: sol_lightmap_sample.hip; the rule: sol_lightmap_sample.h). The handle supplies the
// device, the stream and the staging of the host routes (SolScene::lm_stage); the scene itself is not read: nothing is traced. Every refusal is
// decided before the device is looked for, from the arguments alone - the checks below are not given the handle's contents, only whether there is one.
#include <cmath>

#include "sol_scene.h"

namespace {
constexpr size_t LS_MAX_TRIANGLES = ((size_t)1 << 31) - 2;
constexpr size_t LS_MAX_ROWS = (size_t)1 << 31;

int coords_check(bool have_scene, const char* fn, const void* hits, size_t n, const void* table, size_t n_dfs, const void* out) {
  if (!have_scene) return sol_fail(SOL_EINVAL, "%s: null scene", fn);
  if (n > LS_MAX_ROWS) return sol_fail(SOL_EINVAL, "%s: %zu hits in one call (at most 2^31)", fn, n);
  if (n_dfs > LS_MAX_ROWS) return sol_fail(SOL_EINVAL, "%s: a table of %zu entries (at most 2^31)", fn, n_dfs);
  if (n_dfs > 0 && !table) return sol_fail(SOL_EINVAL, "%s: null table pointer", fn);
  if (!hits || !out) return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !hits ? "hit" : "output");
  if (out == hits) return sol_fail(SOL_EINVAL, "%s: out may not be hits", fn);
  return SOL_OK;
}

int sample_check(bool have_scene, const char* fn, const SolLightmapSampleConfig* c, const void* uvs, size_t n_triangles, const void* texels, const void* values,
                 const void* vertices, const void* points, const void* coords, size_t n, const void* out) {
  if (!have_scene || !c) return sol_fail(SOL_EINVAL, "%s: null %s", fn, !have_scene ? "scene" : "configuration");
  if (c->size != sizeof(SolLightmapSampleConfig))
    return sol_fail(SOL_EINVAL, "%s: SolLightmapSampleConfig.size %u (expected %zu)", fn, c->size, sizeof(SolLightmapSampleConfig));
  if (c->reserved) return sol_fail(SOL_EINVAL, "%s: SolLightmapSampleConfig.reserved must be 0", fn);
  if (c->flags & ~SOL_LIGHTMAP_SAMPLE_NEAREST) return sol_fail(SOL_EINVAL, "%s: SolLightmapSampleConfig.flags 0x%x: unknown bits", fn, c->flags);
  if (c->width == 0 || c->height == 0 || c->width > SOL_LIGHTMAP_MAX_SIZE || c->height > SOL_LIGHTMAP_MAX_SIZE)
    return sol_fail(SOL_EINVAL, "%s: an atlas of %u x %u texels (1 .. %u each way)", fn, c->width, c->height, SOL_LIGHTMAP_MAX_SIZE);
  if (c->channels == 0 || c->channels > 32) return sol_fail(SOL_EINVAL, "%s: %u channels (1 .. 32)", fn, c->channels);
  if (c->stride_bytes % 4 != 0 || c->stride_bytes / 4 < c->channels)
    return sol_fail(SOL_EINVAL, "%s: a stride of %u bytes (a multiple of 4, at least 4 x %u channels)", fn, c->stride_bytes, c->channels);
  if (!(c->chart_radius > 0.0f)) return sol_fail(SOL_EINVAL, "%s: chart_radius %g (> 0, not NaN; +inf switches the guard off)", fn, (double)c->chart_radius);
  if ((vertices != nullptr) != (points != nullptr))
    return sol_fail(SOL_EINVAL, "%s: vertices and points go together (the %s pointer is null)", fn, !vertices ? "vertex" : "point");
  if (std::isfinite(c->chart_radius) && !vertices)
    return sol_fail(SOL_EINVAL, "%s: a finite chart_radius needs the guard arrays (vertices and points)", fn);
  if (n_triangles > LS_MAX_TRIANGLES) return sol_fail(SOL_EINVAL, "%s: %zu triangles in one call (at most 2^31 - 2)", fn, n_triangles);
  if (n > LS_MAX_ROWS) return sol_fail(SOL_EINVAL, "%s: %zu rows in one call (at most 2^31)", fn, n);
  if ((n_triangles > 0 && !uvs) || !texels || !values || !coords || !out)
    return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn,
                    (n_triangles > 0 && !uvs) ? "UV" : !texels ? "texel" : !values ? "value" : !coords ? "coordinate" : "output");
  if (out == values || out == coords) return sol_fail(SOL_EINVAL, "%s: out may not be %s", fn, out == values ? "values" : "coords");
  return SOL_OK;
}

}  // namespace

extern "C" {

int sol_lightmap_coords_dev(SolScene* s, const void* hits_dev, size_t n, const void* triangle_of_dfs_dev, size_t n_dfs, void* coords_out_dev) {
  int rc;
  if ((rc = coords_check(s != nullptr, "sol_lightmap_coords_dev", hits_dev, n, triangle_of_dfs_dev, n_dfs, coords_out_dev))) return rc;
  if (n == 0) return SOL_OK;
  if ((rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(sol_launch_lightmap_coords(hits_dev, (uint32_t)n, triangle_of_dfs_dev, (uint32_t)n_dfs, coords_out_dev, s->stream));
  return SOL_OK;
}

int sol_lightmap_coords(SolScene* s, const SolRayHit* hits, size_t n, const uint32_t* triangle_of_dfs, size_t n_dfs, SolTexel* coords_out) {
  int rc;
  if ((rc = coords_check(s != nullptr, "sol_lightmap_coords", hits, n, triangle_of_dfs, n_dfs, coords_out))) return rc;
  if (n == 0) return SOL_OK;
  if ((rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  SolStage st;
  const size_t at_h = st.add(n * sizeof(SolRayHit)), at_t = st.add(n_dfs * sizeof(uint32_t)), at_o = st.add(n * sizeof(SolTexel));
  if ((rc = s->lm_stage.reserve(s->stream, st.total))) return rc;
  char* base = s->lm_stage.get();
  HIP_TRY(hipMemcpyAsync(base + at_h, hits, n * sizeof(SolRayHit), hipMemcpyHostToDevice, s->stream));
  if (n_dfs) HIP_TRY(hipMemcpyAsync(base + at_t, triangle_of_dfs, n_dfs * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(sol_launch_lightmap_coords(base + at_h, (uint32_t)n, base + at_t, (uint32_t)n_dfs, base + at_o, s->stream));
  HIP_TRY(hipMemcpyAsync(coords_out, base + at_o, n * sizeof(SolTexel), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}

int sol_lightmap_sample_dev(SolScene* s, const SolLightmapSampleConfig* config, const void* uvs_dev, size_t n_triangles, const void* texels_dev,
                            const void* pass_of_dev, const void* values_dev, const void* vertices_dev, const void* points_dev, const void* coords_dev, size_t n,
                            void* out_dev) {
  int rc;
  if ((rc = sample_check(s != nullptr, "sol_lightmap_sample_dev", config, uvs_dev, n_triangles, texels_dev, values_dev, vertices_dev, points_dev, coords_dev, n,
                         out_dev)))
    return rc;
  if (n == 0) return SOL_OK;
  if ((rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(sol_launch_lightmap_sample(*config, (uint32_t)n_triangles, uvs_dev, texels_dev, pass_of_dev, values_dev, vertices_dev, points_dev, coords_dev,
                                     (uint32_t)n, out_dev, s->stream));
  return SOL_OK;
}

int sol_lightmap_sample(SolScene* s, const SolLightmapSampleConfig* config, const float* uvs, size_t n_triangles, const SolTexel* texels, const uint8_t* pass_of,
                        const void* values, const float* vertices, const SolRay* points, const SolTexel* coords, size_t n, void* out) {
  int rc;
  if ((rc = sample_check(s != nullptr, "sol_lightmap_sample", config, uvs, n_triangles, texels, values, vertices, points, coords, n, out))) return rc;
  if (n == 0) return SOL_OK;
  if ((rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const size_t wh = (size_t)config->width * config->height, row = config->stride_bytes, out_row = ((size_t)config->channels + 1) * 4, nt = n_triangles;
  SolStage st;
  const size_t at_uv = st.add(nt * 6 * sizeof(float)), at_t = st.add(wh * sizeof(SolTexel)), at_pass = st.add(pass_of ? wh : 0), at_v = st.add(wh * row);
  const size_t at_vx = st.add(vertices ? nt * 9 * sizeof(float) : 0), at_p = st.add(points ? wh * sizeof(SolRay) : 0), at_c = st.add(n * sizeof(SolTexel));
  const size_t at_o = st.add(n * out_row);
  if ((rc = s->lm_stage.reserve(s->stream, st.total))) return rc;
  char* base = s->lm_stage.get();
  if (nt) HIP_TRY(hipMemcpyAsync(base + at_uv, uvs, nt * 6 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(base + at_t, texels, wh * sizeof(SolTexel), hipMemcpyHostToDevice, s->stream));
  if (pass_of) HIP_TRY(hipMemcpyAsync(base + at_pass, pass_of, wh, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(base + at_v, values, wh * row, hipMemcpyHostToDevice, s->stream));
  if (vertices && nt) HIP_TRY(hipMemcpyAsync(base + at_vx, vertices, nt * 9 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  if (points) HIP_TRY(hipMemcpyAsync(base + at_p, points, wh * sizeof(SolRay), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(base + at_c, coords, n * sizeof(SolTexel), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(sol_launch_lightmap_sample(*config, (uint32_t)nt, base + at_uv, base + at_t, pass_of ? base + at_pass : nullptr, base + at_v,
                                     vertices ? base + at_vx : nullptr, points ? base + at_p : nullptr, base + at_c, (uint32_t)n, base + at_o, s->stream));
  HIP_TRY(hipMemcpyAsync(out, base + at_o, n * out_row, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}

}  // extern "C"
