// sol_lightmap_sample.cpp -- sol_lightmap_coords and sol_lightmap_sample (include/solstrale_hip.h): closest hits turned into surface
// rows, and a baked atlas looked up at surface rows (kernels: sol_lightmap_sample.hip; the rule: sol_lightmap_sample.h). The handle supplies the
// device, the stream and the staging of the host routes (SolScene::lm_stage through SolStaged, sol_stage.h); the scene itself is not read: nothing
// is traced. Every refusal is decided before the device is looked for, from the arguments alone - the checks below (their shared sentences:
// sol_bake_checks.h) are not given the handle's contents, only whether there is one.
#include <cmath>

#include "sol_bake_checks.h"
#include "sol_stage.h"

namespace {
int coords_check(bool have_scene, const char* fn, const void* hits, size_t n, const void* table, size_t n_dfs, const void* out) {
  if (!have_scene) return sol_fail(SOL_EINVAL, "%s: null scene", fn);
  if (const int rc = sol_rows_check(fn, n, "hits")) return rc;
  if (n_dfs > SOL_BAKE_MAX_ROWS) return sol_fail(SOL_EINVAL, "%s: a table of %zu entries (at most 2^31)", fn, n_dfs);
  if (n_dfs > 0 && !table) return sol_fail(SOL_EINVAL, "%s: null table pointer", fn);
  if (!hits || !out) return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !hits ? "hit" : "output");
  if (out == hits) return sol_fail(SOL_EINVAL, "%s: out may not be hits", fn);
  return SOL_OK;
}

int coords_launch(SolScene* s, const void* hits, size_t n, const void* table, size_t n_dfs, void* out) {
  HIP_TRY(sol_launch_lightmap_coords(hits, (uint32_t)n, table, (uint32_t)n_dfs, out, s->stream));
  return SOL_OK;
}

int sample_check(bool have_scene, const char* fn, const SolLightmapSampleConfig* c, const void* uvs, size_t n_triangles, const void* texels, const void* values,
                 const void* vertices, const void* points, const void* coords, size_t n, const void* out) {
  int rc;
  if (!have_scene || !c) return sol_fail(SOL_EINVAL, "%s: null %s", fn, !have_scene ? "scene" : "configuration");
  if ((rc = sol_config_head_check(fn, "SolLightmapSampleConfig", *c, c->flags, SOL_LIGHTMAP_SAMPLE_NEAREST))) return rc;
  if ((rc = sol_atlas_check(fn, c->width, c->height)) || (rc = sol_channels_check(fn, c->channels, c->stride_bytes))) return rc;
  if ((rc = sol_chart_guard_check(fn, c->chart_radius, vertices, points))) return rc;
  if ((rc = sol_triangles_check(fn, n_triangles)) || (rc = sol_rows_check(fn, n, "rows"))) return rc;
  if ((n_triangles > 0 && !uvs) || !texels || !values || !coords || !out)
    return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn,
                    (n_triangles > 0 && !uvs) ? "UV" : !texels ? "texel" : !values ? "value" : !coords ? "coordinate" : "output");
  if (out == values || out == coords) return sol_fail(SOL_EINVAL, "%s: out may not be %s", fn, out == values ? "values" : "coords");
  return SOL_OK;
}

int sample_launch(SolScene* s, const SolLightmapSampleConfig& c, const void* uvs, size_t n_triangles, const void* texels, const void* pass_of, const void* values,
                  const void* vertices, const void* points, const void* coords, size_t n, void* out) {
  HIP_TRY(sol_launch_lightmap_sample(c, (uint32_t)n_triangles, uvs, texels, pass_of, values, vertices, points, coords, (uint32_t)n, out, s->stream));
  return SOL_OK;
}

}  // namespace

extern "C" {

int sol_lightmap_coords_dev(SolScene* s, const void* hits_dev, size_t n, const void* triangle_of_dfs_dev, size_t n_dfs, void* coords_out_dev) {
  int rc;
  if ((rc = coords_check(s != nullptr, "sol_lightmap_coords_dev", hits_dev, n, triangle_of_dfs_dev, n_dfs, coords_out_dev)) || n == 0 || (rc = sol_device_enter(s)))
    return rc;
  return coords_launch(s, hits_dev, n, triangle_of_dfs_dev, n_dfs, coords_out_dev);
}

int sol_lightmap_coords(SolScene* s, const SolRayHit* hits, size_t n, const uint32_t* triangle_of_dfs, size_t n_dfs, SolTexel* coords_out) {
  int rc;
  if ((rc = coords_check(s != nullptr, "sol_lightmap_coords", hits, n, triangle_of_dfs, n_dfs, coords_out)) || n == 0 || (rc = sol_device_enter(s))) return rc;
  SolStaged st(s->stream, s->lm_stage);
  const int h = st.in(hits, n * sizeof(SolRayHit)), t = st.in(triangle_of_dfs, n_dfs * sizeof(uint32_t)), o = st.out(coords_out, n * sizeof(SolTexel));
  if ((rc = st.upload()) || (rc = coords_launch(s, st[h], n, st[t], n_dfs, st[o]))) return rc;
  return st.finish();
}

int sol_lightmap_sample_dev(SolScene* s, const SolLightmapSampleConfig* config, const void* uvs_dev, size_t n_triangles, const void* texels_dev,
                            const void* pass_of_dev, const void* values_dev, const void* vertices_dev, const void* points_dev, const void* coords_dev, size_t n,
                            void* out_dev) {
  int rc;
  if ((rc = sample_check(s != nullptr, "sol_lightmap_sample_dev", config, uvs_dev, n_triangles, texels_dev, values_dev, vertices_dev, points_dev, coords_dev, n,
                         out_dev)) ||
      n == 0 || (rc = sol_device_enter(s)))
    return rc;
  return sample_launch(s, *config, uvs_dev, n_triangles, texels_dev, pass_of_dev, values_dev, vertices_dev, points_dev, coords_dev, n, out_dev);
}

int sol_lightmap_sample(SolScene* s, const SolLightmapSampleConfig* config, const float* uvs, size_t n_triangles, const SolTexel* texels, const uint8_t* pass_of,
                        const void* values, const float* vertices, const SolRay* points, const SolTexel* coords, size_t n, void* out) {
  int rc;
  if ((rc = sample_check(s != nullptr, "sol_lightmap_sample", config, uvs, n_triangles, texels, values, vertices, points, coords, n, out)) || n == 0 ||
      (rc = sol_device_enter(s)))
    return rc;
  const size_t wh = (size_t)config->width * config->height, row = config->stride_bytes, out_row = ((size_t)config->channels + 1) * 4, nt = n_triangles;
  SolStaged st(s->stream, s->lm_stage);
  const int uv = st.in(uvs, nt * 6 * sizeof(float)), t = st.in(texels, wh * sizeof(SolTexel)), pass = st.in_opt(pass_of, wh), v = st.in(values, wh * row);
  const int vx = st.in_opt(vertices, nt * 9 * sizeof(float)), p = st.in_opt(points, wh * sizeof(SolRay)), c = st.in(coords, n * sizeof(SolTexel));
  const int o = st.out(out, n * out_row);
  if ((rc = st.upload()) || (rc = sample_launch(s, *config, st[uv], nt, st[t], st[pass], st[v], st[vx], st[p], st[c], n, st[o]))) return rc;
  return st.finish();
}

}  // extern "C"
