// sol_lightmap_sh.cpp -- sol_lightmap_sh and sol_lightmap_normals (include/solstrale_hip.h): an atlas of SolSh9 rows looked up at
// surface rows and shaded at the caller's normals, and the surface's own normals (kernels: sol_lightmap_sh.hip; the rule: sol_lightmap_sh.h). The
// handle supplies the device, the stream and the staging of the host routes (SolScene::lm_stage through SolStaged, sol_stage.h); the scene itself
// is not read: nothing is traced. Every refusal is decided before the device is looked for, from the arguments alone - the checks below (their
// shared sentences: sol_bake_checks.h; the stride rule is this family's own) are not given the handle's contents, only whether there is one.
#include <cmath>

#include "sol_bake_checks.h"
#include "sol_stage.h"

namespace {
constexpr uint32_t LSH_ROW_BYTES = 112;  // a SolSh9
constexpr uint32_t LSH_FLAGS = SOL_LIGHTMAP_SH_NEAREST | SOL_LIGHTMAP_SH_COEFFICIENTS | SOL_LIGHTMAP_SH_CLAMP;

int sh_check(bool have_scene, const char* fn, const SolLightmapShConfig* c, const void* uvs, size_t n_triangles, const void* texels, const void* values,
             const void* vertices, const void* points, const void* coords, const void* normals, size_t n, const void* out) {
  if (!have_scene || !c) return sol_fail(SOL_EINVAL, "%s: null %s", fn, !have_scene ? "scene" : "configuration");
  if (const int rc = sol_config_head_check(fn, "SolLightmapShConfig", *c, c->flags, LSH_FLAGS)) return rc;
  const bool coefficients = (c->flags & SOL_LIGHTMAP_SH_COEFFICIENTS) != 0;
  if (coefficients && (c->flags & SOL_LIGHTMAP_SH_CLAMP))
    return sol_fail(SOL_EINVAL, "%s: SOL_LIGHTMAP_SH_CLAMP with SOL_LIGHTMAP_SH_COEFFICIENTS (coefficients are not clamped)", fn);
  if (const int rc = sol_atlas_check(fn, c->width, c->height)) return rc;
  if (c->stride_bytes < LSH_ROW_BYTES || c->stride_bytes % 16 != 0)
    return sol_fail(SOL_EINVAL, "%s: a stride of %u bytes (a multiple of 16, at least %u: a SolSh9)", fn, c->stride_bytes, LSH_ROW_BYTES);
  if (const int rc = sol_chart_guard_check(fn, c->chart_radius, vertices, points)) return rc;
  if (!coefficients && !std::isfinite(c->scale)) return sol_fail(SOL_EINVAL, "%s: scale %g (finite)", fn, (double)c->scale);
  if (const int rc = sol_triangles_check(fn, n_triangles)) return rc;
  if (const int rc = sol_rows_check(fn, n, "rows")) return rc;
  if ((n_triangles > 0 && !uvs) || !texels || !values || !coords)
    return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, (n_triangles > 0 && !uvs) ? "UV" : !texels ? "texel" : !values ? "value" : "coordinate");
  if (!coefficients && !normals) return sol_fail(SOL_EINVAL, "%s: null normals pointer (only SOL_LIGHTMAP_SH_COEFFICIENTS reads none)", fn);
  if (!out) return sol_fail(SOL_EINVAL, "%s: null output pointer", fn);
  if (out == values || out == coords || out == normals)
    return sol_fail(SOL_EINVAL, "%s: out may not be %s", fn, out == values ? "values" : out == coords ? "coords" : "normals");
  return SOL_OK;
}

int normals_check(bool have_scene, const char* fn, const void* coords, size_t n, const void* vertices, size_t n_triangles, const void* out) {
  if (!have_scene) return sol_fail(SOL_EINVAL, "%s: null scene", fn);
  if (const int rc = sol_triangles_check(fn, n_triangles)) return rc;
  if (const int rc = sol_rows_check(fn, n, "rows")) return rc;
  if (n_triangles > 0 && !vertices) return sol_fail(SOL_EINVAL, "%s: null vertex pointer", fn);
  if (!coords || !out) return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !coords ? "coordinate" : "output");
  if (out == coords) return sol_fail(SOL_EINVAL, "%s: out may not be coords", fn);
  return SOL_OK;
}

size_t out_row_bytes(const SolLightmapShConfig& c) { return (c.flags & SOL_LIGHTMAP_SH_COEFFICIENTS) ? LSH_ROW_BYTES : sizeof(SolRadiance); }

int sh_launch(SolScene* s, const SolLightmapShConfig& c, const void* uvs, size_t n_triangles, const void* texels, const void* pass_of, const void* values,
              const void* vertices, const void* points, const void* coords, const void* normals, size_t n, void* out) {
  HIP_TRY(sol_launch_lightmap_sh(c, (uint32_t)n_triangles, uvs, texels, pass_of, values, vertices, points, coords, normals, (uint32_t)n, out, s->stream));
  return SOL_OK;
}

int normals_launch(SolScene* s, const void* coords, size_t n, const void* vertices, const void* vertex_normals, size_t n_triangles, void* out) {
  HIP_TRY(sol_launch_lightmap_normals(coords, (uint32_t)n, vertices, vertex_normals, (uint32_t)n_triangles, out, s->stream));
  return SOL_OK;
}

}  // namespace

extern "C" {

int sol_lightmap_sh_dev(SolScene* s, const SolLightmapShConfig* config, const void* uvs_dev, size_t n_triangles, const void* texels_dev,
                        const void* pass_of_dev, const void* values_dev, const void* vertices_dev, const void* points_dev, const void* coords_dev,
                        const void* normals_dev, size_t n, void* out_dev) {
  int rc;
  if ((rc = sh_check(s != nullptr, "sol_lightmap_sh_dev", config, uvs_dev, n_triangles, texels_dev, values_dev, vertices_dev, points_dev, coords_dev,
                     normals_dev, n, out_dev)) ||
      n == 0 || (rc = sol_device_enter(s)))
    return rc;
  return sh_launch(s, *config, uvs_dev, n_triangles, texels_dev, pass_of_dev, values_dev, vertices_dev, points_dev, coords_dev, normals_dev, n, out_dev);
}

int sol_lightmap_sh(SolScene* s, const SolLightmapShConfig* config, const float* uvs, size_t n_triangles, const SolTexel* texels, const uint8_t* pass_of,
                    const void* values, const float* vertices, const SolRay* points, const SolTexel* coords, const float* normals, size_t n, void* out) {
  int rc;
  if ((rc = sh_check(s != nullptr, "sol_lightmap_sh", config, uvs, n_triangles, texels, values, vertices, points, coords, normals, n, out)) || n == 0 ||
      (rc = sol_device_enter(s)))
    return rc;
  const bool coefficients = (config->flags & SOL_LIGHTMAP_SH_COEFFICIENTS) != 0;
  const size_t wh = (size_t)config->width * config->height, row = config->stride_bytes, out_row = out_row_bytes(*config), nt = n_triangles;
  SolStaged st(s->stream, s->lm_stage);
  const int uv = st.in(uvs, nt * 6 * sizeof(float)), t = st.in(texels, wh * sizeof(SolTexel)), pass = st.in_opt(pass_of, wh), v = st.in(values, wh * row);
  const int vx = st.in_opt(vertices, nt * 9 * sizeof(float)), p = st.in_opt(points, wh * sizeof(SolRay)), c = st.in(coords, n * sizeof(SolTexel));
  const int nm = st.in_opt(coefficients ? nullptr : normals, n * 4 * sizeof(float));  // (coefficient mode reads no normals: none staged, whatever the caller passed)
  const int o = st.out(out, n * out_row);
  if ((rc = st.upload()) || (rc = sh_launch(s, *config, st[uv], nt, st[t], st[pass], st[v], st[vx], st[p], st[c], st[nm], n, st[o]))) return rc;
  return st.finish();
}

int sol_lightmap_normals_dev(SolScene* s, const void* coords_dev, size_t n, const void* vertices_dev, const void* vertex_normals_dev, size_t n_triangles,
                             void* normals_out_dev) {
  int rc;
  if ((rc = normals_check(s != nullptr, "sol_lightmap_normals_dev", coords_dev, n, vertices_dev, n_triangles, normals_out_dev)) || n == 0 ||
      (rc = sol_device_enter(s)))
    return rc;
  return normals_launch(s, coords_dev, n, vertices_dev, vertex_normals_dev, n_triangles, normals_out_dev);
}

int sol_lightmap_normals(SolScene* s, const SolTexel* coords, size_t n, const float* vertices, const float* vertex_normals, size_t n_triangles,
                         float* normals_out) {
  int rc;
  if ((rc = normals_check(s != nullptr, "sol_lightmap_normals", coords, n, vertices, n_triangles, normals_out)) || n == 0 || (rc = sol_device_enter(s))) return rc;
  const size_t tri_bytes = n_triangles * 9 * sizeof(float);
  SolStaged st(s->stream, s->lm_stage);
  const int c = st.in(coords, n * sizeof(SolTexel)), v = st.in(vertices, tri_bytes);
  const int vn = st.in_opt(n_triangles ? vertex_normals : nullptr, tri_bytes);  // (without triangles there are no vertex normals: a null pointer at the launch)
  const int o = st.out(normals_out, n * 4 * sizeof(float));
  if ((rc = st.upload()) || (rc = normals_launch(s, st[c], n, st[v], st[vn], n_triangles, st[o]))) return rc;
  return st.finish();
}

}  // extern "C"
