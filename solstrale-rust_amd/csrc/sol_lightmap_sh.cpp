// sol_lightmap_sh.cpp -- sol_lightmap_sh and sol_lightmap_normals (include/solstrale_hip.h): an atlas of SolSh9 rows looked up at
// surface rows and shaded at the caller's normals, and the surface's own normals (kernels: sol_lightmap_sh.hip; the rule: sol_lightmap_sh.h). The
// handle supplies the device, the stream and the staging of the host routes (SolScene::lm_stage); the scene itself is not read: nothing is traced.
// Every refusal is decided before the device is looked for, from the arguments alone - the checks below are not given the handle's contents,
// only whether there is one.
#include <cmath>

#include "sol_scene.h"

namespace {
constexpr size_t LSH_MAX_TRIANGLES = ((size_t)1 << 31) - 2;
constexpr size_t LSH_MAX_ROWS = (size_t)1 << 31;
constexpr uint32_t LSH_ROW_BYTES = 112;  // a SolSh9
constexpr uint32_t LSH_FLAGS = SOL_LIGHTMAP_SH_NEAREST | SOL_LIGHTMAP_SH_COEFFICIENTS | SOL_LIGHTMAP_SH_CLAMP;

int sh_check(bool have_scene, const char* fn, const SolLightmapShConfig* c, const void* uvs, size_t n_triangles, const void* texels, const void* values,
             const void* vertices, const void* points, const void* coords, const void* normals, size_t n, const void* out) {
  if (!have_scene || !c) return sol_fail(SOL_EINVAL, "%s: null %s", fn, !have_scene ? "scene" : "configuration");
  if (c->size != sizeof(SolLightmapShConfig))
    return sol_fail(SOL_EINVAL, "%s: SolLightmapShConfig.size %u (expected %zu)", fn, c->size, sizeof(SolLightmapShConfig));
  if (c->reserved) return sol_fail(SOL_EINVAL, "%s: SolLightmapShConfig.reserved must be 0", fn);
  if (c->flags & ~LSH_FLAGS) return sol_fail(SOL_EINVAL, "%s: SolLightmapShConfig.flags 0x%x: unknown bits", fn, c->flags);
  const bool coefficients = (c->flags & SOL_LIGHTMAP_SH_COEFFICIENTS) != 0;
  if (coefficients && (c->flags & SOL_LIGHTMAP_SH_CLAMP))
    return sol_fail(SOL_EINVAL, "%s: SOL_LIGHTMAP_SH_CLAMP with SOL_LIGHTMAP_SH_COEFFICIENTS (coefficients are not clamped)", fn);
  if (c->width == 0 || c->height == 0 || c->width > SOL_LIGHTMAP_MAX_SIZE || c->height > SOL_LIGHTMAP_MAX_SIZE)
    return sol_fail(SOL_EINVAL, "%s: an atlas of %u x %u texels (1 .. %u each way)", fn, c->width, c->height, SOL_LIGHTMAP_MAX_SIZE);
  if (c->stride_bytes < LSH_ROW_BYTES || c->stride_bytes % 16 != 0)
    return sol_fail(SOL_EINVAL, "%s: a stride of %u bytes (a multiple of 16, at least %u: a SolSh9)", fn, c->stride_bytes, LSH_ROW_BYTES);
  if (!(c->chart_radius > 0.0f)) return sol_fail(SOL_EINVAL, "%s: chart_radius %g (> 0, not NaN; +inf switches the guard off)", fn, (double)c->chart_radius);
  if ((vertices != nullptr) != (points != nullptr))
    return sol_fail(SOL_EINVAL, "%s: vertices and points go together (the %s pointer is null)", fn, !vertices ? "vertex" : "point");
  if (std::isfinite(c->chart_radius) && !vertices)
    return sol_fail(SOL_EINVAL, "%s: a finite chart_radius needs the guard arrays (vertices and points)", fn);
  if (!coefficients && !std::isfinite(c->scale)) return sol_fail(SOL_EINVAL, "%s: scale %g (finite)", fn, (double)c->scale);
  if (n_triangles > LSH_MAX_TRIANGLES) return sol_fail(SOL_EINVAL, "%s: %zu triangles in one call (at most 2^31 - 2)", fn, n_triangles);
  if (n > LSH_MAX_ROWS) return sol_fail(SOL_EINVAL, "%s: %zu rows in one call (at most 2^31)", fn, n);
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
  if (n_triangles > LSH_MAX_TRIANGLES) return sol_fail(SOL_EINVAL, "%s: %zu triangles in one call (at most 2^31 - 2)", fn, n_triangles);
  if (n > LSH_MAX_ROWS) return sol_fail(SOL_EINVAL, "%s: %zu rows in one call (at most 2^31)", fn, n);
  if (n_triangles > 0 && !vertices) return sol_fail(SOL_EINVAL, "%s: null vertex pointer", fn);
  if (!coords || !out) return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !coords ? "coordinate" : "output");
  if (out == coords) return sol_fail(SOL_EINVAL, "%s: out may not be coords", fn);
  return SOL_OK;
}

size_t out_row_bytes(const SolLightmapShConfig& c) { return (c.flags & SOL_LIGHTMAP_SH_COEFFICIENTS) ? LSH_ROW_BYTES : sizeof(SolRadiance); }

}  // namespace

extern "C" {

int sol_lightmap_sh_dev(SolScene* s, const SolLightmapShConfig* config, const void* uvs_dev, size_t n_triangles, const void* texels_dev,
                        const void* pass_of_dev, const void* values_dev, const void* vertices_dev, const void* points_dev, const void* coords_dev,
                        const void* normals_dev, size_t n, void* out_dev) {
  int rc;
  if ((rc = sh_check(s != nullptr, "sol_lightmap_sh_dev", config, uvs_dev, n_triangles, texels_dev, values_dev, vertices_dev, points_dev, coords_dev,
                     normals_dev, n, out_dev)))
    return rc;
  if (n == 0) return SOL_OK;
  if ((rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(sol_launch_lightmap_sh(*config, (uint32_t)n_triangles, uvs_dev, texels_dev, pass_of_dev, values_dev, vertices_dev, points_dev, coords_dev,
                                 normals_dev, (uint32_t)n, out_dev, s->stream));
  return SOL_OK;
}

int sol_lightmap_sh(SolScene* s, const SolLightmapShConfig* config, const float* uvs, size_t n_triangles, const SolTexel* texels, const uint8_t* pass_of,
                    const void* values, const float* vertices, const SolRay* points, const SolTexel* coords, const float* normals, size_t n, void* out) {
  int rc;
  if ((rc = sh_check(s != nullptr, "sol_lightmap_sh", config, uvs, n_triangles, texels, values, vertices, points, coords, normals, n, out))) return rc;
  if (n == 0) return SOL_OK;
  if ((rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const bool coefficients = (config->flags & SOL_LIGHTMAP_SH_COEFFICIENTS) != 0;
  const size_t wh = (size_t)config->width * config->height, row = config->stride_bytes, out_row = out_row_bytes(*config), nt = n_triangles;
  SolStage st;
  const size_t at_uv = st.add(nt * 6 * sizeof(float)), at_t = st.add(wh * sizeof(SolTexel)), at_pass = st.add(pass_of ? wh : 0), at_v = st.add(wh * row);
  const size_t at_vx = st.add(vertices ? nt * 9 * sizeof(float) : 0), at_p = st.add(points ? wh * sizeof(SolRay) : 0), at_c = st.add(n * sizeof(SolTexel));
  const size_t at_n = st.add(coefficients ? 0 : n * 4 * sizeof(float)), at_o = st.add(n * out_row);
  if ((rc = s->lm_stage.reserve(s->stream, st.total))) return rc;
  char* base = s->lm_stage.get();
  if (nt) HIP_TRY(hipMemcpyAsync(base + at_uv, uvs, nt * 6 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(base + at_t, texels, wh * sizeof(SolTexel), hipMemcpyHostToDevice, s->stream));
  if (pass_of) HIP_TRY(hipMemcpyAsync(base + at_pass, pass_of, wh, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(base + at_v, values, wh * row, hipMemcpyHostToDevice, s->stream));
  if (vertices && nt) HIP_TRY(hipMemcpyAsync(base + at_vx, vertices, nt * 9 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  if (points) HIP_TRY(hipMemcpyAsync(base + at_p, points, wh * sizeof(SolRay), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(base + at_c, coords, n * sizeof(SolTexel), hipMemcpyHostToDevice, s->stream));
  if (!coefficients) HIP_TRY(hipMemcpyAsync(base + at_n, normals, n * 4 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(sol_launch_lightmap_sh(*config, (uint32_t)nt, base + at_uv, base + at_t, pass_of ? base + at_pass : nullptr, base + at_v,
                                 vertices ? base + at_vx : nullptr, points ? base + at_p : nullptr, base + at_c, coefficients ? nullptr : base + at_n,
                                 (uint32_t)n, base + at_o, s->stream));
  HIP_TRY(hipMemcpyAsync(out, base + at_o, n * out_row, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}

int sol_lightmap_normals_dev(SolScene* s, const void* coords_dev, size_t n, const void* vertices_dev, const void* vertex_normals_dev, size_t n_triangles,
                             void* normals_out_dev) {
  int rc;
  if ((rc = normals_check(s != nullptr, "sol_lightmap_normals_dev", coords_dev, n, vertices_dev, n_triangles, normals_out_dev))) return rc;
  if (n == 0) return SOL_OK;
  if ((rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(sol_launch_lightmap_normals(coords_dev, (uint32_t)n, vertices_dev, vertex_normals_dev, (uint32_t)n_triangles, normals_out_dev, s->stream));
  return SOL_OK;
}

int sol_lightmap_normals(SolScene* s, const SolTexel* coords, size_t n, const float* vertices, const float* vertex_normals, size_t n_triangles,
                         float* normals_out) {
  int rc;
  if ((rc = normals_check(s != nullptr, "sol_lightmap_normals", coords, n, vertices, n_triangles, normals_out))) return rc;
  if (n == 0) return SOL_OK;
  if ((rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const size_t tri_bytes = n_triangles * 9 * sizeof(float);
  const bool have_normals = vertex_normals && n_triangles;
  SolStage st;
  const size_t at_c = st.add(n * sizeof(SolTexel)), at_v = st.add(tri_bytes), at_n = st.add(have_normals ? tri_bytes : 0), at_o = st.add(n * 4 * sizeof(float));
  if ((rc = s->lm_stage.reserve(s->stream, st.total))) return rc;
  char* base = s->lm_stage.get();
  HIP_TRY(hipMemcpyAsync(base + at_c, coords, n * sizeof(SolTexel), hipMemcpyHostToDevice, s->stream));
  if (n_triangles) HIP_TRY(hipMemcpyAsync(base + at_v, vertices, tri_bytes, hipMemcpyHostToDevice, s->stream));
  if (have_normals) HIP_TRY(hipMemcpyAsync(base + at_n, vertex_normals, tri_bytes, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(sol_launch_lightmap_normals(base + at_c, (uint32_t)n, base + at_v, have_normals ? base + at_n : nullptr, (uint32_t)n_triangles, base + at_o,
                                      s->stream));
  HIP_TRY(hipMemcpyAsync(normals_out, base + at_o, n * 4 * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}

}  // extern "C"
