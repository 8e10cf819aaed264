// sol_lightmap_mips.cpp -- sol_lightmap_mip_layout, sol_lightmap_mips, sol_lightmap_sample_lod and sol_lightmap_lod (include/solstrale_hip.h;
// DESIGN.md 31): the mip chain of a baked atlas, its trilinear lookup and the level of detail of a hit (kernels: sol_lightmap_mips.hip; the rule:
// sol_lightmap_mips.h; the layout: lmm_layout of sol_launch.h). The handle supplies the device, the stream and the staging of the host routes
// (SolScene::lm_stage); the scene itself is not read: nothing is traced. Every refusal is decided before the device is looked for, from the
// arguments alone - the checks below are not given the handle's contents, only whether there is one.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "sol_scene.h"

namespace {
constexpr size_t LMM_MAX_TRIANGLES = ((size_t)1 << 31) - 2;
constexpr size_t LMM_MAX_ROWS = (size_t)1 << 31;

// SOL_LIGHTMAP_MIPS=levels: a launch per level down to 1 x 1, the measured alternative of the tail kernel (the same words)
bool mips_tail() {
  const char* e = std::getenv("SOL_LIGHTMAP_MIPS");
  return !(e && std::strcmp(e, "levels") == 0);
}

int atlas_check(const char* fn, uint32_t width, uint32_t height, uint32_t channels, uint32_t stride_bytes) {
  if (width == 0 || height == 0 || width > SOL_LIGHTMAP_MAX_SIZE || height > SOL_LIGHTMAP_MAX_SIZE)
    return sol_fail(SOL_EINVAL, "%s: an atlas of %u x %u texels (1 .. %u each way)", fn, width, height, SOL_LIGHTMAP_MAX_SIZE);
  if (channels == 0 || channels > 32) return sol_fail(SOL_EINVAL, "%s: %u channels (1 .. 32)", fn, channels);
  if (stride_bytes % 4 != 0 || stride_bytes / 4 < channels)
    return sol_fail(SOL_EINVAL, "%s: a stride of %u bytes (a multiple of 4, at least 4 x %u channels)", fn, stride_bytes, channels);
  return SOL_OK;
}

int levels_check(const char* fn, uint32_t width, uint32_t height, uint32_t levels) {
  const uint32_t full = lmm_layout(width, height, 0).full;
  if (levels > full) return sol_fail(SOL_EINVAL, "%s: %u levels (an atlas of %u x %u texels has %u; 0: all)", fn, levels, width, height, full);
  return SOL_OK;
}

int mips_check(bool have_scene, const char* fn, const void* texels, const void* pass_of, uint32_t width, uint32_t height, const void* values, uint32_t channels,
               uint32_t stride_bytes, uint32_t levels, const void* mips, const void* cover) {
  int rc;
  if (!have_scene) return sol_fail(SOL_EINVAL, "%s: null scene", fn);
  if ((rc = atlas_check(fn, width, height, channels, stride_bytes)) || (rc = levels_check(fn, width, height, levels))) return rc;
  if (!texels || !values) return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !texels ? "texel" : "value");
  if (lmm_layout(width, height, levels).levels > 1) {
    if (!mips || !cover) return sol_fail(SOL_EINVAL, "%s: null %s output pointer", fn, !mips ? "chain" : "cover");
    if (mips == values || mips == texels || mips == cover) return sol_fail(SOL_EINVAL, "%s: mips_out may not be %s", fn, mips == values ? "values" : mips == texels ? "texels" : "cover_out");
    if (cover == values || cover == texels || (pass_of && cover == pass_of))
      return sol_fail(SOL_EINVAL, "%s: cover_out may not be %s", fn, cover == values ? "values" : cover == texels ? "texels" : "pass_of");
  }
  return SOL_OK;
}

int lod_config_check(const char* fn, const SolLightmapLodConfig* c) {
  int rc;
  if (c->size != sizeof(SolLightmapLodConfig))
    return sol_fail(SOL_EINVAL, "%s: SolLightmapLodConfig.size %u (expected %zu)", fn, c->size, sizeof(SolLightmapLodConfig));
  if (c->reserved[0] || c->reserved[1]) return sol_fail(SOL_EINVAL, "%s: SolLightmapLodConfig.reserved must be 0", fn);
  if (c->flags) return sol_fail(SOL_EINVAL, "%s: SolLightmapLodConfig.flags 0x%x: unknown bits", fn, c->flags);
  if ((rc = atlas_check(fn, c->width, c->height, c->channels, c->stride_bytes))) return rc;
  if (!(c->chart_radius > 0.0f)) return sol_fail(SOL_EINVAL, "%s: chart_radius %g (> 0, not NaN; +inf switches the guard off)", fn, (double)c->chart_radius);
  return SOL_OK;
}

int sample_lod_check(bool have_scene, const char* fn, const SolLightmapLodConfig* c, const void* uvs, size_t n_triangles, const void* texels, const void* values,
                     const void* mips, const void* cover, const void* vertices, const void* points, const void* coords, const void* lods, size_t n,
                     const void* out) {
  int rc;
  if (!have_scene || !c) return sol_fail(SOL_EINVAL, "%s: null %s", fn, !have_scene ? "scene" : "configuration");
  if ((rc = lod_config_check(fn, c))) return rc;
  if ((vertices != nullptr) != (points != nullptr))
    return sol_fail(SOL_EINVAL, "%s: vertices and points go together (the %s pointer is null)", fn, !vertices ? "vertex" : "point");
  if (std::isfinite(c->chart_radius) && !vertices)
    return sol_fail(SOL_EINVAL, "%s: a finite chart_radius needs the guard arrays (vertices and points)", fn);
  if ((rc = levels_check(fn, c->width, c->height, c->levels))) return rc;
  if (n_triangles > LMM_MAX_TRIANGLES) return sol_fail(SOL_EINVAL, "%s: %zu triangles in one call (at most 2^31 - 2)", fn, n_triangles);
  if (n > LMM_MAX_ROWS) return sol_fail(SOL_EINVAL, "%s: %zu rows in one call (at most 2^31)", fn, n);
  if ((n_triangles > 0 && !uvs) || !texels || !values || !coords || !lods || !out)
    return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn,
                    (n_triangles > 0 && !uvs) ? "UV" : !texels ? "texel" : !values ? "value" : !coords ? "coordinate" : !lods ? "lod" : "output");
  if (lmm_layout(c->width, c->height, c->levels).levels > 1 && (!mips || !cover))
    return sol_fail(SOL_EINVAL, "%s: null %s pointer with more than one level", fn, !mips ? "chain" : "cover");
  if (out == values || out == coords || out == lods || (mips && out == mips))
    return sol_fail(SOL_EINVAL, "%s: out may not be %s", fn, out == values ? "values" : out == coords ? "coords" : out == lods ? "lods" : "mips");
  return SOL_OK;
}

int lod_check(bool have_scene, const char* fn, const void* rays, const void* hits, const void* coords, size_t n, const void* vertices, const void* uvs,
              size_t n_triangles, uint32_t width, uint32_t height, float spread, float bias, const void* out) {
  if (!have_scene) return sol_fail(SOL_EINVAL, "%s: null scene", fn);
  if (width == 0 || height == 0 || width > SOL_LIGHTMAP_MAX_SIZE || height > SOL_LIGHTMAP_MAX_SIZE)
    return sol_fail(SOL_EINVAL, "%s: an atlas of %u x %u texels (1 .. %u each way)", fn, width, height, SOL_LIGHTMAP_MAX_SIZE);
  if (!(std::isfinite(spread) && spread > 0.0f)) return sol_fail(SOL_EINVAL, "%s: spread %g (finite, > 0)", fn, (double)spread);
  if (!std::isfinite(bias)) return sol_fail(SOL_EINVAL, "%s: bias %g (finite)", fn, (double)bias);
  if (n_triangles > LMM_MAX_TRIANGLES) return sol_fail(SOL_EINVAL, "%s: %zu triangles in one call (at most 2^31 - 2)", fn, n_triangles);
  if (n > LMM_MAX_ROWS) return sol_fail(SOL_EINVAL, "%s: %zu rows in one call (at most 2^31)", fn, n);
  if (n_triangles > 0 && (!vertices || !uvs)) return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !vertices ? "vertex" : "UV");
  if (!rays || !hits || !coords || !out)
    return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !rays ? "ray" : !hits ? "hit" : !coords ? "coordinate" : "output");
  if (out == rays || out == hits || out == coords) return sol_fail(SOL_EINVAL, "%s: out may not be %s", fn, out == rays ? "rays" : out == hits ? "hits" : "coords");
  return SOL_OK;
}

}  // namespace

extern "C" {

int sol_lightmap_mip_layout(uint32_t width, uint32_t height, uint32_t levels, uint32_t* levels_out, uint32_t* widths, uint32_t* heights, uint64_t* row_offsets,
                            uint64_t* total_rows) {
  int rc;
  const char* fn = "sol_lightmap_mip_layout";
  if (width == 0 || height == 0 || width > SOL_LIGHTMAP_MAX_SIZE || height > SOL_LIGHTMAP_MAX_SIZE)
    return sol_fail(SOL_EINVAL, "%s: an atlas of %u x %u texels (1 .. %u each way)", fn, width, height, SOL_LIGHTMAP_MAX_SIZE);
  if ((rc = levels_check(fn, width, height, levels))) return rc;
  const LmmLayout L = lmm_layout(width, height, levels);
  if (levels_out) *levels_out = L.levels;
  for (uint32_t l = 0; l < SOL_LIGHTMAP_MAX_LEVELS; ++l) {
    const bool in = l < L.levels;
    if (widths) widths[l] = in ? L.w[l] : 0;
    if (heights) heights[l] = in ? L.h[l] : 0;
    if (row_offsets) row_offsets[l] = in ? L.at[l] : 0;
  }
  if (total_rows) *total_rows = L.rows;
  return SOL_OK;
}

int sol_lightmap_mips_dev(SolScene* s, const void* texels_dev, const void* pass_of_dev, uint32_t width, uint32_t height, const void* values_dev, uint32_t channels,
                          uint32_t stride_bytes, uint32_t levels, void* mips_out_dev, void* cover_out_dev) {
  int rc;
  if ((rc = mips_check(s != nullptr, "sol_lightmap_mips_dev", texels_dev, pass_of_dev, width, height, values_dev, channels, stride_bytes, levels, mips_out_dev,
                       cover_out_dev)))
    return rc;
  const LmmLayout L = lmm_layout(width, height, levels);
  if (L.levels == 1) return SOL_OK;
  if ((rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(sol_launch_lightmap_mips(L, channels, stride_bytes / 4, mips_tail(), texels_dev, pass_of_dev, values_dev, mips_out_dev, cover_out_dev, s->stream));
  return SOL_OK;
}

int sol_lightmap_mips(SolScene* s, const SolTexel* texels, const uint8_t* pass_of, uint32_t width, uint32_t height, const void* values, uint32_t channels,
                      uint32_t stride_bytes, uint32_t levels, void* mips_out, uint8_t* cover_out) {
  int rc;
  if ((rc = mips_check(s != nullptr, "sol_lightmap_mips", texels, pass_of, width, height, values, channels, stride_bytes, levels, mips_out, cover_out))) return rc;
  const LmmLayout L = lmm_layout(width, height, levels);
  if (L.levels == 1) return SOL_OK;
  if ((rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const size_t wh = (size_t)width * height, row = stride_bytes;
  SolStage st;
  const size_t at_t = st.add(wh * sizeof(SolTexel)), at_p = st.add(pass_of ? wh : 0), at_v = st.add(wh * row), at_m = st.add(L.rows * row), at_c = st.add(L.rows);
  if ((rc = s->lm_stage.reserve(s->stream, st.total))) return rc;
  char* base = s->lm_stage.get();
  HIP_TRY(hipMemcpyAsync(base + at_t, texels, wh * sizeof(SolTexel), hipMemcpyHostToDevice, s->stream));
  if (pass_of) HIP_TRY(hipMemcpyAsync(base + at_p, pass_of, wh, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(base + at_v, values, wh * row, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(sol_launch_lightmap_mips(L, channels, stride_bytes / 4, mips_tail(), base + at_t, pass_of ? base + at_p : nullptr, base + at_v, base + at_m, base + at_c,
                                   s->stream));
  HIP_TRY(hipMemcpyAsync(mips_out, base + at_m, L.rows * row, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(cover_out, base + at_c, L.rows, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}

int sol_lightmap_sample_lod_dev(SolScene* s, const SolLightmapLodConfig* config, const void* uvs_dev, size_t n_triangles, const void* texels_dev,
                                const void* pass_of_dev, const void* values_dev, const void* mips_dev, const void* cover_dev, const void* vertices_dev,
                                const void* points_dev, const void* coords_dev, const void* lods_dev, size_t n, void* out_dev) {
  int rc;
  if ((rc = sample_lod_check(s != nullptr, "sol_lightmap_sample_lod_dev", config, uvs_dev, n_triangles, texels_dev, values_dev, mips_dev, cover_dev, vertices_dev,
                             points_dev, coords_dev, lods_dev, n, out_dev)))
    return rc;
  if (n == 0) return SOL_OK;
  if ((rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(sol_launch_lightmap_sample_lod(*config, lmm_layout(config->width, config->height, config->levels), (uint32_t)n_triangles, uvs_dev, texels_dev,
                                         pass_of_dev, values_dev, mips_dev, cover_dev, vertices_dev, points_dev, coords_dev, lods_dev, (uint32_t)n, out_dev,
                                         s->stream));
  return SOL_OK;
}

int sol_lightmap_sample_lod(SolScene* s, const SolLightmapLodConfig* config, const float* uvs, size_t n_triangles, const SolTexel* texels, const uint8_t* pass_of,
                            const void* values, const void* mips, const uint8_t* cover, const float* vertices, const SolRay* points, const SolTexel* coords,
                            const float* lods, size_t n, void* out) {
  int rc;
  if ((rc = sample_lod_check(s != nullptr, "sol_lightmap_sample_lod", config, uvs, n_triangles, texels, values, mips, cover, vertices, points, coords, lods, n, out)))
    return rc;
  if (n == 0) return SOL_OK;
  if ((rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const LmmLayout L = lmm_layout(config->width, config->height, config->levels);
  const size_t wh = (size_t)config->width * config->height, row = config->stride_bytes, out_row = ((size_t)config->channels + 1) * 4, nt = n_triangles;
  SolStage st;
  const size_t at_uv = st.add(nt * 6 * sizeof(float)), at_t = st.add(wh * sizeof(SolTexel)), at_pass = st.add(pass_of ? wh : 0), at_v = st.add(wh * row);
  const size_t at_m = st.add(L.rows * row), at_cv = st.add(L.rows);
  const size_t at_vx = st.add(vertices ? nt * 9 * sizeof(float) : 0), at_p = st.add(points ? wh * sizeof(SolRay) : 0), at_c = st.add(n * sizeof(SolTexel));
  const size_t at_l = st.add(n * sizeof(float)), at_o = st.add(n * out_row);
  if ((rc = s->lm_stage.reserve(s->stream, st.total))) return rc;
  char* base = s->lm_stage.get();
  if (nt) HIP_TRY(hipMemcpyAsync(base + at_uv, uvs, nt * 6 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(base + at_t, texels, wh * sizeof(SolTexel), hipMemcpyHostToDevice, s->stream));
  if (pass_of) HIP_TRY(hipMemcpyAsync(base + at_pass, pass_of, wh, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(base + at_v, values, wh * row, hipMemcpyHostToDevice, s->stream));
  if (L.rows) {
    HIP_TRY(hipMemcpyAsync(base + at_m, mips, L.rows * row, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(base + at_cv, cover, L.rows, hipMemcpyHostToDevice, s->stream));
  }
  if (vertices && nt) HIP_TRY(hipMemcpyAsync(base + at_vx, vertices, nt * 9 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  if (points) HIP_TRY(hipMemcpyAsync(base + at_p, points, wh * sizeof(SolRay), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(base + at_c, coords, n * sizeof(SolTexel), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(base + at_l, lods, n * sizeof(float), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(sol_launch_lightmap_sample_lod(*config, L, (uint32_t)nt, base + at_uv, base + at_t, pass_of ? base + at_pass : nullptr, base + at_v, base + at_m,
                                         base + at_cv, vertices ? base + at_vx : nullptr, points ? base + at_p : nullptr, base + at_c, base + at_l, (uint32_t)n,
                                         base + at_o, s->stream));
  HIP_TRY(hipMemcpyAsync(out, base + at_o, n * out_row, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}

int sol_lightmap_lod_dev(SolScene* s, const void* rays_dev, const void* hits_dev, const void* coords_dev, size_t n, const void* vertices_dev, const void* uvs_dev,
                         size_t n_triangles, uint32_t width, uint32_t height, float spread, float bias, void* lods_out_dev) {
  int rc;
  if ((rc = lod_check(s != nullptr, "sol_lightmap_lod_dev", rays_dev, hits_dev, coords_dev, n, vertices_dev, uvs_dev, n_triangles, width, height, spread, bias,
                      lods_out_dev)))
    return rc;
  if (n == 0) return SOL_OK;
  if ((rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(sol_launch_lightmap_lod(rays_dev, hits_dev, coords_dev, (uint32_t)n, vertices_dev, uvs_dev, (uint32_t)n_triangles, width, height, spread, bias,
                                  lods_out_dev, s->stream));
  return SOL_OK;
}

int sol_lightmap_lod(SolScene* s, const SolRay* rays, const SolRayHit* hits, const SolTexel* coords, size_t n, const float* vertices, const float* uvs,
                     size_t n_triangles, uint32_t width, uint32_t height, float spread, float bias, float* lods_out) {
  int rc;
  if ((rc = lod_check(s != nullptr, "sol_lightmap_lod", rays, hits, coords, n, vertices, uvs, n_triangles, width, height, spread, bias, lods_out))) return rc;
  if (n == 0) return SOL_OK;
  if ((rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const size_t nt = n_triangles;
  SolStage st;
  const size_t at_r = st.add(n * sizeof(SolRay)), at_h = st.add(n * sizeof(SolRayHit)), at_c = st.add(n * sizeof(SolTexel));
  const size_t at_v = st.add(nt * 9 * sizeof(float)), at_uv = st.add(nt * 6 * sizeof(float)), at_o = st.add(n * sizeof(float));
  if ((rc = s->lm_stage.reserve(s->stream, st.total))) return rc;
  char* base = s->lm_stage.get();
  HIP_TRY(hipMemcpyAsync(base + at_r, rays, n * sizeof(SolRay), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(base + at_h, hits, n * sizeof(SolRayHit), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(base + at_c, coords, n * sizeof(SolTexel), hipMemcpyHostToDevice, s->stream));
  if (nt) {
    HIP_TRY(hipMemcpyAsync(base + at_v, vertices, nt * 9 * sizeof(float), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(base + at_uv, uvs, nt * 6 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  }
  HIP_TRY(sol_launch_lightmap_lod(base + at_r, base + at_h, base + at_c, (uint32_t)n, base + at_v, base + at_uv, (uint32_t)nt, width, height, spread, bias,
                                  base + at_o, s->stream));
  HIP_TRY(hipMemcpyAsync(lods_out, base + at_o, n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}

}  // extern "C"
