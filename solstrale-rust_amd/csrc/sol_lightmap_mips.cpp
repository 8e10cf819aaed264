// sol_lightmap_mips.cpp -- sol_lightmap_mip_layout, sol_lightmap_mips, sol_lightmap_sample_lod and sol_lightmap_lod (include/solstrale_hip.h;
// DESIGN.md 31): the mip chain of a baked atlas, its trilinear lookup and the level of detail of a hit (kernels: sol_lightmap_mips.hip; the rule:
// sol_lightmap_mips.h; the layout: lmm_layout of sol_launch.h). The handle supplies the device, the stream and the staging of the host routes
// (SolScene::lm_stage through SolStaged, sol_stage.h); the scene itself is not read: nothing is traced. Every refusal is decided before the device
// is looked for, from the arguments alone - the checks below (their shared sentences: sol_bake_checks.h) are not given the handle's contents, only
// whether there is one.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "sol_bake_checks.h"
#include "sol_stage.h"

namespace {
// SOL_LIGHTMAP_MIPS=levels: a launch per level down to 1 x 1, the measured alternative of the tail kernel (the same words)
bool mips_tail() {
  const char* e = std::getenv("SOL_LIGHTMAP_MIPS");
  return !(e && std::strcmp(e, "levels") == 0);
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
  if ((rc = sol_atlas_check(fn, width, height)) || (rc = sol_channels_check(fn, channels, stride_bytes)) || (rc = levels_check(fn, width, height, levels)))
    return rc;
  if (!texels || !values) return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !texels ? "texel" : "value");
  if (lmm_layout(width, height, levels).levels > 1) {
    if (!mips || !cover) return sol_fail(SOL_EINVAL, "%s: null %s output pointer", fn, !mips ? "chain" : "cover");
    if (mips == values || mips == texels || mips == cover) return sol_fail(SOL_EINVAL, "%s: mips_out may not be %s", fn, mips == values ? "values" : mips == texels ? "texels" : "cover_out");
    if (cover == values || cover == texels || (pass_of && cover == pass_of))
      return sol_fail(SOL_EINVAL, "%s: cover_out may not be %s", fn, cover == values ? "values" : cover == texels ? "texels" : "pass_of");
  }
  return SOL_OK;
}

int sample_lod_check(bool have_scene, const char* fn, const SolLightmapLodConfig* c, const void* uvs, size_t n_triangles, const void* texels, const void* values,
                     const void* mips, const void* cover, const void* vertices, const void* points, const void* coords, const void* lods, size_t n,
                     const void* out) {
  int rc;
  if (!have_scene || !c) return sol_fail(SOL_EINVAL, "%s: null %s", fn, !have_scene ? "scene" : "configuration");
  if ((rc = sol_config_head_check(fn, "SolLightmapLodConfig", *c, c->flags, 0))) return rc;
  if ((rc = sol_atlas_check(fn, c->width, c->height)) || (rc = sol_channels_check(fn, c->channels, c->stride_bytes))) return rc;
  if ((rc = sol_chart_guard_check(fn, c->chart_radius, vertices, points)) || (rc = levels_check(fn, c->width, c->height, c->levels))) return rc;
  if ((rc = sol_triangles_check(fn, n_triangles)) || (rc = sol_rows_check(fn, n, "rows"))) return rc;
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
  int rc;
  if (!have_scene) return sol_fail(SOL_EINVAL, "%s: null scene", fn);
  if ((rc = sol_atlas_check(fn, width, height))) return rc;
  if (!(std::isfinite(spread) && spread > 0.0f)) return sol_fail(SOL_EINVAL, "%s: spread %g (finite, > 0)", fn, (double)spread);
  if (!std::isfinite(bias)) return sol_fail(SOL_EINVAL, "%s: bias %g (finite)", fn, (double)bias);
  if ((rc = sol_triangles_check(fn, n_triangles)) || (rc = sol_rows_check(fn, n, "rows"))) return rc;
  if (n_triangles > 0 && (!vertices || !uvs)) return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !vertices ? "vertex" : "UV");
  if (!rays || !hits || !coords || !out)
    return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !rays ? "ray" : !hits ? "hit" : !coords ? "coordinate" : "output");
  if (out == rays || out == hits || out == coords) return sol_fail(SOL_EINVAL, "%s: out may not be %s", fn, out == rays ? "rays" : out == hits ? "hits" : "coords");
  return SOL_OK;
}

// The three launches as both routes of an entry point run them, on the scene's stream.
int mips_launch(SolScene* s, const LmmLayout& L, uint32_t channels, uint32_t stride_bytes, const void* texels, const void* pass_of, const void* values, void* mips,
                void* cover) {
  HIP_TRY(sol_launch_lightmap_mips(L, channels, stride_bytes / 4, mips_tail(), texels, pass_of, values, mips, cover, s->stream));
  return SOL_OK;
}

int sample_lod_launch(SolScene* s, const SolLightmapLodConfig& c, const LmmLayout& L, const void* uvs, size_t n_triangles, const void* texels, const void* pass_of,
                      const void* values, const void* mips, const void* cover, const void* vertices, const void* points, const void* coords, const void* lods,
                      size_t n, void* out) {
  HIP_TRY(sol_launch_lightmap_sample_lod(c, L, (uint32_t)n_triangles, uvs, texels, pass_of, values, mips, cover, vertices, points, coords, lods, (uint32_t)n, out,
                                         s->stream));
  return SOL_OK;
}

int lod_launch(SolScene* s, const void* rays, const void* hits, const void* coords, size_t n, const void* vertices, const void* uvs, size_t n_triangles,
               uint32_t width, uint32_t height, float spread, float bias, void* out) {
  HIP_TRY(sol_launch_lightmap_lod(rays, hits, coords, (uint32_t)n, vertices, uvs, (uint32_t)n_triangles, width, height, spread, bias, out, s->stream));
  return SOL_OK;
}

}  // namespace

extern "C" {

int sol_lightmap_mip_layout(uint32_t width, uint32_t height, uint32_t levels, uint32_t* levels_out, uint32_t* widths, uint32_t* heights, uint64_t* row_offsets,
                            uint64_t* total_rows) {
  int rc;
  const char* fn = "sol_lightmap_mip_layout";
  if ((rc = sol_atlas_check(fn, width, height)) || (rc = levels_check(fn, width, height, levels))) return rc;
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
  if (L.levels == 1 || (rc = sol_device_enter(s))) return rc;
  return mips_launch(s, L, channels, stride_bytes, texels_dev, pass_of_dev, values_dev, mips_out_dev, cover_out_dev);
}

int sol_lightmap_mips(SolScene* s, const SolTexel* texels, const uint8_t* pass_of, uint32_t width, uint32_t height, const void* values, uint32_t channels,
                      uint32_t stride_bytes, uint32_t levels, void* mips_out, uint8_t* cover_out) {
  int rc;
  if ((rc = mips_check(s != nullptr, "sol_lightmap_mips", texels, pass_of, width, height, values, channels, stride_bytes, levels, mips_out, cover_out))) return rc;
  const LmmLayout L = lmm_layout(width, height, levels);
  if (L.levels == 1 || (rc = sol_device_enter(s))) return rc;
  const size_t wh = (size_t)width * height, row = stride_bytes;
  SolStaged st(s->stream, s->lm_stage);
  const int t = st.in(texels, wh * sizeof(SolTexel)), p = st.in_opt(pass_of, wh), v = st.in(values, wh * row);
  const int m = st.out(mips_out, L.rows * row), c = st.out(cover_out, L.rows);
  if ((rc = st.upload()) || (rc = mips_launch(s, L, channels, stride_bytes, st[t], st[p], st[v], st[m], st[c]))) return rc;
  return st.finish();
}

int sol_lightmap_sample_lod_dev(SolScene* s, const SolLightmapLodConfig* config, const void* uvs_dev, size_t n_triangles, const void* texels_dev,
                                const void* pass_of_dev, const void* values_dev, const void* mips_dev, const void* cover_dev, const void* vertices_dev,
                                const void* points_dev, const void* coords_dev, const void* lods_dev, size_t n, void* out_dev) {
  int rc;
  if ((rc = sample_lod_check(s != nullptr, "sol_lightmap_sample_lod_dev", config, uvs_dev, n_triangles, texels_dev, values_dev, mips_dev, cover_dev, vertices_dev,
                             points_dev, coords_dev, lods_dev, n, out_dev)) ||
      n == 0 || (rc = sol_device_enter(s)))
    return rc;
  return sample_lod_launch(s, *config, lmm_layout(config->width, config->height, config->levels), uvs_dev, n_triangles, texels_dev, pass_of_dev, values_dev,
                           mips_dev, cover_dev, vertices_dev, points_dev, coords_dev, lods_dev, n, out_dev);
}

int sol_lightmap_sample_lod(SolScene* s, const SolLightmapLodConfig* config, const float* uvs, size_t n_triangles, const SolTexel* texels, const uint8_t* pass_of,
                            const void* values, const void* mips, const uint8_t* cover, const float* vertices, const SolRay* points, const SolTexel* coords,
                            const float* lods, size_t n, void* out) {
  int rc;
  if ((rc = sample_lod_check(s != nullptr, "sol_lightmap_sample_lod", config, uvs, n_triangles, texels, values, mips, cover, vertices, points, coords, lods, n,
                             out)) ||
      n == 0 || (rc = sol_device_enter(s)))
    return rc;
  const LmmLayout L = lmm_layout(config->width, config->height, config->levels);
  const size_t wh = (size_t)config->width * config->height, row = config->stride_bytes, out_row = ((size_t)config->channels + 1) * 4, nt = n_triangles;
  SolStaged st(s->stream, s->lm_stage);
  const int uv = st.in(uvs, nt * 6 * sizeof(float)), t = st.in(texels, wh * sizeof(SolTexel)), pass = st.in_opt(pass_of, wh), v = st.in(values, wh * row);
  const int m = st.in(mips, L.rows * row), cv = st.in(cover, L.rows);  // (one level: no chain, 0 bytes, and still an address)
  const int vx = st.in_opt(vertices, nt * 9 * sizeof(float)), p = st.in_opt(points, wh * sizeof(SolRay)), c = st.in(coords, n * sizeof(SolTexel));
  const int l = st.in(lods, n * sizeof(float)), o = st.out(out, n * out_row);
  if ((rc = st.upload()) ||
      (rc = sample_lod_launch(s, *config, L, st[uv], nt, st[t], st[pass], st[v], st[m], st[cv], st[vx], st[p], st[c], st[l], n, st[o])))
    return rc;
  return st.finish();
}

int sol_lightmap_lod_dev(SolScene* s, const void* rays_dev, const void* hits_dev, const void* coords_dev, size_t n, const void* vertices_dev, const void* uvs_dev,
                         size_t n_triangles, uint32_t width, uint32_t height, float spread, float bias, void* lods_out_dev) {
  int rc;
  if ((rc = lod_check(s != nullptr, "sol_lightmap_lod_dev", rays_dev, hits_dev, coords_dev, n, vertices_dev, uvs_dev, n_triangles, width, height, spread, bias,
                      lods_out_dev)) ||
      n == 0 || (rc = sol_device_enter(s)))
    return rc;
  return lod_launch(s, rays_dev, hits_dev, coords_dev, n, vertices_dev, uvs_dev, n_triangles, width, height, spread, bias, lods_out_dev);
}

int sol_lightmap_lod(SolScene* s, const SolRay* rays, const SolRayHit* hits, const SolTexel* coords, size_t n, const float* vertices, const float* uvs,
                     size_t n_triangles, uint32_t width, uint32_t height, float spread, float bias, float* lods_out) {
  int rc;
  if ((rc = lod_check(s != nullptr, "sol_lightmap_lod", rays, hits, coords, n, vertices, uvs, n_triangles, width, height, spread, bias, lods_out)) || n == 0 ||
      (rc = sol_device_enter(s)))
    return rc;
  const size_t nt = n_triangles;
  SolStaged st(s->stream, s->lm_stage);
  const int r = st.in(rays, n * sizeof(SolRay)), h = st.in(hits, n * sizeof(SolRayHit)), c = st.in(coords, n * sizeof(SolTexel));
  const int v = st.in(vertices, nt * 9 * sizeof(float)), uv = st.in(uvs, nt * 6 * sizeof(float)), o = st.out(lods_out, n * sizeof(float));
  if ((rc = st.upload()) || (rc = lod_launch(s, st[r], st[h], st[c], n, st[v], st[uv], nt, width, height, spread, bias, st[o]))) return rc;
  return st.finish();
}

}  // extern "C"
