// sol_lightmap.cpp -- sol_lightmap_points and sol_lightmap_dilate (include/solstrale_hip.h): a mesh's lightmap UVs rasterised on the
// device into the point rows the gathers take, and the border dilation that finishes a bake (kernels: sol_lightmap.hip; the rule: sol_lightmap.h).
// The handle supplies the device, the stream and the scratch (SolScene::lm_owner; lm_stage for the host routes, laid out by SolStaged,
// sol_stage.h); the scene itself is not read: nothing is traced. Every refusal is decided before the device is looked for (sol_device_enter), from
// the arguments alone; the sentences other families share are sol_bake_checks.h's, their order is this file's.
#include <cmath>
#include <cstring>

#include "sol_bake_checks.h"
#include "sol_stage.h"

namespace {
constexpr size_t LM_CTR_WORDS = 16;  // the two list counters, padded so that the owner words stay 64-byte aligned

int points_check(const SolScene* s, const char* fn, const void* vertices, const void* uvs, size_t n, const SolLightmapConfig* c, const void* points,
                 const void* texels) {
  if (!s || !c) return sol_fail(SOL_EINVAL, "%s: null %s", fn, !s ? "scene" : "configuration");
  if (const int rc = sol_config_head_check(fn, "SolLightmapConfig", *c, c->flags, SOL_LIGHTMAP_CONSERVATIVE)) return rc;
  if (const int rc = sol_atlas_check(fn, c->width, c->height)) return rc;
  if (!(std::isfinite(c->tmin) && c->tmin >= 0.0f && c->tmin <= c->tmax))
    return sol_fail(SOL_EINVAL, "%s: tmin %g, tmax %g (0 <= tmin <= tmax, tmin finite, tmax not NaN)", fn, (double)c->tmin, (double)c->tmax);
  if (const int rc = sol_triangles_check(fn, n)) return rc;
  if (n > 0 && (!vertices || !uvs)) return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !vertices ? "vertex" : "UV");
  if (!points || !texels) return sol_fail(SOL_EINVAL, "%s: null %s output pointer", fn, !points ? "point" : "texel");
  return SOL_OK;
}

// The two passes on the scene's stream. The scratch: counters, owner words, the two work lists.
int points_launch(SolScene* s, const void* vertices, const void* normals, const void* uvs, size_t n, const SolLightmapConfig& c, void* points, void* texels) {
  int rc;
  const size_t wh = (size_t)c.width * c.height;
  if ((rc = s->lm_owner.reserve(s->stream, LM_CTR_WORDS + wh + 2 * n))) return rc;
  uint32_t* ctr = s->lm_owner.get();
  uint32_t* owner = ctr + LM_CTR_WORDS;
  HIP_TRY(hipMemsetAsync(ctr, 0, LM_CTR_WORDS * sizeof(uint32_t), s->stream));
  HIP_TRY(hipMemsetAsync(owner, 0xFF, wh * sizeof(uint32_t), s->stream));
  const uint32_t persistent_blocks = (uint32_t)std::max(1, s->n_cu * 8);
  HIP_TRY(sol_launch_lightmap_points((const float*)vertices, (const float*)normals, (const float*)uvs, (uint32_t)n, c.width, c.height,
                                     (c.flags & SOL_LIGHTMAP_CONSERVATIVE) != 0, c.tmin, c.tmax, s->lm_small_max, s->lm_tiles_max, owner, ctr, owner + wh,
                                     owner + wh + n, persistent_blocks, points, texels, s->stream));
  return SOL_OK;
}

int dilate_check(const SolScene* s, const char* fn, const void* texels, uint32_t width, uint32_t height, const void* values, uint32_t channels,
                 uint32_t stride_bytes, uint32_t passes, const void* out) {
  if (!s) return sol_fail(SOL_EINVAL, "%s: null scene", fn);
  if (!texels || !values || !out) return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !texels ? "texel" : !values ? "value" : "output");
  if (const int rc = sol_atlas_check(fn, width, height)) return rc;
  if (const int rc = sol_channels_check(fn, channels, stride_bytes)) return rc;
  if (passes > 254) return sol_fail(SOL_EINVAL, "%s: %u passes (at most 254)", fn, passes);
  if (out == values) return sol_fail(SOL_EINVAL, "%s: out may not be values", fn);
  return SOL_OK;
}

// The coverage planes ping-pong in the words of the scratch; the last one written is pass_of.
int dilate_launch(SolScene* s, const void* texels, uint32_t width, uint32_t height, const void* values, uint32_t channels, uint32_t stride_bytes, uint32_t passes,
                  void* out, void* pass_of) {
  int rc;
  const size_t wh = (size_t)width * height;
  if ((rc = s->lm_owner.reserve(s->stream, (2 * wh + 3) / 4))) return rc;
  uint8_t* cover[2] = {(uint8_t*)s->lm_owner.get(), (uint8_t*)s->lm_owner.get() + wh};
  HIP_TRY(sol_launch_lightmap_dilate_begin(texels, (uint32_t)wh, values, stride_bytes / 4, out, cover[0], s->stream));
  for (uint32_t k = 1; k <= passes; ++k)
    HIP_TRY(sol_launch_lightmap_dilate_pass(width, height, channels, stride_bytes / 4, k, out, cover[(k - 1) & 1], cover[k & 1], s->stream));
  if (pass_of) HIP_TRY(hipMemcpyAsync(pass_of, cover[passes & 1], wh, hipMemcpyDeviceToDevice, s->stream));
  return SOL_OK;
}

}  // namespace

extern "C" {

int sol_lightmap_points_dev(SolScene* s, const void* vertices_dev, const void* normals_dev, const void* uvs_dev, size_t n_triangles,
                            const SolLightmapConfig* config, void* points_out_dev, void* texels_out_dev) {
  int rc;
  if ((rc = points_check(s, "sol_lightmap_points_dev", vertices_dev, uvs_dev, n_triangles, config, points_out_dev, texels_out_dev)) || (rc = sol_device_enter(s)))
    return rc;
  return points_launch(s, vertices_dev, normals_dev, uvs_dev, n_triangles, *config, points_out_dev, texels_out_dev);
}

int sol_lightmap_points(SolScene* s, const float* vertices, const float* normals, const float* uvs, size_t n_triangles, const SolLightmapConfig* config,
                        SolRay* points_out, SolTexel* texels_out) {
  int rc;
  if ((rc = points_check(s, "sol_lightmap_points", vertices, uvs, n_triangles, config, points_out, texels_out)) || (rc = sol_device_enter(s))) return rc;
  const size_t n = n_triangles, wh = (size_t)config->width * config->height;
  SolStaged st(s->stream, s->lm_stage);
  const int v = st.in(vertices, n * 9 * sizeof(float)), nm = st.in_opt(normals, n * 9 * sizeof(float)), uv = st.in(uvs, n * 6 * sizeof(float));
  const int p = st.out(points_out, wh * sizeof(SolRay)), t = st.out(texels_out, wh * sizeof(SolTexel));
  if ((rc = st.upload()) || (rc = points_launch(s, st[v], st[nm], st[uv], n, *config, st[p], st[t]))) return rc;
  return st.finish();
}

int sol_lightmap_dilate_dev(SolScene* s, const void* texels_dev, uint32_t width, uint32_t height, const void* values_dev, uint32_t channels,
                            uint32_t stride_bytes, uint32_t passes, void* out_dev, void* pass_of_out_dev) {
  int rc;
  if ((rc = dilate_check(s, "sol_lightmap_dilate_dev", texels_dev, width, height, values_dev, channels, stride_bytes, passes, out_dev)) || (rc = sol_device_enter(s)))
    return rc;
  return dilate_launch(s, texels_dev, width, height, values_dev, channels, stride_bytes, passes, out_dev, pass_of_out_dev);
}

int sol_lightmap_dilate(SolScene* s, const SolTexel* texels, uint32_t width, uint32_t height, const void* values, uint32_t channels, uint32_t stride_bytes,
                        uint32_t passes, void* out, uint8_t* pass_of_out) {
  int rc;
  if ((rc = dilate_check(s, "sol_lightmap_dilate", texels, width, height, values, channels, stride_bytes, passes, out)) || (rc = sol_device_enter(s))) return rc;
  const size_t wh = (size_t)width * height;
  SolStaged st(s->stream, s->lm_stage);
  const int t = st.in(texels, wh * sizeof(SolTexel)), v = st.in(values, wh * stride_bytes), o = st.out(out, wh * stride_bytes);
  const int p = st.out(pass_of_out, wh);  // (always staged and written: the launch's last coverage plane; copied back when the caller asked)
  if ((rc = st.upload()) || (rc = dilate_launch(s, st[t], width, height, st[v], channels, stride_bytes, passes, st[o], st[p]))) return rc;
  return st.finish();
}

}  // extern "C"
