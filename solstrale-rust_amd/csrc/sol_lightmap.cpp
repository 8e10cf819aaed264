// sol_lightmap.cpp -- sol_lightmap_points and sol_lightmap_dilate (include/solstrale_hip.h): a mesh's lightmap UVs rasterised on the
// device into the point rows the gathers take, and the border dilation that finishes a bake (kernels: sol_lightmap.hip; the rule: sol_lightmap.h).
// The handle supplies the device, the stream and the scratch (SolScene::lm_owner; lm_stage for the host routes); the scene itself is not read:
// nothing is traced. Every refusal is decided before the device is looked for, from the arguments alone.
#include <cmath>
#include <cstring>

#include "sol_scene.h"

namespace {
constexpr size_t LM_MAX_TRIANGLES = ((size_t)1 << 31) - 2;
constexpr size_t LM_CTR_WORDS = 16;  // the two list counters, padded so that the owner words stay 64-byte aligned

int atlas_check(const char* fn, uint32_t width, uint32_t height) {
  if (width == 0 || height == 0 || width > SOL_LIGHTMAP_MAX_SIZE || height > SOL_LIGHTMAP_MAX_SIZE)
    return sol_fail(SOL_EINVAL, "%s: an atlas of %u x %u texels (1 .. %u each way)", fn, width, height, SOL_LIGHTMAP_MAX_SIZE);
  return SOL_OK;
}

int points_check(const SolScene* s, const char* fn, const void* vertices, const void* uvs, size_t n, const SolLightmapConfig* c, const void* points,
                 const void* texels) {
  if (!s || !c) return sol_fail(SOL_EINVAL, "%s: null %s", fn, !s ? "scene" : "configuration");
  if (c->size != sizeof(SolLightmapConfig)) return sol_fail(SOL_EINVAL, "%s: SolLightmapConfig.size %u (expected %zu)", fn, c->size, sizeof(SolLightmapConfig));
  if (c->reserved[0] || c->reserved[1]) return sol_fail(SOL_EINVAL, "%s: SolLightmapConfig.reserved must be 0", fn);
  if (c->flags & ~SOL_LIGHTMAP_CONSERVATIVE) return sol_fail(SOL_EINVAL, "%s: SolLightmapConfig.flags 0x%x: unknown bits", fn, c->flags);
  if (const int rc = atlas_check(fn, c->width, c->height)) return rc;
  if (!(std::isfinite(c->tmin) && c->tmin >= 0.0f && c->tmin <= c->tmax))
    return sol_fail(SOL_EINVAL, "%s: tmin %g, tmax %g (0 <= tmin <= tmax, tmin finite, tmax not NaN)", fn, (double)c->tmin, (double)c->tmax);
  if (n > LM_MAX_TRIANGLES) return sol_fail(SOL_EINVAL, "%s: %zu triangles in one call (at most 2^31 - 2)", fn, n);
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
  if (const int rc = atlas_check(fn, width, height)) return rc;
  if (channels == 0 || channels > 32) return sol_fail(SOL_EINVAL, "%s: %u channels (1 .. 32)", fn, channels);
  if (stride_bytes % 4 != 0 || stride_bytes / 4 < channels)
    return sol_fail(SOL_EINVAL, "%s: a stride of %u bytes (a multiple of 4, at least 4 x %u channels)", fn, stride_bytes, channels);
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
  if ((rc = points_check(s, "sol_lightmap_points_dev", vertices_dev, uvs_dev, n_triangles, config, points_out_dev, texels_out_dev)) || (rc = sol_device_check()))
    return rc;
  HIP_TRY(hipSetDevice(s->device));
  return points_launch(s, vertices_dev, normals_dev, uvs_dev, n_triangles, *config, points_out_dev, texels_out_dev);
}

int sol_lightmap_points(SolScene* s, const float* vertices, const float* normals, const float* uvs, size_t n_triangles, const SolLightmapConfig* config,
                        SolRay* points_out, SolTexel* texels_out) {
  int rc;
  if ((rc = points_check(s, "sol_lightmap_points", vertices, uvs, n_triangles, config, points_out, texels_out)) || (rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const size_t n = n_triangles, wh = (size_t)config->width * config->height;
  SolStage st;
  const size_t at_v = st.add(n * 9 * sizeof(float)), at_n = st.add(normals ? n * 9 * sizeof(float) : 0), at_uv = st.add(n * 6 * sizeof(float));
  const size_t at_p = st.add(wh * sizeof(SolRay)), at_t = st.add(wh * sizeof(SolTexel));
  if ((rc = s->lm_stage.reserve(s->stream, st.total))) return rc;
  char* base = s->lm_stage.get();
  if (n) {
    HIP_TRY(hipMemcpyAsync(base + at_v, vertices, n * 9 * sizeof(float), hipMemcpyHostToDevice, s->stream));
    if (normals) HIP_TRY(hipMemcpyAsync(base + at_n, normals, n * 9 * sizeof(float), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(base + at_uv, uvs, n * 6 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  }
  if ((rc = points_launch(s, base + at_v, normals ? base + at_n : nullptr, base + at_uv, n, *config, base + at_p, base + at_t))) return rc;
  HIP_TRY(hipMemcpyAsync(points_out, base + at_p, wh * sizeof(SolRay), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(texels_out, base + at_t, wh * sizeof(SolTexel), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}

int sol_lightmap_dilate_dev(SolScene* s, const void* texels_dev, uint32_t width, uint32_t height, const void* values_dev, uint32_t channels,
                            uint32_t stride_bytes, uint32_t passes, void* out_dev, void* pass_of_out_dev) {
  int rc;
  if ((rc = dilate_check(s, "sol_lightmap_dilate_dev", texels_dev, width, height, values_dev, channels, stride_bytes, passes, out_dev)) || (rc = sol_device_check()))
    return rc;
  HIP_TRY(hipSetDevice(s->device));
  return dilate_launch(s, texels_dev, width, height, values_dev, channels, stride_bytes, passes, out_dev, pass_of_out_dev);
}

int sol_lightmap_dilate(SolScene* s, const SolTexel* texels, uint32_t width, uint32_t height, const void* values, uint32_t channels, uint32_t stride_bytes,
                        uint32_t passes, void* out, uint8_t* pass_of_out) {
  int rc;
  if ((rc = dilate_check(s, "sol_lightmap_dilate", texels, width, height, values, channels, stride_bytes, passes, out)) || (rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const size_t wh = (size_t)width * height;
  SolStage st;
  const size_t at_t = st.add(wh * sizeof(SolTexel)), at_v = st.add(wh * stride_bytes), at_o = st.add(wh * stride_bytes), at_p = st.add(wh);
  if ((rc = s->lm_stage.reserve(s->stream, st.total))) return rc;
  char* base = s->lm_stage.get();
  HIP_TRY(hipMemcpyAsync(base + at_t, texels, wh * sizeof(SolTexel), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(base + at_v, values, wh * stride_bytes, hipMemcpyHostToDevice, s->stream));
  if ((rc = dilate_launch(s, base + at_t, width, height, base + at_v, channels, stride_bytes, passes, base + at_o, base + at_p))) return rc;
  HIP_TRY(hipMemcpyAsync(out, base + at_o, wh * stride_bytes, hipMemcpyDeviceToHost, s->stream));
  if (pass_of_out) HIP_TRY(hipMemcpyAsync(pass_of_out, base + at_p, wh, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}

}  // extern "C"
