// sol_depth.cpp -- sol_visibility_oct, sol_volume_build_depth and sol_volume_sample_depth (include/solstrale_hip.h): the directional
// distance moments of an irradiance volume (kernels: sol_depth.hip; the rule: sol_depth.h). The gather is a visibility gather: it shares the
// radiance queries' scratch and staging (SolScene::rad_*) and their launch plan; build and sample trace nothing and stage through
// SolScene::vol_stage. Every refusal is decided before the device is looked for.
#include <algorithm>
#include <cmath>

#include "sol_scene.h"

namespace {
constexpr size_t DEPTH_MAX_POINTS = (size_t)1 << 31;
constexpr size_t DEPTH_STAGE_TEXELS = (size_t)1 << 24;  // the gather's host route stages at most this many SolOctTexel rows at a time (256 MiB)

int device_check() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return sol_fail(SOL_EDEVICE, "no HIP device available");
  return SOL_OK;
}
int oct_config_check(const char* fn, const SolOctConfig* c) {
  if (!c) return sol_fail(SOL_EINVAL, "%s: null SolOctConfig", fn);
  if (c->size != sizeof(SolOctConfig)) return sol_fail(SOL_EINVAL, "%s: SolOctConfig.size is %u, not %zu", fn, c->size, sizeof(SolOctConfig));
  if (c->res != 4u && c->res != 8u && c->res != 16u) return sol_fail(SOL_EINVAL, "%s: SolOctConfig.res is %u (4, 8 or 16)", fn, c->res);
  if (c->sharpness_log2 > 6u) return sol_fail(SOL_EINVAL, "%s: SolOctConfig.sharpness_log2 is %u (0 to 6)", fn, c->sharpness_log2);
  if (c->reserved != 0u) return sol_fail(SOL_EINVAL, "%s: SolOctConfig.reserved must be 0", fn);
  return SOL_OK;
}
// sol_visibility's order with the SolOctConfig directly after the SolIrradianceConfig. *go = false: nothing to do (n == 0).
int gather_check(const SolScene* s, const char* fn, const void* points, size_t n, const SolIrradianceConfig* config, SolRadianceConfig* cfg, const SolOctConfig* oct,
                 const void* out, bool* go) {
  *go = false;
  if (!s) return sol_fail(SOL_EINVAL, "%s: null scene", fn);
  if (const int rc = sol_gather_config_check(fn, n, config, cfg)) return rc;
  if (const int rc = oct_config_check(fn, oct)) return rc;
  if (n == 0) return SOL_OK;
  if (const int rc = sol_query_medium_check(s, fn)) return rc;
  if (!points || !out) return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !points ? "point" : "output");
  *go = true;
  return SOL_OK;
}
int build_check(bool have_scene, const char* fn, const SolVolumeGrid* g, const void* oct, const SolOctConfig* c, float radius, const void* out) {
  if (const int rc = sol_volume_grid_check(have_scene, fn, g)) return rc;
  if (const int rc = oct_config_check(fn, c)) return rc;
  if (!(std::isfinite(radius) && radius > 0.0f)) return sol_fail(SOL_EINVAL, "%s: radius %g (finite and > 0)", fn, (double)radius);
  if (!oct || !out) return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !oct ? "SolOctTexel" : "output");
  return SOL_OK;
}
int sample_check(bool have_scene, const char* fn, const SolVolumeGrid* g, const void* probes, const void* depth, const SolOctConfig* c, const void* points, size_t n,
                 const void* out) {
  if (const int rc = sol_volume_grid_check(have_scene, fn, g)) return rc;
  if (const int rc = oct_config_check(fn, c)) return rc;
  if (n > DEPTH_MAX_POINTS) return sol_fail(SOL_EINVAL, "%s: %zu points in one call (at most 2^31)", fn, n);
  if (n > 0 && (!probes || !depth || !points || !out))
    return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !probes ? "probe" : !depth ? "depth" : !points ? "point" : "output");
  return SOL_OK;
}
size_t probes_of(const SolVolumeGrid& g) { return (size_t)g.nx * g.ny * g.nz; }

struct Stage {
  size_t total = 0;
  size_t add(size_t bytes) { const size_t at = total; total += (bytes + 255) / 256 * 256; return at; }
};

// n <= 2^31 points (and keys, or null) in device memory, n * res * res SolOctTexel out, on the scene's stream: irradiance_sh_launch's plan (sol_api.cpp)
// with this family's kernels. Every launch of the gather kernel writes one word per (point, sample) into the partial buffer and is followed by the
// projection kernel. A launch holds whole chunks of 64 x k points, words = points x samples <= SolScene::rad_partial_max_rows, at least one group of
// one chunk; the call is split over points (answers are per point) and over windows of chunks (the projection kernel carries a texel's sums from one
// window to the next in `out`: the same additions in the same order).
int gather_launch(SolScene* s, const void* points_dev, const void* keys_dev, size_t n, const SolRadianceConfig& cfg, uint32_t key_base, const SolOctConfig& oct,
                  void* out_dev) {
  int rc;
  if ((rc = sol_scene_to_device(s))) return rc;
  const int bpc = sol_depth_each_blocks_per_cu(s->strict_triangles);
  const bool may_spill = s->tree.depth > (uint32_t)SOL_LDS_STACK;
  if ((rc = s->rad_work.reserve(s->stream, 1))) return rc;
  const size_t total_chunks = (size_t)(((uint64_t)cfg.samples + SOL_CHUNK - 1) / SOL_CHUNK);
  const size_t unit = (size_t)64 * SOL_CHUNK;  // words of one group of points over one chunk
  const size_t units = std::max<size_t>(1, std::min<size_t>(s->rad_partial_max_rows, (size_t)1 << 31) / unit);
  const size_t win_chunks = std::min(total_chunks, units);
  const size_t slice_points = units / win_chunks * 64;
  const size_t texels = (size_t)oct.res * oct.res;
  for (size_t at = 0; at < n; at += slice_points) {
    const size_t k = std::min(slice_points, n - at);
    RadianceParams P{};
    P.n_rays = (uint32_t)k;
    P.n_groups = (uint32_t)((k + 63) / 64);
    P.end_sample = cfg.first_sample + cfg.samples;
    P.seed_lo = (uint32_t)cfg.seed; P.seed_hi = (uint32_t)(cfg.seed >> 32);
    P.key_base = key_base + (uint32_t)at;
    P.first_draw = cfg.first_draw;
    P.switch_below = s->switch_below;
    P.mode = cfg.reserved;
    const char* points_at = (const char*)points_dev + at * sizeof(SolRay);
    const char* keys_at = keys_dev ? (const char*)keys_dev + at * sizeof(SolRayKey) : nullptr;
    char* out_at = (char*)out_dev + at * texels * sizeof(SolOctTexel);
    const size_t words = (size_t)P.n_groups * 64 * std::min<size_t>(win_chunks * SOL_CHUNK, cfg.samples);
    if ((rc = s->rad_partial.reserve(s->stream, (words + 3) / 4))) return rc;  // (four words to a row of the buffer)
    for (size_t c0 = 0; c0 < total_chunks; c0 += win_chunks) {
      P.n_chunks = (uint32_t)std::min(win_chunks, total_chunks - c0);
      P.first_sample = cfg.first_sample + (uint32_t)(c0 * SOL_CHUNK);
      const uint32_t win_samples = std::min<uint32_t>(P.n_chunks * (uint32_t)SOL_CHUNK, P.end_sample - P.first_sample);  // (the call's last chunk may be short)
      const uint64_t items = (uint64_t)win_samples * P.n_groups * 64u;  // (<= 2^31 words of the partial buffer)
      P.n_items = (uint32_t)items;
      uint32_t grid;
      if ((rc = sol_launch_plan(s, bpc, items, SOL_LDS_STACK, s->tree.depth, s->rad_spill, &grid))) return rc;
      P.total_threads = grid * SOL_WG;
      HIP_TRY(hipMemsetAsync(s->rad_work.get(), 0, sizeof(uint32_t), s->stream));
      HIP_TRY(sol_launch_depth_each(s->mirror.dev.get(), P, may_spill, s->strict_triangles, points_at, keys_at, s->rad_partial.get(), s->rad_work.get(),
                                    s->rad_spill.get(), grid, s->stream));
      HIP_TRY(sol_launch_depth_project(P, s->depth_project_plain, oct.res, oct.sharpness_log2, points_at, keys_at, s->rad_partial.get(), out_at, win_samples, c0 != 0,
                                       s->stream));
    }
  }
  return SOL_OK;
}
}  // namespace

extern "C" {

int sol_visibility_oct_dev(SolScene* s, const void* points_dev, const void* keys_dev, size_t n, const SolIrradianceConfig* config, const SolOctConfig* oct,
                           void* out_dev) {
  int rc;
  bool go;
  SolRadianceConfig cfg{};
  if ((rc = gather_check(s, "sol_visibility_oct_dev", points_dev, n, config, &cfg, oct, out_dev, &go)) || !go || (rc = device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  return gather_launch(s, points_dev, keys_dev, n, cfg, cfg.key_base, *oct, out_dev);
}

int sol_visibility_oct(SolScene* s, const SolRay* points, const SolRayKey* keys, size_t n, const SolIrradianceConfig* config, const SolOctConfig* oct,
                       SolOctTexel* out) {
  int rc;
  bool go;
  SolRadianceConfig cfg{};
  if ((rc = gather_check(s, "sol_visibility_oct", points, n, config, &cfg, oct, out, &go)) || !go || (rc = device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  // radiance_staged's buffers (sol_api.cpp), the answers' staging grown to the res x res rows of a point's map
  const size_t texels = (size_t)oct->res * oct->res;
  const size_t cap = std::min(n, std::max<size_t>(1, DEPTH_STAGE_TEXELS / texels));
  if ((rc = s->rad_in.reserve(s->stream, cap)) || (rc = s->rad_keys.reserve(s->stream, cap)) || (rc = s->rad_out.reserve(s->stream, cap * texels))) return rc;
  for (size_t at = 0; at < n; at += cap) {  // (answers are per point: the split changes nothing)
    const size_t k = std::min(cap, n - at);
    HIP_TRY(hipMemcpyAsync(s->rad_in.get(), points + at, k * sizeof(SolRay), hipMemcpyHostToDevice, s->stream));
    if (keys) HIP_TRY(hipMemcpyAsync(s->rad_keys.get(), keys + at, k * sizeof(SolRayKey), hipMemcpyHostToDevice, s->stream));
    if ((rc = gather_launch(s, s->rad_in.get(), keys ? s->rad_keys.get() : nullptr, k, cfg, cfg.key_base + (uint32_t)at, *oct, s->rad_out.get()))) return rc;
    HIP_TRY(hipMemcpyAsync(out + at * texels, s->rad_out.get(), k * texels * sizeof(SolOctTexel), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  return SOL_OK;
}

int sol_volume_build_depth_dev(SolScene* s, const SolVolumeGrid* grid, const void* oct_dev, const SolOctConfig* oct, float radius, void* depth_out_dev) {
  int rc;
  if ((rc = build_check(s != nullptr, "sol_volume_build_depth_dev", grid, oct_dev, oct, radius, depth_out_dev)) || (rc = device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(sol_launch_depth_build((uint64_t)probes_of(*grid) * oct->res * oct->res, oct_dev, radius, depth_out_dev, s->stream));
  return SOL_OK;
}

int sol_volume_build_depth(SolScene* s, const SolVolumeGrid* grid, const SolOctTexel* oct_rows, const SolOctConfig* oct, float radius, SolDepthTexel* depth_out) {
  int rc;
  if ((rc = build_check(s != nullptr, "sol_volume_build_depth", grid, oct_rows, oct, radius, depth_out)) || (rc = device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const size_t n = probes_of(*grid) * oct->res * oct->res;
  Stage st;
  const size_t at_in = st.add(n * sizeof(SolOctTexel)), at_out = st.add(n * sizeof(SolDepthTexel));
  if ((rc = s->vol_stage.reserve(s->stream, st.total))) return rc;
  char* base = s->vol_stage.get();
  HIP_TRY(hipMemcpyAsync(base + at_in, oct_rows, n * sizeof(SolOctTexel), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(sol_launch_depth_build((uint64_t)n, base + at_in, radius, base + at_out, s->stream));
  HIP_TRY(hipMemcpyAsync(depth_out, base + at_out, n * sizeof(SolDepthTexel), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}

int sol_volume_sample_depth_dev(SolScene* s, const SolVolumeGrid* grid, const void* probes_dev, const void* depth_dev, const SolOctConfig* oct, const void* points_dev,
                                size_t n, void* out_dev) {
  int rc;
  if ((rc = sample_check(s != nullptr, "sol_volume_sample_depth_dev", grid, probes_dev, depth_dev, oct, points_dev, n, out_dev))) return rc;
  if (n == 0) return SOL_OK;
  if ((rc = device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(sol_launch_volume_sample_depth(*grid, probes_dev, depth_dev, oct->res, points_dev, (uint32_t)n, out_dev, s->stream));
  return SOL_OK;
}

int sol_volume_sample_depth(SolScene* s, const SolVolumeGrid* grid, const SolProbe* probes, const SolDepthTexel* depth, const SolOctConfig* oct, const SolRay* points,
                            size_t n, SolRadiance* out) {
  int rc;
  if ((rc = sample_check(s != nullptr, "sol_volume_sample_depth", grid, probes, depth, oct, points, n, out))) return rc;
  if (n == 0) return SOL_OK;
  if ((rc = device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const size_t np = probes_of(*grid), nt = np * oct->res * oct->res;
  Stage st;
  const size_t at_probes = st.add(np * sizeof(SolProbe)), at_depth = st.add(nt * sizeof(SolDepthTexel)), at_points = st.add(n * sizeof(SolRay)),
               at_out = st.add(n * sizeof(SolRadiance));
  if ((rc = s->vol_stage.reserve(s->stream, st.total))) return rc;
  char* base = s->vol_stage.get();
  HIP_TRY(hipMemcpyAsync(base + at_probes, probes, np * sizeof(SolProbe), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(base + at_depth, depth, nt * sizeof(SolDepthTexel), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(base + at_points, points, n * sizeof(SolRay), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(sol_launch_volume_sample_depth(*grid, base + at_probes, base + at_depth, oct->res, base + at_points, (uint32_t)n, base + at_out, s->stream));
  HIP_TRY(hipMemcpyAsync(out, base + at_out, n * sizeof(SolRadiance), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}

}  // extern "C"
