// sol_volume.cpp -- sol_volume_points, sol_volume_build and sol_volume_sample (include/solstrale_hip.h): a probe grid laid out, packed
// and sampled on the device (kernels: sol_volume.hip; the rule: sol_volume.h). The handle supplies the device, the stream and the staging of the
// host routes (SolScene::vol_stage); the scene itself is not read: nothing is traced. Every refusal is decided before the device is looked for,
// from the arguments alone - the checks below are not given the handle's contents, only whether there is one.
#include <cmath>

#include "sol_scene.h"

namespace {
constexpr size_t VOL_MAX_POINTS = (size_t)1 << 31;

// what all three calls refuse, in the header's order
int grid_check(bool have_scene, const char* fn, const SolVolumeGrid* g) {
  if (!have_scene || !g) return sol_fail(SOL_EINVAL, "%s: null %s", fn, !have_scene ? "scene" : "grid");
  if (g->size != sizeof(SolVolumeGrid)) return sol_fail(SOL_EINVAL, "%s: SolVolumeGrid.size %u (expected %zu)", fn, g->size, sizeof(SolVolumeGrid));
  if (g->flags & ~(SOL_VOLUME_BACKFACE | SOL_VOLUME_CHEBYSHEV)) return sol_fail(SOL_EINVAL, "%s: SolVolumeGrid.flags 0x%x: unknown bits", fn, g->flags);
  if (g->nx == 0 || g->ny == 0 || g->nz == 0) return sol_fail(SOL_EINVAL, "%s: a grid of %u x %u x %u probes (at least 1 each way)", fn, g->nx, g->ny, g->nz);
  if ((uint64_t)g->nx * g->ny > SOL_VOLUME_MAX_PROBES || (uint64_t)g->nx * g->ny * g->nz > SOL_VOLUME_MAX_PROBES)  // (nx * ny <= 2^24: the product of three fits 64 bits)
    return sol_fail(SOL_EINVAL, "%s: %u x %u x %u probes (at most 2^24 in all)", fn, g->nx, g->ny, g->nz);
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(g->origin[a])) return sol_fail(SOL_EINVAL, "%s: origin[%d] %g is not finite", fn, a, (double)g->origin[a]);
  const uint32_t count[3] = {g->nx, g->ny, g->nz};
  for (int a = 0; a < 3; ++a)
    if (count[a] > 1 && !(std::isfinite(g->spacing[a]) && g->spacing[a] > 0.0f))
      return sol_fail(SOL_EINVAL, "%s: spacing[%d] %g (finite and > 0 on an axis with more than one probe)", fn, a, (double)g->spacing[a]);
  if (!std::isfinite(g->normal_bias)) return sol_fail(SOL_EINVAL, "%s: normal_bias %g is not finite", fn, (double)g->normal_bias);
  return SOL_OK;
}
int points_check(bool have_scene, const char* fn, const SolVolumeGrid* g, float tmin, float tmax, const void* points) {
  if (const int rc = grid_check(have_scene, fn, g)) return rc;
  if (!(std::isfinite(tmin) && tmin >= 0.0f && tmin <= tmax))
    return sol_fail(SOL_EINVAL, "%s: tmin %g, tmax %g (0 <= tmin <= tmax, tmin finite, tmax not NaN)", fn, (double)tmin, (double)tmax);
  if (!points) return sol_fail(SOL_EINVAL, "%s: null point output pointer", fn);
  return SOL_OK;
}
int build_check(bool have_scene, const char* fn, const SolVolumeGrid* g, const void* sh, const void* probes) {
  if (const int rc = grid_check(have_scene, fn, g)) return rc;
  if (!sh) return sol_fail(SOL_EINVAL, "%s: null SolSh9 pointer", fn);
  if (!probes) return sol_fail(SOL_EINVAL, "%s: null probe output pointer", fn);
  return SOL_OK;
}
int sample_check(bool have_scene, const char* fn, const SolVolumeGrid* g, const void* probes, const void* points, size_t n, const void* out) {
  if (const int rc = grid_check(have_scene, fn, g)) return rc;
  if (n > VOL_MAX_POINTS) return sol_fail(SOL_EINVAL, "%s: %zu points in one call (at most 2^31)", fn, n);
  if (n > 0 && (!probes || !points || !out)) return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !probes ? "probe" : !points ? "point" : "output");
  return SOL_OK;
}
}  // namespace
int sol_volume_grid_check(bool have_scene, const char* fn, const SolVolumeGrid* g) { return grid_check(have_scene, fn, g); }  // (sol_scene.h: for sol_depth.cpp)
namespace {
size_t probes_of(const SolVolumeGrid& g) { return (size_t)g.nx * g.ny * g.nz; }

}  // namespace

extern "C" {

int sol_volume_points_dev(SolScene* s, const SolVolumeGrid* grid, float tmin, float tmax, void* points_out_dev) {
  int rc;
  if ((rc = points_check(s != nullptr, "sol_volume_points_dev", grid, tmin, tmax, points_out_dev)) || (rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(sol_launch_volume_points(*grid, tmin, tmax, points_out_dev, s->stream));
  return SOL_OK;
}

int sol_volume_points(SolScene* s, const SolVolumeGrid* grid, float tmin, float tmax, SolRay* points_out) {
  int rc;
  if ((rc = points_check(s != nullptr, "sol_volume_points", grid, tmin, tmax, points_out)) || (rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const size_t bytes = probes_of(*grid) * sizeof(SolRay);
  if ((rc = s->vol_stage.reserve(s->stream, bytes))) return rc;
  HIP_TRY(sol_launch_volume_points(*grid, tmin, tmax, s->vol_stage.get(), s->stream));
  HIP_TRY(hipMemcpyAsync(points_out, s->vol_stage.get(), bytes, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}

int sol_volume_build_dev(SolScene* s, const SolVolumeGrid* grid, const void* sh_dev, const void* visibility_dev, float radius, void* probes_out_dev) {
  int rc;
  if ((rc = build_check(s != nullptr, "sol_volume_build_dev", grid, sh_dev, probes_out_dev)) || (rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(sol_launch_volume_build((uint32_t)probes_of(*grid), sh_dev, visibility_dev, radius, probes_out_dev, s->stream));
  return SOL_OK;
}

int sol_volume_build(SolScene* s, const SolVolumeGrid* grid, const SolSh9* sh, const SolVisibility* visibility, float radius, SolProbe* probes_out) {
  int rc;
  if ((rc = build_check(s != nullptr, "sol_volume_build", grid, sh, probes_out)) || (rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const size_t n = probes_of(*grid);
  SolStage st;
  const size_t at_sh = st.add(n * sizeof(SolSh9)), at_vis = st.add(visibility ? n * sizeof(SolVisibility) : 0), at_out = st.add(n * sizeof(SolProbe));
  if ((rc = s->vol_stage.reserve(s->stream, st.total))) return rc;
  char* base = s->vol_stage.get();
  HIP_TRY(hipMemcpyAsync(base + at_sh, sh, n * sizeof(SolSh9), hipMemcpyHostToDevice, s->stream));
  if (visibility) HIP_TRY(hipMemcpyAsync(base + at_vis, visibility, n * sizeof(SolVisibility), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(sol_launch_volume_build((uint32_t)n, base + at_sh, visibility ? base + at_vis : nullptr, radius, base + at_out, s->stream));
  HIP_TRY(hipMemcpyAsync(probes_out, base + at_out, n * sizeof(SolProbe), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}

int sol_volume_sample_dev(SolScene* s, const SolVolumeGrid* grid, const void* probes_dev, const void* points_dev, size_t n, void* out_dev) {
  int rc;
  if ((rc = sample_check(s != nullptr, "sol_volume_sample_dev", grid, probes_dev, points_dev, n, out_dev))) return rc;
  if (n == 0) return SOL_OK;
  if ((rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(sol_launch_volume_sample(*grid, s->vol_load_all, probes_dev, points_dev, (uint32_t)n, out_dev, s->stream));
  return SOL_OK;
}

int sol_volume_sample(SolScene* s, const SolVolumeGrid* grid, const SolProbe* probes, const SolRay* points, size_t n, SolRadiance* out) {
  int rc;
  if ((rc = sample_check(s != nullptr, "sol_volume_sample", grid, probes, points, n, out))) return rc;
  if (n == 0) return SOL_OK;
  if ((rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const size_t np = probes_of(*grid);
  SolStage st;
  const size_t at_probes = st.add(np * sizeof(SolProbe)), at_points = st.add(n * sizeof(SolRay)), at_out = st.add(n * sizeof(SolRadiance));
  if ((rc = s->vol_stage.reserve(s->stream, st.total))) return rc;
  char* base = s->vol_stage.get();
  HIP_TRY(hipMemcpyAsync(base + at_probes, probes, np * sizeof(SolProbe), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(base + at_points, points, n * sizeof(SolRay), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(sol_launch_volume_sample(*grid, s->vol_load_all, base + at_probes, base + at_points, (uint32_t)n, base + at_out, s->stream));
  HIP_TRY(hipMemcpyAsync(out, base + at_out, n * sizeof(SolRadiance), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}

}  // extern "C"
