// sol_volume.cpp -- sol_volume_points, sol_volume_build and sol_volume_sample (include/solstrale_hip.h): a probe grid laid out, packed
// and sampled on the device (kernels: sol_volume.hip; the rule: sol_volume.h). The handle supplies the device, the stream and the staging of the
// host routes (SolScene::vol_stage through SolStaged, sol_stage.h; sol_volume_points has one array and no layout); the scene itself is not read:
// nothing is traced. Every refusal is decided before the device is looked for, from the arguments alone - the checks below are not given the
// handle's contents, only whether there is one.
#include <cmath>

#include "sol_bake_checks.h"
#include "sol_stage.h"

namespace {
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
  if (const int rc = sol_rows_check(fn, n, "points")) return rc;
  if (n > 0 && (!probes || !points || !out)) return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !probes ? "probe" : !points ? "point" : "output");
  return SOL_OK;
}
size_t probes_of(const SolVolumeGrid& g) { return (size_t)g.nx * g.ny * g.nz; }

int build_launch(SolScene* s, size_t n_probes, const void* sh, const void* visibility, float radius, void* probes) {
  HIP_TRY(sol_launch_volume_build((uint32_t)n_probes, sh, visibility, radius, probes, s->stream));
  return SOL_OK;
}
int sample_launch(SolScene* s, const SolVolumeGrid& g, const void* probes, const void* points, size_t n, void* out) {
  HIP_TRY(sol_launch_volume_sample(g, s->vol_load_all, probes, points, (uint32_t)n, out, s->stream));
  return SOL_OK;
}
}  // namespace
int sol_volume_grid_check(bool have_scene, const char* fn, const SolVolumeGrid* g) { return grid_check(have_scene, fn, g); }  // (sol_scene.h: for sol_depth.cpp)

extern "C" {

int sol_volume_points_dev(SolScene* s, const SolVolumeGrid* grid, float tmin, float tmax, void* points_out_dev) {
  int rc;
  if ((rc = points_check(s != nullptr, "sol_volume_points_dev", grid, tmin, tmax, points_out_dev)) || (rc = sol_device_enter(s))) return rc;
  HIP_TRY(sol_launch_volume_points(*grid, tmin, tmax, points_out_dev, s->stream));
  return SOL_OK;
}

int sol_volume_points(SolScene* s, const SolVolumeGrid* grid, float tmin, float tmax, SolRay* points_out) {
  int rc;
  if ((rc = points_check(s != nullptr, "sol_volume_points", grid, tmin, tmax, points_out)) || (rc = sol_device_enter(s))) return rc;
  const size_t bytes = probes_of(*grid) * sizeof(SolRay);  // (one output and nothing to lay out: exactly its bytes are reserved, without SolStaged's rounding)
  if ((rc = s->vol_stage.reserve(s->stream, bytes))) return rc;
  HIP_TRY(sol_launch_volume_points(*grid, tmin, tmax, s->vol_stage.get(), s->stream));
  HIP_TRY(hipMemcpyAsync(points_out, s->vol_stage.get(), bytes, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}

int sol_volume_build_dev(SolScene* s, const SolVolumeGrid* grid, const void* sh_dev, const void* visibility_dev, float radius, void* probes_out_dev) {
  int rc;
  if ((rc = build_check(s != nullptr, "sol_volume_build_dev", grid, sh_dev, probes_out_dev)) || (rc = sol_device_enter(s))) return rc;
  return build_launch(s, probes_of(*grid), sh_dev, visibility_dev, radius, probes_out_dev);
}

int sol_volume_build(SolScene* s, const SolVolumeGrid* grid, const SolSh9* sh, const SolVisibility* visibility, float radius, SolProbe* probes_out) {
  int rc;
  if ((rc = build_check(s != nullptr, "sol_volume_build", grid, sh, probes_out)) || (rc = sol_device_enter(s))) return rc;
  const size_t n = probes_of(*grid);
  SolStaged st(s->stream, s->vol_stage);
  const int h = st.in(sh, n * sizeof(SolSh9)), vis = st.in_opt(visibility, n * sizeof(SolVisibility)), o = st.out(probes_out, n * sizeof(SolProbe));
  if ((rc = st.upload()) || (rc = build_launch(s, n, st[h], st[vis], radius, st[o]))) return rc;
  return st.finish();
}

int sol_volume_sample_dev(SolScene* s, const SolVolumeGrid* grid, const void* probes_dev, const void* points_dev, size_t n, void* out_dev) {
  int rc;
  if ((rc = sample_check(s != nullptr, "sol_volume_sample_dev", grid, probes_dev, points_dev, n, out_dev)) || n == 0 || (rc = sol_device_enter(s))) return rc;
  return sample_launch(s, *grid, probes_dev, points_dev, n, out_dev);
}

int sol_volume_sample(SolScene* s, const SolVolumeGrid* grid, const SolProbe* probes, const SolRay* points, size_t n, SolRadiance* out) {
  int rc;
  if ((rc = sample_check(s != nullptr, "sol_volume_sample", grid, probes, points, n, out)) || n == 0 || (rc = sol_device_enter(s))) return rc;
  SolStaged st(s->stream, s->vol_stage);
  const int pr = st.in(probes, probes_of(*grid) * sizeof(SolProbe)), p = st.in(points, n * sizeof(SolRay)), o = st.out(out, n * sizeof(SolRadiance));
  if ((rc = st.upload()) || (rc = sample_launch(s, *grid, st[pr], st[p], n, st[o]))) return rc;
  return st.finish();
}

}  // extern "C"
