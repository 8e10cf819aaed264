// sol_lightmap_unwrap.cpp -- sol_lightmap_unwrap and sol_lightmap_unwrap_dev (include/solstrale_hip.h): the charts of a mesh
// projected along their dominant axes and packed into an atlas (kernels: sol_lightmap_unwrap.hip; the rule: sol_lightmap_unwrap.h). There is no
// handle: the call names its device, allocates its scratch (and, on the host route, the copies of its arrays), waits for the stream and frees
// them - both routes block. Every refusal is decided before the device is looked for, from the arguments alone (the shared sentences:
// sol_bake_checks.h; the 2^30 triangles are the charts family's).
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "sol_bake_checks.h"

namespace {
// SOL_LIGHTMAP_UNWRAP=collide: the edge hash masked to 4 bits, the tested worst case of the match (the same words); =stages: the stages of
// the call timed by device events for sol_lightmap_unwrap_stage_ms (tests/tools/lightmap_unwrap_bench.py)
bool unwrap_mode(const char* mode) {
  const char* e = std::getenv("SOL_LIGHTMAP_UNWRAP");
  return e && std::strcmp(e, mode) == 0;
}
thread_local float stage_ms[SOL_LU_STAGES + 1] = {};  // the calling thread's last timed call: the stages, then all of them

int unwrap_check(const char* fn, const SolUnwrapConfig* c, const void* vertices, size_t n, const void* uvs, const void* chart_of, const void* result) {
  int rc;
  if (!c) return sol_fail(SOL_EINVAL, "%s: null configuration", fn);
  if ((rc = sol_config_head_check(fn, "SolUnwrapConfig", *c, c->flags, 0u))) return rc;
  if ((rc = sol_atlas_check(fn, c->width, c->height))) return rc;
  if (c->gutter > SOL_UNWRAP_MAX_GUTTER) return sol_fail(SOL_EINVAL, "%s: a gutter of %u texels (at most %u)", fn, c->gutter, SOL_UNWRAP_MAX_GUTTER);
  if (!(std::isfinite(c->texels_per_unit) && c->texels_per_unit > 0.0f))
    return sol_fail(SOL_EINVAL, "%s: texels_per_unit %g (finite, > 0)", fn, (double)c->texels_per_unit);
  if (!(c->crease_cos >= -1.0f && c->crease_cos <= 1.0f)) return sol_fail(SOL_EINVAL, "%s: crease_cos %g (-1 .. 1)", fn, (double)c->crease_cos);
  if (n > SOL_LIGHTMAP_CHARTS_MAX_TRIANGLES) return sol_fail(SOL_EINVAL, "%s: %zu triangles in one call (at most 2^30)", fn, n);
  if (n > 0 && (!vertices || !uvs || !chart_of))
    return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !vertices ? "vertex" : !uvs ? "UV output" : "label output");
  if (!result) return sol_fail(SOL_EINVAL, "%s: null result pointer", fn);
  return SOL_OK;
}

// The unwrap of n triangles on `stream` over device arrays: the scratch of the call is allocated here and freed after the stream was waited for.
int unwrap_run(hipStream_t stream, const SolUnwrapConfig& c, const void* vertices, size_t n_triangles, void* uvs, void* chart_of, void* result) {
  const uint32_t n = (uint32_t)n_triangles;
  LuScratch S{};
  S.words = 16;
  if (n) HIP_TRY(sol_lightmap_unwrap_scratch(n, S));
  DevPtr<uint32_t> scratch;
  if (sol_dev_alloc(scratch, S.words) != hipSuccess) return sol_fail(SOL_ENOMEM, "sol_lightmap_unwrap: hipMalloc of %zu scratch bytes failed", S.words * 4);
  hipEvent_t ev[SOL_LU_STAGES + 1] = {};
  const bool timed = n != 0 && unwrap_mode("stages");
  if (timed)
    for (hipEvent_t& x : ev) HIP_TRY(hipEventCreate(&x));
  const hipError_t e = sol_launch_lightmap_unwrap(c, vertices, n, unwrap_mode("collide"), S, scratch.get(), uvs, chart_of, result, stream, timed ? ev : nullptr);
  const hipError_t w = hipStreamSynchronize(stream);  // (also after a failed launch: the scratch is freed below)
  if (timed) {
    if (e == hipSuccess && w == hipSuccess) {
      for (int k = 0; k < SOL_LU_STAGES; ++k) hipEventElapsedTime(&stage_ms[k], ev[k], ev[k + 1]);
      hipEventElapsedTime(&stage_ms[SOL_LU_STAGES], ev[0], ev[SOL_LU_STAGES]);
    }
    for (hipEvent_t x : ev) hipEventDestroy(x);
  }
  if (e != hipSuccess || w != hipSuccess) return sol_fail(SOL_EDEVICE, "sol_lightmap_unwrap: %s", hipGetErrorString(e != hipSuccess ? e : w));
  return SOL_OK;
}

int unwrap_enter(int device) {
  int n_devices = 0;
  if (const int rc = sol_device_check(&n_devices)) return rc;
  if (device < 0 || device >= n_devices) return sol_fail(SOL_EDEVICE, "sol_lightmap_unwrap: device %d of %d", device, n_devices);
  HIP_TRY(hipSetDevice(device));
  return SOL_OK;
}
}  // namespace

extern "C" {

int sol_lightmap_unwrap_stage_ms(float* stage_ms_out) {
  if (!stage_ms_out) return sol_fail(SOL_EINVAL, "sol_lightmap_unwrap_stage_ms: null output pointer");
  std::memcpy(stage_ms_out, stage_ms, sizeof(stage_ms));
  return SOL_OK;
}

int sol_lightmap_unwrap_dev(int device, void* hip_stream, const SolUnwrapConfig* config, const void* vertices_dev, size_t n_triangles, void* uvs_out_dev,
                            void* chart_of_triangle_out_dev, void* result_out_dev) {
  int rc;
  if ((rc = unwrap_check("sol_lightmap_unwrap_dev", config, vertices_dev, n_triangles, uvs_out_dev, chart_of_triangle_out_dev, result_out_dev)) ||
      (rc = unwrap_enter(device)))
    return rc;
  return unwrap_run((hipStream_t)hip_stream, *config, vertices_dev, n_triangles, uvs_out_dev, chart_of_triangle_out_dev, result_out_dev);
}

int sol_lightmap_unwrap(int device, const SolUnwrapConfig* config, const float* vertices, size_t n_triangles, float* uvs_out, uint32_t* chart_of_triangle_out,
                        SolUnwrapResult* result_out) {
  int rc;
  if ((rc = unwrap_check("sol_lightmap_unwrap", config, vertices, n_triangles, uvs_out, chart_of_triangle_out, result_out))) return rc;
  if (n_triangles == 0) {
    std::memset(result_out, 0, sizeof(SolUnwrapResult));
    return SOL_OK;
  }
  if ((rc = unwrap_enter(device))) return rc;
  const size_t nt = n_triangles;
  DevPtr<float> vx, uv;
  DevPtr<uint32_t> chart, result;
  if (sol_dev_alloc(vx, nt * 9) != hipSuccess || sol_dev_alloc(uv, nt * 6) != hipSuccess || sol_dev_alloc(chart, nt) != hipSuccess ||
      sol_dev_alloc(result, sizeof(SolUnwrapResult) / 4) != hipSuccess)
    return sol_fail(SOL_ENOMEM, "sol_lightmap_unwrap: hipMalloc of the staged arrays failed");
  HIP_TRY(hipMemcpy(vx.get(), vertices, nt * 9 * sizeof(float), hipMemcpyHostToDevice));
  if ((rc = unwrap_run(nullptr, *config, vx.get(), nt, uv.get(), chart.get(), result.get()))) return rc;
  HIP_TRY(hipMemcpy(uvs_out, uv.get(), nt * 6 * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(chart_of_triangle_out, chart.get(), nt * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(result_out, result.get(), sizeof(SolUnwrapResult), hipMemcpyDeviceToHost));
  return SOL_OK;
}

}  // extern "C"
