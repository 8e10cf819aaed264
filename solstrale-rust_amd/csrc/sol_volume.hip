// sol_volume.hip -- irradiance volumes: a probe grid laid out, packed and sampled on the device (sol_volume_points, sol_volume_build,
// sol_volume_sample; sol_volume.cpp). The rule is sol_volume.h; the kernels only fetch, call it and store.
//
//   sol_volume_points_kernel  a thread per probe: the point row (position, tmin, (0, 0, 1), tmax), two dwordx4 stores.
//   sol_volume_build_kernel   a thread per probe: seven dwordx4 of an SolSh9 row and (where given) two of a SolVisibility row in, eight dwordx4 out.
//   sol_volume_sample_kernel  a lane per point: two dwordx4 in, one out, and per corner of the cell that has weight the probe's eight dwordx4,
//                             issued together before the first is used (vol_load_probe pins them; the listing shows eight loads and one wait).
//                             The corners themselves follow one another: a corner's loads are not in flight while the one before it is
//                             summed. No LDS, no scratch, no atomics; the corners are added in the order dz, dy, dx by the one lane, so the
//                             answer does not depend on the schedule.
// The sampler is a gather with little arithmetic: 48 bytes of its own per point and up to 1 KiB of probes that neighbouring points share. Its
// one template parameter is the measured alternative: LOAD_ALL = true fetches all eight corners without looking at the weight (no branch in
// front of the loads; a zero-weight corner is still left out of the sums, so the words are the same). profiles/volume.txt has both.
#include <hip/hip_runtime.h>

#include "../../include/solstrale_hip.h"
#include "sol_launch.h"
#include "sol_volume.h"

#define VOL_WG 256

static_assert(sizeof(SolProbe) == 128 && sizeof(SolVolumeGrid) == 48, "the records of include/solstrale_hip.h");

namespace {
DEV void vol_load_probe(const uint32_t* probes, uint32_t row, uint32_t (&e)[32]) {
  const SOL_AS1 sol_v4u* p = (const SOL_AS1 sol_v4u*)(probes + (size_t)row * 32);
  sol_v4u v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = p[k];
  // All eight are issued here: the empty statement takes the eight values as operands, and the compiler may not sink it into the branch on the
  // probe's valid bit. Without it four of the loads wait behind that bit - a second round of memory latency per corner (profiles/volume.txt 3).
  asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]));
#pragma unroll
  for (int k = 0; k < 8; ++k) { e[4 * k] = v[k].x; e[4 * k + 1] = v[k].y; e[4 * k + 2] = v[k].z; e[4 * k + 3] = v[k].w; }
}
}  // namespace

__global__ __launch_bounds__(VOL_WG) void sol_volume_points_kernel(VolGrid G, uint32_t n_probes, float tmin, float tmax, float* __restrict__ points) {
  const uint32_t x = blockIdx.x * VOL_WG + threadIdx.x;
  if (x >= n_probes) return;
  const uint32_t i = x % G.n[0], jk = x / G.n[0], j = jk % G.n[1], k = jk / G.n[1];
  const f3 at = vol_probe_position(G, i, j, k);
  SOL_AS1 sol_v4f* p = (SOL_AS1 sol_v4f*)(points + (size_t)x * 8);
  p[0] = sol_v4f{at.x, at.y, at.z, tmin};
  p[1] = sol_v4f{0.0f, 0.0f, 1.0f, tmax};
}

__global__ __launch_bounds__(VOL_WG) void sol_volume_build_kernel(uint32_t n_probes, const uint32_t* __restrict__ sh, const uint32_t* __restrict__ visibility,
                                                                  float radius, uint32_t* __restrict__ probes) {
  const uint32_t x = blockIdx.x * VOL_WG + threadIdx.x;
  if (x >= n_probes) return;
  uint32_t in[28], vis[8], out[32];
  const SOL_AS1 sol_v4u* s = (const SOL_AS1 sol_v4u*)(sh + (size_t)x * 28);
#pragma unroll
  for (int k = 0; k < 7; ++k) { const sol_v4u v = s[k]; in[4 * k] = v.x; in[4 * k + 1] = v.y; in[4 * k + 2] = v.z; in[4 * k + 3] = v.w; }
  if (visibility) {
    const SOL_AS1 sol_v4u* t = (const SOL_AS1 sol_v4u*)(visibility + (size_t)x * 8);
#pragma unroll
    for (int k = 0; k < 2; ++k) { const sol_v4u v = t[k]; vis[4 * k] = v.x; vis[4 * k + 1] = v.y; vis[4 * k + 2] = v.z; vis[4 * k + 3] = v.w; }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) vis[k] = 0u;  // (samples == 0: no moments)
  }
  vol_build(in, vis, radius, out);
  SOL_AS1 sol_v4u* p = (SOL_AS1 sol_v4u*)(probes + (size_t)x * 32);
#pragma unroll
  for (int k = 0; k < 8; ++k) p[k] = sol_v4u{out[4 * k], out[4 * k + 1], out[4 * k + 2], out[4 * k + 3]};
}

template <bool LOAD_ALL>
__global__ __launch_bounds__(VOL_WG) void sol_volume_sample_kernel(VolGrid G, const uint32_t* __restrict__ probes, const float* __restrict__ points, uint32_t n,
                                                                   uint32_t* __restrict__ out) {
  const uint32_t x = blockIdx.x * VOL_WG + threadIdx.x;
  if (x >= n) return;
  const SOL_AS1 sol_v4f* row = (const SOL_AS1 sol_v4f*)(points + (size_t)x * 8);
  const sol_v4f r0 = row[0], r1 = row[1];
  sol_v4u answer = {0u, 0u, 0u, 0u};
  VolPoint P;
  if (vol_setup(G, r0, r1, P)) {
    float sum[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f;
    uint32_t samples = 0u;
#pragma unroll
    for (uint32_t c = 0; c < 8u; ++c) {
      const float w = vol_trilinear(P, c);
      if (!LOAD_ALL && w == 0.0f) continue;
      // (the far layer of a one-probe axis and of a point on the last plane has weight zero; its index stays inside the grid all the same)
      const uint32_t i = min(P.i0[0] + (c & 1u), G.n[0] - 1u), j = min(P.i0[1] + ((c >> 1) & 1u), G.n[1] - 1u), k = min(P.i0[2] + (c >> 2), G.n[2] - 1u);
      uint32_t e[32];
      vol_load_probe(probes, (k * G.n[1] + j) * G.n[0] + i, e);
      if (LOAD_ALL && w == 0.0f) continue;
      vol_corner(G, P, w, vol_probe_position(G, i, j, k), e, sum, wsum, samples);
    }
    if (samples != 0u) answer = sol_v4u{__float_as_uint(sum[0] / wsum), __float_as_uint(sum[1] / wsum), __float_as_uint(sum[2] / wsum), samples};
  }
  *(SOL_AS1 sol_v4u*)(out + (size_t)x * 4) = answer;
}

// ---- launches (sol_launch.h) ----
namespace {
VolGrid vol_grid(const SolVolumeGrid& g) {
  return VolGrid{{g.nx, g.ny, g.nz}, {g.origin[0], g.origin[1], g.origin[2]}, {g.spacing[0], g.spacing[1], g.spacing[2]}, g.flags, g.normal_bias};
}
}  // namespace

hipError_t sol_launch_volume_points(const SolVolumeGrid& grid, float tmin, float tmax, void* points, hipStream_t stream) {
  const uint32_t n = grid.nx * grid.ny * grid.nz;
  hipLaunchKernelGGL(sol_volume_points_kernel, dim3((n + VOL_WG - 1) / VOL_WG), dim3(VOL_WG), 0, stream, vol_grid(grid), n, tmin, tmax, (float*)points);
  return hipGetLastError();
}
hipError_t sol_launch_volume_build(uint32_t n_probes, const void* sh, const void* visibility, float radius, void* probes, hipStream_t stream) {
  hipLaunchKernelGGL(sol_volume_build_kernel, dim3((n_probes + VOL_WG - 1) / VOL_WG), dim3(VOL_WG), 0, stream, n_probes, (const uint32_t*)sh,
                     (const uint32_t*)visibility, radius, (uint32_t*)probes);
  return hipGetLastError();
}
hipError_t sol_launch_volume_sample(const SolVolumeGrid& grid, bool load_all, const void* probes, const void* points, uint32_t n, void* out, hipStream_t stream) {
  const dim3 blocks((uint32_t)(((uint64_t)n + VOL_WG - 1) / VOL_WG));
  if (load_all)
    hipLaunchKernelGGL(sol_volume_sample_kernel<true>, blocks, dim3(VOL_WG), 0, stream, vol_grid(grid), (const uint32_t*)probes, (const float*)points, n, (uint32_t*)out);
  else
    hipLaunchKernelGGL(sol_volume_sample_kernel<false>, blocks, dim3(VOL_WG), 0, stream, vol_grid(grid), (const uint32_t*)probes, (const float*)points, n, (uint32_t*)out);
  return hipGetLastError();
}
