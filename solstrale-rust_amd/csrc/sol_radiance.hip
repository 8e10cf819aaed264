// sol_radiance.hip -- radiance queries (include/solstrale_hip.h, sol_radiance / sol_radiance_dev / sol_camera_ray_keys): the
// path-traced colour along the caller's own rays. A path starts from a SolRay instead of the camera and is then the render's path: the
// same search (sol_trace.h), the same vertex shading (shade_vertex, sol_path.h), the same RNG stream keyed by (seed, key, sample).
//
//  sol_radiance_kernel<SPILL, STRICT, ENV, LT, GATHER> -- the persistent-wave schedule of sol_wave.h around a service block of its own, as
//    sol_render_kernel is. A work item is (ray, chunk): the owning lane sums the chunk's samples in order and writes once - no float
//    atomic. Paths differ in length by two orders of magnitude (glass), so the run-to-completion schedule of sol_query_kernel is wrong here.
//  sol_radiance_resolve_kernel -- more than one chunk: adds a ray's chunk sums in chunk order, the association of sol_resolve_kernel.
//  sol_irradiance_rays_kernel -- irradiance queries are sol_radiance_kernel<.., GATHER>: the row is a point with its normal and every
//    sample draws a direction of its own (irradiance_direction, sol_ray.h) where a radiance path copies the caller's. This kernel writes, for
//    one sample, those rays and the keys the paths go on from.
//  sol_radiance_each_kernel, sol_sh_project_kernel -- SH irradiance queries: 27 sums do not fit beside a path, so the GATHER
//    kernel is built once more with EACH - a work item is (point, sample) and the lane writes the sample's colour to [sample][point] -, and one
//    thread per point then draws each sample's direction again, evaluates the basis (sol_sh.h) and adds in the render's association.
//  sol_camera_ray_keys_kernel -- the RNG key and the counter generate_path leaves behind for each pixel of a rectangle: with them a
//    radiance query over sol_camera_rays' rays is the render's own sample, bit for bit.
//
// The ray of an item is read when the item is taken (validity, first sample) and again at the start of each later sample (two dwordx4;
// the key, one dwordx2, at every sample: L2 hits after the first), and its upper end once more on the rare restart at depth 0, instead of
// living in ten registers beside the path: the kernels stay inside the 128 registers of four waves per SIMD without scratch, as the
// render's do.
#include <hip/hip_runtime.h>

#include "sol_launch.h"
#include "sol_ray.h"
#include "sol_sh.h"
#include "sol_wave.h"

namespace {

// tmax of ray `i` (the restarts at depth 0 keep the caller's upper end)
DEV float radiance_tmax(const float4* __restrict__ rays, uint32_t i) { return __uint_as_float(ldg_u32((const float*)(rays + (size_t)i * 2u + 1u) + 3)); }

DEV void radiance_store(sol_v4f* __restrict__ p, f3 sum, uint32_t w) {
  const sol_v4f v = {sum.x, sum.y, sum.z, __uint_as_float(w)};
  *(SOL_AS1 sol_v4f*)p = v;  // one dwordx4
}

}  // namespace

template <bool SPILL, bool STRICT, bool ENV, bool LT, bool GATHER>
__global__ void __launch_bounds__(SOL_WG, SOL_V1_MIN_WAVES)
sol_radiance_kernel(const DevScene* __restrict__ Sp, const RadianceParams P, const float4* __restrict__ rays, const uint2* __restrict__ keys,
                    sol_v4f* __restrict__ out, sol_v4f* __restrict__ partial, uint32_t* __restrict__ work_counter, uint32_t* __restrict__ spill) {
  constexpr bool EACH = false;
#include "sol_radiance_body.h"
}

// The GATHER instances once more with EACH set, under a name of their own: the twenty instances above keep theirs (and with them every
// instruction, tests/test_irradiance_abi.py counts them by name).
template <bool SPILL, bool STRICT, bool ENV, bool LT>
__global__ void __launch_bounds__(SOL_WG, SOL_V1_MIN_WAVES)
sol_radiance_each_kernel(const DevScene* __restrict__ Sp, const RadianceParams P, const float4* __restrict__ rays, const uint2* __restrict__ keys,
                         sol_v4f* __restrict__ out, sol_v4f* __restrict__ partial, uint32_t* __restrict__ work_counter, uint32_t* __restrict__ spill) {
  constexpr bool GATHER = true, EACH = true;
#include "sol_radiance_body.h"
}

// One thread per ray of a launch with more than one chunk (or one window of a longer sample range): the chunk sums in chunk order on top
// of 0 - or, `accumulate`, of what the earlier windows of the same call left in `out` -, ((0 + c0) + c1) + ..: sol_resolve_kernel's
// association. An invalid ray answers (0, 0, 0, samples = 0).
__global__ void __launch_bounds__(256) sol_radiance_resolve_kernel(const RadianceParams P, const float4* __restrict__ rays, const sol_v4f* __restrict__ partial,
                                                                   sol_v4f* __restrict__ out, uint32_t samples, uint32_t accumulate) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= P.n_rays) return;
  if (!query_ray_valid(ldg_f4(rays + (size_t)i * 2u), ldg_f4(rays + (size_t)i * 2u + 1u))) {
    radiance_store(out + i, mk3(0.f, 0.f, 0.f), 0u);
    return;
  }
  f3 sum = mk3(0.f, 0.f, 0.f);
  if (accumulate) {
    const sol_v4f o = *(const SOL_AS1 sol_v4f*)(out + i);
    sum = mk3(o.x, o.y, o.z);
  }
  for (uint32_t k = 0; k < P.n_chunks; ++k) {
    const sol_v4f c = *(const SOL_AS1 sol_v4f*)(partial + (size_t)k * (P.n_groups * 64u) + i);
    sum = sum + mk3(c.x, c.y, c.z);
  }
  radiance_store(out + i, sum, samples);
}

// One thread per pixel of [x0, x0 + w) x [y0, y0 + h), row-major: generate_path's RNG key (row * W + x) and the counter it leaves
// behind - 2 for a pinhole, 2 + twice the rejection rounds of the lens disc for a thin lens.
__global__ void __launch_bounds__(256) sol_camera_ray_keys_kernel(const DevScene* __restrict__ Sp, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                                                  uint32_t sample, uint32_t seed_lo, uint32_t seed_hi, uint2* __restrict__ keys) {
  const DevScene& S = *Sp;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;  // (w * h <= 2^31: checked by the caller)
  if (i >= w * h) return;
  const uint32_t y = i / w, x = i - y * w;
  Path p = {};
  Counters cnt = {};
  generate_path<false>(S, seed_lo, seed_hi, x0 + x, y0 + y, sample, p, cnt);
  keys[i] = make_uint2((y0 + y) * S.width + (x0 + x), p.rng.ctr);
}

// One thread per point of an irradiance query with one sample (P.first_sample): the ray that sample's path starts with - the point's position
// and interval around the drawn direction - and the key it goes on from, (key, the counter after the direction): a radiance query over them
// with samples = 1 and first_sample = P.first_sample is that sample's contribution, bit for bit (the same generator, irradiance_direction,
// from the same state). An invalid point gives an all-zero ray, itself invalid, beside (key, first_draw).
__global__ void __launch_bounds__(256) sol_irradiance_rays_kernel(const RadianceParams P, const float4* __restrict__ points, const uint2* __restrict__ keys,
                                                                  float4* __restrict__ rays_out, uint2* __restrict__ keys_out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= P.n_rays) return;
  const float4 a = ldg_f4(points + (size_t)i * 2u), b = ldg_f4(points + (size_t)i * 2u + 1u);
  uint32_t key = P.key_base + i, ctr = P.first_draw;
  if (keys) { const uint2 k = keys[i]; key = k.x; ctr = k.y; }
  float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra;
  if (query_ray_valid(a, b)) {
    Rng rng;
    rng_init(rng, P.seed_lo, P.seed_hi, key, P.first_sample);
    rng.ctr = ctr;
    const f3 d = irradiance_direction(P.mode, mk3(b.x, b.y, b.z), rng);
    ra = a; rb = make_float4(d.x, d.y, d.z, b.w);
    ctr = rng.ctr;
  }
  rays_out[(size_t)i * 2u] = ra; rays_out[(size_t)i * 2u + 1u] = rb;
  keys_out[i] = make_uint2(key, ctr);
}

// One thread per point of an SH irradiance query, after each sol_radiance_each_kernel launch: the window's `win_samples` colours
// of the point, partial[sample - P.first_sample][point], each times the nine basis values of its direction, added in sol_radiance's
// association - a chunk sum 0 + t + t .. per 16 samples counted from P.first_sample (a window starts on a chunk's first sample), the chunk
// sums in order on top of 0 or, `accumulate`, of what the earlier windows of the call left in `out`. The direction is drawn again exactly as
// the path drew it - rng_init(seed, key, s), the counter at first_draw, irradiance_direction -, so its bits are the path's. The row's validity
// is judged first: no colour of an invalid row is read (none was written), it answers 27 zero words and samples = 0. out: 7 dwordx4 per row.
__global__ void __launch_bounds__(256) sol_sh_project_kernel(const RadianceParams P, const float4* __restrict__ points, const uint2* __restrict__ keys,
                                                             const sol_v4f* __restrict__ partial, sol_v4f* __restrict__ out, uint32_t win_samples,
                                                             uint32_t samples, uint32_t accumulate) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= P.n_rays) return;
  const float4 a = ldg_f4(points + (size_t)i * 2u), b = ldg_f4(points + (size_t)i * 2u + 1u);
  SOL_AS1 sol_v4f* const row = (SOL_AS1 sol_v4f*)(out + (size_t)i * 7u);
  if (!query_ray_valid(a, b)) {
    const sol_v4f zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 7; ++q) row[q] = zero;
    return;
  }
  float total[28], chunk[27];
#pragma unroll
  for (int q = 0; q < 28; ++q) total[q] = 0.f;
  if (accumulate) {
#pragma unroll
    for (int q = 0; q < 7; ++q) {
      const sol_v4f o = row[q];
      total[4 * q] = o.x; total[4 * q + 1] = o.y; total[4 * q + 2] = o.z; total[4 * q + 3] = o.w;
    }
  }
  uint32_t key = P.key_base + i, ctr = P.first_draw;
  if (keys) {
    const unsigned long long kw = *(const SOL_AS1 unsigned long long*)(keys + i);  // one dwordx2: pixel, first_draw
    key = (uint32_t)kw; ctr = (uint32_t)(kw >> 32);
  }
  const f3 normal = mk3(b.x, b.y, b.z);
  const size_t stride = (size_t)P.n_groups * 64u;
  for (uint32_t j0 = 0; j0 < win_samples; j0 += SOL_CHUNK) {
#pragma unroll
    for (int q = 0; q < 27; ++q) chunk[q] = 0.f;
    const uint32_t j1 = win_samples - j0 > (uint32_t)SOL_CHUNK ? j0 + SOL_CHUNK : win_samples;
    for (uint32_t j = j0; j < j1; ++j) {
      Rng rng;
      rng_init(rng, P.seed_lo, P.seed_hi, key, P.first_sample + j);
      rng.ctr = ctr;
      const f3 d = irradiance_direction(P.mode, normal, rng);
      float Y[9];
      sh9_basis(d, Y);
      const sol_v4f c = *(const SOL_AS1 sol_v4f*)(partial + (size_t)j * stride + i);  // coalesced: [sample][point]
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        chunk[3 * k] = chunk[3 * k] + c.x * Y[k];
        chunk[3 * k + 1] = chunk[3 * k + 1] + c.y * Y[k];
        chunk[3 * k + 2] = chunk[3 * k + 2] + c.z * Y[k];
      }
    }
#pragma unroll
    for (int q = 0; q < 27; ++q) total[q] = total[q] + chunk[q];
  }
  total[27] = __uint_as_float(samples);
#pragma unroll
  for (int q = 0; q < 7; ++q) {
    const sol_v4f v = {total[4 * q], total[4 * q + 1], total[4 * q + 2], total[4 * q + 3]};
    row[q] = v;  // one dwordx4
  }
}

// ---- launch wrappers (called from sol_api.cpp) ----
// Built: the default estimator with and without the spill tail, plain and STRICT (4); the ENV / LT estimators SPILL-capable only, plain and
// STRICT (6) - a scene whose tree fits the LDS stack runs them with a spill area it never touches. Each of the ten once more with GATHER, for
// the irradiance queries, and the ten GATHER ones a third time as sol_radiance_each_kernel (EACH) for the SH irradiance queries.
// The variant table: which of them the run-time flags name - the launch and the occupancy query both ask here.
using RadianceKernel = void (*)(const DevScene*, const RadianceParams, const float4*, const uint2*, sol_v4f*, sol_v4f*, uint32_t*, uint32_t*);
template <bool SPILL, bool ENV, bool LT, bool GATHER>
static RadianceKernel radiance_variant_of(bool strict) { return strict ? sol_radiance_kernel<SPILL, true, ENV, LT, GATHER> : sol_radiance_kernel<SPILL, false, ENV, LT, GATHER>; }
template <bool GATHER>
static RadianceKernel radiance_variant_in(bool spill, bool strict, bool env, bool lt) {
  if (env) return lt ? radiance_variant_of<true, true, true, GATHER>(strict) : radiance_variant_of<true, true, false, GATHER>(strict);
  if (lt) return radiance_variant_of<true, false, true, GATHER>(strict);
  return spill ? radiance_variant_of<true, false, false, GATHER>(strict) : radiance_variant_of<false, false, false, GATHER>(strict);
}
template <bool SPILL, bool ENV, bool LT>
static RadianceKernel radiance_each_variant_of(bool strict) { return strict ? sol_radiance_each_kernel<SPILL, true, ENV, LT> : sol_radiance_each_kernel<SPILL, false, ENV, LT>; }
static RadianceKernel radiance_each_variant(bool spill, bool strict, bool env, bool lt) {
  if (env) return lt ? radiance_each_variant_of<true, true, true>(strict) : radiance_each_variant_of<true, true, false>(strict);
  if (lt) return radiance_each_variant_of<true, false, true>(strict);
  return spill ? radiance_each_variant_of<true, false, false>(strict) : radiance_each_variant_of<false, false, false>(strict);
}
static RadianceKernel sol_radiance_variant(bool gather, bool each, bool spill, bool strict, bool env, bool lt) {
  if (each) return radiance_each_variant(spill, strict, env, lt);  // (gather with it: the caller's rows are points)
  return gather ? radiance_variant_in<true>(spill, strict, env, lt) : radiance_variant_in<false>(spill, strict, env, lt);
}

hipError_t sol_launch_radiance(const DevScene* dS, const RadianceParams& P, bool gather, bool each, bool may_spill, bool strict, bool env, bool lt, const void* rays,
                               const void* keys, void* out, void* partial, uint32_t* work, uint32_t* spill, uint32_t grid, hipStream_t stream) {
  const RadianceKernel kernel = sol_radiance_variant(gather, each, may_spill, strict, env, lt);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(SOL_WG), 0, stream, dS, P, (const float4*)rays, (const uint2*)keys, (sol_v4f*)out, (sol_v4f*)partial, work, spill);
  return hipGetLastError();
}
int sol_radiance_blocks_per_cu(bool gather, bool each, bool strict, bool env, bool lt) { return sol_blocks_per_cu(sol_radiance_variant(gather, each, true, strict, env, lt)); }

hipError_t sol_launch_sh_project(const RadianceParams& P, const void* points, const void* keys, const void* partial, void* out, uint32_t win_samples, uint32_t samples,
                                 bool accumulate, hipStream_t stream) {
  hipLaunchKernelGGL(sol_sh_project_kernel, dim3((P.n_rays + 255u) / 256u), dim3(256), 0, stream, P, (const float4*)points, (const uint2*)keys, (const sol_v4f*)partial,
                     (sol_v4f*)out, win_samples, samples, accumulate ? 1u : 0u);
  return hipGetLastError();
}

hipError_t sol_launch_irradiance_rays(const RadianceParams& P, const void* points, const void* keys, void* rays_out, void* keys_out, hipStream_t stream) {
  hipLaunchKernelGGL(sol_irradiance_rays_kernel, dim3((P.n_rays + 255u) / 256u), dim3(256), 0, stream, P, (const float4*)points, (const uint2*)keys,
                     (float4*)rays_out, (uint2*)keys_out);
  return hipGetLastError();
}

hipError_t sol_launch_radiance_resolve(const RadianceParams& P, const void* rays, const void* partial, void* out, uint32_t samples, bool accumulate,
                                       hipStream_t stream) {
  hipLaunchKernelGGL(sol_radiance_resolve_kernel, dim3((P.n_rays + 255u) / 256u), dim3(256), 0, stream, P, (const float4*)rays, (const sol_v4f*)partial,
                     (sol_v4f*)out, samples, accumulate ? 1u : 0u);
  return hipGetLastError();
}

hipError_t sol_launch_camera_ray_keys(const DevScene* dS, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t sample, uint64_t seed, void* keys,
                                      hipStream_t stream) {
  const uint32_t n = w * h;
  hipLaunchKernelGGL(sol_camera_ray_keys_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, dS, x0, y0, w, h, sample, (uint32_t)seed, (uint32_t)(seed >> 32),
                     (uint2*)keys);
  return hipGetLastError();
}
