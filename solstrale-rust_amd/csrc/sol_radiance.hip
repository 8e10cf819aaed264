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
  const DevScene& S = *Sp;
  __shared__ uint32_t lds_stack[SOL_LDS_STACK * SOL_WG];
  __shared__ uint8_t oct_table[SOL_OCT_TABLE_BYTES];
  __shared__ __attribute__((aligned(16))) uint32_t sel_table[SOL_SEL_TABLE_DWORDS];
  __shared__ uint32_t reservoir[SOL_WG / 64][2];  // per wave: next reserved item, end of the reservation
  const uint32_t lane = threadIdx.x & 63u;
  Stack st;
  wave_search_stack(st, S, lds_stack, SOL_LDS_STACK, SPILL, spill, P.total_threads, oct_table, sel_table);
  volatile lds_u32* const res = wave_reservoir(reservoir);
  Counters cnt = {};
  const float inf = __builtin_huge_valf();

  bool have_item = false, alive = false, in_flight = false;
  uint32_t index = 0, s = 0, s_end = 0;  // the item: ray `index` of the launch, samples [s, s_end) of it still to come
  f3 sum = mk3(0.f, 0.f, 0.f);
  Path p = {};
  Trav t;
  t.cur = REF_DONE;

  for (;;) {
    // ---- lanes whose search is over: the service block of sol_render_kernel, with the caller's ray and its interval at depth 0 ----
    const bool again = t.cur == REF_DONE && in_flight && sol_self_hit(p.from, t.h);  // (rule 8; a caller's ray leaves no primitive: depth > 0 only)
    // (STRICT) a refused needle hit: the lane searches the same ray again behind it - at depth 0 up to the ray's own upper end, as query_settle does
    if (STRICT && !again && t.cur == REF_DONE && in_flight && !trav_accept_or_restart(S, t, st) && p.depth == 0u) t.h.t = radiance_tmax(rays, index);
    if (t.cur == REF_DONE) {
      float tmin = RAY_MIN_F, tmax = inf;
      float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra;  // the item's ray as the work fetch of this pass loaded it
      bool fresh_ray = false;
      if (again) {
        p.o = t.o; p.d = t.d;
        tmin = sol_behind(t.h.t);
        if (p.depth == 0u) tmax = radiance_tmax(rays, index);
      } else if (in_flight) {
        in_flight = false;
        p.o = t.o; p.d = t.d;  // (the ray lives in the search state while it is traced)
        f3 c;
        if (shade_vertex<false, STRICT, ENV, LT>(S, p, t.h, c, cnt)) {
          sum = sum + c;  // sums, not means: the render's chunk sum, 0 + c0 + c1 + .. in sample order
          alive = false;
          s++;
          if (s == s_end) {
            // one chunk in the whole call: the answer itself; else the chunk sum at [chunk][ray] for sol_radiance_resolve_kernel
            if (P.direct) radiance_store(out + index, sum, P.end_sample - P.first_sample);
            else radiance_store(partial + (size_t)((s - 1u - P.first_sample) / SOL_CHUNK) * (P.n_groups * 64u) + index, sum, 0u);
            have_item = false;
          }
        }
      }
      // work fetch: the next item from the wave's reservoir (sol_wave.h) - 64 items, 64 consecutive rays of one chunk, per refill
      if (!again && !have_item) {
        const uint32_t item = wave_take_item(res, work_counter, lane);
        if (item >= P.n_items) break;  // no work left for this lane
        // item -> (ray, chunk), chunk-major: an aligned run of 64 items is 64 consecutive rays of one chunk
        const uint32_t pair = item >> 6, chunk = pair / P.n_groups;
        index = (pair - chunk * P.n_groups) * 64u + (item & 63u);
        if (index >= P.n_rays) continue;  // padding of the last group
        // validity, before any search (sol_ray.h): an invalid ray answers (0, 0, 0, samples = 0) - here when the kernel writes the
        // answers itself, else in the resolve kernel
        ra = ldg_f4(rays + (size_t)index * 2u); rb = ldg_f4(rays + (size_t)index * 2u + 1u);
        fresh_ray = true;  // (the first sample of the item starts from these values; the later ones read the ray again)
        if (!query_ray_valid(ra, rb)) {
          if (P.direct) radiance_store(out + index, mk3(0.f, 0.f, 0.f), 0u);
          continue;
        }
        s = P.first_sample + chunk * SOL_CHUNK;
        s_end = P.end_sample - s > (uint32_t)SOL_CHUNK ? s + SOL_CHUNK : P.end_sample;
        sum = mk3(0.f, 0.f, 0.f);
        have_item = true;
        alive = false;
      }
      if (!again && !alive) {
        // the path as generate_path leaves it, with the caller's ray: the RNG keyed by (seed, key, sample), its counter at first_draw
        if (!fresh_ray) { ra = ldg_f4(rays + (size_t)index * 2u); rb = ldg_f4(rays + (size_t)index * 2u + 1u); }
        const float4 a = ra, b = rb;
        uint32_t key = P.key_base + index, ctr = P.first_draw;
        if (keys) {
          const unsigned long long kw = *(const SOL_AS1 unsigned long long*)(keys + index);  // one dwordx2: pixel, first_draw
          key = (uint32_t)kw; ctr = (uint32_t)(kw >> 32);
        }
        rng_init(p.rng, P.seed_lo, P.seed_hi, key, s);
        p.rng.ctr = ctr;
        p.o = mk3(a.x, a.y, a.z);
        // (GATHER) an irradiance query: the row is a point and b.xyz its normal - the sample draws its direction here, while only the row and
        // the generator are live, and the path goes on from the counter the draws leave
        p.d = GATHER ? irradiance_direction(P.mode, mk3(b.x, b.y, b.z), p.rng) : mk3(b.x, b.y, b.z);
        p.A = mk3(1.f, 1.f, 1.f);
        p.C = mk3(inf, inf, inf);
        p.acc_len = 0.0f;
        p.depth = 0;
        p.pdf_seen = false;
        p.from = 0u;
        tmin = a.w; tmax = b.w;  // the depth-0 search runs over the ray's own interval; every later one over [RAY_MIN, +inf)
        alive = true;
      }
      trav_restart_world<STRICT>(t, S, p.o, p.d, tmin, tmax, again);  // (again: a bound the needle rule had set for this ray stays)
      in_flight = true;
    }
    // ---- search: one step per turn for every lane that has one, until the wave votes to leave for the service block ----
#if SOL_LOOP_PRIO
    __builtin_amdgcn_s_setprio(SOL_LOOP_PRIO);
#endif
    for (;;) {
      const bool act = t.cur != REF_DONE;
      if (!wave_keeps_searching(act, P.switch_below)) break;
      trav_step_wave<false, false, STRICT>(S, t, act, st, p.rng, p.depth, cnt);
    }
#if SOL_LOOP_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif
  }
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

// ---- launch wrappers (called from sol_api.cpp) ----
// Built: the default estimator with and without the spill tail, plain and STRICT (4); the ENV / LT estimators SPILL-capable only, plain and
// STRICT (6) - a scene whose tree fits the LDS stack runs them with a spill area it never touches. Each of the ten once more with GATHER, for
// the irradiance queries.
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
static RadianceKernel sol_radiance_variant(bool gather, bool spill, bool strict, bool env, bool lt) {
  return gather ? radiance_variant_in<true>(spill, strict, env, lt) : radiance_variant_in<false>(spill, strict, env, lt);
}

hipError_t sol_launch_radiance(const DevScene* dS, const RadianceParams& P, bool gather, bool may_spill, bool strict, bool env, bool lt, const void* rays,
                               const void* keys, void* out, void* partial, uint32_t* work, uint32_t* spill, uint32_t grid, hipStream_t stream) {
  const RadianceKernel kernel = sol_radiance_variant(gather, may_spill, strict, env, lt);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(SOL_WG), 0, stream, dS, P, (const float4*)rays, (const uint2*)keys, (sol_v4f*)out, (sol_v4f*)partial, work, spill);
  return hipGetLastError();
}
int sol_radiance_blocks_per_cu(bool gather, bool strict, bool env, bool lt) { return sol_blocks_per_cu(sol_radiance_variant(gather, true, strict, env, lt)); }

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
