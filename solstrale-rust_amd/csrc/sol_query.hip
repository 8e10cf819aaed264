// sol_query.hip -- ray queries (include/solstrale_hip.h, sol_query / sol_query_dev / sol_camera_rays): batches of
// caller-made rays answered by the world search of sol_trace.h in the search context of sol_wave.h (wave_search_stack), as the render
// kernel runs it, without a path around them: no shading, no accumulator, no RNG.
//
//  sol_query_kernel<ANY, SPILL, STRICT> -- one ray per lane, run to completion, grid-stride over the batch by whole waves. ANY = false
//    (SOL_QUERY_CLOSEST) writes one SolRayHit per ray, ANY = true (SOL_QUERY_OCCLUDED) one status word and ends a lane's search at its first
//    accepted primitive. SPILL / STRICT as in sol_render.hip: a tree deeper than the LDS stack, a scene with needle triangles.
//  sol_camera_rays_kernel -- generate_path (sol_path.h) of a pixel rectangle, written as rays: the render kernel's own camera rays.
//  (The measured alternative schedule - persistent waves that refill finished lanes from a batch counter - gave the same bytes at half
//  the rate and is not kept: profiles/ray_queries_ab.txt.)
//
// A ray's answer is a function of the ray and the scene alone: the (t, dfs) order of `better` is total, so neither the schedule nor the
// neighbours in the wave (postponed primitive tests, SOL_PRIM_MIN) can change it.
#include <hip/hip_runtime.h>

#include "sol_launch.h"
#include "sol_ray.h"
#include "sol_wave.h"

namespace {

struct QueryLane {
  Trav t;
  float tmax;         // the ray's own upper end (a search behind a refused needle hit starts over with it)
  uint32_t index;     // which ray of the batch
  uint32_t left;      // searches behind a refused hit this ray may still start (closest_hit's guard: 64 searches in all)
  bool busy;          // the lane holds a ray that is not answered yet
};

// (query_ray_valid, the validity rule of a ray: sol_ray.h - the radiance queries decide by the same one; query_when_settled and
// query_occluded_done, the needle rule's restarts and the occlusion early-out: sol_ray.h - the visibility gathers answer by the same ones)

template <bool ANY>
DEV void query_write(const DevScene& S, const Stack& st, void* __restrict__ out, uint32_t i, uint32_t status, const Hit& h) {
  if (ANY) {
    ((uint32_t*)out)[i] = status;
    return;
  }
  sol_v4u w0 = {__float_as_uint(__builtin_huge_valf()), 0u, 0u, status}, w1 = {0u, 0u, 0u, 0u};
  if (status == SOL_RAY_INVALID) w0.x = 0u;
  if (status == SOL_RAY_HIT) {
    const uint32_t kind = SOL_REF_KIND(h.ref), idx = SOL_REF_INDEX(h.ref);
    // the material of the primitive's own record; a sphere's Hit carries no u, v (whatever an earlier candidate left there is not its)
    int32_t mat;
    float u = h.u, v = h.v;
    if (kind == SOL_REF_TRIANGLE) mat = ldg_i32(&st.tris[idx].mat);
    else if (kind == SOL_REF_QUAD) mat = ldg_i32(&S.quads[idx].mat);
    else { mat = ldg_i32(&S.spheres[idx].mat); u = v = 0.0f; }
    w0.x = __float_as_uint(h.t); w0.y = __float_as_uint(u); w0.z = __float_as_uint(v);
    w1.x = kind; w1.y = h.dfs; w1.z = (uint32_t)mat;
  }
  sol_v4u* o = (sol_v4u*)out + (size_t)i * 2u;
  o[0] = w0;
  o[1] = w1;
}

// Takes ray `i` of the batch into the lane: an invalid ray is answered at once, a valid one starts its search.
template <bool ANY>
DEV void query_take(const DevScene& S, const Stack& st, const float4* __restrict__ rays, void* __restrict__ out, uint32_t i, QueryLane& q) {
  const float4 a = ldg_f4(rays + (size_t)i * 2u), b = ldg_f4(rays + (size_t)i * 2u + 1u);
  if (!query_ray_valid(a, b)) {
    Hit none = {};
    query_write<ANY>(S, st, out, i, SOL_RAY_INVALID, none);
    return;
  }
  trav_begin_world(q.t, S, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), a.w, b.w);
  q.tmax = b.w;
  q.index = i;
  q.left = 63u;
  q.busy = true;
}

// The lane's search is over (t.cur == REF_DONE): the ray is answered and written - or (STRICT) its closest hit was a triangle the consistency
// rule refuses, and the lane searches the same ray again behind it, at most 63 times, then the ray misses (query_when_settled, sol_ray.h).
template <bool ANY, bool STRICT>
DEV void query_settle(const DevScene& S, const Stack& st, void* __restrict__ out, QueryLane& q) {
  query_when_settled<STRICT>(S, st, q.t, q.tmax, q.left, [&]() __attribute__((always_inline)) {
    const bool hit = SOL_REF_KIND(q.t.h.ref) != SOL_REF_NONE;
    query_write<ANY>(S, st, out, q.index, hit ? SOL_RAY_HIT : SOL_RAY_MISS, q.t.h);
    q.busy = false;
  });
}

// One step of the wave's searches. ANY: a lane whose search holds an accepted primitive is done (query_occluded_done, sol_ray.h).
template <bool ANY, bool STRICT>
DEV void query_step(const DevScene& S, const Stack& st, const Rng& rng, Counters& cnt, QueryLane& q, bool act) {
  trav_step_wave<false, false, STRICT>(S, q.t, act, st, rng, 0u, cnt);
  if (ANY) query_occluded_done<STRICT>(q.t, act);
}

}  // namespace

template <bool ANY, bool SPILL, bool STRICT>
__global__ void __launch_bounds__(SOL_WG, SOL_V1_MIN_WAVES)
sol_query_kernel(const DevScene* __restrict__ Sp, const float4* __restrict__ rays, uint32_t n, void* __restrict__ out, uint32_t* __restrict__ spill,
                 uint32_t total_threads) {
  const DevScene& S = *Sp;
  __shared__ uint32_t lds_stack[SOL_LDS_STACK * SOL_WG];
  __shared__ uint8_t oct_table[SOL_OCT_TABLE_BYTES];
  __shared__ __attribute__((aligned(16))) uint32_t sel_table[SOL_SEL_TABLE_DWORDS];  // (the node test's permute selectors, as in the render kernel)
  Stack st;
  wave_search_stack(st, S, lds_stack, SOL_LDS_STACK, SPILL, spill, total_threads, oct_table, sel_table);
  Counters cnt = {};
  Rng rng = {};
  QueryLane q;
  q.t.cur = REF_DONE;
  q.busy = false;
  const uint32_t lane = threadIdx.x & 63u;
  // whole waves stride over the batch: `base` is the same in every lane of a wave, so the wave's votes see all of its lanes
  // (n <= 2^31 and the grid holds far fewer than 2^31 threads: base + total_threads does not wrap)
  for (uint32_t base = blockIdx.x * SOL_WG + (threadIdx.x & ~63u); base < n; base += total_threads) {
    if (base + lane < n) query_take<ANY>(S, st, rays, out, base + lane, q);
#if SOL_LOOP_PRIO
    __builtin_amdgcn_s_setprio(SOL_LOOP_PRIO);
#endif
    for (;;) {
      if (q.busy && q.t.cur == REF_DONE) query_settle<ANY, STRICT>(S, st, out, q);
      if (sol_ballot(q.busy) == 0ull) break;
      for (;;) {
        const bool act = q.t.cur != REF_DONE;  // (a lane without a ray rests at REF_DONE)
        if (sol_ballot(act) == 0ull) break;
        query_step<ANY, STRICT>(S, st, rng, cnt, q, act);
      }
    }
#if SOL_LOOP_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif
  }
}

// One thread per pixel of [x0, x0 + w) x [y0, y0 + h), row-major: the camera ray generate_path makes for (pixel, sample, seed).
__global__ void __launch_bounds__(256) sol_camera_rays_kernel(const DevScene* __restrict__ Sp, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                                              uint32_t sample, uint32_t seed_lo, uint32_t seed_hi, float4* __restrict__ rays) {
  const DevScene& S = *Sp;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;  // (w * h <= 2^31: checked by the caller)
  if (i >= w * h) return;
  const uint32_t y = i / w, x = i - y * w;
  Path p = {};
  Counters cnt = {};
  generate_path<false>(S, seed_lo, seed_hi, x0 + x, y0 + y, sample, p, cnt);
  sol_v4f a = {p.o.x, p.o.y, p.o.z, RAY_MIN_F}, b = {p.d.x, p.d.y, p.d.z, __builtin_huge_valf()};
  sol_v4f* o = (sol_v4f*)rays + (size_t)i * 2u;
  o[0] = a;
  o[1] = b;
}

// ---- launch wrappers (called from sol_api.cpp) ----
// The variant table of the family: which instantiation the run-time flags name - the launch and the occupancy query both ask here.
using QueryKernel = void (*)(const DevScene*, const float4*, uint32_t, void*, uint32_t*, uint32_t);
template <bool ANY>
static QueryKernel query_variant_of(bool spill, bool strict) {
  if (spill) return strict ? sol_query_kernel<ANY, true, true> : sol_query_kernel<ANY, true, false>;
  return strict ? sol_query_kernel<ANY, false, true> : sol_query_kernel<ANY, false, false>;
}
static QueryKernel sol_query_variant(bool any, bool spill, bool strict) { return any ? query_variant_of<true>(spill, strict) : query_variant_of<false>(spill, strict); }

hipError_t sol_launch_query(const DevScene* dS, bool any, bool may_spill, bool strict, const void* rays, uint32_t n, void* out, uint32_t* spill,
                            uint32_t grid, hipStream_t stream) {
  const QueryKernel kernel = sol_query_variant(any, may_spill, strict);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(SOL_WG), 0, stream, dS, (const float4*)rays, n, out, spill, grid * SOL_WG);
  return hipGetLastError();
}
int sol_query_blocks_per_cu(bool any, bool strict) { return sol_blocks_per_cu(sol_query_variant(any, true, strict)); }

hipError_t sol_launch_camera_rays(const DevScene* dS, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t sample, uint64_t seed, void* rays,
                                  hipStream_t stream) {
  const uint32_t n = w * h;
  hipLaunchKernelGGL(sol_camera_rays_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, dS, x0, y0, w, h, sample, (uint32_t)seed, (uint32_t)(seed >> 32),
                     (float4*)rays);
  return hipGetLastError();
}
