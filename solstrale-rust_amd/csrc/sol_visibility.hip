// sol_visibility.hip -- visibility gathers (include/solstrale_hip.h, sol_visibility / sol_visibility_dev): per point, how many of
// the directions an irradiance query would draw there are open, the sum of the open ones (the bent normal) and the hit-distance moments of the
// others. A sample is the ray sol_irradiance_rays writes for it (irradiance_direction, sol_ray.h), answered as sol_query answers it
// (query_when_settled, query_occluded_done: sol_ray.h) by the world search of sol_trace.h in the search context of sol_wave.h - without a path.
//
//  sol_visibility_kernel<ANY, SPILL, STRICT> -- a work item is (point, chunk), chunk-major: an aligned run of 64 items is 64 consecutive points
//    of one chunk of SOL_CHUNK samples. The persistent-wave schedule of sol_wave.h, as sol_radiance_kernel runs it: a lane takes its next item
//    from the wave's reservoir the moment its own is written, and the wave leaves the search loop by the render's vote (switch_below). A lane
//    owns its item from the first sample to the last, keeps the chunk's five float sums and two counters in registers and writes once, two
//    dwordx4: the answer itself when the call has one chunk, else a row of the partial buffer. No atomic touches an answer. The lane keeps the
//    point's index, not the point: the row (two dwordx4) and the key (one dwordx2) are read again at each sample - L2 hits after the first, as
//    in sol_radiance_body.h -, the generator is made afresh per sample, and the ray of the running search lives in the search state (Trav::o, d).
//    ANY = true (SOL_QUERY_OCCLUDED) ends a search at its first accepted primitive and adds no distance. SPILL / STRICT as in sol_query.hip.
//    (Measured and not kept: sol_query_kernel's loop, whole waves striding over the items and settling with or without the vote - the same
//    bytes, 0.73 of this schedule's rate on two million points: profiles/visibility.txt.)
//  sol_visibility_resolve_kernel -- more than one chunk: adds a point's chunk rows in chunk order, sol_radiance_resolve_kernel's association.
//
// Every sum is one lane's, in sample order: the answers do not depend on the schedule.
#include <hip/hip_runtime.h>

#include "sol_launch.h"
#include "sol_ray.h"
#include "sol_wave.h"

namespace {

// a SolVisibility row (or a chunk's row of the partial buffer): two dwordx4
DEV void visibility_store(sol_v4f* __restrict__ row, f3 b, uint32_t open, float t_sum, float t2_sum, uint32_t hits, uint32_t samples) {
  const sol_v4f w0 = {b.x, b.y, b.z, __uint_as_float(open)}, w1 = {t_sum, t2_sum, __uint_as_float(hits), __uint_as_float(samples)};
  SOL_AS1 sol_v4f* o = (SOL_AS1 sol_v4f*)row;
  o[0] = w0;
  o[1] = w1;
}

}  // namespace

template <bool ANY, bool SPILL, bool STRICT>
__global__ void __launch_bounds__(SOL_WG, SOL_V1_MIN_WAVES)
sol_visibility_kernel(const DevScene* __restrict__ Sp, const RadianceParams P, const float4* __restrict__ points, const uint2* __restrict__ keys,
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
  Rng none = {};  // (the search draws nothing without a medium)

  Trav t;
  t.cur = REF_DONE;
  bool busy = false, in_flight = false;  // the lane holds an item; a sample's search has been started (running, or over: t.cur == REF_DONE)
  uint32_t index = 0, s = 0, s_end = 0;  // the item: point `index` of the launch, samples [s, s_end) of it still to come
  uint32_t left = 0;                     // searches behind a refused hit the running sample may still start
  f3 b = mk3(0.f, 0.f, 0.f);
  float t_sum = 0.f, t2_sum = 0.f;
  uint32_t open = 0, hits = 0;

  for (;;) {
    // ---- lanes without a running search: settle the sample that is over and account it; write a finished item and take the next one;
    // start the next sample. Every turn moves such a lane on (a sample, a restart out of 63, an item), so the loop ends ----
    if (t.cur == REF_DONE) {
      bool settled = !in_flight;
      if (in_flight) {
        // (the ray's own upper end, for a search behind a refused needle hit: the row's last word, read again)
        const float tmax = STRICT ? __uint_as_float(ldg_u32((const float*)(points + (size_t)index * 2u + 1u) + 3)) : 0.f;
        query_when_settled<STRICT>(S, st, t, tmax, left, [&]() __attribute__((always_inline)) {
          if (SOL_REF_KIND(t.h.ref) != SOL_REF_NONE) {  // SOL_RAY_HIT
            hits++;
            if (!ANY) {
              t_sum = t_sum + t.h.t;
              t2_sum = t2_sum + t.h.t * t.h.t;  // (-ffp-contract=off: the product is rounded on its own)
            }
          } else {  // SOL_RAY_MISS: the direction as drawn
            open++;
            b = b + t.d;
          }
          in_flight = false;
          s++;
          settled = true;
        });
      }
      if (settled && busy && s == s_end) {
        // one chunk in the whole call: the answer itself; else the chunk's row at [chunk][point] for sol_visibility_resolve_kernel
        if (P.direct) visibility_store(out + (size_t)index * 2u, b, open, t_sum, t2_sum, hits, P.end_sample - P.first_sample);
        else visibility_store(partial + ((size_t)((s - 1u - P.first_sample) / SOL_CHUNK) * (P.n_groups * 64u) + index) * 2u, b, open, t_sum, t2_sum, hits, 0u);
        busy = false;
      }
      // work fetch: the next item from the wave's reservoir (sol_wave.h) - 64 items, 64 consecutive points of one chunk, per refill
      if (settled && !busy) {
        const uint32_t item = wave_take_item(res, work_counter, lane);
        if (item >= P.n_items) break;  // no work left for this lane
        const uint32_t pair = item >> 6, chunk = pair / P.n_groups;
        index = (pair - chunk * P.n_groups) * 64u + (item & 63u);
        if (index >= P.n_rays) continue;  // padding of the last group
        // validity, before any search (sol_ray.h): an invalid point answers eight zero words - here when the kernel writes the answers
        // itself, else in the resolve kernel
        if (!query_ray_valid(ldg_f4(points + (size_t)index * 2u), ldg_f4(points + (size_t)index * 2u + 1u))) {
          if (P.direct) visibility_store(out + (size_t)index * 2u, mk3(0.f, 0.f, 0.f), 0u, 0.f, 0.f, 0u, 0u);
          continue;
        }
        s = P.first_sample + chunk * SOL_CHUNK;
        s_end = P.end_sample - s > (uint32_t)SOL_CHUNK ? s + SOL_CHUNK : P.end_sample;
        b = mk3(0.f, 0.f, 0.f);
        t_sum = t2_sum = 0.f;
        open = hits = 0u;
        busy = true;
      }
      if (settled) {
        // the ray sol_irradiance_rays writes for (point, s): the generator of (seed, key, s) with its counter at first_draw
        const float4 a = ldg_f4(points + (size_t)index * 2u), n = ldg_f4(points + (size_t)index * 2u + 1u);
        uint32_t key = P.key_base + index, ctr = P.first_draw;
        if (keys) {
          const unsigned long long kw = *(const SOL_AS1 unsigned long long*)(keys + index);  // one dwordx2: pixel, first_draw
          key = (uint32_t)kw; ctr = (uint32_t)(kw >> 32);
        }
        Rng rng;
        rng_init(rng, P.seed_lo, P.seed_hi, key, s);
        rng.ctr = ctr;
        const f3 d = irradiance_direction(P.mode, mk3(n.x, n.y, n.z), rng);
        if (query_ray_valid(a, make_float4(d.x, d.y, d.z, n.w))) {
          trav_begin_world(t, S, mk3(a.x, a.y, a.z), d, a.w, n.w);
          left = 63u;
          in_flight = true;
        } else {
          s++;  // (a normal whose squared length is no normal number: the made ray is invalid - searched for nothing, counted nowhere)
        }
      }
    }
    // ---- search: one step per turn for every lane that has one, until the wave votes to leave for the block above ----
#if SOL_LOOP_PRIO
    __builtin_amdgcn_s_setprio(SOL_LOOP_PRIO);
#endif
    for (;;) {
      const bool act = t.cur != REF_DONE;
      if (!wave_keeps_searching(act, P.switch_below)) break;
      trav_step_wave<false, false, STRICT>(S, t, act, st, none, 0u, cnt);
      if (ANY) query_occluded_done<STRICT>(t, act);
    }
#if SOL_LOOP_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif
  }
}

// One thread per point of a launch with more than one chunk (or one window of a longer sample range): the chunk rows in chunk order on top
// of 0 - or, `accumulate`, of what the earlier windows of the same call left in `out` -, ((0 + c0) + c1) + ..; the counters are integers.
// An invalid point answers eight zero words.
__global__ void __launch_bounds__(256) sol_visibility_resolve_kernel(const RadianceParams P, const float4* __restrict__ points, const sol_v4f* __restrict__ partial,
                                                                     sol_v4f* __restrict__ out, uint32_t samples, uint32_t accumulate) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= P.n_rays) return;
  sol_v4f* const row = out + (size_t)i * 2u;
  if (!query_ray_valid(ldg_f4(points + (size_t)i * 2u), ldg_f4(points + (size_t)i * 2u + 1u))) {
    visibility_store(row, mk3(0.f, 0.f, 0.f), 0u, 0.f, 0.f, 0u, 0u);
    return;
  }
  f3 b = mk3(0.f, 0.f, 0.f);
  float t_sum = 0.f, t2_sum = 0.f;
  uint32_t open = 0u, hits = 0u;
  if (accumulate) {
    const sol_v4f o0 = *(const SOL_AS1 sol_v4f*)row, o1 = *(const SOL_AS1 sol_v4f*)(row + 1);
    b = mk3(o0.x, o0.y, o0.z); open = __float_as_uint(o0.w);
    t_sum = o1.x; t2_sum = o1.y; hits = __float_as_uint(o1.z);
  }
  for (uint32_t k = 0; k < P.n_chunks; ++k) {
    const sol_v4f* const c = partial + ((size_t)k * (P.n_groups * 64u) + i) * 2u;
    const sol_v4f c0 = *(const SOL_AS1 sol_v4f*)c, c1 = *(const SOL_AS1 sol_v4f*)(c + 1);
    b = b + mk3(c0.x, c0.y, c0.z); open += __float_as_uint(c0.w);
    t_sum = t_sum + c1.x; t2_sum = t2_sum + c1.y; hits += __float_as_uint(c1.z);
  }
  visibility_store(row, b, open, t_sum, t2_sum, hits, samples);
}

// ---- launch wrappers (called from sol_api.cpp) ----
// The variant table of the family: which instantiation the run-time flags name - the launch and the occupancy query both ask here.
using VisibilityKernel = void (*)(const DevScene*, const RadianceParams, const float4*, const uint2*, sol_v4f*, sol_v4f*, uint32_t*, uint32_t*);
template <bool ANY>
static VisibilityKernel visibility_variant_of(bool spill, bool strict) {
  if (spill) return strict ? sol_visibility_kernel<ANY, true, true> : sol_visibility_kernel<ANY, true, false>;
  return strict ? sol_visibility_kernel<ANY, false, true> : sol_visibility_kernel<ANY, false, false>;
}
static VisibilityKernel sol_visibility_variant(bool any, bool spill, bool strict) {
  return any ? visibility_variant_of<true>(spill, strict) : visibility_variant_of<false>(spill, strict);
}

hipError_t sol_launch_visibility(const DevScene* dS, const RadianceParams& P, bool any, bool may_spill, bool strict, const void* points, const void* keys, void* out,
                                 void* partial, uint32_t* work, uint32_t* spill, uint32_t grid, hipStream_t stream) {
  const VisibilityKernel kernel = sol_visibility_variant(any, may_spill, strict);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(SOL_WG), 0, stream, dS, P, (const float4*)points, (const uint2*)keys, (sol_v4f*)out, (sol_v4f*)partial, work, spill);
  return hipGetLastError();
}
int sol_visibility_blocks_per_cu(bool any, bool strict) { return sol_blocks_per_cu(sol_visibility_variant(any, true, strict)); }

hipError_t sol_launch_visibility_resolve(const RadianceParams& P, const void* points, const void* partial, void* out, uint32_t samples, bool accumulate,
                                         hipStream_t stream) {
  hipLaunchKernelGGL(sol_visibility_resolve_kernel, dim3((P.n_rays + 255u) / 256u), dim3(256), 0, stream, P, (const float4*)points, (const sol_v4f*)partial,
                     (sol_v4f*)out, samples, accumulate ? 1u : 0u);
  return hipGetLastError();
}
