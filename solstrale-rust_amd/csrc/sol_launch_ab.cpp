// sol_launch_ab.cpp -- the launches of the measured-and-rejected render-kernel variants: 2 (wave-private pool) and 3 (two-kernel wavefront) of
// sol_wavefront.hip, 4 (the pool kernel) of sol_pool.hip. Like those two files, part of the -DSOL_AB_KERNELS build of the library only (build.py,
// `_build_ab/`): the product library carries one kernel family, and sol_render_impl (sol_launch.cpp) hands every job of another variant to
// sol_render_ab through its one seam. The variants raise the search's lane occupancy (0.45 -> 0.67-0.73) but pay for it in state traffic, refill
// stalls and per-round tails (MI355X, C3, 128 spp: v1 997, v2 905, v3 684 Msamples/s when they were last compared). The steps every
// render launch takes - base parameters, `partial`, counters and timing, resolves, statistics - are sol_launch.cpp's (sol_scene.h).
#include <algorithm>

#include "sol_scene.h"

#ifdef SOL_AB_KERNELS
namespace {

// Variant 3: rounds of (shade, trace) over ONE global pool of path slots until no slot holds work; the live-slot count is read back every few rounds.
int wavefront_rounds(SolScene* s, const SolRenderJob& job, const RenderParams& P, uint32_t grid) {
  uint32_t* ctr = s->wf_ctr.get();  // WfCounters {work_next, slot_cursor, live, pad}
  HIP_TRY(hipMemsetAsync(ctr, 0, 16, s->stream));
  HIP_TRY(hipMemsetAsync(s->pool.get() + (size_t)P.pool_slots * 16, 0, (size_t)P.pool_slots * 16, s->stream));  // record 1: flags
  HIP_TRY(hipMemsetAsync(s->queue.get(), 0, (size_t)P.pool_slots / 64 * 8, s->stream));                              // reservoirs
  const uint32_t check_every = 16;
  for (uint32_t rounds = 1;; ++rounds) {
    HIP_TRY(hipMemsetAsync(ctr + 1, 0, 8, s->stream));  // slot_cursor, live
    HIP_TRY(sol_launch_wf_shade(job.view, P, job.acc, s->partial.get(), ctr, s->pool.get(), s->queue.get(), s->counters.get(), job.count, s->stream));
    HIP_TRY(sol_launch_wf_trace(job.view, P, ctr, s->pool.get(), s->spill.get(), s->counters.get(), grid, job.count, s->has_medium, s->stream));
    if (rounds % check_every == 0) {
      HIP_TRY(hipMemcpyAsync(s->wf_ctr_host.get(), ctr, 16, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipStreamSynchronize(s->stream));
      if (s->wf_ctr_host.get()[2] == 0) return SOL_OK;
      if (rounds > 4000000u) return sol_fail(SOL_EDEVICE, "wavefront did not drain");
    }
  }
}

// One launch (variant 3: one sequence of launches) of `job`. These kernels trace every block: no background tail, no adaptive rounds.
int launch_variant(SolScene* s, const SolRenderJob& job, int variant) {
  const bool count = job.count;
  RenderParams P;
  int rc;
  if ((rc = sol_render_params(s, job, s->n_local_blocks, P))) return rc;
  if (P.n_local_blocks == 0) return SOL_OK;
  const int bpc = variant == 4 ? sol_pool4_blocks_per_cu(s->has_medium, s->strict_triangles)
                : variant == 3 ? sol_wf_trace_blocks_per_cu(count, s->has_medium) : sol_pool_blocks_per_cu(count, s->has_medium);
  uint32_t lds_depth = (uint32_t)SOL_LDS_STACK;
  uint32_t stack_need = s->tree.depth;  // dwords of traversal stack a search of this scene can use
  // (swap_min: lanes waiting before an exchange pass of the search loop; 64 = only when the wave would otherwise leave for the service block, the best setting measured)
  if (variant == 4) { lds_depth = (uint32_t)sol_pool4_lds_stack_depth(); stack_need = s->tree.packed_depth; P.swap_min = s->pool_swap_min ? s->pool_swap_min : 64u; }
  if (variant == 3) lds_depth = (uint32_t)sol_wf_lds_stack_depth();
  uint32_t grid;
  if ((rc = sol_launch_plan(s, bpc, P.n_items, lds_depth, stack_need, s->spill, &grid))) return rc;
  P.total_threads = grid * SOL_WG;
  size_t stage_floats = 0;
  if (variant == 3) {
    // one global pool: enough slots that the trace kernel has >= 16 rays per resident lane, never more than the items
    uint64_t want = std::min<uint64_t>(P.n_items, s->wf_slots);
    want = ((want + SOL_WG - 1) / SOL_WG) * SOL_WG;
    P.pool_slots = (uint32_t)want;
    // POOL_RECORDS float4 per slot; item reservoirs: one uint2 per 64 slots (shade wave)
    if ((rc = s->pool.reserve(s->stream, sol_wf_pool_bytes(P.pool_slots))) || (rc = s->queue.reserve(s->stream, P.pool_slots / 64)) || (rc = s->wf_ctr.reserve(s->stream, 16))) return rc;
    if (!s->wf_ctr_host) HIP_TRY(sol_pinned_alloc(s->wf_ctr_host, 16));
  } else if (variant == 2) {
    // pool of path slots: per wave a multiple of 64, enough that every wave has several rays per lane in flight
    const uint32_t waves = grid * (SOL_WG / 64);
    uint32_t per_wave = (P.n_items + waves - 1) / waves;
    per_wave = ((per_wave + 63u) / 64u) * 64u;
    P.pool_slots = std::min<uint32_t>(SOL_POOL_MAX, std::max<uint32_t>(64u, per_wave));
    if (s->pool_slots_override) P.pool_slots = std::min<uint32_t>(SOL_POOL_MAX, ((s->pool_slots_override + 63u) / 64u) * 64u);
    if ((rc = s->pool.reserve(s->stream, sol_pool_bytes_per_wave(P.pool_slots) * waves))) return rc;
  } else {  // 4: every pair (block, chunk) is handed out sample by sample: the staging area holds the whole launch
    const uint64_t total = (uint64_t)P.n_chunks * P.n_traced_blocks * 64u * SOL_CHUNK;
    if (total > SOL_MAX_ITEMS || (uint64_t)P.stage_at + total > 0xFFFFFFFFull) return sol_fail(SOL_EINVAL, "too many work items in one call (%llu): split the sample range", (unsigned long long)total);
    stage_floats = (size_t)total * 3u;
    P.n_coarse = 0;
    P.n_items = (uint32_t)total;
    // items per reservation of a wave's reservoir: a whole pair (1024 samples) when every resident wave gets at least 16 of them, else 64
    P.pool_slots = total >= (uint64_t)(P.total_threads / 64u) * 1024u * 16u ? 1024u : 64u;
  }
  // the pool kernel writes every chunk sum into `partial` (also when the call has a single chunk); v2 / v3 add a single chunk straight
  // into the accumulator
  const bool via_partial = variant == 4 || P.n_chunks > 1;
  if (via_partial && (rc = sol_render_partial(s, P, stage_floats))) return rc;
  if ((rc = sol_render_begin(s, count))) return rc;
  if (variant == 3) {
    if ((rc = wavefront_rounds(s, job, P, grid))) return rc;
  } else {
    if ((rc = job.mirror->upload(s->stream, job.view))) return rc;
    if (P.n_items > 0 && variant == 4)
      HIP_TRY(sol_launch_pool4(job.view, job.mirror->dev.get(), P, s->partial.get(), s->work.get(), s->spill.get(), grid, s->has_medium, stack_need > lds_depth,
                               count ? s->counters.get() : nullptr, s->stream));
    else if (P.n_items > 0)
      HIP_TRY(sol_launch_pool(job.view, P, job.acc, s->partial.get(), s->work.get(), s->spill.get(), s->pool.get(), s->counters.get(), grid, count, s->has_medium, s->stream));
  }
  return sol_render_end(s, job, P, grid, via_partial);
}
}  // namespace

int sol_render_ab(SolScene* s, const SolRenderJob& job, int variant) {
  if (variant != 4) return launch_variant(s, job, variant);
  // One launch of the pool kernel stages ONE COLOUR PER SAMPLE: a long sample range goes through several launches (chunk-aligned, so the sums
  // do not depend on the split; uncounted), each within the staging budget.
  const uint64_t pairs_per_chunk = (uint64_t)s->n_local_blocks;
  const uint64_t max_chunks = std::max<uint64_t>(1, std::min<uint64_t>((6ull << 30) / std::max<uint64_t>(1, pairs_per_chunk * 64u * SOL_CHUNK * 12u),
                                                                       (uint64_t)SOL_MAX_ITEMS / std::max<uint64_t>(1, pairs_per_chunk * 64u * SOL_CHUNK)));
  if (((uint64_t)job.n + SOL_CHUNK - 1) / SOL_CHUNK <= max_chunks) return launch_variant(s, job, variant);
  SolRenderJob piece = job;
  piece.count = false;
  for (uint32_t left = job.n; left; left -= piece.n, piece.first += piece.n) {
    piece.n = (uint32_t)std::min<uint64_t>(left, max_chunks * SOL_CHUNK);
    if (const int rc = launch_variant(s, piece, variant)) return rc;
  }
  return SOL_OK;
}
#endif  // SOL_AB_KERNELS
