// sol_launch.cpp -- sol_render and its relatives: launch parameters, scratch buffers and launches of the render kernels
// (sol_render.hip), the auxiliary albedo / normal planes, the function-level and path-level debug hooks.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <future>
#include <limits>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "sol_scene.h"

int sol_launch_plan(SolScene* s, int blocks_per_cu, uint64_t items, uint32_t lds_depth, uint32_t stack_need, DevBuf<uint32_t>& spill, uint32_t* grid) {
  if (s->max_bpc > 0) blocks_per_cu = std::max(1, std::min(blocks_per_cu, s->max_bpc));  // SOL_OPT_MAX_BLOCKS_PER_CU
  const uint64_t need_blocks = std::max<uint64_t>(1, (items + SOL_WG - 1) / SOL_WG);
  *grid = (uint32_t)std::min<uint64_t>((uint64_t)(s->n_cu * blocks_per_cu), need_blocks);
  // spill stack only when the tree can out-grow the LDS stack
  return spill.reserve(s->stream, stack_need > lds_depth ? (size_t)*grid * SOL_WG * (stack_need - lds_depth) : 16);
}

// ad != null: one round of adaptive sampling (sol_adaptive.hip). The launch traces the active list `ad->order` - a DevScene copy
// with that work order, uploaded to its own device copy - and leaves the chunk sums in `partial` for sol_adaptive_round, which
// adds them to the accumulator; the product kernel itself is the one a plain render runs.
int sol_render_impl(SolScene* s, uint32_t first, uint32_t n, uint64_t seed, bool count, const SolAdaptiveLaunch* ad) {
  if (!s) return sol_fail(SOL_EINVAL, "null scene");
  if (n == 0) return SOL_OK;
  if ((uint64_t)first + n > 0xFFFFFFFFull) return sol_fail(SOL_EINVAL, "sample range overflows 32 bits");
  HIP_TRY(hipSetDevice(s->device));
  RenderParams P{};
  P.first_sample = first; P.n_samples = n;
  P.n_chunks = (uint32_t)(((uint64_t)n + SOL_CHUNK - 1) / SOL_CHUNK);  // (in 64 bits: n + 15 wraps for the last fifteen values of n)
  P.rank = (uint32_t)s->rank; P.world = (uint32_t)s->world;
  P.n_local_blocks = s->n_local_blocks; P.blocks_x = s->blocks_x;
  P.seed_lo = (uint32_t)seed; P.seed_hi = (uint32_t)(seed >> 32);
  int version = s->kernel_version ? s->kernel_version : 1;
  if (ad) version = 1;  // (the count map must not depend on the kernel variant: rounds always run the product kernel)
  // environment importance sampling: path-tracing renders run the ENV builds of the product kernel, whatever SOL_OPT_KERNEL says.
  // Counted renders are the creation probes here (sol_render_counted refuses while it is on); the other shaders read only the scatter's colour.
  const bool env = s->env_is && !count && s->S.shader == SOL_SHADER_PATH_TRACING;
  // light sampling modes 1 and 2, likewise: the LT builds. With one light they are mode 0's estimator (q_0 = 1), and the
  // default kernels run.
  const bool lt = s->light_mode != 0u && !count && s->S.shader == SOL_SHADER_PATH_TRACING && s->S.n_lights > 1u;
  if (env || lt) version = 1;
  // version 4, the pool kernel (sol_pool.hip): plain renders of the path-tracing... any shader; counted renders (probes, statistics) and trees
  // of 2^17 wide nodes or more (its one-dword node groups carry a 17-bit base) stay with the one-path-per-lane kernel
  if (version == 4 && ((count && !std::getenv("SOL_POOL_COUNT")) || s->tree.n_wide >= SOL_PACK_MAX_NODES)) version = 1;  // (SOL_POOL_COUNT: phase statistics of the pool kernel)
  // one launch of the pool kernel stages ONE COLOUR PER SAMPLE: a long sample range goes through several launches (chunk-aligned, so the sums
  // do not depend on the split), each within the staging budget
  if (version == 4) {
    const uint64_t pairs_per_chunk = (uint64_t)s->n_local_blocks;
    const uint64_t max_chunks = std::max<uint64_t>(1, std::min<uint64_t>((6ull << 30) / std::max<uint64_t>(1, pairs_per_chunk * 64u * SOL_CHUNK * 12u),
                                                                         (uint64_t)SOL_MAX_ITEMS / std::max<uint64_t>(1, pairs_per_chunk * 64u * SOL_CHUNK)));
    if (((uint64_t)n + SOL_CHUNK - 1) / SOL_CHUNK > max_chunks) {
      uint32_t f = first, left = n;
      while (left) {
        const uint32_t k = (uint32_t)std::min<uint64_t>(left, max_chunks * SOL_CHUNK);
        const int rc = sol_render_impl(s, f, k, seed, false);
        if (rc != SOL_OK) return rc;
        f += k; left -= k;
      }
      return SOL_OK;
    }
  }
  // Background blocks - the tail of the work order - are not traced: their sums are written by sol_fill_background_kernel. Counted
  // renders trace everything (their counters describe the whole algorithm; the creation probes are counted renders).
  P.n_traced_blocks = P.n_local_blocks;
  if (ad) P.n_traced_blocks = ad->n_traced;
  else if (version == 1 && (!count || s->background_in_counted) && s->background_enabled && s->S.block_order && s->n_background_local <= P.n_local_blocks)
    P.n_traced_blocks = P.n_local_blocks - s->n_background_local;
  const uint64_t items = (uint64_t)P.n_chunks * P.n_traced_blocks * 64u;
  DevScene Sv = s->S;  // the scene this launch renders: the work order is the active list in a round of adaptive sampling
  if (ad) { Sv.block_order = ad->order; Sv.n_first = ad->n_first; }
  SolSceneMirror& mirror = ad ? *ad->mirror : s->mirror;  // .. and has its own device copy
  // the 32-bit work counter keeps counting after the items run out (every wave adds 64 per refused fetch until all its
  // lanes have left): 16 M of headroom is > 100 times what 5120 resident waves can add
  if ((uint64_t)P.n_chunks * P.n_local_blocks * 64u > SOL_MAX_ITEMS) return sol_fail(SOL_EINVAL, "too many work items in one call (%llu): split the sample range", (unsigned long long)items);
  P.n_items = (uint32_t)items;
  if (P.n_local_blocks == 0) return SOL_OK;
  P.switch_below = s->switch_below;
  // Kernel choice. The product library carries ONE render kernel family, the one-path-per-lane kernel (version 1); the two
  // wavefront variants (2: wave-private pool, 3: two-kernel wavefront; bit-identical images) exist in -DSOL_AB_KERNELS builds for
  // A/B runs: they raise the search's lane occupancy (0.45 -> 0.67-0.73) but pay for it in state traffic, refill stalls and
  // per-round tails (MI355X, C3, 128 spp: v1 997, v2 905, v3 684 Msamples/s when they were last compared).
  if (version != 1 && version != 4 && s->strict_triangles) return sol_fail(SOL_EINVAL, "kernel variant %d does not implement the consistency rule of scenes with needle triangles", version);
#ifndef SOL_AB_KERNELS
  if (version != 1) return sol_fail(SOL_EINVAL, "kernel variant %d exists only in -DSOL_AB_KERNELS builds of the library", version);
  const int bpc = sol_render_blocks_per_cu(version, count, s->has_medium, s->strict_triangles, env, lt);
#else
  const int bpc = version == 3 ? sol_wf_trace_blocks_per_cu(count, s->has_medium) : sol_render_blocks_per_cu(version, count, s->has_medium, s->strict_triangles, env, lt);
#endif
  uint32_t lds_depth = (uint32_t)SOL_LDS_STACK;
  uint32_t stack_need = s->tree.depth;  // dwords of traversal stack a search of this scene can use
#ifdef SOL_AB_KERNELS
  // (swap_min: lanes waiting before an exchange pass of the search loop; 64 = only when the wave would otherwise leave for the service block, the best setting measured)
  if (version == 4) { lds_depth = (uint32_t)sol_pool4_lds_stack_depth(); stack_need = s->tree.packed_depth; P.swap_min = s->pool_swap_min ? s->pool_swap_min : 64u; }
  if (version == 3) lds_depth = (uint32_t)sol_wf_lds_stack_depth();
#endif
  uint32_t grid;
  int rc;
  if ((rc = sol_launch_plan(s, bpc, P.n_items, lds_depth, stack_need, s->spill, &grid))) return rc;
  P.total_threads = grid * SOL_WG;
#ifdef SOL_AB_KERNELS
  if (version == 3) {
    // one global pool: enough slots that the trace kernel has >= 16 rays per resident lane, never more than the items
    uint64_t want = std::min<uint64_t>(P.n_items, s->wf_slots);
    want = ((want + SOL_WG - 1) / SOL_WG) * SOL_WG;
    P.pool_slots = (uint32_t)want;
    // POOL_RECORDS float4 per slot; item reservoirs: one uint2 per 64 slots (shade wave)
    if ((rc = s->pool.reserve(s->stream, sol_wf_pool_bytes(P.pool_slots))) || (rc = s->queue.reserve(s->stream, P.pool_slots / 64)) || (rc = s->wf_ctr.reserve(s->stream, 16))) return rc;
    if (!s->wf_ctr_host) HIP_TRY(sol_pinned_alloc(s->wf_ctr_host, 16));
  } else if (version == 2) {
    // pool of path slots: per wave a multiple of 64, enough that every wave has several rays per lane in flight
    const uint32_t waves = grid * (SOL_WG / 64);
    uint32_t per_wave = (P.n_items + waves - 1) / waves;
    per_wave = ((per_wave + 63u) / 64u) * 64u;
    P.pool_slots = std::min<uint32_t>(SOL_POOL_MAX, std::max<uint32_t>(64u, per_wave));
    if (s->pool_slots_override) P.pool_slots = std::min<uint32_t>(SOL_POOL_MAX, ((s->pool_slots_override + 63u) / 64u) * 64u);
    if ((rc = s->pool.reserve(s->stream, sol_pool_bytes_per_wave(P.pool_slots) * waves))) return rc;
  }
#endif
  const size_t slots3 = (size_t)P.n_local_blocks * 64u * 3u;
  // Fine tail (v1): the last pairs (block, chunk) of the work order - all of them in the last chunk, blocks the probe found light -
  // are handed out one sample at a time: about one whole item per resident lane (SOL_FINE_TAIL quarters), so that single
  // samples are still on offer while the slowest lanes finish their last whole item. Counted launches keep whole items
  // (per-item ray counts).
  P.n_coarse = P.n_items;
  P.fine_count = n - (P.n_chunks - 1u) * SOL_CHUNK;
  P.stage_at = P.n_chunks * P.n_local_blocks * 64u;  // right behind the chunk sums (of every block, traced or not)
  size_t stage_floats = 0;
  const int fine_tail = s->fine_tail >= 0 ? s->fine_tail : s->fine_tail_auto;
  if (version == 4) {  // every pair (block, chunk) is handed out sample by sample: the staging area holds the whole launch
    const uint64_t pairs = (uint64_t)P.n_chunks * P.n_traced_blocks;
    const uint64_t total = pairs * 64u * SOL_CHUNK;
    if (total > SOL_MAX_ITEMS || (uint64_t)P.stage_at + total > 0xFFFFFFFFull) return sol_fail(SOL_EINVAL, "too many work items in one call (%llu): split the sample range", (unsigned long long)total);
    stage_floats = (size_t)total * 3u;
    P.n_coarse = 0;
    P.n_items = (uint32_t)total;
    // items per reservation of a wave's reservoir: a whole pair (1024 samples) when every resident wave gets at least 16 of them, else 64
    P.pool_slots = total >= (uint64_t)(P.total_threads / 64u) * 1024u * 16u ? 1024u : 64u;
  } else if (version == 1 && !count && fine_tail > 0) {
    const uint32_t rest = P.n_traced_blocks - std::min(P.n_traced_blocks, Sv.n_first);
    const uint32_t pairs = std::min<uint32_t>(rest, (uint32_t)(((uint64_t)fine_tail * (P.total_threads / 64u) + 3u) / 4u));
    const uint64_t total = items - (uint64_t)pairs * 64u + (uint64_t)pairs * 64u * SOL_CHUNK;
    if (pairs > 0 && total <= SOL_MAX_ITEMS && (uint64_t)P.stage_at + (uint64_t)pairs * 64u * SOL_CHUNK <= 0xFFFFFFFFull) {
      stage_floats = (size_t)pairs * 64u * SOL_CHUNK * 3u;
      P.n_coarse = (uint32_t)(items - (uint64_t)pairs * 64u);
      P.n_items = (uint32_t)total;
    }
  }
  // v1 writes every chunk sum into `partial` (also when the call has a single chunk); v2 / v3 add a single chunk straight
  // into the accumulator
  const bool via_partial = version == 1 || version == 4 || P.n_chunks > 1;
  if (via_partial) {
    if ((rc = s->partial.reserve(s->stream, slots3 * P.n_chunks + stage_floats))) return rc;
    // padding pixels of edge blocks are never written: keep them zero
    if ((s->S.width % SOL_TILE) || (s->S.height % SOL_TILE)) HIP_TRY(hipMemsetAsync(s->partial.get(), 0, slots3 * P.n_chunks * sizeof(float), s->stream));
  }
  HIP_TRY(hipMemsetAsync(s->work.get(), 0, sizeof(uint32_t), s->stream));
  if (count) HIP_TRY(hipMemsetAsync(s->counters.get(), 0, sizeof(DevCounters), s->stream));
  if (s->timing) HIP_TRY(hipEventRecord(s->ev_start, s->stream));
#ifdef SOL_AB_KERNELS
  if (version == 3) {
    // rounds of (shade, trace) until no slot holds work; the live-slot count is read back every few rounds
    uint32_t* ctr = s->wf_ctr.get();  // WfCounters {work_next, slot_cursor, live, pad}
    HIP_TRY(hipMemsetAsync(ctr, 0, 16, s->stream));
    HIP_TRY(hipMemsetAsync(s->pool.get() + (size_t)P.pool_slots * 16, 0, (size_t)P.pool_slots * 16, s->stream));  // record 1: flags
    HIP_TRY(hipMemsetAsync(s->queue.get(), 0, (size_t)P.pool_slots / 64 * 8, s->stream));                              // reservoirs
    const uint32_t check_every = 16;
    uint32_t rounds = 0;
    for (;;) {
      HIP_TRY(hipMemsetAsync(ctr + 1, 0, 8, s->stream));  // slot_cursor, live
      HIP_TRY(sol_launch_wf_shade(s->S, P, s->acc, s->partial.get(), ctr, s->pool.get(), s->queue.get(), s->counters.get(), count, s->stream));
      HIP_TRY(sol_launch_wf_trace(s->S, P, ctr, s->pool.get(), s->spill.get(), s->counters.get(), grid, count, s->has_medium, s->stream));
      ++rounds;
      if (rounds % check_every == 0) {
        HIP_TRY(hipMemcpyAsync(s->wf_ctr_host.get(), ctr, 16, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        if (s->wf_ctr_host.get()[2] == 0) break;
        if (rounds > 4000000u) return sol_fail(SOL_EDEVICE, "wavefront did not drain");
      }
    }
    s->last_rounds = rounds;
  } else
#endif
  {
    if ((rc = mirror.upload(s->stream, Sv))) return rc;
    if (P.n_items > 0)
      HIP_TRY(sol_launch_render(version, Sv, mirror.dev.get(), P, s->acc, s->partial.get(), s->work.get(), s->spill.get(), s->pool.get(), s->counters.get(), grid, count,
                                s->has_medium, stack_need > lds_depth, env, lt, s->stream));
    if (ad) {
      // the active background blocks are the last ad->n_background entries of the active list: the fill kernel writes the blocks
      // behind its n_traced_blocks
      if (ad->n_background) {
        RenderParams Q = P;
        Q.n_traced_blocks = P.n_local_blocks - ad->n_background;
        HIP_TRY(sol_launch_fill_background(mirror.dev.get(), Q, s->partial.get(), s->stream));
      }
    } else if (P.n_traced_blocks != P.n_local_blocks) {
      HIP_TRY(sol_launch_fill_background(mirror.dev.get(), P, s->partial.get(), s->stream));
    }
  }
  if (s->timing) { HIP_TRY(hipEventRecord(s->ev_stop, s->stream)); s->timed_launches++; }
  s->last_grid = grid;
  s->last_version = version;
  if (P.n_coarse != P.n_items) HIP_TRY(sol_launch_stage_resolve(mirror.dev.get(), P, s->partial.get(), s->stream));
  if (via_partial && !ad) HIP_TRY(sol_launch_resolve(s->acc, s->partial.get(), (uint32_t)slots3, P.n_chunks, s->stream));
  if (count) {
    DevCounters c;
    HIP_TRY(hipMemcpyAsync(&c, s->counters.get(), sizeof c, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->stats.samples = c.samples; s->stats.rays = c.rays; s->stats.node_visits = c.node_visits;
    s->stats.sphere_tests = c.sphere_tests; s->stats.quad_tests = c.quad_tests; s->stats.triangle_tests = c.triangle_tests;
    s->stats.shades = c.shades; s->stats.texel_fetches = c.texel_fetches; s->stats.max_stack = c.max_stack;
    for (int k = 0; k < 6; ++k) s->stats.phase[k] = c.phase[k];
    s->path_stats.size = sizeof(SolPathStats);
    s->path_stats.samples = c.samples; s->path_stats.primary_hits = c.primary_hits;
    for (int k = 0; k < 6; ++k) s->path_stats.path_len[k] = c.path_len[k];
  }
  return SOL_OK;
}

extern "C" {

int sol_render(SolScene* s, uint32_t first, uint32_t n, uint64_t seed) {
  if (s) s->adaptive.open = false;  // (ends an adaptive sampling session)
  return sol_render_impl(s, first, n, seed, false);
}
int sol_render_counted(SolScene* s, uint32_t first, uint32_t n, uint64_t seed) {
  if (s && s->env_is) return sol_fail(SOL_EINVAL, "sol_render_counted: the counted kernels do not implement environment importance sampling (sol_env_sampling mode 0 first)");
  if (s && s->light_mode) return sol_fail(SOL_EINVAL, "sol_render_counted: the counted kernels do not implement the light tree (sol_light_sampling mode 0 first)");
  if (s) s->adaptive.open = false;
  return sol_render_impl(s, first, n, seed, true);
}

// Auxiliary albedo / normal buffers (src/renderer/mod.rs:175-204): at depth 0 the reference evaluates AlbedoShader and
// NormalShader on the hit of the primary ray (background / zero on a miss) and accumulates them beside the pixel colour.
// Those are exactly the single-hit shaders of this library evaluated on the same primary ray - same (seed, pixel, sample)
// key, hence the same jitter and camera ray - so the two planes are two primary-ray-only renders into their own
// accumulators; no path-tracing kernel variant is needed. (For Blend materials the reference's extra scatter call draws its
// branch independently of the path's, as the separate render does.)
int sol_render_aux(SolScene* s, uint32_t first, uint32_t n, uint64_t seed) {
  if (!s) return sol_fail(SOL_EINVAL, "null scene");
  HIP_TRY(hipSetDevice(s->device));
  if (s->aux_floats != s->acc_floats || !s->aux[0]) {  // none yet, or planes of another partition's layout: new sums, all zero
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->aux_floats = 0;  // (no planes until both exist)
    for (int k = 0; k < 2; ++k) {
      if (const int rc = s->aux[k].reserve(s->stream, s->acc_floats)) return rc;
      HIP_TRY(hipMemsetAsync(s->aux[k].get(), 0, std::max<size_t>(s->acc_floats * sizeof(float), 64), s->stream));
    }
    s->aux_floats = s->acc_floats;
    s->aux_samples = 0;
  }
  float* const acc = s->acc;
  const uint32_t shader = s->S.shader;
  const uint32_t kinds[2] = {SOL_SHADER_ALBEDO, SOL_SHADER_NORMAL};
  int rc = SOL_OK;
  const float bg[3] = {s->S.bgx, s->S.bgy, s->S.bgz};
  const float* const env = s->S.env;
  for (int k = 0; k < 2 && rc == SOL_OK; ++k) {
    s->acc = s->aux[k].get();
    s->S.shader = kinds[k];
    if (k == 1) { s->S.bgx = s->S.bgy = s->S.bgz = 0.0f; s->S.env = nullptr; }  // a miss: albedo = background colour, normal = ZERO_VECTOR (mod.rs:197-204)
    rc = sol_render_impl(s, first, n, seed, false);
  }
  s->acc = acc;
  s->S.shader = shader;
  s->S.bgx = bg[0]; s->S.bgy = bg[1]; s->S.bgz = bg[2];
  s->S.env = env;
  if (rc == SOL_OK) s->aux_samples += n;
  return rc;
}

int sol_clear_aux(SolScene* s) {
  if (!s) return sol_fail(SOL_EINVAL, "null scene");
  HIP_TRY(hipSetDevice(s->device));
  for (int k = 0; k < 2; ++k)
    if (s->aux[k] && s->aux_floats == s->acc_floats) HIP_TRY(hipMemsetAsync(s->aux[k].get(), 0, s->aux_floats * sizeof(float), s->stream));
  s->aux_samples = 0;
  return SOL_OK;
}

int sol_read_aux(SolScene* s, float* albedo_sum, float* normal_sum) {
  if (!s || (!albedo_sum && !normal_sum)) return sol_fail(SOL_EINVAL, "null argument");
  if (!s->aux[0] || s->aux_floats != s->acc_floats) return sol_fail(SOL_EINVAL, "no auxiliary buffers: call sol_render_aux first");
  HIP_TRY(hipSetDevice(s->device));
  float* outs[2] = {albedo_sum, normal_sum};
  for (int k = 0; k < 2; ++k) {
    if (!outs[k]) continue;
    HIP_TRY(sol_launch_unpermute(s->aux[k].get(), s->image.get(), s->S.width, s->S.height, s->blocks_x, (uint32_t)s->world, (uint32_t)s->rank,
                                 s->acc_floats, s->slot_of_block.get(), s->stream));
    HIP_TRY(hipMemcpyAsync(outs[k], s->image.get(), (size_t)s->S.width * s->S.height * 3 * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  return SOL_OK;
}

int sol_eval(int device, uint32_t fn, const float* in, uint32_t n, uint32_t in_stride, float* out, uint32_t out_stride) {
  if (!in || !out || !in_stride || !out_stride) return sol_fail(SOL_EINVAL, "bad argument");
  // floats a row of sol_eval_kernel (sol_aux.hip) reads and writes, per function: a narrower stride would read and write past the device copies
  static const uint32_t row_in[9] = {3, 3, 5, 7, 13, 24, 17, 12, 4}, row_out[9] = {7, 5, 2, 18, 2, 4, 4, 2, 7};
  if (fn > 8u) return sol_fail(SOL_EINVAL, "sol_eval: unknown function %u", fn);
  if (in_stride < row_in[fn] || out_stride < row_out[fn])
    return sol_fail(SOL_EINVAL, "sol_eval: function %u reads %u and writes %u floats per row (strides %u / %u)", fn, row_in[fn], row_out[fn], in_stride, out_stride);
  if ((uint64_t)n * std::max(in_stride, out_stride) > (1ull << 32)) return sol_fail(SOL_EINVAL, "sol_eval: more than 2^32 floats");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return sol_fail(SOL_EDEVICE, "no HIP device available");
  HIP_TRY(hipSetDevice(device));
  DevPtr<float> din, dout;
  const size_t ib = (size_t)n * in_stride * sizeof(float), ob = (size_t)n * out_stride * sizeof(float);
  HIP_TRY(sol_dev_alloc(din, (size_t)n * in_stride));
  if (sol_dev_alloc(dout, (size_t)n * out_stride) != hipSuccess) return sol_fail(SOL_ENOMEM, "hipMalloc failed");
  hipError_t e = hipMemcpy(din.get(), in, ib, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout.get(), 0, std::max<size_t>(ob, 64));
  if (e == hipSuccess) e = sol_launch_eval(fn, din.get(), n, in_stride, dout.get(), out_stride, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout.get(), ob, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return sol_fail(SOL_EDEVICE, "sol_eval: %s", hipGetErrorString(e));
  return SOL_OK;
}

int sol_debug_path(SolScene* s, uint32_t x, uint32_t y, uint32_t sample, uint64_t seed, float* rows, uint32_t max_rows) {
  if (!s || !rows || max_rows < 2 || x >= s->S.width || y >= s->S.height) return sol_fail(SOL_EINVAL, "bad argument");
  if (s->env_is) return sol_fail(SOL_EINVAL, "sol_debug_path: follows the default estimator only (sol_env_sampling mode 0 first)");
  if (s->light_mode) return sol_fail(SOL_EINVAL, "sol_debug_path: follows the default estimator only (sol_light_sampling mode 0 first)");
  HIP_TRY(hipSetDevice(s->device));
  RenderParams P{};
  P.seed_lo = (uint32_t)seed; P.seed_hi = (uint32_t)(seed >> 32);
  P.total_threads = 1;
  DevPtr<float> dout;
  DevPtr<uint32_t> dspill;
  const size_t ob = (size_t)max_rows * 12 * sizeof(float);
  HIP_TRY(sol_dev_alloc(dout, (size_t)max_rows * 12));
  hipError_t e = sol_dev_alloc(dspill, (size_t)SOL_SPILL_STACK + 8);
  if (e == hipSuccess) e = hipMemset(dout.get(), 0, ob);
  if (e == hipSuccess) e = sol_launch_debug_path(s->S, P, x, y, sample, dspill.get(), dout.get(), max_rows, s->has_medium, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(rows, dout.get(), ob, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return sol_fail(SOL_EDEVICE, "sol_debug_path: %s", hipGetErrorString(e));
  for (uint32_t r = 0; r < max_rows && rows[r * 12 + 3] != -1.0f; ++r) {  // hit references: device order -> the caller's indices
    uint32_t ref;
    std::memcpy(&ref, &rows[r * 12 + 7], 4);
    const uint32_t kind = SOL_REF_KIND(ref);
    const int a = kind == SOL_REF_TRIANGLE ? 0 : kind == SOL_REF_SPHERE ? 1 : kind == SOL_REF_QUAD ? 2 : -1;  // (DevTree::old_index)
    if (a >= 0 && SOL_REF_INDEX(ref) < s->tree.old_index[a].size()) {
      ref = SOL_MAKE_REF(SOL_REF_KIND(ref), s->tree.old_index[a][SOL_REF_INDEX(ref)]);
      std::memcpy(&rows[r * 12 + 7], &ref, 4);
    }
  }
  return SOL_OK;
}

}  // extern "C"
