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

// ---- the steps of a render launch (sol_scene.h), shared with the A/B variants of sol_launch_ab.cpp ----
int sol_render_params(const SolScene* s, const SolRenderJob& job, uint32_t n_traced, RenderParams& P) {
  P = RenderParams{};
  P.first_sample = job.first; P.n_samples = job.n;
  P.n_chunks = (uint32_t)(((uint64_t)job.n + SOL_CHUNK - 1) / SOL_CHUNK);  // (in 64 bits: n + 15 wraps for the last fifteen values of n)
  P.rank = (uint32_t)s->rank; P.world = (uint32_t)s->world;
  P.n_local_blocks = s->n_local_blocks; P.blocks_x = s->blocks_x;
  P.seed_lo = (uint32_t)job.seed; P.seed_hi = (uint32_t)(job.seed >> 32);
  P.n_traced_blocks = n_traced;
  const uint64_t items = (uint64_t)P.n_chunks * P.n_traced_blocks * 64u;
  // the 32-bit work counter keeps counting after the items run out (every wave adds 64 per refused fetch until all its
  // lanes have left): 16 M of headroom is > 100 times what 5120 resident waves can add
  if ((uint64_t)P.n_chunks * P.n_local_blocks * 64u > SOL_MAX_ITEMS) return sol_fail(SOL_EINVAL, "too many work items in one call (%llu): split the sample range", (unsigned long long)items);
  P.n_items = (uint32_t)items;
  P.switch_below = s->switch_below;
  // whole items only, until the caller decides on a fine tail (n_coarse: the items handed out whole; the rest one sample at a time)
  P.n_coarse = P.n_items;
  P.fine_count = job.n - (P.n_chunks - 1u) * SOL_CHUNK;
  P.stage_at = P.n_chunks * P.n_local_blocks * 64u;  // right behind the chunk sums (of every block, traced or not)
  return SOL_OK;
}
int sol_render_partial(SolScene* s, const RenderParams& P, size_t stage_floats) {
  const size_t sums = (size_t)P.n_local_blocks * 64u * 3u * P.n_chunks;
  if (const int rc = s->partial.reserve(s->stream, sums + stage_floats)) return rc;
  // padding pixels of edge blocks are never written: keep them zero
  if ((s->S.width % SOL_TILE) || (s->S.height % SOL_TILE)) HIP_TRY(hipMemsetAsync(s->partial.get(), 0, sums * sizeof(float), s->stream));
  return SOL_OK;
}
int sol_render_begin(SolScene* s, bool count) {
  HIP_TRY(hipMemsetAsync(s->work.get(), 0, sizeof(uint32_t), s->stream));
  if (count) HIP_TRY(hipMemsetAsync(s->counters.get(), 0, sizeof(DevCounters), s->stream));
  if (s->timing) HIP_TRY(hipEventRecord(s->ev_start, s->stream));
  return SOL_OK;
}
int sol_render_end(SolScene* s, const SolRenderJob& job, const RenderParams& P, uint32_t grid, bool via_partial) {
  if (s->timing) { HIP_TRY(hipEventRecord(s->ev_stop, s->stream)); s->timed_launches++; }
  s->last_grid = grid;
  if (P.n_coarse != P.n_items) HIP_TRY(sol_launch_stage_resolve(job.mirror->dev.get(), P, s->partial.get(), s->stream));
  if (via_partial && !job.round) HIP_TRY(sol_launch_resolve(job.acc, s->partial.get(), P.n_local_blocks * 64u * 3u, P.n_chunks, s->stream));
  if (job.count) {
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

// One launch of the product render kernel (sol_render.hip: one path per lane) over job.view, uploaded to job.mirror, its sums added to job.acc.
// A round of adaptive sampling (job.round) traces the active list that is its view's work order and leaves the chunk sums in `partial` for
// sol_adaptive_round.
int sol_render_impl(SolScene* s, const SolRenderJob& job) {
  if (!s) return sol_fail(SOL_EINVAL, "null scene");
  if (job.n == 0) return SOL_OK;
  if ((uint64_t)job.first + job.n > 0xFFFFFFFFull) return sol_fail(SOL_EINVAL, "sample range overflows 32 bits");
  HIP_TRY(hipSetDevice(s->device));
  const DevScene& Sv = job.view;
  const bool count = job.count, strict = Sv.tri_delta > 0.0f;  // (strict: the scene has needle triangles, SolScene::strict_triangles)
  const SolEstimator est = sol_estimator(s, Sv, count);
  // Kernel choice. The product library carries ONE render kernel family, the one-path-per-lane kernel (variant 1). Variants 2 (wave-private
  // pool), 3 (two-kernel wavefront) and 4 (the pool kernel) - bit-identical images, measured slower: DESIGN.md 9 - exist in the A/B build of
  // the library, behind the one seam below. Rounds of adaptive sampling (the count map must not depend on the variant) and the ENV / LT
  // estimators always run the product kernel; so do, under variant 4, counted renders (probes, statistics) and trees of 2^17 wide nodes or
  // more (its one-dword node groups carry a 17-bit base).
  int version = s->kernel_version ? s->kernel_version : 1;
  if (job.round || est.env || est.lt) version = 1;
  if (version == 4 && ((count && !s->pool_count) || s->tree.n_wide >= SOL_PACK_MAX_NODES)) version = 1;
  if (version != 1 && version != 4 && strict) return sol_fail(SOL_EINVAL, "kernel variant %d does not implement the consistency rule of scenes with needle triangles", version);
#ifdef SOL_AB_KERNELS
  if (version != 1) return sol_render_ab(s, job, version);
#else
  if (version != 1) return sol_fail(SOL_EINVAL, "kernel variant %d exists only in -DSOL_AB_KERNELS builds of the library", version);
#endif
  // Background blocks - the tail of the work order - are not traced: their sums are written by sol_fill_background_kernel. Counted
  // renders trace everything (their counters describe the whole algorithm; the creation probes are counted renders).
  const uint32_t n_filled = job.round ? job.n_background : (!count || s->background_in_counted) ? sol_background_tail(s, Sv) : 0u;
  RenderParams P;
  int rc;
  if ((rc = sol_render_params(s, job, job.round ? job.n_traced : s->n_local_blocks - n_filled, P))) return rc;
  if (P.n_local_blocks == 0) return SOL_OK;
  const uint32_t stack_need = s->tree.depth;  // dwords of traversal stack a search of this scene can use
  uint32_t grid;
  if ((rc = sol_launch_plan(s, sol_render_blocks_per_cu(count, s->has_medium, strict, est.env, est.lt), P.n_items, SOL_LDS_STACK, stack_need, s->spill, &grid))) return rc;
  P.total_threads = grid * SOL_WG;
  // Fine tail: the last pairs (block, chunk) of the work order - all of them in the last chunk, blocks the probe found light -
  // are handed out one sample at a time: about one whole item per resident lane (SOL_FINE_TAIL quarters), so that single
  // samples are still on offer while the slowest lanes finish their last whole item. Counted launches keep whole items
  // (per-item ray counts).
  size_t stage_floats = 0;
  const int fine_tail = s->fine_tail >= 0 ? s->fine_tail : s->fine_tail_auto;
  if (!count && fine_tail > 0) {
    const uint64_t items = P.n_items;
    const uint32_t rest = P.n_traced_blocks - std::min(P.n_traced_blocks, Sv.n_first);
    const uint32_t pairs = std::min<uint32_t>(rest, (uint32_t)(((uint64_t)fine_tail * (P.total_threads / 64u) + 3u) / 4u));
    const uint64_t total = items - (uint64_t)pairs * 64u + (uint64_t)pairs * 64u * SOL_CHUNK;
    if (pairs > 0 && total <= SOL_MAX_ITEMS && (uint64_t)P.stage_at + (uint64_t)pairs * 64u * SOL_CHUNK <= 0xFFFFFFFFull) {
      stage_floats = (size_t)pairs * 64u * SOL_CHUNK * 3u;
      P.n_coarse = (uint32_t)(items - (uint64_t)pairs * 64u);
      P.n_items = (uint32_t)total;
    }
  }
  // the kernel writes every chunk sum into `partial` (also when the call has a single chunk)
  if ((rc = sol_render_partial(s, P, stage_floats)) || (rc = sol_render_begin(s, count)) || (rc = job.mirror->upload(s->stream, Sv))) return rc;
  const DevScene* const dS = job.mirror->dev.get();
  if (P.n_items > 0)
    HIP_TRY(sol_launch_render(dS, P, job.acc, s->partial.get(), s->work.get(), s->spill.get(), s->counters.get(), grid, count, s->has_medium,
                              stack_need > (uint32_t)SOL_LDS_STACK, strict, est.env, est.lt, s->stream));
  if (n_filled) {  // the fill kernel writes the blocks behind its n_traced_blocks: the last n_filled entries of the work order
    RenderParams Q = P;
    Q.n_traced_blocks = P.n_local_blocks - n_filled;
    HIP_TRY(sol_launch_fill_background(dS, Q, s->partial.get(), s->stream));
  }
  return sol_render_end(s, job, P, grid, true);
}

extern "C" {

int sol_render(SolScene* s, uint32_t first, uint32_t n, uint64_t seed) {
  if (!s) return sol_fail(SOL_EINVAL, "null scene");
  s->adaptive.open = false;  // (ends an adaptive sampling session)
  return sol_render_impl(s, sol_render_job(s, first, n, seed, false));
}
int sol_render_counted(SolScene* s, uint32_t first, uint32_t n, uint64_t seed) {
  if (s && s->env_is) return sol_fail(SOL_EINVAL, "sol_render_counted: the counted kernels do not implement environment importance sampling (sol_env_sampling mode 0 first)");
  if (s && s->light_mode) return sol_fail(SOL_EINVAL, "sol_render_counted: the counted kernels do not implement the light tree (sol_light_sampling mode 0 first)");
  if (!s) return sol_fail(SOL_EINVAL, "null scene");
  s->adaptive.open = false;
  return sol_render_impl(s, sol_render_job(s, first, n, seed, true));
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
  // two views of the scene, each into its own accumulator; both through the handle's device copy
  const uint32_t kinds[2] = {SOL_SHADER_ALBEDO, SOL_SHADER_NORMAL};
  int rc = SOL_OK;
  for (int k = 0; k < 2 && rc == SOL_OK; ++k) {
    SolRenderJob job = sol_render_job(s, first, n, seed, false);
    job.acc = s->aux[k].get();
    job.view.shader = kinds[k];
    if (k == 1) { job.view.bgx = job.view.bgy = job.view.bgz = 0.0f; job.view.env = nullptr; }  // a miss: albedo = background colour, normal = ZERO_VECTOR (mod.rs:197-204)
    rc = sol_render_impl(s, job);
  }
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
  if (const int rc = sol_device_check()) return rc;
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
