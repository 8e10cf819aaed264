// sol_gather.h -- what the radiance queries and every gather family built on them share on the host: the checks of their
// configuration, the shape of an entry point, the slice / window launch plan over SolScene::rad_* and the staged host route. The families
// (sol_api.cpp, sol_depth.cpp, sol_gather_adaptive.cpp) supply a description and the launches of their own kernels; nothing here allocates
// per launch - the callables are template parameters.
#pragma once
#include "sol_scene.h"

constexpr size_t SOL_GATHER_MAX_POINTS = (size_t)1 << 31;
constexpr size_t SOL_GATHER_STAGE_POINTS = (size_t)1 << 20;  // the host routes stage at most this many rays or points at a time (32 + 8 bytes each, and the answers)

// An irradiance query is a radiance query whose samples draw their own directions: one configuration layout - the last word is `reserved`
// for the one and `mode` for the other -, one set of checks, one launch.
enum SolRadianceKind { SOL_KIND_RADIANCE = 0, SOL_KIND_IRRADIANCE = 1, SOL_KIND_IRRADIANCE_RAYS = 2 };  // (the last: sol_irradiance_rays, one sample only)
// What every route refuses about the configuration and n; needs neither a device nor a handle: behind a non-null scene pointer both are judged
// before the handle is read for the first time.
int sol_radiance_config_check(const char* fn, SolRadianceKind kind, size_t n, const SolRadianceConfig* cfg);
// The two refusals the visibility gathers share with the ray queries, each in one sentence.
int sol_query_mode_check(const char* fn, int mode);
int sol_query_medium_check(const SolScene* s, const char* fn);

// The caller's configuration as the launches take it, or null; `as` is where a SolIrradianceConfig is converted to.
inline const SolRadianceConfig* sol_gather_config(const SolRadianceConfig* c, SolRadianceConfig&) { return c; }
inline const SolRadianceConfig* sol_gather_config(const SolIrradianceConfig* c, SolRadianceConfig& as) {
  if (!c) return nullptr;
  as = SolRadianceConfig{c->size, c->samples, c->first_sample, c->first_draw, c->seed, c->key_base, c->mode};
  return &as;
}
// An entry point of these families: check(cfg, &go) judges the arguments (cfg null: no configuration; go false: nothing to do, n == 0), then the
// device is looked for and made current, then run(cfg) launches. The order inside `check` is the family's own.
template <typename Config, typename Check, typename Run>
int sol_gather_entry(SolScene* s, const Config* config, Check&& check, Run&& run) {
  SolRadianceConfig as{};
  const SolRadianceConfig* cfg = sol_gather_config(config, as);
  bool go = false;
  int rc;
  if ((rc = check(cfg, &go)) || !go || (rc = sol_device_enter(s))) return rc;
  return run(*cfg);
}

// What differs between the families in the launch plan. Two shapes exist. Chunk sums (chunk_rows 1 or 2: radiance, irradiance, visibility): the
// trace kernel writes chunk_rows rows of rad_partial per (chunk, point) and a resolve kernel adds them up; a call of one chunk goes direct, without
// the buffer and the resolve. Per sample (chunk_rows 0: SH, moments, depth): the trace kernel writes one value per (sample, point), per_row of them
// to a row of rad_partial, and a projection kernel follows every launch; a launch is at least one group of 64 points over one chunk.
struct SolGatherPlan {
  int bpc;              // blocks per CU of the family's trace kernel
  uint32_t chunk_rows;  // chunk sums: rows per (chunk, point); 0: per sample
  uint32_t per_row;     // per sample: (sample, point) values to a row - 1 (a colour), 4 (a word)
  size_t out_stride;    // bytes of `out` per point
  uint32_t mode;        // RadianceParams::mode
};

// n <= 2^31 rays or points (and keys, or null) in device memory, n x out_stride bytes out, on the scene's stream. At most rad_partial_max_rows rows of
// the partial buffer per launch: the call is split over points in slices of whole groups of 64 (answers are per point) and, where the samples of
// one slice do not fit, over windows of whole chunks (the family's second kernel carries a point's sums from one window to the next in `out`: the
// same additions in the same order). Per window: window(const SolGatherWindow&) launches the family's trace kernel and its resolve or projection.
struct SolGatherWindow {
  RadianceParams P;
  bool may_spill;
  const void *points, *keys; void* out;  // of the slice's first point
  uint32_t grid;
  uint32_t samples;  // of this window (the call's last chunk may be short)
  bool first;        // the call's first window: nothing to carry on
};
template <typename Window>
int sol_gather_launch(SolScene* s, const SolGatherPlan& plan, const void* points_dev, const void* keys_dev, size_t n, const SolRadianceConfig& cfg, uint32_t key_base,
                      void* out_dev, Window&& window) {
  int rc;
  if ((rc = sol_scene_to_device(s))) return rc;
  const bool may_spill = s->tree.depth > (uint32_t)SOL_LDS_STACK;
  if ((rc = s->rad_work.reserve(s->stream, 1))) return rc;
  const bool sums = plan.chunk_rows != 0u;
  const size_t total_chunks = (size_t)(((uint64_t)cfg.samples + SOL_CHUNK - 1) / SOL_CHUNK);
  // (the clamp keeps n_items in 32 bits; rad_partial_max_rows is 2^24 or a positive int of SOL_RADIANCE_ROWS, so it changes no reachable value)
  const size_t bound = std::min<size_t>(s->rad_partial_max_rows, (size_t)1 << 31);
  const size_t max_rows = sums ? std::max<size_t>(64, bound / plan.chunk_rows) : 0;  // chunk sums: in (chunk, point) pairs
  const size_t units = std::max<size_t>(1, bound / ((size_t)64 * SOL_CHUNK));         // per sample: in groups of 64 points over one chunk
  const size_t win_chunks = std::min(total_chunks, sums ? max_rows / 64 : units);
  const size_t slice = !sums ? units / win_chunks * 64 : total_chunks == 1 ? n : std::max<size_t>(64, max_rows / win_chunks / 64 * 64);
  for (size_t at = 0; at < n; at += slice) {
    const size_t k = std::min(slice, n - at);
    SolGatherWindow w{};
    RadianceParams& P = w.P;
    w.may_spill = may_spill;
    P.n_rays = (uint32_t)k;
    P.n_groups = (uint32_t)((k + 63) / 64);
    P.end_sample = cfg.first_sample + cfg.samples;
    P.seed_lo = (uint32_t)cfg.seed; P.seed_hi = (uint32_t)(cfg.seed >> 32);
    P.key_base = key_base + (uint32_t)at;
    P.first_draw = cfg.first_draw;
    P.switch_below = s->switch_below;
    P.direct = sums && total_chunks == 1 ? 1u : 0u;
    P.mode = plan.mode;
    w.points = (const char*)points_dev + at * sizeof(SolRay);
    w.keys = keys_dev ? (const char*)keys_dev + at * sizeof(SolRayKey) : nullptr;
    w.out = (char*)out_dev + at * plan.out_stride;
    const size_t rows = sums ? (size_t)P.n_groups * 64 * win_chunks * plan.chunk_rows
                             : ((size_t)P.n_groups * 64 * std::min<size_t>(win_chunks * SOL_CHUNK, cfg.samples) + plan.per_row - 1) / plan.per_row;
    if (!P.direct && (rc = s->rad_partial.reserve(s->stream, rows))) return rc;
    for (size_t c0 = 0; c0 < total_chunks; c0 += win_chunks) {
      P.n_chunks = (uint32_t)std::min(win_chunks, total_chunks - c0);
      P.first_sample = cfg.first_sample + (uint32_t)(c0 * SOL_CHUNK);
      w.samples = std::min<uint32_t>(P.n_chunks * (uint32_t)SOL_CHUNK, P.end_sample - P.first_sample);
      w.first = c0 == 0;
      // (<= 2^31 and <= the rows of the partial buffer: far below the headroom of the 32-bit work counter, SOL_MAX_ITEMS)
      const uint64_t items = (uint64_t)(sums ? P.n_chunks : w.samples) * P.n_groups * 64u;
      P.n_items = (uint32_t)items;
      // the grid and the spill tail of THIS launch (the render launch's area is sized for another)
      if ((rc = sol_launch_plan(s, plan.bpc, items, SOL_LDS_STACK, s->tree.depth, s->rad_spill, &w.grid))) return rc;
      P.total_threads = w.grid * SOL_WG;
      HIP_TRY(hipMemsetAsync(s->rad_work.get(), 0, sizeof(uint32_t), s->stream));
      if ((rc = window(w))) return rc;
    }
  }
  return SOL_OK;
}

// The host route: n rays or points (and keys, or null) of the caller's arrays staged through rad_in / rad_keys, at most `cap` at a time, their
// answers of out_stride bytes each through rad_out (whole SolRadiance rows per point); launch(points_dev, keys_dev, k, key_base, out_dev) runs the
// family's device route over one batch, key_base being the key of its first point when there are no keys. Blocks.
template <typename Launch>
int sol_gather_stage(SolScene* s, const SolRay* points, const SolRayKey* keys, size_t n, size_t cap, void* out, size_t out_stride, uint32_t key_base, Launch&& launch) {
  int rc;
  cap = std::min(n, cap);
  const size_t rows = (out_stride + sizeof(SolRadiance) - 1) / sizeof(SolRadiance);
  if ((rc = s->rad_in.reserve(s->stream, cap)) || (rc = s->rad_keys.reserve(s->stream, cap)) || (rc = s->rad_out.reserve(s->stream, cap * rows))) return rc;
  for (size_t at = 0; at < n; at += cap) {  // (answers are per point: the split changes nothing)
    const size_t k = std::min(cap, n - at);
    HIP_TRY(hipMemcpyAsync(s->rad_in.get(), points + at, k * sizeof(SolRay), hipMemcpyHostToDevice, s->stream));
    if (keys) HIP_TRY(hipMemcpyAsync(s->rad_keys.get(), keys + at, k * sizeof(SolRayKey), hipMemcpyHostToDevice, s->stream));
    if ((rc = launch(s->rad_in.get(), keys ? s->rad_keys.get() : nullptr, k, key_base + (uint32_t)at, s->rad_out.get()))) return rc;
    HIP_TRY(hipMemcpyAsync((char*)out + at * out_stride, s->rad_out.get(), k * out_stride, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  return SOL_OK;
}

// The launches of the per-sample colour gathers over n <= 2^31 points in device memory: n SolSh9 out (sol_irradiance_sh) or, moments,
// n SolMoments (sol_irradiance_moments). carry, total_samples (moments only): a later round of an adaptive gather -
// `out` holds the rows' sums of the earlier rounds, so that the projection accumulates from the first window on, and the rows' count is their new
// total rather than this call's samples.
int sol_irradiance_each_launch(SolScene* s, const void* points_dev, const void* keys_dev, size_t n, const SolRadianceConfig& cfg, uint32_t key_base, void* out_dev,
                               bool moments, bool carry = false, uint32_t total_samples = 0);
