// sol_gather_adaptive.cpp -- sol_irradiance_adaptive and sol_radiance_rescale (include/solstrale_hip.h): an irradiance-moments gather
// in rounds over the points still active (kernels: sol_gather_adaptive.hip; the stop rule: sol_gather_adaptive.h). Round 0 is sol_irradiance_moments's
// launch over the caller's own points, written into the caller's rows; a later round is the same launch over the compact rows the handle owns, with
// the projection carrying the rows' sums on (sol_irradiance_each_launch, sol_gather.cpp), followed by the write-back to the caller's rows. After
// every round: judge, scan, one read-back of four counters, and - while rows go on - the scatter. Every refusal is decided before the device is
// looked for.
#include <cmath>

#include "sol_gather.h"

namespace {
constexpr size_t RESCALE_STAGE_ROWS = (size_t)1 << 20;  // sol_radiance_rescale's host route stages at most this many rows at a time

// In the header's order. *go = false: nothing to do (n == 0).
int adaptive_check(const SolScene* s, const char* fn, const void* points, size_t n, const SolRadianceConfig* cfg, const SolGatherAdaptive* a, const void* out,
                   const SolGatherAdaptiveStats* stats, bool* go) {
  *go = false;
  if (!s) return sol_fail(SOL_EINVAL, "%s: null scene", fn);
  if (const int rc = sol_radiance_config_check(fn, SOL_KIND_IRRADIANCE, n, cfg)) return rc;
  if (!a) return sol_fail(SOL_EINVAL, "%s: null adaptive configuration", fn);
  if (a->size != sizeof(SolGatherAdaptive)) return sol_fail(SOL_EINVAL, "%s: SolGatherAdaptive.size is %u, not %zu", fn, a->size, sizeof(SolGatherAdaptive));
  if (a->reserved != 0u) return sol_fail(SOL_EINVAL, "%s: SolGatherAdaptive.reserved must be 0", fn);
  if (a->round == 0u || a->round % SOL_CHUNK != 0u) return sol_fail(SOL_EINVAL, "%s: round is %u: a positive multiple of %d", fn, a->round, SOL_CHUNK);
  if (a->min_samples % SOL_CHUNK != 0u) return sol_fail(SOL_EINVAL, "%s: min_samples is %u: a multiple of %d", fn, a->min_samples, SOL_CHUNK);
  if (!(std::isfinite(a->threshold) && a->threshold >= 0.0f)) return sol_fail(SOL_EINVAL, "%s: threshold %g (finite, >= 0; 0 never converges)", fn, (double)a->threshold);
  if (!(std::isfinite(a->floor) && a->floor >= 0.0f)) return sol_fail(SOL_EINVAL, "%s: floor %g (finite, >= 0)", fn, (double)a->floor);
  if (stats && stats->size != sizeof(SolGatherAdaptiveStats))
    return sol_fail(SOL_EINVAL, "%s: SolGatherAdaptiveStats.size is %u, not %zu", fn, stats->size, sizeof(SolGatherAdaptiveStats));
  if (n == 0) return SOL_OK;
  if (const int rc = sol_query_medium_check(s, fn)) return rc;
  if (!points || !out) return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !points ? "point" : "output");
  *go = true;
  return SOL_OK;
}

struct Tally { uint32_t rounds = 0; uint64_t paths = 0, valid = 0, converged = 0, capped = 0; };

// n <= ga_max_rows points of the call, from point `key_base - cfg.key_base` on: every round of them, to the end. Blocks.
int adaptive_part(SolScene* s, const void* points, const void* keys, size_t n, const SolRadianceConfig& cfg, uint32_t key_base, const SolGatherAdaptive& a, void* out,
                  Tally& tally) {
  int rc;
  const uint32_t max_samples = cfg.samples;
  const size_t n_wg = (n + 255) / 256;
  if (!s->ga_ctr_host) HIP_TRY(sol_pinned_alloc(s->ga_ctr_host, 4));
  if ((rc = s->ga_ctr.reserve(s->stream, 4)) || (rc = s->ga_scan.reserve(s->stream, 10 * n_wg))) return rc;
  if (max_samples > a.round &&  // (a second round may run)
      ((rc = s->ga_index.reserve(s->stream, 2 * n)) || (rc = s->ga_points.reserve(s->stream, n)) || (rc = s->ga_keys.reserve(s->stream, n)) ||
       (rc = s->ga_totals.reserve(s->stream, n))))
    return rc;
  uint32_t* const ballots = s->ga_scan.get();
  uint32_t* const wg_counts = ballots + 8 * n_wg;
  uint32_t* const wg_offsets = wg_counts + n_wg;
  uint32_t* const ctr = s->ga_ctr.get();
  volatile uint32_t* const host = s->ga_ctr_host.get();
  HIP_TRY(hipMemsetAsync(ctr, 0, 4 * sizeof(uint32_t), s->stream));

  SolRadianceConfig round_cfg = cfg;
  round_cfg.samples = (uint32_t)std::min<uint64_t>(a.round, max_samples);
  if ((rc = sol_irradiance_each_launch(s, points, keys, n, round_cfg, key_base, out, true))) return rc;
  uint32_t n_active = (uint32_t)n, rounds = 0;
  for (uint64_t k = 0;; ++k) {
    const uint32_t count = (uint32_t)std::min<uint64_t>((k + 1) * a.round, max_samples);  // what every active row holds now
    rounds++;
    HIP_TRY(sol_launch_gather_judge(k == 0 ? out : (const void*)s->ga_totals.get(), n_active, max_samples, a.min_samples, a.threshold, a.floor, ballots, wg_counts,
                                    wg_offsets, ctr, s->stream));
    HIP_TRY(hipMemcpyAsync((void*)host, ctr, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const uint32_t n_next = host[0];
    const uint32_t judged = k == 0 ? n_active - host[1] : n_active;  // (rows without samples are in round 0's list only)
    if (k == 0) tally.valid += judged;
    if (n_next > judged || (count == max_samples && n_next != 0u))  // (the rule stops every row at the maximum: the rounds end)
      return sol_fail(SOL_EDEVICE, "sol_irradiance_adaptive: the compaction counted %u of %u rows active at %u of %u samples", n_next, judged, count, max_samples);
    tally.paths += (uint64_t)(judged - n_next) * count;
    if (n_next == 0u) break;
    uint32_t* const index_in = k == 0 ? nullptr : s->ga_index.get() + (k & 1) * n;
    uint32_t* const index_out = s->ga_index.get() + ((k + 1) & 1) * n;
    HIP_TRY(sol_launch_gather_scatter(n_active, index_in, ballots, wg_offsets, points, keys, key_base, cfg.first_draw, out, n_next, index_out, s->ga_points.get(),
                                      s->ga_keys.get(), s->ga_totals.get(), s->stream));
    n_active = n_next;
    const uint64_t done = (k + 1) * a.round;  // (< max_samples: rows went on)
    round_cfg.first_sample = cfg.first_sample + (uint32_t)done;
    round_cfg.samples = (uint32_t)std::min<uint64_t>(a.round, max_samples - done);
    if ((rc = sol_irradiance_each_launch(s, s->ga_points.get(), s->ga_keys.get(), n_active, round_cfg, 0u, s->ga_totals.get(), true, true, (uint32_t)done + round_cfg.samples)))
      return rc;
    HIP_TRY(sol_launch_gather_writeback(n_active, index_out, s->ga_totals.get(), out, s->stream));
  }
  tally.rounds = std::max(tally.rounds, rounds);
  tally.converged += host[2];
  tally.capped += host[3];
  return SOL_OK;
}

// n points in device memory; split over points beyond the bound of the compact buffers (answers are per point).
int adaptive_launch(SolScene* s, const void* points, const void* keys, size_t n, const SolRadianceConfig& cfg, uint32_t key_base, const SolGatherAdaptive& a, void* out,
                    Tally& tally) {
  int rc;
  const size_t cap = std::max<size_t>(1, s->ga_max_rows);
  for (size_t at = 0; at < n; at += cap) {
    const size_t k = std::min(cap, n - at);
    if ((rc = adaptive_part(s, (const char*)points + at * sizeof(SolRay), keys ? (const char*)keys + at * sizeof(SolRayKey) : nullptr, k, cfg, key_base + (uint32_t)at, a,
                            (char*)out + at * sizeof(SolMoments), tally)))
      return rc;
  }
  return SOL_OK;
}

// Both routes: the checks, the device, `run` with the tally of its rounds, and - also when there was nothing to do - the statistics.
template <typename Run>
int adaptive_entry(SolScene* s, const char* fn, const void* points, size_t n, const SolIrradianceConfig* config, const SolGatherAdaptive* a, const void* out,
                   SolGatherAdaptiveStats* stats, Run&& run) {
  Tally t;
  const int rc = sol_gather_entry(s, config, [&](const SolRadianceConfig* c, bool* go) { return adaptive_check(s, fn, points, n, c, a, out, stats, go); },
                                  [&](const SolRadianceConfig& cfg) { return run(cfg, t); });
  if (rc != SOL_OK || !stats) return rc;
  stats->rounds = t.rounds;
  stats->paths = t.paths;
  stats->rows_valid = t.valid;
  stats->rows_converged = t.converged;
  stats->rows_capped = t.capped;
  return SOL_OK;
}

int rescale_check(bool have_scene, const char* fn, const void* rows, size_t n, uint32_t target, const void* out) {
  if (!have_scene) return sol_fail(SOL_EINVAL, "%s: null scene", fn);
  if (target == 0u) return sol_fail(SOL_EINVAL, "%s: target_samples is 0", fn);
  if (n > 0 && (!rows || !out)) return sol_fail(SOL_EINVAL, "%s: null %s pointer", fn, !rows ? "row" : "output");
  return SOL_OK;
}
}  // namespace

extern "C" {

int sol_irradiance_adaptive_dev(SolScene* s, const void* points_dev, const void* keys_dev, size_t n, const SolIrradianceConfig* config, const SolGatherAdaptive* adaptive,
                                void* moments_out_dev, SolGatherAdaptiveStats* stats) {
  return adaptive_entry(s, "sol_irradiance_adaptive_dev", points_dev, n, config, adaptive, moments_out_dev, stats, [&](const SolRadianceConfig& cfg, Tally& tally) {
    return adaptive_launch(s, points_dev, keys_dev, n, cfg, cfg.key_base, *adaptive, moments_out_dev, tally);
  });
}

int sol_irradiance_adaptive(SolScene* s, const SolRay* points, const SolRayKey* keys, size_t n, const SolIrradianceConfig* config, const SolGatherAdaptive* adaptive,
                            SolMoments* out, SolGatherAdaptiveStats* stats) {
  return adaptive_entry(s, "sol_irradiance_adaptive", points, n, config, adaptive, out, stats, [&](const SolRadianceConfig& cfg, Tally& tally) {
    return sol_gather_stage(s, points, keys, n, SOL_GATHER_STAGE_POINTS, out, sizeof(SolMoments), cfg.key_base,
                            [&](const void* p, const void* k, size_t m, uint32_t key_base, void* o) { return adaptive_launch(s, p, k, m, cfg, key_base, *adaptive, o, tally); });
  });
}

int sol_radiance_rescale_dev(SolScene* s, const void* rows_dev, size_t n, uint32_t target_samples, void* out_dev) {
  int rc;
  if ((rc = rescale_check(s != nullptr, "sol_radiance_rescale_dev", rows_dev, n, target_samples, out_dev)) || n == 0 || (rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(sol_launch_radiance_rescale(rows_dev, n, target_samples, out_dev, s->stream));
  return SOL_OK;
}

int sol_radiance_rescale(SolScene* s, const SolRadiance* rows, size_t n, uint32_t target_samples, SolRadiance* out) {
  int rc;
  if ((rc = rescale_check(s != nullptr, "sol_radiance_rescale", rows, n, target_samples, out)) || n == 0 || (rc = sol_device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const size_t cap = std::min(n, RESCALE_STAGE_ROWS);
  if ((rc = s->lm_stage.reserve(s->stream, cap * sizeof(SolRadiance)))) return rc;
  for (size_t at = 0; at < n; at += cap) {
    const size_t k = std::min(cap, n - at);
    HIP_TRY(hipMemcpyAsync(s->lm_stage.get(), rows + at, k * sizeof(SolRadiance), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(sol_launch_radiance_rescale(s->lm_stage.get(), k, target_samples, s->lm_stage.get(), s->stream));
    HIP_TRY(hipMemcpyAsync(out + at, s->lm_stage.get(), k * sizeof(SolRadiance), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  return SOL_OK;
}

}  // extern "C"
