// sol_gather_adaptive.cpp -- sol_irradiance_adaptive and sol_radiance_rescale (include/solstrale_hip.h): an irradiance-moments gather
// in rounds over the points still active (kernels: sol_gather_adaptive.hip; the stop rule: sol_gather_adaptive.h). Round 0 is sol_irradiance_moments's
// launch over the caller's own points, written into the caller's rows; a later round is the same launch over the compact rows the handle owns, with
// the projection carrying the rows' sums on (sol_irradiance_moments_launch, sol_api.cpp), followed by the write-back to the caller's rows. After
// every round: judge, scan, one read-back of four counters, and - while rows go on - the scatter. Every refusal is decided before the device is
// looked for.
#include <cmath>

#include "sol_scene.h"

namespace {
constexpr size_t STAGE_ROWS = (size_t)1 << 20;  // the host routes stage at most this many rows at a time

int device_check() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return sol_fail(SOL_EDEVICE, "no HIP device available");
  return SOL_OK;
}

// In the header's order. *go = false: nothing to do (n == 0). *cfg: the gather's configuration as the launches take it.
int adaptive_check(const SolScene* s, const char* fn, const void* points, size_t n, const SolIrradianceConfig* config, const SolGatherAdaptive* a, const void* out,
                   const SolGatherAdaptiveStats* stats, SolRadianceConfig* cfg, bool* go) {
  *go = false;
  if (!s) return sol_fail(SOL_EINVAL, "%s: null scene", fn);
  if (const int rc = sol_gather_config_check(fn, n, config, cfg)) return rc;
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
  if ((rc = sol_irradiance_moments_launch(s, points, keys, n, round_cfg, key_base, out, false, 0))) return rc;
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
    if ((rc = sol_irradiance_moments_launch(s, s->ga_points.get(), s->ga_keys.get(), n_active, round_cfg, 0u, s->ga_totals.get(), true, (uint32_t)done + round_cfg.samples)))
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

void stats_of(const Tally& t, SolGatherAdaptiveStats* stats) {
  if (!stats) return;
  stats->rounds = t.rounds;
  stats->paths = t.paths;
  stats->rows_valid = t.valid;
  stats->rows_converged = t.converged;
  stats->rows_capped = t.capped;
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
  int rc;
  bool go;
  SolRadianceConfig cfg{};
  if ((rc = adaptive_check(s, "sol_irradiance_adaptive_dev", points_dev, n, config, adaptive, moments_out_dev, stats, &cfg, &go))) return rc;
  Tally tally;
  if (go) {
    if ((rc = device_check())) return rc;
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = adaptive_launch(s, points_dev, keys_dev, n, cfg, cfg.key_base, *adaptive, moments_out_dev, tally))) return rc;
  }
  stats_of(tally, stats);
  return SOL_OK;
}

int sol_irradiance_adaptive(SolScene* s, const SolRay* points, const SolRayKey* keys, size_t n, const SolIrradianceConfig* config, const SolGatherAdaptive* adaptive,
                            SolMoments* out, SolGatherAdaptiveStats* stats) {
  int rc;
  bool go;
  SolRadianceConfig cfg{};
  if ((rc = adaptive_check(s, "sol_irradiance_adaptive", points, n, config, adaptive, out, stats, &cfg, &go))) return rc;
  Tally tally;
  if (go) {
    if ((rc = device_check())) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t cap = std::min(n, STAGE_ROWS);
    if ((rc = s->rad_in.reserve(s->stream, cap)) || (rc = s->rad_keys.reserve(s->stream, cap)) || (rc = s->rad_out.reserve(s->stream, cap * 2))) return rc;
    for (size_t at = 0; at < n; at += cap) {  // (answers are per point: the split changes nothing)
      const size_t k = std::min(cap, n - at);
      HIP_TRY(hipMemcpyAsync(s->rad_in.get(), points + at, k * sizeof(SolRay), hipMemcpyHostToDevice, s->stream));
      if (keys) HIP_TRY(hipMemcpyAsync(s->rad_keys.get(), keys + at, k * sizeof(SolRayKey), hipMemcpyHostToDevice, s->stream));
      if ((rc = adaptive_launch(s, s->rad_in.get(), keys ? s->rad_keys.get() : nullptr, k, cfg, cfg.key_base + (uint32_t)at, *adaptive, s->rad_out.get(), tally))) return rc;
      HIP_TRY(hipMemcpyAsync(out + at, s->rad_out.get(), k * sizeof(SolMoments), hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipStreamSynchronize(s->stream));
    }
  }
  stats_of(tally, stats);
  return SOL_OK;
}

int sol_radiance_rescale_dev(SolScene* s, const void* rows_dev, size_t n, uint32_t target_samples, void* out_dev) {
  int rc;
  if ((rc = rescale_check(s != nullptr, "sol_radiance_rescale_dev", rows_dev, n, target_samples, out_dev)) || n == 0 || (rc = device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(sol_launch_radiance_rescale(rows_dev, n, target_samples, out_dev, s->stream));
  return SOL_OK;
}

int sol_radiance_rescale(SolScene* s, const SolRadiance* rows, size_t n, uint32_t target_samples, SolRadiance* out) {
  int rc;
  if ((rc = rescale_check(s != nullptr, "sol_radiance_rescale", rows, n, target_samples, out)) || n == 0 || (rc = device_check())) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const size_t cap = std::min(n, STAGE_ROWS);
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
