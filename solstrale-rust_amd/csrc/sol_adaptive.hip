// sol_adaptive.hip -- adaptive sampling (include/solstrale_hip.h, sol_adaptive_*): rounds of samples over the 8x8 blocks
// still active, a per-pixel convergence test on the rounds' luminance, one vote per block, and the order-preserving compaction of
// the work order into the next round's active list. The rounds run the product render kernel unchanged (sol_render_impl with a
// SolRenderJob whose `round` is set); only the chunk resolve is replaced, by the update kernel below, which adds the chunk sums of the ACTIVE blocks
// to the accumulator in the association of sol_resolve_kernel: inactive blocks add nothing, whatever `partial` still holds for them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "sol_scene.h"

struct AdaptiveUpdate {
  float* acc;
  const float* partial;
  float* state;                    // per slot: Welford mean, M2
  uint32_t* active;                // per local block
  uint32_t* counts;                // per image block
  const uint32_t* order;           // the active list of the round
  const uint32_t* block_of_local;  // null: lb * world + rank
  uint32_t n_local, n_traced, n_background, world, rank, blocks_x, width, height;
  uint32_t n_chunks, n_round, rounds, n_after, min_samples, max_samples;
  float threshold;
};

// One wave64 per active block, one lane per pixel. Active block w is entry w of the active list when w < n_traced, else one of the
// last n_background entries. The arithmetic is the stop rule of DESIGN.md 11 written with correctly rounded single operations in a
// fixed order (the test's numpy restatement follows it).
__global__ void __launch_bounds__(256) sol_adaptive_update_kernel(const AdaptiveUpdate U) {
  const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (w >= U.n_traced + U.n_background) return;  // (a whole wave)
  const uint32_t k = w < U.n_traced ? w : U.n_local - U.n_background + (w - U.n_traced);
  const uint32_t lb = U.order[k];
  const uint32_t b = U.block_of_local ? U.block_of_local[lb] : lb * U.world + U.rank;
  const uint32_t by = b / U.blocks_x, bx = b - by * U.blocks_x;
  const bool real = bx * SOL_TILE + (lane & 7u) < U.width && by * SOL_TILE + (lane >> 3) < U.height;
  bool open = false;  // a real pixel that has not converged
  if (real) {
    const size_t slot = (size_t)lb * 64u + lane, plane = (size_t)U.n_local * 64u;
    float* a = U.acc + slot * 3;
    float a0 = a[0], a1 = a[1], a2 = a[2];
    float r0 = 0.f, r1 = 0.f, r2 = 0.f;
    for (uint32_t c = 0; c < U.n_chunks; ++c) {  // ((acc + c0) + c1) + ..: sol_resolve_kernel's association
      const float* q = U.partial + ((size_t)c * plane + slot) * 3;
      const float q0 = q[0], q1 = q[1], q2 = q[2];
      a0 = a0 + q0; a1 = a1 + q1; a2 = a2 + q2;
      r0 = r0 + q0; r1 = r1 + q1; r2 = r2 + q2;
    }
    a[0] = a0; a[1] = a1; a[2] = a2;
    const float n = (float)U.n_round;
    const float y = __fadd_rn(__fadd_rn(__fmul_rn(0.2126f, __fdiv_rn(r0, n)), __fmul_rn(0.7152f, __fdiv_rn(r1, n))),
                              __fmul_rn(0.0722f, __fdiv_rn(r2, n)));
    float* st = U.state + slot * 2;
    const float kf = (float)U.rounds;
    const float d = __fsub_rn(y, st[0]);
    const float mean = __fadd_rn(st[0], __fdiv_rn(d, kf));
    const float m2 = __fadd_rn(st[1], __fmul_rn(d, __fsub_rn(y, mean)));
    st[0] = mean; st[1] = m2;
    bool converged = false;
    if (U.threshold > 0.f && U.rounds >= 2u && U.n_after >= U.min_samples) {
      const float se = __fsqrt_rn(__fdiv_rn(m2, __fmul_rn(kf, __fsub_rn(kf, 1.f))));
      converged = se <= __fmul_rn(U.threshold, fmaxf(mean, 1.f / 256.f));
    }
    open = !converged;
  }
  const bool stop = U.n_after >= U.max_samples || __builtin_amdgcn_ballot_w64(open) == 0ull;
  if (lane == 0) {
    U.active[lb] = stop ? 0u : 1u;
    U.counts[b] = U.n_after;
  }
}

#define SOL_COMPACT_WG 1024u
// Entries [lo, hi) of the work order whose block is active go to out[dst ..] in their order (out == null: only counted); entries
// below heavy_below count into *heavy. Every thread of the (single) workgroup returns the same total.
__device__ uint32_t compact_range(const uint32_t* __restrict__ order, const uint32_t* __restrict__ active, uint32_t lo, uint32_t hi,
                                  uint32_t* __restrict__ out, uint32_t dst, uint32_t heavy_below, uint32_t* heavy, uint32_t* wsum) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  uint32_t running = 0;
  for (uint32_t p0 = lo; p0 < hi; p0 += SOL_COMPACT_WG) {
    const uint32_t p = p0 + tid;
    uint32_t lb = 0;
    bool f = false;
    if (p < hi) {
      lb = order ? order[p] : p;
      f = active[lb] != 0u;
    }
    const unsigned long long m = __builtin_amdgcn_ballot_w64(f);
    if (lane == 0) wsum[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t j = 0; j < SOL_COMPACT_WG / 64u; ++j) {
      const uint32_t c = wsum[j];
      if (j < w) before += c;
      total += c;
    }
    if (f) {
      if (out) out[dst + running + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = lb;
      if (p < heavy_below) atomicAdd(heavy, 1u);
    }
    running += total;
    __syncthreads();  // (wsum is rewritten by the next tile)
  }
  return running;
}

// The next round's active list from the work order (order == null: identity): the active blocks of its traced part [0, n_local -
// n_background) in their order at the front, those of its background tail at the end; ctr = {active heavy blocks (entries below
// n_first), active traced blocks, active background blocks}.
__global__ void __launch_bounds__(SOL_COMPACT_WG) sol_adaptive_compact_kernel(const uint32_t* __restrict__ order, uint32_t n_local, uint32_t n_first,
                                                                              uint32_t n_background, const uint32_t* __restrict__ active,
                                                                              uint32_t* __restrict__ out, uint32_t* __restrict__ ctr) {
  __shared__ uint32_t wsum[SOL_COMPACT_WG / 64u];
  __shared__ uint32_t heavy;
  if (threadIdx.x == 0) heavy = 0;
  __syncthreads();
  const uint32_t n_tr = n_local - n_background;
  const uint32_t traced = compact_range(order, active, 0, n_tr, out, 0, n_first, &heavy, wsum);
  const uint32_t bg = compact_range(order, active, n_tr, n_local, nullptr, 0, 0, &heavy, wsum);
  compact_range(order, active, n_tr, n_local, out, n_local - bg, 0, &heavy, wsum);
  __syncthreads();
  if (threadIdx.x == 0) {
    ctr[0] = heavy; ctr[1] = traced; ctr[2] = bg;
  }
}

// sol_tonemap_kernel (sol_aux.hip) with the sample count of each pixel's block: the same arithmetic, so uniform counts give its bytes.
__global__ void __launch_bounds__(256) sol_tonemap_counts_kernel(const float* __restrict__ image, uint8_t* __restrict__ rgb, uint32_t width,
                                                                 uint32_t height, uint32_t blocks_x, const uint32_t* __restrict__ counts) {
  const uint32_t n = width * height * 3u;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t p = i / 3u, y = p / width, x = p - y * width;
    const double scale = 1.0 / (double)counts[(y / SOL_TILE) * blocks_x + x / SOL_TILE];
    double v = sqrt(scale * (double)image[i]);
    if (v < -0.999) v = -0.999;
    if (v > 0.999) v = 0.999;
    double sc = 256.0 * v;
    rgb[i] = isnan(sc) ? (uint8_t)0 : (uint8_t)(sc < 0.0 ? 0.0 : (sc > 255.0 ? 255.0 : sc));
  }
}

// image <- sum * max / n_b (rounded to fp32): the input of the bloom post-processor, which takes one sample count for the image
__global__ void __launch_bounds__(256) sol_adaptive_rescale_kernel(float* __restrict__ image, uint32_t width, uint32_t height, uint32_t blocks_x,
                                                                   const uint32_t* __restrict__ counts, uint32_t max_samples) {
  const uint32_t n = width * height * 3u;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t p = i / 3u, y = p / width, x = p - y * width;
    const uint32_t nb = counts[(y / SOL_TILE) * blocks_x + x / SOL_TILE];
    if (nb != 0u && nb != max_samples) image[i] = (float)((double)image[i] * (double)max_samples / (double)nb);
  }
}

static int adaptive_compact(SolScene* s) {
  SolAdaptiveSession& A = s->adaptive;
  const uint32_t n_bg = sol_background_tail(s, s->S);  // (filled rather than traced, as in a plain render)
  const uint32_t n_first = s->S.block_order ? std::min(s->S.n_first, s->n_local_blocks - n_bg) : 0u;
  hipLaunchKernelGGL(sol_adaptive_compact_kernel, dim3(1), dim3(SOL_COMPACT_WG), 0, s->stream, s->S.block_order, s->n_local_blocks, n_first, n_bg,
                     A.active.get(), A.order.get(), A.ctr.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(A.ctr_host.get(), A.ctr.get(), 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  A.n_first = A.ctr_host.get()[0]; A.n_traced = A.ctr_host.get()[1]; A.n_background = A.ctr_host.get()[2];
  return SOL_OK;
}

extern "C" {

int sol_adaptive_begin(SolScene* s, const SolAdaptive* c) {
  // (the configuration first: its errors do not need a device)
  if (!c) return sol_fail(SOL_EINVAL, "sol_adaptive_begin: null configuration");
  if (c->size < sizeof(SolAdaptive)) return sol_fail(SOL_EINVAL, "sol_adaptive_begin: SolAdaptive.size %u < %zu", c->size, sizeof(SolAdaptive));
  if (c->round == 0 || c->round % SOL_CHUNK) return sol_fail(SOL_EINVAL, "sol_adaptive_begin: round %u is not a positive multiple of 16", c->round);
  if (c->min_samples % SOL_CHUNK) return sol_fail(SOL_EINVAL, "sol_adaptive_begin: min_samples %u is not a multiple of 16", c->min_samples);
  if (c->max_samples == 0 || c->min_samples > c->max_samples)
    return sol_fail(SOL_EINVAL, "sol_adaptive_begin: need 1 <= max_samples and min_samples <= max_samples (%u, %u)", c->min_samples, c->max_samples);
  if (!(c->threshold >= 0.f)) return sol_fail(SOL_EINVAL, "sol_adaptive_begin: threshold must be >= 0 (not NaN)");
  if (!s) return sol_fail(SOL_EINVAL, "null scene");
  if (s->world > 1) return sol_fail(SOL_EINVAL, "sol_adaptive_begin: adaptive sampling is single-rank (world %d)", s->world);
  HIP_TRY(hipSetDevice(s->device));
  SolAdaptiveSession& A = s->adaptive;
  A.open = false;
  const size_t nl = s->n_local_blocks, nb = (size_t)s->blocks_x * s->blocks_y;
  int rc;
  if ((rc = A.state.reserve(s->stream, nl * 64u * 2u)) || (rc = A.order.reserve(s->stream, nl)) || (rc = A.active.reserve(s->stream, nl)) ||
      (rc = A.counts.reserve(s->stream, nb)) || (rc = A.ctr.reserve(s->stream, 4)))
    return rc;
  if (!A.ctr_host) HIP_TRY(sol_pinned_alloc(A.ctr_host, 4));
  HIP_TRY(hipMemsetAsync(s->acc, 0, s->acc_floats * sizeof(float), s->stream));
  HIP_TRY(hipMemsetAsync(A.state.get(), 0, nl * 64u * 2u * sizeof(float), s->stream));
  HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)A.active.get(), 1, nl, s->stream));
  HIP_TRY(hipMemsetAsync(A.counts.get(), 0, nb * sizeof(uint32_t), s->stream));
  HIP_TRY(hipMemsetAsync(A.ctr.get(), 0, 4 * sizeof(uint32_t), s->stream));
  A.round = c->round; A.min_samples = c->min_samples; A.max_samples = c->max_samples; A.threshold = c->threshold;
  A.rounds_done = 0;
  if ((rc = adaptive_compact(s))) return rc;
  A.open = true;
  return SOL_OK;
}

int sol_adaptive_round(SolScene* s, uint64_t seed, uint32_t* active_blocks) {
  if (!s || !active_blocks) return sol_fail(SOL_EINVAL, "null argument");
  SolAdaptiveSession& A = s->adaptive;
  if (!A.open) return sol_fail(SOL_EINVAL, "sol_adaptive_round: no adaptive session (sol_adaptive_begin; sol_clear, sol_render and sol_scene_set_partition end one)");
  HIP_TRY(hipSetDevice(s->device));
  const uint32_t first = A.rounds_done * A.round;
  if (A.n_traced + A.n_background == 0 || first >= A.max_samples) { *active_blocks = 0; return SOL_OK; }
  const uint32_t n = std::min(A.round, A.max_samples - first);
  // the round's job: the scene with the active list as its work order, through the session's own device copy
  SolRenderJob job = sol_render_job(s, first, n, seed, false);
  job.view.block_order = A.order.get(); job.view.n_first = A.n_first;
  job.mirror = &A.mirror;
  job.round = true; job.n_traced = A.n_traced; job.n_background = A.n_background;
  int rc = sol_render_impl(s, job);
  if (rc) { A.open = false; return rc; }
  AdaptiveUpdate U;
  U.acc = s->acc; U.partial = s->partial.get(); U.state = A.state.get(); U.active = A.active.get(); U.counts = A.counts.get(); U.order = A.order.get();
  U.block_of_local = s->S.block_of_local;
  U.n_local = s->n_local_blocks; U.n_traced = A.n_traced; U.n_background = A.n_background;
  U.world = (uint32_t)s->world; U.rank = (uint32_t)s->rank; U.blocks_x = s->blocks_x; U.width = s->S.width; U.height = s->S.height;
  U.n_chunks = (n + SOL_CHUNK - 1) / SOL_CHUNK; U.n_round = n; U.rounds = A.rounds_done + 1; U.n_after = first + n;
  U.min_samples = A.min_samples; U.max_samples = A.max_samples; U.threshold = A.threshold;
  const uint32_t waves = A.n_traced + A.n_background;
  hipLaunchKernelGGL(sol_adaptive_update_kernel, dim3((waves + 3u) / 4u), dim3(256), 0, s->stream, U);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { A.open = false; return sol_fail(SOL_EDEVICE, "sol_adaptive_update_kernel: %s", hipGetErrorString(e)); }
  A.rounds_done++;
  if ((rc = adaptive_compact(s))) { A.open = false; return rc; }
  *active_blocks = A.n_traced + A.n_background;
  return SOL_OK;
}

int sol_adaptive_counts(SolScene* s, uint32_t* per_block, size_t n) {
  if (!s || !per_block) return sol_fail(SOL_EINVAL, "null argument");
  const size_t nb = (size_t)s->blocks_x * s->blocks_y;
  if (n < nb) return sol_fail(SOL_EINVAL, "sol_adaptive_counts: %zu entries < %zu blocks", n, nb);
  if (s->adaptive.counts.capacity() < nb) return sol_fail(SOL_EINVAL, "sol_adaptive_counts: no adaptive session has begun");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipMemcpyAsync(per_block, s->adaptive.counts.get(), nb * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}

int sol_tonemap_rgb8_adaptive(SolScene* s, const void* image, uint8_t* out) {
  if (!s || !image || !out) return sol_fail(SOL_EINVAL, "bad argument");
  if (s->adaptive.counts.capacity() < (size_t)s->blocks_x * s->blocks_y) return sol_fail(SOL_EINVAL, "sol_tonemap_rgb8_adaptive: no adaptive session has begun");
  HIP_TRY(hipSetDevice(s->device));
  const uint32_t n = s->S.width * s->S.height * 3;
  const uint32_t grid = std::min(4096u, (n + 255u) / 256u);
  hipLaunchKernelGGL(sol_tonemap_counts_kernel, dim3(grid), dim3(256), 0, s->stream, (const float*)image, s->rgb8.get(), s->S.width, s->S.height,
                     s->blocks_x, s->adaptive.counts.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, s->rgb8.get(), n, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}

int sol_adaptive_rescale(SolScene* s, void* image) {
  if (!s || !image) return sol_fail(SOL_EINVAL, "bad argument");
  if (s->adaptive.counts.capacity() < (size_t)s->blocks_x * s->blocks_y) return sol_fail(SOL_EINVAL, "sol_adaptive_rescale: no adaptive session has begun");
  HIP_TRY(hipSetDevice(s->device));
  const uint32_t n = s->S.width * s->S.height * 3;
  const uint32_t grid = std::min(4096u, (n + 255u) / 256u);
  hipLaunchKernelGGL(sol_adaptive_rescale_kernel, dim3(grid), dim3(256), 0, s->stream, (float*)image, s->S.width, s->S.height, s->blocks_x,
                     s->adaptive.counts.get(), s->adaptive.max_samples);
  HIP_TRY(hipGetLastError());
  return SOL_OK;
}

}  // extern "C"
