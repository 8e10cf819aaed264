// sol_gather_adaptive.hip -- the device side of the adaptive irradiance gathers (sol_irradiance_adaptive; sol_gather_adaptive.cpp):
// what judges the rows of a round and compacts the ones that go on, and the rescale of rows of different counts (sol_radiance_rescale). The paths
// themselves are sol_radiance_each_kernel's and the sums sol_moments_project_kernel's, as they stand.
//
//   sol_gather_judge_kernel      a thread per active row, 256 per workgroup: the rule of sol_gather_adaptive.h on the row's count and six sums. A
//                                wave's verdicts are one 64-bit ballot, written as it is; the workgroup's count of rows that go on is the sum of
//                                its four popcounts. What stopped, and why, is counted per wave into three integer counters.
//   sol_gather_scan_kernel       ONE workgroup of 1024 threads: the exclusive prefix sum of the workgroup counts, a contiguous run of them per
//                                thread, and the total - the next round's active count, which the host reads back.
//   sol_gather_scatter_kernel    a thread per active row: a row that goes on finds its place - the workgroup's offset, the popcounts of the waves
//                                in front of it, the set bits below its own in its wave's ballot -, writes its index there and gathers its point,
//                                its key (the caller's, or (key_base + index, first_draw)) and its totals so far into the compact buffers.
//   sol_gather_writeback_kernel  a thread per active row of a later round: compact row j back to out[index[j]].
//   sol_rescale_rows_kernel      a thread per SolRadiance row (sol_radiance_rescale).
// The compaction is stable - a row's place is the number of surviving rows in front of it - and so a function of the sums alone. No workgroup
// waits for another: the three steps are three launches. Integer atomics only (their sums do not depend on the order); every store is a vector store.
#include <hip/hip_runtime.h>

#include "../../include/solstrale_hip.h"
#include "sol_gather_adaptive.h"
#include "sol_launch.h"

#define GA_WG 256
#define GA_WAVES (GA_WG / 64)
#define GA_SCAN_WG 1024

typedef uint32_t sol_v2u __attribute__((ext_vector_type(2)));  // one dwordx2

namespace {
DEV unsigned long long ga_ballot_of(const uint32_t* ballots, uint32_t wave) {
  const unsigned long long lo = ldg_u32(ballots + 2u * (size_t)wave), hi = ldg_u32(ballots + 2u * (size_t)wave + 1u);
  return lo | (hi << 32);
}
}  // namespace

// rows: the n_active SolMoments rows the round left (round 0: the caller's `out`; later: the compact totals), row j of them the row of thread j.
// ballots: two words per wave of the grid; wg_counts: one per workgroup; ctr: [1] rows without samples (invalid), [2] converged, [3] capped - added to.
__global__ void __launch_bounds__(GA_WG) sol_gather_judge_kernel(const float4* __restrict__ rows, uint32_t n_active, uint32_t max_samples, uint32_t min_samples,
                                                                 float threshold, float floor, uint32_t* __restrict__ ballots,
                                                                 uint32_t* __restrict__ wg_counts, uint32_t* __restrict__ ctr) {
  __shared__ uint32_t wave_count[GA_WAVES];
  const uint32_t j = blockIdx.x * GA_WG + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t verdict = SOL_GA_BROKEN;
  bool invalid = false;
  if (j < n_active) {
    const float4 m0 = ldg_f4(rows + 2u * (size_t)j), m1 = ldg_f4(rows + 2u * (size_t)j + 1u);
    const uint32_t count = __float_as_uint(m0.w);
    invalid = count == 0u;  // (an invalid point: eight zero words, never traced)
    if (!invalid) verdict = ga_judge(count, max_samples, min_samples, threshold, floor, m0.x, m0.y, m0.z, m1.x, m1.y, m1.z);
  }
  const unsigned long long on = __builtin_amdgcn_ballot_w64(j < n_active && !invalid && verdict == SOL_GA_ACTIVE);
  const unsigned long long n_invalid = __builtin_amdgcn_ballot_w64(invalid);
  const unsigned long long converged = __builtin_amdgcn_ballot_w64(j < n_active && !invalid && verdict == SOL_GA_CONVERGED);
  const unsigned long long capped = __builtin_amdgcn_ballot_w64(j < n_active && !invalid && verdict == SOL_GA_CAPPED);
  if (lane == 0u) {
    const uint32_t w = blockIdx.x * GA_WAVES + wave;
    *(SOL_AS1 sol_v2u*)(ballots + 2u * (size_t)w) = sol_v2u{(uint32_t)on, (uint32_t)(on >> 32)};
    wave_count[wave] = (uint32_t)__popcll(on);
    if (n_invalid) atomicAdd(ctr + 1, (uint32_t)__popcll(n_invalid));
    if (converged) atomicAdd(ctr + 2, (uint32_t)__popcll(converged));
    if (capped) atomicAdd(ctr + 3, (uint32_t)__popcll(capped));
  }
  __syncthreads();
  if (threadIdx.x == 0u) {
    uint32_t total = 0u;
#pragma unroll
    for (int w = 0; w < GA_WAVES; ++w) total += wave_count[w];
    wg_counts[blockIdx.x] = total;
  }
}

// wg_offsets[b] = wg_counts[0] + .. + wg_counts[b - 1]; ctr[0] = their sum. One workgroup: thread t adds the run [t * per, (t + 1) * per), the 1024
// run sums are scanned in LDS, and the thread writes its run's offsets.
__global__ void __launch_bounds__(GA_SCAN_WG) sol_gather_scan_kernel(const uint32_t* __restrict__ wg_counts, uint32_t n_wg, uint32_t* __restrict__ wg_offsets,
                                                                     uint32_t* __restrict__ ctr) {
  __shared__ uint32_t run[GA_SCAN_WG];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (n_wg + GA_SCAN_WG - 1u) / GA_SCAN_WG;
  const uint32_t b0 = t * per < n_wg ? t * per : n_wg, b1 = b0 + per < n_wg ? b0 + per : n_wg;
  uint32_t sum = 0u;
  for (uint32_t b = b0; b < b1; ++b) sum += ldg_u32(wg_counts + b);
  run[t] = sum;
  __syncthreads();
  for (uint32_t d = 1u; d < GA_SCAN_WG; d <<= 1) {  // (an inclusive scan of the run sums, every thread at every barrier)
    const uint32_t add = t >= d ? run[t - d] : 0u;
    __syncthreads();
    run[t] += add;
    __syncthreads();
  }
  uint32_t at = run[t] - sum;
  for (uint32_t b = b0; b < b1; ++b) {
    wg_offsets[b] = at;
    at += ldg_u32(wg_counts + b);
  }
  if (t == GA_SCAN_WG - 1u) ctr[0] = run[t];
}

// index_in: the active list the judged round ran over, or null - row j is row j of the call (round 0). totals: where a row's sums so far stand,
// by its index in the call (`out`, after the write-back). The compact buffers are written, never read: no row is moved within one.
__global__ void __launch_bounds__(GA_WG) sol_gather_scatter_kernel(uint32_t n_active, const uint32_t* __restrict__ index_in, const uint32_t* __restrict__ ballots,
                                                                   const uint32_t* __restrict__ wg_offsets, const float4* __restrict__ points,
                                                                   const uint32_t* __restrict__ keys, uint32_t key_base, uint32_t first_draw,
                                                                   const float4* __restrict__ totals, uint32_t n_next, uint32_t* __restrict__ index_out,
                                                                   float4* __restrict__ points_out, uint32_t* __restrict__ keys_out,
                                                                   float4* __restrict__ totals_out) {
  const uint32_t j = blockIdx.x * GA_WG + threadIdx.x;
  if (j >= n_active) return;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t w0 = blockIdx.x * GA_WAVES;
  const unsigned long long mine = ga_ballot_of(ballots, w0 + wave);
  if (!((mine >> lane) & 1ull)) return;
  uint32_t dst = ldg_u32(wg_offsets + blockIdx.x) + (uint32_t)__popcll(mine & ((1ull << lane) - 1ull));
  for (uint32_t w = 0; w < wave; ++w) dst += (uint32_t)__popcll(ga_ballot_of(ballots, w0 + w));
  if (dst >= n_next) return;  // (cannot happen: n_next is the scan's total; the compact buffers hold n_next rows)
  const uint32_t i = index_in ? ldg_u32(index_in + j) : j;
  index_out[dst] = i;
  SOL_AS1 sol_v4f* const p = (SOL_AS1 sol_v4f*)(points_out + 2u * (size_t)dst);
  const float4 a = ldg_f4(points + 2u * (size_t)i), b = ldg_f4(points + 2u * (size_t)i + 1u);
  p[0] = sol_v4f{a.x, a.y, a.z, a.w};
  p[1] = sol_v4f{b.x, b.y, b.z, b.w};
  sol_v2u key = {key_base + i, first_draw};
  if (keys) key = sol_v2u{ldg_u32(keys + 2u * (size_t)i), ldg_u32(keys + 2u * (size_t)i + 1u)};
  *(SOL_AS1 sol_v2u*)(keys_out + 2u * (size_t)dst) = key;
  SOL_AS1 sol_v4f* const m = (SOL_AS1 sol_v4f*)(totals_out + 2u * (size_t)dst);
  const float4 m0 = ldg_f4(totals + 2u * (size_t)i), m1 = ldg_f4(totals + 2u * (size_t)i + 1u);
  m[0] = sol_v4f{m0.x, m0.y, m0.z, m0.w};
  m[1] = sol_v4f{m1.x, m1.y, m1.z, m1.w};
}

__global__ void __launch_bounds__(GA_WG) sol_gather_writeback_kernel(uint32_t n_active, const uint32_t* __restrict__ index, const float4* __restrict__ rows,
                                                                     float4* __restrict__ out) {
  const uint32_t j = blockIdx.x * GA_WG + threadIdx.x;
  if (j >= n_active) return;
  const uint32_t i = ldg_u32(index + j);
  const float4 m0 = ldg_f4(rows + 2u * (size_t)j), m1 = ldg_f4(rows + 2u * (size_t)j + 1u);
  SOL_AS1 sol_v4f* const o = (SOL_AS1 sol_v4f*)(out + 2u * (size_t)i);
  o[0] = sol_v4f{m0.x, m0.y, m0.z, m0.w};
  o[1] = sol_v4f{m1.x, m1.y, m1.z, m1.w};
}

// word j <- (float)(((double)word_j * (double)target) / (double)count), count <- target; a row without samples is copied. out may be rows: a thread
// reads its row before it writes it and touches no other.
__global__ void __launch_bounds__(GA_WG) sol_rescale_rows_kernel(const float4* rows, size_t n, uint32_t target, float4* out) {
  const size_t x = (size_t)blockIdx.x * GA_WG + threadIdx.x;
  if (x >= n) return;
  const sol_v4f r = *(const SOL_AS1 sol_v4f*)(rows + x);
  const uint32_t count = __float_as_uint(r.w);
  sol_v4f o = r;
  if (count != 0u) {
    const double t = (double)target, c = (double)count;
    o = sol_v4f{(float)(((double)r.x * t) / c), (float)(((double)r.y * t) / c), (float)(((double)r.z * t) / c), __uint_as_float(target)};
  }
  *(SOL_AS1 sol_v4f*)(out + x) = o;
}

// ---- launches (sol_launch.h) ----
hipError_t sol_launch_gather_judge(const void* rows, uint32_t n_active, uint32_t max_samples, uint32_t min_samples, float threshold, float floor, uint32_t* ballots,
                                   uint32_t* wg_counts, uint32_t* wg_offsets, uint32_t* ctr, hipStream_t stream) {
  const uint32_t n_wg = (n_active + GA_WG - 1u) / GA_WG;
  hipLaunchKernelGGL(sol_gather_judge_kernel, dim3(n_wg), dim3(GA_WG), 0, stream, (const float4*)rows, n_active, max_samples, min_samples, threshold, floor, ballots,
                     wg_counts, ctr);
  hipLaunchKernelGGL(sol_gather_scan_kernel, dim3(1), dim3(GA_SCAN_WG), 0, stream, wg_counts, n_wg, wg_offsets, ctr);
  return hipGetLastError();
}

hipError_t sol_launch_gather_scatter(uint32_t n_active, const uint32_t* index_in, const uint32_t* ballots, const uint32_t* wg_offsets, const void* points,
                                     const void* keys, uint32_t key_base, uint32_t first_draw, const void* totals, uint32_t n_next, uint32_t* index_out,
                                     void* points_out, void* keys_out, void* totals_out, hipStream_t stream) {
  hipLaunchKernelGGL(sol_gather_scatter_kernel, dim3((n_active + GA_WG - 1u) / GA_WG), dim3(GA_WG), 0, stream, n_active, index_in, ballots, wg_offsets,
                     (const float4*)points, (const uint32_t*)keys, key_base, first_draw, (const float4*)totals, n_next, index_out, (float4*)points_out,
                     (uint32_t*)keys_out, (float4*)totals_out);
  return hipGetLastError();
}

hipError_t sol_launch_gather_writeback(uint32_t n_active, const uint32_t* index, const void* rows, void* out, hipStream_t stream) {
  hipLaunchKernelGGL(sol_gather_writeback_kernel, dim3((n_active + GA_WG - 1u) / GA_WG), dim3(GA_WG), 0, stream, n_active, index, (const float4*)rows, (float4*)out);
  return hipGetLastError();
}

hipError_t sol_launch_radiance_rescale(const void* rows, size_t n, uint32_t target, void* out, hipStream_t stream) {
  hipLaunchKernelGGL(sol_rescale_rows_kernel, dim3((uint32_t)((n + GA_WG - 1u) / GA_WG)), dim3(GA_WG), 0, stream, (const float4*)rows, n, target, (float4*)out);
  return hipGetLastError();
}
