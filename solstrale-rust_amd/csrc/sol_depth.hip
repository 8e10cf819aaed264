// sol_depth.hip -- directional distance moments for irradiance volumes (sol_visibility_oct, sol_volume_build_depth, sol_volume_sample_depth;
// sol_depth.cpp). The rule is sol_depth.h; the kernels fetch, call it and store.
//
//  sol_depth_each_kernel<SPILL, STRICT> -- sol_visibility_kernel's loop (sol_visibility.hip: the persistent-wave schedule of sol_wave.h, the closest
//    search, query_when_settled) with a work item of one (point, sample), sample-major as in sol_radiance_each_kernel: an aligned run of 64
//    items is 64 consecutive points of one sample. The lane keeps no sum and writes one word per sample to partial[s - first][point]: the hit
//    distance, SOL_DEPTH_MISS for a miss, SOL_DEPTH_NONE where the made ray is invalid. The text is a copy, not a shared header: the eight
//    instances of sol_visibility_kernel keep every instruction.
//  sol_depth_project_kernel<RES> -- after each launch of the kernel above. A wave owns a point's map (four points' at RES 4; at RES 16 a lane
//    owns four texels): per run of 64 samples (16 at RES 4) each lane draws the direction of one sample again exactly as the gather drew it -
//    rng_init(seed, key, s), the counter at first_draw, irradiance_direction -, puts (d, word) into LDS, and then walks the run in sample
//    order reading LDS broadcasts, adding into its texels' four sums in chunks of 16. They continue across windows from what `out` holds.
//  sol_depth_project_plain_kernel -- the measured alternative (SOL_DEPTH_PROJECT=plain): a thread per (point, texel) that draws every direction
//    itself. The same words.
//  sol_depth_build_kernel -- a thread per texel: a SolOctTexel row in, a SolDepthTexel row out.
//  sol_volume_sample_depth_kernel -- sol_volume_sample_kernel's lane per point; per corner with weight, under SOL_VOLUME_CHEBYSHEV, four
//    8-byte texel loads of the probe's map in front of sol_volume.h's corner. (Measured and not kept: the texel addresses computed first and all
//    twelve loads of a corner issued together - 102 VGPRs, 108 against 100 us on two million points: profiles/volume_depth.txt 4.)
// Every sum is one lane's, in sample (or corner) order: the answers do not depend on the schedule. No atomics.
#include <hip/hip_runtime.h>

#include "../../include/solstrale_hip.h"
#include "sol_depth.h"
#include "sol_launch.h"
#include "sol_ray.h"
#include "sol_wave.h"

#define DEPTH_WG 256

static_assert(sizeof(SolOctConfig) == 16 && sizeof(SolOctTexel) == 16 && sizeof(SolDepthTexel) == 8, "the records of include/solstrale_hip.h");

template <bool SPILL, bool STRICT>
__global__ void __launch_bounds__(SOL_WG, SOL_V1_MIN_WAVES)
sol_depth_each_kernel(const DevScene* __restrict__ Sp, const RadianceParams P, const float4* __restrict__ points, const uint2* __restrict__ keys,
                      uint32_t* __restrict__ partial, uint32_t* __restrict__ work_counter, uint32_t* __restrict__ spill) {
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
  bool busy = false, in_flight = false;  // the lane holds an item; its search has been started (running, or over: t.cur == REF_DONE)
  uint32_t index = 0, s = 0;             // the item: sample `s` of point `index` of the launch
  uint32_t left = 0;                     // searches behind a refused hit the sample may still start
  const size_t stride = (size_t)P.n_groups * 64u;

  for (;;) {
    // ---- lanes without a running search: settle the sample that is over and write its word; take the next item; start its search ----
    if (t.cur == REF_DONE) {
      if (in_flight) {
        const float tmax = STRICT ? __uint_as_float(ldg_u32((const float*)(points + (size_t)index * 2u + 1u) + 3)) : 0.f;
        query_when_settled<STRICT>(S, st, t, tmax, left, [&]() __attribute__((always_inline)) {
          const uint32_t word = SOL_REF_KIND(t.h.ref) != SOL_REF_NONE ? __float_as_uint(t.h.t) : SOL_DEPTH_MISS;
          *(SOL_AS1 uint32_t*)(partial + (size_t)(s - P.first_sample) * stride + index) = word;
          in_flight = false;
          busy = false;
        });
      }
      // work fetch: the next item from the wave's reservoir (sol_wave.h) - 64 items, 64 consecutive points of one sample, per refill
      if (!in_flight && !busy) {
        const uint32_t item = wave_take_item(res, work_counter, lane);
        if (item >= P.n_items) break;  // no work left for this lane
        const uint32_t pair = item >> 6, sample = pair / P.n_groups;
        index = (pair - sample * P.n_groups) * 64u + (item & 63u);
        if (index >= P.n_rays) continue;  // padding of the last group
        // validity, before any search (sol_ray.h): the projection kernel judges the row again and reads no word of an invalid one
        if (!query_ray_valid(ldg_f4(points + (size_t)index * 2u), ldg_f4(points + (size_t)index * 2u + 1u))) continue;
        s = P.first_sample + sample;
        busy = true;
      }
      if (!in_flight) {
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
          // (a normal whose squared length is no normal number: the made ray is invalid - searched for nothing, added nowhere)
          *(SOL_AS1 uint32_t*)(partial + (size_t)(s - P.first_sample) * stride + index) = SOL_DEPTH_NONE;
          busy = false;
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
    }
#if SOL_LOOP_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif
  }
}

namespace {
// the key and the counter of point i's stream
DEV void depth_key(const RadianceParams& P, const uint2* __restrict__ keys, uint32_t i, uint32_t& key, uint32_t& ctr) {
  key = P.key_base + i; ctr = P.first_draw;
  if (keys) {
    const unsigned long long kw = *(const SOL_AS1 unsigned long long*)(keys + i);  // one dwordx2: pixel, first_draw
    key = (uint32_t)kw; ctr = (uint32_t)(kw >> 32);
  }
}
// sample `s` of the point's stream: the direction as the gather drew it
DEV f3 depth_direction(const RadianceParams& P, uint32_t key, uint32_t ctr, f3 normal, uint32_t s) {
  Rng rng;
  rng_init(rng, P.seed_lo, P.seed_hi, key, s);
  rng.ctr = ctr;
  return irradiance_direction(P.mode, normal, rng);
}
}  // namespace

// Launched with (n_rays / (4 * PPW)) blocks of four waves; every wave of a block runs the same number of runs (the barriers are uniform).
template <int RES>
__global__ void __launch_bounds__(DEPTH_WG) sol_depth_project_kernel(const RadianceParams P, const float4* __restrict__ points, const uint2* __restrict__ keys,
                                                                     const uint32_t* __restrict__ partial, sol_v4f* __restrict__ out, uint32_t sharpness,
                                                                     uint32_t win_samples, uint32_t accumulate) {
  constexpr uint32_t TEXELS = RES * RES;
  constexpr uint32_t G = TEXELS < 64u ? TEXELS : 64u;  // lanes of one point: the length of a run of samples too
  constexpr uint32_t PPW = 64u / G;                    // points of one wave
  constexpr uint32_t TPL = TEXELS / G;                 // texels of one lane
  __shared__ sol_v4f run[DEPTH_WG];                    // (direction, word) of the run's samples, per wave and point
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, sub = lane / G, gl = lane % G;
  const uint32_t point = (blockIdx.x * (DEPTH_WG / 64u) + wave) * PPW + sub;
  bool active = point < P.n_rays;
  float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
  if (active) {
    b = ldg_f4(points + (size_t)point * 2u + 1u);
    active = query_ray_valid(ldg_f4(points + (size_t)point * 2u), b);
  }
  SOL_AS1 sol_v4f* const rows = (SOL_AS1 sol_v4f*)(out + (size_t)point * TEXELS);
  f3 T[TPL];
  float total[TPL][4], chunk[TPL][4];
#pragma unroll
  for (uint32_t q = 0; q < TPL; ++q) {
    const uint32_t texel = q * G + gl;
    T[q] = oct_texel_direction(texel % RES, texel / RES, RES);
#pragma unroll
    for (int k = 0; k < 4; ++k) total[q][k] = chunk[q][k] = 0.f;
    if (point < P.n_rays && !active) rows[texel] = sol_v4f{0.f, 0.f, 0.f, 0.f};  // an invalid point: zero words
    if (active && accumulate) {
      const sol_v4f o = rows[texel];
      total[q][0] = o.x; total[q][1] = o.y; total[q][2] = o.z; total[q][3] = o.w;
    }
  }
  uint32_t key = 0, ctr = 0;
  if (active) depth_key(P, keys, point, key, ctr);
  const f3 normal = mk3(b.x, b.y, b.z);
  const size_t stride = (size_t)P.n_groups * 64u;
  for (uint32_t j0 = 0; j0 < win_samples; j0 += G) {
    const uint32_t j = j0 + gl;
    sol_v4f e = {0.f, 0.f, 0.f, __uint_as_float(SOL_DEPTH_NONE)};
    if (active && j < win_samples) {
      const f3 d = depth_direction(P, key, ctr, normal, P.first_sample + j);
      e = sol_v4f{d.x, d.y, d.z, __uint_as_float(*(const SOL_AS1 uint32_t*)(partial + (size_t)j * stride + point))};
    }
    run[threadIdx.x] = e;
    __syncthreads();
    const uint32_t count = win_samples - j0 < G ? win_samples - j0 : G;
    if (active) {
      for (uint32_t k = 0; k < count; ++k) {
        const sol_v4f r = run[wave * 64u + sub * G + k];  // one address per point: a broadcast
        const bool close = (k & (uint32_t)(SOL_CHUNK - 1)) == (uint32_t)(SOL_CHUNK - 1) || k + 1u == count;  // (a run starts on a chunk's first sample)
#pragma unroll
        for (uint32_t q = 0; q < TPL; ++q) {
          oct_add_sample(chunk[q], oct_lobe(T[q], mk3(r.x, r.y, r.z), sharpness), __float_as_uint(r.w));
          if (close) {
#pragma unroll
            for (int c = 0; c < 4; ++c) { total[q][c] = total[q][c] + chunk[q][c]; chunk[q][c] = 0.f; }
          }
        }
      }
    }
    __syncthreads();
  }
  if (active) {
#pragma unroll
    for (uint32_t q = 0; q < TPL; ++q) rows[q * G + gl] = sol_v4f{total[q][0], total[q][1], total[q][2], total[q][3]};
  }
}

// The plain alternative: a thread per (point, texel), every direction drawn by every thread.
__global__ void __launch_bounds__(DEPTH_WG) sol_depth_project_plain_kernel(const RadianceParams P, const float4* __restrict__ points, const uint2* __restrict__ keys,
                                                                           const uint32_t* __restrict__ partial, sol_v4f* __restrict__ out, uint32_t res,
                                                                           uint32_t sharpness, uint32_t win_samples, uint32_t accumulate) {
  const uint32_t texels = res * res;
  const uint64_t x = (uint64_t)blockIdx.x * DEPTH_WG + threadIdx.x;
  const uint32_t point = (uint32_t)(x / texels), texel = (uint32_t)(x - (uint64_t)point * texels);
  if (point >= P.n_rays) return;
  SOL_AS1 sol_v4f* const row = (SOL_AS1 sol_v4f*)(out + (size_t)point * texels + texel);
  const float4 b = ldg_f4(points + (size_t)point * 2u + 1u);
  if (!query_ray_valid(ldg_f4(points + (size_t)point * 2u), b)) {
    *row = sol_v4f{0.f, 0.f, 0.f, 0.f};
    return;
  }
  const f3 T = oct_texel_direction(texel % res, texel / res, res);
  float total[4] = {0.f, 0.f, 0.f, 0.f}, chunk[4] = {0.f, 0.f, 0.f, 0.f};
  if (accumulate) {
    const sol_v4f o = *row;
    total[0] = o.x; total[1] = o.y; total[2] = o.z; total[3] = o.w;
  }
  uint32_t key, ctr;
  depth_key(P, keys, point, key, ctr);
  const f3 normal = mk3(b.x, b.y, b.z);
  const size_t stride = (size_t)P.n_groups * 64u;
  for (uint32_t j = 0; j < win_samples; ++j) {
    const f3 d = depth_direction(P, key, ctr, normal, P.first_sample + j);
    oct_add_sample(chunk, oct_lobe(T, d, sharpness), *(const SOL_AS1 uint32_t*)(partial + (size_t)j * stride + point));
    if ((j & (uint32_t)(SOL_CHUNK - 1)) == (uint32_t)(SOL_CHUNK - 1) || j + 1u == win_samples) {
#pragma unroll
      for (int c = 0; c < 4; ++c) { total[c] = total[c] + chunk[c]; chunk[c] = 0.f; }
    }
  }
  *row = sol_v4f{total[0], total[1], total[2], total[3]};
}

__global__ void __launch_bounds__(DEPTH_WG) sol_depth_build_kernel(uint64_t n_texels, const sol_v4f* __restrict__ oct, float radius, float* __restrict__ depth) {
  const uint64_t x = (uint64_t)blockIdx.x * DEPTH_WG + threadIdx.x;
  if (x >= n_texels) return;
  const sol_v4f o = *(const SOL_AS1 sol_v4f*)(oct + x);
  const float sum[4] = {o.x, o.y, o.z, o.w};
  float mean, mean2;
  oct_build(sum, radius, mean, mean2);
  typedef float v2f __attribute__((ext_vector_type(2)));
  *(SOL_AS1 v2f*)(depth + x * 2u) = v2f{mean, mean2};  // one dwordx2
}

namespace {
// (sol_volume.hip's: a probe's eight dwordx4, issued together in front of the valid test)
DEV void depth_load_probe(const uint32_t* probes, uint32_t row, uint32_t (&e)[32]) {
  const SOL_AS1 sol_v4u* p = (const SOL_AS1 sol_v4u*)(probes + (size_t)row * 32);
  sol_v4u v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = p[k];
  asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]));
#pragma unroll
  for (int k = 0; k < 8; ++k) { e[4 * k] = v[k].x; e[4 * k + 1] = v[k].y; e[4 * k + 2] = v[k].z; e[4 * k + 3] = v[k].w; }
}
}  // namespace

__global__ __launch_bounds__(DEPTH_WG) void sol_volume_sample_depth_kernel(VolGrid G, const uint32_t* __restrict__ probes, const float* __restrict__ depth, uint32_t res,
                                                                           const float* __restrict__ points, uint32_t n, uint32_t* __restrict__ out) {
  typedef float v2f __attribute__((ext_vector_type(2)));
  const uint32_t x = blockIdx.x * DEPTH_WG + threadIdx.x;
  if (x >= n) return;
  const SOL_AS1 sol_v4f* row = (const SOL_AS1 sol_v4f*)(points + (size_t)x * 8);
  const sol_v4f r0 = row[0], r1 = row[1];
  sol_v4u answer = {0u, 0u, 0u, 0u};
  VolPoint P;
  if (vol_setup(G, r0, r1, P)) {
    float sum[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f;
    uint32_t samples = 0u;
#pragma unroll
    for (uint32_t c = 0; c < 8u; ++c) {
      const float w = vol_trilinear(P, c);
      if (w == 0.0f) continue;
      const uint32_t i = min(P.i0[0] + (c & 1u), G.n[0] - 1u), j = min(P.i0[1] + ((c >> 1) & 1u), G.n[1] - 1u), k = min(P.i0[2] + (c >> 2), G.n[2] - 1u);
      const uint32_t probe = (k * G.n[1] + j) * G.n[0] + i;
      uint32_t e[32];
      depth_load_probe(probes, probe, e);
      const f3 at = vol_probe_position(G, i, j, k);
      // the probe's moments for this point's direction, in the place of words 27 and 28: sol_volume.h's Chebyshev lines then run as they are
      e[29] &= ~SOL_VOL_MOMENTS;
      if ((G.flags & SOL_VOL_CHEBYSHEV) && (e[29] & SOL_VOL_VALID)) {
        const f3 D = P.q - at;
        if (sqrtf(len2(D)) > 0.0f) {
          uint32_t rows[4];
          float wts[4], m[4], m2[4];
          oct_lookup(D, res, rows, wts);
          const SOL_AS1 v2f* map = (const SOL_AS1 v2f*)(depth + (size_t)probe * (res * res) * 2u);
#pragma unroll
          for (int q = 0; q < 4; ++q) { const v2f t = map[rows[q]]; m[q] = t.x; m2[q] = t.y; }  // four dwordx2
          e[27] = __float_as_uint(oct_bilinear(m, wts));
          e[28] = __float_as_uint(oct_bilinear(m2, wts));
          e[29] |= SOL_VOL_MOMENTS;
        }
      }
      vol_corner(G, P, w, at, e, sum, wsum, samples);
    }
    if (samples != 0u) answer = sol_v4u{__float_as_uint(sum[0] / wsum), __float_as_uint(sum[1] / wsum), __float_as_uint(sum[2] / wsum), samples};
  }
  *(SOL_AS1 sol_v4u*)(out + (size_t)x * 4) = answer;
}

// ---- launches (sol_launch.h) ----
using DepthEachKernel = void (*)(const DevScene*, const RadianceParams, const float4*, const uint2*, uint32_t*, uint32_t*, uint32_t*);
static DepthEachKernel depth_each_variant(bool spill, bool strict) {
  if (spill) return strict ? sol_depth_each_kernel<true, true> : sol_depth_each_kernel<true, false>;
  return strict ? sol_depth_each_kernel<false, true> : sol_depth_each_kernel<false, false>;
}

hipError_t sol_launch_depth_each(const DevScene* dS, const RadianceParams& P, bool may_spill, bool strict, const void* points, const void* keys, void* partial,
                                 uint32_t* work, uint32_t* spill, uint32_t grid, hipStream_t stream) {
  hipLaunchKernelGGL(depth_each_variant(may_spill, strict), dim3(grid), dim3(SOL_WG), 0, stream, dS, P, (const float4*)points, (const uint2*)keys, (uint32_t*)partial,
                     work, spill);
  return hipGetLastError();
}
int sol_depth_each_blocks_per_cu(bool strict) { return sol_blocks_per_cu(depth_each_variant(true, strict)); }

hipError_t sol_launch_depth_project(const RadianceParams& P, bool plain, uint32_t res, uint32_t sharpness, const void* points, const void* keys, const void* partial,
                                    void* out, uint32_t win_samples, bool accumulate, hipStream_t stream) {
  const uint32_t acc = accumulate ? 1u : 0u;
  if (plain) {
    const uint64_t threads = (uint64_t)P.n_rays * res * res;
    hipLaunchKernelGGL(sol_depth_project_plain_kernel, dim3((uint32_t)((threads + DEPTH_WG - 1) / DEPTH_WG)), dim3(DEPTH_WG), 0, stream, P, (const float4*)points,
                       (const uint2*)keys, (const uint32_t*)partial, (sol_v4f*)out, res, sharpness, win_samples, acc);
    return hipGetLastError();
  }
  const uint32_t per_block = (DEPTH_WG / 64u) * (res == 4u ? 4u : 1u);  // points of one block
  const dim3 blocks((P.n_rays + per_block - 1u) / per_block);
  if (res == 4u)
    hipLaunchKernelGGL(sol_depth_project_kernel<4>, blocks, dim3(DEPTH_WG), 0, stream, P, (const float4*)points, (const uint2*)keys, (const uint32_t*)partial,
                       (sol_v4f*)out, sharpness, win_samples, acc);
  else if (res == 8u)
    hipLaunchKernelGGL(sol_depth_project_kernel<8>, blocks, dim3(DEPTH_WG), 0, stream, P, (const float4*)points, (const uint2*)keys, (const uint32_t*)partial,
                       (sol_v4f*)out, sharpness, win_samples, acc);
  else
    hipLaunchKernelGGL(sol_depth_project_kernel<16>, blocks, dim3(DEPTH_WG), 0, stream, P, (const float4*)points, (const uint2*)keys, (const uint32_t*)partial,
                       (sol_v4f*)out, sharpness, win_samples, acc);
  return hipGetLastError();
}

hipError_t sol_launch_depth_build(uint64_t n_texels, const void* oct, float radius, void* depth, hipStream_t stream) {
  hipLaunchKernelGGL(sol_depth_build_kernel, dim3((uint32_t)((n_texels + DEPTH_WG - 1) / DEPTH_WG)), dim3(DEPTH_WG), 0, stream, n_texels, (const sol_v4f*)oct, radius,
                     (float*)depth);
  return hipGetLastError();
}

hipError_t sol_launch_volume_sample_depth(const SolVolumeGrid& g, const void* probes, const void* depth, uint32_t res, const void* points, uint32_t n, void* out,
                                          hipStream_t stream) {
  const VolGrid G{{g.nx, g.ny, g.nz}, {g.origin[0], g.origin[1], g.origin[2]}, {g.spacing[0], g.spacing[1], g.spacing[2]}, g.flags, g.normal_bias};
  hipLaunchKernelGGL(sol_volume_sample_depth_kernel, dim3((uint32_t)(((uint64_t)n + DEPTH_WG - 1) / DEPTH_WG)), dim3(DEPTH_WG), 0, stream, G, (const uint32_t*)probes,
                     (const float*)depth, res, (const float*)points, n, (uint32_t*)out);
  return hipGetLastError();
}
