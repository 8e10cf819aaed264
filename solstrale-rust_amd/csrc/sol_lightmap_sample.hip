// sol_lightmap_sample.hip -- lightmap lookups: hits to surface rows, and a baked atlas sampled at surface rows (sol_lightmap_coords,
// sol_lightmap_sample; sol_lightmap_sample.cpp). The rule is sol_lightmap_sample.h; the kernels only fetch, call it and store.
//
//   sol_lightmap_coords_kernel  a thread per hit: two dwordx4 in, (for a triangle hit the table holds) one word of the table, one dwordx4 out.
//   sol_lightmap_sample_kernel  a lane per surface row: the row as one dwordx4, the triangle's six UV words (and, with the chart guard, its nine
//                               vertex words). Then per tap what decides coverage - a byte of pass_of, or the tap's SolTexel - and, with the guard,
//                               the SolTexel and the first dwordx4 of the tap's point row: a tap that is not covered, or that the guard refuses,
//                               fetches no value. The covered taps' value words are then walked once to judge their finiteness (a tap with one
//                               word that is not finite must not contribute to ANY channel, so this cannot wait for the sums), and the live
//                               taps' words once more, channel by channel, for the sums: the second walk reads what the first one brought into
//                               the cache. The channel count is a run-time number (1..32), so nothing is kept in an array: no scratch.
// No LDS, no scratch, no atomics; the taps are added in tap order by the one lane, so the answer does not depend on the schedule. Every store is a
// vector store.
#include <hip/hip_runtime.h>

#include "../../include/solstrale_hip.h"
#include "sol_launch.h"
#include "sol_lightmap_sample.h"

#define LS_WG 256

static_assert(sizeof(SolRayHit) == 32 && sizeof(SolTexel) == 16 && sizeof(SolRay) == 32, "the records of include/solstrale_hip.h");
static_assert(SOL_LS_NONE == SOL_TEXEL_NONE && SOL_LS_ROTATION_SHIFT == SOL_LIGHTMAP_TABLE_ROTATION_SHIFT &&
              SOL_LS_TRIANGLE_MASK == SOL_LIGHTMAP_TABLE_TRIANGLE_MASK, "the table entry of include/solstrale_hip.h");

__global__ __launch_bounds__(LS_WG) void sol_lightmap_coords_kernel(const uint32_t* __restrict__ hits, uint32_t n, const uint32_t* __restrict__ table,
                                                                    uint32_t n_dfs, uint32_t* __restrict__ out) {
  const uint32_t x = blockIdx.x * LS_WG + threadIdx.x;
  if (x >= n) return;
  const SOL_AS1 sol_v4u* h = (const SOL_AS1 sol_v4u*)(hits + (size_t)x * 8);
  const sol_v4u h0 = h[0], h1 = h[1];  // (t, u, v, status), (kind, dfs_index, material, reserved)
  const bool listed = h0.w == SOL_RAY_HIT && h1.x == SOL_REF_TRIANGLE && h1.y < n_dfs;
  const uint32_t entry = listed ? ldg_u32(table + h1.y) : SOL_LS_NONE;
  const LsRow r = ls_coords(listed, entry, __uint_as_float(h0.y), __uint_as_float(h0.z));
  *(SOL_AS1 sol_v4u*)(out + (size_t)x * 4) = sol_v4u{r.triangle, __float_as_uint(r.b1), __float_as_uint(r.b2), r.flags};
}

struct LsAtlas {
  uint32_t W, H, channels, stride_words, n_triangles;
  uint32_t nearest, guard;
  float chart_radius;
};

__global__ __launch_bounds__(LS_WG) void sol_lightmap_sample_kernel(LsAtlas A, const float* __restrict__ uvs, const uint32_t* __restrict__ texels,
                                                                    const uint8_t* __restrict__ pass_of, const float* __restrict__ values,
                                                                    const float* __restrict__ vertices, const float* __restrict__ points,
                                                                    const uint32_t* __restrict__ coords, uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t x = blockIdx.x * LS_WG + threadIdx.x;
  if (x >= n) return;
  const sol_v4u row = *(const SOL_AS1 sol_v4u*)(coords + (size_t)x * 4);
  uint32_t* o = out + (size_t)x * (A.channels + 1u);
  const float b1 = __uint_as_float(row.y), b2 = __uint_as_float(row.z);

  // 1. the row: nothing of it is an address before it is known to be one
  bool valid = row.w != 0u && row.x != SOL_LS_NONE && row.x < A.n_triangles && lf_finite(b1) && lf_finite(b2);
  float uv[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  const float b0 = (1.0f - b1) - b2;
  if (valid) {
    const SOL_AS1 float* t = (const SOL_AS1 float*)(uvs + (size_t)row.x * 6);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      uv[k] = t[k];
      valid = valid && lf_finite(uv[k]);
    }
    if (A.guard) {
      const SOL_AS1 float* p = (const SOL_AS1 float*)(vertices + (size_t)row.x * 9);
      float v[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        v[k] = p[k];
        valid = valid && lf_finite(v[k]);
      }
      px = ls_lerp3(v[0], v[3], v[6], b0, b1, b2);
      py = ls_lerp3(v[1], v[4], v[7], b0, b1, b2);
      pz = ls_lerp3(v[2], v[5], v[8], b0, b1, b2);
    }
  }
  LsTaps T = {0, 0, 0.0f, 0.0f, 0u};
  if (valid) T = ls_taps(ls_lerp3(uv[0], uv[2], uv[4], b0, b1, b2), ls_lerp3(uv[1], uv[3], uv[5], b0, b1, b2), A.W, A.H, A.nearest != 0u);

  // 2. coverage and the chart guard of every tap, before any value is fetched
  const float r2 = A.chart_radius * A.chart_radius;
  uint32_t live = 0u;  // bit k: tap k
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    if (k >= T.n) continue;
    const int i = ls_tap_i(T, k), j = ls_tap_j(T, k);
    if (!ls_tap_inside(i, j, A.W, A.H)) continue;
    const size_t at = (size_t)j * A.W + (size_t)i;
    sol_v4u tx = {0u, 0u, 0u, 0u};
    if (!pass_of || A.guard) tx = *(const SOL_AS1 sol_v4u*)(texels + at * 4);
    if (!ls_covered(pass_of != nullptr, pass_of ? (uint32_t)ldg_u8(pass_of + at) : 0u, tx.x)) continue;
    if (A.guard && tx.w != 0u) {
      const sol_v4f q = *(const SOL_AS1 sol_v4f*)(points + at * 8);
      if (!ls_guard(tx.w, q.x, q.y, q.z, px, py, pz, r2)) continue;
    }
    live |= 1u << k;
  }
  // 3. the value words of the covered taps: one that is not finite takes its tap out
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    if (!(live & (1u << k))) continue;
    const SOL_AS1 float* val = (const SOL_AS1 float*)(values + ((size_t)ls_tap_j(T, k) * A.W + (size_t)ls_tap_i(T, k)) * A.stride_words);
    bool finite = true;
    for (uint32_t c = 0; c < A.channels; ++c) finite = finite && lf_finite(val[c]);
    if (!finite) live &= ~(1u << k);
  }
  // 4. the answer
  if (A.nearest) {
    if (live) {  // the one tap's words, copied
      const SOL_AS1 uint32_t* val = (const SOL_AS1 uint32_t*)(values + ((size_t)T.j0 * A.W + (size_t)T.i0) * A.stride_words);
      for (uint32_t c = 0; c < A.channels; ++c) o[c] = val[c];
    } else {
      for (uint32_t c = 0; c < A.channels; ++c) o[c] = 0u;
    }
    o[A.channels] = live;
    return;
  }
  float w[4], wsum = 0.0f;
  uint32_t count = 0u;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    w[k] = ls_tap_weight(T, k);
    if (live & (1u << k)) {
      wsum = wsum + w[k];
      ++count;
    }
  }
  if (!(wsum > 0.0f)) live = 0u, count = 0u;
  const size_t at0 = ((size_t)T.j0 * A.W + (size_t)T.i0) * A.stride_words;  // (not an address unless tap 0 is live)
  const size_t step_i = A.stride_words, step_j = (size_t)A.W * A.stride_words;
  for (uint32_t c = 0; c < A.channels; ++c) {
    float sum = 0.0f;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k)
      if (live & (1u << k)) sum = sum + (w[k] * ((const SOL_AS1 float*)values)[at0 + (k & 1u) * step_i + (k >> 1) * step_j + c]);
    o[c] = live ? __float_as_uint(sum / wsum) : 0u;
  }
  o[A.channels] = count;
}

// ---- launches (sol_launch.h) ----
hipError_t sol_launch_lightmap_coords(const void* hits, uint32_t n, const void* table, uint32_t n_dfs, void* out, hipStream_t stream) {
  hipLaunchKernelGGL(sol_lightmap_coords_kernel, dim3((uint32_t)(((uint64_t)n + LS_WG - 1) / LS_WG)), dim3(LS_WG), 0, stream, (const uint32_t*)hits, n,
                     (const uint32_t*)table, n_dfs, (uint32_t*)out);
  return hipGetLastError();
}

hipError_t sol_launch_lightmap_sample(const SolLightmapSampleConfig& c, uint32_t n_triangles, const void* uvs, const void* texels, const void* pass_of,
                                      const void* values, const void* vertices, const void* points, const void* coords, uint32_t n, void* out,
                                      hipStream_t stream) {
  const bool guard = vertices && points && (__builtin_isfinite(c.chart_radius) != 0);
  const LsAtlas A{c.width, c.height, c.channels, c.stride_bytes / 4u, n_triangles, (c.flags & SOL_LIGHTMAP_SAMPLE_NEAREST) ? 1u : 0u, guard ? 1u : 0u,
                  guard ? c.chart_radius : 0.0f};
  hipLaunchKernelGGL(sol_lightmap_sample_kernel, dim3((uint32_t)(((uint64_t)n + LS_WG - 1) / LS_WG)), dim3(LS_WG), 0, stream, A, (const float*)uvs,
                     (const uint32_t*)texels, (const uint8_t*)pass_of, (const float*)values, (const float*)vertices, (const float*)points,
                     (const uint32_t*)coords, n, (uint32_t*)out);
  return hipGetLastError();
}
