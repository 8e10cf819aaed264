// sol_lightmap_charts.hip -- lightmap charts: UV islands labelled on the device, a dilation and a lookup that keep charts apart, and the count
// of mip levels before two charts meet (sol_lightmap_charts, sol_lightmap_dilate_charts, sol_lightmap_sample_charts, sol_lightmap_chart_levels;
// sol_lightmap_charts.cpp). The rule is sol_lightmap_charts.h (and sol_lightmap_sample.h / sol_lightmap.h, whose functions are
// called, not restated); the kernels only fetch, call it and store.
//
//   sol_lightmap_charts_hash_kernel     a lane per triangle: liveness, parent[t] = t, and per edge 3t + e the 64-bit hash of its key and its index.
//   (rocprim::radix_sort_pairs)         (hash, edge) sorted by hash.
//   sol_lightmap_charts_match_kernel    a lane per sorted position: walks back within its run of equal hashes to the nearest edge of a live
//                                       triangle whose full key equals its own, unites the two triangles and stops - a fan of a thousand
//                                       triangles on one edge is a chain of a thousand unions, and a collision costs only the walk.
//   sol_lightmap_charts_flatten_kernel  a lane per triangle: its root, and whether it is one.
//   (rocprim::exclusive_scan)           the roots' ranks.
//   sol_lightmap_charts_ids_kernel      a lane per triangle: the rank of its root; the last lane writes the count.
//   sol_lightmap_dilate_charts_begin_kernel / _pass_kernel   a lane per texel, a launch per pass, as the dilation of sol_lightmap.hip.
//   sol_lightmap_sample_charts_kernel   a lane per surface row, as sol_lightmap_sample_kernel, with one more word per tap.
//   sol_lightmap_chart_level_kernel     a lane per destination texel, 64 x 4 per workgroup, a launch per level; the MIXED texels of a wave are
//                                       one ballot, one popcount and one integer atomicAdd.
//   sol_lightmap_chart_windows_kernel   a lane per window of a finished level, counted the same way.
//   sol_lightmap_chart_answer_kernel    one lane: the level count from the two count arrays.
// The only loops that depend on other lanes are lc_unite's retry after a failed exchange; nothing waits for a store of another lane. Integer
// atomics only (sums and minima are order-free); no LDS, no scratch; every store is a vector store.
#include <hip/hip_runtime.h>

#include <cstring>
#include <rocprim/rocprim.hpp>

#include "../../include/solstrale_hip.h"
#include "sol_launch.h"
#include "sol_lightmap_charts.h"

#define LC_WG 256
#define LC_TILE_W 64
#define LC_TILE_H 4

static_assert(sizeof(SolTexel) == 16, "the records of include/solstrale_hip.h");
static_assert(SOL_LC_NONE == SOL_CHART_NONE && SOL_LC_NONE == SOL_TEXEL_NONE, "the words of include/solstrale_hip.h");
static_assert(SOL_LMM_MAX_LEVELS == SOL_LIGHTMAP_MAX_LEVELS, "the level count of include/solstrale_hip.h");

// ---- the labelling ----
__global__ __launch_bounds__(LC_WG) void sol_lightmap_charts_hash_kernel(const float* __restrict__ uvs, const float* __restrict__ vertices, uint32_t n,
                                                                         uint64_t mask, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                                         uint32_t* __restrict__ parent, uint32_t* __restrict__ chart_of) {
  const uint32_t t = blockIdx.x * LC_WG + threadIdx.x;
  if (t >= n) return;
  const float* uv = uvs + (size_t)t * 6;
  const float* pos = vertices ? vertices + (size_t)t * 9 : nullptr;
  const bool live = lc_triangle_live(uv, pos);
  parent[t] = t;
  chart_of[t] = live ? 0u : SOL_LC_NONE;
#pragma unroll
  for (uint32_t e = 0; e < 3u; ++e) {
    keys[(size_t)t * 3 + e] = live ? (lc_key_hash(lc_edge_key(uv, pos, e)) & mask) : mask;
    vals[(size_t)t * 3 + e] = t * 3u + e;
  }
}

__global__ __launch_bounds__(LC_WG) void sol_lightmap_charts_match_kernel(const float* __restrict__ uvs, const float* __restrict__ vertices, uint32_t n_edges,
                                                                          const uint64_t* __restrict__ keys, const uint32_t* __restrict__ order,
                                                                          const uint32_t* __restrict__ chart_of, uint32_t* parent) {
  const uint32_t p = blockIdx.x * LC_WG + threadIdx.x;
  if (p >= n_edges || p == 0u) return;
  const uint32_t edge = order[p], t = edge / 3u;
  if (ldg_u32(chart_of + t) == SOL_LC_NONE) return;
  const uint64_t h = keys[p];
  if (keys[p - 1u] != h) return;
  const LcKey K = lc_edge_key(uvs + (size_t)t * 6, vertices ? vertices + (size_t)t * 9 : nullptr, edge - t * 3u);
  for (uint32_t q = p; q-- > 0u;) {
    if (keys[q] != h) break;
    const uint32_t edge2 = order[q], t2 = edge2 / 3u;
    if (ldg_u32(chart_of + t2) == SOL_LC_NONE) continue;
    const LcKey K2 = lc_edge_key(uvs + (size_t)t2 * 6, vertices ? vertices + (size_t)t2 * 9 : nullptr, edge2 - t2 * 3u);
    if (!lc_key_equal(K, K2)) continue;
    lc_unite(parent, t, t2);
    break;
  }
}

__global__ __launch_bounds__(LC_WG) void sol_lightmap_charts_flatten_kernel(uint32_t n, const uint32_t* parent, const uint32_t* __restrict__ chart_of,
                                                                            uint32_t* __restrict__ root, uint32_t* __restrict__ flag) {
  const uint32_t t = blockIdx.x * LC_WG + threadIdx.x;
  if (t >= n) return;
  const bool live = ldg_u32(chart_of + t) != SOL_LC_NONE;
  const uint32_t r = live ? lc_find(parent, t) : t;
  root[t] = r;
  flag[t] = (live && r == t) ? 1u : 0u;
}

__global__ __launch_bounds__(LC_WG) void sol_lightmap_charts_ids_kernel(uint32_t n, const uint32_t* __restrict__ root, const uint32_t* __restrict__ flag,
                                                                        const uint32_t* __restrict__ rank, uint32_t* chart_of, uint32_t* __restrict__ n_charts) {
  const uint32_t t = blockIdx.x * LC_WG + threadIdx.x;
  if (t >= n) return;
  if (chart_of[t] != SOL_LC_NONE) chart_of[t] = rank[root[t]];
  if (t == n - 1u) *n_charts = rank[t] + flag[t];
}

// ---- the dilation ----
// Pass 0: an owned texel - its triangle is in range and has a chart - is copied whole; every other row is zero.
__global__ __launch_bounds__(LC_WG) void sol_lightmap_dilate_charts_begin_kernel(const uint32_t* __restrict__ texels, uint32_t n_texels,
                                                                                 const uint32_t* __restrict__ values, uint32_t stride_words,
                                                                                 const uint32_t* __restrict__ chart_of, uint32_t n_triangles,
                                                                                 uint32_t* __restrict__ out, uint8_t* __restrict__ cover,
                                                                                 uint32_t* __restrict__ plane) {
  const uint32_t x = blockIdx.x * LC_WG + threadIdx.x;
  if (x >= n_texels) return;
  const uint32_t tri = ldg_u32(texels + (size_t)x * 4);
  const uint32_t chart = tri < n_triangles ? ldg_u32(chart_of + tri) : SOL_LC_NONE;
  const bool owned = chart != SOL_LC_NONE;
  const size_t at = (size_t)x * stride_words;
  for (uint32_t w = 0; w < stride_words; ++w) out[at + w] = owned ? ldg_u32(values + at + w) : 0u;
  cover[x] = owned ? 0u : 255u;
  plane[x] = chart;
}
// Pass k >= 1, as sol_lightmap_dilate_pass_kernel: the texel joins the chart most of its covered neighbours hold and averages those of that
// chart. The plane is read at texels covered before this pass and written at texels that were not: no word is read and written at once.
__global__ __launch_bounds__(LC_WG) void sol_lightmap_dilate_charts_pass_kernel(uint32_t W, uint32_t H, uint32_t channels, uint32_t stride_words, uint32_t pass,
                                                                                float* out, const uint8_t* __restrict__ cover_in,
                                                                                uint8_t* __restrict__ cover_out, uint32_t* plane) {
  const uint32_t x = blockIdx.x * LC_WG + threadIdx.x;
  if (x >= W * H) return;
  const uint8_t mine = ldg_u8(cover_in + x);
  if (mine != 255u) { cover_out[x] = mine; return; }
  const uint32_t j = x / W, i = x - j * W;
  uint32_t covered = 0u, c[8];
#pragma unroll
  for (uint32_t k = 0; k < 8u; ++k) {
    c[k] = SOL_LC_NONE;
    const int ni = (int)i + lm_di(k), nj = (int)j + lm_dj(k);
    if (ni < 0 || nj < 0 || ni >= (int)W || nj >= (int)H) continue;
    const size_t at = (size_t)nj * W + ni;
    if (ldg_u8(cover_in + at) != 255u) {
      covered |= 1u << k;
      c[k] = plane[at];
    }
  }
  cover_out[x] = covered ? (uint8_t)pass : (uint8_t)255u;
  if (!covered) return;
  uint32_t mask;
  plane[x] = lc_vote(c, covered, mask);
  const float fcount = (float)__builtin_popcount(mask);
  for (uint32_t ch = 0; ch < channels; ++ch) {
    float s = 0.0f;
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k)
      if (mask & (1u << k)) s = s + out[((size_t)((int)j + lm_dj(k)) * W + (size_t)((int)i + lm_di(k))) * stride_words + ch];
    out[(size_t)x * stride_words + ch] = s / fcount;
  }
}

// ---- the lookup ----
struct LcAtlas {
  uint32_t W, H, channels, stride_words, n_triangles, nearest;
};

__global__ __launch_bounds__(LC_WG) void sol_lightmap_sample_charts_kernel(LcAtlas A, const float* __restrict__ uvs, const uint32_t* __restrict__ texels,
                                                                           const uint8_t* __restrict__ pass_of, const float* __restrict__ values,
                                                                           const uint32_t* __restrict__ chart_of, const uint32_t* __restrict__ plane,
                                                                           const uint32_t* __restrict__ coords, uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t x = blockIdx.x * LC_WG + threadIdx.x;
  if (x >= n) return;
  const sol_v4u row = *(const SOL_AS1 sol_v4u*)(coords + (size_t)x * 4);
  uint32_t* o = out + (size_t)x * (A.channels + 1u);
  const float b1 = __uint_as_float(row.y), b2 = __uint_as_float(row.z);

  // 1. the row, as sol_lightmap_sample_kernel judges it, and its chart: nothing of it is an address before it is known to be one
  bool valid = row.w != 0u && row.x != SOL_LS_NONE && row.x < A.n_triangles && lf_finite(b1) && lf_finite(b2);
  float uv[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  uint32_t chart = SOL_LC_NONE;
  const float b0 = (1.0f - b1) - b2;
  if (valid) {
    const SOL_AS1 float* t = (const SOL_AS1 float*)(uvs + (size_t)row.x * 6);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      uv[k] = t[k];
      valid = valid && lf_finite(uv[k]);
    }
    chart = ldg_u32(chart_of + row.x);
    valid = valid && chart != SOL_LC_NONE;
  }
  LsTaps T = {0, 0, 0.0f, 0.0f, 0u};
  if (valid) T = ls_taps(ls_lerp3(uv[0], uv[2], uv[4], b0, b1, b2), ls_lerp3(uv[1], uv[3], uv[5], b0, b1, b2), A.W, A.H, A.nearest != 0u);

  // 2. coverage and the chart of every tap, before any value is fetched
  uint32_t live = 0u;  // bit k: tap k
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    if (k >= T.n) continue;
    const int i = ls_tap_i(T, k), j = ls_tap_j(T, k);
    if (!ls_tap_inside(i, j, A.W, A.H)) continue;
    const size_t at = (size_t)j * A.W + (size_t)i;
    if (!ls_covered(pass_of != nullptr, pass_of ? (uint32_t)ldg_u8(pass_of + at) : 0u, pass_of ? 0u : ldg_u32(texels + at * 4))) continue;
    if (ldg_u32(plane + at) != chart) continue;
    live |= 1u << k;
  }
  // 3. the value words of those taps: one that is not finite takes its tap out
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

// ---- the levels ----
// the lanes of a wave that hold `yes`, added to *counter by its first lane (every lane of the wave arrives here)
DEV void lc_count(bool yes, uint32_t* counter) {
  const unsigned long long b = __builtin_amdgcn_ballot_w64(yes);
  if ((threadIdx.x & 63u) == 0u && b != 0ull) atomicAdd(counter, (uint32_t)__builtin_popcountll(b));
}

// LEVEL0: the source is the caller's plane (and pass_of or null); else a level of the scratch
template <bool LEVEL0>
__global__ __launch_bounds__(LC_WG) void sol_lightmap_chart_level_kernel(const uint32_t* __restrict__ src, const uint8_t* __restrict__ pass_of, uint32_t Ws,
                                                                         uint32_t Hs, uint32_t Wd, uint32_t Hd, uint32_t* __restrict__ dst,
                                                                         uint32_t* mixed_texels) {
  const uint32_t i = blockIdx.x * LC_TILE_W + (threadIdx.x % LC_TILE_W), j = blockIdx.y * LC_TILE_H + (threadIdx.x / LC_TILE_W);
  const bool inside = i < Wd && j < Hd;
  uint32_t acc = SOL_LC_NONE;
  if (inside) {
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      const uint32_t ti = 2u * i + (k & 1u), tj = 2u * j + (k >> 1);
      if (ti >= Ws || tj >= Hs) continue;
      const size_t at = (size_t)tj * Ws + ti;
      uint32_t s = ldg_u32(src + at);
      if (LEVEL0 && pass_of && ldg_u8(pass_of + at) == 255u) s = SOL_LC_NONE;
      acc = lc_merge(acc, s);
    }
    dst[(size_t)j * Wd + i] = acc;
  }
  lc_count(inside && acc == SOL_LC_MIXED, mixed_texels);
}

// window (i, j) of a level: the texels (i, j), (i + 1, j), (i, j + 1), (i + 1, j + 1) inside it
__global__ __launch_bounds__(LC_WG) void sol_lightmap_chart_windows_kernel(const uint32_t* __restrict__ level, uint32_t W, uint32_t H, uint32_t Ww, uint32_t Hw,
                                                                           uint32_t* mixed_windows) {
  const uint32_t i = blockIdx.x * LC_TILE_W + (threadIdx.x % LC_TILE_W), j = blockIdx.y * LC_TILE_H + (threadIdx.x / LC_TILE_W);
  const bool inside = i < Ww && j < Hw;
  uint32_t acc = SOL_LC_NONE;
  if (inside) {
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      const uint32_t ti = i + (k & 1u), tj = j + (k >> 1);
      if (ti >= W || tj >= H) continue;
      acc = lc_merge(acc, ldg_u32(level + (size_t)tj * W + ti));
    }
  }
  lc_count(inside && acc == SOL_LC_MIXED, mixed_windows);
}

__global__ void sol_lightmap_chart_answer_kernel(uint32_t full, const uint32_t* mixed_texels, const uint32_t* mixed_windows, uint32_t* levels) {
  if (blockIdx.x != 0u || threadIdx.x != 0u) return;
  uint32_t l = 1u;
  while (l < full && mixed_texels[l] == 0u && mixed_windows[l] == 0u) ++l;
  *levels = l;
}

// ---- launches (sol_launch.h) ----
namespace {
uint32_t lc_blocks(uint64_t n) { return (uint32_t)((n + LC_WG - 1) / LC_WG); }
}  // namespace

hipError_t sol_lightmap_charts_scratch(uint32_t n, LcScratch& S) {
  const size_t E = (size_t)n * 3;
  S.keys = 0; S.keys2 = 2 * E; S.vals = 4 * E; S.order = 5 * E;
  S.parent = 6 * E; S.root = S.parent + n; S.flag = S.root + n; S.rank = S.flag + n;
  S.tmp = (S.rank + n + 63) / 64 * 64;
  S.sort_bytes = S.scan_bytes = 0;
  size_t few_bits = 0;  // (the sort of the masked hash: the larger of the two needs serves both)
  hipError_t e = rocprim::radix_sort_pairs(nullptr, S.sort_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, E, 0, 64,
                                           (hipStream_t)0);
  if (e != hipSuccess) return e;
  e = rocprim::radix_sort_pairs(nullptr, few_bits, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, E, 0, 4, (hipStream_t)0);
  if (e != hipSuccess) return e;
  if (few_bits > S.sort_bytes) S.sort_bytes = few_bits;
  e = rocprim::exclusive_scan(nullptr, S.scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n, rocprim::plus<uint32_t>(), (hipStream_t)0);
  if (e != hipSuccess) return e;
  const size_t tmp_bytes = S.sort_bytes > S.scan_bytes ? S.sort_bytes : S.scan_bytes;
  S.words = S.tmp + (tmp_bytes + 3) / 4 + 64;
  return hipSuccess;
}

hipError_t sol_launch_lightmap_charts(const void* uvs, const void* vertices, uint32_t n, bool collide, const LcScratch& S, uint32_t* scratch, void* chart_of,
                                      void* n_charts, hipStream_t stream) {
  hipError_t e;
  if (n == 0u) return hipMemsetAsync(n_charts, 0, sizeof(uint32_t), stream);
  const uint32_t E = n * 3u;
  uint64_t* keys = (uint64_t*)(scratch + S.keys);
  uint64_t* keys2 = (uint64_t*)(scratch + S.keys2);
  uint32_t *vals = scratch + S.vals, *order = scratch + S.order, *parent = scratch + S.parent;
  void* tmp = scratch + S.tmp;
  hipLaunchKernelGGL(sol_lightmap_charts_hash_kernel, dim3(lc_blocks(n)), dim3(LC_WG), 0, stream, (const float*)uvs, (const float*)vertices, n,
                     collide ? 0xFull : ~0ull, keys, vals, parent, (uint32_t*)chart_of);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  size_t bytes = S.sort_bytes;
  if ((e = rocprim::radix_sort_pairs(tmp, bytes, keys, keys2, vals, order, (size_t)E, 0, collide ? 4 : 64, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(sol_lightmap_charts_match_kernel, dim3(lc_blocks(E)), dim3(LC_WG), 0, stream, (const float*)uvs, (const float*)vertices, E,
                     (const uint64_t*)keys2, (const uint32_t*)order, (const uint32_t*)chart_of, parent);
  return sol_launch_lightmap_chart_ids(n, S, scratch, chart_of, n_charts, stream);
}

hipError_t sol_launch_lightmap_chart_ids(uint32_t n, const LcScratch& S, uint32_t* scratch, void* chart_of, void* n_charts, hipStream_t stream) {
  hipError_t e;
  uint32_t *parent = scratch + S.parent, *root = scratch + S.root, *flag = scratch + S.flag, *rank = scratch + S.rank;
  void* tmp = scratch + S.tmp;
  hipLaunchKernelGGL(sol_lightmap_charts_flatten_kernel, dim3(lc_blocks(n)), dim3(LC_WG), 0, stream, n, (const uint32_t*)parent, (const uint32_t*)chart_of, root,
                     flag);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  size_t bytes = S.scan_bytes;
  if ((e = rocprim::exclusive_scan(tmp, bytes, flag, rank, 0u, (size_t)n, rocprim::plus<uint32_t>(), stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(sol_lightmap_charts_ids_kernel, dim3(lc_blocks(n)), dim3(LC_WG), 0, stream, n, (const uint32_t*)root, (const uint32_t*)flag,
                     (const uint32_t*)rank, (uint32_t*)chart_of, (uint32_t*)n_charts);
  return hipGetLastError();
}

hipError_t sol_launch_lightmap_dilate_charts_begin(const void* texels, uint32_t n_texels, const void* values, uint32_t stride_words, const void* chart_of,
                                                   uint32_t n_triangles, void* out, uint8_t* cover, void* plane, hipStream_t stream) {
  hipLaunchKernelGGL(sol_lightmap_dilate_charts_begin_kernel, dim3(lc_blocks(n_texels)), dim3(LC_WG), 0, stream, (const uint32_t*)texels, n_texels,
                     (const uint32_t*)values, stride_words, (const uint32_t*)chart_of, n_triangles, (uint32_t*)out, cover, (uint32_t*)plane);
  return hipGetLastError();
}
hipError_t sol_launch_lightmap_dilate_charts_pass(uint32_t W, uint32_t H, uint32_t channels, uint32_t stride_words, uint32_t pass, void* out,
                                                  const uint8_t* cover_in, uint8_t* cover_out, void* plane, hipStream_t stream) {
  hipLaunchKernelGGL(sol_lightmap_dilate_charts_pass_kernel, dim3(lc_blocks((uint64_t)W * H)), dim3(LC_WG), 0, stream, W, H, channels, stride_words, pass,
                     (float*)out, cover_in, cover_out, (uint32_t*)plane);
  return hipGetLastError();
}

hipError_t sol_launch_lightmap_sample_charts(const SolLightmapSampleConfig& c, uint32_t n_triangles, const void* uvs, const void* texels, const void* pass_of,
                                             const void* values, const void* chart_of, const void* plane, const void* coords, uint32_t n, void* out,
                                             hipStream_t stream) {
  const LcAtlas A{c.width, c.height, c.channels, c.stride_bytes / 4u, n_triangles, (c.flags & SOL_LIGHTMAP_SAMPLE_NEAREST) ? 1u : 0u};
  hipLaunchKernelGGL(sol_lightmap_sample_charts_kernel, dim3(lc_blocks(n)), dim3(LC_WG), 0, stream, A, (const float*)uvs, (const uint32_t*)texels,
                     (const uint8_t*)pass_of, (const float*)values, (const uint32_t*)chart_of, (const uint32_t*)plane, (const uint32_t*)coords, n,
                     (uint32_t*)out);
  return hipGetLastError();
}

hipError_t sol_launch_lightmap_chart_levels(const LmmLayout& L, const void* plane, const void* pass_of, uint32_t* scratch, void* levels, void* mixed_texels,
                                            void* mixed_windows, hipStream_t stream) {
  hipError_t e;
  uint32_t *mt = (uint32_t*)mixed_texels, *mw = (uint32_t*)mixed_windows;
  if ((e = hipMemsetAsync(mt, 0, SOL_LMM_MAX_LEVELS * sizeof(uint32_t), stream)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(mw, 0, SOL_LMM_MAX_LEVELS * sizeof(uint32_t), stream)) != hipSuccess) return e;
  for (uint32_t l = 1; l < L.full; ++l) {  // level l - 1 -> level l, then level l's windows
    const uint32_t Ws = L.w[l - 1u], Hs = L.h[l - 1u], Wd = L.w[l], Hd = L.h[l];
    uint32_t* dst = scratch + L.at[l];
    const dim3 grid((Wd + LC_TILE_W - 1) / LC_TILE_W, (Hd + LC_TILE_H - 1) / LC_TILE_H);
    if (l == 1u)
      hipLaunchKernelGGL((sol_lightmap_chart_level_kernel<true>), grid, dim3(LC_WG), 0, stream, (const uint32_t*)plane, (const uint8_t*)pass_of, Ws, Hs, Wd, Hd,
                         dst, mt + l);
    else
      hipLaunchKernelGGL((sol_lightmap_chart_level_kernel<false>), grid, dim3(LC_WG), 0, stream, (const uint32_t*)(scratch + L.at[l - 1u]),
                         (const uint8_t*)nullptr, Ws, Hs, Wd, Hd, dst, mt + l);
    const uint32_t Ww = Wd > 1u ? Wd - 1u : 1u, Hw = Hd > 1u ? Hd - 1u : 1u;
    hipLaunchKernelGGL(sol_lightmap_chart_windows_kernel, dim3((Ww + LC_TILE_W - 1) / LC_TILE_W, (Hw + LC_TILE_H - 1) / LC_TILE_H), dim3(LC_WG), 0, stream,
                       (const uint32_t*)dst, Wd, Hd, Ww, Hw, mw + l);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(sol_lightmap_chart_answer_kernel, dim3(1), dim3(64), 0, stream, L.full, (const uint32_t*)mt, (const uint32_t*)mw, (uint32_t*)levels);
  return hipGetLastError();
}
