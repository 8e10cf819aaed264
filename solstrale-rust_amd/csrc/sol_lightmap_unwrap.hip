// sol_lightmap_unwrap.hip -- the lightmap unwrap: box-projected charts packed into an atlas by the greedy shelf rule (sol_lightmap_unwrap;
// sol_lightmap_unwrap.cpp). The rule is sol_lightmap_unwrap.h (and sol_lightmap_charts.h, whose key, hash and union-find are
// called, not restated); the kernels only fetch, call it and store.
//
//   sol_lightmap_unwrap_normals_kernel  a lane per triangle: liveness, class and unit normal, parent[t] = t, and per edge 3t + e the 64-bit hash
//                                       of its position key and its index; the live triangles of a wave are one ballot and one atomicAdd.
//   (rocprim::radix_sort_pairs)         (hash, edge) sorted by hash.
//   sol_lightmap_unwrap_match_kernel    a lane per sorted position: walks back over its whole run of equal hashes and unites its triangle with
//                                       every live one whose class and normal pass the join and whose full key equals its own. (The charts'
//                                       matcher stops at the nearest equal key, which is right for an equivalence; the join is none.)
//   (sol_launch_lightmap_chart_ids)     the charts' flatten, flag, scan and ids: dense labels in mesh order and the count.
//   sol_lightmap_unwrap_extents_kernel  a lane per triangle: its projected corners' minimum and maximum per axis as ordered integers, reduced
//                                       over neighbouring lanes of the same chart by shuffles, then one atomicMin / atomicMax per run and word.
//   sol_lightmap_unwrap_rects_kernel    a lane per chart: content, rectangle, sort key; content sum and width overflow reduced per wave.
//   (rocprim::radix_sort_pairs)         (key, chart) sorted: height descending, width descending, id ascending.
//   (rocprim::inclusive_scan)           the 64-bit prefix sums of the sorted widths.
//   sol_lightmap_unwrap_next_kernel     a lane per rectangle i: next[i], the first rectangle that no longer fits a shelf opened at i (bisection).
//   sol_lightmap_unwrap_walk_kernel     one lane: the orbit of 0 under next - a shelf per step, at most 5463 steps -, the shelves' tables and
//                                       the result.
//   sol_lightmap_unwrap_place_kernel    a lane per rectangle: its shelf by bisection of the shelves' first indices, its x from the prefix sums.
//   sol_lightmap_unwrap_write_kernel    a lane per triangle: the six UV words, or zeros and SOL_LC_NONE on overflow.
// The only loops that depend on other lanes are lc_unite's retry after a failed exchange; nothing waits for a store of another lane. Integer
// atomics only (minima, maxima, sums and ors are order-free); no LDS, no scratch; every store is a vector store.
#include <hip/hip_runtime.h>

#include <cstring>
#include <rocprim/rocprim.hpp>

#include "../../include/solstrale_hip.h"
#include "sol_launch.h"
#include "sol_lightmap_unwrap.h"

#define LU_WG 256

static_assert(SOL_LC_NONE == SOL_CHART_NONE, "the words of include/solstrale_hip.h");
static_assert(sizeof(SolUnwrapResult) == 32 && sizeof(SolUnwrapConfig) == 32, "the records of include/solstrale_hip.h");
static_assert(SOL_LIGHTMAP_CHARTS_MAX_TRIANGLES <= (1u << 30), "a chart id has 30 bits of the sort key");
static_assert(SOL_LU_MAX_CONTENT + SOL_UNWRAP_MAX_GUTTER < 0xFFFFu, "a rectangle's extent has 16 bits of the sort key");

// the words of LuScratch::misc
enum { LU_N_CHARTS = 0, LU_LIVE = 1, LU_OVERFLOW = 2, LU_N_SHELVES = 3, LU_CONTENT = 4 /* and 5 */, LU_WALKED = 6, LU_MISC_WORDS = 16 };

struct LuNormal {  // a triangle's unit normal and class as the scratch holds them
  float x, y, z;
  uint32_t cls;
};
DEV LuTri lu_load(const LuNormal* nrm, uint32_t t) {
  const sol_v4u w = *(const SOL_AS1 sol_v4u*)(nrm + t);
  return LuTri{__uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z), w.w};
}

__global__ __launch_bounds__(LU_WG) void sol_lightmap_unwrap_normals_kernel(const float* __restrict__ vertices, uint32_t n, uint64_t mask,
                                                                            uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                                            uint32_t* __restrict__ parent, uint32_t* __restrict__ chart_of,
                                                                            LuNormal* __restrict__ nrm, uint32_t* live_count) {
  const uint32_t t = blockIdx.x * LU_WG + threadIdx.x;
  bool live = false;
  if (t < n) {
    float pos[9];
#pragma unroll
    for (uint32_t k = 0; k < 9u; ++k) pos[k] = vertices[(size_t)t * 9 + k];
    const LuTri T = lu_triangle(pos);
    live = T.cls != SOL_LC_NONE;
    parent[t] = t;
    chart_of[t] = live ? 0u : SOL_LC_NONE;
    nrm[t] = LuNormal{T.ux, T.uy, T.uz, T.cls};
#pragma unroll
    for (uint32_t e = 0; e < 3u; ++e) {
      keys[(size_t)t * 3 + e] = live ? (lc_key_hash(lu_edge_key(pos, e)) & mask) : mask;
      vals[(size_t)t * 3 + e] = t * 3u + e;
    }
  }
  const unsigned long long b = __builtin_amdgcn_ballot_w64(live);  // (every lane of the wave arrives here)
  if ((threadIdx.x & 63u) == 0u && b != 0ull) atomicAdd(live_count, (uint32_t)__builtin_popcountll(b));
}

__global__ __launch_bounds__(LU_WG) void sol_lightmap_unwrap_match_kernel(const float* __restrict__ vertices, uint32_t n_edges,
                                                                          const uint64_t* __restrict__ keys, const uint32_t* __restrict__ order,
                                                                          const LuNormal* __restrict__ nrm, float crease_cos, uint32_t* parent) {
  const uint32_t p = blockIdx.x * LU_WG + threadIdx.x;
  if (p >= n_edges || p == 0u) return;
  const uint32_t edge = order[p], t = edge / 3u;
  const LuTri A = lu_load(nrm, t);
  if (A.cls == SOL_LC_NONE) return;
  const uint64_t h = keys[p];
  if (keys[p - 1u] != h) return;
  const LcKey K = lu_edge_key(vertices + (size_t)t * 9, edge - t * 3u);
  for (uint32_t q = p; q-- > 0u;) {
    if (keys[q] != h) break;
    const uint32_t edge2 = order[q], t2 = edge2 / 3u;
    const LuTri B = lu_load(nrm, t2);
    if (B.cls == SOL_LC_NONE || !lu_join(A, B, crease_cos)) continue;
    if (!lc_key_equal(K, lu_edge_key(vertices + (size_t)t2 * 9, edge2 - t2 * 3u))) continue;
    lc_unite(parent, t, t2);
  }
}

// ext: four arrays of n words - minimum x, minimum y (0xFFFFFFFF going in), maximum x, maximum y (0 going in)
__global__ __launch_bounds__(LU_WG) void sol_lightmap_unwrap_extents_kernel(const float* __restrict__ vertices, uint32_t n, const LuNormal* __restrict__ nrm,
                                                                            const uint32_t* __restrict__ chart_of, float texels_per_unit, uint32_t* ext) {
  const uint32_t t = blockIdx.x * LU_WG + threadIdx.x, lane = threadIdx.x & 63u;
  uint32_t c = SOL_LC_NONE, lo_x = 0xFFFFFFFFu, lo_y = 0xFFFFFFFFu, hi_x = 0u, hi_y = 0u;
  if (t < n) c = ldg_u32(chart_of + t);
  if (c != SOL_LC_NONE) {
    const uint32_t cls = ldg_u32(&nrm[t].cls);
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k) {
      float x, y;
      lu_project(vertices + (size_t)t * 9, k, cls, texels_per_unit, x, y);
      const uint32_t ox = lu_ordered(x), oy = lu_ordered(y);
      lo_x = ox < lo_x ? ox : lo_x; hi_x = ox > hi_x ? ox : hi_x;
      lo_y = oy < lo_y ? oy : lo_y; hi_y = oy > hi_y ? oy : hi_y;
    }
  }
  // Lane i takes in what lane i + s holds when both are of one chart: every word a lane gathers is of its own chart, and the first lane of a
  // run of equal charts ends with the whole run (after step s it holds the lanes [i, i + 2s) of the run). Every lane of the wave arrives here.
#pragma unroll
  for (uint32_t s = 1u; s < 64u; s <<= 1) {
    const uint32_t oc = __shfl_down(c, s), a = __shfl_down(lo_x, s), b = __shfl_down(lo_y, s), d = __shfl_down(hi_x, s), e = __shfl_down(hi_y, s);
    if (lane + s < 64u && oc == c) {
      lo_x = a < lo_x ? a : lo_x; lo_y = b < lo_y ? b : lo_y;
      hi_x = d > hi_x ? d : hi_x; hi_y = e > hi_y ? e : hi_y;
    }
  }
  const uint32_t before = __shfl_up(c, 1u);
  if (c == SOL_LC_NONE || (lane != 0u && before == c)) return;
  atomicMin(ext + c, lo_x);  // c < n_charts <= n
  atomicMin(ext + (size_t)n + c, lo_y);
  atomicMax(ext + (size_t)2 * n + c, hi_x);
  atomicMax(ext + (size_t)3 * n + c, hi_y);
}

struct LuAtlas {
  uint32_t W, H, gutter;
  float texels_per_unit;
};

__global__ __launch_bounds__(LU_WG) void sol_lightmap_unwrap_rects_kernel(LuAtlas A, uint32_t n, const uint32_t* __restrict__ ext,
                                                                          uint64_t* __restrict__ skey, uint32_t* __restrict__ sval, uint32_t* misc) {
  const uint32_t c = blockIdx.x * LU_WG + threadIdx.x;
  const uint32_t m = ldg_u32(misc + LU_N_CHARTS);
  unsigned long long content = 0ull;
  bool wide = false;
  if (c < n) {
    uint64_t key = ~0ull;
    if (c < m) {
      float f;
      const uint32_t cw = lu_content(lu_unordered(ldg_u32(ext + c)), lu_unordered(ldg_u32(ext + (size_t)2 * n + c)), f);
      const uint32_t ch = lu_content(lu_unordered(ldg_u32(ext + (size_t)n + c)), lu_unordered(ldg_u32(ext + (size_t)3 * n + c)), f);
      key = lu_sort_key(cw + A.gutter, ch + A.gutter, c);
      content = (unsigned long long)cw * ch;
      wide = cw + A.gutter > A.W;
    }
    skey[c] = key;
    sval[c] = c;
  }
  // every lane of the wave arrives here
#pragma unroll
  for (uint32_t s = 32u; s >= 1u; s >>= 1) content += __shfl_down(content, s);
  const unsigned long long any_wide = __builtin_amdgcn_ballot_w64(wide);
  if ((threadIdx.x & 63u) == 0u) {
    if (content) atomicAdd((unsigned long long*)(misc + LU_CONTENT), content);
    if (any_wide) atomicOr(misc + LU_OVERFLOW, SOL_UNWRAP_OVERFLOW_WIDTH);
  }
}

// the width a sorted key stands for (a key beyond the charts: none)
struct LuKeyWidth {
  __host__ __device__ uint64_t operator()(uint64_t k) const { return k == ~0ull ? 0ull : (uint64_t)(0xFFFFu - (uint32_t)((k >> 30) & 0xFFFFu)); }
};

// prefix[i]: the widths of the sorted rectangles 0 .. i added
__global__ __launch_bounds__(LU_WG) void sol_lightmap_unwrap_next_kernel(uint32_t W, uint32_t n, const uint64_t* __restrict__ prefix,
                                                                         const uint32_t* __restrict__ misc, uint32_t* __restrict__ next) {
  const uint32_t i = blockIdx.x * LU_WG + threadIdx.x;
  const uint32_t m = ldg_u32(misc + LU_N_CHARTS);
  if (i >= n || i >= m) return;
  const uint64_t limit = (i ? prefix[i - 1u] : 0ull) + W;
  uint32_t lo = i + 1u, hi = m;  // the first j in [i + 1, m) with prefix[j] > limit, or m
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (prefix[mid] > limit) hi = mid; else lo = mid + 1u;
  }
  next[i] = lo;
}

__global__ void sol_lightmap_unwrap_walk_kernel(LuAtlas A, const uint64_t* __restrict__ skey, const uint64_t* __restrict__ prefix,
                                                const uint32_t* __restrict__ next, uint32_t* misc, uint32_t* __restrict__ shelf_first,
                                                uint32_t* __restrict__ shelf_y, uint32_t* __restrict__ result) {
  if (blockIdx.x != 0u || threadIdx.x != 0u) return;
  const uint32_t m = misc[LU_N_CHARTS];
  uint32_t i = 0u, y = 0u, k = 0u, used_w = 0u;
  while (i < m && k < SOL_LU_MAX_SHELVES) {
    const uint32_t nx = next[i];  // i < nx <= m
    const uint32_t w = (uint32_t)(prefix[nx - 1u] - (i ? prefix[i - 1u] : 0ull));
    shelf_first[k] = i;
    shelf_y[k] = y;
    used_w = w > used_w ? w : used_w;
    y += lu_key_h(skey[i]);
    ++k;
    i = nx;
    if (y > SOL_LIGHTMAP_MAX_SIZE) break;
  }
  const uint32_t overflow = misc[LU_OVERFLOW] | (y > A.H ? SOL_UNWRAP_OVERFLOW_HEIGHT : 0u);
  misc[LU_OVERFLOW] = overflow;
  misc[LU_N_SHELVES] = k;
  misc[LU_WALKED] = i;
  result[0] = m; result[1] = misc[LU_LIVE];
  result[2] = used_w; result[3] = y;
  result[4] = overflow; result[5] = 0u;
  result[6] = misc[LU_CONTENT]; result[7] = misc[LU_CONTENT + 1];
}

__global__ __launch_bounds__(LU_WG) void sol_lightmap_unwrap_place_kernel(uint32_t n, const uint64_t* __restrict__ skey, const uint64_t* __restrict__ prefix,
                                                                          const uint32_t* __restrict__ misc, const uint32_t* __restrict__ shelf_first,
                                                                          const uint32_t* __restrict__ shelf_y, uint32_t* __restrict__ place) {
  const uint32_t i = blockIdx.x * LU_WG + threadIdx.x;
  const uint32_t m = ldg_u32(misc + LU_N_CHARTS);
  if (i >= n || i >= m) return;
  const uint32_t id = lu_key_id(skey[i]);  // < m: the keys of the charts sort before every key beyond them
  if (id >= m) return;
  uint32_t x = 0u, y = 0u;
  const uint32_t shelves = ldg_u32(misc + LU_N_SHELVES);
  if (i < ldg_u32(misc + LU_WALKED) && shelves > 0u) {  // (a rectangle the walk did not reach: the call overflows, its place is not read)
    uint32_t lo = 0u, hi = shelves;  // the last shelf whose first rectangle is at or before i
    while (hi - lo > 1u) {
      const uint32_t mid = lo + (hi - lo) / 2u;
      if (ldg_u32(shelf_first + mid) <= i) lo = mid; else hi = mid;
    }
    const uint32_t first = ldg_u32(shelf_first + lo);
    x = (uint32_t)((i ? prefix[i - 1u] : 0ull) - (first ? prefix[first - 1u] : 0ull));
    y = ldg_u32(shelf_y + lo);
  }
  place[(size_t)2 * id] = x;
  place[(size_t)2 * id + 1] = y;
}

__global__ __launch_bounds__(LU_WG) void sol_lightmap_unwrap_write_kernel(LuAtlas A, const float* __restrict__ vertices, uint32_t n,
                                                                          const LuNormal* __restrict__ nrm, const uint32_t* __restrict__ ext,
                                                                          const uint32_t* __restrict__ place, const uint32_t* __restrict__ misc,
                                                                          uint32_t* chart_of, float* __restrict__ uvs) {
  const uint32_t t = blockIdx.x * LU_WG + threadIdx.x;
  if (t >= n) return;
  const uint32_t c = chart_of[t];
  float* uv = uvs + (size_t)t * 6;
  if (c == SOL_LC_NONE || ldg_u32(misc + LU_OVERFLOW) != 0u) {
#pragma unroll
    for (uint32_t k = 0; k < 6u; ++k) uv[k] = 0.0f;
    chart_of[t] = SOL_LC_NONE;
    return;
  }
  const uint32_t cls = ldg_u32(&nrm[t].cls);
  const float fx = floorf(lu_unordered(ldg_u32(ext + c))), fy = floorf(lu_unordered(ldg_u32(ext + (size_t)n + c)));
  const uint32_t rx = ldg_u32(place + (size_t)2 * c), ry = ldg_u32(place + (size_t)2 * c + 1);
#pragma unroll
  for (uint32_t k = 0; k < 3u; ++k) {
    float x, y;
    lu_project(vertices + (size_t)t * 9, k, cls, A.texels_per_unit, x, y);
    uv[2u * k] = lu_uv(x, fx, rx, A.W);
    uv[2u * k + 1u] = lu_uv(y, fy, ry, A.H);
  }
}

// ---- launches (sol_launch.h) ----
namespace {
uint32_t lu_blocks(uint64_t n) { return (uint32_t)((n + LU_WG - 1) / LU_WG); }
}  // namespace

hipError_t sol_lightmap_unwrap_scratch(uint32_t n, LuScratch& S) {
  hipError_t e = sol_lightmap_charts_scratch(n, S.C);
  if (e != hipSuccess) return e;
  S.nrm = (S.C.words + 3) / 4 * 4;
  S.misc = S.nrm + (size_t)4 * n;
  S.shelf_first = S.misc + LU_MISC_WORDS;
  S.shelf_y = S.shelf_first + SOL_LU_MAX_SHELVES;
  S.tmp = (S.shelf_y + SOL_LU_MAX_SHELVES + 63) / 64 * 64;
  S.sort_bytes = S.scan_bytes = 0;
  e = rocprim::radix_sort_pairs(nullptr, S.sort_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0, 64,
                                (hipStream_t)0);
  if (e != hipSuccess) return e;
  e = rocprim::inclusive_scan(nullptr, S.scan_bytes, rocprim::make_transform_iterator((const uint64_t*)nullptr, LuKeyWidth()), (uint64_t*)nullptr, (size_t)n,
                              rocprim::plus<uint64_t>(), (hipStream_t)0);
  if (e != hipSuccess) return e;
  const size_t tmp_bytes = S.sort_bytes > S.scan_bytes ? S.sort_bytes : S.scan_bytes;
  S.words = S.tmp + (tmp_bytes + 3) / 4 + 64;
  return hipSuccess;
}

hipError_t sol_launch_lightmap_unwrap(const SolUnwrapConfig& c, const void* vertices, uint32_t n, bool collide, const LuScratch& S, uint32_t* scratch,
                                      void* uvs, void* chart_of, void* result, hipStream_t stream, hipEvent_t* stages) {
  hipError_t e;
  uint32_t stage = 0;
  const auto mark = [&]() { return stages ? hipEventRecord(stages[stage++], stream) : hipSuccess; };  // (SOL_LU_STAGES + 1 of them)
  if (n == 0u) return hipMemsetAsync(result, 0, sizeof(SolUnwrapResult), stream);
  const uint32_t E = n * 3u;
  const LuAtlas A{c.width, c.height, c.gutter, c.texels_per_unit};
  const float* vx = (const float*)vertices;
  // the labelling's arrays
  uint64_t* keys = (uint64_t*)(scratch + S.C.keys);
  uint64_t* keys2 = (uint64_t*)(scratch + S.C.keys2);
  uint32_t *vals = scratch + S.C.vals, *order = scratch + S.C.order, *parent = scratch + S.C.parent;
  // the rectangles' arrays, in the 18 n words of keys .. order once the labelling is done with them: 15 n words, the 64-bit ones at even offsets
  const size_t N = n;
  uint32_t* ext = scratch + S.C.keys;
  uint64_t* skey = (uint64_t*)(scratch + S.C.keys + 4 * N);
  uint64_t* skey2 = (uint64_t*)(scratch + S.C.keys + 6 * N);
  uint64_t* prefix = (uint64_t*)(scratch + S.C.keys + 8 * N);
  uint32_t *sval = scratch + S.C.keys + 10 * N, *sorder = scratch + S.C.keys + 11 * N, *next = scratch + S.C.keys + 12 * N, *place = scratch + S.C.keys + 13 * N;
  LuNormal* nrm = (LuNormal*)(scratch + S.nrm);
  uint32_t *misc = scratch + S.misc, *shelf_first = scratch + S.shelf_first, *shelf_y = scratch + S.shelf_y;
  void* tmp = scratch + S.tmp;

  if ((e = mark()) != hipSuccess) return e;
  if ((e = hipMemsetAsync(misc, 0, LU_MISC_WORDS * sizeof(uint32_t), stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(sol_lightmap_unwrap_normals_kernel, dim3(lu_blocks(n)), dim3(LU_WG), 0, stream, vx, n, collide ? 0xFull : ~0ull, keys, vals, parent,
                     (uint32_t*)chart_of, nrm, misc + LU_LIVE);
  if ((e = hipGetLastError()) != hipSuccess || (e = mark()) != hipSuccess) return e;  // normals and hash
  size_t bytes = S.C.sort_bytes;
  if ((e = rocprim::radix_sort_pairs(scratch + S.C.tmp, bytes, keys, keys2, vals, order, (size_t)E, 0, collide ? 4 : 64, stream)) != hipSuccess) return e;
  if ((e = mark()) != hipSuccess) return e;  // sort
  hipLaunchKernelGGL(sol_lightmap_unwrap_match_kernel, dim3(lu_blocks(E)), dim3(LU_WG), 0, stream, vx, E, (const uint64_t*)keys2, (const uint32_t*)order,
                     (const LuNormal*)nrm, c.crease_cos, parent);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = sol_launch_lightmap_chart_ids(n, S.C, scratch, chart_of, misc + LU_N_CHARTS, stream)) != hipSuccess) return e;
  if ((e = mark()) != hipSuccess) return e;  // unions and ids

  if ((e = hipMemsetAsync(ext, 0xFF, 2 * N * sizeof(uint32_t), stream)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(ext + 2 * N, 0, 2 * N * sizeof(uint32_t), stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(sol_lightmap_unwrap_extents_kernel, dim3(lu_blocks(n)), dim3(LU_WG), 0, stream, vx, n, (const LuNormal*)nrm, (const uint32_t*)chart_of,
                     c.texels_per_unit, ext);
  if ((e = hipGetLastError()) != hipSuccess || (e = mark()) != hipSuccess) return e;  // extents
  hipLaunchKernelGGL(sol_lightmap_unwrap_rects_kernel, dim3(lu_blocks(n)), dim3(LU_WG), 0, stream, A, n, (const uint32_t*)ext, skey, sval, misc);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  bytes = S.sort_bytes;
  if ((e = rocprim::radix_sort_pairs(tmp, bytes, skey, skey2, sval, sorder, N, 0, 64, stream)) != hipSuccess) return e;
  if ((e = mark()) != hipSuccess) return e;  // rectangles and their sort
  bytes = S.scan_bytes;
  if ((e = rocprim::inclusive_scan(tmp, bytes, rocprim::make_transform_iterator((const uint64_t*)skey2, LuKeyWidth()), prefix, N, rocprim::plus<uint64_t>(),
                                   stream)) != hipSuccess)
    return e;
  hipLaunchKernelGGL(sol_lightmap_unwrap_next_kernel, dim3(lu_blocks(n)), dim3(LU_WG), 0, stream, c.width, n, (const uint64_t*)prefix, (const uint32_t*)misc, next);
  hipLaunchKernelGGL(sol_lightmap_unwrap_walk_kernel, dim3(1), dim3(64), 0, stream, A, (const uint64_t*)skey2, (const uint64_t*)prefix, (const uint32_t*)next, misc,
                     shelf_first, shelf_y, (uint32_t*)result);
  hipLaunchKernelGGL(sol_lightmap_unwrap_place_kernel, dim3(lu_blocks(n)), dim3(LU_WG), 0, stream, n, (const uint64_t*)skey2, (const uint64_t*)prefix,
                     (const uint32_t*)misc, (const uint32_t*)shelf_first, (const uint32_t*)shelf_y, place);
  if ((e = hipGetLastError()) != hipSuccess || (e = mark()) != hipSuccess) return e;  // pack
  hipLaunchKernelGGL(sol_lightmap_unwrap_write_kernel, dim3(lu_blocks(n)), dim3(LU_WG), 0, stream, A, vx, n, (const LuNormal*)nrm, (const uint32_t*)ext,
                     (const uint32_t*)place, (const uint32_t*)misc, (uint32_t*)chart_of, (float*)uvs);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return mark();  // write
}
