// sol_lightmap_mips.hip -- lightmap mip chains: coverage-aware levels, the trilinear lookup and the level of detail of a hit (sol_lightmap_mips,
// sol_lightmap_sample_lod, sol_lightmap_lod; sol_lightmap_mips.cpp). The rule is sol_lightmap_mips.h (and sol_lightmap_sample.h,
// whose functions are called, not restated); the kernels only fetch, call it and store.
//
//   sol_lightmap_mips_level_kernel  one destination texel per lane, 64 x 4 texels per workgroup, one launch per level. LEVEL0: the source is the
//                               caller's atlas - coverage from pass_of or ownership, and the channels walked once for their finiteness before any sum.
//                               VEC: stride and addresses are multiples of 16 bytes - the four source rows come as dwordx4 and the row goes out as
//                               dwordx4; else word by word. The row is stored as it is produced and, in the rare case of a sum that overflowed,
//                               written again as zeros by the same lane.
//   sol_lightmap_mips_tail_kernel   one workgroup of 256 lanes takes a source level of at most 64 x 64 texels all the way to the last level: each
//                               level is written to the chain and to one of two LDS buffers, the next level reads the LDS copy. Only for rows of
//                               at most LMM_TAIL_MAX_STRIDE words (the two largest levels and their cover fit 64 KiB of LDS).
//   sol_lightmap_sample_lod_kernel  a lane per surface row: the steps of sol_lightmap_lookup.h once per level. Its own: the walk of the level
//                               layout, lml_taps, the cover byte of the levels above 0 and lml_blend.
//   sol_lightmap_lod_kernel     a thread per row: two dwordx4 of the ray, one of the hit, the surface row, fifteen words of the triangle; one float out.
// No atomics, no scratch; every store is a vector store.
#include <hip/hip_runtime.h>

#include "../../include/solstrale_hip.h"
#include "sol_launch.h"
#include "sol_lightmap_lookup.h"
#include "sol_lightmap_mips.h"

#define LMM_WG 256
#define LMM_TILE_W 64
#define LMM_TILE_H 4
#define LMM_TAIL_MAX_SIZE 64u
#define LMM_TAIL_MAX_STRIDE 12u  // (1024 + 256) rows of 4 * 12 + 1 bytes = 62720 bytes of LDS

static_assert(sizeof(SolRayHit) == 32 && sizeof(SolTexel) == 16 && sizeof(SolRay) == 32, "the records of include/solstrale_hip.h");
static_assert(SOL_LMM_MAX_LEVELS == SOL_LIGHTMAP_MAX_LEVELS, "the level count of include/solstrale_hip.h");

// ---- the sources of a reduction ----
struct LmmSrc0 {  // level 0: the caller's atlas
  const uint32_t* texels;
  const uint8_t* pass_of;
  const uint32_t* values;
  uint32_t W, channels, stride_words;
  DEV size_t at(uint32_t i, uint32_t j) const { return (size_t)j * W + i; }
  DEV bool live(uint32_t i, uint32_t j) const {
    const size_t a = at(i, j);
    if (!ls_covered(pass_of != nullptr, pass_of ? (uint32_t)ldg_u8(pass_of + a) : 0u, pass_of ? 0u : ldg_u32(texels + a * 4))) return false;
    const SOL_AS1 uint32_t* row = (const SOL_AS1 uint32_t*)(values + a * stride_words);
    bool finite = true;
    for (uint32_t c = 0; c < channels; ++c) finite = finite && lf_finite(__uint_as_float(row[c]));
    return finite;
  }
  DEV uint32_t word(uint32_t i, uint32_t j, uint32_t w) const { return ((const SOL_AS1 uint32_t*)values)[at(i, j) * stride_words + w]; }
};
struct LmmSrcLevel {  // a level of the chain in global memory
  const uint32_t* rows;
  const uint8_t* cover;
  uint32_t W, stride_words;
  DEV size_t at(uint32_t i, uint32_t j) const { return (size_t)j * W + i; }
  DEV bool live(uint32_t i, uint32_t j) const { return ldg_u8(cover + at(i, j)) == 0u; }
  DEV uint32_t word(uint32_t i, uint32_t j, uint32_t w) const { return ((const SOL_AS1 uint32_t*)rows)[at(i, j) * stride_words + w]; }
};
struct LmmSrcLds {  // a level of the chain in LDS
  const uint32_t* rows;
  const uint8_t* cover;
  uint32_t W, stride_words;
  DEV bool live(uint32_t i, uint32_t j) const { return cover[j * W + i] == 0u; }
  DEV uint32_t word(uint32_t i, uint32_t j, uint32_t w) const { return rows[(j * W + i) * stride_words + w]; }
};
struct LmmDst {  // a row of the chain, and its copy in LDS or null
  uint32_t* row;
  uint32_t* lds;
  DEV void put(uint32_t w, uint32_t bits) {
    row[w] = bits;
    if (lds) lds[w] = bits;
  }
};

// the four taps of destination texel (i, j) as a mask of the live ones
template <typename Src>
DEV uint32_t lmm_live_taps(const Src& S, uint32_t Ws, uint32_t Hs, uint32_t i, uint32_t j) {
  uint32_t live = 0u;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    const uint32_t ti = 2u * i + (k & 1u), tj = 2u * j + (k >> 1);
    if (ti < Ws && tj < Hs && S.live(ti, tj)) live |= 1u << k;
  }
  return live;
}

template <bool LEVEL0, bool VEC>
__global__ __launch_bounds__(LMM_WG) void sol_lightmap_mips_level_kernel(const uint32_t* __restrict__ texels, const uint8_t* __restrict__ pass_of,
                                                                         const uint32_t* __restrict__ src_rows, const uint8_t* __restrict__ src_cover,
                                                                         uint32_t Ws, uint32_t Hs, uint32_t Wd, uint32_t Hd, uint32_t channels,
                                                                         uint32_t stride_words, uint32_t* __restrict__ dst_rows,
                                                                         uint8_t* __restrict__ dst_cover) {
  const uint32_t i = blockIdx.x * LMM_TILE_W + (threadIdx.x % LMM_TILE_W), j = blockIdx.y * LMM_TILE_H + (threadIdx.x / LMM_TILE_W);
  if (i >= Wd || j >= Hd) return;
  const size_t at = (size_t)j * Wd + i;
  uint32_t* out = dst_rows + at * stride_words;
  uint32_t live;
  if constexpr (LEVEL0) {
    live = lmm_live_taps(LmmSrc0{texels, pass_of, src_rows, Ws, channels, stride_words}, Ws, Hs, i, j);
  } else {
    live = lmm_live_taps(LmmSrcLevel{src_rows, src_cover, Ws, stride_words}, Ws, Hs, i, j);
  }
  if constexpr (VEC) {
    const uint32_t groups = stride_words / 4u;
    const uint32_t c = (uint32_t)__builtin_popcount(live);
    if (c == 0u) {
      for (uint32_t g = 0; g < groups; ++g) ((SOL_AS1 sol_v4u*)out)[g] = sol_v4u{0u, 0u, 0u, 0u};
      dst_cover[at] = (uint8_t)SOL_LMM_UNCOVERED;
      return;
    }
    const float fc = (float)c;
    const uint32_t first = (uint32_t)__builtin_ctz(live);
    const size_t a0 = ((size_t)(2u * j) * Ws + 2u * i) * stride_words, step_i = stride_words, step_j = (size_t)Ws * stride_words;
    bool finite = true;
    for (uint32_t g = 0; g < groups; ++g) {
      sol_v4u x[4];
#pragma unroll
      for (uint32_t k = 0; k < 4u; ++k)
        x[k] = (live & (1u << k)) ? ((const SOL_AS1 sol_v4u*)(src_rows + a0 + (k & 1u) * step_i + (k >> 1) * step_j))[g] : sol_v4u{0u, 0u, 0u, 0u};
      const sol_v4u f = first == 0u ? x[0] : first == 1u ? x[1] : first == 2u ? x[2] : x[3];
      sol_v4u r;
#pragma unroll
      for (uint32_t e = 0; e < 4u; ++e) {
        if (4u * g + e < channels) {
          const float m = lmm_mean(live, __uint_as_float(x[0][e]), __uint_as_float(x[1][e]), __uint_as_float(x[2][e]), __uint_as_float(x[3][e]), fc);
          finite = finite && lf_finite(m);
          r[e] = __float_as_uint(m);
        } else {
          r[e] = f[e];
        }
      }
      ((SOL_AS1 sol_v4u*)out)[g] = r;
    }
    if (!finite)
      for (uint32_t g = 0; g < groups; ++g) ((SOL_AS1 sol_v4u*)out)[g] = sol_v4u{0u, 0u, 0u, 0u};
    dst_cover[at] = finite ? (uint8_t)0u : (uint8_t)SOL_LMM_UNCOVERED;
  } else {
    LmmDst D{out, nullptr};
    uint32_t cover;
    if constexpr (LEVEL0) {
      cover = lmm_reduce(LmmSrc0{texels, pass_of, src_rows, Ws, channels, stride_words}, live, i, j, channels, stride_words, D);
    } else {
      cover = lmm_reduce(LmmSrcLevel{src_rows, src_cover, Ws, stride_words}, live, i, j, channels, stride_words, D);
    }
    dst_cover[at] = (uint8_t)cover;
  }
}

// One step of the tail: level (Ws x Hs, through S) -> level (Wd x Hd) at dst_rows / dst_cover and into the LDS copy.
template <typename Src>
DEV void lmm_tail_step(const Src& S, uint32_t Ws, uint32_t Hs, uint32_t Wd, uint32_t Hd, uint32_t channels, uint32_t stride_words, uint32_t* dst_rows,
                       uint8_t* dst_cover, uint32_t* lds_rows, uint8_t* lds_cover) {
  for (uint32_t t = threadIdx.x; t < Wd * Hd; t += LMM_WG) {
    const uint32_t i = t % Wd, j = t / Wd;
    LmmDst D{dst_rows + (size_t)t * stride_words, lds_rows + t * stride_words};
    const uint32_t cover = lmm_reduce(S, lmm_live_taps(S, Ws, Hs, i, j), i, j, channels, stride_words, D);
    dst_cover[t] = (uint8_t)cover;
    lds_cover[t] = (uint8_t)cover;
  }
}

// src: level `s` (LEVEL0: the caller's atlas), Ws x Hs <= 64 x 64; dst_rows / dst_cover: the chain from level s + 1 on; steps: the levels to make.
// LDS: rows_a (na rows), rows_b (nb rows), cover_a, cover_b - na, nb: the sizes of levels s + 1 and s + 2.
template <bool LEVEL0>
__global__ __launch_bounds__(LMM_WG) void sol_lightmap_mips_tail_kernel(const uint32_t* __restrict__ texels, const uint8_t* __restrict__ pass_of,
                                                                        const uint32_t* src_rows, const uint8_t* src_cover, uint32_t Ws, uint32_t Hs,
                                                                        uint32_t steps, uint32_t channels, uint32_t stride_words, uint32_t* dst_rows,
                                                                        uint8_t* dst_cover) {
  extern __shared__ uint32_t lmm_lds[];
  uint32_t Wd = (Ws + 1u) / 2u, Hd = (Hs + 1u) / 2u;
  const uint32_t na = Wd * Hd, nb = ((Wd + 1u) / 2u) * ((Hd + 1u) / 2u);
  uint32_t* rows_ab[2] = {lmm_lds, lmm_lds + na * stride_words};
  uint8_t* cover_a = (uint8_t*)(lmm_lds + (na + nb) * stride_words);
  uint8_t* cover_ab[2] = {cover_a, cover_a + na};
  if constexpr (LEVEL0) {
    lmm_tail_step(LmmSrc0{texels, pass_of, src_rows, Ws, channels, stride_words}, Ws, Hs, Wd, Hd, channels, stride_words, dst_rows, dst_cover, rows_ab[0],
                  cover_ab[0]);
  } else {
    lmm_tail_step(LmmSrcLevel{src_rows, src_cover, Ws, stride_words}, Ws, Hs, Wd, Hd, channels, stride_words, dst_rows, dst_cover, rows_ab[0], cover_ab[0]);
  }
  size_t at = (size_t)Wd * Hd;
  for (uint32_t k = 1; k < steps; ++k) {
    __syncthreads();
    Ws = Wd; Hs = Hd;
    Wd = (Ws + 1u) / 2u; Hd = (Hs + 1u) / 2u;
    const uint32_t from = (k - 1u) & 1u, to = k & 1u;
    lmm_tail_step(LmmSrcLds{from ? rows_ab[1] : rows_ab[0], from ? cover_ab[1] : cover_ab[0], Ws, stride_words}, Ws, Hs, Wd, Hd, channels, stride_words,
                  dst_rows + at * stride_words, dst_cover + at, to ? rows_ab[1] : rows_ab[0], to ? cover_ab[1] : cover_ab[0]);
    at += (size_t)Wd * Hd;
  }
}

// ---- the trilinear lookup ----
struct LmlAtlas {
  uint32_t W, H, channels, stride_words, n_triangles, levels;
  uint32_t guard;
  float chart_radius;
};
// One level of a row's lookup: the taps, the covered ones, then the live ones and their weights. rows: the level's.
struct LmlLevel {
  LsTaps T;
  uint32_t live, W;
  LsWeights R;
  const float* rows;
};
// a tap of a level above 0: its cover byte (level 0 has texels / pass_of instead: LsGuardTest)
struct LmlCoverTest {
  const uint8_t* cover;
  DEV bool operator()(size_t at) const { return ls_covered(true, (uint32_t)ldg_u8(cover + at), 0u); }
};

__global__ __launch_bounds__(LMM_WG) void sol_lightmap_sample_lod_kernel(LmlAtlas A, const float* __restrict__ uvs, const uint32_t* __restrict__ texels,
                                                                         const uint8_t* __restrict__ pass_of, const float* __restrict__ values,
                                                                         const float* __restrict__ mips, const uint8_t* __restrict__ cover,
                                                                         const float* __restrict__ vertices, const float* __restrict__ points,
                                                                         const uint32_t* __restrict__ coords, const float* __restrict__ lods, uint32_t n,
                                                                         uint32_t* __restrict__ out) {
  const uint32_t x = blockIdx.x * LMM_WG + threadIdx.x;
  if (x >= n) return;
  const sol_v4u row = *(const SOL_AS1 sol_v4u*)(coords + (size_t)x * 4);
  uint32_t* o = out + (size_t)x * (A.channels + 1u);
  const LsSurface S = ls_surface(row, A.n_triangles, uvs, vertices, A.guard != 0u);  // 1. the row

  // 2. the two levels and the fraction
  const float lambda = lml_clamp(((const SOL_AS1 float*)lods)[x], A.levels);
  const float lf = floorf(lambda), f = lambda - lf;
  const uint32_t l0 = (uint32_t)lf;
  const bool two = f != 0.0f;  // (then l0 + 1 <= levels - 1: lambda < levels - 1)
  LmlLevel L[2];
#pragma unroll
  for (uint32_t s = 0; s < 2u; ++s) {
    LmlLevel& Q = L[s];
    Q.T = LsTaps{0, 0, 0.0f, 0.0f, 0u};
    Q.live = 0u; Q.W = 1u; Q.rows = values;
    const uint32_t l = l0 + s;
    if (!S.valid || (s == 1u && !two)) continue;
    // the level's size and place by the layout rule
    uint32_t Wl = A.W, Hl = A.H;
    size_t at = 0;
    for (uint32_t k = 1; k <= l; ++k) {
      Wl = (Wl + 1u) / 2u; Hl = (Hl + 1u) / 2u;
      if (k < l) at += (size_t)Wl * Hl;
    }
    Q.W = Wl;
    Q.T = l == 0u ? ls_taps(S.u, S.v, A.W, A.H, false) : lml_taps(S.u, S.v, A.W, A.H, l, Wl, Hl);
    Q.rows = l == 0u ? values : mips + at * A.stride_words;
    // 3. coverage (and at level 0 the chart guard) of every tap, before any value is fetched
    Q.live = l == 0u ? ls_live_taps(Q.T, Wl, Hl, ls_guard_test(texels, pass_of, points, A.guard != 0u, S, A.chart_radius))
                     : ls_live_taps(Q.T, Wl, Hl, LmlCoverTest{cover + at});
  }
  // 4. the value words of the covered taps: one that is not finite takes its tap out; then weights, wsum and count
#pragma unroll
  for (uint32_t s = 0; s < 2u; ++s) L[s].R = ls_weights(L[s].T, ls_drop_nonfinite(L[s].live, L[s].T, L[s].W, L[s].rows, A.stride_words, A.channels));
  // 5. the answer
  const bool have_a = L[0].R.live != 0u, have_b = L[1].R.live != 0u;
  const float g = 1.0f - f;
  const LsAt at_a = ls_at(L[0].T, L[0].W, A.stride_words), at_b = ls_at(L[1].T, L[1].W, A.stride_words);
  for (uint32_t c = 0; c < A.channels; ++c) {
    float a = 0.0f, b = 0.0f;
    if (have_a) a = ls_bilinear(L[0].R, L[0].rows, at_a, c);
    if (have_b) b = ls_bilinear(L[1].R, L[1].rows, at_b, c);
    o[c] = (have_a && have_b) ? __float_as_uint(lml_blend(a, b, g, f)) : have_a ? __float_as_uint(a) : have_b ? __float_as_uint(b) : 0u;
  }
  o[A.channels] = L[0].R.count + L[1].R.count;
}

// ---- the level of detail of a hit ----
__global__ __launch_bounds__(LMM_WG) void sol_lightmap_lod_kernel(const uint32_t* __restrict__ rays, const uint32_t* __restrict__ hits,
                                                                  const uint32_t* __restrict__ coords, uint32_t n, const float* __restrict__ vertices,
                                                                  const float* __restrict__ uvs, uint32_t n_triangles, uint32_t W, uint32_t H, float spread,
                                                                  float bias, float* __restrict__ out) {
  const uint32_t x = blockIdx.x * LMM_WG + threadIdx.x;
  if (x >= n) return;
  const sol_v4f r0 = *(const SOL_AS1 sol_v4f*)(rays + (size_t)x * 8), r1 = *(const SOL_AS1 sol_v4f*)(rays + (size_t)x * 8 + 4);
  const sol_v4u h0 = *(const SOL_AS1 sol_v4u*)(hits + (size_t)x * 8);  // (t, u, v, status)
  const sol_v4u row = *(const SOL_AS1 sol_v4u*)(coords + (size_t)x * 4);
  const float t = __uint_as_float(h0.x);
  float lambda = 0.0f;
  const bool ok = h0.w == SOL_RAY_HIT && ls_row_listed(row, n_triangles) && lf_finite(t) && t > 0.0f && lf_finite(r0.x) &&
                  lf_finite(r0.y) && lf_finite(r0.z) && lf_finite(r1.x) && lf_finite(r1.y) && lf_finite(r1.z);
  if (ok) {
    float uv[6], pos[9];
    const SOL_AS1 float* a = (const SOL_AS1 float*)(uvs + (size_t)row.x * 6);
    const SOL_AS1 float* p = (const SOL_AS1 float*)(vertices + (size_t)row.x * 9);
#pragma unroll
    for (int k = 0; k < 6; ++k) uv[k] = a[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) pos[k] = p[k];
    lambda = lml_lod(uv, pos, r1.x, r1.y, r1.z, t, W, H, spread, bias);
  }
  ((SOL_AS1 float*)out)[x] = lambda;
}

// ---- launches (sol_launch.h) ----
namespace {
template <bool LEVEL0>
void launch_level(bool vec, const void* texels, const void* pass_of, const void* src_rows, const void* src_cover, uint32_t Ws, uint32_t Hs, uint32_t Wd,
                  uint32_t Hd, uint32_t channels, uint32_t stride_words, void* dst_rows, void* dst_cover, hipStream_t stream) {
  const dim3 grid((Wd + LMM_TILE_W - 1) / LMM_TILE_W, (Hd + LMM_TILE_H - 1) / LMM_TILE_H);
  if (vec)
    hipLaunchKernelGGL((sol_lightmap_mips_level_kernel<LEVEL0, true>), grid, dim3(LMM_WG), 0, stream, (const uint32_t*)texels, (const uint8_t*)pass_of,
                       (const uint32_t*)src_rows, (const uint8_t*)src_cover, Ws, Hs, Wd, Hd, channels, stride_words, (uint32_t*)dst_rows, (uint8_t*)dst_cover);
  else
    hipLaunchKernelGGL((sol_lightmap_mips_level_kernel<LEVEL0, false>), grid, dim3(LMM_WG), 0, stream, (const uint32_t*)texels, (const uint8_t*)pass_of,
                       (const uint32_t*)src_rows, (const uint8_t*)src_cover, Ws, Hs, Wd, Hd, channels, stride_words, (uint32_t*)dst_rows, (uint8_t*)dst_cover);
}
}  // namespace

hipError_t sol_launch_lightmap_mips(const LmmLayout& L, uint32_t channels, uint32_t stride_words, bool tail, const void* texels, const void* pass_of,
                                    const void* values, void* mips, void* cover, hipStream_t stream) {
  const bool vec = stride_words % 4u == 0u && ((uintptr_t)values % 16u) == 0u && ((uintptr_t)mips % 16u) == 0u;
  const size_t row = (size_t)stride_words * 4;
  // the one place where the shape is chosen: level launches down to the first level of at most 64 x 64, then the tail - if its rows fit LDS
  const bool may_tail = tail && stride_words <= LMM_TAIL_MAX_STRIDE;
  for (uint32_t l = 0; l + 1u < L.levels; ++l) {  // level l -> level l + 1
    const void* src_rows = l == 0u ? values : (const char*)mips + L.at[l] * row;
    const void* src_cover = l == 0u ? nullptr : (const char*)cover + L.at[l];
    void* dst_rows = (char*)mips + L.at[l + 1u] * row;
    void* dst_cover = (char*)cover + L.at[l + 1u];
    if (may_tail && L.w[l] <= LMM_TAIL_MAX_SIZE && L.h[l] <= LMM_TAIL_MAX_SIZE) {
      const uint32_t steps = L.levels - 1u - l;
      const size_t na = (size_t)L.w[l + 1u] * L.h[l + 1u], nb = (size_t)((L.w[l + 1u] + 1u) / 2u) * ((L.h[l + 1u] + 1u) / 2u);
      const size_t lds = (na + nb) * row + ((na + nb + 3) / 4) * 4;
      if (l == 0u)
        hipLaunchKernelGGL((sol_lightmap_mips_tail_kernel<true>), dim3(1), dim3(LMM_WG), lds, stream, (const uint32_t*)texels, (const uint8_t*)pass_of,
                           (const uint32_t*)src_rows, (const uint8_t*)src_cover, L.w[l], L.h[l], steps, channels, stride_words, (uint32_t*)dst_rows,
                           (uint8_t*)dst_cover);
      else
        hipLaunchKernelGGL((sol_lightmap_mips_tail_kernel<false>), dim3(1), dim3(LMM_WG), lds, stream, (const uint32_t*)texels, (const uint8_t*)pass_of,
                           (const uint32_t*)src_rows, (const uint8_t*)src_cover, L.w[l], L.h[l], steps, channels, stride_words, (uint32_t*)dst_rows,
                           (uint8_t*)dst_cover);
      return hipGetLastError();
    }
    if (l == 0u)
      launch_level<true>(vec, texels, pass_of, src_rows, src_cover, L.w[l], L.h[l], L.w[l + 1u], L.h[l + 1u], channels, stride_words, dst_rows, dst_cover, stream);
    else
      launch_level<false>(vec, texels, pass_of, src_rows, src_cover, L.w[l], L.h[l], L.w[l + 1u], L.h[l + 1u], channels, stride_words, dst_rows, dst_cover, stream);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t sol_launch_lightmap_sample_lod(const SolLightmapLodConfig& c, const LmmLayout& L, uint32_t n_triangles, const void* uvs, const void* texels,
                                          const void* pass_of, const void* values, const void* mips, const void* cover, const void* vertices,
                                          const void* points, const void* coords, const void* lods, uint32_t n, void* out, hipStream_t stream) {
  const bool guard = vertices && points && (__builtin_isfinite(c.chart_radius) != 0);
  const LmlAtlas A{c.width, c.height, c.channels, c.stride_bytes / 4u, n_triangles, L.levels, guard ? 1u : 0u, guard ? c.chart_radius : 0.0f};
  hipLaunchKernelGGL(sol_lightmap_sample_lod_kernel, dim3((uint32_t)(((uint64_t)n + LMM_WG - 1) / LMM_WG)), dim3(LMM_WG), 0, stream, A, (const float*)uvs,
                     (const uint32_t*)texels, (const uint8_t*)pass_of, (const float*)values, (const float*)mips, (const uint8_t*)cover,
                     (const float*)vertices, (const float*)points, (const uint32_t*)coords, (const float*)lods, n, (uint32_t*)out);
  return hipGetLastError();
}

hipError_t sol_launch_lightmap_lod(const void* rays, const void* hits, const void* coords, uint32_t n, const void* vertices, const void* uvs,
                                   uint32_t n_triangles, uint32_t W, uint32_t H, float spread, float bias, void* out, hipStream_t stream) {
  hipLaunchKernelGGL(sol_lightmap_lod_kernel, dim3((uint32_t)(((uint64_t)n + LMM_WG - 1) / LMM_WG)), dim3(LMM_WG), 0, stream, (const uint32_t*)rays,
                     (const uint32_t*)hits, (const uint32_t*)coords, n, (const float*)vertices, (const float*)uvs, n_triangles, W, H, spread, bias,
                     (float*)out);
  return hipGetLastError();
}
