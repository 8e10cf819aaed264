// sol_lightmap_lookup.h -- the fetch-and-judge steps of a lightmap lookup as device functions, for sol_lightmap_sample_lod_kernel and
// sol_lightmap_sh_kernel (and the row predicate of sol_lightmap_normals_kernel and sol_lightmap_lod_kernel); DESIGN.md 29..31. The arithmetic
// is sol_lightmap_sample.h's, called, not restated; this text is what stands around it - which words are judged before anything is an address,
// in which order taps are refused, and when nothing is live:
//
//   1. the row      ls_row_listed / ls_row_valid, ls_surface: flags, SOL_LS_NONE, < n_triangles, finite b1 and b2; then the triangle's six UV
//                   words and, with the chart guard, its nine vertex words, each judged finite. Nothing is an address before it is known to be one.
//   2. the taps     ls_tap_live / ls_live_taps: a tap must lie inside the level; what then decides it is the caller's test of the texel index -
//                   LsGuardTest (coverage from pass_of or the SolTexel, then the chart guard against the tap's point row), or a kernel's own.
//                   A tap that is not covered, or that the test refuses, fetches no value word.
//   3. finiteness   ls_drop_nonfinite: the covered taps' value words are walked once; a tap with ONE word that is not finite must not contribute
//                   to ANY channel, so this cannot wait for the sums. The sums then read what this walk brought into the cache.
//   4. weights      ls_weights: w[4], wsum = ((0 + w_a) + w_b) .. over the live taps in tap order, count; !(wsum > 0): nothing is live.
//   5. the answer   ls_bilinear: sum / wsum of one channel over the live taps in tap order.
// sol_lightmap_sample_kernel and sol_lightmap_sample_charts_kernel do NOT call these: built on them they measured 0.3 to 1.2 % slower in their
// coherent three-channel cases, so they keep the text they had, which these functions restate (profiles/lightmap_lookup_fold.txt). A change to a
// step is made here and in those two kernels.
// No LDS, no atomics, no exchange between lanes: no function here holds a ballot, a barrier or a shuffle, so a kernel may call them predicated
// by lane. Taps are added in tap order by the calling lane: no answer depends on the schedule.
#pragma once
#include "sol_lightmap_sample.h"

// ---- 1. the surface row ----
DEV bool ls_row_listed(const sol_v4u& row, uint32_t n_triangles) { return row.w != 0u && row.x != SOL_LS_NONE && row.x < n_triangles; }
DEV bool ls_row_valid(const sol_v4u& row, uint32_t n_triangles) {
  return ls_row_listed(row, n_triangles) && lf_finite(__uint_as_float(row.y)) && lf_finite(__uint_as_float(row.z));
}

// The atlas coordinates (u, v) of a row and, with the guard, its point P; !valid: none of them means anything.
struct LsSurface {
  bool valid;
  float u, v, px, py, pz;
};
DEV LsSurface ls_surface(const sol_v4u& row, uint32_t n_triangles, const float* __restrict__ uvs, const float* __restrict__ vertices, bool guard) {
  const float b1 = __uint_as_float(row.y), b2 = __uint_as_float(row.z);
  LsSurface s = {ls_row_valid(row, n_triangles), 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float uv[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  const float b0 = (1.0f - b1) - b2;
  if (s.valid) {
    const SOL_AS1 float* t = (const SOL_AS1 float*)(uvs + (size_t)row.x * 6);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      uv[k] = t[k];
      s.valid = s.valid && lf_finite(uv[k]);
    }
    if (guard) {
      const SOL_AS1 float* p = (const SOL_AS1 float*)(vertices + (size_t)row.x * 9);
      float v[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        v[k] = p[k];
        s.valid = s.valid && lf_finite(v[k]);
      }
      s.px = ls_lerp3(v[0], v[3], v[6], b0, b1, b2);
      s.py = ls_lerp3(v[1], v[4], v[7], b0, b1, b2);
      s.pz = ls_lerp3(v[2], v[5], v[8], b0, b1, b2);
    }
  }
  s.u = ls_lerp3(uv[0], uv[2], uv[4], b0, b1, b2);
  s.v = ls_lerp3(uv[1], uv[3], uv[5], b0, b1, b2);
  return s;
}
// the taps of a surface row at level 0 (none for a row that is not valid)
DEV LsTaps ls_surface_taps(const LsSurface& s, uint32_t W, uint32_t H, bool nearest) {
  LsTaps T = {0, 0, 0.0f, 0.0f, 0u};
  if (s.valid) T = ls_taps(s.u, s.v, W, H, nearest);
  return T;
}

// ---- 2. the tap decision ----
// Tap k of T in a level of W x H texels: there is such a tap, it lies inside, and `test` accepts its texel index. One exit: a lane that is
// refused early still arrives where the caller exchanges.
template <typename Test>
DEV bool ls_tap_live(const LsTaps& T, uint32_t k, uint32_t W, uint32_t H, const Test& test) {
  bool yes = false;
  if (k < T.n) {  // (T.n <= 4)
    const int i = ls_tap_i(T, k), j = ls_tap_j(T, k);
    if (ls_tap_inside(i, j, W, H)) yes = test((size_t)j * W + (size_t)i);
  }
  return yes;
}
// all four, by one lane; bit k: tap k
template <typename Test>
DEV uint32_t ls_live_taps(const LsTaps& T, uint32_t W, uint32_t H, const Test& test) {
  uint32_t live = 0u;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k)
    if (ls_tap_live(T, k, W, H, test)) live |= 1u << k;
  return live;
}
// Level 0 of an atlas: coverage from pass_of (or, without one, from the SolTexel), then the chart guard of P against the tap's point row.
struct LsGuardTest {
  const uint32_t* texels;
  const uint8_t* pass_of;
  const float* points;
  bool guard;
  float px, py, pz, r2;
  DEV bool operator()(size_t at) const {
    sol_v4u tx = {0u, 0u, 0u, 0u};
    if (!pass_of || guard) tx = *(const SOL_AS1 sol_v4u*)(texels + at * 4);
    bool yes = ls_covered(pass_of != nullptr, pass_of ? (uint32_t)ldg_u8(pass_of + at) : 0u, tx.x);
    if (yes && guard && tx.w != 0u) {
      const sol_v4f q = *(const SOL_AS1 sol_v4f*)(points + at * 8);
      yes = ls_guard(tx.w, q.x, q.y, q.z, px, py, pz, r2);
    }
    return yes;
  }
};
DEV LsGuardTest ls_guard_test(const uint32_t* texels, const uint8_t* pass_of, const float* points, bool guard, const LsSurface& s, float chart_radius) {
  return LsGuardTest{texels, pass_of, points, guard, s.px, s.py, s.pz, chart_radius * chart_radius};
}

// ---- 3. the finiteness walk ----
// where the words of tap 0 start in `rows`, and the steps to its neighbours (not an address unless the tap is live)
struct LsAt {
  size_t at0, step_i, step_j;
};
DEV LsAt ls_at(const LsTaps& T, uint32_t W, uint32_t stride_words) {
  return LsAt{((size_t)T.j0 * W + (size_t)T.i0) * stride_words, stride_words, (size_t)W * stride_words};
}
DEV uint32_t ls_drop_nonfinite(uint32_t live, const LsTaps& T, uint32_t W, const float* rows, uint32_t stride_words, uint32_t channels) {
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    if (!(live & (1u << k))) continue;
    const SOL_AS1 float* val = (const SOL_AS1 float*)(rows + ((size_t)ls_tap_j(T, k) * W + (size_t)ls_tap_i(T, k)) * stride_words);
    bool finite = true;
    for (uint32_t c = 0; c < channels; ++c) finite = finite && lf_finite(val[c]);
    if (!finite) live &= ~(1u << k);
  }
  return live;
}

// ---- 4. weights, wsum, count ----
struct LsWeights {
  float w[4], wsum;
  uint32_t live, count;
};
DEV LsWeights ls_weights(const LsTaps& T, uint32_t live) {
  LsWeights R;
  R.wsum = 0.0f;
  R.live = live;
  R.count = 0u;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    R.w[k] = ls_tap_weight(T, k);
    if (live & (1u << k)) {
      R.wsum = R.wsum + R.w[k];
      ++R.count;
    }
  }
  if (!(R.wsum > 0.0f)) R.live = 0u, R.count = 0u;
  return R;
}

// ---- 5. the answer ----
// channel c of the live taps (R.live != 0)
DEV float ls_bilinear(const LsWeights& R, const float* rows, const LsAt& a, uint32_t c) {
  float sum = 0.0f;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k)
    if (R.live & (1u << k)) sum = sum + (R.w[k] * ((const SOL_AS1 float*)rows)[a.at0 + (k & 1u) * a.step_i + (k >> 1) * a.step_j + c]);
  return sum / R.wsum;
}
