// sol_lightmap_charts.h -- the rule of the lightmap charts (sol_lightmap_charts, sol_lightmap_dilate_charts, sol_lightmap_sample_charts,
// sol_lightmap_chart_levels, include/solstrale_hip.h), operation by operation. The kernels of sol_lightmap_charts.hip only fetch,
// call this text and store. Compiled with -ffp-contract=off: every expression is the plain fp32 sequence it spells and `/` is correctly rounded,
// so that tests/lightmap_charts_ref.py can restate the rule in numpy float32 and compare the words. The lookup and the neighbour order are
// sol_lightmap_sample.h's and sol_lightmap.h's, called, not restated; the levels are lmm_layout's (sol_launch.h).
//
//   edge key      edge e of a triangle joins corners e and (e + 1) % 3. An end point is (u, v) or (u, v, x, y, z), every word x + 0.0f (so that
//                 -0 is +0: equal numbers have equal bits; a live triangle has finite words only). The key is the two end points, the lower one
//                 first - lower: the first differing word, as an unsigned integer, is smaller. Two edges are one when their keys are equal
//                 word for word; the 64-bit hash only sorts candidates together and decides nothing.
//   union-find    parent[x] <= x at all times: a find walks strictly downward and ends (a union's find also halves the path it walks); a union
//                 hooks the higher root under the lower with one atomicCAS and looks again when the exchange fails. A component's root is its
//                 lowest index whatever the schedule.
//   dilation      the chart of a filled texel: the chart held by the most of its covered neighbours, the lowest id on a tie.
//   levels        a level word is a chart id, SOL_LC_NONE or SOL_LC_MIXED.
#pragma once
#include "sol_lightmap.h"
#include "sol_lightmap_sample.h"
#include "sol_launch.h"

#define SOL_LC_NONE 0xFFFFFFFFu
#define SOL_LC_MIXED 0xFFFFFFFEu

// ---- the labelling ----
// the bits of a word as the keys hold them
DEV uint32_t lc_canon(float x) { return __float_as_uint(x + 0.0f); }

// The key of one edge: ten words with vertices, four without (the rest stays zero): (u, v, x, y, z) of the lower end point, then the other's.
struct LcKey {
  uint32_t w[10];
};
// uv: the triangle's 6 words, pos: its 9 words or null; e: 0, 1, 2
DEV LcKey lc_edge_key(const float* uv, const float* pos, uint32_t e) {
  const uint32_t a = e, b = e == 2u ? 0u : e + 1u;
  uint32_t pa[5] = {lc_canon(uv[2u * a]), lc_canon(uv[2u * a + 1u]), 0u, 0u, 0u}, pb[5] = {lc_canon(uv[2u * b]), lc_canon(uv[2u * b + 1u]), 0u, 0u, 0u};
  if (pos) {
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k) {
      pa[2u + k] = lc_canon(pos[3u * a + k]);
      pb[2u + k] = lc_canon(pos[3u * b + k]);
    }
  }
  bool swap = false, decided = false;  // b before a: the first differing word of b is the smaller
#pragma unroll
  for (uint32_t k = 0; k < 5u; ++k) {
    if (!decided && pa[k] != pb[k]) {
      swap = pb[k] < pa[k];
      decided = true;
    }
  }
  LcKey K;
#pragma unroll
  for (uint32_t k = 0; k < 5u; ++k) {
    K.w[k] = swap ? pb[k] : pa[k];
    K.w[5u + k] = swap ? pa[k] : pb[k];
  }
  return K;
}
DEV bool lc_key_equal(const LcKey& a, const LcKey& b) {
  bool eq = true;
#pragma unroll
  for (uint32_t k = 0; k < 10u; ++k) eq = eq && a.w[k] == b.w[k];
  return eq;
}
// a 64-bit mix of the key's words; what it is changes no label
DEV uint64_t lc_key_hash(const LcKey& K) {
  uint64_t h = 0x9E3779B97F4A7C15ull;
#pragma unroll
  for (uint32_t k = 0; k < 10u; ++k) {
    h = (h ^ (uint64_t)K.w[k]) * 0xBF58476D1CE4E5B9ull;
    h = h ^ (h >> 29);
  }
  h = h * 0x94D049BB133111EBull;
  return h ^ (h >> 32);
}
// a triangle is live when every word of it is finite
DEV bool lc_triangle_live(const float* uv, const float* pos) {
  bool live = true;
#pragma unroll
  for (uint32_t k = 0; k < 6u; ++k) live = live && lf_finite(uv[k]);
  if (pos) {
#pragma unroll
    for (uint32_t k = 0; k < 9u; ++k) live = live && lf_finite(pos[k]);
  }
  return live;
}

// parent[] is read and written by many lanes at once: every access is one relaxed atomic word
DEV uint32_t lc_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
DEV uint32_t lc_find(const uint32_t* parent, uint32_t x) {
  uint32_t p = lc_load(parent + x);
  while (p != x) {  // p < x: strictly downward
    x = p;
    p = lc_load(parent + x);
  }
  return x;
}
// lc_find that halves the path it walks: a node that is not a root (it never becomes one again; only roots are hooked) is pointed at its
// grandparent - a lower index of the same set, so parent[x] <= x holds and whichever of two such stores lands last is a valid one
DEV uint32_t lc_find_halving(uint32_t* parent, uint32_t x) {
  uint32_t p = lc_load(parent + x);
  while (p != x) {
    const uint32_t g = lc_load(parent + p);
    if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
    p = g;
  }
  return x;
}
DEV void lc_unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {  // one more round only after an exchange that another lane's hook made fail
    a = lc_find_halving(parent, a);
    b = lc_find_halving(parent, b);
    if (a == b) return;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    if (atomicCAS(parent + hi, hi, lo) == hi) return;
  }
}

// ---- the dilation ----
// The chart a texel joins: c[k] the chart of neighbour k, mask its covered neighbours (not empty). Returns the chart and, in `same`, the mask of
// the covered neighbours that hold it.
DEV uint32_t lc_vote(const uint32_t c[8], uint32_t mask, uint32_t& same) {
  uint32_t best = SOL_LC_NONE, best_n = 0u, best_mask = 0u;
#pragma unroll
  for (uint32_t k = 0; k < 8u; ++k) {
    if (!(mask & (1u << k))) continue;
    uint32_t m = 0u;
#pragma unroll
    for (uint32_t q = 0; q < 8u; ++q)
      if ((mask & (1u << q)) && c[q] == c[k]) m |= 1u << q;
    const uint32_t n = (uint32_t)__builtin_popcount(m);
    if (n > best_n || (n == best_n && c[k] < best)) {
      best = c[k];
      best_n = n;
      best_mask = m;
    }
  }
  same = best_mask;
  return best;
}

// ---- the levels ----
// one more source word `s` (NONE: not live) into the reduction `acc` of a level texel
DEV uint32_t lc_merge(uint32_t acc, uint32_t s) {
  if (s == SOL_LC_NONE) return acc;
  if (acc == SOL_LC_NONE) return s;
  return (acc == s && s != SOL_LC_MIXED) ? acc : SOL_LC_MIXED;
}
