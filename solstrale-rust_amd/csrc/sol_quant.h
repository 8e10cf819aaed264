// sol_quant.h -- the quantisation grid of a 7-wide node on the device, written ONCE for the kernel that emits the tree (sol_build.hip, k_emit)
// and the kernels that refit it (sol_geometry.hip): a node's exponent and scale per axis, and the plane bytes of one child on one axis, which
// must CONTAIN the child's box under the device's own decode origin + q * scale (sol_trace.h). The host's own quantiser stays WideBuilder::build (sol_tree.h: its clamping of non-finite quotients differs);
// the bit fields of the node are sol_wide.h's on both sides.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// One axis of a node whose children span [lo, hi] (the two extra pads included): an inverted span becomes [0, 0]; returns the biased exponent
// of the grid step, clamped to [emin, emin + 31], and its scale 2^(e - 127). *over: the span needs an exponent above emin + 31.
__device__ __forceinline__ uint32_t sol_wide_axis_grid(float& lo, float& hi, uint32_t emin, float& scale, bool& over) {
  if (!(hi >= lo)) { lo = 0.f; hi = 0.f; }
  int e = 1;
  const float ext = hi - lo;
  if (ext > 0.f && ext < __builtin_huge_valf()) {
    int ex;
    frexpf(ext / 255.0f, &ex);
    e = min(254, max(1, ex + 127));
  }
  over = e > (int)emin + 31;
  e = max((int)emin, min((int)emin + 31, e));
  scale = __uint_as_float((uint32_t)e << 23);
  return (uint32_t)e;
}
// The plane bytes of [cl, chh] on an axis with origin lo and the grid step `scale`: floor / ceil, then the fix-ups that make them conservative
// under the device's own decode arithmetic. Returns false where that cannot be done and the box was opened fully on this axis (0 .. 255).
__device__ __forceinline__ bool sol_wide_axis_quantise(float cl, float chh, float lo, float scale, uint32_t& ql_out, uint32_t& qh_out) {
  long ql = (long)floorf((cl - lo) / scale), qh = (long)ceilf((chh - lo) / scale);
  ql = min(255L, max(0L, ql));
  qh = min(255L, max(0L, qh));
  while (ql > 0 && lo + (float)ql * scale > cl) --ql;
  while (qh < 255 && lo + (float)qh * scale < chh) ++qh;
  bool ok = true;
  if (lo + (float)ql * scale > cl || lo + (float)qh * scale < chh) { ql = 0; qh = 255; ok = false; }
  ql_out = (uint32_t)ql; qh_out = (uint32_t)qh;
  return ok;
}
