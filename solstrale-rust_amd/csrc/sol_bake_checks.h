// sol_bake_checks.h -- the refusals the bake families share (lightmaps, their filters, lookups, mips and charts; volumes): ONE function per
// sentence, each returning through sol_fail. A family's own *_check calls them in the family's own order (include/solstrale_hip.h states it per
// entry point): what is shared is the wording, not the order. All of them judge arguments alone - no device, no handle.
#pragma once
#include <cmath>
#include <cstring>

#include "sol_scene.h"

constexpr size_t SOL_BAKE_MAX_TRIANGLES = ((size_t)1 << 31) - 2;  // (sol_lightmap_charts has its own, SOL_LIGHTMAP_CHARTS_MAX_TRIANGLES)
constexpr size_t SOL_BAKE_MAX_ROWS = (size_t)1 << 31;

inline int sol_atlas_check(const char* fn, uint32_t width, uint32_t height) {
  if (width == 0 || height == 0 || width > SOL_LIGHTMAP_MAX_SIZE || height > SOL_LIGHTMAP_MAX_SIZE)
    return sol_fail(SOL_EINVAL, "%s: an atlas of %u x %u texels (1 .. %u each way)", fn, width, height, SOL_LIGHTMAP_MAX_SIZE);
  return SOL_OK;
}
// The rows of an atlas: channels, then the stride.
inline int sol_channels_check(const char* fn, uint32_t channels, uint32_t stride_bytes) {
  if (channels == 0 || channels > 32) return sol_fail(SOL_EINVAL, "%s: %u channels (1 .. 32)", fn, channels);
  if (stride_bytes % 4 != 0 || stride_bytes / 4 < channels)
    return sol_fail(SOL_EINVAL, "%s: a stride of %u bytes (a multiple of 4, at least 4 x %u channels)", fn, stride_bytes, channels);
  return SOL_OK;
}
// The head of a configuration `name`: size against sizeof - nothing else is read before it holds -, every reserved word zero, no bit of `flags`
// outside `known` (a configuration without flags passes neither).
template <typename Config>
int sol_config_head_check(const char* fn, const char* name, const Config& c, uint32_t flags = 0, uint32_t known = 0) {
  if (c.size != sizeof(Config)) return sol_fail(SOL_EINVAL, "%s: %s.size %u (expected %zu)", fn, name, c.size, sizeof(Config));
  uint32_t reserved[sizeof(c.reserved) / sizeof(uint32_t)];
  std::memcpy(reserved, &c.reserved, sizeof(reserved));
  for (uint32_t r : reserved)
    if (r) return sol_fail(SOL_EINVAL, "%s: %s.reserved must be 0", fn, name);
  if (flags & ~known) return sol_fail(SOL_EINVAL, "%s: %s.flags 0x%x: unknown bits", fn, name, flags);
  return SOL_OK;
}
// The chart guard of the lookups: the radius, then its two arrays - both or neither, and both with a finite radius.
inline int sol_chart_guard_check(const char* fn, float chart_radius, const void* vertices, const void* points) {
  if (!(chart_radius > 0.0f)) return sol_fail(SOL_EINVAL, "%s: chart_radius %g (> 0, not NaN; +inf switches the guard off)", fn, (double)chart_radius);
  if ((vertices != nullptr) != (points != nullptr))
    return sol_fail(SOL_EINVAL, "%s: vertices and points go together (the %s pointer is null)", fn, !vertices ? "vertex" : "point");
  if (std::isfinite(chart_radius) && !vertices) return sol_fail(SOL_EINVAL, "%s: a finite chart_radius needs the guard arrays (vertices and points)", fn);
  return SOL_OK;
}
inline int sol_triangles_check(const char* fn, size_t n_triangles) {
  if (n_triangles > SOL_BAKE_MAX_TRIANGLES) return sol_fail(SOL_EINVAL, "%s: %zu triangles in one call (at most 2^31 - 2)", fn, n_triangles);
  return SOL_OK;
}
// what: "rows", "hits", "points"
inline int sol_rows_check(const char* fn, size_t n, const char* what) {
  if (n > SOL_BAKE_MAX_ROWS) return sol_fail(SOL_EINVAL, "%s: %zu %s in one call (at most 2^31)", fn, n, what);
  return SOL_OK;
}
