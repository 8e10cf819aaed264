// sol_launch.h -- host-callable launch wrappers of sol_render.hip / sol_aux.hip (internal to libsolstrale_hip.so).
#pragma once
#include <hip/hip_runtime.h>

#include "sol_types.h"

// Workgroups of SOL_WG threads of `kernel` that one CU holds at a time (at least 1): what every persistent launch sizes its grid by. Each kernel
// family asks about the function its variant table (sol_render_variant, ..) names for SPILL = true: the SPILL = false builds need no more registers
// or LDS than those.
template <typename K>
int sol_blocks_per_cu(K kernel) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, SOL_WG, 0) != hipSuccess || n < 1) n = 1;
  return n;
}

// the product kernel, one path per lane. The caller (sol_render_impl) has decided the variant: strict: the scene has needle triangles; env: environment
// importance sampling, lt: light sampling modes 1 and 2 - both uncounted only
hipError_t sol_launch_render(const DevScene* dS, const RenderParams& P, float* acc, float* partial, uint32_t* work, uint32_t* spill, DevCounters* cnt,
                             uint32_t grid, bool count, bool medium, bool may_spill, bool strict, bool env, bool lt, hipStream_t stream);
int sol_render_blocks_per_cu(bool count, bool medium, bool strict, bool env, bool lt);
hipError_t sol_launch_stage_resolve(const DevScene* dS, const RenderParams& P, float* partial, hipStream_t stream);
hipError_t sol_launch_fill_background(const DevScene* dS, const RenderParams& P, float* partial, hipStream_t stream);
hipError_t sol_launch_debug_path(const DevScene& S, const RenderParams& P, uint32_t px, uint32_t py, uint32_t s, uint32_t* spill,
                                 float* out, uint32_t max_rows, bool medium, hipStream_t stream);
// ==== the A/B kernel variants (-DSOL_AB_KERNELS builds only): launched from sol_launch_ab.cpp, nowhere else ====
// ---- sol_pool.hip: version 4, the pool kernel (a second path context per lane in LDS, handed out wave-wide; sample-granular work items) ----
hipError_t sol_launch_pool4(const DevScene& S, const DevScene* dS, const RenderParams& P, float* partial, uint32_t* work, uint32_t* spill, uint32_t grid,
                            bool medium, bool may_spill, DevCounters* cnt, hipStream_t stream);
int sol_pool4_blocks_per_cu(bool medium, bool strict);
int sol_pool4_lds_stack_depth();
// ---- sol_wavefront.hip ----
// version 2: wave-private wavefront over a pool of path slots
hipError_t sol_launch_pool(const DevScene& S, const RenderParams& P, float* acc, float* partial, uint32_t* work, uint32_t* spill, void* pool,
                           DevCounters* cnt, uint32_t grid, bool count, bool medium, hipStream_t stream);
int sol_pool_blocks_per_cu(bool count, bool medium);
size_t sol_pool_bytes_per_wave(uint32_t slots);
// version 3: two-kernel wavefront (one shade + one trace launch per round)
hipError_t sol_launch_wf_shade(const DevScene& S, const RenderParams& P, float* acc, float* partial, void* ctr, void* rec,
                               void* reservoir, DevCounters* cnt, bool count, hipStream_t stream);
hipError_t sol_launch_wf_trace(const DevScene& S, const RenderParams& P, void* ctr, void* rec, uint32_t* spill, DevCounters* cnt,
                               uint32_t grid, bool count, bool medium, hipStream_t stream);
int sol_wf_trace_blocks_per_cu(bool count, bool medium);
size_t sol_wf_pool_bytes(uint32_t slots);
int sol_wf_lds_stack_depth();
// ==== (end of the A/B kernel variants) ====
// ---- sol_query.hip: ray queries. rays: n SolRay on the device; out: n SolRayHit, or n status words when `any` ----
hipError_t sol_launch_query(const DevScene* dS, bool any, bool may_spill, bool strict, const void* rays, uint32_t n, void* out, uint32_t* spill,
                            uint32_t grid, hipStream_t stream);
int sol_query_blocks_per_cu(bool any, bool strict);
hipError_t sol_launch_camera_rays(const DevScene* dS, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t sample, uint64_t seed, void* rays,
                                  hipStream_t stream);
// ---- sol_radiance.hip: radiance queries. One launch: n_rays SolRay (and SolRayKey, or null) on the device, samples
// [first_sample, ..) in n_chunks chunks of SOL_CHUNK, the last one ending at end_sample. Work item = (ray, chunk), chunk-major, 64 consecutive rays per wave ----
struct RadianceParams {
  uint32_t n_rays, n_groups;   // rays of this launch; groups of 64 of them ((n_rays + 63) / 64)
  uint32_t n_chunks, n_items;  // chunks of this launch; n_chunks * n_groups * 64
  uint32_t first_sample;       // the first sample of this launch's first chunk
  uint32_t end_sample;         // one past the call's last sample (the last chunk may be short)
  uint32_t seed_lo, seed_hi;
  uint32_t key_base;           // keys == null: ray i of the launch draws from the stream of key_base + i (wrapping) ..
  uint32_t first_draw;         // .. with its counter starting here
  uint32_t switch_below;       // as RenderParams::switch_below
  uint32_t total_threads;      // grid * SOL_WG (spill stack stride)
  uint32_t direct;             // 1: the call has one chunk, the kernel writes the answers itself; 0: chunk sums into `partial` [chunk][n_groups * 64]
  uint32_t mode;               // irradiance queries (gather launches only): SOL_IRRADIANCE_COSINE or SOL_IRRADIANCE_SPHERE
};
// gather: an irradiance query - the rows are points (position, tmin, normal, tmax) and each sample draws its own direction (P.mode)
// each (with gather; SH irradiance queries): a work item is (point, sample), sample-major - n_items = n_groups * 64 * the launch's
// samples -, and every sample's colour goes to `partial` [sample - first_sample][n_groups * 64]; `out` and P.direct are not used
hipError_t sol_launch_radiance(const DevScene* dS, const RadianceParams& P, bool gather, bool each, bool may_spill, bool strict, bool env, bool lt, const void* rays,
                               const void* keys, void* out, void* partial, uint32_t* work, uint32_t* spill, uint32_t grid, hipStream_t stream);
int sol_radiance_blocks_per_cu(bool gather, bool each, bool strict, bool env, bool lt);
// one thread per point after an `each` launch: the launch's win_samples colours times the SH basis of their directions, added in chunk order onto 0
// (or, accumulate, onto what `out` holds) and written as SolSh9 rows with `samples`
hipError_t sol_launch_sh_project(const RadianceParams& P, const void* points, const void* keys, const void* partial, void* out, uint32_t win_samples, uint32_t samples,
                                 bool accumulate, hipStream_t stream);
// one thread per point of an irradiance query with one sample (P.first_sample): the ray that sample starts with and the key it goes on from
hipError_t sol_launch_irradiance_rays(const RadianceParams& P, const void* points, const void* keys, void* rays_out, void* keys_out, hipStream_t stream);
// the chunk sums of one launch added in chunk order onto 0 (or, accumulate, onto what `out` holds) and written with `samples`
hipError_t sol_launch_radiance_resolve(const RadianceParams& P, const void* rays, const void* partial, void* out, uint32_t samples, bool accumulate,
                                       hipStream_t stream);
hipError_t sol_launch_camera_ray_keys(const DevScene* dS, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t sample, uint64_t seed, void* keys,
                                      hipStream_t stream);
// ---- sol_visibility.hip: visibility gathers. One launch: RadianceParams as for a gather launch of sol_radiance.hip - n_rays points,
// work item = (point, chunk), chunk-major, handed out through `work` (zeroed by the caller) -, answered as a ray query in mode `any` answers each sample's ray.
// out: n_rays SolVisibility when P.direct, else the chunk rows go to `partial`, [chunk][n_groups * 64] rows of two dwordx4 ----
hipError_t sol_launch_visibility(const DevScene* dS, const RadianceParams& P, bool any, bool may_spill, bool strict, const void* points, const void* keys, void* out,
                                 void* partial, uint32_t* work, uint32_t* spill, uint32_t grid, hipStream_t stream);
int sol_visibility_blocks_per_cu(bool any, bool strict);
// the chunk rows of one launch added in chunk order onto 0 (or, accumulate, onto what `out` holds) and written with `samples`
hipError_t sol_launch_visibility_resolve(const RadianceParams& P, const void* points, const void* partial, void* out, uint32_t samples, bool accumulate,
                                         hipStream_t stream);
// ---- sol_lightmap.hip: lightmap texel points and border dilation. owner: W x H words, all 0xFFFFFFFF; ctr: two words, zero; list0,
// list1: n words each - all on `stream` before the launch. A claim walks a box of at most small_max texels with one lane, one of at most tiles_max 8x8
// tiles with one wave, a larger one with every wave of `persistent_blocks` blocks. points: W x H SolRay, texels: W x H SolTexel, 16-byte aligned ----
hipError_t sol_launch_lightmap_points(const float* vertices, const float* normals, const float* uvs, uint32_t n, uint32_t W, uint32_t H, bool conservative,
                                      float tmin, float tmax, uint32_t small_max, uint32_t tiles_max, uint32_t* owner, uint32_t* ctr, uint32_t* list0,
                                      uint32_t* list1, uint32_t persistent_blocks, void* points, void* texels, hipStream_t stream);
// out <- the owned rows of `values`, zero rows elsewhere; cover <- 0 (owned) or 255. Then pass k = 1, 2, ..: cover_out <- cover_in with the texels filled now
hipError_t sol_launch_lightmap_dilate_begin(const void* texels, uint32_t n_texels, const void* values, uint32_t stride_words, void* out, uint8_t* cover,
                                            hipStream_t stream);
hipError_t sol_launch_lightmap_dilate_pass(uint32_t W, uint32_t H, uint32_t channels, uint32_t stride_words, uint32_t pass, void* out, const uint8_t* cover_in,
                                           uint8_t* cover_out, hipStream_t stream);
// ---- sol_volume.hip: irradiance volumes. points: nx * ny * nz SolRay; sh: as many SolSh9, visibility: as many SolVisibility or null,
// probes: as many SolProbe; a sample reads n SolRay points and writes n SolRadiance - all 16-byte aligned. load_all: the measured alternative of the
// sampler, which fetches the zero-weight corners too (the same words) ----
struct SolVolumeGrid;
hipError_t sol_launch_volume_points(const SolVolumeGrid& grid, float tmin, float tmax, void* points, hipStream_t stream);
hipError_t sol_launch_volume_build(uint32_t n_probes, const void* sh, const void* visibility, float radius, void* probes, hipStream_t stream);
hipError_t sol_launch_volume_sample(const SolVolumeGrid& grid, bool load_all, const void* probes, const void* points, uint32_t n, void* out, hipStream_t stream);
// ---- sol_depth.hip: directional distance moments. each: RadianceParams as for an `each` launch of sol_radiance.hip - a work item is
// (point, sample), sample-major, n_items = n_groups * 64 * the launch's samples -, one word per item to `partial` [sample - first_sample][n_groups * 64].
// project: after it, the launch's win_samples words of every point added into its res x res SolOctTexel rows in chunk order onto 0 (or, accumulate,
// onto what `out` holds); plain: the measured alternative, a thread per texel. build: n_texels SolOctTexel in, as many SolDepthTexel out. ----
hipError_t sol_launch_depth_each(const DevScene* dS, const RadianceParams& P, bool may_spill, bool strict, const void* points, const void* keys, void* partial,
                                 uint32_t* work, uint32_t* spill, uint32_t grid, hipStream_t stream);
int sol_depth_each_blocks_per_cu(bool strict);
hipError_t sol_launch_depth_project(const RadianceParams& P, bool plain, uint32_t res, uint32_t sharpness, const void* points, const void* keys, const void* partial,
                                    void* out, uint32_t win_samples, bool accumulate, hipStream_t stream);
hipError_t sol_launch_depth_build(uint64_t n_texels, const void* oct, float radius, void* depth, hipStream_t stream);
hipError_t sol_launch_volume_sample_depth(const SolVolumeGrid& grid, const void* probes, const void* depth, uint32_t res, const void* points, uint32_t n, void* out,
                                          hipStream_t stream);
// ---- sol_lightmap_filter.hip: lightmap filtering. guide: 2 x W x H dwordx4; a value plane: ceil(channels / 4) x W x H dwordx4, by
// channel group. prepare: liveness judged, guides packed, the rows copied to `out` whole, the channels to `plane`. pass i: `in` -> out_plane, or,
// the last one, -> the channel words of the live rows of out_rows. staged: steps 1 and 2 read their taps from a tile in LDS (the same words);
// fold_groups: one lane adds every channel group of its texel instead of one ----
struct SolLightmapFilterConfig;
hipError_t sol_launch_lightmap_filter_prepare(const void* texels, const void* points, const void* values, uint32_t n_texels, uint32_t channels,
                                              uint32_t stride_words, void* guide, void* plane, void* out, hipStream_t stream);
hipError_t sol_launch_lightmap_filter_pass(const SolLightmapFilterConfig& c, uint32_t pass, bool staged, bool fold_groups, const void* guide, const void* in,
                                           void* out_plane, void* out_rows, hipStream_t stream);
// ---- sol_lightmap_filter_var.hip: irradiance moments and the variance-guided lightmap filter. moments_project: one thread per point
// after an `each` launch of sol_radiance.hip - the launch's win_samples colours and their squares added in chunk order onto 0 (or, accumulate, onto
// what `out` holds) and written as SolMoments rows with `samples`. The filter: guide: 2 x W x H dwordx4; a side of the ping-pong: W x H dwordx4 of
// means (x, samples) and as many of variances. prepare: liveness judged, guides packed, side 0 written, and the rows of `out` / `variance_out` (or
// null) of the texels that are not live. pass i: (in_x, in_v) -> (out_x, out_v), or, the last one, -> the live rows of out_rows / var_rows (or
// null). staged: steps 1 and 2 read their taps from a tile in LDS (the same words) ----
hipError_t sol_launch_moments_project(const RadianceParams& P, const void* points, const void* partial, void* out, uint32_t win_samples, uint32_t samples,
                                      bool accumulate, hipStream_t stream);
struct SolLightmapFilterVarConfig;
hipError_t sol_launch_lightmap_filter_var_prepare(const void* texels, const void* points, const void* moments, uint32_t n_texels, void* guide, void* plane_x,
                                                  void* plane_v, void* out, void* variance_out, hipStream_t stream);
hipError_t sol_launch_lightmap_filter_var_pass(const SolLightmapFilterVarConfig& c, uint32_t pass, bool staged, const void* guide, const void* in_x,
                                               const void* in_v, void* out_x, void* out_v, void* out_rows, void* var_rows, hipStream_t stream);
// ---- sol_gather_adaptive.hip: adaptive irradiance gathers. judge: the stop rule on the n_active SolMoments `rows` of a round - one
// 64-bit ballot per wave of 64 rows (two words each) and one count per workgroup of 256 of the rows that go on, ctr[1..3] += rows without samples,
// converged, capped -, then the scan of the counts: wg_offsets, and ctr[0] = the rows that go on. scatter: those rows, in order, to index_out and -
// their point and key by their index in the call, their sums from `totals` by that index - to the compact buffers of n_next rows. writeback:
// compact row j -> out[index[j]]. rescale: n SolRadiance rows brought to `target` samples; out may be rows ----
hipError_t sol_launch_gather_judge(const void* rows, uint32_t n_active, uint32_t max_samples, uint32_t min_samples, float threshold, float floor, uint32_t* ballots,
                                   uint32_t* wg_counts, uint32_t* wg_offsets, uint32_t* ctr, hipStream_t stream);
hipError_t sol_launch_gather_scatter(uint32_t n_active, const uint32_t* index_in, const uint32_t* ballots, const uint32_t* wg_offsets, const void* points,
                                     const void* keys, uint32_t key_base, uint32_t first_draw, const void* totals, uint32_t n_next, uint32_t* index_out,
                                     void* points_out, void* keys_out, void* totals_out, hipStream_t stream);
hipError_t sol_launch_gather_writeback(uint32_t n_active, const uint32_t* index, const void* rows, void* out, hipStream_t stream);
hipError_t sol_launch_radiance_rescale(const void* rows, size_t n, uint32_t target, void* out, hipStream_t stream);
// ---- sol_lightmap_sample.hip: lightmap lookups. coords: n SolRayHit in, n SolTexel surface rows out, table: n_dfs words. sample: n
// surface rows in, n rows of channels + 1 words out; pass_of, and vertices with points, or null; the chart guard is on when vertices and points are
// given and c.chart_radius is finite ----
hipError_t sol_launch_lightmap_coords(const void* hits, uint32_t n, const void* table, uint32_t n_dfs, void* out, hipStream_t stream);
struct SolLightmapSampleConfig;
hipError_t sol_launch_lightmap_sample(const SolLightmapSampleConfig& c, uint32_t n_triangles, const void* uvs, const void* texels, const void* pass_of,
                                      const void* values, const void* vertices, const void* points, const void* coords, uint32_t n, void* out,
                                      hipStream_t stream);
// ---- sol_lightmap_sh.hip: directional lightmaps. sh: n surface rows and n normal rows (x, y, z, unused; null in coefficient mode)
// in, n SolRadiance out - or, with SOL_LIGHTMAP_SH_COEFFICIENTS, n rows of 28 words; the atlas arguments are sol_launch_lightmap_sample's with
// rows of 27 coefficients. normals: n surface rows in, n rows (nx, ny, nz, 0) out; vertex_normals or null ----
struct SolLightmapShConfig;
hipError_t sol_launch_lightmap_sh(const SolLightmapShConfig& c, uint32_t n_triangles, const void* uvs, const void* texels, const void* pass_of,
                                  const void* values, const void* vertices, const void* points, const void* coords, const void* normals, uint32_t n,
                                  void* out, hipStream_t stream);
hipError_t sol_launch_lightmap_normals(const void* coords, uint32_t n, const void* vertices, const void* vertex_normals, uint32_t n_triangles, void* out,
                                       hipStream_t stream);
// ---- sol_lightmap_mips.hip: lightmap mip chains. The layout is the one rule of host and device: level 0 is the caller's W x H
// atlas, W_l = (W_{l-1} + 1) / 2 and H_l likewise, the chain holds levels 1 .. levels - 1 packed in this order with level 0's stride, the cover
// plane one byte per chain row ----
#define SOL_LMM_MAX_LEVELS 15u  // 16384 = 2^14: levels 0 .. 14
struct LmmLayout {
  uint32_t levels, full;  // the count in force (1 .. full); the count at which both sizes reach 1
  uint32_t w[SOL_LMM_MAX_LEVELS], h[SOL_LMM_MAX_LEVELS];
  uint64_t at[SOL_LMM_MAX_LEVELS];  // the first row of level l in the chain (at[0] = 0: level 0 is not in the chain)
  uint64_t rows;                    // the rows of the chain: levels 1 .. levels - 1
};
// levels: 0 = all; a count above the full one is clamped here - the entry points refuse it first
inline LmmLayout lmm_layout(uint32_t W, uint32_t H, uint32_t levels) {
  LmmLayout L;
  uint32_t w = W, h = H, full = 1u;
  while ((w > 1u || h > 1u) && full < SOL_LMM_MAX_LEVELS) { w = (w + 1u) / 2u; h = (h + 1u) / 2u; ++full; }
  L.full = full;
  L.levels = (levels == 0u || levels > full) ? full : levels;
  L.rows = 0;
  w = W; h = H;
  for (uint32_t l = 0; l < SOL_LMM_MAX_LEVELS; ++l) {
    L.w[l] = w; L.h[l] = h;
    L.at[l] = l >= 1u ? L.rows : 0;
    if (l >= 1u && l < L.levels) L.rows += (uint64_t)w * h;
    w = (w + 1u) / 2u; h = (h + 1u) / 2u;
  }
  return L;
}
// mips: levels 1 .. L.levels - 1 from level 0 (texels, pass_of or null, values) into `mips` and `cover`. tail: the levels from the first one whose
// source is at most 64 x 64 are made by one workgroup through LDS where the rows fit (the same words); else a launch per level.
hipError_t sol_launch_lightmap_mips(const LmmLayout& L, uint32_t channels, uint32_t stride_words, bool tail, const void* texels, const void* pass_of,
                                    const void* values, void* mips, void* cover, hipStream_t stream);
// sample_lod: sol_launch_lightmap_sample's arguments, the chain, one float of lod per row
struct SolLightmapLodConfig;
hipError_t sol_launch_lightmap_sample_lod(const SolLightmapLodConfig& c, const LmmLayout& L, uint32_t n_triangles, const void* uvs, const void* texels,
                                          const void* pass_of, const void* values, const void* mips, const void* cover, const void* vertices,
                                          const void* points, const void* coords, const void* lods, uint32_t n, void* out, hipStream_t stream);
// lod: n SolRay, n SolRayHit, n surface rows in, n floats out
hipError_t sol_launch_lightmap_lod(const void* rays, const void* hits, const void* coords, uint32_t n, const void* vertices, const void* uvs,
                                   uint32_t n_triangles, uint32_t W, uint32_t H, float spread, float bias, void* out, hipStream_t stream);
// ---- sol_lightmap_charts.hip: lightmap charts. charts: n triangles (uvs, vertices or null) labelled into chart_of (n words) and
// *n_charts; collide: the hash masked to 4 bits (the same labels). The scratch of a labelling is sized once, by the entry point, and handed to the
// launch: offsets in words of keys, keys2 (two each per edge), vals, order (one per edge), parent, root, flag, rank (one per triangle), then
// rocPRIM's own, 256-byte aligned; `words` in all, 8-byte aligned ----
struct LcScratch {
  size_t keys, keys2, vals, order, parent, root, flag, rank, tmp, words;
  size_t sort_bytes, scan_bytes;
};
hipError_t sol_lightmap_charts_scratch(uint32_t n, LcScratch& S);
hipError_t sol_launch_lightmap_charts(const void* uvs, const void* vertices, uint32_t n, bool collide, const LcScratch& S, uint32_t* scratch, void* chart_of,
                                      void* n_charts, hipStream_t stream);
// chart_ids: the tail of the labelling, which the unwrap shares - parent (a union-find over n triangles, in the scratch) flattened, the roots
// flagged and ranked; chart_of holds SOL_LC_NONE for a dead triangle going in, the dense ids coming out
hipError_t sol_launch_lightmap_chart_ids(uint32_t n, const LcScratch& S, uint32_t* scratch, void* chart_of, void* n_charts, hipStream_t stream);
// ---- sol_lightmap_unwrap.hip: the lightmap unwrap. The scratch of a call is sized once, by the entry point: a labelling's (C),
// then offsets in words of the triangles' normals and classes (four per triangle), the counters, the shelves' two tables and rocPRIM's own for
// the second sort and the prefix sum. The rectangles' arrays live in the words of C the labelling is done with (keys .. order) ----
struct LuScratch {
  LcScratch C;
  size_t nrm, misc, shelf_first, shelf_y, tmp, words;
  size_t sort_bytes, scan_bytes;
};
struct SolUnwrapConfig;
// stages: null, or SOL_LU_STAGES + 1 events recorded around the stages - normals and hash, sort, unions and ids, extents, rectangles and their
// sort, pack, write (not for n == 0)
#define SOL_LU_STAGES 7
hipError_t sol_lightmap_unwrap_scratch(uint32_t n, LuScratch& S);
hipError_t sol_launch_lightmap_unwrap(const SolUnwrapConfig& c, const void* vertices, uint32_t n, bool collide, const LuScratch& S, uint32_t* scratch,
                                      void* uvs, void* chart_of, void* result, hipStream_t stream, hipEvent_t* stages);
// dilate_charts: as the dilation's two launches, with the labels in and the chart plane beside `out`; the plane is written in place (a pass reads
// the words of texels covered before it and writes those of texels that were not)
hipError_t sol_launch_lightmap_dilate_charts_begin(const void* texels, uint32_t n_texels, const void* values, uint32_t stride_words, const void* chart_of,
                                                   uint32_t n_triangles, void* out, uint8_t* cover, void* plane, hipStream_t stream);
hipError_t sol_launch_lightmap_dilate_charts_pass(uint32_t W, uint32_t H, uint32_t channels, uint32_t stride_words, uint32_t pass, void* out,
                                                  const uint8_t* cover_in, uint8_t* cover_out, void* plane, hipStream_t stream);
// sample_charts: sol_launch_lightmap_sample's arguments without the guard arrays, the labels and the plane
hipError_t sol_launch_lightmap_sample_charts(const SolLightmapSampleConfig& c, uint32_t n_triangles, const void* uvs, const void* texels, const void* pass_of,
                                             const void* values, const void* chart_of, const void* plane, const void* coords, uint32_t n, void* out,
                                             hipStream_t stream);
// chart_levels: the plane reduced level by level into `scratch` (L.rows words, L = lmm_layout(W, H, 0)); the two count arrays (SOL_LMM_MAX_LEVELS
// words each) are zeroed here, counted into, and *levels written last
hipError_t sol_launch_lightmap_chart_levels(const LmmLayout& L, const void* plane, const void* pass_of, uint32_t* scratch, void* levels, void* mixed_texels,
                                            void* mixed_windows, hipStream_t stream);
// ---- sol_camera.hip: the background-block proof of a camera move. flags: one byte per 8x8 block, row-major ----
struct SolProofCamera;
hipError_t sol_launch_background_proof(const DWide* wides, uint32_t n_wide, uint32_t emin, const SolProofCamera& cam, uint8_t* flags, hipStream_t stream);
// ---- sol_aux.hip ----
hipError_t sol_launch_resolve(float* acc, const float* partial, uint32_t n_floats, uint32_t n_chunks, hipStream_t stream);
hipError_t sol_launch_unpermute(const float* gathered, float* image, uint32_t width, uint32_t height, uint32_t blocks_x,
                                uint32_t world, uint32_t only_rank, size_t stride, const uint32_t* slot_of_block, hipStream_t stream);
hipError_t sol_launch_tonemap(const float* image, uint8_t* rgb, uint32_t n, uint32_t spp, hipStream_t stream);
// BloomPostProcessor on a W*H*3 fp32 image; a, b: W*H*3 doubles of scratch; rgb == nullptr: result back into `image`
hipError_t sol_launch_bloom(float* image, double* a, double* b, const double* weights, uint32_t k, uint32_t width, uint32_t height,
                            double threshold, double max_intensity, uint8_t* rgb, uint32_t spp, hipStream_t stream);
hipError_t sol_launch_eval(uint32_t fn, const float* in, uint32_t n, uint32_t in_stride, float* out, uint32_t out_stride,
                           hipStream_t stream);
