// sol_scene.h -- the handle behind the C ABI (include/solstrale_hip.h) and what the translation units of libsolstrale_hip.so
// share: error reporting, the developer overrides (environment variables, parsed in ONE place), the device memory of a scene - owned, all of
// it, by DevPtr (an array made once), DevBuf (an array that grows on demand: reserve) and PinnedPtr members that free themselves with their
// owner -, the device copy of the scene record (SolSceneMirror) and the launch plan of the persistent kernels (sol_launch_plan).
//   sol_api.cpp     handle life cycle, options, partition, accumulators, read-back, statistics
//   sol_create.cpp  sol_scene_create in stages: validation of the flattened scene, conversion to the fp32 device layout (sol_types.h), world-tree candidates, upload, probes; the tree diagnostics
//   sol_launch.cpp  sol_render* / auxiliary planes / debug hooks: launches of the kernels in sol_render.hip; sol_launch_plan (grid and spill tail)
//   sol_launch_ab.cpp  (A/B build only, beside sol_wavefront.hip and sol_pool.hip) sol_render_ab: the launches of the measured-and-rejected kernel variants
//   sol_launch.h    the launch wrappers of the .hip files (each family: one variant table for the launch and the occupancy query; sol_blocks_per_cu)
//   sol_camera.cpp  sol_scene_set_camera: a new camera for a live scene, its background blocks re-proved on the device (sol_camera.hip)
//   sol_geometry.cpp sol_scene_set_triangles / sol_scene_set_primitives: the triangles, spheres and quads of a live scene moved, records and tree boxes recomputed on the device (sol_geometry.hip)
//   sol_lightmap.cpp sol_lightmap_points / sol_lightmap_dilate: lightmap UVs rasterised into gather points, chart borders dilated (sol_lightmap.hip)
//   sol_lightmap_filter.cpp sol_lightmap_filter: chart-aware a-trous filtering of a baked atlas (sol_lightmap_filter.hip)
//   sol_lightmap_filter_var.cpp sol_lightmap_filter_var: the same under the guidance of the per-texel variance sol_irradiance_moments gathers (sol_lightmap_filter_var.hip)
//   sol_gather.h/.cpp what the radiance queries and the gather families share: configuration checks, entry shape, slice / window launch plan, staged host route
//   sol_stage.h / sol_bake_checks.h what the bake families (lightmaps, volumes, depth moments) share: the staged host route (SolStaged) and the sentences of their refusals
//   sol_gather_adaptive.cpp sol_irradiance_adaptive / sol_radiance_rescale: rounds of an irradiance-moments gather over the points still active (sol_gather_adaptive.hip)
//   sol_volume.cpp  sol_volume_points / sol_volume_build / sol_volume_sample: a probe grid laid out, packed and sampled (sol_volume.hip)
//   sol_post.cpp    un-permute, Nop tone-map, bloom (kernels in sol_aux.hip)
//   sol_comm.cpp    RCCL communicator and the gather to rank 0
// There is NO CPU fallback: without a HIP device every compute entry point fails with SOL_EDEVICE.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/solstrale_hip.h"
#include "sol_launch.h"
#include "sol_types.h"

// Sets the thread's error string (sol_last_error) and returns `code`.
int sol_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
#define HIP_TRY(expr)                                                                           \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess) return sol_fail(SOL_EDEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

struct SolHipFree { void operator()(void* p) const { hipFree(p); } };
template <typename T> using DevPtr = std::unique_ptr<T, SolHipFree>;  // an owned device array: freed with its owner, empty after a move
// `dev` <- n uninitialised elements (at least 64 bytes: never a null device pointer), or empty when the allocation fails. The callers name the error.
template <typename T> hipError_t sol_dev_alloc(DevPtr<T>& dev, size_t n) {
  T* p = nullptr;
  const hipError_t e = hipMalloc((void**)&p, std::max<size_t>(n * sizeof(T), 64));
  dev.reset(e == hipSuccess ? p : nullptr);
  return e;
}
// `dev` <- a copy of `host`, the rest of the allocation zero
template <typename T>
int sol_upload(const std::vector<T>& host, DevPtr<T>& dev) {
  HIP_TRY(sol_dev_alloc(dev, host.size()));
  HIP_TRY(hipMemset(dev.get(), 0, std::max<size_t>(host.size() * sizeof(T), 64)));
  if (!host.empty()) HIP_TRY(hipMemcpy(dev.get(), host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
  return SOL_OK;
}
struct SolHipHostFree { void operator()(void* p) const { hipHostFree(p); } };
template <typename T> using PinnedPtr = std::unique_ptr<T, SolHipHostFree>;  // an owned array of pinned host memory
template <typename T> hipError_t sol_pinned_alloc(PinnedPtr<T>& host, size_t n) {
  T* p = nullptr;
  const hipError_t e = hipHostMalloc((void**)&p, n * sizeof(T), hipHostMallocDefault);
  host.reset(e == hipSuccess ? p : nullptr);
  return e;
}

// An owned device array that grows on demand, with its capacity in elements: every scratch buffer and table of a handle whose size follows the
// calls (DevPtr: the arrays whose size is fixed when they are made). Freed with its owner.
template <typename T>
class DevBuf {
 public:
  T* get() const { return p_.get(); }
  size_t capacity() const { return cap_; }
  explicit operator bool() const { return (bool)p_; }
  void reset() { p_.reset(); cap_ = 0; }
  // Room for n elements; the contents are NOT kept and NOT zeroed. Nothing happens while the buffer exists and holds n already (no
  // synchronisation, no allocation: the steady state of every launch path). Otherwise launches queued on `stream` may still use the old array:
  // the stream is drained, the array freed and a new one allocated - never a null pointer, also for n = 0. The capacity is recorded after the
  // allocation succeeded; after a failure the buffer is empty with capacity 0, so the next call allocates again instead of trusting a stale size.
  int reserve(hipStream_t stream, size_t n) {
    if (p_ && cap_ >= n) return SOL_OK;
    HIP_TRY(hipStreamSynchronize(stream));
    reset();
    HIP_TRY(sol_dev_alloc(p_, n));
    cap_ = n;
    return SOL_OK;
  }
 private:
  DevPtr<T> p_;
  size_t cap_ = 0;
};
// The device copy of a scene record, which the kernels read through a pointer: the copy, the host image last uploaded and whether there is one.
struct SolSceneMirror {
  DevPtr<DevScene> dev; DevScene uploaded{}; bool valid = false;
  // dev holds S afterwards. Uploaded only when S differs from the copy on the device (rare: scene creation, a tree probe, an auxiliary render in
  // between, a round of adaptive sampling whose active list has a new heavy prefix): launches already queued may still read the old copy.
  int upload(hipStream_t stream, const DevScene& S) {
    if (!dev) HIP_TRY(sol_dev_alloc(dev, 1));
    if (!valid || std::memcmp(&S, &uploaded, sizeof(DevScene)) != 0) {
      HIP_TRY(hipStreamSynchronize(stream));
      HIP_TRY(hipMemcpy(dev.get(), &S, sizeof(DevScene), hipMemcpyHostToDevice));
      std::memcpy(&uploaded, &S, sizeof(DevScene));
      valid = true;
    }
    return SOL_OK;
  }
};
#define SOL_MAX_ITEMS 0xFF000000ull
// SOL_EDEVICE "no HIP device available" unless there is one (sol_api.cpp); *n_devices: how many.
int sol_device_check(int* n_devices = nullptr);

// Developer overrides: environment variables for experiments and A/B runs, parsed by sol_dev_overrides() - the
// only getenv site of the library - once per sol_scene_create / sol_world_tree_check; nothing on the launch path reads the environment.
struct SolDevOverrides {
  int kernel_version = 0;        // SOL_KERNEL=v1|v2|v3 (v2 / v3 exist in -DSOL_AB_KERNELS builds only)
  std::string bvh;               // SOL_BVH=device|host|ref|sah|sah8|sah16|sah64 ("" = SolCreateOptions.world_tree)
  bool greedy_collapse = false;  // SOL_COLLAPSE=greedy
  bool octant_slots = false;     // SOL_SLOTS=octant
  double node_cost = 2.5;        // SOL_NODE_COST
  std::vector<int> sah_bins;     // SOL_SAH_LIST=4,12,.. (empty: 8, 16, 64)
  int ploc_radius = 0;           // SOL_PLOC_R (0: the builder's default)
  int split_percent = -1;        // SOL_SPLIT: pre-split budget of the device build in percent of the primitive count (0 off; -1: not set)
  int split_slack = -1;          // SOL_SPLIT_SLACK: levels below the one-primitive cells a plane must lie to be worth a split (-1: not set)
  int background_blocks = -1;    // SOL_BACKGROUND_BLOCKS: 0 = do not look for background blocks (-1: not set)
  int split_keep = -1;           // SOL_SPLIT_KEEP: keep the splits when the summed box area falls below this percentage (-1: not set)
  int reinsert_rounds = -1;      // SOL_REINSERT: reinsertion rounds of the device build (0 off; -1: not set)
  int reinsert_stride = 0;       // SOL_REINSERT_STRIDE: every n-th node searches per round (0: not set)
  int order_mode = 2;            // SOL_ORDER: 0 no work-order probe, 1 heavy blocks first only, 2 + cost classes
  int switch_below = -1;         // SOL_SWITCH (-1: default)
  int max_bpc = -1;              // SOL_MAX_BPC
  int fine_tail = -2;            // SOL_FINE_TAIL (-2: not set)
  int probe_radii = -1;          // SOL_PROBE_RADII (AUTO device build: 1 = emit and probe both clustering radii, 0 = never, -1 = by the collapse costs)
  int radiance_rows = 0;         // SOL_RADIANCE_ROWS: bound of the radiance queries' partial buffer in rows (0: the default, 2^24) - tests drive the splits with a small one
  int gather_rows = 0;           // SOL_GATHER_ROWS: bound of the adaptive gathers' compact buffers in rows (0: the default, 2^22) - a test forces the split over points with a small one
  int pool_swap_min = 0;         // SOL_POOL_SWAP (pool kernel: RenderParams::swap_min; 0: the default)
  bool pool_count = false;       // SOL_POOL_COUNT (pool kernel: counted renders run its instrumented build - phase statistics)
  int pool_slots = 0, wf_slots = 0, wf_min_items = -1;  // SOL_POOL_SLOTS / SOL_WF_SLOTS / SOL_WF_MIN_ITEMS (v2 / v3)
  std::string rccl_lib;          // SOL_RCCL_LIB: the communication library to dlopen instead of librccl.so.1 (tests)
  int lightmap_claim = 0;        // SOL_LIGHTMAP_CLAIM=lane|wave: the claim pass of sol_lightmap_points as one of its two plain candidates (1, 2; 0: the product's hybrid)
  bool depth_project_plain = false;  // SOL_DEPTH_PROJECT=plain: sol_visibility_oct projects with a thread per (point, texel) that draws every direction itself (the measured alternative; the same words)
  bool volume_load_all = false;  // SOL_VOLUME_SAMPLE=loadall: sol_volume_sample fetches the zero-weight corners of a cell too (the measured alternative; the same words)
  int lightmap_filter = 0;       // SOL_LIGHTMAP_FILTER=plain|staged|fold: the pass kernel of sol_lightmap_filter as one of its measured shapes (1, 2, 3: plain with every channel group in one lane; 0: the product's, staged; the same words)
  bool verbose = false;          // SOL_VERBOSE
};
SolDevOverrides sol_dev_overrides();

// Device memory that depends on the choice of the world tree (sol_scene_create probes several candidates): the 7-wide tree, the
// primitive arrays in that tree's leaf order and every table holding references into them.
struct DevTree {
  DevPtr<DWide> wides; DevPtr<uint32_t> leaf_refs; DevPtr<DTri> tris; DevPtr<DTriShade> tri_shade; DevPtr<DQuad> quads;
  DevPtr<DSphere> spheres; DevPtr<DNode> nodes; DevPtr<DMedium> mediums; DevPtr<uint32_t> lights;
  uint32_t emin = 1, depth = 0, root = 0, light0 = 0;  // depth: dwords of traversal stack a search can use (SolSceneInfo::stack_bound)
  uint32_t n_wide = 0, packed_depth = 0;  // wide nodes; stack bound with one-dword node groups (the pool kernel, sol_pool.hip)
  std::vector<uint32_t> old_index[3];  // triangles / spheres / quads: device index -> index in the caller's SolSceneDesc arrays
  void release() { *this = DevTree{}; }
};

// What a handle created with SolCreateOptions.dynamic_triangles keeps for sol_scene_set_triangles (sol_geometry.cpp); empty otherwise.
struct SolTriStatic { float uv[6]; int32_t material; uint32_t dfs_index; };  // per caller triangle: what a move does not change (uv0, uv1, uv2 in the reference's order)
static_assert(sizeof(SolTriStatic) == 32, "SolTriStatic");
#define SOL_DYN_OUTSIDE 0x80000000u  // rec_tri / rec_sphere / rec_quad: the record's primitive is not reached by the world tree (its box is no part of the root's)
struct SolPrimStatic { int32_t material; uint32_t dfs_index; };  // per caller sphere / quad: what a move does not change
struct SolDynamic {
  bool on = false;
  uint32_t n_tris = 0, n_recs = 0;       // caller triangles; device triangle records (more where pre-splitting made copies)
  uint32_t n_spheres = 0, n_quads = 0, n_leaf_refs = 0;  // lengths of the arrays the refit indexes
  float cam_S = 0.f;                     // box_pad_for's S (largest |fp32 coordinate| of the root box and the camera): the creation camera's share,
  float S_sphere = 0.f, S_quad = 0.f;    //   the spheres' and the quads' as creation or the last committed move left them,
  float S_tri = 0.f; bool needles = false;  // and (dynamic_primitives) the triangles' with the needle flag - a call combines them with the fresh shares of the kinds it moves
  DevPtr<SolTriStatic> tri_static;       // [n_tris]
  DevPtr<uint32_t> rec_tri;              // [n_recs] DevTree::old_index[0], SOL_DYN_OUTSIDE or-ed in
  DevPtr<float> tri_box;                 // [n_recs][8] the unpadded fp32 cast box of the record's triangle (xmin xmax ymin ymax zmin zmax 0 0): the records kernel writes it
  DevPtr<float> sphere_box, quad_box;    // [n][6] the same of the spheres / quads, in device order
  DevPtr<uint32_t> level_nodes;          // wide node indices, level by level (the root first)
  std::vector<uint32_t> level_off;       // level l = level_nodes[level_off[l] .. level_off[l + 1])
  DevPtr<float> node_box;                // [n_wide][6] scratch of the refit: the union of a node's padded child boxes
  DevPtr<DWide> wides2; DevPtr<DTri> tris2; DevPtr<DTriShade> shade2;  // staging: both kernels write here, the commit swaps them with the tree's
  DevPtr<DTri> light_tri2;               // staging of SolScene::light_tri
  DevPtr<uint32_t> light_src;            // [n_lights] caller triangle of light i, 0xFFFFFFFF: not a triangle
  std::vector<uint32_t> light_src_host;
  std::vector<double> light_lum;         // [n_lights] luminance of the light's emission (sol_light_weights_of's factor)
  DevPtr<double> verts;                  // [n_tris][9] where the host route uploads the caller's vertices
  DevPtr<uint32_t> out;                  // device: 4 flag words (non-finite: bit 0 a triangle, 1 a sphere, 2 a quad; needle; the triangles' S bits; refit flags), then
                                         // n_lights f64 areas, then (dynamic_primitives) the spheres' and the quads' S bits
  // ---- SolCreateOptions.dynamic_primitives (sol_scene_set_primitives); empty otherwise ----
  bool primitives = false;
  DevPtr<SolPrimStatic> sphere_static, quad_static;  // [caller spheres] / [caller quads]
  DevPtr<uint32_t> rec_sphere, rec_quad; // [n] DevTree::old_index[1] / [2], SOL_DYN_OUTSIDE or-ed in
  DevPtr<float> tri_box2, sphere_box2, quad_box2;  // staging of the box arrays: swapped at the commit with the records of the kinds a call moved
  DevPtr<DSphere> spheres2; DevPtr<DQuad> quads2;  // staging of DevTree::spheres / quads
  DevPtr<double> sphere_rows, quad_rows; // [n][4] / [n][9] where the host route uploads the caller's rows
  DevPtr<uint32_t> light_prim;           // [n_lights] the description's reference of light i where it is a sphere or a quad, else 0
  std::vector<uint32_t> light_prim_host;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // with sol_kernel_timing: call start, vertices uploaded, records written, tree refitted, call end
  float last_ms[4] = {0.f, 0.f, 0.f, 0.f};
};

// Adaptive sampling (sol_adaptive.hip): the session opened by sol_adaptive_begin and ended by sol_clear, sol_render and
// sol_scene_set_partition. The active list has the layout of the work order: the active traced blocks at the front (the heavy ones
// first), the active background blocks at the very end of its n_local_blocks entries.
struct SolAdaptiveSession {
  bool open = false;
  uint32_t round = 0, min_samples = 0, max_samples = 0; float threshold = 0.f;
  uint32_t rounds_done = 0;                           // rounds rendered since sol_adaptive_begin
  uint32_t n_first = 0, n_traced = 0, n_background = 0;  // the active list the next round renders
  DevBuf<float> state;      // per slot of the accumulator (2 floats): Welford mean and M2 of the rounds' luminance
  DevBuf<uint32_t> active;  // per local block: 1 = still sampled
  DevBuf<uint32_t> order;   // the active list (n_local_blocks entries)
  DevBuf<uint32_t> counts;  // per image block (row-major): samples its pixels hold
  DevBuf<uint32_t> ctr; PinnedPtr<uint32_t> ctr_host;  // what the compaction counted: heavy, traced, background active blocks
  SolSceneMirror mirror;    // the DevScene copy whose work order is the active list
};

struct SolScene {
  int device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  // S changes only where the scene changes: creation, the setters (sol_scene_set_*), the partition / order tables and the sampling modes. It never changes to describe a launch: a launch that renders something else renders a copy (SolRenderJob::view).
  DevScene S{};
  SolSceneMirror mirror;               // device copy of S (the product render kernel and the queries read it through a pointer)
  DevTree tree;                        // the world tree the handle walks and what hangs on it; S points into it
  std::string tree_name;               // which world tree the handle walks ("ref", "sah8", .., "device")
  std::string tree_note;               // why it is not the one asked for (AUTO: the device build failed), else empty
  uint32_t split_references = 0, split_triangles = 0;  // device build: what triangle pre-splitting added
  float split_area_ratio = 1.f;
  uint32_t reinsertion_moves = 0; float reinsertion_area_ratio = 1.f;  // device build: sub-trees moved; summed inner-node area after / before
  // Device memory. Every allocation of the handle is owned by a DevPtr (made once) or a DevBuf (grows on demand) here, in `tree`, `dyn` or
  // `adaptive`, and is freed with the handle (sol_scene_destroy); S and every other raw pointer are views into them.
  DevPtr<DMat> mats; DevPtr<DTex> texs; DevPtr<uint8_t> texels; DevPtr<float> env; DevPtr<DTri> light_tri;
  DevBuf<float> acc_own; float* acc = nullptr; size_t acc_floats = 0;  // acc: acc_own or the caller's bound memory; acc_floats: the size the partition gives it
  DevBuf<float> aux[2]; size_t aux_floats = 0;  // albedo / normal accumulators (sol_render_aux), same layout as acc; aux_floats: the acc_floats they were cleared for
  uint32_t aux_samples = 0;                 // samples sol_render_aux added since the planes were last cleared (sol_resolve_aux)
  DevBuf<float> aux_img[2];                 // row-major albedo / normal planes of sol_resolve_aux (W*H*3 floats each)
  DevBuf<float4> den_buf;                   // sol_denoise scratch (sol_denoise.hip): 4 float4 per pixel
  std::vector<uint32_t> block_cost;  // per 8x8 block (global index): rays of its longest item in the cost probe; empty: no ordering
  std::vector<uint32_t> block_work;  // per 8x8 block (global index): its rays in the cost probe (balanced partition)
  bool balanced = false;             // SOL_OPT_BALANCED_PARTITION
  uint32_t partition_table = 0, partition_crc = 0;  // the partition in force: 1 = the balanced table (0: b % world), checksum of block -> slot
  std::vector<uint32_t> local_blocks;  // balanced partition: image block of every local block of this rank (empty: b = lb * world + rank)
  DevBuf<uint32_t> block_of_local_dev;
  DevBuf<uint32_t> slot_of_block;      // balanced partition (device, all blocks): owner * blocks-per-buffer + local block; empty: modulo
  DevBuf<uint32_t> order_dev;          // DevScene::block_order of the current partition
  DevBuf<float> partial;
  int fine_tail = -1;                // SOL_OPT_FINE_TAIL / SOL_FINE_TAIL: quarters of a whole item per resident lane that the end of a launch hands
                                     // out sample by sample; 0: none; -1: by the creation probe's node visits per sample (fine_tail_auto)
  int fine_tail_auto = 0;
  DevPtr<float> image;  // W*H*3 scratch for sol_read / sol_resolve_image
  DevPtr<uint8_t> rgb8;
  DevBuf<double> bloom_a, bloom_b, bloom_w;  // sol_bloom scratch
  DevPtr<uint32_t> work; DevBuf<uint32_t> spill;  // the render launch's work counter and the spill tail of its grid (sol_launch_plan)
  DevPtr<DevCounters> counters;
  SolStats stats{};
  SolPathStats path_stats{};
  bool has_medium = false;
  bool strict_triangles = false;  // the scene has needle triangles: the STRICT kernel variants (sol_render.hip)
  uint32_t pool_swap_min = 0;             // SOL_POOL_SWAP (pool kernel, RenderParams::swap_min; 0: the default)
  bool pool_count = false;                // SOL_POOL_COUNT (pool kernel: its counted renders run the instrumented build)
  int rank = 0, world = 1;
  uint32_t blocks_x = 0, blocks_y = 0, n_local_blocks = 0;
  int n_cu = 0;
  int kernel_version = 0;          // 0 auto; SOL_KERNEL=v1|v2|v3 forces one (A/B comparisons)
  DevBuf<char> pool;               // path-slot pool of the wavefront kernels
  uint32_t pool_slots_override = 0;  // SOL_POOL_SLOTS (v2: slots per wave)
  uint32_t switch_below = 0;         // SOL_SWITCH (v1, RenderParams::switch_below)
  DevBuf<uint2> queue;               // v3 ray queue: one reservoir per 64 pool slots
  DevBuf<uint32_t> wf_ctr; PinnedPtr<uint32_t> wf_ctr_host;
  uint32_t wf_slots = 4u << 20;       // SOL_WF_SLOTS: pool size of the two-kernel wavefront
  uint32_t wf_min_items = 2u << 20;   // SOL_WF_MIN_ITEMS: jobs below this use the single-launch kernel
  double build_times[4] = {0., 0., 0., 0.};  // sol_scene_build_times
  bool order_enabled = true;         // SOL_OPT_WORK_ORDER
  // background blocks (solstrale_hip.h SolSceneInfo::background_blocks): per 8x8 block (global index) 1 = proved to see only the
  // background; n_background_local: how many of them this rank owns - the LAST so many entries of the work order
  std::vector<uint8_t> background_block;
  uint32_t n_background = 0, n_background_local = 0, background_pixels = 0;
  // what sol_scene_set_camera (sol_camera.cpp) must remember of the creation: the fp32 box pad (the proof's margin is 64 of
  // them), whether creation looked for background blocks (no environment map, not switched off) and ran the cost probe, SOL_VERBOSE; and
  // the device flags its proof kernel writes (one byte per block; allocated by the first move, kept)
  float box_pad = 0.f;
  bool background_proof = false, cost_probe = false, verbose = false;
  DevBuf<uint8_t> proof_flags;
  bool background_enabled = true;    // SOL_OPT_BACKGROUND_BLOCKS
  bool background_in_counted = false;  // (value 2) counted renders skip them too: the counters of exactly what a plain render does
  int order_mode = 2;                // (SOL_ORDER) 1: heavy blocks first only; 2: + cost classes within a chunk
  int max_bpc = 0;                   // SOL_OPT_MAX_BLOCKS_PER_CU (0 = what the occupancy query allows)
  // multi-GPU (sol_comm_init): RCCL communicator of the tile partition and rank 0's receive buffer
  void* comm = nullptr; DevBuf<float> gathered;
  bool timing = false;  // sol_kernel_timing: HIP events around the render kernel on its own stream
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  uint32_t timed_launches = 0, last_grid = 0;
  SolAdaptiveSession adaptive;
  // Environment importance sampling (sol_envmap.hip). env_refusal: why sol_env_sampling refuses this scene ("": it may turn it on),
  // decided at creation from the description (sol_env_refusal); env_tables: one allocation - marginal CDF (H'), conditional CDFs (H' x W'),
  // row totals (H'), total (1) - built on first use and kept; env_is: renders of the path-tracing shader run the ENV kernels.
  std::string env_refusal;
  DevPtr<float> env_tables;
  float env_total = 0.f;
  bool env_is = false;
  // Light tree and power-weighted light sampling (sol_lights.hip). light_w: the f64 weights (area x luminance) of the
  // description's lights, decided at creation; light_tree: the tree (built on first use of mode 1 or 2), light_tables: q then the CDF
  // (mode 2, first use); light_mode: 0 uniform, 1 tree, 2 power - modes 1 and 2 run the LT kernels.
  std::vector<double> light_w;
  double light_total = 0.0;
  DevPtr<float> light_tree;
  size_t light_tree_bytes = 0;
  DevPtr<float> light_tables;
  uint32_t light_mode = 0;
  // Ray queries (sol_query.hip): the handle's staging buffers of the host route (rays in, answers out; query_cap rays each) and
  // the spill area of the query kernel's own grid. None of them is the render launch's.
  DevBuf<SolRay> query_in; DevBuf<SolRayHit> query_out;
  DevBuf<uint32_t> query_spill;
  // Radiance queries (sol_radiance.hip) and every gather family built on them (sol_gather.h): their own work counter, partial buffer
  // (rows of 16 bytes, grown on demand up to the bound), spill tail and host-route staging (rays or points, keys, answers). None of them is the
  // render launch's. rad_partial has two uses. Chunk sums (radiance, irradiance; visibility): one row - visibility: two - per (chunk, point).
  // Per sample (SH, moments; depth): one row - depth: a word, four to a row - per (sample, point), under the same bound counted in those values
  // but never below one group of 64 points over one chunk. rad_out holds whole rows per staged point: 1, 7 (SolSh9), 2 (SolMoments, SolVisibility)
  // or res x res (SolOctTexel).
  DevBuf<uint32_t> rad_work;
  DevBuf<SolRadiance> rad_partial;
  size_t rad_partial_max_rows = (size_t)1 << 24;  // the bound: 256 MiB of chunk sums (SOL_RADIANCE_ROWS)
  DevBuf<uint32_t> rad_spill;
  DevBuf<SolRay> rad_in; DevBuf<SolRayKey> rad_keys; DevBuf<SolRadiance> rad_out;
  // Lightmap texel points and dilation (sol_lightmap.hip). lm_owner: the scratch - 16 words of list counters, the W x H owner words
  // of the claim pass, then its two work lists of n_triangles words each; a dilation keeps its two coverage planes (a byte per texel each) in the
  // same words. lm_stage: what the host routes of every lightmap family stage, inputs and outputs, laid out by SolStaged (sol_stage.h);
  // sol_radiance_rescale batches through it too. lm_small_max / lm_tiles_max: the claim pass's thresholds (SOL_LIGHTMAP_CLAIM).
  DevBuf<uint32_t> lm_owner;
  DevBuf<char> lm_stage;
  uint32_t lm_small_max = 16, lm_tiles_max = 64;
  // Lightmap filtering (sol_lightmap_filter.hip). lf_guide: the packed guide plane, two dwordx4 per texel; lf_planes: the two ping-pong
  // value planes, ceil(channels / 4) dwordx4 per texel each; the host route stages through lm_stage. lf_staged / lf_fold: the pass shape
  // (SOL_LIGHTMAP_FILTER; the product's is staged - steps 1 and 2 from a tile in LDS -, a lane per (texel, channel group): the faster one at
  // 1024^2 and 4096^2, profiles/lightmap_filter.txt). The variance-guided filter (sol_lightmap_filter_var.hip) shares both buffers -
  // lf_planes then holds two sides of a mean plane and a variance plane, four dwordx4 per texel - and lf_staged; either call writes what it reads of
  // them first.
  DevBuf<float4> lf_guide, lf_planes;
  bool lf_staged = true, lf_fold = false;
  // Irradiance volumes (sol_volume.hip). vol_stage: what the host routes stage, inputs and outputs, laid out by SolStaged
  // (sol_stage.h; sol_volume_points: its one array). vol_load_all: the sampler's measured alternative (SOL_VOLUME_SAMPLE=loadall).
  DevBuf<char> vol_stage;
  bool vol_load_all = false;
  // Directional distance moments (sol_depth.hip): the gather runs through rad_*, build and sample stage through vol_stage.
  // depth_project_plain: the projection kernel's measured alternative (SOL_DEPTH_PROJECT=plain).
  bool depth_project_plain = false;
  // Adaptive irradiance gathers (sol_gather_adaptive.hip). The rounds run through the irradiance queries' buffers above; these are
  // the compaction's own, grown on demand to min(n, ga_max_rows) rows - beyond that bound (SOL_GATHER_ROWS) a call is split over points. ga_points,
  // ga_keys, ga_totals: the compact rows a later round runs over; ga_index: two active lists (this round's, the next one's); ga_scan: per wave of
  // 64 rows two ballot words, then per workgroup of 256 a count and an offset; ga_ctr / ga_ctr_host: rows that go on, rows without samples,
  // converged, capped - what the host reads back once per round.
  DevBuf<SolRay> ga_points; DevBuf<SolRayKey> ga_keys; DevBuf<SolMoments> ga_totals;
  DevBuf<uint32_t> ga_index, ga_scan, ga_ctr; PinnedPtr<uint32_t> ga_ctr_host;
  size_t ga_max_rows = (size_t)1 << 22;
  SolDynamic dyn;  // sol_scene_set_triangles / sol_scene_set_primitives (sol_geometry.cpp)
};
// The tail of an entry point's preamble, behind its refusals: the device looked for, then the handle's made current - the first read of the handle.
inline int sol_device_enter(const SolScene* s) {
  if (const int rc = sol_device_check()) return rc;
  HIP_TRY(hipSetDevice(s->device));
  return SOL_OK;
}
// The f64 weights w_i = area_i x Y_i of the lights of `d` in list order (sol_lights.hip; host only; sol_light_weights).
std::vector<double> sol_light_weights_of(const SolSceneDesc* d);
// Why environment importance sampling cannot run on the scene `d` describes, or "" (sol_envmap.hip; host only).
std::string sol_env_refusal(const SolSceneDesc* d);

// The luminance factor of sol_light_weights_of per light (w_i = area_i x luminance_i), and, after a geometry move changed s->light_w and the
// light records: the light tree and the power tables that exist are freed and built again (sol_lights.hip).
std::vector<double> sol_light_luminances_of(const SolSceneDesc* d);
int sol_light_rebuild(SolScene* s);
// What sol_scene_set_camera and sol_scene_set_triangles end with (sol_camera.cpp): the sums and the auxiliary planes cleared, an adaptive session
// ended, the background blocks proved again on the device (unless flags & 1), the cost probe (flags & 2), the work order, the scene record uploaded.
int sol_rederive_view_tables(SolScene* s, uint32_t flags, const char* who);
int sol_rebuild_order(SolScene* s);
// The 4-spp cost probe of the whole frame (sol_create.cpp): the counted render, then its adoption (`rc`: the render's status; frees the tables).
struct SolCostProbe { DevPtr<uint32_t> cost_dev, work_dev; };
int sol_cost_probe_render(SolScene* s, SolCostProbe& p);
int sol_cost_probe_adopt(SolScene* s, SolCostProbe& p, int rc, bool verbose);
inline int sol_scene_to_device(SolScene* s) { return s->mirror.upload(s->stream, s->S); }  // s->mirror.dev holds s->S
// The launch plan of the render, query and radiance launches (sol_launch.cpp): *grid = n_cu x blocks_per_cu (the occupancy of the chosen kernel,
// clamped by SOL_OPT_MAX_BLOCKS_PER_CU), at least 1 and at most the blocks `items` need; `spill` holds the spill tail of that grid afterwards -
// grid x SOL_WG x (stack_need - lds_depth) words, 16 when the searches fit the kernel's LDS stack.
int sol_launch_plan(SolScene* s, int blocks_per_cu, uint64_t items, uint32_t lds_depth, uint32_t stack_need, DevBuf<uint32_t>& spill, uint32_t* grid);
int sol_set_partition(SolScene* s, int rank, int world);
// What every volume call refuses about the scene pointer and the grid, in the header's order (sol_volume.cpp; sol_depth.cpp shares it).
int sol_volume_grid_check(bool have_scene, const char* fn, const SolVolumeGrid* g);

// One launch of sol_render_impl (sol_launch.cpp): what differs between its callers, and nothing else - the handle supplies what is not per launch
// (partition, scratch buffers, options, stream, timing events). sol_render_job is the job with every default: the handle's own scene record,
// device copy and accumulator.
struct SolRenderJob {
  uint32_t first, n; uint64_t seed;  // the sample range and the seed
  bool count;                        // a counted render (statistics, the creation probes)
  float* acc;                        // the accumulator the sums go to
  DevScene view;                     // the scene record this launch renders: s->S, or a copy with another shader / background / environment
                                     // pointer (auxiliary planes), cost tables (cost probe) or work order (a round of adaptive sampling)
  SolSceneMirror* mirror;            // the device copy `view` is uploaded to
  // a round of adaptive sampling (sol_adaptive.hip): the traced and the background blocks of the active list that is the view's work order;
  // the chunk sums stay in `partial` for the caller, which adds them to the accumulator itself
  bool round = false; uint32_t n_traced = 0, n_background = 0;
};
inline SolRenderJob sol_render_job(SolScene* s, uint32_t first, uint32_t n, uint64_t seed, bool count) { return {first, n, seed, count, s->acc, s->S, &s->mirror}; }
int sol_render_impl(SolScene* s, const SolRenderJob& job);
inline int sol_render_probe(SolScene* s) { return sol_render_impl(s, sol_render_job(s, 0, SOL_CHUNK, 0x50B3ull, true)); }

// The estimator a path-tracing launch of `view` runs now: environment importance sampling and light sampling modes 1 and 2
//  are the ENV / LT builds of the render and radiance kernels - uncounted, under the path-tracing shader only (the other shaders
// read only the scatter's colour; counted renders are the creation probes, sol_render_counted refuses while either is on). With one light modes 1
// and 2 are mode 0's estimator (q_0 = 1), and the default kernels run.
struct SolEstimator { bool env, lt; };
inline SolEstimator sol_estimator(const SolScene* s, const DevScene& view, bool count) {
  const bool path_tracing = !count && view.shader == SOL_SHADER_PATH_TRACING;
  return {s->env_is && path_tracing, s->light_mode != 0u && path_tracing && view.n_lights > 1u};
}
// How many blocks at the end of this rank's work order (`view`'s) are filled by sol_fill_background_kernel rather than traced.
inline uint32_t sol_background_tail(const SolScene* s, const DevScene& view) {
  return s->background_enabled && view.block_order && s->n_background_local <= s->n_local_blocks ? s->n_background_local : 0u;
}

// The steps of a render launch that the product path (sol_render_impl) and the A/B variants (sol_render_ab) share, in the order of a launch:
// the base launch parameters of `job` with n_traced blocks traced (refuses more work items than the 32-bit work counter takes); room for the chunk
// sums and stage_floats of staging in s->partial, the padding pixels zero; work counter and counters zeroed, the timing started; and behind the
// kernels: timing stopped, the staged samples and - unless the job leaves them to its caller - the chunk sums resolved, the counters read back.
int sol_render_params(const SolScene* s, const SolRenderJob& job, uint32_t n_traced, RenderParams& P);
int sol_render_partial(SolScene* s, const RenderParams& P, size_t stage_floats);
int sol_render_begin(SolScene* s, bool count);
int sol_render_end(SolScene* s, const SolRenderJob& job, const RenderParams& P, uint32_t grid, bool via_partial);
// sol_launch_ab.cpp, -DSOL_AB_KERNELS builds only: `job` on kernel variant 2, 3 or 4 (sol_wavefront.hip, sol_pool.hip)
int sol_render_ab(SolScene* s, const SolRenderJob& job, int variant);
