// sol_create.cpp -- sol_scene_create as a sequence of stages: validation of the flattened scene, conversion to the fp32 device layout (sol_types.h),
// the world tree (built on the GPU by sol_build.hip, or host candidates - host_tree - and a probe), upload, probes; the two tree diagnostics.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <future>
#include <limits>
#include <map>
#include <memory>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "sol_build.h"
#include "sol_camera.h"
#include "sol_scene.h"
#include "sol_tree.h"
#include "sol_primitive.h"
#include "sol_triangle.h"

// The world tree built on the GPU (sol_build.hip): primitives of the reference-shaped tree under `root_ref` (each once - a
// shared sub-tree is the same geometry twice, one copy finds the same hits), pre-split, clustered and collapsed on the current device.
// With pre-splitting a triangle may have SEVERAL references, each a record of its own in the permuted triangle array (implicit leaf
// addresses want consecutive records): lay.old_of_new[0] then has more entries than the scene has triangles, several of them naming
// the same triangle, and lay.new_of_old[0] names one of a triangle's records (any: they are copies). `split_info`: the build's
// expanded references, for sol_world_tree_check.
struct DeviceSplitInfo {
  std::vector<uint32_t> tri_of_ref;  // expanded reference -> triangle
  std::vector<uint32_t> ref_of_dev;  // device triangle index -> expanded reference
  std::vector<float> ref_box;
  uint32_t split_triangles = 0;
  uint32_t extra_references = 0;
  float area_ratio = 1.f;
  uint32_t reinsertion_moves = 0;
  double area_before = 0., area_after = 0.;
};
// The world's primitives as the device builder takes them (each once, in the order of their references): collected once per scene,
// whatever the number of candidate trees.
static int collect_build_prims(const std::vector<DNode>& bin, uint32_t root_ref, const Box& root_box, std::vector<SolBuildPrim>& prims) {
  prims.clear();
  if (SOL_REF_KIND(root_ref) == SOL_REF_NODE) {
    SahBuilder col;
    if (!col.collect(bin, root_ref)) return sol_fail(SOL_EINVAL, "the world's primitives cannot be collected (non-finite box or fewer than two)");
    // in the order of their references, each once (a shared sub-tree lists its primitives twice): a counting pass per kind instead of a
    // sort - std::sort of C5's 1.09 M records was 0.08 s of sol_scene_create
    uint32_t top[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (const auto& q : col.prims) top[SOL_REF_KIND(q.ref) & 7u] = std::max(top[SOL_REF_KIND(q.ref) & 7u], SOL_REF_INDEX(q.ref) + 1u);
    std::vector<int32_t> first[8];
    for (int k = 0; k < 8; ++k) first[k].assign(top[k], -1);
    for (size_t i = 0; i < col.prims.size(); ++i) {
      int32_t& f = first[SOL_REF_KIND(col.prims[i].ref) & 7u][SOL_REF_INDEX(col.prims[i].ref)];
      if (f < 0) f = (int32_t)i;
    }
    prims.reserve(col.prims.size());
    for (int k = 0; k < 8; ++k)
      for (int32_t f : first[k]) {
        if (f < 0) continue;
        SolBuildPrim p;
        for (int j = 0; j < 6; ++j) p.box[j] = col.prims[(size_t)f].box.v[j];
        p.ref = col.prims[(size_t)f].ref; p.pad = 0;
        prims.push_back(p);
      }
  } else {
    SolBuildPrim p;
    for (int k = 0; k < 6; ++k) p.box[k] = root_box.v[k];
    p.ref = root_ref; p.pad = 0;
    prims.push_back(p);
  }
  return SOL_OK;
}
// A device build in its two halves (sol_build.h): the binary tree with its collapse cost, kept on the device behind `handle`; then the
// emission of the wide nodes and their adoption as a host-side layout record.
struct DevicePrepared {
  SolDeviceBuild* handle = nullptr;
  SolDeviceTree dt;
  uint32_t emin = 1;
  DevicePrepared() = default;
  DevicePrepared(const DevicePrepared&) = delete;
  DevicePrepared& operator=(const DevicePrepared&) = delete;
  ~DevicePrepared() { if (handle) sol_build_world_tree_release(handle); }
};
static int device_world_tree_prepare(const std::vector<SolBuildPrim>& prims, const Box& root_box, float box_pad, const uint32_t counts[3], const std::vector<DTri>& tris,
                                     const SolSplitOptions& split, int ploc_radius, hipStream_t stream, DevicePrepared& pr) {
  pr.emin = WideBuilder::exponent_min(root_box, box_pad);
  std::string err;
  const bool have_tris = tris.size() == counts[0] && counts[0] > 0;
  if (!sol_build_world_tree_prepare(prims.data(), (uint32_t)prims.size(), root_box.v, box_pad, pr.emin, counts, have_tris ? tris.data() : nullptr, split, ploc_radius, stream,
                                    pr.dt, &pr.handle, err))
    return sol_fail(SOL_EDEVICE, "%s", err.c_str());
  return SOL_OK;
}
static int device_world_tree_finish(DevicePrepared& pr, const uint32_t counts[3], const SolSplitOptions& split, WideLayout& lay, uint32_t& emin, DeviceSplitInfo* split_info) {
  const auto t_dbg0 = std::chrono::steady_clock::now();
  auto dbg = [&](const char* what) { if (split.verbose) std::fprintf(stderr, "[solstrale] device_world_tree: %s at %.1f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_dbg0).count()); };
  emin = pr.emin;
  SolDeviceTree& dt = pr.dt;
  std::string err;
  const bool emitted = sol_build_world_tree_emit(pr.handle, dt, err);
  sol_build_world_tree_release(pr.handle);
  pr.handle = nullptr;
  if (!emitted) return sol_fail(SOL_EDEVICE, "%s", err.c_str());
  dbg("device build emitted");
  const std::vector<uint32_t> extra_of = std::move(dt.extra_of);
  if (!lay.adopt_device(std::move(dt.nodes), std::move(dt.leaf_refs), dt.new_of_old, dt.depth)) return sol_fail(SOL_EDEVICE, "%s", lay.error.c_str());
  if (split_info) {
    split_info->extra_references = (uint32_t)extra_of.size();
    split_info->area_ratio = dt.split_area_ratio;
    split_info->split_triangles = dt.split_triangles;
    split_info->reinsertion_moves = dt.reinsertion_moves; split_info->area_before = dt.area_before; split_info->area_after = dt.area_after;
  }
  if (split_info && split.want_boxes) {
    split_info->ref_of_dev = lay.old_of_new[0];
    split_info->tri_of_ref.resize(counts[0] + extra_of.size());
    for (uint32_t e = 0; e < split_info->tri_of_ref.size(); ++e) split_info->tri_of_ref[e] = e < counts[0] ? e : extra_of[e - counts[0]];
    split_info->ref_box = std::move(dt.ref_box);
  }
  if (!extra_of.empty()) {  // expanded references -> triangles
    if (lay.old_of_new[0].size() != (size_t)counts[0] + extra_of.size()) return sol_fail(SOL_EDEVICE, "device tree: split references lost");
    for (uint32_t& o : lay.old_of_new[0])
      if (o >= counts[0]) {
        if (o - counts[0] >= extra_of.size() || extra_of[o - counts[0]] >= counts[0]) return sol_fail(SOL_EDEVICE, "device tree: bad split reference");
        o = extra_of[o - counts[0]];
      }
    lay.new_of_old[0].resize(counts[0]);  // (a triangle's first reference keeps the triangle's own index)
  }
  dbg("layout adopted");
  return SOL_OK;
}

// A triangle's fp32 intersect record (sol_triangle.h, shared with the records kernel of sol_scene_set_triangles): rotated, or `reference_order`.
static void cast_triangle(const SolTriangle& t, bool reference_order, DTri& o, int uv_of[3]) { sol_tri_cast(&t, reference_order, &o, uv_of); }
// the sampling frames of the triangle lights, by light index (entries of other lights stay zero)
static std::vector<DTri> light_triangle_frames(const SolSceneDesc& d) {
  std::vector<DTri> frames(std::max<uint32_t>(1u, d.n_lights), DTri{});
  int uv_of[3];
  for (uint32_t i = 0; i < d.n_lights; ++i)
    if (SOL_REF_KIND(d.lights[i]) == SOL_REF_TRIANGLE && SOL_REF_INDEX(d.lights[i]) < d.n_triangles)
      cast_triangle(d.triangles[SOL_REF_INDEX(d.lights[i])], true, frames[i], uv_of);
  return frames;
}
// the triangles' vertices as the device will hold them (what pre-splitting clips)
static std::vector<DTri> cast_triangles(const SolSceneDesc& d) {
  std::vector<DTri> tris(d.n_triangles);
  int uv_of[3];
  for (uint32_t i = 0; i < d.n_triangles; ++i) cast_triangle(d.triangles[i], false, tris[i], uv_of);
  return tris;
}
// Background blocks: the host side of the proof (sol_proof.h has the argument and the per-block function, which a camera move runs on the
// device). The walk's stack is sized from the layout's own depth: the host gives up on no tree for want of room.
static void find_background_blocks(const WideLayout& L, uint32_t emin, const DCamera& cam, uint32_t width, uint32_t height, double margin,
                                   std::vector<uint8_t>& flags, uint32_t& n_found, uint32_t& n_pixels) {
  SolProofCamera pc;
  const bool attempted = sol_proof_camera(cam, width, height, margin, pc) && !L.nodes.empty();
  flags.assign((size_t)pc.bx_n * pc.by_n, 0);
  n_found = 0; n_pixels = 0;
  if (!attempted) return;
  std::vector<uint32_t> stack(std::max(L.depth, 1u));
  for (uint32_t by = 0; by < pc.by_n; ++by)
    for (uint32_t bx = 0; bx < pc.bx_n; ++bx) {
      const bool background = pc.n_lens == 1 ? sol_block_is_background<1>(L.nodes.data(), (uint32_t)L.nodes.size(), emin, pc, bx, by, stack.data(), (uint32_t)stack.size())
                                             : sol_block_is_background<4>(L.nodes.data(), (uint32_t)L.nodes.size(), emin, pc, bx, by, stack.data(), (uint32_t)stack.size());
      if (!background) continue;
      flags[(size_t)by * pc.bx_n + bx] = 1;
      n_found++;
      n_pixels += (std::min((bx + 1) * SOL_TILE, width) - bx * SOL_TILE) * (std::min((by + 1) * SOL_TILE, height) - by * SOL_TILE);
    }
}

static SolSplitOptions split_options(const SolDevOverrides& ovr, const SolCreateOptions* opt) {
  SolSplitOptions sp;  // (the default: a budget of 30 %, kept when the splits shrink the primitives' summed box area below 85 %)
  if (opt && opt->split_percent < 0) sp.budget = 0.f;
  else if (opt && opt->split_percent > 0) { sp.budget = (float)opt->split_percent / 100.0f; sp.max_area_ratio = 1.f; }  // an explicit budget is kept
  if (ovr.split_percent >= 0) { sp.budget = (float)ovr.split_percent / 100.0f; sp.max_area_ratio = 1.f; }  // SOL_SPLIT (percent; 0 = off)
  if (ovr.split_slack >= 0) sp.level_slack = ovr.split_slack;                                               // SOL_SPLIT_SLACK
  if (ovr.split_keep >= 0) sp.max_area_ratio = (float)ovr.split_keep / 100.0f;                             // SOL_SPLIT_KEEP (percent)
  if (opt && opt->reinsertion_rounds != 0) sp.reinsertion_rounds = std::max(0, opt->reinsertion_rounds);  // (0: the default, 8 rounds)
  if (ovr.reinsert_rounds >= 0) sp.reinsertion_rounds = ovr.reinsert_rounds;                               // SOL_REINSERT (rounds; 0 = off)
  if (ovr.reinsert_stride > 0) sp.reinsertion_stride = ovr.reinsert_stride;                                // SOL_REINSERT_STRIDE
  sp.node_cost = (float)ovr.node_cost;  // (SOL_NODE_COST; 2.5)
  sp.verbose = ovr.verbose;
  return sp;
}

// The dfs_index contract (solstrale_hip.h; DESIGN.md 4, the tie rule and rule 8): every sphere, quad, triangle and medium the world tree
// reaches carries its number in the pre-order walk from `root` (left before right; a medium before its boundary sub-tree, the walk going on
// after the boundary) - what the host's Flattener emits and what the float oracle's walk (later hit wins) decides ties by. A record
// reached more than once (a shared sub-tree) carries the number of its LAST visit, the one that wins its ties in the oracle. Linear in
// the descriptor whatever the sharing: the references form a DAG, each vertex's number of walked records is summed bottom-up, and its
// last visit is the longest path to it (the largest of its parents' last visits plus the edge's offset), relaxed in topological order.
// Records the walk never reaches (a light outside the tree) are never a search candidate and are not checked. Also refuses what
// the walk cannot follow: a reference of an unknown kind or out of range, a cycle (a medium boundary's, which tb.resolve does not walk).
// `counted`: TreeBuilder's count during the world's resolve - the whole answer for a tree without mediums and without sharing (all
// the large scenes: the walk costs nothing beyond resolve's own, where this general one took C5's 2.3 M records 80 ms on its own).
static int check_dfs_numbering(const SolSceneDesc& d, const TreeBuilder::DfsCount& counted) {
  const uint32_t n_of[6] = {0u, d.n_nodes, d.n_spheres, d.n_quads, d.n_triangles, d.n_mediums};
  static const char* const kind_name[6] = {"none", "node", "sphere", "quad", "triangle", "medium"};
  uint64_t base[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int k = 1; k < 6; ++k) base[k + 1] = base[k] + n_of[k];
  if (SOL_REF_KIND(d.root) == SOL_REF_NONE) return SOL_OK;
  const uint64_t n_vert = base[6] - base[1];  // vertex of a reference = base[kind] - base[NODE] + index
  if (n_vert >= 0xFFFFFFFFull) return sol_fail(SOL_EINVAL, "dfs_index check: %llu records", (unsigned long long)n_vert);
  auto vertex = [&](uint32_t ref, uint32_t& v) {
    const uint32_t k = SOL_REF_KIND(ref);
    if (k < SOL_REF_NODE || k > SOL_REF_MEDIUM || SOL_REF_INDEX(ref) >= n_of[k]) return false;
    v = (uint32_t)(base[k] - base[1] + SOL_REF_INDEX(ref));
    return true;
  };
  auto kind_of = [&](uint32_t v) { uint32_t k = 1; while (k < 5 && v >= base[k + 1] - base[1]) ++k; return k; };
  // the references a vertex leads to, in walk order (NONE where there is none)
  auto child = [&](uint32_t v, int which) -> uint32_t {
    if (v < n_of[SOL_REF_NODE]) return which == 0 ? d.nodes[v].left : which == 1 ? d.nodes[v].right : 0u;
    if (v >= base[5] - base[1]) return which == 0 ? d.mediums[v - (base[5] - base[1])].boundary : 0u;
    return 0u;
  };
  auto dfs_of = [&](uint32_t k, uint32_t i) {
    return k == SOL_REF_SPHERE ? d.spheres[i].dfs_index : k == SOL_REF_QUAD ? d.quads[i].dfs_index : k == SOL_REF_TRIANGLE ? d.triangles[i].dfs_index : d.mediums[i].dfs_index;
  };
  auto wrong = [&](uint32_t k, uint32_t i, uint32_t want) {
    return sol_fail(SOL_EINVAL, "dfs_index: %s %u carries %u, the world tree's depth-first order gives it %u (solstrale_hip.h, SolSceneDesc)", kind_name[k], i, dfs_of(k, i), want);
  };
  if (counted.plain) return counted.bad_ref ? wrong(SOL_REF_KIND(counted.bad_ref), SOL_REF_INDEX(counted.bad_ref), counted.bad_want) : SOL_OK;
  const uint32_t cap = 0xFFFFFFFFu;  // (walk lengths and positions saturate - a shared sub-tree can double them per level -; past 2^31 is refused)
  auto add = [&](uint32_t a, uint32_t b) { return a > cap - b ? cap : a + b; };
  std::vector<uint32_t> walked(n_vert, 0), last(n_vert, 0);
  std::vector<uint8_t> state(n_vert, 0);  // 0 unseen, 1 on the DFS path, 2 done
  std::vector<uint32_t> post;
  post.reserve(n_vert);
  uint32_t root;
  if (!vertex(d.root, root)) return sol_fail(SOL_EINVAL, "dfs_index check: root reference out of range");
  std::vector<std::pair<uint32_t, int>> stk{{root, 0}};
  state[root] = 1;
  while (!stk.empty()) {
    const uint32_t v = stk.back().first;
    const int which = stk.back().second++;
    if (which < 2) {
      const uint32_t r = child(v, which);
      if (SOL_REF_KIND(r) == SOL_REF_NONE) continue;
      uint32_t u;
      if (!vertex(r, u)) return sol_fail(SOL_EINVAL, "dfs_index check: %s %u leads to a reference out of range (0x%08x)", kind_name[kind_of(v)], (uint32_t)(v - (base[kind_of(v)] - base[1])), r);
      if (state[u] == 1) return sol_fail(SOL_EINVAL, "dfs_index check: cycle through %s %u", kind_name[kind_of(u)], (uint32_t)(u - (base[kind_of(u)] - base[1])));
      if (state[u] == 0) { state[u] = 1; stk.push_back({u, 0}); }
      continue;
    }
    uint32_t n = kind_of(v) == SOL_REF_NODE ? 0u : 1u;  // the record itself (a medium: then its boundary)
    for (int w = 0; w < 2; ++w) {
      uint32_t u;
      if (vertex(child(v, w), u)) n = add(n, walked[u]);
    }
    walked[v] = n;
    state[v] = 2;
    post.push_back(v);
    stk.pop_back();
  }
  // reverse post-order is a topological order: every parent's last visit is final before its children are relaxed
  for (size_t j = post.size(); j-- > 0;) {
    const uint32_t v = post[j];
    uint32_t at = add(last[v], kind_of(v) == SOL_REF_NODE ? 0u : 1u);
    for (int w = 0; w < 2; ++w) {
      uint32_t u;
      if (!vertex(child(v, w), u)) continue;
      last[u] = std::max(last[u], at);
      at = add(at, walked[u]);
    }
  }
  for (uint32_t v : post) {
    const uint32_t k = kind_of(v);
    if (k == SOL_REF_NODE) continue;
    const uint32_t i = (uint32_t)(v - (base[k] - base[1]));
    if (last[v] > 0x7FFFFFFFu) return sol_fail(SOL_EINVAL, "dfs_index: the world tree walks %s %u at a position beyond 2^31 - 1 (%u)", kind_name[k], i, last[v]);
    if (dfs_of(k, i) != last[v]) return wrong(k, i, last[v]);
  }
  return SOL_OK;
}

// ---- what sol_scene_create and the two tree diagnostics share: the world, and the ONE host pipeline from it to a device layout ----
static bool has_environment(const SolSceneDesc& d) { return d.abi_version >= 2u && d.env_texels && d.env_width && d.env_height; }  // (a version-1 description ends before these fields)
// The world as every entry point sees it: the fp32 box pad, the reference-shaped binary tree (TreeBuilder) and its resolved root.
struct World {
  const float box_pad; TreeBuilder tb;
  uint32_t root_ref = 0, medium_depth = 0;  // medium_depth: the deepest boundary tree of a constant medium
  Box root_box = empty_box();
  bool needles = false; const uint32_t counts[3];  // sol_scene_has_needles (a pass over every triangle: asked once); triangles, spheres, quads
  explicit World(const SolSceneDesc& d) : box_pad(box_pad_for(d)), tb(d, box_pad), counts{d.n_triangles, d.n_spheres, d.n_quads} {}
  bool single() const { return SOL_REF_KIND(root_ref) != SOL_REF_NODE; }  // the world is ONE primitive
  uint32_t stack_dwords(const WideLayout& l) const { return 2u * l.depth + medium_depth + 2; }  // (a wide level keeps at most one sibling group of two dwords)
};
static const uint32_t STACK_LIMIT = SOL_LDS_STACK + SOL_SPILL_STACK;
// A finished host-built world tree: the binary tree it was collapsed from (`sah`: a rebuild; null: the reference's topology), the
// collapse with its area estimate (wb->cost()), the device layout.
struct HostTree { std::unique_ptr<SahBuilder> sah; std::unique_ptr<WideBuilder> wb; WideLayout lay; uint32_t emin = 1; };
static const char* const COLLECT_ERROR = "the world's primitives cannot be collected (non-finite box or fewer than two)";
// The host pipeline, written once: collect and binned-SAH rebuild (`bins` > 0; 0 = the reference's topology as resolved; primitives a
// caller has collected already come in t.sah), collapse into wide nodes under the three SolDevOverrides tunables, device layout; a world of
// one primitive becomes a root with a single child. Returns "" or why there is no tree (t.wb->range_error: the exponent range).
static std::string host_tree(const World& w, int bins, const SolDevOverrides& ovr, HostTree& t) {
  const std::vector<DNode>* bin = &w.tb.nodes;
  uint32_t bin_root = w.root_ref;
  if (bins && !w.single()) {
    if (!t.sah) { t.sah.reset(new SahBuilder()); if (!t.sah->collect(w.tb.nodes, w.root_ref)) return COLLECT_ERROR; }
    Box b;
    t.sah->BINS = bins; bin_root = t.sah->build(0, t.sah->prims.size(), 0, b); bin = &t.sah->nodes;
  }
  t.wb.reset(new WideBuilder(*bin, w.box_pad));
  t.wb->dp_collapse = !ovr.greedy_collapse; t.wb->slot_by_assignment = !ovr.octant_slots; t.wb->NODE_COST = ovr.node_cost;
  t.wb->set_exponent_range(w.root_box);
  const uint32_t wide_root = w.single() ? t.wb->build_single(w.root_ref, w.root_box) : t.wb->build(SOL_REF_INDEX(bin_root), 0);
  if (t.wb->range_error) return "exponent range";
  if (!t.lay.run(t.wb->out, SOL_REF_INDEX(wide_root), t.wb->emin, w.counts[0], w.counts[1], w.counts[2])) return t.lay.error;
  t.emin = t.wb->emin;
  return "";
}
// The diagnostics' world: resolved and numbered as sol_scene_create does it, a tree (no single primitive), its primitives collected (`prims`: a copy,
// before a rebuild reorders them) and the host-built tree `use_sah` names: 0 the reference's topology, 1 sixteen bins, n > 1 that many (at most MAX_BINS), < 0 none.
static int diag_world(const SolSceneDesc& d, int use_sah, const SolDevOverrides& ovr, World& w, HostTree& t, std::vector<SahBuilder::Prim>* prims) {
  if (!w.tb.resolve(d.root, 0, w.root_ref, w.root_box)) return sol_fail(SOL_EINVAL, "world: %s", w.tb.error.c_str());
  if (int rc = check_dfs_numbering(d, w.tb.dfs)) return rc;
  if (w.single()) return sol_fail(SOL_EINVAL, "the world is a single primitive: no tree");
  t.sah.reset(new SahBuilder());
  if (!t.sah->collect(w.tb.nodes, w.root_ref)) return sol_fail(SOL_EINVAL, "%s", COLLECT_ERROR);
  if (prims) *prims = t.sah->prims;
  if (use_sah < 0) return SOL_OK;
  const std::string err = host_tree(w, use_sah > 1 ? std::min((int)SahBuilder::MAX_BINS, use_sah) : use_sah ? 16 : 0, ovr, t);
  return err.empty() ? SOL_OK : sol_fail(SOL_EINVAL, "wide tree layout: %s", err.c_str());
}
static int world_tree_check(const SolSceneDesc* d, int use_sah, SolTreeCheck* out) {
  if (!d || !out) return sol_fail(SOL_EINVAL, "null argument");
  std::memset(out, 0, sizeof *out);
  const SolDevOverrides ovr = sol_dev_overrides();
  World w(*d);
  HostTree tree;
  std::vector<SahBuilder::Prim> prims;
  if (int rc = diag_world(*d, use_sah, ovr, w, tree, &prims)) return rc;
  std::map<uint32_t, int> expected;  // primitive reference -> multiplicity
  std::map<uint32_t, Box> prim_box;
  for (const auto& p : prims) { expected[p.ref]++; prim_box[p.ref] = p.box; }
  if (use_sah < 0)
    for (auto& e : expected) e.second = 1;  // (the device build keeps one copy of a shared sub-tree's primitives)
  out->n_primitives = (uint32_t)prims.size();
  if (use_sah < 0) out->n_primitives = (uint32_t)expected.size();
  const WideLayout& lay = tree.lay;
  DeviceSplitInfo split;
  std::vector<DTri> dev_tris;
  if (use_sah < 0) {  // the tree sol_build.hip builds on the GPU, checked like the host-built ones
    if (const int rc = sol_device_check()) return rc;
    HIP_TRY(hipSetDevice(0));
    dev_tris = cast_triangles(*d);
    SolSplitOptions sp = split_options(ovr, nullptr);
    sp.want_boxes = true;
    std::vector<SolBuildPrim> build_prims;
    int rc = collect_build_prims(w.tb.nodes, w.root_ref, w.root_box, build_prims);
    DevicePrepared pr;
    if (!rc) rc = device_world_tree_prepare(build_prims, w.root_box, w.box_pad, w.counts, dev_tris, sp, ovr.ploc_radius, nullptr, pr);
    if (!rc) rc = device_world_tree_finish(pr, w.counts, sp, tree.lay, tree.emin, &split);
    if (rc) return rc;
    // a split triangle has several references; each is expected once
    for (uint32_t e = d->n_triangles; e < split.tri_of_ref.size(); ++e) {
      auto it = expected.find(SOL_MAKE_REF(SOL_REF_TRIANGLE, split.tri_of_ref[e]));
      if (it != expected.end()) it->second++; else out->leaf_mismatches++;
    }
    out->n_extra_references = (uint32_t)(split.tri_of_ref.size() - d->n_triangles);
    out->n_split_triangles = split.split_triangles;
  } else {
    out->inner_area = tree.wb->inner_area; out->leaf_area = tree.wb->leaf_area;
  }
  out->n_wide = (uint32_t)lay.nodes.size();
  out->depth = lay.depth;
  std::map<uint32_t, int> found;
  // The DEVICE form is what gets checked, decoded exactly as the kernel decodes it (WideView), permuted primitive arrays mapped back
  // to the caller's indices for the comparison.
  const uint32_t ref_kind_of[4] = {SOL_REF_NONE, SOL_REF_TRIANGLE, SOL_REF_SPHERE, SOL_REF_QUAD};
  // returns the union of the padded primitive boxes below node `ni`
  std::function<Box(uint32_t, uint32_t)> walk = [&](uint32_t ni, uint32_t depth) -> Box {
    Box all = empty_box();
    if (depth > 4096 || ni >= lay.nodes.size()) { out->leaf_mismatches++; return all; }
    const WideView v(lay.nodes[ni], tree.emin);
    if (v.imask & v.lmask) out->bad_empty_slots++;
    uint32_t n_children = 0;
    for (int s = 0; s < SOL_WIDE_CHILDREN; ++s) {
      if (!v.occupied(s)) {  // an empty slot must have an inverted box (never hit)
        uint32_t ql[3], qh[3];
        v.plane_bytes(s, ql, qh);
        if (!(ql[0] == 255u && qh[0] == 0u && ql[1] == 255u && qh[1] == 0u && ql[2] == 255u && qh[2] == 0u)) out->bad_empty_slots++;
        continue;
      }
      n_children++;
      Box below;
      if (v.inner(s)) {
        below = walk(v.inner_index(s), depth + 1);
      } else {
        const uint32_t idx = v.prim_index(s);
        uint32_t ref = v.kind == SOL_LEAF_REFS ? (idx < lay.leaf_refs.size() ? lay.leaf_refs[idx] : 0u) : SOL_MAKE_REF(ref_kind_of[v.kind], idx);
        const int a = WideLayout::arr(SOL_REF_KIND(ref));
        const uint32_t dev_idx = SOL_REF_INDEX(ref);  // (index into the permuted device array; for a listed reference too)
        if (a >= 0) ref = SOL_REF_INDEX(ref) < lay.old_of_new[a].size() ? SOL_MAKE_REF(SOL_REF_KIND(ref), lay.old_of_new[a][SOL_REF_INDEX(ref)]) : 0u;
        found[ref]++;
        out->n_leaf_refs++;
        auto it = prim_box.find(ref);
        below = it == prim_box.end() ? empty_box() : it->second;
        if (a == 0 && !split.ref_box.empty() && dev_idx < split.ref_of_dev.size()) {
          // (device build) the box of THIS reference of the triangle: the whole triangle's, or the part a pre-split gave it
          const uint32_t e = split.ref_of_dev[dev_idx];
          if ((size_t)e * 6 + 6 <= split.ref_box.size()) std::memcpy(below.v, &split.ref_box[(size_t)e * 6], 24);
        }
      }
      float lo[3], hi[3];
      v.box(s, lo, hi);
      bool ok = true;
      for (int a = 0; a < 3; ++a)
        if (below.v[2 * a] <= below.v[2 * a + 1] && !(lo[a] <= below.v[2 * a] && hi[a] >= below.v[2 * a + 1])) ok = false;
      if (!ok) out->box_violations++;
      SahBuilder::grow(all, below);
    }
    if (n_children > out->max_children) out->max_children = n_children;
    return all;
  };
  walk(0, 0);
  // Pre-split triangles: the boxes of a triangle's references must cover the triangle between them (a ray that hits the triangle
  // at a point enters the reference box that holds the point). Checked on a fixed set of 67 points per split triangle: corners,
  // edge mid-points, centroid and 60 low-discrepancy interior points.
  if (split.tri_of_ref.size() > d->n_triangles) {
    std::vector<std::vector<uint32_t>> refs_of(d->n_triangles);
    for (uint32_t e = d->n_triangles; e < split.tri_of_ref.size(); ++e) {
      const uint32_t t = split.tri_of_ref[e];
      if (t >= d->n_triangles) { out->split_uncovered++; continue; }
      if (refs_of[t].empty()) refs_of[t].push_back(t);
      refs_of[t].push_back(e);
    }
    for (uint32_t t = 0; t < d->n_triangles; ++t) {
      if (refs_of[t].empty()) continue;
      const DTri& T = dev_tris[t];
      const double v0[3] = {T.v0x, T.v0y, T.v0z}, e1[3] = {T.e1x, T.e1y, T.e1z}, e2[3] = {T.e2x, T.e2y, T.e2z};
      for (int k = 0; k < 67; ++k) {
        double u, v;
        if (k < 7) { const double pts[7][2] = {{0, 0}, {1, 0}, {0, 1}, {.5, 0}, {0, .5}, {.5, .5}, {1. / 3, 1. / 3}}; u = pts[k][0]; v = pts[k][1]; }
        else { u = std::fmod((k - 6) * 0.7548776662466927, 1.0); v = std::fmod((k - 6) * 0.5698402909980532, 1.0); if (u + v > 1.0) { u = 1.0 - u; v = 1.0 - v; } }
        const double p[3] = {v0[0] + u * e1[0] + v * e2[0], v0[1] + u * e1[1] + v * e2[1], v0[2] + u * e1[2] + v * e2[2]};
        bool in_one = false;
        for (uint32_t e : refs_of[t]) {
          if ((size_t)e * 6 + 6 > split.ref_box.size()) continue;
          const float* b = &split.ref_box[(size_t)e * 6];
          if (p[0] >= b[0] && p[0] <= b[1] && p[1] >= b[2] && p[1] <= b[3] && p[2] >= b[4] && p[2] <= b[5]) { in_one = true; break; }
        }
        if (!in_one) out->split_uncovered++;
      }
    }
  }
  // the permutations must be permutations
  for (int a = 0; a < 3; ++a) {
    // (device build with pre-split triangles: the records are a permutation of the EXPANDED references, several of which are
    // copies of one triangle; every triangle must find a copy of itself at new_of_old)
    const bool expanded = a == 0 && split.ref_of_dev.size() > d->n_triangles;
    const std::vector<uint32_t>& perm = expanded ? split.ref_of_dev : lay.old_of_new[a];
    std::vector<uint8_t> seen(perm.size(), 0);
    for (uint32_t o : perm) { if (o >= seen.size() || seen[o]) out->leaf_mismatches++; else seen[o] = 1; }
    if (!expanded && lay.old_of_new[a].size() != lay.new_of_old[a].size()) out->leaf_mismatches++;
    if (expanded) {
      if (lay.new_of_old[0].size() != d->n_triangles || lay.old_of_new[0].size() != perm.size()) out->leaf_mismatches++;
      else
        for (uint32_t t = 0; t < d->n_triangles; ++t)
          if (lay.new_of_old[0][t] >= lay.old_of_new[0].size() || lay.old_of_new[0][lay.new_of_old[0][t]] != t) out->leaf_mismatches++;
    }
  }
  for (const auto& e : expected) {
    auto it = found.find(e.first);
    const int f = it == found.end() ? 0 : it->second;
    if (f != e.second) out->leaf_mismatches += (uint32_t)std::abs(f - e.second);
  }
  for (const auto& f : found)
    if (!expected.count(f.first)) out->leaf_mismatches += (uint32_t)f.second;
  return SOL_OK;
}

// ---- sol_scene_create: the stages, in the order sol_scene_create_ex calls them ----
static double seconds_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
// What every stage may read: the description, the developer overrides (parsed once) and the options in force, SOL_VERBOSE's clock.
struct CreateCtx {
  const SolSceneDesc& d; const SolDevOverrides ovr; SolCreateOptions opt{}; bool has_env = false;
  const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
  void say(const char* what) const { if (ovr.verbose) std::fprintf(stderr, "[solstrale] create: %s at %.1f ms\n", what, 1e3 * seconds_since(t_begin)); }
};
// The description in the device's record types, in the caller's order.
struct HostRecords {
  std::vector<DTex> texs; std::vector<DMat> mats; std::vector<DTri> tris; std::vector<DTriShade> tshade; std::vector<DQuad> quads;
  std::vector<DSphere> spheres; std::vector<DMedium> mediums; std::vector<uint32_t> lights;
};
// A candidate world tree: a host-built one (HostTree) or a device-built layout (lay and emin alone, `built`: what its build did), and
// its device arrays once uploaded - released with the candidate unless the scene has taken them.
struct TreeCand : HostTree { std::string name; uint32_t depth = 0; double cost = 0.; DeviceSplitInfo built; DevTree dev; };
struct SceneDestroy { void operator()(SolScene* s) const { sol_scene_destroy(s); } };
using ScenePtr = std::unique_ptr<SolScene, SceneDestroy>;  // (a stage that fails leaves nothing of the scene behind)
// 1. options and the description's header
static int check_options_and_header(CreateCtx& c, const SolCreateOptions* opt_in) {
  const SolSceneDesc* d = &c.d;
  SolCreateOptions& opt = c.opt;
  if (opt_in) {
    if (opt_in->size < 8 || opt_in->size > 4096) return sol_fail(SOL_EINVAL, "SolCreateOptions.size %u", opt_in->size);
    std::memcpy(&opt, opt_in, std::min<size_t>(opt_in->size, sizeof opt));
  }
  if (opt.world_tree < SOL_TREE_AUTO || opt.world_tree > SOL_TREE_HOST_PROBE) return sol_fail(SOL_EINVAL, "bad world_tree option %d", opt.world_tree);
  if (opt.split_percent > 1000 || opt.reinsertion_rounds > 1024)  // (a typo must not become a build of hours: ten times the references, a thousand rounds)
    return sol_fail(SOL_EINVAL, "SolCreateOptions: split_percent %d (at most 1000) / reinsertion_rounds %d (at most 1024)", opt.split_percent, opt.reinsertion_rounds);
  if (opt.dynamic_triangles != 0 && opt.dynamic_triangles != 1) return sol_fail(SOL_EINVAL, "SolCreateOptions.dynamic_triangles %d (0 or 1)", opt.dynamic_triangles);
  if (opt.dynamic_primitives != 0 && opt.dynamic_primitives != 1)
    return sol_fail(SOL_EINVAL, "SolCreateOptions.dynamic_primitives %d (0 or 1; the reserved2 word of earlier headers)", opt.dynamic_primitives);
  if (opt.dynamic_primitives && !opt.dynamic_triangles)  // (it extends dynamic_triangles; and a stray 1 in what used to be reserved2 is still refused)
    return sol_fail(SOL_EINVAL, "SolCreateOptions.dynamic_primitives (the reserved2 word of earlier headers) needs dynamic_triangles = 1 as well");
  if (d->abi_version != SOL_ABI_VERSION && d->abi_version != 1u) return sol_fail(SOL_EINVAL, "abi_version %u, expected %u (or 1)", d->abi_version, SOL_ABI_VERSION);
  c.has_env = has_environment(*d);
  if (c.has_env && ((uint64_t)d->env_width * d->env_height > (1ull << 28) || !std::isfinite(d->env_scale))) return sol_fail(SOL_EINVAL, "bad environment map");
  if (d->width < 2 || d->height < 2 || (uint64_t)d->width * d->height > 0x3FFFFFFFull) return sol_fail(SOL_EINVAL, "bad image size %ux%u", d->width, d->height);
  if (d->shader_kind > SOL_SHADER_SIMPLE) return sol_fail(SOL_EINVAL, "bad shader kind %u", d->shader_kind);
  if ((d->n_nodes && !d->nodes) || (d->n_spheres && !d->spheres) || (d->n_quads && !d->quads) ||
      (d->n_triangles && !d->triangles) || (d->n_mediums && !d->mediums) || (d->n_materials && !d->materials) ||
      (d->n_textures && !d->textures) || (d->n_texel_bytes && !d->texels) || (d->n_lights && !d->lights))
    return sol_fail(SOL_EINVAL, "null array with non-zero count");
  // Renderer::new: "Scene should have at least one light" (src/renderer/mod.rs:143-147)
  if (d->n_lights == 0) return sol_fail(SOL_ENOLIGHT, "Scene should have at least one light");
  if (d->n_texel_bytes > 0xFFFFFFF0ull) return sol_fail(SOL_EINVAL, "more than 4 GiB of texels");
  return SOL_OK;
}
// 2. textures, materials and the NEEDS_UV closure
static int cast_materials(const SolSceneDesc* d, HostRecords& r) {
  std::vector<DTex>& texs = r.texs;
  texs.resize(d->n_textures);
  for (uint32_t i = 0; i < d->n_textures; ++i) {
    const SolTexture& t = d->textures[i];
    DTex& o = texs[i];
    std::memset(&o, 0, sizeof o);
    o.kind = t.kind;
    if (t.kind == SOL_TEX_IMAGE) {
      // (no sum or product here may wrap: an offset of 2^64 - 1 plus a size is a small number again)
      const uint64_t px = (uint64_t)t.width * t.height;
      if (!t.width || !t.height || px > d->n_texel_bytes / 3 || t.texel_offset > d->n_texel_bytes - px * 3)
        return sol_fail(SOL_EINVAL, "texture %u: image outside texel buffer", i);
      o.w = t.width; o.h = t.height; o.offset = (uint32_t)t.texel_offset;
    } else if (t.kind == SOL_TEX_SOLID) {
      o.r = (float)t.rgb[0]; o.g = (float)t.rgb[1]; o.b = (float)t.rgb[2];
    } else {
      return sol_fail(SOL_EINVAL, "texture %u: bad kind %d", i, t.kind);
    }
  }
  auto tex_ok = [&](int32_t id, bool optional) { return (optional && id < 0) || (id >= 0 && (uint32_t)id < d->n_textures); };
  std::vector<DMat>& mats = r.mats;
  mats.resize(d->n_materials);
  for (uint32_t i = 0; i < d->n_materials; ++i) {
    const SolMaterial& m = d->materials[i];
    DMat& o = mats[i];
    std::memset(&o, 0, sizeof o);
    o.kind = m.kind; o.albedo = m.albedo_tex; o.normal = m.normal_tex; o.m1 = m.m1; o.m2 = m.m2;
    o.param = (float)m.param;
    if (std::isnan(m.param)) o.flags |= DMAT_PARAM_NONE;
    if (m.kind != SOL_MAT_BLEND && m.albedo_tex >= 0 && (uint32_t)m.albedo_tex < d->n_textures && texs[m.albedo_tex].kind == SOL_TEX_SOLID) {
      o.flags |= DMAT_ALBEDO_SOLID;
      o.ar = texs[m.albedo_tex].r; o.ag = texs[m.albedo_tex].g; o.ab = texs[m.albedo_tex].b;
    }
    switch (m.kind) {
      case SOL_MAT_LAMBERTIAN: case SOL_MAT_METAL: case SOL_MAT_DIELECTRIC:
        if (!tex_ok(m.albedo_tex, false) || !tex_ok(m.normal_tex, true)) return sol_fail(SOL_EINVAL, "material %u: bad texture id", i);
        break;
      case SOL_MAT_DIFFUSE_LIGHT: case SOL_MAT_ISOTROPIC:
        if (!tex_ok(m.albedo_tex, false)) return sol_fail(SOL_EINVAL, "material %u: bad texture id", i);
        o.normal = -1;
        break;
      case SOL_MAT_BLEND:
        if (m.m1 < 0 || m.m2 < 0 || (uint32_t)m.m1 >= d->n_materials || (uint32_t)m.m2 >= d->n_materials || (uint32_t)m.m1 == i || (uint32_t)m.m2 == i)
          return sol_fail(SOL_EINVAL, "material %u: bad blend children", i);
        break;
      default: return sol_fail(SOL_EINVAL, "material %u: bad kind %d", i, m.kind);
    }
  }
  // NEEDS_UV: any image texture reachable from the material (Blend children included; bounded iteration)
  for (int pass = 0; pass < 16; ++pass)
    for (uint32_t i = 0; i < d->n_materials; ++i) {
      DMat& o = mats[i];
      bool need = false;
      if (o.kind == SOL_MAT_BLEND) need = (mats[o.m1].flags | mats[o.m2].flags) & DMAT_NEEDS_UV;
      else need = (o.albedo >= 0 && texs[o.albedo].kind == SOL_TEX_IMAGE) || (o.normal >= 0 && texs[o.normal].kind == SOL_TEX_IMAGE);
      if (need) o.flags |= DMAT_NEEDS_UV;
    }
  return SOL_OK;
}
static bool mat_ok(const SolSceneDesc* d, int32_t id) { return id >= 0 && (uint32_t)id < d->n_materials; }

// 3. primitives (plain casts)
static int cast_primitives(const SolSceneDesc* d, HostRecords& r) {
  std::vector<DTri>& tris = r.tris;
  std::vector<DTriShade>& tshade = r.tshade;
  tris.resize(d->n_triangles); tshade.resize(d->n_triangles);
  // (a million triangles are 0.03 s of casts on one core: split over a few threads above 64 k; every triangle is independent)
  auto cast_range = [&](uint32_t i0, uint32_t i1, int64_t* bad) {
    for (uint32_t i = i0; i < i1; ++i) {
      const SolTriangle& t = d->triangles[i];
      if (!mat_ok(d, t.material)) { if (*bad < 0) *bad = i; continue; }
      int uo[3];
      cast_triangle(t, false, tris[i], uo);
      sol_tri_cast_shade(&t, uo, &tshade[i]);
    }
  };
  const uint32_t nt = d->n_triangles;
  const uint32_t n_thr = nt >= 65536u ? std::min<uint32_t>(8u, std::max<uint32_t>(1u, std::thread::hardware_concurrency())) : 1u;
  std::vector<int64_t> bad(n_thr, -1);
  std::vector<std::thread> pool;
  for (uint32_t k = 1; k < n_thr; ++k) pool.emplace_back(cast_range, (uint32_t)((uint64_t)nt * k / n_thr), (uint32_t)((uint64_t)nt * (k + 1) / n_thr), &bad[k]);
  cast_range(0, (uint32_t)((uint64_t)nt / n_thr), &bad[0]);
  for (auto& th : pool) th.join();
  for (int64_t b : bad)
    if (b >= 0) return sol_fail(SOL_EINVAL, "triangle %u: bad material", (uint32_t)b);
  r.quads.resize(d->n_quads);
  for (uint32_t i = 0; i < d->n_quads; ++i) {
    const SolQuad& q = d->quads[i];
    if (!mat_ok(d, q.material)) return sol_fail(SOL_EINVAL, "quad %u: bad material", i);
    sol_quad_cast(&q, &r.quads[i]);
  }
  r.spheres.resize(d->n_spheres);
  for (uint32_t i = 0; i < d->n_spheres; ++i) {
    const SolSphere& s = d->spheres[i];
    if (!mat_ok(d, s.material)) return sol_fail(SOL_EINVAL, "sphere %u: bad material", i);
    sol_sphere_cast(&s, &r.spheres[i]);
  }
  return SOL_OK;
}
// 4. the world: box pad and needles, the 2^38 bound, the reference tree resolved, the constant mediums, the dfs_index numbering
static int resolve_world(const CreateCtx& c, World& w, HostRecords& r) {
  const SolSceneDesc* d = &c.d;
  TreeBuilder& tb = w.tb;
  w.needles = sol_scene_has_needles(d) != 0;
  // (the 7-wide node test's plane parameters must not overflow: sol_trace.h, wide_node_test; pad = largest |coordinate| * 2^-20)
  if (!(w.box_pad * 1048576.0f <= 2.7487791e11f)) return sol_fail(SOL_EINVAL, "the scene's coordinates reach beyond 2^38 (%g): not supported by the fp32 search", (double)w.box_pad * 1048576.0);
  if (!tb.resolve(d->root, 0, w.root_ref, w.root_box)) return sol_fail(SOL_EINVAL, "world: %s", tb.error.c_str());
  if (SOL_REF_KIND(w.root_ref) == SOL_REF_NONE) return sol_fail(SOL_EINVAL, "world is empty");
  const TreeBuilder::DfsCount world_dfs = tb.dfs;  // (the boundaries' resolves below count on)
  c.say("reference tree resolved");
  std::vector<DMedium>& mediums = r.mediums;
  mediums.resize(d->n_mediums);
  for (uint32_t i = 0; i < d->n_mediums; ++i) {
    const SolMedium& m = d->mediums[i];
    if (!mat_ok(d, m.material)) return sol_fail(SOL_EINVAL, "medium %u: bad material", i);
    if (i >= 0x1000u) return sol_fail(SOL_EINVAL, "more than 4096 constant mediums");
    DMedium& o = mediums[i];
    std::memset(&o, 0, sizeof o);
    tb.max_depth = 0;
    uint32_t bref;
    Box bb;
    if (!tb.resolve(m.boundary, 0, bref, bb)) return sol_fail(SOL_EINVAL, "medium %u boundary: %s", i, tb.error.c_str());
    if (SOL_REF_KIND(bref) == SOL_REF_MEDIUM || SOL_REF_KIND(bref) == SOL_REF_NONE) return sol_fail(SOL_EINVAL, "medium %u: unsupported boundary", i);
    w.medium_depth = std::max(w.medium_depth, tb.max_depth);
    o.boundary = bref; o.mat = m.material; o.nid = (float)m.negative_inverse_density; o.dfs = m.dfs_index;
    o.bxmin = bb.v[0]; o.bxmax = bb.v[1]; o.bymin = bb.v[2]; o.bymax = bb.v[3]; o.bzmin = bb.v[4]; o.bzmax = bb.v[5];
  }
  // a medium inside a medium boundary would recurse in the device search: reject (never built by the reference's scenes)
  for (uint32_t i = 0; i < d->n_mediums; ++i) {
    std::vector<uint32_t> stk{mediums[i].boundary};
    while (!stk.empty()) {
      uint32_t ref = stk.back(); stk.pop_back();
      if (SOL_REF_KIND(ref) == SOL_REF_MEDIUM) return sol_fail(SOL_EINVAL, "medium %u: nested ConstantMedium in a boundary is unsupported", i);
      if (SOL_REF_KIND(ref) == SOL_REF_NODE) { stk.push_back(tb.nodes[SOL_REF_INDEX(ref)].left); stk.push_back(tb.nodes[SOL_REF_INDEX(ref)].right); }
    }
  }
  return check_dfs_numbering(*d, world_dfs);  // (after the boundaries: their references are known good here)
}
// 5. 7-wide tree of the world, host candidates: the reference's topology collapsed, and binned-SAH rebuilds over the same primitives
// with 8, 16 and 64 bins (how well the binary splits line up with the wide collapse varies with the bin count: with the
// first, 8-wide layout C2 visited 9.8 / 12.2 / 11.4 nodes per ray at 8 / 16 / 64 bins and 11.2 on the reference's
// topology; C3 13.3 / 13.0 / 12.9 vs 14.4). A counted probe render on the device picks one (probe_candidates).
// SolCreateOptions.world_tree (or SOL_BVH=ref | sah (16 bins) | sah8 | sah16 | sah64) forces a candidate.
// The candidates wanted by `want` ("" = all of them, the probe decides): into `cands`, the provisional best first.
static TreeCand host_candidate(const World& w, const SolDevOverrides& ovr, const std::string& name, int bins) {  // (wb stays null where host_tree makes no tree)
  TreeCand t;
  t.name = name;
  if (!host_tree(w, bins, ovr, t).empty()) t.wb.reset();
  else t.depth = w.stack_dwords(t.lay);
  return t;
}
static int host_candidates(const CreateCtx& c, const World& w, const std::string& want, std::vector<TreeCand>& cands) {
  TreeCand ref = host_candidate(w, c.ovr, "ref", 0);
  if (w.single()) {
    if (!ref.wb) return sol_fail(SOL_EINVAL, "world: %s", ref.lay.error.c_str());
    cands.push_back(std::move(ref));
    return SOL_OK;
  }
  std::string layout_error;
  if (!ref.wb) layout_error = ref.lay.error.empty() ? "wide tree: exponent range" : ref.lay.error;
  else cands.push_back(std::move(ref));
  std::vector<int> bin_list = {8, 16, 64};
  if (!c.ovr.sah_bins.empty()) bin_list = c.ovr.sah_bins;  // (SOL_SAH_LIST)
  // (the rebuilds are independent of each other: one host thread each)
  std::vector<std::future<TreeCand>> jobs;
  for (int bins : bin_list) {
    const std::string name = "sah" + std::to_string(bins);
    if (want == "ref" || (!want.empty() && want != name)) continue;
    jobs.push_back(std::async(std::launch::async, host_candidate, std::cref(w), std::cref(c.ovr), name, bins));
  }
  for (auto& j : jobs) {
    TreeCand t = j.get();
    if (t.wb) cands.push_back(std::move(t));  // (non-finite boxes, a failed layout: no rebuild)
  }
  if (cands.empty()) return sol_fail(SOL_EINVAL, "world: %s", layout_error.c_str());
  // drop what cannot run; a forced choice drops the rest
  std::vector<TreeCand> keep;
  for (auto& t : cands)
    if (t.depth <= STACK_LIMIT && (want.empty() || t.name == want || (want != "ref" && t.name == "ref" && cands.size() == 1))) keep.push_back(std::move(t));
  if (keep.empty()) {
    uint32_t dmin = 0xFFFFFFFFu;
    for (auto& t : cands) if (t.wb) dmin = std::min(dmin, t.depth);
    return sol_fail(SOL_EDEPTH, "BVH depth %u exceeds the traversal stack (%d)", dmin, STACK_LIMIT);
  }
  cands = std::move(keep);
  // provisional choice by the surface-area estimate (it knows nothing of occlusion and visit order: the probe decides)
  size_t best = 0;
  for (size_t i = 1; i < cands.size(); ++i)
    if (cands[i].wb->cost() < cands[best].wb->cost()) best = i;
  std::swap(cands[0], cands[best]);
  return SOL_OK;
}
// 6. lights
static int check_lights(const SolSceneDesc* d, HostRecords& r) {
  r.lights.assign(d->lights, d->lights + d->n_lights);
  for (uint32_t i = 0; i < d->n_lights; ++i) {
    uint32_t k = SOL_REF_KIND(r.lights[i]), x = SOL_REF_INDEX(r.lights[i]);
    if (!((k == SOL_REF_SPHERE && x < d->n_spheres) || (k == SOL_REF_QUAD && x < d->n_quads) || (k == SOL_REF_TRIANGLE && x < d->n_triangles))) return sol_fail(SOL_EINVAL, "light %u: not a sphere/quad/triangle reference", i);
  }
  return SOL_OK;
}
// 7. the device: the handle, its stream, the properties
static int open_device(int device, ScenePtr& scene, std::chrono::steady_clock::time_point& t_upload0) {
  int ndev = 0;
  if (const int rc = sol_device_check(&ndev)) return rc;
  if (device < 0 || device >= ndev) return sol_fail(SOL_EDEVICE, "device %d out of range (%d devices)", device, ndev);
  HIP_TRY(hipSetDevice(device));
  SolScene* s = new SolScene();
  scene.reset(s);
  s->device = device;
  t_upload0 = std::chrono::steady_clock::now();  // ("upload" of sol_scene_build_times starts here, before the properties and the stream)
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  s->n_cu = prop.multiProcessorCount;
  HIP_TRY(hipStreamCreateWithFlags(&s->own_stream, hipStreamNonBlocking));
  s->stream = s->own_stream;
  return SOL_OK;
}
// 8. device candidates (sol_build.hip); where the build cannot make a tree, AUTO falls back to the host candidates
// The clustering radius of the device build decides little on average and a few per cent on any one scene, not monotonically (greedy
// clustering; MI355X, 1080p x 64 spp, ms with radius 8 / 16 / 32 / 64: C3 61.0 / 63.0 / 63.8 / 65.0, C2 37.1 / 35.7 / 34.7 / 37.3, C5
// 37.7 / 38.0 / 37.6 / 36.8, heterogeneous atrium 67.8 / 68.2 / 74.7 / 76.2 - profiles/r04_tree_ploc_radius.txt): round 4's SOL_TREE_AUTO
// built the tree with radius 16, 8 and 32, uploaded all three and let the counted probe choose (the probe's cost - 2.5 per node visit,
// 1 per primitive test - ranks them as the render times do): C5 paid twice the build time for a 0 % choice. An explicit
// SOL_TREE_DEVICE builds one tree (radius 16); SOL_PLOC_R forces a radius.
// Round 5: two radii (16 never won a probe on the four scene families and costs a third of the build time), each built as far as the
// collapse's surface-area cost of the whole tree; what is emitted, uploaded and probed follows from the two costs
// (profiles/r05_scene_creation.txt: on triangle meshes the cost ranks the candidates as the probes and the render times do - C3 1.7 %, the
// heterogeneous atrium 2.1 % apart -; on C5 the candidates are 0.3 % apart and render within 1 % of each other; on C2's spheres they are
// 0.6 % apart and the cost ranks them the WRONG way round - box area overstates how often a sphere is hit - by 7 % of render time):
//   apart by less than 0.4 % or by more than 1.2 %: the cheaper tree, unprobed;   in between: both, the counted probe decides.
static int device_candidates(const CreateCtx& c, const World& w, const std::vector<DTri>& tris, SolScene* s, std::vector<TreeCand>& cands) {
  const SolDevOverrides& ovr = c.ovr;
  const auto t_dev0 = std::chrono::steady_clock::now();
  std::vector<int> radii = {16};
  if (ovr.ploc_radius > 0) radii = {ovr.ploc_radius};
  else if (c.opt.world_tree == SOL_TREE_AUTO && ovr.bvh.empty()) radii = {8, 32};
  std::vector<SolBuildPrim> build_prims;
  int rc = collect_build_prims(w.tb.nodes, w.root_ref, w.root_box, build_prims);
  const SolSplitOptions sopt = split_options(ovr, &c.opt);
  std::vector<std::unique_ptr<DevicePrepared>> prepared;
  std::vector<int> prepared_radius;
  for (int radius : radii) {
    if (rc && prepared.empty()) break;
    std::unique_ptr<DevicePrepared> pr(new DevicePrepared);
    rc = device_world_tree_prepare(build_prims, w.root_box, w.box_pad, w.counts, tris, sopt, radius, s->stream, *pr);
    if (rc) {
      if (!prepared.empty()) { rc = SOL_OK; continue; }  // (a later candidate failed: the earlier ones stand)
      break;
    }
    if (ovr.verbose) std::fprintf(stderr, "[solstrale] device tree (radius %d): collapse cost %.6g\n", radius, (double)pr->dt.collapse_cost);
    prepared.push_back(std::move(pr));
    prepared_radius.push_back(radius);
  }
  if (prepared.size() == 2) {
    const double a = prepared[0]->dt.collapse_cost, b = prepared[1]->dt.collapse_cost;
    const double apart = (a > 0. && b > 0.) ? std::fabs(a - b) / std::min(a, b) : 0.;
    const bool probe_both = ovr.probe_radii > 0 || (ovr.probe_radii < 0 && apart >= 0.004 && apart <= 0.012);  // (SOL_PROBE_RADII=1 / 0 forces)
    if (b < a) { std::swap(prepared[0], prepared[1]); std::swap(prepared_radius[0], prepared_radius[1]); }  // the cheaper one first
    if (ovr.verbose) std::fprintf(stderr, "[solstrale] device trees: collapse costs %.4f %% apart -> %s\n", apart * 100., probe_both ? "both emitted, the probe decides" : "the cheaper one, unprobed");
    if (!probe_both) { prepared.pop_back(); prepared_radius.pop_back(); }
  }
  for (size_t k = 0; k < prepared.size() && !(rc && cands.empty()); ++k) {
    const int radius = prepared_radius[k];
    TreeCand t;
    t.name = radii.size() > 1 ? "device" + std::to_string(radius) : "device";
    DeviceSplitInfo& si = t.built;
    rc = device_world_tree_finish(*prepared[k], w.counts, sopt, t.lay, t.emin, &si);
    if (ovr.verbose) std::fprintf(stderr, "[solstrale] device tree (radius %d): pre-splitting %u triangles into %u extra references, box area ratio %.3f%s; %u reinsertion moves\n",
                                  radius, si.split_triangles, si.extra_references, si.area_ratio, si.extra_references ? "" : " (not kept)", si.reinsertion_moves);
    if (!rc) {
      t.depth = w.stack_dwords(t.lay);
      if (t.depth > STACK_LIMIT) rc = sol_fail(SOL_EDEPTH, "BVH depth %u exceeds the traversal stack (%d)", t.depth, STACK_LIMIT);
    }
    if (rc) {
      if (!cands.empty()) { rc = SOL_OK; continue; }  // (a later candidate failed: the earlier ones stand)
      break;
    }
    // Small scenes: the radii often give the SAME tree (the layout is a function of the tree alone, so equal trees are equal
    // bytes) - a duplicate is not uploaded and probed a second time (the reference's test scene: 33 identical nodes either way).
    bool duplicate = false;
    for (const TreeCand& p : cands) {
      const WideLayout &a = p.lay, &b = t.lay;
      if (p.emin != t.emin || a.nodes.size() != b.nodes.size() || a.leaf_refs != b.leaf_refs) continue;
      if (std::memcmp(a.nodes.data(), b.nodes.data(), a.nodes.size() * sizeof(DWide)) != 0) continue;
      if (a.old_of_new[0] == b.old_of_new[0] && a.old_of_new[1] == b.old_of_new[1] && a.old_of_new[2] == b.old_of_new[2]) { duplicate = true; break; }
    }
    if (duplicate) {
      if (ovr.verbose) std::fprintf(stderr, "[solstrale] device tree (radius %d): the same tree as an earlier candidate, dropped\n", radius);
      continue;
    }
    cands.push_back(std::move(t));
  }
  prepared.clear();
  s->build_times[2] = seconds_since(t_dev0);
  if (!cands.empty()) return SOL_OK;
  // AUTO falls back to the host candidates when the device build cannot make a tree (a primitive with a non-finite or inverted box -
  // e.g. a NaN vertex of an OBJ -, more than 2^23 primitives, no memory for its scratch): scenes the host path accepts are never
  // refused by the default. An explicit SOL_TREE_DEVICE (or SOL_BVH=device) keeps the hard error.
  if (c.opt.world_tree == SOL_TREE_DEVICE || ovr.bvh == "device") return rc;
  s->tree_note = std::string("device build failed (") + sol_last_error() + "): host candidates";
  if (ovr.verbose) std::fprintf(stderr, "[solstrale] world tree: %s\n", s->tree_note.c_str());
  const auto t_host0 = std::chrono::steady_clock::now();
  if ((rc = host_candidates(c, w, "", cands))) return rc;
  s->build_times[0] += seconds_since(t_host0);
  return SOL_OK;
}
// 9. upload. Everything that depends on the choice of the world tree - the tree itself, the permuted primitive arrays and every table of
// references into them - goes into the candidate's DevTree: candidate 0 first, the others only if a probe has to decide.
static int upload_tree(const SolSceneDesc& d, const World& w, const HostRecords& r, TreeCand& c) {
  // (the node test reads plane bytes as the fp16 subnormals q * 2^-24 and keeps the 2^24 in the node scales: sol_trace.h)
  if (c.emin + 31u + 24u > 254u) return sol_fail(SOL_EINVAL, "the scene is too large for the quantised world tree (extent beyond 2^100)");
  const WideLayout& L = c.lay;
  DevTree& t = c.dev;
  std::vector<DTri> ptris(L.old_of_new[0].size());  // (more records than triangles when the device build pre-split some: copies)
  std::vector<DTriShade> pshade(ptris.size()); std::vector<DQuad> pquads(r.quads.size()); std::vector<DSphere> pspheres(r.spheres.size());
  for (size_t i = 0; i < ptris.size(); ++i) { ptris[i] = r.tris[L.old_of_new[0][i]]; pshade[i] = r.tshade[L.old_of_new[0][i]]; }
  for (size_t i = 0; i < r.spheres.size(); ++i) pspheres[i] = r.spheres[L.old_of_new[1][i]];
  for (size_t i = 0; i < r.quads.size(); ++i) pquads[i] = r.quads[L.old_of_new[2][i]];
  std::vector<DNode> pnodes = d.n_mediums > 0 ? w.tb.nodes : std::vector<DNode>();  // the 2-wide tree serves medium boundaries only
  for (auto& n : pnodes) { n.left = L.remap(n.left); n.right = L.remap(n.right); }
  std::vector<DMedium> pmed = r.mediums;
  for (auto& m : pmed) m.boundary = L.remap(m.boundary);
  std::vector<uint32_t> plights = r.lights;
  for (auto& l : plights) l = L.remap(l);
  int e;
  if ((e = sol_upload(L.nodes, t.wides)) || (e = sol_upload(L.leaf_refs, t.leaf_refs)) || (e = sol_upload(ptris, t.tris)) || (e = sol_upload(pshade, t.tri_shade)) ||
      (e = sol_upload(pquads, t.quads)) || (e = sol_upload(pspheres, t.spheres)) || (e = sol_upload(pnodes, t.nodes)) || (e = sol_upload(pmed, t.mediums)) ||
      (e = sol_upload(plights, t.lights)))
    return e;  // (what was uploaded goes with the candidate)
  t.emin = c.emin; t.depth = c.depth; t.root = L.remap(w.root_ref); t.light0 = plights.empty() ? 0u : plights[0];
  t.n_wide = (uint32_t)L.nodes.size(); t.packed_depth = L.depth + w.medium_depth + 2u;  // (stack_dwords: 2 * L.depth + medium_depth + 2 with two dwords per group)
  for (int a = 0; a < 3; ++a) t.old_index[a] = L.old_of_new[a];
  return SOL_OK;
}
// What the kernels read of the tree the scene owns (s->tree): the ONE place that writes the tree-dependent fields of DevScene.
static void bind_tree(SolScene* s) {
  const DevTree& t = s->tree;
  DevScene& S = s->S;
  S.nodes = t.nodes.get(); S.wides = t.wides.get(); S.leaf_refs = t.leaf_refs.get(); S.tris = t.tris.get(); S.tri_shade = t.tri_shade.get();
  S.quads = t.quads.get(); S.spheres = t.spheres.get(); S.mediums = t.mediums.get(); S.lights = t.lights.get();
  S.light0 = t.light0; S.wroot = 0; S.wide_emin = t.emin; S.root = t.root;
}
static void adopt_build_info(SolScene* s, const DeviceSplitInfo& si) {  // what the chosen candidate's build did (a host-built tree: nothing)
  s->split_references = si.extra_references; s->split_triangles = si.split_triangles; s->split_area_ratio = si.area_ratio;
  s->reinsertion_moves = si.reinsertion_moves; s->reinsertion_area_ratio = si.area_before > 0. ? (float)(si.area_after / si.area_before) : 1.f;
}
// candidate 0's tree and what does not depend on the tree
static int upload_scene(const CreateCtx& c, const World& w, const HostRecords& r, SolScene* s, TreeCand& first) {
  const SolSceneDesc* d = &c.d;
  int rc;
  if ((rc = upload_tree(*d, w, r, first)) || (rc = sol_upload(r.mats, s->mats)) || (rc = sol_upload(r.texs, s->texs))) return rc;
  const std::vector<uint8_t> texels(d->texels, d->texels + d->n_texel_bytes);
  if ((rc = sol_upload(texels, s->texels))) return rc;
  HIP_TRY(sol_dev_alloc(s->work, 1));
  HIP_TRY(sol_dev_alloc(s->counters, 1));
  HIP_TRY(hipMemset(s->counters.get(), 0, sizeof(DevCounters)));
  HIP_TRY(sol_dev_alloc(s->image, (size_t)d->width * d->height * 3));
  HIP_TRY(sol_dev_alloc(s->rgb8, (size_t)d->width * d->height * 3));
  return SOL_OK;
}
// ... and the scene's constants: DevScene, the launch parameters the overrides set, the whole-image partition
static int set_scene_constants(const CreateCtx& c, const World& w, SolScene* s, TreeCand& first) {
  const SolSceneDesc* d = &c.d;
  const SolDevOverrides& ovr = c.ovr;
  const Box& root_box = w.root_box;
  int rc;
  DevScene& S = s->S;
  S.mats = s->mats.get(); S.texs = s->texs.get(); S.texels = s->texels.get();
  S.n_lights = d->n_lights;
  s->tree = std::move(first.dev);  // the scene takes ownership
  bind_tree(s);
  adopt_build_info(s, first.built);
  S.rxmin = root_box.v[0]; S.rxmax = root_box.v[1]; S.rymin = root_box.v[2]; S.rymax = root_box.v[3];
  S.rzmin = root_box.v[4]; S.rzmax = root_box.v[5];
  S.width = d->width; S.height = d->height; S.shader = d->shader_kind; S.max_depth = d->max_depth;
  S.sphere_slack = w.box_pad * 0.5f;
  if ((rc = sol_upload(light_triangle_frames(*d), s->light_tri))) return rc;
  S.light_tri = s->light_tri.get();
  S.tri_delta = w.needles ? w.box_pad * 0.8f : 0.0f;
  s->strict_triangles = S.tri_delta > 0.0f;
  S.env = nullptr; S.env_w = S.env_h = 0; S.env_scale = 1.0f;
  if (c.has_env) {
    std::vector<float> env(d->env_texels, d->env_texels + (size_t)d->env_width * d->env_height * 3);
    if ((rc = sol_upload(env, s->env))) return rc;
    S.env = s->env.get(); S.env_w = d->env_width; S.env_h = d->env_height; S.env_scale = (float)d->env_scale;
  }
  s->env_refusal = sol_env_refusal(d);  // (environment importance sampling, sol_envmap.hip: stops at the first cell of positive weight)
  s->light_w = sol_light_weights_of(d);  // (light sampling mode 2, sol_lights.hip: O(L), decided at creation like env_refusal)
  S.bgx = (float)d->background[0]; S.bgy = (float)d->background[1]; S.bgz = (float)d->background[2];
  S.cam = cast_camera(d->camera);
  s->kernel_version = ovr.kernel_version;
  s->pool_swap_min = (uint32_t)ovr.pool_swap_min;
  s->pool_count = ovr.pool_count;
  if (ovr.radiance_rows > 0) s->rad_partial_max_rows = (size_t)ovr.radiance_rows;
  if (ovr.gather_rows > 0) s->ga_max_rows = (size_t)ovr.gather_rows;
  if (ovr.lightmap_claim == 1) s->lm_small_max = 0xFFFFFFFFu;                                 // a lane per triangle
  if (ovr.lightmap_claim == 2) { s->lm_small_max = 0u; s->lm_tiles_max = 0xFFFFFFFFu; }        // a wave per triangle
  s->vol_load_all = ovr.volume_load_all;
  if (ovr.lightmap_filter) { s->lf_staged = ovr.lightmap_filter == 2; s->lf_fold = ovr.lightmap_filter == 3; }
  s->depth_project_plain = ovr.depth_project_plain;
  s->order_mode = ovr.order_mode;
  // v1's search/shade switch (RenderParams::switch_below), measured on MI355X at 1080p x 128 spp (ms, C1 / C2 / C3 / test scene):
  // 0: 29.2 / 162.9 / 236.7 / 25.9, 8: 27.7 / 124.3 / 193.1 / 25.5, 16: 27.5 / 111.8 / 186.9 / 25.6, 24: 28.6 / 108.6 / 192.3 / 26.8.
  s->switch_below = 16u;
  if (ovr.switch_below >= 0) s->switch_below = (uint32_t)ovr.switch_below;
  if (ovr.max_bpc >= 0) s->max_bpc = ovr.max_bpc;  // occupancy experiments
  s->pool_slots_override = (uint32_t)ovr.pool_slots;
  if (ovr.wf_slots > 0) s->wf_slots = (uint32_t)std::max(4096, ovr.wf_slots);
  if (ovr.fine_tail >= -1) s->fine_tail = ovr.fine_tail;
  if (ovr.wf_min_items >= 0) s->wf_min_items = (uint32_t)ovr.wf_min_items;
  s->has_medium = d->n_mediums > 0;
  s->blocks_x = (d->width + SOL_TILE - 1) / SOL_TILE;
  s->blocks_y = (d->height + SOL_TILE - 1) / SOL_TILE;
  if ((rc = sol_set_partition(s, 0, 1))) return rc;
  // a null table would be a GPU memory fault at the first launch, not an error code: refuse here
  const void* tables[] = {S.nodes, S.wides, S.leaf_refs, S.tris, S.tri_shade, S.quads, S.spheres, S.mediums, S.mats, S.texs, S.texels, S.lights};
  for (const void* p : tables)
    if (!p) return sol_fail(SOL_EDEVICE, "internal error: a device table of the scene is missing");
  s->tree_name = first.name;
  return SOL_OK;
}
// 10. Probe every candidate tree with a counted render of 16 samples per pixel over ~256 pixel blocks spread across the image
// and keep the one with the least search work (a wide-node visit weighs ~2.5 primitive tests, by instruction count).
// Images do not depend on the tree, the counters are deterministic, so is the choice. `chosen`: the candidate the scene keeps.
static int probe_candidates(const CreateCtx& c, const World& w, const HostRecords& r, SolScene* s, std::vector<TreeCand>& cands, size_t& chosen) {
  int rc;
  for (size_t k = 1; k < cands.size(); ++k)
    if ((rc = upload_tree(c.d, w, r, cands[k]))) return rc;
  const uint32_t nb = s->blocks_x * s->blocks_y;
  rc = sol_set_partition(s, 0, (int)std::max(1u, nb / 256u));
  size_t pick = 0, current = 0;  // `current`: the candidate whose arrays the scene holds at the moment
  auto swap_in = [&](size_t k) {  // hand the scene's tree back to its candidate, take candidate k's
    if (k == current) return;
    std::swap(s->tree, cands[current].dev);
    std::swap(s->tree, cands[k].dev);
    bind_tree(s);
    current = k;
  };
  for (size_t k = 0; k < cands.size() && !rc; ++k) {
    swap_in(k);
    if (!(rc = sol_clear(s)) && !(rc = sol_render_probe(s)))
      cands[k].cost = 2.5 * (double)s->stats.node_visits + (double)(s->stats.sphere_tests + s->stats.quad_tests + s->stats.triangle_tests);
    if (!rc && cands[k].cost < cands[pick].cost) pick = k;
  }
  if (c.ovr.verbose) {
    std::fprintf(stderr, "[solstrale] world tree probe:");
    for (auto& t : cands) std::fprintf(stderr, " %s %.4g (%zu nodes)", t.name.c_str(), t.cost, t.lay.nodes.size());
    std::fprintf(stderr, " -> %s\n", cands[pick].name.c_str());
  }
  if (hipStreamSynchronize(s->stream) != hipSuccess && !rc) rc = SOL_EDEVICE;
  swap_in(pick);
  chosen = pick;
  s->tree_name = cands[pick].name;
  adopt_build_info(s, cands[pick].built);
  for (auto& t : cands) t.dev.release();  // (the losers' arrays: not kept until the candidates go)
  if (rc) return rc;
  s->stats = SolStats{};
  if ((rc = sol_set_partition(s, 0, 1)) || (rc = sol_clear(s))) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}
// 10b. SolCreateOptions.dynamic_triangles: what sol_scene_set_triangles (sol_geometry.cpp) needs of this creation and cannot derive
// later - the caller's per-triangle constants, the unpadded fp32 boxes of the primitives that do not move, the chosen layout's nodes level by
// level (the layout is on the host here: no kernel), which records the world tree reaches (box_pad_for's S reads the ROOT's box, the union of
// exactly those), the camera's share of S - and the staging copies both kernels write.
template <typename T> static int dev_alloc(DevPtr<T>& p, size_t count) {
  HIP_TRY(sol_dev_alloc(p, count));
  HIP_TRY(hipMemset(p.get(), 0, std::max<size_t>(count * sizeof(T), 64)));
  return SOL_OK;
}
// SolCreateOptions.dynamic_primitives: what sol_scene_set_primitives needs on top - per sphere and quad what a move does not change
// and which caller primitive a device record holds, a second copy of every box array and of the sphere and quad records (staging: a refused
// call must leave the boxes the next partial move refits over as they were), the triangles' boxes and share of S as creation saw them (a
// first call may move the spheres alone), room for the host route's rows, and which sphere or quad each light is.
static int keep_dynamic_primitives(const CreateCtx& c, SolScene* s, const WideLayout& L, const std::vector<uint8_t> (&reached)[3], const std::vector<uint32_t>& rec_tri,
                                   const std::vector<float>& sbox, const std::vector<float>& qbox) {
  const SolSceneDesc& d = c.d;
  SolDynamic& y = s->dyn;
  std::vector<SolPrimStatic> sst(d.n_spheres), qst(d.n_quads);
  for (uint32_t i = 0; i < d.n_spheres; ++i) sst[i] = SolPrimStatic{d.spheres[i].material, d.spheres[i].dfs_index};
  for (uint32_t i = 0; i < d.n_quads; ++i) qst[i] = SolPrimStatic{d.quads[i].material, d.quads[i].dfs_index};
  std::vector<uint32_t> rec_sphere(y.n_spheres), rec_quad(y.n_quads);
  for (uint32_t i = 0; i < y.n_spheres; ++i) rec_sphere[i] = L.old_of_new[1][i] | (reached[1][i] ? 0u : SOL_DYN_OUTSIDE);
  for (uint32_t i = 0; i < y.n_quads; ++i) rec_quad[i] = L.old_of_new[2][i] | (reached[2][i] ? 0u : SOL_DYN_OUTSIDE);
  std::vector<float> tbox((size_t)y.n_recs * 8, 0.0f);
  float S = 0.0f;
  for (uint32_t i = 0; i < y.n_recs; ++i)
    for (int j = 0; j < 6; ++j) {
      const float v = (float)d.triangles[rec_tri[i] & ~SOL_DYN_OUTSIDE].bbox.v[j];
      tbox[(size_t)i * 8 + j] = v;
      const float a = std::fabs(v);
      if (!(rec_tri[i] & SOL_DYN_OUTSIDE) && std::isfinite(a) && a > S) S = a;
    }
  y.S_tri = S;
  y.needles = sol_scene_has_needles(&d) != 0;
  y.light_prim_host.assign(d.n_lights, 0u);
  for (uint32_t i = 0; i < d.n_lights; ++i) {
    const uint32_t k = SOL_REF_KIND(d.lights[i]);
    if (k == SOL_REF_SPHERE || k == SOL_REF_QUAD) y.light_prim_host[i] = d.lights[i];
  }
  int rc;
  if ((rc = sol_upload(sst, y.sphere_static)) || (rc = sol_upload(qst, y.quad_static)) || (rc = sol_upload(rec_sphere, y.rec_sphere)) ||
      (rc = sol_upload(rec_quad, y.rec_quad)) || (rc = sol_upload(tbox, y.tri_box)) || (rc = sol_upload(tbox, y.tri_box2)) ||
      (rc = sol_upload(sbox, y.sphere_box2)) || (rc = sol_upload(qbox, y.quad_box2)) || (rc = sol_upload(y.light_prim_host, y.light_prim)) ||
      (rc = dev_alloc(y.spheres2, y.n_spheres)) || (rc = dev_alloc(y.quads2, y.n_quads)) || (rc = dev_alloc(y.sphere_rows, (size_t)y.n_spheres * 4)) ||
      (rc = dev_alloc(y.quad_rows, (size_t)y.n_quads * 9)) || (rc = dev_alloc(y.out, 4 + 2 * (size_t)d.n_lights + 2)))
    return rc;
  y.primitives = true;
  return SOL_OK;
}
static int keep_dynamic(const CreateCtx& c, const HostRecords& r, SolScene* s, const TreeCand& cand) {
  const SolSceneDesc& d = c.d;
  const WideLayout& L = cand.lay;
  SolDynamic& y = s->dyn;
  y.n_tris = d.n_triangles; y.n_recs = (uint32_t)L.old_of_new[0].size();
  y.n_spheres = (uint32_t)r.spheres.size(); y.n_quads = (uint32_t)r.quads.size(); y.n_leaf_refs = (uint32_t)L.leaf_refs.size();
  std::vector<SolTriStatic> st(d.n_triangles);
  for (uint32_t i = 0; i < d.n_triangles; ++i) {
    const SolTriangle& t = d.triangles[i];
    st[i] = SolTriStatic{{t.uv0[0], t.uv0[1], t.uv1[0], t.uv1[1], t.uv2[0], t.uv2[1]}, t.material, t.dfs_index};
  }
  // the levels of the layout, and which device records it reaches
  std::vector<uint8_t> reached[3];
  for (int a = 0; a < 3; ++a) reached[a].assign(L.old_of_new[a].size(), 0);
  std::vector<uint32_t> level_nodes, level{0u}, next;
  y.level_off.assign(1, 0u);
  const uint32_t ref_kind_of[4] = {SOL_REF_NONE, SOL_REF_TRIANGLE, SOL_REF_SPHERE, SOL_REF_QUAD};
  while (!level.empty()) {
    if (y.level_off.size() > 4096u || level_nodes.size() + level.size() > L.nodes.size()) return sol_fail(SOL_EDEVICE, "dynamic_triangles: the tree layout is not a tree");
    next.clear();
    for (uint32_t ni : level) {
      if (ni >= L.nodes.size()) return sol_fail(SOL_EDEVICE, "dynamic_triangles: node index out of range");
      level_nodes.push_back(ni);
      const WideView v(L.nodes[ni], cand.emin);
      for (int sl = 0; sl < SOL_WIDE_CHILDREN; ++sl) {
        if (v.inner(sl)) { next.push_back(v.inner_index(sl)); continue; }
        if (!v.leaf(sl)) continue;
        const uint32_t idx = v.prim_index(sl);
        uint32_t ref = SOL_MAKE_REF(ref_kind_of[v.kind], idx);
        if (v.kind == SOL_LEAF_REFS) { if (idx >= L.leaf_refs.size()) return sol_fail(SOL_EDEVICE, "dynamic_triangles: listed reference out of range"); ref = L.leaf_refs[idx]; }
        const int a = WideLayout::arr(SOL_REF_KIND(ref));
        if (a < 0) continue;  // (a constant medium: sol_scene_set_triangles refuses such a scene)
        if (SOL_REF_INDEX(ref) >= reached[a].size()) return sol_fail(SOL_EDEVICE, "dynamic_triangles: a leaf reference out of range");
        reached[a][SOL_REF_INDEX(ref)] = 1;
      }
    }
    y.level_off.push_back((uint32_t)level_nodes.size());
    level.swap(next);
  }
  if (level_nodes.size() != L.nodes.size()) return sol_fail(SOL_EDEVICE, "dynamic_triangles: unreachable wide nodes");
  std::vector<uint32_t> rec_tri(y.n_recs);
  for (uint32_t i = 0; i < y.n_recs; ++i) rec_tri[i] = L.old_of_new[0][i] | (reached[0][i] ? 0u : SOL_DYN_OUTSIDE);
  float S = 0.0f;
  auto take = [&](double v) { const float a = std::fabs((float)v); if (std::isfinite(a) && a > S) S = a; };  // (box_pad_for's)
  std::vector<float> sbox(r.spheres.size() * 6), qbox(r.quads.size() * 6);
  // the unpadded fp32 boxes of one kind in device order, and that kind's share of S (over the records the tree reaches)
  auto share = [&](int a, std::vector<float>& box) {
    S = 0.0f;
    for (size_t i = 0; i < box.size() / 6; ++i)
      for (int j = 0; j < 6; ++j) {
        const uint32_t o = L.old_of_new[a][i];
        const double v = a == 1 ? d.spheres[o].bbox.v[j] : d.quads[o].bbox.v[j];
        box[i * 6 + j] = (float)v;
        if (reached[a][i]) take(v);
      }
    return S;
  };
  y.S_sphere = share(1, sbox);
  y.S_quad = share(2, qbox);
  S = 0.0f;
  for (int j = 0; j < 3; ++j) take(d.camera.origin[j]);
  y.cam_S = S;
  y.light_src_host.assign(d.n_lights, 0xFFFFFFFFu);
  for (uint32_t i = 0; i < d.n_lights; ++i)
    if (SOL_REF_KIND(d.lights[i]) == SOL_REF_TRIANGLE) y.light_src_host[i] = SOL_REF_INDEX(d.lights[i]);
  y.light_lum = sol_light_luminances_of(&d);
  int rc;
  if ((rc = sol_upload(st, y.tri_static)) || (rc = sol_upload(rec_tri, y.rec_tri)) || (rc = sol_upload(sbox, y.sphere_box)) || (rc = sol_upload(qbox, y.quad_box)) ||
      (rc = sol_upload(level_nodes, y.level_nodes)) || (rc = sol_upload(y.light_src_host, y.light_src)) || (rc = sol_upload(light_triangle_frames(d), y.light_tri2)) ||
      (rc = dev_alloc(y.tri_box, (size_t)y.n_recs * 8)) || (rc = dev_alloc(y.node_box, L.nodes.size() * 6)) || (rc = dev_alloc(y.wides2, L.nodes.size())) ||
      (rc = dev_alloc(y.tris2, y.n_recs)) || (rc = dev_alloc(y.shade2, y.n_recs)) || (rc = dev_alloc(y.verts, (size_t)y.n_tris * 9)) ||
      (rc = dev_alloc(y.out, 4 + 2 * (size_t)d.n_lights)))
    return rc;
  y.on = true;
  return c.opt.dynamic_primitives ? keep_dynamic_primitives(c, s, L, reached, rec_tri, sbox, qbox) : SOL_OK;
}
// 11. Background blocks: constant background only (an environment map is looked up per ray). The proof is host work (0.06 s for C5 at 1080p): it
// runs on a thread of its own beside the cost probe's render and is adopted after it (the probe traces every block either way).
struct BackgroundProof {
  std::future<void> job; std::vector<uint8_t> block; uint32_t n = 0, pixels = 0;
  void start(const TreeCand& t, const DCamera& cam, uint32_t width, uint32_t height, double margin) {
    auto prove = [this, &t, cam, width, height, margin]() { find_background_blocks(t.lay, t.emin, cam, width, height, margin, block, n, pixels); };
    try { job = std::async(std::launch::async, prove); }
    catch (const std::system_error&) { prove(); job = std::async(std::launch::deferred, []() {}); }  // (no thread to be had: proved here, adopted as usual)
  }
  int adopt(SolScene* s, bool verbose) {  // (waits for the proof; idempotent)
    if (!job.valid()) return SOL_OK;
    job.get();
    s->background_block = std::move(block); s->n_background = n; s->background_pixels = pixels;
    if (verbose) std::fprintf(stderr, "[solstrale] background blocks: %u of %u (%u pixels)\n", s->n_background, s->blocks_x * s->blocks_y, s->background_pixels);
    if (s->n_background == 0) { s->background_block.clear(); return SOL_OK; }
    return sol_rebuild_order(s);  // (also without the cost probe)
  }
  ~BackgroundProof() { if (job.valid()) job.wait(); }  // (an early return must not leave the thread behind)
};
// Cost probe: per 8x8 block, the ray count of the longest 4-sample item in a counted render of the whole frame, for the
// heavy-first work order (rebuild_order; sol_path.h decode_item_ordered). SOL_ORDER=0 switches it off.
// Two halves, so that creation can adopt its host proof between them and a camera move's SOL_CAMERA_REPROBE (sol_camera.cpp) can run both:
// sol_cost_probe_render makes the counted render into the probe's device tables, sol_cost_probe_adopt takes the render's status `rc`, frees
// the tables and, where all went well, adopts the costs.
int sol_cost_probe_render(SolScene* s, SolCostProbe& p) {
  const uint32_t nb = s->blocks_x * s->blocks_y;
  HIP_TRY(sol_dev_alloc(p.cost_dev, nb));
  hipError_t e = hipMemset(p.cost_dev.get(), 0, (size_t)nb * sizeof(uint32_t));
  if (e == hipSuccess) e = sol_dev_alloc(p.work_dev, nb);
  if (e == hipSuccess) e = hipMemset(p.work_dev.get(), 0, (size_t)nb * sizeof(uint32_t));
  if (e != hipSuccess) return SOL_EDEVICE;
  SolRenderJob job = sol_render_job(s, 0, 4, 0xC057ull, true);  // the scene with the probe's tables: only this launch records into them
  job.view.block_cost = p.cost_dev.get();
  job.view.block_work = p.work_dev.get();
  return sol_render_impl(s, job);
}
int sol_cost_probe_adopt(SolScene* s, SolCostProbe& p, int rc, bool verbose) {
  const uint32_t nb = s->blocks_x * s->blocks_y;
  const SolCostProbe tables = std::move(p);  // (freed on every way out; p is empty again)
  uint32_t* const cost_dev = tables.cost_dev.get(); uint32_t* const work_dev = tables.work_dev.get();
  if (!cost_dev) return rc;  // (the render half failed before it had a table)
  s->block_cost.assign(nb, 0u);
  s->block_work.assign(nb, 0u);
  if (rc == SOL_OK && hipMemcpy(s->block_work.data(), work_dev, (size_t)nb * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) rc = SOL_EDEVICE;
  if (rc == SOL_OK && hipMemcpy(s->block_cost.data(), cost_dev, (size_t)nb * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) rc = SOL_EDEVICE;
  if (rc != SOL_OK) return rc == SOL_EDEVICE ? sol_fail(SOL_EDEVICE, "cost probe failed") : rc;
  // The fine tail takes an item fetch per SAMPLE (a dependent load, three integer divisions: ~2 us): worth it where a sample
  // is long. MI355X, 1080p x 64 spp, ms with 0 / 1 / 2 whole items per lane in the tail: C3 (38 node visits per sample) 76.5 /
  // 75.5 / 74.4, C2 (22) 45.5 / 45.7 / 46.3, C1 (2) 10.5 / 11.2 / 11.8.
  // Round 5, re-measured on the round-4 trees and kernel (profiles/r05_fine_tail_sweep.txt; 64 spp, ms with a tail of 0 / 2 / 4 / 8 / 16 whole
  // items per lane): C1 (2 node visits per sample) 9.09 / 9.07 / 9.66 / 9.74 / 9.65, test scene (8) 9.75 / 8.33 / 8.39 / 8.28 / 8.16, C5 (12) 37.9 /
  // 38.2 / 38.8 / 38.2 / 38.3, C2 (19) 33.7 / 32.5 / 31.5 / 31.4 / 31.3, C3 (36) 62.5 / 60.5 / 60.5 / 60.6 / 60.6: the per-sample fetch no longer
  // costs what it did (the reservoir, the work order), a short launch of long paths gains most. By the probe's node visits per sample:
  // below 5 none, 15 .. 30 eight whole items per lane, else two.
  if (s->stats.samples > 0) {
    const double vps = (double)s->stats.node_visits / (double)s->stats.samples;
    s->fine_tail_auto = vps < 5.0 ? 0 : (vps >= 15.0 && vps < 30.0) ? 32 : 8;
  }
  s->stats = SolStats{};
  if ((rc = sol_clear(s)) || (rc = sol_rebuild_order(s))) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (verbose) std::fprintf(stderr, "[solstrale] work order: %u of %u blocks heavy (first)\n", s->S.n_first, s->n_local_blocks);
  return SOL_OK;
}

extern "C" {

// The struct has no size field of its own and grew in round 4 (the three split counters): the plain entry point keeps writing the FIRST
// LAYOUT (through leaf_area, SOL_TREE_CHECK_V1_BYTES) so that a binding compiled against that header is not overrun; callers of this
// header pass their struct's size to sol_world_tree_check_ex and get every field that fits.
int sol_world_tree_check_ex(const SolSceneDesc* d, int use_sah, void* out, size_t out_size) {
  if (!out || out_size < SOL_TREE_CHECK_V1_BYTES) return sol_fail(SOL_EINVAL, "sol_world_tree_check_ex: out is null or smaller than the first layout (%d bytes)", (int)SOL_TREE_CHECK_V1_BYTES);
  SolTreeCheck full{};  // (zero where world_tree_check refuses before filling it)
  const int rc = world_tree_check(d, use_sah, &full);
  std::memset(out, 0, out_size);
  std::memcpy(out, &full, std::min(out_size, sizeof full));
  return rc;
}
int sol_world_tree_check(const SolSceneDesc* d, int use_sah, SolTreeCheck* out) { return sol_world_tree_check_ex(d, use_sah, out, SOL_TREE_CHECK_V1_BYTES); }

// Diagnostic, host only: the background blocks sol_scene_create would find with the host-built tree `use_sah` names (as in
// sol_world_tree_check; the proof does not depend on which tree carries it, the count may).
int sol_background_blocks(const SolSceneDesc* d, int use_sah, uint8_t* flags, size_t n_flags, uint32_t* n_found) {
  if (!d || !n_found || use_sah < 0) return sol_fail(SOL_EINVAL, "bad argument");
  *n_found = 0;
  if (d->width < 2 || d->height < 2 || (uint64_t)d->width * d->height > 0x3FFFFFFFull) return sol_fail(SOL_EINVAL, "bad image size %ux%u", d->width, d->height);
  const uint32_t nb = ((d->width + SOL_TILE - 1) / SOL_TILE) * ((d->height + SOL_TILE - 1) / SOL_TILE);
  if (flags && n_flags < nb) return sol_fail(SOL_EINVAL, "%zu flags for %u blocks", n_flags, nb);
  const SolDevOverrides ovr = sol_dev_overrides();
  World w(*d);
  HostTree tree;
  if (int rc = diag_world(*d, use_sah, ovr, w, tree, nullptr)) return rc;
  std::vector<uint8_t> f(nb, 0);
  uint32_t pixels = 0;
  if (!has_environment(*d)) find_background_blocks(tree.lay, tree.emin, cast_camera(d->camera), d->width, d->height, 64.0 * (double)w.box_pad, f, *n_found, pixels);
  if (flags) std::memcpy(flags, f.data(), nb);
  return SOL_OK;
}

int sol_scene_create(const SolSceneDesc* d, int device, SolScene** out) { return sol_scene_create_ex(d, device, nullptr, out); }

int sol_scene_create_ex(const SolSceneDesc* d, int device, const SolCreateOptions* opt_in, SolScene** out) {
  if (!d || !out) return sol_fail(SOL_EINVAL, "null argument");
  *out = nullptr;
  CreateCtx c{*d, sol_dev_overrides()};
  int rc;
  if ((rc = check_options_and_header(c, opt_in))) return rc;
  HostRecords rec;
  if ((rc = cast_materials(d, rec)) || (rc = cast_primitives(d, rec))) return rc;
  c.say("records cast");
  World world(*d);
  if ((rc = resolve_world(c, world, rec))) return rc;
  std::vector<TreeCand> cands;  // candidate 0: the provisional choice
  // AUTO = the device build: as good a tree as the probed host candidates (node visits per ray, host probe / device: C2 11.0 /
  // 10.9, C3 12.8 / 13.0, C5 6.8 / 6.9) in a sixth to an eighth of the time (sol_scene_create, C3: 0.40 s -> 0.06 s, C5 2.2 s -> 0.3 s)
  static const char* const tree_names[] = {"device", "ref", "sah8", "sah16", "sah64", "device", ""};
  std::string want = !c.ovr.bvh.empty() ? c.ovr.bvh : tree_names[c.opt.world_tree];  // (SOL_BVH: developer override of SolCreateOptions.world_tree)
  if (want == "host") want = "";  // all host candidates + the probe
  if (want != "device" && (rc = host_candidates(c, world, want, cands))) return rc;
  const double t_host_trees = seconds_since(c.t_begin);
  c.say("host part done");
  if ((rc = check_lights(d, rec))) return rc;
  ScenePtr scene;
  std::chrono::steady_clock::time_point t_upload0;
  if ((rc = open_device(device, scene, t_upload0))) return rc;
  SolScene* s = scene.get();
  s->build_times[0] = t_host_trees;
  if (want == "device" && (rc = device_candidates(c, world, rec.tris, s, cands))) return rc;
  if ((rc = upload_scene(c, world, rec, s, cands[0]))) return rc;
  s->build_times[1] = seconds_since(t_upload0) - s->build_times[2];
  const auto t_probe0 = std::chrono::steady_clock::now();
  if ((rc = set_scene_constants(c, world, s, cands[0]))) return rc;
  size_t chosen = 0;
  if (cands.size() > 1 && (rc = probe_candidates(c, world, rec, s, cands, chosen))) return rc;
  if (c.opt.dynamic_triangles && (rc = keep_dynamic(c, rec, s, cands[chosen]))) return rc;
  BackgroundProof proof;  // (after `cands`: it reads the chosen candidate's layout until it is joined)
  // (what a later sol_scene_set_camera must know of this creation: sol_camera.cpp)
  s->box_pad = world.box_pad;
  s->background_proof = !c.opt.no_background_blocks && c.ovr.background_blocks != 0 && !c.has_env;
  s->cost_probe = !c.opt.no_work_order_probe && c.ovr.order_mode != 0;
  s->verbose = c.ovr.verbose;
  if (s->background_proof) proof.start(cands[chosen], s->S.cam, d->width, d->height, 64.0 * (double)world.box_pad);
  if (s->cost_probe && s->blocks_x * s->blocks_y >= 64u) {
    SolCostProbe probe;
    rc = sol_cost_probe_render(s, probe);
    if (int rb = proof.adopt(s, c.ovr.verbose)) { if (rc == SOL_OK) rc = rb; }  // (beside the render; before the costs, whose order puts the background blocks last)
    if ((rc = sol_cost_probe_adopt(s, probe, rc, c.ovr.verbose))) return rc;
  }
  if ((rc = proof.adopt(s, c.ovr.verbose))) return rc;  // (no cost probe ran: the proof is adopted here)
  s->build_times[3] = seconds_since(t_probe0);
  *out = scene.release();
  return SOL_OK;
}

int sol_scene_build_times(const SolScene* s, double out[4]) {
  if (!s || !out) return sol_fail(SOL_EINVAL, "null argument");
  for (int k = 0; k < 4; ++k) out[k] = s->build_times[k];
  return SOL_OK;
}

}  // extern "C"
