// sol_geometry.cpp -- sol_scene_set_triangles and sol_scene_set_primitives: new vertices for the triangles, new centres and radii for the spheres,
// new corners and edges for the quads of a live scene (include/solstrale_hip.h). The device computes every record of the kinds a
// call moves again and refits the boxes of the tree the handle walks (kernels: sol_geometry.hip; what creation keeps for this: keep_dynamic,
// sol_create.cpp); the host derives what creation derives from the scene's extent - the box pad, the needle rule, the root box, the light weights -
// and ends as a camera move ends (sol_rederive_view_tables, sol_camera.cpp). One path serves all entry points: everything up to the commit writes
// staging buffers only, the commit swaps the records AND the box arrays of the moved kinds and remembers their shares of S, so that a refused
// call leaves nothing behind that a later partial move could read. Also the CPU entry points sol_triangle_from_vertices, sol_sphere_from_center
// and sol_quad_from_corner.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sol_geometry.h"
#include "sol_primitive.h"
#include "sol_triangle.h"

namespace {
// The rows of a call: per kind a pointer (null: not moved) and a count.
struct Rows { const double* p[3] = {nullptr, nullptr, nullptr}; uint32_t n[3] = {0, 0, 0}; };  // triangles, spheres, quads
const char* const kKindName[3] = {"triangles", "spheres", "quads"};
const uint32_t kRowDoubles[3] = {9, 4, 9};

int check_update_struct(const SolGeometryUpdate* update, SolGeometryUpdate& u) {
  u = SolGeometryUpdate{};
  if (update) {  // (first: what is wrong with the struct can be told without a handle)
    if (update->size < 8 || update->size > 4096) return sol_fail(SOL_EINVAL, "SolGeometryUpdate.size %u", update->size);
    std::memcpy(&u, update, std::min<size_t>(update->size, sizeof u));
  }
  if (u.flags & ~(SOL_GEOM_NO_BACKGROUND_PROOF | SOL_GEOM_REPROBE)) return sol_fail(SOL_EINVAL, "SolGeometryUpdate.flags 0x%x: unknown bits", u.flags);
  if (u.reserved[0] || u.reserved[1]) return sol_fail(SOL_EINVAL, "SolGeometryUpdate.reserved must be 0");
  return SOL_OK;
}
// What can be told of the handle and the rows before the device is touched (the caller has checked that some kind is given).
int check_rows(const SolScene* s, const Rows& r, const SolGeometryUpdate& u, const char* fn) {
  if (!s->dyn.on) return sol_fail(SOL_EINVAL, "%s: the scene was created without SolCreateOptions.dynamic_triangles", fn);
  if ((r.p[1] || r.p[2]) && !s->dyn.primitives)
    return sol_fail(SOL_EINVAL, "%s: the scene was created without SolCreateOptions.dynamic_primitives (its spheres and quads do not move)", fn);
  if (s->has_medium) return sol_fail(SOL_EINVAL, "%s: the scene has a constant medium - its boundary trees are not refitted", fn);
  const uint32_t have[3] = {s->dyn.n_tris, s->dyn.n_spheres, s->dyn.n_quads};
  for (int k = 0; k < 3; ++k)
    if (r.p[k] && r.n[k] != have[k])
      return sol_fail(SOL_EINVAL, k == 0 ? "%s: %u rows of vertices for the scene's %u %s" : "%s: %u rows for the scene's %u %s", fn, r.n[k], have[k], kKindName[k]);
  if ((u.flags & SOL_GEOM_REPROBE) && s->world > 1) return sol_fail(SOL_EINVAL, "SOL_GEOM_REPROBE: the cost probe renders the whole frame on one rank (world is %d)", s->world);
  return SOL_OK;
}

// `r`: the rows in device memory. Everything up to the commit writes staging buffers only.
int move_primitives(SolScene* s, const Rows& r, const SolGeometryUpdate& u, bool uploaded, const char* fn) {
  SolDynamic& y = s->dyn;
  const bool timed = s->timing;
  const bool mt = r.p[0] != nullptr, ms = r.p[1] != nullptr, mq = r.p[2] != nullptr;
  if (timed)
    for (hipEvent_t& e : y.ev)
      if (!e) HIP_TRY(hipEventCreate(&e));
  if (timed && !uploaded) HIP_TRY(hipEventRecord(y.ev[0], s->stream));  // (the host route recorded it in front of its copies)
  if (timed) HIP_TRY(hipEventRecord(y.ev[1], s->stream));
  const uint32_t n_lights = s->S.n_lights;
  uint32_t* const out = y.out.get();
  double* const area_dev = reinterpret_cast<double*>(out + 4);
  uint32_t* const s_prim = out + 4 + 2 * (size_t)n_lights;  // (dynamic_primitives: the spheres' and the quads' S bits)
  // A handle with dynamic_triangles alone moves all its triangles in every call: one box array serves it. With dynamic_primitives a kind may stay
  // where it is while another moves, so every box array has its staging twin.
  float* const tri_box_st = y.primitives ? y.tri_box2.get() : y.tri_box.get();
  HIP_TRY(hipMemsetAsync(out, 0, 16, s->stream));
  if (y.primitives) HIP_TRY(hipMemsetAsync(s_prim, 0, 8, s->stream));
  if (mt) {
    HIP_TRY(sol_launch_triangle_records(r.p[0], y.tri_static.get(), y.rec_tri.get(), y.n_recs, y.n_tris, y.tris2.get(), y.shade2.get(), tri_box_st, out, s->stream));
    HIP_TRY(sol_launch_triangle_lights(r.p[0], y.tri_static.get(), y.light_src.get(), n_lights, y.n_tris, y.light_tri2.get(), area_dev, s->stream));
  }
  if (ms) HIP_TRY(sol_launch_sphere_records(r.p[1], y.sphere_static.get(), y.rec_sphere.get(), y.n_spheres, y.n_spheres, y.spheres2.get(), y.sphere_box2.get(), out, s_prim, s->stream));
  if (mq) HIP_TRY(sol_launch_quad_records(r.p[2], y.quad_static.get(), y.rec_quad.get(), y.n_quads, y.n_quads, y.quads2.get(), y.quad_box2.get(), out, s_prim + 1, s->stream));
  if (ms || mq) HIP_TRY(sol_launch_primitive_lights(r.p[1], r.p[2], y.light_prim.get(), n_lights, y.n_spheres, y.n_quads, area_dev, s->stream));
  if (timed) HIP_TRY(hipEventRecord(y.ev[2], s->stream));
  std::vector<uint32_t> got(4 + 2 * (size_t)n_lights + (y.primitives ? 2 : 0));
  HIP_TRY(hipMemcpyAsync(got.data(), out, got.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (got[0]) return sol_fail(SOL_EINVAL, "%s: a %s is not finite", fn, (got[0] & 1u) ? "vertex" : (got[0] & 2u) ? "sphere's centre or radius" : "quad's corner or edge");
  // box_pad_for (sol_tree.h) on the moved scene: the root's box is the union of the reached primitives' boxes - the fresh shares of the kinds
  // this call moves, the remembered ones of the others; the camera's share as creation saw it
  const bool needles = mt ? got[1] != 0 : y.needles;
  float share[3] = {y.S_tri, y.S_sphere, y.S_quad};
  if (mt) std::memcpy(&share[0], &got[2], 4);
  if (ms) std::memcpy(&share[1], &got[4 + 2 * (size_t)n_lights], 4);
  if (mq) std::memcpy(&share[2], &got[5 + 2 * (size_t)n_lights], 4);
  float S = 0.0f;
  bool finite = true;
  for (float a : {share[0], share[1], share[2], y.cam_S}) {
    if (std::isfinite(a) && a > S) S = a;
    finite = finite && std::isfinite(a);
  }
  const float box_pad = S * ((needles ? SOL_NEEDLE_PAD : 1.0f) / 1048576.0f);
  if (!finite || !(box_pad * 1048576.0f <= 2.7487791e11f))
    return sol_fail(SOL_EINVAL, "the scene's coordinates reach beyond 2^38 (%g): not supported by the fp32 search", finite ? (double)box_pad * 1048576.0 : (double)INFINITY);
  // the refit: deepest level first, over the staged boxes of the moved kinds and the committed ones of the others
  SolRefitParams P{};
  P.cur = s->tree.wides.get(); P.out = y.wides2.get(); P.leaf_refs = s->tree.leaf_refs.get();
  P.tri_box = mt ? tri_box_st : y.tri_box.get(); P.sphere_box = ms ? y.sphere_box2.get() : y.sphere_box.get(); P.quad_box = mq ? y.quad_box2.get() : y.quad_box.get();
  P.node_box = y.node_box.get(); P.level_nodes = y.level_nodes.get(); P.flags = out + 3; P.pad = box_pad; P.emin = s->tree.emin;
  P.n_wide = s->tree.n_wide; P.n_recs = y.n_recs; P.n_spheres = y.n_spheres; P.n_quads = y.n_quads; P.n_leaf_refs = y.n_leaf_refs;
  for (size_t l = y.level_off.size() - 1; l-- > 0;)
    HIP_TRY(sol_launch_refit_level(P, y.level_off[l], y.level_off[l + 1] - y.level_off[l], s->stream));
  if (timed) HIP_TRY(hipEventRecord(y.ev[3], s->stream));
  uint32_t refit_flags = 0;
  float root[6];
  HIP_TRY(hipMemcpyAsync(&refit_flags, out + 3, 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(root, y.node_box.get(), sizeof root, hipMemcpyDeviceToHost, s->stream));  // (node 0 is the root)
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (refit_flags & SOL_REFIT_CORRUPT) return sol_fail(SOL_EDEVICE, "%s: internal error, an index of the tree leaves its array", fn);
  if (refit_flags & SOL_REFIT_RANGE)
    return sol_fail(SOL_ERANGE, "%s: a node's extent leaves the exponent range the tree was created with (emin %u + 31): re-create the scene", fn, s->tree.emin);
  // ---- commit: the staging buffers of the moved kinds become the scene's, the scene's the next call's staging ----
  DevScene& D = s->S;
  std::swap(s->tree.wides, y.wides2);
  D.wides = s->tree.wides.get();
  if (mt) {
    std::swap(s->tree.tris, y.tris2); std::swap(s->tree.tri_shade, y.shade2); std::swap(s->light_tri, y.light_tri2);
    if (y.primitives) std::swap(y.tri_box, y.tri_box2);
    D.tris = s->tree.tris.get(); D.tri_shade = s->tree.tri_shade.get(); D.light_tri = s->light_tri.get();
  }
  if (ms) { std::swap(s->tree.spheres, y.spheres2); std::swap(y.sphere_box, y.sphere_box2); D.spheres = s->tree.spheres.get(); }
  if (mq) { std::swap(s->tree.quads, y.quads2); std::swap(y.quad_box, y.quad_box2); D.quads = s->tree.quads.get(); }
  y.S_tri = share[0]; y.S_sphere = share[1]; y.S_quad = share[2]; y.needles = needles;
  D.rxmin = root[0]; D.rxmax = root[1]; D.rymin = root[2]; D.rymax = root[3]; D.rzmin = root[4]; D.rzmax = root[5];
  s->box_pad = box_pad;
  D.sphere_slack = box_pad * 0.5f;
  D.tri_delta = needles ? box_pad * 0.8f : 0.0f;
  s->strict_triangles = D.tri_delta > 0.0f;
  // the light weights of the moved lights (sol_light_weights_of: area x luminance), and what was built from them
  bool lights_moved = false;
  for (uint32_t i = 0; i < n_lights && i < s->light_w.size(); ++i) {
    const uint32_t pk = y.primitives ? SOL_REF_KIND(y.light_prim_host[i]) : SOL_REF_NONE;
    const bool moved = (mt && y.light_src_host[i] != 0xFFFFFFFFu) || (ms && pk == SOL_REF_SPHERE) || (mq && pk == SOL_REF_QUAD);
    if (!moved) continue;
    double area;
    std::memcpy(&area, &got[4 + 2 * (size_t)i], 8);
    const double v = area * y.light_lum[i];
    s->light_w[i] = (v > 0.0 && std::isfinite(v)) ? v : 0.0;
    lights_moved = true;
  }
  if (lights_moved) {
    s->light_total = 0.0;
    for (double x : s->light_w) s->light_total += x;
  }
  int rc;
  if ((rc = sol_light_rebuild(s))) return rc;  // (the tree's leaf boxes carry the pad and bound the records, whatever the lights are)
  if ((rc = sol_rederive_view_tables(s, u.flags, fn + 10))) return rc;  // (the name without "sol_scene_")
  if (timed) {
    HIP_TRY(hipEventRecord(y.ev[4], s->stream));
    HIP_TRY(hipEventSynchronize(y.ev[4]));
    for (int k = 0; k < 4; ++k) HIP_TRY(hipEventElapsedTime(&y.last_ms[k], y.ev[k], y.ev[k + 1]));
  }
  return SOL_OK;
}

// The host route: the rows of every kind given are copied into the handle's own device arrays.
int move_from_host(SolScene* s, Rows r, const SolGeometryUpdate& u, const char* fn) {
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));  // a launch in flight reads the staging buffers' other halves and the scene record
  if (s->timing) {
    if (!s->dyn.ev[0]) HIP_TRY(hipEventCreate(&s->dyn.ev[0]));
    HIP_TRY(hipEventRecord(s->dyn.ev[0], s->stream));
  }
  double* const dev[3] = {s->dyn.verts.get(), s->dyn.sphere_rows.get(), s->dyn.quad_rows.get()};
  for (int k = 0; k < 3; ++k) {
    if (!r.p[k]) continue;
    if (r.n[k]) HIP_TRY(hipMemcpyAsync(dev[k], r.p[k], (size_t)r.n[k] * kRowDoubles[k] * sizeof(double), hipMemcpyHostToDevice, s->stream));
    r.p[k] = dev[k];
  }
  return move_primitives(s, r, u, true, fn);
}
int move_from_device(SolScene* s, const Rows& r, const SolGeometryUpdate& u, const char* fn) {
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return move_primitives(s, r, u, false, fn);
}
}  // namespace

extern "C" {

int sol_triangle_from_vertices(const double v[9], const float uv[6], SolTriangle* out) {
  if (!v || !uv || !out) return sol_fail(SOL_EINVAL, "sol_triangle_from_vertices: null %s", !v ? "vertices" : !uv ? "texture coordinates" : "triangle");
  sol_triangle_new(v, uv, out);
  return SOL_OK;
}
int sol_sphere_from_center(const double center[3], double radius, SolSphere* out) {
  if (!center || !out) return sol_fail(SOL_EINVAL, "sol_sphere_from_center: null %s", !center ? "center" : "sphere");
  sol_sphere_new(center, radius, out);
  return SOL_OK;
}
int sol_quad_from_corner(const double q[3], const double u[3], const double v[3], SolQuad* out) {
  if (!q || !u || !v || !out) return sol_fail(SOL_EINVAL, "sol_quad_from_corner: null %s", !q ? "q" : !u ? "u" : !v ? "v" : "quad");
  sol_quad_new(q, u, v, out);
  return SOL_OK;
}

int sol_scene_set_triangles(SolScene* s, const double* vertices, uint32_t n, const SolGeometryUpdate* update) {
  SolGeometryUpdate u;
  Rows r;
  r.p[0] = vertices; r.n[0] = n;
  if (int rc = check_update_struct(update, u)) return rc;
  if (!s || !vertices) return sol_fail(SOL_EINVAL, "sol_scene_set_triangles: null %s", !s ? "scene" : "vertices");
  if (int rc = check_rows(s, r, u, "sol_scene_set_triangles")) return rc;
  return move_from_host(s, r, u, "sol_scene_set_triangles");
}

int sol_scene_set_triangles_dev(SolScene* s, const double* vertices_dev, uint32_t n, const SolGeometryUpdate* update) {
  SolGeometryUpdate u;
  Rows r;
  r.p[0] = vertices_dev; r.n[0] = n;
  if (int rc = check_update_struct(update, u)) return rc;
  if (!s || !vertices_dev) return sol_fail(SOL_EINVAL, "sol_scene_set_triangles_dev: null %s", !s ? "scene" : "vertices");
  if (int rc = check_rows(s, r, u, "sol_scene_set_triangles_dev")) return rc;
  if ((uintptr_t)vertices_dev & 15u) return sol_fail(SOL_EINVAL, "sol_scene_set_triangles_dev: the vertices must be 16-byte aligned");
  return move_from_device(s, r, u, "sol_scene_set_triangles_dev");
}

int sol_scene_set_primitives(SolScene* s, const SolPrimitiveSet* set, const SolGeometryUpdate* update) {
  const char* const fn = "sol_scene_set_primitives";
  SolPrimitiveSet p{};
  if (set) {  // (what is wrong with the struct can be told without a handle)
    if (set->size < 8 || set->size > 4096) return sol_fail(SOL_EINVAL, "SolPrimitiveSet.size %u", set->size);
    std::memcpy(&p, set, std::min<size_t>(set->size, sizeof p));
    if (p.flags & ~SOL_PRIMS_DEVICE) return sol_fail(SOL_EINVAL, "SolPrimitiveSet.flags 0x%x: unknown bits", p.flags);
    if (p.reserved[0] || p.reserved[1] || p.reserved[2]) return sol_fail(SOL_EINVAL, "SolPrimitiveSet.reserved must be 0");
  }
  Rows r;
  r.p[0] = p.triangles; r.p[1] = p.spheres; r.p[2] = p.quads;
  r.n[0] = p.n_triangles; r.n[1] = p.n_spheres; r.n[2] = p.n_quads;
  SolGeometryUpdate u;
  if (int rc = check_update_struct(update, u)) return rc;
  if (!s || !set) return sol_fail(SOL_EINVAL, "%s: null %s", fn, !s ? "scene" : "set");
  if (!r.p[0] && !r.p[1] && !r.p[2]) return sol_fail(SOL_EINVAL, "%s: null pointers for all three kinds (at least one kind must move)", fn);
  if (int rc = check_rows(s, r, u, fn)) return rc;
  if (p.flags & SOL_PRIMS_DEVICE) {
    for (int k = 0; k < 3; ++k)
      if ((uintptr_t)r.p[k] & 15u) return sol_fail(SOL_EINVAL, "%s: the device rows of the %s must be 16-byte aligned", fn, kKindName[k]);
    return move_from_device(s, r, u, fn);
  }
  return move_from_host(s, r, u, fn);
}

int sol_scene_set_triangles_ms(const SolScene* s, float ms[4]) {
  if (!s || !ms) return sol_fail(SOL_EINVAL, "sol_scene_set_triangles_ms: null argument");
  if (!s->dyn.ev[4]) return sol_fail(SOL_EINVAL, "sol_scene_set_triangles_ms: no timed call (sol_kernel_timing, then sol_scene_set_triangles)");
  for (int k = 0; k < 4; ++k) ms[k] = s->dyn.last_ms[k];
  return SOL_OK;
}

int sol_scene_triangle_records(SolScene* s, void* tris, void* shade, uint32_t* triangle_of, size_t capacity, uint32_t* n_records) {
  if (!s || !n_records) return sol_fail(SOL_EINVAL, "sol_scene_triangle_records: null %s", !s ? "scene" : "n_records");
  const size_t n = s->tree.old_index[0].size();
  *n_records = (uint32_t)n;
  if (!tris && !shade && !triangle_of) return SOL_OK;
  if (capacity < n) return sol_fail(SOL_EINVAL, "sol_scene_triangle_records: room for %zu of %zu records", capacity, n);
  if (triangle_of) std::memcpy(triangle_of, s->tree.old_index[0].data(), n * sizeof(uint32_t));
  if (!tris && !shade) return SOL_OK;
  HIP_TRY(hipSetDevice(s->device));
  if (tris) HIP_TRY(hipMemcpyAsync(tris, s->tree.tris.get(), n * sizeof(DTri), hipMemcpyDeviceToHost, s->stream));
  if (shade) HIP_TRY(hipMemcpyAsync(shade, s->tree.tri_shade.get(), n * sizeof(DTriShade), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}

int sol_scene_primitive_records(SolScene* s, int kind, void* records, uint32_t* index_of, size_t capacity, uint32_t* n_records) {
  if (!s || !n_records) return sol_fail(SOL_EINVAL, "sol_scene_primitive_records: null %s", !s ? "scene" : "n_records");
  if (kind != (int)SOL_REF_SPHERE && kind != (int)SOL_REF_QUAD) return sol_fail(SOL_EINVAL, "sol_scene_primitive_records: kind %d (SOL_REF_SPHERE or SOL_REF_QUAD)", kind);
  const bool sphere = kind == (int)SOL_REF_SPHERE;
  const std::vector<uint32_t>& of = s->tree.old_index[sphere ? 1 : 2];
  const size_t n = of.size();
  *n_records = (uint32_t)n;
  if (!records && !index_of) return SOL_OK;
  if (capacity < n) return sol_fail(SOL_EINVAL, "sol_scene_primitive_records: room for %zu of %zu records", capacity, n);
  if (index_of) std::memcpy(index_of, of.data(), n * sizeof(uint32_t));
  if (!records || n == 0) return SOL_OK;
  HIP_TRY(hipSetDevice(s->device));
  if (sphere) HIP_TRY(hipMemcpyAsync(records, s->tree.spheres.get(), n * sizeof(DSphere), hipMemcpyDeviceToHost, s->stream));
  else HIP_TRY(hipMemcpyAsync(records, s->tree.quads.get(), n * sizeof(DQuad), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}

}  // extern "C"
