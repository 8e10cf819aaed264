// sol_geometry.cpp -- sol_scene_set_triangles: new vertices for the triangles of a live scene (include/solstrale_hip.h). The device
// computes every triangle record again and refits the boxes of the tree the handle walks (kernels: sol_geometry.hip; what creation keeps for this:
// keep_dynamic, sol_create.cpp); the host derives what creation derives from the scene's extent - the box pad, the needle rule, the root box, the
// light weights - and ends as a camera move ends (sol_rederive_view_tables, sol_camera.cpp). Also the CPU entry point sol_triangle_from_vertices.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sol_geometry.h"
#include "sol_triangle.h"

namespace {
int check_update(const SolScene* s, const double* vertices, uint32_t n, const SolGeometryUpdate* update, const char* fn, SolGeometryUpdate& u) {
  u = SolGeometryUpdate{};
  if (update) {  // (first: what is wrong with the struct can be told without a handle)
    if (update->size < 8 || update->size > 4096) return sol_fail(SOL_EINVAL, "SolGeometryUpdate.size %u", update->size);
    std::memcpy(&u, update, std::min<size_t>(update->size, sizeof u));
  }
  if (u.flags & ~(SOL_GEOM_NO_BACKGROUND_PROOF | SOL_GEOM_REPROBE)) return sol_fail(SOL_EINVAL, "SolGeometryUpdate.flags 0x%x: unknown bits", u.flags);
  if (u.reserved[0] || u.reserved[1]) return sol_fail(SOL_EINVAL, "SolGeometryUpdate.reserved must be 0");
  if (!s || !vertices) return sol_fail(SOL_EINVAL, "%s: null %s", fn, !s ? "scene" : "vertices");
  if (!s->dyn.on) return sol_fail(SOL_EINVAL, "%s: the scene was created without SolCreateOptions.dynamic_triangles", fn);
  if (s->has_medium) return sol_fail(SOL_EINVAL, "%s: the scene has a constant medium - its boundary trees are not refitted", fn);
  if (n != s->dyn.n_tris) return sol_fail(SOL_EINVAL, "%s: %u rows of vertices for the scene's %u triangles", fn, n, s->dyn.n_tris);
  if ((u.flags & SOL_GEOM_REPROBE) && s->world > 1) return sol_fail(SOL_EINVAL, "SOL_GEOM_REPROBE: the cost probe renders the whole frame on one rank (world is %d)", s->world);
  return SOL_OK;
}

// `verts`: the vertices in device memory. Everything up to the commit writes staging buffers only.
int set_triangles(SolScene* s, const double* verts, const SolGeometryUpdate& u, bool uploaded) {
  SolDynamic& y = s->dyn;
  const bool timed = s->timing;
  if (timed)
    for (hipEvent_t& e : y.ev)
      if (!e) HIP_TRY(hipEventCreate(&e));
  if (timed && !uploaded) HIP_TRY(hipEventRecord(y.ev[0], s->stream));  // (the host route recorded it in front of its copy)
  if (timed) HIP_TRY(hipEventRecord(y.ev[1], s->stream));
  const uint32_t n_lights = s->S.n_lights;
  uint32_t* const out = y.out.get();
  double* const area_dev = reinterpret_cast<double*>(out + 4);
  HIP_TRY(hipMemsetAsync(out, 0, 16, s->stream));
  HIP_TRY(sol_launch_triangle_records(verts, y.tri_static.get(), y.rec_tri.get(), y.n_recs, y.n_tris, y.tris2.get(), y.shade2.get(), y.tri_box.get(), out, s->stream));
  HIP_TRY(sol_launch_triangle_lights(verts, y.tri_static.get(), y.light_src.get(), n_lights, y.n_tris, y.light_tri2, area_dev, s->stream));
  if (timed) HIP_TRY(hipEventRecord(y.ev[2], s->stream));
  std::vector<uint32_t> got(4 + 2 * (size_t)n_lights);
  HIP_TRY(hipMemcpyAsync(got.data(), out, got.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (got[0]) return sol_fail(SOL_EINVAL, "sol_scene_set_triangles: a vertex is not finite");
  // box_pad_for (sol_tree.h) on the moved scene: the root's box is the union of the reached primitives' boxes; the camera's share as creation saw it
  const bool needles = got[1] != 0;
  float S_tri;
  std::memcpy(&S_tri, &got[2], 4);
  float S = 0.0f;
  for (float a : {S_tri, y.static_S, y.cam_S})
    if (std::isfinite(a) && a > S) S = a;
  const float box_pad = S * ((needles ? SOL_NEEDLE_PAD : 1.0f) / 1048576.0f);
  if (!std::isfinite(S_tri) || !(box_pad * 1048576.0f <= 2.7487791e11f))
    return sol_fail(SOL_EINVAL, "the scene's coordinates reach beyond 2^38 (%g): not supported by the fp32 search", std::isfinite(S_tri) ? (double)box_pad * 1048576.0 : (double)S_tri);
  // the refit: deepest level first
  SolRefitParams P{};
  P.cur = s->tree.wides.get(); P.out = y.wides2.get(); P.leaf_refs = s->tree.leaf_refs.get(); P.tri_box = y.tri_box.get(); P.sphere_box = y.sphere_box.get();
  P.quad_box = y.quad_box.get(); P.node_box = y.node_box.get(); P.level_nodes = y.level_nodes.get(); P.flags = out + 3; P.pad = box_pad; P.emin = s->tree.emin;
  P.n_wide = s->tree.n_wide; P.n_recs = y.n_recs; P.n_spheres = y.n_spheres; P.n_quads = y.n_quads; P.n_leaf_refs = y.n_leaf_refs;
  for (size_t l = y.level_off.size() - 1; l-- > 0;)
    HIP_TRY(sol_launch_refit_level(P, y.level_off[l], y.level_off[l + 1] - y.level_off[l], s->stream));
  if (timed) HIP_TRY(hipEventRecord(y.ev[3], s->stream));
  uint32_t refit_flags = 0;
  float root[6];
  HIP_TRY(hipMemcpyAsync(&refit_flags, out + 3, 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(root, y.node_box.get(), sizeof root, hipMemcpyDeviceToHost, s->stream));  // (node 0 is the root)
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (refit_flags & SOL_REFIT_CORRUPT) return sol_fail(SOL_EDEVICE, "sol_scene_set_triangles: internal error, an index of the tree leaves its array");
  if (refit_flags & SOL_REFIT_RANGE)
    return sol_fail(SOL_ERANGE, "sol_scene_set_triangles: a node's extent leaves the exponent range the tree was created with (emin %u + 31): re-create the scene", s->tree.emin);
  // ---- commit: the staging buffers become the scene's, the scene's the next call's staging ----
  std::swap(s->tree.wides, y.wides2); std::swap(s->tree.tris, y.tris2); std::swap(s->tree.tri_shade, y.shade2); std::swap(s->light_tri, y.light_tri2);
  DevScene& D = s->S;
  D.wides = s->tree.wides.get(); D.tris = s->tree.tris.get(); D.tri_shade = s->tree.tri_shade.get(); D.light_tri = s->light_tri;
  D.rxmin = root[0]; D.rxmax = root[1]; D.rymin = root[2]; D.rymax = root[3]; D.rzmin = root[4]; D.rzmax = root[5];
  s->box_pad = box_pad;
  D.sphere_slack = box_pad * 0.5f;
  D.tri_delta = needles ? box_pad * 0.8f : 0.0f;
  s->strict_triangles = D.tri_delta > 0.0f;
  // the light weights of the triangle lights (sol_light_weights_of: area x luminance), and what was built from them
  bool lights_moved = false;
  for (uint32_t i = 0; i < n_lights && i < s->light_w.size(); ++i) {
    if (y.light_src_host[i] == 0xFFFFFFFFu) continue;
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
  if ((rc = sol_rederive_view_tables(s, u.flags, "set_triangles"))) return rc;
  if (timed) {
    HIP_TRY(hipEventRecord(y.ev[4], s->stream));
    HIP_TRY(hipEventSynchronize(y.ev[4]));
    for (int k = 0; k < 4; ++k) HIP_TRY(hipEventElapsedTime(&y.last_ms[k], y.ev[k], y.ev[k + 1]));
  }
  return SOL_OK;
}
}  // namespace

extern "C" {

int sol_triangle_from_vertices(const double v[9], const float uv[6], SolTriangle* out) {
  if (!v || !uv || !out) return sol_fail(SOL_EINVAL, "sol_triangle_from_vertices: null %s", !v ? "vertices" : !uv ? "texture coordinates" : "triangle");
  sol_triangle_new(v, uv, out);
  return SOL_OK;
}

int sol_scene_set_triangles(SolScene* s, const double* vertices, uint32_t n, const SolGeometryUpdate* update) {
  SolGeometryUpdate u;
  if (int rc = check_update(s, vertices, n, update, "sol_scene_set_triangles", u)) return rc;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));  // a launch in flight reads the staging buffers' other halves and the scene record
  if (s->timing) {
    if (!s->dyn.ev[0]) HIP_TRY(hipEventCreate(&s->dyn.ev[0]));
    HIP_TRY(hipEventRecord(s->dyn.ev[0], s->stream));
  }
  HIP_TRY(hipMemcpyAsync(s->dyn.verts.get(), vertices, (size_t)n * 9 * sizeof(double), hipMemcpyHostToDevice, s->stream));
  return set_triangles(s, s->dyn.verts.get(), u, true);
}

int sol_scene_set_triangles_dev(SolScene* s, const double* vertices_dev, uint32_t n, const SolGeometryUpdate* update) {
  SolGeometryUpdate u;
  if (int rc = check_update(s, vertices_dev, n, update, "sol_scene_set_triangles_dev", u)) return rc;
  if ((uintptr_t)vertices_dev & 15u) return sol_fail(SOL_EINVAL, "sol_scene_set_triangles_dev: the vertices must be 16-byte aligned");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return set_triangles(s, vertices_dev, u, false);
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

}  // extern "C"
