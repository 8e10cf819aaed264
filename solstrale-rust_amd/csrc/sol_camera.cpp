// sol_camera.cpp -- sol_scene_set_camera: a new camera for a live scene (include/solstrale_hip.h). The tree, the tables, the
// options, the sampling modes and the partition stay; what creation derived from ITS camera is derived again or dropped: the background
// blocks (re-proved by sol_background_proof_kernel, sol_camera.hip, over the device tree), the cost probe's block costs, the sums.
#include <cstdio>
#include <cstring>
#include <vector>

#include "sol_camera.h"
#include "sol_scene.h"

namespace {
// The handle without a background table and without block costs: plain chunk-major order, which is no table at all (what sol_rebuild_order
// leaves when it has nothing to order by and nothing to put last). Host state only, set here field by field - it cannot fail -, so a call
// that fails later leaves the new camera with an empty table, never with the old one.
void drop_camera_tables(SolScene* s) {
  s->background_block.clear();
  s->n_background = 0; s->background_pixels = 0;
  s->block_cost.clear();
  s->S.block_order = nullptr; s->S.n_first = 0; s->n_background_local = 0;
}
// The flags the proof kernel wrote, adopted as creation adopts the host proof's (BackgroundProof::adopt, sol_create.cpp).
int adopt_flags(SolScene* s, std::vector<uint8_t>& flags, const char* who) {
  uint32_t n = 0, pixels = 0;
  const uint32_t width = s->S.width, height = s->S.height;
  for (uint32_t by = 0; by < s->blocks_y; ++by)
    for (uint32_t bx = 0; bx < s->blocks_x; ++bx) {
      uint8_t& f = flags[(size_t)by * s->blocks_x + bx];
      f = f ? 1 : 0;
      if (!f) continue;
      const uint32_t x0 = bx * SOL_TILE, x1 = std::min(x0 + SOL_TILE, width), y0 = by * SOL_TILE, y1 = std::min(y0 + SOL_TILE, height);
      n++;
      pixels += (x1 - x0) * (y1 - y0);
    }
  if (s->verbose) std::fprintf(stderr, "[solstrale] %s: background blocks: %u of %u (%u pixels)\n", who, n, s->blocks_x * s->blocks_y, pixels);
  if (n == 0) return SOL_OK;
  s->background_block = std::move(flags); s->n_background = n; s->background_pixels = pixels;
  return sol_rebuild_order(s);
}
}  // namespace

// The tail of a camera move and of a geometry move (sol_geometry.cpp): the caller has waited for the stream and changed the scene record.
// flags: SOL_CAMERA_NO_BACKGROUND_PROOF / SOL_CAMERA_REPROBE (= SOL_GEOM_*), checked by the caller.
int sol_rederive_view_tables(SolScene* s, uint32_t flags, const char* who) {
  const bool reprobe = (flags & SOL_CAMERA_REPROBE) != 0;
  s->adaptive.open = false;
  drop_camera_tables(s);
  HIP_TRY(hipMemsetAsync(s->acc, 0, s->acc_floats * sizeof(float), s->stream));
  int rc;
  if ((rc = sol_clear_aux(s))) return rc;
  // the proof, on the scene's stream (in front of the probe's render, as creation starts the host proof before its probe)
  const uint32_t nb = s->blocks_x * s->blocks_y;
  SolProofCamera pc;
  const bool prove = !(flags & SOL_CAMERA_NO_BACKGROUND_PROOF) && s->background_proof && s->tree.n_wide > 0 &&
                     sol_proof_camera(s->S.cam, s->S.width, s->S.height, 64.0 * (double)s->box_pad, pc);
  if (prove) {
    if ((rc = s->proof_flags.reserve(s->stream, nb))) return rc;
    if (s->timing) HIP_TRY(hipEventRecord(s->ev_start, s->stream));
    HIP_TRY(sol_launch_background_proof(s->S.wides, s->tree.n_wide, s->S.wide_emin, pc, s->proof_flags.get(), s->stream));
    if (s->timing) { HIP_TRY(hipEventRecord(s->ev_stop, s->stream)); s->timed_launches++; s->last_grid = (nb + 63u) / 64u; }
  }
  // the cost probe, where creation ran one (it traces every block: the table is still empty)
  if (reprobe && s->cost_probe && nb >= 64u) {
    SolCostProbe probe;
    rc = sol_cost_probe_render(s, probe);
    if ((rc = sol_cost_probe_adopt(s, probe, rc, s->verbose))) return rc;
  }
  if (prove) {
    std::vector<uint8_t> flags_host(nb);
    HIP_TRY(hipMemcpyAsync(flags_host.data(), s->proof_flags.get(), nb, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if ((rc = adopt_flags(s, flags_host, who))) { drop_camera_tables(s); return rc; }
  }
  if ((rc = sol_scene_to_device(s))) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SOL_OK;
}

extern "C" {

int sol_scene_set_camera(SolScene* s, const SolCamera* camera, const SolCameraUpdate* update) {
  if (!s || !camera) return sol_fail(SOL_EINVAL, "sol_scene_set_camera: null %s", !s ? "scene" : "camera");
  SolCameraUpdate u{};
  if (update) {
    if (update->size < 8 || update->size > 4096) return sol_fail(SOL_EINVAL, "SolCameraUpdate.size %u", update->size);
    std::memcpy(&u, update, std::min<size_t>(update->size, sizeof u));
  }
  if (u.flags & ~(SOL_CAMERA_NO_BACKGROUND_PROOF | SOL_CAMERA_REPROBE)) return sol_fail(SOL_EINVAL, "SolCameraUpdate.flags 0x%x: unknown bits", u.flags);
  if (u.reserved[0] || u.reserved[1]) return sol_fail(SOL_EINVAL, "SolCameraUpdate.reserved must be 0");
  if ((u.flags & SOL_CAMERA_REPROBE) && s->world > 1) return sol_fail(SOL_EINVAL, "SOL_CAMERA_REPROBE: the cost probe renders the whole frame on one rank (world is %d)", s->world);
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));  // a launch in flight reads the scene record and the work order
  s->S.cam = cast_camera(*camera);
  return sol_rederive_view_tables(s, u.flags, "set_camera");
}

int sol_scene_background_flags(const SolScene* s, uint8_t* flags, size_t n_flags, uint32_t* n_found) {
  if (!s || !n_found) return sol_fail(SOL_EINVAL, "sol_scene_background_flags: null %s", !s ? "scene" : "n_found");
  const size_t nb = (size_t)s->blocks_x * s->blocks_y;
  if (flags && n_flags < nb) return sol_fail(SOL_EINVAL, "%zu flags for %zu blocks", n_flags, nb);
  *n_found = s->n_background;
  if (flags) {
    std::memset(flags, 0, nb);
    if (!s->background_block.empty()) std::memcpy(flags, s->background_block.data(), std::min(nb, s->background_block.size()));
  }
  return SOL_OK;
}

}  // extern "C"
