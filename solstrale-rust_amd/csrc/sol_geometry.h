// sol_geometry.h -- what sol_geometry.cpp and the kernels of sol_geometry.hip share (sol_scene_set_triangles, sol_scene_set_primitives).
#pragma once
#include <hip/hip_runtime.h>

#include "sol_scene.h"

// flag bits a refit launch may raise in SolRefitParams::flags
#define SOL_REFIT_RANGE 1u    // a node's extent needs an exponent above emin + 31: the call is refused with SOL_ERANGE
#define SOL_REFIT_OPENED 2u   // a child box was opened fully on an axis (k_emit's fallback; cannot happen inside the exponent range)
#define SOL_REFIT_CORRUPT 8u  // an index of the tree leaves its array: nothing is read or written there, the call fails with SOL_EDEVICE

struct SolRefitParams {
  const DWide* cur;             // the tree the handle walks: topology, slots, masks, base indices
  DWide* out;                   // staging
  const uint32_t* leaf_refs;
  const float* tri_box;         // [n_recs][8]
  const float* sphere_box;      // [n_spheres][6]
  const float* quad_box;        // [n_quads][6]
  float* node_box;              // [n_wide][6]
  const uint32_t* level_nodes;
  uint32_t* flags;
  float pad;
  uint32_t emin, n_wide, n_recs, n_spheres, n_quads, n_leaf_refs;
};

// out: word 0 bit 0 a vertex is not finite, 1 a needle triangle, 2 the bits of the largest |fp32 box coordinate| of the records the tree reaches
hipError_t sol_launch_triangle_records(const double* verts, const SolTriStatic* st, const uint32_t* rec_tri, uint32_t n_recs, uint32_t n_tris, DTri* tris,
                                       DTriShade* shade, float* tri_box, uint32_t* out, hipStream_t stream);
hipError_t sol_launch_triangle_lights(const double* verts, const SolTriStatic* st, const uint32_t* light_src, uint32_t n_lights, uint32_t n_tris, DTri* light_tri,
                                      double* area, hipStream_t stream);
// one level of the refit: nodes level_nodes[first .. first + count), eight lanes per node
hipError_t sol_launch_refit_level(const SolRefitParams& P, uint32_t first, uint32_t count, hipStream_t stream);
// Spheres and quads. rows: the caller's [n][4] (centre, radius) / [n][9] (q, u, v) in device memory; rec: the caller's index of every
// device record, SOL_DYN_OUTSIDE or-ed in. Records and unpadded fp32 boxes ([n_recs][6]) go to staging; flags: bit 1 (a sphere) / bit 2 (a quad) of the
// word is set where a parameter is not finite; s_bits: the bits of the largest |fp32 box coordinate| of the records the tree reaches.
hipError_t sol_launch_sphere_records(const double* rows, const SolPrimStatic* st, const uint32_t* rec, uint32_t n_recs, uint32_t n_rows, DSphere* spheres,
                                     float* box, uint32_t* flags, uint32_t* s_bits, hipStream_t stream);
hipError_t sol_launch_quad_records(const double* rows, const SolPrimStatic* st, const uint32_t* rec, uint32_t n_recs, uint32_t n_rows, DQuad* quads,
                                   float* box, uint32_t* flags, uint32_t* s_bits, hipStream_t stream);
// the f64 areas of the lights that are spheres or quads of a kind with rows (a null pointer: that kind is not moved, its entries are left alone)
hipError_t sol_launch_primitive_lights(const double* sphere_rows, const double* quad_rows, const uint32_t* light_prim, uint32_t n_lights, uint32_t n_spheres,
                                       uint32_t n_quads, double* area, hipStream_t stream);
