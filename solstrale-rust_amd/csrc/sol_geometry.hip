// sol_geometry.hip -- the kernels of sol_scene_set_triangles and sol_scene_set_primitives (host side: sol_geometry.cpp).
//
// Records. One thread per device triangle record (a pre-split triangle has several, all copies of one): the caller's 72 bytes of vertices and
// the 32-byte row of what does not move (texture coordinates, material, dfs_index) go through sol_triangle_new (sol_triangle.h: the f64 code the
// CPU entry point sol_triangle_from_vertices runs) and the casts creation uses, and come out as the 48-byte intersect record in the rotated
// frame, the 64-byte shading record and the unpadded fp32 cast box (32 bytes), all stored as dwordx4. Three scene-wide facts are reduced by
// wave, then with one atomic per wave on words whose values order like unsigned integers: a vertex that is not finite, a needle triangle, and
// the largest |fp32 coordinate| over the boxes of the records the world tree reaches - which is the largest |coordinate| of their union, the
// root's box that creation's box_pad_for reads (bvh.rs:95,105: a node's box is the union of its children's): per axis the union is [min of the
// mins, max of the maxs]; a min that is not the least has its own max at or above it, and that max is at most the greatest, so no coordinate
// of any box exceeds max(|least min|, |greatest max|) in magnitude, and both of those are coordinates of some box.
// A second, small launch runs over the lights: a triangle light's sampling frame in the reference's vertex order and its f64 area.
//
// Refit. One launch per level of the tree, deepest first, over that level's nodes. A child's box is the record's unpadded box plus the scene's
// pad (a leaf, found as the render kernel finds it: base_prim or leaf_refs) or what the level below left in node_box (an inner node); from there
// it is the emission's arithmetic (sol_build.hip k_emit, sol_tree.h WideBuilder::build): the node's grid origin two more pads out, the three
// frexpf exponents clamped to [emin, emin + 31] (a larger one raises SOL_REFIT_RANGE), floor / ceil quantisation with the fix-ups under the
// device's own decode - the functions of sol_quant.h, which k_emit calls too. Masks, leaf kind, exponent origin and the slot-7 base bytes
// are copied: the topology does not change. Eight lanes per node: lane s loads and quantises child s, the union goes through three
// __shfl_xor steps, the plane bytes are packed across the lanes and four lanes store the node as dwordx4. (One thread per node was built
// and measured 2.4-3.1x slower over the refit launches, profiles/set_triangles_ab.txt; it is in the history, not in the library.)
// Spheres and quads. One thread per device record: the caller's row (32 / 72 bytes) through the record's caller index and the 8 bytes
// of what does not move go through sol_sphere_new / sol_quad_new (sol_primitive.h: the f64 code of the CPU entry points) and creation's casts; the
// record leaves as dwordx4 stores (2 / 5), the unpadded fp32 box as three dwordx2 (the refit reads these arrays with a stride of 24 bytes). The
// same reduction as the triangles': a parameter that is not finite, the largest |fp32 box coordinate| of the reached records. A third launch over
// the lights writes the f64 area (the quad's |u x v|, 4 pi r^2) of every light of a moved kind.
// Every kernel writes staging buffers only.
#include <hip/hip_runtime.h>

#include "sol_geometry.h"
#include "sol_primitive.h"
#include "sol_quant.h"
#include "sol_triangle.h"
#include "sol_wide.h"

namespace {

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, m));
  return v;
}

__device__ __forceinline__ void load_triangle(const double* __restrict__ verts, const SolTriStatic* __restrict__ st, uint32_t t, SolTriangle& T, bool& finite) {
  double v[9];
  const double* p = verts + (size_t)t * 9;
#pragma unroll
  for (int k = 0; k < 9; ++k) v[k] = p[k];
  const float4* q = reinterpret_cast<const float4*>(st + t);
  const float4 a = q[0], b = q[1];
  const float uv[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
  T.material = __float_as_int(b.z);
  T.dfs_index = __float_as_uint(b.w);
  finite = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) finite = finite && (fabs(v[k]) < __builtin_huge_val());  // (false for a NaN too)
  sol_triangle_new(v, uv, &T);
}

__global__ void __launch_bounds__(256) sol_triangle_records_kernel(const double* __restrict__ verts, const SolTriStatic* __restrict__ st, const uint32_t* __restrict__ rec_tri,
                                                                   uint32_t n_recs, uint32_t n_tris, DTri* __restrict__ tris, DTriShade* __restrict__ shade,
                                                                   float* __restrict__ tri_box, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool bad = false, needle = false;
  uint32_t s_bits = 0u;
  const uint32_t rt = i < n_recs ? rec_tri[i] : 0xFFFFFFFFu;
  const uint32_t t = rt & ~SOL_DYN_OUTSIDE;
  if (i < n_recs && t < n_tris) {
    SolTriangle T;
    bool finite;
    load_triangle(verts, st, t, T, finite);
    bad = !finite;
    needle = sol_triangle_is_needle(&T);
    union { DTri r; float4 q[3]; } ri;
    union { DTriShade r; float4 q[4]; } rs;
    int uo[3];
    sol_tri_cast(&T, false, &ri.r, uo);
    sol_tri_cast_shade(&T, uo, &rs.r);
    float bx[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) bx[k] = (float)T.bbox.v[k];
    if (!(rt & SOL_DYN_OUTSIDE)) {
#pragma unroll
      for (int k = 0; k < 6; ++k) s_bits = max(s_bits, __float_as_uint(fabsf(bx[k])));  // (a NaN's bits are the largest: refused as not finite anyway)
    }
    float4* td = reinterpret_cast<float4*>(tris + i);
    td[0] = ri.q[0]; td[1] = ri.q[1]; td[2] = ri.q[2];
    float4* sd = reinterpret_cast<float4*>(shade + i);
    sd[0] = rs.q[0]; sd[1] = rs.q[1]; sd[2] = rs.q[2]; sd[3] = rs.q[3];
    float4* bd = reinterpret_cast<float4*>(tri_box + (size_t)i * 8);
    bd[0] = make_float4(bx[0], bx[1], bx[2], bx[3]);
    bd[1] = make_float4(bx[4], bx[5], 0.f, 0.f);
  }
  // by wave first, then one atomic per wave and fact (every value is a non-negative float's bits or a flag: unsigned order)
  const bool any_bad = __ballot(bad) != 0ull, any_needle = __ballot(needle) != 0ull;
  s_bits = wave_max_u32(s_bits);
  if ((threadIdx.x & 63u) == 0u) {
    if (any_bad) atomicOr(&out[0], 1u);
    if (any_needle) atomicOr(&out[1], 1u);
    if (s_bits) atomicMax(&out[2], s_bits);
  }
}

__global__ void __launch_bounds__(64) sol_triangle_lights_kernel(const double* __restrict__ verts, const SolTriStatic* __restrict__ st, const uint32_t* __restrict__ light_src,
                                                                 uint32_t n_lights, uint32_t n_tris, DTri* __restrict__ light_tri, double* __restrict__ area) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n_lights) return;
  const uint32_t t = light_src[i];
  if (t >= n_tris) { area[i] = 0.0; return; }
  SolTriangle T;
  bool finite;
  load_triangle(verts, st, t, T, finite);
  union { DTri r; float4 q[3]; } ri;
  int uo[3];
  sol_tri_cast(&T, true, &ri.r, uo);
  float4* td = reinterpret_cast<float4*>(light_tri + i);
  td[0] = ri.q[0]; td[1] = ri.q[1]; td[2] = ri.q[2];
  area[i] = T.area;
}

// ---- spheres and quads ----
__device__ __forceinline__ bool all_finite(const double* v, int n) {
  bool f = true;
  for (int k = 0; k < n; ++k) f = f && (fabs(v[k]) < __builtin_huge_val());  // (false for a NaN too)
  return f;
}
// the end of a records kernel: by wave first, then one atomic per wave and fact
__device__ __forceinline__ void reduce_records(bool bad, uint32_t bad_bit, uint32_t s_bits, uint32_t* __restrict__ flags, uint32_t* __restrict__ s_out) {
  const bool any_bad = __ballot(bad) != 0ull;
  s_bits = wave_max_u32(s_bits);
  if ((threadIdx.x & 63u) == 0u) {
    if (any_bad) atomicOr(flags, bad_bit);
    if (s_bits) atomicMax(s_out, s_bits);
  }
}
__device__ __forceinline__ uint32_t store_box(const SolAabb& b, bool reached, float* __restrict__ dst) {
  float bx[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) bx[k] = (float)b.v[k];
  uint32_t s_bits = 0u;
  if (reached) {
#pragma unroll
    for (int k = 0; k < 6; ++k) s_bits = max(s_bits, __float_as_uint(fabsf(bx[k])));
  }
  float2* bd = reinterpret_cast<float2*>(dst);
  bd[0] = make_float2(bx[0], bx[1]); bd[1] = make_float2(bx[2], bx[3]); bd[2] = make_float2(bx[4], bx[5]);
  return s_bits;
}

__global__ void __launch_bounds__(256) sol_sphere_records_kernel(const double* __restrict__ rows, const SolPrimStatic* __restrict__ st, const uint32_t* __restrict__ rec,
                                                                 uint32_t n_recs, uint32_t n_rows, DSphere* __restrict__ spheres, float* __restrict__ box,
                                                                 uint32_t* __restrict__ flags, uint32_t* __restrict__ s_out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool bad = false;
  uint32_t s_bits = 0u;
  const uint32_t rs = i < n_recs ? rec[i] : 0xFFFFFFFFu;
  const uint32_t t = rs & ~SOL_DYN_OUTSIDE;
  if (i < n_recs && t < n_rows) {
    const double2* p = reinterpret_cast<const double2*>(rows + (size_t)t * 4);
    const double2 a = p[0], b = p[1];
    const double v[4] = {a.x, a.y, b.x, b.y};
    const SolPrimStatic c = st[t];
    SolSphere S;
    S.material = c.material; S.dfs_index = c.dfs_index;
    bad = !all_finite(v, 4);
    sol_sphere_new(v, v[3], &S);
    union { DSphere r; float4 q[2]; } o;
    sol_sphere_cast(&S, &o.r);
    float4* d = reinterpret_cast<float4*>(spheres + i);
    d[0] = o.q[0]; d[1] = o.q[1];
    s_bits = store_box(S.bbox, !(rs & SOL_DYN_OUTSIDE), box + (size_t)i * 6);
  }
  reduce_records(bad, 2u, s_bits, flags, s_out);
}

__global__ void __launch_bounds__(256) sol_quad_records_kernel(const double* __restrict__ rows, const SolPrimStatic* __restrict__ st, const uint32_t* __restrict__ rec,
                                                               uint32_t n_recs, uint32_t n_rows, DQuad* __restrict__ quads, float* __restrict__ box,
                                                               uint32_t* __restrict__ flags, uint32_t* __restrict__ s_out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool bad = false;
  uint32_t s_bits = 0u;
  const uint32_t rs = i < n_recs ? rec[i] : 0xFFFFFFFFu;
  const uint32_t t = rs & ~SOL_DYN_OUTSIDE;
  if (i < n_recs && t < n_rows) {
    double v[9];
    const double* p = rows + (size_t)t * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = p[k];
    const SolPrimStatic c = st[t];
    SolQuad Q;
    Q.material = c.material; Q.dfs_index = c.dfs_index;
    bad = !all_finite(v, 9);
    sol_quad_new(v, v + 3, v + 6, &Q);
    union { DQuad r; float4 q[5]; } o;
    sol_quad_cast(&Q, &o.r);
    float4* d = reinterpret_cast<float4*>(quads + i);
#pragma unroll
    for (int k = 0; k < 5; ++k) d[k] = o.q[k];
    s_bits = store_box(Q.bbox, !(rs & SOL_DYN_OUTSIDE), box + (size_t)i * 6);
  }
  reduce_records(bad, 4u, s_bits, flags, s_out);
}

__global__ void __launch_bounds__(64) sol_primitive_lights_kernel(const double* __restrict__ sphere_rows, const double* __restrict__ quad_rows,
                                                                  const uint32_t* __restrict__ light_prim, uint32_t n_lights, uint32_t n_spheres, uint32_t n_quads,
                                                                  double* __restrict__ area) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n_lights) return;
  const uint32_t ref = light_prim[i], kind = SOL_REF_KIND(ref), idx = SOL_REF_INDEX(ref);
  if (kind == SOL_REF_SPHERE && sphere_rows && idx < n_spheres) {
    const double r = sphere_rows[(size_t)idx * 4 + 3];
    area[i] = 4.0 * 3.14159265358979323846 * r * r;  // sol_light_weights_of's expression
  } else if (kind == SOL_REF_QUAD && quad_rows && idx < n_quads) {
    double v[9];
    const double* p = quad_rows + (size_t)idx * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = p[k];
    SolQuad Q;
    sol_quad_new(v, v + 3, v + 6, &Q);
    area[i] = Q.area;
  }
}

// ---- refit ----
struct Box6 { float lo[3], hi[3]; };

__device__ __forceinline__ Box6 empty_box6() {
  const float inf = __builtin_huge_valf();
  return Box6{{inf, inf, inf}, {-inf, -inf, -inf}};
}
// The padded fp32 box of the child in slot s of a node with `meta` and the two base indices; an empty box for an empty slot.
__device__ __forceinline__ Box6 child_box(const SolRefitParams& P, uint32_t meta, uint32_t base_inner, uint32_t base_prim, int s, uint32_t& flags) {
  const uint32_t imask = sol_wide_imask(meta), lmask = sol_wide_lmask(meta), kind = sol_wide_leaf_kind(meta);
  Box6 b = empty_box6();
  if ((imask >> s) & 1u) {
    const uint32_t ni = base_inner + sol_wide_rank(imask, s);
    if (ni >= P.n_wide) { flags |= SOL_REFIT_CORRUPT; return b; }
    const float* p = P.node_box + (size_t)ni * 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) { b.lo[a] = p[2 * a]; b.hi[a] = p[2 * a + 1]; }
    return b;
  }
  if (!((lmask >> s) & 1u)) return b;
  uint32_t idx = base_prim + sol_wide_rank(lmask, s), k = kind;
  if (kind == SOL_LEAF_REFS) {
    if (idx >= P.n_leaf_refs) { flags |= SOL_REFIT_CORRUPT; return b; }
    const uint32_t ref = P.leaf_refs[idx];
    const uint32_t rk = SOL_REF_KIND(ref);
    k = rk == SOL_REF_TRIANGLE ? SOL_LEAF_TRIANGLES : rk == SOL_REF_SPHERE ? SOL_LEAF_SPHERES : rk == SOL_REF_QUAD ? SOL_LEAF_QUADS : 0u;
    idx = SOL_REF_INDEX(ref);
  }
  const float* p = nullptr;
  if (k == SOL_LEAF_TRIANGLES && idx < P.n_recs) p = P.tri_box + (size_t)idx * 8;
  else if (k == SOL_LEAF_SPHERES && idx < P.n_spheres) p = P.sphere_box + (size_t)idx * 6;
  else if (k == SOL_LEAF_QUADS && idx < P.n_quads) p = P.quad_box + (size_t)idx * 6;
  if (!p) { flags |= SOL_REFIT_CORRUPT; return b; }
#pragma unroll
  for (int a = 0; a < 3; ++a) { b.lo[a] = p[2 * a] - P.pad; b.hi[a] = p[2 * a + 1] + P.pad; }  // cast_box (sol_tree.h)
  return b;
}
// The node's grid from the union of its children's boxes: origin two pads out, exponent and scale per axis (sol_quant.h, k_emit's own).
__device__ __forceinline__ void node_grid(const Box6& u, float pad, uint32_t emin, float lo[3], float hi[3], uint32_t eb[3], float scale[3], uint32_t& flags) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = u.lo[a] - 2.0f * pad; hi[a] = u.hi[a] + 2.0f * pad;
    bool over;
    eb[a] = sol_wide_axis_grid(lo[a], hi[a], emin, scale[a], over);
    if (over) flags |= SOL_REFIT_RANGE;
  }
}
// One axis of one child: the plane bytes that contain [bl - 2 pad, bh + 2 pad]; a bound that is not finite (a primitive whose fp32 box
// overflows: the host's WideBuilder::build makes the same substitution) takes the node's.
__device__ __forceinline__ void quantise_axis(float bl, float bh, float pad, float lo, float hi, float scale, uint32_t& ql, uint32_t& qh, uint32_t& flags) {
  float cl = bl - 2.0f * pad, chh = bh + 2.0f * pad;  // two more pads: the device evaluates the planes in t-space (sol_tree.h)
  if (!(fabsf(cl) < __builtin_huge_valf())) cl = lo;
  if (!(fabsf(chh) < __builtin_huge_valf())) chh = hi;
  if (!sol_wide_axis_quantise(cl, chh, lo, scale, ql, qh)) flags |= SOL_REFIT_OPENED;
}

// Eight lanes per node: lane s of the group is slot s (lane 7, the slot that does not exist, carries the base bytes)
__global__ void __launch_bounds__(64) sol_refit_level8_kernel(SolRefitParams P, uint32_t first, uint32_t count) {
  const uint32_t gi = blockIdx.x * 8u + (threadIdx.x >> 3);
  const int s = (int)(threadIdx.x & 7u);
  const bool live = gi < count;  // (whole groups: every shuffle below stays inside a group of eight)
  uint32_t ni = live ? P.level_nodes[first + gi] : 0u;
  uint32_t flags = 0u;
  if (live && ni >= P.n_wide) { flags |= SOL_REFIT_CORRUPT; ni = 0u; }
  const DWide* wp = P.cur + ni;
  const uint32_t meta = wp->meta;
  const uint32_t base_inner = sol_wide_base_inner(wp->q), base_prim = sol_wide_base_prim(wp->q);
  const uint32_t occupied = sol_wide_imask(meta) | sol_wide_lmask(meta);
  Box6 c = empty_box6();
  if (live && s < SOL_WIDE_CHILDREN) c = child_box(P, meta, base_inner, base_prim, s, flags);
  Box6 u;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    u.lo[a] = fabsf(c.lo[a]) < __builtin_huge_valf() ? c.lo[a] : __builtin_huge_valf();
    u.hi[a] = fabsf(c.hi[a]) < __builtin_huge_valf() ? c.hi[a] : -__builtin_huge_valf();
#pragma unroll
    for (int m = 1; m <= 4; m <<= 1) {
      u.lo[a] = fminf(u.lo[a], __shfl_xor(u.lo[a], m));
      u.hi[a] = fmaxf(u.hi[a], __shfl_xor(u.hi[a], m));
    }
  }
  float lo[3], hi[3], scale[3];
  uint32_t eb[3];
  node_grid(u, P.pad, P.emin, lo, hi, eb, scale, flags);
  // this lane's six plane bytes, in place in the word of its half of the slots
  uint32_t wl[3], wh[3];
  const int shift = 8 * (s & 3);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    uint32_t ql = 255u, qh = 0u;
    if (s < SOL_WIDE_CHILDREN && ((occupied >> s) & 1u)) quantise_axis(c.lo[a], c.hi[a], P.pad, lo[a], hi[a], scale[a], ql, qh, flags);
    wl[a] = ql << shift; wh[a] = qh << shift;
  }
  uint32_t qb[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // (the slot-7 bytes alone)
  sol_wide_set_bases(qb, base_inner, base_prim);
  if (s == 7) { wl[0] = qb[1]; wl[1] = qb[3]; wl[2] = qb[5]; wh[0] = qb[7]; wh[1] = qb[9]; wh[2] = qb[11]; }
  // packed across the four lanes of a half, then exchanged between the halves
  uint32_t ol[3], oh[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    wl[a] |= (uint32_t)__shfl_xor((int)wl[a], 1); wl[a] |= (uint32_t)__shfl_xor((int)wl[a], 2);
    wh[a] |= (uint32_t)__shfl_xor((int)wh[a], 1); wh[a] |= (uint32_t)__shfl_xor((int)wh[a], 2);
    ol[a] = (uint32_t)__shfl_xor((int)wl[a], 4); oh[a] = (uint32_t)__shfl_xor((int)wh[a], 4);
  }
  if (live && !(flags & SOL_REFIT_CORRUPT) && s < 4) {
    // (lanes 0 .. 3 hold the words of slots 0 .. 3 in w*, of slots 4 .. 7 in o*): q[2a] = wl[a], q[2a + 1] = ol[a], q[6 + 2a] = wh[a], q[7 + 2a] = oh[a]
    uint4 v;
    if (s == 0) v = make_uint4(__float_as_uint(lo[0]), __float_as_uint(lo[1]), __float_as_uint(lo[2]),
                               sol_wide_regrid_meta(meta, eb, P.emin));
    else if (s == 1) v = make_uint4(wl[0], ol[0], wl[1], ol[1]);
    else if (s == 2) v = make_uint4(wl[2], ol[2], wh[0], oh[0]);
    else v = make_uint4(wh[1], oh[1], wh[2], oh[2]);
    reinterpret_cast<uint4*>(P.out + ni)[s] = v;
    if (s < 3) {  // the union, for the level above
      float2* nb = reinterpret_cast<float2*>(P.node_box + (size_t)ni * 6);
      nb[s] = s == 0 ? make_float2(u.lo[0], u.hi[0]) : s == 1 ? make_float2(u.lo[1], u.hi[1]) : make_float2(u.lo[2], u.hi[2]);
    }
  }
  if (flags) atomicOr(P.flags, flags);
}

}  // namespace

hipError_t sol_launch_triangle_records(const double* verts, const SolTriStatic* st, const uint32_t* rec_tri, uint32_t n_recs, uint32_t n_tris, DTri* tris,
                                       DTriShade* shade, float* tri_box, uint32_t* out, hipStream_t stream) {
  if (n_recs == 0) return hipSuccess;
  hipLaunchKernelGGL(sol_triangle_records_kernel, dim3((n_recs + 255u) / 256u), dim3(256), 0, stream, verts, st, rec_tri, n_recs, n_tris, tris, shade, tri_box, out);
  return hipGetLastError();
}
hipError_t sol_launch_triangle_lights(const double* verts, const SolTriStatic* st, const uint32_t* light_src, uint32_t n_lights, uint32_t n_tris, DTri* light_tri,
                                      double* area, hipStream_t stream) {
  if (n_lights == 0) return hipSuccess;
  hipLaunchKernelGGL(sol_triangle_lights_kernel, dim3((n_lights + 63u) / 64u), dim3(64), 0, stream, verts, st, light_src, n_lights, n_tris, light_tri, area);
  return hipGetLastError();
}
hipError_t sol_launch_refit_level(const SolRefitParams& P, uint32_t first, uint32_t count, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(sol_refit_level8_kernel, dim3((count + 7u) / 8u), dim3(64), 0, stream, P, first, count);
  return hipGetLastError();
}
hipError_t sol_launch_sphere_records(const double* rows, const SolPrimStatic* st, const uint32_t* rec, uint32_t n_recs, uint32_t n_rows, DSphere* spheres,
                                     float* box, uint32_t* flags, uint32_t* s_bits, hipStream_t stream) {
  if (n_recs == 0) return hipSuccess;
  hipLaunchKernelGGL(sol_sphere_records_kernel, dim3((n_recs + 255u) / 256u), dim3(256), 0, stream, rows, st, rec, n_recs, n_rows, spheres, box, flags, s_bits);
  return hipGetLastError();
}
hipError_t sol_launch_quad_records(const double* rows, const SolPrimStatic* st, const uint32_t* rec, uint32_t n_recs, uint32_t n_rows, DQuad* quads,
                                   float* box, uint32_t* flags, uint32_t* s_bits, hipStream_t stream) {
  if (n_recs == 0) return hipSuccess;
  hipLaunchKernelGGL(sol_quad_records_kernel, dim3((n_recs + 255u) / 256u), dim3(256), 0, stream, rows, st, rec, n_recs, n_rows, quads, box, flags, s_bits);
  return hipGetLastError();
}
hipError_t sol_launch_primitive_lights(const double* sphere_rows, const double* quad_rows, const uint32_t* light_prim, uint32_t n_lights, uint32_t n_spheres,
                                       uint32_t n_quads, double* area, hipStream_t stream) {
  if (n_lights == 0 || (!sphere_rows && !quad_rows)) return hipSuccess;
  hipLaunchKernelGGL(sol_primitive_lights_kernel, dim3((n_lights + 63u) / 64u), dim3(64), 0, stream, sphere_rows, quad_rows, light_prim, n_lights, n_spheres, n_quads, area);
  return hipGetLastError();
}
