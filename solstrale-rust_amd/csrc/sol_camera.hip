// sol_camera.hip -- the background-block proof of a camera move (sol_scene_set_camera, sol_camera.cpp).
//
// sol_background_proof_kernel is find_background_blocks (sol_create.cpp: the argument is in the comment there) for a tree that is already on
// the device: one thread per 8x8 block, the per-camera scalars computed on the host (sol_camera.h) and passed by value, the per-block part
// - corner points, candidate planes, the walk over the DWide nodes - in f64 and in the host function's order of operations, so that both
// flag the same blocks of the same tree (tests/test_gpu_set_camera.py holds them together). A frame of 1080p has 32 400 blocks, less than
// one wave per SIMD, and every walk is a short chain of dependent 64-byte loads: one wave per workgroup, spread over all CUs.
//
// The planes live in registers (the loops over them are unrolled; a pinhole camera has 5 candidates, a lens 17 - two instantiations).
// The walk's stack is in LDS: where the host pushes every inner child that is not culled, this one keeps ONE entry per level - the
// node's first inner child (24 bits) and the set of its inner children still to visit (7 bits) - and takes them from the highest slot
// down, which is the host's order of visits. A tree of n levels needs n - 1 entries; PROOF_STACK = 256 covers every tree a scene can be
// created with (it needs 2 x levels + 2 <= SOL_LDS_STACK + SOL_SPILL_STACK = 512 dwords of traversal stack: at most 255 levels). A walk that would overflow it, like
// one that runs into the cap of 4096 visits or leaves the node array, ends as "reached": the block is traced, never flagged.
#include <hip/hip_runtime.h>

#include "sol_camera.h"
#include "sol_launch.h"

#define PROOF_WAVE 64
#define PROOF_STACK 256
static_assert((SOL_LDS_STACK + SOL_SPILL_STACK - 2) / 2 - 1 <= PROOF_STACK, "the proof's stack must hold every tree the render kernel's holds");

namespace {
struct V3 { double x, y, z; };
__device__ __forceinline__ double dot3(const V3& a, const V3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross3(const V3& a, const V3& b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 sub3(const V3& a, const V3& b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 vec3(const double v[3]) { return V3{v[0], v[1], v[2]}; }
__device__ __forceinline__ double max_std(double a, double b) { return a < b ? b : a; }  // std::max / std::min, operand for operand
__device__ __forceinline__ double min_std(double a, double b) { return b < a ? b : a; }
}  // namespace

// NL: corners of the lens (1: a pinhole, the eye; 4: the square around the lens disc)
template <int NL>
__global__ __launch_bounds__(PROOF_WAVE) void sol_background_proof_kernel(const DWide* __restrict__ wides, uint32_t n_wide, uint32_t emin, SolProofCamera C,
                                                                          uint8_t* __restrict__ flags) {
  constexpr int NP = 4 * NL + 1;
  __shared__ uint32_t stack[PROOF_STACK * PROOF_WAVE];  // entry e of lane l at [e * 64 + l]: a lane's entries never share a bank with another's
  const uint32_t lane = threadIdx.x;
  const uint32_t b = blockIdx.x * PROOF_WAVE + lane;
  if (b >= C.bx_n * C.by_n) return;
  const uint32_t by = b / C.bx_n, bx = b - by * C.bx_n;
  const uint32_t width = C.width, height = C.height;
  const uint32_t x0 = bx * SOL_TILE, x1 = min(x0 + SOL_TILE, width), y0 = by * SOL_TILE, y1 = min(y0 + SOL_TILE, height);
  const V3 org = vec3(C.org), ll = vec3(C.ll), hh = vec3(C.hh), vv = vec3(C.vv);
  // generate_path: u = (px + r) / (W - 1), v = ((H - 1 - py) + r) / (H - 1), r in [0, 1); `grow` pixels of margin on every side
  V3 T[4], Tw[4];
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const double grow = w == 0 ? C.grow : C.grow + 1.0;
    const double u0 = ((double)x0 - grow) / (double)(width - 1), u1 = ((double)x1 + grow) / (double)(width - 1);
    const double v0 = ((double)height - (double)y1 - grow) / (double)(height - 1), v1 = ((double)height - (double)y0 + grow) / (double)(height - 1);
    const double cu[4] = {u0, u1, u1, u0}, cv[4] = {v0, v0, v1, v1};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const V3 t{ll.x + hh.x * cu[k] + vv.x * cv[k], ll.y + hh.y * cu[k] + vv.y * cv[k], ll.z + hh.z * cu[k] + vv.z * cv[k]};
      if (w == 0) T[k] = t; else Tw[k] = t;
    }
  }
  // candidate p is valid (bit p of `valid`) if every ray of the block provably stays in n . x <= a; the host compacts them, here they keep
  // their places (the `outside` test asks whether ANY valid plane has the box on its outer side: the order does not matter)
  V3 pn[NP];
  double pa[NP];
  uint32_t valid = 0;
  auto offer = [&](int p, V3 n) {
    pn[p] = n; pa[p] = 0.;
    const double len = sqrt(dot3(n, n));
    if (!(len > 0.) || !isfinite(len)) return;
    double a = -1e300, bb = -1e300;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const V3 Lj = vec3(C.lens[j]);
      a = max_std(a, dot3(n, Lj));
#pragma unroll
      for (int k = 0; k < 4; ++k) bb = max_std(bb, dot3(n, sub3(T[k], Lj)));
    }
    if (bb <= 0.) { pa[p] = a; valid |= 1u << p; }
  };
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const V3 Lj = NL == 1 ? org : vec3(C.lens_wide[j]);
      V3 n = cross3(sub3(Tw[(k + 1) & 3], Tw[k]), sub3(Tw[k], Lj));
      if (dot3(n, sub3(Tw[(k + 2) & 3], Lj)) > 0.) n = V3{-n.x, -n.y, -n.z};  // the rectangle's far side is inside
      offer(k * NL + j, n);
    }
  {
    const V3 c{T[0].x + T[1].x + T[2].x + T[3].x - 4. * org.x, T[0].y + T[1].y + T[2].y + T[3].y - 4. * org.y, T[0].z + T[1].z + T[2].z + T[3].z - 4. * org.z};
    offer(NP - 1, V3{-c.x, -c.y, -c.z});  // what lies behind the camera
  }
  if (valid == 0) { flags[b] = 0; return; }
  const double margin = C.margin;
  bool reached = false;
  uint32_t visits = 0, sp = 0, ni = 0;
  for (;;) {
    if (ni >= n_wide || ++visits > 4096u) { reached = true; break; }
    // the node as WideView reads it (sol_tree.h; the render kernel's decode, sol_trace.h): exponents over emin, masks, plane bytes
    const uint4* src = reinterpret_cast<const uint4*>(wides + ni);
    const uint4 w0 = src[0], w1 = src[1], w2 = src[2], w3 = src[3];
    const float origin[3] = {__uint_as_float(w0.x), __uint_as_float(w0.y), __uint_as_float(w0.z)};
    const uint32_t meta = w0.w;
    const uint32_t q[12] = {w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w, w3.x, w3.y, w3.z, w3.w};
    const uint32_t imask = (meta >> 15) & 0x7Fu, lmask = (meta >> 22) & 0x7Fu;
    float scale[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) scale[a] = __uint_as_float((((meta >> (5 * a)) & 31u) + emin) << 23);
    const uint32_t base_inner = (q[1] >> 24) | ((q[3] >> 24) << 8) | ((q[5] >> 24) << 16);
    uint32_t pending = 0;  // bit r: the r-th inner child (node base_inner + r) is to be visited
#pragma unroll
    for (int sl = 0; sl < SOL_WIDE_CHILDREN; ++sl) {
      if (reached || !(((imask | lmask) >> sl) & 1u)) continue;
      double lo[3], hi[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const uint32_t ql = (q[2 * a + (sl >> 2)] >> (8 * (sl & 3))) & 0xFFu, qh = (q[6 + 2 * a + (sl >> 2)] >> (8 * (sl & 3))) & 0xFFu;
        const float flo = origin[a] + (float)ql * scale[a], fhi = origin[a] + (float)qh * scale[a];
        lo[a] = (double)flo - margin; hi[a] = (double)fhi + margin;
      }
      if (!(lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2])) { reached = true; continue; }  // (not a box: trace)
      // the least value of n . p over the box: > a = the whole box on the outer side of a valid plane
      bool outside = false;
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const double m = min_std(pn[p].x * lo[0], pn[p].x * hi[0]) + min_std(pn[p].y * lo[1], pn[p].y * hi[1]) + min_std(pn[p].z * lo[2], pn[p].z * hi[2]);
        outside = outside || (((valid >> p) & 1u) && m > pa[p]);
      }
      if (outside) continue;
      if ((lmask >> sl) & 1u) { reached = true; continue; }
      pending |= 1u << __popc(imask & ((1u << sl) - 1u));
    }
    if (reached) break;
    if (pending) {
      if (sp >= PROOF_STACK) { reached = true; break; }
      stack[sp * PROOF_WAVE + lane] = base_inner | (pending << 24);
      ++sp;
    }
    if (sp == 0) break;
    const uint32_t e = stack[(sp - 1) * PROOF_WAVE + lane];
    const uint32_t r = 31u - (uint32_t)__clz((int)(e >> 24));  // the highest slot first, as the host's stack hands them out
    ni = (e & 0x00FFFFFFu) + r;
    const uint32_t rest = e & ~(1u << (24 + r));
    if (rest >> 24) stack[(sp - 1) * PROOF_WAVE + lane] = rest; else --sp;
  }
  flags[b] = reached ? 0 : 1;
}

hipError_t sol_launch_background_proof(const DWide* wides, uint32_t n_wide, uint32_t emin, const SolProofCamera& cam, uint8_t* flags, hipStream_t stream) {
  const uint32_t nb = cam.bx_n * cam.by_n;
  if (nb == 0) return hipSuccess;
  const dim3 grid((nb + PROOF_WAVE - 1) / PROOF_WAVE), block(PROOF_WAVE);
  if (cam.n_lens == 1) hipLaunchKernelGGL(sol_background_proof_kernel<1>, grid, block, 0, stream, wides, n_wide, emin, cam, flags);
  else hipLaunchKernelGGL(sol_background_proof_kernel<4>, grid, block, 0, stream, wides, n_wide, emin, cam, flags);
  return hipGetLastError();
}
