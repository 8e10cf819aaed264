// sol_camera.hip -- the background-block proof of a camera move (sol_scene_set_camera, sol_camera.cpp).
//
// sol_background_proof_kernel runs sol_block_is_background (sol_proof.h: the proof, the argument in the comment there, and the code scene
// creation runs on the host) for a tree that is already on the device: one thread per 8x8 block, the per-camera scalars computed on the host
// and passed by value. A frame of 1080p has 32 400 blocks, less than one wave per SIMD, and every walk is a short chain of dependent 64-byte
// loads: one wave per workgroup, spread over all CUs.
//
// The planes live in registers (a pinhole camera has 5 candidates, a lens 17 - two instantiations). The walk's stack, one entry per level, is
// in LDS. PROOF_STACK = 256 covers every tree a scene can be created with (it needs 2 x levels + 2 <= SOL_LDS_STACK + SOL_SPILL_STACK = 512
// dwords of traversal stack: at most 255 levels, 254 entries).
#include <hip/hip_runtime.h>

#include "sol_camera.h"
#include "sol_launch.h"

#define PROOF_WAVE 64
#define PROOF_STACK 256
static_assert((SOL_LDS_STACK + SOL_SPILL_STACK - 2) / 2 - 1 <= PROOF_STACK, "the proof's stack must hold every tree the render kernel's holds");

namespace {
struct LaneStack {  // entry e of lane l at [e * 64 + l]: a lane's entries never share a bank with another's
  uint32_t* lane;
  __device__ __forceinline__ uint32_t& operator[](uint32_t e) const { return lane[e * PROOF_WAVE]; }
};
}  // namespace

template <int NL>
__global__ __launch_bounds__(PROOF_WAVE) void sol_background_proof_kernel(const DWide* __restrict__ wides, uint32_t n_wide, uint32_t emin, SolProofCamera C,
                                                                          uint8_t* __restrict__ flags) {
  __shared__ uint32_t stack[PROOF_STACK * PROOF_WAVE];
  const uint32_t b = blockIdx.x * PROOF_WAVE + threadIdx.x;
  if (b >= C.bx_n * C.by_n) return;
  const uint32_t by = b / C.bx_n;
  flags[b] = sol_block_is_background<NL>(wides, n_wide, emin, C, b - by * C.bx_n, by, LaneStack{stack + threadIdx.x}, PROOF_STACK) ? 1 : 0;
}

hipError_t sol_launch_background_proof(const DWide* wides, uint32_t n_wide, uint32_t emin, const SolProofCamera& cam, uint8_t* flags, hipStream_t stream) {
  const uint32_t nb = cam.bx_n * cam.by_n;
  if (nb == 0) return hipSuccess;
  const dim3 grid((nb + PROOF_WAVE - 1) / PROOF_WAVE), block(PROOF_WAVE);
  if (cam.n_lens == 1) hipLaunchKernelGGL(sol_background_proof_kernel<1>, grid, block, 0, stream, wides, n_wide, emin, cam, flags);
  else hipLaunchKernelGGL(sol_background_proof_kernel<4>, grid, block, 0, stream, wides, n_wide, emin, cam, flags);
  return hipGetLastError();
}
