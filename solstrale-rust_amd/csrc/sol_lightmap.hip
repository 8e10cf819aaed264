// sol_lightmap.hip -- lightmap texel points and border dilation (sol_lightmap_points, sol_lightmap_dilate; sol_lightmap.cpp).
//
// The rasteriser is two passes over one rule (sol_lightmap.h). The CLAIM pass runs over triangles and the candidate texels of each and does one
// atomicMin on the texel's 32-bit owner word per claim: the result is the minimum of a set of keys and does not depend on scheduling. The EMIT
// pass runs one thread per texel, evaluates the rule again for the owner and writes the point row (two dwordx4) and the SolTexel (one).
//
// The claim pass is balanced by the size of a triangle's candidate box, in three kernels that hand work down through two lists in the scratch:
//   sol_lightmap_claim_small_kernel  one LANE per triangle. A box of at most `small_max` texels (16) is walked by the lane itself - a million
//                                    triangles smaller than a texel are a million lanes with a handful of tests each. A larger one is pushed
//                                    onto list 0.
//   sol_lightmap_claim_tiles_kernel  one WAVE per entry of list 0, a persistent grid striding over the list: the box in 8x8 texel tiles aligned
//                                    to the atlas, one tile per step, a lane per texel. A box of more than `tiles_max` tiles (64) is pushed
//                                    onto list 1.
//   sol_lightmap_claim_large_kernel  every wave of a persistent grid strides over the tiles of each entry of list 1: one triangle over a whole
//                                    4096 x 4096 atlas is 262 144 tiles spread over the device.
// The list lengths stay on the device (the next kernel reads them): no host round trip. small_max and tiles_max are parameters, so that the two
// plain candidates - a lane per triangle (small_max = 2^32 - 1), a wave per triangle (small_max = 0, tiles_max = 2^32 - 1) - are this code too;
// profiles/lightmap.txt has the three measured at both extremes. No float atomics; every store is a vector store.
#include <hip/hip_runtime.h>

#include "sol_launch.h"
#include "sol_lightmap.h"

#define LM_WG 256
#define LM_WAVES (LM_WG / 64)

namespace {
struct LmAtlas {
  uint32_t W, H, conservative;
  float tmin, tmax;
};

// triangle `g` of the caller's arrays and its candidate box; false: it claims nothing
DEV bool lm_triangle(const float* vertices, const float* normals, const float* uvs, uint32_t g, const LmAtlas& A, LmTri& t, uint32_t& i0, uint32_t& i1,
                     uint32_t& j0, uint32_t& j1) {
  if (!lm_setup(uvs + (size_t)g * 6, vertices + (size_t)g * 9, normals ? normals + (size_t)g * 9 : nullptr, (float)A.W, (float)A.H, t)) return false;
  return lm_range(t, A.W, A.H, i0, i1, j0, j1);
}
DEV void lm_claim(const LmTri& t, uint32_t g, uint32_t i, uint32_t j, const LmAtlas& A, uint32_t* owner) {
  const uint32_t c = lm_classify(t, i, j, A.conservative != 0u);
  if (c != 0u) atomicMin(owner + (size_t)j * A.W + i, lm_key(g, c));
}
// tiles `first`, `first + step`, .. of the box, a lane per texel of the 8x8 tile
DEV void lm_claim_tiles(const LmTri& t, uint32_t g, uint32_t i0, uint32_t i1, uint32_t j0, uint32_t j1, uint32_t tiles_x, uint32_t tiles, uint32_t first,
                        uint32_t step, uint32_t lane, const LmAtlas& A, uint32_t* owner) {
  for (uint64_t k = first; k < tiles; k += step) {
    const uint32_t ty = (uint32_t)k / tiles_x, tx = (uint32_t)k - ty * tiles_x;
    const uint32_t i = ((i0 >> 3) + tx) * 8u + (lane & 7u), j = ((j0 >> 3) + ty) * 8u + (lane >> 3);
    if (i >= i0 && i <= i1 && j >= j0 && j <= j1) lm_claim(t, g, i, j, A, owner);
  }
}
}  // namespace

__global__ __launch_bounds__(LM_WG) void sol_lightmap_claim_small_kernel(const float* __restrict__ vertices, const float* __restrict__ normals,
                                                                         const float* __restrict__ uvs, uint32_t n, LmAtlas A, uint32_t small_max,
                                                                         uint32_t* __restrict__ owner, uint32_t* __restrict__ ctr, uint32_t* __restrict__ list0) {
  const uint32_t g = blockIdx.x * LM_WG + threadIdx.x;
  if (g >= n) return;
  LmTri t;
  uint32_t i0, i1, j0, j1;
  if (!lm_triangle(vertices, normals, uvs, g, A, t, i0, i1, j0, j1)) return;
  if ((i1 - i0 + 1u) * (j1 - j0 + 1u) > small_max) {  // (at most 2^28 texels: no overflow)
    list0[atomicAdd(ctr, 1u)] = g;                   // (every triangle at most once: the list holds n)
    return;
  }
  for (uint32_t j = j0; j <= j1; ++j)
    for (uint32_t i = i0; i <= i1; ++i) lm_claim(t, g, i, j, A, owner);
}

__global__ __launch_bounds__(LM_WG) void sol_lightmap_claim_tiles_kernel(const float* __restrict__ vertices, const float* __restrict__ normals,
                                                                         const float* __restrict__ uvs, LmAtlas A, uint32_t tiles_max,
                                                                         uint32_t* __restrict__ owner, uint32_t* __restrict__ ctr,
                                                                         const uint32_t* __restrict__ list0, uint32_t* __restrict__ list1) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * LM_WAVES + (threadIdx.x >> 6)), n_waves = gridDim.x * LM_WAVES;
  const uint32_t count = ldg_u32(ctr);
  for (uint32_t e = wave; e < count; e += n_waves) {
    const uint32_t g = __builtin_amdgcn_readfirstlane(ldg_u32(list0 + e));
    LmTri t;
    uint32_t i0, i1, j0, j1;
    if (!lm_triangle(vertices, normals, uvs, g, A, t, i0, i1, j0, j1)) continue;
    const uint32_t tiles_x = (i1 >> 3) - (i0 >> 3) + 1u, tiles = tiles_x * ((j1 >> 3) - (j0 >> 3) + 1u);  // (at most 2048 x 2048)
    if (tiles > tiles_max) {
      if (lane == 0u) list1[atomicAdd(ctr + 1, 1u)] = g;
      continue;
    }
    lm_claim_tiles(t, g, i0, i1, j0, j1, tiles_x, tiles, 0u, 1u, lane, A, owner);
  }
}

__global__ __launch_bounds__(LM_WG) void sol_lightmap_claim_large_kernel(const float* __restrict__ vertices, const float* __restrict__ normals,
                                                                         const float* __restrict__ uvs, LmAtlas A, uint32_t* __restrict__ owner,
                                                                         const uint32_t* __restrict__ ctr, const uint32_t* __restrict__ list1) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * LM_WAVES + (threadIdx.x >> 6)), n_waves = gridDim.x * LM_WAVES;
  const uint32_t count = ldg_u32(ctr + 1);
  for (uint32_t e = 0; e < count; ++e) {
    const uint32_t g = __builtin_amdgcn_readfirstlane(ldg_u32(list1 + e));
    LmTri t;
    uint32_t i0, i1, j0, j1;
    if (!lm_triangle(vertices, normals, uvs, g, A, t, i0, i1, j0, j1)) continue;
    const uint32_t tiles_x = (i1 >> 3) - (i0 >> 3) + 1u, tiles = tiles_x * ((j1 >> 3) - (j0 >> 3) + 1u);
    lm_claim_tiles(t, g, i0, i1, j0, j1, tiles_x, tiles, wave, n_waves, lane, A, owner);
  }
}

__global__ __launch_bounds__(LM_WG) void sol_lightmap_emit_kernel(const float* __restrict__ vertices, const float* __restrict__ normals,
                                                                  const float* __restrict__ uvs, LmAtlas A, const uint32_t* __restrict__ owner,
                                                                  float* __restrict__ points, uint32_t* __restrict__ texels) {
  const uint32_t x = blockIdx.x * LM_WG + threadIdx.x;
  if (x >= A.W * A.H) return;
  const uint32_t key = ldg_u32(owner + x);
  sol_v4f r0 = {0.f, 0.f, 0.f, 0.f}, r1 = {0.f, 0.f, 0.f, 0.f};
  sol_v4u tx = {SOL_LM_EMPTY, 0u, 0u, 0u};
  if (key != SOL_LM_EMPTY) {
    const uint32_t g = key & ~SOL_LM_CONSERVATIVE_BIT, claim = (key & SOL_LM_CONSERVATIVE_BIT) ? 2u : 1u;
    const uint32_t j = x / A.W, i = x - j * A.W;
    const float* pos = vertices + (size_t)g * 9;
    const float* nrm = normals ? normals + (size_t)g * 9 : nullptr;
    LmTri t;
    lm_setup(uvs + (size_t)g * 6, pos, nrm, (float)A.W, (float)A.H, t);  // (true: the triangle claimed this texel)
    float row[8], b1, b2;
    lm_row(t, pos, nrm, i, j, claim, A.tmin, A.tmax, row, b1, b2);
    r0 = sol_v4f{row[0], row[1], row[2], row[3]};
    r1 = sol_v4f{row[4], row[5], row[6], row[7]};
    tx = sol_v4u{g, __float_as_uint(b1), __float_as_uint(b2), claim};
  }
  SOL_AS1 sol_v4f* p = (SOL_AS1 sol_v4f*)(points + (size_t)x * 8);
  p[0] = r0;
  p[1] = r1;
  *(SOL_AS1 sol_v4u*)(texels + (size_t)x * 4) = tx;
}

// ---- border dilation ----
// Pass 0: owned texels are copied whole, every other row is zero; cover[x] = the pass the texel was covered in (0: owned, 255: not yet).
__global__ __launch_bounds__(LM_WG) void sol_lightmap_dilate_begin_kernel(const uint32_t* __restrict__ texels, uint32_t n_texels, const uint32_t* __restrict__ values,
                                                                          uint32_t stride_words, uint32_t* __restrict__ out, uint8_t* __restrict__ cover) {
  const uint32_t x = blockIdx.x * LM_WG + threadIdx.x;
  if (x >= n_texels) return;
  const bool owned = ldg_u32(texels + (size_t)x * 4) != SOL_LM_EMPTY;
  const size_t at = (size_t)x * stride_words;
  for (uint32_t w = 0; w < stride_words; ++w) out[at + w] = owned ? ldg_u32(values + at + w) : 0u;
  cover[x] = owned ? 0u : 255u;
}
// Pass k >= 1: a texel uncovered at the pass's start with a covered neighbour gets, per channel, (0 + x + x ..) / (float)count over its covered
// neighbours in lm_di / lm_dj's order. It reads rows covered before this pass and writes rows that were not: no row is read and written at once.
__global__ __launch_bounds__(LM_WG) void sol_lightmap_dilate_pass_kernel(uint32_t W, uint32_t H, uint32_t channels, uint32_t stride_words, uint32_t pass,
                                                                         float* __restrict__ out, const uint8_t* __restrict__ cover_in,
                                                                         uint8_t* __restrict__ cover_out) {
  const uint32_t x = blockIdx.x * LM_WG + threadIdx.x;
  if (x >= W * H) return;
  const uint8_t mine = ldg_u8(cover_in + x);
  if (mine != 255u) { cover_out[x] = mine; return; }
  const uint32_t j = x / W, i = x - j * W;
  uint32_t mask = 0u, count = 0u;
  for (uint32_t k = 0; k < 8u; ++k) {
    const int ni = (int)i + lm_di(k), nj = (int)j + lm_dj(k);
    if (ni < 0 || nj < 0 || ni >= (int)W || nj >= (int)H) continue;
    if (ldg_u8(cover_in + (size_t)nj * W + ni) != 255u) { mask |= 1u << k; ++count; }
  }
  cover_out[x] = count ? (uint8_t)pass : (uint8_t)255u;
  if (!count) return;
  const float fcount = (float)count;
  for (uint32_t c = 0; c < channels; ++c) {
    float s = 0.0f;
    for (uint32_t k = 0; k < 8u; ++k)
      if (mask & (1u << k)) s = s + out[((size_t)((int)j + lm_dj(k)) * W + (size_t)((int)i + lm_di(k))) * stride_words + c];
    out[(size_t)x * stride_words + c] = s / fcount;
  }
}

// ---- launches (sol_launch.h) ----
hipError_t sol_launch_lightmap_points(const float* vertices, const float* normals, const float* uvs, uint32_t n, uint32_t W, uint32_t H, bool conservative,
                                      float tmin, float tmax, uint32_t small_max, uint32_t tiles_max, uint32_t* owner, uint32_t* ctr, uint32_t* list0,
                                      uint32_t* list1, uint32_t persistent_blocks, void* points, void* texels, hipStream_t stream) {
  const LmAtlas A{W, H, conservative ? 1u : 0u, tmin, tmax};
  if (n != 0u) {
    hipLaunchKernelGGL(sol_lightmap_claim_small_kernel, dim3((n + LM_WG - 1) / LM_WG), dim3(LM_WG), 0, stream, vertices, normals, uvs, n, A, small_max, owner, ctr,
                       list0);
    hipLaunchKernelGGL(sol_lightmap_claim_tiles_kernel, dim3(persistent_blocks), dim3(LM_WG), 0, stream, vertices, normals, uvs, A, tiles_max, owner, ctr,
                       (const uint32_t*)list0, list1);
    hipLaunchKernelGGL(sol_lightmap_claim_large_kernel, dim3(persistent_blocks), dim3(LM_WG), 0, stream, vertices, normals, uvs, A, owner, (const uint32_t*)ctr,
                       (const uint32_t*)list1);
  }
  hipLaunchKernelGGL(sol_lightmap_emit_kernel, dim3((W * H + LM_WG - 1) / LM_WG), dim3(LM_WG), 0, stream, vertices, normals, uvs, A, (const uint32_t*)owner,
                     (float*)points, (uint32_t*)texels);
  return hipGetLastError();
}

hipError_t sol_launch_lightmap_dilate_begin(const void* texels, uint32_t n_texels, const void* values, uint32_t stride_words, void* out, uint8_t* cover,
                                            hipStream_t stream) {
  hipLaunchKernelGGL(sol_lightmap_dilate_begin_kernel, dim3((n_texels + LM_WG - 1) / LM_WG), dim3(LM_WG), 0, stream, (const uint32_t*)texels, n_texels,
                     (const uint32_t*)values, stride_words, (uint32_t*)out, cover);
  return hipGetLastError();
}
hipError_t sol_launch_lightmap_dilate_pass(uint32_t W, uint32_t H, uint32_t channels, uint32_t stride_words, uint32_t pass, void* out, const uint8_t* cover_in,
                                           uint8_t* cover_out, hipStream_t stream) {
  hipLaunchKernelGGL(sol_lightmap_dilate_pass_kernel, dim3((W * H + LM_WG - 1) / LM_WG), dim3(LM_WG), 0, stream, W, H, channels, stride_words, pass, (float*)out,
                     cover_in, cover_out);
  return hipGetLastError();
}
