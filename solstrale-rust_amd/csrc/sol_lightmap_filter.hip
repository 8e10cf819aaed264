// sol_lightmap_filter.hip -- chart-aware a-trous filtering of a baked atlas (sol_lightmap_filter; sol_lightmap_filter.cpp).
//
//   sol_lightmap_filter_prepare_kernel      a lane per texel: judges liveness once, packs the guides - (position, live word) in one dwordx4,
//                                           (normal, 0) in a second -, copies the row to `out` whole and the channels into the first value plane.
//   sol_lightmap_filter_pass_plain_kernel   a lane per (texel, group of four channels): the 25 taps' guides and values come from global memory.
//   sol_lightmap_filter_pass_staged_kernel  the same body for steps 1 and 2: the workgroup's 16 x 16 tile of guides and values and its halo of
//                                           2 x step texels are staged in LDS first (24 x 24 texels x 64 bytes = 36 KiB at step 2), and the taps
//                                           are read from there.
// The value planes are laid out by channel group: plane[g * W * H + x] is the dwordx4 of channels 4g .. 4g + 3 of texel x (zero behind
// `channels`), so that a wave reads 16 consecutive texels of a tile row as 256 consecutive bytes. A lane of group g > 0 reads group 0 too: the
// value factor compares the first three channels. `groups_per_lane` folds several groups into one lane (the weights are then recomputed per
// group); profiles/lightmap_filter.txt has the shapes measured. Both pass kernels call lf_weight (sol_lightmap_filter.h) and add in tap order,
// one lane per sum: the same words. No float atomics; every store is a vector store.
#include <hip/hip_runtime.h>

#include "../../include/solstrale_hip.h"
#include "sol_launch.h"
#include "sol_lightmap_filter.h"

#define LF_WG 256
#define LF_TILE 16
#define LF_SIDE_MAX (LF_TILE + 8)  // step 2: a halo of 4 texels on each side

namespace {
struct LfArgs {
  uint32_t W, H, step, channels, groups, groups_per_lane, stride_words, last;
  float sigma_position, sigma_plane, sigma_value, value_scale;
  uint32_t normal_power_log2;
  const float4* guide;  // two per texel
  const float4* in;     // [groups][W * H]
  float4* out_plane;    // [groups][W * H]: every pass but the last
  float* out_rows;      // the caller's rows: the last pass
};

DEV float4 lf_zero4() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
DEV bool lf_live(const float4& P) { return __float_as_uint(P.w) != 0u; }

// The tile's side x side texels from (x0, y0) on: guides and group 0 of the pass's input. A texel outside the atlas is staged as not live.
DEV void lf_stage_guides(const LfArgs& A, int x0, int y0, int side, float4* sP, float4* sN, float4* sV0) {
  for (int t = (int)threadIdx.x; t < side * side; t += LF_WG) {
    const int ly = t / side, lx = t - ly * side;
    const int gx = x0 + lx, gy = y0 + ly;
    float4 P = lf_zero4(), N = lf_zero4(), V = lf_zero4();
    if (gx >= 0 && gy >= 0 && gx < (int)A.W && gy < (int)A.H) {
      const size_t q = (size_t)gy * A.W + (size_t)gx;
      P = ldg_f4(A.guide + 2 * q);
      if (lf_live(P)) {
        N = ldg_f4(A.guide + 2 * q + 1);
        V = ldg_f4(A.in + q);
      } else {
        P = lf_zero4();
      }
    }
    sP[t] = P;
    sN[t] = N;
    sV0[t] = V;
  }
}
DEV void lf_stage_group(const LfArgs& A, const float4* in_g, int x0, int y0, int side, const float4* sP, float4* sVg) {
  for (int t = (int)threadIdx.x; t < side * side; t += LF_WG) {
    const int ly = t / side, lx = t - ly * side;
    float4 V = lf_zero4();
    if (lf_live(sP[t])) V = ldg_f4(in_g + ((size_t)(y0 + ly) * A.W + (size_t)(x0 + lx)));  // (live: inside the atlas)
    sVg[t] = V;
  }
}

template <bool STAGED>
DEV void lf_pass(const LfArgs& A, float4* sP, float4* sN, float4* sV0, float4* sVg) {
  const uint32_t tiles_x = (A.W + LF_TILE - 1) / LF_TILE;
  const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const uint32_t lx = threadIdx.x % LF_TILE, ly = threadIdx.x / LF_TILE;
  const uint32_t px = tx * LF_TILE + lx, py = ty * LF_TILE + ly;
  const bool inside = px < A.W && py < A.H;
  const size_t wh = (size_t)A.W * A.H;
  const size_t x = inside ? (size_t)py * A.W + px : 0;
  const int step = (int)A.step, halo = 2 * step, side = LF_TILE + 2 * halo;
  const int x0 = (int)(tx * LF_TILE) - halo, y0 = (int)(ty * LF_TILE) - halo;
  const int lc = ((int)ly + halo) * side + (int)lx + halo;
  if (STAGED) {
    lf_stage_guides(A, x0, y0, side, sP, sN, sV0);
    __syncthreads();
  }
  float4 Pp = lf_zero4(), Np = lf_zero4(), X0 = lf_zero4();
  if (inside) Pp = STAGED ? sP[lc] : ldg_f4(A.guide + 2 * x);
  const bool live = inside && lf_live(Pp);
  if (live) {
    Np = STAGED ? sN[lc] : ldg_f4(A.guide + 2 * x + 1);
    X0 = STAGED ? sV0[lc] : ldg_f4(A.in + x);
  }
  const LfPass c = lf_pass_of(A.sigma_position, A.sigma_plane, A.sigma_value, A.value_scale, A.normal_power_log2, A.channels, A.step);
  const float tp0 = lf_tone(X0.x, c.value_scale), tp1 = lf_tone(X0.y, c.value_scale), tp2 = lf_tone(X0.z, c.value_scale);
  const uint32_t g0 = blockIdx.y * A.groups_per_lane, g1 = g0 + A.groups_per_lane < A.groups ? g0 + A.groups_per_lane : A.groups;
  for (uint32_t g = g0; g < g1; ++g) {
    const float4* in_g = A.in + (size_t)g * wh;
    if (STAGED && g != 0u) {  // (g0, g1 are the workgroup's: every lane meets the barriers)
      __syncthreads();
      lf_stage_group(A, in_g, x0, y0, side, sP, sVg);
      __syncthreads();
    }
    if (!live) continue;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f, wsum = 0.0f;
#pragma nounroll  // (a row of five taps in flight at a time: all 25 unrolled cost 190 VGPRs and two waves per SIMD)
    for (int dj = -2; dj <= 2; ++dj) {
#pragma unroll
      for (int di = -2; di <= 2; ++di) {
        const float k = lf_h(di) * lf_h(dj);
        const bool centre = di == 0 && dj == 0;
        int lq = 0;
        size_t q = 0;
        float4 Pq;
        if (STAGED) {
          lq = lc + (dj * step) * side + di * step;
          Pq = sP[lq];
        } else {
          const int qx = (int)px + di * step, qy = (int)py + dj * step;
          if (qx < 0 || qy < 0 || qx >= (int)A.W || qy >= (int)A.H) continue;
          q = (size_t)qy * A.W + (size_t)qx;
          Pq = ldg_f4(A.guide + 2 * q);
        }
        if (!lf_live(Pq)) continue;
        float w = k;
        float4 Xq = X0;
        if (!centre) {
          const float4 Nq = STAGED ? sN[lq] : ldg_f4(A.guide + 2 * q + 1);
          Xq = STAGED ? sV0[lq] : ldg_f4(A.in + q);
          w = lf_weight(k, Pp.x, Pp.y, Pp.z, Np.x, Np.y, Np.z, Pq.x, Pq.y, Pq.z, Nq.x, Nq.y, Nq.z, tp0, tp1, tp2, Xq.x, Xq.y, Xq.z, c);
          if (!(w > 0.0f)) continue;
        }
        if (g != 0u) Xq = STAGED ? sVg[lq] : ldg_f4(in_g + q);
        s0 = s0 + (w * Xq.x);
        s1 = s1 + (w * Xq.y);
        s2 = s2 + (w * Xq.z);
        s3 = s3 + (w * Xq.w);
        wsum = wsum + w;
      }
    }
    const float4 r = make_float4(s0 / wsum, s1 / wsum, s2 / wsum, s3 / wsum);
    if (A.last) {
      float* row = A.out_rows + x * A.stride_words;
      const uint32_t ch = g * 4u;
      if (ch < A.channels) row[ch] = r.x;
      if (ch + 1u < A.channels) row[ch + 1u] = r.y;
      if (ch + 2u < A.channels) row[ch + 2u] = r.z;
      if (ch + 3u < A.channels) row[ch + 3u] = r.w;
    } else {
      *(SOL_AS1 sol_v4f*)(A.out_plane + (size_t)g * wh + x) = sol_v4f{r.x, r.y, r.z, r.w};
    }
  }
}
}  // namespace

__global__ __launch_bounds__(LF_WG) void sol_lightmap_filter_prepare_kernel(const uint32_t* __restrict__ texels, const float4* __restrict__ points,
                                                                            const uint32_t* __restrict__ values, uint32_t n_texels, uint32_t channels,
                                                                            uint32_t groups, uint32_t stride_words, float4* __restrict__ guide,
                                                                            float4* __restrict__ plane, uint32_t* __restrict__ out) {
  const uint32_t x = blockIdx.x * LF_WG + threadIdx.x;
  if (x >= n_texels) return;
  const float4 p = ldg_f4(points + 2 * (size_t)x), n = ldg_f4(points + 2 * (size_t)x + 1);
  bool live = ldg_u32(texels + (size_t)x * 4) != SOL_LF_TEXEL_NONE;
  live = live && lf_finite(p.x) && lf_finite(p.y) && lf_finite(p.z) && lf_finite(n.x) && lf_finite(n.y) && lf_finite(n.z);
  const size_t at = (size_t)x * stride_words;
  for (uint32_t g = 0; g < groups; ++g) {
    uint32_t w[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      const uint32_t ch = g * 4u + k;
      w[k] = ch < channels ? ldg_u32(values + at + ch) : 0u;
      live = live && (w[k] & 0x7F800000u) != 0x7F800000u;
    }
    *(SOL_AS1 sol_v4u*)(plane + (size_t)g * n_texels + x) = sol_v4u{w[0], w[1], w[2], w[3]};
  }
  for (uint32_t k = 0; k < stride_words; ++k) out[at + k] = ldg_u32(values + at + k);
  *(SOL_AS1 sol_v4f*)(guide + 2 * (size_t)x) = sol_v4f{p.x, p.y, p.z, __uint_as_float(live ? 1u : 0u)};
  *(SOL_AS1 sol_v4f*)(guide + 2 * (size_t)x + 1) = sol_v4f{n.x, n.y, n.z, 0.0f};
}

__global__ __launch_bounds__(LF_WG) void sol_lightmap_filter_pass_plain_kernel(LfArgs A) { lf_pass<false>(A, nullptr, nullptr, nullptr, nullptr); }

__global__ __launch_bounds__(LF_WG) void sol_lightmap_filter_pass_staged_kernel(LfArgs A) {
  __shared__ float4 sP[LF_SIDE_MAX * LF_SIDE_MAX], sN[LF_SIDE_MAX * LF_SIDE_MAX], sV0[LF_SIDE_MAX * LF_SIDE_MAX], sVg[LF_SIDE_MAX * LF_SIDE_MAX];
  lf_pass<true>(A, sP, sN, sV0, sVg);
}

// ---- launches (sol_launch.h) ----
hipError_t sol_launch_lightmap_filter_prepare(const void* texels, const void* points, const void* values, uint32_t n_texels, uint32_t channels,
                                              uint32_t stride_words, void* guide, void* plane, void* out, hipStream_t stream) {
  hipLaunchKernelGGL(sol_lightmap_filter_prepare_kernel, dim3((n_texels + LF_WG - 1) / LF_WG), dim3(LF_WG), 0, stream, (const uint32_t*)texels,
                     (const float4*)points, (const uint32_t*)values, n_texels, channels, (channels + 3u) / 4u, stride_words, (float4*)guide, (float4*)plane,
                     (uint32_t*)out);
  return hipGetLastError();
}

hipError_t sol_launch_lightmap_filter_pass(const SolLightmapFilterConfig& c, uint32_t pass, bool staged, bool fold_groups, const void* guide, const void* in,
                                           void* out_plane, void* out_rows, hipStream_t stream) {
  LfArgs A{};
  A.W = c.width; A.H = c.height; A.step = 1u << pass; A.channels = c.channels; A.groups = (c.channels + 3u) / 4u;
  A.groups_per_lane = fold_groups ? A.groups : 1u;
  A.stride_words = c.stride_bytes / 4u; A.last = pass + 1u == c.iterations ? 1u : 0u;
  A.sigma_position = c.sigma_position; A.sigma_plane = c.sigma_plane; A.sigma_value = c.sigma_value; A.value_scale = c.value_scale;
  A.normal_power_log2 = c.normal_power_log2;
  A.guide = (const float4*)guide; A.in = (const float4*)in; A.out_plane = (float4*)out_plane; A.out_rows = (float*)out_rows;
  const dim3 grid(((c.width + LF_TILE - 1) / LF_TILE) * ((c.height + LF_TILE - 1) / LF_TILE), (A.groups + A.groups_per_lane - 1u) / A.groups_per_lane);
  if (staged && A.step <= 2u)
    hipLaunchKernelGGL(sol_lightmap_filter_pass_staged_kernel, grid, dim3(LF_WG), 0, stream, A);
  else
    hipLaunchKernelGGL(sol_lightmap_filter_pass_plain_kernel, grid, dim3(LF_WG), 0, stream, A);
  return hipGetLastError();
}
