// sol_lightmap_filter_var.hip -- variance-guided a-trous filtering of a baked atlas (sol_lightmap_filter_var; sol_lightmap_filter_var.cpp;
// DESIGN.md 27), and the projection of a gather's per-sample colours onto their two moments (sol_irradiance_moments; sol_api.cpp).
//
//   sol_moments_project_kernel                  a thread per point after each sol_radiance_each_kernel launch: the window's colours and their squares
//                                               added in sol_radiance's association - sol_sh_project_kernel without the direction redraw.
//   sol_lightmap_filter_var_prepare_kernel      a lane per texel: judges liveness once, packs the guides as sol_lightmap_filter_prepare_kernel does
//                                               - (position, live word), (normal, 0) -, writes the mean (x, samples) and the variance of the mean
//                                               (v, 0) into the first side's two dwordx4 planes, and the rows of a texel that is not live.
//   sol_lightmap_filter_var_pass_plain_kernel   a lane per texel: the nine taps of the variance prefilter and the 25 taps' guides, means and
//                                               variances come from global memory.
//   sol_lightmap_filter_var_pass_staged_kernel  the same body for steps 1 and 2: the workgroup's 16 x 16 tile and its halo of 2 x step texels are
//                                               staged in four dwordx4 LDS arrays first (position + live, normal, mean, variance: 24 x 24 texels x
//                                               64 bytes = 36 KiB at step 2). A texel outside the atlas is staged as not live.
// Both pass kernels call the rule of sol_lightmap_filter_var.h and add in tap order, one lane per sum: the same words. The .w word of a mean is the
// centre's `samples`, carried through every pass. No float atomics; every store is a vector store.
#include <hip/hip_runtime.h>

#include "../../include/solstrale_hip.h"
#include "sol_launch.h"
#include "sol_lightmap_filter_var.h"
#include "sol_ray.h"

#define LFV_WG 256
#define LFV_TILE 16
#define LFV_SIDE_MAX (LFV_TILE + 8)  // step 2: a halo of 4 texels on each side

namespace {
struct LfvArgs {
  uint32_t W, H, step, last;
  float sigma_position, sigma_plane, sigma_value, variance_floor;
  uint32_t normal_power_log2;
  const float4* guide;         // two per texel
  const float4 *in_x, *in_v;   // [W * H] each
  float4 *out_x, *out_v;       // every pass but the last
  float4 *out_rows, *var_rows;  // the caller's rows: the last pass (var_rows may be null)
};

DEV float4 lfv_zero4() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
DEV bool lfv_live(const float4& P) { return __float_as_uint(P.w) != 0u; }
DEV void lfv_store(float4* p, float x, float y, float z, float w) { *(SOL_AS1 sol_v4f*)p = sol_v4f{x, y, z, w}; }

// The tile's side x side texels from (x0, y0) on. A texel outside the atlas or not live is staged as not live, with zero words behind it.
DEV void lfv_stage(const LfvArgs& A, int x0, int y0, int side, float4* sP, float4* sN, float4* sX, float4* sV) {
  for (int t = (int)threadIdx.x; t < side * side; t += LFV_WG) {
    const int ly = t / side, lx = t - ly * side;
    const int gx = x0 + lx, gy = y0 + ly;
    float4 P = lfv_zero4(), N = lfv_zero4(), X = lfv_zero4(), V = lfv_zero4();
    if (gx >= 0 && gy >= 0 && gx < (int)A.W && gy < (int)A.H) {
      const size_t q = (size_t)gy * A.W + (size_t)gx;
      P = ldg_f4(A.guide + 2 * q);
      if (lfv_live(P)) {
        N = ldg_f4(A.guide + 2 * q + 1);
        X = ldg_f4(A.in_x + q);
        V = ldg_f4(A.in_v + q);
      } else {
        P = lfv_zero4();
      }
    }
    sP[t] = P;
    sN[t] = N;
    sX[t] = X;
    sV[t] = V;
  }
}

template <bool STAGED>
DEV void lfv_pass(const LfvArgs& A, float4* sP, float4* sN, float4* sX, float4* sV) {
  const uint32_t tiles_x = (A.W + LFV_TILE - 1) / LFV_TILE;
  const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const uint32_t lx = threadIdx.x % LFV_TILE, ly = threadIdx.x / LFV_TILE;
  const uint32_t px = tx * LFV_TILE + lx, py = ty * LFV_TILE + ly;
  const bool inside = px < A.W && py < A.H;
  const size_t x = inside ? (size_t)py * A.W + px : 0;
  const int step = (int)A.step, halo = 2 * step, side = LFV_TILE + 2 * halo;
  const int lc = ((int)ly + halo) * side + (int)lx + halo;
  if (STAGED) {
    lfv_stage(A, (int)(tx * LFV_TILE) - halo, (int)(ty * LFV_TILE) - halo, side, sP, sN, sX, sV);
    __syncthreads();
  }
  float4 Pp = lfv_zero4();
  if (inside) Pp = STAGED ? sP[lc] : ldg_f4(A.guide + 2 * x);
  if (!(inside && lfv_live(Pp))) return;  // (behind the only barrier)
  const float4 Np = STAGED ? sN[lc] : ldg_f4(A.guide + 2 * x + 1);
  const float4 Xp = STAGED ? sX[lc] : ldg_f4(A.in_x + x);
  const float4 Vp = STAGED ? sV[lc] : ldg_f4(A.in_v + x);
  const LfvPass c = lfv_pass_of(A.sigma_position, A.sigma_plane, A.sigma_value, A.variance_floor, A.normal_power_log2, A.step);
  // the variance prefilter: nine texels one apart, whatever the step
  float vb0 = 0.0f, vb1 = 0.0f, vb2 = 0.0f, gs = 0.0f;
#pragma unroll
  for (int dj = -1; dj <= 1; ++dj) {
#pragma unroll
    for (int di = -1; di <= 1; ++di) {
      const float g = lfv_h3(di) * lfv_h3(dj);
      float4 Vq = Vp;
      if (di != 0 || dj != 0) {
        if (STAGED) {
          const int lq = lc + dj * side + di;
          if (!lfv_live(sP[lq])) continue;
          Vq = sV[lq];
        } else {
          const int qx = (int)px + di, qy = (int)py + dj;
          if (qx < 0 || qy < 0 || qx >= (int)A.W || qy >= (int)A.H) continue;
          const size_t q = (size_t)qy * A.W + (size_t)qx;
          if (!lfv_live(ldg_f4(A.guide + 2 * q))) continue;
          Vq = ldg_f4(A.in_v + q);
        }
      }
      lfv_prefilter_add(g, Vq.x, Vq.y, Vq.z, vb0, vb1, vb2, gs);
    }
  }
  const float den = lfv_den(vb0, vb1, vb2, gs, c);
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, u0 = 0.0f, u1 = 0.0f, u2 = 0.0f, wsum = 0.0f;
#pragma nounroll  // (a row of five taps in flight at a time, as in sol_lightmap_filter.hip)
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
      if (!lfv_live(Pq)) continue;
      float w = k;
      float4 Xq = Xp, Vq = Vp;
      if (!centre) {
        const float4 Nq = STAGED ? sN[lq] : ldg_f4(A.guide + 2 * q + 1);
        Xq = STAGED ? sX[lq] : ldg_f4(A.in_x + q);
        const float geometry = lfv_geometry(k, Pp.x, Pp.y, Pp.z, Np.x, Np.y, Np.z, Pq.x, Pq.y, Pq.z, Nq.x, Nq.y, Nq.z, c);
        w = lfv_weight(geometry, Xp.x, Xp.y, Xp.z, Xq.x, Xq.y, Xq.z, den);
        if (!(w > 0.0f)) continue;
        Vq = STAGED ? sV[lq] : ldg_f4(A.in_v + q);
      }
      const float ww = w * w;
      s0 = s0 + (w * Xq.x);
      s1 = s1 + (w * Xq.y);
      s2 = s2 + (w * Xq.z);
      u0 = u0 + (ww * Vq.x);
      u1 = u1 + (ww * Vq.y);
      u2 = u2 + (ww * Vq.z);
      wsum = wsum + w;
    }
  }
  const float w2 = wsum * wsum;
  const float x0 = s0 / wsum, x1 = s1 / wsum, x2 = s2 / wsum;
  const float v0 = u0 / w2, v1 = u1 / w2, v2 = u2 / w2;
  if (A.last) {
    const float N = (float)__float_as_uint(Xp.w);
    lfv_store(A.out_rows + x, x0 * N, x1 * N, x2 * N, Xp.w);
    if (A.var_rows) lfv_store(A.var_rows + x, v0, v1, v2, 0.0f);
  } else {
    lfv_store(A.out_x + x, x0, x1, x2, Xp.w);
    lfv_store(A.out_v + x, v0, v1, v2, 0.0f);
  }
}
}  // namespace

// One thread per point of an irradiance-moments query, after each sol_radiance_each_kernel launch: the window's `win_samples`
// colours of the point, partial[sample - P.first_sample][point], and their squares (one rounding each), added in sol_radiance's association - a
// chunk sum 0 + t + t .. per 16 samples counted from P.first_sample (a window starts on a chunk's first sample), the chunk sums in order on top
// of 0 or, `accumulate`, of what the earlier windows of the call left in `out`. The row's validity is judged first: no colour of an invalid row
// is read (none was written), it answers eight zero words. out: 2 dwordx4 per row.
__global__ void __launch_bounds__(256) sol_moments_project_kernel(const RadianceParams P, const float4* __restrict__ points, const sol_v4f* __restrict__ partial,
                                                                  sol_v4f* __restrict__ out, uint32_t win_samples, uint32_t samples, uint32_t accumulate) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= P.n_rays) return;
  const float4 a = ldg_f4(points + (size_t)i * 2u), b = ldg_f4(points + (size_t)i * 2u + 1u);
  SOL_AS1 sol_v4f* const row = (SOL_AS1 sol_v4f*)(out + (size_t)i * 2u);
  if (!query_ray_valid(a, b)) {
    const sol_v4f zero = {0.f, 0.f, 0.f, 0.f};
    row[0] = zero;
    row[1] = zero;
    return;
  }
  float total[6], chunk[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) total[q] = 0.f;
  if (accumulate) {
    const sol_v4f o0 = row[0], o1 = row[1];
    total[0] = o0.x; total[1] = o0.y; total[2] = o0.z;
    total[3] = o1.x; total[4] = o1.y; total[5] = o1.z;
  }
  const size_t stride = (size_t)P.n_groups * 64u;
  for (uint32_t j0 = 0; j0 < win_samples; j0 += SOL_CHUNK) {
#pragma unroll
    for (int q = 0; q < 6; ++q) chunk[q] = 0.f;
    const uint32_t j1 = win_samples - j0 > (uint32_t)SOL_CHUNK ? j0 + SOL_CHUNK : win_samples;
    for (uint32_t j = j0; j < j1; ++j) {
      const sol_v4f c = *(const SOL_AS1 sol_v4f*)(partial + (size_t)j * stride + i);  // coalesced: [sample][point]
      chunk[0] = chunk[0] + c.x;
      chunk[1] = chunk[1] + c.y;
      chunk[2] = chunk[2] + c.z;
      chunk[3] = chunk[3] + (c.x * c.x);
      chunk[4] = chunk[4] + (c.y * c.y);
      chunk[5] = chunk[5] + (c.z * c.z);
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) total[q] = total[q] + chunk[q];
  }
  const sol_v4f r0 = {total[0], total[1], total[2], __uint_as_float(samples)}, r1 = {total[3], total[4], total[5], 0.f};
  row[0] = r0;  // one dwordx4 each
  row[1] = r1;
}

__global__ __launch_bounds__(LFV_WG) void sol_lightmap_filter_var_prepare_kernel(const uint32_t* __restrict__ texels, const float4* __restrict__ points,
                                                                                 const float4* __restrict__ moments, uint32_t n_texels,
                                                                                 float4* __restrict__ guide, float4* __restrict__ plane_x,
                                                                                 float4* __restrict__ plane_v, float4* __restrict__ out,
                                                                                 float4* __restrict__ variance_out) {
  const uint32_t x = blockIdx.x * LFV_WG + threadIdx.x;
  if (x >= n_texels) return;
  const float4 p = ldg_f4(points + 2 * (size_t)x), n = ldg_f4(points + 2 * (size_t)x + 1);
  const float4 m0 = ldg_f4(moments + 2 * (size_t)x), m1 = ldg_f4(moments + 2 * (size_t)x + 1);
  const uint32_t samples = __float_as_uint(m0.w);
  bool live = ldg_u32(texels + (size_t)x * 4) != SOL_LF_TEXEL_NONE;
  live = live && lf_finite(p.x) && lf_finite(p.y) && lf_finite(p.z) && lf_finite(n.x) && lf_finite(n.y) && lf_finite(n.z);
  live = live && samples >= 2u;
  live = live && lf_finite(m0.x) && lf_finite(m0.y) && lf_finite(m0.z) && lf_finite(m1.x) && lf_finite(m1.y) && lf_finite(m1.z);
  float4 X = lfv_zero4(), V = lfv_zero4();
  if (live) {
    const float N = (float)samples, M = (float)(samples - 1u);
    X.x = lfv_mean(m0.x, N); X.y = lfv_mean(m0.y, N); X.z = lfv_mean(m0.z, N); X.w = m0.w;
    V.x = lfv_variance(m1.x, X.x, N, M); V.y = lfv_variance(m1.y, X.y, N, M); V.z = lfv_variance(m1.z, X.z, N, M);
  } else {
    lfv_store(out + x, m0.x, m0.y, m0.z, m0.w);
    if (variance_out) lfv_store(variance_out + x, 0.0f, 0.0f, 0.0f, 0.0f);
  }
  lfv_store(plane_x + x, X.x, X.y, X.z, X.w);
  lfv_store(plane_v + x, V.x, V.y, V.z, 0.0f);
  lfv_store(guide + 2 * (size_t)x, p.x, p.y, p.z, __uint_as_float(live ? 1u : 0u));
  lfv_store(guide + 2 * (size_t)x + 1, n.x, n.y, n.z, 0.0f);
}

__global__ __launch_bounds__(LFV_WG) void sol_lightmap_filter_var_pass_plain_kernel(LfvArgs A) { lfv_pass<false>(A, nullptr, nullptr, nullptr, nullptr); }

__global__ __launch_bounds__(LFV_WG) void sol_lightmap_filter_var_pass_staged_kernel(LfvArgs A) {
  __shared__ float4 sP[LFV_SIDE_MAX * LFV_SIDE_MAX], sN[LFV_SIDE_MAX * LFV_SIDE_MAX], sX[LFV_SIDE_MAX * LFV_SIDE_MAX], sV[LFV_SIDE_MAX * LFV_SIDE_MAX];
  lfv_pass<true>(A, sP, sN, sX, sV);
}

// ---- launches (sol_launch.h) ----
hipError_t sol_launch_moments_project(const RadianceParams& P, const void* points, const void* partial, void* out, uint32_t win_samples, uint32_t samples,
                                      bool accumulate, hipStream_t stream) {
  hipLaunchKernelGGL(sol_moments_project_kernel, dim3((P.n_rays + 255u) / 256u), dim3(256), 0, stream, P, (const float4*)points, (const sol_v4f*)partial,
                     (sol_v4f*)out, win_samples, samples, accumulate ? 1u : 0u);
  return hipGetLastError();
}

hipError_t sol_launch_lightmap_filter_var_prepare(const void* texels, const void* points, const void* moments, uint32_t n_texels, void* guide, void* plane_x,
                                                  void* plane_v, void* out, void* variance_out, hipStream_t stream) {
  hipLaunchKernelGGL(sol_lightmap_filter_var_prepare_kernel, dim3((n_texels + LFV_WG - 1) / LFV_WG), dim3(LFV_WG), 0, stream, (const uint32_t*)texels,
                     (const float4*)points, (const float4*)moments, n_texels, (float4*)guide, (float4*)plane_x, (float4*)plane_v, (float4*)out,
                     (float4*)variance_out);
  return hipGetLastError();
}

hipError_t sol_launch_lightmap_filter_var_pass(const SolLightmapFilterVarConfig& c, uint32_t pass, bool staged, const void* guide, const void* in_x,
                                               const void* in_v, void* out_x, void* out_v, void* out_rows, void* var_rows, hipStream_t stream) {
  LfvArgs A{};
  A.W = c.width; A.H = c.height; A.step = 1u << pass; A.last = pass + 1u == c.iterations ? 1u : 0u;
  A.sigma_position = c.sigma_position; A.sigma_plane = c.sigma_plane; A.sigma_value = c.sigma_value; A.variance_floor = c.variance_floor;
  A.normal_power_log2 = c.normal_power_log2;
  A.guide = (const float4*)guide; A.in_x = (const float4*)in_x; A.in_v = (const float4*)in_v; A.out_x = (float4*)out_x; A.out_v = (float4*)out_v;
  A.out_rows = (float4*)out_rows; A.var_rows = (float4*)var_rows;
  const dim3 grid(((c.width + LFV_TILE - 1) / LFV_TILE) * ((c.height + LFV_TILE - 1) / LFV_TILE));
  if (staged && A.step <= 2u)
    hipLaunchKernelGGL(sol_lightmap_filter_var_pass_staged_kernel, grid, dim3(LFV_WG), 0, stream, A);
  else
    hipLaunchKernelGGL(sol_lightmap_filter_var_pass_plain_kernel, grid, dim3(LFV_WG), 0, stream, A);
  return hipGetLastError();
}
