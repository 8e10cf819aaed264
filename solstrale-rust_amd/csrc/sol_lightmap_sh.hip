// sol_lightmap_sh.hip -- directional lightmaps: an atlas of SolSh9 rows looked up at surface rows and shaded at the caller's normals, and the
// normals of surface rows (sol_lightmap_sh, sol_lightmap_normals; sol_lightmap_sh.cpp). The rule is sol_lightmap_sh.h (and, for
// the lookup, sol_lightmap_sample.h through the shared steps of sol_lightmap_lookup.h); the kernels only fetch, exchange, call it and store.
//
//   sol_lightmap_sh_kernel       EIGHT lanes to a surface row, eight rows to a wave. Lane g of an octet owns dwordx4 g of a 112-byte value row
//                                (g = 0..6: words 0..27; lane 7 owns none), so a tap of a row is ONE contiguous 112-byte fetch by seven
//                                neighbouring lanes. The row (ls_surface) is read by every lane of the octet - one address, one request. The
//                                tap decision is divided: lane t < 4 decides tap t (ls_tap_live) and a ballot hands all eight lanes the same
//                                mask. The seven value lanes then fetch the covered taps and judge their own words; a ballot per tap is the AND
//                                over the octet. Coefficient mode stores the lane's dwordx4 of the answer (seven to a row). Evaluation mode:
//                                each lane forms t = B_k * L[w] for its words and writes them to LDS as one ds_write_b128 (32 rows x 28 words =
//                                3.5 KiB a workgroup); lanes 0..2 of the octet - one per channel - read their nine words back (row stride 28
//                                words: the 12 reading lanes of a 32-lane half fall on 12 different banks) and add them in k order; two
//                                shuffles bring green and blue to lane 0, which stores the row as one dwordx4. LDS rather than nine rounds of
//                                ds_bpermute: a bpermute fetches ONE register of the source lane, and channel ch wants word (3k + ch) & 3 of lane
//                                (3k + ch) >> 2 - a different register for each of the three receivers - so the transport would take up to
//                                three permutes per k through the same LDS crossbar, against one write and nine conflict-free reads.
//                                No lane leaves before the last exchange: invalid rows, rows beyond n and octets with different tap counts run
//                                to the end of the kernel; every ballot, the barrier and the shuffles stand in uniform control flow, and only
//                                loads, stores and arithmetic are predicated. The sums are made in tap order and in k order by one lane each:
//                                no output word depends on the transport or the schedule.
//   sol_lightmap_normals_kernel  a lane per surface row: the row as one dwordx4, nine vertex words, (where given) nine normal words, one
//                                dwordx4 out.
// No atomics, no scratch; every store is a vector store.
#include <hip/hip_runtime.h>

#include "../../include/solstrale_hip.h"
#include "sol_launch.h"
#include "sol_lightmap_lookup.h"
#include "sol_lightmap_sh.h"

#define LSH_WG 256
#define LSH_ROWS (LSH_WG / 8)  // rows of a workgroup
#define LSH_ROW_WORDS 28

static_assert(sizeof(SolSh9) == 4 * LSH_ROW_WORDS && sizeof(SolTexel) == 16 && sizeof(SolRadiance) == 16 && sizeof(SolRay) == 32,
              "the records of include/solstrale_hip.h");
static_assert(SOL_LSH_CHANNELS == 27u && SOL_LS_NONE == SOL_TEXEL_NONE, "a SolSh9 row is 27 coefficients and the sample count");

struct LshAtlas {
  uint32_t W, H, stride_words, n_triangles;
  uint32_t nearest, guard, coefficients, clamp;
  float chart_radius, scale;
};

// B of word w's term (k = w / 3) without indexing a register array by a lane's number
DEV float lsh_pick(const float (&B)[9], uint32_t k) {
  float b = 0.0f;
#pragma unroll
  for (uint32_t j = 0; j < 9u; ++j) b = k == j ? B[j] : b;
  return b;
}

__global__ __launch_bounds__(LSH_WG) void sol_lightmap_sh_kernel(LshAtlas A, const float* __restrict__ uvs, const uint32_t* __restrict__ texels,
                                                                 const uint8_t* __restrict__ pass_of, const float* __restrict__ values,
                                                                 const float* __restrict__ vertices, const float* __restrict__ points,
                                                                 const uint32_t* __restrict__ coords, const float* __restrict__ normals, uint32_t n,
                                                                 uint32_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float lds_t[LSH_ROWS * LSH_ROW_WORDS];
  const uint32_t g = threadIdx.x & 7u, local_row = threadIdx.x >> 3;
  const uint32_t octet_shift = threadIdx.x & 56u;  // the octet's first lane within the wave
  const uint32_t x = blockIdx.x * LSH_ROWS + local_row;
  const bool in_range = x < n;

  // 1. the row (every lane of the octet: one address): nothing of it is an address before it is known to be one
  sol_v4u row = {SOL_LS_NONE, 0u, 0u, 0u};
  if (in_range) row = *(const SOL_AS1 sol_v4u*)(coords + (size_t)x * 4);
  const LsSurface S = ls_surface(row, A.n_triangles, uvs, vertices, A.guard != 0u);  // (a row beyond n is SOL_LS_NONE: not valid)
  const LsTaps T = ls_surface_taps(S, A.W, A.H, A.nearest != 0u);

  // 2. coverage and the chart guard: lane t of the octet decides tap t, before any value is fetched
  const bool mine = ls_tap_live(T, g, A.W, A.H, ls_guard_test(texels, pass_of, points, A.guard != 0u, S, A.chart_radius));
  uint32_t live = (uint32_t)(sol_ballot(mine) >> octet_shift) & 0xFu;  // bit k: tap k; the same in all eight lanes

  // 3. the value words of the covered taps, a dwordx4 a lane: one word that is not finite takes its tap out (word 27 is not judged)
  sol_v4f val[4];
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    val[k] = sol_v4f{0.0f, 0.0f, 0.0f, 0.0f};
    if ((live & (1u << k)) && g < 7u)
      val[k] = *(const SOL_AS1 sol_v4f*)(values + ((size_t)ls_tap_j(T, k) * A.W + (size_t)ls_tap_i(T, k)) * A.stride_words + 4u * g);
    const bool bad = !(lf_finite(val[k].x) && lf_finite(val[k].y) && lf_finite(val[k].z) && (g == 6u || lf_finite(val[k].w)));
    if ((uint32_t)(sol_ballot(bad) >> octet_shift) & 0xFFu) live &= ~(1u << k);
  }

  // 4. the interpolated coefficients of this lane's four words
  LsWeights R = {{0.0f, 0.0f, 0.0f, 0.0f}, 0.0f, live, live};  // (nearest: the count is the one tap's bit)
  if (!A.nearest) R = ls_weights(T, live);
  live = R.live;
  const uint32_t count = R.count;
  sol_v4f L = {0.0f, 0.0f, 0.0f, 0.0f};
  if (live) {
    if (A.nearest) {
      L = val[0];  // the one tap's words, copied
    } else {
      L.x = lsh_word(live, R.w, val[0].x, val[1].x, val[2].x, val[3].x, R.wsum);
      L.y = lsh_word(live, R.w, val[0].y, val[1].y, val[2].y, val[3].y, R.wsum);
      L.z = lsh_word(live, R.w, val[0].z, val[1].z, val[2].z, val[3].z, R.wsum);
      L.w = lsh_word(live, R.w, val[0].w, val[1].w, val[2].w, val[3].w, R.wsum);
    }
  }

  if (A.coefficients) {  // (uniform: a kernel argument) 28 words a row, seven dwordx4
    if (in_range && g < 7u) {
      sol_v4u o = {__float_as_uint(L.x), __float_as_uint(L.y), __float_as_uint(L.z), __float_as_uint(L.w)};
      if (g == 6u) o.w = count;
      *(SOL_AS1 sol_v4u*)(out + (size_t)x * LSH_ROW_WORDS + 4u * g) = o;
    }
    return;
  }

  // 5. evaluation: the products of this lane's words to LDS, one lane per channel adds them in k order
  sol_v4f nrm = {0.0f, 0.0f, 0.0f, 0.0f};
  if (in_range && live) nrm = *(const SOL_AS1 sol_v4f*)(normals + (size_t)x * 4);
  const bool ok = live != 0u && lsh_normal_ok(nrm.x, nrm.y, nrm.z);
  float B[9];
  lsh_lobe(nrm.x, nrm.y, nrm.z, B);
  if (g < 7u) {
    const uint32_t w0 = 4u * g;
    const sol_v4f t = {lsh_pick(B, w0 / 3u) * L.x, lsh_pick(B, (w0 + 1u) / 3u) * L.y, lsh_pick(B, (w0 + 2u) / 3u) * L.z, lsh_pick(B, (w0 + 3u) / 3u) * L.w};
    *(sol_v4f*)(lds_t + local_row * LSH_ROW_WORDS + w0) = t;
  }
  __syncthreads();
  float E = 0.0f;
  if (g < 3u) {
    float t[9];
#pragma unroll
    for (uint32_t k = 0; k < 9u; ++k) t[k] = lds_t[local_row * LSH_ROW_WORDS + 3u * k + g];
    E = lsh_finish(t, A.scale, A.clamp != 0u);
  }
  const float Eg = __shfl_down(E, 1), Eb = __shfl_down(E, 2);
  if (in_range && g == 0u) {
    const sol_v4u o = {__float_as_uint(E), __float_as_uint(Eg), __float_as_uint(Eb), count};
    *(SOL_AS1 sol_v4u*)(out + (size_t)x * 4) = ok ? o : sol_v4u{0u, 0u, 0u, 0u};
  }
}

__global__ __launch_bounds__(LSH_WG) void sol_lightmap_normals_kernel(const uint32_t* __restrict__ coords, uint32_t n, const float* __restrict__ vertices,
                                                                      const float* __restrict__ vertex_normals, uint32_t n_triangles,
                                                                      uint32_t* __restrict__ out) {
  const uint32_t x = blockIdx.x * LSH_WG + threadIdx.x;
  if (x >= n) return;
  const sol_v4u row = *(const SOL_AS1 sol_v4u*)(coords + (size_t)x * 4);
  const float b1 = __uint_as_float(row.y), b2 = __uint_as_float(row.z);
  bool valid = ls_row_valid(row, n_triangles);
  f3 unit = {0.0f, 0.0f, 0.0f};
  if (valid) {
    float pos[9], nv[9];
    const SOL_AS1 float* p = (const SOL_AS1 float*)(vertices + (size_t)row.x * 9);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      pos[k] = p[k];
      nv[k] = 0.0f;
      valid = valid && lf_finite(pos[k]);
    }
    if (vertex_normals) {
      const SOL_AS1 float* q = (const SOL_AS1 float*)(vertex_normals + (size_t)row.x * 9);
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        nv[k] = q[k];
        valid = valid && lf_finite(nv[k]);
      }
    }
    valid = valid && lsh_surface_normal(pos, vertex_normals ? nv : nullptr, b1, b2, unit);
  }
  const sol_v4u o = {__float_as_uint(unit.x), __float_as_uint(unit.y), __float_as_uint(unit.z), 0u};
  *(SOL_AS1 sol_v4u*)(out + (size_t)x * 4) = valid ? o : sol_v4u{0u, 0u, 0u, 0u};
}

// ---- launches (sol_launch.h) ----
hipError_t sol_launch_lightmap_sh(const SolLightmapShConfig& c, uint32_t n_triangles, const void* uvs, const void* texels, const void* pass_of,
                                  const void* values, const void* vertices, const void* points, const void* coords, const void* normals, uint32_t n,
                                  void* out, hipStream_t stream) {
  const bool guard = vertices && points && (__builtin_isfinite(c.chart_radius) != 0);
  const bool coefficients = (c.flags & SOL_LIGHTMAP_SH_COEFFICIENTS) != 0u;
  const LshAtlas A{c.width, c.height, c.stride_bytes / 4u, n_triangles, (c.flags & SOL_LIGHTMAP_SH_NEAREST) ? 1u : 0u, guard ? 1u : 0u,
                   coefficients ? 1u : 0u, (c.flags & SOL_LIGHTMAP_SH_CLAMP) ? 1u : 0u, guard ? c.chart_radius : 0.0f, coefficients ? 1.0f : c.scale};
  hipLaunchKernelGGL(sol_lightmap_sh_kernel, dim3((uint32_t)(((uint64_t)n + LSH_ROWS - 1) / LSH_ROWS)), dim3(LSH_WG), 0, stream, A, (const float*)uvs,
                     (const uint32_t*)texels, (const uint8_t*)pass_of, (const float*)values, (const float*)vertices, (const float*)points,
                     (const uint32_t*)coords, (const float*)normals, n, (uint32_t*)out);
  return hipGetLastError();
}

hipError_t sol_launch_lightmap_normals(const void* coords, uint32_t n, const void* vertices, const void* vertex_normals, uint32_t n_triangles, void* out,
                                       hipStream_t stream) {
  hipLaunchKernelGGL(sol_lightmap_normals_kernel, dim3((uint32_t)(((uint64_t)n + LSH_WG - 1) / LSH_WG)), dim3(LSH_WG), 0, stream, (const uint32_t*)coords, n,
                     (const float*)vertices, (const float*)vertex_normals, n_triangles, (uint32_t*)out);
  return hipGetLastError();
}
