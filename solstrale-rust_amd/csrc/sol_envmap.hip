// sol_envmap.hip -- environment importance sampling (include/solstrale_hip.h, sol_env_*): the tables the ENV render kernels
// draw from, built on the scene's stream, and the diagnostics that read them back or run the device's sampler and pdf on host data.
//
// Cells. The map is read nearest-texel with x = u (W - 1), y = (1 - v)(H - 1) (env_color, sol_path.h), so with W' = max(W - 1, 1) and
// H' = max(H - 1, 1) cell (i, j), i < W', j < H', is texel (i, j); the last column and row are read on a set of measure zero and get no cell.
// Weight w_ij = Y(texel) * sin(pi (1 - (j + 0.5) / H')), Y = 0.2126 R + 0.7152 G + 0.0722 B; a weight that is not finite or not above 0 is 0.
//
// Summation order (fixed: the tables are bit-identical on every device and rank; no atomics):
//   weights    fp32, ((0.2126f R + 0.7152f G) + 0.0722f B) * s_j, s_j = (float) of the double sin(pi * (1 - (j + 0.5) / H'))
//   row j      c_i = c_{i-1} + w_ij in order of i from c_{-1} = 0; T_j = c_{W'-1}; conditional CDF c_i / T_j, or (i + 1) / W' when T_j == 0
//   marginal   m_j = m_{j-1} + T_j in order of j from m_{-1} = 0; total = m_{H'-1}; marginal CDF m_j / total
// every operation one correctly rounded fp32 operation (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "sol_scene.h"
#include "sol_shade.h"

__host__ __device__ inline float sol_env_row_sin(uint32_t j, uint32_t ch) {
  return (float)sin(3.14159265358979323846 * (1.0 - ((double)j + 0.5) / (double)ch));
}
__host__ __device__ inline float sol_env_weight(const float* t, float row_sin) {
  const float y = 0.2126f * t[0] + 0.7152f * t[1] + 0.0722f * t[2];
  const float w = y * row_sin;
  return (w > 0.0f && w < __builtin_huge_valf()) ? w : 0.0f;  // (NaN fails the first test)
}

// One thread per cell: the weights, into the conditional table.
__global__ void __launch_bounds__(256) sol_env_weights_kernel(const float* __restrict__ env, uint32_t w_tex, uint32_t cw, uint32_t ch, float* __restrict__ cond) {
  const uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (c >= (uint64_t)cw * ch) return;
  const uint32_t j = (uint32_t)(c / cw), i = (uint32_t)(c - (uint64_t)j * cw);
  cond[c] = sol_env_weight(env + ((size_t)j * w_tex + i) * 3, sol_env_row_sin(j, ch));
}
// One thread per row: the running sum in column order, the row total, then the normalised conditional CDF in place.
__global__ void __launch_bounds__(64) sol_env_rows_kernel(float* __restrict__ cond, float* __restrict__ rowtot, uint32_t cw, uint32_t ch) {
  const uint32_t j = blockIdx.x * 64u + threadIdx.x;
  if (j >= ch) return;
  float* row = cond + (size_t)j * cw;
  float s = 0.0f;
  for (uint32_t i = 0; i < cw; ++i) {
    s = s + row[i];
    row[i] = s;
  }
  rowtot[j] = s;
  for (uint32_t i = 0; i < cw; ++i) row[i] = s > 0.0f ? row[i] / s : (float)(i + 1u) / (float)cw;  // (a row of weight 0 is never drawn)
}
// One thread: the marginal CDF over the row totals and the total (a total that is not finite and above 0 is refused by the host).
__global__ void __launch_bounds__(64) sol_env_marginal_kernel(const float* __restrict__ rowtot, float* __restrict__ marg, uint32_t ch, float* __restrict__ total) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float m = 0.0f;
  for (uint32_t j = 0; j < ch; ++j) {
    m = m + rowtot[j];
    marg[j] = m;
  }
  for (uint32_t j = 0; j < ch; ++j) marg[j] = marg[j] / m;
  *total = m;
}
// sol_env_eval: fn 0 (r1, r2) -> (direction xyz, pdf, i, j); fn 1 direction xyz -> (pdf, i, j). The hot path's own functions (sol_shade.h).
__global__ void __launch_bounds__(256) sol_env_eval_kernel(const DevScene S, uint32_t fn, const float* __restrict__ in, uint32_t n, float* __restrict__ out) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  uint32_t ci, cj;
  if (fn == 0) {
    float pdf;
    const f3 d = env_sample(S, in[2 * (size_t)k], in[2 * (size_t)k + 1], pdf, ci, cj);
    float* o = out + 6 * (size_t)k;
    o[0] = d.x; o[1] = d.y; o[2] = d.z; o[3] = pdf; o[4] = (float)ci; o[5] = (float)cj;
  } else {
    const float* d = in + 3 * (size_t)k;
    const float pdf = env_pdf(S, mk3(d[0], d[1], d[2]), ci, cj);
    float* o = out + 3 * (size_t)k;
    o[0] = pdf; o[1] = (float)ci; o[2] = (float)cj;
  }
}

std::string sol_env_refusal(const SolSceneDesc* d) {
  if (!d) return "null scene description";
  const bool has_env = d->abi_version >= 2u && d->env_texels && d->env_width && d->env_height;
  if (!has_env) return "the scene has no environment map";
  if (!(d->env_scale > 0.0) || !std::isfinite(d->env_scale)) return "env_scale must be finite and above 0";
  const uint32_t cw = std::max(d->env_width - 1u, 1u), ch = std::max(d->env_height - 1u, 1u);
  for (uint32_t j = 0; j < ch; ++j) {
    const float rs = sol_env_row_sin(j, ch);
    for (uint32_t i = 0; i < cw; ++i)
      if (sol_env_weight(d->env_texels + ((size_t)j * d->env_width + i) * 3, rs) > 0.0f) return "";
  }
  return "every cell of the environment map has weight 0";
}

static int env_config_check(const SolEnvSampling* c, const char* fn) {
  if (!c) return SOL_OK;  // (NULL: off)
  if (c->size < sizeof(SolEnvSampling)) return sol_fail(SOL_EINVAL, "%s: SolEnvSampling.size %u < %zu", fn, c->size, sizeof(SolEnvSampling));
  if (c->mode > SOL_ENV_SAMPLING_IMPORTANCE) return sol_fail(SOL_EINVAL, "%s: unknown mode %u (0 off, 1 importance)", fn, c->mode);
  if (c->reserved[0] || c->reserved[1]) return sol_fail(SOL_EINVAL, "%s: reserved fields must be 0", fn);
  return SOL_OK;
}

static int env_build(SolScene* s) {
  const uint32_t cw = std::max(s->S.env_w - 1u, 1u), ch = std::max(s->S.env_h - 1u, 1u);
  const size_t cells = (size_t)cw * ch;
  DevPtr<float> tables;
  if (sol_dev_alloc(tables, 2 * (size_t)ch + cells + 1) != hipSuccess) return sol_fail(SOL_ENOMEM, "sol_env_sampling: no memory for the tables");
  float* const t = tables.get();
  float *marg = t, *cond = t + ch, *rowtot = cond + cells, *total = rowtot + ch;
  float tot = 0.0f;
  hipLaunchKernelGGL(sol_env_weights_kernel, dim3((uint32_t)((cells + 255) / 256)), dim3(256), 0, s->stream, s->S.env, s->S.env_w, cw, ch, cond);
  hipLaunchKernelGGL(sol_env_rows_kernel, dim3((ch + 63u) / 64u), dim3(64), 0, s->stream, cond, rowtot, cw, ch);
  hipLaunchKernelGGL(sol_env_marginal_kernel, dim3(1), dim3(64), 0, s->stream, (const float*)rowtot, marg, ch, total);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(&tot, total, sizeof(float), hipMemcpyDeviceToHost, s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  if (e != hipSuccess) return sol_fail(SOL_EDEVICE, "sol_env_sampling: %s", hipGetErrorString(e));
  if (!(tot > 0.0f && tot < __builtin_huge_valf())) return sol_fail(SOL_EINVAL, "sol_env_sampling: the cell weights of the environment map sum to %g", (double)tot);
  s->env_tables = std::move(tables);
  s->env_total = tot;
  s->S.env_marg = marg;
  s->S.env_cond = cond;
  s->S.env_cw = cw;
  s->S.env_ch = ch;
  s->S.env_pdf_scale = (float)((double)cw * (double)ch / (2.0 * 3.14159265358979323846 * 3.14159265358979323846));
  return SOL_OK;
}

extern "C" {

int sol_env_sampling_check(const SolSceneDesc* desc, const SolEnvSampling* config) {
  int rc = env_config_check(config, "sol_env_sampling_check");
  if (rc) return rc;
  if (!config || config->mode == SOL_ENV_SAMPLING_OFF) return SOL_OK;
  const std::string why = sol_env_refusal(desc);
  if (!why.empty()) return sol_fail(SOL_EINVAL, "sol_env_sampling_check: %s", why.c_str());
  return SOL_OK;
}

int sol_env_sampling(SolScene* s, const SolEnvSampling* config) {
  int rc = env_config_check(config, "sol_env_sampling");  // (the configuration first: its errors do not need a device)
  if (rc) return rc;
  if (!s) return sol_fail(SOL_EINVAL, "null scene");
  const bool on = config && config->mode == SOL_ENV_SAMPLING_IMPORTANCE;
  if (on && !s->env_refusal.empty()) return sol_fail(SOL_EINVAL, "sol_env_sampling: %s", s->env_refusal.c_str());
  if (on && !s->env_tables) {
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = env_build(s))) return rc;
  }
  if (on != s->env_is) s->adaptive.open = false;  // (a session's rounds all use one estimator)
  s->env_is = on;
  return SOL_OK;
}

int sol_env_tables(SolScene* s, float* marginal, size_t n_marginal, float* conditional, size_t n_conditional, float* total) {
  if (!s) return sol_fail(SOL_EINVAL, "null scene");
  if (!s->env_tables) return sol_fail(SOL_EINVAL, "sol_env_tables: no tables (sol_env_sampling with mode 1 builds them)");
  const size_t ch = s->S.env_ch, cells = (size_t)s->S.env_cw * ch;
  if ((marginal && n_marginal < ch) || (conditional && n_conditional < cells))
    return sol_fail(SOL_EINVAL, "sol_env_tables: the tables hold %zu and %zu floats (%zu, %zu given)", ch, cells, n_marginal, n_conditional);
  HIP_TRY(hipSetDevice(s->device));
  if (marginal) HIP_TRY(hipMemcpyAsync(marginal, s->S.env_marg, ch * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  if (conditional) HIP_TRY(hipMemcpyAsync(conditional, s->S.env_cond, cells * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (total) *total = s->env_total;
  return SOL_OK;
}

int sol_env_eval(SolScene* s, uint32_t fn, const float* in, uint32_t n, float* out) {
  if (!s || !in || !out) return sol_fail(SOL_EINVAL, "null argument");
  if (fn > 1u) return sol_fail(SOL_EINVAL, "sol_env_eval: unknown function %u (0 sample, 1 pdf)", fn);
  if (!s->env_tables) return sol_fail(SOL_EINVAL, "sol_env_eval: no tables (sol_env_sampling with mode 1 builds them)");
  if (n == 0) return SOL_OK;
  if (n > (1u << 26)) return sol_fail(SOL_EINVAL, "sol_env_eval: more than 2^26 rows");
  HIP_TRY(hipSetDevice(s->device));
  const size_t ib = (size_t)n * (fn == 0 ? 2 : 3) * sizeof(float), ob = (size_t)n * (fn == 0 ? 6 : 3) * sizeof(float);
  DevPtr<float> din_own, dout_own;
  HIP_TRY(sol_dev_alloc(din_own, ib / sizeof(float)));
  if (sol_dev_alloc(dout_own, ob / sizeof(float)) != hipSuccess) return sol_fail(SOL_ENOMEM, "hipMalloc failed");
  float *const din = din_own.get(), *const dout = dout_own.get();
  hipError_t e = hipMemcpyAsync(din, in, ib, hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(sol_env_eval_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s->stream, s->S, fn, (const float*)din, n, dout);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout, ob, hipMemcpyDeviceToHost, s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  if (e != hipSuccess) return sol_fail(SOL_EDEVICE, "sol_env_eval: %s", hipGetErrorString(e));
  return SOL_OK;
}

}  // extern "C"
