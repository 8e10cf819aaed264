// sol_denoise.hip -- the edge-aware a-trous denoiser (include/solstrale_hip.h "denoiser"): the colour sums are demodulated
// by the first-hit albedo, filtered by K passes of the 5x5 B3 a-trous kernel whose taps are weighted by the colour distance (tone-mapped)
// and the first-hit normal, then remodulated and written back as sums. Three kernels: prepare (means, demodulation, guide normal, miss
// flag), one pass launched K times (ping-pong between two buffers), finish (remodulation). Every per-pixel record is one float4 (16 B,
// one dwordx4 load); no atomics and a fixed tap order, so the output is bit-identical run to run. The arithmetic is restated in numpy
// by tests/denoise_ref.py.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "sol_scene.h"

#define SOL_DEN_TX 64  // a workgroup covers 64 x 4 pixels: one wave per image row segment, consecutive lanes on consecutive pixels
#define SOL_DEN_TY 4

// 1.-3. of the contract: c = S / n (non-finite values count as 0), a = A / m, v = N / m; f = a > 0.01 ? a : 1 per channel, e = c / f;
// guide = (v / |v|, 1) when |v| > 1e-3, else (0, 0, 0, 0): a miss.
__global__ void __launch_bounds__(256) sol_denoise_prepare_kernel(const float* __restrict__ image, const float* __restrict__ albedo,
                                                                  const float* __restrict__ normal, float4* __restrict__ e,
                                                                  float4* __restrict__ guide, uint32_t npix, float n, float m) {
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += gridDim.x * blockDim.x) {
    float ev[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float col = image[(size_t)p * 3 + c] / n;
      if (!isfinite(col)) col = 0.f;
      const float a = albedo[(size_t)p * 3 + c] / m;
      ev[c] = col / (a > 0.01f ? a : 1.f);
    }
    e[p] = make_float4(ev[0], ev[1], ev[2], 0.f);
    const float vx = normal[(size_t)p * 3] / m, vy = normal[(size_t)p * 3 + 1] / m, vz = normal[(size_t)p * 3 + 2] / m;
    const float len = sqrtf(vx * vx + vy * vy + vz * vz);
    guide[p] = len > 1e-3f ? make_float4(vx / len, vy / len, vz / len, 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

__device__ __forceinline__ float den_tone(float x) {
  x = fmaxf(x, 0.f);
  return x / (1.f + x);
}

// 4. one a-trous pass at tap spacing `step`: e'_p = sum h[dx] h[dy] w_pq e_q / sum h[dx] h[dy] w_pq over the taps inside the image,
// dy inner, dx outer. w_pq = w_c * w_n; the centre tap counts with w = 1 (w_c = exp(0), and g_p . g_p = 1 up to rounding).
__global__ void __launch_bounds__(256) sol_denoise_pass_kernel(const float4* __restrict__ in, const float4* __restrict__ guide,
                                                               float4* __restrict__ out, uint32_t width, uint32_t height, int step,
                                                               float inv_sigma2, float normal_power) {
  const int x = (int)(blockIdx.x * SOL_DEN_TX + (threadIdx.x & (SOL_DEN_TX - 1))), y = (int)(blockIdx.y * SOL_DEN_TY + threadIdx.x / SOL_DEN_TX);
  if (x >= (int)width || y >= (int)height) return;
  const float h[5] = {1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f};
  const size_t p = (size_t)y * width + x;
  const float4 ep = in[p], gp = guide[p];
  const float tr = den_tone(ep.x), tg = den_tone(ep.y), tb = den_tone(ep.z);
  const bool hit_p = gp.w != 0.f;
  float sr = 0.f, sg = 0.f, sb = 0.f, sw = 0.f;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int qx = x + (i - 2) * step;
    if (qx < 0 || qx >= (int)width) continue;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int qy = y + (j - 2) * step;
      if (qy < 0 || qy >= (int)height) continue;
      float w = h[i] * h[j];
      float4 eq = ep;
      if (i != 2 || j != 2) {
        const size_t q = (size_t)qy * width + qx;
        eq = in[q];
        const float4 gq = guide[q];
        const float dr = tr - den_tone(eq.x), dg = tg - den_tone(eq.y), db = tb - den_tone(eq.z);
        const float wc = expf(-(dr * dr + dg * dg + db * db) * inv_sigma2);
        const bool hit_q = gq.w != 0.f;
        float wn;
        if (hit_p != hit_q) wn = 0.f;
        else if (!hit_p) wn = 1.f;
        else wn = powf(fmaxf(0.f, gp.x * gq.x + gp.y * gq.y + gp.z * gq.z), normal_power);
        w = w * (wc * wn);
      }
      sr = sr + w * eq.x; sg = sg + w * eq.y; sb = sb + w * eq.z; sw = sw + w;
    }
  }
  out[p] = make_float4(sr / sw, sg / sw, sb / sw, 0.f);
}

// 5. out = e_K * f, written as sums (times n): the Nop tone map of these sums with n treats them as it treats a raw frame.
__global__ void __launch_bounds__(256) sol_denoise_finish_kernel(const float4* __restrict__ e, const float* __restrict__ albedo,
                                                                 float* __restrict__ out, uint32_t npix, float n, float m) {
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += gridDim.x * blockDim.x) {
    const float4 v = e[p];
    const float ev[3] = {v.x, v.y, v.z};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float a = albedo[(size_t)p * 3 + c] / m;
      out[(size_t)p * 3 + c] = (ev[c] * (a > 0.01f ? a : 1.f)) * n;
    }
  }
}

// The filter on W*H pixels; scratch = 3 * npix float4 (two ping-pong buffers + the guide). Writes W*H*3 float sums to `out` (may be `image`).
static hipError_t sol_launch_denoise(const float* image, const float* albedo, const float* normal, float* out, float4* scratch, uint32_t width,
                                     uint32_t height, uint32_t n, uint32_t m, const SolDenoise& cfg, hipStream_t stream) {
  const uint32_t npix = width * height;
  if (npix == 0) return hipSuccess;
  float4* buf[2] = {scratch, scratch + npix};
  float4* guide = scratch + 2 * (size_t)npix;
  const uint32_t grid1 = std::min<uint32_t>((npix + 255u) / 256u, 4096u);
  hipLaunchKernelGGL(sol_denoise_prepare_kernel, dim3(grid1), dim3(256), 0, stream, image, albedo, normal, buf[0], guide, npix, (float)n, (float)m);
  const dim3 grid2((width + SOL_DEN_TX - 1) / SOL_DEN_TX, (height + SOL_DEN_TY - 1) / SOL_DEN_TY);
  for (uint32_t i = 0; i < cfg.iterations; ++i) {
    const double sigma2 = (double)cfg.sigma_color * (double)cfg.sigma_color * std::ldexp(1.0, -2 * (int)i);  // sigma_color^2 * 4^-i
    hipLaunchKernelGGL(sol_denoise_pass_kernel, grid2, dim3(256), 0, stream, buf[i & 1], guide, buf[(i + 1) & 1], width, height, 1 << i,
                       (float)(1.0 / sigma2), cfg.normal_power);
  }
  hipLaunchKernelGGL(sol_denoise_finish_kernel, dim3(grid1), dim3(256), 0, stream, buf[cfg.iterations & 1], albedo, out, npix, (float)n, (float)m);
  return hipGetLastError();
}

static int den_no_device() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return sol_fail(SOL_EDEVICE, "no HIP device available");
  return SOL_OK;
}

static int denoise_impl(SolScene* s, const void* image, uint32_t n, const void* albedo, const void* normal, uint32_t m, const SolDenoise* cfg,
                        float* out, uint8_t* rgb8_host) {
  int rc = sol_denoise_check(cfg);
  if (rc != SOL_OK) return rc;
  if ((rc = den_no_device()) != SOL_OK) return rc;
  if (!s || !image || !albedo || !normal) return sol_fail(SOL_EINVAL, "sol_denoise: null argument");
  if (n == 0 || m == 0) return sol_fail(SOL_EINVAL, "sol_denoise: the colour and the auxiliary planes need at least one sample each (n %u, m %u)", n, m);
  SolDenoise c{};
  c.size = sizeof c; c.iterations = SOL_DENOISE_DEFAULT_ITERATIONS; c.sigma_color = SOL_DENOISE_DEFAULT_SIGMA_COLOR;
  c.normal_power = SOL_DENOISE_DEFAULT_NORMAL_POWER;
  if (cfg) c = *cfg;
  HIP_TRY(hipSetDevice(s->device));
  const uint32_t W = s->S.width, H = s->S.height;
  const size_t npix = (size_t)W * H;
  // scratch: ping-pong buffers, guide, and (rgb8) W*H*3 floats of result - one float4 per pixel is room enough for it
  if (const int rc = s->den_buf.reserve(s->stream, npix * 4)) return rc;
  float* dst = out ? out : (float*)(s->den_buf.get() + 3 * npix);
  HIP_TRY(sol_launch_denoise((const float*)image, (const float*)albedo, (const float*)normal, dst, s->den_buf.get(), W, H, n, m, c, s->stream));
  if (rgb8_host) {
    HIP_TRY(sol_launch_tonemap(dst, s->rgb8.get(), (uint32_t)(npix * 3), n, s->stream));
    HIP_TRY(hipMemcpyAsync(rgb8_host, s->rgb8.get(), npix * 3, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  return SOL_OK;
}

extern "C" {

int sol_denoise_check(const SolDenoise* c) {
  if (!c) return SOL_OK;
  if (c->size != sizeof(SolDenoise)) return sol_fail(SOL_EINVAL, "sol_denoise: SolDenoise.size is %u, expected %u", c->size, (unsigned)sizeof(SolDenoise));
  if (c->iterations < 1 || c->iterations > 8) return sol_fail(SOL_EINVAL, "sol_denoise: iterations must be 1..8 (got %u)", c->iterations);
  if (!std::isfinite(c->sigma_color) || !(c->sigma_color > 0.f)) return sol_fail(SOL_EINVAL, "sol_denoise: sigma_color must be finite and above 0 (got %g)", (double)c->sigma_color);
  if (!std::isfinite(c->normal_power) || c->normal_power < 0.f) return sol_fail(SOL_EINVAL, "sol_denoise: normal_power must be finite and not below 0 (got %g)", (double)c->normal_power);
  if (c->reserved[0] || c->reserved[1]) return sol_fail(SOL_EINVAL, "sol_denoise: the reserved fields of SolDenoise must be 0");
  return SOL_OK;
}

int sol_resolve_aux(SolScene* s, void** albedo_dev, void** normal_dev, uint32_t* aux_samples) {
  int rc = den_no_device();
  if (rc != SOL_OK) return rc;
  if (!s) return sol_fail(SOL_EINVAL, "null scene");
  if (s->world > 1) return sol_fail(SOL_EINVAL, "sol_resolve_aux: the auxiliary planes are rank-local (world %d); the denoiser renders on one rank", s->world);
  if (!s->aux[0] || s->aux_floats != s->acc_floats) return sol_fail(SOL_EINVAL, "sol_resolve_aux: no auxiliary planes: call sol_render_aux first");
  HIP_TRY(hipSetDevice(s->device));
  const size_t floats = (size_t)s->S.width * s->S.height * 3;
  void** outs[2] = {albedo_dev, normal_dev};
  for (int k = 0; k < 2; ++k) {
    if (const int rc = s->aux_img[k].reserve(s->stream, floats)) return rc;
    HIP_TRY(sol_launch_unpermute(s->aux[k].get(), s->aux_img[k].get(), s->S.width, s->S.height, s->blocks_x, (uint32_t)s->world, (uint32_t)s->rank,
                                 s->acc_floats, s->slot_of_block.get(), s->stream));
    if (outs[k]) *outs[k] = s->aux_img[k].get();
  }
  if (aux_samples) *aux_samples = s->aux_samples;
  return SOL_OK;
}

int sol_denoise(SolScene* s, void* image_dev, uint32_t n, const void* albedo_dev, const void* normal_dev, uint32_t m, const SolDenoise* cfg) {
  return denoise_impl(s, image_dev, n, albedo_dev, normal_dev, m, cfg, (float*)image_dev, nullptr);
}

int sol_denoise_rgb8(SolScene* s, const void* image_dev, uint32_t n, const void* albedo_dev, const void* normal_dev, uint32_t m, const SolDenoise* cfg,
                     uint8_t* rgb8_host) {
  if (!rgb8_host) {
    int rc = sol_denoise_check(cfg);
    return rc != SOL_OK ? rc : sol_fail(SOL_EINVAL, "sol_denoise_rgb8: null argument");
  }
  return denoise_impl(s, image_dev, n, albedo_dev, normal_dev, m, cfg, nullptr, rgb8_host);
}

}  // extern "C"
