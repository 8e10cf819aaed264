// sol_lights.hip -- light tree and power-weighted light sampling (include/solstrale_hip.h, sol_light_*): the tree and the
// selection tables the LT render kernels read, and the diagnostics that read them back or run the device's own sum and selection.
//
// Tree. An implicit complete 4-ary tree over the light list IN LIST ORDER: depth D = the least with 4^D >= L, leaf i = node
// (4^D - 1) / 3 + i, children of node n = 4n + 1 .. 4n + 4, no pointers. Leaves L .. 4^D - 1 are empty boxes (min +inf, max -inf). A
// leaf box bounds the device record light_pdf_value reads (DQuad: q, q + u, q + v, q + u + v; DTri: v0, v0 + e1, v0 + e2; corners in
// fp32; DSphere: centre -+ |r|), padded outward by the scene's box pad (2 x DevScene::sphere_slack; never less than 2^-20 x the leaf's own
// largest |coordinate|). A node box is the min / max of its children's. Built on the scene's stream: one launch for the leaves, one per
// level above them, min / max only - bit-identical on every device, rank and run.
//
// Weights (mode 2). w_i = area_i x Y_i in f64 from the description (sol_light_weights_of): area = the quad's or triangle's `area`, 4 pi r^2
// for a sphere; Y = 0.2126 R + 0.7152 G + 0.0722 B of the DiffuseLight's texture (solid: its colour; image: the mean texel / 255);
// attenuation ignored; any other material or primitive, or a w that is not finite and above 0: w = 0. W = sum in list order (f64),
// C_i = (float)(prefix_i / W), C_{L-1} = 1.0f, q_i = C_i - C_{i-1} (fp32, C_{-1} = 0).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "sol_scene.h"
#include "sol_shade.h"

#define SOL_LT_MAX_LIGHTS (1u << 30)  // (node indices of the tree stay within 32 bits)

// One thread per leaf (4^D of them): the padded box of light i, or an empty box.
__global__ void __launch_bounds__(256) sol_light_leaves_kernel(const DevScene S, uint32_t n_leaves, uint32_t first, float pad, float* __restrict__ nodes) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_leaves) return;
  const float inf = __builtin_huge_valf();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  auto take = [&](float x, float y, float z) {
    lo[0] = fminf(lo[0], x); lo[1] = fminf(lo[1], y); lo[2] = fminf(lo[2], z);
    hi[0] = fmaxf(hi[0], x); hi[1] = fmaxf(hi[1], y); hi[2] = fmaxf(hi[2], z);
  };
  bool have = false;
  if (i < S.n_lights) {
    const uint32_t ref = S.lights[i], kind = SOL_REF_KIND(ref), idx = SOL_REF_INDEX(ref);
    if (kind == SOL_REF_QUAD) {
      const DQuad Q = S.quads[idx];
      const float ax = Q.qx + Q.ux, ay = Q.qy + Q.uy, az = Q.qz + Q.uz;
      take(Q.qx, Q.qy, Q.qz);
      take(ax, ay, az);
      take(Q.qx + Q.vx, Q.qy + Q.vy, Q.qz + Q.vz);
      take(ax + Q.vx, ay + Q.vy, az + Q.vz);
      have = true;
    } else if (kind == SOL_REF_TRIANGLE) {
      const DTri T = S.tris[idx];
      take(T.v0x, T.v0y, T.v0z);
      take(T.v0x + T.e1x, T.v0y + T.e1y, T.v0z + T.e1z);
      take(T.v0x + T.e2x, T.v0y + T.e2y, T.v0z + T.e2z);
      have = true;
    } else if (kind == SOL_REF_SPHERE) {
      const DSphere Sp = S.spheres[idx];
      const float r = fabsf(Sp.radius);
      take(Sp.cx - r, Sp.cy - r, Sp.cz - r);
      take(Sp.cx + r, Sp.cy + r, Sp.cz + r);
      have = true;
    }
  }
  float* o = nodes + (size_t)(first + i) * 6u;
  if (!have) {  // (padding, or a reference light_pdf_value gives 0 for)
    o[0] = o[1] = o[2] = inf;
    o[3] = o[4] = o[5] = -inf;
    return;
  }
  float m = 0.0f;
  for (int k = 0; k < 3; ++k) m = fmaxf(m, fmaxf(fabsf(lo[k]), fabsf(hi[k])));
  const float p = fmaxf(pad, m * (1.0f / 1048576.0f));  // (NaN coordinates: fmaxf keeps the pad; the box then has NaN planes, which the slab ignores)
  for (int k = 0; k < 3; ++k) {
    o[k] = lo[k] - p;
    o[3 + k] = hi[k] + p;
  }
}
// One thread per node of one level: the union of its four children.
__global__ void __launch_bounds__(256) sol_light_level_kernel(float* __restrict__ nodes, uint32_t begin, uint32_t count) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= count) return;
  const uint32_t n = begin + k;
  const float* c = nodes + (size_t)(4u * n + 1u) * 6u;
  float b[6] = {c[0], c[1], c[2], c[3], c[4], c[5]};
  for (int j = 1; j < 4; ++j) {
    const float* d = c + 6 * j;
    for (int a = 0; a < 3; ++a) {
      b[a] = fminf(b[a], d[a]);
      b[3 + a] = fmaxf(b[3 + a], d[3 + a]);
    }
  }
  float* o = nodes + (size_t)n * 6u;
  for (int a = 0; a < 6; ++a) o[a] = b[a];
}
// sol_light_eval: fn 0 (origin xyz, dir xyz) -> (loop density, tree density, node visits, light tests) with the render kernels' own
// functions; fn 1 u -> the light mode 2 selects.
template <bool ENV>
__global__ void __launch_bounds__(256) sol_light_eval_kernel(const DevScene S, uint32_t fn, const float* __restrict__ in, uint32_t n, float* __restrict__ out) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  if (fn == 1) {
    out[k] = (float)light_select(S, in[k]);
    return;
  }
  const float* r = in + 6 * (size_t)k;
  const f3 o = mk3(r[0], r[1], r[2]), d = mk3(r[3], r[4], r[5]);
  Counters cnt{};
  uint32_t visits = 0, tests = 0, lv = 0, lt = 0;
  const float loop = S.light_power ? light_mix<ENV>(S, light_sum<false, false, false, true>(S, o, d, cnt, lv, lt), d)
                                   : container_pdf_value<false, false, ENV>(S, o, d, cnt);  // (modes 0 and 1: the default kernels' own function)
  const float tree = light_mix<ENV>(S, light_sum<false, false, true, true>(S, o, d, cnt, visits, tests), d);
  float* w = out + 4 * (size_t)k;
  w[0] = loop; w[1] = tree; w[2] = (float)visits; w[3] = (float)tests;
}

static double light_luminance(const SolSceneDesc* d, int32_t mat) {
  if (mat < 0 || (uint32_t)mat >= d->n_materials || !d->materials) return 0.0;
  const SolMaterial& m = d->materials[mat];
  if (m.kind != SOL_MAT_DIFFUSE_LIGHT || m.albedo_tex < 0 || (uint32_t)m.albedo_tex >= d->n_textures || !d->textures) return 0.0;
  const SolTexture& t = d->textures[m.albedo_tex];
  double rgb[3] = {0.0, 0.0, 0.0};
  if (t.kind == SOL_TEX_SOLID) {
    for (int c = 0; c < 3; ++c) rgb[c] = t.rgb[c];
  } else if (t.kind == SOL_TEX_IMAGE) {
    const uint64_t n = (uint64_t)t.width * t.height;
    if (n == 0 || !d->texels || t.texel_offset > d->n_texel_bytes || 3 * n > d->n_texel_bytes - t.texel_offset) return 0.0;
    const uint8_t* p = d->texels + t.texel_offset;
    for (uint64_t k = 0; k < n; ++k)
      for (int c = 0; c < 3; ++c) rgb[c] += (double)p[3 * k + c] / 255.0;  // rgb_to_vec3
    for (int c = 0; c < 3; ++c) rgb[c] /= (double)n;
  }
  return 0.2126 * rgb[0] + 0.7152 * rgb[1] + 0.0722 * rgb[2];
}

std::vector<double> sol_light_weights_of(const SolSceneDesc* d) {
  std::vector<double> w;
  if (!d || !d->lights) return w;
  w.assign(d->n_lights, 0.0);
  for (uint32_t i = 0; i < d->n_lights; ++i) {
    const uint32_t kind = SOL_REF_KIND(d->lights[i]), idx = SOL_REF_INDEX(d->lights[i]);
    double area = 0.0;
    int32_t mat = -1;
    if (kind == SOL_REF_QUAD && idx < d->n_quads && d->quads) { area = d->quads[idx].area; mat = d->quads[idx].material; }
    else if (kind == SOL_REF_TRIANGLE && idx < d->n_triangles && d->triangles) { area = d->triangles[idx].area; mat = d->triangles[idx].material; }
    else if (kind == SOL_REF_SPHERE && idx < d->n_spheres && d->spheres) {
      const double r = d->spheres[idx].radius;
      area = 4.0 * 3.14159265358979323846 * r * r;
      mat = d->spheres[idx].material;
    }
    const double v = area * light_luminance(d, mat);
    w[i] = (v > 0.0 && std::isfinite(v)) ? v : 0.0;
  }
  return w;
}

// The luminance factor alone, per light: what a geometry move (sol_geometry.cpp) multiplies the new areas of the triangle lights with.
std::vector<double> sol_light_luminances_of(const SolSceneDesc* d) {
  std::vector<double> y;
  if (!d || !d->lights) return y;
  y.assign(d->n_lights, 0.0);
  for (uint32_t i = 0; i < d->n_lights; ++i) {
    const uint32_t kind = SOL_REF_KIND(d->lights[i]), idx = SOL_REF_INDEX(d->lights[i]);
    int32_t mat = -1;
    if (kind == SOL_REF_QUAD && idx < d->n_quads && d->quads) mat = d->quads[idx].material;
    else if (kind == SOL_REF_TRIANGLE && idx < d->n_triangles && d->triangles) mat = d->triangles[idx].material;
    else if (kind == SOL_REF_SPHERE && idx < d->n_spheres && d->spheres) mat = d->spheres[idx].material;
    y[i] = light_luminance(d, mat);
  }
  return y;
}

// q_i and C_i (above) from the weights; W = 0: nothing can be drawn.
static double light_tables_of(const std::vector<double>& w, std::vector<float>& q, std::vector<float>& cdf) {
  const size_t L = w.size();
  double W = 0.0;
  for (double x : w) W += x;
  q.assign(L, 0.0f);
  cdf.assign(L, 0.0f);
  if (!(W > 0.0)) return W;
  double prefix = 0.0;
  float prev = 0.0f;
  for (size_t i = 0; i < L; ++i) {
    prefix += w[i];
    cdf[i] = i + 1 == L ? 1.0f : (float)(prefix / W);
    q[i] = cdf[i] - prev;
    prev = cdf[i];
  }
  return W;
}

static int light_config_check(const SolLightSampling* c, const char* fn) {
  if (!c) return SOL_OK;  // (NULL: uniform)
  if (c->size < sizeof(SolLightSampling)) return sol_fail(SOL_EINVAL, "%s: SolLightSampling.size %u < %zu", fn, c->size, sizeof(SolLightSampling));
  if (c->mode > SOL_LIGHT_SAMPLING_POWER) return sol_fail(SOL_EINVAL, "%s: unknown mode %u (0 uniform, 1 tree, 2 power)", fn, c->mode);
  if (c->reserved[0] || c->reserved[1]) return sol_fail(SOL_EINVAL, "%s: reserved fields must be 0", fn);
  return SOL_OK;
}
static int light_scene_check(uint32_t mode, uint32_t n_lights, double total, const char* fn) {
  if (mode != SOL_LIGHT_SAMPLING_UNIFORM && n_lights > SOL_LT_MAX_LIGHTS) return sol_fail(SOL_EINVAL, "%s: more than 2^30 lights", fn);
  if (mode == SOL_LIGHT_SAMPLING_POWER && !(total > 0.0))
    return sol_fail(SOL_EINVAL, "%s: every light has power 0 (area x luminance of a DiffuseLight's emission), mode 2 cannot select", fn);
  return SOL_OK;
}

static int light_tree_build(SolScene* s) {
  const uint32_t L = s->S.n_lights;
  uint32_t depth = 0;
  uint64_t leaves = 1;
  while (leaves < L) { leaves *= 4u; ++depth; }
  const uint64_t first = (leaves - 1u) / 3u, total = (4u * leaves - 1u) / 3u;
  DevPtr<float> tree;
  if (sol_dev_alloc(tree, (size_t)total * 6u) != hipSuccess) return sol_fail(SOL_ENOMEM, "sol_light_sampling: no memory for the light tree");
  float* const t = tree.get();
  hipLaunchKernelGGL(sol_light_leaves_kernel, dim3((uint32_t)((leaves + 255u) / 256u)), dim3(256), 0, s->stream, s->S, (uint32_t)leaves, (uint32_t)first,
                     2.0f * s->S.sphere_slack, t);
  for (uint32_t l = depth; l-- > 0;) {  // levels bottom-up: level l holds nodes (4^l - 1) / 3 .. (4^(l+1) - 1) / 3 - 1
    const uint64_t count = 1ull << (2u * l), begin = (count - 1u) / 3u;
    hipLaunchKernelGGL(sol_light_level_kernel, dim3((uint32_t)((count + 255u) / 256u)), dim3(256), 0, s->stream, t, (uint32_t)begin, (uint32_t)count);
  }
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  if (e != hipSuccess) return sol_fail(SOL_EDEVICE, "sol_light_sampling: %s", hipGetErrorString(e));
  s->light_tree = std::move(tree);
  s->light_tree_bytes = (size_t)total * 6u * sizeof(float);
  s->S.light_nodes = t;
  s->S.light_first_leaf = (uint32_t)first;
  return SOL_OK;
}

static int light_tables_build(SolScene* s) {
  std::vector<float> q, cdf;
  light_tables_of(s->light_w, q, cdf);
  const size_t L = q.size();
  DevPtr<float> tables;
  if (sol_dev_alloc(tables, 2 * L) != hipSuccess) return sol_fail(SOL_ENOMEM, "sol_light_sampling: no memory for the tables");
  float* const t = tables.get();
  hipError_t e = hipMemcpyAsync(t, q.data(), L * sizeof(float), hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(t + L, cdf.data(), L * sizeof(float), hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  if (e != hipSuccess) return sol_fail(SOL_EDEVICE, "sol_light_sampling: %s", hipGetErrorString(e));
  s->light_tables = std::move(tables);
  s->S.light_q = t;
  s->S.light_cdf = t + L;
  return SOL_OK;
}

// After a geometry move: the light records, the box pad and s->light_w have changed - what was built from them is built again.
int sol_light_rebuild(SolScene* s) {
  int rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (s->light_tree) {
    s->light_tree.reset(); s->light_tree_bytes = 0; s->S.light_nodes = nullptr;
    if ((rc = light_tree_build(s))) return rc;
  }
  if (s->light_tables) {
    s->light_tables.reset(); s->S.light_q = nullptr; s->S.light_cdf = nullptr;
    if ((rc = light_tables_build(s))) return rc;
  }
  return SOL_OK;
}

extern "C" {

int sol_light_weights(const SolSceneDesc* desc, double* w, size_t n) {
  if (!desc || (!w && n)) return sol_fail(SOL_EINVAL, "null argument");
  if (n < desc->n_lights) return sol_fail(SOL_EINVAL, "sol_light_weights: %u lights, room for %zu", desc->n_lights, n);
  const std::vector<double> v = sol_light_weights_of(desc);
  std::copy(v.begin(), v.end(), w);
  return SOL_OK;
}

int sol_light_sampling_check(const SolSceneDesc* desc, const SolLightSampling* config) {
  int rc = light_config_check(config, "sol_light_sampling_check");
  if (rc) return rc;
  if (!desc) return sol_fail(SOL_EINVAL, "null scene description");
  const uint32_t mode = config ? config->mode : SOL_LIGHT_SAMPLING_UNIFORM;
  double total = 0.0;
  if (mode == SOL_LIGHT_SAMPLING_POWER)
    for (double x : sol_light_weights_of(desc)) total += x;
  return light_scene_check(mode, desc->n_lights, total, "sol_light_sampling_check");
}

int sol_light_sampling(SolScene* s, const SolLightSampling* config) {
  int rc = light_config_check(config, "sol_light_sampling");  // (the configuration first: its errors do not need a device)
  if (rc) return rc;
  if (!s) return sol_fail(SOL_EINVAL, "null scene");
  const uint32_t mode = config ? config->mode : SOL_LIGHT_SAMPLING_UNIFORM;
  if (!s->light_total)
    for (double x : s->light_w) s->light_total += x;
  if ((rc = light_scene_check(mode, s->S.n_lights, s->light_total, "sol_light_sampling"))) return rc;
  if (mode != SOL_LIGHT_SAMPLING_UNIFORM) {
    HIP_TRY(hipSetDevice(s->device));
    if (!s->light_tree && (rc = light_tree_build(s))) return rc;
    if (mode == SOL_LIGHT_SAMPLING_POWER && !s->light_tables && (rc = light_tables_build(s))) return rc;
  }
  if (mode != s->light_mode) s->adaptive.open = false;  // (a session's rounds all use one estimator)
  s->light_mode = mode;
  s->S.light_power = mode == SOL_LIGHT_SAMPLING_POWER ? 1u : 0u;
  return SOL_OK;
}

int sol_light_tables(SolScene* s, float* q, float* cdf, size_t n, double* total) {
  if (!s) return sol_fail(SOL_EINVAL, "null scene");
  if (!s->light_tables) return sol_fail(SOL_EINVAL, "sol_light_tables: no tables (sol_light_sampling with mode 2 builds them)");
  const size_t L = s->S.n_lights;
  if ((q || cdf) && n < L) return sol_fail(SOL_EINVAL, "sol_light_tables: the tables hold %zu floats (%zu given)", L, n);
  HIP_TRY(hipSetDevice(s->device));
  if (q) HIP_TRY(hipMemcpyAsync(q, s->S.light_q, L * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  if (cdf) HIP_TRY(hipMemcpyAsync(cdf, s->S.light_cdf, L * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (total) *total = s->light_total;
  return SOL_OK;
}

int sol_light_tree(SolScene* s, float* nodes, size_t n_floats, uint32_t* n_nodes, uint32_t* first_leaf, size_t* bytes) {
  if (!s) return sol_fail(SOL_EINVAL, "null scene");
  if (!s->light_tree) return sol_fail(SOL_EINVAL, "sol_light_tree: no tree (sol_light_sampling with mode 1 or 2 builds it)");
  const size_t nf = s->light_tree_bytes / sizeof(float);
  if (nodes && n_floats < nf) return sol_fail(SOL_EINVAL, "sol_light_tree: the tree holds %zu floats (%zu given)", nf, n_floats);
  if (n_nodes) *n_nodes = (uint32_t)(nf / 6u);
  if (first_leaf) *first_leaf = s->S.light_first_leaf;
  if (bytes) *bytes = s->light_tree_bytes;
  if (nodes) {
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpyAsync(nodes, s->light_tree.get(), s->light_tree_bytes, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  return SOL_OK;
}

int sol_light_eval(SolScene* s, uint32_t fn, const float* in, uint32_t n, float* out) {
  if (!s || !in || !out) return sol_fail(SOL_EINVAL, "null argument");
  if (fn > 1u) return sol_fail(SOL_EINVAL, "sol_light_eval: unknown function %u (0 density, 1 selection)", fn);
  if (fn == 0 && !s->light_tree) return sol_fail(SOL_EINVAL, "sol_light_eval: no tree (sol_light_sampling with mode 1 or 2 builds it)");
  if (fn == 1 && !s->light_tables) return sol_fail(SOL_EINVAL, "sol_light_eval: no tables (sol_light_sampling with mode 2 builds them)");
  if (n == 0) return SOL_OK;
  if (n > (1u << 26)) return sol_fail(SOL_EINVAL, "sol_light_eval: more than 2^26 rows");
  HIP_TRY(hipSetDevice(s->device));
  const size_t ib = (size_t)n * (fn == 0 ? 6 : 1) * sizeof(float), ob = (size_t)n * (fn == 0 ? 4 : 1) * sizeof(float);
  DevPtr<float> din_own, dout_own;
  HIP_TRY(sol_dev_alloc(din_own, ib / sizeof(float)));
  if (sol_dev_alloc(dout_own, ob / sizeof(float)) != hipSuccess) return sol_fail(SOL_ENOMEM, "hipMalloc failed");
  float *const din = din_own.get(), *const dout = dout_own.get();
  hipError_t e = hipMemcpyAsync(din, in, ib, hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) {
    DevScene S = s->S;
    S.light_power = fn == 1 ? 1u : S.light_power;
    if (s->env_is) hipLaunchKernelGGL(sol_light_eval_kernel<true>, dim3((n + 255u) / 256u), dim3(256), 0, s->stream, S, fn, (const float*)din, n, dout);
    else hipLaunchKernelGGL(sol_light_eval_kernel<false>, dim3((n + 255u) / 256u), dim3(256), 0, s->stream, S, fn, (const float*)din, n, dout);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout, ob, hipMemcpyDeviceToHost, s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  if (e != hipSuccess) return sol_fail(SOL_EDEVICE, "sol_light_eval: %s", hipGetErrorString(e));
  return SOL_OK;
}

}  // extern "C"
