/*
 * solstrale_hip.h -- C ABI of the MI355X (gfx950) path-tracing library `libsolstrale_hip.so`.
 *
 * This is the drop-in boundary for ONE hot path of DanielPettersson/Solstrale-Rust: the body of the
 * per-pass row loop of `Renderer::render` (reference src/renderer/mod.rs:241-291), i.e. everything under
 * `Renderer::ray_color` (src/renderer/mod.rs:164-206): BVH closest hit (src/hittable/), material scatter
 * and pdf importance sampling (src/material/mod.rs, src/pdf.rs), camera rays (src/camera.rs:77-89) and the
 * per-pixel accumulation (src/renderer/mod.rs:268,361-365).
 *
 * The reference has no FFI of its own on this path: the host (Rust `Renderer`, or the C++
 * mirror in solstrale-rust_amd/host/) keeps scene loading, the BVH builder (src/hittable/bvh.rs:61-162),
 * Camera::new (src/camera.rs:47-74), the pass loop, progress reporting and post-processing; it flattens its
 * `Hittables` tree into the POD arrays below and calls sol_scene_create / sol_render / sol_read.
 *
 * Every struct mirrors the fields of a reference type, in f64 exactly as the reference holds them; the
 * library converts to its fp32 device layout on upload (DESIGN.md "Data layout in HBM").
 *
 * All functions return 0 on success, a negative SOL_E* code otherwise; sol_last_error() gives the
 * thread-local message. Nothing here aborts the process. No torch types appear in any signature.
 */
#ifndef SOLSTRALE_HIP_H
#define SOLSTRALE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SOL_ABI_VERSION 2  /* 2: SolSceneDesc ends with the optional environment map; a version-1 description (without those
                           * fields) is still accepted */

/* ---- error codes ---------------------------------------------------------------------------------- */
#define SOL_OK 0
#define SOL_EINVAL (-1)    /* malformed description / argument                                         */
#define SOL_ENOLIGHT (-2)  /* "Scene should have at least one light" (src/renderer/mod.rs:143-147)      */
#define SOL_EDEVICE (-3)   /* HIP runtime error / no GPU                                               */
#define SOL_EDEPTH (-4)    /* BVH deeper than the traversal stack supports                             */
#define SOL_ENOMEM (-5)
#define SOL_ERANGE (-6)    /* sol_scene_set_triangles / sol_scene_set_primitives: the moved geometry leaves the exponent range of the tree - re-create the scene */

/* ---- child / primitive references ------------------------------------------------------------------
 * A 32-bit reference: kind in bits 31..28, index into the array of that kind in bits 27..0.
 * Mirrors `BvhItem::{Node, Leaf(Box<Hittables>), None}` (src/hittable/bvh.rs:21-25) with the leaf's
 * `Hittables` variant (src/hittable/mod.rs:47-61) made explicit. A nested `Bvh` held in a Leaf is
 * inlined by the flattener as SOL_REF_NODE (Bvh::hit is the same function, so this is exact). */
#define SOL_REF_NONE 0u
#define SOL_REF_NODE 1u
#define SOL_REF_SPHERE 2u
#define SOL_REF_QUAD 3u
#define SOL_REF_TRIANGLE 4u
#define SOL_REF_MEDIUM 5u
#define SOL_REF_KIND(r) ((uint32_t)(r) >> 28)
#define SOL_REF_INDEX(r) ((uint32_t)(r) & 0x0FFFFFFFu)
#define SOL_MAKE_REF(kind, index) ((((uint32_t)(kind)) << 28) | ((uint32_t)(index) & 0x0FFFFFFFu))

/* Axis-aligned box, `Aabb{x,y,z: Interval{min,max}}` (src/geo/mod.rs:39-46): xmin,xmax,ymin,ymax,zmin,zmax */
typedef struct SolAabb {
  double v[6];
} SolAabb;

/* `Bvh{left,right,b_box}` (src/hittable/bvh.rs:14-18) */
typedef struct SolBvhNode {
  SolAabb bbox;
  uint32_t left;  /* SOL_MAKE_REF(...) */
  uint32_t right; /* SOL_MAKE_REF(...) */
} SolBvhNode;

/* `Sphere{center,radius,mat,b_box}` (src/hittable/sphere.rs:15-20) */
typedef struct SolSphere {
  double center[3];
  double radius;
  SolAabb bbox;
  int32_t material;
  uint32_t dfs_index; /* position in the depth-first leaf order of the world tree (tie rule) - see below */
} SolSphere;
/* dfs_index (SolSphere, SolQuad, SolTriangle, SolMedium) decides which of two equal hits wins and which flat primitive a scattered ray
 * leaves (the tie rule and rule 8), so it is checked: walk the world tree in pre-order from `root`, left child before right;
 * every sphere, quad, triangle or medium the walk reaches takes the next number (0, 1, 2 ...), a medium before its boundary sub-tree is
 * walked, the walk going on after the boundary. A record reached more than once (a shared sub-tree) takes the number of its LAST
 * visit. Every reached record must carry exactly its number, or sol_scene_create, sol_world_tree_check(_ex) and sol_background_blocks
 * return SOL_EINVAL naming the record, the value found and the one expected. Records the walk never reaches (a light outside the
 * world) are not checked. The host library's flattening emits this numbering. */

/* `Quad{q,u,v,normal,d,w,mat,b_box,area}` (src/hittable/quad.rs:19-29) */
typedef struct SolQuad {
  double q[3], u[3], v[3], normal[3];
  double d;
  double w[3];
  double area;
  SolAabb bbox;
  int32_t material;
  uint32_t dfs_index;
} SolQuad;

/* `Triangle{v0,v0v1,v0v2,uv0..2,normal,tangent,bi_tangent,mat,b_box,area}` (src/hittable/triangle.rs:14-27) */
typedef struct SolTriangle {
  double v0[3], v0v1[3], v0v2[3];
  double normal[3], tangent[3], bi_tangent[3];
  double area;
  float uv0[2], uv1[2], uv2[2]; /* `Uv{f32,f32}` (src/geo/mod.rs:15-20) */
  SolAabb bbox;
  int32_t material;
  uint32_t dfs_index;
} SolTriangle;

/* `ConstantMedium{boundary,negative_inverse_density,phase_function}` (src/hittable/constant_medium.rs:14-19) */
typedef struct SolMedium {
  uint32_t boundary; /* reference to the boundary hittable (its own sub-tree of nodes/prims)            */
  int32_t material;  /* the Isotropic phase function                                                    */
  double negative_inverse_density;
  SolAabb bbox;
  uint32_t dfs_index;
  uint32_t _pad;
} SolMedium;

/* `Materials` (src/material/mod.rs:134-150) */
#define SOL_MAT_LAMBERTIAN 0
#define SOL_MAT_METAL 1
#define SOL_MAT_DIELECTRIC 2
#define SOL_MAT_DIFFUSE_LIGHT 3
#define SOL_MAT_ISOTROPIC 4
#define SOL_MAT_BLEND 5
typedef struct SolMaterial {
  int32_t kind;
  int32_t albedo_tex; /* Lambertian/Metal/Dielectric.albedo, DiffuseLight.tex, Isotropic.tex; -1 for Blend */
  int32_t normal_tex; /* `normal: Option<Textures>`; -1 = None                                          */
  int32_t m1, m2;     /* Blend.material_1 / material_2 (indices into materials), else -1                 */
  int32_t _pad;
  /* Metal.fuzz | Dielectric.index_of_refraction | Blend.blend_factor |
   * DiffuseLight.attenuation_factor with NaN standing for `None` (src/material/mod.rs:320-340) */
  double param;
} SolMaterial;

/* `Textures::{SolidColor(Vec3), ImageMap{image,max_x,max_y}}` (src/material/texture.rs:26-33,101,128-133) */
#define SOL_TEX_SOLID 0
#define SOL_TEX_IMAGE 1
typedef struct SolTexture {
  int32_t kind;
  uint32_t width, height; /* image only                                                                */
  uint32_t _pad;
  uint64_t texel_offset; /* byte offset of the first RGB8 texel in SolSceneDesc.texels                 */
  double rgb[3];         /* solid colour                                                               */
} SolTexture;

/* `Camera{origin,lower_left_corner,horizontal,vertical,u,v,lens_radius}` (src/camera.rs:35-43),
 * produced on the host by Camera::new (src/camera.rs:47-74). */
typedef struct SolCamera {
  double origin[3], lower_left_corner[3], horizontal[3], vertical[3], u[3], v[3];
  double lens_radius;
} SolCamera;

/* `Shaders` (src/renderer/shader.rs:33-44) */
#define SOL_SHADER_PATH_TRACING 0
#define SOL_SHADER_ALBEDO 1
#define SOL_SHADER_NORMAL 2
#define SOL_SHADER_SIMPLE 3

typedef struct SolSceneDesc {
  uint32_t abi_version; /* SOL_ABI_VERSION */
  uint32_t width, height; /* RenderConfig.width/height (src/renderer/mod.rs:26-30)                      */
  uint32_t shader_kind;   /* SOL_SHADER_*                                                               */
  uint32_t max_depth;     /* PathTracingShader.max_depth (src/renderer/shader.rs:48-50)                 */
  uint32_t root;          /* reference to `Scene.world` (src/renderer/mod.rs:63-72)                     */
  double background[3];   /* Scene.background_color                                                     */
  SolCamera camera;

  const SolBvhNode* nodes;      uint32_t n_nodes;
  const SolSphere* spheres;     uint32_t n_spheres;
  const SolQuad* quads;         uint32_t n_quads;
  const SolTriangle* triangles; uint32_t n_triangles;
  const SolMedium* mediums;     uint32_t n_mediums;
  const SolMaterial* materials; uint32_t n_materials;
  const SolTexture* textures;   uint32_t n_textures;
  const uint8_t* texels;        uint64_t n_texel_bytes;
  /* `Renderer.lights` = world.get_lights() in depth-first order (src/renderer/mod.rs:126,141;
   * src/hittable/bvh.rs:186-193): references to light primitives */
  const uint32_t* lights;       uint32_t n_lights;
  /* ---- abi_version >= 2: EXTENSION, not in the reference (which only has the constant `background_color`,
   * src/renderer/mod.rs:197-204; BASELINE.json config 5 names an "HDRI env light"). A latitude-longitude map of linear RGB
   * radiance, fp32, row 0 = up (+y): a ray that hits nothing returns env_scale * texel(direction) instead of `background`.
   * The direction is mapped like a point on the reference's unit sphere (calculate_sphere_uv, src/hittable/sphere.rs:134-140)
   * and the texel picked like an ImageMap's (nearest, src/material/texture.rs:170-179). By default it is NOT importance-sampled
   * (a ray finds it only when the BSDF's direction escapes); sol_env_sampling turns on sampling it as one more light (opt-in,
   * DESIGN.md 12). The scene still needs a light (Renderer::new). env_texels == NULL (or width/height 0) = no environment. */
  const float* env_texels;      uint32_t env_width, env_height;
  double env_scale;
} SolSceneDesc;

/* fp32 arithmetic contract, vertex order of a triangle's fp32 record. Moller-Trumbore works in the frame (v0; e1 = v1 - v0, e2 = v2 - v0);
 * its rounding error grows with |e1| |e2| / sin(angle between them), i.e. - the area being what it is - with the product of the two
 * edge lengths at v0. The fp32 records (device, and the oracle's float instantiation) therefore start at the vertex OPPOSITE THE LONGEST
 * EDGE: a cyclic rotation (v0, v1, v2) -> (v_k, v_k+1, v_k+2) - same winding, same normal, same set of points; the texture
 * coordinates rotate along, so the interpolated values are the same numbers up to rounding. k = 0 unless another start is strictly
 * better. A triangle that is a LIGHT is INTERSECTED through its rotated record like any other and SAMPLED in the reference's own
 * frame (Triangle::random_direction draws from the parallelogram at the first vertex, triangle.rs:114-117 - a set that depends on the
 * start): both sides keep the unrotated (v0, v0v1, v0v2) of every triangle light for that. For a strip-shaped needle of aspect 300:1
 * the rotation takes the test's noise down by that factor. f64 is untouched. */
static inline int sol_triangle_rotation(const SolTriangle* t) {
  const double a[3] = {t->v0v1[0], t->v0v1[1], t->v0v1[2]}, b[3] = {t->v0v2[0], t->v0v2[1], t->v0v2[2]};
  const double c[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const double l01 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2], l02 = b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
  const double l12 = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
  /* start k: the edge opposite v_k is v_k+1 v_k+2: k = 0: v1v2 (l12), k = 1: v2v0 (l02), k = 2: v0v1 (l01) */
  int k = 0;
  double best = l12;
  if (l02 > best) { best = l02; k = 1; }
  if (l01 > best) { k = 2; }
  return k;
}
/* The rotated record: vertex, two edges and the order of the three texture coordinates (index into {uv0, uv1, uv2}). */
static inline void sol_triangle_rotated(const SolTriangle* t, int k, double v0[3], double e1[3], double e2[3], int uv_of[3]) {
  int i;
  for (i = 0; i < 3; ++i) {
    const double p0 = t->v0[i], a = t->v0v1[i], b = t->v0v2[i];
    if (k == 1) { v0[i] = p0 + a; e1[i] = b - a; e2[i] = -a; }
    else if (k == 2) { v0[i] = p0 + b; e1[i] = -b; e2[i] = a - b; }
    else { v0[i] = p0; e1[i] = a; e2[i] = b; }
  }
  uv_of[0] = k % 3; uv_of[1] = (k + 1) % 3; uv_of[2] = (k + 2) % 3;
}

/* fp32 arithmetic contract, needle triangles. fp32 Moller-Trumbore (src/hittable/triangle.rs:119-140 in single
 * precision) is ill-conditioned for triangles of extreme aspect: it accepts rays that pass many box pads beside the triangle (hundreds, in the
 * reference's vertex order; the rotation above leaves about one candidate in 10^5 beyond ONE thin pad on a mesh with 300:1 rods),
 * and whether such a phantom is seen would depend on which boxes a traversal tested. A scene HAS NEEDLES when some triangle's
 * longest edge squared is at least 2 * 32 times its area (aspect >= 32:1). For such scenes the fp32 contract - the device and the
 * oracle's float instantiation alike; in f64 nothing changes - (i) pads every box by SOL_NEEDLE_PAD * S * 2^-20 instead of S * 2^-20 and (ii)
 * counts a triangle hit only if the ray's point o + t*d and the triangle's point v0 + u*e1 + v*e2 agree within 0.8 pads in
 * every coordinate: an accepted hit then lies inside every box around its part of the triangle, whatever the tree. Both sides decide
 * with THIS function. */
#ifndef SOL_NEEDLE_ASPECT
#define SOL_NEEDLE_ASPECT 32.0
#endif
#ifndef SOL_NEEDLE_PAD
#define SOL_NEEDLE_PAD 4.0f /* such scenes' box pad, in thin pads (S * 2^-20); the rule's tolerance is 0.8 of it */
#endif
static inline int sol_scene_has_needles(const SolSceneDesc* d) {
  uint32_t i;
  for (i = 0; i < d->n_triangles; ++i) {
    const SolTriangle* t = &d->triangles[i];
    const double a[3] = {t->v0v1[0], t->v0v1[1], t->v0v1[2]}, b[3] = {t->v0v2[0], t->v0v2[1], t->v0v2[2]};
    const double c[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    double l2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
    const double lb = b[0] * b[0] + b[1] * b[1] + b[2] * b[2], lc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
    if (lb > l2) l2 = lb;
    if (lc > l2) l2 = lc;
    if (!(l2 < 2.0 * SOL_NEEDLE_ASPECT * t->area)) return 1; /* (a degenerate or NaN triangle counts as a needle) */
  }
  return 0;
}

/* Counters of the last instrumented render (sol_render_counted); zero otherwise. Definitions are the
 * ones SURVEY.md 8d / DESIGN.md use for algorithmic bytes. */
typedef struct SolStats {
  uint64_t samples;       /* ray_color(primary,0,0) evaluations                                         */
  uint64_t rays;          /* world closest-hit queries (src/renderer/mod.rs:165), any depth             */
  uint64_t node_visits;   /* device BVH nodes fetched (sol_record_sizes: 64-B 7-wide nodes of the world)  */
  uint64_t sphere_tests, quad_tests, triangle_tests; /* primitive hit evaluations incl. light pdf tests */
  uint64_t shades;        /* material scatter evaluations                                               */
  uint64_t texel_fetches;
  uint64_t max_stack;     /* deepest traversal stack use                                                */
  /* SIMD lane utilisation of the kernel's phases: [0]/[1] traverse, [2]/[3] shade, [4]/[5] generate, each pair =
   * (active lanes summed over executions, 64 x executions). Instrumentation only. */
  uint64_t phase[6];
} SolStats;

typedef struct SolScene SolScene; /* opaque handle: owns device memory, stream; one host thread at a time */

/* Number of visible HIP devices (0 if none / no driver). */
int sol_device_count(void);

/* Validates and deep-copies `desc` onto HIP device `device` (caller may free its arrays on return).
 * Replaces the buffer/camera/pool set-up of Renderer::render (src/renderer/mod.rs:223-234) and carries
 * Renderer::new's "Scene should have at least one light" check (src/renderer/mod.rs:143-147, SOL_ENOLIGHT). */
int sol_scene_create(const SolSceneDesc* desc, int device, SolScene** out);
void sol_scene_destroy(SolScene* scene);

/* Creation options (no reference analogue: the reference has one BVH builder and no scheduler to tune). All-zero = the
 * defaults of sol_scene_create. The SOL_* environment variables of DESIGN.md 9 remain developer overrides, read once here. */
#define SOL_TREE_AUTO 0    /* the default: the GPU build (SOL_TREE_DEVICE); when that fails - a primitive with a non-finite box,
                              more than 2^23 primitives, no scratch memory - the host candidates + probe (SolSceneInfo says so) */
#define SOL_TREE_REF 1     /* the reference's topology (src/hittable/bvh.rs:84-162), collapsed 8-wide                 */
#define SOL_TREE_SAH8 2    /* host binned-SAH rebuild, 8 / 16 / 64 bins                                              */
#define SOL_TREE_SAH16 3
#define SOL_TREE_SAH64 4
#define SOL_TREE_DEVICE 5  /* built on the GPU (Morton sort, PLOC clustering, 7-wide collapse: sol_build.hip; 8f rank 3) */
#define SOL_TREE_HOST_PROBE 6 /* the four host candidates (1..4) + counted probe renders on the device pick one          */
typedef struct SolCreateOptions {
  uint32_t size;            /* sizeof(SolCreateOptions): lets the struct grow                                         */
  int32_t world_tree;       /* SOL_TREE_*                                                                              */
  int32_t no_work_order_probe; /* 1: skip the 4-spp cost probe of the frame (heavy-first work order); for previews     */
  int32_t split_percent;    /* device build: triangle pre-splitting may add this many references, in percent of the primitive
                               count (a split triangle gets one record per part of it). 0: the default - a budget of 30, used
                               only when it shrinks the summed box area of the primitives below 85 % (meshes of uniform small
                               triangles stay unsplit); > 0: that budget (at most 1000), always used; < 0: no pre-splitting   */
  int32_t reinsertion_rounds; /* device build: rounds of parallel reinsertion after the clustering (every node looks for the place
                               where its sub-tree adds the least surface area; results do not change). 0: the default (8), < 0: none,
                               at most 1024 (the rounds end when nothing moves)                                                  */
  int32_t no_background_blocks; /* 1: do not look for background blocks (below, SolSceneInfo::background_blocks)            */
  int32_t reserved[2];
  int32_t dynamic_triangles; /* 1: the handle keeps what sol_scene_set_triangles needs (per triangle: texture coordinates, material, dfs_index;
                                the primitives' unpadded fp32 boxes; the tree's levels; staging copies of the tree and the triangle records).
                                0: nothing of it is allocated and sol_scene_set_triangles is refused                                         */
  int32_t dynamic_primitives; /* 1 (with dynamic_triangles = 1, which it extends): the handle also keeps what sol_scene_set_primitives needs to move
                                spheres and quads (per sphere and quad: material, dfs_index; a second copy of every box array and of the sphere and
                                quad records). 0: nothing of it is allocated. This word was `reserved2` (0) in earlier headers: same size, same offset */
} SolCreateOptions;
int sol_scene_create_ex(const SolSceneDesc* desc, int device, const SolCreateOptions* options, SolScene** out);
/* Seconds sol_scene_create spent in: [0] host tree candidates, [1] uploads, [2] device tree build, [3] probe renders. */
int sol_scene_build_times(const SolScene* scene, double out[4]);

/* What sol_scene_create decided (diagnostic; no reference analogue). stack_bound: the host's bound on the traversal stack use of
 * any search of this scene, in dwords (2 per level of the 7-wide tree + the deepest medium boundary + 2): SolStats.max_stack of
 * a counted render never exceeds it, and the kernel built without a spill path is launched only when it is <= lds_stack. */
typedef struct SolSceneInfo {
  uint32_t size;            /* in: sizeof(SolSceneInfo)                                                               */
  uint32_t stack_bound, lds_stack, spill_stack;
  uint32_t tree_fallback;   /* 1: SOL_TREE_AUTO's device build failed and the host candidates were used (tree_note)    */
  char tree_name[32];       /* "device", "ref", "sah8", "sah16", "sah64"                                               */
  char tree_note[192];
  uint32_t split_references; /* device build: references that triangle pre-splitting added (0: none, or not kept)            */
  uint32_t split_triangles;  /* triangles with more than one reference                                                    */
  float split_area_ratio;    /* summed box area of the primitives' references after / before pre-splitting (the splits are kept
                                by default when this is below 0.85)                                                         */
  uint32_t reinsertion_moves; /* device build: sub-trees the reinsertion rounds moved                                       */
  float reinsertion_area_ratio; /* summed surface area of the binary tree's inner nodes after / before those rounds          */
  uint32_t partition_table;  /* 1: the balanced partition table is in force (SOL_OPT_BALANCED_PARTITION was set AND the creation
                                probe's block costs exist AND world > 1); 0: block b belongs to rank b % world                  */
  uint32_t partition_crc;    /* checksum of the block -> (rank, local block) mapping in force: equal on every rank of a job, or the
                                ranks render different partitions (each derives the table from its own probe)                     */
  uint32_t strict_triangles; /* 1: the scene has needle triangles (sol_scene_has_needles): fatter box pad, triangle consistency rule  */
  uint32_t background_blocks; /* 8x8 pixel blocks of which sol_scene_create PROVED that no camera ray of any of their pixels, whatever the
                                jitter, comes near a primitive's box (pinhole camera, constant background, the world a tree: the pyramid of
                                the block's rays against the world tree's boxes, conservatively). Every sample of such a pixel is the
                                background colour; sol_render adds those sums up in the reference's order without generating the
                                samples (SOL_OPT_BACKGROUND_BLOCKS). Images never depend on it. 0: none found, or not looked for     */
  uint32_t background_pixels; /* pixels of the image inside those blocks                                                        */
} SolSceneInfo;
int sol_scene_info(const SolScene* scene, SolSceneInfo* out);

/* Scheduler options of a live handle (take effect at the next sol_render; results never depend on them). */
#define SOL_OPT_SWITCH_BELOW 1        /* 0..64: a wave leaves the search loop when fewer 64ths of its lanes search      */
#define SOL_OPT_MAX_BLOCKS_PER_CU 2   /* 0 = as many as fit; n >= 1 caps resident workgroups per CU (occupancy studies)  */
#define SOL_OPT_KERNEL 3              /* 0 auto, 1 one-path-per-lane (product), 2 / 3 wavefront variants (A/B only)      */
#define SOL_OPT_WORK_ORDER 4          /* 0: plain chunk-major order, 1: heavy-first order from the creation probe        */
#define SOL_OPT_FINE_TAIL 5           /* quarters of a 16-sample item per resident lane that the END of a launch hands out one
                                         sample at a time (shorter tail; images unchanged); 0 off, -1 (default) decided by the
                                         creation probe                                                                      */
#define SOL_OPT_BALANCED_PARTITION 6  /* 1: sol_scene_set_partition / sol_comm_init deal the blocks out by their cost in the creation probe
                                         (a table behind the partition, the same on every rank) instead of b % world; for runs that use
                                         sol_gather / sol_read / sol_unpermute of THIS library - a caller with its own collective and
                                         un-permute keeps the default 0, whose layout it can compute. Set it on every rank, before
                                         sol_comm_init. Images never depend on it.                                              */
#define SOL_OPT_BACKGROUND_BLOCKS 7   /* 1 (default): the samples of background blocks (SolSceneInfo::background_blocks) are summed without
                                         being traced; 0: every sample of every pixel is generated and traced. Images never depend on it;
                                         counted renders (sol_render_counted) trace everything - their counters describe the whole
                                         algorithm - unless the value is 2: then they count exactly what a plain render does.      */
int sol_scene_set_option(SolScene* scene, int option, int64_t value);

/* Image-tile sharding for one-process-per-GPU runs (no reference analogue). The image is cut
 * into 8x8-pixel blocks, block b (row-major) belongs to rank b % world (or, with SOL_OPT_BALANCED_PARTITION, to the rank a
 * cost-sorted deal gives it). Each rank accumulates only its own blocks in a compact buffer of sol_accum_floats() floats:
 * [local_block][py][px][rgb]. Default rank 0/1. */
int sol_scene_set_partition(SolScene* scene, int rank, int world);
/* A caller-bound accumulator (sol_scene_bind_accum) whose size would change makes this fail with SOL_EINVAL: unbind
 * (sol_scene_bind_accum(scene, NULL, 0)) first, re-bind a buffer of the new sol_accum_floats() afterwards. */

/* Multi-GPU behind the ABI ("the handle owns the communicators, the read gathers across GPUs"). One
 * process per GPU, each with its own SolScene of the same description:
 *   rank 0:  sol_comm_unique_id(id)  -> ship the 128 bytes to the other ranks by any means (file, socket, MPI, ..)
 *   all:     sol_comm_init(scene, rank, world, id)   collective: ncclCommInitRank (RCCL); also sets the tile partition
 *   all:     sol_render(...)         every rank renders the 8x8 tiles it owns
 *   all:     sol_gather(scene, image_dev)            collective, asynchronous on the scene's stream: the compact fp32
 *            accumulators travel to rank 0 (grouped ncclSend / ncclRecv: every shard rides its own xGMI link into the
 *            root, no ring) and are un-permuted there into `image_dev` (device, W*H*3 floats, row 0 = top; NULL = the
 *            scene's own image buffer, see sol_resolve_image); ranks != 0 ignore image_dev.
 *   rank 0:  sol_read_image(scene, host_rgb_sum)     blocks; copies the gathered image out (or use the device pointer)
 *   all:     sol_comm_destroy(scene)  (also done by sol_scene_destroy)
 * RCCL (librccl.so) is loaded on the first sol_comm_* call; a single-GPU process never needs it. */
#define SOL_UNIQUE_ID_BYTES 128
int sol_comm_unique_id(uint8_t id[SOL_UNIQUE_ID_BYTES]);
int sol_comm_init(SolScene* scene, int rank, int world, const uint8_t id[SOL_UNIQUE_ID_BYTES]);
int sol_comm_destroy(SolScene* scene);
int sol_gather(SolScene* scene, void* image_dev);
/* Diagnostic for single-GPU boxes: sends the accumulator to this very rank through the communicator (the grouped
 * ncclSend / ncclRecv pair sol_gather uses) and compares the bytes. */
int sol_comm_self_check(SolScene* scene);
/* The same gather for ONE process that drives n GPUs (the way a caller of the reference's ray_trace(), src/lib.rs:93-99, is written): scenes[i] is
 * rank i of n (sol_scene_set_partition(scenes[i], i, n)), each created on its own device. Waits for every rank's renders, copies the compact
 * accumulators device to device into rank 0's gather buffer (peer copies; no communicator, RCCL is not loaded) and un-permutes them into rank 0's
 * image buffer; *image_dev = that buffer (W*H*3 floats, row 0 = top, on scenes[0]'s device, valid until the next gather / read / resolve on
 * scenes[0]); asynchronous on scenes[0]'s stream - the post-processors (sol_tonemap_rgb8, sol_bloom*) of scenes[0] take it as they take
 * sol_resolve_image's, sol_read_image copies it to the host. */
int sol_gather_local(SolScene* const* scenes, int n, void** image_dev);
int sol_read_image(SolScene* scene, float* rgb_sum);
/* Largest n_samples one sol_render call accepts for the current partition (the work counter is 32 bits). */
uint32_t sol_max_samples_per_call(const SolScene* scene);

/* Compact accumulator (device memory, fp32 sums over samples). By default the handle owns it; a caller that
 * wants to hand it to a collective (torch.distributed / RCCL) may bind its own device buffer instead. */
size_t sol_accum_floats(const SolScene* scene);
void* sol_accum_ptr(SolScene* scene);
int sol_scene_bind_accum(SolScene* scene, void* device_ptr, size_t n_floats);
/* Use the caller's hipStream_t for all work of this handle (NULL = the handle's own stream). */
int sol_scene_set_stream(SolScene* scene, void* hip_stream);

/* Zero the accumulator. */
int sol_clear(SolScene* scene);

/* Enqueue samples [first_sample, first_sample + n_samples) of every pixel this rank owns; their colours are
 * ADDED to the accumulator (sums, not means: src/renderer/mod.rs:361-365, src/util/rgb_color.rs:21-35).
 * Asynchronous. Replaces the row tasks of one or more passes (src/renderer/mod.rs:241-291). `seed` keys the
 * counter-based RNG that replaces src/random.rs; the result is a pure function of (scene, seed, pixel,
 * sample index) and independent of the partition. */
int sol_render(SolScene* scene, uint32_t first_sample, uint32_t n_samples, uint64_t seed);
/* Same, with instrumentation counters enabled (slower; fills sol_stats). */
int sol_render_counted(SolScene* scene, uint32_t first_sample, uint32_t n_samples, uint64_t seed);
int sol_sync(SolScene* scene);

/* Blocks; writes the full-image fp32 sums, W*H*3 floats, row 0 = image TOP (row index (H-1-y),
 * src/renderer/mod.rs:261). Pixels owned by other ranks are written as 0 when world > 1. */
int sol_read(SolScene* scene, float* rgb_sum);

/* Auxiliary buffers of the first hit (src/renderer/mod.rs:175-204; consumed by denoising post-processors): samples
 * [first, first + n) of the albedo colour (AlbedoShader on the primary hit, background colour on a miss) and of the shading
 * normal (NormalShader, zero on a miss) are ADDED to two accumulators laid out like the colour accumulator (same partition).
 * Independent of sol_render; sol_clear_aux zeroes them, sol_read_aux blocks and writes W*H*3 floats each, row 0 = top
 * (either pointer may be NULL). */
int sol_render_aux(SolScene* scene, uint32_t first_sample, uint32_t n_samples, uint64_t seed);
int sol_clear_aux(SolScene* scene);
int sol_read_aux(SolScene* scene, float* albedo_sum, float* normal_sum);

/* Rank-0 side of the multi-GPU gather: `gathered` is device memory holding world compact buffers back to
 * back (rank r at offset r * sol_accum_floats()), as produced by an RCCL gather; writes the row-major image
 * (W*H*3 floats, row 0 = top) to device memory `image`. */
int sol_unpermute(SolScene* scene, const void* gathered_dev, int world, void* image_dev);

/* Device-side Nop post-processor: sums -> (/spp, sqrt, clamp, *256) -> RGB8, the arithmetic of
 * src/util/rgb_color.rs:14-35 via src/post/nop.rs:19-34. `image_dev` is W*H*3 floats row-major (device),
 * `rgb8_host` receives W*H*3 bytes. */
int sol_tonemap_rgb8(SolScene* scene, const void* image_dev, uint32_t num_samples, uint8_t* rgb8_host);

/* Un-permutes this scene's own accumulators into its internal row-major image buffer (W*H*3 floats, row 0 = top, device
 * memory owned by the scene, valid until the next sol_read / sol_resolve_image) and returns its device pointer: the input
 * of the device-side post-processors when no gather is involved (single GPU). Asynchronous on the scene's stream. */
int sol_resolve_image(SolScene* scene, void** image_dev);

/* Device-side BloomPostProcessor (src/post/bloom.rs:76-150), f64 arithmetic in the reference's summation order on the
 * fp32 sums of `image_dev` (W*H*3 floats, row-major, device). `threshold` and `max_intensity` are per-sample values
 * (BloomPostProcessor::new's defaults: |(1,1,1)| and f64::MAX); kernel_size_fraction outside [0, 0.5] is SOL_EINVAL with
 * the reference's message.
 *   sol_bloom       = intermediate_post_process: image_dev <- pixel + blurred bright pixels, rounded to fp32, in place;
 *   sol_bloom_rgb8  = post_process: the same sums carried in f64 through to_rgb_color into rgb8_host (W*H*3 bytes).
 *  */
int sol_bloom(SolScene* scene, void* image_dev, uint32_t num_samples, double kernel_size_fraction, double threshold,
              double max_intensity);
int sol_bloom_rgb8(SolScene* scene, const void* image_dev, uint32_t num_samples, double kernel_size_fraction, double threshold,
                   double max_intensity, uint8_t* rgb8_host);
/* create_gaussian_blur_weights (src/util/gaussian.rs:11-25), the weights sol_bloom uses; host-only, for known-answer tests. */
int sol_gaussian_blur_weights(uint32_t kernel_size, double std_dev, double* out);

/* ---- adaptive sampling (EXTENSION, not in the reference; opt-in) ------------------------------------------------
 * Rounds of `round_samples` samples over the 8x8 blocks still active; a block stops once every real pixel in it has converged by
 * the batch-means rule of DESIGN.md 11, or when it holds max_samples. Every pixel of a block holds the same count n_b, and its
 * sums are bit-identical to sol_clear + sol_render(scene, 0, n_b, seed). One rank, one device: world > 1 is SOL_EINVAL.
 * sol_clear, sol_render, sol_render_counted and sol_scene_set_partition end the session. */
typedef struct SolAdaptive {
  uint32_t size;           /* in: sizeof(SolAdaptive): lets the struct grow                                              */
  uint32_t round;          /* samples per round, a positive multiple of 16                                              */
  uint32_t min_samples;    /* no block stops before it holds this many (nor before its second round): a multiple of 16  */
  uint32_t max_samples;    /* samples_per_pixel: >= min_samples, >= 1                                                  */
  float threshold;         /* relative standard error of the mean luminance that counts as converged; 0 = never          */
} SolAdaptive;
/* Checks the configuration (before the device is touched), clears the accumulator and the per-pixel state, activates every block. */
int sol_adaptive_begin(SolScene* scene, const SolAdaptive* config);
/* Renders and evaluates one round; *active_blocks = the blocks the next round samples (0: the session is done). Blocks. */
int sol_adaptive_round(SolScene* scene, uint64_t seed, uint32_t* active_blocks);
/* Samples per pixel of every image block, row-major over blocks of 8x8 ((width + 7) / 8 per row); n = the entries of per_block. */
int sol_adaptive_counts(SolScene* scene, uint32_t* per_block, size_t n);
/* The Nop post-processor (sol_tonemap_rgb8) with every pixel scaled by its own block's sample count. */
int sol_tonemap_rgb8_adaptive(SolScene* scene, const void* image_dev, uint8_t* rgb8_host);
/* Rescales image_dev (W*H*3 floats, device) in place to sum * max_samples / n_b, so that sol_bloom / sol_bloom_rgb8 with
 * max_samples see sums of a uniform count. */
int sol_adaptive_rescale(SolScene* scene, void* image_dev);

/* ---- environment importance sampling (EXTENSION, not in the reference; opt-in) -----------------------------------
 * Mode 1 makes the environment map entry L = n_lights of the light mixture: the light half of a Lambertian or Isotropic scatter picks
 * one of L + 1 entries, and its density is (sum of the lights' densities + the map's) / (L + 1). The map is drawn from per cell by
 * luminance times sin(theta) (cell (i, j) = texel (i, j), i < max(W - 1, 1), j < max(H - 1, 1): the texels a lookup reads); the tables
 * are built on the scene's stream on first use, in a fixed order, bit-identical on every device. Only renders of the path-tracing shader
 * change; mode 0 (the default) leaves every frame as it was. While it is on: path-tracing renders run the product kernel whatever
 * SOL_OPT_KERNEL says, adaptive rounds use it, sol_render_counted and sol_debug_path are SOL_EINVAL. Changing the mode ends an adaptive
 * session. SOL_EINVAL: a bad size, an unknown mode, non-zero reserved fields (all checked before the scene), no environment map,
 * env_scale <= 0, or a map whose cell weights sum to 0. */
#define SOL_ENV_SAMPLING_OFF 0u
#define SOL_ENV_SAMPLING_IMPORTANCE 1u
typedef struct SolEnvSampling {
  uint32_t size;           /* in: sizeof(SolEnvSampling): lets the struct grow                                           */
  uint32_t mode;           /* SOL_ENV_SAMPLING_OFF / SOL_ENV_SAMPLING_IMPORTANCE                                          */
  uint32_t reserved[2];    /* 0                                                                                          */
} SolEnvSampling;
/* config == NULL or mode 0: off. */
int sol_env_sampling(SolScene* scene, const SolEnvSampling* config);
/* Host only (no device needed): the checks sol_env_sampling makes, on a description. */
int sol_env_sampling_check(const SolSceneDesc* desc, const SolEnvSampling* config);
/* Diagnostic: the tables (built by sol_env_sampling mode 1): the marginal CDF over the H' cell rows, the conditional CDFs (H' rows of W',
 * row-major), both normalised, and the total cell weight. NULL pointers are skipped. */
int sol_env_tables(SolScene* scene, float* marginal, size_t n_marginal, float* conditional, size_t n_conditional, float* total);
/* Diagnostic: the device's own sampler and density on n host rows. fn 0: (r1, r2) in [0, 1) -> (direction xyz, pdf, cell i, cell j),
 * 2 floats in, 6 out per row; fn 1: direction xyz -> (pdf, cell i, cell j), 3 in, 3 out. Needs the tables. */
int sol_env_eval(SolScene* scene, uint32_t fn, const float* in, uint32_t n, float* out);

/* ---- light tree and power-weighted light sampling (EXTENSION, not in the reference; opt-in) -------------------------------
 * The light half of a Lambertian or Isotropic scatter evaluates the density of the light mixture, by default with one test per light.
 *   mode 0 UNIFORM (default): as the reference - a uniform choice of light, the density a loop over every light. Frames as they were.
 *   mode 1 TREE: the same choice and the same sum, found through a light tree: an implicit complete 4-ary tree over the light list in
 *          list order, built on the device on first use (one launch for the leaves, one per level; bit-identical on every device), about
 *          (4/3) 4^ceil(log4 L) x 24 bytes, freed by sol_scene_destroy. Every box is conservative for the record the light's test reads, so a
 *          light the walk skips would have added exactly +0.0f and the others are added in the loop's order: frames are BIT-IDENTICAL to mode 0.
 *          The tree is tight when the list is spatially coherent (the host library lists lights in the world tree's depth-first order); a
 *          list in arbitrary order renders the same frames, more slowly.
 *   mode 2 POWER: a light is chosen with probability q_i proportional to its power w_i = area_i x luminance of its DiffuseLight's emission
 *          (f64, from the description, at creation; attenuation ignored; other materials 0; sol_light_weights), C_i = (float)(prefix_i / W),
 *          C_{L-1} = 1, q_i = C_i - C_{i-1} in fp32 (sol_light_tables); one draw u, the first k with u < C_k. Density sum_{q_i > 0} q_i pdf_i
 *          through the tree. With the environment sampled as well (sol_env_sampling): the map is entry L of L + 1 as before, a light entry takes
 *          one more draw, and the density is (L * sum q_i pdf_i + p_env) / (L + 1). A new unbiased estimator; SOL_EINVAL if every w_i is 0.
 * With one light modes 1 and 2 are mode 0's estimator and render with its kernels. While the mode is not 0: path-tracing renders run the
 * product kernel whatever SOL_OPT_KERNEL says, adaptive rounds use it, sol_render_counted and sol_debug_path are SOL_EINVAL. Changing the
 * mode ends an adaptive session. SOL_EINVAL: a bad size, an unknown mode, non-zero reserved fields (checked before the scene), more than
 * 2^30 lights (modes 1, 2), mode 2 on a scene whose lights all have power 0. */
#define SOL_LIGHT_SAMPLING_UNIFORM 0u
#define SOL_LIGHT_SAMPLING_TREE 1u
#define SOL_LIGHT_SAMPLING_POWER 2u
typedef struct SolLightSampling {
  uint32_t size;           /* in: sizeof(SolLightSampling): lets the struct grow                                         */
  uint32_t mode;           /* SOL_LIGHT_SAMPLING_UNIFORM / _TREE / _POWER                                                  */
  uint32_t reserved[2];    /* 0                                                                                          */
} SolLightSampling;
/* config == NULL: mode 0. */
int sol_light_sampling(SolScene* scene, const SolLightSampling* config);
/* Host only (no device needed): the checks sol_light_sampling makes, on a description (the all-zero power refusal of mode 2 included). */
int sol_light_sampling_check(const SolSceneDesc* desc, const SolLightSampling* config);
/* Host only: the power w_i of each light of the description (mode 2's weights, f64, list order); n >= desc->n_lights. */
int sol_light_weights(const SolSceneDesc* desc, double* w, size_t n);
/* Diagnostic: mode 2's tables as the device holds them (q, C; n >= n_lights floats each) and W, the f64 sum of the weights. Built by
 * sol_light_sampling mode 2. NULL pointers are skipped. */
int sol_light_tables(SolScene* scene, float* q, float* cdf, size_t n, double* total);
/* Diagnostic: the light tree as the device holds it (6 floats per node: min xyz, max xyz; nodes may be NULL), its node count, the
 * index of leaf 0 and its size in bytes. Built by sol_light_sampling mode 1 or 2. */
int sol_light_tree(SolScene* scene, float* nodes, size_t n_floats, uint32_t* n_nodes, uint32_t* first_leaf, size_t* bytes);
/* Diagnostic: the device's own functions on n host rows. fn 0: (origin xyz, direction xyz) -> (the loop's density, the tree's density,
 * tree nodes visited, light tests), 6 floats in, 4 out, under the current mode's weighting (modes 0 and 1 uniform: the loop is the
 * default kernels' function; mode 2 power) and with the environment's entry while sol_env_sampling is on; needs the tree. fn 1: u in
 * [0, 1) -> the light index mode 2 selects, 1 in, 1 out; needs the tables. */
int sol_light_eval(SolScene* scene, uint32_t fn, const float* in, uint32_t n, float* out);

/* ---- denoiser (EXTENSION, opt-in) --------------------------------------------------------------------------------------
 * An edge-aware a-trous filter of a colour image guided by the first-hit albedo and normal planes (sol_render_aux): the stand-in for the
 * reference's OidnPostProcessor (src/post/oidn.rs), which stays the Nop post-processor. Colour sums S over n samples, albedo and normal sums
 * A, N over m samples, all W*H*3 floats, row-major, row 0 = top, on the scene's device:
 *   c = S / n (a value that is not finite counts as 0), a = A / m, v = N / m; per channel f = a > 0.01 ? a : 1 and e = c / f;
 *   guide normal g = v / |v| when |v| > 1e-3, else the pixel is a miss;
 *   pass i = 0 .. iterations-1: taps q = p + 2^i (dx, dy), dx, dy in -2..2, B3 weights h = (1/16, 1/4, 3/8, 1/4, 1/16), taps outside the
 *   image skipped; e'_p = sum h[dx] h[dy] w_pq e_q / sum h[dx] h[dy] w_pq (dy inner, dx outer), w_pq = w_c w_n with
 *   w_c = exp(-sum_ch (t(e_p) - t(e_q))^2 / (sigma_color^2 4^-i)), t(x) = max(x, 0) / (1 + max(x, 0)), and w_n = 1 if both are misses,
 *   0 if one is, max(0, g_p . g_q)^normal_power otherwise; the centre tap counts with w = 1;
 *   out = e_K * f, written as sums (out * n): sol_tonemap_rgb8 with n tones it as it tones a raw frame.
 * Deterministic (no atomics, fixed tap order). SOL_EINVAL: see sol_denoise_check. */
#define SOL_DENOISE_DEFAULT_ITERATIONS 5u
#define SOL_DENOISE_DEFAULT_SIGMA_COLOR 0.25f
#define SOL_DENOISE_DEFAULT_NORMAL_POWER 64.0f
typedef struct SolDenoise {
  uint32_t size;           /* in: sizeof(SolDenoise): lets the struct grow                                                  */
  uint32_t iterations;     /* passes, 1..8                                                                                  */
  float sigma_color;       /* finite, > 0                                                                                   */
  float normal_power;      /* finite, >= 0                                                                                  */
  uint32_t reserved[2];    /* 0                                                                                             */
} SolDenoise;
/* Host only (no device needed): SOL_EINVAL with a message for a wrong size, iterations outside 1..8, a sigma_color that is not finite or
 * not above 0, a normal_power that is not finite or below 0, a non-zero reserved field. NULL = the defaults above. */
int sol_denoise_check(const SolDenoise* config);
/* Un-permutes the scene's auxiliary planes into two row-major buffers the scene owns (W*H*3 floats each, valid until the next call;
 * not the sol_resolve_image buffer) and returns their device pointers (either may be NULL) and the aux samples added since the last
 * clear (sol_render_aux adds, sol_clear_aux and a partition change that clears the planes reset it). SOL_EINVAL before any
 * sol_render_aux and when world > 1 (the planes are rank-local). Asynchronous on the scene's stream. */
int sol_resolve_aux(SolScene* scene, void** albedo_dev, void** normal_dev, uint32_t* aux_samples);
/* The filter, in place on image_dev, asynchronous on the scene's stream. Scratch is allocated on the scene on first use and kept. */
int sol_denoise(SolScene* scene, void* image_dev, uint32_t num_samples, const void* albedo_dev, const void* normal_dev, uint32_t aux_samples,
                const SolDenoise* config);
/* The same into a scratch image (image_dev is left alone), then the Nop tone map with num_samples into rgb8_host (W*H*3 bytes): the bytes
 * of sol_denoise followed by sol_tonemap_rgb8. Blocks. */
int sol_denoise_rgb8(SolScene* scene, const void* image_dev, uint32_t num_samples, const void* albedo_dev, const void* normal_dev,
                     uint32_t aux_samples, const SolDenoise* config, uint8_t* rgb8_host);

int sol_stats(const SolScene* scene, SolStats* out);
/* What the paths of the last instrumented render (sol_render_counted, one-path-per-lane kernel) looked like - how hard a workload
 * is: the share of camera rays that hit something and the samples by the number of rays of their path (a path of n rays was
 * scattered n - 1 times: src/renderer/shader.rs:62-125). No reference analogue. */
typedef struct SolPathStats {
  uint32_t size, pad;      /* in: sizeof(SolPathStats)                                                              */
  uint64_t samples;
  uint64_t primary_hits;   /* samples whose camera ray hit a primitive                                              */
  uint64_t path_len[6];    /* samples with 1, 2, 3-4, 5-8, 9-16, 17 or more rays                                    */
} SolPathStats;
int sol_path_stats(const SolScene* scene, SolPathStats* out);

/* Diagnostic, host only (no device needed): builds the 7-wide quantised tree of the world exactly as sol_scene_create does
 * (use_sah = 0: collapsed from the reference's topology, 1: from the 16-bin SAH rebuild, n > 1: from the n-bin rebuild; -1: the tree
 * the GPU builder of SOL_TREE_DEVICE makes - this one needs a device) and verifies its structure with the
 * device's decode arithmetic. Returns SOL_OK with the findings in `out`; the tree is sound iff box_violations ==
 * leaf_mismatches == bad_empty_slots == 0. */
typedef struct SolTreeCheck {
  uint32_t n_wide;           /* wide nodes                                                                       */
  uint32_t n_leaf_refs;      /* primitive references reachable from the root                                      */
  uint32_t n_primitives;     /* primitive references of the reference-shaped tree (the multiset the tree must hold)*/
  uint32_t depth;            /* levels of wide nodes                                                              */
  uint32_t max_children;     /* most children in one node (<= 7)                                                  */
  uint32_t box_violations;   /* children whose decoded box does not contain every padded primitive box below it   */
  uint32_t leaf_mismatches;  /* primitive references missing from / surplus in the tree                           */
  uint32_t bad_empty_slots;  /* empty slots that are not (NONE reference, inverted box)                           */
  double inner_area, leaf_area; /* summed box areas of inner / primitive children (the surface-area cost estimate)  */
  uint32_t n_extra_references; /* device build: references that pre-splitting added (a split triangle has several)     */
  uint32_t n_split_triangles;  /* triangles with more than one reference                                              */
  uint32_t split_uncovered;    /* sample points of split triangles that no reference box of their triangle holds (must be 0) */
  uint32_t reserved;
} SolTreeCheck;
/* SolTreeCheck carries no size field and grew after its first release (the three split counters and `reserved`): sol_world_tree_check
 * writes the FIRST layout only - the fields through leaf_area, SOL_TREE_CHECK_V1_BYTES - so a binding compiled against that header is never
 * overrun; sol_world_tree_check_ex takes the caller's sizeof(SolTreeCheck) and fills every field that fits (the rest of `out` is zeroed). */
#define SOL_TREE_CHECK_V1_BYTES 48
int sol_world_tree_check(const SolSceneDesc* desc, int use_sah, SolTreeCheck* out);
int sol_world_tree_check_ex(const SolSceneDesc* desc, int use_sah, void* out, size_t out_size);
/* Diagnostic, host only: the background blocks (SolSceneInfo::background_blocks) found with the host-built tree `use_sah` (>= 0) names:
 * flags[b] = 1 for block b (row-major, (width + 7) / 8 blocks per row), *n_found their number. flags may be NULL. */
int sol_background_blocks(const SolSceneDesc* desc, int use_sah, uint8_t* flags, size_t n_flags, uint32_t* n_found);

/* Diagnostic: traces the single path (pixel x, y counted from the image top; sample index) and writes 12 floats per ray
 * (origin xyz, direction xyz, hit t, hit reference bits, dfs index bits, depth, 0, 0), closed by a row holding the sample's
 * colour in its first three floats and -1 in the fourth. For comparing a path bounce by bounce with the oracle. */
int sol_debug_path(SolScene* scene, uint32_t x, uint32_t y, uint32_t sample, uint64_t seed, float* rows, uint32_t max_rows);

/* Measurement: with timing enabled every sol_render brackets its render kernel with HIP events on the stream it is
 * launched on; sol_last_kernel_ms blocks on the last one and returns its duration (and the grid it was launched with).
 * No reference analogue (the reference reports only passes/s, src/renderer/mod.rs:367-373). */
int sol_kernel_timing(SolScene* scene, int enable);
int sol_last_kernel_ms(SolScene* scene, float* ms, uint32_t* grid_blocks);

/* Function-level evaluation of the device code on n rows of host floats (in_stride / out_stride floats per row), for
 * pinning the fp32 arithmetic contract bit for bit (tests/test_gpu_functions.py). fn: 0 arithmetic, 1 elementary
 * functions, 2 RNG, 3 vector ops + Onb::new, 4 Sphere::hit, 5 Quad::hit, 6 Triangle::hit, 7 Aabb::hit, 8 sampling
 * (row layouts: solstrale-rust_amd/csrc/sol_aux.hip, sol_eval_kernel; floats read / written per row, fn 0..8: 3/7, 3/5, 5/2, 7/18, 13/2,
 * 24/4, 17/4, 12/2, 4/7 - narrower strides and unknown functions are SOL_EINVAL). No reference analogue. */
int sol_eval(int device, uint32_t fn, const float* in, uint32_t n, uint32_t in_stride, float* out, uint32_t out_stride);

/* Sizes of the device records, for the algorithmic-bytes formula: node, sphere, quad, triangle
 * intersect records, shading record, material record (bytes). */
int sol_record_sizes(uint32_t out[6]);

const char* sol_last_error(void);

/* ---- ray queries (EXTENSION, not in the reference) ------------------------------------------------------------------------
 * Batches of the caller's own rays against the world tree the handle owns: the object under a cursor, a depth map, a visibility or
 * ambient-occlusion bake, a line-of-sight test - without rendering a frame. A ray is origin + t * direction, t in units of |direction|
 * (directions are not normalised, as in the reference). It is VALID when every component is finite (tmax may be +inf), the direction is
 * not zero and 0 <= tmin <= tmax; any other ray is answered SOL_RAY_INVALID by the kernel itself, without a search - no bit pattern faults,
 * hangs or runs unbounded.
 *   SOL_QUERY_CLOSEST   one SolRayHit per ray: the primitive with the smallest t in [tmin, tmax] under the world search's own interval test,
 *                       among equal t the last in depth-first order (the (t, dfs) rule); fp32 rules 1-7 as they are, rule 8
 *                       not (a query ray leaves no primitive). u, v: barycentrics of a triangle, planar coordinates of a quad, 0 of a
 *                       sphere; kind: SOL_REF_SPHERE / _QUAD / _TRIANGLE; dfs_index: the primitive's own number in the description (a
 *                       pre-split triangle's parts carry their original's); material: its record's. A miss: status SOL_RAY_MISS, t = +inf,
 *                       the other words 0. An invalid ray: status SOL_RAY_INVALID, the other words 0.
 *   SOL_QUERY_OCCLUDED  one uint32_t status per ray: SOL_RAY_HIT exactly when SOL_QUERY_CLOSEST reports a hit for the same ray (the search
 *                       stops early where it may).
 * n == 0 succeeds and does nothing. SOL_EINVAL: n above 2^31, an unknown mode, a null pointer, a scene with a constant medium (its hits are
 * random draws keyed by a path; a query has none). SOL_EDEVICE without a GPU. A query touches neither the accumulator, the auxiliary planes,
 * the partition nor an adaptive session, and works for any rank / world (the scene is replicated).
 *   Origins.  The fp32 contract's margins are sized by the scene, not by the ray: boxes are padded by S * 2^-20 and a sphere's hit point may
 *             lie S * 2^-21 outside the sphere's own box (rules 1 and 2), where S is the largest |coordinate|, cast to float, of
 *             the world's bounding box (the bbox of the description's root) and of the camera origin of the description the handle was
 *             CREATED from (sol_scene_set_camera does not change S; sol_scene_set_triangles / _set_primitives take the moved boxes). A ray
 *             from origin o carries a rounding error of about |o| * 2^-23 in its hit points and slab parameters. While every coordinate of
 *             the origin stays within 4 * S, the answers are the contract's: the same for every world tree, equal to the float oracle's,
 *             and every hit that the reference's f64 arithmetic finds clear of a primitive's edge is found (measured clean up to 16 * S,
 *             one rung of 4 kept as margin: profiles/far_origins.txt, tests/test_far_origins.py, tests/test_gpu_far_origins.py). Beyond
 *             that every origin that is finite stays VALID, the calls return and each ray is answered SOL_RAY_HIT with a finite t in
 *             [tmin, tmax] and an existing primitive, or SOL_RAY_MISS; but hits may be lost - first at the poles of spheres seen along an
 *             axis (64 * S), then on flat primitives (quads, axis-aligned triangles) whose boxes are flat (256 * S in the float oracle,
 *             4096 * S on the device, whose quantised boxes are fatter) -, and from 4096 * S on the answer may depend on the world tree.
 *             A caller with such rays moves the origin along the ray to within 4 * S and shifts tmin, tmax and the returned t by that step. */
typedef struct SolRay { float ox, oy, oz, tmin, dx, dy, dz, tmax; } SolRay;        /* 32 bytes; 16-byte aligned in device memory */
typedef struct SolRayHit { float t, u, v; uint32_t status, kind, dfs_index, material, reserved; } SolRayHit; /* 32 bytes */
enum { SOL_QUERY_CLOSEST = 0, SOL_QUERY_OCCLUDED = 1 };
enum { SOL_RAY_MISS = 0, SOL_RAY_HIT = 1, SOL_RAY_INVALID = 2 };
/* Device pointers (n SolRay in, n SolRayHit or n uint32_t out, on the scene's device), on the scene's stream, asynchronous. */
int sol_query_dev(SolScene* scene, int mode, const void* rays_dev, size_t n, void* out_dev);
/* Host arrays, staged through buffers the handle owns; blocks. */
int sol_query(SolScene* scene, int mode, const SolRay* rays, size_t n, void* out);
/* Writes the camera rays of the pixels [x0, x1) x [y0, y1) (y counted from the image top), row-major, for (sample, seed) to device memory:
 * exactly the rays a render's samples start with (the same RNG key and draws), tmin = 0.001, tmax = +inf. Asynchronous on the scene's
 * stream. SOL_EINVAL: an empty rectangle or one that leaves the frame. */
int sol_camera_rays(SolScene* scene, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint32_t sample, uint64_t seed, void* rays_dev);

/* ---- radiance queries (EXTENSION, not in the reference) -------------------------------------------------------------------
 * "How much light arrives along this ray?" - the path-traced colour along the caller's own rays: reflection captures, a second viewpoint
 * without a second handle; for light probes, irradiance volumes and lightmap texels see the irradiance queries below. Rays are SolRay rows, valid by the rule of the ray
 * queries above and decided by the kernel itself before any search; an invalid ray answers (0, 0, 0, samples = 0).
 *   Paths.    For a valid ray i, each sample s in [first_sample, first_sample + samples) is one path: the render's RNG stream of
 *             (seed, key, s) with its counter set to first_draw, where (key, first_draw) is the ray's SolRayKey (pixel, first_draw) or, with
 *             keys == NULL, (key_base + i wrapping, the configuration's first_draw). The path starts as a camera path does, with the caller's
 *             origin and direction. Its first search runs over the ray's own [tmin, tmax] - a miss there is the background, or the
 *             environment map along the direction -, every later segment over [0.001, +inf) as in a render.
 *   Shading.  The handle's current shader, max_depth, sol_env_sampling and sol_light_sampling modes: the answer a render would give in
 *             that state (an Albedo or Normal shader gives those quantities along the rays).
 *   Sums.     SolRadiance holds SUMS over the samples, not means, added in the render's order: samples in chunks of 16 counted from
 *             first_sample, a chunk sum 0 + c0 + c1 + .. in sample order, the result ((0 + chunk0) + chunk1) + ..
 *   Identity. Over the rays sol_camera_rays writes for (rectangle, sample s, seed), keyed by what sol_camera_ray_keys writes for the same
 *             arguments, with samples = 1 and first_sample = s, the answers equal bit for bit what sol_clear; sol_render(s, 1, seed);
 *             sol_read leaves in those pixels.
 *   Neutral.  A radiance query writes the caller's output and scratch of its own; it touches neither the accumulator, the auxiliary planes,
 *             the render's work counter, the partition, an adaptive session nor SolStats. Frames rendered around it do not change.
 * SOL_EINVAL (sol_last_error names the reason): a null scene or configuration; a wrong size; reserved != 0; samples == 0, or
 * first_sample + samples beyond 2^32 - 16; n above 2^31; a scene with a constant medium (not supported yet); with n > 0 a null ray or output
 * pointer. n == 0 succeeds and touches nothing. These are checked before the device is: SOL_EDEVICE without a GPU comes after them. */
typedef struct SolRayKey { uint32_t pixel, first_draw; } SolRayKey;            /* 8 bytes; 8-byte aligned in device memory */
typedef struct SolRadiance { float r, g, b; uint32_t samples; } SolRadiance;   /* 16 bytes; sums, not means; 16-byte aligned in device memory */
/* size = sizeof(SolRadianceConfig) = 32: size 0, samples 4, first_sample 8, first_draw 12, seed 16, key_base 24, reserved 28 */
typedef struct SolRadianceConfig { uint32_t size, samples, first_sample, first_draw; uint64_t seed; uint32_t key_base, reserved; } SolRadianceConfig;
/* Device pointers (n SolRay, n SolRayKey or NULL, n SolRadiance out, on the scene's device), on the scene's stream, asynchronous. */
int sol_radiance_dev(SolScene* scene, const void* rays_dev, const void* keys_dev, size_t n, const SolRadianceConfig* config, void* out_dev);
/* Host arrays, staged through buffers the handle owns; blocks. */
int sol_radiance(SolScene* scene, const SolRay* rays, const SolRayKey* keys, size_t n, const SolRadianceConfig* config, SolRadiance* out);
/* Writes one SolRayKey per pixel of [x0, x1) x [y0, y1), row-major like sol_camera_rays, for (sample, seed) to device memory:
 * pixel = row * width + x, first_draw = the RNG counter after the camera ray was made (2 for a pinhole; with a thin lens 2 plus twice the
 * rejection rounds of the lens disc). Asynchronous on the scene's stream. SOL_EINVAL: a null pointer, an empty rectangle or one that
 * leaves the frame. */
int sol_camera_ray_keys(SolScene* scene, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint32_t sample, uint64_t seed, void* keys_dev);

/* ---- irradiance queries (EXTENSION, not in the reference) -----------------------------------------------------------------
 * "How much light arrives at this point?" - the hemisphere (or sphere) gather a lightmap texel, a light probe or an irradiance volume needs:
 * a radiance query whose every sample draws a fresh direction on the device, so the caller uploads n points, not n x samples rays. (sol_gather
 * is the multi-rank image gather; hence the name.)
 *   Points.   A point is a SolRay row read as (position xyz, tmin, normal xyz, tmax), valid by the ray queries' rule exactly as it stands: every
 *             word finite (tmax may be +inf), the normal not zero, 0 <= tmin <= tmax. The normal need not be unit length (its squared length
 *             must be a finite, normal fp32 number). An invalid point answers (0, 0, 0, samples = 0), decided before any search. A position is
 *             the origin of the rays gathered from it: the origin envelope of the ray queries (SolRay, "Origins": every coordinate within
 *             4 * S for the contract's answers; beyond it proper answers, with hits that may be lost) holds for positions as it stands, in
 *             every gather that takes such rows (sol_irradiance*, sol_visibility*, sol_volume_points' probes).
 *   Paths.    For a valid point i, each sample s in [first_sample, first_sample + samples) is one path: the RNG stream of (seed, key, s) with
 *             its counter set to first_draw, (key, first_draw) by sol_radiance's rules (the point's SolRayKey or, with keys == NULL,
 *             (key_base + i wrapping, the configuration's first_draw)). The direction is drawn from that generator:
 *               SOL_IRRADIANCE_COSINE  cosine-weighted about the normal, the two draws of a Lambertian vertex (the reference's CosinePdf::generate);
 *               SOL_IRRADIANCE_SPHERE  uniform over the sphere (random_unit_vector: three draws per rejection round); the normal only counts
 *                                      towards validity.
 *             The path is then sol_radiance's path from (position, direction, [tmin, tmax]) with the generator where the direction left it:
 *             the handle's current shader, max_depth, sol_env_sampling and sol_light_sampling modes.
 *   Sums.     SolRadiance holds SUMS, in sol_radiance's association (chunks of 16 samples counted from first_sample).
 *             COSINE: irradiance = pi x sum / samples.     SPHERE: mean radiance over the sphere = sum / samples.
 *   Rays.     sol_irradiance_rays (samples must be 1) writes, for sample first_sample, one SolRay per point - position, tmin, the drawn direction,
 *             tmax - and one SolRayKey - the key and the generator's counter after the direction. An invalid point gives an all-zero ray (itself
 *             invalid) beside (key, first_draw).
 *   Identity. With the same scene, seed and modes, sol_radiance_dev(rays_out, keys_out, samples = 1, first_sample = s) equals sample s's
 *             contribution to sol_irradiance_dev bit for bit: a caller can project the samples onto a basis of their own (for spherical
 *             harmonics up to l = 2 see sol_irradiance_sh below, which does that in one call).
 *   Neutral.  As sol_radiance: neither the accumulator, the auxiliary planes, the render's work counter, the partition, an adaptive session nor
 *             SolStats is touched. Irradiance and radiance queries share their scratch; calls on one handle are ordered by its stream.
 * SOL_EINVAL (sol_last_error names the reason), in sol_radiance's order and before the device is looked for: a null scene or configuration; a
 * wrong size; samples == 0 (sol_irradiance_rays: samples != 1), or first_sample + samples beyond 2^32 - 16; n above 2^31; an unknown mode; a
 * scene with a constant medium; with n > 0 a null point or output pointer. n == 0 succeeds and touches nothing. */
enum { SOL_IRRADIANCE_COSINE = 0, SOL_IRRADIANCE_SPHERE = 1 };
/* size = sizeof(SolIrradianceConfig) = 32: size 0, samples 4, first_sample 8, first_draw 12, seed 16, key_base 24, mode 28 */
typedef struct SolIrradianceConfig { uint32_t size, samples, first_sample, first_draw; uint64_t seed; uint32_t key_base, mode; } SolIrradianceConfig;
/* Device pointers (n SolRay points, n SolRayKey or NULL, n SolRadiance out, on the scene's device), on the scene's stream, asynchronous. */
int sol_irradiance_dev(SolScene* scene, const void* points_dev, const void* keys_dev, size_t n, const SolIrradianceConfig* config, void* out_dev);
/* Host arrays, staged through buffers the handle owns; blocks. */
int sol_irradiance(SolScene* scene, const SolRay* points, const SolRayKey* keys, size_t n, const SolIrradianceConfig* config, SolRadiance* out);
/* Device pointers (n SolRay points, n SolRayKey or NULL; n SolRay and n SolRayKey out), on the scene's stream, asynchronous. */
int sol_irradiance_rays(SolScene* scene, const void* points_dev, const void* keys_dev, size_t n, const SolIrradianceConfig* config, void* rays_out_dev,
                        void* keys_out_dev);

/* ---- SH irradiance queries (EXTENSION, not in the reference) --------------------------------------------------------------
 * "What light arrives at this point, from where?" - the gather of an irradiance query projected onto spherical harmonics: nine coefficients
 * per colour channel, the form light probes and irradiance volumes keep. One probe then lights any normal, and a volume of probes can be
 * interpolated. One call in place of 2 x samples launches (sol_irradiance_rays + sol_radiance_dev per sample) and a projection of the caller's.
 *   Points.   Points, their validity, keys, first_draw and the two modes are sol_irradiance's, word for word. An invalid point answers 27 zero
 *             words and samples = 0, decided before any search.
 *   Paths.    Sample s of point i draws its direction d_s as sol_irradiance does, from the stream of (seed, key, s) at first_draw, and is then
 *             sol_radiance's path in the handle's current shader, max_depth, sol_env_sampling and sol_light_sampling modes. Its colour c_s is,
 *             on the bits, what sol_radiance_dev(rays_out, keys_out, samples = 1, first_sample = s) answers over what sol_irradiance_rays
 *             writes for sample s: 0 + colour.
 *   Basis.    Real SH up to l = 2 on d_s = (x, y, z) as drawn, not normalised again, without the Condon-Shortley sign, in the order
 *             (l, m) = (0,0), (1,-1), (1,0), (1,1), (2,-2), (2,-1), (2,0), (2,1), (2,2):
 *               Y0 = k0                    Y1 = k1 y                Y2 = k1 z
 *               Y3 = k1 x                  Y4 = (k2 x) y            Y5 = (k2 y) z
 *               Y6 = k3 ((3 (z z)) - 1)    Y7 = (k2 x) z            Y8 = k4 ((x x) - (y y))
 *             k0 .. k4 are the fp32 roundings of 0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005,
 *             0.5462742152960396; every operation is one fp32 rounding in the bracketing shown (no fused multiply-add).
 *   Sums.     SolSh9.c[k][channel] is the SUM over the samples of fl(c_s[channel] x Y_k(d_s)), in sol_radiance's association: chunks of 16
 *             samples counted from first_sample, a chunk sum 0 + t + t .. in sample order, the result ((0 + chunk0) + chunk1) + ..;
 *             SolSh9.samples is the sample count.
 *   Estimators. SOL_IRRADIANCE_SPHERE: the radiance coefficients are L_k = 4 pi x c[k] / samples, and the irradiance for a unit normal n is
 *             the sum over k of A_l(k) L_k Y_k(n) with A = (pi, 2 pi / 3, pi / 4) for l = 0, 1, 2. SOL_IRRADIANCE_COSINE: pi x c[k] / samples
 *             estimates the cosine-weighted projection about the point's normal. The kernels do not care which mode is used.
 *   Neutral.  As sol_radiance. The scratch is shared with the radiance and irradiance queries; calls on one handle are ordered by its stream.
 * SOL_EINVAL: sol_irradiance's refusals, in the same order and with the same words, before the device is looked for - a scene with a constant
 * medium among them. n == 0 succeeds on any scene and touches nothing. There is no host mirror. */
typedef struct SolSh9 { float c[9][3]; uint32_t samples; } SolSh9;   /* 112 bytes; 16-byte aligned in device memory; sums, not means */
/* Device pointers (n SolRay points, n SolRayKey or NULL, n SolSh9 out, on the scene's device), on the scene's stream, asynchronous. */
int sol_irradiance_sh_dev(SolScene* scene, const void* points_dev, const void* keys_dev, size_t n, const SolIrradianceConfig* config, void* out_dev);
/* Host arrays, staged through buffers the handle owns; blocks. */
int sol_irradiance_sh(SolScene* scene, const SolRay* points, const SolRayKey* keys, size_t n, const SolIrradianceConfig* config, SolSh9* out);

/* ---- visibility gathers (EXTENSION, not in the reference) -----------------------------------------------------------------
 * "How much of the hemisphere, or of the sphere, is open at this point?" - ambient occlusion and bent normals for lightmap texels and vertices,
 * sky visibility for probes, and the hit-distance moments an irradiance volume keeps beside its SH coefficients (mean and mean-square distance,
 * the Chebyshev test against light leaking through walls). One call in place of 2 x samples launches (sol_irradiance_rays + sol_query_dev per
 * sample) and a reduction of the caller's.
 *   Points.   Points, their validity, keys, key_base, first_draw, seed, first_sample, samples and the two direction modes are sol_irradiance's,
 *             word for word; the configuration is SolIrradianceConfig as it stands. A point's tmax is the occlusion radius, in units of the
 *             drawn direction's length (1 up to rounding). mode is sol_query's: SOL_QUERY_OCCLUDED or SOL_QUERY_CLOSEST. An invalid point
 *             answers eight zero words, decided before any search.
 *   Samples.  For sample s of a valid point i the ray is exactly the row sol_irradiance_rays writes for (point, s): position, tmin, the
 *             direction d drawn from the stream of (seed, key, s) with its counter at first_draw, tmax. Its status is what sol_query answers
 *             for that ray in the given mode - the (t, dfs) rule, and in a scene with needle triangles the searches behind a refused hit: 63
 *             of them, each up to the ray's own tmax, then a miss.
 *               SOL_RAY_HIT   hits += 1; under SOL_QUERY_CLOSEST also t_sum += t and t2_sum += fl(t x t), t being SolRayHit.t - each one fp32
 *                             rounding, no fused multiply-add. A hit adds nothing to b.
 *               SOL_RAY_MISS  open += 1 and b += d per component. A miss adds nothing to the t sums.
 *             A made ray that is itself invalid is searched for nothing and counted in neither counter; that happens only when the normal's
 *             squared length is not a normal fp32 number (the condition sol_irradiance states). So hits + open <= samples, with equality for
 *             every point that meets the condition. Under SOL_QUERY_OCCLUDED the counters and b are, on the bits, those of
 *             SOL_QUERY_CLOSEST (the searches stop early where they may); t_sum and t2_sum stay +0.
 *   Sums.     The float fields are SUMS in sol_radiance's association: chunks of 16 samples counted from first_sample, a chunk sum
 *             0 + x + x .. in sample order, the result ((0 + chunk0) + chunk1) + ..; the counters are plain integers; `samples` is the sample count.
 *   Estimators. SOL_IRRADIANCE_COSINE: ambient occlusion (the open share of the cosine-weighted hemisphere) = open / samples; the bent normal
 *             is b normalised. SOL_IRRADIANCE_SPHERE: sky visibility = open / samples. With a finite radius tmax the mean hit distance
 *             clamped to it is (t_sum + open x tmax) / samples, and the second moment (t2_sum + open x tmax x tmax) / samples.
 *   Neutral.  As sol_query and sol_radiance: neither the accumulator, the auxiliary planes, the render's work counter, the partition, an
 *             adaptive session nor SolStats is touched. The scratch is shared with the radiance queries; calls on one handle are ordered by
 *             its stream.
 * SOL_EINVAL (sol_last_error names the reason), before the device is looked for and in this order: a null scene; an unknown mode (sol_query's
 * sentence); the configuration and n as sol_irradiance judges them, in its order and words; then n == 0 succeeds on any scene and touches
 * nothing; a scene with a constant medium (sol_query's sentence: a medium's hit is a draw keyed by a path); a null point or output pointer.
 * SOL_EDEVICE without a GPU comes after all of these. There is no host mirror. */
/* 32 bytes; 16-byte aligned in device memory; sums and counts, not means */
typedef struct SolVisibility { float bx, by, bz; uint32_t open; float t_sum, t2_sum; uint32_t hits, samples; } SolVisibility;
/* Device pointers (n SolRay points, n SolRayKey or NULL, n SolVisibility out, on the scene's device), on the scene's stream, asynchronous. */
int sol_visibility_dev(SolScene* scene, int mode, const void* points_dev, const void* keys_dev, size_t n, const SolIrradianceConfig* config, void* out_dev);
/* Host arrays, staged through buffers the handle owns; blocks. */
int sol_visibility(SolScene* scene, int mode, const SolRay* points, const SolRayKey* keys, size_t n, const SolIrradianceConfig* config, SolVisibility* out);

/* ---- lightmap texel points (EXTENSION, not in the reference) ---------------------------------------------------------------
 * The gathers above take points the caller already has. For a lightmap the points are the texels of an atlas: sol_lightmap_points rasterises
 * a mesh's lightmap UVs on the device into the W x H SolRay point rows sol_irradiance, sol_irradiance_sh and sol_visibility take, and
 * sol_lightmap_dilate pads the chart borders of the baked result, so that vertices, uvs -> points -> gather -> dilate is three calls on device
 * memory. The geometry is the caller's (typically what sol_scene_set_triangles gets, as floats); the handle supplies the device, the stream and
 * scratch. Nothing is traced: a scene with a constant medium is not refused. All arithmetic is fp32, every operation rounded once, no fused
 * multiply-add, `/` and sqrt correctly rounded; csrc/sol_lightmap.h is the rule as code and tests/lightmap_ref.py its restatement in numpy.
 *   Atlas.    Texel (i, j), i in [0, W) along u, j in [0, H) along v with row 0 at v = 0, lies at index j * W + i; its centre is
 *             P = ((float)i + 0.5f, (float)j + 0.5f). A UV corner in texel space is (u * (float)W, v * (float)H); A, B, C are a triangle's three.
 *   Skipped.  A triangle claims nothing when one of its 6 UV words, 9 position words or (when given) 9 normal words is not finite; when
 *             area2 = (Bx - Ax) * (Cy - Ay) - (By - Ay) * (Cx - Ax) is zero or not finite; or when the squared length of
 *             cross3(v1 - v0, v2 - v0) is not a finite, normal fp32 number.
 *   Candidates. A triangle claims only among the texels whose closed square [i, i + 1] x [j, j + 1] overlaps its closed texel-space bounding
 *             box: (float)i <= max x && (float)(i + 1) >= min x, and likewise in y.
 *   Edges.    edge(Q, R, P) = (Rx - Qx) * (Py - Qy) - (Ry - Qy) * (Px - Qx), always evaluated with (Q, R) in lexicographic order (x, then y) and
 *             negated when the triangle's own order is the other one: two triangles that share an edge compute the same number for it, a centre
 *             on the edge is inside both and none falls between them. e0 = edge(B, C, P), e1 = edge(C, A, P), e2 = edge(A, B, P); when
 *             area2 < 0 all four are negated.
 *   Claims.   Centre inside: e0 >= 0 && e1 >= 0 && e2 >= 0 at the centre. Conservative only (SOL_LIGHTMAP_CONSERVATIVE, centre not inside):
 *             for each of the three edges the maximum over the square's four corners is >= 0 - evaluated as "some corner's value is >= 0".
 *   Owner.    Among the triangles with the centre inside the lowest index; where there is none, the lowest index among the conservative-only
 *             claims. Whatever the scheduling: one atomic minimum per claim on the key index | (conservative_only << 31).
 *   Row.      b1 = e1 / area2, b2 = e2 / area2, b0 = (1 - b1) - b2. A conservative-only texel clamps first: b_k' = b_k > 0 ? b_k : 0,
 *             s = (b0' + b1') + b2', b1 = b1' / s, b2 = b2' / s, b0 = (1 - b1) - b2. Position per component ((v0 * b0) + (v1 * b1)) + (v2 * b2).
 *             Normal: with normals the same interpolation, then n / sqrt(n.x * n.x + n.y * n.y + n.z * n.z); when that squared length is not a
 *             finite, normal number, or normals is null, the same of cross3(v1 - v0, v2 - v0). The row is (position, tmin, normal, tmax), the
 *             SolTexel (index, b1, b2, 1: centre inside or 2: conservative only).
 *   Unowned.  Eight zero words - an invalid point, which the gathers answer with zeros before any search - and the SolTexel (0xFFFFFFFF, 0, 0, 0).
 * Neutral as the queries are: neither the accumulator, the planes, the work counter nor SolStats is touched.
 * SOL_EINVAL (sol_last_error names the reason), before the device is looked for and in this order: a null scene or configuration; a wrong
 * size; reserved != 0; unknown flags; width or height of 0 or above 16384; tmin / tmax failing the point rule (0 <= tmin <= tmax, tmin finite,
 * tmax not NaN); n_triangles > 2^31 - 2; with n_triangles > 0 a null vertex or UV pointer; a null output pointer. n_triangles == 0 writes an
 * all-empty atlas. SOL_EDEVICE without a GPU comes after all of these. There is no host mirror. */
#define SOL_LIGHTMAP_CONSERVATIVE 1u
#define SOL_LIGHTMAP_MAX_SIZE 16384u
#define SOL_TEXEL_NONE 0xFFFFFFFFu
typedef struct SolLightmapConfig {
  uint32_t size, width, height, flags; /* size = sizeof(SolLightmapConfig); flags: SOL_LIGHTMAP_CONSERVATIVE */
  float tmin, tmax;                    /* written into every point row */
  uint32_t reserved[2];                /* zero */
} SolLightmapConfig;
/* 16 bytes; 16-byte aligned in device memory */
typedef struct SolTexel {
  uint32_t triangle; /* SOL_TEXEL_NONE: no owner */
  float b1, b2;
  uint32_t flags;    /* 1: centre inside; 2: conservative only; 0: no owner */
} SolTexel;
/* Device pointers on the scene's device (n x 9 floats, n x 9 floats or NULL, n x 6 floats; W x H SolRay and W x H SolTexel out, 16-byte aligned),
 * on the scene's stream, asynchronous. */
int sol_lightmap_points_dev(SolScene* scene, const void* vertices_dev, const void* normals_dev, const void* uvs_dev, size_t n_triangles,
                            const SolLightmapConfig* config, void* points_out_dev, void* texels_out_dev);
/* Host arrays, staged through a buffer the handle owns; blocks. */
int sol_lightmap_points(SolScene* scene, const float* vertices, const float* normals, const float* uvs, size_t n_triangles, const SolLightmapConfig* config,
                        SolRay* points_out, SolTexel* texels_out);
/* Border dilation: what finishes a bake, so that bilinear filtering does not bleed black into the chart borders. values: W x H rows of stride_bytes
 * (a multiple of 4, at least 4 x channels) whose leading `channels` words (1..32) are floats - SolRadiance (3 channels, stride 16), SolSh9 (27,
 * 112), plain float planes. Rows of owned texels (texels[x].triangle != SOL_TEXEL_NONE) are copied whole. In pass k = 1 .. passes (at most 254)
 * a texel uncovered at the pass's start with at least one covered neighbour among its eight (none outside the atlas, no wrap) is filled: per
 * channel (0 + x + x ..) / (float)count over the covered neighbours in the order (di, dj) = (-1,-1), (0,-1), (1,-1), (-1,0), (1,0), (-1,1), (0,1),
 * (1,1); the rest of its row is zero; it counts as covered from the next pass on. A row never filled is zero. pass_of (or NULL): per texel 0
 * owned, k filled in pass k, 255 never filled. out may not be values.
 * SOL_EINVAL before the device is looked for, in this order: a null scene; a null texel, value or output pointer; width or height of 0 or
 * above 16384; channels outside 1..32; a stride that is no multiple of 4 or below 4 x channels; passes above 254; out == values. */
int sol_lightmap_dilate_dev(SolScene* scene, const void* texels_dev, uint32_t width, uint32_t height, const void* values_dev, uint32_t channels,
                            uint32_t stride_bytes, uint32_t passes, void* out_dev, void* pass_of_out_dev);
/* Host arrays, staged through a buffer the handle owns; blocks. */
int sol_lightmap_dilate(SolScene* scene, const SolTexel* texels, uint32_t width, uint32_t height, const void* values, uint32_t channels,
                        uint32_t stride_bytes, uint32_t passes, void* out, uint8_t* pass_of_out);

/* ---- irradiance volumes (EXTENSION, not in the reference) -----------------------------------------------------------------
 * The consumer of sol_irradiance_sh and of sol_visibility's hit-distance moments: a regular grid of probes that is laid out, packed and
 * sampled on the device, so that grid -> sol_volume_points -> sol_irradiance_sh (+ sol_visibility) -> sol_volume_build -> sol_volume_sample is
 * a chain of calls on device memory, and a viewer, a lightmap or a moving object is lit from the baked volume without new paths. The handle
 * supplies the device, the stream and the host routes' staging; the scene is never read: nothing is traced, and a scene with a constant medium
 * is not refused. All arithmetic is fp32, every operation rounded once, no fused multiply-add, `/` and sqrt correctly rounded;
 * csrc/sol_volume.h is the rule as code and tests/volume_ref.py its restatement in numpy. dot(a, b) below is ((ax * bx) + (ay * by)) + (az * bz);
 * pos(x) is x > 0 ? x : 0 (a NaN and -0 give +0).
 *   Grid.     nx x ny x nz probes; probe (i, j, k) is row (k * ny + j) * nx + i. Its position per axis is o + ((float)i * s) - two roundings -, and o
 *             itself on an axis with one probe, whose spacing is never read.
 *   Points.   sol_volume_points writes the nx * ny * nz rows (position, tmin, (0, 0, 1), tmax) that sol_irradiance_sh and sol_visibility take: the
 *             baker and the sampler then agree on every probe position on the bits.
 *   Build.    sol_volume_build packs one SolProbe per grid row from an SolSh9 row and, where given, a SolVisibility row. The SolSh9 rows MUST have
 *             been gathered with SOL_IRRADIANCE_SPHERE: the coefficients are that mode's estimator with the cosine lobe folded in,
 *               e[k][c] = ((sh.c[k][c] * K4PI) / (float)sh.samples) * A[l(k)]
 *             K4PI the fp32 rounding of 4 pi, A the fp32 roundings of pi (k = 0), 2 pi / 3 (k = 1..3), pi / 4 (k = 4..8). A probe is INVALID - 32
 *             zero words - when sh.samples == 0 or one of the 27 sums is not finite. flags bit 0: valid; samples = sh.samples. Moments (flags bit
 *             1; else mean = mean2 = 0) need a visibility row with samples != 0, finite t_sum and t2_sum, and a finite radius > 0 - the tmax the
 *             visibility gather ran with, under SOL_QUERY_CLOSEST:
 *               mean  = (t_sum  + ((float)open * radius)) / (float)samples
 *               mean2 = (t2_sum + (((float)open * radius) * radius)) / (float)samples
 *   Sample.   sol_volume_sample answers one SolRadiance per point row (position p, tmin, normal N, tmax; tmin and tmax are not read): r, g, b the
 *             irradiance, `samples` the number of probes that contributed, 0 to 8 - sol_lightmap_dilate takes the rows as they are (3 channels,
 *             stride 16). A row is INVALID - four zero words - when one of its six position or normal words is not finite or dot(N, N) is not a
 *             finite, normal fp32 number (the condition sol_irradiance states). Otherwise
 *               n = N / sqrtf(dot(N, N));  q = p + (n * normal_bias) per component;  Y = the nine terms of sol_irradiance_sh on n
 *               per axis, count == 1: g = 0;  else g = (q - o) / s;  g = g > 0 ? g : 0;  g = g < (float)(count - 1) ? g : (float)(count - 1)
 *                         i0 = min((int)floorf(g), max(count - 2, 0));  f = g - (float)i0
 *             The eight corners (i0 + dx, j0 + dy, k0 + dz) are visited in the order dz, dy, dx ascending, each with the trilinear weight
 *             w = ((wx * wy) * wz), w_axis = d ? f : (1 - f). A corner with w == 0 is skipped and its probe is not read (the far layer of a
 *             one-probe axis, points on a grid plane); a corner whose probe is invalid is skipped. With P the probe's position:
 *               SOL_VOLUME_BACKFACE   D = P - p; l2 = dot(D, D); where l2 > 0: c = dot(D, n) / sqrtf(l2); b = (c + 1) * 0.5; w = w * ((b * b) + 0.2f)
 *               SOL_VOLUME_CHEBYSHEV  where the probe has moments: D' = P - q; d = sqrtf(dot(D', D')); where d > mean:
 *                                     v = pos(mean2 - (mean * mean)); t = d - mean; den = v + (t * t); where den > 0: h = v / den; w = w * ((h * h) * h)
 *             A corner whose final w is not > 0 (a NaN too) is skipped; the others count in `samples` and add
 *               E[c] = pos((((0 + (e[0][c] * Y0)) + (e[1][c] * Y1)) + ..) + (e[8][c] * Y8));  sum[c] = sum[c] + (w * E[c]);  wsum = wsum + w
 *             both sums from 0 in corner order. The answer is (sum[0] / wsum, sum[1] / wsum, sum[2] / wsum, samples); four zero words where no
 *             probe contributed. One lane adds a point's corners in the stated order: the answer does not depend on the schedule.
 *   Limitation. The moments of a SolProbe are isotropic - one mean and one mean square of the hit distance per probe -, so this Chebyshev factor
 *             cannot tell a wall on one side from open space on the other. The per-direction moments are the octahedral maps of the next
 *             section (sol_visibility_oct, sol_volume_build_depth, sol_volume_sample_depth).
 * Neutral as the queries are: neither the accumulator, the planes, the work counter nor SolStats is touched.
 * SOL_EINVAL (sol_last_error names the reason), before the device is looked for and in this order. All three: a null scene; a null grid; a wrong
 * size; unknown flags; nx, ny or nz of 0; nx * ny * nz above 2^24; an origin that is not finite; on an axis with more than one probe a spacing that
 * is not finite and > 0; a normal_bias that is not finite. Then sol_volume_points: tmin / tmax failing the point rule (0 <= tmin <= tmax, tmin
 * finite, tmax not NaN); a null output pointer. sol_volume_build: a null SolSh9 pointer; a null output pointer (visibility may be NULL; radius is
 * judged per probe, above). sol_volume_sample: n above 2^31; then n == 0 succeeds and writes nothing; a null probe, point or output pointer.
 * SOL_EDEVICE without a GPU comes after all of these. There is no host mirror. */
#define SOL_VOLUME_BACKFACE 1u
#define SOL_VOLUME_CHEBYSHEV 2u
#define SOL_VOLUME_MAX_PROBES 16777216u
#define SOL_PROBE_VALID 1u
#define SOL_PROBE_MOMENTS 2u
/* size = sizeof(SolVolumeGrid) = 48: size 0, nx 4, ny 8, nz 12, origin 16, spacing 28, flags 40, normal_bias 44 */
typedef struct SolVolumeGrid {
  uint32_t size, nx, ny, nz; /* size = sizeof(SolVolumeGrid) */
  float origin[3];           /* the position of probe (0, 0, 0) */
  float spacing[3];          /* between neighbouring probes, per axis */
  uint32_t flags;            /* SOL_VOLUME_BACKFACE | SOL_VOLUME_CHEBYSHEV */
  float normal_bias;         /* a sample looks its cell up at position + unit normal * normal_bias */
} SolVolumeGrid;
/* 128 bytes: eight 16-byte words per probe; 16-byte aligned in device memory */
typedef struct SolProbe {
  float e[9][3];     /* words 0..26: the irradiance coefficients, the cosine lobe folded in */
  float mean, mean2; /* words 27, 28: the mean and the mean square of the hit distance, clamped to the radius */
  uint32_t flags;    /* word 29: SOL_PROBE_VALID | SOL_PROBE_MOMENTS */
  uint32_t samples;  /* word 30: the samples of the gather */
  uint32_t reserved; /* word 31: zero */
} SolProbe;
/* Device pointers (nx * ny * nz SolRay out, 16-byte aligned, on the scene's device), on the scene's stream, asynchronous. */
int sol_volume_points_dev(SolScene* scene, const SolVolumeGrid* grid, float tmin, float tmax, void* points_out_dev);
/* A host array, staged through a buffer the handle owns; blocks. */
int sol_volume_points(SolScene* scene, const SolVolumeGrid* grid, float tmin, float tmax, SolRay* points_out);
/* Device pointers (nx * ny * nz SolSh9, as many SolVisibility or NULL; as many SolProbe out; every one 16-byte aligned, on the scene's device),
 * on the scene's stream, asynchronous. */
int sol_volume_build_dev(SolScene* scene, const SolVolumeGrid* grid, const void* sh_dev, const void* visibility_dev, float radius, void* probes_out_dev);
/* Host arrays, staged through a buffer the handle owns; blocks. */
int sol_volume_build(SolScene* scene, const SolVolumeGrid* grid, const SolSh9* sh, const SolVisibility* visibility, float radius, SolProbe* probes_out);
/* Device pointers (nx * ny * nz SolProbe, n SolRay points; n SolRadiance out; every one 16-byte aligned, on the scene's device), on the scene's
 * stream, asynchronous. */
int sol_volume_sample_dev(SolScene* scene, const SolVolumeGrid* grid, const void* probes_dev, const void* points_dev, size_t n, void* out_dev);
/* Host arrays, staged through a buffer the handle owns; blocks. */
int sol_volume_sample(SolScene* scene, const SolVolumeGrid* grid, const SolProbe* probes, const SolRay* points, size_t n, SolRadiance* out);

/* ---- directional distance moments for irradiance volumes: octahedral maps (EXTENSION, not in the reference) ------------------
 * A SolProbe keeps one mean and one mean square of the hit distance for the whole sphere. Here a probe keeps them per direction, in an R x R
 * octahedral map (the depth map of DDGI): sol_visibility_oct gathers the weighted sums at the probes' points, sol_volume_build_depth turns
 * them into moments and sol_volume_sample_depth is sol_volume_sample with the Chebyshev step reading the map towards the shaded point. All
 * arithmetic is fp32, every operation rounded once, no fused multiply-add, `/` and sqrtf correctly rounded; csrc/sol_depth.h is the rule as code
 * and tests/depth_ref.py its restatement in numpy. dot and pos as above; |x| clears the sign bit; sgn(x) is x >= 0 ? 1 : -1; (float)R is exact.
 *   Map.      R = SolOctConfig.res (4, 8 or 16). Texel (i, j), i along u, j along v, is row j * R + i; the map has no gutter.
 *   Texel direction.  u = ((((float)i + 0.5f) / (float)R) * 2) - 1, v likewise from j;  z = (1 - |u|) - |v|;  where z < 0:
 *             (x, y) = ((1 - |v|) * sgn(u), (1 - |u|) * sgn(v)), else (x, y) = (u, v);  T = (x, y, z) / sqrtf(dot((x, y, z), (x, y, z))).
 *   Gather.   sol_visibility_oct: points, their validity, keys, key_base, first_draw, seed, first_sample, samples and the two direction modes are
 *             sol_irradiance's, word for word (use SOL_IRRADIANCE_SPHERE for a probe); a point's tmax is the radius. Sample s is the ray
 *             sol_irradiance_rays writes for it, its status and t what sol_query answers for that ray under SOL_QUERY_CLOSEST, the searches
 *             behind a refused needle hit included. For every texel  c = pos(dot(T, d)), d as drawn, then c = c * c, sharpness_log2 times, and
 *               SOL_RAY_HIT   w = w + c;  ct = c * t;  wt = wt + ct;  wt2 = wt2 + (ct * t)
 *               SOL_RAY_MISS  w = w + c;  w_open = w_open + c
 *             A made ray that is itself invalid adds nothing. Each of the four sums is in sol_radiance's association over the samples: chunks of
 *             16 counted from first_sample, a chunk 0 + x + x .. in sample order, the result ((0 + chunk0) + chunk1) + ... The answer is R * R
 *             SolOctTexel rows per point; an invalid point answers zero words throughout.
 *   Build.    sol_volume_build_depth, per texel:  s = w_open * radius;  mean = (wt + s) / w;  mean2 = (wt2 + (s * radius)) / w. A texel whose w is
 *             not > 0, or one of whose four sums is not finite, is (radius, radius * radius): open as far as the radius, it never attenuates.
 *   Sample.   sol_volume_sample_depth is sol_volume_sample's rule - rows, corner order, skips, the backface factor, the renormalisation and the
 *             answer - with one change to the SOL_VOLUME_CHEBYSHEV step: for a valid probe at P it takes mean and mean2 from the probe's map and
 *             does not consult the probe's SOL_PROBE_MOMENTS bit. D = q - P; d = sqrtf(dot(D, D)); where d is not > 0 the step is left out. Else
 *               s = (|Dx| + |Dy|) + |Dz|;  px = Dx / s;  py = Dy / s;  where Dz < 0: (px, py) = ((1 - |py|) * sgn(px), (1 - |px|) * sgn(py)), both
 *               from the unfolded pair;  u = (px * 0.5f) + 0.5f;  tx = (u * (float)R) - 0.5f;  tx = tx > -0.5f ? tx : -0.5f;
 *               tx = tx < (float)R - 0.5f ? tx : (float)R - 0.5f;  i0 = (int)floorf(tx);  a = tx - floorf(tx);  likewise v, ty, j0, b from py.
 *             The four neighbours (i0, j0), (i0 + 1, j0), (i0, j0 + 1), (i0 + 1, j0 + 1) have the weights (1 - a) * (1 - b), a * (1 - b),
 *             (1 - a) * b, a * b, and m = ((m00 * w00) + (m10 * w10)) + ((m01 * w01) + (m11 * w11)) for mean and for mean2. A neighbour (i, j)
 *             beyond the map is folded by the octahedron's edge rule in integers: oi = i < 0 || i >= R, oj likewise; ci = i clamped to
 *             [0, R - 1], cj likewise; where oi: cj = (R - 1) - cj; where oj: ci = (R - 1) - ci - beyond one edge the other index is mirrored,
 *             beyond a corner both. Then sol_volume_sample's Chebyshev lines as they stand (where d > mean: ..). Without the flag the map is not read.
 * Neutral as sol_visibility is: no accumulator, plane, work counter or statistic is touched; the scratch is shared with the radiance queries.
 * SOL_EINVAL (sol_last_error names the reason), before the device is looked for and in this order. SolOctConfig, wherever it is judged: null; a
 * wrong size; a res that is not 4, 8 or 16; sharpness_log2 above 6; reserved != 0. sol_visibility_oct: a null scene; the SolIrradianceConfig and n
 * as sol_irradiance judges them; the SolOctConfig; then n == 0 succeeds on any scene and touches nothing; a scene with a constant medium
 * (sol_query's sentence); a null point or output pointer. sol_volume_build_depth: the grid as sol_volume_build judges it (a null scene first);
 * the SolOctConfig; a radius that is not finite and > 0; a null SolOctTexel or output pointer. sol_volume_sample_depth: the grid; the
 * SolOctConfig; n above 2^31; then n == 0 succeeds and writes nothing; a null probe, depth, point or output pointer. Build and sample trace
 * nothing and serve a scene with a constant medium. SOL_EDEVICE without a GPU comes after all of these. There is no host mirror. */
/* 16 bytes: size 0, res 4, sharpness_log2 8, reserved 12 */
typedef struct SolOctConfig {
  uint32_t size;           /* sizeof(SolOctConfig) */
  uint32_t res;            /* 4, 8 or 16 texels along each side of a map */
  uint32_t sharpness_log2; /* 0..6: the lobe is pos(dot(T, d)) to the power 2^sharpness_log2 */
  uint32_t reserved;       /* zero */
} SolOctConfig;
/* 16 bytes; 16-byte aligned in device memory; sums, not means */
typedef struct SolOctTexel { float w, w_open, wt, wt2; } SolOctTexel;
/* 8 bytes; 8-byte aligned in device memory */
typedef struct SolDepthTexel { float mean, mean2; } SolDepthTexel;
/* Device pointers (n SolRay points, n SolRayKey or NULL, n * res * res SolOctTexel out, on the scene's device), on the scene's stream, asynchronous. */
int sol_visibility_oct_dev(SolScene* scene, const void* points_dev, const void* keys_dev, size_t n, const SolIrradianceConfig* config, const SolOctConfig* oct_config,
                           void* out_dev);
/* Host arrays, staged through buffers the handle owns; blocks. */
int sol_visibility_oct(SolScene* scene, const SolRay* points, const SolRayKey* keys, size_t n, const SolIrradianceConfig* config, const SolOctConfig* oct_config,
                       SolOctTexel* out);
/* Device pointers (nx * ny * nz * res * res SolOctTexel; as many SolDepthTexel out), on the scene's stream, asynchronous. */
int sol_volume_build_depth_dev(SolScene* scene, const SolVolumeGrid* grid, const void* oct_dev, const SolOctConfig* oct_config, float radius, void* depth_out_dev);
/* Host arrays, staged through a buffer the handle owns; blocks. */
int sol_volume_build_depth(SolScene* scene, const SolVolumeGrid* grid, const SolOctTexel* oct, const SolOctConfig* oct_config, float radius, SolDepthTexel* depth_out);
/* Device pointers (nx * ny * nz SolProbe, nx * ny * nz * res * res SolDepthTexel, n SolRay points; n SolRadiance out), on the scene's stream, asynchronous. */
int sol_volume_sample_depth_dev(SolScene* scene, const SolVolumeGrid* grid, const void* probes_dev, const void* depth_dev, const SolOctConfig* oct_config,
                                const void* points_dev, size_t n, void* out_dev);
/* Host arrays, staged through a buffer the handle owns; blocks. */
int sol_volume_sample_depth(SolScene* scene, const SolVolumeGrid* grid, const SolProbe* probes, const SolDepthTexel* depth, const SolOctConfig* oct_config,
                            const SolRay* points, size_t n, SolRadiance* out);

/* ---- lightmap filtering: chart-aware a-trous denoising of a baked atlas (EXTENSION, not in the reference) --------------------
 * A gather at the sample counts people bake at is noisy, and an atlas is filtered before it is padded: points -> gather -> filter -> dilate
 * is four calls on device memory. The guides are the atlas's own: every texel's world position and normal are in the point rows
 * sol_lightmap_points wrote, ownership is in the SolTexel rows, and irradiance is pre-albedo, so nothing is demodulated. The handle supplies the
 * device, the stream and the scratch; the scene is never read: nothing is traced, and a scene with a constant medium is served. All arithmetic is
 * fp32, every operation rounded once, no fused multiply-add, `/` correctly rounded, no expf or powf; every clamp is a comparison.
 * csrc/sol_lightmap_filter.h is the rule as code and tests/lightmap_filter_ref.py its restatement in numpy. dot(a, b) is
 * ((ax * bx) + (ay * by)) + (az * bz); pos(x) is x > 0 ? x : 0 (a NaN and -0 give +0).
 *   Inputs.   points: W x H SolRay rows as sol_lightmap_points writes them (position, tmin, normal, tmax); texels: W x H SolTexel rows; values:
 *             W x H rows of stride_bytes whose leading `channels` words (1..32) are floats - the rows sol_lightmap_dilate takes: SolRadiance
 *             (3 channels, stride 16), SolSh9 (27, 112), plain planes. out: the same shape; it may not be values.
 *   Live.     A texel is live when texels[x].triangle != SOL_TEXEL_NONE (a conservative-only texel counts), the three position words and the
 *             three normal words of its point row are finite, and its `channels` value words are finite. Judged once, on the call's inputs.
 *   Not live. Row x of out is row x of values, copied whole; the texel is never a tap.
 *   Passes.   Pass i = 0 .. iterations - 1 has step = 1 << i and f = (float)step (exact). Its input x is values for pass 0, else the output of
 *             pass i - 1. For a live centre p at (px, py) the taps are the 25 texels (px + di * step, py + dj * step), dj the outer loop from -2
 *             to 2, di the inner loop from -2 to 2. A tap outside the atlas (no wrap) or not live is skipped.
 *   Weight.   k = h[di + 2] * h[dj + 2], h = (1/16, 1/4, 3/8, 1/4, 1/16): exact products. The centre tap has w = k. Any other tap q, with
 *             E = P_q - P_p per component and n_p, n_q the stored normals (not renormalised):
 *               s  = sigma_position * f;  l2 = dot(E, E);    w_d  = 1 / (1 + (l2 / (s * s)))
 *               sp = sigma_plane * f;     d  = dot(n_p, E);  w_pl = 1 / (1 + ((d * d) / (sp * sp)))
 *               c  = pos(dot(n_p, n_q));  then c = c * c, normal_power_log2 times
 *               m  = min(channels, 3);  D = 0;  per channel j < m in order:  a = pos(x_p[j] * value_scale);  ta = a / (1 + a);  tb likewise from
 *                    x_q[j];  dv = ta - tb;  D = D + (dv * dv)
 *               sv = sigma_value / f;     w_v = 1 / (1 + (D / (sv * sv)));  w_v = w_v * w_v
 *               w  = (((k * w_d) * w_pl) * c) * w_v
 *             A tap whose w is not > 0 (a NaN too) is skipped. A sigma of +inf switches its factor off exactly: x / inf = 0, 1 / (1 + 0) = 1.
 *   Sums.     From 0, in tap order, one lane per sum: sum[j] = sum[j] + (w * x_q[j]) for every channel j < channels; wsum = wsum + w. The pass
 *             writes sum[j] / wsum; the centre always counts, so wsum >= 9/64. The words of a row behind `channels` (a SolRadiance's samples)
 *             are the centre's words in values, carried through every pass. The last pass writes out.
 * No float atomics, no dependence on scheduling. Neutral as the queries are: no accumulator, plane, counter or statistic is touched.
 * SOL_EINVAL (sol_last_error names the reason), before the device is looked for, from the arguments alone and in this order: a null scene; a null
 * configuration; a wrong size; reserved != 0; width or height of 0 or above 16384; iterations outside 1..8; normal_power_log2 above 7; a sigma
 * that is NaN or below 1e-6 (position, plane, value: the first is named); a value_scale that is not finite and > 0; channels outside 1..32; a
 * stride that is no multiple of 4 or below 4 x channels; a null point, texel, value or output pointer, in that order; out == values.
 * SOL_EDEVICE without a GPU comes after all of these. There is no host mirror. */
/* 64 bytes: size 0, width 4, height 8, iterations 12, normal_power_log2 16, channels 20, stride_bytes 24, sigma_position 28, sigma_plane 32,
 * sigma_value 36, value_scale 40, reserved 44 */
typedef struct SolLightmapFilterConfig {
  uint32_t size, width, height; /* size = sizeof(SolLightmapFilterConfig); the atlas, 1 .. 16384 each way */
  uint32_t iterations;          /* 1..8 passes; pass i has step 1 << i */
  uint32_t normal_power_log2;   /* 0..7: the normal factor is pos(dot(n_p, n_q)) to the power 2^normal_power_log2 */
  uint32_t channels;            /* 1..32 leading float words of a row */
  uint32_t stride_bytes;        /* of a row of values and of out: a multiple of 4, at least 4 x channels */
  float sigma_position;         /* a world length; >= 1e-6 or +inf */
  float sigma_plane;            /* a world length; >= 1e-6 or +inf */
  float sigma_value;            /* in tone-mapped units (x / (1 + x)); >= 1e-6 or +inf */
  float value_scale;            /* finite, > 0: what a value is multiplied with before it is tone-mapped (pi / samples for irradiance sums) */
  uint32_t reserved[5];         /* zero */
} SolLightmapFilterConfig;
/* Device pointers (W x H SolRay, W x H SolTexel, W x H rows of stride_bytes in and out; points and texels 16-byte aligned, rows 4-byte aligned;
 * on the scene's device), one stream-ordered sequence of launches on the scene's stream, asynchronous. */
int sol_lightmap_filter_dev(SolScene* scene, const SolLightmapFilterConfig* config, const void* points_dev, const void* texels_dev, const void* values_dev,
                            void* out_dev);
/* Host arrays, staged through a buffer the handle owns; blocks. */
int sol_lightmap_filter(SolScene* scene, const SolLightmapFilterConfig* config, const SolRay* points, const SolTexel* texels, const void* values, void* out);

/* ---- irradiance moments (EXTENSION, not in the reference) -------------------------------------------------------------------
 * "How noisy is this gather?" - sol_irradiance's answer with the sums of the squared sample colours beside it: error bars on a bake, and what a
 * variance-guided filter (sol_lightmap_filter_var, below) weighs its taps with.
 *   Points.   Points, their validity, keys, key_base, first_draw, seed, the sample range and the two modes are sol_irradiance's, word for word. An
 *             invalid point answers eight zero words, decided before any search.
 *   Samples.  c_s is the colour sample s contributes: on the bits what sol_radiance_dev(rays_out, keys_out, samples = 1, first_sample = s)
 *             answers over what sol_irradiance_rays writes for sample s (0 + colour), as for sol_irradiance_sh.
 *   Sums.     r, g, b are the sums of c_s[channel]; r2, g2, b2 the sums of fl(c_s[channel] x c_s[channel]) - the product rounded once, then
 *             added: no fused multiply-add. All six in sol_radiance's association: chunks of 16 samples counted from first_sample, a chunk sum
 *             0 + t + t .. in sample order, the result ((0 + chunk0) + chunk1) + ... samples is the sample count, reserved is 0.
 *             Consequence: (r, g, b, samples) is sol_irradiance's answer to the same call, bit for bit.
 *   Estimators. With N = samples: the mean is x = sum / N, and for N >= 2 the variance of that mean is pos((sum2 / N) - (x x)) / (N - 1).
 *   Neutral.  As sol_radiance. The scratch is shared with the radiance and irradiance queries; calls on one handle are ordered by its stream.
 * SOL_EINVAL: sol_irradiance's refusals, in the same order and with the same words, before the device is looked for - a scene with a constant
 * medium among them. n == 0 succeeds on any scene and touches nothing. There is no host mirror. */
typedef struct SolMoments { float r, g, b; uint32_t samples; float r2, g2, b2; uint32_t reserved; } SolMoments;  /* 32 bytes; 16-byte aligned in device memory; sums */
/* Device pointers (n SolRay points, n SolRayKey or NULL, n SolMoments out, on the scene's device), on the scene's stream, asynchronous. */
int sol_irradiance_moments_dev(SolScene* scene, const void* points_dev, const void* keys_dev, size_t n, const SolIrradianceConfig* config, void* out_dev);
/* Host arrays, staged through buffers the handle owns; blocks. */
int sol_irradiance_moments(SolScene* scene, const SolRay* points, const SolRayKey* keys, size_t n, const SolIrradianceConfig* config, SolMoments* out);

/* ---- variance-guided lightmap filtering (EXTENSION, not in the reference) ---------------------------------------------------
 * sol_lightmap_filter's value factor compares tone-mapped values against one sigma_value, which cannot serve every sample count: the filter
 * does not know how noisy a texel is. This one does - it takes the SolMoments rows of sol_irradiance_moments, carries a variance of the mean
 * beside every value through the passes (as SVGF does for frames) and divides the squared value difference of a tap by it. The chain is
 * points -> sol_irradiance_moments -> sol_lightmap_filter_var -> sol_lightmap_dilate. Nothing is traced and the scene is never read: a scene
 * with a constant medium is served. All arithmetic is fp32, every operation rounded once, no fused multiply-add, `/` correctly rounded, no
 * expf, powf or sqrtf; every clamp is a comparison; dot and pos as for sol_lightmap_filter. csrc/sol_lightmap_filter_var.h is the rule as code
 * and tests/lightmap_filter_var_ref.py its restatement in numpy.
 *   Inputs.   points, texels: as for sol_lightmap_filter. moments: W x H SolMoments rows. out: W x H SolRadiance rows - what sol_lightmap_filter
 *             returns for such a bake and what sol_lightmap_dilate takes (3 channels, stride 16). variance_out: W x H rows of four floats, or NULL.
 *   Live.     A texel is live when texels[x].triangle != SOL_TEXEL_NONE, the three position and the three normal words of its point row are
 *             finite, samples >= 2, and its six sums are finite. Judged once, on the call's inputs.
 *   Not live. Row x of out is the first four words of row x of moments, copied; row x of variance_out is four zero words; never a tap.
 *   Prepare.  Per live texel, N = (float)samples, M = (float)(samples - 1):  x[j] = sum[j] / N;  v[j] = pos((sum2[j] / N) - (x[j] * x[j])) / M.
 *   Passes.   Pass i = 0 .. iterations - 1 has step = 1 << i and f = (float)step; its input (x, v) is the previous pass's output. For a live centre p:
 *     Variance prefilter.  vb[j] and gs from 0 over the nine texels (px + di, py + dj) - one texel apart, not scaled by step -, dj the outer
 *             loop and di the inner, both from -1 to 1, live taps inside the atlas only: g = h3[di + 1] * h3[dj + 1], h3 = (1/4, 1/2, 1/4), exact;
 *             vb[j] = vb[j] + (g * v_q[j]);  gs = gs + g.  V = (((vb[0] / gs) + (vb[1] / gs)) + (vb[2] / gs)) + variance_floor.
 *     Taps.   The 25 taps, their order, the skips, k, E, w_d, w_pl and c are sol_lightmap_filter's (s = sigma_position * f, sp = sigma_plane * f).
 *     Value factor.  D = 0; per channel j = 0, 1, 2: dv = x_p[j] - x_q[j]; D = D + (dv * dv).  den = (sigma_value * sigma_value) * V.
 *             w_v = 1 / (1 + (D / den));  w_v = w_v * w_v.  No tone map, and sigma_value is not divided by f: the variance shrinks from pass to
 *             pass and tightens the factor by itself. sigma_value = +inf switches the factor off exactly.
 *     Weight. w = (((k * w_d) * w_pl) * c) * w_v; the centre has w = k. A tap whose w is not > 0 (a NaN too) is skipped.
 *     Sums.   From 0, in tap order: sum[j] = sum[j] + (w * x_q[j]);  vs[j] = vs[j] + ((w * w) * v_q[j]);  wsum = wsum + w.
 *             The pass writes x'[j] = sum[j] / wsum and v'[j] = vs[j] / (wsum * wsum).
 *   After the last pass: out = (x[0] * N, x[1] * N, x[2] * N, samples) of the centre - pi x sum / samples still reads it -, variance_out =
 *             (v[0], v[1], v[2], 0).
 * No float atomics, no dependence on scheduling; liveness keeps every index inside the atlas. Neutral as the queries are.
 * SOL_EINVAL (sol_last_error names the reason), before the device is looked for, from the arguments alone and in this order: a null scene; a null
 * configuration; a wrong size; reserved != 0; width or height of 0 or above 16384; iterations outside 1..8; normal_power_log2 above 7; a sigma
 * that is NaN or below 1e-6 (position, plane, value: the first is named); a variance_floor that is not finite and > 0; a null point, texel,
 * moments or output pointer, in that order; out == moments, or variance_out equal to moments or out. SOL_EDEVICE without a GPU comes after all
 * of these. There is no host mirror. */
/* 64 bytes: size 0, width 4, height 8, iterations 12, normal_power_log2 16, sigma_position 20, sigma_plane 24, sigma_value 28, variance_floor 32,
 * reserved 36 */
typedef struct SolLightmapFilterVarConfig {
  uint32_t size, width, height; /* size = sizeof(SolLightmapFilterVarConfig); the atlas, 1 .. 16384 each way */
  uint32_t iterations;          /* 1..8 passes; pass i has step 1 << i */
  uint32_t normal_power_log2;   /* 0..7: the normal factor is pos(dot(n_p, n_q)) to the power 2^normal_power_log2 */
  float sigma_position;         /* a world length; >= 1e-6 or +inf */
  float sigma_plane;            /* a world length; >= 1e-6 or +inf */
  float sigma_value;            /* in standard deviations of the mean; >= 1e-6 or +inf (4: SVGF's value; not tuned on a device) */
  float variance_floor;         /* finite, > 0: added to the prefiltered variance (1e-12 is the Python default; not tuned on a device) */
  uint32_t reserved[7];         /* zero */
} SolLightmapFilterVarConfig;
/* Device pointers (W x H SolRay, SolTexel, SolMoments in; W x H SolRadiance and, or NULL, W x H rows of four floats out; all 16-byte aligned; on
 * the scene's device), one stream-ordered sequence of launches on the scene's stream, asynchronous. */
int sol_lightmap_filter_var_dev(SolScene* scene, const SolLightmapFilterVarConfig* config, const void* points_dev, const void* texels_dev,
                                const void* moments_dev, void* out_dev, void* variance_out_dev);
/* Host arrays, staged through a buffer the handle owns; blocks. */
int sol_lightmap_filter_var(SolScene* scene, const SolLightmapFilterVarConfig* config, const SolRay* points, const SolTexel* texels,
                            const SolMoments* moments, SolRadiance* out, float* variance_out);

/* ---- adaptive irradiance gathers (EXTENSION, not in the reference) -----------------------------------------------------------
 * sol_irradiance_moments spends the same number of paths on every point; this call stops sampling a point once its mean has converged. It runs
 * rounds of samples over the points still active, judges each active point after every round from its own two moments and compacts what is left.
 *   Inputs.   SolIrradianceConfig is sol_irradiance_moments's; its `samples` is the MAXIMUM per point (max below). Points, their validity, keys,
 *             key_base, first_draw, seed, first_sample and the two modes are sol_irradiance's, word for word. out: n SolMoments rows.
 *   Rounds.   Round k = 0, 1, .. gives every active row the samples [first_sample + k * round, first_sample + (k + 1) * round), clipped to
 *             first_sample + max. round is a positive multiple of 16 and min_samples a multiple of 16: every round starts on a chunk boundary
 *             of the row's sample range, so the rounds' chunk sums continue ((0 + chunk0) + chunk1) + .. exactly.
 *   Invariant. A row that ends with samples = N equals, in all eight words, the row sol_irradiance_moments answers for the same point, key and
 *             configuration with samples = N. threshold = 0 never converges: the whole answer is then the fixed call's with samples = max, word
 *             for word. An invalid row answers eight zero words and is never traced.
 *   Stop rule. fp32, every operation rounded once, no fused multiply-add, `/` correctly rounded, no sqrtf (csrc/sol_gather_adaptive.h is the rule
 *             as code, tests/irradiance_adaptive_ref.py its restatement in numpy). After a round a valid active row has the count N and the sums
 *             s[3], q[3] (r, g, b and r2, g2, b2). It stops when one of these holds - the first that does names the reason:
 *               1. one of the six sums is not finite (more samples cannot repair it);
 *               2. N == max;
 *               3. threshold > 0, N >= min_samples, N >= 2, and with Nf = (float)N, M = (float)(N - 1), x[j] = s[j] / Nf,
 *                  v[j] = pos((q[j] / Nf) - (x[j] * x[j])) / M (sol_lightmap_filter_var's Prepare) every channel j has v[j] <= t * t,
 *                  t = threshold * (x[j] > floor ? x[j] : floor).
 *             A stopped row never becomes active again. The compaction is stable and the rule reads the sums only: which rows stop when does not
 *             depend on scheduling.
 *   Stats.    (or NULL) size = sizeof(SolGatherAdaptiveStats) on entry. rounds: the rounds launched (a call split over points: the most any part
 *             ran - what the whole would have run); paths: the sum of the rows' final counts; rows_valid; rows_converged: stopped by 3;
 *             rows_capped: stopped by 2. Written only when the call succeeds.
 *   Neutral.  As sol_radiance. The scratch is the irradiance queries' plus compact buffers of the handle's own, grown on demand up to a bound
 *             (2^22 rows); a larger call is split over points - answers are per point.
 * BOTH forms block: after every round the host reads one block of counters back to learn how many rows are still active, as
 * sol_adaptive_round does. The _dev form returns with `moments_out_dev` complete.
 * SOL_EINVAL (sol_last_error names the reason), before the device is looked for and in this order: sol_irradiance's own refusals of the scene
 * pointer, the configuration and n, in its order and words; a null adaptive configuration; a wrong size; reserved != 0; round of 0 or not a
 * multiple of 16; min_samples not a multiple of 16; a threshold that is NaN, negative or infinite; a floor that is NaN, negative or infinite; a
 * non-null stats of wrong size. Then n == 0 succeeds on any scene and touches nothing; then a scene with a constant medium; then a null point or
 * output pointer. There is no host mirror. */
/* 24 bytes: size 0, round 4, min_samples 8, reserved 12, threshold 16, floor 20 */
typedef struct SolGatherAdaptive { uint32_t size, round, min_samples, reserved; float threshold, floor; } SolGatherAdaptive;
/* 40 bytes: size 0, rounds 4, paths 8, rows_valid 16, rows_converged 24, rows_capped 32 */
typedef struct SolGatherAdaptiveStats { uint32_t size, rounds; uint64_t paths, rows_valid, rows_converged, rows_capped; } SolGatherAdaptiveStats;
/* Device pointers (n SolRay points, n SolRayKey or NULL, n SolMoments out, on the scene's device), on the scene's stream. BLOCKS: one read-back
 * of the active count per round. */
int sol_irradiance_adaptive_dev(SolScene* scene, const void* points_dev, const void* keys_dev, size_t n, const SolIrradianceConfig* config,
                                const SolGatherAdaptive* adaptive, void* moments_out_dev, SolGatherAdaptiveStats* stats);
/* Host arrays, staged through buffers the handle owns; blocks. */
int sol_irradiance_adaptive(SolScene* scene, const SolRay* points, const SolRayKey* keys, size_t n, const SolIrradianceConfig* config,
                            const SolGatherAdaptive* adaptive, SolMoments* out, SolGatherAdaptiveStats* stats);
/* Rows of different counts brought to one count, after the filter and before sol_lightmap_dilate, which averages sums: per SolRadiance row whose
 * count c >= 1 word j = 0, 1, 2 becomes (float)(((double)word_j * (double)target_samples) / (double)c) and the count target_samples
 * (sol_adaptive_rescale's arithmetic: a row with c == target_samples comes back bit for bit); a row with count 0 is copied. out may be rows.
 * Nothing is traced and the scene is not read: a scene with a constant medium is served. SOL_EINVAL: a null scene; target_samples == 0; with
 * n > 0 a null pointer. Device pointers (16-byte aligned), on the scene's stream, asynchronous. */
int sol_radiance_rescale_dev(SolScene* scene, const void* rows_dev, size_t n, uint32_t target_samples, void* out_dev);
/* Host arrays, staged through a buffer the handle owns; blocks. */
int sol_radiance_rescale(SolScene* scene, const SolRadiance* rows, size_t n, uint32_t target_samples, SolRadiance* out);

/* ---- lightmap lookups: a baked atlas sampled at surface points and hits (EXTENSION, not in the reference) --------------------
 * The consumer of a bake, as sol_volume_sample is the volume's: sol_camera_rays -> sol_query (CLOSEST) -> sol_lightmap_coords ->
 * sol_lightmap_sample is a chain of calls on device memory that shows a bake from the scene's camera, lights a hit point from it, or reads it at
 * points that are not texel centres - without the caller restating the atlas convention. Nothing is traced and the scene is never read: a scene
 * with a constant medium is served. All arithmetic is fp32, every operation rounded once, no fused multiply-add, `/` correctly rounded, every
 * clamp a comparison, finite(x) = the exponent field is not all ones; csrc/sol_lightmap_sample.h is the rule as code and
 * tests/lightmap_sample_ref.py its restatement in numpy.
 *   Surface row. A SolTexel (triangle, b1, b2, flags): `triangle` is the row of the uvs / vertices arrays sol_lightmap_points was given, b1 and b2
 *             weigh the triangle's second and third corner, flags != 0 marks a usable row. The SolTexel rows sol_lightmap_points writes are
 *             surface rows already.
 *   Coords.   sol_lightmap_coords turns n SolRayHit rows into surface rows through the caller's table triangle_of_dfs[n_dfs]. A triangle hit's
 *             (u, v) weigh the two edges of the triangle's fp32 RECORD, which starts at the vertex opposite the longest edge
 *             (sol_triangle_rotation above), so an entry carries the rotation k of its triangle in the two top bits:
 *             entry = triangle | k << 30 (triangle < 2^30); SOL_TEXEL_NONE, or any entry with k = 3: a primitive without lightmap. The row is
 *             (entry & 0x3FFFFFFF, b1, b2, 1) with (b1, b2) = (u, v) for k = 0, ((1 - u) - v, u) for k = 1, (v, (1 - u) - v) for k = 2, when
 *             status == SOL_RAY_HIT, kind == SOL_REF_TRIANGLE, dfs_index < n_dfs and the entry names a triangle; else (SOL_TEXEL_NONE, 0, 0, 0).
 *             The parts of a pre-split triangle are copies of one record and answer the original's values. After sol_scene_set_triangles a moved
 *             triangle's rotation is that of its new vertices: the table is made again.
 *   Invalid.  sol_lightmap_sample answers channels + 1 zero words for a row with flags == 0; triangle == SOL_TEXEL_NONE or >= n_triangles; b1 or
 *             b2 not finite; one of the triangle's six UV words not finite; with the chart guard, one of its nine vertex words not finite. Nothing
 *             of the row is used as an address before this is decided.
 *   Atlas coordinates. b0 = (1 - b1) - b2; u = ((u0 * b0) + (u1 * b1)) + (u2 * b2), v likewise (sol_lightmap_points' interpolation);
 *             x = (u * (float)W) - 0.5f, y = (v * (float)H) - 0.5f. Unless x >= -1 && x < (float)W && y >= -1 && y < (float)H no tap is live -
 *             decided before any conversion to an integer.
 *   Taps.     i0 = floorf(x), fx = x - (float)i0, likewise in y. The taps (i0, j0), (i0 + 1, j0), (i0, j0 + 1), (i0 + 1, j0 + 1), in this order,
 *             weigh (1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy - one product each of the rounded factors. A tap outside the atlas
 *             is not live: no wrap, no clamp.
 *   Live.     A tap is live when it is covered - pass_of[tap] != 255 where pass_of (sol_lightmap_dilate's plane) is given, else
 *             texels[tap].triangle != SOL_TEXEL_NONE -, its `channels` value words are finite, and the chart guard does not refuse it.
 *   Chart guard. On when vertices and points are given and chart_radius is finite. P = ((v0 * b0) + (v1 * b1)) + (v2 * b2) per component. A tap with
 *             texels[tap].flags != 0 whose three position words in points[tap] are finite is live only when, E = P_tap - P,
 *             ((E.x * E.x) + (E.y * E.y)) + (E.z * E.z) <= r * r, r * r one product. A tap that only the dilation filled has no point row and
 *             stays live untested (so does an owned tap whose position is not finite): the guard protects against an owned texel of a
 *             neighbouring chart, not against a gutter narrower than the dilation.
 *   Answer.   Per channel sum = ((0 + (w_a * x_a)) + (w_b * x_b)) .. over the live taps in tap order, wsum = ((0 + w_a) + w_b) .. likewise. When
 *             wsum > 0: sum / wsum per channel, then the number of live taps as a uint32_t; else channels + 1 zero words. For channels = 3 the row
 *             is a SolRadiance whose `samples` is 0 to 4, as sol_volume_sample reports its probes.
 *   Nearest.  With SOL_LIGHTMAP_SAMPLE_NEAREST: xn = u * (float)W, yn = v * (float)H; unless xn >= 0 && xn < (float)W && yn >= 0 &&
 *             yn < (float)H there is no tap; else the one tap (floorf(xn), floorf(yn)) under the same liveness rules. Its value words are copied,
 *             not multiplied; the count is 1 or 0.
 * Neutral as the queries are: no accumulator, plane, counter or statistic is touched; calls are ordered by the handle's stream.
 * SOL_EINVAL (sol_last_error names the reason), before the device is looked for and in this order. sol_lightmap_sample: a null scene or
 * configuration; a wrong size; reserved != 0; unknown flags; width or height of 0 or above 16384; channels outside 1..32; a stride that is no
 * multiple of 4 or below 4 x channels; a chart_radius that is NaN or not > 0; exactly one of vertices / points given; a finite chart_radius with
 * neither; n_triangles > 2^31 - 2; n > 2^31; a null UV (with n_triangles > 0), texel, value, coordinate or output pointer; out == values or
 * out == coords. sol_lightmap_coords: a null scene; n > 2^31; n_dfs > 2^31; with n_dfs > 0 a null table; a null hit or output pointer;
 * out == hits. Then n == 0 succeeds and writes nothing. SOL_EDEVICE without a GPU comes after all of these. There is no host mirror
 * (DESIGN.md 15). */
#define SOL_LIGHTMAP_SAMPLE_NEAREST 1u
#define SOL_LIGHTMAP_TABLE_ROTATION_SHIFT 30u
#define SOL_LIGHTMAP_TABLE_TRIANGLE_MASK 0x3FFFFFFFu
/* 32 bytes: size 0, width 4, height 8, channels 12, stride_bytes 16, flags 20, chart_radius 24, reserved 28 */
typedef struct SolLightmapSampleConfig {
  uint32_t size, width, height, channels, stride_bytes, flags; /* size = sizeof(SolLightmapSampleConfig); flags: SOL_LIGHTMAP_SAMPLE_NEAREST */
  float chart_radius;                                          /* a world length, > 0; +inf: no chart guard */
  uint32_t reserved;                                           /* zero */
} SolLightmapSampleConfig;
/* Device pointers (n SolRayHit in, n_dfs uint32_t, n SolTexel out, 16-byte aligned; on the scene's device), on the scene's stream, asynchronous. */
int sol_lightmap_coords_dev(SolScene* scene, const void* hits_dev, size_t n, const void* triangle_of_dfs_dev, size_t n_dfs, void* coords_out_dev);
/* Host arrays, staged through a buffer the handle owns; blocks. */
int sol_lightmap_coords(SolScene* scene, const SolRayHit* hits, size_t n, const uint32_t* triangle_of_dfs, size_t n_dfs, SolTexel* coords_out);
/* Device pointers (n_triangles x 6 floats; W x H SolTexel; W x H bytes or NULL; W x H rows of stride_bytes; n_triangles x 9 floats and W x H
 * SolRay, or both NULL; n SolTexel surface rows in, n rows of channels + 1 words out; texels, points and coords 16-byte aligned, the rest 4-byte
 * aligned), on the scene's stream, asynchronous. */
int sol_lightmap_sample_dev(SolScene* scene, const SolLightmapSampleConfig* config, const void* uvs_dev, size_t n_triangles, const void* texels_dev,
                            const void* pass_of_dev, const void* values_dev, const void* vertices_dev, const void* points_dev, const void* coords_dev,
                            size_t n, void* out_dev);
/* Host arrays, staged through a buffer the handle owns; blocks. */
int sol_lightmap_sample(SolScene* scene, const SolLightmapSampleConfig* config, const float* uvs, size_t n_triangles, const SolTexel* texels,
                        const uint8_t* pass_of, const void* values, const float* vertices, const SolRay* points, const SolTexel* coords, size_t n,
                        void* out);

/* ---- directional lightmaps: an atlas of SolSh9 rows shaded at the caller's normals (EXTENSION, not in the reference) ----------
 * sol_lightmap_points -> sol_irradiance_sh -> sol_lightmap_filter -> sol_lightmap_dilate bake an atlas of nine SH terms per channel;
 * sol_lightmap_sh looks it up at surface rows as sol_lightmap_sample does and evaluates the irradiance E(n) at a normal per row - a normal-mapped
 * surface lit from a baked atlas, on device memory. sol_lightmap_normals gives the surface's own normals for rows that have none. Nothing is
 * traced and the scene is never read: a scene with a constant medium is served. All arithmetic is fp32, every operation rounded once, no fused
 * multiply-add, `/` and sqrtf correctly rounded, every clamp a comparison, finite(x) = the exponent field is not all ones;
 * csrc/sol_lightmap_sh.h is the rule as code and tests/lightmap_sh_ref.py its restatement in numpy.
 *   Lookup.   Surface row, row validity, atlas coordinates, taps, liveness, chart guard and nearest mode are sol_lightmap_sample's above, word for
 *             word, with channels fixed at 27 and a value row of stride_bytes (>= 112, a multiple of 16) that starts with a SolSh9's c[9][3]: a tap
 *             is live only when all 27 of its value words are finite. Word 27 of a row (SolSh9.samples) never enters a value and is never judged.
 *             L[w] = sum / wsum, sum = ((0 + (w_a * x_a)) + (w_b * x_b)) .. and wsum = ((0 + w_a) + w_b) .. over the live taps in tap order,
 *             w = 3k + channel; with SOL_LIGHTMAP_SH_NEAREST the one tap's words are copied. count = the number of live taps (0..4), 0 unless
 *             wsum > 0.
 *   Evaluation. n = the row of `normals` (x, y, z, unused) as it comes; it is NOT normalised. Y_k(n) is the basis of sol_irradiance_sh above
 *             (csrc/sol_sh.h), B_k = A_k * Y_k one product with A = the fp32 roundings of pi (k = 0), 2 pi / 3 (k = 1..3), pi / 4 (k = 4..8) - the
 *             cosine lobe's zonal factors. Per channel t_k = B_k * L[3k + channel], E = ((0 + t_0) + t_1) .. + t_8 in k order, then
 *             E = E * scale, then with SOL_LIGHTMAP_SH_CLAMP E = E > 0 ? E : 0 (NaN becomes 0). The answer is a SolRadiance (E_r, E_g, E_b,
 *             count). `scale` is the caller's: 4 pi / samples for a SPHERE-mode sol_irradiance_sh bake whose rows are sums.
 *   Zeros.    Four zero words for an invalid row; when no tap is live or wsum is not > 0; when a word of n is not finite; when
 *             ((n.x * n.x) + (n.y * n.y)) + (n.z * n.z) is not a finite, non-zero, non-subnormal number.
 *   Coefficients. With SOL_LIGHTMAP_SH_COEFFICIENTS no normal is read (normals may be NULL) and no scale is applied (it is not looked at): the
 *             answer is 28 words a row - the 27 L[w], then count - bit for bit what sol_lightmap_sample answers with channels = 27 over the same
 *             arguments.
 *   Normals.  sol_lightmap_normals writes n rows (nx, ny, nz, 0) for n surface rows by sol_lightmap_points' rule: b0 = (1 - b1) - b2;
 *             g = cross(v1 - v0, v2 - v0), each component (a * b) - (c * d); with vertex normals m = ((n0 * b0) + (n1 * b1)) + (n2 * b2) per
 *             component replaces g when ((m.x * m.x) + (m.y * m.y)) + (m.z * m.z) is finite, non-zero and not subnormal; the vector is divided,
 *             component by component, by the sqrtf of its squared length. Four zero words: flags == 0, triangle == SOL_TEXEL_NONE or
 *             >= n_triangles, b1 or b2 not finite; one of the nine vertex words, or of the nine normal words where given, not finite; a squared
 *             length of the vector that would be normalised that is not finite, zero or subnormal.
 * Neutral as the queries are: no accumulator, plane, counter or statistic is touched; calls are ordered by the handle's stream.
 * SOL_EINVAL (sol_last_error names the call and the reason), before the device is looked for and in this order. sol_lightmap_sh: a null scene; a
 * null configuration; a wrong size; reserved != 0; unknown flags; CLAMP together with COEFFICIENTS; width or height of 0 or above 16384; a stride
 * below 112 or no multiple of 16; a chart_radius that is NaN or not > 0; exactly one of vertices / points given; a finite chart_radius with
 * neither; a scale that is not finite (unless COEFFICIENTS); n_triangles > 2^31 - 2; n > 2^31; a null UV (with n_triangles > 0), texel, value or
 * coordinate pointer; a null normals pointer (unless COEFFICIENTS); a null output pointer; out == values, coords or normals.
 * sol_lightmap_normals: a null scene; n_triangles > 2^31 - 2; n > 2^31; with n_triangles > 0 a null vertex pointer; a null coords or output
 * pointer; out == coords. Then n == 0 succeeds and writes nothing. SOL_EDEVICE without a GPU comes after all of these. There is no host mirror
 * (DESIGN.md 15). */
#define SOL_LIGHTMAP_SH_NEAREST 1u
#define SOL_LIGHTMAP_SH_COEFFICIENTS 2u
#define SOL_LIGHTMAP_SH_CLAMP 4u
/* 32 bytes: size 0, width 4, height 8, stride_bytes 12, flags 16, chart_radius 20, scale 24, reserved 28 */
typedef struct SolLightmapShConfig {
  uint32_t size, width, height, stride_bytes, flags; /* size = sizeof(SolLightmapShConfig); flags: SOL_LIGHTMAP_SH_* */
  float chart_radius, scale;                         /* a world length, > 0; +inf: no chart guard. scale: finite, the caller's factor on E */
  uint32_t reserved;                                 /* zero */
} SolLightmapShConfig;
/* Device pointers (the atlas arguments of sol_lightmap_sample_dev; n SolTexel surface rows and n rows of four floats (x, y, z, unused) in; n
 * SolRadiance out, or n rows of 28 words with COEFFICIENTS; values, normals, coords, texels, points and out 16-byte aligned), on the scene's
 * stream, asynchronous. */
int sol_lightmap_sh_dev(SolScene* scene, const SolLightmapShConfig* config, const void* uvs_dev, size_t n_triangles, const void* texels_dev,
                        const void* pass_of_dev, const void* values_dev, const void* vertices_dev, const void* points_dev, const void* coords_dev,
                        const void* normals_dev, size_t n, void* out_dev);
/* Host arrays, staged through a buffer the handle owns; blocks. */
int sol_lightmap_sh(SolScene* scene, const SolLightmapShConfig* config, const float* uvs, size_t n_triangles, const SolTexel* texels,
                    const uint8_t* pass_of, const void* values, const float* vertices, const SolRay* points, const SolTexel* coords,
                    const float* normals, size_t n, void* out);
/* Device pointers (n SolTexel surface rows; n_triangles x 9 floats; as many vertex-normal floats or NULL; n rows of four floats out; coords and
 * out 16-byte aligned), on the scene's stream, asynchronous. */
int sol_lightmap_normals_dev(SolScene* scene, const void* coords_dev, size_t n, const void* vertices_dev, const void* vertex_normals_dev,
                             size_t n_triangles, void* normals_out_dev);
/* Host arrays, staged through a buffer the handle owns; blocks. */
int sol_lightmap_normals(SolScene* scene, const SolTexel* coords, size_t n, const float* vertices, const float* vertex_normals, size_t n_triangles,
                         float* normals_out);

/* ---- lightmap mip chains: coverage-aware levels, trilinear lookups, the level of detail of a hit (EXTENSION, not in the reference) --
 * sol_lightmap_mips reduces a baked atlas to a chain of coarser levels without mixing uncovered or non-finite texels in; sol_lightmap_sample_lod
 * looks the atlas and its chain up trilinearly at a level of detail per row; sol_lightmap_lod gives that level for the hits of a camera. Nothing is
 * traced and the scene is never read: a scene with a constant medium is served. All arithmetic is fp32, every operation rounded once, no fused
 * multiply-add, `/` and sqrtf correctly rounded, every clamp a comparison, finite(x) = the exponent field is not all ones;
 * csrc/sol_lightmap_mips.h is the rule as code and tests/lightmap_mips_ref.py its restatement in numpy.
 *   Layout.   Level 0 is the caller's atlas: W x H rows of stride_bytes whose leading `channels` words (1..32) are floats, sol_lightmap_dilate's
 *             limits. W_l = (W_{l-1} + 1) / 2 and H_l likewise - a ceiling, so no source texel is dropped; 1 stays 1. Texel (i, j) of level l
 *             stands for the level-0 square [i 2^l, (i + 1) 2^l) x [j 2^l, (j + 1) 2^l). `levels` counts level 0: 1 .. the count at which both
 *             sizes reach 1 (at most SOL_LIGHTMAP_MAX_LEVELS), 0 meaning that count. The chain holds levels 1 .. levels - 1, packed in this order
 *             in one buffer of rows of level 0's stride: level l starts at row sum_{k=1}^{l-1} W_k H_k. The cover plane holds one byte per chain
 *             row at the same row index: 0 covered, 255 not - pass_of's convention, so (level l's rows, level l's cover, W_l, H_l) can be handed
 *             to sol_lightmap_sample as (values, pass_of, width, height). Level 0 is not copied. sol_lightmap_mip_layout answers, from the
 *             arguments alone and without a device, the count in force, every level's size and first row (entry 0: level 0's size and 0; the
 *             entries from the count on: 0) and the chain's rows; each out pointer may be NULL, each array has SOL_LIGHTMAP_MAX_LEVELS entries.
 *   Live.     A level-0 texel is live by sol_lightmap_sample's words: covered - pass_of != 255 where the plane is given, else
 *             texels[].triangle != SOL_TEXEL_NONE - and finite in all `channels` words. A chain texel is live when its cover byte is 0.
 *   Reduction. Texel (i, j) of level l + 1 looks at (2i, 2j), (2i + 1, 2j), (2i, 2j + 1), (2i + 1, 2j + 1) of level l, in this order. The taps
 *             inside level l and live count c. With c > 0 each channel is ((0 + x_a) + x_b ..) / (float)c over the live taps in tap order, and the
 *             words of the row behind `channels` are those of the first live tap (a SolRadiance atlas of one sample count keeps it). The cover
 *             byte is 0 if every channel came out finite; else - a sum overflowed - the whole row is zero and the byte 255. With c == 0: a zero
 *             row, byte 255. A level depends on the level below only: how the kernels split the levels among them changes no bit.
 *   Lookup.   sol_lightmap_sample_lod takes sol_lightmap_sample's arguments, the chain's two buffers, `levels` (in the configuration) and one
 *             float per row. lambda = lod[i], 0 unless lod[i] > 0 (NaN reads as 0), levels - 1 when at least that; l0 = floorf(lambda),
 *             f = lambda - l0. One level's lookup is sol_lightmap_sample's bilinear rule over that level: u, v as there;
 *             x = ((u * (float)W) * 2^-l) - 0.5f, y likewise, 2^-l an exact constant; the range test x >= -1 && x < (float)W_l (and y) and
 *             the inside test of a tap run against the level's own size; taps, weights, coverage (the level's cover byte, != 255) and
 *             finiteness as at level 0; sum / wsum over the live taps in tap order with their count n_l, nothing when wsum is not > 0. The chart
 *             guard applies at level 0 only: a coarser texel has no point row. With f == 0 the answer is level l0's, count n_l0. Otherwise both
 *             l0 and l0 + 1 are looked up: if both have wsum > 0 each channel is (a * (1 - f)) + (b * f), 1 - f rounded once, count
 *             n_a + n_b; if one has, that one's answer and count; if neither, channels + 1 zero words. An invalid surface row answers zeros.
 *             With lod <= 0 or levels == 1 the answer is sol_lightmap_sample's, word for word; there is no nearest mode. For an atlas whose
 *             sizes are powers of two and an integral lod = l the answer is sol_lightmap_sample's over level l with its cover as pass_of, at
 *             every level with W_l = W 2^-l and H_l = H 2^-l - all of them for a square atlas -, on rows whose u W and v H are zero or normal.
 *   Level of detail. sol_lightmap_lod takes per row the SolRay, the SolRayHit and the surface row sol_lightmap_coords made of it, the mesh's
 *             vertices and uvs, the atlas size, `spread` - the angle in radians between the rays of neighbouring pixels - and `bias`. With
 *             N = cross(v1 - v0, v2 - v0), nn = |N|^2, dd = |D|^2, dn = D . N (dot and squared length ((x x) + (y y)) + (z z), a cross
 *             component (a b) - (c d)): c2 = (dn * dn) / (dd * nn), taken as 1/64 unless c2 >= 1/64 (a cosine floor of 1/8); a = the absolute
 *             value of (bx - ax) * (cy - ay) - (by - ay) * (cx - ax) over the corners (u * (float)W, v * (float)H) (sol_lightmap_points'
 *             doubled texel-space area); r = spread * t; q = ((r * r) * (a / sqrtf(nn))) / c2 - the squared number of texels along the
 *             footprint's major axis: the isotropic filter would rather blur than alias. lambda = bias, plus 0.5f * plog2(q) when q > 1, and the
 *             answer is lambda if lambda > 0, else 0. plog2(q) = (float)((int)(bits >> 23) - 127) + (float)(bits & 0x7FFFFF) * 2^-23 is the
 *             piecewise-linear logarithm of q's bits: exact at powers of two, monotone, continuous. The answer is 0 for a row that is not a hit
 *             (status != SOL_RAY_HIT) or has flags == 0; triangle == SOL_TEXEL_NONE or >= n_triangles; t not finite or not > 0; an origin or
 *             direction word of the ray not finite (tmin and tmax are not looked at); one of the triangle's 15 words not finite; a texel-space
 *             area that is zero or not finite; nn zero, subnormal or not finite.
 *   Charts.   There are no chart ids: a coarse level mixes charts that lie closer than its texel. The caller bounds `levels` by the atlas's
 *             gutter, as engines do (a gutter of g texels serves levels up to log2(g) + 1).
 * Neutral as the queries are: no accumulator, plane, counter or statistic is touched; calls are ordered by the handle's stream.
 * SOL_EINVAL (sol_last_error names the call and the reason), before the device is looked for and in this order. sol_lightmap_mip_layout: width
 * or height of 0 or above 16384; levels above the full count. sol_lightmap_mips: a null scene; width or height of 0 or above 16384; channels
 * outside 1..32; a stride that is no multiple of 4 or below 4 x channels; levels above the full count; a null texel or value pointer; with more
 * than one level a null chain or cover output; mips_out == values, texels or cover_out; cover_out == values, texels or pass_of. Then one level
 * succeeds and writes nothing. sol_lightmap_sample_lod: a null scene or configuration; a wrong size; reserved != 0; any flag
 * (SOL_LIGHTMAP_SAMPLE_NEAREST is an unknown flag here); width or height of 0 or above 16384; channels outside 1..32; a stride that is no multiple
 * of 4 or below 4 x channels; a chart_radius that is NaN or not > 0; exactly one of vertices / points given; a finite chart_radius with neither;
 * levels above the full count; n_triangles > 2^31 - 2; n > 2^31; a null UV (with n_triangles > 0), texel, value, coordinate, lod or output
 * pointer; with more than one level a null chain or cover pointer; out == values, coords, lods or mips. sol_lightmap_lod: a null scene; width or
 * height of 0 or above 16384; a spread that is not finite or not > 0; a bias that is not finite; n_triangles > 2^31 - 2; n > 2^31; with
 * n_triangles > 0 a null vertex or UV pointer; a null ray, hit, coordinate or output pointer; out == rays, hits or coords. Then n == 0 succeeds
 * and writes nothing. SOL_EDEVICE without a GPU comes after all of these. There is no host mirror. */
#define SOL_LIGHTMAP_MAX_LEVELS 15u
/* 40 bytes: size 0, width 4, height 8, channels 12, stride_bytes 16, flags 20, chart_radius 24, levels 28, reserved 32 */
typedef struct SolLightmapLodConfig {
  uint32_t size, width, height, channels, stride_bytes, flags; /* size = sizeof(SolLightmapLodConfig); flags: zero */
  float chart_radius;                                          /* a world length, > 0; +inf: no chart guard */
  uint32_t levels;                                             /* level 0 counted; 0: all */
  uint32_t reserved[2];                                        /* zero */
} SolLightmapLodConfig;
/* No device, no handle: the layout rule. */
int sol_lightmap_mip_layout(uint32_t width, uint32_t height, uint32_t levels, uint32_t* levels_out, uint32_t* widths, uint32_t* heights,
                            uint64_t* row_offsets, uint64_t* total_rows);
/* Device pointers (W x H SolTexel, 16-byte aligned; W x H bytes or NULL; W x H rows of stride_bytes, 4-byte aligned; the chain's rows and as
 * many bytes out - rows whose stride and addresses are multiples of 16 move as 16-byte words), on the scene's stream, asynchronous. */
int sol_lightmap_mips_dev(SolScene* scene, const void* texels_dev, const void* pass_of_dev, uint32_t width, uint32_t height, const void* values_dev,
                          uint32_t channels, uint32_t stride_bytes, uint32_t levels, void* mips_out_dev, void* cover_out_dev);
/* Host arrays, staged through a buffer the handle owns; blocks. */
int sol_lightmap_mips(SolScene* scene, const SolTexel* texels, const uint8_t* pass_of, uint32_t width, uint32_t height, const void* values,
                      uint32_t channels, uint32_t stride_bytes, uint32_t levels, void* mips_out, uint8_t* cover_out);
/* Device pointers (the arguments of sol_lightmap_sample_dev; the chain's rows and cover bytes, or NULL with one level; n floats of lod; n rows of
 * channels + 1 words out), on the scene's stream, asynchronous. */
int sol_lightmap_sample_lod_dev(SolScene* scene, const SolLightmapLodConfig* config, const void* uvs_dev, size_t n_triangles, const void* texels_dev,
                                const void* pass_of_dev, const void* values_dev, const void* mips_dev, const void* cover_dev, const void* vertices_dev,
                                const void* points_dev, const void* coords_dev, const void* lods_dev, size_t n, void* out_dev);
/* Host arrays, staged through a buffer the handle owns; blocks. */
int sol_lightmap_sample_lod(SolScene* scene, const SolLightmapLodConfig* config, const float* uvs, size_t n_triangles, const SolTexel* texels,
                            const uint8_t* pass_of, const void* values, const void* mips, const uint8_t* cover, const float* vertices,
                            const SolRay* points, const SolTexel* coords, const float* lods, size_t n, void* out);
/* Device pointers (n SolRay, n SolRayHit, n SolTexel surface rows, 16-byte aligned; n_triangles x 9 and x 6 floats; n floats out), on the scene's
 * stream, asynchronous. */
int sol_lightmap_lod_dev(SolScene* scene, const void* rays_dev, const void* hits_dev, const void* coords_dev, size_t n, const void* vertices_dev,
                         const void* uvs_dev, size_t n_triangles, uint32_t width, uint32_t height, float spread, float bias, void* lods_out_dev);
/* Host arrays, staged through a buffer the handle owns; blocks. */
int sol_lightmap_lod(SolScene* scene, const SolRay* rays, const SolRayHit* hits, const SolTexel* coords, size_t n, const float* vertices,
                     const float* uvs, size_t n_triangles, uint32_t width, uint32_t height, float spread, float bias, float* lods_out);

/* ---- lightmap charts: UV islands labelled, kept apart in dilation and lookups (EXTENSION, not in the reference) -----------------
 * A chart is a set of triangles connected through shared edges. sol_lightmap_charts labels them on the device; sol_lightmap_dilate_charts is
 * sol_lightmap_dilate that never averages across charts and says which chart each texel belongs to; sol_lightmap_sample_charts is
 * sol_lightmap_sample that refuses the taps of another chart by id, dilated taps included; sol_lightmap_chart_levels answers how many mip levels
 * an atlas can have before two charts meet in one level. Nothing is traced and the scene is never read: a scene with a constant medium is
 * served. All arithmetic is fp32, every operation rounded once, no fused multiply-add, `/` correctly rounded, finite(x) = the exponent field is
 * not all ones; csrc/sol_lightmap_charts.h is the rule as code and tests/lightmap_charts_ref.py its restatement in numpy.
 *   Labels.   uvs: n_triangles x 6 floats; vertices: n_triangles x 9 floats or NULL (the meshes are not indexed: connectivity is found from the
 *             values). A triangle is skipped when one of its UV words - with vertices, also one of its vertex words - is not finite: it gets
 *             SOL_CHART_NONE and joins nothing. Edge e (0, 1, 2) of a triangle joins its corners e and (e + 1) % 3; an end point is (u, v), with
 *             vertices (u, v, x, y, z); words are compared as numbers (-0 == +0: every word is x + 0.0f before its bits are looked at). Two live
 *             triangles are connected when the unordered pair of end points of an edge of one equals that of an edge of the other; a shared
 *             corner alone connects nothing; an edge shared by three or more triangles connects them all. A chart is a connected component; its
 *             id is the rank of its lowest triangle index among all charts' lowest indices: ids are dense, 0 .. n_charts - 1, in mesh order, and
 *             do not depend on the schedule. chart_of_triangle_out: n_triangles words; n_charts_out: one word (a device word for the _dev form).
 *   Dilation. sol_lightmap_dilate's arguments, chart_of_triangle / n_triangles in, and a chart plane (W x H words) out; the plane and pass_of
 *             are mandatory outputs. A texel is owned when texels[].triangle < n_triangles and that triangle's chart is not SOL_CHART_NONE: its
 *             row is copied whole, its plane word is its chart, its pass_of 0. Any other texel counts as uncovered. Pass k: a texel uncovered at
 *             the pass's start with at least one covered neighbour among its eight joins chart c, the chart held by the most of those covered
 *             neighbours - on a tie the lowest id; per channel its value is (0 + x + x ..) / (float)count over the covered neighbours of chart c
 *             only, in sol_lightmap_dilate's neighbour order; the rest of its row is zero, its plane word c, its pass_of k. Never filled: a
 *             zero row, plane SOL_CHART_NONE, pass_of 255. When every owned texel is of one chart, out and pass_of are sol_lightmap_dilate's.
 *   Lookup.   sol_lightmap_sample's arguments without vertices and points (chart_radius must be +inf), with chart_of_triangle and the chart
 *             plane. A row is invalid - channels + 1 zero words - under sol_lightmap_sample's rule, and also when
 *             chart_of_triangle[row.triangle] == SOL_CHART_NONE. A tap is live when it is live by sol_lightmap_sample's rule (inside, covered,
 *             finite) and plane[tap] == chart_of_triangle[row.triangle]. Sums, renormalisation, nearest mode and the count word are unchanged.
 *   Levels.   A chart plane (W x H words) and pass_of or NULL. A texel is live when its plane word is not SOL_CHART_NONE and, with pass_of
 *             given, pass_of != 255; the word 0xFFFFFFFE is reserved (MIXED below). Levels are sol_lightmap_mip_layout's. A level-l texel
 *             (l >= 1) reduces its four sources (2i, 2j) .. (2i + 1, 2j + 1) that lie inside level l - 1: NONE when none is live; their chart
 *             when all live ones agree; MIXED otherwise, or when a source is MIXED. mixed_texels[l] counts level l's MIXED texels;
 *             mixed_windows[l] counts its windows (i, j), (i + 1, j), (i, j + 1), (i + 1, j + 1) - a bilinear footprint; 0 <= i < max(W_l - 1, 1),
 *             0 <= j < max(H_l - 1, 1), texels outside the level and NONE ignored - that hold two different charts or a MIXED texel.
 *             levels = 1 + the number of consecutive levels from 1 on with both counts zero: the value to hand to sol_lightmap_mips. Both count
 *             arrays have SOL_LIGHTMAP_MAX_LEVELS entries; entry 0 is zero and so is every entry from the full count of levels on. Level 0 is
 *             not judged: charts may abut there, and level 0 has guards.
 * Neutral as the queries are: no accumulator, plane, counter or statistic is touched; calls are ordered by the handle's stream.
 * SOL_LIGHTMAP_CHARTS=collide (read at every call) masks the edge hash of the labelling to 4 bits - the measured and tested worst case of the
 * match; the labels do not change.
 * SOL_EINVAL (sol_last_error names the call and the reason), before the device is looked for and in this order. sol_lightmap_charts: a null
 * scene; n_triangles > SOL_LIGHTMAP_CHARTS_MAX_TRIANGLES; with n_triangles > 0 a null UV or label output pointer; a null n_charts pointer. Then
 * the host form with n_triangles == 0 writes 0 charts and succeeds. sol_lightmap_dilate_charts: a null scene; a null texel, value, output,
 * pass_of or plane pointer; width or height of 0 or above 16384; channels outside 1..32; a stride that is no multiple of 4 or below
 * 4 x channels; passes above 254; out == values; a null chart_of_triangle with n_triangles > 0; n_triangles >
 * SOL_LIGHTMAP_CHARTS_MAX_TRIANGLES. sol_lightmap_sample_charts: a null scene or configuration; a wrong size; reserved != 0; unknown flag bits;
 * width or height of 0 or above 16384; channels outside 1..32; a stride that is no multiple of 4 or below 4 x channels; a chart_radius that is
 * not +inf; n_triangles > SOL_LIGHTMAP_CHARTS_MAX_TRIANGLES; n > 2^31; a null UV or chart_of_triangle pointer (with n_triangles > 0), a null
 * texel, value, plane, coordinate or output pointer; out == values or coords. Then n == 0 succeeds and writes nothing.
 * sol_lightmap_chart_levels: a null scene; width or height of 0 or above 16384; a null plane, levels, mixed_texels or mixed_windows pointer.
 * Then the host form with a 1 x 1 plane answers one level and zero counts. SOL_EDEVICE without a GPU comes after all of these. There is no host
 * mirror. */
#define SOL_CHART_NONE 0xFFFFFFFFu
#define SOL_LIGHTMAP_CHARTS_MAX_TRIANGLES (1u << 30)
/* Device pointers (n_triangles x 6 floats; n_triangles x 9 floats or NULL; n_triangles words and one word out), on the scene's stream,
 * asynchronous. */
int sol_lightmap_charts_dev(SolScene* scene, const void* uvs_dev, const void* vertices_dev, size_t n_triangles, void* chart_of_triangle_out_dev,
                            void* n_charts_out_dev);
/* Host arrays, staged through a buffer the handle owns; blocks. */
int sol_lightmap_charts(SolScene* scene, const float* uvs, const float* vertices, size_t n_triangles, uint32_t* chart_of_triangle_out,
                        uint32_t* n_charts_out);
/* Device pointers (the arguments of sol_lightmap_dilate_dev; n_triangles words; W x H bytes and W x H words out), on the scene's stream,
 * asynchronous. */
int sol_lightmap_dilate_charts_dev(SolScene* scene, const void* texels_dev, uint32_t width, uint32_t height, const void* values_dev, uint32_t channels,
                                   uint32_t stride_bytes, uint32_t passes, const void* chart_of_triangle_dev, size_t n_triangles, void* out_dev,
                                   void* pass_of_out_dev, void* chart_plane_out_dev);
/* Host arrays, staged through a buffer the handle owns; blocks. */
int sol_lightmap_dilate_charts(SolScene* scene, const SolTexel* texels, uint32_t width, uint32_t height, const void* values, uint32_t channels,
                               uint32_t stride_bytes, uint32_t passes, const uint32_t* chart_of_triangle, size_t n_triangles, void* out,
                               uint8_t* pass_of_out, uint32_t* chart_plane_out);
/* Device pointers (the arguments of sol_lightmap_sample_dev without the guard arrays; n_triangles words; W x H words), on the scene's stream,
 * asynchronous. */
int sol_lightmap_sample_charts_dev(SolScene* scene, const SolLightmapSampleConfig* config, const void* uvs_dev, size_t n_triangles,
                                   const void* texels_dev, const void* pass_of_dev, const void* values_dev, const void* chart_of_triangle_dev,
                                   const void* chart_plane_dev, const void* coords_dev, size_t n, void* out_dev);
/* Host arrays, staged through a buffer the handle owns; blocks. */
int sol_lightmap_sample_charts(SolScene* scene, const SolLightmapSampleConfig* config, const float* uvs, size_t n_triangles, const SolTexel* texels,
                               const uint8_t* pass_of, const void* values, const uint32_t* chart_of_triangle, const uint32_t* chart_plane,
                               const SolTexel* coords, size_t n, void* out);
/* Device pointers (W x H words; W x H bytes or NULL; one word and two arrays of SOL_LIGHTMAP_MAX_LEVELS words out), on the scene's stream,
 * asynchronous. */
int sol_lightmap_chart_levels_dev(SolScene* scene, const void* chart_plane_dev, const void* pass_of_dev, uint32_t width, uint32_t height,
                                  void* levels_out_dev, void* mixed_texels_out_dev, void* mixed_windows_out_dev);
/* Host arrays, staged through a buffer the handle owns; blocks. */
int sol_lightmap_chart_levels(SolScene* scene, const uint32_t* chart_plane, const uint8_t* pass_of, uint32_t width, uint32_t height,
                              uint32_t* levels_out, uint32_t* mixed_texels_out, uint32_t* mixed_windows_out);

/* ---- lightmap unwrap: box-projected charts packed into an atlas (EXTENSION, not in the reference) ---------------------------
 * The first link of the lightmap chain: vertices -> (uvs, chart_of_triangle, result). uvs is the [n, 3, 2] array every other lightmap call
 * takes, chart_of_triangle what sol_lightmap_dilate_charts and sol_lightmap_sample_charts take. Deterministic: the words depend on the arguments
 * alone, whatever the schedule. fp32 with one rounding per operation, `/` and sqrtf correctly rounded; tests/lightmap_unwrap_ref.py restates
 * the rule in numpy float32 and the device equals it word for word. The rule, operation by operation (csrc/sol_lightmap_unwrap.h):
 *   Triangle.   Live when its nine words are finite and n = cross(v1 - v0, v2 - v0) has a dot(n, n) = (nx nx + ny ny) + nz nz that is finite,
 *               not zero and not subnormal (sol_lightmap_points' rule). Its class is (a, s): a the index of the largest |n_k|, the lowest on a
 *               tie, s the sign of n_a. Its unit normal is n / sqrt(dot(n, n)), a division per component. A dead triangle gets SOL_CHART_NONE
 *               and six +0 UV words; sol_lightmap_points lets it claim nothing.
 *   Charts.     Two live triangles are joined when they share an edge (the canonical end point words of sol_lightmap_charts over the positions
 *               alone, equal word for word; the hash decides nothing), have the same class, and (ux_a ux_b + uy_a uy_b) + uz_a uz_b >=
 *               crease_cos. With crease_cos = -1 the class alone decides. Every pair of triangles on one edge is judged. Charts are the
 *               connected components, ids dense and in mesh order: a chart's id is the rank of its lowest triangle.
 *   Projection. A corner projects to the coordinates ((a + 1) % 3, (a + 2) % 3) of its position, each (p * texels_per_unit) + 0.0f.
 *   Extent.     Per chart and axis the minimum lo and maximum hi over its corners, f = floor(lo), e = (floor(hi) + 1) - f. The content
 *               rectangle is e + 2 texels: the e whole texels the corners span and a guard texel on each side, which a conservative claim of
 *               a corner on a whole texel line may take. An e outside 1 .. 32765 (a chart no atlas holds) is reported as content 32767.
 *   Packing.    A chart's rectangle is its content plus `gutter` each way (the gutter to the right and above). Rectangles are sorted by height
 *               descending, then width descending, then chart id ascending, and walked in that order by the greedy shelf rule: a rectangle
 *               joins the current shelf at x while x + w <= width, otherwise it opens the next shelf at x = 0 above the one it leaves; a shelf
 *               is as high as its first rectangle. The walk stops once the shelves' height passes SOL_LIGHTMAP_MAX_SIZE.
 *   UVs.        u = ((x - f_x) + (float)(rect_x + 1)) / (float)width, v = ((y - f_y) + (float)(rect_y + 1)) / (float)height. Corners that
 *               share a position inside a chart get identical words.
 *   Result.     n_charts; live_triangles; used_width, the widest shelf; used_height, the shelves' height; overflow - bit 0: a rectangle is
 *               wider than the atlas, bit 1: used_height > height; content_texels, the sum of the content rectangles (fill ratio:
 *               content_texels / (width x used_height)). On overflow the call still returns SOL_OK: every UV word is +0, every label
 *               SOL_CHART_NONE, and the result carries the sizes, so that a caller can choose another density.
 * Density is that of the projection: a tilted face gets up to sqrt(3) fewer texels along one direction. Self-overlap is NOT detected: the join
 * rule keeps a chart one-to-one in projection locally (a fold flips the class), but a connected surface that passes over itself along its axis,
 * such as a spiral ramp, lands on itself in the atlas. A larger crease_cos cuts such charts apart.
 * No scene: nothing is traced, no handle is read. Both routes allocate their scratch for the call and free it after waiting for the stream:
 * BOTH BLOCK, the device route too. SOL_LIGHTMAP_UNWRAP=collide (read at every call) masks the edge hash to 4 bits, the tested worst case of the
 * match; the words do not change. SOL_LIGHTMAP_UNWRAP=stages times the stages (sol_lightmap_unwrap_stage_ms).
 * SOL_EINVAL (sol_last_error names the call and the reason), before the device is looked for and in this order: a null configuration; a wrong
 * size; reserved != 0; unknown flag bits; width or height of 0 or above 16384; gutter above 64; a texels_per_unit that is not finite and > 0; a
 * crease_cos outside [-1, 1]; n_triangles > SOL_LIGHTMAP_CHARTS_MAX_TRIANGLES; with n_triangles > 0 a null vertex, UV output or label output
 * pointer; a null result pointer. Then the host form with n_triangles == 0 writes a zero result and succeeds. SOL_EDEVICE without a GPU comes
 * after all of these. */
#define SOL_UNWRAP_MAX_GUTTER 64u
#define SOL_UNWRAP_OVERFLOW_WIDTH 1u  /* SolUnwrapResult.overflow: a chart with its gutter is wider than the atlas */
#define SOL_UNWRAP_OVERFLOW_HEIGHT 2u /* used_height > height */
typedef struct SolUnwrapConfig {
  uint32_t size;          /* sizeof(SolUnwrapConfig) */
  uint32_t width, height; /* the atlas in texels; height is the most the packing may use */
  uint32_t gutter;        /* texels between the contents of two charts, 0 .. 64 */
  float texels_per_unit;  /* finite, > 0 */
  float crease_cos;       /* -1 .. 1; -1: the class rule alone decides */
  uint32_t flags;         /* none yet */
  uint32_t reserved;
} SolUnwrapConfig;
typedef struct SolUnwrapResult {
  uint32_t n_charts, live_triangles;
  uint32_t used_width, used_height;
  uint32_t overflow, reserved;
  uint64_t content_texels;
} SolUnwrapResult;
/* Host arrays (n_triangles x 9 floats in; n_triangles x 6 floats, n_triangles words and one result out); blocks. */
int sol_lightmap_unwrap(int device, const SolUnwrapConfig* config, const float* vertices, size_t n_triangles, float* uvs_out,
                        uint32_t* chart_of_triangle_out, SolUnwrapResult* result_out);
/* Device pointers of `device`, launched on hip_stream (a hipStream_t, NULL: the default stream); blocks until the stream has finished. */
int sol_lightmap_unwrap_dev(int device, void* hip_stream, const SolUnwrapConfig* config, const void* vertices_dev, size_t n_triangles,
                            void* uvs_out_dev, void* chart_of_triangle_out_dev, void* result_out_dev);
/* Measurement: with SOL_LIGHTMAP_UNWRAP=stages in the environment a call records device events around its stages; this copies the calling
 * thread's last such call as 8 floats of milliseconds - normals and hash, sort, unions and ids, extents, rectangles and their sort, pack, write,
 * and all of them (launches only: the scratch is allocated before the first event and freed after the last). Zeros before any. */
int sol_lightmap_unwrap_stage_ms(float* stage_ms_out);

/* ---- a new camera for a live scene (EXTENSION, not in the reference) -------------------------------------------------------
 * A handle owns what is expensive and does not depend on the camera: the world tree, the records and textures, the light tree, the environment
 * tables. sol_scene_set_camera looks at the same scene from another viewpoint without building any of it again. After it returns SOL_OK every
 * output of the handle - sol_render + sol_read, sol_render_aux + sol_read_aux, sol_camera_rays, sol_debug_path, queries, adaptive rounds - is
 * byte-identical to that of a handle freshly created from the same description with `camera` in it and brought to the same options, modes and
 * partition. The camera is cast to fp32 exactly as sol_scene_create casts it; nothing is validated that creation does not validate.
 *   Reset: the colour accumulator (also a caller-bound one) and the auxiliary planes with their sample count are zeroed; an open adaptive
 *          session ends, as after sol_clear. The call waits for the scene's stream first and blocks until it is done.
 *   Kept:  the tree and every device table, every SOL_OPT_* value, the sol_env_sampling / sol_light_sampling modes and their tables, the stream,
 *          a bound accumulator, the communicator, the partition in force (rank, world, a balanced table; partition_crc does not change). Every
 *          rank of a job calls it with the same camera; it is not a collective.
 *   Background blocks (SolSceneInfo::background_blocks) are proved again for the new camera, on the device, over the tree the handle walks (the
 *          proof sol_scene_create makes on the host, in the same f64 operations), under creation's conditions: none for a scene with an environment
 *          map, for a handle created with no_background_blocks, or for a camera whose fp32 rays err by three pixels or more.
 *          SOL_CAMERA_NO_BACKGROUND_PROOF skips the proof: every block is traced. Images never depend on it.
 *   Work order: the creation probe's block costs describe the old view and are dropped - launches run in plain chunk-major order, background
 *          blocks last; the fine tail and the balanced partition keep what creation measured. SOL_CAMERA_REPROBE runs creation's 4-spp cost
 *          probe again for the new camera (a no-op where creation ran none; SOL_EINVAL while world > 1). Images do not depend on it either.
 *   Far cameras: the handle keeps the box pad of its creation (S of the creation description: SolRay, "Origins"), a fresh handle would take the
 *          new camera's origin into S. The byte identity above is tested for cameras beside the scene and was MEASURED to hold on
 *          one scene up to 256 * S along two axes (profiles/far_origins.txt); what is promised for a camera further than 4 * S (creation's S)
 *          from the origin is the origin envelope's second half: proper frames and answers, in which hits may be lost. A caller that
 *          moves that far creates a new handle.
 * SOL_EINVAL, before the device is touched: a null scene or camera, a size below 8 or above 4096, unknown flag bits, a non-zero reserved field.
 * SOL_EDEVICE: runtime errors; the handle is then as it was, or has the new camera and no background table - never the new camera with the
 * old table. With sol_kernel_timing on, sol_last_kernel_ms after a call without SOL_CAMERA_REPROBE is the proof kernel's duration. */
#define SOL_CAMERA_NO_BACKGROUND_PROOF 1u  /* do not look for background blocks for the new camera (every block is traced) */
#define SOL_CAMERA_REPROBE             2u  /* run the creation's 4-spp cost probe again for the new camera */
typedef struct SolCameraUpdate { uint32_t size, flags, reserved[2]; } SolCameraUpdate;   /* NULL = all zero */
int sol_scene_set_camera(SolScene* scene, const SolCamera* camera, const SolCameraUpdate* update);
/* Diagnostic: the background-block flags in force (row-major over 8x8 blocks, as sol_background_blocks writes them) and their number. flags may be
 * NULL. SOL_EINVAL: a null scene, a null n_found, n_flags below the block count when flags is not NULL. */
int sol_scene_background_flags(const SolScene* scene, uint8_t* flags, size_t n_flags, uint32_t* n_found);

/* ---- moving the triangles of a live scene (EXTENSION, not in the reference) ------------------------------------------------
 * sol_triangle_from_vertices: Triangle::new_with_tex_coords (src/hittable/triangle.rs:53-96) on the CPU, no device needed: fills v0, v0v1, v0v2,
 * normal, tangent, bi_tangent, area, uv0..2 and bbox of `out` from v = (v0, v1, v2) and uv = (uv0, uv1, uv2), bit for bit as the host library
 * builds a triangle; material and dfs_index are left as they are. SOL_EINVAL: a null argument.
 *
 * sol_scene_set_triangles gives every triangle of a handle created with SolCreateOptions.dynamic_triangles = 1 new vertices: row i of `vertices`
 * (9 doubles: v0, v1, v2) is triangle i of the creation description. The device computes every triangle record again (the same f64 code as
 * sol_triangle_from_vertices) and refits the boxes of the tree it walks in place - topology, slots and exponent origin kept. After SOL_OK every
 * output of the handle (frames, auxiliary planes, sol_camera_rays, queries, sol_debug_path, adaptive rounds, SolSceneInfo::strict_triangles) is
 * byte-identical to that of a handle freshly created, with the same options, from the description D' in which every SolTriangle is
 * sol_triangle_from_vertices of its new vertices (uv, material, dfs_index kept) and every SolBvhNode::bbox the union of its children's, then brought
 * to the same modes, partition and - if the camera was moved - sol_scene_set_camera. The dfs_index numbers stay creation's.
 *   Reset / kept / background blocks / work order: as sol_scene_set_camera (SOL_GEOM_NO_BACKGROUND_PROOF, SOL_GEOM_REPROBE).
 *   SOL_EINVAL before the device is touched: null arguments, n != the scene's triangle count, a size below 8 or above 4096, unknown flag bits,
 *     non-zero reserved words, a handle created without the option, a scene with a constant medium, SOL_GEOM_REPROBE while world > 1.
 *   Refused with the handle exactly as before (no sums cleared): a non-finite vertex (SOL_EINVAL), coordinates beyond 2^38 (SOL_EINVAL), a node
 *     extent beyond the tree's exponent range (SOL_ERANGE: re-create the scene).
 *   Any other failure (SOL_EDEVICE, SOL_ENOMEM: a runtime error after the new records and boxes were adopted, while the light tables, the
 *     background blocks or the scene record were being made again) leaves a handle that is fit only for sol_scene_destroy.
 * sol_scene_set_triangles_dev takes the vertices from device memory (16-byte aligned), without a host copy. Both block until done. */
#define SOL_GEOM_NO_BACKGROUND_PROOF 1u
#define SOL_GEOM_REPROBE             2u
typedef struct SolGeometryUpdate { uint32_t size, flags, reserved[2]; } SolGeometryUpdate;   /* NULL = all zero */
int sol_triangle_from_vertices(const double v[9], const float uv[6], SolTriangle* out);
int sol_scene_set_triangles(SolScene* scene, const double* vertices, uint32_t n, const SolGeometryUpdate* update);
int sol_scene_set_triangles_dev(SolScene* scene, const double* vertices_dev, uint32_t n, const SolGeometryUpdate* update);
/* With sol_kernel_timing on: device-event milliseconds of the last successful sol_scene_set_triangles(_dev) - [0] the upload of the vertices (0 for
 * the device route), [1] the records and lights kernels, [2] the refit launches, [3] the rest (light tables, background proof, probe, uploads). */
int sol_scene_set_triangles_ms(const SolScene* scene, float ms[4]);
/* Diagnostic / tests: copies the triangle records the kernels read (n_records x 48 bytes of intersect records, n_records x 64 bytes of shading
 * records, in the tree's leaf order) and the caller's triangle index of each to the host; any pointer may be NULL; *n_records: their number. */
int sol_scene_triangle_records(SolScene* scene, void* tris, void* shade, uint32_t* triangle_of, size_t capacity, uint32_t* n_records);

/* ---- moving the spheres and quads of a live scene, lights included (EXTENSION, not in the reference) ------------------------------
 * sol_sphere_from_center: Sphere::new (src/hittable/sphere.rs:25-36) on the CPU, no device needed: fills center, radius and bbox of `out`, bit for
 * bit as the host library builds a sphere. sol_quad_from_corner: Quad::new (src/hittable/quad.rs:34-66) without a transformer: fills q, u, v, normal,
 * d, w, area and bbox (padded where an extent is below 0.0001). material and dfs_index are left as they are. SOL_EINVAL: a null argument.
 *
 * sol_scene_set_primitives moves any of the three kinds of a handle created with SolCreateOptions.dynamic_primitives = 1 (and dynamic_triangles = 1).
 * Row i of a kind is primitive i of that kind in the creation description: a triangle row is 9 doubles (v0, v1, v2), a sphere row 4 (centre,
 * radius), a quad row 9 (q, u, v). A NULL pointer: that kind stays where the last successful call left it; at least one is not NULL; the count
 * of every kind given equals the scene's. SOL_PRIMS_DEVICE: every pointer given is device memory, 16-byte aligned, and no host copy is made.
 * All kinds of one call share one refit of the tree, one rebuild of the light tables and one background proof. After SOL_OK every output of the
 * handle (frames, auxiliary planes, sol_camera_rays, queries, sol_debug_path, adaptive rounds, SolSceneInfo::strict_triangles, sol_light_tables /
 * sol_light_tree) is byte-identical to that of a handle freshly created, with the same options, from the description D' in which every moved
 * SolSphere / SolQuad / SolTriangle is the CPU constructor's result for its row (material, uv, dfs_index kept) and every SolBvhNode::bbox the
 * union of its children's, then brought to the same modes, partition and - if the camera was moved - sol_scene_set_camera. A sphere or quad that
 * is a light moves as a light: its weight follows sol_light_weights (the quad's area, 4 pi r^2), the light tree and the power tables are rebuilt.
 *   Reset / kept / background blocks / work order: as sol_scene_set_triangles (SolGeometryUpdate and its two flags are the same).
 *   SOL_EINVAL before the device is touched: a null scene or set, all three pointers NULL, a wrong count, a size below 8 or above 4096 (either
 *     struct), unknown flag bits, non-zero reserved words, a misaligned device pointer, a sphere or quad pointer on a handle created without
 *     dynamic_primitives (a triangle pointer alone needs only dynamic_triangles), a scene with a constant medium, SOL_GEOM_REPROBE while world > 1.
 *   Refused with the handle exactly as before (no sums cleared; the kinds the call did not move, and those it tried to move, are where the last
 *     successful call left them): a parameter that is not finite (SOL_EINVAL), coordinates beyond 2^38 (SOL_EINVAL), a node extent beyond the
 *     tree's exponent range (SOL_ERANGE: re-create the scene).
 *   Any other failure: as sol_scene_set_triangles - a handle fit only for sol_scene_destroy.
 * sol_scene_set_triangles(_dev) are this call with the triangle pointer alone. sol_scene_set_triangles_ms reports the last successful move of
 * either entry point ([0] the upload of the rows, [1] the records and lights kernels of every kind moved, [2] the refit, [3] the rest). */
#define SOL_PRIMS_DEVICE 1u  /* the pointers of the set are device memory */
typedef struct SolPrimitiveSet {
  uint32_t size, flags;     /* sizeof(SolPrimitiveSet); SOL_PRIMS_* */
  const double* triangles;  /* [n_triangles][9] or NULL */
  const double* spheres;    /* [n_spheres][4] or NULL   */
  const double* quads;      /* [n_quads][9] or NULL     */
  uint32_t n_triangles, n_spheres, n_quads;
  uint32_t reserved[3];     /* 0 */
} SolPrimitiveSet;
int sol_sphere_from_center(const double center[3], double radius, SolSphere* out);
int sol_quad_from_corner(const double q[3], const double u[3], const double v[3], SolQuad* out);
int sol_scene_set_primitives(SolScene* scene, const SolPrimitiveSet* set, const SolGeometryUpdate* update);
/* Diagnostic / tests: copies the sphere (kind SOL_REF_SPHERE: n_records x 32 bytes) or quad (SOL_REF_QUAD: n_records x 80 bytes) records the
 * kernels read, in device order, and the caller's index of each to the host; either pointer may be NULL; *n_records: their number. */
int sol_scene_primitive_records(SolScene* scene, int kind, void* records, uint32_t* index_of, size_t capacity, uint32_t* n_records);

#ifdef __cplusplus
}
#endif
#endif /* SOLSTRALE_HIP_H */
