/*
 * rfx.h -- C-ABI of the MI355X-native ReflaxMan trace loop (librfx.so).
 *
 * The reference has no plugin/FFI layer: its path sits behind the C++ class API
 * of Render (src/common/Render.h:7-42), Scene (Scene.h:28-40), Camera
 * (Camera.h:30-62), Material (Material.h:5-19), OmniLight and Texture.  Each
 * entry point below replaces one of those calls (cited per function) so a
 * host-side shim -- include/reflaxman/ (C++ headers), reflaxman_amd/render.py
 * (Python/ctypes), or the cgo/JNI/ctypes stubs in INTEGRATION.md -- can drop in
 * for the reference's CPU render() call.
 *
 * Conventions: plain pointers and sizes only; status codes (rfx_status) instead
 * of the reference's assert()+silent clamps; colours are float RGB; ARGB texels
 * are uint32 0xAARRGGBB; images are row-major, row 0 = bottom (the reference's
 * ry < 0 looks down, Render.cpp:146-156).  Device pointers are HIP device
 * memory of the renderer's device; `stream` arguments are hipStream_t (NULL =
 * the renderer's stream).
 */
#ifndef RFX_H
#define RFX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RFX_ABI_VERSION 5

typedef enum {
  RFX_OK = 0,
  RFX_ERR_ARG = -1,      /* invalid argument (reference: assert + clamp/fallback) */
  RFX_ERR_HIP = -2,      /* HIP runtime failure; rfx_last_error() has the text */
  RFX_ERR_STATE = -3,    /* call not valid in the current state */
  RFX_ERR_IO = -4,       /* file could not be read/written (reference returns false) */
  RFX_ERR_RNG = -5,      /* RNG pre-pass ran short of accepted triples (never expected) */
  RFX_ERR_NODEV = -6     /* no HIP device */
} rfx_status;

enum { RFX_METAL = 0, RFX_DIELECTRIC = 1 };  /* Material::Type (Material.h:8) */

typedef struct rfx_scene rfx_scene;
typedef struct rfx_renderer rfx_renderer;

int rfx_abi_version(void);
const char *rfx_last_error(void);
/* Compile-time options of this build (A/B variants, tools/ab.py), as bits: bit 0 (RFX_BUILD_PRIM_LARGE: per-view
 * chunk lists of large scenes, an option no build has any more) reserved, always 0; per-view masks of per-pixel-loop
 * SSAA frames (RFX_PRIM_SSAA, off by default), of the one-lane-per-sample SSAA modes (RFX_PRIM_LANES, on), one-light
 * kernel instantiations (RFX_ONE_LIGHT, on); bits 8-15: sphere pairs per leaf of the large scenes' BVH. */
enum { RFX_BUILD_PRIM_LARGE = 1, RFX_BUILD_PRIM_SSAA = 2, RFX_BUILD_PRIM_LANES = 4, RFX_BUILD_ONE_LIGHT = 8 };
int rfx_build_options(void);

/* ---------------------------------------------------------------- Scene */
/* Scene(const Color & diffLightColor, float diffLightPower)  -- Scene.cpp:10-15 */
rfx_scene *rfx_scene_create(float diff_r, float diff_g, float diff_b, float diff_power);
void rfx_scene_destroy(rfx_scene *scene);
/* Scene::addSphere(center, radius, Material(type, color, reflectivity, transparency))
 *   -- Scene.cpp:29-39, Sphere.cpp:9-20, Material.cpp:8-14.  Returns the object index (>= 0). */
int rfx_scene_add_sphere(rfx_scene *scene, const float center[3], float radius, int material_type,
                         const float rgb[3], float reflectivity, float transparency);
/* Scene::addTriangle(v1, v2, v3, material) -- Scene.cpp:41-46, Triangle.cpp:11-21.  Returns the object index. */
int rfx_scene_add_triangle(rfx_scene *scene, const float v1[3], const float v2[3], const float v3[3],
                           int material_type, const float rgb[3], float reflectivity, float transparency);
/* A triangle mesh in one call: n_triangles calls of rfx_scene_add_triangle, in index order, on the vertices
 * (vertices[3 i .. 3 i + 2] = vertex i) named by indices[3 t .. 3 t + 2] = (v1, v2, v3) of triangle t, all with one
 * material; the same host precompute, the same object order.  Returns the first triangle's object index (the
 * others follow consecutively; rfx_triangle_set_texture works on each).  An index >= n_vertices: RFX_ERR_ARG, and
 * nothing is added. */
int rfx_scene_add_mesh(rfx_scene *scene, const float *vertices, uint32_t n_vertices, const uint32_t *indices,
                       uint32_t n_triangles, int material_type, const float rgb[3], float reflectivity,
                       float transparency);
/* Plane(pos, norm, material) -- Plane.cpp:9-14, traced by Plane::trace (Plane.cpp:36-73).  The reference's
 * Scene cannot hold a Plane (no addPlane); this is its natural extension: the plane takes an
 * object index in insertion order like any other object (closest-hit ties, shadow self-skip).  The normal is
 * used as given (the reference never normalises it).  Returns the object index. */
int rfx_scene_add_plane(rfx_scene *scene, const float pos[3], const float norm[3], int material_type,
                        const float rgb[3], float reflectivity, float transparency);
int rfx_scene_plane_count(const rfx_scene *scene);
/* Triangle::setTexture(texture, u1, v1, u2, v2, u3, v3) -- Triangle.cpp:110-120.  uv = {u1,v1,u2,v2,u3,v3}. */
int rfx_triangle_set_texture(rfx_scene *scene, int object_index, int texture_index, const float uv[6]);
/* Scene::addLight(origin, radius, color, power) -- Scene.cpp:48-59, OmniLight.cpp:8-14.  Returns the light index. */
int rfx_scene_add_light(rfx_scene *scene, const float origin[3], float radius, const float rgb[3], float power);
/* Scene::addTexture -- Scene.cpp:61-66, from memory: argb == NULL or w*h == 0 is the reference's failed
 * load (empty texture -> procedural checker, Texture.cpp:242-243).  Returns the texture index. */
int rfx_scene_add_texture_argb(rfx_scene *scene, uint32_t width, uint32_t height, const uint32_t *argb);
/* Scene::addTexture(fileName) -- TGA loader of Texture.cpp:34-108 (type 2, 24/32 bpp).  A file that does
 * not load yields an empty texture, as in the reference; *loaded (optional) reports success. */
int rfx_scene_add_texture_file(rfx_scene *scene, const char *path, int *loaded);
/* Scene::setSkyboxTexture(fileName) -- Scene.cpp:68-71, Skybox.cpp:21-37.  Returns 1 if loaded, 0 if not
 * (checker fallback, as the reference), < 0 on error. */
int rfx_scene_set_skybox_file(rfx_scene *scene, const char *path);
/* same, from memory (NULL -> checker) */
int rfx_scene_set_skybox_argb(rfx_scene *scene, uint32_t width, uint32_t height, const uint32_t *argb);
int rfx_scene_counts(const rfx_scene *scene, int *spheres, int *triangles, int *lights, int *textures);
/* The triangle BVH rfx_renderer_set_scene would build for this scene (rfx_renderer_set_tri_accel), on the host: no
 * renderer, no device.  counts[5] = {nodes, leaves, residual triangles, triangles per leaf, depth (internal levels)}
 * is always written; call with the arrays NULL to size them, then again to fill those given:
 *   boxes    : nodes x 12 floats -- child 0's box (lo x y z, hi x y z) then child 1's, as built (before the widening
 *              by the cull margin that the device copy gets);
 *   children : nodes x 2 -- c >= 0 an internal node, c < 0 the leaf ~c; the root is node 0;
 *   leaf_ids : leaves x (triangles per leaf) triangle indices in insertion order (0 = the scene's first triangle),
 *              -1 padding a partly filled leaf;
 *   residual : the triangles outside the tree (an ill-conditioned or singular basis), which every ray tests.
 * Returns 1 with a tree, 0 without one (a small scene, or the depth / node limits cannot be met: counts are 0 but
 * for the leaf size), < 0 on error. */
int rfx_scene_tri_bvh_dump(const rfx_scene *scene, int32_t counts[5], float *boxes, int32_t *children,
                           int32_t *leaf_ids, int32_t *residual);
/* The bundle-cull records a renderer would upload for a small scene (at most 32 spheres and 32 triangles), as built
 * (host only; for tests of the culls, DESIGN.md "Exact work skipping"): recs -- 64 lane records of 8 floats (centre x y z,
 * radius, plane normal x y z, plane offset; sphere i in lane (i & 1) 16 + (i >> 1), triangle i in lane 32 + i), tris --
 * 32 footprint records of 12 floats (v0, |gu|, gu, |gv|, gv, |gu + gv|), valid -- the lanes that hold an object.  Any
 * pointer may be null.  RFX_ERR_STATE for a scene that is not small. */
int rfx_scene_cull_dump(const rfx_scene *scene, float recs[64 * 8], float tris[32 * 12], uint64_t *valid);
/* Mate groups of the scene's triangles (host only; DESIGN.md "Coplanar mates"): triangles whose plane-crossing half of
 * Triangle::trace gives one value for every ray -- the third row of axTrans finite and bitwise equal, v0 finite and
 * bitwise equal on every axis whose row-3 coefficient is not zero.  The small-scene kernels compute that half once per
 * group and ray.  rfx_scene_set_tri_mates(scene, 0) makes every triangle its own group (the same pixels; on by default;
 * read by the next rfx_renderer_set_scene).  rfx_scene_tri_mates returns the triangle count and writes, where given,
 * each triangle's leader -- the lowest triangle index (0 = the scene's first triangle) of its group -- into
 * leader[0 .. triangles - 1], and the operands the rule compares into plane[6 t .. 6 t + 5] = v0 x y z, a31 a32 a33. */
int rfx_scene_set_tri_mates(rfx_scene *scene, int on);
int rfx_scene_tri_mates(const rfx_scene *scene, int32_t *leader, float *plane);
/* Far lights (host only; DESIGN.md "Far lights").  A light L is far when the float32 difference L - d is L, bit for bit,
 * for every point d with max |d_i| < near, where near = min_i (spacing of floats just below |L_i|) / 2 > 0, and when
 * its fields are finite, sqlen(L) is finite and above VERY_SMALL_NUMBER, ang = 1 - radius^2 / sqlen(L) > 0, radius >
 * VERY_SMALL_NUMBER and radius / |L| * 1.001 < 0.5.  Scene::trace's terms of such a light that do not read the hit are
 * then constants, and the small-scene kernels of a scene with exactly one light read them from the light's record at
 * every hit inside the bound (the same pixels; a hit outside it takes the general expressions).
 * rfx_scene_set_far_lights (read by the next rfx_renderer_set_scene): 0 never; 1 (the default) when the scene has one
 * light, it is far, and every sphere and triangle vertex lies inside the bound; 2 for any one-light scene whose light is
 * far, whatever the scene's extent.
 * rfx_scene_far_light writes, where given, terms[8] = {len(L), normalized(L) x y z, 1 - sqrt(ang), near, cos and sin of
 * the shadow rays' cone about normalized(L)} of light `light` -- all 0 when it is not far -- and returns 1 when the
 * scene's launches take the far-light kernels under its current setting, 0 when not, < 0 on error. */
int rfx_scene_set_far_lights(rfx_scene *scene, int mode);
int rfx_scene_far_light(const rfx_scene *scene, int light, float terms[8]);
/* A far light's occluder grid (host only; DESIGN.md "Shadow grid").  For a small scene (at most 32 spheres and 32
 * triangles) with exactly one light, which is far, the builder cuts a world-axis box around the spheres and triangles
 * into at most 2^16 cubic cells and keeps per cell a 64-bit mask, in rfx_scene_cull_dump's lane layout, of the objects a
 * shadow ray toward the light may be reported to hit from any origin in the cell: the bundle cull's own verdict for the
 * cell's circumscribed ball and the light's cone.  The far-light kernels OR the masks of a wave's hits instead of culling
 * the wave's own shadow bundle, wherever every such hit lies inside the light's bound and the box (the same pixels).
 * rfx_scene_set_shadow_grid (read by the next rfx_renderer_set_scene; a new scene takes RFX_SHADOW_GRID = 0, 1 or 2
 * from the environment where set): 0 no grid; 1 (the default) where the scene's launches take the far-light kernels
 * (rfx_scene_far_light returns 1); 2 for any small scene with one far light.
 * rfx_scene_shadow_grid returns the number of cells the current setting builds (0: no grid), < 0 on error, and writes,
 * where given, geom[6] = {box corner x y z, 1 / cell size, cell size, radius of the ball a cell's mask is made for
 * about the cell's centre corner + (i + 1/2) size}, dims[3] = {nx, ny, nz} and the masks, cell (ix, iy, iz) at
 * (iz ny + iy) nx + ix; capacity: the masks the caller has room for (RFX_ERR_ARG if fewer than the grid's). */
int rfx_scene_set_shadow_grid(rfx_scene *scene, int mode);
int rfx_scene_shadow_grid(const rfx_scene *scene, float geom[6], int32_t dims[3], uint64_t *masks, uint64_t capacity);

/* ---------------------------------------------------------------- Camera */
/* Camera(eye, at, fov): view = [ox | oy | oz] columns, row-major _11.._33 -- Camera.cpp:24-38 */
void rfx_camera_view(const float eye[3], const float at[3], float view[9]);
/* rz = W / 2 / tanf(fov / 2) -- Render.cpp:148 (host libm tanf, as the reference) */
float rfx_camera_rz(uint32_t width, float fov);

/* ---------------------------------------------------------------- Images & files */
/* Texture::loadFromTGAFile -- Texture.cpp:34-108.  Call with argb == NULL to query w/h. */
int rfx_tga_load(const char *path, uint32_t *width, uint32_t *height, uint32_t *argb, size_t capacity);
/* Texture::saveToTGAFile / saveToBMPFile -- Texture.cpp:110-173 (32 bpp, rows as stored) */
int rfx_tga_save(const char *path, uint32_t width, uint32_t height, const uint32_t *argb);
int rfx_bmp_save(const char *path, uint32_t width, uint32_t height, const uint32_t *argb);
/* Color::argb over a host float RGB image (Color.cpp:114-117) -- Render::copyImage (Render.cpp:82-101) */
void rfx_argb_from_rgb(const float *rgb, size_t pixels, uint32_t *argb);

/* ---------------------------------------------------------------- Renderer (device) */
int rfx_renderer_create(rfx_renderer **out, int device);
void rfx_renderer_destroy(rfx_renderer *r);
int rfx_renderer_device(const rfx_renderer *r);
/* launches go to this stream (hipStream_t); NULL = a non-blocking stream the renderer owns (so work on the
 * legacy default stream is NOT ordered with it: callers that mix in their own work pass their stream) */
int rfx_renderer_set_stream(rfx_renderer *r, void *hip_stream);
/* upload the scene (host precompute already done by the builder calls) */
int rfx_renderer_set_scene(rfx_renderer *r, const rfx_scene *scene);
/* Trace-launch schedule (no effect on any pixel): 1 (default) = on launches of >= 65536 tiles (8x8 pixels,
 * one wave each; 3840x2160 has 129,600) waves take the tiles longest-first, in the order sorted from an
 * earlier launch's measured per-tile clock costs of the same grid (re-sorted every 4th launch; the first
 * launch, or one after a grid change, runs tiles in raster order); 3 = the same on every launch size;
 * 0 = raster order, no cost recording; 2 = raster order with cost recording (A/B of the sort's overhead).
 * Block-preview frames (sample_num < 0) always run in raster order. */
int rfx_renderer_set_tile_order(rfx_renderer *r, int mode);
/* Ray regrouping of plain one-sample frames (no pixel changes): a trace still alive after park_after bounce
 * segments is parked in an HBM queue and resumed by a second kernel whose lanes each take the next queued trace as
 * soon as theirs ends (lanes whose traces ended no longer idle in their tile's wave).  -1 (default) = after 2
 * segments on scenes with more than 32 spheres or triangles, off on small ones; 0 = off; n >= 1 = after n segments
 * on any scene. */
int rfx_renderer_set_regroup(rfx_renderer *r, int park_after);
/* regrouped frames: 1 = the parked traces are counting-sorted by direction octant and origin cell before the bounce
 * kernel takes them, 0 (default) = taken in park order (a tile's survivors together: faster on C5).
 * Changes the schedule, never a value. */
int rfx_renderer_set_regroup_sort(rfx_renderer *r, int on);
/* Which bounce kernel the last trace launch ran: 0 = none (not regrouped), 1 = the global-memory BVH form, 2 = the
 * LDS-staged BVH form (large scenes whose sphere BVH fits the LDS; 1 when the runtime refused its LDS size).  The
 * form speaks of the sphere BVH alone: a scene's triangle BVH is read from global memory in either form (a mesh
 * without a sphere BVH runs form 1), and only the lanes' traversal stacks are shared with it. */
int rfx_renderer_bounce_form(const rfx_renderer *r);
/* Triangle BVH of scenes with more than 32 spheres or more than 32 triangles (no pixel changes): -1 (default) = built
 * for scenes of at least 128 triangles, 0 = off (every ray tests the triangles in 64-wide chunks, culled by the wave
 * bundle only), 1 = built whenever the scene is not small and the tree meets the kernels' limits (16 levels, 32767
 * nodes); 2 = as 1, and narrow bundles (a tile's primary rays) walk the tree too instead of culling every triangle's
 * bound for the wave -- measured slower on all but one scene, kept for A/B timing and the tests.  Takes
 * effect at the next rfx_renderer_set_scene. */
int rfx_renderer_set_tri_accel(rfx_renderer *r, int mode);
/* The hierarchies of the uploaded scene (RFX_ERR_STATE without one): all zero where none was built. */
typedef struct {
  int32_t tri_nodes, tri_depth;   /* triangle BVH: nodes, internal levels */
  int32_t tri_leaf_size;          /* triangles per leaf of this build */
  int32_t tri_in_leaves;          /* triangles the tree holds */
  int32_t tri_residual;           /* triangles outside it, tested by every ray */
  int32_t sph_nodes, sph_depth;   /* sphere-pair BVH */
  int32_t narrow_tri_bvh;         /* 1: narrow bundles (a tile's primary rays) walk the triangle tree too */
} rfx_accel_info;
int rfx_renderer_accel_info(const rfx_renderer *r, rfx_accel_info *out);
/* Primary-bundle cull masks of small-scene plain frames and of SSAA frames run one sample per lane (sampleNum 2, 4,
 * 8, and jittered sampleNum 1) (no pixel changes): the first segment's cull masks of every wave tile, computed by one
 * extra launch for a view (camera, frame geometry, sampling, scene) and reused while the view stays.  1 (default) = built when a view repeats (the second frame of a still camera on), so a camera that
 * moves every frame never pays for them; 2 = built before every launch; 0 = off (per-launch bundles).  SSAA frames of
 * sampleNum > 8 (a wave per pixel) take one closest-hit mask per pixel, built for every view and every launch of a split
 * frame under 1 and 2.  Any call forgets the views seen so far. */
int rfx_renderer_set_prim_masks(rfx_renderer *r, int mode);
/* The masks of a still view narrowed to its primary hits, which depend on the view alone (no pixel changes): 1 (default)
 * = where those hits are known ahead (no jitter, sampleNum <= 8) the closest-hit mask is the set of the tile's winners
 * and each shadow mask drops the one object that all the tile's lit hits lie on (its answer is discarded anyway); 0 = the
 * conservative bundle culls alone.  Any call drops the masks held, so the next frame of the view builds them again. */
int rfx_renderer_set_prim_exact(rfx_renderer *r, int on);
/* Copy the masks the renderer holds for the current view to `host`, after synchronising the stream they were built on:
 * *words = their length in 64-bit words (5 per 8x8 wave tile of a small scene: the closest-hit mask, then one shadow
 * mask per light up to 4, 0 past the scene's lights and where a frame takes no shadow masks; bit (i & 1) * 16 + (i >> 1)
 * is sphere i, bit 32 + i triangle i), 0 when no view's masks are held.  `host` may be NULL to ask for the length alone; a capacity below it is RFX_ERR_ARG. */
int rfx_renderer_get_prim_masks(rfx_renderer *r, uint64_t *host, uint64_t capacity, uint64_t *words);
/* The reference's two LCG streams (trace_math.h:34-39): Vector3.cpp's (randomInsideSphere) and
 * Render.cpp's (additive jitter).  Both persist across frames exactly as the reference's would. */
int rfx_renderer_set_rng(rfx_renderer *r, uint32_t sphere_seed, uint32_t jitter_seed);
int rfx_renderer_get_rng(rfx_renderer *r, uint32_t *sphere_seed, uint32_t *jitter_seed); /* synchronises */

typedef struct {
  float eye[3];        /* Render::renderCameraEye  (Render.cpp:128) */
  float view[9];       /* Render::renderCameraView (Render.cpp:127), row-major */
  float fov;           /* Camera::fov -> rz = W/2/tanf(fov/2) (Render.cpp:148) */
  uint32_t width, height;
  int32_t reflect_num;      /* renderBegin reflectNum (> 0) */
  int32_t sample_num;       /* renderBegin sampleNum: >0 SSAA n x n, <0 |n| block preview, 0 invalid */
  int32_t additive;         /* renderBegin additive */
  int32_t additive_counter; /* Render::additiveCounter after renderBegin (Render.cpp:130-133) */
  uint32_t row_block;       /* strip partition: rows are dealt in blocks of row_block ...   */
  uint32_t rank, nranks;    /* ... block b belongs to rank b % nranks (nranks == 1: whole frame) */
  uint64_t pixel_begin;     /* raster span [pixel_begin, pixel_end) of this call: the Render::renderNext */
  uint64_t pixel_end;       /* cursor span (Render.cpp:136-215); 0, 0 = the whole frame.  nranks == 1, or a band */
  /* Band partition: nranks > 1 with row_block == 0 -- this rank traces the whole rows [pixel_begin, pixel_end) / W of
   * the W x H frame into whole-frame buffers (d_rgb W*H*3, d_argb W*H; only the band's rows are written), with the
   * frame's random stream sliced nranks ways as for strips (rfx_frame_rng_count / rfx_render_frame_counted).  Rank 0
   * can then receive each band straight into its rows of the frame (reflaxman_amd/dist.py BandFrame). */
  uint64_t span_begin;      /* band partition only: the random stream covers the whole rows [span_begin, span_end) / W */
  uint64_t span_end;        /* of the frame (0, 0 = the whole frame) and the band lies within them -- a frame of 2^32 */
                            /* traces or more is rendered as consecutive row spans (rfx_group_render_frame) */
} rfx_frame;

/* rows of `frame` that `rank` owns under the block-cyclic strip partition */
uint32_t rfx_strip_rows(uint32_t height, uint32_t row_block, uint32_t rank, uint32_t nranks);
/* global row of compact strip row `r` */
uint32_t rfx_strip_row_to_y(uint32_t r, uint32_t row_block, uint32_t rank, uint32_t nranks);

/*
 * One Render::renderBegin + renderNext(W*H) pass on the device (Render.cpp:116-215 + Scene::trace,
 * Scene.cpp:73-236): RNG pre-pass, trace kernel, ARGB epilogue, all stream-ordered, no host sync.
 *   d_rgb  : device float RGB, strip_rows x W x 3 (read-modify-write when additive_counter > 1)
 *   d_argb : device uint32, strip_rows x W, Color::argb of the stored value (copyImage), or NULL
 *   d_counters : device uint64[RFX_NCOUNTERS] accumulated event counters (stats kernel), or NULL
 * Any sample count (Pulse's menu reaches 7680x4320 at 256x256 samples, 2.2e12 traces): a span of more traces than the
 * launch limit (rfx_renderer_set_launch_traces) is rendered as consecutive pixel spans (whole rows where a row fits),
 * each its own pre-pass and trace launch, alternating between two streams so one span's tail overlaps the next span's
 * start; the random streams run on from span to span exactly as the reference's cursor does (Render.cpp:136-215).
 */
#define RFX_NCOUNTERS 40
int rfx_render_frame(rfx_renderer *r, const rfx_frame *frame, float *d_rgb, uint32_t *d_argb,
                     uint64_t *d_counters, void *stream);
/* The most traces one rfx_render_frame launch takes (default 2^30: 4 GB of randDir state per buffer, two buffers);
 * 0 = the default.  Splitting changes no pixel (tests/test_gpu_parity.py forces small limits). */
int rfx_renderer_set_launch_traces(rfx_renderer *r, uint64_t max_traces);
/* The RNG pre-pass of one-device unsplit rfx_render_frame launches (no pixel changes): 1 (default) = the cycle table.
 * Whether a triple of draws is accepted depends on the LCG state alone and a triple is an affine map of full period
 * 2^32, so every frame's stream is a run of one cyclic sequence of 2^32 triples; the renderer counts the whole cycle's
 * accepted triples once (on its first such frame: a few ms of GPU time, 8 MB), keeps the stream state's place in the
 * cycle on the device, and every later pre-pass is one launch that looks its offsets up.  0 = the count and emit kernels
 * of every frame, as the multi-GPU, band, strip and split-span paths always take. */
int rfx_renderer_set_rng_prepass(rfx_renderer *r, int mode);
/* Which pre-pass the last launch ran: 0 = the count / emit kernels, 1 = the cycle table, 2 = the one-pass kernel of
 * small launches (taken only where the table is off). */
int rfx_renderer_prepass_form(const rfx_renderer *r);
/* The place of an LCG state in that cycle: the k with (three draws)^k applied to state 0 giving `state` (host only). */
uint32_t rfx_rng_triple_index(uint32_t state);
/* blocks of the cycle table (4096 triples each) */
uint32_t rfx_rng_seq_blocks(void);

/*
 * Multi-GPU form of the RNG pre-pass, around ONE exchange step.  The trace-ordered
 * random stream is cut into nslices equal slices of LCG blocks; rank r counts the accepted triples of
 * slice r only (rfx_frame_rng_count), the per-block counts are all-gathered (RCCL: nslices *
 * blocks_per_slice uint32 on the device), and rfx_render_frame_counted scans them and emits only the
 * randDirs of this rank's strips before tracing them.  Every rank also carries the stream state past
 * the frame's last trace, so the next frame starts where the reference's would.  rfx_render_frame is
 * the same with nslices = 1 and every block counted locally.
 */
int rfx_frame_rng_blocks(rfx_renderer *r, const rfx_frame *frame, uint32_t nslices, uint64_t *blocks_per_slice);
int rfx_frame_rng_count(rfx_renderer *r, const rfx_frame *frame, uint32_t slice, uint32_t nslices,
                        uint32_t *d_blk_counts, void *stream);
int rfx_render_frame_counted(rfx_renderer *r, const rfx_frame *frame, uint32_t nslices, const uint32_t *d_blk_counts,
                             float *d_rgb, uint32_t *d_argb, uint64_t *d_counters, void *stream);
/* The same, recording the caller's hipEvent_t `emitted_event` on `stream` once the randDirs are emitted, before the
 * trace: from then on the next frame's stream state is on the device, so the next frame's rfx_frame_rng_count and
 * all-gather may run on another stream while this frame traces (reflaxman_amd/dist.py count-ahead).  The renderer's
 * RNG stream must not advance in between (no other render call on this renderer). */
int rfx_render_frame_counted_ev(rfx_renderer *r, const rfx_frame *frame, uint32_t nslices,
                                const uint32_t *d_blk_counts, float *d_rgb, uint32_t *d_argb, uint64_t *d_counters,
                                void *stream, void *emitted_event);

/* Emit-ahead (multi-GPU, reflaxman_amd/dist.py): the counted frame split in two, so the next frame's emit can run on
 * another stream while this frame traces.  rfx_frame_rng_emit scans the all-gathered counts and writes the frame's
 * randDirs into the renderer's second randDir buffer (the one the last enqueued trace does not read; order it after
 * the trace before that), records emitted_event, and moves the stream state past the frame;
 * rfx_render_frame_emitted traces that frame.  One emitted frame at a time; rfx_frame_rng_discard forgets it and
 * restores the stream state.  Other render calls fail while a frame is pending. */
int rfx_frame_rng_emit(rfx_renderer *r, const rfx_frame *frame, uint32_t nslices, const uint32_t *d_blk_counts,
                       void *stream, void *emitted_event);
int rfx_render_frame_emitted(rfx_renderer *r, const rfx_frame *frame, float *d_rgb, uint32_t *d_argb,
                             uint64_t *d_counters, void *stream);
int rfx_frame_rng_discard(rfx_renderer *r);
/* The sphere-stream state the next traced frame starts from: the emitted frame's when one is pending (returns 1),
 * else the current state (returns 0).  Synchronises with the renderer's stream; the emit must have completed (order
 * the renderer's stream after the emit's, or synchronise the device).  A single-GPU renderer seeded with it renders
 * that frame (bench.py's steady-state parity check). */
int rfx_frame_rng_pending(rfx_renderer *r, uint32_t *frame_start);

/*
 * Ray batches: Scene::trace(origin, ray, reflNumber) (Scene.h:39, Scene.cpp:73-236) on rays the caller chose -- a
 * panorama or fisheye camera, a lens model, a probe, a pick, a set of pixels traced again.  The call is exactly n
 * consecutive calls Scene::trace(origin_i, ray_i, reflect_num) in index order, stream-ordered with no host sync:
 *   d_rays : device, 6 floats per ray: origin x y z, then direction x y z (rfx_kat_objects' record).  The direction is
 *            used as given, not normalised, as Scene::trace uses it.
 *   d_rgb  : device, 3 floats per ray: the returned colour (overwritten, nothing accumulates)
 *   d_argb : device uint32 per ray, Color::argb of that colour, or NULL
 *   d_counters : device uint64[RFX_NCOUNTERS] accumulated event counters (stats kernel), or NULL
 * Random streams: ray i takes the i-th randomInsideSphere draw of the sphere stream counted from the renderer's current
 * state, and the stream then stands n accepted triples later; the jitter stream is not touched.  A following
 * rfx_render_frame, or another batch, continues where the reference would after those n calls.  The pre-pass is the
 * one an unsplit one-device rfx_render_frame launch of n traces takes (rfx_renderer_set_rng_prepass,
 * rfx_renderer_prepass_form).  A batch is no rfx_render_frame: rfx_frame_rng_rewind after it is RFX_ERR_STATE.
 * raster_width changes the schedule only, never a value: 0 = a wave takes 64 consecutive rays; W > 0 = the batch is a
 * row-major W x ceil(n / W) raster (its last row may be partial) and a wave takes an 8x8 tile of it, the frame
 * kernel's coherence, for rays that come from a camera model.  Either way ray i takes draw i and writes output i.
 * A batch of more rays than the launch limit (rfx_renderer_set_launch_traces, rounded down to whole waves or whole
 * tile rows of 8 W rays, and at least one) runs as consecutive launches on the one stream, the random stream running on.
 * Errors: n == 0, NULL d_rays or d_rgb, reflect_num <= 0: RFX_ERR_ARG; no scene uploaded, or an emitted frame pending
 * (rfx_frame_rng_emit): RFX_ERR_STATE.
 */
int rfx_trace_rays(rfx_renderer *r, const float *d_rays, uint64_t n, int32_t reflect_num, uint32_t raster_width,
                   float *d_rgb, uint32_t *d_argb, uint64_t *d_counters, void *stream);
/* The same on host arrays: copies in and out on the renderer's stream and synchronises; counters (or NULL) are added to. */
int rfx_trace_rays_host(rfx_renderer *r, const float *rays, uint64_t n, int32_t reflect_num, uint32_t raster_width,
                        float *rgb, uint32_t *argb, uint64_t *counters);
/* Undo the random-stream advance of the last call, which must be an rfx_render_frame (else RFX_ERR_STATE): both
 * streams return to that frame's start, its pixels stay as written.  The drop-in Render (dropin/Render.h) renders a
 * whole frame at the first renderNext after renderBegin; when the caller leaves that frame early (renderBegin or
 * setImageSize mid-frame, Pulse.cpp:110-124) it rewinds and renders exactly the span the reference's cursor covered,
 * so the streams end where the reference's do (Render.cpp:136-215, trace_math.h:34-39). */
int rfx_frame_rng_rewind(rfx_renderer *r);

/*
 * Hit queries: the two questions Scene::trace asks of its objects on every segment, on rays the caller chose -- which
 * object a ray meets and where (a pick, a depth or object-id image, a probe), and whether anything stands in a ray's
 * way (a visibility test).  Rays are rfx_trace_rays' records, 6 floats each: origin, then the direction, used as given.
 * Both calls are stream-ordered with no host sync, and raster_width means what it means for rfx_trace_rays: which rays
 * share a wave (0 = 64 consecutive rays, W > 0 = an 8x8 tile of the row-major W-wide raster), never a value.  A batch
 * above rfx_renderer_set_launch_traces runs as consecutive launches on the one stream, rounded as a ray batch's.
 * These entries were added under RFX_ABI_VERSION 5 without raising it (nothing that existed changed): a caller that
 * may meet an older version-5 library detects them by symbol (dlsym).
 *
 * rfx_query_hits: one pass of the closest-hit loop (Scene.cpp:82-107) per ray.  Every object's trace() is tested, and
 * the winner is the reference's: strict `<` on curDist in insertion order, so among equal distances the lowest object
 * index wins.  Each plane of rfx_hit_planes is a device array or NULL (not wanted; at least one is wanted).  Every
 * word of every requested plane is written -- on a miss object = -1, distance = FLT_MAX and the 3-float planes 0 --
 * and nothing else is.  Planes need 4-B alignment only.
 *
 * rfx_query_occluded: d_occluded[i] = 1 if any object other than d_skip[i] returns true from
 * trace(origin, ray, NULL, ...) (Scene.cpp:133-143), else 0.  The ray is unbounded, as the reference's shadow ray is:
 * an object beyond the light still occludes it.  A segment test is rfx_query_occluded_span with d_hi ("Ray intervals"
 * below).  d_skip NULL skips nothing, and so does a value outside [0, objects).
 *
 * Neither call touches the random streams (there is no pre-pass: rfx_renderer_get_rng reads the same before and
 * after), the per-view masks, the tile costs, the regroup queue, the timing sums, or what rfx_frame_rng_rewind may
 * undo: a rewind after "frame, then query" still succeeds.
 * Errors: NULL renderer, rays, out or d_occluded, all planes NULL, n == 0: RFX_ERR_ARG; no scene uploaded: RFX_ERR_STATE.
 */
typedef struct {          /* one plane per output, each may be NULL (not wanted); at least one non-NULL */
  int32_t *object;        /* n    : object index as the add call returned it (insertion order); -1 = no hit */
  float   *distance;      /* n    : curDist of the winner (Scene.cpp:98-100); FLT_MAX on a miss (Scene.cpp:82) */
  float   *point;         /* 3 n  : drop */
  float   *normal;        /* 3 n  : norm as the object returns it (not normalised) */
  float   *reflected;     /* 3 n  : reflect(ray * t, norm) */
  float   *colour;        /* 3 n  : dropMaterial.color: the material's, or a textured triangle's texel */
} rfx_hit_planes;
int rfx_query_hits(rfx_renderer *r, const float *d_rays, uint64_t n, uint32_t raster_width,
                   const rfx_hit_planes *out, void *stream);
int rfx_query_occluded(rfx_renderer *r, const float *d_rays, const int32_t *d_skip, uint64_t n,
                       uint32_t raster_width, uint8_t *d_occluded, void *stream);
/* The same on host arrays: they copy in and out on the renderer's stream and synchronise. */
int rfx_query_hits_host(rfx_renderer *r, const float *rays, uint64_t n, uint32_t raster_width,
                        const rfx_hit_planes *out /* host pointers */);
int rfx_query_occluded_host(rfx_renderer *r, const float *rays, const int32_t *skip, uint64_t n,
                            uint32_t raster_width, uint8_t *occluded);

/*
 * Ray intervals: the two hit queries on a per-ray interval of distances -- "is B visible from A" (a shadow ray to a
 * finite light, a portal, a line of sight) and "what lies behind the first hit" (picking through glass, depth peeling,
 * every hit along a probe).  Added under RFX_ABI_VERSION 5 without raising it, as the hit queries were: detect by
 * symbol (dlsym).  Nothing that existed changes.
 *
 * Candidates: for ray i, object j (the index its add call returned) is a candidate iff the reference's
 * trace(origin, ray, &drop, ..., &curDist, ...) returns true; its distance dist is that call's curDist, a float.  This
 * is rfx_query_hits' notion.  rfx_query_occluded_span is defined by the same out-parameter form, not by
 * trace(origin, ray, NULL, ...).
 *
 * The span: three optional per-ray device arrays, indexed by the ray index i in every form (the ordered forms read
 * d_lo[d_order[s]]).  A candidate is eligible iff
 *   (d_hi == NULL || dist <= hi[i])   -- the upper end is inclusive -- and
 *   (d_lo == NULL || dist > lo[i] || (dist == lo[i] && j > after[i]))
 * i.e. (dist, j) comes after (lo, after) in the reference's own order, distance first, then insertion index.
 * after = -1 (and d_after NULL) makes the lower end inclusive, after = INT32_MAX exclusive, after = the previous winner
 * steps through objects at exactly one distance one at a time.  d_after is read only where d_lo is given.  The
 * comparisons are plain float comparisons on the rounded dist: a NaN end makes nothing eligible, and so do lo = +inf
 * and hi < 0; lo < 0 bounds nothing, hi >= FLT_MAX bounds nothing (curDist still starts at FLT_MAX, Scene.cpp:82),
 * and -0.0 equals 0.0.  span NULL, or all its arrays NULL, means no ends.
 *
 * rfx_query_hits_span: the winner is the eligible candidate with the least dist, among equal dist the lowest index --
 * rfx_query_hits' rule on the eligible set.  The planes are written exactly as rfx_query_hits writes them, the miss
 * values where no candidate is eligible.  Without ends every word is rfx_query_hits'.
 * Layers: calling again with (lo, after) = (the previous distance, the previous object) enumerates a ray's candidates
 * in ascending (dist, index), each exactly once; that sequence defines the ray's layers.
 *
 * rfx_query_occluded_span: d_occluded[i] = 1 iff an eligible candidate other than d_skip[i] exists; it takes d_lo and
 * d_hi only (d_after is not read: the lower end is inclusive).  Without ends it equals rfx_query_occluded on every
 * scene whose objects answer both forms of trace() alike.  A segment test "is b visible from a" is the ray (a, b - a)
 * with hi = |b - a|: the far end is inclusive, and one float below excludes an object at b itself.
 *
 * The ordered and host forms are the hit queries'; launch splitting above rfx_renderer_set_launch_traces advances the
 * span arrays with the other per-ray arrays (ordered forms: slot ranges over whole arrays).  Errors and state rules are
 * those of rfx_query_hits and rfx_query_occluded, and like them the calls touch nothing but the uploaded scene: no
 * random stream, masks, tile costs or rewind state.
 */
typedef struct {
  const float   *d_lo;     /* n, or NULL: no lower end */
  const int32_t *d_after;  /* n, or NULL: -1 for every ray; read only where d_lo is given */
  const float   *d_hi;     /* n, or NULL: no upper end */
} rfx_ray_span;
int rfx_query_hits_span(rfx_renderer *r, const float *d_rays, const rfx_ray_span *span /* or NULL */, uint64_t n,
                        uint32_t raster_width, const rfx_hit_planes *out, void *stream);
int rfx_query_occluded_span(rfx_renderer *r, const float *d_rays, const int32_t *d_skip,
                            const rfx_ray_span *span /* or NULL */, uint64_t n, uint32_t raster_width,
                            uint8_t *d_occluded, void *stream);
int rfx_query_hits_span_ordered(rfx_renderer *r, const float *d_rays, const rfx_ray_span *span /* or NULL */,
                                const uint32_t *d_order, uint64_t n, const rfx_hit_planes *out, void *stream);
int rfx_query_occluded_span_ordered(rfx_renderer *r, const float *d_rays, const int32_t *d_skip,
                                    const rfx_ray_span *span /* or NULL */, const uint32_t *d_order, uint64_t n,
                                    uint8_t *d_occluded, void *stream);
/* The same on host arrays (the span's included): they copy in and out on the renderer's stream and synchronise. */
int rfx_query_hits_span_host(rfx_renderer *r, const float *rays, const rfx_ray_span *span /* host pointers, or NULL */,
                             uint64_t n, uint32_t raster_width, const rfx_hit_planes *out /* host pointers */);
int rfx_query_occluded_span_host(rfx_renderer *r, const float *rays, const int32_t *skip,
                                 const rfx_ray_span *span /* host pointers, or NULL */, uint64_t n,
                                 uint32_t raster_width, uint8_t *occluded);

/*
 * Coherent order: rfx_trace_rays and the hit queries run one lane per ray, and a wave is fast only when its 64 rays are
 * alike.  Rays from bounces, probes or a sampler are not.  rfx_rays_order sorts a batch's indices by a 32-bit key of
 * origin cell and direction, and the ordered calls below run wave w on the rays d_order[64 w .. 64 w + 63] -- the
 * values, the outputs' places and the random draws stay those of the unordered calls.  Added under RFX_ABI_VERSION 5
 * without raising it, as the hit queries were: detect by symbol (dlsym).
 *
 * The key, key = cellMorton << (2 DB) | dirMorton with CB = RFX_ORDER_CELL_BITS and DB = RFX_ORDER_DIR_BITS, origin
 * major (rays from one place lie together, then go by direction).  Every operation below is an IEEE float32 one with no
 * contraction, so a float32 restatement gives the same bits (tests/order_helpers.py):
 *   box    : per axis, lo = the minimum over the spheres' centre - radius and the triangles' vertices, hi = the maximum
 *            over centre + radius and the vertices (float32, insertion order, a NaN never taken); scale = 2^CB / (hi - lo)
 *            where hi > lo and both are finite, else scale = 0 (and a lo that is not finite is given as 0).  Planes do
 *            not count; a scene with neither spheres nor triangles has scale 0.  Computed by rfx_renderer_set_scene.
 *   cell   : c_a = (uint32) fminf(fmaxf((o_a - lo_a) * scale_a, 0), 2^CB - 1) -- a NaN takes the 0 --; cellMorton has
 *            bit b of c_x at 3 b, of c_y at 3 b + 1, of c_z at 3 b + 2.
 *   dir    : the octahedral map.  a = (|dx| + |dy|) + |dz|, px = dx / a, py = dy / a; if dz < 0:
 *            qx = (1 - |py|) * (px < 0 ? -1 : 1), qy = (1 - |px|) * (py < 0 ? -1 : 1), else (qx, qy) = (px, py);
 *            u = (uint32) fminf(fmaxf((qx + 1) * 2^(DB - 1), 0), 2^DB - 1), v likewise from qy; dirMorton has bit b of
 *            u at 2 b, of v at 2 b + 1.  Zero, infinite and NaN directions fall out of these expressions as they stand
 *            (to cell 0 or a clamped cell): that is part of the definition.
 */
#define RFX_ORDER_CELL_BITS 4
#define RFX_ORDER_DIR_BITS 10
/* rays one workgroup of the sort takes per digit pass (the sizes at which the sort's paths change) */
#define RFX_ORDER_TILE 4096
/* The key's box of the uploaded scene; RFX_ERR_STATE without one. */
int rfx_renderer_order_box(const rfx_renderer *r, float lo[3], float scale[3]);
/*
 * d_order[0 .. n) becomes the permutation of [0, n) with nondecreasing keys, equal keys in index order (a stable sort:
 * the result is a function of the rays alone); d_keys[i], where given, is ray i's key (ray order, not sorted order).
 * Stream-ordered, no host sync.  A stable LSD radix sort of (key, index) pairs, 8 bits a pass: per-workgroup digit
 * histograms, one scan over (digit, workgroup), a stable scatter; no kernel waits on another workgroup.  The scratch
 * (ping-pong keys and indices, histograms) is the renderer's own and grows on demand: two order calls of one renderer
 * on streams that are not ordered with each other are the caller's error.  The call touches nothing a frame, a batch
 * or a query keeps: no random stream, no masks, no tile costs, nothing rfx_frame_rng_rewind may undo.
 * Errors: n == 0, n >= 2^31, NULL renderer, rays or order: RFX_ERR_ARG; no scene uploaded: RFX_ERR_STATE.
 */
int rfx_rays_order(rfx_renderer *r, const float *d_rays, uint64_t n, uint32_t *d_order, uint32_t *d_keys /* or NULL */,
                   void *stream);
/* The same on host arrays: copies in and out on the renderer's stream and synchronises. */
int rfx_rays_order_host(rfx_renderer *r, const float *rays, uint64_t n, uint32_t *order, uint32_t *keys /* or NULL */);
/*
 * The ordered calls: rfx_trace_rays, rfx_query_hits and rfx_query_occluded with the schedule given by d_order (n
 * uint32 on the device) instead of raster_width.  Wave w takes slots 64 w .. 64 w + 63, and slot s works on ray
 * i = d_order[s]; everything per ray is indexed by i -- the record, d_skip[i], every output, and, for the trace, draw i
 * of the sphere stream.  For a permutation the results and the stream's end state are therefore word for word those of
 * the unordered call: d_order only moves work between waves.  It need not come from rfx_rays_order.  It must be a
 * permutation of [0, n); that is not checked, but it is made safe: a slot whose index is >= n is a dead lane that reads
 * and writes nothing (an index named twice is traced twice and written twice with the same value; an index never named
 * leaves its outputs unwritten).  Outputs leave per lane (12-B and 4-B stores); there is no counters form.
 * The hit queries above the launch limit (rfx_renderer_set_launch_traces) run as consecutive slot ranges over the whole
 * arrays.  The ordered trace above it is RFX_ERR_ARG, returned before any stream advances: the renderer's randDir
 * state covers that many rays and an ordered launch may name any ray, so a caller splits such a batch and orders each
 * part.  The other errors are the unordered calls' (NULL d_order, or n >= 2^32: RFX_ERR_ARG), RFX_ERR_STATE with an
 * emitted frame pending included.
 */
int rfx_trace_rays_ordered(rfx_renderer *r, const float *d_rays, const uint32_t *d_order, uint64_t n,
                           int32_t reflect_num, float *d_rgb, uint32_t *d_argb, void *stream);
int rfx_query_hits_ordered(rfx_renderer *r, const float *d_rays, const uint32_t *d_order, uint64_t n,
                           const rfx_hit_planes *out, void *stream);
int rfx_query_occluded_ordered(rfx_renderer *r, const float *d_rays, const int32_t *d_skip, const uint32_t *d_order,
                               uint64_t n, uint8_t *d_occluded, void *stream);

/*
 * Paths: Scene::trace (Scene.cpp:73-236) as a state per ray that the caller holds on the device and steps by segment.
 * rfx_trace_rays fixes the depth at the call and keeps everything between the first ray and the final colour to
 * itself; here the variables Scene::trace carries from one loop iteration to the next lie in planes of the caller's,
 * and a step runs the loop's body on them -- bit for bit the operations of the one-shot call, so after k segments a
 * path's colour is Scene::trace(origin, ray, k).  A caller renders to one depth and continues to another without
 * tracing again, drops ended paths and regroups the live ones between segments (rfx_paths_order), brings its own
 * randDir per path, or edits rays and mulColor between segments.  Added under RFX_ABI_VERSION 5 without raising it:
 * detect by symbol (dlsym).  There are no host forms (rfx_device_alloc and rfx_memcpy_* serve C callers) and no
 * counters form.
 */
typedef struct {            /* device planes of n paths; every plane indexed by the path index i */
  float       *d_rays;      /* 6 n : the next segment's origin and ray -- rfx_trace_rays' record, used as given */
  float       *d_mul;       /* 3 n : mulColor   (Scene.cpp:76) */
  float       *d_colour;    /* 3 n : pixelColor (Scene.cpp:77): after k segments it is Scene::trace(.., k) */
  float       *d_rand;      /* 3 n : randDir    (Scene.cpp:75); only rfx_paths_begin writes it */
  int32_t     *d_state;     /* n   : s >= 0: live, s segments run; s < 0: ended, ~s segments run (>= 1) */
  uint32_t    *d_argb;      /* n, or NULL : Color::argb of d_colour, written wherever d_colour is */
} rfx_paths;
/*
 * The start state of the n paths whose d_rays the caller has filled: mul = 1, colour = 0, state = 0, argb where given.
 * draw != 0: d_rand[i] becomes the i-th randomInsideSphere draw from the renderer's current sphere-stream state -- the
 * three floats the batch kernels take for ray i -- and the stream then stands n accepted triples on, exactly as after
 * rfx_trace_rays of n rays (the same pre-pass, the same splitting above the launch limit).  draw == 0: d_rand and both
 * streams are left alone (the caller's own sampler; zero vectors give the noise-free image).
 * Errors: those of rfx_trace_rays (NULL renderer or p, a NULL required plane, n == 0: RFX_ERR_ARG; no scene:
 * RFX_ERR_STATE); an emitted frame pending is RFX_ERR_STATE only when draw != 0.
 */
int rfx_paths_begin(rfx_renderer *r, const rfx_paths *p, uint64_t n, int draw, void *stream);
/*
 * One step.  Wave w takes slots 64 w .. 64 w + 63, and slot s works on path i = d_index ? d_index[s] : s; a slot with
 * i >= n is a dead lane that reads and writes nothing (the ordered calls' rule).  For a named path with
 * st = d_state[i]:
 *   st < 0 or st >= upto : no word of the path is written.
 *   otherwise            : the body of Scene::trace's loop (Scene.cpp:80-234) runs on the path's variables, refl = st,
 *                          until refl == upto or the loop is left by one of its breaks (the sky, 228-233; the mulColor
 *                          cut-off, 220-222).  d_colour[i] (and d_argb[i]) are written either way.  Left by a break:
 *                          d_state[i] = ~(segments run), and the path's d_rays and d_mul words are unspecified from then
 *                          on (the library never reads them again).  Else d_state[i] = upto, d_rays[i] = the (origin,
 *                          ray) of Scene.cpp:225-226 and d_mul[i] = mulColor.
 * d_live (capacity `slots`, must not alias d_index) receives the index of every named path that is live (state >= 0)
 * after the call, whether or not it ran, and d_live_count[0] is set by the call to their number (d_live NULL: the count
 * alone).  Their order in d_live is a schedule, not a value: it may differ from run to run.  An index named twice in
 * one call is the caller's error: that path's words are unspecified, and nothing out of bounds is touched.  `slots`
 * above the launch limit run as consecutive slot ranges over the whole arrays, the count running on.  Stream-ordered,
 * no host sync.  The call touches no random stream, mask, tile cost, timing sum or rewind state (the queries' rule).
 * Errors: NULL renderer or p, any of the five required planes NULL, slots == 0, n == 0 or n >= 2^32, upto < 1 or
 * upto == INT32_MAX, d_live without d_live_count: RFX_ERR_ARG; no scene uploaded: RFX_ERR_STATE.
 */
int rfx_paths_step(rfx_renderer *r, const rfx_paths *p, uint64_t n, const uint32_t *d_index /* or NULL */,
                   uint64_t slots, int32_t upto, uint32_t *d_live /* or NULL */, uint32_t *d_live_count /* or NULL */,
                   void *stream);
/*
 * d_order[0 .. slots) becomes the entries of d_index (NULL: 0 .. slots - 1), stably sorted by the "Coherent order" key
 * of each path's current d_rays record; an entry >= n takes key 0xFFFFFFFF, so it sorts last and is kept.  With
 * d_index NULL and slots == n the result is rfx_rays_order(p->d_rays, n) word for word.  d_order may be d_index.  The
 * renderer's sort scratch and rfx_rays_order's rules for it apply; like it, the call touches nothing else.
 * Errors: NULL renderer, p, d_rays or d_order, n == 0 or n >= 2^32, slots == 0 or slots >= 2^31: RFX_ERR_ARG; no scene:
 * RFX_ERR_STATE.
 */
int rfx_paths_order(rfx_renderer *r, const rfx_paths *p, uint64_t n, const uint32_t *d_index /* or NULL */,
                    uint64_t slots, uint32_t *d_order, void *stream);

/* ---------------------------------------------------------------- Moving meshes
 * A deforming mesh keeps its topology: its triangles' records and boxes change, its tree does not.  These calls give
 * triangles of the uploaded scene new vertices on the device, stream-ordered, without the host rebuild and re-upload of
 * rfx_renderer_set_scene.  (Added under RFX_ABI_VERSION 5; detect them by symbol.)
 *
 * Contract: after the call every launch on the renderer returns, word for word, what a renderer returns whose
 * rfx_renderer_set_scene got the same scene built at the new vertices -- frames of every mode, rfx_trace_rays, the hit
 * queries and spans, the ordered forms, rfx_paths_step -- settings, random streams and inputs being the same.  The update
 * touches neither random stream (rfx_renderer_get_rng reads the same before and after), nor the tile costs, the timing
 * sums, the regroup queue or the rewind state; it drops the per-view masks, as rfx_renderer_set_scene does.  The
 * coherent order's key box (rfx_renderer_order_box) stays as rfx_renderer_set_scene computed it: it is a schedule
 * input, and no value of an ordered call depends on it.
 *
 * What follows a vertex (DESIGN.md "Moving meshes"): the triangle's v0 and axTrans (Triangle.cpp:11-21, the
 * reference's float operations in its operand order), its normal, its bounding sphere, its copy in the triangle BVH's
 * leaves, and the BVH's boxes -- every node refitted on every update from the current vertices alone, by the builder's
 * own widening formula, so repeated updates do not drift.  The tree's topology, the residual list and the margin
 * reference point stay as built: only speed follows a mesh that has moved far from where its tree was cut, and
 * rfx_renderer_set_scene restores it.  A triangle of the tree whose new basis is ill-conditioned (cond >= 300, singular,
 * a non-finite vertex) may report hits far from its vertices: its leaf and every box above it become all of space (NaN
 * bounds, which the kernels' box test keeps for every ray; rfx_renderer_tri_bvh_nodes reports them as 0x7FC00000), so
 * every ray still tests it.  A residual triangle that becomes well-conditioned stays residual.
 *
 * Works on non-small scenes (more than 32 spheres or more than 32 triangles), with or without a triangle BVH.  A small
 * scene is RFX_ERR_STATE: its 64 lane records, footprints and mate groups are uploaded again by
 * rfx_renderer_set_scene in microseconds.  Materials, textures, uv and object indices stay; spheres move by "Moving
 * spheres" below, lights do not move.
 *
 * Triangles [first, first + count) take new vertices; `first` counts triangles in insertion order (0 = the scene's
 * first triangle, rfx_scene_tri_mates' numbering; rfx_scene_object_triangle maps an object index to it).
 *   d_indices == NULL : d_positions holds 9 floats per triangle, (v1, v2, v3) as rfx_scene_add_triangle takes them;
 *                       n_positions == 3 * count.
 *   d_indices != NULL : 3 uint32 per triangle into d_positions (n_positions x 3 floats), rfx_scene_add_mesh's form.  A
 *                       triangle naming an index >= n_positions keeps its old vertices (a dead lane: it cannot be an
 *                       error without a sync).
 * Stream-ordered (NULL = the renderer's stream), no host sync.
 * Errors: NULL renderer or positions, count == 0, first + count > the scene's triangles, d_indices == NULL with
 * n_positions != 3 * count: RFX_ERR_ARG; no scene uploaded, or a small scene: RFX_ERR_STATE. */
int rfx_renderer_update_triangles(rfx_renderer *r, uint32_t first, uint32_t count, const float *d_positions,
                                  uint32_t n_positions, const uint32_t *d_indices, void *stream);
/* The same on host arrays: copies them in on the renderer's stream and synchronises. */
int rfx_renderer_update_triangles_host(rfx_renderer *r, uint32_t first, uint32_t count, const float *positions,
                                       uint32_t n_positions, const uint32_t *indices);
/* The host scene kept in step: Triangle.cpp:11-21 run again in place on triangles [first, first + count) (v0, v1, v2,
 * norm, axTrans and the builder's condition number) from 9 floats each.  Material, texture, uv and object index stay.
 * Read by the next rfx_renderer_set_scene. */
int rfx_scene_set_triangle_vertices(rfx_scene *scene, uint32_t first, uint32_t count, const float *vertices9);
/* The triangle index (insertion order among triangles) of an object, or RFX_ERR_ARG for a non-triangle. */
int rfx_scene_object_triangle(const rfx_scene *scene, int object_index);
/* The words that follow a triangle's vertices, RFX_TRI_RECORD_WORDS uint32 per triangle of [first, first + count), from
 * the host scene and -- a device read-back, synchronises; not for a small scene -- from the uploaded one:
 *   [0, 12)  the geometry record: v0 x y z, axTrans row 3, then (a11, a21), (a12, a22), (a13, a23);
 *   [12, 15) the normal;   [15, 19) the bounding sphere: centre x y z, radius (+inf: never culled);
 *   [19, 28) the vertices as given;   [28] 1 = well-conditioned, 0 = not;
 *   [29, 41) the triangle BVH's copy of the geometry record (a triangle outside the tree, and the host scene: words
 *            [0, 12) again).
 * Every NaN is reported as 0x7FC00000 (its sign and payload carry nothing and differ between processors), so equal
 * scenes give equal words. */
#define RFX_TRI_RECORD_WORDS 41
int rfx_scene_tri_records(const rfx_scene *scene, uint32_t first, uint32_t count, uint32_t *out);
int rfx_renderer_tri_records(rfx_renderer *r, uint32_t first, uint32_t count, uint32_t *out);
/* The tree rfx_scene_tri_bvh_dump reports for `built` -- its topology, leaf membership and residual list -- refitted on
 * the host to the vertices given (9 floats for every triangle of the scene), as the device update refits it: boxes --
 * nodes x 12 floats in the dump's layout, mt -- nodes x 2 margin terms; either may be NULL.  widen = 0: the boxes as
 * built (at the scene's own vertices: the dump's, bit for bit); widen = 1: the device copy, grown by the cull margin
 * from the tree's reference point.  Returns 1 with a tree, 0 without. */
int rfx_scene_tri_bvh_refit(const rfx_scene *built, const float *vertices9_all, int widen, float *boxes, float *mt);
/* The uploaded triangle BVH's nodes read back (synchronises): 16 words per node -- 12 box floats in the dump's layout,
 * the 2 children as int32, the 2 margin terms.  Returns the node count (0: no tree); out may be NULL to ask for it. */
int rfx_renderer_tri_bvh_nodes(rfx_renderer *r, float *out);
/* The uploaded triangle BVH's leaves read back (host only; synchronises the renderer's stream), as the last
 * rfx_renderer_set_scene or rfx_renderer_recut_triangles left them and the updates since rewrote them.  Returns the slot
 * count, leaves x (triangles per leaf), or 0 without a tree; any of the arrays may be NULL:
 *   leaf_ids : one int32 per slot -- the leaf membership the refit reads, in rfx_scene_tri_bvh_dump's leaf_ids layout;
 *   slot     : one int32 per triangle of the scene -- the slot an update writes the triangle's leaf record to, -1 for a
 *              triangle outside the tree;
 *   records  : 14 words per slot, read by position (not through `slot`): the leaf record's twelve geometry words, then
 *              the triangle index and the object index as stored (a padding slot: fourteen zero words).  Every NaN is
 *              reported as 0x7FC00000, as in rfx_renderer_tri_records.
 * Errors: NULL renderer: RFX_ERR_ARG; no scene uploaded: RFX_ERR_STATE. */
int rfx_renderer_tri_leaves(rfx_renderer *r, int32_t *leaf_ids, int32_t *slot, uint32_t *records);

/* ---------------------------------------------------------------- Re-cutting
 * The other half of moving meshes: rfx_renderer_update_triangles keeps the tree's topology as rfx_renderer_set_scene cut
 * it, and a mesh that has left that shape is traced through ever looser boxes.  rfx_renderer_recut_triangles rebuilds
 * the uploaded triangle BVH's topology and leaf membership on the device from the triangles' current vertices -- what
 * the updates so far left -- and refits every box.  Stream-ordered (NULL = the renderer's stream), no host sync, no
 * allocation.  (Added under RFX_ABI_VERSION 5; detect it by symbol.)  Nothing calls it by itself: when to re-cut is the
 * caller's policy.
 *
 * Values contract: no value of any launch changes.  The tree is a schedule (DESIGN.md "Triangle BVH -> Device": winners
 * do not depend on visiting order), so after a re-cut frames of every mode, rfx_trace_rays, the hit queries and spans,
 * the ordered forms and rfx_paths_step return word for word what they returned before it -- and so what a fresh
 * rfx_renderer_set_scene of the moved scene returns.  The call drops the per-view masks, as the update does, and
 * touches no random stream, tile cost, timing sum, regroup queue or rewind state.
 *
 * What stays as rfx_renderer_set_scene left it: the set of in-tree triangles (the T triangles that were well-conditioned
 * then), the residual list, the leaf count G = ceil(T / leaf size), the node count G - 1 (rfx_renderer_accel_info's
 * tri_nodes), the margin reference point and every device pointer.  tri_depth becomes ceil(log2 G).  After a re-cut
 * rfx_renderer_update_triangles keeps working, on the new tree.
 *
 * The cut is a function of the current vertices alone.  Every operation is IEEE float32 with no contraction, so a
 * float32 restatement gives the same bits:
 *   1. Per in-tree triangle t, from its current vertices and the class flag ill[t] the update keeps (word [28] of
 *      rfx_renderer_tri_records, inverted): s_a = (v1_a + v2_a) + v3_a per axis -- three times the centroid, with no
 *      division.  t is placed iff ill[t] == 0 and s_x, s_y, s_z are all finite.
 *   2. Box: per axis, lo_a = min and hi_a = max of s_a over the placed triangles (exact, so in any order);
 *      e = max_a (hi_a - lo_a); scale = 1024 / e where e is finite and > 0, else 0.  One scale for all axes: the cells
 *      are cubic.  The sign of a zero bound does not reach a key.
 *   3. Key: q_a = (uint32) fminf(fmaxf((s_a - lo_a) * scale, 0), 1023); bit b of q_x at 3b, of q_y at 3b + 1, of q_z
 *      at 3b + 2, 30 bits in all.  An in-tree triangle that is not placed takes key 0x40000000: ill triangles gather in
 *      the last leaves, where the all-space (NaN) boxes the refit gives them spoil only one spine of the tree.
 *   4. Order: the in-tree triangles are stably sorted by key, equal keys in ascending triangle index.  Leaf g holds the
 *      sorted entries [L g, L g + L), L = the leaf size (4); the last leaf is padded with -1, and padding records are all
 *      zero.  A leaf record is the triangle's twelve geometry words with its triangle and object index behind them.
 *   5. Topology: fixed by G alone.  node(a, b) over leaves [a, b) with b - a >= 2 takes the next index in pre-order (the
 *      root is node 0) and splits at mid = a + (b - a) / 2; a one-leaf side is the child ~a.  Depth ceil(log2 G) <= 15.
 *      Then the refit of "Moving meshes": every box from the current vertices, NaN bounds above an ill triangle.
 * The sort is rfx_rays_order's and shares the renderer's sort scratch with it (reserved for the in-tree count by
 * rfx_renderer_set_scene): as there, a re-cut and an order call of one renderer, or two re-cuts, on streams that are not
 * ordered with each other are the caller's error.
 *
 * Errors: NULL renderer: RFX_ERR_ARG; no scene uploaded, a small scene, or a scene without a triangle tree
 * (rfx_renderer_accel_info's tri_nodes == 0): RFX_ERR_STATE. */
int rfx_renderer_recut_triangles(rfx_renderer *r, void *stream);
/* The same cut on the host (no device): `built`'s in-tree set and residual list, the triangles classed and cut at
 * cut_vertices9_all, the boxes fitted to vertices9_all (NULL: the cut's) -- 9 floats for every triangle of the scene.
 * counts, boxes, children and leaf_ids in rfx_scene_tri_bvh_dump's layouts (counts[2] the residual count, counts[4] the
 * new depth), mt and widen as rfx_scene_tri_bvh_refit's; the arrays may be NULL.  Returns 1 with a tree, 0 without. */
int rfx_scene_tri_bvh_recut(const rfx_scene *built, const float *cut_vertices9_all, const float *vertices9_all, int widen,
                            int32_t counts[5], float *boxes, int32_t *children, int32_t *leaf_ids, float *mt);

/* ---------------------------------------------------------------- Moving spheres
 * Spheres of the uploaded scene take new centres and radii on the device, stream-ordered, without the host rebuild and
 * re-upload of rfx_renderer_set_scene.  (Added under RFX_ABI_VERSION 5; detect the calls by symbol.)
 *
 * Contract: after the call every launch on the renderer returns, word for word, what a renderer returns whose
 * rfx_renderer_set_scene got the same scene built at the new spheres -- frames of every mode, rfx_trace_rays, the hit
 * queries and spans, the ordered forms, rfx_paths_step -- settings, random streams and inputs being the same.  The update
 * touches neither random stream (rfx_renderer_get_rng reads the same before and after), nor the tile costs, the timing
 * sums, the regroup queue or the rewind state; it drops the per-view masks, as rfx_renderer_set_scene does.  The
 * coherent order's key box (rfx_renderer_order_box) and the regroup sort's cells stay as rfx_renderer_set_scene computed
 * them: they are schedule inputs, and no value depends on them.
 *
 * What follows a sphere (DESIGN.md "Moving spheres"): its centre and squared radius in both device forms, its bounding
 * sphere, the bound of its 64-sphere chunk, and the pair tree's boxes -- every node refitted on every update from the
 * current bounds alone, by the builder's own formulas, so repeated updates do not drift.  The device order of the spheres,
 * the tree's topology and its margin reference point stay as built: only speed follows spheres that have moved far from
 * where the tree was cut, and rfx_renderer_set_scene restores it.  Materials and object indices stay; lights do not move.
 * A sphere that is not finite (a NaN or infinite centre or radius) is never hit, as in the reference; its bounds come
 * out of the same formulas, and every cull keeps what it cannot bound.
 *
 * Works on every non-small scene (more than 32 spheres or more than 32 triangles): with a pair tree (more than 32
 * spheres), without one (at most 32 spheres beside more than 32 triangles, or a tree the walkers cannot take), with or
 * without a triangle tree.  A small scene is RFX_ERR_STATE: rfx_renderer_set_scene uploads it again in microseconds.
 * rfx_renderer_update_spheres, rfx_renderer_update_triangles and rfx_renderer_recut_triangles may follow each other on
 * one stream in any order.
 *
 * d_spheres4 holds four floats per record: centre x, y, z, then the radius.  The radius gets the constructor's clamp
 * (Sphere.cpp:13-19, as rfx_scene_add_sphere: radius <= VERY_SMALL_NUMBER becomes VERY_SMALL_NUMBER; a NaN passes), and
 * the squared radius is radius * radius in float.  `first` counts spheres in insertion order (0 = the scene's first
 * sphere; rfx_scene_object_sphere maps an object index to it).
 *   d_ids == NULL : spheres [first, first + count) take records 0 .. count - 1.
 *   d_ids != NULL : `first` is ignored; record k goes to sphere d_ids[k].  An id >= the scene's sphere count is a dead
 *                   lane (it cannot be an error without a sync).  Two records that name one sphere with different values
 *                   are the caller's error: the sphere's arrays could each take a different winner.
 * Stream-ordered (NULL = the renderer's stream), no host sync, no allocation.
 * Errors: NULL renderer or spheres, count == 0, d_ids == NULL with first + count > the scene's spheres: RFX_ERR_ARG; no
 * scene uploaded, or a small scene: RFX_ERR_STATE. */
int rfx_renderer_update_spheres(rfx_renderer *r, uint32_t first, uint32_t count, const float *d_spheres4,
                                const uint32_t *d_ids /* or NULL */, void *stream);
/* The same on host arrays: copies them in on the renderer's stream and synchronises. */
int rfx_renderer_update_spheres_host(rfx_renderer *r, uint32_t first, uint32_t count, const float *spheres4,
                                     const uint32_t *ids /* or NULL */);
/* The host scene kept in step: spheres [first, first + count) take the centres and (clamped) radii given.  Material and
 * object index stay.  Read by the next rfx_renderer_set_scene. */
int rfx_scene_set_spheres(rfx_scene *scene, uint32_t first, uint32_t count, const float *spheres4);
/* The sphere index (insertion order among spheres) of an object, or RFX_ERR_ARG for a non-sphere. */
int rfx_scene_object_sphere(const rfx_scene *scene, int object_index);
/* The words that follow a sphere's centre and radius, RFX_SPH_RECORD_WORDS uint32 per sphere of [first, first + count)
 * in insertion order, from the host scene and -- a device read-back, synchronises; not for a small scene -- from the
 * uploaded one:
 *   [0, 4)  the sphere's record: centre x y z, squared radius;
 *   [4, 8)  its lane of its pair record (the same four; the host scene: words [0, 4) again);
 *   [8, 12) its bounding sphere: centre x y z, radius * 1.00001f.
 * Every NaN is reported as 0x7FC00000, as in rfx_scene_tri_records. */
#define RFX_SPH_RECORD_WORDS 12
int rfx_scene_sph_records(const rfx_scene *scene, uint32_t first, uint32_t count, uint32_t *out);
int rfx_renderer_sph_records(rfx_renderer *r, uint32_t first, uint32_t count, uint32_t *out);
/* The pair tree a renderer builds for the scene's spheres (host only): counts = {nodes, leaves, spheres per leaf,
 * depth}; boxes -- nodes x 2 children x (lo x y z, hi x y z), as built, without the cull margin; children -- nodes x 2
 * (>= 0 a node, < 0 the leaf ~c); leaf_ids -- leaves x (spheres per leaf) sphere indices of the insertion order, -1
 * padding the last leaf; device_index -- per sphere of the insertion order its index in the device order (leaf g holds
 * device indices [g L, g L + L), chunk k [64 k, 64 k + 64)), filled with or without a tree.  The arrays may be NULL.
 * Returns 1 with a tree, 0 without (a small scene, at most 32 spheres, or a tree the walkers cannot take). */
int rfx_scene_sph_bvh_dump(const rfx_scene *scene, int32_t counts[4], float *boxes, int32_t *children,
                           int32_t *leaf_ids, uint32_t *device_index);
/* The tree rfx_scene_sph_bvh_dump reports for `built` -- its topology, device order and reference point -- refitted on
 * the host to the spheres given (4 floats for every sphere of the scene, insertion order), as the device update refits
 * it: boxes and mt as rfx_scene_tri_bvh_refit's; chunk_bounds -- 4 floats per 64-sphere chunk of the device order
 * (filled with or without a tree); any may be NULL.  widen = 0: the boxes as built (at the scene's own spheres: the
 * dump's, bit for bit); widen = 1: the device copy.  Every NaN is reported as 0x7FC00000.  Returns 1 with a tree, 0
 * without. */
int rfx_scene_sph_bvh_refit(const rfx_scene *built, const float *spheres4_all, int widen, float *boxes, float *mt,
                            float *chunk_bounds);
/* The uploaded pair tree's nodes read back (synchronises): 16 words per node, as rfx_renderer_tri_bvh_nodes, every NaN
 * reported as 0x7FC00000.  Returns the node count (0: no tree); out may be NULL to ask for it. */
int rfx_renderer_sph_bvh_nodes(rfx_renderer *r, float *out);
/* The uploaded chunk bounds read back (synchronises): 4 floats per chunk, NaNs as above.  Returns the chunk count; out
 * may be NULL to ask for it. */
int rfx_renderer_sph_chunk_bounds(rfx_renderer *r, float *out);
/* The padding lanes of the uploaded pair records read back (synchronises): the second lane of an odd count's last pair
 * and, with more than 32 spheres, the pairs that fill the last leaf -- 4 words per lane (centre 0, squared radius -inf:
 * never hit).  No update writes them.  Returns the lane count; out may be NULL to ask for it. */
int rfx_renderer_sph_padding(rfx_renderer *r, uint32_t *out);

/* ---------------------------------------------------------------- Device groups (multi-GPU, one process)
 * A group renders the frame of Render::renderNext (Render.cpp:136-215) on several devices of this process: row bands,
 * one per member, each member counting its slice of the frame's random stream and pushing it to the others (the one
 * exchange step), then emitting and tracing its band; members 1..n-1 copy their band rows into the
 * caller's frame on member 0's device over xGMI (hipMemcpyPeerAsync).  The assembled frame is the single-GPU frame
 * bit for bit.  Bands start equal (8-row multiples) and are re-cut from measured per-member trace times every 8
 * frames (completed measurements only: no frame waits), unless fixed with rfx_group_set_bands.  Member 0's renderer
 * carries the group's random streams: a frame starts every member from member 0's state, so the caller may render
 * other frames (block preview, spans) on member 0 alone in between, and rfx_frame_rng_rewind on member 0 undoes a
 * group frame.  For C/C++ callers without torch.distributed (dropin/Render.h: RFX_DEVICES=0,1,...); the
 * multi-process form is reflaxman_amd/dist.py over RCCL. */
typedef struct rfx_group rfx_group;
int rfx_group_create(rfx_group **out, const int *devices, int n);  /* a device may repeat (one-GPU rehearsal) */
void rfx_group_destroy(rfx_group *g);
int rfx_group_size(const rfx_group *g);
rfx_renderer *rfx_group_renderer(rfx_group *g, int member);       /* per-member settings (tile order, ...) */
int rfx_group_set_scene(rfx_group *g, const rfx_scene *scene);
/* fixed bands: bounds[0] = 0 < bounds[1] < ... < bounds[n] = height rows; bounds NULL = automatic (default) */
int rfx_group_set_bands(rfx_group *g, uint32_t height, const uint32_t *bounds);
int rfx_group_get_bands(const rfx_group *g, uint32_t *bounds);     /* the bands of the last frame (n + 1 rows) */
/* One whole frame (sample_num > 0; SSAA, additive and accumulation included; the partition fields of `frame` must be
 * rank 0 of 1 and the span the whole frame) into d_rgb / d_argb (W*H*3 floats / W*H words, or NULL) on member 0's
 * device, ordered after and before the caller's work on `stream` (member 0's stream; NULL = its renderer's).
 * d_rgb NULL (d_argb given, no accumulation): an ARGB8-only frame -- the members copy 4 B/px to member 0 instead of
 * 16 B/px, for a display that never reads the float image. */
int rfx_group_render_frame(rfx_group *g, const rfx_frame *frame, float *d_rgb, uint32_t *d_argb, void *stream);

/* Optional per-phase timing of rfx_render_frame with HIP events recorded on the launch stream:
 * enable, render, then read the summed device time (ms) of the RNG pre-pass and of the trace kernel
 * over the timed frames since the last read, and their number (synchronises; resets the sums).  enable = 1 times
 * every frame, n > 1 every n-th frame (three event records per timed frame cost ~10 us of a 640x480 frame's ~50). */
int rfx_renderer_set_timing(rfx_renderer *r, int enable);
int rfx_renderer_get_timing(rfx_renderer *r, double *prepass_ms, double *trace_ms, uint64_t *frames);

/* host-buffer convenience for callers without device memory of their own (PCIe-inclusive):
 * rgb: host W*H*3 (in/out), argb: host W*H or NULL.  Partitioning fields must be rank 0 of 1. */
int rfx_render_frame_host(rfx_renderer *r, const rfx_frame *frame, float *rgb, uint32_t *argb,
                          uint64_t *counters);

/* device memory helpers for C/C++ hosts that have no allocator of their own */
int rfx_device_alloc(rfx_renderer *r, size_t bytes, void **dptr);
int rfx_device_free(rfx_renderer *r, void *dptr);
int rfx_memcpy_d2h(rfx_renderer *r, void *dst, const void *src, size_t bytes);
int rfx_memcpy_h2d(rfx_renderer *r, void *dst, const void *src, size_t bytes);
/* device-to-device copy on the renderer's stream (asynchronous) */
int rfx_memcpy_d2d(rfx_renderer *r, void *dst, const void *src, size_t bytes);
int rfx_synchronize(rfx_renderer *r);

/* Sample the RNG stream: the first n randomInsideSphere draws from `seed` (Vector3.cpp:176-188),
 * computed by the device pre-pass, n x 3 floats to host.  *seed_out = state after them. */
int rfx_rand_dirs(rfx_renderer *r, uint32_t seed, uint64_t n, float *out3, uint32_t *seed_out);

/*
 * Device known-answer entry points (validation).  Each runs the trace kernel's own device code on host
 * arrays and returns host results, synchronously, on the scene last uploaded by rfx_renderer_set_scene:
 *   rfx_kat_objects: ray i = rays[6i..6i+5] (origin, direction) against object objects[i] alone ->
 *       out[15i..]: hit, drop3, normal3, reflected ray3, distance, material colour3 (texel of a textured
 *       triangle), any-hit -- SceneObject::trace with and without out-parameters (Sphere.cpp:44-85,
 *       Triangle.cpp:53-108, Plane.cpp:36-73);
 *   rfx_kat_texels: texture >= 0: Texture::getTexelColor(u, v) (in n x 2, Texture.cpp:231-269) of that scene
 *       texture; texture < 0: Skybox::getTexelColor(ray) (in n x 3, Skybox.cpp:39-106) -> out n x 3;
 *   rfx_kat_powf: powf(x, y) as Scene.cpp:175,196 evaluate it (in n x 2 -> out n);
 *   rfx_kat_argb: Color::argb (Color.cpp:114-117) (in n x 3 -> out n);
 *   rfx_kat_powf_cube: the Fresnel site's powf(x, 3) (Scene.cpp:196) as the bounce loop evaluates it (the double
 *       cube where it provably rounds like glibc, rfx_powf.h powf_cube_fast) against glibc's algorithm on the device,
 *       for every float x in [0, 1]: counts[0] = mismatches (0 expected), counts[1] = inputs that took glibc's
 *       algorithm;
 *   rfx_kat_div: the trace loop's division fast paths (rfx_math.h div_rn, normalized's shared reciprocal and the
 *       skybox's div_fast_unit) against IEEE '/' on the operand pairs first .. first + n - 1 of a fixed hash (every
 *       float class, both edges of the fast path's divisor and quotient bounds): counts[0] = quotients whose bits
 *       differ (0 expected), counts[1] = pairs that took div_rn's fast path, counts[2] = quotients checked (5 per
 *       pair).
 *   rfx_kat_far_light: the bounce loop's far-light form against its general form for the scene's first light
 *       (rfx_scene_far_light) at n points d (in n x 3 -> out n x 8): the general expressions' dirToLight x y z, its
 *       length, its direction x y z and 1 - sqrt(ang) (0 unless ang > 0) at d; all eight NaN where d lies inside the
 *       light's bound and the light's recorded terms differ from them in any bit.
 */
int rfx_kat_far_light(rfx_renderer *r, const float *points, uint64_t n, float *out);
int rfx_kat_objects(rfx_renderer *r, const float *rays, const int32_t *objects, uint64_t n, float *out);
int rfx_kat_texels(rfx_renderer *r, int texture, const float *in, uint64_t n, float *out);
int rfx_kat_powf(rfx_renderer *r, const float *xy, uint64_t n, float *out);
int rfx_kat_argb(rfx_renderer *r, const float *rgb, uint64_t n, uint32_t *out);
int rfx_kat_powf_cube(rfx_renderer *r, uint64_t counts[2]);
int rfx_kat_div(rfx_renderer *r, uint64_t first, uint64_t n, uint64_t counts[3]);
/* The kernel-argument layout the bounce loops rely on (rfx_bounce.h launder_scene / kernarg_params: DevScene at kernarg
 * offset 0, FrameParams after it): a one-lane kernel of the trace kernels' signature compares the records read through
 * the kernarg segment pointer with its by-value arguments.  out[0] / out[1] = differing words of the scene record / the
 * frame parameters (0 expected), out[2] = 1 if the build reads the scene record that way.  swapped = 1 runs the same
 * check in a kernel declared (FrameParams, DevScene): the check must report differences there. */
int rfx_kat_kernarg(rfx_renderer *r, int swapped, uint32_t out[3]);
/* The cycle table (rfx_renderer_set_rng_prepass), built if it is not yet: prefix[B] = accepted triples of the cycle's
 * blocks [0, B), B <= rfx_rng_seq_blocks() (the last word: the cycle's total). */
int rfx_kat_rng_seq_prefix(rfx_renderer *r, uint32_t *prefix);
/* The same blocks' accept counts from the per-frame count kernel run on the cycle's origin state:
 * counts[B], B < rfx_rng_seq_blocks(). */
int rfx_kat_rng_seq_legacy(rfx_renderer *r, uint32_t *counts);

#ifdef __cplusplus
}
#endif
#endif /* RFX_H */
