// The host-only part of librfx.so: the scene builder C-ABI of include/rfx.h (scene objects, textures and their TGA / BMP
// files, camera helpers, strip arithmetic), the two hierarchy builders, and SceneBuild -- the host half of
// rfx_renderer_set_scene.  Scene builder calls restate the reference's constructors (host precompute in strict IEEE,
// shared rfx_math.h).  Nothing here touches HIP: the file also compiles with a plain C++ compiler (-ffp-contract=off),
// which is how tests/native/scene_host_check.cpp runs it under the host sanitizers.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "rfx_cull_rule.h"
#include "rfx_math.h"
#include "rfx_refit.h"
#include "rfx_scene.h"

#pragma clang fp contract(off)

using namespace rfx;

static thread_local std::string g_last_error;

int rfx::fail(int code, const char *fmt, ...)
{
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

extern "C" const char *rfx_last_error(void) { return g_last_error.c_str(); }

// ============================================================== scene (host)
// w x h as loaded; no texels = the reference's empty colorBuf (procedural checker).  loaded: the file was read
// (Skybox::loadTexture then derives its half tiles from w and h, Skybox.cpp:21-37).
struct HostTexture { uint32_t w = 0, h = 0; bool loaded = false; std::vector<uint32_t> texels; };
struct HostMat { int dielectric; float r, g, b, refl, transp; };
struct HostSphere { v3 center; float radius, sq_radius; HostMat mat; int obj; };
struct HostTri {
  v3 v0, v1, v2, norm;
  double cond = INFINITY;  // ||M||_F ||M^-1||_F of the basis M = [v2-v0 | v1-v0 | -norm] (cull bound)
  m33 ax, tuv;
  float tu0 = 0, tv0 = 0;
  int tex = -1;
  HostMat mat;
  int obj;
};
struct HostLight { v3 origin; float radius; float r, g, b, power; };
struct HostPlane { v3 pos, norm; HostMat mat; int obj; };

struct rfx_scene {
  col diff, env;
  float diff_power;
  float half_tile_w, half_tile_h;
  int skybox = -1;
  int tri_mates = 1;  // rfx_scene_set_tri_mates
  int far_lights = 1;  // rfx_scene_set_far_lights
  int shadow_grid = 1;  // rfx_scene_set_shadow_grid (rfx_scene_create: RFX_SHADOW_GRID in the environment)
  std::vector<HostSphere> spheres;
  std::vector<HostTri> tris;
  std::vector<HostPlane> planes;
  std::vector<int> obj_kind, obj_idx;  // insertion order: kind 0 sphere, 1 triangle, 2 plane
  std::vector<HostLight> lights;
  std::vector<HostTexture> textures;
};

static void default_half_tiles(rfx_scene *s)  // Skybox.cpp:5-9 / failed load :32-33
{
  s->half_tile_w = 1.0f / 8.0f - kFltEpsilon;
  s->half_tile_h = 1.0f / 6.0f - kFltEpsilon;
}

extern "C" rfx_scene *rfx_scene_create(float dr, float dg, float db, float dp)   // Scene.cpp:10-15
{
  rfx_scene *s = new rfx_scene();
  s->diff = mkc(dr, dg, db);
  s->diff_power = dp;
  s->env = cscale(s->diff, dp);
  default_half_tiles(s);
  // A/B runs of one build: RFX_SHADOW_GRID=0, 1 or 2 in the environment is a new scene's rfx_scene_set_shadow_grid mode
  if (const char *v = getenv("RFX_SHADOW_GRID"))
    if ((v[0] == '0' || v[0] == '1' || v[0] == '2') && !v[1]) s->shadow_grid = v[0] - '0';
  return s;
}

extern "C" void rfx_scene_destroy(rfx_scene *s) { delete s; }

static HostMat make_mat(int type, const float rgb[3], float refl, float transp)      // Material.cpp:8-14
{
  HostMat m;
  m.dielectric = type == RFX_DIELECTRIC;
  m.r = rgb[0]; m.g = rgb[1]; m.b = rgb[2];
  m.refl = clampf(refl, 0.0f, 1.0f);
  m.transp = clampf(transp, 0.0f, 1.0f);
  return m;
}

extern "C" int rfx_scene_add_sphere(rfx_scene *s, const float c[3], float radius, int type, const float rgb[3],
                                    float refl, float transp)                          // Scene.cpp:29-39
{
  if (!s || !c || !rgb || (type != RFX_METAL && type != RFX_DIELECTRIC)) return fail(RFX_ERR_ARG, "add_sphere: bad args");
  if (radius <= kVerySmall) radius = kVerySmall;
  HostSphere sp;
  sp.center = mk(c[0], c[1], c[2]);
  sp.radius = radius;
  sp.sq_radius = radius * radius;                                                    // Sphere.cpp:19
  sp.mat = make_mat(type, rgb, refl, transp);
  sp.obj = (int)s->obj_kind.size();
  s->obj_kind.push_back(0);
  s->obj_idx.push_back((int)s->spheres.size());
  s->spheres.push_back(sp);
  return sp.obj;
}

// Triangle.cpp:11-21 (v0, v1, v2, norm, axTrans) and the builder's condition number of the basis, from the vertices
static void set_tri_vertices(HostTri &t, const float a[3], const float b[3], const float c[3])
{
  const TriSetup u = tri_setup(mk(a[0], a[1], a[2]), mk(b[0], b[1], b[2]), mk(c[0], c[1], c[2]));
  t.v0 = u.v0; t.v1 = u.v1; t.v2 = u.v2;
  t.norm = u.norm;
  t.ax = u.ax;
  t.cond = u.det_ok ? sqrt(u.p) : INFINITY;
}

extern "C" int rfx_scene_add_triangle(rfx_scene *s, const float a[3], const float b[3], const float c[3], int type,
                                      const float rgb[3], float refl, float transp)    // Triangle.cpp:11-21
{
  if (!s || !a || !b || !c || !rgb || (type != RFX_METAL && type != RFX_DIELECTRIC))
    return fail(RFX_ERR_ARG, "add_triangle: bad args");
  HostTri t;
  set_tri_vertices(t, a, b, c);
  t.mat = make_mat(type, rgb, refl, transp);
  memset(&t.tuv, 0, sizeof(t.tuv));
  t.obj = (int)s->obj_kind.size();
  s->obj_kind.push_back(1);
  s->obj_idx.push_back((int)s->tris.size());
  s->tris.push_back(t);
  return t.obj;
}

extern "C" int rfx_scene_add_mesh(rfx_scene *s, const float *vertices, uint32_t n_vertices, const uint32_t *indices,
                                  uint32_t n_triangles, int type, const float rgb[3], float refl, float transp)
{
  if (!s || !rgb || (type != RFX_METAL && type != RFX_DIELECTRIC) || (n_triangles && (!vertices || !indices)))
    return fail(RFX_ERR_ARG, "add_mesh: bad args");
  for (size_t i = 0; i < 3 * (size_t)n_triangles; ++i)
    if (indices[i] >= n_vertices)
      return fail(RFX_ERR_ARG, "add_mesh: index %u of triangle %zu is not below %u vertices", indices[i], i / 3, n_vertices);
  const int first = (int)s->obj_kind.size();
  s->tris.reserve(s->tris.size() + n_triangles);
  for (size_t i = 0; i < n_triangles; ++i)
  {
    const int rc = rfx_scene_add_triangle(s, vertices + 3 * (size_t)indices[3 * i], vertices + 3 * (size_t)indices[3 * i + 1],
                                          vertices + 3 * (size_t)indices[3 * i + 2], type, rgb, refl, transp);
    if (rc < 0) return rc;
  }
  return first;
}

extern "C" int rfx_scene_add_plane(rfx_scene *s, const float pos[3], const float norm[3], int type, const float rgb[3],
                                   float refl, float transp)                         // Plane.cpp:9-14
{
  if (!s || !pos || !norm || !rgb || (type != RFX_METAL && type != RFX_DIELECTRIC))
    return fail(RFX_ERR_ARG, "add_plane: bad args");
  HostPlane p;
  p.pos = mk(pos[0], pos[1], pos[2]);
  p.norm = mk(norm[0], norm[1], norm[2]);
  p.mat = make_mat(type, rgb, refl, transp);
  p.obj = (int)s->obj_kind.size();
  s->obj_kind.push_back(2);
  s->obj_idx.push_back((int)s->planes.size());
  s->planes.push_back(p);
  return p.obj;
}

extern "C" int rfx_triangle_set_texture(rfx_scene *s, int obj, int tex, const float uv[6])  // Triangle.cpp:110-120
{
  if (!s || !uv || obj < 0 || obj >= (int)s->obj_kind.size() || s->obj_kind[obj] != 1)
    return fail(RFX_ERR_ARG, "set_texture: object %d is not a triangle", obj);
  if (tex < 0 || tex >= (int)s->textures.size()) return fail(RFX_ERR_ARG, "set_texture: bad texture %d", tex);
  HostTri &t = s->tris[s->obj_idx[obj]];
  t.tex = tex;
  t.tu0 = uv[0];
  t.tv0 = uv[1];
  const v3 p1 = mk(uv[0], uv[1], 0), p2 = mk(uv[2], uv[3], 0), p3 = mk(uv[4], uv[5], 0);
  t.tuv = from_cols(sub(p3, p1), sub(p2, p1), mk(0, 0, -1));
  return RFX_OK;
}

extern "C" int rfx_scene_add_light(rfx_scene *s, const float o[3], float radius, const float rgb[3], float power)
{                                                                                     // Scene.cpp:48-59
  if (!s || !o || !rgb) return fail(RFX_ERR_ARG, "add_light: bad args");
  if (radius <= kVerySmall) radius = kVerySmall;
  const col c = mkc(rgb[0], rgb[1], rgb[2]);
  s->env = cadd(s->env, cscale(c, power));
  HostLight l;
  l.origin = mk(o[0], o[1], o[2]);
  l.radius = radius;
  l.r = c.r; l.g = c.g; l.b = c.b;
  l.power = clampf(power, 0.0f, 1.0f);                                                // OmniLight.cpp:13
  s->lights.push_back(l);
  return (int)s->lights.size() - 1;
}

extern "C" int rfx_scene_add_texture_argb(rfx_scene *s, uint32_t w, uint32_t h, const uint32_t *argb)
{
  if (!s) return fail(RFX_ERR_ARG, "add_texture: null scene");
  HostTexture t;
  if (argb && w && h)
  {
    t.w = w; t.h = h;
    t.loaded = true;
    t.texels.assign(argb, argb + (size_t)w * h);
  }
  s->textures.push_back(std::move(t));
  return (int)s->textures.size() - 1;
}

// ---- TGA / BMP (Texture.cpp:34-173, image_headers.h) ----
#pragma pack(push, 1)
struct TgaHeader { int8_t idlen, colmptype, imagetype; int16_t cmorg, cmlen; int8_t cmbits; int16_t xoff, yoff, xsize, ysize; int8_t bpix, imagedesc; };
struct BmpFileHeader { uint16_t bfType; uint32_t bfSize; uint16_t r1, r2; uint32_t bfOffBits; };
struct BmpInfoHeader { uint32_t biSize; int32_t biWidth, biHeight; uint16_t biPlanes, biBitCount; uint32_t biCompression, biSizeImage; int32_t xppm, yppm; uint32_t clrUsed, clrImportant; };
#pragma pack(pop)

// Texture::loadFromTGAFile (Texture.cpp:34-108): type 2, 24/32 bpp, rows in file order (origin bit ignored).
// As in the reference a header with a zero width or height loads successfully as an empty texture (w x h kept,
// no texels).  Negative (int16) sizes, which the reference cannot allocate, fail.
static bool tga_read(const char *path, uint32_t &w, uint32_t &h, std::vector<uint32_t> &out)
{
  w = h = 0;
  out.clear();
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  TgaHeader hd;
  bool ok = false;
  if (fread(&hd, sizeof(hd), 1, f) == 1 && hd.imagetype == 2 && hd.xsize >= 0 && hd.ysize >= 0)
  {
    const uint32_t W = (uint32_t)hd.xsize, H = (uint32_t)hd.ysize;
    const int bpp = hd.bpix;
    const long off = (long)sizeof(hd) + hd.idlen + hd.cmlen * hd.cmbits / 8;
    if (!fseek(f, off, SEEK_SET) && (bpp == 24 || bpp == 32))
    {
      const size_t n = (size_t)W * H, ps = (size_t)bpp / 8;
      std::vector<uint8_t> raw(n * ps);
      if (!n || fread(raw.data(), 1, raw.size(), f) == raw.size())
      {
        out.resize(n);
        for (size_t i = 0; i < n; ++i)
        {
          const uint8_t *p = &raw[i * ps];
          const uint32_t a = bpp == 32 ? p[3] : 0xFFu;
          out[i] = a << 24 | (uint32_t)p[2] << 16 | (uint32_t)p[1] << 8 | p[0];
        }
        w = W; h = H;
        ok = true;
      }
    }
  }
  fclose(f);
  if (!ok) out.clear();
  return ok;
}

static bool has_ext(const char *path, const char *ext)
{
  const char *dot = strrchr(path, '.');
  return dot && !strcmp(dot, ext);
}

extern "C" int rfx_tga_load(const char *path, uint32_t *w, uint32_t *h, uint32_t *argb, size_t capacity)
{
  if (!path || !w || !h) return fail(RFX_ERR_ARG, "tga_load: bad args");
  std::vector<uint32_t> px;
  if (!tga_read(path, *w, *h, px)) return fail(RFX_ERR_IO, "tga_load: cannot read %s", path);
  if (argb)
  {
    if (capacity < px.size()) return fail(RFX_ERR_ARG, "tga_load: capacity %zu < %zu", capacity, px.size());
    memcpy(argb, px.data(), px.size() * 4);
  }
  return RFX_OK;
}

extern "C" int rfx_tga_save(const char *path, uint32_t w, uint32_t h, const uint32_t *argb)  // Texture.cpp:110-137
{
  if (!path || !argb || !w || !h) return fail(RFX_ERR_ARG, "tga_save: bad args");
  FILE *f = fopen(path, "wb");
  if (!f) return fail(RFX_ERR_IO, "tga_save: cannot open %s", path);
  TgaHeader hd;
  memset(&hd, 0, sizeof(hd));
  hd.imagetype = 2; hd.xsize = (int16_t)w; hd.ysize = (int16_t)h; hd.bpix = 32;
  bool ok = fwrite(&hd, sizeof(hd), 1, f) == 1 && fwrite(argb, (size_t)w * h * 4, 1, f) == 1;
  fclose(f);
  return ok ? RFX_OK : fail(RFX_ERR_IO, "tga_save: short write");
}

extern "C" int rfx_bmp_save(const char *path, uint32_t w, uint32_t h, const uint32_t *argb)  // Texture.cpp:139-173
{
  if (!path || !argb || !w || !h) return fail(RFX_ERR_ARG, "bmp_save: bad args");
  FILE *f = fopen(path, "wb");
  if (!f) return fail(RFX_ERR_IO, "bmp_save: cannot open %s", path);
  BmpFileHeader fh;
  BmpInfoHeader ih;
  memset(&fh, 0, sizeof(fh));
  memset(&ih, 0, sizeof(ih));
  fh.bfType = ((uint16_t)'M' << 8) | (uint16_t)'B';
  fh.bfSize = (uint32_t)(sizeof(fh) + sizeof(ih) + (size_t)w * h * 4);
  fh.bfOffBits = sizeof(fh) + sizeof(ih);
  ih.biSize = sizeof(ih); ih.biWidth = (int32_t)w; ih.biHeight = (int32_t)h; ih.biPlanes = 1; ih.biBitCount = 32;
  bool ok = fwrite(&fh, sizeof(fh), 1, f) == 1 && fwrite(&ih, sizeof(ih), 1, f) == 1 &&
            fwrite(argb, (size_t)w * h * 4, 1, f) == 1;
  fclose(f);
  return ok ? RFX_OK : fail(RFX_ERR_IO, "bmp_save: short write");
}

extern "C" int rfx_scene_add_texture_file(rfx_scene *s, const char *path, int *loaded)  // Scene.cpp:61-66
{
  if (!s || !path) return fail(RFX_ERR_ARG, "add_texture_file: bad args");
  HostTexture t;
  const bool ok = has_ext(path, ".tga") && tga_read(path, t.w, t.h, t.texels);     // Texture.cpp:175-189
  t.loaded = ok;
  if (loaded) *loaded = ok ? 1 : 0;
  s->textures.push_back(std::move(t));
  return (int)s->textures.size() - 1;
}

static void set_skybox_index(rfx_scene *s, int idx)                                   // Skybox.cpp:21-37
{
  s->skybox = idx;
  const HostTexture &t = s->textures[idx];
  if (t.loaded)
  {
    s->half_tile_w = 1.0f / 8.0f - 1.0f / (float)t.w - kFltEpsilon;
    s->half_tile_h = 1.0f / 6.0f - 1.0f / (float)t.h - kFltEpsilon;
  }
  else
    default_half_tiles(s);
}

extern "C" int rfx_scene_set_skybox_file(rfx_scene *s, const char *path)
{
  if (!s || !path) return fail(RFX_ERR_ARG, "set_skybox_file: bad args");
  int loaded = 0;
  const int idx = rfx_scene_add_texture_file(s, path, &loaded);
  set_skybox_index(s, idx);
  return loaded;
}

extern "C" int rfx_scene_set_skybox_argb(rfx_scene *s, uint32_t w, uint32_t h, const uint32_t *argb)
{
  if (!s) return fail(RFX_ERR_ARG, "set_skybox_argb: null scene");
  const int idx = rfx_scene_add_texture_argb(s, w, h, argb);
  set_skybox_index(s, idx);
  return s->textures[idx].loaded ? 1 : 0;
}

extern "C" int rfx_scene_plane_count(const rfx_scene *s)
{
  if (!s) return fail(RFX_ERR_ARG, "plane_count: null scene");
  return (int)s->planes.size();
}

extern "C" int rfx_scene_counts(const rfx_scene *s, int *ns, int *nt, int *nl, int *nx)
{
  if (!s) return fail(RFX_ERR_ARG, "counts: null scene");
  if (ns) *ns = (int)s->spheres.size();
  if (nt) *nt = (int)s->tris.size();
  if (nl) *nl = (int)s->lights.size();
  if (nx) *nx = (int)s->textures.size();
  return RFX_OK;
}

// ============================================================== camera / images
extern "C" void rfx_camera_view(const float e[3], const float a[3], float view[9])    // Camera.cpp:24-38
{
  const v3 eye = mk(e[0], e[1], e[2]), at = mk(a[0], a[1], a[2]);
  const v3 up = mk(0.0f, 1.0f, 0.0f);
  const v3 oz = normalized(sub(at, eye));
  const v3 ox = normalized(cross(up, oz));
  const v3 oy = normalized(cross(oz, ox));
  const m33 m = from_cols(ox, oy, oz);
  memcpy(view, &m, sizeof(m));
}

extern "C" float rfx_camera_rz(uint32_t width, float fov)                             // Render.cpp:148
{
  return (float)width / 2.0f / tanf(fov / 2.0f);
}

extern "C" void rfx_argb_from_rgb(const float *rgb, size_t n, uint32_t *out)
{
  for (size_t i = 0; i < n; ++i) out[i] = argb(mkc(rgb[i * 3], rgb[i * 3 + 1], rgb[i * 3 + 2]));
}

extern "C" uint32_t rfx_strip_rows(uint32_t H, uint32_t rb, uint32_t rank, uint32_t nranks)
{
  if (nranks <= 1) return H;
  if (!rb || rank >= nranks) return 0;
  const uint32_t full = H / rb, rem = H % rb;
  uint32_t rows = (full / nranks) * rb;
  const uint32_t extra = full % nranks;
  if (rank < extra) rows += rb;
  if (rem && full % nranks == rank) rows += rem;
  return rows;
}

extern "C" uint32_t rfx_strip_row_to_y(uint32_t r, uint32_t rb, uint32_t rank, uint32_t nranks)
{
  if (nranks <= 1) return r;
  return (r / rb * nranks + rank) * rb + r % rb;
}

// ============================================================== hierarchies
// RFX_TRI_BVH_AUTO_MIN: rfx_renderer_set_tri_accel(-1): the triangle count from which a non-small scene gets the
// triangle BVH (DESIGN.md "Triangle BVH": the smallest measured soup size at which the tree wins)
// RFX_TRI_BVH_NARROW_MIN: the triangle count from which narrow bundles (a tile's primary rays) walk the triangle BVH too
// instead of culling every triangle's bound for the wave: never by default -- the bundle cull won on every soup from 64
// to 100,000 triangles (0.8% to 15% less trace time) and lost 1% on a 2,560-triangle height field (DESIGN.md "Triangle BVH")
// Device order of a large scene's spheres: recursive median splits of the centres along their longest axis,
// left parts of even size, so pairs (2j, 2j + 1) are neighbours and every aligned run of 2^k spheres is a
// compact cluster (the 64-sphere chunks of the bundle cull, the leaves of the pair BVH).
static void spatial_order(std::vector<uint32_t> &idx, size_t a, size_t b, const std::vector<HostSphere> &sp)
{
  if (b - a <= 2) return;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (size_t i = a; i < b; ++i)
  {
    const double c[3] = {sp[idx[i]].center.x, sp[idx[i]].center.y, sp[idx[i]].center.z};
    for (int k = 0; k < 3; ++k) { lo[k] = fmin(lo[k], c[k]); hi[k] = fmax(hi[k], c[k]); }
  }
  int axis = 0;
  for (int k = 1; k < 3; ++k)
    if (hi[k] - lo[k] > hi[axis] - lo[axis]) axis = k;
  const size_t mid = a + 2 * ((b - a + 2) / 4);
  auto key = [&](uint32_t i) { return axis == 0 ? sp[i].center.x : axis == 1 ? sp[i].center.y : sp[i].center.z; };
  std::nth_element(idx.begin() + a, idx.begin() + mid, idx.begin() + b,
                   [&](uint32_t x, uint32_t y) { return key(x) < key(y) || (key(x) == key(y) && x < y); });
  spatial_order(idx, a, mid, sp);
  spatial_order(idx, mid, b, sp);
}

// Pair BVH of a large scene: leaves are the device sphere pairs (2j, 2j + 1, neighbours); internal nodes
// split their pairs where the surface-area heuristic is lowest (every position of the pair centres sorted
// along each axis), as long as the split keeps the tree within the kernel's stack depth, else at the
// median of the pair centres along the longest axis (SAH against median splits alone: C5 -0.8%, round 2).  Each
// node stores its two
// children's boxes (spheres grown by their radii); the kernel widens them by its exact-cull margin per ray.
// Returns the node index (or ~pair for a leaf) of range [a, b) of `pairs`; depth: internal levels below.
namespace {
struct PairBox { double lo[3], hi[3], c[3]; };

int build_pair_bvh(std::vector<BvhNode> &nodes, std::vector<uint32_t> &pairs, size_t a, size_t b,
                   const std::vector<PairBox> &box, const double *ref, int level, int &depth, bool widen = true)
{
  if (b - a == 1) return ~(int)pairs[a];
  depth = std::max(depth, level + 1);
  const int id = (int)nodes.size();
  nodes.push_back(BvhNode{});
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (size_t i = a; i < b; ++i)
    for (int k = 0; k < 3; ++k) { lo[k] = fmin(lo[k], box[pairs[i]].c[k]); hi[k] = fmax(hi[k], box[pairs[i]].c[k]); }
  int axis = 0;
  for (int k = 1; k < 3; ++k)
    if (hi[k] - lo[k] > hi[axis] - lo[axis]) axis = k;
  size_t mid = a + (b - a) / 2;
  // surface-area heuristic over sorted pair centres (all three axes, every split position), while the depth
  // budget allows an unbalanced split: the subtree of n leaves must still fit kBvhStack levels
  const size_t cnt = b - a;
  int need = 0;
  while (((size_t)1 << need) < cnt) ++need;
  if (level + need + 2 <= kBvhStack && cnt > 2)
  {
    double best = INFINITY;
    int best_axis = axis;
    size_t best_mid = mid;
    std::vector<uint32_t> tmp(pairs.begin() + a, pairs.begin() + b);
    std::vector<double> right(cnt + 1);
    auto area = [](const double *l, const double *h) {
      const double dx = h[0] - l[0], dy = h[1] - l[1], dz = h[2] - l[2];
      return dx * dy + dy * dz + dz * dx;
    };
    for (int ax = 0; ax < 3; ++ax)
    {
      std::sort(tmp.begin(), tmp.end(), [&](uint32_t x, uint32_t y) {
        return box[x].c[ax] < box[y].c[ax] || (box[x].c[ax] == box[y].c[ax] && x < y);
      });
      double l[3] = {INFINITY, INFINITY, INFINITY}, h[3] = {-INFINITY, -INFINITY, -INFINITY};
      for (size_t i = cnt; i-- > 0;)
      {
        for (int k = 0; k < 3; ++k) { l[k] = fmin(l[k], box[tmp[i]].lo[k]); h[k] = fmax(h[k], box[tmp[i]].hi[k]); }
        right[i] = area(l, h) * (double)(cnt - i);
      }
      for (int k = 0; k < 3; ++k) { l[k] = INFINITY; h[k] = -INFINITY; }
      // a split leaving at most 2^(budget - 1) leaves on each side keeps the depth bound
      const size_t cap = (size_t)1 << std::min(30, kBvhStack - level - 2);
      for (size_t i = 1; i < cnt; ++i)
      {
        for (int k = 0; k < 3; ++k) { l[k] = fmin(l[k], box[tmp[i - 1]].lo[k]); h[k] = fmax(h[k], box[tmp[i - 1]].hi[k]); }
        if (i > cap || cnt - i > cap) continue;
        const double cost = area(l, h) * (double)i + right[i];
        if (cost < best) { best = cost; best_axis = ax; best_mid = a + i; }
      }
    }
    axis = best_axis;
    mid = best_mid;
  }
  std::nth_element(pairs.begin() + a, pairs.begin() + mid, pairs.begin() + b, [&](uint32_t x, uint32_t y) {
    return box[x].c[axis] < box[y].c[axis] || (box[x].c[axis] == box[y].c[axis] && x < y);
  });
  const int kids[2] = {build_pair_bvh(nodes, pairs, a, mid, box, ref, level + 1, depth, widen),
                       build_pair_bvh(nodes, pairs, mid, b, box, ref, level + 1, depth, widen)};
  const size_t range[2][2] = {{a, mid}, {mid, b}};
  BvhNode &n = nodes[id];
  for (int c = 0; c < 2; ++c)
  {
    double l[3] = {INFINITY, INFINITY, INFINITY}, h[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t i = range[c][0]; i < range[c][1]; ++i)
      for (int k = 0; k < 3; ++k) { l[k] = fmin(l[k], box[pairs[i]].lo[k]); h[k] = fmax(h[k], box[pairs[i]].hi[k]); }
    // widened by the cull margin's node part (widen false: rfx_scene_tri_bvh_dump, the boxes as built), rounded
    // outwards to float, with the child's margin term: rfx_refit.h, shared with the refits
    bvh_child_set(n, c, l, h, ref, widen);
    n.child[c] = kids[c];
  }
  return id;
}

// The pair tree of a large scene's spheres (more than 32) from their bounds in device order: the leaves are groups of
// RFX_BVH_LEAF_PAIRS consecutive pairs (compact clusters of the median-split order; rfx_refit.h sph_leaf_box, shared
// with the refits), the reference point the root box centre as the float the kernel measures from.  Returns the depth;
// no nodes (depth 0) for a tree deeper than the kernel's stack or larger than its int16 stack slots hold (rfx_bvh.h):
// the chunk loops.
int sphere_bvh(const std::vector<Bound> &bd, size_t nsph, bool widen, std::vector<BvhNode> &bvh, double *ref)
{
  const size_t npairs = ((nsph + 1) / 2 + RFX_BVH_LEAF_PAIRS - 1) / RFX_BVH_LEAF_PAIRS;
  std::vector<PairBox> box(npairs);
  for (size_t j = 0; j < npairs; ++j)
  {
    const SphBox b = sph_leaf_box(bd.data(), (uint32_t)j, (uint32_t)nsph);
    for (int k = 0; k < 3; ++k) { box[j].lo[k] = b.lo[k]; box[j].hi[k] = b.hi[k]; box[j].c[k] = 0.5 * (b.lo[k] + b.hi[k]); }
  }
  std::vector<uint32_t> pairs(npairs);
  for (size_t j = 0; j < npairs; ++j) pairs[j] = (uint32_t)j;
  for (int k = 0; k < 3; ++k)
  {
    double lo = INFINITY, hi = -INFINITY;
    for (const PairBox &pb : box) { lo = fmin(lo, pb.lo[k]); hi = fmax(hi, pb.hi[k]); }
    ref[k] = (double)(float)(0.5 * (lo + hi));
  }
  int depth = 0;
  bvh.clear();
  build_pair_bvh(bvh, pairs, 0, npairs, box, ref, 0, depth, widen);
  if (depth > kBvhStack || bvh.size() > 32767 || npairs > 32768) { bvh.clear(); depth = 0; }
  return depth;
}

// the spatial order of build_tri_tree (below)
void tri_spatial_order(std::vector<int32_t> &idx, size_t a, size_t b, const std::vector<double> &cen)
{
  if (b - a <= RFX_TRI_BVH_LEAF) return;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (size_t i = a; i < b; ++i)
    for (int k = 0; k < 3; ++k) { lo[k] = fmin(lo[k], cen[3 * idx[i] + k]); hi[k] = fmax(hi[k], cen[3 * idx[i] + k]); }
  int axis = 0;
  for (int k = 1; k < 3; ++k)
    if (hi[k] - lo[k] > hi[axis] - lo[axis]) axis = k;
  const size_t groups = (b - a + RFX_TRI_BVH_LEAF - 1) / RFX_TRI_BVH_LEAF;
  const size_t mid = a + RFX_TRI_BVH_LEAF * (groups / 2);
  std::nth_element(idx.begin() + a, idx.begin() + mid, idx.begin() + b, [&](int32_t x, int32_t y) {
    return cen[3 * x + axis] < cen[3 * y + axis] || (cen[3 * x + axis] == cen[3 * y + axis] && x < y);
  });
  tri_spatial_order(idx, a, mid, cen);
  tri_spatial_order(idx, mid, b, cen);
}

// Triangle BVH of a non-small scene (rfx_types.h RFX_TRI_BVH).  The triangles with a well-conditioned basis
// (cond < 300: their reported hits lie within the cull margin of their vertices, see the bounds in
// SceneBuild below) are put in spatial order -- recursive median splits of the centroids along their longest
// axis, left parts a multiple of the leaf size -- so every aligned run of RFX_TRI_BVH_LEAF is a compact leaf; the
// leaves' vertex boxes then take the pair builder above (SAH within its depth budget).  Every other triangle
// (cond >= 300, a singular basis) goes to the residual list.  The scene's arrays are not reordered: order[] lists
// insertion indices, leaf g = order[RFX_TRI_BVH_LEAF g ..], -1 padding the last leaf (TriTree, rfx_scene.h).
// false: no tree (fewer than two leaves, deeper than the kernel's stack, or more nodes / leaves than an int16 stack
// slot holds) -- the kernels keep their 64-triangle chunk loops
bool build_tri_tree(const std::vector<HostTri> &tris, const double *ref, bool widen, TriTree &T)
{
  T = TriTree{};
  std::vector<int32_t> idx;
  for (size_t i = 0; i < tris.size(); ++i)
    (tris[i].cond < 300.0 ? idx : T.resid).push_back((int32_t)i);
  const size_t nleaf = (idx.size() + RFX_TRI_BVH_LEAF - 1) / RFX_TRI_BVH_LEAF;
  if (nleaf < 2 || nleaf > 32768) { T.resid.clear(); return false; }
  std::vector<double> cen(3 * tris.size(), 0.0);
  for (int32_t i : idx)
  {
    const HostTri &t = tris[i];
    cen[3 * i] = ((double)t.v0.x + t.v1.x + t.v2.x) / 3.0;
    cen[3 * i + 1] = ((double)t.v0.y + t.v1.y + t.v2.y) / 3.0;
    cen[3 * i + 2] = ((double)t.v0.z + t.v1.z + t.v2.z) / 3.0;
  }
  tri_spatial_order(idx, 0, idx.size(), cen);
  T.order.assign(nleaf * RFX_TRI_BVH_LEAF, -1);
  std::copy(idx.begin(), idx.end(), T.order.begin());
  std::vector<PairBox> box(nleaf);
  for (size_t g = 0; g < nleaf; ++g)
  {
    PairBox &b = box[g];
    for (int k = 0; k < 3; ++k) { b.lo[k] = INFINITY; b.hi[k] = -INFINITY; }
    for (int e = 0; e < RFX_TRI_BVH_LEAF; ++e)
    {
      const int32_t i = T.order[RFX_TRI_BVH_LEAF * g + e];
      if (i < 0) continue;
      for (const v3 &q : {tris[i].v0, tris[i].v1, tris[i].v2})
      {
        const double c[3] = {q.x, q.y, q.z};
        for (int k = 0; k < 3; ++k) { b.lo[k] = fmin(b.lo[k], c[k]); b.hi[k] = fmax(b.hi[k], c[k]); }
      }
    }
    for (int k = 0; k < 3; ++k) b.c[k] = 0.5 * (b.lo[k] + b.hi[k]);
  }
  std::vector<uint32_t> leaves(nleaf);
  for (size_t g = 0; g < nleaf; ++g) leaves[g] = (uint32_t)g;
  build_pair_bvh(T.nodes, leaves, 0, nleaf, box, ref, 0, T.depth, widen);
  if (T.depth > kBvhStack || T.nodes.size() > 32767) { T = TriTree{}; return false; }
  return true;
}
}  // namespace

// the margin reference point both trees measure from: the sphere BVH's root box centre, or -- no sphere BVH (at most
// 32 spheres) -- the centre of the triangles' vertex box
static void tri_ref_point(const std::vector<HostTri> &tris, double *ref)
{
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (const HostTri &t : tris)
  {
    if (!(t.cond < 300.0)) continue;
    for (const v3 &q : {t.v0, t.v1, t.v2})
    {
      const double c[3] = {q.x, q.y, q.z};
      for (int k = 0; k < 3; ++k) { lo[k] = fmin(lo[k], c[k]); hi[k] = fmax(hi[k], c[k]); }
    }
  }
  for (int k = 0; k < 3; ++k) ref[k] = lo[k] <= hi[k] ? (double)(float)(0.5 * (lo[k] + hi[k])) : 0.0;
}

// The nodes of a tree by height (a leaf's is 0), lowest first: hlist[hoff[h - 1] .. hoff[h]) are the nodes of height
// h >= 1, each above both its children.  child: nodes x 2, children after their parent (build_pair_bvh's node order and
// cut_topology's pre-order), so one backward pass has every child's height.
static void height_lists(const std::vector<int32_t> &child, std::vector<int32_t> &hlist, std::vector<uint32_t> &hoff)
{
  const size_t n = child.size() / 2;
  std::vector<int> height(n, 0);
  for (size_t i = n; i-- > 0;)
    for (int c = 0; c < 2; ++c) height[i] = std::max(height[i], 1 + (child[2 * i + c] >= 0 ? height[child[2 * i + c]] : 0));
  hlist.clear();
  hoff.assign(1, 0u);
  for (int h = 1; hlist.size() < n; ++h)
  {
    for (size_t i = 0; i < n; ++i)
      if (height[i] == h) hlist.push_back((int32_t)i);
    hoff.push_back((uint32_t)hlist.size());
  }
}

static int cut_node(std::vector<int32_t> &child, size_t a, size_t b, int level, int &depth)
{
  if (b - a == 1) return ~(int)a;
  depth = std::max(depth, level + 1);
  const size_t id = child.size() / 2, mid = a + (b - a) / 2;
  child.resize(child.size() + 2);
  const int l = cut_node(child, a, mid, level + 1, depth), r = cut_node(child, mid, b, level + 1, depth);
  child[2 * id] = l;
  child[2 * id + 1] = r;
  return (int)id;
}

CutTopology rfx::cut_topology(size_t leaves)
{
  CutTopology c;
  if (leaves < 2) return c;
  cut_node(c.child, 0, leaves, 0, c.depth);
  height_lists(c.child, c.hlist, c.hoff);
  return c;
}

extern "C" int rfx_scene_tri_bvh_dump(const rfx_scene *s, int32_t counts[5], float *boxes, int32_t *children,
                                      int32_t *leaf_ids, int32_t *residual)
{
  if (!s || !counts) return fail(RFX_ERR_ARG, "tri_bvh_dump: bad args");
  for (int k = 0; k < 5; ++k) counts[k] = 0;
  counts[3] = RFX_TRI_BVH_LEAF;
  if (s->spheres.size() <= 32 && s->tris.size() <= 32) return 0;  // a small scene: no tree
  TriTree T;
  double ref[3];
  tri_ref_point(s->tris, ref);
  if (!build_tri_tree(s->tris, ref, false, T)) return 0;
  counts[0] = (int32_t)T.nodes.size();
  counts[1] = (int32_t)T.leaves();
  counts[2] = (int32_t)T.resid.size();
  counts[4] = T.depth;
  for (size_t i = 0; i < T.nodes.size(); ++i)
  {
    const BvhNode &n = T.nodes[i];
    if (boxes)
      for (int c = 0; c < 2; ++c)
      {
        float *b = boxes + 12 * i + 6 * c;
        b[0] = n.lx[c]; b[1] = n.ly[c]; b[2] = n.lz[c]; b[3] = n.hx[c]; b[4] = n.hy[c]; b[5] = n.hz[c];
      }
    if (children) { children[2 * i] = n.child[0]; children[2 * i + 1] = n.child[1]; }
  }
  if (leaf_ids) std::copy(T.order.begin(), T.order.end(), leaf_ids);
  if (residual) std::copy(T.resid.begin(), T.resid.end(), residual);
  return 1;
}

// ============================================================== coplanar mates
// Triangle::trace (Triangle.cpp:53-108) starts with the z row of axTrans (o - v0) and of axTrans ray:
//   aoz = (o.x - v0x) a31 + (o.y - v0y) a32 + (o.z - v0z) a33,   arz = ray.x a31 + ray.y a32 + ray.z a33,
// and everything up to t = -aoz / arz and `t > VERY_SMALL_NUMBER` is a function of those two and the ray (rfx_intersect.h
// tri_z).  Triangles A and B are mates iff (a31, a32, a33) are finite and bitwise equal in both, all six v0 components
// are finite, and on each axis i either v0_i is bitwise equal or a3i == 0.  Then for one ray:
//   arz has identical operands in both, so it is identical;
//   aoz differs only in the terms of the axes with a3i == 0: there d a3i is +-0 for a finite difference d (a zero term
//     leaves the float sum's value as it is, only the sign of a zero sum can change), and NaN in both for an infinite
//     or NaN o_i (o_i - v0_i is then the same infinity, or NaN, for any finite v0_i);
//   so aoz, arz and all that tri_z derives from them are equal as values, or NaN in both; every use is blind to the
//   sign of a zero (fabsf, compares with 0, nz nz, the quotient of non-zero operands).
// (A finite o_i whose difference from one v0_i overflows and from the other does not, |o_i| >= 2^127, is outside the rule.)
// The relation is an equivalence (equal keys below), a group's leader its lowest index.  Needs FP contraction off.
static std::vector<int32_t> tri_mate_leaders(const std::vector<HostTri> &tris, bool on)
{
  std::vector<int32_t> leader(tris.size());
  std::map<std::array<uint32_t, 6>, int32_t> first;
  for (size_t i = 0; i < tris.size(); ++i)
  {
    const HostTri &t = tris[i];
    leader[i] = (int32_t)i;
    const float row[3] = {t.ax.m31, t.ax.m32, t.ax.m33}, v0[3] = {t.v0.x, t.v0.y, t.v0.z};
    bool finite = on;
    std::array<uint32_t, 6> key{};
    for (int a = 0; a < 3; ++a)
    {
      finite = finite && std::isfinite(row[a]) && std::isfinite(v0[a]);
      memcpy(&key[a], &row[a], 4);
      if (row[a] != 0.0f) memcpy(&key[3 + a], &v0[a], 4);
    }
    if (finite) leader[i] = first.emplace(key, (int32_t)i).first->second;
  }
  return leader;
}

extern "C" int rfx_scene_set_tri_mates(rfx_scene *s, int on)
{
  if (!s || on < 0 || on > 1) return fail(RFX_ERR_ARG, "scene_set_tri_mates: 0 or 1");
  s->tri_mates = on;
  return RFX_OK;
}

extern "C" int rfx_scene_tri_mates(const rfx_scene *s, int32_t *leader, float *plane)
{
  if (!s) return fail(RFX_ERR_ARG, "scene_tri_mates: null scene");
  const std::vector<int32_t> l = tri_mate_leaders(s->tris, s->tri_mates != 0);
  if (leader) std::copy(l.begin(), l.end(), leader);
  if (plane)
    for (const HostTri &t : s->tris)
      for (float f : {t.v0.x, t.v0.y, t.v0.z, t.ax.m31, t.ax.m32, t.ax.m33}) *plane++ = f;
  return (int)l.size();
}

// ============================================================== far lights
// Scene::trace (Scene.cpp:117-181) forms dirToLight = light.origin - drop at every hit.  For a light L far from the
// scene that difference is L itself in float32: with s_i the spacing of floats just below |L_i| (half the spacing above
// it when |L_i| is a power of two), |d_i| < s_i / 2 puts L_i - d_i strictly nearer to L_i than to either neighbour, so
// it rounds to L_i -- the compare must be strict, at |d_i| = s_i / 2 the tie may round away.  near = min_i s_i / 2.
// With dtl == L every term of the light's shading that does not read the hit is a constant of the light: len(dtl),
// sqlen(dtl), ang = 1 - r^2 / sqlen, normalized(dtl), 1 - sqrt(ang).  They are computed here by rfx_math.h's own
// functions, whose host forms are the correctly rounded '/' and sqrtf the device forms reproduce bit for bit.
// A light is far when every field is finite, near > 0 (so no coordinate is zero: admitting such a light per axis would
// be sound, it is left out), sqlen(L) is finite and above kVerySmall, ang > 0, radius > kVerySmall -- the branches of
// the general form the kernel then takes without testing -- and radius / |L| * 1.001 < 0.5 as rfx_bundle.h
// make_bundle_ball asks of its direction ball.  The shadow rays' directions L + rd radius, |rd| <= 1, then lie in the
// cone of half-angle asin(radius / |L|) about normalized(L); cone_cos / cone_sin are that cone widened exactly as
// make_bundle_ball widens its own (ca = 1, sa = 0: the axis is the ball's centre).
// Returns the record with near > 0 for a far light, with the eight new fields 0 otherwise.
static LightRec far_light_terms(const HostLight &l)
{
  LightRec rec{l.origin.x, l.origin.y, l.origin.z, l.radius, l.r, l.g, l.b, l.power, 0, 0, 0, 0, 0, 0, 0, 0};
  const float c[3] = {l.origin.x, l.origin.y, l.origin.z};
  float near = INFINITY;
  for (int a = 0; a < 3; ++a)
  {
    if (!std::isfinite(c[a])) return rec;
    const float m = fabsf(c[a]);
    near = fminf(near, (m - nextafterf(m, 0.0f)) / 2);
  }
  if (!std::isfinite(l.radius) || !(near > 0.0f)) return rec;
  const v3 dtl = l.origin;
  const float aa = sqlen(dtl);
  if (!std::isfinite(aa) || !(aa > kVerySmall)) return rec;
  const float ang = 1.0f - qdiv(l.radius * l.radius, aa);
  if (!(ang > 0) || !(l.radius > kVerySmall)) return rec;
  const float dlen = len(dtl);
  const float sb = fminf(l.radius / dlen * 1.001f, 1.0f);
  if (!(sb < 0.5f)) return rec;
  const v3 nd = normalized(dtl);
  const float cb = sqrtf(fmaxf(1.0f - sb * sb, 0.0f));
  const float dev = fmaxf(1.0f - cb, 0.0f);
  rec.dlen = dlen;
  rec.ndx = nd.x; rec.ndy = nd.y; rec.ndz = nd.z;
  rec.spec_add = 1.0f - sqrt_rn(ang);
  rec.near = near;
  rec.cone_cos = 1.0f - dev - 4e-6f;
  rec.cone_sin = sqrtf(fmaxf(1.0f - rec.cone_cos * rec.cone_cos, 0.0f) + 1e-7f) * 1.001f;
  return rec;
}

// Whether the launches of this scene may take the far-light kernels (rfx_scene_set_far_lights): exactly one light, far,
// and under mode 1 every sphere (its box) and every triangle vertex inside |coordinate| < near.  The kernels guard every
// hit by the same bound, so the extent decides only whether they pay: a plane, a far eye or a rounding may still put a
// hit outside, and it then takes the general expressions.
static bool far_light_scene(const rfx_scene &s, const LightRec &rec)
{
  if (s.far_lights == 0 || s.lights.size() != 1 || !(rec.near > 0.0f)) return false;
  if (s.far_lights == 2) return true;
  const auto inside = [&](float v) { return fabsf(v) < rec.near; };  // false for a NaN
  for (const HostSphere &h : s.spheres)
    for (float v : {h.center.x - h.radius, h.center.x + h.radius, h.center.y - h.radius, h.center.y + h.radius,
                    h.center.z - h.radius, h.center.z + h.radius})
      if (!inside(v)) return false;
  for (const HostTri &t : s.tris)
    for (const v3 *v : {&t.v0, &t.v1, &t.v2})
      if (!inside(v->x) || !inside(v->y) || !inside(v->z)) return false;
  return true;
}

extern "C" int rfx_scene_set_far_lights(rfx_scene *s, int mode)
{
  if (!s || mode < 0 || mode > 2) return fail(RFX_ERR_ARG, "scene_set_far_lights: 0 (off), 1 (auto) or 2 (any extent)");
  s->far_lights = mode;
  return RFX_OK;
}

extern "C" int rfx_scene_far_light(const rfx_scene *s, int light, float terms[8])
{
  if (!s || light < 0 || light >= (int)s->lights.size()) return fail(RFX_ERR_ARG, "scene_far_light: no light %d", light);
  const LightRec rec = far_light_terms(s->lights[light]);
  if (terms)
    for (float f : {rec.dlen, rec.ndx, rec.ndy, rec.ndz, rec.spec_add, rec.near, rec.cone_cos, rec.cone_sin}) *terms++ = f;
  return far_light_scene(*s, rec) ? 1 : 0;
}

// ============================================================== a far light's occluder grid
// DESIGN.md "Shadow grid".  The shadow rays toward a far light are nearly parallel over the whole scene, so which objects
// one of them can meet depends almost only on where it starts.  The grid cuts a box around the scene into cubic cells
// and keeps, per cell, cull_small's verdict (rfx_cull_rule.h cull_record, the kernels' own rule) for the bundle of
// every shadow ray that starts inside the cell: origins within the cell's circumscribed ball, directions in the light's
// cone (LightRec cone_cos / cone_sin, which hold L + rd radius for every |rd| <= 1 and every hit inside the light's
// bound).  A wave whose facing hits all lie inside the bound and the box ORs its lanes' cell masks instead of culling
// its own bundle (rfx_bounce.h GRID).
//   box    every sphere's box and every triangle vertex, grown on every side by kGridBoxMargin of its longest edge (hits
//          lie on the objects up to rounding; a hit outside the box only sends its wave down the bundle path)
//   cells  the smallest size that keeps nx ny nz at or under RFX_SHADOW_GRID_CELLS, found by bisection and rounded up
//   ball   centre lo + (i + 1/2) size rounded to float, radius the half-diagonal (sqrt(3) / 2) size widened by a relative
//          1e-6 nmax + 1e-5 and by 2.5e-7 of the box's largest |coordinate|: the kernels find a point's cell in float32 --
//          (p - lo) * (1 / size), three roundings, at most 2^-22 n cells off on an axis of n cells, i.e. 4.8e-7 n of the
//          half size -- and the centre's own rounding is at most 2^-24 of a coordinate per axis
// The grid is built when the scene is small, has exactly one light, that light is far, RFX_SHADOW_GRID is not 0 and:
// mode 1, the scene's launches take the far-light kernels (far_light_scene); mode 2, always.
constexpr double kGridBoxMargin = 1.0 / 1024.0;

static bool shadow_grid_scene(const rfx_scene &s, const LightRec &rec, bool small)
{
  if (!RFX_SHADOW_GRID || s.shadow_grid == 0 || !small || s.lights.size() != 1 || !(rec.near > 0.0f)) return false;
  return s.shadow_grid == 2 || far_light_scene(s, rec);
}

static void shadow_grid_build(const rfx_scene &s, const LightRec &light, SceneBuild &B)
{
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  const auto take = [&](int a, double l, double h) { lo[a] = fmin(lo[a], l); hi[a] = fmax(hi[a], h); };
  for (const HostSphere &h : s.spheres)
  {
    const double c[3] = {h.center.x, h.center.y, h.center.z};
    for (int a = 0; a < 3; ++a) take(a, c[a] - h.radius, c[a] + h.radius);
  }
  for (const HostTri &t : s.tris)
    for (const v3 *v : {&t.v0, &t.v1, &t.v2}) { take(0, v->x, v->x); take(1, v->y, v->y); take(2, v->z, v->z); }
  double edge = 0.0;
  for (int a = 0; a < 3; ++a)
  {
    if (!std::isfinite(lo[a]) || !std::isfinite(hi[a])) return;  // no object, or a NaN or infinite one
    edge = fmax(edge, hi[a] - lo[a]);
  }
  if (!(edge > 0.0) || !(edge < 1.0e30)) return;
  float flo[3];
  double ext[3], cmax = 0.0;
  for (int a = 0; a < 3; ++a)
  {
    flo[a] = (float)(lo[a] - kGridBoxMargin * edge);
    if ((double)flo[a] > lo[a] - kGridBoxMargin * edge) flo[a] = nextafterf(flo[a], -INFINITY);
    ext[a] = hi[a] + kGridBoxMargin * edge - (double)flo[a];
  }
  const auto cells = [&](double size, int32_t n[3]) {
    double total = 1.0;
    for (int a = 0; a < 3; ++a)
    {
      const double c = fmax(1.0, ceil(ext[a] / size));
      n[a] = c < 1.0e9 ? (int32_t)c : 1000000000;
      total *= c;
    }
    return total;
  };
  const double budget = (double)RFX_SHADOW_GRID_CELLS;
  int32_t n[3];
  double fits = fmax(ext[0], fmax(ext[1], ext[2])), over = cbrt(ext[0] * ext[1] * ext[2] / budget) * 0.5;
  if (cells(over, n) <= budget) fits = over;  // (cannot be: nx ny nz >= volume / size^3)
  else
    for (int it = 0; it < 60; ++it)
    {
      const double mid = 0.5 * (fits + over);
      (cells(mid, n) <= budget ? fits : over) = mid;
    }
  float size = (float)fits;
  if ((double)size < fits) size = nextafterf(size, INFINITY);
  while (cells((double)size, n) > budget) size = nextafterf(size * 1.000001f, INFINITY);
  const float scale = 1.0f / size;
  if (!(size > 0.0f) || !std::isfinite(size) || !std::isfinite(scale) || !(scale > 0.0f)) return;
  for (int a = 0; a < 3; ++a) cmax = fmax(cmax, fmax(fabs((double)flo[a]), fabs((double)flo[a] + (double)n[a] * size)));
  const int32_t nmax = std::max(n[0], std::max(n[1], n[2]));
  const double ball = 0.5 * sqrt(3.0) * (double)size * (1.0 + 1.0e-6 * nmax + 1.0e-5) + 2.5e-7 * cmax;
  float rw = (float)ball;
  if ((double)rw < ball) rw = nextafterf(rw, INFINITY);
  Bundle cone{};
  cone.rw = rw;
  cone.ax = light.ndx; cone.ay = light.ndy; cone.az = light.ndz;
  cone.cosa = light.cone_cos; cone.sina = light.cone_sin;
  cone.ok = true;
  std::vector<int> lanes;
  for (int l = 0; l < 64; ++l)
    if ((B.d.cull_valid >> l) & 1u) lanes.push_back(l);
  B.gm.assign((size_t)n[0] * n[1] * n[2], 0ull);
  size_t k = 0;
  for (int32_t iz = 0; iz < n[2]; ++iz)
    for (int32_t iy = 0; iy < n[1]; ++iy)
      for (int32_t ix = 0; ix < n[0]; ++ix, ++k)
      {
        cone.cx = (float)((double)flo[0] + (ix + 0.5) * (double)size);
        cone.cy = (float)((double)flo[1] + (iy + 0.5) * (double)size);
        cone.cz = (float)((double)flo[2] + (iz + 0.5) * (double)size);
        uint64_t m = 0;
        for (int l : lanes)
          if (cull_record(B.cs[l], cone).keep) m |= 1ull << l;
        B.gm[k] = m;
      }
  ShadowGrid &g = B.d.shadow_grid;
  g.ox = flo[0]; g.oy = flo[1]; g.oz = flo[2];
  g.scale = scale;
  g.nx = n[0]; g.ny = n[1]; g.nz = n[2];
  g.fnx = (float)n[0]; g.fny = (float)n[1]; g.fnz = (float)n[2];
  B.grid_cell = size;
  B.grid_ball = rw;
}

extern "C" int rfx_scene_set_shadow_grid(rfx_scene *s, int mode)
{
  if (!s || mode < 0 || mode > 2) return fail(RFX_ERR_ARG, "scene_set_shadow_grid: 0 (off), 1 (auto) or 2 (any far light)");
  s->shadow_grid = mode;
  return RFX_OK;
}

extern "C" int rfx_scene_shadow_grid(const rfx_scene *s, float geom[6], int32_t dims[3], uint64_t *masks, uint64_t capacity)
{
  if (!s) return fail(RFX_ERR_ARG, "scene_shadow_grid: no scene");
  const SceneBuild B(*s, 0);
  const ShadowGrid &g = B.d.shadow_grid;
  if (geom)
    for (float f : {g.ox, g.oy, g.oz, g.scale, B.grid_cell, B.grid_ball}) *geom++ = f;
  if (dims)
    for (int32_t v : {g.nx, g.ny, g.nz}) *dims++ = v;
  if (masks)
  {
    if (capacity < B.gm.size()) return fail(RFX_ERR_ARG, "scene_shadow_grid: room for %zu masks needed", B.gm.size());
    if (!B.gm.empty()) memcpy(masks, B.gm.data(), B.gm.size() * sizeof(uint64_t));
  }
  return (int)B.gm.size();
}

// ============================================================== the device form of a scene
// The coherent order's key box (rfx.h "Coherent order"): float32 throughout, objects in insertion order, a NaN never
// taken; planes are unbounded and do not count
static OrderBox order_box_of(const rfx_scene &s)
{
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  const auto take = [&](int a, float l, float h) {
    if (l < lo[a]) lo[a] = l;
    if (h > hi[a]) hi[a] = h;
  };
  for (size_t k = 0; k < s.obj_kind.size(); ++k)
  {
    if (s.obj_kind[k] == 0)
    {
      const HostSphere &h = s.spheres[s.obj_idx[k]];
      const float c[3] = {h.center.x, h.center.y, h.center.z};
      for (int a = 0; a < 3; ++a) take(a, c[a] - h.radius, c[a] + h.radius);
    }
    else if (s.obj_kind[k] == 1)
    {
      const HostTri &t = s.tris[s.obj_idx[k]];
      for (const v3 *v : {&t.v0, &t.v1, &t.v2})
      {
        take(0, v->x, v->x);
        take(1, v->y, v->y);
        take(2, v->z, v->z);
      }
    }
  }
  OrderBox b{};
  for (int a = 0; a < 3; ++a)
  {
    const bool ok = hi[a] > lo[a] && std::isfinite(lo[a]) && std::isfinite(hi[a]);
    b.scale[a] = ok ? (float)(1u << RFX_ORDER_CELL_BITS) / (hi[a] - lo[a]) : 0.0f;
    b.lo[a] = std::isfinite(lo[a]) ? lo[a] : 0.0f;
  }
  return b;
}

SceneBuild::SceneBuild(const rfx_scene &scene, int tri_accel)
{
  const rfx_scene *s = &scene;
  order_box = order_box_of(scene);
  // Large scenes (more than 32 spheres): spheres in spatial order (spatial_order: recursive median splits),
  // so each 64-sphere chunk of the device arrays is compact and its bounding sphere can cull it as a whole,
  // and each pair is a BVH leaf.  Every record keeps its object index (sph_info),
  // and the large-scene kernel path compares (distance, object index), so the order changes no result.
  const size_t nsph = s->spheres.size();
  std::vector<uint32_t> order(nsph);
  for (size_t i = 0; i < nsph; ++i) order[i] = (uint32_t)i;
  if (nsph > 32) spatial_order(order, 0, nsph, s->spheres);

  for (uint32_t oi : order)
  {
    const HostSphere &hs = s->spheres[oi];
    sg.push_back({hs.center.x, hs.center.y, hs.center.z, hs.sq_radius});
    sm.push_back({hs.mat.r, hs.mat.g, hs.mat.b, hs.mat.refl});
    si.push_back(hs.obj);
    si.push_back(hs.mat.dielectric);
  }
  // (large scenes: a whole number of BVH leaves of RFX_BVH_LEAF_PAIRS pairs; the padding pairs never hit)
  const size_t npair_dev = sg.size() > 32 ? ((sg.size() + 1) / 2 + RFX_BVH_LEAF_PAIRS - 1) / RFX_BVH_LEAF_PAIRS *
                                                RFX_BVH_LEAF_PAIRS
                                          : (sg.size() + 1) / 2;
  sp.assign(npair_dev, SpherePair{});
  for (size_t i = 0; i < 2 * sp.size(); ++i)
  {
    SpherePair &p = sp[i / 2];
    const int l = (int)(i & 1);
    const bool real = i < sg.size();
    p.cx[l] = real ? sg[i].cx : 0.0f;
    p.cy[l] = real ? sg[i].cy : 0.0f;
    p.cz[l] = real ? sg[i].cz : 0.0f;
    p.r2[l] = real ? sg[i].sq_radius : -INFINITY;
  }
  for (const HostTri &t : s->tris)
  {
    TriGeo g{};
    g.v0x = t.v0.x; g.v0y = t.v0.y; g.v0z = t.v0.z;
    g.a11 = t.ax.m11; g.a12 = t.ax.m12; g.a13 = t.ax.m13;
    g.a21 = t.ax.m21; g.a22 = t.ax.m22; g.a23 = t.ax.m23;
    g.a31 = t.ax.m31; g.a32 = t.ax.m32; g.a33 = t.ax.m33;
    tg.push_back(g);
    TriShade h{};
    h.nx = t.norm.x; h.ny = t.norm.y; h.nz = t.norm.z;
    h.tu0 = t.tu0; h.tv0 = t.tv0;
    h.t11 = t.tuv.m11; h.t12 = t.tuv.m12; h.t21 = t.tuv.m21; h.t22 = t.tuv.m22;
    h.tex = t.tex; h.dielectric = t.mat.dielectric; h.obj = t.obj;
    ts.push_back(h);
    tm.push_back({t.mat.r, t.mat.g, t.mat.b, t.mat.refl});
  }
  // the mate group's leader in the record's padding (the BVH leaf copies below overwrite theirs)
  const std::vector<int32_t> leader = tri_mate_leaders(s->tris, s->tri_mates != 0);
  for (size_t i = 0; i < tg.size(); ++i) memcpy(&tg[i].pad[0], &leader[i], 4);
  // bounding spheres for the wave-bundle cull: a sphere's own (radius grown by a relative 1e-5), a
  // triangle's centroid and farthest vertex; a triangle whose axTrans is ill-conditioned (the reference
  // falls back to the identity for a singular basis, Matrix33.cpp:58-79) may report hits far from its
  // vertices, so it gets r = +inf and is never culled
  for (uint32_t oi : order)
  {
    const HostSphere &hs = s->spheres[oi];
    bd.push_back(sphere_bound(hs.center.x, hs.center.y, hs.center.z, hs.radius));
  }
  // chunk bounds: 64 consecutive spheres of the device order, centred on their mean centre (rfx_refit.h, shared with the
  // device update)
  for (size_t first = 0; first < nsph; first += 64)
    cb.push_back(sphere_chunk_bound(&bd[first], (uint32_t)(std::min(nsph, first + 64) - first)));
  for (const HostTri &t : s->tris)
  {
    bd.push_back(tri_bound(t.v0, t.v1, t.v2, t.cond < 300.0));
  }
  // small-scene lane table (rfx_types.h CullRec)
  uint64_t cull_valid = 0;
  const bool small = s->spheres.size() <= 32 && s->tris.size() <= 32;
  if (small)
  {
    cs.assign(64, CullRec{});
    ct.assign(32, CullTri{});
    for (size_t i = 0; i < s->spheres.size(); ++i)
    {
      const int lane = (int)(i & 1u) * 16 + (int)(i >> 1);
      const Bound &b = bd[i];
      CullRec c{};
      c.x = b.x; c.y = b.y; c.z = b.z; c.r = b.r;
      cs[lane] = c;
      cull_valid |= 1ull << lane;
    }
    for (size_t i = 0; i < s->tris.size(); ++i)
    {
      const HostTri &t = s->tris[i];
      const Bound &b = bd[s->spheres.size() + i];
      CullRec c{};
      c.x = b.x; c.y = b.y; c.z = b.z; c.r = b.r;
      if (t.cond < 300.0)
      {
        // plane of the triangle in double: unit normal of (v1 - v0) x (v2 - v0), offset n . v0
        const double ax = (double)t.v1.x - t.v0.x, ay = (double)t.v1.y - t.v0.y, az = (double)t.v1.z - t.v0.z;
        const double bx = (double)t.v2.x - t.v0.x, by = (double)t.v2.y - t.v0.y, bz = (double)t.v2.z - t.v0.z;
        double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
        const double nl = sqrt(nx * nx + ny * ny + nz * nz);
        if (nl > 0.0)
        {
          nx /= nl; ny /= nl; nz /= nl;
          c.nx = (float)nx; c.ny = (float)ny; c.nz = (float)nz;
          c.d = (float)(nx * t.v0.x + ny * t.v0.y + nz * t.v0.z);
        }
      }
      cs[32 + i] = c;
      cull_valid |= 1ull << (32 + i);
      // footprint record (primary-bundle masks): the dual rows of the basis (A, B, C) = (v2 - v0, v1 - v0, n) in
      // double (the float inverse the reference computes differs by a relative ~cond eps, inside the test's
      // margins); only for well-conditioned triangles (cond < 100)
      CullTri q{};
      q.v0x = t.v0.x; q.v0y = t.v0.y; q.v0z = t.v0.z;
      q.nu = q.nv = q.nuv = INFINITY;
      if (t.cond < 100.0 && c.nx * c.nx + c.ny * c.ny + c.nz * c.nz > 0.5f)
      {
        const double A[3] = {(double)t.v2.x - t.v0.x, (double)t.v2.y - t.v0.y, (double)t.v2.z - t.v0.z};
        const double Bv[3] = {(double)t.v1.x - t.v0.x, (double)t.v1.y - t.v0.y, (double)t.v1.z - t.v0.z};
        const double Cv[3] = {c.nx, c.ny, c.nz};
        auto cross = [](const double *a, const double *b, double *o) {
          o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
        };
        double bc[3], ca[3];
        cross(Bv, Cv, bc);
        cross(Cv, A, ca);
        const double det = A[0] * bc[0] + A[1] * bc[1] + A[2] * bc[2];
        if (fabs(det) > 0.0)
        {
          const double gu[3] = {bc[0] / det, bc[1] / det, bc[2] / det}, gv[3] = {ca[0] / det, ca[1] / det, ca[2] / det};
          q.gux = (float)gu[0]; q.guy = (float)gu[1]; q.guz = (float)gu[2];
          q.gvx = (float)gv[0]; q.gvy = (float)gv[1]; q.gvz = (float)gv[2];
          q.nu = (float)(sqrt(gu[0] * gu[0] + gu[1] * gu[1] + gu[2] * gu[2]) * 1.001);
          q.nv = (float)(sqrt(gv[0] * gv[0] + gv[1] * gv[1] + gv[2] * gv[2]) * 1.001);
          const double s0 = gu[0] + gv[0], s1 = gu[1] + gv[1], s2 = gu[2] + gv[2];
          q.nuv = (float)(sqrt(s0 * s0 + s1 * s1 + s2 * s2) * 1.001);
        }
      }
      ct[i] = q;
    }
  }
  // pair BVH (large scenes; spheres of a pair whose second slot is padding: r2 = -inf, never hit)
  int bvh_depth = 0;
  double bvh_ref[3] = {0.0, 0.0, 0.0};
  if (nsph > 32) bvh_depth = sphere_bvh(bd, nsph, true, bvh, bvh_ref);
  // triangle BVH (rfx_types.h RFX_TRI_BVH), when rfx_renderer_set_tri_accel asks for it: the nodes, the leaves' copy
  // of the triangle records and the residual list
  const bool want_tri = RFX_TRI_BVH && !small &&
                        (tri_accel >= 1 || (tri_accel < 0 && s->tris.size() >= (size_t)RFX_TRI_BVH_AUTO_MIN));
  if (want_tri)
  {
    if (nsph <= 32) tri_ref_point(s->tris, bvh_ref);
    if (build_tri_tree(s->tris, bvh_ref, true, tt))
    {
      tleaf.assign(tt.order.size(), TriGeo{});
      for (size_t q = 0; q < tt.order.size(); ++q)
      {
        const int32_t i = tt.order[q];
        if (i < 0) continue;  // padding: all zero, never hit
        tleaf[q] = tg[i];
        const int32_t obj = s->tris[i].obj;
        memcpy(&tleaf[q].pad[0], &i, 4);
        memcpy(&tleaf[q].pad[1], &obj, 4);
      }
    }
  }
  // the device update's tables (rfx_scene.h)
  if (!small && !s->tris.empty())
  {
    tslot.assign(s->tris.size(), -1);
    for (size_t q = 0; q < tt.order.size(); ++q)
      if (tt.order[q] >= 0) tslot[tt.order[q]] = (int32_t)q;
    for (const HostTri &t : s->tris)
    {
      for (const v3 *v : {&t.v0, &t.v1, &t.v2}) { tverts.push_back(v->x); tverts.push_back(v->y); tverts.push_back(v->z); }
      till.push_back(t.cond < 300.0 ? 0u : 1u);
    }
    std::vector<int32_t> child;
    for (const BvhNode &n : tt.nodes) { child.push_back(n.child[0]); child.push_back(n.child[1]); }
    height_lists(child, hlist, hoff);
    // the re-cut's tables: a binary tree over G leaves has G - 1 nodes whatever its splits, so the cut's nodes take the
    // built tree's array one for one (were that ever not so, the scene has no re-cut: RFX_ERR_STATE)
    if (!tt.nodes.empty() && tt.nodes.size() + 1 == tt.leaves())
    {
      for (size_t i = 0; i < s->tris.size(); ++i)
        if (tslot[i] >= 0) tin.push_back((uint32_t)i);
      cut = cut_topology(tt.leaves());
    }
  }
  // ... and the sphere update's (rfx.h "Moving spheres"): insertion index -> device index, the pair tree's nodes by height
  small_scene = small;
  sslot.assign(nsph, 0u);
  for (size_t di = 0; di < nsph; ++di) sslot[order[di]] = (uint32_t)di;
  {
    std::vector<int32_t> child;
    for (const BvhNode &n : bvh) { child.push_back(n.child[0]); child.push_back(n.child[1]); }
    height_lists(child, shlist, shoff);
  }
  for (const HostPlane &p : s->planes)
  {
    pg.push_back({p.pos.x, p.pos.y, p.pos.z, p.norm.x, p.norm.y, p.norm.z, p.obj, p.mat.dielectric});
    pm.push_back({p.mat.r, p.mat.g, p.mat.b, p.mat.refl});
  }
  // object index -> (kind, index in the device arrays): spheres through their spatial order
  loc.assign(s->obj_kind.size(), 0);
  {
    for (size_t o = 0; o < loc.size(); ++o)
    {
      const int kind = s->obj_kind[o], idx = s->obj_idx[o];
      loc[o] = kind << 28 | (kind == 0 ? (int32_t)sslot[idx] : idx);
    }
  }
  for (const HostLight &l : s->lights) lr.push_back(far_light_terms(l));
  d.far_light = !lr.empty() && far_light_scene(*s, lr[0]);
  for (const HostTexture &t : s->textures)
  {
    const bool empty = t.texels.empty();  // the reference's empty colorBuf: checker (Texture.cpp:242-243)
    tr.push_back({(uint32_t)pool.size(), empty ? 0u : t.w, empty ? 0u : t.h, 0});
    pool.insert(pool.end(), t.texels.begin(), t.texels.end());
  }
  d.n_tri_resid = (int32_t)tt.resid.size();
  d.n_tri_bvh = (int32_t)tt.nodes.size();
  d.tri_bvh_depth = tt.depth;
  accel.tri_nodes = d.n_tri_bvh;
  accel.tri_depth = tt.depth;
  accel.tri_leaf_size = RFX_TRI_BVH_LEAF;
  accel.tri_in_leaves = tt.nodes.empty() ? 0 : (int32_t)(s->tris.size() - tt.resid.size());
  accel.tri_residual = d.n_tri_resid;
  accel.sph_nodes = (int32_t)bvh.size();
  accel.sph_depth = bvh_depth;
  d.tri_bvh_narrow = !tt.nodes.empty() && (tri_accel == 2 || s->tris.size() >= (size_t)RFX_TRI_BVH_NARROW_MIN);
  accel.narrow_tri_bvh = d.tri_bvh_narrow;
  {
    // the bounce kernel's LDS copy of the node links and margin terms (rfx_types.h DevScene::bvh_aux): mt rounded up
    // to a multiple of mstep (one step more than the ceiling, so the float decode stays above)
    float mt_max = 0.0f;
    for (const BvhNode &n : bvh) mt_max = fmaxf(mt_max, fmaxf(n.mt[0], n.mt[1]));
    const float mstep = mt_max > 0.0f ? mt_max / 65000.0f : 1.0f;
    aux.assign(2 * bvh.size(), 0u);
    for (size_t i = 0; i < bvh.size(); ++i)
    {
      const BvhNode &n = bvh[i];
      uint32_t q[2];
      for (int c = 0; c < 2; ++c) q[c] = (uint32_t)std::min(65535.0, ceil((double)n.mt[c] / mstep) + 1.0);
      aux[2 * i] = ((uint32_t)(uint16_t)(int16_t)n.child[0]) | ((uint32_t)(uint16_t)(int16_t)n.child[1] << 16);
      aux[2 * i + 1] = q[0] | q[1] << 16;
    }
    d.bvh_mstep = mstep;
    d.n_bvh = (int32_t)bvh.size();
  }
  d.n_sph = (int32_t)sg.size();
  d.n_tri = (int32_t)tg.size();
  d.n_light = (int32_t)lr.size();
  d.n_chunk = (int32_t)cb.size();
  d.n_pln = (int32_t)pg.size();
  d.n_tex = (int32_t)tr.size();
  d.bvh_depth = bvh_depth;
  d.bvh_rx = (float)bvh_ref[0]; d.bvh_ry = (float)bvh_ref[1]; d.bvh_rz = (float)bvh_ref[2];
  if (!bvh.empty())  // regroup sort keys: 8 origin cells per axis over the root box
  {
    const BvhNode &root = bvh[0];
    const float lo[3] = {fminf(root.lx[0], root.lx[1]), fminf(root.ly[0], root.ly[1]), fminf(root.lz[0], root.lz[1])};
    const float hi[3] = {fmaxf(root.hx[0], root.hx[1]), fmaxf(root.hy[0], root.hy[1]), fmaxf(root.hz[0], root.hz[1])};
    float s[3];
    for (int k = 0; k < 3; ++k) s[k] = hi[k] > lo[k] ? 8.0f / (hi[k] - lo[k]) : 0.0f;
    d.key_lx = lo[0]; d.key_ly = lo[1]; d.key_lz = lo[2];
    d.key_sx = s[0]; d.key_sy = s[1]; d.key_sz = s[2];
  }
  d.n_obj = (int32_t)loc.size();
  d.cull_valid = cull_valid;
  d.skybox_tex = s->skybox;
  const col amb = cscale(s->diff, s->diff_power);                                    // Scene.cpp:186 (first factor)
  d.amb_r = amb.r; d.amb_g = amb.g; d.amb_b = amb.b;
  d.env_r = s->env.r; d.env_g = s->env.g; d.env_b = s->env.b;
  d.half_tile_w = s->half_tile_w;
  d.half_tile_h = s->half_tile_h;
  if (!lr.empty() && shadow_grid_scene(*s, lr[0], small)) shadow_grid_build(*s, lr[0], *this);
}

// The small-scene cull records as SceneBuild makes them (host only, for the tests of the bundle culls): the 64 lane
// records (rfx_types.h CullRec, 8 floats each), the 32 footprint records (CullTri, 12 floats each), the valid lanes.
extern "C" int rfx_scene_cull_dump(const rfx_scene *s, float recs[64 * 8], float tris[32 * 12], uint64_t *valid)
{
  if (!s) return fail(RFX_ERR_ARG, "scene_cull_dump: no scene");
  if (!(s->spheres.size() <= 32 && s->tris.size() <= 32))
    return fail(RFX_ERR_STATE, "scene_cull_dump: not a small scene (more than 32 spheres or triangles)");
  const SceneBuild B(*s, 0);
  static_assert(sizeof(CullRec) == 8 * sizeof(float) && sizeof(CullTri) == 12 * sizeof(float), "dump layout");
  if (recs) memcpy(recs, B.cs.data(), 64 * sizeof(CullRec));
  if (tris) memcpy(tris, B.ct.data(), 32 * sizeof(CullTri));
  if (valid) *valid = B.d.cull_valid;
  return RFX_OK;
}

// ============================================================== moving meshes (host side)
// rfx.h "Moving meshes".  The device side is rfx_update.cpp / rfx_update_kernels.hip; both take every formula from rfx_refit.h.
extern "C" int rfx_scene_set_triangle_vertices(rfx_scene *s, uint32_t first, uint32_t count, const float *vertices9)
{
  if (!s || !vertices9 || !count || (uint64_t)first + count > s->tris.size())
    return fail(RFX_ERR_ARG, "scene_set_triangle_vertices: a scene, vertices and a range within its %zu triangles",
                s ? s->tris.size() : (size_t)0);
  for (uint32_t i = 0; i < count; ++i)
  {
    const float *v = vertices9 + 9 * (size_t)i;
    set_tri_vertices(s->tris[first + i], v, v + 3, v + 6);
  }
  return RFX_OK;
}

extern "C" int rfx_scene_object_triangle(const rfx_scene *s, int obj)
{
  if (!s || obj < 0 || obj >= (int)s->obj_kind.size() || s->obj_kind[obj] != 1)
    return fail(RFX_ERR_ARG, "scene_object_triangle: object %d is not a triangle", obj);
  return s->obj_idx[obj];
}

void rfx::tri_record_words(uint32_t *out, const TriGeo &g, const TriShade &h, const Bound &b, const float *verts9,
                           bool well, const TriGeo *leaf)
{
  static_assert(kTriRecordWords == 41, "record layout");
  memcpy(out, &g, 48);
  memcpy(out + 12, &h.nx, 12);
  memcpy(out + 15, &b, 16);
  memcpy(out + 19, verts9, 36);
  out[28] = well ? 1u : 0u;
  memcpy(out + 29, leaf ? leaf : &g, 48);
  for (int k = 0; k < kTriRecordWords; ++k)
    if ((out[k] & 0x7FFFFFFFu) > 0x7F800000u) out[k] = 0x7FC00000u;  // a NaN's sign and payload carry nothing
}

extern "C" int rfx_scene_tri_records(const rfx_scene *s, uint32_t first, uint32_t count, uint32_t *out)
{
  if (!s || !out || !count || (uint64_t)first + count > s->tris.size())
    return fail(RFX_ERR_ARG, "scene_tri_records: a scene, an output and a range within its %zu triangles",
                s ? s->tris.size() : (size_t)0);
  for (uint32_t i = 0; i < count; ++i)
  {
    const HostTri &t = s->tris[first + i];
    const float v[9] = {t.v0.x, t.v0.y, t.v0.z, t.v1.x, t.v1.y, t.v1.z, t.v2.x, t.v2.y, t.v2.z};
    TriSetup u{};
    u.v0 = t.v0; u.ax = t.ax;
    TriGeo g{};
    tri_geo_set(g, u);
    TriShade h{};
    h.nx = t.norm.x; h.ny = t.norm.y; h.nz = t.norm.z;
    tri_record_words(out + (size_t)kTriRecordWords * i, g, h, tri_bound(t.v0, t.v1, t.v2, t.cond < 300.0), v,
                     t.cond < 300.0, nullptr);
  }
  return RFX_OK;
}

namespace {
// the unwidened box below child c of the tree, writing every node's children on the way (rfx_refit.h refit_child)
RefitBox refit_below(std::vector<BvhNode> &nodes, int c, const std::vector<RefitBox> &leaf, const double *ref, bool widen)
{
  if (c < 0) return leaf[~c];
  RefitBox b;
  refit_box_empty(b);
  for (int k = 0; k < 2; ++k)
  {
    const RefitBox kid = refit_below(nodes, nodes[c].child[k], leaf, ref, widen);
    refit_child(nodes[c], k, kid, ref, widen);
    refit_box_join(b, kid);
  }
  return b;
}
}  // namespace

// every box of the tree `nodes` over the leaves order[RFX_TRI_BVH_LEAF g ..] from the vertices given, classed there
static void refit_tree(std::vector<BvhNode> &nodes, const std::vector<int32_t> &order, const float *vertices9_all,
                       const double *ref, bool widen)
{
  std::vector<RefitBox> leaf(order.size() / RFX_TRI_BVH_LEAF);
  for (size_t g = 0; g < leaf.size(); ++g)
  {
    refit_box_empty(leaf[g]);
    for (int e = 0; e < RFX_TRI_BVH_LEAF; ++e)
    {
      const int32_t i = order[RFX_TRI_BVH_LEAF * g + e];
      if (i < 0) continue;
      const float *v = vertices9_all + 9 * (size_t)i;
      for (int q = 0; q < 3; ++q) refit_box_vertex(leaf[g], v + 3 * q);
      if (!tri_well(tri_setup(mk(v[0], v[1], v[2]), mk(v[3], v[4], v[5]), mk(v[6], v[7], v[8])))) leaf[g].ill = 1;
    }
  }
  refit_below(nodes, 0, leaf, ref, widen);
}

// the nodes' boxes in rfx_scene_tri_bvh_dump's layout and their margin terms; either may be null
static void report_nodes(const std::vector<BvhNode> &nodes, float *boxes, float *mt)
{
  for (size_t i = 0; i < nodes.size(); ++i)
  {
    const BvhNode &n = nodes[i];
    if (boxes)
      for (int c = 0; c < 2; ++c)
      {
        float *b = boxes + 12 * i + 6 * c;
        b[0] = n.lx[c]; b[1] = n.ly[c]; b[2] = n.lz[c]; b[3] = n.hx[c]; b[4] = n.hy[c]; b[5] = n.hz[c];
      }
    if (mt) { mt[2 * i] = n.mt[0]; mt[2 * i + 1] = n.mt[1]; }
  }
}

extern "C" int rfx_scene_tri_bvh_refit(const rfx_scene *built, const float *vertices9_all, int widen, float *boxes,
                                       float *mt)
{
  if (!built || !vertices9_all || widen < 0 || widen > 1) return fail(RFX_ERR_ARG, "scene_tri_bvh_refit: bad args");
  if (built->spheres.size() <= 32 && built->tris.size() <= 32) return 0;  // a small scene: no tree
  SceneBuild B(*built, 1);
  TriTree &T = B.tt;
  if (T.nodes.empty()) return 0;
  const double ref[3] = {B.d.bvh_rx, B.d.bvh_ry, B.d.bvh_rz};
  refit_tree(T.nodes, T.order, vertices9_all, ref, widen != 0);
  report_nodes(T.nodes, boxes, mt);
  return 1;
}

// rfx.h "Re-cutting": the device re-cut's mirror.  The in-tree set, the residual list and the reference point are
// `built`'s; the order is the stable sort of the in-tree triangles by rfx_refit.h's key at cut_vertices9_all; the
// topology is cut_topology's; the boxes are the refit's at vertices9_all.
extern "C" int rfx_scene_tri_bvh_recut(const rfx_scene *built, const float *cut_vertices9_all, const float *vertices9_all,
                                       int widen, int32_t counts[5], float *boxes, int32_t *children, int32_t *leaf_ids,
                                       float *mt)
{
  if (!built || !cut_vertices9_all || !counts || widen < 0 || widen > 1)
    return fail(RFX_ERR_ARG, "scene_tri_bvh_recut: bad args");
  for (int k = 0; k < 5; ++k) counts[k] = 0;
  counts[3] = RFX_TRI_BVH_LEAF;
  if (built->spheres.size() <= 32 && built->tris.size() <= 32) return 0;  // a small scene: no tree
  SceneBuild B(*built, 1);
  if (B.tin.empty()) return 0;
  const size_t n = B.tin.size(), leaves = B.tt.leaves();
  // steps 1 and 2: the sums, the placed ones' box
  std::vector<float> sum(3 * n);
  std::vector<uint8_t> placed(n);
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (size_t j = 0; j < n; ++j)
  {
    const float *v = cut_vertices9_all + 9 * (size_t)B.tin[j];
    recut_sum(v, &sum[3 * j]);
    const bool well = tri_well(tri_setup(mk(v[0], v[1], v[2]), mk(v[3], v[4], v[5]), mk(v[6], v[7], v[8])));
    placed[j] = recut_placed(&sum[3 * j], well ? 0u : 1u);
    if (placed[j])
      for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], sum[3 * j + a]); hi[a] = fmaxf(hi[a], sum[3 * j + a]); }
  }
  // steps 3 and 4: the keys, the stable order (tin ascends, so equal keys keep ascending triangle indices)
  const float scale = recut_scale(lo, hi);
  std::vector<uint32_t> key(n), at(n);
  for (size_t j = 0; j < n; ++j)
  {
    key[j] = placed[j] ? recut_key(&sum[3 * j], lo, scale) : kRecutLastKey;
    at[j] = (uint32_t)j;
  }
  std::stable_sort(at.begin(), at.end(), [&](uint32_t x, uint32_t y) { return key[x] < key[y]; });
  std::vector<int32_t> order(leaves * RFX_TRI_BVH_LEAF, -1);
  for (size_t j = 0; j < n; ++j) order[j] = (int32_t)B.tin[at[j]];
  // step 5: the topology of the leaf count, in the built tree's node array, then the refit
  std::vector<BvhNode> nodes(B.cut.child.size() / 2);
  for (size_t i = 0; i < nodes.size(); ++i) { nodes[i].child[0] = B.cut.child[2 * i]; nodes[i].child[1] = B.cut.child[2 * i + 1]; }
  const double ref[3] = {B.d.bvh_rx, B.d.bvh_ry, B.d.bvh_rz};
  refit_tree(nodes, order, vertices9_all ? vertices9_all : cut_vertices9_all, ref, widen != 0);
  counts[0] = (int32_t)nodes.size();
  counts[1] = (int32_t)leaves;
  counts[2] = (int32_t)B.tt.resid.size();
  counts[4] = B.cut.depth;
  report_nodes(nodes, boxes, mt);
  if (children)
    for (size_t i = 0; i < nodes.size(); ++i) { children[2 * i] = nodes[i].child[0]; children[2 * i + 1] = nodes[i].child[1]; }
  if (leaf_ids) std::copy(order.begin(), order.end(), leaf_ids);
  return 1;
}

// ============================================================== moving spheres (host side)
// rfx.h "Moving spheres".  The device side is rfx_update.cpp / rfx_sphere_update_kernels.hip; both take every formula
// from rfx_refit.h.
extern "C" int rfx_scene_set_spheres(rfx_scene *s, uint32_t first, uint32_t count, const float *spheres4)
{
  if (!s || !spheres4 || !count || (uint64_t)first + count > s->spheres.size())
    return fail(RFX_ERR_ARG, "scene_set_spheres: a scene, spheres and a range within its %zu spheres",
                s ? s->spheres.size() : (size_t)0);
  for (uint32_t i = 0; i < count; ++i)
  {
    const float *v = spheres4 + 4 * (size_t)i;
    HostSphere &h = s->spheres[first + i];
    h.center = mk(v[0], v[1], v[2]);
    h.radius = sphere_radius(v[3]);
    h.sq_radius = h.radius * h.radius;                                               // Sphere.cpp:19
  }
  return RFX_OK;
}

extern "C" int rfx_scene_object_sphere(const rfx_scene *s, int obj)
{
  if (!s || obj < 0 || obj >= (int)s->obj_kind.size() || s->obj_kind[obj] != 0)
    return fail(RFX_ERR_ARG, "scene_object_sphere: object %d is not a sphere", obj);
  return s->obj_idx[obj];
}

void rfx::sph_record_words(uint32_t *out, const SphereGeo &g, const SpherePair &p, int lane, const Bound &b)
{
  static_assert(kSphRecordWords == 12, "record layout");
  const float w[12] = {g.cx, g.cy, g.cz, g.sq_radius, p.cx[lane], p.cy[lane], p.cz[lane], p.r2[lane], b.x, b.y, b.z, b.r};
  memcpy(out, w, sizeof(w));
  canonical_nans(out, kSphRecordWords);
}

extern "C" int rfx_scene_sph_records(const rfx_scene *s, uint32_t first, uint32_t count, uint32_t *out)
{
  if (!s || !out || !count || (uint64_t)first + count > s->spheres.size())
    return fail(RFX_ERR_ARG, "scene_sph_records: a scene, an output and a range within its %zu spheres",
                s ? s->spheres.size() : (size_t)0);
  for (uint32_t i = 0; i < count; ++i)
  {
    const HostSphere &h = s->spheres[first + i];
    const SphereGeo g{h.center.x, h.center.y, h.center.z, h.sq_radius};
    SpherePair p{};
    p.cx[0] = g.cx; p.cy[0] = g.cy; p.cz[0] = g.cz; p.r2[0] = g.sq_radius;
    sph_record_words(out + (size_t)kSphRecordWords * i, g, p, 0, sphere_bound(g.cx, g.cy, g.cz, h.radius));
  }
  return RFX_OK;
}

extern "C" int rfx_scene_sph_bvh_dump(const rfx_scene *s, int32_t counts[4], float *boxes, int32_t *children,
                                      int32_t *leaf_ids, uint32_t *device_index)
{
  if (!s || !counts) return fail(RFX_ERR_ARG, "sph_bvh_dump: bad args");
  for (int k = 0; k < 4; ++k) counts[k] = 0;
  counts[2] = (int32_t)kSphLeaf;
  const SceneBuild B(*s, 0);
  const size_t nsph = s->spheres.size();
  if (device_index) std::copy(B.sslot.begin(), B.sslot.end(), device_index);
  if (B.bvh.empty()) return 0;  // a small scene, at most 32 spheres, or a tree the walkers cannot take
  std::vector<BvhNode> nodes;
  double ref[3];
  const int depth = sphere_bvh(B.bd, nsph, false, nodes, ref);  // the boxes as built: the topology is the uploaded tree's
  const size_t leaves = nodes.size() + 1;
  counts[0] = (int32_t)nodes.size();
  counts[1] = (int32_t)leaves;
  counts[3] = depth;
  report_nodes(nodes, boxes, nullptr);
  if (boxes) canonical_nans(boxes, 12 * nodes.size());
  if (children)
    for (size_t i = 0; i < nodes.size(); ++i) { children[2 * i] = nodes[i].child[0]; children[2 * i + 1] = nodes[i].child[1]; }
  if (leaf_ids)
  {
    std::fill(leaf_ids, leaf_ids + leaves * kSphLeaf, -1);
    for (size_t i = 0; i < nsph; ++i) leaf_ids[B.sslot[i]] = (int32_t)i;
  }
  return 1;
}

namespace {
// the unwidened box below child c of the pair tree, writing every node's children on the way
SphBox sph_refit_below(std::vector<BvhNode> &nodes, int c, const std::vector<SphBox> &leaf, const double *ref, bool widen)
{
  if (c < 0) return leaf[~c];
  SphBox b;
  sph_box_empty(b);
  for (int k = 0; k < 2; ++k)
  {
    const SphBox kid = sph_refit_below(nodes, nodes[c].child[k], leaf, ref, widen);
    bvh_child_set(nodes[c], k, kid.lo, kid.hi, ref, widen);
    sph_box_join(b, kid);
  }
  return b;
}
}  // namespace

extern "C" int rfx_scene_sph_bvh_refit(const rfx_scene *built, const float *spheres4_all, int widen, float *boxes, float *mt,
                                       float *chunk_bounds)
{
  if (!built || !spheres4_all || widen < 0 || widen > 1) return fail(RFX_ERR_ARG, "scene_sph_bvh_refit: bad args");
  SceneBuild B(*built, 0);
  const size_t nsph = built->spheres.size();
  std::vector<Bound> bd(nsph);
  for (size_t i = 0; i < nsph; ++i)
  {
    const float *v = spheres4_all + 4 * i;
    bd[B.sslot[i]] = sphere_bound(v[0], v[1], v[2], sphere_radius(v[3]));
  }
  if (chunk_bounds)
    for (size_t first = 0; first < nsph; first += 64)
    {
      const Bound c = sphere_chunk_bound(&bd[first], (uint32_t)(std::min(nsph, first + 64) - first));
      memcpy(chunk_bounds + 4 * (first / 64), &c, sizeof(c));
      canonical_nans(chunk_bounds + 4 * (first / 64), 4);
    }
  if (B.bvh.empty()) return 0;
  std::vector<SphBox> leaf(B.bvh.size() + 1);
  for (size_t g = 0; g < leaf.size(); ++g) leaf[g] = sph_leaf_box(bd.data(), (uint32_t)g, (uint32_t)nsph);
  const double ref[3] = {B.d.bvh_rx, B.d.bvh_ry, B.d.bvh_rz};
  sph_refit_below(B.bvh, 0, leaf, ref, widen != 0);
  report_nodes(B.bvh, boxes, mt);
  if (boxes) canonical_nans(boxes, 12 * B.bvh.size());
  if (mt) canonical_nans(mt, 2 * B.bvh.size());
  return 1;
}
