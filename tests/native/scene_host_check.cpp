// Stand-alone check of the library's host-only unit (reflaxman_amd/csrc/rfx_scene.cpp): the rfx_scene_* builders, the
// TGA reader and writer, and SceneBuild (the host half of rfx_renderer_set_scene), compiled together with this file by
// a plain C++ compiler under the address and undefined-behaviour sanitizers (tests/test_scene_host.py).
// usage: scene_host_check <scratch directory>.  Exit status 0 and nothing on stderr: every check held.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "rfx_scene.h"

using namespace rfx;

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond))                                                         \
    {                                                                    \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                           \
    }                                                                    \
  } while (0)

static const float kWhite[3] = {1.0f, 1.0f, 1.0f};

// every child of every node: an internal node of the tree or the code ~g of one of its `leaves` leaves
static void check_children(const std::vector<BvhNode> &nodes, size_t leaves)
{
  for (const BvhNode &n : nodes)
    for (int c = 0; c < 2; ++c)
      CHECK(n.child[c] >= 0 ? (size_t)n.child[c] < nodes.size() : (size_t)~n.child[c] < leaves);
}

// (a) 3 spheres, 2 triangles (the second with three equal vertices), 1 plane, 2 lights, a 4x4 texture on triangle 0
static void small_scene()
{
  rfx_scene *s = rfx_scene_create(1.0f, 1.0f, 1.0f, 0.2f);
  for (int i = 0; i < 3; ++i)
  {
    const float c[3] = {2.0f * (float)i, 1.0f, 5.0f};
    CHECK(rfx_scene_add_sphere(s, c, 0.75f, RFX_METAL, kWhite, 0.5f, 0.0f) == i);
  }
  const float a[3] = {0, 0, 4}, b[3] = {1, 0, 4}, c[3] = {0, 1, 4};
  const int t0 = rfx_scene_add_triangle(s, a, b, c, RFX_METAL, kWhite, 0.1f, 0.0f);
  const int t1 = rfx_scene_add_triangle(s, b, b, b, RFX_DIELECTRIC, kWhite, 0.1f, 0.5f);
  CHECK(t0 == 3 && t1 == 4);
  const float pos[3] = {0, -1, 0}, up[3] = {0, 1, 0};
  CHECK(rfx_scene_add_plane(s, pos, up, RFX_METAL, kWhite, 0.0f, 0.0f) == 5);
  const float l0[3] = {0, 10, 0}, l1[3] = {5, 10, 0};
  CHECK(rfx_scene_add_light(s, l0, 1.0f, kWhite, 0.6f) == 0 && rfx_scene_add_light(s, l1, 0.5f, kWhite, 0.4f) == 1);
  uint32_t texels[16];
  for (uint32_t i = 0; i < 16; ++i) texels[i] = 0xFF000000u | i * 0x0F0F0Fu;
  const int tex = rfx_scene_add_texture_argb(s, 4, 4, texels);
  const float uv[6] = {0, 0, 1, 0, 0, 1};
  CHECK(tex == 0 && rfx_triangle_set_texture(s, t0, tex, uv) == RFX_OK);
  CHECK(rfx_triangle_set_texture(s, 0, tex, uv) == RFX_ERR_ARG);  // object 0 is a sphere

  const SceneBuild B(*s, -1);
  CHECK(B.d.n_sph == 3 && B.d.n_tri == 2 && B.d.n_pln == 1 && B.d.n_light == 2 && B.d.n_tex == 1 && B.d.n_obj == 6);
  CHECK(B.cs.size() == 64 && B.ct.size() == 32);
  uint64_t want = 0;
  for (int i = 0; i < 3; ++i) want |= 1ull << ((i & 1) * 16 + (i >> 1));
  for (int i = 0; i < 2; ++i) want |= 1ull << (32 + i);
  CHECK(B.d.cull_valid == want);
  CHECK(B.bd.size() == 5 && isfinite(B.bd[3].r) && isinf(B.bd[4].r) && B.bd[4].r > 0.0f);
  CHECK(isinf(B.cs[33].r) && isinf(B.ct[1].nu));  // the degenerate triangle: never culled, no footprint test
  CHECK(B.ts[0].tex == 0 && B.ts[1].tex == -1 && B.pool.size() == 16 && B.tr[0].w == 4 && B.tr[0].h == 4);
  CHECK(B.bvh.empty() && B.tt.nodes.empty() && B.d.n_bvh == 0 && B.accel.tri_nodes == 0);
  rfx_scene_destroy(s);
}

// (b) 300 spheres and 200 triangles from a fixed LCG in a 100-unit cube, 5 of the triangles one vertex three times
static void large_scene()
{
  uint32_t state = 12345u;
  auto unit = [&]() { state = state * 1664525u + 1013904223u; return (float)(state >> 8) / 16777216.0f; };
  rfx_scene *s = rfx_scene_create(1.0f, 1.0f, 1.0f, 0.2f);
  const int ns = 300, nt = 200;
  for (int i = 0; i < ns; ++i)
  {
    const float c[3] = {100.0f * unit(), 100.0f * unit(), 100.0f * unit()};
    CHECK(rfx_scene_add_sphere(s, c, 0.5f + 1.5f * unit(), RFX_METAL, kWhite, 0.5f, 0.0f) == i);
  }
  for (int i = 0; i < nt; ++i)
  {
    float v[9];
    for (float &x : v) x = 100.0f * unit();
    const bool singular = i % 40 == 7;  // 5 of them
    CHECK(rfx_scene_add_triangle(s, v, singular ? v : v + 3, singular ? v : v + 6, RFX_METAL, kWhite, 0.1f, 0.0f) == ns + i);
  }
  const float l0[3] = {50, 200, 50};
  rfx_scene_add_light(s, l0, 1.0f, kWhite, 0.6f);

  const SceneBuild B(*s, 1);
  CHECK(B.d.n_sph == ns && B.d.n_tri == nt && B.cs.empty() && B.ct.empty() && B.d.cull_valid == 0);
  // the device order of the spheres is a permutation of the insertion order
  std::set<int32_t> seen;
  for (int i = 0; i < ns; ++i) seen.insert(B.si[2 * i]);
  CHECK(B.si.size() == 2 * (size_t)ns && seen.size() == (size_t)ns && *seen.begin() == 0 && *seen.rbegin() == ns - 1);
  // the pair BVH
  CHECK(B.sp.size() % RFX_BVH_LEAF_PAIRS == 0 && 2 * B.sp.size() >= (size_t)ns);
  CHECK(!B.bvh.empty() && B.d.n_bvh == (int32_t)B.bvh.size() && B.aux.size() == 2 * B.bvh.size());
  CHECK(B.d.bvh_depth >= 1 && B.d.bvh_depth <= kBvhStack && B.accel.sph_depth == B.d.bvh_depth);
  check_children(B.bvh, B.sp.size() / RFX_BVH_LEAF_PAIRS);
  CHECK(B.cb.size() == (size_t)(ns + 63) / 64 && B.d.n_chunk == (int32_t)B.cb.size());
  // the triangle BVH: tree triangles and residual ones are the 200, each once; the singular ones are residual
  CHECK(!B.tt.nodes.empty() && B.d.n_tri_bvh == (int32_t)B.tt.nodes.size());
  CHECK(B.d.tri_bvh_depth >= 1 && B.d.tri_bvh_depth <= kBvhStack);
  check_children(B.tt.nodes, B.tt.leaves());
  std::vector<int> count(nt, 0);
  size_t in_tree = 0;
  CHECK(B.tleaf.size() == B.tt.order.size() && B.tt.order.size() % RFX_TRI_BVH_LEAF == 0);
  for (size_t q = 0; q < B.tt.order.size(); ++q)
  {
    const int32_t i = B.tt.order[q];
    if (i < 0) continue;
    CHECK(i < nt);
    int32_t idx, obj;
    memcpy(&idx, &B.tleaf[q].pad[0], 4);
    memcpy(&obj, &B.tleaf[q].pad[1], 4);
    CHECK(idx == i && obj == ns + i);
    ++count[i];
    ++in_tree;
  }
  for (int32_t i : B.tt.resid)
  {
    CHECK(i >= 0 && i < nt);
    ++count[i];
  }
  for (int i = 0; i < nt; ++i)
  {
    CHECK(count[i] == 1);
    if (i % 40 == 7) CHECK(isinf(B.bd[ns + i].r));
  }
  CHECK(in_tree + B.tt.resid.size() == (size_t)nt && B.tt.resid.size() >= 5);
  CHECK(B.d.n_tri_resid == (int32_t)B.tt.resid.size() && B.accel.tri_in_leaves == (int32_t)in_tree);
  for (int i = 7; i < nt; i += 40) CHECK(std::set<int32_t>(B.tt.resid.begin(), B.tt.resid.end()).count(i) == 1);
  // obj_loc maps every object back to its record
  CHECK(B.loc.size() == (size_t)(ns + nt) && B.d.n_obj == ns + nt);
  for (int o = 0; o < ns + nt; ++o)
  {
    const int kind = B.loc[o] >> 28, idx = B.loc[o] & ((1 << 28) - 1);
    if (o < ns) CHECK(kind == 0 && idx < ns && B.si[2 * idx] == o);
    else CHECK(kind == 1 && idx == o - ns && B.ts[idx].obj == o);
  }
  // the dump of the same tree, boxes as built
  int32_t counts[5];
  CHECK(rfx_scene_tri_bvh_dump(s, counts, nullptr, nullptr, nullptr, nullptr) == 1);
  CHECK(counts[0] == B.d.n_tri_bvh && counts[1] == (int32_t)B.tt.leaves() && counts[2] == B.d.n_tri_resid);
  rfx_scene_destroy(s);
}

static void write_file(const std::string &path, const std::vector<uint8_t> &bytes)
{
  FILE *f = fopen(path.c_str(), "wb");
  CHECK(f && fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size());
  fclose(f);
}

// (c) a 5x3 image through rfx_tga_save and rfx_tga_load, then malformed copies of the file
static void tga_files(const std::string &dir)
{
  uint32_t px[15], back[15] = {0};
  for (uint32_t i = 0; i < 15; ++i) px[i] = 0x80000000u | i << 16 | (255u - i) << 8 | 3u * i;
  const std::string good = dir + "/good.tga";
  CHECK(rfx_tga_save(good.c_str(), 5, 3, px) == RFX_OK);
  uint32_t w = 0, h = 0;
  CHECK(rfx_tga_load(good.c_str(), &w, &h, nullptr, 0) == RFX_OK && w == 5 && h == 3);
  CHECK(rfx_tga_load(good.c_str(), &w, &h, back, 14) == RFX_ERR_ARG);
  CHECK(rfx_tga_load(good.c_str(), &w, &h, back, 15) == RFX_OK && !memcmp(px, back, sizeof(px)));
  std::vector<uint8_t> file(18 + 60);
  FILE *f = fopen(good.c_str(), "rb");
  CHECK(f && fread(file.data(), 1, file.size(), f) == file.size() && fgetc(f) == EOF);
  fclose(f);

  std::vector<std::vector<uint8_t>> bad(4, file);
  bad[0].resize(20);      // the header and 2 bytes
  bad[1].resize(18 + 7);  // the header and 7 bytes
  bad[2][16] = 16;        // bpix
  bad[3][12] = 0xFF;      // xsize = -1
  bad[3][13] = 0xFF;
  rfx_scene *s = rfx_scene_create(1.0f, 1.0f, 1.0f, 0.2f);
  for (size_t i = 0; i < bad.size(); ++i)
  {
    const std::string path = dir + "/bad" + std::to_string(i) + ".tga";
    write_file(path, bad[i]);
    CHECK(rfx_tga_load(path.c_str(), &w, &h, back, 15) == RFX_ERR_IO && w == 0 && h == 0);
    int loaded = 1;
    CHECK(rfx_scene_add_texture_file(s, path.c_str(), &loaded) == (int)i && loaded == 0);
  }
  int loaded = 0;
  CHECK(rfx_scene_add_texture_file(s, good.c_str(), &loaded) == 4 && loaded == 1);
  CHECK(rfx_tga_load((dir + "/none.tga").c_str(), &w, &h, nullptr, 0) == RFX_ERR_IO);
  const SceneBuild B(*s, -1);
  CHECK(B.tr.size() == 5 && B.pool.size() == 15 && !memcmp(B.pool.data(), px, sizeof(px)));
  for (int i = 0; i < 4; ++i) CHECK(B.tr[i].w == 0 && B.tr[i].h == 0);  // left empty: the procedural checker
  CHECK(B.tr[4].offset == 0 && B.tr[4].w == 5 && B.tr[4].h == 3);
  rfx_scene_destroy(s);
}

// (d) nothing added
static void empty_scene()
{
  rfx_scene *s = rfx_scene_create(0.5f, 0.5f, 0.5f, 1.0f);
  for (int accel = -1; accel <= 2; ++accel)
  {
    const SceneBuild B(*s, accel);
    CHECK(B.d.n_sph == 0 && B.d.n_tri == 0 && B.d.n_pln == 0 && B.d.n_light == 0 && B.d.n_tex == 0 && B.d.n_obj == 0);
    CHECK(B.d.n_bvh == 0 && B.d.n_chunk == 0 && B.d.n_tri_bvh == 0 && B.d.n_tri_resid == 0 && B.d.cull_valid == 0);
    CHECK(B.sg.empty() && B.sp.empty() && B.tg.empty() && B.bd.empty() && B.bvh.empty() && B.loc.empty() && B.pool.empty());
    CHECK(B.d.skybox_tex == -1 && B.d.amb_r == 0.5f);
  }
  int ns = -1, nt = -1, nl = -1, nx = -1;
  CHECK(rfx_scene_counts(s, &ns, &nt, &nl, &nx) == RFX_OK && ns == 0 && nt == 0 && nl == 0 && nx == 0);
  rfx_scene_destroy(s);
}

int main(int argc, char **argv)
{
  if (argc != 2) { fprintf(stderr, "usage: scene_host_check <scratch directory>\n"); return 2; }
  small_scene();
  large_scene();
  tga_files(argv[1]);
  empty_scene();
  printf("scene_host_check: ok\n");
  return 0;
}
