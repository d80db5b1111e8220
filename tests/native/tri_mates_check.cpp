// Stand-alone check of the mate groups of reflaxman_amd/csrc/rfx_scene.cpp (tri_mate_leaders, rfx_scene_set_tri_mates,
// rfx_scene_tri_mates and the leader SceneBuild writes into TriGeo::pad[0]), compiled together with that file by a plain
// C++ compiler under the address and undefined-behaviour sanitizers (tests/test_tri_mates.py).
// Exit status 0 and nothing on stderr: every check held.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

static int add_tri(rfx_scene *s, float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz)
{
  const float a[3] = {ax, ay, az}, b[3] = {bx, by, bz}, c[3] = {cx, cy, cz};
  return rfx_scene_add_triangle(s, a, b, c, RFX_METAL, kWhite, 0.5f, 0.0f);
}

// the quad (x0, z0) - (x1, z1) at height y as two triangles
static void add_floor_quad(rfx_scene *s, float y, float x0, float z0, float x1, float z1)
{
  add_tri(s, x0, y, z0, x0, y, z1, x1, y, z0);
  add_tri(s, x0, y, z1, x1, y, z1, x1, y, z0);
}

static std::vector<int32_t> leaders(const rfx_scene *s, std::vector<float> *plane = nullptr)
{
  const int n = rfx_scene_tri_mates(s, nullptr, nullptr);
  CHECK(n >= 0);
  std::vector<int32_t> l((size_t)n, -7);
  if (plane) plane->assign(6 * (size_t)n, -7.0f);
  CHECK(rfx_scene_tri_mates(s, l.data(), plane ? plane->data() : nullptr) == n);
  return l;
}

static int32_t pad_int(const TriGeo &g)
{
  int32_t v;
  memcpy(&v, &g.pad[0], 4);
  return v;
}

// a small scene: two floor quads at one height with a tilted triangle between them, a quad at another height, and
// triangles with an infinite and a NaN vertex
static void small_scene()
{
  rfx_scene *s = rfx_scene_create(1.0f, 1.0f, 1.0f, 0.2f);
  add_floor_quad(s, 0.0f, -1.0f, -1.0f, 1.0f, 1.0f);               // 0 1
  add_tri(s, 0.0f, 1.0f, 0.0f, 1.0f, 1.5f, 0.25f, 0.0f, 2.0f, 1.0f); // 2
  add_floor_quad(s, 0.0f, 5.0f, 5.0f, 9.0f, 7.0f);                 // 3 4: the first quad's plane
  add_floor_quad(s, 2.0f, -1.0f, -1.0f, 1.0f, 1.0f);               // 5 6: another height
  add_tri(s, INFINITY, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f);  // 7
  add_tri(s, INFINITY, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f);  // 8
  add_tri(s, 0.0f, 0.0f, 0.0f, NAN, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f);       // 9
  std::vector<float> plane;
  std::vector<int32_t> l = leaders(s, &plane);
  CHECK(l.size() == 10 && plane.size() == 60);
  const int32_t want[9] = {0, 0, 2, 0, 0, 5, 5, 7, 8};
  for (int i = 0; i < 9; ++i) CHECK(l[i] == want[i]);
  CHECK(l[9] <= 9 && (l[9] == 9 || isfinite(plane[6 * 9 + 3])));
  CHECK(plane[0] == -1.0f && plane[1] == 0.0f && plane[2] == -1.0f && plane[3] == 0.0f && fabsf(plane[4]) == 1.0f);
  {
    const SceneBuild B(*s, -1);
    CHECK(B.tg.size() == 10);
    for (size_t i = 0; i < 10; ++i) CHECK(pad_int(B.tg[i]) == l[i]);
  }
  CHECK(rfx_scene_set_tri_mates(s, 2) == RFX_ERR_ARG && rfx_scene_set_tri_mates(nullptr, 1) == RFX_ERR_ARG);
  CHECK(rfx_scene_tri_mates(nullptr, nullptr, nullptr) == RFX_ERR_ARG);
  CHECK(rfx_scene_set_tri_mates(s, 0) == RFX_OK);
  l = leaders(s);
  for (int i = 0; i < 10; ++i) CHECK(l[i] == i);
  {
    const SceneBuild B(*s, -1);
    for (size_t i = 0; i < 10; ++i) CHECK(pad_int(B.tg[i]) == (int32_t)i);
  }
  CHECK(rfx_scene_set_tri_mates(s, 1) == RFX_OK && leaders(s)[4] == 0);
  rfx_scene_destroy(s);
}

// a scene with a triangle BVH: 40 x 25 floor quads of one plane (2000 triangles, one group); the leaf copies carry the
// insertion and object indices in their padding, the insertion-order records the leaders
static void large_scene()
{
  rfx_scene *s = rfx_scene_create(1.0f, 1.0f, 1.0f, 0.2f);
  for (int i = 0; i < 40; ++i)
    for (int j = 0; j < 25; ++j) add_floor_quad(s, 0.0f, (float)i, (float)j, (float)i + 1.0f, (float)j + 1.0f);
  const std::vector<int32_t> l = leaders(s);
  CHECK(l.size() == 2000);
  for (int32_t v : l) CHECK(v == 0);
  const SceneBuild B(*s, 1);
  CHECK(B.tg.size() == 2000 && !B.tt.nodes.empty() && B.tleaf.size() == B.tt.order.size());
  for (const TriGeo &g : B.tg) CHECK(pad_int(g) == 0);
  for (size_t q = 0; q < B.tt.order.size(); ++q)
    if (B.tt.order[q] >= 0) CHECK(pad_int(B.tleaf[q]) == B.tt.order[q]);
  rfx_scene_destroy(s);
}

static void empty_scene()
{
  rfx_scene *s = rfx_scene_create(0.5f, 0.5f, 0.5f, 1.0f);
  CHECK(rfx_scene_tri_mates(s, nullptr, nullptr) == 0 && leaders(s).empty());
  const SceneBuild B(*s, -1);
  CHECK(B.tg.empty());
  rfx_scene_destroy(s);
}

int main()
{
  small_scene();
  large_scene();
  empty_scene();
  printf("tri_mates_check: ok\n");
  return 0;
}
