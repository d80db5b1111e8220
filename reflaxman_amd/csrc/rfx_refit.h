// What follows a triangle's vertices, written once for the three places that compute it: the host scene builder
// (rfx_scene.cpp: rfx_scene_add_triangle, SceneBuild, build_pair_bvh), the host refit and re-cut (rfx_scene_tri_bvh_refit,
// rfx_scene_tri_bvh_recut) and the device update and re-cut (rfx_update_kernels.hip).  Float steps are rfx_math.h's (the reference's Triangle constructor, operation for
// operation); double steps are IEEE add, multiply, divide and sqrt, so with FP contraction off the device gives the
// host's words.  No HIP needed: a plain C++ compiler builds rfx_scene.cpp with this.
#pragma once
#include <math.h>

#include "rfx_math.h"
#include "rfx_types.h"

#pragma clang fp contract(off)

namespace rfx {

// A triangle is well-conditioned -- its reported hits lie within the cull margin of its vertices, so it may be culled by
// a bound and live in the tree -- when det is usable and cond = sqrt(|M|_F^2 |M^-1|_F^2) < 300.  kTriCondSq is the
// smallest double whose correctly rounded root is >= 300, so p < kTriCondSq <=> sqrt(p) < 300.0 for every double p (the
// root is monotone; NaN fails both): the device decides the class without a double root (tests/test_mesh_update_host.py
// checks the constant's two neighbours).
constexpr double kTriCondSq = 0x1.5f8ffffffffffp+16;

// Triangle.cpp:11-21 from the three vertices as rfx_scene_add_triangle takes them, and the builder's condition terms:
// p = |basis|_F^2 |axTrans|_F^2 in double, det_ok = the basis' float determinant is above kVerySmall
struct TriSetup {
  v3 v0, v1, v2, norm;
  m33 ax;
  double p;
  bool det_ok;
};
RFX_HD TriSetup tri_setup(v3 v0, v3 v1, v3 v2)
{
  TriSetup t;
  t.v0 = v0; t.v1 = v1; t.v2 = v2;
  t.norm = normalized(cross(sub(v1, v0), sub(v2, v0)));
  const m33 basis = from_cols(sub(v2, v0), sub(v1, v0), neg(t.norm));
  t.ax = inverted(basis);
  const float a[9] = {basis.m11, basis.m12, basis.m13, basis.m21, basis.m22, basis.m23, basis.m31, basis.m32, basis.m33};
  const float b[9] = {t.ax.m11, t.ax.m12, t.ax.m13, t.ax.m21, t.ax.m22, t.ax.m23, t.ax.m31, t.ax.m32, t.ax.m33};
  double na = 0.0, nb = 0.0;
  for (int k = 0; k < 9; ++k) { na += (double)a[k] * a[k]; nb += (double)b[k] * b[k]; }
  const float det = basis.m11 * (basis.m22 * basis.m33 - basis.m32 * basis.m23) +
                    basis.m21 * (basis.m32 * basis.m13 - basis.m12 * basis.m33) +
                    basis.m31 * (basis.m12 * basis.m23 - basis.m13 * basis.m22);
  t.p = na * nb;
  t.det_ok = fabsf(det) > kVerySmall;
  return t;
}
RFX_HD bool tri_well(const TriSetup &t) { return t.det_ok && t.p < kTriCondSq; }

// the geometry words of a tri_geo / tri_leaf record (its padding is the caller's)
RFX_HD void tri_geo_set(TriGeo &g, const TriSetup &t)
{
  g.v0x = t.v0.x; g.v0y = t.v0.y; g.v0z = t.v0.z;
  g.a11 = t.ax.m11; g.a12 = t.ax.m12; g.a13 = t.ax.m13;
  g.a21 = t.ax.m21; g.a22 = t.ax.m22; g.a23 = t.ax.m23;
  g.a31 = t.ax.m31; g.a32 = t.ax.m32; g.a33 = t.ax.m33;
}

// Bounding sphere of a triangle for the wave-bundle cull: the centroid and the farthest vertex in double; r = +inf for a
// triangle that is not well-conditioned (never culled)
RFX_HD Bound tri_bound(v3 v0, v3 v1, v3 v2, bool well)
{
  const double cx = ((double)v0.x + v1.x + v2.x) / 3.0, cy = ((double)v0.y + v1.y + v2.y) / 3.0,
               cz = ((double)v0.z + v1.z + v2.z) / 3.0;
  const v3 q[3] = {v0, v1, v2};
  double r2 = 0.0;
  for (int k = 0; k < 3; ++k)
    r2 = fmax(r2, (q[k].x - cx) * (q[k].x - cx) + (q[k].y - cy) * (q[k].y - cy) + (q[k].z - cz) * (q[k].z - cz));
  float r = (float)(sqrt(r2) * 1.0001 + 1e-6);
  if (!well) r = INFINITY;
  Bound b;
  b.x = (float)cx; b.y = (float)cy; b.z = (float)cz; b.r = r;
  return b;
}

// Child c of a hierarchy node from the union [l, h] of the unwidened boxes below it (build_pair_bvh).  widen: the box
// grown by the node part of the kernel's margin, kCullRel mt[c] (rfx_bundle.h kCullRel = 2e-3), from the float mt the
// kernel would have used, with a relative 1e-6 on top (false: rfx_scene_tri_bvh_dump, the boxes as built).  Then rounded
// outwards to float; mt[c]: the margin term of the child against the reference point ref (the root box centre), Euclidean
// |ref - centre|_2 + the half-diagonal (round 3; the L1 form made C5 2.2% slower), rounded up.
RFX_HD void bvh_child_set(BvhNode &n, int c, const double lo[3], const double hi[3], const double ref[3], bool widen)
{
  double l[3] = {lo[0], lo[1], lo[2]}, h[3] = {hi[0], hi[1], hi[2]};
  if (widen)
  {
    double cd = 0.0, hd = 0.0;
    for (int k = 0; k < 3; ++k)
    {
      const double dc = ref[k] - 0.5 * (l[k] + h[k]), dh = 0.5 * (h[k] - l[k]);
      cd += dc * dc;
      hd += dh * dh;
    }
    const double w = 2e-3 * (double)nextafterf((float)((sqrt(cd) + sqrt(hd)) * 1.0001), INFINITY) * (1.0 + 1e-6);
    for (int k = 0; k < 3; ++k) { l[k] -= w; h[k] += w; }
  }
  n.lx[c] = nextafterf((float)l[0], -INFINITY); n.ly[c] = nextafterf((float)l[1], -INFINITY);
  n.lz[c] = nextafterf((float)l[2], -INFINITY);
  n.hx[c] = nextafterf((float)h[0], INFINITY); n.hy[c] = nextafterf((float)h[1], INFINITY);
  n.hz[c] = nextafterf((float)h[2], INFINITY);
  double cd = 0.0, hd = 0.0;
  for (int k = 0; k < 3; ++k)
  {
    const double dc = ref[k] - 0.5 * (l[k] + h[k]), dh = 0.5 * (h[k] - l[k]);
    cd += dc * dc;
    hd += dh * dh;
  }
  const double mt = sqrt(cd) + sqrt(hd);
  n.mt[c] = nextafterf((float)(mt * 1.0001), INFINITY);
}

// The all-space child: a refitted child that holds a triangle which is no longer well-conditioned (its hits may lie
// anywhere, so every ray must reach it).  Its six bounds are NaN (one fixed quiet pattern, set directly, not through the
// formula), its margin term +inf.  rfx_bvh.h bvh_box then has six NaN slab ends whatever the ray: its fminf / fmaxf leave
// t0 = 0 (the 0 of the entry clamp) and t1 = NaN, and `t0 > t1 ...` fails in the keeping direction; the walkers'
// distance prune sees t0 = 0.  Infinite bounds would not do: for an origin and a reciprocal direction whose product
// overflows (an axis-parallel ray from beyond 3.4e8: the reciprocal is clamped to 1e30) the slab constant is infinite,
// inf - inf leaves one end of the slab NaN and fminf / fmaxf take the other, -inf, for both -- t1 = -inf culls the box
// (tests/test_mesh_update_host.py replays both in float32).
RFX_HD void bvh_child_all_space(BvhNode &n, int c)
{
  const float q = u2f(0x7FC00000u);
  n.lx[c] = n.ly[c] = n.lz[c] = q;
  n.hx[c] = n.hy[c] = n.hz[c] = q;
  n.mt[c] = INFINITY;
}

// An unwidened box of the refit: the exact float min / max of the vertices below it, and whether a triangle below it is
// not well-conditioned.  fminf / fmaxf drop a NaN vertex (such a triangle raises `ill`, and the box then does not count).
struct alignas(16) RefitBox { float lo[3], hi[3]; uint32_t ill, pad; };
RFX_HD void refit_box_empty(RefitBox &b)
{
  for (int k = 0; k < 3; ++k) { b.lo[k] = INFINITY; b.hi[k] = -INFINITY; }
  b.ill = 0; b.pad = 0;
}
RFX_HD void refit_box_vertex(RefitBox &b, const float *q)
{
  for (int k = 0; k < 3; ++k) { b.lo[k] = fminf(b.lo[k], q[k]); b.hi[k] = fmaxf(b.hi[k], q[k]); }
}
RFX_HD void refit_box_join(RefitBox &b, const RefitBox &o)
{
  for (int k = 0; k < 3; ++k) { b.lo[k] = fminf(b.lo[k], o.lo[k]); b.hi[k] = fmaxf(b.hi[k], o.hi[k]); }
  b.ill |= o.ill;
}
// child c of node n from the box below it
RFX_HD void refit_child(BvhNode &n, int c, const RefitBox &b, const double ref[3], bool widen)
{
  if (b.ill) { bvh_child_all_space(n, c); return; }
  const double l[3] = {b.lo[0], b.lo[1], b.lo[2]}, h[3] = {b.hi[0], b.hi[1], b.hi[2]};
  bvh_child_set(n, c, l, h, ref, widen);
}

// the per-triangle words rfx_scene_tri_records / rfx_renderer_tri_records report (rfx.h "Moving meshes")
constexpr int kTriRecordWords = 41;

// One launch of the device update (rfx_update_kernels.hip update_tris_kernel): triangles [first, first + count) take the
// vertices at pos (idx null: 9 floats per triangle; else 3 indices per triangle into n_pos vertices, a triangle naming
// an index >= n_pos keeps what it has).  The scene arrays are the uploaded DevScene's, the rest the renderer's own.
struct UpdateParams {
  TriGeo *tri_geo;
  TriShade *tri_shade;
  Bound *tri_bound;      // DevScene::bound + n_sph
  TriGeo *tri_leaf;      // null without a tree
  float *verts;          // 9 floats per triangle: the current vertices
  uint32_t *ill;         // per triangle: 1 = not well-conditioned
  const int32_t *slot;   // per triangle: its record in tri_leaf, -1 outside the tree
  const float *pos;
  const uint32_t *idx;
  uint32_t n_pos, first, count;
};
// The refit's launches (rfx_update_kernels.hip refit_leaves_kernel, refit_nodes_kernel): the leaves' boxes from the current
// vertices, then the nodes of one height from the boxes below them -- list[0 .. n) are that height's nodes
struct RefitParams {
  BvhNode *nodes;
  const int32_t *order;  // leaves x RFX_TRI_BVH_LEAF triangle indices, -1 padding
  const float *verts;
  const uint32_t *ill;
  RefitBox *leaf_box, *node_box;
  const int32_t *list;
  uint32_t n;            // leaves (refit_leaves_kernel) or nodes of this height (refit_nodes_kernel)
  double ref[3];         // DevScene::bvh_rx, bvh_ry, bvh_rz
};

// ---- Re-cutting (rfx.h "Re-cutting"): the cut's formulas, shared by the host mirror (rfx_scene.cpp
// rfx_scene_tri_bvh_recut) and the kernels (rfx_update_kernels.hip).  Every step is one IEEE float32 operation, with no
// contraction, so a float32 restatement gives the same bits.
// three times the centroid, per axis (v1 + v2) + v3: no division
RFX_HD void recut_sum(const float *v9, float s[3])
{
  for (int a = 0; a < 3; ++a) s[a] = (v9[a] + v9[3 + a]) + v9[6 + a];
}
RFX_HD bool recut_finite(float x) { return (f2u(x) & 0x7F800000u) != 0x7F800000u; }
// a triangle of the tree is placed -- it has a cell of the cut's box -- when it is well-conditioned and its sums are finite
RFX_HD bool recut_placed(const float s[3], uint32_t ill)
{
  return !ill && recut_finite(s[0]) && recut_finite(s[1]) && recut_finite(s[2]);
}
// one scale for the three axes (cubic cells) from the placed sums' box [lo, hi]; an empty box (lo = +inf, hi = -inf: the
// extent is -inf), a point and an extent that overflows give 0: every placed triangle then takes key 0
RFX_HD float recut_scale(const float lo[3], const float hi[3])
{
  float e = hi[0] - lo[0];
  e = fmaxf(e, hi[1] - lo[1]);
  e = fmaxf(e, hi[2] - lo[2]);
  return e > 0.0f && recut_finite(e) ? 1024.0f / e : 0.0f;
}
// The key of a placed triangle: 10 bits of cell per axis, bit b of x at 3 b, of y at 3 b + 1, of z at 3 b + 2.
// The sign of a zero bound does not reach the key.  lo_a is a minimum of the sums, and which of -0 and +0 a minimum of
// both returns depends on the reduction's order (the device's integer encoding puts -0 below +0; fminf may keep either).
// For s_a != 0, s_a - (+-0) is s_a.  For s_a = +-0 the difference is a zero of either sign, its product with the scale
// is a zero, fmaxf of two zeros is a zero and the conversion of either zero is 0.  hi_a - lo_a is compared with 0 and
// divides 1024 only where it is positive, so a zero's sign ends there too.
constexpr uint32_t kRecutCells = 1024, kRecutCellBits = 10;
constexpr uint32_t kRecutLastKey = 0x40000000u;  // an in-tree triangle that is not placed: behind every placed one
RFX_HD uint32_t recut_key(const float s[3], const float lo[3], float scale)
{
  uint32_t key = 0;
  for (int a = 0; a < 3; ++a)
  {
    const uint32_t q = (uint32_t)fminf(fmaxf((s[a] - lo[a]) * scale, 0.0f), (float)(kRecutCells - 1u));  // NaN: the 0
    for (uint32_t b = 0; b < kRecutCellBits; ++b) key |= ((q >> b) & 1u) << (3u * b + (uint32_t)a);
  }
  return key;
}
// An order-preserving code of a non-NaN float for integer atomic min / max: a < b as floats => code(a) < code(b), and
// -0 below +0
RFX_HD uint32_t recut_code(float x)
{
  const uint32_t u = f2u(x);
  return u & 0x80000000u ? ~u : u | 0x80000000u;
}
RFX_HD float recut_decode(uint32_t c) { return u2f(c & 0x80000000u ? c & 0x7FFFFFFFu : ~c); }

// The re-cut's launches (rfx_update_kernels.hip).  box: six words, [a] the code of lo_a, [3 + a] the complement of the
// code of hi_a, so that both are atomic minima and one fill with ones empties the box.
struct RecutParams {
  const uint32_t *intree;  // the n in-tree triangles, ascending
  const float *verts;
  const uint32_t *ill;
  uint32_t *box;
  uint32_t *keys;          // n sort keys, in intree's order
  uint32_t n;
};
// ... and after the sort: slot q < slots of `order` (leaves x RFX_TRI_BVH_LEAF, -1 padding) names its triangle; the
// triangle's slot, the leaf record, and -- lanes q < nodes -- the cut's children and by-height list put in place
struct RecutPlaceParams {
  const int32_t *order;
  int32_t *slot;
  const TriGeo *tri_geo;
  const TriShade *tri_shade;
  TriGeo *tri_leaf;
  BvhNode *nodes;
  const int32_t *cut_child;  // nodes x 2
  const int32_t *cut_hlist;  // nodes
  int32_t *hlist;
  uint32_t slots, nodes_n;
};

// ---- Moving spheres (rfx.h "Moving spheres"): what follows a sphere's centre and radius, shared by the host builder
// (rfx_scene.cpp SceneBuild, sphere_bvh), the host mirror (rfx_scene_sph_bvh_refit) and the kernels
// (rfx_sphere_update_kernels.hip).  None of it tests for a non-finite value: DESIGN.md "Moving spheres" has the argument.
// Sphere.cpp:13-19 as rfx_scene_add_sphere runs it: the constructor's clamp (a NaN radius fails the compare and passes)
RFX_HD float sphere_radius(float radius) { return radius <= kVerySmall ? kVerySmall : radius; }
// a sphere's own bound for the wave-bundle cull: the radius grown by a relative 1e-5
RFX_HD Bound sphere_bound(float cx, float cy, float cz, float radius)
{
  Bound b;
  b.x = cx; b.y = cy; b.z = cz; b.r = radius * 1.00001f;
  return b;
}
// The bound of a chunk of n <= 64 consecutive spheres of the device order from their bounds: centred on the mean centre,
// a sequential double sum in device-index order (the order is part of the value), reaching the farthest sphere
RFX_HD Bound sphere_chunk_bound(const Bound *bd, uint32_t n)
{
  double m[3] = {0.0, 0.0, 0.0};
  for (uint32_t i = 0; i < n; ++i) { m[0] += bd[i].x; m[1] += bd[i].y; m[2] += bd[i].z; }
  for (int k = 0; k < 3; ++k) m[k] /= (double)n;
  double r = 0.0;
  for (uint32_t i = 0; i < n; ++i)
  {
    const double dx = bd[i].x - m[0], dy = bd[i].y - m[1], dz = bd[i].z - m[2];
    r = fmax(r, sqrt(dx * dx + dy * dy + dz * dz) + (double)bd[i].r);
  }
  Bound b;
  b.x = (float)m[0]; b.y = (float)m[1]; b.z = (float)m[2]; b.r = (float)(r * 1.0001 + 1e-6);
  return b;
}
// An unwidened box of the pair tree: six doubles (c -+ (double)bound.r does not fit the triangle tree's float RefitBox).
// fmin / fmax drop a NaN, and the join is an exact min / max, so joining node by node gives the builder's range scan.
struct alignas(16) SphBox { double lo[3], hi[3]; };
RFX_HD void sph_box_empty(SphBox &b)
{
  for (int k = 0; k < 3; ++k) { b.lo[k] = INFINITY; b.hi[k] = -INFINITY; }
}
RFX_HD void sph_box_sphere(SphBox &b, const Bound &s)
{
  const double c[3] = {s.x, s.y, s.z}, rr = s.r;
  for (int k = 0; k < 3; ++k) { b.lo[k] = fmin(b.lo[k], c[k] - rr); b.hi[k] = fmax(b.hi[k], c[k] + rr); }
}
RFX_HD void sph_box_join(SphBox &b, const SphBox &o)
{
  for (int k = 0; k < 3; ++k) { b.lo[k] = fmin(b.lo[k], o.lo[k]); b.hi[k] = fmax(b.hi[k], o.hi[k]); }
}
// the box of leaf g of the pair tree: the 2 RFX_BVH_LEAF_PAIRS spheres of the device order it holds, n_sph in all
constexpr uint32_t kSphLeaf = 2 * RFX_BVH_LEAF_PAIRS;
RFX_HD SphBox sph_leaf_box(const Bound *bd, uint32_t g, uint32_t n_sph)
{
  SphBox b;
  sph_box_empty(b);
  const uint32_t q0 = kSphLeaf * g, q1 = q0 + kSphLeaf < n_sph ? q0 + kSphLeaf : n_sph;
  for (uint32_t q = q0; q < q1; ++q) sph_box_sphere(b, bd[q]);
  return b;
}

// the per-sphere words rfx_scene_sph_records / rfx_renderer_sph_records report
constexpr int kSphRecordWords = 12;

// One launch of the sphere update (rfx_sphere_update_kernels.hip update_spheres_kernel): record k of `data` (centre,
// radius) goes to sphere ids[k], or -- ids null -- first + k; a sphere index >= n_sph is a dead lane
struct SphUpdateParams {
  SphereGeo *sph_geo;
  SpherePair *sph_pair;
  Bound *bound;
  uint32_t *dirty;        // per 64-sphere chunk: holds an updated sphere
  const uint32_t *slot;   // insertion index -> device index
  const float *data;
  const uint32_t *ids;
  uint32_t n_sph, first, count;
};
// ... and its refits: the dirty chunks' bounds (refit_chunks_kernel, n = chunks), the leaves' boxes
// (refit_pair_leaves_kernel, n = leaves), then the nodes of one height (refit_pair_nodes_kernel, list[0 .. n))
struct SphRefitParams {
  BvhNode *nodes;
  const Bound *bound;
  Bound *chunk_bound;
  uint32_t *dirty;
  SphBox *leaf_box, *node_box;
  const int32_t *list;
  uint32_t n, n_sph;
  double ref[3];          // DevScene::bvh_rx, bvh_ry, bvh_rz
};

}  // namespace rfx
