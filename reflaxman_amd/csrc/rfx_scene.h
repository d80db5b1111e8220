// The host-only part of librfx.so (rfx_scene.cpp: the scene builder, image files, camera helpers and the hierarchy
// builders) as the rest of the library sees it.  No HIP here: a plain C++ compiler builds rfx_scene.cpp with this.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/rfx.h"
#include "rfx_types.h"
#include "rfx_order_types.h"

namespace rfx {

// records the calling thread's rfx_last_error text, returns code
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// The triangle BVH of a non-small scene (rfx_scene.cpp build_tri_tree): order[] lists insertion indices, leaf g =
// order[RFX_TRI_BVH_LEAF g ..], -1 padding the last leaf; resid: the triangles outside the tree.
struct TriTree {
  std::vector<BvhNode> nodes;
  std::vector<int32_t> order;  // leaves x RFX_TRI_BVH_LEAF insertion indices (-1: padding)
  std::vector<int32_t> resid;
  int depth = 0;
  size_t leaves() const { return order.size() / RFX_TRI_BVH_LEAF; }
};

// The re-cut's topology (rfx.h "Re-cutting"; rfx_scene.cpp cut_topology), a function of the leaf count alone: node(a, b)
// over leaves [a, b), b - a >= 2, takes the next index in pre-order (the root is node 0) and splits at a + (b - a) / 2; a
// one-leaf side is the child ~a.  child: nodes x 2; hlist / hoff: the nodes by height, as SceneBuild's below; depth:
// ceil(log2 leaves)
struct CutTopology {
  std::vector<int32_t> child, hlist;
  std::vector<uint32_t> hoff;
  int depth = 0;
};
CutTopology cut_topology(size_t leaves);

// Everything rfx_renderer_set_scene puts on the device, built on the host from a scene and the renderer's
// rfx_renderer_set_tri_accel mode: one vector per DevScene array (named as there in the comments), the scalar fields
// of `d` (its pointers stay null: the upload sets them) and the hierarchies' summary.
struct SceneBuild {
  SceneBuild(const rfx_scene &scene, int tri_accel);
  std::vector<SphereGeo> sg;                 // sph_geo
  std::vector<SpherePair> sp;                // sph_pair
  std::vector<MatRec> sm, tm, pm;            // sph_mat, tri_mat, pln_mat
  std::vector<int32_t> si, loc;              // sph_info, obj_loc
  std::vector<TriGeo> tg, tleaf;             // tri_geo, tri_leaf
  std::vector<TriShade> ts;                  // tri_shade
  std::vector<Bound> bd, cb;                 // bound, chunk_bound
  std::vector<CullRec> cs;                   // cull_small
  std::vector<CullTri> ct;                   // cull_tri
  std::vector<uint64_t> gm;                  // shadow_grid.cells (empty: no grid; its other fields are set in d)
  float grid_cell = 0, grid_ball = 0;        // the grid's cell size and the radius of a cell's widened ball (for the dump)
  std::vector<BvhNode> bvh;                  // bvh
  std::vector<uint32_t> aux, pool;           // bvh_aux, texels
  TriTree tt;                                // tri_bvh (nodes), tri_resid (resid)
  std::vector<PlaneGeo> pg;                  // pln_geo
  std::vector<LightRec> lr;                  // lights
  std::vector<TexRec> tr;                    // texs
  DevScene d{};
  rfx_accel_info accel{};
  OrderBox order_box{};                      // the coherent order's key box (rfx.h "Coherent order")
  // What rfx_renderer_update_triangles keeps beside the scene (rfx_update.cpp; non-small scenes with triangles, else
  // empty): per triangle its vertices as given (9 floats), its record in tri_leaf (-1: outside the tree) and whether it
  // is not well-conditioned; the tree's nodes by height (a leaf's is 0), lowest first -- hlist[hoff[h - 1] .. hoff[h])
  // are the nodes of height h >= 1, each above both its children
  std::vector<float> tverts;
  std::vector<int32_t> tslot, hlist;
  std::vector<uint32_t> till, hoff;
  // What rfx_renderer_recut_triangles keeps beside them (scenes with a triangle tree, else empty): the in-tree
  // triangles, ascending, and the cut's topology over the tree's leaves
  std::vector<uint32_t> tin;
  CutTopology cut;
  // What rfx_renderer_update_spheres keeps beside the scene (rfx.h "Moving spheres"): per sphere of the insertion order
  // its index in the device arrays, and the pair tree's nodes by height as hlist / hoff above (hoff = {0} without a tree)
  bool small_scene = false;
  std::vector<uint32_t> sslot, shoff;
  std::vector<int32_t> shlist;
};

// rfx_scene.cpp, for rfx_update.cpp: one triangle's record words in rfx_scene_tri_records' layout (NaNs canonical)
// from its geometry records, bound, vertices and class; `leaf`: the tree's copy (null: the triangle's own record)
void tri_record_words(uint32_t *out, const TriGeo &g, const TriShade &h, const Bound &b, const float *verts9, bool well,
                      const TriGeo *leaf);

// every NaN of n words reported as 0x7FC00000: its sign and payload carry nothing and differ between processors
inline void canonical_nans(void *words, size_t n)
{
  uint32_t *w = static_cast<uint32_t *>(words);
  for (size_t k = 0; k < n; ++k)
    if ((w[k] & 0x7FFFFFFFu) > 0x7F800000u) w[k] = 0x7FC00000u;
}
// ... and one sphere's, in rfx_scene_sph_records' layout: its sph_geo record, its lane of its sph_pair record, its bound
void sph_record_words(uint32_t *out, const SphereGeo &g, const SpherePair &p, int lane, const Bound &b);

}  // namespace rfx
