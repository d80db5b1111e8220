// Moving meshes (include/rfx.h "Moving meshes", "Re-cutting"): rfx_renderer_update_triangles and its host form,
// rfx_renderer_recut_triangles, the tables set_scene uploads for them, and the read-backs the tests compare with the host
// mirrors (rfx_scene.cpp).  The kernels are rfx_update_kernels.hip (and, for the re-cut's sort, rfx_order_sort.hip
// through rfx_order.cpp's order_sort); every formula is rfx_refit.h's, shared with the host builder.
#include <stddef.h>
#include <string.h>

#include <vector>

#include "rfx_query_host.h"

using namespace rfx;

template <class T>
static int fill(DevBuf<T> &b, const std::vector<T> &v)
{
  if (v.empty()) return RFX_OK;
  if (b.reserve(v.size()) < 0) return RFX_ERR_HIP;
  HIP_CHECK(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return RFX_OK;
}

int rfx::upload_update_tables(rfx_renderer *r, const SceneBuild &B)
{
  r->upd_tris = 0;
  r->cut_tris = 0;
  r->upd_sph = 0;
  r->upd_leaves = (uint32_t)B.tt.leaves();
  r->upd_hoff = B.hoff;
  RCHECK(fill(r->upd_verts, B.tverts));
  RCHECK(fill(r->upd_slot, B.tslot));
  RCHECK(fill(r->upd_ill, B.till));
  RCHECK(fill(r->upd_order, B.tt.order));
  RCHECK(fill(r->upd_hlist, B.hlist));
  if (r->upd_lbox.reserve(B.tt.leaves()) < 0 || r->upd_nbox.reserve(B.tt.nodes.size()) < 0) return RFX_ERR_HIP;
  r->upd_tris = (uint32_t)B.tslot.size();  // last: non-zero only with every table in place
  // the sphere update's tables (a non-small scene with spheres): the slot map, the pair tree's by-height lists and box
  // scratch, the chunks' dirty flags (clear between calls: refit_chunks_kernel clears what update_spheres_kernel set)
  if (!B.small_scene && !B.sslot.empty())
  {
    r->sph_hoff = B.shoff;
    RCHECK(fill(r->sph_slot, B.sslot));
    RCHECK(fill(r->sph_hlist, B.shlist));
    if (r->sph_dirty.reserve(B.cb.size()) < 0 || r->sph_lbox.reserve(B.bvh.size() + 1) < 0 ||
        r->sph_nbox.reserve(B.bvh.size() + 1) < 0)
      return RFX_ERR_HIP;
    HIP_CHECK(hipMemset(r->sph_dirty.p, 0, B.cb.size() * sizeof(uint32_t)));
    r->upd_sph = (uint32_t)B.sslot.size();  // last, as upd_tris
  }
  // the re-cut's tables, and the sort's scratch for its pairs: rfx_renderer_recut_triangles allocates nothing
  r->cut_hoff = B.cut.hoff;
  r->cut_depth = B.cut.depth;
  if (B.tin.empty()) return RFX_OK;
  RCHECK(fill(r->cut_in, B.tin));
  RCHECK(fill(r->cut_child, B.cut.child));
  RCHECK(fill(r->cut_hlist, B.cut.hlist));
  if (r->cut_box.reserve(6) < 0) return RFX_ERR_HIP;
  int rc;
  if ((rc = order_scratch(r, (uint32_t)B.tin.size())) < 0) return rc;
  r->cut_tris = (uint32_t)B.tin.size();
  return RFX_OK;
}

// Every box of the uploaded triangle tree from the current vertices, enqueued on st: the leaves, then one launch per
// height over the by-height lists as they stand (the built tree's, or the last re-cut's).  Nothing without a tree.
static int enqueue_refit(rfx_renderer *r, hipStream_t st)
{
  const DevScene &d = r->dev;
  if (!d.tri_bvh) return RFX_OK;
  RefitParams F{};
  F.nodes = const_cast<BvhNode *>(d.tri_bvh);
  F.order = r->upd_order;
  F.verts = r->upd_verts;
  F.ill = r->upd_ill;
  F.leaf_box = r->upd_lbox;
  F.node_box = r->upd_nbox;
  F.ref[0] = d.bvh_rx; F.ref[1] = d.bvh_ry; F.ref[2] = d.bvh_rz;
  F.n = r->upd_leaves;
  HIP_CHECK(launch_refit_leaves(F, st));
  for (size_t h = 1; h < r->upd_hoff.size(); ++h)
  {
    F.list = r->upd_hlist.p + r->upd_hoff[h - 1];
    F.n = r->upd_hoff[h] - r->upd_hoff[h - 1];
    HIP_CHECK(launch_refit_nodes(F, st));
  }
  return RFX_OK;
}

// what set_scene, an update and a re-cut all do to the per-view masks: the next frame builds them again
static void drop_masks(rfx_renderer *r)
{
  ++r->scene_gen;
  r->prim_key.clear();
  r->prim_seen.clear();
}

// the update and the whole tree's refit, enqueued on st
static int enqueue_update(rfx_renderer *r, uint32_t first, uint32_t count, const float *d_pos, uint32_t n_pos,
                          const uint32_t *d_idx, hipStream_t st)
{
  const DevScene &d = r->dev;
  UpdateParams U{};
  U.tri_geo = const_cast<TriGeo *>(d.tri_geo);
  U.tri_shade = const_cast<TriShade *>(d.tri_shade);
  U.tri_bound = const_cast<Bound *>(d.bound) + d.n_sph;
  U.tri_leaf = const_cast<TriGeo *>(d.tri_leaf);
  U.verts = r->upd_verts;
  U.ill = r->upd_ill;
  U.slot = r->upd_slot;
  U.pos = d_pos;
  U.idx = d_idx;
  U.n_pos = n_pos;
  U.first = first;
  U.count = count;
  HIP_CHECK(launch_update_tris(U, st));
  RCHECK(enqueue_refit(r, st));
  // the per-view masks are the old geometry's (as after set_scene); the streams, tile costs, timing sums, regroup queue
  // and rewind state are not the update's to touch
  drop_masks(r);
  return RFX_OK;
}

static int check_update(rfx_renderer *r, uint32_t first, uint32_t count, const void *pos, uint32_t n_pos,
                        const void *idx, const char *call)
{
  RCHECK(enter_call(r, pos && count && (idx || (uint64_t)n_pos == 3ull * count), call,
                    "a renderer, positions, count > 0 and, without indices, n_positions == 3 count"));
  if ((uint64_t)first + count > (uint64_t)r->dev.n_tri)
    return fail(RFX_ERR_ARG, "%s: triangles [%u, %llu) of %d", call, first, (unsigned long long)first + count, r->dev.n_tri);
  if (!r->upd_tris)
    return fail(RFX_ERR_STATE, "%s: a small scene (at most 32 spheres and 32 triangles) is uploaded again with "
                "rfx_renderer_set_scene", call);
  return RFX_OK;
}

extern "C" int rfx_renderer_update_triangles(rfx_renderer *r, uint32_t first, uint32_t count, const float *d_positions,
                                             uint32_t n_positions, const uint32_t *d_indices, void *stream)
{
  RCHECK(check_update(r, first, count, d_positions, n_positions, d_indices, "renderer_update_triangles"));
  return enqueue_update(r, first, count, d_positions, n_positions, d_indices, stream_or_own(r, stream));
}

extern "C" int rfx_renderer_update_triangles_host(rfx_renderer *r, uint32_t first, uint32_t count, const float *positions,
                                                  uint32_t n_positions, const uint32_t *indices)
{
  RCHECK(check_update(r, first, count, positions, n_positions, indices, "renderer_update_triangles_host"));
  const hipStream_t st = r->stream;
  // (a grown staging array is a new allocation: the stream is idle after every earlier host-form call)
  if (r->upd_pos.reserve(3 * (size_t)n_positions) < 0 || (indices && r->upd_idx.reserve(3 * (size_t)count) < 0))
    return RFX_ERR_HIP;
  HIP_CHECK(hipMemcpyAsync(r->upd_pos.p, positions, 12 * (size_t)n_positions, hipMemcpyHostToDevice, st));
  if (indices) HIP_CHECK(hipMemcpyAsync(r->upd_idx.p, indices, 12 * (size_t)count, hipMemcpyHostToDevice, st));
  RCHECK(enqueue_update(r, first, count, r->upd_pos, n_positions, indices ? r->upd_idx.p : nullptr, st));
  HIP_CHECK(hipStreamSynchronize(st));
  return RFX_OK;
}

// rfx.h "Re-cutting".  Keys from the current vertices, the renderer's radix sort over the in-tree list straight into the
// leaf membership (its padding, behind the in-tree count, stays -1 from set_scene), slots / leaf records / topology, refit.
extern "C" int rfx_renderer_recut_triangles(rfx_renderer *r, void *stream)
{
  RCHECK(enter_call(r, true, "renderer_recut_triangles", "a renderer"));
  if (!r->cut_tris || !r->dev.tri_bvh)
    return fail(RFX_ERR_STATE, "renderer_recut_triangles: the uploaded scene has no triangle tree (a small scene, or "
                "rfx_renderer_set_tri_accel left it out)");
  const hipStream_t st = stream_or_own(r, stream);
  const DevScene &d = r->dev;
  int rc;
  if ((rc = order_scratch(r, r->cut_tris)) < 0) return rc;  // reserved at set_scene: no allocation here
  RecutParams K{};
  K.intree = r->cut_in;
  K.verts = r->upd_verts;
  K.ill = r->upd_ill;
  K.box = r->cut_box;
  K.keys = r->order_keys;
  K.n = r->cut_tris;
  HIP_CHECK(launch_recut_keys(K, st));
  RCHECK(order_sort(r, r->cut_tris, r->cut_in, reinterpret_cast<uint32_t *>(r->upd_order.p), st));
  RecutPlaceParams Q{};
  Q.order = r->upd_order;
  Q.slot = r->upd_slot;
  Q.tri_geo = d.tri_geo;
  Q.tri_shade = d.tri_shade;
  Q.tri_leaf = const_cast<TriGeo *>(d.tri_leaf);
  Q.nodes = const_cast<BvhNode *>(d.tri_bvh);
  Q.cut_child = r->cut_child;
  Q.cut_hlist = r->cut_hlist;
  Q.hlist = r->upd_hlist;
  Q.slots = r->upd_leaves * RFX_TRI_BVH_LEAF;
  Q.nodes_n = (uint32_t)d.n_tri_bvh;
  HIP_CHECK(launch_recut_place(Q, st));
  // host-known: the by-height lists' shape and the depth are the cut's from here on
  r->upd_hoff = r->cut_hoff;
  r->dev.tri_bvh_depth = r->cut_depth;
  r->accel.tri_depth = r->cut_depth;
  RCHECK(enqueue_refit(r, st));
  drop_masks(r);
  return RFX_OK;
}

extern "C" int rfx_renderer_tri_records(rfx_renderer *r, uint32_t first, uint32_t count, uint32_t *out)
{
  RCHECK(enter_call(r, out && count, "renderer_tri_records", "a renderer, an output and count > 0"));
  if ((uint64_t)first + count > (uint64_t)r->dev.n_tri || !r->upd_tris)
    return fail(RFX_ERR_ARG, "renderer_tri_records: a range within the %d triangles of a scene that is not small",
                r->dev.n_tri);
  const DevScene &d = r->dev;
  HIP_CHECK(hipStreamSynchronize(r->stream));
  std::vector<TriGeo> g(count), leaf((size_t)r->upd_leaves * RFX_TRI_BVH_LEAF);
  std::vector<TriShade> h(count);
  std::vector<Bound> b(count);
  std::vector<float> v(9 * (size_t)count);
  std::vector<uint32_t> ill(count);
  std::vector<int32_t> slot(count);
  HIP_CHECK(hipMemcpy(g.data(), d.tri_geo + first, count * sizeof(TriGeo), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(h.data(), d.tri_shade + first, count * sizeof(TriShade), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(b.data(), d.bound + d.n_sph + first, count * sizeof(Bound), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(v.data(), r->upd_verts.p + 9 * (size_t)first, 36 * (size_t)count, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(ill.data(), r->upd_ill.p + first, 4 * (size_t)count, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(slot.data(), r->upd_slot.p + first, 4 * (size_t)count, hipMemcpyDeviceToHost));
  if (d.tri_leaf && !leaf.empty())
    HIP_CHECK(hipMemcpy(leaf.data(), d.tri_leaf, leaf.size() * sizeof(TriGeo), hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < count; ++i)
    tri_record_words(out + (size_t)kTriRecordWords * i, g[i], h[i], b[i], &v[9 * (size_t)i], ill[i] == 0,
                     d.tri_leaf && slot[i] >= 0 ? &leaf[slot[i]] : nullptr);
  return RFX_OK;
}

extern "C" int rfx_renderer_tri_bvh_nodes(rfx_renderer *r, float *out)
{
  RCHECK(enter_call(r, true, "renderer_tri_bvh_nodes", "a renderer"));
  const int n = r->dev.n_tri_bvh;
  if (!out || !n || !r->dev.tri_bvh) return n;
  HIP_CHECK(hipStreamSynchronize(r->stream));
  std::vector<BvhNode> nodes(n);
  HIP_CHECK(hipMemcpy(nodes.data(), r->dev.tri_bvh, n * sizeof(BvhNode), hipMemcpyDeviceToHost));
  static_assert(sizeof(BvhNode) == 16 * sizeof(float), "node layout");
  for (int i = 0; i < n; ++i)
  {
    const BvhNode &q = nodes[i];
    float *o = out + 16 * (size_t)i;
    for (int c = 0; c < 2; ++c)
    {
      float *b = o + 6 * c;
      b[0] = q.lx[c]; b[1] = q.ly[c]; b[2] = q.lz[c]; b[3] = q.hx[c]; b[4] = q.hy[c]; b[5] = q.hz[c];
    }
    memcpy(o + 12, q.child, 8);
    o[14] = q.mt[0]; o[15] = q.mt[1];
  }
  return n;
}

// ------------------------------------------------------------- moving spheres (rfx.h "Moving spheres")
// The update and everything that follows it, enqueued on st: the records, the dirty chunks' bounds, and -- with a pair
// tree -- every box of it from the current bounds: the leaves, then one launch per height (at most kBvhStack).
static int enqueue_sphere_update(rfx_renderer *r, uint32_t first, uint32_t count, const float *d_spheres4,
                                 const uint32_t *d_ids, hipStream_t st)
{
  const DevScene &d = r->dev;
  SphUpdateParams U{};
  U.sph_geo = const_cast<SphereGeo *>(d.sph_geo);
  U.sph_pair = const_cast<SpherePair *>(d.sph_pair);
  U.bound = const_cast<Bound *>(d.bound);
  U.dirty = r->sph_dirty;
  U.slot = r->sph_slot;
  U.data = d_spheres4;
  U.ids = d_ids;
  U.n_sph = (uint32_t)d.n_sph;
  U.first = first;
  U.count = count;
  HIP_CHECK(launch_update_spheres(U, st));
  SphRefitParams F{};
  F.nodes = const_cast<BvhNode *>(d.bvh);
  F.bound = d.bound;
  F.chunk_bound = const_cast<Bound *>(d.chunk_bound);
  F.dirty = r->sph_dirty;
  F.leaf_box = r->sph_lbox;
  F.node_box = r->sph_nbox;
  F.n_sph = (uint32_t)d.n_sph;
  F.ref[0] = d.bvh_rx; F.ref[1] = d.bvh_ry; F.ref[2] = d.bvh_rz;
  F.n = (uint32_t)d.n_chunk;
  HIP_CHECK(launch_refit_chunks(F, st));
  if (d.bvh)
  {
    F.n = (uint32_t)d.n_bvh + 1;  // a binary tree's leaves
    HIP_CHECK(launch_refit_pair_leaves(F, st));
    for (size_t h = 1; h < r->sph_hoff.size(); ++h)
    {
      F.list = r->sph_hlist.p + r->sph_hoff[h - 1];
      F.n = r->sph_hoff[h] - r->sph_hoff[h - 1];
      HIP_CHECK(launch_refit_pair_nodes(F, st));
    }
  }
  // as the triangle update: the masks are the old geometry's; nothing else of the renderer's state is touched
  drop_masks(r);
  return RFX_OK;
}

static int check_sphere_update(rfx_renderer *r, uint32_t first, uint32_t count, const void *data, const void *ids,
                               const char *call)
{
  RCHECK(enter_call(r, data && count, call, "a renderer, spheres and count > 0"));
  if (!ids && (uint64_t)first + count > (uint64_t)r->dev.n_sph)
    return fail(RFX_ERR_ARG, "%s: spheres [%u, %llu) of %d", call, first, (unsigned long long)first + count, r->dev.n_sph);
  if (r->dev.n_sph <= 32 && r->dev.n_tri <= 32)
    return fail(RFX_ERR_STATE, "%s: a small scene (at most 32 spheres and 32 triangles) is uploaded again with "
                "rfx_renderer_set_scene", call);
  return RFX_OK;
}

extern "C" int rfx_renderer_update_spheres(rfx_renderer *r, uint32_t first, uint32_t count, const float *d_spheres4,
                                           const uint32_t *d_ids, void *stream)
{
  RCHECK(check_sphere_update(r, first, count, d_spheres4, d_ids, "renderer_update_spheres"));
  if (!r->upd_sph) return RFX_OK;  // ids on a scene without spheres: every record names a sphere that is not there
  return enqueue_sphere_update(r, first, count, d_spheres4, d_ids, stream_or_own(r, stream));
}

extern "C" int rfx_renderer_update_spheres_host(rfx_renderer *r, uint32_t first, uint32_t count, const float *spheres4,
                                                const uint32_t *ids)
{
  RCHECK(check_sphere_update(r, first, count, spheres4, ids, "renderer_update_spheres_host"));
  if (!r->upd_sph) return RFX_OK;
  const hipStream_t st = r->stream;
  // (a grown staging array is a new allocation: the stream is idle after every earlier host-form call)
  if (r->sph_data.reserve(4 * (size_t)count) < 0 || (ids && r->sph_ids.reserve(count) < 0)) return RFX_ERR_HIP;
  HIP_CHECK(hipMemcpyAsync(r->sph_data.p, spheres4, 16 * (size_t)count, hipMemcpyHostToDevice, st));
  if (ids) HIP_CHECK(hipMemcpyAsync(r->sph_ids.p, ids, 4 * (size_t)count, hipMemcpyHostToDevice, st));
  RCHECK(enqueue_sphere_update(r, first, count, r->sph_data, ids ? r->sph_ids.p : nullptr, st));
  HIP_CHECK(hipStreamSynchronize(st));
  return RFX_OK;
}

extern "C" int rfx_renderer_sph_records(rfx_renderer *r, uint32_t first, uint32_t count, uint32_t *out)
{
  RCHECK(enter_call(r, out && count, "renderer_sph_records", "a renderer, an output and count > 0"));
  if ((uint64_t)first + count > (uint64_t)r->dev.n_sph || !r->upd_sph)
    return fail(RFX_ERR_ARG, "renderer_sph_records: a range within the %d spheres of a scene that is not small",
                r->dev.n_sph);
  const DevScene &d = r->dev;
  const size_t n = (size_t)d.n_sph;
  HIP_CHECK(hipStreamSynchronize(r->stream));
  std::vector<SphereGeo> g(n);
  std::vector<SpherePair> p((n + 1) / 2);
  std::vector<Bound> b(n);
  std::vector<uint32_t> slot(n);
  HIP_CHECK(hipMemcpy(g.data(), d.sph_geo, n * sizeof(SphereGeo), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(p.data(), d.sph_pair, p.size() * sizeof(SpherePair), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(b.data(), d.bound, n * sizeof(Bound), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(slot.data(), r->sph_slot.p, 4 * n, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < count; ++i)
  {
    const uint32_t q = slot[first + i];
    sph_record_words(out + (size_t)kSphRecordWords * i, g[q], p[q / 2], (int)(q & 1u), b[q]);
  }
  return RFX_OK;
}

extern "C" int rfx_renderer_sph_bvh_nodes(rfx_renderer *r, float *out)
{
  RCHECK(enter_call(r, true, "renderer_sph_bvh_nodes", "a renderer"));
  const int n = r->dev.n_bvh;
  if (!out || !n || !r->dev.bvh) return r->dev.bvh ? n : 0;
  HIP_CHECK(hipStreamSynchronize(r->stream));
  std::vector<BvhNode> nodes(n);
  HIP_CHECK(hipMemcpy(nodes.data(), r->dev.bvh, n * sizeof(BvhNode), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i)
  {
    const BvhNode &q = nodes[i];
    float *o = out + 16 * (size_t)i;
    for (int c = 0; c < 2; ++c)
    {
      float *b = o + 6 * c;
      b[0] = q.lx[c]; b[1] = q.ly[c]; b[2] = q.lz[c]; b[3] = q.hx[c]; b[4] = q.hy[c]; b[5] = q.hz[c];
    }
    canonical_nans(o, 12);
    memcpy(o + 12, q.child, 8);
    o[14] = q.mt[0]; o[15] = q.mt[1];
    canonical_nans(o + 14, 2);
  }
  return n;
}

// The lanes of sph_pair behind the scene's spheres -- the last pair's second lane of an odd count and, with more than 32
// spheres, the last leaf's padding pairs (SceneBuild: centre 0, r2 = -inf, never hit) -- four words per lane.  An update
// must leave them alone.
extern "C" int rfx_renderer_sph_padding(rfx_renderer *r, uint32_t *out)
{
  RCHECK(enter_call(r, true, "renderer_sph_padding", "a renderer"));
  const size_t n = (size_t)r->dev.n_sph;
  const size_t pairs = n > 32 ? ((n + 1) / 2 + RFX_BVH_LEAF_PAIRS - 1) / RFX_BVH_LEAF_PAIRS * RFX_BVH_LEAF_PAIRS : (n + 1) / 2;
  const size_t lanes = 2 * pairs - n;
  if (!out || !lanes) return (int)lanes;
  HIP_CHECK(hipStreamSynchronize(r->stream));
  std::vector<SpherePair> p(pairs);
  HIP_CHECK(hipMemcpy(p.data(), r->dev.sph_pair, pairs * sizeof(SpherePair), hipMemcpyDeviceToHost));
  for (size_t q = n; q < 2 * pairs; ++q)
  {
    const SpherePair &s = p[q / 2];
    const float w[4] = {s.cx[q & 1], s.cy[q & 1], s.cz[q & 1], s.r2[q & 1]};
    memcpy(out + 4 * (q - n), w, sizeof(w));
  }
  return (int)lanes;
}

extern "C" int rfx_renderer_sph_chunk_bounds(rfx_renderer *r, float *out)
{
  RCHECK(enter_call(r, true, "renderer_sph_chunk_bounds", "a renderer"));
  const int n = r->dev.n_chunk;
  if (!out || !n) return n;
  HIP_CHECK(hipStreamSynchronize(r->stream));
  HIP_CHECK(hipMemcpy(out, r->dev.chunk_bound, n * sizeof(Bound), hipMemcpyDeviceToHost));
  canonical_nans(out, 4 * (size_t)n);
  return n;
}

extern "C" int rfx_renderer_tri_leaves(rfx_renderer *r, int32_t *leaf_ids, int32_t *slot, uint32_t *records)
{
  RCHECK(enter_call(r, true, "renderer_tri_leaves", "a renderer"));
  const DevScene &d = r->dev;
  if (!d.n_tri_bvh || !d.tri_bvh || !d.tri_leaf || !r->upd_tris) return 0;
  const size_t slots = (size_t)r->upd_leaves * RFX_TRI_BVH_LEAF;
  HIP_CHECK(hipStreamSynchronize(r->stream));
  if (leaf_ids) HIP_CHECK(hipMemcpy(leaf_ids, r->upd_order.p, 4 * slots, hipMemcpyDeviceToHost));
  if (slot) HIP_CHECK(hipMemcpy(slot, r->upd_slot.p, 4 * (size_t)r->upd_tris, hipMemcpyDeviceToHost));
  if (records && slots)
  {
    std::vector<TriGeo> leaf(slots);
    HIP_CHECK(hipMemcpy(leaf.data(), d.tri_leaf, slots * sizeof(TriGeo), hipMemcpyDeviceToHost));
    static_assert(offsetof(TriGeo, pad) == 48, "twelve geometry words, then pad[0] and pad[1]");
    for (size_t q = 0; q < slots; ++q)
    {
      uint32_t *o = records + 14 * q;
      memcpy(o, &leaf[q], 56);
      for (int k = 0; k < 14; ++k)
        if ((o[k] & 0x7FFFFFFFu) > 0x7F800000u) o[k] = 0x7FC00000u;  // as tri_record_words reports a NaN
    }
  }
  return (int)slots;
}
