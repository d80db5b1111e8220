// rfx_span.h -- the hit queries on a per-ray interval (include/rfx.h "Ray intervals": rfx_query_hits_span,
// rfx_query_occluded_span and their ordered forms).
//
// A candidate is an object whose trace() reports a hit, at the float distance the query reports, dist = sqrt_rn(sq).
// It is eligible iff dist <= hi and (dist, object) > (lo, after) lexicographically (SpanLane::eligible: plain float
// comparisons on the rounded distance).  The closest-hit query keeps rfx_query_hits' rule on the eligible candidates;
// the any-hit query asks whether an eligible candidate other than skip[i] exists.
//
// One walk serves both (span_walk): the scene's loops -- the small scene's cull mask, or the sphere BVH / bundle-culled
// chunks, the triangle BVH / chunks, the planes -- with the primitives' tests of rfx_intersect.h, handing every
// candidate to a visitor.  SpanClosest keeps the winner, SpanAny stops the lane at its first eligible occluder.
//   * The span filters a candidate BEFORE tri_takes: a candidate the span rejects never becomes the running best, so
//     it never feeds the "beyond the closest hit" rejects (tri_z, plane_hit, bvh_beyond).
//   * Those rejects take min(best sq, seed), where seed is hi^2 rounded up and widened by 2^-16 (SpanLane::seed; +inf
//     without a usable hi).  Each of them drops a candidate only when its rounded distance is strictly above
//     sqrt_rn(bound) >= hi, i.e. one the span would refuse anyway; the exact `dist <= hi` stays with the candidate.  The
//     seed lives apart from the winner record: Hit::sq is +inf until an eligible candidate is taken, so a candidate at
//     exactly dist == hi is still taken.  The any-hit walk prunes by the seed alone.
//   * The small-scene triangle loop runs every triangle's own z stage (no TriMates group state), so a mate the span
//     filters out leaves nothing behind for the next one.
// The kernels' outputs are rfx_hits.h's (hit_planes_store), their CFG bits a query's three, their slots ray_slot's rule
// or the ordered one (rfx_ordered.h ordered_query_slot). rfx_trace_span.hip is the one unit that includes this.
#pragma once
#include <hip/hip_runtime.h>

#include "rfx_hits.h"
#include "rfx_ordered.h"
#include "rfx_span_types.h"

#pragma clang fp contract(off)

namespace rfx {

// A lane's interval.  No lower end is lo = -1 (every distance is positive), no upper end hi = +inf.
struct SpanLane {
  float lo, hi, seed;
  int32_t after;
  __device__ __forceinline__ bool eligible(float sq, int obj) const
  {
    const float dist = sqrt_rn(sq);
    return dist <= hi && (dist > lo || (dist == lo && obj > after));
  }
};

// ray i's interval.  seed: for hi^2 a normal float, RN(RN(hi hi) (1 + 2^-16)) >= hi^2 (1 + 2^-17); else no pruning.
__device__ __forceinline__ SpanLane span_lane(const SpanParams &P, uint64_t i, bool live)
{
  SpanLane s;
  s.lo = -1.0f; s.hi = INFINITY; s.seed = INFINITY; s.after = -1;
  if (live)
  {
    if (P.lo)
    {
      s.lo = __builtin_nontemporal_load(P.lo + i);
      if (P.after) s.after = __builtin_nontemporal_load(P.after + i);
    }
    if (P.hi) s.hi = __builtin_nontemporal_load(P.hi + i);
    if (s.hi >= 0x1p-40f) s.seed = s.hi * s.hi * 0x1.0001p+0f;
  }
  return s;
}

// ------------------------------------------------------------- the visitors
// bound(): the square the distance rejects may prune against; take(): a candidate that passed its intersection test;
// done(): the lane wants no more candidates.
struct SpanClosest {
  static constexpr bool kAny = false;
  SpanLane sp;
  Hit h;
  __device__ __forceinline__ float bound() const { return fminf(h.sq, sp.seed); }
  __device__ __forceinline__ bool done() const { return false; }
  __device__ __forceinline__ void take(float sq, int obj, int kind, int i, float t, float u = 0.0f, float v = 0.0f)
  {
    const bool ok = sp.eligible(sq, obj) && tri_takes(sq, h.sq, obj, h.obj);
    hit_take(h, ok, sq, obj, kind, i, t, u, v);
  }
};
struct SpanAny {
  static constexpr bool kAny = true;
  SpanLane sp;
  int32_t skip;  // an object index; one that names no object skips nothing
  bool occ;
  __device__ __forceinline__ float bound() const { return sp.seed; }
  __device__ __forceinline__ bool done() const { return occ; }
  __device__ __forceinline__ void take(float sq, int obj, int, int, float, float = 0.0f, float = 0.0f)
  {
    if (obj != skip && sp.eligible(sq, obj)) occ = true;
  }
};

// ------------------------------------------------------------- the walks
// rfx_bvh.h's walk over either tree for one lane's ray: both children tested, the nearer entered first, a child entered
// beyond vis.bound() left out; leaf(l) runs leaf l's tests.  The stack is the workgroup's (BvhGlobal).
template <class V, class Leaf>
__device__ __forceinline__ void span_bvh(const BvhNode *nodes, const RayInv &ri, float len, V &vis, Leaf &&leaf)
{
  const BvhGlobal ns{};
  BvhSlot *stack = ns.stack();
  int sp = 0, node = 0;
  for (;;)
  {
    if (node >= 0)
    {
      const BvhNode n = nodes[node];
      const float bound = vis.bound();
      float t0, t1;
      const bool h0 = bvh_box(n, 0, ri, t0) && !bvh_beyond(t0, len, bound);
      const bool h1 = bvh_box(n, 1, ri, t1) && !bvh_beyond(t1, len, bound);
      if (h0 && h1)
      {
        const bool first0 = !(t1 < t0);
        stack[BvhGlobal::kStride * sp++] = first0 ? n.child[1] : n.child[0];
        node = first0 ? n.child[0] : n.child[1];
        continue;
      }
      if (h0 || h1)
      {
        node = h0 ? n.child[0] : n.child[1];
        continue;
      }
    }
    else
    {
      leaf(~node);
      if (vis.done()) return;
    }
    if (sp == 0) return;
    node = stack[BvhGlobal::kStride * --sp];
  }
}

// the spheres 2j and 2j + 1 of pair j, given its b and d (SEL: the large-scene form of sphere_tail)
template <bool SEL, class TabsT, class V>
__device__ __forceinline__ void span_pair(const TabsT &T, int j, f2 b, f2 d, v3 ray, const RayConst &k, V &vis, Cnt &cnt)
{
  constexpr bool STATS = false;
  if (!pair_may_hit(b, d)) return;  // both miss: one branch
  float t, sq;
  if (sphere_tail<STATS, false, SEL>(b.x, d.x, ray, k, t, sq, cnt)) vis.take(hit_key(sq), T.sph_info(4 * j), 0, 2 * j, t);
  if (sphere_tail<STATS, false, SEL>(b.y, d.y, ray, k, t, sq, cnt))
    vis.take(hit_key(sq), T.sph_info(4 * j + 2), 0, 2 * j + 1, t);
}

template <class V>
__device__ __forceinline__ void span_planes(const DevScene &S, v3 o, v3 ray, const RayConst &k, V &vis, Cnt &cnt)
{
  constexpr bool STATS = false;
  for (int i = 0; i < S.n_pln && !vis.done(); ++i)
  {
    const PlaneGeo g = S.pln_geo[i];
    float t, sq;
    if (plane_hit<STATS, false>(g, o, ray, t, sq, cnt, k, vis.bound())) vis.take(sq, g.obj, 2, i, t);
  }
}

// Every candidate of (o, ray) to vis.  Call with every lane of the wave active and at least one live; `live` lanes walk.
template <int CFG, class V>
__device__ __forceinline__ void span_walk(const DevScene &S, v3 o, v3 ray, bool live, V &vis, Cnt &cnt)
{
  constexpr bool STATS = false;
  constexpr bool SMALL = (CFG & kCfgSmall) != 0, PLANES = (CFG & kCfgPlanes) != 0, TBVH = (CFG & kCfgTriBvh) != 0;
  const Tabs<SMALL> T{S};
  const RayConst k = ray_const(ray);
  const Bundle B = make_bundle(o, ray, live);
  if constexpr (SMALL)
  {
    // one cull mask for the scene (rfx_queries.h closest_hit_small): the object loops run in the live lanes only
    uint64_t om = S.cull_valid;
    if (B.ok) om = cull_small(T.cull(), S.cull_valid, B);
    if (!live) return;
    for (uint32_t pm = small_pairs(om); pm && !vis.done(); pm &= pm - 1u)
    {
      const int j = __builtin_ctz(pm);
      f2 b, d;
      pair_bd(S.sph_pair[j], o, k, b, d);
      span_pair<false>(T, j, b, d, ray, k, vis, cnt);
    }
    for (uint64_t tm = small_tris(om); tm && !vis.done(); tm &= tm - 1ull)
    {
      const int i = __builtin_ctzll(tm);
      float t, u, v, sq;
      if (tri_hit<STATS, false>(S.tri_geo[i], o, ray, t, u, v, sq, cnt, k, vis.bound()))
        vis.take(hit_key(sq), S.tri_shade[i].obj, 1, i, t, u, v);
    }
  }
  else
  {
    // rfx_queries.h closest_hit / occluded: a narrow bundle's closest hit culls the chunks for the whole wave, every
    // other ray walks the trees lane by lane; a scene without a tree takes the chunk loops
    const bool narrow = !V::kAny && B.ok && B.cosa > kNarrowBundleCos;
    const bool use_bvh = S.bvh != nullptr && !narrow;
    if (use_bvh && live)
    {
      const RayInv ri = ray_inv(S, o, ray);
      span_bvh(S.bvh, ri, prune_len(k), vis, [&](int l) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < RFX_BVH_LEAF_PAIRS; ++e)
        {
          const int j = RFX_BVH_LEAF_PAIRS * l + e;
          f2 b, d;
          pair_bd(S.sph_pair[j], o, k, b, d);
          span_pair<true>(T, j, b, d, ray, k, vis, cnt);
        }
      });
    }
    for (int cfirst = 0; !use_bvh && cfirst < S.n_chunk; cfirst += 64)
    {
      if (V::kAny && __ballot(live && !vis.done()) == 0) return;
      uint64_t cm = B.ok ? cull_chunk(S.chunk_bound, cfirst, min(64, S.n_chunk - cfirst), B)
                         : all_bits(min(64, S.n_chunk - cfirst));
      while (cm)
      {
        const int first = 64 * (cfirst + __builtin_ctzll(cm));
        cm &= cm - 1ull;
        const int n = min(64, S.n_sph - first);
        const uint64_t m = B.ok ? cull_chunk(S.bound, first, n, B) : all_bits(n);
        for (uint32_t pm = pair_bits(m); pm; pm &= pm - 1u)
        {
          const int j = (first >> 1) + __builtin_ctz(pm);
          f2 b, d;
          pair_bd(S.sph_pair[j], o, k, b, d);
          if (live && !vis.done()) span_pair<true>(T, j, b, d, ray, k, vis, cnt);
          // (as occluded(): the wave leaves once every live lane has its occluder)
          if (V::kAny && __ballot(live && !vis.done()) == 0) return;
        }
      }
    }
    bool use_tbvh = false;
#if RFX_TRI_BVH
    if constexpr (TBVH)
    {
      use_tbvh = S.tri_bvh != nullptr && (V::kAny || S.tri_bvh_narrow || !narrow);
      if (use_tbvh && live && !vis.done())
      {
        const RayInv ri = ray_inv(S, o, ray);
        span_bvh(S.tri_bvh, ri, prune_len(k), vis, [&](int l) __attribute__((always_inline)) {
#pragma unroll
          for (int e = 0; e < RFX_TRI_BVH_LEAF; ++e)
          {
            const TriGeo &g = S.tri_leaf[RFX_TRI_BVH_LEAF * l + e];
            float t, u, v, sq;
            if (tri_hit<STATS, false, V::kAny>(g, o, ray, t, u, v, sq, cnt, k, vis.bound()))
              vis.take(hit_key(sq), tri_rec_int(g.pad[1]), 1, tri_rec_int(g.pad[0]), t, u, v);
          }
        });
        // the triangles outside the tree
        for (int q = 0; q < S.n_tri_resid && !vis.done(); ++q)
        {
          const int i = S.tri_resid[q];
          float t, u, v, sq;
          if (tri_hit<STATS, false, V::kAny>(S.tri_geo[i], o, ray, t, u, v, sq, cnt, k, vis.bound()))
            vis.take(hit_key(sq), S.tri_shade[i].obj, 1, i, t, u, v);
        }
      }
    }
#endif
    for (int first = 0; !use_tbvh && first < S.n_tri; first += 64)
    {
      if (V::kAny && __ballot(live && !vis.done()) == 0) return;
      const int n = min(64, S.n_tri - first);
      for (uint64_t m = B.ok ? cull_chunk(S.bound, S.n_sph + first, n, B) : all_bits(n); m; m &= m - 1ull)
      {
        const int i = first + __builtin_ctzll(m);
        float t, u, v, sq;
        if (live && !vis.done() && tri_hit<STATS, false, V::kAny>(S.tri_geo[i], o, ray, t, u, v, sq, cnt, k, vis.bound()))
          vis.take(hit_key(sq), S.tri_shade[i].obj, 1, i, t, u, v);
        if (V::kAny && __ballot(live && !vis.done()) == 0) return;
      }
    }
    if (!live) return;
  }
  if constexpr (PLANES) span_planes(S, o, ray, k, vis, cnt);
}

// ------------------------------------------------------------- the two bodies
// sl: the lane's ray among P's arrays and whether the lane is live (query_hits_body's rule); lut: the kernel's own table
template <int CFG>
__device__ __forceinline__ void query_hits_span_body(const DevScene &S, const SpanParams &P, const RaySlot &sl, float *lut)
{
  static_assert((CFG & ~kHitCfgMask) == 0 && !((CFG & kCfgSmall) && (CFG & kCfgTriBvh)), "a query's CFG bits");
  const bool live = sl.valid;
  const RayRecord r = lane_ray(P.H.rays, sl.i, live);
  const v3 o = r.o, d = r.d;
  SpanClosest vis;
  vis.sp = span_lane(P, sl.i, live);
  vis.h = hit_none();
  for (uint32_t i = threadIdx.x; i < 256; i += kWgThreads) lut[i] = (float)i / 255.0f;  // Color.cpp:11-13
  if constexpr ((CFG & kCfgSmall) != 0) stage_small_scene(S);
  __syncthreads();
  Cnt cnt;
  if (__ballot(live)) span_walk<CFG>(S, o, d, live, vis, cnt);  // (a raster's edge tiles may hold no live lane)
  if (live) hit_planes_store<CFG>(S, P.H, sl, o, d, vis.h, lut, cnt);
}

template <int CFG>
__device__ __forceinline__ void query_occluded_span_body(const DevScene &S, const SpanParams &P, const RaySlot &sl)
{
  static_assert((CFG & ~kHitCfgMask) == 0 && !((CFG & kCfgSmall) && (CFG & kCfgTriBvh)), "a query's CFG bits");
  const bool live = sl.valid;
  const RayRecord r = lane_ray(P.H.rays, sl.i, live);
  const v3 o = r.o, d = r.d;
  SpanAny vis;
  vis.sp = span_lane(P, sl.i, live);
  vis.sp.after = -1;  // (the any-hit has no `after`: its lower end is inclusive)
  vis.skip = live && P.H.skip ? __builtin_nontemporal_load(P.H.skip + sl.i) : -1;
  vis.occ = false;
  if constexpr ((CFG & kCfgSmall) != 0)
  {
    stage_small_scene(S);
    __syncthreads();
  }
  Cnt cnt;
  if (__ballot(live)) span_walk<CFG>(S, o, d, live, vis, cnt);
  if (live) P.H.occluded[sl.i] = vis.occ ? 1 : 0;
}

// ------------------------------------------------------------- the kernels
// ORDERED: the lane's slot is order[slot] of [slot0, slot1) (rfx_ordered.h), else ray_slot's rule on H (rfx_hits.h)
template <bool ORDERED>
__device__ __forceinline__ RaySlot span_slot(const SpanParams &P)
{
  if constexpr (ORDERED)
    return ordered_query_slot(P.order, P.slot0, P.slot1, P.H.n);
  else
    return hit_slot(P.H);
}

template <int CFG, bool ORDERED>
__global__ __launch_bounds__(kWgThreads) void query_hits_span_kernel(DevScene S, SpanParams P)
{
  __shared__ float lut[256];
  query_hits_span_body<CFG>(S, P, span_slot<ORDERED>(P), lut);
}

template <int CFG, bool ORDERED>
__global__ __launch_bounds__(kWgThreads) void query_occluded_span_kernel(DevScene S, SpanParams P)
{
  query_occluded_span_body<CFG>(S, P, span_slot<ORDERED>(P));
}

}  // namespace rfx
