// rfx_queries.h -- the two questions the bounce loop asks of a scene, for every kind of object at once: the closest hit
// (closest_hit: chunk culls or the BVH walkers, then triangles and planes; closest_hit_small: one cull mask for a scene
// of at most 64 objects) and the shadow rays' any-hit (occluded, occluded_small), with the plane loops both share.
#pragma once
#include <hip/hip_runtime.h>

#include "rfx_types.h"
#include "rfx_shade_inputs.h"
#include "rfx_intersect.h"
#include "rfx_bundle.h"
#include "rfx_bvh.h"

#pragma clang fp contract(off)

namespace rfx {

// The planes (Scene::addPlane extension, Plane.cpp:36-73) for one lane, after the other kinds: every lane that
// traces tests every plane (an infinite plane has no bounding sphere to cull with).
template <bool STATS>
__device__ __forceinline__ void closest_planes(const DevScene &S, v3 origin, v3 ray, const RayConst &k, Hit &h, Cnt &cnt)
{
  for (int i = 0; i < S.n_pln; ++i)
  {
    const PlaneGeo g = S.pln_geo[i];
    float t, sq;
    if (plane_hit<STATS, false>(g, origin, ray, t, sq, cnt, k, h.sq))
      hit_take(h, tri_takes(sq, h.sq, g.obj, h.obj), sq, g.obj, 2, i, t);
  }
}

// any-hit over the planes but the hit one (skip_pln)
template <bool STATS>
__device__ __forceinline__ bool occluded_planes(const DevScene &S, v3 o, v3 ray, const RayConst &k, int skip_pln, Cnt &cnt)
{
  float t, sq;
  for (int i = 0; i < S.n_pln; ++i)
  {
    if constexpr (STATS)
    {
      if (i != skip_pln && plane_hit<STATS, true>(S.pln_geo[i], o, ray, t, sq, cnt, k)) return true;
    }
    else if (plane_hit<STATS, true>(S.pln_geo[i], o, ray, t, sq, cnt, k) && i != skip_pln)
      return true;
  }
  return false;
}

// Call with every lane of the wave active; `live` lanes trace (origin, ray).  B: the bundle, or null.
// Large scenes: the spheres are stored in spatial order (recursive median splits), 64 to a chunk with a bounding sphere;
// the bundle culls whole chunks (one lane per chunk), then the spheres of the surviving chunks.  The
// visiting order is then not the insertion order, so spheres take the general (distance, object) rule.
template <bool STATS, bool PLANES, bool TBVH = false, class NS = BvhGlobal>
__device__ __forceinline__ void closest_hit(const DevScene &S, v3 origin, v3 ray, bool live, const Bundle *B, Hit &h,
                                            Cnt &cnt, const NS &ns = NS{})
{
  if (live) RFX_CNT(C_SEGMENTS);
  h.obj = -1; h.kind = 0; h.i = 0; h.t = 0.0f; h.u = 0.0f; h.v = 0.0f; h.sq = kNoHitKey;
  const RayConst k = ray_const(ray);
  const bool cull = B && B->ok;
#ifdef RFX_DEBUG_PROF
  uint32_t st_chunks = 0, st_sph = 0, st_pairs = 0;
#endif
  RFX_PROF_BEGIN(P_SPH);
  // a narrow bundle (the primary rays of a tile: one origin, a cone of ~0.1 degree) culls the spatial chunks and
  // their spheres for the whole wave at once; wider ones walk the BVH lane by lane
  const bool use_bvh = !STATS && S.bvh != nullptr && !(cull && B->cosa > kNarrowBundleCos);
  if (use_bvh && live) closest_spheres_bvh<STATS>(S, origin, ray, k, h, cnt, ns);
  for (int cfirst = 0; !use_bvh && cfirst < S.n_chunk; cfirst += 64)
  {
    uint64_t cm = cull ? cull_chunk(S.chunk_bound, cfirst, min(64, S.n_chunk - cfirst), *B)
                       : all_bits(min(64, S.n_chunk - cfirst));
#ifdef RFX_DEBUG_PROF
    st_chunks += __popcll(cm);
#endif
    while (cm)
    {
      const int first = 64 * (cfirst + __builtin_ctzll(cm));
      cm &= cm - 1ull;
      const int n = min(64, S.n_sph - first);
      const uint64_t m = cull ? cull_chunk(S.bound, first, n, *B) : all_bits(n);
      uint32_t pm = pair_bits(m);
#ifdef RFX_DEBUG_PROF
      st_sph += __popcll(m);
      st_pairs += __popc(pm);
#endif
      while (pm)
      {
        const int j = (first >> 1) + __builtin_ctz(pm);
        pm &= pm - 1u;
        f2 b, d;
        pair_bd(S.sph_pair[j], origin, k, b, d);
        if (!live) continue;
        if constexpr (!STATS)
          if (!pair_may_hit(b, d)) continue;  // both miss: one branch
        float t, sq;
        if (sphere_tail<STATS, false, true>(b.x, d.x, ray, k, t, sq, cnt))
        {
          const float key = hit_key(sq);
          const int obj = S.sph_info[4 * j];
          hit_take(h, tri_takes(key, h.sq, obj, h.obj), key, obj, 0, 2 * j, t);
        }
        if ((!STATS || 2 * j + 1 < S.n_sph) && sphere_tail<STATS, false, true>(b.y, d.y, ray, k, t, sq, cnt))
        {
          const float key = hit_key(sq);
          const int obj = S.sph_info[4 * j + 2];
          hit_take(h, tri_takes(key, h.sq, obj, h.obj), key, obj, 0, 2 * j + 1, t);
        }
      }
    }
  }
  RFX_PROF_END(P_SPH);
#ifdef RFX_DEBUG_PROF
  RFX_CULL_STAT_LARGE(2, cull, __ballot(live), st_chunks, st_sph, st_pairs);
#endif
  RFX_PROF_BEGIN(P_TRI);
  // the triangle tree, lane by lane (rfx_types.h RFX_TRI_BVH; TBVH: the kernel instantiations of scenes that have
  // one): wide bundles, and narrow ones where the host says so (DevScene::tri_bvh_narrow)
  bool use_tbvh = false;
#if RFX_TRI_BVH
  if constexpr (TBVH && !STATS)
  {
    use_tbvh = S.tri_bvh != nullptr && (S.tri_bvh_narrow || !(cull && B->cosa > kNarrowBundleCos));
    if (use_tbvh && live) closest_tris_bvh<STATS>(S, origin, ray, k, h, cnt, ns);
  }
#endif
  for (int first = 0; !use_tbvh && first < S.n_tri; first += 64)
  {
    const int n = min(64, S.n_tri - first);
    uint64_t m = (B && B->ok) ? cull_chunk(S.bound, S.n_sph + first, n, *B) : all_bits(n);
    while (m)
    {
      const int i = first + __builtin_ctzll(m);
      m &= m - 1ull;
      if (!live) continue;
      float t, u, v, sq;
      if (tri_hit<STATS, false>(S.tri_geo[i], origin, ray, t, u, v, sq, cnt, k, h.sq))
      {
        RFX_CNT(C_TRI_D);
        const int obj = S.tri_shade[i].obj;
        const float key = hit_key(sq);
        hit_take(h, tri_takes(key, h.sq, obj, h.obj), key, obj, 1, i, t, u, v);
      }
    }
  }
  if constexpr (PLANES)
    if (live) closest_planes<STATS>(S, origin, ray, k, h, cnt);
  RFX_PROF_END(P_TRI);
}

// ------------------------------------------------------------- small scenes (<= 64 objects)
// One cull mask covers the whole scene (bit l: object l of the bound array, spheres then triangles), so
// the object loops need no wave-wide step and run only in the lanes that trace -- a lane leaves the
// any-hit loop at its first occluder.
// lane-layout masks (CullRec): pair q <- lanes q and 16 + q; triangle i <- lane 32 + i
__device__ __forceinline__ uint32_t small_pairs(uint64_t om) { return (uint32_t)((om | (om >> 16)) & 0xFFFFull); }
__device__ __forceinline__ uint64_t small_tris(uint64_t om) { return om >> 32; }

template <bool STATS, bool PLANES>
__device__ __forceinline__ void closest_hit_small(const DevScene &S, v3 origin, v3 ray, uint64_t om, Hit &h, Cnt &cnt)
{
  RFX_CNT(C_SEGMENTS);
  h.obj = -1; h.kind = 0; h.i = 0; h.t = 0.0f; h.u = 0.0f; h.v = 0.0f; h.sq = kNoHitKey;
  const RayConst k = ray_const(ray);
  RFX_PROF_BEGIN(P_SPH);
  // spheres in index order carry increasing object indices, so among spheres a strict `<` already keeps
  // the first of equal distances
  uint32_t pm = small_pairs(om);
  while (pm)
  {
    const int j = __builtin_ctz(pm);
    pm &= pm - 1u;
    f2 b, d;
    pair_bd(S.sph_pair[j], origin, k, b, d);
    if constexpr (!STATS)
      if (!pair_may_hit(b, d)) continue;  // both miss: one branch
    float t, sq;
    if (sphere_tail<STATS, false>(b.x, d.x, ray, k, t, sq, cnt))
    {
      const float key = hit_key(sq);
      if (sph_takes(key, h.sq)) { h.sq = key; h.obj = 2 * j; h.t = t; }
    }
    if ((!STATS || 2 * j + 1 < S.n_sph) && sphere_tail<STATS, false>(b.y, d.y, ray, k, t, sq, cnt))
    {
      const float key = hit_key(sq);
      if (sph_takes(key, h.sq)) { h.sq = key; h.obj = 2 * j + 1; h.t = t; }
    }
  }
  if (h.obj >= 0)
  {
    h.i = h.obj;
    h.obj = Tabs<true>{S}.sph_info(2 * h.i);
  }
  RFX_PROF_END(P_SPH);
  RFX_PROF_BEGIN(P_TRI);
  uint64_t tm = small_tris(om);
  TriMates<STATS, false> zs;
  while (tm)
  {
    const int i = __builtin_ctzll(tm);
    tm &= tm - 1ull;
    float t, u, v, sq;
    if (zs.hit(S.tri_geo[i], origin, ray, t, u, v, sq, cnt, k, h.sq))
    {
      RFX_CNT(C_TRI_D);
      const int obj = S.tri_shade[i].obj;
      const float key = hit_key(sq);
      hit_take(h, tri_takes(key, h.sq, obj, h.obj), key, obj, 1, i, t, u, v);
    }
  }
  if constexpr (PLANES) closest_planes<STATS>(S, origin, ray, k, h, cnt);
  RFX_PROF_END(P_TRI);
}

// Scene.cpp:129-141 for a small scene (see occluded below for the order and counter notes)
template <bool STATS, bool PLANES>
__device__ __forceinline__ bool occluded_small(const DevScene &S, v3 o, v3 ray, int skip_sph, int skip_tri, int skip_pln,
                                               uint64_t om, Cnt &cnt)
{
  const RayConst k = ray_const(ray);
  float t, sq, u, v;
  uint32_t pm = small_pairs(om);
  while (pm)
  {
    const int j = __builtin_ctz(pm);
    pm &= pm - 1u;
    f2 b, d;
    pair_bd(S.sph_pair[j], o, k, b, d);
    if constexpr (STATS)
    {
      if (2 * j != skip_sph && sphere_tail<STATS, true>(b.x, d.x, ray, k, t, sq, cnt)) return true;
      if (2 * j + 1 != skip_sph && 2 * j + 1 < S.n_sph && sphere_tail<STATS, true>(b.y, d.y, ray, k, t, sq, cnt))
        return true;
    }
    else
    {
      // a miss on both spheres (the common case) costs one branch; the hit object is filtered out after
      // its test, which does not change the boolean
      if (!pair_may_hit(b, d)) continue;
      if (sphere_tail<STATS, true>(b.x, d.x, ray, k, t, sq, cnt) && 2 * j != skip_sph) return true;
      if (sphere_tail<STATS, true>(b.y, d.y, ray, k, t, sq, cnt) && 2 * j + 1 != skip_sph) return true;
    }
  }
  uint64_t tm = small_tris(om);
  TriMates<STATS, true> zs;
  while (tm)
  {
    const int i = __builtin_ctzll(tm);
    tm &= tm - 1ull;
    if constexpr (STATS)
    {
      if (i != skip_tri && tri_hit<STATS, true>(S.tri_geo[i], o, ray, t, u, v, sq, cnt, k)) return true;
    }
    else if (zs.hit(S.tri_geo[i], o, ray, t, u, v, sq, cnt, k) && i != skip_tri)
      return true;
  }
  if constexpr (PLANES) return occluded_planes<STATS>(S, o, ray, k, skip_pln, cnt);
  return false;
}

// ------------------------------------------------------------- shadow any-hit
// Scene.cpp:129-141: every object but the hit one (skip_sph / skip_tri: its sphere or triangle index,
// -1 for the other kind); the boolean does not depend on the order.  Call with every lane of the wave
// active; `live` lanes test (o, ray).  A lane stops at its first occluder and the wave once every live
// lane has one.  (Spheres precede triangles, the reference's order for scenes whose objects are added
// spheres-first -- then even the event counters match it: the second sphere of a pair is counted only
// when the first did not occlude.)
template <bool STATS, bool PLANES, bool TBVH = false, class NS = BvhGlobal>
__device__ __forceinline__ bool occluded(const DevScene &S, v3 o, v3 ray, bool live, int skip_sph, int skip_tri,
                                         int skip_pln, const Bundle *B, Cnt &cnt, const NS &ns = NS{}, int *hint = nullptr)
{
  const RayConst k = ray_const(ray);
  const bool cull = B && B->ok;
  bool occ = false;
  float t, sq, u, v;
  const bool use_bvh = !STATS && S.bvh != nullptr;
  if (use_bvh)
  {
    int found = -1;
    if (live) found = occluded_spheres_bvh<STATS>(S, o, ray, k, skip_sph, cnt, ns, hint ? *hint : -1);
    occ = found >= 0;
    if (RFX_OCC_HINT && hint)
    {
      // the next query's hint: the occluder of this wave's lowest occluded lane
      const uint64_t fm = __ballot(found >= 0);
      if (fm) *hint = __builtin_amdgcn_readlane(found, (int)__builtin_ctzll(fm));
    }
  }
  for (int cfirst = 0; !use_bvh && cfirst < S.n_chunk; cfirst += 64)
  {
    if (__ballot(live && !occ) == 0) return occ;
    uint64_t cm = cull ? cull_chunk(S.chunk_bound, cfirst, min(64, S.n_chunk - cfirst), *B)
                       : all_bits(min(64, S.n_chunk - cfirst));
    while (cm)
    {
      const int first = 64 * (cfirst + __builtin_ctzll(cm));
      cm &= cm - 1ull;
      const int n = min(64, S.n_sph - first);
      const uint64_t m = cull ? cull_chunk(S.bound, first, n, *B) : all_bits(n);
      uint32_t pm = pair_bits(m);
      while (pm)
      {
        const int j = (first >> 1) + __builtin_ctz(pm);
        pm &= pm - 1u;
        f2 b, d;
        pair_bd(S.sph_pair[j], o, k, b, d);
        if (live && !occ)
        {
          if constexpr (STATS)
          {
            if (2 * j != skip_sph && sphere_tail<STATS, true>(b.x, d.x, ray, k, t, sq, cnt)) occ = true;
            else if (2 * j + 1 != skip_sph && 2 * j + 1 < S.n_sph &&
                     sphere_tail<STATS, true>(b.y, d.y, ray, k, t, sq, cnt))
              occ = true;
          }
          else if (pair_may_hit(b, d))
          {
            // the hit object is filtered out after its test, which does not change the boolean
            if (sphere_tail<STATS, true, true>(b.x, d.x, ray, k, t, sq, cnt) && 2 * j != skip_sph) occ = true;
            else if (sphere_tail<STATS, true, true>(b.y, d.y, ray, k, t, sq, cnt) && 2 * j + 1 != skip_sph) occ = true;
          }
        }
        if (__ballot(live && !occ) == 0) return occ;
      }
    }
  }
  bool use_tbvh = false;
#if RFX_TRI_BVH
  if constexpr (TBVH && !STATS)
  {
    use_tbvh = S.tri_bvh != nullptr;
    if (use_tbvh && live && !occ) occ = occluded_tris_bvh<STATS>(S, o, ray, k, skip_tri, cnt, ns);
  }
#endif
  for (int first = 0; !use_tbvh && first < S.n_tri; first += 64)
  {
    if (__ballot(live && !occ) == 0) return occ;
    const int n = min(64, S.n_tri - first);
    uint64_t m = (B && B->ok) ? cull_chunk(S.bound, S.n_sph + first, n, *B) : all_bits(n);
    while (m)
    {
      const int i = first + __builtin_ctzll(m);
      m &= m - 1ull;
      if (live && !occ)
      {
        if constexpr (STATS)
        {
          if (i != skip_tri && tri_hit<STATS, true>(S.tri_geo[i], o, ray, t, u, v, sq, cnt, k)) occ = true;
        }
        else if (tri_hit<STATS, true, true>(S.tri_geo[i], o, ray, t, u, v, sq, cnt, k) && i != skip_tri)
          occ = true;
      }
      if (__ballot(live && !occ) == 0) return occ;
    }
  }
  if constexpr (PLANES)
    if (live && !occ) occ = occluded_planes<STATS>(S, o, ray, k, skip_pln, cnt);
  return occ;
}

}  // namespace rfx
