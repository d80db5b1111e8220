// rfx_hits.h -- the two questions Scene::trace asks of a scene on every segment, asked for a batch of rays the caller
// chose (include/rfx.h rfx_query_hits, rfx_query_occluded): no bounce loop, no shading, no random stream.
//
//   query_hits_kernel<CFG>     : one pass of the closest-hit loop (Scene.cpp:82-107) per ray -- the winner's object
//       index, curDist, and what its trace() returned (drop, norm, reflected ray, dropMaterial.color), each plane of
//       results written only where the caller asked for it.
//   query_occluded_kernel<CFG> : the shadow any-hit loop (Scene.cpp:133-143) per ray, over every object but skip[i].
//   query_hits_body, query_occluded_body : the two kernels' text, written once: the lane's ray and whether it is live
//       come from the caller (these kernels here, the ordered ones in rfx_ordered.h).  The launch tables are
//       rfx_batch_launch.h's.
//   lane_ray, hit_none, hit_planes_store : a lane's ray, the empty hit record, and the closest hit's output planes --
//       written once for these bodies and the span queries' (rfx_span.h).
//
// One lane per ray, a wave's unit and a lane's ray by ray_slot's rule (rfx_ray_slot.h): 64 consecutive rays, or an 8x8 tile
// of the batch read as a row-major raster.  Every lane of a wave reaches the query -- lanes past the batch's end or
// outside the raster as not live -- so the bundles stay wave-wide, and the queries always take the culling path:
// make_bundle over the live lanes, then cull_small, or closest_hit / occluded with the bundle.  The kernels take their
// own parameter record by value and read it as the compiler sees fit: nothing here goes through the kernarg segment
// pointer (rfx_bounce.h), so the signature is free.
#pragma once
#include <hip/hip_runtime.h>

#include "rfx_math.h"
#include "rfx_types.h"
#include "rfx_shade_inputs.h"
#include "rfx_queries.h"
#include "rfx_ray_slot.h"

#pragma clang fp contract(off)

namespace rfx {

// the CFG bits a query kernel is instantiated on: never small together with a triangle tree
constexpr int kHitCfgMask = kCfgSmall | kCfgPlanes | kCfgTriBvh;

__device__ __forceinline__ void store3(float *plane, uint64_t i, v3 v)
{
  float *p = plane + 3u * i;
  p[0] = v.x; p[1] = v.y; p[2] = v.z;
}

// The lane's slot of a linear or raster query: ray_slot's rule on the query's own parameters
__device__ __forceinline__ RaySlot hit_slot(const HitParams &P)
{
  const uint32_t lane = threadIdx.x & 63u, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t w8 = kTileWavesX * gridDim.x;
  return ray_slot(P, ray_unit(P, wv, w8), w8, lane);
}

// The lane's ray: ray i of `rays` in a live lane, zero in every other
__device__ __forceinline__ RayRecord lane_ray(const float *rays, uint64_t i, bool live)
{
  RayRecord r;
  r.o = r.d = mk(0.0f, 0.0f, 0.0f);
  if (live) r = load_ray(rays, i);
  return r;
}

// The closest-hit record before any candidate is taken
__device__ __forceinline__ Hit hit_none()
{
  Hit h;
  h.obj = -1; h.kind = 0; h.i = 0; h.t = 0.0f; h.u = 0.0f; h.v = 0.0f; h.sq = kNoHitKey;
  return h;
}

// A live lane's planes of P from its closest-hit record h (h.obj < 0: the miss values) for the ray (o, d): the one place
// a plane is computed and stored, for the plain queries' body below and the span queries' (rfx_span.h).  lut: the
// kernel's Color(ARGB) table.
template <int CFG>
__device__ __forceinline__ void hit_planes_store(const DevScene &S, const HitParams &P, const RaySlot &sl, v3 o, v3 d,
                                                 const Hit &h, const float *lut, Cnt &cnt)
{
  constexpr bool SMALL = (CFG & kCfgSmall) != 0, PLANES = (CFG & kCfgPlanes) != 0;
  const Tabs<SMALL> T{S};
  // Scene.cpp:82: curDist starts at FLT_MAX, the hit object at none
  const bool hit = h.obj >= 0;
  if (P.object) P.object[sl.i] = hit ? h.obj : -1;
  if (P.distance) P.distance[sl.i] = hit ? sqrt_rn(h.sq) : __FLT_MAX__;
  if (!(P.point || P.normal || P.reflected || P.colour)) return;
  // the winner's outputs, re-derived with the reference's expressions as the bounce loop derives them (trace_from)
  v3 drop = mk(0.0f, 0.0f, 0.0f), norm = drop, refl = drop;
  col c = mkc(0.0f, 0.0f, 0.0f);
  if (hit)
  {
    drop = add(o, mul(d, h.t));
    MatRec m;
    if (h.kind == 0)
    {
      const SphereGeo g = T.sph_geo(h.i);
      norm = sub(drop, mk(g.cx, g.cy, g.cz));                                  // Sphere.cpp:67
      m = T.sph_mat(h.i);
    }
    else if (!PLANES || h.kind == 1)
    {
      const TriShade sh = T.tri_shade(h.i);
      norm = mk(sh.nx, sh.ny, sh.nz);
      m = T.tri_mat(h.i);
      if (P.colour && sh.tex >= 0)                                             // Triangle.cpp:89-96
      {
        const col tc = tri_texel<false>(S, sh, h.u, h.v, lut, cnt);
        m.r = tc.r; m.g = tc.g; m.b = tc.b;
      }
    }
    else
    {
      const PlaneGeo g = S.pln_geo[h.i];
      norm = mk(g.nx, g.ny, g.nz);                                             // Plane.cpp:58-59
      m = S.pln_mat[h.i];                                                      // untextured (Plane.cpp:67-68)
    }
    c = mkc(m.r, m.g, m.b);
    refl = reflect(mul(d, h.t), norm);                                         // trace_math.cpp:14-23
  }
  if (P.point) store3(P.point, sl.i, drop);
  if (P.normal) store3(P.normal, sl.i, norm);
  if (P.reflected) store3(P.reflected, sl.i, refl);
  if (P.colour) store3(P.colour, sl.i, mk(c.r, c.g, c.b));
}

// sl: the lane's ray among P's arrays, and whether the lane is live.  lut: the calling kernel's own 256-entry LDS table
// (declared there, so that each kernel's LDS layout is its own).
template <int CFG>
__device__ __forceinline__ void query_hits_body(const DevScene &S, const HitParams &P, const RaySlot &sl, float *lut)
{
  static_assert((CFG & ~kHitCfgMask) == 0 && !((CFG & kCfgSmall) && (CFG & kCfgTriBvh)), "a query's CFG bits");
  constexpr bool SMALL = (CFG & kCfgSmall) != 0, PLANES = (CFG & kCfgPlanes) != 0, TBVH = (CFG & kCfgTriBvh) != 0;
  const bool live = sl.valid;
  const RayRecord r = lane_ray(P.rays, sl.i, live);
  const v3 o = r.o, d = r.d;
  // the colour plane's texels go through Color(ARGB)'s table; nothing here raises a power
  for (uint32_t i = threadIdx.x; i < 256; i += kWgThreads) lut[i] = (float)i / 255.0f;  // Color.cpp:11-13
  if constexpr (SMALL) stage_small_scene(S);
  __syncthreads();
  Cnt cnt;
  Hit h = hit_none();
  if (__ballot(live))  // (a bundle needs a live lane; a raster's edge tiles may hold none)
  {
    const Bundle B = make_bundle(o, d, live);
    if constexpr (SMALL)
    {
      const Tabs<SMALL> T{S};
      uint64_t om = S.cull_valid;
      if (B.ok) om = cull_small(T.cull(), S.cull_valid, B);
      if (live) closest_hit_small<false, PLANES>(S, o, d, om, h, cnt);
    }
    else
      closest_hit<false, PLANES, TBVH>(S, o, d, live, &B, h, cnt);
  }
  if (live) hit_planes_store<CFG>(S, P, sl, o, d, h, lut, cnt);
}

template <int CFG>
__device__ __forceinline__ void query_occluded_body(const DevScene &S, const HitParams &P, const RaySlot &sl)
{
  static_assert((CFG & ~kHitCfgMask) == 0 && !((CFG & kCfgSmall) && (CFG & kCfgTriBvh)), "a query's CFG bits");
  constexpr bool SMALL = (CFG & kCfgSmall) != 0, PLANES = (CFG & kCfgPlanes) != 0, TBVH = (CFG & kCfgTriBvh) != 0;
  const bool live = sl.valid;
  const RayRecord r = lane_ray(P.rays, sl.i, live);
  const v3 o = r.o, d = r.d;
  // the object left out, as (kind, index within its kind's device arrays): kat_objects' decode of obj_loc
  int skip_sph = -1, skip_tri = -1, skip_pln = -1;
  if (live && P.skip)
  {
    const int32_t sk = __builtin_nontemporal_load(P.skip + sl.i);
    if (sk >= 0 && sk < S.n_obj)
    {
      const int32_t loc = S.obj_loc[sk];
      const int kind = loc >> 28, idx = loc & 0x0FFFFFFF;
      if (kind == 0) skip_sph = idx;
      else if (kind == 1) skip_tri = idx;
      else skip_pln = idx;
    }
  }
  if constexpr (SMALL)
  {
    stage_small_scene(S);
    __syncthreads();
  }
  Cnt cnt;
  bool occ = false;
  if (__ballot(live))
  {
    const Bundle B = make_bundle(o, d, live);
    if constexpr (SMALL)
    {
      const Tabs<SMALL> T{S};
      uint64_t om = S.cull_valid;
      if (B.ok) om = cull_small(T.cull(), S.cull_valid, B);
      if (live) occ = occluded_small<false, PLANES>(S, o, d, skip_sph, skip_tri, skip_pln, om, cnt);
    }
    else
      occ = occluded<false, PLANES, TBVH>(S, o, d, live, skip_sph, skip_tri, skip_pln, &B, cnt);
  }
  if (live) P.occluded[sl.i] = occ ? 1 : 0;
}

template <int CFG>
__global__ __launch_bounds__(kWgThreads) void query_hits_kernel(DevScene S, HitParams P)
{
  __shared__ float lut[256];
  query_hits_body<CFG>(S, P, hit_slot(P), lut);
}

template <int CFG>
__global__ __launch_bounds__(kWgThreads) void query_occluded_kernel(DevScene S, HitParams P)
{
  query_occluded_body<CFG>(S, P, hit_slot(P));
}

}  // namespace rfx
