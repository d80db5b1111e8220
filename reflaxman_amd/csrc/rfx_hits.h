// rfx_hits.h -- the two questions Scene::trace asks of a scene on every segment, asked for a batch of rays the caller
// chose (include/rfx.h rfx_query_hits, rfx_query_occluded): no bounce loop, no shading, no random stream.
//
//   query_hits_kernel<CFG>     : one pass of the closest-hit loop (Scene.cpp:82-107) per ray -- the winner's object
//       index, curDist, and what its trace() returned (drop, norm, reflected ray, dropMaterial.color), each plane of
//       results written only where the caller asked for it.
//   query_occluded_kernel<CFG> : the shadow any-hit loop (Scene.cpp:133-143) per ray, over every object but skip[i].
//   launch_hits_cfg            : a run-time cfg to its instantiation (rfx_trace_hits.hip is the one unit that includes
//       this).
//
// One lane per ray, a wave's unit and a lane's ray by ray_slot's rule (rfx_rays.h): 64 consecutive rays, or an 8x8 tile
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

#pragma clang fp contract(off)

namespace rfx {

// the CFG bits a query kernel is instantiated on: never small together with a triangle tree
constexpr int kHitCfgMask = kCfgSmall | kCfgPlanes | kCfgTriBvh;

// A lane's ray in its wave's unit: ray_slot's rule (rfx_rays.h) on a query's own parameters
struct HitSlot {
  uint64_t i;
  bool live;
};
__device__ __forceinline__ uint32_t hit_unit(const HitParams &P, uint32_t wv, uint32_t w8)
{
  // raster mode: the plain frame kernel's grid, workgroup (x, y) the kTileWavesX x kTileWavesY tiles at its place
  return P.W ? (blockIdx.y * kTileWavesY + wv / kTileWavesX) * w8 + blockIdx.x * kTileWavesX + wv % kTileWavesX
             : kWgWaves * blockIdx.x + wv;
}
__device__ __forceinline__ HitSlot hit_slot(const HitParams &P, uint32_t unit, uint32_t w8, uint32_t lane)
{
  HitSlot s;
  if (P.W)
  {
    const uint32_t gx = (unit % w8) * 8u + (lane & 7u), gy = (unit / w8) * 8u + (lane >> 3);
    s.i = (uint64_t)gy * P.W + gx;
    s.live = gx < P.W && s.i < P.n;  // (the last raster row may be partial)
  }
  else
  {
    s.i = 64ull * unit + lane;
    s.live = s.i < P.n;
  }
  return s;
}

// The lane's 24-B record, read first and non-temporally (trace_rays_kernel's order, DESIGN.md "Ray loads"): it comes
// from HBM once, and the staging that follows runs while it is on its way.
__device__ __forceinline__ void load_ray(const HitParams &P, const HitSlot &sl, v3 &o, v3 &d)
{
  o = mk(0.0f, 0.0f, 0.0f);
  d = mk(0.0f, 0.0f, 0.0f);
  if (sl.live)
  {
    const float *f = P.rays + 6u * sl.i;
    o = mk(__builtin_nontemporal_load(f), __builtin_nontemporal_load(f + 1), __builtin_nontemporal_load(f + 2));
    d = mk(__builtin_nontemporal_load(f + 3), __builtin_nontemporal_load(f + 4), __builtin_nontemporal_load(f + 5));
  }
}

__device__ __forceinline__ void store3(float *plane, uint64_t i, v3 v)
{
  float *p = plane + 3u * i;
  p[0] = v.x; p[1] = v.y; p[2] = v.z;
}

template <int CFG>
__global__ __launch_bounds__(kWgThreads) void query_hits_kernel(DevScene S, HitParams P)
{
  static_assert((CFG & ~kHitCfgMask) == 0 && !((CFG & kCfgSmall) && (CFG & kCfgTriBvh)), "a query's CFG bits");
  constexpr bool SMALL = (CFG & kCfgSmall) != 0, PLANES = (CFG & kCfgPlanes) != 0, TBVH = (CFG & kCfgTriBvh) != 0;
  const uint32_t lane = threadIdx.x & 63u, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t w8 = kTileWavesX * gridDim.x;
  const HitSlot sl = hit_slot(P, hit_unit(P, wv, w8), w8, lane);
  const bool live = sl.live;
  v3 o, d;
  load_ray(P, sl, o, d);
  // the colour plane's texels go through Color(ARGB)'s table; nothing here raises a power
  __shared__ float lut[256];
  for (uint32_t i = threadIdx.x; i < 256; i += kWgThreads) lut[i] = (float)i / 255.0f;  // Color.cpp:11-13
  if constexpr (SMALL) stage_small_scene(S);
  __syncthreads();
  Cnt cnt;
  const Tabs<SMALL> T{S};
  Hit h;
  h.obj = -1; h.kind = 0; h.i = 0; h.t = 0.0f; h.u = 0.0f; h.v = 0.0f; h.sq = kNoHitKey;
  if (__ballot(live))  // (a bundle needs a live lane; a raster's edge tiles may hold none)
  {
    const Bundle B = make_bundle(o, d, live);
    if constexpr (SMALL)
    {
      uint64_t om = S.cull_valid;
      if (B.ok) om = cull_small(T.cull(), S.cull_valid, B);
      if (live) closest_hit_small<false, PLANES>(S, o, d, om, h, cnt);
    }
    else
      closest_hit<false, PLANES, TBVH>(S, o, d, live, &B, h, cnt);
  }
  if (!live) return;
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

template <int CFG>
__global__ __launch_bounds__(kWgThreads) void query_occluded_kernel(DevScene S, HitParams P)
{
  static_assert((CFG & ~kHitCfgMask) == 0 && !((CFG & kCfgSmall) && (CFG & kCfgTriBvh)), "a query's CFG bits");
  constexpr bool SMALL = (CFG & kCfgSmall) != 0, PLANES = (CFG & kCfgPlanes) != 0, TBVH = (CFG & kCfgTriBvh) != 0;
  const uint32_t lane = threadIdx.x & 63u, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t w8 = kTileWavesX * gridDim.x;
  const HitSlot sl = hit_slot(P, hit_unit(P, wv, w8), w8, lane);
  const bool live = sl.live;
  v3 o, d;
  load_ray(P, sl, o, d);
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

// ------------------------------------------------------------- launch (rfx_trace_hits.hip)
template <int CFG>
inline void launch_hits_one(bool any, dim3 grid, const DevScene &S, const HitParams &P, hipStream_t st)
{
  if (any) hipLaunchKernelGGL((query_occluded_kernel<CFG>), grid, dim3(kWgThreads), 0, st, S, P);
  else hipLaunchKernelGGL((query_hits_kernel<CFG>), grid, dim3(kWgThreads), 0, st, S, P);
}

inline void launch_hits_cfg(int cfg, bool any, dim3 grid, const DevScene &S, const HitParams &P, hipStream_t st)
{
  switch (cfg)
  {
    case 0: launch_hits_one<0>(any, grid, S, P, st); break;
    case kCfgPlanes: launch_hits_one<kCfgPlanes>(any, grid, S, P, st); break;
    case kCfgSmall: launch_hits_one<kCfgSmall>(any, grid, S, P, st); break;
    case kCfgSmall | kCfgPlanes: launch_hits_one<kCfgSmall | kCfgPlanes>(any, grid, S, P, st); break;
#if RFX_TRI_BVH
    case kCfgTriBvh: launch_hits_one<kCfgTriBvh>(any, grid, S, P, st); break;
    case kCfgTriBvh | kCfgPlanes: launch_hits_one<kCfgTriBvh | kCfgPlanes>(any, grid, S, P, st); break;
#endif
  }
}

}  // namespace rfx
