// rfx_ordered.h -- the ray batch and the hit queries run in an order the caller gives (include/rfx.h
// rfx_trace_rays_ordered, rfx_query_hits_ordered, rfx_query_occluded_ordered).
//
// The kernels are trace_rays_kernel (rfx_rays.h), query_hits_kernel and query_occluded_kernel (rfx_hits.h) with one
// change: a lane's ray is not its slot but order[slot].  Wave w takes the slots 64 w .. 64 w + 63; the record, the
// randDir state, the skip entry and every output are indexed by the ray, so for a permutation every word is the
// unordered call's and only the company a ray keeps in its wave changes.  A slot past the launch's end, or one whose
// index is not a ray of the batch, is a dead lane: it reads and writes nothing, and reaches the wave-wide code as an
// invalid lane does.  Outputs leave per lane (12-B and 4-B stores): a wave's rays are nowhere near each other, so the
// staged 16-B forms of the unordered kernels do not apply.  There is no stats form.
// rfx_trace_ordered.hip is the one unit that includes this.  It does not include rfx_hits.h, whose launch table would
// instantiate the unordered query kernels a second time here: the three small helpers the queries share are restated.
#pragma once
#include <hip/hip_runtime.h>

#include "rfx_rays.h"
#include "rfx_launch.h"

#pragma clang fp contract(off)

namespace rfx {

// FrameParams as an ordered batch reads it: a linear batch's fields (rfx_rays.h; W = 0, p_end rays and as many slots),
// and the index array in tile_order, the frame kernels' tile schedule, which no code a batch reaches reads.
__host__ __device__ inline const uint32_t *ray_order(const FrameParams &P) { return P.tile_order; }
inline void set_ray_order(FrameParams &P, const uint32_t *d_order) { P.tile_order = d_order; }

struct OrderedSlot {
  uint64_t i;  // the ray
  bool valid;
};
__device__ __forceinline__ OrderedSlot ordered_slot(const uint32_t *order, uint64_t slot, uint64_t slots, uint64_t rays)
{
  OrderedSlot s;
  s.i = 0;
  s.valid = slot < slots;
  if (s.valid)
  {
    s.i = order[slot];
    s.valid = s.i < rays;
  }
  return s;
}

template <int CFG>
__global__ __launch_bounds__(kWgThreads) __attribute__((amdgpu_waves_per_eu(
    (CFG & kCfgSmall) ? RFX_WAVES_PER_EU : RFX_WAVES_PER_EU_LARGE))) void trace_rays_ordered_kernel(DevScene S, FrameParams P)
{
  static_assert(kKernargSig<decltype(&trace_rays_ordered_kernel<CFG>)>, "launder_scene / kernarg_params layout");
  static_assert(!(CFG & kCfgPark), "a ray batch never parks (ray_records rides in a parking field)");
  static_assert((CFG & kCfgCull) != 0, "no stats form: every ordered launch culls");
  constexpr bool MANYL = (CFG & kCfgManyLights) != 0, SMALL = (CFG & kCfgSmall) != 0;
  constexpr bool PLANES = (CFG & kCfgPlanes) != 0, ONEL = (CFG & kCfgOneLight) != 0, TBVH = (CFG & kCfgTriBvh) != 0;
  const uint32_t lane = threadIdx.x & 63u, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t unit = kWgWaves * blockIdx.x + wv;
  // the unit waits in LDS across the bounce loop: the epilogue re-derives the lane's ray from it (as trace_rays_kernel)
  if (lane == 0) s_tile8[wv] = unit;
  const OrderedSlot sl = ordered_slot(ray_order(P), 64ull * unit + lane, P.p_end, P.p_end);
  const bool valid = sl.valid;
  // the record and the randDir state first, the staging while they are on their way (trace_rays_kernel's order)
  v3 o = mk(0.0f, 0.0f, 0.0f), d = mk(0.0f, 0.0f, 0.0f);
  uint32_t rds = 0;
  if (valid)
  {
    const float *f = ray_records(P) + 6u * sl.i;
    o = mk(__builtin_nontemporal_load(f), __builtin_nontemporal_load(f + 1), __builtin_nontemporal_load(f + 2));
    d = mk(__builtin_nontemporal_load(f + 3), __builtin_nontemporal_load(f + 4), __builtin_nontemporal_load(f + 5));
    rds = P.rd_state[sl.i];
  }
  __shared__ float lut[256];
  for (uint32_t i = threadIdx.x; i < 256; i += kWgThreads) lut[i] = (float)i / 255.0f;  // Color.cpp:11-13
  stage_powf_tables();
  if constexpr (SMALL) stage_small_scene(S);
  __syncthreads();
  Cnt cnt;
  const v3 rd = valid ? rd_from_state(rds) : mk(0.0f, 0.0f, 0.0f);
  const col out = trace<false, true, MANYL, SMALL, PLANES, ONEL, TBVH>(S, o, d, P.depth, rd, lut, cnt, valid);
  {
#ifdef RFX_LAUNDER_PARAMS
    const FrameParams &P = kernarg_params();  // shadows the by-value parameter: re-read after the bounce loop
#endif
    const uint32_t ue = ((volatile uint32_t *)s_tile8)[wv];
    uint32_t le = lane;
    asm volatile("" : "+v"(le));  // a fresh lane value: the ray's index is read again, not kept live
    const OrderedSlot se = ordered_slot(ray_order(P), 64ull * ue + le, P.p_end, P.p_end);
    if (se.valid)
    {
      float *p = P.img + se.i * 3;
      p[0] = out.r; p[1] = out.g; p[2] = out.b;
      if (P.argb) P.argb[se.i] = argb(out);
    }
  }
}

// the CFG bits a query kernel is instantiated on (rfx_hits.h kHitCfgMask): never small together with a triangle tree
constexpr int kOrderedHitCfgMask = kCfgSmall | kCfgPlanes | kCfgTriBvh;

// A lane's slot of an ordered query: wave w of the launch takes the slots slot0 + 64 w .. of [slot0, slot1)
struct OrderedHitSlot {
  uint64_t i;
  bool live;
};
__device__ __forceinline__ OrderedHitSlot ordered_hit_slot(const HitOrderParams &P, uint32_t wv, uint32_t lane)
{
  const OrderedSlot s = ordered_slot(P.order, P.slot0 + 64ull * (kWgWaves * blockIdx.x + wv) + lane, P.slot1, P.H.n);
  OrderedHitSlot h;
  h.i = s.i;
  h.live = s.valid;
  return h;
}

// rfx_hits.h load_ray: the lane's 24-B record, read first and non-temporally
__device__ __forceinline__ void ordered_load_ray(const HitParams &P, const OrderedHitSlot &sl, v3 &o, v3 &d)
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

__device__ __forceinline__ void ordered_store3(float *plane, uint64_t i, v3 v)
{
  float *p = plane + 3u * i;
  p[0] = v.x; p[1] = v.y; p[2] = v.z;
}

// query_hits_kernel (rfx_hits.h) on order[slot]
template <int CFG>
__global__ __launch_bounds__(kWgThreads) void query_hits_ordered_kernel(DevScene S, HitOrderParams Q)
{
  static_assert((CFG & ~kOrderedHitCfgMask) == 0 && !((CFG & kCfgSmall) && (CFG & kCfgTriBvh)), "a query's CFG bits");
  constexpr bool SMALL = (CFG & kCfgSmall) != 0, PLANES = (CFG & kCfgPlanes) != 0, TBVH = (CFG & kCfgTriBvh) != 0;
  const HitParams &P = Q.H;
  const uint32_t lane = threadIdx.x & 63u, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const OrderedHitSlot sl = ordered_hit_slot(Q, wv, lane);
  const bool live = sl.live;
  v3 o, d;
  ordered_load_ray(P, sl, o, d);
  __shared__ float lut[256];
  for (uint32_t i = threadIdx.x; i < 256; i += kWgThreads) lut[i] = (float)i / 255.0f;  // Color.cpp:11-13
  if constexpr (SMALL) stage_small_scene(S);
  __syncthreads();
  Cnt cnt;
  const Tabs<SMALL> T{S};
  Hit h;
  h.obj = -1; h.kind = 0; h.i = 0; h.t = 0.0f; h.u = 0.0f; h.v = 0.0f; h.sq = kNoHitKey;
  if (__ballot(live))  // (a bundle needs a live lane)
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
  // the winner's outputs, with the reference's expressions as query_hits_kernel derives them
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
  if (P.point) ordered_store3(P.point, sl.i, drop);
  if (P.normal) ordered_store3(P.normal, sl.i, norm);
  if (P.reflected) ordered_store3(P.reflected, sl.i, refl);
  if (P.colour) ordered_store3(P.colour, sl.i, mk(c.r, c.g, c.b));
}

// query_occluded_kernel (rfx_hits.h) on order[slot]
template <int CFG>
__global__ __launch_bounds__(kWgThreads) void query_occluded_ordered_kernel(DevScene S, HitOrderParams Q)
{
  static_assert((CFG & ~kOrderedHitCfgMask) == 0 && !((CFG & kCfgSmall) && (CFG & kCfgTriBvh)), "a query's CFG bits");
  constexpr bool SMALL = (CFG & kCfgSmall) != 0, PLANES = (CFG & kCfgPlanes) != 0, TBVH = (CFG & kCfgTriBvh) != 0;
  const HitParams &P = Q.H;
  const uint32_t lane = threadIdx.x & 63u, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const OrderedHitSlot sl = ordered_hit_slot(Q, wv, lane);
  const bool live = sl.live;
  v3 o, d;
  ordered_load_ray(P, sl, o, d);
  // the object left out, as (kind, index within its kind's device arrays): query_occluded_kernel's decode
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

// ------------------------------------------------------------- launch (rfx_trace_ordered.hip)
template <int CFG>
inline void launch_ordered_one(dim3 grid, const DevScene &S, const FrameParams &P, hipStream_t st)
{
  hipLaunchKernelGGL((trace_rays_ordered_kernel<CFG>), grid, dim3(kWgThreads), 0, st, S, P);
}

// launch_rays_cfg<false>'s table (rfx_rays.h): the culling configurations, the one-light and triangle-BVH
// instantiations where launch_trace_rays' rule can produce them
inline void launch_ordered_cfg(int cfg, dim3 grid, const DevScene &S, const FrameParams &P, hipStream_t st)
{
#if RFX_TRI_BVH
  if (cfg & kCfgTriBvh)
  {
    switch (cfg & ~kCfgTriBvh)
    {
      case 1: launch_ordered_one<1 | kCfgTriBvh>(grid, S, P, st); return;
      case 3: launch_ordered_one<3 | kCfgTriBvh>(grid, S, P, st); return;
      case 9: launch_ordered_one<9 | kCfgTriBvh>(grid, S, P, st); return;
      case 11: launch_ordered_one<11 | kCfgTriBvh>(grid, S, P, st); return;
      case 1 | kCfgOneLight: launch_ordered_one<1 | kCfgOneLight | kCfgTriBvh>(grid, S, P, st); return;
      case 9 | kCfgOneLight: launch_ordered_one<9 | kCfgOneLight | kCfgTriBvh>(grid, S, P, st); return;
    }
    cfg &= ~kCfgTriBvh;
  }
#endif
  if (cfg & kCfgOneLight)
  {
    switch (cfg & ~kCfgOneLight)
    {
      case 1: launch_ordered_one<1 | kCfgOneLight>(grid, S, P, st); return;
      case 5: launch_ordered_one<5 | kCfgOneLight>(grid, S, P, st); return;
      case 9: launch_ordered_one<9 | kCfgOneLight>(grid, S, P, st); return;
      case 13: launch_ordered_one<13 | kCfgOneLight>(grid, S, P, st); return;
    }
    cfg &= ~kCfgOneLight;
  }
  switch (cfg)
  {
    case 1: launch_ordered_one<1>(grid, S, P, st); break;
    case 3: launch_ordered_one<3>(grid, S, P, st); break;
    case 5: launch_ordered_one<5>(grid, S, P, st); break;
    case 7: launch_ordered_one<7>(grid, S, P, st); break;
    case 9: launch_ordered_one<9>(grid, S, P, st); break;
    case 11: launch_ordered_one<11>(grid, S, P, st); break;
    case 13: launch_ordered_one<13>(grid, S, P, st); break;
    case 15: launch_ordered_one<15>(grid, S, P, st); break;
  }
}

template <int CFG>
inline void launch_hits_ordered_one(bool any, dim3 grid, const DevScene &S, const HitOrderParams &P, hipStream_t st)
{
  if (any) hipLaunchKernelGGL((query_occluded_ordered_kernel<CFG>), grid, dim3(kWgThreads), 0, st, S, P);
  else hipLaunchKernelGGL((query_hits_ordered_kernel<CFG>), grid, dim3(kWgThreads), 0, st, S, P);
}

inline void launch_hits_ordered_cfg(int cfg, bool any, dim3 grid, const DevScene &S, const HitOrderParams &P,
                                    hipStream_t st)
{
  switch (cfg)
  {
    case 0: launch_hits_ordered_one<0>(any, grid, S, P, st); break;
    case kCfgPlanes: launch_hits_ordered_one<kCfgPlanes>(any, grid, S, P, st); break;
    case kCfgSmall: launch_hits_ordered_one<kCfgSmall>(any, grid, S, P, st); break;
    case kCfgSmall | kCfgPlanes: launch_hits_ordered_one<kCfgSmall | kCfgPlanes>(any, grid, S, P, st); break;
#if RFX_TRI_BVH
    case kCfgTriBvh: launch_hits_ordered_one<kCfgTriBvh>(any, grid, S, P, st); break;
    case kCfgTriBvh | kCfgPlanes: launch_hits_ordered_one<kCfgTriBvh | kCfgPlanes>(any, grid, S, P, st); break;
#endif
  }
}

}  // namespace rfx
