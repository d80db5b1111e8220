// rfx_ray_slot.h -- which ray a lane of a batch kernel takes, and its record's load: what the ray batches (rfx_rays.h),
// the hit queries (rfx_hits.h) and their ordered forms (rfx_ordered.h) share below their kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "rfx_math.h"
#include "rfx_types.h"
#include "rfx_shade_inputs.h"

namespace rfx {

// The rays of one launch, whichever record describes it: a trace's FrameParams (rfx_rays.h) or a query's HitParams.
// Both carry the raster width in W.
__device__ __forceinline__ uint64_t ray_count(const FrameParams &P) { return P.p_end; }
__device__ __forceinline__ uint64_t ray_count(const HitParams &P) { return P.n; }

// The lane's ray in its wave's unit (the wave's index in linear mode, its tile of the tile grid w8 wide in raster
// mode): the one slot record and the one raster / linear rule of every batch kernel
struct RaySlot {
  uint64_t i;          // ray index in the launch
  uint32_t x0, row0;   // raster mode: the tile's first column and row
  bool valid;
};
// raster mode: the plain frame kernel's grid, workgroup (x, y) the kTileWavesX x kTileWavesY tiles at its place
template <class Params>
__device__ __forceinline__ uint32_t ray_unit(const Params &P, uint32_t wv, uint32_t w8)
{
  return P.W ? (blockIdx.y * kTileWavesY + wv / kTileWavesX) * w8 + blockIdx.x * kTileWavesX + wv % kTileWavesX
             : kWgWaves * blockIdx.x + wv;
}
template <class Params>
__device__ __forceinline__ RaySlot ray_slot(const Params &P, uint32_t unit, uint32_t w8, uint32_t lane)
{
  RaySlot s;
  if (P.W)
  {
    s.x0 = (unit % w8) * 8u;
    s.row0 = (unit / w8) * 8u;
    const uint32_t gx = s.x0 + (lane & 7u), gy = s.row0 + (lane >> 3);
    s.i = (uint64_t)gy * P.W + gx;
    s.valid = gx < P.W && s.i < ray_count(P);  // (the last raster row may be partial)
  }
  else
  {
    s.x0 = s.row0 = 0;
    s.i = 64ull * unit + lane;
    s.valid = s.i < ray_count(P);
  }
  return s;
}

// Ray i's 24-B record, read non-temporally (the records should not push BVH nodes out of the L2).  A batch kernel
// reads its lane's first (DESIGN.md "Ray loads"): it comes from HBM once, and the staging that follows runs while it
// is on its way.
struct RayRecord { v3 o, d; };
__device__ __forceinline__ RayRecord load_ray(const float *rays, uint64_t i)
{
  const float *f = rays + 6u * i;
  RayRecord r;
  r.o = mk(__builtin_nontemporal_load(f), __builtin_nontemporal_load(f + 1), __builtin_nontemporal_load(f + 2));
  r.d = mk(__builtin_nontemporal_load(f + 3), __builtin_nontemporal_load(f + 4), __builtin_nontemporal_load(f + 5));
  return r;
}

}  // namespace rfx
