// rfx_batch_launch.h -- the host side of a batch launch, shared by the three units that make one (rfx_trace_rays.hip,
// rfx_trace_hits.hip, rfx_trace_ordered.hip): the grid, the cfg a scene takes, and the tables from that run-time cfg
// to a compile-time one.  No kernel is named here: a unit instantiates the kernels its own callable launches, and
// those only.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "rfx_types.h"
#include "rfx_shade_inputs.h"

namespace rfx {

// n rays with a lane each: a wave per 64 consecutive ones, or (W != 0) the plain frame kernel's grid over the
// W x ceil(n / W) raster
inline dim3 batch_grid(uint64_t n, uint32_t W)
{
  if (W) return dim3((W + kTileW - 1) / kTileW, (uint32_t)(((n + W - 1) / W + kTileH - 1) / kTileH));
  return dim3((uint32_t)(((n + 63) / 64 + kWgWaves - 1) / kWgWaves));
}

// A trace's cfg by launch_trace's rule (rfx_kernels.hip): the stats build counts the reference's every test, so it
// never culls and takes neither the one-light nor the triangle-BVH instantiations.
inline int batch_trace_cfg(const DevScene &S, bool stats)
{
  return (S.n_light > 32 ? kCfgManyLights : 0) | (stats ? 0 : kCfgCull) |
         (S.n_sph <= 32 && S.n_tri <= 32 ? kCfgSmall : 0) | (S.n_pln > 0 ? kCfgPlanes : 0) |
         (S.n_light == 1 && !stats && RFX_ONE_LIGHT ? kCfgOneLight : 0) |
         (RFX_TRI_BVH && S.tri_bvh != nullptr && !stats ? kCfgTriBvh : 0);
}

// A query's: the same rule for the three bits a query has, a triangle tree only where the scene is not small
inline int batch_query_cfg(const DevScene &S)
{
  const bool small = S.n_sph <= 32 && S.n_tri <= 32;
  return (small ? kCfgSmall : 0) | (S.n_pln > 0 ? kCfgPlanes : 0) |
         (RFX_TRI_BVH && !small && S.tri_bvh != nullptr ? kCfgTriBvh : 0);
}

// The tables: f(std::integral_constant<int, CFG>()) for the entry that cfg names.  False when there is none -- nothing
// was launched, and the caller reports hipErrorInvalidValue.  A matching case calls f and RETURNS true from the table
// (the macro holds the return); the switches have no default, so a cfg that matches nothing falls out of its switch
// and goes on to the next group, and past the last one to `return false`.
#define RFX_CFG_CASE(c) case (c): f(std::integral_constant<int, (c)>()); return true

// launch_cfg's table (rfx_trace.h) without a mode.  The render kernels (STATS false) are the culling cfgs, the odd
// ones; the one-light and triangle-BVH instantiations exist where batch_trace_cfg can produce them, and every other cfg
// drops the bit.  The counting kernels (STATS true) are the even cfgs and take neither bit.
template <bool STATS, class F>
inline bool dispatch_trace_cfg(int cfg, F &&f)
{
#if RFX_TRI_BVH
  if (cfg & kCfgTriBvh)
  {
    if constexpr (!STATS)
      switch (cfg)  // a match returns; no match: drop the bit below
      {
        RFX_CFG_CASE(1 | kCfgTriBvh);
        RFX_CFG_CASE(3 | kCfgTriBvh);
        RFX_CFG_CASE(9 | kCfgTriBvh);
        RFX_CFG_CASE(11 | kCfgTriBvh);
        RFX_CFG_CASE(1 | kCfgOneLight | kCfgTriBvh);
        RFX_CFG_CASE(9 | kCfgOneLight | kCfgTriBvh);
      }
    cfg &= ~kCfgTriBvh;
  }
#endif
  if (cfg & kCfgOneLight)
  {
    if constexpr (!STATS)
      switch (cfg)  // a match returns; no match: drop the bit below
      {
        RFX_CFG_CASE(1 | kCfgOneLight);
        RFX_CFG_CASE(5 | kCfgOneLight);
        RFX_CFG_CASE(9 | kCfgOneLight);
        RFX_CFG_CASE(13 | kCfgOneLight);
      }
    cfg &= ~kCfgOneLight;
  }
  if constexpr (STATS)
    switch (cfg)  // a match returns; no match: not found
    {
      RFX_CFG_CASE(0);
      RFX_CFG_CASE(2);
      RFX_CFG_CASE(4);
      RFX_CFG_CASE(6);
      RFX_CFG_CASE(8);
      RFX_CFG_CASE(10);
      RFX_CFG_CASE(12);
      RFX_CFG_CASE(14);
    }
  else
    switch (cfg)  // a match returns; no match: not found
    {
      RFX_CFG_CASE(1);
      RFX_CFG_CASE(3);
      RFX_CFG_CASE(5);
      RFX_CFG_CASE(7);
      RFX_CFG_CASE(9);
      RFX_CFG_CASE(11);
      RFX_CFG_CASE(13);
      RFX_CFG_CASE(15);
    }
  return false;
}

// the query kernels' cfgs (rfx_hits.h kHitCfgMask): never small together with a triangle tree
template <class F>
inline bool dispatch_query_cfg(int cfg, F &&f)
{
  switch (cfg)  // a match returns; no match: not found
  {
    RFX_CFG_CASE(0);
    RFX_CFG_CASE(kCfgPlanes);
    RFX_CFG_CASE(kCfgSmall);
    RFX_CFG_CASE(kCfgSmall | kCfgPlanes);
#if RFX_TRI_BVH
    RFX_CFG_CASE(kCfgTriBvh);
    RFX_CFG_CASE(kCfgTriBvh | kCfgPlanes);
#endif
  }
  return false;
}

#undef RFX_CFG_CASE

}  // namespace rfx
