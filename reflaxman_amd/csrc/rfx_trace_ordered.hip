// The ordered ray-batch and hit-query kernels of librfx.so (rfx_ordered.h) and their launches -- its own TU beside the
// ray batches and the hit queries (reflaxman_amd/_build.py).
#include "rfx_ordered.h"

namespace rfx {

// One launch of P.p_end rays in the order d_order gives (as many slots).  The cfg by launch_trace_rays' rule for a
// launch without counters (rfx_trace_rays.hip).
hipError_t launch_trace_rays_ordered(const DevScene &S, const FrameParams &P_in, const float *d_rays,
                                     const uint32_t *d_order, hipStream_t st)
{
  if (!P_in.p_end) return hipSuccess;
  FrameParams P = P_in;
  P.W = 0;
  set_ray_records(P, d_rays);
  set_ray_order(P, d_order);
  const dim3 grid((uint32_t)(((P.p_end + 63) / 64 + kWgWaves - 1) / kWgWaves));
  const int cfg = (S.n_light > 32 ? kCfgManyLights : 0) | kCfgCull | (S.n_sph <= 32 && S.n_tri <= 32 ? kCfgSmall : 0) |
                  (S.n_pln > 0 ? kCfgPlanes : 0) | (S.n_light == 1 && RFX_ONE_LIGHT ? kCfgOneLight : 0) |
                  (RFX_TRI_BVH && S.tri_bvh != nullptr ? kCfgTriBvh : 0);
  launch_ordered_cfg(cfg, grid, S, P, st);
  return hipGetLastError();
}

// One launch of the slots [P.slot0, P.slot1).  The cfg is launch_query_hits' (rfx_trace_hits.hip).
hipError_t launch_query_hits_ordered(const DevScene &S, const HitOrderParams &P, bool any, hipStream_t st)
{
  if (P.slot1 <= P.slot0) return hipSuccess;
  const dim3 grid((uint32_t)(((P.slot1 - P.slot0 + 63) / 64 + kWgWaves - 1) / kWgWaves));
  const bool small = S.n_sph <= 32 && S.n_tri <= 32;
  const int cfg = (small ? kCfgSmall : 0) | (S.n_pln > 0 ? kCfgPlanes : 0) |
                  (RFX_TRI_BVH && !small && S.tri_bvh != nullptr ? kCfgTriBvh : 0);
  launch_hits_ordered_cfg(cfg, any, grid, S, P, st);
  return hipGetLastError();
}

}  // namespace rfx
