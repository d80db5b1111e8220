// The ordered ray-batch and hit-query kernels of librfx.so (rfx_ordered.h) and their launches -- its own TU beside the
// ray batches and the hit queries (reflaxman_amd/_build.py).
#include "rfx_ordered.h"
#include "rfx_batch_launch.h"

namespace rfx {

// One launch of P.p_end rays in the order d_order gives (as many slots), with a ray batch's cfg for a launch without
// counters.
hipError_t launch_trace_rays_ordered(const DevScene &S, const FrameParams &P_in, const float *d_rays,
                                     const uint32_t *d_order, hipStream_t st)
{
  if (!P_in.p_end) return hipSuccess;
  FrameParams P = P_in;
  P.W = 0;
  set_ray_records(P, d_rays);
  set_ray_order(P, d_order);
  const dim3 grid = batch_grid(P.p_end, 0);
  const bool found = dispatch_trace_cfg<false>(batch_trace_cfg(S, false), [&](auto c) {
    hipLaunchKernelGGL((trace_rays_ordered_kernel<decltype(c)::value>), grid, dim3(kWgThreads), 0, st, S, P);
  });
  return found ? hipGetLastError() : hipErrorInvalidValue;
}

// One launch of the slots [P.slot0, P.slot1), with a hit query's cfg
hipError_t launch_query_hits_ordered(const DevScene &S, const HitOrderParams &P, bool any, hipStream_t st)
{
  if (P.slot1 <= P.slot0) return hipSuccess;
  const dim3 grid = batch_grid(P.slot1 - P.slot0, 0);
  const bool found = dispatch_query_cfg(batch_query_cfg(S), [&](auto c) {
    constexpr int CFG = decltype(c)::value;
    if (any) hipLaunchKernelGGL((query_occluded_ordered_kernel<CFG>), grid, dim3(kWgThreads), 0, st, S, P);
    else hipLaunchKernelGGL((query_hits_ordered_kernel<CFG>), grid, dim3(kWgThreads), 0, st, S, P);
  });
  return found ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace rfx
