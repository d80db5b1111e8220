// The hit-query kernels of librfx.so (rfx_hits.h query_hits_kernel, query_occluded_kernel) and their launch -- its own
// TU beside the trace_kernel families and the ray batches (reflaxman_amd/_build.py).
#include "rfx_hits.h"
#include "rfx_launch.h"
#include "rfx_batch_launch.h"

namespace rfx {

// One launch of P.n rays, on a ray batch's grid
hipError_t launch_query_hits(const DevScene &S, const HitParams &P, bool any, hipStream_t st)
{
  if (!P.n) return hipSuccess;
  const dim3 grid = batch_grid(P.n, P.W);
  const bool found = dispatch_query_cfg(batch_query_cfg(S), [&](auto c) {
    constexpr int CFG = decltype(c)::value;
    if (any) hipLaunchKernelGGL((query_occluded_kernel<CFG>), grid, dim3(kWgThreads), 0, st, S, P);
    else hipLaunchKernelGGL((query_hits_kernel<CFG>), grid, dim3(kWgThreads), 0, st, S, P);
  });
  return found ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace rfx
