// The span-query kernels of librfx.so (rfx_span.h query_hits_span_kernel, query_occluded_span_kernel, linear / raster
// and ordered) and their launch -- its own TU beside the hit queries (reflaxman_amd/_build.py).
#include "rfx_span.h"
#include "rfx_batch_launch.h"

namespace rfx {

// One launch of P.H.n rays on a ray batch's grid, or (P.order) of the slots [P.slot0, P.slot1) on a linear one
hipError_t launch_query_span(const DevScene &S, const SpanParams &P, bool any, hipStream_t st)
{
  const bool ordered = P.order != nullptr;
  if (ordered ? P.slot1 <= P.slot0 : !P.H.n) return hipSuccess;
  const dim3 grid = ordered ? batch_grid(P.slot1 - P.slot0, 0) : batch_grid(P.H.n, P.H.W);
  const bool found = dispatch_query_cfg(batch_query_cfg(S), [&](auto c) {
    constexpr int CFG = decltype(c)::value;
    if (any)
    {
      if (ordered) hipLaunchKernelGGL((query_occluded_span_kernel<CFG, true>), grid, dim3(kWgThreads), 0, st, S, P);
      else hipLaunchKernelGGL((query_occluded_span_kernel<CFG, false>), grid, dim3(kWgThreads), 0, st, S, P);
    }
    else if (ordered) hipLaunchKernelGGL((query_hits_span_kernel<CFG, true>), grid, dim3(kWgThreads), 0, st, S, P);
    else hipLaunchKernelGGL((query_hits_span_kernel<CFG, false>), grid, dim3(kWgThreads), 0, st, S, P);
  });
  return found ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace rfx
