// The path kernels of librfx.so (rfx_paths.h paths_step_kernel over the batches' render cfgs, paths_begin_kernel) and
// their launches -- its own TU beside the batch units (reflaxman_amd/_build.py).
#define RFX_PATHS_DEVICE
#include "rfx_paths.h"
#include "rfx_batch_launch.h"

namespace rfx {

hipError_t launch_paths_begin(const PathPlanes &p, uint64_t m, const uint32_t *rd_state, hipStream_t st)
{
  if (!m) return hipSuccess;
  hipLaunchKernelGGL(paths_begin_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, st, p, m, rd_state);
  return hipGetLastError();
}

// One launch of the slots [P.p_begin, P.trace_base): the cfg is a batch's (batch_trace_cfg, never the stats form)
hipError_t launch_paths_step(const DevScene &S, const FrameParams &P, hipStream_t st)
{
  if (P.trace_base <= P.p_begin) return hipSuccess;
  const dim3 grid = batch_grid(P.trace_base - P.p_begin, 0);
  const bool found = dispatch_trace_cfg<false>(batch_trace_cfg(S, false), [&](auto c) {
    hipLaunchKernelGGL((paths_step_kernel<decltype(c)::value>), grid, dim3(kWgThreads), 0, st, S, P);
  });
  if (!found) return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace rfx
