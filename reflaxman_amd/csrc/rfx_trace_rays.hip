// The ray-batch kernels of librfx.so (rfx_rays.h trace_rays_kernel, render and stats) and their launch --
// its own TU beside the trace_kernel families (reflaxman_amd/_build.py).
#include "rfx_rays.h"
#include "rfx_batch_launch.h"

namespace rfx {

// the render (STATS false) or the counting kernel of cfg; false: the table holds no such cfg
template <bool STATS>
static bool launch_rays(int cfg, dim3 grid, const DevScene &S, const FrameParams &P, hipStream_t st)
{
  return dispatch_trace_cfg<STATS>(cfg, [&](auto c) {
    hipLaunchKernelGGL((trace_rays_kernel<STATS, decltype(c)::value>), grid, dim3(kWgThreads), 0, st, S, P);
  });
}

// One launch of P.p_end rays (rfx_rays.h names the FrameParams fields a batch reads)
hipError_t launch_trace_rays(const DevScene &S, const FrameParams &P_in, const float *d_rays, bool stats,
                             hipStream_t st)
{
  if (!P_in.p_end) return hipSuccess;
  FrameParams P = P_in;
  set_ray_records(P, d_rays);
  const dim3 grid = batch_grid(P.p_end, P.W);
  const int cfg = batch_trace_cfg(S, stats);
  if (!(stats ? launch_rays<true>(cfg, grid, S, P, st) : launch_rays<false>(cfg, grid, S, P, st)))
    return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace rfx
