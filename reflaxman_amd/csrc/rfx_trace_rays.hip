// The ray-batch kernels of librfx.so (rfx_rays.h trace_rays_kernel, render and stats) and their launch --
// its own TU beside the trace_kernel families (reflaxman_amd/_build.py).
#include "rfx_rays.h"

namespace rfx {

// One launch of P.p_end rays (rfx_rays.h names the FrameParams fields a batch reads).  The cfg by launch_trace's rule
// (rfx_kernels.hip): the stats build counts the reference's every test, so it never culls and takes neither the
// one-light nor the triangle-BVH instantiations.
hipError_t launch_trace_rays(const DevScene &S, const FrameParams &P_in, const float *d_rays, bool stats,
                             hipStream_t st)
{
  if (!P_in.p_end) return hipSuccess;
  FrameParams P = P_in;
  set_ray_records(P, d_rays);
  dim3 grid;
  if (P.W)  // the plain frame kernel's grid over the W x ceil(n / W) raster
    grid = dim3((P.W + kTileW - 1) / kTileW, (uint32_t)(((P.p_end + P.W - 1) / P.W + kTileH - 1) / kTileH));
  else
    grid = dim3((uint32_t)(((P.p_end + 63) / 64 + kWgWaves - 1) / kWgWaves));
  const int cfg = (S.n_light > 32 ? kCfgManyLights : 0) | (stats ? 0 : kCfgCull) |
                  (S.n_sph <= 32 && S.n_tri <= 32 ? kCfgSmall : 0) | (S.n_pln > 0 ? kCfgPlanes : 0) |
                  (S.n_light == 1 && !stats && RFX_ONE_LIGHT ? kCfgOneLight : 0) |
                  (RFX_TRI_BVH && S.tri_bvh != nullptr && !stats ? kCfgTriBvh : 0);
  if (stats) launch_rays_cfg<true>(cfg, grid, S, P, st);
  else launch_rays_cfg<false>(cfg, grid, S, P, st);
  return hipGetLastError();
}

}  // namespace rfx
