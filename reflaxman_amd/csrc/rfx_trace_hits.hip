// The hit-query kernels of librfx.so (rfx_hits.h query_hits_kernel, query_occluded_kernel) and their launch -- its own
// TU beside the trace_kernel families and the ray batches (reflaxman_amd/_build.py).
#include "rfx_hits.h"
#include "rfx_launch.h"

namespace rfx {

// One launch of P.n rays.  The grid is a ray batch's (rfx_trace_rays.hip); the cfg keeps launch_trace's rule for the
// three bits a query has.
hipError_t launch_query_hits(const DevScene &S, const HitParams &P, bool any, hipStream_t st)
{
  if (!P.n) return hipSuccess;
  dim3 grid;
  if (P.W)  // the plain frame kernel's grid over the W x ceil(n / W) raster
    grid = dim3((P.W + kTileW - 1) / kTileW, (uint32_t)(((P.n + P.W - 1) / P.W + kTileH - 1) / kTileH));
  else
    grid = dim3((uint32_t)(((P.n + 63) / 64 + kWgWaves - 1) / kWgWaves));
  const bool small = S.n_sph <= 32 && S.n_tri <= 32;
  const int cfg = (small ? kCfgSmall : 0) | (S.n_pln > 0 ? kCfgPlanes : 0) |
                  (RFX_TRI_BVH && !small && S.tri_bvh != nullptr ? kCfgTriBvh : 0);
  launch_hits_cfg(cfg, any, grid, S, P, st);
  return hipGetLastError();
}

}  // namespace rfx
