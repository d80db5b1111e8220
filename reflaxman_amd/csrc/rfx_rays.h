// rfx_rays.h -- Scene::trace (Scene.cpp:73-236) on a batch of rays the caller chose (include/rfx.h rfx_trace_rays).
//
//   trace_rays_kernel<STATS, CFG> : one lane per ray around the frame kernels' bounce loop (rfx_bounce.h trace).  A wave
//       takes 64 consecutive rays, or -- the batch laid out as a row-major raster -- an 8x8 tile of it, the plain frame
//       kernel's coherence.  Either way ray i takes randDir i and writes output i; the layout moves work between waves
//       and changes no value.  A lane reads its own 24-B record, before the workgroup stages its LDS tables so that the
//       wait for HBM overlaps the staging; a full wave's colours leave through LDS as one 16-B store per lane
//       (store_wave_tile, store_wave_run).
//   rfx_rays_body.inc : that kernel's text, written once for every rule that gives a lane its ray (RasterRays here,
//       OrderedRays in rfx_ordered.h) and included in each kernel's body.  The launch tables are rfx_batch_launch.h's.
//
// A batch is no frame: no eye, no view, no tile order, no per-view masks, no parking.  Its launch reuses FrameParams
// as it is (the kernels' arguments are (DevScene, FrameParams), kKernargSig); the fields a batch reads are named below.
#pragma once
#include <hip/hip_runtime.h>

#include "rfx_trace.h"
#include "rfx_ray_slot.h"

#pragma clang fp contract(off)

namespace rfx {

// FrameParams as a ray batch reads it (rfx_rays.cpp fills the frame's fields, launch_trace_rays the borrowed one):
//   W         raster_width: 0 = a wave per 64 consecutive rays, else a wave per 8x8 tile of the W-wide raster
//   p_end     rays of this launch, indexed from 0 (a batch of several launches: every pointer starts at the launch's
//             first ray)
//   depth     reflNumber;  rd_state  ray i's randDir state;  img / argb / counters  as a frame's, one entry per ray
// The ray records (6 floats each: origin, direction) ride in queue_order, the regroup sort's entry list: a batch never
// parks a trace (no kCfgPark instantiation here), so no code this kernel reaches reads that field.
__host__ __device__ inline const float *ray_records(const FrameParams &P)
{
  return reinterpret_cast<const float *>(P.queue_order);
}
inline void set_ray_records(FrameParams &P, const float *d_rays) { P.queue_order = reinterpret_cast<const uint32_t *>(d_rays); }

// Linear mode's store_wave_tile: the wave's 64 colours are 768 contiguous bytes of RGB and 256 of ARGB -- lanes 0-47
// store the RGB's 16-B words, lanes 48-63 the ARGB's.  Call with every lane valid; needs 16-B-aligned outputs.
__device__ __forceinline__ void store_wave_run(const FrameParams &P, uint32_t unit, col out, uint32_t lane, uint32_t wave)
{
  uint32_t *s = s_out[wave];
  s[3 * lane] = __float_as_uint(out.r);
  s[3 * lane + 1] = __float_as_uint(out.g);
  s[3 * lane + 2] = __float_as_uint(out.b);
  s[192 + lane] = argb(out);
  __builtin_amdgcn_wave_barrier();
  const bool rgb = lane < 48;
  const uint4 v = *reinterpret_cast<const uint4 *>(s + 4u * lane);  // words 192..255: the ARGB's
  uint32_t *dst = rgb ? reinterpret_cast<uint32_t *>(P.img) + (size_t)unit * 192u + 4u * lane
                      : P.argb + (size_t)unit * 64u + 4u * (lane - 48u);
  if (rgb || P.argb) *reinterpret_cast<uint4 *>(dst) = v;
}

// A trace kernel's rule for its lanes' rays, made in the kernel (here()): unit() is the wave's unit, slot() the lane's
// ray in it -- read on the FrameParams handed in, which the epilogue re-reads -- and kStaged whether a full wave's
// outputs lie together, so that they may leave by the staged 16-B stores.  This one is ray_slot's (rfx_ray_slot.h): 64
// consecutive rays, or an 8x8 tile of the raster.
struct RasterRays {
  static constexpr bool kStaged = true;
  uint32_t w8;
  static __device__ __forceinline__ RasterRays here() { return {kTileWavesX * gridDim.x}; }
  __device__ __forceinline__ uint32_t unit(const FrameParams &P, uint32_t wv) const { return ray_unit(P, wv, w8); }
  __device__ __forceinline__ RaySlot slot(const FrameParams &P, uint32_t unit, uint32_t lane) const
  {
    return ray_slot(P, unit, w8, lane);
  }
};

template <bool STATS, int CFG>
__global__ __launch_bounds__(kWgThreads) __attribute__((amdgpu_waves_per_eu(
    (CFG & kCfgSmall) ? RFX_WAVES_PER_EU : RFX_WAVES_PER_EU_LARGE))) void trace_rays_kernel(DevScene S, FrameParams P)
{
  static_assert(kKernargSig<decltype(&trace_rays_kernel<STATS, CFG>)>, "launder_scene / kernarg_params layout");
  using Rays = RasterRays;
  __shared__ float lut[256];
#include "rfx_rays_body.inc"  // the kernel's text, on S, P, STATS, CFG, Rays and lut
}

}  // namespace rfx
