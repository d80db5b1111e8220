// rfx_rays.h -- Scene::trace (Scene.cpp:73-236) on a batch of rays the caller chose (include/rfx.h rfx_trace_rays).
//
//   trace_rays_kernel<STATS, CFG> : one lane per ray around the frame kernels' bounce loop (rfx_bounce.h trace).  A wave
//       takes 64 consecutive rays, or -- the batch laid out as a row-major raster -- an 8x8 tile of it, the plain frame
//       kernel's coherence.  Either way ray i takes randDir i and writes output i; the layout moves work between waves
//       and changes no value.  A lane reads its own 24-B record, before the workgroup stages its LDS tables so that the
//       wait for HBM overlaps the staging; a full wave's colours leave through LDS as one 16-B store per lane
//       (store_wave_tile, store_wave_run).
//   launch_rays_cfg : a run-time cfg to its instantiation (rfx_trace_rays.hip is the one unit that includes this).
//
// A batch is no frame: no eye, no view, no tile order, no per-view masks, no parking.  Its launch reuses FrameParams
// as it is (the kernels' arguments are (DevScene, FrameParams), kKernargSig); the fields a batch reads are named below.
#pragma once
#include <hip/hip_runtime.h>

#include "rfx_trace.h"

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

// The lane's ray in its wave's unit (the wave's index in linear mode, its tile of the tile grid w8 wide in raster mode)
struct RaySlot {
  uint64_t i;          // ray index in the launch
  uint32_t x0, row0;   // raster mode: the tile's first column and row
  bool valid;
};
__device__ __forceinline__ RaySlot ray_slot(const FrameParams &P, uint32_t unit, uint32_t w8, uint32_t lane)
{
  RaySlot s;
  if (P.W)
  {
    s.x0 = (unit % w8) * 8u;
    s.row0 = (unit / w8) * 8u;
    const uint32_t gx = s.x0 + (lane & 7u), gy = s.row0 + (lane >> 3);
    s.i = (uint64_t)gy * P.W + gx;
    s.valid = gx < P.W && s.i < P.p_end;  // (the last raster row may be partial)
  }
  else
  {
    s.x0 = s.row0 = 0;
    s.i = 64ull * unit + lane;
    s.valid = s.i < P.p_end;
  }
  return s;
}

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

// Every lane of a wave reaches trace() -- lanes past the batch's end or outside the raster as invalid -- so the bounce
// loop's bundles stay wave-wide; with no per-view mask the first segment builds its bundle from what the lanes hold,
// and a wide cone takes the unculled or per-lane BVH path as an incoherent secondary segment does.
template <bool STATS, int CFG>
__global__ __launch_bounds__(kWgThreads) __attribute__((amdgpu_waves_per_eu(
    (CFG & kCfgSmall) ? RFX_WAVES_PER_EU : RFX_WAVES_PER_EU_LARGE))) void trace_rays_kernel(DevScene S, FrameParams P)
{
  static_assert(kKernargSig<decltype(&trace_rays_kernel<STATS, CFG>)>, "launder_scene / kernarg_params layout");
  static_assert(!(CFG & kCfgPark), "a ray batch never parks (ray_records rides in a parking field)");
  constexpr bool CULL = (CFG & kCfgCull) != 0, MANYL = (CFG & kCfgManyLights) != 0, SMALL = (CFG & kCfgSmall) != 0;
  constexpr bool PLANES = (CFG & kCfgPlanes) != 0, ONEL = (CFG & kCfgOneLight) != 0, TBVH = (CFG & kCfgTriBvh) != 0;
  const uint32_t lane = threadIdx.x & 63u, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // raster mode: the plain frame kernel's grid, workgroup (x, y) the kTileWavesX x kTileWavesY tiles at its place
  const uint32_t w8 = kTileWavesX * gridDim.x;
  const uint32_t unit = P.W ? (blockIdx.y * kTileWavesY + wv / kTileWavesX) * w8 + blockIdx.x * kTileWavesX + wv % kTileWavesX
                            : kWgWaves * blockIdx.x + wv;
  // the unit waits in LDS across the bounce loop: the epilogue re-derives the lane's ray from it (as trace_kernel does)
  if (lane == 0) s_tile8[wv] = unit;
  const RaySlot sl = ray_slot(P, unit, w8, lane);
  const bool valid = sl.valid;
  // The lane's record and randDir state are read first: they come from HBM once and are never read again, and the
  // staging below (L2-resident tables, a workgroup barrier) runs while they are on their way.  One 24-B read per lane,
  // non-temporal (the records should not push BVH nodes out of the L2); the same records as 16-B-per-lane loads through
  // LDS measured 0.7 - 1.0% slower (DESIGN.md "Ray batches").
  v3 o = mk(0.0f, 0.0f, 0.0f), d = mk(0.0f, 0.0f, 0.0f);
  uint32_t rds = 0;
  if (valid)
  {
    const float *f = ray_records(P) + 6u * sl.i;
    o = mk(__builtin_nontemporal_load(f), __builtin_nontemporal_load(f + 1), __builtin_nontemporal_load(f + 2));
    d = mk(__builtin_nontemporal_load(f + 3), __builtin_nontemporal_load(f + 4), __builtin_nontemporal_load(f + 5));
    rds = P.rd_state[sl.i];
  }
  __shared__ float lut[256];
  for (uint32_t i = threadIdx.x; i < 256; i += kWgThreads) lut[i] = (float)i / 255.0f;  // Color.cpp:11-13
  stage_powf_tables();
  if constexpr (SMALL) stage_small_scene(S);
  __syncthreads();
  Cnt cnt;
  if constexpr (STATS)
  {
#pragma unroll
    for (int k = 0; k < C_COUNT; ++k) cnt.c[k] = 0;
  }
  const v3 rd = valid ? rd_from_state(rds) : mk(0.0f, 0.0f, 0.0f);
  const col out = trace<STATS, CULL, MANYL, SMALL, PLANES, ONEL, TBVH>(S, o, d, P.depth, rd, lut, cnt, valid);
  {
#ifdef RFX_LAUNDER_PARAMS
    const FrameParams &P = kernarg_params();  // shadows the by-value parameter: re-read after the bounce loop
#endif
    const uint32_t ue = ((volatile uint32_t *)s_tile8)[wv];
    uint32_t le = lane;
    asm volatile("" : "+v"(le));  // a fresh lane value: the ray's index is recomputed, not kept live
    const RaySlot se = ray_slot(P, ue, w8, le);
    const bool aligned = ((reinterpret_cast<uintptr_t>(P.img) | reinterpret_cast<uintptr_t>(P.argb)) & 15u) == 0;
    const bool staged = aligned && (P.W & 3u) == 0 && __builtin_amdgcn_ballot_w64(se.valid) == ~0ull;
    if (staged && P.W)
      store_wave_tile(P, se.x0, se.row0, out, le, wv);
    else if (staged)
      store_wave_run(P, ue, out, le, wv);
    else if (se.valid)
    {
      float *p = P.img + se.i * 3;
      p[0] = out.r; p[1] = out.g; p[2] = out.b;
      if (P.argb) P.argb[se.i] = argb(out);
    }
    flush_counters<STATS>(P, cnt);
  }
}

// ------------------------------------------------------------- launch (rfx_trace_rays.hip)
template <bool STATS, int CFG>
inline void launch_rays_one(dim3 grid, const DevScene &S, const FrameParams &P, hipStream_t st)
{
  static_assert(STATS == !(CFG & kCfgCull), "the stats build never culls, every other launch does");
  hipLaunchKernelGGL((trace_rays_kernel<STATS, CFG>), grid, dim3(kWgThreads), 0, st, S, P);
}

// launch_cfg's table (rfx_trace.h) without a mode: the one-light and triangle-BVH instantiations exist for the culling
// configurations that launch_trace_rays' rule can produce, every other cfg drops the bit
template <bool STATS>
inline void launch_rays_cfg(int cfg, dim3 grid, const DevScene &S, const FrameParams &P, hipStream_t st)
{
#if RFX_TRI_BVH
  if (cfg & kCfgTriBvh)
  {
    if constexpr (!STATS)
      switch (cfg & ~kCfgTriBvh)
      {
        case 1: launch_rays_one<STATS, 1 | kCfgTriBvh>(grid, S, P, st); return;
        case 3: launch_rays_one<STATS, 3 | kCfgTriBvh>(grid, S, P, st); return;
        case 9: launch_rays_one<STATS, 9 | kCfgTriBvh>(grid, S, P, st); return;
        case 11: launch_rays_one<STATS, 11 | kCfgTriBvh>(grid, S, P, st); return;
        case 1 | kCfgOneLight: launch_rays_one<STATS, 1 | kCfgOneLight | kCfgTriBvh>(grid, S, P, st); return;
        case 9 | kCfgOneLight: launch_rays_one<STATS, 9 | kCfgOneLight | kCfgTriBvh>(grid, S, P, st); return;
      }
    cfg &= ~kCfgTriBvh;
  }
#endif
  if (cfg & kCfgOneLight)
  {
    if constexpr (!STATS)
      switch (cfg & ~kCfgOneLight)
      {
        case 1: launch_rays_one<STATS, 1 | kCfgOneLight>(grid, S, P, st); return;
        case 5: launch_rays_one<STATS, 5 | kCfgOneLight>(grid, S, P, st); return;
        case 9: launch_rays_one<STATS, 9 | kCfgOneLight>(grid, S, P, st); return;
        case 13: launch_rays_one<STATS, 13 | kCfgOneLight>(grid, S, P, st); return;
      }
    cfg &= ~kCfgOneLight;
  }
  // a culling launch is never a stats one, and the reverse (launch_trace_rays): the odd cfgs are the render kernels,
  // the even ones the counting kernels
  if constexpr (STATS)
    switch (cfg)
    {
      case 0: launch_rays_one<STATS, 0>(grid, S, P, st); break;
      case 2: launch_rays_one<STATS, 2>(grid, S, P, st); break;
      case 4: launch_rays_one<STATS, 4>(grid, S, P, st); break;
      case 6: launch_rays_one<STATS, 6>(grid, S, P, st); break;
      case 8: launch_rays_one<STATS, 8>(grid, S, P, st); break;
      case 10: launch_rays_one<STATS, 10>(grid, S, P, st); break;
      case 12: launch_rays_one<STATS, 12>(grid, S, P, st); break;
      case 14: launch_rays_one<STATS, 14>(grid, S, P, st); break;
    }
  else
    switch (cfg)
    {
      case 1: launch_rays_one<STATS, 1>(grid, S, P, st); break;
      case 3: launch_rays_one<STATS, 3>(grid, S, P, st); break;
      case 5: launch_rays_one<STATS, 5>(grid, S, P, st); break;
      case 7: launch_rays_one<STATS, 7>(grid, S, P, st); break;
      case 9: launch_rays_one<STATS, 9>(grid, S, P, st); break;
      case 11: launch_rays_one<STATS, 11>(grid, S, P, st); break;
      case 13: launch_rays_one<STATS, 13>(grid, S, P, st); break;
      case 15: launch_rays_one<STATS, 15>(grid, S, P, st); break;
    }
}

}  // namespace rfx
