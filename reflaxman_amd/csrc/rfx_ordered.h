// rfx_ordered.h -- the ray batch and the hit queries run in an order the caller gives (include/rfx.h
// rfx_trace_rays_ordered, rfx_query_hits_ordered, rfx_query_occluded_ordered).
//
// The kernels are trace_rays_kernel (rfx_rays.h), query_hits_kernel and query_occluded_kernel (rfx_hits.h) with one
// change, and say no more than that change: they take the same text (rfx_rays_body.inc; the queries' body functions)
// with a lane's ray not its slot but order[slot].  Wave w takes the slots 64 w .. 64 w + 63; the record, the randDir
// state, the skip entry and every output are indexed by the ray, so for a permutation every word is the unordered
// call's and only the company a ray keeps in its wave changes.  A slot past the launch's end, or one whose index is
// not a ray of the batch, is a dead lane: it reads and writes nothing, and reaches the wave-wide code as an invalid
// lane does.  Outputs leave per lane (12-B and 4-B stores): a wave's rays are nowhere near each other, so the staged
// 16-B forms of the unordered kernels do not apply.  There is no stats form.  rfx_trace_ordered.hip holds these kernels;
// rfx_span.h includes this for ordered_query_slot alone.
#pragma once
#include <hip/hip_runtime.h>

#include "rfx_rays.h"
#include "rfx_hits.h"
#include "rfx_launch.h"

#pragma clang fp contract(off)

namespace rfx {

// FrameParams as an ordered batch reads it: a linear batch's fields (rfx_rays.h; W = 0, p_end rays and as many slots),
// and the index array in tile_order, the frame kernels' tile schedule, which no code a batch reaches reads.
__host__ __device__ inline const uint32_t *ray_order(const FrameParams &P) { return P.tile_order; }
inline void set_ray_order(FrameParams &P, const uint32_t *d_order) { P.tile_order = d_order; }

// slot `slot` of the `slots` a launch holds: the ray order[slot] of `rays`
__device__ __forceinline__ RaySlot ordered_slot(const uint32_t *order, uint64_t slot, uint64_t slots, uint64_t rays)
{
  RaySlot s;
  s.i = 0;
  s.x0 = s.row0 = 0;
  s.valid = slot < slots;
  if (s.valid)
  {
    s.i = order[slot];
    s.valid = s.i < rays;
  }
  return s;
}

// rfx_rays_body.inc's rule (rfx_rays.h RasterRays) for an ordered batch: outputs always leave per lane
struct OrderedRays {
  static constexpr bool kStaged = false;
  static __device__ __forceinline__ OrderedRays here() { return {}; }
  __device__ __forceinline__ uint32_t unit(const FrameParams &, uint32_t wv) const { return kWgWaves * blockIdx.x + wv; }
  __device__ __forceinline__ RaySlot slot(const FrameParams &P, uint32_t unit, uint32_t lane) const
  {
    return ordered_slot(ray_order(P), 64ull * unit + lane, P.p_end, P.p_end);
  }
};

template <int CFG>
__global__ __launch_bounds__(kWgThreads) __attribute__((amdgpu_waves_per_eu(
    (CFG & kCfgSmall) ? RFX_WAVES_PER_EU : RFX_WAVES_PER_EU_LARGE))) void trace_rays_ordered_kernel(DevScene S, FrameParams P)
{
  static_assert(kKernargSig<decltype(&trace_rays_ordered_kernel<CFG>)>, "launder_scene / kernarg_params layout");
  static_assert((CFG & kCfgCull) != 0, "no stats form: every ordered launch culls");
  constexpr bool STATS = false;
  using Rays = OrderedRays;
  __shared__ float lut[256];
#include "rfx_rays_body.inc"  // the kernel's text, on S, P, STATS, CFG, Rays and lut
}

// A lane's slot of an ordered query, plain or span: wave w of the launch takes the slots slot0 + 64 w .. of
// [slot0, slot1), each naming one of the batch's n rays
__device__ __forceinline__ RaySlot ordered_query_slot(const uint32_t *order, uint64_t slot0, uint64_t slot1, uint64_t n)
{
  const uint32_t lane = threadIdx.x & 63u, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  return ordered_slot(order, slot0 + 64ull * (kWgWaves * blockIdx.x + wv) + lane, slot1, n);
}
__device__ __forceinline__ RaySlot ordered_hit_slot(const HitOrderParams &P)
{
  return ordered_query_slot(P.order, P.slot0, P.slot1, P.H.n);
}

template <int CFG>
__global__ __launch_bounds__(kWgThreads) void query_hits_ordered_kernel(DevScene S, HitOrderParams Q)
{
  __shared__ float lut[256];
  query_hits_body<CFG>(S, Q.H, ordered_hit_slot(Q), lut);
}

template <int CFG>
__global__ __launch_bounds__(kWgThreads) void query_occluded_ordered_kernel(DevScene S, HitOrderParams Q)
{
  query_occluded_body<CFG>(S, Q.H, ordered_hit_slot(Q));
}

}  // namespace rfx
