// rfx_parked.h -- the kernels that resume parked traces (ray regrouping): Refill, the park policy whose lanes take the
// next queue entry when their trace ends, bounce_kernel and, with the BVH staged in LDS, bounce_kernel_lds.  Launched by
// rfx_trace_plain_park.hip only.
#pragma once
#include <hip/hip_runtime.h>

#include "rfx_trace.h"

#pragma clang fp contract(off)

namespace rfx {

// The parked traces (rfx_types.h QRay) of a plain-pixel launch resumed in packed waves: each wave claims 64
// queue entries at a time (one atomic), runs the rest of their bounce loops and writes their pixels exactly
// as the trace kernel would have (Render.cpp:185 and the ARGB epilogue).  Waves exit once the queue is
// drained; the queue holds traces from all over the frame, so waves no longer idle on lanes whose traces
// ended (the trace kernel's tail of 1-2 live lanes per wave at depth 3+).
// The bounce kernel's lanes (ray regrouping, large scenes) take a new parked trace as soon as theirs ends: at the end of
// every segment a lane whose trace ended writes its pixel (Render.cpp:185), and the wave's idle lanes claim the next
// queue entries with one atomic -- so a wave stays full while its traces end at different segments, until the queue
// is drained.  Each trace resumes from its own parked state, so every float op is the one the trace kernel would have
// run.
__shared__ uint32_t s_refill_out[kWgWaves][64];  // per lane: the output pixel of its trace in flight (~0u: none)

template <class NS = BvhGlobal>
struct Refill {
  const FrameParams &P;
  uint32_t n;             // queue entries
  uint32_t *outs;         // LDS: the output pixel of each lane's trace in flight (~0u: none), 64 per wave
  NS ns;                  // where the BVH walkers find the nodes
  mutable bool drained;   // wave-uniform: every entry has been claimed
  static constexpr bool kRefill = true;
  __device__ __forceinline__ void ids(uint32_t &t, uint32_t &o) const { t = o = 0u; }  // (never parks)
  __device__ __forceinline__ uint32_t *keys() const { return nullptr; }
  __device__ __forceinline__ const NS &bvh() const { return ns; }
  __device__ __forceinline__ void refill(bool &alive, v3 &origin, v3 &ray, col &mulc, col &pix, int &refl, v3 &rd) const
  {
    const uint32_t lane = __lane_id();
    uint32_t out = outs[lane];
    if (!alive && out != ~0u)
    {
      const col o = cadd(mkc(0.0f, 0.0f, 0.0f), pix);                               // Render.cpp:185
      float *d = P.img + (size_t)out * 3;
      d[0] = o.r; d[1] = o.g; d[2] = o.b;
      if (P.argb) P.argb[out] = argb(o);
      out = ~0u;
    }
    const uint64_t idle = __ballot(out == ~0u);
    if (idle && !drained)
    {
      const int first = __ffsll((long long)idle) - 1;
      const uint32_t k = (uint32_t)__popcll(idle);
      uint32_t base = 0;
      if (lane == (uint32_t)first) base = atomicAdd(P.queue_next, k);
      base = __builtin_amdgcn_readlane(base, first);
      if (base + k >= n) drained = true;
      const uint32_t slot = base + (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
      if (out == ~0u && slot < n)
      {
        const QRay q = P.queue[P.queue_order ? P.queue_order[slot] : slot];
        origin = mk(q.ox, q.oy, q.oz);
        ray = mk(q.dx, q.dy, q.dz);
        mulc = mkc(q.mr, q.mg, q.mb);
        pix = mkc(q.pr, q.pg, q.pb);
        refl = (int)q.refl;
        rd = load_rd(P, q.trace);
        out = q.out;
        alive = refl < P.depth;
      }
    }
    outs[lane] = out;
  }
};

template <int CFG>
__global__ RFX_TRACE_BOUNDS void bounce_kernel(DevScene S, FrameParams P)
{
  static_assert(kKernargSig<decltype(&bounce_kernel<CFG>)>, "launder_scene / kernarg_params layout");
  constexpr bool CULL = (CFG & kCfgCull) != 0, MANYL = (CFG & kCfgManyLights) != 0, SMALL = (CFG & kCfgSmall) != 0;
  constexpr bool PLANES = (CFG & kCfgPlanes) != 0;
  __shared__ float lut[256];
  for (uint32_t i = threadIdx.x; i < 256; i += kWgThreads) lut[i] = (float)i / 255.0f;  // Color.cpp:11-13
  stage_powf_tables();
  if constexpr (SMALL) stage_small_scene(S);
  __syncthreads();
  Cnt cnt;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  s_refill_out[wv][__lane_id()] = ~0u;
  const Refill<> rf{P, *P.queue_count, s_refill_out[wv], BvhGlobal{}, false};
  bool alive = false;
  v3 origin = mk(0.0f, 0.0f, 0.0f), ray = origin, rd = origin;
  col mulc = mkc(0.0f, 0.0f, 0.0f), pix = mulc;
  int refl = 0;
  rf.refill(alive, origin, ray, mulc, pix, refl, rd);  // the wave's first 64 traces
  RFX_WAVE_T0();
  bool parked;
  (void)trace_from<false, CULL, MANYL, SMALL, PLANES, false, decltype(rf), (CFG & kCfgOneLight) != 0, (CFG & kCfgTriBvh) != 0>(
      S, origin, ray, mulc, pix, refl, P.depth, rd, lut, cnt, alive, rf, parked);
  RFX_WAVE_T1(kBounceTimeBase + kWgWaves * blockIdx.x + wv);
}

// The bounce kernel with the BVH staged in LDS (RFX_LDS_BVH; large scenes whose nodes fit): one workgroup of
// kLdsBvhThreads threads per CU copies the node boxes (48 B each) and links + margin terms (8 B, DevScene::bvh_aux)
// into its LDS, then its 16 waves take parked traces as bounce_kernel's do -- the walkers' node fetches become LDS
// reads instead of L2 round trips.  Dynamic LDS: lds_bvh_bytes(n_bvh) (rfx_types.h).
template <int CFG>
__global__ __launch_bounds__(kLdsBvhThreads) __attribute__((amdgpu_waves_per_eu(4)))
void bounce_kernel_lds(DevScene S, FrameParams P)
{
  static_assert(kKernargSig<decltype(&bounce_kernel_lds<CFG>)>, "launder_scene / kernarg_params layout");
  constexpr bool CULL = (CFG & kCfgCull) != 0, MANYL = (CFG & kCfgManyLights) != 0, SMALL = (CFG & kCfgSmall) != 0;
  constexpr bool PLANES = (CFG & kCfgPlanes) != 0;
  static_assert(!SMALL, "large scenes only");
  extern __shared__ float4 s_dyn[];
  const int nn = S.n_bvh;
  float4 *box = s_dyn;
  uint2 *aux = reinterpret_cast<uint2 *>(box + 3 * nn);
  BvhSlot *stk = reinterpret_cast<BvhSlot *>(aux + nn);
  uint32_t *outs = reinterpret_cast<uint32_t *>(stk + kBvhStack * kLdsBvhThreads);
  __shared__ float lut[256];
  for (uint32_t i = threadIdx.x; i < 256; i += kLdsBvhThreads) lut[i] = (float)i / 255.0f;  // Color.cpp:11-13
  stage_powf_tables();
  const float4 *gb = reinterpret_cast<const float4 *>(S.bvh);
  const uint2 *ga = reinterpret_cast<const uint2 *>(S.bvh_aux);
  for (int i = (int)threadIdx.x; i < nn; i += kLdsBvhThreads)
  {
    box[3 * i] = gb[4 * i];
    box[3 * i + 1] = gb[4 * i + 1];
    box[3 * i + 2] = gb[4 * i + 2];
    aux[i] = ga[i];
  }
  __syncthreads();
  Cnt cnt;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  outs[64 * wv + __lane_id()] = ~0u;
  const Refill<BvhLds> rf{P, *P.queue_count, outs + 64 * wv, BvhLds{box, aux, stk, S.bvh_mstep}, false};
  bool alive = false;
  v3 origin = mk(0.0f, 0.0f, 0.0f), ray = origin, rd = origin;
  col mulc = mkc(0.0f, 0.0f, 0.0f), pix = mulc;
  int refl = 0;
  rf.refill(alive, origin, ray, mulc, pix, refl, rd);
  bool parked;
  (void)trace_from<false, CULL, MANYL, SMALL, PLANES, false, decltype(rf), (CFG & kCfgOneLight) != 0, (CFG & kCfgTriBvh) != 0>(
      S, origin, ray, mulc, pix, refl, P.depth, rd, lut, cnt, alive, rf, parked);
}

}  // namespace rfx
