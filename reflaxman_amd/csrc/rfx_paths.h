// rfx_paths.h -- Scene::trace as resumable per-path states, stepped by segment (include/rfx.h "Paths").
//
//   PathParams      : the launch records of the three calls, and the launches' declarations (host and device units).
//   PathStep        : trace_from's policy (rfx_bounce.h, the Refill hook) that ends a step -- at the end of every
//                     segment a lane whose path left the loop, or has run `upto` segments, stores its end state.
//   paths_step_kernel<CFG> : one lane per slot around trace_from, the batch kernels' workgroup and staging.
//   paths_begin_kernel     : the start state of n paths, randDir from the pre-pass's states where the call draws.
//
// A step is no frame and no batch: it reads no randDir state (the path carries its draw) and writes no image.  Its
// launch reuses FrameParams as it is (the kernels' arguments are (DevScene, FrameParams), kKernargSig); the fields a
// step reads are named below.  The device part compiles in rfx_trace_paths.hip only (RFX_PATHS_DEVICE).
#pragma once
#include <hip/hip_runtime.h>

#include "rfx_types.h"
#include "rfx_order_types.h"

namespace rfx {

// The planes of rfx_paths (include/rfx.h), as the host hands them to a launch
struct PathPlanes {
  float *rays, *mul, *colour, *rand;
  int32_t *state;
  uint32_t *argb;
};

// FrameParams as a step reads it (rfx_paths.cpp fills the record through set_path_step):
//   p_end       n, the paths of the planes;  depth  upto
//   p_begin, trace_base   the slots [p_begin, trace_base) of this launch: wave w of it takes p_begin + 64 w ..
//   tile_order  d_index or null (the ordered batches' field);  img / argb  d_colour / d_argb
//   queue_order d_rays (the batches' field, written here too);  queue  d_mul;  rd_state  d_rand;  queue_key  d_state
//   queue_next  d_live or null;  queue_count  d_live_count or null
// No code a step reaches reads the parking fields as what they are: no kCfgPark instantiation, and PathStep is the
// only policy.
inline void set_path_step(FrameParams &P, const PathPlanes &p, uint64_t n, const uint32_t *d_index, uint64_t slot0,
                          uint64_t slot1, int32_t upto, uint32_t *d_live, uint32_t *d_live_count)
{
  P.p_end = n;
  P.depth = upto;
  P.ss = 1;
  P.nranks = 1;
  P.p_begin = slot0;
  P.trace_base = slot1;
  P.tile_order = d_index;
  P.img = p.colour;
  P.argb = p.argb;
  P.queue_order = reinterpret_cast<const uint32_t *>(p.rays);
  P.queue = reinterpret_cast<QRay *>(p.mul);
  P.rd_state = reinterpret_cast<const uint32_t *>(p.rand);
  P.queue_key = reinterpret_cast<uint32_t *>(p.state);
  P.queue_next = d_live;
  P.queue_count = d_live_count;
}

// ---- rfx_trace_paths.hip: the start state of paths [0, m) of the planes (rd_state: the pre-pass's states of these m
// paths, or null: d_rand stays), and one launch of a step (P: set_path_step's record)
hipError_t launch_paths_begin(const PathPlanes &p, uint64_t m, const uint32_t *rd_state, hipStream_t st);
hipError_t launch_paths_step(const DevScene &S, const FrameParams &P, hipStream_t st);
// ---- rfx_order_sort.hip: the keys of the paths index[s] (null: s), s < slots, from their records in `rays`; an entry
// that is no path of the n takes key 0xFFFFFFFF
hipError_t launch_paths_order_keys(const OrderBox &B, const float *d_rays, uint32_t n, const uint32_t *d_index,
                                   uint32_t slots, uint32_t *keys, hipStream_t st);

}  // namespace rfx

#ifdef RFX_PATHS_DEVICE
#include "rfx_trace.h"
#include "rfx_ordered.h"

#pragma clang fp contract(off)

namespace rfx {

__device__ __forceinline__ float *path_rays(const FrameParams &P) { return reinterpret_cast<float *>(const_cast<uint32_t *>(P.queue_order)); }
__device__ __forceinline__ float *path_mul(const FrameParams &P) { return reinterpret_cast<float *>(P.queue); }
__device__ __forceinline__ const float *path_rand(const FrameParams &P) { return reinterpret_cast<const float *>(P.rd_state); }
__device__ __forceinline__ int32_t *path_state(const FrameParams &P) { return reinterpret_cast<int32_t *>(P.queue_key); }

// the lane's path: slot P.p_begin + s of [.., P.trace_base), through the index array where there is one -- the ordered
// calls' rule (rfx_ordered.h ordered_slot)
__device__ __forceinline__ RaySlot path_slot(const FrameParams &P, uint64_t s)
{
  const uint64_t slot = P.p_begin + s;
  if (P.tile_order) return ordered_slot(P.tile_order, slot, P.trace_base, P.p_end);
  RaySlot r;
  r.x0 = r.row0 = 0;
  r.i = slot;
  r.valid = slot < P.trace_base && slot < P.p_end;
  return r;
}

// The wave's words of s_out (rfx_bounce.h; a step stages no output): [lane] the lane's path while it runs (~0u: none),
// [64 + lane] the state it has after the call (a lane that names no path: -1)
constexpr uint32_t kPathNone = ~0u;

// trace_from's policy of a step.  The loop runs with a depth it never reaches; at the end of every segment the lanes
// whose path has left the loop (sky, the mulColor cut-off: alive is false, refl counts the segments before this one)
// or has run `upto` segments store their end state and stop.  The frame parameters are re-read where they are used
// (kernarg_params), so the planes' pointers are not held across the segments.
struct PathStep {
  uint32_t *slots;  // LDS: this wave's 128 words
  static constexpr bool kRefill = true;  // (never parks: trace_from's PARK is false here, so no ids() or keys())
  __device__ __forceinline__ BvhGlobal bvh() const { return BvhGlobal{}; }
  __device__ __forceinline__ void refill(bool &alive, v3 &origin, v3 &ray, col &mulc, col &pix, int &refl, v3 &) const
  {
    const uint32_t lane = __lane_id();
    const uint32_t i = slots[lane];
    if (i == kPathNone) return;
    const FrameParams &P = kernarg_params();
    const bool stop = alive && refl >= P.depth;
    if (alive && !stop) return;
    float *c = P.img + (size_t)i * 3;
    c[0] = pix.r; c[1] = pix.g; c[2] = pix.b;
    if (P.argb) P.argb[i] = argb(pix);
    int32_t s = ~(refl + 1);
    if (stop)
    {
      float *r = path_rays(P) + (size_t)i * 6, *m = path_mul(P) + (size_t)i * 3;
      r[0] = origin.x; r[1] = origin.y; r[2] = origin.z;                         // Scene.cpp:225-226
      r[3] = ray.x; r[4] = ray.y; r[5] = ray.z;
      m[0] = mulc.r; m[1] = mulc.g; m[2] = mulc.b;
      s = refl;
    }
    path_state(P)[i] = s;
    slots[64 + lane] = (uint32_t)s;
    slots[lane] = kPathNone;
    alive = false;
  }
};

template <int CFG>
__global__ __launch_bounds__(kWgThreads) __attribute__((amdgpu_waves_per_eu(
    (CFG & kCfgSmall) ? RFX_WAVES_PER_EU : RFX_WAVES_PER_EU_LARGE))) void paths_step_kernel(DevScene S, FrameParams P)
{
  static_assert(kKernargSig<decltype(&paths_step_kernel<CFG>)>, "launder_scene / kernarg_params layout");
  static_assert((CFG & kCfgCull) != 0 && !(CFG & (kCfgPark | kCfgFarLight)), "the render cfgs of a batch");
  constexpr bool CULL = true, MANYL = (CFG & kCfgManyLights) != 0, SMALL = (CFG & kCfgSmall) != 0;
  constexpr bool PLANES = (CFG & kCfgPlanes) != 0, ONEL = (CFG & kCfgOneLight) != 0, TBVH = (CFG & kCfgTriBvh) != 0;
  __shared__ float lut[256];
  const uint32_t lane = threadIdx.x & 63u, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t wave = kWgWaves * blockIdx.x + wv;
  const RaySlot sl = path_slot(P, 64ull * wave + lane);
  // The lane's state is read first, non-temporally: it comes from HBM once, and the staging below runs while it is on
  // its way (rfx_rays_body.inc).  A lane that names no path, or a path this step does not run, reads no more than its
  // state word and enters the bounce loop as an invalid lane.
  int32_t st = -1;
  if (sl.valid) st = __builtin_nontemporal_load(path_state(P) + sl.i);
  const bool run = sl.valid && st >= 0 && st < P.depth;
  v3 o = mk(0.0f, 0.0f, 0.0f), d = o, rd = o;
  col mulc = mkc(0.0f, 0.0f, 0.0f), pix = mulc;
  if (run)
  {
    const RayRecord r = load_ray(path_rays(P), sl.i);
    o = r.o;
    d = r.d;
    const float *m = path_mul(P) + sl.i * 3, *c = P.img + sl.i * 3, *q = path_rand(P) + sl.i * 3;
    mulc = mkc(__builtin_nontemporal_load(m), __builtin_nontemporal_load(m + 1), __builtin_nontemporal_load(m + 2));
    pix = mkc(__builtin_nontemporal_load(c), __builtin_nontemporal_load(c + 1), __builtin_nontemporal_load(c + 2));
    rd = mk(__builtin_nontemporal_load(q), __builtin_nontemporal_load(q + 1), __builtin_nontemporal_load(q + 2));
  }
  uint32_t *slots = s_out[wv];
  slots[lane] = run ? (uint32_t)sl.i : kPathNone;
  slots[64 + lane] = (uint32_t)st;
  for (uint32_t i = threadIdx.x; i < 256; i += kWgThreads) lut[i] = (float)i / 255.0f;  // Color.cpp:11-13
  stage_powf_tables();
  if constexpr (SMALL) stage_small_scene(S);
  __syncthreads();
  Cnt cnt;
  const PathStep step{slots};
  bool parked;
  (void)trace_from<false, CULL, MANYL, SMALL, PLANES, false, PathStep, ONEL, TBVH>(S, o, d, mulc, pix, st, INT32_MAX, rd, lut,
                                                                            cnt, run, step, parked);
  {
#ifdef RFX_LAUNDER_PARAMS
    const FrameParams &P = kernarg_params();  // shadows the by-value parameter: re-read after the bounce loop
#endif
    if (!P.queue_count) return;
    // the live list: the wave's named paths that are live after the call, appended with one atomic per wave (the
    // parking code's pattern).  The lane's path is derived again from a fresh lane value, not kept live.
    uint32_t le = lane;
    asm volatile("" : "+v"(le));
    const RaySlot se = path_slot(P, 64ull * wave + le);
    const bool live = se.valid && (int32_t)((volatile uint32_t *)slots)[64 + le] >= 0;
    const uint64_t lm = __ballot(live);
    if (!lm) return;
    const int first = __ffsll((long long)lm) - 1;
    uint32_t base = 0;
    if (le == (uint32_t)first) base = atomicAdd(P.queue_count, (uint32_t)__popcll(lm));
    base = __builtin_amdgcn_readlane(base, first);
    // base + rank < the launches' slots so far: every slot is counted at most once
    if (live && P.queue_next) P.queue_next[base + (uint32_t)__popcll(lm & ((1ull << le) - 1ull))] = (uint32_t)se.i;
  }
}

// mul = 1, colour = 0, state = 0 (Scene.cpp:75-78), argb where given; rd_state: randDir i from the pre-pass's state i
__global__ __launch_bounds__(256) void paths_begin_kernel(PathPlanes p, uint64_t m, const uint32_t *rd_state)
{
  const uint64_t i = 256ull * blockIdx.x + threadIdx.x;
  if (i >= m) return;
  float *mu = p.mul + 3 * i, *c = p.colour + 3 * i;
  mu[0] = mu[1] = mu[2] = 1.0f;
  c[0] = c[1] = c[2] = 0.0f;
  p.state[i] = 0;
  if (p.argb) p.argb[i] = argb(mkc(0.0f, 0.0f, 0.0f));
  if (rd_state)
  {
    const v3 rd = rd_from_state(rd_state[i]);
    float *q = p.rand + 3 * i;
    q[0] = rd.x; q[1] = rd.y; q[2] = rd.z;
  }
}

}  // namespace rfx
#endif  // RFX_PATHS_DEVICE
