// rfx_trace.h -- the trace kernel of ReflaxMan's renderer for gfx950 and the launch of its instantiations.
//
//   trace_kernel<STATS, MODE, CFG> : Render::renderNext (Render.cpp:136-215), one lane per trace, a wave per 8x8-pixel
//       tile: the five pixel-loop variants (TraceMode) around the bounce loop, with the park ids of a plain-pixel lane
//       (ParkTile), each trace's randDir (load_rd), the wave's one-store epilogue (store_wave_tile), the STATS counters'
//       flush and, in an RFX_DEBUG_WAVES build, the wave timeline.
//   launch_one / launch_cfg : a run-time cfg to its instantiation, one family (STATS, MODE) per rfx_trace_*.hip unit.
//
// The rest of the device code, each header including those before it that it uses:
//   rfx_diag.h          event counters, the RFX_DEBUG_PROF region clocks and cull statistics
//   rfx_shade_inputs.h  per-workgroup LDS tables (powf, small-scene records), the workgroup shape, texel lookups
//   rfx_intersect.h     sphere pair, triangle and plane tests; Hit and the closest-hit rule
//   rfx_bundle.h        wave ray bundles and the exact culls against them
//   rfx_bvh.h           the BVH walkers of the non-small scenes
//   rfx_queries.h       closest hit and shadow any-hit over a whole scene
//   rfx_bounce.h        Scene::trace: trace_from, parking, the laundered kernel arguments
// and after this one, for the single unit that launches them:
//   rfx_prim_cull.h     prim_cull_kernel, the per-view masks (rfx_kernels.hip)
//   rfx_parked.h        bounce_kernel, bounce_kernel_lds: the parked traces resumed (rfx_trace_plain_park.hip)
//
// Numerics: compiled with -ffp-contract=off, IEEE div/sqrt, f32 denormals on,
// so every operation rounds exactly as the reference's x86-64 build does.
// Work the reference does but whose result cannot matter is skipped only
// where the skip is provably exact (each site says why).
#pragma once
#include <hip/hip_runtime.h>

#include "rfx_math.h"
#include "rfx_launch.h"
#include "rfx_types.h"
#include "rfx_shade_inputs.h"
#include "rfx_bounce.h"

#pragma clang fp contract(off)

namespace rfx {

template <bool STATS>
__device__ __forceinline__ void flush_counters(const FrameParams &P, Cnt &cnt)
{
  if constexpr (STATS)
  {
#pragma unroll
    for (int k = 0; k < C_COUNT; ++k)
    {
      unsigned long long v = cnt.c[k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      if ((threadIdx.x & 63) == 0 && v) atomicAdd(&P.counters[k], v);
    }
  }
}

__device__ __forceinline__ uint32_t strip_row_to_y(uint32_t r, const FrameParams &P)
{
  if (P.nranks <= 1) return r;
  const uint32_t blk = r / P.row_block, w = r % P.row_block;
  return (blk * P.nranks + P.rank) * P.row_block + w;
}

// the wave's schedule tile (index into the wave-tile grid), kept in LDS across the bounce loop
__shared__ uint32_t s_tile8[kWgWaves];

// Park info of a plain-pixel trace-kernel lane: its randDir trace index and output pixel are re-derived from the
// wave's tile index in LDS when the trace parks (a fresh lane id through an empty asm), instead of being kept
// live across the bounce loop (C3 park instantiation: 13 -> 2 VGPR spills)
struct ParkTile {
  int after;
  QRay *queue;
  uint32_t *count;
  const FrameParams &P;
  uint32_t wv, w8;
  __device__ __forceinline__ void ids(uint32_t &t, uint32_t &o) const
  {
    const uint32_t t8 = ((volatile uint32_t *)s_tile8)[wv];
    uint32_t le = __lane_id();
    asm volatile("" : "+v"(le));
#ifdef RFX_LAUNDER_PARAMS
    const FrameParams &P = kernarg_params();
#endif
    const uint32_t gx = (t8 % w8) * 8u + (le & 7u), gy = (t8 / w8) * 8u + (le >> 3);
    const uint32_t y = P.nranks > 1 ? strip_row_to_y(gy, P) : gy + P.row0;
    const uint32_t orow = P.nranks > 1 ? gy : y;
    t = (uint32_t)((uint64_t)y * P.W + gx - P.p_begin);
    o = (uint32_t)((size_t)orow * P.W + gx);
  }
  static constexpr bool kRefill = false;
  __device__ __forceinline__ uint32_t *keys() const { return P.queue_key; }
  __device__ __forceinline__ BvhGlobal bvh() const { return BvhGlobal{}; }
};

// trace i's randomInsideSphere draw (Vector3.cpp:176-188) from the LCG state before its accepted triple
__device__ __forceinline__ v3 rd_from_state(uint32_t s)
{
  const uint32_t s1 = lcg_step(s), s2 = lcg_step(s1), s3 = lcg_step(s2);
  return mk(rand_component_dev(lcg_out(s1)), rand_component_dev(lcg_out(s2)), rand_component_dev(lcg_out(s3)));
}

__device__ __forceinline__ v3 load_rd(const FrameParams &P, uint64_t i) { return rd_from_state(P.rd_state[i]); }

// Diagnostic build only (RFX_DEBUG_WAVES, tools/wave_timeline.py): each plain-mode wave's start and end on the
// chip's constant 100 MHz clock (s_memrealtime), by wave tile, for the last launch -- the shape of a launch's
// critical path (dispatch ramp, tile durations, tail).
#ifdef RFX_DEBUG_WAVES
constexpr uint32_t kWaveTimeMax = 1u << 18;
constexpr uint32_t kBounceTimeBase = 1u << 17;  // the bounce kernel's 64-trace batches, after the trace kernel's tiles
static __device__ unsigned long long g_wave_time[2 * kWaveTimeMax];
__device__ __forceinline__ uint64_t realtime64()
{
  uint64_t c;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(c));
  return c;
}
#define RFX_WAVE_T0() const uint64_t wave_t0_ = realtime64()
#define RFX_WAVE_T1(tile)                                                                  \
  do {                                                                                      \
    const uint64_t t1_ = realtime64();                                                     \
    if (__lane_id() == 0 && (tile) < kWaveTimeMax)                                         \
    {                                                                                       \
      g_wave_time[2 * (tile)] = wave_t0_;                                                   \
      g_wave_time[2 * (tile) + 1] = t1_;                                                    \
    }                                                                                       \
  } while (0)
#else
constexpr uint32_t kBounceTimeBase = 0;
#define RFX_WAVE_T0() \
  do {                \
  } while (0)
#define RFX_WAVE_T1(tile) \
  do {                    \
  } while (0)
#endif

// Shader clock, low 32 bits.  A plain asm statement (no side effects declared, so the compiler may still
// serve the scene loads that follow through the scalar cache -- __builtin_readcyclecounter would count as a
// memory clobber for them); it waits for its own result.
__device__ __forceinline__ uint32_t clock32()
{
  uint64_t c;
  asm("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(c));
  return (uint32_t)c;
}


// A wave's 8x8 pixels (lane = 8 row + column) at output row `row0`, column `x0`: the colours go through the
// wave's LDS slot and leave as ONE 16-B-per-lane store -- lanes 0-47 write the 8 rows of 8 RGB floats
// (96 B = 6 x 16 B per row, Render.cpp:185's interleaved Color layout), lanes 48-63 the 8 rows of 8 ARGB words
// (32 B = 2 x 16 B per row).  Call with every lane valid; needs W % 4 == 0 and 16-B-aligned images.
__device__ __forceinline__ void store_wave_tile(const FrameParams &P, uint32_t x0, uint32_t row0, col out,
                                                uint32_t lane, uint32_t wave)
{
  uint32_t *s = s_out[wave];
  s[3 * lane] = __float_as_uint(out.r);
  s[3 * lane + 1] = __float_as_uint(out.g);
  s[3 * lane + 2] = __float_as_uint(out.b);
  s[192 + lane] = argb(out);
  __builtin_amdgcn_wave_barrier();
  const bool rgb = lane < 48;
  const uint32_t k = rgb ? lane : lane - 48;
  const uint32_t r = rgb ? k / 6u : k >> 1, c = rgb ? k % 6u : k & 1u;
  const uint4 v = *reinterpret_cast<const uint4 *>(s + (rgb ? r * 24u + 4u * c : 192u + r * 8u + 4u * c));
  const size_t pix = (size_t)(row0 + r) * P.W + x0;
  uint32_t *dst = rgb ? reinterpret_cast<uint32_t *>(P.img) + pix * 3 + 4u * c : P.argb + pix + 4u * c;
  if (rgb || P.argb) *reinterpret_cast<uint4 *>(dst) = v;
}

// Pixel loop variants of Render::renderNext: block preview (sampleNum < 0), one plain trace per pixel
// (sampleNum == 1, no jitter, no accumulation -- the benchmark frame), and the general SSAA / additive
// loop.  The plain variant drops the sample loops and their live state (no spills before the bounce loop).
enum TraceMode { kModeSsaa = 0, kModeBlock = 1, kModePlain = 2, kModeSsaaLanes = 3, kModeSsaaChunks = 4 };
// kModeSsaaLanes (sampleNum 1 with jitter or accumulation, 2, 4, 8): one lane per sample -- a wave is a bw x bw block of
// pixels (ss_lane_block), each pixel's ss x ss samples in consecutive lanes, and the wave sums each pixel's samples in the
// reference's order afterwards; kModeSsaaChunks (sampleNum > 8): the same with the wave on one pixel, its samples 64 at
// a time (a separate mode: the chunk loop around the bounce loop costs registers); sampleNum 3, 5, 6, 7 run kModeSsaa
// (one lane per pixel, its samples in turn)
__host__ __device__ constexpr uint32_t ss_lane_block(int ss)
{
  return ss == 1 ? 8u : ss == 2 ? 4u : ss == 4 ? 2u : ss >= 8 ? 1u : 0u;
}
// CFG bits: kCfgCull -- wave-bundle culling (every non-stats launch); kCfgManyLights -- more than 32 lights;
// kCfgSmall -- at most 32 spheres and 32 triangles (one lane-layout cull mask for the whole scene)
// kCfgPlanes -- the scene holds planes (Scene::addPlane extension); kCfgPark -- plain pixels park their traces
// for the bounce kernel (ray regrouping; rfx_trace_plain_park.hip).  The values: rfx_types.h.
// kCfgTriBvh -- a non-small scene with a triangle BVH (rfx_types.h RFX_TRI_BVH): its culling configurations carry the
// triangle walkers; every other scene runs kernels without them (with them C5 traced 3.0% slower)
// kCfgFarLight -- a small scene whose one light is far (rfx_scene.cpp far_light_terms, rfx_bounce.h FARL): plain,
// lanes and chunks frames of the culling configurations 5 and 13 with kCfgOneLight, and the parking form of the first

// one workgroup = kTileW x kTileH output pixels (block mode: block corners), one wave = an 8x8 tile (ray coherence).
// Every lane of a wave reaches trace() -- lanes outside the frame or the cursor span as invalid -- so the
// bounce loop can use wave-wide bundles.
#ifndef RFX_WAVES_PER_EU_LARGE
#define RFX_WAVES_PER_EU_LARGE RFX_WAVES_PER_EU  // large-scene (BVH) trace kernels' occupancy target (experiment)
#endif
template <bool STATS, int MODE, int CFG>
__global__ __launch_bounds__(kWgThreads) __attribute__((amdgpu_waves_per_eu(
    (CFG & kCfgSmall) ? RFX_WAVES_PER_EU : RFX_WAVES_PER_EU_LARGE))) void trace_kernel(DevScene S, FrameParams P)
{
  static_assert(kKernargSig<decltype(&trace_kernel<STATS, MODE, CFG>)>, "launder_scene / kernarg_params layout");
  constexpr bool CULL = (CFG & kCfgCull) != 0, MANYL = (CFG & kCfgManyLights) != 0, SMALL = (CFG & kCfgSmall) != 0;
  constexpr bool PLANES = (CFG & kCfgPlanes) != 0, PARK = MODE == kModePlain && !STATS && (CFG & kCfgPark) != 0;
  constexpr bool ONEL = (CFG & kCfgOneLight) != 0;  // exactly one light: the light loops unrolled
  constexpr bool TBVH = (CFG & kCfgTriBvh) != 0;    // the scene has a triangle BVH
  constexpr bool FARL = (CFG & kCfgFarLight) != 0;  // the one light is far: its constant terms come from its record
  static_assert(!FARL || (MODE == kModePlain || MODE == kModeSsaaLanes || MODE == kModeSsaaChunks), "far-light modes");
  RFX_WAVE_T0();
  __shared__ float lut[256];
  for (uint32_t i = threadIdx.x; i < 256; i += kWgThreads) lut[i] = (float)i / 255.0f;  // Color.cpp:11-13
  stage_powf_tables();
  if constexpr (SMALL) stage_small_scene(S);
  RFX_PROF_INIT();
  // tile cost: the workgroup's start clock (low 32 bits) waits in LDS, so the bounce loop keeps no register for it
  __shared__ uint32_t s_clk0;
  if (P.tile_cost && threadIdx.x == 0) s_clk0 = clock32();
  __syncthreads();
  Cnt cnt;
  if constexpr (STATS)
  {
#pragma unroll
    for (int k = 0; k < C_COUNT; ++k) cnt.c[k] = 0;
  }
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  // the schedule's unit is the wave's 8x8 tile (round 2: -2.7% trace against the workgroup's 16x8): wave v of
  // workgroup w renders tile tile_order[kWgWaves w + v] of the (kTileWavesX gridDim.x) x (kTileWavesY gridDim.y)
  // tile grid -- with a tile order (longest-processing-time first, from an earlier launch's measured tile costs)
  // the most expensive tiles start first and the cheap ones fill the tail; without, the workgroup's own tiles
  const uint32_t wv = __builtin_amdgcn_readfirstlane(wave), wid = blockIdx.y * gridDim.x + blockIdx.x;
  const uint32_t w8 = kTileWavesX * gridDim.x;
  const uint32_t t8 = P.tile_order ? P.tile_order[kWgWaves * wid + wv]
                                   : (blockIdx.y * kTileWavesY + wv / kTileWavesX) * w8 + blockIdx.x * kTileWavesX + wv % kTileWavesX;
  const uint32_t gx = (t8 % w8) * 8u + (lane & 7u), gy = (t8 / w8) * 8u + (lane >> 3);
  // the tile index waits in LDS across the bounce loop: the epilogue re-derives the output coordinates from it
  // instead of keeping (spilling) them
  if (lane == 0) s_tile8[wv] = t8;
  m33 view;
  view.m11 = P.v11; view.m12 = P.v12; view.m13 = P.v13;
  view.m21 = P.v21; view.m22 = P.v22; view.m23 = P.v23;
  view.m31 = P.v31; view.m32 = P.v32; view.m33 = P.v33;
  const v3 eye = mk(P.eye_x, P.eye_y, P.eye_z);

  if constexpr (MODE == kModeSsaaLanes || MODE == kModeSsaaChunks)
  {
    // Render.cpp:174-194 with the sample loops (181-187) across lanes.  sampleNum 2 / 4: lane = ss^2 q + (ss sx + sy) of
    // pixel q of the wave's bw x bw block; sampleNum >= 8: the wave is one pixel, its ss^2 samples taken 64 at a time
    // (lane = sample - 64 chunk).  Trace index (pixel - p_begin) ss^2 + ss sx + sy, as the reference draws them; the
    // pixel's samples are summed in the reference's order (finColor += trace) through the wave's LDS slot, chunk by
    // chunk onto a running sum kept there (s_out words 192-194).
    constexpr bool CHUNKS = MODE == kModeSsaaChunks;
    const uint32_t ss = (uint32_t)P.ss, ss2 = ss * ss, bw = CHUNKS ? 1u : ss_lane_block(P.ss);
    const uint32_t nchunk = CHUNKS ? (ss2 + 63) / 64 : 1;
    float *sm = reinterpret_cast<float *>(s_out[wv]);
    for (uint32_t chunk = 0; chunk < nchunk; ++chunk)
    {
      // every chunk derives its lanes' state afresh (a laundered lane id and frame parameters), so nothing of it is
      // hoisted out of the chunk loop and held across the bounce loop
      uint32_t lane = threadIdx.x & 63u;
      if constexpr (CHUNKS) asm volatile("" : "+v"(lane));
#ifdef RFX_LAUNDER_PARAMS
      const FrameParams &P = kernarg_params<CHUNKS>();
#endif
      const uint32_t q = bw == 1 ? 0 : lane / ss2, kk = bw == 1 ? 64 * chunk + lane : lane - q * ss2;
      const uint32_t sx = kk / ss, sy = kk - sx * ss;
      const uint32_t lx = (t8 % w8) * bw + q % bw, ly = (t8 / w8) * bw + q / bw;
      const uint32_t x = lx;
      const uint32_t y = P.nranks > 1 ? strip_row_to_y(ly, P) : ly + P.row0;
      const uint64_t p = (uint64_t)y * P.W + x;
      const bool valid = lx < P.W && ly < P.grid_rows && p >= P.p_begin && p < P.p_end && kk < ss2;
      const uint64_t pr = p - P.p_begin;
      float rndx = 0.0f, rndy = 0.0f;
      if (P.additive && valid)                                                     // Render.cpp:177-178
      {
        const uint32_t s1 = lcg_jump(P.jitter_seed, 2 * pr + 1);
        rndx = (float)lcg_out(s1) / (float)0x7FFF;
        rndy = (float)lcg_out(lcg_step(s1)) / (float)0x7FFF;
      }
      const float ssf = (float)(int)ss;
      // float(0) / ss == +0 exactly, so the first sample's offsets need no division
      const float ox = sx ? (float)(int)sx / ssf : 0.0f, oy = sy ? (float)(int)sy / ssf : 0.0f;
      const float rx = (float)x - P.wh, ry = (float)y - P.hh;                     // Render.cpp:152-153
      const v3 ray = mmul(view, mk(rx + ox + rndx, ry + oy + rndy, P.rz));         // Render.cpp:183-184
      v3 rd = mk(0.0f, 0.0f, 0.0f);
      if (valid) rd = load_rd(P, pr * (uint64_t)ss2 + kk);
      // the tile's per-view masks (prim_cull_kernel<., true>; chunks: the pixel's closest-hit mask, every chunk)
      const uint64_t *pm = RFX_PRIM_LANES && SMALL && CULL && !STATS && P.prim_mask
                               ? P.prim_mask + (size_t)kPrimStride * t8 : nullptr;
      // (FARL without the occluder grid: rfx_bounce.h SGRID)
      const col c = trace<STATS, CULL, MANYL, SMALL, PLANES, ONEL, TBVH, FARL, false>(S, eye, ray, P.depth, rd, lut, cnt, valid, pm,
                                                                        P.prim_shadow != 0);
      {
#ifdef RFX_LAUNDER_PARAMS
        const FrameParams &P = kernarg_params();  // shadows the by-value parameter: re-read after the bounce loop
#endif
        // the lane's pixel again, from the tile index in LDS and a fresh lane id (not kept live across the bounce loop)
        const uint32_t t8e = ((volatile uint32_t *)s_tile8)[wv];
        uint32_t le = lane;
        asm volatile("" : "+v"(le));
        const uint32_t ss = (uint32_t)P.ss, ss2 = ss * ss, bw = CHUNKS ? 1u : ss_lane_block(P.ss);
        const uint32_t q = bw == 1 ? 0 : le / ss2, kk = bw == 1 ? 64 * chunk + le : le - q * ss2;
        const uint32_t lx = (t8e % w8) * bw + q % bw, ly = (t8e / w8) * bw + q / bw;
        const uint32_t x = lx;
        const uint32_t y = P.nranks > 1 ? strip_row_to_y(ly, P) : ly + P.row0;
        const uint64_t p = (uint64_t)y * P.W + x;
        const bool pvalid = lx < P.W && ly < P.grid_rows && p >= P.p_begin && p < P.p_end;
        sm[3 * le] = c.r;
        sm[3 * le + 1] = c.g;
        sm[3 * le + 2] = c.b;
        __builtin_amdgcn_wave_barrier();
        const uint32_t first = bw == 1 ? 64 * chunk : 0;  // the pixel's sum starts at its sample 0
#if RFX_SSAA_CHANNEL_SUM
        // Color::operator+= adds the three channels independently (r += c.r, ...), so the pixel's first three lanes
        // each run one channel's chain of adds in the reference's order -- a third of the serial sum one lane ran.
        // The final channels wait in the pixel's first sample's words (only lane ch reads word 3 lead + ch), where the
        // pixel's first lane assembles the ARGB word.
        if (ss2 >= 3)
        {
          const uint32_t lead = bw == 1 ? 0u : le - kk, ch = le - lead;  // kk: the lane's sample in its pixel
          const uint32_t n = min(ss2 - first, bw == 1 ? 64u : ss2);
          const bool last = first + n >= ss2;
          if (pvalid && ch < 3)
          {
            float fc = first ? sm[192 + ch] : 0.0f;
#pragma unroll 8
            for (uint32_t j = 0; j < n; ++j) fc = fc + sm[3 * (lead + j) + ch];
            if (!last)
              sm[192 + ch] = fc;  // more chunks to come: the running sum waits in LDS
            else
            {
              const float sq = (float)(int)ss2;                                    // Render.cpp:189
              if (fabsf(sq) > kVerySmall) fc = fc / sq;
              const size_t o = (size_t)(P.nranks > 1 ? ly : y) * P.W + x;
              float *d = P.img + o * 3;
              if (P.accumulate) fc = d[ch] + fc;                                   // Render.cpp:191-194
              d[ch] = fc;
              sm[3 * lead + ch] = fc;
            }
          }
          __builtin_amdgcn_wave_barrier();
          if (last && pvalid && ch == 0 && P.argb)                                 // Render::copyImage
            P.argb[(size_t)(P.nranks > 1 ? ly : y) * P.W + x] = argb(mkc(sm[3 * lead], sm[3 * lead + 1], sm[3 * lead + 2]));
        }
        else
#endif
        if (pvalid && (bw == 1 ? le == 0 : kk == 0))
        {
          col fin = first ? mkc(sm[192], sm[193], sm[194]) : mkc(0.0f, 0.0f, 0.0f);
          const uint32_t n = min(ss2 - first, bw == 1 ? 64u : ss2);
          for (uint32_t j = 0; j < n; ++j)
            fin = cadd(fin, mkc(sm[3 * (le + j)], sm[3 * (le + j) + 1], sm[3 * (le + j) + 2]));
          if (first + n < ss2)  // more chunks to come: the running sum waits in LDS
          {
            sm[192] = fin.r;
            sm[193] = fin.g;
            sm[194] = fin.b;
          }
          else
          {
            const float sq = (float)(int)ss2;                                      // Render.cpp:189
            if (fabsf(sq) > kVerySmall) fin = mkc(fin.r / sq, fin.g / sq, fin.b / sq);
            const size_t o = (size_t)(P.nranks > 1 ? ly : y) * P.W + x;
            float *d = P.img + o * 3;
            if (P.accumulate) fin = mkc(d[0] + fin.r, d[1] + fin.g, d[2] + fin.b);  // Render.cpp:191-194
            d[0] = fin.r; d[1] = fin.g; d[2] = fin.b;
            if (P.argb) P.argb[o] = argb(fin);                                       // Render::copyImage
          }
        }
        __builtin_amdgcn_wave_barrier();
        if (chunk + 1 == nchunk)
        {
          if (P.tile_cost && __lane_id() == 0) P.tile_cost[t8e] = clock32() - s_clk0;
          RFX_WAVE_T1(t8e);
        }
      }
    }
  }
  else if constexpr (MODE == kModeBlock)
  {
    // block preview (Render.cpp:158-172): only block corners inside the cursor span are traced;
    // trace order = raster order of corners, so corner (cx, cy) is trace cy * bw + cx.
    const uint32_t n = (uint32_t)(-P.ss);
    const uint32_t bw = (P.W + n - 1) / n, bh = (P.H + n - 1) / n;
    const uint32_t cx = gx, cy = gy + P.row0;
    const uint32_t x = cx * n, y = cy * n;
    const uint64_t p = (uint64_t)y * P.W + x;
    const bool valid = gy < P.grid_rows && cx < bw && cy < bh && p >= P.p_begin && p < P.p_end;
    const v3 ray = mmul(view, mk((float)x - P.wh, (float)y - P.hh, P.rz));
    v3 rd = mk(0.0f, 0.0f, 0.0f);
    if (valid) rd = load_rd(P, (uint64_t)cy * bw + cx - P.trace_base);
    const col c = trace<STATS, CULL, MANYL, SMALL, PLANES, ONEL, TBVH>(S, eye, ray, P.depth, rd, lut, cnt, valid);
    if (valid)
    {
      const uint32_t ex = min(P.W, x + n), ey = min(P.H, y + n);
      const uint32_t a = argb(c);
      for (uint32_t qy = y; qy < ey; ++qy)
        for (uint32_t qx = x; qx < ex; ++qx)
        {
          float *d = P.img + ((size_t)qy * P.W + qx) * 3;
          d[0] = c.r; d[1] = c.g; d[2] = c.b;
          if (P.argb) P.argb[(size_t)qy * P.W + qx] = a;
        }
    }
  }
  else
  {
    const uint32_t x = gx;
    const uint32_t y = P.nranks > 1 ? strip_row_to_y(gy, P) : gy + P.row0;
    const uint64_t p = (uint64_t)y * P.W + x;
    const bool valid = gx < P.W && gy < P.grid_rows && p >= P.p_begin && p < P.p_end;
    const uint64_t pr = p - P.p_begin;
    const float rx = (float)x - P.wh, ry = (float)y - P.hh;                       // Render.cpp:152-153
    col out;
    bool parked = false;
    if constexpr (MODE == kModePlain)
    {
      // Render.cpp:183 with ssx = ssy = 0, sampleNum = 1, no jitter: float(0) / 1 == +0, rnd == 0
      const v3 ray = mmul(view, mk(rx + 0.0f + 0.0f, ry + 0.0f + 0.0f, P.rz));
      v3 rd = mk(0.0f, 0.0f, 0.0f);
      if (valid) rd = load_rd(P, pr);
      const ParkTile park{P.park_after, P.queue, P.queue_count, P, wv, w8};
      const uint64_t *pm_tile = SMALL && CULL && !STATS && P.prim_mask ? P.prim_mask + (size_t)kPrimStride * t8 : nullptr;
      // (the parking form without the occluder grid, rfx_bounce.h SGRID: with it the kernel spills one VGPR more)
      const col c = trace_from<STATS, CULL, MANYL, SMALL, PLANES, PARK, ParkTile, ONEL, TBVH, FARL, FARL && !PARK>(
          S, eye, ray, mkc(1.0f, 1.0f, 1.0f), mkc(0.0f, 0.0f, 0.0f), 0, P.depth, rd, lut, cnt, valid, park, parked, pm_tile);
      out = cadd(mkc(0.0f, 0.0f, 0.0f), c);                                      // Render.cpp:185 (/ 1.0f exact)
    }
    else
    {
      // SSAA / additive (Render.cpp:174-194): each lane runs its pixel's ss x ss traces in turn
      float rndx = 0.0f, rndy = 0.0f;
      if (P.additive && valid)                                                     // Render.cpp:177-178
      {
        const uint32_t s1 = lcg_jump(P.jitter_seed, 2 * pr + 1);
        rndx = (float)lcg_out(s1) / (float)0x7FFF;
        rndy = (float)lcg_out(lcg_step(s1)) / (float)0x7FFF;
      }
      const int ss = P.ss;
      const float ssf = (float)ss;
      col fin = mkc(0.0f, 0.0f, 0.0f);
      for (int sx = 0; sx < ss; ++sx)                                              // Render.cpp:181-187
        for (int sy = 0; sy < ss; ++sy)
        {
          // float(0) / ss == +0 exactly, so the first sample's offsets need no division
          const float ox = sx ? (float)sx / ssf : 0.0f, oy = sy ? (float)sy / ssf : 0.0f;
          v3 ray = mk(rx + ox + rndx, ry + oy + rndy, P.rz);
          ray = mmul(view, ray);
          v3 rd = mk(0.0f, 0.0f, 0.0f);
          if (valid) rd = load_rd(P, pr * (uint64_t)(ss * ss) + (uint64_t)(sx * ss + sy));
          const uint64_t *pm = RFX_PRIM_SSAA && SMALL && CULL && !STATS && P.prim_mask
                                   ? P.prim_mask + (size_t)kPrimStride * t8 : nullptr;
          fin = cadd(fin, trace<STATS, CULL, MANYL, SMALL, PLANES, false, TBVH>(S, eye, ray, P.depth, rd, lut, cnt, valid, pm,
                                                                   P.prim_shadow != 0));
        }
      if (ss != 1)                                                                 // Render.cpp:189 (x / 1.0f == x)
      {
        const float sq = (float)(ss * ss);
        if (fabsf(sq) > kVerySmall) fin = mkc(fin.r / sq, fin.g / sq, fin.b / sq);
      }
      out = fin;
    }
    // output coordinates again, from the tile index in LDS (volatile: re-read, not kept live)
#ifdef RFX_LAUNDER_PARAMS
    const FrameParams &P = kernarg_params();  // shadows the by-value parameter: re-read after the bounce loop
#endif
    const uint32_t t8e = ((volatile uint32_t *)s_tile8)[wv];
    uint32_t le = lane;
    asm volatile("" : "+v"(le));  // a fresh lane value: its row/column are recomputed, not kept live
    const uint32_t x0e = (t8e % w8) * 8u, row0e = (t8e / w8) * 8u + (P.nranks > 1 ? 0u : P.row0);
    const uint32_t xe = x0e + (le & 7u), rowe = row0e + (le >> 3), wslot = wv;
    if (MODE == kModeSsaa && P.accumulate && valid)                                  // Render.cpp:191-194
    {
      const float *d = P.img + ((size_t)rowe * P.W + xe) * 3;
      out = mkc(d[0] + out.r, d[1] + out.g, d[2] + out.b);
    }
    const bool staged = (P.W & 3u) == 0 &&
                        ((reinterpret_cast<uintptr_t>(P.img) | reinterpret_cast<uintptr_t>(P.argb)) & 15u) == 0 &&
                        __builtin_amdgcn_ballot_w64(valid && !parked) == ~0ull;
    if (staged)
      store_wave_tile(P, x0e, row0e, out, le, wslot);  // Render::copyImage too
    else if (valid && !parked)
    {
      const size_t o = (size_t)rowe * P.W + xe;
      float *d = P.img + o * 3;
      d[0] = out.r; d[1] = out.g; d[2] = out.b;
      if (P.argb) P.argb[o] = argb(out);                                           // Render::copyImage
    }
    if (P.tile_cost && __lane_id() == 0)  // per wave tile, from its output coordinates
      P.tile_cost[(P.nranks > 1 ? rowe : rowe - P.row0) / 8u * P.tiles_x + xe / 8u] = clock32() - s_clk0;
    RFX_WAVE_T1(t8e);
  }
  flush_counters<STATS>(P, cnt);
  RFX_PROF_FLUSH();

}

// ------------------------------------------------------------- launch of one family (the rfx_trace_*.hip TUs)
template <bool STATS, int MODE, int CFG>
inline void launch_one(dim3 grid, const DevScene &S, const FrameParams &P, hipStream_t st)
{
  if constexpr (!STATS || !(CFG & kCfgCull))  // the stats build never culls
    hipLaunchKernelGGL((trace_kernel<STATS, MODE, CFG>), grid, dim3(kWgThreads), 0, st, S, P);
}

template <bool STATS, int MODE>
inline void launch_cfg(int cfg, dim3 grid, const DevScene &S, const FrameParams &P, hipStream_t st)
{
#if RFX_TRI_BVH
  if (cfg & kCfgTriBvh)  // the non-small culling configurations (rfx_kernels.hip launch_trace sets the bit for no other)
  {
    if constexpr (!STATS)
      switch (cfg & ~kCfgTriBvh)
      {
        case 1: launch_one<STATS, MODE, 1 | kCfgTriBvh>(grid, S, P, st); return;
        case 3: launch_one<STATS, MODE, 3 | kCfgTriBvh>(grid, S, P, st); return;
        case 9: launch_one<STATS, MODE, 9 | kCfgTriBvh>(grid, S, P, st); return;
        case 11: launch_one<STATS, MODE, 11 | kCfgTriBvh>(grid, S, P, st); return;
        case 1 | kCfgOneLight: launch_one<STATS, MODE, 1 | kCfgOneLight | kCfgTriBvh>(grid, S, P, st); return;
        case 9 | kCfgOneLight: launch_one<STATS, MODE, 9 | kCfgOneLight | kCfgTriBvh>(grid, S, P, st); return;
      }
    cfg &= ~kCfgTriBvh;
  }
#endif
  if (cfg & kCfgFarLight)  // a far light (rfx_kernels.hip launch_trace sets the bit for these modes and configurations only)
  {
    if constexpr (!STATS && RFX_FAR_LIGHT && (MODE == kModePlain || MODE == kModeSsaaLanes || MODE == kModeSsaaChunks))
      switch (cfg & ~kCfgFarLight)
      {
        case 5 | kCfgOneLight: launch_one<STATS, MODE, 5 | kCfgOneLight | kCfgFarLight>(grid, S, P, st); return;
        case 13 | kCfgOneLight: launch_one<STATS, MODE, 13 | kCfgOneLight | kCfgFarLight>(grid, S, P, st); return;
      }
    cfg &= ~kCfgFarLight;
  }
  if (cfg & kCfgOneLight)  // scenes with exactly one light: the culling configurations have unrolled light loops
  {
    switch (cfg & ~kCfgOneLight)
    {
      case 1: launch_one<STATS, MODE, 1 | kCfgOneLight>(grid, S, P, st); return;
      case 5: launch_one<STATS, MODE, 5 | kCfgOneLight>(grid, S, P, st); return;
      case 9: launch_one<STATS, MODE, 9 | kCfgOneLight>(grid, S, P, st); return;
      case 13: launch_one<STATS, MODE, 13 | kCfgOneLight>(grid, S, P, st); return;
      default: cfg &= ~kCfgOneLight;
    }
  }
  switch (cfg)
  {
    case 0: launch_one<STATS, MODE, 0>(grid, S, P, st); break;
    case 1: launch_one<STATS, MODE, 1>(grid, S, P, st); break;
    case 2: launch_one<STATS, MODE, 2>(grid, S, P, st); break;
    case 3: launch_one<STATS, MODE, 3>(grid, S, P, st); break;
    case 4: launch_one<STATS, MODE, 4>(grid, S, P, st); break;
    case 5: launch_one<STATS, MODE, 5>(grid, S, P, st); break;
    case 6: launch_one<STATS, MODE, 6>(grid, S, P, st); break;
    case 7: launch_one<STATS, MODE, 7>(grid, S, P, st); break;
    case 8: launch_one<STATS, MODE, 8>(grid, S, P, st); break;
    case 9: launch_one<STATS, MODE, 9>(grid, S, P, st); break;
    case 10: launch_one<STATS, MODE, 10>(grid, S, P, st); break;
    case 11: launch_one<STATS, MODE, 11>(grid, S, P, st); break;
    case 12: launch_one<STATS, MODE, 12>(grid, S, P, st); break;
    case 13: launch_one<STATS, MODE, 13>(grid, S, P, st); break;
    case 14: launch_one<STATS, MODE, 14>(grid, S, P, st); break;
    case 15: launch_one<STATS, MODE, 15>(grid, S, P, st); break;
  }
}

}  // namespace rfx
