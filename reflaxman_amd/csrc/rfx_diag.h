// rfx_diag.h -- what the trace device code counts besides rendering.  Cnt / RFX_CNT: the event counters of the STATS
// kernels (indices: rfx_types.h C_*), compiled out of the others.  RFX_DEBUG_PROF build only (tools/regionprof.py,
// tools/build_diag.py): wave clock sums per region of the bounce segment and the bundle cull statistics; in every
// other build the RFX_PROF_* and RFX_CULL_STAT* macros are empty statements.  The RFX_DEBUG_WAVES timeline stands
// with the kernels it times (rfx_trace.h).
#pragma once
#include <hip/hip_runtime.h>

#include "rfx_types.h"

#pragma clang fp contract(off)

namespace rfx {

struct Cnt { uint32_t c[C_COUNT]; };

#define RFX_CNT(k)                   \
  do {                               \
    if constexpr (STATS) cnt.c[k]++; \
  } while (0)

// Diagnostic build only (RFX_DEBUG_PROF, tools/regionprof.py): wave clock cycles spent per region of
// the bounce segment, summed by each region's first active lane into a device-global table.
#ifdef RFX_DEBUG_PROF
enum ProfRegion { P_SPH = 0, P_TRI, P_WIN, P_LIGHT, P_SHADOW, P_MAT, P_SKY, P_SEG, P_COUNT };
static __device__ unsigned long long g_prof[2 * P_COUNT];  // cycles, then wave executions (per TU)
__shared__ unsigned long long s_prof[2 * P_COUNT];  // per workgroup, flushed to g_prof at kernel end
#define RFX_PROF_BEGIN(k) const uint64_t prof_t0_##k = __builtin_amdgcn_s_memtime()
#define RFX_PROF_END(k)                                                                   \
  do {                                                                                    \
    const uint64_t dt_ = __builtin_amdgcn_s_memtime() - prof_t0_##k;                     \
    if ((threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)__ballot(1)) - 1))           \
    {                                                                                     \
      atomicAdd(&s_prof[k], (unsigned long long)dt_);                                     \
      atomicAdd(&s_prof[P_COUNT + k], 1ull);                                              \
    }                                                                                     \
  } while (0)
// cull statistics (diagnostic build): per bundle kind (0 closest hit, 1 shadow): bundles, usable bundles,
// live lanes, kept sphere pairs, kept triangles, valid pairs, valid triangles
static __device__ unsigned long long g_cull[32];
// large scenes (kind 2 closest hit, 3 shadow): bundles, usable bundles, live lanes, kept chunks, kept spheres,
// pair tests run
#define RFX_CULL_STAT_LARGE(kind, ok, live_mask, chunks, spheres, pairs)                            \
  do {                                                                                              \
    if ((threadIdx.x & 63u) == 0u)                                                                  \
    {                                                                                               \
      atomicAdd(&g_cull[8 * (kind) + 0], 1ull);                                                     \
      atomicAdd(&g_cull[8 * (kind) + 1], (ok) ? 1ull : 0ull);                                       \
      atomicAdd(&g_cull[8 * (kind) + 2], (unsigned long long)__popcll(live_mask));                 \
      atomicAdd(&g_cull[8 * (kind) + 3], (unsigned long long)(chunks));                            \
      atomicAdd(&g_cull[8 * (kind) + 4], (unsigned long long)(spheres));                           \
      atomicAdd(&g_cull[8 * (kind) + 5], (unsigned long long)(pairs));                             \
    }                                                                                               \
  } while (0)
#define RFX_CULL_STAT(kind, ok, live_mask, om, valid)                                                 \
  do {                                                                                              \
    if ((threadIdx.x & 63u) == 0u)                                                                  \
    {                                                                                               \
      atomicAdd(&g_cull[8 * (kind) + 0], 1ull);                                                     \
      atomicAdd(&g_cull[8 * (kind) + 1], (ok) ? 1ull : 0ull);                                       \
      atomicAdd(&g_cull[8 * (kind) + 2], (unsigned long long)__popcll(live_mask));                 \
      atomicAdd(&g_cull[8 * (kind) + 3], (unsigned long long)__popc(small_pairs(om)));             \
      atomicAdd(&g_cull[8 * (kind) + 4], (unsigned long long)__popcll(small_tris(om)));            \
      atomicAdd(&g_cull[8 * (kind) + 5], (unsigned long long)__popc(small_pairs(valid)));          \
      atomicAdd(&g_cull[8 * (kind) + 6], (unsigned long long)__popcll(small_tris(valid)));         \
    }                                                                                               \
  } while (0)
#define RFX_PROF_INIT()                                          \
  do {                                                           \
    if (threadIdx.x < 2 * P_COUNT) s_prof[threadIdx.x] = 0ull;   \
  } while (0)
#define RFX_PROF_FLUSH()                                                            \
  do {                                                                              \
    __syncthreads();                                                                \
    if (threadIdx.x < 2 * P_COUNT) atomicAdd(&g_prof[threadIdx.x], s_prof[threadIdx.x]); \
  } while (0)
#else
#define RFX_PROF_INIT() \
  do {                  \
  } while (0)
#define RFX_PROF_FLUSH() \
  do {                   \
  } while (0)
#define RFX_PROF_BEGIN(k) \
  do {                    \
  } while (0)
#define RFX_PROF_END(k) \
  do {                  \
  } while (0)
#define RFX_CULL_STAT(kind, ok, live_mask, om, valid) \
  do {                                                \
  } while (0)
#define RFX_CULL_STAT_LARGE(kind, ok, live_mask, chunks, spheres, pairs) \
  do {                                                                   \
  } while (0)
#endif

}  // namespace rfx
