// The coherent order's sort (include/rfx.h rfx_rays_order): the ray keys and a stable LSD radix sort of (key, index)
// pairs -- its own TU (reflaxman_amd/_build.py).
//
//   order_keys_kernel    : a lane per ray, the 24-B record read non-temporally (rfx_ray_slot.h load_ray's read), the
//                          key of rfx.h "Coherent order" written in ray order.
//   paths_order_keys_kernel : the same key gathered through an index array (rfx.h rfx_paths_order): a lane per slot.
//   order_hist_kernel    : a digit pass's per-workgroup histograms, table[digit][workgroup].
//   order_scan_kernel    : workgroup d scans row d of the table in place (exclusive) and leaves the row's total.
//   order_scatter_kernel : the stable scatter.  A pair's place is (the digits below its own, from the scanned totals) +
//                          (its digit in the workgroups before, from the table) + (in the waves before, LDS prefix sums
//                          of the waves' counts) + (in the wave's earlier rounds, a running LDS offset) + (in the lanes
//                          below, a ballot per digit bit).
// Three launches a pass and nothing waits on another workgroup: no look-back, no tickets.
#include <hip/hip_runtime.h>

#include "../../include/rfx.h"
#include "rfx_launch.h"
#include "rfx_paths.h"

#pragma clang fp contract(off)

namespace rfx {

constexpr uint32_t kCB = RFX_ORDER_CELL_BITS, kDB = RFX_ORDER_DIR_BITS;
static_assert(kCB >= 1 && kDB >= 1 && 3 * kCB + 2 * kDB <= 32, "the key is 32 bits");
static_assert(kOrderTile == RFX_ORDER_TILE, "rfx.h names the sort's tile");
static_assert(kOrderThreads == kOrderDigits, "one thread per digit in the scans");

// ------------------------------------------------------------- the key (rfx.h "Coherent order")
__device__ __forceinline__ uint32_t order_cell(float v, float lo, float s)
{
  return (uint32_t)fminf(fmaxf((v - lo) * s, 0.0f), (float)((1u << kCB) - 1u));  // NaN: fmaxf takes the 0
}
__device__ __forceinline__ uint32_t order_dir(float q)
{
  return (uint32_t)fminf(fmaxf((q + 1.0f) * (float)(1u << (kDB - 1)), 0.0f), (float)((1u << kDB) - 1u));
}
__device__ __forceinline__ uint32_t order_key(const OrderBox &B, float ox, float oy, float oz, float dx, float dy, float dz)
{
  const uint32_t cx = order_cell(ox, B.lo[0], B.scale[0]), cy = order_cell(oy, B.lo[1], B.scale[1]),
                 cz = order_cell(oz, B.lo[2], B.scale[2]);
  uint32_t cm = 0;
#pragma unroll
  for (uint32_t b = 0; b < kCB; ++b)
    cm |= (((cx >> b) & 1u) << (3 * b)) | (((cy >> b) & 1u) << (3 * b + 1)) | (((cz >> b) & 1u) << (3 * b + 2));
  const float a = (fabsf(dx) + fabsf(dy)) + fabsf(dz);
  const float px = dx / a, py = dy / a;
  float qx = px, qy = py;
  if (dz < 0.0f)
  {
    qx = (1.0f - fabsf(py)) * (px < 0.0f ? -1.0f : 1.0f);
    qy = (1.0f - fabsf(px)) * (py < 0.0f ? -1.0f : 1.0f);
  }
  const uint32_t u = order_dir(qx), v = order_dir(qy);
  uint32_t dm = 0;
#pragma unroll
  for (uint32_t b = 0; b < kDB; ++b) dm |= (((u >> b) & 1u) << (2 * b)) | (((v >> b) & 1u) << (2 * b + 1));
  return cm << (2 * kDB) | dm;
}

__global__ __launch_bounds__(kOrderThreads) void order_keys_kernel(OrderBox B, const float *rays, uint32_t n,
                                                                   uint32_t *keys, uint32_t *keys2)
{
  const uint32_t i = blockIdx.x * kOrderThreads + threadIdx.x;
  if (i >= n) return;
  const float *f = rays + 6ull * i;
  const float ox = __builtin_nontemporal_load(f), oy = __builtin_nontemporal_load(f + 1),
              oz = __builtin_nontemporal_load(f + 2), dx = __builtin_nontemporal_load(f + 3),
              dy = __builtin_nontemporal_load(f + 4), dz = __builtin_nontemporal_load(f + 5);
  const uint32_t k = order_key(B, ox, oy, oz, dx, dy, dz);
  keys[i] = k;
  if (keys2) keys2[i] = k;
}

// The paths' form (rfx.h rfx_paths_order): slot s keys the record of path index[s] (null: s); an entry that is no path
// of the n reads nothing and takes the last key, so the sort keeps it behind every path
__global__ __launch_bounds__(kOrderThreads) void paths_order_keys_kernel(OrderBox B, const float *rays, uint32_t n,
                                                                         const uint32_t *index, uint32_t slots,
                                                                         uint32_t *keys)
{
  const uint32_t s = blockIdx.x * kOrderThreads + threadIdx.x;
  if (s >= slots) return;
  const uint32_t i = index ? index[s] : s;
  uint32_t k = 0xFFFFFFFFu;
  if (i < n)
  {
    const float *f = rays + 6ull * i;
    const float ox = __builtin_nontemporal_load(f), oy = __builtin_nontemporal_load(f + 1),
                oz = __builtin_nontemporal_load(f + 2), dx = __builtin_nontemporal_load(f + 3),
                dy = __builtin_nontemporal_load(f + 4), dz = __builtin_nontemporal_load(f + 5);
    k = order_key(B, ox, oy, oz, dx, dy, dz);
  }
  keys[s] = k;
}

// ------------------------------------------------------------- the digit pass
__device__ __forceinline__ uint32_t order_digit(uint32_t key, uint32_t shift) { return (key >> shift) & (kOrderDigits - 1u); }

// Exclusive prefix of v over the workgroup's threads and the sum of all (every thread calls; s_w: kOrderWaves words)
__device__ __forceinline__ uint32_t order_block_scan(uint32_t v, uint32_t *s_w, uint32_t &total)
{
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1)
  {
    const uint32_t t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  uint32_t before = 0;
  total = 0;
#pragma unroll
  for (uint32_t w = 0; w < kOrderWaves; ++w)
  {
    const uint32_t c = s_w[w];
    if (w < wave) before += c;
    total += c;
  }
  __syncthreads();  // s_w may be written again
  return before + inc - v;
}

__global__ __launch_bounds__(kOrderThreads) void order_hist_kernel(const uint32_t *keys, uint32_t n, uint32_t shift,
                                                                   uint32_t *table)
{
  __shared__ uint32_t s_h[kOrderDigits];
  s_h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * kOrderTile + threadIdx.x;
#pragma unroll 4
  for (uint32_t j = 0; j < kOrderItems; ++j)
  {
    const uint32_t i = base + j * kOrderThreads;
    if (i < n) atomicAdd(&s_h[order_digit(keys[i], shift)], 1u);
  }
  __syncthreads();
  table[threadIdx.x * gridDim.x + blockIdx.x] = s_h[threadIdx.x];
}

__global__ __launch_bounds__(kOrderThreads) void order_scan_kernel(uint32_t *table, uint32_t groups, uint32_t *totals)
{
  __shared__ uint32_t s_w[kOrderWaves];
  uint32_t *row = table + (size_t)blockIdx.x * groups;
  uint32_t carry = 0;
  for (uint32_t g0 = 0; g0 < groups; g0 += kOrderThreads)
  {
    const uint32_t g = g0 + threadIdx.x;
    const uint32_t v = g < groups ? row[g] : 0u;
    uint32_t total;
    const uint32_t ex = order_block_scan(v, s_w, total);
    if (g < groups) row[g] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

__global__ __launch_bounds__(kOrderThreads) void order_scatter_kernel(const uint32_t *kin, const uint32_t *iin,
                                                                      uint32_t *kout, uint32_t *iout, uint32_t n,
                                                                      uint32_t shift, const uint32_t *table,
                                                                      const uint32_t *totals)
{
  // per wave and digit: the wave's count, then (after the prefix sums) the place of the wave's next pair of that digit
  __shared__ uint32_t s_cnt[kOrderWaves][kOrderDigits];
  __shared__ uint32_t s_w[kOrderWaves];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t w = 0; w < kOrderWaves; ++w) s_cnt[w][threadIdx.x] = 0;
  // digit threadIdx.x starts after every lower digit of the whole array, and after its own in the workgroups before
  uint32_t all;
  uint32_t place = order_block_scan(totals[threadIdx.x], s_w, all) + table[threadIdx.x * gridDim.x + blockIdx.x];
  // (order_block_scan's barriers stand between the zeroing above and the counting below)
  const uint32_t base = blockIdx.x * kOrderTile + wave * (64u * kOrderItems) + lane;
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t key[kOrderItems], pk[kOrderItems];  // pk: the pair's rank among its digit's lanes, that digit's lanes << 8
#pragma unroll
  for (uint32_t j = 0; j < kOrderItems; ++j)
  {
    const uint32_t i = base + 64u * j;
    const bool live = i < n;
    key[j] = live ? kin[i] : 0u;
    const uint32_t d = order_digit(key[j], shift);
    uint64_t m = __builtin_amdgcn_ballot_w64(live);
#pragma unroll
    for (uint32_t b = 0; b < kOrderDigitBits; ++b)
    {
      const bool bit = (d >> b) & 1u;
      const uint64_t bb = __builtin_amdgcn_ballot_w64(bit);
      m &= bit ? bb : ~bb;
    }
    const uint32_t rank = __popcll(m & below), cnt = __popcll(m);
    pk[j] = rank | cnt << 8;
    // one lane per digit present adds the digit's lanes; the wave's rounds follow one another in program order
    if (live && rank == 0) s_cnt[wave][d] += cnt;
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
#pragma unroll
  for (uint32_t w = 0; w < kOrderWaves; ++w)
  {
    const uint32_t c = s_cnt[w][threadIdx.x];
    s_cnt[w][threadIdx.x] = place;
    place += c;
  }
  __syncthreads();
#pragma unroll
  for (uint32_t j = 0; j < kOrderItems; ++j)
  {
    const uint32_t i = base + 64u * j;
    const bool live = i < n;
    const uint32_t d = order_digit(key[j], shift), rank = pk[j] & 255u, cnt = pk[j] >> 8;
    uint32_t at = 0;
    if (live) at = s_cnt[wave][d];
    __builtin_amdgcn_wave_barrier();  // every lane has read the offset before the digit's first lane moves it on
    if (live && rank == 0) s_cnt[wave][d] = at + cnt;
    __builtin_amdgcn_wave_barrier();
    if (live)
    {
      const uint32_t pos = at + rank;  // < n: the counts of all digits, workgroups, waves and rounds sum to n
      if (kout) kout[pos] = key[j];
      iout[pos] = iin ? iin[i] : i;
    }
  }
}

// ------------------------------------------------------------- launches
uint32_t order_groups(uint32_t n) { return (n + kOrderTile - 1) / kOrderTile; }

hipError_t launch_order_keys(const OrderBox &B, const float *d_rays, uint32_t n, uint32_t *keys, uint32_t *keys2,
                             hipStream_t st)
{
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(order_keys_kernel, dim3((n + kOrderThreads - 1) / kOrderThreads), dim3(kOrderThreads), 0, st, B,
                     d_rays, n, keys, keys2);
  return hipGetLastError();
}

hipError_t launch_paths_order_keys(const OrderBox &B, const float *d_rays, uint32_t n, const uint32_t *d_index,
                                   uint32_t slots, uint32_t *keys, hipStream_t st)
{
  if (!slots) return hipSuccess;
  hipLaunchKernelGGL(paths_order_keys_kernel, dim3((slots + kOrderThreads - 1) / kOrderThreads), dim3(kOrderThreads), 0,
                     st, B, d_rays, n, d_index, slots, keys);
  return hipGetLastError();
}

hipError_t launch_order_pass(const uint32_t *kin, const uint32_t *iin, uint32_t *kout, uint32_t *iout, uint32_t n,
                             uint32_t shift, uint32_t *table, uint32_t *totals, hipStream_t st)
{
  if (!n) return hipSuccess;
  const uint32_t groups = order_groups(n);
  hipLaunchKernelGGL(order_hist_kernel, dim3(groups), dim3(kOrderThreads), 0, st, kin, n, shift, table);
  hipLaunchKernelGGL(order_scan_kernel, dim3(kOrderDigits), dim3(kOrderThreads), 0, st, table, groups, totals);
  hipLaunchKernelGGL(order_scatter_kernel, dim3(groups), dim3(kOrderThreads), 0, st, kin, iin, kout, iout, n, shift,
                     (const uint32_t *)table, (const uint32_t *)totals);
  return hipGetLastError();
}

}  // namespace rfx
