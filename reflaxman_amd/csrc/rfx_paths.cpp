// Paths of librfx.so (include/rfx.h "Paths": rfx_paths_begin, rfx_paths_step, rfx_paths_order): Scene::trace
// (Scene.cpp:73-236) as per-ray states in planes the caller holds on the device, stepped by segment.
//
// begin is a ray batch's pre-pass (rfx_rays.cpp) with the draws written out instead of traced with; a step is a launch
// of paths_step_kernel (rfx_paths.h) per slot range and, like a hit query, leaves every stream, mask and timing sum
// alone; the order is rfx_rays_order's sort (rfx_order.cpp) on keys gathered through the index array.
#include "rfx_internal.h"
#include "rfx_paths.h"

using namespace rfx;

static bool planes_ok(const rfx_paths *p)
{
  return p && p->d_rays && p->d_mul && p->d_colour && p->d_rand && p->d_state;
}
static PathPlanes planes_at(const rfx_paths *p, uint64_t a)
{
  return PathPlanes{p->d_rays + 6 * a, p->d_mul + 3 * a, p->d_colour + 3 * a, p->d_rand + 3 * a, p->d_state + a,
                    p->d_argb ? p->d_argb + a : nullptr};
}

extern "C" int rfx_paths_begin(rfx_renderer *r, const rfx_paths *p, uint64_t n, int draw, void *stream)
{
  int rc;
  if ((rc = enter_call(r, planes_ok(p) && n, "paths_begin", "renderer, the five planes and n > 0 required")) != RFX_OK)
    return rc;
  const hipStream_t st = stream_or_own(r, stream);
  const uint64_t per = rays_per_launch(r, 0);
  for (uint64_t a = 0; a < n; a += per)
  {
    const uint64_t m = std::min(per, n - a);
    // path a + i takes the i-th draw of this part, the stream running on from the part before (rfx_trace_rays' split)
    if (draw && (rc = prepass_traces(r, m, st)) != RFX_OK) return rc;
    HIP_CHECK(launch_paths_begin(planes_at(p, a), m, draw ? r->rd.p : nullptr, st));
  }
  return RFX_OK;
}

extern "C" int rfx_paths_step(rfx_renderer *r, const rfx_paths *p, uint64_t n, const uint32_t *d_index, uint64_t slots,
                              int32_t upto, uint32_t *d_live, uint32_t *d_live_count, void *stream)
{
  int rc;
  if ((rc = enter_call(r, planes_ok(p) && slots && n && n < (1ull << 32) && upto >= 1 && upto != INT32_MAX &&
                              (!d_live || d_live_count),
                       "paths_step",
                       "renderer, the five planes, slots > 0, 0 < n < 2^32, 1 <= upto < INT32_MAX and a count with the "
                       "live list required")) != RFX_OK)
    return rc;
  const hipStream_t st = stream_or_own(r, stream);
  if (d_live_count) HIP_CHECK(hipMemsetAsync(d_live_count, 0, sizeof(uint32_t), st));
  const PathPlanes planes = planes_at(p, 0);
  const uint64_t per = rays_per_launch(r, 0);
  for (uint64_t a = 0; a < slots; a += per)
  {
    FrameParams P{};
    set_path_step(P, planes, n, d_index, a, std::min(slots, a + per), upto, d_live, d_live_count);
    HIP_CHECK(launch_paths_step(r->dev, P, st));
  }
  return RFX_OK;
}

extern "C" int rfx_paths_order(rfx_renderer *r, const rfx_paths *p, uint64_t n, const uint32_t *d_index, uint64_t slots,
                               uint32_t *d_order, void *stream)
{
  constexpr uint32_t kKeyBits = 3 * RFX_ORDER_CELL_BITS + 2 * RFX_ORDER_DIR_BITS;
  constexpr uint32_t kPasses = (kKeyBits + kOrderDigitBits - 1) / kOrderDigitBits;
  static_assert(kPasses >= 2, "d_order may be d_index: the pass that reads the one is not the pass that writes the other");
  int rc;
  if ((rc = enter_call(r, p && p->d_rays && d_order && n && n < (1ull << 32) && slots && slots < (1ull << 31),
                       "paths_order", "renderer, paths, order, 0 < n < 2^32 and 0 < slots < 2^31 required")) != RFX_OK)
    return rc;
  const hipStream_t st = stream_or_own(r, stream);
  const uint32_t m = (uint32_t)slots;
  if ((rc = r->order_keys.reserve(2 * (size_t)m)) < 0 || (rc = r->order_idx.reserve(2 * (size_t)m)) < 0 ||
      (rc = r->order_table.reserve((size_t)kOrderDigits * order_groups(m) + kOrderDigits)) < 0)
    return rc;
  uint32_t *const key[2] = {r->order_keys.p, r->order_keys.p + m}, *const idx[2] = {r->order_idx.p, r->order_idx.p + m};
  uint32_t *const table = r->order_table.p, *const totals = table + (size_t)kOrderDigits * order_groups(m);
  HIP_CHECK(launch_paths_order_keys(r->order_box, p->d_rays, (uint32_t)n, d_index, m, key[0], st));
  // rfx_rays_order's passes; the first takes the caller's entries (or the slot itself) as the pairs' indices
  for (uint32_t q = 0; q < kPasses; ++q)
  {
    const uint32_t a = q & 1u, b = a ^ 1u;
    const bool last = q + 1 == kPasses;
    HIP_CHECK(launch_order_pass(key[a], q ? idx[a] : d_index, last ? nullptr : key[b], last ? d_order : idx[b], m,
                                q * kOrderDigitBits, table, totals, st));
  }
  return RFX_OK;
}
