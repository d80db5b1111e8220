// Paths of librfx.so (include/rfx.h "Paths": rfx_paths_begin, rfx_paths_step, rfx_paths_order): Scene::trace
// (Scene.cpp:73-236) as per-ray states in planes the caller holds on the device, stepped by segment.
//
// begin is a ray batch's pre-pass (rfx_rays.cpp) with the draws written out instead of traced with; a step is a launch
// of paths_step_kernel (rfx_paths.h) per slot range and, like a hit query, leaves every stream, mask and timing sum
// alone; the order is rfx_rays_order's sort (rfx_order.cpp) on keys gathered through the index array.
#include "rfx_query_host.h"
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
  return launch_ranges(r, n, 0, [&](uint64_t a, uint64_t b) -> int {
    // path a + i takes the i-th draw of this part, the stream running on from the part before (rfx_trace_rays' split)
    if (draw) RCHECK(prepass_traces(r, b - a, st));
    HIP_CHECK(launch_paths_begin(planes_at(p, a), b - a, draw ? r->rd.p : nullptr, st));
    return RFX_OK;
  });
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
  return launch_ranges(r, slots, 0, [&](uint64_t a, uint64_t b) -> int {
    FrameParams P{};
    set_path_step(P, planes, n, d_index, a, b, upto, d_live, d_live_count);
    HIP_CHECK(launch_paths_step(r->dev, P, st));
    return RFX_OK;
  });
}

extern "C" int rfx_paths_order(rfx_renderer *r, const rfx_paths *p, uint64_t n, const uint32_t *d_index, uint64_t slots,
                               uint32_t *d_order, void *stream)
{
  int rc;
  if ((rc = enter_call(r, p && p->d_rays && d_order && n && n < (1ull << 32) && slots && slots < (1ull << 31),
                       "paths_order", "renderer, paths, order, 0 < n < 2^32 and 0 < slots < 2^31 required")) != RFX_OK)
    return rc;
  const hipStream_t st = stream_or_own(r, stream);
  const uint32_t m = (uint32_t)slots;
  if ((rc = order_scratch(r, m)) < 0) return rc;
  HIP_CHECK(launch_paths_order_keys(r->order_box, p->d_rays, (uint32_t)n, d_index, m, r->order_keys.p, st));
  // rfx_rays_order's passes; the first takes the caller's entries (or the slot itself) as the pairs' indices
  return order_sort(r, m, d_index, d_order, st);
}
