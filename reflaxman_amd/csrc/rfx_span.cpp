// Span queries of librfx.so (include/rfx.h "Ray intervals": rfx_query_hits_span, rfx_query_occluded_span, their
// ordered and host forms): the hit queries (rfx_hits.cpp) with a per-ray interval of distances.  Like them they read
// the uploaded scene and nothing else of the renderer.
#include "rfx_query_host.h"

using namespace rfx;

static void set_span(SpanParams &P, const rfx_ray_span *span)
{
  if (!span) return;
  P.lo = span->d_lo;
  P.after = span->d_lo ? span->d_after : nullptr;
  P.hi = span->d_hi;
}

// Launches of a ray batch's size (launch_ranges, as rfx_hits.cpp run_query): P holds the whole batch's pointers.
// Linear and raster batches: each launch takes every per-ray pointer, the interval's included, at its first ray.
// Ordered batches (d_order): slot ranges over the whole arrays.
static int run_span(rfx_renderer *r, const SpanParams &P, const uint32_t *d_order, bool any, hipStream_t st)
{
  return launch_ranges(r, P.H.n, d_order ? 0 : P.H.W, [&](uint64_t a, uint64_t b) -> int {
    SpanParams Q = d_order ? P : span_params_at(P, a, b - a);
    if (d_order)
    {
      Q.order = d_order;
      Q.slot0 = a;
      Q.slot1 = b;
    }
    HIP_CHECK(launch_query_span(r->dev, Q, any, st));
    return RFX_OK;
  });
}

extern "C" int rfx_query_hits_span(rfx_renderer *r, const float *d_rays, const rfx_ray_span *span, uint64_t n,
                                   uint32_t raster_width, const rfx_hit_planes *out, void *stream)
{
  int rc;
  if ((rc = enter_call(r, d_rays && n && out && any_plane(out), "query_hits_span",
                       "renderer, rays, n > 0 and at least one output plane required")) != RFX_OK)
    return rc;
  SpanParams P{};
  P.H.rays = d_rays;
  P.H.n = n;
  P.H.W = raster_width;
  set_planes(P.H, out);
  set_span(P, span);
  return run_span(r, P, nullptr, false, stream_or_own(r, stream));
}

extern "C" int rfx_query_occluded_span(rfx_renderer *r, const float *d_rays, const int32_t *d_skip,
                                       const rfx_ray_span *span, uint64_t n, uint32_t raster_width, uint8_t *d_occluded,
                                       void *stream)
{
  int rc;
  if ((rc = enter_call(r, d_rays && n && d_occluded, "query_occluded_span",
                       "renderer, rays, n > 0 and the result array required")) != RFX_OK)
    return rc;
  SpanParams P{};
  P.H.rays = d_rays;
  P.H.skip = d_skip;
  P.H.n = n;
  P.H.W = raster_width;
  P.H.occluded = d_occluded;
  set_span(P, span);
  P.after = nullptr;
  return run_span(r, P, nullptr, true, stream_or_own(r, stream));
}

extern "C" int rfx_query_hits_span_ordered(rfx_renderer *r, const float *d_rays, const rfx_ray_span *span,
                                           const uint32_t *d_order, uint64_t n, const rfx_hit_planes *out, void *stream)
{
  int rc;
  if ((rc = enter_call(r, d_rays && d_order && n && n < (1ull << 32) && out && any_plane(out), "query_hits_span_ordered",
                       "renderer, rays, order, 0 < n < 2^32 and at least one output plane required")) != RFX_OK)
    return rc;
  SpanParams P{};
  P.H.rays = d_rays;
  P.H.n = n;
  set_planes(P.H, out);
  set_span(P, span);
  return run_span(r, P, d_order, false, stream_or_own(r, stream));
}

extern "C" int rfx_query_occluded_span_ordered(rfx_renderer *r, const float *d_rays, const int32_t *d_skip,
                                               const rfx_ray_span *span, const uint32_t *d_order, uint64_t n,
                                               uint8_t *d_occluded, void *stream)
{
  int rc;
  if ((rc = enter_call(r, d_rays && d_order && n && n < (1ull << 32) && d_occluded, "query_occluded_span_ordered",
                       "renderer, rays, order, 0 < n < 2^32 and the result array required")) != RFX_OK)
    return rc;
  SpanParams P{};
  P.H.rays = d_rays;
  P.H.skip = d_skip;
  P.H.n = n;
  P.H.occluded = d_occluded;
  set_span(P, span);
  P.after = nullptr;
  return run_span(r, P, d_order, true, stream_or_own(r, stream));
}

// The host forms: rfx_hits.cpp's, with the interval staged beside the rays
extern "C" int rfx_query_hits_span_host(rfx_renderer *r, const float *rays, const rfx_ray_span *span, uint64_t n,
                                        uint32_t raster_width, const rfx_hit_planes *out)
{
  int rc;
  if ((rc = enter_call(r, rays && n && out && any_plane(out), "query_hits_span_host",
                       "renderer, rays, n > 0 and at least one output plane required")) != RFX_OK)
    return rc;
  return query_hits_host(r, rays, span, true, n, raster_width, out);
}

extern "C" int rfx_query_occluded_span_host(rfx_renderer *r, const float *rays, const int32_t *skip,
                                            const rfx_ray_span *span, uint64_t n, uint32_t raster_width,
                                            uint8_t *occluded)
{
  int rc;
  if ((rc = enter_call(r, rays && n && occluded, "query_occluded_span_host",
                       "renderer, rays, n > 0 and the result array required")) != RFX_OK)
    return rc;
  return query_occluded_host(r, rays, skip, span, true, n, raster_width, occluded);
}
