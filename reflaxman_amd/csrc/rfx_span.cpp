// Span queries of librfx.so (include/rfx.h "Ray intervals": rfx_query_hits_span, rfx_query_occluded_span, their
// ordered and host forms): the hit queries (rfx_hits.cpp) with a per-ray interval of distances.  Like them they read
// the uploaded scene and nothing else of the renderer.
#include "rfx_internal.h"
#include "rfx_span_types.h"

using namespace rfx;

static void set_span(SpanParams &P, const rfx_ray_span *span)
{
  if (!span) return;
  P.lo = span->d_lo;
  P.after = span->d_lo ? span->d_after : nullptr;
  P.hi = span->d_hi;
}

// Launches of a ray batch's size (rays_per_launch, as rfx_hits.cpp run_query): P holds the whole batch's pointers.
// Linear and raster batches: each launch takes every per-ray pointer, the interval's included, at its first ray.
// Ordered batches (d_order): slot ranges over the whole arrays.
static int run_span(rfx_renderer *r, const SpanParams &P, const uint32_t *d_order, bool any, hipStream_t st)
{
  const HitParams &H = P.H;
  const uint64_t per = rays_per_launch(r, d_order ? 0 : H.W);
  for (uint64_t a = 0; a < H.n; a += per)
  {
    SpanParams Q = P;
    if (d_order)
    {
      Q.order = d_order;
      Q.slot0 = a;
      Q.slot1 = std::min(H.n, a + per);
    }
    else
    {
      Q.H.n = std::min(per, H.n - a);
      Q.H.rays = H.rays + 6 * a;
      if (H.skip) Q.H.skip = H.skip + a;
      if (H.object) Q.H.object = H.object + a;
      if (H.distance) Q.H.distance = H.distance + a;
      if (H.point) Q.H.point = H.point + 3 * a;
      if (H.normal) Q.H.normal = H.normal + 3 * a;
      if (H.reflected) Q.H.reflected = H.reflected + 3 * a;
      if (H.colour) Q.H.colour = H.colour + 3 * a;
      if (H.occluded) Q.H.occluded = H.occluded + a;
      if (P.lo) Q.lo = P.lo + a;
      if (P.after) Q.after = P.after + a;
      if (P.hi) Q.hi = P.hi + a;
    }
    HIP_CHECK(launch_query_span(r->dev, Q, any, st));
  }
  return RFX_OK;
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

// The host forms' interval on the device: one staging array of n words per given end (every end is a 4-B word)
struct HostSpan {
  DevBuf<float> d;
  rfx_ray_span dev{};
  int put(rfx_renderer *r, const rfx_ray_span *span, uint64_t n, bool with_after)
  {
    if (!span) return RFX_OK;
    const void *host[3] = {span->d_lo, span->d_lo && with_after ? span->d_after : nullptr, span->d_hi};
    size_t words = 0;
    for (const void *h : host) words += h ? (size_t)n : 0;
    if (!words) return RFX_OK;
    int rc;
    if ((rc = d.reserve(words)) < 0) return rc;
    float *p = d.p;
    const void *at[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < 3; ++k)
      if (host[k])
      {
        HIP_CHECK(hipMemcpyAsync(p, host[k], (size_t)n * sizeof(float), hipMemcpyHostToDevice, r->stream));
        at[k] = p;
        p += n;
      }
    dev.d_lo = static_cast<const float *>(at[0]);
    dev.d_after = static_cast<const int32_t *>(at[1]);
    dev.d_hi = static_cast<const float *>(at[2]);
    return RFX_OK;
  }
};

extern "C" int rfx_query_hits_span_host(rfx_renderer *r, const float *rays, const rfx_ray_span *span, uint64_t n,
                                        uint32_t raster_width, const rfx_hit_planes *out)
{
  int rc;
  if ((rc = enter_call(r, rays && n && out && any_plane(out), "query_hits_span_host",
                       "renderer, rays, n > 0 and at least one output plane required")) != RFX_OK)
    return rc;
  // one staging array, as rfx_query_hits_host: the rays, then the requested planes one after the other
  float *const host[6] = {reinterpret_cast<float *>(out->object), out->distance, out->point, out->normal,
                          out->reflected, out->colour};
  const size_t words[6] = {(size_t)n, (size_t)n, (size_t)n * 3, (size_t)n * 3, (size_t)n * 3, (size_t)n * 3};
  size_t total = (size_t)n * 6, off[6];
  for (int k = 0; k < 6; ++k)
  {
    off[k] = total;
    if (host[k]) total += words[k];
  }
  DevBuf<float> d;
  HostSpan hs;
  if ((rc = d.reserve(total)) < 0 || (rc = hs.put(r, span, n, true)) < 0) return rc;
  HIP_CHECK(hipMemcpyAsync(d, rays, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, r->stream));
  rfx_hit_planes dp{};
  if (host[0]) dp.object = reinterpret_cast<int32_t *>(d.p + off[0]);
  if (host[1]) dp.distance = d.p + off[1];
  if (host[2]) dp.point = d.p + off[2];
  if (host[3]) dp.normal = d.p + off[3];
  if (host[4]) dp.reflected = d.p + off[4];
  if (host[5]) dp.colour = d.p + off[5];
  rc = rfx_query_hits_span(r, d, &hs.dev, n, raster_width, &dp, nullptr);
  // the arrays are freed on return: whatever was enqueued reads and writes them before that
  if (rc != RFX_OK)
  {
    (void)hipStreamSynchronize(r->stream);
    return rc;
  }
  for (int k = 0; k < 6; ++k)
    if (host[k])
      HIP_CHECK(hipMemcpyAsync(host[k], d.p + off[k], words[k] * sizeof(float), hipMemcpyDeviceToHost, r->stream));
  HIP_CHECK(hipStreamSynchronize(r->stream));
  return RFX_OK;
}

extern "C" int rfx_query_occluded_span_host(rfx_renderer *r, const float *rays, const int32_t *skip,
                                            const rfx_ray_span *span, uint64_t n, uint32_t raster_width,
                                            uint8_t *occluded)
{
  int rc;
  if ((rc = enter_call(r, rays && n && occluded, "query_occluded_span_host",
                       "renderer, rays, n > 0 and the result array required")) != RFX_OK)
    return rc;
  DevBuf<float> d_rays;
  DevBuf<int32_t> d_skip;
  DevBuf<uint8_t> d_occ;
  HostSpan hs;
  if ((rc = d_rays.reserve((size_t)n * 6)) < 0 || (rc = d_occ.reserve((size_t)n)) < 0 ||
      (skip && (rc = d_skip.reserve((size_t)n)) < 0) || (rc = hs.put(r, span, n, false)) < 0)
    return rc;
  HIP_CHECK(hipMemcpyAsync(d_rays, rays, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, r->stream));
  if (skip) HIP_CHECK(hipMemcpyAsync(d_skip, skip, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, r->stream));
  rc = rfx_query_occluded_span(r, d_rays, skip ? d_skip.p : nullptr, &hs.dev, n, raster_width, d_occ, nullptr);
  if (rc != RFX_OK)
  {
    (void)hipStreamSynchronize(r->stream);
    return rc;
  }
  HIP_CHECK(hipMemcpyAsync(occluded, d_occ, (size_t)n, hipMemcpyDeviceToHost, r->stream));
  HIP_CHECK(hipStreamSynchronize(r->stream));
  return RFX_OK;
}
