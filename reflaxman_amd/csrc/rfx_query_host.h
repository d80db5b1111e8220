// rfx_query_host.h -- what the host units of the batch calls share and no other unit needs (rfx_hits.cpp, rfx_span.cpp,
// rfx_order.cpp, rfx_paths.cpp): a batch cut into launches, a launch's part of a query's record, the host forms'
// staging, and the coherent order's sort.
#pragma once
#include "rfx_internal.h"
#include "rfx_span_types.h"

namespace rfx {

// ---- a batch in launches
// The n rays (or slots) of a batch of raster width W (0: linear, and every ordered batch) in launches of
// rays_per_launch: launch(a, b) takes [a, b) and returns RFX_OK or the error that ends the call.  A linear or raster
// launch takes its part of the record (hit_params_at, span_params_at); an ordered one takes [a, b) as its slot range
// and sees the whole arrays.
template <class Launch>
inline int launch_ranges(const rfx_renderer *r, uint64_t n, uint64_t W, Launch &&launch)
{
  const uint64_t per = rays_per_launch(r, W);
  for (uint64_t a = 0; a < n; a += per) RCHECK(launch(a, std::min(n, a + per)));
  return RFX_OK;
}

// P for its rays [a, a + m): every per-ray pointer that is given, at ray a
inline HitParams hit_params_at(const HitParams &P, uint64_t a, uint64_t m)
{
  HitParams Q = P;
  Q.n = m;
  Q.rays = P.rays + 6 * a;
  if (P.skip) Q.skip = P.skip + a;
  if (P.object) Q.object = P.object + a;
  if (P.distance) Q.distance = P.distance + a;
  if (P.point) Q.point = P.point + 3 * a;
  if (P.normal) Q.normal = P.normal + 3 * a;
  if (P.reflected) Q.reflected = P.reflected + 3 * a;
  if (P.colour) Q.colour = P.colour + 3 * a;
  if (P.occluded) Q.occluded = P.occluded + a;
  return Q;
}
// ... and the interval's ends with it
inline SpanParams span_params_at(const SpanParams &P, uint64_t a, uint64_t m)
{
  SpanParams Q = P;
  Q.H = hit_params_at(P.H, a, m);
  if (P.lo) Q.lo = P.lo + a;
  if (P.after) Q.after = P.after + a;
  if (P.hi) Q.hi = P.hi + a;
  return Q;
}

// ---- the host forms: copies on the renderer's own stream, and the call's end
inline int copy_in(rfx_renderer *r, void *dev, const void *host, size_t bytes)
{
  HIP_CHECK(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, r->stream));
  return RFX_OK;
}
inline int copy_out(rfx_renderer *r, void *host, const void *dev, size_t bytes)
{
  HIP_CHECK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, r->stream));
  return RFX_OK;
}
// A host form returns rc through this: its device arrays are freed on return, and whatever was enqueued reads and
// writes them before that, after a failure too.
inline int host_done(rfx_renderer *r, int rc)
{
  if (rc != RFX_OK)
  {
    (void)hipStreamSynchronize(r->stream);
    return rc;
  }
  HIP_CHECK(hipStreamSynchronize(r->stream));
  return RFX_OK;
}

// rfx_hits.cpp: the bodies of rfx_query_hits_host / rfx_query_hits_span_host and of rfx_query_occluded_host /
// rfx_query_occluded_span_host, after the entry's own opening tests.  spanned: the call goes through the span entry
// (rfx_query_hits_span, rfx_query_occluded_span) with `span` (host arrays, or null) staged; else through the plain one.
int query_hits_host(rfx_renderer *r, const float *rays, const rfx_ray_span *span, bool spanned, uint64_t n,
                    uint32_t raster_width, const rfx_hit_planes *out);
int query_occluded_host(rfx_renderer *r, const float *rays, const int32_t *skip, const rfx_ray_span *span, bool spanned,
                        uint64_t n, uint32_t raster_width, uint8_t *occluded);

// ---- rfx_order.cpp: the stable radix sort of m (key, index) pairs by the coherent order's key, on the renderer's
// scratch.  order_scratch reserves it; the caller's key kernel then writes the m keys to r->order_keys.p; order_sort
// runs the digit passes, the first with d_index[i] as pair i's index (null: i itself), the last leaving the sorted
// indices in d_order (which may be d_index).
int order_scratch(rfx_renderer *r, uint32_t m);
int order_sort(rfx_renderer *r, uint32_t m, const uint32_t *d_index, uint32_t *d_order, hipStream_t st);

}  // namespace rfx
