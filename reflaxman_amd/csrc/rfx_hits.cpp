// Hit queries of librfx.so (include/rfx.h rfx_query_hits, rfx_query_occluded and their host forms): the two questions
// the reference's Scene::trace asks of its objects on every segment -- the closest hit (Scene.cpp:82-107) and the
// shadow rays' any-hit (Scene.cpp:133-143) -- on rays the caller chose.
//
// A query reads the uploaded scene and nothing else of the renderer: no pre-pass (the random streams stay where they
// are), no tile schedule, no per-view masks, no regroup queue, no timing sums, and nothing rfx_frame_rng_rewind undoes.
#include "rfx_query_host.h"

using namespace rfx;

// Launches of a ray batch's size (launch_ranges).  P holds the whole batch's pointers; each launch takes them at its
// first ray.
static int run_query(rfx_renderer *r, const HitParams &P, bool any, hipStream_t st)
{
  return launch_ranges(r, P.n, P.W, [&](uint64_t a, uint64_t b) -> int {
    const HitParams Q = hit_params_at(P, a, b - a);
    HIP_CHECK(launch_query_hits(r->dev, Q, any, st));
    return RFX_OK;
  });
}

extern "C" int rfx_query_hits(rfx_renderer *r, const float *d_rays, uint64_t n, uint32_t raster_width,
                              const rfx_hit_planes *out, void *stream)
{
  int rc;
  if ((rc = enter_call(r, d_rays && n && out && any_plane(out), "query_hits",
                       "renderer, rays, n > 0 and at least one output plane required")) != RFX_OK)
    return rc;
  HitParams P{};
  P.rays = d_rays;
  P.n = n;
  P.W = raster_width;
  set_planes(P, out);
  return run_query(r, P, false, stream_or_own(r, stream));
}

extern "C" int rfx_query_occluded(rfx_renderer *r, const float *d_rays, const int32_t *d_skip, uint64_t n,
                                  uint32_t raster_width, uint8_t *d_occluded, void *stream)
{
  int rc;
  if ((rc = enter_call(r, d_rays && n && d_occluded, "query_occluded",
                       "renderer, rays, n > 0 and the result array required")) != RFX_OK)
    return rc;
  HitParams P{};
  P.rays = d_rays;
  P.skip = d_skip;
  P.n = n;
  P.W = raster_width;
  P.occluded = d_occluded;
  return run_query(r, P, true, stream_or_own(r, stream));
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
        RCHECK(copy_in(r, p, host[k], (size_t)n * sizeof(float)));
        at[k] = p;
        p += n;
      }
    dev.d_lo = static_cast<const float *>(at[0]);
    dev.d_after = static_cast<const int32_t *>(at[1]);
    dev.d_hi = static_cast<const float *>(at[2]);
    return RFX_OK;
  }
};

int rfx::query_hits_host(rfx_renderer *r, const float *rays, const rfx_ray_span *span, bool spanned, uint64_t n,
                         uint32_t raster_width, const rfx_hit_planes *out)
{
  // one staging array: the rays, then the requested planes one after the other (every plane is made of 4-B words)
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
  int rc;
  if ((rc = d.reserve(total)) < 0 || (rc = hs.put(r, span, n, true)) < 0) return rc;
  RCHECK(copy_in(r, d, rays, (size_t)n * 6 * sizeof(float)));
  rfx_hit_planes dp{};
  if (host[0]) dp.object = reinterpret_cast<int32_t *>(d.p + off[0]);
  if (host[1]) dp.distance = d.p + off[1];
  if (host[2]) dp.point = d.p + off[2];
  if (host[3]) dp.normal = d.p + off[3];
  if (host[4]) dp.reflected = d.p + off[4];
  if (host[5]) dp.colour = d.p + off[5];
  rc = spanned ? rfx_query_hits_span(r, d, &hs.dev, n, raster_width, &dp, nullptr)
               : rfx_query_hits(r, d, n, raster_width, &dp, nullptr);
  for (int k = 0; k < 6 && rc == RFX_OK; ++k)
    if (host[k]) rc = copy_out(r, host[k], d.p + off[k], words[k] * sizeof(float));
  return host_done(r, rc);
}

int rfx::query_occluded_host(rfx_renderer *r, const float *rays, const int32_t *skip, const rfx_ray_span *span,
                             bool spanned, uint64_t n, uint32_t raster_width, uint8_t *occluded)
{
  DevBuf<float> d_rays;
  DevBuf<int32_t> d_skip;
  DevBuf<uint8_t> d_occ;
  HostSpan hs;
  int rc;
  if ((rc = d_rays.reserve((size_t)n * 6)) < 0 || (rc = d_occ.reserve((size_t)n)) < 0 ||
      (skip && (rc = d_skip.reserve((size_t)n)) < 0) || (rc = hs.put(r, span, n, false)) < 0)
    return rc;
  RCHECK(copy_in(r, d_rays, rays, (size_t)n * 6 * sizeof(float)));
  if (skip) RCHECK(copy_in(r, d_skip, skip, (size_t)n * sizeof(int32_t)));
  rc = spanned ? rfx_query_occluded_span(r, d_rays, skip ? d_skip.p : nullptr, &hs.dev, n, raster_width, d_occ, nullptr)
               : rfx_query_occluded(r, d_rays, skip ? d_skip.p : nullptr, n, raster_width, d_occ, nullptr);
  if (rc == RFX_OK) rc = copy_out(r, occluded, d_occ, (size_t)n);
  return host_done(r, rc);
}

extern "C" int rfx_query_hits_host(rfx_renderer *r, const float *rays, uint64_t n, uint32_t raster_width,
                                   const rfx_hit_planes *out)
{
  int rc;
  if ((rc = enter_call(r, rays && n && out && any_plane(out), "query_hits_host",
                       "renderer, rays, n > 0 and at least one output plane required")) != RFX_OK)
    return rc;
  return query_hits_host(r, rays, nullptr, false, n, raster_width, out);
}

extern "C" int rfx_query_occluded_host(rfx_renderer *r, const float *rays, const int32_t *skip, uint64_t n,
                                       uint32_t raster_width, uint8_t *occluded)
{
  int rc;
  if ((rc = enter_call(r, rays && n && occluded, "query_occluded_host",
                       "renderer, rays, n > 0 and the result array required")) != RFX_OK)
    return rc;
  return query_occluded_host(r, rays, skip, nullptr, false, n, raster_width, occluded);
}
