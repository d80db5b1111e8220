// Hit queries of librfx.so (include/rfx.h rfx_query_hits, rfx_query_occluded and their host forms): the two questions
// the reference's Scene::trace asks of its objects on every segment -- the closest hit (Scene.cpp:82-107) and the
// shadow rays' any-hit (Scene.cpp:133-143) -- on rays the caller chose.
//
// A query reads the uploaded scene and nothing else of the renderer: no pre-pass (the random streams stay where they
// are), no tile schedule, no per-view masks, no regroup queue, no timing sums, and nothing rfx_frame_rng_rewind undoes.
#include "rfx_internal.h"

using namespace rfx;

// Launches of a ray batch's size (rays_per_launch).  P holds the whole batch's pointers; each launch takes them at its
// first ray.
static int run_query(rfx_renderer *r, const HitParams &P, bool any, hipStream_t st)
{
  const uint64_t per = rays_per_launch(r, P.W);
  for (uint64_t a = 0; a < P.n; a += per)
  {
    HitParams Q = P;
    Q.n = std::min(per, P.n - a);
    Q.rays = P.rays + 6 * a;
    if (P.skip) Q.skip = P.skip + a;
    if (P.object) Q.object = P.object + a;
    if (P.distance) Q.distance = P.distance + a;
    if (P.point) Q.point = P.point + 3 * a;
    if (P.normal) Q.normal = P.normal + 3 * a;
    if (P.reflected) Q.reflected = P.reflected + 3 * a;
    if (P.colour) Q.colour = P.colour + 3 * a;
    if (P.occluded) Q.occluded = P.occluded + a;
    HIP_CHECK(launch_query_hits(r->dev, Q, any, st));
  }
  return RFX_OK;
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

extern "C" int rfx_query_hits_host(rfx_renderer *r, const float *rays, uint64_t n, uint32_t raster_width,
                                   const rfx_hit_planes *out)
{
  int rc;
  if ((rc = enter_call(r, rays && n && out && any_plane(out), "query_hits_host",
                       "renderer, rays, n > 0 and at least one output plane required")) != RFX_OK)
    return rc;
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
  if ((rc = d.reserve(total)) < 0) return rc;
  HIP_CHECK(hipMemcpyAsync(d, rays, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, r->stream));
  rfx_hit_planes dp{};
  if (host[0]) dp.object = reinterpret_cast<int32_t *>(d.p + off[0]);
  if (host[1]) dp.distance = d.p + off[1];
  if (host[2]) dp.point = d.p + off[2];
  if (host[3]) dp.normal = d.p + off[3];
  if (host[4]) dp.reflected = d.p + off[4];
  if (host[5]) dp.colour = d.p + off[5];
  rc = rfx_query_hits(r, d, n, raster_width, &dp, nullptr);
  // d is freed on return: whatever was enqueued reads and writes it before that
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

extern "C" int rfx_query_occluded_host(rfx_renderer *r, const float *rays, const int32_t *skip, uint64_t n,
                                       uint32_t raster_width, uint8_t *occluded)
{
  int rc;
  if ((rc = enter_call(r, rays && n && occluded, "query_occluded_host",
                       "renderer, rays, n > 0 and the result array required")) != RFX_OK)
    return rc;
  DevBuf<float> d_rays;
  DevBuf<int32_t> d_skip;
  DevBuf<uint8_t> d_occ;
  if ((rc = d_rays.reserve((size_t)n * 6)) < 0 || (rc = d_occ.reserve((size_t)n)) < 0 ||
      (skip && (rc = d_skip.reserve((size_t)n)) < 0))
    return rc;
  HIP_CHECK(hipMemcpyAsync(d_rays, rays, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, r->stream));
  if (skip) HIP_CHECK(hipMemcpyAsync(d_skip, skip, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, r->stream));
  rc = rfx_query_occluded(r, d_rays, skip ? d_skip.p : nullptr, n, raster_width, d_occ, nullptr);
  if (rc != RFX_OK)
  {
    (void)hipStreamSynchronize(r->stream);
    return rc;
  }
  HIP_CHECK(hipMemcpyAsync(occluded, d_occ, (size_t)n, hipMemcpyDeviceToHost, r->stream));
  HIP_CHECK(hipStreamSynchronize(r->stream));
  return RFX_OK;
}
