// Ray batches of librfx.so (include/rfx.h rfx_trace_rays, rfx_trace_rays_host): n calls of the reference's public
// Scene::trace(origin, ray, reflNumber) (Scene.h:39, Scene.cpp:73-236) in index order, on rays the caller chose.
//
// A batch is the renderer's frame path without a frame: the pre-pass of n traces (rfx_host.cpp prepass_traces, in the
// form an unsplit frame launch of n traces takes), then trace_rays_kernel (rfx_rays.h) with one lane per ray.  It keeps
// no per-frame state: no tile schedule, no per-view masks, no regroup queue, no timing sums.
#include "rfx_internal.h"

using namespace rfx;

extern "C" int rfx_trace_rays(rfx_renderer *r, const float *d_rays, uint64_t n, int32_t reflect_num,
                              uint32_t raster_width, float *d_rgb, uint32_t *d_argb, uint64_t *d_counters, void *stream)
{
  int rc;
  if ((rc = enter_call(r, d_rays && d_rgb && n && reflect_num > 0, "trace_rays",
                       "renderer, rays, colours, n > 0 and reflect_num > 0 required")) != RFX_OK)
    return rc;
  const hipStream_t st = stream_or_own(r, stream);
  const uint64_t per = rays_per_launch(r, raster_width);
  for (uint64_t a = 0; a < n; a += per)
  {
    const uint64_t m = std::min(per, n - a);
    // ray a + i takes the i-th draw of this launch, the stream running on from the launch before
    if ((rc = prepass_traces(r, m, st)) != RFX_OK) return rc;
    FrameParams P{};
    P.W = raster_width;
    P.depth = reflect_num;
    P.ss = 1;
    P.nranks = 1;
    P.p_end = m;
    P.img = d_rgb + 3 * a;
    P.argb = d_argb ? d_argb + a : nullptr;
    P.rd_state = r->rd;
    P.counters = (unsigned long long *)d_counters;
    HIP_CHECK(launch_trace_rays(r->dev, P, d_rays + 6 * a, d_counters != nullptr, st));
  }
  return RFX_OK;
}

extern "C" int rfx_trace_rays_host(rfx_renderer *r, const float *rays, uint64_t n, int32_t reflect_num,
                                   uint32_t raster_width, float *rgb, uint32_t *argb_out, uint64_t *counters)
{
  int rc;
  if ((rc = enter_call(r, rays && rgb && n && reflect_num > 0, "trace_rays_host",
                       "renderer, rays, colours, n > 0 and reflect_num > 0 required")) != RFX_OK)
    return rc;
  DevBuf<float> d_rays;
  if ((rc = d_rays.reserve((size_t)n * 6)) < 0 || (rc = r->img.reserve((size_t)n * 3)) < 0 ||
      (rc = r->argb.reserve((size_t)n)) < 0 || (rc = r->cnt.reserve(RFX_NCOUNTERS)) < 0)
    return rc;
  HIP_CHECK(hipMemcpyAsync(d_rays, rays, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, r->stream));
  if (counters) HIP_CHECK(hipMemsetAsync(r->cnt, 0, RFX_NCOUNTERS * sizeof(uint64_t), r->stream));
  rc = rfx_trace_rays(r, d_rays, n, reflect_num, raster_width, r->img, argb_out ? r->argb.p : nullptr,
                      counters ? r->cnt.p : nullptr, nullptr);
  // d_rays is freed on return: whatever was enqueued reads it before that
  if (rc != RFX_OK)
  {
    (void)hipStreamSynchronize(r->stream);
    return rc;
  }
  uint64_t c[RFX_NCOUNTERS] = {};
  HIP_CHECK(hipMemcpyAsync(rgb, r->img, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost, r->stream));
  if (argb_out) HIP_CHECK(hipMemcpyAsync(argb_out, r->argb, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
  if (counters) HIP_CHECK(hipMemcpyAsync(c, r->cnt, sizeof(c), hipMemcpyDeviceToHost, r->stream));
  HIP_CHECK(hipStreamSynchronize(r->stream));
  if (counters)
    for (int k = 0; k < RFX_NCOUNTERS; ++k) counters[k] += c[k];
  return rfx_synchronize(r);
}
