// Device known-answer entry points of librfx.so (include/rfx.h rfx_kat_*): each runs the trace kernel's own device
// code (rfx_kernels.hip kat_*) on host arrays, synchronously.  Only the tests call them.
#include <algorithm>
#include <string>
#include <vector>

#include "rfx_internal.h"

using namespace rfx;

// an error a callee recorded (rfx_last_error), under the entry point's name
static int named(const char *who, int rc)
{
  const std::string cause = rfx_last_error();
  return fail(rc, "%s: %s", who, cause.c_str());
}

// a device array of n elements (at least one), holding src's when given
template <class T>
static int kat_buffer(DevBuf<T> &dev, size_t n, const T *src)
{
  int rc;
  if ((rc = dev.reserve(n ? n : 1)) < 0) return rc;
  if (src && n) HIP_CHECK(hipMemcpy(dev, src, n * sizeof(T), hipMemcpyHostToDevice));
  return RFX_OK;
}

static int kat_run(rfx_renderer *r, int what, int tex, const void *in, size_t in_elems, const int32_t *objs,
                   uint64_t n, void *out, size_t out_elems)
{
  RCHECK(set_dev(r));
  if (n >= (1ull << 31)) return fail(RFX_ERR_ARG, "kat: n too large");
  DevBuf<float> d_in, d_out;
  DevBuf<int32_t> d_obj;
  RCHECK(kat_buffer(d_in, in_elems, (const float *)in));
  if (objs) RCHECK(kat_buffer(d_obj, (size_t)n, objs));
  RCHECK(kat_buffer(d_out, out_elems, (const float *)nullptr));
  hipError_t e = launch_kat(what, r->dev, tex, d_in, d_obj, (uint32_t)n, d_out, r->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
  if (e == hipSuccess) e = hipMemcpy(out, d_out, out_elems * 4, hipMemcpyDeviceToHost);
  return e == hipSuccess ? RFX_OK : fail(RFX_ERR_HIP, "kat: %s", hipGetErrorString(e));
}

extern "C" int rfx_kat_objects(rfx_renderer *r, const float *rays, const int32_t *objects, uint64_t n, float *out)
{
  if (!r || (n && (!rays || !objects || !out))) return fail(RFX_ERR_ARG, "kat_objects: bad args");
  if (!r->has_scene) return fail(RFX_ERR_STATE, "kat_objects: no scene uploaded");
  for (uint64_t i = 0; i < n; ++i)
    if (objects[i] < 0 || objects[i] >= r->dev.n_obj) return fail(RFX_ERR_ARG, "kat_objects: object %d", objects[i]);
  return kat_run(r, 0, 0, rays, (size_t)n * 6, objects, n, out, (size_t)n * 15);
}

extern "C" int rfx_kat_texels(rfx_renderer *r, int texture, const float *in, uint64_t n, float *out)
{
  if (!r || (n && (!in || !out))) return fail(RFX_ERR_ARG, "kat_texels: bad args");
  if (!r->has_scene) return fail(RFX_ERR_STATE, "kat_texels: no scene uploaded");
  if (texture >= r->dev.n_tex) return fail(RFX_ERR_ARG, "kat_texels: texture %d", texture);
  return kat_run(r, 1, texture, in, (size_t)n * (texture >= 0 ? 2 : 3), nullptr, n, out, (size_t)n * 3);
}

extern "C" int rfx_kat_powf(rfx_renderer *r, const float *xy, uint64_t n, float *out)
{
  if (!r || (n && (!xy || !out))) return fail(RFX_ERR_ARG, "kat_powf: bad args");
  return kat_run(r, 2, 0, xy, (size_t)n * 2, nullptr, n, out, (size_t)n);
}

extern "C" int rfx_kat_far_light(rfx_renderer *r, const float *points, uint64_t n, float *out)
{
  if (!r || (n && (!points || !out))) return fail(RFX_ERR_ARG, "kat_far_light: bad args");
  if (!r->has_scene || r->dev.n_light < 1) return fail(RFX_ERR_STATE, "kat_far_light: no scene with a light uploaded");
  return kat_run(r, 4, 0, points, (size_t)n * 3, nullptr, n, out, (size_t)n * 8);
}

extern "C" int rfx_kat_argb(rfx_renderer *r, const float *rgb, uint64_t n, uint32_t *out)
{
  if (!r || (n && (!rgb || !out))) return fail(RFX_ERR_ARG, "kat_argb: bad args");
  return kat_run(r, 3, 0, rgb, (size_t)n * 3, nullptr, n, out, (size_t)n);
}

extern "C" int rfx_kat_powf_cube(rfx_renderer *r, uint64_t counts[2])
{
  if (!r || !counts) return fail(RFX_ERR_ARG, "kat_powf_cube: bad args");
  DevBuf<unsigned long long> d;
  int rc;
  if ((rc = d.reserve(2)) < 0) return named("kat_powf_cube", rc);
  hipError_t e = hipMemsetAsync(d, 0, 2 * sizeof(unsigned long long), r->stream);
  // every float in [0, 1]: bit patterns 0 .. 0x3f800000, in launches of 2^28
  for (uint64_t first = 0; e == hipSuccess && first <= 0x3f800000ull; first += 1ull << 28)
    e = launch_kat_powf_cube((uint32_t)first, (uint32_t)std::min<uint64_t>(1ull << 28, 0x3f800001ull - first), d, r->stream);
  unsigned long long h[2] = {0, 0};
  if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
  if (e == hipSuccess) e = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(RFX_ERR_HIP, "kat_powf_cube: %s", hipGetErrorString(e));
  counts[0] = h[0];
  counts[1] = h[1];
  return RFX_OK;
}

extern "C" int rfx_kat_div(rfx_renderer *r, uint64_t first, uint64_t n, uint64_t counts[3])
{
  if (!r || !counts) return fail(RFX_ERR_ARG, "kat_div: bad args");
  RCHECK(set_dev(r));
  DevBuf<unsigned long long> d;
  int rc;
  if ((rc = d.reserve(3)) < 0) return named("kat_div", rc);
  hipError_t e = hipMemsetAsync(d, 0, 3 * sizeof(unsigned long long), r->stream);
  for (uint64_t k = 0; e == hipSuccess && k < n; k += 1ull << 28)  // launches of up to 2^28 pairs
    e = launch_kat_div(first + k, (uint32_t)std::min<uint64_t>(1ull << 28, n - k), d, r->stream);
  unsigned long long h[3] = {0, 0, 0};
  if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
  if (e == hipSuccess) e = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(RFX_ERR_HIP, "kat_div: %s", hipGetErrorString(e));
  for (int i = 0; i < 3; ++i) counts[i] = h[i];
  return RFX_OK;
}

extern "C" uint32_t rfx_rng_seq_blocks(void) { return rng_seq_blocks(); }

extern "C" int rfx_kat_rng_seq_prefix(rfx_renderer *r, uint32_t *prefix)
{
  if (!r || !prefix) return fail(RFX_ERR_ARG, "kat_rng_seq_prefix: bad args");
  RCHECK(set_dev(r));
  RCHECK(ensure_seq_table(r, r->stream));
  HIP_CHECK(hipStreamSynchronize(r->stream));
  HIP_CHECK(hipMemcpy(prefix, r->seq_p, ((size_t)rng_seq_blocks() + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RFX_OK;
}

extern "C" int rfx_kat_rng_seq_legacy(rfx_renderer *r, uint32_t *counts)
{
  if (!r || !counts) return fail(RFX_ERR_ARG, "kat_rng_seq_legacy: bad args");
  RCHECK(set_dev(r));
  const uint64_t nb = rng_seq_blocks();
  std::vector<uint32_t> jump(2 * (256 + nb));
  rng_jump_table(nb, jump.data());
  DevBuf<uint32_t> d_jump, d_cnt, d_origin;
  int rc;
  if ((rc = d_jump.reserve(jump.size())) < 0 || (rc = d_cnt.reserve(nb)) < 0 || (rc = d_origin.reserve(1)) < 0)
    return named("kat_rng_seq_legacy", rc);
  // both on the kernel's stream: it is a non-blocking one, which the null stream's copies and memsets are not ordered
  // with (and a memset may return before it has run)
  hipError_t e = hipMemcpyAsync(d_jump, jump.data(), jump.size() * sizeof(uint32_t), hipMemcpyHostToDevice, r->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_origin, 0, sizeof(uint32_t), r->stream);  // the cycle's origin state
  if (e == hipSuccess) e = launch_rng_count(d_origin, d_jump, d_cnt, 0, nb, nullptr, r->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
  if (e == hipSuccess) e = hipMemcpy(counts, d_cnt, nb * sizeof(uint32_t), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(RFX_ERR_HIP, "kat_rng_seq_legacy: %s", hipGetErrorString(e));
  return RFX_OK;
}

extern "C" int rfx_kat_kernarg(rfx_renderer *r, int swapped, uint32_t out[3])
{
  if (!r || !out) return fail(RFX_ERR_ARG, "kat_kernarg: bad args");
  if (!r->has_scene) return fail(RFX_ERR_STATE, "kat_kernarg: no scene uploaded");
  RCHECK(set_dev(r));
  FrameParams P;
  uint32_t *w = (uint32_t *)&P;  // every word distinct, so a shifted read cannot match by accident
  for (size_t i = 0; i < sizeof(P) / 4; ++i) w[i] = 0x9E3779B9u * (uint32_t)(i + 1);
  DevBuf<uint32_t> d;
  int rc;
  if ((rc = d.reserve(3)) < 0) return named("kat_kernarg", rc);
  hipError_t e = hipMemsetAsync(d, 0xFF, 3 * sizeof(uint32_t), r->stream);
  if (e == hipSuccess) e = launch_kat_kernarg(r->dev, P, swapped, d, r->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
  if (e == hipSuccess) e = hipMemcpy(out, d, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(RFX_ERR_HIP, "kat_kernarg: %s", hipGetErrorString(e));
  return RFX_OK;
}
