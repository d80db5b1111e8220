// The coherent order of librfx.so (include/rfx.h "Coherent order"): rfx_rays_order sorts a batch's ray indices by the
// key of origin cell and direction (rfx_order_sort.hip), and rfx_trace_rays_ordered, rfx_query_hits_ordered and
// rfx_query_occluded_ordered run the batch with wave w on the rays d_order[64 w .. 64 w + 63] (rfx_ordered.h).
//
// The order call reads the uploaded scene's key box and its own scratch and nothing else of the renderer.  The ordered
// trace is a ray batch (rfx_rays.cpp) in one launch; the ordered queries are hit queries (rfx_hits.cpp) and, like
// them, leave every stream, mask and timing sum alone.
#include "rfx_query_host.h"

using namespace rfx;

// The sort's passes: one per digit of the key.  At least two, so that d_order may be d_index: the pass that reads the one
// is not the pass that writes the other.
constexpr uint32_t kKeyBits = 3 * RFX_ORDER_CELL_BITS + 2 * RFX_ORDER_DIR_BITS;
constexpr uint32_t kPasses = (kKeyBits + kOrderDigitBits - 1) / kOrderDigitBits;
static_assert(kPasses >= 2, "d_order may be d_index: the pass that reads the one is not the pass that writes the other");

int rfx::order_scratch(rfx_renderer *r, uint32_t m)
{
  int rc;
  if ((rc = r->order_keys.reserve(2 * (size_t)m)) < 0 || (rc = r->order_idx.reserve(2 * (size_t)m)) < 0 ||
      (rc = r->order_table.reserve((size_t)kOrderDigits * order_groups(m) + kOrderDigits)) < 0)
    return rc;
  return RFX_OK;
}

int rfx::order_sort(rfx_renderer *r, uint32_t m, const uint32_t *d_index, uint32_t *d_order, hipStream_t st)
{
  uint32_t *const key[2] = {r->order_keys.p, r->order_keys.p + m}, *const idx[2] = {r->order_idx.p, r->order_idx.p + m};
  uint32_t *const table = r->order_table.p, *const totals = table + (size_t)kOrderDigits * order_groups(m);
  // pass p sorts by digit p, least significant first, from half p & 1 to the other; the first takes d_index (or the
  // index itself), the last leaves the indices alone, in the caller's array
  for (uint32_t p = 0; p < kPasses; ++p)
  {
    const uint32_t a = p & 1u, b = a ^ 1u;
    const bool last = p + 1 == kPasses;
    HIP_CHECK(launch_order_pass(key[a], p ? idx[a] : d_index, last ? nullptr : key[b], last ? d_order : idx[b], m,
                                p * kOrderDigitBits, table, totals, st));
  }
  return RFX_OK;
}

extern "C" int rfx_renderer_order_box(const rfx_renderer *r, float lo[3], float scale[3])
{
  if (!r || !lo || !scale) return fail(RFX_ERR_ARG, "renderer_order_box: bad args");
  if (!r->has_scene) return fail(RFX_ERR_STATE, "renderer_order_box: no scene");
  for (int a = 0; a < 3; ++a)
  {
    lo[a] = r->order_box.lo[a];
    scale[a] = r->order_box.scale[a];
  }
  return RFX_OK;
}

extern "C" int rfx_rays_order(rfx_renderer *r, const float *d_rays, uint64_t n, uint32_t *d_order, uint32_t *d_keys,
                              void *stream)
{
  int rc;
  if ((rc = enter_call(r, d_rays && d_order && n && n < (1ull << 31), "rays_order",
                       "renderer, rays, order and 0 < n < 2^31 required")) != RFX_OK)
    return rc;
  const hipStream_t st = stream_or_own(r, stream);
  const uint32_t m = (uint32_t)n;
  if ((rc = order_scratch(r, m)) < 0) return rc;
  HIP_CHECK(launch_order_keys(r->order_box, d_rays, m, r->order_keys.p, d_keys, st));
  return order_sort(r, m, nullptr, d_order, st);
}

extern "C" int rfx_rays_order_host(rfx_renderer *r, const float *rays, uint64_t n, uint32_t *order, uint32_t *keys)
{
  int rc;
  if ((rc = enter_call(r, rays && order && n && n < (1ull << 31), "rays_order_host",
                       "renderer, rays, order and 0 < n < 2^31 required")) != RFX_OK)
    return rc;
  DevBuf<float> d_rays;
  DevBuf<uint32_t> d_out;  // the order, then the keys
  if ((rc = d_rays.reserve((size_t)n * 6)) < 0 || (rc = d_out.reserve((size_t)n * (keys ? 2 : 1))) < 0) return rc;
  RCHECK(copy_in(r, d_rays, rays, (size_t)n * 6 * sizeof(float)));
  rc = rfx_rays_order(r, d_rays, n, d_out, keys ? d_out.p + n : nullptr, nullptr);
  if (rc == RFX_OK) rc = copy_out(r, order, d_out, (size_t)n * sizeof(uint32_t));
  if (rc == RFX_OK && keys) rc = copy_out(r, keys, d_out.p + n, (size_t)n * sizeof(uint32_t));
  return host_done(r, rc);
}

extern "C" int rfx_trace_rays_ordered(rfx_renderer *r, const float *d_rays, const uint32_t *d_order, uint64_t n,
                                      int32_t reflect_num, float *d_rgb, uint32_t *d_argb, void *stream)
{
  int rc;
  if ((rc = check_call(r, d_rays && d_order && d_rgb && n && n < (1ull << 32) && reflect_num > 0, "trace_rays_ordered",
                       "renderer, rays, order, colours, 0 < n < 2^32 and reflect_num > 0 required")) != RFX_OK)
    return rc;
  // one launch: the randDir states of the whole batch must stand, since a slot may name any ray
  if (n > r->launch_traces)
    return fail(RFX_ERR_ARG, "trace_rays_ordered: %llu rays exceed the launch limit of %llu (split the batch and order each part)",
                (unsigned long long)n, (unsigned long long)r->launch_traces);
  if ((rc = set_dev(r)) != RFX_OK) return rc;
  const hipStream_t st = stream_or_own(r, stream);
  if ((rc = prepass_traces(r, n, st)) != RFX_OK) return rc;  // ray i takes draw i
  FrameParams P{};
  P.depth = reflect_num;
  P.ss = 1;
  P.nranks = 1;
  P.p_end = n;
  P.img = d_rgb;
  P.argb = d_argb;
  P.rd_state = r->rd;
  HIP_CHECK(launch_trace_rays_ordered(r->dev, P, d_rays, d_order, st));
  return RFX_OK;
}

// The slots in launches of a linear batch's size (launch_ranges, as rfx_hits.cpp run_query); every launch sees the
// whole arrays.
static int run_query_ordered(rfx_renderer *r, const HitParams &H, const uint32_t *d_order, bool any, hipStream_t st)
{
  return launch_ranges(r, H.n, 0, [&](uint64_t a, uint64_t b) -> int {
    const HitOrderParams Q{H, d_order, a, b};
    HIP_CHECK(launch_query_hits_ordered(r->dev, Q, any, st));
    return RFX_OK;
  });
}

extern "C" int rfx_query_hits_ordered(rfx_renderer *r, const float *d_rays, const uint32_t *d_order, uint64_t n,
                                      const rfx_hit_planes *out, void *stream)
{
  int rc;
  if ((rc = enter_call(r, d_rays && d_order && n && n < (1ull << 32) && out && any_plane(out), "query_hits_ordered",
                       "renderer, rays, order, 0 < n < 2^32 and at least one output plane required")) != RFX_OK)
    return rc;
  HitParams H{};
  H.rays = d_rays;
  H.n = n;
  set_planes(H, out);
  return run_query_ordered(r, H, d_order, false, stream_or_own(r, stream));
}

extern "C" int rfx_query_occluded_ordered(rfx_renderer *r, const float *d_rays, const int32_t *d_skip,
                                          const uint32_t *d_order, uint64_t n, uint8_t *d_occluded, void *stream)
{
  int rc;
  if ((rc = enter_call(r, d_rays && d_order && n && n < (1ull << 32) && d_occluded, "query_occluded_ordered",
                       "renderer, rays, order, 0 < n < 2^32 and the result array required")) != RFX_OK)
    return rc;
  HitParams H{};
  H.rays = d_rays;
  H.skip = d_skip;
  H.n = n;
  H.occluded = d_occluded;
  return run_query_ordered(r, H, d_order, true, stream_or_own(r, stream));
}
