// The renderer of librfx.so: the rfx_renderer_* / rfx_render_* / rfx_frame_* C-ABI of include/rfx.h.
//
// rfx_renderer_set_scene uploads what rfx_scene.cpp's SceneBuild made to SoA device arrays (rfx_types.h), and
// rfx_render_frame enqueues the RNG pre-pass + trace kernel on one HIP stream without any host synchronisation.
#include <string.h>

#include <algorithm>

#include "rfx_internal.h"
#include "rfx_math.h"

#pragma clang fp contract(off)

using namespace rfx;

extern "C" int rfx_abi_version(void) { return RFX_ABI_VERSION; }

// ============================================================== renderer
// RFX_TILE_ORDER_MIN_TILES counts 8x8 wave tiles: C3 (3840x2160) has 129,600, C2 (1920x1080) 32,400, a C4 rank's strips
// at N = 8 65,280 (their trace 0.41 ms unsorted vs 0.34 at N = 4 per eighth of the frame, tools/root_overhead.py)
// RFX_QUEUE_SORT: regrouped frames: the bounce kernel takes the parked traces bucket by bucket (1) or in park order (0).
// tools/ab.py, C5 trace + bounce: park after 3 sorted 3.48 vs 3.40 ms unsorted (+2.3%); after 2: 3.53 vs 3.69 (-4.2%,
// still above park-3 unsorted).  Park order keeps a tile's survivors together, which a coarse cell key cannot beat.
// The tile sort: on the trace launch's own stream (RFX_TILE_SORT_MAIN=0: on a side stream beside the next frame's RNG
// pre-pass, joined by an event pair) every RFX_TILE_SORT_EVERY-th launch.  Trace time against raster order (tools/ab.py,
// C3): every launch -7.5%, every 4th -9.4%, every 16th -9.8%.  The side stream hid the sort but not its events: a kernel
// trace shows ~20 us between two traces on a sorting frame beyond a plain one (fork before the count, join before the
// trace).  Frame ms, interleaved A/B (profiles/r06/ab/*_tile_sort_r6q.jsonl): C3 every 4th beside 0.6556, on the stream
// 0.6526, every 16th beside 0.6513, every 16th on the stream 0.6485 (-1.1%); C2 d4 -0.9%, the 4x4 screenshot -0.4%.
constexpr uint64_t kMaxLaunchTraces = 1ull << 31;  // the band scan's 32-bit offsets (rfx_kernels.hip rng_band_range)
// RFX_SCAN_EMIT_BLOCKS: one-device emits of more RNG blocks than this scan the counts first (rng_band_range) instead of
// summing them per block (rng_emit: O(nblk^2) reads); C3 has 4,066 blocks, the 4x4 screenshot frame 16,219.  Re-checked
// with the multi-workgroup tile scan (round 6, profiles/r06/ab/*_scan_emit_threshold_r6x.jsonl): a threshold of 4,096
// makes the C4 and screenshot pre-passes 0.093 -> 0.104 ms, so the per-block sums stay up to 16,384 blocks

static int timing_event(rfx_renderer *r, hipStream_t st)
{
  if (!r->timing_this) return RFX_OK;
  if (r->events_used == r->events.size())
  {
    hipEvent_t e;
    HIP_CHECK(hipEventCreate(&e));
    r->events.push_back(e);
  }
  HIP_CHECK(hipEventRecord(r->events[r->events_used++], st));
  return RFX_OK;
}

// the first event of a frame: decides whether this frame is one of the timed ones
static int timing_start(rfx_renderer *r, hipStream_t st)
{
  r->timing_this = r->timing && r->timing_seq++ % r->timing_every == 0;
  return timing_event(r, st);
}

extern "C" int rfx_renderer_set_timing(rfx_renderer *r, int enable)
{
  if (!r || enable < 0) return fail(RFX_ERR_ARG, "set_timing: null renderer or negative period");
  r->timing = enable != 0;
  r->timing_every = enable > 1 ? (uint32_t)enable : 1u;
  r->timing_seq = 0;
  r->timing_this = false;
  r->events_used = 0;
  return RFX_OK;
}

extern "C" int rfx_renderer_get_timing(rfx_renderer *r, double *prepass_ms, double *trace_ms, uint64_t *frames)
{
  if (!r) return fail(RFX_ERR_ARG, "get_timing: null renderer");
  double pre = 0.0, tr = 0.0;
  const size_t n = r->events_used / 3;
  if (n) HIP_CHECK(hipEventSynchronize(r->events[3 * n - 1]));
  for (size_t i = 0; i < n; ++i)
  {
    float a = 0.0f, b = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&a, r->events[3 * i], r->events[3 * i + 1]));
    HIP_CHECK(hipEventElapsedTime(&b, r->events[3 * i + 1], r->events[3 * i + 2]));
    pre += a;
    tr += b;
  }
  r->events_used = 0;
  if (prepass_ms) *prepass_ms = pre;
  if (trace_ms) *trace_ms = tr;
  if (frames) *frames = n;
  return RFX_OK;
}

rfx_renderer::rfx_renderer()
    : launch_traces(RFX_LAUNCH_TRACES), rng_prepass(RFX_RNG_SEQ), tile_mode(RFX_TILE_ORDER_DEFAULT),
      queue_sort(RFX_QUEUE_SORT)
{
}

int rfx::set_dev(rfx_renderer *r)
{
  HIP_CHECK(hipSetDevice(r->device));
  return RFX_OK;
}

extern "C" int rfx_renderer_create(rfx_renderer **out, int device)
{
  if (!out) return fail(RFX_ERR_ARG, "renderer_create: null out");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(RFX_ERR_NODEV, "no HIP device");
  if (device < 0 || device >= n) return fail(RFX_ERR_ARG, "device %d out of range (%d devices)", device, n);
  rfx_renderer *r = new rfx_renderer();
  r->device = device;
  int rc;
  if ((rc = set_dev(r)) != RFX_OK) { delete r; return rc; }
  if (hipStreamCreateWithFlags(&r->own_stream, hipStreamNonBlocking) != hipSuccess ||
      r->rng.seed.reserve(3) < 0 || r->err.reserve(1) < 0)
  {
    delete r;
    return fail(RFX_ERR_HIP, "renderer_create: HIP allocation failed");
  }
  r->stream = r->own_stream;
  if (hipDeviceGetAttribute(&r->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || r->cus <= 0)
    r->cus = 256;
  const uint32_t seeds[2] = {1350490027u, 1350490027u};
  if (hipMemcpy(r->rng.seed, seeds, sizeof(seeds), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(r->err, 0, sizeof(int)) != hipSuccess)
  {
    delete r;
    return fail(RFX_ERR_HIP, "renderer_create: HIP init copy failed");
  }
  *out = r;
  return RFX_OK;
}

static void free_scene(rfx_renderer *r)
{
  for (void *p : r->scene_allocs) (void)hipFree(p);
  r->scene_allocs.clear();
  r->has_scene = false;
}

extern "C" void rfx_renderer_destroy(rfx_renderer *r)
{
  if (!r) return;
  (void)hipSetDevice(r->device);
  (void)hipStreamSynchronize(r->stream);
  free_scene(r);
  for (hipEvent_t e : r->events) (void)hipEventDestroy(e);
  if (r->tile_stream) (void)hipStreamSynchronize(r->tile_stream);
  if (r->tile_fork) (void)hipEventDestroy(r->tile_fork);
  if (r->tile_join) (void)hipEventDestroy(r->tile_join);
  if (r->tile_stream) (void)hipStreamDestroy(r->tile_stream);
  if (r->split_stream)
  {
    (void)hipStreamSynchronize(r->split_stream);
    (void)hipStreamDestroy(r->split_stream);
  }
  for (hipEvent_t e : r->split_ev)
    if (e) (void)hipEventDestroy(e);
  if (r->own_stream) (void)hipStreamDestroy(r->own_stream);
  delete r;  // and, with it, every DevBuf
}

extern "C" int rfx_build_options(void)
{
  return (RFX_PRIM_SSAA ? RFX_BUILD_PRIM_SSAA : 0) |  // (bit 0, RFX_BUILD_PRIM_LARGE: reserved, always 0)
         (RFX_PRIM_LANES ? RFX_BUILD_PRIM_LANES : 0) | (RFX_ONE_LIGHT ? RFX_BUILD_ONE_LIGHT : 0) |
         (RFX_BVH_LEAF_PAIRS << 8);
}

extern "C" int rfx_renderer_set_launch_traces(rfx_renderer *r, uint64_t max_traces)
{
  if (!r) return fail(RFX_ERR_ARG, "renderer_set_launch_traces: null renderer");
  r->launch_traces = max_traces ? std::min(max_traces, kMaxLaunchTraces) : (uint64_t)RFX_LAUNCH_TRACES;
  return RFX_OK;
}

extern "C" int rfx_renderer_device(const rfx_renderer *r) { return r ? r->device : -1; }

extern "C" int rfx_renderer_set_tile_order(rfx_renderer *r, int mode)
{
  if (!r || mode < 0 || mode > 3) return fail(RFX_ERR_ARG, "renderer_set_tile_order: mode 0, 1, 2 or 3");
  r->tile_mode = mode;
  return RFX_OK;
}

extern "C" int rfx_renderer_set_prim_masks(rfx_renderer *r, int mode)
{
  if (!r || mode < 0 || mode > 2) return fail(RFX_ERR_ARG, "renderer_set_prim_masks: mode 0, 1 or 2");
  r->prim_mode = mode;
  r->prim_key.clear();
  r->prim_seen.clear();
  return RFX_OK;
}

extern "C" int rfx_renderer_set_prim_exact(rfx_renderer *r, int on)
{
  if (!r || on < 0 || on > 1) return fail(RFX_ERR_ARG, "renderer_set_prim_exact: 0 or 1");
  r->prim_exact = on;
  r->prim_key.clear();  // the next frame builds its masks again (the views seen stay: a repeated view still counts)
  return RFX_OK;
}

extern "C" int rfx_renderer_get_prim_masks(rfx_renderer *r, uint64_t *host, uint64_t capacity, uint64_t *words)
{
  if (!r || !words) return fail(RFX_ERR_ARG, "renderer_get_prim_masks: null argument");
  int rc;
  if ((rc = set_dev(r)) != RFX_OK) return rc;
  const uint64_t n = r->prim_key.empty() ? 0 : r->prim_words;
  *words = n;
  if (!n || !host) return RFX_OK;  // nothing held, or the length alone was asked for
  if (capacity < n) return fail(RFX_ERR_ARG, "renderer_get_prim_masks: the host array is too short");
  HIP_CHECK(hipStreamSynchronize(r->prim_on));
  HIP_CHECK(hipMemcpy(host, r->prim_mask.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return RFX_OK;
}

extern "C" int rfx_renderer_set_rng_prepass(rfx_renderer *r, int mode)
{
  if (!r || mode < 0 || mode > 1) return fail(RFX_ERR_ARG, "renderer_set_rng_prepass: mode 0 or 1");
  r->rng_prepass = mode;
  return RFX_OK;
}

extern "C" int rfx_renderer_prepass_form(const rfx_renderer *r)
{
  if (!r) return fail(RFX_ERR_ARG, "renderer_prepass_form: null renderer");
  return r->rng.prepass_form;
}

extern "C" uint32_t rfx_rng_triple_index(uint32_t state) { return rng_seq_index_of(state); }

extern "C" int rfx_renderer_bounce_form(const rfx_renderer *r)
{
  if (!r) return fail(RFX_ERR_ARG, "renderer_bounce_form: null renderer");
  return r->bounce_form;
}

extern "C" int rfx_renderer_set_regroup(rfx_renderer *r, int park_after)
{
  if (!r || park_after < -1) return fail(RFX_ERR_ARG, "renderer_set_regroup: -1 (default), 0 (off) or segments >= 1");
  r->park_after = park_after;
  return RFX_OK;
}

extern "C" int rfx_renderer_set_regroup_sort(rfx_renderer *r, int on)
{
  if (!r || on < 0 || on > 1) return fail(RFX_ERR_ARG, "renderer_set_regroup_sort: 0 or 1");
  r->queue_sort = on;
  return RFX_OK;
}

extern "C" int rfx_renderer_set_stream(rfx_renderer *r, void *s)
{
  if (!r) return fail(RFX_ERR_ARG, "set_stream: null renderer");
  r->stream = s ? (hipStream_t)s : r->own_stream;
  return RFX_OK;
}

template <class T>
static int upload(rfx_renderer *r, const std::vector<T> &v, const T **dst)
{
  if (v.empty()) { *dst = nullptr; return RFX_OK; }
  void *p = nullptr;
  HIP_CHECK(hipMalloc(&p, v.size() * sizeof(T)));
  r->scene_allocs.push_back(p);
  HIP_CHECK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  *dst = (const T *)p;
  return RFX_OK;
}

extern "C" int rfx_renderer_set_tri_accel(rfx_renderer *r, int mode)
{
  if (!r || mode < -1 || mode > 2)
    return fail(RFX_ERR_ARG, "renderer_set_tri_accel: -1 (automatic), 0 (off), 1 (on) or 2 (on, narrow bundles too)");
  r->tri_accel = mode;
  return RFX_OK;
}

extern "C" int rfx_renderer_accel_info(const rfx_renderer *r, rfx_accel_info *out)
{
  if (!r || !out) return fail(RFX_ERR_ARG, "renderer_accel_info: bad args");
  if (!r->has_scene) return fail(RFX_ERR_STATE, "renderer_accel_info: no scene");
  *out = r->accel;
  return RFX_OK;
}

extern "C" int rfx_renderer_set_scene(rfx_renderer *r, const rfx_scene *s)
{
  if (!r || !s) return fail(RFX_ERR_ARG, "set_scene: bad args");
  int rc;
  if ((rc = set_dev(r)) != RFX_OK) return rc;
  HIP_CHECK(hipStreamSynchronize(r->stream));
  free_scene(r);
  const SceneBuild B(*s, r->tri_accel);
  DevScene d = B.d;
  if ((rc = upload(r, B.sg, &d.sph_geo)) || (rc = upload(r, B.sp, &d.sph_pair)) || (rc = upload(r, B.sm, &d.sph_mat)) ||
      (rc = upload(r, B.si, &d.sph_info)) || (rc = upload(r, B.tg, &d.tri_geo)) || (rc = upload(r, B.ts, &d.tri_shade)) ||
      (rc = upload(r, B.tm, &d.tri_mat)) || (rc = upload(r, B.lr, &d.lights)) || (rc = upload(r, B.tr, &d.texs)) ||
      (rc = upload(r, B.pool, &d.texels)) || (rc = upload(r, B.bd, &d.bound)) || (rc = upload(r, B.cs, &d.cull_small)) ||
      (rc = upload(r, B.ct, &d.cull_tri)) || (rc = upload(r, B.cb, &d.chunk_bound)) || (rc = upload(r, B.pg, &d.pln_geo)) ||
      (rc = upload(r, B.pm, &d.pln_mat)) || (rc = upload(r, B.loc, &d.obj_loc)) || (rc = upload(r, B.bvh, &d.bvh)) ||
      (rc = upload(r, B.tt.nodes, &d.tri_bvh)) || (rc = upload(r, B.tleaf, &d.tri_leaf)) ||
      (rc = upload(r, B.tt.resid, &d.tri_resid)) || (rc = upload(r, B.aux, &d.bvh_aux)) ||
      (rc = upload(r, B.gm, &d.shadow_grid.cells)))
    return rc;
  r->dev = d;
  if ((rc = upload_update_tables(r, B)) != RFX_OK) return rc;
  r->accel = B.accel;
  r->order_box = B.order_box;
  r->dev = d;
  r->has_scene = true;
  ++r->scene_gen;
  r->prim_key.clear();
  r->prim_seen.clear();
  return RFX_OK;
}

extern "C" int rfx_renderer_set_rng(rfx_renderer *r, uint32_t sphere_seed, uint32_t jitter_seed)
{
  if (!r) return fail(RFX_ERR_ARG, "set_rng: null renderer");
  int rc;
  if ((rc = set_dev(r)) != RFX_OK) return rc;
  HIP_CHECK(hipMemcpyAsync(r->rng.cur(), &sphere_seed, sizeof(uint32_t), hipMemcpyHostToDevice, r->stream));
  HIP_CHECK(hipStreamSynchronize(r->stream));
  r->jitter_seed = jitter_seed;
  r->rng.rewind_ok = false;
  r->rng.reset(false);
  return RFX_OK;
}

extern "C" int rfx_renderer_get_rng(rfx_renderer *r, uint32_t *sphere_seed, uint32_t *jitter_seed)
{
  if (!r) return fail(RFX_ERR_ARG, "get_rng: null renderer");
  int rc;
  if ((rc = set_dev(r)) != RFX_OK) return rc;
  uint32_t s = 0;
  int err = 0;
  HIP_CHECK(hipMemcpyAsync(&s, r->rng.cur(), sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
  HIP_CHECK(hipMemcpyAsync(&err, r->err, sizeof(int), hipMemcpyDeviceToHost, r->stream));
  HIP_CHECK(hipStreamSynchronize(r->stream));
  if (err & 1) return fail(RFX_ERR_RNG, "RNG pre-pass ran short of accepted triples");  // (bit 4: an exact fallback)
  if (sphere_seed) *sphere_seed = s;
  if (jitter_seed) *jitter_seed = r->jitter_seed;
  return RFX_OK;
}

// RNG blocks of a frame's traces, split into nslices equal slices (one per rank in the multi-GPU pre-pass)
static uint64_t rng_layout(uint64_t traces, uint32_t nslices, uint64_t *per_slice)
{
  if (!nslices) nslices = 1;
  const uint64_t bps = (rng_blocks_for(traces) + nslices - 1) / nslices;
  if (per_slice) *per_slice = bps;
  return bps * nslices;
}

// The pre-pass workspaces of a launch of `traces` randDirs in nblk blocks.  The per-block arrays grow together (their
// sizes follow nblk); a grown set gets a fresh jump table and cleared status words.  blk_cnt's capacity is the number
// of blocks the whole set is ready for: it is released before the first of the others is touched and reserved after
// the last step, so after a grow that failed part-way it is 0 and the next call, whatever its size, starts over.
static int ensure_rng_workspace(rfx_renderer *r, uint64_t traces, uint64_t nblk)
{
  int rc;
  if ((rc = r->rd.reserve(traces)) < 0) return rc;
  if (nblk <= r->blk_cnt.cap) return RFX_OK;
  r->blk_cnt.release();
  if ((rc = r->rng_status.reserve(nblk)) < 0 || (rc = r->blk_off.reserve(nblk)) < 0 ||
      (rc = r->tile_sum.reserve(nblk / 4096 + 1)) < 0 || (rc = r->rng_range.reserve(4)) < 0 ||
      (rc = r->rng_masks.reserve(nblk * 256)) < 0 || (rc = r->jump.reserve(2 * (256 + nblk))) < 0)
    return rc;
  HIP_CHECK(hipMemset(r->rng_status, 0, nblk * sizeof(unsigned long long)));  // epoch 0: no launch's
  r->rng_epoch = 0;
  if ((rc = r->rng_ticket.reserve(1)) < 0) return rc;
  if (rc) HIP_CHECK(hipMemset(r->rng_ticket, 0, sizeof(unsigned long long)));
  std::vector<uint32_t> jump(2 * (256 + nblk));
  rng_jump_table(nblk, jump.data());
  HIP_CHECK(hipMemcpy(r->jump, jump.data(), jump.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  return (rc = r->blk_cnt.reserve(nblk)) < 0 ? rc : RFX_OK;
}

// Whole pre-pass on one device: every block counted here (the 1-GPU path, and the redundant form of the
// multi-GPU one).  Sphere stream: the current seed word -> pre-pass -> the other word, which becomes current.
static int enqueue_rng(rfx_renderer *r, uint64_t traces, hipStream_t st)
{
  int rc;
  const uint64_t nblk = rng_layout(traces, 1, nullptr);
  if ((rc = ensure_rng_workspace(r, traces, nblk)) != RFX_OK) return rc;
  HIP_CHECK(launch_rng_count(r->rng.cur(), r->jump, r->blk_cnt, 0, nblk, r->rng_masks, st));
  HIP_CHECK(launch_rng_finish(r->rng.cur(), r->jump, r->rng.next(), r->blk_cnt, r->rng_masks, nblk, traces,
                              r->rd, r->err, 1, 1, 1, 0, 1, st));
  r->rng.moved(0);
  r->rng.rewind_ok = false;  // (every other pre-pass runs behind plan_frame, which clears it)
  return RFX_OK;
}

// Validate a frame and build its kernel parameters (everything but the output pointers).
struct FramePlan {
  FrameParams P;
  uint64_t traces = 0;
  hipStream_t st = nullptr;
  // band partition (rfx.h: nranks > 1, row_block 0): the emit writes the randDirs of traces [band_lo, band_hi) only,
  // into a buffer of the band's size (its base pointer offset by band_lo)
  bool band = false;
  uint64_t band_lo = 0, band_hi = UINT64_MAX;
  // one span of a split frame (rfx_render_frame): launches on two streams overlap, so the per-renderer state of
  // single launches (tile schedule, per-view masks, regroup queue) stays out
  bool split = false;
  int split_side = 0;  // the span's stream (0: the caller's, 1: the renderer's second)
  uint64_t rd_traces() const { return band ? band_hi - band_lo : traces; }  // randDir words the plan writes and reads
};

static int plan_frame(rfx_renderer *r, const rfx_frame *f, void *stream, FramePlan &plan)
{
  if (!r || !f) return fail(RFX_ERR_ARG, "render_frame: bad args");
  if (!r->has_scene) return fail(RFX_ERR_STATE, "render_frame: no scene uploaded");
  r->rng.rewind_ok = false;  // every render path moves on from the last rfx_render_frame
  if (!f->width || !f->height || f->reflect_num <= 0 || f->sample_num == 0)
    return fail(RFX_ERR_ARG, "render_frame: W=%u H=%u reflect_num=%d sample_num=%d", f->width, f->height,
                f->reflect_num, f->sample_num);
  const uint32_t nranks = f->nranks ? f->nranks : 1;
  const bool band = nranks > 1 && !f->row_block;  // band partition: this rank's rows [pixel_begin, pixel_end) / W
  if (nranks > 1 && (f->sample_num < 0 || f->rank >= nranks))
    return fail(RFX_ERR_ARG, "render_frame: a partition needs sample_num > 0, rank < nranks");
  if (f->sample_num > 256 || f->sample_num < -4096) return fail(RFX_ERR_ARG, "render_frame: sample_num out of range");
  int rc;
  if ((rc = set_dev(r)) != RFX_OK) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : r->stream;

  const uint32_t W = f->width, H = f->height;
  const uint64_t npx = (uint64_t)W * H;
  uint64_t p0 = f->pixel_begin, p1 = f->pixel_end;
  if (band)
  {
    // the band's rows; the random stream and the trace indices run over the span [span_begin, span_end) of whole rows
    // (the whole W x H frame by default), output rows stay the frame's
    const uint64_t s0 = f->span_begin, s1 = (f->span_begin == 0 && f->span_end == 0) ? npx : f->span_end;
    if (p0 >= p1 || p1 > npx || p0 % W || p1 % W)
      return fail(RFX_ERR_ARG, "render_frame: a band is whole rows [pixel_begin, pixel_end) / W of the frame");
    if (s0 >= s1 || s1 > npx || s0 % W || s1 % W || p0 < s0 || p1 > s1)
      return fail(RFX_ERR_ARG, "render_frame: a band's span is whole rows [span_begin, span_end) / W around the band");
    plan.band = true;
    plan.band_lo = (p0 - s0) * (uint64_t)(f->sample_num * f->sample_num);
    plan.band_hi = (p1 - s0) * (uint64_t)(f->sample_num * f->sample_num);
    p0 = s0;
    p1 = s1;
  }
  if (p0 == 0 && p1 == 0) p1 = npx;
  if (p0 >= p1 || p1 > npx) return fail(RFX_ERR_ARG, "render_frame: pixel span [%llu, %llu) outside frame",
                                        (unsigned long long)p0, (unsigned long long)p1);
  if (nranks > 1 && !band && (p0 != 0 || p1 != npx)) return fail(RFX_ERR_ARG, "render_frame: strips need the whole frame");
  const uint32_t y0 = (uint32_t)(p0 / W), y1 = (uint32_t)((p1 - 1) / W);
  uint64_t traces, trace_base = 0;
  uint32_t grid_rows, row0;
  if (f->sample_num < 0)
  {
    // block preview: corners (x % n == 0 && y % n == 0) inside the span, in raster order (Render.cpp:158-172)
    const uint64_t n = (uint64_t)(-f->sample_num);
    const uint64_t bw = (W + n - 1) / n;
    auto corners_before = [&](uint64_t p) -> uint64_t {
      const uint64_t y = p / W, x = p % W;
      return (y + n - 1) / n * bw + (y % n == 0 ? (x + n - 1) / n : 0);
    };
    trace_base = corners_before(p0);
    traces = corners_before(p1) - trace_base;
    row0 = (uint32_t)(y0 / n);
    grid_rows = (uint32_t)(y1 / n - y0 / n + 1);
  }
  else
  {
    traces = (p1 - p0) * (uint64_t)(f->sample_num * f->sample_num);
    row0 = nranks > 1 ? 0 : y0;
    grid_rows = nranks > 1 ? rfx_strip_rows(H, f->row_block, f->rank, nranks) : y1 - y0 + 1;
    if (band)
    {
      row0 = (uint32_t)(f->pixel_begin / W);
      grid_rows = (uint32_t)((f->pixel_end - f->pixel_begin) / W);
    }
  }
  // one launch (rfx_render_frame splits larger spans before planning them; a band's span must stay within this)
  if (traces > kMaxLaunchTraces)
    return fail(RFX_ERR_ARG, "render_frame: %llu traces in one launch exceed 2^31 (partitions: a smaller span)",
                (unsigned long long)traces);
  plan.traces = traces;
  plan.st = st;
  FrameParams &P = plan.P;
  P = FrameParams{};
  P.eye_x = f->eye[0]; P.eye_y = f->eye[1]; P.eye_z = f->eye[2];
  P.v11 = f->view[0]; P.v12 = f->view[1]; P.v13 = f->view[2];
  P.v21 = f->view[3]; P.v22 = f->view[4]; P.v23 = f->view[5];
  P.v31 = f->view[6]; P.v32 = f->view[7]; P.v33 = f->view[8];
  P.rz = rfx_camera_rz(W, f->fov);
  P.wh = W / 2.0f;
  P.hh = H / 2.0f;
  P.W = W; P.H = H;
  P.depth = f->reflect_num;
  P.ss = f->sample_num;
  P.accumulate = f->sample_num > 0 && f->additive_counter > 1;
  P.additive = f->sample_num > 0 && f->additive;
  P.jitter_seed = r->jitter_seed;
  P.row_block = f->row_block ? f->row_block : 1;
  P.rank = nranks > 1 && !band ? f->rank : 0;
  P.nranks = band ? 1 : nranks;  // a band traces like a 1-GPU span of rows: absolute rows, whole-frame buffers
  P.grid_rows = grid_rows;
  P.row0 = row0;
  P.p_begin = p0;
  P.p_end = p1;
  P.trace_base = trace_base;
  return RFX_OK;
}

extern "C" int rfx_frame_rng_blocks(rfx_renderer *r, const rfx_frame *f, uint32_t nslices, uint64_t *per_slice)
{
  FramePlan pl;
  int rc;
  if ((rc = plan_frame(r, f, nullptr, pl)) != RFX_OK) return rc;
  if (!nslices || !per_slice) return fail(RFX_ERR_ARG, "frame_rng_blocks: nslices > 0 and an output required");
  rng_layout(pl.traces, nslices, per_slice);
  return RFX_OK;
}

extern "C" int rfx_frame_rng_count(rfx_renderer *r, const rfx_frame *f, uint32_t slice, uint32_t nslices,
                                   uint32_t *d_blk_counts, void *stream)
{
  FramePlan pl;
  int rc;
  if ((rc = plan_frame(r, f, stream, pl)) != RFX_OK) return rc;
  if (!d_blk_counts || !nslices || slice >= nslices) return fail(RFX_ERR_ARG, "frame_rng_count: bad slice");
  uint64_t bps = 0;
  const uint64_t nblk = rng_layout(pl.traces, nslices, &bps);
  if ((rc = ensure_rng_workspace(r, pl.rd_traces(), nblk)) != RFX_OK) return rc;
  HIP_CHECK(launch_rng_count(r->rng.cur(), r->jump, d_blk_counts, (uint64_t)slice * bps, bps, nullptr, pl.st));
  return RFX_OK;
}

// Tile schedule of a trace launch: the order sorted from the previous launch's costs when that launch had the
// same grid and mode (key), else the identity; either way this launch records its own costs.
static int tile_schedule(rfx_renderer *r, FrameParams &P, hipStream_t st, uint64_t &key, bool &record)
{
  int rc;
  const uint32_t n = trace_tiles(P);
  key = ((uint64_t)P.W << 40) ^ ((uint64_t)P.grid_rows << 16) ^ ((uint64_t)(uint32_t)P.ss << 4) ^
        (uint64_t)(P.additive * 2 + P.accumulate);
  if (!r->tile_stream)
  {
    HIP_CHECK(hipStreamCreateWithFlags(&r->tile_stream, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&r->tile_fork, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&r->tile_join, hipEventDisableTiming));
  }
  if ((rc = r->tile_scratch.reserve(tile_order_scratch() / sizeof(uint32_t))) < 0) return rc;
  if (n > r->tile_cost.cap)  // (tile_cost's capacity stands for tile_order's too: released first, reserved last)
  {
    HIP_CHECK(hipStreamSynchronize(r->tile_stream));  // a pending sort may still read the old buffers
    if (r->tile_pending) HIP_CHECK(hipEventSynchronize(r->tile_join));  // (RFX_TILE_SORT_MAIN: on the launch's stream)
    HIP_CHECK(hipStreamSynchronize(st));
    r->tile_n = 0;
    r->tile_pending = false;
    r->tile_cost.release();
    if ((rc = r->tile_order.reserve(n)) < 0 || (rc = r->tile_cost.reserve(n)) < 0) return rc;
  }
  // the last sort must have read the costs this launch may overwrite (every workgroup writes its tile's)
  // and written the order it reads
  if (r->tile_pending && r->tile_waited != st)
  {
    HIP_CHECK(hipStreamWaitEvent(st, r->tile_join, 0));
    r->tile_waited = st;
  }
  const bool same = r->tile_pending && r->tile_n == n && r->tile_key == key;
  P.tile_order = (same && r->tile_mode != 2) ? r->tile_order : nullptr;
  // record (and re-sort) every RFX_TILE_SORT_EVERY-th launch, and at once after a grid change
  record = !same || r->tile_count % RFX_TILE_SORT_EVERY == 0;
  P.tile_cost = record ? r->tile_cost : nullptr;
  ++r->tile_count;
  return RFX_OK;
}

static int no_emitted_frame(const rfx_renderer *r)
{
  if (r->emit_pending < 0) return RFX_OK;
  return fail(RFX_ERR_STATE, "render_frame: an emitted frame awaits rfx_render_frame_emitted (or rfx_frame_rng_discard)");
}

// The end of every pre-pass launch: the stream state is past the frame (RngState::moved), then the caller's event, if
// any -- the randDirs are written and the next frame's stream state is known (the next frame's RNG count may start on
// another stream while this frame traces).
static int stream_moved(rfx_renderer *r, int form, hipStream_t st, hipEvent_t emitted)
{
  r->rng.moved(form);
  if (emitted) HIP_CHECK(hipEventRecord(emitted, st));
  return RFX_OK;
}

// The randDirs of a planned frame into rd from its blocks' accept counts (the scan of the counts and the scatter).
static int emit_frame(rfx_renderer *r, FramePlan &pl, const uint32_t *d_counts, const uint16_t *d_masks, uint64_t nblk,
                      uint32_t *rd, hipEvent_t emitted)
{
  const FrameParams &P = pl.P;
  const hipStream_t st = pl.st;
  const uint64_t ss2 = P.ss > 0 ? (uint64_t)(P.ss * P.ss) : 1;
  if (pl.band)  // the band's randDirs into a buffer of the band's size: index trace - band_lo
    HIP_CHECK(launch_rng_finish_band(r->rng.cur(), r->jump, r->rng.next(), d_counts, nullptr, nblk, pl.traces,
                                     rd - pl.band_lo, r->err, pl.band_lo, pl.band_hi, r->blk_off, r->rng_range,
                                     r->tile_sum, st));
  else if (P.nranks <= 1 && nblk > RFX_SCAN_EMIT_BLOCKS)
    HIP_CHECK(launch_rng_finish_band(r->rng.cur(), r->jump, r->rng.next(), d_counts, d_masks, nblk, pl.traces, rd,
                                     r->err, 0, pl.traces, r->blk_off, r->rng_range, r->tile_sum, st));
  else
    HIP_CHECK(launch_rng_finish(r->rng.cur(), r->jump, r->rng.next(), d_counts, d_masks, nblk, pl.traces, rd,
                                r->err, ss2, P.W, P.row_block, P.rank, P.nranks, st));
  return stream_moved(r, 0, st, emitted);  // (the count / emit kernels write the next state alone: no cycle position)
}

// The whole pre-pass of a one-device launch in one kernel (rng_fused: count, look-back scan and scatter), with
// emit_frame's bookkeeping.  RFX_RNG_FUSED=0 keeps the two-kernel form (rng_count, then emit_frame).  Only where the
// cycle table is off (prepass_seq below takes every such launch by default, and measured faster at C1's 166 blocks).
// Launches of at most RFX_RNG_FUSED_MAX_BLOCKS pre-pass blocks take it.  Its block-order ticket (one atomic per
// workgroup on one word) serialises the launch's start in proportion to the blocks, so it pays only on small launches
// (interleaved A/B, frame ms, one-pass / two-kernel, profiles/r06/ab/prepass_limit_*_r6e.jsonl): 640x480 (166 blocks)
// 0.0552 / 0.0565, 960x540 (269) 0.0657 / 0.0643, 1280x720 (466) 0.0841 / 0.0803, 1920x1080 (1,013) 0.0812 / 0.0679.
static bool fused_prepass(const FramePlan &pl, uint64_t nblk)
{
  return RFX_RNG_FUSED && !pl.band && pl.P.nranks <= 1 && nblk <= (uint64_t)RFX_RNG_FUSED_MAX_BLOCKS;
}

static int prepass_fused(rfx_renderer *r, FramePlan &pl, uint64_t nblk, uint32_t *rd, hipEvent_t emitted)
{
  // 1 .. 2^28 - 1, a new tag per launch; when the tags wrap, the words earlier launches left are cleared first (a word
  // of a wider launch could otherwise carry the new tag)
  if (r->rng_epoch == (1u << 28) - 1)
  {
    HIP_CHECK(hipMemsetAsync(r->rng_status, 0, r->rng_status.cap * sizeof(unsigned long long), pl.st));
    r->rng_epoch = 0;
  }
  ++r->rng_epoch;
  HIP_CHECK(launch_rng_fused(r->rng.cur(), r->jump, r->rng.next(), nblk, pl.traces, rd, r->err, r->rng_status,
                             r->rng_ticket, r->rng_tickets, r->rng_epoch, pl.st));
  r->rng_tickets += nblk;  // every block of the launch takes one ticket
  return stream_moved(r, 2, pl.st, emitted);
}

// The pre-pass from the cycle table (rfx_kernels.hip "the cycle table"): one emit launch, after the table's one-off
// build on the first frame that takes it and, when the stream state was last set by anything but a table emit, the
// one-workgroup rng_locate.  A launch takes it when its blocks and the one for the misaligned start stay well under one
// cycle (15/16 of it: a 2^30-trace launch has half a cycle's blocks, the 2^31 limit a whole one and keeps the kernels).
static bool seq_prepass(const rfx_renderer *r, const FramePlan &pl, uint64_t nblk)
{
  return RFX_RNG_SEQ && r->rng_prepass == 1 && !pl.band && (RFX_RNG_SEQ_SPLIT || !pl.split) && pl.P.nranks <= 1 &&
         nblk >= (uint64_t)RFX_RNG_SEQ_MIN_BLOCKS && nblk + 1 <= (uint64_t)rng_seq_blocks() / 16 * 15;
}

int rfx::ensure_seq_table(rfx_renderer *r, hipStream_t st)
{
  if (r->seq_built) return RFX_OK;
  const uint32_t nb = rng_seq_blocks(), nh = rng_seq_header_words();
  std::vector<uint32_t> hdr(nh), state(nb);
  rng_seq_tables(hdr.data(), state.data());
  int rc;
  if ((rc = r->seq_hdr.reserve(nh)) < 0 || (rc = r->seq_state.reserve(nb)) < 0 || (rc = r->rng.pos.reserve(4)) < 0 ||
      (rc = r->seq_tiles.reserve((size_t)nb / 4096 + 4)) < 0 || (rc = r->seq_p.reserve((size_t)nb + 4)) < 0)
    return rc;
  HIP_CHECK(hipMemcpy(r->seq_hdr, hdr.data(), nh * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(r->seq_state, state.data(), (size_t)nb * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_CHECK(launch_rng_seq_build(r->seq_hdr, r->seq_state, r->seq_p, r->seq_tiles, st));
  HIP_CHECK(hipStreamSynchronize(st));  // once per renderer: later frames may come on any stream
  r->seq_built = true;
  r->rng.seq_valid = false;
  return RFX_OK;
}

static int prepass_seq(rfx_renderer *r, FramePlan &pl, uint64_t nblk, uint32_t *rd, hipEvent_t emitted)
{
  int rc;
  if ((rc = ensure_seq_table(r, pl.st)) != RFX_OK) return rc;
  if (!r->rng.seq_valid)
    HIP_CHECK(launch_rng_locate(r->rng.cur(), r->seq_hdr, r->seq_state, r->seq_p, r->rng.cur_pos(), pl.st));
  HIP_CHECK(launch_rng_emit_seq(r->rng.cur_pos(), r->seq_hdr, r->seq_state, r->seq_p, nblk + 1, pl.traces, rd,
                                r->rng.next(), r->rng.next_pos(), r->err, pl.st));
  return stream_moved(r, 1, pl.st, emitted);
}

// The pre-pass of a one-device launch whose every block is counted here, in the form the launch takes -- the cycle
// table, the one-pass kernel, or the count kernel and an emit that takes its accept flags instead of regenerating them
// -- then the caller's event.
static int run_prepass(rfx_renderer *r, FramePlan &pl, uint64_t nblk, uint32_t *rd, hipEvent_t emitted)
{
  if (seq_prepass(r, pl, nblk)) return prepass_seq(r, pl, nblk, rd, emitted);
  if (fused_prepass(pl, nblk)) return prepass_fused(r, pl, nblk, rd, emitted);
  HIP_CHECK(launch_rng_count(r->rng.cur(), r->jump, r->blk_cnt, 0, nblk, r->rng_masks, pl.st));
  return emit_frame(r, pl, r->blk_cnt, r->rng_masks, nblk, rd, emitted);
}

int rfx::prepass_traces(rfx_renderer *r, uint64_t n, hipStream_t st)
{
  int rc;
  if ((rc = no_emitted_frame(r)) != RFX_OK) return rc;
  r->rng.rewind_ok = false;
  FramePlan pl;  // one device, no band, not a span of a split frame: run_prepass reads nothing else of it
  pl.P = FrameParams{};
  pl.P.nranks = 1;
  pl.P.ss = 1;
  pl.P.row_block = 1;
  pl.traces = n;
  pl.st = st;
  const uint64_t nblk = rng_layout(n, 1, nullptr);
  if ((rc = ensure_rng_workspace(r, n, nblk)) != RFX_OK) return rc;
  if ((rc = run_prepass(r, pl, nblk, r->rd, nullptr)) != RFX_OK) return rc;
  r->trace_buf = 0;
  return RFX_OK;
}

// trace_frame's stages.  1: ray regrouping -- plain pixels of a large scene park their traces after park_after segments
// in the queue set up here; the bounce kernel resumes them in packed waves (rfx_parked.h bounce_kernel).
static int setup_regroup_queue(rfx_renderer *r, FramePlan &pl, int park_after, bool sort_queue)
{
  int rc;
  FrameParams &P = pl.P;
  if ((rc = r->queue.reserve(pl.traces)) < 0 || (rc = r->qkey.reserve(pl.traces)) < 0 ||
      (rc = r->qorder.reserve(pl.traces)) < 0 || (rc = r->qctr.reserve(2 + kQueueBuckets)) < 0)
    return rc;
  HIP_CHECK(hipMemsetAsync(r->qctr, 0, (sort_queue ? 2 + kQueueBuckets : 2) * sizeof(uint32_t), pl.st));
  P.queue = r->queue;
  P.queue_count = r->qctr.p;
  P.queue_next = r->qctr.p + 1;
  P.park_after = park_after;
  if (sort_queue)
  {
    P.queue_key = r->qkey;
    P.queue_order = r->qorder;
  }
  return RFX_OK;
}

// 2: primary-bundle cull masks: small scenes, plain and SSAA frames (not block previews), culling launches.  Recomputed
// only when the camera, the frame geometry, the sampling or the scene changed (the bench's frames all reuse one set)
// The chunk mode (sampleNum > 8: a wave per pixel) takes closest-hit masks only, over each pixel's sample rectangle:
// one cheap cull per pixel that every chunk of its samples reuses, so they are built for every view and every span
// of a split frame (into the span's stream side's buffer: the spans of the two streams overlap).
static int select_view_masks(rfx_renderer *r, FramePlan &pl, bool small, bool plain, bool park, bool stats)
{
  int rc;
  FrameParams &P = pl.P;
  const hipStream_t st = pl.st;
  const bool chunks = RFX_PRIM_CHUNKS && RFX_PRIM_LANES && small && trace_chunks(P);
  if (chunks && pl.split && !stats && P.grid_rows && r->prim_mode)
  {
    DevBuf<uint64_t> &mask = r->split_mask[pl.split_side];
    if ((rc = mask.reserve((size_t)trace_tiles(P) * kPrimStride)) < 0) return rc;
    HIP_CHECK(launch_prim_cull(r->dev, P, mask, r->prim_exact != 0, st));
    P.prim_mask = mask;
    P.prim_shadow = 0;
  }
  else if (small && (plain || (RFX_PRIM_LANES && (trace_lanes(P) || chunks)) || (RFX_PRIM_SSAA && P.ss >= 1)) && !park &&
           !stats && P.grid_rows && r->prim_mode && !pl.split)
  {
    struct Key { float cam[15]; uint32_t W, H, grid_rows, row0, row_block, rank, nranks; int32_t depth, ss, additive;
                 uint64_t p_begin, p_end, gen; } k;
    memset(&k, 0, sizeof(k));  // padding bytes too: the key is compared bytewise
    const float cam[15] = {P.eye_x, P.eye_y, P.eye_z, P.v11, P.v12, P.v13, P.v21, P.v22, P.v23,
                           P.v31, P.v32, P.v33, P.rz, P.wh, P.hh};
    memcpy(k.cam, cam, sizeof(cam));
    k.W = P.W; k.H = P.H; k.grid_rows = P.grid_rows; k.row0 = P.row0; k.row_block = P.row_block; k.rank = P.rank;
    k.nranks = P.nranks; k.depth = P.depth > 0 ? 1 : 0; k.p_begin = P.p_begin; k.p_end = P.p_end; k.gen = r->scene_gen;
    k.ss = P.ss; k.additive = P.additive ? 1 : 0;
    std::vector<uint8_t> kb((const uint8_t *)&k, (const uint8_t *)&k + sizeof(k));
    if ((rc = r->prim_mask.reserve((size_t)trace_tiles(P) * kPrimStride)) < 0) return rc;
    if (rc)  // a new array holds no view's masks
    {
      r->prim_key.clear();
      r->prim_seen.clear();
    }
    // a view seen for the first time renders with per-launch bundles (a camera that moves every frame never pays
    // for masks); the masks are built when the same view comes again, and kept while it stays
    if (r->prim_mode == 2 || kb != r->prim_key)
    {
      const bool repeat = kb == r->prim_seen;
      r->prim_seen = kb;
      r->prim_key.clear();
      if (repeat || r->prim_mode == 2 || chunks)
      {
        HIP_CHECK(launch_prim_cull(r->dev, P, r->prim_mask, r->prim_exact != 0, st));
        r->prim_key = kb;
        r->prim_words = (size_t)trace_tiles(P) * kPrimStride;
        r->prim_on = st;
      }
    }
    if (!r->prim_key.empty())
    {
      P.prim_mask = r->prim_mask;
      P.prim_shadow = P.additive || chunks ? 0 : 1;  // jittered frames, chunks: closest-hit masks only (prim_cull_kernel)
    }
  }
  return RFX_OK;
}

// 3: the trace launch and, for a parking one, the bounce kernel over its queue
static int launch_trace_and_bounce(rfx_renderer *r, FramePlan &pl, bool small, bool park, bool sort_queue, bool stats)
{
  const FrameParams &P = pl.P;
  const hipStream_t st = pl.st;
  if (P.grid_rows) HIP_CHECK(launch_trace(r->dev, P, stats, st));
  r->bounce_form = 0;
  if (!park) return RFX_OK;
  // packed waves over the queue, as many as the chip holds at once (RFX_BOUNCE_GROUPS_PER_CU workgroups of two waves
  // per CU: 7 waves per SIMD); a lane whose trace ends takes the next entry, so no wave waits for a slot
  const uint64_t waves = (pl.traces + 63) / 64;
  const uint32_t groups = (uint32_t)std::min<uint64_t>((waves + 1) / 2, (uint64_t)r->cus * RFX_BOUNCE_GROUPS_PER_CU);
  const int cfg = kCfgCull | (r->dev.n_light > 32 ? kCfgManyLights : 0) | (small ? kCfgSmall : 0) |
                  (r->dev.n_pln ? kCfgPlanes : 0) | (RFX_ONE_LIGHT && r->dev.n_light == 1 ? kCfgOneLight : 0) |
                  (RFX_TRI_BVH && r->dev.tri_bvh ? kCfgTriBvh : 0);
  if (sort_queue) HIP_CHECK(launch_queue_sort(r->qctr, r->qkey, r->qctr.p + 2, r->qorder, st));
  // a BVH whose nodes fit the workgroup's LDS (56 B each beside the stacks: up to ~2,100 nodes, i.e. 4,200 spheres):
  // the LDS-staged bounce kernel, one 16-wave workgroup per CU (C5 trace + bounce -4..6%, tools/ab.py); else the
  // two-wave workgroups walking the nodes in global memory
  const uint32_t lgroups = (uint32_t)std::min<uint64_t>((waves + kLdsBvhWaves - 1) / kLdsBvhWaves, (uint64_t)r->cus);
  r->bounce_form = 2;
  if (small || !lds_bvh_fits(r->dev.n_bvh) || launch_bounce_lds(cfg, lgroups, r->dev, P, st) != hipSuccess)
  {
    (void)hipGetLastError();  // an LDS launch the runtime refused: the global-memory form instead
    launch_bounce(cfg, dim3(groups), r->dev, P, st);
    r->bounce_form = 1;  // visible through rfx_renderer_bounce_form, so a silent fall-back shows in the tests
  }
  HIP_CHECK(hipGetLastError());
  return RFX_OK;
}

// 4: a recording launch's tile costs sorted into the next launch's order
static int record_tile_sort(rfx_renderer *r, const FramePlan &pl, uint64_t key)
{
  const hipStream_t st = pl.st;
  const uint32_t n = trace_tiles(pl.P);
#if RFX_TILE_SORT_MAIN
  // on the launch's own stream: no cross-stream events (tile_join only for a later launch on another stream)
  HIP_CHECK(launch_tile_order(r->tile_cost, n, r->tile_order, r->tile_scratch, st));
  HIP_CHECK(hipEventRecord(r->tile_join, st));
  r->tile_waited = st;
#else
  // beside the next frame's pre-pass
  HIP_CHECK(hipEventRecord(r->tile_fork, st));
  HIP_CHECK(hipStreamWaitEvent(r->tile_stream, r->tile_fork, 0));
  HIP_CHECK(launch_tile_order(r->tile_cost, n, r->tile_order, r->tile_scratch, r->tile_stream));
  HIP_CHECK(hipEventRecord(r->tile_join, r->tile_stream));
  r->tile_waited = nullptr;
#endif
  r->tile_pending = true;
  r->tile_n = n;
  r->tile_key = key;
  return RFX_OK;
}

// The trace launch(es) of a planned frame whose randDirs are in rd, and the end-of-frame bookkeeping.
static int trace_frame(rfx_renderer *r, FramePlan &pl, const uint32_t *rd, float *d_rgb, uint32_t *d_argb,
                       uint64_t *d_counters)
{
  int rc;
  FrameParams &P = pl.P;
  const bool stats = d_counters != nullptr;
  P.img = d_rgb;
  P.argb = d_argb;
  P.rd_state = pl.band ? rd - pl.band_lo : rd;  // a band's randDirs are stored from its first trace on (emit_frame)
  P.counters = (unsigned long long *)d_counters;
  const bool small = r->dev.n_sph <= 32 && r->dev.n_tri <= 32;
  const bool plain = P.ss == 1 && !P.additive && !P.accumulate;
  const int park_after = r->park_after < 0 ? (small ? 0 : RFX_PARK_AFTER) : r->park_after;
  const bool park = park_after > 0 && plain && !stats && P.depth > park_after && P.grid_rows && !pl.split;
  const bool sort_queue = park && r->queue_sort;
  if (park && (rc = setup_regroup_queue(r, pl, park_after, sort_queue)) != RFX_OK) return rc;
  // mode 1 schedules only launches of at least RFX_TILE_ORDER_MIN_TILES tiles: on shorter ones the sort's
  // latency (three small launches and a cross-stream wait, ~15 us) is not hidden by the RNG pre-pass
  const bool sched = P.grid_rows && r->tile_mode && !stats && P.ss >= 0 && !pl.split &&
                     (r->tile_mode != 1 || trace_tiles(P) >= RFX_TILE_ORDER_MIN_TILES);
  uint64_t key = 0;
  bool record = false;
  if (sched && (rc = tile_schedule(r, P, pl.st, key, record)) != RFX_OK) return rc;
  if ((rc = select_view_masks(r, pl, small, plain, park, stats)) != RFX_OK) return rc;
  if ((rc = launch_trace_and_bounce(r, pl, small, park, sort_queue, stats)) != RFX_OK) return rc;
  if (record && (rc = record_tile_sort(r, pl, key)) != RFX_OK) return rc;
  if ((rc = timing_event(r, pl.st)) != RFX_OK) return rc;
  if (P.additive)                                                                  // 2 draws per pixel, raster order
    r->jitter_seed = lcg_jump(r->jitter_seed, 2ull * (P.p_end - P.p_begin));
  return RFX_OK;
}

extern "C" int rfx_render_frame_counted(rfx_renderer *r, const rfx_frame *f, uint32_t nslices,
                                        const uint32_t *d_blk_counts, float *d_rgb, uint32_t *d_argb,
                                        uint64_t *d_counters, void *stream)
{
  return rfx_render_frame_counted_ev(r, f, nslices, d_blk_counts, d_rgb, d_argb, d_counters, stream, nullptr);
}

extern "C" int rfx_render_frame_counted_ev(rfx_renderer *r, const rfx_frame *f, uint32_t nslices,
                                           const uint32_t *d_blk_counts, float *d_rgb, uint32_t *d_argb,
                                           uint64_t *d_counters, void *stream, void *emitted_event)
{
  FramePlan pl;
  int rc;
  if ((rc = plan_frame(r, f, stream, pl)) != RFX_OK) return rc;
  if (!d_rgb || !d_blk_counts || !nslices) return fail(RFX_ERR_ARG, "render_frame_counted: bad args");
  if (pl.traces == 0) return RFX_OK;
  const uint64_t nblk = rng_layout(pl.traces, nslices, nullptr);
  if ((rc = ensure_rng_workspace(r, pl.rd_traces(), nblk)) != RFX_OK) return rc;
  if ((rc = timing_start(r, pl.st)) != RFX_OK || (rc = no_emitted_frame(r)) != RFX_OK ||
      (rc = emit_frame(r, pl, d_blk_counts, nullptr, nblk, r->rd, (hipEvent_t)emitted_event)) != RFX_OK)
    return rc;
  r->trace_buf = 0;
  if ((rc = timing_event(r, pl.st)) != RFX_OK) return rc;
  return trace_frame(r, pl, r->rd, d_rgb, d_argb, d_counters);
}

// What an emitted frame's randDirs depend on: the traces and their band, and the frame geometry that maps pixels to
// trace indices.  rfx_render_frame_emitted refuses a frame whose plan differs (its rows' randDirs were never written).
static void plan_key(const FramePlan &pl, uint64_t key[10])
{
  const FrameParams &P = pl.P;
  key[0] = pl.traces;
  key[1] = pl.band_lo;
  key[2] = pl.band_hi;
  key[3] = ((uint64_t)P.W << 32) | P.H;
  key[4] = ((uint64_t)(uint32_t)P.ss << 32) | P.row_block;
  key[5] = ((uint64_t)P.rank << 32) | P.nranks;
  key[6] = ((uint64_t)P.row0 << 32) | P.grid_rows;
  key[7] = P.p_begin;  // the span and its first trace index in words of their own: no two spans share a key
  key[8] = P.p_end;
  key[9] = P.trace_base;
}

// Emit-ahead (multi-GPU): the emit of frame i + 1 on a side stream while frame i traces.  Two randDir buffers: an emit
// writes the one the last enqueued trace does not read, and the next rfx_render_frame_emitted traces from it.
extern "C" int rfx_frame_rng_emit(rfx_renderer *r, const rfx_frame *f, uint32_t nslices, const uint32_t *d_blk_counts,
                                  void *stream, void *emitted_event)
{
  FramePlan pl;
  int rc;
  if ((rc = plan_frame(r, f, stream, pl)) != RFX_OK) return rc;
  if (!d_blk_counts || !nslices) return fail(RFX_ERR_ARG, "frame_rng_emit: bad args");
  if (r->emit_pending >= 0) return fail(RFX_ERR_STATE, "frame_rng_emit: the last emitted frame has not been traced");
  if (pl.traces == 0) return RFX_OK;
  const uint64_t nblk = rng_layout(pl.traces, nslices, nullptr);
  if ((rc = ensure_rng_workspace(r, pl.rd_traces(), nblk)) != RFX_OK) return rc;
  if ((rc = r->rd_alt.reserve(pl.rd_traces())) < 0) return rc;
  const int buf = r->trace_buf == 0 ? 1 : 0;  // not the buffer of the last enqueued trace
  // nor one a split frame's spans on the renderer's second stream may still read (the emit may run on a third stream)
  if (buf == 1 && r->split_alt_busy) HIP_CHECK(hipStreamWaitEvent(pl.st, r->split_ev[2], 0));
  r->split_alt_busy = false;
  if ((rc = emit_frame(r, pl, d_blk_counts, nullptr, nblk, buf ? r->rd_alt : r->rd,
                       (hipEvent_t)emitted_event)) != RFX_OK)
    return rc;
  r->emit_pending = buf;
  plan_key(pl, r->emit_key);
  return RFX_OK;
}

extern "C" int rfx_render_frame_emitted(rfx_renderer *r, const rfx_frame *f, float *d_rgb, uint32_t *d_argb,
                                        uint64_t *d_counters, void *stream)
{
  FramePlan pl;
  int rc;
  if ((rc = plan_frame(r, f, stream, pl)) != RFX_OK) return rc;
  if (!d_rgb) return fail(RFX_ERR_ARG, "render_frame_emitted: null framebuffer");
  if (pl.traces == 0) return RFX_OK;
  if (r->emit_pending < 0) return fail(RFX_ERR_STATE, "render_frame_emitted: no emitted frame (rfx_frame_rng_emit)");
  uint64_t key[10];
  plan_key(pl, key);
  if (memcmp(key, r->emit_key, sizeof(key)) != 0)
    return fail(RFX_ERR_STATE, "render_frame_emitted: the frame differs from the emitted one (band, geometry or traces); "
                               "rfx_frame_rng_discard it first");
  const int buf = r->emit_pending;
  r->emit_pending = -1;
  r->trace_buf = buf;
  if ((rc = timing_start(r, pl.st)) != RFX_OK) return rc;  // (the emit ran on its own stream: no pre-pass time)
  if ((rc = timing_event(r, pl.st)) != RFX_OK) return rc;
  return trace_frame(r, pl, buf ? r->rd_alt : r->rd, d_rgb, d_argb, d_counters);
}

// Forget an emitted, untraced frame: the stream state returns to before it (the emit read one state word and wrote
// the other, so flipping back restores it).
extern "C" int rfx_frame_rng_discard(rfx_renderer *r)
{
  if (!r) return fail(RFX_ERR_ARG, "frame_rng_discard: null renderer");
  r->rng.rewind_ok = false;
  r->rng.seq_valid = false;
  if (r->emit_pending >= 0) r->rng.reset(true);
  r->emit_pending = -1;
  return RFX_OK;
}

extern "C" int rfx_frame_rng_pending(rfx_renderer *r, uint32_t *frame_start)
{
  if (!r || !frame_start) return fail(RFX_ERR_ARG, "frame_rng_pending: bad args");
  int rc;
  if ((rc = set_dev(r)) != RFX_OK) return rc;
  // an emitted frame read the state word it left behind (its emit made the other one current)
  const uint32_t *w = r->emit_pending >= 0 ? r->rng.next() : r->rng.cur();
  HIP_CHECK(hipMemcpyAsync(frame_start, w, sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
  HIP_CHECK(hipStreamSynchronize(r->stream));
  return r->emit_pending >= 0 ? 1 : 0;
}

// The stream state a frame of several launches starts from, kept in seed[2] for rfx_frame_rng_rewind (the seed words
// ping-pong once per launch, so flipping back would restore only the last span's start).
int rfx::save_rewind_state(rfx_renderer *r, hipStream_t st)
{
  HIP_CHECK(hipMemcpyAsync(r->rng.seed.p + 2, r->rng.cur(), sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  return RFX_OK;
}

// Pixel spans [p0, p1) of more than r->launch_traces traces: launches of at most that many traces each, whole rows where
// a row fits.  Span k runs on the caller's stream (k even) or the renderer's split stream (k odd) with its randDirs in
// rd / rd_alt; its pre-pass waits for span k - 1's emit, whose end state it starts from, so span k's trace overlaps
// span k - 1's tail.  Every span is a cursor span of the reference's loop: trace indices and the additive jitter run
// from the span's first pixel (Render.cpp:136-215), so the pixels and both streams equal one launch over [p0, p1).
static int render_split(rfx_renderer *r, const rfx_frame *f, uint64_t p0, uint64_t p1, float *d_rgb, uint32_t *d_argb,
                        uint64_t *d_counters, void *stream)
{
  int rc;
  if ((rc = set_dev(r)) != RFX_OK || (rc = no_emitted_frame(r)) != RFX_OK) return rc;
  const uint64_t W = f->width, spp = (uint64_t)(f->sample_num * f->sample_num);
  uint64_t per = std::max<uint64_t>(1, r->launch_traces / spp);  // pixels per launch
  const bool rows = per >= W;
  if (rows) per = per / W * W;
  const uint64_t cap = per * spp;
  if (!r->split_stream) HIP_CHECK(hipStreamCreateWithFlags(&r->split_stream, hipStreamNonBlocking));
  for (hipEvent_t &e : r->split_ev)
    if (!e) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  const hipStream_t s2[2] = {stream ? (hipStream_t)stream : r->stream, r->split_stream};
  // workspaces for the largest span before any launch (no re-allocation while spans are in flight)
  if ((rc = ensure_rng_workspace(r, cap, rng_layout(cap, 1, nullptr))) != RFX_OK) return rc;
  if ((rc = r->rd_alt.reserve(cap)) < 0) return rc;
  const uint32_t jitter0 = r->jitter_seed;
  if ((rc = save_rewind_state(r, s2[0])) != RFX_OK) return rc;
  // the split stream starts after the caller's earlier work (its first span also waits for span 0's emit)
  HIP_CHECK(hipEventRecord(r->split_ev[2], s2[0]));
  HIP_CHECK(hipStreamWaitEvent(s2[1], r->split_ev[2], 0));
  uint64_t k = 0;
  for (uint64_t a = p0; a < p1; ++k)
  {
    const uint64_t b = std::min(p1, rows ? (a / W) * W + per : a + per);
    rfx_frame fk = *f;
    fk.pixel_begin = a;
    fk.pixel_end = b;
    const int side = RFX_SPLIT_STREAMS > 1 ? (int)(k & 1) : 0;
    FramePlan pl;
    if ((rc = plan_frame(r, &fk, s2[side], pl)) != RFX_OK) return rc;
    pl.split = true;
    pl.split_side = side;
    const uint64_t nblk = rng_layout(pl.traces, 1, nullptr);
    if (k > 0) HIP_CHECK(hipStreamWaitEvent(s2[side], r->split_ev[side ^ 1], 0));  // span k - 1's end state
    if ((rc = timing_start(r, pl.st)) != RFX_OK) return rc;
    uint32_t *rd = side ? r->rd_alt : r->rd;
    // (the cycle table: from the (seed, k, A) the last span's emit wrote)
    if ((rc = run_prepass(r, pl, nblk, rd, r->split_ev[side])) != RFX_OK) return rc;
    if ((rc = timing_event(r, pl.st)) != RFX_OK) return rc;
    if ((rc = trace_frame(r, pl, rd, d_rgb, d_argb, d_counters)) != RFX_OK) return rc;
    a = b;
  }
  // the caller's stream continues after every span
  if (k > 1)
  {
    HIP_CHECK(hipEventRecord(r->split_ev[2], s2[1]));
    HIP_CHECK(hipStreamWaitEvent(s2[0], r->split_ev[2], 0));
  }
  r->trace_buf = 0;            // the last span on the caller's stream read rd; the odd spans read rd_alt until
  r->split_alt_busy = k > 1;   // split_ev[2], which the next emit-ahead into rd_alt waits for
  r->rng.rewindable_saved(jitter0, s2[0]);
  return RFX_OK;
}

extern "C" int rfx_render_frame(rfx_renderer *r, const rfx_frame *f, float *d_rgb, uint32_t *d_argb,
                                uint64_t *d_counters, void *stream)
{
  FramePlan pl;
  int rc;
  if (!d_rgb) return fail(RFX_ERR_ARG, "render_frame: null framebuffer");
  if (r && f && f->sample_num > 0 && f->sample_num <= 256 && f->nranks <= 1 && f->width && f->height)
  {
    // a span of more traces than one launch takes: consecutive pixel spans (Render.cpp:136-215 walks the same cursor)
    const uint64_t npx = (uint64_t)f->width * f->height;
    const uint64_t p0 = f->pixel_begin, p1 = (f->pixel_begin == 0 && f->pixel_end == 0) ? npx : f->pixel_end;
    if (p0 < p1 && p1 <= npx && (p1 - p0) * (uint64_t)(f->sample_num * f->sample_num) > r->launch_traces)
      return render_split(r, f, p0, p1, d_rgb, d_argb, d_counters, stream);
  }
  if ((rc = plan_frame(r, f, stream, pl)) != RFX_OK) return rc;
  const uint32_t jitter0 = r->jitter_seed;
  if (pl.traces == 0)  // a span with no block corner traces nothing (and draws no randDir)
  {
    r->rng.rewindable(jitter0, false);
    return RFX_OK;
  }
  const uint64_t nblk = rng_layout(pl.traces, 1, nullptr);
  if ((rc = ensure_rng_workspace(r, pl.traces, nblk)) != RFX_OK) return rc;
  if ((rc = timing_start(r, pl.st)) != RFX_OK) return rc;
  if ((rc = no_emitted_frame(r)) != RFX_OK || (rc = run_prepass(r, pl, nblk, r->rd, nullptr)) != RFX_OK) return rc;
  r->trace_buf = 0;
  if ((rc = timing_event(r, pl.st)) != RFX_OK) return rc;
  if ((rc = trace_frame(r, pl, r->rd, d_rgb, d_argb, d_counters)) != RFX_OK) return rc;
  r->rng.rewindable(jitter0, true);
  return RFX_OK;
}

// Undo the random-stream advance of the last rfx_render_frame (its pixels stay as written): the pre-pass read the
// frame's start state from one seed word and wrote the end state to the other, so flipping back restores the start
// (a frame of several launches: its start state is copied back from seed[2]).
extern "C" int rfx_frame_rng_rewind(rfx_renderer *r)
{
  if (!r) return fail(RFX_ERR_ARG, "frame_rng_rewind: null renderer");
  if (!r->rng.rewind_ok) return fail(RFX_ERR_STATE, "frame_rng_rewind: the last call was not rfx_render_frame");
  r->rng.reset(r->rng.rewind_flip);
  if (r->rng.rewind_saved)
  {
    int rc;
    if ((rc = set_dev(r)) != RFX_OK) return rc;
    HIP_CHECK(hipMemcpyAsync(r->rng.cur(), r->rng.seed.p + 2, sizeof(uint32_t), hipMemcpyDeviceToDevice, r->rng.rewind_stream));
    ++r->rng.state_seq;
  }
  r->jitter_seed = r->rng.rewind_jitter;
  r->rng.rewind_ok = false;
  r->rng.rewind_saved = false;
  return RFX_OK;
}

extern "C" int rfx_device_alloc(rfx_renderer *r, size_t bytes, void **p)
{
  if (!r || !p) return fail(RFX_ERR_ARG, "device_alloc: bad args");
  int rc;
  if ((rc = set_dev(r)) != RFX_OK) return rc;
  HIP_CHECK(hipMalloc(p, bytes ? bytes : 1));
  return RFX_OK;
}

extern "C" int rfx_device_free(rfx_renderer *r, void *p)
{
  if (!r) return fail(RFX_ERR_ARG, "device_free: null renderer");
  int rc;
  if ((rc = set_dev(r)) != RFX_OK) return rc;
  HIP_CHECK(hipFree(p));
  return RFX_OK;
}

extern "C" int rfx_memcpy_d2h(rfx_renderer *r, void *dst, const void *src, size_t n)
{
  if (!r) return fail(RFX_ERR_ARG, "memcpy: null renderer");
  HIP_CHECK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, r->stream));
  HIP_CHECK(hipStreamSynchronize(r->stream));
  return RFX_OK;
}

extern "C" int rfx_memcpy_d2d(rfx_renderer *r, void *dst, const void *src, size_t n)
{
  if (!r || (n && (!dst || !src))) return fail(RFX_ERR_ARG, "memcpy_d2d: bad args");
  int rc;
  if ((rc = set_dev(r)) != RFX_OK) return rc;
  if (n) HIP_CHECK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, r->stream));
  return RFX_OK;
}

extern "C" int rfx_memcpy_h2d(rfx_renderer *r, void *dst, const void *src, size_t n)
{
  if (!r) return fail(RFX_ERR_ARG, "memcpy: null renderer");
  HIP_CHECK(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, r->stream));
  HIP_CHECK(hipStreamSynchronize(r->stream));
  return RFX_OK;
}

extern "C" int rfx_synchronize(rfx_renderer *r)
{
  if (!r) return fail(RFX_ERR_ARG, "synchronize: null renderer");
  HIP_CHECK(hipStreamSynchronize(r->stream));
  int err = 0;
  HIP_CHECK(hipMemcpy(&err, r->err, sizeof(int), hipMemcpyDeviceToHost));
  if (err & 1) return fail(RFX_ERR_RNG, "RNG pre-pass ran short of accepted triples");  // (bit 4: an exact fallback)
  return RFX_OK;
}

extern "C" int rfx_render_frame_host(rfx_renderer *r, const rfx_frame *f, float *rgb, uint32_t *argb_out,
                                     uint64_t *counters)
{
  if (!r || !f || !rgb) return fail(RFX_ERR_ARG, "render_frame_host: bad args");
  if (f->nranks > 1) return fail(RFX_ERR_ARG, "render_frame_host: whole frames only");
  int rc;
  if ((rc = set_dev(r)) != RFX_OK) return rc;
  const size_t px = (size_t)f->width * f->height;
  if ((rc = r->img.reserve(px * 3)) < 0 || (rc = r->argb.reserve(px)) < 0 || (rc = r->cnt.reserve(RFX_NCOUNTERS)) < 0)
    return rc;
  HIP_CHECK(hipMemcpyAsync(r->img, rgb, px * 3 * sizeof(float), hipMemcpyHostToDevice, r->stream));
  if (counters) HIP_CHECK(hipMemsetAsync(r->cnt, 0, RFX_NCOUNTERS * sizeof(uint64_t), r->stream));
  if ((rc = rfx_render_frame(r, f, r->img, argb_out ? r->argb : nullptr, counters ? r->cnt : nullptr, nullptr)))
    return rc;
  HIP_CHECK(hipMemcpyAsync(rgb, r->img, px * 3 * sizeof(float), hipMemcpyDeviceToHost, r->stream));
  if (argb_out) HIP_CHECK(hipMemcpyAsync(argb_out, r->argb, px * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
  if (counters)
  {
    uint64_t c[RFX_NCOUNTERS];
    HIP_CHECK(hipMemcpyAsync(c, r->cnt, sizeof(c), hipMemcpyDeviceToHost, r->stream));
    HIP_CHECK(hipStreamSynchronize(r->stream));
    for (int k = 0; k < RFX_NCOUNTERS; ++k) counters[k] += c[k];
  }
  return rfx_synchronize(r);
}

extern "C" int rfx_rand_dirs(rfx_renderer *r, uint32_t seed, uint64_t n, float *out3, uint32_t *seed_out)
{
  if (!r || !out3 || !n) return fail(RFX_ERR_ARG, "rand_dirs: bad args");
  int rc;
  if ((rc = set_dev(r)) != RFX_OK) return rc;
  uint32_t saved = 0;
  HIP_CHECK(hipMemcpyAsync(&saved, r->rng.cur(), sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
  HIP_CHECK(hipStreamSynchronize(r->stream));
  HIP_CHECK(hipMemcpyAsync(r->rng.cur(), &seed, sizeof(uint32_t), hipMemcpyHostToDevice, r->stream));
  if ((rc = enqueue_rng(r, n, r->stream)) != RFX_OK) return rc;
  std::vector<uint32_t> states(n);
  HIP_CHECK(hipMemcpyAsync(states.data(), r->rd, n * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
  uint32_t after = 0;
  HIP_CHECK(hipMemcpyAsync(&after, r->rng.cur(), sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));  // flipped
  HIP_CHECK(hipMemcpyAsync(r->rng.cur(), &saved, sizeof(uint32_t), hipMemcpyHostToDevice, r->stream));
  r->rng.seq_valid = false;
  if ((rc = rfx_synchronize(r)) != RFX_OK) return rc;
  for (uint64_t i = 0; i < n; ++i)  // Vector3.cpp:182-184 from each trace's state
  {
    const uint32_t s1 = lcg_step(states[i]), s2 = lcg_step(s1), s3 = lcg_step(s2);
    out3[i * 3] = rand_component(lcg_out(s1));
    out3[i * 3 + 1] = rand_component(lcg_out(s2));
    out3[i * 3 + 2] = rand_component(lcg_out(s3));
  }
  if (seed_out) *seed_out = after;
  return RFX_OK;
}
