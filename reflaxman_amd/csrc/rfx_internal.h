// Internals of librfx shared between its HIP-side translation units (rfx_host.cpp, rfx_group.cpp, rfx_kat.cpp); not
// part of the C-ABI.  The host-only part (rfx::fail, SceneBuild) is rfx_scene.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "rfx_launch.h"
#include "rfx_refit.h"
#include "rfx_scene.h"

#define HIP_CHECK(expr)                                                                          \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess) return rfx::fail(RFX_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
#define RCHECK(expr)               \
  do {                             \
    int rc_ = (expr);              \
    if (rc_ != RFX_OK) return rc_; \
  } while (0)

namespace rfx {

// A device array the renderer owns, freed with it (on the device current at destruction: rfx_renderer_destroy sets
// it).  Grow-only: reserve(n) keeps an array of at least n elements, else frees it and allocates n -- the contents are
// not carried over.  Returns 1 when it allocated (the caller re-initialises what the array held), 0 when the array
// stays, an RFX_ERR_* (< 0) when the allocation failed (the array is then empty: capacity 0).  Where several arrays grow
// as a set behind one array's capacity, release() that array before the first of the others is touched and reserve it
// last: its capacity is then non-zero only while the whole set is allocated and initialised.
template <class T>
struct DevBuf {
  T *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  void release()
  {
    (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  int reserve(size_t n)
  {
    if (n <= cap) return 0;
    release();
    HIP_CHECK(hipMalloc(&p, n * sizeof(T)));
    cap = n;
    return 1;
  }
  operator T *() const { return p; }
};

// The sphere stream's state (the reference's serial LCG, trace_math.h:34-39) and what follows it around.  seed[idx] is
// the current state; a pre-pass reads it and writes the state after its frame to the other word, and moved() makes
// that one current (no device copy between frames).  seed[2]: the start state of a frame of several launches.  pos:
// the state's place in the LCG's cycle, (k, A) beside each of the two seed words (rfx_kernels.hip "the cycle table");
// seq_valid: the pair beside the current word matches that word (a table emit wrote both) -- anything else that sets
// or moves the stream clears it, and the next table emit runs rng_locate first.
struct RngState {
  DevBuf<uint32_t> seed, pos;
  uint32_t idx = 0;
  bool seq_valid = false;
  int prepass_form = 0;  // rfx_renderer_prepass_form: the last pre-pass (0 count + emit, 1 cycle table, 2 one pass)
  // bumped whenever the random streams move or are set (emits, set_rng, rewinds): a device group compares it with the
  // value after its own last frame to know whether the members' streams still equal member 0's
  uint64_t state_seq = 0;
  // rfx_frame_rng_rewind: the last call was an rfx_render_frame; its start states (the sphere stream's is the other
  // seed word while rewind_flip, or seed[2] on rewind_stream while rewind_saved) can be restored
  bool rewind_ok = false, rewind_flip = false, rewind_saved = false;
  uint32_t rewind_jitter = 0;
  hipStream_t rewind_stream = nullptr;

  uint32_t *cur() const { return seed.p + idx; }
  uint32_t *next() const { return seed.p + (idx ^ 1u); }
  uint32_t *cur_pos() const { return pos.p + 2 * idx; }
  uint32_t *next_pos() const { return pos.p + 2 * (idx ^ 1u); }
  // a pre-pass of `form` wrote next() (form 1: next_pos() too)
  void moved(int form)
  {
    idx ^= 1u;
    seq_valid = form == 1;
    prepass_form = form;
    ++state_seq;
  }
  // cur() is about to be written from outside (no pre-pass): its cycle position is unknown
  uint32_t *cur_for_write()
  {
    seq_valid = false;
    return cur();
  }
  // the stream was set from outside, or stepped back one pre-pass (flip: the other word becomes current again)
  void reset(bool flip)
  {
    if (flip) idx ^= 1u;
    seq_valid = false;
    ++state_seq;
  }
  // the call that ends here can be undone by rfx_frame_rng_rewind: by flipping back (flip), or not at all moved
  void rewindable(uint32_t jitter0, bool flip)
  {
    rewind_ok = true;
    rewind_flip = flip;
    rewind_saved = false;
    rewind_jitter = jitter0;
  }
  // ... a frame of several launches: from seed[2] (save_rewind_state before the first), copied back on st
  void rewindable_saved(uint32_t jitter0, hipStream_t st)
  {
    rewindable(jitter0, false);
    rewind_saved = true;
    rewind_stream = st;
  }
};

}  // namespace rfx

struct rfx_renderer {
  rfx_renderer();  // rfx_host.cpp: the defaults its compile-time knobs set
  int device = 0;
  int cus = 256;  // compute units of the device (the bounce kernel's grid: one resident wave per slot)
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  // scene on device
  rfx::DevScene dev{};
  std::vector<void *> scene_allocs;
  bool has_scene = false;
  rfx::RngState rng;
  rfx::DevBuf<int> err;  // the pre-pass kernels' error word (rfx_synchronize)
  uint32_t jitter_seed = 0;
  // workspaces
  rfx::DevBuf<uint32_t> rd;      // per-trace LCG states (rng_emit)
  rfx::DevBuf<uint32_t> rd_alt;  // emit-ahead, the odd spans of a split frame: the second randDir buffer
  int emit_pending = -1;  // emit-ahead: buffer (0 rd, 1 rd_alt) of an emitted, untraced frame, or -1
  int trace_buf = 0;      // buffer the last enqueued trace read
  bool split_alt_busy = false;  // a split frame's odd spans traced from rd_alt on split_stream (done at split_ev[2])
  uint64_t emit_key[10] = {};  // the emitted frame's plan (traces, band, geometry): rfx_render_frame_emitted must match it
  // frames of more traces than launch_traces: consecutive spans alternate between the caller's stream and split_stream
  // (randDirs in rd / rd_alt); split_ev[k] marks span k's emit (the next span's pre-pass starts from its state)
  uint64_t launch_traces;
  hipStream_t split_stream = nullptr;
  hipEvent_t split_ev[3] = {nullptr, nullptr, nullptr};
  // the pre-pass's per-block arrays, sized together for blk_cnt.cap blocks (rfx_host.cpp ensure_rng_workspace): the
  // accept counts; band emits' scanned block offsets, the band's first / last / final block and the multi-workgroup
  // scan's tile totals (one per 4096 blocks); one device's accept flags per pre-pass thread (rng_count -> rng_emit);
  // the LCG jump table (rng_jump_table)
  rfx::DevBuf<uint32_t> blk_cnt, rng_range, tile_sum, jump;
  rfx::DevBuf<uint64_t> blk_off;
  rfx::DevBuf<uint16_t> rng_masks;
  // the one-pass pre-pass (rng_fused): per-block status words, the block ticket word (counts up across launches, never
  // reset), the tickets taken so far, the launch's epoch tag
  rfx::DevBuf<unsigned long long> rng_status, rng_ticket;
  unsigned long long rng_tickets = 0;
  uint32_t rng_epoch = 0;
  // the cycle table, built on the first frame that takes it (seq_built): the jump header, each block's start state,
  // the prefix of the accept counts (4 MB each) and build scratch
  rfx::DevBuf<uint32_t> seq_hdr, seq_state, seq_p, seq_tiles;
  bool seq_built = false;
  int rng_prepass;  // rfx_renderer_set_rng_prepass
  // host staging for rfx_render_frame_host
  rfx::DevBuf<float> img;
  rfx::DevBuf<uint32_t> argb;
  rfx::DevBuf<uint64_t> cnt;
  // tile schedule (rfx_renderer_set_tile_order): a recording trace launch writes per-tile clock costs; a counting
  // sort (lpt_*) turns them into the next launch's order (longest first), on the launch's stream (or, RFX_TILE_SORT_MAIN
  // = 0, on tile_stream while the next frame's RNG pre-pass runs); a launch on another stream waits on tile_join.
  // tile_n: tiles of the launch the order is for.
  int tile_mode;
  rfx::DevBuf<uint32_t> tile_cost, tile_order, tile_scratch;
  uint32_t tile_n = 0;
  uint64_t tile_key = 0;
  hipStream_t tile_stream = nullptr;
  hipEvent_t tile_fork = nullptr, tile_join = nullptr;
  bool tile_pending = false;         // a sort has been launched: its order is valid for (tile_n, tile_key)
  hipStream_t tile_waited = nullptr; // the stream that already waits on the last sort (tile_join)
  uint64_t tile_count = 0;           // scheduled launches (costs are recorded every RFX_TILE_SORT_EVERY-th)
  int park_after = -1;  // rfx_renderer_set_regroup: -1 = default (RFX_PARK_AFTER on large scenes), 0 = off
  // primary-bundle cull masks (small scenes, plain frames): kPrimStride u64 per wave tile, valid for prim_key
  rfx::DevBuf<uint64_t> prim_mask;
  // split frames in the chunk mode: each span's pixel masks, in the buffer of its stream side (render_split)
  rfx::DevBuf<uint64_t> split_mask[2];
  std::vector<uint8_t> prim_key;   // the view the masks hold (empty: none)
  std::vector<uint8_t> prim_seen;  // the view of the last plain small-scene launch
  uint64_t scene_gen = 0;  // bumped by every set_scene
  int prim_mode = 1;       // rfx_renderer_set_prim_masks
  int prim_exact = 1;      // rfx_renderer_set_prim_exact: the masks narrowed to the view's known primary hits
  size_t prim_words = 0;   // words of prim_mask that hold prim_key's masks, built on stream prim_on
  hipStream_t prim_on = nullptr;
  int tri_accel = -1;      // rfx_renderer_set_tri_accel: -1 automatic (RFX_TRI_BVH_AUTO_MIN triangles), 0 off, 1 on,
                           // 2 on with the narrow bundles walking the tree too
  rfx_accel_info accel{};  // the uploaded scene's hierarchies (rfx_renderer_accel_info)
  int bounce_form = 0;     // the last trace launch's bounce kernel: 0 none, 1 global-memory BVH, 2 LDS-staged BVH
  // ray regrouping of large-scene plain frames (RFX_PARK_AFTER): parked traces; qctr: their count, the bounce kernel's
  // claim counter, then the sort's kQueueBuckets histogram words; the regroup sort's per-entry bucket and bucket order
  rfx::DevBuf<rfx::QRay> queue;
  rfx::DevBuf<uint32_t> qctr, qkey, qorder;
  int queue_sort;  // rfx_renderer_set_regroup_sort
  // the coherent order (rfx_order.cpp): the uploaded scene's key box, and rfx_rays_order's scratch -- the ping-pong
  // keys and indices (two halves each) and the digit pass's histogram table with its totals
  rfx::OrderBox order_box{};
  rfx::DevBuf<uint32_t> order_keys, order_idx, order_table;
  // moving meshes (rfx_update.cpp; filled by set_scene for a non-small scene with triangles, upd_tris its count, else
  // 0): per triangle its current vertices, its record in tri_leaf and its class flag; the tree's leaf membership, its
  // nodes by height (upd_hoff: the heights' ends in upd_hlist) and the refit's unwidened boxes; the host form's staging
  rfx::DevBuf<float> upd_verts, upd_pos;
  rfx::DevBuf<int32_t> upd_slot, upd_order, upd_hlist;
  rfx::DevBuf<uint32_t> upd_ill, upd_idx;
  rfx::DevBuf<rfx::RefitBox> upd_lbox, upd_nbox;
  std::vector<uint32_t> upd_hoff;
  uint32_t upd_tris = 0, upd_leaves = 0;
  // re-cutting (rfx_update.cpp; filled by set_scene for a scene with a triangle tree, cut_tris its in-tree count, else
  // 0): the in-tree triangles ascending, the cut's children and by-height node list with their host-known shape, and
  // the key box's six words.  The sort's scratch (order_keys, order_idx, order_table) is reserved for cut_tris pairs at
  // set_scene, so the call allocates nothing.
  rfx::DevBuf<uint32_t> cut_in, cut_box;
  rfx::DevBuf<int32_t> cut_child, cut_hlist;
  std::vector<uint32_t> cut_hoff;
  int cut_depth = 0;
  uint32_t cut_tris = 0;
  // moving spheres (rfx_update.cpp; filled by set_scene for a non-small scene with spheres, upd_sph its count, else 0):
  // per sphere of the insertion order its device index; per 64-sphere chunk the update's dirty flag; the pair tree's
  // nodes by height (sph_hoff: the heights' ends in sph_hlist) and the refit's unwidened boxes; the host form's staging
  rfx::DevBuf<uint32_t> sph_slot, sph_dirty, sph_ids;
  rfx::DevBuf<int32_t> sph_hlist;
  rfx::DevBuf<rfx::SphBox> sph_lbox, sph_nbox;
  rfx::DevBuf<float> sph_data;
  std::vector<uint32_t> sph_hoff;
  uint32_t upd_sph = 0;
  // per-phase event timing: triples {start, after pre-pass, after trace} on every timing_every-th frame (the events'
  // own cost stays off the other frames: ~10 us per frame for three records at C1's 640x480)
  bool timing = false, timing_this = false;
  uint32_t timing_every = 1;
  uint64_t timing_seq = 0;
  std::vector<hipEvent_t> events;
  size_t events_used = 0;
};

namespace rfx {
// rfx_host.cpp, for the other units
int set_dev(rfx_renderer *r);  // hipSetDevice(r->device)
int ensure_seq_table(rfx_renderer *r, hipStream_t st);  // the cycle table, built on first use
// the stream state a frame of several passes starts from, saved on `st` (r's device current) before the first
int save_rewind_state(rfx_renderer *r, hipStream_t st);
// The pre-pass of n traces that are no frame (rfx_rays.cpp), in the form an unsplit one-device frame launch of n traces
// takes: their randDir states into r->rd on `st`, the sphere stream n accepted triples on, the jitter stream untouched.
// Fails while an emitted frame is pending; the call cannot be undone by rfx_frame_rng_rewind.
int prepass_traces(rfx_renderer *r, uint64_t n, hipStream_t st);
// rfx_update.cpp: the moving-mesh tables of the scene set_scene has just uploaded (r's device current, its stream idle)
int upload_update_tables(rfx_renderer *r, const SceneBuild &B);

// ---- what the batch entry points share (rfx_rays.cpp, rfx_hits.cpp, rfx_order.cpp)
// A call's opening tests: its arguments (args_ok false, or no renderer: "<call>: <required>") and an uploaded scene
inline int check_call(const rfx_renderer *r, bool args_ok, const char *call, const char *required)
{
  if (!r || !args_ok) return fail(RFX_ERR_ARG, "%s: %s", call, required);
  if (!r->has_scene) return fail(RFX_ERR_STATE, "%s: no scene uploaded", call);
  return RFX_OK;
}
// ... and the renderer's device made current
inline int enter_call(rfx_renderer *r, bool args_ok, const char *call, const char *required)
{
  RCHECK(check_call(r, args_ok, call, required));
  return set_dev(r);
}
inline hipStream_t stream_or_own(const rfx_renderer *r, void *stream) { return stream ? (hipStream_t)stream : r->stream; }

// Rays per launch of a batch of raster width W (0: linear): at most launch_traces, rounded down to whole waves
// (linear) or whole tile rows (raster) and never below one, so that every launch but the last is made of full waves and
// its outputs start 16-B aligned where the batch's do.  A wave's raster tile is 8 x 8 rays; a raster launch takes whole
// tile rows, at most kMaxTileRowsPerLaunch (the grid's y limit).
constexpr uint64_t kTileRows = 8, kMaxTileRowsPerLaunch = 32768;
inline uint64_t rays_per_launch(const rfx_renderer *r, uint64_t W)
{
  const uint64_t unit = W ? kTileRows * W : 64;
  uint64_t units = std::max<uint64_t>(1, r->launch_traces / unit);
  if (W) units = std::min(units, kMaxTileRowsPerLaunch);
  return units * unit;
}

// a hit query's output planes: whether the caller wants any, and their place in the launch record
inline bool any_plane(const rfx_hit_planes *o)
{
  return o->object || o->distance || o->point || o->normal || o->reflected || o->colour;
}
inline void set_planes(HitParams &P, const rfx_hit_planes *o)
{
  P.object = o->object;
  P.distance = o->distance;
  P.point = o->point;
  P.normal = o->normal;
  P.reflected = o->reflected;
  P.colour = o->colour;
}
}  // namespace rfx
