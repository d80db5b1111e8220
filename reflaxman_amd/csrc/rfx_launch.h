// Every function of namespace rfx that crosses a translation unit of librfx.so, declared once: the host files call
// through this header and the .hip files that define the functions include it (rfx_trace.h does), so the compiler
// checks each definition against its declaration.
#pragma once
#include <hip/hip_runtime.h>

#include "rfx_types.h"
#include "rfx_order_types.h"

namespace rfx {
// ---- rfx_kernels.hip: the RNG pre-pass (count / emit kernels, the one-pass kernel, the cycle table)
uint64_t rng_blocks_for(uint64_t traces);
void rng_jump_table(uint64_t nblk, uint32_t *out);
hipError_t launch_rng_count(const uint32_t *d_seed, const uint32_t *d_jump, uint32_t *d_blk_cnt, uint64_t blk0,
                            uint64_t nblk_slice, uint16_t *d_masks, hipStream_t st);
hipError_t launch_rng_finish(const uint32_t *d_seed, const uint32_t *d_jump, uint32_t *d_next_seed,
                             const uint32_t *d_blk_cnt, const uint16_t *d_masks, uint64_t nblk, uint64_t traces,
                             uint32_t *d_rd_state, int *d_err, uint64_t ss2, uint64_t W, uint32_t row_block,
                             uint32_t rank, uint32_t nranks, hipStream_t st);
hipError_t launch_rng_finish_band(const uint32_t *d_seed, const uint32_t *d_jump, uint32_t *d_next_seed,
                                  const uint32_t *d_blk_cnt, const uint16_t *d_masks, uint64_t nblk, uint64_t traces,
                                  uint32_t *d_rd_state, int *d_err, uint64_t lo, uint64_t hi, uint64_t *d_off,
                                  uint32_t *d_range, uint32_t *d_tile_sum, hipStream_t st);
hipError_t launch_rng_fused(const uint32_t *d_seed, const uint32_t *d_jump, uint32_t *d_next_seed, uint64_t nblk,
                            uint64_t traces, uint32_t *d_rd_state, int *d_err, unsigned long long *d_status,
                            unsigned long long *d_ticket, unsigned long long base, uint32_t epoch, hipStream_t st);
uint32_t rng_seq_blocks();
uint32_t rng_seq_header_words();
void rng_seq_tables(uint32_t *hdr, uint32_t *state);
uint32_t rng_seq_index_of(uint32_t s);
hipError_t launch_rng_seq_build(const uint32_t *d_hdr, const uint32_t *d_state, uint32_t *d_p, uint32_t *d_tiles,
                                hipStream_t st);
hipError_t launch_rng_locate(const uint32_t *d_seed, const uint32_t *d_hdr, const uint32_t *d_state, const uint32_t *d_p,
                             uint32_t *d_pos, hipStream_t st);
hipError_t launch_rng_emit_seq(const uint32_t *d_pos, const uint32_t *d_hdr, const uint32_t *d_state, const uint32_t *d_p,
                               uint64_t nblk, uint64_t traces, uint32_t *d_rd_state, uint32_t *d_next_seed,
                               uint32_t *d_next_pos, int *d_err, hipStream_t st);
// ---- rfx_kernels.hip: the trace launch, its per-view masks, the tile and regroup sorts, the known-answer kernels
hipError_t launch_trace(const DevScene &S, const FrameParams &P, bool stats, hipStream_t st);
hipError_t launch_prim_cull(const DevScene &S, const FrameParams &P, uint64_t *masks, bool narrow, hipStream_t st);
hipError_t launch_queue_sort(const uint32_t *count, const uint32_t *key, uint32_t *hist, uint32_t *order, hipStream_t st);
uint32_t trace_tiles(const FrameParams &P);
bool trace_lanes(const FrameParams &P);
bool trace_chunks(const FrameParams &P);
size_t tile_order_scratch();
hipError_t launch_tile_order(const uint32_t *cost, uint32_t n, uint32_t *order, uint32_t *scratch, hipStream_t st);
hipError_t launch_kat(int what, const DevScene &S, int tex, const void *in, const int32_t *objs, uint32_t n, void *out,
                      hipStream_t st);
hipError_t launch_kat_powf_cube(uint32_t first, uint32_t n, unsigned long long *counts, hipStream_t st);
hipError_t launch_kat_div(uint64_t first, uint32_t n, unsigned long long *counts, hipStream_t st);
hipError_t launch_kat_kernarg(const DevScene &S, const FrameParams &P, int swapped, uint32_t *out, hipStream_t st);
// ---- one trace_kernel family each (rfx_trace_<mode>_<stats>.hip), the parking kernels and the bounce kernels
// (rfx_trace_plain_park.hip)
#define RFX_DECLARE_TRACE_FAMILY(name) \
  void name(int cfg, dim3 grid, const DevScene &S, const FrameParams &P, hipStream_t st)
RFX_DECLARE_TRACE_FAMILY(launch_trace_plain_fast);
RFX_DECLARE_TRACE_FAMILY(launch_trace_plain_stats);
RFX_DECLARE_TRACE_FAMILY(launch_trace_ssaa_fast);
RFX_DECLARE_TRACE_FAMILY(launch_trace_ssaa_stats);
RFX_DECLARE_TRACE_FAMILY(launch_trace_lanes_fast);
RFX_DECLARE_TRACE_FAMILY(launch_trace_lanes_stats);
RFX_DECLARE_TRACE_FAMILY(launch_trace_chunks_fast);
RFX_DECLARE_TRACE_FAMILY(launch_trace_chunks_stats);
RFX_DECLARE_TRACE_FAMILY(launch_trace_block_fast);
RFX_DECLARE_TRACE_FAMILY(launch_trace_block_stats);
RFX_DECLARE_TRACE_FAMILY(launch_trace_plain_park);
RFX_DECLARE_TRACE_FAMILY(launch_bounce);
hipError_t launch_bounce_lds(int cfg, uint32_t groups, const DevScene &S, const FrameParams &P, hipStream_t st);
// ---- rfx_trace_rays.hip: one launch of a ray batch (rfx_rays.h trace_rays_kernel) -- P.p_end rays whose records start
// at d_rays, P.W the raster width or 0
hipError_t launch_trace_rays(const DevScene &S, const FrameParams &P, const float *d_rays, bool stats, hipStream_t st);
// ---- rfx_trace_hits.hip: one launch of a hit query (rfx_hits.h) -- P.n rays; any: the any-hit kernel, else the
// closest-hit one
hipError_t launch_query_hits(const DevScene &S, const HitParams &P, bool any, hipStream_t st);
// ---- rfx_order_sort.hip: the ray keys (keys2: a second copy, or null), and one digit pass of the stable radix sort --
// the pairs (kin[i], iin[i]) (iin null: the index i itself) go to (kout, iout) (kout null: indices only) by the digit
// at `shift`; table: kOrderDigits x order_groups(n) words, totals: kOrderDigits words of scratch
uint32_t order_groups(uint32_t n);
hipError_t launch_order_keys(const OrderBox &B, const float *d_rays, uint32_t n, uint32_t *keys, uint32_t *keys2,
                             hipStream_t st);
hipError_t launch_order_pass(const uint32_t *kin, const uint32_t *iin, uint32_t *kout, uint32_t *iout, uint32_t n,
                             uint32_t shift, uint32_t *table, uint32_t *totals, hipStream_t st);
// ---- rfx_trace_ordered.hip: one launch of an ordered ray batch (rfx_ordered.h trace_rays_ordered_kernel: P.p_end rays
// and as many slots of d_order) and of an ordered hit query
hipError_t launch_trace_rays_ordered(const DevScene &S, const FrameParams &P, const float *d_rays,
                                     const uint32_t *d_order, hipStream_t st);
hipError_t launch_query_hits_ordered(const DevScene &S, const HitOrderParams &P, bool any, hipStream_t st);
// ---- rfx_update_kernels.hip: moving meshes (rfx_refit.h) -- the updated triangles' records, the leaves' boxes, and the nodes
// of one height from the boxes below them
struct UpdateParams;
struct RefitParams;
hipError_t launch_update_tris(const UpdateParams &P, hipStream_t st);
hipError_t launch_refit_leaves(const RefitParams &P, hipStream_t st);
hipError_t launch_refit_nodes(const RefitParams &P, hipStream_t st);
// ... and re-cutting: the in-tree triangles' sort keys from their current vertices (the box reduction, then the keys);
// after the sort, the slots, leaf records and the cut's topology put in place
struct RecutParams;
struct RecutPlaceParams;
hipError_t launch_recut_keys(const RecutParams &P, hipStream_t st);
hipError_t launch_recut_place(const RecutPlaceParams &P, hipStream_t st);
// ---- rfx_sphere_update_kernels.hip: moving spheres (rfx_refit.h) -- the updated spheres' records, the dirty chunks'
// bounds, the pair tree's leaf boxes, and its nodes of one height from the boxes below them
struct SphUpdateParams;
struct SphRefitParams;
hipError_t launch_update_spheres(const SphUpdateParams &P, hipStream_t st);
hipError_t launch_refit_chunks(const SphRefitParams &P, hipStream_t st);
hipError_t launch_refit_pair_leaves(const SphRefitParams &P, hipStream_t st);
hipError_t launch_refit_pair_nodes(const SphRefitParams &P, hipStream_t st);
}  // namespace rfx
