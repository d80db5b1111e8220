// Every compile-time switch of librfx.so, with its default: the one place a switch is given a value, included first by
// rfx_types.h and rfx_math.h, so host and device units always agree.  A build overrides one with -DNAME=value
// (tools/ab.py VARIANTS builds such variants for interleaved A/B timing); tests/test_build_switches.py checks that
// every name a variant passes is declared here and defaulted nowhere else.  Each line: what a non-default value does,
// and where the measurement behind the default is recorded (a DESIGN.md heading or a file under profiles/).
// Experiments that were measured and removed are in DESIGN.md, with the last commit that carries their code.
#pragma once

// ---- exact arithmetic (rfx_math.h)
#ifndef RFX_DIV_FAST
#define RFX_DIV_FAST 1  // 0: every quotient as the compiler lowers '/'; 2: no range guard, timing builds only (DESIGN.md "Division fast path")
#endif
#ifndef RFX_DIV_SINGLE
#define RFX_DIV_SINGLE 0  // 1: a lone quotient takes the guarded fast path too (DESIGN.md "Division fast path")
#endif

// ---- hierarchies (rfx_types.h, rfx_scene.cpp)
#ifndef RFX_BVH_LEAF_PAIRS
#define RFX_BVH_LEAF_PAIRS 4  // sphere pairs per leaf of the pair BVH: 1, 2 or 8 (DESIGN.md "Round-5 kernel changes and experiments")
#endif
#ifndef RFX_TRI_BVH
#define RFX_TRI_BVH 1  // 0: the kernels without the triangle walkers (DESIGN.md "Triangle BVH")
#endif
#ifndef RFX_TRI_BVH_LEAF
#define RFX_TRI_BVH_LEAF 4  // triangle records per leaf of the triangle BVH (DESIGN.md "Triangle BVH")
#endif
#ifndef RFX_TRI_BVH_AUTO_MIN
#define RFX_TRI_BVH_AUTO_MIN 128  // triangles from which rfx_renderer_set_tri_accel(-1) builds the tree (DESIGN.md "Triangle BVH")
#endif
#ifndef RFX_TRI_BVH_NARROW_MIN
#define RFX_TRI_BVH_NARROW_MIN (1 << 30)  // triangles from which narrow bundles walk the tree too; 0: always (DESIGN.md "Triangle BVH")
#endif

// ---- trace kernels (rfx_trace.h and the device headers it includes)
#if !defined(RFX_WAVES_PER_EU) && defined(RFX_LANES_WAVES_PER_EU) && defined(RFX_UNIT_LANES_FAST)
#define RFX_WAVES_PER_EU RFX_LANES_WAVES_PER_EU  // rfx_trace_lanes_fast.hip alone (it defines RFX_UNIT_LANES_FAST): that family's own target
#endif
#ifndef RFX_WAVES_PER_EU
#define RFX_WAVES_PER_EU 7  // the trace kernels' occupancy target: 6 or 8 (rfx_shade_inputs.h, at kWgWaves; DESIGN.md "Large scenes", occupancy re-checked)
#endif
#ifndef RFX_WG_WAVES
#define RFX_WG_WAVES 2  // waves per workgroup: 1 or 4 (measurements in rfx_shade_inputs.h, at kWgWaves)
#endif
#ifndef RFX_TRI_MATES
#define RFX_TRI_MATES 2  // coplanar mates share the z stage: 0 never, 1 both small-scene loops, 3 shadow loop only (DESIGN.md "Exact work skipping", coplanar mates)
#endif
#ifndef RFX_FAR_LIGHT
#define RFX_FAR_LIGHT 1  // a far light's constant terms from its record: 0 never, 2 the shading terms only, 3 the shadow cone only (DESIGN.md "Far lights")
#endif
#ifndef RFX_SHADOW_GRID
#define RFX_SHADOW_GRID 1  // a far light's per-cell occluder masks: 0 no grid is built and the kernels carry no grid path, 2 the mask load after the facing test (DESIGN.md "Shadow grid")
#endif
#ifndef RFX_SHADOW_GRID_CELLS
#define RFX_SHADOW_GRID_CELLS (1 << 16)  // the grid's cell budget, 8 bytes a cell: (1 << 14) or (1 << 18) (DESIGN.md "Shadow grid")
#endif
#ifndef RFX_CULL_FMA
#define RFX_CULL_FMA 1  // 0: the bundle and cull bounds without fused multiply-adds (DESIGN.md "Large scenes", fused cull bounds)
#endif
#ifndef RFX_NARROW_BUNDLE_COS
#define RFX_NARROW_BUNDLE_COS 0.9995f  // bundles narrower than this cull chunks wave-wide; 2.0f: every bundle walks the BVH (profiles/r04/ab/c5_narrow_bundle_cos.jsonl)
#endif
#ifndef RFX_OCC_HINT
#define RFX_OCC_HINT 1  // 0: shadow walks without the wave's last occluder tested first (DESIGN.md "Round-5 kernel changes and experiments")
#endif
#ifndef RFX_ONE_LIGHT
#define RFX_ONE_LIGHT 1  // 0: no one-light kernel instantiations (DESIGN.md "Round-4 kernel specialisations and experiments")
#endif
#ifndef RFX_SSAA_LANES
#define RFX_SSAA_LANES 1  // 0: every SSAA frame runs one lane per pixel (DESIGN.md "SSAA frames: one lane per sample")
#endif
#ifndef RFX_SSAA_CHANNEL_SUM
#define RFX_SSAA_CHANNEL_SUM 1  // 0: SSAA epilogues without one lane per colour channel for the ordered sample sum (DESIGN.md "Round-5 kernel changes and experiments")
#endif
#ifndef RFX_PRIM_SSAA
#define RFX_PRIM_SSAA 0  // 1: per-view masks for kModeSsaa frames too, measured slower (profiles/r04/ab/)
#endif
#ifndef RFX_PRIM_LANES
#define RFX_PRIM_LANES 1  // 0: no per-view masks for kModeSsaaLanes frames (DESIGN.md "SSAA frames: one lane per sample")
#endif
#ifndef RFX_PRIM_CHUNKS
#define RFX_PRIM_CHUNKS 1  // 0: no closest-hit masks for kModeSsaaChunks frames (DESIGN.md "Round-5 kernel changes and experiments")
#endif
#ifndef RFX_NOCULL_MAX_TILES
#define RFX_NOCULL_MAX_TILES 0  // N > 0: small scenes in frames of at most N wave tiles skip the bundle cull (DESIGN.md "Numbers (round 4)")
#endif

// ---- RNG pre-pass (rfx_kernels.hip, rfx_host.cpp)
#ifndef RFX_RNG_INT_ACCEPT
#define RFX_RNG_INT_ACCEPT 1  // 0: the accept test in float for every triple (DESIGN.md "RNG pre-pass: the accept test in integers")
#endif
#ifndef RFX_RNG_TICKET
#define RFX_RNG_TICKET 1  // 0: rng_fused in blockIdx order, timing builds only (DESIGN.md "Round 6 against the round-5 verdict", row 1)
#endif
#ifndef RFX_LOOKBACK_SLEEP
#define RFX_LOOKBACK_SLEEP 1  // s_sleep between polls of a not yet published status word, in units of 64 cycles (rfx_kernels.hip rng_fused)
#endif
#ifndef RFX_LOOKBACK_SPINS
#define RFX_LOOKBACK_SPINS (1u << 22)  // 0: every wait gives up at once, a timing build that exercises the fallback (profiles/r06/ab/c1_r6b.jsonl)
#endif
#ifndef RFX_SCAN_TILES
#define RFX_SCAN_TILES 2  // launches of at least this many tiles of kScanTileCounts blocks scan in many workgroups; 0: never (profiles/r06/ab/shot128_tile_scan_r6c.jsonl)
#endif
#ifndef RFX_SCAN_EMIT_BLOCKS
#define RFX_SCAN_EMIT_BLOCKS 16384  // emits of more RNG blocks scan the counts first (profiles/r06/ab/*_scan_emit_threshold_r6x.jsonl)
#endif
#ifndef RFX_RNG_FUSED
#define RFX_RNG_FUSED 1  // 0: the two-kernel pre-pass where the cycle table is off (profiles/r06/ab/prepass_limit_*_r6e.jsonl)
#endif
#ifndef RFX_RNG_FUSED_MAX_BLOCKS
#define RFX_RNG_FUSED_MAX_BLOCKS 256  // launches of at most this many pre-pass blocks take rng_fused (profiles/r06/ab/prepass_limit_*_r6e.jsonl)
#endif
#ifndef RFX_RNG_SEQ
#define RFX_RNG_SEQ 1  // 0: one-device unsplit frames use the count / emit kernels, no cycle table (DESIGN.md "RNG pre-pass: the LCG's cycle tabulated once")
#endif
#ifndef RFX_RNG_SEQ_SPLIT
#define RFX_RNG_SEQ_SPLIT 1  // 0: the spans of split frames keep the count / scan / emit kernels (DESIGN.md "Numbers (round 7)", seqsplit0)
#endif
#ifndef RFX_RNG_SEQ_MIN_BLOCKS
#define RFX_RNG_SEQ_MIN_BLOCKS 0  // launches of fewer pre-pass blocks keep rng_fused (DESIGN.md "Numbers (round 7)")
#endif

// ---- frame scheduling (rfx_host.cpp)
#ifndef RFX_TILE_ORDER_DEFAULT
#define RFX_TILE_ORDER_DEFAULT 1  // 0: raster order; 2: raster order with the tile costs still recorded (DESIGN.md "Tile schedule")
#endif
#ifndef RFX_TILE_ORDER_MIN_TILES
#define RFX_TILE_ORDER_MIN_TILES 49152  // frames of fewer 8x8 wave tiles keep raster order (DESIGN.md "Tile schedule", threshold)
#endif
#ifndef RFX_TILE_SORT_MAIN
#define RFX_TILE_SORT_MAIN 1  // 0: the tile sort on a side stream (profiles/r06/ab/*_tile_sort_r6q.jsonl)
#endif
#ifndef RFX_TILE_SORT_EVERY
#define RFX_TILE_SORT_EVERY 16  // the tile sort runs every N-th launch (profiles/r06/ab/*_tile_sort_r6q.jsonl)
#endif
#ifndef RFX_PARK_AFTER
#define RFX_PARK_AFTER 2  // large-scene plain frames: segments before a live trace is parked; 0: never (profiles/r04/ab/c5_park_retune.jsonl)
#endif
#ifndef RFX_QUEUE_SORT
#define RFX_QUEUE_SORT 0  // 1: the bounce kernel takes parked traces bucket by bucket, measured slower (measurements in rfx_host.cpp, at kMaxLaunchTraces)
#endif
#ifndef RFX_BOUNCE_GROUPS_PER_CU
#define RFX_BOUNCE_GROUPS_PER_CU 14  // the bounce kernel's workgroups per CU: 8 or 16 measured +-0.6% (DESIGN.md "Large scenes")
#endif
#ifndef RFX_LAUNCH_TRACES
#define RFX_LAUNCH_TRACES (1ull << 30)  // traces per launch of a split frame, rfx_renderer_set_launch_traces (profiles/r06/ab/shot128_launch_size_r6i.jsonl)
#endif
#ifndef RFX_SPLIT_STREAMS
#define RFX_SPLIT_STREAMS 2  // 1: the spans of a split frame on one stream, no overlap (DESIGN.md "Frames of any sample count")
#endif

// ---- switches without a default of their own: unset, each takes the value of the switch it refines
//   RFX_WAVES_PER_EU_LARGE  the large-scene trace kernels' RFX_WAVES_PER_EU (rfx_trace.h, at trace_kernel; profiles/r04/ab/c5_large_scene_occupancy.jsonl)
//   RFX_LANES_WAVES_PER_EU  rfx_trace_lanes_fast.hip's RFX_WAVES_PER_EU, applied above (DESIGN.md "Large scenes", occupancy re-checked)

// ---- presence flags: defined or not, no value
//   RFX_NO_LAUNDER      the kernel arguments held in registers across the bounce loops: neither flag below is derived
//   RFX_LAUNDER_SCENE   the DevScene re-read from the kernarg segment in every segment (derived in rfx_bounce.h)
//   RFX_LAUNDER_PARAMS  the FrameParams re-read after the bounce loop (derived in rfx_bounce.h)
//   RFX_DEBUG_PROF      per-phase cycle counters and cull statistics (tools/build_diag.py)
//   RFX_DEBUG_SEGS      per-trace segment counts
//   RFX_DEBUG_WAVES     per-wave start / end timestamps
