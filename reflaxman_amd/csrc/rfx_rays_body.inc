// rfx_rays_body.inc -- the text of a ray-batch trace kernel, written once and included inside the body of each kernel
// that is one: trace_rays_kernel (rfx_rays.h) and trace_rays_ordered_kernel (rfx_ordered.h).  No unit includes it on
// its own.  The including kernel provides, by these names: its parameters DevScene S and FrameParams P, the template
// arguments or constants STATS and CFG, the type Rays (RasterRays or OrderedRays: which ray a lane takes and whether a
// full wave's outputs lie together), and its own `__shared__ float lut[256]`.
//
// Text, not a function: these kernels sit at their register limit (72 VGPRs at 7 waves per SIMD, spills in every one),
// and a __forceinline__ function template is optimised on its own, with S and P behind pointers, before it is inlined --
// the kernel's passes then start from other IR and the allocator ends elsewhere (profiles/r16: trace_rays<stats,14>
// lost 25 spills that way, against the rule that a refactor leaves every kernel's resource row alone).  Included as
// text the kernels compile as they did with the text written out in each.
//
// Every lane of a wave reaches trace() -- lanes past the batch's end or outside the raster as invalid -- so the bounce
// loop's bundles stay wave-wide; with no per-view mask the first segment builds its bundle from what the lanes hold,
// and a wide cone takes the unculled or per-lane BVH path as an incoherent secondary segment does.
  static_assert(!(CFG & kCfgPark), "a ray batch never parks (ray_records rides in a parking field)");
  constexpr bool CULL = (CFG & kCfgCull) != 0, MANYL = (CFG & kCfgManyLights) != 0, SMALL = (CFG & kCfgSmall) != 0;
  constexpr bool PLANES = (CFG & kCfgPlanes) != 0, ONEL = (CFG & kCfgOneLight) != 0, TBVH = (CFG & kCfgTriBvh) != 0;
  const uint32_t lane = threadIdx.x & 63u, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const Rays rays = Rays::here();
  const uint32_t unit = rays.unit(P, wv);
  // the unit waits in LDS across the bounce loop: the epilogue re-derives the lane's ray from it (as trace_kernel does)
  if (lane == 0) s_tile8[wv] = unit;
  const RaySlot sl = rays.slot(P, unit, lane);
  const bool valid = sl.valid;
  // The lane's record and randDir state are read first: they come from HBM once and are never read again, and the
  // staging below (L2-resident tables, a workgroup barrier) runs while they are on their way.  One 24-B read per lane;
  // the same records as 16-B-per-lane loads through LDS measured 0.7 - 1.0% slower (DESIGN.md "Ray batches").
  v3 o = mk(0.0f, 0.0f, 0.0f), d = mk(0.0f, 0.0f, 0.0f);
  uint32_t rds = 0;
  if (valid)
  {
    const RayRecord r = load_ray(ray_records(P), sl.i);
    o = r.o;
    d = r.d;
    rds = P.rd_state[sl.i];
  }
  for (uint32_t i = threadIdx.x; i < 256; i += kWgThreads) lut[i] = (float)i / 255.0f;  // Color.cpp:11-13
  stage_powf_tables();
  if constexpr (SMALL) stage_small_scene(S);
  __syncthreads();
  Cnt cnt;
  if constexpr (STATS)
  {
#pragma unroll
    for (int k = 0; k < C_COUNT; ++k) cnt.c[k] = 0;
  }
  const v3 rd = valid ? rd_from_state(rds) : mk(0.0f, 0.0f, 0.0f);
  const col out = trace<STATS, CULL, MANYL, SMALL, PLANES, ONEL, TBVH>(S, o, d, P.depth, rd, lut, cnt, valid);
  {
#ifdef RFX_LAUNDER_PARAMS
    const FrameParams &P = kernarg_params();  // shadows the caller's record: re-read after the bounce loop
#endif
    const uint32_t ue = ((volatile uint32_t *)s_tile8)[wv];
    uint32_t le = lane;
    asm volatile("" : "+v"(le));  // a fresh lane value: the ray's index is derived again, not kept live
    const RaySlot se = rays.slot(P, ue, le);
    bool staged = false;
    if constexpr (Rays::kStaged)
    {
      const bool aligned = ((reinterpret_cast<uintptr_t>(P.img) | reinterpret_cast<uintptr_t>(P.argb)) & 15u) == 0;
      staged = aligned && (P.W & 3u) == 0 && __builtin_amdgcn_ballot_w64(se.valid) == ~0ull;
    }
    if (staged && P.W)
      store_wave_tile(P, se.x0, se.row0, out, le, wv);
    else if (staged)
      store_wave_run(P, ue, out, le, wv);
    else if (se.valid)
    {
      float *p = P.img + se.i * 3;
      p[0] = out.r; p[1] = out.g; p[2] = out.b;
      if (P.argb) P.argb[se.i] = argb(out);
    }
    flush_counters<STATS>(P, cnt);
  }
