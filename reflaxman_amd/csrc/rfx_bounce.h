// rfx_bounce.h -- Scene::trace (Scene.cpp:73-236) as a wave-wide bounce loop: trace_from runs the segments of every live
// lane from a start or mid-trace state (closest hit, shadow rays, material, shading, the next ray or the sky), trace is
// its form for a fresh primary ray.  With it: what a trace needs to park for the bounce kernel (Park, queue_key), the
// wave's output staging s_out, and the kernel arguments re-read through the kernarg segment pointer (launder_scene,
// kernarg_params, the layout they assume; RFX_LAUNDER_SCENE / RFX_LAUNDER_PARAMS are derived here).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>

#include "rfx_cull_rule.h"
#include "rfx_math.h"
#include "rfx_types.h"
#include "rfx_shade_inputs.h"
#include "rfx_queries.h"

#pragma clang fp contract(off)

namespace rfx {

// ------------------------------------------------------------- Scene::trace
// Scene::trace (Scene.cpp:73-236) for one trace per lane, the bounce loop run wave-wide: every
// iteration is one segment of every live lane -- closest hit, then per light the facing test and the
// shadow any-hit (Scene.cpp:117-141; the occlusion tests depend on nothing the shading computes, so
// they run first, with few registers live), then material, shading and the next ray or the sky.
// CULL: wave bundles skip objects no live lane can hit (closest hit and shadow rays); MANYL: more than
// 32 lights (shadow masks and shading in blocks of 32); PLANES: the scene holds planes.  Call with every lane
// of the wave active; `valid` lanes trace.  Returns the trace's colour (zero for invalid lanes).
// Parking (ray regrouping): where the bounce loop would start segment `park` of a trace, the trace's state is
// appended to the queue instead (one atomic per wave, packed lane order) and the trace ends here; the bounce
// kernel resumes it from exactly that state, so every float op is the same.
struct Park {
  int after;           // segments before parking (<= 0: never)
  QRay *queue;
  uint32_t *count;
  uint32_t trace, out;  // this lane's randDir trace index and output pixel
  static constexpr bool kRefill = false;
  __device__ __forceinline__ void ids(uint32_t &t, uint32_t &o) const { t = trace; o = out; }
  __device__ __forceinline__ uint32_t *keys() const { return nullptr; }
  __device__ __forceinline__ BvhGlobal bvh() const { return BvhGlobal{}; }
};

// Regroup sort key of a parked trace (RFX_QUEUE_SORT): its direction octant and the Morton index of its origin's cell
// in an 8 x 8 x 8 grid over the BVH root box -- traces of one bucket walk similar BVH paths.  Only the order in which
// the bounce kernel takes the traces depends on it, never a value (every trace resumes from its own state).
__device__ __forceinline__ uint32_t queue_key(const DevScene &S, v3 o, v3 d)
{
  const auto cell = [](float v, float lo, float s) -> uint32_t {
    return (uint32_t)fminf(fmaxf((v - lo) * s, 0.0f), 7.0f);  // NaN: fmaxf takes the 0
  };
  const uint32_t cx = cell(o.x, S.key_lx, S.key_sx), cy = cell(o.y, S.key_ly, S.key_sy), cz = cell(o.z, S.key_lz, S.key_sz);
  uint32_t m = 0;
#pragma unroll
  for (int b = 0; b < 3; ++b)
    m |= (((cx >> b) & 1u) << (3 * b)) | (((cy >> b) & 1u) << (3 * b + 1)) | (((cz >> b) & 1u) << (3 * b + 2));
  const uint32_t oct = (d.x < 0.0f ? 1u : 0u) | (d.y < 0.0f ? 2u : 0u) | (d.z < 0.0f ? 4u : 0u);
  return oct << 9 | m;
}

// Per wave: the epilogue's staging of the wave's 64 pixels (store_wave_tile: 192 RGB floats + 64 ARGB words)
__shared__ __attribute__((aligned(16))) uint32_t s_out[kWgWaves][256];

// Scene::trace from a mid-trace state (mulc, pix after `refl` segments); park: see Park.  *parked: this lane's
// trace was queued and its returned colour is not final.
// Kernel arguments re-read where they are used (round 4, on by default; RFX_NO_LAUNDER turns it off): the DevScene in
// every bounce segment of the large-scene kernels, the FrameParams after the bounce loop.  Kept in SGPRs across the loops, they
// spilled to VGPR lanes (C5 trace kernel: 102 -> 25 SGPR spills, C5 trace + bounce -1.6%; C3: 23 -> 8, -0.3%;
// interleaved A/B, profiles/r04/ab/).
#ifndef RFX_NO_LAUNDER
#define RFX_LAUNDER_SCENE
#define RFX_LAUNDER_PARAMS
#endif
#ifdef RFX_LAUNDER_SCENE
typedef const __attribute__((address_space(4))) DevScene *ConstScenePtr;
// The record is read through the kernarg segment pointer: every kernel that reaches trace_from (trace_kernel,
// bounce_kernel, bounce_kernel_lds) takes the DevScene as its first argument, at offset 0.  (Taking the address of
// the by-value parameter instead makes the compiler copy it to scratch, and a constant-space pointer to that copy
// faults.)
template <bool ON>
__device__ __forceinline__ const DevScene &launder_scene(const DevScene &S)
{
  if constexpr (!ON) return S;
  ConstScenePtr p = (ConstScenePtr)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const DevScene *)p;
}
#define RFX_SCENE_PARAM S_in
#else
#define RFX_SCENE_PARAM S
#endif
// The frame parameters (the kernels' second argument, after the DevScene) read through the kernarg segment pointer, laundered
// by an empty asm: every use reloads them with scalar loads where it stands, so their values are not held in SGPRs
// across a bounce loop (with RFX_LAUNDER_PARAMS: the epilogue and the park ids)
constexpr size_t kParamsOff = (sizeof(DevScene) + alignof(FrameParams) - 1) / alignof(FrameParams) * alignof(FrameParams);
// The layout both readers assume, checked where it is defined (host and device passes): by-value kernel arguments are
// laid out like the members of a struct, so (DevScene, FrameParams, ...) puts the record at 0 and the parameters at
// kParamsOff.  Every kernel that reads them this way asserts its own signature (kKernargSig, in its body), and
// tests/test_gpu_kat.py::test_kernarg_layout compares the laundered reads with the by-value arguments on the device.
struct KernargPair { DevScene S; FrameParams P; };
static_assert(offsetof(KernargPair, S) == 0 && offsetof(KernargPair, P) == kParamsOff,
              "kernel-argument layout: DevScene at offset 0, FrameParams at kParamsOff");
template <class F>
constexpr bool kKernargSig = std::is_same<F, void (*)(DevScene, FrameParams)>::value;
template <bool LAUNDER = true>  // false: the plain kernarg reference, which the compiler may keep in registers
__device__ __forceinline__ const FrameParams &kernarg_params()
{
  typedef const __attribute__((address_space(4))) char *KP;
  KP p = (KP)__builtin_amdgcn_kernarg_segment_ptr();
  if constexpr (LAUNDER) asm volatile("" : "+s"(p));
  return *(const FrameParams *)(const __attribute__((address_space(4))) FrameParams *)(p + kParamsOff);
}

// A far light's bound (rfx_types.h LightRec::near): origin - d is origin, bit for bit, for this d.  A NaN coordinate
// fails, and so does every d when near is 0.
__device__ __forceinline__ bool near_light(const LightRec &L, v3 d)
{
  return fabsf(d.x) < L.near && fabsf(d.y) < L.near && fabsf(d.z) < L.near;
}

// A light's record read again where it is used: the far-light kernels' shading pass, so the 16 dwords are not held in
// SGPRs across the shadow any-hit.  The pointer passes through an empty asm that also takes `when`, a wave-uniform value
// of the current segment, so the read can neither merge with an earlier one nor leave the bounce loop.  The asm is not
// volatile: a volatile one counts as a write to memory, after which no load of the loop is a scalar load any more.  The
// pointer is a constant-space one, or the compiler no longer knows what it points into and reads with flat loads.
__device__ __forceinline__ LightRec reread_light(const LightRec *l, uint64_t when)
{
  typedef const __attribute__((address_space(4))) LightRec *ConstLightPtr;
  ConstLightPtr p = (ConstLightPtr)l;
  asm("" : "+s"(p) : "s"(when));
  return *(const LightRec *)p;
}

// The far light's occluder grid (rfx_types.h ShadowGrid, the DevScene's last member) read from the kernarg segment where
// the shadow pass uses it, as reread_light reads the light: its twelve dwords are not held in SGPRs across the closest
// hit, and the asm is not volatile.  Every kernel that reaches the grid path takes the DevScene at kernarg offset 0
// (kKernargSig).
__device__ __forceinline__ ShadowGrid reread_grid(uint64_t when)
{
  typedef const __attribute__((address_space(4))) char *KP;
  KP p = (KP)__builtin_amdgcn_kernarg_segment_ptr();
  asm("" : "+s"(p) : "s"(when));
  return *(const ShadowGrid *)(const __attribute__((address_space(4))) ShadowGrid *)(p + offsetof(DevScene, shadow_grid));
}

// FARL (with ONEL, SMALL and CULL, never STATS; RFX_FAR_LIGHT picks the halves): the scene's one light is far
// (rfx_scene.cpp far_light_terms), so where a hit lies inside its bound the terms of the light that do not depend on the
// hit -- dtl, its length and direction, ang > 0 and 1 - sqrt(ang) -- are read from the record, and a wave whose facing
// hits all lie inside takes the shadow bundle's cone from it too (make_bundle_far).  Every other hit, and every other
// instantiation, runs the expressions below as they stand.
// GRID (FARL kernels that take the cone, RFX_SHADOW_GRID): where the scene carries the light's occluder grid and every
// facing hit of the wave lies inside both the light's bound and the grid's box, the shadow mask is the OR of the facing
// lanes' cell masks instead of a cull of the wave's bundle: a cell's mask is cull_small's verdict, made on the host, for
// the bundle of every shadow ray that starts in the cell, and a lane's ray is one of them (DESIGN.md "Shadow grid").  One
// ballot decides for the wave; a wave with a facing hit outside takes the bundle path unchanged.  Each hit lane loads
// its cell's mask as soon as drop is known (RFX_SHADOW_GRID 2: the facing lanes, once the wave has chosen the grid).
// SGRID false: a far-light kernel without the grid path -- the SSAA families, whose waves hold the samples of one or a
// few pixels: their hits stay so close together that the wave's own bundle culls tighter than a cell's ball, and the
// 4 x 4 screenshot traced 1.2% slower with the grid; and the parking form, which spilled one VGPR more with it
// (DESIGN.md "Shadow grid").
template <bool STATS, bool CULL, bool MANYL, bool SMALL, bool PLANES, bool PARK, class PK, bool ONEL = false,
          bool TBVH = false, bool FARL = false, bool SGRID = FARL>
__device__ __forceinline__ col trace_from(const DevScene &RFX_SCENE_PARAM, v3 origin, v3 ray, col mulc, col pix, int refl,
                                          int depth, v3 rd, const float *lut, Cnt &cnt, bool valid, const PK &park,
                                          bool &parked, const uint64_t *pm_tile = nullptr, bool pm_shadow = true)
{
#ifdef RFX_LAUNDER_SCENE
  const DevScene &S = S_in;
#endif
  static_assert(!FARL || (ONEL && SMALL && CULL && !MANYL && !STATS), "FARL: the small-scene one-light culling kernels");
  constexpr bool FAR_SHADE = FARL && (RFX_FAR_LIGHT == 1 || RFX_FAR_LIGHT == 2);
  constexpr bool FAR_CONE = FARL && (RFX_FAR_LIGHT == 1 || RFX_FAR_LIGHT == 3);
  constexpr bool GRID = FAR_CONE && SGRID && RFX_SHADOW_GRID != 0;
  constexpr bool GRID_EARLY = GRID && RFX_SHADOW_GRID != 2;
  // the first segment of a plain small-scene trace: this tile's per-view masks (prim_cull_kernel) -- the closest
  // hit's, then one per light for its shadow rays
  bool seg0 = pm_tile != nullptr;
  parked = false;
  if (valid && refl == 0) RFX_CNT(C_RAYS);
  const Tabs<SMALL> T{S};
  bool alive = valid && refl < depth;
  int occ_hint = -1;  // large scenes: the shadow rays' occluder hint (occluded_spheres_bvh)
#ifdef RFX_DEBUG_SEGS
  int nseg = 0;  // diagnostic build only (tools/segstats.py): the trace's segment count replaces its colour
#endif
  RFX_PROF_BEGIN(P_SEG);
  while (__ballot(alive))
  {
#ifdef RFX_DEBUG_SEGS
    if (alive) ++nseg;
#endif
#ifdef RFX_LAUNDER_SCENE
    // experiment: the scene record re-read (scalar loads from the kernarg segment) in every segment instead of its
    // fields held in SGPRs across the bounce loop, where they spill to VGPR lanes
    const DevScene &S = launder_scene<!SMALL>(S_in);  // large scenes only: the small-scene kernel spills VGPRs with it
    const Tabs<SMALL> T{S};
#endif
    Hit h;
    if constexpr (SMALL)
    {
      uint64_t om = S.cull_valid;
      if constexpr (CULL)
      {
        if (seg0)
          om = pm_tile[0];  // the primary bundle's mask, precomputed for this tile's view (prim_cull_kernel)
        else
        {
          const Bundle B = make_bundle(origin, ray, alive);
          if (B.ok) om = cull_small(T.cull(), S.cull_valid, B);
          RFX_CULL_STAT(0, B.ok, __ballot(alive), om, S.cull_valid);
        }
      }
      if (alive) closest_hit_small<STATS, PLANES>(S, origin, ray, om, h, cnt);
      else h.obj = -1;
    }
    else
    {
      Bundle B;
      if constexpr (CULL) B = make_bundle(origin, ray, alive);
      closest_hit<STATS, PLANES, TBVH>(S, origin, ray, alive, CULL ? &B : nullptr, h, cnt, park.bvh());
    }
    const bool hit = alive && h.obj >= 0;
    // re-derive the winner's outputs with the reference's expressions
    v3 drop = origin, norm = mk(0.0f, 0.0f, 0.0f);
    RFX_PROF_BEGIN(P_WIN);
    if (hit)
    {
      drop = add(origin, mul(ray, h.t));
      if (h.kind == 0)
      {
        RFX_CNT(C_HIT_SPH);
        const SphereGeo g = T.sph_geo(h.i);
        norm = sub(drop, mk(g.cx, g.cy, g.cz));                                // Sphere.cpp:67
      }
      else if (!PLANES || h.kind == 1)
      {
        RFX_CNT(C_HIT_TRI);
        const TriShade sh = T.tri_shade(h.i);
        norm = mk(sh.nx, sh.ny, sh.nz);
      }
      else
      {
        RFX_CNT(C_HIT_PLN);
        const PlaneGeo g = S.pln_geo[h.i];
        norm = mk(g.nx, g.ny, g.nz);                                               // Plane.cpp:58-59
      }
    }
    RFX_PROF_END(P_WIN);
    const int skip_sph = h.kind == 0 ? h.i : -1, skip_tri = h.kind == 1 ? h.i : -1;
    const int skip_pln = PLANES && h.kind == 2 ? h.i : -1;
    MatRec m{0.0f, 0.0f, 0.0f, 0.0f};
    int diel = 0;
    v3 reflv = mk(0.0f, 0.0f, 0.0f);
    float rayLen = 0.0f, normLen = 0.0f, reflectLen = 0.0f;
    col sumL = mkc(0.0f, 0.0f, 0.0f), sumS = mkc(0.0f, 0.0f, 0.0f);
    for (int base = 0;; base += 32)                                            // Scene.cpp:117-181
    {
      RFX_PROF_BEGIN(P_SHADOW);
      uint32_t lit = 0;
      const int nl = ONEL ? 1 : min(32, S.n_light - base);  // ONEL: the scene has exactly one light
      for (int q = 0; q < nl; ++q)
      {
        const LightRec L = S.lights[base + q];
        bool facing = false;
        v3 sray = mk(0.0f, 0.0f, 0.0f);
        // the grid: this lane's cell and, loaded ahead of the facing test, its mask (not where the per-view masks serve)
        ShadowGrid G{};
        bool in_grid = false;
        int32_t cell = 0;
        uint64_t cell_mask = 0;
        if constexpr (GRID)
        {
          G = reread_grid(__ballot(hit));
          // no lane is in the grid where there is none, or where the per-view masks serve this segment; the wave's
          // choice below is then one ballot over its facing lanes and reads nothing else
          in_grid = shadow_grid_cell(G, drop.x, drop.y, drop.z, &cell) & hit & (G.cells != nullptr) & !(seg0 && pm_shadow);
          if constexpr (GRID_EARLY)
            if (in_grid) cell_mask = G.cells[cell];
        }
        if (hit)
        {
          RFX_CNT(C_L_EVAL);
          const v3 dtl = sub(mk(L.ox, L.oy, L.oz), drop);
          if (dot(dtl, norm) > kVerySmall)
          {
            RFX_CNT(C_L_FACING);
            facing = true;
            sray = add(dtl, mul(rd, L.radius));                                  // Scene.cpp:129
          }
        }
        if (__ballot(facing))
        {
          if constexpr (SMALL)
          {
            uint64_t om = S.cull_valid;
            if constexpr (CULL)
            {
              if (!MANYL && seg0 && pm_shadow && q < kPrimLights)
                om = pm_tile[1 + q];  // the primary hits' shadow mask for light q, precomputed for the view
              else if (GRID && __ballot(facing & !(in_grid & near_light(L, drop))) == 0)
              {
                if constexpr (!GRID_EARLY)
                  if (facing) cell_mask = G.cells[cell];
                om = wave_or(facing ? cell_mask : 0ull) & S.cull_valid;
                RFX_CULL_STAT(1, true, __ballot(facing), om, S.cull_valid);
              }
              else
              {
                Bundle SB;
                bool far_cone = false;
                if constexpr (FAR_CONE) far_cone = __ballot(facing && !near_light(L, drop)) == 0;  // wave-uniform
                if (far_cone) SB = make_bundle_far(drop, L, facing);
                else SB = make_bundle(drop, sray, facing);
                if (SB.ok) om = cull_small(T.cull(), S.cull_valid, SB);
                RFX_CULL_STAT(1, SB.ok, __ballot(facing), om, S.cull_valid);
              }
            }
            if (facing && !occluded_small<STATS, PLANES>(S, drop, sray, skip_sph, skip_tri, skip_pln, om, cnt))
              lit |= 1u << q;
          }
          else
          {
            Bundle SB;
            if constexpr (CULL) SB = make_bundle(drop, sray, facing);
            const bool occ = occluded<STATS, PLANES, TBVH>(S, drop, sray, facing, skip_sph, skip_tri, skip_pln,
                                                     CULL ? &SB : nullptr, cnt, park.bvh(), &occ_hint);
            if (facing && !occ) lit |= 1u << q;
          }
        }
      }
      RFX_PROF_END(P_SHADOW);
      RFX_PROF_BEGIN(P_LIGHT);
      if (hit)
      {
        if (!MANYL || base == 0)
        {
          // the hit object's material, texel, reflection and lengths (Sphere.cpp:66-80, Triangle.cpp:86-105)
          if (h.kind == 0)
          {
            m = T.sph_mat(h.i);
            diel = T.sph_info(2 * h.i + 1);
          }
          else if (PLANES && h.kind == 2)
          {
            m = S.pln_mat[h.i];                                                  // untextured (Plane.cpp:67-68)
            diel = S.pln_geo[h.i].dielectric;
          }
          else
          {
            const TriShade sh = T.tri_shade(h.i);
            m = T.tri_mat(h.i);
            diel = sh.dielectric;
            if (sh.tex >= 0)
            {
              const col c = tri_texel<STATS>(S, sh, h.u, h.v, lut, cnt);
              m.r = c.r; m.g = c.g; m.b = c.b;
            }
          }
          reflv = reflect(mul(ray, h.t), norm);                                // trace_math.cpp:14-23
          rayLen = len(ray); normLen = len(norm); reflectLen = len(reflv);
        }
        for (int q = 0; q < nl; ++q)
        {
          if (!((lit >> q) & 1u)) continue;
          RFX_CNT(C_L_LIT);
          const LightRec L = FAR_SHADE ? reread_light(S.lights + (base + q), __ballot(lit != 0)) : S.lights[base + q];
          if constexpr (FAR_SHADE)
          {
            // the light's terms from its record where the hit lies inside its bound, by the expressions of the general
            // form below where not; the rest of the shading is the general form's, operation for operation
            v3 dtl = mk(L.ox, L.oy, L.oz), ndl = mk(L.ndx, L.ndy, L.ndz);
            float dlen = L.dlen, spec_add = L.spec_add;
            bool spec = true;
            if (!near_light(L, drop))
            {
              dtl = sub(dtl, drop);
              dlen = len(dtl);
              const float a2 = sqlen(dtl);
              const float ang = (a2 > kVerySmall) ? 1.0f - qdiv(L.radius * L.radius, a2) : 0.0f;
              spec = ang > 0;
              if (spec)
              {
                ndl = normalized(dtl);
                spec_add = 1.0f - sqrt_rn(ang);
              }
            }
            float aa = dlen * normLen;
            const float cosl = (aa > kVerySmall) ? qdiv(dot(dtl, norm), aa) : 0.0f;
            const col lc = mkc(L.r, L.g, L.b);
            if (L.power > kVerySmall) sumL = cadd(sumL, cscale(cscale(lc, cosl), L.power));
            if (spec)
            {
              const v3 dlr = add(ndl, mul(rd, 1.0f - m.refl));
              aa = len(dlr) * reflectLen;
              float sc = (aa > kVerySmall) ? qdiv(dot(dlr, reflv), aa) : 0.0f;
              sc = clampf(sc + spec_add, 0.0f, 1.0f);
              if (sc > kVerySmall && L.radius > kVerySmall)
              {
                const float sp = powf_dev(sc, 1 + qdiv(3 * m.refl * dlen, L.radius)) * m.refl;
                sumS = cadd(sumS, cscale(lc, sp));
              }
            }
            continue;
          }
          const v3 dtl = sub(mk(L.ox, L.oy, L.oz), drop);
          const float dlen = len(dtl);
          float aa = dlen * normLen;
          const float cosl = (aa > kVerySmall) ? qdiv(dot(dtl, norm), aa) : 0.0f;
          const col lc = mkc(L.r, L.g, L.b);
          if (L.power > kVerySmall) sumL = cadd(sumL, cscale(cscale(lc, cosl), L.power));
          aa = sqlen(dtl);
          const float ang = (aa > kVerySmall) ? 1.0f - qdiv(L.radius * L.radius, aa) : 0.0f;
          if (ang > 0)
          {
            RFX_CNT(C_L_SPEC);
            const v3 dlr = add(normalized(dtl), mul(rd, 1.0f - m.refl));
            aa = len(dlr) * reflectLen;
            float sc = (aa > kVerySmall) ? qdiv(dot(dlr, reflv), aa) : 0.0f;
            sc = clampf(sc + (1.0f - sqrt_rn(ang)), 0.0f, 1.0f);
            if (sc > kVerySmall && L.radius > kVerySmall)
            {
              RFX_CNT(C_L_POW);
              const float sp = powf_dev(sc, 1 + qdiv(3 * m.refl * dlen, L.radius)) * m.refl;
              sumS = cadd(sumS, cscale(lc, sp));
            }
          }
        }
      }
      RFX_PROF_END(P_LIGHT);
      if (!MANYL || base + 32 >= S.n_light) break;
    }
    if (hit)
    {
      RFX_PROF_BEGIN(P_MAT);
      sumL = cadd(mkc(S.amb_r, S.amb_g, S.amb_b), sumL);                        // Scene.cpp:186
      const col color = mkc(m.r, m.g, m.b);
      col fin;
      if (diel)                                                                  // Scene.cpp:189-201
      {
        RFX_CNT(C_DIELECTRIC);
        const float aa = rayLen * normLen;
        const float cosA = (aa > kVerySmall) ? clampf(qdiv(dot(ray, neg(norm)), aa), 0.0f, 1.0f) : 0.0f;
        const float r = 0.2f + 0.8f * powf3_dev(1.0f - cosA);
        fin = cadd(cmul(cscale(color, 1.0f - r), sumL), sumS);
        fin = cmul(fin, mulc);
        mulc = cscale(mulc, r);
      }
      else                                                                       // Scene.cpp:202-212
      {
        RFX_CNT(C_METAL);
        const float r = 0.8f;
        fin = cadd(cmul(cscale(color, 1.0f - r), sumL), sumS);
        fin = cmul(fin, mulc);
        mulc = cmul(mulc, cscale(color, r));
      }
      pix = cclamp(cadd(pix, fin));                                              // Scene.cpp:215-216
      RFX_PROF_END(P_MAT);
      if (mulc.r < 0.01f && mulc.g < 0.01f && mulc.b < 0.01f)                    // Scene.cpp:219-220
        alive = false;
      else
      {
        RFX_CNT(C_CONTINUE);
        origin = drop;                                                           // Scene.cpp:223-224
        ray = add(normalized(reflv), mul(rd, 1.0f - m.refl));
        if (++refl >= depth) alive = false;                                      // Scene.cpp:78
      }
    }
    else if (alive)                                                              // Scene.cpp:226-231
    {
      RFX_CNT(C_SKY);
      RFX_PROF_BEGIN(P_SKY);
      pix = cclamp(cadd(pix, cmul(cmul(mulc, skybox_texel<STATS>(S, ray, lut, cnt)), mkc(S.env_r, S.env_g, S.env_b))));
      RFX_PROF_END(P_SKY);
      alive = false;
    }
    seg0 = false;
    if constexpr (!STATS && PARK)
    {
      if (refl == park.after && __ballot(alive))
      {
        // every lane of the wave is here (wave-uniform loop); the live ones append their state
        const uint64_t pm = __ballot(alive);
        uint32_t base = 0;
        if (__lane_id() == (uint32_t)(__ffsll((long long)pm) - 1)) base = atomicAdd(park.count, (uint32_t)__popcll(pm));
        base = __builtin_amdgcn_readlane(base, __ffsll((long long)pm) - 1);
        if (alive)
        {
          QRay q;
          q.ox = origin.x; q.oy = origin.y; q.oz = origin.z; q.dx = ray.x;
          q.dy = ray.y; q.dz = ray.z; q.mr = mulc.r; q.mg = mulc.g;
          q.mb = mulc.b; q.pr = pix.r; q.pg = pix.g; q.pb = pix.b;
          uint32_t qt, qo;
          park.ids(qt, qo);
          q.trace = qt; q.out = qo; q.refl = (uint32_t)refl; q.pad = 0;
          const uint32_t slot = base + (uint32_t)__popcll(pm & ((1ull << __lane_id()) - 1ull));
          park.queue[slot] = q;
          if (uint32_t *keys = park.keys()) keys[slot] = queue_key(S, origin, ray);
          parked = true;
          alive = false;
        }
      }
    }
    // the bounce kernel: traces that ended this segment write their pixels, idle lanes take new ones (Refill)
    if constexpr (PK::kRefill) park.refill(alive, origin, ray, mulc, pix, refl, rd);
  }
  RFX_PROF_END(P_SEG);
#ifdef RFX_DEBUG_SEGS
  return mkc((float)nseg, 0.0f, 0.0f);
#else
  return pix;
#endif
}

template <bool STATS, bool CULL, bool MANYL, bool SMALL, bool PLANES, bool ONEL = false, bool TBVH = false,
          bool FARL = false, bool SGRID = FARL>
__device__ __forceinline__ col trace(const DevScene &S, v3 origin, v3 ray, int depth, v3 rd, const float *lut,
                                     Cnt &cnt, bool valid, const uint64_t *pm_tile = nullptr, bool pm_shadow = true)
{
  bool parked;
  return trace_from<STATS, CULL, MANYL, SMALL, PLANES, false, Park, ONEL, TBVH, FARL, SGRID>(S, origin, ray, mkc(1.0f, 1.0f, 1.0f), mkc(0.0f, 0.0f, 0.0f), 0,
                                                       depth, rd, lut, cnt, valid, Park{0, nullptr, nullptr, 0, 0},
                                                       parked, pm_tile, pm_shadow);
}

}  // namespace rfx
