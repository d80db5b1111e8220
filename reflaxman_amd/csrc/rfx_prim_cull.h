// rfx_prim_cull.h -- prim_cull_kernel: the per-view cull masks of a small scene's frame, built once per view from the
// primary rays trace_kernel will form.  Launched by rfx_kernels.hip (launch_prim_cull) only.
#pragma once
#include <hip/hip_runtime.h>

#include "rfx_trace.h"

#pragma clang fp contract(off)

namespace rfx {

// Per-view masks of a small scene's plain or SSAA frame (FrameParams::prim_mask), kPrimStride words per wave tile t8:
// [0] the cull mask of the tile's primary bundle, [1 + q] that of its primary hits' shadow rays toward light q
// for every randDir (q < kPrimLights).  Wave t8 builds its tile's primary rays exactly as trace_kernel does (same
// tile mapping, same validity), their bundle (one origin: the eye) and cull mask -- with the triangle footprint
// test, which the trace kernel could not afford per segment -- then the primary hits with the same closest-hit
// code and that mask, and per light the bundle of all shadow rays of the facing lanes (make_bundle_ball).  The
// masks depend only on the view (camera, frame geometry, scene), so the host builds them once per view.
// LANES: the tiles of a kModeSsaaLanes frame (sampleNum 1 jittered, 2, 4, 8): wave t8 covers bw x bw pixels, one sample
// per lane, exactly as trace_kernel's lanes branch maps them; its masks cover the lanes' own rays (jittered: each lane's
// unit jitter square), so the shadow masks need one primary hit per lane.  A kModeSsaaChunks frame (sampleNum > 8, the
// wave is one pixel): the closest-hit mask of the pixel's whole sample rectangle, which every chunk of its samples reuses;
// no shadow masks (they would need the primary hit of every sample).
// narrow (rfx_renderer_set_prim_exact): where the hits are known ahead (no jitter, no chunks) the conservative words are
// narrowed to what those hits need -- [0] to the tile's winners, [1 + q] without the one object all its facing hits lie on.
// Per-view masks of SSAA / additive frames (RFX_PRIM_SSAA): built, parity-tested and measured slower in round 4 (the
// screenshot frame +4.3%; interleaved A/B, profiles/r04/ab/), so compiled out by default.  RFX_PRIM_LANES: per-view masks
// of kModeSsaaLanes frames (sampleNum 1 jittered, 2, 4, 8: the wave's own bw x bw pixels)
template <bool PLANES, bool LANES = false>
__global__ RFX_TRACE_BOUNDS void prim_cull_kernel(DevScene S, FrameParams P, uint64_t *masks, int narrow)
{
  stage_small_scene(S);
  __syncthreads();
  const Tabs<true> T{S};
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(wave);
  const uint32_t w8 = kTileWavesX * gridDim.x;
  const uint32_t t8 = (blockIdx.y * kTileWavesY + wv / kTileWavesX) * w8 + blockIdx.x * kTileWavesX + wv % kTileWavesX;
  uint32_t gx, gy, kk = 0;
  float lox = 0.0f, loy = 0.0f;  // LANES: the lane's sample offsets (Render.cpp:183), as trace_kernel forms them
  const bool chunks = LANES && P.ss > 8;
  if constexpr (LANES)
  {
    const uint32_t ss = (uint32_t)P.ss, ss2 = ss * ss, bw = ss_lane_block(P.ss);
    const uint32_t q = bw == 1 ? 0 : lane / ss2;
    kk = chunks ? 0 : bw == 1 ? lane : lane - q * ss2;
    const uint32_t sx = kk / ss, sy = kk - sx * ss;
    gx = (t8 % w8) * bw + q % bw;
    gy = (t8 / w8) * bw + q / bw;
    const float ssf = (float)(int)ss;
    lox = sx ? (float)(int)sx / ssf : 0.0f;
    loy = sy ? (float)(int)sy / ssf : 0.0f;
  }
  else
  {
    gx = (t8 % w8) * 8u + (lane & 7u);
    gy = (t8 / w8) * 8u + (lane >> 3);
  }
  const uint32_t x = gx;
  const uint32_t y = P.nranks > 1 ? strip_row_to_y(gy, P) : gy + P.row0;
  const uint64_t p = (uint64_t)y * P.W + x;
  const bool valid = gx < P.W && gy < P.grid_rows && p >= P.p_begin && p < P.p_end && P.depth > 0 &&
                     (!LANES || kk < (uint32_t)(P.ss * P.ss));
  m33 view;
  view.m11 = P.v11; view.m12 = P.v12; view.m13 = P.v13;
  view.m21 = P.v21; view.m22 = P.v22; view.m23 = P.v23;
  view.m31 = P.v31; view.m32 = P.v32; view.m33 = P.v33;
  const v3 eye = mk(P.eye_x, P.eye_y, P.eye_z);
  const float rx = (float)x - P.wh, ry = (float)y - P.hh;                       // Render.cpp:152-153
  uint64_t *out = masks + (size_t)kPrimStride * t8;
  // one sample per pixel without jitter: the plain rays themselves; SSAA and jittered (additive) frames: every ray of
  // the pixel's sample rectangle [rx, rx + omax] x [ry, ry + omax] (Render.cpp:177-183: offsets (ss - 1) / ss at most,
  // plus a jitter of at most 1 in additive frames), through its four corners
  const int ss = P.ss;
  const bool exact = (LANES || ss == 1) && !P.additive && !chunks;
  uint64_t om = 0;
  if (__ballot(valid))
  {
    Bundle B;
    if (exact)  // as trace_kernel (plain: rx + 0 + 0; lanes: rx + float(sx) / ss + 0)
      B = make_bundle(eye, mmul(view, mk(rx + lox + 0.0f, ry + loy + 0.0f, P.rz)), valid);
    else
    {
      // LANES: the lane's jitter square; else (and chunks) the pixel's sample rectangle
      const float bx = rx + lox, by = ry + loy;
      const float omax = LANES && !chunks ? 1.0f : (float)(ss - 1) / (float)ss + (P.additive ? 1.0f : 0.0f);
      const v3 q[4] = {mmul(view, mk(bx, by, P.rz)), mmul(view, mk(bx + omax, by, P.rz)),
                       mmul(view, mk(bx, by + omax, P.rz)), mmul(view, mk(bx + omax, by + omax, P.rz))};
      B = make_bundle_quad(eye, q, valid);
    }
    om = B.ok ? cull_small<true>(T.cull(), S.cull_valid, B, S.cull_tri) : S.cull_valid;
  }
  // the primary hits of every sample, as trace_from's first segment finds them with this mask (Scene.cpp:86-106), and
  // per light the union of their shadow bundles' masks.  Jittered frames and chunks: the hits are not known ahead, no
  // shadow masks (FrameParams::prim_shadow; the trace kernel builds those bundles itself).
  const bool known = !P.additive && !chunks;
  const int nl = known ? min(S.n_light, kPrimLights) : 0;
  uint64_t sm[kPrimLights] = {0, 0, 0, 0};
  // narrow: the two exact rules on top of the conservative words.  win: the union of the tile's winners' bits -- the
  // closest-hit rule (distance, then object index) does not depend on the order or on the losers tested beside the
  // winner, so every lane finds the same Hit among the winners alone.  own[q]: the one object that every facing
  // (lane, sample) toward light q hit (kOwnNone: no facing lane yet, kOwnMixed: more than one object) -- the any-hit
  // test discards that object's answer (occluded_small: skip_sph / skip_tri), so its bit only costs a test.
  constexpr int kOwnNone = -1, kOwnMixed = -2, kOwnPlane = 64;
  uint64_t win = 0;
  int own[kPrimLights] = {kOwnNone, kOwnNone, kOwnNone, kOwnNone};
  const float ssf = (float)ss;
  const int nss = LANES ? 1 : ss;  // LANES: the lane's one sample
  for (int sx = 0; known && (nl > 0 || narrow) && sx < nss; ++sx)
    for (int sy = 0; sy < nss; ++sy)
    {
      // the sample's ray exactly as trace_kernel forms it (plain: rx + 0 + 0; SSAA: rx + float(sx) / ss + 0)
      const float ox = LANES ? lox : sx ? (float)sx / ssf : 0.0f, oy = LANES ? loy : sy ? (float)sy / ssf : 0.0f;
      const v3 ray = mmul(view, mk(rx + ox + 0.0f, ry + oy + 0.0f, P.rz));
      Cnt cnt;
      Hit h;
      if (valid) closest_hit_small<false, PLANES>(S, eye, ray, om, h, cnt);
      else h.obj = -1;
      const bool hit = valid && h.obj >= 0;
      // the winner's bit in the lane layout of the masks (small_pairs / small_tris); planes are in no mask
      const int bit = !hit ? kOwnPlane : h.kind == 0 ? (h.i & 1) * 16 + (h.i >> 1) : h.kind == 1 ? 32 + h.i : kOwnPlane;
      for (uint64_t c = narrow ? om : 0; c; c &= c - 1ull)  // the winners are among the mask's objects
      {
        const int b = __builtin_ctzll(c);
        if (__ballot(bit == b)) win |= 1ull << b;
      }
      v3 drop = eye, norm = mk(0.0f, 0.0f, 0.0f);
      if (hit)
      {
        drop = add(eye, mul(ray, h.t));
        if (h.kind == 0)
        {
          const SphereGeo g = T.sph_geo(h.i);
          norm = sub(drop, mk(g.cx, g.cy, g.cz));                                // Sphere.cpp:67
        }
        else if (!PLANES || h.kind == 1)
        {
          const TriShade sh = T.tri_shade(h.i);
          norm = mk(sh.nx, sh.ny, sh.nz);
        }
        else
        {
          const PlaneGeo g = S.pln_geo[h.i];
          norm = mk(g.nx, g.ny, g.nz);                                           // Plane.cpp:58-59
        }
      }
      for (int q = 0; q < nl; ++q)
      {
        const LightRec L = S.lights[q];
        const v3 dtl = sub(mk(L.ox, L.oy, L.oz), drop);
        const bool facing = hit && dot(dtl, norm) > kVerySmall;                  // Scene.cpp:125
        const uint64_t fb = __ballot(facing);
        if (fb)
        {
          const Bundle SB = make_bundle_ball(drop, dtl, L.radius, facing);
          sm[q] |= SB.ok ? cull_small(T.cull(), S.cull_valid, SB) : S.cull_valid;
          const int first = __builtin_amdgcn_readlane(bit, __builtin_ctzll(fb));
          const int now = __ballot(facing && bit != first) ? kOwnMixed : first;
          own[q] = own[q] == kOwnNone || own[q] == now ? now : kOwnMixed;
        }
      }
    }
  if (known && narrow)
  {
    om = win;
    // a sphere loses its own bit only: its pair is still tested where the partner's bit is set (small_pairs ORs the two)
    for (int q = 0; q < nl; ++q)
      if (own[q] >= 0 && own[q] < kOwnPlane) sm[q] &= ~(1ull << own[q]);
  }
  if (lane == 0) out[0] = om;
  for (int q = 0; q < kPrimLights; ++q)  // the words past the scene's lights are 0 (never read; a defined read-back)
    if (lane == 0) out[1 + q] = sm[q];
}

}  // namespace rfx
