// rfx_intersect.h -- one ray against one primitive, and which hit wins.  Sphere::trace for a pair of spheres (RayConst,
// pair_bd, pair_may_hit, sphere_tail), Triangle::trace in its stages (tri_z, tri_zt, tri_rows, tri_uv; tri_hit runs
// them, TriMates shares the z stage among coplanar triangles), Plane::trace (plane_hit); then the closest-hit record
// (Hit) and the reference's (distance, insertion index) rule on squared distances (sph_takes, tri_takes).  Every
// expression rounds as the reference's; each early reject says why it is exact.
#pragma once
#include <hip/hip_runtime.h>

#include "rfx_math.h"
#include "rfx_types.h"
#include "rfx_diag.h"

#pragma clang fp contract(off)

namespace rfx {

// ------------------------------------------------------------- primitives
// Per-ray constants of Sphere::trace (Sphere.cpp:50-52,58), hoisted out of the object loop.
struct RayConst {
  v3 ray2;      // 2.0f * ray
  float a4, a2; // 4.0f * a, 2.0f * a  with a = |ray|^2
  bool a_ok;    // a > VERY_SMALL_NUMBER
  DivRcp a2d;   // the divisor 2a of every sphere's t, its reciprocal shared (rfx_math.h div_prep)
};
__device__ __forceinline__ RayConst ray_const(v3 ray)
{
  RayConst k;
  const float a = sqlen(ray);
  k.ray2 = mul(ray, 2.0f);
  k.a4 = 4.0f * a;
  // 2a = +inf (a caller's ray of 1.3e19 or longer) is kept as NaN.  No sphere is hit either way: the reference's
  // t = x / inf is 0 or NaN, and x / NaN fails `t > VERY_SMALL_NUMBER` as well.  But nz^2 * 2a = +inf against a finite
  // bound would let the closest-hit rejects before the division (tri_z, plane_hit) drop a crossing that is nearer than
  // the best hit; with NaN every such comparison fails in the keeping direction.
  const float a2 = 2.0f * a;
  k.a2 = a2 < INFINITY ? a2 : __builtin_nanf("");
  k.a_ok = a > kVerySmall;
  k.a2d = div_prep(k.a2);
  return k;
}

// Sphere::trace (Sphere.cpp:44-85) for spheres 2j and 2j+1 at once, up to the discriminant: each half
// of an f2 runs the reference's scalar expressions in the reference's order (vco = o - c,
// b = 2ray . vco, c = |vco|^2 - r^2, d = b*b - 4a*c), so v_pk_* results round exactly as scalar ones.
typedef float f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void pair_bd(const SpherePair &g, v3 o, const RayConst &k, f2 &b, f2 &d)
{
  const f2 vx = o.x - f2{g.cx[0], g.cx[1]};
  const f2 vy = o.y - f2{g.cy[0], g.cy[1]};
  const f2 vz = o.z - f2{g.cz[0], g.cz[1]};
  b = k.ray2.x * vx + k.ray2.y * vy + k.ray2.z * vz;
  const f2 c = vx * vx + vy * vy + vz * vz - f2{g.r2[0], g.r2[1]};
  d = b * b - k.a4 * c;
}

// Can either sphere of a pair hit?  d < 0 misses; so does b >= 0 (or NaN), since then -b - sqrt(d) <= 0
// gives t <= 0, which `t > VERY_SMALL_NUMBER` rejects (Sphere.cpp:58-60) -- both are exact rejects.
__device__ __forceinline__ bool pair_may_hit(f2 b, f2 d)
{
  return (d.x >= 0.0f && b.x < 0.0f) || (d.y >= 0.0f && b.y < 0.0f);
}

// The rest of Sphere::trace for one sphere given its b and d: on a hit returns t and |ray t|^2.
// `(ray * t).length() > DELTA` (Sphere.cpp:61-64) is tested as |ray t|^2 >= kSqDeltaSphere: the same
// decision without the square root (rfx_math.h).
// SEL (large-scene loops): one branch, the rest computed and decided without branching.  tools/ab.py, trace ms: C5
// 3.143 -> 3.067 (-2.4%); the small-scene kernel +9% with it (its SGPR spills 23 -> 51), so the small loops keep the
// early outs.  The SEL tail divides with '/': the shared reciprocal of 2a, live across the BVH walk, raised the C5 trace
// kernel's VGPR spills from 15 to 36 and its time by 5.9% (tools/ab.py, profiles/r06/ab/c5_div_sel_prefetch_r6c.jsonl)
template <bool STATS, bool SHADOW, bool SEL = false>
__device__ __forceinline__ bool sphere_tail(float b, float d, v3 ray, const RayConst &k, float &t_out,
                                            float &sq_out, Cnt &cnt)
{
  RFX_CNT(SHADOW ? C_SH_SPH_TESTS : C_SPH_TESTS);
  if constexpr (STATS)
    if (!(b > 0.0f)) RFX_CNT(SHADOW ? C_SH_SPH_B : C_SPH_B);
  if constexpr (!STATS && SEL)
  {
    if (!(d >= 0.0f && k.a_ok && b < 0.0f)) return false;
    const float t = (-b - sqrt_rn(d)) / k.a2;
    const float sq = sqlen(mul(ray, t));
    t_out = t;
    sq_out = sq;
    return t > kVerySmall && sq >= kSqDeltaSphere;
  }
  if (!(d >= 0.0f && k.a_ok)) return false;
  // b >= 0 (or NaN): -b - sqrt(d) <= 0, so t <= 0 and `t > VERY_SMALL_NUMBER` rejects -- exact early out
  if constexpr (!STATS)
    if (!(b < 0.0f)) return false;
  if constexpr (STATS)
    if (!(b > 0.0f)) RFX_CNT(SHADOW ? C_SH_SPH_D : C_SPH_D);
  const float t = div_by(-b - sqrt_rn(d), k.a2d);
  if (!(t > kVerySmall)) return false;
  RFX_CNT(SHADOW ? C_SH_SPH_T : C_SPH_T);
  const float sq = sqlen(mul(ray, t));
  if (!(sq >= kSqDeltaSphere)) return false;
  t_out = t;
  sq_out = sq;
  return true;
}

// Triangle::trace (Triangle.cpp:53-108) up to its hit decision; on a hit returns t, u, v, |ray t|^2.
// axTrans * (o - v0) and axTrans * ray are evaluated row by row with the reference's expressions: the
// z row first, then -- only for t > VERY_SMALL_NUMBER -- the x and y rows as one packed chain
// ((aox, aoy), (arx, ary), (u, v)), each half rounding exactly as the scalar expression.
// PRE: reject plane crossings outside the triangle before the divide (below).  tools/ab.py, trace ms: large-scene
// shadow rays 3.399 -> 3.327 on C5 (-2.1%); small scenes (C3) +0.6% in either loop, closest hit on C5 0%.
// The z stage: everything that depends on the triangle only through its plane -- the third row of axTrans and the
// components of v0 that row weighs (coplanar mates, rfx_scene.cpp tri_mate_leaders, share it: tri_z of any member
// gives every member's answer and t).  False: no hit, whatever (u, v).
template <bool STATS, bool SHADOW>
__device__ __forceinline__ bool tri_z(const TriGeo &g, v3 o, v3 ray, const RayConst &k, float best_sq, Cnt &cnt,
                                      float &nz_out, float &arz_out)
{
  RFX_CNT(SHADOW ? C_SH_TRI_TESTS : C_TRI_TESTS);
  const float dx = o.x - g.v0x, dy = o.y - g.v0y, dz = o.z - g.v0z;
  const float aoz = dx * g.a31 + dy * g.a32 + dz * g.a33;
  const float arz = ray.x * g.a31 + ray.y * g.a32 + ray.z * g.a33;
  if (!(fabsf(arz) > kVerySmall)) return false;
  RFX_CNT(SHADOW ? C_SH_TRI_Z : C_TRI_Z);
  // t = -aoz / arz > VERY_SMALL_NUMBER needs -aoz and arz non-zero with equal signs (event counter only)
  const float nz = -aoz;
  const bool same_sign = (nz > 0.0f && arz > 0.0f) || (nz < 0.0f && arz < 0.0f);
  if constexpr (STATS)
    if (same_sign) RFX_CNT(SHADOW ? C_SH_TRI_S : C_TRI_S);
  // exact reject before the division: with opposite signs or a zero (or NaN) numerator, t <= 0 or NaN,
  // which `t > VERY_SMALL_NUMBER` rejects anyway; the divide is skipped when no lane of the wave needs it
  if (!same_sign) return false;
  if constexpr (!STATS)
  {
    // |ray t|^2 = a nz^2 / arz^2 (real, a2 = 2a exactly).  Within DELTA of the origin (a shadow ray or a reflected
    // ray leaving the triangle it starts on, or its coplanar neighbour: nz ~ 0): the reference's sqDistance, within
    // ~10 ulp of it, is at most DELTA^2 under the 2^-15 margin, so `sqDistance > DELTA * DELTA` fails -- exact reject
    // before the divide (tools/ab.py trace ms: C3 -1.1%, C2 d4 -3.4%, C5 -0.4%).
    const float n2a = nz * nz * k.a2, r2 = arz * arz;
    if (n2a < (2.0f * (kDelta * kDelta)) * r2 * 0.99997f) return false;
    // beyond the current closest hit (closest hit only): a 2^-16 margin over the rounding of both sides leaves
    // |ray t| strictly above the best distance after rounding, so the reference could neither take it nor tie
    if constexpr (!SHADOW)
      if (n2a > best_sq * r2 * 2.0000305f) return false;
  }
  nz_out = nz; arz_out = arz;
  return true;
}
// ... and its end: the quotient, one eleven-instruction IEEE divide (DESIGN "Division fast path")
template <bool STATS, bool SHADOW>
__device__ __forceinline__ bool tri_zt(float nz, float arz, float &t_out, Cnt &cnt)
{
  const float t = qdiv(nz, arz);
  if (!(t > kVerySmall)) return false;
  RFX_CNT(SHADOW ? C_SH_TRI_T : C_TRI_T);
  t_out = t;
  return true;
}
// The (u, v) rows of g: axTrans rows 1-2 of (o - v0) and of the ray as one packed chain
__device__ __forceinline__ void tri_rows(const TriGeo &g, v3 o, v3 ray, f2 &ao, f2 &ar)
{
  const float dx = o.x - g.v0x, dy = o.y - g.v0y, dz = o.z - g.v0z;
  const f2 c1{g.a11, g.a21}, c2{g.a12, g.a22}, c3{g.a13, g.a23};
  ao = dx * c1 + dy * c2 + dz * c3;                         // (aox, aoy)
  ar = ray.x * c1 + ray.y * c2 + ray.z * c3;                // (arx, ary)
}
// The uv stage, the triangle's own: is the crossing at t inside, and farther than DELTA (Triangle.cpp:91-104)?
template <bool STATS, bool SHADOW>
__device__ __forceinline__ bool tri_uv(f2 ao, f2 ar, v3 ray, float t, float &u_out, float &v_out, float &sq_out, Cnt &cnt)
{
  const f2 uv = ao + t * ar;                                  // (u, v)
  const float u = uv.x, v = uv.y;
  if (!(u >= 0.0f && v >= 0.0f && u + v < 1.0f)) return false;
  RFX_CNT(SHADOW ? C_SH_TRI_IN : C_TRI_IN);
  const float sq = sqlen(mul(ray, t));
  if (!(sq > kDelta * kDelta)) return false;
  u_out = u; v_out = v; sq_out = sq;
  return true;
}

template <bool STATS, bool SHADOW, bool PRE = false>
__device__ __forceinline__ bool tri_hit(const TriGeo &g, v3 o, v3 ray, float &t_out, float &u_out, float &v_out,
                                        float &sq_out, Cnt &cnt, const RayConst &k, float best_sq = INFINITY)
{
  float nz, arz;
  if (!tri_z<STATS, SHADOW>(g, o, ray, k, best_sq, cnt, nz, arz)) return false;
  f2 ao, ar;
  if constexpr (PRE && !STATS)
  {
    tri_rows(g, o, ray, ao, ar);
    // exact reject of a plane crossing outside the triangle before the correctly rounded divide: with t' = nz rcp(arz)
    // (v_rcp_f32: 1 ulp), u' = aox + t' arx is within (|aox| + |t' arx|) 2^-19 of the reference's rounded u (t
    // within 2^-21 relative, three roundings); the margins are 4x that, so u' < -mu means u < 0, and u' + v' above
    // 1 + mu + mv means u + v > 1.  A NaN keeps the triangle.  A wave whose lanes all cross outside skips the divide.
    const f2 pp = (nz * __builtin_amdgcn_rcpf(arz)) * ar;
    const f2 uvp = ao + pp;
    const float mu = (fabsf(ao.x) + fabsf(pp.x)) * 0x1p-17f, mv = (fabsf(ao.y) + fabsf(pp.y)) * 0x1p-17f;
    if (uvp.x < -mu || uvp.y < -mv || uvp.x + uvp.y > 1.0f + (mu + mv) + 0x1p-20f) return false;
  }
  if (!tri_zt<STATS, SHADOW>(nz, arz, t_out, cnt)) return false;
  if constexpr (!(PRE && !STATS)) tri_rows(g, o, ray, ao, ar);
  return tri_uv<STATS, SHADOW>(ao, ar, ray, t_out, u_out, v_out, sq_out, cnt);
}

// Coplanar mates in the small-scene loops (DESIGN.md "Coplanar mates"): the triangle index of those loops is
// wave-uniform, so the group's leader (TriGeo::pad[0], rfx_scene.cpp tri_mate_leaders) is a scalar.  The loop keeps the
// last z stage -- per lane: did it pass, and t -- with its leader; the next kept triangle of the same group goes straight to
// its own (u, v) rows: 9 dwords and the leader instead of 12, and no second divide.  The visits stay in index order; a
// member whose leader was culled runs the z stage itself.  Closest hit: the kept z stage was decided against the best
// distance before the leader's own test, and a stale bound only rejects less; tri_takes settles each member as before.
// RFX_TRI_MATES: 0 off, 1 both loops, 2 closest hit only (the default), 3 shadow only.  tools/ab.py, C3 trace ms against
// the parent's 0.5970: 0.5838 (1), 0.5843 (2), 0.5998 (3) -- the any-hit loop on its own loses (a lane leaves it at its
// first occluder, and its own triangle fails the z stage's DELTA reject before the divide), so it keeps the per-triangle
// test.  STATS kernels keep it too (their event counters are the reference's).
template <bool STATS, bool SHADOW>
struct TriMates {
  static constexpr bool kOn = !STATS && (RFX_TRI_MATES == 1 || RFX_TRI_MATES == (SHADOW ? 3 : 2));
  int lead = -1;
  bool ok = false;
  float t = 0.0f;
  __device__ __forceinline__ bool hit(const TriGeo &g, v3 o, v3 ray, float &t_out, float &u_out, float &v_out,
                                      float &sq_out, Cnt &cnt, const RayConst &k, float best_sq = INFINITY)
  {
    if constexpr (!kOn) return tri_hit<STATS, SHADOW>(g, o, ray, t_out, u_out, v_out, sq_out, cnt, k, best_sq);
    else
    {
      const int l = __builtin_bit_cast(int, g.pad[0]);
      if (l != lead)
      {
        lead = l;
        float nz, arz;
        ok = tri_z<STATS, SHADOW>(g, o, ray, k, best_sq, cnt, nz, arz) && tri_zt<STATS, SHADOW>(nz, arz, t, cnt);
      }
      if (!ok) return false;
      f2 ao, ar;
      tri_rows(g, o, ray, ao, ar);
      t_out = t;
      return tri_uv<STATS, SHADOW>(ao, ar, ray, t, u_out, v_out, sq_out, cnt);
    }
  }
};

// Plane::trace (Plane.cpp:36-73) up to its hit decision; on a hit returns t and |ray t|^2.  a = norm . ray,
// t = norm . (pos - origin) / a, with tri_hit's two exact rejects before the division (opposite signs or a
// zero numerator give t <= 0; a plane hit beyond the closest hit so far cannot win or tie).
template <bool STATS, bool SHADOW>
__device__ __forceinline__ bool plane_hit(const PlaneGeo &g, v3 o, v3 ray, float &t_out, float &sq_out, Cnt &cnt,
                                          const RayConst &k, float best_sq = INFINITY)
{
  RFX_CNT(SHADOW ? C_SH_PLN_TESTS : C_PLN_TESTS);
  const v3 n = mk(g.nx, g.ny, g.nz);
  const float a = dot(n, ray);                                                     // Plane.cpp:41
  if (!(fabsf(a) > kVerySmall)) return false;
  const float num = dot(n, sub(mk(g.px, g.py, g.pz), o));                          // Plane.cpp:40,45
  if (!((num > 0.0f && a > 0.0f) || (num < 0.0f && a < 0.0f))) return false;
  if constexpr (!SHADOW && !STATS)
    if (num * num * k.a2 > best_sq * (a * a) * 2.0000305f) return false;
  const float t = qdiv(num, a);
  if (!(t > kVerySmall)) return false;
  RFX_CNT(SHADOW ? C_SH_PLN_T : C_PLN_T);
  const float sq = sqlen(mul(ray, t));
  if (!(sq > kDelta * kDelta)) return false;                                       // Plane.cpp:50-53
  t_out = t; sq_out = sq;
  return true;
}

// ------------------------------------------------------------- closest hit
// Scene.cpp:86-106: the reference keeps the first object with the minimal distance, i.e. the
// lexicographic minimum of (distance, insertion index); any visiting order gives it.  Distances are
// compared through their squares (dist = sqrt_rn(sq) for both kinds, Sphere.cpp:61-62,
// Triangle.cpp:70-85): for sq < best_sq, dist < best unless both round to the same float, i.e. unless
// sq >= sq_lower_bound(best); for sq >= best_sq, dist >= best (tests/test_sqrt_bounds.py).
struct Hit {
  int obj, kind, i;  // object index (-1: none), 0 sphere / 1 triangle / 2 plane, index within its kind
  float t, u, v, sq;
};

__device__ __forceinline__ bool strictly_closer(float sq, float best_sq)
{
  return sq < best_sq && (best_sq == INFINITY || sq < sq_lower_bound(sqrt_rn(best_sq)));
}

// Outside a 2^-20 band around best_sq the rounded distances are ordered like the squares: sq < RN(best_sq (1 - 2^-20))
// gives sqrt_rn(sq) < sqrt_rn(best_sq), sq > RN(best_sq (1 + 2^-20)) gives sqrt_rn(sq) > sqrt_rn(best_sq) (sqrt_rn and the
// products each round by at most 2^-24 relative; all squares here are normal).  Only candidates inside the band take the
// exact test above (tests/test_sqrt_bounds.py checks both claims).  best_sq = +inf: every finite sq is below.
constexpr float kTakeBelow = 0x1.ffffep-1f;  // 1 - 2^-20
constexpr float kTakeAbove = 0x1.00001p+0f;  // 1 + 2^-20

// the comparison key of a candidate and the two decisions on it (Hit::sq holds the winner's key)
constexpr float kNoHitKey = INFINITY;
__device__ __forceinline__ float hit_key(float sq) { return sq; }
__device__ __forceinline__ bool sph_takes(float sq, float best_sq)
{
  if (sq < best_sq * kTakeBelow) return true;
  return strictly_closer(sq, best_sq);
}
// dist < best || (dist == best && obj < best_obj)
__device__ __forceinline__ bool tri_takes(float sq, float best_sq, int obj, int best_obj)
{
  if (sq < best_sq * kTakeBelow) return true;
  if (!(sq <= best_sq * kTakeAbove)) return false;
  return sq < best_sq ? (obj < best_obj || strictly_closer(sq, best_sq))
                      : (obj < best_obj && sqrt_rn(sq) == sqrt_rn(best_sq));
}

// The winner's record where the candidate's index is wave-uniform (the object loops: a scalar loop counter), written as
// selects under one mask.  As a branch around the stores -- `if (tri_takes(...)) { h.sq = ...; h.i = i; ... }` -- the
// small-scene triangle loop compiled (ROCm 6 clang, gfx950) to code that moved the scalar i into Hit::i before
// tri_takes' 2^-20 band, used that register as scratch inside the band and restored the old Hit::i after it: a
// candidate that took inside the band got every field but i, and the hit was shaded with another triangle's record
// (caller rays from 1e7 away, where every distance lies in the band: tests/test_gpu_edge_rays.py).
__device__ __forceinline__ void hit_take(Hit &h, bool take, float sq, int obj, int kind, int i, float t,
                                         float u = 0.0f, float v = 0.0f)
{
  h.sq = take ? sq : h.sq;
  h.obj = take ? obj : h.obj;
  h.kind = take ? kind : h.kind;
  h.i = take ? i : h.i;
  h.t = take ? t : h.t;
  h.u = take ? u : h.u;
  h.v = take ? v : h.v;
}

}  // namespace rfx
