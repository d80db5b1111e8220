// rfx_bundle.h -- the wave's live rays as one cone (Bundle: make_bundle, make_bundle_ball for a light's shadow rays,
// make_bundle_quad for a pixel's sample rectangle) and the exact culls against it: cull_chunk (64 bounding spheres, a
// lane each), cull_small (a small scene's lane-layout records, optionally with the triangle footprint test), and the
// mask helpers all_bits / pair_bits.  The Bundle, kCullRel -- the margin every cull and the BVH boxes share -- and the
// verdict on one lane record come from rfx_cull_rule.h, which the host includes too.  wave_or: a mask ORed over the wave.
#pragma once
#include <hip/hip_runtime.h>

#include "rfx_cull_rule.h"
#include "rfx_math.h"
#include "rfx_types.h"

#pragma clang fp contract(off)

namespace rfx {

__device__ __forceinline__ float lane_bcast(float v, int lane)
{
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// max over the wave of a value >= 0 (every lane active): the bit patterns of non-negative floats order
// like the floats, and a NaN pattern (above +inf) wins, which makes the bound unusable below.
// DPP inclusive max-scan within each 16-lane row (row_shr 1, 2, 4, 8), then across rows (row_bcast 15,
// row_bcast 31): lane 63 ends with the wave's maximum.  Lanes a shift leaves without a source keep 0.
__device__ __forceinline__ float wave_max_nonneg(float v)
{
  uint32_t u = __float_as_uint(v);
  u = max(u, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x111, 0xf, 0xf, false));  // row_shr:1
  u = max(u, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x112, 0xf, 0xf, false));  // row_shr:2
  u = max(u, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x114, 0xf, 0xf, false));  // row_shr:4
  u = max(u, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x118, 0xf, 0xf, false));  // row_shr:8
  u = max(u, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x142, 0xa, 0xf, false));  // row_bcast:15
  u = max(u, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x143, 0xc, 0xf, false));  // row_bcast:31
  return __int_as_float(__builtin_amdgcn_readlane((int)u, 63));
}

// OR over the wave of a 64-bit mask (every lane active): wave_max_nonneg's DPP chain on each half, lanes a shift leaves
// without a source contribute 0.
__device__ __forceinline__ uint32_t wave_or32(uint32_t u)
{
  u |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x111, 0xf, 0xf, false);  // row_shr:1
  u |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x112, 0xf, 0xf, false);  // row_shr:2
  u |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x114, 0xf, 0xf, false);  // row_shr:4
  u |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x118, 0xf, 0xf, false);  // row_shr:8
  u |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x142, 0xa, 0xf, false);  // row_bcast:15
  u |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x143, 0xc, 0xf, false);  // row_bcast:31
  return (uint32_t)__builtin_amdgcn_readlane((int)u, 63);
}
__device__ __forceinline__ uint64_t wave_or(uint64_t m)
{
  return (uint64_t)wave_or32((uint32_t)(m >> 32)) << 32 | wave_or32((uint32_t)m);
}

// Bundle of the rays (o, d) of the `live` lanes.  Call with every lane of the wave active and at least
// one live lane.  Approximate square roots are fine here: every bound is widened well past their error.
__device__ __forceinline__ Bundle make_bundle(v3 o, v3 d, bool live)
{
  Bundle B;
  const int ref = __ffsll((long long)__ballot(live)) - 1;
  B.cx = lane_bcast(o.x, ref); B.cy = lane_bcast(o.y, ref); B.cz = lane_bcast(o.z, ref);
  const float dx = lane_bcast(d.x, ref), dy = lane_bcast(d.y, ref), dz = lane_bcast(d.z, ref);
  const float inv = __builtin_amdgcn_rsqf(cdot(dx, dy, dz, dx, dy, dz));
  B.ax = dx * inv; B.ay = dy * inv; B.az = dz * inv;
  const float ex = o.x - B.cx, ey = o.y - B.cy, ez = o.z - B.cz;
  const float e2 = cdot(ex, ey, ez, ex, ey, ez);
  const float cosl = cdot(d.x, d.y, d.z, B.ax, B.ay, B.az) * __builtin_amdgcn_rsqf(cdot(d.x, d.y, d.z, d.x, d.y, d.z));
  const float dev = 1.0f - cosl;
  // a live lane with a non-finite or degenerate ray disables the bound for the whole wave
  const bool bad = live && !(e2 <= 1.0e30f && dev >= -0.5f && dev <= 2.5f);
  const float e2m = wave_max_nonneg(live ? e2 : 0.0f);
  const float devm = wave_max_nonneg(live ? fmaxf(dev, 0.0f) : 0.0f);
  B.rw = __builtin_amdgcn_sqrtf(e2m) * 1.0001f;
  B.cosa = 1.0f - devm - 4e-6f;                                                // approximate cosines: widen
  B.sina = __builtin_amdgcn_sqrtf(fmaxf(1.0f - B.cosa * B.cosa, 0.0f) + 1e-7f) * 1.001f;
  B.ok = __ballot(bad) == 0 && B.cosa > 0.1f && B.rw <= 1.0e15f;
  return B;
}

// Bundle of every ray (o, d + rd R) with |rd| <= 1 of the `live` lanes (the shadow rays toward a light of radius R
// for any randDir, Scene.cpp:128-129): make_bundle's cone widened per lane by the angular radius asin(R / |d|) of
// the direction ball, cos(alpha + beta) = cos a cos b - sin a sin b.  A lane whose ball reaches its own origin's
// side (R >= |d| / 2) disables the bound.  For the per-view primary shadow masks (prim_cull_kernel).
__device__ __forceinline__ Bundle make_bundle_ball(v3 o, v3 d, float R, bool live)
{
  Bundle B;
  const int ref = __ffsll((long long)__ballot(live)) - 1;
  B.cx = lane_bcast(o.x, ref); B.cy = lane_bcast(o.y, ref); B.cz = lane_bcast(o.z, ref);
  const float dx = lane_bcast(d.x, ref), dy = lane_bcast(d.y, ref), dz = lane_bcast(d.z, ref);
  const float inv = __builtin_amdgcn_rsqf(dx * dx + dy * dy + dz * dz);
  B.ax = dx * inv; B.ay = dy * inv; B.az = dz * inv;
  const float ex = o.x - B.cx, ey = o.y - B.cy, ez = o.z - B.cz;
  const float e2 = ex * ex + ey * ey + ez * ez;
  const float d2 = d.x * d.x + d.y * d.y + d.z * d.z;
  const float id = __builtin_amdgcn_rsqf(d2);
  const float ca = fminf((d.x * B.ax + d.y * B.ay + d.z * B.az) * id, 1.0f);      // cos alpha (approximate)
  const float sa = __builtin_amdgcn_sqrtf(fmaxf(1.0f - ca * ca, 0.0f));
  const float sb = fminf(R * id * 1.001f, 1.0f), cb = __builtin_amdgcn_sqrtf(fmaxf(1.0f - sb * sb, 0.0f));
  const float cosl = ca * cb - sa * sb;
  const float dev = 1.0f - cosl;
  const bool bad = live && !(e2 <= 1.0e30f && dev >= -0.5f && dev <= 2.5f && sb < 0.5f);
  const float e2m = wave_max_nonneg(live ? e2 : 0.0f);
  const float devm = wave_max_nonneg(live ? fmaxf(dev, 0.0f) : 0.0f);
  B.rw = __builtin_amdgcn_sqrtf(e2m) * 1.0001f;
  B.cosa = 1.0f - devm - 4e-6f;                                                // approximate cosines: widen
  B.sina = __builtin_amdgcn_sqrtf(fmaxf(1.0f - B.cosa * B.cosa, 0.0f) + 1e-7f) * 1.001f;
  B.ok = __ballot(bad) == 0 && B.cosa > 0.1f && B.rw <= 1.0e15f;
  return B;
}

// Bundle of the shadow rays (o, L + rd R), |rd| <= 1, of the `live` lanes toward a far light (rfx_types.h LightRec,
// near > 0; every live lane's o inside the light's bound, so its direction is L + rd R with the light's own origin L):
// origin and rw as make_bundle finds them, the cone a constant of the light -- its axis normalized(L), its half-angle
// the ball's angular radius asin(R / |L|), widened on the host as make_bundle_ball widens its own (which also covers
// the rounding of L + rd R, a relative 2^-23 of |L|).  The cone make_bundle would find has the first live lane's ray as
// its axis, so its half-angle reaches twice this one's.
__device__ __forceinline__ Bundle make_bundle_far(v3 o, const LightRec &L, bool live)
{
  Bundle B;
  const int ref = __ffsll((long long)__ballot(live)) - 1;
  B.cx = lane_bcast(o.x, ref); B.cy = lane_bcast(o.y, ref); B.cz = lane_bcast(o.z, ref);
  B.ax = L.ndx; B.ay = L.ndy; B.az = L.ndz;
  const float ex = o.x - B.cx, ey = o.y - B.cy, ez = o.z - B.cz;
  const float e2 = cdot(ex, ey, ez, ex, ey, ez);
  const bool bad = live && !(e2 <= 1.0e30f);
  const float e2m = wave_max_nonneg(live ? e2 : 0.0f);
  B.rw = __builtin_amdgcn_sqrtf(e2m) * 1.0001f;
  B.cosa = L.cone_cos;
  B.sina = L.cone_sin;
  B.ok = __ballot(bad) == 0 && B.rw <= 1.0e15f;
  return B;
}

// Bundle of every ray from o with a direction in the quadrilateral d[0..3] of each `live` lane (the sample rays of an SSAA
// pixel: the directions are a linear image of the pixel's sample rectangle, and the cone is convex, so a cone
// holding the four corners holds every ray between them).  For the per-view masks of SSAA frames (prim_cull_kernel).
__device__ __forceinline__ Bundle make_bundle_quad(v3 o, const v3 (&d)[4], bool live)
{
  Bundle B;
  const int ref = __ffsll((long long)__ballot(live)) - 1;
  B.cx = lane_bcast(o.x, ref); B.cy = lane_bcast(o.y, ref); B.cz = lane_bcast(o.z, ref);
  const float dx = lane_bcast(d[0].x, ref), dy = lane_bcast(d[0].y, ref), dz = lane_bcast(d[0].z, ref);
  const float inv = __builtin_amdgcn_rsqf(dx * dx + dy * dy + dz * dz);
  B.ax = dx * inv; B.ay = dy * inv; B.az = dz * inv;
  const float ex = o.x - B.cx, ey = o.y - B.cy, ez = o.z - B.cz;
  const float e2 = ex * ex + ey * ey + ez * ez;
  float dev = 0.0f;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < 4; ++k)
  {
    const v3 v = d[k];
    const float cosl = (v.x * B.ax + v.y * B.ay + v.z * B.az) * __builtin_amdgcn_rsqf(v.x * v.x + v.y * v.y + v.z * v.z);
    const float dk = 1.0f - cosl;
    bad = bad || !(dk >= -0.5f && dk <= 2.5f);
    dev = fmaxf(dev, dk);
  }
  bad = live && (bad || !(e2 <= 1.0e30f));
  const float e2m = wave_max_nonneg(live ? e2 : 0.0f);
  const float devm = wave_max_nonneg(live ? fmaxf(dev, 0.0f) : 0.0f);
  B.rw = __builtin_amdgcn_sqrtf(e2m) * 1.0001f;
  B.cosa = 1.0f - devm - 4e-6f;                                                // approximate cosines: widen
  B.sina = __builtin_amdgcn_sqrtf(fmaxf(1.0f - B.cosa * B.cosa, 0.0f) + 1e-7f) * 1.001f;
  B.ok = __ballot(bad) == 0 && B.cosa > 0.1f && B.rw <= 1.0e15f;
  return B;
}

// Bit l: object first + l (l < n <= 64) of the bounding-sphere array may be hit by a ray of the bundle.
// Call with every lane of the wave active.  Cone test: the ray set meets the grown sphere (centre at
// distance L, radius rp) only if the angle between (centre - c) and the axis is at most
// acos(cosa) + asin(rp / L), i.e. va >= cosa sqrt(L^2 - rp^2) - sina rp.
__device__ __forceinline__ uint64_t cull_chunk(const Bound *bound, int first, int n, const Bundle &B)
{
  const int l = (int)(threadIdx.x & 63u);
  bool keep = false;
  if (l < n)
  {
    const Bound g = bound[first + l];
    const float vx = g.x - B.cx, vy = g.y - B.cy, vz = g.z - B.cz;
    const float L2 = cdot(vx, vy, vz, vx, vy, vz);
    const float L = __builtin_amdgcn_sqrtf(L2);
#if RFX_CULL_FMA
    const float rp = __builtin_fmaf(kCullRel, L + B.rw, g.r + B.rw);
    const float va = cdot(vx, vy, vz, B.ax, B.ay, B.az);
    const float lim = __builtin_fmaf(B.cosa, __builtin_amdgcn_sqrtf(fmaxf(__builtin_fmaf(-rp, rp, L2), 0.0f)), -(B.sina * rp));
#else
    const float rp = g.r + B.rw + kCullRel * (L + B.rw);
    const float va = cdot(vx, vy, vz, B.ax, B.ay, B.az);
    const float lim = B.cosa * __builtin_amdgcn_sqrtf(fmaxf(L2 - rp * rp, 0.0f)) - B.sina * rp;
#endif
    keep = !(L > rp && va < lim);
  }
  return __ballot(keep);
}

// Triangle footprint (primary bundles, prim_cull_kernel): when every origin lies more than rw (plus a margin) on
// one side of the plane and every direction heads into it (the cone's least cosine to the normal, ndmin, at
// least 0.1), the crossing points lie in a disk around the axis ray's crossing P0 of radius
//   R = h chord (1 + 1 / an) / ndmin + rw (1 + 1 / ndmin)
// (h: the bundle centre's height over the plane, an: the axis's cosine to the normal, chord = |dir - axis| <=
// sqrt(2 - 2 cosa): |dir / (n.dir) - a / (n.a)| <= |dir - a| (1 + 1 / n.a) / n.dir, and an origin offset d moves
// a crossing by at most |d| (1 + 1 / n.dir)).  If that disk lies outside the triangle in (u, v) -- u or v below
// 0, or u + v above 1, by more than R |gu|, R |gv|, R |gu + gv| -- no ray of the bundle can hit it.  Margins
// cover the reference's float (u, v): its inverse basis and its t differ from the exact ones by a relative
// ~150 eps for cond < 100 (the host's gate, rfx_scene.cpp), amplified at most 10x by 1 / ndmin; the margins are 1e-2 of |g|
// times the distances involved (|o - v0| plus the travel to the plane).  Measured: tests/test_bundle_cull_bound.py (footprint).
__device__ __forceinline__ bool tri_footprint_misses(const CullTri &q, float side, float an, const Bundle &B)
{
  const float h = fabsf(side), anp = side > 0.0f ? -an : an;  // height, cosine of the axis into the plane
  const float snp = __builtin_amdgcn_sqrtf(fmaxf(1.0f - anp * anp, 0.0f));
  const float ndmin = anp * B.cosa - snp * B.sina;
  if (!(h > B.rw * 1.01f + 1e-4f && ndmin > 0.1f)) return false;
  const float ind = __builtin_amdgcn_rcpf(ndmin) * 1.001f, ian = __builtin_amdgcn_rcpf(anp) * 1.001f;
  const float tp = h * ian * (1.0f / 1.001f);                 // travel of the axis ray to the plane (approximate)
  const float px = B.cx + tp * B.ax - q.v0x, py = B.cy + tp * B.ay - q.v0y, pz = B.cz + tp * B.az - q.v0z;
  const float chord = __builtin_amdgcn_sqrtf(fmaxf(2.0f - 2.0f * B.cosa, 0.0f)) * 1.001f;
  const float R = (h * chord * (1.0f + ian) * ind + B.rw * (1.0f + ind) + 1e-4f * tp) * 1.001f + 1e-6f;
  // distances the reference's rounding scales with: |o - v0| <= |c - v0| + rw, travel <= (h + rw) / ndmin
  const float cvx = B.cx - q.v0x, cvy = B.cy - q.v0y, cvz = B.cz - q.v0z;
  const float mag = __builtin_amdgcn_sqrtf(cvx * cvx + cvy * cvy + cvz * cvz) * 1.001f + B.rw + (h + B.rw) * ind;
  const float m = 1e-2f * mag + 1e-6f;
  const float u0 = q.gux * px + q.guy * py + q.guz * pz, v0 = q.gvx * px + q.gvy * py + q.gvz * pz;
  return u0 + (R + m) * q.nu < 0.0f || v0 + (R + m) * q.nv < 0.0f ||
         u0 + v0 - R * q.nuv - m * (q.nu + q.nv) > 1.0f;
}

// Small scenes: lane l tests cull record l (rfx_types.h CullRec) by rfx_cull_rule.h cull_record -- the cone test of
// cull_chunk, and for a triangle also its plane.  FOOT (the primary masks only): the footprint test above.
// Bits of lanes without an object are cleared.
template <bool FOOT = false>
__device__ __forceinline__ uint64_t cull_small(const CullRec *tab, uint64_t valid, const Bundle &B,
                                               const CullTri *ttab = nullptr)
{
  const CullVerdict v = cull_record(tab[threadIdx.x & 63u], B);
  bool keep = v.keep;
  if constexpr (FOOT)
    if ((threadIdx.x & 63u) >= 32u && keep) keep = !tri_footprint_misses(ttab[(threadIdx.x & 63u) - 32u], v.side, v.an, B);
  return __ballot(keep) & valid;
}

__device__ __forceinline__ uint64_t all_bits(int n) { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); }

// sphere bits (2q, 2q+1) -> pair bit q
__device__ __forceinline__ uint32_t pair_bits(uint64_t m)
{
  uint64_t x = (m | (m >> 1)) & 0x5555555555555555ull;
  x = (x | (x >> 1)) & 0x3333333333333333ull;
  x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
  x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
  x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
  return (uint32_t)x;
}

}  // namespace rfx
