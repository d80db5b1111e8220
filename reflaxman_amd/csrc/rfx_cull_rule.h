// rfx_cull_rule.h -- the bundle cull's decision for one small-scene lane record, in one form for both sides: the
// kernels (rfx_bundle.h cull_small) run it a lane per record, the host (rfx_scene.cpp shadow_grid_build) runs it per
// cell of a far light's occluder grid.  With it: the Bundle it tests against, kCullRel, and cdot.  No HIP here beyond
// the qualifiers rfx_math.h's RFX_HD stands for: a plain C++ compiler builds rfx_scene.cpp with this.
#pragma once
#include "rfx_math.h"
#include "rfx_types.h"

#pragma clang fp contract(off)

namespace rfx {

// ------------------------------------------------------------- wave ray bundles (exact culling)
// The live rays of a wave form a bundle: origins within rw of (cx, cy, cz) -- the first live lane's
// origin -- and directions within the half-angle acos(cosa) of that lane's direction (ax, ay, az).
// A ray the reference's float test reports as hitting a sphere passes within r + 1.25e-3 |o - c| of the
// centre (rounding of d = b^2 - 4ac is at most 104 u a |vco|^2, DESIGN.md "Exact work skipping"; observed worst
// 7.6e-5, tests/test_cull_bound.py); kCullRel = 2e-3 covers the bound 1.6 times (round 2 used 4e-3: C5 trace -7%
// with 2e-3, tools/ab.py), so an object whose bounding sphere, grown by rw and kCullRel (L + rw), lies outside the bundle's cone
// is missed by every lane of the wave and its exact test is skipped for the whole wave.  Skipping a test
// that misses changes no result: the closest hit and the any-hit only ever take hits.  Every cull
// decision is a conjunction of comparisons, so a NaN anywhere keeps the object.
constexpr float kCullRel = 2e-3f;

struct Bundle {
  float cx, cy, cz, rw;
  float ax, ay, az, cosa, sina;
  bool ok;  // wave-uniform: the bound is finite and the cone narrower than ~84 degrees
};

// The bounds' square roots: approximate on the device (v_sqrt_f32, within 1 ulp), sqrtf on the host -- every bound is
// widened well past either's error.
RFX_HD float cull_sqrt(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_sqrtf(x);
#else
  return sqrtf(x);
#endif
}

// Sums of products in the bundle and cull bounds (RFX_CULL_FMA): these are conservative decisions with margins far above
// a rounding, not reference values, so they may fuse their multiply-adds.
RFX_HD float cdot(float ax, float ay, float az, float bx, float by, float bz)
{
#if RFX_CULL_FMA
  return __builtin_fmaf(az, bz, __builtin_fmaf(ay, by, ax * bx));
#else
  return ax * bx + ay * by + az * bz;
#endif
}

// Cull record g (rfx_types.h CullRec) against bundle B: the cone test -- the ray set meets the grown sphere (centre at
// distance L, radius rp) only if the angle between (centre - c) and the axis is at most acos(cosa) + asin(rp / L), i.e.
// va >= cosa sqrt(L^2 - rp^2) - sina rp -- and for a triangle also its plane: when every origin lies more than rw
// (plus a margin) on one side and every direction leaves that side (axis . n beyond sin of the cone's half-angle, plus
// a margin), every ray has t <= 0 for the plane.  The reference's float test then sees -ao.z and ar.z of opposite signs
// too: for a basis with cond <= 1000 their rounding error stays below 2e-4 of |o - v0| and |ray|, inside the 1e-3
// margins (measured with the record's own rounding: tests/test_bundle_cull_bound.py).  A sphere's or an empty lane's
// plane is zero and never says away.  side, an: the bundle centre's height over the plane and the axis's cosine to the
// normal, for the footprint test.
struct CullVerdict { bool keep; float side, an; };
RFX_HD CullVerdict cull_record(const CullRec &g, const Bundle &B)
{
  const float vx = g.x - B.cx, vy = g.y - B.cy, vz = g.z - B.cz;
  const float L2 = cdot(vx, vy, vz, vx, vy, vz);
  const float L = cull_sqrt(L2);
#if RFX_CULL_FMA
  const float rp = __builtin_fmaf(kCullRel, L + B.rw, g.r + B.rw);
  const float va = cdot(vx, vy, vz, B.ax, B.ay, B.az);
  const float lim = __builtin_fmaf(B.cosa, cull_sqrt(fmaxf(__builtin_fmaf(-rp, rp, L2), 0.0f)), -(B.sina * rp));
#else
  const float rp = g.r + B.rw + kCullRel * (L + B.rw);
  const float va = cdot(vx, vy, vz, B.ax, B.ay, B.az);
  const float lim = B.cosa * cull_sqrt(fmaxf(L2 - rp * rp, 0.0f)) - B.sina * rp;
#endif
  CullVerdict v;
  v.side = cdot(g.nx, g.ny, g.nz, B.cx, B.cy, B.cz) - g.d;
  v.an = cdot(g.nx, g.ny, g.nz, B.ax, B.ay, B.az);
  const float ms = B.rw + 1e-3f * (L + g.r + B.rw) + 1e-6f, ma = B.sina + 1e-3f;
  const bool away = (v.side > ms && v.an > ma) || (v.side < -ms && v.an < -ma);
  v.keep = !(L > rp && va < lim) && !away;
  return v;
}

// ------------------------------------------------------------- a far light's occluder grid (DESIGN.md "Shadow grid")
// Cell of point p in the grid G (rfx_types.h ShadowGrid), as the kernels and the host's tests compute it: float32, one
// subtraction and one product per axis, the range test on the floats (a NaN or a point outside the box fails it).
// *cell = (iz ny + iy) nx + ix.  The three roundings move the computed coordinate by at most 2^-22 n cells on an axis of
// n cells, which the cells' widened balls cover (rfx_scene.cpp shadow_grid_build).
RFX_HD bool shadow_grid_cell(const ShadowGrid &G, float px, float py, float pz, int32_t *cell)
{
  const float fx = (px - G.ox) * G.scale, fy = (py - G.oy) * G.scale, fz = (pz - G.oz) * G.scale;
  // (one conjunction of six compares, not a chain of branches)
  const bool in = (fx >= 0.0f) & (fx < G.fnx) & (fy >= 0.0f) & (fy < G.fny) & (fz >= 0.0f) & (fz < G.fnz);
  *cell = in ? ((int32_t)fz * G.ny + (int32_t)fy) * G.nx + (int32_t)fx : 0;
  return in;
}

}  // namespace rfx
