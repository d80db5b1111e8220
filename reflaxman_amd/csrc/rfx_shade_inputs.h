// rfx_shade_inputs.h -- what shading reads, and how a workgroup stages it.  The per-workgroup LDS tables (glibc powf's
// tables with powf_dev / powf3_dev; a small scene's per-object records, read through Tabs<SMALL>), the workgroup shape
// every table and kernel is sized by (kWgWaves, kWgThreads, kTileW x kTileH, RFX_TRACE_BOUNDS), and the texel lookups:
// Color(ARGB) through the 256-entry table, Texture::getColor (texel_uv), the skybox and a textured triangle.
#pragma once
#include <hip/hip_runtime.h>

#include "rfx_math.h"
#include "rfx_powf.h"
#include "rfx_types.h"
#include "rfx_diag.h"

#pragma clang fp contract(off)

namespace rfx {

// Color(ARGB) (Color.cpp:9-14) through a 256-entry LDS table of float(k) / 255.0f:
// the table holds exactly the quotients the reference computes per channel.
__device__ __forceinline__ col from_argb_lut(uint32_t c, const float *lut)
{
  return mkc(lut[(c >> 16) & 0xFFu], lut[(c >> 8) & 0xFFu], lut[c & 0xFFu]);
}

// glibc powf's tables (rfx_powf.h) copied to LDS by each workgroup: the lookups index them per lane,
// and LDS answers such gathers in ~100 cycles where the constant/global path takes several hundred.
__shared__ double s_powf_log[16][2];
__shared__ uint64_t s_powf_exp[32];
__shared__ double s_powf_add[2][4];

__device__ __forceinline__ void stage_powf_tables()
{
  const uint32_t t = threadIdx.x;
  if (t < 32)
  {
    s_powf_exp[t] = kExp2fTab[t];
    s_powf_log[t >> 1][t & 1u] = kPowfLog2Tab[t >> 1][t & 1u];
    if (t < 8) s_powf_add[t >> 2][t & 3u] = kPowfAdd[t >> 2][t & 3u];
  }
}

__device__ __forceinline__ float powf_dev(float x, float y)
{
  return powf_glibc_t(x, y, s_powf_log, s_powf_exp, s_powf_add);
}

// powf(x, 3) for x in [0, 1] (the Fresnel term): the double cube where it provably rounds like glibc, glibc's
// algorithm for the few lanes where it may not (rfx_powf.h powf_cube_fast)
__device__ __forceinline__ float powf3_dev(float x)
{
  float p;
  if (!powf_cube_fast(x, p)) p = powf_dev(x, 3.0f);
  return p;
}

// Small scenes (<= 32 spheres, <= 32 triangles): the per-object records the hit lanes gather by their
// own object index (winner geometry and material, the cull lane table) staged in LDS per workgroup.
__shared__ SphereGeo s_sph_geo[32];
__shared__ MatRec s_sph_mat[32];
__shared__ int32_t s_sph_info[64];
__shared__ TriShade s_tri_shade[32];
__shared__ MatRec s_tri_mat[32];
__shared__ CullRec s_cull[64];

template <bool SMALL>
struct Tabs {
  const DevScene &S;
  __device__ __forceinline__ SphereGeo sph_geo(int i) const { return S.sph_geo[i]; }
  __device__ __forceinline__ MatRec sph_mat(int i) const { return S.sph_mat[i]; }
  __device__ __forceinline__ int32_t sph_info(int k) const { return S.sph_info[k]; }
  __device__ __forceinline__ TriShade tri_shade(int i) const { return S.tri_shade[i]; }
  __device__ __forceinline__ MatRec tri_mat(int i) const { return S.tri_mat[i]; }
  __device__ __forceinline__ const CullRec *cull() const { return S.cull_small; }
};
template <>
struct Tabs<true> {
  const DevScene &S;
  __device__ __forceinline__ SphereGeo sph_geo(int i) const { return s_sph_geo[i]; }
  __device__ __forceinline__ MatRec sph_mat(int i) const { return s_sph_mat[i]; }
  __device__ __forceinline__ int32_t sph_info(int k) const { return s_sph_info[k]; }
  __device__ __forceinline__ TriShade tri_shade(int i) const { return s_tri_shade[i]; }
  __device__ __forceinline__ MatRec tri_mat(int i) const { return s_tri_mat[i]; }
  __device__ __forceinline__ const CullRec *cull() const { return s_cull; }
};

__device__ __forceinline__ void stage_small_scene(const DevScene &S)
{
  const int t = (int)threadIdx.x;
  if (t < S.n_sph)
  {
    s_sph_geo[t] = S.sph_geo[t];
    s_sph_mat[t] = S.sph_mat[t];
    s_sph_info[2 * t] = S.sph_info[2 * t];
    s_sph_info[2 * t + 1] = S.sph_info[2 * t + 1];
  }
  if (t < S.n_tri)
  {
    s_tri_shade[t] = S.tri_shade[t];
    s_tri_mat[t] = S.tri_mat[t];
  }
  if (t < 64) s_cull[t] = S.cull_small[t];
}

// 7 waves per SIMD (<= 72 VGPRs, a few spills): the kernel is VALU-issue bound; more waves hide the
// scene-load and texel latencies better than spills cost (tools/ab.py, C3 trace kernel: 6 -> 7 -2.6%;
// 8 waves / 64 VGPRs spill enough to lose 4-7%)
// waves per workgroup (1, 2 or 4): a wave is an 8x8 pixel tile, a workgroup 8x8 / 16x8 / 16x16 pixels.
// Two: a workgroup's slots free when its slower wave ends, and the per-workgroup LDS staging stays cheap
// (tools/ab.py, C3 trace kernel: 4 -> 2 waves -2.5%, 1 wave +3.6%)
constexpr uint32_t kWgWaves = RFX_WG_WAVES, kWgThreads = 64 * kWgWaves;
constexpr uint32_t kTileWavesX = kWgWaves >= 2 ? 2 : 1, kTileWavesY = kWgWaves / kTileWavesX;
constexpr uint32_t kTileW = 8 * kTileWavesX, kTileH = 8 * kTileWavesY;
static_assert(kWgWaves == 1 || kWgWaves == 2 || kWgWaves == 4, "RFX_WG_WAVES: 1, 2 or 4");
#define RFX_TRACE_BOUNDS __launch_bounds__(kWgThreads) __attribute__((amdgpu_waves_per_eu(RFX_WAVES_PER_EU)))

// ------------------------------------------------------------- sampling
template <bool STATS>
__device__ __forceinline__ col texel_uv(const DevScene &S, int tex, float u, float v, const float *lut, Cnt &cnt)
{                                                                         // Texture.cpp:231-269
  if (u < 0.0f || u > 1.0f || v < 0.0f || v > 1.0f) { RFX_CNT(C_TEX_OTHER); return mkc(0.0f, 0.0f, 0.0f); }
  TexRec t;
  t.w = 0; t.h = 0; t.offset = 0;
  if (tex >= 0) t = S.texs[tex];
  if (t.w == 0)
  {
    RFX_CNT(C_TEX_CHECKER);
    return (((int)(u * 50) % 2) ^ ((int)(v * 50) % 2)) ? mkc(0.5f, 0.5f, 0.5f) : mkc(0.75f, 0.75f, 0.75f);
  }
  const float fx = clampf(u, 0.0f, 1.0f - kFltEpsilon) * (float)t.w;
  const float fy = clampf(v, 0.0f, 1.0f - kFltEpsilon) * (float)t.h;
  const uint32_t x = (uint32_t)fx, y = (uint32_t)fy;
  const uint32_t *px = S.texels + t.offset;
  if (x < t.w - 1 && y < t.h - 1)
  {
    RFX_CNT(C_TEX_BILINEAR);
    const col c00 = from_argb_lut(px[x + t.w * y], lut), c01 = from_argb_lut(px[x + t.w * (y + 1)], lut);
    const col c10 = from_argb_lut(px[x + 1 + t.w * y], lut), c11 = from_argb_lut(px[x + 1 + t.w * (y + 1)], lut);
    const float uf = fx - floorf(fx), vf = fy - floorf(fy);
    const float uo = 1 - uf, vo = 1 - vf;
    return cadd(cscale(cadd(cscale(c00, uo), cscale(c10, uf)), vo), cscale(cadd(cscale(c01, uo), cscale(c11, uf)), vf));
  }
  RFX_CNT(C_TEX_OTHER);
  const uint32_t xi = (uint32_t)fx, yi = (uint32_t)fy;                 // Texture.cpp:216-229
  if (xi >= t.w || yi >= t.h) return mkc(0.0f, 0.0f, 0.0f);
  return from_argb_lut(px[xi + t.w * yi], lut);
}

template <bool STATS>
__device__ __forceinline__ col skybox_texel(const DevScene &S, v3 ray, const float *lut, Cnt &cnt)  // Skybox.cpp:39-106
{
  const float uLeft = 1.0f / 8.0f, vLeft = 3.0f / 6.0f;
  const float uFront = 3.0f / 8.0f, vFront = 3.0f / 6.0f;
  const float uRight = 5.0f / 8.0f, vRight = 3.0f / 6.0f;
  const float uBack = 7.0f / 8.0f, vBack = 3.0f / 6.0f;
  const float uTop = 3.0f / 8.0f, vTop = 5.0f / 6.0f;
  const float uBottom = 3.0f / 8.0f, vBottom = 1.0f / 6.0f;
  const float hw = S.half_tile_w, hh = S.half_tile_h;
  const v3 n = normalized(ray);
  const float x = n.x, y = n.y, z = n.z;
  const float ax = fabsf(x) + kVerySmall, ay = fabsf(y) + kVerySmall, az = fabsf(z) + kVerySmall;
  // the face's two quotients share their divisor (rfx_math.h div_fast_unit): u0 -/+ p / den * hw, v0 -/+ q / den * hh
  float u0, v0, p, q, den, su, sv;
  if (az >= ax && az >= ay)
  {
    den = az;
    if (z > 0) { u0 = uFront; v0 = vFront; p = x; q = y; su = 1.0f; sv = 1.0f; }
    else { u0 = uBack; v0 = vBack; p = x; q = y; su = -1.0f; sv = 1.0f; }
  }
  else if (ax >= ay && ax >= az)
  {
    den = ax;
    if (x > 0) { u0 = uRight; v0 = vRight; p = z; q = y; su = -1.0f; sv = 1.0f; }
    else { u0 = uLeft; v0 = vLeft; p = z; q = y; su = 1.0f; sv = 1.0f; }
  }
  else
  {
    den = ay;
    if (y > 0) { u0 = uTop; v0 = vTop; p = x; q = z; su = 1.0f; sv = -1.0f; }
    else { u0 = uBottom; v0 = vBottom; p = x; q = z; su = 1.0f; sv = 1.0f; }
  }
  // den in [2^-63, 1 + 2^-63] and |p|, |q| <= den: div_fast_unit's bounds
  const float rden = rcp_refined(den);
  bool okp, okq;
  float pd = div_fast_unit(p, den, rden, okp), qd = div_fast_unit(q, den, rden, okq);
  if (__builtin_expect(!(okp && okq), 0)) { pd = p / den; qd = q / den; }
  // u0 + p / den * hw, or u0 - (p / den * hw): a subtraction of the product, as the reference writes it
  const float pu = pd * hw, qv = qd * hh;
  const float u = su > 0.0f ? u0 + pu : u0 - pu, v = sv > 0.0f ? v0 + qv : v0 - qv;
  return texel_uv<STATS>(S, S.skybox_tex, u, v, lut, cnt);
}

// A textured triangle's material colour at barycentrics (u, v) (Triangle.cpp:89-96): tuvTrans * (u, v, 0)
// (whose _13 and _23 are 0) offset by (tu[0], tv[0]).
template <bool STATS>
__device__ __forceinline__ col tri_texel(const DevScene &S, const TriShade &sh, float u, float v, const float *lut,
                                         Cnt &cnt)
{
  const float tvx = u * sh.t11 + v * sh.t12 + 0.0f;
  const float tvy = u * sh.t21 + v * sh.t22 + 0.0f;
  return texel_uv<STATS>(S, sh.tex, sh.tu0 + tvx, sh.tv0 + tvy, lut, cnt);
}

}  // namespace rfx
