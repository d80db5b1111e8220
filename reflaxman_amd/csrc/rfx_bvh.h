// rfx_bvh.h -- the per-ray BVH walks of the non-small scenes: where a walker reads nodes and keeps its stack (BvhGlobal:
// global nodes, the workgroup's s_bvh_stack; BvhLds: nodes staged in LDS by bounce_kernel_lds), the slab test (RayInv,
// ray_inv, bvh_box) and the four walkers -- closest hit and any-hit over the sphere-pair tree, and, with RFX_TRI_BVH,
// over the triangle tree.
#pragma once
#include <hip/hip_runtime.h>

#include "rfx_types.h"
#include "rfx_shade_inputs.h"
#include "rfx_intersect.h"
#include "rfx_bundle.h"

#pragma clang fp contract(off)

namespace rfx {

// ------------------------------------------------------------- large scenes: per-ray pair BVH
// Each lane walks the pair BVH (rfx_types.h BvhNode) with its own ray: both children's boxes are tested per
// step, the nearer one is entered first and the farther one pushed on a per-lane stack in LDS.  The boxes are
// widened per ray by the exact-cull margin of the wave bundles (a sphere the reference's float test reports as
// hit lies within r + 1.25e-3 |o - c| of the ray; kCullRel = 2e-3 covers it 1.6 times, with |o - c| bounded
// by the distance to the box centre plus its half-diagonal), so a box the ray misses holds no sphere the
// reference could report: skipping it changes no result.  Closest hit: a child whose entry distance exceeds
// the best hit so far (with 0.1% slack over rounding; sphere distances computed by the reference are at least
// the entry distance into their widened box) cannot win or tie and is skipped too.  Leaves run the exact
// pair test with the (distance, object index) rule, so the visiting order changes no result.  The stack holds kBvhStack
// (rfx_types.h) levels: the host builds no deeper hierarchy (rfx_scene.cpp: such a scene falls back to the chunk loops).
constexpr float kNarrowBundleCos = RFX_NARROW_BUNDLE_COS;
// Stack slots: int16 node / ~pair indices (the host builds no BVH for 32768 or more nodes or pairs).  Halving the
// stack's LDS against int32 slots (8 -> 4 KB per workgroup) made C5 6.3% faster (tools/ab.py, round 2): workgroups
// holding less LDS fit the CU's LDS with more slack as they finish out of order.
typedef int16_t BvhSlot;
__shared__ BvhSlot s_bvh_stack[kBvhStack * kWgThreads];

// Where the BVH walkers read nodes and keep their per-lane stacks: the scene's node array in global memory and the
// workgroup's LDS stack (kernels of kWgThreads threads), or -- the LDS-staged bounce kernel (RFX_LDS_BVH) -- node
// boxes and links staged in the workgroup's LDS by its kLdsBvhThreads threads.
constexpr int kLdsBvhThreads = 64 * kLdsBvhWaves;
static_assert(kLdsBvhStackSlots == kBvhStack, "rfx_types.h lds_bvh_bytes sizes the stacks");
struct BvhGlobal {
  static constexpr int kStride = kWgThreads;
  __device__ __forceinline__ BvhNode node(const DevScene &S, int i) const { return S.bvh[i]; }
  __device__ __forceinline__ BvhSlot *stack() const { return s_bvh_stack + threadIdx.x; }
};
struct BvhLds {
  const float4 *box;  // 3 per node: the first 48 B of BvhNode (both children's boxes)
  const uint2 *aux;   // DevScene::bvh_aux
  BvhSlot *stk;
  float mstep;
  static constexpr int kStride = kLdsBvhThreads;
  __device__ __forceinline__ BvhNode node(const DevScene &, int i) const
  {
    BvhNode n;
    const float4 a = box[3 * i], b = box[3 * i + 1], c = box[3 * i + 2];
    n.lx[0] = a.x; n.lx[1] = a.y; n.ly[0] = a.z; n.ly[1] = a.w;
    n.lz[0] = b.x; n.lz[1] = b.y; n.hx[0] = b.z; n.hx[1] = b.w;
    n.hy[0] = c.x; n.hy[1] = c.y; n.hz[0] = c.z; n.hz[1] = c.w;
    const uint2 x = aux[i];
    n.child[0] = (int32_t)(int16_t)(x.x & 0xFFFFu);
    n.child[1] = (int32_t)(int16_t)(x.x >> 16);
    n.mt[0] = n.mt[1] = 0.0f;  // the boxes are stored grown by their node margin
    return n;
  }
  __device__ __forceinline__ BvhSlot *stack() const { return stk + threadIdx.x; }
};

// the per-ray slab constants: the reciprocal direction, the per-ray margin dm = kCullRel |o - bvh_ref|_2 + 1e-6
// (approximate root, widened 1e-4), (o + dm) rcp(d) for the low ends and (o - dm) rcp(d) for the high ends
struct RayInv { float ix, iy, iz, dm, lx, ly, lz, hx, hy, hz; };
__device__ __forceinline__ RayInv ray_inv(const DevScene &S, v3 o, v3 ray)
{
  const float ex = o.x - S.bvh_rx, ey = o.y - S.bvh_ry, ez = o.z - S.bvh_rz;
  const float dm = kCullRel * (__builtin_amdgcn_sqrtf(ex * ex + ey * ey + ez * ez) * 1.0001f) + 1e-6f;
  // finite reciprocals for the fused slabs: with rcp(0) = inf the fused form's inf - inf would leave one NaN slab end, and
  // fminf / fmaxf would then take the other end for both (a false cull of an axis-parallel ray, tests/test_bvh_box_bound.py)
  const auto fin = [](float v) { return fminf(fmaxf(v, -1e30f), 1e30f); };
  const float ix = fin(__builtin_amdgcn_rcpf(ray.x)), iy = fin(__builtin_amdgcn_rcpf(ray.y)),
              iz = fin(__builtin_amdgcn_rcpf(ray.z));
  return RayInv{ix, iy, iz, dm, (o.x + dm) * ix, (o.y + dm) * iy, (o.z + dm) * iz,
                (o.x - dm) * ix, (o.y - dm) * iy, (o.z - dm) * iz};
}

// child c of node n against the ray: hit (conservative), and the entry parameter t (>= 0) of the widened box.
// Every decision is a comparison that a NaN fails in the keeping direction.
__device__ __forceinline__ bool bvh_box(const BvhNode &n, int c, const RayInv &ri, float &tn)
{
  const float lx = n.lx[c], ly = n.ly[c], lz = n.lz[c], hx = n.hx[c], hy = n.hy[c], hz = n.hz[c];
  // The host stores each box grown by kCullRel mt[c] (rfx_scene.cpp build_pair_bvh), and |o - c|_2 + half-diagonal <=
  // |o - ref|_2 + mt[c] (c the box centre), so with the per-ray margin dm in the slab constants the total margin is at
  // least kCullRel (|o - c|_2 + half-diagonal) + 1e-6, the per-box bound of the culling argument.  One fused
  // multiply-add per slab end: a cull decision with a margin, not a reference value, so it may round once.
  const float ax = __builtin_fmaf(lx, ri.ix, -ri.lx), bx = __builtin_fmaf(hx, ri.ix, -ri.hx);
  const float ay = __builtin_fmaf(ly, ri.iy, -ri.ly), by = __builtin_fmaf(hy, ri.iy, -ri.hy);
  const float az = __builtin_fmaf(lz, ri.iz, -ri.lz), bz = __builtin_fmaf(hz, ri.iz, -ri.hz);
  // fminf / fmaxf return the other operand for a NaN (0 * inf on an axis-parallel ray): that axis is ignored
  const float t0 = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), 0.0f));
  const float t1 = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
  tn = t0;
  return !(t0 > t1 * 1.00001f + 1e-30f);
}

// The closest-hit walkers' distance prune: a child whose widened box is entered at distance d0 = t0 |ray| beyond the best
// hit so far (0.1% slack on the squares over the rounding here and in the reference's |ray t|^2) cannot hold a closer or
// tying hit.  d0 is formed first: it is a scene distance, so d0 * d0 is a normal float wherever h.sq is, whereas
// t0 * t0 * |ray|^2 overflowed for a caller's ray 1e-18 long (t0 ~ 1e19), was +inf for every t0 > 0 once |ray|^2 was
// (|ray| >= 1.3e19), and lost its bits to a subnormal t0 * t0 in between -- each pruned boxes holding the closest hit
// (tests/test_bvh_prune_bound.py).  |ray| = sqrt(a) where a = |ray|^2 is safely a normal float, else 0: such a ray
// prunes nothing by distance.  A NaN fails the comparison in the keeping direction.
__device__ __forceinline__ float prune_len(const RayConst &k)
{
  const float a = 0.5f * k.a2;                // |ray|^2 (exact: a2 = 2a)
  return a >= 0x1p-100f && a <= 0x1p100f ? __builtin_amdgcn_sqrtf(a) : 0.0f;
}
__device__ __forceinline__ bool bvh_beyond(float t0, float len, float best_sq)
{
  const float d0 = t0 * len;
  return d0 * d0 > best_sq * 1.001f;
}

// closest sphere hit of one lane's ray over the BVH (Scene.cpp:86-106 restricted to the spheres)
template <bool STATS, class NS>
__device__ __forceinline__ void closest_spheres_bvh(const DevScene &S, v3 origin, v3 ray, const RayConst &k, Hit &h,
                                                    Cnt &cnt, const NS &ns)
{
  const RayInv ri = ray_inv(S, origin, ray);
  const float len = prune_len(k);
  BvhSlot *stack = ns.stack();
  int sp = 0, node = 0;
  for (;;)
  {
    if (node >= 0)
    {
      const BvhNode n = ns.node(S, node);
      float t0, t1;
      // a child entered beyond the best hit cannot hold a closer (or tying) sphere
      const bool h0 = bvh_box(n, 0, ri, t0) && !bvh_beyond(t0, len, h.sq);
      const bool h1 = bvh_box(n, 1, ri, t1) && !bvh_beyond(t1, len, h.sq);
      if (h0 && h1)
      {
        const bool first0 = !(t1 < t0);
        stack[NS::kStride * sp++] = first0 ? n.child[1] : n.child[0];
        node = first0 ? n.child[0] : n.child[1];
        continue;
      }
      if (h0 || h1)
      {
        node = h0 ? n.child[0] : n.child[1];
        continue;
      }
    }
    else
    {
#pragma unroll
      for (int e = 0; e < RFX_BVH_LEAF_PAIRS; ++e)
      {
        const int j = RFX_BVH_LEAF_PAIRS * ~node + e;
        f2 b, d;
        pair_bd(S.sph_pair[j], origin, k, b, d);
        if (pair_may_hit(b, d))
        {
          float t, sq;
          if (sphere_tail<STATS, false, true>(b.x, d.x, ray, k, t, sq, cnt))
          {
            const int obj = S.sph_info[4 * j];
            if (tri_takes(sq, h.sq, obj, h.obj)) { h.sq = sq; h.obj = obj; h.i = 2 * j; h.t = t; }
          }
          if (sphere_tail<STATS, false, true>(b.y, d.y, ray, k, t, sq, cnt))
          {
            const int obj = S.sph_info[4 * j + 2];
            if (tri_takes(sq, h.sq, obj, h.obj)) { h.sq = sq; h.obj = obj; h.i = 2 * j + 1; h.t = t; }
          }
        }
      }
    }
    if (sp == 0) break;
    node = stack[NS::kStride * --sp];
  }
}

// any sphere but skip_sph occludes the shadow ray (Scene.cpp:129-141 restricted to the spheres): the occluding pair's
// index, or -1.  hint (wave-uniform, RFX_OCC_HINT): a pair that occluded a lane of this wave before, tested first -- an
// occluder is an occluder whatever the order (Scene.cpp:132-141 breaks at the first), so a lane it occludes skips its walk.
template <bool STATS, class NS>
__device__ __forceinline__ int occluded_spheres_bvh(const DevScene &S, v3 o, v3 ray, const RayConst &k, int skip_sph,
                                                    Cnt &cnt, const NS &ns, int hint = -1)
{
  float t, sq;
  if (RFX_OCC_HINT && hint >= 0)
  {
    f2 b, d;
    pair_bd(S.sph_pair[hint], o, k, b, d);
    if (pair_may_hit(b, d) &&
        ((sphere_tail<STATS, true, true>(b.x, d.x, ray, k, t, sq, cnt) && 2 * hint != skip_sph) ||
         (sphere_tail<STATS, true, true>(b.y, d.y, ray, k, t, sq, cnt) && 2 * hint + 1 != skip_sph)))
      return hint;
  }
  const RayInv ri = ray_inv(S, o, ray);
  BvhSlot *stack = ns.stack();
  int sp = 0, node = 0;
  for (;;)
  {
    if (node >= 0)
    {
      const BvhNode n = ns.node(S, node);
      float t0, t1;
      const bool h0 = bvh_box(n, 0, ri, t0), h1 = bvh_box(n, 1, ri, t1);
      if (h0 && h1)
      {
        stack[NS::kStride * sp++] = n.child[1];
        node = n.child[0];
        continue;
      }
      if (h0 || h1)
      {
        node = h0 ? n.child[0] : n.child[1];
        continue;
      }
    }
    else
    {
#pragma unroll
      for (int e = 0; e < RFX_BVH_LEAF_PAIRS; ++e)
      {
        const int j = RFX_BVH_LEAF_PAIRS * ~node + e;
        f2 b, d;
        pair_bd(S.sph_pair[j], o, k, b, d);
        // the hit object is filtered out after its test, which does not change the boolean
        if (pair_may_hit(b, d) &&
            ((sphere_tail<STATS, true, true>(b.x, d.x, ray, k, t, sq, cnt) && 2 * j != skip_sph) ||
             (sphere_tail<STATS, true, true>(b.y, d.y, ray, k, t, sq, cnt) && 2 * j + 1 != skip_sph)))
          return j;
      }
    }
    if (sp == 0) return -1;
    node = stack[NS::kStride * --sp];
  }
}

#if RFX_TRI_BVH
// ------------------------------------------------------------- non-small scenes: per-ray triangle BVH
// The same walk over the triangle tree (rfx_types.h RFX_TRI_BVH, rfx_scene.cpp build_tri_tree).  A child box is the
// AABB of its triangles' vertices under the margin of the sphere boxes: a triangle in the tree (cond < 300) reports a
// hit only where the ray passes within kCullRel |o - p| of a point p of the triangle (DESIGN.md "Triangle BVH"), and
// the box grown by kCullRel (|o - centre| + half-diagonal) + 1e-6 per axis holds that neighbourhood of every p
// inside it -- so a box the ray misses holds no triangle the reference could report, and a reported hit lies at or
// beyond the entry distance of its box (the h.sq 1.001 reject).  Nodes are read from global memory in every kernel
// form; the lane's stack is the sphere walk's (the two walks run one after the other).  Leaves run the exact test
// with the (distance, object index) rule, so the visiting order changes no result; h.i is the insertion index.
// The residual triangles (DevScene::tri_resid) are tested by every ray after the walk.
__device__ __forceinline__ int tri_rec_int(float bits) { return __builtin_bit_cast(int, bits); }

template <bool STATS, class NS>
__device__ __forceinline__ void closest_tris_bvh(const DevScene &S, v3 origin, v3 ray, const RayConst &k, Hit &h,
                                                 Cnt &cnt, const NS &ns)
{
  const RayInv ri = ray_inv(S, origin, ray);
  const float len = prune_len(k);
  BvhSlot *stack = ns.stack();
  int sp = 0, node = 0;
  for (;;)
  {
    if (node >= 0)
    {
      const BvhNode n = S.tri_bvh[node];
      float t0, t1;
      // a child entered beyond the best hit cannot hold a closer (or tying) triangle
      const bool h0 = bvh_box(n, 0, ri, t0) && !bvh_beyond(t0, len, h.sq);
      const bool h1 = bvh_box(n, 1, ri, t1) && !bvh_beyond(t1, len, h.sq);
      if (h0 && h1)
      {
        const bool first0 = !(t1 < t0);
        stack[NS::kStride * sp++] = first0 ? n.child[1] : n.child[0];
        node = first0 ? n.child[0] : n.child[1];
        continue;
      }
      if (h0 || h1)
      {
        node = h0 ? n.child[0] : n.child[1];
        continue;
      }
    }
    else
    {
#pragma unroll
      for (int e = 0; e < RFX_TRI_BVH_LEAF; ++e)
      {
        const TriGeo &g = S.tri_leaf[RFX_TRI_BVH_LEAF * ~node + e];
        float t, u, v, sq;
        if (tri_hit<STATS, false>(g, origin, ray, t, u, v, sq, cnt, k, h.sq))
        {
          const int obj = tri_rec_int(g.pad[1]);
          const float key = hit_key(sq);
          if (tri_takes(key, h.sq, obj, h.obj))
          {
            h.sq = key; h.obj = obj; h.kind = 1; h.i = tri_rec_int(g.pad[0]); h.t = t; h.u = u; h.v = v;
          }
        }
      }
    }
    if (sp == 0) break;
    node = stack[NS::kStride * --sp];
  }
  for (int q = 0; q < S.n_tri_resid; ++q)
  {
    const int i = S.tri_resid[q];
    float t, u, v, sq;
    if (tri_hit<STATS, false>(S.tri_geo[i], origin, ray, t, u, v, sq, cnt, k, h.sq))
    {
      const int obj = S.tri_shade[i].obj;
      const float key = hit_key(sq);
      hit_take(h, tri_takes(key, h.sq, obj, h.obj), key, obj, 1, i, t, u, v);
    }
  }
}

// any triangle but skip_tri (an insertion index) occludes the shadow ray (Scene.cpp:129-141 restricted to the
// triangles); the hit object is filtered out after its test, which does not change the boolean
template <bool STATS, class NS>
__device__ __forceinline__ bool occluded_tris_bvh(const DevScene &S, v3 o, v3 ray, const RayConst &k, int skip_tri,
                                                  Cnt &cnt, const NS &ns)
{
  float t, u, v, sq;
  const RayInv ri = ray_inv(S, o, ray);
  BvhSlot *stack = ns.stack();
  int sp = 0, node = 0;
  for (;;)
  {
    if (node >= 0)
    {
      const BvhNode n = S.tri_bvh[node];
      float t0, t1;
      const bool h0 = bvh_box(n, 0, ri, t0), h1 = bvh_box(n, 1, ri, t1);
      if (h0 && h1)
      {
        stack[NS::kStride * sp++] = n.child[1];
        node = n.child[0];
        continue;
      }
      if (h0 || h1)
      {
        node = h0 ? n.child[0] : n.child[1];
        continue;
      }
    }
    else
    {
#pragma unroll
      for (int e = 0; e < RFX_TRI_BVH_LEAF; ++e)
      {
        const TriGeo &g = S.tri_leaf[RFX_TRI_BVH_LEAF * ~node + e];
        if (tri_hit<STATS, true, true>(g, o, ray, t, u, v, sq, cnt, k) && tri_rec_int(g.pad[0]) != skip_tri) return true;
      }
    }
    if (sp == 0) break;
    node = stack[NS::kStride * --sp];
  }
  for (int q = 0; q < S.n_tri_resid; ++q)
  {
    const int i = S.tri_resid[q];
    if (tri_hit<STATS, true, true>(S.tri_geo[i], o, ray, t, u, v, sq, cnt, k) && i != skip_tri) return true;
  }
  return false;
}
#endif  // RFX_TRI_BVH

}  // namespace rfx
