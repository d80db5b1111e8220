// Moving meshes on the device (include/rfx.h "Moving meshes", rfx_update.cpp) -- its own TU (reflaxman_amd/_build.py).
//
//   update_tris_kernel  : a lane per updated triangle.  The vertices in, then everything SceneBuild derives from them by
//                         rfx_refit.h's functions -- the reference's float steps and the builder's double steps, so the
//                         words are the host's: tri_geo, the normal of tri_shade, bound, the tree's copy in tri_leaf, the
//                         renderer's current vertices and class flags.
//   refit_leaves_kernel : a lane per leaf, its unwidened box from its triangles' current vertices.
//   refit_nodes_kernel  : a lane per node of one height, both children from the boxes below them (leaf boxes, or the node
//                         boxes the launch of the height below left), then the node's own box for the launch above.
// The refit is one launch per height, lowest first (at most kBvhStack + 1 launches): a parent reads what its children's
// launch wrote, and the stream's order is the only hand-off -- no workgroup waits or spins on another, no loop without a
// static bound.  Every box is a function of the current vertices alone (nothing is grown from the box before).
// The re-cut's kernels (include/rfx.h "Re-cutting") follow the refit's, with their own heading.
#include <hip/hip_runtime.h>

#include "rfx_launch.h"
#include "rfx_refit.h"

#pragma clang fp contract(off)

namespace rfx {

constexpr uint32_t kUpdateThreads = 256;

__global__ __launch_bounds__(kUpdateThreads) void update_tris_kernel(const UpdateParams P)
{
  const uint32_t j = blockIdx.x * kUpdateThreads + threadIdx.x;
  if (j >= P.count) return;
  const uint32_t i = P.first + j;
  float v[9];
  if (P.idx)
  {
    const uint32_t a = P.idx[3 * (size_t)j], b = P.idx[3 * (size_t)j + 1], c = P.idx[3 * (size_t)j + 2];
    if (a >= P.n_pos || b >= P.n_pos || c >= P.n_pos) return;  // a dead lane: the triangle keeps its vertices
    const uint32_t q[3] = {a, b, c};
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int e = 0; e < 3; ++e) v[3 * k + e] = P.pos[3 * (size_t)q[k] + e];
  }
  else
  {
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = P.pos[9 * (size_t)j + k];
  }
  const TriSetup t = tri_setup(mk(v[0], v[1], v[2]), mk(v[3], v[4], v[5]), mk(v[6], v[7], v[8]));
  const bool well = tri_well(t);
  TriGeo g = P.tri_geo[i];
  tri_geo_set(g, t);
  g.pad[0] = __builtin_bit_cast(float, (int32_t)i);  // its own mate group (only the small-scene loops read the leader)
  P.tri_geo[i] = g;
  P.tri_shade[i].nx = t.norm.x;
  P.tri_shade[i].ny = t.norm.y;
  P.tri_shade[i].nz = t.norm.z;
  P.tri_bound[i] = tri_bound(t.v0, t.v1, t.v2, well);
#pragma unroll
  for (int k = 0; k < 9; ++k) P.verts[9 * (size_t)i + k] = v[k];
  P.ill[i] = well ? 0u : 1u;
  const int32_t s = P.slot[i];
  if (s >= 0)
  {
    TriGeo l = P.tri_leaf[s];  // pad[0], pad[1]: the insertion and object index stay
    tri_geo_set(l, t);
    P.tri_leaf[s] = l;
  }
}

__global__ __launch_bounds__(kUpdateThreads) void refit_leaves_kernel(const RefitParams P)
{
  const uint32_t g = blockIdx.x * kUpdateThreads + threadIdx.x;
  if (g >= P.n) return;
  RefitBox b;
  refit_box_empty(b);
#pragma unroll
  for (int e = 0; e < RFX_TRI_BVH_LEAF; ++e)
  {
    const int32_t i = P.order[RFX_TRI_BVH_LEAF * (size_t)g + e];
    if (i < 0) continue;
#pragma unroll
    for (int q = 0; q < 3; ++q) refit_box_vertex(b, P.verts + 9 * (size_t)i + 3 * q);
    b.ill |= P.ill[i];
  }
  P.leaf_box[g] = b;
}

__global__ __launch_bounds__(kUpdateThreads) void refit_nodes_kernel(const RefitParams P)
{
  const uint32_t k = blockIdx.x * kUpdateThreads + threadIdx.x;
  if (k >= P.n) return;
  const int32_t id = P.list[k];
  BvhNode n = P.nodes[id];
  const double ref[3] = {P.ref[0], P.ref[1], P.ref[2]};
  RefitBox b;
  refit_box_empty(b);
#pragma unroll
  for (int c = 0; c < 2; ++c)
  {
    const int32_t kid = n.child[c];
    const RefitBox below = kid >= 0 ? P.node_box[kid] : P.leaf_box[~kid];
    refit_child(n, c, below, ref, true);
    refit_box_join(b, below);
  }
  P.nodes[id] = n;
  P.node_box[id] = b;
}

// ------------------------------------------------------------- re-cutting (rfx.h "Re-cutting", rfx_refit.h)
//   recut_box_kernel   : a lane per in-tree triangle; the placed sums' box by a workgroup reduction in LDS (integer
//                        atomics on rfx_refit.h's order-preserving code: min and max of finite floats are exact, so
//                        any order gives the same box), then six global atomics per workgroup.
//   recut_keys_kernel  : a lane per in-tree triangle, its key from the finished box.
//   (the renderer's radix sort, rfx_order_sort.hip, orders the in-tree list by key between these and the next)
//   recut_place_kernel : a lane per leaf slot: the triangle's slot and its leaf record from tri_geo / tri_shade (a padding
//                        slot: zeros); the first lanes also install the cut's children and by-height list.
// The stream's order is the only hand-off between the launches, as in the refit.
__global__ __launch_bounds__(kUpdateThreads) void recut_box_kernel(const RecutParams P)
{
  __shared__ uint32_t s_box[6];
  if (threadIdx.x < 6) s_box[threadIdx.x] = 0xFFFFFFFFu;
  __syncthreads();
  const uint32_t j = blockIdx.x * kUpdateThreads + threadIdx.x;
  if (j < P.n)
  {
    const uint32_t t = P.intree[j];
    float s[3];
    recut_sum(P.verts + 9 * (size_t)t, s);
    if (recut_placed(s, P.ill[t]))
    {
#pragma unroll
      for (int a = 0; a < 3; ++a)
      {
        const uint32_t c = recut_code(s[a]);
        atomicMin(&s_box[a], c);
        atomicMin(&s_box[3 + a], ~c);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 6 && s_box[threadIdx.x] != 0xFFFFFFFFu) atomicMin(&P.box[threadIdx.x], s_box[threadIdx.x]);
}

__global__ __launch_bounds__(kUpdateThreads) void recut_keys_kernel(const RecutParams P)
{
  const uint32_t j = blockIdx.x * kUpdateThreads + threadIdx.x;
  if (j >= P.n) return;
  const uint32_t t = P.intree[j];
  float s[3];
  recut_sum(P.verts + 9 * (size_t)t, s);
  uint32_t key = kRecutLastKey;
  if (recut_placed(s, P.ill[t]))
  {
    // (a placed lane: the box holds at least this triangle's sums, so the six words decode to finite floats)
    float lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
    {
      lo[a] = recut_decode(P.box[a]);
      hi[a] = recut_decode(~P.box[3 + a]);
    }
    key = recut_key(s, lo, recut_scale(lo, hi));
  }
  P.keys[j] = key;
}

__global__ __launch_bounds__(kUpdateThreads) void recut_place_kernel(const RecutPlaceParams P)
{
  const uint32_t q = blockIdx.x * kUpdateThreads + threadIdx.x;
  if (q < P.nodes_n)
  {
    P.nodes[q].child[0] = P.cut_child[2 * (size_t)q];
    P.nodes[q].child[1] = P.cut_child[2 * (size_t)q + 1];
    P.hlist[q] = P.cut_hlist[q];
  }
  if (q >= P.slots) return;
  const int32_t t = P.order[q];
  if (t < 0)
  {
    P.tri_leaf[q] = TriGeo{};
    return;
  }
  TriGeo l = P.tri_geo[t];
  l.pad[0] = __builtin_bit_cast(float, t);
  l.pad[1] = __builtin_bit_cast(float, P.tri_shade[t].obj);
  P.tri_leaf[q] = l;
  P.slot[t] = (int32_t)q;
}

static dim3 update_grid(uint32_t n) { return dim3((n + kUpdateThreads - 1) / kUpdateThreads); }

hipError_t launch_recut_keys(const RecutParams &P, hipStream_t st)
{
  hipError_t e = hipMemsetAsync(P.box, 0xFF, 6 * sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(recut_box_kernel, update_grid(P.n), dim3(kUpdateThreads), 0, st, P);
  hipLaunchKernelGGL(recut_keys_kernel, update_grid(P.n), dim3(kUpdateThreads), 0, st, P);
  return hipGetLastError();
}

hipError_t launch_recut_place(const RecutPlaceParams &P, hipStream_t st)
{
  hipLaunchKernelGGL(recut_place_kernel, update_grid(P.slots), dim3(kUpdateThreads), 0, st, P);
  return hipGetLastError();
}

hipError_t launch_update_tris(const UpdateParams &P, hipStream_t st)
{
  hipLaunchKernelGGL(update_tris_kernel, update_grid(P.count), dim3(kUpdateThreads), 0, st, P);
  return hipGetLastError();
}

hipError_t launch_refit_leaves(const RefitParams &P, hipStream_t st)
{
  hipLaunchKernelGGL(refit_leaves_kernel, update_grid(P.n), dim3(kUpdateThreads), 0, st, P);
  return hipGetLastError();
}

hipError_t launch_refit_nodes(const RefitParams &P, hipStream_t st)
{
  hipLaunchKernelGGL(refit_nodes_kernel, update_grid(P.n), dim3(kUpdateThreads), 0, st, P);
  return hipGetLastError();
}

}  // namespace rfx
