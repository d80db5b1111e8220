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

static dim3 update_grid(uint32_t n) { return dim3((n + kUpdateThreads - 1) / kUpdateThreads); }

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
