// Moving spheres on the device (include/rfx.h "Moving spheres", rfx_update.cpp) -- its own TU (reflaxman_amd/_build.py),
// so that the other units' code objects stay as they were.
//
//   update_spheres_kernel    : a lane per record.  The centre and radius in, then everything SceneBuild derives from them
//                              by rfx_refit.h's functions: sph_geo, the sphere's lane of sph_pair, bound; the sphere's
//                              64-sphere chunk is marked dirty.
//   refit_chunks_kernel      : a lane per chunk.  A dirty chunk's bound from its spheres' bounds -- one lane runs the
//                              builder's sequential double sum over the chunk (its order is part of the value: no wave
//                              reduction) -- and the flag cleared.
//   refit_pair_leaves_kernel : a lane per leaf of the pair tree, its unwidened box (six doubles) from its spheres' bounds.
//   refit_pair_nodes_kernel  : a lane per node of one height, both children from the boxes below them, then the node's
//                              own box for the launch above.
// The refit is one launch per height, lowest first (at most kBvhStack launches), as the triangle tree's
// (rfx_update_kernels.hip): the stream's order is the only hand-off -- no workgroup waits or spins on another, every loop
// has a static bound.  Every box is a function of the current bounds alone.
#include <hip/hip_runtime.h>

#include "rfx_launch.h"
#include "rfx_refit.h"

#pragma clang fp contract(off)

namespace rfx {

constexpr uint32_t kSphUpdateThreads = 256;

__global__ __launch_bounds__(kSphUpdateThreads) void update_spheres_kernel(const SphUpdateParams P)
{
  const uint32_t j = blockIdx.x * kSphUpdateThreads + threadIdx.x;
  if (j >= P.count) return;
  const uint32_t i = P.ids ? P.ids[j] : P.first + j;
  if (i >= P.n_sph) return;  // a dead lane (ids only: the host checked the range form)
  const float cx = P.data[4 * (size_t)j], cy = P.data[4 * (size_t)j + 1], cz = P.data[4 * (size_t)j + 2];
  const float radius = sphere_radius(P.data[4 * (size_t)j + 3]);
  const float r2 = radius * radius;  // Sphere.cpp:19
  const uint32_t d = P.slot[i];
  SphereGeo g;
  g.cx = cx; g.cy = cy; g.cz = cz; g.sq_radius = r2;
  P.sph_geo[d] = g;
  SpherePair &p = P.sph_pair[d >> 1];  // the other lane is another sphere's, or the padding: not touched
  const uint32_t l = d & 1u;
  p.cx[l] = cx; p.cy[l] = cy; p.cz[l] = cz; p.r2[l] = r2;
  P.bound[d] = sphere_bound(cx, cy, cz, radius);
  P.dirty[d >> 6] = 1u;
}

__global__ __launch_bounds__(kSphUpdateThreads) void refit_chunks_kernel(const SphRefitParams P)
{
  const uint32_t c = blockIdx.x * kSphUpdateThreads + threadIdx.x;
  if (c >= P.n) return;
  if (!P.dirty[c]) return;
  const uint32_t first = 64u * c, left = P.n_sph - first;
  P.chunk_bound[c] = sphere_chunk_bound(P.bound + first, left < 64u ? left : 64u);
  P.dirty[c] = 0u;
}

__global__ __launch_bounds__(kSphUpdateThreads) void refit_pair_leaves_kernel(const SphRefitParams P)
{
  const uint32_t g = blockIdx.x * kSphUpdateThreads + threadIdx.x;
  if (g >= P.n) return;
  P.leaf_box[g] = sph_leaf_box(P.bound, g, P.n_sph);
}

__global__ __launch_bounds__(kSphUpdateThreads) void refit_pair_nodes_kernel(const SphRefitParams P)
{
  const uint32_t k = blockIdx.x * kSphUpdateThreads + threadIdx.x;
  if (k >= P.n) return;
  const int32_t id = P.list[k];
  BvhNode n = P.nodes[id];
  const double ref[3] = {P.ref[0], P.ref[1], P.ref[2]};
  SphBox b;
  sph_box_empty(b);
#pragma unroll
  for (int c = 0; c < 2; ++c)
  {
    const int32_t kid = n.child[c];
    const SphBox below = kid >= 0 ? P.node_box[kid] : P.leaf_box[~kid];
    bvh_child_set(n, c, below.lo, below.hi, ref, true);
    sph_box_join(b, below);
  }
  P.nodes[id] = n;
  P.node_box[id] = b;
}

static dim3 sph_update_grid(uint32_t n) { return dim3((n + kSphUpdateThreads - 1) / kSphUpdateThreads); }

hipError_t launch_update_spheres(const SphUpdateParams &P, hipStream_t st)
{
  hipLaunchKernelGGL(update_spheres_kernel, sph_update_grid(P.count), dim3(kSphUpdateThreads), 0, st, P);
  return hipGetLastError();
}

hipError_t launch_refit_chunks(const SphRefitParams &P, hipStream_t st)
{
  hipLaunchKernelGGL(refit_chunks_kernel, sph_update_grid(P.n), dim3(kSphUpdateThreads), 0, st, P);
  return hipGetLastError();
}

hipError_t launch_refit_pair_leaves(const SphRefitParams &P, hipStream_t st)
{
  hipLaunchKernelGGL(refit_pair_leaves_kernel, sph_update_grid(P.n), dim3(kSphUpdateThreads), 0, st, P);
  return hipGetLastError();
}

hipError_t launch_refit_pair_nodes(const SphRefitParams &P, hipStream_t st)
{
  hipLaunchKernelGGL(refit_pair_nodes_kernel, sph_update_grid(P.n), dim3(kSphUpdateThreads), 0, st, P);
  return hipGetLastError();
}

}  // namespace rfx
