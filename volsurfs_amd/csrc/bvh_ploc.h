// PLOC topology of the device BVH builder (csrc/bvh_ploc.hip), called by vsa_bvh_dev_build_ploc
// (csrc/bvh_device.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int BVH_PLOC_MAX_RADIUS = 32;

// Clusters the n >= 2 triangles, in the Morton order `sorted` (face id at every sorted position) with boxes
// tbox[2 f] / tbox[2 f + 1], and writes the tree in the form bvh_device.hip's bottom-up, pre-order and emit kernels
// consume: order [n] = face ids in the tree's left-to-right leaf order; the n - 1 internal nodes with the root at 0:
// child (internal >= 0, leaf ~position), range = [first, last] leaf position, parent_int / parent_leaf =
// (parent << 1) | side (the root's -1).  A walk that leaves the tree ORs err_walk into *err.  Enqueued on `stream`;
// it synchronises once per batch of iterations to read the live cluster count and once at the end to free its
// scratch.  VSA_ERR_UNSUPPORTED if the clustering does not converge in n - 1 iterations (it always should).
int bvh_ploc_topology(const float4* tbox, const int32_t* sorted, int n, int radius, hipStream_t stream, int32_t* order,
                      int2* child, int2* range, int32_t* parent_int, int32_t* parent_leaf, int32_t* err, int err_walk);
