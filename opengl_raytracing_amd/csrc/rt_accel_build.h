// rt_accel_build.h -- the device-side builder of rt_set_accel's hierarchy (rt_set_accel_builder): what the
// host side (rt_accel.cpp) and the kernels (rt_accel_build.hip) share.  The structure is rt_accel.h's -- rt_accel_node in
// depth-first pre-order with skip links, order[], loose[] -- over another topology: a linear BVH over the 30-bit Morton codes of
// the box centres.  The host classifies (loose / tree) and sizes everything before the first launch; the kernels sort, cut the
// sorted sequence into leaves, build the binary radix tree over the leaves' keys and write the nodes.  Kernel boundaries are the
// only ordering between workgroups: no kernel reads what another workgroup of the same launch wrote.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#define RT_AB_MAX_LEAF 8             // rt_accel.h's RT_ACCEL_MAX_LEAF: a leaf is re-sorted in registers
#define RT_AB_SORT_TILE 512         // keys of one workgroup of a sort pass (one wavefront, RT_AB_SORT_TILE / 64 rounds)
#define RT_AB_SORT_BITS 8            // one digit; 4 passes cover the 30-bit code
#define RT_AB_SORT_PASSES 4
#define RT_AB_SCAN_BLOCK 1024        // the single workgroup that scans a pass's histograms

// what the kernels need of the host's classification pass
struct RtAccelBuildParams {
    double cmin[3], scale[3];        // Morton grid: q = min(1023, (int)floor((c - cmin) * scale))
    int nObj, nTree, leafSize, nLeaves, nNodes;
};

// The scratch of one build, carved out of one allocation (every part 16-byte aligned).  bytes(): the size for nTree / leafSize.
struct RtAccelBuildScratch {
    uint32_t *keys[2], *vals[2];     // the sort's ping-pong pairs; vals[0] arrives from the host: the tree's objects, ascending
    uint32_t *hist;                  // 256 x sort workgroups
    unsigned long long *leafKey;     // K_j = morton << 32 | objectIndex of leaf j's first sorted entry
    float4 *leafBox;                 // 2 per leaf: (lo, -) (hi, -)
    uint32_t *rangeL, *rangeR;       // per inner node of the radix tree: the leaves it covers
    uint32_t *parent;                // per radix-tree node (inner i: slot i; leaf j: slot nLeaves - 1 + j): parent inner << 1 | first child
    uint32_t *nodeIdx;               // per inner node: its pre-order index
    uint32_t *depth;                 // one word: the tree's depth
    static size_t carve(uint8_t *base, int nTree, int leafSize, RtAccelBuildScratch *out);
};

inline int rt_ab_sort_blocks(int nTree) { return (nTree + RT_AB_SORT_TILE - 1) / RT_AB_SORT_TILE; }

// The whole build on stream s.  dObjects: the raw records (RT_OBJECT_STRIDE bytes each); S.vals[0]: the nTree object indices of
// the tree, ascending; dNodes / dOrder: the structure's arrays (nNodes nodes, nTree indices).  The caller has sized everything
// (nTree >= 1) and zeroed nothing: the node array and the depth word are cleared here.
hipError_t rt_launch_accel_build(const uint8_t *dObjects, const RtAccelBuildParams &P, const RtAccelBuildScratch &S, float4 *dNodes,
                                 uint32_t *dOrder, hipStream_t s);
