// rt_accel.h -- the threaded bounding-volume hierarchy behind rt_trace_rays / rt_pick (rt_set_accel; include/rt_mi355.h;
// DESIGN.md section 32): the structure, its host build and the check every structure passes before it is uploaded.  Plain
// C++, no HIP: rt_accel_build_host runs the same code with no GPU.  The traversal kernels are rt_accel.inc's.  A second builder
// of the same structure, on the device and without the check, is rt_accel_build.h's (rt_set_accel_builder).
//
// The hierarchy only CULLS: a node may be skipped iff every object below it fails its own stored-box test (aabb_test).  So a
// node's box is the exact union of its objects' stored boxes (min / max of floats do not round; an inverted stored box counts
// as the swapped one, which aabb_test cannot tell apart), and whatever has no finite union -- a NaN or infinite bound -- or is
// too large to be worth a place in the tree stays on the LOOSE list, which every ray tests by brute force.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "rt_mi355.h"

#define RT_ACCEL_MAX_LEAF 8                 // most objects of a leaf (the count has four bits)
#define RT_ACCEL_DEFAULT_LEAF 4
#define RT_ACCEL_DEFAULT_LARGE 0.5f
// Default rt_accel_desc.minObjects: scenes below it are served by the brute-force kernels.  Measured: the
// smallest size at which RT_ACCEL_AUTO's traversal beats brute force on every ray set and mode; at 256 objects incoherent
// closest-hit rays are still 1.7x slower through the tree.
#define RT_ACCEL_DEFAULT_MIN_OBJECTS 1024

struct RtAccelBuild {
    std::vector<rt_accel_node> nodes;       // depth-first pre-order: the first child of inner node k is k + 1, the second nodes[k + 1].skip
    std::vector<uint32_t> order;            // object indices, addressed by the leaves (first << 4 | count)
    std::vector<uint32_t> loose;            // object indices outside the tree, ascending
    int leaves = 0, depth = 0;
    void clear() {
        nodes.clear();
        order.clear();
        loose.clear();
        leaves = depth = 0;
    }
    size_t bytes() const { return nodes.size() * sizeof(rt_accel_node) + (order.size() + loose.size()) * sizeof(uint32_t); }
};

// `desc` with every zero field replaced by its default, or false with *why set: an unknown traversal, a non-zero reserved word,
// leafSize outside 0..8, a negative minObjects, a negative or non-finite largeFraction.  desc may be null (all defaults, enable 1).
bool rt_accel_resolve_desc(const rt_accel_desc *desc, rt_accel_desc *out, const char **why);

// The structure of nObj caller records (RT_OBJECT_STRIDE bytes each; boundsMin / boundsMax are what rt_launch_compile_scene puts
// into the hot record's h0.xyz / h1.xyz).  Deterministic: the same bytes and desc give the same arrays, on any C++ library.
// desc is a resolved one.  Throws std::bad_alloc only.
void rt_accel_build(const void *objects, int nObj, const rt_accel_desc &desc, RtAccelBuild *out);

// True iff the arrays are a structure a traversal may walk for these objects: pre-order with every skip link strictly forward and
// equal to its subtree's end, every leaf within leafSize and the leaves covering order[] once in sequence, every object index
// below nObj and used exactly once across order[] and loose[], every node box finite and the exact union of its children's
// (a leaf's: of its objects' stored boxes).  Else false with *why set.
bool rt_accel_validate(const void *objects, int nObj, int leafSize, const rt_accel_node *nodes, size_t nNodes, const uint32_t *order,
                       size_t nOrder, const uint32_t *loose, size_t nLoose, const char **why);
