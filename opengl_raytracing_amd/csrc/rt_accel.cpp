// rt_accel.cpp -- the host side of the threaded hierarchy (rt_accel.h): the build, the check, and the entry points
// rt_set_accel / rt_accel_info / rt_accel_build_host of include/rt_mi355.h.  The kernels are rt_accel.inc's.  Also the host side
// of the device builder (rt_set_accel_builder / rt_accel_build_info / rt_accel_read; rt_accel_build.h has its kernels' interface),
// and the two switches that let other launches walk the same tree: rt_set_accel_shading and rt_set_accel_render.
#include "rt_accel.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <new>

#include "rt_accel_build.h"
#include "rt_context.h"

static_assert(RT_AB_MAX_LEAF == RT_ACCEL_MAX_LEAF, "the device builder sorts a leaf in RT_ACCEL_MAX_LEAF registers");

namespace {

struct Box {
    float lo[3], hi[3];
};

// The stored box of object i as the node boxes see it: min / max per axis (an inverted box behaves like the swapped one).
// False when a bound is NaN or infinite: such an object has no union with anything.
bool object_box(const void *objects, uint32_t i, Box *b) {
    float mn[3], mx[3];
    const uint8_t *o = (const uint8_t *)objects + (size_t)i * RT_OBJECT_STRIDE;
    memcpy(mn, o + offsetof(rt_object, boundsMin), sizeof mn);
    memcpy(mx, o + offsetof(rt_object, boundsMax), sizeof mx);
    for (int a = 0; a < 3; a++) {
        if (!isfinite(mn[a]) || !isfinite(mx[a])) return false;
        b->lo[a] = mn[a] < mx[a] ? mn[a] : mx[a];
        b->hi[a] = mn[a] < mx[a] ? mx[a] : mn[a];
    }
    return true;
}

void box_union(Box *into, const Box &b) {
    for (int a = 0; a < 3; a++) {
        if (b.lo[a] < into->lo[a]) into->lo[a] = b.lo[a];
        if (b.hi[a] > into->hi[a]) into->hi[a] = b.hi[a];
    }
}

// (-0 and +0 are the same bound to every comparison of the node test, but not to memcmp: compare as floats)
bool box_equal(const Box &x, const float lo[3], const float hi[3]) {
    for (int a = 0; a < 3; a++)
        if (!(x.lo[a] == lo[a] && x.hi[a] == hi[a])) return false;
    return true;
}

struct Builder {
    const std::vector<Box> &box;            // by object index
    std::vector<uint32_t> &idx;             // the tree's objects; becomes order[]
    std::vector<rt_accel_node> &nodes;
    int leafSize, leaves = 0, depth = 0;

    double centroid(uint32_t i, int a) const { return 0.5 * ((double)box[i].lo[a] + (double)box[i].hi[a]); }

    // The subtree over idx[first, first + count), count >= 1; returns its box.
    Box subtree(size_t first, size_t count, int level) {
        const size_t me = nodes.size();
        nodes.push_back(rt_accel_node());
        if (level > depth) depth = level;
        Box b;
        if (count <= (size_t)leafSize) {
            std::sort(idx.begin() + first, idx.begin() + first + count);     // ascending object index within a leaf
            b = box[idx[first]];
            for (size_t k = 1; k < count; k++) box_union(&b, box[idx[first + k]]);
            nodes[me].leaf = (uint32_t)(first << 4) | (uint32_t)count;
            leaves++;
        } else {
            // median split on the centroids along the axis on which they spread widest
            double lo[3], hi[3];
            for (int a = 0; a < 3; a++) lo[a] = hi[a] = centroid(idx[first], a);
            for (size_t k = 1; k < count; k++)
                for (int a = 0; a < 3; a++) {
                    const double c = centroid(idx[first + k], a);
                    if (c < lo[a]) lo[a] = c;
                    if (c > hi[a]) hi[a] = c;
                }
            int axis = 0;
            for (int a = 1; a < 3; a++)
                if (hi[a] - lo[a] > hi[axis] - lo[axis]) axis = a;
            const size_t half = count / 2;
            // a total order (the index breaks ties), so the two halves are the same sets whatever nth_element does inside
            std::nth_element(idx.begin() + first, idx.begin() + first + half, idx.begin() + first + count, [&](uint32_t x, uint32_t y) {
                const double cx = centroid(x, axis), cy = centroid(y, axis);
                return cx < cy || (cx == cy && x < y);
            });
            b = subtree(first, half, level + 1);
            box_union(&b, subtree(first + half, count - half, level + 1));
            nodes[me].leaf = RT_ACCEL_INNER;
        }
        for (int a = 0; a < 3; a++) {
            nodes[me].lo[a] = b.lo[a];
            nodes[me].hi[a] = b.hi[a];
        }
        nodes[me].skip = (uint32_t)nodes.size();
        return b;
    }
};

}  // namespace

bool rt_accel_resolve_desc(const rt_accel_desc *desc, rt_accel_desc *out, const char **why) {
    rt_accel_desc d;
    memset(&d, 0, sizeof d);
    d.enable = 1;
    if (desc) d = *desc;
    *why = nullptr;
    if (d.traversal != RT_ACCEL_AUTO && d.traversal != RT_ACCEL_LANE && d.traversal != RT_ACCEL_WAVE) *why = "rt_accel_desc: unknown traversal";
    else if (d.reserved[0] || d.reserved[1] || d.reserved[2]) *why = "rt_accel_desc: reserved words must be zero";
    else if (d.leafSize < 0 || d.leafSize > RT_ACCEL_MAX_LEAF) *why = "rt_accel_desc: leafSize outside 0..8";
    else if (d.minObjects < 0) *why = "rt_accel_desc: negative minObjects";
    else if (!(d.largeFraction >= 0.0f) || !isfinite(d.largeFraction)) *why = "rt_accel_desc: largeFraction must be finite and >= 0";
    if (*why) return false;
    if (d.leafSize == 0) d.leafSize = RT_ACCEL_DEFAULT_LEAF;
    if (d.minObjects == 0) d.minObjects = RT_ACCEL_DEFAULT_MIN_OBJECTS;
    if (d.largeFraction == 0.0f) d.largeFraction = RT_ACCEL_DEFAULT_LARGE;
    *out = d;
    return true;
}

namespace {

// The linear pass both builders start with: every object's ordered stored box, and who goes where.  LOOSE: no finite box, or
// "large" -- on some axis the box spans more than largeFraction of the whole scene's extent (the floor and the walls of a room:
// most rays pass their box test anyway, and in a tree they would stretch every ancestor).  Both lists come out ascending.
// centres (may be null): the per-axis minimum [0..2] and maximum [3..5] of the tree objects' box centres, in double.
void classify(const void *objects, int nObj, const rt_accel_desc &desc, std::vector<Box> *boxes, std::vector<uint32_t> *tree,
              std::vector<uint32_t> *loose, double *centres) {
    std::vector<Box> &box = *boxes;
    box.resize((size_t)nObj);
    std::vector<uint8_t> finite((size_t)nObj);
    // the union of every finite box, in double: a difference of two floats cannot overflow there
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = 0; i < nObj; i++) {
        finite[i] = object_box(objects, (uint32_t)i, &box[i]);
        if (!finite[i]) continue;
        for (int a = 0; a < 3; a++) {
            if (box[i].lo[a] < lo[a]) lo[a] = box[i].lo[a];
            if (box[i].hi[a] > hi[a]) hi[a] = box[i].hi[a];
        }
    }
    if (centres)
        for (int a = 0; a < 3; a++) {
            centres[a] = INFINITY;
            centres[3 + a] = -INFINITY;
        }
    for (int i = 0; i < nObj; i++) {
        bool large = !finite[i];
        for (int a = 0; a < 3 && !large; a++)
            large = (double)box[i].hi[a] - (double)box[i].lo[a] > (double)desc.largeFraction * (hi[a] - lo[a]);
        (large ? loose : tree)->push_back((uint32_t)i);
        if (large || !centres) continue;
        for (int a = 0; a < 3; a++) {
            const double c = 0.5 * ((double)box[i].lo[a] + (double)box[i].hi[a]);
            if (c < centres[a]) centres[a] = c;
            if (c > centres[3 + a]) centres[3 + a] = c;
        }
    }
}

}  // namespace

void rt_accel_build(const void *objects, int nObj, const rt_accel_desc &desc, RtAccelBuild *out) {
    out->clear();
    if (nObj <= 0) return;
    std::vector<Box> box;
    classify(objects, nObj, desc, &box, &out->order, &out->loose, nullptr);
    if (out->order.empty()) return;
    out->nodes.reserve(2 * out->order.size());
    Builder b{box, out->order, out->nodes, desc.leafSize};
    b.subtree(0, out->order.size(), 1);
    out->leaves = b.leaves;
    out->depth = b.depth;
}

bool rt_accel_validate(const void *objects, int nObj, int leafSize, const rt_accel_node *nodes, size_t nNodes, const uint32_t *order,
                       size_t nOrder, const uint32_t *loose, size_t nLoose, const char **why) {
#define ACCEL_REQUIRE(cond, text) \
    do {                          \
        if (!(cond)) {            \
            *why = text;          \
            return false;         \
        }                         \
    } while (0)
    *why = nullptr;
    ACCEL_REQUIRE(nObj >= 0 && nOrder + nLoose == (size_t)nObj, "order[] and loose[] do not hold nObj entries");
    ACCEL_REQUIRE(leafSize >= 1 && leafSize <= RT_ACCEL_MAX_LEAF, "leafSize outside 1..8");
    ACCEL_REQUIRE((nNodes == 0) == (nOrder == 0), "a tree without objects, or objects without a tree");
    ACCEL_REQUIRE(nNodes < 0x7fffffffu && nOrder < (1u << 28), "too many nodes");
    std::vector<uint8_t> seen((size_t)nObj, 0);
    for (size_t k = 0; k < nOrder + nLoose; k++) {
        const uint32_t i = k < nOrder ? order[k] : loose[k - nOrder];
        ACCEL_REQUIRE(i < (uint32_t)nObj, "an object index >= nObj");
        ACCEL_REQUIRE(!seen[i], "an object listed twice");
        seen[i] = 1;
    }
    if (nNodes == 0) return true;
    ACCEL_REQUIRE(nodes[0].skip == nNodes, "the root's skip link is not the node count");
    // Pre-order, by induction from the root: node k covers [k, skip); an inner node's children are k + 1, which must end at some
    // c inside, and c, which must end where k does.  Leaves in pre-order take order[] in sequence.
    size_t slot = 0;
    for (size_t k = 0; k < nNodes; k++) {
        const rt_accel_node &n = nodes[k];
        ACCEL_REQUIRE(n.skip > k && n.skip <= nNodes, "a skip link that does not point forward");
        Box b;
        if (n.leaf == RT_ACCEL_INNER) {
            ACCEL_REQUIRE(k + 1 < n.skip, "an inner node without children");
            const size_t c = nodes[k + 1].skip;
            ACCEL_REQUIRE(c > k + 1 && c < n.skip && nodes[c].skip == n.skip, "an inner node whose children do not tile its subtree");
            const rt_accel_node &x = nodes[k + 1], &y = nodes[c];
            for (int a = 0; a < 3; a++) {
                b.lo[a] = x.lo[a] < y.lo[a] ? x.lo[a] : y.lo[a];
                b.hi[a] = x.hi[a] > y.hi[a] ? x.hi[a] : y.hi[a];
            }
        } else {
            const size_t first = n.leaf >> 4, count = n.leaf & 15u;
            ACCEL_REQUIRE(n.skip == k + 1, "a leaf with a subtree");
            ACCEL_REQUIRE(count >= 1 && count <= (size_t)leafSize, "a leaf count outside 1..leafSize");
            ACCEL_REQUIRE(first == slot && first + count <= nOrder, "the leaves do not take order[] in sequence");
            slot += count;
            for (size_t s = 0; s < count; s++) {
                Box ob;
                ACCEL_REQUIRE(object_box(objects, order[first + s], &ob), "an object without a finite box in the tree");
                if (s == 0) b = ob;
                else box_union(&b, ob);
            }
        }
        for (int a = 0; a < 3; a++) ACCEL_REQUIRE(isfinite(n.lo[a]) && isfinite(n.hi[a]), "a node box that is not finite");
        ACCEL_REQUIRE(box_equal(b, n.lo, n.hi), "a node box that is not the union of its children");
    }
    ACCEL_REQUIRE(slot == nOrder, "order[] entries that no leaf addresses");
    return true;
#undef ACCEL_REQUIRE
}

namespace {

// build + check, with the time the two took; false (with *why) when the arrays must not be used
bool build_checked(const void *objects, int nObj, const rt_accel_desc &d, RtAccelBuild *b, double *ms, const char **why) {
    const auto t0 = std::chrono::steady_clock::now();
    bool ok = true;
    *why = nullptr;
    try {
        rt_accel_build(objects, nObj, d, b);
        ok = rt_accel_validate(objects, nObj, d.leafSize, b->nodes.data(), b->nodes.size(), b->order.data(), b->order.size(),
                               b->loose.data(), b->loose.size(), why);
    } catch (const std::bad_alloc &) {
        *why = "out of host memory";
        ok = false;
    }
    *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ok;
}

void fill_report(const RtAccelBuild &b, double ms, rt_accel_report *r) {
    r->nodes = (int32_t)b.nodes.size();
    r->leaves = b.leaves;
    r->depth = b.depth;
    r->loose = (int32_t)b.loose.size();
    r->bytes = b.bytes();
    r->buildMs = ms;
}

// RT_ACCEL_BUILD_DEVICE (rt_accel_build.h): the host classifies, uploads the two index lists and enqueues
// the kernels, all on the context's stream, where the host builder's upload would run.  dObjects holds this scene's records: the
// caller's upload of them is ahead on the same stream.  Every size is known here, so RtAccelDev and the report are filled at once;
// only the depth comes back from the device (rt_accel_info).  A HIP failure leaves `built` false.
int accel_build_device(rt_context *c, const void *objects, int nObj) {
    RtAccelState &A = c->accel;
    rt_accel_report &r = A.report;
    const auto t0 = std::chrono::steady_clock::now();
    auto elapsed = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    std::vector<uint32_t> tree, loose;
    double centres[6];
    bool ok = true;
    try {
        std::vector<Box> box;
        classify(objects, nObj, A.desc, &box, &tree, &loose, centres);
    } catch (const std::bad_alloc &) {
        ok = false;
    }
    r.builds++;
    A.buildsDevice++;
    A.deviceMs = 0.0;
    A.deviceMsPending = A.depthPending = false;
    if (!ok || tree.empty()) {                 // nothing for a tree: brute force serves, as with the host builder
        r.buildMs = A.hostMs = elapsed();
        return RT_OK;
    }
    RtAccelBuildParams P;
    for (int a = 0; a < 3; a++) {
        P.cmin[a] = centres[a];
        P.scale[a] = centres[3 + a] > centres[a] ? 1024.0 / (centres[3 + a] - centres[a]) : 0.0;
    }
    P.nObj = nObj;
    P.nTree = (int)tree.size();
    P.leafSize = A.desc.leafSize;
    P.nLeaves = (P.nTree + P.leafSize - 1) / P.leafSize;
    P.nNodes = 2 * P.nLeaves - 1;
    const size_t nodeBytes = (size_t)P.nNodes * sizeof(rt_accel_node), orderBytes = tree.size() * sizeof(uint32_t),
                 looseBytes = loose.size() * sizeof(uint32_t), bytes = nodeBytes + orderBytes + looseBytes;
    const size_t scratchBytes = RtAccelBuildScratch::carve(nullptr, P.nTree, P.leafSize, nullptr);
    if (!A.dBuf.holds(bytes) || !A.dBuildScratch.holds(scratchBytes)) {
        SCHED_TRY(c, drain());                 // queries on any stream may still read the structure about to be freed, a build the scratch
        HIP_TRY(c, A.dBuf.grow(bytes));
        HIP_TRY(c, A.dBuildScratch.grow(scratchBytes));
    }
    RtAccelBuildScratch S;
    RtAccelBuildScratch::carve(A.dBuildScratch, P.nTree, P.leafSize, &S);
    uint8_t *dOrder = A.dBuf.ptr + nodeBytes, *dLoose = dOrder + orderBytes;
    HIP_TRY(c, A.evBuild[0].create(hipEventDefault));
    HIP_TRY(c, A.evBuild[1].create(hipEventDefault));
    HIP_TRY(c, A.evDepth.create(hipEventDisableTiming));
    HIP_TRY(c, A.hDepth.grow(1));
    const int k = (int)(A.stageSeq++ & 1u);
    if (A.stageUsed[k]) HIP_TRY(c, hipEventSynchronize(A.evStage[k]));      // the copy out of this staging buffer two uploads ago
    HIP_TRY(c, A.hStage[k].grow(orderBytes + looseBytes));
    memcpy(A.hStage[k], tree.data(), orderBytes);
    if (looseBytes) memcpy(A.hStage[k] + orderBytes, loose.data(), looseBytes);
    HIP_TRY(c, hipEventRecord(A.evBuild[0], c->stream));
    HIP_TRY(c, hipMemcpyAsync(S.vals[0], A.hStage[k], orderBytes, hipMemcpyHostToDevice, c->stream));
    if (looseBytes) HIP_TRY(c, hipMemcpyAsync(dLoose, A.hStage[k] + orderBytes, looseBytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, A.evStage[k].create(hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(A.evStage[k], c->stream));
    A.stageUsed[k] = true;
    HIP_TRY(c, rt_launch_accel_build(c->dObjects, P, S, (float4 *)A.dBuf.ptr, (uint32_t *)dOrder, c->stream));
    HIP_TRY(c, hipEventRecord(A.evBuild[1], c->stream));
    HIP_TRY(c, hipMemcpyAsync(A.hDepth, S.depth, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipEventRecord(A.evDepth, c->stream));
    A.deviceMsPending = A.depthPending = true;
    A.dev.nodes = (const float4 *)A.dBuf.ptr;
    A.dev.order = (const unsigned *)dOrder;
    A.dev.loose = (const unsigned *)dLoose;
    A.dev.nNodes = P.nNodes;
    A.dev.nLoose = (int)loose.size();
    A.nOrder = P.nTree;
    A.builtBy = RT_ACCEL_BUILD_DEVICE;
    r.nodes = P.nNodes;
    r.leaves = P.nLeaves;
    r.loose = (int32_t)loose.size();
    r.bytes = bytes;
    r.buildMs = A.hostMs = elapsed();
    A.built = true;
    r.built = 1;
    return RT_OK;
}

// The context's structure for the scene `objects` (the bytes rt_set_scene was given), uploaded on the context's stream.  The
// caller has ordered that stream behind every launch that may still read the old structure (waitForLaunches) and records
// evScene behind this.  A scene the tree is not for -- too small, nothing but loose objects -- and a structure that cannot be
// built or fails its check leave `built` false: the brute-force kernels serve the queries.
int accel_upload(rt_context *c, const void *objects, int nObj) {
    RtAccelState &A = c->accel;
    A.built = false;
    rt_accel_report &r = A.report;
    r.built = r.nodes = r.leaves = r.depth = r.loose = 0;
    r.bytes = 0;
    if (!A.on || nObj < A.desc.minObjects || nObj <= 0) return RT_OK;
    if (A.builder == RT_ACCEL_BUILD_DEVICE) return accel_build_device(c, objects, nObj);
    RtAccelBuild b;
    double ms = 0.0;
    const char *why = nullptr;
    const bool ok = build_checked(objects, nObj, A.desc, &b, &ms, &why);
    r.builds++;
    r.buildMs = ms;
    A.buildsHost++;
    A.hostMs = ms;
    A.deviceMs = 0.0;
    A.deviceMsPending = A.depthPending = false;
    if (!ok || b.nodes.empty()) return RT_OK;
    fill_report(b, ms, &r);
    const size_t nodeBytes = b.nodes.size() * sizeof(rt_accel_node), orderBytes = b.order.size() * sizeof(uint32_t),
                 looseBytes = b.loose.size() * sizeof(uint32_t), bytes = nodeBytes + orderBytes + looseBytes;
    if (!A.dBuf.holds(bytes)) {
        SCHED_TRY(c, drain());                 // queries on any stream may still read the buffer about to be freed
        HIP_TRY(c, A.dBuf.grow(bytes));
    }
    const int k = (int)(A.stageSeq++ & 1u);
    if (A.stageUsed[k]) HIP_TRY(c, hipEventSynchronize(A.evStage[k]));      // the copy out of this staging buffer two uploads ago
    HIP_TRY(c, A.hStage[k].grow(bytes));
    memcpy(A.hStage[k], b.nodes.data(), nodeBytes);
    memcpy(A.hStage[k] + nodeBytes, b.order.data(), orderBytes);
    if (looseBytes) memcpy(A.hStage[k] + nodeBytes + orderBytes, b.loose.data(), looseBytes);
    HIP_TRY(c, hipMemcpyAsync(A.dBuf, A.hStage[k], bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, A.evStage[k].create(hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(A.evStage[k], c->stream));
    A.stageUsed[k] = true;
    A.dev.nodes = (const float4 *)A.dBuf.ptr;
    A.dev.order = (const unsigned *)(A.dBuf.ptr + nodeBytes);
    A.dev.loose = (const unsigned *)(A.dBuf.ptr + nodeBytes + orderBytes);
    A.dev.nNodes = (int)b.nodes.size();
    A.dev.nLoose = (int)b.loose.size();
    A.nOrder = (int)b.order.size();
    A.builtBy = RT_ACCEL_BUILD_HOST;
    A.built = true;
    r.built = 1;
    return RT_OK;
}

// rt_set_accel / rt_set_accel_builder with a scene loaded: the structure of the current scene under the new settings, at once
int rebuild_now(rt_context *c) {
    const size_t objBytes = (size_t)c->nObj * RT_OBJECT_STRIDE;
    if (!c->dCompiled || c->lastScene.size() < objBytes) return RT_OK;      // no scene (bytes) yet: built by the next rt_set_scene that changes them
    HIP_TRY(c, hipSetDevice(c->device));
    SCHED_TRY(c, waitForLaunches(c->stream));
    const int rc = accel_upload(c, c->lastScene.data(), c->nObj);
    if (rc) return rc;
    HIP_TRY(c, hipEventRecord(c->evScene, c->stream));      // foreign streams order behind the upload (caller_stream)
    return RT_OK;
}

}  // namespace

int rt_accel_scene_changed(rt_context *c, const void *objects, int nObj) { return accel_upload(c, objects, nObj); }

extern "C" {

int rt_set_accel(rt_context *c, const rt_accel_desc *desc) {
    if (!c) return RT_ERR_INVALID_ARG;
    RtAccelState &A = c->accel;
    rt_accel_desc d;
    const char *why = nullptr;
    if (!rt_accel_resolve_desc(desc, &d, &why)) return fail(c, RT_ERR_INVALID_ARG, why);
    const bool on = desc && desc->enable != 0;
    // the same settings again: the structure that stands is the one they would build
    if (on && A.on && memcmp(&d, &A.desc, sizeof d) == 0) return RT_OK;
    A.on = on;
    A.desc = d;
    if (!on) {
        A.built = false;       // (the buffer stays: launches in flight may read it, and the next rt_set_accel reuses it)
        A.report.built = A.report.nodes = A.report.leaves = A.report.depth = A.report.loose = 0;
        A.report.bytes = 0;
        return RT_OK;
    }
    return rebuild_now(c);
}

int rt_accel_info(rt_context *c, rt_accel_report *out) {
    if (!c || !out) return RT_ERR_INVALID_ARG;
    RtAccelState &A = c->accel;
    if (A.built && A.depthPending) {           // a device build: the depth is the one word only the device knows
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipEventSynchronize(A.evDepth));
        A.report.depth = (int32_t)A.hDepth[0];
        A.depthPending = false;
    }
    *out = A.report;
    return RT_OK;
}

int rt_set_accel_builder(rt_context *c, int builder) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (builder != RT_ACCEL_BUILD_HOST && builder != RT_ACCEL_BUILD_DEVICE) return fail(c, RT_ERR_INVALID_ARG, "rt_set_accel_builder: unknown builder");
    RtAccelState &A = c->accel;
    if (builder == A.builder) return RT_OK;
    A.builder = builder;
    return A.on ? rebuild_now(c) : RT_OK;
}

int rt_accel_build_info(rt_context *c, rt_accel_build_report *out) {
    if (!c || !out) return RT_ERR_INVALID_ARG;
    RtAccelState &A = c->accel;
    if (A.deviceMsPending) {
        float ms = 0.0f;
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipEventSynchronize(A.evBuild[1]));
        HIP_TRY(c, hipEventElapsedTime(&ms, A.evBuild[0], A.evBuild[1]));
        A.deviceMs = ms;
        A.deviceMsPending = false;
    }
    memset(out, 0, sizeof *out);
    out->builder = A.built ? A.builtBy : 0;
    out->buildsHost = A.buildsHost;
    out->buildsDevice = A.buildsDevice;
    out->hostMs = A.hostMs;
    out->deviceMs = A.deviceMs;
    return RT_OK;
}

int rt_accel_read(rt_context *c, rt_accel_node *nodes, size_t capNodes, uint32_t *order, size_t capOrder, uint32_t *loose, size_t capLoose,
                  rt_accel_report *info) {
    if (!c || !info) return RT_ERR_INVALID_ARG;
    RtAccelState &A = c->accel;
    memset(info, 0, sizeof *info);
    if (!A.built) return RT_OK;
    RT_TRY(rt_accel_info(c, info));
    const size_t nNodes = (size_t)A.dev.nNodes, nOrder = (size_t)A.nOrder, nLoose = (size_t)A.dev.nLoose;
    if (!nodes && !order && !loose) return RT_OK;      // the sizes only
    if (capNodes < nNodes || capOrder < nOrder || capLoose < nLoose) return fail(c, RT_ERR_TOO_LARGE, "rt_accel_read: a capacity is too small");
    if ((nNodes && !nodes) || (nOrder && !order) || (nLoose && !loose)) return fail(c, RT_ERR_INVALID_ARG, "rt_accel_read: a NULL array");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));       // the upload, or the build
    if (nNodes) HIP_TRY(c, hipMemcpy(nodes, A.dev.nodes, nNodes * sizeof(rt_accel_node), hipMemcpyDeviceToHost));
    if (nOrder) HIP_TRY(c, hipMemcpy(order, A.dev.order, nOrder * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (nLoose) HIP_TRY(c, hipMemcpy(loose, A.dev.loose, nLoose * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

// rt_shade_rays through the same tree (rt_accel_shade.inc).  Nothing is built or uploaded here: whether a launch walks the tree
// is decided per launch from `accel.built` (rt_context::accelShadeActive), so the two switches commute.
int rt_set_accel_shading(rt_context *c, const rt_accel_shade_desc *desc) {
    if (!c) return RT_ERR_INVALID_ARG;
    rt_accel_shade_desc d;
    memset(&d, 0, sizeof d);
    if (desc) d = *desc;
    if (d.traversal != RT_ACCEL_AUTO && d.traversal != RT_ACCEL_LANE && d.traversal != RT_ACCEL_WAVE)
        return fail(c, RT_ERR_INVALID_ARG, "rt_accel_shade_desc: unknown traversal");
    for (int k = 0; k < 5; k++)
        if (d.reserved[k]) return fail(c, RT_ERR_INVALID_ARG, "rt_accel_shade_desc: reserved words must be zero");
    if (d.minObjects < 0) return fail(c, RT_ERR_INVALID_ARG, "rt_accel_shade_desc: negative minObjects");
    RtAccelShadeState &S = c->accelShade;
    S.on = desc && d.enable != 0;
    // RT_ACCEL_AUTO: the per-ray walk (DESIGN.md section 33 has the measurement behind it and behind the default minObjects)
    S.lane = d.traversal == RT_ACCEL_WAVE ? 0 : 1;
    S.minObjects = d.minObjects ? d.minObjects : RT_ACCEL_SHADE_DEFAULT_MIN_OBJECTS;
    return RT_OK;
}

int rt_accel_shading_info(rt_context *c, rt_accel_shade_report *out) {
    if (!c || !out) return RT_ERR_INVALID_ARG;
    const RtAccelShadeState &S = c->accelShade;
    memset(out, 0, sizeof *out);
    out->active = c->accelShadeActive() ? 1 : 0;
    out->traversal = !S.on ? 0 : S.lane ? RT_ACCEL_LANE : RT_ACCEL_WAVE;
    out->launchesAccel[0] = S.launchesAccel[0];
    out->launchesAccel[1] = S.launchesAccel[1];
    out->launchesBrute = S.launchesBrute;
    return RT_OK;
}

// The frames through the same tree (rt_accel_render.inc).  Nothing is built or uploaded here either: whether a frame walks the
// tree is decided per launch (rt_context::accelRenderActive, launch_frame in rt_abi.cpp), so the switches commute.
int rt_set_accel_render(rt_context *c, const rt_accel_render_desc *desc) {
    if (!c) return RT_ERR_INVALID_ARG;
    rt_accel_render_desc d;
    memset(&d, 0, sizeof d);
    if (desc) d = *desc;
    if (d.traversal != RT_ACCEL_RENDER_AUTO && d.traversal != RT_ACCEL_RENDER_LANE && d.traversal != RT_ACCEL_RENDER_WAVE &&
        d.traversal != RT_ACCEL_RENDER_SPLIT)
        return fail(c, RT_ERR_INVALID_ARG, "rt_accel_render_desc: unknown traversal");
    for (int k = 0; k < 5; k++)
        if (d.reserved[k]) return fail(c, RT_ERR_INVALID_ARG, "rt_accel_render_desc: reserved words must be zero");
    if (d.minObjects < 0) return fail(c, RT_ERR_INVALID_ARG, "rt_accel_render_desc: negative minObjects");
    RtAccelRenderState &S = c->accelRender;
    S.on = desc && d.enable != 0;
    // RT_ACCEL_RENDER_AUTO: the per-ray walk.  SPLIT and LANE tie within their spreads on every measured scene from 1025 objects up and
    // both beat WAVE there, so the established form stays (DESIGN.md section 37 has the table, also behind the default minObjects)
    S.traversal = d.traversal == RT_ACCEL_RENDER_AUTO ? RT_ACCEL_RENDER_LANE : d.traversal;
    S.minObjects = d.minObjects ? d.minObjects : RT_ACCEL_RENDER_DEFAULT_MIN_OBJECTS;
    return RT_OK;
}

int rt_accel_render_info(rt_context *c, rt_accel_render_report *out) {
    if (!c || !out) return RT_ERR_INVALID_ARG;
    const RtAccelRenderState &S = c->accelRender;
    memset(out, 0, sizeof *out);
    out->active = c->accelRenderActive() ? 1 : 0;
    out->traversal = S.on ? S.traversal : 0;
    out->minObjects = S.minObjects;
    for (int k = 0; k < 3; k++) out->launchesAccel[k] = S.launchesAccel[k];
    out->launchesPacket = S.launchesPacket;
    return RT_OK;
}

int rt_accel_validate_host(const void *objects, int nObj, int leafSize, const rt_accel_node *nodes, size_t nNodes, const uint32_t *order,
                           size_t nOrder, const uint32_t *loose, size_t nLoose) {
    if (nObj < 0 || (nObj > 0 && !objects) || (nNodes && !nodes) || (nOrder && !order) || (nLoose && !loose)) return RT_ERR_INVALID_ARG;
    const char *why = nullptr;
    try {
        return rt_accel_validate(objects, nObj, leafSize, nodes, nNodes, order, nOrder, loose, nLoose, &why) ? RT_OK : RT_ERR_INVALID_ARG;
    } catch (const std::bad_alloc &) {
        return RT_ERR_TOO_LARGE;
    }
}

int rt_accel_build_host(const void *objects, int nObj, const rt_accel_desc *desc, rt_accel_node *nodes, size_t capNodes, uint32_t *order,
                        size_t capOrder, uint32_t *loose, size_t capLoose, rt_accel_report *info) {
    if (nObj < 0 || (nObj > 0 && !objects) || !info) return RT_ERR_INVALID_ARG;
    if (nObj > RT_MAX_OBJECTS) return RT_ERR_TOO_LARGE;
    rt_accel_desc d;
    const char *why = nullptr;
    if (!rt_accel_resolve_desc(desc, &d, &why)) return RT_ERR_INVALID_ARG;
    RtAccelBuild b;
    double ms = 0.0;
    memset(info, 0, sizeof *info);
    if (!build_checked(objects, nObj, d, &b, &ms, &why)) return RT_ERR_TOO_LARGE;      // (out of host memory: the build's own output passes its check)
    fill_report(b, ms, info);
    info->built = 1;
    info->builds = 1;
    if (!nodes && !order && !loose) return RT_OK;      // the sizes only
    if (capNodes < b.nodes.size() || capOrder < b.order.size() || capLoose < b.loose.size()) return RT_ERR_TOO_LARGE;
    if ((b.nodes.size() && !nodes) || (b.order.size() && !order) || (b.loose.size() && !loose)) return RT_ERR_INVALID_ARG;
    if (b.nodes.size()) memcpy(nodes, b.nodes.data(), b.nodes.size() * sizeof(rt_accel_node));
    if (b.order.size()) memcpy(order, b.order.data(), b.order.size() * sizeof(uint32_t));
    if (b.loose.size()) memcpy(loose, b.loose.data(), b.loose.size() * sizeof(uint32_t));
    return RT_OK;
}

}  // extern "C"
