// rt_accel_build.hip -- the kernels of the device-side hierarchy builder (rt_accel_build.h).  A translation
// unit of its own: no other .hip includes it, so no existing kernel's code can move.
//
// The launches of one build, in stream order:
//   rt_ab_keys          one thread per tree object: the Morton code of its box centre
//   4 x { rt_ab_hist, rt_ab_scan, rt_ab_scatter }   a stable LSD radix sort of (code, object index), 8 bits a pass
//   rt_ab_leaves        one thread per leaf: its slice of order[] (ascending object index), its box, its key
//   rt_ab_topology      one thread per inner node of the binary radix tree over the leaves' keys (Karras 2012): its range, and
//                       the parent link of each of its two children
//   rt_ab_emit_leaves   one thread per radix-tree node: its pre-order index from a walk up the parent links; leaves are written
//   rt_ab_emit_inner    one wavefront per inner node: the union of the leaf boxes of its own range, and the node
// A kernel reads only what the host uploaded or an EARLIER launch wrote; within a launch no workgroup reads another's output
// (every parent link, range and node has exactly one writer and no reader in the same launch).  No spin loop, no grid barrier.
#include "rt_accel_build.h"

#include "rt_mi355.h"

#define AB_BLOCK 256
#define AB_WAVE 64

static_assert(offsetof(rt_object, boundsMin) % 16 == 0 && offsetof(rt_object, boundsMax) % 16 == 0 && RT_OBJECT_STRIDE % 16 == 0,
              "the bounds are read as float4");
static_assert(RT_AB_SORT_TILE % AB_WAVE == 0 && RT_AB_SORT_BITS * RT_AB_SORT_PASSES >= 30, "the sort's geometry");

// The stored box of object i as the node boxes see it (rt_accel.cpp's object_box; the host has kept non-finite boxes out).
__device__ __forceinline__ void ab_object_box(const uint8_t *__restrict__ objects, unsigned i, float lo[3], float hi[3]) {
    const uint8_t *o = objects + (size_t)i * RT_OBJECT_STRIDE;
    const float4 mn = *(const float4 *)(o + offsetof(rt_object, boundsMin)), mx = *(const float4 *)(o + offsetof(rt_object, boundsMax));
    lo[0] = mn.x < mx.x ? mn.x : mx.x;
    hi[0] = mn.x < mx.x ? mx.x : mn.x;
    lo[1] = mn.y < mx.y ? mn.y : mx.y;
    hi[1] = mn.y < mx.y ? mx.y : mn.y;
    lo[2] = mn.z < mx.z ? mn.z : mx.z;
    hi[2] = mn.z < mx.z ? mx.z : mn.z;
}

// bit k of a 10-bit q to bit 3k
__device__ __forceinline__ unsigned ab_spread3(unsigned q) {
    q = (q | (q << 16)) & 0x030000ffu;
    q = (q | (q << 8)) & 0x0300f00fu;
    q = (q | (q << 4)) & 0x030c30c3u;
    q = (q | (q << 2)) & 0x09249249u;
    return q;
}

__global__ __launch_bounds__(AB_BLOCK) void rt_ab_keys_kernel(const uint8_t *__restrict__ objects, const RtAccelBuildParams P,
                                                               const uint32_t *__restrict__ tree, uint32_t *__restrict__ keys) {
    const int t = (int)(blockIdx.x * AB_BLOCK + threadIdx.x);
    if (t >= P.nTree) return;
    float lo[3], hi[3];
    ab_object_box(objects, tree[t], lo, hi);
    unsigned q[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double c = 0.5 * ((double)lo[a] + (double)hi[a]);
        int v = (int)floor((c - P.cmin[a]) * P.scale[a]);
        v = v < 0 ? 0 : v;                      // (c >= cmin: the host took cmin over these very centres)
        q[a] = (unsigned)(v > 1023 ? 1023 : v);
    }
    keys[t] = (ab_spread3(q[0]) << 2) | (ab_spread3(q[1]) << 1) | ab_spread3(q[2]);
}

// ---- the sort: one wavefront per tile of RT_AB_SORT_TILE keys ---------------------------------------------------------------
// hist[d * nBlocks + b]: how many keys of tile b have digit d.  Scanned exclusively as one flat array, that is where tile b's
// first key of digit d goes: behind every smaller digit, and behind the same digit of every earlier tile.
__global__ __launch_bounds__(AB_WAVE) void rt_ab_hist_kernel(const uint32_t *__restrict__ keys, int n, int shift, uint32_t *__restrict__ hist,
                                                              int nBlocks) {
    __shared__ unsigned cnt[1 << RT_AB_SORT_BITS];
    const int lane = (int)threadIdx.x, base = (int)blockIdx.x * RT_AB_SORT_TILE;
    for (int k = lane; k < (1 << RT_AB_SORT_BITS); k += AB_WAVE) cnt[k] = 0u;
    __syncthreads();
    for (int r = 0; r < RT_AB_SORT_TILE / AB_WAVE; r++) {
        const int idx = base + r * AB_WAVE + lane;
        if (idx < n) atomicAdd(&cnt[(keys[idx] >> shift) & ((1u << RT_AB_SORT_BITS) - 1u)], 1u);
    }
    __syncthreads();
    for (int k = lane; k < (1 << RT_AB_SORT_BITS); k += AB_WAVE) hist[(size_t)k * nBlocks + blockIdx.x] = cnt[k];
}

// exclusive scan of hist[0 .. n) in place, by one workgroup: a run per thread, the runs' sums scanned in LDS
__global__ __launch_bounds__(RT_AB_SCAN_BLOCK) void rt_ab_scan_kernel(uint32_t *__restrict__ hist, int n) {
    __shared__ unsigned sums[RT_AB_SCAN_BLOCK];
    const int t = (int)threadIdx.x, per = (n + RT_AB_SCAN_BLOCK - 1) / RT_AB_SCAN_BLOCK;
    const int b = t * per < n ? t * per : n, e = b + per < n ? b + per : n;
    unsigned sum = 0u;
    for (int k = b; k < e; k++) sum += hist[k];
    sums[t] = sum;
    __syncthreads();
    for (int off = 1; off < RT_AB_SCAN_BLOCK; off <<= 1) {
        const unsigned v = t >= off ? sums[t - off] : 0u;
        __syncthreads();
        sums[t] += v;
        __syncthreads();
    }
    unsigned run = sums[t] - sum;
    for (int k = b; k < e; k++) {
        const unsigned v = hist[k];
        hist[k] = run;
        run += v;
    }
}

// Stable: a tile's keys are met in ascending position (round, then lane), and a key's place among the tile's keys of its digit
// is the count of those met before it -- earlier rounds in cnt[], the same round by a match over the wavefront.
__global__ __launch_bounds__(AB_WAVE) void rt_ab_scatter_kernel(const uint32_t *__restrict__ keysIn, const uint32_t *__restrict__ valsIn, int n,
                                                                 int shift, const uint32_t *__restrict__ offs, int nBlocks,
                                                                 uint32_t *__restrict__ keysOut, uint32_t *__restrict__ valsOut) {
    __shared__ unsigned cnt[1 << RT_AB_SORT_BITS];
    const int lane = (int)threadIdx.x, base = (int)blockIdx.x * RT_AB_SORT_TILE;
    for (int k = lane; k < (1 << RT_AB_SORT_BITS); k += AB_WAVE) cnt[k] = offs[(size_t)k * nBlocks + blockIdx.x];
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int r = 0; r < RT_AB_SORT_TILE / AB_WAVE; r++) {
        const int idx = base + r * AB_WAVE + lane;
        const bool valid = idx < n;
        const unsigned key = valid ? keysIn[idx] : 0u, val = valid ? valsIn[idx] : 0u;
        const unsigned d = (key >> shift) & ((1u << RT_AB_SORT_BITS) - 1u);
        unsigned long long same = __builtin_amdgcn_ballot_w64(valid);          // the valid lanes with this lane's digit
#pragma unroll
        for (int b = 0; b < RT_AB_SORT_BITS; b++) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long set = __builtin_amdgcn_ballot_w64(bit);
            same &= bit ? set : ~set;
        }
        const unsigned rank = (unsigned)__popcll(same & below);
        const unsigned pos = cnt[d] + rank;
        __syncthreads();                                                        // every lane has read cnt[] ...
        if (valid && rank == 0u) cnt[d] += (unsigned)__popcll(same);           // ... before the digit's first lane moves it on
        __syncthreads();
        if (valid && pos < (unsigned)n) {
            keysOut[pos] = key;
            valsOut[pos] = val;
        }
    }
}

// ---- leaves -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ab_cx(unsigned &a, unsigned &b) {
    const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}

__global__ __launch_bounds__(AB_BLOCK) void rt_ab_leaves_kernel(const uint8_t *__restrict__ objects, const RtAccelBuildParams P,
                                                                 const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                                 uint32_t *__restrict__ order, unsigned long long *__restrict__ leafKey,
                                                                 float4 *__restrict__ leafBox) {
    const int j = (int)(blockIdx.x * AB_BLOCK + threadIdx.x);
    if (j >= P.nLeaves) return;
    const int first = j * P.leafSize, count = P.nTree - first < P.leafSize ? P.nTree - first : P.leafSize;
    leafKey[j] = ((unsigned long long)keys[first] << 32) | vals[first];        // before the re-sort below
    unsigned v[RT_AB_MAX_LEAF];
#pragma unroll
    for (int k = 0; k < RT_AB_MAX_LEAF; k++) v[k] = k < count ? vals[first + k] : 0xffffffffu;
    // ascending object index within the leaf: Batcher's odd-even merge network for 8 (the padding sorts to the end)
    ab_cx(v[0], v[1]); ab_cx(v[2], v[3]); ab_cx(v[4], v[5]); ab_cx(v[6], v[7]);
    ab_cx(v[0], v[2]); ab_cx(v[1], v[3]); ab_cx(v[4], v[6]); ab_cx(v[5], v[7]);
    ab_cx(v[1], v[2]); ab_cx(v[5], v[6]);
    ab_cx(v[0], v[4]); ab_cx(v[1], v[5]); ab_cx(v[2], v[6]); ab_cx(v[3], v[7]);
    ab_cx(v[2], v[4]); ab_cx(v[3], v[5]);
    ab_cx(v[1], v[2]); ab_cx(v[3], v[4]); ab_cx(v[5], v[6]);
    const float inf = __builtin_inff();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
#pragma unroll
    for (int k = 0; k < RT_AB_MAX_LEAF; k++) {
        if (k < count && v[k] < (unsigned)P.nObj) {       // (a permutation of the uploaded indices, all < nObj)
            order[first + k] = v[k];
            float blo[3], bhi[3];
            ab_object_box(objects, v[k], blo, bhi);
#pragma unroll
            for (int a = 0; a < 3; a++) {
                if (blo[a] < lo[a]) lo[a] = blo[a];
                if (bhi[a] > hi[a]) hi[a] = bhi[a];
            }
        }
    }
    leafBox[2 * j] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    leafBox[2 * j + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
}

// ---- topology: the binary radix tree over K_0 < K_1 < ... < K_{M-1} ---------------------------------------------------------
// the length of the common prefix of K_i and K_j, -1 for a j outside the array (the keys are distinct: never 64)
__device__ __forceinline__ int ab_delta(const unsigned long long *__restrict__ K, int M, unsigned long long ki, int j) {
    return j < 0 || j >= M ? -1 : __clzll((long long)(ki ^ K[j]));
}

__global__ __launch_bounds__(AB_BLOCK) void rt_ab_topology_kernel(const unsigned long long *__restrict__ K, int M, uint32_t *__restrict__ rangeL,
                                                                   uint32_t *__restrict__ rangeR, uint32_t *__restrict__ parent) {
    const int i = (int)(blockIdx.x * AB_BLOCK + threadIdx.x);
    if (i >= M - 1) return;
    const unsigned long long ki = K[i];
    // inner node i has leaf i at one end of its range; d: towards the other end
    const int d = ab_delta(K, M, ki, i + 1) - ab_delta(K, M, ki, i - 1) >= 0 ? 1 : -1;
    const int dmin = ab_delta(K, M, ki, i - d);
    int lmax = 2;
    while (lmax < 2 * M && ab_delta(K, M, ki, i + lmax * d) > dmin) lmax *= 2;
    int l = 0;
    for (int t = lmax / 2; t >= 1; t /= 2)
        if (ab_delta(K, M, ki, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    // the split: the last leaf (from i) that shares more than the range's common prefix with K_i
    const int dnode = ab_delta(K, M, ki, j);
    int s = 0, t = l;
    do {
        t = (t + 1) / 2;
        if (ab_delta(K, M, ki, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int g = i + s * d + (d < 0 ? -1 : 0);             // first child [lo, g], second [g + 1, hi]
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    rangeL[i] = (uint32_t)lo;
    rangeR[i] = (uint32_t)hi;
    // (lo <= g < hi for distinct ascending keys; the clamp keeps the two stores inside parent[] whatever the keys hold)
    const int gc = g < 0 ? 0 : g > M - 2 ? M - 2 : g;
    parent[lo == gc ? M - 1 + gc : gc] = ((uint32_t)i << 1) | 1u;
    parent[hi == gc + 1 ? M - 1 + gc + 1 : gc + 1] = (uint32_t)i << 1;
}

// ---- pre-order without a traversal ------------------------------------------------------------------------------------------
// A node covering leaves [l, r] sits at 2 l + A, A = how many of its ancestors hold it in their first child: before it in
// pre-order come the 2 l - (number of subtrees that tile [0, l)) nodes of those subtrees -- one per ancestor that holds it in its
// SECOND child -- and all its ancestors.  Its subtree has 2 (r - l + 1) - 1 nodes.
__global__ __launch_bounds__(AB_BLOCK) void rt_ab_emit_leaves_kernel(const RtAccelBuildParams P, const uint32_t *__restrict__ parent,
                                                                      const uint32_t *__restrict__ rangeL, const float4 *__restrict__ leafBox,
                                                                      uint32_t *__restrict__ nodeIdx, float4 *__restrict__ nodes,
                                                                      uint32_t *__restrict__ depth) {
    const int slot = (int)(blockIdx.x * AB_BLOCK + threadIdx.x), M = P.nLeaves;
    if (slot >= P.nNodes) return;
    unsigned A = 0u, above = 0u, cur = (unsigned)slot;
    for (int step = 0; step < 64 && cur != 0u && cur < (unsigned)P.nNodes; step++) {      // the keys have 62 bits: at most 62 ancestors
        const unsigned p = parent[cur];
        A += p & 1u;
        above++;
        cur = p >> 1;
    }
    if (slot < M - 1) {
        nodeIdx[slot] = 2u * rangeL[slot] + A;
        return;
    }
    const int j = slot - (M - 1), first = j * P.leafSize, count = P.nTree - first < P.leafSize ? P.nTree - first : P.leafSize;
    const unsigned idx = 2u * (unsigned)j + A;
    atomicMax(depth, above + 1u);
    if (idx >= (unsigned)P.nNodes) return;
    const float4 lo = leafBox[2 * j], hi = leafBox[2 * j + 1];
    nodes[2 * (size_t)idx] = make_float4(lo.x, lo.y, lo.z, __uint_as_float(idx + 1u));
    nodes[2 * (size_t)idx + 1] = make_float4(hi.x, hi.y, hi.z, __uint_as_float(((unsigned)first << 4) | (unsigned)count));
}

// min / max of floats do not round: whatever order the lanes and the shuffles take gives the same bounds (up to the sign of zero)
__global__ __launch_bounds__(AB_BLOCK) void rt_ab_emit_inner_kernel(const RtAccelBuildParams P, const uint32_t *__restrict__ rangeL,
                                                                     const uint32_t *__restrict__ rangeR, const uint32_t *__restrict__ nodeIdx,
                                                                     const float4 *__restrict__ leafBox, float4 *__restrict__ nodes) {
    const int i = (int)(blockIdx.x * (AB_BLOCK / AB_WAVE) + threadIdx.x / AB_WAVE), lane = (int)(threadIdx.x % AB_WAVE), M = P.nLeaves;
    if (i >= M - 1) return;                                  // (wave-uniform)
    const unsigned l = rangeL[i], idx = nodeIdx[i];
    unsigned r = rangeR[i];
    r = r < (unsigned)M ? r : (unsigned)M - 1u;
    const float inf = __builtin_inff();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (unsigned j = l + (unsigned)lane; j <= r; j += AB_WAVE) {
        const float4 a = leafBox[2 * (size_t)j], b = leafBox[2 * (size_t)j + 1];
        lo[0] = a.x < lo[0] ? a.x : lo[0];
        lo[1] = a.y < lo[1] ? a.y : lo[1];
        lo[2] = a.z < lo[2] ? a.z : lo[2];
        hi[0] = b.x > hi[0] ? b.x : hi[0];
        hi[1] = b.y > hi[1] ? b.y : hi[1];
        hi[2] = b.z > hi[2] ? b.z : hi[2];
    }
#pragma unroll
    for (int off = AB_WAVE / 2; off >= 1; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float ol = __shfl_xor(lo[a], off, AB_WAVE), oh = __shfl_xor(hi[a], off, AB_WAVE);
            lo[a] = ol < lo[a] ? ol : lo[a];
            hi[a] = oh > hi[a] ? oh : hi[a];
        }
    }
    if (lane != 0 || idx >= (unsigned)P.nNodes) return;
    nodes[2 * (size_t)idx] = make_float4(lo[0], lo[1], lo[2], __uint_as_float(idx + 2u * (r - l + 1u) - 1u));
    nodes[2 * (size_t)idx + 1] = make_float4(hi[0], hi[1], hi[2], __uint_as_float(RT_ACCEL_INNER));
}

// ---- host side --------------------------------------------------------------------------------------------------------------
size_t RtAccelBuildScratch::carve(uint8_t *base, int nTree, int leafSize, RtAccelBuildScratch *out) {
    const size_t n = (size_t)(nTree > 0 ? nTree : 1), M = (n + (size_t)leafSize - 1) / (size_t)leafSize, inner = M > 1 ? M - 1 : 1;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        uint8_t *p = base ? base + at : nullptr;
        at += (bytes + 15) & ~(size_t)15;
        return p;
    };
    RtAccelBuildScratch s;
    for (int k = 0; k < 2; k++) s.keys[k] = (uint32_t *)take(n * 4);
    for (int k = 0; k < 2; k++) s.vals[k] = (uint32_t *)take(n * 4);
    s.hist = (uint32_t *)take(((size_t)rt_ab_sort_blocks((int)n) << RT_AB_SORT_BITS) * 4);
    s.leafKey = (unsigned long long *)take(M * 8);
    s.leafBox = (float4 *)take(M * 32);
    s.rangeL = (uint32_t *)take(inner * 4);
    s.rangeR = (uint32_t *)take(inner * 4);
    s.parent = (uint32_t *)take((2 * M - 1) * 4);
    s.nodeIdx = (uint32_t *)take(inner * 4);
    s.depth = (uint32_t *)take(4);
    if (out) *out = s;
    return at;
}

hipError_t rt_launch_accel_build(const uint8_t *dObjects, const RtAccelBuildParams &P, const RtAccelBuildScratch &S, float4 *dNodes,
                                 uint32_t *dOrder, hipStream_t s) {
    if (P.nTree < 1 || P.leafSize < 1 || P.leafSize > RT_AB_MAX_LEAF || P.nLeaves != (P.nTree + P.leafSize - 1) / P.leafSize ||
        P.nNodes != 2 * P.nLeaves - 1)
        return hipErrorInvalidValue;
    const int n = P.nTree, M = P.nLeaves, nb = rt_ab_sort_blocks(n);
    auto grid = [](int threads) { return dim3((unsigned)((threads + AB_BLOCK - 1) / AB_BLOCK)); };
    hipError_t e;
    // a node no kernel writes would be a leaf of no objects that links to its successor: nothing a walk can leave its arrays through
    if ((e = hipMemsetAsync(dNodes, 0, (size_t)P.nNodes * 2 * sizeof(float4), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(S.depth, 0, sizeof(uint32_t), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(rt_ab_keys_kernel, grid(n), dim3(AB_BLOCK), 0, s, dObjects, P, (const uint32_t *)S.vals[0], S.keys[0]);
    for (int p = 0; p < RT_AB_SORT_PASSES; p++) {
        const int in = p & 1, out = in ^ 1, shift = p * RT_AB_SORT_BITS;
        hipLaunchKernelGGL(rt_ab_hist_kernel, dim3((unsigned)nb), dim3(AB_WAVE), 0, s, (const uint32_t *)S.keys[in], n, shift, S.hist, nb);
        hipLaunchKernelGGL(rt_ab_scan_kernel, dim3(1), dim3(RT_AB_SCAN_BLOCK), 0, s, S.hist, nb << RT_AB_SORT_BITS);
        hipLaunchKernelGGL(rt_ab_scatter_kernel, dim3((unsigned)nb), dim3(AB_WAVE), 0, s, (const uint32_t *)S.keys[in],
                           (const uint32_t *)S.vals[in], n, shift, (const uint32_t *)S.hist, nb, S.keys[out], S.vals[out]);
    }
    static_assert(RT_AB_SORT_PASSES % 2 == 0, "the sorted pairs end in keys[0] / vals[0]");
    hipLaunchKernelGGL(rt_ab_leaves_kernel, grid(M), dim3(AB_BLOCK), 0, s, dObjects, P, (const uint32_t *)S.keys[0], (const uint32_t *)S.vals[0],
                       dOrder, S.leafKey, S.leafBox);
    if (M > 1)
        hipLaunchKernelGGL(rt_ab_topology_kernel, grid(M - 1), dim3(AB_BLOCK), 0, s, (const unsigned long long *)S.leafKey, M, S.rangeL, S.rangeR,
                           S.parent);
    hipLaunchKernelGGL(rt_ab_emit_leaves_kernel, grid(P.nNodes), dim3(AB_BLOCK), 0, s, P, (const uint32_t *)S.parent, (const uint32_t *)S.rangeL,
                       (const float4 *)S.leafBox, S.nodeIdx, dNodes, S.depth);
    if (M > 1)
        hipLaunchKernelGGL(rt_ab_emit_inner_kernel, dim3((unsigned)((M - 1 + AB_BLOCK / AB_WAVE - 1) / (AB_BLOCK / AB_WAVE))), dim3(AB_BLOCK), 0, s, P,
                           (const uint32_t *)S.rangeL, (const uint32_t *)S.rangeR, (const uint32_t *)S.nodeIdx, (const float4 *)S.leafBox, dNodes);
    return hipGetLastError();
}
