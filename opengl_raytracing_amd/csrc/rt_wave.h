// rt_wave.h -- what the image stages' kernels share (rt_display.hip's meter, rt_accum.hip, rt_denoise.hip, rt_post.hip's bloom): the
// wave-level statistics primitives, the Rec.709 luminance, the XCD band map, and the CU count their launch wrappers size a grid by.
// Every device function is inlined and compiles to what its callers' own copies did.  No kernels, no state but rt_cu_count's cache.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>

// 2^48: a sample channel above this magnitude (or NaN) is refused by rt_accum_add and makes a pixel unusable to rt_denoise
constexpr float kRtSampleLimit = 0x1p48f;

// Rec.709 luminance as (R + G) + B (the bloom extract sums in another order and keeps its own).  Three scalars, not a vector: taken
// by value a float4 changes the meter's code, by reference an ext_vector the denoiser's register allocation.
__device__ __forceinline__ float rt_luma(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// Workgroups go to the 8 XCDs round-robin by id: this order gives each XCD one contiguous band of tiles, so that what neighbouring
// tiles share is served by one L2.  The grid is a multiple of 8 workgroups; a caller drops the tiles past its last one.
__device__ __forceinline__ int rt_xcd_tile() { return (int)(blockIdx.x & 7u) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3); }

// A commutative reduction over the 64 lanes of a full wave: four DPP rotations inside each row of 16 lanes (row_ror:8, 4, 2, 1 leave
// the row's result in every one of its lanes), then the four rows through v_readlane.  The result is wave-uniform.
template <class Op>
__device__ __forceinline__ unsigned rt_wave_reduce(unsigned v, Op op) {
    v = op(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false));
    v = op(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, false));
    v = op(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xf, 0xf, false));
    v = op(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xf, 0xf, false));
    return op(op((unsigned)__builtin_amdgcn_readlane((int)v, 0), (unsigned)__builtin_amdgcn_readlane((int)v, 16)),
              op((unsigned)__builtin_amdgcn_readlane((int)v, 32), (unsigned)__builtin_amdgcn_readlane((int)v, 48)));
}

// One count into the wave's LDS histogram for every lane with `pending` set.  Same-address LDS atomics serialise, and coherent
// content puts a whole wave into one or two bins: so up to ROUNDS times the wave takes the first pending lane's bin, a ballot of the
// lanes that share it, and ONE add of the popcount; lanes still pending after that add 1 each.  EVERY lane of the wave must call this
// together, pending or not (the loop is wave-uniform, its ballots read all 64 lanes): a caller's loop ends for the whole wave at once.
template <int ROUNDS>
__device__ __forceinline__ void rt_wave_hist_add(unsigned *waveHist, unsigned bin, bool pending, unsigned lane) {
    unsigned long long todo = __builtin_amdgcn_ballot_w64(pending);
#pragma unroll
    for (int it = 0; it < ROUNDS; it++) {
        if (todo == 0ull) break;                            // (wave-uniform)
        const unsigned leader = (unsigned)__builtin_ctzll(todo);
        const unsigned lb = (unsigned)__builtin_amdgcn_readlane((int)bin, (int)leader);
        const bool same = pending && bin == lb;
        const unsigned long long peers = __builtin_amdgcn_ballot_w64(same);
        if (lane == leader) atomicAdd(&waveHist[lb], (unsigned)__builtin_popcountll(peers));
        pending = pending && !same;
        todo &= ~peers;
    }
    if (pending) atomicAdd(&waveHist[bin], 1u);
}

// Ping-pong inclusive prefix sums of N <= 256 bins in ONE workgroup of 256 threads, all of which call it: thread b < N brings bin b's
// count.  Returns the plane of `scan` that holds the sums (totals below 2^32: 32 bits hold them).
template <int N>
__device__ __forceinline__ int rt_block_scan(unsigned (&scan)[2][N], unsigned b, unsigned count) {
    static_assert(N <= 256 && (N & (N - 1)) == 0, "one thread per bin");
    const bool isBin = N >= 256 || b < (unsigned)N;         // (static for N == 256: a run-time test costs the meter's solve 31 instructions)
    if (isBin) scan[0][b] = count;
    __syncthreads();
    int cur = 0;
#pragma unroll
    for (unsigned d = 1; d < (unsigned)N; d <<= 1) {
        if (isBin) scan[cur ^ 1][b] = scan[cur][b] + (b >= d ? scan[cur][b - d] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    return cur;
}

// The CU count of the current device, for the grids that are sized to the chip: asked once per device id, 256 when the runtime
// does not say.  (Two threads that ask first together store the same figure.)
inline int rt_cu_count() {
    static std::atomic<int> cached[64];                     // by device id; 0: not asked yet
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if ((n = cached[dev].load(std::memory_order_relaxed)) > 0) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cached[dev].store(n, std::memory_order_relaxed);
    return n;
}
