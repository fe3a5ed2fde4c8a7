// rt_accum_solve.h -- the solve of rt_accum_add (include/rt_mi355.h has the definition): histogram of r2 bins -> median and
// 95th-percentile bin, the done flag, the frame count.  Written once for host and device, as rt_meter.h is: the device runs
// its pieces as rt_accum_solve_kernel behind the accumulate kernel (rt_accum.hip), one thread per bin; the host walks the bins
// in a loop (rt_accum_solve, behind rt_accum_solve_host in rt_accum.cpp), which tests/test_accum_host.py pins to a Python-int
// restatement and tests/test_accum.py compares the device with.  Integer arithmetic only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kAccumBins = 128;

// word offsets of rt_accum_state (include/rt_mi355.h pins them)
enum { AS_NPIXELS = 128, AS_NUNSAMPLED = 129, AS_NCONVERGED = 130, AS_NREJECTED = 131, AS_MINCOUNT = 132, AS_MAXCOUNT = 133,
       AS_MAXR2BITS = 134, AS_MEDIANBIN = 135, AS_P95BIN = 136, AS_DONE = 137, AS_FRAMES = 138, AS_RESERVED = 139, AS_WORDS = 256 };

// The position a percentile asks for among n binned pixels: ceil(n * permille / 1000); 0 when n == 0 (n < 2^32: no overflow)
__host__ __device__ inline uint64_t rt_accum_rank(uint64_t n, uint32_t permille) { return (n * permille + 999u) / 1000u; }

// Whether the bin that holds `count` pixels and closes the cumulative count at cumInclusive is the smallest bin whose
// cumulative count reaches rank: true for exactly one bin when rank >= 1, for none when rank == 0 (the answer is bin 0 then)
__host__ __device__ inline bool rt_accum_bin_reaches(uint64_t cumInclusive, uint32_t count, uint64_t rank) {
    return rank != 0 && cumInclusive >= rank && cumInclusive - count < rank;
}

__host__ __device__ inline uint32_t rt_accum_done(uint32_t nConverged, uint32_t nPixels, int32_t donePermille) {
    return (uint64_t)nConverged * 1000u >= (uint64_t)nPixels * (uint64_t)donePermille ? 1u : 0u;
}

__host__ __device__ inline uint32_t rt_accum_next_frames(uint32_t frames) { return frames == 0xffffffffu ? frames : frames + 1u; }

struct RtAccumSolved {
    uint32_t medianBin, p95Bin, done, frames;
};

// hist: the 128 bins
inline RtAccumSolved rt_accum_solve(const uint32_t *hist, uint32_t nConverged, uint32_t nPixels, int32_t donePermille, uint32_t prevFrames) {
    uint64_t n = 0;
    for (int b = 0; b < kAccumBins; b++) n += hist[b];
    const uint64_t r50 = rt_accum_rank(n, 500), r95 = rt_accum_rank(n, 950);
    RtAccumSolved r = {0u, 0u, rt_accum_done(nConverged, nPixels, donePermille), rt_accum_next_frames(prevFrames)};
    uint64_t c = 0;
    for (int b = 0; b < kAccumBins; b++) {
        c += hist[b];
        if (rt_accum_bin_reaches(c, hist[b], r50)) r.medianBin = (uint32_t)b;
        if (rt_accum_bin_reaches(c, hist[b], r95)) r.p95Bin = (uint32_t)b;
    }
    return r;
}
