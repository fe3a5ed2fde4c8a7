// rt_meter.h -- the solve of rt_meter (include/rt_mi355.h has the definition): histogram of log-luminance bins ->
// trimmed mean -> target exposure -> adapted exposure.  Written once for host and device, in the style of
// rt_mesa_math.h: the device runs its pieces as rt_meter_solve_kernel behind the histogram kernel (rt_display.hip), the
// host runs them as rt_meter_solve_host (rt_display.cpp), which tests/test_meter_host.py pins to a numpy / Python-int
// restatement and tests/test_meter.py compares the device with.  Integer arithmetic and single fp32 operations only
// (-ffp-contract=off on both sides): no transcendental runs on the device, the two tables come from the host.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// pow2neg[f] = the fp32 nearest to 2^(-f / 256); log2q16[j] = round(65536 * log2(1 + (j + 0.5) / 8)): the Q16 log2 of
// the middle of the j-th eighth of an octave.  Built on the host in double (rt_meter_tables_host), passed by value.
struct RtMeterTables {
    float pow2neg[256];
    uint32_t log2q16[8];
};

// What the solve needs of rt_meter_desc (validated by the caller).
struct RtMeterSolveIn {
    float key, minExposure, maxExposure, adapt;
    int32_t lowPermille, highPermille;
    float prevExposure;
    uint32_t prevFrames;
};

struct RtMeterSolved {
    uint32_t nMetered, meanLog2Q16;
    float target, exposure;
    uint32_t frames;
};

inline void rt_meter_tables_host(RtMeterTables *t) {
    for (int f = 0; f < 256; f++) t->pow2neg[f] = (float)exp2(-(double)f / 256.0);
    for (int j = 0; j < 8; j++) t->log2q16[j] = (uint32_t)llround(65536.0 * log2(1.0 + ((double)j + 0.5) / 8.0));
}

// Trimming: the metered pixels in bin order occupy positions [0, n); positions [lo, n - hi) survive, so bin b, which
// holds positions [c, c + hist[b]) (c = the sum of the bins below it), keeps the length of its overlap with that range --
// what removing lo counts walking the bins upward and then hi counts walking them downward leaves (lo + hi < n whenever
// n >= 1).  The solve is split along that line: the range (rt_meter_trim), one bin's term of S (rt_meter_bin_term) and
// everything behind the sum (rt_meter_finish).  The host walks the bins in a loop (rt_meter_solve); the device gives every
// bin a thread and takes c from a prefix sum, S from a tree sum (rt_meter_solve_kernel) -- integer sums, so any order of
// summation gives the same bits.
struct RtMeterTrim {
    uint64_t lo, keepEnd, kept;
};

__host__ __device__ inline RtMeterTrim rt_meter_trim(uint64_t n, const RtMeterSolveIn &in) {
    const uint64_t lo = n * (uint64_t)in.lowPermille / 1000u, hi = n * (uint64_t)in.highPermille / 1000u;
    RtMeterTrim t;
    t.lo = lo;
    t.keepEnd = n - hi;
    t.kept = n - lo - hi;
    return t;
}

// hist'[b] * q[b], q[b] = (b >> 3) * 65536 + log2q16[b & 7]; c = hist[0] + ... + hist[b - 1], log2q = log2q16[b & 7]
__host__ __device__ inline uint64_t rt_meter_bin_term(int b, uint64_t c, uint32_t count, const RtMeterTrim &t, uint32_t log2q) {
    const uint64_t end = c + count;
    const uint64_t from = c > t.lo ? c : t.lo, to = end < t.keepEnd ? end : t.keepEnd;
    const uint64_t k = to > from ? to - from : 0;
    return k * ((uint64_t)(b >> 3) * 65536u + log2q);
}

__host__ __device__ inline RtMeterSolved rt_meter_finish(const RtMeterTrim &t, uint64_t S, const RtMeterSolveIn &in, const RtMeterTables &tab) {
    const bool prevOk = in.prevFrames != 0 && in.prevExposure > 0.0f && in.prevExposure < __builtin_huge_valf();
    RtMeterSolved r;
    r.nMetered = (uint32_t)t.kept;
    if (t.kept != 0) {
        const uint32_t m = (uint32_t)(S / t.kept);
        r.meanLog2Q16 = m;
        const float x = in.key * ldexpf(tab.pow2neg[(m >> 8) & 255u], 16 - (int)(m >> 16));
        r.target = x < in.minExposure ? in.minExposure : (x > in.maxExposure ? in.maxExposure : x);
    } else {
        r.meanLog2Q16 = 0;
        r.target = prevOk ? in.prevExposure : 1.0f;
    }
    if (!prevOk || in.adapt >= 1.0f) {
        r.exposure = r.target;
    } else {
        const float d = r.target - in.prevExposure;
        const float p = d * in.adapt;
        r.exposure = in.prevExposure + p;
    }
    r.frames = in.prevFrames == 0xffffffffu ? 0xffffffffu : in.prevFrames + 1u;
    return r;
}

// hist: the 256 untrimmed bins
inline RtMeterSolved rt_meter_solve(const uint32_t *hist, const RtMeterSolveIn &in, const RtMeterTables &tab) {
    uint64_t n = 0;
    for (int b = 0; b < 256; b++) n += hist[b];
    const RtMeterTrim t = rt_meter_trim(n, in);
    uint64_t c = 0, S = 0;
    for (int b = 0; b < 256; b++) {
        S += rt_meter_bin_term(b, c, hist[b], t, tab.log2q16[b & 7]);
        c += hist[b];
    }
    return rt_meter_finish(t, S, in, tab);
}
