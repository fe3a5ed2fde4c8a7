// rt_resample.h -- the polyphase resampler of the display path (rt_display_resample, rt_resample_taps): the tap tables of one
// axis as plain host data, the shape of a launch, the device copies of the two axis tables a context keeps (held by value
// in rt_context, rt_context.h), and the launch wrapper rt_resample.hip implements.  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

// ---- host tables: no HIP type, so a plain host program can build and check them
// One axis, source size S -> destination size D: n taps per destination index, the first source index of each window (it may
// be negative or reach past S - 1: the kernel clamps) and the weights, weights[i * n + k], zero-padded behind a shorter window.
struct RtResampleAxis {
    int n = 0;
    std::vector<int32_t> first;
    std::vector<float> weights;
};

constexpr int kResampleMaxAxis = 1 << 20;       // the longest axis either entry point takes (RT_ERR_TOO_LARGE beyond it)

// Taps of one axis (include/rt_mi355.h has the definition).  With `out` == nullptr only *nTaps is computed.  Returns RT_OK,
// RT_ERR_INVALID_ARG (a size < 1, an unknown filter) or RT_ERR_TOO_LARGE (an axis above kResampleMaxAxis, n above the tap cap).
int rt_resample_build_axis(int S, int D, int filter, int *nTaps, RtResampleAxis *out);

// ---- the shape of a launch: a workgroup of 256 lanes owns tileW x tileH destination pixels and keeps the horizontally
// filtered source rows its vertical windows span, at most ldsRows of tileW float4, in LDS
struct RtResamplePlan {
    int tileW = 64, tileH = 16, ldsRows = 0;
    unsigned tilesX = 0, tilesY = 0;
};
constexpr int kResampleLdsTexels = 2048;        // 32 KiB of float4: five workgroups (20 waves) fit a CU's 160 KiB

// Source rows the destination rows j0 .. j1 read once their windows are clamped to the image
inline void rt_resample_row_span(const int32_t *firstY, int nY, int srcH, int j0, int j1, int *lo, int *hi) {
    const int a = firstY[j0], b = firstY[j1] + nY - 1;
    *lo = a < 0 ? 0 : (a > srcH - 1 ? srcH - 1 : a);
    *hi = b < 0 ? 0 : (b > srcH - 1 ? srcH - 1 : b);
}

// The tallest tile of 64 columns (16, 8, 4, 2, 1 rows) whose row span fits the LDS budget in every tile row; a ratio so large
// that one destination row alone overflows it gets tiles of 32 columns x 1 row (64 taps x 32 columns is the budget).
inline RtResamplePlan rt_resample_plan(const int32_t *firstY, int nY, int srcH, int dstW, int dstH) {
    RtResamplePlan p;
    for (int pass = 0; pass < 6; pass++) {
        p.tileW = pass < 5 ? 64 : 32;
        p.tileH = pass < 5 ? 16 >> pass : 1;
        p.ldsRows = 0;
        for (int j0 = 0; j0 < dstH; j0 += p.tileH) {
            int lo, hi;
            rt_resample_row_span(firstY, nY, srcH, j0, (j0 + p.tileH < dstH ? j0 + p.tileH : dstH) - 1, &lo, &hi);
            if (hi - lo + 1 > p.ldsRows) p.ldsRows = hi - lo + 1;
        }
        if (p.ldsRows * p.tileW <= kResampleLdsTexels) break;
    }
    p.tilesX = (unsigned)((dstW + p.tileW - 1) / p.tileW);
    p.tilesY = (unsigned)((dstH + p.tileH - 1) / p.tileH);
    return p;
}

#ifndef RT_RESAMPLE_HOST_ONLY
#include "rt_devbuf.h"

// The device copies of the two axis tables, keyed by (S, D, filter) per axis.  A launch reads them on whichever stream it
// runs; they are rebuilt and uploaded only when a key changes, and before that the host waits for the last launch that read
// the old ones (the rule the post passes' scratch follows, rt_devbuf.h).  `failed` names the HIP call that went wrong.
class ResampleTables {
public:
    struct Axis {
        int S = 0, D = 0, filter = -1;          // the key; filter -1: nothing built yet
        int n = 0;
        std::vector<int32_t> first;             // host copy: the plan reads the vertical axis' windows
        DevBuf<int32_t> dFirst;
        DevBuf<float> dWeights;                 // x axis: [k * D + i] (lanes of a wave read neighbouring columns); y axis: [j * n + k]
    };
    hipError_t create() { return use.create(); }
    // both axes' tables for this shape: RT_OK, a refusal of rt_resample_build_axis, or RT_ERR_HIP with `failed` / `failedHip` set
    int prepare(int srcW, int srcH, int dstW, int dstH, int filter);
    hipError_t acquire(hipStream_t s) { return use.acquire(s); }
    hipError_t release(hipStream_t s) { return use.release(s); }
    hipError_t drain() { return use.drain(); }

    Axis x, y;
    const char *failed = "";
    hipError_t failedHip = hipSuccess;

private:
    int update(Axis &a, int S, int D, int filter, bool transposed);
    ScratchUse use;
};

// One launch on s: src (srcW x srcH rgba32f) -> dst (dstW x dstH rgba32f) with the tables of `t` and the tiles of `plan`
hipError_t rt_launch_resample(const void *src, void *dst, int srcW, int srcH, int dstW, int dstH, const ResampleTables &t,
                              const RtResamplePlan &plan, hipStream_t s);
#endif
