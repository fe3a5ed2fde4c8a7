// rt_accum.h -- progressive accumulation's launch wrappers: what rt_accum.hip implements for the entry points in rt_accum.cpp,
// and the one convergence rule every kernel that judges a pixel shares (rt_accum.hip, rt_adaptive.hip).
// Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_accum_solve.h"

// what the kernels need of a validated rt_accum_desc
struct RtAccumRule {
    float lumFloor, thr2;           // thr2 = relError * relError, one fp32 multiply on the host
    unsigned minSamples;
    int donePermille;
};

// What a pixel's moments say, the one rule rt_accum_add's statistics, rt_accum_view's maps, rt_accum_select's list and
// rt_accum_add_at's statistics share.
struct RtAccumJudged {
    bool sampled;                   // count >= 2: the pixel is binned; otherwise r2 / bin / converged mean nothing
    bool converged;
    float r2;
    unsigned bin;
};

__device__ __forceinline__ RtAccumJudged rt_accum_judge(float mY, float M2, unsigned count, const RtAccumRule &rule) {
    RtAccumJudged j;
    j.sampled = count >= 2u;
    const float nf = (float)count;
    const float q = M2 / (nf * (nf - 1.0f));
    const float m = fmaxf(mY, rule.lumFloor);
    j.r2 = q / (m * m);
    const int e = (int)(__float_as_uint(j.r2) >> 21) - 396;
    j.bin = j.r2 > 0.0f ? (unsigned)min(max(e, 0), kAccumBins - 1) : 0u;
    j.converged = j.sampled && count >= rule.minSamples && j.r2 <= rule.thr2;
    return j;
}

// The description's own refusals (rt_accum.cpp): RT_OK and *rule (may be NULL), or the status with rt_last_error's text set (c may be NULL)
struct rt_context;
struct rt_accum_desc;
int rt_validate_accum_desc(rt_context *c, const rt_accum_desc *d, RtAccumRule *rule);

// rt_accum_add: clear of the state except `frames`, accumulate, solve -- three operations on s.  image: nPixels float4;
// accum: two planes of nPixels float4; state: one rt_accum_state; nPixels <= 2^31 - 1 (callers refuse larger frames first)
hipError_t rt_launch_accum_add(const void *image, void *accum, void *state, unsigned nPixels, const RtAccumRule &rule, hipStream_t s);
// the solve alone (rt_accum_solve_kernel, one workgroup): behind a statistics pass that filled the cleared state on s
hipError_t rt_launch_accum_solve(void *state, unsigned nPixels, int donePermille, hipStream_t s);
// rt_accum_view: plane 1 of accum -> out, nPixels float4 (v, v, v, 1); mode: rt_accum_view_mode
hipError_t rt_launch_accum_view(const void *accum, void *out, unsigned nPixels, const RtAccumRule &rule, int mode, hipStream_t s);
