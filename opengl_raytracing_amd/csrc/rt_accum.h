// rt_accum.h -- progressive accumulation's launch wrappers: what rt_accum.hip implements for the entry points in rt_accum.cpp.
// Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

// what the kernels need of a validated rt_accum_desc
struct RtAccumRule {
    float lumFloor, thr2;           // thr2 = relError * relError, one fp32 multiply on the host
    unsigned minSamples;
    int donePermille;
};

// rt_accum_add: clear of the state except `frames`, accumulate, solve -- three operations on s.  image: nPixels float4;
// accum: two planes of nPixels float4; state: one rt_accum_state; nPixels <= 2^31 - 1 (callers refuse larger frames first)
hipError_t rt_launch_accum_add(const void *image, void *accum, void *state, unsigned nPixels, const RtAccumRule &rule, hipStream_t s);
// rt_accum_view: plane 1 of accum -> out, nPixels float4 (v, v, v, 1); mode: rt_accum_view_mode
hipError_t rt_launch_accum_view(const void *accum, void *out, unsigned nPixels, const RtAccumRule &rule, int mode, hipStream_t s);
