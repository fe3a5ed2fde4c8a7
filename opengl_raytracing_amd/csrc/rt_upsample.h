// rt_upsample.h -- first-hit-guided upsampling's launch wrappers: what rt_upsample.hip implements for the entry points in
// rt_upsample.cpp (rt_upsample, rt_image_put_at; include/rt_mi355.h has the definition).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// what the kernel needs of a validated rt_upsample_desc
struct RtUpsampleRule {
    int width, height, lowWidth, lowHeight, normalLog2Power;
    float minWeight;
};

// rt_upsample: reconstruct (out, the holes' ballots and the workgroups' totals into scratch, rt_accum_select's layout), then
// rt_launch_select_from_ballots (rt_adaptive.h): scan and emit -- three launches on s, two when capacity == 0.
// low: lowWidth*lowHeight float4; hitsLow / hitsHigh: rt_hit records of the two sizes; out: width*height float4;
// width*height <= 2^31 - 1 (callers refuse larger frames first); capacity <= 2^32 - 1 (the caller saturates it)
hipError_t rt_launch_upsample(const void *low, const void *hitsLow, const void *hitsHigh, void *out, const RtUpsampleRule &rule, void *pixels,
                              unsigned capacity, void *scratch, void *selState, hipStream_t s);
// rt_image_put_at: image[pixels[k]] = samples[k], one lane per entry.  n >= 1, at most one grid of 256-lane workgroups
hipError_t rt_launch_image_put_at(const void *samples, const void *pixels, size_t n, void *image, int width, int height, hipStream_t s);
