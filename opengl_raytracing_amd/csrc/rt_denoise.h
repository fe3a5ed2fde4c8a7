// rt_denoise.h -- the denoiser's launch wrappers: what rt_denoise.hip implements for the entry points in rt_denoise.cpp.
// Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

// what the kernels need of a validated rt_denoise_desc
struct RtDenoiseRule {
    int width, height, iterations, normalLog2Power;
    float sigmaLum, lumEps;
    unsigned minCount;
};

// rt_denoise_guide: hits: nPixels rt_hit; guide: nPixels rt_denoise_guide_rec; one launch on s.  nPixels <= 2^31 - 1 here and
// below (callers refuse larger frames first)
hipError_t rt_launch_denoise_guide(const void *hits, void *guide, unsigned nPixels, hipStream_t s);
// rt_denoise: prepare (image, moments or NULL, guide -> scratch plane A), then rule.iterations launches that read one scratch plane
// and write the other, the last one writing out.  image, moments, guide, out: width*height float4; scratch: two such planes
hipError_t rt_launch_denoise(const void *image, const void *moments, const void *guide, void *scratch, void *out, const RtDenoiseRule &rule,
                             hipStream_t s);
