// rt_post.h -- the post passes' launch wrappers: what rt_post.hip implements for the entry points in rt_post.cpp.  Not part of
// the public ABI.
#pragma once
#include <hip/hip_runtime.h>

hipError_t rt_launch_taa_resolve(const void *current, const void *history, const void *normal, void *out, int W, int H,
                                 float blend, float jx, float jy, hipStream_t s);
// tmpA / tmpB: the rgba16f ping-pong targets, W * H uint2 each
hipError_t rt_launch_bloom(const void *scene, void *tmpA, void *tmpB, void *out, int W, int H, float threshold, float strength,
                           int iterations, hipStream_t s);
// depthPlane: W * H floats of scratch (gPosition.z as a dense plane); noise: nW * nH <= 16 texels of 4 floats
hipError_t rt_launch_ssao(const void *position, const void *normal, void *depthPlane, void *out, int W, int H, const float *noise,
                          int nW, int nH, const float *samples, const float *projection, const float *view, hipStream_t s);
hipError_t rt_launch_ssao_blur(const void *in, void *out, int W, int H, int horizontal, hipStream_t s);
// dTex: W * H uint2 of scratch (the equirect map as RGB16F); dFaces: 6 * S * S * 3 halfs
hipError_t rt_launch_equirect_to_cubemap(const float *dRgb, void *dTex, int W, int H, int S, void *dFaces, hipStream_t s);
