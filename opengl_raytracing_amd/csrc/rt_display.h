// rt_display.h -- the display path's launch wrappers and host tables: what rt_display.hip implements for the entry points
// in rt_display.cpp.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_mi355.h"

// rgba32f -> RGBA8; `out` rows tightly packed, both pointers 16-byte aligned, W * H below 2^32 quads of 4 pixels
hipError_t rt_launch_display_pack(const void *image, void *out, int W, int H, int srgb, int flip, float exposure, hipStream_t s);
const float *rt_display_thresholds();      // the 256 sRGB decision thresholds ([0] = 0), built on the host on first use
// the same pack behind a tone curve (0 none, 1 Reinhard with invW2 = 1 / white^2, 2 ACES) and, when dExposure is not NULL, with the
// exposure multiplied by that device float; (0, NULL) is rt_launch_display_pack
hipError_t rt_launch_display_pack_toned(const void *image, void *out, int W, int H, int srgb, int flip, float exposure, int tone,
                                        float invW2, const void *dExposure, hipStream_t s);
// rgba32f -> NV12 (i420 = 0) or I420: the toned pack's codes behind the integer matrix coef[12] of
// rt_display_yuv_coeffs; `out` holds W * H + 2 * ((W + 1) / 2) * ((H + 1) / 2) bytes, both pointers 16-byte aligned.
// rt_display_yuv_blocks: the lanes such a launch needs; above 0xffffff00 the frame is refused
hipError_t rt_launch_display_pack_yuv(const void *image, void *out, int W, int H, int i420, int srgb, int flip, float exposure, int tone,
                                      float invW2, const void *dExposure, const int *coef, hipStream_t s);
unsigned long long rt_display_yuv_blocks(int W, int H);
// rt_meter: clear, histogram, solve -- three operations on s; state = one rt_meter_state, nPixels <= 2^31 - 1
hipError_t rt_launch_meter(const void *image, void *state, unsigned nPixels, float key, float minExposure, float maxExposure, float adapt,
                           int lowPermille, int highPermille, hipStream_t s);
struct RtMeterTables;
const RtMeterTables &rt_meter_tables_ref();     // the solve's two tables (rt_meter.h), built on the host on first use
// A validated YUV pack, for an entry point that runs one in front of something else (rt_jpeg.cpp): rt_display_pack_yuv's checks
// of everything but the output pointer, then its launch.  `bytes` is the frame's size (rt_display_yuv_layout).
struct rt_context;
struct RtYuvPack {
    int tone = 0;
    float invW2 = 0.0f;
    const void *dExposure = nullptr;
    int32_t coef[12] = {};
    size_t bytes = 0;
};
int rt_yuv_pack_validate(rt_context *c, const void *dImage, const rt_yuv_desc *d, const rt_tone_desc *tone, RtYuvPack *out);
hipError_t rt_yuv_pack_launch(const void *dImage, void *dOut, const rt_yuv_desc *d, const RtYuvPack &p, hipStream_t s);
