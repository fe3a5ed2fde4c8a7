// rt_args.h -- the argument checks the image stages' entry points share (rt_display.cpp, rt_jpeg.cpp, rt_accum.cpp, rt_denoise.cpp,
// rt_resample.cpp, rt_adaptive.cpp, rt_upsample.cpp): pointers, overlapping device ranges, the pixel limit, reserved words.  One
// definition each; an entry point keeps its own order of checks.  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

// ---- the rules themselves: no HIP type and no context, so they are tested without a GPU (tests/test_args_host.py defines
// RT_ARGS_RULES_ONLY and includes nothing but this part)
inline bool rt_aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// `bytes` bytes of device memory at p.  Two ranges overlap when they share a byte: adjacent ones do not, an empty one overlaps nothing.
struct DevRange { const void *p; size_t bytes; };
inline bool overlaps(const DevRange &a, const DevRange &b) {
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a.bytes && b.bytes && a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

// The most pixels a frame of these stages has (their kernels index pixels with 32 bits), and width * height for width, height >= 1
// in 64 bits, or 0 when that is more
constexpr uint64_t kRtMaxPixels = 0x7fffffffull;
inline uint64_t rt_pixel_count(int width, int height) {
    const uint64_t npx = (uint64_t)width * (uint64_t)height;
    return npx > kRtMaxPixels ? 0 : npx;
}

template <size_t N>
inline bool rt_all_zero(const int32_t (&words)[N]) {
    for (int32_t w : words)
        if (w) return false;
    return true;
}

#ifndef RT_ARGS_RULES_ONLY
#include <initializer_list>

#include "rt_context.h"

// ---- the refusals: RT_OK, or the status with rt_last_error's text set (c may be NULL: the status alone)
// In the order given: "the <name> pointer must be non-NULL and 16-byte aligned"; an optional pointer may be NULL
struct RtPointerArg { const void *p; const char *name; bool optional = false; };
inline int rt_check_pointers(rt_context *c, std::initializer_list<RtPointerArg> args) {
    for (const RtPointerArg &a : args)
        if ((!a.p && !a.optional) || !rt_aligned16(a.p))
            return fail(c, RT_ERR_INVALID_ARG, (std::string("the ") + a.name + (a.optional ? " pointer must be 16-byte aligned" : " pointer must be non-NULL and 16-byte aligned")).c_str());
    return RT_OK;
}

// A list of rt_pixel records: 8-byte aligned, and non-NULL where the call reads or writes an entry
inline int rt_check_pixel_pointer(rt_context *c, const void *p, bool required) {
    if ((!p && required) || ((uintptr_t)p & 7u)) return fail(c, RT_ERR_INVALID_ARG, required ? "the pixel list pointer must be non-NULL and 8-byte aligned" : "the pixel list pointer must be 8-byte aligned");
    return RT_OK;
}

// *npx = width * height (both >= 1, checked by the caller first), or RT_ERR_TOO_LARGE
inline int rt_check_pixels(rt_context *c, int width, int height, uint64_t *npx) {
    return (*npx = rt_pixel_count(width, height)) ? RT_OK : fail(c, RT_ERR_TOO_LARGE, "more than 2^31 - 1 pixels");
}

template <size_t N>
inline int rt_check_reserved(rt_context *c, const int32_t (&words)[N]) {
    return rt_all_zero(words) ? RT_OK : fail(c, RT_ERR_INVALID_ARG, "reserved words must be zero");
}

// rt_accum_layout / rt_denoise_layout: two planes of width x height float4, one behind the other (no context: the status alone)
inline int rt_two_plane_layout(int width, int height, size_t offset[2], size_t *bytes) {
    if (!offset || width < 1 || height < 1) return RT_ERR_INVALID_ARG;
    const uint64_t npx = rt_pixel_count(width, height);
    if (!npx) return RT_ERR_TOO_LARGE;
    offset[0] = 0;
    offset[1] = (size_t)npx * 16;
    if (bytes) *bytes = (size_t)npx * 32;
    return RT_OK;
}
#endif
