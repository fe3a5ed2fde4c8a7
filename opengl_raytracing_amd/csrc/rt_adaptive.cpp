// rt_adaptive.cpp -- adaptive sampling's entry points of the C ABI (include/rt_mi355.h has the contract of each):
// rt_accum_select_layout, rt_accum_select, rt_accum_add_at.  (rt_camera_rays_at, the third stage of the loop, reads the noise
// texture and lives beside rt_camera_rays in rt_abi.cpp.)  Every buffer is the caller's; the context keeps nothing of this feature.
// The kernels are rt_adaptive.hip's.
#include "rt_args.h"
#include "rt_adaptive.h"

namespace {

constexpr uint32_t kMaxSampleCap = 1u << 24;
constexpr size_t kMaxListed = (size_t)0x7fffffff * 256;     // one grid of 256-lane workgroups

}  // namespace

extern "C" {

int rt_accum_select_layout(int width, int height, size_t *scratchBytes) {
    if (!scratchBytes || width < 1 || height < 1) return RT_ERR_INVALID_ARG;
    if (!rt_pixel_count(width, height)) return RT_ERR_TOO_LARGE;
    *scratchBytes = rt_select_scratch_bytes(width, height);
    return RT_OK;
}

int rt_accum_select(rt_context *c, const void *dAccum, const rt_accum_desc *d, uint32_t maxSamples, void *dPixels, size_t capacity,
                    void *dScratch, void *dSelState, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    RtAccumRule rule;
    RT_TRY(rt_validate_accum_desc(c, d, &rule));
    if (maxSamples < 1 || maxSamples > kMaxSampleCap) return fail(c, RT_ERR_INVALID_ARG, "maxSamples must be in 1..2^24");
    RT_TRY(rt_check_pointers(c, {{dAccum, "accumulator"}, {dScratch, "scratch"}, {dSelState, "select state"}}));
    RT_TRY(rt_check_pixel_pointer(c, dPixels, capacity != 0));
    uint64_t npx;
    RT_TRY(rt_check_pixels(c, d->width, d->height, &npx));
    const DevRange accum = {dAccum, (size_t)npx * 32};
    const size_t listed = capacity < npx ? capacity : (size_t)npx;                  // the most entries a call writes
    if (overlaps({dPixels, listed * sizeof(rt_pixel)}, accum)) return fail(c, RT_ERR_INVALID_ARG, "the pixel list overlaps the accumulator");
    if (overlaps({dScratch, rt_select_scratch_bytes(d->width, d->height)}, accum)) return fail(c, RT_ERR_INVALID_ARG, "the scratch overlaps the accumulator");
    if (overlaps({dSelState, sizeof(rt_select_state)}, accum)) return fail(c, RT_ERR_INVALID_ARG, "the select state overlaps the accumulator");
    HIP_TRY(c, hipSetDevice(c->device));
    const unsigned cap32 = capacity > 0xffffffffull ? 0xffffffffu : (unsigned)capacity;
    HIP_TRY(c, rt_launch_accum_select(dAccum, d->width, d->height, rule, maxSamples, dPixels, cap32, dScratch, dSelState, stream_or_own(c, hipStream)));
    return RT_OK;
}

int rt_accum_add_at(rt_context *c, const void *dSamples, const void *dPixels, size_t n, void *dAccum, const rt_accum_desc *d, void *dState,
                    void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    RtAccumRule rule;
    RT_TRY(rt_validate_accum_desc(c, d, &rule));
    RT_TRY(rt_check_pointers(c, {{dSamples, "sample", n == 0}, {dAccum, "accumulator"}, {dState, "state"}}));
    RT_TRY(rt_check_pixel_pointer(c, dPixels, n != 0));
    uint64_t npx;
    RT_TRY(rt_check_pixels(c, d->width, d->height, &npx));
    if (n > kMaxListed) return fail(c, RT_ERR_TOO_LARGE, "too many list entries in one call");
    const DevRange accum = {dAccum, (size_t)npx * 32};
    if (overlaps({dSamples, n * 16}, accum)) return fail(c, RT_ERR_INVALID_ARG, "the samples overlap the accumulator");
    if (overlaps({dPixels, n * sizeof(rt_pixel)}, accum)) return fail(c, RT_ERR_INVALID_ARG, "the pixel list overlaps the accumulator");
    if (overlaps({dState, sizeof(rt_accum_state)}, accum)) return fail(c, RT_ERR_INVALID_ARG, "the state overlaps the accumulator");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, rt_launch_accum_add_at(dSamples, dPixels, n, dAccum, dState, d->width, d->height, rule, stream_or_own(c, hipStream)));
    return RT_OK;
}

}  // extern "C"
