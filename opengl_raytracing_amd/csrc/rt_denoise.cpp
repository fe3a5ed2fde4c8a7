// rt_denoise.cpp -- the denoiser's entry points of the C ABI (include/rt_mi355.h has the contract of each): rt_denoise_guide,
// rt_denoise_layout, rt_denoise.  Every buffer is the caller's; the context keeps nothing of this feature.  The kernels are
// rt_denoise.hip's.
#include <math.h>

#include "rt_args.h"
#include "rt_denoise.h"

namespace {

// the description's own rules, in the order the header lists them; *rule is what the kernels take
int validate_denoise_desc(rt_context *c, const rt_denoise_desc *d, RtDenoiseRule *rule) {
    if (!d) return fail(c, RT_ERR_INVALID_ARG, "denoise description is NULL");
    if (d->width < 1 || d->height < 1) return fail(c, RT_ERR_INVALID_ARG, "width/height must be positive");
    if (d->iterations < 1 || d->iterations > 5) return fail(c, RT_ERR_INVALID_ARG, "iterations must be in 1..5");
    if (d->normalLog2Power < 0 || d->normalLog2Power > 7) return fail(c, RT_ERR_INVALID_ARG, "normalLog2Power must be in 0..7");
    if (!(d->sigmaLum > 0.0f) || !(d->sigmaLum < HUGE_VALF)) return fail(c, RT_ERR_INVALID_ARG, "sigmaLum must be finite and > 0");
    if (!(d->lumEps >= 0x1p-40f) || !(d->lumEps < HUGE_VALF)) return fail(c, RT_ERR_INVALID_ARG, "lumEps must be finite and >= 2^-40");
    if (d->minCount < 2) return fail(c, RT_ERR_INVALID_ARG, "minCount must be >= 2");
    RT_TRY(rt_check_reserved(c, d->reserved));
    rule->width = d->width;
    rule->height = d->height;
    rule->iterations = d->iterations;
    rule->normalLog2Power = d->normalLog2Power;
    rule->sigmaLum = d->sigmaLum;
    rule->lumEps = d->lumEps;
    rule->minCount = (unsigned)d->minCount;
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_denoise_layout(int width, int height, size_t offset[2], size_t *bytes) { return rt_two_plane_layout(width, height, offset, bytes); }

int rt_denoise_guide(rt_context *c, const void *dHits, void *dGuide, int width, int height, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (width < 1 || height < 1) return fail(c, RT_ERR_INVALID_ARG, "width/height must be positive");
    RT_TRY(rt_check_pointers(c, {{dHits, "hits"}, {dGuide, "guide"}}));
    uint64_t npx;
    RT_TRY(rt_check_pixels(c, width, height, &npx));
    if (overlaps({dHits, (size_t)npx * 32}, {dGuide, (size_t)npx * 16})) return fail(c, RT_ERR_INVALID_ARG, "the guide overlaps the hits");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, rt_launch_denoise_guide(dHits, dGuide, (unsigned)npx, stream_or_own(c, hipStream)));
    return RT_OK;
}

int rt_denoise(rt_context *c, const void *dImage, const void *dMoments, const void *dGuide, void *dScratch, void *dOut,
               const rt_denoise_desc *d, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    RtDenoiseRule rule;
    RT_TRY(validate_denoise_desc(c, d, &rule));
    RT_TRY(rt_check_pointers(c, {{dImage, "image"}, {dMoments, "moments", true}, {dGuide, "guide"}, {dScratch, "scratch"}, {dOut, "output"}}));
    uint64_t npx;
    RT_TRY(rt_check_pixels(c, d->width, d->height, &npx));
    const size_t plane = (size_t)npx * 16;
    const DevRange scratch = {dScratch, 2 * plane}, out = {dOut, plane};
    const DevRange inputs[3] = {{dImage, plane}, {dMoments, dMoments ? plane : 0}, {dGuide, plane}};        // (an absent plane overlaps nothing)
    for (const DevRange &in : inputs) {
        if (overlaps(scratch, in)) return fail(c, RT_ERR_INVALID_ARG, "the scratch planes overlap an input");
        if (overlaps(out, in)) return fail(c, RT_ERR_INVALID_ARG, "the output overlaps an input");
    }
    if (overlaps(out, scratch)) return fail(c, RT_ERR_INVALID_ARG, "the output overlaps the scratch planes");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, rt_launch_denoise(dImage, dMoments, dGuide, dScratch, dOut, rule, stream_or_own(c, hipStream)));
    return RT_OK;
}

}  // extern "C"
