// rt_denoise.cpp -- the denoiser's entry points of the C ABI (include/rt_mi355.h has the contract of each): rt_denoise_guide,
// rt_denoise_layout, rt_denoise.  Every buffer is the caller's; the context keeps nothing of this feature.  The kernels are
// rt_denoise.hip's.
#include <math.h>

#include "rt_context.h"
#include "rt_denoise.h"

namespace {

constexpr uint64_t kDenoiseMaxPixels = 0x7fffffffull;

// the description's own rules, in the order the header lists them; *rule is what the kernels take
int validate_denoise_desc(rt_context *c, const rt_denoise_desc *d, RtDenoiseRule *rule) {
    if (!d) return fail(c, RT_ERR_INVALID_ARG, "denoise description is NULL");
    if (d->width < 1 || d->height < 1) return fail(c, RT_ERR_INVALID_ARG, "width/height must be positive");
    if (d->iterations < 1 || d->iterations > 5) return fail(c, RT_ERR_INVALID_ARG, "iterations must be in 1..5");
    if (d->normalLog2Power < 0 || d->normalLog2Power > 7) return fail(c, RT_ERR_INVALID_ARG, "normalLog2Power must be in 0..7");
    if (!(d->sigmaLum > 0.0f) || !(d->sigmaLum < HUGE_VALF)) return fail(c, RT_ERR_INVALID_ARG, "sigmaLum must be finite and > 0");
    if (!(d->lumEps >= 0x1p-40f) || !(d->lumEps < HUGE_VALF)) return fail(c, RT_ERR_INVALID_ARG, "lumEps must be finite and >= 2^-40");
    if (d->minCount < 2) return fail(c, RT_ERR_INVALID_ARG, "minCount must be >= 2");
    for (int r : d->reserved)
        if (r) return fail(c, RT_ERR_INVALID_ARG, "reserved words must be zero");
    rule->width = d->width;
    rule->height = d->height;
    rule->iterations = d->iterations;
    rule->normalLog2Power = d->normalLog2Power;
    rule->sigmaLum = d->sigmaLum;
    rule->lumEps = d->lumEps;
    rule->minCount = (unsigned)d->minCount;
    return RT_OK;
}

int validate_pointer(rt_context *c, const void *p, const char *what) {
    if (!p || ((uintptr_t)p & 15u)) return fail(c, RT_ERR_INVALID_ARG, what);
    return RT_OK;
}

struct Range {
    const void *p;
    size_t bytes;
};

bool overlaps(const Range &a, const Range &b) {
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

}  // namespace

extern "C" {

int rt_denoise_layout(int width, int height, size_t offset[2], size_t *bytes) {
    if (!offset || width < 1 || height < 1) return RT_ERR_INVALID_ARG;
    const uint64_t npx = (uint64_t)width * (uint64_t)height;
    if (npx > kDenoiseMaxPixels) return RT_ERR_TOO_LARGE;
    offset[0] = 0;
    offset[1] = (size_t)npx * 16;
    if (bytes) *bytes = (size_t)npx * 32;
    return RT_OK;
}

int rt_denoise_guide(rt_context *c, const void *dHits, void *dGuide, int width, int height, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (width < 1 || height < 1) return fail(c, RT_ERR_INVALID_ARG, "width/height must be positive");
    int rc;
    if ((rc = validate_pointer(c, dHits, "the hits pointer must be non-NULL and 16-byte aligned"))) return rc;
    if ((rc = validate_pointer(c, dGuide, "the guide pointer must be non-NULL and 16-byte aligned"))) return rc;
    const uint64_t npx = (uint64_t)width * (uint64_t)height;
    if (npx > kDenoiseMaxPixels) return fail(c, RT_ERR_TOO_LARGE, "more than 2^31 - 1 pixels");
    if (overlaps({dHits, (size_t)npx * 32}, {dGuide, (size_t)npx * 16})) return fail(c, RT_ERR_INVALID_ARG, "the guide overlaps the hits");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, rt_launch_denoise_guide(dHits, dGuide, (unsigned)npx, stream_or_own(c, hipStream)));
    return RT_OK;
}

int rt_denoise(rt_context *c, const void *dImage, const void *dMoments, const void *dGuide, void *dScratch, void *dOut,
               const rt_denoise_desc *d, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    RtDenoiseRule rule;
    int rc = validate_denoise_desc(c, d, &rule);
    if (rc) return rc;
    if ((rc = validate_pointer(c, dImage, "the image pointer must be non-NULL and 16-byte aligned"))) return rc;
    if (dMoments && (rc = validate_pointer(c, dMoments, "the moments pointer must be 16-byte aligned"))) return rc;
    if ((rc = validate_pointer(c, dGuide, "the guide pointer must be non-NULL and 16-byte aligned"))) return rc;
    if ((rc = validate_pointer(c, dScratch, "the scratch pointer must be non-NULL and 16-byte aligned"))) return rc;
    if ((rc = validate_pointer(c, dOut, "the output pointer must be non-NULL and 16-byte aligned"))) return rc;
    const uint64_t npx = (uint64_t)d->width * (uint64_t)d->height;
    if (npx > kDenoiseMaxPixels) return fail(c, RT_ERR_TOO_LARGE, "more than 2^31 - 1 pixels");
    const size_t plane = (size_t)npx * 16;
    const Range scratch = {dScratch, 2 * plane}, out = {dOut, plane};
    const Range inputs[3] = {{dImage, plane}, {dMoments, dMoments ? plane : 0}, {dGuide, plane}};
    for (const Range &in : inputs) {
        if (!in.bytes) continue;
        if (overlaps(scratch, in)) return fail(c, RT_ERR_INVALID_ARG, "the scratch planes overlap an input");
        if (overlaps(out, in)) return fail(c, RT_ERR_INVALID_ARG, "the output overlaps an input");
    }
    if (overlaps(out, scratch)) return fail(c, RT_ERR_INVALID_ARG, "the output overlaps the scratch planes");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, rt_launch_denoise(dImage, dMoments, dGuide, dScratch, dOut, rule, stream_or_own(c, hipStream)));
    return RT_OK;
}

}  // extern "C"
