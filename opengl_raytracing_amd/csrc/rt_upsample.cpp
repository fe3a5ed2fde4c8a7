// rt_upsample.cpp -- first-hit-guided upsampling's entry points of the C ABI (include/rt_mi355.h has the contract of each):
// rt_upsample_layout, rt_upsample, rt_image_put_at.  Every buffer is the caller's; the context keeps nothing of this feature.
// The kernels are rt_upsample.hip's; the list is made by rt_adaptive.hip's scan and emit.
#include "rt_args.h"
#include "rt_adaptive.h"
#include "rt_upsample.h"

namespace {

constexpr size_t kMaxListed = (size_t)0x7fffffff * 256;     // one grid of 256-lane workgroups

// the description's own rules, in the order the header lists them; *rule is what the kernel takes
int validate_upsample_desc(rt_context *c, const rt_upsample_desc *d, RtUpsampleRule *rule) {
    if (!d) return fail(c, RT_ERR_INVALID_ARG, "upsample description is NULL");
    if (d->width < 1 || d->height < 1) return fail(c, RT_ERR_INVALID_ARG, "width/height must be positive");
    if (d->lowWidth < 1 || d->lowWidth > d->width) return fail(c, RT_ERR_INVALID_ARG, "lowWidth must be in 1..width");
    if (d->lowHeight < 1 || d->lowHeight > d->height) return fail(c, RT_ERR_INVALID_ARG, "lowHeight must be in 1..height");
    if (d->normalLog2Power < 0 || d->normalLog2Power > 7) return fail(c, RT_ERR_INVALID_ARG, "normalLog2Power must be in 0..7");
    if (!(d->minWeight >= 0.0f) || !(d->minWeight <= 1.0f)) return fail(c, RT_ERR_INVALID_ARG, "minWeight must be in 0..1");
    RT_TRY(rt_check_reserved(c, d->reserved));
    rule->width = d->width;
    rule->height = d->height;
    rule->lowWidth = d->lowWidth;
    rule->lowHeight = d->lowHeight;
    rule->normalLog2Power = d->normalLog2Power;
    rule->minWeight = d->minWeight;
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_upsample_layout(int width, int height, size_t *scratchBytes) { return rt_accum_select_layout(width, height, scratchBytes); }

int rt_upsample(rt_context *c, const void *dLow, const void *dHitsLow, const void *dHitsHigh, void *dOut, const rt_upsample_desc *d,
                void *dPixels, size_t capacity, void *dScratch, void *dSelState, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    RtUpsampleRule rule;
    RT_TRY(validate_upsample_desc(c, d, &rule));
    RT_TRY(rt_check_pointers(c, {{dLow, "low-resolution image"}, {dHitsLow, "low-resolution hits"}, {dHitsHigh, "full-resolution hits"},
                                 {dOut, "output"}, {dScratch, "scratch"}, {dSelState, "select state"}}));
    RT_TRY(rt_check_pixel_pointer(c, dPixels, capacity != 0));
    uint64_t npx;
    RT_TRY(rt_check_pixels(c, d->width, d->height, &npx));
    const size_t nLow = (size_t)d->lowWidth * (size_t)d->lowHeight;                 // <= npx
    const size_t listed = capacity < npx ? capacity : (size_t)npx;                  // the most entries a call writes
    const DevRange inputs[3] = {{dLow, nLow * 16}, {dHitsLow, nLow * sizeof(rt_hit)}, {dHitsHigh, (size_t)npx * sizeof(rt_hit)}};
    const DevRange outputs[4] = {{dOut, (size_t)npx * 16}, {dPixels, listed * sizeof(rt_pixel)},
                                 {dScratch, rt_select_scratch_bytes(d->width, d->height)}, {dSelState, sizeof(rt_select_state)}};
    static const char *const overlapsInput[4] = {"the output overlaps an input", "the pixel list overlaps an input", "the scratch overlaps an input",
                                                 "the select state overlaps an input"};
    for (int o = 0; o < 4; o++) {
        for (const DevRange &in : inputs)
            if (overlaps(outputs[o], in)) return fail(c, RT_ERR_INVALID_ARG, overlapsInput[o]);
        for (int p = 0; p < o; p++)
            if (overlaps(outputs[o], outputs[p])) return fail(c, RT_ERR_INVALID_ARG, "the output, the pixel list, the scratch and the select state must not overlap");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    const unsigned cap32 = capacity > 0xffffffffull ? 0xffffffffu : (unsigned)capacity;
    HIP_TRY(c, rt_launch_upsample(dLow, dHitsLow, dHitsHigh, dOut, rule, dPixels, cap32, dScratch, dSelState, stream_or_own(c, hipStream)));
    return RT_OK;
}

int rt_image_put_at(rt_context *c, const void *dSamples, const void *dPixels, size_t n, void *dImage, int width, int height, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (width < 1 || height < 1) return fail(c, RT_ERR_INVALID_ARG, "width/height must be positive");
    RT_TRY(rt_check_pointers(c, {{dSamples, "sample", n == 0}, {dImage, "image"}}));
    RT_TRY(rt_check_pixel_pointer(c, dPixels, n != 0));
    uint64_t npx;
    RT_TRY(rt_check_pixels(c, width, height, &npx));
    if (n > kMaxListed) return fail(c, RT_ERR_TOO_LARGE, "too many list entries in one call");
    const DevRange image = {dImage, (size_t)npx * 16};
    if (overlaps({dSamples, n * 16}, image)) return fail(c, RT_ERR_INVALID_ARG, "the samples overlap the image");
    if (overlaps({dPixels, n * sizeof(rt_pixel)}, image)) return fail(c, RT_ERR_INVALID_ARG, "the pixel list overlaps the image");
    if (!n) return RT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, rt_launch_image_put_at(dSamples, dPixels, n, dImage, width, height, stream_or_own(c, hipStream)));
    return RT_OK;
}

}  // extern "C"
