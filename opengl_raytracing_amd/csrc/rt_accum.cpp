// rt_accum.cpp -- progressive accumulation's entry points of the C ABI (include/rt_mi355.h has the contract of each):
// rt_accum_layout, rt_accum_reset, rt_accum_add, rt_accum_view and the host's run of the solve, rt_accum_solve_host.  The
// accumulator and the state are the caller's; the context keeps nothing of this feature.  The kernels are rt_accum.hip's.
#include <math.h>
#include <string.h>

#include "rt_args.h"
#include "rt_accum.h"
#include "rt_accum_solve.h"

// the description's own rules, in the order the header lists them; *rule is what the kernels take (rt_adaptive.cpp asks too)
int rt_validate_accum_desc(rt_context *c, const rt_accum_desc *d, RtAccumRule *rule) {
    if (!d) return fail(c, RT_ERR_INVALID_ARG, "accumulation description is NULL");
    if (d->width < 1 || d->height < 1) return fail(c, RT_ERR_INVALID_ARG, "width/height must be positive");
    if (!(d->relError > 0.0f) || !(d->relError < HUGE_VALF)) return fail(c, RT_ERR_INVALID_ARG, "relError must be finite and > 0");
    if (!(d->lumFloor >= 0x1p-40f) || !(d->lumFloor < HUGE_VALF)) return fail(c, RT_ERR_INVALID_ARG, "lumFloor must be finite and >= 2^-40");
    if (d->minSamples < 2) return fail(c, RT_ERR_INVALID_ARG, "minSamples must be >= 2");
    if (d->donePermille < 1 || d->donePermille > 1000) return fail(c, RT_ERR_INVALID_ARG, "donePermille must be in 1..1000");
    RT_TRY(rt_check_reserved(c, d->reserved));
    if (rule) {
        rule->lumFloor = d->lumFloor;
        rule->thr2 = d->relError * d->relError;
        rule->minSamples = (unsigned)d->minSamples;
        rule->donePermille = d->donePermille;
    }
    return RT_OK;
}

extern "C" {

int rt_accum_layout(int width, int height, size_t offset[2], size_t *bytes) { return rt_two_plane_layout(width, height, offset, bytes); }

int rt_accum_reset(rt_context *c, void *dAccum, void *dState, int width, int height, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (width < 1 || height < 1) return fail(c, RT_ERR_INVALID_ARG, "width/height must be positive");
    RT_TRY(rt_check_pointers(c, {{dAccum, "accumulator"}, {dState, "state"}}));
    uint64_t npx;
    RT_TRY(rt_check_pixels(c, width, height, &npx));
    if (overlaps({dState, sizeof(rt_accum_state)}, {dAccum, (size_t)npx * 32})) return fail(c, RT_ERR_INVALID_ARG, "the state overlaps the accumulator");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = stream_or_own(c, hipStream);
    HIP_TRY(c, hipMemsetAsync(dAccum, 0, (size_t)npx * 32, s));
    HIP_TRY(c, hipMemsetAsync(dState, 0, sizeof(rt_accum_state), s));
    return RT_OK;
}

int rt_accum_add(rt_context *c, const void *dImage, void *dAccum, const rt_accum_desc *d, void *dState, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    RtAccumRule rule;
    RT_TRY(rt_validate_accum_desc(c, d, &rule));
    RT_TRY(rt_check_pointers(c, {{dImage, "image"}, {dAccum, "accumulator"}, {dState, "state"}}));
    uint64_t npx;
    RT_TRY(rt_check_pixels(c, d->width, d->height, &npx));
    if (overlaps({dImage, (size_t)npx * 16}, {dAccum, (size_t)npx * 32})) return fail(c, RT_ERR_INVALID_ARG, "the image overlaps the accumulator");
    if (overlaps({dState, sizeof(rt_accum_state)}, {dAccum, (size_t)npx * 32})) return fail(c, RT_ERR_INVALID_ARG, "the state overlaps the accumulator");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, rt_launch_accum_add(dImage, dAccum, dState, (unsigned)npx, rule, stream_or_own(c, hipStream)));
    return RT_OK;
}

int rt_accum_view(rt_context *c, const void *dAccum, void *dOut, const rt_accum_desc *d, int mode, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    RtAccumRule rule;
    RT_TRY(rt_validate_accum_desc(c, d, &rule));
    if (mode != RT_ACCUM_VIEW_RELERR && mode != RT_ACCUM_VIEW_COUNT && mode != RT_ACCUM_VIEW_CONVERGED)
        return fail(c, RT_ERR_INVALID_ARG, "unknown accumulation view mode");
    RT_TRY(rt_check_pointers(c, {{dAccum, "accumulator"}, {dOut, "output"}}));
    uint64_t npx;
    RT_TRY(rt_check_pixels(c, d->width, d->height, &npx));
    if (overlaps({dOut, (size_t)npx * 16}, {dAccum, (size_t)npx * 32})) return fail(c, RT_ERR_INVALID_ARG, "the output overlaps the accumulator");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, rt_launch_accum_view(dAccum, dOut, (unsigned)npx, rule, mode, stream_or_own(c, hipStream)));
    return RT_OK;
}

int rt_accum_solve_host(const rt_accum_state *in, const rt_accum_desc *d, rt_accum_state *out) {
    if (!in || !out) return RT_ERR_INVALID_ARG;
    RT_TRY(rt_validate_accum_desc(nullptr, d, nullptr));
    uint64_t n = in->nUnsampled;
    for (int b = 0; b < kAccumBins; b++) n += in->hist[b];
    if (n > 0xffffffffull) return RT_ERR_TOO_LARGE;
    const RtAccumSolved r = rt_accum_solve(in->hist, in->nConverged, in->nPixels, d->donePermille, in->frames);
    if (out != in) *out = *in;
    out->medianBin = r.medianBin;
    out->p95Bin = r.p95Bin;
    out->done = r.done;
    out->frames = r.frames;
    memset(out->reserved, 0, sizeof out->reserved);
    return RT_OK;
}

}  // extern "C"
