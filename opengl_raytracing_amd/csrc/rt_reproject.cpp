// rt_reproject.cpp -- reprojection's entry points of the C ABI (include/rt_mi355.h has the contract of each): rt_reproject_layout,
// rt_reproject_project and rt_accum_reproject.  Every buffer is the caller's; the context keeps nothing of this feature.  The kernel
// is rt_reproject.hip's, the projection rt_reproject.h's.
#include <math.h>

#include "rt_args.h"
#include "rt_reproject.h"

namespace {

// one view's own rules; *v is what the projection takes
int validate_view(rt_context *c, const rt_params &p, int width, int height, RtReprojectView *v) {
    if (p.width != width || p.height != height) return fail(c, RT_ERR_INVALID_ARG, "a view's width/height differ from the description's");
    if (!rt_reproject_view(p, v)) return fail(c, RT_ERR_INVALID_ARG, "fovDeg/focalLength give a view scale that is not finite and > 0");
    return RT_OK;
}

// the description's own rules, in the order the header lists them; *rule is what the kernel takes
int validate_reproject_desc(rt_context *c, const rt_reproject_desc *d, RtReprojectRule *rule) {
    if (!d) return fail(c, RT_ERR_INVALID_ARG, "reprojection description is NULL");
    if (d->width < 1 || d->height < 1) return fail(c, RT_ERR_INVALID_ARG, "width/height must be positive");
    RT_TRY(validate_view(c, d->prev, d->width, d->height, &rule->prev));
    RT_TRY(validate_view(c, d->cur, d->width, d->height, &rule->cur));
    if (!(d->normalCosMin >= -1.0f) || !(d->normalCosMin <= 1.0f)) return fail(c, RT_ERR_INVALID_ARG, "normalCosMin must be in [-1, 1]");
    if (!(d->planeTol >= 0.0f) || !(d->planeTol < HUGE_VALF)) return fail(c, RT_ERR_INVALID_ARG, "planeTol must be finite and >= 0");
    if (d->maxHistory < 1 || d->maxHistory > (1 << 24) - 1) return fail(c, RT_ERR_INVALID_ARG, "maxHistory must be in 1..2^24-1");
    RT_TRY(rt_check_reserved(c, d->reserved));
    rule->width = d->width;
    rule->height = d->height;
    rule->hx = 0.5f * (float)d->width;
    rule->hy = 0.5f * (float)d->height;
    rule->normalCosMin = d->normalCosMin;
    rule->planeTol = d->planeTol;
    rule->maxHistory = (unsigned)d->maxHistory;
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_reproject_layout(int width, int height, size_t offset[2], size_t *bytes) { return rt_two_plane_layout(width, height, offset, bytes); }

int rt_reproject_project(const rt_params *view, const float P[3], float f[2], int *valid) {
    if (!view || !P || !f || !valid) return RT_ERR_INVALID_ARG;
    if (view->width < 1 || view->height < 1) return RT_ERR_INVALID_ARG;
    RtReprojectView v;
    RT_TRY(validate_view(nullptr, *view, view->width, view->height, &v));
    *valid = rt_reproject_proj(v, 0.5f * (float)view->width, 0.5f * (float)view->height, P[0], P[1], P[2], &f[0], &f[1]) ? 1 : 0;
    return RT_OK;
}

int rt_accum_reproject(rt_context *c, const void *dAccumPrev, const void *dHitsPrev, const void *dHitsCur, void *dAccumCur,
                       const rt_reproject_desc *d, void *dReport, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    RtReprojectRule rule;
    RT_TRY(validate_reproject_desc(c, d, &rule));
    RT_TRY(rt_check_pointers(c, {{dAccumPrev, "previous accumulator"}, {dHitsPrev, "previous hits"}, {dHitsCur, "current hits"},
                                 {dAccumCur, "current accumulator"}, {dReport, "report"}}));
    uint64_t npx;
    RT_TRY(rt_check_pixels(c, d->width, d->height, &npx));
    const size_t bytes = (size_t)npx * 32;                  // an accumulator and a plane of rt_hit records alike
    const DevRange out = {dAccumCur, bytes}, report = {dReport, sizeof(rt_reproject_report)};
    for (const DevRange &in : {DevRange{dAccumPrev, bytes}, DevRange{dHitsPrev, bytes}, DevRange{dHitsCur, bytes}}) {
        if (overlaps(out, in)) return fail(c, RT_ERR_INVALID_ARG, "the current accumulator overlaps an input");
        if (overlaps(report, in)) return fail(c, RT_ERR_INVALID_ARG, "the report overlaps an input");
    }
    if (overlaps(report, out)) return fail(c, RT_ERR_INVALID_ARG, "the report overlaps the current accumulator");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, rt_launch_reproject(dAccumPrev, dHitsPrev, dHitsCur, dAccumCur, dReport, rule, stream_or_own(c, hipStream)));
    return RT_OK;
}

}  // extern "C"
