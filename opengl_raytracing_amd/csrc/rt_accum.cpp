// rt_accum.cpp -- progressive accumulation's entry points of the C ABI (include/rt_mi355.h has the contract of each):
// rt_accum_layout, rt_accum_reset, rt_accum_add, rt_accum_view and the host's run of the solve, rt_accum_solve_host.  The
// accumulator and the state are the caller's; the context keeps nothing of this feature.  The kernels are rt_accum.hip's.
#include <math.h>
#include <string.h>

#include "rt_context.h"
#include "rt_accum.h"
#include "rt_accum_solve.h"

namespace {

constexpr uint64_t kAccumMaxPixels = 0x7fffffffull;

// the description's own rules, in the order the header lists them; *rule is what the kernels take
int validate_accum_desc(rt_context *c, const rt_accum_desc *d, RtAccumRule *rule) {
    if (!d) return fail(c, RT_ERR_INVALID_ARG, "accumulation description is NULL");
    if (d->width < 1 || d->height < 1) return fail(c, RT_ERR_INVALID_ARG, "width/height must be positive");
    if (!(d->relError > 0.0f) || !(d->relError < HUGE_VALF)) return fail(c, RT_ERR_INVALID_ARG, "relError must be finite and > 0");
    if (!(d->lumFloor >= 0x1p-40f) || !(d->lumFloor < HUGE_VALF)) return fail(c, RT_ERR_INVALID_ARG, "lumFloor must be finite and >= 2^-40");
    if (d->minSamples < 2) return fail(c, RT_ERR_INVALID_ARG, "minSamples must be >= 2");
    if (d->donePermille < 1 || d->donePermille > 1000) return fail(c, RT_ERR_INVALID_ARG, "donePermille must be in 1..1000");
    if (d->reserved[0] || d->reserved[1] || d->reserved[2] || d->reserved[3]) return fail(c, RT_ERR_INVALID_ARG, "reserved words must be zero");
    if (rule) {
        rule->lumFloor = d->lumFloor;
        rule->thr2 = d->relError * d->relError;
        rule->minSamples = (unsigned)d->minSamples;
        rule->donePermille = d->donePermille;
    }
    return RT_OK;
}

int validate_pointer(rt_context *c, const void *p, const char *what) {
    if (!p || ((uintptr_t)p & 15u)) return fail(c, RT_ERR_INVALID_ARG, what);
    return RT_OK;
}

bool overlaps(const void *a, size_t aBytes, const void *b, size_t bBytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + bBytes && b0 < a0 + aBytes;
}

}  // namespace

extern "C" {

int rt_accum_layout(int width, int height, size_t offset[2], size_t *bytes) {
    if (!offset || width < 1 || height < 1) return RT_ERR_INVALID_ARG;
    const uint64_t npx = (uint64_t)width * (uint64_t)height;
    if (npx > kAccumMaxPixels) return RT_ERR_TOO_LARGE;
    offset[0] = 0;
    offset[1] = (size_t)npx * 16;
    if (bytes) *bytes = (size_t)npx * 32;
    return RT_OK;
}

int rt_accum_reset(rt_context *c, void *dAccum, void *dState, int width, int height, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (width < 1 || height < 1) return fail(c, RT_ERR_INVALID_ARG, "width/height must be positive");
    int rc;
    if ((rc = validate_pointer(c, dAccum, "the accumulator pointer must be non-NULL and 16-byte aligned"))) return rc;
    if ((rc = validate_pointer(c, dState, "the state pointer must be non-NULL and 16-byte aligned"))) return rc;
    const uint64_t npx = (uint64_t)width * (uint64_t)height;
    if (npx > kAccumMaxPixels) return fail(c, RT_ERR_TOO_LARGE, "more than 2^31 - 1 pixels");
    if (overlaps(dState, sizeof(rt_accum_state), dAccum, (size_t)npx * 32)) return fail(c, RT_ERR_INVALID_ARG, "the state overlaps the accumulator");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = stream_or_own(c, hipStream);
    HIP_TRY(c, hipMemsetAsync(dAccum, 0, (size_t)npx * 32, s));
    HIP_TRY(c, hipMemsetAsync(dState, 0, sizeof(rt_accum_state), s));
    return RT_OK;
}

int rt_accum_add(rt_context *c, const void *dImage, void *dAccum, const rt_accum_desc *d, void *dState, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    RtAccumRule rule;
    int rc = validate_accum_desc(c, d, &rule);
    if (rc) return rc;
    if ((rc = validate_pointer(c, dImage, "the image pointer must be non-NULL and 16-byte aligned"))) return rc;
    if ((rc = validate_pointer(c, dAccum, "the accumulator pointer must be non-NULL and 16-byte aligned"))) return rc;
    if ((rc = validate_pointer(c, dState, "the state pointer must be non-NULL and 16-byte aligned"))) return rc;
    const uint64_t npx = (uint64_t)d->width * (uint64_t)d->height;
    if (npx > kAccumMaxPixels) return fail(c, RT_ERR_TOO_LARGE, "more than 2^31 - 1 pixels");
    if (overlaps(dImage, (size_t)npx * 16, dAccum, (size_t)npx * 32)) return fail(c, RT_ERR_INVALID_ARG, "the image overlaps the accumulator");
    if (overlaps(dState, sizeof(rt_accum_state), dAccum, (size_t)npx * 32)) return fail(c, RT_ERR_INVALID_ARG, "the state overlaps the accumulator");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, rt_launch_accum_add(dImage, dAccum, dState, (unsigned)npx, rule, stream_or_own(c, hipStream)));
    return RT_OK;
}

int rt_accum_view(rt_context *c, const void *dAccum, void *dOut, const rt_accum_desc *d, int mode, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    RtAccumRule rule;
    int rc = validate_accum_desc(c, d, &rule);
    if (rc) return rc;
    if (mode != RT_ACCUM_VIEW_RELERR && mode != RT_ACCUM_VIEW_COUNT && mode != RT_ACCUM_VIEW_CONVERGED)
        return fail(c, RT_ERR_INVALID_ARG, "unknown accumulation view mode");
    if ((rc = validate_pointer(c, dAccum, "the accumulator pointer must be non-NULL and 16-byte aligned"))) return rc;
    if ((rc = validate_pointer(c, dOut, "the output pointer must be non-NULL and 16-byte aligned"))) return rc;
    const uint64_t npx = (uint64_t)d->width * (uint64_t)d->height;
    if (npx > kAccumMaxPixels) return fail(c, RT_ERR_TOO_LARGE, "more than 2^31 - 1 pixels");
    if (overlaps(dOut, (size_t)npx * 16, dAccum, (size_t)npx * 32)) return fail(c, RT_ERR_INVALID_ARG, "the output overlaps the accumulator");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, rt_launch_accum_view(dAccum, dOut, (unsigned)npx, rule, mode, stream_or_own(c, hipStream)));
    return RT_OK;
}

int rt_accum_solve_host(const rt_accum_state *in, const rt_accum_desc *d, rt_accum_state *out) {
    if (!in || !out) return RT_ERR_INVALID_ARG;
    int rc = validate_accum_desc(nullptr, d, nullptr);
    if (rc) return rc;
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
