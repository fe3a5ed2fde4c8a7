// rt_resample.cpp -- the resampler's entry points of the C ABI (include/rt_mi355.h has the contract of each): rt_resample_taps,
// the one builder of the tap tables, and rt_display_resample, which keeps the device copies of the two axis tables in the
// context (ResampleTables, rt_resample.h) and launches rt_resample.hip's kernel.
#include <math.h>
#include <string.h>

#include <new>

#include "rt_args.h"
#include "rt_resample.h"

namespace {

// sinc, exactly 1 at 0 and exactly 0 at every other x that is an integer in double
double sinc(double x) {
    if (x == 0.0) return 1.0;
    if (x == floor(x)) return 0.0;
    const double px = M_PI * x;
    return sin(px) / px;
}

double kernel_value(int filter, double x) {
    x = fabs(x);
    if (filter == RT_RESAMPLE_TRIANGLE) return x < 1.0 ? 1.0 - x : 0.0;
    return x < 3.0 ? sinc(x) * sinc(x / 3.0) : 0.0;
}

int64_t floor_div(int64_t a, int64_t b) {       // b > 0
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// The window of destination index i, [*j0, *j1], decided in integers so that no rounding moves a pixel across its edge.
// AREA: the source pixels the destination pixel's footprint [iS, (i+1)S) / D touches.  TRIANGLE / LANCZOS3: the pixels
// strictly inside c +- R fs, c = ((2i+1)S - D) / 2D, fs = max(1, S/D): with M = max(S, D) that is |2Dj - (2i+1)S + D| < 2RM.
void window(int S, int D, int filter, int i, int64_t *j0, int64_t *j1) {
    const int64_t s = S, d = D;
    if (filter == RT_RESAMPLE_AREA) {
        *j0 = (i * s) / d;
        *j1 = ((i + 1) * s + d - 1) / d - 1;
        return;
    }
    const int64_t R = filter == RT_RESAMPLE_TRIANGLE ? 1 : 3, M = s > d ? s : d;
    const int64_t c2 = (2 * (int64_t)i + 1) * s - d;            // 2D c
    *j0 = floor_div(c2 - 2 * R * M, 2 * d) + 1;                 // the first j with 2Dj > c2 - 2RM
    *j1 = floor_div(c2 + 2 * R * M - 1, 2 * d);                 // the last j with 2Dj < c2 + 2RM
}

}  // namespace

int rt_resample_build_axis(int S, int D, int filter, int *nTaps, RtResampleAxis *out) {
    if (S < 1 || D < 1) return RT_ERR_INVALID_ARG;
    if (filter != RT_RESAMPLE_AREA && filter != RT_RESAMPLE_TRIANGLE && filter != RT_RESAMPLE_LANCZOS3) return RT_ERR_INVALID_ARG;
    if (S > kResampleMaxAxis || D > kResampleMaxAxis) return RT_ERR_TOO_LARGE;
    int64_t n = 0;
    for (int i = 0; i < D; i++) {
        int64_t j0, j1;
        window(S, D, filter, i, &j0, &j1);
        if (j1 - j0 + 1 > n) n = j1 - j0 + 1;
    }
    if (n > RT_RESAMPLE_MAX_TAPS) return RT_ERR_TOO_LARGE;
    if (nTaps) *nTaps = (int)n;
    if (!out) return RT_OK;
    out->n = (int)n;
    out->first.assign((size_t)D, 0);
    out->weights.assign((size_t)D * (size_t)n, 0.0f);
    const int64_t s = S, d = D, M = s > d ? s : d;
    double f[RT_RESAMPLE_MAX_TAPS];
    for (int i = 0; i < D; i++) {
        int64_t j0, j1;
        window(S, D, filter, i, &j0, &j1);
        out->first[(size_t)i] = (int32_t)j0;
        float *w = &out->weights[(size_t)i * (size_t)n];
        if (filter == RT_RESAMPLE_AREA) {
            for (int64_t j = j0; j <= j1; j++) {
                const int64_t hi = (i + 1) * s < (j + 1) * d ? (i + 1) * s : (j + 1) * d, lo = i * s > j * d ? i * s : j * d;
                w[j - j0] = (float)((double)(hi - lo) / (double)S);
            }
            continue;
        }
        // x = (j - c) / fs = (2Dj - (2i+1)S + D) / 2M: one quotient of integers, so mirrored indices get mirrored x exactly
        double sum = 0.0;
        for (int64_t j = j0; j <= j1; j++) {
            const int64_t num = 2 * d * j - (2 * (int64_t)i + 1) * s + d;
            sum += f[j - j0] = kernel_value(filter, (double)num / (double)(2 * M));
        }
        for (int64_t j = j0; j <= j1; j++) w[j - j0] = (float)(f[j - j0] / sum);
    }
    return RT_OK;
}

// ---- the device copies of the tables
int ResampleTables::update(Axis &a, int S, int D, int filter, bool transposed) {
    if (a.filter == filter && a.S == S && a.D == D) return RT_OK;
    RtResampleAxis t;
    RT_TRY(rt_resample_build_axis(S, D, filter, nullptr, &t));
    auto hip = [&](const char *call, hipError_t e) {
        if (e == hipSuccess) return false;
        failed = call;
        failedHip = e;
        a.filter = -1;                          // whatever the buffers hold now is no table of any key
        return true;
    };
    if (hip("hipEventSynchronize(resample tables)", drain())) return RT_ERR_HIP;    // the last launch that read the old tables
    a.filter = -1;
    if (hip("hipMalloc(resample first)", a.dFirst.grow(t.first.size()))) return RT_ERR_HIP;
    if (hip("hipMalloc(resample weights)", a.dWeights.grow(t.weights.size()))) return RT_ERR_HIP;
    std::vector<float> tw;
    if (transposed) {
        tw.resize(t.weights.size());
        for (int i = 0; i < D; i++)
            for (int k = 0; k < t.n; k++) tw[(size_t)k * D + i] = t.weights[(size_t)i * t.n + k];
    }
    const std::vector<float> &w = transposed ? tw : t.weights;
    if (hip("hipMemcpy(resample first)", hipMemcpy(a.dFirst, t.first.data(), t.first.size() * sizeof(int32_t), hipMemcpyHostToDevice))) return RT_ERR_HIP;
    if (hip("hipMemcpy(resample weights)", hipMemcpy(a.dWeights, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice))) return RT_ERR_HIP;
    a.first.swap(t.first);
    a.n = t.n;
    a.S = S; a.D = D; a.filter = filter;
    return RT_OK;
}

int ResampleTables::prepare(int srcW, int srcH, int dstW, int dstH, int filter) {
    failed = "";
    failedHip = hipSuccess;
    // both axes are checked before either is rebuilt: a refused shape leaves the tables of the last good one in place
    int rc = rt_resample_build_axis(srcW, dstW, filter, nullptr, nullptr);
    if (!rc) rc = rt_resample_build_axis(srcH, dstH, filter, nullptr, nullptr);
    if (!rc) rc = update(x, srcW, dstW, filter, true);
    if (!rc) rc = update(y, srcH, dstH, filter, false);
    return rc;
}

extern "C" {

int rt_resample_taps(int srcSize, int dstSize, int filter, int *nTaps, int32_t *first, float *weights, size_t capWeights) {
    if (!nTaps || (first == nullptr) != (weights == nullptr)) return RT_ERR_INVALID_ARG;
    int n = 0;
    int rc = rt_resample_build_axis(srcSize, dstSize, filter, &n, nullptr);
    if (rc) return rc;
    if (!first) {
        *nTaps = n;
        return RT_OK;
    }
    if ((size_t)dstSize * (size_t)n > capWeights) return RT_ERR_TOO_LARGE;
    RtResampleAxis t;
    try {
        rc = rt_resample_build_axis(srcSize, dstSize, filter, &n, &t);
    } catch (const std::bad_alloc &) {
        return RT_ERR_TOO_LARGE;
    }
    if (rc) return rc;
    *nTaps = n;
    memcpy(first, t.first.data(), t.first.size() * sizeof(int32_t));
    memcpy(weights, t.weights.data(), t.weights.size() * sizeof(float));
    return RT_OK;
}

int rt_display_resample(rt_context *c, const void *dSrc, void *dDst, const rt_resample_desc *d, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!d) return fail(c, RT_ERR_INVALID_ARG, "resample description is NULL");
    if (d->srcWidth < 1 || d->srcHeight < 1 || d->dstWidth < 1 || d->dstHeight < 1) return fail(c, RT_ERR_INVALID_ARG, "every size must be positive");
    if (d->filter != RT_RESAMPLE_AREA && d->filter != RT_RESAMPLE_TRIANGLE && d->filter != RT_RESAMPLE_LANCZOS3)
        return fail(c, RT_ERR_INVALID_ARG, "unknown resample filter");
    if (d->flags) return fail(c, RT_ERR_INVALID_ARG, "unknown resample flag bits");
    RT_TRY(rt_check_reserved(c, d->reserved));
    RT_TRY(rt_check_pointers(c, {{dSrc, "source"}, {dDst, "destination"}}));
    const size_t srcBytes = (size_t)d->srcWidth * d->srcHeight * 16, dstBytes = (size_t)d->dstWidth * d->dstHeight * 16;
    if (overlaps({dSrc, srcBytes}, {dDst, dstBytes})) return fail(c, RT_ERR_INVALID_ARG, "rt_display_resample cannot run in place: source and destination overlap");
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    try {
        rc = c->resample.prepare(d->srcWidth, d->srcHeight, d->dstWidth, d->dstHeight, d->filter);
    } catch (const std::bad_alloc &) {
        return fail(c, RT_ERR_TOO_LARGE, "no host memory for the tap tables");
    }
    if (rc == RT_ERR_TOO_LARGE) return fail(c, rc, "an axis needs more than RT_RESAMPLE_MAX_TAPS taps or is longer than 2^20 pixels");
    if (rc) return fail(c, rc, c->resample.failed, c->resample.failedHip);
    const ResampleTables::Axis &y = c->resample.y;
    const RtResamplePlan plan = rt_resample_plan(y.first.data(), y.n, d->srcHeight, d->dstWidth, d->dstHeight);
    if ((uint64_t)plan.tilesX * plan.tilesY > 0x7fffffffull) return fail(c, RT_ERR_TOO_LARGE, "more tiles than one resample launch holds");
    hipStream_t s = stream_or_own(c, hipStream);
    HIP_TRY(c, c->resample.acquire(s));
    HIP_TRY(c, rt_launch_resample(dSrc, dDst, d->srcWidth, d->srcHeight, d->dstWidth, d->dstHeight, c->resample, plan, s));
    HIP_TRY(c, c->resample.release(s));
    return RT_OK;
}

}  // extern "C"
