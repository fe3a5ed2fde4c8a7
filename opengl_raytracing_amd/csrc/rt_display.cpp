// rt_display.cpp -- the display path's entry points of the C ABI (include/rt_mi355.h has the contract of each): RGBA8 and
// YUV 4:2:0 packing with exposure and tone, exposure metering, and the delivery of packed frames to the host through the
// present ring (rt_present.h).  The kernels are rt_display.hip's.
#include <math.h>
#include <string.h>

#include <string>

#include "rt_args.h"
#include "rt_display.h"
#include "rt_meter.h"

namespace {

// the rules an RGBA8 and a YUV description share, in the order both check them
template <size_t N>
int validate_common(rt_context *c, uint32_t flags, float exposure, const int32_t (&reserved)[N], const void *dImage) {
    if (flags & ~RT_DISPLAY_FLIP_ROWS) return fail(c, RT_ERR_INVALID_ARG, "unknown display flag bits");
    if (!(exposure > 0.0f) || !(exposure < HUGE_VALF)) return fail(c, RT_ERR_INVALID_ARG, "exposure must be finite and > 0");
    RT_TRY(rt_check_reserved(c, reserved));
    return rt_check_pointers(c, {{dImage, "image"}});
}

int validate_display(rt_context *c, const void *dImage, const rt_display_desc *d) {
    if (!d) return fail(c, RT_ERR_INVALID_ARG, "display description is NULL");
    if (d->width <= 0 || d->height <= 0) return fail(c, RT_ERR_INVALID_ARG, "width/height must be positive");
    if (d->format != RT_DISPLAY_RGBA8_LINEAR && d->format != RT_DISPLAY_RGBA8_SRGB) return fail(c, RT_ERR_INVALID_ARG, "unknown display format");
    RT_TRY(validate_common(c, d->flags, d->exposure, d->reserved, dImage));
    if ((((uint64_t)d->width + 3) / 4) * (uint64_t)d->height > 0xffffff00ull) return fail(c, RT_ERR_TOO_LARGE, "frame too large for one pack launch");
    return RT_OK;
}

// A pack's output: `entry` is the entry point's name, outBytes what it writes behind dOut (the image is npx float4).
int validate_output(rt_context *c, const char *entry, const void *dImage, size_t npx, const void *dOut, size_t outBytes) {
    RT_TRY(rt_check_pointers(c, {{dOut, "output"}}));
    if (overlaps({dImage, npx * 16}, {dOut, outBytes}))
        return fail(c, RT_ERR_INVALID_ARG, (std::string(entry) + " cannot run in place: image and output overlap").c_str());
    return RT_OK;
}

// what the toned entry points add to a display description, validated
struct ToneArgs {
    int op = RT_TONE_NONE;
    float invW2 = 0.0f;
    const void *dExposure = nullptr;
};
const rt_tone_desc kNoTone = {};        // RT_TONE_NONE, no dExposure: what the untoned entry points pass

int validate_tone(rt_context *c, const rt_tone_desc *t, ToneArgs *out) {
    if (!t) return fail(c, RT_ERR_INVALID_ARG, "tone description is NULL");
    if (t->op != RT_TONE_NONE && t->op != RT_TONE_REINHARD && t->op != RT_TONE_ACES) return fail(c, RT_ERR_INVALID_ARG, "unknown tone operator");
    if (t->op == RT_TONE_REINHARD && (!(t->white >= 1.0f / 256.0f) || !(t->white < HUGE_VALF)))
        return fail(c, RT_ERR_INVALID_ARG, "Reinhard's white must be finite and >= 1/256");
    if ((uintptr_t)t->dExposure & 3u) return fail(c, RT_ERR_INVALID_ARG, "dExposure must be 4-byte aligned");
    RT_TRY(rt_check_reserved(c, t->reserved));
    out->op = t->op;
    out->invW2 = t->op == RT_TONE_REINHARD ? 1.0f / (t->white * t->white) : 0.0f;
    out->dExposure = t->dExposure;
    return RT_OK;
}

hipError_t launch_rgba8(const void *dImage, void *dOut, const rt_display_desc *d, const ToneArgs &t, hipStream_t s) {
    return rt_launch_display_pack_toned(dImage, dOut, d->width, d->height, d->format == RT_DISPLAY_RGBA8_SRGB,
                                        (d->flags & RT_DISPLAY_FLIP_ROWS) != 0, d->exposure, t.op, t.invW2, t.dExposure, s);
}

// rt_display_pack (tone = &kNoTone: the launch is the untoned kernel's) and rt_display_pack_toned
int display_pack(rt_context *c, const char *entry, const void *dImage, void *dOut, const rt_display_desc *d, const rt_tone_desc *tone,
                 void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    RT_TRY(validate_display(c, dImage, d));
    ToneArgs t;
    RT_TRY(validate_tone(c, tone, &t));
    const size_t npx = (size_t)d->width * d->height;
    RT_TRY(validate_output(c, entry, dImage, npx, dOut, npx * 4));
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_rgba8(dImage, dOut, d, t, stream_or_own(c, hipStream)));
    return RT_OK;
}

// rt_present_submit (tone = &kNoTone) and rt_present_submit_toned
int present_submit(rt_context *c, const void *dImage, const rt_display_desc *d, const rt_tone_desc *tone, void *hipStream, uint64_t *ticket) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!ticket) return fail(c, RT_ERR_INVALID_ARG, "ticket is NULL");
    RT_TRY(validate_display(c, dImage, d));
    ToneArgs t;
    RT_TRY(validate_tone(c, tone, &t));
    PRESENT_TRY(c, enqueue((size_t)d->width * d->height * 4, stream_or_own(c, hipStream), ticket,
                           [&](void *stage, hipStream_t s) { return launch_rgba8(dImage, stage, d, t, s); }));
    return RT_OK;
}

// a validated rt_yuv_desc with its optional tone description: what the launch takes
struct YuvArgs {
    ToneArgs tone;
    int32_t coef[12];
    size_t bytes = 0;
};

int validate_yuv(rt_context *c, const void *dImage, const rt_yuv_desc *d, const rt_tone_desc *tone, YuvArgs *out) {
    if (!d) return fail(c, RT_ERR_INVALID_ARG, "YUV description is NULL");
    if (d->width < 1 || d->height < 1) return fail(c, RT_ERR_INVALID_ARG, "width/height must be positive");
    if (d->format != RT_YUV_NV12 && d->format != RT_YUV_I420) return fail(c, RT_ERR_INVALID_ARG, "unknown YUV format");
    if (rt_display_yuv_coeffs(d->matrix, d->range, out->coef) != RT_OK) return fail(c, RT_ERR_INVALID_ARG, "unknown YUV matrix or range");
    if (d->transfer != RT_DISPLAY_RGBA8_LINEAR && d->transfer != RT_DISPLAY_RGBA8_SRGB) return fail(c, RT_ERR_INVALID_ARG, "unknown transfer");
    RT_TRY(validate_common(c, d->flags, d->exposure, d->reserved, dImage));
    if (tone) RT_TRY(validate_tone(c, tone, &out->tone));
    if (rt_display_yuv_blocks(d->width, d->height) > 0xffffff00ull) return fail(c, RT_ERR_TOO_LARGE, "frame too large for one pack launch");
    size_t offset[3], pitch[3];
    (void)rt_display_yuv_layout(d, offset, pitch, &out->bytes);
    return RT_OK;
}

hipError_t launch_yuv(const void *dImage, void *dOut, const rt_yuv_desc *d, const YuvArgs &a, hipStream_t s) {
    return rt_launch_display_pack_yuv(dImage, dOut, d->width, d->height, d->format == RT_YUV_I420, d->transfer == RT_DISPLAY_RGBA8_SRGB,
                                      (d->flags & RT_DISPLAY_FLIP_ROWS) != 0, d->exposure, a.tone.op, a.tone.invW2, a.tone.dExposure, a.coef, s);
}

int validate_meter_desc(rt_context *c, const rt_meter_desc *d) {
    if (!d) return fail(c, RT_ERR_INVALID_ARG, "meter description is NULL");
    if (d->width < 1 || d->height < 1) return fail(c, RT_ERR_INVALID_ARG, "width/height must be positive");
    if (!(d->key > 0.0f) || !(d->key < HUGE_VALF)) return fail(c, RT_ERR_INVALID_ARG, "key must be finite and > 0");
    if (!(d->minExposure > 0.0f) || !(d->maxExposure < HUGE_VALF) || !(d->minExposure <= d->maxExposure))
        return fail(c, RT_ERR_INVALID_ARG, "exposure limits: 0 < minExposure <= maxExposure, both finite");
    if (!(d->adapt > 0.0f) || !(d->adapt <= 1.0f)) return fail(c, RT_ERR_INVALID_ARG, "adapt must be in (0, 1]");
    if (d->lowPermille < 0 || d->highPermille < 0 || (int64_t)d->lowPermille + d->highPermille >= 1000)
        return fail(c, RT_ERR_INVALID_ARG, "permilles: >= 0 and lowPermille + highPermille < 1000");
    return rt_check_reserved(c, d->reserved);
}

}  // namespace

int rt_yuv_pack_validate(rt_context *c, const void *dImage, const rt_yuv_desc *d, const rt_tone_desc *tone, RtYuvPack *out) {
    YuvArgs a;
    RT_TRY(validate_yuv(c, dImage, d, tone, &a));
    out->tone = a.tone.op;
    out->invW2 = a.tone.invW2;
    out->dExposure = a.tone.dExposure;
    memcpy(out->coef, a.coef, sizeof a.coef);
    out->bytes = a.bytes;
    return RT_OK;
}

hipError_t rt_yuv_pack_launch(const void *dImage, void *dOut, const rt_yuv_desc *d, const RtYuvPack &p, hipStream_t s) {
    return rt_launch_display_pack_yuv(dImage, dOut, d->width, d->height, d->format == RT_YUV_I420, d->transfer == RT_DISPLAY_RGBA8_SRGB,
                                      (d->flags & RT_DISPLAY_FLIP_ROWS) != 0, d->exposure, p.tone, p.invW2, p.dExposure, p.coef, s);
}

extern "C" {

// ---- RGBA8 packing
int rt_display_srgb_thresholds(float out[256]) {
    if (!out) return RT_ERR_INVALID_ARG;
    memcpy(out, rt_display_thresholds(), 256 * sizeof(float));
    return RT_OK;
}

int rt_display_pack(rt_context *c, const void *dImage, void *dOut, const rt_display_desc *d, void *hipStream) {
    return display_pack(c, "rt_display_pack", dImage, dOut, d, &kNoTone, hipStream);
}

int rt_display_pack_toned(rt_context *c, const void *dImage, void *dOut, const rt_display_desc *d, const rt_tone_desc *tone, void *hipStream) {
    return display_pack(c, "rt_display_pack_toned", dImage, dOut, d, tone, hipStream);
}

// ---- YUV 4:2:0 output
int rt_display_yuv_coeffs(int matrix, int range, int32_t out[12]) {
    if (!out || (matrix != RT_YUV_BT709 && matrix != RT_YUV_BT601) || (range != RT_YUV_LIMITED && range != RT_YUV_FULL)) return RT_ERR_INVALID_ARG;
    const double Kr = matrix == RT_YUV_BT709 ? 0.2126 : 0.299, Kb = matrix == RT_YUV_BT709 ? 0.0722 : 0.114;
    const double sY = range == RT_YUV_LIMITED ? 219.0 / 255.0 : 1.0, sC = range == RT_YUV_LIMITED ? 224.0 / 255.0 : 1.0;
    auto rne = [](double x) { return (int32_t)nearbyint(x); };       // (the default rounding mode: to nearest, ties to even)
    const int32_t cYR = rne(65536.0 * Kr * sY), cYB = rne(65536.0 * Kb * sY), cYG = rne(65536.0 * sY) - cYR - cYB;
    const int32_t cC = rne(32768.0 * sC);
    const int32_t cBR = rne(-65536.0 * sC * Kr / (2.0 * (1.0 - Kb))), cRB = rne(-65536.0 * sC * Kb / (2.0 * (1.0 - Kr)));
    const int32_t t[12] = {cYR, cYG, cYB, range == RT_YUV_LIMITED ? 16 : 0, cBR, -cC - cBR, cC, 0, cC, -cC - cRB, cRB, 0};
    memcpy(out, t, sizeof t);
    return RT_OK;
}

int rt_display_yuv_layout(const rt_yuv_desc *d, size_t offset[3], size_t pitch[3], size_t *bytes) {
    if (!d || !offset || !pitch) return RT_ERR_INVALID_ARG;
    if (d->width < 1 || d->height < 1 || (d->format != RT_YUV_NV12 && d->format != RT_YUV_I420)) return RT_ERR_INVALID_ARG;
    const size_t W = (size_t)d->width, H = (size_t)d->height, cw = (W + 1) / 2, ch = (H + 1) / 2;
    offset[0] = 0;
    offset[1] = W * H;
    pitch[0] = W;
    if (d->format == RT_YUV_NV12) {
        offset[2] = offset[1] + 1;
        pitch[1] = pitch[2] = 2 * cw;
    } else {
        offset[2] = offset[1] + cw * ch;
        pitch[1] = pitch[2] = cw;
    }
    if (bytes) *bytes = W * H + 2 * cw * ch;
    return RT_OK;
}

int rt_display_pack_yuv(rt_context *c, const void *dImage, void *dOut, const rt_yuv_desc *d, const rt_tone_desc *tone, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    YuvArgs a;
    RT_TRY(validate_yuv(c, dImage, d, tone, &a));
    RT_TRY(validate_output(c, "rt_display_pack_yuv", dImage, (size_t)d->width * d->height, dOut, a.bytes));
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_yuv(dImage, dOut, d, a, stream_or_own(c, hipStream)));
    return RT_OK;
}

// ---- exposure metering (the solve is rt_meter.h's, here and on the device)
int rt_meter(rt_context *c, const void *dImage, const rt_meter_desc *d, void *dState, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    RT_TRY(validate_meter_desc(c, d));
    RT_TRY(rt_check_pointers(c, {{dImage, "image"}, {dState, "state"}}));
    uint64_t npx;
    RT_TRY(rt_check_pixels(c, d->width, d->height, &npx));
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, rt_launch_meter(dImage, dState, (unsigned)npx, d->key, d->minExposure, d->maxExposure, d->adapt, d->lowPermille,
                               d->highPermille, stream_or_own(c, hipStream)));
    return RT_OK;
}

int rt_meter_solve_host(const rt_meter_state *in, const rt_meter_desc *d, rt_meter_state *out) {
    if (!in || !out) return RT_ERR_INVALID_ARG;
    RT_TRY(validate_meter_desc(nullptr, d));
    uint64_t n = 0;
    for (int b = 0; b < 256; b++) n += in->hist[b];
    if (n > 0xffffffffull) return RT_ERR_TOO_LARGE;
    RtMeterSolveIn si;
    si.key = d->key; si.minExposure = d->minExposure; si.maxExposure = d->maxExposure; si.adapt = d->adapt;
    si.lowPermille = d->lowPermille; si.highPermille = d->highPermille;
    si.prevExposure = in->exposure;
    si.prevFrames = in->frames;
    const RtMeterSolved r = rt_meter_solve(in->hist, si, rt_meter_tables_ref());
    if (out != in) *out = *in;
    out->nMetered = r.nMetered;
    out->meanLog2Q16 = r.meanLog2Q16;
    out->target = r.target;
    out->exposure = r.exposure;
    out->frames = r.frames;
    memset(out->reserved, 0, sizeof out->reserved);
    return RT_OK;
}

int rt_meter_tables(float pow2neg[256], uint32_t log2q16[8]) {
    if (!pow2neg || !log2q16) return RT_ERR_INVALID_ARG;
    const RtMeterTables &t = rt_meter_tables_ref();
    memcpy(pow2neg, t.pow2neg, sizeof t.pow2neg);
    memcpy(log2q16, t.log2q16, sizeof t.log2q16);
    return RT_OK;
}

// ---- delivery to the host: the ring keeps its own rules (rt_present.h)
int rt_present_configure(rt_context *c, int slots) {
    if (!c) return RT_ERR_INVALID_ARG;
    PRESENT_TRY(c, configure(slots));
    return RT_OK;
}

int rt_present_submit(rt_context *c, const void *dImage, const rt_display_desc *d, void *hipStream, uint64_t *ticket) {
    return present_submit(c, dImage, d, &kNoTone, hipStream, ticket);
}

int rt_present_submit_toned(rt_context *c, const void *dImage, const rt_display_desc *d, const rt_tone_desc *tone, void *hipStream,
                            uint64_t *ticket) {
    return present_submit(c, dImage, d, tone, hipStream, ticket);
}

int rt_present_submit_yuv(rt_context *c, const void *dImage, const rt_yuv_desc *d, const rt_tone_desc *tone, void *hipStream, uint64_t *ticket) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!ticket) return fail(c, RT_ERR_INVALID_ARG, "ticket is NULL");
    YuvArgs a;
    RT_TRY(validate_yuv(c, dImage, d, tone, &a));
    PRESENT_TRY(c, enqueue(a.bytes, stream_or_own(c, hipStream), ticket,
                           [&](void *stage, hipStream_t s) { return launch_yuv(dImage, stage, d, a, s); }));
    return RT_OK;
}

int rt_present_poll(rt_context *c, uint64_t ticket, int *ready) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!ready) return fail(c, RT_ERR_INVALID_ARG, "ready is NULL");
    *ready = 0;
    PRESENT_TRY(c, poll(ticket, ready));
    return RT_OK;
}

int rt_present_wait(rt_context *c, uint64_t ticket, const void **hostPixels, size_t *bytes) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!hostPixels) return fail(c, RT_ERR_INVALID_ARG, "hostPixels is NULL");
    *hostPixels = nullptr;
    if (bytes) *bytes = 0;
    PRESENT_TRY(c, wait(ticket, hostPixels, bytes));
    return RT_OK;
}

}  // extern "C"
