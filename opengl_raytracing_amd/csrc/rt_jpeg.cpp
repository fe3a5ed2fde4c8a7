// rt_jpeg.cpp -- the baseline JPEG encoder's entry points of the C ABI (include/rt_mi355.h has the contract of each): the host-only
// functions (DCT matrix, quantisers, header, layout), the encode of a packed YUV frame, the pack-and-encode of an rgba32f surface
// and its delivery through the present ring.  The kernels are rt_jpeg.hip's.
#include <math.h>
#include <string.h>

#include "rt_args.h"
#include "rt_display.h"
#include "rt_jpeg.h"

namespace {

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

// how a validated rt_jpeg_desc divides the frame and its scratch
struct JpegPlan {
    uint64_t nMcu = 0, nSegments = 0;
    size_t offset[3] = {0, 0, 0};        // coefficient plane, segment offsets, the private region
    size_t segBytes = 0, segStuffed = 0, yuv = 0;    // within the scratch: the private region's three parts
    size_t yuvBytes = 0, scratchBytes = 0, worstBytes = 0;
};

// The description alone; *tooLarge when the worst stream would pass 2^32 - 1 bytes (then plan is not filled in)
bool plan_jpeg(const rt_jpeg_desc *d, JpegPlan *p, bool *tooLarge) {
    *tooLarge = false;
    if (!d || d->width < 1 || d->width > 65535 || d->height < 1 || d->height > 65535 || d->quality < 1 || d->quality > 100 ||
        d->restartInterval < 1 || d->restartInterval > 65535 || !rt_all_zero(d->reserved))
        return false;
    const uint64_t W = (uint64_t)d->width, H = (uint64_t)d->height, cw = (W + 1) / 2, ch = (H + 1) / 2;
    p->nMcu = ((W + 15) / 16) * ((H + 15) / 16);
    p->nSegments = (p->nMcu + (uint64_t)d->restartInterval - 1) / (uint64_t)d->restartInterval;
    const uint64_t worst = kJpegHeaderBytes + p->nMcu * kJpegMcuWorstBytes + 2 * (p->nSegments - 1) + 2;
    if (worst > 0xffffffffull) {
        *tooLarge = true;
        return false;
    }
    p->worstBytes = (size_t)worst;
    p->yuvBytes = (size_t)(W * H + 2 * cw * ch);
    p->offset[0] = 0;
    p->offset[1] = align16((size_t)p->nMcu * 6 * 64 * sizeof(int16_t));
    p->offset[2] = p->offset[1] + align16(((size_t)p->nSegments + 1) * sizeof(uint32_t));
    p->segBytes = p->offset[2];
    p->segStuffed = p->segBytes + (size_t)p->nSegments * sizeof(uint32_t);
    p->yuv = align16(p->segStuffed + (size_t)p->nSegments * sizeof(uint32_t));
    p->scratchBytes = p->yuv + align16(p->yuvBytes);
    return true;
}

int validate_jpeg(rt_context *c, const rt_jpeg_desc *d, JpegPlan *p) {
    if (!d) return fail(c, RT_ERR_INVALID_ARG, "JPEG description is NULL");
    bool tooLarge;
    if (plan_jpeg(d, p, &tooLarge)) return RT_OK;
    if (tooLarge) return fail(c, RT_ERR_TOO_LARGE, "the worst-case stream passes 2^32 - 1 bytes");
    if (d->width < 1 || d->width > 65535 || d->height < 1 || d->height > 65535) return fail(c, RT_ERR_INVALID_ARG, "width/height must be 1..65535");
    if (d->quality < 1 || d->quality > 100) return fail(c, RT_ERR_INVALID_ARG, "quality must be 1..100");
    if (d->restartInterval < 1 || d->restartInterval > 65535) return fail(c, RT_ERR_INVALID_ARG, "restartInterval must be 1..65535");
    return fail(c, RT_ERR_INVALID_ARG, "reserved words must be zero");
}

void dct_matrix(int32_t out[64]) {
    for (int u = 0; u < 8; u++)
        for (int x = 0; x < 8; x++)
            out[u * 8 + x] = (int32_t)nearbyint(16384.0 * (u ? 0.5 : 1.0 / (2.0 * sqrt(2.0))) * cos((2 * x + 1) * u * M_PI / 16.0));
}

void quant_tables(int quality, uint8_t luma[64], uint8_t chroma[64]) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; i++) {
        const int l = (kJpegQuantLuma[i] * s + 50) / 100, ch = (kJpegQuantChroma[i] * s + 50) / 100;
        luma[i] = (uint8_t)(l < 1 ? 1 : l > 255 ? 255 : l);
        chroma[i] = (uint8_t)(ch < 1 ? 1 : ch > 255 ? 255 : ch);
    }
}

// the 629 bytes in front of the entropy-coded data
void build_header(const rt_jpeg_desc *d, uint8_t *out) {
    uint8_t *p = out;
    auto put = [&](std::initializer_list<int> bytes) { for (int b : bytes) *p++ = (uint8_t)b; };
    auto be16 = [&](int v) { put({v >> 8, v & 255}); };
    uint8_t q[2][64];
    quant_tables(d->quality, q[0], q[1]);
    put({0xff, 0xd8});
    put({0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int t = 0; t < 2; t++) {
        put({0xff, 0xdb, 0, 67, t});
        for (int k = 0; k < 64; k++) *p++ = q[t][kJpegZigzag.order[k]];
    }
    put({0xff, 0xc0, 0, 17, 8});
    be16(d->height);
    be16(d->width);
    put({3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
    const RtJpegHuffSpec *specs[4] = {&kJpegDcLuma, &kJpegAcLuma, &kJpegDcChroma, &kJpegAcChroma};
    const int ids[4] = {0x00, 0x10, 0x01, 0x11};
    for (int t = 0; t < 4; t++) {
        put({0xff, 0xc4});
        be16(19 + specs[t]->n);
        *p++ = (uint8_t)ids[t];
        memcpy(p, specs[t]->bits, 16);
        memcpy(p + 16, specs[t]->vals, (size_t)specs[t]->n);
        p += 16 + specs[t]->n;
    }
    put({0xff, 0xdd, 0, 4});
    be16(d->restartInterval);
    put({0xff, 0xda, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
}

// the planes of an rt_yuv_desc as the encoder reads them: size and format only
int validate_planes(rt_context *c, const rt_yuv_desc *planes, const rt_jpeg_desc *d, RtJpegGeom *g) {
    if (!planes) return fail(c, RT_ERR_INVALID_ARG, "plane description is NULL");
    if (planes->format != RT_YUV_NV12 && planes->format != RT_YUV_I420) return fail(c, RT_ERR_INVALID_ARG, "unknown YUV format");
    if (planes->width != d->width || planes->height != d->height) return fail(c, RT_ERR_INVALID_ARG, "the planes' size differs from the JPEG description's");
    (void)rt_display_yuv_layout(planes, g->planeOffset, g->planePitch, nullptr);
    g->chromaStep = planes->format == RT_YUV_NV12 ? 2 : 1;
    return RT_OK;
}

hipError_t launch_encode(const void *dPlanes, RtJpegGeom g, const rt_jpeg_desc *d, const JpegPlan &p, void *dScratch, void *dOut, size_t capBytes,
                         void *dState, hipStream_t s) {
    g.W = d->width;
    g.H = d->height;
    g.cw = (d->width + 1) / 2;
    g.ch = (d->height + 1) / 2;
    g.mw = (unsigned)((d->width + 15) / 16);
    g.nMcu = (unsigned)p.nMcu;
    g.nSegments = (unsigned)p.nSegments;
    g.interval = (unsigned)d->restartInterval;
    RtJpegTables tab;
    dct_matrix(tab.M);
    uint8_t q[2][64];
    quant_tables(d->quality, q[0], q[1]);
    for (int t = 0; t < 2; t++)
        for (int i = 0; i < 64; i++) tab.q[t][i] = (uint32_t)q[t][i] << 21 | ((1u << 20) / q[t][i] + 1u);
    RtJpegHeaderImage hdr = {};
    uint8_t bytes[sizeof hdr.w] = {};
    build_header(d, bytes);
    memcpy(hdr.w, bytes, sizeof hdr.w);          // (little-endian host, as the device)
    uint8_t *scratch = (uint8_t *)dScratch;
    return rt_launch_jpeg_encode(dPlanes, g, tab, hdr, scratch + p.offset[0], scratch + p.offset[1], scratch + p.segBytes, scratch + p.segStuffed,
                                 dOut, capBytes, dState, s);
}

// the output side of an encode: pointers, and no two of the ranges sharing a byte (`in`: what the call reads)
int validate_ranges(rt_context *c, const char *entry, DevRange in, const char *inName, const void *dScratch, size_t scratchBytes, const void *dOut,
                    size_t capBytes, const void *dState) {
    RT_TRY(rt_check_pointers(c, {{in.p, inName}, {dScratch, "scratch"}, {dOut, "output"}, {dState, "state"}}));
    const DevRange r[4] = {in, {dScratch, scratchBytes}, {dOut, capBytes}, {dState, sizeof(rt_jpeg_state)}};
    for (int i = 0; i < 4; i++)
        for (int j = i + 1; j < 4; j++)
            if (overlaps(r[i], r[j])) return fail(c, RT_ERR_INVALID_ARG, (std::string(entry) + ": two of its device ranges overlap").c_str());
    return RT_OK;
}

int validate_pack(rt_context *c, const void *dImage, const rt_yuv_desc *yuv, const rt_tone_desc *tone, const rt_jpeg_desc *d, JpegPlan *p,
                  RtJpegGeom *g, RtYuvPack *pack) {
    RT_TRY(validate_jpeg(c, d, p));
    RT_TRY(rt_yuv_pack_validate(c, dImage, yuv, tone, pack));
    if (yuv->matrix != RT_YUV_BT601 || yuv->range != RT_YUV_FULL) return fail(c, RT_ERR_INVALID_ARG, "a JFIF file holds full-range BT.601 only");
    return validate_planes(c, yuv, d, g);
}

}  // namespace

extern "C" {

int rt_jpeg_dct_matrix(int32_t out[64]) {
    if (!out) return RT_ERR_INVALID_ARG;
    dct_matrix(out);
    return RT_OK;
}

int rt_jpeg_quant(int quality, uint8_t luma[64], uint8_t chroma[64]) {
    if (!luma || !chroma || quality < 1 || quality > 100) return RT_ERR_INVALID_ARG;
    quant_tables(quality, luma, chroma);
    return RT_OK;
}

int rt_jpeg_layout(const rt_jpeg_desc *d, size_t offset[3], size_t *scratchBytes, size_t *worstBytes) {
    JpegPlan p;
    bool tooLarge;
    if (!offset) return RT_ERR_INVALID_ARG;
    if (!plan_jpeg(d, &p, &tooLarge)) return tooLarge ? RT_ERR_TOO_LARGE : RT_ERR_INVALID_ARG;
    memcpy(offset, p.offset, sizeof p.offset);
    if (scratchBytes) *scratchBytes = p.scratchBytes;
    if (worstBytes) *worstBytes = p.worstBytes;
    return RT_OK;
}

int rt_jpeg_header(const rt_jpeg_desc *d, uint8_t *buf, size_t cap, size_t *n) {
    JpegPlan p;
    bool tooLarge;
    if (!buf || !n) return RT_ERR_INVALID_ARG;
    if (!plan_jpeg(d, &p, &tooLarge)) return tooLarge ? RT_ERR_TOO_LARGE : RT_ERR_INVALID_ARG;
    if (cap < kJpegHeaderBytes) return RT_ERR_INVALID_ARG;
    build_header(d, buf);
    *n = kJpegHeaderBytes;
    return RT_OK;
}

int rt_jpeg_encode(rt_context *c, const void *dPlanes, const rt_yuv_desc *planes, const rt_jpeg_desc *d, void *dScratch, void *dOut,
                   size_t capBytes, void *dState, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    JpegPlan p;
    RtJpegGeom g = {};
    RT_TRY(validate_jpeg(c, d, &p));
    RT_TRY(validate_planes(c, planes, d, &g));
    RT_TRY(validate_ranges(c, "rt_jpeg_encode", {dPlanes, p.yuvBytes}, "planes", dScratch, p.scratchBytes, dOut, capBytes, dState));
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_encode(dPlanes, g, d, p, dScratch, dOut, capBytes, dState, stream_or_own(c, hipStream)));
    return RT_OK;
}

int rt_display_pack_jpeg(rt_context *c, const void *dImage, const rt_yuv_desc *yuv, const rt_tone_desc *tone, const rt_jpeg_desc *d,
                         void *dScratch, void *dOut, size_t capBytes, void *dState, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    JpegPlan p;
    RtJpegGeom g = {};
    RtYuvPack pack;
    RT_TRY(validate_pack(c, dImage, yuv, tone, d, &p, &g, &pack));
    RT_TRY(validate_ranges(c, "rt_display_pack_jpeg", {dImage, (size_t)d->width * d->height * 16}, "image", dScratch, p.scratchBytes, dOut, capBytes,
                           dState));
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = stream_or_own(c, hipStream);
    uint8_t *dPlanes = (uint8_t *)dScratch + p.yuv;
    HIP_TRY(c, rt_yuv_pack_launch(dImage, dPlanes, yuv, pack, s));
    HIP_TRY(c, launch_encode(dPlanes, g, d, p, dScratch, dOut, capBytes, dState, s));
    return RT_OK;
}

int rt_present_submit_jpeg(rt_context *c, const void *dImage, const rt_yuv_desc *yuv, const rt_tone_desc *tone, const rt_jpeg_desc *d,
                           size_t capBytes, void *hipStream, uint64_t *ticket) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!ticket) return fail(c, RT_ERR_INVALID_ARG, "ticket is NULL");
    JpegPlan p;
    RtJpegGeom g = {};
    RtYuvPack pack;
    RT_TRY(validate_pack(c, dImage, yuv, tone, d, &p, &g, &pack));
    if (capBytes == 0) capBytes = p.worstBytes;
    if (capBytes > 0xffffffffull) return fail(c, RT_ERR_TOO_LARGE, "capBytes passes 2^32 - 1");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = stream_or_own(c, hipStream);
    // the context's scratch, one for every stream: grown behind its last user, then used one submit after another
    HIP_TRY(c, c->jpegUse.create());
    if (!c->dJpegScratch.holds(p.scratchBytes)) {
        HIP_TRY(c, c->jpegUse.drain());
        HIP_TRY(c, c->dJpegScratch.grow(p.scratchBytes));
    }
    HIP_TRY(c, c->jpegUse.acquire(s));
    uint8_t *scratch = c->dJpegScratch.ptr;
    const int rc = c->present.enqueue(sizeof(rt_jpeg_state) + capBytes, s, ticket, [&](void *stage, hipStream_t st) {
        hipError_t e = rt_yuv_pack_launch(dImage, scratch + p.yuv, yuv, pack, st);
        if (e != hipSuccess) return e;
        return launch_encode(scratch + p.yuv, g, d, p, scratch, (uint8_t *)stage + sizeof(rt_jpeg_state), capBytes, stage, st);
    });
    const hipError_t released = c->jpegUse.release(s);                 // whatever became of the submit: its launches may be in the scratch
    if (rc) return fail(c, rc, c->present.failed, c->present.failedHip);
    HIP_TRY(c, released);
    return RT_OK;
}

}  // extern "C"
