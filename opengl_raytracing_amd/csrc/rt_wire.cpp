// rt_wire.cpp -- the strip transport's entry points of the C ABI (include/rt_mi355.h has the contract of each): which rows a
// device of an interleaved strip plan owns, the reassembly of gathered strips, and the 30-byte-a-pixel wire format of the gather.
// The kernels stand in rt_kernels.hip (rt_wire.h).  rt_mgpu.cpp and the multi-process driver call these through the public ABI.
#include "rt_context.h"
#include "rt_wire.h"

extern "C" {

int rt_strip_local_rows(int height, int stripRows, int stripCount, int stripIndex) {
    if (height < 0 || stripRows <= 0 || stripCount <= 0 || stripIndex < 0 || stripIndex >= stripCount) return RT_ERR_INVALID_ARG;
    int nStrips = (height + stripRows - 1) / stripRows;
    int rows = 0;
    for (int s = stripIndex; s < nStrips; s += stripCount) {
        int r0 = s * stripRows, r1 = r0 + stripRows;
        if (r1 > height) r1 = height;
        rows += r1 - r0;
    }
    return rows;
}

int rt_deinterleave(rt_context *c, const void *src, void *dst, int width, int height, int bytesPerPixel,
                    int stripRows, int stripCount, size_t rankStrideBytes, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!src || !dst || width <= 0 || height <= 0 || bytesPerPixel <= 0 || stripRows <= 0 || stripCount <= 0)
        return fail(c, RT_ERR_INVALID_ARG, "bad deinterleave arguments");
    if (((size_t)width * bytesPerPixel) % 4 != 0 || rankStrideBytes % 4 != 0)
        return fail(c, RT_ERR_INVALID_ARG, "row bytes and rank stride must be multiples of 4");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = stream_or_own(c, hipStream);
    HIP_TRY(c, rt_launch_deinterleave(src, dst, width, height, bytesPerPixel, stripRows, stripCount, rankStrideBytes, s));
    return RT_OK;
}

size_t rt_wire_bytes(size_t nPixels) { return (nPixels * 30 + 15) / 16 * 16; }

int rt_wire_pack(rt_context *c, const void *dColor, const void *dPosition, const void *dNormal, void *dWire, size_t nPixels,
                 void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!dColor || !dPosition || !dNormal || !dWire) return fail(c, RT_ERR_INVALID_ARG, "bad wire_pack arguments");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = stream_or_own(c, hipStream);
    HIP_TRY(c, rt_launch_wire_pack(dColor, dPosition, dNormal, dWire, nPixels, s));
    return RT_OK;
}

int rt_wire_unpack(rt_context *c, const void *dWire, size_t rankStrideBytes, size_t rankPixels, const void *dRootColor,
                   const void *dRootPosition, const void *dRootNormal, int rootStrips, void *dColor, void *dPosition,
                   void *dNormal, int width, int height, int stripRows, int stripCount, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!dWire || !dColor || !dPosition || !dNormal || width <= 0 || height <= 0 || stripRows <= 0 || stripCount <= 0 ||
        rootStrips <= 0)
        return fail(c, RT_ERR_INVALID_ARG, "bad wire_unpack arguments");
    const bool rootLocal = dRootColor || dRootPosition || dRootNormal;
    if (rootLocal && !(dRootColor && dRootPosition && dRootNormal))
        return fail(c, RT_ERR_INVALID_ARG, "the root's three local surfaces must be given together");
    if (!rootLocal && rootStrips != 1) return fail(c, RT_ERR_INVALID_ARG, "a larger root share needs the root's local surfaces");
    // every rank buffer must hold the rank's whole strips, and the f32 / f16 planes must stay aligned
    const int cycleRows = (rootStrips + stripCount - 1) * stripRows;
    const int nCycles = (height + cycleRows - 1) / cycleRows;
    const size_t needPixels = (size_t)nCycles * stripRows * width;
    if (rankPixels < needPixels || rankStrideBytes % 4 != 0 || rankStrideBytes < rankPixels * 30)
        return fail(c, RT_ERR_INVALID_ARG, "rank buffers too small or misaligned for this strip plan");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = stream_or_own(c, hipStream);
    HIP_TRY(c, rt_launch_wire_unpack(dWire, rankStrideBytes, rankPixels, dRootColor, dRootPosition, dRootNormal,
                                     rootStrips * stripRows, dColor, dPosition, dNormal, width, height, stripRows, stripCount, s));
    return RT_OK;
}

}  // extern "C"
