// rt_wire.h -- the strip transport's launch wrappers, for the entry points in rt_wire.cpp.  The three copy kernels behind them
// live in rt_kernels.hip (they share nothing with the tracer; DESIGN.md section 30 has why they stay there).  Not part of the
// public ABI.
#pragma once
#include <hip/hip_runtime.h>

// hipErrorInvalidValue when no unit of 4, 8 or 16 bytes divides the row, the rank stride and both addresses
hipError_t rt_launch_deinterleave(const void *src, void *dst, int width, int height, int bytesPerPixel,
                                  int stripRows, int stripCount, size_t rankStrideBytes, hipStream_t s);
hipError_t rt_launch_wire_pack(const void *dColor, const void *dPos, const void *dNormal, void *dWire, size_t nPixels,
                               hipStream_t s);
// rootRows: the root's rows per cycle (its strips * stripRows)
hipError_t rt_launch_wire_unpack(const void *dWire, size_t rankStrideBytes, size_t rankPixels, const void *dRootColor,
                                 const void *dRootPos, const void *dRootNormal, int rootRows, void *dColor, void *dPos,
                                 void *dNormal, int width, int height, int stripRows, int stripCount, hipStream_t s);
