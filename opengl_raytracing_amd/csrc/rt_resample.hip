// rt_resample.hip -- the separable polyphase resampler of the display path, both passes in one kernel.  A
// workgroup owns a tile of destination pixels: it filters the source rows the tile's vertical windows span horizontally from
// global memory into LDS, and after one barrier filters those rows vertically out of LDS into the destination.  No fp32
// intermediate goes through HBM.  The arithmetic is the header's, in its order: the accumulator starts as the first product,
// every tap of the table follows (zero padding included), multiply and add stay separate (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include "rt_resample.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ float4 mul4(float w, float4 s) { return make_float4(w * s.x, w * s.y, w * s.z, w * s.w); }
__device__ __forceinline__ float4 mad4(float4 a, float w, float4 s) {          // a + w * s, two roundings per channel
    const float4 p = mul4(w, s);
    return make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
}

// TW: 64 or 32 columns per tile (a wave is one tile row; with 32 columns its upper half idles in both passes, which only the
// largest ratios reach).  tileH, ldsRows and the tables are the host's (rt_resample_plan): the row span of every tile fits
// ldsRows by construction, and the clamps below keep a disagreement from ever leaving the LDS allocation.
template <int TW>
__global__ __launch_bounds__(kThreads) void rt_resample_kernel(const float4 *__restrict__ src, float4 *__restrict__ dst, int srcW, int srcH,
                                                               int dstW, int dstH, const int32_t *__restrict__ firstX,
                                                               const float *__restrict__ wX, int nX, const int32_t *__restrict__ firstY,
                                                               const float *__restrict__ wY, int nY, int tileH, int ldsRows,
                                                               unsigned tilesX) {
    extern __shared__ float4 hrows[];             // [ldsRows][TW]
    const unsigned tile = blockIdx.x;             // row-major; one contiguous band of tiles per XCD measured no better
    const int i0 = (int)(tile % tilesX) * TW, j0 = (int)(tile / tilesX) * tileH;
    const int j1 = min(j0 + tileH, dstH) - 1;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = i0 + lane;
    const bool column = lane < TW && i < dstW;    // ragged right tiles, and the idle half of a 32-column tile

    const int rowLo = clampi(firstY[j0], 0, srcH - 1);
    const int rowHi = clampi(firstY[j1] + nY - 1, 0, srcH - 1);
    const int rows = min(rowHi - rowLo + 1, ldsRows);

    // ---- horizontal: wave w takes rows w, w + 4, ...; a lane one column.  One row per wave at a time: four rows per wave at once,
    // with each tap's weight and column fetched once for all of them, measured twice as slow at 2:1 Lanczos
    if (column) {
        const int f = firstX[i];
        for (int r = wave; r < rows; r += kWaves) {
            const float4 *__restrict__ row = src + (size_t)(rowLo + r) * (size_t)srcW;
            float4 acc = mul4(wX[i], row[clampi(f, 0, srcW - 1)]);
#pragma unroll 4
            for (int k = 1; k < nX; k++) acc = mad4(acc, wX[(size_t)k * dstW + i], row[clampi(f + k, 0, srcW - 1)]);
            hrows[r * TW + lane] = acc;
        }
    }
    __syncthreads();

    // ---- vertical: wave w takes destination rows j0 + w, j0 + w + 4, ...; the row's window and weights are wave-uniform
    for (int j = j0 + wave; j <= j1; j += kWaves) {
        const int f = firstY[j];
        const float *__restrict__ w = wY + (size_t)j * nY;
        const auto ldsRow = [&](int y) { return clampi(clampi(y, 0, srcH - 1) - rowLo, 0, rows - 1); };
        if (column) {
            float4 acc = mul4(w[0], hrows[ldsRow(f) * TW + lane]);
#pragma unroll 4
            for (int k = 1; k < nY; k++) acc = mad4(acc, w[k], hrows[ldsRow(f + k) * TW + lane]);
            dst[(size_t)j * (size_t)dstW + i] = acc;
        }
    }
}

}  // namespace

hipError_t rt_launch_resample(const void *src, void *dst, int srcW, int srcH, int dstW, int dstH, const ResampleTables &t,
                              const RtResamplePlan &plan, hipStream_t s) {
    const unsigned long long tiles = (unsigned long long)plan.tilesX * plan.tilesY;
    if (tiles == 0 || tiles > 0x7fffffffull || plan.ldsRows < 1 || plan.ldsRows * plan.tileW > kResampleLdsTexels) return hipErrorInvalidValue;
    const size_t lds = (size_t)plan.ldsRows * plan.tileW * sizeof(float4);
    auto k = plan.tileW == 64 ? rt_resample_kernel<64> : rt_resample_kernel<32>;
    hipLaunchKernelGGL(k, dim3((unsigned)tiles), dim3(kThreads), lds, s, (const float4 *)src, (float4 *)dst, srcW, srcH, dstW, dstH,
                       t.x.dFirst.ptr, t.x.dWeights.ptr, t.x.n, t.y.dFirst.ptr, t.y.dWeights.ptr, t.y.n, plan.tileH, plan.ldsRows, plan.tilesX);
    return hipGetLastError();
}
