// rt_accum.hip -- progressive accumulation (rt_accum_add, rt_accum_view; include/rt_mi355.h has the definition): one more
// sample of every pixel into a running mean and Welford's moments of its luminance, the convergence statistics of the whole
// image into the caller's 1 KiB state, then the solve of rt_accum_solve.h as a launch of its own.
//
// Bandwidth-bound at 80 compulsory bytes per pixel (16 read from the image, 32 read from and 32 written to the accumulator);
// the seven IEEE divisions a pixel costs hide behind them.  A workgroup of 256 lanes takes chunks of 256 * RT_ACCUM_PPL
// consecutive pixels; slot k of lane t is pixel chunk * 256 * PPL + k * 256 + t, so every load and store instruction of a wave
// covers 1 KiB of consecutive bytes, and the 3 * PPL 16-byte loads of a chunk are issued before the first is used.  The grid is
// RT_ACCUM_WGS_PER_CU workgroups per CU walking the chunks with a grid stride (0: one workgroup per chunk).  Two per CU is the
// measured choice: at 1080p 512 workgroups take 40 us where one per chunk (2025 of them) takes 64; every workgroup ends with up
// to 134 global atomics on the one 1 KiB state, which is the suspect, not a measured cause.  The accumulator's loads and stores
// are non-temporal (RT_ACCUM_NT): neutral while accumulator and image fit the Infinity Cache (1080p), 15 % faster where they
// do not (4K).  DESIGN.md 20 has the figures of every form.
// The statistics are built the way rt_meter_hist_kernel's are (rt_display.hip), from the same pieces (rt_wave.h): one LDS histogram
// per wave behind rt_wave_hist_add (a converged image puts a whole wave into one or two bins), the counters in registers for the
// whole loop, reduced once per wave and once per workgroup, then one no-return integer atomic per workgroup for every non-empty
// bin and counter.  minCount accumulates as the maximum of the complement, so that the cleared state is neutral.
// No workgroup waits for another; the solve sees the complete histogram because it is the next launch on the stream.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_accum.h"
#include "rt_accum_solve.h"
#include "rt_wave.h"

#ifndef RT_ACCUM_PPL
#define RT_ACCUM_PPL 4            // pixels per lane and chunk: 3 * PPL 16-byte loads in flight
#endif
#ifndef RT_ACCUM_WGS_PER_CU
#define RT_ACCUM_WGS_PER_CU 2     // grid-stride form: workgroups per CU; 0: the tile form, one workgroup per chunk
#endif
#ifndef RT_ACCUM_NT
#define RT_ACCUM_NT 1             // 1: non-temporal loads and stores on the accumulator (the image is read with plain loads)
#endif
#ifndef RT_ACCUM_PEER
#define RT_ACCUM_PEER 2           // aggregation rounds per pixel slot before every pending lane adds 1 for itself
#endif

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr size_t AS_CLEAR_BYTES = AS_FRAMES * 4;        // everything in front of `frames`

template <bool NT>
__device__ __forceinline__ f4 accum_load(const f4 *p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}
template <bool NT>
__device__ __forceinline__ void accum_store(f4 *p, f4 v) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

}  // namespace

template <int PPL, bool NT>
__global__ __launch_bounds__(256) void rt_accum_add_kernel(const f4 *__restrict__ image, f4 *__restrict__ mean, f4 *__restrict__ moments,
                                                           unsigned nPixels, unsigned nChunks, const RtAccumRule rule,
                                                           unsigned *__restrict__ state) {
    __shared__ unsigned hist[4][kAccumBins];                // one histogram per wave
    __shared__ unsigned red[6];                             // nUnsampled, nConverged, nRejected, max(~count), max(count), max(bits(r2))
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    hist[tid >> 7][tid & 127u] = 0u;
    hist[2u + (tid >> 7)][tid & 127u] = 0u;
    if (tid < 6u) red[tid] = 0u;
    __syncthreads();
    unsigned *wh = hist[tid >> 6];
    unsigned cUnsampled = 0u, cConverged = 0u, cRejected = 0u, mnC = 0u, mxCount = 0u, mxR2 = 0u;
    // (the chunk is the workgroup's: every lane of a wave leaves the loop together, so the ballots below see all of them)
    for (unsigned chunk = blockIdx.x; chunk < nChunks; chunk += gridDim.x) {
        const unsigned base = chunk * (256u * PPL) + tid;   // below nPixels + 256 * PPL < 2^32
        f4 x[PPL], mu[PPL], mo[PPL];
#pragma unroll
        for (int k = 0; k < PPL; k++) {
            const unsigned i = base + (unsigned)k * 256u;
            const bool have = i < nPixels;
            const f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
            x[k] = have ? *(image + i) : zero;
            mu[k] = have ? accum_load<NT>(mean + i) : zero;
            mo[k] = have ? accum_load<NT>(moments + i) : zero;
        }
#pragma unroll
        for (int k = 0; k < PPL; k++) {
            const unsigned i = base + (unsigned)k * 256u;
            const bool have = i < nPixels;
            const f4 s = x[k];
            float mY = mo[k].x, M2 = mo[k].y;
            unsigned count = __float_as_uint(mo[k].z);
            const bool inRange = fabsf(s.x) <= kRtSampleLimit && fabsf(s.y) <= kRtSampleLimit && fabsf(s.z) <= kRtSampleLimit && fabsf(s.w) <= kRtSampleLimit;
            const bool accept = have && inRange && count < (1u << 24);
            if (accept) {
                count += 1u;
                const float nf = (float)count;
                f4 m = mu[k];
                m.x = m.x + (s.x - m.x) / nf;
                m.y = m.y + (s.y - m.y) / nf;
                m.z = m.z + (s.z - m.z) / nf;
                m.w = m.w + (s.w - m.w) / nf;
                const float Y = rt_luma(s.x, s.y, s.z);
                const float dY = Y - mY;
                mY = mY + dY / nf;
                M2 = M2 + dY * (Y - mY);
                const f4 o = {mY, M2, __uint_as_float(count), 0.0f};
                accum_store<NT>(mean + i, m);
                accum_store<NT>(moments + i, o);
            }
            cRejected += (have && !accept) ? 1u : 0u;
            const RtAccumJudged j = rt_accum_judge(mY, M2, count, rule);
            const bool binned = have && j.sampled;
            cUnsampled += (have && !j.sampled) ? 1u : 0u;
            cConverged += (have && j.converged) ? 1u : 0u;
            mnC = max(mnC, have ? ~count : 0u);
            mxCount = max(mxCount, have ? count : 0u);
            mxR2 = max(mxR2, binned ? __float_as_uint(j.r2) : 0u);
            rt_wave_hist_add<RT_ACCUM_PEER>(wh, j.bin, binned, lane);
        }
    }
    // once per wave: reduce the registers across the lanes, lane 0 carries the wave's figures into the workgroup's
    const auto add = [](unsigned a, unsigned b) { return a + b; };
    const auto umax = [](unsigned a, unsigned b) { return max(a, b); };
    cUnsampled = rt_wave_reduce(cUnsampled, add);
    cConverged = rt_wave_reduce(cConverged, add);
    cRejected = rt_wave_reduce(cRejected, add);
    mnC = rt_wave_reduce(mnC, umax);
    mxCount = rt_wave_reduce(mxCount, umax);
    mxR2 = rt_wave_reduce(mxR2, umax);
    if (lane == 0u) {
        if (cUnsampled) atomicAdd(&red[0], cUnsampled);
        if (cConverged) atomicAdd(&red[1], cConverged);
        if (cRejected) atomicAdd(&red[2], cRejected);
        if (mnC) atomicMax(&red[3], mnC);
        if (mxCount) atomicMax(&red[4], mxCount);
        if (mxR2) atomicMax(&red[5], mxR2);
    }
    __syncthreads();
    // flush: non-empty bins and counters only, no-return integer atomics, one per workgroup and quantity
    if (tid < (unsigned)kAccumBins) {
        const unsigned sum = (hist[0][tid] + hist[1][tid]) + (hist[2][tid] + hist[3][tid]);
        if (sum) atomicAdd(&state[tid], sum);
    } else if (tid < (unsigned)kAccumBins + 3u) {
        const unsigned v = red[tid - kAccumBins];
        if (v) atomicAdd(&state[AS_NUNSAMPLED + (tid - kAccumBins)], v);
    } else if (tid < (unsigned)kAccumBins + 6u) {
        const unsigned v = red[tid - kAccumBins];
        if (v) atomicMax(&state[AS_MINCOUNT + (tid - kAccumBins - 3u)], v);
    }
}

// One workgroup, one thread per bin: an inclusive prefix sum of the bins, every bin asks rt_accum_solve.h whether it is the
// one a percentile's rank falls into (the words were cleared to 0, the answer when nothing is binned), thread 128 writes the
// other words, the threads behind it keep the reserved words zero.
__global__ __launch_bounds__(256) void rt_accum_solve_kernel(unsigned *__restrict__ state, unsigned nPixels, int donePermille) {
    __shared__ unsigned scan[2][kAccumBins];                // ping-pong inclusive prefix sums (n < 2^31: 32 bits hold them)
    const unsigned b = threadIdx.x;
    const bool isBin = b < (unsigned)kAccumBins;
    const unsigned count = isBin ? state[b] : 0u;
    const int cur = rt_block_scan(scan, b, count);
    if (isBin) {
        const uint64_t n = scan[cur][kAccumBins - 1], c = scan[cur][b];
        if (rt_accum_bin_reaches(c, count, rt_accum_rank(n, 500))) state[AS_MEDIANBIN] = b;
        if (rt_accum_bin_reaches(c, count, rt_accum_rank(n, 950))) state[AS_P95BIN] = b;
    } else if (b == (unsigned)kAccumBins) {
        state[AS_NPIXELS] = nPixels;
        state[AS_MINCOUNT] = ~state[AS_MINCOUNT];           // max(~count) over nPixels >= 1 pixels -> min(count)
        state[AS_DONE] = rt_accum_done(state[AS_NCONVERGED], nPixels, donePermille);
        state[AS_FRAMES] = rt_accum_next_frames(state[AS_FRAMES]);
    } else if (b >= (unsigned)AS_RESERVED) {
        state[b] = 0u;
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void rt_accum_view_kernel(const f4 *__restrict__ moments, f4 *__restrict__ out, unsigned nPixels,
                                                            const RtAccumRule rule) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nPixels) return;
    const f4 mo = moments[i];
    const unsigned count = __float_as_uint(mo.z);
    float v;
    if (MODE == 1) {
        v = (float)count;
    } else {
        const RtAccumJudged j = rt_accum_judge(mo.x, mo.y, count, rule);
        if (MODE == 0) v = j.sampled ? sqrtf(j.r2) : __builtin_huge_valf();
        else v = j.converged ? 1.0f : 0.0f;
    }
    const f4 o = {v, v, v, 1.0f};
    out[i] = o;
}

hipError_t rt_launch_accum_add(const void *image, void *accum, void *state, unsigned nPixels, const RtAccumRule &rule, hipStream_t s) {
    constexpr unsigned chunkPixels = 256u * RT_ACCUM_PPL;
    const unsigned nChunks = (nPixels + chunkPixels - 1u) / chunkPixels;
    const unsigned cap = RT_ACCUM_WGS_PER_CU ? (unsigned)rt_cu_count() * RT_ACCUM_WGS_PER_CU : nChunks;
    hipError_t e = hipMemsetAsync(state, 0, AS_CLEAR_BYTES, s);
    if (e != hipSuccess) return e;
    f4 *mean = (f4 *)accum;
    hipLaunchKernelGGL((rt_accum_add_kernel<RT_ACCUM_PPL, RT_ACCUM_NT != 0>), dim3(nChunks < cap ? nChunks : cap), dim3(256), 0, s,
                       (const f4 *)image, mean, mean + nPixels, nPixels, nChunks, rule, (unsigned *)state);
    return rt_launch_accum_solve(state, nPixels, rule.donePermille, s);
}

hipError_t rt_launch_accum_solve(void *state, unsigned nPixels, int donePermille, hipStream_t s) {
    hipLaunchKernelGGL(rt_accum_solve_kernel, dim3(1), dim3(256), 0, s, (unsigned *)state, nPixels, donePermille);
    return hipGetLastError();
}

hipError_t rt_launch_accum_view(const void *accum, void *out, unsigned nPixels, const RtAccumRule &rule, int mode, hipStream_t s) {
    const f4 *moments = (const f4 *)accum + nPixels;
    const dim3 grid((nPixels + 255u) / 256u);
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, moments, (f4 *)out, nPixels, rule); };
    if (mode == 0) go(rt_accum_view_kernel<0>);
    else if (mode == 1) go(rt_accum_view_kernel<1>);
    else if (mode == 2) go(rt_accum_view_kernel<2>);
    else return hipErrorInvalidValue;                       // (callers refuse unknown modes first)
    return hipGetLastError();
}
