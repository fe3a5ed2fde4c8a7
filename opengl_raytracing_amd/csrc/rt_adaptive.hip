// rt_adaptive.hip -- adaptive sampling (rt_accum_select, rt_accum_add_at; include/rt_mi355.h has the definition): the accumulator's
// verdict as an ordered list of the pixels that still need samples, and one more sample folded into listed pixels only.
//
// SELECT is three launches, ordered by the stream alone -- no workgroup waits for another:
//   judge  a wave takes a tile of 8 x 8 pixels (lane l is pixel (l & 7, l >> 3) of it: raster order inside the tile), reads the 16
//          bytes of moments of each, asks rt_accum_judge (rt_accum.h, the rule rt_accum_add uses) and stores the ballot of the
//          selected lanes, 8 bytes per tile.  A workgroup of four waves takes chunks of 32 consecutive tiles; the grid is at most
//          kSelectMaxWgs workgroups and workgroup g owns the chunks [g * per, (g + 1) * per): a contiguous run, so that its total is
//          one number.  It leaves that total and the total of capped pixels in the scratch header (plain stores, every launched
//          workgroup its own word: dirty scratch is fine and nothing has to be cleared).
//   scan   ONE workgroup: an exclusive prefix sum (rt_block_scan, integers) of the at most 512 totals, two per thread, in place;
//          then the select state, written whole.
//   emit   the judge's grid again.  A workgroup starts at its offset and walks its chunks in order; every wave reads the 32 ballots
//          of the chunk, scans their popcounts across its lanes, and for each of its 8 tiles a lane with its bit set stores
//          (x, y) at offset + rank -- after checking that index against the capacity.  Consecutive entries are consecutive
//          addresses.  The moments are not read again.
//   Scan and emit know nothing of the judge but its ballots and totals: rt_launch_select_from_ballots runs them for rt_upsample.hip too.
// ADD_AT is a scatter of one lane per list entry (the per-pixel arithmetic of rt_accum_add_kernel, to the letter), then the
// statistics over every pixel -- rt_accum_add_kernel's second half on its own: per-wave LDS histograms behind rt_wave_hist_add,
// counters in registers, one no-return integer atomic per workgroup and non-empty quantity, grid-stride -- then rt_accum.hip's solve.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_adaptive.h"
#include "rt_wave.h"

#ifndef RT_ADAPT_STATS_PPL
#define RT_ADAPT_STATS_PPL 4      // statistics: pixels per lane and chunk (16-byte loads in flight)
#endif
#ifndef RT_ADAPT_WGS_PER_CU
#define RT_ADAPT_WGS_PER_CU 2     // statistics: workgroups per CU (rt_accum_add's measured choice)
#endif
#ifndef RT_ADAPT_PEER
#define RT_ADAPT_PEER 2           // aggregation rounds of rt_wave_hist_add
#endif

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr unsigned kTile = kSelectTile, kTilesPerChunk = kSelectTilesPerChunk, kTilesPerWave = kSelectTilesPerChunk / 4;
constexpr size_t AS_CLEAR_BYTES = AS_FRAMES * 4;        // everything in front of `frames`
static_assert(kTile * kTile == 64 && kSelectMaxWgs == 512, "a tile is a wave; the scan takes two totals per thread");

}  // namespace

// ---- rt_accum_select ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rt_select_judge_kernel(const f4 *__restrict__ moments, unsigned width, unsigned height, unsigned tilesX,
                                                              unsigned nTiles, unsigned nChunks, unsigned chunksPerWg, const RtAccumRule rule,
                                                              unsigned maxSamples, u64 *__restrict__ ballots, unsigned *__restrict__ totals) {
    __shared__ unsigned red[2];                             // selected, capped
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid < 2u) red[tid] = 0u;
    __syncthreads();
    const unsigned c0 = blockIdx.x * chunksPerWg;
    const unsigned c1 = min(c0 + chunksPerWg, nChunks);
    unsigned nSel = 0u, nCap = 0u;                          // wave-uniform
    for (unsigned chunk = c0; chunk < c1; chunk++) {
        const unsigned tile0 = chunk * kTilesPerChunk + wave * kTilesPerWave;       // <= nTiles + 31 < 2^32
        f4 mo[kTilesPerWave];
        bool have[kTilesPerWave];
#pragma unroll
        for (unsigned k = 0; k < kTilesPerWave; k++) {
            const unsigned tile = tile0 + k;
            const unsigned ty = tile / tilesX, tx = tile - ty * tilesX;
            const unsigned x = tx * kTile + (lane & 7u), y = ty * kTile + (lane >> 3);
            have[k] = tile < nTiles && x < width && y < height;
            const f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
            mo[k] = have[k] ? moments[y * width + x] : zero;                        // (the index is formed for pixels of the image only)
        }
#pragma unroll
        for (unsigned k = 0; k < kTilesPerWave; k++) {
            const unsigned count = __float_as_uint(mo[k].z);
            const RtAccumJudged j = rt_accum_judge(mo[k].x, mo[k].y, count, rule);
            const bool open = have[k] && !j.converged;
            const bool sel = open && count < maxSamples;
            const u64 bal = __builtin_amdgcn_ballot_w64(sel);
            const u64 cap = __builtin_amdgcn_ballot_w64(open && !sel);
            if (lane == 0u && tile0 + k < nTiles) ballots[tile0 + k] = bal;
            nSel += (unsigned)__builtin_popcountll(bal);
            nCap += (unsigned)__builtin_popcountll(cap);
        }
    }
    if (lane == 0u) {
        if (nSel) atomicAdd(&red[0], nSel);
        if (nCap) atomicAdd(&red[1], nCap);
    }
    __syncthreads();
    if (tid < 2u) totals[tid * kSelectMaxWgs + blockIdx.x] = red[tid];
}

// One workgroup: totals[0 .. nWgs) -> their exclusive prefix sums in place, then the 16 words of the select state.
__global__ __launch_bounds__(256) void rt_select_scan_kernel(unsigned *__restrict__ totals, unsigned nWgs, unsigned nPixels, unsigned capacity,
                                                             unsigned *__restrict__ selState) {
    __shared__ unsigned scanSel[2][256], scanCap[2][256];   // (sums are at most nPixels < 2^31)
    const unsigned b = threadIdx.x, i0 = 2u * b, i1 = 2u * b + 1u;
    const unsigned s0 = i0 < nWgs ? totals[i0] : 0u, s1 = i1 < nWgs ? totals[i1] : 0u;
    const unsigned k0 = i0 < nWgs ? totals[kSelectMaxWgs + i0] : 0u, k1 = i1 < nWgs ? totals[kSelectMaxWgs + i1] : 0u;
    const int curSel = rt_block_scan(scanSel, b, s0 + s1);
    const int curCap = rt_block_scan(scanCap, b, k0 + k1);
    const unsigned excl = scanSel[curSel][b] - (s0 + s1);
    if (i0 < nWgs) totals[i0] = excl;
    if (i1 < nWgs) totals[i1] = excl + s0;
    if (b < 16u) {
        const unsigned nSelected = scanSel[curSel][255], nCapped = scanCap[curCap][255];
        unsigned v = 0u;                                    // the reserved words
        if (b == 0u) v = nPixels;
        else if (b == 1u) v = nSelected;
        else if (b == 2u) v = min(nSelected, capacity);
        else if (b == 3u) v = capacity;
        else if (b == 4u) v = nSelected > capacity ? 1u : 0u;
        else if (b == 5u) v = nCapped;
        selState[b] = v;
    }
}

__global__ __launch_bounds__(256) void rt_select_emit_kernel(const u64 *__restrict__ ballots, const unsigned *__restrict__ offsets, unsigned tilesX,
                                                             unsigned nTiles, unsigned nChunks, unsigned chunksPerWg, uint2 *__restrict__ pixels,
                                                             unsigned capacity) {
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const unsigned c0 = blockIdx.x * chunksPerWg;
    const unsigned c1 = min(c0 + chunksPerWg, nChunks);
    unsigned base = offsets[blockIdx.x];                    // workgroup-uniform
    for (unsigned chunk = c0; chunk < c1 && base < capacity; chunk++) {
        // every wave scans the chunk's 32 popcounts for itself: lanes 0..31 hold a tile each, no LDS and no barrier
        const unsigned t = chunk * kTilesPerChunk + (lane & 31u);
        const u64 mine = (lane < kTilesPerChunk && t < nTiles) ? ballots[t] : 0ull;
        const unsigned cnt = (unsigned)__builtin_popcountll(mine);
        unsigned incl = cnt;
#pragma unroll
        for (unsigned d = 1u; d < kTilesPerChunk; d <<= 1) {
            const unsigned up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        const unsigned chunkTotal = __shfl(incl, (int)kTilesPerChunk - 1);
        const unsigned exclMine = incl - cnt;
#pragma unroll
        for (unsigned k = 0; k < kTilesPerWave; k++) {
            const int slot = (int)(wave * kTilesPerWave + k);
            const u64 bal = __shfl(mine, slot);
            const unsigned off = __shfl(exclMine, slot);
            const unsigned tile = chunk * kTilesPerChunk + (unsigned)slot;
            const unsigned ty = tile / tilesX, tx = tile - ty * tilesX;
            const unsigned rank = (unsigned)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
            const unsigned index = base + off + rank;       // <= nSelected < 2^31
            if (((bal >> lane) & 1ull) && index < capacity) pixels[index] = make_uint2(tx * kTile + (lane & 7u), ty * kTile + (lane >> 3));
        }
        base += chunkTotal;
    }
}

// ---- rt_accum_add_at -----------------------------------------------------------------------------------------------------------
// One lane per list entry.  The arithmetic of an accepted sample is rt_accum_add_kernel's (rt_accum.hip), in its order.
__global__ __launch_bounds__(256) void rt_accum_scatter_kernel(const f4 *__restrict__ samples, const uint2 *__restrict__ pixels, size_t n,
                                                               f4 *__restrict__ mean, f4 *__restrict__ moments, unsigned width, unsigned height,
                                                               unsigned *__restrict__ state) {
    __shared__ unsigned red;
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    if (tid == 0u) red = 0u;
    __syncthreads();
    const size_t k = (size_t)blockIdx.x * 256u + tid;
    const bool have = k < n;
    const uint2 px = have ? pixels[k] : make_uint2(0u, 0u);
    const bool inside = have && px.x < width && px.y < height;
    bool accept = false;
    if (inside) {
        const unsigned i = px.y * width + px.x;             // < width * height
        const f4 s = samples[k];
        const f4 mo = moments[i];
        float mY = mo.x, M2 = mo.y;
        unsigned count = __float_as_uint(mo.z);
        const bool inRange = fabsf(s.x) <= kRtSampleLimit && fabsf(s.y) <= kRtSampleLimit && fabsf(s.z) <= kRtSampleLimit && fabsf(s.w) <= kRtSampleLimit;
        accept = inRange && count < (1u << 24);
        if (accept) {
            count += 1u;
            const float nf = (float)count;
            f4 m = mean[i];
            m.x = m.x + (s.x - m.x) / nf;
            m.y = m.y + (s.y - m.y) / nf;
            m.z = m.z + (s.z - m.z) / nf;
            m.w = m.w + (s.w - m.w) / nf;
            const float Y = rt_luma(s.x, s.y, s.z);
            const float dY = Y - mY;
            mY = mY + dY / nf;
            M2 = M2 + dY * (Y - mY);
            const f4 o = {mY, M2, __uint_as_float(count), 0.0f};
            mean[i] = m;
            moments[i] = o;
        }
    }
    const unsigned rejected = (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(have && !accept));
    if (lane == 0u && rejected) atomicAdd(&red, rejected);
    __syncthreads();
    if (tid == 0u && red) atomicAdd(&state[AS_NREJECTED], red);
}

// The statistics of rt_accum_add over the accumulator as it stands: everything of the state but nRejected and the solve's words.
template <int PPL>
__global__ __launch_bounds__(256) void rt_accum_stats_kernel(const f4 *__restrict__ moments, unsigned nPixels, unsigned nChunks, const RtAccumRule rule,
                                                             unsigned *__restrict__ state) {
    __shared__ unsigned hist[4][kAccumBins];                // one histogram per wave
    __shared__ unsigned red[5];                             // nUnsampled, nConverged, max(~count), max(count), max(bits(r2))
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    hist[tid >> 7][tid & 127u] = 0u;
    hist[2u + (tid >> 7)][tid & 127u] = 0u;
    if (tid < 5u) red[tid] = 0u;
    __syncthreads();
    unsigned *wh = hist[tid >> 6];
    unsigned cUnsampled = 0u, cConverged = 0u, mnC = 0u, mxCount = 0u, mxR2 = 0u;
    // (the chunk is the workgroup's: every lane of a wave leaves the loop together, so the ballots below see all of them)
    for (unsigned chunk = blockIdx.x; chunk < nChunks; chunk += gridDim.x) {
        const unsigned base = chunk * (256u * PPL) + tid;   // below nPixels + 256 * PPL < 2^32
        f4 mo[PPL];
#pragma unroll
        for (int k = 0; k < PPL; k++) {
            const unsigned i = base + (unsigned)k * 256u;
            const f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
            mo[k] = i < nPixels ? moments[i] : zero;
        }
#pragma unroll
        for (int k = 0; k < PPL; k++) {
            const bool have = base + (unsigned)k * 256u < nPixels;
            const unsigned count = __float_as_uint(mo[k].z);
            const RtAccumJudged j = rt_accum_judge(mo[k].x, mo[k].y, count, rule);
            const bool binned = have && j.sampled;
            cUnsampled += (have && !j.sampled) ? 1u : 0u;
            cConverged += (have && j.converged) ? 1u : 0u;
            mnC = max(mnC, have ? ~count : 0u);
            mxCount = max(mxCount, have ? count : 0u);
            mxR2 = max(mxR2, binned ? __float_as_uint(j.r2) : 0u);
            rt_wave_hist_add<RT_ADAPT_PEER>(wh, j.bin, binned, lane);
        }
    }
    const auto add = [](unsigned a, unsigned b) { return a + b; };
    const auto umax = [](unsigned a, unsigned b) { return max(a, b); };
    cUnsampled = rt_wave_reduce(cUnsampled, add);
    cConverged = rt_wave_reduce(cConverged, add);
    mnC = rt_wave_reduce(mnC, umax);
    mxCount = rt_wave_reduce(mxCount, umax);
    mxR2 = rt_wave_reduce(mxR2, umax);
    if (lane == 0u) {
        if (cUnsampled) atomicAdd(&red[0], cUnsampled);
        if (cConverged) atomicAdd(&red[1], cConverged);
        if (mnC) atomicMax(&red[2], mnC);
        if (mxCount) atomicMax(&red[3], mxCount);
        if (mxR2) atomicMax(&red[4], mxR2);
    }
    __syncthreads();
    // flush: non-empty bins and counters only, no-return integer atomics, one per workgroup and quantity
    if (tid < (unsigned)kAccumBins) {
        const unsigned sum = (hist[0][tid] + hist[1][tid]) + (hist[2][tid] + hist[3][tid]);
        if (sum) atomicAdd(&state[tid], sum);
    } else if (tid < (unsigned)kAccumBins + 2u) {
        const unsigned v = red[tid - kAccumBins];
        if (v) atomicAdd(&state[AS_NUNSAMPLED + (tid - kAccumBins)], v);
    } else if (tid < (unsigned)kAccumBins + 5u) {
        const unsigned v = red[tid - kAccumBins];
        if (v) atomicMax(&state[AS_MINCOUNT + (tid - kAccumBins - 2u)], v);
    }
}

// ---- launch wrappers -------------------------------------------------------------------------------------------------------------
hipError_t rt_launch_accum_select(const void *accum, int width, int height, const RtAccumRule &rule, unsigned maxSamples, void *pixels,
                                  unsigned capacity, void *scratch, void *selState, hipStream_t s) {
    const unsigned w = (unsigned)width, h = (unsigned)height, nPixels = w * h;
    const RtSelectGrid g(width, height);
    unsigned *totals = (unsigned *)scratch;
    u64 *ballots = (u64 *)((char *)scratch + kSelectScratchHeader);
    const f4 *moments = (const f4 *)accum + nPixels;
    hipLaunchKernelGGL(rt_select_judge_kernel, dim3(g.nWgs), dim3(256), 0, s, moments, w, h, g.tilesX, g.nTiles, g.nChunks, g.chunksPerWg, rule,
                       maxSamples, ballots, totals);
    return rt_launch_select_from_ballots(scratch, width, height, pixels, capacity, selState, s);
}

hipError_t rt_launch_select_from_ballots(void *scratch, int width, int height, void *pixels, unsigned capacity, void *selState, hipStream_t s) {
    const unsigned nPixels = (unsigned)width * (unsigned)height;
    const RtSelectGrid g(width, height);
    unsigned *totals = (unsigned *)scratch;
    const u64 *ballots = (const u64 *)((char *)scratch + kSelectScratchHeader);
    hipLaunchKernelGGL(rt_select_scan_kernel, dim3(1), dim3(256), 0, s, totals, g.nWgs, nPixels, capacity, (unsigned *)selState);
    if (capacity)
        hipLaunchKernelGGL(rt_select_emit_kernel, dim3(g.nWgs), dim3(256), 0, s, ballots, (const unsigned *)totals, g.tilesX, g.nTiles, g.nChunks,
                           g.chunksPerWg, (uint2 *)pixels, capacity);
    return hipGetLastError();
}

hipError_t rt_launch_accum_add_at(const void *samples, const void *pixels, size_t n, void *accum, void *state, int width, int height,
                                  const RtAccumRule &rule, hipStream_t s) {
    const unsigned w = (unsigned)width, h = (unsigned)height, nPixels = w * h;
    constexpr unsigned chunkPixels = 256u * RT_ADAPT_STATS_PPL;
    const unsigned nChunks = (nPixels + chunkPixels - 1u) / chunkPixels;
    const unsigned cap = (unsigned)rt_cu_count() * RT_ADAPT_WGS_PER_CU;
    hipError_t e = hipMemsetAsync(state, 0, AS_CLEAR_BYTES, s);
    if (e != hipSuccess) return e;
    f4 *mean = (f4 *)accum;
    if (n)
        hipLaunchKernelGGL(rt_accum_scatter_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, s, (const f4 *)samples, (const uint2 *)pixels, n,
                           mean, mean + nPixels, w, h, (unsigned *)state);
    hipLaunchKernelGGL((rt_accum_stats_kernel<RT_ADAPT_STATS_PPL>), dim3(nChunks < cap ? nChunks : cap), dim3(256), 0, s, (const f4 *)(mean + nPixels),
                       nPixels, nChunks, rule, (unsigned *)state);
    return rt_launch_accum_solve(state, nPixels, rule.donePermille, s);
}
