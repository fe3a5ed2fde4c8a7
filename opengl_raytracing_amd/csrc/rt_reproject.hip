// rt_reproject.hip -- reprojection of the accumulator across a camera move (rt_accum_reproject; include/rt_mi355.h has the arithmetic,
// in order): every current pixel projects its first hit into both views, gathers the 2 x 2 footprint of the previous view's hits and
// accumulator around the motion-compensated position, keeps the taps that lie on its own surface and writes what they agree on.
//
// Bandwidth-bound: 96 compulsory bytes read and 32 written per pixel (the current hit; a previous hit and both accumulator planes,
// which the four taps of neighbouring pixels share; the output), against two projections with four IEEE divisions, five
// normalisations and four tap tests.  One pixel per lane, a workgroup of 256 lanes per tile; RT_REPROJECT_WX is the width of the
// block of pixels a wave covers (64 x 1, 32 x 2 or 8 x 8), and a tile is 64 x 4 pixels for 64, 32 x 8 otherwise.  Every load is 16
// bytes: the 16 loads of the footprint are requested as one batch before the first is used, a tap outside the image reading the
// nearest texel inside instead of branching around its loads.  RT_REPROJECT_XCD gives each XCD one contiguous band of tiles
// (rt_wave.h), so that the rows neighbouring tiles share are served by one L2; RT_REPROJECT_NT stores the output non-temporally, as
// the accumulator's own kernel does: nothing reads it before the next launch.  The three lane maps, the two tile orders and the
// two kinds of store read within 2 % of each other at 1080p and 4 % at 4K.  No LDS staging: the footprint moves with the motion vector, and the lines
// it touches are already shared by neighbouring lanes of a wave through the vector L1.  DESIGN.md 23 has the figures of every form.
// One workgroup per tile ends every workgroup with up to seven atomics on the one 64-byte report, about 8 ns each whatever XCD they
// come from: 466 us at 1080p.  So RT_REPROJECT_WGS_PER_CU workgroups per CU walk the tiles with a grid stride, as rt_accum_add's
// do: two per CU take 96 us at 1080p and 326 at 4K, four 104 and 270, eight 145 and 297.  Two is kept, for 1080p.
// The report is built the way rt_accum_add's is (rt_wave.h): counters in registers for the whole loop, reduced once per wave, once
// per workgroup in LDS, then one no-return integer atomic per workgroup and non-zero quantity.  The clear that precedes the launch
// leaves minCount at 2^32 - 1, so that the minimum needs no pass behind the kernel.  No workgroup waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_reproject.h"
#include "rt_wave.h"

#ifndef RT_REPROJECT_WX
#define RT_REPROJECT_WX 32          // a wave covers WX x 64/WX pixels: 64, 32 or 8
#endif
#ifndef RT_REPROJECT_XCD
#define RT_REPROJECT_XCD 1          // 1: XCD-aware tile order, tile = (id & 7) * (grid / 8) + id / 8; 0: tile = id
#endif
#ifndef RT_REPROJECT_WGS_PER_CU
#define RT_REPROJECT_WGS_PER_CU 2   // grid-stride form: workgroups per CU (its 101 VGPRs let 4 be resident); 0: one workgroup per tile
#endif
#ifndef RT_REPROJECT_NT
#define RT_REPROJECT_NT 1           // 1: non-temporal stores of the output accumulator
#endif

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int RP_TILE_W = RT_REPROJECT_WX >= 32 ? RT_REPROJECT_WX : 32;
constexpr int RP_WAVES_X = RP_TILE_W / RT_REPROJECT_WX, RP_WAVE_H = 64 / RT_REPROJECT_WX;
constexpr int RP_TILE_H = (4 / RP_WAVES_X) * RP_WAVE_H;
static_assert(RT_REPROJECT_WX == 64 || RT_REPROJECT_WX == 32 || RT_REPROJECT_WX == 8, "a wave covers 64 x 1, 32 x 2 or 8 x 8 pixels");
static_assert(RP_TILE_W * RP_TILE_H == 256, "one pixel per lane");

enum { RP_REUSED = 0, RP_REJECTED = 1, RP_OFFSCREEN = 2, RP_MISS = 3, RP_NONE = 4 };

__device__ __forceinline__ void rp_store(f4 *p, f4 v) {
    if (RT_REPROJECT_NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// rt_denoise_guide's rule: s > 0 ? n / sqrtf(s) : 0
__device__ __forceinline__ void rp_normalise(float x, float y, float z, float &ox, float &oy, float &oz) {
    const float s = (x * x + y * y) + z * z;
    ox = oy = oz = 0.0f;
    if (s > 0.0f) {
        const float r = sqrtf(s);
        ox = x / r;
        oy = y / r;
        oz = z / r;
    }
}

}  // namespace

__global__ __launch_bounds__(256) void rt_reproject_kernel(const f4 *__restrict__ meanPrev, const f4 *__restrict__ momPrev,
                                                           const f4 *__restrict__ hitsPrev, const f4 *__restrict__ hitsCur,
                                                           f4 *__restrict__ meanCur, f4 *__restrict__ momCur, const RtReprojectRule r, int tilesX,
                                                           int nTiles, int nSlots, unsigned *__restrict__ report) {
    __shared__ unsigned red[6];                             // the four categories, max(~n'), max(n')
    __shared__ unsigned long long redSum;                   // sum(n')
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid < 6u) red[tid] = 0u;
    if (tid == 6u) redSum = 0ull;
    __syncthreads();
    const int W = r.width, H = r.height;
    unsigned cReused = 0u, cRejected = 0u, cOffscreen = 0u, cMiss = 0u, mnC = 0u, mxC = 0u;
    unsigned long long sumC = 0ull;
    // the workgroup walks the slots v = id, id + grid, ...; with the XCD order slot v is tile (v & 7) * (slots / 8) + v / 8, and the
    // grid is a multiple of 8, so a workgroup stays inside its XCD's band.  Every lane of the workgroup leaves the loop together
    for (int v = (int)blockIdx.x; v < nSlots; v += (int)gridDim.x) {
        const int tile = RT_REPROJECT_XCD ? (v & 7) * (nSlots >> 3) + (v >> 3) : v;
        const int x = (tile % tilesX) * RP_TILE_W + (int)(wave % RP_WAVES_X) * RT_REPROJECT_WX + (int)(lane % RT_REPROJECT_WX);
        const int y = (tile / tilesX) * RP_TILE_H + (int)(wave / RP_WAVES_X) * RP_WAVE_H + (int)(lane / RT_REPROJECT_WX);
        const bool live = tile < nTiles && x < W && y < H;
        int cat = RP_NONE;
        unsigned nOut = 0u;
        if (live) {
            const size_t i = (size_t)y * W + x;
            const f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
            f4 oMean = zero, oMom = zero;
            const f4 hp = hitsCur[2 * i], hn = hitsCur[2 * i + 1];          // {P, t}, {n, object}
            const int objP = __float_as_int(hn.w);
            cat = RP_MISS;
            if (objP >= 0) {
                cat = RP_OFFSCREEN;
                float pfx, pfy, cfx, cfy;
                const bool vPrev = rt_reproject_proj(r.prev, r.hx, r.hy, hp.x, hp.y, hp.z, &pfx, &pfy);
                const bool vCur = rt_reproject_proj(r.cur, r.hx, r.hy, hp.x, hp.y, hp.z, &cfx, &cfy);
                const float gx = (float)x + (pfx - cfx), gy = (float)y + (pfy - cfy);
                // in float, before any conversion: a NaN or an infinity fails these comparisons, so g is finite behind them
                if (vPrev && vCur && gx > -1.0f && gx < (float)W && gy > -1.0f && gy < (float)H) {
                    cat = RP_REJECTED;
                    const float flx = floorf(gx), fly = floorf(gy);
                    const int x0 = (int)flx, y0 = (int)fly;                 // -1 .. W-1, -1 .. H-1
                    const float ax = gx - flx, ay = gy - fly;
                    float npx, npy, npz;
                    rp_normalise(hn.x, hn.y, hn.z, npx, npy, npz);
                    // the footprint: one batch of loads
                    float w[4];
                    bool in[4];
                    f4 qp[4], qn[4], qm[4], qo[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int ti = k & 1, tj = k >> 1;
                        const int qx = x0 + ti, qy = y0 + tj;
                        w[k] = (ti ? ax : 1.0f - ax) * (tj ? ay : 1.0f - ay);
                        in[k] = !(w[k] == 0.0f) && qx >= 0 && qx < W && qy >= 0 && qy < H;
                        // (every lane loads, from the nearest texel inside: a load under a condition of its own makes the compiler wait
                        // for it before the next tap's, and the clamped texel's lines are its neighbours' anyway)
                        const size_t qi = (size_t)min(max(qy, 0), H - 1) * W + min(max(qx, 0), W - 1);
                        qp[k] = hitsPrev[2 * qi];
                        qn[k] = hitsPrev[2 * qi + 1];
                        qm[k] = meanPrev[qi];
                        qo[k] = momPrev[qi];
                    }
                    const float tol = r.planeTol * hp.w;
                    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sa = 0.0f, sY = 0.0f, sS = 0.0f;
                    unsigned nMin = 0xffffffffu;
                    bool kept = false;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const unsigned count = __float_as_uint(qo[k].z);
                        if (!in[k] || count == 0u || __float_as_int(qn[k].w) != objP) continue;
                        float nqx, nqy, nqz;
                        rp_normalise(qn[k].x, qn[k].y, qn[k].z, nqx, nqy, nqz);
                        if ((npx * nqx + npy * nqy) + npz * nqz < r.normalCosMin) continue;
                        const float dx = hp.x - qp[k].x, dy = hp.y - qp[k].y, dz = hp.z - qp[k].z;
                        if (fabsf((dx * npx + dy * npy) + dz * npz) > tol) continue;
                        const float s2 = count >= 2u ? qo[k].y / (float)(count - 1u) : 0.0f;
                        sw = sw + w[k];
                        sr = sr + w[k] * qm[k].x;
                        sg = sg + w[k] * qm[k].y;
                        sb = sb + w[k] * qm[k].z;
                        sa = sa + w[k] * qm[k].w;
                        sY = sY + w[k] * qo[k].x;
                        sS = sS + w[k] * s2;
                        nMin = min(nMin, count);
                        kept = true;
                    }
                    if (kept) {                                             // (a kept tap's weight is not zero: sw > 0)
                        cat = RP_REUSED;
                        nOut = min(nMin, r.maxHistory);
                        oMean.x = sr / sw;
                        oMean.y = sg / sw;
                        oMean.z = sb / sw;
                        oMean.w = sa / sw;
                        oMom.x = sY / sw;
                        oMom.y = (sS / sw) * (float)(nOut - 1u);
                        oMom.z = __uint_as_float(nOut);
                    }
                }
            }
            rp_store(meanCur + i, oMean);
            rp_store(momCur + i, oMom);
        }
        const bool reused = cat == RP_REUSED;
        cReused += reused ? 1u : 0u;
        cRejected += cat == RP_REJECTED ? 1u : 0u;
        cOffscreen += cat == RP_OFFSCREEN ? 1u : 0u;
        cMiss += cat == RP_MISS ? 1u : 0u;
        mnC = max(mnC, reused ? ~nOut : 0u);                    // n' >= 1: ~n' is never 0 for a reused pixel
        mxC = max(mxC, nOut);
        sumC += nOut;
    }
    // once per wave: reduce the registers across the lanes (full waves: no lane has left), lane 0 carries the wave's figures into
    // the workgroup's.  A lane's counters stay below its share of 2^31 pixels; its 64-bit sum goes through the 32-bit reduction in
    // three pieces whose wave totals fit (64 * 65535 < 2^22)
    const auto add = [](unsigned a, unsigned b) { return a + b; };
    const auto umax = [](unsigned a, unsigned b) { return max(a, b); };
    cReused = rt_wave_reduce(cReused, add);
    cRejected = rt_wave_reduce(cRejected, add);
    cOffscreen = rt_wave_reduce(cOffscreen, add);
    cMiss = rt_wave_reduce(cMiss, add);
    mnC = rt_wave_reduce(mnC, umax);
    mxC = rt_wave_reduce(mxC, umax);
    const unsigned long long sumHi = rt_wave_reduce((unsigned)(sumC >> 32), add);
    const unsigned long long sumMid = rt_wave_reduce((unsigned)(sumC >> 16) & 0xffffu, add);
    const unsigned long long sumLo = rt_wave_reduce((unsigned)sumC & 0xffffu, add);
    const unsigned long long sumW = (sumHi << 32) + (sumMid << 16) + sumLo;
    if (lane == 0u) {
        if (cReused) atomicAdd(&red[0], cReused);
        if (cRejected) atomicAdd(&red[1], cRejected);
        if (cOffscreen) atomicAdd(&red[2], cOffscreen);
        if (cMiss) atomicAdd(&red[3], cMiss);
        if (mnC) atomicMax(&red[4], mnC);
        if (mxC) atomicMax(&red[5], mxC);
        if (sumW) atomicAdd(&redSum, sumW);
    }
    __syncthreads();
    // flush: non-zero quantities only, no-return integer atomics, one per workgroup and quantity (the clear left minCount at
    // 2^32 - 1, the neutral element of the minimum); nPixels is workgroup 0's word alone
    if (tid == 0u) {
        if (red[0]) atomicAdd(&report[RR_NREUSED], red[0]);
        if (red[1]) atomicAdd(&report[RR_NREJECTED], red[1]);
        if (red[2]) atomicAdd(&report[RR_NOFFSCREEN], red[2]);
        if (red[3]) atomicAdd(&report[RR_NMISS], red[3]);
        if (red[4]) atomicMin(&report[RR_MINCOUNT], ~red[4]);
        if (red[5]) atomicMax(&report[RR_MAXCOUNT], red[5]);
        if (redSum) atomicAdd((unsigned long long *)(report + RR_SUMCOUNT), redSum);
        if (blockIdx.x == 0u) report[RR_NPIXELS] = (unsigned)W * (unsigned)H;
    }
}

hipError_t rt_launch_reproject(const void *accumPrev, const void *hitsPrev, const void *hitsCur, void *accumCur, void *report,
                               const RtReprojectRule &rule, hipStream_t s) {
    const size_t npx = (size_t)rule.width * (size_t)rule.height;
    const int tilesX = (rule.width + RP_TILE_W - 1) / RP_TILE_W;
    const int nTiles = tilesX * ((rule.height + RP_TILE_H - 1) / RP_TILE_H);  // at most (2^31 - 1) / 256 + W + H tiles: far below 2^31
    const int nSlots = RT_REPROJECT_XCD ? ((nTiles + 7) / 8) * 8 : nTiles;      // (padded for the XCD order: the slots past the last tile are empty)
    const int cap = RT_REPROJECT_WGS_PER_CU ? rt_cu_count() * RT_REPROJECT_WGS_PER_CU : nSlots;        // (a multiple of 8 on every gfx950 partition)
    const unsigned grid = (unsigned)(nSlots < cap ? nSlots : (RT_REPROJECT_XCD ? (cap + 7) / 8 * 8 : cap));
    hipError_t e = hipMemsetAsync(report, 0, RR_WORDS * 4, s);
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)((unsigned *)report + RR_MINCOUNT), -1, 1, s);     // the minimum's neutral element
    if (e != hipSuccess) return e;
    const f4 *prev = (const f4 *)accumPrev;
    f4 *cur = (f4 *)accumCur;
    hipLaunchKernelGGL(rt_reproject_kernel, dim3(grid), dim3(256), 0, s, prev, prev + npx, (const f4 *)hitsPrev, (const f4 *)hitsCur, cur,
                       cur + npx, rule, tilesX, nTiles, nSlots, (unsigned *)report);
    return hipGetLastError();
}
