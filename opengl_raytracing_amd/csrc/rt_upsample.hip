// rt_upsample.hip -- first-hit-guided upsampling (rt_upsample, rt_image_put_at; include/rt_mi355.h has the arithmetic, in order): a
// low-resolution frame reconstructed at full resolution by a joint bilateral filter that never mixes two objects, steered by the
// first hits of both resolutions, and the list of the pixels no low-resolution ray saw on their own surface.
//
// RECONSTRUCT takes the judge kernel's geometry (rt_adaptive.hip): a wave per tile of 8 x 8 output pixels (lane l is pixel (l & 7,
// l >> 3) of it), a workgroup of four waves per chunk of 32 consecutive tiles, at most kSelectMaxWgs workgroups that own a contiguous
// run of chunks each.  A lane reads the upper half of its rt_hit (the normal and the object: 16 of the record's 32 bytes), gathers
// the 2 x 2 low-resolution taps -- the upper half of each tap's rt_hit and its colour, 32 B -- and stores 16 bytes.  The ballot of
// the lanes whose taps did not carry the weight is the tile's word of rt_accum_select's scratch, their count and the orphans' are
// the workgroup's two totals: rt_select_scan_kernel and rt_select_emit_kernel run on them as they stand.
// A wave takes its tiles one at a time: the hit, then the four taps (predicated loads, no branch in between), then the arithmetic.
// Only holes enter the 4 x 4 window: a divergent branch behind stage 1.  Keeping the loads of 2 or 4 tiles in flight was tried and
// bought 0 to 3 %: the gathers are not what bounds the kernel; the dependent chains of the contract's IEEE divisions
// and square roots (five normalisations and four quotients per pixel) at two waves per SIMD are, which is why staging the taps in
// LDS was not pursued.
// The taps are gathers through the vector L1 / L2: the 2 x 2 footprint of a tile is at most (8 * low / high + 2)^2 records of 48 B,
// and neighbouring lanes share most of them.
// The normalisation of both normals is rt_denoise_guide_kernel's, done here per tap: no guide planes, no launch in front.
// No atomics beyond the workgroup's own two LDS counters (integers), no cross-workgroup traffic: bit-identical from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_adaptive.h"
#include "rt_upsample.h"
#include "rt_wave.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr unsigned kTile = kSelectTile, kTilesPerChunk = kSelectTilesPerChunk, kTilesPerWave = kSelectTilesPerChunk / 4;
static_assert(kTile * kTile == 64, "a tile is a wave");

__device__ __forceinline__ float up_max0(float x) { return x > 0.0f ? x : 0.0f; }
__device__ __forceinline__ float up_min1(float x) { return x < 1.0f ? x : 1.0f; }
__device__ __forceinline__ bool up_usable(const f4 c) {
    return fabsf(c.x) <= kRtSampleLimit && fabsf(c.y) <= kRtSampleLimit && fabsf(c.z) <= kRtSampleLimit && fabsf(c.w) <= kRtSampleLimit;
}

// {n^, object} of the upper half of an rt_hit: rt_denoise_guide's rule
__device__ __forceinline__ f4 up_guide(const f4 h) {
    const float s = (h.x * h.x + h.y * h.y) + h.z * h.z;
    f4 o = {0.0f, 0.0f, 0.0f, h.w};
    if (s > 0.0f) {
        const float r = sqrtf(s);
        o.x = h.x / r;
        o.y = h.y / r;
        o.z = h.z / r;
    }
    return o;
}

// The position of output coordinate v (of `high`) in the low image (of `low` <= high): i0 = floor(((2v + 1) * low - high) / (2 * high)),
// >= -1, and the fraction behind it, in 64-bit integers.  2v + 1, the denominator 2 * high (< 2^32), the quotient (< low) and the
// remainder (< 2 * high) fit 32 bits each, so the products are 32 x 32 -> 64 and the two conversions to float are of 32-bit values.
__device__ __forceinline__ void up_position(unsigned v, unsigned low, unsigned high, int &i0, float &f) {
    const unsigned den = 2u * high;
    const u64 a = (u64)(2u * v + 1u) * low;
    unsigned rem;
    if (a < (u64)high) {                                    // the numerator is in [-high, 0): the quotient is -1
        i0 = -1;
        rem = (unsigned)a + high;                           // (a - high) + 2 * high
    } else {
        const u64 num = a - high;
        const unsigned q = (unsigned)(num / den);
        i0 = (int)q;                                        // < low
        rem = (unsigned)(num - (u64)q * den);
    }
    f = (float)rem / (float)den;
}

// the normal weight of a tap of the centre's object (gp: the centre's guide, hq: the upper half of the tap's rt_hit)
__device__ __forceinline__ float up_normal_weight(const f4 gp, const f4 hq, int power) {
    const f4 gq = up_guide(hq);
    float c = up_min1(up_max0((gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z));
    for (int k = 0; k < power; k++) c = c * c;
    return __float_as_int(gp.w) < 0 ? 1.0f : c;
}

struct UpSums {
    float sw;
    f4 s;
    __device__ __forceinline__ void clear() {
        sw = 0.0f;
        s.x = s.y = s.z = s.w = 0.0f;
    }
    __device__ __forceinline__ void add(float w, const f4 c) {
        sw = sw + w;
        s.x = s.x + w * c.x;
        s.y = s.y + w * c.y;
        s.z = s.z + w * c.z;
        s.w = s.w + w * c.w;
    }
    __device__ __forceinline__ f4 mean() const {
        f4 o;
        o.x = s.x / sw;
        o.y = s.y / sw;
        o.z = s.z / sw;
        o.w = s.w / sw;
        return o;
    }
};

}  // namespace

__global__ __launch_bounds__(256) void rt_upsample_kernel(const f4 *__restrict__ low, const f4 *__restrict__ hitsLow, const f4 *__restrict__ hitsHigh,
                                                          f4 *__restrict__ out, unsigned width, unsigned height, unsigned lowW, unsigned lowH,
                                                          int power, float minWeight, unsigned tilesX, unsigned nTiles, unsigned nChunks,
                                                          unsigned chunksPerWg, u64 *__restrict__ ballots, unsigned *__restrict__ totals) {
    __shared__ unsigned red[2];                             // holes, orphans
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid < 2u) red[tid] = 0u;
    __syncthreads();
    const unsigned c0 = blockIdx.x * chunksPerWg;
    const unsigned c1 = min(c0 + chunksPerWg, nChunks);
    const int LW = (int)lowW, LH = (int)lowH;
    const f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    unsigned nHole = 0u, nOrphan = 0u;                      // wave-uniform
    for (unsigned chunk = c0; chunk < c1; chunk++) {
#pragma unroll 1
        for (unsigned b = 0; b < kTilesPerWave; b++) {
            const unsigned tile = chunk * kTilesPerChunk + wave * kTilesPerWave + b;        // <= nTiles + 31 < 2^32
            const unsigned ty = tile / tilesX, tx = tile - ty * tilesX;
            const unsigned px = tx * kTile + (lane & 7u), py = ty * kTile + (lane >> 3);
            const bool have = tile < nTiles && px < width && py < height;
            const f4 hp = have ? hitsHigh[2 * ((size_t)py * width + px) + 1] : zero;        // (the index is formed for pixels of the image only)
            // the position and the 2 x 2 taps: a tap's index is formed once the tap is known to lie inside the low image
            int ix0, iy0;
            float fx, fy;
            up_position(px, lowW, width, ix0, fx);
            up_position(py, lowH, height, iy0, fy);
            bool in[4];
            f4 hq[4], cq[4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int qx = ix0 + (t & 1), qy = iy0 + (t >> 1);
                in[t] = have && qx >= 0 && qx < LW && qy >= 0 && qy < LH;
                const size_t qi = in[t] ? (size_t)qy * lowW + (size_t)qx : 0;
                hq[t] = in[t] ? hitsLow[2 * qi + 1] : zero;
                cq[t] = in[t] ? low[qi] : zero;
            }
            const f4 gp = up_guide(hp);
            const int objP = __float_as_int(gp.w);
            // stage 1: the 2 x 2 taps with their bilinear weights, j outer and i inner
            const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
            UpSums a;
            a.clear();
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const bool keep = in[t] && __float_as_int(hq[t].w) == objP && up_usable(cq[t]);
                const float w = (wx[t & 1] * wy[t >> 1]) * up_normal_weight(gp, hq[t], power);
                if (keep) a.add(w, cq[t]);
            }
            const bool hole = have && !(a.sw > 0.0f && a.sw >= minWeight);
            bool orphan = false;
            f4 o = zero;
            if (have && !hole) o = a.mean();
            if (hole) {
                // stage 2: a hole looks for its own surface in the 4 x 4 window, by the normal weight alone
                a.clear();
                for (int j = -1; j <= 2; j++) {
                    for (int i = -1; i <= 2; i++) {
                        const int qx = ix0 + i, qy = iy0 + j;
                        if (qx < 0 || qx >= LW || qy < 0 || qy >= LH) continue;
                        const size_t qi = (size_t)qy * lowW + (size_t)qx;
                        const f4 h = hitsLow[2 * qi + 1];
                        if (__float_as_int(h.w) != objP) continue;
                        const f4 c = low[qi];
                        if (!up_usable(c)) continue;
                        const float w = up_normal_weight(gp, h, power);
                        if (w == 0.0f) continue;
                        a.add(w, c);
                    }
                }
                if (a.sw > 0.0f) {
                    o = a.mean();
                } else {
                    // stage 3: an orphan takes the low pixel it lies in, as it stands
                    orphan = true;
                    const unsigned lx = min((unsigned)(((u64)px * lowW) / width), lowW - 1u);
                    const unsigned ly = min((unsigned)(((u64)py * lowH) / height), lowH - 1u);
                    o = low[(size_t)ly * lowW + lx];
                }
            }
            if (have) out[(size_t)py * width + px] = o;
            const u64 bal = __builtin_amdgcn_ballot_w64(hole);
            const u64 orp = __builtin_amdgcn_ballot_w64(orphan);
            if (lane == 0u && tile < nTiles) ballots[tile] = bal;
            nHole += (unsigned)__builtin_popcountll(bal);
            nOrphan += (unsigned)__builtin_popcountll(orp);
        }
    }
    if (lane == 0u) {
        if (nHole) atomicAdd(&red[0], nHole);
        if (nOrphan) atomicAdd(&red[1], nOrphan);
    }
    __syncthreads();
    if (tid < 2u) totals[tid * kSelectMaxWgs + blockIdx.x] = red[tid];
}

// One lane per list entry: image[pixels[k]] = samples[k]; an entry outside the image forms no address.
__global__ __launch_bounds__(256) void rt_image_put_kernel(const f4 *__restrict__ samples, const uint2 *__restrict__ pixels, size_t n,
                                                           f4 *__restrict__ image, unsigned width, unsigned height) {
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const uint2 px = pixels[k];
    if (px.x < width && px.y < height) image[(size_t)px.y * width + px.x] = samples[k];
}

hipError_t rt_launch_upsample(const void *low, const void *hitsLow, const void *hitsHigh, void *out, const RtUpsampleRule &r, void *pixels,
                              unsigned capacity, void *scratch, void *selState, hipStream_t s) {
    const RtSelectGrid g(r.width, r.height);
    unsigned *totals = (unsigned *)scratch;
    u64 *ballots = (u64 *)((char *)scratch + kSelectScratchHeader);
    hipLaunchKernelGGL(rt_upsample_kernel, dim3(g.nWgs), dim3(256), 0, s, (const f4 *)low, (const f4 *)hitsLow, (const f4 *)hitsHigh, (f4 *)out,
                       (unsigned)r.width, (unsigned)r.height, (unsigned)r.lowWidth, (unsigned)r.lowHeight, r.normalLog2Power, r.minWeight, g.tilesX,
                       g.nTiles, g.nChunks, g.chunksPerWg, ballots, totals);
    return rt_launch_select_from_ballots(scratch, r.width, r.height, pixels, capacity, selState, s);
}

hipError_t rt_launch_image_put_at(const void *samples, const void *pixels, size_t n, void *image, int width, int height, hipStream_t s) {
    hipLaunchKernelGGL(rt_image_put_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, s, (const f4 *)samples, (const uint2 *)pixels, n,
                       (f4 *)image, (unsigned)width, (unsigned)height);
    return hipGetLastError();
}
