// rt_denoise.hip -- the denoiser (rt_denoise_guide, rt_denoise; include/rt_mi355.h has the arithmetic, in order): the guide plane from
// first-hit records, the prepare pass (image + moments -> (r, g, b, var)), and one launch per a-trous iteration.
//
// An iteration moves 48 compulsory bytes per pixel (32 read, 16 written) and gathers 25 taps of 32 B (16 B of colour + variance,
// 16 B of guide) -- but what it is bound by is the vector ALU: the contract's 25 IEEE divisions and 25 exp_ per pixel, with the
// luminance, the normal weight and the five sums of every tap, are about 1750 VALU instructions per lane (70 per tap), which at 64
// lanes per clock and CU is 90 us for a 1080p frame; the kernel takes 75 to 100.  Where the taps come from decides the rest.  One
// lane per pixel, a workgroup of 256 lanes per tile of TW x 256/TW pixels.  Two forms of the tap fetch:
//   * LD = 1, 2 (steps 1 and 2): the tile plus an apron of 2*step texels of both planes is staged in LDS the way the bloom kernel
//     stages its patch (rt_post.hip): requested as one batch of independent 16-byte loads per lane into registers, written to LDS
//     afterwards, then every tap is a ds_read_b128.  With TW >= 32 a 16-lane group of a ds_read_b128 never spans two tile rows, and
//     16 consecutive 16-byte texels cover the 64 banks once: conflict-free at any row stride, so the rows are not padded.
//     Measured against the gather form: step 2 takes 76 instead of 121 us at 1080p, 276 instead of 451 at 4K.
//   * LD = 0 (steps 4, 8, 16, whose apron would exceed the tile; every step when RT_DENOISE_LDS is 0): global gathers, served
//     by the vector L1 / L2.  RT_DENOISE_TW_GATHER chooses the lane -> pixel map of a wave: 64 x 1 and 32 x 2 pixels read alike
//     (within 3 % either way, by step and size), 16 x 4 loses from step 8 on (step 16: 224 against 122 us at 1080p).
// RT_DENOISE_XCD gives each XCD one contiguous band of tiles (the bloom kernel's order), so that the lines neighbouring tiles share
// are served by one L2: at 1080p the gather steps take 98 instead of 121 us and four iterations 361 instead of 413; at 4K the
// LDS steps do not care and steps 8 and 16 lose 5 and 9 % (four iterations 1530 against 1509 us).  Kept for the 1080p gain.
// DESIGN.md 21 has the figures of every form.
// No atomics, no cross-workgroup traffic: every pixel is a pure function of the planes read, so the result is bit-identical from
// run to run and from form to form.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_denoise.h"
#include "rt_mesa_math.h"
#include "rt_wave.h"

#ifndef RT_DENOISE_LDS
#define RT_DENOISE_LDS 1            // 1: steps 1 and 2 fetch their taps from an LDS tile; 0: every step gathers from global memory
#endif
#ifndef RT_DENOISE_TW_LDS
#define RT_DENOISE_TW_LDS 32        // tile width of the LDS form (32 or 64; the tile is TW x 256/TW)
#endif
#ifndef RT_DENOISE_TW_GATHER
#define RT_DENOISE_TW_GATHER 32     // tile width of the gather form: 64, 32 or 16 -- a wave covers 64 x 1, 32 x 2 or 16 x 4 pixels
#endif
#ifndef RT_DENOISE_XCD
#define RT_DENOISE_XCD 1            // 1: XCD-aware tile order, tile = (id & 7) * (grid / 8) + id / 8; 0: tile = id
#endif

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool dn_usable(const f4 c) { return fabsf(c.x) <= kRtSampleLimit && fabsf(c.y) <= kRtSampleLimit && fabsf(c.z) <= kRtSampleLimit; }
__device__ __forceinline__ bool dn_skipped(float var) { return (__float_as_uint(var) >> 31) != 0u; }      // the sign bit of var is the mark
__device__ __forceinline__ float dn_max0(float x) { return x > 0.0f ? x : 0.0f; }
__device__ __forceinline__ float dn_min1(float x) { return x < 1.0f ? x : 1.0f; }

// the tile a workgroup works on, or -1 when the grid's padding gave it none
__device__ __forceinline__ int dn_tile(int nTiles) {
    const int tile = RT_DENOISE_XCD ? rt_xcd_tile() : (int)blockIdx.x;
    return tile < nTiles ? tile : -1;
}

}  // namespace

__global__ __launch_bounds__(256) void rt_denoise_guide_kernel(const f4 *__restrict__ hits, f4 *__restrict__ guide, unsigned nPixels) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nPixels) return;
    const f4 h = hits[2 * (size_t)i + 1];                   // {normal[3], object}: the upper half of the rt_hit
    const float s = (h.x * h.x + h.y * h.y) + h.z * h.z;
    f4 o = {0.0f, 0.0f, 0.0f, h.w};
    if (s > 0.0f) {
        const float r = sqrtf(s);
        o.x = h.x / r;
        o.y = h.y / r;
        o.z = h.z / r;
    }
    guide[i] = o;
}

// image (+ moments) -> plane A: (r, g, b, var).  Tiles of 64 x 4 pixels, a wave per row segment of 1 KiB.  The spatial estimate is a
// branch only the pixels below minCount take: 25 gathers of 16 B of image and 4 B of guide each.
template <bool MOMENTS>
__global__ __launch_bounds__(256) void rt_denoise_prepare_kernel(const f4 *__restrict__ image, const f4 *__restrict__ moments,
                                                                 const f4 *__restrict__ guide, f4 *__restrict__ dst, int W, int H, int tilesX,
                                                                 int nTiles, unsigned minCount) {
    const int tile = dn_tile(nTiles);
    if (tile < 0) return;
    const int x = (tile % tilesX) * 64 + (int)(threadIdx.x & 63u), y = (tile / tilesX) * 4 + (int)(threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * W + x;
    const f4 c = image[i];
    unsigned count = 1u;
    float M2 = 0.0f;
    if (MOMENTS) {
        const f4 m = moments[i];
        M2 = m.y;
        count = __float_as_uint(m.z);
    }
    float var;
    if (!dn_usable(c)) {
        var = -0.0f;
    } else if (count >= minCount) {
        const float nf = (float)count;
        var = M2 / (nf * (nf - 1.0f));
    } else {
        const int obj = __float_as_int(guide[i].w);
        float sY = 0.0f, sYY = 0.0f;
        int k = 0;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int qx = x + dx, qy = y + dy;
                if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                const size_t qi = (size_t)qy * W + qx;
                const f4 q = image[qi];
                if (__float_as_int(guide[qi].w) != obj || !dn_usable(q)) continue;
                const float Y = rt_luma(q.x, q.y, q.z);
                sY = sY + Y;
                sYY = sYY + Y * Y;
                k++;
            }
        }
        const float kf = (float)k;                          // k >= 1: the centre is usable and has its own object
        const float m1 = sY / kf, m2 = sYY / kf;
        var = dn_max0(m2 - m1 * m1) / (float)max(count, 1u);
    }
    const f4 o = {c.x, c.y, c.z, var};
    dst[i] = o;
}

// One a-trous iteration.  LD: 0 = taps gathered from global memory at the run-time `step`; 1, 2 = the step itself, taps from an LDS
// tile with an apron of 2 * LD texels.  alpha != NULL: the last iteration, which stores alpha[i].w in place of the variance.
template <int TW, int LD>
__global__ __launch_bounds__(256) void rt_denoise_iter_kernel(const f4 *__restrict__ src, const f4 *__restrict__ guide, f4 *__restrict__ dst,
                                                              const f4 *__restrict__ alpha, int W, int H, int step, int tilesX, int nTiles,
                                                              float sigmaLum, float lumEps, int power) {
    constexpr int TH = 256 / TW;
    constexpr int AP = 2 * LD, PW = TW + 2 * AP, PH = TH + 2 * AP, NT = PW * PH, NLD = (NT + 255) / 256;
    static_assert(TW * TH == 256 && (LD == 0 || TW >= 32), "a 16-lane group of a ds_read_b128 must stay inside one tile row");
    __shared__ f4 sC[LD ? NT : 1], sG[LD ? NT : 1];         // LD = 2, TW = 32: 2 * 640 * 16 B = 20 KiB
    const int tile = dn_tile(nTiles);
    if (tile < 0) return;                                   // (the whole workgroup)
    const int x0 = (tile % tilesX) * TW, y0 = (tile / tilesX) * TH;
    const int lx = (int)threadIdx.x % TW, ly = (int)threadIdx.x / TW;
    const int x = x0 + lx, y = y0 + ly;
    if (LD) {
        // the patch of both planes: requested as one batch of loads into registers, then written to LDS.  Texels outside the image
        // are zero; no tap reads them
        f4 pc[NLD], pg[NLD];
#pragma unroll
        for (int j = 0; j < NLD; j++) {
            const int k = (int)threadIdx.x + j * 256;
            const int gx = x0 + k % PW - AP, gy = y0 + k / PW - AP;
            const bool have = k < NT && gx >= 0 && gx < W && gy >= 0 && gy < H;
            const size_t gi = have ? (size_t)gy * W + gx : 0;
            const f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
            pc[j] = have ? src[gi] : zero;
            pg[j] = have ? guide[gi] : zero;
        }
#pragma unroll
        for (int j = 0; j < NLD; j++) {
            const int k = (int)threadIdx.x + j * 256;
            if (k < NT) {
                sC[k] = pc[j];
                sG[k] = pg[j];
            }
        }
        __syncthreads();
    }
    if (x >= W || y >= H) return;
    const int d = LD ? LD : step;
    const size_t i = (size_t)y * W + x;
    const int li = (ly + AP) * PW + lx + AP;                // the centre in the LDS patch
    const f4 cp = LD ? sC[li] : src[i];
    const f4 gp = LD ? sG[li] : guide[i];
    const bool skipP = dn_skipped(cp.w);
    const int objP = __float_as_int(gp.w);
    // the prefiltered variance: 3 x 3 Gaussian at stride 1 over the kept taps (inside, usable, the centre's object), renormalised
    float sg = 0.0f, sgv = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const float vq = LD ? sC[li + dy * PW + dx].w : src[(size_t)qy * W + qx].w;
            const float oq = LD ? sG[li + dy * PW + dx].w : guide[(size_t)qy * W + qx].w;
            if (dn_skipped(vq) || __float_as_int(oq) != objP) continue;
            const float g = (dx ? 0.25f : 0.5f) * (dy ? 0.25f : 0.5f);
            sg = sg + g;
            sgv = sgv + g * vq;
        }
    }
    const float gv = sg > 0.0f ? sgv / sg : 0.0f;
    const float sl = sigmaLum * sqrtf(gv) + lumEps;
    const float Yp = rt_luma(cp.x, cp.y, cp.z);
    float sw = 0.0f, sr = 0.0f, sgr = 0.0f, sb = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + d * dx, qy = y + d * dy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            f4 cq, gq;
            if (LD) {
                const int lq = li + (LD * dy) * PW + LD * dx;
                cq = sC[lq];
                gq = sG[lq];
            } else {
                const size_t qi = (size_t)qy * W + qx;
                cq = src[qi];
                gq = guide[qi];
            }
            if (dn_skipped(cq.w) || __float_as_int(gq.w) != objP) continue;
            float c = dn_min1(dn_max0((gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z));
            for (int k = 0; k < power; k++) c = c * c;
            const float wn = objP < 0 ? 1.0f : c;
            const float wl = skipP ? 0.0f : fabsf(Yp - rt_luma(cq.x, cq.y, cq.z)) / sl;
            const float hx = dx == 0 ? 0.375f : (dx == 1 || dx == -1) ? 0.25f : 0.0625f;
            const float hy = dy == 0 ? 0.375f : (dy == 1 || dy == -1) ? 0.25f : 0.0625f;
            const float w = ((hx * hy) * wn) * rtm::exp_(-wl);
            sw = sw + w;
            sr = sr + w * cq.x;
            sgr = sgr + w * cq.y;
            sb = sb + w * cq.z;
            sv = sv + (w * w) * cq.w;
        }
    }
    f4 o = {cp.x, cp.y, cp.z, 0.0f};
    if (!(sw == 0.0f)) {
        o.x = sr / sw;
        o.y = sgr / sw;
        o.z = sb / sw;
        o.w = sv / (sw * sw);
    }
    if (skipP) o.w = -0.0f;
    if (alpha) o.w = alpha[i].w;
    dst[i] = o;
}

hipError_t rt_launch_denoise_guide(const void *hits, void *guide, unsigned nPixels, hipStream_t s) {
    hipLaunchKernelGGL(rt_denoise_guide_kernel, dim3((nPixels + 255u) / 256u), dim3(256), 0, s, (const f4 *)hits, (f4 *)guide, nPixels);
    return hipGetLastError();
}

namespace {

// tiles of tw x 256/tw pixels over the image: the grid (padded to a multiple of 8 for the XCD order), tiles per row, tiles
struct DnGrid {
    int tilesX, nTiles;
    dim3 grid;
    DnGrid(int W, int H, int tw) {
        const int th = 256 / tw;
        tilesX = (W + tw - 1) / tw;
        nTiles = tilesX * ((H + th - 1) / th);              // at most (2^31 - 1) / 256 + W + H tiles: far below 2^31
        grid = dim3((unsigned)(RT_DENOISE_XCD ? ((nTiles + 7) / 8) * 8 : nTiles));
    }
};

template <int TW, int LD>
void dn_launch_iter(const f4 *src, const f4 *guide, f4 *dst, const f4 *alpha, int step, const RtDenoiseRule &r, hipStream_t s) {
    const DnGrid g(r.width, r.height, TW);
    hipLaunchKernelGGL((rt_denoise_iter_kernel<TW, LD>), g.grid, dim3(256), 0, s, src, guide, dst, alpha, r.width, r.height, step, g.tilesX,
                       g.nTiles, r.sigmaLum, r.lumEps, r.normalLog2Power);
}

}  // namespace

hipError_t rt_launch_denoise(const void *image, const void *moments, const void *guide, void *scratch, void *out, const RtDenoiseRule &r,
                             hipStream_t s) {
    const size_t npx = (size_t)r.width * (size_t)r.height;
    f4 *plane[2] = {(f4 *)scratch, (f4 *)scratch + npx};
    const f4 *g = (const f4 *)guide;
    {
        const DnGrid pg(r.width, r.height, 64);
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, pg.grid, dim3(256), 0, s, (const f4 *)image, (const f4 *)moments, g, plane[0], r.width, r.height, pg.tilesX,
                               pg.nTiles, r.minCount);
        };
        if (moments) go(rt_denoise_prepare_kernel<true>);
        else go(rt_denoise_prepare_kernel<false>);
    }
    for (int it = 0; it < r.iterations; it++) {
        const bool last = it == r.iterations - 1;
        const f4 *src = plane[it & 1];
        f4 *dst = last ? (f4 *)out : plane[(it & 1) ^ 1];
        const f4 *alpha = last ? (const f4 *)image : nullptr;
        const int step = 1 << it;
        if (RT_DENOISE_LDS && step == 1) dn_launch_iter<RT_DENOISE_TW_LDS, 1>(src, g, dst, alpha, step, r, s);
        else if (RT_DENOISE_LDS && step == 2) dn_launch_iter<RT_DENOISE_TW_LDS, 2>(src, g, dst, alpha, step, r, s);
        else dn_launch_iter<RT_DENOISE_TW_GATHER, 0>(src, g, dst, alpha, step, r, s);
    }
    return hipGetLastError();
}
