// rt_display.hip -- the display path on the device, as gfx950 HIP kernels: any rgba32f surface -> RGBA8 or YUV 4:2:0 behind an
// exposure, a tone curve and a transfer function, and the exposure meter that feeds it.  It has no counterpart in the
// reference beyond the quantisation of its 8-bit default framebuffer; include/rt_mi355.h defines every byte.  The entry points
// are in rt_display.cpp, the ring that delivers packed frames to the host in rt_present.cpp.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>

#include "rt_display.h"
#include "rt_fastmath.h"
#include "rt_meter.h"
#include "rt_wave.h"

// =========================================================================================
// Display packing: any rgba32f surface -> RGBA8, the quantisation an 8-bit default framebuffer applies to what
// bloom_combineFs.glsl draws into it (ForwardShadingPipeline.cpp:220-228, then glfwSwapBuffers).
// Purely bandwidth-bound: 16 B read + 4 B written per pixel.  A lane owns four consecutive pixels of ONE row (a "quad";
// the last quad of a row is short when W % 4 != 0, so a lane never straddles rows): four 16-B loads issued together,
// one 16-B store; consecutive lanes take consecutive quads, so a wave reads 4 KiB and writes 1 KiB contiguously.
// FLIP_ROWS only changes the row the store goes to.  Per colour channel (include/rt_mi355.h has the definition):
// y = x * exposure; NaN and y <= 0 -> 0, y >= 1 -> 255; LINEAR q = rint(y * 255) (v_rndne_f32: nearest even);
// SRGB q = #{i in 1..255 : T[i] <= y}, T the host-built table of rt_display_thresholds().  The kernel finds that
// count with a branch-free 8-step descent of the table laid out as an implicit search tree in LDS (node n's
// children are 2n and 2n + 1, level d occupies the 2^d consecutive entries from 2^d): after 8 steps the node
// number minus 256 IS the count, and the lanes of a wave spread over consecutive banks at every level where a
// sorted layout would put levels 2..5 on one or two banks.  No transcendental runs on the device.
// =========================================================================================
struct RtDisplayTree { float node[256]; };       // node[0] unused; 1 KiB of kernel arguments, staged into LDS by each workgroup

namespace {
struct DisplayTables {
    float thresholds[256];
    RtDisplayTree tree;
};
const DisplayTables &display_tables() {
    static const DisplayTables tables = [] {               // built once, on first use (thread-safe: a function-local static)
        DisplayTables t;
        t.thresholds[0] = 0.0f;
        for (int i = 1; i < 256; i++) {          // the sRGB EOTF at the midpoint between codes i - 1 and i, in double
            const double s = ((double)i - 0.5) / 255.0;
            const double f = s <= 0.04045 ? s / 12.92 : pow((s + 0.055) / 1.055, 2.4);
            t.thresholds[i] = (float)f;
        }
        t.tree.node[0] = 0.0f;
        for (int d = 0; d < 8; d++)              // level d, position p: the key of rank (2p + 1) * 2^(7 - d)
            for (int p = 0; p < (1 << d); p++) t.tree.node[(1 << d) + p] = t.thresholds[(2 * p + 1) << (7 - d)];
        return t;
    }();
    return tables;
}

template <bool SRGB>
__device__ __forceinline__ unsigned display_code(float x, float exposure, const float *tree) {
    const float y = x * exposure;
    const float yc = !(y > 0.0f) ? 0.0f : (y >= 1.0f ? 1.0f : y);     // NaN, -0, -inf -> 0; +inf -> 1
    if constexpr (SRGB) {
        unsigned n = 1;
#pragma unroll
        for (int d = 0; d < 8; d++) n = 2 * n + (tree[n] <= yc ? 1u : 0u);
        return n - 256u;
    } else {
        return (unsigned)rintf(yc * 255.0f);
    }
}
// The tone curves of rt_display_pack_toned (include/rt_mi355.h), on ys = y for y > 0 (at most 65536), else 0: both map 0 to 0, so
// the curve runs branch-free in front of display_code's own rule.  Every operation is a single fp32 instruction (the build has
// -ffp-contract=off), the division is hipcc's correctly rounded one.
enum { TONE_NONE = 0, TONE_REINHARD = 1, TONE_ACES = 2 };
template <int TONE>
__device__ __forceinline__ float tone_curve(float x, float e, float invW2) {
    if constexpr (TONE == TONE_NONE) {
        return x;
    } else {
        const float y = x * e;
        const float ys = !(y > 0.0f) ? 0.0f : fminf(y, 65536.0f);
        if constexpr (TONE == TONE_REINHARD) {
            const float a = ys * invW2, b = 1.0f + a, c = ys * b, d = 1.0f + ys;
            return c / d;
        } else {
            const float n = ys * ((2.51f * ys) + 0.03f), d = (ys * ((2.43f * ys) + 0.59f)) + 0.14f;
            return n / d;
        }
    }
}

// QUADS: W % 4 == 0 -- every quad is whole and every output quad 16-B aligned: no predicate anywhere, one 16-B store.
// Otherwise the rows of the output are only 4-B aligned and the last quad of a row is short: predicated loads, 4-B stores.
// One body for the untoned kernel (rt_display_pack / rt_present_submit: TONE_NONE, the exposure a kernel argument) and the
// toned one below; with TONE_NONE display_code sees (x, exposure) exactly as before.
template <bool SRGB, bool QUADS, int TONE>
__device__ __forceinline__ void display_pack_body(const float4 *__restrict__ in, unsigned *__restrict__ out, int W, int H, unsigned quadsPerRow,
                                                  unsigned nQuads, int flip, float exposure, float invW2, const RtDisplayTree &tree, float *lds) {
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    const bool valid = g < nQuads;                           // (no early return: the sRGB form has a barrier below)
    const unsigned j = g / quadsPerRow, q = g - j * quadsPerRow;
    const int x0 = (int)(q * 4u);
    const int r = !valid ? 0 : (QUADS ? 4 : min(4, W - x0)); // pixels of this quad: 4, or 1..3 at a ragged row end
    const float4 *src = in + (size_t)j * W + x0;
    float4 p[4];
#pragma unroll
    for (int k = 0; k < 4; k++) p[k] = k < r ? src[k] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if constexpr (SRGB) {                                    // the table goes to LDS while the pixels are on their way
        lds[threadIdx.x] = tree.node[threadIdx.x];
        __syncthreads();
    }
    if (!valid) return;
    // TONE_NONE: code(x * exposure); a curve: code(t * 1), t = curve(x * exposure) -- the product with 1.0f is exact
    const float ce = TONE == TONE_NONE ? exposure : 1.0f;
    auto code = [&](float x) -> unsigned { return display_code<SRGB>(tone_curve<TONE>(x, exposure, invW2), ce, lds); };
    unsigned px[4];
#pragma unroll
    for (int k = 0; k < 4; k++) px[k] = code(p[k].x) | (code(p[k].y) << 8) | (code(p[k].z) << 16) | 0xff000000u;
    const unsigned jo = flip ? (unsigned)(H - 1) - j : j;
    unsigned *dst = out + (size_t)jo * W + x0;
    if constexpr (QUADS) {
        *(uint4 *)dst = make_uint4(px[0], px[1], px[2], px[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < r) dst[k] = px[k];
    }
}
}  // namespace

const float *rt_display_thresholds() { return display_tables().thresholds; }

template <bool SRGB, bool QUADS>
__global__ __launch_bounds__(256) void rt_display_pack_kernel(const float4 *__restrict__ in, unsigned *__restrict__ out, int W, int H,
                                                              unsigned quadsPerRow, unsigned nQuads, int flip, float exposure,
                                                              const RtDisplayTree tree) {
    __shared__ float lds[SRGB ? 256 : 1];
    display_pack_body<SRGB, QUADS, TONE_NONE>(in, out, W, H, quadsPerRow, nQuads, flip, exposure, 0.0f, tree, lds);
}

// rt_display_pack_toned / rt_present_submit_toned: the same pack with a tone curve and, when dExposure is not NULL, the
// descriptor's exposure multiplied by a float in device memory (rt_meter's state, written earlier on the same stream).  The
// address is a kernel argument and so wave-uniform: one scalar load and one multiply per wave, no host round trip.
template <bool SRGB, bool QUADS, int TONE>
__global__ __launch_bounds__(256) void rt_display_pack_toned_kernel(const float4 *__restrict__ in, unsigned *__restrict__ out, int W, int H,
                                                                    unsigned quadsPerRow, unsigned nQuads, int flip, float exposure,
                                                                    const float *__restrict__ dExposure, float invW2,
                                                                    const RtDisplayTree tree) {
    __shared__ float lds[SRGB ? 256 : 1];
    const float e = dExposure ? exposure * *dExposure : exposure;
    display_pack_body<SRGB, QUADS, TONE>(in, out, W, H, quadsPerRow, nQuads, flip, e, invW2, tree, lds);
}

// The run-time (tone, srgb) of a launch as compile-time constants: f(integral_constant<int, TONE_*>, bool_constant<srgb>).
template <class F>
void with_tone_and_transfer(int tone, int srgb, F f) {
    auto withTone = [&](auto srgbC) {
        if (tone == TONE_NONE) f(std::integral_constant<int, TONE_NONE>{}, srgbC);
        else if (tone == TONE_REINHARD) f(std::integral_constant<int, TONE_REINHARD>{}, srgbC);
        else f(std::integral_constant<int, TONE_ACES>{}, srgbC);
    };
    if (srgb) withTone(std::true_type{});
    else withTone(std::false_type{});
}

hipError_t rt_launch_display_pack(const void *image, void *out, int W, int H, int srgb, int flip, float exposure, hipStream_t s) {
    const unsigned quadsPerRow = ((unsigned)W + 3u) / 4u;
    const unsigned long long nQuads = (unsigned long long)quadsPerRow * (unsigned)H;
    if (nQuads > 0xffffff00ull) return hipErrorInvalidValue;       // (callers refuse such frames first)
    const dim3 grid((unsigned)((nQuads + 255) / 256));
    const RtDisplayTree &tree = display_tables().tree;
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, (const float4 *)image, (unsigned *)out, W, H, quadsPerRow, (unsigned)nQuads,
                           flip, exposure, tree);
    };
    const bool quads = (W & 3) == 0;
    with_tone_and_transfer(TONE_NONE, srgb, [&](auto, auto srgbC) {      // (this kernel has no tone parameter)
        constexpr bool S = decltype(srgbC)::value;
        quads ? go(rt_display_pack_kernel<S, true>) : go(rt_display_pack_kernel<S, false>);
    });
    return hipGetLastError();
}

// tone: 0 none, 1 Reinhard (invW2 = 1 / white^2), 2 ACES; dExposure: device float or NULL.  (none, NULL) is the untoned launch.
hipError_t rt_launch_display_pack_toned(const void *image, void *out, int W, int H, int srgb, int flip, float exposure, int tone,
                                        float invW2, const void *dExposure, hipStream_t s) {
    if (tone == TONE_NONE && !dExposure) return rt_launch_display_pack(image, out, W, H, srgb, flip, exposure, s);
    const unsigned quadsPerRow = ((unsigned)W + 3u) / 4u;
    const unsigned long long nQuads = (unsigned long long)quadsPerRow * (unsigned)H;
    if (nQuads > 0xffffff00ull || tone < TONE_NONE || tone > TONE_ACES) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((nQuads + 255) / 256));
    const RtDisplayTree &tree = display_tables().tree;
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, (const float4 *)image, (unsigned *)out, W, H, quadsPerRow, (unsigned)nQuads,
                           flip, exposure, (const float *)dExposure, invW2, tree);
    };
    const bool quads = (W & 3) == 0;
    with_tone_and_transfer(tone, srgb, [&](auto toneC, auto srgbC) {
        constexpr int T = decltype(toneC)::value;
        constexpr bool S = decltype(srgbC)::value;
        quads ? go(rt_display_pack_toned_kernel<S, true, T>) : go(rt_display_pack_toned_kernel<S, false, T>);
    });
    return hipGetLastError();
}

// =========================================================================================
// YUV 4:2:0 packing (rt_display_pack_yuv, include/rt_mi355.h): the same rgba32f surface -> the NV12 / I420 frame a video encoder
// takes.  The R'G'B' codes are the pack's own (display_code and tone_curve above, the sRGB tree staged in LDS the same way); behind
// them an integer matrix with Q16 coefficients that arrive as kernel arguments (wave-uniform).  Bandwidth-bound like the pack: 16 B
// read, 1.5 B written per pixel.  A lane owns a block of RT_YUV_BW x 2 OUTPUT pixels -- one row pair, so every chroma sample's four
// pixels sit in one lane and no lane talks to another -- and consecutive lanes own consecutive blocks of the row pair: a wave reads
// two contiguous runs of 64 * RT_YUV_BW * 16 B.
// FAST (W % 8 == 0 and H even): every block is whole and every segment a lane stores is naturally aligned (the planes start at
// multiples of 8, I420's chroma rows at multiples of 4): 2 x RT_YUV_BW 16-B loads, two RT_YUV_BW-byte luma stores, one
// RT_YUV_BW-byte NV12 chroma store or two half as wide for I420, no edge predicate.  Otherwise the loads go to coordinates clamped
// into the image (the edge replication of the definition) and every byte is stored on its own under its predicate.
// Each output byte is written by exactly one lane, once.
// =========================================================================================
#ifndef RT_YUV_BW
#define RT_YUV_BW 4               // block width in pixels: 4 or 8 (DESIGN.md 16 has both measured: 8 costs occupancy and time)
#endif
static_assert(RT_YUV_BW == 8 || RT_YUV_BW == 4, "a block is 8 or 4 pixels wide");
struct RtYuvCoef { int v[12]; };  // rt_display_yuv_coeffs' order: cYR cYG cYB yOff | cBR cBG cBB 0 | cRR cRG cRB 0

namespace {
template <int N> struct yuv_seg;                              // N bytes stored at once
template <> struct yuv_seg<8> { typedef uint2 type; };
template <> struct yuv_seg<4> { typedef unsigned type; };
template <> struct yuv_seg<2> { typedef unsigned short type; };
// bytes b[0..N-1] (each 0..255) to p, N-byte aligned, as one store
template <int N>
__device__ __forceinline__ void yuv_store(unsigned char *p, const unsigned (&b)[N]) {
    if constexpr (N == 2) {
        *(unsigned short *)p = (unsigned short)(b[0] | (b[1] << 8));
    } else {
        unsigned w[N / 4];
#pragma unroll
        for (int k = 0; k < N / 4; k++) w[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | (b[4 * k + 3] << 24);
        if constexpr (N == 8) *(uint2 *)p = make_uint2(w[0], w[1]);
        else *(unsigned *)p = w[0];
    }
}
}  // namespace

template <bool SRGB, int TONE, bool I420, bool FAST>
__global__ __launch_bounds__(256) void rt_display_pack_yuv_kernel(const float4 *__restrict__ in, unsigned char *__restrict__ out, int W, int H,
                                                                  unsigned blocksPerRow, unsigned nBlocks, int flip, float exposure,
                                                                  const float *__restrict__ dExposure, float invW2, const RtYuvCoef cf,
                                                                  const RtDisplayTree tree) {
    constexpr int BW = RT_YUV_BW;
    __shared__ float lds[SRGB ? 256 : 1];
    const float e = dExposure ? exposure * *dExposure : exposure;      // (wave-uniform: one scalar load, one multiply)
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    const bool valid = g < nBlocks;                           // (no early return: the sRGB form has a barrier below)
    const unsigned jp = g / blocksPerRow, bq = g - jp * blocksPerRow;
    const int x0 = (int)bq * BW, j0 = (int)jp * 2;            // the block's first output column and row
    const int j1 = FAST ? j0 + 1 : min(j0 + 1, H - 1);        // its second output row, replicated at the top of an odd frame
    const int jr[2] = {flip ? H - 1 - j0 : j0, flip ? H - 1 - j1 : j1};       // the image rows behind the two output rows
    float4 p[2][BW];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const float4 *src = in + (size_t)jr[r] * W;
#pragma unroll
        for (int k = 0; k < BW; k++) {
            const int x = FAST ? x0 + k : min(x0 + k, W - 1); // the right edge replicated
            p[r][k] = valid ? src[x] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
    if constexpr (SRGB) {                                     // the table goes to LDS while the pixels are on their way
        lds[threadIdx.x] = tree.node[threadIdx.x];
        __syncthreads();
    }
    if (!valid) return;
    const float ce = TONE == TONE_NONE ? e : 1.0f;            // as display_pack_body: code(x * e), or code(curve(x * e) * 1)
    auto code = [&](float x) -> int { return (int)display_code<SRGB>(tone_curve<TONE>(x, e, invW2), ce, lds); };
    unsigned yb[2][BW], cb[BW / 2], cr[BW / 2];
#pragma unroll
    for (int c = 0; c < BW / 2; c++) {                        // one chroma sample: columns 2c, 2c + 1 of both rows
        int Rs = 0, Gs = 0, Bs = 0;
#pragma unroll
        for (int r = 0; r < 2; r++) {
#pragma unroll
            for (int d = 0; d < 2; d++) {
                const float4 q = p[r][2 * c + d];
                const int R = code(q.x), G = code(q.y), B = code(q.z);
                Rs += R; Gs += G; Bs += B;
                yb[r][2 * c + d] = (unsigned)(cf.v[3] + ((cf.v[0] * R + cf.v[1] * G + cf.v[2] * B + 32768) >> 16));
            }
        }
        const int u = 128 + ((cf.v[4] * Rs + cf.v[5] * Gs + cf.v[6] * Bs + 131072) >> 18);
        const int v = 128 + ((cf.v[8] * Rs + cf.v[9] * Gs + cf.v[10] * Bs + 131072) >> 18);
        cb[c] = (unsigned)min(max(u, 0), 255);
        cr[c] = (unsigned)min(max(v, 0), 255);
    }
    const int cw = (W + 1) >> 1, ch = (H + 1) >> 1;
    const size_t lumaBytes = (size_t)W * H;
    unsigned char *y0 = out + (size_t)j0 * W + x0, *y1 = out + (size_t)(j0 + 1) * W + x0;
    unsigned char *c0 = out + lumaBytes + (I420 ? (size_t)jp * cw + (x0 >> 1) : (size_t)jp * 2 * cw + x0);     // Cb, or the Cb,Cr pairs
    unsigned char *c1 = c0 + (size_t)cw * ch;                                                                  // I420's Cr
    if constexpr (FAST) {
        yuv_store<BW>(y0, yb[0]);
        yuv_store<BW>(y1, yb[1]);
        if constexpr (I420) {
            yuv_store<BW / 2>(c0, cb);
            yuv_store<BW / 2>(c1, cr);
        } else {
            unsigned uv[BW];
#pragma unroll
            for (int c = 0; c < BW / 2; c++) { uv[2 * c] = cb[c]; uv[2 * c + 1] = cr[c]; }
            yuv_store<BW>(c0, uv);
        }
    } else {
        const bool row1 = j0 + 1 < H;
#pragma unroll
        for (int k = 0; k < BW; k++) {
            if (x0 + k < W) {
                y0[k] = (unsigned char)yb[0][k];
                if (row1) y1[k] = (unsigned char)yb[1][k];
            }
        }
#pragma unroll
        for (int c = 0; c < BW / 2; c++) {
            if ((x0 >> 1) + c < cw) {
                if constexpr (I420) { c0[c] = (unsigned char)cb[c]; c1[c] = (unsigned char)cr[c]; }
                else { c0[2 * c] = (unsigned char)cb[c]; c0[2 * c + 1] = (unsigned char)cr[c]; }
            }
        }
    }
}

unsigned long long rt_display_yuv_blocks(int W, int H) {
    return (unsigned long long)(((unsigned)W + RT_YUV_BW - 1u) / RT_YUV_BW) * (((unsigned)H + 1u) / 2u);
}

// srgb / tone / dExposure / invW2 as rt_launch_display_pack_toned; i420: 0 NV12, 1 I420; coef: rt_display_yuv_coeffs' twelve words
hipError_t rt_launch_display_pack_yuv(const void *image, void *out, int W, int H, int i420, int srgb, int flip, float exposure, int tone,
                                      float invW2, const void *dExposure, const int *coef, hipStream_t s) {
    const unsigned blocksPerRow = ((unsigned)W + RT_YUV_BW - 1u) / RT_YUV_BW;
    const unsigned long long nBlocks = rt_display_yuv_blocks(W, H);
    if (nBlocks > 0xffffff00ull || tone < TONE_NONE || tone > TONE_ACES) return hipErrorInvalidValue;   // (callers refuse such frames first)
    const dim3 grid((unsigned)((nBlocks + 255) / 256));
    const RtDisplayTree &tree = display_tables().tree;
    RtYuvCoef cf;
    memcpy(cf.v, coef, sizeof cf.v);
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, (const float4 *)image, (unsigned char *)out, W, H, blocksPerRow, (unsigned)nBlocks,
                           flip, exposure, (const float *)dExposure, invW2, cf, tree);
    };
    const bool fast = (W & 7) == 0 && (H & 1) == 0;
    with_tone_and_transfer(tone, srgb, [&](auto toneC, auto srgbC) {
        constexpr int T = decltype(toneC)::value;
        constexpr bool S = decltype(srgbC)::value;
        if (i420) fast ? go(rt_display_pack_yuv_kernel<S, T, true, true>) : go(rt_display_pack_yuv_kernel<S, T, true, false>);
        else fast ? go(rt_display_pack_yuv_kernel<S, T, false, true>) : go(rt_display_pack_yuv_kernel<S, T, false, false>);
    });
    return hipGetLastError();
}

// =========================================================================================
// Exposure metering (rt_meter, include/rt_mi355.h): a 256-bin histogram of log-luminance over any rgba32f surface, then the solve
// of rt_meter.h as a launch of its own behind it.  Bandwidth-bound like the pack (16 B read per pixel, nothing written but the
// 1 KiB state), and the code base's one device-wide reduction: integer atomics only, so the state is bit-identical from run to run.
// Grid sized to the chip -- RT_METER_WGS_PER_CU workgroups of 256 threads per CU, a grid-stride loop over quads of four consecutive
// pixels of the flat surface (four 16-B loads in flight per lane) -- so a frame flushes (workgroups x non-empty bins) global atomics
// however large it is.  Every wave keeps a histogram of its own in LDS (ds_add_u32, no return), filled through rt_wave_hist_add
// (rt_wave.h): coherent content (a floor, the sky) puts all 64 lanes of a wave into one or two bins, so same-bin lanes are merged by
// ballot for RT_METER_PEER rounds before the LDS atomic.  The counters and the extremes stay in registers for the whole loop and are
// reduced once per wave (rt_wave_reduce), then once per workgroup through LDS: one global atomic per workgroup and
// quantity.  minLum accumulates as the maximum of the complemented bit pattern (positive floats order like their bits), so that
// the cleared state -- zero bytes, one hipMemsetAsync in front of the kernel -- is its neutral element.
// No workgroup waits for another anywhere; the solve sees the complete histogram because it is the next launch on the stream.
// =========================================================================================
#ifndef RT_METER_WGS_PER_CU
#define RT_METER_WGS_PER_CU 2
#endif
#ifndef RT_METER_PEER
#define RT_METER_PEER 2           // aggregation rounds per pixel slot (0: every metered lane issues its own ds_add)
#endif

namespace {
// word offsets of rt_meter_state (include/rt_mi355.h pins them)
enum { MS_NPIXELS = 256, MS_NNONPOS = 257, MS_NNAN = 258, MS_NINF = 259, MS_MINLUM = 260, MS_MAXLUM = 261, MS_NMETERED = 262,
       MS_MEANLOG2 = 263, MS_TARGET = 264, MS_EXPOSURE = 265, MS_FRAMES = 266, MS_RESERVED = 267, MS_WORDS = 272 };
constexpr size_t MS_CLEAR_BYTES = MS_NMETERED * 4;      // hist, the counters, minLum / maxLum: what the histogram kernel accumulates into
}  // namespace

__global__ __launch_bounds__(256) void rt_meter_hist_kernel(const float4 *__restrict__ in, unsigned nPixels, unsigned nQuads,
                                                            unsigned *__restrict__ state) {
    __shared__ unsigned hist[4][256];                       // one histogram per wave
    __shared__ unsigned red[5];                             // nNonPositive, nNaN, nInf, max(~bits), max(bits) of the workgroup
    const unsigned tid = threadIdx.x, lane = tid & 63u;
#pragma unroll
    for (int k = 0; k < 4; k++) hist[k][tid] = 0u;
    if (tid < 5u) red[tid] = 0u;
    __syncthreads();
    unsigned *wh = hist[tid >> 6];
    unsigned cNonPos = 0u, cNaN = 0u, cInf = 0u, mnC = 0u, mx = 0u;
    const unsigned stride = gridDim.x * 256u;
    // (q - lane is the wave's first quad: the whole wave leaves the loop together, so the ballots below see every lane)
    for (unsigned q = blockIdx.x * 256u + tid; q - lane < nQuads; q += stride) {
        const unsigned first = q * 4u;                      // q < 2^29 whenever it is used
        const unsigned r = q < nQuads ? min(4u, nPixels - first) : 0u;   // pixels of this quad: 4, 1..3 at the end of the surface, 0 past it
        float4 p[4];
#pragma unroll
        for (int k = 0; k < 4; k++) p[k] = (unsigned)k < r ? in[(size_t)first + k] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool have = (unsigned)k < r;
            const float Y = rt_luma(p[k].x, p[k].y, p[k].z);
            const unsigned bits = __float_as_uint(Y);
            const bool isNaN = Y != Y, isInf = Y == __builtin_huge_valf(), pos = Y > 0.0f;
            const bool metered = have && pos && !isInf;
            cNaN += (have && isNaN) ? 1u : 0u;
            cInf += (have && isInf) ? 1u : 0u;
            cNonPos += (have && !pos && !isNaN) ? 1u : 0u;
            const int e = (int)(bits >> 20) - 888;
            const unsigned bin = (unsigned)min(max(e, 0), 255);
            mnC = max(mnC, metered ? ~bits : 0u);
            mx = max(mx, metered ? bits : 0u);
            rt_wave_hist_add<RT_METER_PEER>(wh, bin, metered, lane);
        }
    }
    // once per wave: reduce the registers across the lanes, lane 0 carries the wave's figures into the workgroup's
    const auto add = [](unsigned a, unsigned b) { return a + b; };
    const auto umax = [](unsigned a, unsigned b) { return max(a, b); };
    cNonPos = rt_wave_reduce(cNonPos, add);
    cNaN = rt_wave_reduce(cNaN, add);
    cInf = rt_wave_reduce(cInf, add);
    mnC = rt_wave_reduce(mnC, umax);
    mx = rt_wave_reduce(mx, umax);
    if (lane == 0u) {
        if (cNonPos) atomicAdd(&red[0], cNonPos);
        if (cNaN) atomicAdd(&red[1], cNaN);
        if (cInf) atomicAdd(&red[2], cInf);
        if (mnC) atomicMax(&red[3], mnC);
        if (mx) atomicMax(&red[4], mx);
    }
    __syncthreads();
    // flush: non-empty bins only, no-return integer atomics; one atomic per workgroup for each of the five other quantities
    const unsigned sum = (hist[0][tid] + hist[1][tid]) + (hist[2][tid] + hist[3][tid]);
    if (sum) atomicAdd(&state[tid], sum);
    if (tid < 3u && red[tid]) atomicAdd(&state[MS_NNONPOS + tid], red[tid]);
    if ((tid == 3u || tid == 4u) && red[tid]) atomicMax(&state[MS_MINLUM + (tid - 3u)], red[tid]);
}

struct RtMeterSolveArgs {
    RtMeterTables tab;
    float key, minExposure, maxExposure, adapt;
    int lowPermille, highPermille;
    unsigned nPixels;
};

// One workgroup, one thread per bin, rt_meter.h's pieces: a prefix sum of the bins gives every bin its first position, each thread
// adds its bin's term of S, a tree sum gives S, thread 0 finishes and writes the rest of the state.  (A single thread walking the
// 256 bins twice through LDS took about 35 us, several times the histogram kernel; measured in DESIGN.md 15.)
__global__ __launch_bounds__(256) void rt_meter_solve_kernel(unsigned *__restrict__ state, const RtMeterSolveArgs a) {
    __shared__ unsigned scan[2][256];                       // ping-pong inclusive prefix sums (n < 2^31: 32 bits hold them)
    __shared__ unsigned long long part[256];
    __shared__ unsigned lq[8];
    const unsigned b = threadIdx.x;
    const unsigned count = state[b];
    if (b < 8u) lq[b] = a.tab.log2q16[b];                   // (visible behind the scan's barriers)
    const int cur = rt_block_scan(scan, b, count);
    RtMeterSolveIn in;
    in.key = a.key; in.minExposure = a.minExposure; in.maxExposure = a.maxExposure; in.adapt = a.adapt;
    in.lowPermille = a.lowPermille; in.highPermille = a.highPermille;
    in.prevExposure = __uint_as_float(state[MS_EXPOSURE]);
    in.prevFrames = state[MS_FRAMES];
    const RtMeterTrim t = rt_meter_trim(scan[cur][255], in);
    part[b] = rt_meter_bin_term((int)b, scan[cur][b] - count, count, t, lq[b & 7u]);
    __syncthreads();
#pragma unroll
    for (unsigned d = 128u; d > 0u; d >>= 1) {
        if (b < d) part[b] += part[b + d];
        __syncthreads();
    }
    if (b != 0u) return;
    const RtMeterSolved r = rt_meter_finish(t, part[0], in, a.tab);
    const unsigned mnC = state[MS_MINLUM];                  // max(~bits) over the metered pixels; 0: there was none
    state[MS_NPIXELS] = a.nPixels;
    state[MS_MINLUM] = mnC ? ~mnC : 0x7f800000u;            // (maxLum is already its own bits, 0 when nothing was metered)
    state[MS_NMETERED] = r.nMetered;
    state[MS_MEANLOG2] = r.meanLog2Q16;
    state[MS_TARGET] = __float_as_uint(r.target);
    state[MS_EXPOSURE] = __float_as_uint(r.exposure);
    state[MS_FRAMES] = r.frames;
#pragma unroll
    for (int k = MS_RESERVED; k < MS_WORDS; k++) state[k] = 0u;
}

const RtMeterTables &rt_meter_tables_ref() {
    static const RtMeterTables tables = [] { RtMeterTables t; rt_meter_tables_host(&t); return t; }();
    return tables;
}

// Three stream operations: clear the accumulators, histogram, solve.  nPixels <= 2^31 - 1 (callers refuse larger frames first).
hipError_t rt_launch_meter(const void *image, void *state, unsigned nPixels, float key, float minExposure, float maxExposure, float adapt,
                           int lowPermille, int highPermille, hipStream_t s) {
    const unsigned nQuads = (nPixels + 3u) / 4u;
    const unsigned want = (nQuads + 255u) / 256u, cap = (unsigned)rt_cu_count() * RT_METER_WGS_PER_CU;
    hipError_t e = hipMemsetAsync(state, 0, MS_CLEAR_BYTES, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rt_meter_hist_kernel, dim3(want < cap ? want : cap), dim3(256), 0, s, (const float4 *)image, nPixels, nQuads, (unsigned *)state);
    RtMeterSolveArgs a;
    a.tab = rt_meter_tables_ref();
    a.key = key; a.minExposure = minExposure; a.maxExposure = maxExposure; a.adapt = adapt;
    a.lowPermille = lowPermille; a.highPermille = highPermille; a.nPixels = nPixels;
    hipLaunchKernelGGL(rt_meter_solve_kernel, dim3(1), dim3(256), 0, s, (unsigned *)state, a);
    return hipGetLastError();
}
