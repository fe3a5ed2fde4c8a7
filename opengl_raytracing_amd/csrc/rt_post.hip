// rt_post.hip -- post passes that consume the ray tracer's surfaces, as gfx950 HIP kernels.
// First (and so far only) one: the TAA resolve of /root/reference/shader/taaFs.glsl:13-53, driven
// like /root/reference/src/ForwardShadingPipeline.cpp:231-260.  Unlike the ray tracer this IS a
// bandwidth-bound kernel: 56 B of compulsory HBM traffic per pixel (current 16 + history 16 +
// gNormal 8 read, 16 written) against ~150 flops.
//
// Layout: 256-thread workgroup = 64x4 pixels, one lane per pixel, 16-B loads and one float4 store per
// lane.  The 3x3 neighbourhood, the jittered bilinear tap, history's 4 taps (normally collapsing onto
// one texel) and the gNormal tap(s) are served by L1/L2 (RT_TAA_LDS=1 stages the current tile + halo in
// LDS instead: measured equal).
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>

#include "rt_fastmath.h"
#include "rt_meter.h"

#ifndef RT_TAA_LDS
#define RT_TAA_LDS 0   // 1: stage the current-frame tile (+halo) in LDS; 0: neighbourhood straight from L1/L2.
#endif                // Measured equal within noise (29-31 us @1080p for every tile shape): the pass is limited by the
                      // memory pipeline, not by how the 3x3 taps are fetched; the simpler form is the default.  An XCD-aware
                      // tile order (one contiguous band of tiles per XCD, as in the bloom kernels) measured 3 % slower here.

namespace {

#ifndef RT_TAA_TX
#define RT_TAA_TX 64
#endif
constexpr int TX = RT_TAA_TX, TY = 256 / RT_TAA_TX, HALO = 1;
[[maybe_unused]] constexpr int LW = TX + 2 * HALO, LH = TY + 2 * HALO;

__device__ __forceinline__ int wrapi(int i, int n) { int r = i % n; return r < 0 ? r + n : r; }
__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

struct rgb { float x, y, z; };
__device__ __forceinline__ rgb lerp3(rgb a, rgb b, float w) {   // a + w*(b-a), per llvmpipe's float path
    rgb r; r.x = a.x + w * (b.x - a.x); r.y = a.y + w * (b.y - a.y); r.z = a.z + w * (b.z - a.z); return r;
}

}  // namespace

__global__ __launch_bounds__(256) void rt_taa_resolve_kernel(const float4 *__restrict__ current,
                                                             const float4 *__restrict__ history,
                                                             const uint2 *__restrict__ normal,   // half4 per pixel
                                                             float4 *__restrict__ out, int W, int H, float blendFactor,
                                                             float jitterX, float jitterY) {
#if RT_TAA_LDS
    __shared__ float4 tile[LH][LW];
#endif
    const int bx = blockIdx.x * TX, by = blockIdx.y * TY;
    // stage the current-frame tile; texels outside the image are stored with REPEAT addressing (what the
    // bilinear tap needs); the 3x3 clamp below substitutes 0 for them itself (texelFetch out of range)
#if RT_TAA_LDS
    for (int k = threadIdx.x; k < LW * LH; k += 256) {
        const int lx = k % LW, ly = k / LW;
        const int gx = wrapi(bx + lx - HALO, W), gy = wrapi(by + ly - HALO, H);
        tile[ly][lx] = current[(size_t)gy * W + gx];
    }
    __syncthreads();
#endif
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int i = bx + tx, j = by + ty;
    if (i >= W || j >= H) return;

    auto cur_at = [&](int x, int y) -> rgb {   // REPEAT-addressed current texel (x, y may be any integer)
        const int lx = x - bx + HALO, ly = y - by + HALO;
        float4 q;
#if RT_TAA_LDS
        if (lx >= 0 && lx < LW && ly >= 0 && ly < LH) q = tile[ly][lx];
        else
#endif
        q = current[(size_t)wrapi(y, H) * W + wrapi(x, W)];
        (void)lx; (void)ly;
        rgb r; r.x = q.x; r.y = q.y; r.z = q.z; return r;
    };

    const float u = ((float)i + 0.5f) / (float)W, v = ((float)j + 0.5f) / (float)H;   // TexCoords
    const float ju = u + jitterX, jv = v + jitterY;                                     // taaFs.glsl:23
    // current = texture(uCurrentFrame, jitteredUV): LINEAR, REPEAT                     :24
    rgb cur;
    {
        const float x = ju * (float)W - 0.5f, y = jv * (float)H - 0.5f;
        const float fx = floorf(x), fy = floorf(y);
        const float wx = x - fx, wy = y - fy;
        const int x0 = (int)fx, y0 = (int)fy;
        rgb a = lerp3(cur_at(x0, y0), cur_at(x0 + 1, y0), wx);
        rgb b = lerp3(cur_at(x0, y0 + 1), cur_at(x0 + 1, y0 + 1), wx);
        cur = lerp3(a, b, wy);
    }
    // history = texture(uHistory, TexCoords): LINEAR, CLAMP_TO_EDGE                   :27
    rgb his;
    {
        const float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
        const float fx = floorf(x), fy = floorf(y);
        const float wx = x - fx, wy = y - fy;
        const int x0 = clampi((int)fx, W), x1 = clampi((int)fx + 1, W), y0 = clampi((int)fy, H), y1 = clampi((int)fy + 1, H);
        auto h_at = [&](int xx, int yy) -> rgb { float4 q = history[(size_t)yy * W + xx]; rgb r; r.x = q.x; r.y = q.y; r.z = q.z; return r; };
        rgb a = lerp3(h_at(x0, y0), h_at(x1, y0), wx);
        rgb b = lerp3(h_at(x0, y1), h_at(x1, y1), wx);
        his = lerp3(a, b, wy);
    }
    // neighbourhood colour box, texelFetch (0 outside the image)                       :30-37
    rgb mn = cur, mx = cur;
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
            const int x = i + dx, y = j + dy;
            const bool inb = x >= 0 && y >= 0 && x < W && y < H;
#if RT_TAA_LDS
            const float4 q = tile[ty + dy + HALO][tx + dx + HALO];
#else
            const float4 q = current[(size_t)clampi(y, H) * W + clampi(x, W)];
#endif
            const float nx = inb ? q.x : 0.0f, ny = inb ? q.y : 0.0f, nz = inb ? q.z : 0.0f;
            mn.x = fminf(mn.x, nx); mn.y = fminf(mn.y, ny); mn.z = fminf(mn.z, nz);
            mx.x = fmaxf(mx.x, nx); mx.y = fmaxf(mx.y, ny); mx.z = fmaxf(mx.z, nz);
        }
    }
    // normal check, NEAREST / REPEAT                                                   :40-45
    float bf = 0.0f;
    {
        const int px = wrapi((int)floorf(u * (float)W), W), py = wrapi((int)floorf(v * (float)H), H);
        const int cx = wrapi((int)floorf(ju * (float)W), W), cy = wrapi((int)floorf(jv * (float)H), H);
        const uint2 pn = normal[(size_t)py * W + px];
        const uint2 cn = (cx == px && cy == py) ? pn : normal[(size_t)cy * W + cx];   // sub-texel jitter: same texel
        const float pnx = __half2float(__ushort_as_half((unsigned short)(pn.x & 0xffffu))), pny = __half2float(__ushort_as_half((unsigned short)(pn.x >> 16)));
        const float pnz = __half2float(__ushort_as_half((unsigned short)(pn.y & 0xffffu)));
        const float cnx = __half2float(__ushort_as_half((unsigned short)(cn.x & 0xffffu))), cny = __half2float(__ushort_as_half((unsigned short)(cn.x >> 16)));
        const float cnz = __half2float(__ushort_as_half((unsigned short)(cn.y & 0xffffu)));
        const float d = (pnz * cnz + pny * cny) + pnx * cnx;
        if (d < 0.9f) bf = blendFactor * 0.2f;
    }
    // clipAABB (:13-19) then mix(history, current, blendFactor) (:51)
    auto resolve = [&](float h, float c, float lo, float hi) -> float {
        const float center = 0.5f * (hi + lo), extents = 0.5f * (hi - lo);
        float clip = h - center;
        clip = fminf(fmaxf(clip, -extents), extents);
        const float hc = center + clip;
        return hc + bf * (c - hc);
    };
    out[(size_t)j * W + i] = make_float4(resolve(his.x, cur.x, mn.x, mx.x), resolve(his.y, cur.y, mn.y, mx.y),
                                         resolve(his.z, cur.z, mn.z, mx.z), 1.0f);
}

// The same resolve with a REGISTER WINDOW: one lane per column walks RT_TAA_ROWS consecutive rows and keeps three rows x three
// columns of `current` and of `history` in registers, so a pixel costs 6 x (ROWS + 2) / ROWS texel loads instead of 17.  The
// one-texel-per-lane kernel above is bound by the L1 pipeline rather than by HBM: its 17 loads per pixel are 288 B of L1 traffic
// against 56 B of compulsory bytes -- with the neighbourhood and bilinear loads stubbed out (timing experiment) it runs 20.3 us at
// 1080p against 28.7.  Arithmetic per pixel is the kernel above's, operation for operation; what changes is where a tap's texel
// comes from: the bilinear taps of `current` (REPEAT) are taken from the window when they fall inside it and inside the image (the
// jitter is a fraction of a texel: taaFs.glsl:23 with ForwardShadingPipeline.cpp:241-242) and loaded as before otherwise; the
// history taps (CLAMP_TO_EDGE) are window texels whenever floor(u * W - 0.5) is i - 1 or i, which fp32 guarantees for every pixel
// centre; the 3x3 box is the window itself (texelFetch: 0 outside the image).
// Measured, bit-identical (tools/bench_taa.py, same run): 1080p 28.8 -> 27.1 us, 4K 135 -> 118 us, 8K 498 -> 427 us.  Two
// further forms were written, pass the same tests and were NOT kept: each lane loading only its own column and taking the
// neighbouring columns from the adjacent lanes (DPP wave shifts), one row ahead of its use -- a quarter of the loads again, but
// 136 VGPRs / 3 waves and two loads in flight per wave: 36 / 139 / 531 us; and both surfaces staged as 64 x 8..32 pixel tiles in
// LDS (1.2 loads per pixel and surface, taps from LDS): 30 / 118 / 415 us at best.
#ifndef RT_TAA_ROWS
#define RT_TAA_ROWS 8
#endif
__global__ __launch_bounds__(256) void rt_taa_resolve_rows_kernel(const float4 *__restrict__ current, const float4 *__restrict__ history,
                                                                  const uint2 *__restrict__ normal, float4 *__restrict__ out, int W, int H,
                                                                  float blendFactor, float jitterX, float jitterY) {
    constexpr int R = RT_TAA_ROWS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + lane;
    const int j0 = (blockIdx.y * 4 + wave) * R;
    if (i >= W || j0 >= H) return;
    const int xl = clampi(i - 1, W), xr = clampi(i + 1, W);
    rgb c[3][3], h[3][3];            // [row slot][column: left, middle, right], rows / columns at CLAMPED addresses
    auto load_row = [&](int slot, int y) {
        const size_t o = (size_t)clampi(y, H) * W;
        const float4 c0 = current[o + xl], c1 = current[o + i], c2 = current[o + xr];
        const float4 h0 = history[o + xl], h1 = history[o + i], h2 = history[o + xr];
        c[slot][0] = {c0.x, c0.y, c0.z}; c[slot][1] = {c1.x, c1.y, c1.z}; c[slot][2] = {c2.x, c2.y, c2.z};
        h[slot][0] = {h0.x, h0.y, h0.z}; h[slot][1] = {h1.x, h1.y, h1.z}; h[slot][2] = {h2.x, h2.y, h2.z};
    };
    auto sel = [](bool first, rgb a, rgb b) -> rgb { rgb r; r.x = first ? a.x : b.x; r.y = first ? a.y : b.y; r.z = first ? a.z : b.z; return r; };
    load_row(0, j0 - 1);
    load_row(1, j0);
    const float u = ((float)i + 0.5f) / (float)W;
    const float ju = u + jitterX;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int j = j0 + r;
        if (j >= H) break;                                   // (wave-uniform)
        const int sa = r % 3, sm = (r + 1) % 3, sb = (r + 2) % 3;          // slots of rows j - 1, j, j + 1
        load_row(sb, j + 1);
        const float v = ((float)j + 0.5f) / (float)H;
        const float jv = v + jitterY;
        // current = texture(uCurrentFrame, jitteredUV): LINEAR, REPEAT                     :24
        rgb cur;
        {
            const float x = ju * (float)W - 0.5f, y = jv * (float)H - 0.5f;
            const float fx = floorf(x), fy = floorf(y);
            const float wx = x - fx, wy = y - fy;
            const int x0 = (int)fx, y0 = (int)fy;
            const int dx = x0 - i, dy = y0 - j;
            const bool inWin = (dx == -1 || dx == 0) && (dy == -1 || dy == 0) && x0 >= 0 && x0 + 1 < W && y0 >= 0 && y0 + 1 < H;
            const bool left = dx == -1, up = dy == -1;
            rgb t00 = sel(up, sel(left, c[sa][0], c[sa][1]), sel(left, c[sm][0], c[sm][1]));
            rgb t10 = sel(up, sel(left, c[sa][1], c[sa][2]), sel(left, c[sm][1], c[sm][2]));
            rgb t01 = sel(up, sel(left, c[sm][0], c[sm][1]), sel(left, c[sb][0], c[sb][1]));
            rgb t11 = sel(up, sel(left, c[sm][1], c[sm][2]), sel(left, c[sb][1], c[sb][2]));
            if (!inWin) {                                    // image border (REPEAT wraps around) or a jitter of a texel and more
                auto cur_at = [&](int xx, int yy) -> rgb { const float4 q = current[(size_t)wrapi(yy, H) * W + wrapi(xx, W)]; rgb t; t.x = q.x; t.y = q.y; t.z = q.z; return t; };
                t00 = cur_at(x0, y0); t10 = cur_at(x0 + 1, y0); t01 = cur_at(x0, y0 + 1); t11 = cur_at(x0 + 1, y0 + 1);
            }
            const rgb a = lerp3(t00, t10, wx), b = lerp3(t01, t11, wx);
            cur = lerp3(a, b, wy);
        }
        // history = texture(uHistory, TexCoords): LINEAR, CLAMP_TO_EDGE                   :27
        rgb his;
        {
            const float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
            const float fx = floorf(x), fy = floorf(y);
            const float wx = x - fx, wy = y - fy;
            const int dx = (int)fx - i, dy = (int)fy - j;
            const bool inWin = (dx == -1 || dx == 0) && (dy == -1 || dy == 0);
            const bool left = dx == -1, up = dy == -1;
            // clamp(i + dx) and clamp(i + dx + 1) ARE the window's clamped columns (rows alike)
            rgb t00 = sel(up, sel(left, h[sa][0], h[sa][1]), sel(left, h[sm][0], h[sm][1]));
            rgb t10 = sel(up, sel(left, h[sa][1], h[sa][2]), sel(left, h[sm][1], h[sm][2]));
            rgb t01 = sel(up, sel(left, h[sm][0], h[sm][1]), sel(left, h[sb][0], h[sb][1]));
            rgb t11 = sel(up, sel(left, h[sm][1], h[sm][2]), sel(left, h[sb][1], h[sb][2]));
            if (!inWin) {
                const int x0 = clampi((int)fx, W), x1 = clampi((int)fx + 1, W), y0 = clampi((int)fy, H), y1 = clampi((int)fy + 1, H);
                auto h_at = [&](int xx, int yy) -> rgb { const float4 q = history[(size_t)yy * W + xx]; rgb t; t.x = q.x; t.y = q.y; t.z = q.z; return t; };
                t00 = h_at(x0, y0); t10 = h_at(x1, y0); t01 = h_at(x0, y1); t11 = h_at(x1, y1);
            }
            const rgb a = lerp3(t00, t10, wx), b = lerp3(t01, t11, wx);
            his = lerp3(a, b, wy);
        }
        // neighbourhood colour box, texelFetch (0 outside the image)                       :30-37
        rgb mn = cur, mx = cur;
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
#pragma unroll
            for (int dy = -1; dy <= 1; dy++) {
                const int x = i + dx, y = j + dy;
                const bool inb = x >= 0 && y >= 0 && x < W && y < H;
                const rgb q = c[dy < 0 ? sa : (dy == 0 ? sm : sb)][dx + 1];
                const float nx = inb ? q.x : 0.0f, ny = inb ? q.y : 0.0f, nz = inb ? q.z : 0.0f;
                mn.x = fminf(mn.x, nx); mn.y = fminf(mn.y, ny); mn.z = fminf(mn.z, nz);
                mx.x = fmaxf(mx.x, nx); mx.y = fmaxf(mx.y, ny); mx.z = fmaxf(mx.z, nz);
            }
        }
        // normal check, NEAREST / REPEAT                                                   :40-45
        float bf = 0.0f;
        {
            const int px = wrapi((int)floorf(u * (float)W), W), py = wrapi((int)floorf(v * (float)H), H);
            const int cx = wrapi((int)floorf(ju * (float)W), W), cy = wrapi((int)floorf(jv * (float)H), H);
            const uint2 pn = normal[(size_t)py * W + px];
            const uint2 cn = (cx == px && cy == py) ? pn : normal[(size_t)cy * W + cx];   // sub-texel jitter: same texel
            const float pnx = __half2float(__ushort_as_half((unsigned short)(pn.x & 0xffffu))), pny = __half2float(__ushort_as_half((unsigned short)(pn.x >> 16)));
            const float pnz = __half2float(__ushort_as_half((unsigned short)(pn.y & 0xffffu)));
            const float cnx = __half2float(__ushort_as_half((unsigned short)(cn.x & 0xffffu))), cny = __half2float(__ushort_as_half((unsigned short)(cn.x >> 16)));
            const float cnz = __half2float(__ushort_as_half((unsigned short)(cn.y & 0xffffu)));
            const float d = (pnz * cnz + pny * cny) + pnx * cnx;
            if (d < 0.9f) bf = blendFactor * 0.2f;
        }
        // clipAABB (:13-19) then mix(history, current, blendFactor) (:51)
        auto resolve = [&](float hh, float cc, float lo, float hi) -> float {
            const float center = 0.5f * (hi + lo), extents = 0.5f * (hi - lo);
            float clip = hh - center;
            clip = fminf(fmaxf(clip, -extents), extents);
            const float hc = center + clip;
            return hc + bf * (cc - hc);
        };
        out[(size_t)j * W + i] = make_float4(resolve(his.x, cur.x, mn.x, mx.x), resolve(his.y, cur.y, mn.y, mx.y),
                                             resolve(his.z, cur.z, mn.z, mx.z), 1.0f);
    }
}

#ifndef RT_TAA_WINDOW
#define RT_TAA_WINDOW 1         // 0: the one-texel-per-lane kernel for every launch
#endif
hipError_t rt_launch_taa_resolve(const void *current, const void *history, const void *normal, void *out, int W, int H,
                                 float blend, float jx, float jy, hipStream_t s) {
    // (`out` must not alias the inputs in either form; frames of a few rows keep the one-texel-per-lane kernel)
    if (RT_TAA_WINDOW && H >= 4 * RT_TAA_ROWS) {
        dim3 grid((W + 63) / 64, (H + 4 * RT_TAA_ROWS - 1) / (4 * RT_TAA_ROWS));
        hipLaunchKernelGGL(rt_taa_resolve_rows_kernel, grid, dim3(256), 0, s, (const float4 *)current, (const float4 *)history,
                           (const uint2 *)normal, (float4 *)out, W, H, blend, jx, jy);
        return hipGetLastError();
    }
    dim3 grid((W + TX - 1) / TX, (H + TY - 1) / TY);
    hipLaunchKernelGGL(rt_taa_resolve_kernel, grid, dim3(256), 0, s, (const float4 *)current, (const float4 *)history,
                       (const uint2 *)normal, (float4 *)out, W, H, blend, jx, jy);
    return hipGetLastError();
}

// =========================================================================================
// Bloom: brightness_extractFS.glsl, gaussian_blurFs.glsl, bloom_combineFs.glsl as
// driven by /root/reference/src/ForwardShadingPipeline.cpp:189-228.  Intermediate targets are rgba16f
// (:67-88) and the reference's GL rounds render-target writes toward zero, so every pass stores
// RTZ halfs; all taps sit on texel centres (LINEAR returns the texel), CLAMP_TO_EDGE at the borders.
// The chain runs as fused horizontal+vertical pairs (rt_bloom_hv_kernel, below); the single-pass kernels
// remain for odd / zero iteration counts.
// =========================================================================================
namespace {

// fp32 -> fp16 toward zero in hardware: v_cvt_pkrtz_f16_f32 is IEEE round-toward-zero (overflow saturates to
// +-65504, fp16 denormals kept -- the kernel runs with the default f16 denormal mode), i.e. the same function
// as the oracle's software orc_float_to_half_rtz on every non-NaN input; NaNs stay NaNs (payload not compared).
typedef __fp16 rt_h2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned cvt_pkrtz_u(float lo, float hi) {
    union { rt_h2v h; unsigned u; } c;
    c.h = __builtin_amdgcn_cvt_pkrtz(lo, hi);
    return c.u;
}
__device__ __forceinline__ float h2f_u(unsigned h) { return __half2float(__ushort_as_half((unsigned short)(h & 0xffffu))); }
__device__ __forceinline__ uint2 pack_half4(float r, float g, float b) {
    return make_uint2(cvt_pkrtz_u(r, g), cvt_pkrtz_u(b, 1.0f));
}

}  // namespace

// brightness extract (brightness_extractFS.glsl:11-19)
__global__ __launch_bounds__(256) void rt_bloom_extract_kernel(const float4 *__restrict__ scene, uint2 *__restrict__ out,
                                                               size_t n, float threshold) {
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (size_t)gridDim.x * 256) {
        const float4 c = scene[k];
        const float brightness = (c.z * 0.0722f + c.y * 0.7152f) + c.x * 0.2126f;
        out[k] = (brightness > threshold) ? pack_half4(c.x, c.y, c.z) : make_uint2(0u, 0x3c00u << 16);
    }
}

// one separable 9-tap pass (gaussian_blurFs.glsl:8-26)
template <bool HORIZONTAL>
__global__ __launch_bounds__(256) void rt_bloom_blur_kernel(const uint2 *__restrict__ in, uint2 *__restrict__ out, int W, int H) {
    const float w0 = 0.227027f, w1 = 0.1945946f, w2 = 0.1216216f, w3 = 0.054054f, w4 = 0.016216f;
    const int i = blockIdx.x * 64 + (threadIdx.x & 63), j = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= W || j >= H) return;
    auto tap = [&](int t) -> uint2 {
        const int x = HORIZONTAL ? min(max(i + t, 0), W - 1) : i, y = HORIZONTAL ? j : min(max(j + t, 0), H - 1);
        return in[(size_t)y * W + x];
    };
    const uint2 c = tap(0);
    float r = h2f_u(c.x) * w0, g = h2f_u(c.x >> 16) * w0, b = h2f_u(c.y) * w0;
    auto acc = [&](int t, float w) {
        const uint2 p = tap(t), m = tap(-t);
        r += h2f_u(p.x) * w; g += h2f_u(p.x >> 16) * w; b += h2f_u(p.y) * w;      // result += tex(+i)*w
        r += h2f_u(m.x) * w; g += h2f_u(m.x >> 16) * w; b += h2f_u(m.y) * w;      // result += tex(-i)*w
    };
    acc(1, w1); acc(2, w2); acc(3, w3); acc(4, w4);
    out[(size_t)j * W + i] = pack_half4(r, g, b);
}

// combine (bloom_combineFs.glsl:10-14)
__global__ __launch_bounds__(256) void rt_bloom_combine_kernel(const float4 *__restrict__ scene, const uint2 *__restrict__ bloom,
                                                               float4 *__restrict__ out, size_t n, float strength) {
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (size_t)gridDim.x * 256) {
        const float4 s = scene[k];
        const uint2 bl = bloom[k];
        out[k] = make_float4(s.x + h2f_u(bl.x) * strength, s.y + h2f_u(bl.x >> 16) * strength, s.z + h2f_u(bl.y) * strength, 1.0f);
    }
}

// Fused horizontal+vertical pass pair (one blur "iteration pair" of ForwardShadingPipeline.cpp:207-216):
// a 64x24-pixel workgroup tile stages its 72x32 input patch (4-texel apron each way, CLAMP_TO_EDGE applied
// while staging, in image space) in LDS as halfs, runs the horizontal pass into a second LDS array --
// rounded to fp16 toward zero exactly where the unfused chain stores its rgba16f target -- then the
// vertical pass from LDS.  Both passes use register sliding windows: a lane owns 4 consecutive outputs
// along the blur axis (3 for the vertical pass) on each of two lines, so it reads 3 (3.7) texels per output
// instead of 9, and the two lines share packed-fp32 arithmetic.  Lane->row mapping with odd-ish row strides (73 / 65 texels) keeps the
// ds_read_b64 / ds_write_b64 of 16 consecutive lanes on distinct banks.
// FIRST folds the brightness extract into the staging (reads the rgba32f scene), LAST folds the combine
// into the store (writes rgba32f).  HBM traffic per pair: 8 B in + 8 B out per pixel (+ apron re-reads
// served by L2) instead of 32 B for two unfused passes.
namespace {
constexpr int FX = 64, FY = 24, AP = 4, IW = FX + 2 * AP, IH = FY + 2 * AP;   // 72 x 32 patch
constexpr int IWP = IW + 1, FXP = FX + 1;                                     // padded LDS row strides
constexpr int HSPAN = 4, VSPAN = 3;                                           // outputs per lane and per half of the pair
static_assert((IH / 2) * (FX / HSPAN) == 256 && (FX / 2) * (FY / VSPAN) == 256, "one work item per thread in both passes");
typedef float rt_f2 __attribute__((ext_vector_type(2)));
}

// One 9-tap window on TWO independent lines at once (.x / .y): every multiply and add is a packed fp32
// instruction (v_pk_mul_f32 / v_pk_add_f32: IEEE, no contraction), which halves the VALU work this
// VALU-bound kernel issues; the order of operations per line is the reference's.
template <int N>
__device__ __forceinline__ void blur_window2(const rt_f2 (&r)[N + 8], const rt_f2 (&g)[N + 8], const rt_f2 (&b)[N + 8], int k,
                                             rt_f2 &orr, rt_f2 &og, rt_f2 &ob) {
    const float w[5] = {0.227027f, 0.1945946f, 0.1216216f, 0.054054f, 0.016216f};
    const int c = k + 4;
    rt_f2 ar = r[c] * w[0], ag = g[c] * w[0], ab = b[c] * w[0];  // gaussian_blurFs.glsl:13
#pragma unroll
    for (int t = 1; t < 5; t++) {                                 // :15-24: result += tex(+t)*w; result += tex(-t)*w
        ar += r[c + t] * w[t]; ag += g[c + t] * w[t]; ab += b[c + t] * w[t];
        ar += r[c - t] * w[t]; ag += g[c - t] * w[t]; ab += b[c - t] * w[t];
    }
    orr = ar; og = ag; ob = ab;
}

#ifndef RT_BLOOM_XCD
#define RT_BLOOM_XCD 1      // XCD-aware tile order of the fused kernels (needs RT_BLOOM_TPW == 1)
#endif
#ifndef RT_BLOOM_TPW
#define RT_BLOOM_TPW 1      // tiles per workgroup of the fused kernels (see rt_bloom_hv_kernel)
#endif
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void rt_bloom_hv_kernel(const void *__restrict__ inV, const float4 *__restrict__ scene,
                                                          void *__restrict__ outV, int W, int H, float threshold, float strength) {
    // one LDS array, used twice: the input patch (halfs; patch (r,c) <-> image (clamp(y0+r-4), clamp(x0+c-4))),
    // then -- once every lane holds its window in registers -- the horizontal-pass result (halfs, RTZ) for
    // patch rows 0..IH-1, tile columns 0..FX-1.  18.7 KB per workgroup: 8 workgroups (32 waves) per CU.
    __shared__ uint2 sin_[IH * IWP];
    uint2 *sh_ = sin_;
    // The patch is REQUESTED as one batch of NLD independent loads per thread into registers and written to LDS afterwards
    // (round 1 interleaved load -> ds_write per texel, which serialised the memory latency: 88 -> 72 us for the 1080p chain,
    // 249 -> 226 us at 4K).  The tile loop also lets a workgroup walk several tiles with the next patch in flight during
    // the two passes (RT_BLOOM_TPW tiles per workgroup): measured SLOWER -- 72 / 79 / 81 / 96 / 104 us at 1, 2, 3, 4, 6
    // tiles per workgroup at 1080p -- the 1 350 one-tile workgroups are all co-resident and cover each other's phases
    // better than fewer, longer-lived ones; the default stays one tile per workgroup.
    const int tilesX = (W + FX - 1) / FX, nTiles = tilesX * ((H + FY - 1) / FY);
    constexpr int NLD = (IW * IH) / 256;                               // patch texels per thread (9)
    static_assert(NLD * 256 == IW * IH, "whole patch in NLD loads per thread");
    float4 preF[FIRST ? NLD : 1];                                      // FIRST: the rgba32f scene texel (extract happens at the LDS write)
    uint2 preH[FIRST ? 1 : NLD];
    auto request = [&](int tile) {
        const int x0 = (tile % tilesX) * FX, y0 = (tile / tilesX) * FY;
#pragma unroll
        for (int j = 0; j < NLD; j++) {
            const int k = threadIdx.x + j * 256;
            const int lx = k % IW, ly = k / IW;
            const int gx = min(max(x0 + lx - AP, 0), W - 1), gy = min(max(y0 + ly - AP, 0), H - 1);
            if (FIRST) preF[j] = scene[(size_t)gy * W + gx];
            else preH[j] = ((const uint2 *)inV)[(size_t)gy * W + gx];
        }
    };
#if RT_BLOOM_XCD
    // workgroups go to the 8 XCDs round-robin by id: give each XCD one contiguous band of tiles, so that the aprons a tile shares
    // with its neighbours are served by the SAME L2 instead of being fetched from HBM once per XCD
    int tile = (int)(blockIdx.x & 7u) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
#else
    int tile = blockIdx.x;
#endif
    if (tile < nTiles) request(tile);
    for (; tile < nTiles; tile += (RT_BLOOM_TPW == 1 ? nTiles : (int)gridDim.x)) {      // (one trip when RT_BLOOM_TPW == 1)
    const int x0 = (tile % tilesX) * FX, y0 = (tile / tilesX) * FY;
    // ---- the requested patch -> LDS
#pragma unroll
    for (int j = 0; j < NLD; j++) {
        const int k = threadIdx.x + j * 256;
        uint2 v;
        if (FIRST) {     // brightness_extractFS.glsl:11-19 on the fly
            const float4 c = preF[j];
            const float brightness = (c.z * 0.0722f + c.y * 0.7152f) + c.x * 0.2126f;
            v = (brightness > threshold) ? pack_half4(c.x, c.y, c.z) : make_uint2(0u, 0x3c00u << 16);
        } else {
            v = preH[j];
        }
        sin_[(k / IW) * IWP + (k % IW)] = v;
    }
    __syncthreads();
    if (RT_BLOOM_TPW > 1 && tile + (int)gridDim.x < nTiles) request(tile + (int)gridDim.x);     // in flight during the two passes below
    {   // ---- horizontal pass: lane -> patch rows (rp, rp+16), 4 consecutive columns of each
        const int rp = threadIdx.x % (IH / 2), grp = threadIdx.x / (IH / 2);
        rt_f2 r[HSPAN + 8], g[HSPAN + 8], b[HSPAN + 8];
#pragma unroll
        for (int c = 0; c < HSPAN + 8; c++) {
            const uint2 v0 = sin_[rp * IWP + grp * HSPAN + c], v1 = sin_[(rp + IH / 2) * IWP + grp * HSPAN + c];
            r[c].x = h2f_u(v0.x); g[c].x = h2f_u(v0.x >> 16); b[c].x = h2f_u(v0.y);
            r[c].y = h2f_u(v1.x); g[c].y = h2f_u(v1.x >> 16); b[c].y = h2f_u(v1.y);
        }
        __syncthreads();     // every window is in registers: the patch storage may be overwritten
#pragma unroll
        for (int k = 0; k < HSPAN; k++) {
            rt_f2 orr, og, ob;
            blur_window2<HSPAN>(r, g, b, k, orr, og, ob);
            sh_[rp * FXP + grp * HSPAN + k] = pack_half4(orr.x, og.x, ob.x);
            sh_[(rp + IH / 2) * FXP + grp * HSPAN + k] = pack_half4(orr.y, og.y, ob.y);
        }
    }
    __syncthreads();
    {   // ---- vertical pass: lane -> columns (lx, lx+32), 3 consecutive rows of each
        const int lx = threadIdx.x % (FX / 2), seg = threadIdx.x / (FX / 2);
        rt_f2 r[VSPAN + 8], g[VSPAN + 8], b[VSPAN + 8];
#pragma unroll
        for (int c = 0; c < VSPAN + 8; c++) {
            const uint2 v0 = sh_[(seg * VSPAN + c) * FXP + lx], v1 = sh_[(seg * VSPAN + c) * FXP + lx + FX / 2];
            r[c].x = h2f_u(v0.x); g[c].x = h2f_u(v0.x >> 16); b[c].x = h2f_u(v0.y);
            r[c].y = h2f_u(v1.x); g[c].y = h2f_u(v1.x >> 16); b[c].y = h2f_u(v1.y);
        }
        __syncthreads();     // the horizontal result is in registers: the next tile's patch may overwrite the LDS array
#pragma unroll
        for (int k = 0; k < VSPAN; k++) {
            const int y = y0 + seg * VSPAN + k;
            if (y >= H) continue;
            rt_f2 orr, og, ob;
            blur_window2<VSPAN>(r, g, b, k, orr, og, ob);
#pragma unroll
            for (int half = 0; half < 2; half++) {
                const int x = x0 + lx + half * (FX / 2);
                if (x >= W) continue;
                const uint2 hv = half ? pack_half4(orr.y, og.y, ob.y) : pack_half4(orr.x, og.x, ob.x);   // the rgba16f store
                if (LAST) {      // bloom_combineFs.glsl:10-14
                    const float4 sc = scene[(size_t)y * W + x];
                    ((float4 *)outV)[(size_t)y * W + x] = make_float4(sc.x + h2f_u(hv.x) * strength, sc.y + h2f_u(hv.x >> 16) * strength,
                                                                      sc.z + h2f_u(hv.y) * strength, 1.0f);
                } else {
                    ((uint2 *)outV)[(size_t)y * W + x] = hv;
                }
            }
        }
    }
    }   // tiles of this workgroup
}

hipError_t rt_launch_bloom(const void *scene, void *tmpA, void *tmpB, void *out, int W, int H, float threshold, float strength,
                           int iterations, hipStream_t s) {
    const size_t n = (size_t)W * H;
    int blocks = (int)((n + 255) / 256);
    if (blocks > 256 * 16) blocks = 256 * 16;
    uint2 *a = (uint2 *)tmpA, *b = (uint2 *)tmpB;
    const float4 *sc = (const float4 *)scene;
    const int pairs = iterations / 2;
    const bool odd = (iterations & 1) != 0;
    const int nTilesF = ((W + FX - 1) / FX) * ((H + FY - 1) / FY);
    dim3 fgrid(RT_BLOOM_XCD ? ((nTilesF + 7) / 8) * 8 : (nTilesF + RT_BLOOM_TPW - 1) / RT_BLOOM_TPW), grid((W + 63) / 64, (H + 3) / 4);
    if (pairs == 0) {            // 0 or 1 iterations: the unfused kernels
        hipLaunchKernelGGL(rt_bloom_extract_kernel, dim3(blocks), dim3(256), 0, s, sc, a, n, threshold);
        if (odd) { hipLaunchKernelGGL(rt_bloom_blur_kernel<true>, grid, dim3(256), 0, s, a, b, W, H); a = b; }
        hipLaunchKernelGGL(rt_bloom_combine_kernel, dim3(blocks), dim3(256), 0, s, sc, a, (float4 *)out, n, strength);
        return hipGetLastError();
    }
    for (int p = 0; p < pairs; p++) {
        const bool first = p == 0, last = (p == pairs - 1) && !odd;
        void *dst = last ? out : (void *)b;
        if (first && last) hipLaunchKernelGGL((rt_bloom_hv_kernel<true, true>), fgrid, dim3(256), 0, s, (const void *)a, sc, dst, W, H, threshold, strength);
        else if (first) hipLaunchKernelGGL((rt_bloom_hv_kernel<true, false>), fgrid, dim3(256), 0, s, (const void *)a, sc, dst, W, H, threshold, strength);
        else if (last) hipLaunchKernelGGL((rt_bloom_hv_kernel<false, true>), fgrid, dim3(256), 0, s, (const void *)a, sc, dst, W, H, threshold, strength);
        else hipLaunchKernelGGL((rt_bloom_hv_kernel<false, false>), fgrid, dim3(256), 0, s, (const void *)a, sc, dst, W, H, threshold, strength);
        if (!last) { uint2 *t = a; a = b; b = t; }
    }
    if (odd) {                   // trailing horizontal pass, then the combine
        hipLaunchKernelGGL(rt_bloom_blur_kernel<true>, grid, dim3(256), 0, s, a, b, W, H);
        hipLaunchKernelGGL(rt_bloom_combine_kernel, dim3(blocks), dim3(256), 0, s, sc, b, (float4 *)out, n, strength);
    }
    return hipGetLastError();
}

// =========================================================================================
// SSAO: ssaoFs.glsl:16-46 + ssao_blurFs.glsl:11-29 as driven by
// /root/reference/src/AO.cpp:86-117.  G-buffer consumer: gPosition (rgba32f) and gNormal (rgba16f) as the ray
// kernel wrote them, NEAREST with the default REPEAT wrap (ForwardShadingPipeline.cpp:115-126).  Same fp32
// expression shapes as oracle/rt_post_oracle.c::orc_ssao (pinned bit for bit to the shader on llvmpipe).
// MI355X mapping: the 64 kernel samples, both matrices and the 4x4 rotation texture are kernel arguments
// (1.2 KB): wave-uniform, so they arrive as SGPR operands by s_load; a wave owns an 8x8 pixel tile so its
// 64 x 64 depth gathers (4 B out of every 16 B texel) stay in a few L1/L2 lines.
// =========================================================================================
#ifndef RT_SSAO_UNROLL
#define RT_SSAO_UNROLL 8
#endif
#ifndef RT_SSAO_XCD
#define RT_SSAO_XCD 0             // 1: one contiguous image band per XCD.  Measured neutral at 1080p (387 vs 386 us) and
#endif                            // 1.5 % slower at 4K: the kernel is VALU-bound, not L2-bound; kept as a switch.
#ifndef RT_SSAO_TILE_W
#define RT_SSAO_TILE_W 8          // wave tile width in pixels (height = 64 / width)
#endif
struct RtSsaoArgs {
    float samples[64][3];
    float projection[16], view[16];
    float noise[16][4];
    int nW, nH, W, H;
};

namespace {
__device__ __forceinline__ int ssao_nearest_repeat(float u, int size) {
    if ((size & (size - 1)) == 0) return ((int)floorf(u * (float)size)) & (size - 1);
    float fr = u - floorf(u);
    if (!(fr < 1.0f)) fr = 0.99999994f;
    if (!(fr >= 0.0f)) fr = 0.0f;
    return (int)(fr * (float)size);
}
__device__ __forceinline__ void ssao_nrm3(float x, float y, float z, float &ox, float &oy, float &oz) {
    const float d = (z * z + y * y) + x * x;
    const float r = 1.0f / sqrtf(d);
    ox = x * r; oy = y * r; oz = z * r;
}
}  // namespace

// gPosition.z as a dense plane: the 64 depth gathers per pixel then touch 4x fewer cache lines
__global__ __launch_bounds__(256) void rt_ssao_depth_kernel(const float4 *__restrict__ position, float *__restrict__ depth, size_t n) {
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (size_t)gridDim.x * 256) depth[k] = position[k].z;
}

#ifndef RT_SSAO_FASTDIV
#define RT_SSAO_FASTDIV 1       // 0 = the compiler's IEEE divisions in the sample loop
#endif

// ssaoFs.glsl:27-44, the 64 kernel samples of one pixel.  FAST: divisions by rt_fastmath.h's fast paths; returns NaN when
// any of them left its exact range (the caller then takes the IEEE instantiation).  The true sum is never NaN-free-checked:
// a genuine NaN (NaN G-buffer) also sends the wave through the IEEE loop, which reproduces it.
template <bool FAST>
__device__ __forceinline__ float ssao_samples(const RtSsaoArgs &a, const float *__restrict__ depth, const float4 fp, float nx, float ny, float nz,
                                              float tx, float ty, float tz, float bx, float by, float bz, int W, int H) {
    float occlusion = 0.0f;
    bool bad = false;
    const float *V = a.view, *P = a.projection;
#pragma unroll RT_SSAO_UNROLL
    for (int k = 0; k < 64; k++) {
        const float s0 = a.samples[k][0], s1 = a.samples[k][1], s2 = a.samples[k][2];
        float px = (tx * s0 + bx * s1) + nx * s2, py = (ty * s0 + by * s1) + ny * s2, pz = (tz * s0 + bz * s1) + nz * s2;
        px = fp.x + px * 0.5f; py = fp.y + py * 0.5f; pz = fp.z + pz * 0.5f;
        float vw[4], of[4];
#pragma unroll
        for (int r = 0; r < 4; r++) vw[r] = ((V[r] * px + V[4 + r] * py) + V[8 + r] * pz) + V[12 + r] * 1.0f;
#pragma unroll
        for (int r = 0; r < 4; r++) of[r] = ((P[r] * vw[0] + P[4 + r] * vw[1]) + P[8 + r] * vw[2]) + P[12 + r] * vw[3];
        float ox, oy;
        if constexpr (FAST) {           // offset.xy / offset.w: one refined reciprocal, two Markstein corrections
            bool oky, ok0, ok1;
            const float y = rtf::rcp_fast(of[3], oky);
            ox = rtf::div_fast(of[0], of[3], y, ok0);
            oy = rtf::div_fast(of[1], of[3], y, ok1);
            bad |= !(oky & ok0 & ok1);
        } else {
            ox = of[0] / of[3]; oy = of[1] / of[3];
        }
        ox = ox * 0.5f + 0.5f;
        oy = oy * 0.5f + 0.5f;
        const float sampleDepth = depth[(size_t)ssao_nearest_repeat(oy, H) * W + ssao_nearest_repeat(ox, W)];
        const float adz = fabsf(fp.z - sampleDepth);
        float x;
        if constexpr (FAST) {           // 0.5 / |dz| = RN(1 / |dz|) * 0.5: the halving is exact while reciprocal and product are normal
            bool okr;
            x = rtf::rcp_fast(adz, okr) * 0.5f;
            const bool zero = adz == 0.0f;        // equal depths (flat regions, the pixel itself): 0.5 / 0 = +inf, no reason to leave the fast loop
            x = zero ? __builtin_huge_valf() : x;
            bad |= !((okr & (adz <= 0x1p125f)) | zero);
        } else {
            x = 0.5f / adz;
        }
        const float tt = fminf(fmaxf(x, 0.0f), 1.0f);
        const float rangeCheck = tt * (tt * (3.0f - 2.0f * tt));
        occlusion += (sampleDepth >= pz + 0.025f ? 1.0f : 0.0f) * rangeCheck;
    }
    return (FAST && bad) ? __builtin_nanf("") : occlusion;
}

__global__ __launch_bounds__(256) void rt_ssao_kernel(const float4 *__restrict__ position, const uint2 *__restrict__ normal,
                                                      const float *__restrict__ depth, float *__restrict__ out, const RtSsaoArgs a) {
    // 256 threads = 4 waves, each an 8x8 tile of a 32x8 block
    constexpr int TW = RT_SSAO_TILE_W, TH = 64 / TW;
    const int wave = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int W = a.W, H = a.H;
    // XCD-aware block -> tile map: workgroup b runs on XCD b % 8, so give each XCD one contiguous band of the image
    // (its 4 MB L2 then holds the band's depth neighbourhood instead of 1/8 of every neighbourhood of the frame)
    const int nbx = (W + 4 * TW - 1) / (4 * TW);
#if RT_SSAO_XCD
    const unsigned nb = gridDim.x, per = (nb + 7u) / 8u;
    const unsigned lb = (blockIdx.x % 8u) * per + blockIdx.x / 8u;
    if (lb >= nb) return;            // nb not a multiple of 8: the map below covers [0, nb) exactly once (see launch)
#else
    const unsigned lb = blockIdx.x;
#endif
    const int blkX = (int)(lb % (unsigned)nbx), blkY = (int)(lb / (unsigned)nbx);
    const int i = blkX * (4 * TW) + wave * TW + (ln % TW), j = blkY * TH + (ln / TW);
    if (i >= W || j >= H) return;
    const float u = ((float)i + 0.5f) / (float)W, v = ((float)j + 0.5f) / (float)H;
    const size_t self = (size_t)ssao_nearest_repeat(v, H) * W + ssao_nearest_repeat(u, W);
    const float4 fp = position[self];
    const uint2 nh = normal[self];
    float nx, ny, nz, rx, ry, rz;
    ssao_nrm3(h2f_u(nh.x), h2f_u(nh.x >> 16), h2f_u(nh.y), nx, ny, nz);
    const float nu = u * 200.0f, nv = v * 200.0f;                                       // ssaoFs.glsl:14,20
    const int nt = ssao_nearest_repeat(nv, a.nH) * a.nW + ssao_nearest_repeat(nu, a.nW);
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
#pragma unroll
    for (int k = 0; k < 16; k++)       // per-lane pick from the SGPR-resident texture (<= 16 texels)
        if (k == nt) { qx = a.noise[k][0]; qy = a.noise[k][1]; qz = a.noise[k][2]; }
    ssao_nrm3(qx, qy, qz, rx, ry, rz);
    const float d = (rz * nz + ry * ny) + rx * nx;
    float tx, ty, tz;
    ssao_nrm3(rx - nx * d, ry - ny * d, rz - nz * d, tx, ty, tz);
    const float bx = ny * tz - ty * nz, by = nz * tx - tz * nx, bz = nx * ty - tx * ny;
    // The three divisions per sample (offset.xy / offset.w, 0.5 / |dz|) without the compiler's 11-instruction IEEE sequences
    // (rt_fastmath.h: correctly rounded for operands in the ordinary exponent range, each with an `ok` flag).  The sample loop
    // stays BRANCH-FREE -- a wave-uniform fallback branch per sample keeps the unrolled iterations' depth gathers from
    // overlapping (measured: 398 -> 449 us @1080p with it, i.e. slower than the IEEE divisions) -- so the flags are only
    // OR-ed, and a wave in which any lane's any sample left the fast range redoes its 64 samples with the IEEE divisions.
    // (a wave holding a pixel without geometry -- zero normal, NaN basis: the sky -- goes to the IEEE loop directly)
    const float chk = ((tx + ty) + tz) + ((bx + by) + bz) + ((fp.x + fp.y) + fp.z);
    float occlusion;
    if (RT_SSAO_FASTDIV != 0 && __builtin_amdgcn_ballot_w64(!(fabsf(chk) < __builtin_huge_valf())) == 0ull) {
        occlusion = ssao_samples<true>(a, depth, fp, nx, ny, nz, tx, ty, tz, bx, by, bz, W, H);
        if (__builtin_amdgcn_ballot_w64(occlusion != occlusion) != 0ull)
            occlusion = ssao_samples<false>(a, depth, fp, nx, ny, nz, tx, ty, tz, bx, by, bz, W, H);
    } else {
        occlusion = ssao_samples<false>(a, depth, fp, nx, ny, nz, tx, ty, tz, bx, by, bz, W, H);
    }
    out[(size_t)j * W + i] = 1.0f - occlusion / 64.0f;
}

template <bool HORIZONTAL>
__global__ __launch_bounds__(256) void rt_ssao_blur_kernel(const float *__restrict__ in, float *__restrict__ out, int W, int H) {
    const float wgt[5] = {0.227027f, 0.1945946f, 0.1216216f, 0.054054f, 0.016216f};
    const int i = blockIdx.x * 64 + (threadIdx.x & 63), j = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= W || j >= H) return;
    const float u = ((float)i + 0.5f) / (float)W, v = ((float)j + 0.5f) / (float)H;
    const float tx = 1.0f / (float)W, ty = 1.0f / (float)H;
    float r = in[(size_t)ssao_nearest_repeat(v, H) * W + ssao_nearest_repeat(u, W)] * wgt[0];
#pragma unroll
    for (int k = 1; k < 5; k++) {
        const float du = HORIZONTAL ? tx * (float)k : 0.0f, dv = HORIZONTAL ? 0.0f : ty * (float)k;
        r += in[(size_t)ssao_nearest_repeat(v + dv, H) * W + ssao_nearest_repeat(u + du, W)] * wgt[k];
        r += in[(size_t)ssao_nearest_repeat(v - dv, H) * W + ssao_nearest_repeat(u - du, W)] * wgt[k];
    }
    out[(size_t)j * W + i] = r;
}

hipError_t rt_launch_ssao(const void *position, const void *normal, void *depthPlane, void *out, int W, int H, const float *noise,
                          int nW, int nH, const float *samples, const float *projection, const float *view, hipStream_t s) {
    RtSsaoArgs a;
    memset(&a, 0, sizeof a);
    memcpy(a.samples, samples, sizeof a.samples);
    memcpy(a.projection, projection, sizeof a.projection);
    memcpy(a.view, view, sizeof a.view);
    memcpy(a.noise, noise, (size_t)nW * nH * 4 * sizeof(float));
    a.nW = nW; a.nH = nH; a.W = W; a.H = H;
    constexpr int TW = RT_SSAO_TILE_W, TH = 64 / TW;
    unsigned nBlocks = (unsigned)(((W + 4 * TW - 1) / (4 * TW)) * ((H + TH - 1) / TH));
#if RT_SSAO_XCD
    nBlocks = (nBlocks + 7u) / 8u * 8u;      // whole groups of 8 so that b -> (b % 8) * per + b / 8 is a bijection
#endif
    dim3 grid(nBlocks);
    const size_t n = (size_t)W * H;
    size_t blocks = (n + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(rt_ssao_depth_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const float4 *)position, (float *)depthPlane, n);
    hipLaunchKernelGGL(rt_ssao_kernel, grid, dim3(256), 0, s, (const float4 *)position, (const uint2 *)normal,
                       (const float *)depthPlane, (float *)out, a);
    return hipGetLastError();
}

hipError_t rt_launch_ssao_blur(const void *in, void *out, int W, int H, int horizontal, hipStream_t s) {
    dim3 grid((W + 63) / 64, (H + 3) / 4);
    if (horizontal) hipLaunchKernelGGL(rt_ssao_blur_kernel<true>, grid, dim3(256), 0, s, (const float *)in, (float *)out, W, H);
    else hipLaunchKernelGGL(rt_ssao_blur_kernel<false>, grid, dim3(256), 0, s, (const float *)in, (float *)out, W, H);
    return hipGetLastError();
}

// =========================================================================================
// Equirectangular -> cubemap: ConvertHDRToCubemap (TextureLoader.cpp:118-194) with
// skyboxVs.glsl / skyboxFs.glsl -- six 90-degree captures of a unit cube, per texel
// texture(equirect, SampleSphericalMap(normalize(localPos))).  Same fp32 expression shapes as
// oracle/rt_post_oracle.c::orc_equirect_to_cubemap, including Mesa's atan2 / asin lowerings (the oracle is
// pinned to the shader on llvmpipe with them).  One-off producer of the ray kernel's skybox (6 x 512^2 texels):
// one lane per face texel, the equirect map is converted to RGB16F once (what GL's upload does, toward zero
// on the reference's GL) and gathered with 4 bilinear taps; faces are written as packed RGB16F, round toward zero.
// =========================================================================================
namespace {
__device__ __forceinline__ float cm_sign(float x) { return x > 0.0f ? 1.0f : x < 0.0f ? -1.0f : 0.0f; }
__device__ __forceinline__ float cm_atan(float yx) {
    const float a = fabsf(yx);
    const float t = fminf(a, 1.0f) / fmaxf(a, 1.0f);
    const float x2 = t * t, x3 = x2 * t, x5 = x3 * x2, x7 = x5 * x2, x9 = x7 * x2, x11 = x9 * x2;
    float p = t * 0.9999793128310355f;
    p = x3 * -0.3326756418091246f + p;
    p = x5 * 0.1938924977115610f + p;
    p = x7 * -0.1173503194786851f + p;
    p = x9 * 0.0536813784310406f + p;
    p = x11 * -0.0121323213173444f + p;
    p = p + (a > 1.0f ? 1.0f : 0.0f) * (p * -2.0f + 1.57079632679489661923f);
    return p * cm_sign(yx);
}
__device__ __forceinline__ float cm_atan2(float y, float x) {
    const bool flip = 0.0f >= x;
    const float s = flip ? fabsf(x) : y, t = flip ? y : fabsf(x);
    const float scale = fabsf(t) >= 1e18f ? 0.25f : 1.0f;
    const float rcp = 1.0f / (t * scale);
    const float s_over_t = (s * scale) * rcp;
    const float tn = fabsf(fabsf(x) == fabsf(y) ? 1.0f : s_over_t);
    const float arc = (flip ? 1.0f : 0.0f) * 1.57079632679489661923f + cm_atan(tn);
    return fminf(y, rcp) < 0.0f ? -arc : arc;
}
__device__ __forceinline__ float cm_asin(float x) {
    const float ax = fabsf(x);
    const float pi4m1 = 0.78539816339744830962f - 1.0f;
    float t = ax * -0.03102955f + 0.086566724f;
    t = ax * t + pi4m1;
    t = ax * t + 1.57079632679489661923f;
    const float r = 1.57079632679489661923f - sqrtf(1.0f - ax) * t;
    return cm_sign(x) * r;
}
__constant__ float CM_S[6][3] = {{0, 0, -1}, {0, 0, 1}, {1, 0, 0}, {1, 0, 0}, {1, 0, 0}, {-1, 0, 0}};
__constant__ float CM_U[6][3] = {{0, -1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}, {0, -1, 0}, {0, -1, 0}};
__constant__ float CM_F[6][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
}  // namespace

// f32 RGB -> RGB16F texels (glTexImage2D(GL_RGB16F, GL_FLOAT) upload: the reference's GL rounds toward zero there
// too -- tests/golden/cubemap.npz's upload probe), padded to 4 halfs
__global__ __launch_bounds__(256) void rt_equirect_upload_kernel(const float *__restrict__ rgb, uint2 *__restrict__ tex, size_t n) {
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (size_t)gridDim.x * 256) {
        tex[k] = make_uint2(cvt_pkrtz_u(rgb[3 * k], rgb[3 * k + 1]), cvt_pkrtz_u(rgb[3 * k + 2], 1.0f));
    }
}

__global__ __launch_bounds__(256) void rt_equirect_to_cubemap_kernel(const uint2 *__restrict__ tex, int W, int H, int S,
                                                                     unsigned short *__restrict__ faces) {
    const int i = blockIdx.x * 32 + (threadIdx.x & 31), j = blockIdx.y * 8 + (threadIdx.x >> 5), f = blockIdx.z;
    if (i >= S || j >= S) return;
    const float xn = (((float)i + 0.5f) / (float)S) * 2.0f - 1.0f, yn = (((float)j + 0.5f) / (float)S) * 2.0f - 1.0f;
    const float px = CM_F[f][0] + xn * CM_S[f][0] + yn * CM_U[f][0], py = CM_F[f][1] + xn * CM_S[f][1] + yn * CM_U[f][1];
    const float pz = CM_F[f][2] + xn * CM_S[f][2] + yn * CM_U[f][2];
    const float dd = (pz * pz + py * py) + px * px;
    const float r = 1.0f / sqrtf(dd);
    const float dx = px * r, dy = py * r, dz = pz * r;                           // normalize(localPos)
    float u = cm_atan2(dz, dx), v = cm_asin(dy);                                 // SampleSphericalMap
    u = u * 0.1591f + 0.5f;
    v = v * 0.3183f + 0.5f;
    const float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;                // LINEAR, CLAMP_TO_EDGE
    const float fx = floorf(x), fy = floorf(y);
    const float wx = x - fx, wy = y - fy;
    const int x0 = min(max((int)fx, 0), W - 1), x1 = min(max((int)fx + 1, 0), W - 1);
    const int y0 = min(max((int)fy, 0), H - 1), y1 = min(max((int)fy + 1, 0), H - 1);
    const uint2 t00 = tex[(size_t)y0 * W + x0], t10 = tex[(size_t)y0 * W + x1], t01 = tex[(size_t)y1 * W + x0], t11 = tex[(size_t)y1 * W + x1];
    auto lerp2 = [&](float a00, float a10, float a01, float a11) -> float {
        const float a = a00 + wx * (a10 - a00), b = a01 + wx * (a11 - a01);
        return a + wy * (b - a);
    };
    const float cr = lerp2(h2f_u(t00.x), h2f_u(t10.x), h2f_u(t01.x), h2f_u(t11.x));
    const float cg = lerp2(h2f_u(t00.x >> 16), h2f_u(t10.x >> 16), h2f_u(t01.x >> 16), h2f_u(t11.x >> 16));
    const float cb = lerp2(h2f_u(t00.y), h2f_u(t10.y), h2f_u(t01.y), h2f_u(t11.y));
    const unsigned rg = cvt_pkrtz_u(cr, cg), b1 = cvt_pkrtz_u(cb, 1.0f);
    unsigned short *o = faces + (((size_t)f * S + j) * S + i) * 3;
    o[0] = (unsigned short)(rg & 0xffffu); o[1] = (unsigned short)(rg >> 16); o[2] = (unsigned short)(b1 & 0xffffu);
}

hipError_t rt_launch_equirect_to_cubemap(const float *dRgb, void *dTex, int W, int H, int S, void *dFaces, hipStream_t s) {
    const size_t n = (size_t)W * H;
    size_t blocks = (n + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(rt_equirect_upload_kernel, dim3((unsigned)blocks), dim3(256), 0, s, dRgb, (uint2 *)dTex, n);
    dim3 grid((S + 31) / 32, (S + 7) / 8, 6);
    hipLaunchKernelGGL(rt_equirect_to_cubemap_kernel, grid, dim3(256), 0, s, (const uint2 *)dTex, W, H, S, (unsigned short *)dFaces);
    return hipGetLastError();
}

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
    if (srgb) quads ? go(rt_display_pack_kernel<true, true>) : go(rt_display_pack_kernel<true, false>);
    else quads ? go(rt_display_pack_kernel<false, true>) : go(rt_display_pack_kernel<false, false>);
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
    auto pick = [&](auto toneC) {
        constexpr int T = decltype(toneC)::value;
        if (srgb) quads ? go(rt_display_pack_toned_kernel<true, true, T>) : go(rt_display_pack_toned_kernel<true, false, T>);
        else quads ? go(rt_display_pack_toned_kernel<false, true, T>) : go(rt_display_pack_toned_kernel<false, false, T>);
    };
    if (tone == TONE_NONE) pick(std::integral_constant<int, TONE_NONE>{});
    else if (tone == TONE_REINHARD) pick(std::integral_constant<int, TONE_REINHARD>{});
    else pick(std::integral_constant<int, TONE_ACES>{});
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
    auto pick = [&](auto toneC, auto srgbC) {
        constexpr int T = decltype(toneC)::value;
        constexpr bool S = decltype(srgbC)::value;
        if (i420) fast ? go(rt_display_pack_yuv_kernel<S, T, true, true>) : go(rt_display_pack_yuv_kernel<S, T, true, false>);
        else fast ? go(rt_display_pack_yuv_kernel<S, T, false, true>) : go(rt_display_pack_yuv_kernel<S, T, false, false>);
    };
    auto pickTone = [&](auto srgbC) {
        if (tone == TONE_NONE) pick(std::integral_constant<int, TONE_NONE>{}, srgbC);
        else if (tone == TONE_REINHARD) pick(std::integral_constant<int, TONE_REINHARD>{}, srgbC);
        else pick(std::integral_constant<int, TONE_ACES>{}, srgbC);
    };
    if (srgb) pickTone(std::true_type{});
    else pickTone(std::false_type{});
    return hipGetLastError();
}

// =========================================================================================
// Exposure metering (rt_meter, include/rt_mi355.h): a 256-bin histogram of log-luminance over any rgba32f surface, then the solve
// of rt_meter.h as a launch of its own behind it.  Bandwidth-bound like the pack (16 B read per pixel, nothing written but the
// 1 KiB state), and the code base's one device-wide reduction: integer atomics only, so the state is bit-identical from run to run.
// Grid sized to the chip -- RT_METER_WGS_PER_CU workgroups of 256 threads per CU, a grid-stride loop over quads of four consecutive
// pixels of the flat surface (four 16-B loads in flight per lane) -- so a frame flushes (workgroups x non-empty bins) global atomics
// however large it is.  Every wave keeps a histogram of its own in LDS (ds_add_u32, no return).  Coherent content (a floor, the sky)
// puts all 64 lanes of a wave into one or two bins, and same-address LDS atomics serialise: before touching LDS the wave takes up to
// RT_METER_PEER rounds of "the first pending lane's bin, a ballot of the lanes that share it, ONE add of the popcount"; lanes still
// pending after that add 1 each.  The counters and the extremes stay in registers for the whole loop and are reduced once per wave
// (DPP rotations inside the rows of 16 lanes, v_readlane across the four rows), then once per workgroup through LDS: one global atomic per
// workgroup and quantity.  minLum accumulates as the maximum of the complemented bit pattern (positive floats order like their bits),
// so that the cleared state -- zero bytes, one hipMemsetAsync in front of the kernel -- is its neutral element.
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
// A commutative reduction over the 64 lanes of a full wave: four DPP rotations inside each row of 16 lanes (row_ror:8, 4, 2, 1 leave
// the row's result in every one of its lanes), then the four rows through v_readlane.  The result is wave-uniform.
template <class Op>
__device__ __forceinline__ unsigned meter_wave_reduce(unsigned v, Op op) {
    v = op(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false));
    v = op(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, false));
    v = op(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xf, 0xf, false));
    v = op(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xf, 0xf, false));
    return op(op((unsigned)__builtin_amdgcn_readlane((int)v, 0), (unsigned)__builtin_amdgcn_readlane((int)v, 16)),
              op((unsigned)__builtin_amdgcn_readlane((int)v, 32), (unsigned)__builtin_amdgcn_readlane((int)v, 48)));
}
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
            const float Y = (0.2126f * p[k].x + 0.7152f * p[k].y) + 0.0722f * p[k].z;
            const unsigned bits = __float_as_uint(Y);
            const bool isNaN = Y != Y, isInf = Y == __builtin_huge_valf(), pos = Y > 0.0f;
            bool metered = have && pos && !isInf;
            cNaN += (have && isNaN) ? 1u : 0u;
            cInf += (have && isInf) ? 1u : 0u;
            cNonPos += (have && !pos && !isNaN) ? 1u : 0u;
            const int e = (int)(bits >> 20) - 888;
            const unsigned bin = (unsigned)min(max(e, 0), 255);
            mnC = max(mnC, metered ? ~bits : 0u);
            mx = max(mx, metered ? bits : 0u);
            unsigned long long todo = __builtin_amdgcn_ballot_w64(metered);
#pragma unroll
            for (int it = 0; it < RT_METER_PEER; it++) {
                if (todo == 0ull) break;                    // (wave-uniform)
                const unsigned leader = (unsigned)__builtin_ctzll(todo);
                const unsigned lb = (unsigned)__builtin_amdgcn_readlane((int)bin, (int)leader);
                const bool same = metered && bin == lb;
                const unsigned long long peers = __builtin_amdgcn_ballot_w64(same);
                if (lane == leader) atomicAdd(&wh[lb], (unsigned)__builtin_popcountll(peers));
                metered = metered && !same;
                todo &= ~peers;
            }
            if (metered) atomicAdd(&wh[bin], 1u);
        }
    }
    // once per wave: reduce the registers across the lanes, lane 0 carries the wave's figures into the workgroup's
    const auto add = [](unsigned a, unsigned b) { return a + b; };
    const auto umax = [](unsigned a, unsigned b) { return max(a, b); };
    cNonPos = meter_wave_reduce(cNonPos, add);
    cNaN = meter_wave_reduce(cNaN, add);
    cInf = meter_wave_reduce(cInf, add);
    mnC = meter_wave_reduce(mnC, umax);
    mx = meter_wave_reduce(mx, umax);
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
    scan[0][b] = count;
    if (b < 8u) lq[b] = a.tab.log2q16[b];
    __syncthreads();
    int cur = 0;
#pragma unroll
    for (unsigned d = 1; d < 256u; d <<= 1) {
        scan[cur ^ 1][b] = scan[cur][b] + (b >= d ? scan[cur][b - d] : 0u);
        cur ^= 1;
        __syncthreads();
    }
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
    static const int nCU = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        return n;
    }();
    const unsigned nQuads = (nPixels + 3u) / 4u;
    const unsigned want = (nQuads + 255u) / 256u, cap = (unsigned)nCU * RT_METER_WGS_PER_CU;
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
