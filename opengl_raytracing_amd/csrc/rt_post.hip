// rt_post.hip -- the reference's post passes that consume the ray tracer's surfaces, as gfx950 HIP kernels: the TAA resolve,
// bloom, SSAO and the equirectangular-to-cubemap conversion, each under a banner of its own.
// First one: the TAA resolve of /root/reference/shader/taaFs.glsl:13-53, driven
// like /root/reference/src/ForwardShadingPipeline.cpp:231-260.  Unlike the ray tracer this IS a
// bandwidth-bound kernel: 56 B of compulsory HBM traffic per pixel (current 16 + history 16 +
// gNormal 8 read, 16 written) against ~150 flops.
//
// Layout: 256-thread workgroup = 64x4 pixels, one lane per pixel, 16-B loads and one float4 store per
// lane.  The 3x3 neighbourhood, the jittered bilinear tap, history's 4 taps (normally collapsing onto
// one texel) and the gNormal tap(s) are served by L1/L2.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rt_fastmath.h"
#include "rt_post.h"
#include "rt_wave.h"

// ---- the tunables of this file (-D overrides them; each is described where it is used)
#ifndef RT_TAA_ROWS
#define RT_TAA_ROWS 8           // rows a lane of the register-window TAA kernel walks
#endif
#ifndef RT_BLOOM_XCD
#define RT_BLOOM_XCD 1          // XCD-aware tile order of the fused bloom kernels
#endif
#ifndef RT_SSAO_UNROLL
#define RT_SSAO_UNROLL 8        // unroll of the 64-sample loop
#endif
#ifndef RT_SSAO_TILE_W
#define RT_SSAO_TILE_W 8        // wave tile width in pixels (height = 64 / width)
#endif
#ifndef RT_SSAO_FASTDIV
#define RT_SSAO_FASTDIV 1       // 0 = the compiler's IEEE divisions in the sample loop
#endif
// Settled, and built one way only (the figure is why the other form is gone):
//   the TAA tile + halo staged in LDS, at any tile shape: equal within noise (29-31 us @1080p) -- the pass is limited by the memory pipeline;
//   an XCD-aware TAA tile order (one band of tiles per XCD, as in the bloom kernels): 3 % slower;
//   the one-texel-per-lane TAA kernel for every frame instead of the register window: 28.8 against 27.1 us @1080p, 135 / 118 @4K;
//   several bloom tiles per workgroup with the next patch in flight: 72 / 79 / 81 / 96 / 104 us at 1, 2, 3, 4, 6 tiles @1080p;
//   an XCD-aware SSAO block order: neutral at 1080p (387 vs 386 us), 1.5 % slower at 4K -- the kernel is VALU-bound, not L2-bound.

namespace {

constexpr int TX = 64, TY = 4;      // the one-texel-per-lane kernel's workgroup tile

__device__ __forceinline__ int wrapi(int i, int n) { int r = i % n; return r < 0 ? r + n : r; }
__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

struct rgb { float x, y, z; };
__device__ __forceinline__ rgb rgb_of(float4 q) { rgb r; r.x = q.x; r.y = q.y; r.z = q.z; return r; }
__device__ __forceinline__ rgb lerp3(rgb a, rgb b, float w) {   // a + w*(b-a), per llvmpipe's float path
    rgb r; r.x = a.x + w * (b.x - a.x); r.y = a.y + w * (b.y - a.y); r.z = a.z + w * (b.z - a.z); return r;
}

// ---- the resolve arithmetic both TAA kernels share (taaFs.glsl); how a texel is fetched is each kernel's own
// LINEAR: four texels around a sample, weights = the sample's fractional position
__device__ __forceinline__ rgb taa_bilinear(rgb t00, rgb t10, rgb t01, rgb t11, float wx, float wy) {
    const rgb a = lerp3(t00, t10, wx), b = lerp3(t01, t11, wx);
    return lerp3(a, b, wy);
}
// one more texel into the neighbourhood colour box; texelFetch reads 0 outside the image                    :30-37
__device__ __forceinline__ void taa_box(rgb &mn, rgb &mx, rgb q, bool inb) {
    const float nx = inb ? q.x : 0.0f, ny = inb ? q.y : 0.0f, nz = inb ? q.z : 0.0f;
    mn.x = fminf(mn.x, nx); mn.y = fminf(mn.y, ny); mn.z = fminf(mn.z, nz);
    mx.x = fmaxf(mx.x, nx); mx.y = fmaxf(mx.y, ny); mx.z = fmaxf(mx.z, nz);
}
__device__ __forceinline__ float taa_half(unsigned h) { return __half2float(__ushort_as_half((unsigned short)h)); }
// normal check, NEAREST / REPEAT: the blend factor of a pixel whose normal and jittered normal disagree, else 0     :40-45
__device__ __forceinline__ float taa_normal_blend(const uint2 *normal, int W, int H, float u, float v, float ju, float jv,
                                                  float blendFactor) {
    const int px = wrapi((int)floorf(u * (float)W), W), py = wrapi((int)floorf(v * (float)H), H);
    const int cx = wrapi((int)floorf(ju * (float)W), W), cy = wrapi((int)floorf(jv * (float)H), H);
    const uint2 pn = normal[(size_t)py * W + px];
    const uint2 cn = (cx == px && cy == py) ? pn : normal[(size_t)cy * W + cx];   // sub-texel jitter: same texel
    const float pnx = taa_half(pn.x & 0xffffu), pny = taa_half(pn.x >> 16), pnz = taa_half(pn.y & 0xffffu);
    const float cnx = taa_half(cn.x & 0xffffu), cny = taa_half(cn.x >> 16), cnz = taa_half(cn.y & 0xffffu);
    const float d = (pnz * cnz + pny * cny) + pnx * cnx;
    return d < 0.9f ? blendFactor * 0.2f : 0.0f;
}
// clipAABB (:13-19) then mix(history, current, blendFactor) (:51), one channel
__device__ __forceinline__ float taa_clip_mix(float h, float c, float lo, float hi, float bf) {
    const float center = 0.5f * (hi + lo), extents = 0.5f * (hi - lo);
    float clip = h - center;
    clip = fminf(fmaxf(clip, -extents), extents);
    const float hc = center + clip;
    return hc + bf * (c - hc);
}
__device__ __forceinline__ float4 taa_resolve(rgb his, rgb cur, rgb mn, rgb mx, float bf) {
    return make_float4(taa_clip_mix(his.x, cur.x, mn.x, mx.x, bf), taa_clip_mix(his.y, cur.y, mn.y, mx.y, bf),
                       taa_clip_mix(his.z, cur.z, mn.z, mx.z, bf), 1.0f);
}

}  // namespace

__global__ __launch_bounds__(256) void rt_taa_resolve_kernel(const float4 *__restrict__ current,
                                                             const float4 *__restrict__ history,
                                                             const uint2 *__restrict__ normal,   // half4 per pixel
                                                             float4 *__restrict__ out, int W, int H, float blendFactor,
                                                             float jitterX, float jitterY) {
    const int bx = blockIdx.x * TX, by = blockIdx.y * TY;
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int i = bx + tx, j = by + ty;
    if (i >= W || j >= H) return;

    auto cur_at = [&](int x, int y) -> rgb {   // REPEAT-addressed current texel (x, y may be any integer)
        return rgb_of(current[(size_t)wrapi(y, H) * W + wrapi(x, W)]);
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
        cur = taa_bilinear(cur_at(x0, y0), cur_at(x0 + 1, y0), cur_at(x0, y0 + 1), cur_at(x0 + 1, y0 + 1), wx, wy);
    }
    // history = texture(uHistory, TexCoords): LINEAR, CLAMP_TO_EDGE                   :27
    rgb his;
    {
        const float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
        const float fx = floorf(x), fy = floorf(y);
        const float wx = x - fx, wy = y - fy;
        const int x0 = clampi((int)fx, W), x1 = clampi((int)fx + 1, W), y0 = clampi((int)fy, H), y1 = clampi((int)fy + 1, H);
        auto h_at = [&](int xx, int yy) -> rgb { return rgb_of(history[(size_t)yy * W + xx]); };
        his = taa_bilinear(h_at(x0, y0), h_at(x1, y0), h_at(x0, y1), h_at(x1, y1), wx, wy);
    }
    // neighbourhood colour box
    rgb mn = cur, mx = cur;
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
            const int x = i + dx, y = j + dy;
            const bool inb = x >= 0 && y >= 0 && x < W && y < H;
            taa_box(mn, mx, rgb_of(current[(size_t)clampi(y, H) * W + clampi(x, W)]), inb);
        }
    }
    // (taa_normal_blend, written out: through the function this kernel's schedule gains an s_nop, and the shipped code stays as it is)
    float bf = 0.0f;
    {
        const int px = wrapi((int)floorf(u * (float)W), W), py = wrapi((int)floorf(v * (float)H), H);
        const int cx = wrapi((int)floorf(ju * (float)W), W), cy = wrapi((int)floorf(jv * (float)H), H);
        const uint2 pn = normal[(size_t)py * W + px];
        const uint2 cn = (cx == px && cy == py) ? pn : normal[(size_t)cy * W + cx];
        const float pnx = taa_half(pn.x & 0xffffu), pny = taa_half(pn.x >> 16), pnz = taa_half(pn.y & 0xffffu);
        const float cnx = taa_half(cn.x & 0xffffu), cny = taa_half(cn.x >> 16), cnz = taa_half(cn.y & 0xffffu);
        const float d = (pnz * cnz + pny * cny) + pnx * cnx;
        if (d < 0.9f) bf = blendFactor * 0.2f;
    }
    out[(size_t)j * W + i] = taa_resolve(his, cur, mn, mx, bf);
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
        c[slot][0] = rgb_of(c0); c[slot][1] = rgb_of(c1); c[slot][2] = rgb_of(c2);
        h[slot][0] = rgb_of(h0); h[slot][1] = rgb_of(h1); h[slot][2] = rgb_of(h2);
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
                auto cur_at = [&](int xx, int yy) -> rgb { return rgb_of(current[(size_t)wrapi(yy, H) * W + wrapi(xx, W)]); };
                t00 = cur_at(x0, y0); t10 = cur_at(x0 + 1, y0); t01 = cur_at(x0, y0 + 1); t11 = cur_at(x0 + 1, y0 + 1);
            }
            cur = taa_bilinear(t00, t10, t01, t11, wx, wy);
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
                auto h_at = [&](int xx, int yy) -> rgb { return rgb_of(history[(size_t)yy * W + xx]); };
                t00 = h_at(x0, y0); t10 = h_at(x1, y0); t01 = h_at(x0, y1); t11 = h_at(x1, y1);
            }
            his = taa_bilinear(t00, t10, t01, t11, wx, wy);
        }
        // neighbourhood colour box: the window itself
        rgb mn = cur, mx = cur;
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
#pragma unroll
            for (int dy = -1; dy <= 1; dy++) {
                const int x = i + dx, y = j + dy;
                taa_box(mn, mx, c[dy < 0 ? sa : (dy == 0 ? sm : sb)][dx + 1], x >= 0 && y >= 0 && x < W && y < H);
            }
        }
        const float bf = taa_normal_blend(normal, W, H, u, v, ju, jv, blendFactor);
        out[(size_t)j * W + i] = taa_resolve(his, cur, mn, mx, bf);
    }
}

hipError_t rt_launch_taa_resolve(const void *current, const void *history, const void *normal, void *out, int W, int H,
                                 float blend, float jx, float jy, hipStream_t s) {
    // (`out` must not alias the inputs in either form; frames of a few rows keep the one-texel-per-lane kernel)
    if (H >= 4 * RT_TAA_ROWS) {
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
// brightness extract of one scene texel (brightness_extractFS.glsl:11-19) -> rgba16f
__device__ __forceinline__ uint2 bloom_extract(float4 c, float threshold) {
    const float brightness = (c.z * 0.0722f + c.y * 0.7152f) + c.x * 0.2126f;
    return (brightness > threshold) ? pack_half4(c.x, c.y, c.z) : make_uint2(0u, 0x3c00u << 16);
}
// combine of one scene texel with its blurred rgba16f texel (bloom_combineFs.glsl:10-14)
__device__ __forceinline__ float4 bloom_combine(float4 s, uint2 bl, float strength) {
    return make_float4(s.x + h2f_u(bl.x) * strength, s.y + h2f_u(bl.x >> 16) * strength, s.z + h2f_u(bl.y) * strength, 1.0f);
}

}  // namespace

__global__ __launch_bounds__(256) void rt_bloom_extract_kernel(const float4 *__restrict__ scene, uint2 *__restrict__ out,
                                                               size_t n, float threshold) {
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (size_t)gridDim.x * 256) out[k] = bloom_extract(scene[k], threshold);
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

__global__ __launch_bounds__(256) void rt_bloom_combine_kernel(const float4 *__restrict__ scene, const uint2 *__restrict__ bloom,
                                                               float4 *__restrict__ out, size_t n, float strength) {
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (size_t)gridDim.x * 256) out[k] = bloom_combine(scene[k], bloom[k], strength);
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
    // 249 -> 226 us at 4K).  One tile per workgroup: the 1 350 one-tile workgroups of a 1080p frame are all co-resident and cover
    // each other's phases better than fewer, longer-lived ones.
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
    // (one band of tiles per XCD: the aprons a tile shares with its neighbours come from the SAME L2, not from HBM once per XCD)
    int tile = RT_BLOOM_XCD ? rt_xcd_tile() : (int)blockIdx.x;
    if (tile < nTiles) request(tile);
    // ONE trip (a workgroup past the last tile makes none).  Kept a loop, with the request a lambda ahead of it and the barrier at
    // its end: as straight-line code the four instantiations compile to other schedules (12 to 32 instructions more or less), and
    // the shipped code stays as it is.
    for (; tile < nTiles; tile += nTiles) {
    const int x0 = (tile % tilesX) * FX, y0 = (tile / tilesX) * FY;
    // ---- the requested patch -> LDS
#pragma unroll
    for (int j = 0; j < NLD; j++) {
        const int k = threadIdx.x + j * 256;
        sin_[(k / IW) * IWP + (k % IW)] = FIRST ? bloom_extract(preF[j], threshold) : preH[j];      // FIRST: the extract on the fly
    }
    __syncthreads();
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
        __syncthreads();     // (the loop's: nothing writes the LDS array after it in the one trip)
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
                if (LAST) ((float4 *)outV)[(size_t)y * W + x] = bloom_combine(scene[(size_t)y * W + x], hv, strength);
                else ((uint2 *)outV)[(size_t)y * W + x] = hv;
            }
        }
    }
    }   // (one trip)
}

namespace {
// the fused kernel of one pass pair: FIRST reads the scene, LAST writes the combined image
using BloomHvKernel = void (*)(const void *, const float4 *, void *, int, int, float, float);
BloomHvKernel bloom_hv_kernel(bool first, bool last) {
    return first ? (last ? rt_bloom_hv_kernel<true, true> : rt_bloom_hv_kernel<true, false>)
                 : (last ? rt_bloom_hv_kernel<false, true> : rt_bloom_hv_kernel<false, false>);
}
}  // namespace

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
    dim3 fgrid(RT_BLOOM_XCD ? ((nTilesF + 7) / 8) * 8 : nTilesF), grid((W + 63) / 64, (H + 3) / 4);
    if (pairs == 0) {            // 0 or 1 iterations: the unfused kernels
        hipLaunchKernelGGL(rt_bloom_extract_kernel, dim3(blocks), dim3(256), 0, s, sc, a, n, threshold);
        if (odd) { hipLaunchKernelGGL(rt_bloom_blur_kernel<true>, grid, dim3(256), 0, s, a, b, W, H); a = b; }
        hipLaunchKernelGGL(rt_bloom_combine_kernel, dim3(blocks), dim3(256), 0, s, sc, a, (float4 *)out, n, strength);
        return hipGetLastError();
    }
    for (int p = 0; p < pairs; p++) {
        const bool first = p == 0, last = (p == pairs - 1) && !odd;
        void *dst = last ? out : (void *)b;
        hipLaunchKernelGGL(bloom_hv_kernel(first, last), fgrid, dim3(256), 0, s, (const void *)a, sc, dst, W, H, threshold, strength);
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
    const int nbx = (W + 4 * TW - 1) / (4 * TW);
    const int blkX = (int)(blockIdx.x % (unsigned)nbx), blkY = (int)(blockIdx.x / (unsigned)nbx);
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
    dim3 grid((unsigned)(((W + 4 * TW - 1) / (4 * TW)) * ((H + TH - 1) / TH)));
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
