// rt_shade.inc -- main() of raytracingCs.glsl (:509-584) on caller-supplied rays (rt_shade_rays; include/rt_mi355.h).
// #included at the end of rt_kernels.hip, after rt_query.inc.  The path tracer itself is rt_lane.inc's, the one rt_render_kernel
// runs, so a shaded ray is the same fp32 expression tree as a rendered pixel; this file holds where the scene lives (ShadeScene),
// the ray -> pixel map, the loads, the stores and the launch.  rt_render_kernel stages the whole compiled scene in LDS (capped at
// RT_EXHAUSTIVE_MAX_*); here every wave-uniform record (object bounds and shapes in the loops, light records, Halton entries)
// comes by scalar loads from the global copy through the constant address space, the hit object's records by per-lane loads,
// and closest hits from rt_query.inc's loop.  No LDS, no cap on the scene size.  Design and measurements: DESIGN.md "Shading rays".

// rt_lane.inc's accessor over the global copy of the compiled scene.  Offsets of its sections (rt_device.h, rt_compiled_f4):
// hot, material, lights, Halton 2 / 3.
struct ShadeScene {
    const float4 *cmp;
    int nObj, nLt;
    int matF4, lgtF4, haltonFloat;
    static constexpr bool fastPbr = true;
    struct Rec {            // a hot record by scalar loads
        const float4 *cmp;
        int b;
        __device__ __forceinline__ float4 operator[](int k) const { return q_hot(cmp, b + k); }
    };
    __device__ __forceinline__ Rec rec(int i) const { return Rec{cmp, i * RT_HOT_F4}; }
    __device__ __forceinline__ float4 light(int i, int k) const { return q_hot(cmp, lgtF4 + i * RT_LGT_F4 + k); }
    __device__ __forceinline__ float halton(int which, int i, int base) const {
        return (i < RT_HALTON_N) ? ((pk_uni1_t)(unsigned long long)cmp)[haltonFloat + which * RT_HALTON_N + i] : halton_eval(i, base);
    }
    __device__ __forceinline__ const float4 *lane_hot(int idx) const { return cmp + (size_t)idx * RT_HOT_F4; }
    __device__ __forceinline__ const float4 *lane_mat(int idx) const { return cmp + matF4 + (size_t)idx * RT_MAT_F4; }
    __device__ __forceinline__ bool shape(const Ray &r, float a, Rec h, float4 h0, float4 h1, float &t) const {
        return q_shape(cmp, h.b, r, a, h0, h1, t);
    }
    __device__ __forceinline__ int closest(const Ray &r, float maxDist, float &t) const {
        return q_trace<false>(cmp, nObj, r, maxDist, true, t);
    }
    template <int COUNT>
    __device__ __forceinline__ bool any(const Ray &r, float maxDist, float limit, unsigned &rays) const {
        return lane_any<COUNT>(*this, nObj, r, maxDist, limit, rays);
    }
};

__device__ __forceinline__ ShadeScene sh_scene(const float4 *cmp, int nObj, int nLt) {
    ShadeScene s;
    s.cmp = cmp;
    s.nObj = nObj;
    s.nLt = nLt;
    s.matF4 = nObj * RT_HOT_F4;
    s.lgtF4 = s.matF4 + nObj * RT_MAT_F4;
    s.haltonFloat = (s.lgtF4 + nLt * RT_LGT_F4) * 4;
    return s;
}

#define RT_SH_BLOCK 256

// One ray per lane.  rays[2k] = (origin, tMax), rays[2k+1] = (direction, -).  pixels: the (gx, gy) ray k is shaded as, or
// null: ray k is surface index k of rt_render_to(f.p) (rt_camera_rays' layout), window pixels outside the image get
// all-zero records.  Tail lanes store nothing.  pos / nrm may be null (not stored).
__global__ __launch_bounds__(RT_SH_BLOCK) void rt_shade_rays_kernel(const RtFrame f, const float4 *__restrict__ cmp,
                                                                    const uint8_t *__restrict__ noise,
                                                                    const uint16_t *__restrict__ sky,
                                                                    const float4 *__restrict__ rays,
                                                                    const uint2 *__restrict__ pixels, size_t nRays,
                                                                    float4 *__restrict__ gColor, float4 *__restrict__ gPosition,
                                                                    uint2 *__restrict__ gNormal) {
    const size_t k = (size_t)blockIdx.x * RT_SH_BLOCK + threadIdx.x;
    if (k >= nRays) return;
    unsigned gx, gy;
    if (pixels) {
        const uint2 px = pixels[k];
        gx = px.x;
        gy = px.y;
    } else {
        const int i = (int)(k % (size_t)f.p.regionW), j = (int)(k / (size_t)f.p.regionW);
        const int gxI = f.p.x0 + i;
        const int ly = f.p.y0 + j;
        const int gyI = (ly / f.p.stripRows) * f.p.stripCycleRows + f.p.stripOffsetRows + ly % f.p.stripRows;
        if (gxI >= f.p.width || gyI >= f.p.height) {      // rt_render_to's record of a pixel outside the image
            gColor[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (gPosition) gPosition[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (gNormal) gNormal[k] = make_uint2(0u, 0u);
            return;
        }
        gx = (unsigned)gxI;
        gy = (unsigned)gyI;
    }
    const ShadeScene sc = sh_scene(cmp, f.nObj, f.nLt);
    const float nz = sample_noise(f, noise, gx, gy);     // the PCF jitter (:359); the camera jitter is the caller's

    const float4 r0 = rays[2 * k], r1 = rays[2 * k + 1];
    Ray ray;
    ray.o = V3(r0);
    ray.d = V3(r1);

    // the primary segment ends at the ray's tMax (rt_trace_rays CLOSEST); no ray counter (COUNT = 0: `rays` is never touched)
    unsigned noRays = 0;
    const LanePath out = lane_path<0>(sc, f, sky, ray, r0.w, gx, gy, nz, noRays);
    const v3 P = out.P, N = out.N;

    gColor[k] = make_float4(out.color.x, out.color.y, out.color.z, 1.0f);
    if (gPosition) gPosition[k] = make_float4(P.x, P.y, P.z, 1.0f);
    if (gNormal) gNormal[k] = make_uint2(f2h_rtz(N.x) | (f2h_rtz(N.y) << 16), f2h_rtz(N.z) | (0x3c00u << 16));
}

hipError_t rt_launch_shade_rays(const RtFrame &f, const float4 *dCompiled, const uint8_t *dNoise, const uint16_t *dSky,
                                const float4 *dRays, const uint2 *dPixels, size_t nRays, float4 *dColor, float4 *dPos,
                                uint2 *dNormal, hipStream_t s) {
    if (nRays == 0) return hipSuccess;
    const size_t blocks = (nRays + RT_SH_BLOCK - 1) / RT_SH_BLOCK;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rt_shade_rays_kernel, dim3((unsigned)blocks), dim3(RT_SH_BLOCK), 0, s, f, dCompiled, dNoise, dSky, dRays,
                       dPixels, nRays, dColor, dPos, dNormal);
    return hipGetLastError();
}
