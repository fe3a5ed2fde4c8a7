// rt_query.inc -- ray queries on the compiled scene (rt_trace_rays, rt_camera_rays, rt_pick; include/rt_mi355.h).
// #included at the end of rt_kernels.hip: it reuses the render kernels' helpers (aabb_test, shape_test, rtf::rcp3,
// sample_noise, rt_lane.inc's camera_ray, the scalar-load types of rt_packet.inc), so a query is the same fp32 expression
// tree as the frame's intersectObjects (raytracingCs.glsl:155-196) and generateCameraRay (:198-217).  q_hot, q_shape and
// q_trace<false> are also rt_shade.inc's record fetch and closest-hit loop.  Design and measurements: DESIGN.md "Ray queries".

// One object's hot record, read through a wave-uniform address in the constant address space: s_load_dwordx4 into
// SGPRs, so the bounds and shape operands reach the VALU as scalar operands (no per-lane loads, no LDS staging,
// no cap on the scene size).
__device__ __forceinline__ float4 q_hot(const float4 *hot, int f4Index) {
    pk_f4 v = ((pk_uni4_t)(unsigned long long)hot)[f4Index];
    return make_float4(v.x, v.y, v.z, v.w);
}

// shape_test of the object whose hot record starts at float4 b and whose h0, h1 the caller holds, operands from SGPRs
__device__ __forceinline__ bool q_shape(const float4 *hot, int b, const Ray &r, float a, float4 h0, float4 h1, float &t) {
    if (__float_as_int(h0.w) == 0) {
        const float4 hs[3] = {h0, h1, q_hot(hot, b + 2)};
        return shape_test(r, a, hs, 0, t);
    }
    const float4 hs[6] = {h0, h1, q_hot(hot, b + 2), q_hot(hot, b + 3), q_hot(hot, b + 4), q_hot(hot, b + 5)};
    return shape_test(r, a, hs, __float_as_int(h0.w), t);
}

// intersectObjects (:155-196) with maxRayDistance := tMax.  ANY: stop at the first object with 0 < t < tMax and leave the
// loop once no lane of the wave is unresolved (as lane_any); closest: every object, the lowest index wins ties (strict <).
// Returns the hit index or -1 (ANY: 0 / -1); t = minT.
template <bool ANY>
__device__ __forceinline__ int q_trace(const float4 *hot, int nObj, const Ray &r, float tMax, bool live, float &tOut) {
    v3 inv;
    rtf::rcp3(r.d.x, r.d.y, r.d.z, inv.x, inv.y, inv.z);
    const float a = dot(r.d, r.d);
    float minT = tMax;
    int hit = -1;
    for (int i = 0; i < nObj; i++) {
        const int b = i * RT_HOT_F4;
        const float4 h0 = q_hot(hot, b), h1 = q_hot(hot, b + 1);
        if ((!ANY || hit < 0) && aabb_test(r, inv, h0, h1, tMax)) {
            float t;
            if (q_shape(hot, b, r, a, h0, h1, t) && t > 0.0f && t < minT) {
                minT = ANY ? minT : t;
                hit = ANY ? 0 : i;
            }
        }
        if (ANY && __builtin_amdgcn_ballot_w64(live && hit < 0 && tMax > 0.0f) == 0ull) break;   // no unresolved live lane
    }
    tOut = minT;
    return hit;
}

// The rt_hit of a closest-hit query: the render kernels' P and N (rt_render_kernel: hit normal :187-191).  The hit
// object's type / centre come by per-lane loads (once per ray, after the loop).
__device__ __forceinline__ void q_hit_record(const float4 *hot, const Ray &r, int idx, float t, float4 &w0, float4 &w1) {
    v3 P = V3(0.0f, 0.0f, 0.0f), N = V3(0.0f, 0.0f, 0.0f);   // a miss: undefined locals read as zero (A.3)
    if (idx >= 0) {
        const float4 *h = hot + (size_t)idx * RT_HOT_F4;
        if (__float_as_int(h[0].w) == 0) N = normalize((r.o + r.d * t) - V3(h[2]));
        else N = V3(h[3]);
        P = r.o + r.d * t;
    }
    w0 = make_float4(P.x, P.y, P.z, t);
    w1 = make_float4(N.x, N.y, N.z, __int_as_float(idx));
}

// generateCameraRay (:198-217) of image pixel (gxI, gyI): rt_render_kernel's (rt_lane.inc) on the pixel's noise sample
__device__ __forceinline__ Ray q_camera_ray(const RtFrame &f, const uint8_t *noise, int gxI, int gyI) {
    return camera_ray(f, sample_noise(f, noise, (unsigned)gxI, (unsigned)gyI), gxI, gyI);
}

#define RT_Q_BLOCK 256

// One ray per lane; rays[2k] = (origin, tMax), rays[2k+1] = (direction, reserved).  Closest: out = 2 float4 per ray
// (rt_hit); ANY: one int per ray.  Tail lanes trace a dead ray (tMax 0) and store nothing.
template <bool ANY>
__global__ __launch_bounds__(RT_Q_BLOCK) void rt_trace_rays_kernel(const float4 *__restrict__ rays, size_t nRays,
                                                                    const float4 *__restrict__ hot, int nObj,
                                                                    void *__restrict__ out) {
    const size_t k = (size_t)blockIdx.x * RT_Q_BLOCK + threadIdx.x;
    const bool live = k < nRays;
    float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
    if (live) {
        r0 = rays[2 * k];
        r1 = rays[2 * k + 1];
    }
    Ray r;
    r.o = V3(r0);
    r.d = V3(r1);
    float t;
    const int idx = q_trace<ANY>(hot, nObj, r, r0.w, live, t);
    if (!live) return;
    if (ANY) {
        ((int *)out)[k] = idx >= 0 ? 1 : 0;
    } else {
        float4 w0, w1;
        q_hit_record(hot, r, idx, t, w0, w1);
        float4 *o = (float4 *)out;
        o[2 * k] = w0;
        o[2 * k + 1] = w1;
    }
}

// The primary rays of a window, in rt_render_kernel's output layout (local row j, column i -> j * regionW + i) and
// local-row -> image-row map.  Pixels outside the image: an all-zero ray (tMax 0 misses).
__global__ __launch_bounds__(RT_Q_BLOCK) void rt_camera_rays_kernel(const RtFrame f, const uint8_t *__restrict__ noise,
                                                                     float4 *__restrict__ out) {
    const size_t k = (size_t)blockIdx.x * RT_Q_BLOCK + threadIdx.x;
    const size_t n = (size_t)f.p.regionW * (size_t)f.p.regionH;
    if (k >= n) return;
    const int i = (int)(k % (size_t)f.p.regionW), j = (int)(k / (size_t)f.p.regionW);
    const int gxI = f.p.x0 + i;
    const int ly = f.p.y0 + j;
    const int gyI = (ly / f.p.stripRows) * f.p.stripCycleRows + f.p.stripOffsetRows + ly % f.p.stripRows;
    float4 w0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), w1 = w0;
    if (gxI < f.p.width && gyI < f.p.height) {
        const Ray r = q_camera_ray(f, noise, gxI, gyI);
        w0 = make_float4(r.o.x, r.o.y, r.o.z, f.p.maxRayDistance);
        w1 = make_float4(r.d.x, r.d.y, r.d.z, 0.0f);
    }
    out[2 * k] = w0;
    out[2 * k + 1] = w1;
}

// The primary rays of listed image pixels (rt_camera_rays_at): ray k is pixel pixels[k]'s, the record rt_camera_rays_kernel writes
// for it under an identity window.  An entry outside the image: the all-zero ray, and never an address.
__global__ __launch_bounds__(RT_Q_BLOCK) void rt_camera_rays_at_kernel(const RtFrame f, const uint8_t *__restrict__ noise,
                                                                        const uint2 *__restrict__ pixels, size_t n, float4 *__restrict__ out) {
    const size_t k = (size_t)blockIdx.x * RT_Q_BLOCK + threadIdx.x;
    if (k >= n) return;
    const uint2 px = pixels[k];
    float4 w0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), w1 = w0;
    if (px.x < (unsigned)f.p.width && px.y < (unsigned)f.p.height) {
        const Ray r = q_camera_ray(f, noise, (int)px.x, (int)px.y);
        w0 = make_float4(r.o.x, r.o.y, r.o.z, f.p.maxRayDistance);
        w1 = make_float4(r.d.x, r.d.y, r.d.z, 0.0f);
    }
    out[2 * k] = w0;
    out[2 * k + 1] = w1;
}

// rt_pick: the camera ray of image pixel (px, py) and its closest hit, one wave (lane 0 live).
__global__ __launch_bounds__(64) void rt_pick_kernel(const RtFrame f, const uint8_t *__restrict__ noise,
                                                     const float4 *__restrict__ hot, int px, int py, float4 *__restrict__ out) {
    const bool live = threadIdx.x == 0;
    const Ray r = q_camera_ray(f, noise, px, py);
    float t;
    const int idx = q_trace<false>(hot, f.nObj, r, f.p.maxRayDistance, live, t);
    if (!live) return;
    float4 w0, w1;
    q_hit_record(hot, r, idx, t, w0, w1);
    out[0] = w0;
    out[1] = w1;
}

hipError_t rt_launch_trace_rays(const float4 *dRays, size_t nRays, const float4 *dCompiled, int nObj, int anyHit, void *dOut,
                                hipStream_t s) {
    if (nRays == 0) return hipSuccess;
    const size_t blocks = (nRays + RT_Q_BLOCK - 1) / RT_Q_BLOCK;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    if (anyHit)
        hipLaunchKernelGGL(rt_trace_rays_kernel<true>, dim3((unsigned)blocks), dim3(RT_Q_BLOCK), 0, s, dRays, nRays, dCompiled, nObj, dOut);
    else
        hipLaunchKernelGGL(rt_trace_rays_kernel<false>, dim3((unsigned)blocks), dim3(RT_Q_BLOCK), 0, s, dRays, nRays, dCompiled, nObj, dOut);
    return hipGetLastError();
}

hipError_t rt_launch_camera_rays(const RtFrame &f, const uint8_t *dNoise, float4 *dRays, hipStream_t s) {
    const size_t n = (size_t)f.p.regionW * (size_t)f.p.regionH;
    if (n == 0) return hipSuccess;
    const size_t blocks = (n + RT_Q_BLOCK - 1) / RT_Q_BLOCK;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rt_camera_rays_kernel, dim3((unsigned)blocks), dim3(RT_Q_BLOCK), 0, s, f, dNoise, dRays);
    return hipGetLastError();
}

hipError_t rt_launch_camera_rays_at(const RtFrame &f, const uint8_t *dNoise, const uint2 *dPixels, size_t n, float4 *dRays, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const size_t blocks = (n + RT_Q_BLOCK - 1) / RT_Q_BLOCK;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rt_camera_rays_at_kernel, dim3((unsigned)blocks), dim3(RT_Q_BLOCK), 0, s, f, dNoise, dPixels, n, dRays);
    return hipGetLastError();
}

hipError_t rt_launch_pick(const RtFrame &f, const uint8_t *dNoise, const float4 *dCompiled, int px, int py, float4 *dOut,
                          hipStream_t s) {
    hipLaunchKernelGGL(rt_pick_kernel, dim3(1), dim3(64), 0, s, f, dNoise, dCompiled, px, py, dOut);
    return hipGetLastError();
}
