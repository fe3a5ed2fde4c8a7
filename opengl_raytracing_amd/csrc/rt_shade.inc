// rt_shade.inc -- main() of raytracingCs.glsl (:509-584) on caller-supplied rays (rt_shade_rays; include/rt_mi355.h).
// #included at the end of rt_kernels.hip, after rt_query.inc: it reuses the render kernels' helpers (aabb_test, shape_test,
// compute_pbr, fresnel_schlick, calc_refraction, hemisphere_dir, random2, sample_noise, sample_cube, f2h_rtz, halton_eval,
// build_frame's hemi rows) and rt_query.inc's closest-hit loop without moving or editing them, and follows
// rt_render_kernel's structure line for line, so a shaded ray is the same fp32 expression tree as a rendered pixel.
// What differs is where the scene lives: rt_render_kernel stages the whole compiled scene in LDS (capped at
// RT_EXHAUSTIVE_MAX_*); here every wave-uniform record (object bounds and shapes in the loops, light records, Halton
// entries) comes by scalar loads from the global copy through the constant address space, and the hit object's material
// by one per-lane load per hit.  No LDS, no cap on the scene size.  Design and measurements: DESIGN.md "Shading rays".

// Offsets of the compiled scene's sections (rt_device.h, rt_compiled_f4): hot, material, lights, Halton 2 / 3.
struct ShadeScene {
    const float4 *cmp;
    int nObj, nLt;
    int matF4, lgtF4, haltonFloat;
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

// halton_lookup with the table entry (wave-uniform index) by a scalar load
__device__ __forceinline__ float sh_halton(const ShadeScene &sc, int which, int i, int base) {
    return (i < RT_HALTON_N) ? ((pk_uni1_t)(unsigned long long)sc.cmp)[sc.haltonFloat + which * RT_HALTON_N + i]
                             : halton_eval(i, base);
}

// load_mat of object idx (per lane, once per hit)
__device__ __forceinline__ Mat sh_mat(const ShadeScene &sc, int idx) {
    const float4 *m = sc.cmp + sc.matF4 + (size_t)idx * RT_MAT_F4;
    float4 m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3];
    Mat r;
    r.albedo = V3(m0); r.metallic = m0.w;
    r.roughness = m1.x; r.diffuseStrength = m1.y; r.ior = m1.z; r.transparency = m1.w;
    r.sssColor = V3(m2); r.sss = m2.w; r.scatterDistance = m3.x;
    return r;
}

// trace_any's rule with the object records by scalar loads: cull at maxDist, occluded by 0 < t < limit, leave the loop once
// no active lane is unoccluded.  (rt_query.inc's q_trace<true> culls at the value it accepts, so it is not this rule.)
__device__ __forceinline__ bool sh_any(const ShadeScene &sc, const Ray &r, float maxDist, float limit) {
    v3 inv;
    rtf::rcp3(r.d.x, r.d.y, r.d.z, inv.x, inv.y, inv.z);
    const float a = dot(r.d, r.d);
    const float4 *hot = sc.cmp;
    bool occ = false;
    for (int i = 0; i < sc.nObj; i++) {
        const int b = i * RT_HOT_F4;
        const float4 h0 = q_hot(hot, b), h1 = q_hot(hot, b + 1);
        if (!occ && aabb_test(r, inv, h0, h1, maxDist)) {
            float t;
            bool ok;
            if (__float_as_int(h0.w) == 0) {
                const float4 hs[3] = {h0, h1, q_hot(hot, b + 2)};
                ok = shape_test(r, a, hs, 0, t);
            } else {
                const float4 hs[6] = {h0, h1, q_hot(hot, b + 2), q_hot(hot, b + 3), q_hot(hot, b + 4), q_hot(hot, b + 5)};
                ok = shape_test(r, a, hs, __float_as_int(h0.w), t);
            }
            if (ok && t > 0.0f && t < limit) occ = true;
        }
        if (__builtin_amdgcn_ballot_w64(!occ) == 0ull) break;   // every active lane occluded
    }
    return occ;
}

// pcf_shadow (:342-397)
__device__ __forceinline__ float sh_pcf(const ShadeScene &sc, const RtFrame &f, v3 origin, int ltype, int pcfSamples,
                                        float filterSize, v3 lightDir, float limit, float jitterR) {
    float shadow = 0.0f;
    v3 tangent = normalize(cross(lightDir, V3(0.0f, 1.0f, 0.0f)));
    v3 bitangent = cross(lightDir, tangent);
    for (int i = 0; i < pcfSamples; i++) {
        float rx = fract(sh_halton(sc, 0, i, 2) + jitterR);
        float ry = fract(sh_halton(sc, 1, i, 3) + 0.0f);
        v3 jd = (lightDir + (tangent * rx) * filterSize) + (bitangent * ry) * filterSize;
        if (ltype != 1) jd = normalize(jd);
        Ray sr; sr.o = origin; sr.d = jd;
        bool occ = sh_any(sc, sr, f.p.maxRayDistance, limit);
        shadow += occ ? 0.0f : 1.0f;
    }
    return shadow / (float)pcfSamples;
}

// pcss_shadow (:400-440)
__device__ __forceinline__ float sh_pcss(const ShadeScene &sc, const RtFrame &f, v3 origin, int ltype, int pcfSamples,
                                         float filterSize, float searchSize, v3 lightDir, float limit, float jitterR) {
    bool any = false;
    for (int i = 0; i < 16; i++) {
        float rr = sh_halton(sc, 1, i, 3) * 2.0f - 1.0f;
        v3 sd = (lightDir + splat(rr * searchSize)) + splat(rr * searchSize);
        Ray sr; sr.o = origin; sr.d = normalize(sd);
        any |= sh_any(sc, sr, f.p.maxRayDistance, limit);
    }
    if (!any) return 1.0f;
    return sh_pcf(sc, f, origin, ltype, pcfSamples, filterSize, lightDir, limit, jitterR);
}

// compute_sss (:316-339)
__device__ v3 sh_sss(const ShadeScene &sc, const RtFrame &f, v3 P, v3 N, const Mat &m) {
    v3 sss = V3(0.0f, 0.0f, 0.0f);
    for (int i = 0; i < 4; i++) {
        Ray r;
        r.o = P + N * 0.001f;
        r.d = hemisphere_dir(V3(f.sssHemi[i][0], f.sssHemi[i][1], f.sssHemi[i][2]), N);
        float t;
        int idx = q_trace<false>(sc.cmp, sc.nObj, r, f.p.maxRayDistance, true, t);
        if (idx >= 0) {
            float att = det_expf(-t / m.scatterDistance);
            sss = sss + V3(sc.cmp[sc.matF4 + (size_t)idx * RT_MAT_F4]) * att;
        }
    }
    return ((sss * m.sssColor) * m.sss) / 4.0f;
}

// compute_lighting (:457-507), the light records by scalar loads
__device__ __forceinline__ v3 sh_lighting(const ShadeScene &sc, const RtFrame &f, v3 P, v3 N, const Mat &m, v3 V,
                                          float jitterR) {
    v3 Lo = V3(0.0f, 0.0f, 0.0f);
    v3 shadowOrigin = P + N * 0.001f;
    for (int i = 0; i < sc.nLt; i++) {
        const int b = sc.lgtF4 + i * RT_LGT_F4;
        float4 l0 = q_hot(sc.cmp, b), l1 = q_hot(sc.cmp, b + 1), l2 = q_hot(sc.cmp, b + 2), l3 = q_hot(sc.cmp, b + 3);
        int ltype = __float_as_int(l0.w);
        v3 lightDir = V3(0.0f, 0.0f, 0.0f);
        float attenuation = 1.0f, lightDistance = 0.0f;
        if (ltype == 0) {
            lightDir = V3(l0) - P;
            lightDistance = length(lightDir);
            attenuation = rtf::rcp(1.0f + 0.1f * lightDistance + 0.01f * lightDistance * lightDistance);
            lightDir = normalize(lightDir);
        } else if (ltype == 1) {
            lightDir = V3(l1);
            lightDistance = 1e6f;
        } else if (ltype == 2) {
            lightDir = V3(l0) - P;
            float q = dot(lightDir, lightDir);
            lightDistance = length(lightDir);
            lightDir = normalize(lightDir);
            attenuation = rtf::rcp(fabsf(q));
            float lc = fmaxf(dot(lightDir, V3(l1)), 0.0f);
            attenuation *= lc;
        }
        int shadowType = __float_as_int(l3.x), pcfSamples = __float_as_int(l3.y);
        float shadowFactor = 1.0f;
        if (shadowType != 0) {
            float limit = (ltype == 1) ? f.p.maxRayDistance : fminf(f.p.maxRayDistance, lightDistance);
            if (ltype != 1 && !(lightDistance == lightDistance)) limit = -1.0f;
            if (shadowType == 1)
                shadowFactor = sh_pcf(sc, f, shadowOrigin, ltype, pcfSamples, l2.w, lightDir, limit, jitterR);
            else if (shadowType == 2)
                shadowFactor = sh_pcss(sc, f, shadowOrigin, ltype, pcfSamples, l2.w, l3.z, lightDir, limit, jitterR);
            else
                shadowFactor = 0.0f;
        }
        v3 L = normalize(lightDir);
        v3 H = normalize(V + L);
        v3 radiance = (V3(l2) * attenuation) * l1.w;
        Lo = Lo + compute_pbr<true>(m, N, V, L, H, radiance) * shadowFactor;
    }
    if (m.sss > 0.0f) Lo = Lo + sh_sss(sc, f, P, N, m);
    return Lo;
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

    v3 finalColor = V3(0.0f, 0.0f, 0.0f), throughput = V3(1.0f, 1.0f, 1.0f);
    v3 P = V3(0.0f, 0.0f, 0.0f), N = V3(0.0f, 0.0f, 0.0f);

    for (int depth = 0; depth < f.p.maxRayDepth; ++depth) {
        float t;
        // the primary segment ends at the ray's tMax (rt_trace_rays CLOSEST), every later one at maxRayDistance
        int idx = q_trace<false>(sc.cmp, sc.nObj, ray, depth == 0 ? r0.w : f.p.maxRayDistance, true, t);
        if (idx < 0) {
            if (f.p.useSkybox && sky) finalColor = finalColor + throughput * sample_cube(sky, f.skySize, ray.d);
            break;
        }
        {
            const float4 *h = sc.cmp + (size_t)idx * RT_HOT_F4;
            if (__float_as_int(h[0].w) == 0) N = normalize((ray.o + ray.d * t) - V3(h[2]));
            else N = V3(h[3]);
        }
        const Mat m = sh_mat(sc, idx);
        P = ray.o + ray.d * t;
        v3 V = normalize(-ray.d);
        v3 Lo = sh_lighting(sc, f, P, N, m, V, nz);
        finalColor = finalColor + throughput * Lo;

        if (depth > 2) {
            float dw = length(m.albedo) * m.diffuseStrength;
            float cp = fminf(fmaxf(throughput.x, fmaxf(throughput.y, throughput.z)) * 0.95f + dw, 0.99f);
            float rnd = random2((float)(gx + (unsigned)depth), (float)(gy + (unsigned)depth));
            if (rnd > cp) break;
            throughput = div3(throughput, cp);
        }
        float F = fresnel_schlick(fmaxf(dot(V, N), 0.0f), m.ior);
        if (m.diffuseStrength > 0.0f) {
            const int dd = depth < RT_MAX_DEPTH ? depth : RT_MAX_DEPTH - 1;
            v3 sd = reflect(ray.d, N);
            v3 hd = hemisphere_dir(V3(f.hemi[dd][0], f.hemi[dd][1], f.hemi[dd][2]), N);
            ray.d = normalize(mix_fast(sd, hd, m.roughness));
            ray.o = P + N * 0.001f;
            throughput = throughput * (m.albedo * m.diffuseStrength);
        } else if (m.transparency > 0.0f) {
            ray.d = calc_refraction(ray, N, m.ior);
            ray.o = P - N * 0.001f;
            throughput = throughput * ((m.albedo * (1.0f - F)) * m.transparency);
        } else {
            ray.d = reflect(ray.d, N);
            ray.o = P + N * 0.001f;
            throughput = throughput * (m.albedo * F);
        }
    }

    gColor[k] = make_float4(finalColor.x, finalColor.y, finalColor.z, 1.0f);
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
