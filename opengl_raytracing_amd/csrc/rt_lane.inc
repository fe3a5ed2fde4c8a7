// rt_lane.inc -- main() of raytracingCs.glsl (:509-584) for one lane: the per-lane path tracer behind rt_render_kernel (the
// exhaustive cross-check, variant 0) and rt_shade_rays_kernel, written once.  #included in rt_kernels.hip's namespace after
// the arithmetic helpers.  (The packet kernel, rt_packet.inc, is organised around the wavefront and is its own code.)
//
// The functions are templates over a scene accessor A, which says where the compiled records come from and nothing else:
//   int nObj, nLt                       the scene's counts
//   Rec rec(int i)                      object i's hot record, i wave-uniform (the traversal loops): h[k] is its float4 k
//   bool shape(r, a, h, h0, h1, t)      shape_test of that object, whose first two float4 the caller holds
//   int closest(r, maxDist, t)          intersectObjects (:155-196): the hit index or -1, t = minT
//   bool any<COUNT>(r, maxDist, limit, rays)   a shadow / blocker ray's answer (lane_any's rule; LaneLds and ShadeScene call it)
//   float4 light(int i, int k)          float4 k of light i's record, i wave-uniform
//   float halton(which, i, base)        haltonSequence(i, base), i wave-uniform: entry i of table `which` (0: base 2, 1: base
//                                       3), halton_eval beyond RT_HALTON_N
//   const float4 *lane_hot(int idx)     the hit object's hot record, idx per lane
//   const float4 *lane_mat(int idx)     the hit object's material record, idx per lane
//   static constexpr bool fastPbr       compute_pbr's form
// LaneLds (rt_kernels.hip) reads the workgroup's LDS copy; ShadeScene (rt_shade.inc) reads the global copy by scalar loads and
// per-lane loads.  The counts and the record handle are the accessor's, not the frame's, because the compiler then keeps both
// kernels' code as it was with a tracer each (DESIGN.md section 28).  COUNT: the instrumented build's ray counter; with
// COUNT = 0 `rays` is never touched.

// generateCameraRay (:198-217) of image pixel (gxI, gyI); nz = the pixel's noise sample (jitter :512-514: .x from the R8
// sample, .y of an R8 texture is 0 -> -1, A.1#3)
__device__ __forceinline__ Ray camera_ray(const RtFrame &f, float nz, int gxI, int gyI) {
    const float jx = nz * 2.0f - 1.0f, jy = 0.0f * 2.0f - 1.0f;
    float ux = (((float)gxI + 0.5f) + jx) / (float)f.p.width;
    float uy = (((float)gyI + 0.5f) + jy) / (float)f.p.height;
    ux = ux * 2.0f - 1.0f;
    uy = uy * 2.0f - 1.0f;
    ux *= f.sx;
    uy *= f.sy;
    const v3 cd = V3(f.p.camDir[0], f.p.camDir[1], f.p.camDir[2]);
    const v3 cr = V3(f.p.camRight[0], f.p.camRight[1], f.p.camRight[2]);
    const v3 cu = V3(f.p.camUp[0], f.p.camUp[1], f.p.camUp[2]);
    Ray ray;
    ray.o = V3(f.p.camPos[0], f.p.camPos[1], f.p.camPos[2]);
    ray.d = normalize((cd + cr * ux) + cu * uy);
    return ray;
}

__device__ __forceinline__ Mat load_mat(const float4 *m) {
    float4 m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3];
    Mat r;
    r.albedo = V3(m0); r.metallic = m0.w;
    r.roughness = m1.x; r.diffuseStrength = m1.y; r.ior = m1.z; r.transparency = m1.w;
    r.sssColor = V3(m2); r.sss = m2.w; r.scatterDistance = m3.x;
    return r;
}

// Any-hit form for shadow / PCSS blocker rays (trace_any's rule): true iff some object is hit with 0 < t < limit, limit =
// min(maxRayDistance, lightDistance) for point/area lights and maxRayDistance for directional ones (exactly the reference's
// closest-hit test, A.1#14).  Culls at maxDist.  Lanes that found an occluder idle; the loop ends when the whole wave is done.
template <int COUNT, typename A>
__device__ __forceinline__ bool lane_any(const A &sc, int nObj, const Ray &r, float maxDist, float limit, unsigned &rays) {
    if (COUNT) rays++;
    v3 inv;
    rtf::rcp3(r.d.x, r.d.y, r.d.z, inv.x, inv.y, inv.z);
    float a = dot(r.d, r.d);
    bool occ = false;
    for (int i = 0; i < nObj; i++) {
        const auto h = sc.rec(i);
        const float4 h0 = h[0], h1 = h[1];
        if (!occ && aabb_test(r, inv, h0, h1, maxDist)) {
            float t;
            if (sc.shape(r, a, h, h0, h1, t) && t > 0.0f && t < limit) occ = true;
        }
        if (__builtin_amdgcn_ballot_w64(!occ) == 0ull) break;   // every active lane occluded
    }
    return occ;
}

// pcfShadow (:342-397)
template <int COUNT, typename A>
__device__ __forceinline__ float lane_pcf(const A &sc, const RtFrame &f, v3 origin, int ltype, int pcfSamples,
                                          float filterSize, v3 lightDir, float limit, float jitterR, unsigned &rays) {
    float shadow = 0.0f;
    v3 tangent = normalize(cross(lightDir, V3(0.0f, 1.0f, 0.0f)));
    v3 bitangent = cross(lightDir, tangent);
    for (int i = 0; i < pcfSamples; i++) {
        float rx = fract(sc.halton(0, i, 2) + jitterR);
        float ry = fract(sc.halton(1, i, 3) + 0.0f);
        v3 jd = (lightDir + (tangent * rx) * filterSize) + (bitangent * ry) * filterSize;
        if (ltype != 1) jd = normalize(jd);
        Ray sr; sr.o = origin; sr.d = jd;
        bool occ = sc.template any<COUNT>(sr, f.p.maxRayDistance, limit, rays);
        shadow += occ ? 0.0f : 1.0f;
    }
    return shadow / (float)pcfSamples;
}

// pcssShadow (:400-440): 16 blocker-search rays; any blocker -> plain PCF (penumbra size is dead)
template <int COUNT, typename A>
__device__ __forceinline__ float lane_pcss(const A &sc, const RtFrame &f, v3 origin, int ltype, int pcfSamples,
                                           float filterSize, float searchSize, v3 lightDir, float limit, float jitterR,
                                           unsigned &rays) {
    bool any = false;
    for (int i = 0; i < 16; i++) {
        float rr = sc.halton(1, i, 3) * 2.0f - 1.0f;
        v3 sd = (lightDir + splat(rr * searchSize)) + splat(rr * searchSize);
        Ray sr; sr.o = origin; sr.d = normalize(sd);
        any |= sc.template any<COUNT>(sr, f.p.maxRayDistance, limit, rays);
    }
    if (!any) return 1.0f;
    return lane_pcf<COUNT>(sc, f, origin, ltype, pcfSamples, filterSize, lightDir, limit, jitterR, rays);
}

// computeSubsurfaceScattering (:316-339)
template <int COUNT, typename A>
__device__ v3 lane_sss(const A &sc, const RtFrame &f, v3 P, v3 N, const Mat &m, unsigned &rays) {
    v3 sss = V3(0.0f, 0.0f, 0.0f);
    for (int i = 0; i < 4; i++) {
        Ray r;
        r.o = P + N * 0.001f;
        r.d = hemisphere_dir(V3(f.sssHemi[i][0], f.sssHemi[i][1], f.sssHemi[i][2]), N);
        float t;
        if (COUNT) rays++;
        int idx = sc.closest(r, f.p.maxRayDistance, t);
        if (idx >= 0) {
            float att = det_expf(-t / m.scatterDistance);
            sss = sss + V3(sc.lane_mat(idx)[0]) * att;
        }
    }
    return ((sss * m.sssColor) * m.sss) / 4.0f;
}

// computeLighting (:457-507)
template <int COUNT, typename A>
__device__ __forceinline__ v3 lane_lighting(const A &sc, const RtFrame &f, v3 P, v3 N, const Mat &m, v3 V, float jitterR,
                                            unsigned &rays) {
    v3 Lo = V3(0.0f, 0.0f, 0.0f);
    v3 shadowOrigin = P + N * 0.001f;     // :381, :412
    for (int i = 0; i < sc.nLt; i++) {
        float4 l0 = sc.light(i, 0), l1 = sc.light(i, 1), l2 = sc.light(i, 2), l3 = sc.light(i, 3);
        int ltype = __float_as_int(l0.w);
        v3 lightDir = V3(0.0f, 0.0f, 0.0f);
        float attenuation = 1.0f, lightDistance = 0.0f;
        if (ltype == 0) {
            lightDir = V3(l0) - P;
            lightDistance = length(lightDir);
            attenuation = rtf::rcp(1.0f + 0.1f * lightDistance + 0.01f * lightDistance * lightDistance);
            lightDir = normalize(lightDir);
        } else if (ltype == 1) {
            lightDir = V3(l1);             // normalize(-direction), folded by the scene compiler
            lightDistance = 1e6f;
        } else if (ltype == 2) {
            lightDir = V3(l0) - P;
            // lightDistance*lightDistance = sqrt(q)*sqrt(q) folds to |q| on the reference's GL
            float q = dot(lightDir, lightDir);
            lightDistance = length(lightDir);
            lightDir = normalize(lightDir);
            attenuation = rtf::rcp(fabsf(q));
            float lc = fmaxf(dot(lightDir, V3(l1)), 0.0f);   // l1 = normalize(direction)
            attenuation *= lc;
        }
        int shadowType = __float_as_int(l3.x), pcfSamples = __float_as_int(l3.y);
        float shadowFactor = 1.0f;
        if (shadowType != 0) {
            // any-hit limit: closest t < lightDistance for point/area lights (:390-392, :421-423)
            float limit = (ltype == 1) ? f.p.maxRayDistance : fminf(f.p.maxRayDistance, lightDistance);
            // NaN lightDistance: the reference's `t < NaN` is false -> never occluded
            if (ltype != 1 && !(lightDistance == lightDistance)) limit = -1.0f;
            if (shadowType == 1)
                shadowFactor = lane_pcf<COUNT>(sc, f, shadowOrigin, ltype, pcfSamples, l2.w, lightDir, limit, jitterR, rays);
            else if (shadowType == 2)
                shadowFactor = lane_pcss<COUNT>(sc, f, shadowOrigin, ltype, pcfSamples, l2.w, l3.z, lightDir, limit, jitterR, rays);
            else
                shadowFactor = 0.0f;       // calculateShadow's `float shadow = 0.0` fall-through (:445)
        }
        v3 L = normalize(lightDir);
        v3 H = normalize(V + L);
        v3 radiance = (V3(l2) * attenuation) * l1.w;
        Lo = Lo + compute_pbr<A::fastPbr>(m, N, V, L, H, radiance) * shadowFactor;
    }
    if (m.sss > 0.0f) Lo = Lo + lane_sss<COUNT>(sc, f, P, N, m, rays);
    return Lo;
}

// The bounce loop (:519-577) of the pixel (gx, gy) from its primary ray, whose segment ends at tMax0 (every later one at
// maxRayDistance); nz = the pixel's noise sample (the PCF jitter, :359).  Yields finalColor and the last hit's P and N.
struct LanePath { v3 color, P, N; };
template <int COUNT, typename A>
__device__ __forceinline__ LanePath lane_path(const A &sc, const RtFrame &f, const uint16_t *sky, Ray ray, float tMax0, unsigned gx,
                                          unsigned gy, float nz, unsigned &rays) {
    v3 finalColor = V3(0.0f, 0.0f, 0.0f), throughput = V3(1.0f, 1.0f, 1.0f);
    v3 P = V3(0.0f, 0.0f, 0.0f), N = V3(0.0f, 0.0f, 0.0f);   // undefined locals read as zero (A.3)
    for (int depth = 0; depth < f.p.maxRayDepth; ++depth) {
        float t;
        if (COUNT) rays++;
        int idx = sc.closest(ray, depth == 0 ? tMax0 : f.p.maxRayDistance, t);
        if (idx < 0) {
            if (f.p.useSkybox && sky) finalColor = finalColor + throughput * sample_cube(sky, f.skySize, ray.d);
            // else `finalColor += throughput * vec3(0.0)` (:532): x*0.0 folds to 0.0 on the reference's
            // GL, so a NaN/inf throughput does not poison the colour on a miss (nan fixture).
            break;
        }
        // hit normal (:187-191): sphere = normalize(hit - centre); plane = raw normal
        {
            const float4 *h = sc.lane_hot(idx);
            if (__float_as_int(h[0].w) == 0) N = normalize((ray.o + ray.d * t) - V3(h[2]));
            else N = V3(h[3]);
        }
        const Mat m = load_mat(sc.lane_mat(idx));
        P = ray.o + ray.d * t;
        v3 V = normalize(-ray.d);
        v3 Lo = lane_lighting<COUNT>(sc, f, P, N, m, V, nz, rays);
        finalColor = finalColor + throughput * Lo;

        if (depth > 2) {   // Russian roulette (:544-549)
            float dw = length(m.albedo) * m.diffuseStrength;
            float cp = fminf(fmaxf(throughput.x, fmaxf(throughput.y, throughput.z)) * 0.95f + dw, 0.99f);
            float rnd = random2((float)(gx + (unsigned)depth), (float)(gy + (unsigned)depth));
            if (rnd > cp) break;
            throughput = div3(throughput, cp);
        }
        float F = fresnel_schlick(fmaxf(dot(V, N), 0.0f), m.ior);
        if (m.diffuseStrength > 0.0f) {          // :555-567
            const int dd = depth < RT_MAX_DEPTH ? depth : RT_MAX_DEPTH - 1;
            v3 sd = reflect(ray.d, N);
            v3 hd = hemisphere_dir(V3(f.hemi[dd][0], f.hemi[dd][1], f.hemi[dd][2]), N);
            ray.d = normalize(mix_fast(sd, hd, m.roughness));
            ray.o = P + N * 0.001f;
            throughput = throughput * (m.albedo * m.diffuseStrength);
        } else if (m.transparency > 0.0f) {      // :568-571
            ray.d = calc_refraction(ray, N, m.ior);
            ray.o = P - N * 0.001f;
            throughput = throughput * ((m.albedo * (1.0f - F)) * m.transparency);
        } else {                                  // :572-576
            ray.d = reflect(ray.d, N);
            ray.o = P + N * 0.001f;
            throughput = throughput * (m.albedo * F);
        }
    }
    LanePath out; out.color = finalColor; out.P = P; out.N = N;
    return out;
}
