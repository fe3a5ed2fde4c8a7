// rt_accel_shade.inc -- rt_shade_rays through the threaded hierarchy of rt_set_accel (rt_set_accel_shading; DESIGN.md section 33).
// #included at the end of rt_kernels.hip, after rt_accel.inc.  The path tracer is rt_lane.inc's, the kernel body a copy of rt_shade.inc's;
// this file holds the accessor whose closest() and any() walk the tree instead of testing every object, and the launch.
//
// closest() is rt_accel.inc's a_trace_lane<false> / a_trace_wave<false>, which section 32 proves equal to q_trace<false>.  any()
// is new: lane_any's rule has TWO distances -- the stored-box gate culls at maxDist, the hit is accepted on 0 < t < limit -- so
// rt_accel.inc's one-distance any-hit walks are not it.  The walks below test nodes and gate objects at maxDist and accept at
// limit.  The answer is existential ("some object passes its own gate and its shape with 0 < t < limit"), the set of objects that
// pass their own gate is the brute-force loop's by the superset property, and so the visiting order and the early outs cannot
// change it.  limit <= 0 or NaN (lane_lighting's -1 for a NaN light distance) accepts nothing: such a lane never walks.
//
// Both walks run under the path tracer's divergence: lanes whose path has ended, or that are in another branch, are inactive and
// so take part in no ballot.  No stack, no LDS.

// lane_any's loop body on object i, records by scalar loads (i is wave-uniform)
__device__ __forceinline__ void as_object_uniform(const float4 *hot, int i, const Ray &r, v3 inv, float a, float maxDist, float limit, bool &occ) {
    const int b = i * RT_HOT_F4;
    const float4 h0 = q_hot(hot, b), h1 = q_hot(hot, b + 1);
    if (!occ && aabb_test(r, inv, h0, h1, maxDist)) {
        float t;
        if (q_shape(hot, b, r, a, h0, h1, t) && t > 0.0f && t < limit) occ = true;
    }
}

// ... and with the records read per lane (i differs between lanes), as a_object_lane reads them
__device__ __forceinline__ void as_object_lane(const float4 *hot, int i, const Ray &r, v3 inv, float a, float maxDist, float limit, bool &occ) {
    const float4 *h = hot + (size_t)i * RT_HOT_F4;
    const float4 h0 = h[0], h1 = h[1];
    if (aabb_test(r, inv, h0, h1, maxDist)) {
        float t;
        if (shape_test(r, a, h, __float_as_int(h0.w), t) && t > 0.0f && t < limit) occ = true;
    }
}

// The loose list, as lane_any tests it: in ascending order, until no active lane is unresolved
__device__ __forceinline__ void as_loose(const RtAccelDev &A, const float4 *hot, const Ray &r, v3 inv, float a, float maxDist, float limit, bool open, bool &occ) {
    for (int k = 0; k < A.nLoose; k++) {
        if (__builtin_amdgcn_ballot_w64(open && !occ) == 0ull) break;
        as_object_uniform(hot, (int)((a_uni_u32_t)(unsigned long long)A.loose)[k], r, inv, a, maxDist, limit, occ);
    }
}

// WAVE: one walk for the active lanes of the wavefront; the node comes by scalar loads and the walk descends iff some active,
// unresolved lane passes it.
__device__ __forceinline__ bool as_any_wave(const RtAccelDev &A, const float4 *hot, const Ray &r, float maxDist, float limit) {
    v3 inv;
    rtf::rcp3(r.d.x, r.d.y, r.d.z, inv.x, inv.y, inv.z);
    const float a = dot(r.d, r.d);
    const bool open = limit > 0.0f;
    bool occ = false;
    int cur = 0;
    while (cur < A.nNodes) {
        if (__builtin_amdgcn_ballot_w64(open && !occ) == 0ull) break;      // no unresolved active lane
        const float4 n0 = q_hot(A.nodes, 2 * cur), n1 = q_hot(A.nodes, 2 * cur + 1);
        const unsigned leaf = __float_as_uint(n1.w);
        int next = (int)__float_as_uint(n0.w);
        const bool pass = open && !occ && a_node_test(r, inv, n0, n1, maxDist);
        if (__builtin_amdgcn_ballot_w64(pass) != 0ull) {
            if (leaf == RT_ACCEL_INNER) {
                next = cur + 1;
            } else {
                const int first = (int)(leaf >> 4), count = (int)(leaf & 15u);
                for (int s = 0; s < count; s++)
                    as_object_uniform(hot, (int)((a_uni_u32_t)(unsigned long long)A.order)[first + s], r, inv, a, maxDist, limit, occ);
            }
        }
        cur = next > cur ? next : cur + 1;      // strictly forward
    }
    as_loose(A, hot, r, inv, a, maxDist, limit, open, occ);
    return occ;
}

// LANE: one walk per ray; nodes, indices and records by per-lane loads, no ballot in the tree.  A lane stops at its first occluder.
__device__ __forceinline__ bool as_any_lane(const RtAccelDev &A, const float4 *hot, const Ray &r, float maxDist, float limit) {
    v3 inv;
    rtf::rcp3(r.d.x, r.d.y, r.d.z, inv.x, inv.y, inv.z);
    const float a = dot(r.d, r.d);
    const bool open = limit > 0.0f;
    bool occ = false;
    int cur = open ? 0 : A.nNodes;
    while (cur < A.nNodes) {
        const float4 n0 = A.nodes[2 * (size_t)cur], n1 = A.nodes[2 * (size_t)cur + 1];
        const unsigned leaf = __float_as_uint(n1.w);
        int next = (int)__float_as_uint(n0.w);
        if (a_node_test(r, inv, n0, n1, maxDist)) {
            if (leaf == RT_ACCEL_INNER) {
                next = cur + 1;
            } else {
                const unsigned first = leaf >> 4, count = leaf & 15u;
                for (unsigned s = 0; s < count; s++) as_object_lane(hot, (int)A.order[first + s], r, inv, a, maxDist, limit, occ);
            }
        }
        cur = next > cur ? next : cur + 1;      // strictly forward
        if (occ) break;
    }
    as_loose(A, hot, r, inv, a, maxDist, limit, open, occ);
    return occ;
}

// ShadeScene with the two traversal loops replaced; lights, Halton entries, the hit's records and compute_pbr's form are its own
template <bool LANE>
struct AccelShadeScene : ShadeScene {
    RtAccelDev acc;
    __device__ __forceinline__ int closest(const Ray &r, float maxDist, float &t) const {
        return LANE ? a_trace_lane<false>(acc, cmp, r, maxDist, true, t) : a_trace_wave<false>(acc, cmp, r, maxDist, true, t);
    }
    template <int COUNT>
    __device__ __forceinline__ bool any(const Ray &r, float maxDist, float limit, unsigned &rays) const {
        if (COUNT) rays++;
        return LANE ? as_any_lane(acc, cmp, r, maxDist, limit) : as_any_wave(acc, cmp, r, maxDist, limit);
    }
};

// rt_shade_rays_kernel over the hierarchy: its ray -> pixel map, zero records, loads, stores and tail-lane exit, restated (sharing
// the body through a template changed the operand order of three instructions of rt_shade_rays_kernel, which stays as it was)
template <bool LANE>
__global__ __launch_bounds__(RT_SH_BLOCK) void rt_shade_rays_accel_kernel(const RtFrame f, const float4 *__restrict__ cmp, const RtAccelDev acc,
                                                                          const uint8_t *__restrict__ noise, const uint16_t *__restrict__ sky,
                                                                          const float4 *__restrict__ rays, const uint2 *__restrict__ pixels,
                                                                          size_t nRays, float4 *__restrict__ gColor,
                                                                          float4 *__restrict__ gPosition, uint2 *__restrict__ gNormal) {
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
    AccelShadeScene<LANE> sc;
    static_cast<ShadeScene &>(sc) = sh_scene(cmp, f.nObj, f.nLt);
    sc.acc = acc;
    const float nz = sample_noise(f, noise, gx, gy);     // the PCF jitter (:359); the camera jitter is the caller's

    const float4 r0 = rays[2 * k], r1 = rays[2 * k + 1];
    Ray ray;
    ray.o = V3(r0);
    ray.d = V3(r1);

    unsigned noRays = 0;                                  // (COUNT = 0: never touched)
    const LanePath out = lane_path<0>(sc, f, sky, ray, r0.w, gx, gy, nz, noRays);
    const v3 P = out.P, N = out.N;

    gColor[k] = make_float4(out.color.x, out.color.y, out.color.z, 1.0f);
    if (gPosition) gPosition[k] = make_float4(P.x, P.y, P.z, 1.0f);
    if (gNormal) gNormal[k] = make_uint2(f2h_rtz(N.x) | (f2h_rtz(N.y) << 16), f2h_rtz(N.z) | (0x3c00u << 16));
}

hipError_t rt_launch_shade_rays_accel(const RtFrame &f, const float4 *dCompiled, const RtAccelDev &acc, int lane, const uint8_t *dNoise,
                                      const uint16_t *dSky, const float4 *dRays, const uint2 *dPixels, size_t nRays, float4 *dColor,
                                      float4 *dPos, uint2 *dNormal, hipStream_t s) {
    if (nRays == 0) return hipSuccess;
    const size_t blocks = (nRays + RT_SH_BLOCK - 1) / RT_SH_BLOCK;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 g((unsigned)blocks), b(RT_SH_BLOCK);
    if (lane) hipLaunchKernelGGL(rt_shade_rays_accel_kernel<true>, g, b, 0, s, f, dCompiled, acc, dNoise, dSky, dRays, dPixels, nRays, dColor, dPos, dNormal);
    else hipLaunchKernelGGL(rt_shade_rays_accel_kernel<false>, g, b, 0, s, f, dCompiled, acc, dNoise, dSky, dRays, dPixels, nRays, dColor, dPos, dNormal);
    return hipGetLastError();
}
