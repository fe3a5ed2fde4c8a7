// rt_accel.inc -- rt_trace_rays / rt_pick through the threaded hierarchy of rt_set_accel (rt_accel.h has the structure, DESIGN.md
// section 32 the argument).  #included at the end of rt_kernels.hip: aabb_test, shape_test and rt_query.inc's q_hot, q_shape and
// q_hit_record are called as they are, so an object that is tested is tested by the brute-force kernels' own arithmetic.
//
// The hierarchy only culls.  A node is skipped iff every lane fails a_node_test, which no ray that passes the aabb_test of an
// object below the node can fail (the superset property); nothing is skipped for lying behind the current hit.  So the objects
// that count are the brute-force loop's, in another order, and a_accept restores the loop's tie rule (lowest index among equal
// t).  No stack: nodes lie in depth-first pre-order, "descend" is cur + 1, "skip" the node's link.  cur only ever grows, so a
// walk ends within nNodes steps whatever the links hold.

typedef const __attribute__((address_space(4))) unsigned *a_uni_u32_t;

// intersectAABB on a node's box, with one change: an axis on which either product is NaN does not constrain (the slab is
// [-inf, +inf]).  fminf / fmaxf alone would drop only the NaN operand, and a node whose face coincides with the origin of a ray
// with a zero direction component would then fail (NaN, +inf -> [inf, inf]) where a flat box below it passes (NaN, NaN: axis
// ignored).
__device__ __forceinline__ bool a_node_test(const Ray &r, v3 inv, float4 lo, float4 hi, float maxDist) {
    const float inf = __builtin_inff();
    const float t0x = (lo.x - r.o.x) * inv.x, t1x = (hi.x - r.o.x) * inv.x;
    const float t0y = (lo.y - r.o.y) * inv.y, t1y = (hi.y - r.o.y) * inv.y;
    const float t0z = (lo.z - r.o.z) * inv.z, t1z = (hi.z - r.o.z) * inv.z;
    const bool ux = (t0x != t0x) | (t1x != t1x), uy = (t0y != t0y) | (t1y != t1y), uz = (t0z != t0z) | (t1z != t1z);
    const float sx = ux ? -inf : fminf(t0x, t1x), lx = ux ? inf : fmaxf(t0x, t1x);
    const float sy = uy ? -inf : fminf(t0y, t1y), ly = uy ? inf : fmaxf(t0y, t1y);
    const float sz = uz ? -inf : fminf(t0z, t1z), lz = uz ? inf : fmaxf(t0z, t1z);
    const float tMin = fmaxf(fmaxf(sx, sy), sz), tMax = fminf(fminf(lx, ly), lz);
    return (tMax >= tMin) && (tMin < maxDist) && (tMax > 0.0f);
}

// q_trace's `t > 0 && t < minT` for objects that do not come in ascending order: among equal t the lower index wins
__device__ __forceinline__ bool a_accept(float t, int i, float minT, int hit) { return t > 0.0f && (t < minT || (t == minT && i < hit)); }

// q_trace's loop body on object i, records by scalar loads (i is wave-uniform)
template <bool ANY>
__device__ __forceinline__ void a_object_uniform(const float4 *hot, int i, const Ray &r, v3 inv, float a, float tMax, float &minT, int &hit) {
    const int b = i * RT_HOT_F4;
    const float4 h0 = q_hot(hot, b), h1 = q_hot(hot, b + 1);
    if ((!ANY || hit < 0) && aabb_test(r, inv, h0, h1, tMax)) {
        float t;
        if (q_shape(hot, b, r, a, h0, h1, t) && (ANY ? (t > 0.0f && t < minT) : a_accept(t, i, minT, hit))) {
            minT = ANY ? minT : t;
            hit = ANY ? 0 : i;
        }
    }
}

// ... and with the records read per lane (i differs between lanes): q_shape's two record shapes through shape_test's own indexing
template <bool ANY>
__device__ __forceinline__ void a_object_lane(const float4 *hot, int i, const Ray &r, v3 inv, float a, float tMax, float &minT, int &hit) {
    const float4 *h = hot + (size_t)i * RT_HOT_F4;
    const float4 h0 = h[0], h1 = h[1];
    if (aabb_test(r, inv, h0, h1, tMax)) {
        float t;
        if (shape_test(r, a, h, __float_as_int(h0.w), t) && (ANY ? (t > 0.0f && t < minT) : a_accept(t, i, minT, hit))) {
            minT = ANY ? minT : t;
            hit = ANY ? 0 : i;
        }
    }
}

// The loose list: q_trace's loop over loose[] (ascending), after either traversal
template <bool ANY>
__device__ __forceinline__ void a_loose(const RtAccelDev &A, const float4 *hot, const Ray &r, v3 inv, float a, float tMax, bool live, float &minT, int &hit) {
    for (int k = 0; k < A.nLoose; k++) {
        if (ANY && __builtin_amdgcn_ballot_w64(live && hit < 0 && tMax > 0.0f) == 0ull) break;   // no unresolved live lane
        a_object_uniform<ANY>(hot, (int)((a_uni_u32_t)(unsigned long long)A.loose)[k], r, inv, a, tMax, minT, hit);
    }
}

// WAVE: one walk per wavefront.  The node comes by scalar loads, every live lane tests it, and the wave descends iff some lane
// passes.  Lanes meet objects their own walk would have skipped; the object's own aabb_test is the gate, as in q_trace.
template <bool ANY>
__device__ __forceinline__ int a_trace_wave(const RtAccelDev &A, const float4 *hot, const Ray &r, float tMax, bool live, float &tOut) {
    v3 inv;
    rtf::rcp3(r.d.x, r.d.y, r.d.z, inv.x, inv.y, inv.z);
    const float a = dot(r.d, r.d);
    float minT = tMax;
    int hit = -1;
    int cur = 0;
    while (cur < A.nNodes) {
        if (ANY && __builtin_amdgcn_ballot_w64(live && hit < 0 && tMax > 0.0f) == 0ull) break;   // no unresolved live lane
        const float4 n0 = q_hot(A.nodes, 2 * cur), n1 = q_hot(A.nodes, 2 * cur + 1);
        const unsigned leaf = __float_as_uint(n1.w);
        int next = (int)__float_as_uint(n0.w);
        const bool pass = live && (!ANY || hit < 0) && a_node_test(r, inv, n0, n1, tMax);
        if (__builtin_amdgcn_ballot_w64(pass) != 0ull) {
            if (leaf == RT_ACCEL_INNER) {
                next = cur + 1;
            } else {
                const int first = (int)(leaf >> 4), count = (int)(leaf & 15u);
                for (int s = 0; s < count; s++)
                    a_object_uniform<ANY>(hot, (int)((a_uni_u32_t)(unsigned long long)A.order)[first + s], r, inv, a, tMax, minT, hit);
            }
        }
        cur = next > cur ? next : cur + 1;      // strictly forward
    }
    a_loose<ANY>(A, hot, r, inv, a, tMax, live, minT, hit);
    tOut = minT;
    return hit;
}

// LANE: one walk per ray; nodes, indices and records by per-lane loads.  An ANY lane stops at its first hit.
template <bool ANY>
__device__ __forceinline__ int a_trace_lane(const RtAccelDev &A, const float4 *hot, const Ray &r, float tMax, bool live, float &tOut) {
    v3 inv;
    rtf::rcp3(r.d.x, r.d.y, r.d.z, inv.x, inv.y, inv.z);
    const float a = dot(r.d, r.d);
    float minT = tMax;
    int hit = -1;
    int cur = live ? 0 : A.nNodes;
    while (cur < A.nNodes) {
        const float4 n0 = A.nodes[2 * (size_t)cur], n1 = A.nodes[2 * (size_t)cur + 1];
        const unsigned leaf = __float_as_uint(n1.w);
        int next = (int)__float_as_uint(n0.w);
        if (a_node_test(r, inv, n0, n1, tMax)) {
            if (leaf == RT_ACCEL_INNER) {
                next = cur + 1;
            } else {
                const unsigned first = leaf >> 4, count = leaf & 15u;
                for (unsigned s = 0; s < count; s++) a_object_lane<ANY>(hot, (int)A.order[first + s], r, inv, a, tMax, minT, hit);
            }
        }
        cur = next > cur ? next : cur + 1;      // strictly forward
        if (ANY && hit >= 0) break;
    }
    a_loose<ANY>(A, hot, r, inv, a, tMax, live, minT, hit);
    tOut = minT;
    return hit;
}

// rt_trace_rays_kernel (rt_query.inc) with the closest-hit loop replaced: same rays, same records out, same dead tail lanes
template <bool ANY, bool LANE>
__global__ __launch_bounds__(RT_Q_BLOCK) void rt_trace_rays_accel_kernel(const float4 *__restrict__ rays, size_t nRays,
                                                                          const float4 *__restrict__ hot, const RtAccelDev A,
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
    const int idx = LANE ? a_trace_lane<ANY>(A, hot, r, r0.w, live, t) : a_trace_wave<ANY>(A, hot, r, r0.w, live, t);
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

// rt_pick_kernel with the per-wavefront walk (lane 0 live)
__global__ __launch_bounds__(64) void rt_pick_accel_kernel(const RtFrame f, const uint8_t *__restrict__ noise, const float4 *__restrict__ hot,
                                                           const RtAccelDev A, int px, int py, float4 *__restrict__ out) {
    const bool live = threadIdx.x == 0;
    const Ray r = q_camera_ray(f, noise, px, py);
    float t;
    const int idx = a_trace_wave<false>(A, hot, r, f.p.maxRayDistance, live, t);
    if (!live) return;
    float4 w0, w1;
    q_hit_record(hot, r, idx, t, w0, w1);
    out[0] = w0;
    out[1] = w1;
}

hipError_t rt_launch_trace_rays_accel(const float4 *dRays, size_t nRays, const float4 *dCompiled, const RtAccelDev &acc, int anyHit, int lane,
                                      void *dOut, hipStream_t s) {
    if (nRays == 0) return hipSuccess;
    const size_t blocks = (nRays + RT_Q_BLOCK - 1) / RT_Q_BLOCK;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 g((unsigned)blocks), b(RT_Q_BLOCK);
    if (anyHit && lane) hipLaunchKernelGGL((rt_trace_rays_accel_kernel<true, true>), g, b, 0, s, dRays, nRays, dCompiled, acc, dOut);
    else if (anyHit) hipLaunchKernelGGL((rt_trace_rays_accel_kernel<true, false>), g, b, 0, s, dRays, nRays, dCompiled, acc, dOut);
    else if (lane) hipLaunchKernelGGL((rt_trace_rays_accel_kernel<false, true>), g, b, 0, s, dRays, nRays, dCompiled, acc, dOut);
    else hipLaunchKernelGGL((rt_trace_rays_accel_kernel<false, false>), g, b, 0, s, dRays, nRays, dCompiled, acc, dOut);
    return hipGetLastError();
}

hipError_t rt_launch_pick_accel(const RtFrame &f, const uint8_t *dNoise, const float4 *dCompiled, const RtAccelDev &acc, int px, int py,
                                float4 *dOut, hipStream_t s) {
    hipLaunchKernelGGL(rt_pick_accel_kernel, dim3(1), dim3(64), 0, s, f, dNoise, dCompiled, acc, px, py, dOut);
    return hipGetLastError();
}
