// rt_accel_render.inc -- whole frames through the threaded hierarchy of rt_set_accel (rt_set_accel_render; DESIGN.md section 37).
// #included at the end of rt_kernels.hip, after rt_accel_shade.inc.  The path tracer is rt_lane.inc's, the pixel map and the
// stores are rt_render_kernel's, the walks rt_accel.inc's and rt_accel_shade.inc's; this file holds the frame kernel that puts
// them together -- camera ray and noise sample from the frame, no ray buffer, no pixel list -- the SPLIT accessor, and the launch.
//
// LANE and WAVE are AccelShadeScene<true> / <false> as they stand.  SPLIT is the mix a ray batch cannot make and a frame can: the
// 64 primary rays of an 8x8 tile are coherent, so the depth-0 closest hit is one a_trace_wave<false> walk for the wavefront
// (nodes in SGPRs); every later ray -- bounce, shadow, blocker, subsurface -- is not, and takes the per-ray walks.  Both walks
// answer the brute-force bits for every ray (sections 32, 33), so which of them a given ray takes changes no pixel.
//
// No LDS, no stack, no scratch; the kernel has no loop of its own: the walks' (cur strictly forward, below nNodes) and lane_path's.

// Measured alternatives (DESIGN.md section 37; tools/bench_accel_render.py --variant).  The shipped form is 64-thread workgroups
// in raster order: the XCD-band order was 3-41 % slower on all seven measured scenes, 256-thread workgroups 13-26 % slower.
#ifndef RT_AR_BLOCK
#define RT_AR_BLOCK 64           // threads per workgroup: 64 (one 8x8 tile) or 256 (16x16 pixels, rt_render_kernel's shape)
#endif
#ifndef RT_AR_XCD
#define RT_AR_XCD 0              // 1: one band of workgroups per XCD (the bloom kernels' map) instead of raster order
#endif
static_assert(RT_AR_BLOCK == 64 || RT_AR_BLOCK == 256, "one wavefront per 8x8 tile, one or four of them per workgroup");

// AccelShadeScene<true> whose FIRST closest() of a lane is the per-wavefront walk.  lane_path makes that call at depth 0, where
// every in-image lane of the wave is still on its path, before any other ray of the pixel; the flag is the lane's own.
struct AccelSplitScene : AccelShadeScene<true> {
    mutable bool primary;
    __device__ __forceinline__ int closest(const Ray &r, float maxDist, float &t) const {
        if (primary) {
            primary = false;
            return a_trace_wave<false>(acc, cmp, r, maxDist, true, t);
        }
        return a_trace_lane<false>(acc, cmp, r, maxDist, true, t);
    }
};

template <int TRAV> struct AccelRenderScene { typedef AccelShadeScene<TRAV == RT_ACCEL_RENDER_LANE> type; };
template <> struct AccelRenderScene<RT_ACCEL_RENDER_SPLIT> { typedef AccelSplitScene type; };

// Workgroup b of a grid of n (a multiple of 8 when RT_AR_XCD) -> the tile group it renders
__device__ __forceinline__ unsigned ar_group() {
    return RT_AR_XCD ? (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3) : blockIdx.x;
}

template <int TRAV>
__global__ __launch_bounds__(RT_AR_BLOCK) void rt_render_accel_kernel(const RtFrame f, const float4 *__restrict__ cmp, const RtAccelDev acc,
                                                                      const uint8_t *__restrict__ noise, const uint16_t *__restrict__ sky,
                                                                      float4 *__restrict__ gColor, float4 *__restrict__ gPosition,
                                                                      uint2 *__restrict__ gNormal) {
    // ---- lane -> pixel: rt_render_kernel's map inside the 8x8 tile of the wave
    constexpr int edge = RT_AR_BLOCK == 64 ? 8 : 16;
    const int groupsX = (f.p.regionW + edge - 1) / edge, groupsY = (f.p.regionH + edge - 1) / edge;
    const unsigned group = ar_group();
    if (group >= (unsigned)groupsX * (unsigned)groupsY) return;      // (the padding of an XCD-banded grid)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = (int)(group % (unsigned)groupsX) * edge + (wave & 1) * 8 + (lane & 7);
    const int j = (int)(group / (unsigned)groupsX) * edge + (wave >> 1) * 8 + (lane >> 3);
    if (i >= f.p.regionW || j >= f.p.regionH) return;
    const int gxI = f.p.x0 + i;
    const int ly = f.p.y0 + j;
    const int gyI = (ly / f.p.stripRows) * f.p.stripCycleRows + f.p.stripOffsetRows + ly % f.p.stripRows;
    const size_t outIdx = f.imageStores ? (size_t)gyI * f.p.width + gxI : (size_t)j * f.p.regionW + i;
    if (gxI >= f.p.width || gyI >= f.p.height) {   // outside the image: GL discards the imageStore
        if (!f.imageStores) {                      // (a whole-image surface has no such pixel)
            gColor[outIdx] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            gPosition[outIdx] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            gNormal[outIdx] = make_uint2(0u, 0u);
        }
        return;
    }
    const unsigned gx = (unsigned)gxI, gy = (unsigned)gyI;

    typename AccelRenderScene<TRAV>::type sc;
    static_cast<ShadeScene &>(sc) = sh_scene(cmp, f.nObj, f.nLt);
    sc.acc = acc;
    if constexpr (TRAV == RT_ACCEL_RENDER_SPLIT) sc.primary = true;

    const float nz = sample_noise(f, noise, gx, gy);
    unsigned noRays = 0;                                  // (COUNT = 0: never touched)
    const LanePath out = lane_path<0>(sc, f, sky, camera_ray(f, nz, gxI, gyI), f.p.maxRayDistance, gx, gy, nz, noRays);
    const v3 P = out.P, N = out.N;

    gColor[outIdx] = make_float4(out.color.x, out.color.y, out.color.z, 1.0f);
    gPosition[outIdx] = make_float4(P.x, P.y, P.z, 1.0f);
    gNormal[outIdx] = make_uint2(f2h_rtz(N.x) | (f2h_rtz(N.y) << 16), f2h_rtz(N.z) | (0x3c00u << 16));
}

// traversal: RT_ACCEL_RENDER_LANE / _WAVE / _SPLIT (resolved: not AUTO)
hipError_t rt_launch_render_accel(const RtFrame &f, const float4 *dCompiled, const RtAccelDev &acc, int traversal, const uint8_t *dNoise,
                                  const uint16_t *dSky, float4 *dColor, float4 *dPos, uint2 *dNormal, hipStream_t s) {
    if (f.p.regionW <= 0 || f.p.regionH <= 0) return hipSuccess;
    constexpr int edge = RT_AR_BLOCK == 64 ? 8 : 16;
    size_t groups = (size_t)((f.p.regionW + edge - 1) / edge) * (size_t)((f.p.regionH + edge - 1) / edge);
    if (RT_AR_XCD) groups = (groups + 7) / 8 * 8;
    if (groups > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 g((unsigned)groups), b(RT_AR_BLOCK);
    if (traversal == RT_ACCEL_RENDER_LANE)
        hipLaunchKernelGGL(rt_render_accel_kernel<RT_ACCEL_RENDER_LANE>, g, b, 0, s, f, dCompiled, acc, dNoise, dSky, dColor, dPos, dNormal);
    else if (traversal == RT_ACCEL_RENDER_WAVE)
        hipLaunchKernelGGL(rt_render_accel_kernel<RT_ACCEL_RENDER_WAVE>, g, b, 0, s, f, dCompiled, acc, dNoise, dSky, dColor, dPos, dNormal);
    else if (traversal == RT_ACCEL_RENDER_SPLIT)
        hipLaunchKernelGGL(rt_render_accel_kernel<RT_ACCEL_RENDER_SPLIT>, g, b, 0, s, f, dCompiled, acc, dNoise, dSky, dColor, dPos, dNormal);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}
