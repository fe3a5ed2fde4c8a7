// rt_reproject.h -- reprojection of the accumulator (rt_accum_reproject; include/rt_mi355.h has the contract): the per-view constants
// and the projection, written once for host and device as rt_meter.h and rt_accum_solve.h are (the kernel in rt_reproject.hip and
// rt_reproject_project in rt_reproject.cpp run the same rt_reproject_proj), and the launch wrapper.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_mesa_math.h"
#include "rt_mi355.h"

// what the projection reads of an rt_params
struct RtReprojectView {
    float pos[3], dir[3], right[3], up[3];
    float sx, sy;
};

// what the kernel needs of a validated rt_reproject_desc
struct RtReprojectRule {
    RtReprojectView prev, cur;
    int width, height;
    float hx, hy;                   // 0.5f * width, 0.5f * height
    float normalCosMin, planeTol;
    unsigned maxHistory;
};

// word offsets of rt_reproject_report (include/rt_mi355.h pins them)
enum { RR_NPIXELS = 0, RR_NREUSED = 1, RR_NREJECTED = 2, RR_NOFFSCREEN = 3, RR_NMISS = 4, RR_MINCOUNT = 5, RR_MAXCOUNT = 6, RR_SUMCOUNT = 8,
       RR_WORDS = 16 };

// sx, sy exactly as build_frame (rt_abi.cpp) computes them for the render; false when either is not finite and > 0
inline bool rt_reproject_view(const rt_params &p, RtReprojectView *v) {
    for (int k = 0; k < 3; k++) {
        v->pos[k] = p.camPos[k];
        v->dir[k] = p.camDir[k];
        v->right[k] = p.camRight[k];
        v->up[k] = p.camUp[k];
    }
    const float aspect = (float)p.width / (float)p.height;
    const float tanFov = rtm::tan_((p.fovDeg * 0.017453292519943295f) * 0.5f);
    v->sx = aspect * tanFov * p.focalLength;
    v->sy = tanFov * p.focalLength;
    return v->sx > 0.0f && v->sx < __builtin_huge_valf() && v->sy > 0.0f && v->sy < __builtin_huge_valf();
}

// proj(V, P): (fx, fy) in pixel coordinates (pixel centres at integers); true iff z > 0.  fp32, never fused, IEEE divide
__host__ __device__ inline bool rt_reproject_proj(const RtReprojectView &v, float hx, float hy, float px, float py, float pz, float *fx,
                                                  float *fy) {
    const float vx = px - v.pos[0], vy = py - v.pos[1], vz = pz - v.pos[2];
    const float z = (vx * v.dir[0] + vy * v.dir[1]) + vz * v.dir[2];
    const float x = (vx * v.right[0] + vy * v.right[1]) + vz * v.right[2];
    const float y = (vx * v.up[0] + vy * v.up[1]) + vz * v.up[2];
    *fx = ((x / z) / v.sx + 1.0f) * hx - 0.5f;
    *fy = ((y / z) / v.sy + 1.0f) * hy - 0.5f;
    return z > 0.0f;
}

// rt_accum_reproject: a clear of the report (zero; minCount 2^32 - 1), then one launch on s.  accumPrev, accumCur: two planes of width*height float4; hitsPrev,
// hitsCur: width*height rt_hit; report: one rt_reproject_report.  width*height <= 2^31 - 1 (callers refuse larger frames first)
hipError_t rt_launch_reproject(const void *accumPrev, const void *hitsPrev, const void *hitsCur, void *accumCur, void *report,
                               const RtReprojectRule &rule, hipStream_t s);
