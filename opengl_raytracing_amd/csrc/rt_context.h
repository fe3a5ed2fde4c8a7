// rt_context.h -- what the files that implement context entry points share (rt_abi.cpp, rt_post.cpp, rt_wire.cpp, and with
// rt_args.h's checks on top of it rt_display.cpp, rt_jpeg.cpp, rt_resample.cpp, rt_accum.cpp, rt_denoise.cpp, rt_reproject.cpp,
// rt_adaptive.cpp): the context itself, the way an entry point reports a failure, the stream it works on, and the rules a frame's
// rt_params obey.  Nothing else knows the context's layout (rt_mgpu.cpp drives contexts through the public ABI).  Not part of the public ABI.
#pragma once
#include <string>
#include <vector>

#include "rt_device.h"
#include "rt_firsthit.h"
#include "rt_present.h"
#include "rt_resample.h"
#include "rt_sched.h"

// rt_set_accel's state (rt_accel.cpp): the settings, the device copy of the current scene's structure and the counters of
// rt_accel_info.  `built`: the queries of the current scene walk the tree (else they run the brute-force kernels).
struct RtAccelState {
    bool on = false, built = false;
    rt_accel_desc desc = {};                   // resolved: no zero field
    RtAccelDev dev;
    DevBuf<uint8_t> dBuf;                      // nodes, order[], loose[]
    PinnedBuf<uint8_t> hStage[2];              // double-buffered like the scene's: a buffer is rewritten only after its last copy has ended
    DevEvent evStage[2];
    bool stageUsed[2] = {false, false};
    unsigned stageSeq = 0;
    rt_accel_report report = {};
    int nOrder = 0;                            // entries of the standing structure's order[] (rt_accel_read)
    // rt_set_accel_builder: who builds, who built what stands, and the device builder's own state
    int builder = RT_ACCEL_BUILD_HOST, builtBy = RT_ACCEL_BUILD_HOST;
    uint64_t buildsHost = 0, buildsDevice = 0;
    double hostMs = 0.0, deviceMs = 0.0;
    DevBuf<uint8_t> dBuildScratch;             // RtAccelBuildScratch's parts: sort ping-pong, histograms, leaf boxes and keys, ranges, parents
    DevEvent evBuild[2], evDepth;              // around the last device build; behind the copy of its depth word
    PinnedBuf<uint32_t> hDepth;
    bool deviceMsPending = false, depthPending = false;      // fetched on first request (rt_accel_build_info, rt_accel_info)
};

// rt_set_accel_shading's state (rt_accel.cpp): whether rt_shade_rays walks rt_set_accel's tree, by which traversal and from how
// many objects, and the launch counters of rt_accel_shading_info.  It owns no structure: `accel.built` says whether there is one.
struct RtAccelShadeState {
    bool on = false;
    int lane = 1;                              // resolved traversal: 1 = per ray, 0 = per wavefront (the index of launchesAccel)
    int minObjects = RT_ACCEL_SHADE_DEFAULT_MIN_OBJECTS;
    uint64_t launchesAccel[2] = {0, 0}, launchesBrute = 0;
};

// rt_set_accel_render's state (rt_accel.cpp): whether plain frames walk rt_set_accel's tree (rt_accel_render.inc), by which
// traversal and from how many objects, and the frame counters of rt_accel_render_info.  It owns no structure either.
struct RtAccelRenderState {
    bool on = false;
    int traversal = RT_ACCEL_RENDER_LANE;      // resolved: RT_ACCEL_RENDER_LANE, _WAVE or _SPLIT
    int minObjects = RT_ACCEL_RENDER_DEFAULT_MIN_OBJECTS;
    uint64_t launchesAccel[3] = {0, 0, 0}, launchesPacket = 0;      // [0] per-wavefront, [1] per-ray, [2] SPLIT
};

// Everything the context allocates is held by an owner (rt_devbuf.h): after rt_destroy has drained the streams, `delete`
// releases it all.  The stream comes first so that it goes last.
struct rt_context {
    int device = 0;
    DevStream stream;
    DevEvent evStart, evStop, evScene;
    bool timed = false;
    // raw SSBO bytes + compiled scene
    DevBuf<uint8_t> dObjects, dLights;
    DevBuf<float4> dCompiled;
    int nObj = 0, nLt = 0;
    bool anyPcss = false;               // some light of the current scene has shadowType 2 (selects the kernel instantiation)
    // double-buffered pinned staging so rt_set_scene never blocks on the GPU and the caller's
    // bytes are consumed before it returns (glBufferData semantics)
    PinnedBuf<uint8_t> hStage[2];
    DevEvent evStage[2];
    bool stageUsed[2] = {false, false};
    unsigned stageSeq = 0;
    // textures
    DevBuf<uint8_t> dNoise;
    int noiseW = 0, noiseH = 0;
    DevBuf<uint16_t> dSky;
    int skySize = 0;
    // context-owned output surfaces
    DevBuf<float4> dColor, dPos;
    DevBuf<uint2> dNormal;
    int surfW = 0, surfH = 0;
    DevBuf<unsigned long long> dRayCounter;
    int variant = 1;   // 1 = wavefront-packet kernel (default), 0 = exhaustive per-lane loop
    unsigned long long lastStats[32] = {};   // rt_count_rays diagnostics (rt_debug_stats)
    RtTileScheduler sched;                     // tile order of the packet kernel's frames; the record of every stream launches go to
    RtFirstHit firstHit;                       // which launches record / replay their first hit (rt_firsthit.h) ...
    DevBuf<uint8_t> dFirstHit;                 // ... and the records: rt_first_hit_bytes() of the recorded window, allocated by the first recording frame
    // settled tiles ride on the first-hit cache, same buffer and lifetime; RT_SETTLED_TILES=0 at rt_create /
    // rt_set_variant's bit 11 (0x800) switch them off
    bool settledEnvOn = true, settledVariantOn = true;
    bool settledOn() const { return settledEnvOn && settledVariantOn; }
    // prefix replay, likewise: RT_PREFIX_REPLAY=0 at rt_create / rt_set_variant's bit 12 (0x1000) switch it off
    bool prefixEnvOn = true, prefixVariantOn = true;
    bool prefixOn() const { return prefixEnvOn && prefixVariantOn; }
    DevBuf<uint2> dBloom[2];                   // rgba16f ping-pong targets of rt_bloom
    DevBuf<float> dSsaoDepth;                  // gPosition.z plane of rt_ssao
    ScratchUse bloomUse, ssaoUse;              // who ran last in dBloom / dSsaoDepth, on whichever stream
    // rt_frame: AO result (raw, blurred), TAA history ping-pong, bloom-combined image when the caller passes none
    DevBuf<float> dFrameAO[2];
    DevBuf<float4> dHistory[2];
    DevBuf<float4> dFrameDisplay;
    int frameW = 0, frameH = 0, lastHistory = -1;
    bool frameAOValid = false;
    // shadow tables of the current scene (rt_shadowtab.inc)
    DevBuf<unsigned> dShadowTab;
    bool shadowTabValid = false;
    bool shadowTabBlocker = false;             // the buffer also holds the blocker-ray tables of the scene's PCSS lights
    std::vector<uint8_t> lastScene;            // the bytes of the current scene (objects, then lights): an identical re-upload is a no-op
    bool stOnePhase = false;                   // RT_ST_BUILD=full: the one-phase builder (every object in every cell; comparison builds only)
    RtShadowTabGeom stGeomSmall = {48, 96, 32}, stGeomLarge = {32, 64, 32};      // <= 32 objects / more (RT_ST_GEOM overrides both); measured: DESIGN.md
    unsigned sceneGen = 0, texGen = 0;         // bumped by rt_set_scene / rt_set_noise / rt_set_skybox / rt_equirect_to_cubemap
    // rt_pick: the hit record on the device and its pinned host copy
    DevBuf<float4> dPick;
    PinnedBuf<rt_hit> hPick;
    PresentRing present;                       // rt_present_*: the frames on their way to the host (rt_present.h)
    ResampleTables resample;                   // rt_display_resample: the device copies of the two axis tables (rt_resample.h)
    DevBuf<uint8_t> dJpegScratch;              // rt_present_submit_jpeg: rt_jpeg_layout's scratch (YUV planes included) ...
    ScratchUse jpegUse;                        // ... and who ran last in it, on whichever stream
    RtAccelState accel;                        // rt_set_accel: the hierarchy behind rt_trace_rays / rt_pick
    RtAccelShadeState accelShade;              // rt_set_accel_shading: ... and, opted into separately, behind rt_shade_rays
    // the next rt_shade_rays walks the tree
    bool accelShadeActive() const { return accelShade.on && accel.built && nObj >= accelShade.minObjects; }
    RtAccelRenderState accelRender;            // rt_set_accel_render: ... and, opted into separately again, behind the frames
    // the next plain frame (packet variant, no ray counter) walks the tree
    bool accelRenderActive() const { return accelRender.on && accel.built && nObj >= accelRender.minObjects; }
    std::string err;
};

// rt_set_scene's hook (rt_accel.cpp): the structure of the new scene, uploaded on the context's stream.  Called between
// waitForLaunches and the record of evScene.
int rt_accel_scene_changed(rt_context *c, const void *objects, int nObj);

inline int fail(rt_context *c, int code, const char *what, hipError_t e = hipSuccess) {
    if (c) {
        c->err = what;
        if (e != hipSuccess) {
            c->err += ": ";
            c->err += hipGetErrorString(e);
        }
    }
    return code;
}

#define HIP_TRY(c, call)                                        \
    do {                                                        \
        hipError_t e_ = (call);                                 \
        if (e_ != hipSuccess) return fail(c, RT_ERR_HIP, #call, e_); \
    } while (0)

// a check of the entry point's own (a validate_* function, rt_args.h): its refusal, which has set the error text, is passed on
#define RT_TRY(check)                                           \
    do {                                                        \
        const int rc_ = (check);                                \
        if (rc_) return rc_;                                    \
    } while (0)

// a call of the scheduler's: the error string names the HIP call that failed inside it
#define SCHED_TRY(c, call)                                      \
    do {                                                        \
        hipError_t e_ = (c)->sched.call;                        \
        if (e_ != hipSuccess) return fail(c, RT_ERR_HIP, (c)->sched.failedCall, e_); \
    } while (0)

// a call of the present ring's: the ring says what was refused, or which HIP call failed inside it
#define PRESENT_TRY(c, call)                                    \
    do {                                                        \
        int rc_ = (c)->present.call;                            \
        if (rc_) return fail(c, rc_, (c)->present.failed, (c)->present.failedHip); \
    } while (0)

// the ABI's `void *hipStream`: the caller's stream, or the context's own when it is NULL
inline hipStream_t stream_or_own(const rt_context *c, void *hipStream) { return hipStream ? (hipStream_t)hipStream : c->stream.s; }

// the rt_params of a frame, as the renders, the queries and rt_frame check them
inline int validate_params(rt_context *c, const rt_params *p) {
    if (!p) return fail(c, RT_ERR_INVALID_ARG, "params is NULL");
    if (p->width <= 0 || p->height <= 0) return fail(c, RT_ERR_INVALID_ARG, "width/height must be positive");
    if (p->regionW < 0 || p->regionH < 0 || p->x0 < 0 || p->y0 < 0)
        return fail(c, RT_ERR_INVALID_ARG, "negative window");
    if (p->stripRows <= 0) return fail(c, RT_ERR_INVALID_ARG, "bad strip mapping");
    if (p->stripCycleRows > 0) {
        if (p->stripOffsetRows < 0 || p->stripOffsetRows + p->stripRows > p->stripCycleRows)
            return fail(c, RT_ERR_INVALID_ARG, "bad strip mapping (offset + rows exceed the cycle)");
    } else if (p->stripCycleRows < 0 || p->stripCount <= 0 || p->stripIndex < 0 || p->stripIndex >= p->stripCount) {
        return fail(c, RT_ERR_INVALID_ARG, "bad strip mapping");
    }
    if (p->maxRayDepth < 0 || p->maxRayDepth > RT_MAX_DEPTH)
        return fail(c, RT_ERR_INVALID_ARG, "maxRayDepth outside [0, 32]");
    return RT_OK;
}
