// rt_abi.cpp -- the tracer's entry points of the C ABI declared in include/rt_mi355.h: context,
// device buffers, per-frame constants, launches, ray queries and shading, readback, timing, the debug views.  Each entry point
// stands in for a piece of the reference's dispatch site
// (/root/reference/src/ForwardShadingPipeline.cpp:155-182); see the header for the map.
// The tile order of a frame and the stream records are rt_sched.cpp's; the post passes and rt_frame are rt_post.cpp's, the
// strip transport rt_wire.cpp's, the display path rt_display.cpp's.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <new>

#include "rt_context.h"
#include "rt_mesa_math.h"

namespace {

// haltonSequence (/root/reference/shader/raytracingCs.glsl:278-288), host copy for the
// per-depth bounce sample.
float halton_host(int index, int base) {
    float result = 0.0f;
    float f = 1.0f / (float)base;
    int i = index;
    while (i > 0) {
        result += f * (float)(i % base);
        i = i / base;
        f = f / (float)base;
    }
    return result;
}

// cosineWeightedHemisphere's local direction (:292-300) for a given (rand.x, rand.y)
void hemi_local(float rx, float ry, float out[4]) {
    const float PI_F = 3.14159265359f;
    float phi = 2.0f * PI_F * rx;
    float cosTheta = sqrtf(ry);
    float sinTheta = sqrtf(1.0f - ry);
    out[0] = sinTheta * rtm::cos_(phi);      // the reference GL's own cos / sin (rt_mesa_math.h), not libm's
    out[1] = cosTheta;
    out[2] = sinTheta * rtm::sin_(phi);
    out[3] = 0.0f;
}

// The most items (rays, pixels, records) of one launch: 2^31 - 1 workgroups of 256
constexpr size_t kMaxLaunchItems = ((size_t)0x7fffffff) * 256;

// rt_pick / rt_camera_rays_at: only the camera, image size and ray fields of p matter, so p is validated, and the frame built,
// with an identity window
rt_params identity_window(const rt_params &p) {
    rt_params q = p;
    q.x0 = q.y0 = 0;
    q.regionW = q.width;
    q.regionH = q.height;
    q.stripRows = q.stripCount = 1;
    q.stripIndex = q.stripCycleRows = q.stripOffsetRows = 0;
    return q;
}

void build_frame(const rt_context *c, const rt_params *p, RtFrame *f) {
    memset(f, 0, sizeof *f);
    f->p = *p;
    if (p->stripCycleRows <= 0) {      // equal strips: normalise to the cycle/offset form the kernels use
        f->p.stripCycleRows = p->stripRows * p->stripCount;
        f->p.stripOffsetRows = p->stripIndex * p->stripRows;
    }
    f->nObj = c->nObj;
    f->nLt = c->nLt;
    f->anyPcss = c->anyPcss ? 1 : 0;
    f->noiseW = c->noiseW;
    f->noiseH = c->noiseH;
    f->skySize = c->skySize;
    // generateCameraRay (:208-211): aspect, tan(radians(fov)*0.5); radians(x) = x*fl(pi/180)
    float aspect = (float)p->width / (float)p->height;
    // Mesa's tan = sin/cos by its own polynomials (rt_mesa_math.h); libm's tanf is 1 ulp off at fov 45, which
    // perturbs every camera ray and showed up as silhouette flips against the reference's pixels
    float tanFov = rtm::tan_((p->fovDeg * 0.017453292519943295f) * 0.5f);
    f->sx = aspect * tanFov * p->focalLength;
    f->sy = tanFov * p->focalLength;
    // hammersley(depth*64 + frameCount, 64) (:557, :311-313): same sample for every pixel
    for (int d = 0; d < RT_MAX_DEPTH; d++) {
        int hi = d * 64 + p->frameCount;
        hemi_local((float)hi / 64.0f, halton_host(hi, 2), f->hemi[d]);
    }
    for (int i = 0; i < 4; i++) hemi_local((float)i / 4.0f, halton_host(i, 2), f->sssHemi[i]);   // :320
}

// The first-hit reuse of a launch the scheduler may order (packet kernel, no ray counter): which of rt_firsthit.h's three modes
// it is, with the record buffer in place for a recording one.  A buffer that cannot be had (or a window above the cap, which
// decide() has already turned down) is no error: the frame is a normal one, and HIP's error state is cleared.
RtFirstHit::Mode first_hit_mode(rt_context *c, const RtFirstHitKey &key) {
    RtFirstHit::Mode mode = c->firstHit.decide(key);
    if (mode == RtFirstHit::RECORD) {
        const size_t bytes = rt_first_hit_bytes(key.p.regionW, key.p.regionH);
        if (!c->dFirstHit.holds(bytes)) {
            // replays of an earlier, smaller window may still read the old buffer on any stream
            hipError_t e = c->sched.drain();
            if (e == hipSuccess) e = c->dFirstHit.grow(bytes);
            // (zero-initialised when it grows: no flag of the new buffer reads as settled before a recording frame has written it)
            if (e == hipSuccess) e = hipMemsetAsync(c->dFirstHit.ptr, 0, bytes, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                c->firstHit.refuse(key);
                mode = RtFirstHit::NORMAL;
            }
        }
    }
    return mode;
}

// The launches of one frame (launch(), below, is what the entry points call): the first-hit mode, the scheduler's plan, the
// render kernel between the timing events.
int launch_frame(rt_context *c, const rt_params *p, float4 *dColor, float4 *dPos, uint2 *dNormal,
                 unsigned long long *counter, hipStream_t s, bool timed, int countMode, bool imageStores, bool reusable,
                 int *blockerGroup) {
    RtFrame f;
    build_frame(c, p, &f);
    f.imageStores = imageStores ? 1 : 0;
    RtDeviceScene sc;
    sc.compiled = c->dCompiled;
    sc.noise = c->dNoise;
    sc.sky = c->dSky;
    sc.shadowTab = c->shadowTabValid ? c->dShadowTab.ptr : nullptr;
    if (!c->dCompiled) return fail(c, RT_ERR_INVALID_ARG, "rt_set_scene has not been called");
    if (c->variant != 1 && (c->nObj > RT_EXHAUSTIVE_MAX_OBJECTS || c->nLt > RT_EXHAUSTIVE_MAX_LIGHTS))
        return fail(c, RT_ERR_TOO_LARGE, "the exhaustive cross-check kernel stages the scene in LDS: at most 512 objects / 64 lights (use the default kernel)");
    // rt_set_accel_render: a plain frame of a scene whose tree stands is rt_accel_render.inc's.  It keeps out
    // of the first-hit cache and of the tile scheduler -- no key, no plan, no count, as an instrumented launch keeps out of the
    // cache -- but its launch is recorded, so the uploads order behind it.  With the switch off nothing here differs.
    if (c->accelRender.on) {
        if (c->variant == 1 && !counter && c->accelRenderActive()) {
            const int traversal = c->accelRender.traversal;
            if (timed) HIP_TRY(c, hipEventRecord(c->evStart, s));
            HIP_TRY(c, rt_launch_render_accel(f, c->dCompiled, c->accel.dev, traversal, c->dNoise, c->dSky, dColor, dPos, dNormal, s));
            if (timed) {
                HIP_TRY(c, hipEventRecord(c->evStop, s));
                c->timed = true;
            }
            SCHED_TRY(c, recordLaunch(s));
            c->accelRender.launchesAccel[traversal == RT_ACCEL_RENDER_WAVE ? 0 : traversal == RT_ACCEL_RENDER_LANE ? 1 : 2]++;
            return RT_OK;
        }
        c->accelRender.launchesPacket++;
    }
    RtFirstHit::Mode mode = RtFirstHit::NORMAL;
    RtFirstHitKey key;
    // (with reuse switched off nothing below differs from a context that never had it)
    const bool reuse = reusable && c->firstHit.on();
    if (reuse) {
        key = rt_first_hit_key(c->sceneGen, c->texGen, c->nObj, c->nLt, c->variant, c->dNoise != nullptr, c->dSky != nullptr, *p);
        mode = first_hit_mode(c, key);
    }
    RtTileScheduler::Plan plan;
    SCHED_TRY(c, begin(f, sc, s, c->variant == 1 && !counter, ((unsigned long long)c->sceneGen << 32) | c->texGen, &plan,
                       mode == RtFirstHit::REPLAY ? 1 : 0));
    if (mode == RtFirstHit::RECORD) SCHED_TRY(c, beforeFirstHitRecord(s));
    if (mode == RtFirstHit::REPLAY) SCHED_TRY(c, beforeFirstHitReplay(s, plan.rec));
    const RtSplitDesc *split = nullptr;          // a replaying frame whose heaviest tiles run in parts, or null
    if (mode == RtFirstHit::REPLAY) SCHED_TRY(c, splitFor(plan, sc, c->dFirstHit.ptr, s, &split));
    if (timed) HIP_TRY(c, hipEventRecord(c->evStart, s));
    HIP_TRY(c, rt_launch_render(f, sc, dColor, dPos, dNormal, counter, c->variant, s, countMode, (int)mode,
                                mode == RtFirstHit::NORMAL ? nullptr
                                    : (void *)((uintptr_t)c->dFirstHit.ptr | (mode == RtFirstHit::RECORD && !c->settledOn() ? RT_FIRST_HIT_NO_SETTLED : 0) |
                                               (mode == RtFirstHit::RECORD && !c->prefixOn() ? RT_FIRST_HIT_NO_PREFIX : 0)),
                                blockerGroup, split));
    if (timed) {
        HIP_TRY(c, hipEventRecord(c->evStop, s));
        c->timed = true;
    }
    if (mode == RtFirstHit::RECORD) SCHED_TRY(c, afterFirstHitRecord(s, plan.rec));
    SCHED_TRY(c, end(plan, s));
    if (reusable) {
        if (reuse) c->firstHit.launched(mode, key);
        else c->firstHit.counts[RtFirstHit::NORMAL]++;
    }
    return RT_OK;
}

// One frame.  Whatever goes wrong in a launch that could have recorded or replayed (a refusal, a failed HIP call) leaves the
// first-hit state empty: the next frame is a normal one.
int launch(rt_context *c, const rt_params *p, float4 *dColor, float4 *dPos, uint2 *dNormal,
           unsigned long long *counter, hipStream_t s, bool timed, int countMode = 1, bool imageStores = false,
           int *blockerGroup = nullptr) {
    // instrumented launches and the exhaustive kernel always trace the whole frame and leave the cache as it is
    const bool reusable = c->variant == 1 && !counter;
    const int rc = launch_frame(c, p, dColor, dPos, dNormal, counter, s, timed, countMode, imageStores, reusable, blockerGroup);
    if (rc != RT_OK && reusable) c->firstHit.invalidate();
    return rc;
}

// A launch on the caller's stream (null = the context's own) that reads the device scene: a foreign stream first orders
// itself behind the last scene upload (evScene).
int caller_stream(rt_context *c, void *hipStream, hipStream_t *out) {
    hipStream_t s = stream_or_own(c, hipStream);
    if (s != c->stream) HIP_TRY(c, hipStreamWaitEvent(s, c->evScene, 0));
    *out = s;
    return RT_OK;
}

// Which traversal of the hierarchy an rt_trace_rays launch takes (1 = per ray, 0 = per wavefront; the index of
// rt_accel_report.launchesAccel).  RT_ACCEL_AUTO is the per-ray form: the host cannot see whether a batch is coherent, and the
// per-ray walk is the one that never lost to brute force from 1024 objects up (DESIGN.md section 32's table: 7.8-109x on primary
// rays, 1.3-32x on incoherent ones), where the per-wavefront walk is 2x faster still on primary rays but 1.3x slower than brute
// force on incoherent rays at 1024 objects.  A caller that knows its rays are coherent asks for RT_ACCEL_WAVE.
int accel_lane(const rt_accel_desc &d) { return d.traversal == RT_ACCEL_WAVE ? 0 : 1; }

// rt_render_to / rt_render_into_image
int render_on(rt_context *c, const rt_params *p, void *dColor, void *dPosition, void *dNormal, void *hipStream, bool imageStores) {
    if (!c) return RT_ERR_INVALID_ARG;
    int rc = validate_params(c, p);
    if (rc) return rc;
    if (!dColor || !dPosition || !dNormal) return fail(c, RT_ERR_INVALID_ARG, "NULL device surface");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s;
    if ((rc = caller_stream(c, hipStream, &s))) return rc;
    return launch(c, p, (float4 *)dColor, (float4 *)dPosition, (uint2 *)dNormal, nullptr, s, true, 1, imageStores);
}

}  // namespace

extern "C" {

int rt_create(rt_context **out, int deviceId) {
    if (!out) return RT_ERR_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || deviceId < 0 || deviceId >= n) return RT_ERR_NO_DEVICE;
    if (hipSetDevice(deviceId) != hipSuccess) return RT_ERR_NO_DEVICE;
    rt_context *c = new (std::nothrow) rt_context();
    if (!c) return RT_ERR_HIP;
    c->device = deviceId;
    if (const char *e = getenv("RT_ST_BUILD")) c->stOnePhase = strcmp(e, "full") == 0;
    if (const char *e = getenv("RT_FIRST_HIT_REUSE")) c->firstHit.envOn = atoi(e) != 0;
    if (const char *e = getenv("RT_SETTLED_TILES")) c->settledEnvOn = atoi(e) != 0;
    if (const char *e = getenv("RT_PREFIX_REPLAY")) c->prefixEnvOn = atoi(e) != 0;
    if (const char *e = getenv("RT_ST_GEOM")) {        // "Kcube,Kplan,NB": measurement override of the shadow-table geometry
        int kc = 0, kp = 0, nb = 0;
        if (sscanf(e, "%d,%d,%d", &kc, &kp, &nb) == 3 && kc >= 4 && kc <= 128 && kp >= 4 && kp <= 256 && nb >= 1 && nb <= 128)
            c->stGeomSmall = c->stGeomLarge = RtShadowTabGeom{kc, kp, nb};
    }
    if (c->stream.create() != hipSuccess || c->evStart.create(hipEventDefault) != hipSuccess ||
        c->evStop.create(hipEventDefault) != hipSuccess || c->evScene.create(hipEventDisableTiming) != hipSuccess ||
        c->bloomUse.create() != hipSuccess || c->ssaoUse.create() != hipSuccess || c->resample.create() != hipSuccess || c->dRayCounter.grow(32) != hipSuccess) {
        rt_destroy(c);
        return RT_ERR_HIP;
    }
    c->sched.init(c->stream);
    c->present.init(deviceId);
    *out = c;
    return RT_OK;
}

int rt_destroy(rt_context *c) {
    if (!c) return RT_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    (void)c->sched.drain();            // the context's stream, the phase stream, every stream's last launch
    (void)c->bloomUse.drain();         // post passes on caller streams: the scratch they work in goes with the context
    (void)c->ssaoUse.drain();
    (void)c->resample.drain();         // the last launch that read the resampler's tables
    (void)c->jpegUse.drain();          // the last JPEG submit in the context's scratch
    (void)c->present.drain();          // frames on their way to the pinned buffers (and, before them, their packs)
    delete c;
    return RT_OK;
}

int rt_set_scene(rt_context *c, const void *objects, int nObj, const void *lights, int nLt) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (nObj < 0 || nLt < 0 || (nObj > 0 && !objects) || (nLt > 0 && !lights))
        return fail(c, RT_ERR_INVALID_ARG, "bad scene arguments");
    if (nObj > RT_MAX_OBJECTS || nLt > RT_MAX_LIGHTS) return fail(c, RT_ERR_TOO_LARGE, "scene exceeds RT_MAX_OBJECTS/RT_MAX_LIGHTS");
    HIP_TRY(c, hipSetDevice(c->device));
    // The reference re-specifies both SSBOs every frame whether or not anything moved (ImGUIManager.cpp:202, :338).  Identical
    // bytes leave the device scene, its compiled form and its shadow tables as they are (and the scheduler's view of "the same
    // frame as before" intact).
    const size_t objBytes = (size_t)nObj * RT_OBJECT_STRIDE, ltBytes = (size_t)nLt * RT_LIGHT_STRIDE;
    if (c->dCompiled && c->nObj == nObj && c->nLt == nLt && c->lastScene.size() == objBytes + ltBytes &&
        (objBytes == 0 || memcmp(c->lastScene.data(), objects, objBytes) == 0) &&
        (ltBytes == 0 || memcmp(c->lastScene.data() + objBytes, lights, ltBytes) == 0))
        return RT_OK;
    c->lastScene.clear();                  // (refilled at the end: a failed update must not look like the current scene)
    c->sceneGen++;
    c->firstHit.invalidate();              // changed bytes: the recorded first hits are another scene's (identical bytes keep them)
    c->accel.built = false;                // ... and so is the hierarchy, until rt_accel_scene_changed below has built this scene's
    HIP_TRY(c, c->dObjects.grow(objBytes));
    HIP_TRY(c, c->dLights.grow(ltBytes));
    HIP_TRY(c, c->dCompiled.grow(rt_compiled_total_f4(nObj, nLt)));
    // The scene buffers are about to be rewritten on the context's stream: order that behind the last launch of
    // EVERY stream frames have been issued on (one event per stream; a single shared event would only cover the
    // most recent one -- ADVICE r1).  The reference re-uploads its SSBOs every frame, so this is the common path.
    SCHED_TRY(c, waitForLaunches(c->stream));
    const int k = (int)(c->stageSeq++ & 1u);
    if (c->stageUsed[k]) HIP_TRY(c, hipEventSynchronize(c->evStage[k]));
    if (objBytes + ltBytes > c->hStage[k].cap) HIP_TRY(c, c->hStage[k].grow(objBytes + ltBytes < 65536 ? 65536 : objBytes + ltBytes));
    if (objBytes) memcpy(c->hStage[k], objects, objBytes);
    if (ltBytes) memcpy(c->hStage[k] + objBytes, lights, ltBytes);
    if (objBytes) HIP_TRY(c, hipMemcpyAsync(c->dObjects, c->hStage[k], objBytes, hipMemcpyHostToDevice, c->stream));
    if (ltBytes) HIP_TRY(c, hipMemcpyAsync(c->dLights, c->hStage[k] + objBytes, ltBytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, c->evStage[k].create(hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(c->evStage[k], c->stream));
    c->stageUsed[k] = true;
    HIP_TRY(c, rt_launch_compile_scene(c->dObjects, nObj, c->dLights, nLt, c->dCompiled, c->stream));
    bool pcss = false;            // a PCSS light: its blocker rays get a table of their own (the PCSS kernel instantiations read it)
    for (int i = 0; i < nLt; i++) {
        rt_light l;
        memcpy(&l, (const uint8_t *)lights + (size_t)i * RT_LIGHT_STRIDE, sizeof l);
        pcss = pcss || l.shadowType == 2;
    }
    // the lights' shadow tables of this scene (light-space candidate masks, rt_shadowtab.inc)
    c->shadowTabValid = false;
    if (nObj > 0 && nLt > 0 && nObj <= RT_ST_MAX_OBJECTS && nLt <= RT_ST_MAX_LIGHTS) {
        const RtShadowTabGeom &g = nObj <= 32 ? c->stGeomSmall : c->stGeomLarge;
        c->shadowTabBlocker = pcss;
        HIP_TRY(c, c->dShadowTab.grow(rt_shadowtab_dwords(g, nObj, nLt, pcss)));
        HIP_TRY(c, rt_launch_shadow_tables(c->dCompiled, nObj, nLt, c->dShadowTab, g, c->stream, c->stOnePhase, pcss));
        c->shadowTabValid = true;
    }
    RT_TRY(rt_accel_scene_changed(c, objects, nObj));    // rt_set_accel: the new scene's hierarchy, uploaded on the same stream
    HIP_TRY(c, hipEventRecord(c->evScene, c->stream));   // foreign streams order behind this (rt_render_to)
    try {
        c->lastScene.resize(objBytes + ltBytes);
        if (objBytes) memcpy(c->lastScene.data(), objects, objBytes);
        if (ltBytes) memcpy(c->lastScene.data() + objBytes, lights, ltBytes);
    } catch (...) {
        c->lastScene.clear();
    }
    c->nObj = nObj;
    c->nLt = nLt;
    c->anyPcss = pcss;
    return RT_OK;
}

int rt_set_noise(rt_context *c, const uint8_t *r8, int w, int h) {
    if (!c) return RT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    SCHED_TRY(c, drain());                 // frames on every stream read the texture
    c->texGen++;
    c->firstHit.invalidate();
    HIP_TRY(c, c->dNoise.release());
    c->noiseW = c->noiseH = 0;
    if (!r8) return RT_OK;
    if (w <= 0 || h <= 0) return fail(c, RT_ERR_INVALID_ARG, "noise size must be positive");
    HIP_TRY(c, c->dNoise.grow((size_t)w * h));
    HIP_TRY(c, hipMemcpy(c->dNoise, r8, (size_t)w * h, hipMemcpyHostToDevice));
    c->noiseW = w;
    c->noiseH = h;
    return RT_OK;
}

int rt_set_skybox(rt_context *c, const uint16_t *rgb16f, int size) {
    if (!c) return RT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    SCHED_TRY(c, drain());
    c->texGen++;
    c->firstHit.invalidate();
    HIP_TRY(c, c->dSky.release());
    c->skySize = 0;
    if (!rgb16f) return RT_OK;
    if (size <= 0) return fail(c, RT_ERR_INVALID_ARG, "skybox size must be positive");
    size_t bytes = (size_t)6 * size * size * 3 * sizeof(uint16_t);
    HIP_TRY(c, c->dSky.grow(bytes / sizeof(uint16_t)));
    HIP_TRY(c, hipMemcpy(c->dSky, rgb16f, bytes, hipMemcpyHostToDevice));
    c->skySize = size;
    return RT_OK;
}

int rt_render(rt_context *c, const rt_params *p) {
    if (!c) return RT_ERR_INVALID_ARG;
    int rc = validate_params(c, p);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    size_t npx = (size_t)p->regionW * p->regionH;
    if (!(c->dColor.holds(npx) && c->dPos.holds(npx) && c->dNormal.holds(npx))) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, c->dColor.grow(npx));
        HIP_TRY(c, c->dPos.grow(npx));
        HIP_TRY(c, c->dNormal.grow(npx));
    }
    c->surfW = p->regionW;
    c->surfH = p->regionH;
    return launch(c, p, c->dColor, c->dPos, c->dNormal, nullptr, c->stream, true);
}

int rt_render_to(rt_context *c, const rt_params *p, void *dColor, void *dPosition, void *dNormal, void *hipStream) {
    return render_on(c, p, dColor, dPosition, dNormal, hipStream, false);
}

int rt_render_into_image(rt_context *c, const rt_params *p, void *dColorImage, void *dPositionImage, void *dNormalImage, void *hipStream) {
    return render_on(c, p, dColorImage, dPositionImage, dNormalImage, hipStream, true);
}

// ---- ray queries (rt_query.inc).  They read the compiled scene, so they join the render launches' stream protocol: a
// foreign stream first waits for the last scene upload (caller_stream), and every launch records its stream's `last` event
// (recordLaunch), which rt_set_scene orders the next rewrite behind.  No scheduling state or timing event is touched.
int rt_trace_rays(rt_context *c, const void *dRays, size_t nRays, int mode, void *dOut, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (mode != RT_QUERY_CLOSEST && mode != RT_QUERY_ANY) return fail(c, RT_ERR_INVALID_ARG, "unknown query mode");
    if (!c->dCompiled) return fail(c, RT_ERR_INVALID_ARG, "rt_set_scene has not been called");
    if (nRays == 0) return RT_OK;
    if (!dRays || !dOut) return fail(c, RT_ERR_INVALID_ARG, "NULL ray or result pointer");
    if (((uintptr_t)dRays | (uintptr_t)dOut) & 15u) return fail(c, RT_ERR_INVALID_ARG, "ray and result pointers must be 16-byte aligned");
    if (nRays > kMaxLaunchItems) return fail(c, RT_ERR_TOO_LARGE, "too many rays in one call");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s;
    int rc = caller_stream(c, hipStream, &s);
    if (rc) return rc;
    if (c->accel.built) {
        const int lane = accel_lane(c->accel.desc);
        HIP_TRY(c, rt_launch_trace_rays_accel((const float4 *)dRays, nRays, c->dCompiled, c->accel.dev, mode == RT_QUERY_ANY, lane, dOut, s));
        c->accel.report.launchesAccel[lane]++;
    } else {
        HIP_TRY(c, rt_launch_trace_rays((const float4 *)dRays, nRays, c->dCompiled, c->nObj, mode == RT_QUERY_ANY, dOut, s));
        if (c->accel.on) c->accel.report.launchesBrute++;
    }
    SCHED_TRY(c, recordLaunch(s));
    return RT_OK;
}

int rt_camera_rays(rt_context *c, const rt_params *p, void *dRays, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    int rc = validate_params(c, p);
    if (rc) return rc;
    if (!dRays) return fail(c, RT_ERR_INVALID_ARG, "NULL ray pointer");
    if ((uintptr_t)dRays & 15u) return fail(c, RT_ERR_INVALID_ARG, "ray pointer must be 16-byte aligned");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s;
    if ((rc = caller_stream(c, hipStream, &s))) return rc;
    RtFrame f;
    build_frame(c, p, &f);
    HIP_TRY(c, rt_launch_camera_rays(f, c->dNoise, (float4 *)dRays, s));
    SCHED_TRY(c, recordLaunch(s));      // rt_set_noise drains it before freeing the texture
    return RT_OK;
}

// The adaptive loop's ray stage: the rays of listed image pixels.  Like rt_pick, only the camera, image size and ray fields of p
// matter, so p is validated with an identity window; like rt_camera_rays it reads the noise texture and records its launch.
int rt_camera_rays_at(rt_context *c, const rt_params *p, const void *dPixels, size_t n, void *dRays, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!p) return fail(c, RT_ERR_INVALID_ARG, "params is NULL");
    const rt_params q = identity_window(*p);
    int rc = validate_params(c, &q);
    if (rc) return rc;
    if (n == 0) return RT_OK;
    if (!dPixels || !dRays) return fail(c, RT_ERR_INVALID_ARG, "NULL pixel list or ray pointer");
    if ((uintptr_t)dPixels & 7u) return fail(c, RT_ERR_INVALID_ARG, "pixel list pointer must be 8-byte aligned");
    if ((uintptr_t)dRays & 15u) return fail(c, RT_ERR_INVALID_ARG, "ray pointer must be 16-byte aligned");
    if (n > kMaxLaunchItems) return fail(c, RT_ERR_TOO_LARGE, "too many pixels in one call");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s;
    if ((rc = caller_stream(c, hipStream, &s))) return rc;
    RtFrame f;
    build_frame(c, &q, &f);
    HIP_TRY(c, rt_launch_camera_rays_at(f, c->dNoise, (const uint2 *)dPixels, n, (float4 *)dRays, s));
    SCHED_TRY(c, recordLaunch(s));      // rt_set_noise drains it before freeing the texture
    return RT_OK;
}

// ---- ray shading (rt_shade.inc): the query stream protocol; it also reads the noise texture and the skybox, which
// rt_set_noise / rt_set_skybox / an installing rt_equirect_to_cubemap free only after draining every recorded stream.
int rt_shade_rays(rt_context *c, const rt_params *p, const void *dRays, const void *dPixels, size_t nRays, void *dColor,
                  void *dPosition, void *dNormal, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    int rc = validate_params(c, p);
    if (rc) return rc;
    if (!c->dCompiled) return fail(c, RT_ERR_INVALID_ARG, "rt_set_scene has not been called");
    if (!dPixels && nRays != (size_t)p->regionW * (size_t)p->regionH)
        return fail(c, RT_ERR_INVALID_ARG, "without pixels, nRays must equal regionW * regionH");
    if (nRays == 0) return RT_OK;
    if (!dRays || !dColor) return fail(c, RT_ERR_INVALID_ARG, "NULL ray or colour pointer");
    if (((uintptr_t)dRays | (uintptr_t)dColor | (uintptr_t)dPosition) & 15u)
        return fail(c, RT_ERR_INVALID_ARG, "ray, colour and position pointers must be 16-byte aligned");
    if (((uintptr_t)dPixels | (uintptr_t)dNormal) & 7u) return fail(c, RT_ERR_INVALID_ARG, "pixel and normal pointers must be 8-byte aligned");
    if (nRays > kMaxLaunchItems) return fail(c, RT_ERR_TOO_LARGE, "too many rays in one call");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s;
    if ((rc = caller_stream(c, hipStream, &s))) return rc;
    RtFrame f;
    build_frame(c, p, &f);
    // rt_set_accel_shading: the same kernel body over the tree.  The tree is read under the protocol above: this launch is
    // recorded on s, rt_set_scene / rt_set_accel rebuild behind waitForLaunches, and the buffer grows only after drain().
    if (c->accelShadeActive()) {
        const int lane = c->accelShade.lane;
        HIP_TRY(c, rt_launch_shade_rays_accel(f, c->dCompiled, c->accel.dev, lane, c->dNoise, c->dSky, (const float4 *)dRays,
                                              (const uint2 *)dPixels, nRays, (float4 *)dColor, (float4 *)dPosition, (uint2 *)dNormal, s));
        c->accelShade.launchesAccel[lane]++;
    } else {
        HIP_TRY(c, rt_launch_shade_rays(f, c->dCompiled, c->dNoise, c->dSky, (const float4 *)dRays, (const uint2 *)dPixels, nRays,
                                        (float4 *)dColor, (float4 *)dPosition, (uint2 *)dNormal, s));
        if (c->accelShade.on) c->accelShade.launchesBrute++;
    }
    SCHED_TRY(c, recordLaunch(s));
    return RT_OK;
}

int rt_pick(rt_context *c, const rt_params *p, int px, int py, rt_hit *hit) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!hit) return fail(c, RT_ERR_INVALID_ARG, "NULL hit pointer");
    if (!p) return fail(c, RT_ERR_INVALID_ARG, "params is NULL");
    const rt_params q = identity_window(*p);
    int rc = validate_params(c, &q);
    if (rc) return rc;
    if (px < 0 || py < 0 || px >= q.width || py >= q.height) return fail(c, RT_ERR_INVALID_ARG, "pixel outside the image");
    if (!c->dCompiled) return fail(c, RT_ERR_INVALID_ARG, "rt_set_scene has not been called");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->dPick.grow(2));
    HIP_TRY(c, c->hPick.grow(1));
    RtFrame f;
    build_frame(c, &q, &f);
    if (c->accel.built) {
        HIP_TRY(c, rt_launch_pick_accel(f, c->dNoise, c->dCompiled, c->accel.dev, px, py, c->dPick, c->stream));
        c->accel.report.launchesAccel[0]++;
    } else {
        HIP_TRY(c, rt_launch_pick(f, c->dNoise, c->dCompiled, px, py, c->dPick, c->stream));
        if (c->accel.on) c->accel.report.launchesBrute++;
    }
    HIP_TRY(c, hipMemcpyAsync(c->hPick, c->dPick, sizeof(rt_hit), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    memcpy(hit, c->hPick, sizeof(rt_hit));
    return RT_OK;
}

int rt_context_stream(rt_context *c, void **hipStream) {
    if (!c || !hipStream) return RT_ERR_INVALID_ARG;
    *hipStream = (void *)c->stream;
    return RT_OK;
}

int rt_sync(rt_context *c) {
    if (!c) return RT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

int rt_readback(rt_context *c, float *gColor, float *gPosition, uint16_t *gNormal) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!c->dColor || c->surfW <= 0 || c->surfH <= 0) return fail(c, RT_ERR_NO_SURFACES, "no rendered surfaces");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    size_t npx = (size_t)c->surfW * c->surfH;
    if (gColor) HIP_TRY(c, hipMemcpy(gColor, c->dColor, npx * sizeof(float4), hipMemcpyDeviceToHost));
    if (gPosition) HIP_TRY(c, hipMemcpy(gPosition, c->dPos, npx * sizeof(float4), hipMemcpyDeviceToHost));
    if (gNormal) HIP_TRY(c, hipMemcpy(gNormal, c->dNormal, npx * sizeof(uint2), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_get_surfaces(rt_context *c, void **dColor, void **dPosition, void **dNormal) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!c->dColor) return fail(c, RT_ERR_NO_SURFACES, "no rendered surfaces");
    if (dColor) *dColor = c->dColor;
    if (dPosition) *dPosition = c->dPos;
    if (dNormal) *dNormal = c->dNormal;
    return RT_OK;
}

int rt_last_kernel_ms(rt_context *c, float *ms) {
    if (!c || !ms) return RT_ERR_INVALID_ARG;
    if (!c->timed) return fail(c, RT_ERR_NO_SURFACES, "no timed render yet");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(c->evStop));
    HIP_TRY(c, hipEventElapsedTime(ms, c->evStart, c->evStop));
    return RT_OK;
}

// The instrumented builds of the render kernel (rt_launch_render's countMode): the frame into the caller's surfaces or, with
// none, into scratch that is freed again; the ray total and the diagnostics of rt_debug_stats_ex.  The launch never records
// or replays first hits and leaves the cached ones as they are (launch()).
int rt_count_rays_to(rt_context *c, const rt_params *p, int mode, void *dColor, void *dPosition, void *dNormal, uint64_t *rays) {
    if (!c || !rays) return RT_ERR_INVALID_ARG;
    *rays = 0;
    if (mode != 1 && mode != 2) return fail(c, RT_ERR_INVALID_ARG, "rt_count_rays_to: mode must be 1 (reference rays) or 2 (traced rays)");
    int rc = validate_params(c, p);
    if (rc) return rc;
    const bool own = !dColor && !dPosition && !dNormal;
    if (!own && (!dColor || !dPosition || !dNormal)) return fail(c, RT_ERR_INVALID_ARG, "rt_count_rays_to: all three surfaces or none");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t npx = (size_t)p->regionW * p->regionH;
    DevBuf<float4> col, pos;
    DevBuf<uint2> nrm;
    if (own) {
        hipError_t e = col.grow(npx);
        if (e == hipSuccess) e = pos.grow(npx);
        if (e == hipSuccess) e = nrm.grow(npx);
        if (e != hipSuccess) return fail(c, RT_ERR_HIP, "hipMalloc (ray count scratch)", e);
        dColor = col.ptr;
        dPosition = pos.ptr;
        dNormal = nrm.ptr;
    }
    int group = 1;
    if (hipMemsetAsync(c->dRayCounter, 0, 32 * sizeof(unsigned long long), c->stream) != hipSuccess) rc = RT_ERR_HIP;
    if (!rc) rc = launch(c, p, (float4 *)dColor, (float4 *)dPosition, (uint2 *)dNormal, c->dRayCounter, c->stream, false, mode, false, &group);
    unsigned long long v[32] = {};
    if (!rc && (hipStreamSynchronize(c->stream) != hipSuccess ||
                hipMemcpy(v, c->dRayCounter, sizeof v, hipMemcpyDeviceToHost) != hipSuccess))
        rc = fail(c, RT_ERR_HIP, "ray counter readback");
    v[31] = (unsigned long long)group;       // written here, not by the kernel: the launched instantiation's blocker group
    *rays = v[0];
    for (int k = 0; k < 32; k++) c->lastStats[k] = v[k];
    return rc;
}
int rt_count_rays(rt_context *c, const rt_params *p, uint64_t *rays) { return rt_count_rays_to(c, p, 1, nullptr, nullptr, nullptr, rays); }
int rt_count_rays_traced(rt_context *c, const rt_params *p, uint64_t *rays) { return rt_count_rays_to(c, p, 2, nullptr, nullptr, nullptr, rays); }

int rt_set_variant(rt_context *c, int variant) {
    if (!c) return RT_ERR_INVALID_ARG;
    // another kernel, or first-hit reuse (bit 10, 0x400 = off), its settled tiles (bit 11, 0x800 = off) or its prefix replay
    // (bit 12, 0x1000 = off) switched: the next frame is a normal one
    const bool reuseOn = (variant & 0x400) == 0, settledOn = (variant & 0x800) == 0, prefixOn = (variant & 0x1000) == 0;
    if ((variant & 0xff) != c->variant || reuseOn != c->firstHit.variantOn || settledOn != c->settledVariantOn || prefixOn != c->prefixVariantOn)
        c->firstHit.invalidate();
    c->firstHit.variantOn = reuseOn;
    c->settledVariantOn = settledOn;
    c->prefixVariantOn = prefixOn;
    c->variant = variant & 0xff;
    c->sched.setMode(variant);         // bits 8 and 9: the tile order
    return RT_OK;
}

int rt_debug_first_hit(rt_context *c, uint64_t counts[3]) {
    if (!c || !counts) return RT_ERR_INVALID_ARG;
    for (int k = 0; k < 3; k++) counts[k] = c->firstHit.counts[k];
    return RT_OK;
}

// The flags of the cached window, read back after everything in flight has ended (a recording frame may still be writing them).
static int settled_flags(rt_context *c, std::vector<uint8_t> *flags) {
    flags->clear();
    if (!c->firstHit.valid || !c->dFirstHit.ptr) return RT_OK;
    const rt_params &p = c->firstHit.cached.p;
    const RtFirstHitLayout l = rt_first_hit_layout(p.regionW, p.regionH);
    if (!c->dFirstHit.holds(l.bytes)) return RT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->sched.drain());
    flags->resize(l.tiles);
    HIP_TRY(c, hipMemcpy(flags->data(), c->dFirstHit.ptr + l.flags, l.tiles, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_debug_settled_tiles(rt_context *c, uint64_t out[2]) {
    if (!c || !out) return RT_ERR_INVALID_ARG;
    out[0] = out[1] = 0;
    std::vector<uint8_t> flags;
    RT_TRY(settled_flags(c, &flags));
    out[0] = flags.size();
    for (uint8_t v : flags) out[1] += rt_prefix_flag_settled(v);
    return RT_OK;
}

int rt_debug_prefix_tiles(rt_context *c, uint64_t out[9]) {
    if (!c || !out) return RT_ERR_INVALID_ARG;
    for (int k = 0; k < 9; k++) out[k] = 0;
    std::vector<uint8_t> flags;
    RT_TRY(settled_flags(c, &flags));
    for (uint8_t v : flags) {
        const int k = rt_prefix_flag_depth(v);
        out[rt_prefix_flag_settled(v) ? 0 : 1 + (k < RT_PREFIX_CAP ? k : RT_PREFIX_CAP)]++;
    }
    return RT_OK;
}

int rt_debug_settled_map(rt_context *c, uint8_t *flags, size_t n) {
    if (!c || (!flags && n)) return RT_ERR_INVALID_ARG;
    std::vector<uint8_t> have;
    RT_TRY(settled_flags(c, &have));
    if (n != have.size()) return fail(c, RT_ERR_INVALID_ARG, "rt_debug_settled_map: n is not the cached window's tile count (rt_debug_settled_tiles)");
    for (size_t i = 0; i < n; i++) flags[i] = rt_prefix_flag_settled(have[i]) ? 1 : 0;      // (the byte also carries the prefix depth)
    return RT_OK;
}

int rt_debug_stats(rt_context *c, uint64_t out[4]) {
    if (!c || !out) return RT_ERR_INVALID_ARG;
    for (int k = 0; k < 4; k++) out[k] = c->lastStats[k];
    return RT_OK;
}

int rt_debug_stats_ex(rt_context *c, uint64_t out[32]) {
    if (!c || !out) return RT_ERR_INVALID_ARG;
    for (int k = 0; k < 32; k++) out[k] = c->lastStats[k];
    return RT_OK;
}

int rt_debug_shadow_tables(rt_context *c, uint32_t *out, size_t capDwords, size_t *nDwords, int *wordsPerCell) {
    if (!c || !nDwords) return RT_ERR_INVALID_ARG;
    *nDwords = 0;
    if (wordsPerCell) *wordsPerCell = 0;
    if (!c->shadowTabValid) return RT_OK;
    const RtShadowTabGeom &g = c->nObj <= 32 ? c->stGeomSmall : c->stGeomLarge;
    const size_t n = rt_shadowtab_table_dwords(g, c->nObj, c->nLt, c->shadowTabBlocker);      // (the builder's scratch behind the tables is not part of them)
    *nDwords = n;
    if (wordsPerCell) *wordsPerCell = rt_shadowtab_words(c->nObj);
    if (!out) return RT_OK;
    if (capDwords < n) return fail(c, RT_ERR_TOO_LARGE, "buffer smaller than the shadow tables");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out, c->dShadowTab, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_debug_predicted_classes(rt_context *c, uint8_t *out, int cap, int *nTiles) {
    if (!c || !out || cap < 0 || !nTiles) return RT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    SCHED_TRY(c, predictedClasses(out, cap, nTiles));
    return RT_OK;
}

int rt_debug_tile_costs(rt_context *c, unsigned *out, int cap, int *nTiles, int *tilesX) {
    if (!c || !out || cap < 0 || !nTiles || !tilesX) return RT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    SCHED_TRY(c, tileCosts(out, cap, nTiles, tilesX));
    return RT_OK;
}

int rt_debug_tile_order(rt_context *c, uint32_t *out, int cap, int *nTiles, int *policy) {
    if (!c || !out || cap < 0 || !nTiles || !policy) return RT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    SCHED_TRY(c, tileOrder(out, cap, nTiles, policy));
    return RT_OK;
}

int rt_debug_lpt_sort(rt_context *c, uint32_t *costs, int nTiles, uint32_t *order, uint32_t *accum) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!costs || !order) return fail(c, RT_ERR_INVALID_ARG, "rt_debug_lpt_sort: NULL costs or order");
    if (nTiles < 1 || nTiles > (1 << 20)) return fail(c, RT_ERR_INVALID_ARG, "rt_debug_lpt_sort: nTiles outside [1, 2^20]");
    HIP_TRY(c, hipSetDevice(c->device));
    SCHED_TRY(c, lptSortOf(costs, nTiles, order, accum));
    return RT_OK;
}

int rt_debug_split_tiles(rt_context *c, uint8_t *out, int cap, int *nTiles) {
    if (!c || !out || cap < 0 || !nTiles) return RT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    SCHED_TRY(c, splitTiles(out, cap, nTiles));
    return RT_OK;
}

int rt_debug_split_plan(rt_context *c, const uint32_t *order, const uint32_t *costs, int nTiles, uint32_t waveSlots, int depth, int nLt, int forceParts,
                        const uint8_t *prevParts, uint8_t *parts, uint32_t *slot, uint32_t *extra, uint32_t counts[2]) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!order || !costs || !parts || !slot || !extra || !counts) return fail(c, RT_ERR_INVALID_ARG, "rt_debug_split_plan: NULL array");
    if (nTiles < 1 || nTiles > (1 << 20)) return fail(c, RT_ERR_INVALID_ARG, "rt_debug_split_plan: nTiles outside [1, 2^20]");
    if (depth < 0 || depth > RT_MAX_DEPTH || nLt < 0 || nLt > 1024 || forceParts < 0 || forceParts > RT_SPLIT_MAX_PARTS || forceParts == 1)
        return fail(c, RT_ERR_INVALID_ARG, "rt_debug_split_plan: depth, nLt or forceParts out of range");
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<unsigned short> slots((size_t)nTiles);
    SCHED_TRY(c, splitPlanOf(order, costs, nTiles, waveSlots, depth, nLt, forceParts, prevParts, parts, slots.data(), extra, counts));
    for (int i = 0; i < nTiles; i++) slot[i] = slots[(size_t)i];
    return RT_OK;
}

const char *rt_last_error(rt_context *c) { return c ? c->err.c_str() : "NULL context"; }

int rt_debug_mesa_math(const float *in, float *out, int n) {
    if (!in || !out || n < 0) return RT_ERR_INVALID_ARG;
    for (int i = 0; i < n; i++) {
        out[4 * i] = rtm::sin_(in[i]);
        out[4 * i + 1] = rtm::cos_(in[i]);
        out[4 * i + 2] = rtm::tan_(in[i]);
        out[4 * i + 3] = rtm::exp_(in[i]);
    }
    return RT_OK;
}

// The device-side primitives on caller-supplied operands (rt_kernels.hip).  It reads nothing the context owns, so it takes
// no part in the scene streams' protocol: ordered on the given stream like the post passes.
int rt_debug_device_math(rt_context *c, int op, const void *dIn, void *dOut, size_t n, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (op < 0 || op >= RT_DM_OP_COUNT) return fail(c, RT_ERR_INVALID_ARG, "unknown device math op");
    if (n == 0) return RT_OK;
    if (!dIn || !dOut) return fail(c, RT_ERR_INVALID_ARG, "NULL input or output pointer");
    if (((uintptr_t)dIn | (uintptr_t)dOut) & 15u) return fail(c, RT_ERR_INVALID_ARG, "input and output pointers must be 16-byte aligned");
    if (n > kMaxLaunchItems) return fail(c, RT_ERR_TOO_LARGE, "too many records in one call");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = stream_or_own(c, hipStream);
    HIP_TRY(c, rt_launch_device_math(op, (const uint4 *)dIn, (uint4 *)dOut, n, s));
    return RT_OK;
}

}  // extern "C"
