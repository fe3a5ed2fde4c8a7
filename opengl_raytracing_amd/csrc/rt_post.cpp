// rt_post.cpp -- the post passes' entry points of the C ABI (include/rt_mi355.h has the contract of each): the TAA resolve,
// bloom, SSAO and its blur, the equirectangular-to-cubemap conversion, and rt_frame, which drives the render and these passes
// through the public ABI like any caller.  The kernels are rt_post.hip's.  Each entry point keeps its own refusal texts
// (tests/test_post_refusals.py pins them); none is word for word an rt_args.h rule.
#include "rt_context.h"
#include "rt_post.h"

extern "C" {

int rt_taa_resolve(rt_context *c, const void *dCurrent, const void *dHistory, const void *dNormal, void *dOut, int width,
                   int height, float blendFactor, float jitterX, float jitterY, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!dCurrent || !dHistory || !dNormal || !dOut || width <= 0 || height <= 0)
        return fail(c, RT_ERR_INVALID_ARG, "bad rt_taa_resolve arguments");
    if (dOut == dCurrent || dOut == dHistory) return fail(c, RT_ERR_INVALID_ARG, "rt_taa_resolve cannot run in place");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = stream_or_own(c, hipStream);
    HIP_TRY(c, rt_launch_taa_resolve(dCurrent, dHistory, dNormal, dOut, width, height, blendFactor, jitterX, jitterY, s));
    return RT_OK;
}

int rt_bloom(rt_context *c, const void *dScene, void *dOut, int width, int height, float threshold, float strength,
             int iterations, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!dScene || !dOut || width <= 0 || height <= 0 || iterations < 0) return fail(c, RT_ERR_INVALID_ARG, "bad rt_bloom arguments");
    if (dOut == dScene) return fail(c, RT_ERR_INVALID_ARG, "rt_bloom cannot run in place");     // the fused passes read neighbouring tiles' scene texels
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = stream_or_own(c, hipStream);
    const size_t npx = (size_t)width * height;
    if (!(c->dBloom[0].holds(npx) && c->dBloom[1].holds(npx))) {
        HIP_TRY(c, c->bloomUse.drain());       // the last pass in the old targets, on whichever stream it ran
        HIP_TRY(c, c->dBloom[0].grow(npx));
        HIP_TRY(c, c->dBloom[1].grow(npx));
    }
    HIP_TRY(c, c->bloomUse.acquire(s));
    HIP_TRY(c, rt_launch_bloom(dScene, c->dBloom[0], c->dBloom[1], dOut, width, height, threshold, strength, iterations, s));
    HIP_TRY(c, c->bloomUse.release(s));
    return RT_OK;
}

int rt_equirect_to_cubemap(rt_context *c, const float *hEquirectRGB, int width, int height, int size, void *dFacesOut,
                           int install) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!hEquirectRGB || width <= 0 || height <= 0 || size <= 0) return fail(c, RT_ERR_INVALID_ARG, "bad rt_equirect_to_cubemap arguments");
    if (!dFacesOut && !install) return fail(c, RT_ERR_INVALID_ARG, "nowhere to put the faces");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const size_t npx = (size_t)width * height, faceBytes = (size_t)6 * size * size * 3 * sizeof(uint16_t);
    DevBuf<float> rgb;
    DevBuf<uint2> tex;                  // rgba16f
    DevBuf<uint16_t> faces;
    hipError_t e = rgb.grow(npx * 3);
    if (e == hipSuccess) e = tex.grow(npx);
    if (e == hipSuccess) e = faces.grow(faceBytes / sizeof(uint16_t));
    if (e == hipSuccess) e = hipMemcpyAsync(rgb, hEquirectRGB, npx * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = rt_launch_equirect_to_cubemap(rgb, tex, width, height, size, faces, c->stream);
    if (e == hipSuccess && dFacesOut) e = hipMemcpyAsync(dFacesOut, faces, faceBytes, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, RT_ERR_HIP, "rt_equirect_to_cubemap", e);
    if (install) {
        SCHED_TRY(c, drain());          // frames and shades on every stream read the old skybox
        c->texGen++;
        c->firstHit.invalidate();
        c->dSky.swap(faces);            // (the old one goes with `faces`)
        c->skySize = size;
    }
    return RT_OK;
}

int rt_ssao(rt_context *c, const void *dPosition, const void *dNormal, void *dOut, int width, int height, const float *hNoise,
            int noiseW, int noiseH, const float *hSamples, const float *hProjection, const float *hView, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!dPosition || !dNormal || !dOut || !hNoise || !hSamples || !hProjection || !hView || width <= 0 || height <= 0)
        return fail(c, RT_ERR_INVALID_ARG, "bad rt_ssao arguments");
    if (noiseW <= 0 || noiseH <= 0 || noiseW * noiseH > 16) return fail(c, RT_ERR_TOO_LARGE, "rotation texture larger than 16 texels");
    if (dOut == dPosition || dOut == dNormal) return fail(c, RT_ERR_INVALID_ARG, "rt_ssao cannot run in place");   // samples read other pixels' G-buffer
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = stream_or_own(c, hipStream);
    const size_t npx = (size_t)width * height;
    if (!c->dSsaoDepth.holds(npx)) {
        HIP_TRY(c, c->ssaoUse.drain());        // the last pass that read the old plane, on whichever stream it ran
        HIP_TRY(c, c->dSsaoDepth.grow(npx));
    }
    HIP_TRY(c, c->ssaoUse.acquire(s));
    HIP_TRY(c, rt_launch_ssao(dPosition, dNormal, c->dSsaoDepth, dOut, width, height, hNoise, noiseW, noiseH, hSamples, hProjection,
                              hView, s));
    HIP_TRY(c, c->ssaoUse.release(s));
    return RT_OK;
}

int rt_ssao_blur(rt_context *c, const void *dIn, void *dOut, int width, int height, int horizontal, void *hipStream) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!dIn || !dOut || width <= 0 || height <= 0) return fail(c, RT_ERR_INVALID_ARG, "bad rt_ssao_blur arguments");
    if (dIn == dOut) return fail(c, RT_ERR_INVALID_ARG, "rt_ssao_blur cannot run in place");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = stream_or_own(c, hipStream);
    HIP_TRY(c, rt_launch_ssao_blur(dIn, dOut, width, height, horizontal, s));
    return RT_OK;
}

int rt_frame(rt_context *c, const rt_params *p, const rt_frame_desc *d, void *dDisplay) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!d) return fail(c, RT_ERR_INVALID_ARG, "frame description is NULL");
    if (d->enableAO && (!d->aoSamples || !d->aoNoise)) return fail(c, RT_ERR_INVALID_ARG, "AO needs its kernel samples and rotation texture");
    if (d->bloomIterations < 0) return fail(c, RT_ERR_INVALID_ARG, "bloomIterations < 0");
    int rc = validate_params(c, p);
    if (rc) return rc;
    if (p->x0 != 0 || p->y0 != 0 || p->regionW != p->width || p->regionH != p->height || p->stripCycleRows != 0 || p->stripCount != 1)
        return fail(c, RT_ERR_INVALID_ARG, "rt_frame renders the whole image on one device");
    const int W = p->width, H = p->height;
    const size_t npx = (size_t)W * H;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!(c->dFrameAO[0].holds(npx) && c->dFrameAO[1].holds(npx) && c->dHistory[0].holds(npx) && c->dHistory[1].holds(npx) &&
          c->dFrameDisplay.holds(npx))) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (int k = 0; k < 2; k++) {
            HIP_TRY(c, c->dFrameAO[k].grow(npx));
            HIP_TRY(c, c->dHistory[k].grow(npx));
        }
        HIP_TRY(c, c->dFrameDisplay.grow(npx));
        c->frameW = c->frameH = 0;
    }
    if (c->frameW != W || c->frameH != H) {      // new size: the history starts as zeros (glTexImage2D(..., nullptr))
        HIP_TRY(c, hipMemsetAsync(c->dHistory[0], 0, npx * sizeof(float4), c->stream));
        HIP_TRY(c, hipMemsetAsync(c->dHistory[1], 0, npx * sizeof(float4), c->stream));
        c->frameW = W;
        c->frameH = H;
        c->lastHistory = -1;
    }
    rc = rt_render(c, p);                                                   // :155-182
    if (rc) return rc;
    c->frameAOValid = false;
    if (d->enableAO) {                                                      // :185-187, AO.cpp:86-117
        float view[16], proj[16];
        rc = rt_camera_matrices(p->camPos, p->camDir, p->camUp, p->fovDeg, (float)W / (float)H, view, proj);
        if (rc) return fail(c, rc, "rt_camera_matrices");
        rc = rt_ssao(c, c->dPos, c->dNormal, c->dFrameAO[0], W, H, d->aoNoise, 4, 4, d->aoSamples, proj, view, nullptr);
        if (rc) return rc;
        rc = rt_ssao_blur(c, c->dFrameAO[0], c->dFrameAO[1], W, H, 0, nullptr);   // `horizontal` is never set upstream
        if (rc) return rc;
        c->frameAOValid = true;
    }
    rc = rt_bloom(c, c->dColor, dDisplay ? dDisplay : (void *)c->dFrameDisplay, W, H, d->bloomThreshold, d->bloomStrength,
                  d->bloomIterations, nullptr);                             // :189-228
    if (rc) return rc;
    if (d->enableTAA) {                                                     // :231-258
        const int cur = ((p->frameCount % 2) + 2) % 2;
        float jx, jy;
        rc = rt_taa_jitter(p->frameCount, W, H, &jx, &jy);
        if (rc) return fail(c, rc, "rt_taa_jitter");
        rc = rt_taa_resolve(c, c->dColor, c->dHistory[1 - cur], c->dNormal, c->dHistory[cur], W, H, d->taaBlendFactor, jx, jy, nullptr);
        if (rc) return rc;
        c->lastHistory = cur;
    }
    return RT_OK;
}

int rt_frame_surfaces(rt_context *c, void **dColor, void **dPosition, void **dNormal, void **dAO, void **dHistory) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (dColor) *dColor = c->dColor;
    if (dPosition) *dPosition = c->dPos;
    if (dNormal) *dNormal = c->dNormal;
    if (dAO) *dAO = c->frameAOValid ? c->dFrameAO[1] : nullptr;
    if (dHistory) *dHistory = c->lastHistory >= 0 ? c->dHistory[c->lastHistory] : nullptr;
    return RT_OK;
}

}  // extern "C"
