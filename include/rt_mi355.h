/*
 * rt_mi355.h -- C ABI of librt_mi355.so: the MI355X (gfx950) replacement for the
 * reference's ray-tracing compute dispatch.
 *
 * The reference has no FFI; its seam is the GL call sequence in
 * ForwardShadingPipline::Render() (/root/reference/src/ForwardShadingPipeline.cpp:155-182):
 * upload two SSBO byte arrays, set the uniforms, bind the cubemap, glDispatchCompute,
 * glMemoryBarrier -- after which three textures hold the result.  Every entry point
 * below names the reference call(s) it stands in for.  Plain pointers and sizes only;
 * no torch / STL types cross this boundary.  All functions return 0 on success or a
 * negative rt_status; nothing throws or aborts across the ABI.
 *
 * Threading: a context is owned by one thread at a time (the reference likewise has
 * one GL context on one thread).  Multi-GPU = one context per device / process.
 */
#ifndef RT_MI355_H
#define RT_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_OBJECT_STRIDE 176 /* sizeof(Object), /root/reference/src/Object.h:13-21 */
#define RT_LIGHT_STRIDE 96   /* sizeof(Light),  /root/reference/src/Light.h:7-20  */
/* The shader's SSBOs are runtime-sized arrays whose lengths come from uniforms (raytracingCs.glsl:65-73); the default kernel
 * takes any count up to these sanity caps.  The exhaustive cross-check kernel (rt_set_variant 0) stages the whole scene in LDS
 * and refuses scenes beyond RT_EXHAUSTIVE_MAX_* with RT_ERR_TOO_LARGE at render time. */
#define RT_MAX_OBJECTS 65536
#define RT_MAX_LIGHTS 4096
#define RT_EXHAUSTIVE_MAX_OBJECTS 512   /* 512 * 160 B = 80 KiB of the CU's 160 KiB LDS */
#define RT_EXHAUSTIVE_MAX_LIGHTS 64

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID_ARG = -1,
    RT_ERR_NO_DEVICE = -2,   /* no HIP device / HIP runtime error on create */
    RT_ERR_HIP = -3,         /* a HIP call failed; see rt_last_error */
    RT_ERR_TOO_LARGE = -4,   /* scene exceeds RT_MAX_OBJECTS / RT_MAX_LIGHTS (or RT_EXHAUSTIVE_MAX_* under variant 0) */
    RT_ERR_NO_SURFACES = -5, /* readback before any render */
    RT_ERR_PARSE = -6
} rt_status;

/* Host mirror of the std430 records (offsets asserted below).
 * The ABI takes raw bytes; these structs exist so C/C++ callers can fill them. */
typedef struct rt_material { /* /root/reference/src/Material.h:11-23 */
    int32_t type;            /* never read by the shader */
    int32_t _pad0[3];
    float albedo[3];
    float metallic;
    float roughness;
    float diffuseStrength;
    float ior;
    float transparency;
    float specular;          /* never read by the shader */
    float subsurfaceScatter;
    int32_t _pad1[2];
    float subsurfaceColor[3];
    float scatterDistance;
} rt_material;

typedef struct rt_object { /* /root/reference/src/Object.h:13-21 */
    int32_t type;          /* 0 sphere, 1 plane */
    int32_t _pad0[3];
    float position[3];
    float radius;
    float normal[3];
    int32_t _pad1;
    float size[2];
    int32_t _pad2[2];
    rt_material material;
    float boundsMin[3];
    int32_t _pad3;
    float boundsMax[3];
    int32_t _pad4;
} rt_object;

typedef struct rt_light { /* /root/reference/src/Light.h:7-20 */
    int32_t type;         /* 0 point, 1 directional, 2 area */
    int32_t _pad0[3];
    float position[3];
    int32_t _pad1;
    float direction[3];
    int32_t _pad2;
    float color[3];
    float intensity;
    float radius;         /* dead in the shader */
    int32_t samples;      /* dead in the shader */
    float shadowSoftness;
    int32_t shadowType;   /* 0 none, 1 PCF, 2 PCSS */
    int32_t pcfSamples;
    float lightSize;
    float angularRadius;  /* dead in the shader */
    int32_t _pad3;
} rt_light;

/* The shader's uniform block (raytracingCs.glsl:72-89; uploaded by name at
 * ForwardShadingPipeline.cpp:155-166) + imageSize(outputImage) (:200) + the render
 * window.  Layout is shared with oracle/rt_oracle.h's orc_params. */
typedef struct rt_params {
    float camPos[3], camDir[3], camUp[3], camRight[3];
    float fovDeg;         /* degrees; Camera::FOV */
    float focalLength;    /* shader default 1.0 (never uploaded by the reference) */
    float maxRayDistance; /* shader default 114514.0 (never uploaded) */
    float noiseScale[2];  /* reference uploads 1/1024 */
    int32_t frameCount;
    int32_t useSkybox;
    int32_t maxRayDepth;  /* #define MAX_RAY_DEPTH (3 as shipped) */
    int32_t width, height;/* full image size: uv depends on it even for a window */
    /* Window rendered by this call, in local-row space.  The output surfaces are
     * regionW x regionH, row-major, row 0 = bottom (GL origin). */
    int32_t x0, y0, regionW, regionH;
    /* Interleaved row strips for multi-GPU tiling: local row ly is image row
     * ((ly / stripRows) * stripCount + stripIndex) * stripRows + ly % stripRows.
     * {1,1,0} is the identity (single GPU). */
    int32_t stripRows, stripCount, stripIndex;
    int32_t reserved0;
    /* Unequal strips (a rank that owns stripRows rows out of every stripCycleRows, starting at
     * stripOffsetRows): when stripCycleRows > 0 local row ly is image row
     * (ly / stripRows) * stripCycleRows + stripOffsetRows + ly % stripRows
     * and stripCount / stripIndex are ignored.  0 = the equal-strip rule above, which is the same
     * formula with stripCycleRows = stripRows * stripCount, stripOffsetRows = stripIndex * stripRows. */
    int32_t stripCycleRows, stripOffsetRows;
} rt_params;

typedef struct rt_context rt_context;

/* ---- lifetime: ForwardShadingPipline::Init() / dtor (ForwardShadingPipeline.cpp:6-20,
 *      .h:38-48): shader "compile" + stream + timing events on HIP device deviceId. */
int rt_create(rt_context **out, int deviceId);
int rt_destroy(rt_context *ctx);

/* ---- SSBO::update() + LightSSBO::update() (/root/reference/src/SSBO.h:16-23,
 *      LightSSBO.h:16-25): copies nObj*176 + nLt*96 bytes; caller keeps ownership; cheap
 *      enough to call every frame as the reference does (ImGUIManager.cpp:202,338). */
int rt_set_scene(rt_context *ctx, const void *objects, int nObj, const void *lights, int nLt);

/* ---- InitBlueNoiseTex (ForwardShadingPipeline.cpp:39-49): R8 texels, NEAREST/REPEAT.
 *      NULL = the shipped behaviour (sampler reads 0). */
int rt_set_noise(rt_context *ctx, const uint8_t *r8, int w, int h);

/* ---- glBindTexture(GL_TEXTURE_CUBE_MAP, ...) (ForwardShadingPipeline.cpp:167-170):
 *      6 faces (+X,-X,+Y,-Y,+Z,-Z) of size^2 RGB fp16, the format
 *      TextureLoader.cpp:140-147 allocates.  NULL unbinds. */
int rt_set_skybox(rt_context *ctx, const uint16_t *rgb16f, int size);

/* ---- glDispatchCompute + glMemoryBarrier (ForwardShadingPipeline.cpp:175-180).
 *      Asynchronous on the context's stream; renders into context-owned surfaces
 *      (outputImage rgba32f, gPosition rgba32f, gNormal rgba16f; raytracingCs.glsl:61-63). */
int rt_render(rt_context *ctx, const rt_params *p);

/* Same, into caller-provided DEVICE surfaces (regionW*regionH*16, *16, *8 bytes) on a
 * caller-provided hipStream_t (NULL = the context's stream).  Used for interop and for
 * the multi-GPU strip buffers that RCCL gathers. */
int rt_render_to(rt_context *ctx, const rt_params *p, void *dColor, void *dPosition,
                 void *dNormal, void *hipStream);

/* Same dispatch, but the three surfaces are WHOLE width x height images and every pixel of the rendered window (p->x0.., the
 * strip mapping) is stored at its image position (row-major, row 0 = bottom).  Several contexts -- one per GPU of a node, each
 * rendering its interleaved strips -- can thus fill ONE frame in place: on peer-mapped devices the stores of the other GPUs go
 * straight over xGMI into the frame's memory (rt_mgpu_render below does exactly that).  Pixels outside the image are skipped. */
int rt_render_into_image(rt_context *ctx, const rt_params *p, void *dColorImage, void *dPositionImage, void *dNormalImage,
                         void *hipStream);
/* The context's own hipStream_t (the stream rt_render / rt_set_scene use). */
int rt_context_stream(rt_context *ctx, void **hipStream);

/* ---- glFinish (PerformanceProfiler.cpp:51). */
int rt_sync(rt_context *ctx);

/* ---- glGetTexImage equivalents: host copies of the last rt_render's surfaces.
 *      Any pointer may be NULL. gNormal is 4 x fp16 per pixel (round-toward-zero). */
int rt_readback(rt_context *ctx, float *gColor, float *gPosition, uint16_t *gNormal);

/* Device pointers of the context-owned surfaces of the last rt_render. */
int rt_get_surfaces(rt_context *ctx, void **dColor, void **dPosition, void **dNormal);

/* ---- PerformanceProfiler Begin/EndGPUSection(RayTracing)
 *      (ForwardShadingPipeline.cpp:172-182, PerformanceProfiler.cpp:23-31): duration of
 *      the last render kernel from hipEvents on the launch stream; synchronises. */
int rt_last_kernel_ms(rt_context *ctx, float *ms);

/* Exact number of intersectObjects calls ("rays") for this frame,
 * counted by an instrumented build of the same kernel.  Synchronises. */
int rt_count_rays(rt_context *ctx, const rt_params *p, uint64_t *rays);
/* Rays the PRODUCTION kernel actually traverses for this frame: the same instrumented build, but keeping the
 * skips the timed kernel applies to rays whose result provably cannot reach a pixel (shadow / PCSS-blocker rays of
 * lanes whose light term is +-0 or NaN for every finite shadow value, blocker rays after the first blocker; DESIGN.md
 * section 4 items 6-8).  <= rt_count_rays; equal for variant 0.  Synchronises. */
int rt_count_rays_traced(rt_context *ctx, const rt_params *p, uint64_t *rays);
/* Both of them, with the instrumented build's frame made visible.  mode = 1 counts the reference's rays (rt_count_rays), mode = 2
 * the traced ones (rt_count_rays_traced); any other mode is refused.  dColor / dPosition / dNormal are DEVICE surfaces sized like
 * rt_render_to's (regionW*regionH*16, *16, *8 bytes) that receive the frame the instrumented launch renders -- the same bits as
 * rt_render_to's in both modes, which is what makes the skipped rays provably dead -- or all three NULL: the frame then goes into
 * scratch that is freed again.  Runs on the context's stream and synchronises.  Never records or replays first hits, and leaves
 * the cached ones, rt_debug_first_hit and rt_debug_prefix_tiles as they were.
 *
 * The traced count, exactly.  Primary, bounce and subsurface rays always count.  Per hit point and light with shadowType 1 or 2:
 *   lit = pcfSamples < 1 (the shadow factor is 0/0 then: nothing is skipped), or otherwise both
 *         max(dot(N, normalize(lightDir)), 0) > 0 and some channel of (color * attenuation) * intensity neither +-0 nor NaN;
 *   an unlit point traces no shadow ray for that light;
 *   a lit point under PCSS traces its 16 blocker rays in groups of G: a group is traced whole if no blocker was found before its
 *         first ray, and no group after that.  G is the launched kernel's blocker rays per traversal: RT_PK_BLOCKER_GROUP (4) in
 *         every packet kernel of a scene with a PCSS light, 1 otherwise; rt_debug_stats_ex reports it in out[31];
 *   a lit point traces the PCF rays the reference traces (pcfSamples each; under PCSS only where a blocker was found).
 * Variant 0 ignores the mode: its traced count is the reference count. */
int rt_count_rays_to(rt_context *ctx, const rt_params *p, int mode, void *dColor, void *dPosition, void *dNormal, uint64_t *rays);

/* Kernel variant: 1 (default) = wavefront-packet kernel (packet culling, scalar-fed traversal),
 * 0 = exhaustive per-lane loop over all objects.  Both produce bit-identical surfaces; the switch
 * exists for A/B measurements and as a cross-check in the tests.  Adding 0x100
 * disables the cost-feedback tile order of the packet kernel (frame k's measured tile costs give
 * frame k+1's longest-first workgroup order; scheduling only, no pixel depends on it). */
int rt_set_variant(rt_context *ctx, int variant);

/* First-hit reuse (default kernel, on unless the variant carries 0x400 or RT_FIRST_HIT_REUSE=0 was set at rt_create): while
 * the scene, the textures and every rt_params field stay what they were -- frameCount may advance as long as no noise texture
 * is loaded -- the second such frame also records every pixel's first hit and direct lighting, and the following ones replay
 * them instead of tracing depth 0 again.  The surfaces are the same bits either way.  counts[0..2] = frames of this context
 * that ran normal / recording / replaying since rt_create (instrumented and variant-0 launches are not counted). */
int rt_debug_first_hit(rt_context *ctx, uint64_t counts[3]);

/* Settled tiles (part of first-hit reuse; on unless the variant carries 0x800 or RT_SETTLED_TILES=0 was set at rt_create): an
 * 8x8 tile of the recorded window none of whose paths read the frame's bounce sample gives the same bits for every frameCount,
 * so the recording frame keeps its three surface values and replaying frames copy them out instead of tracing the tile.
 * out[0] = tiles of the cached window, out[1] = how many of them are settled; zeros while no recorded window is cached. */
int rt_debug_settled_tiles(rt_context *ctx, uint64_t out[2]);
/* The cached window's flags, one byte per tile in row-major tile order (1 = settled); n must be out[0] of
 * rt_debug_settled_tiles (0 without a cache).  Both calls wait for the context's work in flight. */
int rt_debug_settled_map(rt_context *ctx, uint8_t *flags, size_t n);
/* Prefix replay (part of first-hit reuse; on unless the variant carries 0x1000 or RT_PREFIX_REPLAY=0 was set at rt_create): a
 * tile none of whose paths reads the frame's bounce sample before depth K is the same bits up to the lighting of depth K for
 * every frameCount, so the recording frame keeps each pixel's path state there and replaying frames resume the tile at depth
 * K (capped at 7) instead of depth 0.  out[0] = settled tiles of the cached window, out[1 + K] = tiles that resume at depth
 * K = 0 .. 7; the nine add up to the window's tile count, and are zeros while no recorded window is cached.  Waits for the
 * context's work in flight. */
int rt_debug_prefix_tiles(rt_context *ctx, uint64_t out[9]);

/* Diagnostics of the last rt_count_rays / rt_count_rays_traced / rt_count_rays_to launch: out[0] rays (the total that call
 * returned), out[1] wave-level ray packets, out[2] candidate objects summed over packets (after packet culling, or from a
 * light's shadow table), out[3] 64-object cull passes.  [1..3] are zero for variant 0 (no packet culling). */
int rt_debug_stats(rt_context *ctx, uint64_t out[4]);
/* The same plus packet-coherence diagnostics of the packet kernel: out[4..7] packets whose direction boxes leave 3 / 2 / 1 / 0
 * axes usable for culling (an axis is lost when the packet's directions straddle zero on it), out[8] packets that cannot be
 * culled at all (NaN lanes, non-finite origins), out[9] / out[10] candidates summed over the 3-axis packets / the others,
 * out[11] active lanes summed over packets; out[12..19] section timers of a -DRT_PK_TIMERS=1 build (shader clocks summed over
 * waves; zero otherwise): closest-hit traversals, a light's packet + candidate masks, its PCF sample loops, the whole wave,
 * the light packet's set-up alone, masks of octant-split light packets, split / unsplit light packets; out[20] / out[21]
 * candidates entering / leaving the per-lane cull level of a light's PCF rays; timers build only: out[22] candidate trips of
 * the PCF sample loops, out[23] those in which some lane passes the slab test, out[24] lanes passing, out[25] sample groups, out[26] the whole
 * light loop, out[27] the subsurface section, out[28] PCSS blocker searches, out[29] hit shading set-up, out[30] roulette + next
 * direction (clocks); out[31] the blocker group G of that launch (rt_count_rays_to; written by the host, 1 for variant 0).
 * Relations that hold for every launch: the counters are sums of integers over waves, so two launches of the same frame give
 * the same out[0..11], out[20] and out[21]; out[21] <= out[20]; variant 0 leaves out[1..30] zero; out[12..19] and out[22..30]
 * are zero unless built with -DRT_PK_TIMERS=1.  Packets whose candidates come from a light's shadow table (PCF and blocker
 * rays of scenes that have tables) are counted in out[1] and out[2] only: no direction box is formed and no cull pass made for
 * them, so they appear in none of out[3..11].  Hence out[4] + ... + out[8] <= out[1] and out[9] + out[10] <= out[2], with
 * equality when no table served the launch; out[11] <= 64 * (out[4] + ... + out[8]) <= 64 * out[1]; out[0] <= 64 * out[1] (a
 * packet carries at most one ray per lane); out[11] >= the window's pixels inside the image (every primary ray is a lane of a
 * boxed packet); a mode-2 launch's out[0], out[1] and out[11] never exceed the mode-1 launch's of the same frame (the skips only
 * take packets and lanes away); and a packet-kernel launch
 * on a scene with objects in view has out[1], out[2], out[3] > 0 (the primary rays' packets are never table-driven). */
int rt_debug_stats_ex(rt_context *ctx, uint64_t out[32]);
/* Measured cost (shader clock cycles / 64, summed over the tile's waves) of every workgroup tile of the
 * last feedback-scheduled rt_render / rt_render_to launch, in raster tile order; synchronises.  Writes up
 * to cap entries, *nTiles / *tilesX describe the tile grid.  Measurement hook, no reference counterpart. */
int rt_debug_tile_costs(rt_context *ctx, unsigned *out, int cap, int *nTiles, int *tilesX);

/* Cost classes (0 lightest .. 31 heaviest, ratio 2^(1/4)) the tile-order predictor gave the tiles of the last predicted
 * launch, raster tile order; *nTiles = capacity of the class buffer (>= that launch's tiles).  Measurement hook; synchronises. */
int rt_debug_predicted_classes(rt_context *ctx, uint8_t *out, int cap, int *nTiles);

/* The tile order the last packet-kernel rt_render / rt_render_to / rt_render_into_image launch was given, and who supplied
 * it: out[k] = the tile workgroup k rendered (up to cap entries), *nTiles = that launch's tiles, *policy = 0 raster (no order
 * buffer: out = 0 .. n-1), 1 measured (an adopted longest-first sort of the tile costs), 2 predicted (from the frame's own
 * inputs), 3 the order of the frame's phase (frameCount mod 64).  Only in a context created with RT_DEBUG_TILE_ORDER=1 in the
 * environment, which then copies every launch's order aside before the launch (the sorts rewrite the live buffers behind
 * it); otherwise, and before the first such launch or after rt_set_variant, *nTiles = 0.  The copy is ONE buffer per
 * context: it is the last launch's order only if the caller synchronises between frames.  Test hook; synchronises.  No
 * reference counterpart. */
int rt_debug_tile_order(rt_context *ctx, uint32_t *out, int cap, int *nTiles, int *policy);

/* The longest-first sort of the measured order (256 linear cost bins, heaviest bin first, any order inside a bin) on
 * caller-supplied costs: HOST arrays of nTiles entries, sorted in device buffers of the call's own on the context's stream;
 * synchronises.  costs comes back as the kernel leaves it (cleared for the next accumulation), order[k] = the k-th tile to
 * start, accum (may be NULL; in/out) += the costs read.  Touches no scheduler state.  RT_ERR_INVALID_ARG: NULL context,
 * costs or order, nTiles outside [1, 2^20].  Test hook, no reference counterpart. */
int rt_debug_lpt_sort(rt_context *ctx, uint32_t *costs, int nTiles, uint32_t *order, uint32_t *accum);

/* TILE SPLIT: a replaying frame (first-hit reuse) on the measured tile order runs its heaviest tiles as
 * P = 2 .. 4 one-wave jobs that divide the tile's lighting among themselves; the pixels are the same bits.  RT_TILE_SPLIT=0 in
 * the environment at rt_create switches it off, RT_DEBUG_SPLIT_PARTS=2|3|4 makes every plan split every tile it can into that
 * many parts (tests).  rt_debug_split_tiles: out[t] = P of tile t (raster tile order, up to cap entries; 0 = the tile ran whole)
 * in the last replaying launch, *nTiles = that launch's tiles, 0 before the first one; a launch that ran without a plan reports
 * zeros.  A settled tile listed with a P was copied out by its first job alone.  Test hook; synchronises.  No reference counterpart. */
int rt_debug_split_tiles(rt_context *ctx, uint8_t *out, int cap, int *nTiles);

/* The split plan's rule on caller-supplied HOST arrays: order[k] = the k-th tile to start and costs[t] = tile t's cost (nTiles
 * entries each), waveSlots = the resident wave slots the costs' sum is divided by, depth / nLt = the frame's maxRayDepth and
 * lights, forceParts = 0 or RT_DEBUG_SPLIT_PARTS' value, prevParts (may be NULL) = the plan in use.  Out: parts[t] = P or 0,
 * slot[t] = a split tile's scratch slot, extra[1536] = the jobs beyond each split tile's first (tile | part << 28; entries
 * beyond counts[0] are 0xffffffff), counts = (extra jobs, split tiles).  Touches no scheduler state; synchronises.
 * RT_ERR_INVALID_ARG: NULL context or array, nTiles outside [1, 2^20], depth outside [0, 32], forceParts not 0, 2, 3 or 4.
 * Test hook, no reference counterpart. */
int rt_debug_split_plan(rt_context *ctx, const uint32_t *order, const uint32_t *costs, int nTiles, uint32_t waveSlots, int depth, int nLt,
                        int forceParts, const uint8_t *prevParts, uint8_t *parts, uint32_t *slot, uint32_t *extra, uint32_t counts[2]);

/* The lights' SHADOW TABLES of the current scene (built by rt_set_scene for scenes of <= 256 objects; csrc/rt_shadowtab.inc):
 * per light 28 dwords of header -- (kind, base dword, K, NB) (invBinW, binMax, wlo, nmax^2) (pmin, qmin, invCell, cells)
 * (T0, eta) (B0, nmax) (light position or direction, binW) (base dword of the light's BLOCKER table or 0, its eta, -, -);
 * kind 0 no table, 1 cube map x distance bins (point / area), 2 planar grid x depth bins (directional) -- followed by the
 * cells, *wordsPerCell dwords each, bit i = object i may occlude a PCF ray of a shading point that reads the cell; scenes
 * with a PCSS light: a second table per such light, same cells, for pcssShadow's 16 blocker rays
 * (raytracingCs.glsl:409-427).  out == NULL only queries *nDwords.  Test hook
 * (tests/test_shadow_tables.py checks the tables against brute-force rays); synchronises.  No reference counterpart. */
int rt_debug_shadow_tables(rt_context *ctx, uint32_t *out, size_t capDwords, size_t *nDwords, int *wordsPerCell);

/* The GL driver's own sin / cos / tan / exp as the path evaluates them (csrc/rt_mesa_math.h: tan(radians(fov)/2) of
 * raytracingCs.glsl:209, cos/sin of :296-298, sin of random() :274, exp of :334), host side: out[4i..4i+3] =
 * sin, cos, tan, exp of in[i].  Test hook (no GPU needed), no reference counterpart. */
int rt_debug_mesa_math(const float *in, float *out, int n);

/* The device-side arithmetic primitives of the render kernels, one call each on caller-supplied operands: the inline
 * functions of csrc/rt_fastmath.h, the DEVICE instantiation of csrc/rt_mesa_math.h and the small helpers of
 * csrc/rt_kernels.hip, compiled in the render kernels' translation unit with their flags (no copy of the arithmetic).
 * dIn / dOut: n records of four 32-bit words (device, 16-byte aligned); in = (a, b, c, d) as float bit patterns unless
 * stated, out words not listed are 0:
 *   RCP       rtf::rcp(a),  rtf::rcp_fast(a, ok),  ok (0 / 1)
 *   RCP3      rtf::rcp3(a, b, c): 1/a, 1/b, 1/c
 *   SQRT      rtf::sqrt(a),  rtf::sqrt_fast(a, ok),  ok
 *   RCP_SQRT  rtf::rcp_sqrt(a),  rtf::rcp_sqrt_fast(a, ok),  ok
 *   DIV2      rtf::div2(a, b, c): a/c, b/c;  rtf::div_fast(a, c, y = rtf::rcp_fast(c, oky), ok0),  oky & ok0
 *   DIV3      rtf::div3(a, b, c, d): a/d, b/d, c/d
 *   MESA      rtm::sin_(a), cos_(a), tan_(a), exp_(a)
 *   F2H       f2h_rtz(a) (the fp16 bits, round toward zero, as a uint32),  half_bits_to_float(low 16 bits of b)
 *   POW5      pow5(a)
 *   HALTON    halton_eval(index = a as int32, base = b as int32); a base < 2 (the loop would not end) gives 0 uncalled
 * LAUNCH GEOMETRY (fixed; tests/test_device_math.py composes wavefronts with it): 256-thread blocks, exactly one record per
 * thread, record i is processed by lane i % 64 of wavefront i / 64, no grid-stride loop.  n need not be a multiple of 64:
 * the tail lanes of the last wavefront exit BEFORE the primitive is called, so they take no part in its ballot, and
 * nothing past record n - 1 is written.  The rtf:: functions replace their fast path by the IEEE sequence for a whole
 * wavefront when any of its lanes needs it (wave-uniform branch), so what a lane's operand exercises depends on its 63
 * neighbours; the *_fast outputs are the lane's own fast-path value and its guard.
 * n == 0 is a no-op.  RT_ERR_INVALID_ARG: NULL context, unknown op, NULL / misaligned pointer; RT_ERR_TOO_LARGE: more
 * records than one grid holds.  Asynchronous on hipStream (NULL = the context's stream).  Test hook, no reference
 * counterpart. */
typedef enum rt_device_math_op {
    RT_DM_RCP = 0, RT_DM_RCP3 = 1, RT_DM_SQRT = 2, RT_DM_RCP_SQRT = 3, RT_DM_DIV2 = 4, RT_DM_DIV3 = 5, RT_DM_MESA = 6,
    RT_DM_F2H = 7, RT_DM_POW5 = 8, RT_DM_HALTON = 9, RT_DM_OP_COUNT = 10
} rt_device_math_op;
int rt_debug_device_math(rt_context *ctx, int op, const void *dIn, void *dOut, size_t n, void *hipStream);

/* ---- ray queries on the scene of the last rt_set_scene: the shader's intersectObjects (raytracingCs.glsl:155-196)
 *      outside a frame, for the questions a host asks about the scene (which object is under the mouse, is a segment
 *      blocked, where does a ray first hit).  No reference counterpart: the reference's editor can only pick from a list
 *      (ImGUIManager::DrawObjectsList).  Same fp32 arithmetic as the render kernels, bit for bit.
 *
 * rt_ray (32 B): the ray o + d*t, 0 < t < tMax.  d need not be normalised.  reserved is ignored (write 0).
 * rt_hit (32 B), RT_QUERY_CLOSEST: intersectObjects with maxRayDistance replaced by the ray's tMax -- the AABB cull
 *      uses tMax, minT starts at tMax, equal t keeps the lower object index.  Hit: object = index into the caller's
 *      object array, t = hit distance, position = o + d*t, normal = normalize(o + d*t - centre) for a sphere and the
 *      raw (unnormalised) plane normal for a plane -- the render kernels' P and N.  Miss: object = -1, t = tMax
 *      (the shader's minT), position and normal 0.  A ray whose tMax is <= 0 or NaN misses.
 * RT_QUERY_ANY: one int32_t per ray, 1 iff some object passes the AABB cull and the shape test with 0 < t < tMax,
 *      else 0; equal to (closest.object >= 0) for every ray. */
typedef struct rt_ray { float origin[3]; float tMax; float direction[3]; int32_t reserved; } rt_ray;
typedef struct rt_hit { float position[3]; float t; float normal[3]; int32_t object; } rt_hit;
typedef enum rt_query_mode { RT_QUERY_CLOSEST = 0, RT_QUERY_ANY = 1 } rt_query_mode;

/* nRays rays (device, rt_ray) -> nRays rt_hit (CLOSEST) or int32_t (ANY) (device).  Both pointers 16-byte aligned.
 * nRays == 0 is a no-op.  RT_ERR_INVALID_ARG: NULL / misaligned pointer, unknown mode, no scene set.  Asynchronous
 * on hipStream (NULL = the context's stream), ordered with rt_set_scene like rt_render_to. */
int rt_trace_rays(rt_context *ctx, const void *dRays, size_t nRays, int mode, void *dOut, void *hipStream);
/* The primary rays of rt_render_to(p): regionW x regionH rt_ray (device, 16-byte aligned) in exactly the surface
 * layout rt_render_to writes for the same p (local rows, window, strips), bit-identical to the rays the renderer
 * traces (noise jitter, frameCount, the GL's tan); tMax = p->maxRayDistance.  Window pixels outside the image get an
 * all-zero record (zero direction, tMax = 0: they miss).  Asynchronous on hipStream (NULL = the context's stream). */
int rt_camera_rays(rt_context *ctx, const rt_params *p, void *dRays, void *hipStream);
/* Closest hit of the primary ray of IMAGE pixel (px, py) (row 0 = bottom, as in the surfaces; the window and strip
 * fields of p are ignored) -- click-to-select.  Synchronous on the context's stream.  A pixel outside the image or
 * no scene set: RT_ERR_INVALID_ARG. */
int rt_pick(rt_context *ctx, const rt_params *p, int px, int py, rt_hit *hit);

/* ---- an opt-in acceleration structure behind rt_trace_rays and rt_pick.  Off by default: every query
 *      then runs the brute-force kernels, which test every object.  Switched on, the host builds a bounding-volume hierarchy over
 *      the objects' STORED boxes at every scene change, and the queries walk it.  The results are the brute-force ones bit for
 *      bit, for every ray and every scene: the hierarchy only skips objects whose own stored-box test (the AABB cull above) would
 *      fail, never anything "behind the current hit", so the set of objects that count does not change, and among equal t the
 *      lower object index wins whatever the visiting order.  By default rt_shade_rays does not use it (rt_set_accel_shading
 *      below switches that on), and neither do the renders (rt_set_accel_render, further below, switches that on).
 *
 *   Structure.  A binary tree, median split on the box centres, stored in depth-first pre-order: the first child of inner node k is
 *      node k + 1, and `skip` is the index of the first node behind k's subtree (the node count behind the last one), so a walk
 *      needs no stack -- "descend" is k + 1, "skip" is nodes[k].skip.  `leaf` is 0xffffffff for an inner node, else first << 4 |
 *      count: the leaf's objects are order[first .. first + count).  lo / hi: the exact union of the stored boxes below (an
 *      inverted stored box counts as the swapped one).  Objects with a NaN or infinite bound, and objects whose box spans more
 *      than largeFraction of the extent of all finite boxes on some axis (a floor, the walls of a room), are kept out of the tree
 *      on the LOOSE list, which every ray tests as the brute-force kernels do.  order[] and loose[] together hold every object
 *      index exactly once.
 *   rt_accel_desc: zero = the default of every field.  enable: 0 switches the feature off.  leafSize: most objects of a leaf,
 *      1..8 (default 4).  traversal: RT_ACCEL_WAVE walks the tree once per wavefront (nodes by scalar loads; for coherent rays),
 *      RT_ACCEL_LANE once per ray; RT_ACCEL_AUTO (default) chooses per launch -- today always the per-ray form, the one that is
 *      never slower than brute force from the default minObjects up whatever the rays; primary rays (rt_camera_rays) run another 2x
 *      faster with RT_ACCEL_WAVE, which pays from 64 objects (DESIGN.md section 32 has the table).  rt_pick always uses the
 *      per-wavefront form.  minObjects: scenes with fewer objects are served
 *      by the brute-force kernels (default 1024), as are scenes whose tree would be empty.  largeFraction: default 0.5.
 *   rt_set_accel: sticky for the context; NULL or enable == 0 switches it off.  While on, rt_set_scene rebuilds the structure
 *      when the scene bytes change (an identical re-upload stays a no-op), and rt_set_accel itself builds at once when a scene is
 *      loaded.  The upload is ordered like the scene's own.  RT_ERR_INVALID_ARG: an unknown traversal, a non-zero reserved word,
 *      leafSize outside 0..8, a negative minObjects, a negative or non-finite largeFraction.
 *   rt_accel_info: built (the current scene's queries walk a tree), nodes, leaves, depth, loose, bytes (of the device structure),
 *      buildMs (host time of the last build and its check), builds (since rt_create), and how many query launches (rt_trace_rays
 *      and rt_pick) went each way since rt_create: launchesAccel[0] per-wavefront, [1] per-ray, launchesBrute (counted only while
 *      the feature is on).
 *   rt_accel_build_host: the same build with no GPU and no context (enable and minObjects are not looked at).  nodes / order /
 *      loose all NULL: only info is filled (nodes, loose and nObj - loose give the sizes).  Else the arrays are written;
 *      RT_ERR_TOO_LARGE when a capacity (in elements) is too small or nObj > RT_MAX_OBJECTS. */
#define RT_ACCEL_INNER 0xffffffffu   /* rt_accel_node.leaf of an inner node */
typedef enum rt_accel_traversal { RT_ACCEL_AUTO = 0, RT_ACCEL_LANE = 1, RT_ACCEL_WAVE = 2 } rt_accel_traversal;
typedef struct rt_accel_desc {
    int32_t enable, leafSize, traversal, minObjects;
    float largeFraction;
    int32_t reserved[3];
} rt_accel_desc;                     /* 32 B */
typedef struct rt_accel_node { float lo[3]; uint32_t skip; float hi[3]; uint32_t leaf; } rt_accel_node;   /* 32 B */
typedef struct rt_accel_report {
    int32_t built, nodes, leaves, depth, loose, reserved0;
    uint64_t bytes;
    double buildMs;
    uint64_t builds, launchesAccel[2], launchesBrute, reserved[3];
} rt_accel_report;                   /* 96 B */
int rt_set_accel(rt_context *ctx, const rt_accel_desc *desc);
int rt_accel_info(rt_context *ctx, rt_accel_report *info);
int rt_accel_build_host(const void *objects, int nObj, const rt_accel_desc *desc, rt_accel_node *nodes, size_t capNodes, uint32_t *order,
                        size_t capOrder, uint32_t *loose, size_t capLoose, rt_accel_report *info);
/* The check every structure passes before the context uploads it, on caller arrays (no GPU): RT_OK iff a walk may use them for these
 * objects -- pre-order, every skip link strictly forward and equal to its subtree's end, the leaves within leafSize (1..8) and taking
 * order[] in sequence, every object index below nObj and used exactly once across order[] and loose[], every node box finite and the
 * exact union of its children's; else RT_ERR_INVALID_ARG.  It reads nothing outside the arrays whatever they hold. */
int rt_accel_validate_host(const void *objects, int nObj, int leafSize, const rt_accel_node *nodes, size_t nNodes, const uint32_t *order,
                           size_t nOrder, const uint32_t *loose, size_t nLoose);

/* ---- who builds the hierarchy.  RT_ACCEL_BUILD_HOST (default): one host thread, median splits, the check
 *      above before the upload -- everything as described so far.  RT_ACCEL_BUILD_DEVICE: HIP kernels on the context's stream build
 *      the SAME structure (rt_accel_node in pre-order with skip links, order[], loose[]) over another topology, a linear BVH:
 *      the host only classifies (loose[] is the host builder's, for the same bytes and desc), the device sorts the tree's objects
 *      by (30-bit Morton code of the box centre, object index), cuts the sequence into leaves of leafSize (within a leaf ascending
 *      object index), and builds the binary radix tree over the leaves' keys; every box is the exact union of the stored boxes
 *      below, as before.  The hierarchy only culls, so queries and shading answer the same bits through either tree; the Morton
 *      tree is coarser (slower to walk) and far cheaper to build from a few thousand objects up -- for scenes that change every
 *      frame.  A device-built structure is not run through the host check; what keeps the walks inside their arrays whatever the
 *      device wrote is stated in DESIGN.md section 36.
 *
 *   rt_set_accel_builder: sticky, independent of rt_set_accel and of the order of the two calls.  A change while rt_set_accel is on
 *      and a scene is loaded rebuilds at once (ordered like rt_set_accel's own rebuild); the same value again does nothing.
 *      RT_ERR_INVALID_ARG: a NULL context, an unknown value.  A HIP failure during a device build is RT_ERR_HIP, and the queries
 *      are served by brute force until the next build.
 *   rt_accel_build_info: builder (of the structure that stands; 0 while none does), buildsHost / buildsDevice (since rt_create;
 *      their sum is rt_accel_info's builds), hostMs (the last build's host time inside the call: the host build and its check, or
 *      the classification and the enqueue of the device build), deviceMs (the last device build between the two events around it;
 *      0 after a host build; the first request after a build waits for it).
 *   rt_accel_info after a device build: nodes, leaves, loose, bytes and builds are known at once; depth is fetched from the device
 *      on the first request, which waits for the build; buildMs is hostMs.
 *   rt_accel_read: the structure that stands on the device, from either builder, copied to the host; it waits for the context's
 *      stream.  info: rt_accel_info's.  nodes / order / loose all NULL: only info (nodes, loose and nObj - loose give the sizes).
 *      Else the arrays are written; RT_ERR_TOO_LARGE when a capacity (in elements) is too small.  While nothing is built info is
 *      all zeros and nothing is written. */
typedef enum rt_accel_builder { RT_ACCEL_BUILD_HOST = 0, RT_ACCEL_BUILD_DEVICE = 1 } rt_accel_builder;
int rt_set_accel_builder(rt_context *ctx, int builder);
typedef struct rt_accel_build_report {
    int32_t builder;        /* of the structure that stands; 0 while none is built */
    int32_t reserved0;
    uint64_t buildsHost, buildsDevice;
    double hostMs;          /* last build: host time inside the call (classification + enqueue, or the host build) */
    double deviceMs;        /* last device build between its two events; 0 for a host build; the call waits for it */
    uint64_t reserved[3];
} rt_accel_build_report;             /* 64 B */
int rt_accel_build_info(rt_context *ctx, rt_accel_build_report *info);
int rt_accel_read(rt_context *ctx, rt_accel_node *nodes, size_t capNodes, uint32_t *order, size_t capOrder,
                  uint32_t *loose, size_t capLoose, rt_accel_report *info);

/* ---- the same hierarchy behind rt_shade_rays.  Off by default, also while rt_set_accel is on: rt_shade_rays
 *      then launches the brute-force kernel, which tests every object for every closest-hit, shadow, PCSS-blocker and subsurface
 *      ray.  Switched on, those four kinds of ray walk the tree rt_set_accel built (this switch builds nothing; the two switches
 *      are independent and may be set in either order).  The colour, position and normal written are the brute-force kernel's,
 *      bit for bit, for every ray and every scene: closest hits by the argument above; a shadow or blocker ray's answer is "some
 *      object passes its own stored-box test at maxRayDistance and is hit with 0 < t < min(maxRayDistance, lightDistance)", the
 *      walk tests nodes and gates objects at the first distance and accepts at the second, and an existential answer does not
 *      depend on the visiting order.
 *
 *   rt_accel_shade_desc: zero = the default of every field.  enable: 0 switches the feature off.  traversal: rt_accel_traversal's
 *      values, independent of rt_accel_desc's: RT_ACCEL_WAVE walks once per wavefront (the lanes still on a path share the walk),
 *      RT_ACCEL_LANE once per ray; RT_ACCEL_AUTO (default) is the per-ray form, which from 256 objects up was faster than the
 *      brute-force kernel on every measured ray set and from 1024 up faster than the per-wavefront form too; RT_ACCEL_WAVE pays
 *      from 64 objects and is the faster form on camera frames and probes up to 256 (DESIGN.md section 33 has the table).
 *      minObjects: scenes with fewer objects are shaded by the brute-force kernel (0 = the default, 256).  rt_set_accel has a
 *      minObjects of its own (default 1024) below which it builds no tree: to shade smaller scenes through one, lower both.
 *   rt_set_accel_shading: sticky for the context; NULL or enable == 0 switches it off.  RT_ERR_INVALID_ARG: a NULL context, an
 *      unknown traversal, a non-zero reserved word, a negative minObjects.
 *   rt_accel_shading_info: active (1 iff the next rt_shade_rays would walk the tree: the switch is on, rt_set_accel has built the
 *      current scene's tree, and the scene has at least minObjects objects), traversal (the resolved one: RT_ACCEL_LANE or
 *      RT_ACCEL_WAVE; 0 while off), and how many rt_shade_rays launches went each way since rt_create: launchesAccel[0]
 *      per-wavefront, [1] per-ray, launchesBrute (counted only while this switch is on).  rt_accel_info's counters count queries
 *      only. */
#define RT_ACCEL_SHADE_DEFAULT_MIN_OBJECTS 256
typedef struct rt_accel_shade_desc { int32_t enable, traversal, minObjects, reserved[5]; } rt_accel_shade_desc;   /* 32 B; zero = defaults */
typedef struct rt_accel_shade_report {
    int32_t active, traversal;
    uint64_t launchesAccel[2], launchesBrute, reserved[2];
} rt_accel_shade_report;             /* 48 B */
int rt_set_accel_shading(rt_context *ctx, const rt_accel_shade_desc *desc);
int rt_accel_shading_info(rt_context *ctx, rt_accel_shade_report *info);

/* ---- the same hierarchy behind the frames: rt_render, rt_render_to, rt_render_into_image, and rt_frame through rt_render
 *      (DESIGN.md section 37).  Off by default, also while the two switches above are on: a frame then runs the packet kernel,
 *      which has shadow tables up to 256 objects and 64 lights and above that tests every object for every closest-hit, shadow,
 *      blocker and subsurface ray.  Switched on, a frame of a scene whose tree stands is rendered by a kernel of its own -- one
 *      wavefront per 8x8 pixel tile, the per-lane path tracer rt_shade_rays runs, camera ray and noise sample taken from the
 *      frame -- whose four kinds of ray walk the tree.  It writes the same three surfaces in the same formats and layouts (window,
 *      local rows, both strip rules, rt_render_into_image's stores, all-zero records for window pixels outside the image), and
 *      every value is the packet kernel's bit for bit, by the two arguments above.  This switch builds nothing: it uses the tree
 *      rt_set_accel built, from either builder, and is independent of the other three switches and of the order of the calls.
 *
 *   rt_accel_render_desc: zero = the default of every field.  enable: 0 switches the feature off.  traversal:
 *      RT_ACCEL_RENDER_LANE walks once per ray and RT_ACCEL_RENDER_WAVE once per wavefront, as in rt_shade_rays;
 *      RT_ACCEL_RENDER_SPLIT takes the depth-0 closest hit -- the 64 coherent primary rays of a tile -- by one per-wavefront walk
 *      and every later ray by the per-ray walks; RT_ACCEL_RENDER_AUTO (default) is the per-ray form: measured from 1025 objects
 *      up, LANE and SPLIT lie within each other's spread on every scene and both are 1.2-2.2x faster than WAVE (section 37).
 *      rt_accel_traversal keeps its three values: rt_set_accel and rt_set_accel_shading refuse 3.  minObjects: scenes with
 *      fewer objects keep the packet kernel (0 = RT_ACCEL_RENDER_DEFAULT_MIN_OBJECTS, the smallest measured scene from which
 *      AUTO beat the packet kernel beyond both spreads: 3.4x there, 5.7x at 16386 objects; at 1026 the two were level, at 258
 *      and below the packet kernel, which has shadow tables up to 256 objects, is 1.6-9.5x faster); rt_set_accel has a minObjects
 *      of its own (default 1024) below which there is no tree.
 *   rt_set_accel_render: sticky for the context; NULL or enable == 0 switches it off.  RT_ERR_INVALID_ARG: a NULL context, an
 *      unknown traversal, a non-zero reserved word, a negative minObjects.
 *   Which frames take it: those for which `active` holds, except the exhaustive cross-check kernel (rt_set_variant's variant 0)
 *      and every instrumented launch (rt_count_rays*), which stay what they were.  A frame through the tree neither records nor
 *      replays first hits and leaves that cache and rt_debug_first_hit's counts as it found them; it takes no part in the tile
 *      scheduler (orders, costs and predicted classes of the packet frames are untouched); rt_last_kernel_ms times it, and scene
 *      and texture uploads order behind it like behind any frame.  rt_mgpu_* has no accel API and never takes it.
 *   rt_accel_render_info: active (1 iff the next plain frame would walk the tree: the switch is on, rt_set_accel has built the
 *      current scene's tree, and the scene has at least minObjects objects), traversal (the resolved one, never AUTO; 0 while
 *      off), minObjects (the resolved one), and how many frames went each way since rt_create: launchesAccel[0] per-wavefront,
 *      [1] per-ray (the order of the other two reports), [2] SPLIT; launchesPacket: frames that took the existing kernels while
 *      this switch was on.  rt_accel_info's and rt_accel_shading_info's counters do not count frames. */
typedef enum rt_accel_render_traversal {
    RT_ACCEL_RENDER_AUTO = 0, RT_ACCEL_RENDER_LANE = 1, RT_ACCEL_RENDER_WAVE = 2, RT_ACCEL_RENDER_SPLIT = 3
} rt_accel_render_traversal;
#define RT_ACCEL_RENDER_DEFAULT_MIN_OBJECTS 4098
typedef struct rt_accel_render_desc { int32_t enable, traversal, minObjects, reserved[5]; } rt_accel_render_desc;   /* 32 B; zero = defaults */
typedef struct rt_accel_render_report {
    int32_t active, traversal, minObjects, reserved0;
    uint64_t launchesAccel[3], launchesPacket, reserved[2];
} rt_accel_render_report;            /* 64 B */
int rt_set_accel_render(rt_context *ctx, const rt_accel_render_desc *desc);
int rt_accel_render_info(rt_context *ctx, rt_accel_render_report *info);

/* ---- ray shading on the scene of the last rt_set_scene: main() of raytracingCs.glsl (:509-584) on caller-supplied rays,
 *      for what a frame's pinhole camera cannot ask (cubemap / environment probes, panoramas, stereo, fisheye or
 *      orthographic views, re-shading a sparse set of pixels).  No reference counterpart.  Same fp32 arithmetic as the
 *      render kernels, bit for bit.
 *
 * rt_pixel (8 B): the gl_GlobalInvocationID.xy ray k is shaded as.  It feeds only the noise tap sample_noise(x, y) that
 *      PCF's jitter reads (:359) and the Russian roulette's random(gid + depth) (:547).
 * Ray k runs main() with generateCameraRay replaced by the ray's (origin, direction), taken as given (no normalisation,
 *      no jitter).  The primary segment (depth 0) runs intersectObjects with maxRayDistance replaced by the ray's tMax --
 *      the AABB cull and where minT starts, as rt_trace_rays CLOSEST; every later bounce and every shadow, PCSS-blocker
 *      and SSS ray uses p->maxRayDistance.  p->frameCount (hammersley rows, noise offset), maxRayDepth, maxRayDistance,
 *      useSkybox and noiseScale keep their meaning; the camera fields are ignored when dPixels != NULL, but p is still
 *      validated as for rt_render_to.  Outputs in rt_render_to's per-pixel formats: colour (finalColor, 1), position
 *      (P, 1), normal (N, 1) as fp16 rounded toward zero; P / N are the last hit's.  A miss on the primary segment gives
 *      P = N = 0 and colour skybox(d) (or 0 without a skybox / useSkybox).
 * dPixels == NULL: the rays are in rt_camera_rays(p)'s surface layout, nRays must equal regionW * regionH, and ray k is
 *      shaded as the image pixel rt_render_to(p) writes at surface index k (window, local rows, strips); window pixels
 *      outside the image get the all-zero records rt_render_to writes.  So rt_shade_rays(p, rt_camera_rays(p), NULL)
 *      equals rt_render_to(p) bit for bit on all three surfaces. */
typedef struct rt_pixel { uint32_t x, y; } rt_pixel;

/* nRays rays (device, rt_ray, 16-byte aligned) and pixels (device, rt_pixel, 8-byte aligned, or NULL: see above) ->
 * nRays float4 colours (required), float4 positions and 4 x fp16 normals (each NULL = not stored), all device and
 * 16- / 16- / 8-byte aligned.  nRays == 0 is a no-op.  RT_ERR_INVALID_ARG: no scene set, NULL required / misaligned
 * pointer, dPixels == NULL with nRays != regionW * regionH, p failing rt_render_to's checks (e.g. maxRayDepth > 32);
 * RT_ERR_TOO_LARGE: more rays than one grid holds (as rt_trace_rays).  Asynchronous on hipStream (NULL = the context's
 * stream), ordered with rt_set_scene like rt_render_to; rt_set_noise / rt_set_skybox wait for it. */
int rt_shade_rays(rt_context *ctx, const rt_params *p, const void *dRays, const void *dPixels, size_t nRays, void *dColor,
                  void *dPosition, void *dNormal, void *hipStream);

const char *rt_last_error(rt_context *ctx);

/* ---- host-side feeders of the byte contract (no GPU needed) */
/* GenerateAABBForObject (/root/reference/src/SceneIO.h:75-104), in place on n records. */
int rt_generate_aabb(void *objects, int n);
/* Camera::UpdateVectors (/root/reference/src/Camera.h:26-34). */
int rt_camera_vectors(float yawDeg, float pitchDeg, float front[3], float right[3], float up[3]);
/* SceneIO::Load's parser (/root/reference/src/SceneIO.h:108-122,145-186) on an in-memory
 * text; fills up to maxObj/maxLt records (AABBs generated), returns counts. */
int rt_scene_parse(const char *text, void *objects, int maxObj, int *nObj, void *lights,
                   int maxLt, int *nLt);

/* SceneIO::Save's writer (/root/reference/src/SceneIO.h:50-73, 124-142) into a caller buffer:
 * one "OBJECT <TYPE> <name> 18 numbers" / "LIGHT <TYPE> <name> 12 numbers" line per record, default
 * ostream float formatting.  Names may be NULL ("Object<i>" / "Light<i>").  *needed receives the
 * size including the terminator; out == NULL only queries it; too small -> RT_ERR_TOO_LARGE.
 * Lossy exactly like the reference's format (diffuseStrength, subsurface*, shadow fields are not stored). */
int rt_scene_write(const void *objects, int nObj, const void *lights, int nLt,
                   const char *const *objNames, const char *const *lightNames, char *out,
                   size_t cap, size_t *needed);

/* ---- next row after the ray tracer: the TAA resolve pass
 *      (/root/reference/shader/taaFs.glsl:13-53; host side ForwardShadingPipeline.cpp:231-260).
 *      dCurrent = gColor of this frame (rgba32f, sampled LINEAR/REPEAT), dHistory = the previous
 *      resolve (rgba32f, LINEAR/CLAMP_TO_EDGE), dNormal = gNormal (rgba16f, NEAREST/REPEAT), all
 *      width x height device surfaces as produced by rt_render; dOut = the new history (rgba32f).
 *      The caller ping-pongs dHistory/dOut like historyTex[2] (:233, :248); dOut == dCurrent or
 *      dOut == dHistory is refused (RT_ERR_INVALID_ARG).  Asynchronous on hipStream (NULL = the
 *      context's stream).
 *
 *      Streams and the post passes (rt_taa_resolve, rt_bloom, rt_ssao, rt_ssao_blur): they may be issued
 *      on any streams concurrently, and next to rt_frame on the context's stream.  A pass is ordered
 *      on its stream like any kernel there, so the caller orders its own surfaces (inputs written
 *      before, outputs read after, on that stream or behind an event).  The scratch a pass keeps inside
 *      the context (rt_bloom's rgba16f targets, rt_ssao's depth plane) is one per context: the library
 *      orders each pass behind the previous user of that scratch with an event, on the device, whichever
 *      streams the two ran on -- such passes run one after another -- and waits for the last user on
 *      the host only when the scratch has to grow for a larger frame, and in rt_destroy. */
int rt_taa_resolve(rt_context *ctx, const void *dCurrent, const void *dHistory, const void *dNormal,
                   void *dOut, int width, int height, float blendFactor, float jitterX,
                   float jitterY, void *hipStream);
/* uJitterX / uJitterY of ForwardShadingPipeline.cpp:241-242 (global.cpp:41-51's haltonSequence). */
int rt_taa_jitter(int frameCount, int width, int height, float *jitterX, float *jitterY);

/* ---- bloom: brightness extract (threshold), `iterations` alternating 9-tap
 *      Gaussian passes on rgba16f targets starting horizontal, combine scene + bloom*strength
 *      (/root/reference/shader/{brightness_extractFS,gaussian_blurFs,bloom_combineFs}.glsl;
 *      ForwardShadingPipeline.cpp:189-228 uses threshold 1.0, 10 iterations, strength 0.5).
 *      dScene = gColor (rgba32f), dOut = combined rgba32f (what the reference draws to the default
 *      framebuffer, before display quantisation); dOut == dScene is refused (RT_ERR_INVALID_ARG: a
 *      fused pass reads neighbouring tiles' scene texels while other workgroups store theirs), and the
 *      surfaces may not overlap in any other way either.  Asynchronous on hipStream (NULL = the
 *      context's stream). */
int rt_bloom(rt_context *ctx, const void *dScene, void *dOut, int width, int height, float threshold,
             float strength, int iterations, void *hipStream);

/* ---- next row: SSAO -- shader/ssaoFs.glsl:16-46 and ssao_blurFs.glsl:11-29 as driven by AOManager::RenderSSAO
 *      (AO.cpp:86-117).  dPosition (rgba32f) / dNormal (rgba16f) are the ray kernel's G-buffer surfaces;
 *      hNoise = the rotation texture (nW x nH rgba32f texels, nW*nH <= 16; AO.cpp:38-51 makes it 4x4),
 *      hSamples = the 64 kernel samples (AO.cpp:23-36), hProjection / hView = column-major mat4 (the glm
 *      matrices AO.cpp:91-92 uploads; rt_camera_matrices builds them like Camera.h:36-42); all four are HOST
 *      pointers, copied at the call.  dOut = width*height floats: the value the fragment shader writes (the
 *      reference renders it into FBOs without attachments, so upstream nothing consumes it); dOut ==
 *      dPosition or dOut == dNormal is refused (RT_ERR_INVALID_ARG: every pixel samples its neighbours'
 *      G-buffer).
 *      rt_ssao_blur: one separable 9-tap pass (the reference draws a single pass and never sets `horizontal`,
 *      i.e. vertical); dOut == dIn is refused.  Asynchronous on hipStream (NULL = the context's stream). */
int rt_ssao(rt_context *ctx, const void *dPosition, const void *dNormal, void *dOut, int width, int height,
            const float *hNoise, int noiseW, int noiseH, const float *hSamples, const float *hProjection,
            const float *hView, void *hipStream);
int rt_ssao_blur(rt_context *ctx, const void *dIn, void *dOut, int width, int height, int horizontal, void *hipStream);
/* glm::lookAt(Position, Position + Front, Up) and glm::perspective(radians(FOV), aspect, 0.1, 100) of
 * Camera.h:36-42, column-major, fp32. */
int rt_camera_matrices(const float position[3], const float front[3], const float up[3], float fovDeg, float aspect,
                       float view[16], float projection[16]);

/* ---- next row: equirectangular -> cubemap -- ConvertHDRToCubemap (TextureLoader.cpp:118-194) with
 *      shader/skyboxVs.glsl + skyboxFs.glsl: hEquirectRGB = width*height*3 HOST floats as stbi_loadf returns
 *      them after the vertical flip (row 0 = bottom); the map is stored as RGB16F (rounded toward zero, as the
 *      reference's GL does on upload) and
 *      sampled LINEAR / CLAMP_TO_EDGE into six size x size RGB16F faces (GL face order, the layout
 *      rt_set_skybox takes).  dFacesOut (device, 6*size*size*3 halfs) may be NULL; install != 0 makes the
 *      result the context's skybox (what LoadHDRAsCubemap's caller does with the GL texture).  Synchronous. */
int rt_equirect_to_cubemap(rt_context *ctx, const float *hEquirectRGB, int width, int height, int size,
                           void *dFacesOut, int install);

/* ---- the caller of the path: one iteration of ForwardShadingPipline::Render()'s GPU work
 *      (ForwardShadingPipeline.cpp:155-260) in one call, on the context's own surfaces and stream:
 *        ray trace (:155-182)  ->  AO (:185-187, if enableAO)  ->  bloom: extract, blur passes, combine into the
 *        image the reference draws to the default framebuffer (:189-228)  ->  TAA resolve into
 *        historyTex[frameCount % 2] from historyTex[1 - frameCount % 2] (:231-258, if enableTAA).
 *      p->frameCount plays the reference's static frameCount (:141-142): it selects the history slot and the
 *      TAA jitter and is the shader's frameCount uniform; like the reference, the caller advances it only on
 *      frames with TAA enabled (:254).  History surfaces start as zeros.  dDisplay (device, width*height
 *      rgba32f) receives the bloom-combined image; may be NULL.  Asynchronous on the context's stream;
 *      rt_frame_surfaces returns the context-owned results (valid until the next size change). */
typedef struct rt_frame_desc {
    int32_t enableAO, enableTAA;
    float taaBlendFactor;            /* imguiManager.GetTAABlendFactor() */
    float bloomThreshold;            /* 1.0  (:197) */
    float bloomStrength;             /* 0.5  (:223) */
    int32_t bloomIterations;         /* 10   (:212) */
    const float *aoSamples;          /* 64 x 3 host floats (AO.cpp:23-36); required when enableAO */
    const float *aoNoise;            /* 4 x 4 x 4 host floats (AO.cpp:38-51) */
    float camYawPitchUnused[2];      /* reserved, zero */
} rt_frame_desc;
int rt_frame(rt_context *ctx, const rt_params *p, const rt_frame_desc *desc, void *dDisplay);
/* dAO = blurred AO (floats), dHistory = the history slot the last rt_frame wrote (rgba32f); NULL when that
 * pass has not run. */
int rt_frame_surfaces(rt_context *ctx, void **dColor, void **dPosition, void **dNormal, void **dAO, void **dHistory);

/* ---- the last step of Render(): the default framebuffer and glfwSwapBuffers (ForwardShadingPipeline.cpp:220-228 draws
 *      bloom_combineFs.glsl into the 8-bit default framebuffer, glfwSwapBuffers at :267 puts it on the screen).  This card has no display
 *      engine: the frame reaches a screen, an encoder or a file through host memory, as the 4 B per pixel those consume.
 *      rt_display_pack: dImage (device, width*height rgba32f: gColor, rt_frame's dDisplay -- the image BEFORE this
 *      quantisation --, a TAA history slot, rt_shade_rays' colour) -> dOut (device, width*height*4 bytes: R, G, B, A in byte
 *      order, rows tightly packed).  Both pointers 16-byte aligned; the two ranges must not overlap.  Asynchronous on
 *      hipStream (NULL = the context's stream).  Per colour channel x, all in fp32:
 *        y = x * exposure;  NaN -> 0;  y <= 0 (with -0, -inf) -> 0;  y >= 1 (with +inf) -> 255;  otherwise
 *        RT_DISPLAY_RGBA8_LINEAR  q = rint(y * 255.0f), round to nearest even: GL's float -> UNORM8 conversion, what the
 *                                 reference's framebuffer stores (it never enables GL_FRAMEBUFFER_SRGB);
 *        RT_DISPLAY_RGBA8_SRGB    q = the number of i in 1..255 with T[i] <= y, T[i] = the fp32 nearest to
 *                                 f((i - 0.5) / 255) evaluated in double, f(s) = s / 12.92 for s <= 0.04045, else
 *                                 ((s + 0.055) / 1.055)^2.4: the sRGB code whose decoded value interval holds y.
 *      Alpha out is 255: every surface's alpha is the constant 1.0 (raytracingCs.glsl:581-583, bloom_combineFs.glsl:13).
 *      exposure must be finite and > 0; unknown format or flag bits and non-zero reserved words are refused.
 *      rt_display_srgb_thresholds: the table T (out[0] = 0), built on the host; needs no GPU. */
typedef enum rt_display_format { RT_DISPLAY_RGBA8_LINEAR = 0, RT_DISPLAY_RGBA8_SRGB = 1 } rt_display_format;
#define RT_DISPLAY_FLIP_ROWS 1u   /* output row 0 = TOP image row (file / encoder order); default keeps row 0 = bottom */
typedef struct rt_display_desc {
    int32_t width, height;
    int32_t format;                  /* rt_display_format */
    uint32_t flags;                  /* RT_DISPLAY_FLIP_ROWS */
    float exposure;
    int32_t reserved[3];             /* zero */
} rt_display_desc;
int rt_display_pack(rt_context *ctx, const void *dImage, void *dOut, const rt_display_desc *desc, void *hipStream);
int rt_display_srgb_thresholds(float out[256]);

/* ---- pipelined delivery of packed frames to the host.  A ring of `slots` (2..8, default 3) entries, each a device staging
 *      buffer, a pinned host buffer and an event.  rt_present_submit packs dImage (as rt_display_pack) into the next slot on
 *      hipStream (NULL = the context's stream) and has a context-owned non-blocking copy stream move the 4 B per pixel to the
 *      slot's pinned buffer behind it; it returns a ticket (0, 1, 2, ...; slot = ticket % slots) and does not block the host
 *      in steady state.  Two consequences:
 *        - dImage is consumed in hipStream's order: work enqueued on hipStream after rt_present_submit returns may overwrite
 *          it at once (the next frame's render into the same surface, for one);
 *        - the copy is not in hipStream's order: it overlaps whatever the caller launches next.
 *      rt_present_wait blocks the host until THAT ticket's copy is complete, and on nothing else; it returns the slot's pinned
 *      pixels (rt_display_pack's layout) and width*height*4.  The pointer stays valid until the submit of ticket + slots,
 *      which reuses the slot; a ticket older than that has expired and, like one not issued yet, gives RT_ERR_INVALID_ARG.
 *      Waiting twice on a live ticket is allowed.  rt_present_poll: the same rules without blocking (*ready = 0 or 1).
 *      A slot's buffers grow when the slot is next used for a larger frame, after a host wait for that slot's own last copy
 *      (the rule of the post passes' scratch); other slots' tickets stay valid.  rt_present_configure changes the slot count
 *      and expires every ticket issued so far; it is refused (RT_ERR_INVALID_ARG) while a ticket is outstanding: live and not
 *      yet seen complete by the host (returned by rt_present_wait, or reported ready by rt_present_poll).  rt_destroy waits
 *      for the copies in flight.  The loop of a host that shows frame k - 1 while frame k renders:
 *          rt_frame(ctx, &p, &d, dDisplay);                                (or any producer of an rgba32f surface)
 *          rt_present_submit(ctx, dDisplay, &desc, NULL, &t);  if (t) rt_present_wait(ctx, t - 1, &pixels, &bytes);
 *      Multi-GPU frames (rt_mgpu_*) have no delivery of their own: the root's surfaces and stream (rt_mgpu_get_surfaces) can
 *      be passed to rt_present_submit of a context on the root device. */
int rt_present_configure(rt_context *ctx, int slots);
int rt_present_submit(rt_context *ctx, const void *dImage, const rt_display_desc *desc, void *hipStream, uint64_t *ticket);
int rt_present_poll(rt_context *ctx, uint64_t ticket, int *ready);
int rt_present_wait(rt_context *ctx, uint64_t ticket, const void **hostPixels, size_t *bytes);

/* ---- exposure metering: what turns the HDR surfaces above into an `exposure` for the pack without a read-back.  The
 *      reference has no counterpart (it clips at 1); this is the auto-exposure with eye adaptation every HDR display path has.
 *      rt_meter: dImage (device, width*height rgba32f, 16-byte aligned, alpha ignored) -> dState (device, one rt_meter_state,
 *      16-byte aligned, owned by the caller).  Asynchronous on hipStream (NULL = the context's stream): a clear, a histogram
 *      kernel and a one-workgroup solve kernel in stream order, no host synchronisation.  The caller zeroes the state once
 *      (frames == 0) and passes it to every later call; a call reads only `exposure` and `frames` of the previous state and
 *      overwrites everything else.  All arithmetic is fp32 without fused multiply-add, or integer:
 *        Y = (0.2126f*r + 0.7152f*g) + 0.0722f*b;
 *        Y NaN -> nNaN;  Y == +inf -> nInf;  !(Y > 0) (with -0, -inf) -> nNonPositive;  otherwise the pixel is METERED:
 *        bin = clamp((bits(Y) >> 20) - 888, 0, 255): 8 bins per octave, linear in the top three mantissa bits, over
 *        2^-16 <= Y < 2^16; smaller Y (denormals too) in bin 0, larger in bin 255.  minLum / maxLum: the extremes of the
 *        metered Y, bit-exact (+inf / 0 when no pixel is metered).  sum(hist) + nNaN + nInf + nNonPositive == nPixels.
 *      Solve, on the device behind the histogram (integer atomics only: the state is bit-identical from run to run):
 *        n = sum(hist); lo = n*lowPermille/1000, hi = n*highPermille/1000 (64-bit floor division); hist' = hist with lo
 *        counts removed walking the bins upward, then hi counts walking downward; nMetered = n' = n - lo - hi;
 *        S = sum(hist'[b] * q[b]), q[b] = (b>>3)*65536 + log2q16[b&7];  meanLog2Q16 = m = S / n' (uint64 floor division):
 *        m/65536 - 16 is the log2 of the trimmed geometric-mean luminance to within a bin;
 *        target = clamp(key * ldexpf(pow2neg[(m>>8)&255], 16 - (m>>16)), minExposure, maxExposure): one fp32 multiply;
 *        n' == 0: target = the stored exposure when frames != 0 and it is finite and > 0, else 1.0f;
 *        exposure = target when frames == 0, the stored exposure is not finite and > 0, or adapt >= 1; otherwise
 *        old + (target - old) * adapt (a subtraction, a multiplication, an addition, in that order);
 *        frames = frames + 1, saturating at 2^32 - 1.  `hist` stays the untrimmed histogram.
 *      rt_meter_tables: pow2neg[f] = the fp32 nearest to 2^(-f/256), log2q16[j] = round(65536*log2(1 + (j+0.5)/8)), both
 *      evaluated in double on the host.  rt_meter_solve_host: the same solve (one source, csrc/rt_meter.h) from in->hist,
 *      in->exposure and in->frames; the counters and minLum / maxLum are copied; out may be in.  Neither needs a GPU.
 *      Refused with RT_ERR_INVALID_ARG: NULL context, descriptor, image or state; a pointer not 16-byte aligned; width or
 *      height < 1; key not finite and > 0; not 0 < minExposure <= maxExposure < inf; adapt outside (0, 1]; a negative
 *      permille or lowPermille + highPermille >= 1000; non-zero reserved words.  width*height > 2^31 - 1 (rt_meter) or
 *      sum(hist) > 2^32 - 1 (rt_meter_solve_host): RT_ERR_TOO_LARGE. */
typedef struct rt_meter_desc {
    int32_t width, height;
    float key;                         /* target mid-grey, e.g. 0.18 */
    float minExposure, maxExposure;
    float adapt;                       /* in (0, 1]; 1 = follow the image at once */
    int32_t lowPermille, highPermille; /* share of the metered pixels dropped at each end */
    int32_t reserved[4];               /* zero */
} rt_meter_desc;
typedef struct rt_meter_state {
    uint32_t hist[256];
    uint32_t nPixels, nNonPositive, nNaN, nInf;
    float minLum, maxLum;
    uint32_t nMetered;                 /* n' */
    uint32_t meanLog2Q16;              /* m; 0 when n' == 0 */
    float target, exposure;
    uint32_t frames;
    uint32_t reserved[5];
} rt_meter_state;
#define RT_METER_EXPOSURE_OFFSET 1060  /* offsetof(rt_meter_state, exposure): the device float rt_tone_desc.dExposure takes */
int rt_meter(rt_context *ctx, const void *dImage, const rt_meter_desc *desc, void *dState, void *hipStream);
int rt_meter_solve_host(const rt_meter_state *in, const rt_meter_desc *desc, rt_meter_state *out);
int rt_meter_tables(float pow2neg[256], uint32_t log2q16[8]);

/* ---- tone curves and a device-resident exposure in the pack.  rt_display_pack_toned / rt_present_submit_toned are
 *      rt_display_pack / rt_present_submit (layout, flip, formats, ring, refusals; one ring serves both submits) with, per
 *      colour channel x:
 *        e = desc->exposure * (*dExposure): one fp32 multiply, the float read on the device in hipStream's order -- e.g.
 *            (char *)dState + RT_METER_EXPOSURE_OFFSET behind rt_meter on the same stream; dExposure == NULL: e = desc->exposure;
 *        y = x * e;  NaN and !(y > 0) -> 0;  otherwise t = curve(min(y, 65536.0f)), every operation rounded to fp32, IEEE division:
 *        RT_TONE_NONE      t = y;
 *        RT_TONE_REINHARD  invW2 = 1.0f/(white*white) (host);  a = y*invW2; b = 1+a; c = y*b; d = 1+y; t = c/d  (white maps to 1);
 *        RT_TONE_ACES      n = y*((2.51f*y)+0.03f); d = (y*((2.43f*y)+0.59f))+0.14f; t = n/d  (Narkowicz's fit);
 *        then rt_display_pack's rule on t: t >= 1 -> 255, else LINEAR rint(t*255) or the sRGB threshold count.
 *      With RT_TONE_NONE and dExposure == NULL the bytes are rt_display_pack's.  Refused (RT_ERR_INVALID_ARG) beyond
 *      rt_display_pack's refusals: NULL tone description, unknown op, REINHARD with white not finite or < 1/256, dExposure not
 *      4-byte aligned, non-zero reserved words.  The frame loop with auto-exposure, no host round trip anywhere:
 *          rt_frame(ctx, &p, &d, dDisplay);  rt_meter(ctx, dDisplay, &m, dState, NULL);
 *          tone.dExposure = (char *)dState + RT_METER_EXPOSURE_OFFSET;
 *          rt_present_submit_toned(ctx, dDisplay, &desc, &tone, NULL, &t);  if (t) rt_present_wait(ctx, t - 1, &pixels, &bytes); */
typedef enum rt_tone_op { RT_TONE_NONE = 0, RT_TONE_REINHARD = 1, RT_TONE_ACES = 2 } rt_tone_op;
typedef struct rt_tone_desc {
    int32_t op;                      /* rt_tone_op */
    float white;                     /* REINHARD: the y that maps to 1; ignored otherwise */
    const void *dExposure;           /* device float, or NULL */
    int32_t reserved[4];             /* zero */
} rt_tone_desc;
int rt_display_pack_toned(rt_context *ctx, const void *dImage, void *dOut, const rt_display_desc *desc, const rt_tone_desc *tone,
                          void *hipStream);
int rt_present_submit_toned(rt_context *ctx, const void *dImage, const rt_display_desc *desc, const rt_tone_desc *tone,
                            void *hipStream, uint64_t *ticket);

/* ---- YUV 4:2:0 video output: what a video encoder takes where a screen or an image writer takes RGBA8.
 *      rt_display_pack_yuv: dImage (device, width*height rgba32f, as rt_display_pack) -> dOut (device, `bytes` of the layout below).
 *      Both pointers 16-byte aligned; the two ranges must not overlap.  Asynchronous on hipStream (NULL = the context's stream).
 *      Codes: for every pixel and colour channel, R, G, B in 0..255 are exactly the bytes rt_display_pack_toned writes for
 *        format = desc->transfer, desc->exposure, the same tone description and *dExposure (tone == NULL: RT_TONE_NONE, no
 *        dExposure), the NaN / <= 0 / >= 1 rules included.
 *      Rows: output luma row j is image row j; with RT_DISPLAY_FLIP_ROWS it is image row height-1-j.  Everything below is in
 *        OUTPUT rows, so for an odd height a flipped frame pairs other image rows into a chroma sample than an unflipped one.
 *      Luma, per pixel:  Y = yOff + ((cYR*R + cYG*G + cYB*B + 32768) >> 16).
 *      Chroma, one sample per 2x2 block of output pixels, sited at the block's centre: Rs, Gs, Bs = the sums of the four codes;
 *        a block that reaches past the right or top edge of an odd-sized frame replicates the edge pixel (coordinates clamped
 *        to width-1 / height-1);  Cb = clamp(128 + ((cBR*Rs + cBG*Gs + cBB*Bs + 131072) >> 18), 0, 255), Cr alike with cR*.
 *        >> on the signed 32-bit sum is arithmetic (floor); every sum fits in int32.
 *      Coefficients (rt_display_yuv_coeffs; Q16, built on the host in double, rne = round to nearest even):
 *        BT709: Kr, Kb = 0.2126, 0.0722;  BT601: 0.299, 0.114.  LIMITED: sY = 219/255, sC = 224/255, yOff = 16;  FULL: sY = sC = 1,
 *        yOff = 0.   cYR = rne(65536*Kr*sY), cYB = rne(65536*Kb*sY), cYG = rne(65536*sY) - cYR - cYB (white gives exactly 235 / 255);
 *        cBB = cRR = rne(32768*sC), cBR = rne(-65536*sC*Kr/(2*(1-Kb))), cRB = rne(-65536*sC*Kb/(2*(1-Kr))), cBG = -cBB - cBR,
 *        cRG = -cRR - cRB (each chroma row sums to 0: every grey gives exactly 128).
 *        out[12] = {cYR, cYG, cYB, yOff, cBR, cBG, cBB, 0, cRR, cRG, cRB, 0}.  LIMITED keeps Y in 16..235 and chroma in 16..240
 *        without the clamp; FULL reaches 256 in chroma before it.
 *      Layout (rt_display_yuv_layout; tightly packed, cw = (width+1)/2, ch = (height+1)/2, bytes = width*height + 2*cw*ch):
 *        RT_YUV_NV12: Y plane width x height at offset 0, then one plane of interleaved Cb, Cr, 2*cw x ch bytes, at width*height
 *                     (offset[2] = offset[1] + 1, pitch[1] = pitch[2] = 2*cw);
 *        RT_YUV_I420: Y, then Cb cw x ch at width*height, then Cr at width*height + cw*ch (pitch cw).
 *      rt_present_submit_yuv: rt_present_submit with this pack.  One ring and one ticket sequence serve every submit; the slot's
 *        buffers are sized by the frame's `bytes`; rt_present_wait returns the buffer and `bytes`, the planes are found with
 *        rt_display_yuv_layout.  The frame loop feeding an encoder:
 *          rt_frame(ctx, &p, &d, dDisplay);
 *          rt_present_submit_yuv(ctx, dDisplay, &yuv, NULL, NULL, &t);  if (t) rt_present_wait(ctx, t - 1, &frame, &bytes);
 *      Refused with RT_ERR_INVALID_ARG: NULL context, descriptor or pointers; misaligned or overlapping ranges; width or height
 *      < 1; unknown format / matrix / range / transfer; unknown flag bits; exposure not finite and > 0; non-zero reserved words;
 *      rt_display_pack_toned's refusals of a tone description.  RT_ERR_TOO_LARGE: more pixel blocks than one launch holds.
 *      rt_display_yuv_coeffs and rt_display_yuv_layout need no GPU; the layout reads width, height and format only. */
typedef enum rt_yuv_format { RT_YUV_NV12 = 0, RT_YUV_I420 = 1 } rt_yuv_format;
typedef enum rt_yuv_matrix { RT_YUV_BT709 = 0, RT_YUV_BT601 = 1 } rt_yuv_matrix;
typedef enum rt_yuv_range { RT_YUV_LIMITED = 0, RT_YUV_FULL = 1 } rt_yuv_range;
typedef struct rt_yuv_desc {
    int32_t width, height;           /* >= 1; odd sizes allowed */
    int32_t format, matrix, range;   /* rt_yuv_format, rt_yuv_matrix, rt_yuv_range */
    int32_t transfer;                /* rt_display_format: how the R'G'B' codes are made (LINEAR / SRGB) */
    uint32_t flags;                  /* RT_DISPLAY_FLIP_ROWS */
    float exposure;                  /* finite, > 0 */
    int32_t reserved[4];             /* zero */
} rt_yuv_desc;
int rt_display_yuv_coeffs(int matrix, int range, int32_t out[12]);
int rt_display_yuv_layout(const rt_yuv_desc *desc, size_t offset[3], size_t pitch[3], size_t *bytes);
int rt_display_pack_yuv(rt_context *ctx, const void *dImage, void *dOut, const rt_yuv_desc *desc, const rt_tone_desc *tone,
                        void *hipStream);
int rt_present_submit_yuv(rt_context *ctx, const void *dImage, const rt_yuv_desc *desc, const rt_tone_desc *tone, void *hipStream,
                          uint64_t *ticket);

/* ---- baseline JPEG output: the YUV pack's planes compressed on the device into a JFIF file any decoder opens (the chip has no
 *      encode block).  Every byte below is normative: tests/jpeg_oracle.py restates it in numpy and the device is
 *      compared with it bit for bit.
 *      Input: the planes of rt_display_pack_yuv (NV12 or I420, found through rt_display_yuv_layout).  Plane row 0 is the file's
 *        top row: pack with RT_DISPLAY_FLIP_ROWS for an upright file.  JFIF means full-range BT.601 with centre-sited 4:2:0, which
 *        is what the pack writes for matrix = RT_YUV_BT601, range = RT_YUV_FULL.
 *      Geometry: 1 <= width, height <= 65535; 4:2:0; MCU = 16x16 luma, mw = (width+15)/16, mh = (height+15)/16, MCUs in raster order,
 *        blocks in an MCU Y00 Y01 Y10 Y11 Cb Cr; samples outside a plane replicate its edge (coordinates clamped to width-1 /
 *        height-1, and to cw-1 / ch-1 in chroma).
 *      Forward DCT, in int32: M[u][x] = rne(16384 * a(u) * cos((2x+1) u pi / 16)), a(0) = 1/(2 sqrt 2), a(u>0) = 1/2, built in double
 *        on the host (rt_jpeg_dct_matrix, out[u*8+x]).  With f = sample - 128:
 *          r[y][u] = (sum_x M[u][x] * f[y][x] + 1024) >> 11        F[v][u] = (sum_y M[v][y] * r[y][u] + 65536) >> 17
 *        (>> arithmetic).  |AC| <= 1020 and -1024 <= DC <= 1016 over the sign patterns of the 64 basis functions.
 *      Quantiser: Annex K.1 (luma) / K.2 (chroma) scaled the IJG way, s = quality < 50 ? 5000/quality : 200 - 2*quality,
 *        Q = clamp((base*s + 50) / 100, 1, 255) (rt_jpeg_quant, natural order);  q = sign(F) * ((|F| + (Q >> 1)) / Q).
 *      Entropy coding: baseline Huffman, the typical tables K.3 / K.5 (luma) and K.4 / K.6 (chroma).  DC: the difference to the
 *        previous block of the same component (category 0..11); AC: (run, size) symbols, ZRL 0xF0 for runs above 15, EOB 0x00 when
 *        zeros trail; magnitude bits v for v >= 0, else v + 2^size - 1; bits MSB first.  A restart segment is restartInterval
 *        consecutive MCUs (the last may be shorter): the three DC predictors start at 0, the last partial byte is padded with
 *        1-bits, every 0xFF data byte (a padded one included) is followed by 0x00, and behind every segment but the last comes
 *        FF D0+(segment & 7).
 *      Header, 629 bytes: SOI; APP0 JFIF 1.01, units 0, density 1x1, no thumbnail; DQT 0; DQT 1 (own segments, 8-bit, zigzag);
 *        SOF0 (8, height, width, (1, 0x22, 0), (2, 0x11, 1), (3, 0x11, 1)); DHT DC0, AC0, DC1, AC1; DRI (always); SOS ((1, 0x00),
 *        (2, 0x11), (3, 0x11), 0, 63, 0).  The stream ends with EOI.  rt_jpeg_header writes the header into buf (cap >= 629).
 *      rt_jpeg_layout: the scratch of one encode.  offset[0]: the quantised coefficients, int16, zigzag order, 64 per block, 6 blocks
 *        per MCU, MCU order.  offset[1]: uint32[nSegments + 1], the byte offset of every segment within the entropy-coded data (its
 *        RST marker counted with it), the last entry their sum.  offset[2]: private -- two uint32 per segment, then room for
 *        the YUV planes of rt_display_pack_jpeg, so ONE layout serves both entry points.  Both documented planes are complete
 *        when the encode is, overflow or not.  worstBytes = 629 + nMcu*2488 + 2*(nSegments-1) + 2 (a block is at most 20 + 63*26
 *        bits, stuffing doubles it); RT_ERR_TOO_LARGE above 2^32 - 1.
 *      rt_jpeg_encode: dPlanes -> dOut, asynchronous on hipStream (NULL = the context's), no host synchronisation.  Of `planes`
 *        width, height and format are read.  dState receives one rt_jpeg_state.  When needed > capBytes: overflow = 1, bytes = 0,
 *        needed still exact, and nothing in dOut is written.  All pointers 16-byte aligned; planes, scratch, output (capBytes) and
 *        state must not overlap.
 *      rt_display_pack_jpeg: rt_display_pack_yuv into the scratch's private region, then rt_jpeg_encode; refused unless matrix is
 *        RT_YUV_BT601 and range RT_YUV_FULL.  rt_present_submit_jpeg: the same through the present ring, one ring and one ticket
 *        sequence with every other submit; the slot holds [64-byte rt_jpeg_state][stream], capBytes = 0 means worstBytes, the
 *        scratch is the context's; rt_present_wait returns the slot (64 + capBytes bytes), the stream is `bytes` long behind
 *        the state.
 *      Refused with RT_ERR_INVALID_ARG: NULL context, descriptions, pointers or ticket; misaligned or overlapping ranges; width or
 *      height outside 1..65535; quality outside 1..100; restartInterval outside 1..65535; non-zero reserved words; planes of
 *      another size or an unknown format; rt_display_pack_yuv's refusals.  rt_jpeg_dct_matrix, rt_jpeg_quant, rt_jpeg_header and
 *      rt_jpeg_layout need no GPU. */
typedef struct rt_jpeg_desc {
    int32_t width, height;           /* 1..65535 */
    int32_t quality;                 /* 1..100 */
    int32_t restartInterval;         /* MCUs per restart segment, 1..65535 */
    int32_t reserved[4];             /* zero */
} rt_jpeg_desc;
typedef struct rt_jpeg_state {
    uint32_t bytes;                  /* the stream's length in dOut; 0 on overflow */
    uint32_t needed;                 /* the stream's length, whether it fitted or not */
    uint32_t overflow;               /* 1: needed > capBytes, dOut untouched */
    uint32_t nSegments, nMcu;
    uint32_t headerBytes;            /* 629 */
    uint32_t stuffedBytes;           /* 0x00 bytes inserted behind 0xFF */
    uint32_t reserved[9];            /* zero */
} rt_jpeg_state;
int rt_jpeg_dct_matrix(int32_t out[64]);
int rt_jpeg_quant(int quality, uint8_t luma[64], uint8_t chroma[64]);
int rt_jpeg_header(const rt_jpeg_desc *desc, uint8_t *buf, size_t cap, size_t *n);
int rt_jpeg_layout(const rt_jpeg_desc *desc, size_t offset[3], size_t *scratchBytes, size_t *worstBytes);
int rt_jpeg_encode(rt_context *ctx, const void *dPlanes, const rt_yuv_desc *planes, const rt_jpeg_desc *desc, void *dScratch, void *dOut,
                   size_t capBytes, void *dState, void *hipStream);
int rt_display_pack_jpeg(rt_context *ctx, const void *dImage, const rt_yuv_desc *yuv, const rt_tone_desc *tone, const rt_jpeg_desc *desc,
                         void *dScratch, void *dOut, size_t capBytes, void *dState, void *hipStream);
int rt_present_submit_jpeg(rt_context *ctx, const void *dImage, const rt_yuv_desc *yuv, const rt_tone_desc *tone, const rt_jpeg_desc *desc,
                           size_t capBytes, void *hipStream, uint64_t *ticket);

/* ---- resampling in linear light, in front of rt_meter / rt_display_pack* / rt_present_submit*: render at one size, deliver
 *      another (4K -> 1080p is 4x supersampling; a fraction of the output size scaled up keeps a heavy scene at display rate).
 *      rt_display_resample: dSrc (device, srcWidth*srcHeight rgba32f) -> dDst (device, dstWidth*dstHeight rgba32f), any ratio,
 *      the axes independent.  Both pointers 16-byte aligned; the two ranges must not overlap.  Asynchronous on hipStream (NULL =
 *      the context's stream).  Separable, horizontal first, every channel (alpha included) alike, in fp32 with separate
 *      multiplies and adds (never fused), the accumulator starting as the first product and the taps in table order:
 *        h[r][i] = (((wx[i][0]*s[r][X(i,0)]) + wx[i][1]*s[r][X(i,1)]) + ...)    X(i,k) = clamp(firstx[i]+k, 0, srcWidth-1)
 *        d[j][i] = (((wy[j][0]*h[Y(j,0)][i]) + wy[j][1]*h[Y(j,1)][i]) + ...)    Y(j,k) = clamp(firsty[j]+k, 0, srcHeight-1)
 *      Edge pixels are replicated (the clamps).  Zero-weight padding taps are multiplied and added like any other, so by IEEE
 *      rules a NaN or infinite texel poisons every output whose window holds it (0 * inf = NaN), padding included.  With
 *      src size == dst size, AREA and TRIANGLE have one tap of weight 1: the call is a bit-exact copy.
 *      rt_resample_taps (host only, needs no GPU) returns the tables of one axis the kernel uses, source size S -> destination
 *      size D: *nTaps = n, the taps per destination index (the same for every index of the axis); first[D], the first source
 *      index of each window (it may be negative or reach past S-1); weights[D*n], weights[i*n+k].  first == weights == NULL
 *      asks for n only; otherwise capWeights is the capacity of `weights` in floats (below D*n: RT_ERR_TOO_LARGE) and `first`
 *      holds D entries.  Windows are decided in integers, weights evaluated in double and rounded to fp32 once:
 *        AREA (exact coverage): j0 = (i*S) div D, j1 = ((i+1)*S + D - 1) div D - 1,
 *          w_j = (min((i+1)*S, (j+1)*D) - max(i*S, j*D)) / S.
 *        TRIANGLE: f(x) = max(0, 1-|x|), R = 1.  LANCZOS3: f(x) = sinc(x)*sinc(x/3) for |x| < 3, R = 3, sinc exactly 1 at 0 and
 *          exactly 0 at every other x that is an integer in double.  fs = max(1, S/D), c = ((2i+1)*S - D) / (2*D); the window is
 *          the source pixels strictly inside c +- R*fs; w_j = f(x_j) / sum f, x_j = (j-c)/fs evaluated as the one quotient
 *          (2*D*j - (2i+1)*S + D) / (2*max(S,D)), the sum taken in window order.
 *        n is the largest window of the axis; a shorter window starts at its own j0 and is padded with zero weights at the end.
 *      n > RT_RESAMPLE_MAX_TAPS: RT_ERR_TOO_LARGE (LANCZOS3 reaches about 1/10 scale, AREA 1/64).
 *      The context keeps device copies of the two axis tables, keyed by (S, D, filter) per axis: a frame loop of one shape
 *      builds them once; a new shape waits for the last launch that read the old tables, then rebuilds and uploads.
 *      Refused with RT_ERR_INVALID_ARG: NULL context, descriptor or pointers (rt_resample_taps: NULL nTaps, or exactly one of
 *      first / weights NULL); misaligned or overlapping ranges; a size < 1; an unknown filter; non-zero flags or reserved words.
 *      RT_ERR_TOO_LARGE: an axis over the tap cap or longer than 2^20 pixels; more than 2^31 - 1 tiles of 64 x 16 destination
 *      pixels (fewer rows per tile at large ratios).  The context stays usable after a refusal.  The 1080p loop off a 4K render:
 *          rt_render(ctx, &p4k);  rt_get_surfaces(ctx, &dColor, NULL, NULL);
 *          rt_display_resample(ctx, dColor, dSmall, &rs, NULL);  rt_meter(ctx, dSmall, &m, dState, NULL);
 *          rt_present_submit_toned(ctx, dSmall, &disp1080, &tone, NULL, &t); */
typedef enum rt_resample_filter { RT_RESAMPLE_AREA = 0, RT_RESAMPLE_TRIANGLE = 1, RT_RESAMPLE_LANCZOS3 = 2 } rt_resample_filter;
typedef struct rt_resample_desc {
    int32_t srcWidth, srcHeight, dstWidth, dstHeight;   /* >= 1, any ratio, the axes independent */
    int32_t filter;                                      /* rt_resample_filter */
    uint32_t flags;                                      /* zero */
    int32_t reserved[2];                                 /* zero */
} rt_resample_desc;
#define RT_RESAMPLE_MAX_TAPS 64
int rt_resample_taps(int srcSize, int dstSize, int filter, int *nTaps, int32_t *first, float *weights, size_t capWeights);
int rt_display_resample(rt_context *ctx, const void *dSrc, void *dDst, const rt_resample_desc *desc, void *hipStream);

/* ---- progressive accumulation: the running mean of many one-sample frames, and a convergence report that stays on the device.
 *      The accumulator (device, caller-owned, 16-byte aligned, all-zero = empty; rt_accum_layout gives offset[2] = {0,
 *      width*height*16} and bytes = width*height*32) is two planes of width*height float4:
 *        plane 0: the running MEAN rgba32f -- as it stands a valid input of rt_meter, rt_display_resample, every pack and every
 *                 present submit; there is no resolve pass;
 *        plane 1: {mY, M2, count (the bits of a uint32), 0}: Welford's moments of the sample luminance.
 *      The state (device, one rt_accum_state of 1 KiB, 16-byte aligned, caller-owned, zeroed once -- or by rt_accum_reset).
 *      rt_accum_add: dImage (device, width*height rgba32f, 16-byte aligned) is one more sample of every pixel.  Asynchronous on
 *      hipStream (NULL = the context's stream), no host synchronisation: a clear of the state except `frames`, the accumulate
 *      kernel, a one-workgroup solve, in stream order.  Per pixel, in fp32, never fused, IEEE division, in exactly this order:
 *        Y = (0.2126f*r + 0.7152f*g) + 0.0722f*b of the sample (rt_meter's formula).
 *        The sample is ACCEPTED when all four channels are finite with |x| <= 2^48 and count < 2^24; otherwise the pixel's 32
 *        bytes are left untouched and nRejected counts it.  With this bound and the floor's, no value the accumulator ever holds
 *        is NaN or infinite: |mean|, |mY| <= 2^48, every term of M2 is at most 2^49 * 2^49, so M2 <= 2^24 * 2^98 = 2^122 < 2^128;
 *        and m*m >= 2^-80 below is a normal number.
 *        Accepted:  n = count+1; nf = (float)n;  per channel d = x - mean; mean = mean + d/nf;
 *                   dY = Y - mY; mY' = mY + dY/nf; M2 = M2 + dY*(Y - mY');  mY = mY'; count = n.
 *        Afterwards, for EVERY pixel, on the state it now holds:
 *          count < 2: nUnsampled counts it.  Otherwise  nf = (float)count; q = M2/(nf*(nf-1.0f)); m = fmaxf(mY, lumFloor);
 *          r2 = q/(m*m) -- the squared relative standard error of the mean luminance -- and the pixel is BINNED:
 *          bin = !(r2 > 0) ? 0 : clamp((bits(r2) >> 21) - 396, 0, 127): four bins per octave over 2^-28 <= r2 < 2^4; hist[bin]++.
 *          It is CONVERGED (nConverged) when count >= minSamples && r2 <= thr2, thr2 = relError*relError (one fp32 multiply
 *          on the host).  minCount / maxCount run over all pixels, maxR2Bits = max bits(r2) over the binned ones (0: none).
 *          sum(hist) + nUnsampled == nPixels.
 *        Solve: with n = sum(hist), medianBin / p95Bin = the smallest bin whose cumulative count reaches ceil(n*500/1000) /
 *          ceil(n*950/1000) (64-bit integers; 0 when n == 0); done = nConverged*1000 >= (uint64)nPixels*donePermille;
 *          frames = frames+1, saturating at 2^32-1.  rt_accum_solve_host runs the same solve (one source for host and device)
 *          from in->hist, nUnsampled, nConverged, nPixels and frames without a GPU and copies the other words.
 *      Every reduction is an integer atomic: the state is bit-identical from run to run.
 *      rt_accum_view: dAccum -> dOut (device, width*height rgba32f (v,v,v,1), 16-byte aligned, not overlapping the accumulator):
 *        RT_ACCUM_VIEW_RELERR: v = sqrtf(r2), +inf where count < 2 (packs to white);  RT_ACCUM_VIEW_COUNT: v = (float)count;
 *        RT_ACCUM_VIEW_CONVERGED: v = 1 or 0.  The heat maps of where the noise is.
 *      rt_accum_reset: two asynchronous memsets; the accumulator is empty and the state zero (`frames` too) behind it.
 *      Refused before anything is enqueued, with RT_ERR_INVALID_ARG: NULL context, descriptor or pointer; a pointer not 16-byte
 *      aligned; dImage, dOut or dState overlapping the accumulator; width or height < 1; relError not finite and > 0; lumFloor
 *      not finite or < 2^-40; minSamples < 2; donePermille outside 1..1000; an unknown view mode; non-zero reserved words.
 *      RT_ERR_TOO_LARGE: width*height > 2^31 - 1; in rt_accum_solve_host, sum(hist) + nUnsampled above 2^32 - 1.  The context
 *      stays usable after a refusal and keeps no state of this feature.  The loop:
 *          rt_render(ctx, &p);  rt_get_surfaces(ctx, &dColor, NULL, NULL);  rt_accum_add(ctx, dColor, dAccum, &a, dState, NULL);
 *          every k frames a 4-byte read of dState + offsetof(rt_accum_state, done);
 *          rt_present_submit_toned(ctx, dAccum, &disp, &tone, NULL, &t);          (plane 0 is the image) */
typedef enum rt_accum_view_mode { RT_ACCUM_VIEW_RELERR = 0, RT_ACCUM_VIEW_COUNT = 1, RT_ACCUM_VIEW_CONVERGED = 2 } rt_accum_view_mode;
typedef struct rt_accum_desc {
    int32_t width, height;           /* >= 1 */
    float relError;                  /* target relative standard error of a pixel's mean luminance: finite, > 0 (e.g. 0.02f) */
    float lumFloor;                  /* finite, >= 2^-40: a mean luminance below it is judged against the floor instead */
    int32_t minSamples;              /* >= 2: a pixel with fewer accepted samples is never converged */
    int32_t donePermille;            /* 1..1000: the share of all pixels that must be converged for state.done */
    int32_t reserved[4];             /* zero */
} rt_accum_desc;
typedef struct rt_accum_state {
    uint32_t hist[128];              /* pixels per bin of r2, four bins per octave */
    uint32_t nPixels, nUnsampled, nConverged, nRejected;
    uint32_t minCount, maxCount, maxR2Bits;
    uint32_t medianBin, p95Bin, done, frames;
    uint32_t reserved[117];          /* zero */
} rt_accum_state;
int rt_accum_layout(int width, int height, size_t offset[2], size_t *bytes);
int rt_accum_reset(rt_context *ctx, void *dAccum, void *dState, int width, int height, void *hipStream);
int rt_accum_add(rt_context *ctx, const void *dImage, void *dAccum, const rt_accum_desc *desc, void *dState, void *hipStream);
int rt_accum_solve_host(const rt_accum_state *in, const rt_accum_desc *desc, rt_accum_state *out);
int rt_accum_view(rt_context *ctx, const void *dAccum, void *dOut, const rt_accum_desc *desc, int mode, void *hipStream);

/* ---- denoising: the spatial half of SVGF -- a variance-guided 5x5 B3-spline a-trous wavelet filter, steered by first-hit records.
 *      It makes the first frames of a still view presentable while the accumulator converges.  Three device planes of
 *      width*height 16-byte records go in, one comes out, all caller-owned and 16-byte aligned:
 *        dImage:   rgba32f -- the accumulator's plane 0, or one raw frame;
 *        dMoments: the accumulator's plane 1 {mY, M2, count (the bits of a uint32), 0}, or NULL (every count reads as 1);
 *        dGuide:   rt_denoise_guide_rec records {n[3], object}, made once per still view by rt_denoise_guide from the rt_hit
 *                  records of rt_camera_rays -> rt_trace_rays(RT_QUERY_CLOSEST).  The render's own gPosition / gNormal are the
 *                  path's LAST hit and change with frameCount; the first hit is exact and still.  The plane is dense on purpose:
 *                  a tap gathered from the upper half of 32-byte rt_hit records would touch twice the cache lines;
 *        dScratch: two planes A, B of width*height float4 (rt_denoise_layout: offset[2] = {0, width*height*16}, bytes =
 *                  width*height*32), holding (r, g, b, var);
 *        dOut:     rgba32f -- as it stands a valid input of rt_meter, rt_display_resample, every pack and every present submit.
 *      Asynchronous on hipStream (NULL = the context's stream), no host synchronisation, and the context keeps no state of the
 *      feature: rt_denoise_guide is one launch, rt_denoise is 1 + iterations launches in stream order.  All arithmetic is fp32,
 *      never fused, with IEEE divide and sqrt; exp_ is rtm::exp_ of csrc/rt_mesa_math.h (one source for host and device).  Every
 *      sum below starts at +0 and adds the kept terms one by one in row-major order of the window (dy outer, dx inner); max0(x)
 *      is x > 0 ? x : 0 and min1(x) is x < 1 ? x : 1 (fmaxf / fminf that give +0 for -0 and drop a NaN).
 *      Y(r, g, b) = (0.2126f*r + 0.7152f*g) + 0.0722f*b, rt_meter's and the accumulator's luminance.
 *      GUIDE.  s = (nx*nx + ny*ny) + nz*nz of the hit's normal;  s > 0: n^ = n / sqrtf(s) per component, otherwise n^ = 0; object
 *        is copied.  A plane's raw, unnormalised normal becomes the unit normal; a miss (object -1, normal 0) stays 0.  The
 *        hits' normals are finite, as rt_trace_rays' are; a normal too short or too long for s to be a normal number loses its
 *        direction (s == 0 or s == inf both give n^ = 0, and such a pixel passes through the filter unchanged).
 *      PREPARE (dImage, dMoments, dGuide -> plane A).  A pixel is USABLE when r, g and b are finite with |x| <= 2^48; otherwise it
 *        is SKIPPED everywhere below: it is never a tap of another pixel, and is itself filled from its neighbours.  The mark of a
 *        skipped pixel is the sign bit of var: it stores (r, g, b, -0.0f), as it does in every later plane; a usable pixel's var is
 *        never negative (M2 is the accumulator's: >= +0).  For a usable pixel, count = the moments' count (1 without moments):
 *          count >= minCount:  nf = (float)count;  var = M2 / (nf*(nf - 1.0f));
 *          otherwise the spatial estimate: over the k usable pixels of the 5x5 window (stride 1) that lie inside the image and have
 *          the centre's object (the centre is one of them):  m1 = sum(Y)/kf;  m2 = sum(Y*Y)/kf;  var = max0(m2 - m1*m1) /
 *          (float)max(count, 1).
 *        With the bound, as in the accumulator, every sum stays finite: |Y| <= 2^49, Y*Y <= 2^98, M2 <= 2^122, var <= 2^121, a
 *        weight is at most about 1, so 25 terms of w*rgb stay below 2^53 and 25 of (w*w)*var below 2^126.
 *      ITERATION i = 0 .. iterations-1, step d = 1 << i, reads one plane and writes the other (0: A -> B, 1: B -> A, ...); the
 *        last one writes dOut.  For the centre p with its record (rgb_p, var_p), guide (n^p, object_p) and Yp = Y(rgb_p):
 *          gv = sum(g*var_q) / sum(g) over the 3x3 window at stride 1 with g = gk[dx]*gk[dy], gk = {1/4, 1/2, 1/4}, taps outside the
 *            image, skipped or of another object dropped -- the variance of a neighbouring object must not reach across the edge
 *            either -- (sum(g) == 0: gv = 0);   sl = sigmaLum*sqrtf(gv) + lumEps;
 *          the 25 taps q = p + d*(dx, dy), dx, dy = -2..2, h = {1/16, 1/4, 3/8, 1/4, 1/16}: a tap is DROPPED when it lies outside the
 *            image (no clamping), when it is skipped, or when object_q != object_p.  For the others
 *              c = min1(max0((n^p.x*n^q.x + n^p.y*n^q.y) + n^p.z*n^q.z));   wn = c squared normalLog2Power times (c = c*c), or 1
 *              when object_p < 0 (sky filters with sky);   wl = fabsf(Yp - Yq) / sl, or 0 when p is skipped;
 *              w = ((h[dx]*h[dy]) * wn) * exp_(-wl);
 *          sw = sum(w);  rgb' = sum(w*rgb_q) / sw per channel;  var' = sum((w*w)*var_q) / (sw*sw);
 *          sw == 0 (p skipped without a usable neighbour of its object, or n^p = 0): rgb' = rgb_p, var' = 0.
 *          A skipped p stores var' = -0.0f whatever the sums say.  The last iteration stores dImage's alpha of the pixel instead
 *          of var'.
 *      Refused before anything is enqueued, with RT_ERR_INVALID_ARG: NULL context, descriptor or pointer (except dMoments); a
 *      pointer not 16-byte aligned; dOut or dScratch overlapping an input or each other, dGuide overlapping dHits; width or height
 *      < 1; iterations outside 1..5; normalLog2Power outside 0..7; sigmaLum not finite and > 0; lumEps not finite or < 2^-40;
 *      minCount < 2; non-zero reserved words.  RT_ERR_TOO_LARGE: width*height > 2^31 - 1.  The context stays usable.  The loop:
 *          once per still view:  rt_camera_rays(ctx, &p, dRays, s);  rt_trace_rays(ctx, dRays, n, RT_QUERY_CLOSEST, dHits, s);
 *                                rt_denoise_guide(ctx, dHits, dGuide, w, h, s);
 *          at display cadence:   rt_render;  rt_accum_add(ctx, dColor, dAccum, &a, dState, s);
 *                                rt_denoise(ctx, dAccum, dAccum + w*h*16, dGuide, dScratch, dOut, &dn, s);
 *                                rt_present_submit_toned(ctx, dOut, &disp, &tone, s, &t); */
typedef struct rt_denoise_guide_rec { float n[3]; int32_t object; } rt_denoise_guide_rec;   /* one pixel of the guide plane */
typedef struct rt_denoise_desc {
    int32_t width, height;           /* >= 1 */
    int32_t iterations;              /* 1..5: steps 1, 2, 4, 8, 16 */
    int32_t normalLog2Power;         /* 0..7: the normal weight is the clamped cosine to the power 2^normalLog2Power */
    float sigmaLum;                  /* finite, > 0: luminance differences are measured in sigmaLum standard deviations */
    float lumEps;                    /* finite, >= 2^-40: added to that scale */
    int32_t minCount;                /* >= 2: a pixel with fewer samples takes the spatial variance estimate */
    int32_t reserved[5];             /* zero */
} rt_denoise_desc;
int rt_denoise_guide(rt_context *ctx, const void *dHits, void *dGuide, int width, int height, void *hipStream);
int rt_denoise_layout(int width, int height, size_t offset[2], size_t *bytes);
int rt_denoise(rt_context *ctx, const void *dImage, const void *dMoments, const void *dGuide, void *dScratch, void *dOut,
               const rt_denoise_desc *desc, void *hipStream);

/* ---- reprojection: the temporal half of SVGF -- the accumulator of the previous view carried over to a new camera, so that a camera
 *      move no longer means rt_accum_reset.  The scene is taken as static between the two views (a moved object is the caller's
 *      reason to reset).  Device buffers, all caller-owned and 16-byte aligned:
 *        dAccumPrev: the previous view's accumulator, both planes (rt_accum_layout; rt_reproject_layout gives the same answer);
 *        dHitsPrev, dHitsCur: width*height rt_hit records of rt_camera_rays -> rt_trace_rays(RT_QUERY_CLOSEST) for the previous and
 *                    the current view (the current ones are what rt_denoise_guide needs anyway);
 *        dAccumCur:  a second accumulator, written in full: the history every current pixel can legitimately keep, as it stands an
 *                    input of rt_accum_add, rt_denoise and the display path;
 *        dReport:    one rt_reproject_report (64 B).
 *      Asynchronous on hipStream (NULL = the context's stream), no host synchronisation, and the context keeps no state of the
 *      feature: a clear of the report (two memsets), then one kernel, in stream order.  All arithmetic is fp32, never fused, with IEEE divide and
 *      sqrt; dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
 *      VIEWS.  Of desc.prev and desc.cur only camPos, camDir, camRight, camUp, fovDeg, focalLength, width and height are read; both
 *        widths and heights must equal desc.width / desc.height.  The basis is taken as orthonormal, which is what rt_camera_vectors
 *        produces; with any other basis the projection is merely wrong, and the tap tests below turn that into lost history, never
 *        into false history.  Per view, on the host, exactly as the render does (rtm::tan_ of csrc/rt_mesa_math.h):
 *          tanFov = tan_((fovDeg * 0.017453292519943295f) * 0.5f);  sx = ((float)width / (float)height) * tanFov * focalLength;
 *          sy = tanFov * focalLength;   and for both  hx = 0.5f*(float)width,  hy = 0.5f*(float)height.
 *      PROJECTION proj(V, P):  v = P - camPos per component;  z = dot(v, camDir);  x = dot(v, camRight);  y = dot(v, camUp);
 *          valid iff z > 0 (a NaN fails);  fx = ((x / z) / sx + 1.0f) * hx - 0.5f;  fy = ((y / z) / sy + 1.0f) * hy - 0.5f.
 *        This inverts generateCameraRay's pixel -> uv map without its jitter: the centre of pixel (px, py) projects to (px, py).
 *        rt_reproject_project runs it on the host (one source for host and device): f[2] = {fx, fy}, *valid = 0 / 1.
 *      MOTION.  rt_camera_rays jitters every ray by up to a pixel, so the hit P of pixel p = (px, py) is not at the pixel's centre.
 *        The jitter is removed to first order by projecting P into BOTH views:  m = proj(prev, P) - proj(cur, P) per component;
 *        g = ((float)px + m.x, (float)py + m.y).  With identical views m is exactly (0, 0).
 *      CATEGORIES.  Every pixel falls into exactly one, in this order, and the report counts each:
 *        MISS:      object_p < 0.  Sky is not reprojected.
 *        OFFSCREEN: either projection is invalid, or g is not finite, or not (-1 < gx < (float)width and -1 < gy < (float)height)
 *                   -- tested in float before any conversion to integer.
 *        REJECTED:  no tap below is kept.
 *        REUSED:    otherwise.
 *        All but REUSED store 32 zero bytes: an empty pixel, exactly what rt_accum_reset leaves.
 *      TAPS.  x0 = (int)floorf(gx);  ax = gx - (float)x0;  likewise y0, ay.  The four taps q = (x0+i, y0+j), i, j = 0, 1, have the
 *        bilinear weights w = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay).  With n^ = (s = dot(n, n)) > 0 ? n / sqrtf(s) per
 *        component : 0 (rt_denoise_guide's rule) for the current normal n^p and the tap's n^q, a tap is DROPPED when any of
 *          w == 0;   q outside the image;   count_q == 0;   object_q != object_p;   dot(n^p, n^q) < normalCosMin;
 *          fabsf(dot(P - P_q, n^p)) > planeTol * t_p
 *        holds (comparisons as written: a NaN operand does not drop).  The last asks whether the previous hit lies in the current
 *        hit's tangent plane: exact for planes, second order for spheres, insensitive to the sub-pixel offsets of the two jitters.
 *      RESULT.  Sums run over the kept taps in the order (0,0), (1,0), (0,1), (1,1), starting at +0:
 *          sw = sum(w);   mean' = sum(w*mean_q) / sw per channel (alpha too);   mY' = sum(w*mY_q) / sw;
 *          s2_q = count_q >= 2 ? M2_q / (float)(count_q - 1) : 0;   s2' = sum(w*s2_q) / sw;
 *          n' = min(min over the kept taps of count_q, maxHistory);   M2' = s2' * (float)(n' - 1);
 *        plane 0 = mean', plane 1 = {mY', M2', bits(n'), 0}.  A single kept tap of weight 1 reproduces its mean and mY bit for bit
 *        (+0 + 1*x = x, x / 1 = x; a -0 comes out as +0) and M2 within two roundings.  Capping n' at maxHistory makes the next
 *        rt_accum_add weigh its sample at least 1 / (maxHistory + 1): that bounds the lag of a moving view.
 *        With the accumulator's own bounds (|mean|, |mY| <= 2^48; M2 <= count * 2^98, so s2_q <= 2^99) every sum stays finite: the
 *        weights are products of two numbers in [0, 1] that sum to at most 1 + 2^-22, so sum(w*x) <= 2^49 and sum(w*s2) <= 2^100; a
 *        quotient by sw is a weighted mean up to rounding -- at most twice the largest term even when w is denormal -- so
 *        |mean'|, |mY'| <= 2^50, s2' <= 2^101 and M2' <= 2^101 * 2^24 = 2^125 < 2^128.  2^24 further samples add at most 2^122.
 *      REPORT.  nReused + nRejected + nOffscreen + nMiss == nPixels = width*height;  minCount / maxCount = min / max of n' over the
 *        REUSED pixels (2^32 - 1 and 0 when there is none);  sumCount = sum of n' over them.  Every field is built with integer atomics: it
 *        is bit-identical from run to run, as is the accumulator (every pixel is a pure function of the inputs).
 *      Refused before anything is enqueued, with RT_ERR_INVALID_ARG: NULL context, descriptor or pointer; a pointer not 16-byte
 *      aligned; dAccumCur or dReport overlapping an input or each other; width or height < 1; a view whose width / height differ
 *      from the descriptor's; a fovDeg or focalLength for which sx or sy is not finite and > 0; normalCosMin not finite or outside
 *      [-1, 1]; planeTol not finite or < 0; maxHistory outside 1..2^24-1; non-zero reserved words.  RT_ERR_TOO_LARGE: width*height
 *      > 2^31 - 1.  The context stays usable.  rt_reproject_project refuses NULL pointers and such a view the same way.  The loop:
 *          view changes:  rt_camera_rays(ctx, &cur, dRays, s);  rt_trace_rays(ctx, dRays, n, RT_QUERY_CLOSEST, dHitsCur, s);
 *                         rt_accum_reproject(ctx, dAccumPrev, dHitsPrev, dHitsCur, dAccumCur, &desc, dReport, s);
 *                         swap(prev, cur) of the accumulators and of the hits;  rt_denoise_guide on the new hits
 *          every frame:   rt_render;  rt_accum_add(ctx, dColor, dAccum, &a, dState, s);  rt_denoise(...);  rt_present_submit_toned(...) */
typedef struct rt_reproject_desc {
    int32_t width, height;           /* >= 1 */
    rt_params prev, cur;             /* the two views; see VIEWS for the fields that are read */
    float normalCosMin;              /* finite, in [-1, 1]: a tap whose normal is turned further from the current one is dropped */
    float planeTol;                  /* finite, >= 0: distance of the tap's hit from the current tangent plane, in units of t_p */
    int32_t maxHistory;              /* 1..2^24-1: the most samples a reprojected pixel counts for */
    int32_t reserved[3];             /* zero */
} rt_reproject_desc;
typedef struct rt_reproject_report {
    uint32_t nPixels, nReused, nRejected, nOffscreen, nMiss;
    uint32_t minCount, maxCount;     /* of n' over the reused pixels; 2^32 - 1 and 0 when there is none */
    uint32_t reserved0;              /* zero */
    uint64_t sumCount;               /* of n' over the reused pixels */
    uint32_t reserved[6];            /* zero */
} rt_reproject_report;
int rt_reproject_layout(int width, int height, size_t offset[2], size_t *bytes);
int rt_reproject_project(const rt_params *view, const float P[3], float f[2], int *valid);
int rt_accum_reproject(rt_context *ctx, const void *dAccumPrev, const void *dHitsPrev, const void *dHitsCur, void *dAccumCur,
                       const rt_reproject_desc *desc, void *dReport, void *hipStream);

/* ---- adaptive sampling: the accumulator's convergence report as a scheduler -- trace only the pixels that have not converged.
 *      Three stages around rt_shade_rays; every call is asynchronous on hipStream (NULL = the context's stream), none synchronises
 *      with the host, every buffer is the caller's and the context keeps no state of this feature.
 *      rt_accum_select: dAccum (an accumulator, see above; read only) -> the list of pixels that still need samples.
 *        A pixel is SELECTED when it is not CONVERGED by exactly rt_accum_add's rule (desc's relError, lumFloor, minSamples; a pixel
 *        with count < 2 is unconverged) and its count < maxSamples.  maxSamples (1..2^24) is a budget cap: pixels that are unconverged
 *        but at the cap are counted in nCapped and not selected.  desc->donePermille is validated and not used.
 *        ORDER, part of the contract: the image is cut into tiles of 8 x 8 pixels; tiles go in raster order (tile = (y/8) *
 *        ceil(width/8) + x/8), pixels in raster order inside a tile; ragged tiles have fewer pixels.  64 consecutive entries lie in a
 *        few neighbouring tiles, which keeps rt_shade_rays' waves coherent and rt_accum_add_at's accesses compact.
 *        dPixels (device, rt_pixel, 8-byte aligned, room for `capacity` entries; may be NULL when capacity == 0): exactly the first
 *        nListed = min(nSelected, capacity) entries of that order are written and nothing behind them is touched; every store is
 *        checked against the capacity.  capacity == 0 gives a pure count.
 *        dSelState (device, one rt_select_state of 64 B, 16-byte aligned) is written whole by every call: nPixels; nSelected, the full
 *        number whatever the capacity; nListed; capacity (saturated at 2^32 - 1); overflow = nSelected > capacity; nCapped.
 *        dScratch (device, 16-byte aligned, rt_accum_select_layout's scratchBytes; content unspecified, need not be cleared).
 *        Form: per-tile ballots and popcounts, an exclusive integer scan of the totals, the emit -- three launches (two when
 *        capacity == 0) ordered by the stream alone; no workgroup waits for another; the result is bit-identical from run to run.
 *      rt_camera_rays_at: ray k (dRays: device, n rt_ray, 16-byte aligned) is the primary ray of IMAGE pixel dPixels[k] (device, n
 *        rt_pixel, 8-byte aligned) of rt_render_to(p): noise jitter, frameCount, the GL's tan, tMax = p->maxRayDistance -- bit-identical
 *        to the record rt_camera_rays(p) writes for that pixel.  The window and strip fields of p are ignored (p is validated with an
 *        identity window, as in rt_pick).  An entry outside the image gives the all-zero record and is never used as an address.
 *        n == 0 is a no-op.  Ordered with rt_set_noise as rt_camera_rays is.
 *      rt_accum_add_at: dSamples[k] (device, n rgba32f, 16-byte aligned -- rt_shade_rays' colour) is one more sample of pixel
 *        dPixels[k].  Per pixel the arithmetic is rt_accum_add's, to the letter: the same accept / reject (finite, |x| <= 2^48,
 *        count < 2^24), the same mean and Welford updates in the same order, unfused, IEEE division; a rejected sample leaves the
 *        pixel's 32 bytes untouched and counts in nRejected.  An entry with x >= width or y >= height is skipped, counted in
 *        nRejected and never forms an address.  Pixels not listed are not written at all.  The list must name a pixel at most once
 *        (rt_accum_select's lists do); with duplicates, which of the duplicate samples a pixel keeps is unspecified, but every access
 *        stays inside the accumulator.  Afterwards the statistics of rt_accum_add run over EVERY pixel on the state the accumulator
 *        now holds, then the solve with frames + 1: dState comes out exactly as rt_accum_add defines it (hist, nUnsampled,
 *        nConverged, min / max count, maxR2Bits, the bins, done).  n == 0 is legal -- a frame in which nothing needed sampling: it
 *        refreshes the report and counts a frame; dSamples and dPixels may then be NULL.
 *      Refused before anything is enqueued, with RT_ERR_INVALID_ARG: NULL context, descriptor or required pointer; a pointer not
 *      16-byte aligned (dPixels: 8); dPixels, dScratch, dSelState, dSamples or dState overlapping the accumulator; width or height
 *      < 1 and the accumulator descriptor's other refusals; maxSamples outside 1..2^24; non-zero reserved words; for
 *      rt_camera_rays_at whatever rt_pick's validation of p refuses.  RT_ERR_TOO_LARGE: width*height > 2^31 - 1; n beyond one grid
 *      (2^31 - 1 workgroups of 256).  The context stays usable after a refusal.  The loop, once the share rt_accum_select reports has
 *      dropped below the crossover (DESIGN.md 25 has the measurement; above it full frames -- rt_render + rt_accum_add -- are cheaper):
 *          every k frames:  rt_accum_select(ctx, dAccum, &a, maxSamples, dPixels, capacity, dScratch, dSel, s);
 *                           an 8-byte read of dSel + offsetof(rt_select_state, nSelected): nSelected and nListed (they differ
 *                           exactly when `overflow` is set) -- the read that already fetches rt_accum_state.done
 *          every frame:     p.frameCount++;  rt_camera_rays_at(ctx, &p, dPixels, nListed, dRays, s);
 *                           rt_shade_rays(ctx, &p, dRays, dPixels, nListed, dSamples, NULL, NULL, s);
 *                           rt_accum_add_at(ctx, dSamples, dPixels, nListed, dAccum, &a, dState, s);
 *      A list reused for k frames gives a few pixels a few samples more than they needed, which is harmless.  Stopping a pixel on
 *      its own estimated error biases it slightly (the known price of adaptive sampling); a pixel whose samples are always rejected
 *      is selected for ever, and `done` never counts it either. */
typedef struct rt_select_state {
    uint32_t nPixels, nSelected, nListed, capacity, overflow, nCapped;
    uint32_t reserved[10];           /* zero */
} rt_select_state;
int rt_accum_select_layout(int width, int height, size_t *scratchBytes);
int rt_accum_select(rt_context *ctx, const void *dAccum, const rt_accum_desc *desc, uint32_t maxSamples, void *dPixels, size_t capacity,
                    void *dScratch, void *dSelState, void *hipStream);
int rt_camera_rays_at(rt_context *ctx, const rt_params *p, const void *dPixels, size_t n, void *dRays, void *hipStream);
int rt_accum_add_at(rt_context *ctx, const void *dSamples, const void *dPixels, size_t n, void *dAccum, const rt_accum_desc *desc,
                    void *dState, void *hipStream);

/* ---- first-hit-guided upsampling: shade at a fraction of the resolution, trace first hits at full resolution, reconstruct the full
 *      frame by a joint bilateral filter that never mixes two surfaces, and re-shade exactly the pixels whose surface no
 *      low-resolution ray saw.  The cost of a frame is almost all shading; first hits are cheap and exact.  Where rt_display_resample
 *      -- a linear filter -- smears every silhouette across the two objects, this keeps it at full resolution.  Device buffers, all
 *      caller-owned and 16-byte aligned:
 *        dLow:      rgba32f, lowWidth*lowHeight -- a render's gColor at the low resolution, or a denoised plane;
 *        dHitsLow, dHitsHigh: lowWidth*lowHeight and width*height rt_hit records (32 B) of rt_camera_rays -> rt_trace_rays(
 *                   RT_QUERY_CLOSEST) for the low-resolution and the full-resolution rt_params of one view;
 *        dOut:      rgba32f, width*height, written in full -- as it stands a valid input of every image stage;
 *        dPixels:   rt_pixel, 8-byte aligned, room for `capacity` entries (may be NULL when capacity == 0): the HOLES;
 *        dScratch:  rt_upsample_layout's scratchBytes (the same answer as rt_accum_select_layout's; content unspecified, need not be
 *                   cleared);   dSelState: one rt_select_state (64 B), written whole.
 *      Asynchronous on hipStream (NULL = the context's stream), no host synchronisation, and the context keeps no state of the
 *      feature: the reconstruction, then rt_accum_select's scan and emit -- three launches (two when capacity == 0) in stream order.
 *      All arithmetic is fp32, never fused, with IEEE divide and sqrt; every sum starts at +0 and adds the kept terms one by one in
 *      the stated order.  max0, min1 and the normalisation n^ of a hit's normal are exactly rt_denoise's (GUIDE above), applied to the
 *      records of both hit planes inside the kernel: no guide plane is needed.
 *      POSITION of output pixel p = (x, y), in 64-bit integers (pixel centres of both grids over the same image; floor_div rounds
 *        towards minus infinity):   numX = (2x + 1)*lowWidth - width;   ix0 = floor_div(numX, 2*width);
 *        fx = (float)(numX - ix0*2*width) / (float)(2*width);   wx = {1.0f - fx, fx};   likewise numY, iy0, fy, wy with the heights.
 *        ix0 lies in -1 .. lowWidth-1: the tap ix0 may be -1 and the tap ix0 + 1 may be lowWidth; 0 <= fx < 1.
 *      A low texel is USABLE when all four channels are finite with |v| <= 2^48.  A tap q of p is DROPPED when it lies outside the
 *        low image (no clamping), when its texel is not usable, or when object_q != object_p (the records' `object`, misses being
 *        -1).  The index of a tap is formed only after the tap is known to lie inside the low image.  The normal weight of a tap is
 *          wn = 1 when object_p < 0 (sky takes sky), otherwise c = min1(max0((n^p.x*n^q.x + n^p.y*n^q.y) + n^p.z*n^q.z)) squared
 *          normalLog2Power times (c = c*c).
 *      STAGE 1.  The 2x2 taps q = (ix0 + i, iy0 + j), j outer and i inner, with w = (wx[i]*wy[j]) * wn over the kept ones:
 *          sw = sum(w);   when sw > 0 and sw >= minWeight:  out = sum(w*rgba_q) / sw per channel, alpha too.  p is INTERPOLATED.
 *      STAGE 2.  Otherwise p is a HOLE.  The 4x4 taps q = (ix0 + i, iy0 + j), i, j = -1 .. 2, j outer and i inner, the same drop rule,
 *          w = wn (1 for sky; a tap with wn == 0 contributes nothing):   sw = sum(w);   when sw > 0:  out = sum(w*rgba_q) / sw.
 *      STAGE 3.  Otherwise p is an ORPHAN hole: out = the low texel (min(x*lowWidth / width, lowWidth - 1), min(y*lowHeight / height,
 *          lowHeight - 1)) (integer division), copied as it stands, usable or not.
 *      With the bound every sum stays finite: a weight is at most 1, so 16 terms of w*v stay below 2^52, and a quotient by sw is a
 *      weighted mean up to rounding.  With lowWidth == width and lowHeight == height the position is exact (fx = fy = 0) and an
 *      interpolated pixel is its own low texel, w*v / w.  minWeight 0 makes a hole of a pixel only when no tap carries weight.
 *      HOLES.  dPixels receives the holes in exactly rt_accum_select's ORDER (tiles of 8 x 8 pixels in raster order, raster order
 *        inside a tile): exactly the first nListed = min(nHoles, capacity) entries are written, nothing behind them is touched and
 *        every store is checked against the capacity.  dSelState: nPixels = width*height; nSelected = the holes, whatever the
 *        capacity; nListed; capacity (saturated at 2^32 - 1); overflow = nSelected > capacity; nCapped = the orphans among the holes.
 *        A hole's value in dOut is a stand-in: the loop below replaces it with the pixel rt_render_to(pHigh) computes.  The result --
 *        dOut, the list, the state -- is bit-identical from run to run.
 *      rt_image_put_at: dImage[dPixels[k]] = dSamples[k] for k < n, 16 bytes each (dImage: rgba32f, width*height; dSamples: n
 *        rgba32f, rt_shade_rays' colour; dPixels: n rt_pixel, 8-byte aligned).  An entry with x >= width or y >= height is skipped and
 *        never forms an address.  n == 0 is a no-op; dSamples and dPixels may then be NULL.  With duplicates, which of the duplicate
 *        samples a pixel keeps is unspecified, but every access stays inside the image.  One launch.
 *      Refused before anything is enqueued, with RT_ERR_INVALID_ARG: NULL context, descriptor or required pointer; a pointer not
 *      16-byte aligned (dPixels: 8); dOut, dPixels, dScratch or dSelState overlapping dLow, dHitsLow or dHitsHigh or each other; for
 *      rt_image_put_at dSamples or dPixels overlapping dImage; width or height < 1; lowWidth outside 1..width, lowHeight outside
 *      1..height; normalLog2Power outside 0..7; minWeight not finite or outside [0, 1]; non-zero reserved words.  RT_ERR_TOO_LARGE:
 *      width*height > 2^31 - 1; n beyond one grid (2^31 - 1 workgroups of 256).  rt_upsample_layout refuses as rt_accum_select_layout
 *      does.  The context stays usable after a refusal.  The loop of a frame, with pLow and pHigh the rt_params of one view at the two
 *      sizes (DESIGN.md 31 has the measurements, stage by stage: at 2x per axis the loop costs more than rt_render_to(pHigh) alone on
 *      the shipped scenes -- a low render is not a quarter of a full one, and rt_shade_rays has a floor however few holes it shades):
 *          rt_render_to(ctx, &pLow, dLow, ...);
 *          rt_camera_rays(ctx, &pLow, dRays, s);   rt_trace_rays(ctx, dRays, nLow, RT_QUERY_CLOSEST, dHitsLow, s);
 *          rt_camera_rays(ctx, &pHigh, dRays, s);  rt_trace_rays(ctx, dRays, nHigh, RT_QUERY_CLOSEST, dHitsHigh, s);
 *          rt_upsample(ctx, dLow, dHitsLow, dHitsHigh, dOut, &u, dPixels, capacity, dScratch, dSel, s);
 *          an 8-byte read of dSel + offsetof(rt_select_state, nSelected): nSelected and nListed
 *          rt_camera_rays_at(ctx, &pHigh, dPixels, nListed, dRays, s);
 *          rt_shade_rays(ctx, &pHigh, dRays, dPixels, nListed, dSamples, NULL, NULL, s);
 *          rt_image_put_at(ctx, dSamples, dPixels, nListed, dOut, width, height, s);
 *      Afterwards every listed pixel of dOut holds rt_render_to(pHigh)'s bits and every other pixel is interpolated from low-resolution
 *      pixels of its own object. */
typedef struct rt_upsample_desc {
    int32_t width, height;           /* the output, >= 1 */
    int32_t lowWidth, lowHeight;     /* 1 <= lowWidth <= width, 1 <= lowHeight <= height; any ratio, per axis */
    int32_t normalLog2Power;         /* 0..7, as rt_denoise_desc */
    float minWeight;                 /* finite, 0..1: a pixel whose kept 2x2 weight is below it is a hole */
    int32_t reserved[10];            /* zero */
} rt_upsample_desc;                  /* 64 B */
int rt_upsample_layout(int width, int height, size_t *scratchBytes);
int rt_upsample(rt_context *ctx, const void *dLow, const void *dHitsLow, const void *dHitsHigh, void *dOut, const rt_upsample_desc *desc,
                void *dPixels, size_t capacity, void *dScratch, void *dSelState, void *hipStream);
int rt_image_put_at(rt_context *ctx, const void *dSamples, const void *dPixels, size_t n, void *dImage, int width, int height,
                    void *hipStream);

/* ---- multi-GPU strip helpers */
/* Number of local rows a rank owns for interleaved strips. */
int rt_strip_local_rows(int height, int stripRows, int stripCount, int stripIndex);
/* Rank-0 reassembly of gathered strip buffers.  src holds stripCount per-rank buffers,
 * rankStrideBytes apart, each made of whole strips of `width` pixels of bytesPerPixel (rows in
 * the rank's local order); dst = the full width x height image.  Device pointers;
 * asynchronous on hipStream (NULL = the context's stream). */
int rt_deinterleave(rt_context *ctx, const void *src, void *dst, int width, int height,
                    int bytesPerPixel, int stripRows, int stripCount, size_t rankStrideBytes,
                    void *hipStream);

/* Wire format for the gather (30 bytes per pixel instead of 40): every surface's alpha is the
 * constant 1.0 (raytracingCs.glsl:581-583), so a rank ships only
 *     [ gColor rgb f32 x nPixels | gPosition rgb f32 x nPixels | gNormal rgb f16 x nPixels ]
 * (rt_wire_bytes(nPixels) bytes, padded to 16) and rank 0 restores rgba with alpha = 1.0 while it
 * puts the strips back in image order.  No counterpart in the reference (single GPU).
 * rt_wire_pack: this rank's three surfaces (nPixels each, any row order) -> dWire.
 * rt_wire_unpack: dWire = stripCount rank buffers rankStrideBytes apart, each packed from
 * rankPixels pixels (whole strips of `width`); dst* = full width x height surfaces.  The image is
 * made of cycles of rootStrips strips of rank 0 followed by one strip of each other rank
 * (rootStrips = 1: the equal interleave).  With dRootColor/dRootPosition/dRootNormal != NULL rank
 * 0's rows are copied from its own local rgba surfaces (they never travel, wire slot 0 is ignored
 * and rank 0 may own a larger share: its rt_params use stripRows = rootStrips * stripRows,
 * stripCycleRows = (rootStrips + stripCount - 1) * stripRows, stripOffsetRows = 0); with NULL they
 * come from wire slot 0 and rootStrips must be 1.
 * Device pointers; asynchronous on hipStream (NULL = the context's stream). */
size_t rt_wire_bytes(size_t nPixels);
int rt_wire_pack(rt_context *ctx, const void *dColor, const void *dPosition, const void *dNormal, void *dWire,
                 size_t nPixels, void *hipStream);
int rt_wire_unpack(rt_context *ctx, const void *dWire, size_t rankStrideBytes, size_t rankPixels,
                   const void *dRootColor, const void *dRootPosition, const void *dRootNormal, int rootStrips,
                   void *dColor, void *dPosition, void *dNormal, int width, int height, int stripRows, int stripCount,
                   void *hipStream);

/* ---- one frame on N GPUs of a node from ONE process and ONE host thread -- what the reference's host is
 *      (/root/reference/src/main.cpp:3-7, ForwardShadingPipeline.cpp:129-271).  One context per entry of deviceIds (entries
 *      may repeat: N "devices" that are all device 0 run the N-way plan on a one-GPU box); device deviceIds[0] owns the frame.
 *      rt_mgpu_render splits the frame into interleaved strips of stripRows rows (default 8, rt_mgpu_set_strip_rows), every
 *      device renders its strips and its kernel stores them straight into the root's full-frame surfaces over xGMI (peer
 *      access; csrc/rt_mgpu.cpp) -- no gather buffer, no collective.  Asynchronous: the root context's stream (returned by
 *      rt_mgpu_get_surfaces) is ordered behind every device's stores, so work enqueued on it afterwards sees the whole frame;
 *      rt_mgpu_sync / rt_mgpu_readback wait for it.  p describes the WHOLE frame (identity window and strip fields).
 *      rt_mgpu_last_ms: duration of every device's share of the last frame (HIP events on its stream).
 *      A refused rt_mgpu_render changes nothing: parameters that are not a whole frame's, a maxRayDepth outside [0, 32] or a
 *      handle without a scene are turned down before the handle is touched, so the surfaces, the size rt_mgpu_readback copies
 *      and the frame rt_mgpu_last_ms times stay those of the last good frame (none, RT_ERR_NO_SURFACES, on a fresh handle).
 *      rt_mgpu_context: the context of device slot `slot` (0 <= slot < rt_mgpu_device_count), BORROWED -- the handle keeps
 *      ownership, rt_destroy on it is an error of the caller's.  For tests and instrumentation (the rt_debug_* read-outs of one
 *      device's share); RT_ERR_INVALID_ARG: NULL m or out, slot out of range. */
typedef struct rt_mgpu rt_mgpu;
int rt_mgpu_create(rt_mgpu **out, const int *deviceIds, int nDevices);
int rt_mgpu_destroy(rt_mgpu *m);
int rt_mgpu_device_count(rt_mgpu *m);
int rt_mgpu_set_scene(rt_mgpu *m, const void *objects, int nObj, const void *lights, int nLt);
int rt_mgpu_set_noise(rt_mgpu *m, const uint8_t *r8, int w, int h);
int rt_mgpu_set_skybox(rt_mgpu *m, const uint16_t *rgb16f, int size);
int rt_mgpu_set_strip_rows(rt_mgpu *m, int stripRows);
int rt_mgpu_render(rt_mgpu *m, const rt_params *p);
int rt_mgpu_sync(rt_mgpu *m);
int rt_mgpu_get_surfaces(rt_mgpu *m, void **dColor, void **dPosition, void **dNormal, void **rootStream);
int rt_mgpu_readback(rt_mgpu *m, float *gColor, float *gPosition, uint16_t *gNormal);
int rt_mgpu_last_ms(rt_mgpu *m, float *perDeviceMs, int cap);
const char *rt_mgpu_last_error(rt_mgpu *m);
int rt_mgpu_context(rt_mgpu *m, int slot, rt_context **out);

#ifdef __cplusplus
}
#endif

#if defined(__cplusplus) || (defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L)
#ifdef __cplusplus
#define RT_SA(c, m) static_assert(c, m)
#else
#define RT_SA(c, m) _Static_assert(c, m)
#endif
RT_SA(sizeof(rt_material) == 80, "Material is 80 B");
RT_SA(sizeof(rt_frame_desc) == 32 + 2 * sizeof(void *), "rt_frame_desc layout");
RT_SA(sizeof(rt_object) == RT_OBJECT_STRIDE, "Object stride is 176 B");
RT_SA(sizeof(rt_light) == RT_LIGHT_STRIDE, "Light stride is 96 B");
RT_SA(offsetof(rt_object, position) == 16 && offsetof(rt_object, radius) == 28, "Object.position/radius");
RT_SA(offsetof(rt_object, normal) == 32 && offsetof(rt_object, size) == 48, "Object.normal/size");
RT_SA(offsetof(rt_object, material) == 64, "Object.material");
RT_SA(offsetof(rt_object, boundsMin) == 144 && offsetof(rt_object, boundsMax) == 160, "Object.bounds");
RT_SA(offsetof(rt_material, albedo) == 16 && offsetof(rt_material, metallic) == 28, "Material.albedo/metallic");
RT_SA(offsetof(rt_material, roughness) == 32 && offsetof(rt_material, diffuseStrength) == 36, "Material.roughness/diffuseStrength");
RT_SA(offsetof(rt_material, ior) == 40 && offsetof(rt_material, transparency) == 44, "Material.ior/transparency");
RT_SA(offsetof(rt_material, specular) == 48 && offsetof(rt_material, subsurfaceScatter) == 52, "Material.specular/sss");
RT_SA(offsetof(rt_material, subsurfaceColor) == 64 && offsetof(rt_material, scatterDistance) == 76, "Material.sssColor/scatterDistance");
RT_SA(offsetof(rt_light, position) == 16 && offsetof(rt_light, direction) == 32, "Light.position/direction");
RT_SA(offsetof(rt_light, color) == 48 && offsetof(rt_light, intensity) == 60, "Light.color/intensity");
RT_SA(offsetof(rt_light, radius) == 64 && offsetof(rt_light, samples) == 68, "Light.radius/samples");
RT_SA(offsetof(rt_light, shadowSoftness) == 72 && offsetof(rt_light, shadowType) == 76, "Light.shadowSoftness/shadowType");
RT_SA(offsetof(rt_light, pcfSamples) == 80 && offsetof(rt_light, lightSize) == 84, "Light.pcfSamples/lightSize");
RT_SA(offsetof(rt_light, angularRadius) == 88, "Light.angularRadius");
RT_SA(sizeof(rt_params) == 128, "rt_params is 128 B");
RT_SA(sizeof(rt_ray) == 32 && offsetof(rt_ray, tMax) == 12 && offsetof(rt_ray, direction) == 16 && offsetof(rt_ray, reserved) == 28,
      "rt_ray layout");
RT_SA(sizeof(rt_hit) == 32 && offsetof(rt_hit, t) == 12 && offsetof(rt_hit, normal) == 16 && offsetof(rt_hit, object) == 28,
      "rt_hit layout");
RT_SA(sizeof(rt_pixel) == 8 && offsetof(rt_pixel, y) == 4, "rt_pixel layout");
RT_SA(sizeof(rt_accel_desc) == 32 && offsetof(rt_accel_desc, largeFraction) == 16 && offsetof(rt_accel_desc, reserved) == 20, "rt_accel_desc is 32 B");
RT_SA(sizeof(rt_accel_node) == 32 && offsetof(rt_accel_node, skip) == 12 && offsetof(rt_accel_node, hi) == 16 && offsetof(rt_accel_node, leaf) == 28,
      "rt_accel_node is 32 B");
RT_SA(sizeof(rt_accel_report) == 96 && offsetof(rt_accel_report, bytes) == 24 && offsetof(rt_accel_report, buildMs) == 32 &&
      offsetof(rt_accel_report, builds) == 40 && offsetof(rt_accel_report, launchesAccel) == 48 && offsetof(rt_accel_report, launchesBrute) == 64,
      "rt_accel_report is 96 B");
RT_SA(sizeof(rt_accel_build_report) == 64 && offsetof(rt_accel_build_report, buildsHost) == 8 && offsetof(rt_accel_build_report, buildsDevice) == 16 &&
      offsetof(rt_accel_build_report, hostMs) == 24 && offsetof(rt_accel_build_report, deviceMs) == 32 &&
      offsetof(rt_accel_build_report, reserved) == 40, "rt_accel_build_report is 64 B");
RT_SA(sizeof(rt_accel_shade_desc) == 32 && offsetof(rt_accel_shade_desc, traversal) == 4 && offsetof(rt_accel_shade_desc, minObjects) == 8 &&
      offsetof(rt_accel_shade_desc, reserved) == 12, "rt_accel_shade_desc is 32 B");
RT_SA(sizeof(rt_accel_shade_report) == 48 && offsetof(rt_accel_shade_report, traversal) == 4 && offsetof(rt_accel_shade_report, launchesAccel) == 8 &&
      offsetof(rt_accel_shade_report, launchesBrute) == 24 && offsetof(rt_accel_shade_report, reserved) == 32, "rt_accel_shade_report is 48 B");
RT_SA(sizeof(rt_accel_render_desc) == 32 && offsetof(rt_accel_render_desc, traversal) == 4 && offsetof(rt_accel_render_desc, minObjects) == 8 &&
      offsetof(rt_accel_render_desc, reserved) == 12, "rt_accel_render_desc is 32 B");
RT_SA(sizeof(rt_accel_render_report) == 64 && offsetof(rt_accel_render_report, traversal) == 4 && offsetof(rt_accel_render_report, minObjects) == 8 &&
      offsetof(rt_accel_render_report, launchesAccel) == 16 && offsetof(rt_accel_render_report, launchesPacket) == 40 &&
      offsetof(rt_accel_render_report, reserved) == 48, "rt_accel_render_report is 64 B");
RT_SA(RT_ACCEL_RENDER_DEFAULT_MIN_OBJECTS >= 257, "up to 256 objects the packet kernel has its shadow tables");
RT_SA(sizeof(rt_display_desc) == 32 && offsetof(rt_display_desc, flags) == 12 && offsetof(rt_display_desc, exposure) == 16,
      "rt_display_desc is 32 B");
RT_SA(sizeof(rt_meter_desc) == 48 && offsetof(rt_meter_desc, adapt) == 20 && offsetof(rt_meter_desc, reserved) == 32,
      "rt_meter_desc is 48 B");
RT_SA(sizeof(rt_meter_state) == 1088 && offsetof(rt_meter_state, nPixels) == 1024 && offsetof(rt_meter_state, minLum) == 1040 &&
      offsetof(rt_meter_state, nMetered) == 1048 && offsetof(rt_meter_state, exposure) == RT_METER_EXPOSURE_OFFSET &&
      offsetof(rt_meter_state, frames) == 1064, "rt_meter_state is 1088 B");
RT_SA(sizeof(rt_tone_desc) == 16 + 2 * sizeof(void *) && offsetof(rt_tone_desc, dExposure) == 8, "rt_tone_desc layout");
RT_SA(sizeof(rt_yuv_desc) == 48 && offsetof(rt_yuv_desc, transfer) == 20 && offsetof(rt_yuv_desc, flags) == 24 &&
      offsetof(rt_yuv_desc, exposure) == 28 && offsetof(rt_yuv_desc, reserved) == 32, "rt_yuv_desc is 48 B");
RT_SA(sizeof(rt_jpeg_desc) == 32 && offsetof(rt_jpeg_desc, restartInterval) == 12 && offsetof(rt_jpeg_desc, reserved) == 16, "rt_jpeg_desc is 32 B");
RT_SA(sizeof(rt_jpeg_state) == 64 && offsetof(rt_jpeg_state, overflow) == 8 && offsetof(rt_jpeg_state, stuffedBytes) == 24 &&
      offsetof(rt_jpeg_state, reserved) == 28, "rt_jpeg_state is 64 B");
RT_SA(sizeof(rt_resample_desc) == 32 && offsetof(rt_resample_desc, filter) == 16 && offsetof(rt_resample_desc, flags) == 20 &&
      offsetof(rt_resample_desc, reserved) == 24, "rt_resample_desc is 32 B");
RT_SA(sizeof(rt_accum_desc) == 40 && offsetof(rt_accum_desc, relError) == 8 && offsetof(rt_accum_desc, minSamples) == 16 &&
      offsetof(rt_accum_desc, reserved) == 24, "rt_accum_desc is 40 B");
RT_SA(sizeof(rt_accum_state) == 1024 && offsetof(rt_accum_state, nPixels) == 512 && offsetof(rt_accum_state, minCount) == 528 &&
      offsetof(rt_accum_state, medianBin) == 540 && offsetof(rt_accum_state, done) == 548 && offsetof(rt_accum_state, frames) == 552 &&
      offsetof(rt_accum_state, reserved) == 556, "rt_accum_state is 1 KiB");
RT_SA(sizeof(rt_denoise_guide_rec) == 16 && offsetof(rt_denoise_guide_rec, object) == 12, "rt_denoise_guide_rec is the upper half of rt_hit");
RT_SA(sizeof(rt_denoise_desc) == 48 && offsetof(rt_denoise_desc, iterations) == 8 && offsetof(rt_denoise_desc, sigmaLum) == 16 &&
      offsetof(rt_denoise_desc, minCount) == 24 && offsetof(rt_denoise_desc, reserved) == 28, "rt_denoise_desc is 48 B");
RT_SA(sizeof(rt_reproject_desc) == 288 && offsetof(rt_reproject_desc, prev) == 8 && offsetof(rt_reproject_desc, cur) == 136 &&
      offsetof(rt_reproject_desc, normalCosMin) == 264 && offsetof(rt_reproject_desc, maxHistory) == 272 &&
      offsetof(rt_reproject_desc, reserved) == 276, "rt_reproject_desc is 288 B");
RT_SA(sizeof(rt_reproject_report) == 64 && offsetof(rt_reproject_report, minCount) == 20 && offsetof(rt_reproject_report, sumCount) == 32 &&
      offsetof(rt_reproject_report, reserved) == 40, "rt_reproject_report is 64 B");
RT_SA(sizeof(rt_select_state) == 64 && offsetof(rt_select_state, nSelected) == 4 && offsetof(rt_select_state, overflow) == 16 &&
      offsetof(rt_select_state, reserved) == 24, "rt_select_state is 64 B");
#undef RT_SA
#endif

#endif /* RT_MI355_H */
