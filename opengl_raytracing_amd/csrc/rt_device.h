// rt_device.h -- shared declarations between the tracer's HIP kernels (rt_kernels.hip) and the C-ABI
// implementation (rt_abi.cpp, rt_sched.cpp): per-launch constants, the device scene, buffer sizes, launch wrappers.  The post
// passes' are in rt_post.h, the strip transport's in rt_wire.h, the display path's in rt_display.h.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_mi355.h"
#include "rt_firsthit.h"

#define RT_MAX_DEPTH 32      // per-depth bounce-sample table in kernarg memory
#define RT_HALTON_N 64       // tabulated Halton indices (UI range of pcfSamples is 1..16)

// "Compiled" scene record sizes, in float4 units.  See DESIGN.md "Data layout".
#define RT_HOT_F4 6          // per object: AABB + shape, read for every ray
#define RT_MAT_F4 4          // per object: material, read once per closest hit
#define RT_LGT_F4 4          // per light

// Per-launch constants, passed by value in kernarg memory (scalar loads, no staging).
struct RtFrame {
    rt_params p;
    int32_t nObj, nLt;
    int32_t noiseW, noiseH, skySize;
    int32_t anyPcss;                    // some light has shadowType 2: kernel instantiation with paired blocker rays
    int32_t imageStores;                // 1: the surfaces are whole width x height images, a pixel goes to (image row, image column)
                                        // (rt_render_into_image: strips of several devices land in one frame); 0: regionW x regionH window
    float sx, sy;                       // (aspect*tanFov)*focalLength, tanFov*focalLength
    // cosineWeightedHemisphere's local direction for the bounce at each depth
    // (identical for every pixel: hammersley(depth*64+frameCount, 64))
    float hemi[RT_MAX_DEPTH][4];
    float sssHemi[4][4];                // same for computeSubsurfaceScattering's 4 samples
};

struct RtDeviceScene {
    const float4 *compiled;   // [nObj*RT_HOT_F4][nObj*RT_MAT_F4][nLt*RT_LGT_F4][halton2: 16][halton3: 16]
    const uint8_t *noise;     // R8 texels or nullptr
    const uint16_t *sky;      // 6*size*size*3 halfs or nullptr
    // Cost-feedback tile scheduling (packet kernel): workgroup b renders tile tileOrder[b] (or b when
    // null) and records its duration in tileCost[tile]; rt_launch_lpt_sort turns the costs of frame k
    // into the longest-first order of frame k+1.  Pure scheduling: no pixel value depends on it.
    const unsigned *tileOrder;
    unsigned *tileCost;
    // Shadow tables (rt_shadowtab.inc): per light RT_ST_HDR_F4 float4 of header, then the lights' cells (one bit per object);
    // built by rt_set_scene for scenes of <= RT_ST_MAX_OBJECTS objects, nullptr otherwise.
    const unsigned *shadowTab;
};

#define RT_ST_HDR_F4 7            // float4 per light header
#define RT_ST_MAX_OBJECTS 256     // 8 dwords per cell
#define RT_ST_MAX_LIGHTS 64       // (a table is 0.4-6 MB per light)
// dwords per cell for a scene of nObj objects (the packet kernel's profiles are compiled for exactly these: rt_packet.inc)
static inline int rt_shadowtab_words(int nObj) { return nObj <= 32 ? 1 : (nObj <= 64 ? 2 : 8); }
// Table geometry: cube-map cells per face edge (point / area lights), grid cells per axis (directional), bins; and the
// buffer size in dwords that holds any mix of light types.
struct RtShadowTabGeom { int Kcube, Kplan, NB; };
// direction cells of one light (the builder's phase-1 supersets, stored behind the tables)
static inline size_t rt_shadowtab_dir_cells(const RtShadowTabGeom &g) {
    const size_t cube = (size_t)6 * g.Kcube * g.Kcube, plan = (size_t)g.Kplan * g.Kplan;
    return cube > plan ? cube : plan;
}
// dwords of headers + cells (what the render kernel reads, and rt_debug_shadow_tables returns).  `blocker`: the scene has a PCSS
// light -- a second set of tables, for pcssShadow's blocker rays, follows the first (rt_shadowtab.inc)
static inline size_t rt_shadowtab_table_dwords(const RtShadowTabGeom &g, int nObj, int nLt, bool blocker) {
    const size_t cube = (size_t)g.NB * 6 * g.Kcube * g.Kcube, plan = (size_t)g.NB * g.Kplan * g.Kplan + 1;
    return (size_t)nLt * RT_ST_HDR_F4 * 4 + (size_t)(blocker ? 2 : 1) * nLt * (cube > plan ? cube : plan) * rt_shadowtab_words(nObj) + 4;
}
// ... + the builder's scratch
static inline size_t rt_shadowtab_dwords(const RtShadowTabGeom &g, int nObj, int nLt, bool blocker) {
    return rt_shadowtab_table_dwords(g, nObj, nLt, blocker) + (size_t)(blocker ? 2 : 1) * nLt * rt_shadowtab_dir_cells(g) * rt_shadowtab_words(nObj);
}
hipError_t rt_launch_shadow_tables(const float4 *dCompiled, int nObj, int nLt, unsigned *dTab, const RtShadowTabGeom &g, hipStream_t s, bool onePhase = false,
                                   bool blocker = false);

#define RT_PCF_TAB_N 16      // PCF samples tabulated per directional light (UI range of pcfSamples is 1..16)
// float4 count of the whole compiled buffer: the staged part (rt_compiled_f4) + per light RT_PCF_TAB_N x 2 float4
// of precomputed PCF rays (direction, dot(d,d)) (1/direction, -), meaningful for directional lights only
static inline size_t rt_compiled_f4(int nObj, int nLt);
static inline size_t rt_compiled_total_f4(int nObj, int nLt) { return rt_compiled_f4(nObj, nLt) + (size_t)nLt * RT_PCF_TAB_N * 2; }
static inline size_t rt_compiled_f4(int nObj, int nLt) {
    return (size_t)nObj * (RT_HOT_F4 + RT_MAT_F4) + (size_t)nLt * RT_LGT_F4 + 2 * (RT_HALTON_N / 4);
}

// Launch wrappers implemented in rt_kernels.hip
hipError_t rt_launch_compile_scene(const uint8_t *dObjects, int nObj, const uint8_t *dLights, int nLt,
                                   float4 *dCompiled, hipStream_t s);
hipError_t rt_launch_render(const RtFrame &f, const RtDeviceScene &sc, float4 *dColor, float4 *dPos,
                            uint2 *dNormal, unsigned long long *dRayCounter, int variant, hipStream_t s, int countMode = 1,
                            int firstMode = 0, void *dFirstHit = nullptr, int *blockerGroup = nullptr, const struct RtSplitDesc *dSplit = nullptr);
// (blockerGroup, optional: receives how many of pcssShadow's blocker rays the launched instantiation takes per traversal --
// RT_PK_BLOCKER_GROUP in the profiles with blockerPairs / blockerTab, 1 in the others and in the exhaustive kernel; the
// granularity at which a countMode-2 launch stops a lane's blocker search.)
// (the record buffer of a regionW x regionH window, render_packet FIRST != 0: rt_first_hit_bytes() and the offsets of its parts
// are rt_firsthit.h's.)  Bit 0 of the dFirstHit pointer a RECORDING launch passes switches settled tiles OFF (DESIGN.md
// section 27: every tile's flag is then written as 0, which is all a replaying launch looks at): the buffer is aligned far
// beyond that, and one more kernel argument would move the hidden arguments of every instantiation.
#define RT_FIRST_HIT_NO_SETTLED ((uintptr_t)1)
// Bit 1, likewise, switches prefix replay OFF: the recording launch writes no prefix record and every
// tile's flag says K = 0 or settled, which is the buffer as section 27 left it.
#define RT_FIRST_HIT_NO_PREFIX ((uintptr_t)2)
#define RT_FIRST_HIT_SWITCHES (RT_FIRST_HIT_NO_SETTLED | RT_FIRST_HIT_NO_PREFIX)

// ---- TILE SPLIT: a replaying frame's heaviest tiles run as P one-wave jobs that share the path geometry
// and divide the lighting units (depth, light) and (depth, subsurface section) among themselves; the job that ends last adds up.
#define RT_SPLIT_MAX_TILES 512                            // S: tiles split per frame at most
#define RT_SPLIT_MAX_PARTS 4                              // P <= 4
#define RT_SPLIT_EXTRA_BLOCKS (3 * RT_SPLIT_MAX_TILES)    // E: workgroups ahead of the tiles' own, one per extra job (the host never reads the count)
#define RT_SPLIT_UNITS_PER_PART 32                        // a tile of more than 32 P units stays whole
// Frames of more tiles than this per resident wave slot are launched whole: their longest tile is a small part of a slot's load
// (C3 and C4, 21-25 tiles per slot: no tile above the plan's target; C2, 6.3: some 300), and a launch with a plan runs the
// kernel that carries the split's code, which costs the whole tiles 3-10 %
#define RT_SPLIT_MAX_TILES_PER_SLOT 16
// g, the share of a heavy replaying tile's time that every part repeats (the start, closest hits, hit set-up, roulette, next
// direction), in 1/256.  Measured (profiles/tile_split_bench.json, "geometry_share"): the section timers on windows of the 300
// heaviest C2 tiles give 0.14-0.16 for whole frames, whose depth-0 lighting a replaying tile does not have; the ten heaviest
// replaying tiles cost 1.89 times as much in four parts as whole, which is g = (1.89 - 1) / 3 = 0.30 -- the figure used.
#define RT_SPLIT_G256 76
// A split tile's scratch slot, in dwords, for frames of `depth` bounces and nLt lights: 64 of header (dword 0 = the arrival
// counter), then SoA columns of 64 lanes -- 4 per unit (x, y, z, and for a subsurface unit the lane's needs-it bit), 4 per depth
// (throughput, then bit 0 alive / bit 1 a miss that adds the sky), 4 for that sky term.
RT_FH_INLINE unsigned rt_split_units(int depth, int nLt) { return (unsigned)depth * (unsigned)(nLt + 1); }
RT_FH_INLINE size_t rt_split_slot_dwords(int depth, int nLt) { return 64u + ((size_t)rt_split_units(depth, nLt) * 4u + (size_t)depth * 4u + 4u) * 64u; }
struct RtSplitDesc {
    const unsigned char *records;      // the first-hit record buffer
    const unsigned char *parts;        // [nTiles] P of a split tile, 0 of any other
    const unsigned short *slot;        // [nTiles] a split tile's scratch slot, < RT_SPLIT_MAX_TILES
    const unsigned *extra;             // [RT_SPLIT_EXTRA_BLOCKS] the jobs beyond part 0, heaviest tile first: tile | part << 28
    const unsigned *counts;            // [0] extra jobs, [1] split tiles
    float *scratch;                    // [RT_SPLIT_MAX_TILES] slots of rt_split_slot_dwords() each
};
// The plan of the order buffer `order` (rt_sched.cpp launches it behind the sort that wrote the order): walks it heaviest first.
// forceParts: RT_DEBUG_SPLIT_PARTS; prevParts (may be null): the plan in use, whose split tiles stay split.
hipError_t rt_launch_split_plan(const unsigned *dOrder, const unsigned *dCost, int nTiles, unsigned waveSlots, int depth, int nLt, int forceParts,
                                const unsigned char *dPrevParts, unsigned char *dParts, unsigned short *dSlot, unsigned *dExtra,
                                unsigned *dCounts, unsigned epoch, unsigned *hSeen, hipStream_t s);      // hSeen (pinned, may be null): (split tiles, epoch)
hipError_t rt_launch_split_desc(RtSplitDesc *dDesc, const RtSplitDesc &v, hipStream_t s);
// resident waves per SIMD of the packet-kernel instantiation rt_launch_render picks for this frame
int rt_packet_profile_waves(const RtFrame &f, const RtDeviceScene &sc);
// Tile geometry of the packet kernel for a given scene size / window (so the ABI layer can size the
// feedback buffers): workgroup threads, tile edge, tiles per row, total tiles.
void rt_packet_geometry(int nObj, int regionW, int regionH, int *bt, int *tile, int *tilesX, int *nTiles);
// Heavy-first tile order predicted from the frame's own inputs (rt_predict_tiles_kernel): no history involved.
hipError_t rt_launch_predict_order(const RtFrame &f, const RtDeviceScene &sc, int tilesX, int nTiles, unsigned *dSeg, int segStride,
                                   unsigned *dCursors, unsigned *dNextCursors, unsigned char *dCls, unsigned *dOrder, hipStream_t s);
hipError_t rt_launch_lpt_sort(unsigned *dCost, unsigned *dSnap, unsigned *dOrder, int nTiles, hipStream_t s, unsigned *dAccum = nullptr,
                              unsigned *dKeep = nullptr);      // dKeep (optional): the costs as read, for the split plan
hipError_t rt_launch_iota(unsigned *dOrder, int n, hipStream_t s);      // dOrder[i] = i (identity tile order)
// Ray queries (rt_query.inc).  dRays / dOut: 2 float4 per ray / hit (rt_ray / rt_hit), anyHit: one int per ray.
hipError_t rt_launch_trace_rays(const float4 *dRays, size_t nRays, const float4 *dCompiled, int nObj, int anyHit, void *dOut,
                                hipStream_t s);
hipError_t rt_launch_camera_rays(const RtFrame &f, const uint8_t *dNoise, float4 *dRays, hipStream_t s);
// rt_camera_rays_at: f built from an identity window; dPixels: one uint2 (rt_pixel) per ray
hipError_t rt_launch_camera_rays_at(const RtFrame &f, const uint8_t *dNoise, const uint2 *dPixels, size_t n, float4 *dRays, hipStream_t s);
hipError_t rt_launch_pick(const RtFrame &f, const uint8_t *dNoise, const float4 *dCompiled, int px, int py, float4 *dOut,
                          hipStream_t s);
// The same queries through the threaded hierarchy (rt_accel.inc; rt_accel.h has the structure): nodes = 2 float4 per node
// (lo, skip) (hi, leaf), order / loose = object indices.  lane: the per-ray traversal, else the per-wavefront one.  The host
// builder's structure has passed rt_accel_validate; the device builder's (rt_accel_build.h) is bounded by construction; the
// kernels' loops are bounded by nNodes whatever it holds.
struct RtAccelDev {
    const float4 *nodes = nullptr;
    const unsigned *order = nullptr, *loose = nullptr;
    int nNodes = 0, nLoose = 0;
};
hipError_t rt_launch_trace_rays_accel(const float4 *dRays, size_t nRays, const float4 *dCompiled, const RtAccelDev &acc, int anyHit, int lane,
                                      void *dOut, hipStream_t s);
hipError_t rt_launch_pick_accel(const RtFrame &f, const uint8_t *dNoise, const float4 *dCompiled, const RtAccelDev &acc, int px, int py,
                                float4 *dOut, hipStream_t s);
// rt_debug_device_math: one rt_device_math_op on n records of four words, one record per thread (rt_kernels.hip).
hipError_t rt_launch_device_math(int op, const uint4 *dIn, uint4 *dOut, size_t n, hipStream_t s);
// Ray shading (rt_shade.inc).  dRays: 2 float4 per ray (rt_ray); dPixels: one uint2 per ray, or null = rt_render_to(f.p)'s
// surface layout; dColor / dPos: one float4 per ray, dNormal: one packed half4 per ray (dPos / dNormal may be null).
hipError_t rt_launch_shade_rays(const RtFrame &f, const float4 *dCompiled, const uint8_t *dNoise, const uint16_t *dSky,
                                const float4 *dRays, const uint2 *dPixels, size_t nRays, float4 *dColor, float4 *dPos,
                                uint2 *dNormal, hipStream_t s);
// ... and through the hierarchy (rt_accel_shade.inc; rt_set_accel_shading): the same kernel body, closest-hit, shadow, blocker
// and subsurface rays by a walk of `acc`.  lane: the per-ray traversal, else the per-wavefront one.
hipError_t rt_launch_shade_rays_accel(const RtFrame &f, const float4 *dCompiled, const RtAccelDev &acc, int lane, const uint8_t *dNoise,
                                      const uint16_t *dSky, const float4 *dRays, const uint2 *dPixels, size_t nRays, float4 *dColor,
                                      float4 *dPos, uint2 *dNormal, hipStream_t s);
// A frame through the hierarchy (rt_accel_render.inc; rt_set_accel_render): rt_render_kernel's surfaces -- window, strips,
// imageStores, zero records outside the image -- by the per-lane path tracer over `acc`.  traversal: RT_ACCEL_RENDER_LANE, _WAVE
// or _SPLIT (the resolved one).
hipError_t rt_launch_render_accel(const RtFrame &f, const float4 *dCompiled, const RtAccelDev &acc, int traversal, const uint8_t *dNoise,
                                  const uint16_t *dSky, float4 *dColor, float4 *dPos, uint2 *dNormal, hipStream_t s);
