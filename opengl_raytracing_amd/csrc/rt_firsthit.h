// rt_firsthit.h -- when a packet-kernel frame may reuse the previous frame's first hit and direct lighting,
// held by value in rt_context (rt_context.h).  Depth 0 of a frame -- the camera ray, its shadow rays and subsurface probes -- is
// a function of the scene, the textures and every rt_params field except frameCount (which enters depth 0 only through the
// noise texture): while those stay what they were, the frame after a still one RECORDS what depth 0 ends with, and the frames
// after that REPLAY it (render_packet's FIRST parameter, rt_packet.inc).  This header decides which of the three a launch is; it
// holds no HIP type, so it is compiled and tested alone (tests/test_first_hit_host.py).  The record buffer, the events between
// the streams and the launches themselves are rt_abi.cpp's and rt_sched.cpp's; the buffer's layout, which section 27's settled
// tiles extend, is below.  Not part of the public ABI.
#pragma once
#include <stdint.h>
#include <string.h>

#include "rt_mi355.h"

// Everything depth 0 of a frame is a function of.  Output pointers, imageStores, the stream and the scheduler's bits are not
// in it: they decide where and in which tile order the frame is written, not what depth 0 computes.
struct RtFirstHitKey {
    uint32_t sceneGen, texGen;       // bumped by every change of the scene's bytes / of a texture
    int32_t nObj, nLt;
    int32_t variant;                 // rt_set_variant's low byte
    int32_t noise, sky;              // 1 = a noise texture / a skybox is loaded
    rt_params p;                     // every field; frameCount as 0 while no noise texture is loaded
};

inline RtFirstHitKey rt_first_hit_key(uint32_t sceneGen, uint32_t texGen, int nObj, int nLt, int variant, bool noise, bool sky, const rt_params &p) {
    RtFirstHitKey k;
    memset(&k, 0, sizeof k);         // (padding too: keys are compared as bytes)
    k.sceneGen = sceneGen;
    k.texGen = texGen;
    k.nObj = nObj;
    k.nLt = nLt;
    k.variant = variant & 0xff;
    k.noise = noise ? 1 : 0;
    k.sky = sky ? 1 : 0;
    // field by field, so that no padding of the caller's struct gets into the key
    for (int i = 0; i < 3; i++) { k.p.camPos[i] = p.camPos[i]; k.p.camDir[i] = p.camDir[i]; k.p.camUp[i] = p.camUp[i]; k.p.camRight[i] = p.camRight[i]; }
    k.p.fovDeg = p.fovDeg; k.p.focalLength = p.focalLength; k.p.maxRayDistance = p.maxRayDistance;
    k.p.noiseScale[0] = p.noiseScale[0]; k.p.noiseScale[1] = p.noiseScale[1];
    // frameCount reaches depth 0 through sample_noise alone (the bounce sample it also feeds is used from the next direction
    // on, the roulette starts at depth 3): without a noise texture frames that differ only in it share their first hit
    k.p.frameCount = noise ? p.frameCount : 0;
    k.p.useSkybox = p.useSkybox; k.p.maxRayDepth = p.maxRayDepth;
    k.p.width = p.width; k.p.height = p.height;
    k.p.x0 = p.x0; k.p.y0 = p.y0; k.p.regionW = p.regionW; k.p.regionH = p.regionH;
    k.p.stripRows = p.stripRows; k.p.stripCount = p.stripCount; k.p.stripIndex = p.stripIndex; k.p.reserved0 = p.reserved0;
    k.p.stripCycleRows = p.stripCycleRows; k.p.stripOffsetRows = p.stripOffsetRows;
    return k;
}

// The record buffer of a regionW x regionH window: four parts in one allocation, each starting on a multiple of 16 bytes.
//   hits     8 B/pixel   (t, hit object) of the first hit                                   } the first-hit records (section 26),
//   colours  12 B/pixel  finalColor after depth 0                                           } packed: 20 B/pixel
//   finals   32 B/pixel  what a settled tile stored to the three surfaces (section 27): two 16-byte halves,
//                        (colour.xyz, position.x) and (position.y, position.z, the packed normal pair)
//   flags    1 B/tile    1 = the 8x8 tile is settled, 1 + K = it resumes at depth K from prefix records (rt_prefix_flag, below),
//                        indexed by the window-local tile id tileY * tilesX + tileX
// Pixels are indexed window-locally, j * regionW + i.  Plain integer arithmetic: the kernel (render_packet), the ABI layer and
// a host-only test (tests/test_settled_layout_host.py) all take the offsets from here.
struct RtFirstHitLayout {
    uint64_t pixels, tiles;
    uint64_t hits, colours, finals, flags;      // byte offsets of the four parts
    uint64_t bytes;                             // of the whole buffer
};
#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_FH_INLINE __host__ __device__ inline
#else
#define RT_FH_INLINE inline
#endif
RT_FH_INLINE uint64_t rt_first_hit_align16(uint64_t v) { return (v + 15u) & ~(uint64_t)15u; }
RT_FH_INLINE uint64_t rt_first_hit_tiles(int regionW, int regionH) {
    return (uint64_t)((regionW + 7) / 8) * (uint64_t)((regionH + 7) / 8);
}
RT_FH_INLINE uint64_t rt_first_hit_colours_offset(int regionW, int regionH) {
    return rt_first_hit_align16((uint64_t)regionW * (uint64_t)regionH * 8u);
}
RT_FH_INLINE uint64_t rt_first_hit_finals_offset(int regionW, int regionH) {
    return rt_first_hit_align16(rt_first_hit_colours_offset(regionW, regionH) + (uint64_t)regionW * (uint64_t)regionH * 12u);
}
RT_FH_INLINE uint64_t rt_first_hit_flags_offset(int regionW, int regionH) {
    return rt_first_hit_finals_offset(regionW, regionH) + (uint64_t)regionW * (uint64_t)regionH * 32u;
}
RT_FH_INLINE uint64_t rt_first_hit_bytes(int regionW, int regionH) {
    return rt_first_hit_flags_offset(regionW, regionH) + rt_first_hit_align16(rt_first_hit_tiles(regionW, regionH));
}
inline RtFirstHitLayout rt_first_hit_layout(int regionW, int regionH) {
    RtFirstHitLayout l;
    l.pixels = (uint64_t)regionW * (uint64_t)regionH;
    l.tiles = rt_first_hit_tiles(regionW, regionH);
    l.hits = 0;
    l.colours = rt_first_hit_colours_offset(regionW, regionH);
    l.finals = rt_first_hit_finals_offset(regionW, regionH);
    l.flags = rt_first_hit_flags_offset(regionW, regionH);
    l.bytes = rt_first_hit_bytes(regionW, regionH);
    return l;
}

// PREFIX REPLAY.  frameCount reaches a path only where a lane takes the diffuse branch of the
// next-direction step (section 27's TAINT), so everything a tile does up to the first depth K at which one of its lanes is
// tainted is the same bits for every frameCount.  Section 26 resumes every tile behind the lighting of depth 0; a tile with
// K >= 1 resumes behind the lighting of depth K instead.  The tile's flag byte says which:
//   0       K = 0: depth 0 is replayed from the (hits, colours) records (section 26)
//   1       settled: the tile is copied out of its final records (section 27)
//   1 + K   K = 1 .. RT_PREFIX_CAP: the bounce loop starts at depth K from the pixel's PREFIX record
// Resuming at any depth <= K is exact, so K is capped: a tile that taints later (or, with settled tiles switched off, never)
// resumes at the last depth it recorded.
#define RT_PREFIX_CAP 7
RT_FH_INLINE unsigned rt_prefix_flag(bool settled, int k) { return settled ? 1u : (k >= 1 ? 1u + (unsigned)(k < RT_PREFIX_CAP ? k : RT_PREFIX_CAP) : 0u); }
RT_FH_INLINE bool rt_prefix_flag_settled(unsigned flag) { return flag == 1u; }
RT_FH_INLINE int rt_prefix_flag_depth(unsigned flag) { return flag >= 2u ? (int)flag - 1 : 0; }      // 0 for K = 0 and for settled tiles
// A prefix record is the parked path state as it stands behind the lighting of depth K and in front of the roulette: 13 dwords.
//   w[0]       the hit object of depth K for a lane that is alive there, -1 for a lane whose path has ended
//   w[1..3]    finalColor
//   w[4..6]    P of the last hit
//   w[7..12]   alive: throughput, then the incoming direction rd (N is recomputed from P and the hit object)
//              ended: N of the last hit, then zeros
// It lives in the 8 + 12 + 32 bytes the pixel already owns in the hits, colours and finals parts -- a K >= 1 tile needs neither
// its depth-0 record nor a final record: w[0..1] -> hits, w[2..4] -> colours, w[5..12] -> finals.
#define RT_PREFIX_DWORDS 13
struct RtPrefixRecord { uint32_t w[RT_PREFIX_DWORDS]; };
RT_FH_INLINE uint32_t rt_prefix_bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
RT_FH_INLINE float rt_prefix_float(uint32_t u) { float v; memcpy(&v, &u, 4); return v; }
RT_FH_INLINE RtPrefixRecord rt_prefix_pack(bool alive, int hit, const float fc[3], const float P[3], const float thrOrN[3], const float rd[3]) {
    RtPrefixRecord r;
    r.w[0] = alive ? (uint32_t)hit : 0xffffffffu;
    for (int k = 0; k < 3; k++) {
        r.w[1 + k] = rt_prefix_bits(fc[k]);
        r.w[4 + k] = rt_prefix_bits(P[k]);
        r.w[7 + k] = rt_prefix_bits(thrOrN[k]);
        r.w[10 + k] = alive ? rt_prefix_bits(rd[k]) : 0u;
    }
    return r;
}
// returns alive; fills thr and rd for a lane that is, N for one that is not (the other outputs are left as they were)
RT_FH_INLINE bool rt_prefix_unpack(const RtPrefixRecord &r, int nObj, int *hit, float fc[3], float P[3], float thr[3], float rd[3], float N[3]) {
    const int h = (int)r.w[0];
    const bool alive = h >= 0 && h < nObj;          // (a record never holds anything else; no gather may leave the scene)
    *hit = alive ? h : -1;
    for (int k = 0; k < 3; k++) {
        fc[k] = rt_prefix_float(r.w[1 + k]);
        P[k] = rt_prefix_float(r.w[4 + k]);
        if (alive) { thr[k] = rt_prefix_float(r.w[7 + k]); rd[k] = rt_prefix_float(r.w[10 + k]); }
        else N[k] = rt_prefix_float(r.w[7 + k]);
    }
    return alive;
}
// byte offset of dword d of pixel `at`'s prefix record in the buffer of a regionW x regionH window
RT_FH_INLINE uint64_t rt_prefix_dword_offset(int regionW, int regionH, uint64_t at, int d) {
    if (d < 2) return at * 8u + (uint64_t)d * 4u;
    if (d < 5) return rt_first_hit_colours_offset(regionW, regionH) + at * 12u + (uint64_t)(d - 2) * 4u;
    return rt_first_hit_finals_offset(regionW, regionH) + at * 32u + (uint64_t)(d - 5) * 4u;
}

struct RtFirstHit {
    enum Mode { NORMAL = 0, RECORD = 1, REPLAY = 2 };
    // Windows above this many pixels are never recorded (52 bytes per pixel and one per tile: 832 MiB at the cap, which a
    // 4096 x 4096 window reaches; 1080p takes 108 MB).  Larger ones render normal frames.  The cap stays where section 26 put
    // it: a buffer that cannot be had is refused at no cost (refuse()), so the cap only bounds what is ever asked for.
    static constexpr uint64_t kMaxPixels = (uint64_t)1 << 24;

    bool envOn = true;               // RT_FIRST_HIT_REUSE=0 at rt_create clears it
    bool variantOn = true;           // rt_set_variant's bit 10 (0x400) clears it
    bool haveLast = false;           // `last` is the key of the previous eligible launch, with nothing invalidating in between
    bool valid = false;              // the buffer holds the records of `cached`
    RtFirstHitKey last, cached;
    uint64_t refusedPixels = 0;      // a record buffer of this many pixels could not be had: windows that large are not tried again
    uint64_t counts[3] = {0, 0, 0};  // launches since creation: normal, recorded, replayed (rt_debug_first_hit)

    bool on() const { return envOn && variantOn; }

    // What the next eligible launch (packet kernel, no ray counter) with key k is.  A key other than the cached one drops the
    // cache: the view has moved on, and only the frame after a still one records again.
    //   key == the valid cache's key                            -> REPLAY
    //   else key == the previous launch's key (no valid cache)  -> RECORD
    //   else                                                    -> NORMAL
    Mode decide(const RtFirstHitKey &k) {
        if (!on() || k.p.maxRayDepth < 1 || k.p.regionW <= 0 || k.p.regionH <= 0) return NORMAL;
        if (valid && memcmp(&k, &cached, sizeof k) == 0) return REPLAY;
        valid = false;
        const uint64_t px = (uint64_t)k.p.regionW * (uint64_t)k.p.regionH;
        if (px > kMaxPixels || (refusedPixels && px >= refusedPixels)) return NORMAL;
        if (haveLast && memcmp(&k, &last, sizeof k) == 0) return RECORD;
        return NORMAL;
    }
    // the record buffer could not be allocated: the launch decided as RECORD runs as a normal frame, now and from now on
    void refuse(const RtFirstHitKey &k) { refusedPixels = (uint64_t)k.p.regionW * (uint64_t)k.p.regionH; }
    // the launch went out as mode m
    void launched(Mode m, const RtFirstHitKey &k) {
        counts[m]++;
        if (!on()) { invalidate(); return; }
        if (m == RECORD) { cached = k; valid = true; }
        last = k;
        haveLast = true;
    }
    // a setter changed an input, the launch failed or was refused, or reuse was switched off: the next launch is a normal frame
    void invalidate() { valid = false; haveLast = false; }
};
