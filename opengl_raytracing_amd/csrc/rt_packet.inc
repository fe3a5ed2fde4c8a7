// rt_packet.inc -- the wavefront-packet variant of the render kernel (included by
// rt_kernels.hip inside its anonymous namespace; uses the helpers defined there).
//
// Same arithmetic per lane as rt_render_kernel -- the exact AABB / sphere / plane tests are
// evaluated by the very same functions -- but organised around the 64-lane wavefront:
//
//   1. CONTROL FLOW IS WAVE-UNIFORM.  Bounce loop, light loop, PCF/PCSS sample loops and the
//      SSS block are entered by the whole wave; lanes carry predicates (`alive`, `need`)
//      instead of sitting in divergent branches.  That keeps EXEC full where the cross-lane
//      operations below run, and keeps shadow rays of neighbouring pixels in lock-step.
//   2. PACKET CULLING.  Before a ray packet walks the scene, the wave reduces the packet's
//      origin box and reciprocal-direction box (DPP butterflies, no LDS traffic), then tests
//      64 objects AT ONCE -- lane l tests object l's AABB against the packet with interval
//      arithmetic -- and `__ballot`s the survivors into a 64-bit candidate mask.  The per-lane
//      exact tests then visit only the set bits (scalar s_ff1 loop).  The interval test is
//      rigorous in fp32 (rounding is monotone, so the rounded corner products bound every
//      lane's rounded slab distances); an object is skipped only if NO lane's exact
//      intersectAABB could pass, so results are bit-identical to the exhaustive loop.
//      Packets with NaNs, non-finite bounds or mixed-sign / zero direction components on an
//      axis simply lose that axis' constraint (or all culling).
//   3. NO OBJECT DATA LIVES IN REGISTERS ACROSS THE KERNEL.  Every cull pass reads the lane's object's AABB again (pk_bounds: from
//      LDS in the LIGHT profile, from the global copy -- L1 / L2 hits -- in the others), 64 objects per pass.  Round 1 kept the
//      first chunk's AABB in 8 VGPRs per lane; the registers were worth more as occupancy (DESIGN.md section 4).
//
// Kernel PROFILES (template constants, chosen per scene size by the launcher; measured in DESIGN.md section 4).  The kernel is
// latency-bound, so what a profile really trades is VGPRs (= resident waves) against re-reads and LDS per wave.  Every profile
// keeps the path state a bounce only touches at its ends and the shading point (P, N, V, material) in a per-lane LDS parking
// area (PK_PARK_FLOATS floats / lane) while a light's shadow rays are traced:
//   LIGHT (<= RT_PK_LIGHT_SCENE objects): AABBs staged in LDS (<= 1 KB), PCF rays four at a time -- no scratch at all;
//   HEAVY (more objects): PCF rays in pairs (each candidate record fetched once per pair: with 15-50 candidates per packet
//         that beats one at a time by 8-14 %), the cull passes read the AABBs from the GLOBAL copy (L1 / L2 hits) -- a per-wave
//         LDS copy of 256 objects' AABBs (8 KB) capped occupancy at 2.5 waves/SIMD.  A light's candidates come from its shadow
//         table (rt_shadowtab.inc); scenes beyond the tables (HUGE) use the packet-level masks and the per-lane shape level.
//
// ---- tunables: one macro each, re-tryable with -D (which side wins has flipped with the compiler's behaviour before: DESIGN.md
// section 4 item 36).  Alternatives that were structurally dead or superseded are gone (DESIGN.md section 18).
#ifndef RT_PK_LIGHT_SCENE
#define RT_PK_LIGHT_SCENE 32    // objects: at or below, the LIGHT profile (rt_launch_render)
#endif
#ifndef RT_PK_STRAIGHT
#define RT_PK_STRAIGHT 12   // (profile constant `straight` of the LIGHT profile; bits: 1 closest-hit, 2 any-hit, 4 PCF pair loop, 8 PCF
#endif                      // single loop) candidate tests in mask-algebra form -- lane predicates combined with & / |, wave-uniform
                            // skips only -- instead of nested per-lane ifs: 35 % fewer exec-mask save / restore pairs and execz
                            // branches, bit-identical.  Round 2 measured it 7 % SLOWER everywhere (the nested form skips more
                            // work when only a quarter of the candidate trips had a passing lane).  With the shadow tables 94 % of
                            // C2's trips have one (49 lanes on average), there is nothing left to skip, and the straight form wins
                            // in the few-object profile's PCF loops: C2 0.3465 -> 0.3218 ms with bits 4 / 12, 0.3236 with all four
                            // (the closest-hit and any-hit traversals gain nothing).  PCSS (C3 +0.7 % with 15) and the many-object
                            // profiles (all four: C4 +1.1 %, C5 +1.9 %; closest-hit only: +-0) keep the nested form.
#ifndef RT_LIGHT_FAST_PBR
#define RT_LIGHT_FAST_PBR 1     // computePBR's nine divisions through rt_fastmath.h's shared-reciprocal quotients (compute_pbr, rt_kernels.hip).
#endif                          // With the SLP vectorizer on it was a loss in LIGHT (C2 0.347 -> 0.367 ms, C3 3.39 -> 3.44) and a gain in HEAVY
                                // (C4 4.78 -> 4.66, C5 25.3 -> 24.9); built with -fno-slp-vectorize it pays everywhere: C2 0.311 -> 0.299, C3 2.775 -> 2.747
#ifndef RT_HEAVY_FAST_PBR
#define RT_HEAVY_FAST_PBR 1
#endif
#ifndef RT_LIGHT_GROUPN
#define RT_LIGHT_GROUPN 4       // PCF samples per traversal in the LIGHT profile: GROUPN rays are set up together and every candidate record is
                                // fetched once for the group (more ILP, fewer scalar loads, +~25 VGPRs per extra ray).  C2: 0.402 ms one at a
                                // time, 0.383 in pairs (92 B/lane of cold scratch; 0.4065 at 4 waves/SIMD without any), 0.449 in fours; round 2's
                                // first attempt at pairs was 8 % SLOWER -- where the allocator puts the spills decides, and that moved with the
                                // surrounding code.  Built without the SLP vectorizer fours fit 96 VGPRs without scratch: C2 0.298 -> 0.294 ms
                                // on top of the probes in fours
#endif
#ifndef RT_HEAVY_GROUPN
#define RT_HEAVY_GROUPN 2       // ... in the HEAVY profiles: pairs (4 costs too many registers there)
#endif
#ifndef RT_LIGHT_SSS_GROUP
#define RT_LIGHT_SSS_GROUP 4    // subsurface probe rays per traversal (pk_trace_closest_group): 1, 2 or 4.  Round 2 (registers full): C2 0.385 / 0.403 / 0.453 ms;
                                // with the path state resident in LDS (round 3) pairs won: C2 0.352 -> 0.347 ms; built without the SLP vectorizer
                                // (96 VGPRs, no scratch either way) all four at once: C2 0.301 -> 0.298, C3 2.76 -> 2.66 ms
#endif
#ifndef RT_HEAVY_SSS_GROUP
#define RT_HEAVY_SSS_GROUP 2    // (round 3, path state resident in LDS: C5 26.1 -> 25.4 ms, C4 unchanged)
#endif
#ifndef RT_PK_BLOCKER_GROUP
#define RT_PK_BLOCKER_GROUP 4   // pcssShadow's blocker rays per traversal (2, 4, 8 or 16).  C3: 4.83 ms single, 4.00 in pairs, 3.50 in fours, 3.89 in eights (spills)
#endif
#ifndef RT_PK_WAVES_SMALL
#define RT_PK_WAVES_SMALL 5     // resident waves per SIMD the LIGHT kernels are compiled for (96 VGPRs)
#endif
#ifndef RT_PK_WAVES_PCSS
#define RT_PK_WAVES_PCSS RT_PK_WAVES_SMALL      // ... every profile for scenes with a PCSS light
#endif
#ifndef RT_HEAVY_WAVES
#define RT_HEAVY_WAVES 6        // the multi-chunk HEAVY profile is compiled for 6 waves/SIMD (80 VGPRs): after the shape level the loops are short and
#endif                          // latency-bound again, a sixth wave buys C5 36.0 -> 34.5 ms (for 56 B/lane more cold scratch); LIGHT stays at 5
#ifndef RT_HEAVY1_WAVES
#define RT_HEAVY1_WAVES 6       // with the shadow tables the 64-object profile gains from the sixth wave too (C4 5.07 -> 4.88 ms; before them
#endif                          // 6 waves meant C4 6.27 -> 6.09 ms for three times the scratch traffic)
#ifndef RT_PK_CACHE_CHUNKS
#define RT_PK_CACHE_CHUNKS 4    // 64-object chunks whose light candidate masks the multi-chunk HEAVY profile keeps in SGPR pairs (pk_pcf_shadow)
#endif
#ifndef RT_PK_REACH_MIN_SAMPLES
#define RT_PK_REACH_MIN_SAMPLES 3       // `reach` profiles: the per-lane shape level of a light's PCF rays runs from this many samples on (pk_pcf_shadow)
#endif
#ifndef RT_PK_CONE_MIN_SAMPLES
#define RT_PK_CONE_MIN_SAMPLES 8        // the other profiles (LIGHT): interval slab test of the candidates' AABBs per lane, from this many samples on.
#endif                                  // (Stays: the LIGHT kernel compiles and reaches it, so removing it would change a shipped profile's code.)
#ifndef RT_PK_TIMERS
#define RT_PK_TIMERS 0          // 1: section timers in the instrumented (COUNT) build (pk_clock; off by default: they serialise the scalar unit)
#endif

#ifndef RT_FIRST_HIT_NT
#define RT_FIRST_HIT_NT 1       // a recording frame (render_packet, FIRST = 1) writes its first-hit records with non-temporal stores: they are read a
                                // frame later by another kernel.  Measured no different from plain stores (C2 recording frame 0.337 / 0.339 ms
                                // against 0.336 / 0.338, two runs each, tools/bench_first_hit.py)
#endif

constexpr int PK_PARK_FLOATS = 23;      // floats per lane of the LDS parking area: finalColor, throughput, ray.d, P, N, V, albedo (3 each), metallic, roughness

// ---- profiles ---------------------------------------------------------------------------------------------------------
struct PkLight {
    // light packets whose directions straddle zero on an axis culled per direction octant (pk_pcf_shadow).  Bought 3 % on C4 / C5
    // before the per-lane shape level existed; with it, off is 2-3 % faster and spills less.  Off in every profile.
    static constexpr bool split = false;
    // the cull passes read the lanes' AABBs from a per-workgroup LDS copy (false: from the global copy, L1 / L2)
    static constexpr bool boundsLds = true;
    // pcssShadow's 16 blocker rays go RT_PK_BLOCKER_GROUP per traversal (pk_trace_any_group).  Separate ...S instantiations
    // because the group code costs the PCF-only kernels registers they need (measured with the pair code merely present:
    // C2 +8 %, C4 +7 %, C5 +4 %), while it takes 12 % off C3.
    static constexpr bool blockerPairs = false;
    // ... and take their candidates from the lights' blocker tables (rt_shadowtab.inc) where a light has one
    static constexpr bool blockerTab = false;
    // fetch the light's colour / intensity again after its shadow rays instead of carrying 8 SGPRs across them.  Scalar
    // pressure decides these kernels -- 55-110 SGPRs are spilled to VGPR lanes, and a loop that has to v_readlane its
    // operands back every trip is what a slow build looks like (tools/isa_loops.py) -- but which build the allocator
    // produces is not monotone in the pressure, so it is set per instantiation by measurement: C4 (PkHeavy1) 8.20 -> 7.76 ms,
    // C3 (PkLightS) 3.52 -> 3.49, C2 (PkLight) unchanged, C5 (PkHeavy) 39.1 -> 43.9 (off there).
    static constexpr bool reloadLight = false;
    // the hit object's records requested as one batch of gathers (render_packet)
    static constexpr bool hitBatch = true;
    // per-lane second cull level of a light's PCF rays (pk_pcf_shadow): true = spheres on their shape from
    // RT_PK_REACH_MIN_SAMPLES samples on; false = every candidate on its AABB from RT_PK_CONE_MIN_SAMPLES samples on.
    // LIGHT: C2 0.385 ms without the shape level, 0.447 with (3 candidates per packet: nothing to prune).
    static constexpr bool reach = false;
    static constexpr bool fastPbr = RT_LIGHT_FAST_PBR;
    static constexpr int sssGroup = RT_LIGHT_SSS_GROUP;
    static constexpr int groupN = RT_LIGHT_GROUPN;
    static constexpr int cacheChunks = 1;
    static constexpr int waves = RT_PK_WAVES_SMALL;
    // dwords per shadow-table cell = 32-object groups the profile's scenes can have; 0 = no tables (the light's candidate
    // masks then come from per-packet interval tests)
    static constexpr int tabWords = 1;
    static constexpr int straight = RT_PK_STRAIGHT;
};
struct PkHeavy {
    static constexpr bool split = false;
    static constexpr bool boundsLds = false;
    static constexpr bool blockerPairs = false;
    static constexpr bool blockerTab = false;
    static constexpr bool reloadLight = false;
    // the hit records one after the other again.  With the per-lane shape level in place the batch form (and the octant
    // split) lost their edge: C4 6.40 -> 6.26 ms, C5 36.9 -> 35.8 ms and 32-36 B/lane less scratch without both
    static constexpr bool hitBatch = false;
    static constexpr bool reach = true;
    static constexpr bool fastPbr = RT_HEAVY_FAST_PBR;
    static constexpr int sssGroup = RT_HEAVY_SSS_GROUP;
    static constexpr int groupN = RT_HEAVY_GROUPN;
    static constexpr int cacheChunks = RT_PK_CACHE_CHUNKS;
    static constexpr int waves = RT_HEAVY_WAVES;
    static constexpr int tabWords = 8;
    static constexpr int straight = 0;
};
// HEAVY for scenes of one 64-object chunk: the light's candidate mask is one SGPR pair, no chunk cache (its four pairs cost
// the 64-object C4 4 % through SGPR spills while buying the 256-object C5 4 %)
struct PkHeavy1 : PkHeavy {
    static constexpr int cacheChunks = 1;
    static constexpr int waves = RT_HEAVY1_WAVES;
    static constexpr int tabWords = 2;
    static constexpr bool reloadLight = true;
};
// The same three for scenes with a PCSS light (RtFrame::anyPcss); blocker tables: 1 / 2 / 8 dwords per cell
struct PkLightS : PkLight {
    static constexpr bool blockerPairs = true;
    static constexpr bool blockerTab = true;
    static constexpr bool reloadLight = true;
    static constexpr int straight = 0;
    static constexpr int waves = RT_PK_WAVES_PCSS;
    static constexpr int groupN = 1;            // (PCF pairs here: C3 3.50 -> 3.56 ms)
};
struct PkHeavyS : PkHeavy {
    static constexpr bool blockerPairs = true;
    static constexpr bool blockerTab = true;
    static constexpr int waves = RT_PK_WAVES_PCSS;
};
struct PkHeavy1S : PkHeavy1 {
    static constexpr bool blockerPairs = true;
    static constexpr bool blockerTab = true;
    static constexpr int waves = RT_PK_WAVES_PCSS;
};
// scenes beyond the tables' 256 objects or 64 lights, and small scenes without tables: the packet-level masks of rounds 1-2
// (chunks recomputed per sample group past the cache) and the per-lane shape level
struct PkHuge : PkHeavy {
    static constexpr int tabWords = 0;
};
struct PkHugeS : PkHeavyS {
    static constexpr int tabWords = 0;
    static constexpr bool blockerTab = false;
};

constexpr float PK_INF = __builtin_huge_valf();

// Wave-uniform reads of the compiled scene.  The record index is the same for all 64 lanes
// (a candidate bit, the light index, a sample index), so the natural home of the data is the
// SCALAR register file: the records are fetched with s_load_dwordx4 from the
// global copy of the compiled scene (constant address space; 16 KiB scalar cache, then L2) and
// feed the VALU as SGPR operands -- no LDS instruction, no VGPRs.  Per-lane-indexed data
// (materials by hit index, the cull pass' per-lane AABBs) stays in LDS.
typedef float pk_f4 __attribute__((ext_vector_type(4)));
typedef unsigned pk_u2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(4))) pk_f4 *pk_uni4_t;
typedef const __attribute__((address_space(4))) float *pk_uni1_t;
__device__ __forceinline__ float4 uni_load4(const SceneLds &sc, int f4Index) {
    pk_f4 v = ((pk_uni4_t)(unsigned long long)sc.global)[f4Index];
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float uni_load1(const SceneLds &sc, int floatIndex) {
    return ((pk_uni1_t)(unsigned long long)sc.global)[floatIndex];
}
// Per-lane-indexed records.  Bounds (cull passes) come from the LDS copy (two float4 per object) or the global one, by profile;
// the shape / material fields a lane reads by its hit index once per bounce come from the global copy (sc.compact is true in every
// kernel that calls these; folding it away changes the shipped kernels' instruction sequences, so the select stays).
__device__ __forceinline__ float4 pk_bounds(const SceneLds &sc, int obj, int k) {
    return sc.boundsLds ? sc.hot[obj * sc.hotStride + k] : sc.global[obj * RT_HOT_F4 + k];
}
__device__ __forceinline__ float4 pk_lane_hot(const SceneLds &sc, int obj, int k) {
    return sc.compact ? sc.global[obj * RT_HOT_F4 + k] : sc.hot[obj * RT_HOT_F4 + k];
}
__device__ __forceinline__ float4 pk_lane_mat(const SceneLds &sc, int obj, int k) {
    return sc.compact ? sc.global[sc.matF4Base + obj * RT_MAT_F4 + k] : sc.mat[obj * RT_MAT_F4 + k];
}
// Halton table entry (wave-uniform index), falling back to evaluation beyond the table
__device__ __forceinline__ float pk_halton(const SceneLds &sc, int which, int i, int base) {
    return (i < RT_HALTON_N) ? uni_load1(sc, sc.haltonFloatBase + which * RT_HALTON_N + i) : halton_eval(i, base);
}

// ---- shadow tables (rt_shadowtab.inc): a lane's candidate mask for one light ---------------------------------------------
// header float4 of light li (wave-uniform -> scalar loads)
__device__ __forceinline__ float4 st_hdr4(const SceneLds &sc, int li, int k) {
    pk_f4 v = ((pk_uni4_t)(unsigned long long)sc.stab)[li * RT_ST_HDR_F4 + k];
    return make_float4(v.x, v.y, v.z, v.w);
}

// OR over the 64 lanes of NW dwords each (every lane must be active): fused v_or_b32_dpp butterflies, the NW chains
// interleaved (a DPP source written by the previous VALU instruction needs two wait states: s_nop where the chains are
// too few to cover them).  The results are wave-uniform (read from lane 63).
#define ST_OR_STEP1(ctrl) "v_or_b32_dpp %0, %0, %0 " ctrl "\n\ts_nop 1\n\t"
#define ST_OR_STEP2(ctrl) "v_or_b32_dpp %0, %0, %0 " ctrl "\n\tv_or_b32_dpp %1, %1, %1 " ctrl "\n\ts_nop 0\n\t"
#define ST_OR_STEP4(ctrl) "v_or_b32_dpp %0, %0, %0 " ctrl "\n\tv_or_b32_dpp %1, %1, %1 " ctrl "\n\tv_or_b32_dpp %2, %2, %2 " ctrl "\n\tv_or_b32_dpp %3, %3, %3 " ctrl "\n\t"
#define ST_OR_ALL(STEP)                                         \
    "s_nop 1\n\t"                                               \
    STEP("quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf")      \
    STEP("quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf")      \
    STEP("row_half_mirror row_mask:0xf bank_mask:0xf")          \
    STEP("row_mirror row_mask:0xf bank_mask:0xf")               \
    STEP("row_bcast:15 row_mask:0xa bank_mask:0xf")             \
    STEP("row_bcast:31 row_mask:0xc bank_mask:0xf")             \
    "s_nop 0"
template <int NW>
__device__ __forceinline__ void wave_or(unsigned (&m)[NW]) {
    if constexpr (NW == 1) {
        asm volatile(ST_OR_ALL(ST_OR_STEP1) : "+v"(m[0]));
    } else if constexpr (NW == 2) {
        asm volatile(ST_OR_ALL(ST_OR_STEP2) : "+v"(m[0]), "+v"(m[1]));
    } else {
        static_assert(NW % 4 == 0, "1, 2, 4 or 8 dwords per cell");
#pragma unroll
        for (int k = 0; k < NW; k += 4) asm volatile(ST_OR_ALL(ST_OR_STEP4) : "+v"(m[k]), "+v"(m[k + 1]), "+v"(m[k + 2]), "+v"(m[k + 3]));
    }
#pragma unroll
    for (int k = 0; k < NW; k++) m[k] = (unsigned)__builtin_amdgcn_readlane((int)m[k], 63);
}
#undef ST_OR_ALL
#undef ST_OR_STEP1
#undef ST_OR_STEP2
#undef ST_OR_STEP4

// The objects this lane's PCF rays toward light li can possibly hit, from the light's table (rt_shadowtab.inc): NW dwords,
// bit i = object i.  Lanes outside `need` contribute nothing; lanes the table does not cover (|N| too large, distance beyond
// the table or NaN) and lights without a table take every object.  O = the rays' origin, Lpos / D / lightDir = the light's
// position, this lane's light distance and (directional lights) the common direction, nn = dot(N, N) of the shading normal.
// BLOCKER: the light's second table, for pcssShadow's blocker rays (same cells; lights without one: every object).
template <int NW, bool BLOCKER = false>
__device__ __forceinline__ void st_lane_mask(const SceneLds &sc, int li, int nObj, v3 O, v3 Lpos, v3 lightDir, float D, float nn,
                                             bool need, unsigned (&m)[NW]) {
    const float4 h0 = st_hdr4(sc, li, 0), h1 = st_hdr4(sc, li, 1);
    int kind = __builtin_amdgcn_readfirstlane(__float_as_int(h0.x)), base = __builtin_amdgcn_readfirstlane(__float_as_int(h0.y));
    const int K = __builtin_amdgcn_readfirstlane(__float_as_int(h0.z)), NB = __builtin_amdgcn_readfirstlane(__float_as_int(h0.w));
    if constexpr (BLOCKER) {
        base = __builtin_amdgcn_readfirstlane(__float_as_int(st_hdr4(sc, li, 6).x));
        if (base == 0) kind = 0;
    }
    bool all = need;          // lanes that take every object
    int idx = 0;
    if (kind == 1) {          // cube map around a point / area light x distance bins
        const v3 u = O - Lpos;
        const float ax = fabsf(u.x), ay = fabsf(u.y), az = fabsf(u.z);
        const bool mx = (ax >= ay) & (ax >= az), my = !mx & (ay >= az);
        const float ma = mx ? ax : (my ? ay : az);
        const float um = mx ? u.x : (my ? u.y : u.z);
        const float us = mx ? u.y : u.x;                  // X-major: (y, z); Y-major: (x, z); Z-major: (x, y)
        const float ut = (mx | my) ? u.z : u.y;
        const int face = (mx ? 0 : (my ? 2 : 4)) + (um < 0.0f ? 1 : 0);
        const float inv = __builtin_amdgcn_rcpf(ma);
        const float half = 0.5f * (float)K;
        int ia = (int)floorf(__builtin_fmaf(us * inv, half, half)), ib = (int)floorf(__builtin_fmaf(ut * inv, half, half));
        ia = min(max(ia, 0), K - 1); ib = min(max(ib, 0), K - 1);
        const bool ok = (D < h1.y) & (nn <= h1.w);        // (NaN: false)
        int bin = (int)(D * h1.x);
        bin = min(max(bin, 0), NB - 1);
        idx = ((bin * 6 + face) * K + ib) * K + ia;
        all = need & !ok;
    } else if (kind == 2) {   // grid orthogonal to a directional light x depth bins
        const float4 h2 = st_hdr4(sc, li, 2), h3 = st_hdr4(sc, li, 3), h4 = st_hdr4(sc, li, 4);
        const float p = (O.z * h3.z + O.y * h3.y) + O.x * h3.x, q = (O.z * h4.z + O.y * h4.y) + O.x * h4.x;
        const float w = (O.z * lightDir.z + O.y * lightDir.y) + O.x * lightDir.x;
        const float fp = (p - h2.x) * h2.z, fq = (q - h2.y) * h2.z, fb = (w - h1.z) * h1.x, fK = (float)K;
        const bool inside = (fp >= 0.0f) & (fp < fK) & (fq >= 0.0f) & (fq < fK);
        const int ip = min(max((int)fp, 0), K - 1), iq = min(max((int)fq, 0), K - 1);
        const int bin = min(max((int)fminf(fb, 65536.0f), 0), NB - 1);
        idx = inside ? (bin * K + iq) * K + ip : NB * K * K;          // outside the grid: the light's extra cell
        // below the table's depth range, or any NaN / infinity in the three projections: every object
        const bool ok = (fb >= 0.0f) && (fabsf(fp) < PK_INF) && (fabsf(fq) < PK_INF) && (fabsf(fb) < PK_INF);
        all = need & !ok;
    }
#pragma unroll
    for (int k = 0; k < NW; k++) m[k] = 0u;
    if (need && !all) {
        const unsigned *cell = sc.stab + (size_t)base + (size_t)idx * NW;
        // (non-temporal gathers measured equal to 0.5 % slower on C2-C5: plain loads)
        if constexpr (NW == 1) m[0] = cell[0];
        else if constexpr (NW == 2) { const uint2 t = *(const uint2 *)cell; m[0] = t.x; m[1] = t.y; }
        else {
#pragma unroll
            for (int k = 0; k < NW; k += 4) { const uint4 t = *(const uint4 *)(cell + k); m[k] = t.x; m[k + 1] = t.y; m[k + 2] = t.z; m[k + 3] = t.w; }
        }
    }
#pragma unroll
    for (int k = 0; k < NW; k++) {
        const int nb = nObj - 32 * k;
        const unsigned valid = nb >= 32 ? 0xffffffffu : (nb > 0 ? ((1u << nb) - 1u) : 0u);
        m[k] = all ? valid : (m[k] & valid);
    }
}

// intersectSphere / intersectPlane (see shape_test) with the record fetched through uni_load4
__device__ __forceinline__ bool pk_shape_test(const SceneLds &sc, const Ray &r, float a, int obj, float radius2, int type,
                                              float &t) {
    if (type == 0) {
        float4 h2 = uni_load4(sc, obj * RT_HOT_F4 + 2);
        v3 oc = r.o - V3(h2);
        float b = 2.0f * dot(oc, r.d);
        float c = dot(oc, oc) - radius2;
        float disc = b * b - 4.0f * a * c;
        if (disc < 0.0f) return false;
        t = (-b - rtf::sqrt(disc)) / (2.0f * a);
        return t > 0.0f;
    } else if (type == 1) {
        float4 h2 = uni_load4(sc, obj * RT_HOT_F4 + 2), h3 = uni_load4(sc, obj * RT_HOT_F4 + 3);
        v3 n = V3(h3);
        float denom = dot(n, r.d);
        if (fabsf(denom) > 1e-6f) {
            t = dot(V3(h2) - r.o, n) / denom;
            if (t < 0.0f) return false;
            float4 h4 = uni_load4(sc, obj * RT_HOT_F4 + 4), h5 = uni_load4(sc, obj * RT_HOT_F4 + 5);
            v3 lo = (r.o + r.d * t) - V3(h2);
            float x = dot(lo, V3(h4)), z = dot(lo, V3(h5));
            if (fabsf(x) > h3.w || fabsf(z) > h4.w) return false;
            return true;
        }
        return false;
    }
    return false;
}

__device__ __forceinline__ bool pk_wave_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0ull; }
// The same two tests for the lanes in `pass`, written as predicate algebra: every comparison is evaluated in the
// reference's form (`disc < 0` / `t < 0` / `abs(x) > size` negated, so NaNs fall where the GLSL lets them fall),
// garbage in lanes outside the predicate never reaches the result, and the only branches are wave-uniform skips.
__device__ __forceinline__ bool pk_shape_hit(const SceneLds &sc, const Ray &r, float a, int obj, float radius2, int type,
                                             bool pass, float &t) {
    if (type == 0) {
        const float4 h2 = uni_load4(sc, obj * RT_HOT_F4 + 2);
        const v3 oc = r.o - V3(h2);
        const float b = 2.0f * dot(oc, r.d);
        const float c = dot(oc, oc) - radius2;
        const float disc = b * b - 4.0f * a * c;
        const bool cand = pass & !(disc < 0.0f);
        if (!pk_wave_any(cand)) return false;
        t = (-b - rtf::sqrt(disc)) / (2.0f * a);
        return cand & (t > 0.0f);
    } else if (type == 1) {
        const float4 h2 = uni_load4(sc, obj * RT_HOT_F4 + 2), h3 = uni_load4(sc, obj * RT_HOT_F4 + 3);
        const v3 n = V3(h3);
        const float denom = dot(n, r.d);
        const bool c1 = pass & (fabsf(denom) > 1e-6f);
        if (!pk_wave_any(c1)) return false;
        t = dot(V3(h2) - r.o, n) / denom;
        const bool c2 = c1 & !(t < 0.0f);
        if (!pk_wave_any(c2)) return false;
        const float4 h4 = uni_load4(sc, obj * RT_HOT_F4 + 4), h5 = uni_load4(sc, obj * RT_HOT_F4 + 5);
        const v3 lo = (r.o + r.d * t) - V3(h2);
        const float x = dot(lo, V3(h4)), z = dot(lo, V3(h5));
        const bool inX = !(fabsf(x) > h3.w), inZ = !(fabsf(z) > h4.w);
        return (c2 & inX) & inZ;
    }
    return false;
}

// Section timers of the instrumented (COUNT) build (RT_PK_TIMERS):
// slots [12] closest-hit traversals, [13] a light's packet + candidate masks, [14] its PCF sample loops, [15] the whole wave.
template <int COUNT>
__device__ __forceinline__ unsigned long long pk_clock() {
#if RT_PK_TIMERS
    if (COUNT) return __builtin_readcyclecounter();
#endif
    return 0ull;
}

// Diagnostic counters of the instrumented (COUNT) build, after the ray count:
// [1] packets (rays as seen by a wave), [2] candidate objects summed over packets,
// [3] 64-object cull passes.  Lane 0 of each wave adds.
#if RT_PK_TIMERS
// A timers build accumulates the timer slots in LDS (one wave per workgroup) and adds them to the global counters once, when the
// wave ends; the other diagnostics stay off: their global atomics would sit inside the timed sections (a following vector load
// waits for them).
__shared__ unsigned long long pkTimerAcc[20];
#endif
template <int COUNT>
__device__ __forceinline__ void pk_stat(const SceneLds &sc, int slot, unsigned long long v) {
    if (COUNT) {
#if RT_PK_TIMERS
        if (slot >= 12 && slot < 32 && (threadIdx.x & 63) == 0) pkTimerAcc[slot - 12] += v;
#else
        if ((threadIdx.x & 63) == 0 && sc.stats) atomicAdd(&sc.stats[slot], v);
#endif
    }
}
template <int COUNT>
__device__ __forceinline__ void pk_timers_begin() {
#if RT_PK_TIMERS
    if (COUNT) { if (threadIdx.x < 20) pkTimerAcc[threadIdx.x] = 0ull; __syncthreads(); }
#endif
}
template <int COUNT>
__device__ __forceinline__ void pk_timers_end(const SceneLds &sc) {
#if RT_PK_TIMERS
    if (COUNT) { __syncthreads(); if (threadIdx.x < 20 && sc.stats) atomicAdd(&sc.stats[12 + threadIdx.x], pkTimerAcc[threadIdx.x]); }
#endif
}

// ---- wave reductions (fused DPP; every one of the 64 lanes must be active at the call site) --
// Six values at once (three mins, three maxes): 36 v_min/max_f32_dpp, the six independent
// chains interleaved so that no DPP hazard nops are needed between dependent steps.  After
// the block lane 63 holds the wave-wide results (row_bcast15/31 are gfx9-family DPP controls).
#define PK_STEP(ctrl)                                   \
    "v_min_f32_dpp %0, %0, %0 " ctrl "\n\t"             \
    "v_min_f32_dpp %1, %1, %1 " ctrl "\n\t"             \
    "v_min_f32_dpp %2, %2, %2 " ctrl "\n\t"             \
    "v_max_f32_dpp %3, %3, %3 " ctrl "\n\t"             \
    "v_max_f32_dpp %4, %4, %4 " ctrl "\n\t"             \
    "v_max_f32_dpp %5, %5, %5 " ctrl "\n\t"
__device__ __forceinline__ void wave_minmax6(float &m0, float &m1, float &m2, float &x0, float &x1, float &x2) {
    asm volatile("s_nop 1\n\t"
                 PK_STEP("quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf")
                 PK_STEP("quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf")
                 PK_STEP("row_half_mirror row_mask:0xf bank_mask:0xf")
                 PK_STEP("row_mirror row_mask:0xf bank_mask:0xf")
                 PK_STEP("row_bcast:15 row_mask:0xa bank_mask:0xf")
                 PK_STEP("row_bcast:31 row_mask:0xc bank_mask:0xf")
                 "s_nop 0"
                 : "+v"(m0), "+v"(m1), "+v"(m2), "+v"(x0), "+v"(x1), "+v"(x2));
}
#undef PK_STEP
__device__ __forceinline__ float lane63(float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63)); }
__device__ __forceinline__ bool wave_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0ull; }

struct Box3 { float lox, loy, loz, hix, hiy, hiz; };   // wave-uniform

// Box of v over the lanes with `active` set (inactive lanes contribute the neutral element;
// NaN components are ignored by v_min/v_max and must be handled by the caller).
__device__ __forceinline__ Box3 wave_box(v3 v, bool active) {
    float m0 = active ? v.x : PK_INF, m1 = active ? v.y : PK_INF, m2 = active ? v.z : PK_INF;
    float x0 = active ? v.x : -PK_INF, x1 = active ? v.y : -PK_INF, x2 = active ? v.z : -PK_INF;
    wave_minmax6(m0, m1, m2, x0, x1, x2);
    Box3 b;
    b.lox = lane63(m0); b.loy = lane63(m1); b.loz = lane63(m2);
    b.hix = lane63(x0); b.hiy = lane63(x1); b.hiz = lane63(x2);
    return b;
}

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) < PK_INF; }

// One axis of the packet-vs-AABB interval test: lower bound of every lane's min(t0,t1) and
// upper bound of every lane's max(t0,t1), t0 = (bmin-o)*inv, t1 = (bmax-o)*inv, for
// o in [olo,ohi], inv in [ilo,ihi] (same sign, finite).  Rounded corner products bound the
// lanes' rounded values because fp32 rounding is monotone.
__device__ __forceinline__ void pk_axis(float bmin, float bmax, float olo, float ohi, float ilo, float ihi, bool ok,
                                        float &lb, float &ub, float &ubSmall, float &lbLarge) {
    float a0 = bmin - ohi, a1 = bmin - olo, b0 = bmax - ohi, b1 = bmax - olo;
    float p0 = a0 * ilo, p1 = a0 * ihi, p2 = a1 * ilo, p3 = a1 * ihi;
    float q0 = b0 * ilo, q1 = b0 * ihi, q2 = b1 * ilo, q3 = b1 * ihi;
    const float lo0 = fminf(fminf(p0, p1), fminf(p2, p3)), hi0 = fmaxf(fmaxf(p0, p1), fmaxf(p2, p3));   // t0 in [lo0, hi0]
    const float lo1 = fminf(fminf(q0, q1), fminf(q2, q3)), hi1 = fmaxf(fmaxf(q0, q1), fmaxf(q2, q3));   // t1 in [lo1, hi1]
    // No corner can be NaN here: o and inv boxes are finite with inv != 0 (checked per packet), and
    // objects whose own bounds hold a NaN are kept as candidates by the caller (objNan).
    lb = ok ? fminf(lo0, lo1) : -PK_INF;          // <= min(t0,t1) of every lane
    ub = ok ? fmaxf(hi0, hi1) : PK_INF;           // >= max(t0,t1) of every lane
    // (the opposite bounds: no caller reads them, but without them the shipped kernels' instruction sequences change -- they stay)
    ubSmall = ok ? fminf(hi0, hi1) : PK_INF;      // >= min(t0,t1) of every lane
    lbLarge = ok ? fmaxf(lo0, lo1) : -PK_INF;     // <= max(t0,t1) of every lane
}

// true if any of the six bounds is NaN (inf + -inf also reports true: merely conservative)
__device__ __forceinline__ bool bounds_nan(float4 bmn, float4 bmx) {
    float s = ((bmn.x + bmn.y) + (bmn.z + bmx.x)) + (bmx.y + bmx.z);
    return !(s == s);
}

struct Packet {            // wave-uniform description of one ray packet
    Box3 o, inv;
    bool okx, oky, okz;    // axis usable: all active lanes' 1/d finite, non-zero, same sign
    bool cull;             // false: no culling possible (NaN lanes, non-finite origins)
};

__device__ __forceinline__ Packet make_packet(const Box3 &ob, bool obFinite, v3 inv, const Ray &r, bool active) {
    Packet p;
    p.o = ob;
    p.inv = wave_box(inv, active);
    // any NaN in an active lane's ray disables culling for this packet (such lanes pass or fail
    // intersectAABB on a subset of axes, which the interval test does not model)
    bool lane_nan = active && !((r.o.x == r.o.x) & (r.o.y == r.o.y) & (r.o.z == r.o.z) &
                                (r.d.x == r.d.x) & (r.d.y == r.d.y) & (r.d.z == r.d.z));
    p.cull = obFinite && !wave_any(lane_nan);
    p.okx = finite_f(p.inv.lox) && finite_f(p.inv.hix) && (p.inv.lox > 0.0f || p.inv.hix < 0.0f);
    p.oky = finite_f(p.inv.loy) && finite_f(p.inv.hiy) && (p.inv.loy > 0.0f || p.inv.hiy < 0.0f);
    p.okz = finite_f(p.inv.loz) && finite_f(p.inv.hiz) && (p.inv.loz > 0.0f || p.inv.hiz < 0.0f);
    return p;
}


__device__ __forceinline__ bool box_finite(const Box3 &b) {
    return finite_f(b.lox) && finite_f(b.loy) && finite_f(b.loz) && finite_f(b.hix) && finite_f(b.hiy) && finite_f(b.hiz);
}

// Candidate mask of one 64-object chunk: bit l set unless object (chunk*64 + l) provably fails
// intersectAABB for every active lane.  bmn/bmx = this lane's object's bounds.
__device__ __forceinline__ unsigned long long pk_candidates(const Packet &p, float4 bmn, float4 bmx, bool objValid,
                                                            bool objNan, float maxDist) {
    if (!p.cull) return __builtin_amdgcn_ballot_w64(objValid);
    float lbx, ubx, lby, uby, lbz, ubz, usx, usy, usz, llx, lly, llz;
    pk_axis(bmn.x, bmx.x, p.o.lox, p.o.hix, p.inv.lox, p.inv.hix, p.okx, lbx, ubx, usx, llx);
    pk_axis(bmn.y, bmx.y, p.o.loy, p.o.hiy, p.inv.loy, p.inv.hiy, p.oky, lby, uby, usy, lly);
    pk_axis(bmn.z, bmx.z, p.o.loz, p.o.hiz, p.inv.loz, p.inv.hiz, p.okz, lbz, ubz, usz, llz);
    float enter = fmaxf(fmaxf(lbx, lby), lbz);     // <= every lane's tMin
    float leave = fminf(fminf(ubx, uby), ubz);     // >= every lane's tMax
    // lane test: tMax >= tMin && tMin < maxDist && tMax > 0
    bool dead = (leave < enter) || (enter >= maxDist) || (leave <= 0.0f);
    return __builtin_amdgcn_ballot_w64(objValid && (objNan || !dead));
}

__device__ __forceinline__ void pk_set_ok(Packet &p) {
    p.okx = finite_f(p.inv.lox) && finite_f(p.inv.hix) && (p.inv.lox > 0.0f || p.inv.hix < 0.0f);
    p.oky = finite_f(p.inv.loy) && finite_f(p.inv.hiy) && (p.inv.loy > 0.0f || p.inv.hiy < 0.0f);
    p.okz = finite_f(p.inv.loz) && finite_f(p.inv.hiz) && (p.inv.loz > 0.0f || p.inv.hiz < 0.0f);
}
__device__ __forceinline__ unsigned sign_octant(v3 d) {
    return (__float_as_uint(d.x) >> 31) | ((__float_as_uint(d.y) >> 31) << 1) | ((__float_as_uint(d.z) >> 31) << 2);
}

// (A packet whose directions straddle zero on an axis loses that axis' constraint -- measured (tools/gpu_packet_stats.py): 8 % of
// C2's packets, 25 % of C4's, 20 % of C5's, carrying 10 / 44 / 150 candidates instead of 2 / 9 / 33.  Culling such a packet per
// direction OCTANT bought 3 % on C4 / C5 until the per-lane shape level existed; with it the split cost 2-3 % and spilled more.
// The single-ray form (pk_ray_mask) was removed; the light packets' form in pk_pcf_shadow stays, switched off: DESIGN.md section 18.)

// Closest hit over the packet.  `active` lanes get (index or -1, t = minT); others are untouched.
template <int COUNT>
__device__ __forceinline__ int pk_trace_closest(const SceneLds &sc, int nObj, const Ray &r, bool active,
                                                const Box3 &ob, bool obFinite, float maxDist, float &tOut, unsigned &rays) {
    if (COUNT) rays += active ? 1u : 0u;
    v3 inv;
    rtf::rcp3(r.d.x, r.d.y, r.d.z, inv.x, inv.y, inv.z);
    float a = dot(r.d, r.d);
    float minT = maxDist;
    int hit = -1;
    const Packet pk = make_packet(ob, obFinite, inv, r, active);
    const int lane = threadIdx.x & 63;
    pk_stat<COUNT>(sc, 1, 1);
    if (COUNT) {
        const int nok = (int)pk.okx + (int)pk.oky + (int)pk.okz;
        pk_stat<COUNT>(sc, pk.cull ? 7 - nok : 8, 1);
        pk_stat<COUNT>(sc, 11, (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(active)));
    }
    for (int base = 0; base < nObj; base += 64) {
        float4 bmn = make_float4(0.f, 0.f, 0.f, 0.f), bmx = make_float4(0.f, 0.f, 0.f, 0.f);          // (lanes beyond the scene: objValid is false)
        bool bnan = false;
        if (base + lane < nObj) {
            bmn = pk_bounds(sc, base + lane, 0);
            bmx = pk_bounds(sc, base + lane, 1);
            bnan = bounds_nan(bmn, bmx);
        }
        unsigned long long m = pk_candidates(pk, bmn, bmx, base + lane < nObj, bnan, maxDist);
        pk_stat<COUNT>(sc, 2, (unsigned long long)__builtin_popcountll(m));
        pk_stat<COUNT>(sc, 3, 1);
        if (COUNT) pk_stat<COUNT>(sc, (pk.cull && pk.okx && pk.oky && pk.okz) ? 9 : 10, (unsigned long long)__builtin_popcountll(m));
        while (m) {
            const int bit = __builtin_ctzll(m);
            const int i = base + bit;
            m &= m - 1;
            const float4 h0 = uni_load4(sc, i * RT_HOT_F4), h1 = uni_load4(sc, i * RT_HOT_F4 + 1);
            if (sc.straight & 1) {
            const bool pass = active & aabb_test(r, inv, h0, h1, maxDist);
            if (pk_wave_any(pass)) {
                float t = 0.0f;
                const bool better = pk_shape_hit(sc, r, a, i, h1.w, __float_as_int(h0.w), pass, t) & (t > 0.0f) & (t < minT);
                minT = better ? t : minT;
                hit = better ? i : hit;
            }
            } else {
            if (active && aabb_test(r, inv, h0, h1, maxDist)) {
                float t;
                if (pk_shape_test(sc, r, a, i, h1.w, __float_as_int(h0.w), t) && t > 0.0f && t < minT) {
                    minT = t;
                    hit = i;
                }
            }
            }
        }
    }
    tOut = minT;
    return hit;
}

// Closest hit for NR rays of one origin per lane in ONE traversal (computeSubsurfaceScattering's four probes, :327-337): one
// packet spanning the group, one candidate mask, every candidate record fetched once.  Candidates are visited in index order
// and each ray keeps its own (minT, hit) under the same strict `t < minT` as pk_trace_closest, so every ray's result is the
// single-ray one.
template <int COUNT, int NR>
__device__ __forceinline__ void pk_trace_closest_group(const SceneLds &sc, int nObj, v3 origin, const v3 (&d)[NR], bool active, const Box3 &ob,
                                                       bool obFinite, float maxDist, int (&hit)[NR], float (&tOut)[NR], unsigned &rays) {
    if (COUNT) rays += active ? (unsigned)NR : 0u;
    v3 inv[NR];
    bool dirNan = false;
#pragma unroll
    for (int k = 0; k < NR; k++) {
        rtf::rcp3(d[k].x, d[k].y, d[k].z, inv[k].x, inv[k].y, inv[k].z);
        dirNan |= !((d[k].x == d[k].x) & (d[k].y == d[k].y) & (d[k].z == d[k].z));
        hit[k] = -1;
        tOut[k] = maxDist;
    }
    Packet pk;
    pk.o = ob;
    {
        float m0 = PK_INF, m1 = PK_INF, m2 = PK_INF, x0 = -PK_INF, x1 = -PK_INF, x2 = -PK_INF;
#pragma unroll
        for (int k = 0; k < NR; k++) {
            m0 = fminf(m0, inv[k].x); m1 = fminf(m1, inv[k].y); m2 = fminf(m2, inv[k].z);
            x0 = fmaxf(x0, inv[k].x); x1 = fmaxf(x1, inv[k].y); x2 = fmaxf(x2, inv[k].z);
        }
        m0 = active ? m0 : PK_INF; m1 = active ? m1 : PK_INF; m2 = active ? m2 : PK_INF;
        x0 = active ? x0 : -PK_INF; x1 = active ? x1 : -PK_INF; x2 = active ? x2 : -PK_INF;
        wave_minmax6(m0, m1, m2, x0, x1, x2);
        pk.inv.lox = lane63(m0); pk.inv.loy = lane63(m1); pk.inv.loz = lane63(m2);
        pk.inv.hix = lane63(x0); pk.inv.hiy = lane63(x1); pk.inv.hiz = lane63(x2);
    }
    const bool lane_nan = active && (dirNan || !((origin.x == origin.x) & (origin.y == origin.y) & (origin.z == origin.z)));
    pk.cull = obFinite && !wave_any(lane_nan);
    pk_set_ok(pk);
    const int lane = threadIdx.x & 63;
    pk_stat<COUNT>(sc, 1, NR);
    if (COUNT) {
        const int nok = (int)pk.okx + (int)pk.oky + (int)pk.okz;
        pk_stat<COUNT>(sc, pk.cull ? 7 - nok : 8, NR);
        pk_stat<COUNT>(sc, 11, (unsigned long long)NR * (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(active)));
    }
    for (int base = 0; base < nObj; base += 64) {
        float4 bmn = make_float4(0.f, 0.f, 0.f, 0.f), bmx = make_float4(0.f, 0.f, 0.f, 0.f);          // (lanes beyond the scene: objValid is false)
        bool bnan = false;
        if (base + lane < nObj) {
            bmn = pk_bounds(sc, base + lane, 0);
            bmx = pk_bounds(sc, base + lane, 1);
            bnan = bounds_nan(bmn, bmx);
        }
        unsigned long long m = pk_candidates(pk, bmn, bmx, base + lane < nObj, bnan, maxDist);
        pk_stat<COUNT>(sc, 2, (unsigned long long)NR * (unsigned long long)__builtin_popcountll(m));
        pk_stat<COUNT>(sc, 3, 1);
        if (COUNT) pk_stat<COUNT>(sc, (pk.cull && pk.okx && pk.oky && pk.okz) ? 9 : 10, (unsigned long long)NR * (unsigned long long)__builtin_popcountll(m));
        while (m) {
            const int bit = __builtin_ctzll(m);
            const int i = base + bit;
            m &= m - 1;
            const float4 h0 = uni_load4(sc, i * RT_HOT_F4), h1 = uni_load4(sc, i * RT_HOT_F4 + 1);
            const int type = __float_as_int(h0.w);
#pragma unroll
            for (int k = 0; k < NR; k++) {
                Ray r;
                r.o = origin; r.d = d[k];
                if (active && aabb_test(r, inv[k], h0, h1, maxDist)) {
                    float t;
                    if (pk_shape_test(sc, r, dot(d[k], d[k]), i, h1.w, type, t) && t > 0.0f && t < tOut[k]) {
                        tOut[k] = t;
                        hit[k] = i;
                    }
                }
            }
        }
    }
}

// Any-hit over the packet (see trace_any): true for active lanes with an occluder in (0, limit).
template <int COUNT>
__device__ __forceinline__ bool pk_trace_any(const SceneLds &sc, int nObj, const Ray &r, bool active, const Box3 &ob,
                                             bool obFinite, float maxDist, float limit, unsigned &rays) {
    if (COUNT) rays += active ? 1u : 0u;
    v3 inv;
    rtf::rcp3(r.d.x, r.d.y, r.d.z, inv.x, inv.y, inv.z);
    float a = dot(r.d, r.d);
    bool todo = active;          // lanes still looking for an occluder
    const Packet pk = make_packet(ob, obFinite, inv, r, active);
    const int lane = threadIdx.x & 63;
    pk_stat<COUNT>(sc, 1, 1);
    if (COUNT) {
        const int nok = (int)pk.okx + (int)pk.oky + (int)pk.okz;
        pk_stat<COUNT>(sc, pk.cull ? 7 - nok : 8, 1);
        pk_stat<COUNT>(sc, 11, (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(active)));
    }
    for (int base = 0; base < nObj; base += 64) {
        float4 bmn = make_float4(0.f, 0.f, 0.f, 0.f), bmx = make_float4(0.f, 0.f, 0.f, 0.f);          // (lanes beyond the scene: objValid is false)
        bool bnan = false;
        if (base + lane < nObj) {
            bmn = pk_bounds(sc, base + lane, 0);
            bmx = pk_bounds(sc, base + lane, 1);
            bnan = bounds_nan(bmn, bmx);
        }
        unsigned long long m = pk_candidates(pk, bmn, bmx, base + lane < nObj, bnan, maxDist);
        pk_stat<COUNT>(sc, 2, (unsigned long long)__builtin_popcountll(m));
        pk_stat<COUNT>(sc, 3, 1);
        if (COUNT) pk_stat<COUNT>(sc, (pk.cull && pk.okx && pk.oky && pk.okz) ? 9 : 10, (unsigned long long)__builtin_popcountll(m));
        while (m) {
            const int bit = __builtin_ctzll(m);
            const int i = base + bit;
            m &= m - 1;
            const float4 h0 = uni_load4(sc, i * RT_HOT_F4), h1 = uni_load4(sc, i * RT_HOT_F4 + 1);
            if (sc.straight & 2) {
            const bool pass = todo & aabb_test(r, inv, h0, h1, maxDist);
            if (pk_wave_any(pass)) {
                float t = 0.0f;
                const bool occ = pk_shape_hit(sc, r, a, i, h1.w, __float_as_int(h0.w), pass, t) & (t > 0.0f) & (t < limit);
                todo = todo & !occ;
            }
            } else {
            if (todo && aabb_test(r, inv, h0, h1, maxDist)) {
                float t;
                if (pk_shape_test(sc, r, a, i, h1.w, __float_as_int(h0.w), t) && t > 0.0f && t < limit) todo = false;
            }
            }
            if (!wave_any(todo)) return active;     // every active lane is occluded
        }
    }
    return active && !todo;
}

// Any-hit for NR rays of one origin per lane whose results are only OR-ed (pcssShadow's blocker search, :409-427): one packet
// (the reciprocal box spans all of them), one candidate mask and one fetch of every candidate record for the group; a lane
// stops testing as soon as any of its rays is occluded.  Each ray's own test is the exact one of pk_trace_any.
template <int COUNT, int NR>
__device__ __forceinline__ bool pk_trace_any_group(const SceneLds &sc, int nObj, v3 origin, const v3 (&d)[NR], bool active, const Box3 &ob,
                                                   bool obFinite, float maxDist, float limit, unsigned &rays) {
    if (COUNT) rays += active ? (unsigned)NR : 0u;
    v3 inv[NR];
    bool dirNan = false;
#pragma unroll
    for (int k = 0; k < NR; k++) {
        rtf::rcp3(d[k].x, d[k].y, d[k].z, inv[k].x, inv[k].y, inv[k].z);
        dirNan |= !((d[k].x == d[k].x) & (d[k].y == d[k].y) & (d[k].z == d[k].z));
    }
    bool todo = active;          // lanes still looking for an occluder on any of their rays
    Packet pk;
    pk.o = ob;
    {
        float m0 = PK_INF, m1 = PK_INF, m2 = PK_INF, x0 = -PK_INF, x1 = -PK_INF, x2 = -PK_INF;
#pragma unroll
        for (int k = 0; k < NR; k++) {
            m0 = fminf(m0, inv[k].x); m1 = fminf(m1, inv[k].y); m2 = fminf(m2, inv[k].z);
            x0 = fmaxf(x0, inv[k].x); x1 = fmaxf(x1, inv[k].y); x2 = fmaxf(x2, inv[k].z);
        }
        m0 = active ? m0 : PK_INF; m1 = active ? m1 : PK_INF; m2 = active ? m2 : PK_INF;
        x0 = active ? x0 : -PK_INF; x1 = active ? x1 : -PK_INF; x2 = active ? x2 : -PK_INF;
        wave_minmax6(m0, m1, m2, x0, x1, x2);
        pk.inv.lox = lane63(m0); pk.inv.loy = lane63(m1); pk.inv.loz = lane63(m2);
        pk.inv.hix = lane63(x0); pk.inv.hiy = lane63(x1); pk.inv.hiz = lane63(x2);
    }
    // (a NaN in any ray of an active lane disables culling for the group, as in make_packet)
    const bool lane_nan = active && (dirNan || !((origin.x == origin.x) & (origin.y == origin.y) & (origin.z == origin.z)));
    pk.cull = obFinite && !wave_any(lane_nan);
    pk_set_ok(pk);
    const int lane = threadIdx.x & 63;
    pk_stat<COUNT>(sc, 1, NR);
    if (COUNT) {
        const int nok = (int)pk.okx + (int)pk.oky + (int)pk.okz;
        pk_stat<COUNT>(sc, pk.cull ? 7 - nok : 8, NR);
        pk_stat<COUNT>(sc, 11, (unsigned long long)NR * (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(active)));
    }
    for (int base = 0; base < nObj; base += 64) {
        float4 bmn = make_float4(0.f, 0.f, 0.f, 0.f), bmx = make_float4(0.f, 0.f, 0.f, 0.f);          // (lanes beyond the scene: objValid is false)
        bool bnan = false;
        if (base + lane < nObj) {
            bmn = pk_bounds(sc, base + lane, 0);
            bmx = pk_bounds(sc, base + lane, 1);
            bnan = bounds_nan(bmn, bmx);
        }
        unsigned long long m = pk_candidates(pk, bmn, bmx, base + lane < nObj, bnan, maxDist);
        pk_stat<COUNT>(sc, 2, (unsigned long long)NR * (unsigned long long)__builtin_popcountll(m));
        pk_stat<COUNT>(sc, 3, 1);
        if (COUNT) pk_stat<COUNT>(sc, (pk.cull && pk.okx && pk.oky && pk.okz) ? 9 : 10, (unsigned long long)NR * (unsigned long long)__builtin_popcountll(m));
        while (m) {
            const int bit = __builtin_ctzll(m);
            const int i = base + bit;
            m &= m - 1;
            const float4 h0 = uni_load4(sc, i * RT_HOT_F4), h1 = uni_load4(sc, i * RT_HOT_F4 + 1);
            const int type = __float_as_int(h0.w);
#pragma unroll
            for (int k = 0; k < NR; k++) {
                Ray r;
                r.o = origin; r.d = d[k];
                if (todo && aabb_test(r, inv[k], h0, h1, maxDist)) {
                    float t;          // (dot(d,d) re-evaluated here, for the few candidates that pass the slab test, instead of living in NR registers)
                    if (pk_shape_test(sc, r, dot(d[k], d[k]), i, h1.w, type, t) && t > 0.0f && t < limit) todo = false;
                }
            }
            if (!wave_any(todo)) return active;     // every active lane has its blocker
        }
    }
    return active && !todo;
}

// NR blocker rays of one origin per lane against the lanes' own candidate masks (the blocker table's cell of each lane: st_lane_mask
// <1, true>): the wave walks the union of the masks of the lanes still searching; a lane tests a candidate only if its own mask
// lists it.  No packet, reciprocal box or cull pass per group.  Each ray's own slab / shape test is the exact one of pk_trace_any.
template <int COUNT, int NR, int NW>
__device__ __forceinline__ bool pk_trace_any_group_masked(const SceneLds &sc, v3 origin, const v3 (&d)[NR], bool active, const unsigned (&laneMask)[NW],
                                                          float maxDist, float limit, unsigned &rays) {
    if (COUNT) rays += active ? (unsigned)NR : 0u;
    v3 inv[NR];
#pragma unroll
    for (int k = 0; k < NR; k++) rtf::rcp3(d[k].x, d[k].y, d[k].z, inv[k].x, inv[k].y, inv[k].z);
    bool todo = active;
    unsigned wm[NW];
#pragma unroll
    for (int k = 0; k < NW; k++) wm[k] = active ? laneMask[k] : 0u;
    wave_or<NW>(wm);
    pk_stat<COUNT>(sc, 1, NR);
#pragma unroll
    for (int w = 0; w < NW; w++) {
        unsigned m = wm[w];
        pk_stat<COUNT>(sc, 2, (unsigned long long)NR * (unsigned long long)__builtin_popcount(m));
        while (m) {
            const int bit = __builtin_ctz(m);
            const int i = 32 * w + bit;
            m &= m - 1u;
            const bool mine = todo && ((laneMask[w] >> bit) & 1u);
            if (!wave_any(mine)) continue;          // the lanes that listed it have found their blocker meanwhile
            const float4 h0 = uni_load4(sc, i * RT_HOT_F4), h1 = uni_load4(sc, i * RT_HOT_F4 + 1);
            const int type = __float_as_int(h0.w);
#pragma unroll
            for (int k = 0; k < NR; k++) {
                Ray r;
                r.o = origin; r.d = d[k];
                if (mine && todo && aabb_test(r, inv[k], h0, h1, maxDist)) {
                    float t;
                    if (pk_shape_test(sc, r, dot(d[k], d[k]), i, h1.w, type, t) && t > 0.0f && t < limit) todo = false;
                }
            }
            if (!wave_any(todo)) return active;
        }
    }
    return active && !todo;
}

// (Round 3, measured and removed: a per-LANE candidate mask for pcssShadow's blocker fan in the few-object profile -- every lane's
// 16 blocker rays lie in the plane through its origin spanned by lightDir and (1,1,1), so a sphere whose centre is further than
// its radius (+ rounding margins) from that plane, or beside / behind / beyond the fan by the tests of the PCF shape level with
// the fan's angle bound, can leave the lane's 32-bit mask; the four ray groups then walk the union of the masks without any
// packet or cull pass.  Bit-identical on the whole suite and it prunes as intended -- candidates per blocker packet 3.82 -> 2.20
// on C3 (tools/gpu_packet_stats.py) -- but 18 objects x ~45 VALU per lane and light cost what the saved candidate trips bring:
// C3 3.39 -> 3.57 ms; with the next object's records prefetched 3.65, with the plane test alone 3.81.  DESIGN.md section 4 item 32.)

// (Measured and removed: a convergent-packet "wedge" cull of the shadow rays toward point / area lights -- the rays of one light
// lie in the double cone through the light and the packet's origin box, a far smaller set than origin box + t * direction box.
// Bit-identical on 300 fuzz seeds and it pruned as modelled -- candidates per packet at 1080p: C4 16.3 -> 12.0, C5 50.3 -> 31.5 --
// but its ~130 VALU per cull pass and the extra SGPR pressure cost more than the pruned tests saved at the configs' own sizes:
// C4 8.38 -> 9.14 ms, C5 41.1 -> 47.0 ms applied always; 8.50 / 40.3 ms applied only to chunks with >= 16 candidates.  The shadow
// tables have since taken over these scenes.  DESIGN.md section 4 and section 18.)

// pcfShadow (:342-397) for a packet: ONE candidate mask per light serves all pcfSamples rays.
// The jittered directions are jd = normalize(L + rx*T*fs + ry*B*fs) with rx,ry in [0,1), |T| = 1,
// |B| <= 1, so every component lies within delta = 4|fs|/(1-2|fs|) of L's (2|fs| for the
// un-normalised directional form); the packet's direction box is L's box widened by delta
// (+1 % and 2e-5 of slack for the fp32 evaluation), and 1/x is monotone on a sign-definite
// interval, which gives the reciprocal box without a second reduction.
// NWT > 0: the light's candidate masks come from its shadow table (rt_shadowtab.inc; NWT dwords per cell, li = the light's
// index, nn = dot(N, N) of the shading normal) instead of the packet's interval tests below.
template <int COUNT, int GROUPN, int CACHE = 1, bool REACH = false, int NWT = 0>
__device__ __forceinline__ float pk_pcf_shadow(const SceneLds &sc, int nObj, v3 origin, bool need, const Box3 &ob,
                                               bool obFinite, int ltype,
                                               int pcfSamples, float filterSize, v3 lightDir, float limit, float nz,
                                               float maxDist, unsigned &rays, int tabF4 = -1, v3 lightPos = V3(0.f, 0.f, 0.f),
                                               float lightDist = 0.0f, int li = 0, float nn = 0.0f) {
    const int lane = threadIdx.x & 63;
    const unsigned long long tEnter = pk_clock<COUNT>();
    // every sample tabulated (directional light, no noise): the jitter frame is not needed
    const bool allTab = tabF4 >= 0 && pcfSamples <= RT_PCF_TAB_N;          // wave-uniform
    v3 tangent = V3(0.0f, 0.0f, 0.0f), bitangent = tangent;
    if (!allTab) {
        tangent = normalize(cross(lightDir, V3(0.0f, 1.0f, 0.0f)));
        bitangent = cross(lightDir, tangent);
    }
    if (GROUPN <= 1 && pcfSamples > 32) {      // beyond the per-lane sample bitmask: one packet per ray
        float shadow = 0.0f;
        for (int s = 0; s < pcfSamples; s++) {
            float rx = fract(pk_halton(sc, 0, s, 2) + nz);
            float ry = fract(pk_halton(sc, 1, s, 3) + 0.0f);
            v3 jd = (lightDir + (tangent * rx) * filterSize) + (bitangent * ry) * filterSize;
            if (ltype != 1) jd = normalize(jd);
            Ray sr; sr.o = origin; sr.d = jd;
            bool occ = pk_trace_any<COUNT>(sc, nObj, sr, need, ob, obFinite, maxDist, limit, rays);
            shadow += occ ? 0.0f : 1.0f;
        }
        return shadow / (float)pcfSamples;
    }
    if (COUNT) rays += need ? (unsigned)pcfSamples : 0u;

    // ---- the light's packet
    Packet pk;
    pk.o = ob;
    const float fsA = fabsf(__int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(filterSize))));
    Box3 lb;
    lb.lox = lb.hix = lb.loy = lb.hiy = lb.loz = lb.hiz = 0.0f;
    if constexpr (NWT == 0) {
    if (ltype == 1) {      // a directional light's direction is the same for every lane: its box is the vector itself
        const float ux = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(lightDir.x)));
        const float uy = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(lightDir.y)));
        const float uz = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(lightDir.z)));
        lb.lox = lb.hix = ux; lb.loy = lb.hiy = uy; lb.loz = lb.hiz = uz;
    } else {
        lb = wave_box(lightDir, need);
    }
    const bool originNan = wave_any(need && !((origin.x == origin.x) & (origin.y == origin.y) & (origin.z == origin.z)));
    pk.cull = obFinite && !originNan && fsA < 0.2f;
    } else {
    pk.cull = fsA < 0.2f;       // (table path: only the per-lane shape level below reads it; a NaN origin keeps its candidates there)
    pk.okx = pk.oky = pk.okz = false;
    pk.inv = lb;
    }
    // The reciprocal box only has to CONTAIN the reciprocals (it feeds the conservative cull, never a pixel), so the
    // six wave-uniform divisions need not be IEEE: v_rcp_f32 (1 ulp) widened outward by 3e-7 relative is rigorous
    // and a third of the instructions.  The 1 % slack of the jitter bound likewise absorbs the approximate division.
    const float delta = (4.0f * fsA * __builtin_amdgcn_rcpf(1.0f - 2.0f * fsA)) * 1.01f + 2e-5f;
    auto rcp_lo = [](float x) { const float r = __builtin_amdgcn_rcpf(x); return r - fabsf(r) * 3e-7f; };
    auto rcp_hi = [](float x) { const float r = __builtin_amdgcn_rcpf(x); return r + fabsf(r) * 3e-7f; };
    // reciprocal-direction box of the jittered rays from the box of the lanes' light directions
    auto inv_box = [&](const Box3 &b, Packet &p) {
        float dlo = b.lox - delta, dhi = b.hix + delta;
        p.inv.lox = rcp_lo(dhi); p.inv.hix = rcp_hi(dlo);
        p.okx = (dlo > 0.0f || dhi < 0.0f) && finite_f(p.inv.lox) && finite_f(p.inv.hix);
        dlo = b.loy - delta; dhi = b.hiy + delta;
        p.inv.loy = rcp_lo(dhi); p.inv.hiy = rcp_hi(dlo);
        p.oky = (dlo > 0.0f || dhi < 0.0f) && finite_f(p.inv.loy) && finite_f(p.inv.hiy);
        dlo = b.loz - delta; dhi = b.hiz + delta;
        p.inv.loz = rcp_lo(dhi); p.inv.hiz = rcp_hi(dlo);
        p.okz = (dlo > 0.0f || dhi < 0.0f) && finite_f(p.inv.loz) && finite_f(p.inv.hiz);
    };
    if constexpr (NWT == 0) inv_box(lb, pk);
    // Candidate mask of one chunk for this light's rays.  `split` (false in every profile): when the lanes' light directions straddle
    // zero on an axis (a light roughly above the tile: x and z change sign across it), the packet is culled per OCTANT of the light
    // direction -- each sub-packet's direction box is its lanes' light-direction box widened by the jitter bound, so it still
    // contains every jittered ray of its lanes (a component within `delta` of zero simply keeps straddling and loses the axis).
    // (Stays although no profile switches it on: without this branch the table-less kernels compile 2.5 % slower, DESIGN.md section 18.)
    const bool splitLight = NWT == 0 && sc.split && ltype != 1 && pk.cull && !(pk.okx && pk.oky && pk.okz);       // wave-uniform
    auto light_mask = [&](float4 bmn, float4 bmx, bool objValid, bool objNan) -> unsigned long long {
        if (splitLight) {
            const unsigned oct = sign_octant(lightDir);
            unsigned long long rem = __builtin_amdgcn_ballot_w64(need), m = 0ull;
            while (rem) {
                const unsigned o = (unsigned)__builtin_amdgcn_readlane((int)oct, __builtin_ctzll(rem));
                const bool sel = need && oct == o;
                rem &= ~__builtin_amdgcn_ballot_w64(sel);
                Packet q;
                q.o = pk.o;
                q.cull = true;
                inv_box(wave_box(lightDir, sel), q);
                m |= pk_candidates(q, bmn, bmx, objValid, objNan, maxDist);
            }
            return m;
        }
        return pk_candidates(pk, bmn, bmx, objValid, objNan, maxDist);
    };
    // ---- table path: every lane gathers its cell, the wave ORs the masks (NWT dwords = up to CACHE 64-object chunks)
    unsigned long long tm[CACHE];
#pragma unroll
    for (int c = 0; c < CACHE; c++) tm[c] = 0ull;
    if constexpr (NWT > 0) {
        static_assert(NWT <= 2 * CACHE, "the table's dwords must fit the cached chunk masks");
        // (the gather is issued HERE, at its point of use: requesting it in the light loop as soon as the light vector is known, so that
        //  its L2 latency overlaps the lit test, measured 5-9 % SLOWER on C2 and 3 % on C4 -- the cell's registers live across the test)
        unsigned mw[NWT];
        st_lane_mask<NWT>(sc, li, nObj, origin, lightPos, lightDir, lightDist, nn, need, mw);
        wave_or<NWT>(mw);
#pragma unroll
        for (int c = 0; c < CACHE; c++) {
            const unsigned lo = (2 * c < NWT) ? mw[(2 * c < NWT) ? 2 * c : 0] : 0u, hi = (2 * c + 1 < NWT) ? mw[(2 * c + 1 < NWT) ? 2 * c + 1 : 0] : 0u;
            tm[c] = (unsigned long long)lo | ((unsigned long long)hi << 32);
        }
        pk_stat<COUNT>(sc, 1, (unsigned long long)pcfSamples);
#pragma unroll
        for (int c = 0; c < CACHE; c++) pk_stat<COUNT>(sc, 2, (unsigned long long)__builtin_popcountll(tm[c]) * (unsigned long long)pcfSamples);
    }
    if (COUNT && NWT == 0) {        // the light's packet, once per light: the same coherence diagnostics as the single-ray packets
        const int nok = (int)pk.okx + (int)pk.oky + (int)pk.okz;
        pk_stat<COUNT>(sc, pk.cull ? 7 - nok : 8, (unsigned long long)pcfSamples);
        pk_stat<COUNT>(sc, 11, (unsigned long long)pcfSamples * __builtin_popcountll(__builtin_amdgcn_ballot_w64(need)));
    }

    if constexpr (GROUPN > 1) {
    // ---- samples in groups of GROUPN: the rays of a group are set up together (GROUPN
    // independent normalize / reciprocal chains for the scheduler to interleave) and every
    // candidate object is fetched from LDS once and tested against all four.
    // The light's candidate masks are computed ONCE and serve every sample group: up to CACHE (a profile constant) 64-object chunks
    // are cached in SGPR pairs (256 objects; recomputing them per group cost a fifth of C5's frame), larger scenes
    // recompute per group.
    const int nChunks = (nObj + 63) >> 6;
    const bool cached = NWT > 0 || nChunks <= CACHE;          // wave-uniform (a table always covers the scene)
    unsigned long long cm[CACHE];
#if RT_PK_TIMERS
    const unsigned long long tSetup = pk_clock<COUNT>();
    pk_stat<COUNT>(sc, 16, tSetup - tEnter);                       // [16] light packet set-up (before the masks)
    if (splitLight) pk_stat<COUNT>(sc, 18, 1); else pk_stat<COUNT>(sc, 19, 1);      // [18]/[19] split / unsplit light packets
#endif
#pragma unroll
    for (int c = 0; c < CACHE; c++) {
        cm[c] = tm[c];
        if (NWT == 0 && cached && c < nChunks) {
            const int base = c * 64;
            float4 b0 = make_float4(0.f, 0.f, 0.f, 0.f), b1 = make_float4(0.f, 0.f, 0.f, 0.f);
            bool bn = false;
            if (base + lane < nObj) { b0 = pk_bounds(sc, base + lane, 0); b1 = pk_bounds(sc, base + lane, 1); bn = bounds_nan(b0, b1); }
            cm[c] = light_mask(b0, b1, base + lane < nObj, bn);
            if (c == 0) pk_stat<COUNT>(sc, 1, (unsigned long long)pcfSamples);
            pk_stat<COUNT>(sc, 2, (unsigned long long)__builtin_popcountll(cm[c]) * (unsigned long long)pcfSamples);
            pk_stat<COUNT>(sc, (pk.cull && pk.okx && pk.oky && pk.okz) ? 9 : 10, (unsigned long long)__builtin_popcountll(cm[c]) * (unsigned long long)pcfSamples);
            pk_stat<COUNT>(sc, 3, 1);
        }
    }
    // ---- second cull level, per LANE and on the SHAPE: can any of this lane's jittered rays toward the light hit the candidate?
    // The packet test above treats the lanes' origins and light directions as independent boxes; for the incoherent packets of
    // deep bounces it keeps several times the objects any single lane can reach (C5: 16.5 candidate trips per sample pair, a
    // lane passes even the slab test in 20 % of them).  A candidate that no lane can hit may leave the light's mask whatever
    // its AABB says -- intersectObjects only reports it through intersectSphere (:105-118) -- so the test is made on the
    // sphere itself, once per (lane, candidate) for ALL of the lane's samples:
    //   * every sample direction is lightDir + (tangent*rx + bitangent*ry)*filterSize with rx, ry in [0,1) and a unit frame
    //     orthogonal to lightDir (cross products with exact zeros: rt_packet's PCF set-up), normalised or not; as a unit
    //     vector it is within eta = sqrt(2)*|filterSize| (+0.1 %) of lightDir;
    //   * with OC = centre - origin, s = |OC|, p = OC.lightDir: the sphere's distance from the line of sample k is at least
    //     sqrt(s^2 - p^2) - s*eta, every point of it has ray parameter within p +- (r + s*eta);
    //   * fp32: the kernel's discriminant b^2 - 4ac equals 4(a r^2 - |OC x d|^2) up to 40 roundings of magnitude a(s^2 + r^2),
    //     i.e. it can report a hit only if dist^2 <= r^2 + 6e-7 (s^2 + r^2); the margins below are 2e-5 (s^2 + r^2) on the
    //     squared distance and 1e-4 s on the ray parameter, 30-100 times that, and absorb this block's own roundings too.
    // So: unreachable  <=  s^2 - p^2 > (|r| + s*eta')^2 + 2e-5 (s^2 + r^2)   (passes beside it)
    //                  or  p + |r| + s*eta' < 0                               (wholly behind the origin: t > 0 fails)
    //                  or  p - |r| - s*eta' > limit   (point / area lights)   (wholly beyond the light: t < limit fails)
    // with eta' = eta + 1e-4.  NaN / infinite operands make the comparisons false (the candidate stays) except s^2 = inf, where
    // the exact test cannot report a hit either (its discriminant is -inf or NaN); planes and unknown types always stay (testing
    // them on their AABB here as well was measured and removed: DESIGN.md section 4 item 16).
    // ~28 VALU per candidate against two exact slab tests per candidate and PAIR of samples: pays from 3 samples per light on.
    if constexpr (REACH) {
    if (cached && pk.cull && pcfSamples >= RT_PK_REACH_MIN_SAMPLES) {          // wave-uniform
        const float etaP = fsA * 1.41563f + 1.02e-4f;
#pragma unroll
        for (int c = 0; c < CACHE; c++) {
            unsigned long long m = cm[c], keep = 0ull;
            while (m) {
                const int bit = __builtin_ctzll(m);
                m &= m - 1;
                const int i = c * 64 + bit;
                const float4 h0 = uni_load4(sc, i * RT_HOT_F4);
                bool reach = need;
                if (__float_as_int(h0.w) == 0) {          // sphere (wave-uniform)
                    const float4 h2 = uni_load4(sc, i * RT_HOT_F4 + 2);
                    const v3 oc = V3(h2) - origin;
                    const float m2 = dot(oc, oc), p = dot(oc, lightDir);
                    const float rA = fabsf(h2.w);
                    const float rr = rA + __builtin_amdgcn_sqrtf(m2) * etaP;
                    const bool beside = (m2 - p * p) > rr * rr + 2e-5f * (m2 + rA * rA);
                    const bool behind = p + rr < 0.0f;
                    const bool beyond = (ltype != 1) && (p - rr > limit);
                    reach = need && !(beside || behind || beyond);
                }
                if (wave_any(reach)) keep |= 1ull << bit;
            }
            pk_stat<COUNT>(sc, 20, (unsigned long long)__builtin_popcountll(cm[c]));     // [20] candidates entering / [21] leaving the lane level
            pk_stat<COUNT>(sc, 21, (unsigned long long)__builtin_popcountll(keep));
            cm[c] = keep;
        }
    }
    } else {
    // (profiles without the shape level -- LIGHT: 3 candidates per packet, nothing to gain at 4 samples -- keep round 2's first form:
    // the AABB interval test for every candidate, from RT_PK_CONE_MIN_SAMPLES samples on)
    if (cached && pk.cull && pcfSamples >= RT_PK_CONE_MIN_SAMPLES) {          // wave-uniform
        v3 ilo, ihi;
        bool okx, oky, okz;
        {
            float dlo = lightDir.x - delta, dhi = lightDir.x + delta;
            ilo.x = rcp_lo(dhi); ihi.x = rcp_hi(dlo);
            okx = (dlo > 0.0f || dhi < 0.0f) && finite_f(ilo.x) && finite_f(ihi.x);
            dlo = lightDir.y - delta; dhi = lightDir.y + delta;
            ilo.y = rcp_lo(dhi); ihi.y = rcp_hi(dlo);
            oky = (dlo > 0.0f || dhi < 0.0f) && finite_f(ilo.y) && finite_f(ihi.y);
            dlo = lightDir.z - delta; dhi = lightDir.z + delta;
            ilo.z = rcp_lo(dhi); ihi.z = rcp_hi(dlo);
            okz = (dlo > 0.0f || dhi < 0.0f) && finite_f(ilo.z) && finite_f(ihi.z);
        }
#pragma unroll
        for (int c = 0; c < CACHE; c++) {
            unsigned long long m = cm[c], keep = 0ull;
            while (m) {
                const int bit = __builtin_ctzll(m);
                m &= m - 1;
                const int i = c * 64 + bit;
                const float4 h0 = uni_load4(sc, i * RT_HOT_F4), h1 = uni_load4(sc, i * RT_HOT_F4 + 1);
                float lbx, ubx, lby, uby, lbz, ubz, u0, u1;
                pk_axis(h0.x, h1.x, origin.x, origin.x, ilo.x, ihi.x, okx, lbx, ubx, u0, u1);
                pk_axis(h0.y, h1.y, origin.y, origin.y, ilo.y, ihi.y, oky, lby, uby, u0, u1);
                pk_axis(h0.z, h1.z, origin.z, origin.z, ilo.z, ihi.z, okz, lbz, ubz, u0, u1);
                const float enter = fmaxf(fmaxf(lbx, lby), lbz), leave = fminf(fminf(ubx, uby), ubz);
                const bool dead = (leave < enter) || (enter >= maxDist) || (leave <= 0.0f);
                if (wave_any(need && (bounds_nan(h0, h1) || !dead))) keep |= 1ull << bit;
            }
            pk_stat<COUNT>(sc, 20, (unsigned long long)__builtin_popcountll(cm[c]));
            pk_stat<COUNT>(sc, 21, (unsigned long long)__builtin_popcountll(keep));
            cm[c] = keep;
        }
    }
    }
    float shadow = 0.0f;
    const unsigned long long tMasks = pk_clock<COUNT>();
    pk_stat<COUNT>(sc, 13, tMasks - tEnter);
#if RT_PK_TIMERS
    if (splitLight) pk_stat<COUNT>(sc, 17, tMasks - tSetup);       // [17] masks of split packets
#endif
    for (int s0 = 0; s0 < pcfSamples; s0 += GROUPN) {
#if RT_PK_TIMERS
        pk_stat<COUNT>(sc, 25, 1);                                               // [25] sample groups (timers build only, like [22..24])
#endif
        Ray sr[GROUPN];
        v3 inv[GROUPN];
        float a[GROUPN];
        bool todo[GROUPN];
#pragma unroll
        for (int k = 0; k < GROUPN; k++) {
            const int s = s0 + k;
            todo[k] = need && s < pcfSamples;
            sr[k].o = origin;
            if (tabF4 >= 0 && s < RT_PCF_TAB_N) {      // directional light, no noise: the ray is tabulated (wave-uniform)
                const float4 t0 = uni_load4(sc, tabF4 + 2 * s), t1 = uni_load4(sc, tabF4 + 2 * s + 1);
                sr[k].d = V3(t0);
                a[k] = t0.w;
                inv[k] = V3(t1);
            } else {
            float rx = fract(pk_halton(sc, 0, s, 2) + nz);
            float ry = fract(pk_halton(sc, 1, s, 3) + 0.0f);
            v3 jd = (lightDir + (tangent * rx) * filterSize) + (bitangent * ry) * filterSize;
            if (ltype != 1) jd = normalize(jd);
            sr[k].d = jd;
            rtf::rcp3(jd.x, jd.y, jd.z, inv[k].x, inv[k].y, inv[k].z);
            a[k] = dot(jd, jd);
            }
        }
        for (int base = 0; base < nObj; base += 64) {
            const int ci = base >> 6;
            unsigned long long m = 0ull;
#pragma unroll
            for (int c = 0; c < CACHE; c++) m = (ci == c) ? cm[c] : m;        // wave-uniform select, no dynamic SGPR index
            if (NWT == 0 && !cached) {
                float4 bmn = make_float4(0.f, 0.f, 0.f, 0.f), bmx = make_float4(0.f, 0.f, 0.f, 0.f);          // (lanes beyond the scene: objValid is false)
                bool bnan = false;
                if (base + lane < nObj) {
                    bmn = pk_bounds(sc, base + lane, 0);
                    bmx = pk_bounds(sc, base + lane, 1);
                    bnan = bounds_nan(bmn, bmx);
                }
                m = light_mask(bmn, bmx, base + lane < nObj, bnan);
                const int ns = pcfSamples - s0 < GROUPN ? pcfSamples - s0 : GROUPN;
                if (base == 0) pk_stat<COUNT>(sc, 1, (unsigned long long)ns);
                pk_stat<COUNT>(sc, 2, (unsigned long long)__builtin_popcountll(m) * (unsigned long long)ns);
                pk_stat<COUNT>(sc, (pk.cull && pk.okx && pk.oky && pk.okz) ? 9 : 10, (unsigned long long)__builtin_popcountll(m) * (unsigned long long)ns);
                pk_stat<COUNT>(sc, 3, 1);
            }
            while (m) {
                bool anyTodo = false;
#pragma unroll
                for (int k = 0; k < GROUPN; k++) anyTodo |= todo[k];
                if (!wave_any(anyTodo)) break;
                const int bit = __builtin_ctzll(m);
                const int i = base + bit;
                m &= m - 1;
                const float4 h0 = uni_load4(sc, i * RT_HOT_F4), h1 = uni_load4(sc, i * RT_HOT_F4 + 1);
                const int type = __float_as_int(h0.w);
#if RT_PK_TIMERS
                pk_stat<COUNT>(sc, 22, 1);                                       // [22] candidate trips of the sample loops
                {
                    bool anyPass = false;
#pragma unroll
                    for (int k = 0; k < GROUPN; k++) anyPass |= todo[k] && aabb_test(sr[k], inv[k], h0, h1, maxDist);
                    if (wave_any(anyPass)) pk_stat<COUNT>(sc, 23, 1);            // [23] ... in which some lane passes the slab test
                    pk_stat<COUNT>(sc, 24, (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(anyPass)));   // [24] lanes passing
                }
#endif
#pragma unroll
                for (int k = 0; k < GROUPN; k++) {
                    if (sc.straight & 4) {
                    const bool pass = todo[k] & aabb_test(sr[k], inv[k], h0, h1, maxDist);
                    if (pk_wave_any(pass)) {
                        float t = 0.0f;
                        const bool occ = pk_shape_hit(sc, sr[k], a[k], i, h1.w, type, pass, t) & (t > 0.0f) & (t < limit);
                        todo[k] = todo[k] & !occ;
                    }
                    } else {
                    if (todo[k] && aabb_test(sr[k], inv[k], h0, h1, maxDist)) {
                        float t;
                        if (pk_shape_test(sc, sr[k], a[k], i, h1.w, type, t) && t > 0.0f && t < limit) todo[k] = false;
                    }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < GROUPN; k++) {
            if (s0 + k < pcfSamples) shadow += (need && !todo[k]) ? 0.0f : 1.0f;
        }
    }
    pk_stat<COUNT>(sc, 14, pk_clock<COUNT>() - tMasks);
    return shadow / (float)pcfSamples;
    } else {
    unsigned occBits = 0;          // bit s: sample s of this lane is occluded (pcfSamples <= 32 here)
    const unsigned long long tMasks = pk_clock<COUNT>();
    pk_stat<COUNT>(sc, 13, tMasks - tEnter);
    for (int base = 0; base < nObj; base += 64) {
        float4 bmn = make_float4(0.f, 0.f, 0.f, 0.f), bmx = make_float4(0.f, 0.f, 0.f, 0.f);          // (lanes beyond the scene: objValid is false)
        bool bnan = false;
        if (NWT == 0 && base + lane < nObj) {
            bmn = pk_bounds(sc, base + lane, 0);
            bmx = pk_bounds(sc, base + lane, 1);
            bnan = bounds_nan(bmn, bmx);
        }
        unsigned long long mask = 0ull;
        if constexpr (NWT > 0) {
#pragma unroll
            for (int c = 0; c < CACHE; c++) mask = ((base >> 6) == c) ? tm[c] : mask;
        } else {
            mask = light_mask(bmn, bmx, base + lane < nObj, bnan);
        }
        if (NWT == 0) {       // (a table-driven light is booked above, in [1] and [2] only: it has no direction box and makes no cull pass)
        pk_stat<COUNT>(sc, 2, (unsigned long long)__builtin_popcountll(mask) * (unsigned long long)pcfSamples);
        pk_stat<COUNT>(sc, (pk.cull && pk.okx && pk.oky && pk.okz) ? 9 : 10, (unsigned long long)__builtin_popcountll(mask) * (unsigned long long)pcfSamples);
        pk_stat<COUNT>(sc, 3, 1);
        if (base == 0) pk_stat<COUNT>(sc, 1, (unsigned long long)pcfSamples);
        }
        if (mask == 0ull) continue;
        for (int s = 0; s < pcfSamples; s++) {
            bool todo = need && !((occBits >> (s & 31)) & 1u);
            if (!wave_any(todo)) continue;
            Ray sr; sr.o = origin;
            v3 inv; float a;
            if (tabF4 >= 0 && s < RT_PCF_TAB_N) {      // directional light, no noise: the ray is tabulated (wave-uniform)
                const float4 t0 = uni_load4(sc, tabF4 + 2 * s), t1 = uni_load4(sc, tabF4 + 2 * s + 1);
                sr.d = V3(t0); a = t0.w; inv = V3(t1);
            } else {
                float rx = fract(pk_halton(sc, 0, s, 2) + nz);
                float ry = fract(pk_halton(sc, 1, s, 3) + 0.0f);
                v3 jd = (lightDir + (tangent * rx) * filterSize) + (bitangent * ry) * filterSize;
                if (ltype != 1) jd = normalize(jd);
                sr.d = jd;
                rtf::rcp3(jd.x, jd.y, jd.z, inv.x, inv.y, inv.z);
                a = dot(jd, jd);
            }
            unsigned long long m = mask;
            while (m) {
                const int bit = __builtin_ctzll(m);
                const int i = base + bit;
                m &= m - 1;
                const float4 h0 = uni_load4(sc, i * RT_HOT_F4), h1 = uni_load4(sc, i * RT_HOT_F4 + 1);
                if (sc.straight & 8) {
                const bool pass = todo & aabb_test(sr, inv, h0, h1, maxDist);
                if (pk_wave_any(pass)) {
                    float t = 0.0f;
                    const bool occ = pk_shape_hit(sc, sr, a, i, h1.w, __float_as_int(h0.w), pass, t) & (t > 0.0f) & (t < limit);
                    todo = todo & !occ;
                }
                } else {
                if (todo && aabb_test(sr, inv, h0, h1, maxDist)) {
                    float t;
                    if (pk_shape_test(sc, sr, a, i, h1.w, __float_as_int(h0.w), t) && t > 0.0f && t < limit) todo = false;
                }
                }
                if (!wave_any(todo)) break;
            }
            if (need && !todo) occBits |= 1u << (s & 31);
        }
    }
    float shadow = 0.0f;
    pk_stat<COUNT>(sc, 14, pk_clock<COUNT>() - tMasks);
    for (int s = 0; s < pcfSamples; s++) shadow += ((occBits >> (s & 31)) & 1u) ? 0.0f : 1.0f;
    return shadow / (float)pcfSamples;
    }
}

// A replaying frame's SETTLED tile (DESIGN.md section 27; render_packet below has the rule and the recording side): where the
// tile's flag says so every lane copies its final record to the three surfaces -- alpha and the zeros
// outside the image regenerated as at the end of render_packet -- and the tile is done.  Called at the very top of the kernel
// with nothing but the kernel's arguments alive and sharing no value with render_packet: placed inside it, the early-out
// cost the replaying instantiations 6-20 more spilled SGPRs over the whole bounce loop (C3 +2.5 %).
__device__ __forceinline__ void pk_replay_settled_tile(const RtFrame &f, int tileX, int tileY, const unsigned char *records, float4 *gColor,
                                                       float4 *gPosition, uint2 *gNormal) {
    const int ln = threadIdx.x & 63;
    const int i = tileX * 8 + (ln & 7), j = tileY * 8 + (ln >> 3);
    if (i < f.p.regionW && j < f.p.regionH) {
        const int gxI = f.p.x0 + i, ly = f.p.y0 + j;
        const int gyI = (ly / f.p.stripRows) * f.p.stripCycleRows + f.p.stripOffsetRows + ly % f.p.stripRows;
        const size_t at = (size_t)j * f.p.regionW + i;
        const size_t out = f.imageStores ? (size_t)gyI * f.p.width + gxI : at;
        if (gxI < f.p.width && gyI < f.p.height) {
            const float4 *fin = (const float4 *)(records + rt_first_hit_finals_offset(f.p.regionW, f.p.regionH)) + 2 * at;
            const float4 a = fin[0], b = fin[1];
            gColor[out] = make_float4(a.x, a.y, a.z, 1.0f);
            gPosition[out] = make_float4(a.w, b.x, b.y, 1.0f);
            gNormal[out] = make_uint2(__float_as_uint(b.z), __float_as_uint(b.w));
        } else if (!f.imageStores) {   // outside the image: GL discards the imageStore (a whole-image surface has no such pixel)
            gColor[out] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            gPosition[out] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            gNormal[out] = make_uint2(0u, 0u);
        }
    }
}

// Parking columns that hand a replaying tile's record from pk_replay_park to render_packet: (t, hit) of a K = 0 tile, the hit
// object of a K >= 1 tile, and K itself (every lane its own copy: nothing travels between lanes, so no access is volatile).
// They are V's columns, which the hit set-up of the first bounce that runs writes for every lane -- behind render_packet's
// reads of these three.
constexpr int PK_PARK_REC_T = 15, PK_PARK_REC_HIT = 16, PK_PARK_REC_K = 17;

// The START of a replaying frame's tile (DESIGN.md section 35) is two steps around the kernel's settled test.
// pk_replay_request issues, without waiting for any of them, the loads whose addresses need only the tile and the kernel's
// arguments: the tile's flag byte, each window lane's (hits, colours) slots -- the whole record of a K = 0 tile, the first 20
// bytes of a prefix record, nothing a settled tile wants (20 bytes per lane it loads for nothing, and 16 more where bounds
// are staged) -- and the lane's share of the first 64 staged bounds.  The kernel waits for all of them together (the lanes
// beyond the window have issued fewer loads, so no count short of zero says that the flag has come) and tests the flag.
// pk_replay_park requests the finals slot where K >= 1,
// finishes the staging and moves each piece from its load straight into the parking column render_packet wants it in:
// nothing of the record is held in a register inside render_packet, whose bounce loop is what a K = 0 tile runs, and a tile
// waits for memory once (K = 0) or twice (K >= 1) behind its tile id where it waited four or five times.  What a lane beyond the
// window parks is what render_packet's own initialisation and the defaults of its loads gave it; such a lane forms no address.
// Ends with the barrier behind the staging; shares no live value with render_packet (section 27's lesson).
struct PkReplayLoads {
    unsigned flag;          // the tile's flag byte (rt_firsthit.h has the encoding), as loaded: not yet uniform
    uint2 w01;              // the hits slot: (t, hit) for K = 0, (hit, finalColor.x) for K >= 1
    float c0, c1, c2;       // the colours slot
    float4 bounds;          // float4 threadIdx.x of the staged bounds
};
template <int BT, bool BOUNDS_LDS>
__device__ __forceinline__ void pk_replay_request(const RtFrame &f, const RtDeviceScene &dsc, int tileX, int tileY, const unsigned char *records,
                                                  PkReplayLoads &ld) {
    const int tilesX = (f.p.regionW + 7) / 8;
    ld.flag = records[rt_first_hit_flags_offset(f.p.regionW, f.p.regionH) + (size_t)(tileY * tilesX + tileX)];
    // (the bounds ahead of the record: the compiler waits for the record's first piece where the window's lanes rejoin the others,
    // and by then everything is in flight)
    ld.bounds = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (BOUNDS_LDS && (int)threadIdx.x < f.nObj * 2) ld.bounds = dsc.compiled[(threadIdx.x >> 1) * RT_HOT_F4 + (threadIdx.x & 1)];
    const int ln = threadIdx.x & 63;
    const int i = tileX * 8 + (ln & 7), j = tileY * 8 + (ln >> 3);
    ld.w01 = make_uint2(0u, 0u);
    ld.c0 = ld.c1 = ld.c2 = 0.0f;
    if (i < f.p.regionW && j < f.p.regionH) {
        const size_t at = (size_t)j * f.p.regionW + i;
        const float *col = (const float *)(records + rt_first_hit_colours_offset(f.p.regionW, f.p.regionH)) + 3 * at;
        ld.w01 = ((const uint2 *)records)[at];
        ld.c0 = col[0]; ld.c1 = col[1]; ld.c2 = col[2];
    }
}
template <int BT, bool BOUNDS_LDS>
__device__ __forceinline__ void pk_replay_park(const RtFrame &f, const RtDeviceScene &dsc, int tileX, int tileY, unsigned flag,
                                               const unsigned char *records, float4 *lds, const PkReplayLoads &ld) {
    const int nF4 = BOUNDS_LDS ? f.nObj * 2 : 0;
    float *pk_ = (float *)(lds + nF4 + 1) + threadIdx.x;          // (sc.park of the kernel)
    int k = rt_prefix_flag_depth(flag);
    if (k > RT_PREFIX_CAP) k = RT_PREFIX_CAP;          // (a flag never holds more)
    const int ln = threadIdx.x & 63;
    const int i = tileX * 8 + (ln & 7), j = tileY * 8 + (ln >> 3);
    const bool inWindow = i < f.p.regionW && j < f.p.regionH;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (k > 0 && inWindow) {
        const float4 *fin = (const float4 *)(records + rt_first_hit_finals_offset(f.p.regionW, f.p.regionH)) + 2 * ((size_t)j * f.p.regionW + i);
        a = fin[0]; b = fin[1];
    }
    if ((int)threadIdx.x < nF4) lds[threadIdx.x] = ld.bounds;
    for (int s = threadIdx.x + BT; s < nF4; s += BT) lds[s] = dsc.compiled[(s >> 1) * RT_HOT_F4 + (s & 1)];
    if (k > 0) {
        const int hitRec = inWindow ? (int)ld.w01.x : -1;
        const int hit = (hitRec >= 0 && hitRec < f.nObj) ? hitRec : -1;      // (a record never holds anything else; no gather may leave the scene)
        const bool alive = hit >= 0;
        pk_[0 * BT] = __uint_as_float(ld.w01.y); pk_[1 * BT] = ld.c0; pk_[2 * BT] = ld.c1;               // finalColor
        pk_[3 * BT] = alive ? a.z : 1.0f; pk_[4 * BT] = alive ? a.w : 1.0f; pk_[5 * BT] = alive ? b.x : 1.0f;    // throughput
        pk_[6 * BT] = b.y; pk_[7 * BT] = b.z; pk_[8 * BT] = b.w;                                         // the incoming direction, if alive
        pk_[9 * BT] = ld.c2; pk_[10 * BT] = a.x; pk_[11 * BT] = a.y;                                     // P of the last hit
        pk_[12 * BT] = alive ? 0.0f : a.z; pk_[13 * BT] = alive ? 0.0f : a.w; pk_[14 * BT] = alive ? 0.0f : b.x;   // N where the path has ended
        pk_[PK_PARK_REC_HIT * BT] = __int_as_float(hit);
    } else {
        pk_[0 * BT] = ld.c0; pk_[1 * BT] = ld.c1; pk_[2 * BT] = ld.c2;         // finalColor after depth 0: the sky or zero where it missed
        pk_[3 * BT] = 1.0f; pk_[4 * BT] = 1.0f; pk_[5 * BT] = 1.0f;            // throughput
        pk_[9 * BT] = 0.0f; pk_[10 * BT] = 0.0f; pk_[11 * BT] = 0.0f;          // P, N of the last hit: undefined locals read as zero (A.3)
        pk_[12 * BT] = 0.0f; pk_[13 * BT] = 0.0f; pk_[14 * BT] = 0.0f;
        pk_[PK_PARK_REC_T * BT] = inWindow ? __uint_as_float(ld.w01.x) : f.p.maxRayDistance;          // a miss where there is no record
        pk_[PK_PARK_REC_HIT * BT] = inWindow ? __uint_as_float(ld.w01.y) : __int_as_float(-1);
    }
    pk_[PK_PARK_REC_K * BT] = __int_as_float(k);
    __syncthreads();
}

// main() of raytracingCs.glsl (:509-584) for one 64-lane packet of pixels.
// FIRST (DESIGN.md section 26; the host side is rt_firsthit.h): 0 = the frame as it always was.  1 = the same frame, which also
// RECORDS what depth 0 ends with, one record of 20 bytes per pixel of the window at window-local index j * regionW + i:
// firstHit[idx] = (t of the closest hit, the hit object or -1 for a miss or a pixel outside the image), and in the buffer's
// `colours` part (rt_firsthit.h has the layout) three floats per pixel, finalColor as parked after depth 0.  2 = REPLAY: depth 0 takes (finalColor, t, hit) from the record in place of
// the closest-hit traversal, the light loop and the subsurface section, recomputes the shading point from them by the
// expressions of the normal frame, and goes on with the next direction and depth 1 as ever.  Every value is copied bitwise or
// recomputed by the identical expression, so the three frames are the same bits.  On top of that the recording frame marks the
// SETTLED tiles and keeps their surface values, and the replaying frame copies those out (below; DESIGN.md section 27); and it
// keeps, for every tile that reaches depth 1 before one of its lanes reads the frame's bounce sample, the path state behind
// the lighting of the last such depth, from which the replaying frame resumes the tile (PREFIX replay, DESIGN.md section 34).
template <int COUNT, int BT, typename PROFILE, int FIRST = 0>
__device__ __forceinline__ void render_packet(const RtFrame &f, const RtDeviceScene &dsc, const SceneLds &sc,
                                              float4 *gColor,
                                              float4 *gPosition, uint2 *gNormal, unsigned &rays, uint2 *firstHit = nullptr) {
    static_assert(BT == 64, "one-wave workgroups: the 8x8 tile and the parking area's stride assume it");
    static_assert(FIRST == 0 || COUNT == 0, "the instrumented builds always trace the whole frame");
    constexpr int GROUPN = PROFILE::groupN;
    const int nObj = f.nObj;
    const float maxDist = f.p.maxRayDistance;
    pk_timers_begin<COUNT>();
    const unsigned long long tWave = pk_clock<COUNT>();

    // lane -> pixel (wave w owns the 8x8 tile (w&1, w>>1) of the 16x16 workgroup tile).  The ids are
    // recomputed at their three points of use instead of staying live across the bounce loop.
    auto pixel = [&](int &gxI, int &gyI, size_t &outIdx) -> bool {
        const int wave = threadIdx.x >> 6, ln = threadIdx.x & 63;
        const int i = sc.tileX * 8 + (wave & 1) * 8 + (ln & 7);
        const int j = sc.tileY * 8 + (wave >> 1) * 8 + (ln >> 3);
        gxI = f.p.x0 + i;
        const int ly = f.p.y0 + j;
        gyI = (ly / f.p.stripRows) * f.p.stripCycleRows + f.p.stripOffsetRows + ly % f.p.stripRows;
        outIdx = f.imageStores ? (size_t)gyI * f.p.width + gxI : (size_t)j * f.p.regionW + i;
        return i < f.p.regionW && j < f.p.regionH;
    };
    // this lane's first-hit record (FIRST != 0): window-local pixel index, or -1 for the lanes of an edge tile beyond the window
    [[maybe_unused]] auto firstIndex = [&]() -> long long {
        const int wave = threadIdx.x >> 6, ln = threadIdx.x & 63;
        const int i = sc.tileX * 8 + (wave & 1) * 8 + (ln & 7);
        const int j = sc.tileY * 8 + (wave >> 1) * 8 + (ln >> 3);
        return (i < f.p.regionW && j < f.p.regionH) ? (long long)j * f.p.regionW + i : -1ll;
    };
    // SETTLED TILES (FIRST != 0, DESIGN.md section 27).  A lane is TAINTED when, alive after the roulette, it takes the diffuse
    // branch of the next-direction step: the only reader of f.hemi, which is the only value of the frame's bounce sample that
    // reaches this function without a noise texture.  A tile none of whose lanes was tainted is SETTLED: its three surface
    // values are the same bits for every frameCount, so the recording frame keeps them (32 bytes per pixel, the buffer's
    // `finals` part) with one flag per tile, and a replaying frame whose tile is flagged copies them out and is done
    // (pk_replay_settled_tile, which the kernel calls ahead of everything else).
    // Bit 0 of a RECORDING launch's record pointer switches it off (rt_device.h): every flag is then written as 0.  The taint
    // is one word of LDS, the block counter's slot ahead of the parking area that only the instrumented builds use: nothing
    // the light loop has to carry in a register; the pointer is masked where it is used for the same reason.  The word travels
    // between lanes, so every access is volatile: no store may be dropped or forwarded to the load behind the loop (LDS
    // operations of one wave complete in order, and the workgroup is that one wave).
    [[maybe_unused]] volatile unsigned *const taintWord = (volatile unsigned *)sc.park - 4;
    [[maybe_unused]] auto records = [&]() -> unsigned char * { return (unsigned char *)((uintptr_t)firstHit & ~RT_FIRST_HIT_SWITCHES); };
    if constexpr (FIRST == 1) *taintWord = 0u;
    // TILE SPLIT (FIRST == 3: a replaying frame launched with a split plan, DESIGN.md section 38).  The tile is run by P one-wave jobs, this one being `part` (P = 1: the tile
    // is whole, and nothing below does anything).  Every job traces the whole path geometry -- closest hits, hit set-up,
    // roulette, next direction: deterministic, so all of them hold the same bits -- but evaluates only the lighting UNITS it
    // owns: unit d * (nLt + 1) + li is light li of depth d, li = nLt that depth's subsurface section, and a job owns the units
    // u with u mod P == part.  A split job adds nothing into finalColor: it stores each owned unit's v3 into the tile's scratch
    // slot (rt_device.h has the layout), part 0 also what the sums need of each depth, and the job that arrives last at the
    // slot's counter replays the additions in the source's order (below, ahead of the surface stores).  The kernel has left
    // (the depths passed, part | P << 8, the slot's address) in the four words of the counter slot, which a replaying
    // launch has no other use for: nothing of this stays in a register across the shadow rays.
    [[maybe_unused]] volatile unsigned *const splitWord = (volatile unsigned *)sc.park - 4;
    // (part | P << 8 is fetched once per depth: a word of LDS read inside the light loop would wait for the light's scalar loads too)
    [[maybe_unused]] auto splitState = [&]() -> unsigned { return (unsigned)__builtin_amdgcn_readfirstlane((int)splitWord[1]); };
    [[maybe_unused]] auto splitOwns = [&](unsigned pw, int depth_, int li_) -> bool {          // wave-uniform
        const unsigned P_ = pw >> 8, u = (unsigned)depth_ * (unsigned)(f.nLt + 1) + (unsigned)li_;
        const unsigned q = P_ == 3u ? (u * 43691u) >> 17 : u >> (P_ >> 1);       // u / P for P = 1 .. 4, u < 2^15
        return u - q * P_ == (pw & 0xffu);
    };
    // column c of unit u (u < 0: of depth -1 - u's record, or -33: the sky term's) in the slot, this lane's entry
    [[maybe_unused]] auto splitSlot = [&]() -> unsigned long long {
        return ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)splitWord[3]) << 32) |
               (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)splitWord[2]);
    };
    [[maybe_unused]] auto splitColumn = [&](int u, int c) -> float * {
        const unsigned long long at = splitSlot();
        const unsigned units = rt_split_units(f.p.maxRayDepth, f.nLt);
        const unsigned col = u >= 0 ? (unsigned)u * 4u : u == -33 ? (units + (unsigned)f.p.maxRayDepth) * 4u : (units + (unsigned)(-1 - u)) * 4u;
        return (float *)at + 64u + (col + (unsigned)c) * 64u + (threadIdx.x & 63);
    };
    int gxI, gyI;
    size_t outIdx;
    const bool inWindow0 = pixel(gxI, gyI, outIdx);
    const bool inImage0 = inWindow0 && gxI < f.p.width && gyI < f.p.height;
    bool alive = inImage0;
    const bool inImage = inImage0;
    const unsigned gx = (unsigned)gxI, gy = (unsigned)gyI;

    const float nz = inImage ? sample_noise(f, dsc.noise, gx, gy) : 0.0f;
    const float jx = nz * 2.0f - 1.0f, jy = 0.0f * 2.0f - 1.0f;
    Ray ray;
    {   // generateCameraRay (:198-217)
        float ux = (((float)gxI + 0.5f) + jx) / (float)f.p.width;
        float uy = (((float)gyI + 0.5f) + jy) / (float)f.p.height;
        ux = ux * 2.0f - 1.0f;
        uy = uy * 2.0f - 1.0f;
        ux *= f.sx;
        uy *= f.sy;
        v3 cd = V3(f.p.camDir[0], f.p.camDir[1], f.p.camDir[2]);
        v3 cr = V3(f.p.camRight[0], f.p.camRight[1], f.p.camRight[2]);
        v3 cu = V3(f.p.camUp[0], f.p.camUp[1], f.p.camUp[2]);
        ray.o = V3(f.p.camPos[0], f.p.camPos[1], f.p.camPos[2]);
        ray.d = normalize((cd + cr * ux) + cu * uy);
    }
    // The path state a bounce only touches at its ends -- finalColor, throughput, the last hit's P and N -- LIVES in the parking
    // area (SoA, one column per thread; read-modify-write where it changes) instead of travelling between registers and LDS: it
    // is not live across the closest-hit traversal and the loop's back edge, which is where the compiler spilled (6 scratch
    // stores per bounce at the loop header: two thirds of C2's scratch traffic).  Measured, bit-identical: scratch 96 -> 0 B/lane
    // in LIGHT (C2 0.360 -> 0.353 ms), 156 -> 60 in HEAVY1 (C4 unchanged), 164 -> 68 in HEAVY (C5 25.5 -> 26.0 ms: +2 % for 2.4x
    // less scratch traffic, which the paired subsurface probes it makes room for win back: 25.4 ms); PCSS profiles, with the
    // subsurface probes in pairs: C3 3.44 -> 3.39 ms, scratch 156 -> 68 B/lane (with single probes it was 3.73).
    v3 P = V3(0.0f, 0.0f, 0.0f), N = V3(0.0f, 0.0f, 0.0f);
    if constexpr (FIRST < 2) {         // (a replaying tile's columns are filled already, record included: pk_replay_park)
        float *pk_ = sc.park + threadIdx.x;
        pk_[0 * BT] = 0.0f; pk_[1 * BT] = 0.0f; pk_[2 * BT] = 0.0f;            // finalColor
        pk_[3 * BT] = 1.0f; pk_[4 * BT] = 1.0f; pk_[5 * BT] = 1.0f;            // throughput
        pk_[9 * BT] = 0.0f; pk_[10 * BT] = 0.0f; pk_[11 * BT] = 0.0f;          // P, N of the last hit: undefined locals read as zero (A.3)
        pk_[12 * BT] = 0.0f; pk_[13 * BT] = 0.0f; pk_[14 * BT] = 0.0f;
    }

    // origin box of the current bounce rays: the camera position for depth 0 (uniform)
    Box3 rayBox;
    rayBox.lox = rayBox.hix = f.p.camPos[0];
    rayBox.loy = rayBox.hiy = f.p.camPos[1];
    rayBox.loz = rayBox.hiz = f.p.camPos[2];
    bool rayBoxFinite = box_finite(rayBox);

    // FIRST == 1, the two halves of this lane's record.  (t, hit) go out right behind the closest-hit traversal: held until the
    // colour is known they would stay live across the whole lighting section, in kernels that have no register to spare ...
    [[maybe_unused]] auto firstRecordHit = [&](float tHit_, int hit_) {
        const long long at = firstIndex();
        if (at >= 0) {
            const pk_u2 rec = {__float_as_uint(tHit_), (unsigned)hit_};
#if RT_FIRST_HIT_NT
            __builtin_nontemporal_store(rec, (pk_u2 *)records() + at);
#else
            ((pk_u2 *)records())[at] = rec;
#endif
        }
    };
    // ... the colour when depth 0 has ended for this wave: after its lighting, or with every lane a miss or outside the image
    [[maybe_unused]] auto firstRecordColour = [&]() {
        asm volatile("" ::: "memory");
        const float *pk_ = sc.park + threadIdx.x;
        const long long at = firstIndex();
        if (at >= 0) {
            float *col = (float *)(records() + rt_first_hit_colours_offset(f.p.regionW, f.p.regionH)) + 3 * at;
#pragma unroll
            for (int k = 0; k < 3; k++) {
#if RT_FIRST_HIT_NT
                __builtin_nontemporal_store(pk_[k * BT], col + k);
#else
                col[k] = pk_[k * BT];
#endif
            }
        }
    };

    // PREFIX (DESIGN.md section 34; the record and the flag's encoding are rt_firsthit.h's).  FIRST == 1: behind the lighting of
    // every depth 1 .. RT_PREFIX_CAP that the tile reaches untainted, each window lane overwrites its prefix record with the
    // parked state as it stands there, and the taint word's low byte keeps that depth (bit 8 is the taint itself).
    [[maybe_unused]] auto prefixRecord = [&](int depth_, bool alive_, int idx_) {
        asm volatile("" ::: "memory");
        const float *pk_ = sc.park + threadIdx.x;
        const long long at = firstIndex();
        if (at >= 0) {
            const float *tn = pk_ + (alive_ ? 3 : 12) * BT;          // throughput, or N of the last hit where the path has ended
            const pk_u2 w01 = {alive_ ? (unsigned)idx_ : 0xffffffffu, __float_as_uint(pk_[0 * BT])};
            const pk_f4 a = {pk_[10 * BT], pk_[11 * BT], tn[0 * BT], tn[1 * BT]};
            const pk_f4 b = {tn[2 * BT], alive_ ? pk_[6 * BT] : 0.0f, alive_ ? pk_[7 * BT] : 0.0f, alive_ ? pk_[8 * BT] : 0.0f};
            float *col = (float *)(records() + rt_first_hit_colours_offset(f.p.regionW, f.p.regionH)) + 3 * at;
            pk_f4 *fin = (pk_f4 *)(records() + rt_first_hit_finals_offset(f.p.regionW, f.p.regionH)) + 2 * at;
            __builtin_nontemporal_store(w01, (pk_u2 *)records() + at);
            __builtin_nontemporal_store(pk_[1 * BT], col + 0);
            __builtin_nontemporal_store(pk_[2 * BT], col + 1);
            __builtin_nontemporal_store(pk_[9 * BT], col + 2);
            __builtin_nontemporal_store(a, fin);
            __builtin_nontemporal_store(b, fin + 1);
        }
        *taintWord = (unsigned)depth_;
    };
    // FIRST == 2, a tile with K >= 1 (its parking column, where pk_replay_park has left the flag's depth: the flag is fetched
    // from memory once per tile, and nothing stays live across the scene set-up): the PROLOGUE below stands for the bounces 0 .. K.
    // The lane's prefix record -- finalColor, P, throughput and direction (alive) or N (ended) -- is parked already; the
    // prologue sets the hit of depth K up by the expressions
    // of the loop's hit set-up (P is the record's, N and V follow from it), runs that depth's roulette and next direction,
    // and the loop starts at depth K + 1: its body is, to the letter, what a K = 0 tile needs, and carries nothing for this.
    int depth0 = 0;
    if constexpr (FIRST >= 2) {
        float *pk_ = sc.park + threadIdx.x;
        const int k = __builtin_amdgcn_readfirstlane(__float_as_int(pk_[PK_PARK_REC_K * BT]));
        if (k > 0) {
            const int idx = __float_as_int(pk_[PK_PARK_REC_HIT * BT]);
            alive = idx >= 0;
            if (alive) {
                ray.d = V3(pk_[6 * BT], pk_[7 * BT], pk_[8 * BT]);
                P = V3(pk_[9 * BT], pk_[10 * BT], pk_[11 * BT]);
            }
            depth0 = f.p.maxRayDepth;          // nothing left to trace, unless ...
            if (wave_any(alive) && k + 1 < f.p.maxRayDepth) {
                const int ii = alive ? idx : 0;
                const float4 hb = pk_bounds(sc, ii, 0), h2 = pk_lane_hot(sc, ii, 2), h3 = pk_lane_hot(sc, ii, 3);
                const float4 m0 = pk_lane_mat(sc, ii, 0), m1 = pk_lane_mat(sc, ii, 1);
                const v3 Ns = normalize(P - V3(h2));
                N = (__float_as_int(hb.w) == 0) ? Ns : V3(h3);
                const v3 V = normalize(-ray.d);
                pk_[6 * BT] = ray.d.x; pk_[7 * BT] = ray.d.y; pk_[8 * BT] = ray.d.z;
                if (alive) { pk_[12 * BT] = N.x; pk_[13 * BT] = N.y; pk_[14 * BT] = N.z; }
                pk_[15 * BT] = V.x; pk_[16 * BT] = V.y; pk_[17 * BT] = V.z;
                pk_[18 * BT] = m0.x; pk_[19 * BT] = m0.y; pk_[20 * BT] = m0.z;
                pk_[22 * BT] = m1.x;
                {
                    const int depth = k;
#include "rt_packet_bounce.inc"
                }
                rayBox = wave_box(ray.o, alive);
                rayBoxFinite = box_finite(rayBox);
                depth0 = k + 1;
            } else if (wave_any(alive)) {       // (the last depth: its hit only has to leave N behind)
                const int ii = alive ? idx : 0;
                const float4 hb = pk_bounds(sc, ii, 0), h2 = pk_lane_hot(sc, ii, 2), h3 = pk_lane_hot(sc, ii, 3);
                const v3 Ns = normalize(P - V3(h2));
                N = (__float_as_int(hb.w) == 0) ? Ns : V3(h3);
                if (alive) { pk_[12 * BT] = N.x; pk_[13 * BT] = N.y; pk_[14 * BT] = N.z; }
            }
        }
    }

    for (int depth = depth0; depth < f.p.maxRayDepth; ++depth) {
        if (!wave_any(alive)) {
            if constexpr (FIRST == 1) { if (depth == 0) { firstRecordHit(maxDist, -1); firstRecordColour(); } }
            break;
        }
        bool replay = false;            // this bounce comes from the record: wave-uniform, and false wherever FIRST < 2
        if constexpr (FIRST >= 2) replay = depth == 0;
        float t;
        int idx;
        unsigned long long tHit = 0ull;
        [[maybe_unused]] bool skyMiss = false;          // (FIRST == 3: this lane's miss of a split tile adds the sky)
        [[maybe_unused]] unsigned pw = 0x100u;          // (FIRST == 3: part | P << 8 of this job)
        if constexpr (FIRST == 3) pw = splitState();
        if (replay) {
            const float *pk_ = sc.park + threadIdx.x;          // (t, hit) as pk_replay_park left them; finalColor after depth 0 stands in its columns
            const int hitRec = __float_as_int(pk_[PK_PARK_REC_HIT * BT]);
            idx = (hitRec >= 0 && hitRec < nObj) ? hitRec : -1;          // (a record never holds anything else; no gather may leave the scene)
            t = pk_[PK_PARK_REC_T * BT];
        } else {
        const unsigned long long tTrace = pk_clock<COUNT>();
        idx = pk_trace_closest<COUNT>(sc, nObj, ray, alive, rayBox, rayBoxFinite, maxDist, t, rays);
        tHit = pk_clock<COUNT>();
        pk_stat<COUNT>(sc, 12, tHit - tTrace);
        const bool missed = alive && idx < 0;
        if (wave_any(missed && f.p.useSkybox && dsc.sky != nullptr)) {
            if (missed && f.p.useSkybox && dsc.sky) {
                float *pk_ = sc.park + threadIdx.x;
                const v3 fc = V3(pk_[0 * BT], pk_[1 * BT], pk_[2 * BT]), thr = V3(pk_[3 * BT], pk_[4 * BT], pk_[5 * BT]);
                if constexpr (FIRST == 3) {
                    // (a lane misses once, and nothing is added for it afterwards: a split tile has one sky term per lane)
                    const v3 term = thr * sample_cube(dsc.sky, f.skySize, ray.d);
                    if ((pw >> 8) > 1u) {
                        skyMiss = true;
                        if ((pw & 0xffu) == 0u) { *splitColumn(-33, 0) = term.x; *splitColumn(-33, 1) = term.y; *splitColumn(-33, 2) = term.z; }
                    } else {
                        const v3 nf = fc + term;
                        pk_[0 * BT] = nf.x; pk_[1 * BT] = nf.y; pk_[2 * BT] = nf.z;
                    }
                } else {
                const v3 nf = fc + thr * sample_cube(dsc.sky, f.skySize, ray.d);
                pk_[0 * BT] = nf.x; pk_[1 * BT] = nf.y; pk_[2 * BT] = nf.z;
                }
            }
        }
        }
        alive = alive && idx >= 0;          // a miss ends the path (:533)
        if constexpr (FIRST == 3) {
            if (!replay) {
                *splitWord = *splitWord | (1u << (depth & 31));          // (every lane the same word: this depth's lighting is passed)
                if ((pw >> 8) > 1u && (pw & 0xffu) == 0u) {              // part 0: what the sums need of this depth
                    asm volatile("" ::: "memory");
                    const float *pk_ = sc.park + threadIdx.x;
                    *splitColumn(-1 - depth, 0) = pk_[3 * BT]; *splitColumn(-1 - depth, 1) = pk_[4 * BT]; *splitColumn(-1 - depth, 2) = pk_[5 * BT];
                    *splitColumn(-1 - depth, 3) = __uint_as_float((alive ? 1u : 0u) | (skyMiss ? 2u : 0u));
                }
            }
        }
        if constexpr (FIRST == 1) { if (depth == 0) firstRecordHit(t, alive ? idx : -1); }
        if (!wave_any(alive)) {
            if constexpr (FIRST == 1) { if (depth == 0) firstRecordColour(); }
            break;
        }

        // Only the fields computePBR reads stay live across the light loop; the bounce / SSS
        // fields are re-read from LDS (per-lane gather by hit index) where they are used.
        v3 albedo; float metallic, roughness;
        const int ii = alive ? idx : 0;
        {
            if constexpr (PROFILE::hitBatch) {
            // the hit object's records by per-lane gathers, ALL requested before the first is used: the type-dependent second
            // load (sphere centre or plane normal) used to wait for the first, two memory round trips per bounce
            const float4 hb = pk_bounds(sc, ii, 0), h2 = pk_lane_hot(sc, ii, 2), h3 = pk_lane_hot(sc, ii, 3);
            const float4 m0 = pk_lane_mat(sc, ii, 0), m1 = pk_lane_mat(sc, ii, 1);
            // (P, N are this bounce's temporaries, written to the parking area for the lanes that hit)
            P = ray.o + ray.d * t;
            const v3 Ns = normalize(P - V3(h2));
            N = (__float_as_int(hb.w) == 0) ? Ns : V3(h3);
            albedo = V3(m0); metallic = m0.w; roughness = m1.x;
            } else {
            if (__float_as_int(pk_bounds(sc, ii, 0).w) == 0) N = normalize((ray.o + ray.d * t) - V3(pk_lane_hot(sc, ii, 2)));
            else N = V3(pk_lane_hot(sc, ii, 3));
            P = ray.o + ray.d * t;
            const float4 m0 = pk_lane_mat(sc, ii, 0), m1 = pk_lane_mat(sc, ii, 1);
            albedo = V3(m0); metallic = m0.w; roughness = m1.x;
            }
        }
        v3 V = normalize(-ray.d);
        const v3 shadowOrigin = P + N * 0.001f;
        // one origin box per bounce serves every shadow / SSS ray leaving these shading points (a replayed bounce has none)
        Box3 shBox = rayBox;
        if (!replay) shBox = wave_box(shadowOrigin, alive);
        const bool shBoxFinite = box_finite(shBox);

        {   // the ray's direction waits in LDS for the next-direction step; the hit's P and N replace the last hit's for the lanes that hit
            float *pk_ = sc.park + threadIdx.x;
            pk_[6 * BT] = ray.d.x; pk_[7 * BT] = ray.d.y; pk_[8 * BT] = ray.d.z;
            if (alive) {
                pk_[9 * BT] = P.x; pk_[10 * BT] = P.y; pk_[11 * BT] = P.z;
                pk_[12 * BT] = N.x; pk_[13 * BT] = N.y; pk_[14 * BT] = N.z;
            }
            // ... and the rest of the shading point: constant over the light loop, needed only before (P, N: light vector, lit
            // test) and after (N, V, material: computePBR) a light's shadow rays -- not while they are traced
            pk_[15 * BT] = V.x; pk_[16 * BT] = V.y; pk_[17 * BT] = V.z;
            pk_[18 * BT] = albedo.x; pk_[19 * BT] = albedo.y; pk_[20 * BT] = albedo.z;
            pk_[21 * BT] = metallic; pk_[22 * BT] = roughness;
        }
        unsigned long long tAfter = 0ull;
        if (!replay) {          // (a replayed bounce's direct lighting is in the recorded finalColor)
        // ---- computeLighting (:457-507), light loop wave-uniform
        v3 Lo = V3(0.0f, 0.0f, 0.0f);
        const unsigned long long tLights = pk_clock<COUNT>();
        pk_stat<COUNT>(sc, 29, tLights - tHit);                                  // [29] hit shading set-up (normal, material, origin box, parking)
        for (int li = 0; li < f.nLt; li++) {
            if constexpr (FIRST == 3) { if (!splitOwns(pw, depth, li)) continue; }          // (a whole tile owns every unit)
            const int lb4 = sc.lgtF4Base + li * RT_LGT_F4;
            const float4 l0 = uni_load4(sc, lb4), l1 = uni_load4(sc, lb4 + 1), l2 = uni_load4(sc, lb4 + 2), l3 = uni_load4(sc, lb4 + 3);
            const int ltype = __builtin_amdgcn_readfirstlane(__float_as_int(l0.w));
            v3 Pl, Nl0;             // this light's view of the shading point, re-read from the parking area
            {
                asm volatile("" ::: "memory");
                const float *pk_ = sc.park + threadIdx.x;
                Pl = V3(pk_[9 * BT], pk_[10 * BT], pk_[11 * BT]);
                Nl0 = V3(pk_[12 * BT], pk_[13 * BT], pk_[14 * BT]);
            }
            v3 lightDir = V3(0.0f, 0.0f, 0.0f);
            float attenuation = 1.0f, lightDistance = 0.0f;
            if (ltype == 0) {
                lightDir = V3(l0) - Pl;
                lightDistance = length(lightDir);
                attenuation = rtf::rcp(1.0f + 0.1f * lightDistance + 0.01f * lightDistance * lightDistance);
                lightDir = normalize(lightDir);
            } else if (ltype == 1) {
                lightDir = V3(l1);
                lightDistance = 1e6f;
            } else if (ltype == 2) {
                lightDir = V3(l0) - Pl;
                float q = dot(lightDir, lightDir);
                lightDistance = length(lightDir);
                lightDir = normalize(lightDir);
                attenuation = rtf::rcp(fabsf(q));
                float lc = fmaxf(dot(lightDir, V3(l1)), 0.0f);
                attenuation *= lc;
            }
            const int shadowType = __builtin_amdgcn_readfirstlane(__float_as_int(l3.x));
            const int pcfSamples = __builtin_amdgcn_readfirstlane(__float_as_int(l3.y));
            float shadowFactor = 1.0f;
            if (shadowType == 1 || shadowType == 2) {
                float limit = (ltype == 1) ? maxDist : fminf(maxDist, lightDistance);
                if (ltype != 1 && !(lightDistance == lightDistance)) limit = -1.0f;
                const float filterSize = l2.w;
                // Which lanes' shadow term can reach the image.  computePBR ends in `... * radiance * NdotL` with
                // NdotL = max(dot(N, L), 0) (:251-252) and computeLighting multiplies that by the shadow factor
                // (:500): where NdotL is 0 the product is +-0 (or NaN, if the BRDF blew up) for EVERY finite shadow
                // value, so those lanes need no shadow rays.  The factor is finite whenever pcfSamples >= 1 (a PCF of
                // zero samples is 0/0, :396); the instrumented build traces everything so that its ray count stays
                // the reference's.
                bool lit = alive;
                if (COUNT != 1 && pcfSamples >= 1) {
                    // ... and the same holds where the light's radiance (color * attenuation) * intensity (:493) is +-0
                    // or NaN in all three channels (an area light facing away from the point, :487-489; a black light)
                    const v3 rad = (V3(l2) * attenuation) * l1.w;
                    const bool shines = ((rad.x != 0.0f) & (rad.x == rad.x)) | ((rad.y != 0.0f) & (rad.y == rad.y)) |
                                        ((rad.z != 0.0f) & (rad.z == rad.z));
                    lit = alive && shines && (fmaxf(dot(Nl0, normalize(lightDir)), 0.0f) > 0.0f);
                }
                bool needPcf = lit;
                if (shadowType == 2) {          // pcssShadow (:400-440): 16 blocker rays, then PCF if any
                    const float searchSize = l3.z;
                    bool anyBlocker = false;
                    const unsigned long long tBlk = pk_clock<COUNT>();
                    // the 16 blocker rays only feed an OR (:409-427): a lane that has found one blocker needs no more
                    // (the instrumented build keeps tracing them all for the reference's ray count)
                    // few-object scenes: each lane's candidates from the light's BLOCKER table (rt_shadowtab.inc), one gather for
                    // all 16 rays; lights without one (fan wider than the tables' bound, no table at all) keep the packet path
                    bool hasBlockerTab = false;
                    if constexpr (PROFILE::blockerTab) hasBlockerTab = sc.stab && __builtin_amdgcn_readfirstlane(__float_as_int(st_hdr4(sc, li, 6).x)) != 0;
                    if (PROFILE::blockerTab && hasBlockerTab) {
                        constexpr int NB = RT_PK_BLOCKER_GROUP;
                        constexpr int BW = PROFILE::tabWords > 0 ? PROFILE::tabWords : 1;
                        unsigned bm[BW];
                        st_lane_mask<BW, true>(sc, li, nObj, shadowOrigin, V3(l0), lightDir, lightDistance, dot(Nl0, Nl0), lit, bm);
                        for (int s = 0; s < 16; s += NB) {
                            const bool search = (COUNT == 1) ? lit : (lit && !anyBlocker);
                            if (!wave_any(search)) break;
                            v3 bd[NB];
#pragma unroll
                            for (int k = 0; k < NB; k++) {
                                const float rr = pk_halton(sc, 1, s + k, 3) * 2.0f - 1.0f;
                                bd[k] = normalize((lightDir + splat(rr * searchSize)) + splat(rr * searchSize));
                            }
                            anyBlocker |= pk_trace_any_group_masked<COUNT, NB, BW>(sc, shadowOrigin, bd, search, bm, maxDist, limit, rays);
                        }
                    } else
                    if constexpr (PROFILE::blockerPairs) {
                    constexpr int NB = RT_PK_BLOCKER_GROUP;          // blocker rays per traversal (pk_trace_any_group)
                    for (int s = 0; s < 16; s += NB) {
                        const bool search = (COUNT == 1) ? lit : (lit && !anyBlocker);
                        if (!wave_any(search)) break;
                        v3 bd[NB];
#pragma unroll
                        for (int k = 0; k < NB; k++) {
                            const float rr = pk_halton(sc, 1, s + k, 3) * 2.0f - 1.0f;
                            bd[k] = normalize((lightDir + splat(rr * searchSize)) + splat(rr * searchSize));
                        }
                        anyBlocker |= pk_trace_any_group<COUNT, NB>(sc, nObj, shadowOrigin, bd, search, shBox, shBoxFinite, maxDist, limit, rays);
                    }
                    } else {
                    for (int s = 0; s < 16; s++) {
                        const bool search = (COUNT == 1) ? lit : (lit && !anyBlocker);
                        if (!wave_any(search)) break;
                        float rr = pk_halton(sc, 1, s, 3) * 2.0f - 1.0f;
                        v3 sd = (lightDir + splat(rr * searchSize)) + splat(rr * searchSize);
                        Ray sr; sr.o = shadowOrigin; sr.d = normalize(sd);
                        anyBlocker |= pk_trace_any<COUNT>(sc, nObj, sr, search, shBox, shBoxFinite, maxDist, limit, rays);
                    }
                    }
                    needPcf = lit && anyBlocker;
                    pk_stat<COUNT>(sc, 28, pk_clock<COUNT>() - tBlk);            // [28] PCSS blocker search
                }
                if (wave_any(needPcf)) {        // pcfShadow (:342-397)
                    float shadow = pk_pcf_shadow<COUNT, GROUPN, PROFILE::cacheChunks, PROFILE::reach, PROFILE::tabWords>(sc, nObj, shadowOrigin, needPcf, shBox, shBoxFinite,
                                                        ltype, pcfSamples, filterSize, lightDir, limit, nz, maxDist, rays,
                                                        (ltype == 1 && sc.pcfTabF4 >= 0) ? sc.pcfTabF4 + li * (RT_PCF_TAB_N * 2) : -1,
                                                        V3(l0), lightDistance, li, dot(Nl0, Nl0));
                    if (needPcf) shadowFactor = shadow;
                }
            } else if (shadowType != 0) {
                shadowFactor = 0.0f;            // calculateShadow's fall-through (:445)
            }
            v3 Nl, Vl;
            Mat ml;   // view for compute_pbr (unused fields are never read there)
            {
                asm volatile("" ::: "memory");      // keep these reads AFTER the shadow rays: that is the whole point
                const float *pk_ = sc.park + threadIdx.x;
                Nl = V3(pk_[12 * BT], pk_[13 * BT], pk_[14 * BT]);
                Vl = V3(pk_[15 * BT], pk_[16 * BT], pk_[17 * BT]);
                ml.albedo = V3(pk_[18 * BT], pk_[19 * BT], pk_[20 * BT]);
                ml.metallic = pk_[21 * BT]; ml.roughness = pk_[22 * BT];
            }
            const v3 L = normalize(lightDir);
            const v3 H = normalize(Vl + L);
            v3 radiance;
            if constexpr (PROFILE::reloadLight) {
            // the light's colour / intensity are fetched AGAIN here (the index goes through an opaque asm so that the compiler
            // cannot merge the two loads): 8 SGPRs less to carry across the shadow rays, whose loops otherwise reload spilled
            // scalars lane by lane (v_readlane) -- tools/isa_loops.py counts them per loop
            int lb4r = lb4;
            asm volatile("" : "+s"(lb4r));
            const float4 l1r = uni_load4(sc, lb4r + 1), l2r = uni_load4(sc, lb4r + 2);
            radiance = (V3(l2r) * attenuation) * l1r.w;
            } else {
            radiance = (V3(l2) * attenuation) * l1.w;
            }
            if constexpr (FIRST == 3) {
                const v3 term = compute_pbr<PROFILE::fastPbr>(ml, Nl, Vl, L, H, radiance, alive) * shadowFactor;
                if ((pw >> 8) > 1u) {
                    const int u = depth * (f.nLt + 1) + li;
                    *splitColumn(u, 0) = term.x; *splitColumn(u, 1) = term.y; *splitColumn(u, 2) = term.z;
                } else {
                    Lo = Lo + term;
                }
            } else {
            Lo = Lo + compute_pbr<PROFILE::fastPbr>(ml, Nl, Vl, L, H, radiance, alive) * shadowFactor;
            }
        }
        const unsigned long long tSss = pk_clock<COUNT>();
        pk_stat<COUNT>(sc, 26, tSss - tLights);                                  // [26] the whole light loop
        // ---- computeSubsurfaceScattering (:316-339), entered if any lane needs it
        const float4 m2 = pk_lane_mat(sc, ii, 2);          // (subsurfaceColor, subsurfaceScatter)
        const bool needSss = alive && m2.w > 0.0f;
        bool enterSss = wave_any(needSss);
        if constexpr (FIRST == 3) {          // the subsurface section is the depth's unit nLt; its owner in a split tile also keeps which lanes it is for
            const bool owns = splitOwns(pw, depth, f.nLt);
            enterSss = enterSss && owns;
            if (owns && (pw >> 8) > 1u) *splitColumn(depth * (f.nLt + 1) + f.nLt, 3) = __uint_as_float(needSss ? 1u : 0u);
        }
        if (enterSss) {
            const float scatterDistance = pk_lane_mat(sc, ii, 3).x;
            v3 sss = V3(0.0f, 0.0f, 0.0f);
            if constexpr (PROFILE::sssGroup > 1) {       // the four probes PROFILE::sssGroup per traversal
                constexpr int NS = PROFILE::sssGroup;
                for (int s0 = 0; s0 < 4; s0 += NS) {
                    v3 Ns;
                    {
                        asm volatile("" ::: "memory");
                        const float *pkn_ = sc.park + threadIdx.x;
                        Ns = V3(pkn_[12 * BT], pkn_[13 * BT], pkn_[14 * BT]);
                    }
                    v3 pd[NS];
#pragma unroll
                    for (int s = 0; s < NS; s++) pd[s] = hemisphere_dir(V3(f.sssHemi[s0 + s][0], f.sssHemi[s0 + s][1], f.sssHemi[s0 + s][2]), Ns);
                    int sid[NS];
                    float tsd[NS];
                    pk_trace_closest_group<COUNT, NS>(sc, nObj, shadowOrigin, pd, needSss, shBox, shBoxFinite, maxDist, sid, tsd, rays);
#pragma unroll
                    for (int s = 0; s < NS; s++) {
                        if (needSss && sid[s] >= 0) {
                            float att = det_expf(-tsd[s] / scatterDistance);
                            sss = sss + V3(pk_lane_mat(sc, sid[s], 0)) * att;
                        }
                    }
                }
            } else
            for (int s = 0; s < 4; s++) {
                Ray r;
                r.o = shadowOrigin;
                v3 Ns;
                {      // the normal stays parked around the traversal
                    asm volatile("" ::: "memory");
                    const float *pkn_ = sc.park + threadIdx.x;
                    Ns = V3(pkn_[12 * BT], pkn_[13 * BT], pkn_[14 * BT]);
                }
                r.d = hemisphere_dir(V3(f.sssHemi[s][0], f.sssHemi[s][1], f.sssHemi[s][2]), Ns);
                float ts;
                int si = pk_trace_closest<COUNT>(sc, nObj, r, needSss, shBox, shBoxFinite, maxDist, ts, rays);
                if (needSss && si >= 0) {
                    float att = det_expf(-ts / scatterDistance);
                    sss = sss + V3(pk_lane_mat(sc, si, 0)) * att;
                }
            }
            if constexpr (FIRST == 3) {
                const v3 term = ((sss * V3(m2)) * m2.w) / 4.0f;
                if ((pw >> 8) > 1u) {
                    const int u = depth * (f.nLt + 1) + f.nLt;
                    if (needSss) { *splitColumn(u, 0) = term.x; *splitColumn(u, 1) = term.y; *splitColumn(u, 2) = term.z; }
                } else if (needSss) {
                    Lo = Lo + term;
                }
            } else {
            if (needSss) Lo = Lo + ((sss * V3(m2)) * m2.w) / 4.0f;
            }
        }
        tAfter = pk_clock<COUNT>();
        pk_stat<COUNT>(sc, 27, tAfter - tSss);                                 // [27] subsurface section
        bool addLo = alive;
        if constexpr (FIRST == 3) addLo = alive && (pw >> 8) == 1u;          // (a split tile's sums are made at its end)
        if (addLo) {        // finalColor += throughput * Lo, in place
            asm volatile("" ::: "memory");
            float *pk_ = sc.park + threadIdx.x;
            const v3 fc = V3(pk_[0 * BT], pk_[1 * BT], pk_[2 * BT]), thr = V3(pk_[3 * BT], pk_[4 * BT], pk_[5 * BT]);
            const v3 nf = fc + thr * Lo;
            pk_[0 * BT] = nf.x; pk_[1 * BT] = nf.y; pk_[2 * BT] = nf.z;
        }
        }
        if constexpr (FIRST == 1) {
            if (depth == 0) firstRecordColour();
            else if (depth <= RT_PREFIX_CAP && ((uintptr_t)firstHit & RT_FIRST_HIT_NO_PREFIX) == 0 && __builtin_amdgcn_readfirstlane((int)*taintWord) < 0x100)
                prefixRecord(depth, alive, idx);
        }
        // After the last iteration nothing reads `alive`, `throughput` or the ray again, so its Russian roulette and bounce set-up
        // are dead (SURVEY.md A.1#17: at MAX_RAY_DEPTH = 4 the roulette can never change the output).
        if (depth + 1 >= f.p.maxRayDepth) break;
        {
#include "rt_packet_bounce.inc"
        }
        rayBox = wave_box(ray.o, alive);
        rayBoxFinite = box_finite(rayBox);
        pk_stat<COUNT>(sc, 30, pk_clock<COUNT>() - tAfter);                      // [30] roulette + next direction
    }

    pk_stat<COUNT>(sc, 15, pk_clock<COUNT>() - tWave);
    pk_timers_end<COUNT>(sc);
    int sx_, sy_;
    size_t so_;
    const bool inWindow = pixel(sx_, sy_, so_);
    const bool inImageS = inWindow && sx_ < f.p.width && sy_ < f.p.height;
    const size_t outIdxS = so_;
    v3 finalColor;
    {
        asm volatile("" ::: "memory");
        const float *pk_ = sc.park + threadIdx.x;
        finalColor = V3(pk_[0 * BT], pk_[1 * BT], pk_[2 * BT]);
        P = V3(pk_[9 * BT], pk_[10 * BT], pk_[11 * BT]);
        N = V3(pk_[12 * BT], pk_[13 * BT], pk_[14 * BT]);
    }
    if constexpr (FIRST == 3) {
        const unsigned P_ = splitState() >> 8;
        if (P_ > 1u) {
            // A split tile's job has stored its units (part 0 the depths' records too): an agent-scope release -- L2 is per
            // XCD, and the jobs of a tile run wherever they were dispatched -- behind a wait for every store, then ONE add on the
            // slot's counter.  Every job but the last to arrive ends here; no job ever waits for another.  The last one puts
            // the counter back for the next frame, makes the acquire that its loads below sit behind, and adds up in the
            // source's order: per depth Lo = 0, + each light's term, + the subsurface term where the lane needs it, then
            // finalColor + throughput * Lo where the lane is alive; the sky term where the lane's miss adds it.
            unsigned *const counter = (unsigned *)splitSlot();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            unsigned seen = 0u;
            if ((threadIdx.x & 63) == 0) seen = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            seen = (unsigned)__builtin_amdgcn_readfirstlane((int)seen);
            if (seen != P_ - 1u) return;
            if ((threadIdx.x & 63) == 0) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            const unsigned passed = (unsigned)__builtin_amdgcn_readfirstlane((int)splitWord[0]);
            for (int d = 0; d < f.p.maxRayDepth && d < RT_MAX_DEPTH; d++) {
                if (!((passed >> d) & 1u)) continue;
                const unsigned bits = __float_as_uint(*splitColumn(-1 - d, 3));
                if (bits & 2u) finalColor = finalColor + V3(*splitColumn(-33, 0), *splitColumn(-33, 1), *splitColumn(-33, 2));
                if (bits & 1u) {
                    const v3 thr = V3(*splitColumn(-1 - d, 0), *splitColumn(-1 - d, 1), *splitColumn(-1 - d, 2));
                    v3 Lo = V3(0.0f, 0.0f, 0.0f);
                    const int u0 = d * (f.nLt + 1);
                    for (int li = 0; li < f.nLt; li++) Lo = Lo + V3(*splitColumn(u0 + li, 0), *splitColumn(u0 + li, 1), *splitColumn(u0 + li, 2));
                    if (__float_as_uint(*splitColumn(u0 + f.nLt, 3)) & 1u)
                        Lo = Lo + V3(*splitColumn(u0 + f.nLt, 0), *splitColumn(u0 + f.nLt, 1), *splitColumn(u0 + f.nLt, 2));
                    finalColor = finalColor + thr * Lo;
                }
            }
        }
    }
    if (inWindow) {
        if (inImageS) {
            gColor[outIdxS] = make_float4(finalColor.x, finalColor.y, finalColor.z, 1.0f);
            gPosition[outIdxS] = make_float4(P.x, P.y, P.z, 1.0f);
            gNormal[outIdxS] = make_uint2(f2h_rtz(N.x) | (f2h_rtz(N.y) << 16), f2h_rtz(N.z) | (0x3c00u << 16));
        } else if (!f.imageStores) {   // outside the image: GL discards the imageStore (a whole-image surface has no such pixel)
            gColor[outIdxS] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            gPosition[outIdxS] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            gNormal[outIdxS] = make_uint2(0u, 0u);
        }
    }
    if constexpr (FIRST == 1) {   // every exit of the bounce loop comes through here: the tile's flag, and a settled tile's final records
        asm volatile("" ::: "memory");
        const unsigned taint = (unsigned)__builtin_amdgcn_readfirstlane((int)*taintWord);      // bit 8: tainted; low byte: the depth of the last prefix record
        const bool settled = ((uintptr_t)firstHit & RT_FIRST_HIT_NO_SETTLED) == 0 && taint < 0x100u;
        unsigned char *flags = records() + rt_first_hit_flags_offset(f.p.regionW, f.p.regionH);
        if ((threadIdx.x & 63) == 0) flags[sc.tileY * ((f.p.regionW + 7) / 8) + sc.tileX] = (unsigned char)rt_prefix_flag(settled, (int)(taint & 0xffu));
        const long long at = firstIndex();
        if (settled && at >= 0) {
            pk_f4 *fin = (pk_f4 *)(records() + rt_first_hit_finals_offset(f.p.regionW, f.p.regionH)) + 2 * at;
            const pk_f4 a = {finalColor.x, finalColor.y, finalColor.z, P.x};
            const pk_f4 b = {P.y, P.z, __uint_as_float(f2h_rtz(N.x) | (f2h_rtz(N.y) << 16)), __uint_as_float(f2h_rtz(N.z) | (0x3c00u << 16))};
            __builtin_nontemporal_store(a, fin);
            __builtin_nontemporal_store(b, fin + 1);
        }
    }
}
