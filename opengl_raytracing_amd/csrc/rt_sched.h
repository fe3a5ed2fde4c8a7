// rt_sched.h -- the packet kernel's tile scheduler, held by value in rt_context (rt_context.h).  It keeps the record of every
// stream a launch has been issued on (the stream protocol that renders, queries, shading and the scene / texture setters share)
// and decides the tile order of each frame: begin() before rt_launch_render, end() after it.  Not part of the public ABI.
#pragma once
#include "rt_devbuf.h"
#include "rt_device.h"

struct RtTileScheduler {
    // Every stream a launch has been issued on (the context's own and the callers'): `last` = its most recent
    // launch (recorded on EVERY launch, feedback or not: rt_set_scene orders the scene rewrite behind all of
    // them), `seenGen` = the tile-order adoption it has already ordered itself behind.
    struct StreamRec {
        hipStream_t s = nullptr;
        DevEvent last;
        unsigned seenGen = 0;
        unsigned seenFirst = 0;                // the first-hit recording it has already ordered itself behind (firstGen)
        // predicted tile order of the last frame issued on this stream, and the inputs it was predicted from
        // (predOrder: the order, then 32 class segments of predCls.cap tile ids each; predCounts: two sets of 32 class sizes, used
        // alternately -- a prediction clears the other set)
        DevBuf<unsigned> predOrder, predCounts;
        DevBuf<unsigned char> predCls;
        unsigned long long predKey = 0;
        bool predValid = false;
        int predSet = 0;
        // tile split (below): the scratch slots of this stream's split launches -- frames on different streams never share them --
        // and the two descriptors its launches pass, one per plan buffer, with what each was last written from
        DevBuf<float> splitScratch;
        size_t splitStride = 0;                // rt_split_slot_dwords() of the launches whose counters it holds at zero (0: nobody's;
                                               // under another stride the counters lie in old column data: splitFor zeroes it first)
        size_t splitRefused = 0;               // a scratch of this many floats could not be had on this stream
        DevBuf<RtSplitDesc> splitDesc;
        unsigned descGen[2] = {0, 0};
        const void *descRecords[2] = {nullptr, nullptr};
        const void *descScratch[2] = {nullptr, nullptr};
    };
    // What begin() decided for one launch; end() takes it back.
    struct Plan {
        StreamRec *rec = nullptr;
        int nTiles = 0, tilesX = 0, bt = 0;
        int costClass = 0;                     // what the frame's tile costs are comparable with: 0 = whole frames, 1 = first-hit replays
        int phase = -1;                        // frameCount mod 64 when the frame records into (and sorts) its phase's buffers
        bool sortAfter = false;                // the frame was scheduled: the measured order's bookkeeping runs after it
        int depth = 0, nLt = 0;                // the frame's maxRayDepth and lights, and the resident waves per SIMD of its kernel:
        int waves = 0;                         // what a split plan made behind this frame is made for
        bool sameStream = false;               // the context's previous packet launch was on this stream too
    };

    void init(hipStream_t contextStream);      // + the environment overrides (RT_FB_PERIOD, RT_PRED_MIN_TILES, RT_PHASE_ORDER, RT_DEBUG_PRED_CLASSES, RT_DEBUG_TILE_ORDER, RT_TILE_SPLIT, RT_DEBUG_SPLIT_PARTS)
    void setMode(int variant);                 // rt_set_variant's bits 8 and 9; forgets the geometry

    // ---- stream protocol
    hipError_t record(hipStream_t s, StreamRec **out);                  // the record of stream s (created on first use)
    hipError_t recordLaunch(hipStream_t s);                             // s's last launch is whatever was just enqueued on it
    hipError_t waitForLaunches(hipStream_t t, bool ownToo = false);     // t waits for every recorded stream's last launch (its own record only if asked)
    hipError_t drain();                                                 // the host waits for every stream and every sort

    // ---- one frame.  `packet`: the launch is one the scheduler may order (packet kernel, no ray counter); `inputsGen`
    // changes whenever the scene or a texture does.  begin() fills sc.tileOrder / sc.tileCost.  `costClass`: 1 for a frame that
    // replays its first hit (rt_firsthit.h) -- its tiles cost nothing like a whole frame's, so a change of class restarts the
    // cost feedback exactly as a new window geometry does (costs cleared, orders reset, sorts on the first two frames, phases forgotten).
    hipError_t begin(const RtFrame &f, RtDeviceScene &sc, hipStream_t s, bool packet, unsigned long long inputsGen, Plan *plan, int costClass = 0);
    hipError_t end(const Plan &plan, hipStream_t s);

    // ---- the context's first-hit records: one buffer, written by a recording frame, read by replays on any stream.  A
    // recording frame overwrites it only behind every stream's last launch (beforeFirstHitRecord, ahead of the launch) and
    // records the event (afterFirstHitRecord) that every stream's first replay after it waits for (beforeFirstHitReplay).
    hipError_t beforeFirstHitRecord(hipStream_t s);
    hipError_t afterFirstHitRecord(hipStream_t s, StreamRec *rec);
    hipError_t beforeFirstHitReplay(hipStream_t s, StreamRec *rec);

    // ---- TILE SPLIT (rt_device.h has the device side).  Behind every sort of a replaying frame's costs
    // (cost class 1, measured order) the plan kernel decides, on the context's stream and ahead of the sort's event, which tiles
    // of the new order run as P one-wave jobs: the plan is double-buffered with the order and adopted with it -- the same event,
    // the same seenGen wait.  A new geometry or cost class drops both plans, as it drops the orders.  splitFor(), between
    // begin() and the launch of a REPLAYING frame: the descriptor to launch with, or null -- no plan for the order in use, a
    // phase's or a predicted order, the previous packet launch on another stream (frames in flight on several streams fill each
    // other's tails, and would only pay the split's extra work), no scratch to be had (no error: the frame runs whole).
    hipError_t splitFor(const Plan &plan, const RtDeviceScene &sc, const void *records, hipStream_t s, const RtSplitDesc **out);

    // ---- debug read-outs (rt_debug_tile_costs, rt_debug_predicted_classes, rt_debug_tile_order)
    hipError_t tileCosts(unsigned *out, int cap, int *nTiles, int *tilesX);
    hipError_t predictedClasses(unsigned char *out, int cap, int *nTiles);
    hipError_t tileOrder(unsigned *out, int cap, int *nTiles, int *policy);
    // rt_debug_lpt_sort: rt_launch_lpt_sort on the caller's host arrays, in device buffers of its own on the context's stream;
    // synchronises.  Reads and writes nothing of the scheduler's (failedCall aside).
    hipError_t lptSortOf(unsigned *costs, int nTiles, unsigned *order, unsigned *accum);

    // rt_debug_split_tiles: P per tile (0 = whole) of the plan the last replaying launch ran with; *nTiles = 0 before any
    hipError_t splitTiles(unsigned char *out, int cap, int *nTiles);
    // rt_debug_split_plan: rt_launch_split_plan on the caller's host arrays (order, costs; prevParts may be null), in device
    // buffers of its own on the context's stream; synchronises.  counts = (extra jobs, split tiles).
    hipError_t splitPlanOf(const unsigned *order, const unsigned *costs, int nTiles, unsigned waveSlots, int depth, int nLt, int forceParts,
                           const unsigned char *prevParts, unsigned char *parts, unsigned short *slot, unsigned *extra, unsigned *counts);

    const char *failedCall = "";               // the HIP call behind the last error returned

private:
    hipError_t measuredBegin(RtDeviceScene &sc, hipStream_t s, Plan *plan, bool *newGeometry);
    hipError_t measuredEnd(const Plan &plan);
    hipError_t predictedBegin(const RtFrame &f, RtDeviceScene &sc, hipStream_t s, unsigned long long inputsGen, const Plan &plan);
    hipError_t phaseBegin(const RtFrame &f, RtDeviceScene &sc, Plan *plan);
    hipError_t phaseEnd(const Plan &plan);
    void phaseForget();
    hipError_t noteOrder(const RtDeviceScene &sc, hipStream_t s, int nTiles, const StreamRec *rec);

    hipStream_t own = nullptr;                 // the context's stream: the periodic sort runs on it
    // schedMode 2 (default): tiles run longest-first by their MEASURED cost over the last frames of the same window geometry (the
    // feedback of rounds 1-2); while no measured order exists yet, frames of >= predMinTiles tiles run in the heavy-first order
    // PREDICTED from their own inputs (rt_predict_tiles_kernel, in the frame's own stream, buffers per stream in StreamRec).
    // 1: measured costs only.  0: raster order.
    int schedMode = 2;

    static constexpr int kMaxStreams = 8;
    StreamRec recs[kMaxStreams];
    int nRecs = 0;

    // ---- measured order.  Frames may be issued on several streams (frames in flight overlapping on the device), so the order
    // is double-buffered: a sort writes the buffer no launch is reading, and later launches wait for it.
    DevBuf<unsigned> dTileCost, dTileSnap, dTileOrder[2];
    DevEvent evSort[2];                        // completion of the rt_lpt_sort that wrote dTileOrder[k]
    int fbCur = -1;                            // order buffer new launches read (-1 = raster order)
    int fbNext = 0;                            // order buffer the pending sort is writing
    bool sortPending = false;                  // a sort has been enqueued on the context's own stream, not yet adopted
    unsigned sortAge = 0;                      // fbAge at which it was enqueued
    int fbTiles = 0, fbTilesX = 0, fbBt = 0;   // geometry the current order was measured on (0 = none)
    int fbClass = 0;                           // ... and the cost class of the frames it was measured on (Plan::costClass)
    DevEvent evFirst;                          // completion of the last frame that recorded first hits
    unsigned firstGen = 0;                     // bumped by every such frame
    unsigned fbAge = 0;                        // frames since that geometry was first seen
    unsigned adoptGen = 0;                     // bumped whenever fbCur changes to a freshly sorted buffer
    unsigned fbPeriod = 32;                    // re-sort period in frames (RT_FB_PERIOD overrides, for measurements)

    // ---- tile split
    bool splitOn = true;                       // RT_TILE_SPLIT=0 clears it: no plan is made, every replaying frame is the whole-tile one
    int splitForce = 0;                        // RT_DEBUG_SPLIT_PARTS=2|3|4: every tile the layout takes is split into that many (tests)
    unsigned simds = 0;                        // SIMDs of the device (init): the plan's target is the costs' sum / (simds x waves)
    DevBuf<unsigned> dCostKeep;                // the costs the last sort read
    DevBuf<unsigned char> dSplitParts[2];      // the plan of dTileOrder[k]: P per tile,
    DevBuf<unsigned short> dSplitSlot[2];      // a split tile's scratch slot,
    DevBuf<unsigned> dSplitExtra[2];           // the jobs beyond part 0
    DevBuf<unsigned> dSplitCounts[2];          // and how many (extra jobs, split tiles)
    // Whether the plans of the current feedback epoch split anything, as the device last said: (split tiles, epoch), two words of
    // pinned host memory that every plan kernel writes and nobody waits for.  A launch takes the split kernel only once a plan
    // of ITS epoch has been seen to split a tile -- the kernel that carries the split's code costs the whole tiles a few per
    // cent, and a frame whose plans split nothing must not pay it.  The host may run many frames ahead of the device: those
    // frames run whole; split tiles stay split within an epoch, so a count once seen above zero stays above zero.
    PinnedBuf<unsigned> hSplitSeen;
    unsigned splitEpoch = 1;                   // bumped whenever the feedback restarts (0 is no epoch's)
    bool planValid[2] = {false, false};
    int planDepth[2] = {0, 0}, planNLt[2] = {0, 0};
    unsigned planGen[2] = {0, 0}, planCount = 0;
    hipStream_t lastPacketStream = nullptr;    // the stream of the context's previous packet launch
    bool haveLastPacket = false;
    int dbgSplitK = -2;                        // plan buffer of the last replaying launch (-1: it ran whole, -2: there was none)
    int dbgSplitTiles = 0;

    // ---- predicted order
    int predMinTiles = 49152;                  // frames of at least this many tiles get a predicted order while no measured one exists (RT_PRED_MIN_TILES)
    bool dbgWantCls = false;                   // RT_DEBUG_PRED_CLASSES=1: predictions also store each tile's class
    const unsigned char *dbgPredCls = nullptr; // class buffer of the last predicted launch (rt_debug_predicted_classes)
    int dbgPredTiles = 0;

    // ---- RT_DEBUG_TILE_ORDER=1: begin() ends by copying the order it chose (device to device, on the launch's stream, ahead of
    // the launch) into dDbgOrder -- the sorts rewrite the live buffers behind the launch, phaseEnd the very one the frame read.
    // One buffer per context: the read-out means the last launch's order only if the caller synchronises between frames.
    bool dbgWantOrder = false;
    DevBuf<unsigned> dDbgOrder;
    int dbgOrderTiles = 0;                     // tiles of the last packet launch begin() saw (0 = none since init / setMode)
    int dbgOrderPolicy = 0;                    // who supplied its order: 0 raster (nothing copied), 1 measured, 2 predicted, 3 phase

    // ---- per-phase orders.  Free-running frameCount (the reference with TAA on, ForwardShadingPipeline.cpp:254): frameCount
    // enters the frame through hammersley(depth*64 + frameCount, 64) (:557) -- the bounce sample ALL pixels share -- whose azimuth
    // is periodic in frameCount with period 64 and whose cos^2(theta) = halton2 repeats to within 2^-6.  A frame's tile costs
    // therefore repeat, nearly, every 64 frames, while consecutive frames differ a lot (tools/gpu_phase_costs.py: list-scheduling
    // makespan over the ideal, C2: 1.04 in the frame's own order, 1.06-1.09 in the order of the frame 64 earlier, 1.07-1.17 in the
    // all-phase average order, 1.29-1.34 in raster order).  So once frameCount is seen advancing, every frame's costs go to its
    // PHASE's buffer (frameCount mod 64) and are sorted, beside the following frames on a stream of their own, into that phase's
    // order, which the frame 64 later runs in; phases not seen yet use the all-phase average order as before (the per-phase
    // sorts feed it).
    DevStream phaseStream;
    DevBuf<unsigned> dPhaseCost, dPhaseOrder, dPhaseSnap;   // [64][phaseTiles], [64][phaseTiles], [phaseTiles]
    int phaseTiles = 0;                        // tiles per phase of the current geometry (0 = none)
    DevEvent evPhase[64];                      // completion of the last sort into phase k's order
    unsigned char phaseState[64] = {};         // 0 = no order, 1 = sort issued, 2 = seen complete
    bool phaseOn = true;                       // RT_PHASE_ORDER=0 switches it off (measurements)
    bool haveLastFc = false;
    int lastFc = 0, freeRun = 0;               // consecutive scheduled launches whose frameCount differed from the previous one's
};
