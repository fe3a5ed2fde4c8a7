// rt_sched.cpp -- the tile scheduler of rt_sched.h: the stream records, then the three ordering policies (measured,
// predicted, per-phase), each with its part before and its part after the render launch, then begin() / end() that string
// them together.
#include "rt_sched.h"

#include <stdlib.h>
#include <string.h>

// a failing HIP call: remember its text for the ABI's error string, pass the error on
#define SCHED_TRY(call)                 \
    do {                                \
        hipError_t e_ = (call);         \
        if (e_ != hipSuccess) {         \
            failedCall = #call;         \
            return e_;                  \
        }                               \
    } while (0)
// a failing call of the scheduler's own: it has already set failedCall
#define SCHED_PASS(call)                \
    do {                                \
        hipError_t e_ = (call);         \
        if (e_ != hipSuccess) return e_; \
    } while (0)

void RtTileScheduler::init(hipStream_t contextStream) {
    own = contextStream;
    if (const char *e = getenv("RT_FB_PERIOD")) {
        const int v = atoi(e);
        if (v >= 1 && v <= 1024) fbPeriod = (unsigned)v;
    }
    if (const char *e = getenv("RT_DEBUG_PRED_CLASSES")) dbgWantCls = atoi(e) != 0;
    if (const char *e = getenv("RT_DEBUG_TILE_ORDER")) dbgWantOrder = atoi(e) != 0;
    if (const char *e = getenv("RT_PRED_MIN_TILES")) predMinTiles = atoi(e);
    if (const char *e = getenv("RT_PHASE_ORDER")) phaseOn = atoi(e) != 0;
    if (const char *e = getenv("RT_TILE_SPLIT")) splitOn = atoi(e) != 0;
    if (const char *e = getenv("RT_DEBUG_SPLIT_PARTS")) {
        const int v = atoi(e);
        if (v >= 2 && v <= RT_SPLIT_MAX_PARTS) splitForce = v;
    }
    // the resident wave slots a frame fills are SIMDs x the kernel's waves per SIMD; a CDNA compute unit has four SIMDs
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
        simds = 4u * (unsigned)cus;
    else
        (void)hipGetLastError();
}

void RtTileScheduler::setMode(int variant) {
    // bit 8 (0x100): raster tile order every frame; bit 9 (0x200): the measured-cost feedback order of rounds 1-2 instead of the
    // predicted one (default)
    schedMode = (variant & 0x100) ? 0 : ((variant & 0x200) ? 1 : 2);
    fbTiles = 0;
    dbgOrderTiles = 0;
}

// ---- stream protocol ----------------------------------------------------------------------------------------------------

hipError_t RtTileScheduler::drain() {
    if (own) SCHED_TRY(hipStreamSynchronize(own));
    if (phaseStream) SCHED_TRY(hipStreamSynchronize(phaseStream));
    for (int i = 0; i < nRecs; i++) SCHED_TRY(hipEventSynchronize(recs[i].last));
    for (int k = 0; k < 2; k++)
        if (evSort[k]) SCHED_TRY(hipEventSynchronize(evSort[k]));
    return hipSuccess;
}

// More streams than slots: drain and start over (not a hot path).
hipError_t RtTileScheduler::record(hipStream_t s, StreamRec **out) {
    for (int i = 0; i < nRecs; i++)
        if (recs[i].s == s) { *out = &recs[i]; return hipSuccess; }
    if (nRecs == kMaxStreams) {
        SCHED_PASS(drain());
        nRecs = 0;
    }
    StreamRec *m = &recs[nRecs];
    SCHED_TRY(m->last.create(hipEventDisableTiming));
    nRecs++;
    m->s = s;
    m->predValid = false;
    m->seenGen = 0;                // adoptGen starts at 1 with the first adoption: a new stream always orders itself
    m->seenFirst = 0;              // (firstGen likewise)
    m->splitStride = 0;            // a recycled record's scratch is another stream's: this one zeroes it before its first split
    SCHED_TRY(hipEventRecord(m->last, s));
    *out = m;
    return hipSuccess;
}

hipError_t RtTileScheduler::recordLaunch(hipStream_t s) {
    StreamRec *rec = nullptr;
    SCHED_PASS(record(s, &rec));
    SCHED_TRY(hipEventRecord(rec->last, s));
    return hipSuccess;
}

hipError_t RtTileScheduler::waitForLaunches(hipStream_t t, bool ownToo) {
    for (int i = 0; i < nRecs; i++)
        if (ownToo || recs[i].s != t) SCHED_TRY(hipStreamWaitEvent(t, recs[i].last, 0));
    return hipSuccess;
}

// ---- first-hit records (rt_sched.h) ---------------------------------------------------------------------------------------

hipError_t RtTileScheduler::beforeFirstHitRecord(hipStream_t s) {
    // replays still queued on the other streams read the buffer this frame rewrites; s's own are ahead of it by stream order
    return waitForLaunches(s);
}

hipError_t RtTileScheduler::afterFirstHitRecord(hipStream_t s, StreamRec *rec) {
    SCHED_TRY(evFirst.create(hipEventDisableTiming));
    SCHED_TRY(hipEventRecord(evFirst, s));
    firstGen++;
    rec->seenFirst = firstGen;         // (the recording stream's own replays follow by stream order)
    return hipSuccess;
}

hipError_t RtTileScheduler::beforeFirstHitReplay(hipStream_t s, StreamRec *rec) {
    // the seenGen / adoptGen pattern of measuredBegin: which frame recorded last is context-global, streams are not ordered
    // with each other, so EVERY stream's first replay after a recording waits for it (a no-op once it has completed)
    if (rec->seenFirst != firstGen) {
        SCHED_TRY(hipStreamWaitEvent(s, evFirst, 0));
        rec->seenFirst = firstGen;
    }
    return hipSuccess;
}

// ---- measured order -------------------------------------------------------------------------------------------------------
// Longest-first tile order from the previous frames' measured tile costs (same window geometry, any
// stream).  The first frame of a geometry runs in raster order and only records costs.

hipError_t RtTileScheduler::measuredBegin(RtDeviceScene &sc, hipStream_t s, Plan *plan, bool *newGeometry) {
    const int nTiles = plan->nTiles;
    if (!(dTileCost.holds(nTiles) && dTileSnap.holds(nTiles) && dTileOrder[0].holds(nTiles) && dTileOrder[1].holds(nTiles))) {
        SCHED_PASS(drain());
        fbTiles = 0;
        fbCur = -1;
        sortPending = false;
        planValid[0] = planValid[1] = false;
        splitEpoch++;
        for (DevBuf<unsigned> *b : {&dTileCost, &dTileSnap, &dTileOrder[0], &dTileOrder[1]}) SCHED_TRY(b->release());
        for (DevBuf<unsigned> *b : {&dTileCost, &dTileSnap, &dTileOrder[0], &dTileOrder[1]}) SCHED_TRY(b->grow(nTiles));
        // the split plans live and die with the orders they belong to (a context with the split off never makes one)
        SCHED_TRY(dCostKeep.release());
        for (int k = 0; k < 2; k++) { SCHED_TRY(dSplitParts[k].release()); SCHED_TRY(dSplitSlot[k].release()); }
        if (splitOn) {
            if (!hSplitSeen) {
                SCHED_TRY(hSplitSeen.grow(2));
                hSplitSeen.ptr[0] = hSplitSeen.ptr[1] = 0u;
            }
            SCHED_TRY(dCostKeep.grow(nTiles));
            for (int k = 0; k < 2; k++) {
                SCHED_TRY(dSplitParts[k].grow(nTiles));
                SCHED_TRY(dSplitSlot[k].grow(nTiles));
                SCHED_TRY(dSplitExtra[k].grow(RT_SPLIT_EXTRA_BLOCKS));
                SCHED_TRY(dSplitCounts[k].grow(2));
            }
        }
    }
    *newGeometry = !(fbTiles == nTiles && fbTilesX == plan->tilesX && fbBt == plan->bt && fbClass == plan->costClass);
    if (*newGeometry) {
        // New geometry (or frames of another cost class: first-hit replays after whole frames, or back): nobody may still be using the old costs / orders, and a sort of the old geometry must
        // never be adopted.  Both order buffers restart as the identity permutation (a launch that reads one
        // before its first sort -- it cannot, fbCur is -1 -- would still visit every tile exactly once).
        SCHED_PASS(waitForLaunches(s));
        for (int k = 0; k < 2; k++)
            if (evSort[k]) SCHED_TRY(hipStreamWaitEvent(s, evSort[k], 0));
        SCHED_TRY(hipMemsetAsync(dTileCost, 0, (size_t)nTiles * sizeof(unsigned), s));
        SCHED_TRY(rt_launch_iota(dTileOrder[0], nTiles, s));
        SCHED_TRY(rt_launch_iota(dTileOrder[1], nTiles, s));
        SCHED_TRY(hipEventRecord(plan->rec->last, s));      // later sorts (context stream) order behind the re-initialisation
        fbCur = -1;
        sortPending = false;
        fbAge = 0;
        planValid[0] = planValid[1] = false;          // the feedback restarts: so does the split
        splitEpoch++;
    } else if (sortPending) {
        // The sort runs on the context's own stream, beside the frames; its order is adopted by the first launch
        // issued after it has completed, so no render stream waits for a sort in steady state.
        const hipError_t q = hipEventQuery(evSort[fbNext]);
        (void)hipGetLastError();           // hipErrorNotReady is an answer, not an error to find later
        // Not ready: the host is running ahead of the device.  No order at all yet (second frame of a geometry),
        // or the sort was issued more than one launch per render stream ago (it sits behind a frame that is no
        // longer in flight when this launch reaches the device, so it is all but done): adopt it anyway -- every
        // stream orders itself behind the sort's event on its next launch (seenGen below).
        if (q == hipSuccess || fbCur < 0 || fbAge - sortAge >= 1u + (unsigned)nRecs) {
            fbCur = fbNext;
            sortPending = false;
            adoptGen++;
        }
    }
    // EVERY stream's first launch after an adoption waits for the sort that wrote the adopted buffer (a no-op
    // once it has completed).  Adoption state is context-global, streams are not ordered with each other: without
    // this, a frame on stream B could read an order that only stream A had waited for.
    if (fbCur >= 0 && plan->rec->seenGen != adoptGen) {
        SCHED_TRY(hipStreamWaitEvent(s, evSort[fbCur], 0));
        plan->rec->seenGen = adoptGen;
    }
    sc.tileOrder = fbCur >= 0 ? dTileOrder[fbCur].ptr : nullptr;
    sc.tileCost = dTileCost;
    plan->sortAfter = true;
    return hipSuccess;
}

hipError_t RtTileScheduler::measuredEnd(const Plan &plan) {
    // Re-sort on the first two frames of a geometry, then every fbPeriod-th.  Costs accumulate in between, so
    // the order follows each tile's AVERAGE cost over the period: with a free-running frameCount (which rotates
    // the bounce sample all pixels share) the last frame alone is a poor predictor of the next (C2, measured:
    // 0.63 ms/frame ordering by the last frame every 8th, 0.56 by the 8-frame average, 0.54 by the 32-frame one).
    if ((fbAge < 2 || (fbAge % fbPeriod) == 0) && !sortPending) {
        const int next = fbCur == 0 ? 1 : 0;
        // the buffer about to be rewritten was last read before the previous adoption: every stream's last
        // launch (this one included) is after those reads, and gives the sort this frame's costs
        SCHED_PASS(waitForLaunches(own, true));
        // replaying frames: the split plan of the new order, behind the sort and ahead of its event -- adopted with the order
        // (a frame of more units than any split takes gets no plan at all)
        // Not for frames in flight on several streams, which fill each other's tails, nor while frameCount advances: the order is
        // then the all-phase average, the tiles that are long in one frame are not the ones that are long on average, and the
        // split only added its work (measured: the first free-running period +8.5 %, two frames in flight +2 % with plans made
        // that no launch used).  RT_DEBUG_SPLIT_PARTS plans regardless of frameCount.
        const bool planned = splitOn && plan.costClass == 1 && plan.sameStream && (freeRun == 0 || splitForce) && simds > 0 && plan.waves > 0 && dCostKeep.holds(plan.nTiles) && hSplitSeen &&
                             plan.depth >= 2 && plan.depth <= RT_MAX_DEPTH &&
                             rt_split_units(plan.depth, plan.nLt) <= (unsigned)(RT_SPLIT_UNITS_PER_PART * RT_SPLIT_MAX_PARTS) &&
                             (unsigned)plan.nTiles <= (unsigned)RT_SPLIT_MAX_TILES_PER_SLOT * simds * (unsigned)plan.waves;
        SCHED_TRY(rt_launch_lpt_sort(dTileCost, dTileSnap, dTileOrder[next], plan.nTiles, own, nullptr, planned ? dCostKeep.ptr : nullptr));
        planValid[next] = false;
        if (planned) {
            const int cur = fbCur >= 0 && planValid[fbCur] && planDepth[fbCur] == plan.depth && planNLt[fbCur] == plan.nLt ? fbCur : -1;
            SCHED_TRY(rt_launch_split_plan(dTileOrder[next], dCostKeep, plan.nTiles, simds * (unsigned)plan.waves, plan.depth, plan.nLt, splitForce,
                                           cur >= 0 ? dSplitParts[cur].ptr : nullptr, dSplitParts[next], dSplitSlot[next], dSplitExtra[next],
                                           dSplitCounts[next], splitEpoch, hSplitSeen, own));
            planValid[next] = true;
            planDepth[next] = plan.depth;
            planNLt[next] = plan.nLt;
            planGen[next] = ++planCount;
        }
        SCHED_TRY(evSort[next].create(hipEventDisableTiming));
        SCHED_TRY(hipEventRecord(evSort[next], own));
        fbNext = next;
        sortPending = true;
        sortAge = fbAge;
    }
    fbAge++;
    fbTiles = plan.nTiles;
    fbTilesX = plan.tilesX;
    fbBt = plan.bt;
    fbClass = plan.costClass;
    return hipSuccess;
}

// ---- tile split (rt_sched.h has the rule) ----------------------------------------------------------------------------------

hipError_t RtTileScheduler::splitFor(const Plan &plan, const RtDeviceScene &sc, const void *records, hipStream_t s, const RtSplitDesc **out) {
    *out = nullptr;
    dbgSplitK = -1;
    dbgSplitTiles = plan.nTiles;
    const int k = fbCur;
    if (!(splitOn && plan.sortAfter && plan.costClass == 1 && plan.sameStream && k >= 0 && planValid[k] && sc.tileOrder == dTileOrder[k].ptr &&
          planDepth[k] == plan.depth && planNLt[k] == plan.nLt && plan.depth >= 2 && plan.depth <= RT_MAX_DEPTH && records))
        return hipSuccess;
    if (rt_split_units(plan.depth, plan.nLt) > (unsigned)(RT_SPLIT_UNITS_PER_PART * RT_SPLIT_MAX_PARTS)) return hipSuccess;
    if (freeRun != 0 && !splitForce) return hipSuccess;          // (frameCount advances: measuredEnd has the why)
    const volatile unsigned *seen = hSplitSeen.ptr;          // (split tiles, epoch) of the plan kernel that ran last
    if (!(seen && seen[1] == splitEpoch && seen[0] > 0u)) return hipSuccess;
    StreamRec *rec = plan.rec;
    const size_t stride = rt_split_slot_dwords(plan.depth, plan.nLt);
    const size_t need = (size_t)RT_SPLIT_MAX_TILES * stride;
    if (rec->splitRefused && need >= rec->splitRefused) return hipSuccess;          // (could not be had before: not asked for again)
    if (!rec->splitScratch.holds(need) || !rec->splitDesc) {
        // (a launch of this stream may still be working in a smaller scratch)
        if (rec->splitScratch.ptr) SCHED_TRY(hipStreamSynchronize(s));
        rec->splitStride = 0;
        hipError_t e = rec->splitScratch.grow(need);
        if (e == hipSuccess) e = rec->splitDesc.grow(2);
        if (e != hipSuccess) {          // no scratch to be had: the frame runs whole, as it does without a first-hit buffer
            (void)hipGetLastError();
            (void)rec->splitScratch.release();
            rec->splitRefused = need;
            return hipSuccess;
        }
    }
    if (rec->splitStride != stride) {
        // Every slot's arrival counter starts at zero, and the job that arrives last puts it back -- at ITS stride.  A frame of
        // another depth or light count finds slot j's counter at j * stride, in what the earlier frames left of their columns.
        // On the launch's stream: behind the stream's earlier split launches, ahead of the descriptor and of this one.
        SCHED_TRY(hipMemsetAsync(rec->splitScratch.ptr, 0, need * sizeof(float), s));
        rec->splitStride = stride;
    }
    if (rec->descGen[k] != planGen[k] || rec->descRecords[k] != records || rec->descScratch[k] != rec->splitScratch.ptr) {
        RtSplitDesc d;
        d.records = (const unsigned char *)records;
        d.parts = dSplitParts[k];
        d.slot = dSplitSlot[k];
        d.extra = dSplitExtra[k];
        d.counts = dSplitCounts[k];
        d.scratch = rec->splitScratch;
        // on the launch's stream: behind the stream's earlier launches that read this descriptor, ahead of this one
        SCHED_TRY(rt_launch_split_desc(rec->splitDesc.ptr + k, d, s));
        rec->descGen[k] = planGen[k];
        rec->descRecords[k] = records;
        rec->descScratch[k] = rec->splitScratch.ptr;
    }
    *out = rec->splitDesc.ptr + k;
    dbgSplitK = k;
    return hipSuccess;
}

hipError_t RtTileScheduler::splitTiles(unsigned char *out, int cap, int *nTiles) {
    *nTiles = 0;
    if (dbgSplitK == -2) return hipSuccess;
    SCHED_PASS(drain());
    *nTiles = dbgSplitTiles;
    const int n = dbgSplitTiles < cap ? dbgSplitTiles : cap;
    if (dbgSplitK < 0 || !dSplitParts[dbgSplitK].holds(dbgSplitTiles)) memset(out, 0, (size_t)n);
    else SCHED_TRY(hipMemcpy(out, dSplitParts[dbgSplitK], (size_t)n, hipMemcpyDeviceToHost));
    return hipSuccess;
}

hipError_t RtTileScheduler::splitPlanOf(const unsigned *order, const unsigned *costs, int nTiles, unsigned waveSlots, int depth, int nLt, int forceParts,
                                        const unsigned char *prevParts, unsigned char *parts, unsigned short *slot, unsigned *extra, unsigned *counts) {
    const size_t n = (size_t)nTiles;
    DevBuf<unsigned> dOrder, dCost, dExtra, dCounts;
    DevBuf<unsigned char> dPrev, dParts;
    DevBuf<unsigned short> dSlot;
    SCHED_TRY(dOrder.grow(n));
    SCHED_TRY(dCost.grow(n));
    SCHED_TRY(dParts.grow(n));
    SCHED_TRY(dSlot.grow(n));
    SCHED_TRY(dExtra.grow(RT_SPLIT_EXTRA_BLOCKS));
    SCHED_TRY(dCounts.grow(2));
    if (prevParts) SCHED_TRY(dPrev.grow(n));
    SCHED_TRY(hipMemcpyAsync(dOrder, order, n * sizeof(unsigned), hipMemcpyHostToDevice, own));
    SCHED_TRY(hipMemcpyAsync(dCost, costs, n * sizeof(unsigned), hipMemcpyHostToDevice, own));
    if (prevParts) SCHED_TRY(hipMemcpyAsync(dPrev, prevParts, n, hipMemcpyHostToDevice, own));
    SCHED_TRY(hipMemsetAsync(dExtra, 0xFF, RT_SPLIT_EXTRA_BLOCKS * sizeof(unsigned), own));      // an entry the plan leaves unwritten is no job
    SCHED_TRY(rt_launch_split_plan(dOrder, dCost, nTiles, waveSlots, depth, nLt, forceParts, prevParts ? dPrev.ptr : nullptr, dParts, dSlot, dExtra,
                                   dCounts, 0u, nullptr, own));
    SCHED_TRY(hipStreamSynchronize(own));
    SCHED_TRY(hipMemcpy(parts, dParts, n, hipMemcpyDeviceToHost));
    SCHED_TRY(hipMemcpy(slot, dSlot, n * sizeof(unsigned short), hipMemcpyDeviceToHost));
    SCHED_TRY(hipMemcpy(extra, dExtra, RT_SPLIT_EXTRA_BLOCKS * sizeof(unsigned), hipMemcpyDeviceToHost));
    SCHED_TRY(hipMemcpy(counts, dCounts, 2 * sizeof(unsigned), hipMemcpyDeviceToHost));
    return hipSuccess;
}

hipError_t RtTileScheduler::tileCosts(unsigned *out, int cap, int *nTiles, int *tilesX) {
    *nTiles = fbTiles;
    *tilesX = fbTilesX;
    if (fbTiles == 0 || !dTileCost) return hipSuccess;
    SCHED_PASS(drain());
    const int n = fbTiles < cap ? fbTiles : cap;
    SCHED_TRY(hipMemcpy(out, dTileCost, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost));
    return hipSuccess;
}

// ---- predicted order ------------------------------------------------------------------------------------------------------
// No measured order yet (the first frames of a geometry): the order PREDICTED from the frame's own inputs, made in this stream
// just before the frame (cached per stream and inputs).  Only for frames large enough that the pass (one path per tile against
// every object, 36 us at 1080p / 18 objects) costs less than the order gains: measured it pays from 4K on
// (C4: 6.97 -> 6.61 ms), at 1080p the raster order of the configs' scenes is already close to heavy-first and it does not.

hipError_t RtTileScheduler::predictedBegin(const RtFrame &f, RtDeviceScene &sc, hipStream_t s, unsigned long long inputsGen, const Plan &plan) {
    const int nTiles = plan.nTiles;
    const double work = (double)nTiles * (double)(f.p.maxRayDepth > 0 ? f.p.maxRayDepth : 1) * (double)(f.nObj > 0 ? f.nObj : 1);
    // (no objects: nothing to predict from -- every tile costs the same -- and the kernel stages the objects in LDS sized by nObj)
    if (nTiles < predMinTiles || f.nObj <= 0 || f.nObj > RT_ST_MAX_OBJECTS || work > 3.0e8) return hipSuccess;
    // the inputs this frame's tile costs are a function of
    unsigned long long key = 1469598103934665603ull;
    auto mix = [&key](const void *in, size_t n) {
        for (size_t k = 0; k < n; k++) key = (key ^ ((const unsigned char *)in)[k]) * 1099511628211ull;
    };
    mix(&f, sizeof f);
    mix(&inputsGen, sizeof inputsGen);
    StreamRec *rec = plan.rec;
    if (!(rec->predOrder.holds((size_t)33 * nTiles) && rec->predCls.holds(nTiles) && rec->predCounts)) {
        SCHED_TRY(hipStreamSynchronize(s));
        rec->predValid = false;
        SCHED_TRY(rec->predOrder.release());
        SCHED_TRY(rec->predCls.release());
        SCHED_TRY(rec->predOrder.grow((size_t)33 * nTiles));      // the order, then the 32 class segments
        SCHED_TRY(rec->predCls.grow(nTiles));
        if (!rec->predCounts) {
            SCHED_TRY(rec->predCounts.grow(64));
            SCHED_TRY(hipMemsetAsync(rec->predCounts, 0, 64 * sizeof(unsigned), s));
            rec->predSet = 1;
        }
    }
    const size_t segStride = rec->predCls.cap;      // the tile count both buffers were sized for
    if (!rec->predValid || rec->predKey != key) {
        rec->predSet ^= 1;
        SCHED_TRY(rt_launch_predict_order(f, sc, plan.tilesX, nTiles, rec->predOrder + segStride, (int)segStride,
                                          rec->predCounts + 32 * rec->predSet, rec->predCounts + 32 * (rec->predSet ^ 1),
                                          dbgWantCls ? rec->predCls.ptr : nullptr, rec->predOrder, s));
        rec->predKey = key;
        rec->predValid = true;
    }
    sc.tileOrder = rec->predOrder;
    dbgPredCls = rec->predCls;
    dbgPredTiles = nTiles;
    return hipSuccess;
}

hipError_t RtTileScheduler::predictedClasses(unsigned char *out, int cap, int *nTiles) {
    *nTiles = 0;
    if (!dbgPredCls) return hipSuccess;
    SCHED_PASS(drain());
    *nTiles = dbgPredTiles;
    const int n = *nTiles < cap ? *nTiles : cap;
    SCHED_TRY(hipMemcpy(out, dbgPredCls, (size_t)n, hipMemcpyDeviceToHost));
    return hipSuccess;
}

// ---- per-phase orders (rt_sched.h has the why) ----------------------------------------------------------------------------

void RtTileScheduler::phaseForget() {
    // the phases' orders belong to the old geometry.  Sorts still queued on the phase stream finish before any
    // sort of the new geometry (one stream), and an order is read only once its own sort has been seen complete.
    memset(phaseState, 0, sizeof phaseState);
    phaseTiles = 0;
}

hipError_t RtTileScheduler::phaseBegin(const RtFrame &f, RtDeviceScene &sc, Plan *plan) {
    const int nTiles = plan->nTiles, fc = f.p.frameCount;
    freeRun = (haveLastFc && fc != lastFc) ? (freeRun < 1000 ? freeRun + 1 : 1000) : 0;
    lastFc = fc;
    haveLastFc = true;
    if (!(phaseOn && schedMode == 2 && freeRun >= 2 && (size_t)nTiles * 64 * 2 * sizeof(unsigned) <= ((size_t)1 << 30))) return hipSuccess;
    SCHED_TRY(phaseStream.create());
    if (!(dPhaseCost.holds((size_t)nTiles * 64) && dPhaseOrder.holds((size_t)nTiles * 64) && dPhaseSnap.holds(nTiles))) {
        SCHED_PASS(drain());
        phaseTiles = 0;
        for (DevBuf<unsigned> *b : {&dPhaseCost, &dPhaseOrder, &dPhaseSnap}) SCHED_TRY(b->release());
        SCHED_TRY(dPhaseCost.grow((size_t)nTiles * 64));
        SCHED_TRY(dPhaseOrder.grow((size_t)nTiles * 64));
        SCHED_TRY(dPhaseSnap.grow(nTiles));
    }
    if (phaseTiles != nTiles) {       // first free-running frame of this geometry: every phase starts empty
        memset(phaseState, 0, sizeof phaseState);
        SCHED_TRY(hipMemsetAsync(dPhaseCost, 0, (size_t)nTiles * 64 * sizeof(unsigned), phaseStream));
        phaseTiles = nTiles;
    }
    const int phase = ((fc % 64) + 64) % 64;
    if (phaseState[phase] == 1) {
        const hipError_t q = hipEventQuery(evPhase[phase]);
        (void)hipGetLastError();
        if (q == hipSuccess) phaseState[phase] = 2;
    }
    // (a phase whose sort has not been SEEN complete keeps the average order chosen before: no stream ever waits for a sort)
    if (phaseState[phase] == 2) sc.tileOrder = dPhaseOrder + (size_t)phase * nTiles;
    sc.tileCost = dPhaseCost + (size_t)phase * nTiles;
    plan->phase = phase;
    return hipSuccess;
}

hipError_t RtTileScheduler::phaseEnd(const Plan &plan) {
    // this frame's costs -> its phase's order, behind every launch that may still read that order (this one included), on
    // the phase stream; the costs also join the all-phase average (dTileCost) that the periodic sort works on
    const size_t at = (size_t)plan.phase * plan.nTiles;
    SCHED_PASS(waitForLaunches(phaseStream));
    SCHED_TRY(rt_launch_lpt_sort(dPhaseCost + at, dPhaseSnap, dPhaseOrder + at, plan.nTiles, phaseStream, dTileCost));
    SCHED_TRY(evPhase[plan.phase].create(hipEventDisableTiming));
    SCHED_TRY(hipEventRecord(evPhase[plan.phase], phaseStream));
    phaseState[plan.phase] = 1;
    return hipSuccess;
}

// ---- the order a launch was given (rt_debug_tile_order; rt_sched.h has the why) ------------------------------------------------

hipError_t RtTileScheduler::noteOrder(const RtDeviceScene &sc, hipStream_t s, int nTiles, const StreamRec *rec) {
    // who supplied the order is read off the pointer begin() ended up with (no bookkeeping on the path of a context that never asks):
    // the adopted measured buffer, this stream's prediction, else a phase's slice of dPhaseOrder
    const unsigned *o = sc.tileOrder;
    dbgOrderPolicy = !o ? 0 : (fbCur >= 0 && o == dTileOrder[fbCur].ptr) ? 1 : (o == rec->predOrder.ptr) ? 2 : 3;
    dbgOrderTiles = nTiles;
    if (!o) return hipSuccess;
    if (!dDbgOrder.holds(nTiles)) {
        SCHED_PASS(drain());           // copies into the old buffer may still be queued
        SCHED_TRY(dDbgOrder.grow(nTiles));
    }
    // behind everything begin() has put on s for this order (the waits for its sort, the prediction), ahead of the launch
    SCHED_TRY(hipMemcpyAsync(dDbgOrder, o, (size_t)nTiles * sizeof(unsigned), hipMemcpyDeviceToDevice, s));
    return hipSuccess;
}

hipError_t RtTileScheduler::tileOrder(unsigned *out, int cap, int *nTiles, int *policy) {
    *nTiles = 0;
    *policy = 0;
    if (!dbgWantOrder || dbgOrderTiles == 0) return hipSuccess;
    SCHED_PASS(drain());
    *nTiles = dbgOrderTiles;
    *policy = dbgOrderPolicy;
    const int n = dbgOrderTiles < cap ? dbgOrderTiles : cap;
    if (dbgOrderPolicy == 0)
        for (int i = 0; i < n; i++) out[i] = (unsigned)i;
    else
        SCHED_TRY(hipMemcpy(out, dDbgOrder, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost));
    return hipSuccess;
}

hipError_t RtTileScheduler::lptSortOf(unsigned *costs, int nTiles, unsigned *order, unsigned *accum) {
    const size_t bytes = (size_t)nTiles * sizeof(unsigned);
    DevBuf<unsigned> dCost, dSnap, dOrder, dAccum;
    SCHED_TRY(dCost.grow(nTiles));
    SCHED_TRY(dSnap.grow(nTiles));
    SCHED_TRY(dOrder.grow(nTiles));
    if (accum) SCHED_TRY(dAccum.grow(nTiles));
    SCHED_TRY(hipMemcpyAsync(dCost, costs, bytes, hipMemcpyHostToDevice, own));
    SCHED_TRY(hipMemsetAsync(dOrder, 0xFF, bytes, own));      // an entry the sort leaves unwritten is no tile id
    if (accum) SCHED_TRY(hipMemcpyAsync(dAccum, accum, bytes, hipMemcpyHostToDevice, own));
    SCHED_TRY(rt_launch_lpt_sort(dCost, dSnap, dOrder, nTiles, own, accum ? dAccum.ptr : nullptr));
    SCHED_TRY(hipStreamSynchronize(own));
    SCHED_TRY(hipMemcpy(costs, dCost, bytes, hipMemcpyDeviceToHost));
    SCHED_TRY(hipMemcpy(order, dOrder, bytes, hipMemcpyDeviceToHost));
    if (accum) SCHED_TRY(hipMemcpy(accum, dAccum, bytes, hipMemcpyDeviceToHost));
    return hipSuccess;
}

// ---- one frame ------------------------------------------------------------------------------------------------------------

hipError_t RtTileScheduler::begin(const RtFrame &f, RtDeviceScene &sc, hipStream_t s, bool packet, unsigned long long inputsGen, Plan *plan, int costClass) {
    *plan = Plan();
    plan->costClass = costClass;
    sc.tileOrder = nullptr;
    sc.tileCost = nullptr;
    SCHED_PASS(record(s, &plan->rec));
    if (packet) {
        plan->sameStream = haveLastPacket && lastPacketStream == s;
        lastPacketStream = s;
        haveLastPacket = true;
    }
    if (!(packet && schedMode != 0 && f.p.regionW > 0 && f.p.regionH > 0)) {
        if (dbgWantOrder && packet && f.p.regionW > 0 && f.p.regionH > 0) {      // raster mode: the launch still has an order to report
            int bt = 0, tile = 0, tilesX = 0, nTiles = 0;
            rt_packet_geometry(f.nObj, f.p.regionW, f.p.regionH, &bt, &tile, &tilesX, &nTiles);
            SCHED_PASS(noteOrder(sc, s, nTiles, plan->rec));
        }
        return hipSuccess;
    }
    int tile = 0;
    rt_packet_geometry(f.nObj, f.p.regionW, f.p.regionH, &plan->bt, &tile, &plan->tilesX, &plan->nTiles);
    plan->depth = f.p.maxRayDepth;
    plan->nLt = f.nLt;
    plan->waves = rt_packet_profile_waves(f, sc);
    bool newGeometry = false;
    SCHED_PASS(measuredBegin(sc, s, plan, &newGeometry));
    if (newGeometry) phaseForget();
    if (fbCur < 0 && schedMode == 2) SCHED_PASS(predictedBegin(f, sc, s, inputsGen, *plan));
    SCHED_PASS(phaseBegin(f, sc, plan));
    if (dbgWantOrder) SCHED_PASS(noteOrder(sc, s, plan->nTiles, plan->rec));
    return hipSuccess;
}

hipError_t RtTileScheduler::end(const Plan &plan, hipStream_t s) {
    SCHED_TRY(hipEventRecord(plan.rec->last, s));      // every launch, on every stream: rt_set_scene orders behind it
    if (plan.phase >= 0) SCHED_PASS(phaseEnd(plan));
    if (plan.sortAfter) SCHED_PASS(measuredEnd(plan));
    return hipSuccess;
}
