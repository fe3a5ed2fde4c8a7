// rt_present.cpp -- the present ring's HIP side (rt_present.h has the contract).  The order of the HIP operations of a
// submit -- acquire(), the caller's pack, deliver() -- is what makes a ticket's bytes the frame that was submitted.
#include "rt_present.h"

#define RING_TRY(call)                                          \
    do {                                                        \
        hipError_t e_ = (call);                                 \
        if (e_ != hipSuccess) return hipFailed(#call, e_);      \
    } while (0)

int PresentRing::configure(int slots) {
    if (slots < 2 || slots > PresentBook::kMaxSlots) return refused("rt_present_configure: 2..8 slots");
    if (book.outstanding()) return refused("rt_present_configure: a ticket is outstanding (wait for it first)");
    // every live ticket's copy has been seen complete, older ones finished before them (one copy stream): nothing reads the buffers
    RING_TRY(hipSetDevice(device));
    for (int k = slots; k < PresentBook::kMaxSlots; k++) {
        RING_TRY(slot[k].dStage.release());
        RING_TRY(slot[k].hPixels.release());
    }
    book.rebase(slots);
    return RT_OK;
}

int PresentRing::acquire(size_t bytes, hipStream_t s, void **stage) {
    RING_TRY(hipSetDevice(device));
    const int k = book.slotOf(book.next);
    Slot &sl = slot[k];
    const bool used = book.slot[k].used;
    RING_TRY(copy.create());
    RING_TRY(sl.packed.create(hipEventDisableTiming));
    RING_TRY(sl.done.create(hipEventDisableTiming));
    if (!(sl.dStage.holds(bytes) && sl.hPixels.holds(bytes))) {
        if (used) RING_TRY(hipEventSynchronize(sl.done));       // this slot's own last copy; the other slots are untouched
        RING_TRY(sl.dStage.grow(bytes));
        RING_TRY(sl.hPixels.grow(bytes));
    }
    if (used) RING_TRY(hipStreamWaitEvent(s, sl.done, 0));      // the copy of ticket - slots has left the staging buffer
    *stage = sl.dStage.ptr;
    return RT_OK;
}

int PresentRing::deliver(size_t bytes, hipStream_t s, uint64_t *ticket) {
    Slot &sl = slot[book.slotOf(book.next)];
    RING_TRY(hipEventRecord(sl.packed, s));
    RING_TRY(hipStreamWaitEvent(copy, sl.packed, 0));
    RING_TRY(hipMemcpyAsync(sl.hPixels, sl.dStage, bytes, hipMemcpyDeviceToHost, copy));
    RING_TRY(hipEventRecord(sl.done, copy));
    *ticket = book.issue(bytes);
    return RT_OK;
}

int PresentRing::lookup(uint64_t ticket, int *k) {
    if (ticket >= book.next) return refused("ticket has not been issued");
    if (!book.live(ticket)) return refused("ticket has expired (its slot was reused or the ring reconfigured)");
    *k = book.slotOf(ticket);
    return RT_OK;
}

int PresentRing::poll(uint64_t ticket, int *ready) {
    int k;
    int rc = lookup(ticket, &k);
    if (rc) return rc;
    RING_TRY(hipSetDevice(device));
    const hipError_t e = hipEventQuery(slot[k].done);
    if (e == hipErrorNotReady) {
        (void)hipGetLastError();           // not an error: keep it out of the next launch's hipGetLastError()
        return RT_OK;
    }
    if (e != hipSuccess) return hipFailed("hipEventQuery(done)", e);
    book.slot[k].seen = true;
    *ready = 1;
    return RT_OK;
}

int PresentRing::wait(uint64_t ticket, const void **hostPixels, size_t *bytes) {
    int k;
    int rc = lookup(ticket, &k);
    if (rc) return rc;
    RING_TRY(hipSetDevice(device));
    RING_TRY(hipEventSynchronize(slot[k].done));
    book.slot[k].seen = true;
    *hostPixels = slot[k].hPixels.ptr;
    if (bytes) *bytes = book.slot[k].bytes;
    return RT_OK;
}

hipError_t PresentRing::drain() { return copy ? hipStreamSynchronize(copy) : hipSuccess; }
