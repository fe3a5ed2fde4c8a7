// rt_present.h -- the ring rt_present_submit* deliver packed frames through, held by value in rt_context (rt_context.h).
// Ticket t lives in slot t % slots: the pack kernel writes the slot's device staging buffer on the caller's stream, the copy
// stream moves it to the slot's pinned buffer behind `packed` and records `done`.  The next user of the slot orders its pack
// behind `done` on the device; the host waits on `done` only for the ticket it asks for, before the slot's buffers grow, and
// (the copy stream as a whole) before the ring goes.  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

// Which tickets are live, and what the host knows of each slot: no HIP type, so it is tested without a GPU
// (tests/test_present_ring_host.py defines RT_PRESENT_BOOK_ONLY and includes nothing but this part).
struct PresentBook {
    static constexpr int kMaxSlots = 8;
    struct Slot {
        bool used = false;               // `done` has been recorded at least once
        bool seen = false;               // the host has seen the slot's current ticket complete (wait, or a ready poll)
        uint64_t ticket = 0;
        size_t bytes = 0;
    };
    int slots = 3;
    uint64_t next = 0;                   // the ticket the next submit returns
    uint64_t base = 0;                   // tickets below it were expired by a reconfiguration
    Slot slot[kMaxSlots];

    bool live(uint64_t t) const { return t < next && t >= base && next - t <= (uint64_t)slots; }
    int slotOf(uint64_t t) const { return (int)(t % (uint64_t)slots); }
    bool outstanding() const {           // some live ticket has not been seen complete
        for (int k = 0; k < slots; k++)
            if (slot[k].used && live(slot[k].ticket) && !slot[k].seen) return true;
        return false;
    }
    uint64_t issue(size_t bytes) {       // the next ticket takes its slot (and so expires ticket next - slots)
        Slot &sl = slot[slotOf(next)];
        sl.used = true;
        sl.seen = false;
        sl.ticket = next;
        sl.bytes = bytes;
        return next++;
    }
    void rebase(int n) {                 // n slots from now on; every earlier ticket expires, the numbering goes on
        slots = n;
        base = next;
    }
};

#ifndef RT_PRESENT_BOOK_ONLY
#include "rt_devbuf.h"
#include "rt_mi355.h"

// Every method returns RT_OK or an rt_status and then says in `failed` (and `failedHip`, for a HIP call) what went wrong.
class PresentRing {
public:
    void init(int deviceId) { device = deviceId; }
    int configure(int slots);            // refused while a live ticket is unseen; releases the slots above; expires every earlier ticket
    // A submit's way through the ring: the next slot, grown to `bytes` if need be, pack(stage, s) into its staging buffer on the
    // caller's stream s, the copy behind it, a ticket.  One ring and one ticket sequence for every format.  A submit that fails
    // half way issues no ticket.
    template <class Pack>
    int enqueue(size_t bytes, hipStream_t s, uint64_t *ticket, Pack pack) {
        void *stage;
        int rc = acquire(bytes, s, &stage);
        if (rc) return rc;
        const hipError_t e = pack(stage, s);
        if (e != hipSuccess) return hipFailed("pack(stage, s)", e);
        return deliver(bytes, s, ticket);
    }
    int poll(uint64_t ticket, int *ready);                                  // *ready = 1 once wait() would not block
    int wait(uint64_t ticket, const void **hostPixels, size_t *bytes);      // bytes may be NULL
    hipError_t drain();                  // frames on their way to the pinned buffers (and, before them, their packs)

    const char *failed = "";
    hipError_t failedHip = hipSuccess;

private:
    struct Slot {
        DevBuf<uint8_t> dStage;
        PinnedBuf<uint8_t> hPixels;
        DevEvent packed, done;
    };
    int acquire(size_t bytes, hipStream_t s, void **stage);     // device, copy stream, events, growth, s behind the slot's last copy
    int deliver(size_t bytes, hipStream_t s, uint64_t *ticket); // `packed`, the copy, `done`; then the bookkeeping
    int lookup(uint64_t ticket, int *k);
    int failedWith(int rc, const char *what, hipError_t e) { failed = what; failedHip = e; return rc; }
    int refused(const char *what) { return failedWith(RT_ERR_INVALID_ARG, what, hipSuccess); }
    int hipFailed(const char *call, hipError_t e) { return failedWith(RT_ERR_HIP, call, e); }

    int device = 0;
    PresentBook book;
    DevStream copy;                      // created by the first submit: a context that never presents opens no second stream
    Slot slot[PresentBook::kMaxSlots];
};
#endif
