"""CPU-only test of the present ring's bookkeeping (csrc/rt_present.h, the part without a HIP type): which tickets are live, when
one expires, when a reconfiguration is refused.  A stand-alone C++ program with its own main includes that part alone, replays a
script of operations and prints the outcome of each; the test compares the print-out with a restatement of the rules in Python
that keeps no slots at all, only the set of tickets seen.  No GPU call is made."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "opengl_raytracing_amd", "csrc")

PROGRAM = r"""
#define RT_PRESENT_BOOK_ONLY
#include "rt_present.h"
#include <stdio.h>
#include <stdlib.h>

static const char *state(const PresentBook &b, uint64_t t) { return t >= b.next ? "unissued" : (b.live(t) ? "live" : "expired"); }

int main(int argc, char **argv) {
    PresentBook b;
    for (int k = 1; k + 1 < argc; k += 2) {
        const char op = argv[k][0];
        const uint64_t v = strtoull(argv[k + 1], nullptr, 10);
        if (op == 'i') {                                    // issue a ticket for a frame of v bytes
            const uint64_t t = b.issue((size_t)v);
            printf("i %llu -> ticket %llu slot %d\n", (unsigned long long)v, (unsigned long long)t, b.slotOf(t));
        } else if (op == 's') {                             // the host sees ticket v complete (a live one only, as the ring does)
            if (b.live(v)) b.slot[b.slotOf(v)].seen = true;
            printf("s %llu -> %s\n", (unsigned long long)v, state(b, v));
        } else if (op == 'c') {                             // reconfigure to v slots
            const bool refused = b.outstanding();
            if (!refused) b.rebase((int)v);
            printf("c %llu -> %s\n", (unsigned long long)v, refused ? "refused" : "ok");
        } else if (op == 'q') {                             // query ticket v
            if (b.live(v)) printf("q %llu -> live slot %d bytes %zu\n", (unsigned long long)v, b.slotOf(v), b.slot[b.slotOf(v)].bytes);
            else printf("q %llu -> %s\n", (unsigned long long)v, state(b, v));
        } else {
            return 2;
        }
    }
    return 0;
}
"""


def model(script):
    """The rules of include/rt_mi355.h's rt_present_* in terms of tickets alone: ticket t is live from its issue until ticket
    t + slots is issued or the ring is reconfigured; a reconfiguration is refused while a live ticket has not been seen."""
    slots, nxt, base, seen, size, out = 3, 0, 0, set(), {}, []
    live = lambda t: base <= t < nxt and nxt - t <= slots
    state = lambda t: "unissued" if t >= nxt else ("live" if live(t) else "expired")
    for op, v in script:
        if op == "i":
            size[nxt] = v
            out.append(f"i {v} -> ticket {nxt} slot {nxt % slots}")
            nxt += 1
        elif op == "s":
            if live(v):
                seen.add(v)
            out.append(f"s {v} -> {state(v)}")
        elif op == "c":
            refused = any(live(t) and t not in seen for t in range(nxt))
            if not refused:
                slots, base = v, nxt
            out.append(f"c {v} -> {'refused' if refused else 'ok'}")
        else:
            out.append(f"q {v} -> live slot {v % slots} bytes {size[v]}" if live(v) else f"q {v} -> {state(v)}")
    return out


def q(*tickets):
    return [("q", t) for t in tickets]


# the default 3 slots: ticket t expires exactly when ticket t + 3 is issued; 99 was never issued
SCRIPT = [("q", 0), ("i", 10), ("i", 11), ("i", 12), *q(0, 1, 2, 3, 99), ("i", 13), *q(0, 1, 3), ("i", 14), *q(1, 2, 4)]
# a reconfiguration is refused while a live ticket is unseen (expired ones do not count, seeing one of two is not enough) ...
SCRIPT += [("c", 2), ("s", 0), ("s", 2), ("s", 3), ("c", 2), ("s", 4), ("s", 99)]
# ... allowed once all are seen; it expires every earlier ticket, and the numbering goes on.  2 slots: t expires at t + 2
SCRIPT += [("c", 2), *q(2, 3, 4, 5), ("i", 20), *q(4, 5), ("i", 21), *q(5, 6), ("i", 22), *q(5, 6, 7), ("i", 23), *q(6, 7, 8)]
SCRIPT += [("c", 8), ("s", 7), ("c", 8), ("s", 8), ("c", 8), *q(7, 8)]
# 8 slots: nine tickets, the first expires with the ninth; a reconfiguration to the same count expires the rest all the same
SCRIPT += [("i", 30 + k) for k in range(8)] + q(9, 16, 17) + [("i", 38)] + q(9, 10, 17) + [("s", t) for t in range(9, 18)]
SCRIPT += [("c", 8), *q(10, 17, 18), ("i", 40), *q(17, 18), ("c", 3), ("s", 18), ("c", 3), ("i", 41), *q(18, 19, 20)]


def test_model_covers_what_the_script_is_for():
    """The restatement itself says what the issue of a later ticket, a reconfiguration and a missing ticket do."""
    out = model(SCRIPT)
    assert "q 0 -> live slot 0 bytes 10" in out and out.index("q 0 -> expired") == out.index("i 13 -> ticket 3 slot 0") + 1
    assert "q 99 -> unissued" in out and "s 99 -> unissued" in out
    assert out.count("c 2 -> refused") == 2 and out.count("c 2 -> ok") == 1
    assert out[out.index("c 2 -> ok") + 1: out.index("c 2 -> ok") + 4] == ["q 2 -> expired", "q 3 -> expired", "q 4 -> expired"]
    assert "i 20 -> ticket 5 slot 1" in out and "i 38 -> ticket 17 slot 1" in out and "i 41 -> ticket 19 slot 1" in out


def test_ring_bookkeeping_matches_the_model(tmp_path):
    src = tmp_path / "ring.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "ring"
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)]
    sanitized = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True)
    if sanitized.returncode != 0:              # a compiler without the sanitizers' runtimes: the same program without them
        subprocess.run(base, check=True)
    args = [str(x) for step in SCRIPT for x in step]
    run = subprocess.run([str(exe), *args], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    got, want = run.stdout.splitlines(), model(SCRIPT)
    assert len(got) == len(want) == len(SCRIPT)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"step {k} {SCRIPT[k]}: the ring says {g!r}, the model {w!r}"
