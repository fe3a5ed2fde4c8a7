"""CPU-only test of prefix replay's host side (csrc/rt_firsthit.h, which holds no HIP type): the tile
flag's encoding, the 13-dword prefix record and where its dwords live in the record buffer.  A stand-alone C++ program with its
own main includes the header alone, built with the address and undefined-behaviour sanitizers; it checks the round trips itself
(exit status) and prints the byte offsets of every dword for the pixels the test asks about, which the test holds against the
three slots the pixel owns in the hits, colours and finals parts.  No GPU call is made."""
import os
import subprocess
import warnings

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "opengl_raytracing_amd", "csrc")
INCLUDE = os.path.join(REPO, "include")

PROGRAM = r"""
#include "rt_firsthit.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static bool same3(const float *a, const float *b) { return memcmp(a, b, 12) == 0; }

int main(int argc, char **argv) {
    // ---- the flag byte: 0 = K 0, 1 = settled, 1 + K = K 1 .. cap; larger K resume at the cap
    CHECK(RT_PREFIX_CAP == 7 && RT_PREFIX_DWORDS == 13 && sizeof(RtPrefixRecord) == 52);
    CHECK(rt_prefix_flag(false, 0) == 0 && rt_prefix_flag(true, 0) == 1);
    for (int k = 0; k <= 300; k++) {
        const unsigned f = rt_prefix_flag(false, k);
        CHECK(f <= 255 && f != 1);                             // fits the byte, never reads as settled
        CHECK(!rt_prefix_flag_settled(f));
        CHECK(rt_prefix_flag_depth(f) == (k < RT_PREFIX_CAP ? k : RT_PREFIX_CAP));
        CHECK(rt_prefix_flag(true, k) == 1 && rt_prefix_flag_settled(rt_prefix_flag(true, k)) && rt_prefix_flag_depth(1) == 0);
    }
    CHECK(rt_prefix_flag(false, -3) == 0);
    // ---- records: every bit pattern comes back, NaN payloads, -0 and denormals included
    const uint32_t odd[6] = {0x80000000u, 0x7fc01234u, 0xffffffffu, 0x00000001u, 0x7f800000u, 0x3f800000u};
    for (int trial = 0; trial < 64; trial++) {
        float fc[3], P[3], a[3], rd[3];
        for (int k = 0; k < 3; k++) {
            fc[k] = rt_prefix_float(odd[(trial + k) % 6]);
            P[k] = rt_prefix_float(0x40000000u + 7919u * (unsigned)(trial * 3 + k));
            a[k] = rt_prefix_float(odd[(trial + k + 3) % 6]);
            rd[k] = rt_prefix_float(0xbf000000u + 104729u * (unsigned)(trial * 3 + k));
        }
        const int nObj = 18, hit = trial % nObj;
        {   // a lane that is alive: hit, finalColor, P, throughput, rd
            const RtPrefixRecord r = rt_prefix_pack(true, hit, fc, P, a, rd);
            int h = -2;
            float fc2[3], P2[3], thr2[3], rd2[3], N2[3] = {1.0f, 2.0f, 3.0f};
            CHECK(rt_prefix_unpack(r, nObj, &h, fc2, P2, thr2, rd2, N2));
            CHECK(h == hit && same3(fc, fc2) && same3(P, P2) && same3(a, thr2) && same3(rd, rd2));
            CHECK(N2[0] == 1.0f && N2[1] == 2.0f && N2[2] == 3.0f);                  // N is not the record's to give
            // an object id beyond the scene never reaches a gather: the lane reads as ended
            CHECK(!rt_prefix_unpack(r, hit, &h, fc2, P2, thr2, rd2, N2) && h == -1);
        }
        {   // a lane whose path has ended: finalColor, P, N; the hit is -1 whatever idx held
            const RtPrefixRecord r = rt_prefix_pack(false, hit, fc, P, a, rd);
            int h = -2;
            float fc2[3], P2[3], thr2[3] = {4.0f, 5.0f, 6.0f}, rd2[3] = {7.0f, 8.0f, 9.0f}, N2[3];
            CHECK(!rt_prefix_unpack(r, nObj, &h, fc2, P2, thr2, rd2, N2));
            CHECK(h == -1 && r.w[0] == 0xffffffffu && same3(fc, fc2) && same3(P, P2) && same3(a, N2));
            CHECK(thr2[0] == 4.0f && rd2[2] == 9.0f && r.w[10] == 0 && r.w[11] == 0 && r.w[12] == 0);
        }
    }
    // ---- where the dwords live: "w h at" triples -> 13 byte offsets each
    for (int k = 1; k + 2 < argc; k += 3) {
        const int w = atoi(argv[k]), h = atoi(argv[k + 1]);
        const unsigned long long at = strtoull(argv[k + 2], nullptr, 10);
        printf("%d %d %llu", w, h, at);
        for (int d = 0; d < RT_PREFIX_DWORDS; d++) printf(" %llu", (unsigned long long)rt_prefix_dword_offset(w, h, at, d));
        printf("\n");
    }
    return 0;
}
"""

WINDOWS = [(1, 1), (8, 8), (52, 35), (1920, 1080)]


def pixels_of(w, h):
    """first, last, the corners of the first and last tile, and a stride through the middle"""
    px = w * h
    picks = {0, px - 1, min(7, px - 1), min(w * min(7, h - 1), px - 1), px // 2, px // 3, (px * 2) // 3}
    picks |= set(range(0, px, max(1, px // 97)))
    return sorted(picks)


@pytest.fixture(scope="module")
def offsets(tmp_path_factory):
    d = tmp_path_factory.mktemp("prefix_host")
    src, exe = d / "prefix.cpp", d / "prefix"
    src.write_text(PROGRAM)
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-I", INCLUDE, str(src), "-o", str(exe)]
    sanitized = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True)
    if sanitized.returncode != 0:              # a compiler without the sanitizers' runtimes: the same program without them, and said so
        warnings.warn("the prefix program was built WITHOUT -fsanitize=address,undefined: " + sanitized.stderr.decode(errors="replace")[-400:])
        subprocess.run(base, check=True)
    args = [str(v) for (w, h) in WINDOWS for at in pixels_of(w, h) for v in (w, h, at)]
    run = subprocess.run([str(exe), *args], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr          # the round trips of the flag and of the records are checked in the program
    out = {}
    for ln in run.stdout.splitlines():
        f = [int(x) for x in ln.split()]
        out[(f[0], f[1], f[2])] = f[3:]
    return out


def test_flag_and_record_round_trips(offsets):
    assert offsets                                   # (the program exits non-zero on the first round trip that fails)


@pytest.mark.parametrize("w,h", WINDOWS)
def test_the_52_bytes_stay_inside_the_pixels_three_slots(offsets, w, h):
    px = w * h
    align16 = lambda v: (v + 15) & ~15
    colours = align16(8 * px)                        # the layout tests/test_settled_layout_host.py pins
    finals = align16(colours + 12 * px)
    flags = finals + 32 * px
    seen = set()
    for at in pixels_of(w, h):
        off = offsets[(w, h, at)]
        assert len(off) == 13
        slots = [(8 * at, 8), (colours + 12 * at, 12), (finals + 32 * at, 32)]          # (offset, bytes) the pixel owns
        want = [s + 4 * k for s, n in slots for k in range(n // 4)]
        assert off == want, f"pixel {at} of {w} x {h}: dwords at {off}, its slots are {slots}"
        assert all(o % 4 == 0 and o + 4 <= flags for o in off)
        assert not (seen & set(off)), "two pixels share a dword"
        seen |= set(off)
