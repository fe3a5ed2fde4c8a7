"""CPU-only test of the record buffer's layout (csrc/rt_firsthit.h, which holds no HIP type): first-hit records and colours
(DESIGN.md section 26), behind them the settled tiles' final records and the tile flags (section 27), all in one allocation.
A stand-alone C++ program with its own main includes the header alone, built with the address and undefined-behaviour
sanitizers, and prints the layout of every window given to it; the test checks the four parts against what the kernel and the
ABI layer rely on.  No GPU call is made."""
import os
import subprocess
import warnings

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "opengl_raytracing_amd", "csrc")
INCLUDE = os.path.join(REPO, "include")

PROGRAM = r"""
#include "rt_firsthit.h"
#include <stdio.h>
#include <stdlib.h>

int main(int argc, char **argv) {
    printf("cap %llu\n", (unsigned long long)RtFirstHit::kMaxPixels);
    for (int k = 1; k + 1 < argc; k += 2) {
        const int w = atoi(argv[k]), h = atoi(argv[k + 1]);
        const RtFirstHitLayout l = rt_first_hit_layout(w, h);
        printf("%d %d pixels %llu tiles %llu hits %llu colours %llu finals %llu flags %llu bytes %llu fn %llu %llu %llu %llu\n", w, h,
               (unsigned long long)l.pixels, (unsigned long long)l.tiles, (unsigned long long)l.hits, (unsigned long long)l.colours,
               (unsigned long long)l.finals, (unsigned long long)l.flags, (unsigned long long)l.bytes,
               (unsigned long long)rt_first_hit_bytes(w, h), (unsigned long long)rt_first_hit_colours_offset(w, h),
               (unsigned long long)rt_first_hit_finals_offset(w, h), (unsigned long long)rt_first_hit_flags_offset(w, h));
    }
    return 0;
}
"""

CAP = 1 << 24
WINDOWS = [(1, 1), (8, 8), (48, 32), (52, 35), (1920, 1080), (4096, 4096), (CAP, 1), (1, CAP)]      # the last three: the cap


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    d = tmp_path_factory.mktemp("settled_layout")
    src, exe = d / "layout.cpp", d / "layout"
    src.write_text(PROGRAM)
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-I", INCLUDE, str(src), "-o", str(exe)]
    sanitized = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True)
    if sanitized.returncode != 0:              # a compiler without the sanitizers' runtimes: the same program without them, and said so
        warnings.warn("the layout program was built WITHOUT -fsanitize=address,undefined: " + sanitized.stderr.decode(errors="replace")[-400:])
        subprocess.run(base, check=True)
    run = subprocess.run([str(exe), *[str(v) for wh in WINDOWS for v in wh]], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    assert lines[0] == f"cap {CAP}"
    out = {}
    for ln in lines[1:]:
        f = ln.split()
        out[(int(f[0]), int(f[1]))] = dict(zip(f[2:16:2], map(int, f[3:16:2])), fn=[int(x) for x in f[17:]])
    assert set(out) == set(WINDOWS)
    return out


@pytest.mark.parametrize("w,h", WINDOWS)
def test_parts_are_aligned_disjoint_and_add_up(layouts, w, h):
    l = layouts[(w, h)]
    px = w * h
    assert px <= CAP and l["pixels"] == px
    assert l["tiles"] == -(-w // 8) * -(-h // 8)
    # (offset, bytes the kernel addresses there) of the four parts, in buffer order
    parts = [(l["hits"], 8 * px), (l["colours"], 12 * px), (l["finals"], 32 * px), (l["flags"], l["tiles"])]
    for at, _ in parts:
        assert at % 16 == 0
    assert parts[0][0] == 0
    for (at, size), (nxt, _) in zip(parts, parts[1:] + [(l["bytes"], 0)]):
        assert at + size <= nxt, "two parts overlap (or the last one leaves the buffer)"
        assert nxt - (at + size) < 16, "more than alignment padding between two parts"
    assert l["bytes"] % 16 == 0
    assert l["fn"] == [l["bytes"], l["colours"], l["finals"], l["flags"]]       # the functions the kernel calls agree with the struct


def test_memory_is_what_the_design_states(layouts):
    """52 bytes per pixel and one per tile: 1080p takes 108 MB, the cap 832 MiB (+ 256 KiB of flags)."""
    assert layouts[(1920, 1080)]["bytes"] == 52 * 1920 * 1080 + 32400
    assert layouts[(4096, 4096)]["bytes"] == 52 * CAP + (CAP // 64)
