"""CPU-only test of the argument rules the image stages' entry points share (csrc/rt_args.h, the part without a HIP type or a
context): which device ranges overlap, the pixel limit, reserved words, pointer alignment.  A stand-alone C++ program with its own
main includes that part alone and prints the outcome of each case; the test compares the print-out with the outcomes the public
header promises.  No GPU call is made."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "opengl_raytracing_amd", "csrc")

PROGRAM = r"""
#define RT_ARGS_RULES_ONLY
#include "rt_args.h"
#include <stdio.h>

static void ov(const char *what, uintptr_t a, size_t an, uintptr_t b, size_t bn) {
    const DevRange ra = {(const void *)a, an}, rb = {(const void *)b, bn};
    printf("%s %d %d\n", what, (int)overlaps(ra, rb), (int)overlaps(rb, ra));
}

int main() {
    ov("adjacent", 0x1000, 256, 0x1100, 256);
    ov("one_byte", 0x1000, 257, 0x1100, 256);
    ov("inside", 0x1000, 4096, 0x1800, 16);
    ov("same", 0x1000, 16, 0x1000, 16);
    ov("apart", 0x1000, 16, 0x9000, 16);
    ov("empty_inside", 0x1800, 0, 0x1000, 4096);
    ov("empty_at_start", 0x1000, 0, 0x1000, 4096);
    ov("empty_null", 0, 0, 0x1000, 4096);
    ov("both_empty", 0x1000, 0, 0x1000, 0);
    printf("px 1x1 %llu\n", (unsigned long long)rt_pixel_count(1, 1));
    printf("px 2^31-1 %llu\n", (unsigned long long)rt_pixel_count(2147483647, 1));
    printf("px 1x2^31-1 %llu\n", (unsigned long long)rt_pixel_count(1, 2147483647));
    printf("px 2^31 %llu\n", (unsigned long long)rt_pixel_count(65536, 32768));
    printf("px 46340 %llu\n", (unsigned long long)rt_pixel_count(46340, 46340));
    printf("px 46341 %llu\n", (unsigned long long)rt_pixel_count(46341, 46341));
    printf("px max %llu\n", (unsigned long long)rt_pixel_count(2147483647, 2147483647));
    printf("limit %llu\n", (unsigned long long)kRtMaxPixels);
    const int32_t zero[4] = {0, 0, 0, 0}, last[4] = {0, 0, 0, 1}, first[2] = {-1, 0}, one[1] = {0};
    printf("zero %d %d %d %d\n", (int)rt_all_zero(zero), (int)rt_all_zero(last), (int)rt_all_zero(first), (int)rt_all_zero(one));
    printf("aligned");
    for (uintptr_t p = 0x2000; p <= 0x2010; p += 4) printf(" %d", (int)rt_aligned16((const void *)p));
    printf(" %d\n", (int)rt_aligned16(nullptr));
    return 0;
}
"""

WANT = """adjacent 0 0
one_byte 1 1
inside 1 1
same 1 1
apart 0 0
empty_inside 0 0
empty_at_start 0 0
empty_null 0 0
both_empty 0 0
px 1x1 1
px 2^31-1 2147483647
px 1x2^31-1 2147483647
px 2^31 0
px 46340 2147395600
px 46341 0
px max 0
limit 2147483647
zero 1 0 0 1
aligned 1 0 0 0 1 1
""".splitlines()


def test_shared_argument_rules(tmp_path):
    """Adjacent ranges do not overlap, a shared byte does, an empty range overlaps nothing (rt_denoise's absent moments plane);
    2^31 - 1 pixels pass, 2^31 do not, and 46341 x 46341 is refused without overflowing (the sanitizer's to catch)."""
    src = tmp_path / "args.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "args"
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)]
    sanitized = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True)
    if sanitized.returncode != 0:              # a compiler without the sanitizers' runtimes: the same program without them
        subprocess.run(base, check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    got = run.stdout.splitlines()
    assert len(got) == len(WANT)
    for g, w in zip(got, WANT):
        assert g == w, f"rt_args.h says {g!r}, the contract {w!r}"
