"""CPU-only tests of the YUV output's host side (include/rt_mi355.h): rt_display_yuv_coeffs against the formulas restated in
tests/yuv_oracle.py and against the published tables, the properties the definition promises of them (white and greys exact, the
ranges of the cube corners), rt_display_yuv_layout, the byte layout of rt_yuv_desc and the refusals.  No GPU call is made."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import yuv_oracle as YO
from opengl_raytracing_amd import layout as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = list(itertools.product(YO.MATRICES, YO.RANGES))
CORNERS = np.array(list(itertools.product((0, 255), repeat=3)), dtype=np.int64)       # the eight corners of the RGB cube
INVALID = -1


@pytest.mark.parametrize("matrix,rng", PAIRS, ids=[f"{m}-{r}" for m, r in PAIRS])
def test_coeffs_match_the_formulas_and_the_published_tables(host, matrix, rng):
    got = host.yuv_coeffs(matrix, rng)
    assert got.dtype == np.int32 and got.shape == (12,)
    want = YO.coeffs(matrix, rng)
    assert got.tolist() == want
    y, cb, cr = YO.PUBLISHED[(matrix, rng)]
    assert (tuple(want[0:3]), tuple(want[4:7]), tuple(want[8:11])) == (y, cb, cr)
    assert want[3] == (16 if rng == "limited" else 0) and want[7] == 0 and want[11] == 0


@pytest.mark.parametrize("matrix,rng", PAIRS, ids=[f"{m}-{r}" for m, r in PAIRS])
def test_rows_sum_as_promised(host, matrix, rng):
    c = host.yuv_coeffs(matrix, rng).tolist()
    sY = YO.RANGES[rng][0]
    assert sum(c[0:3]) == YO.rne(65536 * sY)
    assert sum(c[4:7]) == 0 and sum(c[8:11]) == 0
    assert c[6] == c[8] == YO.rne(32768 * YO.RANGES[rng][1])
    grey = np.repeat(np.arange(256, dtype=np.int64), 3).reshape(1, 256, 3)
    Y, Cb, Cr = YO.matrix_unclamped(grey, c)
    assert (Cb == 128).all() and (Cr == 128).all()
    assert Y[0, 0] == c[3] and Y[0, 255] == (235 if rng == "limited" else 255)
    assert (np.diff(Y[0]) >= 0).all()


@pytest.mark.parametrize("matrix,rng", PAIRS, ids=[f"{m}-{r}" for m, r in PAIRS])
def test_cube_corners_stay_in_range(host, matrix, rng):
    """One corner per 2x2 block (the sums are four times the code).  LIMITED needs no clamp; FULL reaches 256 in both chroma
    channels (pure blue, pure red), which is what the clamp is for."""
    c = host.yuv_coeffs(matrix, rng).tolist()
    img = np.repeat(np.repeat(CORNERS.reshape(1, 8, 3), 2, axis=0), 2, axis=1)
    Y, Cb, Cr = YO.matrix_unclamped(img, c)
    if rng == "limited":
        assert (Y.min(), Y.max()) == (16, 235)
        assert (Cb.min(), Cb.max()) == (16, 240) and (Cr.min(), Cr.max()) == (16, 240)
    else:
        assert (Y.min(), Y.max()) == (0, 255)
        assert (Cb.min(), Cb.max()) == (1, 256) and (Cr.min(), Cr.max()) == (1, 256)     # (-127.5 + 0.5 floors to -127)


@pytest.mark.parametrize("fmt", YO.FORMATS)
@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (3, 5), (8, 2), (1920, 1080)])
def test_layout(host, w, h, fmt):
    got = host.yuv_layout(w, h, fmt)
    off, pitch, n = YO.layout(w, h, fmt)
    assert (got.offset, got.pitch, got.bytes) == (off, pitch, n)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    assert n == w * h + 2 * cw * ch
    if fmt == "nv12":
        assert got.offset[2] == got.offset[1] + 1 and got.pitch[2] == got.pitch[1] == 2 * cw
    else:
        assert got.offset[2] + cw * ch == n
    frame = np.arange(n, dtype=np.uint32).astype(np.uint8)
    planes = host.yuv_planes(frame, w, h, fmt)
    assert planes[0].shape == (h, w) and planes[0][h - 1, w - 1] == frame[w * h - 1]
    if fmt == "nv12":
        assert planes[1].shape == (ch, cw, 2)
        assert planes[1][ch - 1, cw - 1, 0] == frame[n - 2] and planes[1][ch - 1, cw - 1, 1] == frame[n - 1]
    else:
        assert planes[1].shape == planes[2].shape == (ch, cw)
        assert planes[1][0, 0] == frame[w * h] and planes[2][ch - 1, cw - 1] == frame[n - 1]


def test_1080p_moves_three_megabytes(host):
    assert host.yuv_layout(1920, 1080, "nv12").bytes == 1920 * 1080 * 3 // 2 == host.yuv_layout(1920, 1080, "i420").bytes


def test_yuv_desc_layout(tmp_path):
    """rt_yuv_desc is 48 bytes with the header's field order, in C (the header's own static assert compiles) and in ctypes."""
    assert ctypes.sizeof(L.RtYuvDesc) == 48
    exp = dict(width=0, height=4, format=8, matrix=12, range=16, transfer=20, flags=24, exposure=28, reserved=32)
    for k, v in exp.items():
        assert getattr(L.RtYuvDesc, k).offset == v, k
    header = open(os.path.join(REPO, "include", "rt_mi355.h")).read()
    assert "sizeof(rt_yuv_desc) == 48" in header
    src = tmp_path / "y.c"
    src.write_text('#include "rt_mi355.h"\n'
                   "int main(void){ rt_yuv_desc d = {0}; d.format = RT_YUV_I420; d.matrix = RT_YUV_BT601; d.range = RT_YUV_FULL;\n"
                   " d.transfer = RT_DISPLAY_RGBA8_SRGB; d.flags = RT_DISPLAY_FLIP_ROWS;\n"
                   " return sizeof d == 48 && d.format == 1 && d.matrix == 1 && d.range == 1 && RT_YUV_NV12 == 0 && RT_YUV_BT709 == 0\n"
                   "        && RT_YUV_LIMITED == 0 ? 0 : 1; }\n")
    exe = tmp_path / "y"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_make_yuv_desc():
    d = L.make_yuv_desc(7, 5, "i420", "bt601", "full", "linear", flip=True, exposure=0.5)
    assert (d.width, d.height, d.format, d.matrix, d.range, d.transfer, d.flags, d.exposure) == (
        7, 5, L.YUV_I420, L.YUV_BT601, L.YUV_FULL, L.DISPLAY_RGBA8_LINEAR, L.DISPLAY_FLIP_ROWS, 0.5)
    assert list(d.reserved) == [0, 0, 0, 0]
    d = L.make_yuv_desc(7, 5)
    assert (d.format, d.matrix, d.range, d.transfer, d.flags, d.exposure) == (L.YUV_NV12, L.YUV_BT709, L.YUV_LIMITED, L.DISPLAY_RGBA8_SRGB, 0, 1.0)


def test_host_functions_refuse(host):
    lib = host.load_library()
    out = (ctypes.c_int32 * 12)(*([77] * 12))
    for matrix, rng in [(2, 0), (-1, 0), (0, 2), (0, -1), (7, 7)]:
        assert lib.rt_display_yuv_coeffs(matrix, rng, out) == INVALID
    assert lib.rt_display_yuv_coeffs(0, 0, None) == INVALID
    assert list(out) == [77] * 12                              # a refused call writes nothing
    assert lib.rt_display_yuv_coeffs(1, 1, out) == 0 and list(out) == YO.coeffs("bt601", "full")
    off, pitch, n = (ctypes.c_size_t * 3)(), (ctypes.c_size_t * 3)(), ctypes.c_size_t(5)
    good = L.make_yuv_desc(3, 5, "i420")
    bad = [L.make_yuv_desc(0, 5), L.make_yuv_desc(3, 0), L.make_yuv_desc(-2, 5), L.make_yuv_desc(3, -1), L.make_yuv_desc(3, 5, format=2),
           L.make_yuv_desc(3, 5, format=-1)]
    for d in bad:
        assert lib.rt_display_yuv_layout(ctypes.byref(d), off, pitch, ctypes.byref(n)) == INVALID
    assert lib.rt_display_yuv_layout(None, off, pitch, ctypes.byref(n)) == INVALID
    assert lib.rt_display_yuv_layout(ctypes.byref(good), None, pitch, ctypes.byref(n)) == INVALID
    assert lib.rt_display_yuv_layout(ctypes.byref(good), off, None, ctypes.byref(n)) == INVALID
    assert n.value == 5
    assert lib.rt_display_yuv_layout(ctypes.byref(good), off, pitch, None) == 0          # the byte count alone is optional
    assert (tuple(off), tuple(pitch)) == YO.layout(3, 5, "i420")[:2]
    odd = L.make_yuv_desc(3, 5, "i420", matrix=9, range=9, transfer=9, exposure=-1.0)   # the layout reads width, height and format only
    odd.flags, odd.reserved[2] = 8, 1
    assert lib.rt_display_yuv_layout(ctypes.byref(odd), off, pitch, ctypes.byref(n)) == 0 and n.value == 15 + 2 * 2 * 3
