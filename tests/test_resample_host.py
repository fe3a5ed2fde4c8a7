"""CPU-only tests of the resampler's host side (include/rt_mi355.h): rt_resample_taps against the independent builder of
tests/resample_oracle.py (windows exact; weights the same float32 or an adjacent one, since the library's double evaluation can
land on the other side of a float32 rounding tie but no further), the properties the definition promises of the tables, the
tap cap, the byte layout of rt_resample_desc and the refusals.  No GPU call is made."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import resample_oracle as RO
from opengl_raytracing_amd import layout as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, TOO_LARGE = -1, -4
FILTER_NAMES = ("area", "triangle", "lanczos3")
# src -> dst of tests/test_resample.py, per axis
SHAPES = [((1, 1), (1, 1)), ((1, 1), (5, 3)), ((7, 5), (1, 1)), ((8, 8), (4, 4)), ((64, 32), (32, 16)), ((67, 9), (33, 5)),
          ((33, 5), (67, 9)), ((16, 4), (16, 4)), ((257, 3), (64, 7)), ((640, 4), (64, 4)), ((640, 360), (213, 120)), ((96, 54), (640, 360))]
AXES = sorted({(s[k], d[k]) for s, d in SHAPES for k in (0, 1)})


def adjacent(a, b):
    """Every element of float32 a is b or one of b's float32 neighbours."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return bool(((a == b) | (a == np.nextafter(b, np.float32(np.inf))) | (a == np.nextafter(b, np.float32(-np.inf)))).all())


@pytest.fixture(scope="module")
def tables(host):
    """(S, D, filter) -> the library's table, built once for every test here."""
    return {(S, D, f): host.resample_taps(S, D, f) for S, D in AXES for f in FILTER_NAMES}


@pytest.mark.parametrize("filter", FILTER_NAMES)
def test_taps_match_the_independent_builder(tables, filter):
    for S, D in AXES:
        n, first, w = tables[(S, D, filter)]
        on, ofirst, ow = RO.taps(S, D, filter)
        assert n == on and w.shape == (D, n) and first.dtype == np.int32 and w.dtype == np.float32, (S, D)
        assert (first == ofirst).all(), (S, D)
        assert adjacent(w, ow), (S, D, np.abs(w - ow).max())


def test_the_count_alone(host):
    lib = host.load_library()
    n = ctypes.c_int(-7)
    assert lib.rt_resample_taps(640, 213, L.RESAMPLE_LANCZOS3, ctypes.byref(n), None, None, 0) == 0
    assert n.value == host.resample_taps(640, 213, "lanczos3")[0] == RO.taps(640, 213, "lanczos3")[0]


@pytest.mark.parametrize("S,D", [(8, 4), (64, 32), (640, 64), (9, 3), (64, 1), (128, 2)])
def test_area_of_a_whole_ratio_is_a_box(host, S, D):
    n, first, w = host.resample_taps(S, D, "area")
    assert n == S // D and (first == np.arange(D) * (S // D)).all()
    assert (w == np.float32(D / S)).all()


@pytest.mark.parametrize("S", [1, 4, 16, 257])
def test_equal_sizes_are_the_identity(host, S):
    for f in ("area", "triangle"):
        n, first, w = host.resample_taps(S, S, f)
        assert n == 1 and (first == np.arange(S)).all() and (w == np.float32(1)).all()
    n, first, w = host.resample_taps(S, S, "lanczos3")
    assert n == 5 and (first == np.arange(S) - 2).all()
    assert (w[:, 2] == np.float32(1)).all() and (np.delete(w, 2, axis=1) == 0).all()


@pytest.mark.parametrize("filter", FILTER_NAMES)
def test_mirrored_indices_have_mirrored_taps(tables, filter):
    """Index D-1-i reads the mirror image of index i's window with the weights reversed (the zero padding set aside)."""
    for S, D in AXES:
        n, first, w = tables[(S, D, filter)]
        win = RO.windows(S, D, filter)
        for i in range(D):
            j0, j1 = win[i]
            m0, m1 = win[D - 1 - i]
            assert (m0, m1) == (S - 1 - j1, S - 1 - j0), (S, D, i)
            k = j1 - j0 + 1
            assert (w[i, :k] == w[D - 1 - i, :k][::-1]).all(), (S, D, i)
            assert (w[i, k:] == 0).all()


@pytest.mark.parametrize("filter", FILTER_NAMES)
def test_rows_sum_to_one(tables, filter):
    for S, D in AXES:
        n, _, w = tables[(S, D, filter)]
        assert np.abs(w.astype(np.float64).sum(axis=1) - 1.0).max() <= n * 2.0 ** -24, (S, D)


def test_the_tap_cap(host):
    lib = host.load_library()
    n = ctypes.c_int(-7)
    assert lib.rt_resample_taps(650, 10, L.RESAMPLE_LANCZOS3, ctypes.byref(n), None, None, 0) == TOO_LARGE
    assert lib.rt_resample_taps(130, 2, L.RESAMPLE_AREA, ctypes.byref(n), None, None, 0) == TOO_LARGE
    assert n.value == -7                                       # a refused call writes nothing
    assert RO.taps(650, 10, "lanczos3") is None and RO.taps(130, 2, "area") is None
    n64, first, w = host.resample_taps(640, 64, "lanczos3")     # the widest legal Lanczos window
    assert n64 <= L.RESAMPLE_MAX_TAPS == RO.MAX_TAPS == 64 and n64 == RO.taps(640, 64, "lanczos3")[0] >= 59
    assert host.resample_taps(128, 2, "area")[0] == 64
    with pytest.raises(host.RtError) as e:
        host.resample_taps(650, 10, "lanczos3")
    assert e.value.code == TOO_LARGE


def test_refusals(host):
    lib = host.load_library()
    n = ctypes.c_int(-7)
    first, w = (ctypes.c_int32 * 8)(*([77] * 8)), (ctypes.c_float * 64)(*([77.0] * 64))
    for S, D, f in [(8, 4, 3), (8, 4, -1), (0, 4, 0), (8, 0, 0), (-3, 4, 1), (8, -1, 2)]:
        assert lib.rt_resample_taps(S, D, f, ctypes.byref(n), None, None, 0) == INVALID, (S, D, f)
        assert lib.rt_resample_taps(S, D, f, ctypes.byref(n), first, w, 64) == INVALID, (S, D, f)
    assert lib.rt_resample_taps(8, 4, 0, None, None, None, 0) == INVALID
    assert lib.rt_resample_taps(8, 4, 0, ctypes.byref(n), first, None, 64) == INVALID           # one table without the other
    assert lib.rt_resample_taps(8, 4, 0, ctypes.byref(n), None, w, 64) == INVALID
    assert lib.rt_resample_taps(8, 4, 2, ctypes.byref(n), first, w, 4 * 12 - 1) == TOO_LARGE     # weights too short for D * n
    assert lib.rt_resample_taps(1 << 21, 1 << 21, 0, ctypes.byref(n), None, None, 0) == TOO_LARGE
    assert n.value == -7 and list(first) == [77] * 8 and list(w) == [77.0] * 64
    assert lib.rt_resample_taps(8, 4, 2, ctypes.byref(n), first, w, 4 * 12) == 0 and n.value == 12


def test_resample_desc_layout(tmp_path):
    """rt_resample_desc is 32 bytes with the header's field order, in C (the header's own static assert compiles) and in ctypes."""
    assert ctypes.sizeof(L.RtResampleDesc) == 32
    exp = dict(srcWidth=0, srcHeight=4, dstWidth=8, dstHeight=12, filter=16, flags=20, reserved=24)
    for k, v in exp.items():
        assert getattr(L.RtResampleDesc, k).offset == v, k
    header = open(os.path.join(REPO, "include", "rt_mi355.h")).read()
    assert "sizeof(rt_resample_desc) == 32" in header
    src = tmp_path / "r.c"
    src.write_text('#include "rt_mi355.h"\n'
                   "int main(void){ rt_resample_desc d = {0}; d.filter = RT_RESAMPLE_LANCZOS3; d.reserved[1] = 0;\n"
                   " return sizeof d == 32 && d.filter == 2 && RT_RESAMPLE_AREA == 0 && RT_RESAMPLE_TRIANGLE == 1\n"
                   "        && RT_RESAMPLE_MAX_TAPS == 64 ? 0 : 1; }\n")
    exe = tmp_path / "r"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_make_resample_desc():
    d = L.make_resample_desc(3840, 2160, 1920, 1080)
    assert (d.srcWidth, d.srcHeight, d.dstWidth, d.dstHeight, d.filter, d.flags) == (3840, 2160, 1920, 1080, L.RESAMPLE_LANCZOS3, 0)
    assert list(d.reserved) == [0, 0]
    assert [L.make_resample_desc(1, 1, 1, 1, f).filter for f in FILTER_NAMES] == [0, 1, 2]


def test_the_oracle_on_a_case_done_by_hand():
    """4 -> 2 AREA is the mean of pixel pairs; 2 -> 4 TRIANGLE is the 3/4, 1/4 blend with replicated edges."""
    src = np.zeros((1, 4, 4), dtype=np.float32)
    src[0, :, 0] = (1, 3, 10, 20)
    one = RO.taps(1, 1, "area")
    assert RO.resample(src, RO.taps(4, 2, "area"), one)[0, :, 0].tolist() == [2.0, 15.0]
    got = RO.resample(src[:, :2], RO.taps(2, 4, "triangle"), one)[0, :, 0]
    assert got.tolist() == [1.0, 1.5, 2.5, 3.0]
