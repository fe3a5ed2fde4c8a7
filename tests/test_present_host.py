"""CPU-only tests of the display path's host side: the sRGB decision thresholds rt_display_pack's RT_DISPLAY_RGBA8_SRGB format
is defined by (include/rt_mi355.h) against the formula in numpy, and the byte layout of rt_display_desc.  No GPU call is made."""
import ctypes
import os
import subprocess

import numpy as np

from opengl_raytracing_amd import layout as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _formula():
    """f((i - 0.5) / 255) for i = 1..255 in double: the sRGB EOTF at the midpoint between codes i - 1 and i."""
    s = (np.arange(1, 256, dtype=np.float64) - 0.5) / 255.0
    return np.where(s <= 0.04045, s / 12.92, ((s + 0.055) / 1.055) ** 2.4)


def test_thresholds_are_strictly_increasing_from_zero(host):
    t = host.display_srgb_thresholds()
    assert t.dtype == np.float32 and t.shape == (256,)
    assert t[0] == 0.0
    assert (np.diff(t.astype(np.float64)) > 0).all()
    assert 0.0 < t[1] and t[255] < 1.0          # code 0 and code 255 both keep a non-empty interval of [0, 1]


def test_thresholds_match_the_formula_within_one_ulp(host):
    t = host.display_srgb_thresholds()[1:]
    want = _formula().astype(np.float32)
    lo, hi = np.nextafter(want, np.float32(0)), np.nextafter(want, np.float32(2))
    bad = np.nonzero((t < lo) | (t > hi))[0] + 1
    assert bad.size == 0, f"thresholds {bad.tolist()} are more than one fp32 ulp from the double formula"


def test_thresholds_refuse_null(host):
    assert host.load_library().rt_display_srgb_thresholds(None) == -1


def test_display_desc_layout(tmp_path):
    """rt_display_desc is 32 bytes with the header's field order, in C (the header's own static assert compiles) and in ctypes."""
    assert ctypes.sizeof(L.RtDisplayDesc) == 32
    exp = dict(width=0, height=4, format=8, flags=12, exposure=16, reserved=20)
    for k, v in exp.items():
        assert getattr(L.RtDisplayDesc, k).offset == v, k
    header = open(os.path.join(REPO, "include", "rt_mi355.h")).read()
    assert "sizeof(rt_display_desc) == 32" in header
    src = tmp_path / "d.c"
    src.write_text('#include "rt_mi355.h"\n'
                   "int main(void){ rt_display_desc d = {0}; d.flags = RT_DISPLAY_FLIP_ROWS; d.format = RT_DISPLAY_RGBA8_SRGB;\n"
                   " return sizeof d == 32 && d.flags == 1u && d.format == 1 ? 0 : 1; }\n")
    exe = tmp_path / "d"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_make_display_desc():
    d = L.make_display_desc(7, 5, "srgb", flip=True, exposure=0.5)
    assert (d.width, d.height, d.format, d.flags, d.exposure) == (7, 5, L.DISPLAY_RGBA8_SRGB, L.DISPLAY_FLIP_ROWS, 0.5)
    assert list(d.reserved) == [0, 0, 0]
    d = L.make_display_desc(7, 5)
    assert (d.format, d.flags, d.exposure) == (L.DISPLAY_RGBA8_LINEAR, 0, 1.0)
