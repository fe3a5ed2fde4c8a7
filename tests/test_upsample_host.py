"""CPU-only tests of first-hit-guided upsampling's host side (include/rt_mi355.h): rt_upsample_desc in C and in ctypes,
rt_upsample_layout against rt_accum_select_layout, the refusals the host decides alone, that the benchmark tool parses its arguments
without a device -- and the numpy oracle of tests/upsample_oracle.py against the definition's own words: the position rule against
exact fractions, the list's order against adaptive_oracle's, the three stages on inputs small enough to work out by hand.  No GPU call
is made."""
import ctypes
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import adaptive_oracle as DO
import denoise_oracle as NO
import upsample_oracle as UO
from opengl_raytracing_amd import layout as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, TOO_LARGE = -1, -4
F = np.float32


# ---- layouts --------------------------------------------------------------------------------------------------------------------------
def test_upsample_desc_in_c_and_ctypes(host, tmp_path):
    assert ctypes.sizeof(L.RtUpsampleDesc) == 64
    fields = dict(width=0, height=4, lowWidth=8, lowHeight=12, normalLog2Power=16, minWeight=20, reserved=24)
    for k, v in fields.items():
        assert getattr(L.RtUpsampleDesc, k).offset == v, k
    checks = " && ".join([f"offsetof(rt_upsample_desc, {k}) == {v}" for k, v in fields.items()] + ["sizeof(rt_upsample_desc) == 64"])
    src = tmp_path / "a.c"
    src.write_text('#include <stddef.h>\n#include "rt_mi355.h"\nint main(void){ return (' + checks + ") ? 0 : 1; }\n")
    exe = tmp_path / "a"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
    for name in ("rt_upsample_layout", "rt_upsample", "rt_image_put_at"):
        assert name in host.EXPORTS and getattr(host.load_library(), name)
    d = L.make_upsample_desc(7, 5, 3, 2, 6, 0.5)
    assert (d.width, d.height, d.lowWidth, d.lowHeight, d.normalLog2Power, d.minWeight) == (7, 5, 3, 2, 6, 0.5) and not any(d.reserved)


def test_upsample_layout_is_accum_select_layout(host):
    for w, h in [(1, 1), (8, 8), (9, 8), (67, 9), (130, 70), (1920, 1080), (3840, 2160), (46340, 46340), (2 ** 31 - 1, 1), (1, 2 ** 31 - 1)]:
        assert host.upsample_layout(w, h) == host.accum_select_layout(w, h) == host.RayTracer.upsample_layout(w, h), (w, h)
    lib = host.load_library()
    n = ctypes.c_size_t(7)
    assert lib.rt_upsample_layout(4, 4, None) == INVALID
    for w, h in [(0, 4), (4, 0), (-1, 4), (4, -3)]:
        assert lib.rt_upsample_layout(w, h, ctypes.byref(n)) == INVALID, (w, h)
    for w, h in [(65536, 32768), (2 ** 31 - 1, 2)]:
        assert lib.rt_upsample_layout(w, h, ctypes.byref(n)) == TOO_LARGE, (w, h)
    assert n.value == 7, "a refusal wrote its output"


def test_null_context_is_refused(host):
    lib, vp = host.load_library(), ctypes.c_void_p
    d = L.make_upsample_desc(4, 4, 2, 2)
    assert lib.rt_upsample(None, vp(4096), vp(8192), vp(16384), vp(32768), ctypes.byref(d), vp(65536), 4, vp(131072), vp(262144), None) == INVALID
    assert lib.rt_image_put_at(None, vp(4096), vp(8192), 4, vp(16384), 4, 4, None) == INVALID


def test_tool_help_needs_no_device():
    run = subprocess.run([sys.executable, os.path.join(REPO, "tools", "bench_upsample.py"), "--help"], capture_output=True, text=True,
                         env={**os.environ, "HIP_VISIBLE_DEVICES": "-1"})
    assert run.returncode == 0, run.stderr
    for option in ("--out", "--frames", "--repeats", "--parent-lib"):
        assert option in run.stdout


# ---- the position rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("low,high", [(1, 1), (1, 5), (3, 7), (5, 8), (7, 7), (540, 1920)])
def test_position_against_exact_fractions(low, high):
    """The centre of output pixel x lies at (x + 1/2) * low / high - 1/2 in low texel coordinates: ix0 is its floor, fx its fraction,
    exact up to the one rounding of the quotient (the numerator and 2 * high are exact in float32 at these sizes)."""
    i0, f = UO.position(low, high)
    assert i0.dtype == np.int64 and f.dtype == np.float32
    for x in range(high):
        pos = (Fraction(2 * x + 1, 2) * low) / high - Fraction(1, 2)
        fl = pos.numerator // pos.denominator
        assert i0[x] == fl and -1 <= i0[x] <= low - 1, x
        frac = pos - fl
        assert 0 <= frac < 1
        assert 0.0 <= f[x] < 1.0, x
        assert abs(Fraction(float(f[x])) - frac) <= Fraction(1, 2 ** 24), x            # half an ulp below 1
        w0, w1 = F(1.0) - f[x], f[x]
        assert abs(float(w0) + float(w1) - 1.0) <= 2.0 ** -23, x
    assert i0[0] == (-1 if low < high else 0) and i0[-1] == low - 1
    if low == high:
        assert (i0 == np.arange(high)).all() and (f == 0).all()


# ---- the oracle against the definition ------------------------------------------------------------------------------------------------
def _flat(obj, normal=(0.0, 0.0, 1.0)):
    obj = np.asarray(obj, dtype=np.int32)
    n = np.zeros(obj.shape + (3,), dtype=np.float32)
    n[...] = normal
    return NO.make_hits(n, obj)


@pytest.mark.parametrize("shape", UO.SHAPES, ids=UO.shape_id)
def test_list_is_the_holes_in_tile_order(shape):
    (lw, lh), (w, h) = shape
    low, hl, hh = UO.make_case(shape)
    for mw in (0.0, 0.25, 1.0):
        r = UO.upsample(low, hl, hh, 3, mw)
        hole = r["stage"] != UO.INTERPOLATED
        xs, ys = DO.tile_order(w, h)
        want = [(int(x), int(y)) for x, y in zip(xs, ys) if hole[y, x]]
        assert r["full_list"].dtype == np.uint32 and [tuple(p) for p in r["full_list"].tolist()] == want
        st = r["state"]
        assert (int(st["nPixels"]), int(st["nSelected"]), int(st["nListed"]), int(st["capacity"]), int(st["overflow"]), int(st["nCapped"])) == \
            (w * h, len(want), len(want), len(want), 0, int((r["stage"] == UO.ORPHAN).sum()))
        assert not st["reserved"].any()
        assert sum(bin(int(b)).count("1") for b in r["ballots"]) == len(want)
        for x, y in want[:3] + want[-3:]:
            assert (int(r["ballots"][(y // 8) * ((w + 7) // 8) + x // 8]) >> ((y % 8) * 8 + x % 8)) & 1
        for cap in {0, max(len(want) - 1, 0), len(want), len(want) + 7}:
            part = UO.upsample(low, hl, hh, 3, mw, capacity=cap)
            assert part["list"].tolist() == r["full_list"][:cap].tolist()
            ps = part["state"]
            assert (int(ps["nSelected"]), int(ps["nListed"]), int(ps["capacity"]), int(ps["overflow"])) == \
                (len(want), min(cap, len(want)), cap, int(len(want) > cap))
            assert part["out"].tobytes() == r["out"].tobytes()
    if w * h >= 600:                                            # the planted cases are the cases they claim to be
        r = UO.upsample(low, hl, hh, 3, 0.25)
        assert (r["stage"] == UO.INTERPOLATED).sum() > w * h // 2
        assert (r["stage"] == UO.HOLE).any() and (r["stage"] == UO.ORPHAN).any()
        assert (r["stage"][hh["object"] == 9] == UO.ORPHAN).all(), "an object the low plane lacks"
        assert (hh["object"] < 0).any() and not UO.usable(low).all()


def test_ratio_one_reproduces_usable_texels_of_matching_objects():
    shape = ((7, 7), (7, 7))
    low, hl, _ = UO.make_case(shape)
    r = UO.upsample(low, hl, hl, 0, 0.0)
    gd = NO.guide(hl)
    n = gd["n"]
    own = np.where(gd["object"] < 0, F(1), np.minimum((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2], F(1)))
    direct = UO.usable(low) & (own > 0)
    assert direct.any() and (r["stage"][direct] == UO.INTERPOLATED).all() and (r["stage"][~direct] != UO.INTERPOLATED).all()
    with np.errstate(all="ignore"):
        want = (F(0) + own[..., None] * low) / own[..., None]   # (+0 + w*v) / w: the texel up to two roundings, a -0 as +0
    assert r["out"][direct].tobytes() == want[direct].astype(np.float32).tobytes()
    assert np.allclose(r["out"][direct], low[direct], rtol=2.0 ** -22, atol=2.0 ** -148)


def test_three_stages_by_hand():
    """2 x 1 -> 4 x 1.  Output x = 0..3 sits at -1/4, 1/4, 3/4, 5/4 of the low row: taps (-1, 0), (0, 1), (0, 1), (1, 2) with fx = 3/4,
    1/4, 3/4, 1/4; a single row, so iy0 = 0, fy = 0 and only j = 0 carries weight."""
    low = np.array([[[1, 2, 3, 1], [5, 6, 7, 0.5]]], dtype=np.float32)
    hl = _flat([[0, 1]])
    # (a) objects 0 0 1 1: x = 1 keeps tap 0 alone (weight 3/4), x = 2 keeps tap 1 alone (3/4); the ends keep their one inside tap
    r = UO.upsample(low, hl, _flat([[0, 0, 1, 1]]), 2, 0.5)
    assert (r["stage"] == UO.INTERPOLATED).all() and r["sw1"].tolist() == [[0.75, 0.75, 0.75, 0.75]]
    assert r["out"].tolist() == [[[1, 2, 3, 1], [1, 2, 3, 1], [5, 6, 7, 0.5], [5, 6, 7, 0.5]]]
    # (b) minWeight above 3/4: every pixel is a hole, filled from the window by the normal weight alone -- the same values
    r = UO.upsample(low, hl, _flat([[0, 0, 1, 1]]), 2, 0.875)
    assert (r["stage"] == UO.HOLE).all() and r["state"]["nSelected"] == 4 and r["state"]["nCapped"] == 0
    assert r["out"].tolist() == [[[1, 2, 3, 1], [1, 2, 3, 1], [5, 6, 7, 0.5], [5, 6, 7, 0.5]]] and r["ballots"].tolist() == [0b1111]
    # (c) objects 1 0 0 5: x = 0 finds object 1 only in the window (its taps are -1 and 0), x = 3 finds object 5 nowhere and copies low
    #     texel min(3 * 2 / 4, 1) = 1; x = 1 and 2 interpolate with weights 3/4 and 1/4
    r = UO.upsample(low, hl, _flat([[1, 0, 0, 5]]), 2, 0.25)
    assert r["stage"].tolist() == [[UO.HOLE, UO.INTERPOLATED, UO.INTERPOLATED, UO.ORPHAN]]
    assert r["out"].tolist() == [[[5, 6, 7, 0.5], [1, 2, 3, 1], [1, 2, 3, 1], [5, 6, 7, 0.5]]]
    assert r["full_list"].tolist() == [[0, 0], [3, 0]] and r["state"]["nCapped"] == 1 and r["ballots"].tolist() == [0b1001]
    # (d) one object, both taps kept: the bilinear mean; an unusable texel drops out and the other tap takes all the weight
    hh = _flat([[0, 0, 0, 0]])
    r = UO.upsample(low, _flat([[0, 0]]), hh, 0, 0.0)
    assert r["out"][0, 1].tolist() == [2, 3, 4, 0.875] and r["out"][0, 2].tolist() == [4, 5, 6, 0.625]
    bad = low.copy()
    bad[0, 1, 3] = np.inf
    r = UO.upsample(bad, _flat([[0, 0]]), hh, 0, 0.0)
    assert r["out"][0, 1].tolist() == [1, 2, 3, 1] and r["out"][0, 2].tolist() == [1, 2, 3, 1]
    assert r["stage"].tolist() == [[0, 0, 0, UO.HOLE]] and r["out"][0, 3].tolist() == [1, 2, 3, 1]
    # (e) antiparallel normals: the 2 x 2 weight is zero, and so is the window's -- an orphan that copies its texel, unusable or not
    r = UO.upsample(bad, _flat([[0, 0]], (0, 0, -1.0)), hh, 1, 0.0)
    assert (r["stage"] == UO.ORPHAN).all() and r["out"].tobytes() == bad[:, [0, 0, 1, 1]].tobytes()
    # (f) sky takes sky whatever the normals say
    r = UO.upsample(low, _flat([[-1, -1]], (0, 0, 0)), _flat([[-1, -1, -1, -1]], (0, 0, 0)), 7, 1.0)
    assert r["stage"].tolist() == [[UO.HOLE, 0, 0, UO.HOLE]] and r["out"][0, 1].tolist() == [2, 3, 4, 0.875]


def test_image_put_at_oracle():
    img = np.arange(3 * 5 * 4, dtype=np.float32).reshape(3, 5, 4)
    px = np.array([[4, 2], [5, 0], [0, 3], [2 ** 32 - 1, 1], [0, 0]], dtype=np.uint32)
    smp = -np.arange(20, dtype=np.float32).reshape(5, 4) - 1
    out = UO.image_put_at(img, smp, px)
    want = img.copy()
    want[2, 4], want[0, 0] = smp[0], smp[4]
    assert out.tobytes() == want.tobytes()
    assert UO.image_put_at(img, smp[:0], px[:0]).tobytes() == img.tobytes()
