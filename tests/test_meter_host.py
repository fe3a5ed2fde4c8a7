"""CPU-only tests of the metering path's host side (include/rt_mi355.h): the two tables of rt_meter's solve against their formulas,
the byte layouts of rt_meter_desc / rt_meter_state / rt_tone_desc in C and in ctypes, rt_meter_solve_host -- the host instantiation of
csrc/rt_meter.h, the code the device runs -- against the numpy / Python-int restatement of tests/meter_oracle.py on 200 histograms,
and every refusal.  No GPU call is made; all comparisons are exact."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import meter_oracle as MO
from opengl_raytracing_amd import layout as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, TOO_LARGE = -1, -4


@pytest.fixture(scope="module")
def tables(host):
    return host.meter_tables()


# ---- tables -------------------------------------------------------------------------------------------------------------------------
def test_log2_table_matches_the_formula(tables):
    q = tables[1]
    assert q.dtype == np.uint32 and q.shape == (8,)
    want = 65536.0 * np.log2(1.0 + (np.arange(8, dtype=np.float64) + 0.5) / 8.0)
    assert (np.abs(q.astype(np.float64) - np.rint(want)) <= 1).all()
    assert (np.diff(q.astype(np.int64)) > 0).all() and 0 < q[0] and q[7] < 65536


def test_pow2_table_matches_the_formula(tables):
    p = tables[0]
    assert p.dtype == np.float32 and p.shape == (256,)
    assert p[0] == 1.0
    assert (np.diff(p.astype(np.float64)) < 0).all()
    want = np.exp2(-np.arange(256, dtype=np.float64) / 256.0).astype(np.float32)
    lo, hi = np.nextafter(want, np.float32(0)), np.nextafter(want, np.float32(2))
    assert ((p >= lo) & (p <= hi)).all()
    assert p[255] > 0.5


def test_tables_refuse_null(host):
    lib = host.load_library()
    p, q = (ctypes.c_float * 256)(), (ctypes.c_uint32 * 8)()
    assert lib.rt_meter_tables(None, q) == INVALID
    assert lib.rt_meter_tables(p, None) == INVALID
    assert lib.rt_meter_tables(p, q) == 0


# ---- layout -------------------------------------------------------------------------------------------------------------------------
def test_layouts_in_c_and_ctypes(tmp_path):
    assert ctypes.sizeof(L.RtMeterDesc) == 48 and ctypes.sizeof(L.RtToneDesc) == 32 and L.METER_STATE_DTYPE.itemsize == 1088
    for k, v in dict(width=0, height=4, key=8, minExposure=12, maxExposure=16, adapt=20, lowPermille=24, highPermille=28, reserved=32).items():
        assert getattr(L.RtMeterDesc, k).offset == v, k
    for k, v in dict(op=0, white=4, dExposure=8, reserved=16).items():
        assert getattr(L.RtToneDesc, k).offset == v, k
    state = dict(hist=0, nPixels=1024, nNonPositive=1028, nNaN=1032, nInf=1036, minLum=1040, maxLum=1044, nMetered=1048, meanLog2Q16=1052,
                 target=1056, exposure=1060, frames=1064, reserved=1068)
    for k, v in state.items():
        assert L.METER_STATE_DTYPE.fields[k][1] == v, k
    assert L.METER_EXPOSURE_OFFSET == 1060
    checks = " && ".join([f"offsetof(rt_meter_state, {k}) == {v}" for k, v in state.items()] +
                         ["sizeof(rt_meter_state) == 1088", "sizeof(rt_meter_desc) == 48", "sizeof(rt_tone_desc) == 32",
                          "offsetof(rt_meter_desc, highPermille) == 28", "offsetof(rt_tone_desc, dExposure) == 8",
                          "offsetof(rt_tone_desc, reserved) == 16", "RT_METER_EXPOSURE_OFFSET == 1060",
                          "RT_TONE_NONE == 0 && RT_TONE_REINHARD == 1 && RT_TONE_ACES == 2"])
    src = tmp_path / "m.c"
    src.write_text('#include <stddef.h>\n#include "rt_mi355.h"\nint main(void){ return (' + checks + ") ? 0 : 1; }\n")
    exe = tmp_path / "m"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_make_descs():
    d = L.make_meter_desc(7, 5)
    assert (d.width, d.height, d.adapt, d.lowPermille, d.highPermille) == (7, 5, 1.0, 0, 0) and list(d.reserved) == [0] * 4
    assert d.key == np.float32(0.18) and 0 < d.minExposure <= d.maxExposure
    t = L.make_tone_desc()
    assert (t.op, t.dExposure) == (L.TONE_NONE, None) and list(t.reserved) == [0] * 4
    t = L.make_tone_desc("reinhard", 4.0, 4096)
    assert (t.op, t.white, t.dExposure) == (L.TONE_REINHARD, 4.0, 4096)
    assert L.make_tone_desc("aces").op == L.TONE_ACES


# ---- the solve ----------------------------------------------------------------------------------------------------------------------
def _cases():
    """200 (hist, prev_exposure, prev_frames, desc) cases: the named edge cases first, crossed with the descriptor settings the
    definition branches on, then random histograms of every magnitude."""
    rng = np.random.default_rng(20)
    one_bin = lambda b, c: np.bincount([b], weights=[c], minlength=256).astype(np.uint32)
    hists = [np.zeros(256, dtype=np.uint32), one_bin(77, 1), one_bin(0, 230400), one_bin(100, 230400), one_bin(255, 230400),
             one_bin(3, 2 ** 31 - 1), one_bin(200, 2 ** 31 - 1), one_bin(128, 2 ** 31 - 2) + one_bin(255, 1)]
    for k in range(42):
        mag = [1, 3, 100, 2 ** 12, 2 ** 20, 2 ** 23][k % 6]
        h = rng.integers(0, mag + 1, 256).astype(np.uint32)
        if k % 3 == 0:                                      # sparse: most bins empty
            h[rng.uniform(0, 1, 256) < 0.9] = 0
        if k % 7 == 0:                                      # one dominant bin near 2^31 beside the rest
            h[rng.integers(0, 256)] = 2 ** 31 - int(h.sum()) - 1 if h.sum() < 2 ** 30 else h[0]
        hists.append(h)
    permilles = [(0, 0), (0, 999), (999, 0), (499, 500), (10, 10)]
    frames = [0, 1, 2 ** 32 - 1]
    olds = [1.0, 0.37, 5.5, np.nan, 0.0, np.inf, -2.0, 1e-30]
    adapts = [1.0, 0.25, 2.0 ** -20]
    limits = [(2.0 ** -10, 2.0 ** 10), (1e-30, 1e30), (100.0, 200.0), (1e-6, 2e-6), (1.0, 1.0)]
    keys = [0.18, 1.0, 3e38, 1e-38]
    cases = []
    for k in range(200):
        lo, hi = permilles[k % 5]
        mn, mx = limits[(k // 5) % 5]
        cases.append((hists[k % len(hists)], np.float32(olds[(k // 3) % 8]), frames[(k // 2) % 3],
                      dict(key=keys[(k // 25) % 4] if k % 4 == 0 else 0.18, min_exposure=mn, max_exposure=mx, adapt=adapts[(k // 7) % 3],
                           low_permille=lo, high_permille=hi)))
    return cases


def _solve_host(lib, hist, old, frames, desc, extra=None):
    src = np.zeros(1, dtype=L.METER_STATE_DTYPE)
    src["hist"][0], src["exposure"][0], src["frames"][0] = hist, old, frames
    if extra:
        for k, v in extra.items():
            src[k][0] = v
    out = np.full(1, 0xA5, dtype=np.uint8).repeat(1088).view(L.METER_STATE_DTYPE)
    d = L.make_meter_desc(640, 360, **desc)
    rc = lib.rt_meter_solve_host(src.ctypes.data, ctypes.byref(d), out.ctypes.data)
    return rc, src[0], out[0]


def test_solve_host_matches_the_restatement(host, tables):
    lib = host.load_library()
    cases = _cases()
    assert len(cases) == 200
    seen = dict(clamp_lo=0, clamp_hi=0, unclamped=0, empty=0, blend=0, jump=0, saturated=0)
    for k, (hist, old, frames, desc) in enumerate(cases):
        extra = dict(nPixels=12345, nNonPositive=3, nNaN=2, nInf=1, minLum=0.25, maxLum=9.5)
        rc, src, got = _solve_host(lib, hist, old, frames, desc, extra)
        assert rc == 0, k
        want = src.copy()
        s = MO.solve(hist, old, frames, tables, **desc)
        for f in ("nMetered", "meanLog2Q16", "target", "exposure", "frames"):
            want[f] = s[f]
        assert MO.state_bytes(got).tobytes() == MO.state_bytes(want).tobytes(), (k, desc, MO.describe_difference(got, want))
        if s["raw"] is None:
            seen["empty"] += 1
        else:
            seen["clamp_lo"] += bool(s["raw"] < np.float32(desc["min_exposure"]))
            seen["clamp_hi"] += bool(s["raw"] > np.float32(desc["max_exposure"]))
            seen["unclamped"] += bool(s["target"] == s["raw"])
        seen["blend" if (frames and np.isfinite(old) and old > 0 and desc["adapt"] < 1) else "jump"] += 1
        seen["saturated"] += s["frames"] == 2 ** 32 - 1 and frames == 2 ** 32 - 1
    assert all(v > 0 for v in seen.values()), seen          # the cases reach every branch of the definition


def test_solve_host_in_place_and_untrimmed_histogram(host, tables):
    lib = host.load_library()
    rng = np.random.default_rng(21)
    st = np.zeros(1, dtype=L.METER_STATE_DTYPE)
    st["hist"][0] = rng.integers(0, 1000, 256)
    hist = st["hist"][0].copy()
    d = L.make_meter_desc(8, 8, low_permille=100, high_permille=200)
    want = MO.solve(hist, 0.0, 0, tables, low_permille=100, high_permille=200)
    assert lib.rt_meter_solve_host(st.ctypes.data, ctypes.byref(d), st.ctypes.data) == 0
    assert (st["hist"][0] == hist).all()                   # the state keeps the untrimmed histogram
    assert st["nMetered"][0] == want["nMetered"] == int(hist.sum()) - int(hist.sum()) * 100 // 1000 - int(hist.sum()) * 200 // 1000
    assert st["meanLog2Q16"][0] == want["meanLog2Q16"] and st["exposure"][0] == want["exposure"] and st["frames"][0] == 1
    got = host.meter_solve_host(st[0], 8, 8, low_permille=100, high_permille=200, adapt=0.5)      # the wrapper, second frame
    want2 = MO.solve(hist, st["exposure"][0], 1, tables, low_permille=100, high_permille=200, adapt=0.5)
    assert got["exposure"] == want2["exposure"] and got["frames"] == 2


def test_mean_is_the_log2_of_the_geometric_mean_to_within_a_bin(host):
    """The sense of meanLog2Q16 / 65536 - 16, checked loosely on the host: constant luminance 2^k lands within one bin (1/8 octave)."""
    for k in (-10, -1, 0, 3, 12):
        hist = np.zeros(256, dtype=np.uint32)
        hist[MO.bins_of(np.float32([2.0 ** k]))[0]] = 1000
        rc, _, got = _solve_host(host.load_library(), hist, 0.0, 0, dict(min_exposure=1e-30, max_exposure=1e30))
        assert rc == 0
        assert abs(got["meanLog2Q16"] / 65536.0 - 16 - k) <= 1 / 8
        assert abs(np.log2(got["target"] / 0.18) + k) <= 1 / 8 + 1 / 256


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_solve_host_refusals(host):
    lib = host.load_library()
    st = np.zeros(1, dtype=L.METER_STATE_DTYPE)
    st["hist"][0][5] = 10
    out = np.zeros(1, dtype=L.METER_STATE_DTYPE)

    def desc(**kw):
        d = L.make_meter_desc(4, 4)
        for k, v in kw.items():
            if k == "reserved":
                d.reserved[v] = 1
            else:
                setattr(d, k, v)
        return d

    nan, inf = float("nan"), float("inf")
    bad = [desc(width=0), desc(width=-1), desc(height=0), desc(height=-7),
           desc(key=0.0), desc(key=-0.18), desc(key=nan), desc(key=inf),
           desc(minExposure=0.0), desc(minExposure=-1.0), desc(minExposure=nan), desc(maxExposure=inf), desc(maxExposure=nan),
           desc(minExposure=2.0, maxExposure=1.0), desc(minExposure=inf, maxExposure=inf),
           desc(adapt=0.0), desc(adapt=-0.5), desc(adapt=1.0000001), desc(adapt=nan), desc(adapt=inf),
           desc(lowPermille=-1), desc(highPermille=-1), desc(lowPermille=1000), desc(highPermille=1000), desc(lowPermille=500, highPermille=500),
           desc(lowPermille=2 ** 31 - 1, highPermille=2 ** 31 - 1),
           desc(reserved=0), desc(reserved=1), desc(reserved=2), desc(reserved=3)]
    for k, d in enumerate(bad):
        assert lib.rt_meter_solve_host(st.ctypes.data, ctypes.byref(d), out.ctypes.data) == INVALID, k
    assert lib.rt_meter_solve_host(None, ctypes.byref(desc()), out.ctypes.data) == INVALID
    assert lib.rt_meter_solve_host(st.ctypes.data, None, out.ctypes.data) == INVALID
    assert lib.rt_meter_solve_host(st.ctypes.data, ctypes.byref(desc()), None) == INVALID
    assert (out.view(np.uint8) == 0).all()                  # a refused call writes nothing
    big = st.copy()
    big["hist"][0][:] = 2 ** 24                             # 2^32 counts: nMetered would not fit
    assert lib.rt_meter_solve_host(big.ctypes.data, ctypes.byref(desc()), out.ctypes.data) == TOO_LARGE
    for d in (desc(), desc(minExposure=1.0, maxExposure=1.0), desc(adapt=1.0), desc(lowPermille=999), desc(lowPermille=499, highPermille=500)):
        assert lib.rt_meter_solve_host(st.ctypes.data, ctypes.byref(d), out.ctypes.data) == 0
    assert out["frames"][0] == 1 and out["nMetered"][0] >= 1
