"""CPU-only tests of progressive accumulation's host side (include/rt_mi355.h): the byte layouts of rt_accum_desc / rt_accum_state in C
and in ctypes, rt_accum_layout, rt_accum_solve_host -- the host instantiation of csrc/rt_accum_solve.h, the code the device runs --
against the Python-int restatement of tests/accum_oracle.py on structured and random histograms, every refusal the host decides alone,
and the oracle's own recurrence against float64: how far the float32 running mean and M2 stray from the exact ones, and that nothing the
accumulator holds is ever NaN, infinite or a negative M2.  No GPU call is made."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import accum_oracle as AO
from opengl_raytracing_amd import layout as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, TOO_LARGE = -1, -4
F = np.float32


# ---- layout -------------------------------------------------------------------------------------------------------------------------
def test_layouts_in_c_and_ctypes(host, tmp_path):
    assert host.RtAccumDesc is L.RtAccumDesc and host.RtAccumState is L.RtAccumState
    assert ctypes.sizeof(L.RtAccumDesc) == 40 and ctypes.sizeof(L.RtAccumState) == 1024 and L.ACCUM_STATE_DTYPE.itemsize == 1024
    for k, v in dict(width=0, height=4, relError=8, lumFloor=12, minSamples=16, donePermille=20, reserved=24).items():
        assert getattr(L.RtAccumDesc, k).offset == v, k
    state = dict(hist=0, nPixels=512, nUnsampled=516, nConverged=520, nRejected=524, minCount=528, maxCount=532, maxR2Bits=536,
                 medianBin=540, p95Bin=544, done=548, frames=552, reserved=556)
    for k, v in state.items():
        assert L.ACCUM_STATE_DTYPE.fields[k][1] == v, k
        assert getattr(L.RtAccumState, k).offset == v, k
    assert L.ACCUM_DONE_OFFSET == 548
    checks = " && ".join([f"offsetof(rt_accum_state, {k}) == {v}" for k, v in state.items()] +
                         ["sizeof(rt_accum_state) == 1024", "sizeof(rt_accum_desc) == 40", "offsetof(rt_accum_desc, donePermille) == 20",
                          "offsetof(rt_accum_desc, reserved) == 24",
                          "RT_ACCUM_VIEW_RELERR == 0 && RT_ACCUM_VIEW_COUNT == 1 && RT_ACCUM_VIEW_CONVERGED == 2"])
    src = tmp_path / "a.c"
    src.write_text('#include <stddef.h>\n#include "rt_mi355.h"\nint main(void){ return (' + checks + ") ? 0 : 1; }\n")
    exe = tmp_path / "a"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_make_desc():
    d = L.make_accum_desc(7, 5)
    assert (d.width, d.height, d.minSamples, d.donePermille) == (7, 5, 16, 950) and list(d.reserved) == [0] * 4
    assert d.relError == F(0.02) and d.lumFloor == F(2.0 ** -10)
    assert L.ACCUM_VIEWS == dict(relerr=0, count=1, converged=2)


def test_accum_layout(host):
    for w, h in AO.SHAPES + [(3840, 2160), (46340, 46340), (2 ** 31 - 1, 1)]:
        lay = host.accum_layout(w, h)
        assert lay.offset == (0, w * h * 16) and lay.bytes == w * h * 32
    lib = host.load_library()
    off, n = (ctypes.c_size_t * 2)(), ctypes.c_size_t(7)
    assert lib.rt_accum_layout(4, 4, off, None) == 0 and tuple(off) == (0, 256)           # bytes may be NULL
    assert lib.rt_accum_layout(4, 4, None, ctypes.byref(n)) == INVALID
    for w, h in [(0, 4), (4, 0), (-1, 4), (4, -3)]:
        assert lib.rt_accum_layout(w, h, off, ctypes.byref(n)) == INVALID, (w, h)
    for w, h in [(65536, 32768), (2 ** 31 - 1, 2), (2 ** 31 - 1, 2 ** 31 - 1)]:
        assert lib.rt_accum_layout(w, h, off, ctypes.byref(n)) == TOO_LARGE, (w, h)
    assert n.value == 7 and tuple(off) == (0, 256), "a refusal wrote its outputs"


# ---- the solve ----------------------------------------------------------------------------------------------------------------------
def _state(hist, nUnsampled=0, nConverged=0, nPixels=None, frames=0, **other):
    s = np.zeros(1, dtype=L.ACCUM_STATE_DTYPE)[0]
    s["hist"] = hist
    n = int(np.asarray(hist, dtype=np.uint64).sum()) + nUnsampled
    s["nUnsampled"], s["nConverged"], s["frames"] = nUnsampled, nConverged, frames
    s["nPixels"] = n if nPixels is None else nPixels
    for k, v in other.items():
        s[k] = v
    return s


def _hist(**bins):
    h = np.zeros(128, dtype=np.uint32)
    for k, v in bins.items():
        h[int(k[1:])] = v
    return h


def _check_solve(host, s, done_permille=950):
    got = host.accum_solve_host(s, 4, 4, done_permille=done_permille)
    want = s.copy()
    for k, v in AO.solve(s["hist"], s["nConverged"], s["nPixels"], done_permille, s["frames"]).items():
        want[k] = v
    want["reserved"] = 0
    assert AO.state_bytes(got).tobytes() == AO.state_bytes(want).tobytes(), AO.describe_difference(got, want)
    return got


def test_solve_on_structured_histograms(host):
    big = 2 ** 32 - 1
    cases = [
        (_state(_hist()), (0, 0)),                                                     # empty
        (_state(_hist(), nUnsampled=9), (0, 0)),
        (_state(_hist(b0=1)), (0, 0)),
        (_state(_hist(b5=1)), (5, 5)),                                                 # one bin
        (_state(_hist(b5=1000), nConverged=1000), (5, 5)),
        (_state(_hist(b127=77)), (127, 127)),                                          # all in bin 127
        (_state(_hist(b0=1, b127=1)), (0, 127)),                                       # ranks 1 and 2
        (_state(_hist(b3=50, b9=45, b64=5)), (3, 9)),                                  # ranks 50 and 95: reached exactly
        (_state(_hist(b3=49, b9=45, b64=6)), (9, 64)),                                 # both ranks fall one pixel behind a bin's end
        (_state(_hist(b3=49, b9=45, b64=6, b100=900)), (100, 100)),
        (_state(_hist(b3=big)), (3, 3)),                                               # counts near 2^32
        (_state(_hist(b3=2 ** 31, b90=2 ** 31 - 1)), (3, 90)),
        (_state(_hist(b0=2 ** 31 - 1, b1=2 ** 31)), (1, 1)),
        (_state(_hist(b10=big - 5), nUnsampled=5), (10, 10)),
        (_state(_hist(b126=2 ** 30, b127=2 ** 30, b1=2 ** 30, b0=2 ** 30 - 1)), (126, 127)),
    ]
    for s, (median, p95) in cases:
        got = _check_solve(host, s)
        assert (int(got["medianBin"]), int(got["p95Bin"])) == (median, p95)
        assert got["frames"] == 1


def test_solve_done_and_frames(host):
    h = _hist(b7=1000)
    for conv, permille, done in [(950, 950, 1), (949, 950, 0), (1000, 1000, 1), (999, 1000, 0), (1, 1, 1), (0, 1, 0)]:
        got = _check_solve(host, _state(h, nConverged=conv), done_permille=permille)
        assert got["done"] == done, (conv, permille)
    # 64-bit products: nConverged * 1000 and nPixels * donePermille both pass 2^32
    big = _hist(b7=2 ** 32 - 1)
    assert _check_solve(host, _state(big, nConverged=2 ** 32 - 1), 1000)["done"] == 1
    assert _check_solve(host, _state(big, nConverged=2 ** 32 - 2), 1000)["done"] == 0
    assert _check_solve(host, _state(big, nConverged=4080218931), 950)["done"] == 1      # ceil((2^32 - 1) * 0.95)
    assert _check_solve(host, _state(big, nConverged=4080218930), 950)["done"] == 0
    for frames, nxt in [(0, 1), (41, 42), (2 ** 32 - 2, 2 ** 32 - 1), (2 ** 32 - 1, 2 ** 32 - 1)]:
        assert _check_solve(host, _state(h, frames=frames))["frames"] == nxt
    # the other words are copied, the reserved ones zeroed; in place works too
    s = _state(h, nRejected=3, minCount=2, maxCount=9, maxR2Bits=0x3f800000, medianBin=99, p95Bin=99, done=7)
    s["reserved"] = 5
    got = _check_solve(host, s)
    assert (got["nRejected"], got["minCount"], got["maxCount"], got["maxR2Bits"]) == (3, 2, 9, 0x3f800000) and not got["reserved"].any()
    lib = host.load_library()
    buf = np.ascontiguousarray(s.reshape(1))
    d = L.make_accum_desc(4, 4)
    assert lib.rt_accum_solve_host(buf.ctypes.data, ctypes.byref(d), buf.ctypes.data) == 0
    assert AO.state_bytes(buf[0]).tobytes() == AO.state_bytes(got).tobytes()


def test_solve_on_random_histograms(host):
    rng = np.random.default_rng(2024)
    for k in range(200):
        nb = int(rng.integers(1, 129))
        h = np.zeros(128, dtype=np.uint32)
        h[rng.choice(128, nb, replace=False)] = rng.integers(0, [4, 1000, 2 ** 24][k % 3], nb)
        n = int(h.sum())
        s = _state(h, nUnsampled=int(rng.integers(0, 50)), nConverged=int(rng.integers(0, n + 1)), frames=k)
        _check_solve(host, s, done_permille=int(rng.integers(1, 1001)))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_host_side_refusals(host):
    lib, vp = host.load_library(), ctypes.c_void_p
    s = np.ascontiguousarray(_state(_hist(b4=10)).reshape(1))
    out = np.zeros(1, dtype=L.ACCUM_STATE_DTYPE)

    def desc(**kw):
        d = L.make_accum_desc(4, 4)
        for k, v in kw.items():
            if k == "reserved":
                d.reserved[v] = 1
            else:
                setattr(d, k, v)
        return d

    def solve(src, d, dst):
        return lib.rt_accum_solve_host(vp(src), ctypes.byref(d) if d is not None else None, vp(dst))

    nan, inf = float("nan"), float("inf")
    assert solve(s.ctypes.data, desc(), out.ctypes.data) == 0
    bad = [desc(width=0), desc(width=-2), desc(height=0), desc(height=-1), desc(relError=0.0), desc(relError=-0.02), desc(relError=nan),
           desc(relError=inf), desc(lumFloor=0.0), desc(lumFloor=2.0 ** -41), desc(lumFloor=-1.0), desc(lumFloor=nan), desc(lumFloor=inf),
           desc(minSamples=1), desc(minSamples=0), desc(minSamples=-5), desc(donePermille=0), desc(donePermille=1001), desc(donePermille=-1),
           desc(reserved=0), desc(reserved=1), desc(reserved=2), desc(reserved=3), None]
    for k, d in enumerate(bad):
        out[:] = 0
        assert solve(s.ctypes.data, d, out.ctypes.data) == INVALID, k
        assert not out.view(np.uint8).any(), "a refusal wrote its output"
    for d in (desc(lumFloor=2.0 ** -40), desc(minSamples=2), desc(donePermille=1), desc(donePermille=1000), desc(relError=1e-30)):
        assert solve(s.ctypes.data, d, out.ctypes.data) == 0                              # the edges of the allowed ranges
    assert solve(None, desc(), out.ctypes.data) == INVALID
    assert solve(s.ctypes.data, desc(), None) == INVALID
    # sum(hist) + nUnsampled: 2^32 - 1 passes, 2^32 does not
    edge = np.ascontiguousarray(_state(_hist(b4=2 ** 32 - 2), nUnsampled=1, nPixels=2 ** 32 - 1).reshape(1))
    assert solve(edge.ctypes.data, desc(), out.ctypes.data) == 0
    for h, u in [(_hist(b4=2 ** 32 - 2), 2), (_hist(b4=2 ** 32 - 1, b5=1), 0), (_hist(b0=2 ** 31, b127=2 ** 31), 0)]:
        over = np.ascontiguousarray(_state(h, nUnsampled=u, nPixels=1).reshape(1))
        assert solve(over.ctypes.data, desc(), out.ctypes.data) == TOO_LARGE
    # the entry points that need a context refuse a NULL one before they touch anything
    d = desc()
    assert lib.rt_accum_add(None, vp(16), vp(32), ctypes.byref(d), vp(64), None) == INVALID
    assert lib.rt_accum_view(None, vp(16), vp(32), ctypes.byref(d), 0, None) == INVALID
    assert lib.rt_accum_reset(None, vp(16), vp(32), 4, 4, None) == INVALID


# ---- the recurrence against float64 -------------------------------------------------------------------------------------------------
def _run(frames):
    h, w = frames[0].shape[:2]
    acc = AO.empty(w, h)
    for x in frames:
        acc, rejected = AO.add(acc, x)
        assert np.isfinite(acc[..., :2]).all() and np.isfinite(acc[0]).all(), "a NaN or an infinity in the accumulator"
        assert (acc[1, ..., 1] >= 0).all() and not np.signbit(acc[1, ..., 1]).any(), "negative M2"
        assert not acc[1, ..., 3].any()
    return acc


@pytest.mark.parametrize("N", [2, 17, 256])
def test_oracle_against_float64(N):
    """Positive log-normal radiance times gamma noise, 1024 pixels.  The running mean in float32 does one rounded subtract, divide and
    add per sample: its error grows like a random walk of N steps of half an ulp, and 4 * sqrt(N) ulps bounds what the recurrence
    was measured to do (1.5 / 4.3 / 17 ulps at N = 2 / 17 / 256).  M2 / (N - 1) against the float64 sample variance of the float32
    luminances: 1e-4 relative (measured worst case 9e-5, at N = 2, where the variance is one rounded difference squared)."""
    rng = np.random.default_rng(1)
    h, w = 16, 64
    base = np.exp2(rng.normal(0, 4, (h, w, 4)))
    frames = [(base * rng.gamma(2.0, 0.5, (h, w, 4))).astype(np.float32) for _ in range(N)]
    acc = _run(frames)
    assert (AO.counts(acc) == N).all()
    ref = np.mean(np.stack(frames).astype(np.float64), axis=0)
    rel = np.abs(acc[0].astype(np.float64) - ref) / np.abs(ref)
    bound = 4.0 * np.sqrt(N) * 2.0 ** -24
    print(f"N={N}: mean error {rel.max() / 2.0 ** -24:.2f} ulps (bound {bound / 2.0 ** -24:.1f})")
    assert rel.max() <= bound
    Y = np.stack([AO.luminance(x) for x in frames]).astype(np.float64)
    var = Y.var(axis=0, ddof=1)
    relv = np.abs(acc[1, ..., 1].astype(np.float64) / (N - 1) - var) / var
    print(f"N={N}: variance error {relv.max():.3g} relative (bound 1e-4)")
    assert relv.max() <= 1e-4
    mY = Y.mean(axis=0)
    assert (np.abs(acc[1, ..., 0].astype(np.float64) - mY) / mY).max() <= bound


def test_oracle_state_stays_finite_on_signed_and_extreme_data():
    rng = np.random.default_rng(3)
    signed = [(rng.normal(0, 1, (8, 8, 4)) * 100 + 1).astype(np.float32) for _ in range(64)]
    acc = _run(signed)
    assert (acc[1, ..., 0] < 0).any() and (acc[1, ..., 0] > 0).any()
    # +-2^48 in every channel, alternating and in runs: the largest |mean|, dY and M2 the bound allows
    big = F(2.0 ** 48)
    pattern = rng.choice([big, -big], (96, 4, 4, 4)).astype(np.float32)
    pattern[:32:2], pattern[1:32:2] = big, -big
    acc = _run(list(pattern))
    assert acc[1, ..., 1].max() > 2.0 ** 100 and (np.abs(acc[0]) <= big).all()
    j = AO.judge(acc)
    assert not np.isnan(j["r2"]).any() and (j["r2"] > 0).all() and (j["bin"] == 127).any()
    # planted specials: rejected samples change nothing, the counts diverge
    frames = AO.noisy_frames(rng, AO.base_image(rng, 67, 9), 17)
    acc = _run(frames)
    c = AO.counts(acc)
    assert c.max() == 17 and c.min() < 17
    # denormal samples only: M2 underflows to +0, never below
    tiny = [np.full((2, 2, 4), v, dtype=np.float32) for v in (1e-40, -1e-40, 1.4e-45, 0.0, -0.0, 1e-39)]
    acc = _run(tiny)
    assert (AO.counts(acc) == 6).all()


def test_oracle_rejects_and_saturates():
    acc = AO.empty(4, 2)
    x = np.ones((2, 4, 4), dtype=np.float32)
    acc, rej = AO.add(acc, x)
    assert not rej.any() and (AO.counts(acc) == 1).all() and (acc[0] == 1).all() and (acc[1, ..., :2] == [1, 0]).all()
    AO.set_counts(acc, np.array([[True, False, False, False], [False, False, False, True]]), [2 ** 24 - 1, 2 ** 24])
    bad = x.copy()
    bad[0, 1, 3] = np.nan                                   # alpha counts too
    bad[0, 2, 0] = np.nextafter(F(2.0 ** 48), F(np.inf))
    bad[0, 3, 1] = -2.0 ** 48                               # exactly at the bound: accepted
    before = acc.copy()
    acc, rej = AO.add(acc, bad)
    assert rej.tolist() == [[False, True, True, False], [False, False, False, True]]
    assert acc[:, rej].tobytes() == before[:, rej].tobytes()
    assert AO.counts(acc).tolist() == [[2 ** 24, 1, 1, 2], [2, 2, 2, 2 ** 24]]
    j = AO.judge(acc, min_samples=2)
    assert j["sampled"].tolist() == [[True, False, False, True], [True, True, True, True]]
    assert j["bin"][1, 1] == 0 and j["converged"][1, 1] and not j["converged"][0, 3]
