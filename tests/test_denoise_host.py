"""CPU-only tests of the denoiser's host side (include/rt_mi355.h): the byte layouts of rt_denoise_desc and the guide record in C and in
ctypes, rt_denoise_layout, every refusal the host decides alone -- and the properties of tests/denoise_oracle.py, which is the feature's
reference: the filter stops exactly at object edges, reduces the noise of an accumulated image, lowers the variance it carries, fills a
skipped pixel without letting it touch a neighbour, and falls back to the spatial variance estimate below minCount.  No GPU call is made."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import accum_oracle as AO
import denoise_oracle as DO
from opengl_raytracing_amd import layout as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, TOO_LARGE = -1, -4
F = np.float32
W, H, FRAMES = 64, 48, 8


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---- layout -------------------------------------------------------------------------------------------------------------------------
def test_layouts_in_c_and_ctypes(host, tmp_path):
    assert ctypes.sizeof(L.RtDenoiseDesc) == 48 and L.DENOISE_GUIDE_DTYPE.itemsize == 16
    desc = dict(width=0, height=4, iterations=8, normalLog2Power=12, sigmaLum=16, lumEps=20, minCount=24, reserved=28)
    for k, v in desc.items():
        assert getattr(L.RtDenoiseDesc, k).offset == v, k
    assert L.DENOISE_GUIDE_DTYPE.fields["n"][1] == 0 and L.DENOISE_GUIDE_DTYPE.fields["object"][1] == 12
    # the guide record is the upper half of an rt_hit
    assert L.HIT_DTYPE.fields["normal"][1] == 16 and L.HIT_DTYPE.fields["object"][1] == 28
    checks = " && ".join([f"offsetof(rt_denoise_desc, {k}) == {v}" for k, v in desc.items()] +
                         ["sizeof(rt_denoise_desc) == 48", "sizeof(rt_denoise_guide_rec) == 16", "offsetof(rt_denoise_guide_rec, object) == 12",
                          "offsetof(rt_hit, normal) == 16"])
    src = tmp_path / "a.c"
    src.write_text('#include <stddef.h>\n#include "rt_mi355.h"\nint main(void){ return (' + checks + ") ? 0 : 1; }\n")
    exe = tmp_path / "a"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_make_desc():
    d = L.make_denoise_desc(7, 5)
    assert (d.width, d.height, d.iterations, d.normalLog2Power, d.minCount) == (7, 5, 4, 5, 4) and list(d.reserved) == [0] * 5
    assert d.sigmaLum == F(4.0) and d.lumEps == F(2.0 ** -10)
    assert L.DENOISE_DEFAULTS == dict(iterations=4, normal_log2_power=5, sigma_lum=4.0, lum_eps=2.0 ** -10, min_count=4)


def test_denoise_layout(host):
    for w, h in [(1, 1), (5, 3), (1920, 1080), (3840, 2160), (46340, 46340), (2 ** 31 - 1, 1)]:
        lay = host.denoise_layout(w, h)
        assert lay.offset == (0, w * h * 16) and lay.bytes == w * h * 32
    lib = host.load_library()
    off, n = (ctypes.c_size_t * 2)(), ctypes.c_size_t(7)
    assert lib.rt_denoise_layout(4, 4, off, None) == 0 and tuple(off) == (0, 256)         # bytes may be NULL
    assert lib.rt_denoise_layout(4, 4, None, ctypes.byref(n)) == INVALID
    for w, h in [(0, 4), (4, 0), (-1, 4), (4, -3)]:
        assert lib.rt_denoise_layout(w, h, off, ctypes.byref(n)) == INVALID, (w, h)
    for w, h in [(65536, 32768), (2 ** 31 - 1, 2), (2 ** 31 - 1, 2 ** 31 - 1)]:
        assert lib.rt_denoise_layout(w, h, off, ctypes.byref(n)) == TOO_LARGE, (w, h)
    assert n.value == 7 and tuple(off) == (0, 256), "a refusal wrote its outputs"
    assert lib.rt_denoise_layout(4, 4, off, ctypes.byref(n)) == 0 and n.value == 512      # a valid call is still accepted
    with pytest.raises(host.RtError):
        host.denoise_layout(0, 1)


def test_host_side_refusals(host):
    """The entry points that need a context refuse a NULL one before they touch anything."""
    lib, vp = host.load_library(), ctypes.c_void_p
    d = L.make_denoise_desc(4, 4)
    assert lib.rt_denoise(None, vp(16), vp(32), vp(48), vp(64), vp(128), ctypes.byref(d), None) == INVALID
    assert lib.rt_denoise(None, vp(16), None, vp(48), vp(64), vp(128), None, None) == INVALID
    assert lib.rt_denoise_guide(None, vp(16), vp(1024), 4, 4, None) == INVALID
    assert host.denoise_layout(4, 4).bytes == 512


# ---- the guide ----------------------------------------------------------------------------------------------------------------------
def test_guide_oracle():
    normals = np.array([[0, 2, 0], [3, 0, 4], [0, 0, 0], [-0.0, -0.0, -5], [1e-30, 0, 0], [1e30, 1e30, 0], [1e-10, 2e-10, 2e-10]], dtype=np.float32)
    hits = DO.make_hits(normals[None], np.array([[0, 1, -1, 2, 3, 4, 5]], dtype=np.int32), np.random.default_rng(0))
    g = DO.guide(hits)[0]
    assert g["object"].tolist() == [0, 1, -1, 2, 3, 4, 5]
    assert g["n"][0].tolist() == [0, 1, 0] and same_bits(g["n"][1], np.array([F(3) / F(5), 0, F(4) / F(5)], dtype=np.float32))
    assert not g["n"][2].any() and not np.signbit(g["n"][2]).any()           # a miss stays +0
    assert g["n"][3].tolist() == [0, 0, -1]
    assert not g["n"][4].any()                                               # s underflows to 0: no direction
    assert not g["n"][5].any()                                               # s overflows: n / inf = 0
    assert abs(float(np.linalg.norm(g["n"][6].astype(np.float64))) - 1) < 1e-6


# ---- properties of the oracle -------------------------------------------------------------------------------------------------------
class Case:
    """The synthetic case: 64 x 48, two objects split by a slanted edge plus a strip of misses, clean values 0.2 / 3.0 / 1.0, log-normal
    noise with a fixed seed, eight frames through accum_oracle, four iterations with the defaults."""

    def __init__(self):
        self.guide, self.dist = DO.synthetic_guide(W, H)
        self.clean = DO.clean_image(self.guide)
        self.frames = DO.lognormal_frames(np.random.default_rng(2024), self.clean, FRAMES)
        self.acc = self.accumulate(self.frames)
        self.result = DO.denoise(self.acc[0], self.acc[1], self.guide)
        self.far = self.dist >= 16

    @staticmethod
    def accumulate(frames):
        acc = AO.empty(W, H)
        for f in frames:
            acc, rejected = AO.add(acc, f)
        return acc


@pytest.fixture(scope="module")
def case(host):
    return Case()


def test_case_has_what_the_properties_need(case):
    obj = case.guide["object"]
    assert set(np.unique(obj)) == {-1, 0, 1} and (AO.counts(case.acc) == FRAMES).all()
    assert (obj[case.far] == 0).sum() > 100 and (obj[case.far] == 1).sum() > 100
    n1 = case.guide["n"][obj == 1]
    assert np.abs(np.linalg.norm(n1.astype(np.float64), axis=-1) - 1).max() < 1e-6 and np.ptp(n1[:, 0]) > 0.3      # the normal turns


def test_edges_stop_the_filter_exactly(case):
    """Every sample of object 1 times 1000: every byte of every plane and of the output at the pixels of object 0 and of the sky
    stays as it was."""
    obj = case.guide["object"]
    frames = [np.where((obj == 1)[..., None], f * F(1000), f).astype(np.float32) for f in case.frames]
    acc = Case.accumulate(frames)
    other = DO.denoise(acc[0], acc[1], case.guide)
    keep = obj != 1
    assert keep.sum() > 1000 and (obj[keep] == -1).any() and (obj[keep] == 0).any()
    for a, b in zip(case.result["planes"] + [case.result["out"]], other["planes"] + [other["out"]]):
        assert same_bits(a[keep], b[keep])
        assert not same_bits(a[~keep], b[~keep])
    assert np.isfinite(other["out"]).all()


def test_noise_falls(case):
    """RMSE against the clean image over the pixels at least 16 texels from any object edge: the accumulated mean's over the denoised
    image's.  One unweighted 5 x 5 B3 pass alone has sum(h^2) = (70/256)^2 = 0.075, a factor of 3.7, so 2 is a safe floor; the oracle
    reaches 15.5 here (four iterations, eight frames, sigma 0.5 log-normal), and half of that is asserted too."""
    def rmse(img):
        return float(np.sqrt(np.mean((img[case.far][:, :3].astype(np.float64) - case.clean[case.far][:, :3]) ** 2)))
    before, after = rmse(case.acc[0]), rmse(case.result["out"])
    print(f"RMSE of the mean {before:.5f}, denoised {after:.5f}: a factor of {before / after:.2f}")
    assert before / after >= 2.0
    assert before / after >= MEASURED_REDUCTION / 2
    # every iteration helps on its own
    errs = [rmse(p) for p in case.result["planes"]]
    assert all(b < a for a, b in zip(errs, errs[1:])), errs


MEASURED_REDUCTION = 15.5


def test_variance_falls(case):
    vin, vout = case.result["planes"][0][..., 3], case.result["last"][..., 3]
    assert (vin[case.far] > 0).all() and (vout[case.far] >= 0).all()
    assert (vout[case.far] < vin[case.far]).all()
    assert not np.signbit(vout).any() and np.isfinite(vout).all()
    print(f"mean variance {vin[case.far].mean():.4g} -> {vout[case.far].mean():.4g}")


def test_alpha_is_the_image_s(case):
    img = case.acc[0].copy()
    img[..., 3] = np.random.default_rng(5).uniform(0, 1, (H, W)).astype(np.float32)
    r = DO.denoise(img, case.acc[1], case.guide, iterations=2)
    assert same_bits(r["out"][..., 3], img[..., 3]) and same_bits(r["out"][..., :3], DO.denoise(case.acc[0], case.acc[1], case.guide, iterations=2)["out"][..., :3])


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 2.0 ** 49, np.nextafter(F(2.0 ** 48), F(np.inf))])
def test_skipped_pixel_is_filled_and_touches_no_neighbour(case, bad):
    """A planted pixel in each object (one channel bad).  On the noisy case it is filled with a finite value inside the range of its
    object, and nothing else turns non-finite.
    The exact comparison: a noise-free image with a fixed spatial pattern and moments with M2 = 0 (count 8), so that the variance
    plane is zero.  Run A plants the bad value; run B makes the same pixel usable with the value 2^40 in every channel, whose luminance
    lies so far from every neighbour's that exp_ gives the weight 0 in every iteration (wl >= 2^39 / lumEps), and which keeps that
    value (its own tap is the only one with weight).  Then every byte of every OTHER pixel, in the prepared plane, after every iteration
    and in the output, is the same in A and B: a dropped tap and a tap of weight 0 add the same to every sum."""
    obj = case.guide["object"]
    spots = [(30, 10), (20, 50), (2, 30)]                                     # (y, x) in object 0, object 1, the sky
    assert [int(obj[s]) for s in spots] == [0, 1, -1]
    img = case.acc[0].copy()
    for k, s in enumerate(spots):
        img[s][k] = bad
    r = DO.denoise(img, case.acc[1], case.guide)
    assert np.isfinite(r["out"]).all()
    for s in spots:
        mine = case.acc[0][obj == obj[s]][:, :3]
        assert (r["out"][s][:3] >= mine.min()).all() and (r["out"][s][:3] <= mine.max()).all()
        assert all(np.signbit(p[s][3]) and p[s][3] == 0 for p in r["planes"])              # the mark travels: var = -0
    assert sum(np.signbit(p[..., 3]).sum() for p in r["planes"]) == 3 * len(r["planes"])
    # the exact statement
    pattern = np.exp(np.random.default_rng(8).normal(0, 0.3, (H, W, 1))).astype(np.float32)
    base = case.clean.copy()
    base[..., :3] *= pattern
    mom = np.zeros((H, W, 4), dtype=np.float32)
    mom[..., 0] = DO.luminance(base)
    mom[..., 2] = np.full((H, W), FRAMES, dtype=np.uint32).view(np.float32)
    a, b = base.copy(), base.copy()
    for k, s in enumerate(spots):
        a[s][k] = bad
        b[s][:3] = 2.0 ** 40
    ra, rb = DO.denoise(a, mom, case.guide), DO.denoise(b, mom, case.guide)
    others = np.ones((H, W), dtype=bool)
    for s in spots:
        others[s] = False
    for pa, pb in zip(ra["planes"] + [ra["out"]], rb["planes"] + [rb["out"]]):
        assert same_bits(pa[others], pb[others])
    for s in spots:
        assert (rb["out"][s][:3] == F(2.0 ** 40)).all() and np.isfinite(ra["out"][s]).all() and ra["out"][s][0] < 10
    assert not same_bits(ra["planes"][1], ra["planes"][0]), "the filter did nothing"


def test_skipped_pixel_without_neighbours_passes_through(host):
    """A skipped pixel that is alone in its object has no tap: it passes through unchanged, the mark stays."""
    obj = np.zeros((5, 5), dtype=np.int32)
    obj[2, 2] = 7
    n = np.zeros((5, 5, 3), dtype=np.float32)
    n[..., 2] = 1
    img = np.ones((5, 5, 4), dtype=np.float32)
    img[2, 2] = (np.nan, 2.0, np.inf, 0.5)
    r = DO.denoise(img, None, DO.make_guide(n, obj), iterations=3)
    assert same_bits(r["out"][2, 2], img[2, 2])
    assert all(same_bits(p[2, 2], np.array([np.nan, 2.0, np.inf, -0.0], dtype=np.float32)) for p in r["planes"])
    rest = np.ones((5, 5), dtype=bool)
    rest[2, 2] = False
    assert (r["out"][rest] == 1).all()


# ---- the spatial fallback -----------------------------------------------------------------------------------------------------------
def _spatial_by_hand(img, obj, x, y, count):
    """The header's spatial estimate of one pixel in scalar float32 arithmetic, written out."""
    h, w = obj.shape
    sY, sYY, k = F(0), F(0), 0
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            qx, qy = x + dx, y + dy
            if not (0 <= qx < w and 0 <= qy < h) or obj[qy, qx] != obj[y, x]:
                continue
            r, g, b = (F(v) for v in img[qy, qx, :3])
            if not all(abs(v) <= F(2.0 ** 48) for v in (r, g, b)):
                continue
            Y = F(F(F(0.2126) * r) + F(F(0.7152) * g)) + F(F(0.0722) * b)
            sY = F(sY + Y)
            sYY = F(sYY + F(Y * Y))
            k += 1
    m1, m2 = F(sY / F(k)), F(sYY / F(k))
    v = F(m2 - F(m1 * m1))
    return F((v if v > 0 else F(0)) / F(max(count, 1))), k


def test_spatial_fallback_on_a_hand_computed_window(host):
    rng = np.random.default_rng(11)
    img = rng.uniform(0.1, 4.0, (5, 5, 4)).astype(np.float32)
    obj = np.zeros((5, 5), dtype=np.int32)
    obj[0, :3] = 1                                             # three pixels of another object: not in the centre's window sum
    img[3, 3, 1] = np.nan                                      # and one skipped pixel
    n = np.zeros((5, 5, 3), dtype=np.float32)
    n[..., 1] = 1
    gd = DO.make_guide(n, obj)
    # the centre's variance by the textbook formula in float64: what the float32 recurrence must be close to
    Y = DO.luminance(img).astype(np.float64)
    mask = (obj == 0) & DO.usable(img)
    assert mask.sum() == 21
    textbook = Y[mask].var()
    # (a) no moments: every count reads 1
    plane = DO.prepare(img, None, gd, min_count=4)
    want, k = _spatial_by_hand(img, obj, 2, 2, 1)
    assert k == 21 and same_bits(plane[2, 2, 3], want) and abs(float(want) / textbook - 1) < 1e-4
    for (x, y), kk in {(0, 0): 3, (4, 4): 8, (3, 0): 10, (0, 2): 12}.items():
        want, k = _spatial_by_hand(img, obj, x, y, 1)
        assert k == kk and same_bits(plane[y, x, 3], want), (x, y)
    assert np.signbit(plane[3, 3, 3]) and plane[3, 3, 3] == 0 and same_bits(plane[..., :3], img[..., :3])
    # (b) moments with counts on both sides of min_count: below it the spatial estimate over the count, from it on M2 / (n (n - 1))
    mom = np.zeros((5, 5, 4), dtype=np.float32)
    mom[..., 1] = 6.0
    cnt = np.full((5, 5), 3, dtype=np.uint32)
    cnt[2, 2], cnt[2, 3], cnt[1, 1], cnt[1, 2] = 3, 4, 0, 1
    mom[..., 2] = cnt.view(np.float32)
    plane = DO.prepare(img, mom, gd, min_count=4)
    assert same_bits(plane[2, 2, 3], _spatial_by_hand(img, obj, 2, 2, 3)[0])
    assert same_bits(plane[2, 2, 3], F(_spatial_by_hand(img, obj, 2, 2, 1)[0] / F(3)))
    assert plane[2, 3, 3] == F(6.0) / (F(4) * F(3))
    assert same_bits(plane[1, 1, 3], _spatial_by_hand(img, obj, 1, 1, 0)[0]) and same_bits(plane[1, 2, 3], _spatial_by_hand(img, obj, 2, 1, 1)[0])
    plane5 = DO.prepare(img, mom, gd, min_count=5)
    assert same_bits(plane5[2, 3, 3], _spatial_by_hand(img, obj, 3, 2, 4)[0])
    # what the filter then uses: the first iteration's prefiltered variance comes from these values
    r = DO.denoise(img, None, gd, iterations=1)
    assert same_bits(r["planes"][0], DO.prepare(img, None, gd)) and np.isfinite(r["out"]).all()
