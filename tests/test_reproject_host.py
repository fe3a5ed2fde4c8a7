"""CPU-only tests of reprojection's host side (include/rt_mi355.h): the byte layouts of rt_reproject_desc and rt_reproject_report in C and
in ctypes, rt_reproject_layout, every refusal the host decides alone, rt_reproject_project against the oracle's projection bit for
bit -- and the properties of tests/reproject_oracle.py, which is the feature's reference: identical views return the accumulator, a
sideways move over a fronto-parallel plane interpolates a linear ramp exactly, history never crosses a disocclusion edge, the report
agrees with the output plane, and a reprojected history beats a reset.  No GPU call is made."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import accum_oracle as AO
import reproject_oracle as RO
from opengl_raytracing_amd import layout as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, TOO_LARGE = -1, -4
F = np.float32
W, H = 64, 48


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---- layout -------------------------------------------------------------------------------------------------------------------------
def test_layouts_in_c_and_ctypes(host, tmp_path):
    desc = dict(width=0, height=4, prev=8, cur=136, normalCosMin=264, planeTol=268, maxHistory=272, reserved=276)
    rep = dict(nPixels=0, nReused=4, nRejected=8, nOffscreen=12, nMiss=16, minCount=20, maxCount=24, reserved0=28, sumCount=32, reserved=40)
    assert ctypes.sizeof(L.RtReprojectDesc) == 288 and ctypes.sizeof(L.RtReprojectReport) == 64 == L.REPROJECT_REPORT_DTYPE.itemsize
    for k, v in desc.items():
        assert getattr(L.RtReprojectDesc, k).offset == v, k
    for k, v in rep.items():
        assert getattr(L.RtReprojectReport, k).offset == v == L.REPROJECT_REPORT_DTYPE.fields[k][1], k
    checks = " && ".join([f"offsetof(rt_reproject_desc, {k}) == {v}" for k, v in desc.items()] +
                         [f"offsetof(rt_reproject_report, {k}) == {v}" for k, v in rep.items()] +
                         ["sizeof(rt_reproject_desc) == 288", "sizeof(rt_reproject_report) == 64", "sizeof(rt_params) == 128"])
    src = tmp_path / "a.c"
    src.write_text('#include <stddef.h>\n#include "rt_mi355.h"\nint main(void){ return (' + checks + ") ? 0 : 1; }\n")
    exe = tmp_path / "a"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_make_desc(host):
    a, b = RO.make_view(7, 5), RO.make_view(7, 5, pos=(1.0, 2.0, 3.0), yaw=-80.0)
    d = L.make_reproject_desc(a, b)
    assert (d.width, d.height, d.maxHistory) == (7, 5, 32) and list(d.reserved) == [0] * 3
    assert d.normalCosMin == F(0.9) and d.planeTol == F(0.01) and bytes(d.prev) == bytes(a) and bytes(d.cur) == bytes(b)
    assert L.REPROJECT_DEFAULTS == RO.DEFAULTS == dict(normal_cos_min=0.9, plane_tol=0.01, max_history=32)


def test_reproject_layout(host):
    for w, h in [(1, 1), (5, 3), (1920, 1080), (3840, 2160), (46340, 46340), (2 ** 31 - 1, 1)]:
        lay = host.reproject_layout(w, h)
        assert lay.offset == (0, w * h * 16) and lay.bytes == w * h * 32 and tuple(lay) == tuple(host.accum_layout(w, h))
    lib = host.load_library()
    off, n = (ctypes.c_size_t * 2)(), ctypes.c_size_t(7)
    assert lib.rt_reproject_layout(4, 4, off, None) == 0 and tuple(off) == (0, 256)       # bytes may be NULL
    assert lib.rt_reproject_layout(4, 4, None, ctypes.byref(n)) == INVALID
    for w, h in [(0, 4), (4, 0), (-1, 4), (4, -3)]:
        assert lib.rt_reproject_layout(w, h, off, ctypes.byref(n)) == INVALID, (w, h)
    for w, h in [(65536, 32768), (2 ** 31 - 1, 2), (2 ** 31 - 1, 2 ** 31 - 1)]:
        assert lib.rt_reproject_layout(w, h, off, ctypes.byref(n)) == TOO_LARGE, (w, h)
    assert n.value == 7 and tuple(off) == (0, 256), "a refusal wrote its outputs"
    with pytest.raises(host.RtError):
        host.reproject_layout(0, 1)
    assert host.RayTracer.reproject_layout(4, 4).bytes == 512


def test_host_side_refusals(host):
    """rt_accum_reproject refuses a NULL context before it touches anything; rt_reproject_project needs none and refuses NULL
    pointers and every view the device call would refuse."""
    lib, vp = host.load_library(), ctypes.c_void_p
    v = RO.make_view(4, 4)
    d = L.make_reproject_desc(v, v)
    assert lib.rt_accum_reproject(None, vp(16), vp(1024), vp(2048), vp(4096), ctypes.byref(d), vp(8192), None) == INVALID
    assert lib.rt_accum_reproject(None, vp(16), vp(1024), vp(2048), vp(4096), None, vp(8192), None) == INVALID
    P3, f, ok = (ctypes.c_float * 3)(0, 0, -1), (ctypes.c_float * 2)(7, 7), ctypes.c_int(7)
    project = lib.rt_reproject_project
    assert project(ctypes.byref(v), P3, f, ctypes.byref(ok)) == 0 and ok.value == 1
    f[0] = f[1] = 7
    ok.value = 7
    assert project(None, P3, f, ctypes.byref(ok)) == INVALID and project(ctypes.byref(v), None, f, ctypes.byref(ok)) == INVALID
    assert project(ctypes.byref(v), P3, None, ctypes.byref(ok)) == INVALID and project(ctypes.byref(v), P3, f, None) == INVALID
    nan, inf = float("nan"), float("inf")
    bad = [dict(width=0), dict(height=0), dict(width=-3), dict(fovDeg=0.0), dict(fovDeg=-45.0), dict(fovDeg=180.0), dict(fovDeg=nan),
           dict(fovDeg=inf), dict(focalLength=0.0), dict(focalLength=-1.0), dict(focalLength=nan), dict(focalLength=inf),
           dict(focalLength=3e38, fovDeg=170.0)]
    for kw in bad:
        q = L.copy_params(v, **kw)
        assert project(ctypes.byref(q), P3, f, ctypes.byref(ok)) == INVALID, kw
    assert (f[0], f[1], ok.value) == (7, 7, 7), "a refusal wrote its outputs"
    with pytest.raises(host.RtError):
        host.reproject_project(L.copy_params(v, fovDeg=0.0), (0, 0, -1))


# ---- the projection -----------------------------------------------------------------------------------------------------------------
VIEWS = [dict(), dict(pos=(3.0, -2.0, 7.0), yaw=-70.0, pitch=12.0), dict(pos=(-20.0, 5.0, 1.5), yaw=135.0, pitch=-30.0, fov=60.0),
         dict(pos=(0.5, 0.25, -0.125), yaw=10.0, pitch=45.0, fov=20.0)]


@pytest.mark.parametrize("k", range(len(VIEWS)))
def test_projection_round_trip(host, k):
    """Points camPos + t * (camDir + ux * right + uy * up) at the pixel centres of a 64 x 48 view, depths between 0.5 and 20 so that
    every coordinate stays below 64: rt_reproject_project equals the oracle's projection bit for bit, and f lies within 2^-10 px of
    the centre (fp32 rounding of coordinates below 64 moves f by 2^-17 px per ulp at these scales; the four views measure up to
    2^-13.6 px, printed below)."""
    v = RO.make_view(W, H, **VIEWS[k])
    px, py = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    t = np.random.default_rng(k).uniform(0.5, 20.0, (H, W))
    P = RO.unproject(v, px, py, t)
    assert np.abs(P).max() < 64
    fx, fy, valid = RO.project(v, P)
    assert valid.all()
    got = np.zeros((H, W, 2), dtype=np.float32)
    for y in range(H):
        for x in range(W):
            f, ok = host.reproject_project(v, P[y, x])
            assert ok
            got[y, x] = f
    assert same_bits(got[..., 0], fx) and same_bits(got[..., 1], fy)
    err = max(float(np.abs(got[..., 0] - px).max()), float(np.abs(got[..., 1] - py).max()))
    print(f"view {k}: largest distance from the pixel centre {err:.3g} px")
    assert err <= 2.0 ** -10
    # behind the camera, and NaN: invalid, in the oracle and in the library alike
    for point in [RO.unproject(v, 3.0, 4.0, -2.0), np.array([np.nan, 0, 0], dtype=np.float32), np.array(list(v.camPos), dtype=np.float32)]:
        f, ok = host.reproject_project(v, point)
        ofx, ofy, ovalid = RO.project(v, point)
        assert not ok and not ovalid and same_bits(F(f[0]), ofx) and same_bits(F(f[1]), ofy)


# ---- the oracle's properties ----------------------------------------------------------------------------------------------------------
def _jitter(rng, w, h):
    """Ray offsets of up to a pixel either way in x and y (rt_camera_rays' own jitter is up to a pixel)."""
    return rng.uniform(-1.0, 1.0, (h, w, 2))


def test_identical_views_return_the_accumulator(host):
    rng = np.random.default_rng(1)
    v = RO.make_view(W, H, pos=(0.3, -0.2, 1.0), yaw=-85.0, pitch=4.0)
    hits = RO.trace_plane_and_sphere(v, -6.0, ((0.4, -0.1, -4.0), 1.0), jitter=_jitter(rng, W, H))
    hits["object"][:3, :5] = -1                                  # a patch of sky
    count = rng.integers(1, 41, (H, W)).astype(np.uint32)
    count[10, :8] = [1, 2, 31, 32, 33, 2 ** 24 - 1, 2 ** 24, 40]
    acc = RO.random_accum(rng, W, H, count)
    r = RO.reproject(acc, hits, hits, v, v, max_history=32)
    hit = hits["object"] >= 0
    assert (r["cat"][hit] == RO.REUSED).all() and (r["cat"][~hit] == RO.MISS).all() and (~hit).sum() == 15
    assert (r["g"][0] == np.arange(W, dtype=np.float32)[None, :]).all() and (r["g"][1] == np.arange(H, dtype=np.float32)[:, None]).all()
    assert r["kept"][0][hit].all() and not r["kept"][1:].any()
    out = r["acc"]
    assert same_bits(out[0][hit], acc[0][hit]) and same_bits(out[1, ..., 0][hit], acc[1, ..., 0][hit])
    assert not out[:, ~hit].any()
    n = RO.counts(out)
    assert (n[hit] == np.minimum(count, 32)[hit]).all() and (count > 32).sum() > 100 and n[10, :8].tolist() == [1, 2, 31, 32, 32, 32, 32, 32]
    # M2' = (M2 / (n - 1)) * (n' - 1): two roundings
    exact = acc[1, ..., 1].astype(np.float64) / np.maximum(count.astype(np.float64) - 1, 1) * (n.astype(np.float64) - 1)
    ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    assert (np.abs(out[1, ..., 1].astype(np.float64) - exact)[hit] <= 2 * ulp[hit]).all()
    same = hit & (count <= 32)
    ulp_in = np.spacing(acc[1, ..., 1]).astype(np.float64)
    assert (np.abs(out[1, ..., 1].astype(np.float64) - acc[1, ..., 1])[same] <= 2 * ulp_in[same]).all()
    assert (out[1, ..., 1][count == 1] == 0).all() and (out[1, ..., 3] == 0).all()
    check_report(r)


def check_report(r):
    rep, acc, cat = r["report"], r["acc"], r["cat"]
    assert int(rep["nReused"]) + int(rep["nRejected"]) + int(rep["nOffscreen"]) + int(rep["nMiss"]) == int(rep["nPixels"]) == cat.size
    n = RO.counts(acc)
    reused = n > 0
    assert (reused == (cat == RO.REUSED)).all() and int(rep["nReused"]) == int(reused.sum())
    assert not acc[:, ~reused].any()
    if reused.any():
        assert int(rep["sumCount"]) == int(n.astype(np.uint64).sum()) and int(rep["minCount"]) == int(n[reused].min())
        assert int(rep["maxCount"]) == int(n.max())
    else:
        assert int(rep["sumCount"]) == int(rep["maxCount"]) == 0 and int(rep["minCount"]) == 2 ** 32 - 1
    assert int(rep["reserved0"]) == 0 and not rep["reserved"].any()


def ramp(P):
    """Linear in world x and y."""
    return 2.0 + 0.75 * P[..., 0].astype(np.float64) - 0.5 * P[..., 1].astype(np.float64)


def test_sideways_move_over_a_facing_plane_is_exact(host):
    """The plane z = -5 fills both views, the camera moves parallel to it by (2.37, -1.61) pixels, the previous accumulator holds a ramp
    that is linear in world x and y.  Pixel <-> world is affine, so bilinear interpolation is exact up to rounding: every REUSED pixel
    whose footprint lies inside the previous image has the ramp's value at its own hit within 2^-10 of the ramp's range.  A footprint
    that sticks out over the border (-1 < g < 0, W-1 < g < W) is renormalised over the taps inside by the contract, which is the ramp at
    g clamped to the image: those pixels are held to that, with the same bound.  The OFFSCREEN pixels are exactly those whose g
    (in float64, from the shift) falls outside."""
    a = RO.make_view(W, H)
    sx, sy = (np.float64(s) for s in RO.view_scale(a))
    px_world = (2.0 * sx * 5.0 / W, 2.0 * sy * 5.0 / H)           # the size of a pixel on the plane
    shift = (2.37, -1.61)                                          # of g against the pixel, in pixels
    b = RO.make_view(W, H, pos=(shift[0] * px_world[0], shift[1] * px_world[1], 0.0))
    hits_a, hits_b = RO.trace_plane_and_sphere(a, -5.0), RO.trace_plane_and_sphere(b, -5.0)
    assert (hits_a["object"] == 0).all() and (hits_b["object"] == 0).all()
    acc = RO.random_accum(np.random.default_rng(2), W, H, 8)
    values = ramp(hits_a["position"])
    acc[0] = values[..., None].astype(np.float32)
    acc[1, ..., 0] = values.astype(np.float32)
    r = RO.reproject(acc, hits_a, hits_b, a, b)
    px, py = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    gx, gy = px + shift[0], py + shift[1]
    assert np.abs(r["g"][0] - gx).max() < 1e-3 and np.abs(r["g"][1] - gy).max() < 1e-3
    outside = ~((gx > -1) & (gx < W) & (gy > -1) & (gy < H))
    assert ((r["cat"] == RO.OFFSCREEN) == outside).all() and 0 < outside.sum() < W * H // 4
    assert (r["cat"][~outside] == RO.REUSED).all()
    bound = 2.0 ** -10 * (values.max() - values.min())
    full = ~outside & (gx >= 0) & (gx <= W - 1) & (gy >= 0) & (gy <= H - 1)
    partial = ~outside & ~full
    assert full.sum() > W * H // 2 and partial.sum() > 0
    want = ramp(hits_b["position"])
    err = np.abs(r["acc"][0][..., 0].astype(np.float64) - want)
    print(f"largest error over the full footprints {err[full].max():.3g}, bound {bound:.3g}")
    assert err[full].max() <= bound
    assert same_bits(r["acc"][0][..., 0], r["acc"][0][..., 3]) and np.abs(r["acc"][1, ..., 0][full] - want[full]).max() <= bound
    # the ramp at g clamped to the image: g is (cx, cy) pixels of view a, whose pixel (0, 0) looks at hits_a["position"][0, 0]
    cx, cy = np.clip(gx, 0, W - 1), np.clip(gy, 0, H - 1)
    origin = hits_a["position"][0, 0].astype(np.float64)
    clamped = np.stack([origin[0] + cx * px_world[0], origin[1] + cy * px_world[1]], axis=-1)
    assert np.abs(r["acc"][0][..., 0].astype(np.float64) - ramp(clamped))[partial].max() <= bound
    assert (RO.counts(r["acc"])[~outside] == 8).all()
    check_report(r)


class Disocclusion:
    """A sphere of radius 1 at depth 4 in front of the plane z = -8; the camera moves 0.35 to the right, so the sphere moves about four
    pixels to the left over the plane.  Both views' hits are analytic, through jittered pixels."""

    def __init__(self, w=W, h=H, seed=3):
        rng = np.random.default_rng(seed)
        self.w, self.h = w, h
        self.a, self.b = RO.make_view(w, h), RO.make_view(w, h, pos=(0.35, 0.05, 0.0))
        sphere = ((0.2, 0.1, -4.0), 1.0)
        self.hits_a = RO.trace_plane_and_sphere(self.a, -8.0, sphere, jitter=_jitter(rng, w, h))
        self.hits_b = RO.trace_plane_and_sphere(self.b, -8.0, sphere, jitter=_jitter(rng, w, h))
        self.acc = RO.random_accum(rng, w, h, rng.integers(1, 20, (h, w)))
        self.result = RO.reproject(self.acc, self.hits_a, self.hits_b, self.a, self.b)


@pytest.fixture(scope="module")
def dis(host):
    return Disocclusion()


def test_history_does_not_cross_a_disocclusion_edge(dis):
    """Every previous-accumulator value on sphere pixels times 1000: no byte of any output pixel whose current object is the plane
    changes.  And every plane pixel all four of whose taps land on previous sphere pixels is REJECTED and empty."""
    r = dis.result
    was_sphere, is_plane = dis.hits_a["object"] == 1, dis.hits_b["object"] == 0
    assert was_sphere.sum() > 100 and is_plane.sum() > 1000 and (dis.hits_b["object"] == 1).sum() > 100
    acc2 = dis.acc.copy()
    acc2[0][was_sphere] *= F(1000)
    acc2[1, ..., 0][was_sphere] *= F(1000)
    acc2[1, ..., 1][was_sphere] *= F(1000)
    r2 = RO.reproject(acc2, dis.hits_a, dis.hits_b, dis.a, dis.b)
    assert same_bits(r["acc"][:, is_plane], r2["acc"][:, is_plane])
    assert not same_bits(r["acc"][:, ~is_plane], r2["acc"][:, ~is_plane])
    assert (r["cat"] == r2["cat"]).all()
    # plane pixels whose whole footprint lies on the previous sphere
    gx, gy = r["g"]
    inside = (gx >= 0) & (gx <= dis.w - 1) & (gy >= 0) & (gy <= dis.h - 1)
    x0, y0 = np.floor(np.where(inside, gx, 0)).astype(int), np.floor(np.where(inside, gy, 0)).astype(int)
    x1, y1 = np.minimum(x0 + 1, dis.w - 1), np.minimum(y0 + 1, dis.h - 1)
    covered = inside & is_plane & was_sphere[y0, x0] & was_sphere[y0, x1] & was_sphere[y1, x0] & was_sphere[y1, x1]
    assert covered.sum() >= 20
    assert (r["cat"][covered] == RO.REJECTED).all() and not r["acc"][:, covered].any()
    # both outcomes, and nothing reused across the two objects
    assert (r["cat"][is_plane] == RO.REUSED).sum() > 1000
    for k in range(4):
        i, j = k & 1, k >> 1
        kx, ky = np.clip(x0 + i, 0, dis.w - 1), np.clip(y0 + j, 0, dis.h - 1)
        kept = r["kept"][k]
        assert (dis.hits_a["object"][ky, kx][kept] == dis.hits_b["object"][kept]).all()
    check_report(r)


def test_report_agrees_with_the_output(dis):
    rep = dis.result["report"]
    check_report(dis.result)
    assert rep["nReused"] > 0 and rep["nRejected"] > 0 and rep["nOffscreen"] > 0 and rep["nMiss"] == 0
    assert 1 <= rep["minCount"] <= rep["maxCount"] <= 19
    hits = dis.hits_b.copy()
    hits["object"][:4] = -1
    r = RO.reproject(dis.acc, dis.hits_a, hits, dis.a, dis.b, max_history=5)
    check_report(r)
    assert r["report"]["nMiss"] == 4 * dis.w and r["report"]["maxCount"] == 5
    none = RO.reproject(dis.acc, dis.hits_a, RO.empty_hits(dis.w, dis.h), dis.a, dis.b)
    check_report(none)
    assert none["report"]["nMiss"] == dis.w * dis.h


def test_reprojected_history_beats_a_reset(dis):
    """What the feature buys: 16 noisy frames of view A, the move, then ONE new sample of view B.  RMSE against the clean image over
    the REUSED pixels: with the reprojected history in front of the sample, and with a reset.  Only the order is asserted; the factor
    is printed (DESIGN.md 23 quotes it)."""
    rng = np.random.default_rng(9)

    def clean(hits):
        P = hits["position"].astype(np.float64)
        v = np.where(hits["object"] == 1, 3.0, 1.0 + 0.1 * P[..., 0] - 0.05 * P[..., 1])
        return np.repeat(v[..., None], 4, axis=-1)

    def sample(img):
        return (img * rng.gamma(4.0, 0.25, img.shape)).astype(np.float32)          # mean 1, sigma 0.5

    acc = AO.empty(dis.w, dis.h)
    for _ in range(16):
        acc, _ = AO.add(acc, sample(clean(dis.hits_a)))
    r = RO.reproject(acc, dis.hits_a, dis.hits_b, dis.a, dis.b)
    reused = r["cat"] == RO.REUSED
    truth = clean(dis.hits_b)
    new = sample(truth)
    with_history, _ = AO.add(r["acc"], new)
    after_reset, _ = AO.add(AO.empty(dis.w, dis.h), new)

    def rmse(img):
        return float(np.sqrt(np.mean((img[reused][:, :3].astype(np.float64) - truth[reused][:, :3]) ** 2)))
    e_hist, e_reset = rmse(with_history[0]), rmse(after_reset[0])
    print(f"RMSE over {int(reused.sum())} reused pixels: reprojection + 1 sample {e_hist:.4f}, reset + 1 sample {e_reset:.4f}: "
          f"a factor of {e_reset / e_hist:.2f}")
    assert reused.sum() > 1000 and (AO.counts(with_history)[reused] >= 2).all()
    assert e_hist < e_reset
