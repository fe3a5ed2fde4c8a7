"""Reprojection on the GPU (include/rt_mi355.h): both planes of the accumulator rt_accum_reproject writes and its whole report, bit for
bit, against the numpy restatement of tests/reproject_oracle.py -- over shapes from one pixel to a second row of workgroups, on hits
and accumulators written by hand: points placed with the projection's inverse so that g lands exactly on pixel centres, halfway
between them, within a pixel outside every border, at -1 and at W exactly and far outside; positions behind a camera, at denormal
and overflowing depths, NaN and infinite; object blocks, single-pixel objects and checkerboards; normals parallel, turned to both
sides of normalCosMin, antiparallel, zero, denormal and huge; plane distances on both sides of planeTol * t and exactly at it;
counts from 0 to 2^24 around maxHistory; M2 = 0 and means at +-2^48 -- run to run, behind the renderer on a caller's stream feeding
rt_accum_add, rt_denoise, rt_meter and rt_display_pack_toned with no host synchronisation in between; then every refusal.  Every
comparison is exact equality; guard bytes around every buffer the call writes stay untouched."""
import ctypes

import numpy as np
import pytest

import accum_oracle as AO
import denoise_oracle as DO
import meter_oracle as MO
import reproject_oracle as RO
from opengl_raytracing_amd import layout as L
from test_accum import Guarded, same_bits, up

pytestmark = pytest.mark.gpu

INVALID, TOO_LARGE = -1, -4
F = np.float32
SHAPES = [(1, 1), (3, 1), (5, 3), (67, 9), (257, 3), (130, 70)]
# (normalCosMin, planeTol, maxHistory) of the four variants; the last one runs on identical views
RULES = [dict(normal_cos_min=0.9, plane_tol=2.0 ** -6, max_history=32), dict(normal_cos_min=0.0, plane_tol=0.0, max_history=5),
         dict(normal_cos_min=-1.0, plane_tol=2.0 ** -6, max_history=1), dict(normal_cos_min=0.9, plane_tol=2.0 ** -6, max_history=2 ** 24 - 1)]
DEPTH = 4.0                                                     # of the previous view's surface, the plane z = -4
MOVE = (0.25, -0.125, 0.5)                                      # of the current camera: right, down and BACK, so that m depends on X and Y


@pytest.fixture(scope="module")
def rt(host):
    t = host.RayTracer(0)
    yield t
    t.close()


class Device:
    """Guarded output accumulator and report of one shape; run() is rt_accum_reproject and reads both back."""

    def __init__(self, w, h):
        self.w, self.h = w, h
        self.accum = Guarded(w * h * 32)
        self.report = Guarded(64)

    def run(self, rt, acc_prev, hits_prev, hits_cur, prev, cur, stream=None, **rule):
        rt.reproject(up(acc_prev), up(hits_prev.view(np.uint8)), up(hits_cur.view(np.uint8)), self.accum.t, self.report.t, prev, cur,
                     stream=stream, **rule)
        return self.read()

    def read(self):
        return self.accum.read().view(np.float32).reshape(2, self.h, self.w, 4), self.report.read().view(L.REPROJECT_REPORT_DTYPE)[0]


def check_accum(got, want, what=""):
    if not same_bits(got, want):
        bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)).any(axis=(0, 3)))
        y, x = bad[0]
        raise AssertionError((what, f"{len(bad)} pixels differ; first ({x}, {y}): got {got[:, y, x]!r} want {want[:, y, x]!r}"))


def check_report(got, want, what=""):
    assert same_bits(RO.report_bytes(got), RO.report_bytes(want)), (what, RO.describe_difference(got, want))
    assert int(got["nReused"]) + int(got["nRejected"]) + int(got["nOffscreen"]) + int(got["nMiss"]) == int(got["nPixels"])


# ---- inputs written by hand ---------------------------------------------------------------------------------------------------------
def views(w, h, same):
    """Axis-aligned views (every dot product with the basis is exact): the previous one at the origin looking down -z, the current one
    moved by MOVE."""
    prev = L.make_params(w, h, 3)
    return prev, (prev if same else L.make_params(w, h, 3, cam_pos=MOVE))


def targets(w, rng, n):
    """n wanted coordinates of g along an axis of w pixels: ordinary ones (a centre plus a fraction) and, every fourth, a special one."""
    k = rng.integers(0, w, n).astype(np.float64)
    special = np.array([0.0, 0.5, -0.5, -0.25, -1.0 + 2.0 ** -10, w - 1.0, w - 0.5, w - 0.25, -1.0, float(w), w - 2.0 ** -10, -1000.0, w + 1000.0,
                        2.0 ** 24, -2.0 ** 24, 2.0 ** 31, -2.0 ** 31, 1.0, 1.5])
    t = k + rng.uniform(0, 1, n)
    pick = np.arange(n) % 4 == 1
    t[pick] = np.resize(special, n)[pick]
    t[np.arange(n) % 4 == 2] = (k + np.resize([0.0, 0.5], n))[np.arange(n) % 4 == 2]       # exactly a centre, exactly halfway
    return t


def place(prev, cur, tx, ty):
    """World positions on the plane z = -DEPTH whose motion puts g at (tx, ty) ([h, w] float64): the projection's inverse for the two
    axis-aligned views in float64, then a search of up to +-96 ulp in X and in Y for the float32 position whose g -- by the oracle's
    own float32 projection -- is the wanted value exactly.  Where none is (or the value is not a float32 below 2^20), the nearest
    stays."""
    h, w = tx.shape
    sx, sy = (np.float64(v) for v in RO.view_scale(prev))
    kx, ky = 0.5 * w / sx, 0.5 * h / sy
    zp, zc = DEPTH, DEPTH + MOVE[2]
    px, py = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    inv = 1.0 / zp - 1.0 / zc
    X = (((tx - px) / kx - MOVE[0] / zc) / inv).astype(np.float32)
    Y = (((ty - py) / ky - MOVE[1] / zc) / inv).astype(np.float32)
    P = np.stack([X, Y, np.full((h, w), -DEPTH, dtype=np.float32)], axis=-1)
    steps = np.arange(-96, 97)
    for axis, want in ((0, tx), (1, ty)):
        cand = P[..., axis][..., None] + steps * np.spacing(np.abs(P[..., axis]))[..., None]
        Pc = np.repeat(P[:, :, None, :], len(steps), axis=2)
        Pc[..., axis] = cand.astype(np.float32)
        pf = RO.project(prev, Pc)[axis]
        cf = RO.project(cur, Pc)[axis]
        with np.errstate(all="ignore"):
            g = (px if axis == 0 else py).astype(np.float32)[..., None] + (pf - cf)
        exact = g == want.astype(np.float32)[..., None]
        best = np.where(exact.any(axis=-1), exact.argmax(axis=-1), len(steps) // 2)
        P[..., axis] = np.take_along_axis(Pc[..., axis], best[..., None], axis=-1)[..., 0]
    return P


# positions that are no point of any surface: (x, y, z) with the previous camera at the origin looking down -z
STRANGE = [(0.0, 0.0, 0.0), (1.0, 1.0, 0.0), (0.5, 0.5, 1.0), (0.3, 0.2, 0.25), (0.3, 0.2, -0.25), (0.0, 0.0, -1e-40), (1.0, 0.0, -1e-40),
           (100.0, -100.0, -1e-37), (0.0, 0.0, -1.5e-45), (np.nan, 0.0, -4.0), (0.0, np.nan, -4.0), (0.0, 0.0, np.nan), (np.inf, 0.0, -4.0),
           (0.0, -np.inf, -4.0), (0.0, 0.0, -np.inf), (0.0, 0.0, np.inf), (3e38, 3e38, -4.0), (1e30, 0.0, -1e30)]
NORMALS = [(0, 0, 1), (0, 0, 3), (0, 0, 1), (0.4358, 0, 0.9), (0, 0.436, 0.9), (0, 0, -1), (0, 0, 0), (0, 0, 1e-40), (0, 0, 1e30), (0, 0, 1),
           (1, 0, 0), (0, 0, 2.0 ** -70), (0, 0, 2.0 ** 63)]


def planted(w, h, variant):
    """Everything one call takes, written by hand -> (prev, cur, acc_prev, hits_prev, hits_cur, rule)."""
    rng = np.random.default_rng(1000 * w + 10 * h + variant)
    rule = RULES[variant]
    prev, cur = views(w, h, same=variant == 3)
    n = w * h
    tol = F(rule["plane_tol"]) * F(DEPTH + MOVE[2])
    # the previous view: the plane z = -DEPTH seen through the pixel centres, pushed off the plane by both sides of the tolerance
    px, py = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    hits_prev = RO.empty_hits(w, h)
    hits_prev["position"] = RO.unproject(prev, px, py, np.full((h, w), DEPTH))
    up1, dn1 = np.nextafter(tol, F(np.inf)), np.nextafter(tol, F(0))
    offs = np.array([0, 0, 0, tol, -tol, up1, -up1, dn1, -dn1, 2 * tol, -2 * tol, 0, 0], dtype=np.float32)
    hits_prev["position"][..., 2] = F(-DEPTH) + np.resize(offs, n).reshape(h, w)[:, ::-1]
    hits_prev["t"] = F(DEPTH)
    hits_prev["normal"] = np.resize(np.array(NORMALS, dtype=np.float32), (n + 5, 3))[5:].reshape(h, w, 3)
    obj = [(px.astype(int) // 4 + py.astype(int) // 2) % 3, (px.astype(int) + py.astype(int)) & 1,
           ((px.astype(int) >> 1) + (py.astype(int) >> 1)) & 1, np.zeros((h, w), dtype=int)][variant].astype(np.int32)
    lone = rng.uniform(0, 1, (h, w)) < 0.04                     # single-pixel objects
    obj[lone] = 100 + np.arange(int(lone.sum()))
    obj[rng.uniform(0, 1, (h, w)) < 0.03] = -1                  # and holes of sky in the previous view
    hits_prev["object"] = obj
    mh = rule["max_history"]
    count = np.resize(np.array([7, 0, 1, 2, max(mh - 1, 1), mh, mh + 1, 2 ** 24, 3, 19, 12], dtype=np.uint32), n).reshape(h, w)
    acc = RO.random_accum(rng, w, h, count)
    flat = acc.reshape(2, n, 4)
    flat[1, 3::17, 1] = 0.0                                     # M2 = 0
    big = np.arange(n)[5::23][(count.reshape(-1) != 0)[5::23]]
    flat[0, big] = np.resize(np.array([2.0 ** 48, -2.0 ** 48], dtype=np.float32), (len(big), 4))
    flat[1, big, 0] = 2.0 ** 48
    flat[1, big, 1] = flat[1, big, 1] * F(2.0 ** 90)
    # the current view
    hits_cur = RO.empty_hits(w, h)
    if variant == 3:
        P = RO.unproject(cur, px + rng.uniform(-1, 1, (h, w)), py + rng.uniform(-1, 1, (h, w)), np.full((h, w), DEPTH))
        P[..., 2] = -DEPTH
        tx, ty = px, py
    else:
        tx, ty = targets(w, rng, n).reshape(h, w), targets(h, rng, n)[::-1].reshape(h, w)
        corners = np.arange(n)[np.arange(n) % 9 == (6 + variant) % 9][:8]       # footprints that stick out over each corner
        tx.reshape(n)[corners] = np.resize([-0.5, w - 0.5, -0.25, w - 0.75], len(corners))
        ty.reshape(n)[corners] = np.resize([-0.5, -0.25, h - 0.5, h - 0.75], len(corners))
        P = place(prev, cur, tx, ty)
    strange = np.arange(n) % 9 == (4 + variant) % 9
    P.reshape(n, 3)[strange] = np.resize(np.roll(np.array(STRANGE, dtype=np.float32), -5 * variant, axis=0), (int(strange.sum()), 3))
    hits_cur["position"] = P
    hits_cur["t"] = F(DEPTH + MOVE[2])
    hits_cur["t"].reshape(n)[7::31] = np.resize(np.array([0.0, np.inf, np.nan, -1.0], dtype=np.float32), len(range(7, n, 31)))
    hits_cur["normal"] = (0.0, 0.0, 2.0)
    hits_cur["normal"].reshape(n, 3)[2::13] = np.resize(np.array([(0, 0, 0), (0.1, 0, 1), (0, 0, -1), (0, 0, 1e-30)], dtype=np.float32), (len(range(2, n, 13)), 3))
    # the object of the previous pixel g points at, most of the time; another one, or sky, otherwise
    with np.errstate(all="ignore"):
        qx = np.clip(np.nan_to_num(np.floor(tx + 0.5), nan=0, posinf=w, neginf=-1), 0, w - 1).astype(int)
        qy = np.clip(np.nan_to_num(np.floor(ty + 0.5), nan=0, posinf=h, neginf=-1), 0, h - 1).astype(int)
    oc = np.where(obj[qy, qx] >= 0, obj[qy, qx], 0)
    roll = rng.uniform(0, 1, (h, w))
    oc = np.where(roll < 0.1, oc + 1, np.where(roll < 0.18, -1, oc))
    hits_cur["object"] = oc
    return prev, cur, acc, hits_prev, hits_cur, rule


def run_case(rt, w, h, variant):
    prev, cur, acc, hits_prev, hits_cur, rule = planted(w, h, variant)
    want = RO.reproject(acc, hits_prev, hits_cur, prev, cur, **rule)
    dev = Device(w, h)
    got_acc, got_rep = dev.run(rt, acc, hits_prev, hits_cur, prev, cur, **rule)
    check_accum(got_acc, want["acc"], (w, h, variant))
    check_report(got_rep, want["report"], (w, h, variant))
    return want, rule, (prev, cur, acc, hits_prev, hits_cur)


# ---- 1. parity over shapes and rules ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", range(4))
@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_matches_numpy(rt, w, h, variant):
    want, rule, _ = run_case(rt, w, h, variant)
    check_coverage(want, rule, w, h, variant)


def check_coverage(want, rule, w, h, variant):
    """The planted cases are the cases they claim to be (asked of the oracle's result, from 600 pixels on)."""
    rep, cat, (gx, gy) = want["report"], want["cat"], want["g"]
    n = RO.counts(want["acc"])
    assert np.isfinite(want["acc"]).all() and n.max() <= rule["max_history"]
    if w * h < 600:
        return
    assert min(int(rep["nReused"]), int(rep["nRejected"]), int(rep["nOffscreen"]), int(rep["nMiss"])) > 0, rep
    kept = want["kept"]
    if variant == 3:                                            # identical views: g is the pixel, one tap of weight 1
        moved = (cat == RO.REUSED) | (cat == RO.REJECTED)
        assert (gx == np.arange(w, dtype=np.float32)[None, :])[moved].all() and not kept[1:].any()
        assert rep["maxCount"] == 2 ** 24 - 1 and rep["minCount"] == 1
        return
    moved = (cat == RO.REUSED) | (cat == RO.REJECTED)
    fx, fy = np.where(moved, gx, 0.25), np.where(moved, gy, 0.25)
    on_centre = (fx == np.floor(fx)) & (fy == np.floor(fy))
    assert on_centre.sum() >= 3 and (fx - np.floor(fx) == 0.5).sum() >= 3 and (fy - np.floor(fy) == 0.5).sum() >= 3
    assert ((gx == -1) & (cat == RO.OFFSCREEN)).any() and ((gx == w) & (cat == RO.OFFSCREEN)).any()
    assert ((gy == -1) & (cat == RO.OFFSCREEN)).any() and ((gy == h) & (cat == RO.OFFSCREEN)).any()
    for lo, hi, size, g in ((-1, 0, w, gx), (w - 1, w, w, gx), (-1, 0, h, gy), (h - 1, h, h, gy)):
        assert (moved & (g > lo) & (g < hi)).any(), "no footprint sticks out over this border"
    assert (moved & (gx < 0) & (gy < 0)).any() or (moved & (gx > w - 1) & (gy > h - 1)).any() or (moved & (gx < 0) & (gy > h - 1)).any() \
        or (moved & (gx > w - 1) & (gy < 0)).any(), "no footprint sticks out over a corner"
    assert (np.abs(gx) >= 2.0 ** 24).any() and (np.abs(gx) >= 2.0 ** 31).any() and np.isnan(gx).any() and np.isinf(gx).any()
    per_pixel = kept.sum(axis=0)
    assert (per_pixel == 1).any() and (per_pixel == 2).any() and (per_pixel.max() == 4 or w * h < 5000 or variant == 1)        # (a checkerboard of period 1 shares two)
    assert rep["maxCount"] == rule["max_history"] and rep["minCount"] == 1
    assert (np.abs(want["acc"][0]) >= 2.0 ** 47).any(), "no mean near 2^48 was carried over"


def test_plane_distance_exactly_at_the_tolerance(rt):
    """Identical views, one tap: the previous hit lies planeTol * t off the current tangent plane exactly (kept), one float further
    (dropped), one float nearer (kept), on both sides; with planeTol = 0 only a hit in the plane is kept.  Then the normal: turned
    just inside and just outside normalCosMin."""
    w, h = 16, 2
    v = L.make_params(w, h, 3, cam_pos=(0.0, 0.0, 4.0))         # the surface is the plane z = 0: every offset from it is exact
    px, py = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    hits = RO.empty_hits(w, h)
    hits["position"] = RO.unproject(v, px, py, np.full((h, w), 4.0))
    hits["position"][..., 2] = 0.0
    hits["t"], hits["normal"], hits["object"] = 8.0, (0.0, 0.0, 5.0), 3
    acc = RO.random_accum(np.random.default_rng(4), w, h, 6)
    tol = F(2.0 ** -6) * F(8.0)
    up1, dn1 = np.nextafter(tol, F(1)), np.nextafter(tol, F(0))
    offs = np.array([0, tol, -tol, up1, -up1, dn1, -dn1, 2.0 ** -149, -2.0 ** -149, 1.0, 0, 0, 0, 0, 0, 0], dtype=np.float32)
    prev = hits.copy()
    prev["position"][0, :, 2] = offs
    cosines = np.array([1.0, 0.9 + 1e-3, 0.9 - 1e-3, 0.9 + 1e-6, 0.9 - 1e-6, 0.0, -0.9, -1.0] * 2)
    prev["normal"][1, :, 2] = cosines
    prev["normal"][1, :, 0] = np.sqrt(1 - cosines ** 2)
    dev = Device(w, h)
    for tolk, keep_row0 in ((2.0 ** -6, [1, 1, 1, 0, 0, 1, 1, 1, 1, 0] + [1] * 6), (0.0, [1] + [0] * 9 + [1] * 6)):
        rule = dict(normal_cos_min=0.9, plane_tol=tolk, max_history=32)
        want = RO.reproject(acc, prev, hits, v, v, **rule)
        assert (want["cat"][0] == RO.REUSED).astype(int).tolist() == keep_row0
        assert (want["cat"][1] == RO.REUSED).astype(int).tolist() == [1, 1, 0, 1, 0, 0, 0, 0] * 2
        got_acc, got_rep = dev.run(rt, acc, prev, hits, v, v, **rule)
        check_accum(got_acc, want["acc"], tolk)
        check_report(got_rep, want["report"], tolk)
        assert same_bits(got_acc[0][want["cat"] == RO.REUSED], acc[0][want["cat"] == RO.REUSED])


# ---- 2. determinism -------------------------------------------------------------------------------------------------------------------
def test_same_call_same_bytes(rt):
    w, h = 130, 70
    prev, cur, acc, hits_prev, hits_cur, rule = planted(w, h, 0)
    d_acc, d_hp, d_hc = up(acc), up(hits_prev.view(np.uint8)), up(hits_cur.view(np.uint8))
    runs = []
    for _ in range(3):
        dev = Device(w, h)
        rt.reproject(d_acc, d_hp, d_hc, dev.accum.t, dev.report.t, prev, cur, **rule)
        runs.append((dev.accum.read().tobytes(), dev.report.read().tobytes()))
    assert runs[0] == runs[1] == runs[2]
    dev = Device(w, h)                                          # the report is cleared by the call itself: a dirty one gives the same bytes
    dev.report.t.fill_(0x5A)
    rt.reproject(d_acc, d_hp, d_hc, dev.accum.t, dev.report.t, prev, cur, **rule)
    assert (dev.accum.read().tobytes(), dev.report.read().tobytes()) == runs[0]


# ---- 3. behind the renderer, on a caller's stream -----------------------------------------------------------------------------------
def test_render_move_reproject_accumulate_denoise_on_a_side_stream(rt, host):
    """The noise-textured scene at 96 x 54.  View A: eight frames rendered and accumulated, its first hits traced.  The camera yaws
    three degrees and moves; view B's hits are traced, rt_accum_reproject carries the accumulator over, four more frames of view B are
    rendered and accumulated on the new accumulator, then denoise_guide, denoise, meter and display_pack -- all on one side stream,
    the host running ahead; the only wait is the one before the read-back.  Every result equals the chain of oracles."""
    import torch
    from opengl_raytracing_amd import scenes
    sc = scenes.make_scene(3, host.generate_aabb)
    w, h, na, nb = 96, 54, 8, 4
    rt.load(sc)
    adesc = dict(rel_error=0.15, lum_floor=2.0 ** -6, min_samples=3, done_permille=400)
    mdesc = dict(key=0.3, low_permille=5, high_permille=5)
    rule = dict(normal_cos_min=0.9, plane_tol=0.02, max_history=6)
    table, tables = host.display_srgb_thresholds(), host.meter_tables()
    front, right, upv = host.camera_vectors(-87.0, -1.0)
    accum_a, state = Guarded(w * h * 32), Guarded(1024)
    dev = Device(w, h)
    guide, scratch, out = Guarded(w * h * 16), Guarded(w * h * 32), Guarded(w * h * 16)
    d_meter, d_packed = Guarded(1088), Guarded(w * h * 4)
    colours = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(na + nb)]
    d_pos = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    d_nrm = torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()

    def view(k, moved):
        sc.frame_count = k
        p = sc.params(width=w, height=h)
        if moved:
            pos = tuple(p.camPos)
            p = L.copy_params(p, camPos=(pos[0] + 0.3, pos[1] + 0.1, pos[2] - 0.2), camDir=front, camRight=right, camUp=upv)
        return p

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for k in range(na):
            rt.render_to(view(k, False), colours[k].data_ptr(), d_pos.data_ptr(), d_nrm.data_ptr(), stream=s.cuda_stream)
            rt.accum_add(colours[k], accum_a.t, state.t, w, h, stream=s, **adesc)
        pa, pb = view(0, False), view(0, True)
        d_hits_a = rt.trace_rays(rt.camera_rays(pa, stream=s), "closest", stream=s)
        d_hits_b = rt.trace_rays(rt.camera_rays(pb, stream=s), "closest", stream=s)
        rt.reproject(accum_a.t, d_hits_a, d_hits_b, dev.accum.t, dev.report.t, pa, pb, stream=s, **rule)
        d_after = dev.accum.t.clone()
        for k in range(na, na + nb):
            rt.render_to(view(k, True), colours[k].data_ptr(), d_pos.data_ptr(), d_nrm.data_ptr(), stream=s.cuda_stream)
            rt.accum_add(colours[k], dev.accum.t, state.t, w, h, stream=s, **adesc)
        rt.denoise_guide(d_hits_b, w, h, out=guide.t, stream=s)
        rt.denoise(rt.accum_mean(dev.accum.t, w, h), rt.accum_moments(dev.accum.t, w, h), guide.t, scratch.t, out.t, w, h, stream=s)
        rt.meter(out.t, d_meter.t, w, h, stream=s, **mdesc)
        rt.display_pack(out.t, d_packed.t, w, h, format="srgb", flip=True, exposure=0.75, stream=s, tone="aces",
                        d_exposure=d_meter.t.data_ptr() + L.METER_EXPOSURE_OFFSET)
    s.synchronize()
    frames = [c.cpu().numpy() for c in colours]
    acc = AO.empty(w, h)
    for k in range(na):
        acc, _ = AO.accumulate(acc, frames[k], k, **adesc)
    check_accum(accum_a.read().view(np.float32).reshape(2, h, w, 4), acc, "view A")
    hits_a = d_hits_a.cpu().numpy().reshape(h, w, 8).view(L.HIT_DTYPE).reshape(h, w)
    hits_b = d_hits_b.cpu().numpy().reshape(h, w, 8).view(L.HIT_DTYPE).reshape(h, w)
    want = RO.reproject(acc, hits_a, hits_b, pa, pb, **rule)
    check_accum(d_after.cpu().numpy().view(np.float32).reshape(2, h, w, 4), want["acc"], "reprojected")
    rep = dev.report.read().view(L.REPROJECT_REPORT_DTYPE)[0]
    check_report(rep, want["report"])
    assert same_bits(RO.report_bytes(host.reproject_report(dev.report.t)), RO.report_bytes(rep))
    assert rep["nReused"] > w * h // 2 and rep["nRejected"] + rep["nOffscreen"] > 0 and rep["maxCount"] == 6
    acc_b = want["acc"]
    for k in range(na, na + nb):
        acc_b, state_want = AO.accumulate(acc_b, frames[k], k, **adesc)
    check_accum(dev.accum.read().view(np.float32).reshape(2, h, w, 4), acc_b, "view B")
    got_state = state.read().view(L.ACCUM_STATE_DTYPE)[0]
    assert same_bits(AO.state_bytes(got_state), AO.state_bytes(state_want)), AO.describe_difference(got_state, state_want)
    n = AO.counts(acc_b)
    assert n.max() == 6 + nb and n.min() == nb and got_state["minCount"] == nb
    gd = DO.guide(hits_b)
    assert same_bits(guide.read().view(L.DENOISE_GUIDE_DTYPE).reshape(h, w), gd)
    dn = DO.denoise(acc_b[0], acc_b[1], gd)
    planes = scratch.read().view(np.float32).reshape(2, h, w, 4)
    assert same_bits(planes[0], dn["A"]) and same_bits(planes[1], dn["B"])
    got_out = out.read().view(np.float32).reshape(h, w, 4)
    assert same_bits(got_out, dn["out"]) and np.isfinite(got_out).all()
    want_meter = MO.meter(dn["out"], np.zeros(1, dtype=L.METER_STATE_DTYPE)[0], tables, **mdesc)
    got_meter = d_meter.read().view(L.METER_STATE_DTYPE)[0]
    assert same_bits(MO.state_bytes(got_meter), MO.state_bytes(want_meter)), MO.describe_difference(got_meter, want_meter)
    got = d_packed.read().reshape(h, w, 4)
    assert (got == MO.pack_toned(dn["out"], "srgb", True, 0.75, table, "aces", dev_exposure=want_meter["exposure"])).all()
    assert len(np.unique(got[..., :3])) > 32


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(rt):
    import torch
    w, h = 8, 4
    prev, cur, acc, hits_prev, hits_cur, rule = planted(w, h, 0)
    want = RO.reproject(acc, hits_prev, hits_cur, prev, cur, **rule)
    d_acc, d_hp, d_hc = up(acc), up(hits_prev.view(np.uint8)), up(hits_cur.view(np.uint8))
    dev = Device(w, h)
    lib, ctx, vp = rt.lib, rt.ctx, ctypes.c_void_p

    def desc(**kw):
        d = L.make_reproject_desc(prev, cur, **rule)
        for k, v in kw.items():
            if k == "reserved":
                d.reserved[v] = 1
            elif k in ("prev", "cur"):
                setattr(d, k, L.copy_params(getattr(d, k), **v))
            else:
                setattr(d, k, v)
        return d

    def call(ap, hp, hc, ac, d, rep, c=ctx):
        return lib.rt_accum_reproject(c, vp(ap), vp(hp), vp(hc), vp(ac), ctypes.byref(d) if d is not None else None, vp(rep), None)

    ap, hp, hc, ac, rp = d_acc.data_ptr(), d_hp.data_ptr(), d_hc.data_ptr(), dev.accum.t.data_ptr(), dev.report.t.data_ptr()

    def still_works():
        dev.accum.t.fill_(0x77)
        torch.cuda.synchronize()
        assert call(ap, hp, hc, ac, desc(), rp) == 0
        rt.sync()
        got_acc, got_rep = dev.read()
        check_accum(got_acc, want["acc"])
        check_report(got_rep, want["report"])

    still_works()
    nan, inf = float("nan"), float("inf")
    bad = [None, desc(width=0), desc(width=-2), desc(height=0), desc(height=-1), desc(prev=dict(width=w + 1)), desc(cur=dict(height=h - 1)),
           desc(width=w + 1), desc(prev=dict(fovDeg=0.0)), desc(cur=dict(fovDeg=180.0)), desc(prev=dict(fovDeg=nan)), desc(cur=dict(fovDeg=-30.0)),
           desc(prev=dict(focalLength=0.0)), desc(cur=dict(focalLength=inf)), desc(cur=dict(focalLength=nan)), desc(prev=dict(focalLength=-1.0)),
           desc(normalCosMin=nan), desc(normalCosMin=1.0001), desc(normalCosMin=-1.0001), desc(normalCosMin=inf), desc(planeTol=-1e-6),
           desc(planeTol=nan), desc(planeTol=inf), desc(maxHistory=0), desc(maxHistory=-1), desc(maxHistory=2 ** 24), desc(reserved=0),
           desc(reserved=1), desc(reserved=2)]
    for k, d in enumerate(bad):
        assert call(ap, hp, hc, ac, d, rp) == INVALID, k
    for ok in (desc(normalCosMin=1.0), desc(normalCosMin=-1.0), desc(planeTol=0.0), desc(maxHistory=1), desc(maxHistory=2 ** 24 - 1)):
        assert call(ap, hp, hc, ac, ok, rp) == 0
    still_works()
    nb = w * h * 32
    for args in [(None, hp, hc, ac, rp), (ap, None, hc, ac, rp), (ap, hp, None, ac, rp), (ap, hp, hc, None, rp), (ap, hp, hc, ac, None),
                 (ap + 4, hp, hc, ac, rp), (ap, hp + 8, hc, ac, rp), (ap, hp, hc + 4, ac, rp), (ap, hp, hc, ac + 8, rp), (ap, hp, hc, ac, rp + 4),
                 (ap, hp, hc, ap, rp), (ap, hp, hc, hp, rp), (ap, hp, hc, hc, rp), (ap, hp, hc, ap + nb - 16, rp), (ap, hp, hc, ac, ap),
                 (ap, hp, hc, ac, hp + 16), (ap, hp, hc, ac, hc + nb - 16), (ap, hp, hc, ac, ac), (ap, hp, hc, ac, ac + nb - 16)]:
        assert call(args[0], args[1], args[2], args[3], desc(), args[4]) == INVALID, args
    assert call(ap, hp, hp, ac, desc(), rp) == 0                # the inputs may overlap each other
    still_works()
    assert call(ap, hp, hc, ac, desc(), rp, c=None) == INVALID
    huge = desc(width=65536, height=32768, prev=dict(width=65536, height=32768), cur=dict(width=65536, height=32768))      # 2^31 pixels
    assert call(ap, hp, hc, ac, huge, rp) == TOO_LARGE
    still_works()
    torch.cuda.synchronize()
