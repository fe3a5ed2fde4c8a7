"""First-hit-guided upsampling on the GPU (include/rt_mi355.h): rt_upsample's output, hole list, select state and scratch ballots, and
rt_image_put_at's image, bit for bit, against the numpy restatement of tests/upsample_oracle.py -- on hand-written inputs over ragged
shapes and non-integer ratios, every normalLog2Power, minWeight at 0, 1 and on both sides of a planted weight, every capacity around the
number of holes, run to run over dirty buffers; chained behind the renderer on one caller's stream; then every refusal.  Every
comparison is exact equality; guard bytes around every buffer the calls write stay untouched."""
import ctypes

import numpy as np
import pytest

import upsample_oracle as UO
from opengl_raytracing_amd import layout as L
from test_accum import SENTINEL, Guarded, same_bits, up

pytestmark = pytest.mark.gpu

INVALID, TOO_LARGE = -1, -4
F = np.float32
HEADER = 4096                                                   # the scratch's two runs of 512 totals, in front of the ballots
# normalLog2Power 0..7, each with a minWeight of its own: 0, 1, and values between
COMBOS = [(0, 0.25), (1, 0.0), (2, 1.0), (3, 0.5), (4, 0.75), (5, 2.0 ** -20), (6, 0.25), (7, 0.9375)]


@pytest.fixture(scope="module")
def rt(host):
    t = host.RayTracer(0)
    yield t
    t.close()


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Device:
    """The inputs of one case on the device, and guarded output, list (room for every pixel and eight more), scratch and select state."""

    def __init__(self, host, low, hits_low, hits_high):
        self.lh, self.lw = low.shape[:2]
        self.h, self.w = hits_high.shape
        assert L.HIT_DTYPE.itemsize == 32
        self.low, self.hits_low, self.hits_high = up(as_bytes(low)), up(as_bytes(hits_low)), up(as_bytes(hits_high))
        self.out = Guarded(self.w * self.h * 16)
        self.list = Guarded((self.w * self.h + 8) * 8)
        self.scratch = Guarded(host.upsample_layout(self.w, self.h))
        self.sel = Guarded(64)
        self.tiles = ((self.w + 7) // 8) * ((self.h + 7) // 8)

    def run(self, rt, capacity, power, min_weight, stream=None):
        """One rt_upsample over an output and a list refilled with the guard pattern -> (out [h, w, 4], the whole list buffer as uint32
        rows, the state, the ballots)."""
        self.out.t.fill_(SENTINEL)
        self.list.t.fill_(SENTINEL)
        rt.upsample(self.low, self.hits_low, self.hits_high, self.out.t, self.list.t if capacity else None, capacity, self.scratch.t,
                    self.sel.t, self.w, self.h, self.lw, self.lh, normal_log2_power=power, min_weight=min_weight, stream=stream)
        return (self.out.read().view(np.float32).reshape(self.h, self.w, 4), self.list.read().view(np.uint32).reshape(-1, 2),
                self.sel.read().view(L.SELECT_STATE_DTYPE)[0], self.scratch.read()[HEADER: HEADER + 8 * self.tiles].view(np.uint64))


def first_difference(got, want):
    bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)).any(axis=-1))
    y, x = bad[0]
    return f"{len(bad)} pixels differ; first ({x}, {y}): got {got[y, x]!r} want {want[y, x]!r}"


def check(dev, rt, want, capacity, power, min_weight, what=""):
    """`want`: the oracle's answer without a capacity."""
    got_out, got_list, got_state, got_ballots = dev.run(rt, capacity, power, min_weight)
    n_holes = len(want["full_list"])
    n = min(n_holes, capacity)
    state = want["state"].copy()
    state["nListed"], state["capacity"], state["overflow"] = n, capacity, int(n_holes > capacity)
    what = (what, power, min_weight, capacity)
    assert same_bits(got_out, want["out"]), (what, first_difference(got_out, want["out"]))
    assert same_bits(as_bytes(got_state), as_bytes(state)), (what, got_state, state)
    assert np.array_equal(got_list[:n], want["full_list"][:n]), (what, "the list")
    assert (got_list[n:].view(np.uint8) == SENTINEL).all(), (what, "an entry behind nListed was written")
    assert np.array_equal(got_ballots, want["ballots"]), (what, "the ballots")


def capacities(n):
    return sorted({0, max(n - 1, 0), n, n + 7})


# ---- 1. rt_upsample against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", UO.SHAPES, ids=UO.shape_id)
def test_upsample_matches_oracle(rt, host, shape):
    (lw, lh), (w, h) = shape
    low, hl, hh = UO.make_case(shape)
    dev = Device(host, low, hl, hh)
    stages = set()
    for power, mw in COMBOS:
        want = UO.upsample(low, hl, hh, power, mw)
        n = len(want["full_list"])
        print(f"{UO.shape_id(shape)} power {power} minWeight {mw}: {n} holes of {w * h}, {int(want['state']['nCapped'])} orphans")
        for cap in capacities(n):
            check(dev, rt, want, cap, power, mw)
        stages |= set(np.unique(want["stage"]).tolist())
    if w * h >= 600:
        assert stages == {UO.INTERPOLATED, UO.HOLE, UO.ORPHAN}
    assert same_bits(dev.low.cpu().numpy(), as_bytes(low)) and same_bits(dev.hits_high.cpu().numpy(), as_bytes(hh))


# strips of one pixel's breadth whose position integers leave 32 bits: (2v + 1) * low reaches 2 * high * low -- the last shape below
# 2^32 (4 294 883 880), the first above it (4 295 069 244), and 4.8e9 along x and along y (7500 tiles: every workgroup, several
# chunks each)
STRIPS = [((46340, 1), (46341, 1)), ((46341, 1), (46342, 1)), ((40000, 1), (60000, 1)), ((1, 40000), (1, 60000))]


@pytest.mark.parametrize("shape", STRIPS, ids=UO.shape_id)
def test_position_around_32_bits(rt, host, shape):
    (lw, lh), (w, h) = shape
    assert (max(2 * w * lw, 2 * h * lh) > 2 ** 32) == (shape != STRIPS[0])
    low, hl, hh = UO.make_case(shape)
    dev = Device(host, low, hl, hh)
    stages = set()
    for power, mw in ((5, 0.25), (0, 1.0)):
        want = UO.upsample(low, hl, hh, power, mw)
        n = len(want["full_list"])
        print(f"{UO.shape_id(shape)} power {power} minWeight {mw}: {n} holes of {w * h}, {int(want['state']['nCapped'])} orphans")
        for cap in (n - 1, n):
            check(dev, rt, want, cap, power, mw)
        stages |= set(np.unique(want["stage"]).tolist())
    assert stages == {UO.INTERPOLATED, UO.HOLE, UO.ORPHAN}


def test_min_weight_on_both_sides_of_a_planted_weight(rt, host):
    """minWeight one float below, at, and one float above the 2 x 2 weight of a chosen pixel: a hole exactly in the last case."""
    shape = ((65, 35), (130, 70))
    low, hl, hh = UO.make_case(shape)
    dev = Device(host, low, hl, hh)
    base = UO.upsample(low, hl, hh, 2, 0.0)
    sw = base["sw1"]
    cand = np.argwhere((sw > 0.3) & (sw < 0.9))
    assert len(cand) > 10
    for y, x in cand[[0, len(cand) // 2, -1]]:
        v = sw[y, x]
        for mw, hole in ((np.nextafter(v, F(0)), False), (v, False), (np.nextafter(v, F(2)), True)):
            want = UO.upsample(low, hl, hh, 2, float(mw))
            assert (want["stage"][y, x] != UO.INTERPOLATED) == hole
            check(dev, rt, want, len(want["full_list"]), 2, float(mw), f"pixel ({x}, {y})")


def test_same_bytes_over_dirty_buffers(rt, host):
    import torch
    shape = ((133, 5), (265, 9))
    low, hl, hh = UO.make_case(shape)
    dev = Device(host, low, hl, hh)
    rng = np.random.default_rng(3)
    runs = []
    for k in range(3):
        dev.scratch.t.copy_(torch.from_numpy(rng.integers(0, 256, dev.scratch.n, dtype=np.uint8)).cuda())
        dev.sel.t.fill_(0x11 * (k + 1))
        out, lst, st, bal = dev.run(rt, dev.w * dev.h, 5, 0.25)
        runs.append((out.tobytes(), lst.tobytes(), st.tobytes(), bal.tobytes()))
    assert runs[0] == runs[1] == runs[2]
    want = UO.upsample(low, hl, hh, 5, 0.25)
    assert runs[0][0] == want["out"].tobytes() and runs[0][3] == want["ballots"].tobytes()


# ---- 2. rt_image_put_at --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (67, 9), (130, 70)])
def test_image_put_at_matches_numpy(rt, w, h):
    import adaptive_oracle as DO
    rng = np.random.default_rng(7 * w + h)
    img = rng.normal(0, 1, (h, w, 4)).astype(np.float32)
    image = Guarded(w * h * 16, img)
    xs, ys = DO.tile_order(w, h)
    full = np.stack([xs, ys], axis=-1).astype(np.uint32)
    outside = np.array([[w, 0], [0, h], [w, h], [2 ** 31, 0], [2 ** 32 - 1, 3], [2 ** 32 - 1, 2 ** 32 - 1]], dtype=np.uint32)
    for k in range(3):
        keep = rng.permutation(len(full))[: max(1, int(len(full) * (1.0, 0.4, 0.05)[k]))]
        lst = np.concatenate([outside[:3], full[keep], outside[3:]])
        lst = lst[rng.permutation(len(lst))] if k else lst
        samples = rng.normal(0, 1, (len(lst), 4)).astype(np.float32)
        samples.reshape(-1)[:4] = (np.nan, np.inf, -0.0, 1e-40)      # copied as they stand
        img = UO.image_put_at(img, samples, lst)
        rt.image_put_at(up(samples), up(lst.view(np.int32)), len(lst), image.t, w, h)
        assert same_bits(image.read().view(np.float32).reshape(h, w, 4), img), k
    rt.image_put_at(None, None, 0, image.t, w, h)
    assert same_bits(image.read().view(np.float32).reshape(h, w, 4), img), "n = 0"


# ---- 3. the chain on the renderer ----------------------------------------------------------------------------------------------------------
def _luma(img):
    return (F(0.2126) * img[..., 0] + F(0.7152) * img[..., 1]) + F(0.0722) * img[..., 2]


def test_chain_reshades_exactly_the_holes(rt, host):
    """C2 at 64 x 36 -> 128 x 72 on one caller's stream, the header's loop: the low render, first hits at both sizes, rt_upsample, the
    8-byte read of nSelected / nListed -- the only wait in front of the read-back -- then camera_rays_at -> shade_rays ->
    image_put_at on the holes.  Every listed pixel equals rt_render_to(pHigh)'s bit for bit, every other pixel the oracle's, and
    along the silhouettes (output pixels whose 3 x 3 neighbourhood of first hits holds more than one object) the mean |dY| against
    the full render is smaller than that of rt_display_resample(TRIANGLE) of the same low frame."""
    import torch
    from opengl_raytracing_amd import scenes
    sc = scenes.make_scene(2, host.generate_aabb)
    rt.load(sc)
    sc.frame_count = 3
    (lw, lh), (w, h) = (64, 36), (128, 72)
    p_low, p_high = sc.params(width=lw, height=lh), sc.params(width=w, height=h)
    power, mw = 5, 0.25
    low, ref, out, tri = Guarded(lw * lh * 16), Guarded(w * h * 16), Guarded(w * h * 16), Guarded(w * h * 16)
    lst, scratch, sel = Guarded((w * h + 1) * 8), Guarded(host.upsample_layout(w, h)), Guarded(64)
    lst.t.fill_(SENTINEL)
    d_pos = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    d_nrm = torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32).pin_memory()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        rt.render_to(p_high, ref.t.data_ptr(), d_pos.data_ptr(), d_nrm.data_ptr(), stream=s.cuda_stream)
        rt.render_to(p_low, low.t.data_ptr(), d_pos.data_ptr(), d_nrm.data_ptr(), stream=s.cuda_stream)
        d_hits_low = rt.trace_rays(rt.camera_rays(p_low, stream=s), "closest", stream=s)
        d_hits_high = rt.trace_rays(rt.camera_rays(p_high, stream=s), "closest", stream=s)
        rt.upsample(low.t, d_hits_low, d_hits_high, out.t, lst.t, w * h, scratch.t, sel.t, w, h, lw, lh, normal_log2_power=power,
                    min_weight=mw, stream=s)
        rt.resample(low.t, tri.t, lw, lh, w, h, filter="triangle", stream=s)
        counts.copy_(sel.t[L.SELECT_NSELECTED_OFFSET: L.SELECT_NSELECTED_OFFSET + 8].view(torch.int32), non_blocking=True)
        s.synchronize()                                         # the loop's 8-byte read
        n_holes, n = int(counts[0]), int(counts[1])
        pixels = lst.t[: n * 8].view(torch.int32).view(n, 2)
        rays = rt.camera_rays_at(p_high, pixels, n, stream=s)
        colour = rt.shade_rays(p_high, rays, pixels=pixels, stream=s, position=False, normal=False)[0]
        rt.image_put_at(colour, pixels, n, out.t, w, h, stream=s)
    s.synchronize()
    img_low = low.read().view(np.float32).reshape(lh, lw, 4)
    hits_low = d_hits_low.cpu().numpy().reshape(lh, lw, 8).view(L.HIT_DTYPE).reshape(lh, lw)
    hits_high = d_hits_high.cpu().numpy().reshape(h, w, 8).view(L.HIT_DTYPE).reshape(h, w)
    want = UO.upsample(img_low, hits_low, hits_high, power, mw, capacity=w * h)
    state = sel.read().view(L.SELECT_STATE_DTYPE)[0]
    assert same_bits(as_bytes(state), as_bytes(want["state"])), (state, want["state"])
    assert n == n_holes == len(want["full_list"]) and 0 < n < w * h // 2
    got_list = lst.read().view(np.uint32).reshape(-1, 2)
    assert np.array_equal(got_list[:n], want["full_list"]) and (got_list[n:].view(np.uint8) == SENTINEL).all()
    full = ref.read().view(np.float32).reshape(h, w, 4)
    got = out.read().view(np.float32).reshape(h, w, 4)
    listed = want["stage"] != UO.INTERPOLATED
    assert same_bits(got[listed], full[listed]), "a listed pixel differs from rt_render_to's"
    assert same_bits(got[~listed], want["out"][~listed]), "an interpolated pixel differs from the oracle's"
    obj = hits_high["object"]
    pad = np.pad(obj, 1, mode="edge")
    edge = np.zeros((h, w), dtype=bool)
    for dy in range(3):
        for dx in range(3):
            edge |= pad[dy: dy + h, dx: dx + w] != obj
    assert edge.sum() > 100
    triangle = tri.read().view(np.float32).reshape(h, w, 4)
    err_up = float(np.abs(_luma(got) - _luma(full))[edge].astype(np.float64).mean())
    err_tri = float(np.abs(_luma(triangle) - _luma(full))[edge].astype(np.float64).mean())
    print(f"holes {n} of {w * h} ({n / (w * h):.3f}), orphans {int(state['nCapped'])}; mean |dY| over {int(edge.sum())} silhouette pixels: "
          f"upsample + re-shade {err_up:.5f}, triangle {err_tri:.5f}")
    assert err_up < err_tri
    del rays, colour


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(rt, host):
    import torch
    shape = ((9, 5), (20, 12))
    (lw, lh), (w, h) = shape
    low, hl, hh = UO.make_case(shape)
    dev = Device(host, low, hl, hh)
    want = UO.upsample(low, hl, hh, 5, 0.25)
    n = len(want["full_list"])
    assert n > 0
    samples = np.random.default_rng(9).normal(0, 1, (n, 4)).astype(np.float32)
    d_samples = up(samples)
    lib, ctx, vp = rt.lib, rt.ctx, ctypes.c_void_p
    lo, hlo, hhi, o, px, scr, sl, sm = (x.data_ptr() for x in (dev.low, dev.hits_low, dev.hits_high, dev.out.t, dev.list.t, dev.scratch.t,
                                                                dev.sel.t, d_samples))

    def desc(**kw):
        d = L.make_upsample_desc(w, h, lw, lh, 5, 0.25)
        for k, v in kw.items():
            if k == "reserved":
                d.reserved[v] = 1
            else:
                setattr(d, k, v)
        return d

    def upsample(low=lo, hits_low=hlo, hits_high=hhi, out=o, d="default", pixels=px, capacity=w * h, scratch=scr, sel=sl, c=ctx):
        d = desc() if d == "default" else d
        return lib.rt_upsample(c, vp(low), vp(hits_low), vp(hits_high), vp(out), ctypes.byref(d) if d is not None else None, vp(pixels),
                               capacity, vp(scratch), vp(sel), None)

    def put(smp=sm, pixels=px, count=n, image=o, width=w, height=h, c=ctx):
        return lib.rt_image_put_at(c, vp(smp), vp(pixels), count, vp(image), width, height, None)

    def still_works():
        dev.out.t.fill_(SENTINEL)
        dev.list.t.fill_(SENTINEL)
        torch.cuda.synchronize()
        assert upsample() == 0 and put() == 0
        rt.sync()
        assert same_bits(as_bytes(dev.sel.read().view(L.SELECT_STATE_DTYPE)[0]), as_bytes(UO.upsample(low, hl, hh, 5, 0.25, w * h)["state"]))
        assert np.array_equal(dev.list.read().view(np.uint32).reshape(-1, 2)[:n], want["full_list"])
        assert same_bits(dev.out.read().view(np.float32).reshape(h, w, 4), UO.image_put_at(want["out"], samples, want["full_list"]))
        dev.scratch.read()

    still_works()
    nan, inf = float("nan"), float("inf")
    bad = [desc(width=0), desc(width=-2), desc(height=0), desc(height=-1), desc(lowWidth=0), desc(lowWidth=-1), desc(lowWidth=w + 1),
           desc(lowHeight=0), desc(lowHeight=h + 1), desc(normalLog2Power=-1), desc(normalLog2Power=8), desc(minWeight=-0.5),
           desc(minWeight=1.5), desc(minWeight=nan), desc(minWeight=inf), desc(minWeight=-inf)] + [desc(reserved=k) for k in range(10)] + [None]
    for k, d in enumerate(bad):
        assert upsample(d=d) == INVALID, k
    still_works()
    nl, nh = lw * lh, w * h
    for kw in [dict(low=None), dict(hits_low=None), dict(hits_high=None), dict(out=None), dict(scratch=None), dict(sel=None), dict(pixels=None),
               dict(low=lo + 8), dict(hits_low=hlo + 4), dict(hits_high=hhi + 8), dict(out=o + 8), dict(scratch=scr + 8), dict(sel=sl + 4),
               dict(pixels=px + 4),
               # an output overlapping an input
               dict(out=lo), dict(out=hlo + nl * 32 - 16), dict(out=hhi + nh * 32 - 16), dict(low=o + nh * 16 - 16), dict(pixels=lo),
               dict(pixels=hhi + nh * 32 - 8), dict(scratch=hlo), dict(scratch=hhi + 16), dict(sel=lo + nl * 16 - 16), dict(sel=hhi),
               # two outputs overlapping
               dict(pixels=o), dict(pixels=o + nh * 16 - 8), dict(scratch=o + 16), dict(sel=o + 32), dict(sel=scr), dict(sel=px), dict(scratch=px),
               dict(c=None)]:
        assert upsample(**kw) == INVALID, kw
    assert upsample(pixels=None, capacity=0) == 0               # a pure count needs no list
    assert upsample(pixels=o, capacity=0) == 0                  # and an empty list overlaps nothing
    still_works()
    huge = desc(width=65536, height=32768)                      # 2^31 pixels
    assert upsample(d=huge) == TOO_LARGE
    for kw in [dict(smp=None), dict(pixels=None), dict(image=None), dict(smp=sm + 8), dict(pixels=px + 4), dict(image=o + 4), dict(width=0),
               dict(height=0), dict(width=-3), dict(smp=o), dict(smp=o + nh * 16 - 16), dict(pixels=o + 8), dict(pixels=o + nh * 16 - 8),
               dict(image=sm), dict(c=None)]:
        assert put(**kw) == INVALID, kw
    assert put(width=65536, height=32768) == TOO_LARGE and put(count=(2 ** 31 - 1) * 256 + 1) == TOO_LARGE
    assert put(smp=None, pixels=None, count=0) == 0
    still_works()
    torch.cuda.synchronize()
