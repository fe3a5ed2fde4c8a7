"""rt_display_pack_toned / rt_present_submit_toned on the GPU (include/rt_mi355.h) against the numpy float32 restatement of
tests/meter_oracle.py: the untoned form byte for byte equal to rt_display_pack, Reinhard and ACES with the exposure taken from the
descriptor, from device memory and from both, every code transition of every operator located by bisecting the ORACLE over float32
bit patterns, a rendered frame metered and presented end to end, and the refusals.  Every comparison is exact equality of uint8."""
import ctypes

import numpy as np
import pytest

import meter_oracle as MO
from opengl_raytracing_amd import layout as L

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
INVALID = -1
OPS = [("reinhard", 1.0), ("reinhard", 4.0), ("reinhard", 1.0 / 256.0), ("reinhard", 1e4), ("aces", 1.0)]


@pytest.fixture(scope="module")
def rt(host):
    t = host.RayTracer(0)
    yield t
    t.close()


@pytest.fixture(scope="module")
def table(host):
    return host.display_srgb_thresholds()


def up(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def packed(rt, d_img, w, h, **kw):
    """display_pack into a buffer with a guard row behind it -> uint8 [h, w, 4]."""
    import torch
    d_out = torch.full(((h + 1) * w * 4,), SENTINEL, dtype=torch.uint8, device="cuda")
    rt.display_pack(d_img, d_out, w, h, **kw)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert (got[h * w * 4:] == SENTINEL).all(), f"guard row written ({kw})"
    return got[: h * w * 4].reshape(h, w, 4)


# ---- 1. no curve, no device exposure: rt_display_pack's bytes ---------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["linear", "srgb"])
@pytest.mark.parametrize("w,h", MO.SHAPES, ids=[f"{w}x{h}" for w, h in MO.SHAPES])
def test_untoned_equals_display_pack(rt, table, w, h, fmt):
    img = MO.hdr_image(np.random.default_rng(3000 * w + h), w, h)
    d_img = up(img)
    for flip in (False, True):
        plain = packed(rt, d_img, w, h, format=fmt, flip=flip, exposure=0.37)
        toned = packed(rt, d_img, w, h, format=fmt, flip=flip, exposure=0.37, tone="none")
        assert (toned == plain).all(), f"flip={flip}"
        assert (plain == MO.pack_toned(img, fmt, flip, 0.37, table)).all(), f"flip={flip}"


# ---- 2. the curves, with every source of the exposure -----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["linear", "srgb"])
@pytest.mark.parametrize("w,h", MO.SHAPES, ids=[f"{w}x{h}" for w, h in MO.SHAPES])
def test_curves_match_numpy(rt, table, w, h, fmt):
    img = MO.hdr_image(np.random.default_rng(4000 * w + h), w, h)
    d_img = up(img)
    dev = np.float32(0.61)
    d_exp = up(np.array([dev], dtype=np.float32))
    sources = [dict(exposure=2.5), dict(exposure=1.0, d_exposure=d_exp.data_ptr()), dict(exposure=0.37, d_exposure=d_exp.data_ptr())]
    for tone, white in OPS + [("none", 1.0)]:
        for src in sources:
            if tone == "none" and "d_exposure" not in src:
                continue                                       # (test 1)
            want = MO.pack_toned(img, fmt, False, src["exposure"], table, tone, white, dev if "d_exposure" in src else None)
            for flip in (False, True):                         # (the flipped oracle is the oracle's rows reversed)
                got = packed(rt, d_img, w, h, format=fmt, flip=flip, tone=tone, white=white, **src)
                assert (got == (want[::-1] if flip else want)).all(), (flip, tone, white, src)


# ---- 3. code transitions ------------------------------------------------------------------------------------------------------------
def _first_y_reaching(tone, white, fmt, table):
    """For every code c = 1..255 the smallest positive float32 y (by bit pattern, found by bisection of the numpy oracle between the
    smallest denormal and 65536) whose code is >= c."""
    code = lambda bits: MO.code_of(MO.tone_curve(bits.astype(np.uint32).view(np.float32), tone, white), fmt, table)
    c = np.arange(1, 256)
    lo = np.full(255, 1, dtype=np.int64)
    hi = np.full(255, int(np.float32(65536.0).view(np.uint32)), dtype=np.int64)
    assert (code(lo) == 0).all() and (code(hi) == 255).all()
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        up_ = code(mid) >= c
        hi = np.where(up_, mid, hi)
        lo = np.where(up_, lo, mid)
    return hi.astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("fmt", ["linear", "srgb"])
@pytest.mark.parametrize("tone,white", [("reinhard", 4.0), ("reinhard", 1.0 / 256.0), ("aces", 1.0)], ids=["reinhard4", "reinhard1_256", "aces"])
def test_code_transitions(rt, table, tone, white, fmt):
    y = _first_y_reaching(tone, white, fmt, table)
    assert (np.diff(y.astype(np.float64)) >= 0).all() and y[0] > 0
    around = np.stack([(y.view(np.int32) + k).view(np.float32) for k in (-2, -1, 0, 1, 2)], axis=1).reshape(-1)
    vals = np.concatenate([around, np.float32([65536.0, 65537.0, 1e5, 3e38, np.inf])])
    n = len(vals)
    assert n == 1280
    for w in (n, 5):
        h = n // w
        img = np.zeros((h * w, 4), dtype=np.float32)
        img[:, 0], img[:, 1], img[:, 2], img[:, 3] = vals, np.roll(vals, -1), np.roll(vals, -2), 0.25
        img = img.reshape(h, w, 4)
        got = packed(rt, up(img), w, h, format=fmt, tone=tone, white=white)
        assert (got == MO.pack_toned(img, fmt, False, 1.0, table, tone, white)).all(), f"width {w}"
        red = got.reshape(-1, 4)[: 255 * 5, 0].reshape(255, 5)
        assert (red[:, 2] == np.arange(1, 256)).all() and (red[:, 1] < np.arange(1, 256)).all(), f"width {w}"
        assert (got.reshape(-1, 4)[255 * 5:, 0] == 255).all()


# ---- 4. end to end --------------------------------------------------------------------------------------------------------------------
def test_render_meter_present_end_to_end(host, table):
    import torch
    from opengl_raytracing_amd import scenes
    sc = scenes.make_scene(2, host.generate_aabb)
    w, h = 64, 36
    p = sc.params(width=w, height=h)
    tables = host.meter_tables()
    desc = dict(key=0.18, low_permille=10, high_permille=10)
    ring = host.RayTracer(0)
    try:
        ring.load(sc)
        d_state = torch.zeros((1088,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ring.render(p)
        d_color = ring.get_surfaces()[0]
        ring.meter(d_color, d_state, w, h, **desc)
        t = ring.present_submit(d_color, w, h, format="srgb", flip=True, tone="reinhard", white=4.0,
                                d_exposure=d_state.data_ptr() + L.METER_EXPOSURE_OFFSET)
        got = ring.present_wait(t)
        color = ring.readback()[0]
        torch.cuda.synchronize()
        state = d_state.cpu().numpy().view(L.METER_STATE_DTYPE)[0]
        want_state = MO.meter(color, np.zeros(1, dtype=L.METER_STATE_DTYPE)[0], tables, **desc)
        assert MO.state_bytes(state).tobytes() == MO.state_bytes(want_state).tobytes(), MO.describe_difference(state, want_state)
        assert state["nMetered"] > 0 and state["exposure"] != 1.0
        assert (got == MO.pack_toned(color, "srgb", True, 1.0, table, "reinhard", 4.0, want_state["exposure"])).all()
        assert len(np.unique(got[..., :3])) > 16
    finally:
        ring.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(host, table):
    import torch
    w, h = 8, 4
    img = MO.hdr_image(np.random.default_rng(99), w, h)
    d_img = up(img)
    d_out = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    d_exp = up(np.array([0.5, 0.25], dtype=np.float32))
    ring = host.RayTracer(0)
    lib, ctx, vp = ring.lib, ring.ctx, ctypes.c_void_p
    want = MO.pack_toned(img, "linear", False, 1.0, table, "aces", dev_exposure=np.float32(0.5))

    def tone(**kw):
        t = L.make_tone_desc("aces", 1.0, d_exp.data_ptr())
        for k, v in kw.items():
            if k == "reserved":
                t.reserved[v] = 1
            else:
                setattr(t, k, v)
        return t

    def pack(t, d=None):
        d = d or L.make_display_desc(w, h)
        return lib.rt_display_pack_toned(ctx, vp(d_img.data_ptr()), vp(d_out.data_ptr()), ctypes.byref(d), ctypes.byref(t) if t is not None else None, None)

    def submit(t, d=None):
        d = d or L.make_display_desc(w, h)
        k = ctypes.c_uint64(0)
        return lib.rt_present_submit_toned(ctx, vp(d_img.data_ptr()), ctypes.byref(d), ctypes.byref(t) if t is not None else None, None, ctypes.byref(k))

    def still_works():
        d_out.zero_()
        torch.cuda.synchronize()
        assert pack(tone()) == 0
        ring.sync()
        assert (d_out.cpu().numpy() == want).all()

    try:
        nan, inf = float("nan"), float("inf")
        bad = [tone(op=3), tone(op=-1), tone(op=L.TONE_REINHARD, white=0.0), tone(op=L.TONE_REINHARD, white=1.0 / 512.0),
               tone(op=L.TONE_REINHARD, white=-4.0), tone(op=L.TONE_REINHARD, white=nan), tone(op=L.TONE_REINHARD, white=inf),
               tone(dExposure=d_exp.data_ptr() + 1), tone(dExposure=d_exp.data_ptr() + 2), tone(dExposure=d_exp.data_ptr() + 3),
               tone(reserved=0), tone(reserved=1), tone(reserved=2), tone(reserved=3), None]
        for k, t in enumerate(bad):
            assert pack(t) == INVALID, k
            assert submit(t) == INVALID, k
            still_works()
        bad_display = L.make_display_desc(w, h, exposure=0.0)                  # rt_display_pack's own refusals hold
        assert pack(tone(), bad_display) == INVALID and submit(tone(), bad_display) == INVALID
        bad_display = L.make_display_desc(w, h)
        bad_display.reserved[1] = 1
        assert pack(tone(), bad_display) == INVALID and submit(tone(), bad_display) == INVALID
        still_works()
        assert pack(tone(white=nan)) == 0 and pack(tone(op=L.TONE_NONE, white=-1.0)) == 0      # white is ignored unless Reinhard
        assert pack(tone(op=L.TONE_REINHARD, white=1.0 / 256.0, dExposure=d_exp.data_ptr() + 4)) == 0
        ring.sync()
        assert (d_out.cpu().numpy() == MO.pack_toned(img, "linear", False, 1.0, table, "reinhard", 1.0 / 256.0, np.float32(0.25))).all()
        ready = ctypes.c_int(0)
        assert lib.rt_present_poll(ctx, 0, ctypes.byref(ready)) == INVALID      # every refused submit took no ticket
        t = ring.present_submit(d_img, w, h, tone="aces", d_exposure=d_exp.data_ptr())
        assert t == 0
        assert (ring.present_wait(t) == want).all()
        t = ring.present_submit(d_img, w, h)                                     # the untoned submit shares the ring and its tickets
        assert t == 1
        assert (ring.present_wait(t) == MO.pack_toned(img, "linear", False, 1.0, table)).all()
    finally:
        ring.close()
