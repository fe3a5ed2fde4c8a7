"""rt_display_pack_yuv / rt_present_submit_yuv on the GPU (include/rt_mi355.h) against the numpy restatement of tests/yuv_oracle.py:
every shape class of the kernel (whole pixel blocks, ragged widths, odd heights, single pixels) in both plane formats and row
orders, the RGBA8 bytes of the existing pack pushed through the integer matrix, greys and cube corners, the tone curves and a
device-resident exposure, the shared ring, and the refusals.  Every comparison is exact equality of uint8."""
import ctypes
import itertools

import numpy as np
import pytest

import meter_oracle as MO
import yuv_oracle as YO
from opengl_raytracing_amd import layout as L

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 256
INVALID, TOO_LARGE = -1, -4
SHAPES = [(1, 1), (2, 2), (3, 2), (2, 3), (5, 7), (8, 2), (16, 4), (64, 5), (24, 6), (67, 9), (257, 3), (640, 360)]
MATRIX_NAMES, RANGE_NAMES, TRANSFERS, EXPOSURES = ("bt709", "bt601"), ("limited", "full"), ("srgb", "linear"), (1.0, 0.37, 2.5)


def is_fast(w, h):
    """The shapes the kernel's unpredicated form takes."""
    return w % 8 == 0 and h % 2 == 0


def plan(si):
    """The four launches of shape number si: (format, flip) in full, the other options cycled so that every value of each meets
    every shape (test_plan_covers_every_option checks it)."""
    out = []
    for j, (fmt, flip) in enumerate(itertools.product(YO.FORMATS, (False, True))):
        out.append(dict(fmt=fmt, flip=flip, matrix_name=MATRIX_NAMES[(j + si) % 2], rng=RANGE_NAMES[(j // 2 + si) % 2],
                        transfer=TRANSFERS[(j + j // 2 + si) % 2], exposure=EXPOSURES[(j + si) % 3]))
    return out


def test_plan_covers_every_option():
    for cls in (True, False):
        launches = [o for si, (w, h) in enumerate(SHAPES) if is_fast(w, h) == cls for o in plan(si)]
        assert launches
        for key, values in (("fmt", YO.FORMATS), ("flip", (False, True)), ("matrix_name", MATRIX_NAMES), ("rng", RANGE_NAMES),
                            ("transfer", TRANSFERS), ("exposure", EXPOSURES)):
            assert {o[key] for o in launches} == set(values), (cls, key)
    for si in range(len(SHAPES)):                              # and within every single shape
        for key, n in (("fmt", 2), ("flip", 2), ("matrix_name", 2), ("rng", 2), ("transfer", 2), ("exposure", 3)):
            assert len({o[key] for o in plan(si)}) == n, (si, key)
    assert any(is_fast(w, 2) and h % 2 for w, h in SHAPES) and (2, 3) in SHAPES and (3, 2) in SHAPES


@pytest.fixture(scope="module")
def rt(host):
    t = host.RayTracer(0)
    yield t
    t.close()


@pytest.fixture()
def ring(host):
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


def kw_of(o):
    """An oracle option set as display_pack_yuv's keywords."""
    return dict(format=o["fmt"], matrix=o["matrix_name"], range=o["rng"], transfer=o["transfer"], flip=o["flip"], exposure=o["exposure"])


def packed(rt, host, d_img, w, h, **kw):
    """display_pack_yuv into a buffer with a guard region behind the frame -> the flat uint8 frame."""
    import torch
    n = host.yuv_layout(w, h, kw.get("format", "nv12")).bytes
    d_out = torch.full((n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    rt.display_pack_yuv(d_img, d_out, w, h, **kw)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert (got[n:] == SENTINEL).all(), f"guard region written ({kw})"
    return got[:n]


def flat(planes):
    """present_wait_yuv's planes as the flat frame."""
    return np.concatenate([p.reshape(-1) for p in planes])


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(SHAPES)), ids=[f"{w}x{h}" for w, h in SHAPES])
def test_pack_matches_numpy(rt, host, table, si):
    w, h = SHAPES[si]
    img = MO.hdr_image(np.random.default_rng(7000 * w + h), w, h)
    d_img = up(img)
    for o in plan(si):
        got = packed(rt, host, d_img, w, h, **kw_of(o))
        want = YO.pack_yuv(img, table, **o)
        assert got.shape == want.shape and (got == want).all(), (o, np.nonzero(got != want)[0][:8])


# ---- 2. against the existing kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(5, 7), (16, 4), (67, 9)])
def test_matrix_of_the_rgba8_pack(rt, host, w, h):
    """The R'G'B' codes come from rt_display_pack / rt_display_pack_toned ON THE GPU, not from numpy; only the integer matrix is
    the oracle's."""
    import torch
    img = MO.hdr_image(np.random.default_rng(8000 * w + h), w, h)
    d_img = up(img)
    d_exp = up(np.array([0.61], dtype=np.float32))
    d_rgba = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    cases = [dict(), dict(tone="reinhard", white=4.0, d_exposure=d_exp.data_ptr()), dict(tone="aces")]
    for k, (extra, transfer, flip) in enumerate(itertools.product(cases, TRANSFERS, (False, True))):
        fmt, matrix, rng = YO.FORMATS[k % 2], MATRIX_NAMES[(k // 2) % 2], RANGE_NAMES[(k // 3) % 2]
        rt.display_pack(d_img, d_rgba, w, h, format=transfer, flip=flip, exposure=0.37, **extra)
        torch.cuda.synchronize()
        rgb = d_rgba.cpu().numpy()[..., :3]                    # (already in output row order)
        got = packed(rt, host, d_img, w, h, format=fmt, matrix=matrix, range=rng, transfer=transfer, flip=flip, exposure=0.37, **extra)
        assert (got == YO.frame_from_codes(rgb, fmt, matrix, rng)).all(), (extra, transfer, flip, fmt, matrix, rng)


# ---- 3. greys and corners --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix,rng", list(itertools.product(MATRIX_NAMES, RANGE_NAMES)))
def test_greys_have_no_colour(rt, host, table, matrix, rng):
    """256 greys, one per 2x2 block of a 32x32 frame, as code / 255 with the linear transfer."""
    code = np.arange(256).reshape(16, 16)
    img = np.ones((32, 32, 4), dtype=np.float32)
    img[..., :3] = np.repeat(np.repeat(code, 2, axis=0), 2, axis=1)[..., None].astype(np.float32) / np.float32(255.0)
    rgb = YO.codes(img, "linear", 1.0, table)
    assert (rgb[::2, ::2, 0].reshape(-1) == np.arange(256)).all() and (rgb == rgb[..., :1]).all()
    c = YO.coeffs(matrix, rng)
    for fmt in YO.FORMATS:
        got = host.yuv_planes(packed(rt, host, up(img), 32, 32, format=fmt, matrix=matrix, range=rng, transfer="linear"), 32, 32, fmt)
        assert all((p == 128).all() for p in got[1:]), fmt
        want_y = c[3] + ((sum(c[0:3]) * np.arange(256) + 32768) >> 16)
        assert (got[0][::2, ::2].reshape(-1) == want_y).all() and (got[0] == np.repeat(np.repeat(got[0][::2, ::2], 2, axis=0), 2, axis=1)).all()
        assert got[0].min() == (16 if rng == "limited" else 0) and got[0].max() == (235 if rng == "limited" else 255)


@pytest.mark.parametrize("matrix,rng", list(itertools.product(MATRIX_NAMES, RANGE_NAMES)))
def test_cube_corners(rt, host, table, matrix, rng):
    """Row pair 0: the eight corners of the RGB cube, a 2x2 block each; row pair 1: blocks of four different corners; then the same
    with a ragged right edge (15 wide) and an odd height (3)."""
    corners = np.array(list(itertools.product((0.0, 1.0), repeat=3)), dtype=np.float32)
    img = np.ones((4, 16, 4), dtype=np.float32)
    img[:2, :, :3] = np.repeat(np.repeat(corners.reshape(1, 8, 3), 2, axis=0), 2, axis=1)
    for b in range(8):
        img[2:, 2 * b: 2 * b + 2, :3] = corners[[(b + 1) % 8, (b + 3) % 8, (b + 4) % 8, (b + 6) % 8]].reshape(2, 2, 3)
    c = YO.coeffs(matrix, rng)
    Y, Cb, Cr = YO.matrix_unclamped(YO.codes(img, "linear", 1.0, table), c)
    if rng == "full":
        assert Cb.max() == 256 and Cr.max() == 256             # the clamp is exercised
    else:
        assert 16 <= min(Cb.min(), Cr.min()) and max(Cb.max(), Cr.max()) <= 240
    for (w, h), fmt in itertools.product([(16, 4), (15, 3)], YO.FORMATS):
        sub = np.ascontiguousarray(img[:h, :w])
        got = packed(rt, host, up(sub), w, h, format=fmt, matrix=matrix, range=rng, transfer="linear")
        assert (got == YO.pack_yuv(sub, table, fmt, matrix, rng, "linear")).all(), (w, h, fmt)
        if rng == "full" and (w, h) == (16, 4):
            assert got[w * h:].max() == 255


# ---- 4. tone and device exposure -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(24, 6), (67, 9)])
def test_tone_curves(rt, host, table, w, h):
    img = MO.hdr_image(np.random.default_rng(9000 * w + h), w, h)
    d_img = up(img)
    dev = np.float32(0.61)
    d_exp = up(np.array([dev], dtype=np.float32))
    for k, ((tone, white), transfer) in enumerate(itertools.product([("reinhard", 4.0), ("reinhard", 1.0 / 256.0), ("aces", 1.0), ("none", 1.0)], TRANSFERS)):
        o = dict(fmt=YO.FORMATS[k % 2], flip=bool(k & 2), matrix_name=MATRIX_NAMES[(k // 2) % 2], rng=RANGE_NAMES[k % 2], transfer=transfer,
                 exposure=0.37)
        got = packed(rt, host, d_img, w, h, tone=tone, white=white, d_exposure=d_exp.data_ptr(), **kw_of(o))
        assert (got == YO.pack_yuv(img, table, tone=tone, white=white, dev_exposure=dev, **o)).all(), (tone, white, o)
        if tone != "none":
            o["exposure"] = 2.5
            got = packed(rt, host, d_img, w, h, tone=tone, white=white, **kw_of(o))
            assert (got == YO.pack_yuv(img, table, tone=tone, white=white, **o)).all(), (tone, white, o)


def test_metered_exposure_without_a_host_round_trip(rt, host, table):
    import torch
    w, h = 67, 9
    img = MO.hdr_image(np.random.default_rng(31), w, h)
    d_img = up(img)
    n = host.yuv_layout(w, h, "nv12").bytes
    d_state = torch.zeros((1088,), dtype=torch.uint8, device="cuda")
    d_out = torch.full((n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rt.meter(d_img, d_state, w, h, key=0.18, low_permille=10, high_permille=10, stream=s)
        rt.display_pack_yuv(d_img, d_out, w, h, tone="aces", d_exposure=d_state.data_ptr() + L.METER_EXPOSURE_OFFSET, stream=s)
    s.synchronize()
    state = d_state.cpu().numpy().view(L.METER_STATE_DTYPE)[0]
    want_state = MO.meter(img, np.zeros(1, dtype=L.METER_STATE_DTYPE)[0], host.meter_tables(), key=0.18, low_permille=10, high_permille=10)
    assert state["exposure"] == want_state["exposure"] and state["exposure"] != 1.0
    got = d_out.cpu().numpy()
    assert (got[n:] == SENTINEL).all()
    assert (got[:n] == YO.pack_yuv(img, table, tone="aces", dev_exposure=state["exposure"])).all()


# ---- 5. the ring -----------------------------------------------------------------------------------------------------------------------
def test_one_ring_serves_every_format(ring, host, table):
    import torch
    w, h = 67, 9
    rng = np.random.default_rng(41)
    frames = [MO.hdr_image(rng, w, h) for _ in range(4)]
    d = [up(f) for f in frames]
    ring.present_configure(4)
    s = torch.cuda.Stream()
    t = [ring.present_submit(d[0], w, h, format="srgb", exposure=0.37, stream=s),
         ring.present_submit_yuv(d[1], w, h, format="nv12", exposure=0.37, stream=s),
         ring.present_submit_yuv(d[2], w, h, format="i420", matrix="bt601", range="full", flip=True, stream=s),
         ring.present_submit(d[3], w, h, format="linear", tone="reinhard", white=4.0, stream=s)]
    assert t == [0, 1, 2, 3]
    px, nb = ctypes.c_void_p(), ctypes.c_size_t(0)
    for ticket, fmt in ((2, "i420"), (1, "nv12")):
        assert ring.lib.rt_present_wait(ring.ctx, ticket, ctypes.byref(px), ctypes.byref(nb)) == 0
        assert nb.value == host.yuv_layout(w, h, fmt).bytes == YO.layout(w, h, fmt)[2]
    got = ring.present_wait_yuv(2)
    assert len(got) == 3 and got[0].shape == (h, w) and got[1].shape == got[2].shape == ((h + 1) // 2, (w + 1) // 2)
    assert (flat(got) == YO.pack_yuv(frames[2], table, "i420", "bt601", "full", flip=True)).all()
    assert (ring.present_wait(3) == MO.pack_toned(frames[3], "linear", False, 1.0, table, "reinhard", 4.0)).all()
    assert (ring.present_wait(0) == MO.pack_toned(frames[0], "srgb", False, 0.37, table)).all()
    got = ring.present_wait_yuv(1, copy=False)
    assert len(got) == 2 and got[1].shape == ((h + 1) // 2, (w + 1) // 2, 2) and not got[0].flags.writeable
    assert (flat(got) == YO.pack_yuv(frames[1], table, "nv12", exposure=0.37)).all()
    with pytest.raises(ValueError, match="YUV"):
        ring.present_wait(1)                                   # a clear error, not present_wait's size assertion
    with pytest.raises(ValueError, match="YUV"):
        ring.present_wait_yuv(0)


def test_source_may_be_overwritten_behind_the_submit(ring, host, table):
    import torch
    w, h = 640, 360
    img = MO.hdr_image(np.random.default_rng(43), w, h)
    d = up(img)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = ring.present_submit_yuv(d, w, h, stream=s)
        d.zero_()
    assert (flat(ring.present_wait_yuv(t)) == YO.pack_yuv(img, table)).all()


def test_slot_grows_from_yuv_to_rgba8_under_a_live_ticket(ring, host, table):
    """Two slots.  A small YUV frame in each, then a large RGBA8 frame into slot 0, whose buffers hold 1.5 B per small pixel: they
    grow, after a host wait for that slot's own last copy.  The YUV ticket in slot 1 stays valid and right."""
    import torch
    rng = np.random.default_rng(47)
    small, large = (64, 36), (640, 360)
    frames = [MO.hdr_image(rng, *small), MO.hdr_image(rng, *small), MO.hdr_image(rng, *large), MO.hdr_image(rng, *small)]
    d = [up(f) for f in frames]
    ring.present_configure(2)
    s = torch.cuda.Stream()
    assert ring.present_submit_yuv(d[0], *small, format="i420", stream=s) == 0
    assert ring.present_submit_yuv(d[1], *small, format="nv12", stream=s) == 1
    assert (flat(ring.present_wait_yuv(0)) == YO.pack_yuv(frames[0], table, "i420")).all()
    view1 = ring.present_wait_yuv(1, copy=False)
    want1 = YO.pack_yuv(frames[1], table, "nv12")
    assert ring.present_submit(d[2], *large, format="srgb", stream=s) == 2        # slot 0 grows under ticket 1 in slot 1
    assert (flat(view1) == want1).all()
    assert (flat(ring.present_wait_yuv(1)) == want1).all()
    assert (ring.present_wait(2) == MO.pack_toned(frames[2], "srgb", False, 1.0, table)).all()
    assert ring.present_submit_yuv(d[3], *small, format="nv12", flip=True, stream=s) == 3        # a small frame into slot 1
    assert (flat(ring.present_wait_yuv(3)) == YO.pack_yuv(frames[3], table, "nv12", flip=True)).all()


def test_frame_to_planes_end_to_end(ring, host, table):
    import torch
    from opengl_raytracing_amd import scenes
    sc = scenes.make_scene(2, host.generate_aabb)
    w, h = 96, 64
    p = sc.params(width=w, height=h)
    ring.load(sc)
    d_display = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ring.frame(p, d_display=d_display.data_ptr())
    t = ring.present_submit_yuv(d_display, w, h, format="nv12", flip=True)
    y, uv = ring.present_wait_yuv(t)
    ring.sync()
    surface = d_display.cpu().numpy()
    assert np.nanmax(surface[..., :3]) > 0.05                                # a picture, not a cleared buffer
    assert (flat((y, uv)) == YO.pack_yuv(surface, table, "nv12", flip=True)).all()
    assert len(np.unique(y)) > 16 and len(np.unique(uv)) > 4


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(ring, host, table):
    import torch
    w, h = 8, 4
    img = MO.hdr_image(np.random.default_rng(53), w, h)
    d_img = up(img)
    nbytes = host.yuv_layout(w, h, "nv12").bytes
    d_big = torch.zeros((h * w * 4 + 64,), dtype=torch.float32, device="cuda")         # room for overlapping placements
    d_out = torch.zeros((nbytes,), dtype=torch.uint8, device="cuda")
    d_exp = up(np.array([0.5, 0.25], dtype=np.float32))
    torch.cuda.synchronize()
    lib, ctx, vp = ring.lib, ring.ctx, ctypes.c_void_p
    want = YO.pack_yuv(img, table)

    def desc(**kw):
        d = L.make_yuv_desc(w, h)
        for k, v in kw.items():
            if k == "reserved":
                d.reserved[v] = 1
            else:
                setattr(d, k, v)
        return d

    def tone(**kw):
        t = L.make_tone_desc("aces", 1.0, d_exp.data_ptr())
        for k, v in kw.items():
            if k == "reserved":
                t.reserved[v] = 1
            else:
                setattr(t, k, v)
        return t

    ref = lambda x: ctypes.byref(x) if x is not None else None

    def pack(image, out, d, t=None, context=True):
        return lib.rt_display_pack_yuv(ctx if context else None, vp(image), vp(out), ref(d), ref(t), None)

    def submit(image, d, t=None, ticket=True, context=True):
        k = ctypes.c_uint64(0)
        return lib.rt_present_submit_yuv(ctx if context else None, vp(image), ref(d), ref(t), None, ctypes.byref(k) if ticket else None)

    def still_works():
        d_out.zero_()
        torch.cuda.synchronize()
        assert pack(d_img.data_ptr(), d_out.data_ptr(), desc()) == 0
        ring.sync()
        assert (d_out.cpu().numpy() == want).all()

    i, o = d_img.data_ptr(), d_out.data_ptr()
    nan, inf = float("nan"), float("inf")
    bad_descs = [desc(exposure=0.0), desc(exposure=-1.0), desc(exposure=inf), desc(exposure=nan),
                 desc(format=2), desc(format=-1), desc(matrix=2), desc(matrix=-1), desc(range=2), desc(range=-1), desc(transfer=2),
                 desc(transfer=-1), desc(flags=2), desc(flags=3), desc(reserved=0), desc(reserved=1), desc(reserved=2), desc(reserved=3),
                 desc(width=0), desc(width=-3), desc(height=0), desc(height=-1), None]
    for k, d in enumerate(bad_descs):
        assert pack(i, o, d) == INVALID, k
        assert submit(i, d) == INVALID, k
        still_works()
    bad_tones = [tone(op=3), tone(op=-1), tone(op=L.TONE_REINHARD, white=0.0), tone(op=L.TONE_REINHARD, white=1.0 / 512.0),
                 tone(op=L.TONE_REINHARD, white=nan), tone(op=L.TONE_REINHARD, white=inf), tone(dExposure=d_exp.data_ptr() + 1),
                 tone(dExposure=d_exp.data_ptr() + 2), tone(reserved=0), tone(reserved=3)]
    for k, t in enumerate(bad_tones):
        assert pack(i, o, desc(), t) == INVALID, k
        assert submit(i, desc(), t) == INVALID, k
        still_works()
    b = d_big.data_ptr()
    bad_ptrs = [(None, o), (i, None), (i + 4, o), (i, o + 4), (i + 8, o + 8),
                (b, b), (b, b + 16), (b, b + h * w * 16 - 16), (b + 32, b), (b + 128, b + nbytes + 112)]
    for image, out in bad_ptrs:
        assert pack(image, out, desc()) == INVALID, (image, out)
        still_works()
    assert pack(b, b + h * w * 16, desc()) == 0                # adjacent, not overlapping
    assert pack(b + nbytes, b, desc()) == 0
    ring.sync()
    assert pack(i, o, desc(), context=False) == INVALID and submit(i, desc(), context=False) == INVALID
    for image in (None, i + 4):
        assert submit(image, desc()) == INVALID
    assert submit(i, desc(), ticket=False) == INVALID
    huge = desc(width=2 ** 31 - 1, height=2 ** 31 - 1)         # more blocks than a launch holds; refused before anything is touched
    assert pack(i, o, huge) == TOO_LARGE and submit(i, huge) == TOO_LARGE
    still_works()
    assert pack(i, o, desc(), tone(op=L.TONE_NONE, white=nan)) == 0                   # white is ignored unless Reinhard
    ring.sync()
    assert (d_out.cpu().numpy() == YO.pack_yuv(img, table, dev_exposure=np.float32(0.5))).all()
    ready = ctypes.c_int(0)
    assert lib.rt_present_poll(ctx, 0, ctypes.byref(ready)) == INVALID          # nothing issued: every refused submit took no ticket
    t = ring.present_submit_yuv(d_img, w, h)
    assert t == 0
    assert (flat(ring.present_wait_yuv(t)) == want).all()
    t = ring.present_submit(d_img, w, h)                                          # the RGBA8 submit shares the ring and its tickets
    assert t == 1
    assert (ring.present_wait(t) == MO.pack_toned(img, "linear", False, 1.0, table)).all()
    still_works()
