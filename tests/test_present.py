"""rt_display_pack and the rt_present_* ring on the GPU (include/rt_mi355.h): the packing arithmetic bit for bit against numpy
written from the header's definition (the library's own threshold table for sRGB; tests/test_present_host.py pins that table to
the formula), the four-pixel lane tail and the row flip over ragged shapes, every decision boundary of both formats, and the
delivery ring: tickets in and out of order, the source overwritten behind the submit, slot reuse and expiry, a caller's stream
with the host running ahead, buffers growing under a live ticket, rt_frame's and rt_render's surfaces end to end, and every
refusal.  Every comparison is exact equality of uint8 arrays."""
import ctypes

import numpy as np
import pytest

from opengl_raytracing_amd import layout as L

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
INVALID = -1                                    # RT_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def rt(host):
    t = host.RayTracer(0)
    yield t
    t.close()


@pytest.fixture
def ring(host):
    """A context of the test's own: its ring starts empty, with ticket 0."""
    t = host.RayTracer(0)
    yield t
    t.close()


@pytest.fixture(scope="module")
def table(host):
    return host.display_srgb_thresholds()


# ---- the oracle: the header's definition, in numpy ------------------------------------------------------------------------------
def pack_oracle(img, fmt, flip, exposure, table):
    """img float32 [h, w, 4] -> uint8 [h, w, 4]."""
    with np.errstate(all="ignore"):
        y = img[..., :3].astype(np.float32) * np.float32(exposure)          # 1. one fp32 multiply
        inside = (y > 0) & (y < 1)
        ys = np.where(inside, y, np.float32(0.5)).astype(np.float32)
        if fmt == "linear":
            q = np.rint(ys * np.float32(255.0)).astype(np.int64)            # 3. one fp32 multiply, nearest even
        else:
            # 4. the number of i in 1..255 with T[i] <= y: for an increasing table (tests/test_present_host.py) that is the
            #    insertion point to the right of y
            q = np.searchsorted(table[1:], ys.reshape(-1), side="right").reshape(ys.shape)
        q = np.where(y >= 1, 255, q)                                        # 2. +inf included
        q = np.where(~(y > 0), 0, q)                                        #    NaN, -0, -inf, y <= 0
    out = np.empty(img.shape[:2] + (4,), dtype=np.uint8)
    out[..., :3] = q
    out[..., 3] = 255                                                       # 5.
    return out[::-1].copy() if flip else out


SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, -1e-40, 1.0, 0.0, 1.4e-45, -1.0, np.float32(1.0) - np.float32(2.0 ** -24)],
                    dtype=np.float32)


def hdr_image(rng, w, h):
    """uniform^4 * 8 in every channel (alpha too), the special values planted over the colour channels as far as they fit."""
    img = (rng.uniform(0, 1, (h, w, 4)) ** 4 * 8).astype(np.float32)
    flat = img.reshape(-1, 4)
    n = flat.shape[0] * 3
    for k, v in enumerate(SPECIALS[: n]):
        pos = (k * 7919 + 3) % n if n > len(SPECIALS) else k
        flat[pos // 3, pos % 3] = v
    return img


def up(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


# ---- 1. pack parity over shapes ---------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (3, 2), (5, 7), (64, 4), (67, 9), (257, 3), (640, 360)]


@pytest.mark.parametrize("fmt", ["linear", "srgb"])
@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_pack_matches_numpy(rt, table, w, h, fmt):
    """Both row orders and three exposures per shape and format; the output is followed by a guard row of a sentinel byte that
    must come back untouched (the ragged widths end every row in a short quad)."""
    import torch
    rng = np.random.default_rng(1000 * w + h)
    img = hdr_image(rng, w, h)
    d_img = up(img)
    for flip in (False, True):
        for exposure in (1.0, 0.37, 2.5):
            d_out = torch.full(((h + 1) * w * 4,), SENTINEL, dtype=torch.uint8, device="cuda")
            rt.display_pack(d_img, d_out, w, h, format=fmt, flip=flip, exposure=exposure)
            torch.cuda.synchronize()
            got = d_out.cpu().numpy()
            assert (got[h * w * 4:] == SENTINEL).all(), f"guard row written (flip={flip}, exposure={exposure})"
            want = pack_oracle(img, fmt, flip, exposure, table)
            assert (got[: h * w * 4].reshape(h, w, 4) == want).all(), f"flip={flip}, exposure={exposure}"


# ---- 2. decision boundaries --------------------------------------------------------------------------------------------------------
def _ulps(v, k):
    """float32 v moved by k units in the last place (positive finite v)."""
    return (np.asarray(v, dtype=np.float32).view(np.int32) + np.int32(k)).view(np.float32)


def _boundary_values(fmt, table):
    if fmt == "srgb":                          # every threshold and its fp32 neighbours on both sides: 765 values
        t = table[1:]
        vals = np.stack([_ulps(t, -1), t, _ulps(t, 1)], axis=1).reshape(-1)
        codes = np.stack([np.arange(0, 255), np.arange(1, 256), np.arange(1, 256)], axis=1).reshape(-1)
        return vals, codes
    c = ((np.arange(255, dtype=np.float64) + 0.5) / 255.0).astype(np.float32)   # the tie points of rint(y * 255)
    return np.stack([_ulps(c, k) for k in (-2, -1, 0, 1, 2)], axis=1).reshape(-1), None


@pytest.mark.parametrize("fmt", ["linear", "srgb"])
def test_decision_boundaries(rt, table, fmt):
    """Exposure 1, so y is the stored value itself.  The value goes to red, its successors in the list to green and blue; laid
    out as one row and as a 5-wide image (every row then ends in a one-pixel quad)."""
    import torch
    vals, codes = _boundary_values(fmt, table)
    n = len(vals)
    assert n == (765 if fmt == "srgb" else 1275)
    for w in (n, 5):
        h = (n + w - 1) // w
        img = np.zeros((h * w, 4), dtype=np.float32)
        img[:n, 0], img[:n, 1], img[:n, 2] = vals, np.roll(vals, -1), np.roll(vals, -2)
        img[:, 3] = 0.25
        img = img.reshape(h, w, 4)
        d_out = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
        rt.display_pack(up(img), d_out, w, h, format=fmt)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert (got == pack_oracle(img, fmt, False, 1.0, table)).all(), f"width {w}"
        if codes is not None:                  # the definition read directly: T[i] itself and above is code i, just below it i - 1
            assert (got.reshape(-1, 4)[:n, 0] == codes).all(), f"width {w}"


# ---- 3. the ring, in order and out of order --------------------------------------------------------------------------------------
def test_ring_in_and_out_of_order(ring, table):
    import torch
    rng = np.random.default_rng(3)
    w, h = 257, 33
    frames = [hdr_image(rng, w, h) for _ in range(3)]
    kinds = [("linear", False, 1.0), ("srgb", True, 0.37), ("srgb", False, 2.5)]
    d = [up(f) for f in frames]
    ring.present_configure(3)
    s = torch.cuda.Stream()
    tickets = [ring.present_submit(d[k], w, h, format=kinds[k][0], flip=kinds[k][1], exposure=kinds[k][2], stream=s) for k in range(3)]
    assert tickets == [0, 1, 2]
    for k in (2, 0, 1):
        got = ring.present_wait(tickets[k])
        assert got.shape == (h, w, 4) and got.dtype == np.uint8
        assert (got == pack_oracle(frames[k], *kinds[k], table)).all(), f"ticket {k}"
        assert ring.present_poll(tickets[k]) is True
    view = ring.present_wait(0, copy=False)                    # a second wait on a live ticket; the pinned slot itself
    assert not view.flags.writeable
    assert (view == pack_oracle(frames[0], *kinds[0], table)).all()


# ---- 4. the source may be overwritten ---------------------------------------------------------------------------------------------
def test_source_may_be_overwritten_behind_the_submit(ring, table):
    import torch
    w, h = 640, 360
    img = hdr_image(np.random.default_rng(4), w, h)
    d = up(img)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = ring.present_submit(d, w, h, format="srgb", stream=s)
        d.fill_(7.0)                                           # next in s's order: the pack has consumed the image by then
    got = ring.present_wait(t)
    assert (got == pack_oracle(img, "srgb", False, 1.0, table)).all()
    s.synchronize()
    assert float(d[0, 0, 0]) == 7.0


# ---- 5. reuse and expiry -----------------------------------------------------------------------------------------------------------
def test_slot_reuse_expiry_and_reconfigure(ring, host, table):
    import torch
    rng = np.random.default_rng(5)
    w, h = 67, 9
    frames = [hdr_image(rng, w, h) for _ in range(5)]
    d = [up(f) for f in frames]
    ring.present_configure(2)
    s = torch.cuda.Stream()
    for k in range(5):
        t = ring.present_submit(d[k], w, h, format="linear", exposure=0.37, stream=s)
        assert t == k
        if k:
            assert (ring.present_wait(k - 1) == pack_oracle(frames[k - 1], "linear", False, 0.37, table)).all(), f"ticket {k - 1}"
    for bad in (0, 99):                                        # expired; not issued
        with pytest.raises(host.RtError) as e:
            ring.present_wait(bad)
        assert e.value.code == INVALID
        with pytest.raises(host.RtError) as e:
            ring.present_poll(bad)
        assert e.value.code == INVALID
    with pytest.raises(host.RtError) as e:                     # ticket 4 is live and has not been seen complete
        ring.present_configure(3)
    assert e.value.code == INVALID
    assert (ring.present_wait(4) == pack_oracle(frames[4], "linear", False, 0.37, table)).all()
    assert (ring.present_wait(3) == pack_oracle(frames[3], "linear", False, 0.37, table)).all()    # still live, still right
    ring.present_configure(3)                                  # drained: every live ticket has been waited for
    with pytest.raises(host.RtError) as e:                     # reconfiguring expired what was issued before
        ring.present_wait(4)
    assert e.value.code == INVALID
    t = ring.present_submit(d[0], w, h, format="srgb", stream=s)
    assert t == 5
    assert (ring.present_wait(t) == pack_oracle(frames[0], "srgb", False, 1.0, table)).all()


# ---- 6. the caller's stream ---------------------------------------------------------------------------------------------------------
def test_submit_on_the_producers_stream(ring, table):
    """The image reaches the device by a non-blocking copy on a side stream and the submit goes on that stream; the host does not
    synchronise before the wait.  A pack that did not run behind the copy would deliver the zeros the buffer held."""
    import torch
    w, h = 900, 400
    img = hdr_image(np.random.default_rng(6), w, h)
    pinned = torch.from_numpy(img).pin_memory()
    d = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d.copy_(pinned, non_blocking=True)
        t = ring.present_submit(d, w, h, format="srgb", flip=True, stream=s)
    got = ring.present_wait(t)
    assert (got == pack_oracle(img, "srgb", True, 1.0, table)).all()


# ---- 7. growth -------------------------------------------------------------------------------------------------------------------------
def test_buffers_grow_under_live_tickets(ring, table):
    """Two slots.  64x36, 640x360 (slot 1 allocates), 64x36, 64x36, then 640x360 into slot 0, whose buffers hold a small frame:
    they grow, after a host wait for that slot's own last copy.  The ticket in the other slot stays valid and right each time."""
    import torch
    rng = np.random.default_rng(7)
    small, large = (64, 36), (640, 360)
    sizes = [small, large, small, small, large]
    frames = [hdr_image(rng, w, h) for w, h in sizes]
    d = [up(f) for f in frames]
    ring.present_configure(2)
    s = torch.cuda.Stream()
    want = [pack_oracle(f, "srgb", False, 1.0, table) for f in frames]
    sub = lambda k: ring.present_submit(d[k], sizes[k][0], sizes[k][1], format="srgb", stream=s)
    assert sub(0) == 0 and sub(1) == 1
    assert (ring.present_wait(0) == want[0]).all()             # live across slot 1's allocation
    assert (ring.present_wait(1) == want[1]).all()
    assert sub(2) == 2 and sub(3) == 3
    view3 = ring.present_wait(3, copy=False)
    assert sub(4) == 4                                         # slot 0 grows under ticket 3 in slot 1
    assert (view3 == want[3]).all()
    assert (ring.present_wait(3) == want[3]).all()
    assert (ring.present_wait(4) == want[4]).all()


# ---- 8. end to end ---------------------------------------------------------------------------------------------------------------------
def test_frame_and_render_surfaces_end_to_end(ring, host, table):
    import torch
    from opengl_raytracing_amd import scenes
    sc = scenes.make_scene(2, host.generate_aabb)
    w, h = 96, 64
    p = sc.params(width=w, height=h)
    ring.load(sc)
    d_display = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ring.frame(p, d_display=d_display.data_ptr())
    t = ring.present_submit(d_display, w, h, format="srgb", flip=True)
    got = ring.present_wait(t)
    ring.sync()
    surface = d_display.cpu().numpy()
    assert np.nanmax(surface[..., :3]) > 0.05                                # a picture, not a cleared buffer
    assert (got == pack_oracle(surface, "srgb", True, 1.0, table)).all()
    ring.render(p)
    d_color = ring.get_surfaces()[0]
    t = ring.present_submit(d_color, w, h, format="srgb", flip=True)
    got = ring.present_wait(t)
    color = ring.readback()[0]
    assert (got == pack_oracle(color, "srgb", True, 1.0, table)).all()
    assert len(np.unique(got[..., :3])) > 16


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(ring, table):
    import torch
    w, h = 8, 4
    img = hdr_image(np.random.default_rng(9), w, h)
    d_img = up(img)
    d_big = torch.zeros((h * w * 4 + 64,), dtype=torch.float32, device="cuda")         # room for overlapping placements
    d_out = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    lib, ctx = ring.lib, ring.ctx
    vp = ctypes.c_void_p
    want = pack_oracle(img, "linear", False, 1.0, table)

    def desc(**kw):
        d = L.make_display_desc(w, h)
        for k, v in kw.items():
            if k == "reserved":
                d.reserved[v] = 1
            else:
                setattr(d, k, v)
        return d

    def pack(image, out, d):
        return lib.rt_display_pack(ctx, vp(image), vp(out), ctypes.byref(d) if d is not None else None, None)

    def submit(image, d, ticket=True):
        t = ctypes.c_uint64(0)
        return lib.rt_present_submit(ctx, vp(image), ctypes.byref(d) if d is not None else None, None, ctypes.byref(t) if ticket else None)

    def still_works():
        d_out.zero_()
        torch.cuda.synchronize()
        assert pack(d_img.data_ptr(), d_out.data_ptr(), desc()) == 0
        ring.sync()
        assert (d_out.cpu().numpy() == want).all()

    i, o = d_img.data_ptr(), d_out.data_ptr()
    bad_descs = [desc(exposure=0.0), desc(exposure=-1.0), desc(exposure=float("inf")), desc(exposure=float("nan")),
                 desc(format=2), desc(format=-1), desc(flags=2), desc(flags=3), desc(reserved=0), desc(reserved=1), desc(reserved=2),
                 desc(width=0), desc(width=-3), desc(height=0), desc(height=-1), None]
    for d in bad_descs:
        assert pack(i, o, d) == INVALID
        assert submit(i, d) == INVALID
        still_works()
    b = d_big.data_ptr()
    bad_ptrs = [(None, o), (i, None), (i + 4, o), (i, o + 4), (i + 8, o + 8),
                (b, b), (b, b + 16), (b, b + h * w * 16 - 16), (b + 64, b), (b + 128, b + h * w * 4 + 112)]
    for image, out in bad_ptrs:
        assert pack(image, out, desc()) == INVALID, (image, out)
        still_works()
    assert pack(b, b + h * w * 16, desc()) == 0                # adjacent, not overlapping
    assert pack(b + h * w * 4, b, desc()) == 0
    ring.sync()
    for image in (None, i + 4):
        assert submit(image, desc()) == INVALID
    assert submit(i, desc(), ticket=False) == INVALID
    for slots in (1, 9, 0, -2):
        assert lib.rt_present_configure(ctx, slots) == INVALID
    ready, px, nb = ctypes.c_int(0), vp(), ctypes.c_size_t(0)
    assert lib.rt_present_poll(ctx, 0, ctypes.byref(ready)) == INVALID          # nothing issued: every refused submit took no ticket
    assert lib.rt_present_wait(ctx, 0, ctypes.byref(px), ctypes.byref(nb)) == INVALID
    t = ring.present_submit(d_img, w, h)
    assert t == 0
    assert lib.rt_present_poll(ctx, 0, None) == INVALID
    assert lib.rt_present_wait(ctx, 0, None, ctypes.byref(nb)) == INVALID
    assert (ring.present_wait(t) == want).all()
    still_works()


# ---- 10. the ring drains itself ----------------------------------------------------------------------------------------------------------
def test_close_with_frames_in_flight(host, table):
    """Three frames submitted on a side stream to a fresh 3-slot ring -- two 67x9 RGBA8 (ragged quads, odd height), one 16x4 NV12 --
    and none waited for: close() has to drain the copy stream before the ring's buffers go.  The next context starts over at
    ticket 0 and delivers the right bytes."""
    import torch
    rng = np.random.default_rng(10)
    w, h = 67, 9
    frames = [hdr_image(rng, w, h), hdr_image(rng, w, h), hdr_image(rng, 16, 4)]
    d = [up(f) for f in frames]
    first = host.RayTracer(0)
    try:
        first.present_configure(3)
        s = torch.cuda.Stream()
        assert first.present_submit(d[0], w, h, format="srgb", flip=True, stream=s) == 0
        assert first.present_submit(d[1], w, h, format="linear", exposure=0.37, stream=s) == 1
        assert first.present_submit_yuv(d[2], 16, 4, format="nv12", stream=s) == 2
    finally:
        first.close()
    second = host.RayTracer(0)
    try:
        t = second.present_submit(d[1], w, h, format="srgb", exposure=2.5, stream=s)
        assert t == 0
        assert (second.present_wait(t) == pack_oracle(frames[1], "srgb", False, 2.5, table)).all()
    finally:
        second.close()
    s.synchronize()
