"""rt_jpeg_encode / rt_display_pack_jpeg / rt_present_submit_jpeg on the GPU (include/rt_mi355.h) against the numpy restatement of
tests/jpeg_oracle.py, bit for bit: the stream, the state record, the coefficient plane and the segment offsets.  Sizes from one
sample to 256x144 (one MCU, replicated edges, the restart index wrapping past 7), every quality and interval class, both plane
formats, inputs the oracle confirms to take each path of the entropy coder, the quantiser's division at every quotient boundary,
overflow, stream order, the shared ring -- and one 1080p frame decoded by Pillow."""
import collections
import ctypes

import numpy as np
import pytest

import jpeg_oracle as JO
import meter_oracle as MO
from opengl_raytracing_amd import layout as L

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 256
INVALID, TOO_LARGE = -1, -4


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


Device = collections.namedtuple("Device", "stream state coef seg_offsets out")


def device_encode(rt, host, planes, w, h, fmt="nv12", quality=75, interval=1, cap=None):
    """jpeg_encode of (y, cb, cr) with guard regions behind the scratch, the output and the state -> Device."""
    import torch
    lay = host.jpeg_layout(w, h, quality, interval)
    cap = lay.worst_bytes if cap is None else cap
    d_planes = up(JO.join_frame(*planes, fmt))
    d_scratch = torch.full((lay.scratch_bytes + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_out = torch.full((cap + 16 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_state = torch.full((64 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    rt.jpeg_encode(d_planes, d_scratch, d_out, cap, d_state, w, h, fmt, quality, interval)
    torch.cuda.synchronize()
    scratch, out, state = d_scratch.cpu().numpy(), d_out.cpu().numpy(), d_state.cpu().numpy()
    assert (scratch[lay.scratch_bytes:] == SENTINEL).all(), "written behind the scratch"
    assert (out[cap:] == SENTINEL).all(), "written behind dOut + capBytes"
    assert (state[64:] == SENTINEL).all(), "written behind the state"
    st = state[:64].view(L.JPEG_STATE_DTYPE)[0]
    coef = scratch[lay.offset[0]: lay.offset[0] + lay.n_mcu * 768].view(np.int16).reshape(-1, 64)
    seg = scratch[lay.offset[1]: lay.offset[1] + 4 * (lay.n_segments + 1)].view(np.uint32)
    return Device(out[:int(st["bytes"])], state[:64].view(np.uint32), coef, seg, out[:cap])


def check(got, want, where=""):
    """Stage by stage, so that a failure names the first stage that differs."""
    assert got.coef.shape == want.coef.shape and (got.coef == want.coef).all(), (where, "coefficient plane", np.argwhere(got.coef != want.coef)[:4])
    assert (got.seg_offsets == want.seg_offsets).all(), (where, "segment offsets", got.seg_offsets[:8], want.seg_offsets[:8])
    assert (got.state == want.state).all(), (where, "state", got.state[:8], want.state[:8])
    assert got.stream.size == want.stream.size and (got.stream == want.stream).all(), (where, "stream", np.nonzero(got.stream != want.stream)[0][:8])


# ---- 1. parity: sizes, qualities, intervals, formats ------------------------------------------------------------------------------------
SIZES = [(1, 1), (16, 16), (17, 17), (37, 19), (64, 48), (129, 65), (256, 144)]


def settings(w, h):
    """(quality, interval, format): every quality, every interval class and both formats meet every size, cycled rather than crossed."""
    n_mcu = JO.geometry(w, h, 1)[2]
    intervals = [1, 2, 7, n_mcu, 65535]
    return [(q, intervals[(k + w) % 5], ("nv12", "i420")[(k + h) % 2]) for k, q in enumerate((1, 50, 90, 100))] + \
        [(75, iv, ("i420", "nv12")[k % 2]) for k, iv in enumerate(intervals)]


def test_settings_cover_every_option():
    seen = [s for w, h in SIZES for s in settings(w, h)]
    assert {q for q, _, _ in seen} >= {1, 50, 90, 100} and {f for _, _, f in seen} == {"nv12", "i420"}
    for w, h in SIZES:
        n_mcu = JO.geometry(w, h, 1)[2]
        assert {iv for _, iv, _ in settings(w, h)} == {1, 2, 7, n_mcu, 65535}


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_encode_matches_numpy(rt, host, w, h):
    planes = JO.content("noise", w, h, seed=1000 * w + h)
    if (w, h) == (17, 17):
        planes = JO.content("ramp", w, h)                          # three of four MCUs are mostly replicated edge: a picture, so that the edge matters
    for quality, interval, fmt in settings(w, h):
        want = JO.encode(*planes, quality, interval)
        check(device_encode(rt, host, planes, w, h, fmt, quality, interval), want, (quality, interval, fmt))
    if (w, h) == (64, 48):
        want = JO.encode(*planes, 75, 1)
        assert want.stats["rst"] == 11 >= 9 and want.stream[629 + want.seg_offsets[9] - 1] == 0xD0     # the ninth marker wrapped to RST0
        assert want.stream[629 + want.seg_offsets[8] - 1] == 0xD7 and want.stream[629 + want.seg_offsets[8] - 2] == 0xFF


# ---- 2. contents that take each path of the entropy coder ---------------------------------------------------------------------------------
def test_noise_at_quality_100_stuffs_bytes_and_reaches_the_largest_categories(rt, host):
    w, h = 64, 48
    planes = JO.content("binary", w, h, seed=1)
    want = JO.encode(*planes, 100, 2)
    assert want.stats["stuffed"] > 0 and want.stats["max_ac_cat"] == 10 and want.state[6] == want.stats["stuffed"]
    check(device_encode(rt, host, planes, w, h, "nv12", 100, 2), want)
    planes = JO.content("blocks", w, h)
    want = JO.encode(*planes, 100, 65535)
    assert want.stats["max_dc_cat"] == 11
    check(device_encode(rt, host, planes, w, h, "i420", 100, 65535), want)
    planes = JO.content("noise", 129, 65, seed=9)
    want = JO.encode(*planes, 100, 7)
    assert want.stats["stuffed"] > 0
    check(device_encode(rt, host, planes, 129, 65, "nv12", 100, 7), want)


def test_checkerboard_needs_zrl(rt, host):
    for quality, (w, h) in ((1, (64, 48)), (50, (37, 19)), (100, (33, 17))):
        planes = JO.content("checker", w, h)
        want = JO.encode(*planes, quality, 1)
        if quality == 1:
            assert want.stats["zrl"] > 0
        check(device_encode(rt, host, planes, w, h, "nv12", quality, 1), want, quality)


def test_black_is_eob_only(rt, host):
    for kind in ("black", "white"):
        planes = JO.content(kind, 37, 19)
        want = JO.encode(*planes, 50, 2)
        assert want.stats["eob"] == want.coef.shape[0] and want.stats["max_ac_cat"] == 0 and want.stats["zrl"] == 0
        check(device_encode(rt, host, planes, 37, 19, "i420", 50, 2), want, kind)


# ---- 3. the quantiser's division ----------------------------------------------------------------------------------------------------------
def sweep_planes():
    """2048 x 1024: 32768 luma and 2 x 8192 chroma blocks.  Family A: a constant s with the first j samples one higher -- the DC
    coefficient takes every value it can.  Family B: amplitude a times the sign pattern of basis function (v, u), both signs -- every
    coefficient position is driven from 0 to its bound."""
    m = JO.dct_matrix()
    ramp = (np.arange(64)[None, :] < np.arange(64)[:, None]).reshape(64, 8, 8)                    # [j]: the first j samples set
    fam_a = (np.arange(255)[:, None, None, None] + ramp[None]).reshape(-1, 8, 8)                   # 16320 blocks
    sign = np.array([np.where(np.outer(m[v], m[u]) > 0, 1, -1) for v in range(8) for u in range(8)])      # [64, 8, 8]
    amp = np.arange(128)[None, :, None, None]
    fam_b = np.concatenate([(128 + amp * sign[:, None]).reshape(-1, 8, 8), (127 - amp * sign[:, None]).reshape(-1, 8, 8)])   # 2 x 8192
    luma = np.concatenate([fam_a, fam_b, np.full((32768 - 16320 - 16384, 8, 8), 128)])
    cb = fam_b[:8192]
    cr = np.concatenate([fam_a[::2], np.full((8192 - 8160, 8, 8), 128)])
    assert luma.min() >= 0 and luma.max() <= 255 and cb.max() <= 255 and cb.min() >= 0
    mw, mh = 128, 64
    y = luma.reshape(mh, mw, 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(mh * 16, mw * 16)
    plane = lambda b: b.reshape(mh, mw, 8, 8).transpose(0, 2, 1, 3).reshape(mh * 8, mw * 8)
    return y.astype(np.uint8), plane(cb).astype(np.uint8), plane(cr).astype(np.uint8)


def test_quantiser_division_at_every_quotient_boundary(rt, host):
    planes = sweep_planes()
    w, h = 2048, 1024
    F = JO.fdct(JO.blocks_of(*planes)).reshape(-1, 6, 64)
    absF = np.abs(F)
    assert absF[:, :, 1:].max() <= 1020 and F[:, :, 0].min() == -1024 and F[:, :, 0].max() == 1016
    assert set(np.unique(absF[:, :4, 0])) >= set(range(0, 1017))                 # every DC magnitude, in luma
    for pos in range(1, 64):
        assert absF[:, :4, pos].max() >= 800, pos                               # every AC position driven far up its range
    for quality in (1, 50, 100):
        tables = JO.quant(quality)
        if quality in (1, 100):
            for comp, blocks in ((0, slice(0, 4)), (1, slice(4, 6))):
                for Q in sorted(set(tables[comp])):                             # every Q value of the table ...
                    positions = [i for i in range(64) if tables[comp][i] == Q]
                    seen = set(np.unique(absF[:, blocks][:, :, positions]))
                    for k in range(1, (1000 + (Q >> 1)) // Q + 1):              # ... meets both sides of every quotient boundary up to |F| = 1000
                        edge = k * Q - (Q >> 1)
                        assert edge in seen and (edge - 1 in seen or edge == 0), (quality, comp, Q, k)
        import torch
        lay = host.jpeg_layout(w, h, quality, 128)
        d_planes = up(JO.join_frame(*planes, "i420"))
        d_scratch = torch.zeros((lay.scratch_bytes,), dtype=torch.uint8, device="cuda")
        d_out = torch.zeros((16,), dtype=torch.uint8, device="cuda")
        d_state = torch.zeros((64,), dtype=torch.uint8, device="cuda")
        rt.jpeg_encode(d_planes, d_scratch, d_out, 16, d_state, w, h, "i420", quality, 128)       # (overflows: the coefficient plane is complete all the same)
        torch.cuda.synchronize()
        got = d_scratch.cpu().numpy()[: lay.n_mcu * 768].view(np.int16).reshape(-1, 64)
        want = JO.coefficients(*planes, quality)
        assert (got == want).all(), (quality, np.argwhere(got != want)[:4])
        assert d_state.cpu().numpy().view(L.JPEG_STATE_DTYPE)[0]["overflow"] == 1


# ---- 4. overflow -------------------------------------------------------------------------------------------------------------------------
def test_overflow_reports_the_exact_size_and_writes_nothing(rt, host):
    w, h = 37, 19
    planes = JO.content("noise", w, h, seed=77)
    want = JO.encode(*planes, 90, 2)
    need = int(want.stream.size)
    got = device_encode(rt, host, planes, w, h, "nv12", 90, 2, cap=need)          # exactly enough
    check(got, want)
    for cap in (need - 1, 629, 100, 0):
        got = device_encode(rt, host, planes, w, h, "nv12", 90, 2, cap=cap)       # (asserts the canaries behind dOut + cap and the scratch)
        st = got.state.view(L.JPEG_STATE_DTYPE)[0]
        assert (st["bytes"], st["needed"], st["overflow"]) == (0, need, 1), cap
        assert (st["nSegments"], st["nMcu"], st["headerBytes"], st["stuffedBytes"]) == tuple(int(v) for v in want.state[3:7])
        assert (got.out == SENTINEL).all(), cap                                   # not one byte of dOut
        assert (got.coef == want.coef).all() and (got.seg_offsets == want.seg_offsets).all()


# ---- 5. stream behaviour -------------------------------------------------------------------------------------------------------------------
def pack_jpeg(rt, host, d_img, w, h, cap=None, **kw):
    import torch
    lay = host.jpeg_layout(w, h, kw.get("quality", 90), kw.get("restart_interval"))
    cap = lay.worst_bytes if cap is None else cap
    d_scratch = torch.full((lay.scratch_bytes + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_out = torch.full((cap + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_state = torch.zeros((64,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rt.display_pack_jpeg(d_img, d_scratch, d_out, cap, d_state, w, h, **kw)
    return lay, cap, d_scratch, d_out, d_state


def test_pack_jpeg_is_pack_yuv_then_encode(rt, host, table):
    import torch
    for (w, h), fmt, flip in (((67, 9), "nv12", True), ((40, 24), "i420", False)):
        img = MO.hdr_image(np.random.default_rng(w), w, h)
        d_img = up(img)
        lay, cap, d_scratch, d_out, d_state = pack_jpeg(rt, host, d_img, w, h, format=fmt, quality=90, restart_interval=2, flip=flip, exposure=0.37,
                                                        tone="aces")
        d_yuv = torch.zeros((host.yuv_layout(w, h, fmt).bytes,), dtype=torch.uint8, device="cuda")
        rt.display_pack_yuv(d_img, d_yuv, w, h, format=fmt, matrix="bt601", range="full", flip=flip, exposure=0.37, tone="aces")
        torch.cuda.synchronize()
        planes = JO.split_frame(d_yuv.cpu().numpy(), w, h, fmt)
        two_step = device_encode(rt, host, planes, w, h, fmt, 90, 2)
        check(two_step, JO.encode(*planes, 90, 2))
        st = d_state.cpu().numpy().view(L.JPEG_STATE_DTYPE)[0]
        out, scratch = d_out.cpu().numpy(), d_scratch.cpu().numpy()
        assert (out[cap:] == SENTINEL).all() and (scratch[lay.scratch_bytes:] == SENTINEL).all()
        assert st["bytes"] == two_step.stream.size and (out[:st["bytes"]] == two_step.stream).all()


def test_encode_is_ordered_behind_a_render_on_the_callers_stream(ring, host, table):
    import torch
    from opengl_raytracing_amd import scenes
    sc = scenes.make_scene(2, host.generate_aabb)
    w, h = 96, 64
    p = sc.params(width=w, height=h)
    ring.load(sc)
    d_color = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    d_pos = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    d_normal = torch.zeros((h, w, 2), dtype=torch.int32, device="cuda")
    lay = host.jpeg_layout(w, h, 90, 6)
    d_scratch = torch.zeros((lay.scratch_bytes,), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros((lay.worst_bytes,), dtype=torch.uint8, device="cuda")
    d_state = torch.zeros((64,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ring.render_to(p, d_color.data_ptr(), d_pos.data_ptr(), d_normal.data_ptr(), stream=s.cuda_stream)
        ring.display_pack_jpeg(d_color, d_scratch, d_out, lay.worst_bytes, d_state, w, h, quality=90, restart_interval=6, stream=s)
    s.synchronize()
    surface = d_color.cpu().numpy()
    assert np.nanmax(surface[..., :3]) > 0.05                                  # a picture, not the cleared buffer
    import yuv_oracle as YO
    planes = JO.split_frame(YO.pack_yuv(surface, table, "nv12", "bt601", "full", flip=True), w, h, "nv12")
    want = JO.encode(*planes, 90, 6)
    st = d_state.cpu().numpy().view(L.JPEG_STATE_DTYPE)[0]
    assert st["bytes"] == want.stream.size and (d_out.cpu().numpy()[:st["bytes"]] == want.stream).all()


def jpeg_of(img, table, w, h, fmt="nv12", quality=90, interval=None, **kw):
    """What present_submit_jpeg should deliver for a surface: the YUV oracle's planes through the JPEG oracle."""
    import yuv_oracle as YO
    interval = L.JPEG_DEFAULT_INTERVAL if interval is None else interval
    planes = JO.split_frame(YO.pack_yuv(img, table, fmt, "bt601", "full", flip=kw.pop("flip", True), **kw), w, h, fmt)
    return JO.encode(*planes, quality, interval).stream


def test_one_ring_serves_jpeg_rgba8_and_yuv(ring, host, table):
    import torch
    import yuv_oracle as YO
    w, h = 67, 9
    rng = np.random.default_rng(41)
    frames = [MO.hdr_image(rng, w, h) for _ in range(5)]
    d = [up(f) for f in frames]
    ring.present_configure(5)
    s = torch.cuda.Stream()
    t = [ring.present_submit_jpeg(d[0], w, h, quality=90, stream=s),
         ring.present_submit(d[1], w, h, format="srgb", exposure=0.37, stream=s),
         ring.present_submit_jpeg(d[2], w, h, cap_bytes=4096, format="i420", quality=50, restart_interval=1, flip=False, stream=s),
         ring.present_submit_yuv(d[3], w, h, format="nv12", stream=s),
         ring.present_submit_jpeg(d[4], w, h, quality=100, restart_interval=65535, exposure=0.37, tone="reinhard", white=4.0, stream=s)]
    assert t == [0, 1, 2, 3, 4]
    px, nb = ctypes.c_void_p(), ctypes.c_size_t(0)
    assert ring.lib.rt_present_wait(ring.ctx, 2, ctypes.byref(px), ctypes.byref(nb)) == 0 and nb.value == 64 + 4096
    assert ring.lib.rt_present_wait(ring.ctx, 0, ctypes.byref(px), ctypes.byref(nb)) == 0 and nb.value == 64 + host.jpeg_layout(w, h).worst_bytes
    got = ring.present_wait_jpeg(4)
    assert (got == jpeg_of(frames[4], table, w, h, quality=100, interval=65535, exposure=0.37, tone="reinhard", white=4.0)).all()
    assert (ring.present_wait(1) == MO.pack_toned(frames[1], "srgb", False, 0.37, table)).all()
    got = ring.present_wait_jpeg(2, copy=False)
    assert not got.flags.writeable and (got == jpeg_of(frames[2], table, w, h, "i420", 50, 1, flip=False)).all()
    assert (np.concatenate([p.reshape(-1) for p in ring.present_wait_yuv(3)]) == YO.pack_yuv(frames[3], table, "nv12")).all()
    got = ring.present_wait_jpeg(0)
    assert got.dtype == np.uint8 and (got == jpeg_of(frames[0], table, w, h)).all()
    for wrong in (ring.present_wait, ring.present_wait_yuv):
        with pytest.raises(ValueError, match="JPEG"):
            wrong(0)
    for ticket in (1, 3):
        with pytest.raises(ValueError, match="JPEG"):
            ring.present_wait_jpeg(ticket)


def test_slot_grows_and_a_small_cap_overflows(ring, host, table):
    import torch
    rng = np.random.default_rng(47)
    small, large = (64, 36), (320, 180)
    frames = [MO.hdr_image(rng, *small), MO.hdr_image(rng, *small), MO.hdr_image(rng, *large)]
    d = [up(f) for f in frames]
    ring.present_configure(2)
    s = torch.cuda.Stream()
    assert ring.present_submit_jpeg(d[0], *small, stream=s) == 0
    assert ring.present_submit_jpeg(d[1], *small, cap_bytes=700, stream=s) == 1            # header and little else: overflows
    want0 = jpeg_of(frames[0], table, *small)
    assert (ring.present_wait_jpeg(0) == want0).all()
    need1 = jpeg_of(frames[1], table, *small).size
    with pytest.raises(host.RtError, match=str(need1)):
        ring.present_wait_jpeg(1)
    assert ring.present_submit_jpeg(d[2], *large, stream=s) == 2                            # slot 0 and the context's scratch grow
    assert (ring.present_wait_jpeg(2) == jpeg_of(frames[2], table, *large)).all()
    assert ring.present_submit_jpeg(d[0], *small, stream=s) == 3                            # a small frame into the grown buffers
    assert (ring.present_wait_jpeg(3) == want0).all()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(ring, host, table):
    import torch
    w, h = 37, 19
    planes = JO.content("ramp", w, h)
    want = JO.encode(*planes, 75, 2)
    lay = host.jpeg_layout(w, h, 75, 2)
    d_planes = up(JO.join_frame(*planes, "nv12"))
    d_img = up(MO.hdr_image(np.random.default_rng(3), w, h))
    d_scratch = torch.zeros((lay.scratch_bytes + 64,), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros((lay.worst_bytes,), dtype=torch.uint8, device="cuda")
    d_state = torch.zeros((128,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    lib, ctx, vp = ring.lib, ring.ctx, ctypes.c_void_p
    ref = lambda x: ctypes.byref(x) if x is not None else None
    P, S, O, T, I = d_planes.data_ptr(), d_scratch.data_ptr(), d_out.data_ptr(), d_state.data_ptr(), d_img.data_ptr()
    cap = lay.worst_bytes

    def jd(**kw):
        d = L.make_jpeg_desc(w, h, 75, 2)
        for k, v in kw.items():
            if k == "reserved":
                d.reserved[v] = 1
            else:
                setattr(d, k, v)
        return d

    def yd(**kw):
        d = L.make_yuv_desc(w, h, "nv12", "bt601", "full")
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def encode(planes=P, y=yd(), j=jd(), scratch=S, out=O, cap=cap, state=T, context=True):
        return lib.rt_jpeg_encode(ctx if context else None, vp(planes), ref(y), ref(j), vp(scratch), vp(out), cap, vp(state), None)

    def pack(image=I, y=yd(), j=jd(), scratch=S, out=O, cap=cap, state=T, context=True):
        return lib.rt_display_pack_jpeg(ctx if context else None, vp(image), ref(y), None, ref(j), vp(scratch), vp(out), cap, vp(state), None)

    def submit(image=I, y=yd(), j=jd(), ticket=True, context=True):
        k = ctypes.c_uint64(0)
        return lib.rt_present_submit_jpeg(ctx if context else None, vp(image), ref(y), None, ref(j), 0, None, ctypes.byref(k) if ticket else None)

    def still_works():
        d_out.zero_()
        torch.cuda.synchronize()
        assert encode() == 0
        ring.sync()
        assert (d_out.cpu().numpy()[:want.stream.size] == want.stream).all()

    still_works()
    bad_j = [jd(width=0), jd(width=65536), jd(height=0), jd(height=-1), jd(quality=0), jd(quality=101), jd(restartInterval=0),
             jd(restartInterval=65536), jd(reserved=0), jd(reserved=3), jd(width=w + 1), jd(height=h - 1), None]
    for k, j in enumerate(bad_j):
        assert encode(j=j) == INVALID and pack(j=j) == INVALID and submit(j=j) == INVALID, k
    still_works()
    for k, y in enumerate([yd(format=2), yd(format=-1), yd(width=w + 1), None]):
        assert encode(y=y) == INVALID and pack(y=y) == INVALID and submit(y=y) == INVALID, k
    for k, y in enumerate([yd(matrix=L.YUV_BT709), yd(range=L.YUV_LIMITED), yd(exposure=0.0), yd(flags=2), yd(transfer=5)]):
        assert pack(y=y) == INVALID and submit(y=y) == INVALID, k                  # a JFIF file cannot say otherwise; the pack's own refusals
    assert encode(y=yd(matrix=L.YUV_BT709, range=L.YUV_LIMITED, exposure=0.0)) == 0   # the encoder reads the planes' size and format only
    ring.sync()
    for kw in (dict(planes=None), dict(scratch=None), dict(out=None), dict(state=None), dict(planes=P + 4), dict(scratch=S + 8), dict(out=O + 4),
               dict(state=T + 4), dict(context=False)):
        assert encode(**kw) == INVALID, kw
    for kw in (dict(image=None), dict(image=I + 4), dict(scratch=None), dict(out=O + 8), dict(state=None), dict(context=False)):
        assert pack(**kw) == INVALID, kw
    assert submit(image=None) == INVALID and submit(image=I + 4) == INVALID and submit(ticket=False) == INVALID and submit(context=False) == INVALID
    overlapping = [dict(out=S), dict(out=S + lay.scratch_bytes - 16), dict(state=S + 16), dict(state=O), dict(state=O + cap - 16), dict(planes=S),
                   dict(planes=O), dict(out=T - 16, cap=32), dict(scratch=P)]
    for kw in overlapping:
        assert encode(**kw) == INVALID, kw
    assert encode(state=S + lay.scratch_bytes) == 0                            # adjacent, not overlapping
    ring.sync()
    assert pack(out=I) == INVALID and pack(scratch=I) == INVALID and pack(state=I + 16) == INVALID
    huge = jd(width=65535, height=65535)
    assert encode(j=huge, y=yd(width=65535, height=65535)) == TOO_LARGE
    still_works()
    ready = ctypes.c_int(0)
    assert lib.rt_present_poll(ctx, 0, ctypes.byref(ready)) == INVALID          # every refused submit took no ticket
    assert pack() == 0 and submit() == 0
    ring.sync()


# ---- 7. frame scale ------------------------------------------------------------------------------------------------------------------------
def test_1080p_frame_decodes_as_well_as_pillows(ring, host, table):
    pytest.importorskip("PIL")
    import torch
    from opengl_raytracing_amd import scenes
    sc = scenes.make_scene(2, host.generate_aabb)
    w, h = 1920, 1080
    p = sc.params(width=w, height=h)
    ring.load(sc)
    d_display = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    d_yuv = torch.zeros((host.yuv_layout(w, h, "nv12").bytes,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ring.frame(p, d_display=d_display.data_ptr())
    t = ring.present_submit_jpeg(d_display, w, h, cap_bytes=4 << 20, quality=90)
    ring.display_pack_yuv(d_display, d_yuv, w, h, format="nv12", matrix="bt601", range="full", flip=True)
    stream = ring.present_wait_jpeg(t)
    ring.sync()
    torch.cuda.synchronize()
    y, cb, cr = JO.split_frame(d_yuv.cpu().numpy(), w, h, "nv12")
    assert len(np.unique(y)) > 16                                              # a picture
    assert stream[:2].tolist() == [0xFF, 0xD8] and stream[-2:].tolist() == [0xFF, 0xD9]
    assert (stream[:629] == JO.header(w, h, 90, L.JPEG_DEFAULT_INTERVAL)).all()
    planes = JO.decode_planes(stream)
    assert planes[0].shape == (h, w)
    ours, theirs = JO.luma_rms(stream, y), JO.luma_rms(JO.pillow_encode(y, cb, cr, 90), y)
    print(f"1080p C2 q90: {stream.size} bytes, luma rms {ours:.4f}, Pillow's {theirs:.4f}")
    assert ours <= theirs * 1.02 + 0.5, (ours, theirs)
