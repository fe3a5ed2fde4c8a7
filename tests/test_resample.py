"""rt_display_resample on the GPU (include/rt_mi355.h) against the numpy restatement of tests/resample_oracle.py fed with the
library's own tables (host.resample_taps): every comparison is equality of float32 bit patterns (NaN payloads set aside).
Shapes reach a single-pixel tile, ragged tiles on both edges, several tiles per axis, clamping on all four borders and every
tile form the host can pick (test_plan_covers_every_tile_form)."""
import ctypes

import numpy as np
import pytest

import resample_oracle as RO
from opengl_raytracing_amd import layout as L
from test_present import pack_oracle

pytestmark = pytest.mark.gpu

INVALID, TOO_LARGE = -1, -4
FILTER_NAMES = ("area", "triangle", "lanczos3")
SHAPES = [((1, 1), (1, 1)), ((1, 1), (5, 3)), ((7, 5), (1, 1)), ((8, 8), (4, 4)), ((64, 32), (32, 16)), ((67, 9), (33, 5)),
          ((33, 5), (67, 9)), ((16, 4), (16, 4)), ((257, 3), (64, 7)), ((640, 4), (64, 4)), ((640, 360), (213, 120)), ((96, 54), (640, 360))]
# vertical ratios of 4, 5 and 10: the tile forms the shapes above do not reach (two rows, one row, one row of 32 columns)
TALL = [((6, 128), (6, 32)), ((5, 200), (5, 40)), ((70, 640), (70, 64))]
GUARD = 64                                       # float32 words in front of and behind the destination
SENTINEL = np.float32(-1234.5)


def ident(shape):
    (sw, sh), (dw, dh) = shape
    return f"{sw}x{sh}-{dw}x{dh}"


def tile_form(first_y, n_y, src_h, dst_h):
    """(columns, rows) of the destination tile the host picks: the tallest tile of 64 columns whose clamped row span, times the
    columns, fits 2048 float4 of LDS in every tile row; else 32 columns x 1 row (the rule of csrc/rt_resample.h, restated)."""
    for tw, th in ((64, 16), (64, 8), (64, 4), (64, 2), (64, 1), (32, 1)):
        rows = 0
        for j0 in range(0, dst_h, th):
            j1 = min(j0 + th, dst_h) - 1
            lo = min(max(int(first_y[j0]), 0), src_h - 1)
            hi = min(max(int(first_y[j1]) + n_y - 1, 0), src_h - 1)
            rows = max(rows, hi - lo + 1)
        if rows * tw <= 2048:
            return tw, th
    raise AssertionError("no tile form fits")


def test_plan_covers_every_tile_form(host):
    seen = {}
    for shape in SHAPES + TALL:
        (sw, sh), (dw, dh) = shape
        for f in FILTER_NAMES:
            n, first, _ = host.resample_taps(sh, dh, f)
            seen.setdefault(tile_form(first, n, sh, dh), []).append((ident(shape), f))
    assert set(seen) == {(64, 16), (64, 8), (64, 4), (64, 2), (64, 1), (32, 1)}, sorted(seen)
    assert any(dw > 64 and dw % 64 for (_, _), (dw, _) in SHAPES) and any(dh % 16 for (_, _), (_, dh) in SHAPES)     # ragged both ways
    assert any(dw > 32 and dw % 32 for (_, _), (dw, _) in TALL)


@pytest.fixture(scope="module")
def rt(host):
    t = host.RayTracer(0)
    yield t
    t.close()


def hdr_image(rng, w, h):
    """Log-normal magnitudes over about 2^-20 .. 2^20 in every channel, a quarter of them negative, with +-0 and denormals planted."""
    img = np.exp2(np.clip(rng.normal(0.0, 7.0, (h, w, 4)), -20.0, 20.0)).astype(np.float32)
    img[rng.uniform(size=img.shape) < 0.25] *= np.float32(-1)
    flat = img.reshape(-1)
    specials = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1.1754942e-38], dtype=np.float32)
    for k, v in enumerate(specials[: flat.size]):
        flat[(k * 7919 + 3) % flat.size if flat.size > len(specials) else k] = v
    return img


def up(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def same_bits(a, b):
    """Equal float32 bit patterns, NaN matching NaN whatever its payload."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def resampled(rt, d_src, shape, f, stream=None):
    """rt.resample into a destination between two guard regions -> the destination, [dh, dw, 4]."""
    import torch
    (sw, sh), (dw, dh) = shape
    n = dw * dh * 4
    buf = torch.full((n + 2 * GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rt.resample(d_src, buf.data_ptr() + 4 * GUARD, sw, sh, dw, dh, filter=f, stream=stream)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + n:] == SENTINEL).all(), f"guard region written ({ident(shape)}, {f})"
    return got[GUARD: GUARD + n].reshape(dh, dw, 4)


def expected(host, img, shape, f):
    (sw, sh), (dw, dh) = shape
    return RO.resample(img, host.resample_taps(sw, dw, f), host.resample_taps(sh, dh, f))


# ---- 1. exactness, guards, determinism -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + TALL, ids=ident)
def test_resample_matches_numpy_bit_for_bit(rt, host, shape):
    (sw, sh), (dw, dh) = shape
    img = hdr_image(np.random.default_rng(9000 * sw + sh), sw, sh)
    d_src = up(img)
    for f in FILTER_NAMES:
        got = resampled(rt, d_src, shape, f)
        want = expected(host, img, shape, f)
        assert np.isfinite(want).all()
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (f, len(bad), bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])
        again = resampled(rt, d_src, shape, f)
        assert again.tobytes() == got.tobytes(), f


# ---- 2. non-finite texels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [((67, 9), (33, 5)), ((33, 5), (67, 9)), ((16, 4), (16, 4))], ids=ident)
def test_non_finite_texels_poison_their_windows(rt, host, shape):
    (sw, sh), (dw, dh) = shape
    img = hdr_image(np.random.default_rng(77 * sw + sh), sw, sh)
    img[sh // 2, sw // 2, 1] = np.nan                          # interior
    img[0, 0, 0] = np.inf                                      # a corner: the clamp replicates it
    img[sh - 1, sw // 3, 2] = -np.inf                          # the top edge
    d_src = up(img)
    for f in FILTER_NAMES:
        got, want = resampled(rt, d_src, shape, f), expected(host, img, shape, f)
        assert np.isnan(want).any() and (np.isnan(got) == np.isnan(want)).all(), f
        assert same_bits(got, want), f
        if f != "lanczos3":
            assert np.isinf(want).any(), f                      # (Lanczos' zero and negative weights turn an infinity's windows to NaN)


# ---- 3. identity ------------------------------------------------------------------------------------------------------------------------
def test_equal_sizes_copy(rt):
    shape = ((16, 4), (16, 4))
    img = hdr_image(np.random.default_rng(5), 16, 4)
    d_src = up(img)
    for f in ("area", "triangle"):
        assert resampled(rt, d_src, shape, f).tobytes() == img.tobytes(), f
    assert (resampled(rt, d_src, shape, "lanczos3") == img).all()          # equal values: -0 + 0 is +0


# ---- 4. the caller's stream -------------------------------------------------------------------------------------------------------------
def test_resample_on_the_producers_stream(rt, host):
    """The source reaches the device by a non-blocking copy on a side stream, the resample goes on that stream and its result
    leaves by a non-blocking copy behind it; the host waits once, at the end.  A pass that ran anywhere but behind the copy on that
    stream would read the zeros the buffer held; one the stream did not wait for would not have written the output in time."""
    import torch
    shape = ((900, 400), (450, 200))
    (sw, sh), (dw, dh) = shape
    img = hdr_image(np.random.default_rng(6), sw, sh)
    pinned = torch.from_numpy(img).pin_memory()
    d_src = torch.zeros((sh, sw, 4), dtype=torch.float32, device="cuda")
    d_dst = torch.full((dh, dw, 4), float("nan"), dtype=torch.float32, device="cuda")
    h_dst = torch.zeros((dh, dw, 4), dtype=torch.float32).pin_memory()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_src.copy_(pinned, non_blocking=True)
        rt.resample(d_src, d_dst, sw, sh, dw, dh, filter="area", stream=s)
        h_dst.copy_(d_dst, non_blocking=True)
    s.synchronize()
    assert same_bits(h_dst.numpy(), expected(host, img, shape, "area"))


# ---- 5. the tables are rebuilt under way ------------------------------------------------------------------------------------------
def test_tables_follow_the_shape(host):
    """A, B, A on one fresh context without a host wait in between: each launch reads the tables of its own shape."""
    import torch
    a, b = ((640, 360), (213, 120)), ((96, 54), (640, 360))
    rng = np.random.default_rng(8)
    img = {a: hdr_image(rng, 640, 360), b: hdr_image(rng, 96, 54)}
    d_src = {k: up(v) for k, v in img.items()}
    order = [(a, "lanczos3"), (b, "triangle"), (a, "lanczos3"), (a, "area")]
    outs = [torch.zeros((shape[1][1], shape[1][0], 4), dtype=torch.float32, device="cuda") for shape, _ in order]
    torch.cuda.synchronize()
    with host.RayTracer(0) as t:
        for (shape, f), d_out in zip(order, outs):
            (sw, sh), (dw, dh) = shape
            t.resample(d_src[shape], d_out, sw, sh, dw, dh, filter=f)
        t.sync()
        torch.cuda.synchronize()
        for (shape, f), d_out in zip(order, outs):
            assert same_bits(d_out.cpu().numpy(), expected(host, img[shape], shape, f)), (ident(shape), f)


# ---- 6. render -> resample -> present -----------------------------------------------------------------------------------------------
def test_render_resample_present_chain(host):
    import os
    import torch
    from conftest import GOLDEN_DIR
    objs, lts = host.parse_scene(open(os.path.join(GOLDEN_DIR, "scenes", "SIMPLE.scene")).read())
    shape = ((128, 72), (64, 36))
    (sw, sh), (dw, dh) = shape
    p = L.make_params(sw, sh, 4, cam_pos=(0.0, 2.0, 9.0))
    d_small = torch.zeros((dh, dw, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with host.RayTracer(0) as t:
        t.set_scene(objs, lts)
        t.render(p)
        d_color = t.get_surfaces()[0]
        t.resample(d_color, d_small, sw, sh, dw, dh, filter="area")
        ticket = t.present_submit(d_small, dw, dh, format="srgb")
        got = t.present_wait(ticket)
        color = t.readback()[0]
    small = RO.resample(color, host.resample_taps(sw, dw, "area"), host.resample_taps(sh, dh, "area"))
    assert (got == pack_oracle(small, "srgb", False, 1.0, host.display_srgb_thresholds())).all()
    assert len(np.unique(got[..., :3])) > 16                                  # a picture, not a cleared buffer


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(host):
    import torch
    from opengl_raytracing_amd import scenes
    sw, sh, dw, dh = 8, 4, 4, 2
    img = hdr_image(np.random.default_rng(9), sw, sh)
    d_src = up(img)
    d_dst = torch.zeros((dh, dw, 4), dtype=torch.float32, device="cuda")
    d_big = torch.zeros((2 * sw * sh * 4 + 64,), dtype=torch.float32, device="cuda")          # room for overlapping placements
    d_huge = torch.zeros((650 * 4 * 4,), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    vp = ctypes.c_void_p
    want = expected(host, img, ((sw, sh), (dw, dh)), "triangle")
    with host.RayTracer(0) as t:
        lib, ctx = t.lib, t.ctx

        def desc(**kw):
            d = L.make_resample_desc(sw, sh, dw, dh, "triangle")
            for k, v in kw.items():
                if k == "reserved":
                    d.reserved[v] = 1
                else:
                    setattr(d, k, v)
            return d

        def call(src, dst, d):
            return lib.rt_display_resample(ctx, vp(src), vp(dst), ctypes.byref(d) if d is not None else None, None)

        def still_works():
            d_dst.zero_()
            torch.cuda.synchronize()
            assert call(d_src.data_ptr(), d_dst.data_ptr(), desc()) == 0
            t.sync()
            assert same_bits(d_dst.cpu().numpy(), want)

        still_works()
        s, o = d_src.data_ptr(), d_dst.data_ptr()
        bad_descs = [desc(filter=3), desc(filter=-1), desc(flags=1), desc(flags=0x80000000), desc(reserved=0), desc(reserved=1),
                     desc(srcWidth=0), desc(srcHeight=0), desc(dstWidth=0), desc(dstHeight=0), desc(srcWidth=-8), desc(dstHeight=-2), None]
        for d in bad_descs:
            assert call(s, o, d) == INVALID
            still_works()
        assert lib.rt_display_resample(None, vp(s), vp(o), ctypes.byref(desc()), None) == INVALID
        b = d_big.data_ptr()
        nsrc, ndst = sw * sh * 16, dw * dh * 16
        bad_ptrs = [(None, o), (s, None), (s + 4, o), (s, o + 4), (s + 8, o + 8), (b, b), (b, b + 16), (b, b + nsrc - 16), (b + ndst - 16, b)]
        for src, dst in bad_ptrs:
            assert call(src, dst, desc()) == INVALID, (src, dst)
            still_works()
        assert call(b, b + nsrc, desc()) == 0 and call(b + ndst, b, desc()) == 0          # adjacent, not overlapping
        t.sync()
        h = d_huge.data_ptr()
        for d in (L.make_resample_desc(650, 4, 10, 4, "lanczos3"), L.make_resample_desc(4, 650, 4, 10, "lanczos3"),
                  L.make_resample_desc(130, 4, 2, 4, "area"), L.make_resample_desc(4, 130, 4, 2, "area")):
            assert call(h, o, d) == TOO_LARGE
            assert b"RT_RESAMPLE_MAX_TAPS" in lib.rt_last_error(ctx)
            still_works()
        # and the context still renders
        sc = scenes.make_scene(1, host.generate_aabb)
        p = sc.params(width=64, height=32)
        t.load(sc)
        t.render(p)
        first = t.readback()[0].copy()
        with host.RayTracer(0) as fresh:
            fresh.load(sc)
            fresh.render(p)
            assert same_bits(first, fresh.readback()[0])
        assert np.nanmax(first[..., :3]) > 0.05
