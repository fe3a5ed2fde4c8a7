"""What the post passes and the strip transport refuse, and in which words: the status code and the exact rt_last_error text
of every refusal branch of rt_taa_resolve, rt_bloom, rt_ssao, rt_ssao_blur, rt_equirect_to_cubemap, rt_frame, rt_deinterleave,
rt_wire_pack and rt_wire_unpack, and the two device-free functions (rt_strip_local_rows, rt_wire_bytes) on the CPU.  Every
refusal comes before the entry point's first HIP call, so nothing here launches a kernel; where a refusal needs device
pointers they are 8 x 8 tensors."""
import ctypes

import numpy as np
import pytest

from opengl_raytracing_amd import layout as L

INVALID, TOO_LARGE = -1, -4
W = H = 8


# ---- the two device-free functions ---------------------------------------------------------------------------------------
def strip_rows(height, strip_rows_, strip_count, strip_index):
    """rt_strip_local_rows restated: the rows of strips strip_index, strip_index + strip_count, ... (the last one may be ragged)."""
    n_strips = -(-height // strip_rows_)
    return sum(min((s + 1) * strip_rows_, height) - s * strip_rows_ for s in range(strip_index, n_strips, strip_count))


def test_strip_local_rows_refusals(host):
    f = host.load_library().entry["rt_strip_local_rows"]
    assert f(16, 4, 2, 0) == 8
    for args in ((-1, 4, 2, 0),        # height < 0
                 (16, 0, 2, 0),        # stripRows <= 0
                 (16, -4, 2, 0),
                 (16, 4, 0, 0),        # stripCount <= 0
                 (16, 4, -2, 0),
                 (16, 4, 2, -1),       # stripIndex < 0
                 (16, 4, 2, 2),        # stripIndex >= stripCount
                 (16, 4, 2, 3)):
        assert f(*args) == INVALID, args


@pytest.mark.parametrize("height,rows,count", [
    (0, 4, 2),          # no rows at all
    (16, 4, 2),         # whole strips, two each
    (18, 4, 2),         # ragged last strip (2 rows), owned by index 0
    (14, 4, 3),         # ragged last strip (2 rows), owned by index 0 again; index 1 and 2 own one strip
    (10, 4, 8),         # stripCount larger than the number of strips: indices 3.. own nothing
    (7, 16, 2),         # one ragged strip shorter than stripRows
    (1080, 8, 8),
])
def test_strip_local_rows_values(host, height, rows, count):
    got = [host.strip_local_rows(height, rows, count, i) for i in range(count)]
    assert got == [strip_rows(height, rows, count, i) for i in range(count)]
    assert sum(got) == height


def test_strip_local_rows_literal(host):
    assert [host.strip_local_rows(18, 4, 2, i) for i in range(2)] == [10, 8]
    assert [host.strip_local_rows(10, 4, 8, i) for i in range(8)] == [4, 4, 2, 0, 0, 0, 0, 0]


def test_wire_bytes(host):
    f = host.load_library().entry["rt_wire_bytes"]
    assert [f(n) for n in (0, 1, 8, 9)] == [0, 32, 240, 272]      # 30 bytes a pixel, rounded up to 16


# ---- refusals with a live context ----------------------------------------------------------------------------------------
class Ctx:
    """A tracer's library and handle, and the way this file calls an entry point: raw, so that the status comes back."""

    def __init__(self, tracer):
        self.lib, self.ctx = tracer.lib, tracer.ctx

    def refused(self, name, args, code, text):
        """`name`(ctx, *args) answers `code` and leaves exactly `text` in rt_last_error.  The text is first set to another
        refusal's, so it is this call that wrote it."""
        assert self.lib.entry["rt_pick"](self.ctx, None, 0, 0, None) == INVALID
        assert self.lib.rt_last_error(self.ctx) == b"NULL hit pointer"
        rc = self.lib.entry[name](self.ctx, *args)
        got = self.lib.rt_last_error(self.ctx).decode()
        assert (rc, got) == (code, text), f"{name}{tuple(args)}"


@pytest.fixture
def ctx(tracer):
    return Ctx(tracer)


@pytest.fixture(scope="module")
def dev():
    """Device addresses of 8 x 8 surfaces: float4 a / b / c / d, half4 n / m, float p / q, and a wire buffer."""
    import torch
    t = {k: torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for k in "abcd"}
    t.update({k: torch.zeros((H, W, 4), dtype=torch.float16, device="cuda") for k in "nm"})
    t.update({k: torch.zeros((H, W), dtype=torch.float32, device="cuda") for k in "pq"})
    t["wire"] = torch.zeros(4 * W * H * 30 + 64, dtype=torch.uint8, device="cuda")
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    ptrs["_keep"] = t
    return ptrs


def variations(valid, bad):
    """`valid` (an ordered name -> value dict) with one argument replaced at a time: bad = {name: (values, ...)}."""
    for name, values in bad.items():
        for v in values:
            yield [v if k == name else x for k, x in valid.items()]


def fptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


@pytest.mark.gpu
def test_null_context(tracer):
    """Every entry point answers RT_ERR_INVALID_ARG to a NULL context before it looks at anything else, and rt_last_error(NULL)
    has a text of its own."""
    e = tracer.lib.entry
    assert tracer.lib.rt_last_error(None) == b"NULL context"
    assert e["rt_taa_resolve"](None, None, None, None, None, 0, 0, 0.0, 0.0, 0.0, None) == INVALID
    assert e["rt_bloom"](None, None, None, 0, 0, 0.0, 0.0, -1, None) == INVALID
    assert e["rt_ssao"](None, None, None, None, 0, 0, None, 0, 0, None, None, None, None) == INVALID
    assert e["rt_ssao_blur"](None, None, None, 0, 0, 0, None) == INVALID
    assert e["rt_equirect_to_cubemap"](None, None, 0, 0, 0, None, 0) == INVALID
    assert e["rt_frame"](None, None, None, None) == INVALID
    assert e["rt_frame_surfaces"](None, None, None, None, None, None) == INVALID
    assert e["rt_deinterleave"](None, None, None, 0, 0, 0, 0, 0, 0, None) == INVALID
    assert e["rt_wire_pack"](None, None, None, None, None, 0, None) == INVALID
    assert e["rt_wire_unpack"](None, None, 0, 0, None, None, None, 0, None, None, None, 0, 0, 0, 0, None) == INVALID


@pytest.mark.gpu
def test_scheduler_hook_refusals(ctx):
    """rt_debug_tile_order and rt_debug_lpt_sort (the hooks of tests/test_sched.py): NULL pointers and tile counts outside
    [1, 2^20].  The read-out's refusals leave no text, as those of the other two scheduler read-outs."""
    e, c = ctx.lib.entry, ctx.ctx
    buf = (ctypes.c_uint32 * 4)()
    n, policy = ctypes.c_int(0), ctypes.c_int(0)
    assert e["rt_debug_tile_order"](None, buf, 4, ctypes.byref(n), ctypes.byref(policy)) == INVALID
    for args in ((None, 4, ctypes.byref(n), ctypes.byref(policy)), (buf, -1, ctypes.byref(n), ctypes.byref(policy)),
                 (buf, 4, None, ctypes.byref(policy)), (buf, 4, ctypes.byref(n), None)):
        assert e["rt_debug_tile_order"](c, *args) == INVALID, args
    assert e["rt_debug_lpt_sort"](None, buf, 4, buf, None) == INVALID
    order = (ctypes.c_uint32 * 4)()
    for args in ((None, 4, order, None), (buf, 4, None, None), (None, 4, None, buf)):
        ctx.refused("rt_debug_lpt_sort", args, INVALID, "rt_debug_lpt_sort: NULL costs or order")
    for bad in (0, -1, (1 << 20) + 1, -(1 << 31)):
        ctx.refused("rt_debug_lpt_sort", (buf, bad, order, None), INVALID, "rt_debug_lpt_sort: nTiles outside [1, 2^20]")
    assert list(buf) == [0, 0, 0, 0] and list(order) == [0, 0, 0, 0]


@pytest.mark.gpu
def test_taa_resolve_refusals(ctx, dev):
    valid = dict(cur=dev["a"], his=dev["b"], nrm=dev["n"], out=dev["c"], w=W, h=H, blend=0.1, jx=0.0, jy=0.0, stream=None)
    bad = dict(cur=(None,), his=(None,), nrm=(None,), out=(None,), w=(0, -1), h=(0, -1))
    for args in variations(valid, bad):
        ctx.refused("rt_taa_resolve", args, INVALID, "bad rt_taa_resolve arguments")
    for args in variations(valid, dict(out=(dev["a"], dev["b"]))):
        ctx.refused("rt_taa_resolve", args, INVALID, "rt_taa_resolve cannot run in place")


@pytest.mark.gpu
def test_bloom_refusals(ctx, dev):
    valid = dict(scene=dev["a"], out=dev["b"], w=W, h=H, threshold=1.0, strength=0.5, iterations=2, stream=None)
    bad = dict(scene=(None,), out=(None,), w=(0, -1), h=(0, -1), iterations=(-1,))
    for args in variations(valid, bad):
        ctx.refused("rt_bloom", args, INVALID, "bad rt_bloom arguments")
    for args in variations(valid, dict(out=(dev["a"],))):
        ctx.refused("rt_bloom", args, INVALID, "rt_bloom cannot run in place")


@pytest.mark.gpu
def test_ssao_refusals(ctx, dev, host):
    samples, noise = host.ssao_kernel()
    samples, noise = np.ascontiguousarray(samples, np.float32), np.ascontiguousarray(noise, np.float32)
    mat = np.eye(4, dtype=np.float32)
    valid = dict(pos=dev["a"], nrm=dev["n"], out=dev["p"], w=W, h=H, noise=fptr(noise), nw=4, nh=4, samples=fptr(samples),
                 proj=fptr(mat), view=fptr(mat), stream=None)
    bad = dict(pos=(None,), nrm=(None,), out=(None,), noise=(None,), samples=(None,), proj=(None,), view=(None,), w=(0, -1), h=(0, -1))
    for args in variations(valid, bad):
        ctx.refused("rt_ssao", args, INVALID, "bad rt_ssao arguments")
    for args in variations(valid, dict(nw=(0, -4, 5, 17), nh=(0, -4, 5))):       # 0 and negative sizes, 4 x 5 and 5 x 4 = 20, 17 x 4
        ctx.refused("rt_ssao", args, TOO_LARGE, "rotation texture larger than 16 texels")
    for args in variations(valid, dict(out=(dev["a"], dev["n"]))):
        ctx.refused("rt_ssao", args, INVALID, "rt_ssao cannot run in place")


@pytest.mark.gpu
def test_ssao_blur_refusals(ctx, dev):
    valid = dict(src=dev["p"], out=dev["q"], w=W, h=H, horizontal=0, stream=None)
    for args in variations(valid, dict(src=(None,), out=(None,), w=(0, -1), h=(0, -1))):
        ctx.refused("rt_ssao_blur", args, INVALID, "bad rt_ssao_blur arguments")
    for horizontal in (0, 1):
        ctx.refused("rt_ssao_blur", [dev["p"], dev["p"], W, H, horizontal, None], INVALID, "rt_ssao_blur cannot run in place")


@pytest.mark.gpu
def test_equirect_to_cubemap_refusals(ctx, dev):
    eq = np.zeros((4, 8, 3), dtype=np.float32)
    valid = dict(eq=fptr(eq), w=8, h=4, size=2, faces=dev["a"], install=0)
    for args in variations(valid, dict(eq=(None,), w=(0, -1), h=(0, -1), size=(0, -1))):
        ctx.refused("rt_equirect_to_cubemap", args, INVALID, "bad rt_equirect_to_cubemap arguments")
    ctx.refused("rt_equirect_to_cubemap", [fptr(eq), 8, 4, 2, None, 0], INVALID, "nowhere to put the faces")


@pytest.mark.gpu
def test_frame_refusals(ctx, dev, host):
    samples, noise = host.ssao_kernel()
    samples, noise = np.ascontiguousarray(samples, np.float32), np.ascontiguousarray(noise, np.float32)

    def desc(ao=0, iterations=2, with_samples=True, with_noise=True):
        d = host.RtFrameDesc()
        d.enableAO, d.enableTAA, d.taaBlendFactor = ao, 1, 0.1
        d.bloomThreshold, d.bloomStrength, d.bloomIterations = 1.0, 0.5, iterations
        if with_samples:
            d.aoSamples = fptr(samples)
        if with_noise:
            d.aoNoise = fptr(noise)
        return d

    p = L.make_params(W, H, 1)
    ctx.refused("rt_frame", [ctypes.byref(p), None, None], INVALID, "frame description is NULL")
    for kw in (dict(with_samples=False), dict(with_noise=False), dict(with_samples=False, with_noise=False)):
        ctx.refused("rt_frame", [ctypes.byref(p), ctypes.byref(desc(ao=1, **kw)), None], INVALID,
                    "AO needs its kernel samples and rotation texture")
    ctx.refused("rt_frame", [ctypes.byref(p), ctypes.byref(desc(iterations=-1)), None], INVALID, "bloomIterations < 0")
    # the description is looked at first, then the parameters as every render looks at them ...
    d = desc()
    ctx.refused("rt_frame", [None, ctypes.byref(d), None], INVALID, "params is NULL")
    ctx.refused("rt_frame", [ctypes.byref(L.copy_params(p, width=0)), ctypes.byref(d), None], INVALID, "width/height must be positive")
    ctx.refused("rt_frame", [ctypes.byref(L.copy_params(p, maxRayDepth=33)), ctypes.byref(d), None], INVALID, "maxRayDepth outside [0, 32]")
    # ... then the whole-image rule: no window, no strips
    for updates in (dict(x0=1), dict(y0=1), dict(regionW=W - 1), dict(regionH=H - 1), dict(regionW=W + 1),
                    dict(stripCycleRows=1), dict(stripCount=2), dict(stripCount=2, stripIndex=1)):
        ctx.refused("rt_frame", [ctypes.byref(L.copy_params(p, **updates)), ctypes.byref(d), None], INVALID,
                    "rt_frame renders the whole image on one device")


@pytest.mark.gpu
def test_deinterleave_refusals(ctx, dev):
    valid = dict(src=dev["a"], dst=dev["b"], w=W, h=H, bpp=16, rows=2, count=2, stride=W * H * 16, stream=None)
    bad = dict(src=(None,), dst=(None,), w=(0, -1), h=(0, -1), bpp=(0, -1), rows=(0, -1), count=(0, -1))
    for args in variations(valid, bad):
        ctx.refused("rt_deinterleave", args, INVALID, "bad deinterleave arguments")
    for updates in (dict(w=1, bpp=6), dict(w=3, bpp=2), dict(stride=W * H * 16 + 2), dict(stride=1)):
        args = list({**valid, **updates}.values())
        ctx.refused("rt_deinterleave", args, INVALID, "row bytes and rank stride must be multiples of 4")


@pytest.mark.gpu
def test_wire_pack_refusals(ctx, dev):
    valid = dict(col=dev["a"], pos=dev["b"], nrm=dev["n"], wire=dev["wire"], n=W * H, stream=None)
    for args in variations(valid, dict(col=(None,), pos=(None,), nrm=(None,), wire=(None,))):
        ctx.refused("rt_wire_pack", args, INVALID, "bad wire_pack arguments")


@pytest.mark.gpu
def test_wire_unpack_refusals(ctx, dev):
    # two ranks, strips of 2 rows, root share 1: a cycle is 4 rows, 2 cycles in 8 rows, so a rank holds 2 * 2 * 8 = 32 pixels
    need = 32
    valid = dict(wire=dev["wire"], stride=need * 30 + 4, pixels=need, rcol=None, rpos=None, rnrm=None, root=1, col=dev["a"],
                 pos=dev["b"], nrm=dev["n"], w=W, h=H, rows=2, count=2, stream=None)
    bad = dict(wire=(None,), col=(None,), pos=(None,), nrm=(None,), w=(0, -1), h=(0, -1), rows=(0, -1), count=(0, -1), root=(0, -1))
    for args in variations(valid, bad):
        ctx.refused("rt_wire_unpack", args, INVALID, "bad wire_unpack arguments")
    local = dict(rcol=dev["c"], rpos=dev["d"], rnrm=dev["m"])
    for missing in ("rcol", "rpos", "rnrm"):                     # two of the three
        args = list({**valid, **local, missing: None}.values())
        ctx.refused("rt_wire_unpack", args, INVALID, "the root's three local surfaces must be given together")
    for given in ("rcol", "rpos", "rnrm"):                       # one of the three
        args = list({**valid, given: local[given]}.values())
        ctx.refused("rt_wire_unpack", args, INVALID, "the root's three local surfaces must be given together")
    for root in (2, 3):
        ctx.refused("rt_wire_unpack", list({**valid, "root": root}.values()), INVALID, "a larger root share needs the root's local surfaces")
    # the size rule: whole strips per rank, a stride of whole words that holds the rank's 30 bytes a pixel
    for updates in (dict(pixels=need - 1),                                   # fewer pixels than the plan's strips
                    dict(stride=need * 30 + 2),                              # not a multiple of 4
                    dict(stride=need * 30 - 4),                              # smaller than the rank's planes
                    dict(pixels=need + 8, stride=need * 30 + 4),             # ... which follow rankPixels, not the need
                    dict(h=H + 1)):                                          # a ragged third cycle needs a third strip
        ctx.refused("rt_wire_unpack", list({**valid, **updates}.values()), INVALID,
                    "rank buffers too small or misaligned for this strip plan")
    # a root share of 2 strips with local surfaces: cycle = (2 + 1) * 2 = 6 rows, 2 cycles -> still 32 pixels a rank
    ctx.refused("rt_wire_unpack", list({**valid, **local, "root": 2, "pixels": need - 1}.values()), INVALID,
                "rank buffers too small or misaligned for this strip plan")
