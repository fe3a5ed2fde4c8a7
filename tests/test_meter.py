"""rt_meter on the GPU (include/rt_mi355.h): the whole rt_meter_state, bit for bit, against the numpy / Python-int restatement of
tests/meter_oracle.py -- histogram, counters, extremes, trimmed mean, target, exposure, frames -- over ragged shapes with every special
value planted, on coherent content (where every lane of a wave hits one bin), at every one of the 257 bin edges, run to run, through
an adaptation sequence, and on a caller's stream feeding rt_present_submit_toned with no host synchronisation in between; then every
refusal.  Every comparison is exact equality."""
import ctypes

import numpy as np
import pytest

import meter_oracle as MO
from opengl_raytracing_amd import layout as L

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0xA5
INVALID, TOO_LARGE = -1, -4
ZERO = np.zeros(1, dtype=L.METER_STATE_DTYPE)[0]


@pytest.fixture(scope="module")
def rt(host):
    t = host.RayTracer(0)
    yield t
    t.close()


@pytest.fixture(scope="module")
def tables(host):
    return host.meter_tables()


def up(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def new_state():
    """A zeroed device state followed by GUARD sentinel bytes."""
    import torch
    s = torch.full((1088 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    s[:1088] = 0
    torch.cuda.synchronize()
    return s


def read_state(d_state):
    import torch
    torch.cuda.synchronize()
    raw = d_state.cpu().numpy()
    assert (raw[1088:] == SENTINEL).all(), "bytes behind the state were written"
    return raw[:1088].copy().view(L.METER_STATE_DTYPE)[0]


def check(got, want, what=""):
    assert MO.state_bytes(got).tobytes() == MO.state_bytes(want).tobytes(), (what, MO.describe_difference(got, want))
    assert int(got["hist"].sum()) + int(got["nNaN"]) + int(got["nInf"]) + int(got["nNonPositive"]) == int(got["nPixels"])


def meter_once(rt, img, **desc):
    h, w = img.shape[:2]
    d_state = new_state()
    rt.meter(up(img), d_state, w, h, **desc)
    return read_state(d_state)


def nan_planted(rng, w, h):
    """hdr_image plus pixels whose channels are finite or infinite but whose Y is NaN (inf - inf), as far as the image has room."""
    img = MO.hdr_image(rng, w, h)
    flat = img.reshape(-1, 4)
    if flat.shape[0] >= 8:
        flat[flat.shape[0] // 2, :3] = (np.inf, -np.inf, 1.0)
        flat[flat.shape[0] // 3, :3] = (0.5, np.inf, -np.inf)
    return img


# ---- 1. parity over shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", MO.SHAPES, ids=[f"{w}x{h}" for w, h in MO.SHAPES])
def test_state_matches_numpy(rt, tables, w, h):
    rng = np.random.default_rng(2000 * w + h)
    img = nan_planted(rng, w, h)
    if w * h >= 8:
        assert np.isnan(MO.luminance(img)).sum() >= 2
    for desc in (dict(), dict(key=0.5, low_permille=100, high_permille=50, min_exposure=0.25, max_exposure=4.0)):
        check(meter_once(rt, img, **desc), MO.meter(img, ZERO, tables, **desc), desc)


# ---- 2. coherent content -----------------------------------------------------------------------------------------------------------
def _coherent(kind):
    w, h = 640, 360
    img = np.empty((h, w, 4), dtype=np.float32)
    img[...] = (0.8, 0.4, 0.2, 1.0)
    if kind == "checker":                                      # 8x8 blocks of two colours, three octaves apart
        yy, xx = np.mgrid[0:h, 0:w]
        img[((yy // 8 + xx // 8) & 1) == 1] = (6.0, 3.0, 2.0, 1.0)
    elif kind == "one_pixel":
        img[h // 2, w // 3] = (300.0, 200.0, 100.0, 1.0)
    elif kind == "non_positive":
        img[...] = (-1.0, 0.0, -0.0, 1.0)
        img[::2] = (0.0, 0.0, 0.0, 1.0)
    return img


@pytest.mark.parametrize("kind", ["constant", "checker", "one_pixel", "non_positive"])
def test_coherent_content(rt, tables, kind):
    img = _coherent(kind)
    got = meter_once(rt, img)
    check(got, MO.meter(img, ZERO, tables), kind)
    nonzero = int((got["hist"] != 0).sum())
    assert nonzero == dict(constant=1, checker=2, one_pixel=2, non_positive=0)[kind]
    if kind == "constant":
        assert got["hist"].max() == 230400 and got["minLum"] == got["maxLum"]
    if kind == "non_positive":
        assert got["nNonPositive"] == 230400 and got["nMetered"] == 0 and got["exposure"] == 1.0
        assert np.isposinf(got["minLum"]) and got["maxLum"] == 0.0


@pytest.mark.parametrize("w", [64, 63])
@pytest.mark.parametrize("k", [1, 2, 3, 64])
def test_distinct_bins_in_one_ballot(rt, tables, k, w):
    """One wave, 64 quads: slot j of lane t is pixel 4t + j, so the 64 lanes' slot-j pixels meet in one ballot of the histogram add
    (csrc/rt_wave.h).  Every slot holds k distinct bins among its lanes: one round suffices (1), exactly the two rounds there are
    (2), one bin left to the lanes that add for themselves (3), every lane alone (64).  Width 63: the last lane has no pixel."""
    lanes = w                                                   # 4 rows of w pixels are w quads
    t, j = np.divmod(np.arange(4 * lanes), 4)
    want_bin = 40 + 3 * ((7 * t + j) % k) + j
    grey = (((888 + want_bin).astype(np.uint32) << 20) | (1 << 19)).view(np.float32)          # the middle of the bin
    img = np.ones((4, w, 4), dtype=np.float32)
    img.reshape(-1, 4)[:, :3] = grey[:, None]
    bins = MO.bins_of(MO.luminance(img)).reshape(-1)
    assert (bins == want_bin).all()
    for slot in range(4):
        assert len(set(bins[slot::4].tolist())) == min(k, lanes)
    got = meter_once(rt, img)
    check(got, MO.meter(img, ZERO, tables), (k, w))
    assert got["nMetered"] == 4 * lanes and int((got["hist"] != 0).sum()) == len(set(want_bin.tolist()))


# ---- 3. bin edges ------------------------------------------------------------------------------------------------------------------
def test_bin_edges(rt, tables):
    """Edge k (k = 0..256) is the float32 with bits (888 + k) << 20: the lower end of bin k (k = 256: the first value clamped into bin
    255 from above).  Pixels (0, g, 0) with g near E / 0.7152 put Y = 0.7152f * g within a few ulps of it on both sides."""
    edges = ((888 + np.arange(257, dtype=np.uint32)) << 20).view(np.float32)
    g0 = (edges.astype(np.float64) / np.float64(np.float32(0.7152))).astype(np.float32)
    g = np.stack([(g0.view(np.int32) + k).view(np.float32) for k in (-2, -1, 0, 1, 2)], axis=1)        # [257, 5]
    Y = MO.luminance(np.stack([np.zeros_like(g), g, np.zeros_like(g), np.ones_like(g)], axis=-1))
    assert ((Y < edges[:, None]).any(axis=1) & (Y >= edges[:, None]).any(axis=1)).all(), "the inputs do not straddle every edge"
    n = g.size
    for w in (n, 5):
        img = np.zeros((n // w, w, 4), dtype=np.float32)
        img[..., 1] = g.reshape(n // w, w)
        got = meter_once(rt, img)
        check(got, MO.meter(img, ZERO, tables), f"width {w}")
        assert got["nMetered"] == n


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------------
def test_same_image_same_bytes(rt):
    img = nan_planted(np.random.default_rng(44), 640, 360)
    d_img = up(img)
    runs = []
    for _ in range(5):
        d_state = new_state()
        rt.meter(d_img, d_state, 640, 360, low_permille=20, high_permille=20)
        runs.append(read_state(d_state).tobytes())
    assert all(r == runs[0] for r in runs[1:])


# ---- 5. adaptation -----------------------------------------------------------------------------------------------------------------
def test_adaptation_sequence(rt, host, tables):
    rng = np.random.default_rng(55)
    w, h = 67, 9
    desc = dict(adapt=0.25, low_permille=10, high_permille=10, min_exposure=2.0 ** -6, max_exposure=2.0 ** 6)
    d_state = new_state()
    prev = ZERO
    exposures = []
    for k, gain in enumerate((1.0, 40.0, 0.01, 3.0)):
        img = (MO.hdr_image(rng, w, h) * np.float32(gain)).astype(np.float32)
        rt.meter(up(img), d_state, w, h, **desc)
        got = read_state(d_state)
        check(got, MO.meter(img, prev, tables, **desc), f"frame {k}")
        seeded = prev.copy()                                    # the recurrence: the device's histogram, the previous exposure and frames
        seeded["hist"] = got["hist"]
        for f in ("nPixels", "nNonPositive", "nNaN", "nInf", "minLum", "maxLum"):
            seeded[f] = got[f]
        check(got, host.meter_solve_host(seeded, w, h, **desc), f"frame {k} vs rt_meter_solve_host")
        assert got["frames"] == k + 1
        assert (got["exposure"] == got["target"]) == (k == 0)      # the first frame jumps, the later ones blend
        exposures.append(float(got["exposure"]))
        prev = got
    assert len(set(exposures)) == 4


# ---- 6. streams --------------------------------------------------------------------------------------------------------------------
def test_meter_feeds_the_toned_submit_on_a_side_stream(host, tables):
    """Upload, meter and present_submit(d_exposure = the state's exposure) on one side stream, the host running ahead: the only wait
    is present_wait.  The bytes equal the oracle's pack with the oracle's own exposure."""
    import torch
    w, h = 900, 400
    img = MO.hdr_image(np.random.default_rng(66), w, h)
    desc = dict(key=0.3, low_permille=5, high_permille=5)
    table = host.display_srgb_thresholds()
    ring = host.RayTracer(0)
    try:
        pinned = torch.from_numpy(img).pin_memory()
        d = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        d_state = new_state()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            d.copy_(pinned, non_blocking=True)
            ring.meter(d, d_state, w, h, stream=s, **desc)
            t = ring.present_submit(d, w, h, format="srgb", flip=True, exposure=0.75, stream=s, tone="aces",
                                    d_exposure=d_state.data_ptr() + L.METER_EXPOSURE_OFFSET)
        got = ring.present_wait(t)
        want_state = MO.meter(img, ZERO, tables, **desc)
        assert (got == MO.pack_toned(img, "srgb", True, 0.75, table, "aces", dev_exposure=want_state["exposure"])).all()
        check(read_state(d_state), want_state)
        assert len(np.unique(got[..., :3])) > 64
    finally:
        ring.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(rt, tables):
    import torch
    w, h = 8, 4
    img = MO.hdr_image(np.random.default_rng(77), w, h)
    d_img = up(img)
    d_state = new_state()
    lib, ctx, vp = rt.lib, rt.ctx, ctypes.c_void_p
    want = MO.meter(img, ZERO, tables)

    def desc(**kw):
        d = L.make_meter_desc(w, h)
        for k, v in kw.items():
            if k == "reserved":
                d.reserved[v] = 1
            else:
                setattr(d, k, v)
        return d

    def meter(image, d, state, c=ctx):
        return lib.rt_meter(c, vp(image), ctypes.byref(d) if d is not None else None, vp(state), None)

    def still_works():
        d_state[:1088] = 0
        torch.cuda.synchronize()
        assert meter(d_img.data_ptr(), desc(), d_state.data_ptr()) == 0
        rt.sync()
        check(read_state(d_state), want)

    i, s = d_img.data_ptr(), d_state.data_ptr()
    nan, inf = float("nan"), float("inf")
    bad = [desc(width=0), desc(width=-2), desc(height=0), desc(height=-1), desc(key=0.0), desc(key=-1.0), desc(key=nan), desc(key=inf),
           desc(minExposure=0.0), desc(minExposure=nan), desc(maxExposure=inf), desc(maxExposure=nan), desc(minExposure=2.0, maxExposure=1.0),
           desc(adapt=0.0), desc(adapt=1.5), desc(adapt=nan), desc(lowPermille=-1), desc(highPermille=-1), desc(lowPermille=600, highPermille=400),
           desc(reserved=0), desc(reserved=1), desc(reserved=2), desc(reserved=3), None]
    for k, d in enumerate(bad):
        assert meter(i, d, s) == INVALID, k
        still_works()
    for image, state in [(None, s), (i, None), (i + 4, s), (i + 8, s), (i, s + 4), (i, s + 8)]:
        assert meter(image, desc(), state) == INVALID, (image, state)
        still_works()
    assert meter(i, desc(), s, c=None) == INVALID
    assert meter(i, desc(width=65536, height=32768), s) == TOO_LARGE         # 2^31 pixels
    still_works()
