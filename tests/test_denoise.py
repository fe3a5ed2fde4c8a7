"""The denoiser on the GPU (include/rt_mi355.h): the guide plane, both scratch planes and the output of rt_denoise, bit for bit, against
the numpy restatement of tests/denoise_oracle.py -- for 1 to 5 iterations over shapes from one pixel to several tiles, on guides and
images written by hand (object checkerboards, misses, zero / denormal / huge / antiparallel / orthogonal normals, every normal power,
NaN, infinities, values at and beyond 2^48, signed zeros and denormals, counts on both sides of minCount, luminance gaps on both sides
of exp_'s clamp), without moments, run to run, behind the renderer on a caller's stream feeding rt_meter and rt_display_pack_toned
with no host synchronisation in between; then every refusal.  Every comparison is exact equality; guard bytes around every buffer the
calls write stay untouched."""
import ctypes

import numpy as np
import pytest

import accum_oracle as AO
import denoise_oracle as DO
import meter_oracle as MO
from opengl_raytracing_amd import layout as L
from test_accum import Guarded, same_bits, up

pytestmark = pytest.mark.gpu

INVALID, TOO_LARGE = -1, -4
F = np.float32
SHAPES = [(1, 1), (3, 1), (5, 3), (67, 9), (257, 3), (130, 70)]
MIN_COUNT = 4
COUNTS = np.array([0, 1, MIN_COUNT - 1, MIN_COUNT, 2 ** 24, 9], dtype=np.uint32)


@pytest.fixture(scope="module")
def rt(host):
    t = host.RayTracer(0)
    yield t
    t.close()


class Device:
    """Guarded guide, scratch planes and output of one shape: make_guide() is rt_denoise_guide, denoise() is rt_denoise; both read back."""

    def __init__(self, w, h):
        self.w, self.h = w, h
        self.guide = Guarded(w * h * 16)
        self.scratch = Guarded(w * h * 32)
        self.out = Guarded(w * h * 16)

    def make_guide(self, rt, hits):
        rt.denoise_guide(up(hits.view(np.uint8)), self.w, self.h, out=self.guide.t)
        return self.guide.read().view(L.DENOISE_GUIDE_DTYPE).reshape(self.h, self.w)

    def denoise(self, rt, img, moments, **desc):
        rt.denoise(up(img), up(moments) if moments is not None else None, self.guide.t, self.scratch.t, self.out.t, self.w, self.h, **desc)
        planes = self.scratch.read().view(np.float32).reshape(2, self.h, self.w, 4)
        return planes[0], planes[1], self.out.read().view(np.float32).reshape(self.h, self.w, 4)


def check_plane(got, want, what):
    if not same_bits(got, want):
        bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)).any(axis=-1))
        y, x = bad[0]
        raise AssertionError((what, f"{len(bad)} pixels differ; first ({x}, {y}): got {got[y, x]!r} want {want[y, x]!r}"))


def check_run(rt, dev, hits, img, moments, what="", **desc):
    """Guide, both scratch planes and the output of one run against the oracle -> the oracle's result."""
    want_guide = DO.guide(hits)
    got_guide = dev.make_guide(rt, hits)
    assert same_bits(got_guide, want_guide), (what, "guide")
    want = DO.denoise(img, moments, want_guide, **desc)
    A, B, out = dev.denoise(rt, img, moments, **desc)
    check_plane(A, want["A"], (what, "scratch plane A"))
    check_plane(B, want["B"], (what, "scratch plane B"))       # (one iteration never writes plane B: it stays zero)
    check_plane(out, want["out"], (what, "output"))
    return want


# ---- inputs written by hand ---------------------------------------------------------------------------------------------------------
def objects_blobs(rng, w, h):
    """Blocks of a few objects with a scatter of misses and of single-pixel objects."""
    y, x = np.mgrid[0:h, 0:w]
    obj = ((x // 11) % 3 + 3 * ((y // 5) % 2)).astype(np.int32)
    obj[rng.uniform(size=(h, w)) < 0.06] = -1
    obj[rng.uniform(size=(h, w)) < 0.03] = 40
    return obj


def objects_checker(w, h, period):
    y, x = np.mgrid[0:h, 0:w]
    return (((x // period) + (y // period)) % 2).astype(np.int32)


def raw_normals(rng, obj):
    """Per object one axis a; every pixel takes +a, -a (antiparallel), a vector orthogonal to a, a slightly turned a, or a random
    direction, at a random length -- and a few are zero, denormal (the squared length underflows to 0) or huge (it overflows).  Misses
    have the normal 0."""
    h, w = obj.shape
    axis = rng.normal(size=(64, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    a = axis[obj % 64]
    rnd = rng.normal(size=(h, w, 3))
    rnd /= np.linalg.norm(rnd, axis=-1, keepdims=True)
    ortho = np.cross(a, rnd)
    ortho /= np.linalg.norm(ortho, axis=-1, keepdims=True)
    kind = rng.integers(0, 10, (h, w))[..., None]
    n = np.where(kind < 4, a + 0.05 * rnd, np.where(kind == 4, -a, np.where(kind == 5, ortho, np.where(kind == 6, rnd, a))))
    n = n * rng.uniform(0.5, 3.0, (h, w, 1))
    special = rng.integers(0, 40, (h, w))[..., None]
    n = np.where(special == 0, 0.0, np.where(special == 1, 1e-40 * np.sign(n), np.where(special == 2, 1e30 * np.sign(n), n)))
    n[obj < 0] = 0.0
    return n.astype(np.float32)


def image_with_specials(rng, w, h, planted=True):
    """Positive radiance over four decades, alpha too; with `planted`, accum_oracle's special values over the colour channels."""
    base = (rng.uniform(0, 1, (h, w, 4)) ** 4 * 8).astype(np.float32)
    return AO.noisy_frames(rng, base, 1, planted=planted)[0]


def moments_by_hand(rng, img, counts=COUNTS):
    """Plane 1 of an accumulator: mY the image's luminance where that is finite, M2 positive (zero in a fifth of the pixels), the
    count one of `counts`."""
    h, w = img.shape[:2]
    mom = np.zeros((h, w, 4), dtype=np.float32)
    mom[..., 0] = np.nan_to_num(DO.luminance(img), nan=0.0, posinf=0.0, neginf=0.0)
    M2 = (rng.uniform(0, 1, (h, w)) ** 3 * 200).astype(np.float32)
    M2[rng.uniform(size=(h, w)) < 0.2] = 0.0
    mom[..., 1] = M2
    mom[..., 2] = rng.choice(counts, (h, w)).astype(np.uint32).view(np.float32)
    return mom


def inputs(w, h, seed=0, objects=None):
    rng = np.random.default_rng(1000 * w + 7 * h + seed)
    obj = objects_blobs(rng, w, h) if objects is None else objects
    hits = DO.make_hits(raw_normals(rng, obj), obj, rng)
    img = image_with_specials(rng, w, h)
    return hits, img, moments_by_hand(rng, img)


# ---- 1. parity over shapes and iteration counts -------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_matches_numpy(rt, w, h, iterations):
    hits, img, mom = inputs(w, h)
    desc = dict(iterations=iterations, normal_log2_power=iterations - 1, sigma_lum=2.0, lum_eps=2.0 ** -6, min_count=MIN_COUNT)
    want = check_run(rt, Device(w, h), hits, img, mom, **desc)
    if w * h >= 600:                                           # the case is the case it claims to be
        g = DO.guide(hits)
        skipped = np.signbit(want["planes"][0][..., 3])
        assert 0 < skipped.sum() < 30 and (g["object"] == -1).any() and not g["n"][g["object"] == -1].any()
        zero = (g["object"] >= 0) & ~g["n"].any(axis=-1)
        assert zero.sum() >= 3, "zero, denormal and huge raw normals all give the guide normal 0"
        c = DO.counts(mom)
        assert all((c == k).any() for k in COUNTS) and (mom[..., 1] == 0).any()
        assert not same_bits(want["out"][..., :3], img[..., :3]) and np.isfinite(want["out"][~skipped]).all()
        assert np.isfinite(want["out"][skipped][:, :3]).any(), "no skipped pixel was filled"


@pytest.mark.parametrize("w,h", [(5, 3), (67, 9), (130, 70)])
def test_without_moments(rt, w, h):
    """dMoments = NULL: one raw frame, every variance is the spatial estimate."""
    hits, img, _ = inputs(w, h, seed=1)
    want = check_run(rt, Device(w, h), hits, img, None, iterations=3, min_count=2)
    var = want["planes"][0][..., 3]
    assert same_bits(var[~np.signbit(var)], DO.spatial_variance(img, DO.guide(hits), np.ones((h, w), np.uint32))[0][~np.signbit(var)])


@pytest.mark.parametrize("power", range(8))
def test_every_normal_power(rt, power):
    w, h = 67, 9
    hits, img, mom = inputs(w, h, seed=2)
    check_run(rt, Device(w, h), hits, img, mom, iterations=2, normal_log2_power=power, min_count=MIN_COUNT)


@pytest.mark.parametrize("period", [1, 2, 4, 8, 16])
def test_object_checkerboards(rt, period):
    """Two objects in cells of `period` texels, five iterations: at the step that equals the period every tap at an odd multiple lands
    in the other object, at period 1 the direct neighbours do."""
    w, h = 130, 70
    hits, img, mom = inputs(w, h, seed=3, objects=objects_checker(w, h, period))
    want = check_run(rt, Device(w, h), hits, img, mom, iterations=5, min_count=MIN_COUNT)
    assert np.isfinite(want["out"][~np.signbit(want["planes"][0][..., 3])]).all()


def test_luminance_gaps_around_the_clamp_of_exp(rt):
    """One object, one normal, moments with M2 = 0 at count 8: the variance plane is zero and sl = lumEps = 2^-10 exactly.  A grey ramp
    of 0.0215 per texel with a jitter of 1e-3 puts the luminance gap of taps four texels apart at about 88.03 * 2^-10, where
    -wl * log2(e) crosses exp_'s lower clamp -126.99999: gaps on both sides of it, and exact zeros, are in the image."""
    w, h = 67, 9
    rng = np.random.default_rng(17)
    obj = np.zeros((h, w), dtype=np.int32)
    n = np.zeros((h, w, 3), dtype=np.float32)
    n[..., 2] = 2.0
    hits = DO.make_hits(n, obj)
    grey = (np.arange(w)[None, :] * 0.0215 + rng.uniform(-1e-3, 1e-3, (h, w))).astype(np.float32)
    grey[4] = grey[4, 0]                                       # a constant row: gaps of exactly 0
    img = np.ones((h, w, 4), dtype=np.float32)
    img[..., :3] = grey[..., None]
    mom = np.zeros((h, w, 4), dtype=np.float32)
    mom[..., 0] = DO.luminance(img)
    mom[..., 2] = np.full((h, w), 8, dtype=np.uint32).view(np.float32)
    Y = DO.luminance(img)
    x2 = np.abs(Y[:, 4:] - Y[:, :-4]) / F(2.0 ** -10) * F(1.44269504088896340736)
    assert (x2 > 127.2).any() and (x2 < 126.8).any() and (np.abs(x2 - 126.99999) < 0.05).any() and (x2 == 0).any()
    want = check_run(rt, Device(w, h), hits, img, mom, iterations=3, lum_eps=2.0 ** -10)
    assert not want["planes"][0][..., 3].any() and not same_bits(want["out"], img)


def test_same_run_same_bytes(rt):
    w, h = 130, 70
    hits, img, mom = inputs(w, h, seed=4)
    d_hits, d_img, d_mom = up(hits.view(np.uint8)), up(img), up(mom)
    runs = []
    for _ in range(3):
        dev = Device(w, h)
        rt.denoise_guide(d_hits, w, h, out=dev.guide.t)
        rt.denoise(d_img, d_mom, dev.guide.t, dev.scratch.t, dev.out.t, w, h, iterations=5)
        runs.append((dev.guide.read().tobytes(), dev.scratch.read().tobytes(), dev.out.read().tobytes()))
    assert all(r == runs[0] for r in runs[1:])


# ---- 2. behind the renderer, on a caller's stream -----------------------------------------------------------------------------------
def test_render_accumulate_denoise_meter_pack_on_a_side_stream(rt, host):
    """The noise-textured scene at 96 x 54: eight frames rendered into caller-owned surfaces and accumulated, the first-hit guide from
    camera_rays -> trace_rays -> denoise_guide, denoise on the accumulator's two planes, meter on the denoised image, display_pack with
    the meter's exposure -- all on one side stream, the host running ahead; the only wait is the one before the read-back.  Every
    result equals the chain of oracles fed with the rendered frames."""
    import torch
    from opengl_raytracing_amd import scenes
    sc = scenes.make_scene(3, host.generate_aabb)
    w, h, n = 96, 54, 8
    rt.load(sc)
    adesc = dict(rel_error=0.15, lum_floor=2.0 ** -6, min_samples=3, done_permille=400)
    mdesc = dict(key=0.3, low_permille=5, high_permille=5)
    table, tables = host.display_srgb_thresholds(), host.meter_tables()
    dev = Device(w, h)
    accum, state = Guarded(w * h * 32), Guarded(1024)
    d_meter, d_packed = Guarded(1088), Guarded(w * h * 4)
    colours = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(n)]
    d_pos = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    d_nrm = torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for k in range(n):
            sc.frame_count = k
            rt.render_to(sc.params(width=w, height=h), colours[k].data_ptr(), d_pos.data_ptr(), d_nrm.data_ptr(), stream=s.cuda_stream)
            rt.accum_add(colours[k], accum.t, state.t, w, h, stream=s, **adesc)
        sc.frame_count = 0
        p = sc.params(width=w, height=h)
        d_hits = rt.trace_rays(rt.camera_rays(p, stream=s), "closest", stream=s)
        rt.denoise_guide(d_hits, w, h, out=dev.guide.t, stream=s)
        rt.denoise(rt.accum_mean(accum.t, w, h), rt.accum_moments(accum.t, w, h), dev.guide.t, dev.scratch.t, dev.out.t, w, h, stream=s)
        rt.meter(dev.out.t, d_meter.t, w, h, stream=s, **mdesc)
        rt.display_pack(dev.out.t, d_packed.t, w, h, format="srgb", flip=True, exposure=0.75, stream=s, tone="aces",
                        d_exposure=d_meter.t.data_ptr() + L.METER_EXPOSURE_OFFSET)
    s.synchronize()
    acc = AO.empty(w, h)
    for k in range(n):
        acc, _ = AO.accumulate(acc, colours[k].cpu().numpy(), k, **adesc)
    assert same_bits(accum.read().view(np.float32).reshape(2, h, w, 4), acc)
    hits = d_hits.cpu().numpy().reshape(h, w, 8).view(L.HIT_DTYPE).reshape(h, w)
    gd = DO.guide(hits)
    assert same_bits(dev.guide.read().view(L.DENOISE_GUIDE_DTYPE).reshape(h, w), gd)
    assert len(np.unique(gd["object"])) >= 2 and np.abs(np.linalg.norm(gd["n"][gd["object"] >= 0].astype(np.float64), axis=-1) - 1).max() < 1e-6
    want = DO.denoise(acc[0], acc[1], gd)
    planes = dev.scratch.read().view(np.float32).reshape(2, h, w, 4)
    check_plane(planes[0], want["A"], "scratch plane A")
    check_plane(planes[1], want["B"], "scratch plane B")
    out = dev.out.read().view(np.float32).reshape(h, w, 4)
    check_plane(out, want["out"], "output")
    assert np.isfinite(out).all() and (AO.counts(acc) == n).all()
    # the filter did its work: neighbouring pixels of one object differ less than they did in the mean
    same = gd["object"][:, 1:] == gd["object"][:, :-1]

    def roughness(img):
        return float(np.abs(img[:, 1:, :3] - img[:, :-1, :3])[same].mean())
    assert roughness(out) < roughness(acc[0])
    want_meter = MO.meter(want["out"], np.zeros(1, dtype=L.METER_STATE_DTYPE)[0], tables, **mdesc)
    got_meter = d_meter.read().view(L.METER_STATE_DTYPE)[0]
    assert same_bits(MO.state_bytes(got_meter), MO.state_bytes(want_meter)), MO.describe_difference(got_meter, want_meter)
    got = d_packed.read().reshape(h, w, 4)
    assert (got == MO.pack_toned(want["out"], "srgb", True, 0.75, table, "aces", dev_exposure=want_meter["exposure"])).all()
    assert len(np.unique(got[..., :3])) > 32


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(rt):
    import torch
    w, h = 8, 4
    hits, img, mom = inputs(w, h, seed=5)
    dev = Device(w, h)
    d_hits, d_img, d_mom = up(hits.view(np.uint8)), up(img), up(mom)
    lib, ctx, vp = rt.lib, rt.ctx, ctypes.c_void_p
    gd = DO.guide(hits)
    want = DO.denoise(img, mom, gd)
    want_raw = DO.denoise(img, None, gd)

    def desc(**kw):
        d = L.make_denoise_desc(w, h)
        for k, v in kw.items():
            if k == "reserved":
                d.reserved[v] = 1
            else:
                setattr(d, k, v)
        return d

    def ref(d):
        return ctypes.byref(d) if d is not None else None

    def denoise(image, moments, guide, scratch, out, d, c=ctx):
        return lib.rt_denoise(c, vp(image), vp(moments), vp(guide), vp(scratch), vp(out), ref(d), None)

    def make_guide(hits_, guide, gw, gh, c=ctx):
        return lib.rt_denoise_guide(c, vp(hits_), vp(guide), gw, gh, None)

    i, m, g, s, o, hp = d_img.data_ptr(), d_mom.data_ptr(), dev.guide.t.data_ptr(), dev.scratch.t.data_ptr(), dev.out.t.data_ptr(), d_hits.data_ptr()
    plane = w * h * 16

    def still_works():
        assert make_guide(hp, g, w, h) == 0
        assert denoise(i, m, g, s, o, desc()) == 0
        rt.sync()
        assert same_bits(dev.guide.read().view(L.DENOISE_GUIDE_DTYPE).reshape(h, w), gd)
        check_plane(dev.out.read().view(np.float32).reshape(h, w, 4), want["out"], "output")
        assert denoise(i, None, g, s, o, desc()) == 0
        rt.sync()
        check_plane(dev.out.read().view(np.float32).reshape(h, w, 4), want_raw["out"], "output without moments")

    nan, inf = float("nan"), float("inf")
    bad = [desc(width=0), desc(width=-2), desc(height=0), desc(height=-1), desc(iterations=0), desc(iterations=6), desc(iterations=-1),
           desc(normalLog2Power=-1), desc(normalLog2Power=8), desc(sigmaLum=0.0), desc(sigmaLum=-1.0), desc(sigmaLum=nan), desc(sigmaLum=inf),
           desc(lumEps=0.0), desc(lumEps=2.0 ** -41), desc(lumEps=-1.0), desc(lumEps=nan), desc(lumEps=inf), desc(minCount=1), desc(minCount=0),
           desc(minCount=-3), desc(reserved=0), desc(reserved=1), desc(reserved=2), desc(reserved=3), desc(reserved=4), None]
    for k, d in enumerate(bad):
        assert denoise(i, m, g, s, o, d) == INVALID, k
    still_works()
    for d in (desc(iterations=1), desc(iterations=5), desc(normalLog2Power=0), desc(normalLog2Power=7), desc(lumEps=2.0 ** -40),
              desc(minCount=2), desc(sigmaLum=1e-30)):
        assert denoise(i, m, g, s, o, d) == 0                   # the edges of the allowed ranges
    rt.sync()
    for args in [(None, m, g, s, o), (i, m, None, s, o), (i, m, g, None, o), (i, m, g, s, None),                  # NULL
                 (i + 4, m, g, s, o), (i, m + 8, g, s, o), (i, m, g + 4, s, o), (i, m, g, s + 8, o), (i, m, g, s, o + 4),      # misaligned
                 (i, m, g, s, i), (i, m, g, s, m), (i, m, g, s, g), (i, m, g, s, g + plane - 16),                     # out on an input
                 (i, m, g, i, o), (i, m, g, m - plane, o), (i, m, g, g - 2 * plane + 16, o),                          # scratch on an input
                 (i, m, g, s, s), (i, m, g, s, s + plane), (i, m, g, s, s + 2 * plane - 16), (i, m, g, o - plane, o)]:   # out on scratch
        assert denoise(*args, desc()) == INVALID, args
    assert denoise(i, None, g, s, m, desc()) == 0               # without moments that plane is no input: it may take the output
    rt.sync()
    d_mom.copy_(torch.from_numpy(mom))
    torch.cuda.synchronize()
    still_works()
    for args in [(None, g, w, h), (hp, None, w, h), (hp + 8, g, w, h), (hp, g + 4, w, h), (hp, g, 0, h), (hp, g, w, -1), (hp, hp, w, h),
                 (hp, hp + 2 * plane - 16, w, h), (g, g, w, h)]:
        assert make_guide(*args) == INVALID, args
    still_works()
    assert denoise(i, m, g, s, o, desc(), c=None) == INVALID and make_guide(hp, g, w, h, c=None) == INVALID
    huge = desc(width=65536, height=32768)                      # 2^31 pixels
    assert denoise(i, m, g, s, o, huge) == TOO_LARGE and make_guide(hp, g, 65536, 32768) == TOO_LARGE
    still_works()
    torch.cuda.synchronize()
