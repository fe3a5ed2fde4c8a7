"""The definitions of rt_accum_add, rt_accum_view and the accumulation solve (include/rt_mi355.h) restated in numpy float32 / uint32
and Python integers: the oracle of tests/test_accum_host.py and tests/test_accum.py.  Not a test module.  Every floating-point step is
one elementwise numpy float32 operation in the header's order (numpy never fuses a multiply with an add; its float32 divide and sqrt
are correctly rounded, as the device's are), every integer step of the solve a Python int.

An accumulator is a float32 array [2, h, w, 4] with the device's bytes: [0] the running mean, [1] {mY, M2, count as uint32 bits, 0}."""
import numpy as np

from opengl_raytracing_amd import layout as L

F = np.float32
LIMIT = F(2.0 ** 48)
MAX_COUNT = 1 << 24
SHAPES = [(1, 1), (3, 1), (5, 3), (67, 9), (257, 3), (640, 360)]
DESC_DEFAULTS = dict(rel_error=0.02, lum_floor=2.0 ** -10, min_samples=16, done_permille=950)
SPECIALS = np.array([np.nan, np.inf, -np.inf, 2.0 ** 48, -2.0 ** 48, np.nextafter(F(2.0 ** 48), F(np.inf)), -np.nextafter(F(2.0 ** 48), F(np.inf)),
                     -0.0, 0.0, 1e-40, -1e-40, 1.4e-45, -1.0, 3.0e38], dtype=np.float32)
N_REJECTED_SPECIALS = 6            # NaN, +-inf, +-nextafter(2^48), 3e38: the samples that are refused


def empty(w, h):
    return np.zeros((2, h, w, 4), dtype=np.float32)


def counts(acc):
    """The per-pixel sample counts, uint32 [h, w]."""
    return np.ascontiguousarray(acc[1, ..., 2]).view(np.uint32)


def set_counts(acc, mask, value):
    """Write `value` into the count word of the pixels of `mask` (the tests plant counts near 2^24 this way)."""
    c = counts(acc)
    c[mask] = value
    acc[1, ..., 2] = c.view(np.float32)


def luminance(img):
    """Y = (0.2126f*r + 0.7152f*g) + 0.0722f*b: three float32 multiplies, two float32 adds."""
    with np.errstate(all="ignore"):
        r, g, b = (np.asarray(img[..., k], dtype=np.float32) for k in range(3))
        return ((F(0.2126) * r + F(0.7152) * g) + F(0.0722) * b).astype(np.float32)


def add(acc, img):
    """One rt_accum_add's update of the accumulator: -> (the new accumulator, the mask of rejected pixels)."""
    x = np.asarray(img, dtype=np.float32)
    mean, mY, M2, count = acc[0], acc[1, ..., 0], acc[1, ..., 1], counts(acc)
    with np.errstate(all="ignore"):
        ok = (np.abs(x) <= LIMIT).all(axis=-1) & (count < MAX_COUNT)       # (NaN compares false)
        n = count + ok.astype(np.uint32)
        nf = np.where(ok, n, 1).astype(np.float32)
        d = x - mean
        mean1 = mean + d / nf[..., None]
        Y = luminance(x)
        dY = Y - mY
        mY1 = mY + dY / nf
        M21 = M2 + dY * (Y - mY1)
    assert mean1.dtype == mY1.dtype == M21.dtype == np.float32
    out = acc.copy()
    out[0][ok] = mean1[ok]
    mom = np.stack([mY1, M21, n.view(np.float32), np.zeros_like(mY1)], axis=-1)
    out[1][ok] = mom[ok]
    return out, ~ok


def judge(acc, rel_error=0.02, lum_floor=2.0 ** -10, min_samples=16, done_permille=950):
    """The per-pixel rule rt_accum_add's statistics and rt_accum_view share: dict(count, sampled, r2, bits, bin, converged)."""
    mY, M2, count = acc[1, ..., 0], acc[1, ..., 1], counts(acc)
    sampled = count >= 2
    with np.errstate(all="ignore"):
        nf = count.astype(np.float32)
        q = M2 / (nf * (nf - F(1.0)))
        m = np.maximum(mY, F(lum_floor))
        r2 = (q / (m * m)).astype(np.float32)
        thr2 = F(rel_error) * F(rel_error)
        bits = np.ascontiguousarray(r2).view(np.uint32)
        e = (bits >> 21).astype(np.int64) - 396
        bins = np.where(r2 > 0, np.clip(e, 0, 127), 0)
        converged = sampled & (count >= int(min_samples)) & (r2 <= thr2)
    assert r2.dtype == np.float32 and thr2.dtype == np.float32
    return dict(count=count, sampled=sampled, r2=r2, bits=bits, bin=bins, converged=converged)


def percentile_bin(hist, n, permille):
    """The smallest bin whose cumulative count reaches ceil(n * permille / 1000); 0 when n == 0."""
    if n == 0:
        return 0
    rank = -((-n * permille) // 1000)
    c = 0
    for b, k in enumerate(hist):
        c += k
        if c >= rank:
            return b
    raise AssertionError("the rank lies behind the last bin")


def solve(hist, n_converged, n_pixels, done_permille, prev_frames):
    h = [int(x) for x in hist]
    n = sum(h)
    return dict(medianBin=percentile_bin(h, n, 500), p95Bin=percentile_bin(h, n, 950),
                done=int(int(n_converged) * 1000 >= int(n_pixels) * int(done_permille)), frames=min(int(prev_frames) + 1, 2 ** 32 - 1))


def report(acc, rejected, prev_frames, **desc):
    """What rt_accum_add leaves in the state for the accumulator it left: one ACCUM_STATE_DTYPE record."""
    j = judge(acc, **desc)
    s = j["sampled"]
    out = np.zeros(1, dtype=L.ACCUM_STATE_DTYPE)[0]
    out["hist"] = np.bincount(j["bin"][s].reshape(-1), minlength=128).astype(np.uint32)
    out["nPixels"] = s.size
    out["nUnsampled"] = int((~s).sum())
    out["nConverged"] = int(j["converged"].sum())
    out["nRejected"] = int(np.asarray(rejected).sum())
    out["minCount"], out["maxCount"] = int(j["count"].min()), int(j["count"].max())
    out["maxR2Bits"] = int(j["bits"][s].max()) if s.any() else 0
    sol = solve(out["hist"], out["nConverged"], out["nPixels"], desc.get("done_permille", DESC_DEFAULTS["done_permille"]), prev_frames)
    for k, v in sol.items():
        out[k] = v
    return out


def accumulate(acc, img, prev_frames, **desc):
    """rt_accum_add: -> (the new accumulator, the state record)."""
    new, rejected = add(acc, img)
    return new, report(new, rejected, prev_frames, **desc)


def view(acc, mode, **desc):
    """rt_accum_view: float32 [h, w, 4], (v, v, v, 1)."""
    j = judge(acc, **desc)
    if mode == "relerr":
        with np.errstate(all="ignore"):
            v = np.where(j["sampled"], np.sqrt(j["r2"]), F(np.inf)).astype(np.float32)
    elif mode == "count":
        v = j["count"].astype(np.float32)
    else:
        assert mode == "converged"
        v = j["converged"].astype(np.float32)
    out = np.ones(v.shape + (4,), dtype=np.float32)
    out[..., :3] = v[..., None]
    return out


def state_bytes(rec):
    return np.asarray(rec, dtype=L.ACCUM_STATE_DTYPE).reshape(1).view(np.uint8)


def describe_difference(got, want):
    """Field names in which two state records differ bit for bit (for assertion messages)."""
    g, w = np.asarray(got, dtype=L.ACCUM_STATE_DTYPE).reshape(1), np.asarray(want, dtype=L.ACCUM_STATE_DTYPE).reshape(1)
    return [f"{k}: got {g[k][0]!r} want {w[k][0]!r}" for k in L.ACCUM_STATE_DTYPE.names
            if np.ascontiguousarray(g[k]).tobytes() != np.ascontiguousarray(w[k]).tobytes()]


# ---- samples ------------------------------------------------------------------------------------------------------------------------
def base_image(rng, w, h):
    """uniform^4 * 8 in every channel (alpha too): the radiance the frames of a sequence scatter around."""
    return (rng.uniform(0, 1, (h, w, 4)) ** 4 * 8).astype(np.float32)


def noisy_frames(rng, base, n, planted=True):
    """n one-sample frames of `base`: every channel times an independent gamma(2, 1/2) factor (mean 1), so pixels converge at
    different rates.  With `planted`, special values go over the colour channels of frame k -- one for every 8 channels the image
    has, all of them from 104 channels on, which ones and where moving from frame to frame: the per-pixel counts diverge."""
    frames = []
    for k in range(n):
        img = (base * rng.gamma(2.0, 0.5, base.shape)).astype(np.float32)
        flat = img.reshape(-1, 4)
        m = flat.shape[0] * 3
        if planted:
            for s in range(min(len(SPECIALS), m // 8 + 1)):
                pos = (s * 7919 + 3 + 101 * k) % m
                flat[pos // 3, pos % 3] = SPECIALS[(s + k) % len(SPECIALS)]
        frames.append(img)
    return frames
