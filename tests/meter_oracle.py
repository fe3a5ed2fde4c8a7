"""The definitions of rt_meter and rt_display_pack_toned (include/rt_mi355.h) restated in numpy float32 and Python integers: the
oracle of tests/test_meter_host.py, tests/test_meter.py and tests/test_tone.py.  Not a test module.  Every floating-point step is one
numpy float32 operation (numpy never fuses a multiply with an add), every integer step a Python int.  The solve's two tables and the
sRGB thresholds are the library's own; test_meter_host.py and test_present_host.py pin them to their formulas."""
import numpy as np

from opengl_raytracing_amd import layout as L

F = np.float32
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, -1e-40, 1.0, 0.0, 1.4e-45, -1.0, np.float32(1.0) - np.float32(2.0 ** -24)],
                    dtype=np.float32)
SHAPES = [(1, 1), (3, 2), (5, 7), (64, 4), (67, 9), (257, 3), (640, 360)]
DESC_DEFAULTS = dict(key=0.18, min_exposure=2.0 ** -10, max_exposure=2.0 ** 10, adapt=1.0, low_permille=0, high_permille=0)


def hdr_image(rng, w, h):
    """uniform^4 * 8 in every channel (alpha too), the special values planted over the colour channels as far as they fit."""
    img = (rng.uniform(0, 1, (h, w, 4)) ** 4 * 8).astype(np.float32)
    flat = img.reshape(-1, 4)
    n = flat.shape[0] * 3
    for k, v in enumerate(SPECIALS[: n]):
        pos = (k * 7919 + 3) % n if n > len(SPECIALS) else k
        flat[pos // 3, pos % 3] = v
    return img


def luminance(img):
    """Y = (0.2126f*r + 0.7152f*g) + 0.0722f*b: three float32 multiplies, two float32 adds."""
    with np.errstate(all="ignore"):
        r, g, b = (img[..., k].astype(np.float32) for k in range(3))
        return ((F(0.2126) * r + F(0.7152) * g) + F(0.0722) * b).astype(np.float32)


def bins_of(Y):
    """bin = clamp((bits(Y) >> 20) - 888, 0, 255) of positive finite float32 Y."""
    e = (np.ascontiguousarray(Y, dtype=np.float32).view(np.uint32) >> 20).astype(np.int64) - 888
    return np.clip(e, 0, 255)


def histogram(img):
    """-> dict(hist, nPixels, nNonPositive, nNaN, nInf, minLum, maxLum) of an [h, w, 4] float32 image."""
    Y = luminance(img).reshape(-1)
    nan = np.isnan(Y)
    inf = Y == np.inf
    with np.errstate(invalid="ignore"):
        nonpos = ~nan & ~(Y > 0)
    met = ~nan & ~inf & ~nonpos
    Ym = Y[met]
    return dict(hist=np.bincount(bins_of(Ym), minlength=256).astype(np.uint32), nPixels=Y.size, nNonPositive=int(nonpos.sum()),
                nNaN=int(nan.sum()), nInf=int(inf.sum()), minLum=F(Ym.min()) if Ym.size else F(np.inf), maxLum=F(Ym.max()) if Ym.size else F(0))


def solve(hist, prev_exposure, prev_frames, tables, key=0.18, min_exposure=2.0 ** -10, max_exposure=2.0 ** 10, adapt=1.0,
          low_permille=0, high_permille=0):
    """The solve, literally: -> dict(nMetered, meanLog2Q16, target, exposure, frames, raw) (raw: the target before the clamp, None
    when nothing is metered)."""
    pow2neg, log2q16 = tables
    key, lo_e, hi_e, adapt, old = F(key), F(min_exposure), F(max_exposure), F(adapt), F(prev_exposure)
    h = [int(x) for x in hist]
    n = sum(h)
    lo, hi = n * int(low_permille) // 1000, n * int(high_permille) // 1000
    rem = lo
    for b in range(256):                                   # lo counts removed walking upward
        t = min(h[b], rem)
        h[b] -= t
        rem -= t
    rem = hi
    for b in range(255, -1, -1):                           # then hi counts walking downward
        t = min(h[b], rem)
        h[b] -= t
        rem -= t
    n2 = n - lo - hi
    assert sum(h) == n2 and (n2 >= 1 or n == 0)
    old_ok = int(prev_frames) != 0 and bool(np.isfinite(old)) and bool(old > 0)
    raw = None
    if n2:
        S = sum(h[b] * ((b >> 3) * 65536 + int(log2q16[b & 7])) for b in range(256))
        m = S // n2
        with np.errstate(over="ignore", under="ignore"):
            raw = key * F(np.ldexp(F(pow2neg[(m >> 8) & 255]), 16 - (m >> 16)))      # ldexp is exact: one float32 multiply
        target = lo_e if raw < lo_e else (hi_e if raw > hi_e else raw)
    else:
        m = 0
        target = old if old_ok else F(1.0)
    if not old_ok or adapt >= F(1.0):
        exposure = target
    else:
        with np.errstate(over="ignore", under="ignore"):
            d = F(target - old)
            p = F(d * adapt)
            exposure = F(old + p)
    return dict(nMetered=n2, meanLog2Q16=m, target=F(target), exposure=F(exposure), frames=min(int(prev_frames) + 1, 2 ** 32 - 1), raw=raw)


def meter(img, prev_state, tables, **desc):
    """What rt_meter leaves in the state: one METER_STATE_DTYPE record.  prev_state: the record before the call (zeros at first)."""
    out = np.zeros(1, dtype=L.METER_STATE_DTYPE)[0]
    hs = histogram(img)
    for k, v in hs.items():
        out[k] = v
    s = solve(hs["hist"], prev_state["exposure"], prev_state["frames"], tables, **desc)
    for k in ("nMetered", "meanLog2Q16", "target", "exposure", "frames"):
        out[k] = s[k]
    return out


def state_bytes(rec):
    return np.asarray(rec, dtype=L.METER_STATE_DTYPE).reshape(1).view(np.uint8)


def describe_difference(got, want):
    """Field names in which two state records differ bit for bit (for assertion messages)."""
    g, w = np.asarray(got, dtype=L.METER_STATE_DTYPE).reshape(1), np.asarray(want, dtype=L.METER_STATE_DTYPE).reshape(1)
    return [f"{k}: got {g[k][0]!r} want {w[k][0]!r}" for k in L.METER_STATE_DTYPE.names
            if np.ascontiguousarray(g[k]).tobytes() != np.ascontiguousarray(w[k]).tobytes()]


# ---- the toned pack ---------------------------------------------------------------------------------------------------------------
def tone_curve(y, tone, white):
    """t of the header for y = x * e (float32 array): NaN and !(y > 0) -> 0 here (code 0 either way)."""
    with np.errstate(all="ignore"):
        ys = np.where(y > 0, np.minimum(y, F(65536.0)), F(0.0)).astype(np.float32)
        if tone == "reinhard":
            invW2 = F(1.0) / (F(white) * F(white))
            a = ys * invW2
            b = F(1.0) + a
            c = ys * b
            d = F(1.0) + ys
            return (c / d).astype(np.float32)
        assert tone == "aces"
        n = ys * ((F(2.51) * ys) + F(0.03))
        d = (ys * ((F(2.43) * ys) + F(0.59))) + F(0.14)
        return (n / d).astype(np.float32)


def code_of(t, fmt, table):
    """rt_display_pack's rule on float32 t: NaN and !(t > 0) -> 0, t >= 1 -> 255, else rint(t * 255) or the threshold count."""
    with np.errstate(all="ignore"):
        inside = (t > 0) & (t < 1)
        ts = np.where(inside, t, F(0.5)).astype(np.float32)
        if fmt == "linear":
            q = np.rint(ts * F(255.0)).astype(np.int64)
        else:
            q = np.searchsorted(table[1:], ts.reshape(-1), side="right").reshape(ts.shape)
        q = np.where(t >= 1, 255, q)
        q = np.where(~(t > 0), 0, q)
    return q


def pack_toned(img, fmt, flip, exposure, table, tone="none", white=1.0, dev_exposure=None):
    """img float32 [h, w, 4] -> uint8 [h, w, 4]; dev_exposure: the float32 the device holds, or None."""
    with np.errstate(all="ignore"):
        e = F(exposure) if dev_exposure is None else F(F(exposure) * F(dev_exposure))
        y = (img[..., :3].astype(np.float32) * e).astype(np.float32)
        t = y if tone == "none" else tone_curve(y, tone, white)
    out = np.empty(img.shape[:2] + (4,), dtype=np.uint8)
    out[..., :3] = code_of(t, fmt, table)
    out[..., 3] = 255
    return out[::-1].copy() if flip else out
