"""numpy restatement of rt_display_resample (include/rt_mi355.h) and an independent builder of its tap tables.

resample() is the two formulas of the header in np.float32 throughout, vectorised over pixels and looped over taps, with the
tables as arguments: separate multiplies and adds, the accumulator starting as the first product, taps in table order, indices
clamped to the image.  taps() builds the table of one axis without the library: AREA and TRIANGLE in fractions.Fraction (windows
and weights exact, one rounding to float32), LANCZOS3 in Python doubles."""
import math
from fractions import Fraction

import numpy as np

AREA, TRIANGLE, LANCZOS3 = 0, 1, 2
FILTERS = {"area": AREA, "triangle": TRIANGLE, "lanczos3": LANCZOS3}
MAX_TAPS = 64


def _sinc(x):
    if x == 0.0:
        return 1.0
    if x == math.floor(x):
        return 0.0
    return math.sin(math.pi * x) / (math.pi * x)


def _lanczos3(x):
    x = abs(x)
    return _sinc(x) * _sinc(x / 3.0) if x < 3.0 else 0.0


def windows(S, D, filter):
    """[(j0, j1)] per destination index, exact."""
    f = FILTERS.get(filter, filter)
    out = []
    for i in range(D):
        if f == AREA:
            out.append(((i * S) // D, ((i + 1) * S + D - 1) // D - 1))
            continue
        R = 1 if f == TRIANGLE else 3
        fs = max(Fraction(1), Fraction(S, D))
        c = Fraction((2 * i + 1) * S - D, 2 * D)
        lo, hi = c - R * fs, c + R * fs
        j0, j1 = math.floor(lo) + 1, math.ceil(hi) - 1               # strictly inside (lo, hi)
        assert lo < j0 and j0 - 1 <= lo and j1 < hi and hi <= j1 + 1
        out.append((j0, j1))
    return out


def taps(S, D, filter):
    """-> (n, first int32[D], weights float32[D, n]) or None when n exceeds the cap."""
    f = FILTERS.get(filter, filter)
    win = windows(S, D, f)
    n = max(j1 - j0 + 1 for j0, j1 in win)
    if n > MAX_TAPS:
        return None
    first = np.array([j0 for j0, _ in win], dtype=np.int32)
    weights = np.zeros((D, n), dtype=np.float32)
    fs = max(Fraction(1), Fraction(S, D))
    for i, (j0, j1) in enumerate(win):
        c = Fraction((2 * i + 1) * S - D, 2 * D)
        if f == AREA:
            w = [Fraction(min((i + 1) * S, (j + 1) * D) - max(i * S, j * D), S) for j in range(j0, j1 + 1)]
        elif f == TRIANGLE:
            v = [max(Fraction(0), 1 - abs((j - c) / fs)) for j in range(j0, j1 + 1)]
            w = [x / sum(v) for x in v]
        else:
            M = max(S, D)
            v = [_lanczos3((2 * D * j - (2 * i + 1) * S + D) / (2 * M)) for j in range(j0, j1 + 1)]      # (j - c) / fs, one quotient
            tot = 0.0
            for x in v:
                tot += x
            w = [x / tot for x in v]
        weights[i, : len(w)] = [np.float32(float(x)) if not isinstance(x, Fraction) else _f32(x) for x in w]
    return n, first, weights


def _f32(q):
    """A Fraction rounded to the nearest float32.  float(q) is correctly rounded to double; when that is q itself, numpy's
    rounding to float32 is the answer (ties to even).  Otherwise q is no float32 tie (a tie is a double), so the nearest of
    the float32 around float(q) is unique: picked by exact distance, which undoes a double rounding."""
    d = float(q)
    f = np.float32(d)
    if Fraction(d) == q:
        return f
    cands = (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf)))
    return min(cands, key=lambda c: abs(Fraction(float(c)) - q))


def _pass(src, first, weights, axis):
    """One separable pass along `axis` of src [H, W, 4] float32."""
    size = src.shape[axis]
    n = weights.shape[1]
    acc = None
    with np.errstate(all="ignore"):
        for k in range(n):
            idx = np.clip(first.astype(np.int64) + k, 0, size - 1)
            s = np.take(src, idx, axis=axis)
            w = weights[:, k].astype(np.float32)
            w = w[None, :, None] if axis == 1 else w[:, None, None]
            p = (w * s).astype(np.float32)
            acc = p if acc is None else (acc + p).astype(np.float32)
    return acc


def resample(src, tx, ty):
    """src [srcH, srcW, 4] float32; tx, ty = (n, first, weights) of the x and y axis -> [dstH, dstW, 4] float32."""
    src = np.ascontiguousarray(src, dtype=np.float32)
    h = _pass(src, tx[1], tx[2], 1)
    return _pass(h, ty[1], ty[2], 0)
