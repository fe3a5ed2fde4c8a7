"""The definitions of rt_upsample and rt_image_put_at (include/rt_mi355.h) restated in numpy float32: the oracle of
tests/test_upsample_host.py and tests/test_upsample.py.  Not a test module.  The position is computed in Python integers; every
floating-point step is one elementwise numpy float32 operation in the header's order (numpy never fuses a multiply with an add; its
float32 divide and sqrt are correctly rounded, as the device's are); every sum starts at +0 and takes the kept terms one by one, j outer
and i inner; the normalisation of the normals is denoise_oracle.guide and the list's order is adaptive_oracle.tile_order.

A low image is float32 [lh, lw, 4]; hits are [h, w] arrays of layout.HIT_DTYPE records; a list is a uint32 array [n, 2] of (x, y) rows."""
import numpy as np

import adaptive_oracle as DO
import denoise_oracle as NO
from opengl_raytracing_amd import layout as L

F = np.float32
LIMIT = F(2.0 ** 48)
TILE = L.SELECT_TILE
INTERPOLATED, HOLE, ORPHAN = 0, 1, 2
# low -> high, (width, height) each: the shapes of the GPU tests
SHAPES = [((1, 1), (1, 1)), ((1, 1), (5, 3)), ((3, 2), (7, 5)), ((7, 7), (7, 7)), ((9, 5), (67, 9)), ((65, 3), (257, 3)),
          ((133, 5), (265, 9)), ((65, 35), (130, 70))]


def shape_id(shape):
    (lw, lh), (w, h) = shape
    return f"{lw}x{lh}-{w}x{h}"


def position(low, high):
    """The position of every output coordinate 0 .. high-1 in a low image of `low` texels -> (i0 int64 [high], f float32 [high]):
    num = (2v + 1)*low - high;  i0 = floor(num / (2*high));  f = (float)(num - i0*2*high) / (float)(2*high).  Python integers."""
    i0, f = np.zeros(high, dtype=np.int64), np.zeros(high, dtype=np.float32)
    for v in range(high):
        num = (2 * v + 1) * low - high
        q = num // (2 * high)                                   # Python's // rounds towards minus infinity
        i0[v] = q
        f[v] = F(num - q * 2 * high) / F(2 * high)
    return i0, f


def usable(img):
    """All four channels finite with |v| <= 2^48 (a NaN compares false)."""
    with np.errstate(all="ignore"):
        return (np.abs(np.asarray(img, dtype=np.float32)) <= LIMIT).all(axis=-1)


def _normal_weight(gp, gq, power):
    with np.errstate(all="ignore"):
        n, nq = gp["n"], gq["n"]
        c = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
        c = np.where(c > 0, c, F(0)).astype(np.float32)         # max0
        c = np.where(c < 1, c, F(1)).astype(np.float32)         # min1
        for _ in range(int(power)):
            c = c * c
    assert c.dtype == np.float32
    return np.where(gp["object"] < 0, F(1), c).astype(np.float32)


def _divide(s, sw, on):
    """s / sw per channel where `on`, zeros elsewhere."""
    with np.errstate(all="ignore"):
        den = np.where(on, sw, F(1)).astype(np.float32)
        return np.where(on[..., None], s / den[..., None], F(0)).astype(np.float32)


def upsample(low, hits_low, hits_high, normal_log2_power=5, min_weight=0.25, capacity=None):
    """rt_upsample -> dict(out float32 [h, w, 4]; stage int [h, w] (INTERPOLATED, HOLE: filled by stage 2, ORPHAN); sw1: stage 1's sw;
    full_list: every hole in the list's order; list: its first min(holes, capacity) entries (capacity None: all); state: one
    SELECT_STATE_DTYPE record; ballots: uint64 [tiles], bit (y % 8) * 8 + x % 8 of a tile's word set for a hole)."""
    low = np.asarray(low, dtype=np.float32)
    lh, lw = low.shape[:2]
    h, w = hits_high.shape
    assert hits_low.shape == (lh, lw) and 1 <= lw <= w and 1 <= lh <= h
    gl, gh = NO.guide(hits_low), NO.guide(hits_high)
    ok = usable(low)
    ix0, fx = position(lw, w)
    iy0, fy = position(lh, h)
    IX0, IY0 = np.broadcast_to(ix0[None, :], (h, w)), np.broadcast_to(iy0[:, None], (h, w))
    wx = [np.broadcast_to((F(1.0) - fx)[None, :], (h, w)), np.broadcast_to(fx[None, :], (h, w))]
    wy = [np.broadcast_to((F(1.0) - fy)[:, None], (h, w)), np.broadcast_to(fy[:, None], (h, w))]
    objp = gh["object"]

    def window(offsets, weight):
        sw, s = np.zeros((h, w), F), np.zeros((h, w, 4), F)
        with np.errstate(all="ignore"):
            for j in offsets:
                for i in offsets:
                    qx, qy = IX0 + i, IY0 + j
                    inside = (qx >= 0) & (qx < lw) & (qy >= 0) & (qy < lh)
                    cx, cy = np.clip(qx, 0, lw - 1), np.clip(qy, 0, lh - 1)     # (read only where `inside`)
                    keep = inside & ok[cy, cx] & (gl["object"][cy, cx] == objp)
                    wn = _normal_weight(gh, gl[cy, cx], normal_log2_power)
                    wt, keep = weight(i, j, wn, keep)
                    assert wt.dtype == np.float32
                    sw = np.where(keep, sw + wt, sw)
                    s = np.where(keep[..., None], s + wt[..., None] * low[cy, cx], s)
        assert sw.dtype == np.float32 and s.dtype == np.float32
        return sw, s

    sw1, s1 = window((0, 1), lambda i, j, wn, keep: ((wx[i] * wy[j]) * wn, keep))
    with np.errstate(all="ignore"):
        interpolated = (sw1 > 0) & (sw1 >= F(min_weight))
    sw2, s2 = window((-1, 0, 1, 2), lambda i, j, wn, keep: (wn, keep & (wn != 0)))
    filled = ~interpolated & (sw2 > 0)
    orphan = ~interpolated & ~filled
    xs, ys = np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64)
    lx, ly = np.minimum(xs * lw // w, lw - 1), np.minimum(ys * lh // h, lh - 1)
    copied = low[ly[:, None], lx[None, :]]
    out = np.where(interpolated[..., None], _divide(s1, sw1, interpolated), np.where(filled[..., None], _divide(s2, sw2, filled), copied))
    out = np.ascontiguousarray(out, dtype=np.float32)
    out[orphan] = copied[orphan]                                # as it stands: the bits, NaN payloads included
    stage = np.where(interpolated, INTERPOLATED, np.where(filled, HOLE, ORPHAN))
    hole = ~interpolated
    ox, oy = DO.tile_order(w, h)
    keep = hole[oy, ox]
    full = np.stack([ox[keep], oy[keep]], axis=-1).astype(np.uint32)
    n = len(full)
    cap = n if capacity is None else int(capacity)
    state = np.zeros(1, dtype=L.SELECT_STATE_DTYPE)[0]
    state["nPixels"], state["nSelected"], state["nListed"] = w * h, n, min(n, cap)
    state["capacity"], state["overflow"], state["nCapped"] = min(cap, 2 ** 32 - 1), int(n > cap), int(orphan.sum())
    tiles_x = (w + TILE - 1) // TILE
    ballots = np.zeros(tiles_x * ((h + TILE - 1) // TILE), dtype=np.uint64)
    hy, hx = np.nonzero(hole)
    np.bitwise_or.at(ballots, (hy // TILE) * tiles_x + hx // TILE, np.uint64(1) << ((hy % TILE) * TILE + hx % TILE).astype(np.uint64))
    return dict(out=out, stage=stage, sw1=sw1, full_list=full, list=full[:min(n, cap)].copy(), state=state, ballots=ballots)


def image_put_at(image, samples, pixels):
    """rt_image_put_at: image float32 [h, w, 4], samples float32 [n, 4], pixels uint32 [n, 2] (each image pixel at most once) -> the
    new image; entries outside the image are skipped."""
    h, w = image.shape[:2]
    pixels = np.asarray(pixels).astype(np.uint32).reshape(-1, 2)
    samples = np.asarray(samples, dtype=np.float32).reshape(-1, 4)
    inside = (pixels[:, 0] < w) & (pixels[:, 1] < h)
    x, y = pixels[inside, 0].astype(np.int64), pixels[inside, 1].astype(np.int64)
    assert len(set(zip(x.tolist(), y.tolist()))) == len(x), "a pixel is listed twice: the result is unspecified"
    out = image.copy()
    out.view(np.uint32)[y, x] = samples.view(np.uint32)[inside]
    return out


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
SPECIAL_TEXELS = np.array([np.nan, np.inf, -np.inf, 2.0 ** 49, -(2.0 ** 49), np.nextafter(F(2.0 ** 48), F(np.inf)), 2.0 ** 48, -(2.0 ** 48), 0.0,
                           -0.0, 1e-40, -3.5], dtype=np.float32)   # the first six are not usable


def _scene(u, v):
    """Object index and raw normal of the point (u, v) of the unit square, the same function for both resolutions: a plane (object 0,
    one raw normal of length 2), a sphere (1, the normal turns across it), a second plane with the opposite normal (2), a strip of
    sky along the top (-1, normal 0)."""
    obj = np.where(u + 0.3 * (v - 0.5) < 0.45, 0, 1).astype(np.int32)
    obj = np.where((u - 0.25) ** 2 + (v - 0.6) ** 2 < 0.03, 2, obj)
    obj = np.where(v < 0.12, -1, obj).astype(np.int32)
    n = np.zeros(u.shape + (3,), dtype=np.float32)
    n[obj == 0] = (0.0, 2.0, 0.0)
    a, b = (u - 0.8) / 0.9, (v - 0.5) / 0.9
    sph = np.stack([a, b, np.sqrt(np.maximum(1 - a * a - b * b, 0.01))], axis=-1).astype(np.float32)
    n[obj == 1] = sph[obj == 1]
    n[obj == 2] = (0.0, -0.5, 0.0)
    return obj, n


def _hits(w, h, rng):
    y, x = np.mgrid[0:h, 0:w]
    obj, n = _scene((x + 0.5) / w, (y + 0.5) / h)
    return NO.make_hits(n, obj, rng)


def make_case(shape, seed=0):
    """Hand-written inputs of one shape -> (low float32 [lh, lw, 4], hits_low, hits_high).  Both hit planes sample one scene; then the
    high plane alone receives what the low plane misses -- a blob of an object the low plane does not have (orphans), checkerboards of
    period 1, 2 and 3 between the pixel's object and objects 7 / 8 (8 has low-resolution pixels nearby only where planted: stage 2),
    a few more misses -- and both receive zero, denormal, huge and antiparallel normals.  The low image is noise with every special
    value of SPECIAL_TEXELS planted in colour and in alpha."""
    (lw, lh), (w, h) = shape
    rng = np.random.default_rng(1000 * w + 10 * h + lw + seed)
    hl, hh = _hits(lw, lh, rng), _hits(w, h, rng)
    y, x = np.mgrid[0:h, 0:w]
    # an object only the high plane has, and one the low plane has a single pixel of
    # (the smallest shapes keep most of the scene: one pixel of the blob, no checkerboards)
    blob = ((x - 0.6 * w) ** 2 + (y - 0.7 * h) ** 2) < max(1.5, 0.004 * w * h) if w * h >= 200 else (x == w - 1) & (y == h - 1) & (w * h > 1)
    hh["object"][blob] = 9
    hh["normal"][blob] = (0.0, 0.0, 1.0)
    for period, x0 in ((1, 0.05), (2, 0.35), (3, 0.7)) if w >= 16 else ():
        band = (x >= int(x0 * w)) & (x < int(x0 * w) + max(2, w // 6)) & (y >= h // 3)
        cells = ((x // period + y // period) % 2 == 0) & band
        hh["object"][cells] = 7 if period == 2 else 8
        hh["normal"][cells] = (0.6, 0.0, 0.8)
    if lw >= 8:                                                 # (one low pixel of object 8: its neighbours in the 4 x 4 window find it)
        hl["object"][lh // 2, int(0.1 * lw)] = 8
        hl["normal"][lh // 2, int(0.1 * lw)] = (0.3, 0.0, 0.4)
    miss = rng.uniform(0, 1, (h, w)) < 0.02
    hh["object"][miss] = -1
    hh["normal"][miss] = 0.0
    # special normals on both planes: zero, denormal, too long for s, long, antiparallel
    for hits, n in ((hl, lw * lh), (hh, w * h)):
        flat_n, k = hits["normal"].reshape(-1, 3), n // 23      # (none on a plane of fewer than 23 pixels)
        pick = rng.permutation(n)[: 5 * k]
        flat_n[pick[:k]] = 0.0
        flat_n[pick[k:2 * k]] = (1e-40, 0.0, -1e-41)
        flat_n[pick[2 * k:3 * k]] = (1e30, -1e30, 1e25)
        flat_n[pick[3 * k:4 * k]] *= F(1e15)
        flat_n[pick[4 * k:]] *= F(-1.0)
    low = rng.uniform(0.0, 4.0, (lh, lw, 4)).astype(np.float32)
    low[..., 3] = rng.uniform(0.5, 1.0, (lh, lw))
    flat = low.reshape(-1)
    if lw * lh >= 12:
        at = rng.permutation(lw * lh)[: min(2 * len(SPECIAL_TEXELS), lw * lh // 3)]
        for k, t in enumerate(at):
            flat[4 * t + (3 if k % 2 else k // 2 % 3)] = SPECIAL_TEXELS[k % len(SPECIAL_TEXELS)]
    return low, hl, hh
