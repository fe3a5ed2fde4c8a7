"""The definitions of rt_denoise_guide and rt_denoise (include/rt_mi355.h) restated in numpy float32: the oracle of
tests/test_denoise_host.py and tests/test_denoise.py.  Not a test module.  Every floating-point step is one elementwise numpy float32
operation in the header's order (numpy never fuses a multiply with an add; its float32 divide and sqrt are correctly rounded, as the
device's are); every sum starts at +0 and takes the kept terms one by one in row-major order of its window; exp is the host
instantiation of csrc/rt_mesa_math.h (host.mesa_math), the source the device compiles.

A plane is a float32 array [h, w, 4] holding (r, g, b, var); the sign bit of var marks a skipped pixel.  A guide is an [h, w] array of
layout.DENOISE_GUIDE_DTYPE records."""
import numpy as np

from opengl_raytracing_amd import host
from opengl_raytracing_amd import layout as L

F = np.float32
LIMIT = F(2.0 ** 48)
H5 = [F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16)]
G3 = [F(1 / 4), F(1 / 2), F(1 / 4)]


def luminance(img):
    """Y = (0.2126f*r + 0.7152f*g) + 0.0722f*b: three float32 multiplies, two float32 adds."""
    with np.errstate(all="ignore"):
        r, g, b = (np.asarray(img[..., k], dtype=np.float32) for k in range(3))
        return ((F(0.2126) * r + F(0.7152) * g) + F(0.0722) * b).astype(np.float32)


def usable(img):
    with np.errstate(all="ignore"):
        return (np.abs(np.asarray(img, dtype=np.float32)[..., :3]) <= LIMIT).all(axis=-1)          # (NaN compares false)


def make_guide(normals, objects):
    """A guide plane from unit normals float32 [h, w, 3] and object indices [h, w], as they stand."""
    g = np.zeros(np.shape(objects), dtype=L.DENOISE_GUIDE_DTYPE)
    g["n"], g["object"] = normals, objects
    return g


def make_hits(normals, objects, rng=None):
    """rt_hit records [h, w] with the given raw normals and objects; position and t are noise the guide must ignore."""
    hits = np.zeros(np.shape(objects), dtype=L.HIT_DTYPE)
    hits["normal"], hits["object"] = normals, objects
    if rng is not None:
        hits["position"] = rng.normal(0, 10, hits["position"].shape)
        hits["t"] = rng.uniform(0, 100, hits["t"].shape)
    return hits


def guide(hits):
    """rt_denoise_guide: HIT_DTYPE records -> DENOISE_GUIDE_DTYPE records of the same shape."""
    n = np.asarray(hits["normal"], dtype=np.float32)
    with np.errstate(all="ignore"):
        s = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        r = np.sqrt(s)
        unit = (n / r[..., None]).astype(np.float32)
    out = np.zeros(hits.shape, dtype=L.DENOISE_GUIDE_DTYPE)
    out["n"] = np.where((s > 0)[..., None], unit, F(0))
    out["object"] = hits["object"]
    return out


def _shift(a, dx, dy):
    """out[y, x] = a[y + dy, x + dx] where that lies inside, 0 elsewhere."""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def _inside(h, w, dx, dy):
    y, x = np.mgrid[0:h, 0:w]
    return (y + dy >= 0) & (y + dy < h) & (x + dx >= 0) & (x + dx < w)


def _max0(x):
    with np.errstate(all="ignore"):
        return np.where(x > 0, x, F(0)).astype(np.float32)


def _exp(x):
    return host.mesa_math(np.ascontiguousarray(x, dtype=np.float32).reshape(-1))[:, 3].reshape(np.shape(x))


def counts(moments):
    return np.ascontiguousarray(moments[..., 2]).view(np.uint32)


def spatial_variance(img, gd, count):
    """The spatial estimate of every pixel (meaningless where the pixel is skipped): (var, k)."""
    h, w = img.shape[:2]
    ok, Y, obj = usable(img), luminance(img), gd["object"]
    sY, sYY, k = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), np.int64)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                keep = _inside(h, w, dx, dy) & _shift(ok, dx, dy) & (_shift(obj, dx, dy) == obj)
                Yq = _shift(Y, dx, dy)
                sY = np.where(keep, sY + Yq, sY)
                sYY = np.where(keep, sYY + Yq * Yq, sYY)
                k += keep
        kf = k.astype(np.float32)
        m1, m2 = sY / kf, sYY / kf
        var = _max0(m2 - m1 * m1) / np.maximum(count, 1).astype(np.float32)
    assert var.dtype == np.float32
    return var, k


def prepare(img, moments, gd, min_count=4):
    """The prepare pass: -> plane A."""
    img = np.asarray(img, dtype=np.float32)
    h, w = img.shape[:2]
    ok = usable(img)
    if moments is None:
        count, M2 = np.ones((h, w), np.uint32), np.zeros((h, w), F)
    else:
        count, M2 = counts(moments), np.asarray(moments[..., 1], dtype=np.float32)
    with np.errstate(all="ignore"):
        nf = count.astype(np.float32)
        temporal = (M2 / (nf * (nf - F(1.0)))).astype(np.float32)
    spatial, _ = spatial_variance(img, gd, count)
    var = np.where(count >= np.uint32(min_count), temporal, spatial)
    var = np.where(ok, var, F(-0.0)).astype(np.float32)
    out = img.copy()
    out[..., 3] = var
    return out


def iterate(src, gd, step, sigma_lum=4.0, lum_eps=2.0 ** -10, normal_log2_power=5):
    """One a-trous iteration at `step`: plane -> plane."""
    h, w = src.shape[:2]
    var, skip = src[..., 3], np.signbit(src[..., 3])
    n, obj = gd["n"], gd["object"]
    Y = luminance(src)
    zero = np.zeros((h, w), F)
    with np.errstate(all="ignore"):
        sg, sgv = zero, zero
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                keep = _inside(h, w, dx, dy) & ~_shift(skip, dx, dy) & (_shift(obj, dx, dy) == obj)
                g = G3[dx + 1] * G3[dy + 1]
                sg = np.where(keep, sg + g, sg)
                sgv = np.where(keep, sgv + g * _shift(var, dx, dy), sgv)
        gv = np.where(sg > 0, sgv / np.where(sg > 0, sg, F(1)), F(0)).astype(np.float32)
        sl = F(sigma_lum) * np.sqrt(gv) + F(lum_eps)
        sw, sv, srgb = zero, zero, [zero, zero, zero]
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ox, oy = step * dx, step * dy
                keep = _inside(h, w, ox, oy) & ~_shift(skip, ox, oy) & (_shift(obj, ox, oy) == obj)
                nq = _shift(n, ox, oy)
                c = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                c = _max0(c)
                c = np.where(c < 1, c, F(1)).astype(np.float32)
                for _ in range(int(normal_log2_power)):
                    c = c * c
                wn = np.where(obj < 0, F(1), c)
                wl = np.where(skip, F(0), np.abs(Y - _shift(Y, ox, oy)) / sl).astype(np.float32)
                wgt = ((H5[dx + 2] * H5[dy + 2]) * wn) * _exp(-wl)
                q = _shift(src, ox, oy)
                sw = np.where(keep, sw + wgt, sw)
                for k in range(3):
                    srgb[k] = np.where(keep, srgb[k] + wgt * q[..., k], srgb[k])
                sv = np.where(keep, sv + (wgt * wgt) * q[..., 3], sv)
        through = sw == 0
        den = np.where(through, F(1), sw)
        out = src.copy()
        for k in range(3):
            out[..., k] = np.where(through, src[..., k], srgb[k] / den)
        v = np.where(through, F(0), sv / (den * den))
        out[..., 3] = np.where(skip, F(-0.0), v)
    assert out.dtype == np.float32 and sw.dtype == np.float32 and sl.dtype == np.float32
    return out


def denoise(img, moments, gd, iterations=4, normal_log2_power=5, sigma_lum=4.0, lum_eps=2.0 ** -10, min_count=4):
    """rt_denoise: dict(A, B: what the two scratch planes hold afterwards; out: the output surface; last: the last iteration's plane
    with its variance, which the device replaces by the image's alpha; planes: the prepared plane and the one after every iteration)."""
    img = np.asarray(img, dtype=np.float32)
    planes = [prepare(img, moments, gd, min_count)]
    scratch = [planes[0], np.zeros_like(planes[0])]
    for it in range(int(iterations)):
        nxt = iterate(planes[-1], gd, 1 << it, sigma_lum, lum_eps, normal_log2_power)
        planes.append(nxt)
        if it < iterations - 1:
            scratch[(it & 1) ^ 1] = nxt
    out = planes[-1].copy()
    out[..., 3] = img[..., 3]
    return dict(A=scratch[0], B=scratch[1], out=out, last=planes[-1], planes=planes)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def synthetic_guide(w=64, h=48):
    """Two objects split by a slanted edge and a strip of misses along the top: object 0 is a plane (one normal), object 1 a sphere
    (the normal turns across it), the strip is sky (object -1, normal 0).  -> (guide, distance to the nearest edge in texels)."""
    y, x = np.mgrid[0:h, 0:w]
    obj = np.where(x + 0.25 * (y - 0.5 * h) < 0.5 * w, 0, 1).astype(np.int32)
    obj[:6] = -1
    n = np.zeros((h, w, 3), dtype=np.float32)
    n[obj == 0] = (0.0, 1.0, 0.0)
    u, v = (x - 0.8 * w) / (0.9 * w), (y - 0.5 * h) / (0.9 * w)
    sph = np.stack([u, v, np.sqrt(np.maximum(1 - u * u - v * v, 0.01))], axis=-1)
    sph /= np.linalg.norm(sph, axis=-1, keepdims=True)
    n[obj == 1] = sph[obj == 1].astype(np.float32)
    # Chebyshev distance to the nearest pixel of another object (the image border is no edge)
    dist = np.full((h, w), 64, dtype=np.int64)
    for r in range(1, 33):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if max(abs(dx), abs(dy)) != r:
                    continue
                other = _inside(h, w, dx, dy) & (_shift(obj, dx, dy) != obj)
                dist = np.where(other & (dist > r), r, dist)
    return make_guide(n, obj), dist


def clean_image(gd, values=(0.2, 3.0, 1.0)):
    """The noise-free image of a synthetic guide: grey `values` for object 0, object 1 and the sky; alpha 1."""
    obj = gd["object"]
    v = np.where(obj == 0, values[0], np.where(obj == 1, values[1], values[2])).astype(np.float32)
    img = np.ones(obj.shape + (4,), dtype=np.float32)
    img[..., :3] = v[..., None]
    return img


def lognormal_frames(rng, clean, n, sigma=0.5):
    """n one-sample frames: every colour channel of `clean` times an independent log-normal factor of mean 1."""
    frames = []
    for _ in range(n):
        f = clean.copy()
        f[..., :3] *= np.exp(rng.normal(-0.5 * sigma * sigma, sigma, clean[..., :3].shape)).astype(np.float32)
        frames.append(f.astype(np.float32))
    return frames
