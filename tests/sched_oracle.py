"""Plain numpy references of the tile scheduler (csrc/rt_sched.cpp, the three scheduling kernels of csrc/rt_kernels.hip), for
tests/test_sched.py and tests/test_sched_host.py.

lpt_bins restates rt_lpt_sort_kernel's binning exactly.  predicted_classes restates rt_predict_tiles_kernel: one path per tile,
hits from rt_trace_rays, costs summed in fp64 with the kernel's prices, and an INTERVAL of classes per tile where this
restatement alone cannot decide what the kernel's fp32 arithmetic decides (a cost on a class boundary, a light at grazing
incidence, a centre pixel on a silhouette)."""
import collections
import fractions

import numpy as np

F = np.float32

# ---- the predictor's prices, rt_kernels.hip:700-759 (rt_predict_tiles_kernel) ---------------------------------------------------
PRICE = dict(
    start=300.0,                          # :700  ray generation, stores
    trav=(250.0, 12.0, 64, 2.0),          # :713  250 + 12 * min(nObj, 64) + 2 * nObj per traversal
    cand=(1.5, 1.0 / 28.0),               # :714  1.5 + nObj / 28 candidates per shadow ray
    hit=350.0,                            # :740  hit set-up, parking, next direction
    light=330.0,                          # :753  light set-up + computePBR, per light of a hit
    shadow=(120.0, 64, 50.0, 70.0),       # :755  120 + min(pcf, 64) * (50 + 70 * cand), a lit PCF / PCSS light
    pcss=(16.0, 60.0, 25.0, 32),          # :756  + 16 * (60 + 25 * min(nObj, 32)), a lit PCSS light
    sss=(4.0, 60.0),                      # :759  4 * (trav + 60) on a subsurface material
)
CLASS_EPS = 1e-3                          # 4 * log2(cost) this close to an integer: either class
LIT_EPS = 1e-3                            # a `lit` dot product this close to zero: either price
NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1))


# ---- the measured order ----------------------------------------------------------------------------------------------------------
def lpt_bins(costs):
    """The bin (0 heaviest .. 255 lightest) rt_lpt_sort_kernel puts every cost in: scale = 255.0f / (float)max(1, max cost),
    bin = 255 - min(255, (int)((float)cost * scale)).  IEEE division, no contraction, (float)unsigned rounds to nearest even as
    numpy's astype does: exact."""
    c = np.asarray(costs, dtype=np.uint32).reshape(-1)
    if c.size == 0:
        return np.zeros(0, dtype=np.int64)
    scale = F(255) / F(max(1, int(c.max())))
    scaled = c.astype(F) * scale
    assert scaled.dtype == F
    return 255 - np.minimum(255, scaled.astype(np.int64))


def f32_round(q):
    """A positive rational rounded to the nearest fp32 (ties to even), as a rational; integers only (normal range)."""
    q = fractions.Fraction(q)
    if q == 0:
        return q
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if fractions.Fraction(2) ** e > q:
        e -= 1
    assert fractions.Fraction(2) ** e <= q < fractions.Fraction(2) ** (e + 1) and e > -126
    ulp = fractions.Fraction(2) ** (e - 23)
    k = q / ulp
    r = k.numerator // k.denominator
    rem = k - r
    if rem > fractions.Fraction(1, 2) or (rem == fractions.Fraction(1, 2) and r % 2 == 1):
        r += 1
    return r * ulp


def lpt_bins_integer(costs):
    """lpt_bins in Python integers and rationals, no floating-point type involved."""
    costs = [int(c) for c in costs]
    scale = f32_round(fractions.Fraction(255) / f32_round(max([1] + costs)))
    out = []
    for c in costs:
        v = f32_round(f32_round(c) * scale)
        out.append(255 - min(255, v.numerator // v.denominator))
    return out


# ---- the predicted order ---------------------------------------------------------------------------------------------------------
def cost_class(cost, eps=0.0):
    """clamp(int(4 * log2(max(cost, 1))) - 32, 0, 31), with 4 * log2 shifted by eps first."""
    x = 4.0 * np.log2(np.maximum(np.asarray(cost, dtype=np.float64), 1.0)) + eps
    return np.clip(np.floor(x).astype(np.int64) - 32, 0, 31)


def pull_up(cls):
    """The neighbour pull-up as coded: in every block of 64 consecutive tile indices c = max(c, max(left, right) - 1), all lanes at
    once from the classes before it; lane 0 has no left neighbour, lane 63 no right one, lanes past the last tile carry the class
    of the start cost.  Monotonic in every input, so an interval goes through it bound by bound."""
    cls = np.asarray(cls, dtype=np.int64)
    n = cls.size
    padded = np.full(-(-n // 64) * 64, int(cost_class(PRICE["start"])), dtype=np.int64)
    padded[:n] = cls
    rows = padded.reshape(-1, 64)
    left = np.zeros_like(rows)
    right = np.zeros_like(rows)
    left[:, 1:] = rows[:, :-1]
    right[:, :-1] = rows[:, 1:]
    return np.maximum(rows, np.maximum(left, right) - 1).reshape(-1)[:n]


# lo, hi: the class interval; ambiguous: the tile's OWN path is undecided (class boundary, grazing light, silhouette); decided:
# lo == hi (an unambiguous tile beside an ambiguous one may still have an interval, through the pull-up); pcf / pcss / pulled:
# decided unambiguous tiles priced with a shadow term / the blocker-search term / the subsurface term / whose class the pull-up raised
Predicted = collections.namedtuple("Predicted", "lo hi ambiguous decided pcf pcss sss pulled")


def _dot(a, b):
    return (a * b).sum(-1)


def _unit(v):
    return v / np.sqrt(_dot(v, v))[..., None]


def predicted_classes(rt, sc, p):
    """The class interval [lo, hi] of every tile of frame p of scene sc (raster tile order) and the masks of `Predicted`.
    rt: a context holding sc, for rt_camera_rays and rt_trace_rays.

    No hemisphere_dir and no refraction here: maxRayDepth == 1, or every object a followed path bounces off has
    diffuseStrength == 0 and transparency == 0 (asserted)."""
    import torch
    obj, lts = sc.objects, sc.lights
    n_obj, n_lt, depth = len(obj), len(lts), int(p.maxRayDepth)
    w, h = int(p.regionW), int(p.regionH)
    tiles_x, tiles_y = -(-w // 8), -(-h // 8)
    n = tiles_x * tiles_y
    ti, tj = np.arange(n) % tiles_x, np.arange(n) // tiles_x
    ci, cj = np.minimum(8 * ti + 4, w - 1), np.minimum(8 * tj + 4, h - 1)

    d_rays = rt.camera_rays(p)
    torch.cuda.synchronize()
    image = d_rays.cpu().numpy()
    rays = np.stack([image[np.clip(cj + dj, 0, h - 1), np.clip(ci + di, 0, w - 1)] for di, dj in ((0, 0),) + NEIGHBOURS], axis=1).copy()
    live = ~(rays[..., 4:7] == 0).all(-1)                      # [n, 5]; the all-zero ray: a pixel outside the image, a dead lane
    watch = live[:, 1:] & live[:, :1]                          # (which pixels lie outside the image is integer arithmetic: no doubt there)

    t_a, t_b, t_cap, t_c = PRICE["trav"]
    trav = t_a + t_b * min(n_obj, t_cap) + t_c * n_obj
    cand = PRICE["cand"][0] + n_obj * PRICE["cand"][1]
    s_a, s_cap, s_b, s_c = PRICE["shadow"]
    b_n, b_a, b_b, b_cap = PRICE["pcss"]
    shadow = np.zeros(n_lt)
    for k in range(n_lt):
        if int(lts["shadowType"][k]) in (1, 2):
            shadow[k] = s_a + min(max(int(lts["pcfSamples"][k]), 0), s_cap) * (s_b + s_c * cand)
            if int(lts["shadowType"][k]) == 2:
                shadow[k] += b_n * (b_a + b_b * min(n_obj, b_cap))
    sss = PRICE["sss"][0] * (trav + PRICE["sss"][1])
    worst_bounce = trav + PRICE["hit"] + n_lt * PRICE["light"] + shadow.sum() + (sss if n_obj and (obj["subsurfaceScatter"] > 0).any() else 0.0)

    lo = np.full(n, PRICE["start"])
    hi = lo.copy()
    doubt = np.zeros(n, dtype=bool)                            # some price of the path was either-or
    pcf = np.zeros(n, dtype=bool)
    pcss = np.zeros(n, dtype=bool)
    subsurface = np.zeros(n, dtype=bool)
    alive = live[:, 0].copy()
    for d in range(depth):
        if not alive.any():
            break
        hits = rt.trace_rays(rays.reshape(-1, 8)).reshape(n, 5)
        o = hits["object"]
        # a silhouette: the kernel's slabs may send the centre ray either way.  From the path ending here (this traversal, a miss)
        # to the costliest continuation.
        edge = alive & (watch & (o[:, 1:] != o[:, :1])).any(1)
        lo[edge] += trav
        hi[edge] += (depth - d) * worst_bounce
        doubt |= edge
        alive &= ~edge
        lo[alive] += trav
        hi[alive] += trav
        alive &= o[:, 0] >= 0
        lo[alive] += PRICE["hit"]
        hi[alive] += PRICE["hit"]
        idx = np.maximum(o[:, 0], 0)
        pos, nrm = hits["position"][:, 0].astype(np.float64), hits["normal"][:, 0].astype(np.float64)
        for k in range(n_lt):
            ltype = int(lts["type"][k])
            stored = _unit(lts["direction"][k].astype(np.float64) * (-1.0 if ltype == 1 else 1.0))      # as rt_compile_scene_kernel stores it
            if ltype == 1:
                ld = np.broadcast_to(stored, pos.shape)
                dots = _dot(nrm, ld)[:, None]
            else:
                with np.errstate(invalid="ignore", divide="ignore"):
                    ld = _unit(lts["position"][k].astype(np.float64) - pos)
                dots = _dot(nrm, ld)[:, None]
                if ltype == 2:
                    dots = np.concatenate([dots, _dot(ld, stored)[:, None]], axis=1)
            surely = alive & (dots > LIT_EPS).all(1)
            maybe = alive & (dots > -LIT_EPS).all(1)
            lo[alive] += PRICE["light"]
            hi[alive] += PRICE["light"]
            if shadow[k] > 0.0:
                lo[surely] += shadow[k]
                hi[maybe] += shadow[k]
                doubt |= maybe & ~surely
                pcf |= surely
                if int(lts["shadowType"][k]) == 2:
                    pcss |= surely
        sub = alive & (obj["subsurfaceScatter"][idx] > 0) if n_obj else alive & False
        lo[sub] += sss
        hi[sub] += sss
        subsurface |= sub
        if d + 1 >= depth:
            break
        bouncing = np.unique(o[(alive[:, None] & np.concatenate([np.ones((n, 1), bool), watch], axis=1)) & (o >= 0)])
        assert not (obj["diffuseStrength"][bouncing] > 0).any() and not (obj["transparency"][bouncing] > 0).any(), \
            "predicted_classes follows mirror reflections only"
        rd, nn, pp = rays[..., 4:7], hits["normal"], hits["position"]
        dn = (nn[..., 2] * rd[..., 2] + nn[..., 1] * rd[..., 1]) + nn[..., 0] * rd[..., 0]       # the kernel's order of additions
        nxt = rays.copy()
        nxt[..., 4:7] = rd - nn * (F(2.0) * dn)[..., None]                                         # reflect(rd, N), fp32
        nxt[..., 0:3] = pp + nn * F(0.001)
        keep = o < 0
        nxt[keep] = rays[keep]
        rays = nxt
        watch &= o[:, 1:] >= 0

    own_lo, own_hi = cost_class(lo, -CLASS_EPS), cost_class(hi, CLASS_EPS)
    c_lo, c_hi = pull_up(own_lo), pull_up(own_hi)
    assert (c_lo <= c_hi).all()
    ambiguous = (own_lo != own_hi) | doubt
    sure = ~ambiguous & (c_lo == c_hi)
    return Predicted(c_lo, c_hi, ambiguous, c_lo == c_hi, pcf & sure, pcss & sure, subsurface & sure, sure & (c_lo > own_lo))
