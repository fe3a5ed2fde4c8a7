"""The definition of rt_accum_reproject (include/rt_mi355.h) restated in numpy float32 / uint32: the oracle of
tests/test_reproject_host.py and tests/test_reproject.py.  Not a test module.  Every floating-point step is one elementwise numpy
float32 operation in the header's order (numpy never fuses a multiply with an add; its float32 divide and sqrt are correctly
rounded, as the device's are).  tan_ is the host instantiation of csrc/rt_mesa_math.h (host.mesa_math), the source the library
compiles.

An accumulator is a float32 array [2, h, w, 4] with the device's bytes (accum_oracle's), hits are layout.HIT_DTYPE arrays [h, w]."""
import numpy as np

from opengl_raytracing_amd import host
from opengl_raytracing_amd import layout as L

F = np.float32
REUSED, REJECTED, OFFSCREEN, MISS = 0, 1, 2, 3
DEFAULTS = dict(normal_cos_min=0.9, plane_tol=0.01, max_history=32)


def view_scale(p):
    """(sx, sy) of an RtParams, as build_frame computes them: float32 throughout."""
    aspect = F(p.width) / F(p.height)
    tan_fov = host.mesa_math(np.array([(F(p.fovDeg) * F(0.017453292519943295)) * F(0.5)], dtype=np.float32))[0, 2]
    fl = F(p.focalLength)
    return F(F(aspect * tan_fov) * fl), F(tan_fov * fl)


def _vec(a):
    return [F(a[0]), F(a[1]), F(a[2])]


def dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def project(p, P):
    """proj(V, P) for P float32 [..., 3] -> (fx, fy, valid)."""
    P = np.asarray(P, dtype=np.float32)
    sx, sy = view_scale(p)
    hx, hy = F(0.5) * F(p.width), F(0.5) * F(p.height)
    pos, d, r, u = _vec(p.camPos), _vec(p.camDir), _vec(p.camRight), _vec(p.camUp)
    with np.errstate(all="ignore"):
        vx, vy, vz = P[..., 0] - pos[0], P[..., 1] - pos[1], P[..., 2] - pos[2]
        z = dot3(vx, vy, vz, *d)
        x = dot3(vx, vy, vz, *r)
        y = dot3(vx, vy, vz, *u)
        fx = ((x / z) / sx + F(1.0)) * hx - F(0.5)
        fy = ((y / z) / sy + F(1.0)) * hy - F(0.5)
    assert fx.dtype == fy.dtype == np.float32
    return fx, fy, z > 0


def unproject(p, fx, fy, t=1.0):
    """A world position that projects to (fx, fy) in the view p, at depth t along camDir (float64, rounded once to float32): what
    the tests place points with.  The orthonormal basis of rt_camera_vectors is assumed."""
    sx, sy = (np.float64(v) for v in view_scale(p))
    ux = ((np.asarray(fx, dtype=np.float64) + 0.5) / (0.5 * p.width) - 1.0) * sx
    uy = ((np.asarray(fy, dtype=np.float64) + 0.5) / (0.5 * p.height) - 1.0) * sy
    pos, d, r, u = (np.array(list(v), dtype=np.float64) for v in (p.camPos, p.camDir, p.camRight, p.camUp))
    t = np.asarray(t, dtype=np.float64)
    return (pos + t[..., None] * (d + ux[..., None] * r + uy[..., None] * u)).astype(np.float32)


def normalise(n):
    """rt_denoise_guide's rule on float32 [..., 3]: s > 0 ? n / sqrtf(s) : 0."""
    n = np.asarray(n, dtype=np.float32)
    with np.errstate(all="ignore"):
        s = dot3(n[..., 0], n[..., 1], n[..., 2], n[..., 0], n[..., 1], n[..., 2])
        rs = np.sqrt(s)
        out = np.where((s > 0)[..., None], n / rs[..., None], F(0.0)).astype(np.float32)
    return out


def motion(prev, cur, hits_cur):
    """g of every pixel and whether both projections are valid: (gx, gy, valid), float32 [h, w]."""
    h, w = hits_cur.shape
    P = hits_cur["position"]
    pfx, pfy, pv = project(prev, P)
    cfx, cfy, cv = project(cur, P)
    px, py = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    with np.errstate(all="ignore"):
        gx = px + (pfx - cfx)
        gy = py + (pfy - cfy)
    return gx, gy, pv & cv


def reproject(acc_prev, hits_prev, hits_cur, prev, cur, normal_cos_min=0.9, plane_tol=0.01, max_history=32):
    """rt_accum_reproject -> dict(acc: the new accumulator, report: one REPROJECT_REPORT_DTYPE record, cat: the category of every
    pixel, g: (gx, gy), kept: bool [4, h, w], which taps were kept)."""
    h, w = hits_cur.shape
    assert acc_prev.shape == (2, h, w, 4) and hits_prev.shape == (h, w) and acc_prev.dtype == np.float32
    cos_min, tol_k, max_history = F(normal_cos_min), F(plane_tol), int(max_history)
    obj_p = hits_cur["object"]
    gx, gy, valid = motion(prev, cur, hits_cur)
    with np.errstate(all="ignore"):
        inside = valid & (gx > F(-1.0)) & (gx < F(w)) & (gy > F(-1.0)) & (gy < F(h))        # (NaN and inf compare false)
    hit = obj_p >= 0
    tapped = hit & inside
    gxs, gys = np.where(tapped, gx, F(0.0)), np.where(tapped, gy, F(0.0))
    flx, fly = np.floor(gxs), np.floor(gys)
    x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
    ax, ay = gxs - flx, gys - fly
    n_p = normalise(hits_cur["normal"])
    P, t_p = hits_cur["position"], hits_cur["t"]
    mean_q, mY_q, M2_q = acc_prev[0], acc_prev[1, ..., 0], acc_prev[1, ..., 1]
    count_q = np.ascontiguousarray(acc_prev[1, ..., 2]).view(np.uint32)
    n_q_all = normalise(hits_prev["normal"])
    sw = np.zeros((h, w), dtype=np.float32)
    sm = np.zeros((h, w, 4), dtype=np.float32)
    sY = np.zeros((h, w), dtype=np.float32)
    sS = np.zeros((h, w), dtype=np.float32)
    n_min = np.full((h, w), 0xffffffff, dtype=np.uint32)
    kept_any = np.zeros((h, w), dtype=bool)
    kept_taps = np.zeros((4, h, w), dtype=bool)
    with np.errstate(all="ignore"):
        tol = tol_k * t_p
        for k in range(4):
            i, j = k & 1, k >> 1
            qx, qy = x0 + i, y0 + j
            wt = ((ax if i else F(1.0) - ax) * (ay if j else F(1.0) - ay)).astype(np.float32)
            ok = tapped & (wt != 0) & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            cnt = count_q[cy, cx]
            ok &= cnt != 0
            ok &= hits_prev["object"][cy, cx] == obj_p
            nq = n_q_all[cy, cx]
            ok &= ~(dot3(n_p[..., 0], n_p[..., 1], n_p[..., 2], nq[..., 0], nq[..., 1], nq[..., 2]) < cos_min)
            Pq = hits_prev["position"][cy, cx]
            dd = dot3(P[..., 0] - Pq[..., 0], P[..., 1] - Pq[..., 1], P[..., 2] - Pq[..., 2], n_p[..., 0], n_p[..., 1], n_p[..., 2])
            ok &= ~(np.abs(dd) > tol)
            s2 = np.where(cnt >= 2, M2_q[cy, cx] / (cnt.astype(np.int64) - 1).astype(np.float32), F(0.0)).astype(np.float32)
            sw = np.where(ok, sw + wt, sw)
            sm = np.where(ok[..., None], sm + wt[..., None] * mean_q[cy, cx], sm)
            sY = np.where(ok, sY + wt * mY_q[cy, cx], sY)
            sS = np.where(ok, sS + wt * s2, sS)
            n_min = np.where(ok, np.minimum(n_min, cnt), n_min)
            kept_any |= ok
            kept_taps[k] = ok
        n_out = np.minimum(n_min, np.uint32(max_history)).astype(np.uint32)
        mean_o = sm / sw[..., None]
        mY_o = sY / sw
        M2_o = (sS / sw) * (n_out.astype(np.int64) - 1).astype(np.float32)
    assert sw.dtype == sm.dtype == sY.dtype == sS.dtype == mean_o.dtype == mY_o.dtype == M2_o.dtype == np.float32
    acc = np.zeros((2, h, w, 4), dtype=np.float32)
    acc[0][kept_any] = mean_o[kept_any]
    mom = np.stack([mY_o, M2_o, n_out.view(np.float32), np.zeros_like(mY_o)], axis=-1)
    acc[1][kept_any] = mom[kept_any]
    cat = np.where(~hit, MISS, np.where(~inside, OFFSCREEN, np.where(kept_any, REUSED, REJECTED)))
    return dict(acc=acc, report=report(cat, n_out), cat=cat, g=(gx, gy), kept=kept_taps)


def report(cat, n_out):
    """What rt_accum_reproject leaves in the report for these categories and counts: one REPROJECT_REPORT_DTYPE record."""
    out = np.zeros(1, dtype=L.REPROJECT_REPORT_DTYPE)[0]
    r = cat == REUSED
    out["nPixels"] = cat.size
    out["nReused"], out["nRejected"] = int(r.sum()), int((cat == REJECTED).sum())
    out["nOffscreen"], out["nMiss"] = int((cat == OFFSCREEN).sum()), int((cat == MISS).sum())
    out["minCount"] = 0xffffffff                                # the minimum's neutral element: what stays when nothing is reused
    if r.any():
        out["minCount"], out["maxCount"] = int(n_out[r].min()), int(n_out[r].max())
        out["sumCount"] = int(n_out[r].astype(np.uint64).sum())
    return out


def report_bytes(rec):
    return np.asarray(rec, dtype=L.REPROJECT_REPORT_DTYPE).reshape(1).view(np.uint8)


def describe_difference(got, want):
    """Field names in which two report records differ bit for bit (for assertion messages)."""
    g, w = np.asarray(got, dtype=L.REPROJECT_REPORT_DTYPE).reshape(1), np.asarray(want, dtype=L.REPROJECT_REPORT_DTYPE).reshape(1)
    return [f"{k}: got {g[k][0]!r} want {w[k][0]!r}" for k in L.REPROJECT_REPORT_DTYPE.names
            if np.ascontiguousarray(g[k]).tobytes() != np.ascontiguousarray(w[k]).tobytes()]


def counts(acc):
    return np.ascontiguousarray(acc[1, ..., 2]).view(np.uint32)


# ---- analytic scenes: what a first-hit query of them returns, in numpy ------------------------------------------------------------
def empty_hits(w, h):
    hits = np.zeros((h, w), dtype=L.HIT_DTYPE)
    hits["object"] = -1
    return hits


def trace_plane_and_sphere(p, plane_z, sphere=None, jitter=None):
    """The first hits of the view p (looking down -z from rt_camera_vectors' default basis or any other) on the plane z = plane_z
    (object 0, normal (0, 0, 1)) and, in front of it, an optional sphere (centre[3], radius) (object 1), through the pixel centres
    moved by `jitter` pixels ([h, w, 2], default none).  float64 geometry, rounded once: these are inputs, not a contract."""
    w, h = p.width, p.height
    px, py = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    if jitter is not None:
        px, py = px + jitter[..., 0], py + jitter[..., 1]
    sx, sy = (np.float64(v) for v in view_scale(p))
    ux = ((px + 0.5) / (0.5 * w) - 1.0) * sx
    uy = ((py + 0.5) / (0.5 * h) - 1.0) * sy
    pos, d, r, u = (np.array(list(v), dtype=np.float64) for v in (p.camPos, p.camDir, p.camRight, p.camUp))
    dirs = d + ux[..., None] * r + uy[..., None] * u
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    hits = empty_hits(w, h)
    t_pl = (plane_z - pos[2]) / dirs[..., 2]
    on = t_pl > 0
    t = np.where(on, t_pl, np.inf)
    obj = np.where(on, 0, -1)
    normal = np.zeros((h, w, 3))
    normal[on] = (0.0, 0.0, 1.0)
    if sphere is not None:
        c, rad = np.asarray(sphere[0], dtype=np.float64), float(sphere[1])
        oc = pos - c
        b = (dirs * oc).sum(-1)
        disc = b * b - ((oc * oc).sum() - rad * rad)
        ts = -b - np.sqrt(np.where(disc > 0, disc, 0.0))
        hs = (disc > 0) & (ts > 0) & (ts < t)
        t = np.where(hs, ts, t)
        obj = np.where(hs, 1, obj)
        pts = pos + ts[..., None] * dirs
        normal[hs] = ((pts - c) / rad)[hs]
    got = obj >= 0
    hits["object"] = obj
    hits["t"][got] = t[got].astype(np.float32)
    hits["position"][got] = (pos + t[..., None] * dirs)[got].astype(np.float32)
    hits["normal"][got] = normal[got].astype(np.float32)
    return hits


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def make_view(w, h, pos=(0.0, 0.0, 0.0), yaw=-90.0, pitch=0.0, fov=45.0):
    """An RtParams of w x h with rt_camera_vectors' basis (yaw -90, pitch 0 looks down -z with x to the right and y up)."""
    front, right, up = host.camera_vectors(yaw, pitch)
    return L.make_params(w, h, 3, cam_pos=pos, cam_dir=front, cam_right=right, cam_up=up, fov_deg=fov)


def random_accum(rng, w, h, count):
    """An accumulator with means in [0.1, 4), their luminance as mY, M2 in [0, 2 * count) (0 where count < 2) and the given counts."""
    acc = np.zeros((2, h, w, 4), dtype=np.float32)
    acc[0] = rng.uniform(0.1, 4.0, (h, w, 4)).astype(np.float32)
    count = np.broadcast_to(np.asarray(count, dtype=np.uint32), (h, w)).copy()
    acc[1, ..., 0] = (F(0.2126) * acc[0, ..., 0] + F(0.7152) * acc[0, ..., 1]) + F(0.0722) * acc[0, ..., 2]
    acc[1, ..., 1] = np.where(count >= 2, rng.uniform(0.0, 2.0, (h, w)) * count, 0.0).astype(np.float32)
    acc[1, ..., 2] = count.view(np.float32)
    acc[:, count == 0] = 0.0
    return acc
