"""numpy float32 restatement of the two-distance any-hit behind rt_set_accel_shading (csrc/rt_accel_shade.inc): a shadow or blocker
ray of rt_shade_rays is occluded iff some object passes its stored-box test at maxDist and its shape test with 0 < t < limit
(rt_lane.inc's lane_any).  brute_any states that rule over every object; walk_any states the threaded walk over
host.accel_build_host's arrays -- node test at maxDist (accel_oracle.node_pass), object gate at maxDist, accept at limit, then the
loose list -- per ray and per group of 64.  A ray's maxDist is its tMax field.  Also here: the scenes and lights the GPU tests share."""
import numpy as np

import accel_oracle as A
from opengl_raytracing_amd import layout as L
from opengl_raytracing_amd import scenes
from test_query import _cross, _dot, _normalize

F = np.float32
LIMIT_CLASSES = ("minus_one", "zero", "below", "max_dist", "inf")


def shape_hit(ob, o, d, a):
    """(ok[n], t[n]) of shape_test on one object: test_query.restate's arithmetic."""
    typ = int(ob["type"])
    pos = ob["position"].astype(F)
    with np.errstate(all="ignore"):
        if typ == 0:
            oc = o - pos
            b = F(2.0) * _dot(oc, d)
            r = F(ob["radius"])
            cc = _dot(oc, oc) - r * r
            disc = b * b - (F(4.0) * a) * cc
            t = (-b - np.sqrt(disc)) / (F(2.0) * a)
            return ~(disc < F(0.0)) & (t > F(0.0)), t
        if typ == 1:
            nrm = ob["normal"].astype(F)
            denom = _dot(np.broadcast_to(nrm, d.shape), d)
            t = _dot(pos - o, np.broadcast_to(nrm, o.shape)) / denom
            hp = o + d * t[:, None]
            up = np.array([0, 0, 1], F) if abs(F(nrm[1])) > F(0.9) else np.array([0, 1, 0], F)
            right = _normalize(_cross(nrm, up))
            fwd = _normalize(_cross(right, nrm))
            lo = hp - pos
            x = _dot(lo, np.broadcast_to(right, lo.shape))
            z = _dot(lo, np.broadcast_to(fwd, lo.shape))
            sx, sz = F(ob["size"][0]) / F(2.0), F(ob["size"][1]) / F(2.0)
            return (np.abs(denom) > F(1e-6)) & ~(t < F(0.0)) & ~((np.abs(x) > sx) | (np.abs(z) > sz)), t
    return np.zeros(len(o), bool), np.zeros(len(o), F)


def _occludes(ob, o, d, inv, a, max_dist, limit):
    """lane_any's loop body on one object: the stored-box gate at max_dist, the acceptance at limit."""
    gate = A.aabb_pass(ob["bounds_min"].astype(F), ob["bounds_max"].astype(F), o, inv, max_dist)
    ok, t = shape_hit(ob, o, d, a)
    with np.errstate(invalid="ignore"):
        return gate & ok & (t > F(0.0)) & (t < limit)


def brute_any(objects, rays, limit):
    """lane_any: every object for every ray."""
    o, max_dist, d, inv = A._ray_parts(rays)
    with np.errstate(all="ignore"):
        a = _dot(d, d)
    occ = np.zeros(len(o), bool)
    for ob in objects:
        occ |= _occludes(ob, o, d, inv, a, max_dist, limit)
    return occ


def walk_any(objects, acc, rays, limit, group=1):
    """The threaded walk.  group = 1: one walk per ray (LANE); 64: one per 64 consecutive rays, the group descending wherever some
    unresolved ray of it passes the node (WAVE).  A ray with limit <= 0 or NaN is never unresolved: nothing could be accepted."""
    o, max_dist, d, inv = A._ray_parts(rays)
    n = len(o)
    with np.errstate(all="ignore"):
        a = _dot(d, d)
        is_open = limit > F(0.0)
    occ = np.zeros(n, bool)
    nodes = acc.nodes

    def spread(mask):
        if group == 1:
            return mask
        pad = (-n) % group
        g = np.concatenate([mask, np.zeros(pad, bool)]).reshape(-1, group).any(1)
        return np.repeat(g, group)[:n]

    def meet(i, who):
        idx = np.flatnonzero(who & ~occ)
        if len(idx):
            occ[idx] |= _occludes(objects[i], o[idx], d[idx], inv[idx], a[idx], max_dist[idx], limit[idx])

    par = A.parents(nodes)
    reach = np.zeros((len(nodes), n), bool)
    for k in range(len(nodes)):
        reach[k] = reach[par[k]] if par[k] >= 0 else spread(is_open)
        if not reach[k].any():
            continue
        reach[k] &= spread(A.node_pass(nodes["lo"][k], nodes["hi"][k], o, inv, max_dist) & reach[k] & is_open & ~occ)
        if nodes["leaf"][k] != A.INNER:
            first, count = int(nodes["leaf"][k]) >> 4, int(nodes["leaf"][k]) & 15
            for i in acc.order[first:first + count]:
                meet(int(i), reach[k])
    for i in acc.loose:
        meet(int(i), spread(is_open & ~occ))
    return occ


def draw_limits(rays, seed):
    """One limit per ray, its class cycling through LIMIT_CLASSES -> (limit[n], class index[n])."""
    r = np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8)
    max_dist = r[:, 3]
    n = len(r)
    rng = np.random.default_rng(seed)
    cls = np.arange(n) % len(LIMIT_CLASSES)
    with np.errstate(invalid="ignore"):
        below = np.where(np.isfinite(max_dist) & (max_dist > 0), rng.uniform(0, 1, n) * max_dist, rng.uniform(0, 30, n)).astype(F)
    limit = np.select([cls == 0, cls == 1, cls == 2, cls == 3], [F(-1.0), F(0.0), below, max_dist], F(np.inf)).astype(F)
    return limit, cls


# ---- what the GPU tests share ----------------------------------------------------------------------------------------
def branch_cloud_scene(host):
    """test_shade.branch_scene(host, 3)'s six objects and four lights plus 250 filler spheres from default_rng(33): a scene that
    takes every branch of the path tracer and has a real tree."""
    from test_shade import branch_scene
    sc = branch_scene(host, 3)
    rng = np.random.default_rng(33)
    m, base = 250, len(sc.objects)
    objs = L.default_objects(base + m)
    objs[:base] = sc.objects
    extra = objs[base:]
    extra["type"] = L.SPHERE
    extra["position"] = np.stack([rng.uniform(-8, 8, m), rng.uniform(-0.8, 5, m), rng.uniform(-10, 2, m)], -1)
    extra["radius"] = rng.uniform(0.08, 0.35, m)
    extra["albedo"] = rng.uniform(0.2, 1, (m, 3))
    extra["metallic"] = rng.choice([0.0, 1.0], m)
    extra["roughness"] = rng.choice([0.05, 0.5, 1.0], m)
    extra["diffuseStrength"] = rng.choice([0.0, 0.6, 1.0], m)
    extra["transparency"] = rng.choice([0.0, 0.0, 0.9], m)
    extra["ior"] = rng.choice([1.0, 1.5], m)
    extra["subsurfaceScatter"] = rng.choice([0.0, 0.0, 0.0, 0.5], m)
    objs[base:] = extra
    host.generate_aabb(objs)
    sc.objects = objs
    sc.name = "branches+250"
    return sc


def hostile_lights():
    """The five lights of the hostile-scene test: point PCF x 4, directional PCF x 3, area PCSS x 4, a point light of shadowType
    3, and a point PCF light whose position x is NaN (lightDistance NaN: the limit = -1 path)."""
    lt = L.default_lights(5)
    lt[0]["type"], lt[0]["position"], lt[0]["intensity"] = L.POINT, (2.0, 9.0, 3.0), 40.0
    lt[0]["shadowType"], lt[0]["pcfSamples"] = L.SHADOW_PCF, 4
    lt[1]["type"], lt[1]["direction"], lt[1]["intensity"] = L.DIRECTIONAL, (0.5, -1.0, -0.5), 2.0
    lt[1]["shadowType"], lt[1]["pcfSamples"] = L.SHADOW_PCF, 3
    lt[2]["type"], lt[2]["position"], lt[2]["direction"], lt[2]["intensity"] = L.AREA, (-6.0, 12.0, -4.0), (0.0, 1.0, 0.0), 120.0
    lt[2]["shadowType"], lt[2]["pcfSamples"] = L.SHADOW_PCSS, 4
    lt[3]["type"], lt[3]["position"], lt[3]["intensity"] = L.POINT, (-4.0, 5.0, 2.0), 4.0
    lt[3]["shadowType"] = 3
    lt[4]["type"], lt[4]["position"], lt[4]["intensity"] = L.POINT, (np.nan, 6.0, -3.0), 8.0
    lt[4]["shadowType"], lt[4]["pcfSamples"] = L.SHADOW_PCF, 4
    return lt


def cloud_lights_for(n):
    """scenes.lit_cloud's lights for a cloud of n spheres."""
    return scenes.cloud_lights(4.0 * max(n, 1) ** (1.0 / 3.0))
