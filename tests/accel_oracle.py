"""numpy float32 restatement of the threaded traversal behind rt_set_accel (csrc/rt_accel.inc), over the arrays
host.accel_build_host returns: the node test with its NaN rule, the leaves, then the loose list.  An object that is reached is
judged by test_query.restate's own arithmetic (restate on that one object), so what this file adds is only what the feature
adds: which objects a ray reaches, and the tie rule among equal t.  Also here: the structure's invariants re-checked
independently of rt_accel_validate, the hostile scene and rays the host and the GPU tests share, and the seeded sphere clouds."""
import numpy as np

from opengl_raytracing_amd import layout as L
from opengl_raytracing_amd import scenes
from test_query import random_rays, restate

F = np.float32
INNER = L.ACCEL_INNER


# ---- scenes ----------------------------------------------------------------------------------------------------------
def cloud_scene(host, n, seed, floor=True):
    """scenes.sphere_cloud's objects: n seeded spheres at constant density, plus a floor plane under them."""
    return scenes.sphere_cloud(n, seed, host.generate_aabb, floor)[0]


def hostile_scene(host):
    """The constructed scene of the issue: honest spheres and small flat planes spread over several leaves, plus inverted
    boxes, NaN and infinite bounds, boxes that do not contain their shape, duplicate shapes under different boxes (so that they
    land in different leaves, in both orders of index against traversal), zero radius, unknown types, a floor."""
    rng = np.random.default_rng(20240)
    n = 96
    objs = L.default_objects(n)
    objs["type"] = L.SPHERE
    objs["position"] = np.round(rng.uniform(-10, 10, (n, 3)) * 4) / 4            # quarter-unit grid: many exactly equal coordinates
    objs["radius"] = rng.choice([0.25, 0.5, 0.75, 1.0], n)
    flat = np.arange(0, 24)                                                      # small planes: flat boxes on y, x or z
    objs["type"][flat] = L.PLANE
    objs["normal"][flat] = np.array([(0, 1, 0), (1, 0, 0), (0, 0, 1)], F)[flat % 3]
    objs["size"][flat] = rng.choice([1.0, 2.0, 3.0], (len(flat), 2))
    objs["radius"][24:27] = 0.0                                                  # zero radius
    objs["type"][27:31] = (2, 7, -1, 1 << 30)                                    # unknown types: shape_test rejects them
    objs[64]["type"] = L.PLANE                                                   # a floor: a "large" box
    objs[64]["position"] = (0, -11, 0)
    objs[64]["normal"] = (0, 1, 0)
    objs[64]["size"] = (60, 60)
    host.generate_aabb(objs)
    # duplicates: the same sphere at i < j, the second under a box stretched to one side (still around the sphere), so its centre
    # -- and its leaf -- differ.  Pairs (40, 41): the stretched copy has the higher index; (43, 42): the lower.
    objs[41] = objs[40]
    objs["bounds_min"][41][0] -= 18.0
    objs[42] = objs[43]
    objs["bounds_max"][42][0] += 18.0
    for keep, stretch in ((44, 45), (47, 46)):
        objs[stretch] = objs[keep]
        objs["bounds_min"][stretch][2] -= 18.0
    # exact duplicates, box and all (the same leaf or neighbouring ones)
    objs[49] = objs[48]
    # boxes that do not contain their shape: the box lies off to one side, so the hit comes before the box entry
    for i, shift in ((50, (3.0, 0, 0)), (51, (0, -2.5, 0)), (52, (0, 0, 4.0)), (53, (-1.5, 1.5, 0))):
        objs["bounds_min"][i] += np.array(shift, F)
        objs["bounds_max"][i] += np.array(shift, F)
        objs["radius"][i] = 1.5
    # inverted boxes: on one axis, on all
    for i, axes in ((54, (0,)), (55, (1,)), (56, (2,)), (57, (0, 1, 2)), (5, (1,)), (6, (0, 2))):
        for a in axes:
            lo, hi = objs["bounds_min"][i][a], objs["bounds_max"][i][a]
            objs["bounds_min"][i][a], objs["bounds_max"][i][a] = hi, lo
    # NaN and infinite bounds: these cannot be in the tree
    objs["bounds_min"][58][0] = np.nan
    objs["bounds_max"][59][1] = np.nan
    objs["bounds_min"][60] = np.nan
    objs["bounds_max"][61][2] = np.inf
    objs["bounds_min"][62][0] = -np.inf
    objs["bounds_min"][63], objs["bounds_max"][63] = -np.inf, np.inf
    objs["bounds_min"][7][1] = np.nan                                            # a plane's, too
    return objs


def face_rays(objects, acc, n, seed):
    """Rays whose origin coordinates are box faces -- the objects' stored bounds and the nodes' -- with axis-aligned directions or
    directions with exact zero components: the products (b - o) * inv that are 0 * inf."""
    rng = np.random.default_rng(seed)
    faces = [np.concatenate([objects["bounds_min"][:, a], objects["bounds_max"][:, a], acc.nodes["lo"][:, a], acc.nodes["hi"][:, a]]).astype(F)
             for a in range(3)]
    faces = [f[np.isfinite(f)] for f in faces]
    r = np.zeros(n, dtype=L.RAY_DTYPE)
    o = np.stack([rng.choice(f, n) if len(f) else np.zeros(n, F) for f in faces], axis=-1).astype(F)
    off = rng.random((n, 3)) < 0.35                                              # some coordinates off the faces
    o[off] = (o + rng.uniform(-1.5, 1.5, (n, 3)).astype(F))[off]
    d = rng.normal(size=(n, 3)).astype(F)
    kind = rng.integers(0, 4, n)
    ax = rng.integers(0, 3, n)
    rows = np.arange(n)
    sel = kind <= 1                                                              # axis-aligned
    d[sel] = 0.0
    d[rows[sel], ax[sel]] = rng.choice([-1.0, 1.0, 2.5, -0.0], int(sel.sum()))
    sel = kind == 2                                                              # one exact zero (of either sign)
    d[rows[sel], ax[sel]] = rng.choice([0.0, -0.0], int(sel.sum()))
    sel = kind == 3                                                              # two
    d[rows[sel], ax[sel]] = 0.0
    d[rows[sel], (ax[sel] + 1) % 3] = -0.0
    tk = rng.integers(0, 6, n)
    tmax = np.full(n, 114514.0, F)
    tmax[tk == 1] = np.inf
    tmax[tk == 2] = rng.uniform(0, 12, int((tk == 2).sum()))
    r["origin"], r["direction"], r["tMax"] = o, d, tmax
    return r


def hostile_rays(objects, acc, n, seed):
    """test_query's hostile generator plus the face rays, n in all."""
    k = n // 2
    out = np.zeros(n, dtype=L.RAY_DTYPE)
    out[:k] = random_rays(objects, k, seed)
    out[k:] = face_rays(objects, acc, n - k, seed + 1)
    return out


# ---- the structure's invariants, independently of rt_accel_validate --------------------------------------------------
def norm_boxes(objects):
    """(lo[n,3], hi[n,3], finite[n]): the stored boxes as the node boxes see them."""
    a, b = objects["bounds_min"].astype(F), objects["bounds_max"].astype(F)
    with np.errstate(invalid="ignore"):
        return np.minimum(a, b), np.maximum(a, b), np.isfinite(a).all(-1) & np.isfinite(b).all(-1)


def parents(nodes):
    """parent[k] of every node (-1 for the root), from pre-order and the skip links alone."""
    par = np.full(len(nodes), -1, np.int64)
    stack = []                                     # (node, end of its subtree)
    for k in range(len(nodes)):
        while stack and stack[-1][1] <= k:
            stack.pop()
        if stack:
            par[k] = stack[-1][0]
        if nodes["leaf"][k] == INNER:
            stack.append((k, int(nodes["skip"][k])))
    return par


def check_structure(objects, acc, leaf_size):
    nodes, order, loose = acc.nodes, acc.order, acc.loose
    n, nn = len(objects), len(nodes)
    lo, hi, finite = norm_boxes(objects)
    both = np.concatenate([order, loose]).astype(np.int64)
    assert len(both) == n and (both < n).all() and len(np.unique(both)) == n, "order[] and loose[] are not a permutation of the objects"
    assert (np.diff(loose.astype(np.int64)) > 0).all(), "loose[] is not ascending"
    assert finite[order].all(), "an object without a finite box is in the tree"
    assert (nn == 0) == (len(order) == 0)
    if nn == 0:
        return
    skip, leaf = nodes["skip"].astype(np.int64), nodes["leaf"]
    assert skip[0] == nn and (skip > np.arange(nn)).all() and (skip <= nn).all(), "skip links must point strictly forward"
    assert np.isfinite(nodes["lo"]).all() and np.isfinite(nodes["hi"]).all()
    par = parents(nodes)
    slot = depth = 0
    level = np.zeros(nn, np.int64)
    for k in range(nn):
        level[k] = level[par[k]] + 1 if par[k] >= 0 else 1
        if par[k] >= 0:
            assert skip[k] <= skip[par[k]], "a subtree that leaves its parent's"
        if leaf[k] == INNER:
            c1, c2 = k + 1, skip[k + 1]
            assert c1 < c2 < skip[k] and skip[c2] == skip[k], f"node {k}: its two children do not tile its subtree"
            assert par[c1] == k and par[c2] == k
            want_lo, want_hi = np.minimum(nodes["lo"][c1], nodes["lo"][c2]), np.maximum(nodes["hi"][c1], nodes["hi"][c2])
        else:
            first, count = int(leaf[k]) >> 4, int(leaf[k]) & 15
            assert skip[k] == k + 1 and 1 <= count <= leaf_size and first == slot, f"leaf {k}"
            slot += count
            ids = order[first:first + count]
            want_lo, want_hi = lo[ids].min(0), hi[ids].max(0)
        assert (nodes["lo"][k] == want_lo).all() and (nodes["hi"][k] == want_hi).all(), f"node {k}: box is not the union of its children"
    assert slot == len(order), "order[] entries that no leaf addresses"
    info = acc.info
    assert info["nodes"] == nn and info["leaves"] == int((leaf != INNER).sum()) and info["loose"] == len(loose)
    assert info["depth"] == level.max() and info["bytes"] == 32 * nn + 4 * n


# ---- the two box tests -----------------------------------------------------------------------------------------------
def _products(lo, hi, o, inv):
    return (lo - o) * inv, (hi - o) * inv


def aabb_pass(lo, hi, o, inv, tmax):
    """intersectAABB as restate states it (fmin / fmax drop a NaN operand)."""
    with np.errstate(all="ignore"):
        t0, t1 = _products(lo, hi, o, inv)
        ts, tl = np.fmin(t0, t1), np.fmax(t0, t1)
        tMin = np.fmax(np.fmax(ts[:, 0], ts[:, 1]), ts[:, 2])
        tMaxB = np.fmin(np.fmin(tl[:, 0], tl[:, 1]), tl[:, 2])
        return (tMaxB >= tMin) & (tMin < tmax) & (tMaxB > F(0.0))


def node_pass(lo, hi, o, inv, tmax):
    """The node test: an axis on which either product is NaN does not constrain."""
    with np.errstate(all="ignore"):
        t0, t1 = _products(lo, hi, o, inv)
        un = np.isnan(t0) | np.isnan(t1)
        ts = np.where(un, F(-np.inf), np.fmin(t0, t1))
        tl = np.where(un, F(np.inf), np.fmax(t0, t1))
        tMin = np.fmax(np.fmax(ts[:, 0], ts[:, 1]), ts[:, 2])
        tMaxB = np.fmin(np.fmin(tl[:, 0], tl[:, 1]), tl[:, 2])
        return (tMaxB >= tMin) & (tMin < tmax) & (tMaxB > F(0.0))


def _ray_parts(rays):
    r = np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8)
    o, tmax, d = r[:, 0:3].copy(), r[:, 3].copy(), r[:, 4:7].copy()
    with np.errstate(all="ignore"):
        inv = F(1.0) / d
    return o, tmax, d, inv


def superset_violations(objects, acc, rays):
    """How many (ray, object) pairs pass the object's own stored-box test while some ancestor's node test fails."""
    o, tmax, _, inv = _ray_parts(rays)
    nodes = acc.nodes
    par = parents(nodes)
    chain = np.zeros((len(nodes), len(o)), bool)               # this node and all its ancestors pass
    for k in range(len(nodes)):
        p = node_pass(nodes["lo"][k], nodes["hi"][k], o, inv, tmax)
        chain[k] = p & chain[par[k]] if par[k] >= 0 else p
    bad = 0
    bmin, bmax = objects["bounds_min"].astype(F), objects["bounds_max"].astype(F)
    for k in np.flatnonzero(nodes["leaf"] != INNER):
        first, count = int(nodes["leaf"][k]) >> 4, int(nodes["leaf"][k]) & 15
        for i in acc.order[first:first + count]:
            bad += int((aabb_pass(bmin[i], bmax[i], o, inv, tmax) & ~chain[k]).sum())
    return bad


# ---- the traversal ---------------------------------------------------------------------------------------------------
def traverse(objects, acc, rays, group=1):
    """-> restate()'s tuple (position, t, normal, object), by the threaded walk.  group = 1: one walk per ray (LANE); 64: one per
    64 consecutive rays, every ray of the group meeting whatever some ray of it reaches (WAVE)."""
    o, tmax, _, inv = _ray_parts(rays)
    n = len(o)
    nodes = acc.nodes
    minT, hit = tmax.copy(), np.full(n, -1, np.int32)
    position, normal = np.zeros((n, 3), F), np.zeros((n, 3), F)

    def spread(mask):                                            # what some ray of a group does, the whole group does
        if group == 1:
            return mask
        pad = (-n) % group
        g = np.concatenate([mask, np.zeros(pad, bool)]).reshape(-1, group).any(1)
        return np.repeat(g, group)[:n]

    def meet(i, who):                                            # the rays `who` test object i
        nonlocal minT, hit
        idx = np.flatnonzero(who)
        if len(idx) == 0:
            return
        pos, t, nrm, h = restate(objects[i:i + 1], rays[idx])    # counts on its own: box test against tMax, 0 < t < tMax
        with np.errstate(invalid="ignore"):
            take = (h == 0) & ((t < minT[idx]) | ((t == minT[idx]) & (i < hit[idx])))
        sel = idx[take]
        minT[sel], hit[sel], position[sel], normal[sel] = t[take], i, pos[take], nrm[take]

    par = parents(nodes)
    reach = np.zeros((len(nodes), n), bool)
    for k in range(len(nodes)):
        reach[k] = reach[par[k]] if par[k] >= 0 else True
        if not reach[k].any():
            continue
        reach[k] &= spread(node_pass(nodes["lo"][k], nodes["hi"][k], o, inv, tmax) & reach[k])
        if nodes["leaf"][k] != INNER:
            first, count = int(nodes["leaf"][k]) >> 4, int(nodes["leaf"][k]) & 15
            for i in acc.order[first:first + count]:
                meet(int(i), reach[k])
    for i in acc.loose:
        meet(int(i), np.ones(n, bool))
    return position, minT, normal, hit
