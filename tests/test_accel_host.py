"""CPU-only tests of the hierarchy behind rt_set_accel (rt_accel_build_host; csrc/rt_accel.cpp): the structure's invariants
re-checked in numpy, determinism, the superset property on hostile scenes and rays -- every ray that passes an object's own
stored-box test passes the node test of every ancestor -- the traversal restated in numpy against test_query.restate on every
field, the loose list's size on sphere clouds, and the refusals."""
import ctypes

import numpy as np
import pytest

import accel_oracle as A
from conftest import bits_equal
from opengl_raytracing_amd import layout as L
from opengl_raytracing_amd import scenes
from test_query import random_rays, restate


def _config(host, cfg):
    return scenes.make_scene(cfg, host.generate_aabb).objects


SCENES = {
    "c2": lambda host: _config(host, 2),
    "c4": lambda host: _config(host, 4),
    "c5": lambda host: _config(host, 5),
    "cloud1024": lambda host: A.cloud_scene(host, 1024, seed=1),
    "cloud4096": lambda host: A.cloud_scene(host, 4096, seed=2),
    "spheres65536": lambda host: A.cloud_scene(host, 65536, seed=3, floor=False),
    "empty": lambda host: L.default_objects(0),
    "one": lambda host: A.cloud_scene(host, 1, seed=4, floor=False),
    "all_loose": lambda host: _all_loose(host),
    "hostile": lambda host: A.hostile_scene(host),
}


def _all_loose(host):
    objs = A.cloud_scene(host, 12, seed=5)
    objs["bounds_min"][:, 0] = np.nan
    return objs


@pytest.mark.parametrize("leaf", [1, 4, 8])
@pytest.mark.parametrize("name", list(SCENES))
def test_structure_invariants_and_determinism(host, name, leaf):
    objs = SCENES[name](host)
    acc = host.accel_build_host(objs, leaf_size=leaf)
    A.check_structure(objs, acc, leaf)
    again = host.accel_build_host(objs.copy(), leaf_size=leaf)
    assert acc.nodes.tobytes() == again.nodes.tobytes() and acc.order.tobytes() == again.order.tobytes()
    assert acc.loose.tobytes() == again.loose.tobytes()
    if name in ("empty", "one", "all_loose"):
        assert len(acc.nodes) == 0 and len(acc.loose) == len(objs)
    else:
        assert len(acc.nodes) > 0 and acc.info["leaves"] >= -(-len(acc.order) // leaf)
        assert acc.info["depth"] <= 2 + int(np.ceil(np.log2(len(acc.order))))      # median splits: a balanced tree


def test_default_leaf_size_is_four(host):
    objs = A.cloud_scene(host, 300, seed=6)
    assert host.accel_build_host(objs).nodes.tobytes() == host.accel_build_host(objs, leaf_size=4).nodes.tobytes()
    A.check_structure(objs, host.accel_build_host(objs), 4)


@pytest.mark.parametrize("n", [1024, 2048, 4096])
def test_clouds_keep_nearly_everything_in_the_tree(host, n):
    """A build that dumped the objects on the loose list would leave every other test vacuous."""
    objs = A.cloud_scene(host, n, seed=n)
    acc = host.accel_build_host(objs)
    assert len(acc.loose) <= 1 + len(objs) // 256
    assert n in acc.loose, "the floor is a large box: loose"


def test_what_goes_on_the_loose_list(host):
    objs = A.hostile_scene(host)
    acc = host.accel_build_host(objs)
    loose = set(acc.loose.tolist())
    assert {58, 59, 60, 61, 62, 63, 7} <= loose, "NaN and infinite bounds cannot be bounded by a union"
    assert 64 in loose, "the floor"
    assert not ({54, 55, 56, 57, 50, 51, 52, 53} & loose), "inverted and dishonest boxes are finite boxes: in the tree"
    for cfg in (2, 4, 5):
        objs = _config(host, cfg)
        acc = host.accel_build_host(objs)
        assert set(acc.loose.tolist()) == {len(objs) - 2, len(objs) - 1}, "the two planes of a shipped scene"
    # largeFraction is the knob: at 1 nothing finite is large
    objs = _config(host, 2)
    assert len(host.accel_build_host(objs, large_fraction=1.0).loose) == 0


def _leaf_of(acc):
    """object index -> node index of its leaf"""
    out = {}
    for k in np.flatnonzero(acc.nodes["leaf"] != A.INNER):
        first, count = int(acc.nodes["leaf"][k]) >> 4, int(acc.nodes["leaf"][k]) & 15
        for i in acc.order[first:first + count]:
            out[int(i)] = int(k)
    return out


@pytest.mark.parametrize("leaf", [1, 4])
def test_superset_property_and_traversal_on_the_hostile_scene(host, leaf):
    objs = A.hostile_scene(host)
    acc = host.accel_build_host(objs, leaf_size=leaf)
    A.check_structure(objs, acc, leaf)
    where = _leaf_of(acc)
    for a, b in ((40, 41), (42, 43), (44, 45), (46, 47)):
        assert where[a] != where[b], "the duplicate shapes were meant to land in different leaves"
    pre = {int(i): k for k, i in enumerate(acc.order)}
    assert {pre[a] < pre[b] for a, b in ((40, 41), (42, 43), (44, 45), (46, 47))} == {True, False}, "the lower index is met first, and second"
    rays = A.hostile_rays(objs, acc, 6000, seed=77)
    assert A.superset_violations(objs, acc, rays) == 0
    want = restate(objs, rays)
    for group in (1, 64):
        got = A.traverse(objs, acc, rays, group=group)
        assert (got[3] == want[3]).all(), f"group {group}: object differs on {int((got[3] != want[3]).sum())} rays"
        for name, g, w in zip(("position", "t", "normal"), got[:3], want[:3]):
            assert bits_equal(g, w), f"group {group}: {name}"
    # the cases are really in there: rays that hit a duplicated shape (the lower index wins wherever both boxes pass; the higher
    # one only where the lower one's own box test fails), hits in front of the box entry
    hit = want[3]
    assert min(int((hit == i).sum()) for i in (40, 42, 44, 46, 48)) > 0
    o, tmax, _, inv = A._ray_parts(rays)
    for i in (40, 42, 44, 46, 48):
        lower_box_passes = A.aabb_pass(objs["bounds_min"][i], objs["bounds_max"][i], o, inv, tmax)
        assert not (lower_box_passes & (hit == i + 1)).any()
    assert np.isin(hit, (50, 51, 52, 53)).sum() > 0
    assert (hit == 64).sum() > 0 and (hit == -1).sum() > 0


@pytest.mark.parametrize("name", ["c2", "c5", "cloud1024"])
def test_superset_property_and_traversal_on_scenes(host, name):
    objs = SCENES[name](host)
    acc = host.accel_build_host(objs)
    rays = A.hostile_rays(objs, acc, 3000, seed=5)
    assert A.superset_violations(objs, acc, rays) == 0
    want = restate(objs, rays)
    got = A.traverse(objs, acc, rays, group=1)
    assert (got[3] == want[3]).all()
    for g, w in zip(got[:3], want[:3]):
        assert bits_equal(g, w)
    assert (want[3] >= 0).sum() > 100


def test_the_nan_rule_is_needed(host):
    """The constructed case of the design: a flat box, a ray origin exactly on it, a zero direction component.  The object's axis
    is ignored (NaN, NaN) and the object can pass; an enclosing box whose own face coincides with the origin gives (NaN, inf),
    which plain fmin / fmax turn into the slab [inf, inf].  The node test must not fail there."""
    F = np.float32
    o = np.array([[0.0, 1.0, -5.0]], F)
    d = np.array([[0.0, 0.0, 1.0]], F)
    with np.errstate(all="ignore"):
        inv = F(1.0) / d
    tmax = np.array([100.0], F)
    flat_lo, flat_hi = np.array([-1, 1, -1], F), np.array([1, 1, 1], F)          # flat on y, at the origin's y
    par_lo, par_hi = np.array([-1, 1, -1], F), np.array([1, 3, 1], F)            # a parent whose lower face coincides with it
    assert A.aabb_pass(flat_lo, flat_hi, o, inv, tmax)[0], "the object passes"
    assert not A.aabb_pass(par_lo, par_hi, o, inv, tmax)[0], "plain fmin / fmax would cull its parent"
    assert A.node_pass(par_lo, par_hi, o, inv, tmax)[0], "the node test does not"


def test_the_check_refuses_every_broken_invariant(host):
    """rt_accel_validate stands between the builder and the device: a structure it refuses is never uploaded.  Every invariant,
    broken one at a time on a good structure, is refused -- and random words in any field are refused or harmless."""
    objs = A.cloud_scene(host, 200, seed=11)
    acc = host.accel_build_host(objs, leaf_size=4)
    ok = lambda nodes=acc.nodes, order=acc.order, loose=acc.loose, leaf=4, o=objs: host.accel_validate_host(o, nodes, order, loose, leaf)
    assert ok()
    inner = int(np.flatnonzero(acc.nodes["leaf"] == A.INNER)[3])
    leaf = int(np.flatnonzero(acc.nodes["leaf"] != A.INNER)[5])
    count = int(acc.nodes["leaf"][leaf]) & 15

    def broken(k, field, value):
        n = acc.nodes.copy()
        n[field][k] = value
        return n

    assert not ok(broken(inner, "skip", inner)), "a skip link onto itself: the hang the check is there to prevent"
    assert not ok(broken(inner, "skip", inner - 1)), "a skip link backwards"
    assert not ok(broken(inner, "skip", int(acc.nodes["skip"][inner]) + 1)), "a subtree that ends behind its own end"
    assert not ok(broken(0, "skip", len(acc.nodes) + 1)), "a root that ends behind the array"
    assert not ok(broken(leaf, "skip", leaf + 2)), "a leaf with a subtree"
    for wrong in (0, count - 1, count + 1, 9, 15):
        assert not ok(broken(leaf, "leaf", (int(acc.nodes["leaf"][leaf]) & ~15) | wrong)), f"leaf count {count} -> {wrong}"
    assert not ok(broken(leaf, "leaf", (1 << 27) | 4)), "a leaf that addresses beyond order[]"
    assert not ok(broken(leaf, "leaf", A.INNER)), "a leaf turned inner"
    assert not ok(broken(inner, "leaf", 4)), "an inner node turned leaf"
    assert (acc.nodes["leaf"][acc.nodes["leaf"] != A.INNER] & 15).max() == 4
    assert not ok(leaf=3) and ok(leaf=8), "leaves of four objects under leafSize 3"
    assert not ok(leaf=0) and not ok(leaf=9)
    for field in ("lo", "hi"):
        for value in (np.nan, np.inf, acc.nodes[field][inner][0] + np.float32(0.5)):
            n = acc.nodes.copy()
            n[field][inner][0] = value
            assert not ok(n), f"node {field} = {value}: not the finite union of its children"
    order = acc.order.copy()
    order[7] = len(objs)
    assert not ok(order=order), "an object index == nObj"
    order = acc.order.copy()
    order[7] = order[8]
    assert not ok(order=order), "an object twice, another never"
    assert not ok(loose=np.array([int(acc.order[0])], np.uint32)), "an object in the tree and on the loose list"
    assert not ok(order=acc.order[:-1]), "an object nowhere"
    assert not ok(nodes=acc.nodes[:-1]) and not ok(nodes=acc.nodes[:0])
    nan_box = objs.copy()
    nan_box["bounds_min"][int(acc.order[3])][1] = np.nan
    assert not ok(o=nan_box), "an object without a finite box in the tree"
    rng = np.random.default_rng(12)
    for trial in range(300):
        n, o = acc.nodes.copy(), acc.order.copy()
        words = n.view(np.uint32).reshape(-1, 8)
        if trial % 3 == 2:
            o[rng.integers(len(o))] = rng.integers(0, 2 ** 32, dtype=np.uint64)
        else:
            words[rng.integers(len(n)), (3, 7)[trial % 3]] = rng.integers(0, 2 ** 32, dtype=np.uint64)
        same = n.tobytes() == acc.nodes.tobytes() and o.tobytes() == acc.order.tobytes()
        assert ok(n, o) == same


def test_refusals(host):
    lib = host.load_library()
    objs = A.cloud_scene(host, 64, seed=9)
    info = L.RtAccelReport()
    op = objs.ctypes.data_as(ctypes.c_void_p)

    def build(desc, nodes=None, cap_nodes=0, order=None, cap_order=0, loose=None, cap_loose=0, n=len(objs)):
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
        return lib.rt_accel_build_host(op, n, ctypes.byref(desc) if desc is not None else None, p(nodes), cap_nodes, p(order), cap_order,
                                       p(loose), cap_loose, ctypes.byref(info))

    assert build(None) == 0 and info.nodes > 0 and info.loose == 1, "NULL desc: the defaults"
    nn, nl = info.nodes, info.loose
    bad = L.make_accel_desc()
    bad.traversal = 3
    assert build(bad) == -1
    bad.traversal = -1
    assert build(bad) == -1
    for k in range(3):
        bad = L.make_accel_desc()
        bad.reserved[k] = 1
        assert build(bad) == -1
    for leaf in (-1, 9, 16):
        assert build(L.make_accel_desc(leaf_size=leaf)) == -1
    assert build(L.make_accel_desc(min_objects=-1)) == -1
    for frac in (-0.5, float("nan"), float("inf")):
        assert build(L.make_accel_desc(large_fraction=frac)) == -1
    nodes, order, loose = np.zeros(nn, L.ACCEL_NODE_DTYPE), np.zeros(len(objs) - nl, np.uint32), np.zeros(nl, np.uint32)
    d = L.make_accel_desc()
    assert build(d, nodes, nn, order, len(order), loose, nl) == 0
    assert build(d, nodes, nn - 1, order, len(order), loose, nl) == -4
    assert build(d, nodes, nn, order, len(order) - 1, loose, nl) == -4
    assert build(d, nodes, nn, order, len(order), loose, nl - 1) == -4
    assert build(d, n=-1) == -1 and build(d, n=65537) == -4
    assert lib.rt_accel_build_host(None, 4, ctypes.byref(d), None, 0, None, 0, None, 0, ctypes.byref(info)) == -1
    assert lib.rt_accel_build_host(op, 4, ctypes.byref(d), None, 0, None, 0, None, 0, None) == -1
    # enable and minObjects are the context's business: the host build does not look at them
    off = L.make_accel_desc(enable=False, min_objects=10 ** 6)
    assert build(off) == 0 and info.nodes == nn
