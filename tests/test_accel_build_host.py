"""CPU-only tests of the device builder's structure as accel_build_oracle restates it (rt_set_accel_builder):
the restatement is a structure the walks may use -- it passes rt_accel_validate_host and accel_oracle.check_structure -- its loose
list is the host builder's, a walk over it answers what brute force answers on every field, the degenerate inputs (coincident
centres, tiny trees, duplicates) give valid trees, and the new ABI: the struct's layout and rt_set_accel_builder's refusals."""
import ctypes

import numpy as np
import pytest

import accel_build_oracle as B
import accel_oracle as A
from conftest import bits_equal
from opengl_raytracing_amd import layout as L
from opengl_raytracing_amd import scenes
from test_query import restate

LEAVES = [1, 4, 8]


def _config(host, cfg):
    return scenes.make_scene(cfg, host.generate_aabb).objects


SCENES = {
    "c2": lambda host: _config(host, 2),
    "c4": lambda host: _config(host, 4),
    "c5": lambda host: _config(host, 5),
    "cloud1024": lambda host: A.cloud_scene(host, 1024, seed=1),
    "cloud4096": lambda host: A.cloud_scene(host, 4096, seed=2),
    "spheres65536": lambda host: A.cloud_scene(host, 65536, seed=3, floor=False),
    "hostile": lambda host: A.hostile_scene(host),
}


def spheres(n, seed, same_axes=()):
    """n unit-box spheres at seeded positions; on `same_axes` every centre is the first one's."""
    rng = np.random.default_rng(seed)
    objs = L.default_objects(n)
    objs["type"] = L.SPHERE
    pos = np.round(rng.uniform(-8, 8, (n, 3)) * 8) / 8
    for a in same_axes:
        pos[:, a] = pos[0, a]
    objs["position"], objs["radius"] = pos, 0.5
    objs["bounds_min"], objs["bounds_max"] = pos - 0.5, pos + 0.5
    return objs


def check(host, objs, leaf, large_fraction=0.0):
    acc = B.build(objs, leaf, large_fraction)
    assert host.accel_validate_host(objs, acc.nodes, acc.order, acc.loose, leaf)
    A.check_structure(objs, acc, leaf)
    ref = host.accel_build_host(objs, leaf_size=leaf, large_fraction=large_fraction)
    assert (acc.loose == ref.loose).all() and len(acc.loose) == len(ref.loose), "the loose list is the host builder's"
    assert sorted(acc.order.tolist()) == sorted(ref.order.tolist())
    if len(acc.order):
        assert acc.info["leaves"] == -(-len(acc.order) // leaf) and len(acc.nodes) == 2 * acc.info["leaves"] - 1
    return acc


@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("name", list(SCENES))
def test_the_restatement_is_a_valid_structure(host, name, leaf):
    objs = SCENES[name](host)
    acc = check(host, objs, leaf)
    assert len(acc.nodes) > 0
    again = B.build(objs.copy(), leaf)
    assert B.same_structure(again, acc) is None and again.nodes.tobytes() == acc.nodes.tobytes()


@pytest.mark.parametrize("leaf", [1, 4])
def test_a_walk_over_it_answers_what_brute_force_answers(host, leaf):
    objs = A.hostile_scene(host)
    acc = check(host, objs, leaf)
    rays = A.hostile_rays(objs, acc, 6000, seed=77)
    assert A.superset_violations(objs, acc, rays) == 0
    want = restate(objs, rays)
    for group in (1, 64):
        got = A.traverse(objs, acc, rays, group=group)
        assert (got[3] == want[3]).all(), f"group {group}: object differs on {int((got[3] != want[3]).sum())} rays"
        for name, g, w in zip(("position", "t", "normal"), got[:3], want[:3]):
            assert bits_equal(g, w), f"group {group}: {name}"
    assert (want[3] >= 0).sum() > 500 and (want[3] < 0).sum() > 500


@pytest.mark.parametrize("leaf", LEAVES)
def test_coincident_centres(host, leaf):
    """Every centre identical: all codes are 0 and the radix tree is over the index bits alone.  Equal on two axes: a code of ten
    significant bits, most of them shared."""
    for n in (2, 37, 300):
        objs = spheres(n, seed=n, same_axes=(0, 1, 2))
        acc = check(host, objs, leaf, large_fraction=1.0)
        assert len(acc.loose) == 0
        lo, hi, tree, _ = B.classify(objs, 1.0)
        assert (B.morton_codes(lo, hi, tree) == 0).all()
        assert (acc.order == np.arange(n)).all(), "sorted by index alone"
        objs = spheres(n, seed=n, same_axes=(1, 2))
        check(host, objs, leaf, large_fraction=1.0)
        code = B.morton_codes(*B.classify(objs, 1.0)[:3])
        assert (code & 0o3333333333).max() == 0 and code.max() > 0, "only x bits"


@pytest.mark.parametrize("leaf", LEAVES)
def test_tiny_trees_and_duplicates(host, leaf):
    for n in sorted({1, 2, leaf, leaf + 1}):
        objs = spheres(n, seed=10 + n)
        acc = check(host, objs, leaf, large_fraction=1.0)
        assert len(acc.order) == n and len(acc.nodes) == 2 * -(-n // leaf) - 1
        if n <= 2 * leaf:
            assert acc.info["depth"] == (1 if n <= leaf else 2)
    # duplicate shapes, boxes and all: equal codes, told apart by the index
    objs = spheres(40, seed=3)
    objs[1::2] = objs[0::2]
    acc = check(host, objs, leaf, large_fraction=1.0)
    rays = A.hostile_rays(objs, acc, 1500, seed=4)
    want, got = restate(objs, rays), A.traverse(objs, acc, rays)
    assert (got[3] == want[3]).all() and bits_equal(got[1], want[1])
    assert (want[3] >= 0).sum() > 30 and (want[3][want[3] >= 0] % 2 == 0).all(), "the lower index of a pair wins"


def test_morton_codes_and_the_sort_order(host):
    """Item 2 of the structure on a case small enough to state by hand: centres on the grid's corners."""
    objs = spheres(8, seed=0)
    pos = np.array([[x, y, z] for x in (0.0, 4.0) for y in (0.0, 4.0) for z in (0.0, 4.0)])
    objs["position"], objs["bounds_min"], objs["bounds_max"] = pos, pos - 0.5, pos + 0.5
    lo, hi, tree, loose = B.classify(objs, 1.0)
    code = B.morton_codes(lo, hi, tree)
    top = lambda x, y, z: sum(((1023 * b) >> k & 1) << (3 * k + s) for k in range(10) for b, s in ((x, 2), (y, 1), (z, 0)))
    assert code.tolist() == [top(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)]
    acc = B.build(objs[::-1].copy(), 1, 1.0)                      # the same objects in reverse index order
    assert acc.order.tolist() == list(range(7, -1, -1)), "x is the most significant axis, then y, then z"
    assert acc.nodes["skip"].tolist() == [15, 8, 5, 4, 5, 8, 7, 8, 15, 12, 11, 12, 15, 14, 15]


def test_the_new_structs_and_constants(host):
    r = L.RtAccelBuildReport
    assert ctypes.sizeof(r) == 64
    want = dict(builder=0, reserved0=4, buildsHost=8, buildsDevice=16, hostMs=24, deviceMs=32, reserved=40)
    assert {name: getattr(r, name).offset for name, _ in r._fields_} == want
    assert (L.ACCEL_BUILD_HOST, L.ACCEL_BUILD_DEVICE) == (0, 1) and L.ACCEL_BUILDERS == {"host": 0, "device": 1}
    for name in ("rt_set_accel_builder", "rt_accel_build_info", "rt_accel_read"):
        assert name in host.EXPORTS and getattr(host.load_library(), name)
    for method in ("set_accel_builder", "accel_build_info", "accel_read"):
        assert callable(getattr(host.RayTracer, method))


def test_refusals_without_a_context(host):
    """A NULL context is refused before anything is touched: no GPU is needed to see it."""
    lib = host.load_library()
    info, report = L.RtAccelBuildReport(), L.RtAccelReport()
    for builder in (0, 1, 2, -1):
        assert lib.rt_set_accel_builder(None, builder) == -1
    assert lib.rt_accel_build_info(None, ctypes.byref(info)) == -1
    assert lib.rt_accel_read(None, None, 0, None, 0, None, 0, ctypes.byref(report)) == -1
