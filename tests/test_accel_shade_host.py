"""CPU-only tests of rt_set_accel_shading's parts that need no GPU: the two-distance any-hit of rt_shade_rays' shadow and blocker
rays restated in numpy (accel_shade_oracle.py) -- the threaded walk, per ray and per group of 64, against the brute-force rule on
the hostile scene -- the new structs' sizes and offsets, make_accel_shade_desc, lit_cloud, and the refusals that need no context."""
import ctypes

import numpy as np
import pytest

import accel_oracle as A
import accel_shade_oracle as S
from opengl_raytracing_amd import layout as L
from opengl_raytracing_amd import scenes


@pytest.mark.parametrize("leaf", [1, 4, 8])
def test_the_walk_gives_the_brute_force_answer_on_the_hostile_scene(host, leaf):
    objs = A.hostile_scene(host)
    acc = host.accel_build_host(objs, leaf_size=leaf)
    rays = A.hostile_rays(objs, acc, 6000, seed=77)
    limit, cls = S.draw_limits(rays, seed=leaf)
    want = S.brute_any(objs, rays, limit)
    for name, k in zip(S.LIMIT_CLASSES, range(len(S.LIMIT_CLASSES))):
        occluded, free = int(want[cls == k].sum()), int((~want[cls == k]).sum())
        if name in ("minus_one", "zero"):
            assert occluded == 0, f"limit class {name}: nothing can be accepted"
        else:
            assert occluded >= 1 and free >= 1, f"limit class {name}: {occluded} occluded, {free} unoccluded"
    for group in (1, 64):
        got = S.walk_any(objs, acc, rays, limit, group=group)
        assert (got == want).all(), f"leaf {leaf}, group {group}: {int((got != want).sum())} rays differ"


def test_two_distances_are_not_one(host):
    """The rule the one-distance any-hit walk of the queries would state -- gate and accept at the same distance -- is another one:
    some ray of the batch tells them apart, so the test above would catch a walk that used either distance for both."""
    objs = A.hostile_scene(host)
    acc = host.accel_build_host(objs)
    rays = A.hostile_rays(objs, acc, 6000, seed=77)
    limit, _ = S.draw_limits(rays, seed=4)
    want = S.brute_any(objs, rays, limit)
    at_limit = np.ascontiguousarray(rays).copy()
    at_limit["tMax"] = limit                                     # gate at `limit` too
    assert (S.brute_any(objs, at_limit, limit) != want).any()
    max_dist = np.ascontiguousarray(rays)["tMax"].astype(np.float32)
    assert (S.brute_any(objs, rays, max_dist) != want).any()     # accept at maxDist too


def test_struct_layouts():
    D, R = L.RtAccelShadeDesc, L.RtAccelShadeReport
    assert ctypes.sizeof(D) == 32 and ctypes.sizeof(R) == 48
    assert (D.enable.offset, D.traversal.offset, D.minObjects.offset, D.reserved.offset) == (0, 4, 8, 12)
    assert D.reserved.size == 20 and R.launchesAccel.size == 16 and R.reserved.size == 16
    assert (R.active.offset, R.traversal.offset, R.launchesAccel.offset, R.launchesBrute.offset, R.reserved.offset) == (0, 4, 8, 24, 32)


def test_make_accel_shade_desc():
    d = L.make_accel_shade_desc()
    assert (d.enable, d.traversal, d.minObjects, list(d.reserved)) == (1, L.ACCEL_AUTO, 0, [0] * 5)
    d = L.make_accel_shade_desc(False, "wave", 77)
    assert (d.enable, d.traversal, d.minObjects) == (0, L.ACCEL_WAVE, 77)
    assert L.make_accel_shade_desc(traversal="lane").traversal == L.ACCEL_LANE and L.make_accel_shade_desc(traversal=9).traversal == 9


def test_entry_points_refuse_a_null_context(host):
    lib = host.load_library()
    d, r = L.make_accel_shade_desc(), L.RtAccelShadeReport()
    assert lib.rt_set_accel_shading(None, ctypes.byref(d)) == -1
    assert lib.rt_accel_shading_info(None, ctypes.byref(r)) == -1


def test_lit_cloud(host):
    sc = scenes.lit_cloud(256, 5, host.generate_aabb)
    objs, half = scenes.sphere_cloud(256, 5, host.generate_aabb)
    assert len(sc.objects) == 257
    for f in ("type", "position", "radius", "bounds_min", "bounds_max"):
        assert (sc.objects[f] == objs[f]).all(), f
    sph = sc.objects[:256]
    k = np.arange(256)
    sss = k % 16 == 15
    assert (sph["subsurfaceScatter"][sss] > 0).all() and (sph["subsurfaceScatter"][~sss] == 0).all()
    plain = ~sss
    assert (sph["metallic"][plain & (k % 3 == 0)] == 1).all() and (sph["diffuseStrength"][plain & (k % 3 == 0)] == 0).all()
    assert (sph["transparency"][plain & (k % 3 == 1)] > 0).all() and (sph["diffuseStrength"][plain & (k % 3 == 1)] == 0).all()
    assert (sph["diffuseStrength"][k % 3 == 2] > 0).all()
    lt = sc.lights
    assert list(lt["type"]) == [L.POINT, L.DIRECTIONAL, L.AREA]
    assert list(lt["shadowType"]) == [L.SHADOW_PCF, L.SHADOW_PCF, L.SHADOW_PCSS] and list(lt["pcfSamples"]) == [4, 4, 4]
    assert np.allclose(lt[0]["position"], np.array([0.3, 1.5, 0.4]) * half)
    big = scenes.lit_cloud(2048, 5, host.generate_aabb, floor=False)
    assert len(big.objects) == 2048 and big.lights[0]["position"][1] > lt[0]["position"][1]
