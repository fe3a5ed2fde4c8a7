"""The tile scheduler (csrc/rt_sched.cpp; rt_predict_tiles_kernel, rt_compact_order_kernel, rt_lpt_sort_kernel) held to what it
is for.  No pixel depends on a tile order, so the frame comparisons of the other files only prove that an order is a
permutation.  Here: the longest-first sort against an exact reference on given costs (rt_debug_lpt_sort), the predictor's
classes against a host restatement of its pricing, tile by tile (rt_debug_predicted_classes, sched_oracle.predicted_classes),
and which policy supplies each frame's order -- raster, measured, predicted, per-phase -- read back from the launch itself
(rt_debug_tile_order, RT_DEBUG_TILE_ORDER=1).

Frames: 48 x 32 (24 tiles, one partial predictor wave), test_first_hit_reuse.py's ragged strip-interleaved window (35 tiles)
and 200 x 136 (425 tiles in rows of 25: the predictor's blocks of 64 tile indices end in mid-row; 7 predictor waves, 2
compaction blocks).  First-hit reuse is off (rt_set_variant's bit 10) unless a case is about it."""
import functools

import numpy as np
import pytest

from opengl_raytracing_amd import layout as L
from opengl_raytracing_amd import scenes
from sched_oracle import lpt_bins, predicted_classes
from test_exponent_range import _gen_aabb, _own
from test_first_hit_reuse import base_scene, ragged
from test_prefix_replay import hall_of_mirrors, opaque

pytestmark = pytest.mark.gpu

REUSE_OFF = 0x400
RASTER, MEASURED, PREDICTED, PHASE = 0, 1, 2, 3
SCHED_ENV = ("RT_PRED_MIN_TILES", "RT_DEBUG_PRED_CLASSES", "RT_DEBUG_TILE_ORDER", "RT_FB_PERIOD", "RT_PHASE_ORDER", "RT_VARIANT")
F = np.float32


@pytest.fixture
def make_rt(host, monkeypatch):
    """A context of its own per call: the scheduler reads its environment when the context is created."""
    made = []

    def make(variant=1 | REUSE_OFF, **env):
        for k in SCHED_ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        rt = host.RayTracer(0)
        made.append(rt)
        rt.set_variant(variant)
        return rt
    yield make
    for rt in made:
        rt.close()


def tiles_of(p):
    return -(-p.regionW // 8) * -(-p.regionH // 8)


def is_permutation(order, n):
    return order.shape == (n,) and np.array_equal(np.sort(order), np.arange(n, dtype=order.dtype))


def frame(rt, p):
    """One frame, the device drained behind it -> (order, policy) the launch was given."""
    rt.render(p)
    rt.sync()
    return rt.tile_order()


# ---- the sort, on given costs ---------------------------------------------------------------------------------------------------
def cost_patterns(n, rng):
    full = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    full[0] = 0xFFFFFFFF
    if n > 1:
        full[n // 2] = (1 << 24) + 1
        full[n - 1] = 0
    hot = np.zeros(n, dtype=np.uint32)
    hot[n // 3] = 4000
    ramp = (np.arange(n, dtype=np.uint32) * 3 + 1)
    return [("all zero", np.zeros(n, dtype=np.uint32)), ("all equal", np.full(n, 1234, dtype=np.uint32)), ("one hot tile", hot),
            ("ascending", ramp), ("descending", ramp[::-1].copy()), ("full range", full),
            ("real range", rng.integers(0, 4001, n, dtype=np.uint64).astype(np.uint32))]


@pytest.fixture(scope="module")
def sort_rt(host):
    with host.RayTracer(0) as rt:
        yield rt


@pytest.mark.parametrize("with_accum", [False, True], ids=["no accum", "accum"])
@pytest.mark.parametrize("n", [1, 63, 1023, 1024, 1025, 4097])
def test_lpt_sort_is_heaviest_bin_first(sort_rt, n, with_accum):
    """rt_lpt_sort_kernel on caller-supplied costs: the order is a permutation, runs through sched_oracle.lpt_bins' bins from the
    heaviest down, holds in every bin exactly the reference's tiles, and the kernel clears the costs and adds them to accum."""
    rng = np.random.default_rng(0x5C4ED + n)
    for name, costs in cost_patterns(n, rng):
        what = f"n={n} {name}"
        prefill = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) if with_accum else None
        order, left, accum = sort_rt.lpt_sort(costs, prefill)
        assert is_permutation(order, n), f"{what}: not a permutation"
        bins = lpt_bins(costs)
        ran = bins[order]
        assert (np.diff(ran) >= 0).all(), f"{what}: not heaviest bin first"
        edges = np.flatnonzero(np.diff(ran)) + 1
        for seg in np.split(order, edges):
            b = bins[seg[0]]
            assert np.array_equal(np.sort(seg), np.flatnonzero(bins == b)), f"{what}: bin {b} holds other tiles than the reference's"
        assert not left.any(), f"{what}: costs not cleared"
        if with_accum:
            assert np.array_equal(accum, prefill + costs), f"{what}: accum is not prefill + costs (mod 2^32)"      # (uint32 wraps)
        else:
            assert accum is None


# ---- the predictor ----------------------------------------------------------------------------------------------------------------
def looking(p, pos=None, yaw=0.0, pitch=0.0):
    """p with the camera at pos (default: where it is) turned by yaw and pitch (degrees) from the scene's -z view."""
    cy, sy, cp, sp = np.cos(np.radians(yaw)), np.sin(np.radians(yaw)), np.cos(np.radians(pitch)), np.sin(np.radians(pitch))
    fwd = (float(F(sy * cp)), float(F(sp)), float(F(-cy * cp)))
    up = (float(F(-sy * sp)), float(F(cp)), float(F(cy * sp)))
    right = (float(F(cy)), 0.0, float(F(sy)))
    kw = dict(camDir=fwd, camUp=up, camRight=right)
    if pos is not None:
        kw["camPos"] = pos
    return L.copy_params(p, **kw)


@functools.lru_cache(maxsize=None)
def pred_scene(name):
    c2 = base_scene("c2")
    if name in ("c2", "c3"):
        return base_scene(name)
    if name == "spot+directional":
        # the spot ("area") light's cone leaves half of the floor unlit; the directional one lights what faces it
        sc = _own(c2, name, lights=c2.lights[:2].copy())
        sc.lights[0]["type"] = L.AREA
        sc.lights[0]["position"] = (0.0, 3.0, -4.0)
        sc.lights[0]["direction"] = (1.0, 0.2, 0.0)
        sc.lights[0]["intensity"] = 40.0
        sc.lights[1]["type"] = L.DIRECTIONAL
        sc.lights[1]["direction"] = (0.5, -1.0, -0.5)
        return sc
    if name == "hall":
        return hall_of_mirrors(diffuse_plane=False)      # (every hit object a mirror: the restriction of sched_oracle.predicted_classes)
    if name == "mirror c2":
        sc = opaque(c2, name)
        sc.objects["diffuseStrength"][:] = F(0.0)
        return sc
    if name == "subsurface":
        sc = _own(c2, name)                               # C2's subsurface sphere, and its floor made of the same stuff
        floor = int(np.flatnonzero(sc.objects["type"] == L.PLANE)[0])
        sc.objects["subsurfaceScatter"][floor] = F(0.5)
        return sc
    raise KeyError(name)


FRAMES = ("48x32", "ragged", "200x136")


def pred_params(sc, size, depth, view):
    if size == "ragged":
        p = ragged(sc, max_ray_depth=depth)
    else:
        w, h = (48, 32) if size == "48x32" else (200, 136)
        p = sc.params(width=w, height=h, max_ray_depth=depth)
    return looking(p, **view) if view else p


# (scene, depth, frame) -> the view of it: camera position (default: the scene's), yaw and pitch.  At these sizes a pixel is a
# degree wide and the scenes' own view puts half of the tile centres on a silhouette; these views were chosen, from a grid of
# 210, so that the reference alone decides at least 90 % of the tiles (none of check_prediction's conditions looks at the
# kernel's answer).  A case that does not meet them gets another view, never a larger cap.
NEAR, LEFT, RIGHT, FAR = (0.0, 1.5, 3.0), (-6.0, 3.0, 6.0), (5.0, 4.0, 2.0), (0.0, 6.0, 14.0)
VIEWS = {
    ("c2", 1, "48x32"): dict(pos=NEAR, yaw=60.0, pitch=-10.0),
    ("c2", 1, "ragged"): dict(pitch=20.0),
    ("c2", 1, "200x136"): dict(pos=RIGHT, yaw=-60.0, pitch=-25.0),
    ("c3", 1, "48x32"): dict(pos=FAR, yaw=-60.0),
    ("c3", 1, "ragged"): dict(pos=NEAR, yaw=-20.0, pitch=10.0),
    ("c3", 1, "200x136"): dict(pos=NEAR, yaw=40.0, pitch=-10.0),
    ("spot+directional", 1, "48x32"): dict(pos=NEAR, yaw=60.0, pitch=-10.0),
    ("spot+directional", 1, "ragged"): dict(pos=LEFT, yaw=40.0, pitch=-25.0),
    ("spot+directional", 1, "200x136"): dict(pos=RIGHT, yaw=-60.0, pitch=-25.0),
    ("hall", 3, "48x32"): dict(pos=LEFT, yaw=-60.0),
    ("hall", 8, "48x32"): dict(pos=LEFT, yaw=-60.0),
    ("hall", 3, "200x136"): dict(yaw=60.0, pitch=10.0),
    ("hall", 8, "200x136"): dict(pos=RIGHT, yaw=40.0),
    ("mirror c2", 3, "48x32"): dict(pos=LEFT, yaw=-60.0, pitch=10.0),
    ("mirror c2", 8, "48x32"): dict(pos=LEFT, yaw=-60.0, pitch=10.0),
    ("mirror c2", 3, "200x136"): dict(pos=NEAR, yaw=60.0, pitch=-25.0),
    ("mirror c2", 8, "200x136"): dict(pos=NEAR, yaw=60.0, pitch=-25.0),
    ("subsurface", 1, "48x32"): dict(pos=NEAR, yaw=60.0, pitch=-10.0),
    ("subsurface", 1, "200x136"): dict(pos=RIGHT, yaw=-60.0, pitch=-25.0),
}
PRED_CASES = ([(s, 1, f) for s in ("c2", "c3", "spot+directional") for f in FRAMES]
              + [(s, d, f) for s in ("hall", "mirror c2") for d in (3, 8) for f in ("48x32", "200x136")]
              + [("subsurface", 1, f) for f in ("48x32", "200x136")])


def check_prediction(rt, sc, p, lit, pcss, sss, what):
    """One frame of a fresh geometry: its order is the predicted one, runs through the classes from the heaviest down, keeps the
    ballot-prefix order inside a class and a block of 64 tile indices, and every tile's class lies in the reference's interval."""
    n = tiles_of(p)
    order, policy = frame(rt, p)
    cls = rt.predicted_classes(n).astype(np.int64)
    want = predicted_classes(rt, sc, p)
    sure = ~want.ambiguous & want.decided
    print(f"{what}: {n} tiles, {int(want.ambiguous.sum())} ambiguous, classes of the rest {sorted(set(want.lo[sure].tolist()))}, "
          f"pcf {int(want.pcf.sum())}, pcss {int(want.pcss.sum())}, sss {int(want.sss.sum())}, pulled up {int(want.pulled.sum())}; outside the interval: {int(((cls < want.lo) | (cls > want.hi)).sum())}")
    # the case itself, from the reference alone
    assert want.ambiguous.sum() <= 0.10 * n, f"{what}: {int(want.ambiguous.sum())} of {n} tiles are ambiguous"
    assert len(set(want.lo[sure].tolist())) >= 3, f"{what}: the unambiguous tiles hold fewer than three classes"
    assert not lit or want.pcf.any(), f"{what}: no unambiguous tile is priced with a PCF term"
    assert not pcss or want.pcss.any(), f"{what}: no unambiguous tile is priced with the PCSS term"
    assert not sss or want.sss.any(), f"{what}: no unambiguous tile is priced with the subsurface term"
    assert want.pulled.any(), f"{what}: no unambiguous tile owes its class to the neighbour pull-up"
    # the scheduler
    assert policy == PREDICTED, f"{what}: policy {policy}"
    assert is_permutation(order, n), f"{what}: the order is not a permutation"
    ran = cls[order]
    assert (np.diff(ran) <= 0).all(), f"{what}: the order does not run from the heaviest class down"
    group = ran * 1_000_000 + order.astype(np.int64) // 64
    for g in np.unique(group):
        ids = order[group == g].astype(np.int64)
        assert (np.diff(ids) > 0).all(), f"{what}: class {g // 1_000_000}, block {g % 1_000_000}: tile ids {ids.tolist()} do not ascend"
    bad = np.flatnonzero((cls < want.lo) | (cls > want.hi))
    assert bad.size == 0, f"{what}: tiles {bad.tolist()[:12]} have classes {cls[bad].tolist()[:12]}, the reference allows " \
                          f"{list(zip(want.lo[bad].tolist(), want.hi[bad].tolist()))[:12]}"


@pytest.mark.parametrize("name,depth,size", PRED_CASES, ids=[f"{s}-d{d}-{f}" for s, d, f in PRED_CASES])
def test_predicted_classes_and_order(make_rt, name, depth, size):
    sc = pred_scene(name)
    rt = make_rt(variant=1, RT_PRED_MIN_TILES=1, RT_DEBUG_PRED_CLASSES=1, RT_DEBUG_TILE_ORDER=1)
    rt.load(sc)
    p = pred_params(sc, size, depth, VIEWS[name, depth, size])
    check_prediction(rt, sc, p, lit=name in ("c2", "c3", "spot+directional", "subsurface"), pcss=name == "c3", sss=name == "subsurface",
                     what=f"{name} depth {depth} {size}")


# ---- which order a frame gets -----------------------------------------------------------------------------------------------------
def two_frames(sc):
    return [("48x32", sc.params()), ("ragged", ragged(sc))]


def identity(n):
    return np.arange(n, dtype=np.uint32)


def test_default_mode_predicts_then_measures(make_rt):
    sc = base_scene("c2")
    for what, p in two_frames(sc):
        rt = make_rt(RT_PRED_MIN_TILES=1, RT_DEBUG_TILE_ORDER=1)
        rt.load(sc)
        n = tiles_of(p)
        assert rt.tile_order()[0].size == 0, "no launch yet"
        assert frame(rt, p)[1] == PREDICTED, what
        for k in (1, 2):
            order, policy = frame(rt, p)
            assert policy == MEASURED and is_permutation(order, n), f"{what} frame {k}: policy {policy}"


def test_small_frames_start_in_raster_order(make_rt):
    """RT_PRED_MIN_TILES unset: no prediction for frames this small; and the measured-only and raster modes."""
    sc = base_scene("c2")
    for what, p in two_frames(sc):
        n = tiles_of(p)
        for variant, want in ((1 | REUSE_OFF, (RASTER, MEASURED, MEASURED)), (0x201 | REUSE_OFF, (RASTER, MEASURED, MEASURED)),
                              (0x101 | REUSE_OFF, (RASTER, RASTER, RASTER))):
            rt = make_rt(variant=variant, RT_DEBUG_TILE_ORDER=1)
            rt.load(sc)
            for k, policy_wanted in enumerate(want):
                order, policy = frame(rt, p)
                assert policy == policy_wanted, f"{what} variant {variant:#x} frame {k}: policy {policy}"
                assert is_permutation(order, n)
                if policy == RASTER:
                    assert np.array_equal(order, identity(n)), f"{what} variant {variant:#x} frame {k}"
            rt.close()


def test_without_the_variable_nothing_is_reported(make_rt):
    sc = base_scene("c2")
    rt = make_rt(RT_PRED_MIN_TILES=1)
    rt.load(sc)
    rt.render(sc.params())
    order, policy = rt.tile_order()
    assert order.size == 0 and policy == RASTER


def test_the_adopted_order_changes_only_behind_a_sort(make_rt):
    """RT_FB_PERIOD=4: measuredEnd sorts behind the frames of age 0, 1, 4, 8, ..., each sort is adopted by the next frame (the
    device is drained in between), and the frames up to the next adoption run in that very order."""
    sc = base_scene("c2")
    for what, p in two_frames(sc):
        rt = make_rt(RT_PRED_MIN_TILES=1, RT_DEBUG_TILE_ORDER=1, RT_FB_PERIOD=4)
        rt.load(sc)
        n = tiles_of(p)
        got = [frame(rt, p) for _ in range(13)]
        assert [q for _, q in got] == [PREDICTED] + [MEASURED] * 12, what
        assert all(is_permutation(o, n) for o, _ in got)
        adopted_at = (1, 2, 5, 9)                             # the frame behind each sort
        for k in range(2, 13):
            if k not in adopted_at:
                assert np.array_equal(got[k][0], got[k - 1][0]), f"{what}: frame {k} runs in another order than frame {k - 1}, with no sort between them"
        rt.close()


def test_new_geometry_and_mode_switch_restart_the_sequence(make_rt):
    sc = base_scene("c2")
    rt = make_rt(RT_PRED_MIN_TILES=1, RT_DEBUG_TILE_ORDER=1)
    rt.load(sc)
    small, window = sc.params(), ragged(sc)
    for what, p in (("48x32", small), ("ragged", window), ("48x32 again", small)):
        assert [frame(rt, p)[1] for _ in range(3)] == [PREDICTED, MEASURED, MEASURED], what
    rt.set_variant(1 | REUSE_OFF)
    assert rt.tile_order()[0].size == 0, "a mode switch forgets the last launch"
    assert [frame(rt, small)[1] for _ in range(3)] == [PREDICTED, MEASURED, MEASURED], "after rt_set_variant"
    rt.set_variant(0x201 | REUSE_OFF)
    assert [frame(rt, small)[1] for _ in range(3)] == [RASTER, MEASURED, MEASURED], "after the switch to measured only"


def test_the_first_replaying_frame_restarts_the_sequence(make_rt):
    """Reuse on, a still view: the replaying frames' tiles cost nothing like a whole frame's (Plan::costClass in rt_sched.h), so
    the first of them starts the feedback over: it does not run in a measured order, the next one does."""
    sc = base_scene("c2")
    for what, p in two_frames(sc):
        rt = make_rt(variant=1, RT_PRED_MIN_TILES=1, RT_DEBUG_TILE_ORDER=1)
        rt.load(sc)
        policies, replays = [], []
        for _ in range(5):
            before = rt.debug_first_hit()[2]
            policies.append(frame(rt, p)[1])
            replays.append(rt.debug_first_hit()[2] - before)
        assert 1 in replays and replays[-1] == 1, f"{what}: no frame replayed ({replays})"
        first = replays.index(1)
        assert first >= 2 and policies[first - 1] == MEASURED, f"{what}: policies {policies}, replays {replays}"
        assert policies[first] != MEASURED and policies[first + 1] == MEASURED, f"{what}: policies {policies}, replays {replays}"
        rt.close()


def test_tile_costs_of_a_measured_frame(make_rt):
    """Behind the third frame of a geometry (no sort clears the costs there) every tile with a pixel inside the image has a cost."""
    import torch
    from test_settled_tiles import tile_any
    sc = base_scene("c2")
    for what, p in two_frames(sc):
        rt = make_rt(RT_DEBUG_TILE_ORDER=1)
        rt.load(sc)
        for _ in range(3):
            order, policy = frame(rt, p)
        assert policy == MEASURED
        costs = rt.tile_costs()
        assert costs.shape == (-(-p.regionH // 8), -(-p.regionW // 8)), what
        rays = rt.camera_rays(p)
        torch.cuda.synchronize()
        inside = tile_any(~(rays.cpu().numpy()[..., 4:7] == 0).all(-1))
        assert inside.any() and (costs[inside] > 0).all(), f"{what}: tiles {np.argwhere(inside & (costs == 0)).tolist()} have no cost"
        rt.close()


# ---- phases -----------------------------------------------------------------------------------------------------------------------
def test_phase_orders_are_used_64_frames_later(make_rt):
    """frameCount advancing by one: from the third frame on every frame sorts its costs into its phase's order (frameCount mod
    64), which the frame 64 later runs in; until then the all-phase measured order."""
    sc = base_scene("c2")
    rt = make_rt(RT_DEBUG_TILE_ORDER=1)
    rt.load(sc)
    n = 24
    policies = []
    for k in range(140):
        order, policy = frame(rt, L.copy_params(sc.params(), frameCount=k))
        assert is_permutation(order, n), f"frame {k}"
        policies.append(policy)
    assert policies[0] == RASTER
    assert policies[1:66] == [MEASURED] * 65, policies[:66]
    assert policies[66:] == [PHASE] * 74, policies[66:]


def test_phase_orders_switched_off(make_rt):
    sc = base_scene("c2")
    rt = make_rt(RT_DEBUG_TILE_ORDER=1, RT_PHASE_ORDER=0)
    rt.load(sc)
    policies = [frame(rt, L.copy_params(sc.params(), frameCount=k))[1] for k in range(72)]
    assert policies == [RASTER] + [MEASURED] * 71


# ---- empty scenes -----------------------------------------------------------------------------------------------------------------
def test_an_empty_scene_is_not_predicted(make_rt):
    """Nothing to predict from, and rt_predict_tiles_kernel stages the objects in LDS sized by their count: raster order."""
    c2 = base_scene("c2")
    sc = _own(c2, "empty", objects=c2.objects[:0].copy())
    rt = make_rt(RT_PRED_MIN_TILES=1, RT_DEBUG_TILE_ORDER=1)
    rt.load(sc)
    order, policy = frame(rt, sc.params())
    assert policy == RASTER and np.array_equal(order, identity(24))
    assert frame(rt, sc.params())[1] == MEASURED
