"""GPU tests of the hierarchy behind rt_trace_rays / rt_pick (rt_set_accel; csrc/rt_accel.inc).

The reference is the SAME context with the feature off: the brute-force kernels, which test_query.py pins to the oracle.  With the
feature on, every rt_hit equals theirs on all 32 bytes (NaN payloads aside, conftest.bits_equal's convention) and every any-hit
int equals theirs, for every ray -- both traversals, both modes -- and the launch counters of rt_accel_info prove that the tree was
walked and nothing fell back."""
import numpy as np
import pytest

import accel_oracle as A
from opengl_raytracing_amd import layout as L
from opengl_raytracing_amd import scenes
from test_query import random_rays

pytestmark = pytest.mark.gpu

TRAVERSALS = ["wave", "lane"]
SLOT = {"wave": 0, "lane": 1}              # rt_accel_report.launchesAccel


@pytest.fixture(scope="module")
def rt(host):
    """A context of this module's own: rt_set_accel is sticky, and the session's tracers are other tests' reference."""
    r = host.RayTracer(0)
    yield r
    r.close()


def same_hits(got, want):
    """[n, 8] float32 rt_hit rows: the seven floats bit for bit (NaN == NaN), the object index exactly."""
    g, w = np.ascontiguousarray(got).reshape(-1, 8), np.ascontiguousarray(want).reshape(-1, 8)
    gi, wi = g.view(np.uint32), w.view(np.uint32)
    floats = (gi[:, :7] == wi[:, :7]) | (np.isnan(g[:, :7]) & np.isnan(w[:, :7]))
    return bool(floats.all() and (gi[:, 7] == wi[:, 7]).all())


def to_device(rays):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8).copy()).cuda()


def trace_both_modes(rt, d):
    import torch
    h, a = rt.trace_rays(d, "closest"), rt.trace_rays(d, "any")
    torch.cuda.synchronize()
    return h.cpu().numpy(), a.cpu().numpy()


def check_against_brute_force(rt, d, traversal, what, leaf_size=0):
    """Both modes over the device rays d with the feature off, then on: equal, through the tree, with nothing falling back."""
    rt.set_accel(None)
    want_h, want_a = trace_both_modes(rt, d)
    rt.set_accel(traversal=traversal, min_objects=1, leaf_size=leaf_size)
    before = rt.accel_info()
    assert before["built"] and before["nodes"] > 0, what
    got_h, got_a = trace_both_modes(rt, d)
    after = rt.accel_info()
    rt.set_accel(None)
    k = SLOT[traversal]
    assert after["launches_accel"][k] == before["launches_accel"][k] + 2 and after["launches_accel"][1 - k] == before["launches_accel"][1 - k], what
    assert after["launches_brute"] == before["launches_brute"], what
    assert same_hits(got_h, want_h), f"{what} {traversal}: closest hits differ on {int((got_h.view(np.uint32) != want_h.view(np.uint32)).any(-1).sum())} rays"
    assert (got_a == want_a).all(), f"{what} {traversal}: any-hit differs on {int((got_a != want_a).sum())} rays"
    obj = want_h.view(np.int32)[:, 7]
    assert (want_a == (obj >= 0)).all(), what
    return obj


@pytest.mark.parametrize("traversal", TRAVERSALS)
@pytest.mark.parametrize("cfg", [2, 4, 5])
def test_shipped_scenes_camera_and_hostile_rays(rt, host, cfg, traversal):
    import torch
    sc = scenes.make_scene(cfg, host.generate_aabb)
    rt.load(sc)
    cam = rt.camera_rays(sc.params(width=160, height=90)).reshape(-1, 8)
    torch.cuda.synchronize()
    obj = check_against_brute_force(rt, cam, traversal, f"C{cfg} camera")
    assert len(np.unique(obj)) > 3
    acc = host.accel_build_host(sc.objects)
    rays = A.hostile_rays(sc.objects, acc, 2 ** 16 + 37, seed=100 + cfg)
    check_against_brute_force(rt, to_device(rays), traversal, f"C{cfg} hostile")


@pytest.mark.parametrize("traversal", TRAVERSALS)
@pytest.mark.parametrize("name", ["cloud2048", "cloud4096", "hostile"])
def test_clouds_and_the_constructed_scene(rt, host, name, traversal):
    objs = A.hostile_scene(host) if name == "hostile" else A.cloud_scene(host, int(name[5:]), seed=int(name[5:]))
    rt.set_scene(objs, L.default_lights(1))
    acc = host.accel_build_host(objs)
    rays = A.hostile_rays(objs, acc, 2 ** 15 + 37, seed=7)
    for leaf in ((1, 4, 8) if name == "hostile" else (0,)):
        obj = check_against_brute_force(rt, to_device(rays), traversal, name, leaf_size=leaf)
    assert (obj >= 0).sum() > 1000 and (obj < 0).sum() > 1000
    if name != "hostile":
        assert len(acc.loose) <= 1 + len(objs) // 256


@pytest.mark.parametrize("traversal", TRAVERSALS)
def test_65536_spheres(rt, host, traversal):
    objs = A.cloud_scene(host, 65536, seed=3, floor=False)
    rt.set_scene(objs, L.default_lights(1))
    rays = random_rays(objs, 4096, seed=12)
    obj = check_against_brute_force(rt, to_device(rays), traversal, "65536 spheres")
    assert (obj >= 0).sum() > 500


@pytest.mark.parametrize("n", [1, 63, 65, 257, 3 * 2 ** 16 + 5])
def test_ray_counts_and_tails(rt, host, n):
    import torch
    sc = scenes.make_scene(4, host.generate_aabb)
    rt.set_scene(sc.objects, sc.lights)
    d = to_device(random_rays(sc.objects, n, seed=n))
    rt.set_accel(None)
    want_h, want_a = trace_both_modes(rt, d)
    for traversal in TRAVERSALS:
        rt.set_accel(traversal=traversal, min_objects=1)
        out = torch.full((n + 64, 8), 12345.0, dtype=torch.float32, device="cuda")
        outa = torch.full((n + 64,), 7, dtype=torch.int32, device="cuda")
        rt.trace_rays(d, "closest", out=out[:n])
        rt.trace_rays(d, "any", out=outa[:n])
        torch.cuda.synchronize()
        h, a = out.cpu().numpy(), outa.cpu().numpy()
        assert (h[n:] == 12345.0).all() and (a[n:] == 7).all(), f"{traversal}: a query wrote past its last ray"
        assert same_hits(h[:n], want_h) and (a[:n] == want_a).all(), f"{traversal} n={n}"
    rt.set_accel(None)


def test_pick_equals_the_brute_force_pick(rt, host):
    sc = scenes.make_scene(5, host.generate_aabb)
    rt.load(sc)
    W, H = 320, 180
    p = sc.params(width=W, height=H)
    rng = np.random.default_rng(5)
    pts = [(0, 0), (W - 1, H - 1)] + [(int(x), int(y)) for x, y in zip(rng.integers(0, W, 30), rng.integers(0, H, 30))]
    rt.set_accel(None)
    want = [rt.pick(p, x, y) for x, y in pts]
    rt.set_accel(min_objects=1)
    before = rt.accel_info()
    got = [rt.pick(p, x, y) for x, y in pts]
    after = rt.accel_info()
    rt.set_accel(None)
    assert after["launches_accel"][0] == before["launches_accel"][0] + len(pts) and after["launches_brute"] == before["launches_brute"]
    for g, w in zip(got, want):
        row = lambda k: np.concatenate([k.position, [k.t], k.normal]).astype(np.float32)
        assert g.object == w.object and same_hits(np.append(row(g), 0), np.append(row(w), 0))
    assert len({w.object for w in want}) > 3


def test_first_hit_records_of_a_view_are_the_same_bytes(rt, host):
    """camera_rays -> trace_rays is what the denoiser's guide, the reprojection and the upsampler are fed: identical records with
    the feature on (RT_ACCEL_AUTO, and the per-wavefront walk a caller of camera rays would ask for) and off."""
    import torch
    sc = scenes.make_scene(5, host.generate_aabb)
    rt.load(sc)
    p = sc.params(width=384, height=216)
    rt.set_accel(None)
    want = rt.trace_rays(rt.camera_rays(p)).cpu().numpy()
    for traversal in ("auto", "wave"):
        rt.set_accel(traversal=traversal, min_objects=64)
        before = rt.accel_info()
        assert before["built"]
        got = rt.trace_rays(rt.camera_rays(p)).cpu().numpy()
        torch.cuda.synchronize()
        after = rt.accel_info()
        rt.set_accel(None)
        assert sum(after["launches_accel"]) == sum(before["launches_accel"]) + 1 and after["launches_brute"] == before["launches_brute"]
        assert same_hits(got, want), traversal
    assert (want.view(np.int32)[..., 7] >= 0).mean() > 0.3


def test_defaults_build_from_1024_objects_and_auto_walks_per_ray(rt, host):
    for n_spheres, built in ((1023, True), (1022, False)):              # + the floor
        objs = A.cloud_scene(host, n_spheres, seed=8)
        rt.set_accel(None)
        rt.set_scene(objs, L.default_lights(1))
        d = to_device(random_rays(objs, 1000, seed=8))
        want, _ = trace_both_modes(rt, d)
        rt.set_accel()
        before = rt.accel_info()
        assert before["built"] == built
        got, _ = trace_both_modes(rt, d)
        after = rt.accel_info()
        rt.set_accel(None)
        assert same_hits(got, want)
        assert after["launches_accel"] == (before["launches_accel"][0], before["launches_accel"][1] + (2 if built else 0))
        assert after["launches_brute"] == before["launches_brute"] + (0 if built else 2)


def test_counters_and_lifecycle(rt, host):
    A2, B4 = scenes.make_scene(2, host.generate_aabb), scenes.make_scene(4, host.generate_aabb)
    d = to_device(random_rays(B4.objects, 4096, seed=3))
    rt.set_scene(B4.objects, B4.lights)
    rt.set_accel(None)
    want_b, _ = trace_both_modes(rt, d)
    rt.set_scene(A2.objects, A2.lights)
    want_a, _ = trace_both_modes(rt, d)
    off = rt.accel_info()
    assert not off["built"] and off["nodes"] == 0
    # below minObjects (18 objects < the default 1024): served by brute force, and counted as such
    rt.set_accel()
    i0 = rt.accel_info()
    assert not i0["built"] and i0["builds"] == off["builds"]
    got, _ = trace_both_modes(rt, d)
    i1 = rt.accel_info()
    assert i1["launches_brute"] == i0["launches_brute"] + 2 and i1["launches_accel"] == i0["launches_accel"]
    assert same_hits(got, want_a)
    # switched on for this scene: built at once
    rt.set_accel(min_objects=1)
    i2 = rt.accel_info()
    assert i2["built"] and i2["builds"] == i1["builds"] + 1 and i2["loose"] == 2 and i2["leaves"] >= 4 and i2["bytes"] == 32 * i2["nodes"] + 4 * 18
    # an identical scene: no rebuild; a changed one: a rebuild, and the next query is the new scene's
    rt.set_scene(A2.objects, A2.lights)
    assert rt.accel_info()["builds"] == i2["builds"]
    rt.set_scene(B4.objects, B4.lights)
    i3 = rt.accel_info()
    assert i3["builds"] == i2["builds"] + 1 and i3["built"] and i3["nodes"] > i2["nodes"]
    got, _ = trace_both_modes(rt, d)
    i4 = rt.accel_info()
    assert same_hits(got, want_b)
    assert sum(i4["launches_accel"]) == sum(i3["launches_accel"]) + 2 and i4["launches_brute"] == i3["launches_brute"]
    # off: the counters stand still, the results stay
    rt.set_accel(None)
    i5 = rt.accel_info()
    got, _ = trace_both_modes(rt, d)
    i6 = rt.accel_info()
    assert same_hits(got, want_b)
    assert (i6["launches_accel"], i6["launches_brute"], i6["builds"]) == (i5["launches_accel"], i5["launches_brute"], i5["builds"])
    assert not i6["built"]
    with pytest.raises(host.RtError):
        rt.set_accel(traversal=5)
    with pytest.raises(host.RtError):
        rt.set_accel(leaf_size=9)


@pytest.mark.parametrize("traversal", TRAVERSALS)
def test_queries_on_a_side_stream_are_ordered_with_scene_updates(rt, host, traversal):
    """test_query.py's stream test with the feature on: the structure's upload is ordered like the scene's own."""
    import torch
    A2, B4 = scenes.make_scene(2, host.generate_aabb), scenes.make_scene(4, host.generate_aabb)
    d = to_device(random_rays(A2.objects, 1 << 18, seed=5))
    rt.set_accel(None)
    rt.set_scene(B4.objects, B4.lights)
    want_b = rt.trace_rays(d).cpu().numpy()
    rt.set_scene(A2.objects, A2.lights)
    want_a = rt.trace_rays(d).cpu().numpy()
    rt.set_accel(traversal=traversal, min_objects=1)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d2 = d.clone()
        qa = rt.trace_rays(d2, "closest", stream=s)
    rt.set_scene(B4.objects, B4.lights)
    with torch.cuda.stream(s):
        qb = rt.trace_rays(d2, "closest", stream=s)
    torch.cuda.synchronize()
    info = rt.accel_info()
    rt.set_accel(None)
    assert info["built"] and info["launches_accel"][SLOT[traversal]] >= 2
    assert same_hits(qa.cpu().numpy(), want_a), "query before rt_set_scene(B)"
    assert same_hits(qb.cpu().numpy(), want_b), "query after rt_set_scene(B)"
