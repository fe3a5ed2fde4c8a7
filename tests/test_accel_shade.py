"""GPU tests of rt_shade_rays through the hierarchy (rt_set_accel_shading; csrc/rt_accel_shade.inc).

The reference is the SAME context with shading-accel off: the brute-force kernel, which test_shade.py pins to the oracle and to both
render kernels.  With the feature on, colour, position and normal equal its output bit for bit (NaN == NaN) for every ray -- both
traversals -- and the launch counters of rt_accel_shading_info prove that the tree was walked, that nothing fell back, and that
rt_accel_info's query counters stood still."""
import ctypes

import numpy as np
import pytest

import accel_oracle as A
import accel_shade_oracle as S
from opengl_raytracing_amd import layout as L
from opengl_raytracing_amd import scenes
from test_query import random_rays
from test_shade import _np, assert_surfaces_equal, big_scene, branch_params, check_camera_identity

pytestmark = pytest.mark.gpu

TRAVERSALS = ["wave", "lane"]
SLOT = {"wave": 0, "lane": 1}              # rt_accel_shade_report.launchesAccel
LEAVES = [1, 4, 8]


@pytest.fixture(scope="module")
def rt(host):
    """A context of this module's own: both switches are sticky, and the session's tracers are other tests' reference."""
    r = host.RayTracer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def branches(host, oracle):
    """Test 1's scene and the oracle's frames of it, computed once: depth 6, depth 3, and depth 6 without shadows."""
    sc = S.branch_cloud_scene(host)
    p = branch_params(sc, 6)
    want = oracle.render(sc, p)[:3]
    shallow = oracle.render(sc, branch_params(sc, 3))[:3]
    unshadowed = scenes.Scene(sc.name, sc.objects, sc.lights.copy(), sc.width, sc.height, sc.max_ray_depth, sc.camera, sc.frame_count,
                              sc.noise, sc.skybox, sc.use_skybox)
    unshadowed.lights["shadowType"] = 0
    flat = oracle.render(unshadowed, branch_params(unshadowed, 6))[:3]
    return sc, p, want, shallow, flat


def to_device(rays):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8).copy()).cuda()


def random_pixels(n, seed):
    import torch
    px = np.random.default_rng(seed).integers(0, 2 ** 32, (n, 2), dtype=np.uint64).astype(np.uint32)
    return torch.from_numpy(px.view(np.int32)).cuda()


def shade(rt, p, rays, pixels=None, **kw):
    return [_np(t) for t in rt.shade_rays(p, rays, pixels=pixels, **kw)]


def query_counters(rt):
    i = rt.accel_info()
    return i["launches_accel"], i["launches_brute"]


def shade_on(rt, traversal, launch, launches, what, leaf_size=0):
    """launch() with the feature on (`launches` rt_shade_rays calls): through the tree by `traversal`, nothing falling back, the
    query counters standing still."""
    rt.set_accel(min_objects=1, leaf_size=leaf_size)
    rt.set_accel_shading(traversal=traversal, min_objects=1)
    before, q0 = rt.accel_shading_info(), query_counters(rt)
    assert before["active"] and rt.accel_info()["built"], what
    assert before["traversal"] == L.ACCEL_TRAVERSALS[traversal], what
    got = launch()
    after, q1 = rt.accel_shading_info(), query_counters(rt)
    rt.set_accel_shading(None)
    k = SLOT[traversal]
    assert after["launches_accel"][k] == before["launches_accel"][k] + launches, what
    assert after["launches_accel"][1 - k] == before["launches_accel"][1 - k] and after["launches_brute"] == before["launches_brute"], what
    assert q1 == q0, f"{what}: rt_accel_info counts queries only"
    return got


def check_on_off(rt, p, rays, pixels, traversal, what, leaf_size=0):
    """One shade of `rays` with the feature off, then on: equal on all three outputs.  -> the off result."""
    rt.set_accel_shading(None)
    want = shade(rt, p, rays, pixels)
    got = shade_on(rt, traversal, lambda: shade(rt, p, rays, pixels), 1, what, leaf_size)
    assert_surfaces_equal(got, want, f"{what} {traversal} leaf={leaf_size}")
    return want


def primary_hits(off):
    """Rays whose primary segment hit something, from the off result: a path that misses at once leaves P = 0."""
    return (off[1][..., :3] != 0).any(-1)


# ---- 1. every branch, in a scene with a real tree --------------------------------------------------------------------
def test_the_oracles_frame_is_not_flat(branches, host):
    sc, p, want, shallow, flat = branches
    hit = (want[1][..., :3] != 0).any(-1)
    assert hit.any() and (~hit).any(), "the frame needs both hit and miss pixels"
    assert len(np.unique(want[0][..., :3].reshape(-1, 3).view(np.uint32), axis=0)) >= 100, "fewer than 100 distinct colours"
    differs = lambda a, b: (~((a == b) | (np.isnan(a) & np.isnan(b)))).any(-1)
    assert differs(want[0], flat[0]).sum() >= 100, "fewer than 100 pixels change when every light's shadowType is 0"
    assert differs(want[0], shallow[0]).sum() >= 20, "fewer than 20 pixels differ between maxRayDepth 3 and 6"
    acc = host.accel_build_host(sc.objects)
    assert acc.info["nodes"] >= 63 and acc.info["depth"] >= 5, "a real tree"


@pytest.mark.parametrize("traversal", TRAVERSALS)
@pytest.mark.parametrize("leaf", LEAVES)
def test_every_branch_on_off_oracle_and_packet_render(rt, branches, leaf, traversal):
    import torch
    sc, p, want, _, _ = branches
    rt.set_variant(1)
    rt.load(sc)
    rays = rt.camera_rays(p)
    off = check_on_off(rt, p, rays, None, traversal, sc.name, leaf_size=leaf)
    assert_surfaces_equal(off, want, f"{sc.name}: rt_shade_rays (off) vs the oracle")
    col = torch.empty((p.regionH, p.regionW, 4), dtype=torch.float32, device="cuda")
    pos, nrm = torch.empty_like(col), torch.empty((p.regionH, p.regionW, 4), dtype=torch.float16, device="cuda")
    rt.render_to(p, col, pos, nrm)
    torch.cuda.synchronize()
    assert_surfaces_equal([_np(col), _np(pos), _np(nrm)], want, f"{sc.name}: packet rt_render_to vs the oracle")


# ---- 2. the hostile scene --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("traversal", TRAVERSALS)
def test_hostile_scene_and_rays(rt, host, traversal):
    objs = A.hostile_scene(host)
    sc = scenes.Scene("hostile", objs, S.hostile_lights(), 64, 64, 4, dict(scenes.CAMERA), frame_count=3)
    rt.load(sc)
    acc = host.accel_build_host(objs)
    n = 2 ** 13 + 37
    rays, pix = to_device(A.hostile_rays(objs, acc, n, seed=7)), random_pixels(n, 7)
    p = sc.params(max_ray_depth=4)
    for leaf in LEAVES:
        off = check_on_off(rt, p, rays, pix, traversal, "hostile", leaf_size=leaf)
    hit = primary_hits(off)
    assert hit.sum() >= 1000 and (~hit).sum() >= 1000, f"{int(hit.sum())} primary hits, {int((~hit).sum())} misses"


# ---- 3. size ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("traversal", TRAVERSALS)
@pytest.mark.parametrize("n", [2048, 4096])
def test_lit_clouds(rt, host, n, traversal):
    sc = scenes.lit_cloud(n, n, host.generate_aabb)
    rt.load(sc)
    p = sc.params(width=64, height=36, max_ray_depth=3)
    off = check_on_off(rt, p, rt.camera_rays(p), None, traversal, f"{sc.name} camera")
    assert primary_hits(off).mean() > 0.2, "the camera frame sees the cloud (the restatement: 32 % of the rays at 2048, 38 % at 4096)"
    acc = host.accel_build_host(sc.objects)
    m = 2 ** 13 + 37
    off = check_on_off(rt, p, to_device(A.hostile_rays(sc.objects, acc, m, seed=7)), random_pixels(m, n), traversal, f"{sc.name} hostile")
    hit = primary_hits(off)
    assert hit.sum() >= 1000 and (~hit).sum() >= 1000, f"{int(hit.sum())} primary hits, {int((~hit).sum())} misses"


@pytest.mark.parametrize("traversal", TRAVERSALS)
def test_65536_spheres(rt, host, traversal):
    objs = A.cloud_scene(host, 65536, seed=3, floor=False)
    sc = scenes.Scene("spheres65536", objs, S.cloud_lights_for(65536), 64, 64, 2, dict(scenes.CAMERA))
    rt.load(sc)
    off = check_on_off(rt, sc.params(), to_device(random_rays(objs, 1024, seed=12)), random_pixels(1024, 12), traversal, sc.name)
    assert primary_hits(off).sum() >= 100


# ---- 4. tails, layouts and optional outputs --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_ray_counts_and_tails(rt, branches, n):
    import torch
    sc, p, _, _, _ = branches
    rt.load(sc)
    rays, pix = to_device(random_rays(sc.objects, n, seed=n)), random_pixels(n, n)
    rt.set_accel_shading(None)
    want = shade(rt, p, rays, pix)
    for traversal in TRAVERSALS:
        outs = (torch.full((n + 64, 4), 12345.0, dtype=torch.float32, device="cuda"),
                torch.full((n + 64, 4), 12345.0, dtype=torch.float32, device="cuda"),
                torch.full((n + 64, 4), 7.0, dtype=torch.float16, device="cuda"))
        shade_on(rt, traversal, lambda: rt.shade_rays(p, rays, pixels=pix, out=tuple(t[:n] for t in outs)), 1, f"n={n}")
        full = [_np(t) for t in outs]
        assert (full[0][n:] == 12345.0).all() and (full[1][n:] == 12345.0).all() and (full[2][n:] == 7.0).all(), f"{traversal}: wrote past the last ray"
        assert_surfaces_equal([f[:n] for f in full], want, f"{traversal} n={n}")


@pytest.mark.parametrize("traversal", TRAVERSALS)
def test_optional_outputs_windows_strips_and_permutations(rt, host, branches, traversal):
    import torch
    sc, p, _, _, _ = branches
    rt.load(sc)
    # colour alone
    rays = rt.camera_rays(p)
    rt.set_accel_shading(None)
    want = shade(rt, p, rays)
    col, no_pos, no_nrm = shade_on(rt, traversal, lambda: rt.shade_rays(p, rays, position=False, normal=False), 1, "colour alone")
    assert no_pos is None and no_nrm is None
    assert_surfaces_equal([_np(col)], want[:1], "colour without position / normal outputs")
    # pixels=None, a window that crosses the image's right and top edge: zero records outside
    q = sc.params(window=(sc.width - 20, sc.height - 10, 40, 24), max_ray_depth=4)
    q.noiseScale[0], q.noiseScale[1] = 1.0 / 64.0, 1.0 / 32.0
    off = check_on_off(rt, q, rt.camera_rays(q), None, traversal, "window across the edge")
    j, i = np.mgrid[0:q.regionH, 0:q.regionW]
    outside = (q.x0 + i >= sc.width) | (q.y0 + j >= sc.height)
    assert outside.any() and (~outside).any()
    for name, o in zip(("colour", "position", "normal"), off):
        assert (o.reshape(q.regionH, q.regionW, 4)[outside].view(np.uint16 if name == "normal" else np.uint32) == 0).all(), f"{name}: not zero outside the image"
    # a strip layout
    rows, cnt, idx = 4, 3, 1
    local = host.strip_local_rows(sc.height, rows, cnt, idx)
    s = sc.params(window=(3, 1, 40, local - 1), strips=(rows, cnt, idx), max_ray_depth=4)
    s.noiseScale[0], s.noiseScale[1] = 1.0 / 64.0, 1.0 / 32.0
    check_on_off(rt, s, rt.camera_rays(s), None, traversal, "strips")
    # a permutation of the rays permutes the outputs
    n = 1000
    r, pix = to_device(random_rays(sc.objects, n, seed=41)), random_pixels(n, 41)
    base = shade(rt, p, r, pix)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(n)).cuda()
    got = shade_on(rt, traversal, lambda: shade(rt, p, r[perm].contiguous(), pix[perm].contiguous()), 1, "permuted")
    assert_surfaces_equal(got, [b[perm.cpu().numpy()] for b in base], "permuted rays")


# ---- 5. against the renderer -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("traversal", TRAVERSALS)
def test_big_scene_equals_the_packet_render(rt, host, traversal):
    sc = big_scene(host)
    rt.set_variant(1)
    rt.load(sc)
    p = sc.params()
    assert (p.regionW, p.regionH) == (128, 72)
    shade_on(rt, traversal, lambda: check_camera_identity(rt, p, "2048 objects / 70 lights, feature on, vs the packet render", explicit=False), 1,
             "big scene")


# ---- 6. downstream ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("traversal", TRAVERSALS)
def test_sparse_pixels_through_camera_rays_at(rt, branches, traversal):
    import torch
    sc, p, _, _, _ = branches
    rt.load(sc)
    rt.set_accel_shading(None)
    full = shade(rt, p, rt.camera_rays(p))
    rng = np.random.default_rng(6)
    n = 301
    flat = rng.choice(sc.width * sc.height, n, replace=False)
    px = np.stack([flat % sc.width, flat // sc.width], -1).astype(np.int32)
    d = torch.from_numpy(px).cuda()
    got = shade_on(rt, traversal, lambda: shade(rt, p, rt.camera_rays_at(p, d, n), d), 1, "sparse pixels")
    assert_surfaces_equal(got, [f.reshape(-1, 4)[flat] for f in full], "camera_rays_at -> shade_rays vs the full frame")


# ---- 7. switches, counters, lifecycle --------------------------------------------------------------------------------
def _state(rt):
    i = rt.accel_shading_info()
    return i["active"], i["traversal"]


def test_switches_counters_and_lifecycle(rt, host, branches):
    sc, p, _, _, _ = branches
    other = scenes.lit_cloud(300, 9, host.generate_aabb)
    rt.set_accel(None)
    rt.set_accel_shading(None)
    rt.load(sc)
    rays = rt.camera_rays(p)
    want = shade(rt, p, rays)
    # off by default: rt_set_accel alone changes nothing for rt_shade_rays
    rt.set_accel(min_objects=1)
    i0 = rt.accel_shading_info()
    assert not i0["active"] and i0["traversal"] == 0
    assert_surfaces_equal(shade(rt, p, rays), want, "rt_set_accel alone")
    assert rt.accel_shading_info() == i0, "a shade launch counts nothing while shading-accel is off"
    # either order of the two switches gives the same state
    rt.set_accel_shading(traversal="wave", min_objects=1)
    first = _state(rt)
    rt.set_accel(None)
    rt.set_accel_shading(None)
    rt.set_accel_shading(traversal="wave", min_objects=1)
    assert _state(rt) == (False, L.ACCEL_WAVE), "shading on, no tree yet"
    rt.set_accel(min_objects=1)
    assert _state(rt) == first == (True, L.ACCEL_WAVE)
    assert rt.accel_shading_info()["launches_accel"] == i0["launches_accel"]
    # auto resolves to one of the two walks
    rt.set_accel_shading()
    assert rt.accel_shading_info()["traversal"] in (L.ACCEL_LANE, L.ACCEL_WAVE)
    # rt_set_accel(None): brute force, counted as such
    rt.set_accel_shading(traversal="lane", min_objects=1)
    rt.set_accel(None)
    i1 = rt.accel_shading_info()
    assert not i1["active"]
    assert_surfaces_equal(shade(rt, p, rays), want, "no tree")
    i2 = rt.accel_shading_info()
    assert i2["launches_brute"] == i1["launches_brute"] + 1 and i2["launches_accel"] == i1["launches_accel"]
    # below min_objects: brute force
    rt.set_accel(min_objects=1)
    rt.set_accel_shading(traversal="lane", min_objects=len(sc.objects) + 1)
    assert not rt.accel_shading_info()["active"]
    assert_surfaces_equal(shade(rt, p, rays), want, "below min_objects")
    i3 = rt.accel_shading_info()
    assert i3["launches_brute"] == i2["launches_brute"] + 1 and i3["launches_accel"] == i2["launches_accel"]
    rt.set_accel_shading(traversal="lane", min_objects=len(sc.objects))
    assert rt.accel_shading_info()["active"], "nObj >= minObjects"
    # rt_set_scene with changed bytes: the next shade is the new scene's; an identical re-upload rebuilds nothing
    rt.set_accel_shading(None)
    q = other.params(width=48, height=32, max_ray_depth=3)
    rt.load(other)
    rays_o = rt.camera_rays(q)
    want_o = shade(rt, q, rays_o)
    rt.load(sc)
    rt.set_accel_shading(traversal="lane", min_objects=1)
    builds = rt.accel_info()["builds"]
    rt.set_scene(other.objects, other.lights)
    rt.set_noise(other.noise)
    rt.set_skybox(None)
    assert rt.accel_info()["builds"] == builds + 1 and rt.accel_shading_info()["active"]
    i4 = rt.accel_shading_info()
    assert_surfaces_equal(shade(rt, q, rays_o), want_o, "after rt_set_scene with changed bytes")
    rt.set_scene(other.objects, other.lights)
    assert rt.accel_info()["builds"] == builds + 1, "an identical re-upload rebuilds nothing"
    assert_surfaces_equal(shade(rt, q, rays_o), want_o, "after an identical re-upload")
    i5 = rt.accel_shading_info()
    assert i5["launches_accel"] == (i4["launches_accel"][0], i4["launches_accel"][1] + 2) and i5["launches_brute"] == i4["launches_brute"]
    rt.set_accel_shading(None)
    rt.set_accel(None)


def test_refusals(rt, host):
    lib, ctx = rt.lib, rt.ctx
    before = rt.accel_shading_info()
    assert lib.rt_accel_shading_info(ctx, None) == -1, "NULL report"
    assert lib.rt_accel_shading_info(None, ctypes.byref(L.RtAccelShadeReport())) == -1, "NULL context"
    assert lib.rt_set_accel_shading(None, None) == -1, "NULL context"
    for bad in (dict(traversal=3), dict(traversal=-1), dict(min_objects=-1)):
        with pytest.raises(host.RtError):
            rt.set_accel_shading(**bad)
    for k in range(5):
        d = L.make_accel_shade_desc()
        d.reserved[k] = 1
        assert lib.rt_set_accel_shading(ctx, ctypes.byref(d)) == -1, f"reserved[{k}]"
    assert rt.accel_shading_info() == before, "a refused call changes nothing"
    d = L.make_accel_shade_desc(False, "wave", 5)
    assert lib.rt_set_accel_shading(ctx, ctypes.byref(d)) == 0 and rt.accel_shading_info()["traversal"] == 0, "enable == 0: off"


# ---- 8. ordering -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("traversal", TRAVERSALS)
def test_shading_on_a_side_stream_is_ordered_with_scene_updates(rt, host, traversal):
    """test_accel.py's stream test for shade launches: the tree's re-upload waits for a shade in flight on a foreign stream, and a
    shade issued after rt_set_scene walks the new tree."""
    import torch
    A2, B4 = scenes.make_scene(2, host.generate_aabb), scenes.make_scene(4, host.generate_aabb)
    p = A2.params(width=512, height=288, max_ray_depth=3)
    rt.set_accel(None)
    rt.set_accel_shading(None)
    rt.load(B4)
    rays = rt.camera_rays(p)
    want_b = shade(rt, p, rays)
    rt.load(A2)
    want_a = shade(rt, p, rays)
    rt.set_accel(min_objects=1)
    rt.set_accel_shading(traversal=traversal, min_objects=1)
    before = rt.accel_shading_info()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        r2 = rays.clone()
        qa = rt.shade_rays(p, r2, stream=s)
    rt.set_scene(B4.objects, B4.lights)
    with torch.cuda.stream(s):
        qb = rt.shade_rays(p, r2, stream=s)
    torch.cuda.synchronize()
    after = rt.accel_shading_info()
    rt.set_accel_shading(None)
    rt.set_accel(None)
    assert after["active"] and after["launches_accel"][SLOT[traversal]] == before["launches_accel"][SLOT[traversal]] + 2
    assert_surfaces_equal([_np(t) for t in qa], want_a, "shade before rt_set_scene(B)")
    assert_surfaces_equal([_np(t) for t in qb], want_b, "shade after rt_set_scene(B)")
