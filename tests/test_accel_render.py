"""GPU tests of whole frames through the hierarchy (rt_set_accel_render; csrc/rt_accel_render.inc).

The reference is the SAME context with the switch off: the packet kernel, which test_gpu_parity.py and test_shade.py pin to the
oracle.  With the switch on, all three surfaces equal its output bit for bit (NaN == NaN) -- LANE, WAVE and SPLIT -- and
rt_accel_render_info, read before and after every comparison, proves which kernel ran: the expected slot rose by the number of
frames, the other slots and launchesPacket stood still, and so did rt_accel_info's and rt_accel_shading_info's counters.  Every
surface a frame is rendered into is followed by sentinels, which must survive."""
import ctypes

import numpy as np
import pytest

import accel_oracle as A
import accel_shade_oracle as S
from opengl_raytracing_amd import layout as L
from opengl_raytracing_amd import scenes
from test_shade import _np, assert_surfaces_equal, big_scene, branch_params

pytestmark = pytest.mark.gpu

TRAVERSALS = ["wave", "lane", "split"]
SLOT = {"wave": 0, "lane": 1, "split": 2}          # rt_accel_render_report.launchesAccel
PACKET = "packet"                                  # ... or launchesPacket
PAD = 64                                           # sentinel pixels behind every surface
COLOUR_SENTINEL, NORMAL_SENTINEL = 12345.0, 7.0


@pytest.fixture(scope="module")
def rt(host):
    """A context of this module's own: the switches are sticky, and the session's tracers are other tests' reference."""
    r = host.RayTracer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def branches(host, oracle):
    """Test 1's scene, its depth-6 frame and the oracle's surfaces of it, computed once."""
    sc = S.branch_cloud_scene(host)
    p = branch_params(sc, 6)
    return sc, p, oracle.render(sc, p)[:3]


def window_params(sc, window=None, strips=None, depth=4, **updates):
    """An 80 x 40 image of the branch scene (so that windows up to 65 pixels wide fit), its noise texture addressed as in test 1."""
    p = sc.params(width=80, height=40, window=window, strips=strips, max_ray_depth=depth)
    p.noiseScale[0], p.noiseScale[1] = 1.0 / 64.0, 1.0 / 32.0
    return L.copy_params(p, **updates) if updates else p


def snapshot(rt):
    a, s = rt.accel_info(), rt.accel_shading_info()
    return rt.accel_render_info(), (a["launches_accel"], a["launches_brute"]), (s["launches_accel"], s["launches_brute"])


def assert_counted(before, after, slot, frames, what):
    """`frames` frames went to `slot` (SLOT's index, or PACKET) and nothing else moved."""
    (r0, q0, s0), (r1, q1, s1) = before, after
    want = list(r0["launches_accel"])
    packet = r0["launches_packet"]
    if slot == PACKET:
        packet += frames
    else:
        want[slot] += frames
    assert list(r1["launches_accel"]) == want, f"{what}: launchesAccel {r0['launches_accel']} -> {r1['launches_accel']}, expected {want}"
    assert r1["launches_packet"] == packet, f"{what}: launchesPacket {r0['launches_packet']} -> {r1['launches_packet']}, expected {packet}"
    assert q1 == q0, f"{what}: rt_accel_info counts queries only"
    assert s1 == s0, f"{what}: rt_accel_shading_info counts rt_shade_rays launches only"


def frames_on(rt, traversal, launch, frames, what, leaf_size=0):
    """launch() with the switch on (`frames` frames): through the tree by `traversal`, nothing taking the packet kernel."""
    rt.set_accel(min_objects=1, leaf_size=leaf_size)
    rt.set_accel_render(traversal=traversal, min_objects=1)
    before = snapshot(rt)
    assert before[0]["active"] and rt.accel_info()["built"], what
    assert before[0]["traversal"] == L.ACCEL_RENDER_TRAVERSALS[traversal] and before[0]["min_objects"] == 1, what
    got = launch()
    after = snapshot(rt)
    rt.set_accel_render(None)
    assert_counted(before, after, SLOT[traversal], frames, f"{what} {traversal}")
    return got


def surfaces(n):
    """Three flat surfaces of n pixels, PAD sentinel pixels behind each (and every pixel a sentinel until a frame writes it)."""
    import torch
    bufs = (torch.full((n + PAD, 4), COLOUR_SENTINEL, dtype=torch.float32, device="cuda"),
            torch.full((n + PAD, 4), COLOUR_SENTINEL, dtype=torch.float32, device="cuda"),
            torch.full((n + PAD, 4), NORMAL_SENTINEL, dtype=torch.float16, device="cuda"))
    torch.cuda.synchronize()               # (filled on torch's stream, which the render streams are not ordered with)
    return bufs


def fetch(rt, bufs, n, shape, what):
    """After the frames: the sentinels behind the surfaces survived -> the three surfaces as numpy arrays of `shape`."""
    import torch
    rt.sync()
    torch.cuda.synchronize()
    full = [_np(b) for b in bufs]
    assert (full[0][n:] == COLOUR_SENTINEL).all() and (full[1][n:] == COLOUR_SENTINEL).all() and (full[2][n:] == NORMAL_SENTINEL).all(), \
        f"{what}: wrote past the end of a surface"
    return [f[:n].reshape(*shape, 4) for f in full]


def render_to(rt, p, what="", stream=None):
    """One rt_render_to of p into fresh surfaces -> (colour, position, normal)."""
    n = p.regionW * p.regionH
    bufs = surfaces(n)
    rt.render_to(p, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), stream=stream)
    return fetch(rt, bufs, n, (p.regionH, p.regionW), what)


def check_on_off(rt, p, traversal, what, leaf_size=0, want=None):
    """One rt_render_to of p with the switch off (or `want`, an earlier such frame), then on: equal.  -> the off result."""
    if want is None:
        rt.set_accel_render(None)
        want = render_to(rt, p, f"{what} off")
    got = frames_on(rt, traversal, lambda: render_to(rt, p, f"{what} {traversal}"), 1, what, leaf_size)
    assert_surfaces_equal(got, want, f"{what} {traversal} leaf={leaf_size}")
    return want


def hits(off):
    """Pixels whose path hit something, from a frame's position surface."""
    return (off[1][..., :3] != 0).any(-1)


_off_frames = {}


def off_frame(rt, key, sc, p):
    """The switch-off frame of (sc, p), rendered once per module and shared by the traversals; the scene is left loaded."""
    rt.load(sc)
    if key not in _off_frames:
        rt.set_accel_render(None)
        _off_frames[key] = render_to(rt, p, f"{key} off")
    return _off_frames[key]


# ---- 1. every branch, in a scene with a real tree --------------------------------------------------------------------
@pytest.mark.parametrize("traversal", TRAVERSALS)
@pytest.mark.parametrize("leaf", [1, 4, 8])
def test_every_branch_on_off_and_oracle(rt, branches, leaf, traversal):
    sc, p, want = branches
    rt.set_variant(1)
    off = off_frame(rt, "branches", sc, p)
    assert_surfaces_equal(off, want, f"{sc.name}: rt_render_to (off) vs the oracle")
    check_on_off(rt, p, traversal, sc.name, leaf_size=leaf, want=off)
    assert hits(off).any() and (~hits(off)).any(), "the frame needs both hit and miss pixels"


def test_every_branch_on_the_device_builders_tree(rt, branches):
    sc, p, want = branches
    off = off_frame(rt, "branches", sc, p)
    rt.set_accel_builder("device")
    try:
        for traversal in TRAVERSALS:
            got = frames_on(rt, traversal, lambda: render_to(rt, p, "device builder"), 1, "device builder")
            assert rt.accel_build_info()["builder"] == "device"
            assert_surfaces_equal(got, off, f"device builder {traversal} vs off")
            assert_surfaces_equal(got, want, f"device builder {traversal} vs the oracle")
    finally:
        rt.set_accel_builder("host")


# ---- 2. tile edges and layouts ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("traversal", TRAVERSALS)
def test_windows_of_every_tile_shape(rt, branches, traversal):
    sc = branches[0]
    rt.load(sc)
    for w, h in [(1, 1), (7, 5), (8, 8), (9, 17), (63, 2), (65, 3)]:
        for x0, y0 in [(0, 0), (3, 5)]:                    # (3, 5): x0 / y0 not multiples of 8
            check_on_off(rt, window_params(sc, window=(x0, y0, w, h)), traversal, f"window {w}x{h} at ({x0}, {y0})")


@pytest.mark.parametrize("traversal", TRAVERSALS)
def test_window_across_the_image_edges_and_strips(rt, host, branches, traversal):
    sc = branches[0]
    rt.load(sc)
    # a window that crosses the right and the top edge: all-zero records outside the image
    q = window_params(sc, window=(80 - 20, 40 - 10, 40, 24))
    off = check_on_off(rt, q, traversal, "window across the edges")
    j, i = np.mgrid[0:q.regionH, 0:q.regionW]
    outside = (q.x0 + i >= q.width) | (q.y0 + j >= q.height)
    assert outside.any() and (~outside).any()
    for name, o in zip(("colour", "position", "normal"), off):
        assert (o[outside].view(np.uint16 if name == "normal" else np.uint32) == 0).all(), f"{name}: not zero outside the image"
    assert hits(off)[~outside].any()
    # equal strips, both indices
    for idx in (0, 1):
        local = host.strip_local_rows(40, 3, 2, idx)
        check_on_off(rt, window_params(sc, window=(3, 1, 70, local - 1), strips=(3, 2, idx)), traversal, f"equal strips, index {idx}")
    # unequal strips: 5 rows at offset 3 of every 8; the sixth cycle lies beyond the image
    u = window_params(sc, window=(0, 0, 80, 30), stripRows=5, stripCycleRows=8, stripOffsetRows=3)
    off = check_on_off(rt, u, traversal, "unequal strips")
    assert (off[0][25:].view(np.uint32) == 0).all() and hits(off)[:25].any()


@pytest.mark.parametrize("traversal", TRAVERSALS)
def test_render_into_image_and_render_readback(rt, host, branches, traversal):
    sc, p, want = branches
    rt.load(sc)
    W, H = p.width, p.height
    assert (W, H) == (48, 32)

    def into_image():
        """The image from two strip calls that own columns 5..44; every other pixel keeps the sentinel."""
        bufs = surfaces(W * H)
        for idx in (0, 1):
            q = L.copy_params(p, x0=5, y0=0, regionW=40, regionH=host.strip_local_rows(H, 3, 2, idx), stripRows=3, stripCount=2, stripIndex=idx)
            rt._check(rt.lib.rt_render_into_image(rt.ctx, ctypes.byref(q), *[ctypes.c_void_p(b.data_ptr()) for b in bufs], None), "rt_render_into_image")
        return fetch(rt, bufs, W * H, (H, W), "rt_render_into_image")

    rt.set_accel_render(None)
    off = into_image()
    got = frames_on(rt, traversal, into_image, 2, "rt_render_into_image")
    assert_surfaces_equal(got, off, f"rt_render_into_image {traversal}")
    owned = np.zeros((H, W), bool)
    owned[:, 5:45] = True
    assert_surfaces_equal(got, want, "rt_render_into_image vs the oracle", mask=owned)
    assert (got[0][~owned] == COLOUR_SENTINEL).all() and (got[1][~owned] == COLOUR_SENTINEL).all() and (got[2][~owned] == NORMAL_SENTINEL).all(), \
        "a pixel no call owns was written"

    def own():
        rt.render(p)
        return rt.readback()

    got = frames_on(rt, traversal, own, 1, "rt_render + rt_readback")
    assert_surfaces_equal(got, want, f"rt_render + rt_readback {traversal} vs the oracle")


# ---- 3. hostile data -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("traversal", TRAVERSALS)
def test_hostile_scene(rt, host, traversal):
    sc = scenes.Scene("hostile", A.hostile_scene(host), S.hostile_lights(), 64, 64, 4, dict(scenes.CAMERA), frame_count=3)
    p = sc.params(max_ray_depth=4)
    off = off_frame(rt, "hostile", sc, p)
    check_on_off(rt, p, traversal, "hostile", want=off)
    assert hits(off).any() and (~hits(off)).any()


# ---- 4. size ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("traversal", TRAVERSALS)
@pytest.mark.parametrize("n", [2048, 4096])
def test_lit_clouds(rt, host, n, traversal):
    sc = scenes.lit_cloud(n, n, host.generate_aabb)
    p = sc.params(width=64, height=36, max_ray_depth=3)
    off = off_frame(rt, f"lit{n}", sc, p)
    check_on_off(rt, p, traversal, sc.name, want=off)
    assert hits(off).mean() > 0.2, "the frame sees the cloud"


@pytest.mark.parametrize("traversal", ["split", "lane"])
def test_65536_spheres(rt, host, traversal):
    objs = A.cloud_scene(host, 65536, seed=3, floor=False)
    sc = scenes.Scene("spheres65536", objs, S.cloud_lights_for(65536), 64, 36, 2, dict(scenes.CAMERA))
    p = sc.params()
    off = off_frame(rt, "spheres65536", sc, p)
    check_on_off(rt, p, traversal, sc.name, want=off)
    assert hits(off).sum() >= 100


@pytest.mark.parametrize("traversal", TRAVERSALS)
def test_big_scene(rt, host, traversal):
    sc = big_scene(host)                               # 2048 objects, 70 lights
    p = sc.params(width=64, height=36)
    off = off_frame(rt, "big", sc, p)
    check_on_off(rt, p, traversal, sc.name, want=off)


# ---- 5. textures -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("traversal", TRAVERSALS)
def test_noise_texture_and_skybox(rt, host, traversal):
    base = scenes.lit_cloud(300, 11, host.generate_aabb)
    sc = scenes.Scene("lit300-textured", base.objects, base.lights, 64, 36, 4, base.camera, 2, scenes.hash_noise(64, 32, seed=8),
                      scenes.procedural_skybox(32), True)
    p = sc.params()
    p.noiseScale[0], p.noiseScale[1] = 1.0 / 64.0, 1.0 / 32.0
    assert p.useSkybox == 1
    off = off_frame(rt, "textured", sc, p)
    check_on_off(rt, p, traversal, sc.name, want=off)
    bare = scenes.Scene("lit300-bare", base.objects, base.lights, 64, 36, 4, base.camera, 2)
    q = bare.params()
    q.noiseScale[0], q.noiseScale[1] = 1.0 / 64.0, 1.0 / 32.0
    without = off_frame(rt, "untextured", bare, q)
    differs = ~((off[0] == without[0]) | (np.isnan(off[0]) & np.isnan(without[0]))).all(-1)
    assert differs[~hits(off)].any() and differs[hits(off)].any(), "the skybox and the noise texture each change some pixel"


# ---- 6. rt_frame -----------------------------------------------------------------------------------------------------
def _d2h(ptr, shape, dtype):
    import torch
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = np.empty(shape, dtype=dtype)
    torch.cuda.synchronize()
    assert hip.hipMemcpy(out.ctypes.data, ctypes.c_void_p(ptr), out.nbytes, 2) == 0      # hipMemcpyDeviceToHost
    return out


@pytest.mark.parametrize("traversal", TRAVERSALS)
def test_rt_frame(host, branches, traversal):
    """Two fresh contexts (rt_frame keeps a TAA history): three consecutive frames, the second with TAA off."""
    import torch
    sc, p, _ = branches
    h, w = p.height, p.width
    samples, noise = host.ssao_kernel()
    on, off = host.RayTracer(0), host.RayTracer(0)
    try:
        for t in (on, off):
            t.load(sc)
        on.set_accel(min_objects=1)
        on.set_accel_render(traversal=traversal, min_objects=1)
        disp = {t: torch.empty((h, w, 4), dtype=torch.float32, device="cuda") for t in (on, off)}
        for frame in range(3):
            q = L.copy_params(p, frameCount=frame)
            before = snapshot(on)
            for t in (on, off):
                t.frame(q, enable_ao=True, enable_taa=frame != 1, taa_blend=0.1, ao_samples=samples, ao_noise=noise, d_display=disp[t].data_ptr())
                t.sync()
            assert_counted(before, snapshot(on), SLOT[traversal], 1, f"rt_frame {frame}")
            a, b = on.frame_surfaces(), off.frame_surfaces()
            shapes = [((h, w, 4), np.float32), ((h, w, 4), np.float32), ((h, w, 4), np.uint16), ((h, w), np.float32), ((h, w, 4), np.float32)]
            for name, x, y, (shape, dt) in zip(("colour", "position", "normal", "AO", "history"), a, b, shapes):
                assert (x is None) == (y is None), f"frame {frame}: {name}"
                if x is not None:
                    gx, gy = _d2h(x, shape, dt), _d2h(y, shape, dt)
                    same = (gx == gy) | ((gx != gx) & (gy != gy)) if dt == np.float32 else (gx == gy)
                    assert same.all(), f"frame {frame}: {name} differs on {int((~same).sum())} values"
            gx, gy = _np(disp[on]), _np(disp[off])
            assert ((gx == gy) | (np.isnan(gx) & np.isnan(gy))).all(), f"frame {frame}: display"
    finally:
        on.close()
        off.close()


# ---- 7. switches, counters, lifecycle --------------------------------------------------------------------------------
def _state(rt):
    i = rt.accel_render_info()
    return i["active"], i["traversal"], i["min_objects"]


def packet_frame(rt, p, want, what, launch=None):
    """A frame with the switch on that must take the existing kernels: counted in launchesPacket, the off bits."""
    before = snapshot(rt)
    assert not before[0]["active"] or launch is not None, what
    got = (launch or (lambda: render_to(rt, p, what)))()
    assert_counted(before, snapshot(rt), PACKET, 1, what)
    if want is not None:
        assert_surfaces_equal(got, want, what)
    return got


def test_switches_and_lifecycle(rt, host, branches):
    sc, p, want = branches
    other = scenes.lit_cloud(300, 9, host.generate_aabb)
    q = other.params(width=48, height=32, max_ray_depth=3)
    rt.set_variant(1)
    rt.set_accel(None)
    rt.set_accel_render(None)
    want_o = off_frame(rt, "lit300", other, q)
    off_frame(rt, "branches", sc, p)
    # off by default: rt_set_accel alone changes nothing for the frames, and nothing is counted
    rt.set_accel(min_objects=1)
    i0 = snapshot(rt)
    assert _state(rt) == (False, 0, L.ACCEL_RENDER_DEFAULT_MIN_OBJECTS)
    assert_surfaces_equal(render_to(rt, p), want, "rt_set_accel alone")
    assert snapshot(rt) == i0, "a frame counts nothing while the switch is off"
    # either order of the switches gives the same state
    rt.set_accel_render(traversal="wave", min_objects=1)
    first = _state(rt)
    rt.set_accel(None)
    rt.set_accel_render(None)
    rt.set_accel_render(traversal="wave", min_objects=1)
    assert _state(rt) == (False, L.ACCEL_RENDER_WAVE, 1), "on, no tree yet"
    rt.set_accel(min_objects=1)
    assert _state(rt) == first == (True, L.ACCEL_RENDER_WAVE, 1)
    # auto resolves to one of the three; the default minObjects keeps a 256-object scene on the packet kernel
    rt.set_accel_render()
    assert _state(rt)[1] in (L.ACCEL_RENDER_LANE, L.ACCEL_RENDER_WAVE, L.ACCEL_RENDER_SPLIT)
    assert _state(rt)[2] == L.ACCEL_RENDER_DEFAULT_MIN_OBJECTS and not _state(rt)[0]
    packet_frame(rt, p, want, "default minObjects")
    # minObjects above the scene, and exactly the scene
    rt.set_accel_render(traversal="split", min_objects=len(sc.objects) + 1)
    packet_frame(rt, p, want, "below minObjects")
    rt.set_accel_render(traversal="split", min_objects=len(sc.objects))
    assert _state(rt)[0], "nObj >= minObjects"
    # rt_set_accel off: no tree
    rt.set_accel_render(traversal="split", min_objects=1)
    rt.set_accel(None)
    packet_frame(rt, p, want, "rt_set_accel off")
    rt.set_accel(min_objects=1)
    assert _state(rt)[0]
    # variant 0 and rt_count_rays keep their kernels though `active` holds
    rt.set_variant(0)
    packet_frame(rt, p, want, "variant 0", launch=lambda: render_to(rt, p, "variant 0"))
    rt.set_variant(1)
    rays = []
    packet_frame(rt, p, None, "rt_count_rays", launch=lambda: rays.append(rt.count_rays(p)))
    rt.set_accel_render(None)
    assert rays[0] == rt.count_rays(p) > 0
    # rt_last_kernel_ms after a frame through the tree
    frames_on(rt, "split", lambda: render_to(rt, p), 1, "timed")
    assert rt.last_kernel_ms() > 0.0
    # a scene change, and an identical re-upload
    rt.set_accel(min_objects=1)
    rt.set_accel_render(traversal="lane", min_objects=1)
    builds = rt.accel_info()["builds"]
    before = snapshot(rt)
    rt.load(other)
    assert rt.accel_info()["builds"] == builds + 1 and _state(rt)[0]
    assert_surfaces_equal(render_to(rt, q), want_o, "after rt_set_scene with changed bytes")
    rt.set_scene(other.objects, other.lights)
    assert rt.accel_info()["builds"] == builds + 1, "an identical re-upload rebuilds nothing"
    assert_surfaces_equal(render_to(rt, q), want_o, "after an identical re-upload")
    assert_counted(before, snapshot(rt), SLOT["lane"], 2, "scene change")
    # an all-loose scene has no tree
    loose = other.objects[:3].copy()                   # three concentric spheres: each spans most of the scene's extent
    loose["position"], loose["radius"] = (0.0, 2.0, 0.0), (1.0, 0.9, 0.8)
    host.generate_aabb(loose)
    rt.set_accel_render(None)
    rt.set_scene(loose, other.lights)
    want_l = render_to(rt, q, "all loose, off")
    rt.set_accel_render(traversal="lane", min_objects=1)
    assert not rt.accel_info()["built"] and not _state(rt)[0]
    packet_frame(rt, q, want_l, "all-loose scene")
    rt.set_accel_render(None)
    rt.set_accel(None)


def test_set_accel_render_before_any_scene(host, branches):
    sc, p, want = branches
    t = host.RayTracer(0)
    try:
        t.set_accel_render(traversal="split", min_objects=1)
        t.set_accel(min_objects=1)
        assert _state(t) == (False, L.ACCEL_RENDER_SPLIT, 1)
        t.load(sc)
        assert _state(t)[0]
        before = snapshot(t)
        got = render_to(t, p, "fresh context")
        assert_counted(before, snapshot(t), SLOT["split"], 1, "fresh context")
        assert_surfaces_equal(got, want, "switch set before any scene vs the oracle")
    finally:
        t.close()


def test_first_hit_cache_is_left_as_found(host, branches):
    """With reuse on (the default) and a still view: normal, record, then a frame through the tree, then the replay the cache was
    ready for -- as if the frame in between had not happened."""
    sc, p, want = branches
    t = host.RayTracer(0)
    try:
        t.load(sc)
        t.set_accel(min_objects=1)
        modes = []
        for k in range(5):
            c0 = t.debug_first_hit()
            if k == 2:
                got = frames_on(t, "split", lambda: render_to(t, p, "between"), 1, "between two packet frames")
                t.set_accel(min_objects=1)
            else:
                got = render_to(t, p, f"packet frame {k}")
            modes.append([int(a - b) for a, b in zip(t.debug_first_hit(), c0)])
            assert_surfaces_equal(got, want, f"frame {k} vs the oracle")
        assert modes == [[1, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, 1], [0, 0, 1]], f"(normal, record, replay) per frame: {modes}"
    finally:
        t.close()


def test_refusals(rt, host, branches):
    sc, p, want = branches
    lib, ctx = rt.lib, rt.ctx
    rt.load(sc)
    rt.set_accel(min_objects=1)
    rt.set_accel_render(traversal="wave", min_objects=1)
    before = rt.accel_render_info()
    assert lib.rt_accel_render_info(ctx, None) == -1, "NULL report"
    assert lib.rt_accel_render_info(None, ctypes.byref(L.RtAccelRenderReport())) == -1, "NULL context"
    assert lib.rt_set_accel_render(None, None) == -1, "NULL context"
    assert rt.accel_render_info() == before
    for bad in (dict(traversal=4), dict(traversal=-1), dict(min_objects=-1)):
        with pytest.raises(host.RtError):
            rt.set_accel_render(**bad)
        assert rt.accel_render_info() == before, f"{bad}: a refused call changes nothing"
    for k in range(5):
        d = L.make_accel_render_desc()
        d.reserved[k] = 1
        assert lib.rt_set_accel_render(ctx, ctypes.byref(d)) == -1, f"reserved[{k}]"
        assert rt.accel_render_info() == before, f"reserved[{k}]: a refused call changes nothing"
    # rt_accel_traversal keeps its three values
    for setter in (rt.set_accel, rt.set_accel_shading):
        with pytest.raises(host.RtError):
            setter(traversal=L.ACCEL_RENDER_SPLIT)
    i0 = snapshot(rt)
    assert_surfaces_equal(render_to(rt, p, "after the refusals"), want, "the context stays usable")
    assert_counted(i0, snapshot(rt), SLOT["wave"], 1, "after the refusals")
    d = L.make_accel_render_desc(False, "wave", 5)
    assert lib.rt_set_accel_render(ctx, ctypes.byref(d)) == 0 and rt.accel_render_info()["traversal"] == 0, "enable == 0: off"
    rt.set_accel(None)


# ---- 8. ordering -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("traversal", TRAVERSALS)
def test_frames_on_a_foreign_stream_across_scene_updates(rt, host, traversal):
    """Eight rt_set_scene calls of a moving cloud, each followed by a frame on a foreign stream, with no host wait in between: the
    re-upload of the scene and of its tree waits for the frame in flight, and the frame issued behind it walks the new tree."""
    import torch
    base = scenes.lit_cloud(300, 21, host.generate_aabb)
    p = base.params(width=128, height=72, max_ray_depth=3)
    n = p.regionW * p.regionH
    moved = []
    for k in range(8):
        objs = base.objects.copy()
        objs["position"][:300, 0] += 0.4 * k
        host.generate_aabb(objs)
        moved.append(objs)
    rt.set_accel(None)
    rt.set_accel_render(None)
    rt.load(base)
    want = []
    for objs in moved:
        rt.set_scene(objs, base.lights)
        want.append(render_to(rt, p, "off"))
    assert not all(np.array_equal(want[0][0], w[0]) for w in want[1:]), "the cloud moves"
    rt.set_accel(min_objects=1)
    rt.set_accel_render(traversal=traversal, min_objects=1)
    bufs = [surfaces(n) for _ in moved]
    s = torch.cuda.Stream()
    before = snapshot(rt)
    torch.cuda.synchronize()
    for objs, b in zip(moved, bufs):
        rt.set_scene(objs, base.lights)
        rt.render_to(p, b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    after = snapshot(rt)
    rt.set_accel_render(None)
    rt.set_accel(None)
    assert_counted(before, after, SLOT[traversal], 8, "foreign stream")
    for k, b in enumerate(bufs):
        assert_surfaces_equal(fetch(rt, b, n, (p.regionH, p.regionW), f"scene {k}"), want[k], f"{traversal}: the frame of scene {k}")
