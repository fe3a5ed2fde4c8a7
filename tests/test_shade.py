"""GPU tests of ray shading (rt_shade_rays; include/rt_mi355.h).

* Camera identity: shading rt_camera_rays(p) with pixels=None reproduces rt_render_to(p) bit for bit on all three surfaces
  -- through both render kernel variants (conftest's `tracer`), over the configs, windows, strips, depths, frame counts,
  noise and skybox.  The render surfaces are pinned to the oracle, so this pins shading to it.
* Arbitrary rays against the oracle: a ray (o, d) shaded as pixel (x, y) is the oracle's pixel (x, y) of a degenerate
  camera (camPos = o, camDir = d, camRight = camUp = 0) whose generateCameraRay gives exactly (o, normalize(d)).
* The primary segment's tMax, order independence and launch sizes, scenes beyond the exhaustive kernel's caps, errors,
  and ordering against scene / texture updates on torch streams.
"""
import ctypes

import numpy as np
import pytest

from conftest import bits_equal
from opengl_raytracing_amd import layout as L
from opengl_raytracing_amd import scenes

pytestmark = pytest.mark.gpu

F = np.float32
INT_MAX = 2 ** 31 - 1


def _np(t):
    return None if t is None else t.cpu().numpy()


def render_surfaces(tracer, p):
    tracer.render(p)
    return tracer.readback()


def shade_camera(tracer, p, pixels=None):
    import torch
    rays = tracer.camera_rays(p)
    col, pos, nrm = tracer.shade_rays(p, rays, pixels=pixels)
    torch.cuda.current_stream().synchronize()
    return _np(col), _np(pos), _np(nrm)


def assert_surfaces_equal(got, want, what, mask=None):
    for name, g, w in zip(("colour", "position", "normal"), got, want):
        g = g.reshape(w.shape)
        if name == "normal":
            g, w = g.view(np.uint16), w.view(np.uint16)
        if mask is not None:
            g, w = g[mask], w[mask]
        same = (g == w) | (np.isnan(g) & np.isnan(w)) if name != "normal" else (g == w)
        assert same.all(), f"{what}: {name} differs on {int((~same).reshape(-1, 4).any(-1).sum())} pixels"


def surface_pixels(p):
    """(x, y) of the image pixel rt_render_to(p) writes at each surface index, and whether it is inside the image."""
    cyc = p.stripCycleRows if p.stripCycleRows > 0 else p.stripRows * p.stripCount
    off = p.stripOffsetRows if p.stripCycleRows > 0 else p.stripIndex * p.stripRows
    j, i = np.mgrid[0:p.regionH, 0:p.regionW]
    gx = p.x0 + i
    ly = p.y0 + j
    gy = (ly // p.stripRows) * cyc + off + ly % p.stripRows
    inside = (gx < p.width) & (gy < p.height)
    return np.stack([gx, gy], -1).astype(np.uint32), inside


def check_camera_identity(tracer, p, what, explicit=True):
    import torch
    want = render_surfaces(tracer, p)
    assert_surfaces_equal(shade_camera(tracer, p), want, f"{what} (pixels=None)")
    if explicit:
        px, inside = surface_pixels(p)
        d = torch.from_numpy(px.view(np.int32).copy()).cuda()
        assert_surfaces_equal(shade_camera(tracer, p, d), want, f"{what} (explicit pixels)", mask=inside)


# ---- 1. camera identity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5])
def test_camera_rays_shade_to_the_rendered_frame(tracer, host, cfg):
    sc = scenes.make_scene(cfg, host.generate_aabb)
    tracer.load(sc)
    for depth in (0, 1, 3, 4, 6):
        for fc in ((0, 71) if depth >= 3 else (5,)):
            sc.frame_count = fc
            p = sc.params(width=192, height=108, max_ray_depth=depth)
            check_camera_identity(tracer, p, f"C{cfg} depth={depth} fc={fc}")
    # noise and skybox toggled (the scene's own state is restored by the next load)
    sc.frame_count = 9
    rng = np.random.default_rng(cfg)
    faces = rng.uniform(0, 2, (6, 16, 16, 3)).astype(np.float16)
    for noise in (None, scenes.hash_noise(64, 32, seed=cfg)):
        tracer.set_noise(noise)
        for sky in (0, 1):
            tracer.set_skybox(faces if sky else None)
            p = sc.params(width=160, height=90, max_ray_depth=4)
            p.useSkybox = sky
            p.noiseScale[0], p.noiseScale[1] = 1.0 / 64.0, 1.0 / 32.0
            check_camera_identity(tracer, p, f"C{cfg} noise={noise is not None} sky={sky}")
    tracer.load(sc)
    # full-resolution windows crossing the image's right / top edge
    for win in ((sc.width - 64, sc.height // 2, 96, 48), (sc.width // 3, sc.height - 20, 64, 40)):
        check_camera_identity(tracer, sc.params(window=win, max_ray_depth=3), f"C{cfg} window {win}")


def test_full_c2_frame_and_nan_scene(tracer, host):
    sc = scenes.make_scene(2, host.generate_aabb)
    tracer.load(sc)
    check_camera_identity(tracer, sc.params(), "C2 1920x1080", explicit=False)
    sc = scenes.nan_parity_scene(host.generate_aabb)
    tracer.load(sc)
    for fc in (0, 3):
        for depth in (1, 4, 6):
            sc.frame_count = fc
            check_camera_identity(tracer, sc.params(max_ray_depth=depth), f"nan scene fc={fc} depth={depth}")


def test_window_and_strip_layouts(tracer, host):
    sc = scenes.make_scene(3, host.generate_aabb)          # noise texture + PCSS: the pixel matters
    tracer.load(sc)
    W, H = 200, 120
    cases = [dict(window=(17, 9, 64, 33)), dict(window=(150, 100, 80, 40)), dict(strips=(8, 3, 1)), dict(strips=(4, 2, 0)),
             dict(strips=(8, 3, 2), window=(5, 3, 150, 20)), dict(cycle=(6, 16, 4)), dict(cycle=(8, 24, 0), window=(0, 1, 190, 30))]
    for cs in cases:
        if "cycle" in cs:
            rows, cyc, off = cs["cycle"]
            local = -(-H // cyc) * rows
            p = sc.params(width=W, height=H, window=cs.get("window", (0, 0, W, local)), strips=(rows, 1, 0), max_ray_depth=4)
            p.stripCycleRows, p.stripOffsetRows = cyc, off
        else:
            rows, cnt, idx = cs["strips"] if "strips" in cs else (1, 1, 0)
            local = host.strip_local_rows(H, rows, cnt, idx)
            p = sc.params(width=W, height=H, window=cs.get("window", (0, 0, W, local)), strips=(rows, cnt, idx), max_ray_depth=4)
        check_camera_identity(tracer, p, f"layout {cs}")


# ---- 2. arbitrary rays against the oracle ---------------------------------------------------------------------------
def hostile_rays(sc, n, rng):
    """Origins anywhere / inside spheres / on objects' centres (planes: on the plane) / at 1e4-1e6; directions with zero
    components, unnormalised and axis-aligned; pixel ids up to 2^32 - 1."""
    objs = sc.objects
    o = rng.uniform(-10, 10, (n, 3)).astype(F)
    kind = rng.integers(0, 5, n)
    if len(objs):
        k = rng.integers(0, len(objs), n)
        cen = objs["position"][k].astype(F)
        sel = kind == 1
        o[sel] = cen[sel] + (rng.uniform(-0.5, 0.5, (int(sel.sum()), 3)) * objs["radius"][k][sel, None]).astype(F)
        sel = kind == 2
        o[sel] = cen[sel]
    sel = kind == 3
    o[sel] = (rng.uniform(-1, 1, (int(sel.sum()), 3)) * 10.0 ** rng.uniform(4, 6, (int(sel.sum()), 1))).astype(F)
    d = rng.normal(size=(n, 3)).astype(F)
    if len(objs):
        k = rng.integers(0, len(objs), n)
        aim = rng.random(n) < 0.6
        d[aim] = (objs["position"][k].astype(F) + rng.normal(scale=0.5, size=(n, 3)).astype(F) - o)[aim]
    dk = rng.integers(0, 6, n)
    ax = rng.integers(0, 3, n)
    d[dk == 1, ax[dk == 1]] = 0.0
    d[dk == 2] = 0.0
    d[dk == 2, ax[dk == 2]] = rng.choice([-1.0, 1.0, 3.5], int((dk == 2).sum()))
    d[dk == 3] *= F(1e3)
    d[dk == 4, ax[dk == 4]] = F(-0.0)
    pk = rng.integers(0, 4, (n, 2))
    px = np.where(pk == 0, rng.integers(0, 4096, (n, 2)),
                  np.where(pk == 1, rng.integers(0, INT_MAX - 1, (n, 2)),
                           np.where(pk == 2, rng.integers(2 ** 31, 2 ** 32, (n, 2)), 2 ** 32 - 1 - rng.integers(0, 3, (n, 2)))))
    return o, d, px.astype(np.uint64)


def degenerate_params(sc, o, d, px, depth, noise_scale):
    """The oracle's window (x0, y0) and a valid rt_params for rt_camera_rays whose generateCameraRay is (o, normalize(d)) with
    the same signs of zero: camRight = camUp = +0 and ux, uy of the same sign in both (pixel ids >= 2^31 are negative x0 /
    y0 in the oracle, which reads them as uint32; their ux, uy < 0 like pixel 0's)."""
    p = sc.params(width=INT_MAX, height=INT_MAX, window=(0, 0, 1, 1), max_ray_depth=depth)
    p.camPos[:] = o
    p.camDir[:] = d
    p.camRight[:] = (0.0, 0.0, 0.0)
    p.camUp[:] = (0.0, 0.0, 0.0)
    p.noiseScale[0], p.noiseScale[1] = noise_scale
    q = L.copy_params(p)
    ox, oy = (int(v) if v < 2 ** 31 else int(v) - 2 ** 32 for v in px)
    q.x0, q.y0 = ox, oy
    p.x0, p.y0 = max(ox, 0), max(oy, 0)
    return p, q


def check_against_oracle(tracer, oracle, sc, n, seed, depth=None):
    import torch
    rng = np.random.default_rng(seed)
    tracer.load(sc)
    depth = sc.max_ray_depth if depth is None else depth
    ns = (1.0 / 64.0, 1.0 / 32.0) if sc.noise is not None else (1.0 / 1024.0, 1.0 / 1024.0)
    o, d, px = hostile_rays(sc, n, rng)
    rays, want = [], []
    for k in range(n):
        p, q = degenerate_params(sc, o[k], d[k], px[k], depth, ns)
        rays.append(tracer.camera_rays(p).reshape(1, 8))
        c, ps, nr, _ = oracle.render(sc, q)
        want.append((c.reshape(4), ps.reshape(4), nr.reshape(4)))
    p0 = degenerate_params(sc, o[0], d[0], px[0], depth, ns)[0]
    rays = torch.cat(rays)
    pix = torch.from_numpy(px.astype(np.uint32).view(np.int32).reshape(n, 2)).cuda()
    got = [_np(t) for t in tracer.shade_rays(p0, rays, pixels=pix)]
    wc, wp, wn = (np.stack(w) for w in zip(*want))
    assert_surfaces_equal(got, (wc, wp, wn), f"{sc.name}: {n} rays vs the oracle")


@pytest.mark.parametrize("which", ["C2", "C3", "C4", "nan"])
def test_arbitrary_rays_match_the_oracle(tracer, host, oracle, which):
    sc = scenes.nan_parity_scene(host.generate_aabb) if which == "nan" else scenes.make_scene(int(which[1]), host.generate_aabb)
    sc.frame_count = 13
    check_against_oracle(tracer, oracle, sc, 768, seed={"C2": 2, "C3": 3, "C4": 4, "nan": 9}[which])
    if which != "nan":
        check_against_oracle(tracer, oracle, sc, 256, seed=7, depth=6)


def test_arbitrary_rays_in_fuzzed_scenes_match_the_oracle(tracer, host, oracle):
    from test_gpu_parity import _fuzz_scene
    for seed in range(24):
        check_against_oracle(tracer, oracle, _fuzz_scene(seed), 160, seed=500 + seed)


# ---- 3. tMax on the primary segment ---------------------------------------------------------------------------------
def test_primary_segment_ends_at_tmax(tracer, host, oracle):
    import torch
    for cfg in (2, 4):
        sc = scenes.make_scene(cfg, host.generate_aabb)
        tracer.load(sc)
        faces = np.random.default_rng(cfg).uniform(0, 2, (6, 16, 16, 3)).astype(np.float16)
        tracer.set_skybox(faces)
        n = 1 << 14
        rng = np.random.default_rng(40 + cfg)
        o, d, _ = hostile_rays(sc, n, rng)
        tmax = rng.uniform(0, 30, n).astype(F)
        tk = rng.integers(0, 6, n)
        tmax[tk == 1] = 0.0
        tmax[tk == 2] = -rng.uniform(0, 10, int((tk == 2).sum()))
        tmax[tk == 3] = np.nan
        tmax[tk == 4] = np.inf
        r = np.zeros(n, L.RAY_DTYPE)
        r["origin"], r["direction"], r["tMax"] = o, d, tmax
        rays = torch.from_numpy(r.view(np.float32).reshape(n, 8).copy()).cuda()
        pix = torch.from_numpy(rng.integers(0, 2 ** 32, (n, 2), dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()
        hits = tracer.trace_rays(rays, "closest").cpu().numpy().view(L.HIT_DTYPE).reshape(n)
        for sky in (0, 1):
            p = sc.params(width=64, height=64, max_ray_depth=1)
            p.useSkybox = sky
            col, pos, nrm = (_np(t) for t in tracer.shade_rays(p, rays, pixels=pix))
            assert bits_equal(pos[:, :3], hits["position"]), f"C{cfg}: position != rt_trace_rays CLOSEST"
            assert (pos[:, 3] == 1.0).all() and (col[:, 3] == 1.0).all()
            n16 = oracle.float_to_half_rtz(hits["normal"])
            both_nan = np.isnan(hits["normal"]) & np.isnan(nrm[:, :3].astype(F))
            assert ((nrm[:, :3].view(np.uint16) == n16) | both_nan).all(), f"C{cfg}: normal != fp16-RTZ of the hit normal"
            miss = hits["object"] < 0
            want = oracle.sample_cube(faces, d[miss]) if sky else np.zeros((int(miss.sum()), 3), F)
            assert bits_equal(col[miss, :3], want.astype(F)), f"C{cfg} sky={sky}: miss colour"
            assert miss.any() and (~miss).any()


# ---- 4. order independence, sizes, optional outputs -----------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2 ** 20 + 3])
def test_order_independence_and_sizes(tracer, host, n):
    import torch
    sc = scenes.make_scene(3, host.generate_aabb)
    tracer.load(sc)
    rng = np.random.default_rng(n)
    o, d, px = hostile_rays(sc, n, rng)
    r = np.zeros(n, L.RAY_DTYPE)
    r["origin"], r["direction"], r["tMax"] = o, d, 114514.0
    rays = torch.from_numpy(r.view(np.float32).reshape(n, 8).copy()).cuda()
    pix = torch.from_numpy(px.astype(np.uint32).view(np.int32).reshape(n, 2)).cuda()
    p = sc.params(width=64, height=64)
    sentinel = 12345.0
    outs = (torch.full((n + 64, 4), sentinel, dtype=torch.float32, device="cuda"),
            torch.full((n + 64, 4), sentinel, dtype=torch.float32, device="cuda"),
            torch.full((n + 64, 4), 7.0, dtype=torch.float16, device="cuda"))
    tracer.shade_rays(p, rays, pixels=pix, out=tuple(t[:n] for t in outs))
    full = [_np(t) for t in outs]
    assert (full[0][n:] == sentinel).all() and (full[1][n:] == sentinel).all() and (full[2][n:] == 7.0).all(), "wrote past the last ray"
    base = [f[:n] for f in full]
    perm = torch.from_numpy(rng.permutation(n)).cuda()
    got = [_np(t) for t in tracer.shade_rays(p, rays[perm].contiguous(), pixels=pix[perm].contiguous())]
    pn = perm.cpu().numpy()
    assert_surfaces_equal(got, [b[pn] for b in base], f"n={n} permuted")
    col_only, no_pos, no_nrm = tracer.shade_rays(p, rays, pixels=pix, position=False, normal=False)
    assert no_pos is None and no_nrm is None
    assert bits_equal(_np(col_only), base[0]), f"n={n}: colour changed without position / normal outputs"


# ---- 5. beyond the exhaustive kernel's caps -------------------------------------------------------------------------
def big_scene(host):
    rng = np.random.default_rng(2048)
    base = scenes.make_scene(2, host.generate_aabb)
    n, nl = 2048, 70
    objs = L.default_objects(n)
    objs[:len(base.objects)] = base.objects
    m = n - len(base.objects)
    extra = objs[len(base.objects):]
    extra["type"] = rng.choice([0, 0, 0, 1], m)
    extra["position"] = np.stack([rng.uniform(-9, 9, m), rng.uniform(0, 6, m), rng.uniform(-12, 2, m)], -1)
    extra["radius"] = rng.uniform(0.05, 0.3, m)
    extra["normal"] = rng.normal(size=(m, 3))
    extra["size"] = rng.uniform(0.2, 1.0, (m, 2))
    extra["albedo"] = rng.uniform(0.2, 1, (m, 3))
    extra["metallic"] = rng.choice([0.0, 1.0], m)
    extra["roughness"] = rng.choice([0.05, 0.5, 1.0], m)
    extra["diffuseStrength"] = rng.choice([0.0, 0.6, 1.0], m)
    extra["transparency"] = rng.choice([0.0, 0.0, 0.9], m)
    extra["ior"] = rng.choice([1.0, 1.5], m)
    extra["subsurfaceScatter"] = rng.choice([0.0, 0.0, 0.0, 0.5], m)
    objs[len(base.objects):] = extra
    host.generate_aabb(objs)
    lts = L.default_lights(nl)
    lts["type"] = rng.integers(0, 3, nl)
    lts["position"] = np.stack([rng.uniform(-8, 8, nl), rng.uniform(3, 8, nl), rng.uniform(-10, 2, nl)], -1)
    lts["direction"] = rng.normal(size=(nl, 3))
    lts["intensity"] = rng.uniform(0.5, 5, nl)
    lts["shadowType"] = rng.choice([0, 1, 1, 2], nl)
    lts["pcfSamples"] = rng.choice([1, 2, 4], nl)
    return scenes.Scene("big2048x70", objs, lts, 128, 72, 3, dict(scenes.CAMERA), frame_count=3)


def test_scene_beyond_the_exhaustive_caps(host, oracle):
    import torch
    sc = big_scene(host)
    rt = host.RayTracer(0)
    try:
        rt.set_variant(1)
        rt.load(sc)
        p = sc.params()
        check_camera_identity(rt, p, "2048 objects / 70 lights vs the packet render", explicit=False)
        q = sc.params(window=(40, 20, 32, 32))
        got = shade_camera(rt, q)
        want = oracle.render(sc, q)[:3]
        assert_surfaces_equal(got, want, "2048 objects / 70 lights, 32x32 window vs the oracle")
        torch.cuda.synchronize()
    finally:
        rt.close()


# ---- 6. errors ------------------------------------------------------------------------------------------------------
def test_shade_errors(host):
    import torch
    rt = host.RayTracer(0)
    try:
        lib, ctx = rt.lib, rt.ctx
        sc = scenes.make_scene(1, host.generate_aabb)
        p = sc.params(width=8, height=8)
        d = torch.zeros((64, 8), dtype=torch.float32, device="cuda")
        c = torch.zeros((64 + 4, 4), dtype=torch.float32, device="cuda")
        nb = torch.zeros((64 + 4, 4), dtype=torch.float16, device="cuda")
        px = torch.zeros((64 + 2, 2), dtype=torch.int32, device="cuda")
        v = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
        P = ctypes.byref(p)
        assert lib.rt_shade_rays(ctx, P, v(d), None, 64, v(c), v(c), v(nb), None) == -1, "no scene set"
        rt.load(sc)
        assert lib.rt_shade_rays(ctx, P, v(d), None, 64, v(c), v(c), v(nb), None) == 0
        assert lib.rt_shade_rays(ctx, P, v(d), v(px), 64, v(c), None, None, None) == 0
        assert lib.rt_shade_rays(ctx, P, None, None, 64, v(c), None, None, None) == -1, "NULL rays"
        assert lib.rt_shade_rays(ctx, P, v(d), None, 64, None, None, None, None) == -1, "NULL colour"
        assert lib.rt_shade_rays(ctx, P, v(d, 4), v(px), 63, v(c), None, None, None) == -1, "misaligned rays"
        assert lib.rt_shade_rays(ctx, P, v(d), v(px, 4), 63, v(c), None, None, None) == -1, "misaligned pixels"
        assert lib.rt_shade_rays(ctx, P, v(d), v(px), 63, v(c, 8), None, None, None) == -1, "misaligned colour"
        assert lib.rt_shade_rays(ctx, P, v(d), v(px), 63, v(c), v(c, 4), None, None) == -1, "misaligned position"
        assert lib.rt_shade_rays(ctx, P, v(d), v(px), 63, v(c), None, v(nb, 2), None) == -1, "misaligned normal"
        assert lib.rt_shade_rays(ctx, P, v(d), v(px, 8), 63, v(c, 16), v(c, 16), v(nb, 8), None) == 0, "8 / 16-byte offsets are fine"
        assert lib.rt_shade_rays(ctx, P, v(d), None, 63, v(c), None, None, None) == -1, "pixels=NULL with nRays != regionW*regionH"
        bad = L.copy_params(p)
        bad.maxRayDepth = 33
        assert lib.rt_shade_rays(ctx, ctypes.byref(bad), v(d), v(px), 64, v(c), None, None, None) == -1, "maxRayDepth 33"
        assert lib.rt_shade_rays(ctx, None, v(d), v(px), 64, v(c), None, None, None) == -1, "NULL params"
        assert lib.rt_shade_rays(ctx, P, None, v(px), 0, None, None, None, None) == 0, "nRays == 0 is a no-op"
        assert lib.rt_shade_rays(ctx, P, v(d), None, 2 ** 40, v(c), None, None, None) == -1, "pixels=NULL with a wrong count"
        assert lib.rt_shade_rays(ctx, P, v(d), v(px), 2 ** 40, v(c), None, None, None) == -4, "above the grid limit"
        with pytest.raises(ValueError):
            rt.shade_rays(p, d[:63])
        torch.cuda.synchronize()
    finally:
        rt.close()


# ---- 7. ordering ----------------------------------------------------------------------------------------------------
def test_side_stream_sees_scene_noise_and_skybox_updates(tracer, host):
    import torch
    A = scenes.make_scene(2, host.generate_aabb)
    B = scenes.make_scene(3, host.generate_aabb)
    p = B.params(width=96, height=64, max_ray_depth=4)
    p.useSkybox = 1
    faces = np.random.default_rng(3).uniform(0, 2, (6, 16, 16, 3)).astype(np.float16)
    # the reference answer: B, its noise and this skybox, rendered
    tracer.load(B)
    tracer.set_skybox(faces)
    want = render_surfaces(tracer, p)
    tracer.load(A)
    tracer.set_skybox(None)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    tracer.set_scene(B.objects, B.lights)
    tracer.set_noise(B.noise)
    tracer.set_skybox(faces)
    with torch.cuda.stream(s):
        rays = tracer.camera_rays(p, stream=s)
        got = tracer.shade_rays(p, rays, stream=s)
    s.synchronize()
    assert_surfaces_equal([_np(t) for t in got], want, "side stream after set_scene / set_noise / set_skybox")


def test_set_scene_during_a_large_shade_leaves_it_unchanged(tracer, host):
    import torch
    A = scenes.make_scene(4, host.generate_aabb)
    B = scenes.make_scene(2, host.generate_aabb)
    p = A.params(width=1024, height=1024, max_ray_depth=4)
    tracer.load(A)
    want = render_surfaces(tracer, p)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rays = tracer.camera_rays(p, stream=s)
        got = tracer.shade_rays(p, rays, stream=s)
    tracer.set_scene(B.objects, B.lights)                  # issued while the shade is in flight
    s.synchronize()
    assert_surfaces_equal([_np(t) for t in got], want, "shade in flight across rt_set_scene")
    with torch.cuda.stream(s):
        after = tracer.shade_rays(p, tracer.camera_rays(p, stream=s), stream=s)
    s.synchronize()
    assert_surfaces_equal([_np(t) for t in after], render_surfaces(tracer, p), "shade after rt_set_scene sees the new scene")


# ---- 8. every branch of the per-lane path tracer, through both of its scene accessors at once ------------------------
def branch_scene(host, directional_pcf_samples):
    """Six objects (diffuse floor, diffuse / mirror / glass / subsurface spheres, a mirror wall) under a point light with 70
    PCF samples (past the Halton tables' 64 entries), a directional PCF light, a PCSS area light and a light of shadowType 3
    (calculateShadow's fall-through: always shadowed); noise texture and skybox bound."""
    o = L.default_objects(6)
    o["diffuseStrength"] = 0.0
    o[0]["type"] = L.PLANE
    o[0]["position"], o[0]["normal"], o[0]["size"] = (0.0, -1.0, -4.0), (0.0, 1.0, 0.0), (40.0, 40.0)
    o[0]["albedo"], o[0]["roughness"], o[0]["diffuseStrength"] = (0.8, 0.7, 0.6), 0.6, 0.5
    o[1]["position"], o[1]["radius"] = (-3.0, 0.5, -3.0), 1.2                                    # diffuse
    o[1]["albedo"], o[1]["roughness"], o[1]["diffuseStrength"] = (0.9, 0.3, 0.2), 0.8, 0.8
    o[2]["position"], o[2]["radius"] = (0.0, 1.0, -5.0), 1.5                                     # mirror
    o[2]["albedo"], o[2]["metallic"], o[2]["roughness"] = (0.9, 0.9, 0.95), 1.0, 0.05
    o[3]["position"], o[3]["radius"] = (3.0, 0.5, -2.0), 1.2                                     # glass
    o[3]["albedo"], o[3]["roughness"], o[3]["ior"], o[3]["transparency"] = (0.9, 1.0, 0.9), 0.05, 1.5, 0.95
    o[4]["position"], o[4]["radius"] = (-0.5, 0.0, 0.5), 0.9                                     # subsurface
    o[4]["albedo"], o[4]["diffuseStrength"] = (0.8, 0.6, 0.5), 0.6
    o[4]["subsurfaceScatter"], o[4]["subsurfaceColor"], o[4]["scatterDistance"] = 0.5, (1.0, 0.6, 0.5), 0.8
    o[5]["type"] = L.PLANE
    o[5]["position"], o[5]["normal"], o[5]["size"] = (-4.0, 1.5, -9.0), (0.0, 0.0, 1.0), (6.0, 5.0)
    o[5]["albedo"], o[5]["roughness"] = (0.7, 0.75, 0.8), 0.4
    host.generate_aabb(o)
    lt = L.default_lights(4)
    lt[0]["type"], lt[0]["position"], lt[0]["intensity"] = L.POINT, (0.0, 6.0, -3.0), 8.0
    lt[0]["shadowType"], lt[0]["pcfSamples"] = L.SHADOW_PCF, 70
    lt[1]["type"], lt[1]["direction"], lt[1]["intensity"] = L.DIRECTIONAL, (0.5, -1.0, -0.5), 3.0
    lt[1]["shadowType"], lt[1]["pcfSamples"] = L.SHADOW_PCF, directional_pcf_samples
    lt[2]["type"], lt[2]["position"], lt[2]["direction"], lt[2]["intensity"] = L.AREA, (3.0, 8.0, -6.0), (0.0, 1.0, 0.0), 40.0
    lt[2]["shadowType"], lt[2]["pcfSamples"] = L.SHADOW_PCSS, 4
    lt[3]["type"], lt[3]["position"], lt[3]["intensity"] = L.POINT, (-4.0, 5.0, 2.0), 4.0
    lt[3]["shadowType"] = 3
    return scenes.Scene(f"branches-pcf{directional_pcf_samples}", o, lt, 48, 32, 6, dict(scenes.CAMERA), frame_count=5,
                        noise=scenes.hash_noise(64, 32, seed=8), skybox=scenes.procedural_skybox(32), use_skybox=True)


def branch_params(sc, depth):
    p = sc.params(max_ray_depth=depth)
    p.noiseScale[0], p.noiseScale[1] = 1.0 / 64.0, 1.0 / 32.0
    return p


@pytest.mark.parametrize("directional_pcf_samples", [0, 3])
def test_every_branch_through_both_accessors(host, oracle, directional_pcf_samples):
    """One 48x32 frame at depth 6: exhaustive render == rt_shade_rays(rt_camera_rays) == packet render == oracle, bit for
    bit on colour, position and normal.  The exhaustive kernel and rt_shade_rays run the same per-lane tracer
    (csrc/rt_lane.inc) over the LDS and the scalar-load accessor.
    pcfSamples 0 on the directional light makes pcfShadow return 0/0, so every hit pixel's colour is NaN at every depth
    (774 of the 1536 pixels in the oracle's frame) and no colour can differ between two depths: that frame shows the deeper
    bounces by the positions that differ instead (21 pixels), and the same scene with 3 samples on that light carries the
    colour check (54 pixels differ between depth 3 and 6)."""
    import torch
    sc = branch_scene(host, directional_pcf_samples)
    p = branch_params(sc, 6)
    want = oracle.render(sc, p)[:3]
    shallow = oracle.render(sc, branch_params(sc, 3))[:3]
    # the oracle's frame alone: not empty, not flat, and bounces past the third matter
    hit = (want[1][..., :3] != 0).any(-1)
    assert hit.any() and (~hit).any(), "the frame needs both hit and miss pixels"
    assert len(np.unique(want[0][..., :3].reshape(-1, 3).view(np.uint32), axis=0)) >= 100, "fewer than 100 distinct colours"
    differs = lambda a, b: (~((a == b) | (np.isnan(a) & np.isnan(b)))).any(-1)
    if directional_pcf_samples == 0:
        assert np.isnan(want[0][hit][:, :3]).all() and not np.isnan(want[0][~hit]).any(), "0/0 shadow factor: NaN on every hit"
        assert differs(want[1], shallow[1]).any(), "no pixel's position differs between maxRayDepth 3 and 6"
    else:
        assert not np.isnan(want[0]).any()
        assert differs(want[0], shallow[0]).any(), "no pixel's colour differs between maxRayDepth 3 and 6"
    rt = host.RayTracer(0)
    try:
        rt.load(sc)
        for variant, name in ((0, "exhaustive render"), (1, "packet render")):
            rt.set_variant(variant)
            assert_surfaces_equal(render_surfaces(rt, p), want, f"{sc.name}: {name} vs the oracle")
            assert_surfaces_equal(shade_camera(rt, p), want, f"{sc.name}: rt_shade_rays(rt_camera_rays) vs the oracle")
        torch.cuda.synchronize()
    finally:
        rt.close()
