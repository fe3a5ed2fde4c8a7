"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI,
against the CPU oracle on the same inputs and against the committed reference fixtures.

Bars:
* HIP vs oracle: BIT-EXACT on all three surfaces and an identical ray count -- both evaluate
  the same fp32 expression tree (no FMA contraction, IEEE div/sqrt, shared deterministic
  sin/exp/pow5), so any difference is a kernel bug.
* HIP vs reference fixture (llvmpipe runs of the reference GLSL, low-res frames, full-resolution windows and
  7680x4320 windows): gPosition / gNormal BIT-EXACT, gColor within 1e-4 relative on >= 99.9 % of pixels
  (REF_GATES below; the host and the kernel evaluate tan / sin / cos / exp as the reference's GL does).
"""
import ctypes

import os

import numpy as np
import pytest

from conftest import GoldenScene, bits_equal, compare_surface, load_golden, params_from_bytes
from opengl_raytracing_amd import layout as L
from opengl_raytracing_amd import scenes

pytestmark = pytest.mark.gpu


def render_gpu(tracer, sc, p):
    tracer.load(sc)
    tracer.render(p)
    return tracer.readback()


def assert_bit_exact(gpu, cpu, what=""):
    col, pos, nrm = gpu
    oc, op, on = cpu[:3]
    assert bits_equal(col, oc), f"{what}: gColor differs on {int((~compare_surface(col, oc, 0, 0)['exact_mask']).sum())} px"
    assert bits_equal(pos, op), f"{what}: gPosition differs"
    nan_n = np.isnan(nrm.astype(np.float32)) & np.isnan(on.astype(np.float32))
    assert ((nrm.view(np.uint16) == on.view(np.uint16)) | nan_n).all(), f"{what}: gNormal differs"


LOWRES = {1: (256, 256), 2: (480, 270), 3: (384, 216), 4: (256, 144), 5: (256, 144)}


@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5])
def test_configs_lowres_bit_exact_vs_oracle(tracer, host, oracle, cfg):
    """Every BASELINE.json config's scene, whole frame at reduced size (C1 at its full size)."""
    sc = scenes.make_scene(cfg, host.generate_aabb)
    w, h = LOWRES[cfg]
    p = sc.params(width=w, height=h)
    gpu = render_gpu(tracer, sc, p)
    cpu = oracle.render(sc, p)
    assert_bit_exact(gpu, cpu, f"C{cfg} {w}x{h}")
    assert tracer.count_rays(p) == cpu[3]


@pytest.mark.parametrize("cfg", [2, 3, 4, 5])
def test_configs_fullres_windows_bit_exact_vs_oracle(tracer, host, oracle, cfg):
    """At BASELINE.json's full sizes (up to 7680x4320) the oracle renders 6 windows of 48x48;
    the GPU renders the same windows through the window parameters of the ABI."""
    sc = scenes.make_scene(cfg, host.generate_aabb)
    tracer.load(sc)
    W, H = sc.width, sc.height
    for fx, fy in [(0.1, 0.05), (0.5, 0.2), (0.3, 0.45), (0.7, 0.6), (0.9, 0.3), (0.45, 0.33)]:
        x0, y0 = int(fx * W) - 24, int(fy * H) - 24
        p = sc.params(window=(max(x0, 0), max(y0, 0), 48, 48))
        tracer.render(p)
        assert_bit_exact(tracer.readback(), oracle.render(sc, p), f"C{cfg} window @({x0},{y0})")


def test_c2_full_frame_properties(tracer, host, oracle):
    """The benchmark workload itself (1920x1080, 16 spheres + 2 planes, 3 lights, depth 4):
    whole frame bit-exact vs the oracle, ray count identical, render is deterministic, and the
    G-buffer conventions hold (alpha 1, miss pixels zero)."""
    sc = scenes.make_scene(2, host.generate_aabb)
    p = sc.params()
    gpu = render_gpu(tracer, sc, p)
    cpu = oracle.render(sc, p)
    assert_bit_exact(gpu, cpu, "C2 full")
    assert tracer.count_rays(p) == cpu[3]
    again = render_gpu(tracer, sc, p)
    assert_bit_exact(again, gpu, "C2 rerun")
    col, pos, nrm = gpu
    assert (col[..., 3] == 1).all() and (pos[..., 3] == 1).all() and (nrm[..., 3] == np.float16(1)).all()


# HIP vs the REFERENCE's own pixels (llvmpipe runs of the unmodified GLSL, tests/golden/*.npz), directly -- not through
# the oracle.  The host side evaluates tan / cos / sin and the kernel random()'s sin and SSS's exp exactly as the
# reference's GL does (csrc/rt_mesa_math.h), so the geometry surfaces must be the reference's BIT FOR BIT and gColor
# within north_star's 1e-4 (the one arithmetic difference left is pow(x,5): exact product here, exp2(5 log2 x)
# polynomials on llvmpipe, <= 1.3e-6 apart).  fixture -> (min bit-exact fraction of gPosition and of gNormal,
# min fraction of gColor pixels within 1e-4 relative).  The one residue left is an artefact of llvmpipe, not of the shader:
# C5 at depth 8, 8 px of 14 400 whose reference colour is cut short by gallivm's 65 535-iteration loop limiter (explained and
# emulated in tests/test_oracle_golden.py); C3's 20 px of round 2 are gone (NIR's factored bitangent.x, restated).
REF_GATES = {"c1": (1.0, 1.0), "c2": (1.0, 1.0), "c3": (1.0, 1.0), "c4": (1.0, 1.0), "c5": (1.0, 0.999), "nan": (1.0, 1.0)}


def _frac_exact(a, b):
    return compare_surface(a, b, rtol=0, atol=0)["exact_frac"]


@pytest.mark.parametrize("name", ["c1", "c2", "c3", "c4", "c5", "nan"])
def test_lowres_frame_against_reference_fixture(tracer, name):
    """Whole low-resolution frame of every config's scene against the reference's pixels."""
    g = load_golden(name)
    sc = GoldenScene(g)
    p = params_from_bytes(g["lowres_params"])
    col, pos, nrm = render_gpu(tracer, sc, p)
    exact_min, color_min = REF_GATES[name]
    ep, en = _frac_exact(pos, g["lowres_pos"]), _frac_exact(nrm.astype(np.float32), g["lowres_normal"].astype(np.float32))
    cc = compare_surface(col, g["lowres_color"])
    print(f"{name}: HIP vs reference lowres: gPosition exact {ep:.6f} gNormal exact {en:.6f} gColor 1e-4 {cc['pass_frac']:.6f}")
    assert ep >= exact_min, f"{name}: gPosition bit-exact on {ep:.6f}"
    assert en >= exact_min, f"{name}: gNormal bit-exact on {en:.6f}"
    assert cc["pass_frac"] >= color_min, f"{name}: gColor within 1e-4 on {cc['pass_frac']:.6f} ({cc['n_fail']} px)"


@pytest.mark.parametrize("name", ["c1", "c2", "c3", "c4", "c5"])
def test_fullres_windows_against_reference_fixture(tracer, name):
    """Eight 32x32 windows cut from the reference's FULL-resolution frame (C2 1080p, C3 / C4 4K; C5: its scene at
    1080p) -- the HIP path renders just those windows of the full-size image through the ABI's window parameters."""
    g = load_golden(name)
    if "win_params" not in g.files:
        pytest.skip("no full-resolution windows in this fixture")
    sc = GoldenScene(g)
    tracer.load(sc)
    base = params_from_bytes(g["win_params"])
    exact_min, color_min = REF_GATES[name]
    n_px = ep = en = okc = 0
    for k, (x0, y0) in enumerate(g["win_origins"]):
        p = L.copy_params(base, x0=int(x0), y0=int(y0), regionW=32, regionH=32)
        tracer.render(p)
        col, pos, nrm = tracer.readback()
        n_px += 32 * 32
        ep += compare_surface(pos, g["win_pos"][k], rtol=0, atol=0)["exact_mask"].sum()
        en += compare_surface(nrm.astype(np.float32), g["win_normal"][k].astype(np.float32), rtol=0, atol=0)["exact_mask"].sum()
        okc += compare_surface(col, g["win_color"][k])["ok_mask"].sum()
    print(f"{name}: HIP vs reference windows: gPosition exact {ep / n_px:.6f} gNormal exact {en / n_px:.6f} gColor 1e-4 {okc / n_px:.6f}")
    assert ep / n_px >= min(exact_min, 0.9995) and en / n_px >= min(exact_min, 0.9995)
    assert okc / n_px >= min(color_min, 0.999)


def test_c5_at_7680x4320_against_reference_fixture(tracer):
    """C5 at its REAL size: windows of the reference's 7680x4320 frame (partial dispatches of the unmodified GLSL
    on the full-size images, tests/golden/make_golden.py make_c5_8k) -- uv depends on imageSize and random() sees
    arguments up to 7e5 only here (raytracingCs.glsl:200-211, :273-275)."""
    g = load_golden("c5_8k")
    sc = GoldenScene(dict(objects=g["objects"], lights=g["lights"], frame_count=g["frame_count"], has_noise=0, has_skybox=1))
    tracer.load(sc)
    base = params_from_bytes(g["params"])
    assert (base.width, base.height) == (7680, 4320)
    win = g["win8k_color"].shape[1]
    n_px = ep = en = okc = 0
    for k, (x0, y0) in enumerate(g["win8k_origins"]):
        p = L.copy_params(base, x0=int(x0), y0=int(y0), regionW=win, regionH=win)
        tracer.render(p)
        col, pos, nrm = tracer.readback()
        n_px += win * win
        ep += compare_surface(pos, g["win8k_pos"][k], rtol=0, atol=0)["exact_mask"].sum()
        en += compare_surface(nrm.astype(np.float32), g["win8k_normal"][k].astype(np.float32), rtol=0, atol=0)["exact_mask"].sum()
        okc += compare_surface(col, g["win8k_color"][k])["ok_mask"].sum()
    print(f"c5 8K: HIP vs reference: gPosition exact {ep / n_px:.6f} gNormal exact {en / n_px:.6f} gColor 1e-4 {okc / n_px:.6f}")
    # (the gates of the oracle's own comparison with this fixture, tests/test_oracle_golden.py: HIP == oracle bit for bit)
    assert ep / n_px >= 0.9995 and en / n_px >= 0.9995
    assert okc / n_px >= 0.999


def test_nan_and_ub_corners_match_oracle(tracer, host, oracle):
    """roughness 0 (0/0 in the NDF), light straight above (NaN PCF tangent), ior 0 refraction
    (inf eta), unnormalised plane normal: same NaNs, same bits as the oracle."""
    sc = scenes.nan_parity_scene(host.generate_aabb)
    p = sc.params()
    gpu = render_gpu(tracer, sc, p)
    cpu = oracle.render(sc, p)
    assert_bit_exact(gpu, cpu, "nan scene")


def test_edge_sizes_and_empty_scenes(tracer, host, oracle):
    """Ragged sizes (not multiples of the 16x16 tile), 1x1, empty object / light lists."""
    sc = scenes.make_scene(2, host.generate_aabb)
    for w, h in [(1, 1), (17, 9), (31, 33), (250, 3), (3, 250)]:
        p = sc.params(width=w, height=h)
        assert_bit_exact(render_gpu(tracer, sc, p), oracle.render(sc, p), f"{w}x{h}")
    empty = scenes.Scene("empty", sc.objects[:0], sc.lights, 40, 24, 4, dict(scenes.CAMERA))
    p = empty.params()
    col, pos, nrm = render_gpu(tracer, empty, p)
    assert (col == np.array([0, 0, 0, 1], dtype=np.float32)).all() and (pos == np.array([0, 0, 0, 1], dtype=np.float32)).all()
    assert tracer.count_rays(p) == 40 * 24
    nolight = scenes.Scene("nolight", sc.objects, sc.lights[:0], 40, 24, 4, dict(scenes.CAMERA))
    p = nolight.params()
    assert_bit_exact(render_gpu(tracer, nolight, p), oracle.render(nolight, p), "no lights")
    # depth 0: nothing traced, everything (0,0,0,1)
    p0 = sc.params(width=32, height=32, max_ray_depth=0)
    col, pos, nrm = render_gpu(tracer, sc, p0)
    assert (col == np.array([0, 0, 0, 1], dtype=np.float32)).all()


def test_many_objects_and_limits(tracer, host, oracle):
    """The SSBOs are runtime-sized (raytracingCs.glsl:65-73): the default kernel takes any object count (2 048 here, against the
    oracle); the exhaustive cross-check kernel stages the scene in LDS and refuses more than 512 objects at render time with
    RT_ERR_TOO_LARGE, leaving the context usable."""
    rng = scenes.SplitMix64(99)
    objs = scenes._spheres(rng, 512)
    objs["radius"] *= 0.4
    host.generate_aabb(objs)
    lights = scenes._lights3(L.SHADOW_PCF)[:1]
    sc = scenes.Scene("max", objs, lights, 64, 48, 2, dict(scenes.CAMERA))
    p = sc.params()
    assert_bit_exact(render_gpu(tracer, sc, p), oracle.render(sc, p), "512 objects")
    big = scenes._spheres(rng, 2048)
    big["radius"] *= 0.25
    host.generate_aabb(big)
    lights3 = scenes._lights3(L.SHADOW_PCF)
    scb = scenes.Scene("big", big, lights3, 64, 48, 3, dict(scenes.CAMERA))
    if tracer.variant == 0:
        tracer.set_scene(big, lights3)
        with pytest.raises(host.RtError) as e:
            tracer.render(scb.params())
        assert e.value.code == -4
    else:
        assert_bit_exact(render_gpu(tracer, scb, scb.params()), oracle.render(scb, scb.params()), "2048 objects")
        assert tracer.count_rays(scb.params()) == oracle.render(scb, scb.params())[3]
        many = scenes._lights3(L.SHADOW_PCF)
        many = scenes._concat([many] * 24)[:70].copy()             # 70 lights: beyond the shadow tables' 64 -> the per-packet light culls
        many["position"][:, 0] += np.linspace(-4, 4, 70).astype(np.float32)
        scl = scenes.Scene("lights70", sc.objects[:40].copy(), many, 48, 32, 2, dict(scenes.CAMERA))
        assert_bit_exact(render_gpu(tracer, scl, scl.params()), oracle.render(scl, scl.params()), "70 lights")
    tracer.set_scene(objs, lights)   # context still usable
    with pytest.raises(host.RtError) as e:
        tracer.render(sc.params(max_ray_depth=33))
    assert e.value.code == -1
    bad = sc.params()
    bad.stripIndex = 3
    with pytest.raises(host.RtError):
        tracer.render(bad)


def test_pcf_sample_counts_and_shadow_types(tracer, host, oracle):
    """pcfSamples 1..16 (the UI range) and beyond the Halton table (70), shadowType 0/1/2 and an
    out-of-range shadowType (calculateShadow's fall-through returns 0), pcfSamples 0 (0/0 NaN)."""
    sc = scenes.make_scene(2, host.generate_aabb)
    for samples, stype in [(1, 1), (7, 1), (16, 2), (70, 1), (4, 0), (4, 5), (0, 1)]:
        sc.lights["pcfSamples"] = samples
        sc.lights["shadowType"] = stype
        p = sc.params(width=96, height=54)
        assert_bit_exact(render_gpu(tracer, sc, p), oracle.render(sc, p), f"pcf {samples} type {stype}")


@pytest.mark.parametrize("cfg,samples", [(4, 3), (4, 8), (4, 16), (5, 3), (5, 9), (5, 16)])
def test_many_pcf_samples_in_many_object_scenes(tracer, host, oracle, cfg, samples):
    """From RT_PK_REACH_MIN_SAMPLES = 3 samples per light on, the many-object kernel profiles refine each light's candidate mask
    per LANE on the spheres themselves before the sample loops (rt_packet.inc, the profiles' `reach`): C4's / C5's scenes at the
    threshold (3), at 8 / 9 and at the UI's maximum of 16 PCF samples, and with a softness near the bound where the jitter interval
    swallows whole direction components (filterSize 0.15 of the 0.2 limit).  Both scenes have shadow tables (PkHeavy1 / PkHeavy), so
    what this reaches is the shape level applied to the TABLES' masks; the packet-level light culls and the shape level on their
    masks run only in scenes without tables (PkHuge / PkHugeS): tests/test_exponent_range.py's huge300 cases pin those."""
    sc = scenes.make_scene(cfg, host.generate_aabb)
    sc.lights["pcfSamples"] = samples
    p = sc.params(width=80, height=48)
    assert_bit_exact(render_gpu(tracer, sc, p), oracle.render(sc, p), f"C{cfg} pcf {samples}")
    sc.lights["shadowSoftness"] = 30.0
    sc.lights["type"][1] = L.DIRECTIONAL
    sc.lights["type"][2] = L.POINT
    assert_bit_exact(render_gpu(tracer, sc, p), oracle.render(sc, p), f"C{cfg} pcf {samples}, wide jitter, mixed light types")


def test_noise_skybox_and_framecount(tracer, host, oracle):
    """Noise texture bound / unbound, frameCount > 0, skybox on / off, non-power-of-two noise."""
    sc = scenes.make_scene(3, host.generate_aabb)
    p = sc.params(width=128, height=72)
    assert_bit_exact(render_gpu(tracer, sc, p), oracle.render(sc, p), "noise + frameCount 7")
    sc.noise = scenes.hash_noise(100, 60, seed=3)
    sc.frame_count = 123
    p = sc.params(width=128, height=72)
    p.noiseScale[0], p.noiseScale[1] = 1.0 / 100.0, 1.0 / 60.0
    assert_bit_exact(render_gpu(tracer, sc, p), oracle.render(sc, p), "100x60 noise")
    sc5 = scenes.make_scene(5, host.generate_aabb)
    sc5.objects = sc5.objects[:40].copy()
    p = sc5.params(width=128, height=72)
    assert_bit_exact(render_gpu(tracer, sc5, p), oracle.render(sc5, p), "skybox")
    sc5.use_skybox = False
    p = sc5.params(width=128, height=72)
    assert_bit_exact(render_gpu(tracer, sc5, p), oracle.render(sc5, p), "skybox off")


def test_strip_tiling_equals_single_render(tracer, host):
    """Multi-GPU tiling invariant on one device: rendering the interleaved strips of each rank
    and re-assembling them (rt_deinterleave) reproduces the single render bit for bit."""
    import torch
    from opengl_raytracing_amd import dist as D
    sc = scenes.make_scene(2, host.generate_aabb)
    base = sc.params(width=322, height=187)
    col, pos, nrm = render_gpu(tracer, sc, base)
    for world, strip_rows in [(2, 16), (4, 16), (8, 8), (3, 32)]:
        plan = D.StripPlan(322, 187, strip_rows, world)
        gathered = torch.empty((world, plan.rank_bytes), dtype=torch.uint8, device="cuda")
        for r in range(world):
            vc, vp, vn = D.surface_views(gathered[r], plan)
            tracer.render_to(plan.params(base, r), vc.data_ptr(), vp.data_ptr(), vn.data_ptr())
        tracer.sync()
        outs = D.deinterleave_hip(tracer, gathered, plan)
        tracer.sync()
        torch.cuda.synchronize()
        check = D.deinterleave_torch(gathered, plan)
        for out, chk, ref in zip(outs, check, (col, pos, nrm)):
            assert bits_equal(out.cpu().numpy(), ref), f"world {world}"
            it = torch.int16 if out.dtype == torch.float16 else torch.int32
            assert torch.equal(out.view(it), chk.view(it))
        # the same frame through the 30 B/pixel wire format bench.py gathers (rt_wire_pack / rt_wire_unpack)
        wires = torch.zeros((world, plan.wire_bytes), dtype=torch.uint8, device="cuda")
        for r in range(world):
            D.pack_wire_hip(tracer, D.surface_views(gathered[r], plan), wires[r], plan)
            assert torch.equal(wires[r], D.pack_wire_torch(D.surface_views(gathered[r], plan), plan)), f"pack, world {world}"
        wouts = D.unpack_wire_hip(tracer, wires, plan)
        tracer.sync()
        for out, wout in zip(outs, wouts):
            it = torch.int16 if out.dtype == torch.float16 else torch.int32
            assert torch.equal(out.view(it), wout.view(it)), f"wire path, world {world}"
        for a, b in zip(wouts, D.unpack_wire_torch(wires, plan)):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    # weighted root: rank 0 owns root_weight strips per cycle and its rows never enter the wire
    for world, strip_rows, w0 in [(2, 8, 2), (4, 8, 3), (8, 8, 2), (3, 16, 4)]:
        plan = D.StripPlan(322, 187, strip_rows, world, w0)
        root = D.alloc_rank_buffer(plan, "cuda", 0)
        rviews = D.surface_views(root, plan, 0)
        tracer.render_to(plan.params(base, 0), *(v.data_ptr() for v in rviews))
        wires = torch.zeros((world, plan.wire_bytes), dtype=torch.uint8, device="cuda")
        peer = D.alloc_rank_buffer(plan, "cuda", 1)
        pviews = D.surface_views(peer, plan, 1)
        for r in range(1, world):
            tracer.render_to(plan.params(base, r), *(v.data_ptr() for v in pviews))
            D.pack_wire_hip(tracer, pviews, wires[r], plan)
        wouts = D.unpack_wire_hip(tracer, wires, plan, root_views=rviews)
        tracer.sync()
        torch.cuda.synchronize()
        for out, ref in zip(wouts, (col, pos, nrm)):
            assert bits_equal(out.cpu().numpy(), ref), f"weighted root, world {world} w0 {w0}"
        for a, b in zip(wouts, D.unpack_wire_torch(wires, plan, root_views=rviews)):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("cfg", [2, 4])
def test_shadow_type_switches_the_kernel_instantiation_per_scene(tracer, host, oracle, cfg):
    """rt_set_scene picks the kernel instantiation with grouped PCSS blocker rays when any light has shadowType 2
    (rt_abi.cpp: anyPcss) and the PCF-only one otherwise: PCF -> one PCSS light among PCF lights -> all PCSS -> PCF again on one
    context, each frame against the oracle (few- and many-object profiles)."""
    sc = scenes.make_scene(cfg, host.generate_aabb)
    p = sc.params(width=96, height=54)
    for types in ([L.SHADOW_PCF] * len(sc.lights), None, [L.SHADOW_PCSS] * len(sc.lights), [L.SHADOW_PCF] * len(sc.lights)):
        if types is None:
            sc.lights["shadowType"] = L.SHADOW_PCF
            sc.lights["shadowType"][len(sc.lights) // 2] = L.SHADOW_PCSS
        else:
            sc.lights["shadowType"] = types
        assert_bit_exact(render_gpu(tracer, sc, p), oracle.render(sc, p), f"C{cfg} shadow types {list(sc.lights['shadowType'])}")


def test_scene_update_every_frame_and_timing(tracer, host, oracle):
    """The reference re-uploads both SSBOs every frame (ImGUIManager.cpp:202,338): back-to-back
    set_scene/render pairs must each see their own scene; the timing hook returns a duration."""
    a = scenes.make_scene(2, host.generate_aabb)
    b = scenes.make_scene(2, host.generate_aabb)
    b.objects["position"][:, 0] += 1.5
    host.generate_aabb(b.objects)
    p = a.params(width=160, height=90)
    want_a, want_b = oracle.render(a, p), oracle.render(b, p)
    for _ in range(3):
        tracer.set_scene(a.objects, a.lights)
        tracer.render(p)
        ga = tracer.readback()
        tracer.set_scene(b.objects, b.lights)
        tracer.render(p)
        gb = tracer.readback()
        assert_bit_exact(ga, want_a, "scene a")
        assert_bit_exact(gb, want_b, "scene b")
    assert 0 < tracer.last_kernel_ms() < 1000


def _fuzz_scene(seed):
    """Random scene drawn to stress the packet culling's rigour: tilted / unnormalised / degenerate
    planes, tiny and huge spheres, camera inside objects, lights inside geometry or at a shading
    point, all shadow types, large softness (culling disabled above the jitter bound), random
    pcfSamples / frameCount, occasional inf / NaN / zero fields and malformed (min > max) AABBs."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 70 if seed % 5 else 140))
    if seed % 13 == 5:
        n = int(rng.integers(257, 420))                           # four-wave workgroups, AABB-only staging
    objs = L.default_objects(n)
    objs["type"] = rng.integers(0, 2, n)
    if seed % 7 == 0:
        objs["type"][rng.integers(0, n)] = 3                      # unknown type: never hit
    objs["position"] = rng.uniform(-8, 8, (n, 3)) * rng.choice([0.2, 1.0, 3.0])
    objs["radius"] = rng.choice([0.01, 0.3, 1.0, 4.0, 30.0], n) * rng.uniform(0.5, 1.5, n)
    nrm = rng.normal(size=(n, 3)) * rng.choice([0.1, 1.0, 5.0], (n, 1))
    axis = rng.integers(0, 4, n)
    for k in range(3):
        sel = axis == k
        nrm[sel] = 0
        nrm[sel, k] = rng.choice([-1.0, 1.0, 2.0], sel.sum())
    objs["normal"] = nrm
    objs["size"] = rng.uniform(0.0, 30.0, (n, 2))
    objs["albedo"] = rng.uniform(0, 1, (n, 3))
    objs["metallic"] = rng.choice([0.0, 1.0, 0.5], n)
    objs["roughness"] = rng.choice([0.0, 0.05, 0.5, 1.0], n)
    objs["diffuseStrength"] = rng.choice([0.0, 0.0, 0.6, 1.0], n)
    objs["ior"] = rng.choice([0.0, 1.0, 1.5, 2.5], n)
    objs["transparency"] = rng.choice([0.0, 0.0, 0.95], n)
    objs["subsurfaceScatter"] = rng.choice([0.0, 0.0, 0.0, 0.5], n)
    objs["scatterDistance"] = rng.choice([0.1, 0.8, 0.0], n)
    from opengl_raytracing_amd import host as H
    H.generate_aabb(objs)
    if seed % 3 == 0:      # hostile records: the kernel trusts `bounds` as given
        k = int(rng.integers(0, n))
        objs["bounds_min"][k], objs["bounds_max"][k] = objs["bounds_max"][k].copy(), objs["bounds_min"][k].copy()
        k = int(rng.integers(0, n))
        objs["bounds_min"][k] = -np.inf
        objs["bounds_max"][k] = np.inf
    if seed % 11 == 0:
        objs["bounds_min"][int(rng.integers(0, n)), int(rng.integers(0, 3))] = np.nan
        objs["position"][int(rng.integers(0, n)), 0] = np.nan
    nl = int(rng.integers(0, 5))
    lts = L.default_lights(nl)
    if nl:
        lts["type"] = rng.integers(0, 3, nl)
        lts["position"] = rng.uniform(-10, 10, (nl, 3))
        lts["direction"] = rng.normal(size=(nl, 3))
        if seed % 4 == 0:
            lts["direction"][0] = (0.0, -1.0, 0.0)
        lts["color"] = rng.uniform(0.2, 1, (nl, 3))
        lts["intensity"] = rng.uniform(0.5, 20, nl)
        lts["shadowType"] = rng.integers(0, 3, nl)
        lts["pcfSamples"] = rng.choice([1, 3, 4, 9, 16], nl)
        lts["shadowSoftness"] = rng.choice([0.0, 1.0, 2.0, 60.0, -1.0], nl)     # 60 -> filterSize 0.3 > cull bound
        lts["lightSize"] = rng.choice([0.1, 1.0, 5.0], nl)
    cam = dict(scenes.CAMERA)
    cam["cam_pos"] = tuple(rng.uniform(-6, 6, 3))
    f, r, u = H.camera_vectors(float(rng.uniform(-180, 180)), float(rng.uniform(-60, 60)))
    cam["cam_dir"], cam["cam_right"], cam["cam_up"] = f, r, u
    cam["fov_deg"] = float(rng.choice([20.0, 45.0, 90.0]))
    sc = scenes.Scene(f"fuzz{seed}", objs, lts, 48, 40, int(rng.integers(1, 7)), cam,
                      frame_count=int(rng.integers(0, 200)))
    if seed % 2:
        sc.noise = scenes.hash_noise(64, 32, seed=seed)
    return sc


@pytest.mark.parametrize("block", range(int(os.environ.get("RT_FUZZ_BLOCKS", "10"))))      # 10 seeds per block
def test_fuzzed_scenes_bit_exact_vs_oracle(tracer, host, oracle, block):
    """100 random scenes per kernel variant (see _fuzz_scene): all three surfaces and the ray count
    must equal the oracle's bit for bit -- in particular, packet culling may never drop an object
    some lane's exact intersectAABB would have passed."""
    for seed in range(block * 10, block * 10 + 10):
        sc = _fuzz_scene(seed)
        p = sc.params()
        if sc.noise is not None:
            p.noiseScale[0], p.noiseScale[1] = 1.0 / 64.0, 1.0 / 32.0
        gpu = render_gpu(tracer, sc, p)
        cpu = oracle.render(sc, p)
        assert_bit_exact(gpu, cpu, f"fuzz seed {seed}")
        assert tracer.count_rays(p) == cpu[3], f"fuzz seed {seed}: ray count"


def test_cpp_host_example_matches_python_path(host, oracle, tmp_path):
    """examples/host_swap.cpp drives the C ABI from plain C++ the way the reference's host would
    (parse scene -> rt_set_scene -> rt_render -> rt_readback); its surface hashes must equal the
    ctypes path's and the oracle's on the same scene."""
    import json
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "host_swap")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(repo, "include"), os.path.join(repo, "examples", "host_swap.cpp"),
                    "-L", os.path.join(repo, "opengl_raytracing_amd"), "-lrt_mi355",
                    "-Wl,-rpath," + os.path.join(repo, "opengl_raytracing_amd"), "-o", exe], check=True)
    out = json.loads(subprocess.run([exe, "200", "120"], check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1])
    text = [l.split('"')[1].replace("\\n", "") for l in open(os.path.join(repo, "examples", "host_swap.cpp")) if l.strip().startswith('"OBJECT') or l.strip().startswith('"LIGHT')]
    objs, lts = host.parse_scene("\n".join(text))
    f, r, u = host.camera_vectors(-90.0, 0.0)
    sc = scenes.Scene("cpp", objs, lts, 200, 120, 3, dict(cam_pos=(0.0, 1.0, 3.0), cam_dir=f, cam_up=u, cam_right=r, fov_deg=45.0))
    col, pos, nrm, rays = oracle.render(sc, sc.params())

    def fnv(a):
        h = 1469598103934665603
        for b in a.tobytes():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return f"{h:016x}"

    assert out["rays"] == rays
    assert out["color"] == fnv(col) and out["position"] == fnv(pos) and out["normal"] == fnv(nrm)


def test_frames_in_flight_on_several_streams(tracer, host):
    """bench.py's N > 1 pipeline keeps several frames in flight on separate render streams while the tile-order
    feedback re-sorts beside them (double-buffered order, sort on the context's stream).  Every frame must still
    cover every tile exactly once: buffers are zeroed before each launch, so a torn order would leave holes."""
    import torch
    sc = scenes.make_scene(2, host.generate_aabb)
    p = sc.params(width=640, height=360)
    tracer.load(sc)
    ref = render_gpu(tracer, sc, p)
    streams = [torch.cuda.Stream() for _ in range(3)]
    bufs = [(torch.empty((360, 640, 4), dtype=torch.float32, device="cuda"), torch.empty((360, 640, 4), dtype=torch.float32, device="cuda"),
             torch.empty((360, 640, 4), dtype=torch.float16, device="cuda")) for _ in range(3)]
    for k in range(150):
        s, (c, q, n) = streams[k % 3], bufs[k % 3]
        with torch.cuda.stream(s):
            c.zero_(); q.zero_(); n.zero_()
        tracer.render_to(p, c.data_ptr(), q.data_ptr(), n.data_ptr(), stream=s.cuda_stream)
        if k % 37 == 36 or k >= 147:
            torch.cuda.synchronize()
            for got, want in zip((c, q, n), ref):
                assert bits_equal(got.cpu().numpy(), want), f"frame {k}"
    torch.cuda.synchronize()


def test_first_frames_of_a_new_geometry_on_three_streams(host):
    """the tile order is adopted per CONTEXT but streams are not ordered with each other, so on a
    never-seen geometry frame 2 (third stream) used to read an order buffer only frame 1's stream had waited for.
    A fresh context, three streams, a geometry it has never rendered, zeroed targets: frames 0..7 must each cover
    every tile exactly once (bit-exact vs a single-stream render).  Repeated for several geometries so that the
    order buffers also carry a stale permutation of the PREVIOUS geometry when the next one starts."""
    import torch
    sc = scenes.make_scene(2, host.generate_aabb)
    with host.RayTracer(0) as rt:
        rt.load(sc)
        streams = [torch.cuda.Stream() for _ in range(3)]
        for (w, h) in [(640, 360), (320, 200), (648, 368), (640, 360)]:
            p = sc.params(width=w, height=h)
            with host.RayTracer(0) as ref_rt:
                ref_rt.load(sc)
                ref_rt.set_variant(0x101)        # packet kernel, raster order: no feedback state involved
                ref_rt.render(p)
                ref = ref_rt.readback()
            bufs = [(torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"), torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"),
                     torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")) for _ in range(8)]
            torch.cuda.synchronize()
            for k in range(8):                   # host runs ahead: nothing synchronises between the launches
                c, q, n = bufs[k]
                rt.render_to(p, c.data_ptr(), q.data_ptr(), n.data_ptr(), stream=streams[k % 3].cuda_stream)
            torch.cuda.synchronize()
            for k in range(8):
                for got, want in zip(bufs[k], ref):
                    assert bits_equal(got.cpu().numpy(), want), f"{w}x{h} frame {k}"


def test_free_running_framecount_over_three_periods_on_three_streams(host):
    """frameCount advancing every frame (ForwardShadingPipeline.cpp:254): from the third such frame on the context keeps one
    measured tile order per phase (frameCount mod 64), sorted beside the frames on a stream of its own and read 64 frames later.
    Scheduling only: every frame of 200 consecutive frameCounts, issued on three streams into zeroed targets with the host
    running ahead, must equal the raster-order render of the same frameCount bit for bit (a bad or half-written order would
    leave tiles black or rendered twice).  Then a geometry change in mid-run, and back."""
    import torch
    from opengl_raytracing_amd import layout as L
    sc = scenes.make_scene(2, host.generate_aabb)
    with host.RayTracer(0) as rt, host.RayTracer(0) as ref_rt:
        rt.load(sc)
        ref_rt.load(sc)
        ref_rt.set_variant(0x101)                # packet kernel, raster order: no scheduler state
        streams = [torch.cuda.Stream() for _ in range(3)]
        fc = 5
        for (w, h), n_frames in [((320, 200), 200), ((328, 136), 70), ((320, 200), 70)]:
            base = sc.params(width=w, height=h)
            bufs = [(torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"), torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"),
                     torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")) for _ in range(n_frames)]
            torch.cuda.synchronize()
            for k in range(n_frames):
                c, q, n = bufs[k]
                rt.render_to(L.copy_params(base, frameCount=fc + k), c.data_ptr(), q.data_ptr(), n.data_ptr(), stream=streams[k % 3].cuda_stream)
            torch.cuda.synchronize()
            for k in range(n_frames):
                ref_rt.render(L.copy_params(base, frameCount=fc + k))
                ref = ref_rt.readback()
                for got, want in zip(bufs[k], ref):
                    assert bits_equal(got.cpu().numpy(), want), f"{w}x{h} frameCount {fc + k}"
            fc += n_frames


def test_scene_updates_between_frames_in_flight_on_three_streams(host, oracle):
    """the reference re-uploads its SSBOs every frame (ImGUIManager.cpp:202, :338), so rt_set_scene
    alternates with frames that are still in flight on several caller streams.  Each frame must be rendered from
    the scene that was current when it was issued: rt_set_scene orders the rewrite of the device scene behind the
    last launch of EVERY stream, not only the most recent one."""
    import torch
    base = scenes.make_scene(2, host.generate_aabb)
    w, h = 480, 270
    p = base.params(width=w, height=h)
    variants = []
    for k in range(4):
        sc = scenes.make_scene(2, host.generate_aabb)
        sc.objects["position"][:, 0] += 0.35 * k
        sc.objects["position"][:, 1] += 0.1 * k
        host.generate_aabb(sc.objects)
        variants.append((sc, oracle.render(sc, p)))
    with host.RayTracer(0) as rt:
        streams = [torch.cuda.Stream() for _ in range(3)]
        n_frames = 24
        bufs = [(torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"), torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"),
                 torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")) for _ in range(n_frames)]
        torch.cuda.synchronize()
        for k in range(n_frames):
            sc, _ = variants[k % 4]
            rt.set_scene(sc.objects, sc.lights)          # while frames k-1, k-2 are still running on other streams
            c, q, n = bufs[k]
            rt.render_to(p, c.data_ptr(), q.data_ptr(), n.data_ptr(), stream=streams[k % 3].cuda_stream)
        torch.cuda.synchronize()
        for k in range(n_frames):
            want = variants[k % 4][1]
            assert_bit_exact(tuple(t.cpu().numpy() for t in bufs[k]), want, f"frame {k} (scene {k % 4})")


def _zeroed_targets(w, h, n):
    import torch
    return [(torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"), torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"),
             torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")) for _ in range(n)]


def test_more_render_streams_than_stream_records(host, monkeypatch):
    """The scheduler keeps one record per stream frames were issued on, eight at most; a ninth stream drains everything
    and starts the records over, after which a record (its `last` event, its prediction buffers) belongs to another stream
    than before.  Nine streams round-robin, the host running ahead: 27 frames of one geometry, then 18 of a second one, into
    zeroed targets; every frame must equal the raster-order render bit for bit.  RT_PRED_MIN_TILES=1 lets these small frames
    take the predicted order too, so the first frame of each geometry predicts into the buffers of whichever record its stream
    holds by then."""
    import torch
    monkeypatch.setenv("RT_PRED_MIN_TILES", "1")      # read when the context is created
    sc = scenes.make_scene(2, host.generate_aabb)
    with host.RayTracer(0) as rt, host.RayTracer(0) as ref_rt:
        rt.load(sc)
        ref_rt.load(sc)
        ref_rt.set_variant(0x101)                # packet kernel, raster order: no scheduler state
        streams = [torch.cuda.Stream() for _ in range(9)]
        issued = 0
        for (w, h), n_frames in [((320, 200), 27), ((328, 136), 18)]:
            p = sc.params(width=w, height=h)
            ref_rt.render(p)
            ref = ref_rt.readback()
            bufs = _zeroed_targets(w, h, n_frames)
            torch.cuda.synchronize()
            for k in range(n_frames):            # nothing synchronises between the launches
                c, q, n = bufs[k]
                rt.render_to(p, c.data_ptr(), q.data_ptr(), n.data_ptr(), stream=streams[(issued + k) % 9].cuda_stream)
            issued += n_frames
            torch.cuda.synchronize()
            for k in range(n_frames):
                for got, want in zip(bufs[k], ref):
                    assert bits_equal(got.cpu().numpy(), want), f"{w}x{h} frame {k}"


def test_mode_switches_in_mid_run_on_three_streams(host):
    """rt_set_variant between frames in flight: 12 frames in each of the modes 1 (predicted, measured and per-phase orders),
    0x201 (measured only), 0x101 (raster), 1 again, on three streams with frameCount advancing and nothing synchronised at the
    switches; every frame must equal the raster-order render of its frameCount bit for bit.  A mode switch forgets the
    geometry: rt_debug_tile_costs reports zero tiles right after it (which returns before touching the device).  A read-out
    of real costs drains every stream, so it comes after the run: one more block in mode 0x201 must report the geometry's
    25 x 40 tiles of 8 x 8 pixels with a non-zero sum."""
    import torch
    sc = scenes.make_scene(2, host.generate_aabb)
    w, h = 320, 200
    base = sc.params(width=w, height=h)
    with host.RayTracer(0) as rt, host.RayTracer(0) as ref_rt:
        rt.load(sc)
        ref_rt.load(sc)
        ref_rt.set_variant(0x101)
        streams = [torch.cuda.Stream() for _ in range(3)]
        modes = [1, 0x201, 0x101, 1, 0x201]
        bufs = _zeroed_targets(w, h, 12 * len(modes))
        torch.cuda.synchronize()

        def block(b):
            rt.set_variant(modes[b])
            assert rt.tile_costs().size == 0, f"block {b}: the geometry survived the mode switch"
            for k in range(12 * b, 12 * b + 12):
                c, q, n = bufs[k]
                rt.render_to(L.copy_params(base, frameCount=5 + k), c.data_ptr(), q.data_ptr(), n.data_ptr(), stream=streams[k % 3].cuda_stream)

        for b in range(4):
            block(b)
        torch.cuda.synchronize()
        block(4)
        costs = rt.tile_costs()
        assert costs.shape == ((h + 7) // 8, (w + 7) // 8)
        assert int(costs.sum(dtype=np.uint64)) > 0
        rt.set_variant(1)
        assert rt.tile_costs().size == 0
        torch.cuda.synchronize()
        for k in range(len(bufs)):
            ref_rt.render(L.copy_params(base, frameCount=5 + k))
            ref = ref_rt.readback()
            for got, want in zip(bufs[k], ref):
                assert bits_equal(got.cpu().numpy(), want), f"mode {modes[k // 12]:#x} frameCount {5 + k}"


def _grazing_scene(kind, scale, offset, samples, softness, ltype, seed):
    """Shadow rays that graze: a floor under a light, 40 spheres between them whose shadow limbs cross the view -- every pixel on
    a shadow's edge is a ray within rounding of a sphere's limb.  kind: 'tiny' (radii 1e-3..1e-2 of the scene's scale), 'mixed',
    'huge' (one sphere of radius 1e3 scales whose limb cuts the view), 'axis' (centres exactly on the segment shading point ->
    light of the central pixels, where dot(oc, oc) - p*p cancels).  The whole scene is scaled and moved far from the origin
    (|coordinates| up to 1e5: the differences the cull levels take cancel there)."""
    rng = np.random.default_rng(seed)
    s = np.float32(scale)
    off = np.array(offset, dtype=np.float32)
    n = 40
    objs = L.default_objects(n + 1)
    objs["type"][:n] = L.SPHERE
    lightp = np.array([0.3, 8.0, -0.2], dtype=np.float32) * s
    if kind == "tiny":
        r = 10.0 ** rng.uniform(-3, -2, n)
        pos = np.stack([rng.uniform(-2, 2, n), rng.uniform(0.05, 0.5, n), rng.uniform(-2, 2, n)], 1)
    elif kind == "huge":
        r = 10.0 ** rng.uniform(-1, 0, n)
        pos = np.stack([rng.uniform(-3, 3, n), rng.uniform(1, 5, n), rng.uniform(-3, 3, n)], 1)
        r[0] = 1000.0
        pos[0] = (1000.6, 3.0, 0.0)                       # its limb passes 0.6 from the light's axis
    elif kind == "axis":
        r = 10.0 ** rng.uniform(-2, -0.5, n)
        tq = rng.uniform(0.1, 0.9, n)
        q = np.stack([rng.uniform(-2, 2, n), np.zeros(n), rng.uniform(-2, 2, n)], 1)      # floor points
        pos = q + tq[:, None] * (lightp / s - q)          # centres ON the segments floor point -> light
    else:
        r = 10.0 ** rng.uniform(-2.5, 0.3, n)
        pos = np.stack([rng.uniform(-3, 3, n), rng.uniform(0.2, 6, n), rng.uniform(-3, 3, n)], 1)
    objs["position"][:n] = (pos * s).astype(np.float32) + off
    objs["radius"][:n] = (r * s).astype(np.float32)
    objs["albedo"][:n] = 0.7
    objs["roughness"][:n] = 0.4
    objs["type"][n] = L.PLANE                              # the floor the shadows fall on (diffuse: a second bounce of grazing rays)
    objs["position"][n] = off
    objs["normal"][n] = (0, 1, 0)
    objs["size"][n] = (4000 * s, 4000 * s)
    objs["albedo"][n] = 0.8
    objs["diffuseStrength"][n] = 0.7
    from opengl_raytracing_amd import host as H
    H.generate_aabb(objs)
    lts = L.default_lights(1)
    lts["type"] = ltype
    lts["position"] = lightp + off
    lts["direction"] = (-0.1, -1.0, 0.05) if ltype == L.DIRECTIONAL else (0.0, 1.0, 0.0)
    lts["intensity"] = 30.0 * float(s) * float(s) if ltype == L.AREA else 6.0
    lts["shadowType"] = L.SHADOW_PCF
    lts["pcfSamples"] = samples
    lts["shadowSoftness"] = softness
    cam = dict(cam_pos=tuple((np.array([0.0, 9.0, 0.3], dtype=np.float32) * s + off).tolist()), cam_dir=(0.0, -1.0, 0.0),
               cam_up=(0.0, 0.0, -1.0), cam_right=(1.0, 0.0, 0.0), fov_deg=40.0)
    return scenes.Scene(f"graze-{kind}", objs, lts, 96, 64, 2, cam)


@pytest.mark.parametrize("kind", ["tiny", "mixed", "huge", "axis"])
def test_grazing_shadow_rays_far_from_the_origin(tracer, host, oracle, kind):
    """ADVICE r2 / VERDICT r2 #4b: the per-lane sphere level (the profiles' `reach`) and the shadow tables drop candidates on margin
    arguments; this aims rays at sphere limbs -- shadow edges of tiny, huge and on-axis spheres, at scales 1 and 1e3 and offsets
    up to 1e5 from the origin, 3 / 4 / 16 samples, softness 0 to the 0.2 filter bound, point / area / directional lights (41
    objects: the many-object profile, per-lane level on from 3 samples) -- against the oracle, bit for bit."""
    k = 0
    for scale, offset in [(1.0, (0, 0, 0)), (1.0, (1e4, -3e3, 2e4)), (1e3, (0, 0, 0)), (1.0, (1e5, 1e5, -1e5)), (1e-2, (50.0, 0.0, -20.0))]:
        for samples, softness, ltype in [(3, 1.0, L.POINT), (4, 0.0, L.AREA), (16, 39.0, L.POINT), (4, 1.0, L.DIRECTIONAL), (16, 10.0, L.AREA)]:
            k += 1
            if (k + len(kind)) % 2:           # half of the 25 combinations per kind, a different half for each
                continue
            sc = _grazing_scene(kind, scale, offset, samples, softness, ltype, seed=k)
            p = sc.params()
            gpu = render_gpu(tracer, sc, p)
            cpu = oracle.render(sc, p)
            assert_bit_exact(gpu, cpu, f"{kind} scale {scale} offset {offset} samples {samples} softness {softness} light {ltype}")
            assert tracer.count_rays(p) == cpu[3]


def _blocker_fan_scene(kind, scale, offset, light_size, ltype, seed):
    """A PCSS light above a floor with <= 31 spheres (the few-object PCSS profile: blocker rays four per packet).
    The 16 blocker rays of a floor pixel fan out in the plane spanned by its light direction and (1,1,1); spheres are placed so
    that many pixels' fan planes graze them: 'onplane' = centres at r (1 +- 1e-6 .. 1e-2) from the fan plane of a floor point,
    'diag' = the light straight along (1,1,1) from the scene's centre (degenerate fan plane for the central pixels), 'tiny' / 'mixed'
    = random spheres whose limbs cross many fans."""
    rng = np.random.default_rng(seed)
    s = np.float32(scale)
    off = np.array(offset, dtype=np.float32)
    n = 30
    objs = L.default_objects(n + 1)
    objs["type"][:n] = L.SPHERE
    lightp = (np.array([4.0, 4.0, 4.0]) if kind == "diag" else np.array([0.3, 8.0, -0.2]))
    u = np.ones(3) / np.sqrt(3.0)
    if kind == "onplane":
        r = 10.0 ** rng.uniform(-2, -0.3, n)
        pos = np.zeros((n, 3))
        for k in range(n):
            q = np.array([rng.uniform(-2, 2), 0.001, rng.uniform(-2, 2)])           # a floor point's shadow-ray origin
            l = lightp - q
            l /= np.linalg.norm(l)
            nrm = np.cross(l, u)
            nrm /= np.linalg.norm(nrm)
            along = q + l * rng.uniform(1.0, 6.0) + u * rng.uniform(-0.3, 0.3)     # a point of the fan's plane
            eps = 10.0 ** rng.uniform(-6, -2) * rng.choice([-1.0, 1.0])
            pos[k] = along + nrm * r[k] * (1.0 + eps) * rng.choice([-1.0, 1.0])
        pos[:, 1] = np.maximum(pos[:, 1], r + 0.01)
    elif kind == "tiny":
        r = 10.0 ** rng.uniform(-3, -1.5, n)
        pos = np.stack([rng.uniform(-2, 2, n), rng.uniform(0.05, 1.5, n), rng.uniform(-2, 2, n)], 1)
    else:
        r = 10.0 ** rng.uniform(-2, 0.2, n)
        pos = np.stack([rng.uniform(-3, 3, n), rng.uniform(0.3, 5, n), rng.uniform(-3, 3, n)], 1)
        pos[:, 1] = np.maximum(pos[:, 1], r + 0.01)
    objs["position"][:n] = (pos * s).astype(np.float32) + off
    objs["radius"][:n] = (r * s).astype(np.float32)
    objs["albedo"][:n] = 0.7
    objs["roughness"][:n] = 0.4
    objs["type"][n] = L.PLANE
    objs["position"][n] = off
    objs["normal"][n] = (0, 1, 0)
    objs["size"][n] = (4000 * s, 4000 * s)
    objs["albedo"][n] = 0.8
    objs["diffuseStrength"][n] = 0.7
    from opengl_raytracing_amd import host as H
    H.generate_aabb(objs)
    lts = L.default_lights(1)
    lts["type"] = ltype
    lts["position"] = (lightp * s).astype(np.float32) + off
    lts["direction"] = (-1.0, -1.0, -1.0) if (ltype == L.DIRECTIONAL and kind == "diag") else (-0.1, -1.0, 0.05) if ltype == L.DIRECTIONAL else (0.0, 1.0, 0.0)
    lts["intensity"] = 30.0 * float(s) * float(s) if ltype == L.AREA else 6.0
    lts["shadowType"] = L.SHADOW_PCSS
    lts["pcfSamples"] = 4
    lts["lightSize"] = light_size
    cam = dict(cam_pos=tuple((np.array([0.0, 9.0, 0.3], dtype=np.float32) * s + off).tolist()), cam_dir=(0.0, -1.0, 0.0),
               cam_up=(0.0, 0.0, -1.0), cam_right=(1.0, 0.0, 0.0), fov_deg=40.0)
    return scenes.Scene(f"fan-{kind}", objs, lts, 96, 64, 2, cam)


@pytest.mark.parametrize("kind", ["onplane", "diag", "tiny", "mixed"])
def test_pcss_blocker_fans_grazing_spheres(tracer, host, oracle, kind):
    """pcssShadow's blocker search (16 rays per light in the plane of lightDir and (1,1,1), traced four per packet with a shared
    reciprocal box and candidate mask) on grazing geometry: spheres tangent to the fans' planes within 1e-6 .. 1e-2 of their radius,
    a light along (1,1,1) (degenerate fan), tiny and mixed spheres; light sizes 0.02 .. 3 (fans of +-0.4 degrees to wider than a
    right angle); scales 1 / 1e3 / 1e-2 and offsets up to 1e5; point / area / directional lights -- bit for bit.  (Written for a
    per-lane fan cull that was measured slower and removed, rt_packet.inc; kept as the PCSS counterpart of the PCF grazing test.)"""
    k = 0
    for scale, offset in [(1.0, (0, 0, 0)), (1.0, (1e4, -3e3, 2e4)), (1e3, (0, 0, 0)), (1.0, (1e5, 1e5, -1e5)), (1e-2, (50.0, 0.0, -20.0))]:
        for light_size, ltype in [(1.0, L.POINT), (0.02, L.AREA), (1.4, L.POINT), (1.0, L.DIRECTIONAL), (0.3, L.AREA), (1.5, L.POINT), (3.0, L.DIRECTIONAL)]:
            k += 1
            if (k + len(kind)) % 2:
                continue
            sc = _blocker_fan_scene(kind, scale, offset, light_size, ltype, seed=100 + k)
            p = sc.params()
            gpu = render_gpu(tracer, sc, p)
            cpu = oracle.render(sc, p)
            assert_bit_exact(gpu, cpu, f"{kind} scale {scale} offset {offset} lightSize {light_size} light {ltype}")
            assert tracer.count_rays(p) == cpu[3]


@pytest.mark.parametrize("cfg", [3, 4, 5])
def test_whole_frames_packet_kernel_equals_exhaustive_kernel(host, oracle, cfg):
    """VERDICT r2 #4a: C3, C4, C5 at their REAL sizes (3840x2160, 7680x4320), whole frame: the packet kernel (shadow tables, packet
    and per-lane culls, predicted / measured tile order) against the exhaustive kernel (every object for every ray, raster order)
    -- two independently structured kernels, the second one checked against the oracle on windows of the same frames -- all three
    surfaces bit for bit on the device, equal ray counts; plus 64 random 32x32 windows of the frame against the oracle."""
    import torch
    from opengl_raytracing_amd import dist as D
    sc = scenes.make_scene(cfg, host.generate_aabb)
    p = sc.params()
    W, H = sc.width, sc.height
    one = D.StripPlan(W, H, H, 1)
    outs = []
    rays = []
    for variant in (1, 0):
        with host.RayTracer(0) as rt:
            rt.load(sc)
            rt.set_variant(variant)
            buf = D.alloc_rank_buffer(one, "cuda")
            c, q, n = D.surface_views(buf, one)
            rt.render_to(p, c.data_ptr(), q.data_ptr(), n.data_ptr())
            if variant == 1:      # a second and third frame: the measured-cost order replaces the predicted one
                rt.render_to(p, c.data_ptr(), q.data_ptr(), n.data_ptr())
                rt.render_to(p, c.data_ptr(), q.data_ptr(), n.data_ptr())
            rt.sync()
            torch.cuda.synchronize()
            outs.append((c, q, n))
            rays.append(rt.count_rays(p))
    assert rays[0] == rays[1]
    for a, b, name in zip(outs[0], outs[1], ("gColor", "gPosition", "gNormal")):
        it = torch.int16 if a.dtype == torch.float16 else torch.int32
        same = torch.equal(a.view(it), b.view(it))
        if not same:          # NaN payloads may differ: compare as floats with NaN == NaN
            fa, fb = a.float(), b.float()
            same = bool((((fa == fb) | (fa.isnan() & fb.isnan()))).all().item())
        assert same, f"C{cfg} {W}x{H}: {name} of the packet kernel differs from the exhaustive kernel's"
    rng = np.random.default_rng(100 + cfg)
    col, pos, nrm = (t.cpu().numpy() for t in outs[0])
    for _ in range(64):
        x0, y0 = int(rng.integers(0, W - 32)), int(rng.integers(0, H - 32))
        oc, op, on, _ = oracle.render(sc, sc.params(window=(x0, y0, 32, 32)))
        assert_bit_exact((col[y0:y0 + 32, x0:x0 + 32], pos[y0:y0 + 32, x0:x0 + 32], nrm[y0:y0 + 32, x0:x0 + 32]), (oc, op, on),
                         f"C{cfg} window @({x0},{y0}) of the whole frame")
