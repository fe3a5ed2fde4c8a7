"""GPU tests on the three scene files the reference ships (fixtures ref_default / ref_simple / ref_performance_test and
ref_frame_*: the reference's own shaders on llvmpipe, tests/golden/make_golden.py --only refscenes,ref_frame).  Both kernel
variants (conftest's `tracer`); nothing outside the repository is read.

* HIP vs oracle: bit for bit on all three surfaces, equal ray counts -- a difference is a kernel or host bug.
* HIP vs the reference's pixels, directly: gPosition / gNormal bit for bit and gColor within 1e-4 on every pixel
  (tests/test_refscenes_oracle.py's REF_GATES, where the inputs these files add are listed).
* The same inputs through the rest of the ABI: window parameters at 800x800, whole 800x800 frames of both kernels, ray
  queries, picking, ray shading, scene switches between 3 and 8 lights on one context, and rt_frame's post chain.
"""
import numpy as np
import pytest

from conftest import GoldenScene, bits_equal, load_golden, params_from_bytes
from opengl_raytracing_amd import layout as L
from test_frame import _d2h
from test_gpu_parity import assert_bit_exact
from test_query import _gbuffer_check
from test_refscenes_oracle import (FRAME_FIXTURES, SCENE_FILES, assert_reference_gates, assert_taa_gates, case_scene, cases_of,
                                   reference_fractions)

pytestmark = pytest.mark.gpu

NAMES = list(SCENE_FILES)


def _render(tracer, sc, p):
    tracer.load(sc)
    tracer.render(p)
    return tracer.readback()


def _same(a, b, what):
    for x, y, s in zip(a[:3], b[:3], ("gColor", "gPosition", "gNormal")):
        assert bits_equal(x.astype(np.float32), y.astype(np.float32)), f"{what}: {s} differs"


@pytest.mark.parametrize("name", NAMES)
def test_every_stored_view(tracer, oracle, name):
    """Six views, `shipped` and `steep` also without shadows at depth 1 and with PCSS everywhere at depth 8 (and performance_test
    with two walls' normals off unit length, `wall_tilted`): against the oracle
    (bits, ray count) and against the reference's pixels; frameCount 7 gives the `shipped` bytes (no noise texture is bound, no
    object has a diffuseStrength)."""
    g = load_golden(name)
    shipped = None
    for case in cases_of(name):
        sc = case_scene(g, case)
        p = params_from_bytes(g[f"{case}_params"])
        gpu = _render(tracer, sc, p)
        cpu = oracle.render(sc, p)
        assert_bit_exact(gpu, cpu, f"{name} {case}")
        assert tracer.count_rays(p) == cpu[3], f"{name} {case}: ray count"
        assert_reference_gates(name, f"{case} (HIP)", reference_fractions(gpu, g, case), p.width * p.height)
        if case == "shipped":
            shipped = gpu
    p7 = params_from_bytes(g["shipped_fc7_params"])
    assert p7.frameCount == 7
    _same(_render(tracer, GoldenScene(g), p7), shipped, f"{name} frameCount 7 vs frameCount 0")


@pytest.mark.parametrize("name", NAMES)
def test_windows_of_the_800x800_frame(tracer, oracle, name):
    """Eight 32x32 windows of the reference's real frame through the ABI's window parameters: the reference's pixels, the oracle's bits."""
    g = load_golden(name)
    sc = GoldenScene(g)
    tracer.load(sc)
    base = params_from_bytes(g["win_params"])
    assert (base.width, base.height) == (800, 800)
    tot = np.zeros(3, dtype=np.int64)
    nan_same = True
    for k, (x0, y0) in enumerate(g["win_origins"]):
        p = L.copy_params(base, x0=int(x0), y0=int(y0), regionW=32, regionH=32)
        tracer.render(p)
        gpu = tracer.readback()
        assert_bit_exact(gpu, oracle.render(sc, p), f"{name} window @({x0},{y0})")
        ep, en, okc, ns = reference_fractions(gpu, g, "win", k)
        tot += (ep, en, okc)
        nan_same &= ns
    assert_reference_gates(name, "800x800 windows (HIP)", (*tot, nan_same), 8 * 32 * 32)


@pytest.mark.parametrize("name", NAMES)
def test_whole_800x800_frame_packet_kernel_equals_exhaustive_kernel(host, oracle, name):
    """The frame at the reference's real size, square where every config scene is 16:9: the packet kernel (three frames, so the
    measured tile order replaces the predicted one) against the exhaustive kernel, bit for bit with equal ray counts; for
    default.scene also the whole frame against the oracle."""
    g = load_golden(name)
    sc = GoldenScene(g)
    p = params_from_bytes(g["win_params"])
    outs, rays = [], []
    for variant in (1, 0):
        with host.RayTracer(0) as rt:
            rt.set_variant(variant)
            rt.load(sc)
            for _ in range(3 if variant == 1 else 1):
                rt.render(p)
            outs.append(rt.readback())
            rays.append(rt.count_rays(p))
    assert rays[0] == rays[1]
    _same(outs[0], outs[1], f"{name} 800x800 packet vs exhaustive")
    for k, (x0, y0) in enumerate(g["win_origins"]):      # and the frame holds the reference's windows where they were cut
        crop = tuple(s[y0:y0 + 32, x0:x0 + 32] for s in outs[0])
        ep, en, okc, ns = reference_fractions(crop, g, "win", k)
        assert (ep, en, okc, ns) == (1024, 1024, 1024, True), f"{name} window {k} of the whole frame"
    if name == "ref_default":
        cpu = oracle.render(sc, p)
        assert_bit_exact(outs[0], cpu, "default.scene 800x800")
        assert rays[0] == cpu[3]


@pytest.mark.parametrize("name", NAMES)
def test_queries_reproduce_the_references_gbuffer(tracer, oracle, name):
    """camera_rays -> trace_rays("closest") against llvmpipe's gPosition and gNormal themselves, on the two stored depth-1 frames
    (the shader stores the LAST hit of the path, raytracingCs.glsl:582-583: only at depth 1 is that the camera ray's); any-hit
    agrees on hit or miss; pick equals both.  From inside the glass sphere: against a depth-1 render of that view."""
    import torch
    g = load_golden(name)
    inglass = L.copy_params(params_from_bytes(g["inglass_params"]), maxRayDepth=1)
    _gbuffer_check(tracer, oracle, GoldenScene(g), inglass, f"{name} inglass at depth 1")
    for case in ("shipped_noshadow", "steep_noshadow"):
        p = params_from_bytes(g[f"{case}_params"])
        assert p.maxRayDepth == 1
        H, W = p.height, p.width
        rays = tracer.camera_rays(p)
        hits = tracer.trace_rays(rays, "closest")
        anyh = tracer.trace_rays(rays, "any")
        torch.cuda.synchronize()
        h = hits.cpu().numpy().view(L.HIT_DTYPE).reshape(H, W)
        ref_pos, ref_nrm = g[f"{case}_pos"], g[f"{case}_normal"]
        assert bits_equal(h["position"], ref_pos[..., :3]), f"{name} {case}: hit position != the reference's gPosition"
        assert (oracle.float_to_half_rtz(h["normal"]) == ref_nrm[..., :3].view(np.uint16)).all(), f"{name} {case}: hit normal != gNormal"
        hit = (ref_nrm[..., :3].astype(np.float32) != 0).any(axis=-1)
        assert ((h["object"] >= 0) == hit).all() and (anyh.cpu().numpy() == hit).all(), f"{name} {case}: hit or miss"
        rng = np.random.default_rng(len(name))
        pts = [(0, 0), (W - 1, H - 1), (W // 2, H // 2)] + [(int(x), int(y)) for x, y in zip(rng.integers(0, W, 5), rng.integers(0, H, 5))]
        for x, y in pts:
            k = tracer.pick(p, x, y)
            e = h[y, x]
            assert k.object == e["object"] and bits_equal(np.float32(k.t), e["t"]) and bits_equal(k.normal, e["normal"]), (name, case, x, y)
            assert bits_equal(k.position, ref_pos[y, x, :3]), (name, case, x, y)


@pytest.mark.parametrize("name", NAMES)
def test_shading_the_camera_rays_gives_the_rendered_frame(tracer, name):
    """shade_rays on camera_rays(p) = render(p), bit for bit, on the file's own lights, with PCSS on all of them at depth 8, and
    from inside the glass sphere."""
    import torch
    g = load_golden(name)
    for case in ("shipped", "shipped_pcss", "inglass"):
        sc = case_scene(g, case)
        p = params_from_bytes(g[f"{case}_params"])
        want = _render(tracer, sc, p)
        col, pos, nrm = tracer.shade_rays(p, tracer.camera_rays(p))
        torch.cuda.current_stream().synchronize()
        _same((col.cpu().numpy(), pos.cpu().numpy(), nrm.cpu().numpy()), want, f"{name} {case}: shade_rays vs render")


def test_switching_between_the_scene_files_on_one_context(tracer, oracle):
    """default -> performance_test -> default -> SIMPLE on one context, `shipped` rendered after each load: 3 -> 8 -> 3 lights
    switches the kernel instantiation and rebuilds the shadow tables.  Every render is the oracle's; a scene that comes back
    renders its first result again; uploading the very same scene again changes nothing."""
    first = {}
    for name in ("ref_default", "ref_performance_test", "ref_default", "ref_simple"):
        g = load_golden(name)
        sc = GoldenScene(g)
        p = params_from_bytes(g["shipped_params"])
        tracer.set_scene(sc.objects, sc.lights)
        tracer.set_noise(None)
        tracer.set_skybox(None)
        tracer.render(p)
        got = tracer.readback()
        if name in first:
            _same(got, first[name], f"{name} after another scene")
        else:
            first[name] = got
            assert_bit_exact(got, oracle.render(sc, p), f"{name} after a scene switch")
        tracer.set_scene(sc.objects, sc.lights)
        tracer.render(p)
        _same(tracer.readback(), got, f"{name} uploaded twice")
    assert [len(GoldenScene(load_golden(n)).lights) for n in ("ref_default", "ref_performance_test", "ref_simple")] == [3, 8, 3]


@pytest.mark.parametrize("name", FRAME_FIXTURES)
def test_frame_chain_on_the_reference_scenes(tracer, host, oracle, name):
    """rt_frame, three frames (frameCount 0, 1, 2) with AO and TAA on and the reference's default blend factor: the chain composed
    from the oracle's pieces bit for bit (tests/test_frame.py's pattern); the display against llvmpipe's combine of its own frame
    with tests/test_bloom.py's combine gate, and the history of frame 0 against llvmpipe's with tests/test_taa.py's gates."""
    import torch
    g = load_golden(name)
    sc = GoldenScene(g)
    base = params_from_bytes(g["params"])
    w, h = base.width, base.height
    blend = float(g["blend"])
    tracer.load(sc)
    # the context keeps its history across frames of one size, as the reference's window does, and other tests have left theirs:
    # one frame of another size first, so that this chain starts from zeros like the fixture's
    tracer.frame(L.copy_params(base, width=16, height=16, regionW=16, regionH=16), enable_ao=False, enable_taa=False)
    samples, noise = host.ssao_kernel()
    hist = [np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)]
    d_disp = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    for frame in range(3):
        p = L.copy_params(base, frameCount=frame)
        tracer.frame(p, enable_ao=True, enable_taa=True, taa_blend=blend, ao_samples=samples, ao_noise=noise, d_display=d_disp.data_ptr())
        tracer.sync()
        col, pos, nrm, _ = oracle.render(sc, p)
        nrm16 = np.ascontiguousarray(nrm).view(np.float16).reshape(h, w, 4)
        view, proj = host.camera_matrices(p.camPos[:], p.camDir[:], p.camUp[:], p.fovDeg, w / h)
        want_ao = oracle.ssao_blur(oracle.ssao(pos, nrm16, noise, samples, proj, view), False)
        want_disp = oracle.bloom(col, 1.0, 0.5, 10)
        d_c, d_p, d_n, d_ao, d_hist = tracer.frame_surfaces()
        assert bits_equal(_d2h(d_c, (h, w, 4), np.float32), col), f"{name} gColor frame {frame}"
        assert bits_equal(_d2h(d_ao, (h, w), np.float32), want_ao), f"{name} AO frame {frame}"
        disp = d_disp.cpu().numpy()
        assert bits_equal(disp, want_disp), f"{name} display frame {frame}"
        cur = frame % 2
        jx, jy = oracle.taa_jitter(frame, w, h)
        hist[cur] = oracle.taa_resolve(col, hist[1 - cur], nrm16.astype(np.float32), blend, jx, jy)
        got_hist = _d2h(d_hist, (h, w, 4), np.float32)
        assert bits_equal(got_hist, hist[cur]), f"{name} history frame {frame}"
        if frame == 0:
            comb = g["combined"]
            err = np.abs(disp - comb)
            exact = (disp == comb).all(axis=-1).mean()
            print(f"{name}: display vs reference: exact {exact:.6f}, max rel err {float((err / np.maximum(np.abs(comb), 1e-30)).max()):.3g}")
            assert (err <= 1.5e-3 * np.maximum(np.abs(disp), np.abs(comb)) + 1e-6).all(), f"{name}: display vs the reference's combine"
            assert exact >= 0.9, f"{name}: display bit-exact on {exact:.4f}"
            assert_taa_gates(got_hist, g, 0, f"{name} (HIP)")
