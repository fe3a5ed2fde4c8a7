"""The three scene files the reference ships (tests/golden/scenes: default, SIMPLE, performance_test), as the reference's own
shader draws them on llvmpipe (fixtures ref_default / ref_simple / ref_performance_test and ref_frame_*, written by
tests/golden/make_golden.py --only refscenes,ref_frame), against the parser and the oracle.  CPU only; reads fixtures only.

What these files hold that no generated scene does: default.scene's older column order (ior 0, metallic 0.924, albedo.r 0),
metals of roughness 0 and a line one token short, a camera inside a closed room (every primary ray hits), 15 objects under 8
lights of all three types with `samples` 0, 1 and 16, planes that carry a radius of 1 and -1, and a square frame at depth 3.
(performance_test's "LeftWall -10 0 0 1 1 0 0" reads as position, radius 1, normal (1, 0, 0): every plane normal of the three
files IS of unit length, and an oracle that normalised a plane's normal before intersecting passed every case of these files --
and the `nan` fixture, whose normal (0, 0, 2) scales exactly.  Hence one case beyond the files, `wall_tilted` of
ref_performance_test: that scene with the two walls' normals set to (1, 1, 0) and (-1, -1, 0).)

Gates: those of tests/test_oracle_golden.py at their strictest -- gPosition / gNormal bit for bit and gColor within
compare_surface's 1e-4 on EVERY pixel (NaN == NaN), for all stored views and settings; the post chain with the gates of
tests/test_bloom.py (case a) and tests/test_taa.py.  The helpers below are shared with the GPU tests (tests/test_refscenes.py).
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, GoldenScene, compare_surface, load_golden, params_from_bytes
from opengl_raytracing_amd import layout as L
from test_taa import _local_max

SCENE_FILES = {"ref_default": "default.scene", "ref_simple": "SIMPLE.scene", "ref_performance_test": "performance_test.scene"}
VIEWS = ["shipped", "down", "corner", "inglass", "behind", "steep"]
SETTINGS = {"noshadow": (1, L.SHADOW_NONE), "pcss": (8, L.SHADOW_PCSS)}       # setting -> (depth, shadowType of every light)
CASES = VIEWS + [f"{v}_{s}" for v in ("shipped", "steep") for s in SETTINGS]
# one more in ref_performance_test: LeftWall / RightWall with the normals (1, 1, 0) / (-1, -1, 0), NOT of unit length, from a pose
# that faces LeftWall (the fixture's `tilted_objects`; see the module docstring)
EXTRA_CASES = {"ref_performance_test": ["wall_tilted"]}


def cases_of(name):
    return CASES + EXTRA_CASES.get(name, [])
REF_GATES = (1.0, 1.0)          # min bit-exact fraction of gPosition and of gNormal, min fraction of gColor within 1e-4
FRAME_FIXTURES = ["ref_frame_default", "ref_frame_performance_test"]


def case_scene(g, case):
    """The scene a stored case was rendered from: the parsed file, with the setting's lights where the case has one."""
    sc = GoldenScene(g)
    setting = case.split("_")[1] if "_" in case else None
    if case == "wall_tilted":
        sc.objects = np.frombuffer(g["tilted_objects"].tobytes(), dtype=L.OBJECT_DTYPE).copy()
    if setting in SETTINGS:
        sc.lights = np.frombuffer(g[f"{setting}_lights"].tobytes(), dtype=L.LIGHT_DTYPE).copy()
    return sc


def reference_fractions(surfaces, g, prefix, index=None):
    """(gPosition exact, gNormal exact, gColor within 1e-4) pixel COUNTS of `surfaces` against the stored reference pixels."""
    col, pos, nrm = surfaces[:3]
    ref = [g[f"{prefix}_{k}"] if index is None else g[f"{prefix}_{k}"][index] for k in ("color", "pos", "normal")]
    ep = compare_surface(pos, ref[1], rtol=0, atol=0)["exact_mask"].sum()
    en = compare_surface(nrm.astype(np.float32), ref[2].astype(np.float32), rtol=0, atol=0)["exact_mask"].sum()
    cc = compare_surface(col, ref[0])
    nan_same = (np.isnan(col).any(axis=-1) == np.isnan(ref[0]).any(axis=-1)).all()
    return int(ep), int(en), int(cc["ok_mask"].sum()), bool(nan_same)


def assert_reference_gates(name, what, counts, n_px):
    ep, en, okc, nan_same = counts
    print(f"{name} {what}: vs reference: gPosition exact {ep / n_px:.6f} gNormal exact {en / n_px:.6f} gColor 1e-4 {okc / n_px:.6f} ({n_px} px)")
    assert ep / n_px >= REF_GATES[0], f"{name} {what}: gPosition bit-exact on {ep / n_px:.6f}"
    assert en / n_px >= REF_GATES[0], f"{name} {what}: gNormal bit-exact on {en / n_px:.6f}"
    assert okc / n_px >= REF_GATES[1], f"{name} {what}: gColor within 1e-4 on {okc / n_px:.6f} ({n_px - okc} px)"
    assert nan_same, f"{name} {what}: the NaN pixels are not the reference's"


def assert_bloom_gates(st, out, g, what):
    """tests/test_bloom.py's gates of its power-of-two case: extract bit for bit; every blur stage >= 99 % of pixels bit-exact and
    the rest within half an fp16 ulp plus the neighbourhood term; the fp32 combine within 1.5e-3 relative, >= 90 % bit-exact."""
    stages, comb = g["stages"], g["combined"]
    assert len(st) == len(stages) == 11
    e0 = (st[0].view(np.uint16) == stages[0].view(np.uint16)).all(axis=-1)
    assert e0.all(), f"{what} extract: exact {e0.mean():.6f}"
    fracs = [1.0]
    for k in range(1, 11):
        a, b = st[k].astype(np.float32)[..., :3], stages[k].astype(np.float32)[..., :3]
        exact = (a == b).all(axis=-1).mean()
        fracs.append(float(exact))
        assert exact >= 0.99, f"{what} stage {k}: exact {exact:.4f}"
        local = np.abs(stages[k - 1].astype(np.float32)[..., :3]).max()
        assert (np.abs(a - b) <= np.maximum(np.abs(a), np.abs(b)) / 1024 + 4e-6 * local + 1e-7).all(), f"{what} stage {k}"
        assert (st[k].view(np.uint16)[..., 3] == 0x3C00).all()
    err = np.abs(out - comb)
    exact_c = (out == comb).all(axis=-1).mean()
    print(f"{what}: bloom stages exact min {min(fracs):.6f}, combine exact {exact_c:.6f}, max rel err "
          f"{float((err / np.maximum(np.maximum(np.abs(out), np.abs(comb)), 1e-30)).max()):.3g}")
    assert (err <= 1.5e-3 * np.maximum(np.abs(out), np.abs(comb)) + 1e-6).all(), f"{what} combine"
    assert exact_c >= 0.9, f"{what} combine: exact {exact_c:.4f}"


def assert_taa_gates(out, g, k, what):
    """tests/test_taa.py's gates on TAA frame k of a ref_frame fixture."""
    cur, his, ref = g[f"taa{k}_current"], g[f"taa{k}_history"], g[f"taa{k}_out"]
    M = np.maximum(_local_max(cur), _local_max(his))[..., None]
    err = np.abs(out.astype(np.float64) - ref)
    ok = (err <= 1e-5 * np.maximum(np.abs(out), np.abs(ref)) + 8e-6 * M + 1e-7).all(axis=-1)
    exact = (out == ref).all(axis=-1).mean()
    print(f"{what} TAA frame {k}: pass {ok.mean():.6f} exact {exact:.6f}")
    assert ok.mean() >= 0.999, f"{what} TAA frame {k}: pass {ok.mean():.5f}"
    assert exact >= 0.6, f"{what} TAA frame {k}: exact {exact:.3f}"
    border = np.ones(out.shape[:2], bool)
    border[1:-1, 1:-1] = False
    assert ok[border].mean() >= 0.99
    assert (out[..., 3] == 1).all()


# ---- parser ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENE_FILES))
def test_parser_gives_the_fixtures_bytes(host, name):
    """host.parse_scene on the committed scene file = the objects and lights the reference pixels were rendered from, byte for
    byte (AABBs included): parser drift fails here, not as a colour difference somewhere."""
    g = load_golden(name)
    objs, lts = host.parse_scene(open(os.path.join(GOLDEN_DIR, "scenes", SCENE_FILES[name])).read())
    assert objs.tobytes() == g["objects"].tobytes(), f"{name}: objects"
    assert lts.tobytes() == g["lights"].tobytes(), f"{name}: lights"


def test_the_scene_files_keep_their_unusual_inputs():
    """What makes these files worth their fixtures is in the bytes under test (module docstring)."""
    perf = GoldenScene(load_golden("ref_performance_test"))
    assert len(perf.objects) == 15 and len(perf.lights) == 8
    assert sorted(set(perf.lights["type"].tolist())) == sorted([L.DIRECTIONAL, L.POINT, L.AREA])
    assert sorted(set(perf.lights["samples"].tolist())) == [0, 1, 16]
    planes = perf.objects[perf.objects["type"] == L.PLANE]
    assert sorted(planes["radius"].tolist()) == [-1.0, 0.0, 0.0, 0.0, 1.0], "LeftWall / RightWall: a radius the shader never reads"
    for sc in (perf, GoldenScene(load_golden("ref_simple")), GoldenScene(load_golden("ref_default"))):
        pl = sc.objects[sc.objects["type"] == L.PLANE]
        assert ((pl["normal"].astype(np.float64) ** 2).sum(axis=1) == 1.0).all()      # see the module docstring
    dflt = GoldenScene(load_golden("ref_default"))
    assert dflt.objects[0]["ior"] == 0 and dflt.objects[0]["albedo"][0] == 0 and np.isclose(dflt.objects[0]["metallic"], 0.924)
    simple = GoldenScene(load_golden("ref_simple"))
    metals = simple.objects[(simple.objects["type"] == L.SPHERE) & (simple.objects["mat_type"] == L.MATERIAL_METALLIC)]
    assert len(metals) == 4 and (metals["roughness"] == 0).all() and (metals["ior"] == 0).all()


# ---- rays -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,case", [(n, c) for n in SCENE_FILES for c in cases_of(n)])
def test_views_against_reference(oracle, name, case):
    g = load_golden(name)
    assert list(g["cases"]) == cases_of(name)
    sc = case_scene(g, case)
    p = params_from_bytes(g[f"{case}_params"])
    depth, stype = SETTINGS.get(case.split("_")[-1], (3, None))
    if case == "wall_tilted":
        n = g[f"{case}_normal"].astype(np.float32)
        on_walls = ((np.abs(n[..., 0]) == 1) & (np.abs(n[..., 1]) == 1)).mean()
        print(f"{name} {case}: {on_walls:.4f} of the last hits lie on the unnormalised walls")
        assert on_walls >= 0.25
    assert (p.width, p.height, p.fovDeg, p.maxRayDepth) == (p.regionW, p.regionH, 45.0, depth)
    if stype is not None:
        assert (sc.lights["shadowType"] == stype).all()
    got = oracle.render(sc, p)
    assert_reference_gates(name, case, reference_fractions(got, g, case), p.width * p.height)
    # the case has not turned into a trivial one
    ref_col, ref_nrm = g[f"{case}_color"], g[f"{case}_normal"].astype(np.float32)
    hit = (ref_nrm[..., :3] != 0).any(axis=-1).mean()
    reds = len(np.unique(ref_col[..., 0][~np.isnan(ref_col[..., 0])]))
    nan_px = int(np.isnan(ref_col).any(axis=-1).sum())
    print(f"{name} {case}: hit fraction {hit:.4f}, {reds} distinct red values, {nan_px} NaN px")
    assert reds >= 1000
    if case == "shipped" and name != "ref_default":
        assert hit == 1.0, "the camera is inside the closed room: every primary ray hits"
    if case.endswith("_pcss") and name != "ref_default":
        assert nan_px >= 1, "depth 8 with PCSS on every light reaches the reference's NaN corners in this scene"


@pytest.mark.parametrize("name", list(SCENE_FILES))
def test_framecount_7_gives_the_shipped_bytes(oracle, name):
    """frameCount reaches the image through the noise texture's coordinates (none is bound) and through the diffuse bounce's
    hammersley index (the file format carries no diffuseStrength, so it stays 0 on every object): llvmpipe's frame of frameCount 7
    IS the stored `shipped` frame (asserted by the generator), and so must the oracle's be."""
    g = load_golden(name)
    p7 = params_from_bytes(g["shipped_fc7_params"])
    assert p7.frameCount == 7 and bytes(L.copy_params(p7, frameCount=0)) == g["shipped_params"].tobytes()
    sc = GoldenScene(g)
    assert (sc.objects["diffuseStrength"] == 0).all()
    got = oracle.render(sc, p7)
    assert_reference_gates(name, "shipped, frameCount 7", reference_fractions(got, g, "shipped"), p7.width * p7.height)
    base = oracle.render(sc, params_from_bytes(g["shipped_params"]))
    for a, b in zip(got[:3], base[:3]):
        assert np.array_equal(a, b, equal_nan=True)
    assert got[3] == base[3]


@pytest.mark.parametrize("name", list(SCENE_FILES))
def test_windows_of_the_800x800_frame_against_reference(oracle, name):
    """Eight 32x32 windows of the frame at the reference's real size (800x800: square, where every config scene is 16:9)."""
    g = load_golden(name)
    sc = GoldenScene(g)
    base = params_from_bytes(g["win_params"])
    assert (base.width, base.height, base.maxRayDepth) == (800, 800, 3) and tuple(g["full_size"]) == (800, 800)
    tot = np.zeros(3, dtype=np.int64)
    nan_same = True
    for k, (x0, y0) in enumerate(g["win_origins"]):
        p = L.copy_params(base, x0=int(x0), y0=int(y0), regionW=32, regionH=32)
        ep, en, okc, ns = reference_fractions(oracle.render(sc, p), g, "win", k)
        tot += (ep, en, okc)
        nan_same &= ns
    assert_reference_gates(name, "800x800 windows", (*tot, nan_same), 8 * 32 * 32)


# ---- post chain -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FRAME_FIXTURES)
def test_bloom_chain_on_the_reference_frame(oracle, name):
    """extract -> ten blurs -> combine on llvmpipe's own raytraced frame.  At 128x128 every stage of the oracle equals
    llvmpipe's bit for bit here; the gates stay those of tests/test_bloom.py."""
    g = load_golden(name)
    assert g["scene"].shape == (128, 128, 4)
    out, st = oracle.bloom(g["scene"], 1.0, 0.5, 10, keep=True)
    assert_bloom_gates(st, out, g, name)
    assert (g["scene"][..., :3] > 1.0).any(), "nothing above the bloom threshold: the chain would be the identity"


@pytest.mark.parametrize("name", FRAME_FIXTURES)
def test_taa_frames_on_the_reference_frame(oracle, host, name):
    """Three TAA frames (frameCount 0, 1, 2) with the reference's default blend factor, each fed the fixture's own inputs."""
    g = load_golden(name)
    assert float(g["blend"]) == float(np.float32(0.1))
    assert not g["taa0_history"].any(), "the history starts as zeros"
    for k in range(3):
        fc, blend, jx, jy = g[f"taa{k}_params"]
        assert int(fc) == k and (float(jx), float(jy)) == host.taa_jitter(k, 128, 128) and blend == g["blend"]
        if k:
            assert np.array_equal(g[f"taa{k}_history"], g[f"taa{k - 1}_out"], equal_nan=True), "history ping-pong"
        out = oracle.taa_resolve(g[f"taa{k}_current"], g[f"taa{k}_history"], g[f"taa{k}_normal"], float(blend), float(jx), float(jy))
        assert_taa_gates(out, g, k, name)


@pytest.mark.parametrize("name", FRAME_FIXTURES)
def test_the_oracles_frame_feeds_the_chain_like_the_references(oracle, name):
    """The frame the chain starts from: the oracle's render of the fixture's scene against llvmpipe's `scene` / gNormal."""
    g = load_golden(name)
    p = params_from_bytes(g["params"])
    col, _, nrm, _ = oracle.render(GoldenScene(g), p)
    cc = compare_surface(col, g["scene"])
    en = compare_surface(nrm.astype(np.float32), g["taa0_normal"].astype(np.float32), rtol=0, atol=0)
    print(f"{name}: frame vs reference: gColor 1e-4 {cc['pass_frac']:.6f} gNormal exact {en['exact_frac']:.6f}")
    assert cc["pass_frac"] >= REF_GATES[1] and en["exact_frac"] >= REF_GATES[0]
