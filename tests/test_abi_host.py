"""CPU-only tests of the drop-in boundary: the C-ABI library loads and exports every symbol
include/rt_mi355.h declares, the byte layouts match the reference's structs
(/root/reference/src/Object.h:13-21, Material.h:11-23, Light.h:7-20),
and the host-side feeders (AABB generation, camera vectors, scene text parser) behave like
the reference's host code.  No compute call is made here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN_DIR, load_golden
from opengl_raytracing_amd import layout as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rt_mi355.h")


def declared_symbols():
    from test_binding_host import prototypes
    return sorted({p.name for p in prototypes(HEADER)})


def test_library_exports_every_declared_symbol(host):
    lib = host.load_library()
    syms = declared_symbols()
    assert len(syms) >= 19
    for s in syms:
        assert hasattr(lib, s), f"librt_mi355.so does not export {s}"
    assert sorted(host.EXPORTS) == syms


def test_header_compiles_as_c_and_asserts_layout(tmp_path):
    """The static_asserts in the header (every Appendix-B offset) hold under a plain C compiler."""
    src = tmp_path / "t.c"
    src.write_text('#include "rt_mi355.h"\nint main(void){return sizeof(rt_object)==176 && sizeof(rt_light)==96 ? 0 : 1;}\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_numpy_dtypes_match_appendix_b():
    o = L.OBJECT_DTYPE
    assert o.itemsize == 176
    exp = dict(type=0, position=16, radius=28, normal=32, size=48, mat_type=64, albedo=80, metallic=92,
               roughness=96, diffuseStrength=100, ior=104, transparency=108, specular=112,
               subsurfaceScatter=116, subsurfaceColor=128, scatterDistance=140, bounds_min=144, bounds_max=160)
    for k, v in exp.items():
        assert o.fields[k][1] == v, k
    l = L.LIGHT_DTYPE
    assert l.itemsize == 96
    exp = dict(type=0, position=16, direction=32, color=48, intensity=60, radius=64, samples=68,
               shadowSoftness=72, shadowType=76, pcfSamples=80, lightSize=84, angularRadius=88)
    for k, v in exp.items():
        assert l.fields[k][1] == v, k
    assert ctypes.sizeof(L.RtParams) == 128


def test_no_device_is_reported_not_faked(host):
    """Without a GPU rt_create must fail with RT_ERR_NO_DEVICE -- there is no CPU fallback."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(host.RtError) as e:
        host.RayTracer(0)
    assert e.value.code in (-2, -3)


def test_generate_aabb_matches_oracle_and_rule(host, oracle):
    """GenerateAABBForObject (SceneIO.h:75-104): sphere = centre +- r; plane = zero-thickness
    box shifted by normal*0.01."""
    rng = np.random.default_rng(7)
    n = 64
    objs = L.default_objects(n)
    objs["type"] = rng.integers(0, 2, n)
    objs["position"] = rng.uniform(-10, 10, (n, 3))
    objs["radius"] = rng.uniform(0.1, 3, n)
    normals = np.array([(0, 1, 0), (0, -1, 0), (1, 0, 0), (0, 0, 1), (0.3, 0.2, 0.9), (0, 0.95, 0.1)], dtype=np.float32)
    objs["normal"] = normals[rng.integers(0, len(normals), n)]
    objs["size"] = rng.uniform(1, 40, (n, 2))
    a = objs.copy()
    b = objs.copy()
    host.generate_aabb(a)
    oracle.generate_aabb(b)
    for fld in a.dtype.names:   # (padding bytes are not compared: numpy does not copy them)
        assert a[fld].tobytes() == b[fld].tobytes(), fld
    sph = a[a["type"] == 0]
    np.testing.assert_array_equal(sph["bounds_min"], (sph["position"] - sph["radius"][:, None]).astype(np.float32))
    np.testing.assert_array_equal(sph["bounds_max"], (sph["position"] + sph["radius"][:, None]).astype(np.float32))
    ground = L.default_objects(1)
    ground["type"] = L.PLANE
    ground["position"] = (0, -1, -4)
    ground["size"] = (40, 40)
    host.generate_aabb(ground)
    np.testing.assert_allclose(ground["bounds_min"][0], (-20, -0.99, -24), rtol=0, atol=1e-6)
    np.testing.assert_allclose(ground["bounds_max"][0], (20, -0.99, 16), rtol=0, atol=1e-6)


def test_camera_vectors_defaults(host):
    """Camera::UpdateVectors (Camera.h:26-34) at the default yaw -90, pitch 0 looks down -z."""
    f, r, u = host.camera_vectors(-90.0, 0.0)
    np.testing.assert_allclose(f, (0, 0, -1), atol=1e-6)
    np.testing.assert_allclose(r, (1, 0, 0), atol=1e-6)
    np.testing.assert_allclose(u, (0, 1, 0), atol=1e-6)
    f, r, u = host.camera_vectors(-45.0, 30.0)
    for v in (f, r, u):
        assert abs(np.linalg.norm(v) - 1) < 1e-6
    assert abs(np.dot(f, r)) < 1e-6 and abs(np.dot(f, u)) < 1e-6


SCENE_TEXT = """OBJECT SPHERE Ball -2.5 0.5 -5 1 0 0 0 0 0 0 0.9 0.8 0.7 1 0.25 1.5 0.5 0.3
OBJECT PLANE Ground 0 -1 -5 0 0 1 0 10 12 2 0.8 0.8 0.8 0 0.6 1 0 0
garbage line that the reader skips

OBJECT SPHERE Short 1 2 3 0.5 0 0 0 0 0 1 0.1 0.2 0.3 0 0.05 1.5 0.95
LIGHT DIRECTIONAL Sun 0 5 0 0.5 -1 -0.5 1 1 1 3 0 1
LIGHT AREA Panel 0 3.5 0 0 -1 0 1 1 0.9 5 0.5 16
LIGHT POINT Bulb 0 2.5 -3 0 0 0 1 0.8 0.7 8 1.5 0
"""


def test_scene_parser_follows_sceneio(host):
    """SceneIO::Load / ParseObject / ParseLight (SceneIO.h:108-122,145-186): token order, type
    strings, defaults for the fields the format does not carry, a short line leaves the
    missing trailing field at its default (istream sentry failure at EOF), AABBs generated."""
    objs, lts = host.parse_scene(SCENE_TEXT)
    assert len(objs) == 3 and len(lts) == 3
    assert list(objs["type"]) == [0, 1, 0]
    np.testing.assert_allclose(objs[0]["position"], (-2.5, 0.5, -5))
    assert objs[0]["radius"] == 1 and objs[0]["mat_type"] == 0
    np.testing.assert_allclose(objs[0]["albedo"], (0.9, 0.8, 0.7))
    assert objs[0]["metallic"] == 1 and objs[0]["roughness"] == 0.25 and objs[0]["ior"] == 1.5
    assert objs[0]["transparency"] == 0.5 and np.isclose(objs[0]["specular"], 0.3)
    # fields not in the file keep Material.h's initialisers; diffuseStrength is defined as 0 here
    assert objs[0]["subsurfaceScatter"] == 0 and np.isclose(objs[0]["scatterDistance"], 0.1)
    assert objs[0]["diffuseStrength"] == 0
    np.testing.assert_allclose(objs[1]["normal"], (0, 1, 0))
    np.testing.assert_allclose(objs[1]["size"], (10, 12))
    np.testing.assert_allclose(objs[1]["bounds_min"], (-5, -0.99, -11), atol=1e-6)
    # one token short (as performance_test.scene:9 is): the stream is already at EOF, the
    # extraction sentry fails and the field keeps Material.h's initialiser
    assert objs[2]["specular"] == 0.5 and np.isclose(objs[2]["transparency"], 0.95)
    np.testing.assert_allclose(objs[0]["bounds_min"], (-3.5, -0.5, -6))
    assert list(lts["type"]) == [1, 2, 0]
    np.testing.assert_allclose(lts[0]["direction"], (0.5, -1, -0.5))
    assert lts[1]["samples"] == 16 and lts[2]["intensity"] == 8
    # shadow fields keep Light.h:15-18 defaults
    assert list(lts["shadowType"]) == [1, 1, 1] and list(lts["pcfSamples"]) == [4, 4, 4]


def test_scene_writer_round_trip(host):
    """SceneIO::Save format (SceneIO.h:50-73,124-142): parse(write(x)) reproduces every field the
    format carries (6 significant digits, as ostream prints floats); the rest falls back to defaults."""
    objs, lts = host.parse_scene(SCENE_TEXT)
    text = host.write_scene(objs, lts)
    lines = text.strip().splitlines()
    assert len(lines) == 6 and lines[0].startswith("OBJECT SPHERE Object0 -2.5 0.5 -5 1 ")
    assert lines[3].startswith("LIGHT DIRECTIONAL Light0 0 5 0 0.5 -1 -0.5 1 1 1 3 0 1")
    assert all(len(l.split()) == 21 for l in lines[:3]) and all(len(l.split()) == 15 for l in lines[3:])
    o2, l2 = host.parse_scene(text)
    for fld in ("type", "position", "radius", "normal", "size", "mat_type", "albedo", "metallic", "roughness", "ior",
                "transparency", "specular", "bounds_min", "bounds_max"):
        np.testing.assert_allclose(o2[fld], objs[fld], rtol=1e-5, err_msg=fld)
    for fld in ("type", "position", "direction", "color", "intensity", "radius", "samples"):
        np.testing.assert_allclose(l2[fld], lts[fld], rtol=1e-5, err_msg=fld)


def test_scene_parser_on_the_reference_scene_files(host):
    """The three scenes the reference ships (res/Scene, copied verbatim to tests/golden/scenes) parse to the counts
    SURVEY.md lists."""
    root = os.path.join(GOLDEN_DIR, "scenes")
    want = {"default.scene": (4, 3), "SIMPLE.scene": (15, 3), "performance_test.scene": (15, 8)}
    for name, (no, nl) in want.items():
        objs, lts = host.parse_scene(open(os.path.join(root, name)).read())
        assert (len(objs), len(lts)) == (no, nl), name
    objs, _ = host.parse_scene(open(os.path.join(root, "default.scene")).read())
    # older column order: default.scene:1 parses to albedo (0,.95,.9), metallic .924, ior 0
    np.testing.assert_allclose(objs[0]["albedo"], (0, 0.95, 0.9))
    assert np.isclose(objs[0]["metallic"], 0.924) and objs[0]["ior"] == 0


def test_strip_bookkeeping(host):
    from opengl_raytracing_amd.dist import StripPlan
    for h, sr, world in [(1080, 16, 8), (1080, 16, 3), (270, 32, 2), (17, 4, 4), (5, 16, 8)]:
        plan = StripPlan(64, h, sr, world)
        rows = [plan.local_rows(r) for r in range(world)]
        assert sum(rows) == h
        assert rows == [host.strip_local_rows(h, sr, world, r) for r in range(world)]
        seen = []
        for r in range(world):
            seen += [plan.global_row(r, ly) for ly in range(plan.max_local_rows) if plan.global_row(r, ly) < h]
        assert sorted(seen) == list(range(h))
        idx = plan.row_index()
        for y in (0, h // 2, h - 1):
            r, ly = divmod(idx[y], plan.max_local_rows)
            assert plan.global_row(r, ly) == y


def test_mesa_trig_host(host):
    """csrc/rt_mesa_math.h (host instantiation, the one rt_abi.cpp uses for tan(radians(fov)/2) and the bounce
    sample's cos / sin) against the llvmpipe fixture directly: sin, cos, tan and exp BIT FOR BIT.  The device
    instantiation of the same header is pinned by tests/test_device_math.py: against this fixture, and against this host
    instantiation on every exponent, beyond the int32 range of the reduction and across exp's clamp points."""
    g = load_golden("trig")
    x, ref = g["trig_in"], g["trig_out"]
    got = host.mesa_math(x)
    ok = (np.abs(x) < 1.6e9) | ~np.isfinite(x)
    for k, name in enumerate(("sin", "cos", "tan")):
        eq = (got[:, k].view(np.uint32) == ref[:, k].view(np.uint32)) | (np.isnan(got[:, k]) & np.isnan(ref[:, k]))
        assert eq[ok].all(), f"{name}: {int((~eq[ok]).sum())} differ"
    y, refe = g["explog_in"], g["explog_out"][:, 3]
    gote = host.mesa_math(y)[:, 3]
    eq = (gote.view(np.uint32) == refe.view(np.uint32)) | (np.isnan(gote) & np.isnan(refe))
    assert eq.all(), f"exp: {int((~eq).sum())} differ"
    half = (g["fov_in"] * np.float32(0.017453292519943295)) * np.float32(0.5)
    assert (host.mesa_math(half)[:, 2].view(np.uint32) == g["fov_tan"].view(np.uint32)).all()
