"""The ray kernels against the oracle across fp32's exponent range.

Every other parity test renders coordinates of 1e-2 .. 1e5 and material / light fields from small sets of ordinary values.
Four kinds of hot-path code are therefore exercised only where nothing can go wrong in them:

* the in-situ IEEE redo branches of the fast reciprocals / square roots (csrc/rt_fastmath.h) at their call sites -- grouped `ok`
  flags, the `live` mask of compute_pbr<true>, the wave-uniform branches -- which ordinary scenes never take with a non-NaN answer;
* the conservative fp32 bounds of the packet culls, the per-lane cull levels and the shadow tables, whose soundness needs products
  that neither overflow nor underflow;
* the dead-ray skips (a light term of +-0 or NaN), which a denormal light term must not trigger -- nothing else renders denormals;
* the query and shade kernels, which share the intersection code but are kernels of their own.

The oracle (oracle/rt_oracle.c) is plain IEEE C, so it answers all of it bit for bit.  One case list (all_cases) feeds both the
CPU test, which holds the ORACLE's frames to conditions that keep a comparison from degenerating into NaN == NaN or black ==
black, and the GPU tests, which compare all three surfaces and the ray count with the oracle exactly as test_gpu_parity.py does.
Frames are 48 x 32: 24 one-wave tiles.

1. uniform scale: every length of a scene times 2^k, k = -70 .. 70, one base scene per kernel profile of rt_launch_render;
2. one material or light field at a time at extreme magnitudes, on every record and on every third record (wavefronts that mix
   lanes which need the IEEE redo with lanes which do not);
3. mixed magnitudes within one scene;
4. rt_camera_rays / rt_trace_rays / rt_shade_rays on a subset of the same scenes;
5. the shadow tables of scaled scenes against brute-force fp64 rays (soundness only);
6. (not a matter of magnitudes, but this file has the table-less base scene) the packet-level light culls and the per-lane shape
   level of scenes WITHOUT shadow tables: huge300 under PCSS lights and with 2 / 3 / 7 / 8 / 16 PCF samples per light.
"""
import dataclasses
import functools

import numpy as np
import pytest

from opengl_raytracing_amd import layout as L
from opengl_raytracing_amd import scenes

W, H = 48, 32
FLT_MAX = float(np.finfo(np.float32).max)
MAX_RAY_DISTANCE = 114514.0                      # the shader's default (layout.make_params)
F = np.float32


@dataclasses.dataclass
class RangeScene(scenes.Scene):
    """A scenes.Scene whose params() are this file's 48 x 32 frame with the scene's own maxRayDistance."""
    max_ray_distance: float = MAX_RAY_DISTANCE

    def params(self, width=None, height=None, **kw):
        p = super().params(width=W if width is None else width, height=H if height is None else height, **kw)
        p.maxRayDistance = self.max_ray_distance
        return p


@dataclasses.dataclass
class Case:
    name: str
    scene: RangeScene
    group: str                       # which GPU test renders it
    finite: bool = False             # conditions on the ORACLE's frame (test_oracle_keeps_the_cases_meaningful) ...
    nonzero_min: float = 0.0         # ... fraction of pixels with colour != 0
    hit_min: float = 0.0             # ... fraction of pixels with gPosition != 0
    denormal_min: float = 0.0        # ... fraction of pixels holding a denormal non-zero colour channel
    all_miss: bool = False           # ... no pixel has a hit
    raw: bool = False                # member of the raw-intensity sweep (one k of it must render denormals without NaN)


def _gen_aabb(objs):
    from oracle import binding
    return binding.generate_aabb(objs)


def _own(sc, name, **over):
    """A private RangeScene copy of a scenes.Scene."""
    kw = dict(name=name, objects=sc.objects.copy(), lights=sc.lights.copy(), width=W, height=H, max_ray_depth=sc.max_ray_depth,
              camera=dict(sc.camera), frame_count=sc.frame_count, noise=sc.noise, skybox=sc.skybox, use_skybox=sc.use_skybox,
              max_ray_distance=getattr(sc, "max_ray_distance", MAX_RAY_DISTANCE))
    kw.update(over)
    return RangeScene(**kw)


def scaled(scene, k, intensity_mode="compensated", max_ray_distance=None):
    """`scene` with every length multiplied by the exact power of two 2^k: object positions, radii and sizes, light positions and
    the camera position; AABBs regenerated; maxRayDistance = min(114514 * 2^k, FLT_MAX) unless given.  intensity_mode
    "compensated" multiplies the lights' intensity by 4^clamp(k, +-30) (what the inverse-square attenuation takes away, as far
    as the intensity stays a normal number); "raw" leaves it alone, so the lighting underflows to denormals and 0 or overflows."""
    assert intensity_mode in ("compensated", "raw")
    s = np.ldexp(F(1.0), k)
    sc = _own(scene, f"{scene.name}*2^{k}{'' if intensity_mode == 'compensated' else '-raw'}")
    for field in ("position", "radius", "size"):
        sc.objects[field] = sc.objects[field] * s
    sc.lights["position"] = sc.lights["position"] * s
    if intensity_mode == "compensated":
        sc.lights["intensity"] = sc.lights["intensity"] * np.ldexp(F(1.0), 2 * max(-30, min(30, k)))
    sc.camera["cam_pos"] = tuple(float(F(c) * s) for c in sc.camera["cam_pos"])
    _gen_aabb(sc.objects)
    sc.max_ray_distance = min(MAX_RAY_DISTANCE * 2.0 ** k, FLT_MAX) if max_ray_distance is None else max_ray_distance
    return sc


# ---- base scenes: one per kernel profile of rt_launch_render ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bases():
    c2 = scenes.make_scene(2, _gen_aabb)
    c5 = scenes.make_scene(5, _gen_aabb)
    o96 = scenes._concat([c5.objects[:96], c5.objects[-2:]])
    huge = scenes._concat([scenes._spheres(scenes.SplitMix64(0x5EED0300), 300), scenes._planes()])
    _gen_aabb(huge)
    # C4's scene is lit by eight area lights only and a third of its spheres are pure metal.  Where squared distances overflow
    # (k >= 63) every light term of such a scene is 0, and at roughness 1e-12 the metal spheres (13 % of the frame) are black:
    # the oracle's frame would miss the floors of test_oracle_keeps_the_cases_meaningful.  So the first ring light is made the
    # directional light of C2 / C3 (no attenuation) and the metal spheres keep half of their diffuse term.
    c4 = _own(scenes.make_scene(4, _gen_aabb), "c4")
    c4.lights[0]["type"] = L.DIRECTIONAL
    c4.lights[0]["direction"] = (0.5, -1.0, -0.5)
    c4.lights[0]["intensity"] = 3.0
    c4.objects["metallic"][c4.objects["metallic"] == 1.0] = 0.5
    return {
        "c3": _own(scenes.make_scene(3, _gen_aabb), "c3"),                          # 18 objects, noise, PCSS: PkLightS
        "c4": c4,                                                                   # 64 objects: PkHeavy1
        "c5_96": _own(c5, "c5_96", objects=o96),                                    # 98 objects, skybox: PkHeavy
        "huge300": _own(c2, "huge300", objects=huge),                               # 302 objects, no shadow tables: PkHuge
        "c5_96_pcss": _own(c5, "c5_96_pcss", objects=o96.copy(), lights=scenes._lights3(L.SHADOW_PCSS)),   # PkHeavyS
    }


K_FULL = (-60, -52, -40, -20, 20, 40, 52, 60, 63, 64, 70)
K_SOME = (-60, -40, 40, 63, 70)
K_QUERY = (-60, -40, 40, 63)
K_TABLES = (-40, 40, 60)


def _scale_cases():
    out = []
    for bname, base in _bases().items():
        group = f"scale-{bname}"
        for k in (K_FULL if bname == "c3" else K_SOME):
            out.append(Case(f"{bname}/k={k}", scaled(base, k), group, finite=True, nonzero_min=0.15, hit_min=0.20))
            if bname == "c3":
                out.append(Case(f"{bname}/k={k}/raw", scaled(base, k, "raw"), group, raw=True))
        if bname == "c3":
            out.append(Case("c3/k=-70", scaled(base, -70), group))                 # beyond the range: squares leave fp32
            # the directional light has no attenuation, so in the rows above every lit pixel keeps a normal colour (denormal
            # channels on 0.3 % of the frame at most, k = 59).  Without it the point and the area light alone remain:
            # denormal channels on 1.0 % (k = 56) to 5.8 % (k = 60) of the frame; from k = 61 on the squared distances overflow
            nosun = _own(base, "c3-nosun", lights=base.lights[[0, 2]].copy())
            for k in (56, 59, 60, 61):
                out.append(Case(f"c3-nosun/k={k}/raw", scaled(nosun, k, "raw"), group, raw=True))
        for k in (20, 40):                                                         # scaled geometry, the shader's own ray limit:
            out.append(Case(f"{bname}/k={k}/maxdist=114514", scaled(base, k, max_ray_distance=MAX_RAY_DISTANCE), group,
                            finite=True, all_miss=True))                           # everything beyond it, the cull's maxDist decides
    return out


# ---- one field at a time -----------------------------------------------------------------------------------------------
ONE_ULP = float(np.ldexp(1.0, -23))
OBJECT_FIELDS = {
    "roughness": (1e-12, 1e-5, 1e-3, 4.0, 1e10),
    "albedo": (1e-39, 1e-25, 1e20),
    "metallic": (1e-30, 2.0, 1e20),
    "ior": (-1.0, 1e-30, 1.0 - ONE_ULP, 1.0 + ONE_ULP, 1e20),
    "diffuseStrength": (1e-30, 1e30),
    "scatterDistance": (1e-42, 1e-30, 1e30),         # with subsurfaceScatter 0.5 on the same records
}
LIGHT_FIELDS = {
    "intensity": (1e-42, 1e-30, 1e30, 3e38),
    "color": (1e-38, 1e30),
    "shadowSoftness": (1e-30, 1e30),
    "lightSize": (1e-30, 1e30),
}
# (field, value) pairs whose oracle frame was measured all finite with >= 95 % of the pixels non-zero (and, where the third
# entry is set, a denormal colour channel on >= 1 % of them): the comparison is of real pictures there
MEASURED = {("roughness", 1e-12): 0, ("roughness", 1e-5): 0, ("albedo", 1e-39): 0.01, ("albedo", 1e-25): 0, ("intensity", 1e-30): 0,
            ("intensity", 1e30): 0, ("color", 1e-38): 0.01, ("scatterDistance", 1e-30): 0}


def with_field(scene, field, value, every):
    """`scene` with `field` = value on every `every`-th object (or light) record."""
    sc = _own(scene, f"{scene.name}/{field}={value:.9g}/{'all' if every == 1 else f'every{every}'}")
    recs = sc.lights if field in LIGHT_FIELDS else sc.objects
    sel = np.arange(len(recs)) % every == 0
    recs[field][sel] = value
    if field == "scatterDistance":
        recs["subsurfaceScatter"][sel] = 0.5
    return sc


def _field_cases():
    out = []
    for bname in ("c3", "c4"):
        base = _bases()[bname]
        for field, values in list(OBJECT_FIELDS.items()) + list(LIGHT_FIELDS.items()):
            for v in values:
                for every in (1, 3):
                    sc = with_field(base, field, v, every)
                    c = Case(sc.name, sc, f"field-{bname}-{field}")
                    # the measured conditions hold for the value on every record; on every third record the rest of the frame
                    # is the ordinary scene, so the frame stays a real picture but the denormal share shrinks with the records
                    if (field, v) in MEASURED:
                        c.finite, c.nonzero_min = True, 0.95
                        if every == 1:
                            c.denormal_min = MEASURED[(field, v)]
                    out.append(c)
    return out


# ---- mixed magnitudes in one scene -----------------------------------------------------------------------------------------
def _mixed_cases():
    c2 = _bases()["huge300"]                      # C2's camera, lights and depth
    c2objs = scenes.make_scene(2, _gen_aabb).objects
    out = []
    # unit spheres on a floor; a sphere of radius 2^40 at 2^41 whose limb crosses the sky of the view; a sphere of radius 2^-20
    # four radii in front of the camera (the ray limit is raised so that the far sphere can be hit at all).  Under C2's point
    # and area lights the oracle's colour is NaN on 6 % of the frame (pixels of the far sphere), so the case that must be finite
    # is lit by two directional lights (PCF and PCSS) and the one under C2's lights carries no condition
    objs = scenes._concat([scenes._spheres(scenes.SplitMix64(0x5EED0301), 14), scenes._planes(two=False), L.default_objects(2)])
    d = np.array([np.sin(np.radians(38.0)), 0.42, -np.cos(np.radians(38.0))])
    d /= np.linalg.norm(d)
    objs[15]["position"] = tuple(np.array(c2.camera["cam_pos"]) + d * 2.0 ** 41)
    objs[15]["radius"] = 2.0 ** 40
    objs[15]["albedo"] = (0.9, 0.6, 0.3)
    objs[15]["diffuseStrength"] = 0.6
    objs[16]["position"] = (0.0, 2.0, 9.0 - 2.0 ** -18)
    objs[16]["radius"] = 2.0 ** -20
    objs[16]["albedo"] = (0.3, 0.9, 0.4)
    _gen_aabb(objs)
    sun = scenes._lights3(L.SHADOW_PCF)[[1, 1]].copy()
    sun[1]["direction"] = (-0.3, -1.0, 0.4)
    sun[1]["shadowType"] = L.SHADOW_PCSS
    out.append(Case("mixed/radii-2^40-and-2^-20", _own(c2, "mixed-radii", objects=objs, lights=sun, max_ray_distance=2.0 ** 50),
                    "mixed-radii", finite=True, nonzero_min=0.15, hit_min=0.20))
    out.append(Case("mixed/radii-2^40-and-2^-20/point-and-area-lights", _own(c2, "mixed-radii-c2-lights", objects=objs, max_ray_distance=2.0 ** 50),
                    "mixed-radii"))
    # C2's scene, one more object 2^60 away and one whose AABB is +-FLT_MAX (the kernel trusts `bounds` as given)
    objs = scenes._concat([c2objs, L.default_objects(2)])
    objs[18]["position"] = (0.6 * 2.0 ** 60, 0.3 * 2.0 ** 60, -0.74 * 2.0 ** 60)
    objs[18]["radius"] = 2.0 ** 57
    objs[19]["position"] = (1.0, 3.5, 2.0)
    objs[19]["radius"] = 0.8
    objs[19]["albedo"] = (0.9, 0.2, 0.2)
    _gen_aabb(objs)
    objs[19]["bounds_min"] = -FLT_MAX
    objs[19]["bounds_max"] = FLT_MAX
    out.append(Case("mixed/far-object-and-FLT_MAX-box", _own(c2, "mixed-far", objects=objs), "mixed-far", finite=True))
    out.append(Case("mixed/far-object-and-FLT_MAX-box/maxdist=FLT_MAX", _own(c2, "mixed-far-inf", objects=objs, max_ray_distance=FLT_MAX),
                    "mixed-far", finite=True))
    # C2's scene through a telescope: from 2^30 away with fovDeg 1e-3 (a pixel is wider than the scene), from 2^20 away (the
    # scene fills the frame; hit points are rounded to 2^-3), and through a fisheye of 179.9 degrees from its own camera
    for dist_log2 in (30, 20):
        cam = dict(c2.camera)
        cam["cam_pos"] = (0.0, 2.0, 2.0 ** dist_log2)
        cam["fov_deg"] = 1e-3
        out.append(Case(f"mixed/fov=1e-3-from-2^{dist_log2}", _own(c2, f"mixed-tele{dist_log2}", objects=c2objs.copy(), camera=cam,
                                                                  max_ray_distance=2.0 ** (dist_log2 + 2)), "mixed-fov", finite=True))
    cam = dict(c2.camera)
    cam["fov_deg"] = 179.9
    out.append(Case("mixed/fov=179.9", _own(c2, "mixed-fisheye", objects=c2objs.copy(), camera=cam), "mixed-fov", finite=True))
    return out


# ---- scenes without shadow tables: the packet-level light culls and the per-lane shape level ----------------------------------
REACH_SAMPLES = (2, 3, 7, 8, 16)                  # below, at and above RT_PK_REACH_MIN_SAMPLES = 3, and across 8
REACH_NAMES = ("huge300_pcss",) + tuple(f"huge300/pcf={n}" for n in REACH_SAMPLES)


def _reach_cases():
    """Scenes with shadow tables (<= 256 objects, <= 64 lights) take their light candidates from the tables, so the packet-level
    light culls and the per-lane shape level of pk_pcf_shadow run in the table-less profiles only: huge300 (302 objects) under
    PCSS lights is PkHugeS's one deterministic case, and huge300 with 2 / 3 / 7 / 8 / 16 PCF samples per light walks PkHuge
    across the shape level's sample threshold."""
    base = _bases()["huge300"]
    floors = dict(finite=True, nonzero_min=0.15, hit_min=0.20)
    out = [Case("huge300_pcss", _own(base, "huge300_pcss", lights=scenes._lights3(L.SHADOW_PCSS)), "reach", **floors)]
    for n in REACH_SAMPLES:
        sc = _own(base, f"huge300-pcf{n}")
        sc.lights["pcfSamples"] = n
        out.append(Case(f"huge300/pcf={n}", sc, "reach", **floors))
    assert tuple(c.name for c in out) == REACH_NAMES
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = _scale_cases() + _field_cases() + _mixed_cases() + _reach_cases()
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def cases_of(group):
    out = [c for c in all_cases() if c.group == group]
    assert out, group
    return out


def case(name):
    return next(c for c in all_cases() if c.name == name)


_REFERENCE = {}


def reference(oracle, c):
    """The oracle's frame of a case, rendered once per session and shared (never modified)."""
    if c.name not in _REFERENCE:
        _REFERENCE[c.name] = oracle.render(c.scene, c.scene.params())
    return _REFERENCE[c.name]


def frame_stats(ref):
    col, pos = ref[0][..., :3], ref[1][..., :3]
    tiny = np.finfo(np.float32).tiny
    with np.errstate(invalid="ignore"):
        return dict(finite=float(np.isfinite(col).all(-1).mean()), nan=float(np.isnan(col).any(-1).mean()),
                    nonzero=float((col != 0).any(-1).mean()), hit=float((pos != 0).any(-1).mean()),
                    denormal=float(((col != 0) & (np.abs(col) < tiny)).any(-1).mean()))


# ---- 0. the oracle keeps the cases meaningful (CPU) ----------------------------------------------------------------------------
def test_oracle_keeps_the_cases_meaningful(oracle):
    """Conditions on the REFERENCE frames only.  Compensated scale rows -60 <= k <= 70: colour finite everywhere, >= 15 % of the
    pixels non-zero, >= 20 % with a hit.  The raw-intensity sweep: one k renders denormal colour channels on >= 1 % of the pixels
    without a NaN.  The measured field values: finite, >= 95 % non-zero, denormals where listed.  Mixed scenes: finite."""
    bad = []
    raw_ok = []
    for c in all_cases():
        st = frame_stats(reference(oracle, c))
        print(f"{c.name:58s} finite {st['finite']:6.1%}  NaN {st['nan']:6.1%}  colour != 0 {st['nonzero']:6.1%}  hit {st['hit']:6.1%}  "
              f"denormal channel {st['denormal']:6.1%}")
        if c.finite and st["finite"] < 1.0:
            bad.append(f"{c.name}: colour finite on {st['finite']:.1%} of the pixels only")
        if st["nonzero"] < c.nonzero_min:
            bad.append(f"{c.name}: colour != 0 on {st['nonzero']:.1%} < {c.nonzero_min:.0%}")
        if st["hit"] < c.hit_min:
            bad.append(f"{c.name}: gPosition != 0 on {st['hit']:.1%} < {c.hit_min:.0%}")
        if st["denormal"] < c.denormal_min:
            bad.append(f"{c.name}: denormal channel on {st['denormal']:.1%} < {c.denormal_min:.0%}")
        if c.all_miss and st["hit"] != 0.0:
            bad.append(f"{c.name}: {st['hit']:.1%} of the pixels hit something inside the ray limit")
        if c.raw and st["denormal"] >= 0.01 and st["nan"] == 0.0:
            raw_ok.append(c.name)
    assert not bad, "\n".join(bad)
    assert raw_ok, "no k of the raw-intensity sweep renders denormal colour on >= 1 % of the pixels without a NaN"
    print("raw-intensity frames with denormal colour and no NaN:", ", ".join(raw_ok))


# ---- 1.-3. the render kernels ------------------------------------------------------------------------------------------------------
def check_cases(tracer, oracle, cases):
    """Every case against the oracle as test_gpu_parity.py compares: three surfaces bit for bit and the ray count; all cases
    are rendered before the first failure is reported."""
    from test_gpu_parity import assert_bit_exact, render_gpu
    failed = []
    for c in cases:
        p = c.scene.params()
        cpu = reference(oracle, c)
        try:
            assert_bit_exact(render_gpu(tracer, c.scene, p), cpu, c.name)
            rays = tracer.count_rays(p)
            assert rays == cpu[3], f"{c.name}: ray count {rays} != {cpu[3]}"
        except AssertionError as e:
            failed.append(str(e).splitlines()[0])
    assert not failed, f"{len(failed)} of {len(cases)} cases differ from the oracle:\n" + "\n".join(failed)


@pytest.mark.gpu
@pytest.mark.parametrize("base", ["c3", "c4", "c5_96", "huge300", "c5_96_pcss"])
def test_uniform_scale_sweep(tracer, oracle, base):
    check_cases(tracer, oracle, cases_of(f"scale-{base}"))


@pytest.mark.gpu
@pytest.mark.parametrize("field", list(OBJECT_FIELDS) + list(LIGHT_FIELDS))
@pytest.mark.parametrize("base", ["c3", "c4"])
def test_material_and_light_magnitudes(tracer, oracle, base, field):
    check_cases(tracer, oracle, cases_of(f"field-{base}-{field}"))


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["mixed-radii", "mixed-far", "mixed-fov"])
def test_mixed_magnitudes_in_one_scene(tracer, oracle, group):
    check_cases(tracer, oracle, cases_of(group))


@pytest.mark.gpu
@pytest.mark.parametrize("name", REACH_NAMES)
def test_light_culls_of_scenes_without_shadow_tables(tracer, oracle, name):
    """One 48 x 32 frame per case of _reach_cases, in both kernel variants: surfaces bit for bit, equal ray counts."""
    check_cases(tracer, oracle, [case(name)])


# ---- 4. the query and shade kernels on the same scenes -----------------------------------------------------------------------------
def _query_cases(which):
    if which == "mixed":
        return [c for c in all_cases() if c.group.startswith("mixed-")]
    return [case(f"{which}/k={k}") for k in K_QUERY]


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["c3", "c4", "mixed"])
def test_query_and_shade_kernels(tracer, oracle, which):
    """rt_camera_rays + rt_trace_rays reproduce gPosition / gNormal, ANY equals closest.object >= 0, and
    rt_shade_rays(p, rt_camera_rays(p), NULL) equals rt_render_to(p) on all three surfaces."""
    import torch
    from test_query import _gbuffer_check
    from test_shade import check_camera_identity
    failed = []
    for c in _query_cases(which):
        p = c.scene.params()
        p1 = c.scene.params(max_ray_depth=1)          # gPosition / gNormal hold the LAST bounce's hit: depth 1 = the primary ray's
        try:
            h = _gbuffer_check(tracer, oracle, c.scene, p1, c.name)
            anyh = tracer.trace_rays(tracer.camera_rays(p1), "any")
            torch.cuda.synchronize()
            assert (anyh.cpu().numpy() == (h["object"] >= 0)).all(), f"{c.name}: any-hit != closest-hit >= 0"
            check_camera_identity(tracer, p, c.name)
        except AssertionError as e:
            failed.append(str(e).splitlines()[0])
    assert not failed, "\n".join(failed)


# ---- 5. shadow tables at scale --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", K_TABLES)
@pytest.mark.parametrize("base", ["c3", "c4"])
def test_shadow_tables_are_sound_at_scale(tracer, base, k):
    """Soundness only: every object a shadow ray hits (brute force, fp64) has its bit in the cell the fp32 lookup reads.  A
    light without a table (kind 0) is sound by definition, and so is a scene for which rt_set_scene builds none (measured:
    at k = 60 no light gets a table).  The selectivity is printed, not gated.  At k = -40 the shader's 0.001 offset of a
    shadow ray's origin is far outside the scene, so no ray hits anything: only the lookup's arithmetic runs there."""
    from test_shadow_tables import _check_scene
    sc = scaled(_bases()[base], k)
    tracer.load(sc)
    tab, nw = tracer.shadow_tables()
    if tab is None:
        print(f"{sc.name}: rt_set_scene built no shadow tables")
        return
    kinds = [int(tab[li * 28]) for li in range(len(sc.lights))]
    st = _check_scene(tracer, sc, np.random.default_rng(100 + k), n_points=300)
    print(f"{sc.name}: table kinds {kinds}; mean candidate bits per lane and light {np.mean(st['cells_mean_bits']):.2f} of "
          f"{len(sc.objects)}; {st['lanes_all']} of {st['lanes']} lanes take every object; {st['hits']} ray hits checked")
