"""The scenes of the instrumented-build tests (test_count_model_host.py on the CPU, test_instrumented.py on the GPU) and the
oracle's answers for them: the three surfaces, the reference ray count `rays` and the traced count T(G) of a skip-exact tracer
that takes pcssShadow's blocker rays G per traversal (oracle/rt_oracle.h, orc_render_traced).

Base scenes: one per instantiation of the packet kernel, as test_exponent_range._bases() picks them, plus C2's.  Each is also
run with one light at a time replaced by an EDGE of the skip rule (EDGES below), and there is one scene built so that its counts
can be written down by hand (hand_scene)."""
import functools

import numpy as np

from opengl_raytracing_amd import layout as L
from opengl_raytracing_amd import scenes
from test_exponent_range import RangeScene, _bases, _gen_aabb, _own

GROUPS = (1, 2, 4, 8, 16)
F = np.float32


@functools.lru_cache(maxsize=None)
def base_scenes():
    """c2: PkLight, c3: PkLightS (noise, PCSS), c4: PkHeavy1, c5_96: PkHeavy (skybox), huge300: PkHuge (no shadow tables),
    c5_96_pcss: PkHeavyS."""
    out = {"c2": _own(scenes.make_scene(2, _gen_aabb), "c2")}
    out.update(_bases())
    return out


# ---- one light replaced by an edge of the skip rule --------------------------------------------------------------------
def _black(l):
    l["color"] = (0.0, 0.0, 0.0)


def _intensity(value):
    def edit(l):
        l["intensity"] = F(value)
    return edit


def _area_away(color):
    """An area light above everything that faces up: max(dot(lightDir, direction), 0) is 0 at every point below it, so its
    attenuation is +0 and its radiance color * 0: +0, or NaN for an infinite colour."""
    def edit(l):
        l["type"] = L.AREA
        l["position"] = (3.0, 30.0, -6.0)
        l["direction"] = (0.0, -1.0, 0.0)       # (the shader's sign: +y lights what is below, scenes._lights3)
        l["color"] = (color, color, color)
        l["intensity"] = 40.0
    return edit


def _no_samples(shadow_type):
    def edit(l):
        l["shadowType"] = shadow_type
        l["pcfSamples"] = 0
    return edit


def _perpendicular(l):
    """A directional light along +x: dot(N, L) of the floor plane (normal +y) is exactly 0."""
    l["type"] = L.DIRECTIONAL
    l["direction"] = (1.0, 0.0, 0.0)
    l["intensity"] = 3.0


def _fan(direction, light_size):
    """A directional PCSS light.  Its 16 blocker rays are lightDir + 2 * rr_i * (lightSize / 10) * (1, 1, 1) with rr_0 = -1 the
    far end of the fan and rr_15 = -13/27 inside it, between rays 6 and 1: spheres that ray 0 finds are common, shading points
    where ray 15 alone finds one are rare.  The second light of EDGES was found by a search over directions and sizes; what it
    has to deliver is asserted of the oracle's numbers (check_edge_is_meaningful)."""
    def edit(l):
        l["type"] = L.DIRECTIONAL
        l["direction"] = direction
        l["color"] = (1.0, 1.0, 1.0)
        l["intensity"] = 3.0
        l["shadowType"] = L.SHADOW_PCSS
        l["pcfSamples"] = 4
        l["lightSize"] = F(light_size)
    return edit


# name -> (edit of the light's record, what the ORACLE's numbers must show for the case to test anything):
#   "dark":  the reference's rays are the base scene's and the traced count is smaller than the base scene's at G = 16, where no
#            blocker search stops early: unlit lanes alone removed rays;
#   "unlit": T(16) < rays;   "first" / "last": some lit blocker search finds its first blocker with ray 0 / with ray 15
EDGES = {
    "black": (_black, "dark"),
    "intensity+0": (_intensity(0.0), "dark"),
    "intensity-0": (_intensity(-0.0), "dark"),
    "nan-radiance": (_area_away(np.inf), "unlit"),
    "area-away": (_area_away(1.0), "unlit"),
    "pcf-no-samples": (_no_samples(L.SHADOW_PCF), ""),
    "pcss-no-samples": (_no_samples(L.SHADOW_PCSS), ""),
    "perpendicular": (_perpendicular, "unlit"),
    "fan-first": (_fan((0.5, -1.0, -0.5), 4.0), "first"),
    "fan-last": (_fan((-0.32, -1.0, -1.0), 4.5), "last"),
}


@functools.lru_cache(maxsize=None)
def edge_scene(base, edge, li):
    sc = _own(base_scenes()[base], f"{base}/{edge}/light{li}")
    EDGES[edge][0](sc.lights[li:li + 1])
    return sc


# ---- a scene whose counts can be written down ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hand_scene():
    """One directional PCSS light (4 PCF samples) straight above a mirror floor, a sphere of radius 50 hanging over both, and a
    camera two units above the floor that looks straight down; depth 2.  Every pixel's path is the same:

      depth 0: the floor.  N.L = 1, the radiance is (3, 3, 3): lit.  Every blocker ray runs into the sphere, so the search
               finds its first blocker with ray 0, and the PCF follows: the reference traces 1 + 16 + 4 rays, a skip-exact
               tracer 1 + G + 4.
      depth 1: the mirrored ray goes up into the sphere's underside, whose normal points down: N.L < 0, unlit.  The reference
               still traces the 16 blocker rays (they start 0.001 below the surface and enter the sphere at once, so every one
               is a blocker) and the 4 PCF rays: 1 + 16 + 4; a skip-exact tracer traces the bounce ray alone.

    rays = 42 per pixel, T(G) = G + 6 per pixel."""
    objs = L.default_objects(2)
    objs[0]["type"] = L.PLANE
    objs[0]["position"] = (0.0, -1.0, 0.0)
    objs[0]["normal"] = (0.0, 1.0, 0.0)
    objs[0]["size"] = (40.0, 40.0)
    objs[0]["albedo"] = (0.8, 0.8, 0.8)
    objs[0]["roughness"] = 0.6
    objs[0]["diffuseStrength"] = 0.0
    objs[1]["type"] = L.SPHERE
    objs[1]["position"] = (0.0, 60.0, 0.0)
    objs[1]["radius"] = 50.0
    objs[1]["albedo"] = (0.7, 0.5, 0.3)
    objs[1]["roughness"] = 0.5
    _gen_aabb(objs)
    lights = L.default_lights(1)
    lights[0]["type"] = L.DIRECTIONAL
    lights[0]["direction"] = (0.0, -1.0, 0.0)
    lights[0]["intensity"] = 3.0
    lights[0]["shadowType"] = L.SHADOW_PCSS
    lights[0]["pcfSamples"] = 4
    cam = dict(cam_pos=(0.0, 1.0, 0.0), cam_dir=(0.0, -1.0, 0.0), cam_up=(0.0, 0.0, -1.0), cam_right=(1.0, 0.0, 0.0), fov_deg=45.0)
    return RangeScene("hand", objs, lights, 48, 32, 2, cam)


HAND_RAYS_PER_PIXEL = 42


def hand_traced_per_pixel(group):
    return group + 6


# ---- the oracle's answers ------------------------------------------------------------------------------------------------
class Answer:
    """The oracle's frame of (scene, params): surfaces, rays, and T(G) on demand."""

    def __init__(self, sc, p):
        from oracle import binding
        self._render = lambda g: binding.render(sc, p, blocker_group=g, blocker_hist=True)
        col, pos, nrm, self.rays, t1, self.first_blocker = self._render(1)
        self.surfaces = (col, pos, nrm)
        self._traced = {1: t1}

    def traced(self, group):
        if group not in self._traced:
            self._traced[group] = self._render(group)[4]
        return self._traced[group]


_ANSWERS = {}


def answer(sc, p):
    """Computed once per (scene, params) and shared: both kernel variants ask for the same frames."""
    key = (sc.name, bytes(p))
    if key not in _ANSWERS:
        _ANSWERS[key] = (sc, Answer(sc, p))
    assert _ANSWERS[key][0] is sc, f"two scenes are called {sc.name}"
    return _ANSWERS[key][1]


def check_edge_is_meaningful(base, edge, li, p_of):
    """What EDGES promises of the ORACLE's numbers for this case (p_of(scene) = the frame's parameters)."""
    kind = EDGES[edge][1]
    sc = edge_scene(base, edge, li)
    a = answer(sc, p_of(sc))
    what = f"{sc.name}: rays {a.rays}, T(1) {a.traced(1)}, T(16) {a.traced(16)}, first blockers {a.first_blocker.tolist()}"
    if kind == "dark":
        b = answer(base_scenes()[base], p_of(base_scenes()[base]))
        assert a.rays == b.rays and a.traced(16) < b.traced(16), f"{what}; base scene: rays {b.rays}, T(16) {b.traced(16)}"
    elif kind == "unlit":
        assert a.traced(16) < a.rays, what
    elif kind == "first":
        assert a.first_blocker[0] > 0 and a.traced(1) < a.traced(4) < a.rays, what
    elif kind == "last":
        assert a.first_blocker[15] > 0, what
