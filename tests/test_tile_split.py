"""Tile split (rt_split_plan_kernel, the FIRST == 3 head of rt_render_packet_kernel and render_packet's
split paths in csrc/rt_packet.inc) on the GPU: a replaying frame on the measured order runs the tiles its plan names as P
one-wave jobs that divide the lighting units among themselves, the job that arrives last adds the pieces up in the source's
order, and the frames stay the same bits.

Three contexts render every frame, as in test_replay_start.py: split FORCED (RT_DEBUG_SPLIT_PARTS=P at rt_create: every tile the
scratch layout takes is split into P parts, whatever it costs), split OFF (RT_TILE_SPLIT=0) and reuse off (bit 10), which runs
the kernel the project always had.  All three surfaces are poisoned with 0xFF bytes before every render and compared bitwise
between the contexts and with the CPU oracle.  rt_debug_split_tiles is read after every launch: the first replay of a view has
no measured order and therefore no plan, every later one on the same stream must have run the tiles meant to be split in
exactly the expected number of parts, and the split-off context none -- without that all of this would pass with the feature
idle.  The plan's rule itself is held to a NumPy restatement on planted costs through rt_debug_split_plan."""
import contextlib
import os

import numpy as np
import pytest

from opengl_raytracing_amd import layout as L
from opengl_raytracing_amd import scenes
from test_exponent_range import _bases, _own
from test_first_hit_reuse import NORMAL, RECORD, REPLAY, base_scene, ragged
from test_prefix_replay import hall_of_mirrors
from test_replay_start import STEPS4, RigS, down, one_lane_window, profile_scene, shapes
from test_settled_tiles import REUSE_OFF, first_hits, tiles_of

pytestmark = pytest.mark.gpu

S, E, G256 = 512, 1536, 76             # rt_device.h: RT_SPLIT_MAX_TILES, RT_SPLIT_EXTRA_BLOCKS, RT_SPLIT_G256
F = np.float32


@contextlib.contextmanager
def environment(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: v for k, v in kw.items() if v is not None})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def expected_parts(depth, n_lights, force):
    """P of a tile the forced plan splits: capped at 4, at the units a K = 0 tile can own, and 0 where the layout refuses."""
    own = (depth - 1) * (n_lights + 1) if depth > 1 else 0
    parts = min(force, own, 4)
    return parts if parts >= 2 and depth * (n_lights + 1) <= 32 * parts else 0


class RigT(RigS):
    """RigS whose first context splits (forced into `parts` parts; 0: by the natural rule) and whose middle context has the
    split switched off and everything else on."""

    def __init__(self, host, oracle, sc, parts=2, bits=0):
        super().__init__(host, oracle, sc, bits=bits)
        self.on.close()
        self.mid.close()
        with environment(RT_DEBUG_SPLIT_PARTS=str(parts) if parts else None):
            self.on = host.RayTracer(0)
        with environment(RT_TILE_SPLIT="0"):
            self.mid = host.RayTracer(0)
        self.on.set_variant(1 | bits)
        self.mid.set_variant(1 | bits)
        self.off.set_variant(1 | REUSE_OFF | bits)
        self.on.load(sc)
        self.mid.load(sc)
        self.parts = parts
        self.replay_no = 0
        self.split_frames = 0
        self.expect_split = True           # False: frames that must run whole (alternating streams)

    def check_settled(self, p, mode, settled, what):
        tx, ty = tiles_of(p)
        n = 0 if mode == NORMAL else tx * ty
        on, mid, off = (rt.debug_prefix_tiles() for rt in (self.on, self.mid, self.off))
        assert sum(on) == n and on == mid and off == [0] * 9, f"{what}: prefix tiles {on} / {mid} / {off}"
        self.hist = on if mode != NORMAL else None
        self.replay_no = self.replay_no + 1 if mode == REPLAY else 0
        if mode == REPLAY:
            self.check_split(p, what)
        return on

    def check_split(self, p, what):
        tx, ty = tiles_of(p)
        got, none = self.on.split_tiles(), self.mid.split_tiles()
        assert got.shape == (tx * ty,) and none.shape == (tx * ty,) and not none.any(), f"{what}: the split-off context split {none}"
        want = expected_parts(p.maxRayDepth, len(self.sc.lights), self.parts or 4)
        if self.replay_no < 2 or not self.expect_split:          # no measured order yet: no plan
            assert not got.any(), f"{what}: replay {self.replay_no} ran split: {got}"
        elif self.parts:
            assert set(np.unique(got)) <= {0, want} and int((got == want).sum()) == (min(tx * ty, S) if want else tx * ty), \
                f"{what}: parts {np.bincount(got)} where every tile (at most {S}) was to run in {want}"
            self.split_frames += bool(want)
        else:                                                     # the natural rule: every tile that is not settled is over the target
            settled = self.on.debug_settled_map() != 0
            assert (got[~settled] == want).all() and set(np.unique(got)) <= {0, 2, 3, 4}, f"{what}: parts {got} settled {settled}"
            self.split_frames += bool(want) and not settled.all()


@pytest.fixture
def rig(host, oracle):
    made = []

    def make(sc, **kw):
        made.append(RigT(host, oracle, sc, **kw))
        return made[-1]
    yield make
    for r in made:
        r.close()


# ---- C2 over the shapes, P = 2, 3, 4 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", [2, 3, 4])
def test_c2_forced_parts_over_the_shapes(rig, parts):
    """The mirror floor: K = 0 and K = 1 tiles next to settled ones, lanes that die at different depths, C2's subsurface sphere."""
    sc = base_scene("c2")
    r = rig(sc, parts=parts)
    for name, p, api in shapes(sc, max_ray_depth=4):
        h = r.run(down(p), f"c2 P={parts} {name}", api=api)
        assert h[1] > 0 and h[2] > 0, f"{name}: {h}"
    assert r.split_frames >= 12


def test_c2_one_lane_tile(rig):
    sc = base_scene("c2")
    r = rig(sc, parts=3)
    p, cls = one_lane_window(r, sc, max_ray_depth=4)
    h = r.run(p, "c2 9x9 P=3")
    assert h[cls] > 0 and r.split_frames == 3


@pytest.mark.parametrize("depth", [1, 2, 8])
def test_depths(rig, depth):
    """Depth 1: nothing to split.  Depth 2: one depth's units.  Depth 8 in the hall of mirrors: K >= 3 prologues in every part,
    the roulette, 32 units."""
    sc = hall_of_mirrors() if depth == 8 else base_scene("c2")
    r = rig(sc, parts=4)
    for name, p, api in shapes(sc, max_ray_depth=depth)[:2]:
        h = r.run(p if depth == 8 else down(p), f"depth {depth} {name}", api=api)
        if depth == 8:
            assert sum(h[4:]) > 0, f"{name}: no tile with K >= 3 in {h}"
    assert r.split_frames == (0 if depth == 1 else 6)


def test_one_light_caps_the_parts(rig):
    """nLt = 1 at depth 2: two units, so P = 4 is capped at 2."""
    sc = _own(base_scene("c2"), "c2-one-light", lights=scenes._lights3(L.SHADOW_PCF)[:1])
    r = rig(sc, parts=4)
    assert expected_parts(2, 1, 4) == 2
    r.run(down(sc.params(max_ray_depth=2)), "one light depth 2")
    r.run(down(ragged(sc, max_ray_depth=3)), "one light depth 3 ragged")
    assert r.split_frames == 6


def test_subsurface_everywhere(rig):
    """Every object scatters: the subsurface unit of every depth is live in every tile, owned by another part from depth to depth."""
    sc = _own(base_scene("c2"), "c2-sss")
    sc.objects["subsurfaceScatter"][:] = F(0.6)
    for parts in (2, 3):
        r = rig(sc, parts=parts)
        r.run(down(sc.params(max_ray_depth=4)), f"sss P={parts}")
        assert r.split_frames == 3


@pytest.mark.parametrize("base", ["c2", "c2_pcss", "c3", "c4", "c5_96", "c4_pcss", "c5_96_pcss", "huge300", "huge300_pcss"])
def test_every_replaying_instantiation(rig, base):
    """One scene per profile, PCSS lights included.  c3, PkLightS's scene, has a noise texture: a new frameCount is a normal
    frame there and a repeated one records and replays once, which never meets a plan -- so c2_pcss, C2's objects under PCSS
    lights without a texture, runs PkLightS's split kernel through the four replays like the others."""
    sc = _own(base_scene("c2"), "c2_pcss", lights=scenes._lights3(L.SHADOW_PCSS)) if base == "c2_pcss" else profile_scene(base)
    r = rig(sc, parts=3)
    p = down(ragged(sc))
    h = r.run(p, f"{base} ragged", replays=sc.noise is None)
    assert sum(h[1:]) > 0, f"{base}: {h}"
    if base == "c2_pcss":
        assert sc.noise is None and expected_parts(p.maxRayDepth, len(sc.lights), 3) == 3 and r.split_frames == 3
    elif sc.noise is None:
        assert r.split_frames == (3 if expected_parts(p.maxRayDepth, len(sc.lights), 3) else 0)


def test_skybox_misses_inside_split_tiles(rig, oracle):
    """C2 under a skybox, looking down at the mirror floor: paths that hit an object first and leave the scene later add the
    sky at depth >= 1, inside tiles that all run in three parts.  That such pixels exist is read off the oracle: the frame
    with the skybox switched off differs on pixels whose first hit is an object."""
    sc = _own(base_scene("c2"), "c2-sky", skybox=scenes.procedural_skybox(16), use_skybox=True)
    r = rig(sc, parts=3)
    p = down(sc.params(max_ray_depth=4))
    assert p.useSkybox
    lit, unlit = oracle.render(sc, p)[0], oracle.render(sc, L.copy_params(p, useSkybox=0))[0]
    hit_first = first_hits(r.on, p) >= 0
    later_sky = hit_first & (lit.view(np.uint32) != unlit.view(np.uint32)).any(-1)
    assert later_sky.sum() > 64, f"{int(later_sky.sum())} pixels add the sky behind their first hit"
    r.run(p, "c2 skybox P=3")
    assert r.split_frames == 3


def test_more_tiles_than_slots(rig):
    """256 x 192: 768 tiles want a split, 512 get one; the other extra workgroups end at once."""
    sc = base_scene("c2")
    r = rig(sc, parts=2)
    r.run(down(sc.params(width=256, height=192, max_ray_depth=3)), "256x192")
    assert r.split_frames == 3


def test_natural_rule(rig):
    """No forcing, a still frameCount (the natural rule leaves free-running frames whole): on a window this small the target
    (the costs' sum / the device's wave slots) is below every tile that traces anything, so every tile that is not settled is
    split, into 4."""
    sc = base_scene("c2")
    r = rig(sc, parts=0)
    p = down(sc.params(max_ray_depth=4))
    r.frame(p, NORMAL)
    r.frame(p, RECORD)
    for k in range(4):
        r.frame(p, REPLAY, what=f"still replay {k}")
    assert r.split_frames == 3
    # ... and with frameCount advancing the same context runs whole again
    r.expect_split = False
    for k in range(3):
        p = L.copy_params(p, frameCount=p.frameCount + 1)
        r.frame(p, REPLAY, what=f"free-running replay {k}")


def test_twelve_replays_on_one_stream(rig):
    """The arrival counters are put back by every frame and the plan is kept (and re-made) across the sorts."""
    sc = base_scene("c2")
    r = rig(sc, parts=3)
    p = down(sc.params(max_ray_depth=4))
    r.frame(p, NORMAL)
    r.frame(p, RECORD)
    for k in range(12):
        p = L.copy_params(p, frameCount=p.frameCount + 1 + k % 3)
        r.frame(p, REPLAY, what=f"replay {k}")
    assert r.split_frames == 11


def test_two_streams_run_whole(rig):
    """Replays alternate between two streams: the previous packet launch was always on the other one, so no frame is split."""
    import torch
    sc = base_scene("c2")
    r = rig(sc, parts=2)
    r.expect_split = False
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    p = down(sc.params(width=96, height=64, max_ray_depth=4))
    modes = [NORMAL, RECORD] + [REPLAY] * 4
    r.prepare(p, len(modes))
    fc = p.frameCount
    for k, m in enumerate(modes):
        fc += STEPS4[k - 2] if k >= 2 else 0
        r.frame(L.copy_params(p, frameCount=fc), m, stream=streams[k % 2], defer=True, what=f"stream {k % 2} frame {k}")
    r.check_pending()
    assert not r.on.split_tiles().any()


def test_scene_edit_drops_the_plan(rig):
    sc = base_scene("c2")
    r = rig(sc, parts=2)
    p = down(sc.params(max_ray_depth=4))
    r.run(p, "before the edit")
    flipped = _own(sc, "c2-flipped")
    d = flipped.objects["diffuseStrength"]
    d[:] = np.where(d > 0, F(0.0), F(0.5))
    r.sc = flipped
    r.each(lambda rt: rt.set_scene(flipped.objects, flipped.lights))
    r.hist = None
    r.run(p, "after the edit")          # (its first replay must run whole again: check_split)
    assert r.split_frames == 6


# ---- the plan's rule ---------------------------------------------------------------------------------------------------------------
def plan_reference(order, costs, wave_slots, depth, n_lights, force=0, prev=None):
    target = int(costs.astype(np.uint64).sum()) // max(wave_slots, 1)
    own, units = ((depth - 1) * (n_lights + 1) if depth > 1 else 0), depth * (n_lights + 1)
    cap = min(own, 4)
    parts, slot, extra, n = np.zeros(order.size, np.uint8), np.zeros(order.size, np.uint16), [], 0
    for t in order:
        c, was, P = int(costs[t]), (int(prev[t]) if prev is not None else 0), 0
        if force >= 2:
            P = force
        elif c > target or was >= 2:
            P = 2
            while P < 4 and c * (G256 * P + (256 - G256)) > target * 256 * P:
                P += 1
            P = max(P, was)
        P = min(P, cap)
        if P < 2 or units > 32 * P:
            P = 0
        if P and n < S:
            parts[t], slot[t] = P, n
            extra += [int(t) | (k << 28) for k in range(1, P)]
            n += 1
    return parts, slot, np.array(extra, dtype=np.uint32), (len(extra), n)


def test_plan_rule_against_numpy(host):
    rt = host.RayTracer(0)
    try:
        rng = np.random.default_rng(38)
        heavy = (rng.pareto(1.5, 3000) * 150 + 20).astype(np.uint32)
        cases = [("heavy tail", heavy, 64, 4, 3, 0, None),
                 ("many slots", heavy, 5120, 4, 3, 0, None),
                 ("all zero", np.zeros(700, np.uint32), 64, 4, 3, 0, None),
                 ("ties", np.full(1500, 77, np.uint32), 8, 4, 3, 0, None),
                 ("over the cap", np.full(1500, 77, np.uint32), 100000, 4, 3, 0, None),
                 ("forced", heavy[:600], 64, 4, 3, 3, None),
                 ("forced over the cap", heavy, 64, 4, 3, 2, None),
                 ("sticky", heavy, 64, 4, 3, 0, (rng.integers(0, 5, 3000) * (rng.random(3000) < 0.05)).astype(np.uint8)),
                 ("depth 1", heavy, 64, 1, 3, 4, None),
                 ("one light", heavy, 64, 2, 1, 4, None),
                 ("units over 32 P", heavy, 64, 8, 8, 2, None),
                 ("units within 32 P", heavy, 64, 8, 8, 3, None),
                 ("one tile", np.array([9], np.uint32), 1, 4, 3, 0, None)]
        for name, costs, slots, depth, n_lights, force, prev in cases:
            if prev is not None:
                prev = np.where(prev == 1, 0, prev).astype(np.uint8)
            order = np.argsort(-costs.astype(np.int64), kind="stable").astype(np.uint32)
            parts, slot, extra, counts = rt.split_plan(order, costs, slots, depth, n_lights, force, prev)
            want = plan_reference(order, costs, slots, depth, n_lights, force, prev)
            assert counts == want[3], f"{name}: counts {counts}, expected {want[3]}"
            assert (parts == want[0]).all(), f"{name}: parts differ on {int((parts != want[0]).sum())} tiles"
            assert (slot[parts > 0] == want[1][parts > 0]).all(), f"{name}: slots"
            assert (extra[:counts[0]] == want[2]).all() and (extra[counts[0]:] == 0xFFFFFFFF).all(), f"{name}: extra jobs"
            assert counts[1] <= S and counts[0] <= E
            print(f"{name}: {counts[1]} tiles split, {counts[0]} extra jobs, parts {np.bincount(parts, minlength=5)}")
    finally:
        rt.close()
