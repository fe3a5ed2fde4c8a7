"""Settled tiles (render_packet's FIRST parameter, csrc/rt_firsthit.h's layout) on the GPU: a replaying
frame copies out the tiles whose paths never read the frame's bounce sample, and the frames stay the same bits.

Three contexts render every frame: settled tiles on (the default), settled tiles off but first-hit reuse on (rt_set_variant's
bit 11), and reuse off (bit 10), which runs the kernel the project always had.  All three surfaces are poisoned with 0xFF bytes
before every render, compared bitwise between the contexts and with the CPU oracle; rt_debug_first_hit and
rt_debug_settled_tiles are read after every launch -- without them all of this would pass with the feature never engaged.
Every case renders a normal frame, a recording one and five replays with frameCount advancing by 1, 1, 3, 12 and 23.  Frames
are 48 x 32 (24 one-wave tiles) and test_first_hit_reuse.py's ragged 52 x 35 window (35 tiles, half-empty ones among them)."""
import ctypes

import numpy as np
import pytest

from conftest import bits_equal
from opengl_raytracing_amd import layout as L
from opengl_raytracing_amd import scenes
from test_exponent_range import _gen_aabb, _own
from test_first_hit_reuse import NAMES, NORMAL, RECORD, REPLAY, Rig, base_scene, ragged

pytestmark = pytest.mark.gpu

REUSE_OFF, SETTLED_OFF = 0x400, 0x800
STEPS = (1, 1, 3, 12, 23)              # frameCount advances of the five replays


def tiles_of(p):
    return -(-p.regionW // 8), -(-p.regionH // 8)


def tile_any(mask):
    """[regionH, regionW] bool -> [tilesY, tilesX] bool: some pixel of the 8 x 8 tile is set."""
    h, w = mask.shape
    padded = np.zeros((-(-h // 8) * 8, -(-w // 8) * 8), dtype=bool)
    padded[:h, :w] = mask
    return padded.reshape(padded.shape[0] // 8, 8, padded.shape[1] // 8, 8).any(axis=(1, 3))


class Rig3(Rig):
    """Rig with a third context between the two: first-hit reuse on, settled tiles off."""

    def __init__(self, host, oracle, sc):
        self.mid = host.RayTracer(0)
        self.mid.set_variant(1 | SETTLED_OFF)
        super().__init__(host, oracle, sc)

    def close(self):
        super().close()
        self.mid.close()

    def each(self, fn):
        fn(self.on)
        fn(self.mid)
        fn(self.off)

    def prepare(self, p, n, image=False):
        self.torch.cuda.synchronize()
        self.pool = [[self.surfaces(p, image) for _ in range(3)] for _ in range(n)]
        self.torch.cuda.synchronize()

    def frame(self, p, mode, api="to", stream=None, defer=False, what="", settled=None):
        """One frame on the three contexts; the two that reuse must run it as `mode`.  settled: the flag map [tilesY, tilesX]
        the settled-tiles context must report after it (None: only its shape is checked; never read when `defer`, because the
        debug calls wait for the device)."""
        what = f"{what or self.sc.name} {api} {NAMES[mode]} frameCount {p.frameCount}"
        ctxs = (self.on, self.mid, self.off)
        before = [rt.debug_first_hit() for rt in ctxs]
        if api == "own":
            self.each(lambda rt: rt.render(p))
            got = [rt.readback() for rt in ctxs]
        else:
            if not self.pool:
                self.prepare(p, 1, api == "image")
            got = self.pool.pop()
            for rt, b in zip(ctxs, got):
                self.launch(rt, p, b, api, stream)
        delta = [[a - b for a, b in zip(rt.debug_first_hit(), was)] for rt, was in zip(ctxs, before)]
        want = [int(k == mode) for k in range(3)]
        assert delta == [want, want, [1, 0, 0]], f"{what}: ran as {delta} (normal, record, replay)"
        if not defer:
            self.check_settled(p, mode, settled, what)
        self.pending.append((p, api, got, what))
        if not defer:
            self.check_pending()

    def check_settled(self, p, mode, settled, what):
        tx, ty = tiles_of(p)
        n = 0 if mode == NORMAL else tx * ty                # a normal frame leaves no valid cache
        on, mid, off = (rt.debug_settled_tiles() for rt in (self.on, self.mid, self.off))
        assert on[0] == n and mid == [n, 0] and off == [0, 0], f"{what}: settled tiles {on} / {mid} / {off}"
        flags = self.on.debug_settled_map()
        assert flags.shape == (n,) and int((flags != 0).sum()) == on[1] and set(np.unique(flags)) <= {0, 1}
        assert not self.mid.debug_settled_map().any()
        if n and settled is not None:
            got = flags.reshape(ty, tx) != 0
            assert (got == settled).all(), f"{what}: settled map\n{got.astype(int)}\nexpected\n{settled.astype(int)}"
        return flags.reshape(ty, tx) != 0 if n else None

    def check_pending(self):
        self.torch.cuda.synchronize()
        self.each(lambda rt: rt.sync())
        for p, api, got, what in self.pending:
            on, mid, off = ([np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x) for x in g] for g in got)
            for k, name in enumerate(("gColor", "gPosition", "gNormal")):
                v = np.uint16 if k == 2 else np.uint32
                for other, who in ((mid, "settled-off"), (off, "reuse-off")):
                    a, b = on[k].view(v), other[k].view(v)
                    assert (a == b).all(), f"{what}: {name} differs from the {who} context on {int((a != b).any(-1).sum())} px"
            if api != "image":                     # (whole-image surfaces keep the poison outside the window)
                want = self.expected(p)
                assert bits_equal(on[0], want[0]), f"{what}: gColor differs from the oracle"
                assert bits_equal(on[1], want[1]), f"{what}: gPosition differs from the oracle"
                nan_n = np.isnan(on[2].astype(np.float32)) & np.isnan(want[2].astype(np.float32))
                assert ((on[2].view(np.uint16) == want[2].view(np.uint16)) | nan_n).all(), f"{what}: gNormal differs from the oracle"
        self.pending = []

    def sequence(self, p, settled=None, replays=True, **kw):
        """normal, record, five replays with frameCount advancing; -> the last parameters.  replays=False: a noise texture is
        loaded, so every new frameCount is a normal frame, and a repeated one records and replays."""
        self.frame(p, NORMAL, settled=settled, **kw)
        self.frame(p, RECORD, settled=settled, **kw)
        for step in STEPS:
            p = L.copy_params(p, frameCount=p.frameCount + step)
            self.frame(p, REPLAY if replays else NORMAL, settled=settled, **kw)
        if not replays:
            self.frame(p, RECORD, settled=settled, **kw)
            self.frame(p, REPLAY, settled=settled, **kw)
        return p


@pytest.fixture
def rig(host, oracle):
    made = []

    def make(sc):
        made.append(Rig3(host, oracle, sc))
        return made[-1]
    yield make
    for r in made:
        r.close()


def with_diffuse(sc, name, value):
    out = _own(sc, name)
    out.objects["diffuseStrength"][:] = np.float32(value)
    return out


def views(sc, **kw):
    return [("48x32", sc.params(**kw)), ("ragged", ragged(sc, **kw))]


def first_hits(rt, p):
    """Object id of every window pixel's first hit, -1 for a miss or a pixel outside the image (rt_camera_rays + rt_trace_rays)."""
    import torch
    rays = rt.camera_rays(p)
    hits = rt.trace_rays(rays)
    torch.cuda.synchronize()
    ids = hits.view(torch.int32)[..., 7].cpu().numpy().copy()
    ids[(rays[..., 4:7] == 0).all(-1).cpu().numpy()] = -1
    return ids


# ---- cases with an exact prediction of the flag map ---------------------------------------------------------------------------
def test_no_diffuse_object_settles_every_tile(rig):
    sc = with_diffuse(base_scene("c2"), "c2-mirror", 0.0)
    r = rig(sc)
    for name, p in views(sc, max_ray_depth=4):
        r.sequence(p, settled=np.ones(tiles_of(p)[::-1], dtype=bool), what=f"no diffuse {name}")


def test_depth_one_settles_every_tile(rig):
    sc = base_scene("c2")
    r = rig(sc)
    for name, p in views(sc, max_ray_depth=1):
        r.sequence(p, settled=np.ones(tiles_of(p)[::-1], dtype=bool), what=f"depth 1 {name}")


def test_all_diffuse_settles_the_tiles_that_hit_nothing(rig, oracle):
    c2 = base_scene("c2")
    sc = with_diffuse(_own(c2, "c2-diffuse", objects=c2.objects[c2.objects["type"] != L.PLANE].copy()), "c2-diffuse", 0.5)
    _gen_aabb(sc.objects)                                                    # (spheres only: the tiles between them hit nothing)
    r = rig(sc)
    for name, p in views(sc, max_ray_depth=4):
        normal = oracle.render(sc, L.copy_params(p, maxRayDepth=1))[2]                                    # N is zero exactly where depth 0 hit nothing
        hit = (normal[..., :3].view(np.uint16) & 0x7FFF != 0).any(-1)
        r.sequence(p, settled=~tile_any(hit), what=f"all diffuse {name}")


def test_depth_two_settles_by_the_first_hit_material(rig):
    sc = base_scene("c2")
    assert (sc.objects["diffuseStrength"] == 0).any() and (sc.objects["diffuseStrength"] > 0).any()
    r = rig(sc)
    for name, p in views(sc, max_ray_depth=2):
        ids = first_hits(r.off, p)
        diffuse = np.where(ids >= 0, sc.objects["diffuseStrength"][np.maximum(ids, 0)] > 0, False)
        r.sequence(p, settled=~tile_any(diffuse), what=f"depth 2 {name}")


# ---- cases without one -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fine", [False, True])
def test_c2_settled_tiles_are_invariant_in_the_oracle(rig, oracle, fine):
    """The taint rule is conservative: whatever the device marks settled must be wholly invariant in the oracle.  At 48 x 32 no
    tile of C2 settles at depth 4 (the oracle finds three invariant ones), so the case also runs where tiles are small enough
    to lie inside a mirror sphere: the 40 x 56 window at (152, 0) of the 192 x 128 frame (35 tiles, aligned with the frame's),
    in which some must settle."""
    sc = base_scene("c2")
    r = rig(sc)
    p = sc.params(width=192, height=128, window=(152, 0, 40, 56), max_ray_depth=4) if fine else sc.params(max_ray_depth=4)
    r.frame(p, NORMAL)
    r.frame(p, RECORD)
    got = r.check_settled(p, RECORD, None, "c2")
    base = r.expected(p)
    varies = np.zeros((p.regionH, p.regionW), dtype=bool)
    for step in (1, 2, 3, 5, 17, 40):
        q = L.copy_params(p, frameCount=p.frameCount + step)
        r.frame(q, REPLAY, what=f"c2 fine={fine}")
        other = r.expected(q)
        for a, b in zip(base, other):
            varies |= (a.view(np.uint16 if a.dtype == np.float16 else np.uint32) != b.view(np.uint16 if b.dtype == np.float16 else np.uint32)).any(-1)
    assert not (got & tile_any(varies)).any(), f"settled tiles that vary in the oracle:\n{(got & tile_any(varies)).astype(int)}"
    if fine:
        assert got.any(), "no tile settled where the whole 192 x 128 frame has seven"


@pytest.mark.parametrize("base", ["c2", "c3", "c4", "c5_96", "huge300"])
def test_every_instantiation(rig, base):
    """PkLight, PkLightS (noise texture: a new frameCount does not replay, a repeated one does), PkHeavy1, PkHeavy (skybox: tiles
    whose mirror rays end in the sky are settled), PkHuge."""
    sc = base_scene(base)
    r = rig(sc)
    p = r.sequence(sc.params(), replays=sc.noise is None, what=base)
    if sc.use_skybox:
        assert r.on.debug_settled_tiles()[1] > 0, "no settled tile under the skybox"
    r.sequence(L.copy_params(ragged(sc), frameCount=p.frameCount + 1), replays=sc.noise is None, what=f"{base} ragged")


def test_roulette_runs_inside_settled_tiles(rig):
    sc = with_diffuse(base_scene("c2"), "c2-mirror-8", 0.0)
    r = rig(sc)
    p = sc.params(max_ray_depth=8)
    r.sequence(p, settled=np.ones(tiles_of(p)[::-1], dtype=bool), what="depth 8 mirrors")


def test_invalidation(rig):
    sc = base_scene("c2")
    r = rig(sc)
    p = sc.params(max_ray_depth=2)

    def record(what):
        r.frame(p, NORMAL, what=what)
        r.frame(p, RECORD, what=what)
        r.frame(L.copy_params(p, frameCount=p.frameCount + 1), REPLAY, what=what)
        return r.on.debug_settled_map()
    first = record("c2")
    assert 0 < first.sum() < first.size
    r.each(lambda rt: rt.set_scene(sc.objects, sc.lights))                  # identical bytes keep the cache and its map
    r.frame(p, REPLAY, what="identical bytes")
    assert (r.on.debug_settled_map() == first).all()
    flipped = _own(sc, "c2-flipped")
    d = flipped.objects["diffuseStrength"]
    d[:] = np.where(d > 0, np.float32(0.0), np.float32(0.5))
    r.sc = flipped
    r.each(lambda rt: rt.set_scene(flipped.objects, flipped.lights))
    second = record("flipped diffuseStrength")
    assert (second != first).any()
    noisy = _own(flipped, "c2-noise", noise=scenes.hash_noise())
    r.sc = noisy
    r.each(lambda rt: rt.set_noise(noisy.noise))
    r.frame(p, NORMAL, what="noise set")
    r.frame(p, RECORD, what="noise set")
    r.frame(p, REPLAY, what="noise set")
    r.frame(L.copy_params(p, frameCount=p.frameCount + 1), NORMAL, what="noise set")
    r.sc = flipped
    r.each(lambda rt: rt.set_noise(None))
    assert (record("noise removed") == second).all()
    sky = _own(flipped, "c2-sky", skybox=scenes.procedural_skybox(64), use_skybox=True)
    r.sc = sky
    r.each(lambda rt: rt.set_skybox(sky.skybox))
    record("skybox set")
    # the exhaustive kernel and back
    for rt, bits in ((r.on, 0), (r.mid, SETTLED_OFF), (r.off, REUSE_OFF)):
        rt.set_variant(0 | bits)
    r.each(lambda rt: rt.render(p))
    assert r.on.debug_settled_tiles() == [0, 0]
    for rt, bits in ((r.on, 0), (r.mid, SETTLED_OFF), (r.off, REUSE_OFF)):
        rt.set_variant(1 | bits)
    record("variant 0 and back")
    # the new switch off and back: the cache is dropped both times, and no tile is settled while it is off
    r.on.set_variant(1 | SETTLED_OFF)
    assert r.on.debug_settled_tiles() == [0, 0]
    before = r.on.debug_first_hit()
    r.each(lambda rt: rt.render(p))
    r.each(lambda rt: rt.render(p))
    r.each(lambda rt: rt.render(p))
    assert r.on.debug_settled_tiles() == [24, 0] and [x - y for x, y in zip(r.on.debug_first_hit(), before)] == [1, 1, 1]
    r.on.set_variant(1)
    assert r.on.debug_settled_tiles() == [0, 0]
    r.mid.set_variant(1)                                                    # (the other way round: on and off again, so that all three start over)
    r.mid.set_variant(1 | SETTLED_OFF)
    assert r.mid.debug_settled_tiles() == [0, 0]
    assert record("switched on again").sum() > 0


def test_two_streams(rig):
    """Frames alternate between two streams with surfaces of their own and nothing synchronises in between; a re-record runs
    while the other stream's replays of the earlier records are queued."""
    import torch
    sc = base_scene("c2")
    r = rig(sc)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    p = sc.params(width=96, height=64, max_ray_depth=2)                    # (96 one-wave tiles: frames that overlap; depth 2: tiles settle)
    q = L.copy_params(p, camPos=(0.5, 2.0, 9.0))
    modes = [NORMAL, RECORD] + [REPLAY] * 5
    r.prepare(p, 3 * len(modes))
    for view in (p, q, p):
        fc = view.frameCount
        for k, m in enumerate(modes):
            fc += STEPS[k - 2] if k >= 2 else 0
            r.frame(L.copy_params(view, frameCount=fc), m, stream=streams[k % 2], defer=True, what=f"stream {k % 2} frame {k}")
    r.check_pending()
    tiles, settled = r.on.debug_settled_tiles()
    assert tiles == 96 and 0 < settled < tiles


def test_the_three_render_calls_share_one_cache(rig):
    sc = base_scene("c2")
    r = rig(sc)
    for p in (sc.params(max_ray_depth=2), ragged(sc, max_ray_depth=2)):  # (depth 2: some tiles settle, some do not)
        fc = p.frameCount
        r.frame(p, NORMAL, api="own")
        r.frame(p, RECORD, api="to")
        for k, api in enumerate(("image", "own", "to")):
            r.frame(L.copy_params(p, frameCount=fc + 1 + k), REPLAY, api=api)
        tiles, settled = r.on.debug_settled_tiles()
        assert 0 < settled < tiles
