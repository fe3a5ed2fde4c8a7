"""The start of a replaying frame's tile (pk_replay_request / pk_replay_park in csrc/rt_packet.inc and the
FIRST == 2 head of rt_render_packet_kernel) on the GPU: the tile's flag, its lanes' records and the staged bounds are requested
together ahead of the settled test, the record reaches render_packet through the parking area, and the frames stay the same bits.

Three contexts render every frame, as in test_prefix_replay.py: prefix replay on (the default), prefix replay off with settled
tiles on (bit 12), and reuse off (bit 10), which runs the kernel the project always had.  All three surfaces are poisoned with
0xFF bytes before every render and compared bitwise between the contexts and with the CPU oracle -- whole-image surfaces too,
row by row through the strip plan, with the poison intact everywhere else.  rt_debug_first_hit and rt_debug_prefix_tiles are
read after every launch, and every case asserts that its histogram holds tiles of the class it is about.  A case renders a
normal frame, a recording one and four replays with frameCount advancing by 1, 1, 3 and 12: the first replay runs in raster or
predicted order (no measured order yet), the later ones with the feedback scheduler's measured costs at hand (the order
itself has no read-out; the floor case checks that the costs are there).

Shapes: 48 x 32; test_first_hit_reuse.py's ragged 52 x 35 window, whose edge tiles have lanes beyond the window (they must
request nothing); a 9 x 9 window, which has a tile with one live lane; a window at a non-zero (x0, y0) inside a larger image;
and the rows of the second of two ranks in strips of 8 rendered into a whole-image surface (imageStores addressing)."""
import numpy as np
import pytest

from conftest import bits_equal
from opengl_raytracing_amd import layout as L
from opengl_raytracing_amd import scenes
from test_exponent_range import _bases, _own
from test_first_hit_reuse import NORMAL, RECORD, REPLAY, base_scene, ragged
from test_prefix_replay import PREFIX_OFF, RigP, hall_of_mirrors
from test_settled_tiles import REUSE_OFF

pytestmark = pytest.mark.gpu

SCHEDULER_OFF = 0x100
STEPS4 = (1, 1, 3, 12)                 # frameCount advances of the four replays
F = np.float32


class RigS(RigP):
    """RigP whose three contexts share `bits` of rt_set_variant besides their own, and whose whole-image frames are compared with
    the oracle as well."""

    def __init__(self, host, oracle, sc, bits=0):
        super().__init__(host, oracle, sc, on_bits=bits)
        self.mid.set_variant(1 | PREFIX_OFF | bits)
        self.off.set_variant(1 | REUSE_OFF | bits)

    def check_pending(self):
        self.torch.cuda.synchronize()
        self.each(lambda rt: rt.sync())
        for p, api, got, what in self.pending:
            if api == "image":
                self.check_image(p, [np.asarray(x.cpu().numpy()) for x in got[0]], what)
        super().check_pending()

    def check_image(self, p, on, what):
        """The window's pixels of a whole-image surface against the oracle's window, the rest of the surface against the poison."""
        want = self.expected(p)
        rows, cycle = p.stripRows, p.stripRows * p.stripCount
        ly = p.y0 + np.arange(p.regionH)
        gy = (ly // rows) * cycle + p.stripIndex * rows + ly % rows
        gx = p.x0 + np.arange(p.regionW)
        vr, vc = gy < p.height, gx < p.width
        assert vr.any() and vc.any()
        touched = np.zeros((p.height, p.width), dtype=bool)
        touched[np.ix_(gy[vr], gx[vc])] = True
        for k, name in enumerate(("gColor", "gPosition", "gNormal")):
            a, b = on[k][np.ix_(gy[vr], gx[vc])], want[k][np.ix_(vr, vc)]
            if k < 2:
                assert bits_equal(a, b), f"{what}: {name} of the whole-image surface differs from the oracle"
            else:
                nan_n = np.isnan(a.astype(np.float32)) & np.isnan(b.astype(np.float32))
                assert ((a.view(np.uint16) == b.view(np.uint16)) | nan_n).all(), f"{what}: gNormal of the whole-image surface differs from the oracle"
            assert (on[k].view(np.uint8)[~touched] == 0xFF).all(), f"{what}: {name} was written outside the window"

    def run(self, p, what, api="to", replays=True):
        """normal, record, four replays with frameCount advancing -> the histogram.  replays=False: a noise texture is loaded, so
        a new frameCount is a normal frame and a repeated one records and replays."""
        self.frame(p, NORMAL, api=api, what=what)
        self.frame(p, RECORD, api=api, what=what)
        for step in STEPS4:
            p = L.copy_params(p, frameCount=p.frameCount + step)
            self.frame(p, REPLAY if replays else NORMAL, api=api, what=what)
        if not replays:
            self.frame(p, RECORD, api=api, what=what)
            self.frame(p, REPLAY, api=api, what=what)
        print(f"{what}: settled and K = 0 .. 7 tiles {self.hist}")
        assert sum(self.hist) == -(-p.regionW // 8) * -(-p.regionH // 8)
        return self.hist


@pytest.fixture
def rig(host, oracle):
    made = []

    def make(sc, **kw):
        made.append(RigS(host, oracle, sc, **kw))
        return made[-1]
    yield make
    for r in made:
        r.close()


def down(p):
    """The camera pitched down to C2's mirror floor (test_prefix_replay.py's ragged_down)."""
    return L.copy_params(p, camDir=(0.0, -0.3, -0.954), camUp=(0.0, 0.954, -0.3))


def one_lane_window(r, sc, **kw):
    """A 9 x 9 window of the 48 x 32 frame, looking down, whose one-lane tile (its last pixel) is not settled, and that tile's
    index in the histogram: the pixel rendered as a window of its own is one tile, whose class rt_debug_prefix_tiles names."""
    base = down(sc.params(**kw))
    for x0, y0 in ((20, 12), (4, 4), (34, 20), (12, 22), (28, 2), (0, 0)):
        q = L.copy_params(base, x0=x0 + 8, y0=y0 + 8, regionW=1, regionH=1)
        r.each(lambda rt: rt.render(q))
        r.each(lambda rt: rt.render(q))
        h = r.on.debug_prefix_tiles()
        assert sum(h) == 1, h
        if h[0] == 0:
            return L.copy_params(base, x0=x0, y0=y0, regionW=9, regionH=9), h.index(1)
    pytest.fail("every candidate's one-lane tile is settled")


def shapes(sc, **kw):
    """(name, parameters, render call) of the five shapes, the camera as the scene has it."""
    return [("48x32", sc.params(**kw), "to"),
            ("ragged", ragged(sc, **kw), "to"),
            ("offset", sc.params(width=64, height=48, window=(11, 6, 40, 29), **kw), "to"),
            ("strips8", sc.params(width=48, height=32, window=(0, 0, 48, 16), strips=(8, 2, 1), **kw), "image")]


# ---- C2 over the shapes ---------------------------------------------------------------------------------------------------------
def test_c2_diffuse_wall_is_all_k0(rig):
    """Looking straight at the diffuse wall: tiles with K = 0, the class that requests 20 bytes per lane and nothing more.  The
    ragged window sees nothing but the wall: every tile that is not settled has K = 0."""
    sc = base_scene("c2")
    r = rig(sc)
    for name, p, api in shapes(sc, max_ray_depth=4):
        h = r.run(p, f"c2 wall {name}", api=api)
        assert h[1] > 0, f"{name}: no K = 0 tile in {h}"
        if name == "ragged":
            assert sum(h[2:]) == 0, f"{name}: tiles with K >= 1 in {h}"


def test_c2_mirror_floor_has_k1_and_settled_tiles(rig):
    """Pitched down to the mirror floor: tiles with K = 1, whose lanes request all 52 bytes, next to K = 0 tiles.  Settled
    tiles come with the ragged window (its tiles beyond the image) and with test_settled_tiles.py's 40 x 56 window at (152, 0)
    of the 192 x 128 frame, whose tiles are small enough to lie inside a mirror sphere.  Behind the replays the feedback
    scheduler must hold measured costs of the window's tiles: the later replays ran with it on."""
    sc = base_scene("c2")
    r = rig(sc)
    for name, p, api in shapes(sc, max_ray_depth=4):
        p = down(p)
        h = r.run(p, f"c2 floor {name}", api=api)
        assert h[2] > 0 and h[1] > 0, f"{name}: no K = 1 tile next to K = 0 tiles in {h}"
        if name == "ragged":
            assert h[0] > 0, f"{name}: no settled tile in {h}"
        costs = r.on.tile_costs()
        assert costs.shape == (-(-p.regionH // 8), -(-p.regionW // 8)) and costs.any(), f"{name}: no measured tile costs {costs.shape}"
    h = r.run(sc.params(width=192, height=128, window=(152, 0, 40, 56), max_ray_depth=4), "c2 fine window")
    assert h[0] > 0 and h[1] > 0, f"fine window: no settled tile next to K = 0 tiles in {h}"


@pytest.mark.parametrize("depth", [1, 2, 4])
def test_c2_one_lane_tile(rig, depth):
    """The 9 x 9 window: three of its four tiles have lanes beyond the window, the last has one lane inside it.  Depth 1: nothing
    taints, every tile is settled and the start ends at the settled test.  Depth 2: a tile is K = 0 or settled."""
    sc = base_scene("c2")
    r = rig(sc)
    if depth == 1:
        h = r.run(down(sc.params(window=(20, 12, 9, 9), max_ray_depth=1)), "c2 9x9 depth 1")
        assert h == [4] + [0] * 8, h
        return
    p, cls = one_lane_window(r, sc, max_ray_depth=depth)
    h = r.run(p, f"c2 9x9 depth {depth} at ({p.x0}, {p.y0})")
    assert h[cls] > 0 and h[0] < 4, f"the one-lane tile's class {cls} is missing in {h}"
    if depth == 2:
        assert sum(h[2:]) == 0, h


@pytest.mark.parametrize("depth", [1, 2])
def test_c2_shallow_depths(rig, depth):
    sc = base_scene("c2")
    r = rig(sc)
    for name, p, api in shapes(sc, max_ray_depth=depth):
        h = r.run(down(p), f"c2 depth {depth} {name}", api=api)
        if depth == 1:
            assert h[0] == sum(h), f"{name}: {h}"
        else:
            assert h[0] > 0 and h[1] > 0 and sum(h[2:]) == 0, f"{name}: {h}"


# ---- deeper prefixes, every instantiation ---------------------------------------------------------------------------------------
def test_hall_of_mirrors_starts_with_a_roulette(rig):
    """Depth 8, mirrors in front of a diffuse plane: tiles with K >= 3, whose prologue reads the parked record and runs a roulette."""
    sc = hall_of_mirrors()
    r = rig(sc)
    for name, p, api in shapes(sc, max_ray_depth=8):
        h = r.run(p, f"mirrors depth 8 {name}", api=api)
        assert sum(h[3:]) > 0, f"{name}: no tile with K >= 2 in {h}"
        if name in ("48x32", "ragged"):
            assert sum(h[4:]) > 0, f"{name}: no tile with K >= 3 in {h}"


def profile_scene(name):
    """One scene per profile of rt_launch_render; the PCSS variants of C4's and the 302-object scene reach PkHeavy1S and PkHugeS."""
    if name == "c4_pcss":
        return _own(_bases()["c4"], "c4_pcss", lights=scenes._lights3(L.SHADOW_PCSS))
    if name == "huge300_pcss":
        return _own(_bases()["huge300"], "huge300_pcss", lights=scenes._lights3(L.SHADOW_PCSS))
    if name == "c5_96_pcss":
        return _bases()[name]
    return base_scene(name)


@pytest.mark.parametrize("base", ["c2", "c3", "c4", "c5_96", "c4_pcss", "c5_96_pcss", "huge300", "huge300_pcss"])
def test_every_replaying_instantiation(rig, base):
    """PkLight, PkLightS (noise texture), PkHeavy1, PkHeavy (no staged bounds: the staging loop runs zero times), PkHeavy1S,
    PkHeavyS, PkHuge and PkHugeS (above the shadow tables' limits); each must have tiles that resume behind depth 0."""
    sc = profile_scene(base)
    r = rig(sc)
    h = r.run(sc.params(), base, replays=sc.noise is None)
    assert sum(h[2:]) > 0 and sum(h[1:]) > 0, f"{base}: no tile with K >= 1 in {h}"
    # the ragged window, looking down: edge tiles with lanes beyond the window in every instantiation
    h = r.run(down(ragged(sc)), f"{base} ragged", replays=sc.noise is None)
    assert sum(h[2:]) > 0, f"{base} ragged: no tile with K >= 1 in {h}"


# ---- order, streams, the cache --------------------------------------------------------------------------------------------------
def test_scheduler_off(rig):
    """Bit 0x100: every frame in raster order, no measured order ever."""
    sc = base_scene("c2")
    r = rig(sc, bits=SCHEDULER_OFF)
    for name, p, api in shapes(sc, max_ray_depth=4):
        h = r.run(down(p), f"scheduler off {name}", api=api)
        assert h[2] > 0 and h[1] > 0, f"{name}: {h}"


def test_two_streams(rig):
    """Replays alternate between two streams with surfaces of their own and nothing synchronises in between."""
    import torch
    sc = base_scene("c2")
    r = rig(sc)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    p = down(sc.params(width=96, height=64, max_ray_depth=4))               # (96 one-wave tiles: frames that overlap)
    q = L.copy_params(p, camPos=(0.5, 2.0, 9.0))
    modes = [NORMAL, RECORD] + [REPLAY] * 4
    r.prepare(p, 3 * len(modes))
    for view in (p, q, p):
        fc = view.frameCount
        for k, m in enumerate(modes):
            fc += STEPS4[k - 2] if k >= 2 else 0
            r.frame(L.copy_params(view, frameCount=fc), m, stream=streams[k % 2], defer=True, what=f"stream {k % 2} frame {k}")
    r.check_pending()
    h = r.on.debug_prefix_tiles()
    assert sum(h) == 96 and h[2] > 0 and h[1] > 0, h


def test_scene_edit_then_new_recording(rig):
    """A scene edit between two recordings of one view: K and the parked record of the second come from its own flags and
    records, never from the first's.  The edit swaps diffuse and mirror materials, so tiles change class both ways."""
    sc = base_scene("c2")
    r = rig(sc)
    p = down(sc.params(max_ray_depth=4))
    first = list(r.run(p, "c2 before the edit"))
    flipped = _own(sc, "c2-flipped")
    d = flipped.objects["diffuseStrength"]
    d[:] = np.where(d > 0, F(0.0), F(0.5))
    r.sc = flipped
    r.each(lambda rt: rt.set_scene(flipped.objects, flipped.lights))
    r.hist = None
    second = list(r.run(p, "c2 after the edit"))
    assert second != first and sum(second) == sum(first) and sum(second[1:]) > 0, f"{first} -> {second}"
    r.sc = sc
    r.each(lambda rt: rt.set_scene(sc.objects, sc.lights))
    r.hist = None
    assert list(r.run(p, "c2 edited back")) == first
