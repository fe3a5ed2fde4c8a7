"""First-hit reuse (csrc/rt_firsthit.h, render_packet's FIRST parameter) on the GPU: frames that record or replay their first hit
are the same bits as frames that trace everything, and every launch runs in the mode the policy says.

Two contexts render every frame: one with reuse on (the default), one with the off switch (rt_set_variant's bit 10), which runs
the kernel the project always had.  All three surfaces are poisoned with 0xFF bytes (NaN in fp32 and fp16) before every render,
compared bitwise between the two contexts and with the CPU oracle, and rt_debug_first_hit must have counted the launch in the
expected mode -- without the counter all of this would pass with the feature never engaged.  Frames are 48 x 32 (24 one-wave
tiles) and a ragged 52 x 35 window at a non-zero (x0, y0) with interleaved strips that reaches beyond the image on two sides.
Base scenes: one per instantiation of the packet kernel, as tests/test_exponent_range.py chooses them, plus C2's (PkLight)."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import bits_equal
from opengl_raytracing_amd import layout as L
from opengl_raytracing_amd import scenes
from test_exponent_range import _bases, _gen_aabb, _own

pytestmark = pytest.mark.gpu

W, H = 48, 32
NORMAL, RECORD, REPLAY = 0, 1, 2
NAMES = ["normal", "record", "replay"]
OFF = 0x400


@functools.lru_cache(maxsize=None)
def base_scene(name):
    if name == "c2":
        return _own(scenes.make_scene(2, _gen_aabb), "c2")                       # 18 objects, PCF lights: PkLight
    return _bases()[name]              # c3: PkLightS (noise), c4: PkHeavy1, c5_96: PkHeavy (skybox), huge300: PkHuge


def ragged(sc, **kw):
    """A 52 x 35 window at (13, 9) of a 60 x 80 image in strips of 5 rows, every second strip: it ends in half tiles, and reaches
    beyond the image to the right and at the top."""
    return sc.params(width=60, height=80, window=(13, 9, 52, 35), strips=(5, 2, 1), **kw)


class Rig:
    """The two contexts, the scene they hold, and the oracle's frames of it."""

    def __init__(self, host, oracle, sc):
        import torch
        self.torch, self.host, self.oracle = torch, host, oracle
        self.on, self.off = host.RayTracer(0), host.RayTracer(0)
        self.off.set_variant(1 | OFF)
        self.want = {}
        self.pending = []
        self.pool = []
        self.load(sc)

    def close(self):
        self.on.close()
        self.off.close()

    def each(self, fn):
        fn(self.on)
        fn(self.off)

    def load(self, sc):
        self.sc = sc
        self.each(lambda rt: rt.load(sc))

    def expected(self, p):
        key = (id(self.sc), bytes(p))
        if key not in self.want:
            self.want[key] = (self.sc, self.oracle.render(self.sc, p)[:3])
        return self.want[key][1]

    def surfaces(self, p, image=False):
        t = self.torch
        h, w = (p.height, p.width) if image else (p.regionH, p.regionW)
        bufs = (t.empty((h, w, 4), dtype=t.float32, device="cuda"), t.empty((h, w, 4), dtype=t.float32, device="cuda"),
                t.empty((h, w, 4), dtype=t.float16, device="cuda"))
        for b in bufs:
            b.view(t.uint8).fill_(0xFF)
        return bufs

    def prepare(self, p, n, image=False):
        """n pairs of poisoned surfaces for frames of p.  The poison is written on torch's stream, which the render streams are
        not ordered with: the device is drained on both sides, here and not between the frames that use them."""
        self.torch.cuda.synchronize()
        self.pool = [[self.surfaces(p, image) for _ in range(2)] for _ in range(n)]
        self.torch.cuda.synchronize()

    def launch(self, rt, p, bufs, api, stream):
        ptrs = [ctypes.c_void_p(b.data_ptr()) for b in bufs]
        s = ctypes.c_void_p(stream.cuda_stream) if stream is not None else None
        fn = rt.lib.rt_render_into_image if api == "image" else rt.lib.rt_render_to
        rt._check(fn(rt.ctx, ctypes.byref(p), *ptrs, s), api)

    def frame(self, p, mode, api="to", stream=None, defer=False, what=""):
        """One frame on both contexts; the reuse context must run it as `mode`.  api: "to" = rt_render_to, "image" =
        rt_render_into_image (whole-image surfaces), "own" = rt_render into the context's surfaces (which cannot be poisoned from
        here: the frames before them have filled them with other views).  defer: nothing synchronises here, the comparison waits
        for check_pending()."""
        t = self.torch
        what = f"{what or self.sc.name} {api} {NAMES[mode]}"
        before = self.on.debug_first_hit()
        if api == "own":
            self.each(lambda rt: rt.render(p))
            got = [rt.readback() for rt in (self.on, self.off)]
        else:
            if not self.pool:
                self.prepare(p, 1, api == "image")
            bufs = self.pool.pop()
            for rt, b in zip((self.on, self.off), bufs):
                self.launch(rt, p, b, api, stream)
            got = bufs
        after = self.on.debug_first_hit()
        delta = [a - b for a, b in zip(after, before)]
        assert delta == [int(k == mode) for k in range(3)], f"{what}: ran as {delta} (normal, record, replay)"
        self.pending.append((p, api, got, what))
        if not defer:
            self.check_pending()

    def check_pending(self):
        self.torch.cuda.synchronize()
        self.each(lambda rt: rt.sync())
        for p, api, got, what in self.pending:
            on, off = ([np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x) for x in g] for g in got)
            for k, name in enumerate(("gColor", "gPosition", "gNormal")):
                a, b = on[k].view(np.uint16 if k == 2 else np.uint32), off[k].view(np.uint16 if k == 2 else np.uint32)
                assert (a == b).all(), f"{what}: {name} differs from the reuse-off context on {int((a != b).any(-1).sum())} px"
            if api != "image":                     # (whole-image surfaces keep the poison outside the window)
                want = self.expected(p)
                assert bits_equal(on[0], want[0]), f"{what}: gColor differs from the oracle"
                assert bits_equal(on[1], want[1]), f"{what}: gPosition differs from the oracle"
                nan_n = np.isnan(on[2].astype(np.float32)) & np.isnan(want[2].astype(np.float32))
                assert ((on[2].view(np.uint16) == want[2].view(np.uint16)) | nan_n).all(), f"{what}: gNormal differs from the oracle"
        self.pending = []

    def still(self, p, n=3, **kw):
        """n frames of an unseen view: normal, record, then replays."""
        for k in range(n):
            self.frame(p, [NORMAL, RECORD, REPLAY][min(k, 2)], **kw)


@pytest.fixture
def rig(host, oracle):
    made = []

    def make(sc):
        made.append(Rig(host, oracle, sc))
        return made[-1]
    yield make
    for r in made:
        r.close()


@pytest.mark.parametrize("base", ["c2", "c3", "c4", "c5_96", "huge300"])
def test_record_and_replay_are_the_normal_frame(rig, base):
    """Per kernel instantiation: four identical frames, frameCount advancing (with and without a noise texture), ray depths
    1, 2 and 4, and the ragged window."""
    sc = base_scene(base)
    r = rig(sc)
    p = sc.params()
    r.still(p, 4)
    fc = p.frameCount
    if sc.noise is None:               # depth 0 does not see frameCount: it keeps replaying
        r.frame(L.copy_params(p, frameCount=fc + 1), REPLAY)
        r.frame(L.copy_params(p, frameCount=fc + 2), REPLAY)
    else:                              # the noise texture is sampled at frameCount: no replay across values, repeated values replay
        r.frame(L.copy_params(p, frameCount=fc + 1), NORMAL)
        r.frame(L.copy_params(p, frameCount=fc + 2), NORMAL)
        r.still(L.copy_params(p, frameCount=fc + 3), 4)
    for depth in (1, 2, 4):
        q = L.copy_params(p, maxRayDepth=depth, frameCount=fc + 7)
        r.still(q, 3, what=f"{base} depth {depth}")
    r.still(ragged(sc), 4, what=f"{base} ragged")
    # frameCount advancing on the ragged window as well (replay of an edge tile's half-empty waves)
    q = L.copy_params(ragged(sc), frameCount=fc + 1)
    if sc.noise is None:
        r.frame(q, REPLAY, what=f"{base} ragged")
    else:
        r.still(q, 3, what=f"{base} ragged")


FIELD_CHANGES = [
    ("position", dict(camPos=(0.5, 2.0, 9.0))),
    ("direction", dict(camDir=(0.1, 0.0, -1.0))),
    ("up", dict(camUp=(0.1, 1.0, 0.0))),
    ("right", dict(camRight=(1.0, 0.1, 0.0))),
    ("fov", dict(fovDeg=50.0)),
    ("focal length", dict(focalLength=1.25)),
    ("max distance", dict(maxRayDistance=9.5)),
    ("depth", dict(maxRayDepth=3)),
    ("size", dict(width=W + 2, height=H + 1)),
    ("window", dict(x0=3, y0=2, regionW=W - 5, regionH=H - 3)),
    ("strips", dict(stripRows=4, stripCount=2, stripIndex=1)),
    ("useSkybox", dict(useSkybox=1)),
    ("noise scale", dict(noiseScale=(1.0 / 512.0, 1.0 / 1024.0))),
]


def test_every_params_field_is_in_the_key(rig):
    """Each rt_params field changed alone against a replaying view: the next frame must not replay and must be right; standing
    still there records and replays again."""
    sc = base_scene("c2")
    r = rig(sc)
    p = sc.params()
    r.still(p, 3)
    for name, change in FIELD_CHANGES:
        q = L.copy_params(p, **change)
        r.still(q, 3, what=f"changed {name}")
        r.frame(p, NORMAL, what=f"back from {name}")          # one buffer: the first view has to be recorded again
        r.frame(p, RECORD, what=f"back from {name}")
        r.frame(p, REPLAY, what=f"back from {name}")


def test_setters_invalidate(rig):
    """rt_set_scene with changed bytes, rt_set_noise, rt_set_skybox and the exhaustive kernel and back all end the replays;
    identical scene bytes do not."""
    sc = base_scene("c2")
    r = rig(sc)
    p = sc.params()
    r.still(p, 3)
    r.each(lambda rt: rt.set_scene(sc.objects, sc.lights))                  # identical bytes
    r.frame(p, REPLAY, what="identical bytes")
    moved = _own(sc, "c2-moved")
    moved.objects["position"][0] += np.float32(0.25)
    _gen_aabb(moved.objects)
    r.sc = moved
    r.each(lambda rt: rt.set_scene(moved.objects, moved.lights))
    r.still(p, 3, what="changed bytes")
    noisy = _own(moved, "c2-noise", noise=scenes.hash_noise())
    r.sc = noisy
    r.each(lambda rt: rt.set_noise(noisy.noise))
    r.still(p, 3, what="noise set")
    r.frame(L.copy_params(p, frameCount=p.frameCount + 1), NORMAL, what="noise set")
    r.sc = moved
    r.each(lambda rt: rt.set_noise(None))
    r.still(p, 3, what="noise removed")
    sky = _own(moved, "c2-sky", skybox=scenes.procedural_skybox(64), use_skybox=True)
    ps = L.copy_params(p, useSkybox=1)
    r.still(ps, 3, what="before the skybox")                                # (useSkybox without a texture: nothing to sample)
    r.sc = sky
    r.each(lambda rt: rt.set_skybox(sky.skybox))
    r.still(ps, 3, what="skybox set")
    # the exhaustive kernel never records, replays or counts; coming back starts over
    r.on.set_variant(0)
    r.off.set_variant(0 | OFF)
    before = r.on.debug_first_hit()
    r.each(lambda rt: rt.render(ps))
    assert r.on.debug_first_hit() == before
    r.on.set_variant(1)
    r.off.set_variant(1 | OFF)
    r.still(ps, 3, what="variant 0 and back")
    # the off switch and back
    r.on.set_variant(1 | OFF)
    before = r.on.debug_first_hit()
    r.each(lambda rt: rt.render(ps))
    r.each(lambda rt: rt.render(ps))
    after = r.on.debug_first_hit()
    assert [a - b for a, b in zip(after, before)] == [2, 0, 0]
    r.on.set_variant(1)
    r.still(ps, 3, what="switched on again")


def test_two_streams_share_the_records(rig):
    """Frames alternate between two streams with surfaces of their own and nothing synchronises in between: a stream's first
    replay waits for the recording frame on the other stream, and a later recording frame overwrites the records only behind the
    replays still queued on the other stream."""
    import torch
    sc = base_scene("c2")
    r = rig(sc)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    p = sc.params(width=96, height=64)                                     # (96 one-wave tiles: frames that overlap)
    q = L.copy_params(p, camPos=(0.5, 2.0, 9.0))
    modes = [NORMAL, RECORD] + [REPLAY] * 6
    r.prepare(p, 3 * len(modes) + 5)
    for view in (p, q, p):
        for k, m in enumerate(modes):
            r.frame(view, m, stream=streams[k % 2], defer=True, what=f"stream {k % 2} frame {k}")
    r.check_pending()
    # the recording frame on the stream that did not record before
    for k, m in enumerate([NORMAL, RECORD, REPLAY, REPLAY, REPLAY]):
        r.frame(q, m, stream=streams[(k + 1) % 2], defer=True, what=f"stream {(k + 1) % 2} frame {k}")
    r.check_pending()


def test_the_three_render_calls_share_one_cache(rig):
    sc = base_scene("c2")
    r = rig(sc)
    p = sc.params()
    r.frame(p, NORMAL, api="own")
    r.frame(p, RECORD, api="to")
    r.frame(p, REPLAY, api="image")
    r.frame(p, REPLAY, api="own")
    r.frame(p, REPLAY, api="to")
    q = ragged(sc)
    r.frame(q, NORMAL, api="image")
    r.frame(q, RECORD, api="own")
    r.frame(q, REPLAY, api="image")
    r.frame(q, REPLAY, api="to")
