"""rt_mgpu_* (include/rt_mi355.h, csrc/rt_mgpu.cpp) frame after frame on ONE handle: every frame is rendered into root surfaces
poisoned with 0xFF bytes and compared bitwise with the CPU oracle, the contexts' own counters say what ran on every device slot,
the handle is taken through changes of strip height, frame size, depth and light count, frames are issued back to back with a
consumer on the root stream and no host synchronisation, and a refused render must change nothing.  tests/test_mgpu.py renders
one frame three times and reads it back once: an unwritten tile shows the frame before, and with three frames neither the tile
split nor more than one replay ever runs.

The N "devices" are all device 0 ([0] * N), as in test_mgpu.py: every context, stream, event and the image-addressed stores run,
on one GPU.  What that cannot show is in DESIGN.md section 5.

Poison: hipMemsetAsync of the three root surfaces ON THE ROOT STREAM, before a render -- ordered like any consumer of the frame
before, so the peers' stores of the next frame come behind it only through rt_mgpu_render's own events.  A fresh handle (and a
frame larger than every one before) has no surfaces to poison until a frame has been rendered, so each sequence starts with a
warm-up frame of ANOTHER view (the camera as the scene has it, where the frames under test look down): it allocates, is compared
with the oracle unpoisoned, and leaves the first-hit caches with a key the frames under test do not match.  Counters are read as
differences from behind the warm-up.

Every comparison is bitwise: conftest.bits_equal for gColor and gPosition, uint16 equality modulo NaN for gNormal."""
import ctypes
import functools
import math

import numpy as np
import pytest

from conftest import bits_equal
from opengl_raytracing_amd import layout as L
from opengl_raytracing_amd import scenes
from test_exponent_range import _own
from test_first_hit_reuse import base_scene
from test_replay_start import STEPS4, down, profile_scene
from test_settled_tiles import tiles_of
from test_tile_split import environment, expected_parts

gpu = pytest.mark.gpu                  # (every test but the first, which checks the inputs on the CPU)

NAMES = ("gColor", "gPosition", "gNormal")
BYTES = (16, 16, 8)                    # per pixel of the three surfaces
D2D = 3                                # hipMemcpyDeviceToDevice
NO_SURFACES = -5


@functools.lru_cache(maxsize=None)
def hip():
    lib = ctypes.CDLL("libamdhip64.so")
    lib.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    lib.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    return lib


_WANT = {}


def expected(oracle, sc, p):
    """The oracle's three surfaces of (sc, p), rendered once and shared by the tests (the scene is kept alive with them)."""
    key = (id(sc), bytes(p))
    if key not in _WANT:
        _WANT[key] = (sc, oracle.render(sc, p)[:3])
    return _WANT[key][1]


def differences(got, want):
    """-> what differs between two (gColor, gPosition, gNormal), as text; empty when they are the same bits."""
    out = []
    for k, name in enumerate(NAMES):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.shape != b.shape:
            out.append(f"{name}: shape {a.shape}, expected {b.shape}")
        elif k < 2:
            if not bits_equal(a, b):
                bad = ~((a == b) | (np.isnan(a) & np.isnan(b))).all(-1)
                out.append(f"{name}: {int(bad.sum())} px differ, {poisoned(a.view(np.uint32))} px are poison, first at (y, x) {tuple(np.argwhere(bad)[0])}")
        else:
            nan_n = np.isnan(a.astype(np.float32)) & np.isnan(b.astype(np.float32))
            bad = ~((a.view(np.uint16) == b.view(np.uint16)) | nan_n).all(-1)
            if bad.any():
                out.append(f"{name}: {int(bad.sum())} px differ, {poisoned(a.view(np.uint16))} px are poison, first at (y, x) {tuple(np.argwhere(bad)[0])}")
    return out


def poisoned(words):
    """Pixels of an unsigned-integer view [h, w, 4] whose four words are all ones."""
    return int((words == np.iinfo(words.dtype).max).all(-1).sum())


def poison(mg):
    """0xFF over the three root surfaces -- all the pixels they hold, mg.cap_pixels, the largest frame so far -- on the root stream."""
    *surfaces, stream = mg.get_surfaces()
    for ptr, b in zip(surfaces, BYTES):
        assert hip().hipMemsetAsync(ptr, 0xFF, mg.cap_pixels * b, stream) == 0


def render(mg, p):
    mg.render(p)
    mg.cap_pixels = max(getattr(mg, "cap_pixels", 0), p.width * p.height)


def check(mg, oracle, sc, p, what):
    """The frame just issued against the oracle, and its timings: N finite values >= 0, idle slots included."""
    want = expected(oracle, sc, p)
    # no pixel of the oracle's is the poison: wherever the poison shows, it was left there
    assert poisoned(want[0].view(np.uint32)) == 0, f"{what}: the oracle's frame holds a pixel of four 0xFFFFFFFF words"
    bad = differences(mg.readback(), want)
    assert not bad, f"{what}: {'; '.join(bad)}"
    ms = mg.last_ms()
    assert len(ms) == mg.n and all(math.isfinite(m) and m >= 0 for m in ms), f"{what}: last_ms {ms}"


def warm_up(mg, oracle, sc, p, what):
    """Where the surfaces cannot hold p's frame yet: a frame of p's size from another camera, so that they can be poisoned."""
    if p.width * p.height > getattr(mg, "cap_pixels", 0):
        q = L.copy_params(p, camDir=(0.0, 0.0, -1.0), camUp=(0.0, 1.0, 0.0), camPos=(0.25, 2.0, 9.0))
        assert bytes(q) != bytes(p)
        render(mg, q)
        check(mg, oracle, sc, q, f"{what}: warm-up")


def frame(mg, oracle, sc, p, what):
    """poison, render, compare."""
    warm_up(mg, oracle, sc, p, what)
    poison(mg)
    render(mg, p)
    check(mg, oracle, sc, p, what)


def slot_rows(host, mg, p, rows):
    return [host.strip_local_rows(p.height, rows, mg.n, d) for d in range(mg.n)]


def slot_tiles(p, rows):
    """8 x 8 tiles of a slot's window: the frame's width by the slot's local rows."""
    tx, ty = tiles_of(L.copy_params(p, regionH=rows))
    return tx * ty


def first_hits(mg):
    return [mg.context(d).debug_first_hit() for d in range(mg.n)]


def deltas(after, before):
    return [[a - b for a, b in zip(x, y)] for x, y in zip(after, before)]


def c2_one_light():
    return _own(base_scene("c2"), "c2-one-light", lights=scenes._lights3(L.SHADOW_PCF)[:1])


# ---- 1. poisoned frames over the small shapes ----------------------------------------------------------------------------------
SHAPES = [(48, 32, 2, 8),              # baseline
          (61, 37, 3, 3),              # ragged in both axes; strips cut the 8 x 8 tiles
          (48, 10, 8, 8),              # six devices own no row
          (9, 9, 4, 1),                # the smallest shape with more rows than devices
          (64, 48, 5, 24),             # a ragged last strip: two strips for five devices
          (1, 1, 2, 8)]                # one pixel


def test_shapes_on_the_cpu(host, oracle):
    """What the GPU cases rest on, checked without a device: no pixel of the oracle's frames is the poison (every NaN of theirs is
    genuine), and the strip plan gives the idle slots the table claims."""
    sc = base_scene("c2")
    for w, h, n, rows in SHAPES:
        want = expected(oracle, sc, down(sc.params(width=w, height=h, max_ray_depth=4)))
        assert want[0].shape == (h, w, 4) and poisoned(want[0].view(np.uint32)) == 0, f"{w}x{h}"
    idle = {(w, h, n, rows): sum(host.strip_local_rows(h, rows, n, d) == 0 for d in range(n)) for w, h, n, rows in SHAPES}
    assert idle[(48, 10, 8, 8)] == 6 and idle[(64, 48, 5, 24)] == 3 and idle[(1, 1, 2, 8)] == 1 and idle[(61, 37, 3, 3)] == 0


@gpu
@pytest.mark.parametrize("w,h,n,rows", SHAPES, ids=[f"{w}x{h}-N{n}-rows{r}" for w, h, n, r in SHAPES])
def test_poisoned_frames_over_the_small_shapes(host, oracle, w, h, n, rows):
    """Four frames of a still view, every one into poisoned surfaces: a normal, a recording and two replaying frames on every slot
    that owns a row.  A tile left unwritten shows the poison."""
    sc = base_scene("c2")
    p = down(sc.params(width=w, height=h, max_ray_depth=4))
    with host.MultiGpuRayTracer([0] * n, strip_rows=rows) as mg:
        mg.load(sc)
        warm_up(mg, oracle, sc, p, "warm-up")
        before = first_hits(mg)
        for k in range(4):
            frame(mg, oracle, sc, p, f"{w}x{h} N={n} rows={rows} frame {k}")
        ran = deltas(first_hits(mg), before)
        owns = slot_rows(host, mg, p, rows)
        print(f"{w}x{h} N={n} rows={rows}: rows per slot {owns}, (normal, record, replay) per slot {ran}")
        for d in range(n):
            if owns[d]:
                assert sum(ran[d]) == 4 and ran[d][2] >= 1, f"slot {d} ({owns[d]} rows) never replayed: {ran}"
            else:
                assert ran[d] == [0, 0, 0], f"slot {d} owns no row and ran {ran[d]}"


# ---- 2. replay and split on every device, observed -----------------------------------------------------------------------------
@gpu
def test_replay_and_split_on_every_slot(host, oracle):
    """64 x 48 on three slots in strips of 8: every slot's window is 64 x 16, 16 tiles.  One handle whose contexts split every tile
    into three parts, one whose contexts never split; two frames on a still frameCount and four with it advancing.  Every slot of
    both must have run one normal, one recording and four replaying frames; from the second replay on (the first has no measured
    order and so no plan) every tile of every slot of the forced handle ran in expected_parts(4, lights, 3) parts and no tile
    of the other handle ever did.  Without this the poisoned frames would pass with replay and split idle."""
    sc = base_scene("c2")
    p = down(sc.params(width=64, height=48, max_ray_depth=4))
    n, rows = 3, 8
    parts = expected_parts(4, len(sc.lights), 3)
    assert parts == 3
    with environment(RT_DEBUG_SPLIT_PARTS="3"):
        forced = host.MultiGpuRayTracer([0] * n, strip_rows=rows)
    with environment(RT_TILE_SPLIT="0"):
        whole = host.MultiGpuRayTracer([0] * n, strip_rows=rows)
    with forced, whole:
        before = {}
        for mg in (forced, whole):
            mg.load(sc)
            warm_up(mg, oracle, sc, p, "warm-up")
            before[mg] = first_hits(mg)
        owns = slot_rows(host, forced, p, rows)
        assert owns == [16, 16, 16]
        fc, steps = p.frameCount, (0, 0) + STEPS4
        for k, step in enumerate(steps):
            fc += step
            q = L.copy_params(p, frameCount=fc)
            for mg, who in ((forced, "forced"), (whole, "split off")):
                frame(mg, oracle, sc, q, f"{who} frame {k} frameCount {fc}")
                got = [mg.context(d).split_tiles() for d in range(n)]
                if k < 2:
                    continue                    # (before the first replaying launch the read-out is the warm-up's: empty)
                for d in range(n):
                    assert got[d].shape == (slot_tiles(p, owns[d]),), f"{who} frame {k} slot {d}: {got[d].shape}"
                    want = parts if mg is forced and k >= 3 else 0
                    assert (got[d] == want).all(), f"{who} frame {k} slot {d}: parts per tile {got[d]}, expected {want} on every tile"
        for mg, who in ((forced, "forced"), (whole, "split off")):
            ran = deltas(first_hits(mg), before[mg])
            print(f"{who}: (normal, record, replay) per slot {ran}")
            assert ran == [[1, 1, 4]] * n, f"{who}: (normal, record, replay) per slot {ran}"


@gpu
def test_natural_rule_splits_on_some_slot(host, oracle, monkeypatch):
    """Neither variable set, six frames on a still frameCount (the natural rule leaves free-running frames whole), 48 x 32 on two
    slots: a slot's window has 12 tiles, so the target -- the costs' sum over the device's wave slots -- lies below every tile that
    traces anything, and every tile that is not settled is split (tests/test_tile_split.py's test_natural_rule)."""
    sc = base_scene("c2")
    p = down(sc.params(width=48, height=32, max_ray_depth=4))
    monkeypatch.delenv("RT_DEBUG_SPLIT_PARTS", raising=False)
    monkeypatch.delenv("RT_TILE_SPLIT", raising=False)
    mg = host.MultiGpuRayTracer([0] * 2, strip_rows=8)
    with mg:
        mg.load(sc)
        warm_up(mg, oracle, sc, p, "warm-up")
        before = first_hits(mg)
        split = []
        for k in range(6):
            frame(mg, oracle, sc, p, f"natural rule frame {k}")
            split.append([int((mg.context(d).split_tiles() >= 2).sum()) if k >= 2 else 0 for d in range(mg.n)])
        ran = deltas(first_hits(mg), before)
        print(f"natural rule: split tiles per frame and slot {split}, (normal, record, replay) per slot {ran}")
        assert ran == [[1, 1, 4]] * 2, f"(normal, record, replay) per slot {ran}"
        assert any(any(s) for s in split), f"no frame ran split on any slot: {split}"


@gpu
def test_noise_scene_replays_only_a_repeated_frame_count(host, oracle):
    """c3 (PkLightS) samples its noise texture at frameCount: a new value is a normal frame on every slot, a repeated one records
    and then replays.  48 x 32 -- the smallest of the replay tests' shapes -- on three slots, which own 16, 8 and 8 rows."""
    sc = profile_scene("c3")
    assert sc.noise is not None
    p = down(sc.params())
    n, rows = 3, 8
    with host.MultiGpuRayTracer([0] * n, strip_rows=rows) as mg:
        mg.load(sc)
        warm_up(mg, oracle, sc, p, "warm-up")
        assert slot_rows(host, mg, p, rows) == [16, 8, 8]
        fc = p.frameCount
        plan = [(fc, 0), (fc, 1), (fc, 2), (fc + 1, 0), (fc + 2, 0), (fc + 2, 1), (fc + 2, 2), (fc + 2, 2)]
        for k, (count, mode) in enumerate(plan):
            before = first_hits(mg)
            frame(mg, oracle, sc, L.copy_params(p, frameCount=count), f"c3 frame {k} frameCount {count}")
            ran = deltas(first_hits(mg), before)
            assert ran == [[int(m == mode) for m in range(3)]] * n, f"c3 frame {k} frameCount {count}: (normal, record, replay) per slot {ran}, expected mode {mode}"


# ---- 3. transitions on one live handle -----------------------------------------------------------------------------------------
@gpu
def test_transitions_on_one_handle(host, oracle):
    """One handle of four slots, every tile forced into two parts, taken through: strips of 8, 16, 1 and 8 rows; frames of 48 x 32,
    96 x 64 (the root surfaces are freed and allocated anew), 40 x 24 (inside the same buffers) and 48 x 32 again; depth 4, 2, 4, 3;
    one light instead of three, and back -- section 38's stride changes (5440 -> 2880 -> 5440 -> 4160 -> 2624 -> 4160 dwords a
    slot), once per device context.  Every step differs from the one before in what keys the first-hit cache, so each is a
    normal, a recording and two replaying frames (frameCount still, still, + 1, + 1) on every slot that owns a row, and the second
    replay, the first that has a measured order, must have run every tile of the slot's window in two parts."""
    three, one = base_scene("c2"), c2_one_light()
    steps = [(48, 32, 8, 4, three), (48, 32, 16, 4, three), (48, 32, 1, 4, three), (48, 32, 8, 4, three),
             (96, 64, 8, 4, three), (40, 24, 8, 4, three), (48, 32, 8, 4, three),
             (48, 32, 8, 2, three), (48, 32, 8, 4, three), (48, 32, 8, 3, three),
             (48, 32, 8, 3, one), (48, 32, 8, 3, three)]
    assert all(a != b for a, b in zip(steps, steps[1:]))
    n = 4
    report = []
    with environment(RT_DEBUG_SPLIT_PARTS="2"):
        mg = host.MultiGpuRayTracer([0] * n, strip_rows=8)
    with mg:
        for k, (w, h, rows, depth, sc) in enumerate(steps):
            what = f"step {k}: {w}x{h}, strips of {rows}, depth {depth}, {len(sc.lights)} lights"
            mg.set_strip_rows(rows)
            if k == 0 or sc is not steps[k - 1][4]:
                mg.load(sc)
            p = down(sc.params(width=w, height=h, max_ray_depth=depth))
            warm_up(mg, oracle, sc, p, what)
            parts = expected_parts(depth, len(sc.lights), 2)
            assert parts == 2
            owns = slot_rows(host, mg, p, rows)
            before = first_hits(mg)
            for j, step in enumerate((0, 0, 1, 1)):
                p = L.copy_params(p, frameCount=p.frameCount + step)
                frame(mg, oracle, sc, p, f"{what}, frame {j}")
            ran = deltas(first_hits(mg), before)
            split = [mg.context(d).split_tiles() if owns[d] else None for d in range(n)]
            report.append(f"{what}: rows per slot {owns}, (normal, record, replay) {ran}, tiles in two parts "
                          f"{[None if s is None else int((s == parts).sum()) for s in split]}")
            print(report[-1])
            for d in range(n):
                if not owns[d]:
                    assert ran[d] == [0, 0, 0], report[-1]
                    continue
                assert ran[d] == [1, 1, 2], report[-1]
                assert split[d].shape == (slot_tiles(p, owns[d]),) and (split[d] == parts).all(), f"slot {d} of {report[-1]}: {split[d]}"


# ---- 4. back-to-back frames with a consumer on the root stream -------------------------------------------------------------------
@gpu
def test_back_to_back_frames_with_a_consumer_on_the_root_stream(host, oracle):
    """The loop include/rt_mi355.h documents: per frame a scene upload, the poison, rt_mgpu_render, and -- on the root stream only
    -- a device-to-device copy of the three surfaces into that frame's snapshot; nothing synchronises with the host until one
    rt_mgpu_sync behind the last frame.  Eight frames of C2 at 320 x 200 on four slots, two scenes taken in turn and four camera
    positions, so every frame differs from its neighbours; every snapshot must be its oracle frame.  A peer that overwrites a
    frame its consumer has not read yet (the peers' wait for frameStart), or a root stream that runs ahead of a peer's stores
    (its waits for the done events), shows as another frame's pixels or as poison.

    A missing wait is a RACE: it is not guaranteed to show, and a pass does not prove the waits are there.  What this is worth
    was measured once against two builds of the library, each with one of the two hipStreamWaitEvent calls of rt_mgpu_render
    removed.

    The scenes go up through rt_mgpu_set_scene alone (MultiGpuRayTracer.set_scene), which is asynchronous; load() also sets the
    noise texture and the skybox, and those setters wait for every frame in flight, which would order the frames from the host."""
    import torch
    a = scenes.make_scene(2, host.generate_aabb)
    b = scenes.make_scene(2, host.generate_aabb)
    b.objects["position"][:, 1] += 0.4
    host.generate_aabb(b.objects)
    base = a.params(width=320, height=200)
    views = [L.copy_params(base, camPos=(0.125 * v, 2.0, 9.0 - 0.25 * v)) for v in range(4)]
    frames = [((a, b)[k & 1], views[k % 4]) for k in range(8)]
    want = [expected(oracle, sc, p) for sc, p in frames]
    for k in range(1, len(frames)):
        assert not bits_equal(want[k][0], want[k - 1][0]), f"frames {k - 1} and {k} are the same picture"
    npx = base.width * base.height
    with host.MultiGpuRayTracer([0] * 4, strip_rows=8) as mg:
        mg.load(a)
        warm_up(mg, oracle, a, L.copy_params(base, camPos=(-0.5, 2.0, 9.0)), "warm-up")
        snaps = [[torch.zeros(npx * nb, dtype=torch.uint8, device="cuda") for nb in BYTES] for _ in frames]
        torch.cuda.synchronize()
        *surfaces, root = mg.get_surfaces()
        for k, (sc, p) in enumerate(frames):                   # ---- nothing in here waits for the device
            mg.set_scene(sc.objects, sc.lights)
            poison(mg)
            render(mg, p)
            assert mg.get_surfaces() == (*surfaces, root)
            for src, dst, nb in zip(surfaces, snaps[k], BYTES):
                assert hip().hipMemcpyAsync(dst.data_ptr(), src, npx * nb, D2D, root) == 0
        mg.sync()
        bad = []
        for k, (sc, p) in enumerate(frames):
            col, pos, nrm = (s.cpu().numpy() for s in snaps[k])
            got = (col.view(np.float32).reshape(p.height, p.width, 4), pos.view(np.float32).reshape(p.height, p.width, 4),
                   nrm.view(np.float16).reshape(p.height, p.width, 4))
            bad += [f"snapshot {k}: {d}" for d in differences(got, want[k])]
        assert not bad, "; ".join(bad)


# ---- 5. refusals change nothing ----------------------------------------------------------------------------------------------------
GUARD = 0xA5


def guarded_readback(mg, pixels, room):
    """rt_mgpu_readback into host arrays with room for `room` pixels, filled with GUARD bytes: -> the three surfaces' first
    `pixels` pixels as [pixels, 4] arrays, and how many bytes behind them were written.  (A handle that has taken a refused
    frame's size for its own copies that many pixels; MultiGpuRayTracer.readback sizes its arrays by the last good render.)"""
    assert room >= pixels
    raw = [np.full(room * b, GUARD, dtype=np.uint8) for b in BYTES]
    mg._call("rt_mgpu_readback", *[r.ctypes.data_as(ctypes.c_void_p) for r in raw])
    beyond = sum(int((r[pixels * b:] != GUARD).sum()) for r, b in zip(raw, BYTES))
    return [r[:pixels * b].view(t).reshape(pixels, 4) for r, b, t in zip(raw, BYTES, (np.float32, np.float32, np.float16))], beyond
@gpu
def test_a_refused_render_changes_nothing(host, oracle):
    """A render the handle or its contexts refuse leaves the frame before, its surfaces and its timings as they were."""
    sc = base_scene("c2")
    p = down(sc.params(width=48, height=32, max_ray_depth=4))
    big = down(sc.params(width=96, height=64, max_ray_depth=4))
    n = 4
    with host.MultiGpuRayTracer([0] * n, strip_rows=8) as mg:
        mg.load(sc)
        frame(mg, oracle, sc, p, "the good frame")
        good = mg.readback()
        assert not differences(good, expected(oracle, sc, p))
        surfaces = mg.get_surfaces()
        refused = [("maxRayDepth 33 at 96x64 (passes the handle's check, is larger, a context refuses it)", L.copy_params(big, maxRayDepth=33)),
                   ("maxRayDepth -1 at 96x64", L.copy_params(big, maxRayDepth=-1)),
                   ("stripIndex 1", L.copy_params(p, stripIndex=1)),
                   ("regionH halved", L.copy_params(p, regionH=p.regionH // 2))]
        for what, q in refused:
            with pytest.raises(host.RtError):
                mg.render(q)
            got, beyond = guarded_readback(mg, p.width * p.height, big.width * big.height)
            bad = differences([g.reshape(p.height, p.width, 4) for g in got], good)
            assert not bad and beyond == 0, \
                f"after {what}: the 48 x 32 frame is gone: {'; '.join(bad)}; readback wrote {beyond} bytes behind 48 x 32 pixels"
            assert not differences(mg.readback(), good)
            assert mg.get_surfaces() == surfaces, f"after {what}: surfaces {mg.get_surfaces()}, were {surfaces}"
            ms = mg.last_ms()
            assert len(ms) == n and all(math.isfinite(m) and m >= 0 for m in ms), f"after {what}: last_ms {ms}"
        frame(mg, oracle, sc, p, "a good frame after the refusals")
        frame(mg, oracle, sc, big, "the larger frame, now with a valid depth")


@gpu
def test_a_refused_render_on_a_fresh_handle(host, oracle):
    """No scene loaded: the render is refused, and the handle still has no frame to show (RT_ERR_NO_SURFACES)."""
    sc = base_scene("c2")
    p = down(sc.params(width=48, height=32, max_ray_depth=4))
    with host.MultiGpuRayTracer([0] * 2, strip_rows=8) as mg:
        for k in range(2):
            with pytest.raises(host.RtError):
                mg.render(p)
            for call in (mg.readback, mg.get_surfaces, mg.last_ms):
                with pytest.raises(host.RtError) as e:
                    call()
                assert e.value.code == NO_SURFACES, f"{call.__name__} after refused render {k}: {e.value}"
        mg.load(sc)
        for k in range(3):
            frame(mg, oracle, sc, p, f"frame {k} after load")
        assert len(mg.get_surfaces()) == 4


@gpu
def test_context_is_borrowed(host):
    """rt_mgpu_context: the slots' contexts are distinct, out-of-range slots are refused, and closing a view destroys nothing."""
    with host.MultiGpuRayTracer([0] * 3) as mg:
        views = [mg.context(d) for d in range(3)]
        assert len({v.ctx.value for v in views}) == 3
        for slot in (-1, 3):
            with pytest.raises(host.RtError) as e:
                mg.context(slot)
            assert e.value.code == -1
        assert mg.lib.rt_mgpu_context(mg.ctx, 0, None) == -1, "NULL out"
        for v in views:
            v.close()
        assert views[0].ctx is None and mg.context(0).debug_first_hit() == [0, 0, 0]
