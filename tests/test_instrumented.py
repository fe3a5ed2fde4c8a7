"""The instrumented builds of the render kernel on the GPU: rt_count_rays_to's two modes (rt_packet.inc's COUNT = 1 and
COUNT = 2, rt_render_kernel<1> under variant 0) render the production frame, count what the oracle counts, book their
diagnostics as include/rt_mi355.h says, and leave the first-hit cache alone.

Mode 1 traces every ray of the reference and mode 2 keeps the production skips, so their surfaces being the same bits -- and
the oracle's, and the production launch's -- is the other half of the claim that the skipped rays cannot reach a pixel.  Mode 1's
total must be the oracle's `rays`, mode 2's the oracle's traced count T(G) (tests/test_count_model_host.py) at the blocker group
G the launch reports in rt_debug_stats_ex's out[31]; the exhaustive kernel ignores the mode.  Everything is exact.  All
surfaces are poisoned with 0xFF bytes before every launch.  Frames are 48 x 32, and the ragged 52 x 35 window of
test_first_hit_reuse.  Scenes: tests/count_cases.py."""
import numpy as np
import pytest

import count_cases as C
from conftest import bits_equal
from opengl_raytracing_amd import layout as L
from test_first_hit_reuse import ragged

pytestmark = pytest.mark.gpu

NAMES = ("gColor", "gPosition", "gNormal")
BASES = list(C.base_scenes())


def poisoned(p):
    import torch
    h, w = p.regionH, p.regionW
    bufs = (torch.empty((h, w, 4), dtype=torch.float32, device="cuda"), torch.empty((h, w, 4), dtype=torch.float32, device="cuda"),
            torch.empty((h, w, 4), dtype=torch.float16, device="cuda"))
    for b in bufs:
        b.view(torch.uint8).fill_(0xFF)
    torch.cuda.synchronize()          # (the poison is written on torch's stream, the launches run on the context's)
    return bufs


def host_copy(bufs):
    return [b.cpu().numpy() for b in bufs]


def same_bits(a, b):
    return all((x.view(np.uint16 if k == 2 else np.uint32) == y.view(np.uint16 if k == 2 else np.uint32)).all()
               for k, (x, y) in enumerate(zip(a, b)))


def assert_is_the_oracles(got, want, what):
    assert bits_equal(got[0], want[0]), f"{what}: gColor differs from the oracle"
    assert bits_equal(got[1], want[1]), f"{what}: gPosition differs from the oracle"
    nan_n = np.isnan(got[2].astype(np.float32)) & np.isnan(want[2].astype(np.float32))
    assert ((got[2].view(np.uint16) == want[2].view(np.uint16)) | nan_n).all(), f"{what}: gNormal differs from the oracle"


def instrumented(rt, p, mode):
    """One rt_count_rays_to launch into poisoned surfaces -> (surfaces on the host, total, the 32 counters)."""
    bufs = poisoned(p)
    total = rt.count_rays_to(p, mode, *bufs)
    return host_copy(bufs), total, rt.debug_stats_ex()


def run_case(rt, sc, p, what):
    """The frame of (sc, p) by the production launch and by both instrumented ones, against the oracle."""
    a = C.answer(sc, p)
    rt.load(sc)
    bufs = poisoned(p)
    rt.render_to(p, *bufs)
    rt.sync()
    production = host_copy(bufs)
    assert_is_the_oracles(production, a.surfaces, f"{what}: production")
    got = {}
    for mode in (1, 2):
        surf, total, stats = instrumented(rt, p, mode)
        got[mode] = surf
        assert_is_the_oracles(surf, a.surfaces, f"{what}: mode {mode}")
        assert same_bits(surf, production), f"{what}: mode {mode}'s surfaces are not the production frame's"
        assert stats[0] == total, f"{what}: mode {mode} returned {total}, out[0] is {stats[0]}"
        group = stats[31]
        assert group in C.GROUPS, f"{what}: out[31] = {group}"
        if mode == 1 or rt.variant == 0:
            want = a.rays
        else:
            want = a.traced(group)
        print(f"{what}: mode {mode} G {group}: {total} rays, the oracle {want} (rays {a.rays}, T(1) {a.traced(1)})")
        assert total == want, f"{what}: mode {mode} (G = {group}) counted {total}, the oracle {want}"
    assert same_bits(got[1], got[2]), f"{what}: the two instrumented builds render different frames"


# ---- the cases must be able to tell a wrong count from a right one: asserted of the ORACLE's numbers, before any launch ----
@pytest.fixture(scope="module")
def discriminating(oracle):
    c3, c2 = C.base_scenes()["c3"], C.base_scenes()["c2"]
    a = C.answer(c3, c3.params())
    assert a.traced(1) < a.traced(4) < a.rays, "c3: the blocker group must matter"
    b = C.answer(c2, c2.params())
    assert not (c2.lights["shadowType"] == L.SHADOW_PCSS).any() and b.traced(1) == b.traced(16) < b.rays, "c2: unlit lanes alone must remove rays"
    h = C.hand_scene()
    n = h.width * h.height
    a = C.answer(h, h.params())
    assert a.rays == n * C.HAND_RAYS_PER_PIXEL and all(a.traced(g) == n * C.hand_traced_per_pixel(g) for g in C.GROUPS)


@pytest.mark.parametrize("window", ["frame", "ragged"])
@pytest.mark.parametrize("base", BASES)
def test_base_scenes(tracer, discriminating, base, window):
    sc = C.base_scenes()[base]
    run_case(tracer, sc, sc.params() if window == "frame" else ragged(sc), f"{base} {window}")


def test_hand_built_scene(tracer, discriminating):
    """The counts of count_cases.hand_scene are written down there: 42 rays per pixel, G + 6 traced."""
    sc = C.hand_scene()
    run_case(tracer, sc, sc.params(), "hand")
    rt = tracer
    n = sc.width * sc.height
    assert rt.count_rays_to(sc.params(), 1) == n * 42
    group = rt.debug_stats_ex()[31]
    assert rt.count_rays_to(sc.params(), 2) == (n * 42 if rt.variant == 0 else n * (group + 6))


@pytest.mark.parametrize("edge", list(C.EDGES))
@pytest.mark.parametrize("base", BASES)
def test_edge_lights(tracer, discriminating, base, edge):
    """One light at a time replaced by an edge of the skip rule (count_cases.EDGES)."""
    sc0 = C.base_scenes()[base]
    for li in range(len(sc0.lights)):
        C.check_edge_is_meaningful(base, edge, li, lambda s: s.params())
        sc = C.edge_scene(base, edge, li)
        run_case(tracer, sc, sc.params(), sc.name)


def test_refusals_and_the_scratch_form(tracer, host):
    rt = tracer
    sc = C.base_scenes()["c2"]
    p = sc.params()
    rt.load(sc)
    a = C.answer(sc, p)
    for mode in (0, 3, -1):
        with pytest.raises(host.RtError):
            rt.count_rays_to(p, mode)
    bufs = poisoned(p)
    with pytest.raises(host.RtError):          # all three surfaces or none
        rt.count_rays_to(p, 1, bufs[0], None, bufs[2])
    assert (host_copy(bufs)[0].view(np.uint32) == 0xFFFFFFFF).all(), "a refused call wrote"
    # without surfaces it is rt_count_rays / rt_count_rays_traced
    assert rt.count_rays_to(p, 1) == rt.count_rays(p) == a.rays
    group = rt.debug_stats_ex()[31]
    assert rt.count_rays_to(p, 2) == rt.count_rays_traced(p) == (a.rays if rt.variant == 0 else a.traced(group))


# ---- the diagnostics of rt_debug_stats_ex: what include/rt_mi355.h promises of them -----------------------------------------
STABLE = list(range(12)) + [20, 21]          # sums of integers over waves: the same for every launch of a frame
TIMERS = list(range(12, 20)) + list(range(22, 31))


@pytest.mark.parametrize("base", BASES + ["hand"])
def test_counters(tracer, base):
    rt = tracer
    sc = C.hand_scene() if base == "hand" else C.base_scenes()[base]
    rt.load(sc)
    for p in (sc.params(), ragged(sc)):
        for mode in (1, 2):
            _, total, s = instrumented(rt, p, mode)
            _, total2, s2 = instrumented(rt, p, mode)
            what = f"{base} {p.regionW}x{p.regionH} mode {mode}: {s}"
            assert s[0] == total and total2 == total, what
            assert [s[k] for k in STABLE] == [s2[k] for k in STABLE], f"{what} then {s2}"
            assert s[31] == s2[31] and s[31] in C.GROUPS, what
            assert s[21] <= s[20], what
            assert all(s[k] == 0 for k in TIMERS), f"timer slots in the default build: {what}"
            if rt.variant == 0:
                assert all(s[k] == 0 for k in range(1, 31)) and s[31] == 1, what
                continue
            assert s[1] > 0 and s[2] > 0 and s[3] > 0, what
            boxed = sum(s[4:9])          # packets that formed a direction box: all but the table-driven ones
            assert s[11] <= 64 * boxed <= 64 * s[1], what
            assert boxed <= s[1] and s[9] + s[10] <= s[2], what
            # every pixel's primary ray is one lane of a boxed packet, and every ray counted belongs to a packet of at most 64
            inside = sum(1 for j in range(p.regionH) for i in range(p.regionW) if p.x0 + i < p.width and _image_row(p, j) < p.height)
            assert s[11] >= inside and s[0] <= 64 * s[1], what
            if base == "huge300":          # no shadow tables, no PCSS light: every packet forms a direction box
                assert boxed == s[1] and s[9] + s[10] == s[2] and s[31] == 1, what
        if rt.variant == 1:          # the skips only ever remove packets and lanes
            s1, s2 = instrumented(rt, p, 1)[2], instrumented(rt, p, 2)[2]
            assert all(s2[k] <= s1[k] for k in (0, 1, 11)), f"{base}: mode 1 {s1}, mode 2 {s2}"


def _image_row(p, j):
    ly = p.y0 + j
    cycle = p.stripCycleRows if p.stripCycleRows > 0 else p.stripRows * p.stripCount
    offset = p.stripOffsetRows if p.stripCycleRows > 0 else p.stripIndex * p.stripRows
    return (ly // p.stripRows) * cycle + offset + ly % p.stripRows


# ---- count launches between the frames of a still view ----------------------------------------------------------------------
@pytest.mark.parametrize("base", ["c2", "c3", "c4"])
def test_count_launches_leave_the_first_hit_cache(host, oracle, base):
    import torch
    sc = C.base_scenes()[base]
    p = sc.params()
    a = C.answer(sc, p)
    q = L.copy_params(ragged(sc), frameCount=p.frameCount + 3)
    aq = C.answer(sc, q)
    rt = host.RayTracer(0)
    try:
        rt.variant = 1
        rt.load(sc)

        def frame(mode, stream=None, what=""):
            before = rt.debug_first_hit()
            bufs = poisoned(p)
            if stream is None:
                rt.render_to(p, *bufs)
            else:
                rt.render_to(p, *bufs, stream=stream.cuda_stream)
            after = rt.debug_first_hit()
            assert [x - y for x, y in zip(after, before)] == [int(k == mode) for k in range(3)], f"{base} {what}: ran as {after} - {before}"
            return bufs

        def counts(what):
            """Both modes, on the view's own window and on another window at another frameCount."""
            before, tiles = rt.debug_first_hit(), rt.debug_prefix_tiles()
            for pp, aa in ((p, a), (q, aq)):
                for mode in (1, 2):
                    surf, total, stats = instrumented(rt, pp, mode)
                    assert_is_the_oracles(surf, aa.surfaces, f"{base} {what}: mode {mode}")
                    assert total == (aa.rays if mode == 1 else aa.traced(stats[31])), f"{base} {what}: mode {mode} counted {total}"
            assert rt.debug_first_hit() == before, f"{base} {what}: a count launch was counted as a frame"
            assert rt.debug_prefix_tiles() == tiles, f"{base} {what}: a count launch changed the cached window's tiles"
            return tiles

        frame(0, what="first frame")
        frame(1, what="second frame")
        rt.sync()
        tiles = counts("after the recording frame")
        assert sum(tiles) == ((p.regionW + 7) // 8) * ((p.regionH + 7) // 8), tiles
        bufs = frame(2, what="after the count launches")
        rt.sync()
        assert_is_the_oracles(host_copy(bufs), a.surfaces, f"{base}: the replay after the count launches")
        assert rt.debug_prefix_tiles() == tiles
        # ... and between two replaying frames on two streams
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        b1 = frame(2, s1, "stream 1")
        assert counts("between two streams") == tiles
        b2 = frame(2, s2, "stream 2")
        s1.synchronize()
        s2.synchronize()
        assert_is_the_oracles(host_copy(b1), a.surfaces, f"{base}: stream 1's replay")
        assert_is_the_oracles(host_copy(b2), a.surfaces, f"{base}: stream 2's replay")
        assert rt.debug_prefix_tiles() == tiles
    finally:
        rt.close()
