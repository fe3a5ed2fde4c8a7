"""Adaptive sampling on the GPU (include/rt_mi355.h): rt_accum_select's list and state, rt_camera_rays_at's rays, rt_accum_add_at's
accumulator and state, bit for bit, against the numpy restatement of tests/adaptive_oracle.py -- on accumulators planted by hand over
ragged shapes and every capacity around nSelected, run to run over dirty buffers, over sequences of calls with changing lists and every
special sample, chained behind the renderer on one caller's stream; then every refusal.  Every comparison is exact equality; guard
bytes around every buffer the calls write stay untouched."""
import ctypes

import numpy as np
import pytest

import accum_oracle as AO
import adaptive_oracle as DO
import denoise_oracle as NO
import meter_oracle as MO
from opengl_raytracing_amd import layout as L
from test_accum import SENTINEL, Guarded, check_accum, check_state, same_bits, up

pytestmark = pytest.mark.gpu

INVALID, TOO_LARGE = -1, -4
F = np.float32
DESC = dict(rel_error=0.15, lum_floor=2.0 ** -6, min_samples=3, done_permille=400)
# 2056 x 520 pixels are 257 x 65 = 16705 tiles = 523 chunks of 32 tiles: more than the 512 workgroups the selection's grid has at most
# (kSelectMaxWgs, csrc/rt_adaptive.h), so every workgroup owns two chunks, the last ones fewer, and the last chunk is ragged (1 tile)
MANY_CHUNKS = (2056, 520)


@pytest.fixture(scope="module")
def rt(host):
    t = host.RayTracer(0)
    yield t
    t.close()


class Device:
    """Guarded accumulator, accumulation state, pixel list (room for every pixel and one more), scratch and select state of one shape."""

    def __init__(self, host, w, h, acc=None):
        self.w, self.h = w, h
        self.accum = Guarded(w * h * 32, acc)
        self.state = Guarded(1024)
        self.list = Guarded((w * h + 1) * 8)
        self.scratch = Guarded(host.accum_select_layout(w, h))
        self.sel = Guarded(64)

    def select(self, rt, capacity, max_samples, **desc):
        """One rt_accum_select over a list buffer refilled with the guard pattern -> (the whole list buffer as uint32 rows, the state)."""
        self.list.t.fill_(SENTINEL)
        rt.accum_select(self.accum.t, self.list.t if capacity else None, capacity, self.scratch.t, self.sel.t, self.w, self.h,
                        max_samples=max_samples, **desc)
        self.scratch.read()
        return self.list.read().view(np.uint32).reshape(-1, 2), self.sel.read().view(L.SELECT_STATE_DTYPE)[0]

    def pixels(self, n):
        """The first n entries of the list as the int32 [n, 2] tensor shade_rays takes (shares the list's memory)."""
        import torch
        return self.list.t[: n * 8].view(torch.int32).view(n, 2)

    def read_accum(self):
        return self.accum.read().view(np.float32).reshape(2, self.h, self.w, 4)

    def read_state(self):
        return self.state.read().view(L.ACCUM_STATE_DTYPE)[0]


def check_select(dev, rt, acc, capacity, max_samples, what="", **desc):
    want_list, want = DO.select(acc, max_samples, capacity, **desc)
    got_list, got = dev.select(rt, capacity, max_samples, **desc)
    assert same_bits(DO.sel_state_bytes(got), DO.sel_state_bytes(want)), (what, capacity, DO.describe_sel_difference(got, want))
    n = int(want["nListed"])
    assert np.array_equal(got_list[:n], want_list), (what, capacity, "the list")
    assert (got_list[n:].view(np.uint8) == SENTINEL).all(), (what, capacity, "an entry behind nListed was written")
    return want


def check_capacities(dev, rt, acc, max_samples, what="", **desc):
    n = int(DO.select(acc, max_samples, 0, **desc)[1]["nSelected"])
    for cap in sorted({0, 1, max(n - 1, 0), n, n + 1}):
        want = check_select(dev, rt, acc, cap, max_samples, what, **desc)
        assert want["nSelected"] == n and want["nListed"] == min(n, cap)
    return n


# ---- 1. rt_accum_select ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", DO.SHAPES, ids=[f"{w}x{h}" for w, h in DO.SHAPES])
def test_select_planted_masks(rt, host, w, h):
    rng = np.random.default_rng(50 * w + h)
    dev = Device(host, w, h)
    for name, mask in DO.masks(w, h, rng).items():
        acc = DO.planted(w, h, mask)
        dev.accum.t.copy_(up(acc.view(np.uint8).reshape(-1)))
        n = check_capacities(dev, rt, acc, DO.PLANT_MAX_SAMPLES, name, **DO.PLANT_DESC)
        assert n == int(mask.sum()), name
        assert same_bits(dev.read_accum(), acc), (name, "the accumulator was written")


@pytest.mark.parametrize("w,h", DO.SHAPES, ids=[f"{w}x{h}" for w, h in DO.SHAPES])
def test_select_edge_cases(rt, host, w, h):
    """Counts on both sides of minSamples and maxSamples and at 2^24, r2 at thr2 and one float to either side, M2 = 0, a mean below the
    floor and a negative one (adaptive_oracle.edge_cases)."""
    desc, cap = DO.PLANT_DESC, DO.PLANT_MAX_SAMPLES
    acc = DO.edge_cases(w, h)
    dev = Device(host, w, h, acc)
    n = check_capacities(dev, rt, acc, cap, **desc)
    want = DO.select(acc, cap, w * h, **desc)[1]
    if w * h >= 600:                                            # the planted cases are the cases they claim to be
        j = AO.judge(acc, **desc)
        thr2 = F(desc["rel_error"]) * F(desc["rel_error"])
        at = j["sampled"] & (acc[1, ..., 0] == 1)
        for v in (thr2, np.nextafter(thr2, F(0)), np.nextafter(thr2, F(1))):
            assert (j["r2"][at] == v).any(), v
        assert 0 < n < w * h and want["nCapped"] > 0
        c = j["count"]
        sel, capped = DO.selected_mask(acc, cap, **desc)
        assert sel[c < 2].all() and not sel[c >= cap].any() and capped[(c == 2 ** 24) & ~j["converged"]].all()
        assert (j["converged"] & (acc[1, ..., 1] == 0) & (c >= desc["min_samples"])).any()
        assert sel[c == cap - 1].any() and capped[c == cap].any() and not sel[j["converged"]].any()
    # the cap alone: maxSamples 1 selects the empty pixels only, 2^24 everything unconverged but the saturated ones
    check_select(dev, rt, acc, w * h, 1, "maxSamples 1", **desc)
    check_select(dev, rt, acc, w * h, 2 ** 24, "maxSamples 2^24", **desc)


def test_select_more_chunks_than_workgroups(rt, host):
    w, h = MANY_CHUNKS
    assert ((w + 7) // 8) * ((h + 7) // 8) == 16705 > 512 * 32
    rng = np.random.default_rng(8)
    dev = Device(host, w, h)
    all_masks = DO.masks(w, h, rng)
    for name in ("random_50", "one_per_tile", "last", "all"):
        acc = DO.planted(w, h, all_masks[name])
        dev.accum.t.copy_(up(acc.view(np.uint8).reshape(-1)))
        n = int(all_masks[name].sum())
        for cap in sorted({n, max(n - 1, 0)}):
            want = check_select(dev, rt, acc, cap, DO.PLANT_MAX_SAMPLES, name, **DO.PLANT_DESC)
            assert want["nSelected"] == n
    assert same_bits(dev.read_accum(), acc)


def test_select_same_bytes_over_dirty_state_and_scratch(rt, host):
    import torch
    w, h = 130, 70
    rng = np.random.default_rng(21)
    acc = DO.planted(w, h, DO.masks(w, h, rng)["random_50"])
    dev = Device(host, w, h, acc)
    runs = []
    for k in range(3):
        dev.scratch.t.copy_(torch.from_numpy(rng.integers(0, 256, dev.scratch.n, dtype=np.uint8)).cuda())
        dev.sel.t.fill_(0x11 * (k + 1))
        lst, st = dev.select(rt, w * h, DO.PLANT_MAX_SAMPLES, **DO.PLANT_DESC)
        runs.append((lst.tobytes(), st.tobytes()))
    assert runs[0] == runs[1] == runs[2]
    want_list, want = DO.select(acc, DO.PLANT_MAX_SAMPLES, w * h, **DO.PLANT_DESC)
    assert runs[0][1] == DO.sel_state_bytes(want).tobytes()


# ---- 2. rt_camera_rays_at ----------------------------------------------------------------------------------------------------------------
def test_camera_rays_at_equals_camera_rays(rt, host):
    import torch
    from opengl_raytracing_amd import scenes
    sc = scenes.make_scene(3, host.generate_aabb)
    w, h = 96, 54
    rt.load(sc)
    sc.frame_count = 5
    p = sc.params(width=w, height=h)
    ref = rt.camera_rays(p)
    torch.cuda.synchronize()
    ref = ref.cpu().numpy()
    assert ref.shape == (h, w, 8)
    rng = np.random.default_rng(4)
    xs, ys = DO.tile_order(w, h)
    full = np.stack([xs, ys], axis=-1).astype(np.uint32)
    outside = np.array([[w, 0], [0, h], [w, h], [2 ** 32 - 1, 3], [3, 2 ** 32 - 1], [2 ** 32 - 1, 2 ** 32 - 1]], dtype=np.uint32)
    lists = [full[rng.permutation(len(full))], full] + [full[rng.permutation(len(full))[:n]] for n in (1, 63, 64, 65, 700)]
    lists.append(np.concatenate([outside, full[:58], outside]))
    window = sc.params(width=w, height=h)
    window.x0, window.y0, window.regionW, window.regionH = 8, 8, 16, 16        # ignored
    for k, lst in enumerate(lists):
        n = len(lst)
        rays = Guarded(n * 32)
        rays.t.fill_(SENTINEL)
        rt.camera_rays_at(window if k % 2 else p, up(lst.view(np.int32)), n, out=rays.t)
        got = rays.read().view(np.float32).reshape(n, 8)
        inside = (lst[:, 0] < w) & (lst[:, 1] < h)
        want = np.zeros((n, 8), dtype=np.float32)
        want[inside] = ref[lst[inside, 1].astype(np.int64), lst[inside, 0].astype(np.int64)]
        assert same_bits(got, want), (k, n)
    assert len(np.unique(ref[..., 4])) > w, "the jitter did not move the rays"


# ---- 3. rt_accum_add_at ------------------------------------------------------------------------------------------------------------------
def _changing_list(rng, w, h, k):
    """Call k's list: a shuffled share of the pixels that moves from call to call (everything on call 0), with out-of-image entries
    sprinkled in from call 1 on, and nothing at all on call 3."""
    xs, ys = DO.tile_order(w, h)
    full = np.stack([xs, ys], axis=-1).astype(np.uint32)
    if k == 0:
        return full
    if k == 3:
        return full[:0]
    keep = rng.permutation(len(full))[: max(1, int(len(full) * rng.uniform(0.05, 0.9)))]
    outside = np.array([[w, 0], [0, h], [2 ** 32 - 1, 2 ** 32 - 1]], dtype=np.uint32)
    lst = np.concatenate([full[keep], outside])
    return lst[rng.permutation(len(lst))]


@pytest.mark.parametrize("n", [1, 2, 3, 17])
@pytest.mark.parametrize("w,h", DO.SHAPES, ids=[f"{w}x{h}" for w, h in DO.SHAPES])
def test_add_at_sequence_matches_numpy(rt, host, w, h, n):
    rng = np.random.default_rng(4000 * w + 13 * h + n)
    frames = AO.noisy_frames(rng, AO.base_image(rng, w, h), n)
    dev = Device(host, w, h)
    acc = AO.empty(w, h)
    for k, img in enumerate(frames):
        lst = _changing_list(rng, w, h, k)
        inside = (lst[:, 0] < w) & (lst[:, 1] < h)
        samples = np.ones((len(lst), 4), dtype=np.float32)
        samples[inside] = img[lst[inside, 1].astype(np.int64), lst[inside, 0].astype(np.int64)]
        acc, want = DO.add_at(acc, samples, lst, k, **DESC)
        if len(lst):
            rt.accum_add_at(up(samples), up(lst.view(np.int32)), len(lst), dev.accum.t, dev.state.t, w, h, **DESC)
        else:
            rt.accum_add_at(None, None, 0, dev.accum.t, dev.state.t, w, h, **DESC)
        check_accum(dev.read_accum(), acc, f"call {k}")
        check_state(dev.read_state(), want, f"call {k}")
    assert want["frames"] == n and want["nPixels"] == w * h
    if n == 17 and w * h >= 600:
        assert want["minCount"] < want["maxCount"] and want["nRejected"] >= 3 and 0 < want["nConverged"] < w * h


def test_add_at_specials_and_outside_entries(rt, host):
    """Every special sample in every channel, and entries outside the image: refused ones leave the pixel's 32 bytes, all are counted."""
    w, h = 67, 9
    rng = np.random.default_rng(6)
    dev = Device(host, w, h)
    acc = AO.empty(w, h)
    xs, ys = DO.tile_order(w, h)
    full = np.stack([xs, ys], axis=-1).astype(np.uint32)
    for k in range(3):
        img = AO.noisy_frames(rng, AO.base_image(rng, w, h), 1, planted=False)[0]
        samples = img[ys, xs]
        samples.reshape(-1)[np.arange(0, samples.size, 5)[: 4 * len(AO.SPECIALS)]] = np.tile(AO.SPECIALS, 4)
        outside = np.array([[w, 0], [0, h], [w, h], [2 ** 31, 0], [2 ** 32 - 1, 2 ** 32 - 1]], dtype=np.uint32)
        lst = np.concatenate([outside, full])
        samples = np.concatenate([np.ones((len(outside), 4), dtype=np.float32), samples])
        acc, want = DO.add_at(acc, samples, lst, k, **DESC)
        rt.accum_add_at(up(samples), up(lst.view(np.int32)), len(lst), dev.accum.t, dev.state.t, w, h, **DESC)
        check_accum(dev.read_accum(), acc, f"call {k}")
        check_state(dev.read_state(), want, f"call {k}")
        assert want["nRejected"] >= len(outside) + AO.N_REJECTED_SPECIALS
    assert want["minCount"] < want["maxCount"] == 3


def test_add_at_more_chunks_than_workgroups(rt, host):
    """1031 x 599 pixels are 604 chunks of 1024 for the statistics' grid of two workgroups per CU (512 on an MI355X), as in
    test_accum.test_more_chunks_than_workgroups; the list is every other pixel."""
    w, h = 1031, 599
    rng = np.random.default_rng(32)
    frames = AO.noisy_frames(rng, AO.base_image(rng, w, h), 2)
    dev = Device(host, w, h)
    acc, _ = AO.accumulate(AO.empty(w, h), frames[0], 0, **DESC)
    rt.accum_add(up(frames[0]), dev.accum.t, dev.state.t, w, h, **DESC)
    xs, ys = DO.tile_order(w, h)
    lst = np.stack([xs, ys], axis=-1).astype(np.uint32)[::2]
    samples = frames[1][lst[:, 1].astype(np.int64), lst[:, 0].astype(np.int64)]
    acc, want = DO.add_at(acc, samples, lst, 1, **DESC)
    rt.accum_add_at(up(samples), up(lst.view(np.int32)), len(lst), dev.accum.t, dev.state.t, w, h, **DESC)
    check_accum(dev.read_accum(), acc)
    check_state(dev.read_state(), want)
    assert want["frames"] == 2 and want["maxCount"] == 2 and want["minCount"] <= 1


# ---- 4. the chain on the renderer --------------------------------------------------------------------------------------------------------
def _scene(rt, host):
    from opengl_raytracing_amd import scenes
    sc = scenes.make_scene(3, host.generate_aabb)
    rt.load(sc)
    return sc


def _full_frames(rt, sc, frame_counts, w, h, accum, state, stream, **desc):
    """rt_render_to + rt_accum_add of the given frameCounts on `stream` -> the colour tensors (kept alive by the caller)."""
    import torch
    colours = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in frame_counts]
    d_pos = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    d_nrm = torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    for c, k in zip(colours, frame_counts):
        sc.frame_count = k
        rt.render_to(sc.params(width=w, height=h), c.data_ptr(), d_pos.data_ptr(), d_nrm.data_ptr(), stream=stream.cuda_stream)
        rt.accum_add(c, accum.t, state.t, w, h, stream=stream, **desc)
    return colours, (d_pos, d_nrm)


def _adaptive_frames(rt, sc, frame_counts, w, h, dev, n, stream, **desc):
    """camera_rays_at -> shade_rays -> accum_add_at of the first n entries of dev's list for the given frameCounts on `stream`."""
    import torch
    keep = []
    pixels = dev.pixels(n)
    for k in frame_counts:
        sc.frame_count = k
        p = sc.params(width=w, height=h)
        rays = rt.camera_rays_at(p, pixels, n, stream=stream)
        colour = rt.shade_rays(p, rays, pixels=pixels, stream=stream, position=False, normal=False)[0]
        rt.accum_add_at(colour, pixels, n, dev.accum.t, dev.state.t, w, h, stream=stream, **desc)
        keep.append((rays, colour))
    return keep


def test_chain_on_an_empty_accumulator_equals_full_frames(rt, host):
    """(a) rt_accum_select lists every pixel of an empty accumulator; four frames of camera_rays_at -> shade_rays -> accum_add_at leave
    accumulator and state byte-identical to rt_render_to + rt_accum_add of the same four frameCounts.  One stream, one wait."""
    import torch
    sc = _scene(rt, host)
    w, h = 96, 54
    full_accum, full_state = Guarded(w * h * 32), Guarded(1024)
    dev = Device(host, w, h)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        keep_full = _full_frames(rt, sc, range(4), w, h, full_accum, full_state, s, **DESC)
        rt.accum_select(dev.accum.t, dev.list.t, w * h, dev.scratch.t, dev.sel.t, w, h, stream=s, **DESC)
        keep = _adaptive_frames(rt, sc, range(4), w, h, dev, w * h, s, **DESC)
    s.synchronize()
    sel = dev.sel.read().view(L.SELECT_STATE_DTYPE)[0]
    assert sel["nSelected"] == sel["nListed"] == w * h and sel["overflow"] == 0
    xs, ys = DO.tile_order(w, h)
    assert np.array_equal(dev.list.read().view(np.uint32).reshape(-1, 2)[: w * h], np.stack([xs, ys], axis=-1))
    want_acc = full_accum.read().view(np.float32).reshape(2, h, w, 4)
    check_accum(dev.read_accum(), want_acc)
    check_state(dev.read_state(), full_state.read().view(L.ACCUM_STATE_DTYPE)[0])
    assert (AO.counts(want_acc) == 4).all() and dev.read_state()["frames"] == 4
    assert not same_bits(keep_full[0][0].cpu().numpy(), keep_full[0][1].cpu().numpy()), "frameCount did not move the samples"
    del keep


CHAIN_DESC = dict(rel_error=0.05, lum_floor=2.0 ** -6, min_samples=3, done_permille=950)


def test_chain_after_full_frames_touches_listed_pixels_only(rt, host):
    """(b) Eight full frames, then rt_accum_select at relError 0.05 (the oracle, fed with the device's accumulator bytes, selects a
    share of the pixels that is neither nothing nor everything: 1120 of 5184, 21.6 %), then four adaptive frames: listed pixels hold the
    bytes the full path gives them for those frameCounts, unlisted pixels keep theirs, the state is the oracle's report; then
    denoise_guide -> denoise -> meter -> display_pack(toned) on the adaptive accumulator, each against its oracle."""
    import torch
    sc = _scene(rt, host)
    w, h = 96, 54
    desc = CHAIN_DESC
    mdesc = dict(key=0.3, low_permille=5, high_permille=5)
    table, tables = host.display_srgb_thresholds(), host.meter_tables()
    full_accum, full_state = Guarded(w * h * 32), Guarded(1024)
    dev = Device(host, w, h)
    guide, scratch, out = Guarded(w * h * 16), Guarded(w * h * 32), Guarded(w * h * 16)
    d_meter, d_packed = Guarded(1088), Guarded(w * h * 4)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        keep1 = _full_frames(rt, sc, range(8), w, h, full_accum, full_state, s, **desc)
        dev.accum.t.copy_(full_accum.t, non_blocking=True)
        dev.state.t.copy_(full_state.t, non_blocking=True)
        rt.accum_select(dev.accum.t, dev.list.t, w * h, dev.scratch.t, dev.sel.t, w, h, stream=s, **desc)
    s.synchronize()
    acc8 = dev.read_accum()
    want_list, want_sel = DO.select(acc8, 2 ** 24, w * h, **desc)
    n = int(want_sel["nSelected"])
    print(f"selected share after 8 frames at relError {desc['rel_error']}: {n} of {w * h} = {n / (w * h):.3f}")
    assert 0 < n < w * h
    sel = dev.sel.read().view(L.SELECT_STATE_DTYPE)[0]
    assert same_bits(DO.sel_state_bytes(sel), DO.sel_state_bytes(want_sel)), DO.describe_sel_difference(sel, want_sel)
    assert np.array_equal(dev.list.read().view(np.uint32).reshape(-1, 2)[:n], want_list)
    with torch.cuda.stream(s):
        keep2 = _full_frames(rt, sc, range(8, 12), w, h, full_accum, full_state, s, **desc)
        keep3 = _adaptive_frames(rt, sc, range(8, 12), w, h, dev, n, s, **desc)
        sc.frame_count = 0
        p = sc.params(width=w, height=h)
        d_hits = rt.trace_rays(rt.camera_rays(p, stream=s), "closest", stream=s)
        rt.denoise_guide(d_hits, w, h, out=guide.t, stream=s)
        rt.denoise(rt.accum_mean(dev.accum.t, w, h), rt.accum_moments(dev.accum.t, w, h), guide.t, scratch.t, out.t, w, h, stream=s)
        rt.meter(out.t, d_meter.t, w, h, stream=s, **mdesc)
        rt.display_pack(out.t, d_packed.t, w, h, format="srgb", flip=True, exposure=0.75, stream=s, tone="aces",
                        d_exposure=d_meter.t.data_ptr() + L.METER_EXPOSURE_OFFSET)
    s.synchronize()
    acc12 = full_accum.read().view(np.float32).reshape(2, h, w, 4)
    listed = np.zeros((h, w), dtype=bool)
    listed[want_list[:, 1], want_list[:, 0]] = True
    want_acc = np.where(listed[None, :, :, None], acc12, acc8)
    got_acc = dev.read_accum()
    check_accum(got_acc, want_acc)
    c = AO.counts(got_acc)
    assert (c[listed] == 12).all() and (c[~listed] == 8).all()
    check_state(dev.read_state(), AO.report(want_acc, [0], 11, **desc))
    # the display chain on the adaptive accumulator
    hits = d_hits.cpu().numpy().reshape(h, w, 8).view(L.HIT_DTYPE).reshape(h, w)
    gd = NO.guide(hits)
    assert same_bits(guide.read().view(L.DENOISE_GUIDE_DTYPE).reshape(h, w), gd)
    want = NO.denoise(want_acc[0], want_acc[1], gd)
    got_out = out.read().view(np.float32).reshape(h, w, 4)
    assert same_bits(got_out, want["out"]), "denoise"
    want_meter = MO.meter(want["out"], np.zeros(1, dtype=L.METER_STATE_DTYPE)[0], tables, **mdesc)
    got_meter = d_meter.read().view(L.METER_STATE_DTYPE)[0]
    assert same_bits(MO.state_bytes(got_meter), MO.state_bytes(want_meter)), MO.describe_difference(got_meter, want_meter)
    got = d_packed.read().reshape(h, w, 4)
    assert (got == MO.pack_toned(want["out"], "srgb", True, 0.75, table, "aces", dev_exposure=want_meter["exposure"])).all()
    del keep1, keep2, keep3


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(rt, host):
    import torch
    sc = _scene(rt, host)
    w, h = 16, 12
    rng = np.random.default_rng(78)
    acc0 = DO.planted(w, h, DO.masks(w, h, rng)["random_50"])
    dev = Device(host, w, h, acc0)
    want_list, want_sel = DO.select(acc0, DO.PLANT_MAX_SAMPLES, w * h, **DO.PLANT_DESC)
    n = len(want_list)
    samples = AO.noisy_frames(rng, AO.base_image(rng, 1, n), 1, planted=False)[0].reshape(n, 4)
    d_samples = up(samples)
    rays = Guarded(w * h * 32)
    lib, ctx, vp = rt.lib, rt.ctx, ctypes.c_void_p
    p = sc.params(width=w, height=h)

    def desc(**kw):
        d = L.make_accum_desc(w, h, **DO.PLANT_DESC)
        for k, v in kw.items():
            if k == "reserved":
                d.reserved[v] = 1
            else:
                setattr(d, k, v)
        return d

    def ref(d):
        return ctypes.byref(d) if d is not None else None

    a, st, px, scr, sl, sm, ry = (x.data_ptr() for x in (dev.accum.t, dev.state.t, dev.list.t, dev.scratch.t, dev.sel.t, d_samples, rays.t))

    def select(accum=a, d="default", max_samples=DO.PLANT_MAX_SAMPLES, pixels=px, capacity=w * h, scratch=scr, sel=sl, c=ctx):
        return lib.rt_accum_select(c, vp(accum), ref(desc() if d == "default" else d), max_samples, vp(pixels), capacity, vp(scratch), vp(sel), None)

    def add_at(smp=sm, pixels=px, count=n, accum=a, d="default", state=st, c=ctx):
        return lib.rt_accum_add_at(c, vp(smp), vp(pixels), count, vp(accum), ref(desc() if d == "default" else d), vp(state), None)

    def rays_at(params=p, pixels=px, count=n, out=ry, c=ctx):
        return lib.rt_camera_rays_at(c, ctypes.byref(params) if params is not None else None, vp(pixels), count, vp(out), None)

    def still_works():
        dev.accum.t.copy_(up(acc0.view(np.uint8).reshape(-1)))
        dev.state.t.zero_()
        torch.cuda.synchronize()
        assert select() == 0 and rays_at() == 0 and add_at() == 0
        rt.sync()
        got_sel = dev.sel.read().view(L.SELECT_STATE_DTYPE)[0]
        assert same_bits(DO.sel_state_bytes(got_sel), DO.sel_state_bytes(want_sel))
        assert np.array_equal(dev.list.read().view(np.uint32).reshape(-1, 2)[:n], want_list)
        want_acc, want_state = DO.add_at(acc0, samples, want_list, 0, **DO.PLANT_DESC)
        check_accum(dev.read_accum(), want_acc)
        check_state(dev.read_state(), want_state)
        rays.read()

    still_works()
    nan, inf = float("nan"), float("inf")
    bad = [desc(width=0), desc(width=-2), desc(height=0), desc(height=-1), desc(relError=0.0), desc(relError=-1.0), desc(relError=nan),
           desc(relError=inf), desc(lumFloor=0.0), desc(lumFloor=2.0 ** -41), desc(lumFloor=nan), desc(lumFloor=inf), desc(minSamples=1),
           desc(minSamples=-1), desc(donePermille=0), desc(donePermille=1001), desc(reserved=0), desc(reserved=1), desc(reserved=2),
           desc(reserved=3), None]
    for k, d in enumerate(bad):
        assert select(d=d) == INVALID, k
        assert add_at(d=d) == INVALID, k
    for m in (0, 2 ** 24 + 1, 2 ** 32 - 1):
        assert select(max_samples=m) == INVALID, m
    still_works()
    nb = w * h * 32
    for kw in [dict(accum=None), dict(scratch=None), dict(sel=None), dict(pixels=None), dict(accum=a + 8), dict(scratch=scr + 8), dict(sel=sl + 4),
               dict(pixels=px + 4), dict(pixels=a), dict(pixels=a + nb - 8), dict(scratch=a + 16), dict(scratch=a + nb - 16), dict(sel=a + 32),
               dict(sel=a + nb - 16), dict(accum=px), dict(accum=scr), dict(c=None)]:
        assert select(**kw) == INVALID, kw
    assert select(pixels=None, capacity=0) == 0                 # a pure count needs no list
    for kw in [dict(smp=None), dict(pixels=None), dict(accum=None), dict(state=None), dict(smp=sm + 8), dict(pixels=px + 4), dict(accum=a + 4),
               dict(state=st + 8), dict(smp=a), dict(smp=a + nb - 16), dict(pixels=a + 8), dict(pixels=a + nb - 8), dict(state=a + 16),
               dict(state=a + nb - 16), dict(accum=st), dict(c=None)]:
        assert add_at(**kw) == INVALID, kw
    still_works()
    huge = desc(width=65536, height=32768)                      # 2^31 pixels
    assert select(d=huge) == TOO_LARGE and add_at(d=huge) == TOO_LARGE
    assert add_at(count=(2 ** 31 - 1) * 256 + 1) == TOO_LARGE and rays_at(count=(2 ** 31 - 1) * 256 + 1) == TOO_LARGE
    # rt_camera_rays_at: what rt_pick's validation of the parameters refuses, and its own pointers
    deep = sc.params(width=w, height=h)
    deep.maxRayDepth = 33
    flat = sc.params(width=w, height=h)
    flat.width = 0
    for kw in [dict(params=None), dict(params=deep), dict(params=flat), dict(pixels=None), dict(out=None), dict(pixels=px + 4), dict(out=ry + 8), dict(c=None)]:
        assert rays_at(**kw) == INVALID, list(kw)
    assert rays_at(pixels=None, out=None, count=0) == 0
    still_works()
    torch.cuda.synchronize()
