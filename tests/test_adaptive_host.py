"""CPU-only tests of adaptive sampling's host side (include/rt_mi355.h): rt_select_state in C and in ctypes, rt_accum_select_layout, the
refusals the host decides alone, that the benchmark tool parses its arguments without a device -- and the numpy oracle of
tests/adaptive_oracle.py against the definition's own words: the list's order, the capacity's prefix, add_at against accum_oracle.add,
and the adaptive loop against uniform frames on a noisy image.  No GPU call is made."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import accum_oracle as AO
import adaptive_oracle as DO
from opengl_raytracing_amd import layout as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, TOO_LARGE = -1, -4
F = np.float32
DESC = dict(rel_error=0.15, lum_floor=2.0 ** -6, min_samples=3, done_permille=400)


# ---- layouts --------------------------------------------------------------------------------------------------------------------------
def test_select_state_in_c_and_ctypes(host, tmp_path):
    assert ctypes.sizeof(L.RtSelectState) == 64 == L.SELECT_STATE_DTYPE.itemsize == L.SELECT_STATE_BYTES
    fields = dict(nPixels=0, nSelected=4, nListed=8, capacity=12, overflow=16, nCapped=20, reserved=24)
    for k, v in fields.items():
        assert L.SELECT_STATE_DTYPE.fields[k][1] == v and getattr(L.RtSelectState, k).offset == v, k
    assert L.SELECT_NSELECTED_OFFSET == 4
    checks = " && ".join([f"offsetof(rt_select_state, {k}) == {v}" for k, v in fields.items()] + ["sizeof(rt_select_state) == 64"])
    src = tmp_path / "a.c"
    src.write_text('#include <stddef.h>\n#include "rt_mi355.h"\nint main(void){ return (' + checks + ") ? 0 : 1; }\n")
    exe = tmp_path / "a"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
    for name in ("rt_accum_select_layout", "rt_accum_select", "rt_camera_rays_at", "rt_accum_add_at"):
        assert name in host.EXPORTS and getattr(host.load_library(), name)


def test_select_layout_is_monotone_in_16_byte_steps(host):
    sizes = [(1, 1), (8, 8), (9, 8), (9, 9), (67, 9), (130, 70), (1920, 1080), (3840, 2160), (46340, 46340), (2 ** 31 - 1, 1), (1, 2 ** 31 - 1)]
    prev = 0
    for w, h in sizes:
        n = host.accum_select_layout(w, h)
        tiles = ((w + 7) // 8) * ((h + 7) // 8)
        assert n % 16 == 0 and n >= 8 * tiles, (w, h)
        assert host.RayTracer.accum_select_layout(w, h) == n
        if w * h >= 64 and max(w, h) < 2 ** 20:
            assert n >= prev, (w, h)
            prev = n
    for w in range(1, 40):                                      # monotone in each dimension
        assert host.accum_select_layout(w + 1, 17) >= host.accum_select_layout(w, 17)
        assert host.accum_select_layout(17, w + 1) >= host.accum_select_layout(17, w)
    lib = host.load_library()
    n = ctypes.c_size_t(7)
    assert lib.rt_accum_select_layout(4, 4, None) == INVALID
    for w, h in [(0, 4), (4, 0), (-1, 4), (4, -3)]:
        assert lib.rt_accum_select_layout(w, h, ctypes.byref(n)) == INVALID, (w, h)
    for w, h in [(65536, 32768), (2 ** 31 - 1, 2)]:
        assert lib.rt_accum_select_layout(w, h, ctypes.byref(n)) == TOO_LARGE, (w, h)
    assert n.value == 7, "a refusal wrote its output"


def test_null_context_is_refused(host):
    lib, vp = host.load_library(), ctypes.c_void_p
    d = L.make_accum_desc(4, 4)
    assert lib.rt_accum_select(None, vp(4096), ctypes.byref(d), 16, vp(8192), 4, vp(16384), vp(32768), None) == INVALID
    assert lib.rt_accum_add_at(None, vp(4096), vp(8192), 4, vp(16384), ctypes.byref(d), vp(32768), None) == INVALID
    assert lib.rt_camera_rays_at(None, None, vp(4096), 4, vp(8192), None) == INVALID


def test_tool_help_needs_no_device():
    run = subprocess.run([sys.executable, os.path.join(REPO, "tools", "bench_adaptive.py"), "--help"], capture_output=True, text=True,
                         env={**os.environ, "HIP_VISIBLE_DEVICES": "-1"})
    assert run.returncode == 0, run.stderr
    for option in ("--out", "--frames", "--repeats", "--parent-lib"):
        assert option in run.stdout


# ---- the oracle against the definition ------------------------------------------------------------------------------------------------
def _slow_order(w, h):
    """The definition's order, one pixel at a time."""
    tx_n = (w + 7) // 8
    return sorted(((x, y) for y in range(h) for x in range(w)), key=lambda p: ((p[1] // 8) * tx_n + p[0] // 8, p[1] % 8, p[0] % 8))


@pytest.mark.parametrize("w,h", DO.SHAPES, ids=[f"{w}x{h}" for w, h in DO.SHAPES])
def test_list_is_the_unconverged_uncapped_pixels_in_tile_order(w, h):
    rng = np.random.default_rng(100 * w + h)
    frames = AO.noisy_frames(rng, AO.base_image(rng, w, h), 9)
    acc = AO.empty(w, h)
    for x in frames:
        acc, _ = AO.add(acc, x)
    AO.set_counts(acc, rng.uniform(0, 1, (h, w)) < 0.1, 9 + 3)         # some pixels at a cap of 12
    j = AO.judge(acc, **DESC)
    want = [(x, y) for x, y in _slow_order(w, h) if not j["converged"][y, x] and j["count"][y, x] < 12]
    capped = sum(1 for x, y in _slow_order(w, h) if not j["converged"][y, x] and j["count"][y, x] >= 12)
    lst, st = DO.select(acc, 12, w * h, **DESC)
    assert lst.dtype == np.uint32 and [tuple(p) for p in lst.tolist()] == want
    assert (int(st["nPixels"]), int(st["nSelected"]), int(st["nListed"]), int(st["capacity"]), int(st["overflow"]), int(st["nCapped"])) == \
        (w * h, len(want), len(want), w * h, 0, capped)
    assert not st["reserved"].any()
    if w * h > 64:
        assert 0 < len(want) < w * h and capped > 0
    # the capacity truncates to a prefix and leaves nSelected whole
    for cap in {0, 1, max(len(want) - 1, 0), len(want), len(want) + 1}:
        part, ps = DO.select(acc, 12, cap, **DESC)
        assert part.tolist() == lst[:cap].tolist()
        assert (int(ps["nSelected"]), int(ps["nListed"]), int(ps["capacity"]), int(ps["overflow"])) == (len(want), min(cap, len(want)), cap, int(len(want) > cap))
    # a pixel with fewer than two samples is selected whatever its moments say; max_samples = 1 caps everything that has a sample
    empty_list, es = DO.select(AO.empty(w, h), 1, w * h, **DESC)
    assert len(empty_list) == w * h and es["nCapped"] == 0
    one, _ = AO.add(AO.empty(w, h), frames[0])
    _, os_ = DO.select(one, 1, w * h, **DESC)
    assert os_["nSelected"] == int((AO.counts(one) == 0).sum()) and os_["nCapped"] == int((AO.counts(one) == 1).sum())


def test_tile_order_covers_every_pixel_once():
    for w, h in DO.SHAPES + [(8, 8), (16, 8), (9, 17)]:
        xs, ys = DO.tile_order(w, h)
        assert list(zip(xs.tolist(), ys.tolist())) == _slow_order(w, h)


@pytest.mark.parametrize("w,h", [(5, 3), (67, 9), (130, 70)])
def test_add_at_is_add_on_the_listed_pixels(w, h):
    rng = np.random.default_rng(7 * w + h)
    frames = AO.noisy_frames(rng, AO.base_image(rng, w, h), 4)
    acc = AO.empty(w, h)
    for x in frames[:3]:
        acc, _ = AO.add(acc, x)
    xs, ys = DO.tile_order(w, h)
    full = np.stack([xs, ys], axis=-1).astype(np.uint32)
    img = frames[3]
    # the full list: accum_oracle.accumulate, byte for byte
    want_acc, want_state = AO.accumulate(acc, img, 3, **DESC)
    got_acc, got_state = DO.add_at(acc, img[ys, xs], full, 3, **DESC)
    assert got_acc.tobytes() == want_acc.tobytes()
    assert AO.state_bytes(got_state).tobytes() == AO.state_bytes(want_state).tobytes(), AO.describe_difference(got_state, want_state)
    # a subset in a shuffled order: listed pixels as in the full add, no byte of an unlisted pixel changes
    keep = rng.permutation(len(full))[: max(1, len(full) // 3)]
    sub = full[keep]
    got_acc, got_state = DO.add_at(acc, img[sub[:, 1], sub[:, 0]], sub, 3, **DESC)
    listed = np.zeros((h, w), dtype=bool)
    listed[sub[:, 1], sub[:, 0]] = True
    assert got_acc[:, listed].tobytes() == want_acc[:, listed].tobytes()
    assert got_acc[:, ~listed].tobytes() == acc[:, ~listed].tobytes()
    assert got_state["frames"] == 4 and AO.state_bytes(got_state).tobytes() == AO.state_bytes(AO.report(got_acc, [got_state["nRejected"]], 3, **DESC)).tobytes()
    # the empty list: the report of the accumulator as it stands, one more frame
    same_acc, st = DO.add_at(acc, np.zeros((0, 4), dtype=np.float32), np.zeros((0, 2), dtype=np.uint32), 3, **DESC)
    assert same_acc.tobytes() == acc.tobytes() and st["frames"] == 4 and st["nRejected"] == 0
    assert st["nConverged"] == int(AO.judge(acc, **DESC)["converged"].sum())


def test_outside_entries_and_special_samples_only_move_nrejected():
    w, h = 67, 9
    rng = np.random.default_rng(5)
    acc = AO.empty(w, h)
    for x in AO.noisy_frames(rng, AO.base_image(rng, w, h), 3, planted=False):
        acc, _ = AO.add(acc, x)
    outside = np.array([[w, 0], [0, h], [w, h], [2 ** 32 - 1, 0], [0, 2 ** 32 - 1], [2 ** 32 - 1, 2 ** 32 - 1]], dtype=np.uint32)
    refused = AO.SPECIALS[[0, 1, 2, 5, 6, 13]]
    inside = np.array([[k, k % h] for k in range(len(refused))], dtype=np.uint32)
    samples = np.ones((len(outside) + len(refused), 4), dtype=np.float32)
    samples[len(outside):, 1] = refused
    got, st = DO.add_at(acc, samples, np.concatenate([outside, inside]), 3, **DESC)
    assert got.tobytes() == acc.tobytes()
    assert st["nRejected"] == len(outside) + AO.N_REJECTED_SPECIALS and st["frames"] == 4
    base = AO.report(acc, [0], 3, **DESC)
    for k in L.ACCUM_STATE_DTYPE.names:
        if k != "nRejected":
            assert np.array_equal(st[k], base[k]), k
    # the accepted specials (zeros, denormals, -1, +-2^48) do move the pixel
    ok = np.array([v for v in AO.SPECIALS if np.isfinite(v) and abs(v) <= 2.0 ** 48], dtype=np.float32)
    samples = np.ones((len(ok), 4), dtype=np.float32)
    samples[:, 2] = ok
    pix = np.array([[3 * k, 1] for k in range(len(ok))], dtype=np.uint32)
    got, st = DO.add_at(acc, samples, pix, 3, **DESC)
    assert st["nRejected"] == 0 and (AO.counts(got)[1, pix[:, 0]] == 4).all()


# ---- the adaptive loop against uniform frames -------------------------------------------------------------------------------------------
def test_adaptive_loop_needs_fewer_samples_than_uniform_frames():
    """64 x 48: the left half bright and noisy (gamma(2, 1/2) factors), the right half quiet (factors within 2 %).  Uniform frames until
    `done`; the adaptive loop (select every frame, add_at of the same frame's samples at the listed pixels) until `done`.  A listed
    pixel sees the same samples in the same order under both loops until it stops, so at every frame the adaptive loop's converged set
    contains the uniform one's: it is done no later, and run on to the uniform loop's frame count it has converged every pixel the
    uniform loop has.  Measured: uniform sampling is done after 31 frames = 95 232 samples; the adaptive loop is done
    at frame 29 with 29 688 samples and holds 29 936 after 31 frames (the selected share falls from 100 % over 44 % at frame 5 to 4 %)."""
    w, h = 64, 48
    desc = dict(rel_error=0.125, lum_floor=2.0 ** -10, min_samples=4, done_permille=950)
    rng = np.random.default_rng(2025)
    base = AO.base_image(rng, w, h) + F(0.25)
    base[:, : w // 2] *= F(4.0)

    def frame(k):
        r = np.random.default_rng(1000 + k)
        f = r.gamma(2.0, 0.5, base.shape)
        f[:, w // 2:] = r.uniform(0.98, 1.02, (h, w - w // 2, 4))
        return (base * f).astype(np.float32)

    acc_u, n_u = AO.empty(w, h), 0
    while True:
        acc_u, st = AO.accumulate(acc_u, frame(n_u), n_u, **desc)
        n_u += 1
        if st["done"]:
            break
        assert n_u < 400
    total_u = int(AO.counts(acc_u).sum())
    assert total_u == n_u * w * h

    acc_a, n_a, done_at, shares = AO.empty(w, h), 0, None, []
    while n_a < n_u:
        lst, sel = DO.select(acc_a, 2 ** 24, w * h, **desc)
        shares.append(int(sel["nSelected"]) / (w * h))
        img = frame(n_a)
        acc_a, st = DO.add_at(acc_a, img[lst[:, 1], lst[:, 0]], lst, n_a, **desc)
        n_a += 1
        if st["done"] and done_at is None:
            done_at, total_at_done = n_a, int(AO.counts(acc_a).sum())
    total_a = int(AO.counts(acc_a).sum())
    print(f"uniform: {n_u} frames, {total_u} samples; adaptive: done at frame {done_at} with {total_at_done} samples, {total_a} after {n_a} frames; "
          f"selected share per frame {[round(s, 2) for s in shares]}")
    assert done_at is not None and done_at <= n_u
    assert total_at_done <= total_a < total_u
    conv_u, conv_a = AO.judge(acc_u, **desc)["converged"], AO.judge(acc_a, **desc)["converged"]
    assert conv_a[conv_u].all(), "a pixel that uniform sampling converged is not converged"
    assert shares[0] == 1.0 and shares[-1] < 0.5
