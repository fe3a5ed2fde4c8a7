"""The post passes at frame scale.  Seven kernels cap their grid and walk the rest of the frame with a grid-stride loop:
rt_bloom_extract / rt_bloom_combine / rt_ssao_depth / rt_equirect_upload at 4096 blocks (1 048 576 elements),
rt_deinterleave / rt_wire_pack / rt_wire_unpack at 2048 blocks (524 288 units).  The other post tests stay far below both caps,
so only here does any of those loops take a second trip.  The base shape 2056x516 (1 060 896 px) is the smallest comfortable
frame above the larger cap and is ragged against every tile (2056 = 32*64 + 8, 516 = 21*24 + 12 = 16*32 + 4).  The second half
are extreme aspect ratios: many tile columns with few tile rows and the reverse, tile counts that are no multiple of 8, pixel
coordinates in the thousands.  Every comparison is bit for bit, against the CPU oracle or -- the pure copies -- against dist.py's
torch restatements and a numpy row gather written here.  DESIGN.md ("The post passes at frame scale and on caller streams")
has the measured conditions and what the mutations of the loops did to these tests."""
import ctypes

import numpy as np
import pytest

from conftest import bits_equal

pytestmark = pytest.mark.gpu

W0, H0 = 2056, 516
CAP_POST = 4096 * 256           # elements the first trip of the rt_post.hip loops covers
CAP_COPY = 2048 * 256           # units the first trip of the copy kernels' loops covers


@pytest.fixture(scope="module")
def rt(host):
    """The post passes do not depend on the ray-kernel variant: one context of this module's own."""
    t = host.RayTracer(0)
    yield t
    t.close()


def _up(*arrays):
    """Host arrays -> device tensors, complete before anything is launched on another stream."""
    import torch
    arrays = [np.ascontiguousarray(a) if a.flags.writeable else a.copy() for a in arrays]     # (torch wants writable memory)
    out = [torch.from_numpy(a.view(np.int16) if a.dtype == np.float16 else a).cuda() for a in arrays]
    torch.cuda.synchronize()
    return out if len(out) > 1 else out[0]


def _n_differ(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())


# ---- bloom ------------------------------------------------------------------------------------------------------------------
def _hdr_scene(w, h, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0, 1, (h, w, 4)) ** 4 * 8).astype(np.float32)


@pytest.fixture(scope="module")
def bloom_scene():
    """Random HDR data as in test_bloom.py, with one inf and one NaN texel in the part only the loops' second trip reaches."""
    sc = _hdr_scene(W0, H0, 21)
    flat = sc.reshape(-1, 4)
    flat[CAP_POST + 2056 * 2 + 100, 0] = np.inf
    flat[CAP_POST + 2056 * 4 + 2000, 1] = np.nan
    sc.setflags(write=False)
    return sc


def _bright_fraction(texels, threshold):
    """Share of texels the extract keeps (brightness_extractFS.glsl: dot(rgb, (0.2126, 0.7152, 0.0722)) > threshold)."""
    with np.errstate(invalid="ignore"):
        lum = texels[..., :3].astype(np.float64) @ np.array([0.2126, 0.7152, 0.0722])
        return float((lum > threshold).mean())


def _run_bloom(rt, scene, threshold, strength, iters):
    import torch
    h, w = scene.shape[:2]
    d_scene = _up(scene)
    d_out = torch.empty_like(d_scene)
    rt.bloom(d_scene.data_ptr(), d_out.data_ptr(), w, h, threshold, strength, iters)
    rt.sync()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("iters", [0, 1, 3, 10])
def test_bloom_frame_scale(rt, oracle, bloom_scene, iters):
    """0 and 1 iterations: only the unfused extract, blur and combine kernels; 3: a fused pair, then the trailing unfused pass and
    the combine; 10: the fused chain.  Both branches of the extract must be populated in the strided part."""
    frac = _bright_fraction(bloom_scene.reshape(-1, 4)[CAP_POST:], 1.0)
    print(f"bloom {W0}x{H0}: {frac:.3f} of the texels past element {CAP_POST} pass the threshold")
    assert 0.10 <= frac <= 0.90
    assert 0.10 <= _bright_fraction(bloom_scene, 1.0) <= 0.90
    want = oracle.bloom(bloom_scene, 1.0, 0.5, iters)
    got = _run_bloom(rt, bloom_scene, 1.0, 0.5, iters)
    assert bits_equal(got, want), f"{iters} iterations: {_n_differ(got, want)} values differ, " \
                                  f"{_n_differ(got.reshape(-1, 4)[CAP_POST:], want.reshape(-1, 4)[CAP_POST:])} of them past the cap"


@pytest.mark.parametrize("w,h", [(7680, 30), (70, 4320)])
def test_bloom_extreme_aspect(rt, oracle, w, h):
    """120 x 2 and 2 x 180 fused tiles through the XCD band map; the clamp of the taps at pixel coordinates in the thousands."""
    sc = _hdr_scene(w, h, 22)
    sc[h // 2, w // 2, 0] = np.inf
    sc[h - 1, w - 2, 1] = np.nan
    assert 0.10 <= _bright_fraction(sc, 1.0) <= 0.90
    want = oracle.bloom(sc, 1.0, 0.5, 10)
    got = _run_bloom(rt, sc, 1.0, 0.5, 10)
    assert bits_equal(got, want), f"{w}x{h}: {_n_differ(got, want)} values differ"


# ---- TAA --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(7680, 40), (64, 4320)])
def test_taa_extreme_aspect(rt, host, oracle, w, h):
    """The jitters of frames 1..3 at this size, none, and one of more than a texel.  At W = 7680 the history tap's
    floor(u*W - 0.5) lands on i-1 instead of i for some columns (fp32 rounding of (i+0.5)/W*W), at H = 4320 for some rows."""
    import torch
    rng = np.random.default_rng(23)
    cur = rng.uniform(0, 4, (h, w, 4)).astype(np.float32)
    his = rng.uniform(0, 4, (h, w, 4)).astype(np.float32)
    nrm = rng.normal(size=(h, w, 4)).astype(np.float16)
    nrm[rng.uniform(size=(h, w)) < 0.3] = 0
    cur[0, 1, 0] = np.nan
    his[h // 2, w // 2, 1] = np.inf
    d_cur, d_his, d_nrm = _up(cur, his, nrm)
    d_out = torch.empty_like(d_cur)
    jitters = [host.taa_jitter(f, w, h) for f in (1, 2, 3)] + [(0.0, 0.0), (1.7 / w, -2.3 / h)]
    for jx, jy in jitters:
        want = oracle.taa_resolve(cur, his, nrm, 0.3, jx, jy)
        rt.taa_resolve(d_cur.data_ptr(), d_his.data_ptr(), d_nrm.data_ptr(), d_out.data_ptr(), w, h, 0.3, jx, jy)
        rt.sync()
        got = d_out.cpu().numpy()
        assert bits_equal(got, want), f"{w}x{h} jitter ({jx},{jy}): {_n_differ(got, want)} values differ"


# ---- SSAO -------------------------------------------------------------------------------------------------------------------
def _gbuffer(w, h, seed):
    """A wall facing the camera at z = -5 minus a random depth in [0, 1), x and y on a 0.004 grid around the axis, random unit
    normals towards the camera (z >= 0.2 before normalising), rounded to half."""
    rng = np.random.default_rng(seed)
    pos = np.zeros((h, w, 4), np.float32)
    nrm = np.zeros((h, w, 4), np.float16)
    ys, xs = np.mgrid[0:h, 0:w]
    pos[..., 0] = (xs - w / 2) * 0.004
    pos[..., 1] = (ys - h / 2) * 0.004
    pos[..., 2] = -5 - rng.random((h, w)).astype(np.float32)
    pos[..., 3] = 1
    n = rng.normal(size=(h, w, 3)).astype(np.float32)
    n[..., 2] = np.abs(n[..., 2]) + 0.2
    nrm[..., :3] = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float16)
    nrm[..., 3] = 1
    return pos, nrm


def _ssao_and_blurs(rt, host, oracle, w, h, seed):
    import torch
    pos, nrm = _gbuffer(w, h, seed)
    samples, noise = host.ssao_kernel()
    view, proj = host.camera_matrices((0, 0, 0), (0, 0, -1), (0, 1, 0), 45.0, w / h)
    want = oracle.ssao(pos, nrm, noise, samples, proj, view)
    occluded = float((want < 1).mean())
    print(f"ssao {w}x{h}: {occluded:.3f} of the oracle's AO values are below 1")
    d_pos, d_nrm = _up(pos, nrm)
    d_ao = torch.empty((h, w), dtype=torch.float32, device="cuda")
    rt.ssao(d_pos.data_ptr(), d_nrm.data_ptr(), d_ao.data_ptr(), w, h, noise, samples, proj, view)
    rt.sync()
    got = d_ao.cpu().numpy()
    assert bits_equal(got, want), f"ssao {w}x{h}: {_n_differ(got, want)} values differ"
    d_b = torch.empty_like(d_ao)
    for hz in (0, 1):
        rt.ssao_blur(d_ao.data_ptr(), d_b.data_ptr(), w, h, hz)
        rt.sync()
        blurred, want_b = d_b.cpu().numpy(), oracle.ssao_blur(want, hz)
        assert bits_equal(blurred, want_b), f"blur {hz} {w}x{h}: {_n_differ(blurred, want_b)} values differ"
    return occluded


def test_ssao_frame_scale(rt, host, oracle):
    """rt_ssao_depth_kernel's loop strides here; the depth plane past the cap is what the last six rows' samples read."""
    assert _ssao_and_blurs(rt, host, oracle, W0, H0, 24) >= 0.50


@pytest.mark.parametrize("w,h", [(4096, 8), (4096, 12), (100, 256), (24, 4320)])
def test_ssao_extreme_aspect(rt, host, oracle, w, h):
    """ssao_nearest_repeat's power-of-two branch on both axes, on either one, on neither; frames one or two tiles thin."""
    assert _ssao_and_blurs(rt, host, oracle, w, h, 25) >= 0.50


# ---- equirect -> cubemap ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,min_reading_tail", [(32, 0), (256, 50)])
def test_cubemap_from_frame_scale_panorama(rt, oracle, size, min_reading_tail):
    """rt_equirect_upload_kernel strides on a 2056x516 panorama (random, not fp16-representable).  What the loop's second trip
    uploads is the top six rows, around the +Y pole: no texel of a 32-wide face samples them (its nearest texel centres are 0.044
    rad off the pole, the rows begin 0.033 rad off), so the 256-wide faces are what sees that trip.  How many face texels read the
    tail is counted on the CPU, by running the oracle on a panorama with the tail zeroed."""
    import torch
    rng = np.random.default_rng(26)
    pano = (rng.uniform(0, 1, (H0, W0, 3)) ** 3 * 20).astype(np.float32)
    want = oracle.equirect_to_cubemap(pano, size)
    cut = pano.copy()
    cut.reshape(-1, 3)[CAP_POST:] = 0
    reading_tail = int((oracle.equirect_to_cubemap(cut, size).view(np.uint16) != want.view(np.uint16)).any(axis=-1).sum())
    print(f"cubemap S={size}: {reading_tail} face texels read the panorama past element {CAP_POST}")
    assert reading_tail >= min_reading_tail
    d_faces = torch.zeros((6, size, size, 3), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    rt.equirect_to_cubemap(pano, size, d_faces_out=d_faces.data_ptr())
    got = d_faces.cpu().numpy()
    assert (got.view(np.uint16) == want.view(np.uint16)).all(), f"S={size}: {int((got.view(np.uint16) != want.view(np.uint16)).sum())} halfs differ"


# ---- the copies -------------------------------------------------------------------------------------------------------------
BPP = (16, 16, 8)
DT = (np.uint32, np.uint32, np.uint16)      # the surfaces as raw words: 4 per pixel


def _random_surfaces(rng, rows, width):
    """Three surfaces of random bit patterns (as words), alpha = 1.0 on each: the wire format drops it."""
    col = rng.integers(0, 2 ** 32, (rows, width, 4), dtype=np.uint32)
    pos = rng.integers(0, 2 ** 32, (rows, width, 4), dtype=np.uint32)
    nrm = rng.integers(0, 2 ** 16, (rows, width, 4), dtype=np.uint16)
    col[..., 3] = pos[..., 3] = 0x3F800000
    nrm[..., 3] = 0x3C00
    return [col, pos, nrm]


def _rank_buffer(surfs):
    return np.concatenate([s.reshape(-1).view(np.uint8) for s in surfs])


def _owner_rows(height, strip_rows, world, w0):
    """(rank, local row) of every image row, written out here: cycles of w0 root strips, then one strip per peer."""
    cycle = (w0 + world - 1) * strip_rows
    ranks, local = np.empty(height, np.int64), np.empty(height, np.int64)
    for y in range(height):
        c, r = divmod(y, cycle)
        if r < w0 * strip_rows:
            ranks[y], local[y] = 0, c * w0 * strip_rows + r
        else:
            ranks[y], local[y] = 1 + (r - w0 * strip_rows) // strip_rows, c * strip_rows + (r - w0 * strip_rows) % strip_rows
    return ranks, local


def _gather_rows(per_rank, ranks, local):
    """Image-order surfaces from each rank's local ones."""
    return [np.stack([per_rank[r][s][ly] for r, ly in zip(ranks, local)]) for s in range(3)]


def _pack_numpy(surfs, wire_bytes):
    n = surfs[0].shape[0] * surfs[0].shape[1]
    wire = np.zeros(wire_bytes, np.uint8)
    wire[:12 * n] = np.ascontiguousarray(surfs[0].reshape(n, 4)[:, :3]).view(np.uint8).reshape(-1)
    wire[12 * n:24 * n] = np.ascontiguousarray(surfs[1].reshape(n, 4)[:, :3]).view(np.uint8).reshape(-1)
    wire[24 * n:30 * n] = np.ascontiguousarray(surfs[2].reshape(n, 4)[:, :3]).view(np.uint8).reshape(-1)
    return wire


def _words(t):
    """A device surface tensor as the raw words _random_surfaces makes."""
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.float16 else a.view(np.uint32)


def _same_bits(a, b):
    import torch
    it = torch.int16 if a.dtype == torch.float16 else torch.int32
    return torch.equal(a.view(it), b.view(it))


@pytest.mark.parametrize("world,strip_rows", [(3, 16), (8, 8)])
def test_copies_frame_scale(rt, world, strip_rows):
    """rt_deinterleave, rt_wire_pack and rt_wire_unpack on a 2056x516 frame of random bits: nothing is rendered.  The
    de-interleave of every surface (1028 or 2056 16-byte units per row x 516 rows) and the unpack (1 060 896 pixels) stride."""
    import torch
    from opengl_raytracing_amd import dist as D
    rng = np.random.default_rng(27 + world)
    plan = D.StripPlan(W0, H0, strip_rows, world)
    assert W0 * BPP[2] // 16 * H0 > CAP_COPY                # even the rgba16f surface is past the cap
    per_rank = [_random_surfaces(rng, plan.max_local_rows, W0) for _ in range(world)]
    ranks, local = _owner_rows(H0, strip_rows, world, 1)
    want = _gather_rows(per_rank, ranks, local)
    gathered = _up(np.stack([_rank_buffer(s) for s in per_rank]))
    assert gathered.shape == (world, plan.rank_bytes)
    outs = D.deinterleave_hip(rt, gathered, plan)
    rt.sync()
    for out, chk, ref in zip(outs, D.deinterleave_torch(gathered, plan), want):
        assert (_words(out) == ref).all(), f"deinterleave, world {world}"
        assert _same_bits(out, chk)
    wires = torch.zeros((world, plan.wire_bytes), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for r in range(world):
        D.pack_wire_hip(rt, D.surface_views(gathered[r], plan), wires[r], plan)
    rt.sync()
    for r in range(world):
        assert (wires[r].cpu().numpy() == _pack_numpy(per_rank[r], plan.wire_bytes)).all(), f"pack, world {world} rank {r}"
        assert torch.equal(wires[r], D.pack_wire_torch(D.surface_views(gathered[r], plan), plan))
    wouts = D.unpack_wire_hip(rt, wires, plan)
    rt.sync()
    for out, chk, ref in zip(wouts, D.unpack_wire_torch(wires, plan), want):
        assert (_words(out) == ref).all(), f"unpack, world {world}"       # alpha is 1.0 throughout, so the wire loses nothing
        assert _same_bits(out, chk)


def test_copies_frame_scale_weighted_root(rt):
    """Four ranks, 8-row strips, the root owning three strips of every cycle: its rows come from its local surfaces."""
    import torch
    from opengl_raytracing_amd import dist as D
    rng = np.random.default_rng(31)
    world, strip_rows, w0 = 4, 8, 3
    plan = D.StripPlan(W0, H0, strip_rows, world, w0)
    per_rank = [_random_surfaces(rng, plan.buffer_rows(r), W0) for r in range(world)]
    ranks, local = _owner_rows(H0, strip_rows, world, w0)
    want = _gather_rows(per_rank, ranks, local)
    root = _up(_rank_buffer(per_rank[0]))
    rviews = D.surface_views(root, plan, 0)
    wires = torch.zeros((world, plan.wire_bytes), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    peers = []
    for r in range(1, world):
        peers.append(_up(_rank_buffer(per_rank[r])))
        D.pack_wire_hip(rt, D.surface_views(peers[-1], plan, r), wires[r], plan)
    wouts = D.unpack_wire_hip(rt, wires, plan, root_views=rviews)
    rt.sync()
    for r in range(1, world):
        assert (wires[r].cpu().numpy() == _pack_numpy(per_rank[r], plan.wire_bytes)).all(), f"pack, rank {r}"
    for out, chk, ref in zip(wouts, D.unpack_wire_torch(wires, plan, root_views=rviews), want):
        assert (_words(out) == ref).all()
        assert _same_bits(out, chk)


def test_wire_pack_whole_frame(rt):
    """A rank's share of the plans above stays below rt_wire_pack's 524 288-pixel cap; the whole frame as one rank's (a world of
    one) does not."""
    import torch
    from opengl_raytracing_amd import dist as D
    rng = np.random.default_rng(32)
    plan = D.StripPlan(W0, H0, H0, 1)
    assert plan.rank_pixels == W0 * H0 > CAP_COPY
    surfs = _random_surfaces(rng, H0, W0)
    buf = _up(_rank_buffer(surfs))
    views = D.surface_views(buf, plan)
    wire = torch.zeros(plan.wire_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    D.pack_wire_hip(rt, views, wire, plan)
    rt.sync()
    assert (wire.cpu().numpy() == _pack_numpy(surfs, plan.wire_bytes)).all()
    assert torch.equal(wire, D.pack_wire_torch(views, plan))


# ---- rt_frame with other bloom chains ---------------------------------------------------------------------------------------
def _d2h(ptr, shape, dtype):
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = np.empty(shape, dtype=dtype)
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemcpy(out.ctypes.data, ctypes.c_void_p(ptr), out.nbytes, 2) == 0      # hipMemcpyDeviceToHost
    return out


FRAME_W, FRAME_H = 200, 120


@pytest.fixture(scope="module")
def frame_oracle(host, oracle):
    """Two frames of the C2 scene at 200x120 through the oracle, once for both bloom settings: the render, the blurred AO and
    the TAA history chain (none of which depends on the bloom)."""
    from opengl_raytracing_amd import scenes
    sc = scenes.make_scene(2, host.generate_aabb)
    w, h = FRAME_W, FRAME_H
    samples, noise = host.ssao_kernel()
    frames, hist = [], np.zeros((h, w, 4), np.float32)
    for frame in range(2):
        p = sc.params(width=w, height=h)
        p.frameCount = frame
        col, pos, nrm, _ = oracle.render(sc, p)
        nrm16 = np.ascontiguousarray(nrm).view(np.float16).reshape(h, w, 4)
        view, proj = host.camera_matrices(p.camPos[:], p.camDir[:], p.camUp[:], p.fovDeg, w / h)
        ao = oracle.ssao_blur(oracle.ssao(pos, nrm16, noise, samples, proj, view), False)
        jx, jy = oracle.taa_jitter(frame, w, h)
        hist = oracle.taa_resolve(col, hist, nrm16.astype(np.float32), 0.1, jx, jy)
        frames.append((p, col, ao, hist))
    return sc, samples, noise, frames


@pytest.mark.parametrize("iters", [0, 3])
def test_frame_with_other_bloom_chains(rt, frame_oracle, oracle, iters):
    """rt_frame with bloomIterations 0 (extract and combine alone) and 3 (fused pair, trailing pass): test_frame.py runs 10."""
    import torch
    sc, samples, noise, frames = frame_oracle
    w, h = FRAME_W, FRAME_H
    rt.load(sc)
    d_disp = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p0 = sc.params(width=w + 8, height=h)          # another size first: the history of the frames below starts as zeros
    rt.frame(p0, enable_ao=False, enable_taa=False, bloom_iterations=iters)
    for frame, (p, col, ao, hist) in enumerate(frames):
        rt.frame(p, enable_ao=True, enable_taa=True, taa_blend=0.1, bloom_iterations=iters, ao_samples=samples, ao_noise=noise,
                 d_display=d_disp.data_ptr())
        rt.sync()
        d_c, d_p, d_n, d_ao, d_hist = rt.frame_surfaces()
        assert bits_equal(_d2h(d_c, (h, w, 4), np.float32), col), f"colour, frame {frame}"
        assert bits_equal(_d2h(d_ao, (h, w), np.float32), ao), f"AO, frame {frame}"
        assert bits_equal(d_disp.cpu().numpy(), oracle.bloom(col, 1.0, 0.5, iters)), f"display, frame {frame}, {iters} iterations"
        assert bits_equal(_d2h(d_hist, (h, w, 4), np.float32), hist), f"history, frame {frame}"
