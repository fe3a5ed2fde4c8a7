"""The post passes on caller streams.  rt_taa_resolve, rt_bloom, rt_ssao and rt_ssao_blur are asynchronous on the hipStream
they are given; rt_bloom and rt_ssao work in scratch the context owns (the rgba16f ping-pong targets, the depth plane), one per
context whichever stream the call names.  include/rt_mi355.h states the rule: the passes may be issued on any streams
concurrently, the library orders the users of a scratch one behind the other with an event and waits on the host only before
the scratch grows or goes.  Here: each pass fed and drained on a stream of the caller's with the host running ahead; many calls
in flight on three streams, rt_frame among them; a frame size that grows the scratch in mid-run; the aliases the passes refuse.
Every result is compared bit for bit with the oracle's for that call's own input."""
import numpy as np
import pytest

from conftest import bits_equal

pytestmark = pytest.mark.gpu

W, H = 640, 360                 # the frames of the multi-stream runs
N_CALLS, N_STREAMS = 24, 3


@pytest.fixture(scope="module")
def rt(host):
    t = host.RayTracer(0)
    yield t
    t.close()


def _as_tensor(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.float16 else a)


def _up(*arrays):
    import torch
    out = [_as_tensor(a).cuda() for a in arrays]
    torch.cuda.synchronize()
    return out if len(out) > 1 else out[0]


def _hdr_scene(rng, w, h):
    sc = (rng.uniform(0, 1, (h, w, 4)) ** 4 * 8).astype(np.float32)
    sc[h // 2, w // 2, 0] = np.inf
    sc[1, 2, 1] = np.nan
    return sc


def _gbuffer(rng, w, h):
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


def _ssao_setup(host, w, h):
    samples, noise = host.ssao_kernel()
    view, proj = host.camera_matrices((0, 0, 0), (0, 0, -1), (0, 1, 0), 45.0, w / h)
    return noise, samples, proj, view


# ---- 1. the pass runs on the stream it is given -------------------------------------------------------------------------------
def _fed_on_stream(inputs, out_shape, launch):
    """inputs: host arrays.  On a fresh stream s: non-blocking copies of them from pinned memory into device buffers that hold
    zeros, launch(device pointers, out pointer, s.cuda_stream), a non-blocking copy of the output into pinned memory -- nothing
    in between waits on the host and the context's stream stays idle.  A pass that ran anywhere but behind the copies on s
    would read the zeros, and one s does not wait for would not have written the output by the time it is copied."""
    import torch
    s = torch.cuda.Stream()
    pinned = [_as_tensor(a).pin_memory() for a in inputs]
    dev = [torch.zeros(p.shape, dtype=p.dtype, device="cuda") for p in pinned]
    d_out = torch.full(out_shape, float("nan"), dtype=torch.float32, device="cuda")
    h_out = torch.zeros(out_shape, dtype=torch.float32).pin_memory()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for d, p in zip(dev, pinned):
            d.copy_(p, non_blocking=True)
        launch([d.data_ptr() for d in dev], d_out.data_ptr(), s.cuda_stream)
        h_out.copy_(d_out, non_blocking=True)
    s.synchronize()
    return h_out.numpy().copy()


FED_W, FED_H = 900, 400          # 5.8 MB per rgba32f surface: the copies that feed a pass take longer than its launch


def test_taa_on_caller_stream(rt, oracle):
    rng = np.random.default_rng(41)
    w, h = FED_W, FED_H
    cur = rng.uniform(0, 4, (h, w, 4)).astype(np.float32)
    his = rng.uniform(0, 4, (h, w, 4)).astype(np.float32)
    nrm = rng.normal(size=(h, w, 4)).astype(np.float16)
    nrm[rng.uniform(size=(h, w)) < 0.3] = 0
    jx, jy = 0.3 / w, -0.2 / h
    got = _fed_on_stream([cur, his, nrm], (h, w, 4),
                         lambda d, out, s: rt.taa_resolve(d[0], d[1], d[2], out, w, h, 0.3, jx, jy, stream=s))
    assert bits_equal(got, oracle.taa_resolve(cur, his, nrm, 0.3, jx, jy))


@pytest.mark.parametrize("iters", [10, 1])
def test_bloom_on_caller_stream(rt, oracle, iters):
    w, h = FED_W, FED_H
    sc = _hdr_scene(np.random.default_rng(42), w, h)
    got = _fed_on_stream([sc], (h, w, 4), lambda d, out, s: rt.bloom(d[0], out, w, h, 1.0, 0.5, iters, stream=s))
    assert bits_equal(got, oracle.bloom(sc, 1.0, 0.5, iters))


def test_ssao_on_caller_stream(rt, host, oracle):
    w, h = FED_W, FED_H
    pos, nrm = _gbuffer(np.random.default_rng(43), w, h)
    noise, samples, proj, view = _ssao_setup(host, w, h)
    got = _fed_on_stream([pos, nrm], (h, w), lambda d, out, s: rt.ssao(d[0], d[1], out, w, h, noise, samples, proj, view, stream=s))
    assert bits_equal(got, oracle.ssao(pos, nrm, noise, samples, proj, view))


@pytest.mark.parametrize("horizontal", [False, True])
def test_ssao_blur_on_caller_stream(rt, oracle, horizontal):
    w, h = FED_W, FED_H
    ao = np.random.default_rng(44).random((h, w)).astype(np.float32)
    got = _fed_on_stream([ao], (h, w), lambda d, out, s: rt.ssao_blur(d[0], out, w, h, horizontal, stream=s))
    assert bits_equal(got, oracle.ssao_blur(ao, horizontal))


# ---- 2. passes in flight on several streams ----------------------------------------------------------------------------------
def _streams(n):
    import torch
    return [torch.cuda.Stream() for _ in range(n)]


def test_blooms_in_flight_on_three_streams(rt, oracle):
    """24 calls round-robin on three streams, 10 and 3 iterations alternating (the fused chain; a fused pair with the trailing
    unfused pass), every call with its own input and output, the host running ahead.  All of them work in the context's one pair
    of ping-pong targets."""
    import torch
    rng = np.random.default_rng(45)
    scenes_ = [_hdr_scene(rng, W, H) for _ in range(N_CALLS)]
    d_in = _up(*scenes_)
    d_out = [torch.zeros_like(d) for d in d_in]
    torch.cuda.synchronize()
    streams = _streams(N_STREAMS)
    for k in range(N_CALLS):
        rt.bloom(d_in[k].data_ptr(), d_out[k].data_ptr(), W, H, 1.0, 0.5, 10 if k % 2 == 0 else 3,
                 stream=streams[k % N_STREAMS].cuda_stream)
    torch.cuda.synchronize()
    bad = [k for k in range(N_CALLS)
           if not bits_equal(d_out[k].cpu().numpy(), oracle.bloom(scenes_[k], 1.0, 0.5, 10 if k % 2 == 0 else 3))]
    assert not bad, f"calls {bad} of {N_CALLS} differ from the oracle of their own input"


def test_ssaos_in_flight_on_three_streams(rt, host, oracle):
    """The same for rt_ssao: every call's samples read the context's one depth plane."""
    import torch
    rng = np.random.default_rng(46)
    noise, samples, proj, view = _ssao_setup(host, W, H)
    gbufs = [_gbuffer(rng, W, H) for _ in range(N_CALLS)]
    d_pos = _up(*[g[0] for g in gbufs])
    d_nrm = _up(*[g[1] for g in gbufs])
    d_out = [torch.zeros((H, W), dtype=torch.float32, device="cuda") for _ in range(N_CALLS)]
    torch.cuda.synchronize()
    streams = _streams(N_STREAMS)
    for k in range(N_CALLS):
        rt.ssao(d_pos[k].data_ptr(), d_nrm[k].data_ptr(), d_out[k].data_ptr(), W, H, noise, samples, proj, view,
                stream=streams[k % N_STREAMS].cuda_stream)
    torch.cuda.synchronize()
    bad = [k for k in range(N_CALLS)
           if not bits_equal(d_out[k].cpu().numpy(), oracle.ssao(gbufs[k][0], gbufs[k][1], noise, samples, proj, view))]
    assert not bad, f"calls {bad} of {N_CALLS} differ from the oracle of their own input"


def test_frames_and_caller_stream_blooms_in_flight(rt, host, oracle):
    """rt_frame on the context's stream (its bloom runs in the same targets) between rt_bloom calls on two streams of the
    caller's: 24 calls, every third one a frame into a display surface of its own.  The frames repeat one image (no TAA, no AO,
    one frameCount), so one oracle render serves them all."""
    import torch
    from opengl_raytracing_amd import scenes
    sc = scenes.make_scene(2, host.generate_aabb)
    p = sc.params(width=W, height=H)
    rt.load(sc)
    rng = np.random.default_rng(47)
    kinds = ["frame" if k % N_STREAMS == 0 else "bloom" for k in range(N_CALLS)]
    inputs = [None if kind == "frame" else _hdr_scene(rng, W, H) for kind in kinds]
    d_in = [None if a is None else _up(a) for a in inputs]
    d_out = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(N_CALLS)]
    torch.cuda.synchronize()
    streams = _streams(N_STREAMS - 1)
    for k, kind in enumerate(kinds):
        if kind == "frame":
            rt.frame(p, enable_ao=False, enable_taa=False, bloom_iterations=10, d_display=d_out[k].data_ptr())
        else:
            rt.bloom(d_in[k].data_ptr(), d_out[k].data_ptr(), W, H, 1.0, 0.5, 10 if k % 2 == 0 else 3,
                     stream=streams[k % N_STREAMS - 1].cuda_stream)
    rt.sync()
    torch.cuda.synchronize()
    want_frame = oracle.bloom(oracle.render(sc, p)[0], 1.0, 0.5, 10)
    bad = [(k, kind) for k, kind in enumerate(kinds)
           if not bits_equal(d_out[k].cpu().numpy(),
                             want_frame if kind == "frame" else oracle.bloom(inputs[k], 1.0, 0.5, 10 if k % 2 == 0 else 3))]
    assert not bad, f"calls {bad} of {N_CALLS} differ from their oracle"


# ---- 3. a size change in mid-run -------------------------------------------------------------------------------------------------
def test_scratch_grows_between_streams(host, oracle):
    """A context of this test's own, so that the scratch starts empty: four blooms and four SSAOs at 320x200 on stream A, the same
    at 640x360 on stream B (both scratches grow while A's calls may still run in the old ones), 320x200 on A again -- no host
    synchronisation anywhere -- and the context destroyed with the last calls in flight."""
    import torch
    rng = np.random.default_rng(48)
    small, large = (320, 200), (W, H)
    plan = [(small, 0)] * 4 + [(large, 1)] * 4 + [(small, 0)] * 4
    sa, sb = _streams(2)
    calls = []
    for (w, h), which in plan:
        sc, (pos, nrm) = _hdr_scene(rng, w, h), _gbuffer(rng, w, h)
        d_sc, d_pos, d_nrm = _up(sc, pos, nrm)
        calls.append(dict(w=w, h=h, stream=(sa, sb)[which], sc=sc, pos=pos, nrm=nrm, d_sc=d_sc, d_pos=d_pos, d_nrm=d_nrm,
                          d_bloom=torch.zeros_like(d_sc), d_ao=torch.zeros((h, w), dtype=torch.float32, device="cuda"),
                          ssao=_ssao_setup(host, w, h)))
    torch.cuda.synchronize()
    rt2 = host.RayTracer(0)
    for c in calls:
        s = c["stream"].cuda_stream
        rt2.bloom(c["d_sc"].data_ptr(), c["d_bloom"].data_ptr(), c["w"], c["h"], 1.0, 0.5, 10, stream=s)
        rt2.ssao(c["d_pos"].data_ptr(), c["d_nrm"].data_ptr(), c["d_ao"].data_ptr(), c["w"], c["h"], *c["ssao"], stream=s)
    rt2.close()
    torch.cuda.synchronize()
    for k, c in enumerate(calls):
        assert bits_equal(c["d_bloom"].cpu().numpy(), oracle.bloom(c["sc"], 1.0, 0.5, 10)), f"bloom of call {k} ({c['w']}x{c['h']})"
        assert bits_equal(c["d_ao"].cpu().numpy(), oracle.ssao(c["pos"], c["nrm"], *c["ssao"])), f"ssao of call {k} ({c['w']}x{c['h']})"


# ---- 4. refused aliases ------------------------------------------------------------------------------------------------------
def test_in_place_calls_are_refused(rt, host):
    import torch
    w, h = 64, 32
    noise, samples, proj, view = _ssao_setup(host, w, h)
    d_scene = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    d_nrm = torch.zeros((h, w, 4), dtype=torch.int16, device="cuda")
    d_ao = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    d_out = torch.empty_like(d_scene)
    torch.cuda.synchronize()
    for iters in (0, 2, 10):
        with pytest.raises(host.RtError):
            rt.bloom(d_scene.data_ptr(), d_scene.data_ptr(), w, h, 1.0, 0.5, iters)
    with pytest.raises(host.RtError):
        rt.ssao(d_scene.data_ptr(), d_nrm.data_ptr(), d_scene.data_ptr(), w, h, noise, samples, proj, view)
    with pytest.raises(host.RtError):
        rt.ssao(d_scene.data_ptr(), d_nrm.data_ptr(), d_nrm.data_ptr(), w, h, noise, samples, proj, view)
    rt.bloom(d_scene.data_ptr(), d_out.data_ptr(), w, h, 1.0, 0.5, 2)       # the refusals left the context usable
    rt.ssao(d_scene.data_ptr(), d_nrm.data_ptr(), d_ao.data_ptr(), w, h, noise, samples, proj, view)
    rt.sync()
