"""Secondary measurement (not the BASELINE metric): what progressive accumulation costs, at 1920x1080 and 3840x2160, all in one run:

  (a) rt_accum_add (clear + accumulate + solve) from device events over back-to-back launches on noisy content, beside a device copy
      that moves the same 80 bytes per pixel (40 read, 40 written) in the same run: the achieved bytes per second of both and the
      fraction.  The clear, the solve and the launches cost the same whatever the frame's size: rt_accum_add on a 1 x 1 frame is
      reported as that fixed part, the rest as the accumulate kernel.  Repeated launches over one accumulator are served by the
      Infinity Cache where it fits (1080p: 66 MB + 33 MB of image); the 4K accumulator (265 MB) does not.
      --variant NAME=PATH (repeatable) times libraries built with other RT_ACCUM_* macros (tools/build_variants.py) alternately
      with this build's, here and in the loop of (b): the kernel forms of DESIGN.md 20.
  (b) host loops on the context's own stream and surfaces: rt_render on a library built from the PARENT commit (--parent-lib) and on
      this build, alternating, and rt_render + rt_accum_add on this build.
  (c) how many samples per pixel and how much wall time the loop of (b) takes until state.done at relError 0.02 / donePermille 950,
      reading the 4 bytes of `done` every 8 frames, on C2 and on C3's scene (the one with the noise texture) at 1080p.

Writes one record per size to --out (default profiles/accum_bench.json)."""
import argparse, ctypes, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from opengl_raytracing_amd import host, scenes
from opengl_raytracing_amd import layout as L

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "accum_bench.json"))
ap.add_argument("--parent-lib", default=None, help="librt_mi355.so built from the parent commit (build_library(out=...))")
ap.add_argument("--variant", action="append", default=[], help="NAME=PATH of a library built with other RT_ACCUM_* macros")
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--launches", type=int, default=100)
ap.add_argument("--max-spp", type=int, default=4096)
args = ap.parse_args()


def tracer(path):
    """A RayTracer on the library at `path` (None: this build's)."""
    host._LIB = None
    if path:
        os.environ["RT_LIB"] = path
    try:
        return host.RayTracer(0)
    finally:
        os.environ.pop("RT_LIB", None)
        host._LIB = None


new = tracer(None)
old = tracer(args.parent_lib) if args.parent_lib else new
variants = {"this": new}
for spec in args.variant:
    name, _, path = spec.partition("=")
    variants[name] = tracer(path)
sc = scenes.make_scene(2, host.generate_aabb)
for t in {id(x): x for x in [new, old, *variants.values()]}.values():
    t.load(sc)
side = torch.cuda.Stream()
blocker_a = torch.zeros(256 << 20, dtype=torch.uint8, device="cuda")
blocker_b = torch.empty_like(blocker_a)


def hold(stream):
    """Keep `stream` busy for a few milliseconds so that the launches timed behind it are all queued before the first one starts."""
    with torch.cuda.stream(stream):
        for _ in range(40):
            blocker_b.copy_(blocker_a)


def device_us(launch, K):
    """Microseconds per call of launch() from device events around K back-to-back calls on `side`."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    hold(side)
    e0.record(side)
    for _ in range(K):
        launch()
    e1.record(side)
    side.synchronize()
    return e0.elapsed_time(e1) / K * 1e3


def alternate(launches, K, repeats):
    """launches: {name: callable}; every repeat times each once, in alternating order -> {name: [us per repeat]}."""
    for f in launches.values():
        for _ in range(10):
            f()
    side.synchronize()
    us = {k: [] for k in launches}
    for r in range(repeats):
        for k in (list(launches) if r % 2 == 0 else list(launches)[::-1]):
            us[k].append(device_us(launches[k], K))
    return us


def put(rec, key, us):
    rec[key + "_us"] = round(statistics.median(us), 2)
    rec[key + "_us_all"] = [round(x, 2) for x in us]


def check(t, rc, what):
    if rc:
        raise host.RtError(rc, f"{what}: {t.lib.rt_last_error(t.ctx).decode()}")


def render_loop(t, p, accum=None):
    """n frames of rt_render (+ rt_accum_add on the colour surface when `accum` = (d_accum, d_state, desc)) on t's own stream."""
    lib, ctx, d_color = t.lib, t.ctx, ctypes.c_void_p()
    check(t, lib.rt_render(ctx, ctypes.byref(p)), "rt_render")
    check(t, lib.rt_get_surfaces(ctx, ctypes.byref(d_color), None, None), "rt_get_surfaces")

    def loop(n):
        for _ in range(n):
            check(t, lib.rt_render(ctx, ctypes.byref(p)), "rt_render")
            if accum:
                check(t, lib.rt_accum_add(ctx, d_color, ctypes.c_void_p(accum[0].data_ptr()), ctypes.byref(accum[2]),
                                          ctypes.c_void_p(accum[1].data_ptr()), None), "rt_accum_add")
        t.sync()
    return loop


def until_done(t, scene, w, h):
    """Frames and seconds until state.done under the default description, the frame count moving the samples; `done` is read every
    8 frames (a 4-byte copy behind a sync of the context's stream)."""
    t.load(scene)
    d_accum, d_state = t.accum_alloc(w, h)
    desc = L.make_accum_desc(w, h)
    lib, ctx, d_color = t.lib, t.ctx, ctypes.c_void_p()
    done = torch.zeros(1, dtype=torch.int32).pin_memory()
    frames, t0 = 0, time.perf_counter()
    while frames < args.max_spp:
        scene.frame_count = frames
        p = scene.params(width=w, height=h)
        check(t, lib.rt_render(ctx, ctypes.byref(p)), "rt_render")
        check(t, lib.rt_get_surfaces(ctx, ctypes.byref(d_color), None, None), "rt_get_surfaces")
        check(t, lib.rt_accum_add(ctx, d_color, ctypes.c_void_p(d_accum.data_ptr()), ctypes.byref(desc), ctypes.c_void_p(d_state.data_ptr()), None), "rt_accum_add")
        frames += 1
        if frames % 8 == 0:
            t.sync()
            done.copy_(d_state[L.ACCUM_DONE_OFFSET: L.ACCUM_DONE_OFFSET + 4].view(torch.int32))
            if int(done[0]):
                break
    t.sync()
    seconds = time.perf_counter() - t0
    st = d_state.cpu().numpy().view(L.ACCUM_STATE_DTYPE)[0]
    return {"frames": frames, "seconds": round(seconds, 4), "done": int(st["done"]), "converged_share": round(int(st["nConverged"]) / (w * h), 4),
            "medianBin": int(st["medianBin"]), "p95Bin": int(st["p95Bin"]), "nUnsampled": int(st["nUnsampled"])}


records = []
for (w, h) in [(1920, 1080), (3840, 2160)]:
    rec = {"size": [w, h], "frames": args.frames, "repeats": args.repeats, "launches": args.launches,
           "parent": "parent build" if args.parent_lib else "this build"}
    rng = np.random.default_rng(w)
    base = (rng.uniform(0, 1, (h, w, 4)) ** 4 * 8).astype(np.float32)
    imgs = [torch.from_numpy((base * rng.gamma(2.0, 0.5, base.shape)).astype(np.float32)).cuda() for _ in range(2)]
    d_accum, d_state = new.accum_alloc(w, h)
    tiny_accum, tiny_state = new.accum_alloc(1, 1)
    copy_src = torch.zeros(w * h * 40, dtype=torch.uint8, device="cuda")
    copy_dst = torch.empty_like(copy_src)
    torch.cuda.synchronize()
    flip = [0]

    def add(t, img=None):
        flip[0] ^= 1
        t.accum_add(imgs[flip[0]], d_accum, d_state, w, h, stream=side)

    # ---- (a) the add beside a copy of the same bytes; the kernel forms beside each other
    launches = {"copy80": lambda: copy_dst.copy_(copy_src), "fixed": lambda: new.accum_add(imgs[0], tiny_accum, tiny_state, 1, 1, stream=side)}
    for name, t in variants.items():
        launches["add_" + name] = lambda t=t: add(t)
    with torch.cuda.stream(side):
        us = alternate(launches, args.launches, args.repeats)
    for k, v in us.items():
        put(rec, k, v)
    nbytes = w * h * 80
    rec["copy80_TBps"] = round(nbytes / rec["copy80_us"] * 1e-6, 3)
    for name in variants:
        rec[f"add_{name}_TBps"] = round(nbytes / rec[f"add_{name}_us"] * 1e-6, 3)
        rec[f"add_{name}_over_copy80"] = round(rec[f"add_{name}_us"] / rec["copy80_us"], 3)
    rec["add_this_kernel_us"] = round(rec["add_this_us"] - rec["fixed_us"], 2)
    rec["add_this_kernel_TBps"] = round(nbytes / rec["add_this_kernel_us"] * 1e-6, 3)
    rec["add_this_fraction_of_copy80"] = round(rec["copy80_us"] / rec["add_this_us"], 3)
    new.accum_view(d_accum, copy_dst, w, h, mode="relerr", stream=side)
    side.synchronize()
    del copy_src, copy_dst, imgs

    # ---- (b) host loops on each context's own surfaces and stream
    p = sc.params(width=w, height=h)
    new.accum_reset(d_accum, d_state, w, h)
    torch.cuda.synchronize()
    loops = {"render_parent": render_loop(old, p), "render_this": render_loop(new, p),
             "render_accum": render_loop(new, p, (d_accum, d_state, L.make_accum_desc(w, h)))}
    for name, t in variants.items():                       # the other kernel forms in the loop, where the render evicts between two adds
        if t is not new:
            loops["render_accum_" + name] = render_loop(t, p, (d_accum, d_state, L.make_accum_desc(w, h)))
    times = {k: [] for k in loops}
    for f in loops.values():
        f(20)
    for r in range(args.repeats):
        for k in (list(loops) if r % 2 == 0 else list(loops)[::-1]):
            t0 = time.perf_counter()
            loops[k](args.frames)
            times[k].append((time.perf_counter() - t0) / args.frames * 1e3)
    for k, v in times.items():
        rec[k + "_ms"] = round(statistics.median(v), 4)
        rec[k + "_ms_all"] = [round(x, 4) for x in v]
    rec["render_parent_spread_ms"] = round(max(times["render_parent"]) - min(times["render_parent"]), 4)
    rec["render_this_minus_parent_ms"] = round(rec["render_this_ms"] - rec["render_parent_ms"], 4)
    rec["accum_residual_ms"] = round(rec["render_accum_ms"] - rec["render_this_ms"], 4)
    del d_accum, d_state

    # ---- (c) until done
    if (w, h) == (1920, 1080):
        rec["until_done_c2"] = until_done(new, scenes.make_scene(2, host.generate_aabb), w, h)
        rec["until_done_c3_scene"] = until_done(new, scenes.make_scene(3, host.generate_aabb), w, h)
        new.load(sc)
    print(json.dumps(rec), flush=True)
    records.append(rec)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump({"tool": "tools/bench_accum.py", "scene": "C2", "variants": {k: v for k, v in (s.split("=", 1) for s in args.variant)},
               "records": records}, f, indent=1)
    f.write("\n")
for t in {id(x): x for x in [new, old, *variants.values()]}.values():
    t.close()
