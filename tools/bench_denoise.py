"""Secondary measurement (not the BASELINE metric): what the denoiser costs, at 1920x1080 and 3840x2160, all in one run:

  (a) rt_denoise (prepare + n iterations) for n = 1..5 from device events over back-to-back launches on an accumulator of eight noisy
      frames and a guide of blocks of objects with turning normals; the difference of n and n - 1 iterations is the cost of the step
      2^(n-1).  Beside it, in the same run, a device copy that moves the 48 compulsory bytes per pixel of one iteration (24 read, 24
      written): the ratio to that copy and the achieved compulsory bytes per second.  rt_denoise_guide and a 1 x 1 rt_denoise (the
      launches alone) are timed too.
      --variant NAME=PATH (repeatable) times libraries built with other RT_DENOISE_* macros (tools/build_variants.py) alternately
      with this build's: the kernel forms of DESIGN.md 21.
  (b) host loops on the context's own stream and surfaces: rt_render + rt_accum_add on a library built from the PARENT commit
      (--parent-lib) and on this build, alternating, and rt_render + rt_accum_add + rt_denoise on this build: the frame-loop residual.

Writes one record per size to --out (default profiles/denoise_bench.json)."""
import argparse, ctypes, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from opengl_raytracing_amd import host, scenes
from opengl_raytracing_amd import layout as L

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "denoise_bench.json"))
ap.add_argument("--parent-lib", default=None, help="librt_mi355.so built from the parent commit (build_library(out=...))")
ap.add_argument("--variant", action="append", default=[], help="NAME=PATH of a library built with other RT_DENOISE_* macros")
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--launches", type=int, default=50)
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
        for _ in range(5):
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


def synthetic_hits(w, h):
    """rt_hit records on the device: objects in blocks of 97 x 61 pixels with a band of misses, normals that turn across each block."""
    y, x = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
    obj = ((x // 97) % 5 + 5 * ((y // 61) % 3)).to(torch.int32)
    obj[(y % 200) < 12] = -1
    u, v = (x % 97).float() / 97 - 0.5, (y % 61).float() / 61 - 0.5
    n = torch.stack([u, v, torch.sqrt(1 - u * u - v * v)], dim=-1) * 1.7
    n[obj < 0] = 0
    hits = torch.zeros((h, w, 8), dtype=torch.float32, device="cuda")
    hits[..., 4:7] = n
    hits[..., 7] = obj.view(torch.float32)
    return hits


def loop(t, p, accum=None, denoise=None):
    """n frames of rt_render (+ rt_accum_add with `accum` = (d_accum, d_state, desc)) (+ rt_denoise with `denoise` = (d_guide,
    d_scratch, d_out, desc)) on t's own stream."""
    lib, ctx, d_color, vp = t.lib, t.ctx, ctypes.c_void_p(), ctypes.c_void_p
    check(t, lib.rt_render(ctx, ctypes.byref(p)), "rt_render")
    check(t, lib.rt_get_surfaces(ctx, ctypes.byref(d_color), None, None), "rt_get_surfaces")
    plane = p.regionW * p.regionH * 16

    def run(n):
        for _ in range(n):
            check(t, lib.rt_render(ctx, ctypes.byref(p)), "rt_render")
            if accum:
                check(t, lib.rt_accum_add(ctx, d_color, vp(accum[0].data_ptr()), ctypes.byref(accum[2]), vp(accum[1].data_ptr()), None), "rt_accum_add")
            if denoise:
                check(t, lib.rt_denoise(ctx, vp(accum[0].data_ptr()), vp(accum[0].data_ptr() + plane), vp(denoise[0].data_ptr()),
                                        vp(denoise[1].data_ptr()), vp(denoise[2].data_ptr()), ctypes.byref(denoise[3]), None), "rt_denoise")
        t.sync()
    return run


records = []
for (w, h) in [(1920, 1080), (3840, 2160)]:
    rec = {"size": [w, h], "frames": args.frames, "repeats": args.repeats, "launches": args.launches,
           "parent": "parent build" if args.parent_lib else "this build"}
    gen = torch.Generator(device="cuda").manual_seed(w)
    base = torch.rand((h, w, 4), device="cuda", generator=gen) ** 4 * 8
    d_accum, d_state = new.accum_alloc(w, h)
    for _ in range(8):
        new.accum_add(base * torch.exp(0.5 * torch.randn((h, w, 4), device="cuda", generator=gen) - 0.125), d_accum, d_state, w, h)
    d_hits = synthetic_hits(w, h)
    d_guide = new.denoise_guide(d_hits, w, h)
    d_scratch, d_out = new.denoise_alloc(w, h)
    tiny = [torch.zeros(64, dtype=torch.uint8, device="cuda") for _ in range(5)]
    copy_src = torch.zeros(w * h * 24, dtype=torch.uint8, device="cuda")
    copy_dst = torch.empty_like(copy_src)
    mean, moments = new.accum_mean(d_accum, w, h), new.accum_moments(d_accum, w, h)
    torch.cuda.synchronize()

    # ---- (a) the filter beside a copy of one iteration's compulsory bytes; the kernel forms beside each other
    launches = {"copy48": lambda: copy_dst.copy_(copy_src),
                "guide": lambda: new.denoise_guide(d_hits, w, h, out=d_guide, stream=side),
                "fixed4": lambda: new.denoise(tiny[0], tiny[1], tiny[2], tiny[3], tiny[4], 1, 1, stream=side)}
    for name, t in variants.items():
        for n in range(1, 6):
            launches[f"denoise{n}_{name}"] = lambda t=t, n=n: t.denoise(mean, moments, d_guide, d_scratch, d_out, w, h, iterations=n, stream=side)
    with torch.cuda.stream(side):
        us = alternate(launches, args.launches, args.repeats)
    for k, v in us.items():
        put(rec, k, v)
    nbytes = w * h * 48
    rec["copy48_TBps"] = round(nbytes / rec["copy48_us"] * 1e-6, 3)
    for name in variants:
        t = [rec[f"denoise{n}_{name}_us"] for n in range(1, 6)]
        rec[f"steps_{name}_us"] = {"prepare+step1": t[0], **{f"step{1 << n}": round(t[n] - t[n - 1], 2) for n in range(1, 5)}}
        rec[f"denoise4_{name}_per_iteration_us"] = round(t[3] / 4, 2)
        rec[f"denoise4_{name}_over_copy48_per_iteration"] = round(t[3] / 4 / rec["copy48_us"], 3)
        rec[f"denoise4_{name}_TBps"] = round((4 * nbytes + w * h * 64) / t[3] * 1e-6, 3)       # + prepare: 48 read, 16 written
    out_this = d_out.clone()
    for name, t in variants.items():                          # faster and different is not faster: every form gives the same bytes
        t.denoise(mean, moments, d_guide, d_scratch, d_out, w, h, iterations=5, stream=side)
        side.synchronize()
        if name == "this":
            out_this = d_out.clone()
        rec[f"denoise5_{name}_same_bytes_as_this"] = bool(torch.equal(d_out.view(torch.int32), out_this.view(torch.int32)))
    del copy_src, copy_dst

    # ---- (b) host loops on each context's own surfaces and stream
    p = sc.params(width=w, height=h)
    new.accum_reset(d_accum, d_state, w, h)
    torch.cuda.synchronize()
    adesc, ddesc = L.make_accum_desc(w, h), L.make_denoise_desc(w, h)
    loops = {"render_accum_parent": loop(old, p, (d_accum, d_state, adesc)), "render_accum_this": loop(new, p, (d_accum, d_state, adesc)),
             "render_accum_denoise": loop(new, p, (d_accum, d_state, adesc), (d_guide, d_scratch, d_out, ddesc))}
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
    rec["render_accum_parent_spread_ms"] = round(max(times["render_accum_parent"]) - min(times["render_accum_parent"]), 4)
    rec["render_accum_this_minus_parent_ms"] = round(rec["render_accum_this_ms"] - rec["render_accum_parent_ms"], 4)
    rec["denoise_residual_ms"] = round(rec["render_accum_denoise_ms"] - rec["render_accum_this_ms"], 4)
    del d_accum, d_state, d_guide, d_scratch, d_out, d_hits, mean, moments, out_this, base
    print(json.dumps(rec), flush=True)
    records.append(rec)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump({"tool": "tools/bench_denoise.py", "scene": "C2", "variants": {k: v for k, v in (s.split("=", 1) for s in args.variant)},
               "records": records}, f, indent=1)
    f.write("\n")
for t in {id(x): x for x in [new, old, *variants.values()]}.values():
    t.close()
