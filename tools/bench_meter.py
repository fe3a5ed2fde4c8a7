"""Secondary measurement (not the BASELINE metric): what exposure metering and tone mapping cost, at 1920x1080 and 3840x2160, all in
one run, against a library built from the PARENT commit (--parent-lib; without it the yardstick is this build's own untoned pack):

  (a) rt_meter (clear + histogram + solve) from device events over back-to-back launches, on three contents -- a rendered C2 frame,
      uniform noise, one constant colour -- beside the yardstick rt_display_pack (linear) of the parent, which reads the same 16 B per
      pixel; ratio per content.  Repeated launches over one surface are served by the Infinity Cache (256 MiB holds a 4K rgba32f
      frame twice over): these are cache-resident figures, as DESIGN.md 14's are.
  (b) the old entry points (rt_display_pack linear / sRGB) on the parent's build and on this one, alternating, and the toned variants
      (Reinhard, ACES, with a device-resident exposure) beside them;
  (c) host loops: rt_render + rt_present_submit on the parent against rt_render + rt_meter + rt_present_submit_toned on this build,
      waiting for the previous ticket in every iteration.

Writes one record per size to --out (default profiles/meter_bench.json)."""
import argparse, ctypes, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from opengl_raytracing_amd import host, scenes
from opengl_raytracing_amd import layout as L

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "meter_bench.json"))
ap.add_argument("--parent-lib", default=None, help="librt_mi355.so built from the parent commit (build_library(out=...))")
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--launches", type=int, default=200)
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
sc = scenes.make_scene(2, host.generate_aabb)
for t in {id(new): new, id(old): old}.values():
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
        for _ in range(20):
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


records = []
for (w, h) in [(1920, 1080), (3840, 2160)]:
    p = sc.params(width=w, height=h)
    rec = {"size": [w, h], "frames": args.frames, "repeats": args.repeats, "launches": args.launches,
           "yardstick": "parent" if args.parent_lib else "this build"}
    rng = np.random.default_rng(w)
    col = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    pos = torch.empty_like(col)
    nrm = torch.empty((h, w, 4), dtype=torch.float16, device="cuda")
    new.render_to(p, col.data_ptr(), pos.data_ptr(), nrm.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    contents = {"rendered": col,
                "noise": torch.from_numpy((rng.uniform(0, 1, (h, w, 4)) ** 4 * 8).astype(np.float32)).cuda(),
                "constant": torch.full((h, w, 4), 0.5, dtype=torch.float32, device="cuda")}
    del pos, nrm
    out8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    state = torch.zeros(1088, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    # ---- (a) the meter on three contents beside the parent's linear pack of the same surface
    for name, img in contents.items():
        us = alternate({"meter": lambda img=img: new.meter(img, state, w, h, low_permille=10, high_permille=10, stream=side),
                        "pack": lambda img=img: old.display_pack(img, out8, w, h, format="linear", flip=True, stream=side)},
                       args.launches, args.repeats)
        put(rec, f"meter_{name}", us["meter"])
        put(rec, f"yardstick_pack_linear_{name}", us["pack"])
        rec[f"meter_over_pack_{name}"] = round(statistics.median(us["meter"]) / statistics.median(us["pack"]), 3)
    spread = lambda k: max(rec[k + "_us_all"]) - min(rec[k + "_us_all"])
    rec["meter_constant_minus_noise_us"] = round(rec["meter_constant_us"] - rec["meter_noise_us"], 2)
    rec["meter_repeat_spread_us"] = round(max(spread("meter_constant"), spread("meter_noise")), 2)

    # ---- (b) the old entry points on both builds, alternating; the toned variants beside them
    exposure = state[L.METER_EXPOSURE_OFFSET:].data_ptr()
    for fmt in ("linear", "srgb"):
        launches = {"parent": lambda: old.display_pack(col, out8, w, h, format=fmt, flip=True, stream=side),
                    "this": lambda: new.display_pack(col, out8, w, h, format=fmt, flip=True, stream=side),
                    "none_dev": lambda: new.display_pack(col, out8, w, h, format=fmt, flip=True, stream=side, d_exposure=exposure),
                    "reinhard": lambda: new.display_pack(col, out8, w, h, format=fmt, flip=True, stream=side, tone="reinhard", white=4.0),
                    "aces": lambda: new.display_pack(col, out8, w, h, format=fmt, flip=True, stream=side, tone="aces"),
                    "aces_dev": lambda: new.display_pack(col, out8, w, h, format=fmt, flip=True, stream=side, tone="aces", d_exposure=exposure)}
        us = alternate(launches, args.launches, args.repeats)
        for k, v in us.items():
            put(rec, f"pack_{fmt}_{k}", v)
        rec[f"pack_{fmt}_this_minus_parent_us"] = round(rec[f"pack_{fmt}_this_us"] - rec[f"pack_{fmt}_parent_us"], 2)
        rec[f"pack_{fmt}_parent_spread_us"] = round(spread(f"pack_{fmt}_parent"), 2)
    del contents, col, out8

    # ---- (c) host loops on each context's own surfaces and stream
    def frame_loop(t, metered):
        lib, ctx = t.lib, t.ctx
        d_color = ctypes.c_void_p()
        desc = L.make_display_desc(w, h, "srgb", flip=True)
        md = L.make_meter_desc(w, h, adapt=0.25, low_permille=10, high_permille=10)
        tone = L.make_tone_desc("aces", 1.0, exposure)

        def check(rc, what):
            if rc:
                raise host.RtError(rc, f"{what}: {lib.rt_last_error(ctx).decode()}")

        check(lib.rt_render(ctx, ctypes.byref(p)), "rt_render")
        check(lib.rt_get_surfaces(ctx, ctypes.byref(d_color), None, None), "rt_get_surfaces")

        def loop(n):
            px, nb, tk = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_uint64()
            prev = None
            for _ in range(n):
                check(lib.rt_render(ctx, ctypes.byref(p)), "rt_render")
                if metered:
                    check(lib.rt_meter(ctx, d_color, ctypes.byref(md), ctypes.c_void_p(state.data_ptr()), None), "rt_meter")
                    check(lib.rt_present_submit_toned(ctx, d_color, ctypes.byref(desc), ctypes.byref(tone), None, ctypes.byref(tk)), "rt_present_submit_toned")
                else:
                    check(lib.rt_present_submit(ctx, d_color, ctypes.byref(desc), None, ctypes.byref(tk)), "rt_present_submit")
                if prev is not None:
                    check(lib.rt_present_wait(ctx, prev, ctypes.byref(px), ctypes.byref(nb)), "rt_present_wait")
                prev = tk.value
            check(lib.rt_present_wait(ctx, prev, ctypes.byref(px), ctypes.byref(nb)), "rt_present_wait")
            t.sync()
        return loop

    loops = {"render_present_parent": frame_loop(old, False), "render_meter_present_toned": frame_loop(new, True)}
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
    rec["meter_and_tone_residual_ms"] = round(rec["render_meter_present_toned_ms"] - rec["render_present_parent_ms"], 4)
    print(json.dumps(rec), flush=True)
    records.append(rec)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump({"tool": "tools/bench_meter.py", "scene": "C2", "records": records}, f, indent=1)
    f.write("\n")
for t in {id(new): new, id(old): old}.values():
    t.close()
