"""Secondary measurement (not the BASELINE metric): what the YUV 4:2:0 output costs, at 1920x1080 and 3840x2160, all in one run,
against a library built from the PARENT commit (--parent-lib; without it the yardstick is this build's own RGBA8 pack):

  (a) rt_display_pack_yuv (NV12 and I420, sRGB and linear transfer, and NV12 behind ACES with a device-resident exposure) from device
      events over back-to-back launches on a rendered C2 frame, beside the yardstick rt_display_pack of the same transfer on the
      same surface (parent's build and this one), timed alternately; ratio to the parent's pack per variant.  Repeated launches
      over one surface are served by the Infinity Cache (256 MiB holds a 4K rgba32f frame twice over): these are cache-resident
      figures, as DESIGN.md 14's are.
  (b) host loops on the context's own surfaces and stream, waiting for the previous ticket in every iteration:
      rt_render alone, rt_render + rt_present_submit (parent's build), rt_render + rt_present_submit_yuv.

Writes one record per size to --out (default profiles/yuv_bench.json)."""
import argparse, ctypes, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from opengl_raytracing_amd import host, scenes
from opengl_raytracing_amd import layout as L

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "yuv_bench.json"))
ap.add_argument("--parent-lib", default=None, help="librt_mi355.so built from the parent commit (build_library(out=...))")
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--note", default=None, help="free text stored with the records (e.g. the build variant measured)")
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
    col = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    pos = torch.empty_like(col)
    nrm = torch.empty((h, w, 4), dtype=torch.float16, device="cuda")
    new.render_to(p, col.data_ptr(), pos.data_ptr(), nrm.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    del pos, nrm
    out8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    outyuv = torch.empty((host.yuv_layout(w, h).bytes,), dtype=torch.uint8, device="cuda")
    state = torch.zeros(1088, dtype=torch.uint8, device="cuda")
    new.meter(col, state, w, h, low_permille=10, high_permille=10, stream=side)
    side.synchronize()
    exposure = state[L.METER_EXPOSURE_OFFSET:].data_ptr()

    # ---- (a) the YUV pack beside the RGBA8 pack of the same transfer on the same surface
    for transfer in ("srgb", "linear"):
        yuv = lambda fmt, **kw: (lambda: new.display_pack_yuv(col, outyuv, w, h, format=fmt, transfer=transfer, flip=True, stream=side, **kw))
        launches = {"rgba8_parent": lambda: old.display_pack(col, out8, w, h, format=transfer, flip=True, stream=side),
                    "rgba8_this": lambda: new.display_pack(col, out8, w, h, format=transfer, flip=True, stream=side),
                    "nv12": yuv("nv12"), "i420": yuv("i420"), "nv12_aces_dev": yuv("nv12", tone="aces", d_exposure=exposure)}
        us = alternate(launches, args.launches, args.repeats)
        for k, v in us.items():
            put(rec, f"pack_{transfer}_{k}", v)
        for k in ("nv12", "i420"):
            rec[f"pack_{transfer}_{k}_over_rgba8_parent"] = round(rec[f"pack_{transfer}_{k}_us"] / rec[f"pack_{transfer}_rgba8_parent_us"], 3)
        rec[f"pack_{transfer}_rgba8_this_minus_parent_us"] = round(rec[f"pack_{transfer}_rgba8_this_us"] - rec[f"pack_{transfer}_rgba8_parent_us"], 2)
    del col, out8, outyuv

    # ---- (b) host loops on each context's own surfaces and stream
    def frame_loop(t, kind):
        lib, ctx = t.lib, t.ctx
        d_color = ctypes.c_void_p()
        desc = L.make_display_desc(w, h, "srgb", flip=True)
        ydesc = L.make_yuv_desc(w, h, "nv12", flip=True)

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
                if kind == "render":
                    continue
                if kind == "yuv":
                    check(lib.rt_present_submit_yuv(ctx, d_color, ctypes.byref(ydesc), None, None, ctypes.byref(tk)), "rt_present_submit_yuv")
                else:
                    check(lib.rt_present_submit(ctx, d_color, ctypes.byref(desc), None, ctypes.byref(tk)), "rt_present_submit")
                if prev is not None:
                    check(lib.rt_present_wait(ctx, prev, ctypes.byref(px), ctypes.byref(nb)), "rt_present_wait")
                prev = tk.value
            if prev is not None:
                check(lib.rt_present_wait(ctx, prev, ctypes.byref(px), ctypes.byref(nb)), "rt_present_wait")
            t.sync()
        return loop

    loops = {"render_only": frame_loop(new, "render"), "render_present_rgba8_parent": frame_loop(old, "rgba8"),
             "render_present_yuv": frame_loop(new, "yuv")}
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
    rec["yuv_delivery_residual_ms"] = round(rec["render_present_yuv_ms"] - rec["render_only_ms"], 4)
    rec["rgba8_delivery_residual_ms"] = round(rec["render_present_rgba8_parent_ms"] - rec["render_only_ms"], 4)
    print(json.dumps(rec), flush=True)
    records.append(rec)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump({"tool": "tools/bench_yuv.py", "scene": "C2", "note": args.note, "records": records}, f, indent=1)
    f.write("\n")
for t in {id(new): new, id(old): old}.values():
    t.close()
