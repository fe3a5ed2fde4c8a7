"""Secondary measurement (not the BASELINE metric): what rt_display_resample costs, all in one run.

  (a) the kernel from device events over back-to-back launches, for 3840x2160 -> 1920x1080, 1920x1080 -> 3840x2160 and
      1920x1080 -> 1920x1080 with all three filters, beside a device-to-device copy (torch's copy_ of a contiguous float32
      tensor) that moves the same compulsory bytes -- the source read once plus the destination written once, so the copy is of
      half their sum -- timed alternately in the same run; each figure also as a multiple of that copy.  Both rotate over enough
      source buffers (--rotate-mib in all, default 640) that no launch finds its source in the 256 MiB Infinity Cache; with
      --rotate-mib 0 one source is reused and the figures are cache-resident ones.
  (b) --variant-lib: the same launches through another build of the library (e.g. -DRT_RESAMPLE_XCD=1), alternating with this one.
  (c) host loops on the context's own surfaces and stream, waiting for the previous ticket in every iteration:
      rt_render at 4K alone (--parent-lib: through the parent's build, else this one), and rt_render at 4K +
      rt_display_resample to 1080p + rt_present_submit at 1080p; the difference is the residual cost of delivering a
      supersampled 1080p frame.

Writes --out (default profiles/resample_bench.json)."""
import argparse, ctypes, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from opengl_raytracing_amd import host, scenes
from opengl_raytracing_amd import layout as L

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "resample_bench.json"))
ap.add_argument("--parent-lib", default=None, help="librt_mi355.so built from the parent commit (build_library(out=...))")
ap.add_argument("--variant-lib", default=None, help="another build of this library to time beside it")
ap.add_argument("--variant-name", default="variant")
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--launches", type=int, default=100)
ap.add_argument("--rotate-mib", type=int, default=640)
ap.add_argument("--note", default=None, help="free text stored with the records")
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
variant = tracer(args.variant_lib) if args.variant_lib else None
old = tracer(args.parent_lib) if args.parent_lib else new
side = torch.cuda.Stream()
blocker_a = torch.zeros(256 << 20, dtype=torch.uint8, device="cuda")
blocker_b = torch.empty_like(blocker_a)


def hold(stream):
    """Keep `stream` busy for a few milliseconds so that the launches timed behind it are all queued before the first one starts."""
    with torch.cuda.stream(stream):
        for _ in range(40):
            blocker_b.copy_(blocker_a)


def device_us(launch, K):
    """Microseconds per call of launch(k) from device events around K back-to-back calls on `side`."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    hold(side)
    e0.record(side)
    for k in range(K):
        launch(k)
    e1.record(side)
    side.synchronize()
    return e0.elapsed_time(e1) / K * 1e3


def alternate(launches, K, repeats):
    """launches: {name: callable(k)}; every repeat times each once, in alternating order -> {name: [us per repeat]}."""
    for f in launches.values():
        for k in range(20):
            f(k)
    side.synchronize()
    us = {k: [] for k in launches}
    for r in range(repeats):
        for k in (list(launches) if r % 2 == 0 else list(launches)[::-1]):
            us[k].append(device_us(launches[k], K))
    return us


records = []
gen = torch.Generator(device="cuda").manual_seed(1)
for (sw, sh), (dw, dh) in [((3840, 2160), (1920, 1080)), ((1920, 1080), (3840, 2160)), ((1920, 1080), (1920, 1080))]:
    src_bytes, dst_bytes = sw * sh * 16, dw * dh * 16
    n_src = max(1, -(-(args.rotate_mib << 20) // src_bytes)) if args.rotate_mib else 1
    srcs = [torch.rand((sh, sw, 4), dtype=torch.float32, device="cuda", generator=gen) for _ in range(n_src)]
    dst = torch.empty((dh, dw, 4), dtype=torch.float32, device="cuda")
    copy_floats = (src_bytes + dst_bytes) // 8                  # half the compulsory bytes in, the same out
    n_copy = max(1, -(-(args.rotate_mib << 20) // (copy_floats * 4))) if args.rotate_mib else 1
    copy_src = [torch.rand((copy_floats,), dtype=torch.float32, device="cuda", generator=gen) for _ in range(n_copy)]
    copy_dst = torch.empty((copy_floats,), dtype=torch.float32, device="cuda")
    rec = {"src": [sw, sh], "dst": [dw, dh], "compulsory_bytes": src_bytes + dst_bytes, "launches": args.launches, "repeats": args.repeats,
           "source_buffers": n_src, "copy_source_buffers": n_copy, "rotate_mib": args.rotate_mib}

    def copy(k):
        with torch.cuda.stream(side):
            copy_dst.copy_(copy_src[k % n_copy])

    launches = {"copy": copy}
    for f in ("area", "triangle", "lanczos3"):
        launches[f] = (lambda f: lambda k: new.resample(srcs[k % n_src], dst, sw, sh, dw, dh, filter=f, stream=side))(f)
        if variant is not None:
            launches[f"{f}_{args.variant_name}"] = (lambda f: lambda k: variant.resample(srcs[k % n_src], dst, sw, sh, dw, dh, filter=f, stream=side))(f)
    us = alternate(launches, args.launches, args.repeats)
    for k, v in us.items():
        rec[k + "_us"] = round(statistics.median(v), 2)
        rec[k + "_us_all"] = [round(x, 2) for x in v]
    for k in us:
        if k != "copy":
            rec[k + "_over_copy"] = round(rec[k + "_us"] / rec["copy_us"], 3)
    rec["copy_GBps"] = round((src_bytes + dst_bytes) / rec["copy_us"] / 1e3, 1)
    for f in ("area", "triangle", "lanczos3"):
        rec[f + "_taps"] = [host.resample_taps(sw, dw, f)[0], host.resample_taps(sh, dh, f)[0]]
    print(json.dumps(rec), flush=True)
    records.append(rec)
    del srcs, dst, copy_src, copy_dst

# ---- (c) the 1080p frame loop off a 4K render
sc = scenes.make_scene(2, host.generate_aabb)
for t in {id(new): new, id(old): old}.values():
    t.load(sc)
W4, H4, W2, H2 = 3840, 2160, 1920, 1080
p4 = sc.params(width=W4, height=H4)
d_small = torch.empty((H2, W2, 4), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()


def frame_loop(t, kind, filter):
    lib, ctx = t.lib, t.ctx
    d_color = ctypes.c_void_p()
    desc = L.make_display_desc(W2, H2, "srgb", flip=True)
    rdesc = L.make_resample_desc(W4, H4, W2, H2, filter)
    small = ctypes.c_void_p(d_small.data_ptr())

    def check(rc, what):
        if rc:
            raise host.RtError(rc, f"{what}: {lib.rt_last_error(ctx).decode()}")

    check(lib.rt_render(ctx, ctypes.byref(p4)), "rt_render")
    check(lib.rt_get_surfaces(ctx, ctypes.byref(d_color), None, None), "rt_get_surfaces")

    def loop(n):
        px, nb, tk = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_uint64()
        prev = None
        for _ in range(n):
            check(lib.rt_render(ctx, ctypes.byref(p4)), "rt_render")
            if kind == "render":
                continue
            check(lib.rt_display_resample(ctx, d_color, small, ctypes.byref(rdesc), None), "rt_display_resample")
            check(lib.rt_present_submit(ctx, small, ctypes.byref(desc), None, ctypes.byref(tk)), "rt_present_submit")
            if prev is not None:
                check(lib.rt_present_wait(ctx, prev, ctypes.byref(px), ctypes.byref(nb)), "rt_present_wait")
            prev = tk.value
        if prev is not None:
            check(lib.rt_present_wait(ctx, prev, ctypes.byref(px), ctypes.byref(nb)), "rt_present_wait")
        t.sync()
    return loop


loops = {"render4k_only_parent": frame_loop(old, "render", "area"), "render4k_only": frame_loop(new, "render", "area")}
for f in ("area", "triangle", "lanczos3"):
    loops[f"render4k_resample_{f}_present1080"] = frame_loop(new, "deliver", f)
times = {k: [] for k in loops}
for f in loops.values():
    f(20)
for r in range(args.repeats):
    for k in (list(loops) if r % 2 == 0 else list(loops)[::-1]):
        t0 = time.perf_counter()
        loops[k](args.frames)
        times[k].append((time.perf_counter() - t0) / args.frames * 1e3)
loop_rec = {"scene": "C2", "render": [W4, H4], "deliver": [W2, H2], "frames": args.frames, "repeats": args.repeats,
            "yardstick": "parent" if args.parent_lib else "this build"}
for k, v in times.items():
    loop_rec[k + "_ms"] = round(statistics.median(v), 4)
    loop_rec[k + "_ms_all"] = [round(x, 4) for x in v]
for f in ("area", "triangle", "lanczos3"):
    loop_rec[f"residual_{f}_ms"] = round(loop_rec[f"render4k_resample_{f}_present1080_ms"] - loop_rec["render4k_only_parent_ms"], 4)
print(json.dumps(loop_rec), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump({"tool": "tools/bench_resample.py", "note": args.note, "records": records, "frame_loop": loop_rec}, f, indent=1)
    f.write("\n")
for t in {id(x): x for x in (new, old, variant) if x is not None}.values():
    t.close()
