"""Secondary measurement (not the BASELINE metric): what it costs to get a rendered frame to the host, at 1920x1080 and 3840x2160
on the bench scene, all in one run:

  (a) rt_display_pack alone, both formats, from device events (20 B of compulsory HBM traffic per pixel: 16 read, 4 written);
  (b) a loop of rt_render + rt_readback(gColor only): the path before rt_present_*, the baseline;
  (c) the same loop with rt_render alone;
  (d) rt_render + rt_present_submit, waiting for the PREVIOUS ticket in every iteration.

(b), (c) and (d) are host wall-clock times per frame over a loop that ends with everything complete; (d) - (c) is the residual cost
of delivery, (b) - (c) what it replaces.  Writes one record per size to --out (default profiles/present_bench.json)."""
import argparse, ctypes, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from opengl_raytracing_amd import host, scenes
from opengl_raytracing_amd import layout as L

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "present_bench.json"))
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()

HBM_PEAK = 8.0e12
rt = host.RayTracer(0)
lib, ctx = rt.lib, rt.ctx
sc = scenes.make_scene(2, host.generate_aabb)
rt.load(sc)
side = torch.cuda.Stream()


def check(rc, what):
    if rc:
        raise host.RtError(rc, f"{what}: {lib.rt_last_error(ctx).decode()}")


def hold(stream):
    """Keep `stream` busy for a few milliseconds so that the launches timed behind it are all queued before the first one starts:
    the pack runs for microseconds, less than a launch takes to enqueue."""
    with torch.cuda.stream(stream):
        for _ in range(40):
            blocker_b.copy_(blocker_a)


blocker_a = torch.zeros(256 << 20, dtype=torch.uint8, device="cuda")
blocker_b = torch.empty_like(blocker_a)
records = []
for (w, h) in [(1920, 1080), (3840, 2160)]:
    p = sc.params(width=w, height=h)
    npx = w * h
    rec = {"size": [w, h], "frames": args.frames, "repeats": args.repeats}

    # ---- (a) the pack kernel alone, on a surface the ray tracer produced
    col = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    pos = torch.empty_like(col)
    nrm = torch.empty((h, w, 4), dtype=torch.float16, device="cuda")
    out8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    rt.render_to(p, col.data_ptr(), pos.data_ptr(), nrm.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    for fmt in ("linear", "srgb"):
        for _ in range(20):
            rt.display_pack(col, out8, w, h, format=fmt, flip=True, stream=side)
        side.synchronize()
        K, us = 200, []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            hold(side)
            e0.record(side)
            for _ in range(K):
                rt.display_pack(col, out8, w, h, format=fmt, flip=True, stream=side)
            e1.record(side)
            side.synchronize()
            us.append(e0.elapsed_time(e1) / K * 1e3)
        med = statistics.median(us)
        rec[f"pack_{fmt}_us"] = round(med, 2)
        rec[f"pack_{fmt}_us_all"] = [round(x, 2) for x in us]
        rec[f"pack_{fmt}_hbm_frac"] = round(npx * 20 / (med * 1e-6) / HBM_PEAK, 3)
    del col, pos, nrm, out8

    # ---- (b), (c), (d): host loops on the context's own surfaces and stream
    h_color = np.empty((h, w, 4), dtype=np.float32)
    desc = L.make_display_desc(w, h, "srgb", flip=True)
    d_color = ctypes.c_void_p()

    def render():
        check(lib.rt_render(ctx, ctypes.byref(p)), "rt_render")

    def loop_readback(n):
        for _ in range(n):
            render()
            check(lib.rt_readback(ctx, h_color.ctypes.data_as(ctypes.c_void_p), None, None), "rt_readback")

    def loop_render(n):
        for _ in range(n):
            render()
        rt.sync()

    def loop_present(n):
        px, nb, t = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_uint64()
        prev = None
        for _ in range(n):
            render()
            check(lib.rt_present_submit(ctx, d_color, ctypes.byref(desc), None, ctypes.byref(t)), "rt_present_submit")
            if prev is not None:
                check(lib.rt_present_wait(ctx, prev, ctypes.byref(px), ctypes.byref(nb)), "rt_present_wait")
            prev = t.value
        check(lib.rt_present_wait(ctx, prev, ctypes.byref(px), ctypes.byref(nb)), "rt_present_wait")
        rt.sync()

    render()
    check(lib.rt_get_surfaces(ctx, ctypes.byref(d_color), None, None), "rt_get_surfaces")
    loops = {"render_readback_color": loop_readback, "render": loop_render, "render_present": loop_present}
    times = {k: [] for k in loops}
    for f in loops.values():
        f(20)
    for r in range(args.repeats):
        order = list(loops) if r % 2 == 0 else list(loops)[::-1]
        for k in order:
            t0 = time.perf_counter()
            loops[k](args.frames)
            times[k].append((time.perf_counter() - t0) / args.frames * 1e3)
    for k, v in times.items():
        rec[k + "_ms"] = round(statistics.median(v), 4)
        rec[k + "_ms_all"] = [round(x, 4) for x in v]
    rec["delivery_residual_ms"] = round(rec["render_present_ms"] - rec["render_ms"], 4)
    rec["readback_cost_ms"] = round(rec["render_readback_color_ms"] - rec["render_ms"], 4)
    rec["taa_resolve_hbm_frac_for_scale"] = [0.49, 0.55]
    print(json.dumps(rec), flush=True)
    records.append(rec)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump({"tool": "tools/bench_present.py", "scene": "C2", "hbm_peak_Bps": HBM_PEAK, "records": records}, f, indent=1)
    f.write("\n")
rt.close()
