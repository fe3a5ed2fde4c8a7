"""Secondary measurement (not the BASELINE metric): what it costs to get a rendered frame to the host, at 1920x1080 and 3840x2160
on the bench scene, all in one run:

  (a) rt_display_pack alone, both formats, from device events (20 B of compulsory HBM traffic per pixel: 16 read, 4 written);
  (b) a loop of rt_render + rt_readback(gColor only): the path before rt_present_*, the baseline;
  (c) the same loop with rt_render alone;
  (d) rt_render + rt_present_submit, waiting for the PREVIOUS ticket in every iteration.

(b), (c) and (d) are host wall-clock times per frame over a loop that ends with everything complete; (d) - (c) is the residual cost
of delivery, (b) - (c) what it replaces.  Writes one record per size to --out (default profiles/present_bench.json)."""
import argparse, ctypes, json, statistics
import stagebench as sb                                         # (puts the repository on sys.path)
import numpy as np
import torch
from opengl_raytracing_amd import host, scenes
from opengl_raytracing_amd import layout as L

ap = argparse.ArgumentParser()
sb.add_common_args(ap, "present_bench.json", parent_lib=False)
args = ap.parse_args()
K, WARM = 200, 20                                               # launches per timed batch; of each format in front of the first batch

HBM_PEAK = 8.0e12
rt = host.RayTracer(0)
lib, ctx = rt.lib, rt.ctx
sc = scenes.make_scene(2, host.generate_aabb)
rt.load(sc)
side = sb.side()
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
    launches = {fmt: lambda fmt=fmt: rt.display_pack(col, out8, w, h, format=fmt, flip=True, stream=side) for fmt in ("linear", "srgb")}
    for fmt, us in sb.alternate(launches, K, args.repeats, WARM).items():
        sb.summarise(rec, f"pack_{fmt}", us, "us")
        rec[f"pack_{fmt}_hbm_frac"] = round(npx * 20 / (statistics.median(us) * 1e-6) / HBM_PEAK, 3)
    del col, pos, nrm, out8

    # ---- (b), (c), (d): host loops on the context's own surfaces and stream
    h_color = np.empty((h, w, 4), dtype=np.float32)
    desc = L.make_display_desc(w, h, "srgb", flip=True)

    def readback(d_color, k):                                   # returns with the frame on the host: the loop's sync finds an idle stream
        sb.check(rt, lib.rt_readback(ctx, h_color.ctypes.data_as(ctypes.c_void_p), None, None), "rt_readback")

    def submit(d_color, tk):
        sb.check(rt, lib.rt_present_submit(ctx, d_color, ctypes.byref(desc), None, tk), "rt_present_submit")

    loops = {"render_readback_color": sb.render_loop(rt, p, [readback]), "render": sb.render_loop(rt, p),
             "render_present": sb.present_loop(rt, p, submit)}
    for k, v in sb.time_host_loops(loops, args.frames, args.repeats).items():
        sb.summarise(rec, k, v, "ms")
    rec["delivery_residual_ms"] = round(rec["render_present_ms"] - rec["render_ms"], 4)
    rec["readback_cost_ms"] = round(rec["render_readback_color_ms"] - rec["render_ms"], 4)
    rec["taa_resolve_hbm_frac_for_scale"] = [0.49, 0.55]
    print(json.dumps(rec), flush=True)
    records.append(rec)

sb.write_records(args.out, "tools/bench_present.py", records, scene="C2", hbm_peak_Bps=HBM_PEAK)
rt.close()
