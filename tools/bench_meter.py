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
import argparse, ctypes, json, statistics
import stagebench as sb                                         # (puts the repository on sys.path)
import numpy as np
import torch
from opengl_raytracing_amd import host, scenes
from opengl_raytracing_amd import layout as L

ap = argparse.ArgumentParser()
sb.add_common_args(ap, "meter_bench.json", launches=200)
args = ap.parse_args()
WARM = 20                                                       # launches of each candidate in front of the first timed batch

new, old, _ = sb.open_tracers(args.parent_lib, {})
sc = scenes.make_scene(2, host.generate_aabb)
for t in sb.distinct([new, old]):
    t.load(sc)
side = sb.side()


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
        us = sb.alternate({"meter": lambda img=img: new.meter(img, state, w, h, low_permille=10, high_permille=10, stream=side),
                           "pack": lambda img=img: old.display_pack(img, out8, w, h, format="linear", flip=True, stream=side)},
                          args.launches, args.repeats, WARM)
        sb.summarise(rec, f"meter_{name}", us["meter"], "us")
        sb.summarise(rec, f"yardstick_pack_linear_{name}", us["pack"], "us")
        rec[f"meter_over_pack_{name}"] = round(statistics.median(us["meter"]) / statistics.median(us["pack"]), 3)
    spread = lambda k: sb.spread(rec[k + "_us_all"])
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
        us = sb.alternate(launches, args.launches, args.repeats, WARM)
        for k, v in us.items():
            sb.summarise(rec, f"pack_{fmt}_{k}", v, "us")
        rec[f"pack_{fmt}_this_minus_parent_us"] = round(rec[f"pack_{fmt}_this_us"] - rec[f"pack_{fmt}_parent_us"], 2)
        rec[f"pack_{fmt}_parent_spread_us"] = round(spread(f"pack_{fmt}_parent"), 2)
    del contents, col, out8

    # ---- (c) host loops on each context's own surfaces and stream
    def frame_loop(t, metered):
        lib, ctx = t.lib, t.ctx
        desc = L.make_display_desc(w, h, "srgb", flip=True)
        md = L.make_meter_desc(w, h, adapt=0.25, low_permille=10, high_permille=10)
        tone = L.make_tone_desc("aces", 1.0, exposure)

        def submit(d_color, tk):
            if metered:
                sb.check(t, lib.rt_meter(ctx, d_color, ctypes.byref(md), ctypes.c_void_p(state.data_ptr()), None), "rt_meter")
                sb.check(t, lib.rt_present_submit_toned(ctx, d_color, ctypes.byref(desc), ctypes.byref(tone), None, tk), "rt_present_submit_toned")
            else:
                sb.check(t, lib.rt_present_submit(ctx, d_color, ctypes.byref(desc), None, tk), "rt_present_submit")
        return sb.present_loop(t, p, submit)

    loops = {"render_present_parent": frame_loop(old, False), "render_meter_present_toned": frame_loop(new, True)}
    for k, v in sb.time_host_loops(loops, args.frames, args.repeats).items():
        sb.summarise(rec, k, v, "ms")
    rec["meter_and_tone_residual_ms"] = round(rec["render_meter_present_toned_ms"] - rec["render_present_parent_ms"], 4)
    print(json.dumps(rec), flush=True)
    records.append(rec)

sb.write_records(args.out, "tools/bench_meter.py", records, scene="C2")
sb.close_all([new, old])
