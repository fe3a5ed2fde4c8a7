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
import argparse, ctypes, json
import stagebench as sb                                         # (puts the repository on sys.path)
import torch
from opengl_raytracing_amd import host, scenes
from opengl_raytracing_amd import layout as L

ap = argparse.ArgumentParser()
sb.add_common_args(ap, "yuv_bench.json", launches=200)
ap.add_argument("--note", default=None, help="free text stored with the records (e.g. the build variant measured)")
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
        us = sb.alternate(launches, args.launches, args.repeats, WARM)
        for k, v in us.items():
            sb.summarise(rec, f"pack_{transfer}_{k}", v, "us")
        for k in ("nv12", "i420"):
            rec[f"pack_{transfer}_{k}_over_rgba8_parent"] = round(rec[f"pack_{transfer}_{k}_us"] / rec[f"pack_{transfer}_rgba8_parent_us"], 3)
        rec[f"pack_{transfer}_rgba8_this_minus_parent_us"] = round(rec[f"pack_{transfer}_rgba8_this_us"] - rec[f"pack_{transfer}_rgba8_parent_us"], 2)
    del col, out8, outyuv

    # ---- (b) host loops on each context's own surfaces and stream
    def frame_loop(t, kind):
        lib, ctx = t.lib, t.ctx
        desc = L.make_display_desc(w, h, "srgb", flip=True)
        ydesc = L.make_yuv_desc(w, h, "nv12", flip=True)

        def submit(d_color, tk):
            if kind == "yuv":
                sb.check(t, lib.rt_present_submit_yuv(ctx, d_color, ctypes.byref(ydesc), None, None, tk), "rt_present_submit_yuv")
            else:
                sb.check(t, lib.rt_present_submit(ctx, d_color, ctypes.byref(desc), None, tk), "rt_present_submit")
        return sb.present_loop(t, p, submit)

    loops = {"render_only": sb.render_loop(new, p), "render_present_rgba8_parent": frame_loop(old, "rgba8"),
             "render_present_yuv": frame_loop(new, "yuv")}
    for k, v in sb.time_host_loops(loops, args.frames, args.repeats).items():
        sb.summarise(rec, k, v, "ms")
    rec["yuv_delivery_residual_ms"] = round(rec["render_present_yuv_ms"] - rec["render_only_ms"], 4)
    rec["rgba8_delivery_residual_ms"] = round(rec["render_present_rgba8_parent_ms"] - rec["render_only_ms"], 4)
    print(json.dumps(rec), flush=True)
    records.append(rec)

sb.write_records(args.out, "tools/bench_yuv.py", records, scene="C2", note=args.note)
sb.close_all([new, old])
