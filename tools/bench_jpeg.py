"""Secondary measurement (not the BASELINE metric): what the baseline JPEG output costs, at 1920x1080 and 3840x2160, quality 50 and
90, restart interval 1, 8 (the Python default) and one MCU row, on a rendered C2 frame and on uniform noise, all in one run:

  (a) rt_jpeg_encode (its four launches) from device events over back-to-back calls on packed NV12 planes, with the stream's bytes
      and bytes per pixel read from the state record; repeated calls over one frame are served by the Infinity Cache, as the YUV
      pack's figures are;
  (b) host loops on the context's own surfaces and stream, waiting for the previous ticket in every iteration:
      rt_render alone, rt_render + rt_present_submit_yuv, rt_render + rt_present_submit_jpeg (quality 90, 8 MCUs per segment,
      --cap-kib of slot per frame), alternating, and the residual of each over the render.

--trace-only issues 20 encodes of every configuration of (a) and nothing else: the program to put behind
`rocprofv3 --kernel-trace --output-format csv` for the split per kernel (rt_jpeg_transform, rt_jpeg_entropy<false> = count,
rt_jpeg_scan, rt_jpeg_entropy<true> = emit); --summarise-trace <its kernel_trace.csv> then adds each kernel's median per
configuration to the record file, without a GPU.  Writes one record per size to --out (default profiles/jpeg_bench.json)."""
import argparse, csv, ctypes, json, os, statistics, sys
import numpy as np

SIZES = "1920x1080,3840x2160"
KERNELS = (("transform", "rt_jpeg_transform"), ("count", "rt_jpeg_entropy<false>"), ("scan", "rt_jpeg_scan"), ("emit", "rt_jpeg_entropy<true>"))
TRACE_CALLS = 20


def configurations(w):
    """The (key, quality, interval) of part (a), in the order they are launched."""
    return [(f"{content}_q{quality}_{name}", content, quality, interval) for content in ("c2", "noise") for quality in (50, 90)
            for name, interval in (("mcu", 1), ("eight", 8), ("row", (w + 15) // 16))]


def summarise_trace(trace_csv, out, sizes):
    """--trace-only's kernel trace -> the median microseconds of each of the four kernels per configuration, into the record file.
    The dispatches come in launch order: TRACE_CALLS encodes of four kernels for every configuration of every size.  Needs no GPU."""
    with open(trace_csv, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "rt_jpeg_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    keys = [(size, key) for size in sizes for key, _, _, _ in configurations(size[0])]
    assert len(rows) == len(keys) * TRACE_CALLS * 4, (len(rows), len(keys))
    split = {}
    for n, (size, key) in enumerate(keys):
        chunk = rows[n * TRACE_CALLS * 4: (n + 1) * TRACE_CALLS * 4]
        rec = {}
        for name, pattern in KERNELS:
            mine = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in chunk if pattern in r["Kernel_Name"]]
            assert len(mine) == TRACE_CALLS, (key, name, len(mine))
            rec[f"{name}_us"] = round(statistics.median(mine), 2)
        split.setdefault(f"{size[0]}x{size[1]}", {})[key] = rec
    with open(out) as f:
        doc = json.load(f)
    doc["kernel_split_us"] = split
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return split


if "--summarise-trace" in sys.argv:                             # (before the imports that want a device)
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarise-trace", required=True, metavar="KERNEL_TRACE_CSV")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "jpeg_bench.json"))
    ap.add_argument("--sizes", default=SIZES)
    a = ap.parse_args()
    print(json.dumps(summarise_trace(a.summarise_trace, a.out, [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]), indent=1))
    sys.exit(0)

import stagebench as sb                                         # (puts the repository on sys.path)
import torch
from opengl_raytracing_amd import host, scenes
from opengl_raytracing_amd import layout as L

ap = argparse.ArgumentParser()
sb.add_common_args(ap, "jpeg_bench.json", launches=50, parent_lib=False)
ap.add_argument("--cap-kib", type=int, default=1024, help="slot capacity of the present loop per 1080p frame (scaled by the pixel count)")
ap.add_argument("--trace-only", action="store_true")
ap.add_argument("--sizes", default=SIZES)
args = ap.parse_args()
WARM = 5

new = sb.tracer(None)
sc = scenes.make_scene(2, host.generate_aabb)
new.load(sc)
side = sb.side()

records = []
for (w, h) in [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]:
    p = sc.params(width=w, height=h)
    rec = {"size": [w, h], "frames": args.frames, "repeats": args.repeats, "launches": args.launches}
    col = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    pos = torch.empty_like(col)
    nrm = torch.empty((h, w, 4), dtype=torch.float16, device="cuda")
    new.render_to(p, col.data_ptr(), pos.data_ptr(), nrm.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    del pos, nrm
    nbytes = host.yuv_layout(w, h).bytes
    planes = {"c2": torch.empty((nbytes,), dtype=torch.uint8, device="cuda"),
              "noise": torch.from_numpy(np.random.default_rng(1).integers(0, 256, nbytes, dtype=np.uint8)).cuda()}
    new.display_pack_yuv(col, planes["c2"], w, h, format="nv12", matrix="bt601", range="full", flip=True, stream=side)
    side.synchronize()
    del col
    row = (w + 15) // 16

    # ---- (a) the encode alone
    launches, keep = {}, {}
    assert L.JPEG_DEFAULT_INTERVAL == 8
    for key, content, quality, interval in configurations(w):
        lay = host.jpeg_layout(w, h, quality, interval)
        bufs = (torch.empty((lay.scratch_bytes,), dtype=torch.uint8, device="cuda"), torch.empty((lay.worst_bytes,), dtype=torch.uint8, device="cuda"),
                torch.zeros((64,), dtype=torch.uint8, device="cuda"))
        keep[key] = bufs
        launches[key] = (lambda pl=planes[content], b=bufs, lay=lay, q=quality, iv=interval:
                         new.jpeg_encode(pl, b[0], b[1], lay.worst_bytes, b[2], w, h, "nv12", q, iv, stream=side))
    if args.trace_only:
        for f in launches.values():
            for _ in range(TRACE_CALLS):
                f()
        side.synchronize()
        continue
    us = sb.alternate(launches, args.launches, args.repeats, WARM)
    for k, v in us.items():
        sb.summarise(rec, f"encode_{k}", v, "us")
        st = keep[k][2].cpu().numpy().view(L.JPEG_STATE_DTYPE)[0]
        assert st["overflow"] == 0
        rec[f"encode_{k}_bytes"] = int(st["bytes"])
        rec[f"encode_{k}_bytes_per_pixel"] = round(int(st["bytes"]) / (w * h), 4)
        rec[f"encode_{k}_segments"] = int(st["nSegments"])
    del launches, keep, planes

    # ---- (b) host loops on the context's own surfaces and stream
    cap = args.cap_kib * 1024 * (w * h) // (1920 * 1080)
    rec["present_cap_bytes"] = cap

    def frame_loop(kind):
        lib, ctx = new.lib, new.ctx
        ydesc = L.make_yuv_desc(w, h, "nv12", "bt601", "full", flip=True)
        jdesc = L.make_jpeg_desc(w, h, 90)

        def submit(d_color, tk):
            if kind == "yuv":
                sb.check(new, lib.rt_present_submit_yuv(ctx, d_color, ctypes.byref(ydesc), None, None, tk), "rt_present_submit_yuv")
            else:
                sb.check(new, lib.rt_present_submit_jpeg(ctx, d_color, ctypes.byref(ydesc), None, ctypes.byref(jdesc), cap, None, tk), "rt_present_submit_jpeg")
        return sb.present_loop(new, p, submit)

    loops = {"render_only": sb.render_loop(new, p), "render_present_yuv": frame_loop("yuv"), "render_present_jpeg": frame_loop("jpeg")}
    for k, v in sb.time_host_loops(loops, args.frames, args.repeats).items():
        sb.summarise(rec, k, v, "ms")
    rec["yuv_delivery_residual_ms"] = round(rec["render_present_yuv_ms"] - rec["render_only_ms"], 4)
    rec["jpeg_delivery_residual_ms"] = round(rec["render_present_jpeg_ms"] - rec["render_only_ms"], 4)
    print(json.dumps(rec), flush=True)
    records.append(rec)

if not args.trace_only:
    sb.write_records(args.out, "tools/bench_jpeg.py", records, scene="C2")
new.close()
