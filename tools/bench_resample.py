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
import argparse, ctypes, itertools, json
import stagebench as sb                                         # (puts the repository on sys.path)
import torch
from opengl_raytracing_amd import host, scenes
from opengl_raytracing_amd import layout as L

ap = argparse.ArgumentParser()
sb.add_common_args(ap, "resample_bench.json", launches=100)
ap.add_argument("--variant-lib", default=None, help="another build of this library to time beside it")
ap.add_argument("--variant-name", default="variant")
ap.add_argument("--rotate-mib", type=int, default=640)
ap.add_argument("--note", default=None, help="free text stored with the records")
args = ap.parse_args()
WARM = 20                                                       # launches of each candidate in front of the first timed batch

new, old, variants = sb.open_tracers(args.parent_lib, {args.variant_name: args.variant_lib} if args.variant_lib else {})
variant = variants[args.variant_name] if args.variant_lib else None
side = sb.side()

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

    turn = itertools.count()                                    # every launch reads the buffer after the one the launch before it read

    def copy():
        with torch.cuda.stream(side):
            copy_dst.copy_(copy_src[next(turn) % n_copy])

    launches = {"copy": copy}
    for f in ("area", "triangle", "lanczos3"):
        launches[f] = lambda f=f: new.resample(srcs[next(turn) % n_src], dst, sw, sh, dw, dh, filter=f, stream=side)
        if variant is not None:
            launches[f"{f}_{args.variant_name}"] = lambda f=f: variant.resample(srcs[next(turn) % n_src], dst, sw, sh, dw, dh, filter=f, stream=side)
    us = sb.alternate(launches, args.launches, args.repeats, WARM)
    for k, v in us.items():
        sb.summarise(rec, k, v, "us")
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
for t in sb.distinct([new, old]):
    t.load(sc)
W4, H4, W2, H2 = 3840, 2160, 1920, 1080
p4 = sc.params(width=W4, height=H4)
d_small = torch.empty((H2, W2, 4), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()


def deliver_loop(t, filter):
    lib, ctx = t.lib, t.ctx
    desc = L.make_display_desc(W2, H2, "srgb", flip=True)
    rdesc = L.make_resample_desc(W4, H4, W2, H2, filter)
    small = ctypes.c_void_p(d_small.data_ptr())

    def submit(d_color, tk):
        sb.check(t, lib.rt_display_resample(ctx, d_color, small, ctypes.byref(rdesc), None), "rt_display_resample")
        sb.check(t, lib.rt_present_submit(ctx, small, ctypes.byref(desc), None, tk), "rt_present_submit")
    return sb.present_loop(t, p4, submit)


loops = {"render4k_only_parent": sb.render_loop(old, p4), "render4k_only": sb.render_loop(new, p4)}
for f in ("area", "triangle", "lanczos3"):
    loops[f"render4k_resample_{f}_present1080"] = deliver_loop(new, f)
loop_rec = {"scene": "C2", "render": [W4, H4], "deliver": [W2, H2], "frames": args.frames, "repeats": args.repeats,
            "yardstick": "parent" if args.parent_lib else "this build"}
for k, v in sb.time_host_loops(loops, args.frames, args.repeats).items():
    sb.summarise(loop_rec, k, v, "ms")
for f in ("area", "triangle", "lanczos3"):
    loop_rec[f"residual_{f}_ms"] = round(loop_rec[f"render4k_resample_{f}_present1080_ms"] - loop_rec["render4k_only_parent_ms"], 4)
print(json.dumps(loop_rec), flush=True)

sb.write_records(args.out, "tools/bench_resample.py", records, note=args.note, tail={"frame_loop": loop_rec})
sb.close_all([new, old, *variants.values()])
