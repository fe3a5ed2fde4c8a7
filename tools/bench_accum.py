"""Secondary measurement (not the BASELINE metric): what progressive accumulation costs, at 1920x1080 and 3840x2160, all in one run:

  (a) rt_accum_add (clear + accumulate + solve) from device events over back-to-back launches on noisy content, beside a device copy
      that moves the same 80 bytes per pixel (40 read, 40 written) in the same run: the achieved bytes per second of both and the
      fraction.  The clear, the solve and the launches cost the same whatever the frame's size: rt_accum_add on a 1 x 1 frame is
      reported as that fixed part, the rest as the accumulate kernel.  Repeated launches over one accumulator are served by the
      Infinity Cache where it fits (1080p: 66 MB + 33 MB of image); the 4K accumulator (265 MB) does not.
      --variant NAME=PATH (repeatable) times libraries built with other RT_ACCUM_* macros (tools/build_variants.py) alternately
      with this build's, here and in the loop of (b): the kernel forms of DESIGN.md 20.
  (b) host loops on the context's own stream and surfaces: rt_render on a library built from the PARENT commit (--parent-lib) and on
      this build, alternating, and rt_render + rt_accum_add on this build.
  (c) how many samples per pixel and how much wall time the loop of (b) takes until state.done at relError 0.02 / donePermille 950,
      reading the 4 bytes of `done` every 8 frames, on C2 and on C3's scene (the one with the noise texture) at 1080p.

Writes one record per size to --out (default profiles/accum_bench.json)."""
import argparse, ctypes, json, time
import stagebench as sb                                         # (puts the repository on sys.path)
import numpy as np
import torch
from opengl_raytracing_amd import host, scenes
from opengl_raytracing_amd import layout as L

ap = argparse.ArgumentParser()
sb.add_common_args(ap, "accum_bench.json", launches=100, variant_macros="RT_ACCUM_")
ap.add_argument("--max-spp", type=int, default=4096)
args = ap.parse_args()
variant_libs = sb.parse_variants(args.variant)
WARM = 10                                                       # launches of each candidate in front of the first timed batch

new, old, variants = sb.open_tracers(args.parent_lib, variant_libs)
tracers = sb.distinct([new, old, *variants.values()])
sc = scenes.make_scene(2, host.generate_aabb)
for t in tracers:
    t.load(sc)
side = sb.side()


def render_loop(t, p, accum=None):
    """n frames of rt_render (+ rt_accum_add on the colour surface when `accum` = (d_accum, d_state, desc)) on t's own stream."""
    lib, ctx = t.lib, t.ctx

    def add(d_color, k):
        sb.check(t, lib.rt_accum_add(ctx, d_color, ctypes.c_void_p(accum[0].data_ptr()), ctypes.byref(accum[2]),
                                     ctypes.c_void_p(accum[1].data_ptr()), None), "rt_accum_add")
    return sb.render_loop(t, p, [add] if accum else [])


def until_done(t, scene, w, h):
    """Frames and seconds until state.done under the default description, the frame count moving the samples; `done` is read every
    8 frames (a 4-byte copy behind a sync of the context's stream)."""
    t.load(scene)
    d_accum, d_state = t.accum_alloc(w, h)
    desc = L.make_accum_desc(w, h)
    lib, ctx, d_color = t.lib, t.ctx, ctypes.c_void_p()
    done = torch.zeros(1, dtype=torch.int32).pin_memory()
    frames, t0 = 0, time.perf_counter()
    while frames < args.max_spp:
        scene.frame_count = frames
        p = scene.params(width=w, height=h)
        sb.check(t, lib.rt_render(ctx, ctypes.byref(p)), "rt_render")
        sb.check(t, lib.rt_get_surfaces(ctx, ctypes.byref(d_color), None, None), "rt_get_surfaces")
        sb.check(t, lib.rt_accum_add(ctx, d_color, ctypes.c_void_p(d_accum.data_ptr()), ctypes.byref(desc), ctypes.c_void_p(d_state.data_ptr()), None), "rt_accum_add")
        frames += 1
        if frames % 8 == 0:
            t.sync()
            done.copy_(d_state[L.ACCUM_DONE_OFFSET: L.ACCUM_DONE_OFFSET + 4].view(torch.int32))
            if int(done[0]):
                break
    t.sync()
    seconds = time.perf_counter() - t0
    st = d_state.cpu().numpy().view(L.ACCUM_STATE_DTYPE)[0]
    return {"frames": frames, "seconds": round(seconds, 4), "done": int(st["done"]), "converged_share": round(int(st["nConverged"]) / (w * h), 4),
            "medianBin": int(st["medianBin"]), "p95Bin": int(st["p95Bin"]), "nUnsampled": int(st["nUnsampled"])}


records = []
for (w, h) in [(1920, 1080), (3840, 2160)]:
    rec = {"size": [w, h], "frames": args.frames, "repeats": args.repeats, "launches": args.launches,
           "parent": "parent build" if args.parent_lib else "this build"}
    rng = np.random.default_rng(w)
    base = (rng.uniform(0, 1, (h, w, 4)) ** 4 * 8).astype(np.float32)
    imgs = [torch.from_numpy((base * rng.gamma(2.0, 0.5, base.shape)).astype(np.float32)).cuda() for _ in range(2)]
    d_accum, d_state = new.accum_alloc(w, h)
    tiny_accum, tiny_state = new.accum_alloc(1, 1)
    copy_src = torch.zeros(w * h * 40, dtype=torch.uint8, device="cuda")
    copy_dst = torch.empty_like(copy_src)
    torch.cuda.synchronize()
    flip = [0]

    def add(t, img=None):
        flip[0] ^= 1
        t.accum_add(imgs[flip[0]], d_accum, d_state, w, h, stream=side)

    # ---- (a) the add beside a copy of the same bytes; the kernel forms beside each other
    launches = {"copy80": lambda: copy_dst.copy_(copy_src), "fixed": lambda: new.accum_add(imgs[0], tiny_accum, tiny_state, 1, 1, stream=side)}
    for name, t in variants.items():
        launches["add_" + name] = lambda t=t: add(t)
    with torch.cuda.stream(side):
        us = sb.alternate(launches, args.launches, args.repeats, WARM)
    for k, v in us.items():
        sb.summarise(rec, k, v, "us")
    nbytes = w * h * 80
    rec["copy80_TBps"] = round(nbytes / rec["copy80_us"] * 1e-6, 3)
    for name in variants:
        rec[f"add_{name}_TBps"] = round(nbytes / rec[f"add_{name}_us"] * 1e-6, 3)
        rec[f"add_{name}_over_copy80"] = round(rec[f"add_{name}_us"] / rec["copy80_us"], 3)
    rec["add_this_kernel_us"] = round(rec["add_this_us"] - rec["fixed_us"], 2)
    rec["add_this_kernel_TBps"] = round(nbytes / rec["add_this_kernel_us"] * 1e-6, 3)
    rec["add_this_fraction_of_copy80"] = round(rec["copy80_us"] / rec["add_this_us"], 3)
    new.accum_view(d_accum, copy_dst, w, h, mode="relerr", stream=side)
    side.synchronize()
    del copy_src, copy_dst, imgs

    # ---- (b) host loops on each context's own surfaces and stream
    p = sc.params(width=w, height=h)
    new.accum_reset(d_accum, d_state, w, h)
    torch.cuda.synchronize()
    loops = {"render_parent": render_loop(old, p), "render_this": render_loop(new, p),
             "render_accum": render_loop(new, p, (d_accum, d_state, L.make_accum_desc(w, h)))}
    for name, t in variants.items():                       # the other kernel forms in the loop, where the render evicts between two adds
        if t is not new:
            loops["render_accum_" + name] = render_loop(t, p, (d_accum, d_state, L.make_accum_desc(w, h)))
    times = sb.time_host_loops(loops, args.frames, args.repeats)
    for k, v in times.items():
        sb.summarise(rec, k, v, "ms")
    rec["render_parent_spread_ms"] = round(sb.spread(times["render_parent"]), 4)
    rec["render_this_minus_parent_ms"] = round(rec["render_this_ms"] - rec["render_parent_ms"], 4)
    rec["accum_residual_ms"] = round(rec["render_accum_ms"] - rec["render_this_ms"], 4)
    del d_accum, d_state

    # ---- (c) until done
    if (w, h) == (1920, 1080):
        rec["until_done_c2"] = until_done(new, scenes.make_scene(2, host.generate_aabb), w, h)
        rec["until_done_c3_scene"] = until_done(new, scenes.make_scene(3, host.generate_aabb), w, h)
        new.load(sc)
    print(json.dumps(rec), flush=True)
    records.append(rec)

sb.write_records(args.out, "tools/bench_accum.py", records, scene="C2", variants=variant_libs)
sb.close_all(tracers)
