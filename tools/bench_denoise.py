"""Secondary measurement (not the BASELINE metric): what the denoiser costs, at 1920x1080 and 3840x2160, all in one run:

  (a) rt_denoise (prepare + n iterations) for n = 1..5 from device events over back-to-back launches on an accumulator of eight noisy
      frames and a guide of blocks of objects with turning normals; the difference of n and n - 1 iterations is the cost of the step
      2^(n-1).  Beside it, in the same run, a device copy that moves the 48 compulsory bytes per pixel of one iteration (24 read, 24
      written): the ratio to that copy and the achieved compulsory bytes per second.  rt_denoise_guide and a 1 x 1 rt_denoise (the
      launches alone) are timed too.
      --variant NAME=PATH (repeatable) times libraries built with other RT_DENOISE_* macros (tools/build_variants.py) alternately
      with this build's: the kernel forms of DESIGN.md 21.
  (b) host loops on the context's own stream and surfaces: rt_render + rt_accum_add on a library built from the PARENT commit
      (--parent-lib) and on this build, alternating, and rt_render + rt_accum_add + rt_denoise on this build: the frame-loop residual.

Writes one record per size to --out (default profiles/denoise_bench.json)."""
import argparse, ctypes, json
import stagebench as sb                                         # (puts the repository on sys.path)
import torch
from opengl_raytracing_amd import host, scenes
from opengl_raytracing_amd import layout as L

ap = argparse.ArgumentParser()
sb.add_common_args(ap, "denoise_bench.json", launches=50, variant_macros="RT_DENOISE_")
args = ap.parse_args()
variant_libs = sb.parse_variants(args.variant)
WARM = 5                                                        # launches of each candidate in front of the first timed batch

new, old, variants = sb.open_tracers(args.parent_lib, variant_libs)
tracers = sb.distinct([new, old, *variants.values()])
sc = scenes.make_scene(2, host.generate_aabb)
for t in tracers:
    t.load(sc)
side = sb.side()


def synthetic_hits(w, h):
    """rt_hit records on the device: objects in blocks of 97 x 61 pixels with a band of misses, normals that turn across each block."""
    y, x = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
    obj = ((x // 97) % 5 + 5 * ((y // 61) % 3)).to(torch.int32)
    obj[(y % 200) < 12] = -1
    u, v = (x % 97).float() / 97 - 0.5, (y % 61).float() / 61 - 0.5
    n = torch.stack([u, v, torch.sqrt(1 - u * u - v * v)], dim=-1) * 1.7
    n[obj < 0] = 0
    hits = torch.zeros((h, w, 8), dtype=torch.float32, device="cuda")
    hits[..., 4:7] = n
    hits[..., 7] = obj.view(torch.float32)
    return hits


def loop(t, p, accum=None, denoise=None):
    """n frames of rt_render (+ rt_accum_add with `accum` = (d_accum, d_state, desc)) (+ rt_denoise with `denoise` = (d_guide,
    d_scratch, d_out, desc)) on t's own stream."""
    lib, ctx, vp = t.lib, t.ctx, ctypes.c_void_p
    plane = p.regionW * p.regionH * 16

    def add(d_color, k):
        sb.check(t, lib.rt_accum_add(ctx, d_color, vp(accum[0].data_ptr()), ctypes.byref(accum[2]), vp(accum[1].data_ptr()), None), "rt_accum_add")

    def smooth(d_color, k):
        sb.check(t, lib.rt_denoise(ctx, vp(accum[0].data_ptr()), vp(accum[0].data_ptr() + plane), vp(denoise[0].data_ptr()),
                                   vp(denoise[1].data_ptr()), vp(denoise[2].data_ptr()), ctypes.byref(denoise[3]), None), "rt_denoise")
    return sb.render_loop(t, p, ([add] if accum else []) + ([smooth] if denoise else []))


records = []
for (w, h) in [(1920, 1080), (3840, 2160)]:
    rec = {"size": [w, h], "frames": args.frames, "repeats": args.repeats, "launches": args.launches,
           "parent": "parent build" if args.parent_lib else "this build"}
    gen = torch.Generator(device="cuda").manual_seed(w)
    base = torch.rand((h, w, 4), device="cuda", generator=gen) ** 4 * 8
    d_accum, d_state = new.accum_alloc(w, h)
    for _ in range(8):
        new.accum_add(base * torch.exp(0.5 * torch.randn((h, w, 4), device="cuda", generator=gen) - 0.125), d_accum, d_state, w, h)
    d_hits = synthetic_hits(w, h)
    d_guide = new.denoise_guide(d_hits, w, h)
    d_scratch, d_out = new.denoise_alloc(w, h)
    tiny = [torch.zeros(64, dtype=torch.uint8, device="cuda") for _ in range(5)]
    copy_src = torch.zeros(w * h * 24, dtype=torch.uint8, device="cuda")
    copy_dst = torch.empty_like(copy_src)
    mean, moments = new.accum_mean(d_accum, w, h), new.accum_moments(d_accum, w, h)
    torch.cuda.synchronize()

    # ---- (a) the filter beside a copy of one iteration's compulsory bytes; the kernel forms beside each other
    launches = {"copy48": lambda: copy_dst.copy_(copy_src),
                "guide": lambda: new.denoise_guide(d_hits, w, h, out=d_guide, stream=side),
                "fixed4": lambda: new.denoise(tiny[0], tiny[1], tiny[2], tiny[3], tiny[4], 1, 1, stream=side)}
    for name, t in variants.items():
        for n in range(1, 6):
            launches[f"denoise{n}_{name}"] = lambda t=t, n=n: t.denoise(mean, moments, d_guide, d_scratch, d_out, w, h, iterations=n, stream=side)
    with torch.cuda.stream(side):
        us = sb.alternate(launches, args.launches, args.repeats, WARM)
    for k, v in us.items():
        sb.summarise(rec, k, v, "us")
    nbytes = w * h * 48
    rec["copy48_TBps"] = round(nbytes / rec["copy48_us"] * 1e-6, 3)
    for name in variants:
        t = [rec[f"denoise{n}_{name}_us"] for n in range(1, 6)]
        rec[f"steps_{name}_us"] = {"prepare+step1": t[0], **{f"step{1 << n}": round(t[n] - t[n - 1], 2) for n in range(1, 5)}}
        rec[f"denoise4_{name}_per_iteration_us"] = round(t[3] / 4, 2)
        rec[f"denoise4_{name}_over_copy48_per_iteration"] = round(t[3] / 4 / rec["copy48_us"], 3)
        rec[f"denoise4_{name}_TBps"] = round((4 * nbytes + w * h * 64) / t[3] * 1e-6, 3)       # + prepare: 48 read, 16 written
    out_this = d_out.clone()
    for name, t in variants.items():                          # faster and different is not faster: every form gives the same bytes
        t.denoise(mean, moments, d_guide, d_scratch, d_out, w, h, iterations=5, stream=side)
        side.synchronize()
        if name == "this":
            out_this = d_out.clone()
        rec[f"denoise5_{name}_same_bytes_as_this"] = bool(torch.equal(d_out.view(torch.int32), out_this.view(torch.int32)))
    del copy_src, copy_dst

    # ---- (b) host loops on each context's own surfaces and stream
    p = sc.params(width=w, height=h)
    new.accum_reset(d_accum, d_state, w, h)
    torch.cuda.synchronize()
    adesc, ddesc = L.make_accum_desc(w, h), L.make_denoise_desc(w, h)
    loops = {"render_accum_parent": loop(old, p, (d_accum, d_state, adesc)), "render_accum_this": loop(new, p, (d_accum, d_state, adesc)),
             "render_accum_denoise": loop(new, p, (d_accum, d_state, adesc), (d_guide, d_scratch, d_out, ddesc))}
    times = sb.time_host_loops(loops, args.frames, args.repeats)
    for k, v in times.items():
        sb.summarise(rec, k, v, "ms")
    rec["render_accum_parent_spread_ms"] = round(sb.spread(times["render_accum_parent"]), 4)
    rec["render_accum_this_minus_parent_ms"] = round(rec["render_accum_this_ms"] - rec["render_accum_parent_ms"], 4)
    rec["denoise_residual_ms"] = round(rec["render_accum_denoise_ms"] - rec["render_accum_this_ms"], 4)
    del d_accum, d_state, d_guide, d_scratch, d_out, d_hits, mean, moments, out_this, base
    print(json.dumps(rec), flush=True)
    records.append(rec)

sb.write_records(args.out, "tools/bench_denoise.py", records, scene="C2", variants=variant_libs)
sb.close_all(tracers)
