"""Secondary measurement (not the BASELINE metric): what rt_accum_reproject costs, at 1920x1080 and 3840x2160, all in one run:

  (a) rt_accum_reproject from device events over back-to-back launches on a realistic warp: a plane behind a grid of about a
      thousand small spheres, first hits through jittered pixels for two views a small sideways move apart -- a few pixels of motion
      (the spheres twice the plane's) and about a tenth of the pixels disoccluded, as the report that is kept in the record says.
      Beside it, in the same run, a device copy that moves the 128 compulsory bytes per pixel (64 read, 64 written): the ratio to
      that copy and the achieved compulsory bytes per second.  A 1 x 1 call (the clear and the launch alone) is timed too.
      --variant NAME=PATH (repeatable) times libraries built with other RT_REPROJECT_* macros (tools/build_variants.py) alternately
      with this build's: the kernel forms of DESIGN.md 23.  Every form must give the same bytes.
  (b) host loops on the context's own stream and surfaces: rt_render + rt_accum_add on a library built from the PARENT commit
      (--parent-lib) and on this build, alternating, and rt_render + rt_accum_reproject + rt_accum_add on this build (a
      reprojection EVERY frame, ping-pong accumulators): the frame-loop residual.

Writes one record per size to --out (default profiles/reproject_bench.json)."""
import argparse, ctypes, json, math
import stagebench as sb                                         # (puts the repository on sys.path)
import torch
from opengl_raytracing_amd import host, scenes
from opengl_raytracing_amd import layout as L

ap = argparse.ArgumentParser()
sb.add_common_args(ap, "reproject_bench.json", launches=50, variant_macros="RT_REPROJECT_")
args = ap.parse_args()
variant_libs = sb.parse_variants(args.variant)
WARM = 5                                                        # launches of each candidate in front of the first timed batch

new, old, variants = sb.open_tracers(args.parent_lib, variant_libs)
tracers = sb.distinct([new, old, *variants.values()])
sc = scenes.make_scene(2, host.generate_aabb)
for t in tracers:
    t.load(sc)
side = sb.side()


# ---- the warp: a plane at z = -8 behind 43 x 24 spheres of radius 0.06 at z = -4, 0.14 apart
PLANE_Z, SPHERE_Z, SPACING, RADIUS = -8.0, -4.0, 0.14, 0.06
MOVE = 0.037                                                    # sideways: the spheres move 12 px at 1080p, the plane 6


def first_hits(p, gen):
    """rt_hit records [h, w, 8] on the device for the view p (axis-aligned, looking down -z) through pixels jittered by up to one
    pixel either way.  Object 0 is the plane, 1 + k sphere k.  Every ray meets at most the spheres of the four grid cells around the
    point where it crosses z = SPHERE_Z."""
    w, h = p.width, p.height
    tan = math.tan(math.radians(p.fovDeg) * 0.5)
    sx, sy = w / h * tan, tan
    y, x = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float64), torch.arange(w, device="cuda", dtype=torch.float64), indexing="ij")
    j = torch.rand((2, h, w), device="cuda", generator=gen, dtype=torch.float64) * 2 - 1
    ux, uy = ((x + j[0] + 0.5) / (0.5 * w) - 1) * sx, ((y + j[1] + 0.5) / (0.5 * h) - 1) * sy
    d = torch.stack([ux, uy, -torch.ones_like(ux)], dim=-1)
    d = d / d.norm(dim=-1, keepdim=True)
    o = torch.tensor(list(p.camPos), device="cuda", dtype=torch.float64)
    t = (PLANE_Z - o[2]) / d[..., 2]
    obj = torch.zeros((h, w), device="cuda", dtype=torch.int32)
    n = torch.zeros((h, w, 3), device="cuda", dtype=torch.float64)
    n[..., 2] = 1
    at = o + ((SPHERE_Z - o[2]) / d[..., 2])[..., None] * d       # where the ray crosses the spheres' plane
    for di in (0, 1):
        for dj in (0, 1):
            ci, cj = torch.floor(at[..., 0] / SPACING) + di, torch.floor(at[..., 1] / SPACING) + dj
            c = torch.stack([ci * SPACING, cj * SPACING, torch.full_like(ci, SPHERE_Z)], dim=-1)
            oc = o - c
            b = (d * oc).sum(-1)
            disc = b * b - ((oc * oc).sum(-1) - RADIUS * RADIUS)
            ts = -b - torch.sqrt(disc.clamp(min=0))
            hit = (disc > 0) & (ts > 0) & (ts < t)
            t = torch.where(hit, ts, t)
            obj = torch.where(hit, (1 + (ci + 64) + 128 * (cj + 64)).to(torch.int32), obj)
            n = torch.where(hit[..., None], (o + ts[..., None] * d - c) / RADIUS, n)
    hits = torch.zeros((h, w, 8), dtype=torch.float32, device="cuda")
    hits[..., 0:3] = (o + t[..., None] * d).float()
    hits[..., 3] = t.float()
    hits[..., 4:7] = n.float()
    hits[..., 7] = obj.view(torch.float32)
    return hits


def loop(t, p, accum, reproject=None):
    """n frames of rt_render + rt_accum_add with `accum` = (d_accum, d_state, desc) on t's own stream; with `reproject` = (d_hits_prev,
    d_hits_cur, d_accum_other, desc, d_report) a reprojection in front of every add, the two accumulators taking turns."""
    lib, ctx, vp = t.lib, t.ctx, ctypes.c_void_p
    acc = [accum[0].data_ptr(), reproject[2].data_ptr() if reproject else 0]

    def stage(d_color, k):
        cur = 0
        if reproject:
            cur = (k + 1) & 1
            sb.check(t, lib.rt_accum_reproject(ctx, vp(acc[cur ^ 1]), vp(reproject[0].data_ptr()), vp(reproject[1].data_ptr()), vp(acc[cur]),
                                               ctypes.byref(reproject[3]), vp(reproject[4].data_ptr()), None), "rt_accum_reproject")
        sb.check(t, lib.rt_accum_add(ctx, d_color, vp(acc[cur]), ctypes.byref(accum[2]), vp(accum[1].data_ptr()), None), "rt_accum_add")
    return sb.render_loop(t, p, [stage])


records = []
for (w, h) in [(1920, 1080), (3840, 2160)]:
    rec = {"size": [w, h], "frames": args.frames, "repeats": args.repeats, "launches": args.launches,
           "parent": "parent build" if args.parent_lib else "this build"}
    gen = torch.Generator(device="cuda").manual_seed(w)
    pa = L.make_params(w, h, 3)
    pb = L.make_params(w, h, 3, cam_pos=(MOVE, MOVE / 4, 0.0))
    d_hits_a, d_hits_b = first_hits(pa, gen), first_hits(pb, gen)
    base = torch.rand((h, w, 4), device="cuda", generator=gen) ** 4 * 8
    d_prev, d_state = new.accum_alloc(w, h)
    for _ in range(8):
        new.accum_add(base * torch.exp(0.5 * torch.randn((h, w, 4), device="cuda", generator=gen) - 0.125), d_prev, d_state, w, h)
    d_cur = torch.zeros_like(d_prev)
    d_report = torch.zeros(64, dtype=torch.uint8, device="cuda")
    tiny = [torch.zeros(64, dtype=torch.uint8, device="cuda") for _ in range(5)]
    p1 = L.make_params(1, 1, 3)
    copy_src = torch.zeros(w * h * 64, dtype=torch.uint8, device="cuda")
    copy_dst = torch.empty_like(copy_src)
    torch.cuda.synchronize()

    # ---- (a) the call beside a copy of its compulsory bytes; the kernel forms beside each other
    launches = {"copy128": lambda: copy_dst.copy_(copy_src),
                "fixed": lambda: new.reproject(tiny[0], tiny[1], tiny[2], tiny[3], tiny[4], p1, p1, stream=side)}
    for name, t in variants.items():
        launches[f"reproject_{name}"] = lambda t=t: t.reproject(d_prev, d_hits_a, d_hits_b, d_cur, d_report, pa, pb, stream=side)
    with torch.cuda.stream(side):
        us = sb.alternate(launches, args.launches, args.repeats, WARM)
    for k, v in us.items():
        sb.summarise(rec, k, v, "us")
    nbytes = w * h * 128
    rec["copy128_TBps"] = round(nbytes / rec["copy128_us"] * 1e-6, 3)
    out_this = None
    for name, t in variants.items():
        rec[f"reproject_{name}_over_copy128"] = round(rec[f"reproject_{name}_us"] / rec["copy128_us"], 3)
        rec[f"reproject_{name}_TBps"] = round(nbytes / rec[f"reproject_{name}_us"] * 1e-6, 3)
        with torch.cuda.stream(side):                           # faster and different is not faster: every form gives the same bytes
            d_cur.fill_(0x55)
            t.reproject(d_prev, d_hits_a, d_hits_b, d_cur, d_report, pa, pb, stream=side)
        side.synchronize()
        both = torch.cat([d_cur, d_report])
        if name == "this":
            out_this = both.clone()
            r = host.reproject_report(d_report)
            rec["report"] = {k: int(r[k]) for k in ("nPixels", "nReused", "nRejected", "nOffscreen", "nMiss", "minCount", "maxCount", "sumCount")}
            rec["disoccluded_share"] = round((int(r["nRejected"]) + int(r["nOffscreen"])) / int(r["nPixels"]), 4)
        rec[f"reproject_{name}_same_bytes_as_this"] = bool(torch.equal(both, out_this))
    del copy_src, copy_dst

    # ---- (b) host loops on each context's own surfaces and stream
    p = sc.params(width=w, height=h)
    new.accum_reset(d_prev, d_state, w, h)
    torch.cuda.synchronize()
    adesc, rdesc = L.make_accum_desc(w, h), L.make_reproject_desc(pa, pb)
    loops = {"render_accum_parent": loop(old, p, (d_prev, d_state, adesc)), "render_accum_this": loop(new, p, (d_prev, d_state, adesc)),
             "render_reproject_accum": loop(new, p, (d_prev, d_state, adesc), (d_hits_a, d_hits_b, d_cur, rdesc, d_report))}
    times = sb.time_host_loops(loops, args.frames, args.repeats)
    for k, v in times.items():
        sb.summarise(rec, k, v, "ms")
    rec["render_accum_parent_spread_ms"] = round(sb.spread(times["render_accum_parent"]), 4)
    rec["render_accum_this_minus_parent_ms"] = round(rec["render_accum_this_ms"] - rec["render_accum_parent_ms"], 4)
    rec["reproject_residual_ms"] = round(rec["render_reproject_accum_ms"] - rec["render_accum_this_ms"], 4)
    del d_prev, d_cur, d_state, d_hits_a, d_hits_b, base, out_this
    print(json.dumps(rec), flush=True)
    records.append(rec)

sb.write_records(args.out, "tools/bench_reproject.py", records, scene="C2", variants=variant_libs)
sb.close_all(tracers)
