#!/usr/bin/env python3
"""tools/bench_accel_render.py -- whole frames with and without the hierarchy (rt_set_accel_render, csrc/rt_accel_render.inc), on
tools/stagebench.py's procedure.

    python tools/bench_accel_render.py --parent-lib PATH [--scenes c4,c5,257,1025,4097,4097:device,16385] [--repeats 5]
                                       [--variant NAME=PATH ...] [--out profiles/accel_render_bench.json]

Candidates, one context each on the same scene, alternating in the same call: parent (the parent commit's library: the packet
kernel), off (this build, the switch off: the same kernel), lane, wave and split (rt_set_accel + rt_set_accel_render, minObjects 1),
comp (the composition the fused frame replaces: rt_camera_rays into a ray buffer, then rt_shade_rays with rt_set_accel_shading's
per-ray walk), and one per --variant: a library built with other RT_AR_* macros (tile order, workgroup size), run as split and as
lane.  Scenes: C4 and C5 of scenes.make_scene, and scenes.lit_cloud(n) (n spheres and a floor); `:device` builds the tree with the
device builder.  Frames are DESIGN.md section 33's: 1920x1080, 960x540 from 4096 objects up.  Every candidate is one rt_render_to
(comp: two launches) on stagebench's side stream; per scene one event pair around K back-to-back frames (K shrinks with the scene),
`repeats` times, forward and reversed order in turn.  Reported per candidate: the median and the p10-p90 of the repeats in
microseconds per frame; per scene whether `off` lies inside the parent's p10-p90, which candidates beat or lose to the parent
beyond both spreads, which traversal beats the other two beyond theirs, whether the fused frame loses to the composition, and that
every candidate's three surfaces equal the off path's bit for bit."""
import argparse
import ctypes

import stagebench as sb                    # (sets sys.path for the package)
import torch

from opengl_raytracing_amd import host, scenes

WALKS = ("lane", "wave", "split")


def percentile(values, f):
    v = sorted(values)
    return v[min(len(v) - 1, int(f * len(v)))]


def scene_of(name):
    if name.startswith("c"):
        return scenes.make_scene(int(name[1:]), host.generate_aabb)
    n = int(name)
    return scenes.lit_cloud(n, 0x5AADE + n, host.generate_aabb)


def same_bits(a, b):
    """Two surface triples equal bit for bit, NaN == NaN."""
    for x, y in zip(a, b):
        x, y = x.float(), y.float()
        if not bool(((x == y) | (x.isnan() & y.isnan())).all()):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    sb.add_common_args(ap, "accel_render_bench.json", variant_macros="RT_AR_")
    ap.add_argument("--scenes", default="c4,c5,257,1025,4097,4097:device,16385")
    a = ap.parse_args()
    new, old, _ = sb.open_tracers(a.parent_lib, {})
    tracers = {"parent": old, "off": new, **{w: host.RayTracer(0) for w in WALKS}, "comp": host.RayTracer(0)}
    walk_of = {w: w for w in WALKS}
    for name, path in sb.parse_variants(a.variant).items():
        for w in ("split", "lane"):
            tracers[f"{name}:{w}"] = sb.tracer(path)
            walk_of[f"{name}:{w}"] = w
    through_tree = [k for k in tracers if k not in ("parent", "off")]
    for name in through_tree:
        tracers[name].set_accel(min_objects=1)
    for name, w in walk_of.items():
        tracers[name].set_accel_render(traversal=w, min_objects=1)
    tracers["comp"].set_accel_shading(traversal="lane", min_objects=1)
    side = sb.side()
    records, builds = [], []
    for scene_name in (s for s in a.scenes.split(",") if s):
        base, _, builder = scene_name.partition(":")
        sc = scene_of(base)
        n_obj = len(sc.objects)
        for name in through_tree:
            tracers[name].set_accel_builder(builder or "host")
        for t in sb.distinct(tracers.values()):
            t.load(sc)
        info = tracers["lane"].accel_info()
        assert all(tracers[name].accel_render_info()["active"] for name in walk_of) and tracers["comp"].accel_shading_info()["active"]
        builds.append(dict(scene=sc.name, objects=n_obj, builder=builder or "host",
                           **{k: info[k] for k in ("nodes", "leaves", "depth", "loose", "bytes", "build_ms")}))
        W, H = (1920, 1080) if n_obj < 4096 else (960, 540)
        p = sc.params(width=W, height=H)
        outs = {k: tuple(torch.empty((H, W, 4), dtype=dt, device="cuda") for dt in (torch.float32, torch.float32, torch.float16))
                for k in ("off", "other")}
        rays = torch.empty((H * W, 8), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def frame(name, o):
            t = tracers[name]
            if name == "comp":
                t._call("rt_camera_rays", ctypes.byref(p), ctypes.c_void_p(rays.data_ptr()), ctypes.c_void_p(side.cuda_stream))
                t.shade_rays(p, rays, out=tuple(x.view(-1, 4) for x in o), stream=side)
            else:
                t.render_to(p, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), stream=side.cuda_stream)

        # the record's own check: every candidate's surfaces against the off path's
        frame("off", outs["off"])
        identical = {}
        for name in tracers:
            if name == "off":
                continue
            for x in outs["other"]:
                x.view(torch.uint8).fill_(0xFF)
            torch.cuda.synchronize()
            frame(name, outs["other"])
            side.synchronize()
            identical[name] = same_bits(outs["other"], outs["off"])
        K = max(1, min(8, 1024 // n_obj))
        us = sb.alternate({name: (lambda name=name: frame(name, outs["other"])) for name in tracers}, K, a.repeats, warm=1)
        rec = dict(scene=sc.name, objects=n_obj, builder=builder or "host", frame=f"{W}x{H}", K=K, identical=identical)
        for name, v in us.items():
            sb.summarise(rec, name, v, "us")
            rec[f"{name}_p10_us"], rec[f"{name}_p90_us"] = round(percentile(v, 0.1), 2), round(percentile(v, 0.9), 2)
        rec["off_inside_parent_p10_p90"] = bool(rec["parent_p10_us"] <= rec["off_us"] <= rec["parent_p90_us"])
        for name in through_tree:
            rec[f"parent_over_{name}"] = round(rec["parent_us"] / rec[f"{name}_us"], 3)
            rec[f"{name}_beats_parent"] = bool(rec[f"{name}_p90_us"] < rec["parent_p10_us"])
            rec[f"{name}_loses_to_parent"] = bool(rec[f"{name}_p10_us"] > rec["parent_p90_us"])
        best = [w for w in WALKS if all(rec[f"{w}_p90_us"] < rec[f"{o}_p10_us"] for o in WALKS if o != w)]
        rec["best_walk"] = best[0] if best else None                # None: a tie within the spreads
        for w in WALKS:
            rec[f"{w}_loses_to_comp"] = bool(rec[f"{w}_p10_us"] > rec["comp_p90_us"])
        for name in (n for n in tracers if ":" in n):               # a form is kept only if its p90 lies below the other's p10
            w = walk_of[name]
            rec[f"{name}_beats_shipped"] = bool(rec[f"{name}_p90_us"] < rec[f"{w}_p10_us"])
            rec[f"{name}_loses_to_shipped"] = bool(rec[f"{name}_p10_us"] > rec[f"{w}_p90_us"])
        records.append(rec)
        print(f"{scene_name:<14}{n_obj:>6} {W}x{H} K={K:<2}" + "".join(
            f"  {name} {rec[name + '_us']:>11.1f} ({rec[name + '_p10_us']:.1f}-{rec[name + '_p90_us']:.1f})" for name in tracers)
            + f"  best {rec['best_walk']}  identical {all(identical.values())}", flush=True)
    for b in builds:
        print(f"{b['scene']:<20}{b['objects']:>6} {b['builder']:<6} nodes {b['nodes']:>6} leaves {b['leaves']:>6} depth {b['depth']:>3} "
              f"loose {b['loose']:>3} {b['bytes']:>8} B  build {b['build_ms']:.2f} ms")
    sb.write_records(a.out, "tools/bench_accel_render.py", records, tail=dict(builds=builds), repeats=a.repeats,
                     unit="us per frame", parent_lib=bool(a.parent_lib), variants=sorted(sb.parse_variants(a.variant)))
    sb.close_all(list(tracers.values()))


if __name__ == "__main__":
    main()
