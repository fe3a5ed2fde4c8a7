#!/usr/bin/env python3
"""tools/bench_accel.py -- rt_trace_rays with and without the hierarchy of rt_set_accel (csrc/rt_accel.inc), on
tools/stagebench.py's procedure.

    python tools/bench_accel.py [--sizes 256,1024,4096,16384,65536] [--repeats 5] [--out profiles/accel_bench.json]

Scenes: scenes.sphere_cloud (seeded spheres at constant density plus a floor, n objects in all) at every size, and C4 and C5 themselves.
Ray sets: coherent = the primary rays of a 1920x1080 frame (for a cloud: a camera on the +z side that sees the whole cube);
incoherent = tools/bench_query.py's 2^22 seeded rays (origins uniform in a cube, isotropic directions; for a cloud the cube is
the cloud's own).  Modes: closest and any.  Paths: off (the brute-force kernels), wave and lane (minObjects 1), one context each
on the same scene, alternating in the same call: per case one event pair around K back-to-back launches, `repeats` times, forward
and reversed order in turn.  Reported per path: the median and the p10-p90 of the repeats in microseconds per launch; per scene
the host build time.  K shrinks with the scene (a brute-force launch over 65536 objects takes a tenth of a second)."""
import argparse
import os
import statistics
import sys

import stagebench as sb                    # (sets sys.path for the package)
import torch

from opengl_raytracing_amd import host, scenes
from opengl_raytracing_amd import layout as L

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_query import incoherent_rays  # noqa: E402

PATHS = {"off": None, "wave": dict(traversal="wave", min_objects=1), "lane": dict(traversal="lane", min_objects=1)}


def cloud(n):
    objs, half = scenes.sphere_cloud(n - 1, 0xACCE1 + n, host.generate_aabb)      # n objects with the floor
    cam = dict(scenes.CAMERA, cam_pos=(0.0, 0.0, 3.5 * half))
    return scenes.Scene(f"cloud{n}", objs, L.default_lights(1), 1920, 1080, 1, cam), half


def percentile(values, f):
    v = sorted(values)
    return v[min(len(v) - 1, int(f * len(v)))]


def main():
    ap = argparse.ArgumentParser()
    sb.add_common_args(ap, "accel_bench.json", parent_lib=False)
    ap.add_argument("--sizes", default="256,1024,4096,16384,65536")
    ap.add_argument("--configs", default="4,5")
    ap.add_argument("--incoherent", type=int, default=1 << 22)
    a = ap.parse_args()
    cases = [cloud(int(n)) for n in a.sizes.split(",") if n] + [(scenes.make_scene(int(c), host.generate_aabb), 20.0) for c in a.configs.split(",") if c]
    tracers = {name: host.RayTracer(0) for name in PATHS}
    for name, desc in PATHS.items():
        if desc:
            tracers[name].set_accel(**desc)
    side = sb.side()
    records, builds = [], []
    base = incoherent_rays(a.incoherent)
    for sc, half in cases:
        n_obj = len(sc.objects)
        for t in tracers.values():
            t.load(sc)
        info = {name: tracers[name].accel_info() for name in ("wave", "lane")}
        assert all(i["built"] for i in info.values())
        builds.append(dict(scene=sc.name, objects=n_obj, **{k: info["wave"][k] for k in ("nodes", "leaves", "depth", "loose", "bytes", "build_ms")}))
        inc = base.clone()
        inc[:, 0:3] *= half / 20.0
        sets = {"coherent": tracers["off"].camera_rays(sc.params(width=1920, height=1080)).reshape(-1, 8), "incoherent": inc}
        torch.cuda.synchronize()
        K = max(1, min(20, 8192 // n_obj))
        for set_name, rays in sets.items():
            n = rays.shape[0]
            for mode in ("closest", "any"):
                out = (torch.empty((n, 8), dtype=torch.float32, device="cuda") if mode == "closest" else torch.empty(n, dtype=torch.int32, device="cuda"))
                launches = {name: (lambda t=t: t.trace_rays(rays, mode, out=out, stream=side)) for name, t in tracers.items()}
                us = sb.alternate(launches, K, a.repeats, warm=2)
                rec = dict(scene=sc.name, objects=n_obj, rays=set_name, n=n, mode=mode, K=K)
                for name, v in us.items():
                    sb.summarise(rec, name, v, "us")
                    rec[f"{name}_p10_us"], rec[f"{name}_p90_us"] = round(percentile(v, 0.1), 2), round(percentile(v, 0.9), 2)
                rec["off_over_wave"] = round(statistics.median(us["off"]) / statistics.median(us["wave"]), 3)
                rec["off_over_lane"] = round(statistics.median(us["off"]) / statistics.median(us["lane"]), 3)
                records.append(rec)
                print(f"{sc.name:<22}{n_obj:>6} {set_name:<10} {mode:<7} K={K:<3}" + "".join(
                    f"  {name} {rec[name + '_us']:>10.1f} ({rec[name + '_p10_us']:.1f}-{rec[name + '_p90_us']:.1f})" for name in PATHS), flush=True)
    for b in builds:
        print(f"{b['scene']:<22}{b['objects']:>6} nodes {b['nodes']:>6} leaves {b['leaves']:>6} depth {b['depth']:>3} loose {b['loose']:>3} "
              f"{b['bytes']:>8} B  build {b['build_ms']:.2f} ms")
    sb.write_records(a.out, "tools/bench_accel.py", records, tail=dict(builds=builds), repeats=a.repeats, unit="us per rt_trace_rays launch")
    sb.close_all(tracers.values())


if __name__ == "__main__":
    main()
