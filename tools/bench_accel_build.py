#!/usr/bin/env python3
"""tools/bench_accel_build.py -- what a scene change costs with the hierarchy on, by builder (rt_set_accel_builder; DESIGN.md
section 36), on tools/stagebench.py's procedure.

    python tools/bench_accel_build.py --parent-lib PATH [--sizes 1024,4096,16384,65536] [--out profiles/accel_build_bench.json]

Three contexts alternate in one call: `parent` (the parent commit's library, which has the host builder only), `host` and `device`
(this build with RT_ACCEL_BUILD_HOST / RT_ACCEL_BUILD_DEVICE), all with rt_set_accel on at minObjects 1.  Scenes: bench_accel.py's
sphere clouds (n objects with the floor) and C5.

(i)   rt_set_scene of a CHANGED scene followed by rt_sync: host wall time per change (two versions of the scene, the spheres of
      the second displaced, uploaded in turn), and for `device` the deviceMs of rt_accel_build_info after every loop;
(ii)  rt_trace_rays on the tree each builder left: bench_accel.py's coherent (1920x1080 primary rays) and incoherent (2^22 seeded
      rays) sets, closest and any, per-wavefront and per-ray walk; device events around K back-to-back launches;
(iii) per scene and builder, (i) plus one coherent closest per-wavefront query: the cost of a frame whose scene changed.

Per figure: the median and the p10-p90 of the repeats."""
import argparse
import os
import sys

import stagebench as sb                    # (sets sys.path for the package)
import torch

from opengl_raytracing_amd import host, scenes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_accel import cloud, percentile  # noqa: E402
from bench_query import incoherent_rays  # noqa: E402

BUILDERS = ("parent", "host", "device")


def moved(sc, seed):
    """The scene with every sphere displaced by up to a radius: other bytes, the same statistics."""
    import numpy as np
    objs = sc.objects.copy()
    spheres = objs["type"] == objs["type"][0]
    objs["position"][spheres] += np.random.default_rng(seed).uniform(-0.5, 0.5, (int(spheres.sum()), 3)).astype(np.float32)
    host.generate_aabb(objs)
    return objs


def stats(rec, key, values, unit):
    sb.summarise(rec, key, values, unit)
    digits = {"us": 2, "ms": 4}[unit]
    rec[f"{key}_p10_{unit}"], rec[f"{key}_p90_{unit}"] = round(percentile(values, 0.1), digits), round(percentile(values, 0.9), digits)


def main():
    ap = argparse.ArgumentParser()
    sb.add_common_args(ap, "accel_build_bench.json", launches=20)
    ap.add_argument("--sizes", default="1024,4096,16384,65536")
    ap.add_argument("--configs", default="5")
    ap.add_argument("--incoherent", type=int, default=1 << 22)
    a = ap.parse_args()
    if not a.parent_lib:
        ap.error("--parent-lib is needed: the parent's figures are taken in the same call")
    cases = [cloud(int(n)) for n in a.sizes.split(",") if n] + [(scenes.make_scene(int(c), host.generate_aabb), 20.0) for c in a.configs.split(",") if c]
    tracers = {"parent": sb.tracer(a.parent_lib), "host": sb.tracer(None), "device": sb.tracer(None)}
    tracers["device"].set_accel_builder("device")
    side = sb.side()
    base = incoherent_rays(a.incoherent)
    changes, queries, frames = [], [], []
    for sc, half in cases:
        n_obj = len(sc.objects)
        versions = [sc.objects, moved(sc, n_obj)]
        for t in tracers.values():
            t.set_accel(traversal="wave", min_objects=1)
            t.load(sc)
        built = {name: t.accel_info() for name, t in tracers.items()}
        assert all(i["built"] for i in built.values())
        assert tracers["device"].accel_build_info()["builder"] == "device" and tracers["host"].accel_build_info()["builder"] == "host"
        # (i) a changed scene, then a sync
        device_ms = []

        def change_loop(name):
            t, count = tracers[name], [0]

            def loop(n):
                for _ in range(n):
                    count[0] += 1
                    t.set_scene(versions[count[0] & 1], sc.lights)
                    t.sync()
                if name == "device":
                    device_ms.append(t.accel_build_info()["device_ms"])
            return loop

        n_frames = max(10, min(a.frames, (1 << 21) // n_obj))
        ms = sb.time_host_loops({name: change_loop(name) for name in BUILDERS}, n_frames, a.repeats, warm=4)
        rec = dict(scene=sc.name, objects=n_obj, frames=n_frames, **{f"{name}_{k}": built[name][k] for name in ("host", "device") for k in ("nodes", "leaves", "depth", "loose")})
        for name in BUILDERS:
            stats(rec, name, ms[name], "ms")
        stats(rec, "device_deviceMs", device_ms[1:], "ms")         # (the first entry is the warm-up loop's)
        changes.append(rec)
        print(f"{sc.name:<22}{n_obj:>6} change+sync ms" + "".join(f"  {name} {rec[name + '_ms']:.4f} ({rec[name + '_p10_ms']:.4f}-{rec[name + '_p90_ms']:.4f})" for name in BUILDERS) +
              f"  deviceMs {rec['device_deviceMs_ms']:.4f}  depth host {rec['host_depth']} device {rec['device_depth']}", flush=True)
        # (ii) the queries on the tree each builder left
        for t in tracers.values():
            t.set_scene(versions[0], sc.lights)
        inc = base.clone()
        inc[:, 0:3] *= half / 20.0
        sets = {"coherent": tracers["host"].camera_rays(sc.params(width=1920, height=1080)).reshape(-1, 8), "incoherent": inc}
        torch.cuda.synchronize()
        primary = {}
        for traversal in ("wave", "lane"):
            for t in tracers.values():
                t.set_accel(traversal=traversal, min_objects=1)
            for set_name, rays in sets.items():
                n = rays.shape[0]
                for mode in ("closest", "any"):
                    out = (torch.empty((n, 8), dtype=torch.float32, device="cuda") if mode == "closest" else torch.empty(n, dtype=torch.int32, device="cuda"))
                    launches = {name: (lambda t=t: t.trace_rays(rays, mode, out=out, stream=side)) for name, t in tracers.items()}
                    us = sb.alternate(launches, a.launches, a.repeats, warm=2)
                    rec = dict(scene=sc.name, objects=n_obj, traversal=traversal, rays=set_name, n=n, mode=mode, K=a.launches)
                    for name in BUILDERS:
                        stats(rec, name, us[name], "us")
                    rec["device_over_host"] = round(rec["device_us"] / rec["host_us"], 3)
                    queries.append(rec)
                    if (traversal, set_name, mode) == ("wave", "coherent", "closest"):
                        primary = rec
                    print(f"{sc.name:<22}{n_obj:>6} {traversal:<5}{set_name:<11}{mode:<8}" + "".join(
                        f"  {name} {rec[name + '_us']:>9.1f} ({rec[name + '_p10_us']:.1f}-{rec[name + '_p90_us']:.1f})" for name in BUILDERS), flush=True)
        # (iii) one 1080p primary-ray query per scene change
        rec = dict(scene=sc.name, objects=n_obj)
        for name in BUILDERS:
            rec[f"{name}_ms"] = round(changes[-1][f"{name}_ms"] + primary[f"{name}_us"] * 1e-3, 4)
        frames.append(rec)
        print(f"{sc.name:<22}{n_obj:>6} change + 1080p primary rays ms" + "".join(f"  {name} {rec[name + '_ms']:.4f}" for name in BUILDERS), flush=True)
    sb.write_records(a.out, "tools/bench_accel_build.py", changes, tail=dict(queries=queries, frames=frames), repeats=a.repeats,
                     unit="records: ms per rt_set_scene + rt_sync of a changed scene; queries: us per rt_trace_rays launch; frames: their sum, ms")
    sb.close_all(tracers.values())


if __name__ == "__main__":
    main()
