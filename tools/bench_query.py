#!/usr/bin/env python3
"""tools/bench_query.py -- throughput of the ray queries (rt_trace_rays, csrc/rt_query.inc) against their two bounds.

    python tools/bench_query.py [--min-seconds 0.5] [--json]

Scenes C2 (18 objects), C4 (64), C5 (256) of scenes.make_scene; two ray sets per scene:
  coherent   = the primary rays of the 1920x1080 frame (rt_camera_rays of the scene's camera);
  incoherent = 2^22 seeded random rays: origins uniform in [-20, 20]^3, isotropic directions, tMax 114514.
Both modes (closest, any).  Per case: kernel time from HIP events around every launch (after warm-up, repeated until at
least --min-seconds of kernel time), median and p10 / p90, Grays/s, and two bounds:
  VALU: VALU instructions per object of the cull block every ray pays (counted in the ISA of rt_trace_rays_kernel,
        hipcc --save-temps, DESIGN.md "Ray queries") x objects x rays / 64 lanes / the issue peak
        (1024 SIMDs x one wave64 VALU instruction per 2 cycles x 2.4 GHz, MI355X_MICROARCH.md);
  HBM:  64 B per closest ray (32 in, 32 out) or 36 B per any ray (32 in, 4 out) / 8 TB/s peak (6.3 achievable).
The larger bound binds; `frac` = that bound's time / the measured median.  Also rt_pick's host round trip (us).
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from opengl_raytracing_amd import host, scenes  # noqa: E402

VALU_PER_OBJECT = {"closest": 23, "any": 27}     # cull block (+ the any-hit loop's resolved-lane test and ballot)
ISSUE_PEAK = 1024 * 2.4e9 / 2                    # wave64 VALU instructions per second
HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12
BYTES_PER_RAY = {"closest": 64, "any": 36}


def incoherent_rays(n, seed=0x51ED):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    r = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    r[:, 0:3] = torch.rand((n, 3), generator=g, device="cuda") * 40.0 - 20.0
    d = torch.randn((n, 3), generator=g, device="cuda")
    r[:, 4:7] = d / d.norm(dim=1, keepdim=True)
    r[:, 3] = 114514.0
    return r


def time_query(rt, rays, mode, min_seconds):
    """Launches and events on one side stream: the query runs on it directly (torch's default stream would add the
    event fences RayTracer puts around a launch it has to move to the context's stream)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        return _time_query(rt, rays, mode, min_seconds, side)


def _time_query(rt, rays, mode, min_seconds, side):
    out = (torch.empty((rays.shape[0], 8), dtype=torch.float32, device="cuda") if mode == "closest"
           else torch.empty(rays.shape[0], dtype=torch.int32, device="cuda"))
    for _ in range(5):
        rt.trace_rays(rays, mode, out=out, stream=side)
    torch.cuda.synchronize()
    times, total = [], 0.0
    busy = torch.randn((4096, 4096), device="cuda")
    while total < min_seconds or len(times) < 20:
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(10)]
        busy = busy @ busy * 1e-3               # ~1 ms on the stream while the host queues the batch: no launch gap inside a pair
        for a, b in evs:
            a.record(side)
            rt.trace_rays(rays, mode, out=out, stream=side)
            b.record(side)
        torch.cuda.synchronize()
        for a, b in evs:
            ms = a.elapsed_time(b)
            times.append(ms)
            total += ms * 1e-3
    times.sort()
    q = lambda f: times[min(len(times) - 1, int(f * len(times)))]
    return dict(median_ms=statistics.median(times), p10_ms=q(0.1), p90_ms=q(0.9), reps=len(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--json", action="store_true", help="print one JSON line instead of the table")
    a = ap.parse_args()
    rows = []
    with host.RayTracer(0) as rt:
        for cfg in (2, 4, 5):
            sc = scenes.make_scene(cfg, host.generate_aabb)
            rt.load(sc)
            n_obj = len(sc.objects)
            sets = {"coherent": rt.camera_rays(sc.params(width=1920, height=1080)).reshape(-1, 8),
                    "incoherent": incoherent_rays(1 << 22)}
            for name, rays in sets.items():
                n = rays.shape[0]
                for mode in ("closest", "any"):
                    t = time_query(rt, rays, mode, a.min_seconds)
                    s = t["median_ms"] * 1e-3
                    t_valu = VALU_PER_OBJECT[mode] * n_obj * n / 64 / ISSUE_PEAK
                    t_hbm = BYTES_PER_RAY[mode] * n / HBM_PEAK
                    bound = "valu" if t_valu >= t_hbm else "hbm"
                    rows.append(dict(config=f"C{cfg}", objects=n_obj, rays=name, n=n, mode=mode, **t, grays_s=n / s / 1e9,
                                     valu_bound_ms=t_valu * 1e3, hbm_bound_ms=t_hbm * 1e3,
                                     hbm_achievable_ms=BYTES_PER_RAY[mode] * n / HBM_ACHIEVABLE * 1e3,
                                     bound=bound, frac=max(t_valu, t_hbm) / s))
        sc = scenes.make_scene(2, host.generate_aabb)
        rt.load(sc)
        p = sc.params()
        for _ in range(20):
            rt.pick(p, 960, 540)
        us = []
        rng = np.random.default_rng(3)
        for x, y in zip(rng.integers(0, 1920, 400), rng.integers(0, 1080, 400)):
            t0 = time.perf_counter()
            rt.pick(p, int(x), int(y))
            us.append((time.perf_counter() - t0) * 1e6)
        pick = dict(median_us=statistics.median(us), p10_us=sorted(us)[40], p90_us=sorted(us)[360])
    if a.json:
        print(json.dumps(dict(cases=rows, pick=pick)))
        return
    print(f"{'case':<28}{'median ms':>10}{'p10-p90 ms':>17}{'Grays/s':>9}{'VALU ms':>9}{'HBM ms':>9}  bound  frac")
    for r in rows:
        print(f"{r['config'] + ' ' + r['rays'] + ' ' + r['mode']:<28}{r['median_ms']:>10.4f}"
              f"{r['p10_ms']:>8.4f}-{r['p90_ms']:<8.4f}{r['grays_s']:>9.2f}{r['valu_bound_ms']:>9.4f}{r['hbm_bound_ms']:>9.4f}"
              f"  {r['bound']:<5}  {r['frac']:.2f}")
    print(f"rt_pick round trip: median {pick['median_us']:.1f} us (p10 {pick['p10_us']:.1f}, p90 {pick['p90_us']:.1f})")
    print(json.dumps(dict(cases=rows, pick=pick)))


if __name__ == "__main__":
    main()
