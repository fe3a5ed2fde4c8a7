#!/usr/bin/env python3
"""tools/bench_shade.py -- throughput of ray shading (rt_shade_rays, csrc/rt_shade.inc) against a VALU bound.

    python tools/bench_shade.py [--min-seconds 0.5] [--configs 2,4,5] [--json]

Scenes C2 (18 objects), C4 (64), C5 (256) of scenes.make_scene at full size and depth; three ray sets per scene:
  (a) coherent   = the 1920x1080 frame's primary rays (rt_camera_rays) shaded with pixels=None -- the same frame as
                   rt_render_to, which is timed in the same run, alternating launch by launch;
  (b) probe      = six 256x256 cube-face ray sets from the point (0, 2, -3) inside the scene, one launch per face;
  (c) incoherent = 2^21 seeded random rays (tools/bench_query.py's set), random pixel ids.
Per case: kernel time from HIP events around every launch on one side stream (after warm-up, repeated until at least
--min-seconds of kernel time), median and p10 / p90, Mrays/s (primary rays), and a VALU bound:
  rays x objects x 23 VALU instructions (the closest-hit cull block per object, counted in the ISA of the query kernels,
  DESIGN.md "Ray queries"; the shading kernel's object loops are the same code) / 64 lanes / the issue peak
  (1024 SIMDs x one wave64 VALU instruction per 2 cycles x 2.4 GHz, MI355X_MICROARCH.md).  For (a), `rays` is the
  oracle's ray count of the frame (every primary, bounce, shadow, PCSS-blocker and SSS ray, rt_count_rays); for (b) and
  (c) no oracle count exists, and `rays` is the primary rays alone, a loose lower bound.  The output is the ~40 B a ray
  stores (HBM bound < 0.01 ms for every case), so the VALU bound is the one that binds; `frac` = its time / the median.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

from bench_query import incoherent_rays  # noqa: E402
from opengl_raytracing_amd import host, scenes  # noqa: E402

VALU_PER_OBJECT = 23
ISSUE_PEAK = 1024 * 2.4e9 / 2                    # wave64 VALU instructions per second
PROBE_POINT = (0.0, 2.0, -3.0)
PROBE_SIZE = 256


def probe_faces(size=PROBE_SIZE, point=PROBE_POINT):
    """Six cube faces' rays (rt_ray rows) and pixel ids (face f's texel (i, j) -> (f * size + i, j))."""
    j, i = torch.meshgrid(torch.arange(size, device="cuda"), torch.arange(size, device="cuda"), indexing="ij")
    s = (i.float() + 0.5) / size * 2.0 - 1.0
    t = (j.float() + 0.5) / size * 2.0 - 1.0
    one = torch.ones_like(s)
    dirs = [(one, -t, -s), (-one, -t, s), (s, one, t), (s, -one, -t), (s, -t, one), (-s, -t, -one)]   # GL cube-map faces
    faces = []
    for f, (x, y, z) in enumerate(dirs):
        r = torch.zeros((size * size, 8), dtype=torch.float32, device="cuda")
        r[:, 0:3] = torch.tensor(point, device="cuda")
        r[:, 3] = 114514.0
        r[:, 4:7] = torch.stack([x, y, z], -1).reshape(-1, 3)
        px = torch.stack([i + f * size, j], -1).reshape(-1, 2).to(torch.int32)
        faces.append((r, px))
    return faces


def timed(launches, min_seconds, side):
    """launches: list of (name, fn(stream)); each is timed with HIP events, the list alternated until every entry has at
    least min_seconds of kernel time -> {name: stats}."""
    for _ in range(3):
        for _, fn in launches:
            fn(side)
    torch.cuda.synchronize()
    times = {name: [] for name, _ in launches}
    busy = torch.randn((4096, 4096), device="cuda")
    while min(sum(v) for v in times.values()) * 1e-3 < min_seconds or min(len(v) for v in times.values()) < 20:
        evs = []
        with torch.cuda.stream(side):
            busy = busy @ busy * 1e-3           # keeps the stream busy while the host queues the batch
        for _ in range(5):
            for name, fn in launches:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(side)
                fn(side)
                b.record(side)
                evs.append((name, a, b))
        torch.cuda.synchronize()
        for name, a, b in evs:
            times[name].append(a.elapsed_time(b))
    out = {}
    for name, ts in times.items():
        ts.sort()
        q = lambda f: ts[min(len(ts) - 1, int(f * len(ts)))]
        out[name] = dict(median_ms=statistics.median(ts), p10_ms=q(0.1), p90_ms=q(0.9), reps=len(ts))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--configs", default="2,4,5")
    ap.add_argument("--json", action="store_true", help="print one JSON line instead of the table")
    a = ap.parse_args()
    rows = []
    side = torch.cuda.Stream()
    with host.RayTracer(0) as rt:
        for cfg in (int(c) for c in a.configs.split(",")):
            sc = scenes.make_scene(cfg, host.generate_aabb)
            rt.load(sc)
            n_obj = len(sc.objects)
            p = sc.params()
            n_px = p.regionW * p.regionH
            with torch.cuda.stream(side):
                cam = rt.camera_rays(p, stream=side).reshape(-1, 8)
                col = torch.empty((n_px, 4), dtype=torch.float32, device="cuda")
                pos = torch.empty((n_px, 4), dtype=torch.float32, device="cuda")
                nrm = torch.empty((n_px, 4), dtype=torch.float16, device="cuda")
            side.synchronize()
            rays_ref = rt.count_rays(p)
            out = (col, pos, nrm)
            # (a) the same frame both ways, alternated
            t = timed([("shade", lambda s: rt.shade_rays(p, cam, out=out, stream=s)),
                       ("render", lambda s: rt.render_to(p, col.data_ptr(), pos.data_ptr(), nrm.data_ptr(), stream=s.cuda_stream))],
                      a.min_seconds, side)
            for name in ("shade", "render"):
                rows.append(dict(config=f"C{cfg}", objects=n_obj, case=f"(a) coherent, rt_{name}{'_rays' if name == 'shade' else '_to'}",
                                 n=n_px, rays_for_bound=rays_ref, **t[name]))
            # (b) a cube probe, six launches of 256x256
            faces = probe_faces()
            fout = [tuple(torch.empty((PROBE_SIZE * PROBE_SIZE, 4), dtype=dt, device="cuda")
                          for dt in (torch.float32, torch.float32, torch.float16)) for _ in faces]
            def probe(s):
                for (r, px), o in zip(faces, fout):
                    rt.shade_rays(p, r, pixels=px, out=o, stream=s)
            t = timed([("probe", probe)], a.min_seconds, side)
            rows.append(dict(config=f"C{cfg}", objects=n_obj, case="(b) probe, 6 x 256^2", n=6 * PROBE_SIZE ** 2,
                             rays_for_bound=6 * PROBE_SIZE ** 2, **t["probe"]))
            # (c) incoherent
            n = 1 << 21
            rr = incoherent_rays(n)
            px = torch.randint(0, 1 << 30, (n, 2), dtype=torch.int32, device="cuda")
            iout = tuple(torch.empty((n, 4), dtype=dt, device="cuda") for dt in (torch.float32, torch.float32, torch.float16))
            t = timed([("inc", lambda s: rt.shade_rays(p, rr, pixels=px, out=iout, stream=s))], a.min_seconds, side)
            rows.append(dict(config=f"C{cfg}", objects=n_obj, case="(c) incoherent, 2^21", n=n, rays_for_bound=n, **t["inc"]))
    for r in rows:
        s = r["median_ms"] * 1e-3
        t_valu = VALU_PER_OBJECT * r["objects"] * r["rays_for_bound"] / 64 / ISSUE_PEAK
        r.update(mrays_s=r["n"] / s / 1e6, valu_bound_ms=t_valu * 1e3, bound="valu", frac=t_valu / s)
    if a.json:
        print(json.dumps(dict(cases=rows)))
        return
    print(f"{'case':<40}{'median ms':>10}{'p10-p90 ms':>19}{'Mrays/s':>10}{'VALU ms':>9}  frac")
    for r in rows:
        print(f"{r['config'] + ' ' + r['case']:<40}{r['median_ms']:>10.4f}  {r['p10_ms']:>7.4f}-{r['p90_ms']:<8.4f}"
              f"{r['mrays_s']:>10.1f}{r['valu_bound_ms']:>9.4f}  {r['frac']:.2f}")
    print(json.dumps(dict(cases=rows)))


if __name__ == "__main__":
    main()
