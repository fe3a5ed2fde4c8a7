"""Secondary measurement (not the BASELINE metric): what first-hit-guided upsampling costs and where it pays, at 2 x per axis, in one run:

  (i)   rt_upsample (reconstruct + scan + emit) from device events over back-to-back launches at 960x540 -> 1920x1080 and 1920x1080 ->
        3840x2160 on C2's frame and first hits, beside a device copy that moves the call's compulsory bytes -- 32 per output pixel
        read (the rt_hit) plus 16 written -- in the same run: the ratio.  The hole and orphan shares of C2, C3 and C4 at both sizes.
  (ii)  the stages of one frame of the loop from device events, per scene and size: the low render, the first hits at both sizes, the
        upsample, the re-shade of the listed holes (rt_camera_rays_at + rt_shade_rays + rt_image_put_at), the re-shade of EVERY pixel
        (the slope of the loop's cost in the hole share) and rt_render_to at full resolution.  The hole share at which the loop costs
        what the full render costs is the crossover: (full - fixed) / reshade_all with fixed = low + hits + upsample.
  (iii) the whole loop against rt_render_to(pHigh) alone on a host clock, the camera moving every frame, alternated; the loop waits
        once per frame for its 8-byte read of nSelected / nListed, the full render once per batch of frames.  With --parent-lib the
        parent build's full render is alternated with them on the same card.  The low render has a context of its own (two sizes
        alternating in one context make the packet kernel's tile scheduler start over every frame), as a host of the loop would.

Writes one record per scene to --out (default profiles/upsample_bench.json)."""
import argparse, ctypes, json
import stagebench as sb                                         # (puts the repository on sys.path)
import numpy as np
import torch
from opengl_raytracing_amd import host, scenes
from opengl_raytracing_amd import layout as L

ap = argparse.ArgumentParser()
sb.add_common_args(ap, "upsample_bench.json", launches=20, variant_macros="RT_UPSAMPLE_")
ap.add_argument("--scenes", default="2,3,4", help="BASELINE configs to measure (default 2,3,4)")
ap.add_argument("--min-weight", type=float, default=L.UPSAMPLE_DEFAULTS["min_weight"])
ap.add_argument("--skip-4k", action="store_true")
ap.add_argument("--skip-loops", action="store_true", help="(i) only: no stages of the loop, no loops")
args = ap.parse_args()
WARM = 3
SIZES = [((960, 540), (1920, 1080))] + ([] if args.skip_4k else [((1920, 1080), (3840, 2160))])
POWER = L.UPSAMPLE_DEFAULTS["normal_log2_power"]

new, old, builds = sb.open_tracers(args.parent_lib, sb.parse_variants(args.variant))
low_ctx = sb.tracer(None)                                       # the low render's own context: the packet kernel's tile scheduler learns per context and size
side = sb.side()
ptr = host._dev_ptr


class Frame:
    """The buffers of one (low, high) pair of sizes and the stages of the loop on them, each a launch on side()."""

    def __init__(self, t, t_low, scene, low, high):
        self.t, self.t_low, self.scene = t, t_low, scene
        (self.lw, self.lh), (self.w, self.h) = low, high
        f32 = dict(dtype=torch.float32, device="cuda")
        nl, nh = self.lw * self.lh, self.w * self.h
        self.low, self.out, self.full = torch.zeros((nl, 4), **f32), torch.zeros((nh, 4), **f32), torch.zeros((nh, 4), **f32)
        self.pos, self.nrm = torch.zeros((nh, 4), **f32), torch.zeros((nh, 4), dtype=torch.float16, device="cuda")
        self.rays, self.hits_low, self.hits_high = torch.zeros((nh, 8), **f32), torch.zeros((nl, 8), **f32), torch.zeros((nh, 8), **f32)
        self.samples = torch.zeros((nh, 4), **f32)
        self.pixels, self.scratch, self.sel = t.accum_select_alloc(self.w, self.h, nh)
        self.counts = torch.zeros(2, dtype=torch.int32).pin_memory()
        self.k = 0
        self.move()

    def move(self):
        """The next frame's view: the camera a step further along x, the frame count moving."""
        self.k += 1
        self.scene.frame_count = self.k
        self.p_low, self.p_high = self.scene.params(width=self.lw, height=self.lh), self.scene.params(width=self.w, height=self.h)
        for p in (self.p_low, self.p_high):
            p.camPos[0] += 0.01 * (self.k % 64)

    def render_low(self):
        self.t_low.render_to(self.p_low, self.low.data_ptr(), self.pos.data_ptr(), self.nrm.data_ptr(), stream=side.cuda_stream)

    def render_full(self, t=None):
        (t or self.t).render_to(self.p_high, self.full.data_ptr(), self.pos.data_ptr(), self.nrm.data_ptr(), stream=side.cuda_stream)

    def first_hits(self, p, hits):
        self.t._launch(side, "rt_camera_rays", ctypes.byref(p), ptr(self.rays))
        self.t._launch(side, "rt_trace_rays", ptr(self.rays), p.width * p.height, L.QUERY_CLOSEST, ptr(hits))

    def hits_both(self):
        self.first_hits(self.p_low, self.hits_low)
        self.first_hits(self.p_high, self.hits_high)

    def upsample(self):
        self.t.upsample(self.low, self.hits_low, self.hits_high, self.out, self.pixels, self.w * self.h, self.scratch, self.sel, self.w, self.h,
                        self.lw, self.lh, normal_log2_power=POWER, min_weight=args.min_weight, stream=side)

    def read_counts(self):
        """The loop's 8-byte read: (nSelected, nListed).  Waits for side()."""
        with torch.cuda.stream(side):
            self.counts.copy_(self.sel[L.SELECT_NSELECTED_OFFSET: L.SELECT_NSELECTED_OFFSET + 8].view(torch.int32), non_blocking=True)
        side.synchronize()
        return int(self.counts[0]), int(self.counts[1])

    def reshade(self, n, pixels=None):
        if not n:
            return
        pixels = self.pixels if pixels is None else pixels
        self.t.camera_rays_at(self.p_high, pixels, n, out=self.rays, stream=side)
        self.t.shade_rays(self.p_high, self.rays[:n], pixels=pixels[:n], out=(self.samples[:n], None, None), stream=side, position=False, normal=False)
        self.t.image_put_at(self.samples, pixels, n, self.out, self.w, self.h, stream=side)

    def loop_frame(self):
        self.move()
        self.render_low()
        self.hits_both()
        self.upsample()
        self.reshade(self.read_counts()[1])


def every_pixel(w, h):
    """Every pixel of the image in the list's order, as the int32 [n, 2] tensor the re-shade takes."""
    ty, tx = np.meshgrid(np.arange(0, h, 8), np.arange(0, w, 8), indexing="ij")
    out = []
    for y0, x0 in zip(ty.reshape(-1), tx.reshape(-1)):
        yy, xx = np.meshgrid(np.arange(y0, min(y0 + 8, h)), np.arange(x0, min(x0 + 8, w)), indexing="ij")
        out.append(np.stack([xx.reshape(-1), yy.reshape(-1)], axis=-1))
    return torch.from_numpy(np.concatenate(out).astype(np.int32)).cuda()


records = []
for cfg in [int(c) for c in args.scenes.split(",")]:
    scene = scenes.make_scene(cfg, host.generate_aabb)
    for t in sb.distinct([new, old, low_ctx, *builds.values()]):
        t.load(scene)
    rec = {"scene": f"C{cfg}", "repeats": args.repeats, "launches": args.launches, "min_weight": args.min_weight, "normal_log2_power": POWER, "sizes": []}
    for low, high in SIZES:
        f = Frame(new, low_ctx, scene, low, high)
        npx = high[0] * high[1]
        with torch.cuda.stream(side):
            f.render_low()
            f.hits_both()
            f.upsample()
        n_holes, n = f.read_counts()
        st = f.sel.cpu().numpy().view(L.SELECT_STATE_DTYPE)[0]
        row = {"low": list(low), "high": list(high), "holes": n_holes, "hole_share": round(n_holes / npx, 5), "orphans": int(st["nCapped"]),
               "orphan_share": round(int(st["nCapped"]) / npx, 5)}
        launches = {"upsample": f.upsample}
        for name, vt in builds.items():                         # the same call through a library built with other RT_UPSAMPLE_* macros
            if vt is not new:
                launches[f"upsample_{name}"] = lambda vt=vt: vt.upsample(
                    f.low, f.hits_low, f.hits_high, f.out, f.pixels, npx, f.scratch, f.sel, f.w, f.h, f.lw, f.lh, normal_log2_power=POWER,
                    min_weight=args.min_weight, stream=side)
        if cfg == 2:
            src = torch.zeros(24 * npx, dtype=torch.uint8, device="cuda")          # 24 B read + 24 B written per pixel: the 48 compulsory ones
            dst = torch.empty_like(src)
            launches["copy"] = lambda: dst.copy_(src)
        if not args.skip_loops:
            all_pixels = every_pixel(*high)
            launches.update({"render_low": f.render_low, "first_hits_low": lambda: f.first_hits(f.p_low, f.hits_low),
                             "first_hits_high": lambda: f.first_hits(f.p_high, f.hits_high), "reshade_holes": lambda: f.reshade(n),
                             "reshade_all": lambda: f.reshade(npx, all_pixels), "render_full": f.render_full})
        with torch.cuda.stream(side):
            us = sb.alternate(launches, args.launches if cfg < 4 else max(2, args.launches // 5), args.repeats, WARM)
        for key, v in us.items():
            sb.summarise(row, key, v, "us")
        row["compulsory_bytes"] = 48 * npx
        row["upsample_gbps"] = round(48 * npx / row["upsample_us"] / 1e3, 1)
        if "copy_us" in row:
            row["upsample_over_copy"] = round(row["upsample_us"] / row["copy_us"], 3)
        if not args.skip_loops:
            fixed = row["render_low_us"] + row["first_hits_low_us"] + row["first_hits_high_us"] + row["upsample_us"]
            row["loop_fixed_us"] = round(fixed, 2)
            row["loop_device_us"] = round(fixed + row["reshade_holes_us"], 2)
            row["loop_over_full_device"] = round(row["loop_device_us"] / row["render_full_us"], 3)
            row["crossover_hole_share"] = round((row["render_full_us"] - fixed) / row["reshade_all_us"], 4)

            def loop(k):
                with torch.cuda.stream(side):
                    for _ in range(k):
                        f.loop_frame()
                side.synchronize()

            def full(k, t=new):
                with torch.cuda.stream(side):
                    for _ in range(k):
                        f.move()
                        f.render_full(t)
                side.synchronize()

            loops = {"loop": loop, "full": full}
            if old is not new:
                loops["full_parent"] = lambda k: full(k, old)
            for key, v in sb.time_host_loops(loops, args.frames if cfg < 4 else max(10, args.frames // 4), args.repeats).items():
                sb.summarise(row, key + "_frame", v, "ms")
            row["loop_over_full_host"] = round(row["loop_frame_ms"] / row["full_frame_ms"], 3)
        rec["sizes"].append(row)
        print(json.dumps({"scene": rec["scene"], **row}), flush=True)
        del f
    records.append(rec)

sb.write_records(args.out, "tools/bench_upsample.py", records)
sb.close_all([new, old, low_ctx, *builds.values()])
