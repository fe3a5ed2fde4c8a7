"""First-hit reuse A/B inside one process (DESIGN.md sections 26, 27 and 34): blocks of C2 frames in four arms -- `prefix` (the
default: reuse with settled tiles and prefix replay), `settled` (prefix replay off, rt_set_variant's bit 12), `on` (reuse without
either, bits 11 and 12) and `off` (no reuse, bit 10) -- alternate on one context, every frame between two events on the launch stream as in bench.py.  Then the two frames reuse could make
slower: the recording frame, and the frames of a camera that moves every frame with reuse on (which must never run anything but
the normal kernel).

  gain        the `on` frames' p90 lies below the `off` frames' p10; the `settled` frames' p90 below the `on` frames' p10; the
              `prefix` frames' p90 below the `settled` frames' p10
  regression  the moving camera's median with reuse on, and the recording frames' median, lie within the [min, max] of the same
              moving views rendered with reuse off (the recording frame is also held to the still view's off frames)

usage: python tools/bench_first_hit.py [--blocks 6] [--frames 100] [--warmup 20] [--cfg 2] [--out profiles/first_hit_bench.json]"""
import argparse, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stagebench as SB
import torch
from opengl_raytracing_amd import dist as D
from opengl_raytracing_amd import host, scenes, layout as L

OFF = 0x400
ARMS = {"prefix": 1, "settled": 1 | 0x1000, "on": 1 | 0x800 | 0x1000, "off": 1 | OFF}      # rt_set_variant's argument of each arm


def stats(ms):
    a = np.asarray(ms, dtype=np.float64)
    q = lambda x: round(float(np.percentile(a, x)), 4)
    return {"n": int(a.size), "min": round(float(a.min()), 4), "p10": q(10), "median": q(50), "p90": q(90), "max": round(float(a.max()), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cfg", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(SB.ROOT, "profiles", "first_hit_bench.json"))
    a = ap.parse_args()
    assert a.blocks >= 5, "at least five blocks each"

    sc = scenes.make_scene(a.cfg, host.generate_aabb)
    base = sc.params()
    rt = SB.tracer(None)
    rt.load(sc)
    stream = torch.cuda.Stream()
    one = D.StripPlan(sc.width, sc.height, sc.height, 1)
    col, pos, nrm = D.surface_views(D.alloc_rank_buffer(one, torch.device("cuda", 0)), one)

    def render(p):
        rt.render_to(p, col.data_ptr(), pos.data_ptr(), nrm.data_ptr(), stream=stream.cuda_stream)

    def timed(frames):
        """Every frame of `frames` between two events -> ms per frame."""
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(len(frames) + 1)]
        for e, p in zip(evs, frames):
            e.record(stream)
            render(p)
        evs[-1].record(stream)
        torch.cuda.synchronize()
        return [evs[i].elapsed_time(evs[i + 1]) for i in range(len(frames))]

    def counts():
        return rt.debug_first_hit()

    ms = {name: [] for name in ARMS}
    modes = {name: [] for name in ARMS}
    tiles = {name: [] for name in ARMS}
    prefixes = {name: [] for name in ARMS}
    for b in range(a.blocks):
        for name in SB.alternating(list(ARMS), b):
            rt.set_variant(ARMS[name])
            for _ in range(a.warmup):
                render(base)
            torch.cuda.synchronize()
            c0 = counts()
            ms[name] += timed([base] * a.frames)
            modes[name].append([x - y for x, y in zip(counts(), c0)])
            tiles[name].append(rt.debug_settled_tiles())
            prefixes[name].append(rt.debug_prefix_tiles())
    # the timed `prefix`, `settled` and `on` frames must all have replayed, the `off` frames all have run the normal kernel; only
    # the `prefix` and `settled` arms may have found settled tiles, the same ones, and must have found some; only the `prefix`
    # arm may resume a tile behind depth 0, and it must do so for some
    assert all(m == [0, 0, a.frames] for m in modes["prefix"] + modes["settled"] + modes["on"]), modes
    assert all(m == [a.frames, 0, 0] for m in modes["off"]), modes["off"]
    assert all(t[0] > 0 and t[1] > 0 for t in tiles["settled"]) and all(t[0] > 0 and t[1] == 0 for t in tiles["on"]), tiles
    assert tiles["prefix"] == tiles["settled"], tiles
    assert all(t == [0, 0] for t in tiles["off"]), tiles["off"]
    assert all(sum(h[2:]) > 0 for h in prefixes["prefix"]) and all(sum(h[2:]) == 0 for h in prefixes["settled"] + prefixes["on"] + prefixes["off"]), prefixes

    # a camera that moves every frame: the normal kernel only, with reuse on as with reuse off (the control: the same views)
    x0 = base.camPos[0]
    view = lambda k: L.copy_params(base, camPos=(x0 + 1e-3 * k, base.camPos[1], base.camPos[2]))
    moving_ms = {"on": [], "off": []}
    for b in range(4):
        for name in SB.alternating(["on", "off"], b):
            rt.set_variant(1 | (0 if name == "on" else OFF))
            c0 = counts()
            t = timed([view(1 + k) for k in range(a.warmup + a.frames)])
            assert [x - y for x, y in zip(counts(), c0)] == [a.warmup + a.frames, 0, 0]
            moving_ms[name] += t[a.warmup:]
    # stop and go: ten frames of motion, then the view stands for three -- the first of them records, the other two replay
    rt.set_variant(1)
    k = 1000
    before, recording, after = [], [], []
    c0 = counts()
    for cycle in range(12):
        path = [view(k + j) for j in range(10)]
        k += 10
        t = timed(path + [path[-1]] * 3)
        if cycle >= 2:
            before += t[5:10]                          # the normal frames right in front of the recording one
            recording.append(t[10])
            after += t[11:]
    dc = [x - y for x, y in zip(counts(), c0)]
    assert dc == [120, 12, 24], dc

    on, off, settled, prefix = stats(ms["on"]), stats(ms["off"]), stats(ms["settled"]), stats(ms["prefix"])
    mon, moff = stats(moving_ms["on"]), stats(moving_ms["off"])
    rec = {"config": f"C{a.cfg}", "size": [sc.width, sc.height], "blocks_each": a.blocks, "frames_per_block": a.frames, "warmup_per_block": a.warmup,
           "prefix_ms": prefix, "prefix_tiles_settled_then_k0_to_k7": prefixes["prefix"][0],
           "prefix_block_medians_ms": [round(float(np.median(ms["prefix"][i * a.frames:(i + 1) * a.frames])), 4) for i in range(a.blocks)],
           "gain_prefix_p90_below_settled_p10": bool(prefix["p90"] < settled["p10"]),
           "settled_ms": settled, "settled_tiles_of_window": tiles["settled"][0],
           "settled_block_medians_ms": [round(float(np.median(ms["settled"][i * a.frames:(i + 1) * a.frames])), 4) for i in range(a.blocks)],
           "gain_settled_p90_below_on_p10": bool(settled["p90"] < on["p10"]),
           "on_ms": on, "off_ms": off, "on_block_medians_ms": [round(float(np.median(ms["on"][i * a.frames:(i + 1) * a.frames])), 4) for i in range(a.blocks)],
           "off_block_medians_ms": [round(float(np.median(ms["off"][i * a.frames:(i + 1) * a.frames])), 4) for i in range(a.blocks)],
           "moving_camera_reuse_on_ms": mon, "moving_camera_reuse_off_ms": moff,
           "stop_and_go_normal_frames_before_recording_ms": stats(before), "recording_frame_ms": stats(recording),
           "replay_after_recording_ms": stats(after),
           "gain_on_p90_below_off_p10": bool(on["p90"] < off["p10"]),
           "moving_camera_within_off_spread": bool(moff["min"] <= mon["median"] <= moff["max"]),
           "recording_frame_within_off_spread": bool(moff["min"] <= stats(recording)["median"] <= moff["max"]),
           "recording_frame_within_still_view_off_spread": bool(off["min"] <= stats(recording)["median"] <= off["max"]),
           "note": "off spread = [min, max] of the reuse-off frames; the moving camera and the recording frame are held to the reuse-off "
                   "frames of the same moving views, the recording frame also to those of the still view"}
    SB.write_records(a.out, "tools/bench_first_hit.py", [rec], device=torch.cuda.get_device_name(0))
    for key in ("prefix_ms", "settled_ms", "on_ms", "off_ms", "moving_camera_reuse_on_ms", "moving_camera_reuse_off_ms", "stop_and_go_normal_frames_before_recording_ms",
                "recording_frame_ms", "replay_after_recording_ms"):
        print(f"{key:46s} {rec[key]}")
    print(f"{'settled_tiles_of_window':46s} {rec['settled_tiles_of_window']}")
    print(f"{'prefix_tiles_settled_then_k0_to_k7':46s} {rec['prefix_tiles_settled_then_k0_to_k7']}")
    for key in ("gain_prefix_p90_below_settled_p10", "gain_settled_p90_below_on_p10", "gain_on_p90_below_off_p10", "moving_camera_within_off_spread", "recording_frame_within_off_spread",
                "recording_frame_within_still_view_off_spread"):
        print(f"{key:46s} {rec[key]}")
    rt.close()


if __name__ == "__main__":
    main()
