#!/usr/bin/env python3
"""Condense rocprofv3 csv output (run_profile.sh) into small committed summaries:
<prefix>_kernel_stats.csv (per-kernel count / avg / total from the kernel trace) and
<prefix>_pmc.json (per-kernel mean of every counter collected, per dispatch)."""
import csv
import glob
import json
import os
import sys
from collections import defaultdict


def main(src, prefix):
    def newest(pattern):
        """gpurun MERGES output directories: keep only the most recent file of each rocprofv3 output directory."""
        by_dir = defaultdict(list)
        for f in glob.glob(pattern, recursive=True):
            by_dir[os.path.dirname(f)].append(f)
        return [max(fs, key=os.path.getmtime) for fs in by_dir.values()]

    stats = defaultdict(lambda: [0, 0.0, 1e30, 0.0])
    for f in newest(os.path.join(src, "trace", "**", "*kernel_trace.csv")):
        for row in csv.DictReader(open(f)):
            name = row.get("Kernel_Name", "?")
            dur = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
            s = stats[name]
            s[0] += 1; s[1] += dur; s[2] = min(s[2], dur); s[3] = max(s[3], dur)
            s.append(None) if False else None
            stats[name + "|meta"] = [row.get("VGPR_Count", ""), row.get("SGPR_Count", ""), row.get("LDS_Block_Size", ""),
                                     row.get("Workgroup_Size", row.get("Workgroup_Size_X", "")), row.get("Grid_Size", row.get("Grid_Size_X", ""))]
    with open(prefix + "_kernel_stats.csv", "w") as out:
        out.write("kernel,calls,avg_us,min_us,max_us,total_us,vgpr,sgpr,lds_bytes,workgroup,grid\n")
        for name, s in sorted(((k, v) for k, v in stats.items() if not k.endswith("|meta")), key=lambda kv: -kv[1][1]):
            meta = stats.get(name + "|meta", [""] * 5)
            out.write(f"\"{name}\",{s[0]},{s[1] / s[0]:.3f},{s[2]:.3f},{s[3]:.3f},{s[1]:.1f},{','.join(str(m) for m in meta)}\n")
    pmc = defaultdict(lambda: defaultdict(list))
    for f in newest(os.path.join(src, "pmc_*", "**", "*counter_collection.csv")):
        for row in csv.DictReader(open(f)):
            pmc[row.get("Kernel_Name", "?")][row["Counter_Name"]].append(float(row["Counter_Value"]))
    res = {k: {c: {"mean": sum(v) / len(v), "n": len(v)} for c, v in cs.items()} for k, cs in pmc.items()}
    json.dump(res, open(prefix + "_pmc.json", "w"), indent=1, sort_keys=True)
    print("wrote", prefix + "_kernel_stats.csv", prefix + "_pmc.json")
    # Per-launch counters of the dominant render kernel for bench.py (roofline / hbm_physical):
    # profiles/kernel_counters.json[cN].  HBM bytes = (2*FETCH_SIZE + WRITE_SIZE) KB -- MI355X_MICROARCH.md:
    # FETCH_SIZE counts 64 B per 128-B request on gfx950 (exact for wide streaming reads, an upper bound
    # otherwise); WRITE_SIZE exact.  src_hash ties the record to the kernel sources it was measured on.
    cfg = os.environ.get("RT_PROFILE_CFG", "c2")
    if os.environ.get("RT_PROFILE_PROG", "bench.py") != "bench.py":
        return      # a secondary chain was profiled: the render kernel's launches there are not bench.py's workload
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        from bench import kernel_source_hash
        src_hash = kernel_source_hash()
    except Exception:
        src_hash = None
    # A run holds several render kernels: the instrumented launches in front, one normal and one recording frame, then the
    # first-hit replays the timed frames run.  The dominant one is the one dispatched most often.
    for k, cs in sorted(res.items(), key=lambda kv: -kv[1].get("SQ_INSTS_VALU", {}).get("n", 0)):
        if ("render_packet_kernel<0" in k or "render_packet_kernel<false" in k or "render_kernel<0" in k) and "SQ_INSTS_VALU" in cs:
            tpath = os.path.join(os.path.dirname(prefix), "kernel_counters.json")
            t = json.load(open(tpath)) if os.path.exists(tpath) else {}
            rec = {c: v["mean"] for c, v in cs.items()}
            rec.update({"fetch_size_kb": cs.get("FETCH_SIZE", {}).get("mean"), "write_size_kb": cs.get("WRITE_SIZE", {}).get("mean"),
                        "kernel": (k[:k.index(">(") + 1] if ">(" in k else k.split("(")[0]), "source": os.path.basename(prefix) + "_pmc.json", "src_hash": src_hash})
            st = stats.get(k)
            if st:
                rec["kernel_avg_us"] = round(st[1] / st[0], 3)
                rec["kernel_calls"] = st[0]
            if rec["fetch_size_kb"] is not None and rec["write_size_kb"] is not None:
                rec["hbm_bytes_per_launch"] = int((2 * rec["fetch_size_kb"] + rec["write_size_kb"]) * 1024)
            t[cfg] = rec
            json.dump(t, open(tpath, "w"), indent=1, sort_keys=True)
            print("wrote", tpath, cfg)
            break


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
