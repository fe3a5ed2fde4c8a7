#!/usr/bin/env python3
"""Compare the gfx950 code of every kernel between two trees of this repository.

    tools/compare_asm.py OLD_TREE NEW_TREE [--keep DIR] [file.hip ...]

Each .hip file of csrc/ (all of them unless some are named) is compiled device-only to assembly with build.py's flags, from both
trees.  Per kernel symbol the instruction lines are compared with local labels renumbered, and the .amdhsa_ directives as they are;
the __hip_cuid_* symbol is ignored.  A kernel is reported as `identical`, as `reordered` (as many instructions of every mnemonic, in
another order or on other registers, with equal directives) or as `DIFFERENT`; for the last two the first and last differing line
are printed.  Exit status 1 when any kernel is DIFFERENT or exists on one side only."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opengl_raytracing_amd import build as B  # noqa: E402

LABEL = re.compile(r"\.LBB\d+_\d+|\.Ltmp\d+|\.LJTI\d+_\d+|\.Lfunc_\w+")


def assemble(tree, name, out):
    csrc = os.path.join(tree, "opengl_raytracing_amd", "csrc")
    flags = [f for f in B.HIPCC_FLAGS if f != "-shared"]
    subprocess.run([B._hipcc(), *flags, "-w", "-I", os.path.join(tree, "include"), "-I", csrc, "-x", "hip", "--cuda-device-only", "-S",
                    os.path.join(csrc, name), "-o", out], check=True)
    return open(out).read()


def kernels(asm):
    """{symbol: (instruction lines, .amdhsa_ directives)} of every kernel in one assembly file."""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    body, hsa, cur, desc = collections.defaultdict(list), collections.defaultdict(list), None, None
    for raw in asm.splitlines():
        line = raw.split(";")[0].strip()
        if not line:
            continue
        m = re.match(r"^(\w+):$", line)
        if m:
            cur = m.group(1) if m.group(1) in names else None
            continue
        if line.startswith(".amdhsa_kernel"):
            desc = line.split()[1]
        elif line.startswith(".end_amdhsa_kernel"):
            desc = None
        elif desc and line.startswith(".amdhsa_"):
            hsa[desc].append(" ".join(line.split()))
        elif cur and (line.startswith(".Lfunc_end") or line.startswith(".section")):
            cur = None
        elif cur and re.match(r"^\.L\w+:$", line):
            body[cur].append(line)                        # a local label: kept, renumbered below
        elif cur and not line.startswith("."):
            body[cur].append(" ".join(line.split()))
    out = {}
    for k in names:
        seen = {}
        text = [LABEL.sub(lambda m: seen.setdefault(m.group(0), f"L{len(seen)}"), ln) for ln in body[k]]
        out[k] = (text, hsa[k])
    return out


def mnemonics(lines):
    return collections.Counter(ln.split()[0] for ln in lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("files", nargs="*")
    ap.add_argument("--keep", help="directory that keeps the assembly files")
    a = ap.parse_intermixed_args()
    files = a.files or sorted(f for f in os.listdir(os.path.join(a.new, "opengl_raytracing_amd", "csrc")) if f.endswith(".hip"))
    keep = a.keep or tempfile.mkdtemp(prefix="compare_asm_")
    os.makedirs(keep, exist_ok=True)
    count = collections.Counter()
    for f in files:
        old, new = (kernels(assemble(t, f, os.path.join(keep, f"{side}_{f}.s"))) for side, t in (("old", a.old), ("new", a.new)))
        for k in sorted(set(old) | set(new)):
            if k not in old or k not in new:
                verdict = "ONLY IN " + ("new" if k in new else "old")
            elif old[k] == new[k]:
                verdict = "identical"
            elif old[k][1] == new[k][1] and mnemonics(old[k][0]) == mnemonics(new[k][0]):
                verdict = "reordered"
            else:
                verdict = "DIFFERENT"
            count[verdict] += 1
            if verdict != "identical":
                n = [len([ln for ln in side[k][0] if not ln.endswith(":")]) if k in side else 0 for side in (old, new)]
                print(f"{f}: {k}: {verdict} (instructions {n[0]} -> {n[1]}, directives {'equal' if old.get(k, (0, 0))[1] == new.get(k, (0, 1))[1] else 'differ'})")
                if k in old and k in new:
                    o, w = old[k][0], new[k][0]
                    bad = [i for i in range(max(len(o), len(w))) if i >= len(o) or i >= len(w) or o[i] != w[i]]
                    if bad:
                        print(f"    lines {bad[0] + 1}..{bad[-1] + 1} of {len(o)} -> {len(w)} differ")
    print(f"{sum(count.values())} kernels in {len(files)} files:", ", ".join(f"{v} {k}" for k, v in sorted(count.items())))
    return 1 if any(k not in ("identical", "reordered") for k in count) else 0


if __name__ == "__main__":
    sys.exit(main())
