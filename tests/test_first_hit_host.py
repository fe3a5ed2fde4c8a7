"""CPU-only test of the first-hit reuse policy (csrc/rt_firsthit.h, which holds no HIP type): which launches run as normal
frames, which record their first hits and which replay them.  A stand-alone C++ program with its own main includes that header
alone, replays a script of launches, invalidations and switches and prints the mode of every launch; the test compares the
print-out with a restatement of the policy in Python.  No GPU call is made.

A launch is `L <view> <frameCount> <window>`: three small integers that stand for "every rt_params field but frameCount", the
frameCount and the window size.  The other steps: `S` = rt_set_scene with changed bytes, `I` = rt_set_scene with identical bytes
(nothing happens), `N 1|0` = rt_set_noise with / without a texture, `K` = rt_set_skybox, `V <low byte>` = rt_set_variant of
the low byte, `O 1|0` = the off switch (bit 10) cleared / set, `F` = a launch that fails or is refused, `A <pixels>` = from now
on a record buffer of that many pixels or more cannot be allocated."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "opengl_raytracing_amd", "csrc")
INCLUDE = os.path.join(REPO, "include")

PROGRAM = r"""
#include "rt_firsthit.h"
#include <stdio.h>
#include <stdlib.h>

int main(int argc, char **argv) {
    RtFirstHit fh;
    uint32_t sceneGen = 0, texGen = 0;
    int variant = 1;
    bool noise = false, sky = false;
    unsigned long long allocLimit = ~0ull;
    static const char *const names[3] = {"normal", "record", "replay"};
    for (int k = 1; k < argc;) {
        const char op = argv[k++][0];
        auto arg = [&]() -> long { return k < argc ? strtol(argv[k++], nullptr, 10) : 0; };
        if (op == 'L') {
            const long view = arg(), fc = arg(), win = arg();
            rt_params p;
            memset(&p, 0xA5, sizeof p);                    // whatever the caller's padding holds must not matter
            for (int i = 0; i < 3; i++) { p.camPos[i] = (float)view; p.camDir[i] = 0.0f; p.camUp[i] = 1.0f; p.camRight[i] = 0.5f; }
            p.fovDeg = 45.0f; p.focalLength = 1.0f; p.maxRayDistance = 114514.0f; p.noiseScale[0] = p.noiseScale[1] = 1.0f / 1024.0f;
            p.frameCount = (int32_t)fc; p.useSkybox = 0; p.maxRayDepth = 4; p.width = 1920; p.height = 1080;
            p.x0 = p.y0 = 0; p.regionW = (int32_t)win; p.regionH = 1;
            p.stripRows = 1; p.stripCount = 1; p.stripIndex = 0; p.reserved0 = 0; p.stripCycleRows = 0; p.stripOffsetRows = 0;
            RtFirstHit::Mode m = RtFirstHit::NORMAL;
            if (variant == 1 && fh.on()) {                  // as rt_abi.cpp's launch does
                const RtFirstHitKey key = rt_first_hit_key(sceneGen, texGen, 18, 3, variant, noise, sky, p);
                m = fh.decide(key);
                if (m == RtFirstHit::RECORD && (unsigned long long)win >= allocLimit) { fh.refuse(key); m = RtFirstHit::NORMAL; }
                fh.launched(m, key);
            } else if (variant == 1) {
                fh.counts[0]++;
            }
            printf("L %ld %ld %ld -> %s\n", view, fc, win, variant == 1 ? names[m] : "exhaustive");
        } else if (op == 'S') { sceneGen++; fh.invalidate(); printf("S\n"); }
        else if (op == 'I') { printf("I\n"); }
        else if (op == 'N') { noise = arg() != 0; texGen++; fh.invalidate(); printf("N\n"); }
        else if (op == 'K') { sky = !sky; texGen++; fh.invalidate(); printf("K\n"); }
        else if (op == 'V') {
            const int v = (int)arg();
            if (v != variant) fh.invalidate();
            variant = v;
            printf("V\n");
        } else if (op == 'O') {
            const bool on = arg() != 0;
            if (on != fh.variantOn) fh.invalidate();
            fh.variantOn = on;
            printf("O\n");
        } else if (op == 'F') { fh.invalidate(); printf("F\n"); }
        else if (op == 'A') { allocLimit = (unsigned long long)arg(); printf("A\n"); }
        else return 2;
    }
    printf("counts %llu %llu %llu\n", (unsigned long long)fh.counts[0], (unsigned long long)fh.counts[1], (unsigned long long)fh.counts[2]);
    return 0;
}
"""

MAX_PIXELS = 1 << 24


def model(script):
    """The policy in terms of what a frame's depth 0 depends on.  `state` is everything but frameCount; frameCount joins it
    only while a noise texture is loaded.  cache = the inputs of the recorded frame (None: no valid records), last = the inputs
    of the previous launch (None after anything that invalidates)."""
    gen, noise, sky, variant, on, limit = 0, False, False, 1, True, None
    cache = last = refused = None
    counts, out = [0, 0, 0], []
    for step in script:
        op, a = step[0], step[1:]
        if op == "L":
            view, fc, win = a
            if variant != 1:
                out.append(f"L {view} {fc} {win} -> exhaustive")
                continue
            mode = "normal"
            if on:
                inputs = (gen, noise, sky, view, win, fc if noise else 0)
                if cache == inputs:
                    mode = "replay"
                else:
                    cache = None                    # another view: the records are of no use any more
                    too_large = win > MAX_PIXELS or (refused is not None and win >= refused)
                    if last == inputs and not too_large:
                        if limit is not None and win >= limit:
                            refused = win           # no buffer: a normal frame, and no further attempt at that size
                        else:
                            mode, cache = "record", inputs
                last = inputs
            counts[["normal", "record", "replay"].index(mode)] += 1
            out.append(f"L {view} {fc} {win} -> {mode}")
            continue
        if op == "S":
            gen += 1
        elif op == "N":
            noise, gen = bool(a[0]), gen + 1
        elif op == "K":
            sky, gen = not sky, gen + 1
        elif op == "V":
            if a[0] == variant:
                out.append(op)
                continue
            variant = a[0]
        elif op == "O":
            if bool(a[0]) == on:
                out.append(op)
                continue
            on = bool(a[0])
        elif op == "A":
            limit = a[0]
            out.append(op)
            continue
        elif op == "I":
            out.append(op)
            continue
        cache = last = None                          # S, N, K, F and an effective V / O invalidate
        out.append(op)
    out.append("counts %d %d %d" % tuple(counts))
    return out


def frames(view, n, win=64, fc=0, step=0):
    return [("L", view, fc + k * step, win) for k in range(n)]


# four identical frames: normal, record, replay, replay; an advancing frameCount without noise replays all the same
SCRIPT = frames(1, 4) + frames(1, 3, fc=5, step=1)
# a camera that moves every frame never leaves the normal kernel; standing still again records on the second frame
SCRIPT += frames(2, 1) + frames(3, 1) + frames(4, 1) + frames(4, 2) + frames(5, 1) + frames(4, 3)
# another window is another frame; going back to the first window starts over (one buffer)
SCRIPT += frames(4, 3, win=32) + frames(4, 3, win=64)
# changed scene bytes invalidate, identical bytes do not
SCRIPT += [("S",)] + frames(4, 3) + [("I",)] + frames(4, 2)
# with a noise texture frameCount is an input: no replay across values, repeated values replay
SCRIPT += [("N", 1)] + frames(4, 4, fc=0, step=1) + frames(4, 3, fc=9) + frames(4, 1, fc=10) + frames(4, 1, fc=9) + frames(4, 2, fc=9)
SCRIPT += [("N", 0)] + frames(4, 3, fc=0, step=1) + [("K",)] + frames(4, 3) + [("K",)] + frames(4, 3)
# the exhaustive kernel and back; the off switch and back; the same value again changes nothing
SCRIPT += [("V", 0)] + frames(4, 2) + [("V", 1)] + frames(4, 3) + [("V", 1)] + frames(4, 1)
SCRIPT += [("O", 0)] + frames(4, 3) + [("O", 1)] + frames(4, 3) + [("O", 1)] + frames(4, 1)
# a failed or refused launch in between
SCRIPT += [("F",)] + frames(4, 3) + frames(6, 2) + [("F",)] + frames(6, 3)
# the cap
SCRIPT += frames(8, 3, win=MAX_PIXELS) + frames(8, 3, win=MAX_PIXELS + 1)
# no buffer to be had: normal frames, silently, for windows that large (also once memory is back); smaller ones still record
SCRIPT += [("A", 100)] + frames(7, 4, win=128) + frames(7, 3, win=99) + frames(7, 3, win=100) + [("A", 1 << 30)] + frames(7, 3, win=128)


def test_model_covers_what_the_script_is_for():
    out = model(SCRIPT)
    modes = [ln.split(" -> ")[1] for ln in out if " -> " in ln]
    assert modes[:7] == ["normal", "record", "replay", "replay", "replay", "replay", "replay"]
    assert modes[7:12] == ["normal", "normal", "normal", "record", "replay"] and modes[12:16] == ["normal", "normal", "record", "replay"]
    assert {"normal", "record", "replay", "exhaustive"} == set(modes)
    noise_at = out.index("N")
    assert [ln.split(" -> ")[1] for ln in out[noise_at + 1: noise_at + 5]] == ["normal"] * 4          # frameCount advancing under noise
    assert [ln.split(" -> ")[1] for ln in out[noise_at + 5: noise_at + 8]] == ["normal", "record", "replay"]
    of_view = lambda v: [ln.split(" -> ")[1] for ln in out if ln.startswith(f"L {v} ")]
    assert of_view(8) == ["normal", "record", "replay", "normal", "normal", "normal"]                 # at the cap, one pixel above it
    assert of_view(7) == ["normal"] * 4 + ["normal", "record", "replay"] + ["normal"] * 6             # 128 refused, 99 fits, 100 and 128 not tried


def test_policy_matches_the_model(tmp_path):
    src = tmp_path / "firsthit.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "firsthit"
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-I", INCLUDE, str(src), "-o", str(exe)]
    sanitized = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True)
    if sanitized.returncode != 0:              # a compiler without the sanitizers' runtimes: the same program without them
        subprocess.run(base, check=True)
    args = [str(x) for step in SCRIPT for x in step]
    run = subprocess.run([str(exe), *args], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    got, want = run.stdout.splitlines(), model(SCRIPT)
    assert len(got) == len(want) == len(SCRIPT) + 1
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"step {k} {SCRIPT[k] if k < len(SCRIPT) else 'counts'}: rt_firsthit.h says {g!r}, the model {w!r}"
