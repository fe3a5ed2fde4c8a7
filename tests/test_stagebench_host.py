"""tools/stagebench.py, the measurement procedure the stage benchmarks share: the parts that need no device (the order of the
repeats, the warm-up, the host clock, the record keys and the file), tracer()'s clean-up, and that every tool still parses its
arguments before it opens a device."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = ["accum", "denoise", "meter", "present", "reproject", "resample", "yuv"]


@pytest.fixture(scope="module")
def sb():
    """tools/ is not a package and is kept out of collection: the module is loaded by its path."""
    spec = importlib.util.spec_from_file_location("stagebench", os.path.join(REPO, "tools", "stagebench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def logged_alternate(sb, names, repeats, warm, K=7):
    """alternate() on launches that log their calls and a time_one that logs instead of launching -> (log, result)."""
    log = []
    launches = {n: (lambda n=n: log.append(("launch", n))) for n in names}
    by_launch = {f: n for n, f in launches.items()}

    def time_one(launch, k):
        assert k == K
        log.append(("time", by_launch[launch]))
        return float(len(log))

    return log, sb.alternate(launches, K, repeats, warm, time_one=time_one)


def test_alternate_warms_every_launch_then_alternates(sb):
    log, us = logged_alternate(sb, "abc", repeats=3, warm=2)
    first = log.index(("time", "a"))
    assert log[:first] == [("launch", n) for n in "aabbcc"]            # exactly `warm` calls of each before the first timing
    assert log[first:] == [("time", n) for n in "abc" "cba" "abc"]     # and nothing but timings after it
    assert list(us) == ["a", "b", "c"] and all(len(v) == 3 for v in us.values())
    assert us["a"] == [7.0, 12.0, 13.0]                                # each value with its own launch, in the order of the repeats


def test_alternate_one_repeat_and_one_name(sb):
    log, us = logged_alternate(sb, "abc", repeats=1, warm=2)
    assert [e for e in log if e[0] == "time"] == [("time", n) for n in "abc"] and all(len(v) == 1 for v in us.values())
    log, us = logged_alternate(sb, "a", repeats=3, warm=2)
    assert log == [("launch", "a")] * 2 + [("time", "a")] * 3 and list(us) == ["a"] and len(us["a"]) == 3


def test_alternating(sb):
    assert sb.alternating({"x": 1, "y": 2, "z": 3}, 0) == ["x", "y", "z"]
    assert sb.alternating(["x", "y", "z"], 1) == ["z", "y", "x"]
    assert sb.alternating(["x", "y", "z"], 2) == ["x", "y", "z"]


def test_time_host_loops_with_a_fake_clock(sb):
    now, calls = [0.0], []
    cost = {"a": 0.25, "b": 0.5, "c": 2.0}                             # seconds that one call of the loop takes, whatever n (exact in binary)

    def loop(name):
        def run(n):
            calls.append((name, n))
            now[0] += cost[name]
        return run

    ms = sb.time_host_loops({n: loop(n) for n in "abc"}, frames=8, repeats=3, clock=lambda: now[0])
    assert calls[:3] == [(n, 20) for n in "abc"]                       # one warm-up call of 20 frames per loop
    assert calls[3:] == [(n, 8) for n in "abc" "cba" "abc"]
    assert ms == {n: [cost[n] / 8 * 1e3] * 3 for n in "abc"}
    calls.clear()
    sb.time_host_loops({"a": loop("a")}, frames=8, repeats=1, warm=5, clock=lambda: now[0])
    assert calls == [("a", 5), ("a", 8)]


def test_summarise(sb):
    rec = {}
    sb.summarise(rec, "odd", [3.14159, 1.0, 2.71828], "us")
    sb.summarise(rec, "even", [4.0, 1.00004, 2.00006, 3.0], "ms")
    assert rec == {"odd_us": 2.72, "odd_us_all": [3.14, 1.0, 2.72], "even_ms": 2.5, "even_ms_all": [4.0, 1.0, 2.0001, 3.0]}
    assert list(rec) == ["odd_us", "odd_us_all", "even_ms", "even_ms_all"]
    with pytest.raises(KeyError):
        sb.summarise(rec, "x", [1.0], "s")


def test_spread(sb):
    assert sb.spread([2.5, 1.0, 4.0]) == 3.0 and sb.spread([7.0]) == 0.0


def test_write_records(sb, tmp_path):
    out = tmp_path / "not" / "yet" / "there.json"
    records = [{"size": [4, 2], "a_us": 1.25, "a_us_all": [1.25]}]
    sb.write_records(str(out), "tools/bench_x.py", records, scene="C2", note=None, tail={"frame_loop": {"frames": 3}})
    text = out.read_text()
    assert text.endswith("}\n") and not text.endswith("\n\n") and text.splitlines()[1].startswith(' "tool"')      # indent=1
    doc = json.loads(text)
    assert doc == {"tool": "tools/bench_x.py", "scene": "C2", "note": None, "records": records, "frame_loop": {"frames": 3}}
    assert list(doc) == ["tool", "scene", "note", "records", "frame_loop"]
    sb.write_records(str(out), "tools/bench_x.py", [])                # the directory may exist; the file is replaced
    assert json.loads(out.read_text()) == {"tool": "tools/bench_x.py", "records": []}


def test_parse_variants(sb):
    assert sb.parse_variants([]) == {}
    assert sb.parse_variants(["a=x/y.so", "b=exp/lib_K=4.so"]) == {"a": "x/y.so", "b": "exp/lib_K=4.so"}
    for bad in ("x/y.so", "=x/y.so", "a="):
        with pytest.raises(ValueError, match="NAME=PATH"):
            sb.parse_variants(["a=x/y.so", bad])


@pytest.mark.parametrize("preset", [False, True], ids=["RT_LIB-unset", "RT_LIB-set"])
def test_tracer_cleans_up_when_no_context_can_be_made(sb, host, monkeypatch, preset):
    """tracer() leaves neither a cached library nor RT_LIB behind when rt_create fails.  Without a device that is what RayTracer(0)
    does by itself; where the suite runs beside one, a RayTracer that fails in the same way stands in for it."""
    import torch
    assert sb.host is host
    monkeypatch.setattr(host, "_LIB", host._LIB)                       # the session's library comes back after the test
    monkeypatch.delenv("RT_LIB", raising=False)
    if preset:
        monkeypatch.setenv("RT_LIB", host._build.LIB_PATH)
    if torch.cuda.is_available():
        def no_device(device=0):
            host.load_library()
            raise host.RtError(-2, "rt_create (is a HIP device present?)")
        monkeypatch.setattr(host, "RayTracer", no_device)
    with pytest.raises(host.RtError):
        sb.tracer(None)
    assert host._LIB is None and "RT_LIB" not in os.environ


@pytest.mark.parametrize("tool", TOOLS)
def test_help_needs_no_device(tool):
    """Every tool parses its arguments before it opens a device, so --help is a rehearsal of its imports and options anywhere."""
    run = subprocess.run([sys.executable, os.path.join(REPO, "tools", f"bench_{tool}.py"), "--help"], capture_output=True, text=True,
                         env={**os.environ, "HIP_VISIBLE_DEVICES": "-1"})      # devices hidden: opening one fails beside a GPU as well
    assert run.returncode == 0, run.stderr
    for option in ("--out", "--frames", "--repeats"):
        assert option in run.stdout
