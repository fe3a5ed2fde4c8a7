"""The measurement procedure of the stage benchmarks (tools/bench_accum.py, bench_denoise.py, bench_jpeg.py, bench_meter.py,
bench_present.py, bench_reproject.py, bench_resample.py, bench_yuv.py), defined once. Every speed figure those tools record rests on it:

  device figures  one event pair on the side stream around K back-to-back launches, behind 40 copies between two 256 MiB blockers
                  that keep the stream busy until the whole batch is queued; microseconds per call;
  host figures    a host clock around a loop of `frames` frames that ends in a sync or a wait; milliseconds per frame, behind 20
                  warm-up frames per loop;
  both            `repeats` repeats, the candidates in forward order on even repeats and in reversed order on odd ones, the median
                  and every repeat's value in the record.

A launch is a callable without arguments that issues its work on side(); one that rotates through buffers keeps its own counter.
The first part needs no device; nothing here touches the GPU at import: the side stream and the blockers are made on first use."""
import ctypes, functools, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from opengl_raytracing_amd import host


# ---- no device needed ------------------------------------------------------------------------------------------------------------
def add_common_args(ap, out_name, launches=None, parent_lib=True, variant_macros=None):
    """--out (default profiles/<out_name>), --frames and --repeats; --launches with the default `launches`, --parent-lib and, for
    libraries built with other <variant_macros>* macros, --variant where the tool has them."""
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out_name))
    if parent_lib:
        ap.add_argument("--parent-lib", default=None, help="librt_mi355.so built from the parent commit (build_library(out=...))")
    if variant_macros:
        ap.add_argument("--variant", action="append", default=[], help=f"NAME=PATH of a library built with other {variant_macros}* macros")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    if launches:
        ap.add_argument("--launches", type=int, default=launches)


def parse_variants(specs):
    """["NAME=PATH", ...] -> {name: path}; the path may hold further `=`."""
    out = {}
    for spec in specs:
        name, eq, path = spec.partition("=")
        if not (name and eq and path):
            raise ValueError(f"a variant is given as NAME=PATH, not {spec!r}")
        out[name] = path
    return out


def alternating(names, r):
    """The order of repeat r: forward on even repeats, reversed on odd ones."""
    names = list(names)
    return names if r % 2 == 0 else names[::-1]


def summarise(rec, key, values, unit):
    """The median of `values` as rec[<key>_<unit>] and all of them as rec[<key>_<unit>_all]; unit is "us" or "ms"."""
    digits = {"us": 2, "ms": 4}[unit]
    rec[f"{key}_{unit}"] = round(statistics.median(values), digits)
    rec[f"{key}_{unit}_all"] = [round(x, digits) for x in values]


def spread(values):
    return max(values) - min(values)


def time_host_loops(loops, frames, repeats, warm=20, clock=time.perf_counter):
    """loops: {name: callable(n) that runs n frames and returns with all of them complete}; `warm` frames of each first, then every
    repeat times each once over `frames` frames, in alternating order -> {name: [ms per frame per repeat]}."""
    for f in loops.values():
        f(warm)
    ms = {k: [] for k in loops}
    for r in range(repeats):
        for k in alternating(loops, r):
            t0 = clock()
            loops[k](frames)
            ms[k].append((clock() - t0) / frames * 1e3)
    return ms


def alternate(launches, K, repeats, warm, time_one=None):
    """launches: {name: callable}; `warm` calls of each first, then every repeat times each once with time_one(launch, K) (default:
    device_us), in alternating order -> {name: [us per repeat]}."""
    for f in launches.values():
        for _ in range(warm):
            f()
    if time_one is None:
        side().synchronize()
        time_one = device_us
    us = {k: [] for k in launches}
    for r in range(repeats):
        for k in alternating(launches, r):
            us[k].append(time_one(launches[k], K))
    return us


def write_records(out, tool, records, tail=None, **top):
    """The file every tool leaves: {"tool", <top>, "records", <tail>}."""
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"tool": tool, **top, "records": records, **(tail or {})}, f, indent=1)
        f.write("\n")


# ---- device ----------------------------------------------------------------------------------------------------------------------
def tracer(path):
    """A RayTracer on the library at `path` (None: this build's)."""
    host._LIB = None
    if path:
        os.environ["RT_LIB"] = path
    try:
        return host.RayTracer(0)
    finally:
        os.environ.pop("RT_LIB", None)
        host._LIB = None


def open_tracers(parent_lib, variants):
    """-> (new, old, {"this": new, name: tracer, ...}): this build's tracer, the parent library's (this build's again without one) and
    one per entry of `variants` = {name: path}."""
    new = tracer(None)
    old = tracer(parent_lib) if parent_lib else new
    return new, old, {"this": new, **{name: tracer(path) for name, path in variants.items()}}


def distinct(tracers):
    """Each tracer of `tracers` once, in order."""
    return list({id(t): t for t in tracers}.values())


def close_all(tracers):
    for t in distinct(tracers):
        t.close()


def check(t, rc, what):
    """t._check(rc, what) when rc says failure: for the stage benchmarks that call the library directly inside timed loops."""
    if rc:
        t._check(rc, what)


@functools.cache
def _device():
    """The side stream and the two 256 MiB blockers, made together on first use.  A tool asks for side() before it allocates its own
    buffers, so the blockers are allocated in front of them, as they were when every tool made its own."""
    stream = torch.cuda.Stream()
    a = torch.zeros(256 << 20, dtype=torch.uint8, device="cuda")
    return stream, a, torch.empty_like(a)


def side():
    """The one side stream that device figures are taken on."""
    return _device()[0]


def hold():
    """Keep side() busy for a few milliseconds so that the launches timed behind it are all queued before the first one starts: a
    stage runs for microseconds, less than a launch takes to enqueue."""
    _, a, b = _device()
    with torch.cuda.stream(side()):
        for _ in range(40):
            b.copy_(a)


def device_us(launch, K):
    """Microseconds per call of launch() from device events around K back-to-back calls on side()."""
    s = side()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    hold()
    e0.record(s)
    for _ in range(K):
        launch()
    e1.record(s)
    s.synchronize()
    return e0.elapsed_time(e1) / K * 1e3


def _rendered(t, p):
    """One rt_render of p on t -> (render(), the colour surface's device address)."""
    lib, ctx, d_color = t.lib, t.ctx, ctypes.c_void_p()

    def render():
        t._check(lib.rt_render(ctx, ctypes.byref(p)), "rt_render")

    render()
    t._check(lib.rt_get_surfaces(ctx, ctypes.byref(d_color), None, None), "rt_get_surfaces")
    return render, d_color


def render_loop(t, p, stages=()):
    """-> loop(n): n frames of rt_render and then every stage(d_color, k) of frame k, on t's own stream and surfaces, then a sync."""
    render, d_color = _rendered(t, p)

    def loop(n):
        for k in range(n):
            render()
            for stage in stages:
                stage(d_color, k)
        t.sync()
    return loop


def present_loop(t, p, submit):
    """-> loop(n): n frames of rt_render and submit(d_color, ticket_ref), which issues the stages and one rt_present_submit* that fills
    the ticket; every frame waits for the PREVIOUS frame's ticket, the loop for the last one, then a sync."""
    render, d_color = _rendered(t, p)

    def loop(n):
        px, nb, tk = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_uint64()
        prev = None
        for _ in range(n):
            render()
            submit(d_color, ctypes.byref(tk))
            if prev is not None:
                t._check(t.lib.rt_present_wait(t.ctx, prev, ctypes.byref(px), ctypes.byref(nb)), "rt_present_wait")
            prev = tk.value
        t._check(t.lib.rt_present_wait(t.ctx, prev, ctypes.byref(px), ctypes.byref(nb)), "rt_present_wait")
        t.sync()
    return loop
