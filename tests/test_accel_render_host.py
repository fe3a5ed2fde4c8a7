"""CPU-only tests of rt_set_accel_render's parts that need no GPU (include/rt_mi355.h): the two structs in C and in ctypes, the enum
and the default minObjects in the header against layout.py's, make_accel_render_desc, and the refusals that need no context."""
import ctypes
import os
import subprocess

from opengl_raytracing_amd import layout as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def c_check(tmp_path, checks):
    """A C program that includes the public header and returns 0 iff every check holds."""
    src, exe = tmp_path / "a.c", tmp_path / "a"
    src.write_text('#include <stddef.h>\n#include "rt_mi355.h"\nint main(void){ return (' + " && ".join(checks) + ") ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)]).returncode == 0


def test_struct_layouts_in_c_and_ctypes(tmp_path):
    D, R = L.RtAccelRenderDesc, L.RtAccelRenderReport
    desc = dict(enable=0, traversal=4, minObjects=8, reserved=12)
    rep = dict(active=0, traversal=4, minObjects=8, reserved0=12, launchesAccel=16, launchesPacket=40, reserved=48)
    assert ctypes.sizeof(D) == 32 and ctypes.sizeof(R) == 64
    for k, v in desc.items():
        assert getattr(D, k).offset == v, k
    for k, v in rep.items():
        assert getattr(R, k).offset == v, k
    assert D.reserved.size == 20 and R.launchesAccel.size == 24 and R.reserved.size == 16
    assert c_check(tmp_path, [f"offsetof(rt_accel_render_desc, {k}) == {v}" for k, v in desc.items()] +
                   [f"offsetof(rt_accel_render_report, {k}) == {v}" for k, v in rep.items()] +
                   ["sizeof(rt_accel_render_desc) == 32", "sizeof(rt_accel_render_report) == 64"])


def test_the_headers_constants_are_layouts(tmp_path):
    assert L.ACCEL_RENDER_TRAVERSALS == dict(auto=0, lane=1, wave=2, split=3)
    assert (L.ACCEL_RENDER_AUTO, L.ACCEL_RENDER_LANE, L.ACCEL_RENDER_WAVE, L.ACCEL_RENDER_SPLIT) == (0, 1, 2, 3)
    assert L.ACCEL_RENDER_DEFAULT_MIN_OBJECTS >= 257, "up to 256 objects the packet kernel has its shadow tables"
    assert c_check(tmp_path, [f"RT_ACCEL_RENDER_{k.upper()} == {v}" for k, v in L.ACCEL_RENDER_TRAVERSALS.items()] +
                   [f"RT_ACCEL_RENDER_DEFAULT_MIN_OBJECTS == {L.ACCEL_RENDER_DEFAULT_MIN_OBJECTS}",
                    # the first two traversals are rt_accel_traversal's, which keeps its three values
                    "(int)RT_ACCEL_RENDER_LANE == (int)RT_ACCEL_LANE", "(int)RT_ACCEL_RENDER_WAVE == (int)RT_ACCEL_WAVE",
                    "(int)RT_ACCEL_RENDER_AUTO == (int)RT_ACCEL_AUTO"])


def test_make_accel_render_desc():
    d = L.make_accel_render_desc()
    assert (d.enable, d.traversal, d.minObjects, list(d.reserved)) == (1, L.ACCEL_RENDER_AUTO, 0, [0] * 5)
    d = L.make_accel_render_desc(False, "split", 77)
    assert (d.enable, d.traversal, d.minObjects) == (0, L.ACCEL_RENDER_SPLIT, 77)
    assert L.make_accel_render_desc(traversal="wave").traversal == L.ACCEL_RENDER_WAVE and L.make_accel_render_desc(traversal=9).traversal == 9


def test_entry_points_refuse_a_null_context(host):
    lib = host.load_library()
    d, r = L.make_accel_render_desc(), L.RtAccelRenderReport()
    assert lib.rt_set_accel_render(None, ctypes.byref(d)) == -1
    assert lib.rt_set_accel_render(None, None) == -1
    assert lib.rt_accel_render_info(None, ctypes.byref(r)) == -1
