"""CPU-only checks of the ray-query ABI (rt_trace_rays / rt_camera_rays / rt_pick, include/rt_mi355.h): the library
exports the entry points, the 32-byte rt_ray / rt_hit records have the documented layout in C, numpy and ctypes, and
bad arguments are refused before any device is touched."""
import ctypes
import os
import subprocess

import numpy as np

from opengl_raytracing_amd import layout as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID_ARG = -1


def test_library_exports_the_query_entry_points(host):
    lib = host.load_library()
    for name in ("rt_trace_rays", "rt_camera_rays", "rt_pick"):
        assert hasattr(lib, name), name
        assert name in host.EXPORTS, name


def test_header_compiles_as_c_with_ray_and_hit_layout(tmp_path):
    src = tmp_path / "q.c"
    src.write_text(
        '#include <stddef.h>\n#include "rt_mi355.h"\n'
        '_Static_assert(sizeof(rt_ray) == 32, "rt_ray");\n'
        '_Static_assert(offsetof(rt_ray, origin) == 0 && offsetof(rt_ray, tMax) == 12, "rt_ray.origin/tMax");\n'
        '_Static_assert(offsetof(rt_ray, direction) == 16 && offsetof(rt_ray, reserved) == 28, "rt_ray.direction/reserved");\n'
        '_Static_assert(sizeof(rt_hit) == 32, "rt_hit");\n'
        '_Static_assert(offsetof(rt_hit, position) == 0 && offsetof(rt_hit, t) == 12, "rt_hit.position/t");\n'
        '_Static_assert(offsetof(rt_hit, normal) == 16 && offsetof(rt_hit, object) == 28, "rt_hit.normal/object");\n'
        '_Static_assert(RT_QUERY_CLOSEST == 0 && RT_QUERY_ANY == 1, "modes");\n'
        'int main(void) { rt_hit h; rt_ray r; (void)h; (void)r;\n'
        '  int (*a)(rt_context *, const void *, size_t, int, void *, void *) = rt_trace_rays;\n'
        '  int (*b)(rt_context *, const rt_params *, void *, void *) = rt_camera_rays;\n'
        '  int (*c)(rt_context *, const rt_params *, int, int, rt_hit *) = rt_pick;\n'
        '  return (a && b && c) ? 0 : 1; }\n')
    obj = tmp_path / "q.o"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", "-I", os.path.join(REPO, "include"), str(src), "-o", str(obj)],
                   check=True)


def test_ray_and_hit_dtypes_match_the_header():
    assert L.RAY_DTYPE.itemsize == 32 and L.HIT_DTYPE.itemsize == 32
    for name, off in dict(origin=0, tMax=12, direction=16, reserved=28).items():
        assert L.RAY_DTYPE.fields[name][1] == off, name
        assert getattr(L.RtRay, name).offset == off, name
    for name, off in dict(position=0, t=12, normal=16, object=28).items():
        assert L.HIT_DTYPE.fields[name][1] == off, name
        assert getattr(L.RtHit, name).offset == off, name
    assert ctypes.sizeof(L.RtRay) == 32 and ctypes.sizeof(L.RtHit) == 32
    # a float32 [n, 8] buffer reinterprets as records
    a = np.arange(16, dtype=np.float32).reshape(2, 8)
    r = a.view(L.RAY_DTYPE).reshape(2)
    assert r["tMax"][1] == 11.0 and (r["direction"][0] == (4.0, 5.0, 6.0)).all()


def test_null_context_and_null_pointers_are_invalid_arguments(host):
    lib = host.load_library()
    p = L.make_params(64, 32, 1)
    hit = L.RtHit()
    buf = ctypes.create_string_buffer(64)
    for mode in (0, 1):
        assert lib.rt_trace_rays(None, buf, 1, mode, buf, None) == RT_ERR_INVALID_ARG
        assert lib.rt_trace_rays(None, None, 1, mode, None, None) == RT_ERR_INVALID_ARG
    assert lib.rt_trace_rays(None, buf, 0, 0, buf, None) == RT_ERR_INVALID_ARG
    assert lib.rt_camera_rays(None, ctypes.byref(p), buf, None) == RT_ERR_INVALID_ARG
    assert lib.rt_camera_rays(None, None, None, None) == RT_ERR_INVALID_ARG
    assert lib.rt_pick(None, ctypes.byref(p), 0, 0, ctypes.byref(hit)) == RT_ERR_INVALID_ARG
    assert lib.rt_pick(None, None, 0, 0, None) == RT_ERR_INVALID_ARG


def test_device_math_entry_refuses_bad_arguments_without_a_device(host, tmp_path):
    """rt_debug_device_math (the test hook behind tests/test_device_math.py): exported, declared with the documented C
    signature and op numbers, and a NULL context -- with or without pointers, for every op -- is an invalid argument
    before any device is touched."""
    lib = host.load_library()
    assert hasattr(lib, "rt_debug_device_math") and "rt_debug_device_math" in host.EXPORTS
    buf = ctypes.create_string_buffer(64)
    for op in list(host.DEVICE_MATH_OPS.values()) + [-1, len(host.DEVICE_MATH_OPS)]:
        assert lib.rt_debug_device_math(None, op, buf, buf, 1, None) == RT_ERR_INVALID_ARG
        assert lib.rt_debug_device_math(None, op, None, None, 1, None) == RT_ERR_INVALID_ARG
        assert lib.rt_debug_device_math(None, op, None, buf, 0, None) == RT_ERR_INVALID_ARG
    src = tmp_path / "m.c"
    names = dict(rcp="RCP", rcp3="RCP3", sqrt="SQRT", rcp_sqrt="RCP_SQRT", div2="DIV2", div3="DIV3", mesa="MESA", f2h="F2H",
                 pow5="POW5", halton="HALTON")
    assert set(names) == set(host.DEVICE_MATH_OPS)
    checks = " && ".join(f"RT_DM_{c} == {host.DEVICE_MATH_OPS[k]}" for k, c in names.items())
    src.write_text(
        '#include <stddef.h>\n#include "rt_mi355.h"\n'
        f'_Static_assert({checks} && RT_DM_OP_COUNT == {len(names)}, "rt_device_math_op");\n'
        'int main(void) { int (*f)(rt_context *, int, const void *, void *, size_t, void *) = rt_debug_device_math;\n'
        '  return f ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", "-I", os.path.join(REPO, "include"), str(src), "-o",
                    str(tmp_path / "m.o")], check=True)
