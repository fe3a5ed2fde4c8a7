"""CPU-only checks of the ray-shading ABI (rt_shade_rays, include/rt_mi355.h): the library exports the entry point, the
header declares it and the 8-byte rt_pixel record with the documented layout in C, numpy and ctypes, and bad arguments
are refused before any device is touched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from opengl_raytracing_amd import layout as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID_ARG = -1


def test_library_exports_the_shade_entry_point(host):
    lib = host.load_library()
    assert hasattr(lib, "rt_shade_rays")
    assert "rt_shade_rays" in host.EXPORTS


def test_header_compiles_as_c_with_pixel_layout(tmp_path):
    src = tmp_path / "s.c"
    src.write_text(
        '#include <stddef.h>\n#include "rt_mi355.h"\n'
        '_Static_assert(sizeof(rt_pixel) == 8, "rt_pixel");\n'
        '_Static_assert(offsetof(rt_pixel, x) == 0 && offsetof(rt_pixel, y) == 4, "rt_pixel.x/y");\n'
        '_Static_assert(sizeof(((rt_pixel *)0)->x) == 4 && (__typeof__(((rt_pixel *)0)->y))-1 > 0, "unsigned 32-bit");\n'
        'int main(void) {\n'
        '  int (*f)(rt_context *, const rt_params *, const void *, const void *, size_t, void *, void *, void *, void *) = rt_shade_rays;\n'
        '  return f ? 0 : 1; }\n')
    obj = tmp_path / "s.o"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", "-I", os.path.join(REPO, "include"), str(src), "-o", str(obj)],
                   check=True)


def test_pixel_dtype_matches_the_header():
    assert L.PIXEL_DTYPE.itemsize == 8
    assert L.PIXEL_DTYPE.fields["x"][1] == 0 and L.PIXEL_DTYPE.fields["y"][1] == 4
    assert L.PIXEL_DTYPE.fields["x"][0] == np.dtype("<u4") and L.PIXEL_DTYPE.fields["y"][0] == np.dtype("<u4")
    assert L.RtPixel.x.offset == 0 and L.RtPixel.y.offset == 4 and ctypes.sizeof(L.RtPixel) == 8
    a = np.array([[3, 0xffffffff]], dtype=np.uint32)
    r = a.view(L.PIXEL_DTYPE).reshape(1)
    assert r["x"][0] == 3 and r["y"][0] == 0xffffffff


def test_null_context_and_null_params_are_invalid_arguments(host):
    lib = host.load_library()
    p = L.make_params(64, 32, 1)
    buf = ctypes.create_string_buffer(64)
    assert lib.rt_shade_rays(None, ctypes.byref(p), buf, None, 1, buf, None, None, None) == RT_ERR_INVALID_ARG
    assert lib.rt_shade_rays(None, None, None, None, 0, None, None, None, None) == RT_ERR_INVALID_ARG


class _NoDevice:
    """RayTracer's methods on an object without a device context: any call that reached the ABI would fail differently."""
    def __init__(self, host):
        self.lib = None
        self.ctx = None


def _shade(host, *a, **k):
    return host.RayTracer.shade_rays(_NoDevice(host), *a, **k)


def test_python_argument_checks_fail_before_any_device_call(host):
    torch = pytest.importorskip("torch")
    p = L.make_params(8, 4, 2)                      # 32 pixels
    rays = torch.zeros((32, 8), dtype=torch.float32)
    px = torch.zeros((32, 2), dtype=torch.int32)
    bad = [
        dict(rays=np.zeros((32, 8), np.float32)),                        # not a tensor
        dict(rays=torch.zeros((32, 8), dtype=torch.float64)),            # wrong dtype
        dict(rays=torch.zeros((32, 7), dtype=torch.float32)),            # not rt_ray rows
        dict(rays=torch.zeros((31, 8), dtype=torch.float32)),            # pixels=None: not regionW * regionH rays
        dict(pixels=torch.zeros((32, 2), dtype=torch.int64)),            # wrong pixel dtype
        dict(pixels=torch.zeros((31, 2), dtype=torch.int32)),            # one pixel short
        dict(pixels=torch.zeros((32, 3), dtype=torch.int32)),            # not (x, y) rows
        dict(pixels=px, out=(torch.zeros((32, 4), dtype=torch.float16), None, None)),   # colour must be float32
        dict(pixels=px, out=(None, None, torch.zeros((32, 4), dtype=torch.float32))),   # normal must be float16
        dict(pixels=px, out=(torch.zeros((31, 4), dtype=torch.float32), None, None)),   # one row short
        dict(),                                                          # valid shapes, but host tensors
        dict(pixels=px),
    ]
    for case in bad:
        kw = dict(case)
        r = kw.pop("rays", rays)
        with pytest.raises(ValueError):
            _shade(host, p, r, **kw)
