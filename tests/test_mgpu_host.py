"""CPU-only tests of rt_mgpu_* (include/rt_mi355.h, csrc/rt_mgpu.cpp): the argument refusals that are decided before any device is
touched.  No context is created and no GPU call is made; tests/test_mgpu_frames.py holds the GPU half."""
import ctypes


def test_create_refuses_bad_arguments(host):
    lib = host.load_library()
    m = ctypes.c_void_p(0xDEAD)
    one = (ctypes.c_int * 1)(0)
    many = (ctypes.c_int * 65)(*([0] * 65))
    assert lib.rt_mgpu_create(None, one, 1) == -1, "NULL out"
    assert lib.rt_mgpu_create(ctypes.byref(m), None, 1) == -1, "NULL device ids"
    assert lib.rt_mgpu_create(ctypes.byref(m), one, 0) == -1, "no device"
    assert lib.rt_mgpu_create(ctypes.byref(m), one, -1) == -1, "a negative device count"
    assert lib.rt_mgpu_create(ctypes.byref(m), many, 65) == -1, "65 devices"
    assert m.value == 0xDEAD, "a refused rt_mgpu_create wrote its out parameter"


def test_entry_points_refuse_a_null_handle(host):
    lib = host.load_library()
    assert lib.rt_mgpu_destroy(None) == -1
    assert lib.rt_mgpu_device_count(None) == -1
    assert lib.rt_mgpu_set_strip_rows(None, 0) == -1 and lib.rt_mgpu_set_strip_rows(None, 8) == -1
    assert lib.rt_mgpu_set_scene(None, None, 0, None, 0) == -1
    assert lib.rt_mgpu_set_noise(None, None, 0, 0) == -1
    assert lib.rt_mgpu_set_skybox(None, None, 0) == -1
    assert lib.rt_mgpu_render(None, None) == -1
    assert lib.rt_mgpu_sync(None) == -1
    assert lib.rt_mgpu_get_surfaces(None, None, None, None, None) == -1
    assert lib.rt_mgpu_readback(None, None, None, None) == -1
    ms = (ctypes.c_float * 4)()
    assert lib.rt_mgpu_last_ms(None, ms, 4) == -1
    assert lib.rt_mgpu_last_error(None) == b"NULL rt_mgpu"


def test_context_refuses_null_arguments(host):
    """rt_mgpu_context: NULL handle (with and without a place for the answer); the out-of-range slots need a handle and are in
    the GPU half."""
    lib = host.load_library()
    c = ctypes.c_void_p(0xDEAD)
    assert lib.rt_mgpu_context(None, 0, ctypes.byref(c)) == -1
    assert lib.rt_mgpu_context(None, 0, None) == -1
    assert c.value == 0xDEAD, "a refused rt_mgpu_context wrote its out parameter"
    assert "rt_mgpu_context" in host.EXPORTS and host.SIGNATURES["rt_mgpu_context"][0] is ctypes.c_int
