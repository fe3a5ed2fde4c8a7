"""ctypes binding of librt_mi355.so -- the Python-side mirror of the reference's dispatch
site (/root/reference/src/ForwardShadingPipeline.cpp:155-182).

``RayTracer`` plays the part of ``ForwardShadingPipline``'s ray-tracing members:

=====================================  ====================================================
reference (C++ / GL)                   here
=====================================  ====================================================
``ssbo.update(); lightSSBO.update()``  ``RayTracer.set_scene(objects, lights)``
``raytracingShader.setXxx(...)``       fields of ``RtParams`` (layout.make_params)
``glBindTexture(CUBE_MAP, ...)``       ``RayTracer.set_skybox(faces)``
blue-noise texture                     ``RayTracer.set_noise(r8)``
``glDispatchCompute + glMemoryBarrier````RayTracer.render(params)``
``glGetTexImage``                      ``RayTracer.readback()``
``gProfiler`` RayTracing stage         ``RayTracer.last_kernel_ms()``
=====================================  ====================================================

There is no CPU fallback: if the HIP library is missing or no GPU is present the calls
raise ``RtError``.
"""
import collections
import ctypes
import os

import numpy as np

from . import build as _build
from . import layout as L

_LIB = None


class RtFrameDesc(ctypes.Structure):
    """``rt_frame_desc`` of include/rt_mi355.h."""
    _fields_ = [("enableAO", ctypes.c_int32), ("enableTAA", ctypes.c_int32), ("taaBlendFactor", ctypes.c_float),
                ("bloomThreshold", ctypes.c_float), ("bloomStrength", ctypes.c_float), ("bloomIterations", ctypes.c_int32),
                ("aoSamples", ctypes.POINTER(ctypes.c_float)), ("aoNoise", ctypes.POINTER(ctypes.c_float)),
                ("reserved", ctypes.c_float * 2)]


RtAccumDesc, RtAccumState = L.RtAccumDesc, L.RtAccumState      # rt_accum_desc / rt_accum_state (layout.py has every record)

RT_OK = 0
STATUS_NAMES = {0: "RT_OK", -1: "RT_ERR_INVALID_ARG", -2: "RT_ERR_NO_DEVICE", -3: "RT_ERR_HIP",
                -4: "RT_ERR_TOO_LARGE", -5: "RT_ERR_NO_SURFACES", -6: "RT_ERR_PARSE"}


class RtError(RuntimeError):
    def __init__(self, code, msg=""):
        self.code = code
        super().__init__(f"{STATUS_NAMES.get(code, code)}: {msg}")


def _signatures():
    """Every entry point of include/rt_mi355.h, in the header's order: name -> (restype, argtypes).  The one place a prototype is
    written down on this side; tests/test_binding_host.py holds it to the header."""
    P = ctypes.POINTER
    vp, ci, cf, sz, cs = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_char_p
    u8, u32, i32, u64 = ctypes.c_uint8, ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint64
    params, tone, yuv, jpeg, accum = P(L.RtParams), P(L.RtToneDesc), P(L.RtYuvDesc), P(L.RtJpegDesc), P(L.RtAccumDesc)
    display = P(L.RtDisplayDesc)
    return {
        "rt_create": (ci, [P(vp), ci]),
        "rt_destroy": (ci, [vp]),
        "rt_set_scene": (ci, [vp, vp, ci, vp, ci]),
        "rt_set_noise": (ci, [vp, vp, ci, ci]),
        "rt_set_skybox": (ci, [vp, vp, ci]),
        "rt_render": (ci, [vp, params]),
        "rt_render_to": (ci, [vp, params, vp, vp, vp, vp]),
        "rt_render_into_image": (ci, [vp, params, vp, vp, vp, vp]),
        "rt_context_stream": (ci, [vp, P(vp)]),
        "rt_sync": (ci, [vp]),
        "rt_readback": (ci, [vp, vp, vp, vp]),
        "rt_get_surfaces": (ci, [vp, P(vp), P(vp), P(vp)]),
        "rt_last_kernel_ms": (ci, [vp, P(cf)]),
        "rt_count_rays": (ci, [vp, params, P(u64)]),
        "rt_count_rays_traced": (ci, [vp, params, P(u64)]),
        "rt_count_rays_to": (ci, [vp, params, ci, vp, vp, vp, P(u64)]),
        "rt_set_variant": (ci, [vp, ci]),
        "rt_debug_first_hit": (ci, [vp, P(u64)]),
        "rt_debug_settled_tiles": (ci, [vp, P(u64)]),
        "rt_debug_settled_map": (ci, [vp, P(u8), sz]),
        "rt_debug_prefix_tiles": (ci, [vp, P(u64)]),
        "rt_debug_stats": (ci, [vp, P(u64)]),
        "rt_debug_stats_ex": (ci, [vp, P(u64)]),
        "rt_debug_tile_costs": (ci, [vp, P(u32), ci, P(ci), P(ci)]),
        "rt_debug_predicted_classes": (ci, [vp, vp, ci, P(ci)]),
        "rt_debug_tile_order": (ci, [vp, P(u32), ci, P(ci), P(ci)]),
        "rt_debug_lpt_sort": (ci, [vp, P(u32), ci, P(u32), P(u32)]),
        "rt_debug_split_tiles": (ci, [vp, P(u8), ci, P(ci)]),
        "rt_debug_split_plan": (ci, [vp, P(u32), P(u32), ci, u32, ci, ci, ci, P(u8), P(u8), P(u32), P(u32), P(u32)]),
        "rt_debug_shadow_tables": (ci, [vp, vp, sz, P(sz), P(ci)]),
        "rt_debug_mesa_math": (ci, [vp, vp, ci]),
        "rt_debug_device_math": (ci, [vp, ci, vp, vp, sz, vp]),
        "rt_trace_rays": (ci, [vp, vp, sz, ci, vp, vp]),
        "rt_camera_rays": (ci, [vp, params, vp, vp]),
        "rt_pick": (ci, [vp, params, ci, ci, P(L.RtHit)]),
        "rt_set_accel": (ci, [vp, P(L.RtAccelDesc)]),
        "rt_accel_info": (ci, [vp, P(L.RtAccelReport)]),
        "rt_accel_build_host": (ci, [vp, ci, P(L.RtAccelDesc), vp, sz, vp, sz, vp, sz, P(L.RtAccelReport)]),
        "rt_accel_validate_host": (ci, [vp, ci, ci, vp, sz, vp, sz, vp, sz]),
        "rt_set_accel_builder": (ci, [vp, ci]),
        "rt_accel_build_info": (ci, [vp, P(L.RtAccelBuildReport)]),
        "rt_accel_read": (ci, [vp, vp, sz, vp, sz, vp, sz, P(L.RtAccelReport)]),
        "rt_set_accel_shading": (ci, [vp, P(L.RtAccelShadeDesc)]),
        "rt_accel_shading_info": (ci, [vp, P(L.RtAccelShadeReport)]),
        "rt_set_accel_render": (ci, [vp, P(L.RtAccelRenderDesc)]),
        "rt_accel_render_info": (ci, [vp, P(L.RtAccelRenderReport)]),
        "rt_shade_rays": (ci, [vp, params, vp, vp, sz, vp, vp, vp, vp]),
        "rt_last_error": (cs, [vp]),
        "rt_generate_aabb": (ci, [vp, ci]),
        "rt_camera_vectors": (ci, [cf, cf, P(cf), P(cf), P(cf)]),
        "rt_scene_parse": (ci, [cs, vp, ci, P(ci), vp, ci, P(ci)]),
        "rt_scene_write": (ci, [vp, ci, vp, ci, vp, vp, cs, sz, P(sz)]),
        "rt_taa_resolve": (ci, [vp, vp, vp, vp, vp, ci, ci, cf, cf, cf, vp]),
        "rt_taa_jitter": (ci, [ci, ci, ci, P(cf), P(cf)]),
        "rt_bloom": (ci, [vp, vp, vp, ci, ci, cf, cf, ci, vp]),
        "rt_ssao": (ci, [vp, vp, vp, vp, ci, ci, P(cf), ci, ci, P(cf), P(cf), P(cf), vp]),
        "rt_ssao_blur": (ci, [vp, vp, vp, ci, ci, ci, vp]),
        "rt_camera_matrices": (ci, [P(cf), P(cf), P(cf), cf, cf, P(cf), P(cf)]),
        "rt_equirect_to_cubemap": (ci, [vp, P(cf), ci, ci, ci, vp, ci]),
        "rt_frame": (ci, [vp, params, P(RtFrameDesc), vp]),
        "rt_frame_surfaces": (ci, [vp, P(vp), P(vp), P(vp), P(vp), P(vp)]),
        "rt_display_pack": (ci, [vp, vp, vp, display, vp]),
        "rt_display_srgb_thresholds": (ci, [P(cf)]),
        "rt_present_configure": (ci, [vp, ci]),
        "rt_present_submit": (ci, [vp, vp, display, vp, P(u64)]),
        "rt_present_poll": (ci, [vp, u64, P(ci)]),
        "rt_present_wait": (ci, [vp, u64, P(vp), P(sz)]),
        "rt_meter": (ci, [vp, vp, P(L.RtMeterDesc), vp, vp]),
        "rt_meter_solve_host": (ci, [vp, P(L.RtMeterDesc), vp]),
        "rt_meter_tables": (ci, [P(cf), P(u32)]),
        "rt_display_pack_toned": (ci, [vp, vp, vp, display, tone, vp]),
        "rt_present_submit_toned": (ci, [vp, vp, display, tone, vp, P(u64)]),
        "rt_display_yuv_coeffs": (ci, [ci, ci, P(i32)]),
        "rt_display_yuv_layout": (ci, [yuv, P(sz), P(sz), P(sz)]),
        "rt_display_pack_yuv": (ci, [vp, vp, vp, yuv, tone, vp]),
        "rt_present_submit_yuv": (ci, [vp, vp, yuv, tone, vp, P(u64)]),
        "rt_jpeg_dct_matrix": (ci, [P(i32)]),
        "rt_jpeg_quant": (ci, [ci, P(u8), P(u8)]),
        "rt_jpeg_header": (ci, [jpeg, P(u8), sz, P(sz)]),
        "rt_jpeg_layout": (ci, [jpeg, P(sz), P(sz), P(sz)]),
        "rt_jpeg_encode": (ci, [vp, vp, yuv, jpeg, vp, vp, sz, vp, vp]),
        "rt_display_pack_jpeg": (ci, [vp, vp, yuv, tone, jpeg, vp, vp, sz, vp, vp]),
        "rt_present_submit_jpeg": (ci, [vp, vp, yuv, tone, jpeg, sz, vp, P(u64)]),
        "rt_resample_taps": (ci, [ci, ci, ci, P(ci), P(i32), P(cf), sz]),
        "rt_display_resample": (ci, [vp, vp, vp, P(L.RtResampleDesc), vp]),
        "rt_accum_layout": (ci, [ci, ci, P(sz), P(sz)]),
        "rt_accum_reset": (ci, [vp, vp, vp, ci, ci, vp]),
        "rt_accum_add": (ci, [vp, vp, vp, accum, vp, vp]),
        "rt_accum_solve_host": (ci, [vp, accum, vp]),
        "rt_accum_view": (ci, [vp, vp, vp, accum, ci, vp]),
        "rt_denoise_guide": (ci, [vp, vp, vp, ci, ci, vp]),
        "rt_denoise_layout": (ci, [ci, ci, P(sz), P(sz)]),
        "rt_denoise": (ci, [vp, vp, vp, vp, vp, vp, P(L.RtDenoiseDesc), vp]),
        "rt_reproject_layout": (ci, [ci, ci, P(sz), P(sz)]),
        "rt_reproject_project": (ci, [params, P(cf), P(cf), P(ci)]),
        "rt_accum_reproject": (ci, [vp, vp, vp, vp, vp, P(L.RtReprojectDesc), vp, vp]),
        "rt_accum_select_layout": (ci, [ci, ci, P(sz)]),
        "rt_accum_select": (ci, [vp, vp, accum, u32, vp, sz, vp, vp, vp]),
        "rt_camera_rays_at": (ci, [vp, params, vp, sz, vp, vp]),
        "rt_accum_add_at": (ci, [vp, vp, vp, sz, vp, accum, vp, vp]),
        "rt_upsample_layout": (ci, [ci, ci, P(sz)]),
        "rt_upsample": (ci, [vp, vp, vp, vp, vp, P(L.RtUpsampleDesc), vp, sz, vp, vp, vp]),
        "rt_image_put_at": (ci, [vp, vp, vp, sz, vp, ci, ci, vp]),
        "rt_strip_local_rows": (ci, [ci, ci, ci, ci]),
        "rt_deinterleave": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, sz, vp]),
        "rt_wire_bytes": (sz, [sz]),
        "rt_wire_pack": (ci, [vp, vp, vp, vp, vp, sz, vp]),
        "rt_wire_unpack": (ci, [vp, vp, sz, sz, vp, vp, vp, ci, vp, vp, vp, ci, ci, ci, ci, vp]),
        "rt_mgpu_create": (ci, [P(vp), P(ci), ci]),
        "rt_mgpu_destroy": (ci, [vp]),
        "rt_mgpu_device_count": (ci, [vp]),
        "rt_mgpu_set_scene": (ci, [vp, vp, ci, vp, ci]),
        "rt_mgpu_set_noise": (ci, [vp, vp, ci, ci]),
        "rt_mgpu_set_skybox": (ci, [vp, vp, ci]),
        "rt_mgpu_set_strip_rows": (ci, [vp, ci]),
        "rt_mgpu_render": (ci, [vp, params]),
        "rt_mgpu_sync": (ci, [vp]),
        "rt_mgpu_get_surfaces": (ci, [vp, P(vp), P(vp), P(vp), P(vp)]),
        "rt_mgpu_readback": (ci, [vp, vp, vp, vp]),
        "rt_mgpu_last_ms": (ci, [vp, P(cf), ci]),
        "rt_mgpu_last_error": (cs, [vp]),
        "rt_mgpu_context": (ci, [vp, ci, P(vp)]),
    }


SIGNATURES = _signatures()
EXPORTS = list(SIGNATURES)


def load_library(build_if_missing=True):
    """dlopen the in-tree librt_mi355.so (building it first if asked and absent)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = os.environ.get("RT_LIB", _build.LIB_PATH)   # RT_LIB: experiment builds (tools/gpu_explore.py)
    if not os.path.exists(path):
        if not build_if_missing:
            raise RtError(-2, f"{path} not built (run python -m opengl_raytracing_amd.build)")
        _build.build_library()
    lib = ctypes.CDLL(path)
    lib.entry = {}                      # name -> bound function, resolved once: what the _call helpers go through
    for name, (restype, argtypes) in SIGNATURES.items():
        if "RT_LIB" in os.environ and not hasattr(lib, name):
            # an experiment build (tools/gpu_try.py) may predate newer entry points: bind what it has, the rest raises when called
            def fn(*a, name=name):
                raise RtError(-2, f"{name} is not exported by {path}")
            setattr(lib, name, fn)
        else:
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        lib.entry[name] = fn
    _LIB = lib
    return lib


# ---- how the functions below reach the library ---------------------------------------------------
# A context-free entry point goes through _call, one that takes a handle through the handle's _call, one that is launched in the
# order of a torch stream through RayTracer._launch.  There are two stream conventions and both stay: the older methods
# (render_to, the post passes, deinterleave, wire_*) take `stream` as a raw hipStream_t (an int, None = the context's stream) and
# pass it straight through; the newer ones take a torch stream and go through _on_torch_stream.
def _call(name, *args, count=False):
    """The context-free entry point `name`; RtError(rc, name) when it fails.  `count`: it answers a count (returned) or a negative status."""
    rc = (_LIB or load_library()).entry[name](*args)
    if rc < 0 if count else rc:
        raise RtError(rc, name)
    return rc


def _ptr(a):
    """A host address: a numpy array's data, or None."""
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _typed(a, ctype):
    """A numpy array's data as a pointer to `ctype`."""
    return a.ctypes.data_as(ctypes.POINTER(ctype))


def _dev_ptr(x):
    """A device address: a raw pointer (int), anything with data_ptr() (a torch tensor), or None."""
    return ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x)


def _ref(s):
    """byref of a description, or None."""
    return ctypes.byref(s) if s is not None else None


def _tone(tone, white, d_exposure):
    """The optional rt_tone_desc of the pack / submit methods: None unless `tone` or `d_exposure` asks for one."""
    return None if tone is None and d_exposure is None else L.make_tone_desc(tone or "none", white, d_exposure)


def _plane_layout(name, kind, width, height):
    """The two plane offsets and the size that the rt_*_layout entry point `name` answers, as the namedtuple `kind`."""
    off, n = (ctypes.c_size_t * 2)(), ctypes.c_size_t(0)
    _call(name, int(width), int(height), off, ctypes.byref(n))
    return kind(tuple(off), n.value)


# ---- host-side feeders (no GPU) ------------------------------------------------------------
def generate_aabb(objects):
    """GenerateAABBForObject (/root/reference/src/SceneIO.h:75-104), in place."""
    assert objects.dtype == L.OBJECT_DTYPE and objects.flags["C_CONTIGUOUS"]
    _call("rt_generate_aabb", _ptr(objects), len(objects))
    return objects


def camera_vectors(yaw_deg=-90.0, pitch_deg=0.0):
    """Camera::UpdateVectors (/root/reference/src/Camera.h:26-34) -> (front, right, up)."""
    f, r, u = (ctypes.c_float * 3)(), (ctypes.c_float * 3)(), (ctypes.c_float * 3)()
    _call("rt_camera_vectors", yaw_deg, pitch_deg, f, r, u)
    return tuple(f), tuple(r), tuple(u)


def camera_matrices(position, front, up, fov_deg=45.0, aspect=16.0 / 9.0):
    """Camera::GetViewMatrix / GetProjectionMatrix (/root/reference/src/Camera.h:36-42) -> (view[16],
    projection[16]) float32, column-major."""
    a3 = lambda v: (ctypes.c_float * 3)(*[float(x) for x in v])
    view, proj = (ctypes.c_float * 16)(), (ctypes.c_float * 16)()
    _call("rt_camera_matrices", a3(position), a3(front), a3(up), fov_deg, aspect, view, proj)
    return np.array(view, dtype=np.float32), np.array(proj, dtype=np.float32)


def ssao_kernel(seed=0x55A0):
    """The 64 hemisphere samples and the 4x4 rotation texture of AOManager::InitSSAO (AO.cpp:23-51), same
    construction; the reference draws them from std::default_random_engine (implementation-defined
    sequence), this generator uses SplitMix64 -- they are inputs of rt_ssao either way."""
    from .scenes import SplitMix64
    rng = SplitMix64(seed)
    samples = np.zeros((64, 3), dtype=np.float32)
    for i in range(64):
        s = np.array([rng.uniform(0, 1) * 2.0 - 1.0, rng.uniform(0, 1) * 2.0 - 1.0, rng.uniform(0, 1)], dtype=np.float32)
        s = s / np.float32(np.sqrt(np.dot(s, s)))
        s = s * np.float32(rng.uniform(0, 1))
        scale = np.float32(i) / np.float32(64.0)
        scale = np.float32(0.1) + (scale * scale) * np.float32(0.9)
        samples[i] = s * scale
    noise = np.zeros((4, 4, 4), dtype=np.float32)      # uploaded as GL_RGB into RGBA32F: alpha reads 1
    for k in range(16):
        noise[k // 4, k % 4, 0] = rng.uniform(0, 1) * 2.0 - 1.0
        noise[k // 4, k % 4, 1] = rng.uniform(0, 1) * 2.0 - 1.0
    noise[..., 3] = 1.0
    return samples, noise


def parse_scene(text, max_objects=512, max_lights=64):
    """SceneIO::Load (/root/reference/src/SceneIO.h:108-122) on in-memory text."""
    objs = np.zeros(max_objects, dtype=L.OBJECT_DTYPE)
    lts = np.zeros(max_lights, dtype=L.LIGHT_DTYPE)
    no, nl = ctypes.c_int(0), ctypes.c_int(0)
    _call("rt_scene_parse", text.encode("utf-8"), _ptr(objs), max_objects, ctypes.byref(no), _ptr(lts), max_lights, ctypes.byref(nl))
    # (a copy() of a padded record array leaves the padding bytes of the new array uninitialised: assign into zeros instead,
    #  so the same text always gives the same bytes, as the library wrote them)
    out_o, out_l = np.zeros(no.value, dtype=L.OBJECT_DTYPE), np.zeros(nl.value, dtype=L.LIGHT_DTYPE)
    out_o[:], out_l[:] = objs[: no.value], lts[: nl.value]
    return out_o, out_l


def write_scene(objects, lights):
    """SceneIO::Save (/root/reference/src/SceneIO.h:124-142) -> text."""
    objects = np.ascontiguousarray(objects)
    lights = np.ascontiguousarray(lights)
    need = ctypes.c_size_t(0)
    _call("rt_scene_write", _ptr(objects), len(objects), _ptr(lights), len(lights), None, None, None, 0, ctypes.byref(need))
    buf = ctypes.create_string_buffer(need.value)
    _call("rt_scene_write", _ptr(objects), len(objects), _ptr(lights), len(lights), None, None, buf, need.value, ctypes.byref(need))
    return buf.value.decode()


def taa_jitter(frame_count, width, height):
    """uJitterX/uJitterY of /root/reference/src/ForwardShadingPipeline.cpp:241-242."""
    jx, jy = ctypes.c_float(), ctypes.c_float()
    _call("rt_taa_jitter", frame_count, width, height, ctypes.byref(jx), ctypes.byref(jy))
    return jx.value, jy.value


def mesa_math(x):
    """(sin, cos, tan, exp) of float32 x as the HIP path's host side evaluates them (csrc/rt_mesa_math.h)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros((len(x), 4), dtype=np.float32)
    _call("rt_debug_mesa_math", _ptr(x), _ptr(out), len(x))
    return out


def strip_local_rows(height, strip_rows, strip_count, strip_index):
    return _call("rt_strip_local_rows", height, strip_rows, strip_count, strip_index, count=True)


def display_srgb_thresholds():
    """The 256 decision thresholds of the sRGB display format (rt_display_srgb_thresholds): float32, [0] = 0; a colour value
    y in (0, 1) becomes the number of entries 1..255 that are <= y.  Needs no GPU."""
    out = np.zeros(256, dtype=np.float32)
    _call("rt_display_srgb_thresholds", _typed(out, ctypes.c_float))
    return out


def meter_tables():
    """(pow2neg float32[256], log2q16 uint32[8]): the two tables of rt_meter's solve (rt_meter_tables).  Needs no GPU."""
    p, q = np.zeros(256, dtype=np.float32), np.zeros(8, dtype=np.uint32)
    _call("rt_meter_tables", _typed(p, ctypes.c_float), _typed(q, ctypes.c_uint32))
    return p, q


def meter_solve_host(state, width, height, **desc):
    """rt_meter's solve on the host (rt_meter_solve_host): `state` is one METER_STATE_DTYPE record (hist, exposure and frames are
    read, the counters and extremes copied) -> the record rt_meter would leave.  `desc`: make_meter_desc's keywords.  Needs no GPU."""
    src = np.ascontiguousarray(np.asarray(state, dtype=L.METER_STATE_DTYPE).reshape(1))
    out = np.zeros(1, dtype=L.METER_STATE_DTYPE)
    d = L.make_meter_desc(width, height, **desc)
    _call("rt_meter_solve_host", _ptr(src), ctypes.byref(d), _ptr(out))
    return out[0]


YuvLayout = collections.namedtuple("YuvLayout", "offset pitch bytes")
YuvLayout.__doc__ = """rt_display_yuv_layout's answer: byte offsets and row pitches of the Y, Cb and Cr planes (NV12: Cb and Cr interleaved,
offset[2] = offset[1] + 1), and the size of the whole frame."""


def yuv_coeffs(matrix="bt709", range="limited"):
    """The twelve Q16 words of the YUV matrix (rt_display_yuv_coeffs): int32 [cYR, cYG, cYB, yOff, cBR, cBG, cBB, 0, cRR, cRG, cRB, 0].
    Needs no GPU."""
    d = L.make_yuv_desc(1, 1, matrix=matrix, range=range)
    out = np.zeros(12, dtype=np.int32)
    _call("rt_display_yuv_coeffs", d.matrix, d.range, _typed(out, ctypes.c_int32))
    return out


def yuv_layout(width, height, format="nv12"):
    """Where the planes of a width x height NV12 / I420 frame lie (rt_display_yuv_layout) -> YuvLayout.  Needs no GPU."""
    d = L.make_yuv_desc(width, height, format=format)
    off, pitch, n = (ctypes.c_size_t * 3)(), (ctypes.c_size_t * 3)(), ctypes.c_size_t(0)
    _call("rt_display_yuv_layout", ctypes.byref(d), off, pitch, ctypes.byref(n))
    return YuvLayout(tuple(off), tuple(pitch), n.value)


def yuv_planes(frame, width, height, format="nv12"):
    """Views of the planes of one frame (uint8, yuv_layout(...).bytes long): (y[H, W], uv[ch, cw, 2]) for NV12,
    (y[H, W], cb[ch, cw], cr[ch, cw]) for I420."""
    w, h = int(width), int(height)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    lay = yuv_layout(w, h, format)
    frame = np.asarray(frame).reshape(-1)
    assert frame.dtype == np.uint8 and frame.size == lay.bytes
    y = frame[: w * h].reshape(h, w)
    if L.make_yuv_desc(w, h, format=format).format == L.YUV_NV12:
        return y, frame[lay.offset[1]:].reshape(ch, cw, 2)
    return y, frame[lay.offset[1]: lay.offset[2]].reshape(ch, cw), frame[lay.offset[2]:].reshape(ch, cw)


JpegLayout = collections.namedtuple("JpegLayout", "offset scratch_bytes worst_bytes n_mcu n_segments")
JpegLayout.__doc__ = """rt_jpeg_layout's answer: byte offsets of the coefficient plane (int16 [n_mcu * 6, 64], zigzag), of the segment offsets
(uint32 [n_segments + 1]) and of the private region within the scratch, the scratch's size and the largest stream the frame can make."""


def jpeg_dct_matrix():
    """M[u, x] of the encoder's integer DCT (rt_jpeg_dct_matrix): int32 [8, 8].  Needs no GPU."""
    out = np.zeros(64, dtype=np.int32)
    _call("rt_jpeg_dct_matrix", _typed(out, ctypes.c_int32))
    return out.reshape(8, 8)


def jpeg_quant(quality):
    """The two quantisers of `quality` (rt_jpeg_quant) -> (luma uint8 [64], chroma uint8 [64]), natural order.  Needs no GPU."""
    luma, chroma = np.zeros(64, dtype=np.uint8), np.zeros(64, dtype=np.uint8)
    _call("rt_jpeg_quant", int(quality), _typed(luma, ctypes.c_uint8), _typed(chroma, ctypes.c_uint8))
    return luma, chroma


def jpeg_header(width, height, quality=90, restart_interval=None):
    """The 629 bytes in front of the entropy-coded data (rt_jpeg_header) -> uint8 [629].  Needs no GPU."""
    d = L.make_jpeg_desc(width, height, quality, restart_interval)
    out, n = np.zeros(L.JPEG_HEADER_BYTES, dtype=np.uint8), ctypes.c_size_t(0)
    _call("rt_jpeg_header", ctypes.byref(d), _typed(out, ctypes.c_uint8), out.size, ctypes.byref(n))
    return out[:n.value]


def jpeg_layout(width, height, quality=90, restart_interval=None):
    """The scratch of one encode (rt_jpeg_layout) -> JpegLayout.  Needs no GPU."""
    d = L.make_jpeg_desc(width, height, quality, restart_interval)
    off, scratch, worst = (ctypes.c_size_t * 3)(), ctypes.c_size_t(0), ctypes.c_size_t(0)
    _call("rt_jpeg_layout", ctypes.byref(d), off, ctypes.byref(scratch), ctypes.byref(worst))
    n_mcu = ((d.width + 15) // 16) * ((d.height + 15) // 16)
    return JpegLayout(tuple(off), scratch.value, worst.value, n_mcu, (n_mcu + d.restartInterval - 1) // d.restartInterval)


def resample_taps(src, dst, filter="lanczos3"):
    """The tap table of one axis of rt_display_resample, source size `src` -> destination size `dst` (rt_resample_taps):
    (n, first int32[dst], weights float32[dst, n]) -- destination index i reads source pixels clamp(first[i] + k, 0, src - 1),
    k = 0..n-1, with weights[i, k] (zero padding behind a shorter window).  filter "area", "triangle" or "lanczos3".  Needs no GPU."""
    f = int(L.RESAMPLE_FILTERS.get(filter, filter))
    n = ctypes.c_int(0)
    _call("rt_resample_taps", int(src), int(dst), f, ctypes.byref(n), None, None, 0)
    first, weights = np.zeros(int(dst), dtype=np.int32), np.zeros((int(dst), n.value), dtype=np.float32)
    _call("rt_resample_taps", int(src), int(dst), f, ctypes.byref(n), _typed(first, ctypes.c_int32), _typed(weights, ctypes.c_float), weights.size)
    return n.value, first, weights


AccumLayout = collections.namedtuple("AccumLayout", "offset bytes")
AccumLayout.__doc__ = """rt_accum_layout's answer: byte offsets of the accumulator's two planes (the mean, the moments) and its size."""


def accum_layout(width, height):
    """Where the two planes of a width x height accumulator lie (rt_accum_layout) -> AccumLayout.  Needs no GPU."""
    return _plane_layout("rt_accum_layout", AccumLayout, width, height)


def accum_solve_host(state, width, height, **desc):
    """rt_accum_add's solve on the host (rt_accum_solve_host): `state` is one ACCUM_STATE_DTYPE record (hist, nUnsampled,
    nConverged, nPixels and frames are read, the other words copied) -> the record rt_accum_add would leave.  `desc`:
    make_accum_desc's keywords.  Needs no GPU."""
    src = np.ascontiguousarray(np.asarray(state, dtype=L.ACCUM_STATE_DTYPE).reshape(1))
    out = np.zeros(1, dtype=L.ACCUM_STATE_DTYPE)
    d = L.make_accum_desc(width, height, **desc)
    _call("rt_accum_solve_host", _ptr(src), ctypes.byref(d), _ptr(out))
    return out[0]


def accum_select_layout(width, height):
    """The scratch bytes rt_accum_select needs for a width x height accumulator (rt_accum_select_layout).  Needs no GPU."""
    n = ctypes.c_size_t(0)
    _call("rt_accum_select_layout", int(width), int(height), ctypes.byref(n))
    return n.value


def upsample_layout(width, height):
    """The scratch bytes rt_upsample needs for a width x height output (rt_upsample_layout; the same answer as
    accum_select_layout's).  Needs no GPU."""
    n = ctypes.c_size_t(0)
    _call("rt_upsample_layout", int(width), int(height), ctypes.byref(n))
    return n.value


DenoiseLayout = collections.namedtuple("DenoiseLayout", "offset bytes")
DenoiseLayout.__doc__ = """rt_denoise_layout's answer: byte offsets of the two scratch planes of rt_denoise and the size of both."""


def denoise_layout(width, height):
    """Where the two scratch planes of a width x height rt_denoise lie (rt_denoise_layout) -> DenoiseLayout.  Needs no GPU."""
    return _plane_layout("rt_denoise_layout", DenoiseLayout, width, height)


ReprojectLayout = collections.namedtuple("ReprojectLayout", "offset bytes")
ReprojectLayout.__doc__ = """rt_reproject_layout's answer: byte offsets of the two planes of reproject's output accumulator and its size."""


def reproject_layout(width, height):
    """Where the two planes of the accumulator rt_accum_reproject writes lie (rt_reproject_layout; the same answer as accum_layout's)
    -> ReprojectLayout.  Needs no GPU."""
    return _plane_layout("rt_reproject_layout", ReprojectLayout, width, height)


def reproject_project(view, point):
    """rt_accum_reproject's projection on the host (rt_reproject_project): the world position `point` (3 floats) through the
    RtParams `view` -> ((fx, fy) as np.float32 in pixel coordinates, pixel centres at integers; valid: the point lies in front of
    the camera).  Needs no GPU."""
    P3 = (ctypes.c_float * 3)(*[float(x) for x in point])
    f, valid = (ctypes.c_float * 2)(), ctypes.c_int(0)
    _call("rt_reproject_project", ctypes.byref(view), P3, f, ctypes.byref(valid))
    return (np.float32(f[0]), np.float32(f[1])), bool(valid.value)


def reproject_report(d_report):
    """The read-back of a reproject report (a CUDA tensor of 64 bytes; waits for the device) as one layout.REPROJECT_REPORT_DTYPE
    record: nPixels, nReused, nRejected, nOffscreen, nMiss, minCount, maxCount, sumCount."""
    return d_report.cpu().numpy().view(np.uint8).reshape(-1)[:L.REPROJECT_REPORT_BYTES].view(L.REPROJECT_REPORT_DTYPE)[0]


AccelStructure = collections.namedtuple("AccelStructure", "nodes order loose info")
AccelStructure.__doc__ = """rt_accel_build_host's answer: nodes (layout.ACCEL_NODE_DTYPE records, depth-first pre-order), order and loose (uint32
object indices: the leaves' slots, the objects outside the tree) and info (the counts, as accel_info's dict)."""


def _accel_report(r):
    """An rt_accel_report as a dict (launches_accel: (per-wavefront, per-ray))."""
    return dict(built=bool(r.built), nodes=r.nodes, leaves=r.leaves, depth=r.depth, loose=r.loose, bytes=r.bytes, build_ms=r.buildMs,
                builds=r.builds, launches_accel=tuple(r.launchesAccel), launches_brute=r.launchesBrute)


def accel_build_host(objects, desc=None, **kw):
    """The hierarchy RayTracer.set_accel builds for `objects` (OBJECT_DTYPE records), on the host (rt_accel_build_host) ->
    AccelStructure.  `desc`: an RtAccelDesc, or make_accel_desc's keywords.  Needs no GPU."""
    objects = np.ascontiguousarray(objects)
    assert objects.dtype.itemsize == L.OBJECT_STRIDE
    d = desc if desc is not None else L.make_accel_desc(**kw)
    n, info = len(objects), L.RtAccelReport()
    op = _ptr(objects) if n else None
    _call("rt_accel_build_host", op, n, ctypes.byref(d), None, 0, None, 0, None, 0, ctypes.byref(info))
    nodes = np.zeros(info.nodes, dtype=L.ACCEL_NODE_DTYPE)
    order, loose = np.zeros(n - info.loose, dtype=np.uint32), np.zeros(info.loose, dtype=np.uint32)
    _call("rt_accel_build_host", op, n, ctypes.byref(d), _ptr(nodes), len(nodes), _ptr(order), len(order), _ptr(loose), len(loose),
          ctypes.byref(info))
    return AccelStructure(nodes, order, loose, _accel_report(info))


def accel_validate_host(objects, nodes, order, loose, leaf_size=4):
    """True iff the arrays pass the check every structure passes before it is uploaded (rt_accel_validate_host).  Needs no GPU."""
    objects, nodes = np.ascontiguousarray(objects), np.ascontiguousarray(nodes, dtype=L.ACCEL_NODE_DTYPE)
    order, loose = np.ascontiguousarray(order, dtype=np.uint32), np.ascontiguousarray(loose, dtype=np.uint32)
    p = lambda a: _ptr(a) if len(a) else None
    rc = (_LIB or load_library()).entry["rt_accel_validate_host"](p(objects), len(objects), int(leaf_size), p(nodes), len(nodes), p(order), len(order),
                                                                  p(loose), len(loose))
    if rc not in (0, -1):
        raise RtError(rc, "rt_accel_validate_host")
    return rc == 0


PickHit = collections.namedtuple("PickHit", "object t position normal")
PickHit.__doc__ = """rt_pick's answer: object index (-1 = nothing under the pixel), hit distance (tMax on a miss), hit position and
normal (float32[3] each; zero on a miss)."""


# rt_device_math_op of include/rt_mi355.h
DEVICE_MATH_OPS = {"rcp": 0, "rcp3": 1, "sqrt": 2, "rcp_sqrt": 3, "div2": 4, "div3": 5, "mesa": 6, "f2h": 7, "pow5": 8, "halton": 9}


def _query_mode(mode):
    m = {"closest": L.QUERY_CLOSEST, "any": L.QUERY_ANY}.get(mode, mode)
    if m not in (L.QUERY_CLOSEST, L.QUERY_ANY):
        raise ValueError(f"mode must be 'closest' or 'any', not {mode!r}")
    return m


# ---- the device context ---------------------------------------------------------------------
# what the Python side remembers of a present_submit* ticket: "rgba8", "yuv" or "jpeg", the frame's size, the description's format
_PresentTicket = collections.namedtuple("_PresentTicket", "kind width height format")


class _Handle:
    """What RayTracer and MultiGpuRayTracer share: a library (`lib`) and a handle of it (`ctx`) whose entry points begin with _PREFIX
    and take the handle first; its lifetime; the three-surface readback of `_size` pixels."""
    _PREFIX = None

    def _create(self, failure, *args):
        """self.lib and self.ctx from <_PREFIX>create(&ctx, *args); RtError(rc, failure) when that fails."""
        self.lib = load_library()
        self.ctx = ctypes.c_void_p()
        rc = getattr(self.lib, self._PREFIX + "create")(ctypes.byref(self.ctx), *args)
        if rc:
            self.ctx = None
            raise RtError(rc, failure)
        self._size = None                             # (width, height) of the last render: what readback() fetches

    def _check(self, rc, what):
        if rc:
            raise RtError(rc, f"{what}: {getattr(self.lib, self._PREFIX + 'last_error')(self.ctx).decode()}")

    def _call(self, name, *args):
        """The entry point `name` of self.lib on this handle; a failure goes through _check."""
        if rc := self.lib.entry[name](self.ctx, *args):
            self._check(rc, name)

    def close(self):
        if getattr(self, "ctx", None):
            getattr(self.lib, self._PREFIX + "destroy")(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sync(self):
        self._call(self._PREFIX + "sync")

    def readback(self):
        """-> (gColor float32[h,w,4], gPosition float32[h,w,4], gNormal float16[h,w,4]); row 0 = bottom."""
        w, h = self._size
        col = np.empty((h, w, 4), dtype=np.float32)
        pos = np.empty((h, w, 4), dtype=np.float32)
        nrm = np.empty((h, w, 4), dtype=np.float16)
        self._call(self._PREFIX + "readback", _ptr(col), _ptr(pos), _ptr(nrm))
        return col, pos, nrm


class RayTracer(_Handle):
    _PREFIX = "rt_"

    def __init__(self, device=0):
        self._create("rt_create (is a HIP device present?)", device)
        self._present_tickets = {}                    # ticket -> _PresentTicket, for present_wait / present_wait_yuv
        v = int(os.environ.get("RT_VARIANT", "-1"))   # A/B switch for measurements and tests
        if v >= 0:
            self.set_variant(v)

    def set_scene(self, objects, lights):
        objects = np.ascontiguousarray(objects)
        lights = np.ascontiguousarray(lights)
        assert objects.dtype.itemsize == L.OBJECT_STRIDE and lights.dtype.itemsize == L.LIGHT_STRIDE
        self._call("rt_set_scene", _ptr(objects) if len(objects) else None, len(objects), _ptr(lights) if len(lights) else None, len(lights))

    def set_noise(self, r8):
        if r8 is None:
            self._call("rt_set_noise", None, 0, 0)
            return
        r8 = np.ascontiguousarray(r8, dtype=np.uint8)
        self._call("rt_set_noise", _ptr(r8), r8.shape[1], r8.shape[0])

    def set_skybox(self, faces):
        if faces is None:
            self._call("rt_set_skybox", None, 0)
            return
        faces = np.ascontiguousarray(faces, dtype=np.float16)
        assert faces.ndim == 4 and faces.shape[0] == 6 and faces.shape[1] == faces.shape[2] and faces.shape[3] == 3
        self._call("rt_set_skybox", _ptr(faces), faces.shape[1])

    def load(self, scene):
        """Upload a scenes.Scene (objects, lights, noise, skybox)."""
        self.set_scene(scene.objects, scene.lights)
        self.set_noise(scene.noise)
        self.set_skybox(scene.skybox if scene.use_skybox else None)

    def set_variant(self, v):
        self._call("rt_set_variant", int(v))

    def render(self, params):
        self._call("rt_render", ctypes.byref(params))
        self._size = (params.regionW, params.regionH)

    def render_to(self, params, d_color, d_position, d_normal, stream=None):
        """Render into caller-owned device memory (raw device pointers as ints)."""
        self._call("rt_render_to", ctypes.byref(params), _dev_ptr(d_color), _dev_ptr(d_position), _dev_ptr(d_normal), _dev_ptr(stream))

    # ---- ray queries -------------------------------------------------------------------------
    def _launch(self, stream, name, *args, after=()):
        """_call(name, *args, hipStream_t, *after) in the order of torch stream `stream` (_on_torch_stream): the stream handle
        follows `args`, and `after` holds what the entry point takes behind it (the ticket of the present submits)."""
        self._on_torch_stream(stream, lambda h: self._call(name, *args, ctypes.c_void_p(h), *after))

    def _on_torch_stream(self, stream, launch):
        """launch(hipStream_t) asynchronously in the order of torch stream `stream` (default: the current one).  torch's
        default stream has the handle 0, which the C ABI reads as "the context's stream": then the launch goes to the
        context's stream, fenced on both sides with events against torch's stream."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        h = s.cuda_stream if hasattr(s, "cuda_stream") else int(s)
        if h:
            launch(h)
            return
        if not hasattr(self, "_ctx_stream"):
            cs = ctypes.c_void_p()
            self._call("rt_context_stream", ctypes.byref(cs))
            self._ctx_stream = torch.cuda.ExternalStream(cs.value)
        self._ctx_stream.wait_stream(s)
        launch(self._ctx_stream.cuda_stream)
        s.wait_stream(self._ctx_stream)

    def trace_rays(self, rays, mode="closest", out=None, stream=None):
        """Closest-hit ("closest") or any-hit ("any") query of the current scene.

        rays: a CUDA torch tensor float32 [..., 8] (rt_ray per row: origin, tMax, direction, reserved) -> a CUDA torch
        tensor, asynchronous on `stream` (default torch.cuda.current_stream()): closest float32 [..., 8] (rt_hit: position,
        t, normal, object -- the last column holds int32 bits, `.view(torch.int32)[..., 7]`), any int32 [...].  `out`
        may supply it.  Or a numpy array (RAY_DTYPE records or float32 [..., 8]) -> numpy HIT_DTYPE records / int32,
        synchronously."""
        m = _query_mode(mode)
        if isinstance(rays, np.ndarray):
            import torch
            a = np.ascontiguousarray(rays)
            if a.dtype == L.RAY_DTYPE:
                shape, flat = a.shape, a.view(np.float32).reshape(-1, 8)
            else:
                assert a.dtype == np.float32 and a.shape[-1] == 8, "numpy rays: RAY_DTYPE records or float32 [..., 8]"
                shape, flat = a.shape[:-1], a.reshape(-1, 8)
            d = self.trace_rays(torch.from_numpy(flat.copy()).cuda(), m)
            torch.cuda.current_stream().synchronize()
            h = d.cpu().numpy()
            return h.view(L.HIT_DTYPE).reshape(shape) if m == L.QUERY_CLOSEST else h.reshape(shape)
        import torch
        assert rays.is_cuda and rays.dtype == torch.float32 and rays.shape[-1] == 8, "rays: CUDA float32 [..., 8]"
        rays = rays.contiguous()
        shape = tuple(rays.shape[:-1])
        if out is None:
            out = (torch.empty(shape + (8,), dtype=torch.float32, device=rays.device) if m == L.QUERY_CLOSEST
                   else torch.empty(shape, dtype=torch.int32, device=rays.device))
        assert out.is_contiguous() and out.numel() * out.element_size() == rays.numel() // 8 * (32 if m == L.QUERY_CLOSEST else 4)
        n = rays.numel() // 8
        self._launch(stream, "rt_trace_rays", _dev_ptr(rays), n, m, _dev_ptr(out))
        return out

    def camera_rays(self, params, stream=None):
        """The primary rays of render(params): CUDA float32 [regionH, regionW, 8] (rt_ray, surface layout),
        asynchronous on `stream` (default torch.cuda.current_stream())."""
        import torch
        out = torch.empty((params.regionH, params.regionW, 8), dtype=torch.float32, device="cuda")
        self._launch(stream, "rt_camera_rays", ctypes.byref(params), _dev_ptr(out))
        return out

    def camera_rays_at(self, params, d_pixels, n, out=None, stream=None):
        """The primary rays of render(params) for listed image pixels (rt_camera_rays_at): d_pixels holds n rt_pixel records (a raw
        device pointer or a CUDA tensor, 8-byte aligned; e.g. accum_select's list) -> CUDA float32 [n, 8] (rt_ray; `out` may supply
        it, or a raw pointer to write at, which is then returned as given), asynchronous on `stream` (default
        torch.cuda.current_stream()).  The window and strip fields of params are ignored; an entry outside the image gives the
        all-zero ray."""
        import torch
        n = int(n)
        if out is None:
            out = torch.empty((n, 8), dtype=torch.float32, device="cuda")
        self._launch(stream, "rt_camera_rays_at", ctypes.byref(params), _dev_ptr(d_pixels), n, _dev_ptr(out))
        return out

    def shade_rays(self, params, rays, pixels=None, out=None, stream=None, position=True, normal=True):
        """main() of the shader on the given rays (rt_shade_rays): what the renderer computes along each ray.

        rays: CUDA float32 [..., 8] (rt_ray per row, e.g. from camera_rays).  pixels: CUDA int32 / uint32 [..., 2], the
        (x, y) each ray is shaded as (bits read as uint32), or None: rays in camera_rays(params)' surface layout, shaded as
        render(params)'s pixels.  -> (colour float32 [..., 4], position float32 [..., 4] or None, normal float16 [..., 4]
        or None), asynchronous on `stream` (default torch.cuda.current_stream()).  `out` may supply the three tensors (None
        entries are allocated when requested)."""
        import torch
        # every shape / dtype check first, then the device: nothing reaches the ABI unchecked
        if not isinstance(rays, torch.Tensor) or rays.dtype != torch.float32 or rays.ndim < 1 or rays.shape[-1] != 8:
            raise ValueError("rays: a CUDA float32 tensor [..., 8] (rt_ray rows)")
        shape = tuple(rays.shape[:-1])
        n = rays.numel() // 8
        tensors = [rays]
        if pixels is None:
            if n != params.regionW * params.regionH:
                raise ValueError(f"pixels=None: {n} rays, but the window has regionW * regionH = {params.regionW * params.regionH} pixels")
        else:
            ok_dtypes = (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ())
            if not isinstance(pixels, torch.Tensor) or pixels.dtype not in ok_dtypes or pixels.ndim < 1 or pixels.shape[-1] != 2:
                raise ValueError("pixels: a CUDA int32 / uint32 tensor [..., 2]")
            if pixels.numel() != 2 * n:
                raise ValueError(f"pixels: {tuple(pixels.shape)} does not give one (x, y) per ray ({n} rays)")
            tensors.append(pixels)
        col, pos, nrm = out if out is not None else (None, None, None)
        res = []
        for t, on, dt in ((col, True, torch.float32), (pos, position, torch.float32), (nrm, normal, torch.float16)):
            if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_contiguous() or t.numel() != 4 * n):
                raise ValueError(f"out: expected a contiguous CUDA {dt} tensor of {n} x 4 elements")
            if t is not None:
                tensors.append(t)
            res.append(t)
        if not all(t.is_cuda and t.device == rays.device for t in tensors):
            raise ValueError("shade_rays: rays, pixels and out must be CUDA tensors on one device")
        rays = rays.contiguous()
        pixels = pixels.contiguous() if pixels is not None else None
        for k, (on, dt) in enumerate(((True, torch.float32), (position, torch.float32), (normal, torch.float16))):
            if res[k] is None and on:
                res[k] = torch.empty(shape + (4,), dtype=dt, device=rays.device)
        self._launch(stream, "rt_shade_rays", ctypes.byref(params), _dev_ptr(rays), _dev_ptr(pixels), n, *[_dev_ptr(t) for t in res])
        return tuple(res)

    def device_math(self, op, inputs, n=None, out=None):
        """One device-side arithmetic primitive (rt_debug_device_math; `op` a DEVICE_MATH_OPS name or number) on numpy
        records of four 32-bit words: inputs [m, 4] uint32 / int32 / float32 (bits taken as they are) -> uint32 [m, 4],
        synchronously.  Record i runs in lane i % 64 of wavefront i / 64.  `n` < m launches the first n records only and
        `out` (uint32 [>= n, 4]) supplies what the rows the launch does not write keep: the tail tests' sentinels."""
        import torch
        o = DEVICE_MATH_OPS.get(op, op)
        a = np.ascontiguousarray(inputs)
        if a.ndim != 2 or a.shape[1] != 4 or a.dtype.itemsize != 4:
            raise ValueError("inputs: [m, 4] records of 32-bit words")
        n = len(a) if n is None else int(n)
        if not 0 <= n <= len(a):
            raise ValueError(f"n = {n} outside 0..{len(a)}")
        d_in = torch.from_numpy(a.view(np.int32).copy()).cuda()
        if out is None:
            d_out = torch.zeros((len(a), 4), dtype=torch.int32, device="cuda")
        else:
            h = np.ascontiguousarray(out)
            if h.ndim != 2 or h.shape[1] != 4 or h.dtype.itemsize != 4 or len(h) < n:
                raise ValueError("out: [>= n, 4] records of 32-bit words")
            d_out = torch.from_numpy(h.view(np.int32).copy()).cuda()
        self._launch(None, "rt_debug_device_math", int(o), _dev_ptr(d_in), _dev_ptr(d_out), n)
        torch.cuda.current_stream().synchronize()
        return d_out.cpu().numpy().view(np.uint32)

    def pick(self, params, x, y):
        """Closest hit of the primary ray of image pixel (x, y), row 0 = bottom (rt_pick) -> PickHit."""
        h = L.RtHit()
        self._call("rt_pick", ctypes.byref(params), int(x), int(y), ctypes.byref(h))
        return PickHit(h.object, h.t, np.array(h.position, dtype=np.float32), np.array(h.normal, dtype=np.float32))

    def set_accel(self, desc=True, **kw):
        """Switch the hierarchy behind trace_rays / pick on or off (rt_set_accel; sticky).  None / False: off.  True or keywords
        (make_accel_desc's: leaf_size, traversal, min_objects, large_fraction): on; or an RtAccelDesc.  The results of the queries
        do not change, bit for bit."""
        if desc is None or desc is False:
            self._call("rt_set_accel", None)
            return
        d = desc if isinstance(desc, L.RtAccelDesc) else L.make_accel_desc(**kw)
        self._call("rt_set_accel", ctypes.byref(d))

    def accel_info(self):
        """rt_accel_info as a dict: built, nodes, leaves, depth, loose, bytes, build_ms, builds, launches_accel (per-wavefront,
        per-ray), launches_brute."""
        r = L.RtAccelReport()
        self._call("rt_accel_info", ctypes.byref(r))
        return _accel_report(r)

    def set_accel_builder(self, builder="host"):
        """Who builds set_accel's hierarchy (rt_set_accel_builder; sticky, "host" by default): "host", one host thread and median
        splits; "device", HIP kernels on the context's stream and a Morton-code tree -- the same answers from every query, a
        build that no longer grows on the CPU.  A change while the feature is on and a scene is loaded rebuilds at once."""
        self._call("rt_set_accel_builder", int(L.ACCEL_BUILDERS.get(builder, builder)))

    def accel_build_info(self):
        """rt_accel_build_info as a dict: builder (of the structure that stands: "host" / "device", None while none does),
        builds_host, builds_device, host_ms and device_ms of the last build (device_ms waits for it; 0 after a host build)."""
        r = L.RtAccelBuildReport()
        self._call("rt_accel_build_info", ctypes.byref(r))
        built = self.accel_info()["built"]
        return dict(builder=("host", "device")[r.builder] if built else None, builds_host=r.buildsHost, builds_device=r.buildsDevice,
                    host_ms=r.hostMs, device_ms=r.deviceMs)

    def accel_read(self):
        """The structure that stands on the device, from either builder, read back (rt_accel_read; waits for the context's stream)
        -> AccelStructure, as accel_build_host answers; empty arrays while nothing is built."""
        info = L.RtAccelReport()
        self._call("rt_accel_read", None, 0, None, 0, None, 0, ctypes.byref(info))
        n_order = (info.bytes - 32 * info.nodes) // 4 - info.loose          # bytes: 32 per node, 4 per object
        nodes = np.zeros(info.nodes, dtype=L.ACCEL_NODE_DTYPE)
        order, loose = np.zeros(n_order, dtype=np.uint32), np.zeros(info.loose, dtype=np.uint32)
        if info.built:
            self._call("rt_accel_read", _ptr(nodes), len(nodes), _ptr(order), len(order), _ptr(loose), len(loose), ctypes.byref(info))
        return AccelStructure(nodes, order, loose, _accel_report(info))

    def set_accel_shading(self, enable=True, traversal="auto", min_objects=0):
        """Let shade_rays walk the hierarchy set_accel built (rt_set_accel_shading; sticky, off by default, independent of
        set_accel's own switch and of the order of the two calls).  traversal: "auto", "lane", "wave"; min_objects: scenes with fewer
        objects keep the brute-force kernel (0: the default).  The shaded surfaces do not change, bit for bit."""
        if enable is None or enable is False:
            self._call("rt_set_accel_shading", None)
            return
        d = enable if isinstance(enable, L.RtAccelShadeDesc) else L.make_accel_shade_desc(True, traversal, min_objects)
        self._call("rt_set_accel_shading", ctypes.byref(d))

    def accel_shading_info(self):
        """rt_accel_shading_info as a dict: active (the next shade_rays walks the tree), traversal, launches_accel (per-wavefront,
        per-ray), launches_brute (shade launches only; accel_info's counters count the queries)."""
        r = L.RtAccelShadeReport()
        self._call("rt_accel_shading_info", ctypes.byref(r))
        return dict(active=bool(r.active), traversal=r.traversal, launches_accel=tuple(r.launchesAccel), launches_brute=r.launchesBrute)

    def set_accel_render(self, enable=True, traversal="auto", min_objects=0):
        """Let the frames (render, render_to, render_into_image, frame) walk the hierarchy set_accel built (rt_set_accel_render;
        sticky, off by default, independent of the other accel switches and of the order of the calls).  traversal: "auto", "lane",
        "wave", "split" (primary rays per wavefront, every later ray per ray); min_objects: scenes with fewer objects keep the
        packet kernel (0: the default).  The surfaces do not change, bit for bit."""
        if enable is None or enable is False:
            self._call("rt_set_accel_render", None)
            return
        d = enable if isinstance(enable, L.RtAccelRenderDesc) else L.make_accel_render_desc(True, traversal, min_objects)
        self._call("rt_set_accel_render", ctypes.byref(d))

    def accel_render_info(self):
        """rt_accel_render_info as a dict: active (the next plain frame walks the tree), traversal and min_objects (resolved),
        launches_accel (per-wavefront, per-ray, split), launches_packet (frames that kept the existing kernels while the switch was on)."""
        r = L.RtAccelRenderReport()
        self._call("rt_accel_render_info", ctypes.byref(r))
        return dict(active=bool(r.active), traversal=r.traversal, min_objects=r.minObjects, launches_accel=tuple(r.launchesAccel),
                    launches_packet=r.launchesPacket)

    def get_surfaces(self):
        """Device pointers (ints) of the context-owned gColor, gPosition, gNormal of the last rt_render."""
        dc, dp, dn = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._call("rt_get_surfaces", ctypes.byref(dc), ctypes.byref(dp), ctypes.byref(dn))
        return dc.value, dp.value, dn.value

    def last_kernel_ms(self):
        ms = ctypes.c_float()
        self._call("rt_last_kernel_ms", ctypes.byref(ms))
        return ms.value

    def count_rays(self, params):
        n = ctypes.c_uint64()
        self._call("rt_count_rays", ctypes.byref(params), ctypes.byref(n))
        return n.value

    def count_rays_traced(self, params):
        """Rays the production kernel traverses (keeps its dead-ray skips); <= count_rays."""
        n = ctypes.c_uint64()
        self._call("rt_count_rays_traced", ctypes.byref(params), ctypes.byref(n))
        return n.value

    def count_rays_to(self, params, mode, d_color=None, d_position=None, d_normal=None):
        """The instrumented launch of mode 1 (reference rays) or 2 (traced rays) with its frame rendered into caller-owned
        device surfaces (raw device pointers as ints or CUDA tensors, sized like render_to's; all three or none) -> the ray
        total (rt_count_rays_to).  On the context's stream; synchronises."""
        n = ctypes.c_uint64()
        self._call("rt_count_rays_to", ctypes.byref(params), int(mode), _dev_ptr(d_color), _dev_ptr(d_position), _dev_ptr(d_normal),
                   ctypes.byref(n))
        return n.value

    def taa_resolve(self, d_current, d_history, d_normal, d_out, width, height, blend, jx, jy, stream=None):
        """TAA resolve pass on device surfaces (raw device pointers as ints)."""
        self._call("rt_taa_resolve", _dev_ptr(d_current), _dev_ptr(d_history), _dev_ptr(d_normal), _dev_ptr(d_out), width, height,
                   blend, jx, jy, _dev_ptr(stream))

    def bloom(self, d_scene, d_out, width, height, threshold=1.0, strength=0.5, iterations=10, stream=None):
        """Bloom chain on device surfaces (raw device pointers as ints)."""
        self._call("rt_bloom", _dev_ptr(d_scene), _dev_ptr(d_out), width, height, threshold, strength, iterations, _dev_ptr(stream))

    # ---- display packing and delivery to the host ------------------------------------------
    def display_pack(self, d_image, d_out, width, height, format="linear", flip=False, exposure=1.0, stream=None,
                     tone=None, white=1.0, d_exposure=None):
        """rgba32f surface -> RGBA8 on the device (rt_display_pack).  d_image / d_out: raw device pointers (ints) or CUDA
        tensors, 16-byte aligned, not overlapping; d_out holds height * width * 4 bytes (R, G, B, A), row 0 = bottom unless
        `flip`.  format "linear" or "srgb".  Asynchronous on torch stream `stream` (default torch.cuda.current_stream()).
        With `tone` ("none", "reinhard" with `white`, "aces") or `d_exposure` (the address of a device float the exposure is
        multiplied by, e.g. a meter state's + layout.METER_EXPOSURE_OFFSET) the call is rt_display_pack_toned."""
        d = L.make_display_desc(width, height, format, flip, exposure)
        t = _tone(tone, white, d_exposure)
        if t is None:
            self._launch(stream, "rt_display_pack", _dev_ptr(d_image), _dev_ptr(d_out), ctypes.byref(d))
        else:
            self._launch(stream, "rt_display_pack_toned", _dev_ptr(d_image), _dev_ptr(d_out), ctypes.byref(d), ctypes.byref(t))

    def resample(self, d_src, d_dst, src_w, src_h, dst_w, dst_h, filter="lanczos3", stream=None):
        """rgba32f surface src_w x src_h -> rgba32f surface dst_w x dst_h on the device, in linear light, in front of meter /
        display_pack / present_submit (rt_display_resample).  d_src / d_dst: raw device pointers (ints) or CUDA tensors, 16-byte
        aligned, not overlapping.  filter "area" (exact coverage), "triangle" or "lanczos3"; the taps are resample_taps'.
        Asynchronous on torch stream `stream` (default torch.cuda.current_stream())."""
        d = L.make_resample_desc(src_w, src_h, dst_w, dst_h, filter)
        self._launch(stream, "rt_display_resample", _dev_ptr(d_src), _dev_ptr(d_dst), ctypes.byref(d))

    def meter(self, d_image, d_state, width, height, key=0.18, min_exposure=2.0 ** -10, max_exposure=2.0 ** 10, adapt=1.0,
              low_permille=0, high_permille=0, stream=None):
        """Meter the rgba32f surface d_image into the rt_meter_state at d_state (rt_meter; raw device pointers or CUDA tensors,
        16-byte aligned; the state is 1088 bytes, zeroed once by the caller and passed to every later call): histogram of
        log-luminance, trimmed mean, target exposure key / mean, adapted exposure.  Asynchronous on torch stream `stream`
        (default torch.cuda.current_stream()); nothing comes back to the host -- hand the state's exposure to display_pack /
        present_submit as d_exposure = state address + layout.METER_EXPOSURE_OFFSET, or read the state back
        (layout.METER_STATE_DTYPE) when the host wants the figures."""
        d = L.make_meter_desc(width, height, key, min_exposure, max_exposure, adapt, low_permille, high_permille)
        self._launch(stream, "rt_meter", _dev_ptr(d_image), ctypes.byref(d), _dev_ptr(d_state))

    # ---- progressive accumulation ----------------------------------------------------------
    def accum_alloc(self, width, height):
        """(d_accum, d_state): a zeroed accumulator (torch uint8, accum_layout(width, height).bytes: the mean plane, then the
        moments) and a zeroed rt_accum_state (torch uint8, 1024 bytes) on the current device -- empty, ready for accum_add."""
        import torch
        return (torch.zeros(accum_layout(width, height).bytes, dtype=torch.uint8, device="cuda"),
                torch.zeros(L.ACCUM_STATE_BYTES, dtype=torch.uint8, device="cuda"))

    def accum_reset(self, d_accum, d_state, width, height, stream=None):
        """Empty the accumulator and zero the state, `frames` included (rt_accum_reset): two asynchronous memsets on torch
        stream `stream` (default torch.cuda.current_stream())."""
        self._launch(stream, "rt_accum_reset", _dev_ptr(d_accum), _dev_ptr(d_state), int(width), int(height))

    def accum_add(self, d_image, d_accum, d_state, width, height, rel_error=0.02, lum_floor=2.0 ** -10, min_samples=16,
                  done_permille=950, stream=None):
        """One more sample of every pixel (rt_accum_add): the rgba32f surface d_image into the running mean and the luminance
        moments of d_accum, the convergence report of the whole image into d_state (raw device pointers or CUDA tensors, 16-byte
        aligned).  A pixel is converged when it has min_samples samples and the relative standard error of its mean luminance
        (judged against lum_floor where the mean is darker) is at most rel_error; state.done says that done_permille / 1000 of all
        pixels are.  Asynchronous on torch stream `stream` (default torch.cuda.current_stream()); nothing comes back to the host:
        read the 4 bytes at state address + layout.ACCUM_DONE_OFFSET every few frames, or the whole state
        (layout.ACCUM_STATE_DTYPE) when the host wants the figures."""
        d = L.make_accum_desc(width, height, rel_error, lum_floor, min_samples, done_permille)
        self._launch(stream, "rt_accum_add", _dev_ptr(d_image), _dev_ptr(d_accum), ctypes.byref(d), _dev_ptr(d_state))

    # ---- adaptive sampling (the loop: accum_select every k frames; camera_rays_at -> shade_rays -> accum_add_at every frame) ----
    accum_select_layout = staticmethod(accum_select_layout)

    def accum_select_alloc(self, width, height, capacity):
        """(d_pixels, d_scratch, d_sel_state) for accum_select on the current device: the list (torch int32 [capacity, 2], rt_pixel
        rows), the scratch (torch uint8, accum_select_layout(width, height) bytes; its content means nothing) and a zeroed
        rt_select_state (torch uint8, 64 bytes)."""
        import torch
        return (torch.zeros((max(int(capacity), 1), 2), dtype=torch.int32, device="cuda")[:int(capacity)],
                torch.empty(accum_select_layout(width, height), dtype=torch.uint8, device="cuda"),
                torch.zeros(L.SELECT_STATE_BYTES, dtype=torch.uint8, device="cuda"))

    def accum_select(self, d_accum, d_pixels, capacity, d_scratch, d_sel_state, width, height, max_samples=L.SELECT_MAX_SAMPLES,
                     rel_error=0.02, lum_floor=2.0 ** -10, min_samples=16, done_permille=950, stream=None):
        """The pixels of d_accum that still need samples (rt_accum_select): unconverged by accum_add's rule and with fewer than
        max_samples samples, as rt_pixel records in tile order (8 x 8 tiles in raster order, raster order inside a tile) at d_pixels
        -- the first min(nSelected, capacity) of them; capacity 0 counts only and d_pixels may be None.  d_sel_state receives the 64
        bytes of rt_select_state (layout.SELECT_STATE_DTYPE).  Raw device pointers or CUDA tensors; asynchronous on `stream`
        (default torch.cuda.current_stream()), no host synchronisation."""
        d = L.make_accum_desc(width, height, rel_error, lum_floor, min_samples, done_permille)
        self._launch(stream, "rt_accum_select", _dev_ptr(d_accum), ctypes.byref(d), int(max_samples), _dev_ptr(d_pixels), int(capacity),
                     _dev_ptr(d_scratch), _dev_ptr(d_sel_state))

    def accum_add_at(self, d_samples, d_pixels, n, d_accum, d_state, width, height, rel_error=0.02, lum_floor=2.0 ** -10, min_samples=16,
                     done_permille=950, stream=None):
        """One more sample of the n listed pixels only (rt_accum_add_at): d_samples[k] (rgba32f, e.g. shade_rays' colour) goes into
        pixel d_pixels[k] of d_accum by accum_add's arithmetic, no other pixel is written, and d_state receives accum_add's report
        over every pixel, `frames` advanced.  n = 0 refreshes the report only (d_samples and d_pixels may be None).  A pixel may be
        listed at most once.  Raw device pointers or CUDA tensors; asynchronous on `stream` (default torch.cuda.current_stream())."""
        d = L.make_accum_desc(width, height, rel_error, lum_floor, min_samples, done_permille)
        self._launch(stream, "rt_accum_add_at", _dev_ptr(d_samples), _dev_ptr(d_pixels), int(n), _dev_ptr(d_accum), ctypes.byref(d),
                     _dev_ptr(d_state))

    # ---- first-hit-guided upsampling (the loop: render low; first hits at both sizes; upsample; camera_rays_at -> shade_rays ->
    # image_put_at on the holes) ----
    upsample_layout = staticmethod(upsample_layout)

    def upsample(self, d_low, d_hits_low, d_hits_high, d_out, d_pixels, capacity, d_scratch, d_sel_state, width, height, low_width,
                 low_height, normal_log2_power=5, min_weight=0.25, stream=None):
        """The low_width x low_height rgba32f surface d_low reconstructed at width x height into d_out (rt_upsample), guided by the
        first hits of both sizes (d_hits_low, d_hits_high: trace_rays(camera_rays(params)) of the two rt_params): a pixel is
        interpolated from the 2 x 2 low-resolution pixels of its own object, or is a hole -- filled from the 4 x 4 window as a
        stand-in and listed at d_pixels (rt_pixel records in accum_select's tile order, the first min(holes, capacity) of them;
        capacity 0 counts only and d_pixels may be None).  d_scratch: upsample_layout(width, height) bytes; d_sel_state receives the 64
        bytes of rt_select_state (layout.SELECT_STATE_DTYPE): nSelected = the holes, nCapped = those without any pixel of their
        object in the window.  accum_select_alloc allocates the three.  Raw device pointers or CUDA tensors; asynchronous on `stream`
        (default torch.cuda.current_stream()), no host synchronisation."""
        d = L.make_upsample_desc(width, height, low_width, low_height, normal_log2_power, min_weight)
        self._launch(stream, "rt_upsample", _dev_ptr(d_low), _dev_ptr(d_hits_low), _dev_ptr(d_hits_high), _dev_ptr(d_out), ctypes.byref(d),
                     _dev_ptr(d_pixels), int(capacity), _dev_ptr(d_scratch), _dev_ptr(d_sel_state))

    def image_put_at(self, d_samples, d_pixels, n, d_image, width, height, stream=None):
        """d_image[d_pixels[k]] = d_samples[k] for the n listed pixels (rt_image_put_at): shade_rays' colours of upsample's holes
        into the width x height rgba32f surface.  An entry outside the image is skipped; n = 0 is a no-op (d_samples and d_pixels
        may be None).  Raw device pointers or CUDA tensors; asynchronous on `stream` (default torch.cuda.current_stream())."""
        self._launch(stream, "rt_image_put_at", _dev_ptr(d_samples), _dev_ptr(d_pixels), int(n), _dev_ptr(d_image), int(width), int(height))

    def accum_view(self, d_accum, d_out, width, height, mode="relerr", rel_error=0.02, lum_floor=2.0 ** -10, min_samples=16,
                   done_permille=950, stream=None):
        """A heat map of the accumulator as an rgba32f surface (v, v, v, 1) at d_out (rt_accum_view): mode "relerr" (the relative
        standard error, +inf where a pixel has fewer than 2 samples), "count" (samples) or "converged" (1 or 0, by accum_add's
        rule for the same keywords).  Asynchronous on torch stream `stream`."""
        d = L.make_accum_desc(width, height, rel_error, lum_floor, min_samples, done_permille)
        m = int(L.ACCUM_VIEWS.get(mode, mode))
        self._launch(stream, "rt_accum_view", _dev_ptr(d_accum), _dev_ptr(d_out), ctypes.byref(d), m)

    # ---- denoising ------------------------------------------------------------------------
    def denoise_guide(self, d_hits, width, height, out=None, stream=None):
        """The guide plane of rt_denoise from first-hit records (rt_denoise_guide): d_hits is trace_rays(camera_rays(params))'s
        CUDA tensor (or a raw device pointer) of width * height rt_hit -> a CUDA uint8 tensor of width * height
        layout.DENOISE_GUIDE_DTYPE records (`out` may supply it), asynchronous on torch stream `stream` (default
        torch.cuda.current_stream()).  Made once per still view."""
        import torch
        if out is None:
            out = torch.empty(int(width) * int(height) * 16, dtype=torch.uint8, device="cuda")
        self._launch(stream, "rt_denoise_guide", _dev_ptr(d_hits), _dev_ptr(out), int(width), int(height))
        return out

    def denoise_alloc(self, width, height):
        """(d_scratch, d_out): the two scratch planes of denoise (torch uint8, denoise_layout(width, height).bytes) and an rgba32f
        output surface (torch float32 [height, width, 4]) on the current device."""
        import torch
        return (torch.empty(denoise_layout(width, height).bytes, dtype=torch.uint8, device="cuda"),
                torch.empty((int(height), int(width), 4), dtype=torch.float32, device="cuda"))

    def denoise(self, d_image, d_moments, d_guide, d_scratch, d_out, width, height, iterations=4, normal_log2_power=5, sigma_lum=4.0,
                lum_eps=2.0 ** -10, min_count=4, stream=None):
        """The variance-guided a-trous filter (rt_denoise): the rgba32f surface d_image -- the accumulator's plane 0, or one raw
        frame -- with the accumulator's plane 1 as d_moments (None: the variance is estimated spatially) and denoise_guide's plane
        as d_guide, through the scratch planes d_scratch into the rgba32f surface d_out, which rt_meter, rt_display_resample, every
        pack and every present submit take as it stands.  Raw device pointers or CUDA tensors, 16-byte aligned; asynchronous on
        torch stream `stream` (default torch.cuda.current_stream()): 1 + iterations launches, no host synchronisation."""
        d = L.make_denoise_desc(width, height, iterations, normal_log2_power, sigma_lum, lum_eps, min_count)
        self._launch(stream, "rt_denoise", _dev_ptr(d_image), _dev_ptr(d_moments), _dev_ptr(d_guide), _dev_ptr(d_scratch), _dev_ptr(d_out),
                     ctypes.byref(d))

    # ---- reprojection ------------------------------------------------------------------------
    def reproject(self, d_accum_prev, d_hits_prev, d_hits_cur, d_accum_cur, d_report, prev, cur, normal_cos_min=0.9, plane_tol=0.01,
                  max_history=32, stream=None):
        """Carry the accumulator of the view `prev` over to the view `cur` (rt_accum_reproject; both RtParams of one size): every
        current pixel keeps the history its first hit (d_hits_cur) finds on its own surface in the previous view's hits and
        accumulator, capped at max_history samples, or becomes empty; d_accum_cur is written in full and is accum_add's,
        denoise's and the display path's input as it stands, d_report takes the 64-byte report (reproject_report reads it).  Raw
        device pointers or CUDA tensors, 16-byte aligned; asynchronous on torch stream `stream` (default
        torch.cuda.current_stream()): a clear and one launch, no host synchronisation.  The caller swaps the accumulators and
        the hits afterwards."""
        d = L.make_reproject_desc(prev, cur, normal_cos_min, plane_tol, max_history)
        self._launch(stream, "rt_accum_reproject", _dev_ptr(d_accum_prev), _dev_ptr(d_hits_prev), _dev_ptr(d_hits_cur),
                     _dev_ptr(d_accum_cur), ctypes.byref(d), _dev_ptr(d_report))

    reproject_layout = staticmethod(reproject_layout)
    reproject_project = staticmethod(reproject_project)
    reproject_report = staticmethod(reproject_report)

    @staticmethod
    def accum_moments(d_accum, width, height):
        """Plane 1 of an accum_alloc accumulator, the luminance moments, as a uint8 tensor that shares its memory: denoise's
        d_moments."""
        n = int(width) * int(height) * 16
        return d_accum[n: 2 * n]

    @staticmethod
    def accum_mean(d_accum, width, height):
        """Plane 0 of an accum_alloc accumulator, the running mean, as a float32 [height, width, 4] tensor that shares its
        memory: what meter, resample, display_pack* and present_submit* take as it stands."""
        import torch
        n = int(width) * int(height) * 16
        return d_accum[:n].view(torch.float32).view(int(height), int(width), 4)

    def present_configure(self, slots):
        """Number of frames that can be on their way to the host at once (2..8, default 3); expires every earlier ticket and
        is refused while one is outstanding (submitted, not yet waited for or polled ready)."""
        self._call("rt_present_configure", int(slots))

    def present_submit(self, d_image, width, height, format="linear", flip=False, exposure=1.0, stream=None,
                       tone=None, white=1.0, d_exposure=None):
        """Pack the rgba32f surface d_image (raw device pointer or CUDA tensor) as display_pack does (`tone`, `white` and
        `d_exposure` included: rt_present_submit_toned) and start its copy into a pinned host buffer -> ticket (0, 1, 2, ...).
        Ordered on torch stream `stream` (default torch.cuda.current_stream()): later work on that stream may overwrite d_image
        at once, and the copy overlaps it.  Does not block the host."""
        d = L.make_display_desc(width, height, format, flip, exposure)
        td, t = _tone(tone, white, d_exposure), ctypes.c_uint64()
        if td is None:
            self._launch(stream, "rt_present_submit", _dev_ptr(d_image), ctypes.byref(d), after=(ctypes.byref(t),))
        else:
            self._launch(stream, "rt_present_submit_toned", _dev_ptr(d_image), ctypes.byref(d), ctypes.byref(td), after=(ctypes.byref(t),))
        self._present_issued(t.value, "rgba8", width, height, d.format)
        return t.value

    def present_poll(self, ticket):
        """True once present_wait(ticket) would not block."""
        ready = ctypes.c_int(0)
        self._call("rt_present_poll", int(ticket), ctypes.byref(ready))
        return bool(ready.value)

    def present_wait(self, ticket, copy=True):
        """Block until the frame of `ticket` is in host memory -> uint8 [height, width, 4].  copy=False returns a read-only
        view of the ring's pinned slot instead: valid until the present_submit that returns ticket + slots (or
        present_configure, or close()), after which its memory is rewritten or gone -- copy what must outlive that."""
        rec = self._present_tickets.get(int(ticket))
        if rec is not None and rec.kind == "yuv":
            raise ValueError(f"ticket {int(ticket)} is a YUV frame (present_submit_yuv): wait for it with present_wait_yuv")
        if rec is not None and rec.kind == "jpeg":
            raise ValueError(f"ticket {int(ticket)} is a JPEG stream (present_submit_jpeg): wait for it with present_wait_jpeg")
        view = self._present_pinned(ticket, copy)
        rec = self._present_tickets[int(ticket)]
        assert view.size == rec.height * rec.width * 4
        return view.reshape(rec.height, rec.width, 4)

    def _present_issued(self, ticket, kind, width, height, format):
        """Remember what `ticket` holds; forget the tickets no ring can still hold (one rule: 16 back, twice the largest ring)."""
        self._present_tickets[ticket] = _PresentTicket(kind, int(width), int(height), format)
        for old in [k for k in self._present_tickets if k + 16 <= ticket]:
            del self._present_tickets[old]

    def _present_pinned(self, ticket, copy):
        """rt_present_wait -> the ticket's bytes, uint8 [n]: a copy, or a read-only view of the ring's pinned slot."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t(0)
        self._call("rt_present_wait", int(ticket), ctypes.byref(p), ctypes.byref(n))
        view = np.frombuffer((ctypes.c_uint8 * n.value).from_address(p.value), dtype=np.uint8)
        if copy:
            return view.copy()
        view.flags.writeable = False
        return view

    # ---- YUV 4:2:0 output: the frame a video encoder takes ------------------------------------
    def display_pack_yuv(self, d_image, d_out, width, height, format="nv12", matrix="bt709", range="limited", transfer="srgb",
                         flip=False, exposure=1.0, tone=None, white=1.0, d_exposure=None, stream=None):
        """rgba32f surface -> NV12 or I420 on the device (rt_display_pack_yuv).  d_image / d_out: raw device pointers or CUDA
        tensors, 16-byte aligned, not overlapping; d_out holds yuv_layout(width, height, format).bytes.  The R'G'B' codes are
        display_pack's for format=`transfer` with the same `exposure`, `tone`, `white` and `d_exposure`; matrix "bt709" / "bt601",
        range "limited" / "full"; `flip` makes output row 0 the top image row.  Asynchronous on torch stream `stream`."""
        d = L.make_yuv_desc(width, height, format, matrix, range, transfer, flip, exposure)
        self._launch(stream, "rt_display_pack_yuv", _dev_ptr(d_image), _dev_ptr(d_out), ctypes.byref(d), _ref(_tone(tone, white, d_exposure)))

    def present_submit_yuv(self, d_image, width, height, format="nv12", matrix="bt709", range="limited", transfer="srgb",
                           flip=False, exposure=1.0, tone=None, white=1.0, d_exposure=None, stream=None):
        """present_submit with display_pack_yuv's frame: same ring, same ticket sequence.  Wait for the ticket with present_wait_yuv."""
        d = L.make_yuv_desc(width, height, format, matrix, range, transfer, flip, exposure)
        t = ctypes.c_uint64()
        self._launch(stream, "rt_present_submit_yuv", _dev_ptr(d_image), ctypes.byref(d), _ref(_tone(tone, white, d_exposure)),
                     after=(ctypes.byref(t),))
        self._present_issued(t.value, "yuv", width, height, d.format)
        return t.value

    def present_wait_yuv(self, ticket, copy=True):
        """Block until the YUV frame of `ticket` is in host memory -> (y[H, W], uv[ch, cw, 2]) for NV12, (y[H, W], cb[ch, cw],
        cr[ch, cw]) for I420, uint8.  copy=False returns read-only views of the ring's pinned slot (present_wait's rules)."""
        rec = self._present_tickets.get(int(ticket))
        if rec is not None and rec.kind == "jpeg":
            raise ValueError(f"ticket {int(ticket)} is a JPEG stream (present_submit_jpeg), not a YUV frame: wait for it with present_wait_jpeg")
        if rec is None or rec.kind != "yuv":
            raise ValueError(f"ticket {int(ticket)} is not a live YUV frame of present_submit_yuv (RGBA8 tickets: present_wait)")
        frame = self._present_pinned(ticket, copy)
        if frame.size != yuv_layout(rec.width, rec.height, rec.format).bytes:
            raise RtError(-1, f"ticket {int(ticket)} holds {frame.size} bytes, not a {rec.width}x{rec.height} YUV frame")
        return yuv_planes(frame, rec.width, rec.height, rec.format)

    # ---- baseline JPEG output: the file a viewer, a browser or a disk takes ------------------------
    def jpeg_layout(self, width, height, quality=90, restart_interval=None):
        """host.jpeg_layout: the scratch jpeg_encode and display_pack_jpeg work in."""
        return jpeg_layout(width, height, quality, restart_interval)

    def jpeg_encode(self, d_planes, d_scratch, d_out, cap_bytes, d_state, width, height, format="nv12", quality=90, restart_interval=None,
                    stream=None):
        """NV12 / I420 planes of display_pack_yuv (row 0 = the file's top row) -> a baseline JPEG stream in d_out, at most cap_bytes
        long, and one layout.JPEG_STATE_DTYPE record in d_state (rt_jpeg_encode).  d_scratch holds jpeg_layout(...).scratch_bytes.
        Raw device pointers or CUDA tensors, 16-byte aligned, not overlapping.  Asynchronous on torch stream `stream`."""
        yd = L.make_yuv_desc(width, height, format, "bt601", "full")
        jd = L.make_jpeg_desc(width, height, quality, restart_interval)
        self._launch(stream, "rt_jpeg_encode", _dev_ptr(d_planes), ctypes.byref(yd), ctypes.byref(jd), _dev_ptr(d_scratch), _dev_ptr(d_out),
                     int(cap_bytes), _dev_ptr(d_state))

    def display_pack_jpeg(self, d_image, d_scratch, d_out, cap_bytes, d_state, width, height, format="nv12", quality=90, restart_interval=None,
                          transfer="srgb", flip=True, exposure=1.0, tone=None, white=1.0, d_exposure=None, stream=None):
        """rgba32f surface -> JPEG stream on the device (rt_display_pack_jpeg): display_pack_yuv (full-range BT.601, planes in
        `format`) into the scratch, then jpeg_encode.  flip=True (the default here) makes the file upright."""
        yd = L.make_yuv_desc(width, height, format, "bt601", "full", transfer, flip, exposure)
        jd = L.make_jpeg_desc(width, height, quality, restart_interval)
        self._launch(stream, "rt_display_pack_jpeg", _dev_ptr(d_image), ctypes.byref(yd), _ref(_tone(tone, white, d_exposure)), ctypes.byref(jd),
                     _dev_ptr(d_scratch), _dev_ptr(d_out), int(cap_bytes), _dev_ptr(d_state))

    def present_submit_jpeg(self, d_image, width, height, cap_bytes=0, format="nv12", quality=90, restart_interval=None, transfer="srgb",
                            flip=True, exposure=1.0, tone=None, white=1.0, d_exposure=None, stream=None):
        """present_submit with display_pack_jpeg's stream: same ring, same ticket sequence; the slot holds the state record and up
        to cap_bytes of stream (0: the frame's worst case).  Wait for the ticket with present_wait_jpeg."""
        yd = L.make_yuv_desc(width, height, format, "bt601", "full", transfer, flip, exposure)
        jd = L.make_jpeg_desc(width, height, quality, restart_interval)
        t = ctypes.c_uint64()
        self._launch(stream, "rt_present_submit_jpeg", _dev_ptr(d_image), ctypes.byref(yd), _ref(_tone(tone, white, d_exposure)), ctypes.byref(jd),
                     int(cap_bytes), after=(ctypes.byref(t),))
        self._present_issued(t.value, "jpeg", width, height, yd.format)
        return t.value

    def present_wait_jpeg(self, ticket, copy=True):
        """Block until the JPEG stream of `ticket` is in host memory -> uint8 [bytes], the whole file.  Raises RtError when the
        stream did not fit the submit's cap_bytes (the message says how many bytes it needed).  copy=False returns a read-only
        view of the ring's pinned slot (present_wait's rules)."""
        rec = self._present_tickets.get(int(ticket))
        if rec is None or rec.kind != "jpeg":
            raise ValueError(f"ticket {int(ticket)} is not a live JPEG stream of present_submit_jpeg")
        slot = self._present_pinned(ticket, False)
        state = slot[:L.JPEG_STATE_BYTES].view(L.JPEG_STATE_DTYPE)[0]
        if state["overflow"]:
            raise RtError(-4, f"ticket {int(ticket)}: the stream needed {int(state['needed'])} bytes, the slot held {slot.size - L.JPEG_STATE_BYTES}")
        stream = slot[L.JPEG_STATE_BYTES: L.JPEG_STATE_BYTES + int(state["bytes"])]
        return stream.copy() if copy else stream

    def tile_costs(self):
        """(costs[tilesY, tilesX] uint32, cycles/64 per tile) of the last feedback-scheduled launch."""
        n, tx = ctypes.c_int(0), ctypes.c_int(0)
        probe = (ctypes.c_uint32 * 1)()
        self._call("rt_debug_tile_costs", probe, 0, ctypes.byref(n), ctypes.byref(tx))
        if n.value == 0:
            return np.zeros((0, 0), dtype=np.uint32)
        out = (ctypes.c_uint32 * n.value)()
        self._call("rt_debug_tile_costs", out, n.value, ctypes.byref(n), ctypes.byref(tx))
        return np.frombuffer(out, dtype=np.uint32).reshape(-1, tx.value).copy()

    def frame(self, params, enable_ao=True, enable_taa=True, taa_blend=0.1, bloom_threshold=1.0, bloom_strength=0.5,
              bloom_iterations=10, ao_samples=None, ao_noise=None, d_display=None):
        """One iteration of the reference's Render() GPU work (ray trace, AO, bloom, TAA) on the context's surfaces."""
        d = RtFrameDesc()
        d.enableAO, d.enableTAA, d.taaBlendFactor = int(bool(enable_ao)), int(bool(enable_taa)), taa_blend
        d.bloomThreshold, d.bloomStrength, d.bloomIterations = bloom_threshold, bloom_strength, bloom_iterations
        keep = []
        if enable_ao:
            if ao_samples is None or ao_noise is None:
                ao_samples, ao_noise = ssao_kernel()
            for name, arr, n in (("aoSamples", ao_samples, 192), ("aoNoise", ao_noise, 64)):
                a = np.ascontiguousarray(arr, dtype=np.float32).reshape(n)
                keep.append(a)
                setattr(d, name, _typed(a, ctypes.c_float))
        self._call("rt_frame", ctypes.byref(params), ctypes.byref(d), _dev_ptr(d_display))

    def frame_surfaces(self):
        """(dColor, dPosition, dNormal, dAO, dHistory) device pointers (ints or None) after rt_frame."""
        ptrs = [ctypes.c_void_p() for _ in range(5)]
        self._call("rt_frame_surfaces", *[ctypes.byref(q) for q in ptrs])
        return tuple(q.value for q in ptrs)

    def equirect_to_cubemap(self, equirect_rgb, size, d_faces_out=None, install=False):
        """ConvertHDRToCubemap: equirect f32[h,w,3] (row 0 = bottom) -> six RGB16F faces on the device
        (d_faces_out: raw pointer, 6*size*size*3 halfs) and / or installed as this context's skybox."""
        e = np.ascontiguousarray(equirect_rgb, dtype=np.float32)
        h, w = e.shape[:2]
        self._call("rt_equirect_to_cubemap", _typed(e, ctypes.c_float), w, h, size, _dev_ptr(d_faces_out), int(bool(install)))

    def ssao(self, d_position, d_normal, d_out, width, height, noise, samples, projection, view, stream=None):
        """SSAO on the G-buffer surfaces (raw device pointers as ints); noise [nh,nw,4], samples [64,3],
        matrices [16] are host arrays."""
        fa = lambda x, n: np.ascontiguousarray(x, dtype=np.float32).reshape(n)
        noise = np.ascontiguousarray(noise, dtype=np.float32)
        nh, nw = noise.shape[:2]
        fp = lambda x: _typed(x, ctypes.c_float)
        nz, sm, pj, vw = fa(noise, nh * nw * 4), fa(samples, 192), fa(projection, 16), fa(view, 16)
        self._call("rt_ssao", _dev_ptr(d_position), _dev_ptr(d_normal), _dev_ptr(d_out), width, height, fp(nz), nw, nh, fp(sm), fp(pj),
                   fp(vw), _dev_ptr(stream))

    def ssao_blur(self, d_in, d_out, width, height, horizontal=False, stream=None):
        self._call("rt_ssao_blur", _dev_ptr(d_in), _dev_ptr(d_out), width, height, int(bool(horizontal)), _dev_ptr(stream))

    def predicted_classes(self, n_tiles):
        """Cost classes (uint8[n_tiles], raster tile order) of the last predicted launch."""
        out = np.zeros(n_tiles, dtype=np.uint8)
        n = ctypes.c_int(0)
        self._call("rt_debug_predicted_classes", _ptr(out), n_tiles, ctypes.byref(n))
        return out

    def tile_order(self):
        """(order uint32[nTiles], policy) of the last packet launch (rt_debug_tile_order): order[k] = the tile workgroup k rendered,
        policy 0 raster / 1 measured / 2 predicted / 3 phase.  An empty order unless the context was created with
        RT_DEBUG_TILE_ORDER=1; the last launch's only if the caller synchronises between frames."""
        n, policy = ctypes.c_int(0), ctypes.c_int(0)
        probe = np.zeros(1, dtype=np.uint32)
        self._call("rt_debug_tile_order", _typed(probe, ctypes.c_uint32), 0, ctypes.byref(n), ctypes.byref(policy))
        out = np.zeros(max(n.value, 1), dtype=np.uint32)
        self._call("rt_debug_tile_order", _typed(out, ctypes.c_uint32), n.value, ctypes.byref(n), ctypes.byref(policy))
        return out[:n.value], policy.value

    def lpt_sort(self, costs, accum=None):
        """rt_lpt_sort_kernel on the given tile costs (rt_debug_lpt_sort) -> (order uint32[n], costs as the kernel leaves them,
        accum + costs or None).  The arguments are not modified."""
        u32p = lambda a: _typed(a, ctypes.c_uint32)
        costs = np.array(costs, dtype=np.uint32).reshape(-1)
        order = np.zeros(costs.size, dtype=np.uint32)
        if accum is not None:
            accum = np.array(accum, dtype=np.uint32).reshape(-1)
            assert accum.size == costs.size
        self._call("rt_debug_lpt_sort", u32p(costs), costs.size, u32p(order), u32p(accum) if accum is not None else None)
        return order, costs, accum

    def split_tiles(self):
        """P per tile (uint8[nTiles], raster tile order; 0 = the tile ran whole) of the last replaying launch's split plan
        (rt_debug_split_tiles); empty before the first replaying launch."""
        n = ctypes.c_int(0)
        probe = np.zeros(1, dtype=np.uint8)
        self._call("rt_debug_split_tiles", _typed(probe, ctypes.c_uint8), 0, ctypes.byref(n))
        out = np.zeros(max(n.value, 1), dtype=np.uint8)
        self._call("rt_debug_split_tiles", _typed(out, ctypes.c_uint8), n.value, ctypes.byref(n))
        return out[:n.value]

    def split_plan(self, order, costs, wave_slots, depth, n_lights, force_parts=0, prev_parts=None):
        """rt_split_plan_kernel on the given order and costs (rt_debug_split_plan) -> (parts uint8[n], slot uint32[n],
        extra uint32[1536], (extra jobs, split tiles))."""
        order = np.ascontiguousarray(order, dtype=np.uint32).reshape(-1)
        costs = np.ascontiguousarray(costs, dtype=np.uint32).reshape(-1)
        assert order.size == costs.size
        parts, slot = np.zeros(order.size, dtype=np.uint8), np.zeros(order.size, dtype=np.uint32)
        extra, counts = np.zeros(1536, dtype=np.uint32), np.zeros(2, dtype=np.uint32)
        prev = None
        if prev_parts is not None:
            prev_parts = np.ascontiguousarray(prev_parts, dtype=np.uint8).reshape(-1)
            assert prev_parts.size == order.size
            prev = _typed(prev_parts, ctypes.c_uint8)
        self._call("rt_debug_split_plan", _typed(order, ctypes.c_uint32), _typed(costs, ctypes.c_uint32), order.size, int(wave_slots), int(depth),
                   int(n_lights), int(force_parts), prev, _typed(parts, ctypes.c_uint8), _typed(slot, ctypes.c_uint32),
                   _typed(extra, ctypes.c_uint32), _typed(counts, ctypes.c_uint32))
        return parts, slot, extra, (int(counts[0]), int(counts[1]))

    def shadow_tables(self):
        """(dwords uint32[n], words per cell) of the current scene's shadow tables (headers + cells), or (None, 0)."""
        n, w = ctypes.c_size_t(0), ctypes.c_int(0)
        self._call("rt_debug_shadow_tables", None, 0, ctypes.byref(n), ctypes.byref(w))
        if n.value == 0:
            return None, 0
        out = np.zeros(n.value, dtype=np.uint32)
        self._call("rt_debug_shadow_tables", _ptr(out), n.value, ctypes.byref(n), ctypes.byref(w))
        return out, w.value

    def _counters(self, name, n):
        """The n uint64 counters that the rt_debug_* entry point `name` fills, as a list."""
        out = (ctypes.c_uint64 * n)()
        self._call(name, out)
        return list(out)

    def debug_stats(self):
        return self._counters("rt_debug_stats", 4)

    def debug_stats_ex(self):
        return self._counters("rt_debug_stats_ex", 32)

    def debug_first_hit(self):
        """[normal, recorded, replayed] packet-kernel frames of this context since its creation (first-hit reuse)."""
        return self._counters("rt_debug_first_hit", 3)

    def debug_settled_tiles(self):
        """[tiles of the cached first-hit window, settled ones among them]; zeros without a valid cache."""
        return self._counters("rt_debug_settled_tiles", 2)

    def debug_settled_map(self):
        """The cached window's settled flags, one uint8 per 8x8 tile in row-major tile order (empty without a valid cache)."""
        n = self.debug_settled_tiles()[0]
        flags = (ctypes.c_uint8 * max(n, 1))()
        self._call("rt_debug_settled_map", flags, n)
        return np.frombuffer(flags, dtype=np.uint8, count=n).copy()

    def debug_prefix_tiles(self):
        """[settled tiles, tiles that resume at depth K = 0 .. 7] of the cached first-hit window; zeros without a valid cache."""
        return self._counters("rt_debug_prefix_tiles", 9)

    def deinterleave(self, d_src, d_dst, width, height, bytes_per_pixel, strip_rows, strip_count,
                     rank_stride_bytes, stream=None):
        self._call("rt_deinterleave", _dev_ptr(d_src), _dev_ptr(d_dst), width, height, bytes_per_pixel, strip_rows, strip_count,
                   rank_stride_bytes, _dev_ptr(stream))

    def wire_pack(self, d_color, d_pos, d_normal, d_wire, n_pixels, stream=None):
        """This rank's three surfaces -> the 30 B/pixel gather wire format (device pointers as ints)."""
        self._call("rt_wire_pack", _dev_ptr(d_color), _dev_ptr(d_pos), _dev_ptr(d_normal), _dev_ptr(d_wire), n_pixels, _dev_ptr(stream))

    def wire_unpack(self, d_wire, rank_stride_bytes, rank_pixels, d_color, d_pos, d_normal, width, height, strip_rows,
                    strip_count, root=None, root_strips=1, stream=None):
        """Gathered wire buffers -> full rgba surfaces in image order (alpha restored to 1.0).  root = (d_color,
        d_pos, d_normal) of rank 0's own local surfaces: its rows are copied from there instead of wire slot 0."""
        self._call("rt_wire_unpack", _dev_ptr(d_wire), rank_stride_bytes, rank_pixels, *[_dev_ptr(x) for x in root or (None,) * 3],
                   root_strips, _dev_ptr(d_color), _dev_ptr(d_pos), _dev_ptr(d_normal), width, height, strip_rows, strip_count,
                   _dev_ptr(stream))


class _BorrowedRayTracer(RayTracer):
    """A RayTracer view of a context somebody else owns (MultiGpuRayTracer.context): every method works on it, close() and the
    garbage collector only let go of it -- rt_destroy is the owner's.  It is valid as long as its owner is open."""

    def __init__(self, lib, ctx):
        self.lib, self.ctx = lib, ctx
        self._size = None
        self._present_tickets = {}

    def close(self):
        self.ctx = None


class MultiGpuRayTracer(_Handle):
    """rt_mgpu_*: one frame on N devices from one process; the devices' kernels store their strips straight into device 0's frame
    (include/rt_mi355.h).  `devices` may repeat an id (the N-way plan on one GPU)."""
    _PREFIX = "rt_mgpu_"
    m = property(lambda self: self.ctx, doc="the rt_mgpu handle")

    def __init__(self, devices, strip_rows=8):
        self._create("rt_mgpu_create (peer access between the devices?)", (ctypes.c_int * len(devices))(*devices), len(devices))
        self.n = len(devices)
        self._call("rt_mgpu_set_strip_rows", strip_rows)

    def set_scene(self, objects, lights):
        """rt_mgpu_set_scene alone: the per-frame upload, asynchronous on every context's stream (load() also sets the
        textures, which waits for every frame in flight)."""
        objects, lights = np.ascontiguousarray(objects), np.ascontiguousarray(lights)
        self._call("rt_mgpu_set_scene", _ptr(objects) if len(objects) else None, len(objects),
                   _ptr(lights) if len(lights) else None, len(lights))

    def load(self, scene):
        self.set_scene(scene.objects, scene.lights)
        if scene.noise is None:
            self._call("rt_mgpu_set_noise", None, 0, 0)
        else:
            r8 = np.ascontiguousarray(scene.noise, dtype=np.uint8)
            self._call("rt_mgpu_set_noise", _ptr(r8), r8.shape[1], r8.shape[0])
        faces = np.ascontiguousarray(scene.skybox, dtype=np.float16) if scene.use_skybox else None
        self._call("rt_mgpu_set_skybox", _ptr(faces), faces.shape[1] if faces is not None else 0)

    def render(self, params):
        self._call("rt_mgpu_render", ctypes.byref(params))
        self._size = (params.width, params.height)

    def readback(self):
        if self._size is None:             # no frame of this handle's yet: the library says so (RT_ERR_NO_SURFACES)
            self._call("rt_mgpu_readback", None, None, None)
        return super().readback()

    def last_ms(self):
        out = (ctypes.c_float * self.n)()
        self._call("rt_mgpu_last_ms", out, self.n)
        return list(out)

    def set_strip_rows(self, n):
        """Rows per strip of the frames from now on (rt_mgpu_set_strip_rows)."""
        self._call("rt_mgpu_set_strip_rows", int(n))

    def get_surfaces(self):
        """Device pointers (ints) of the root's full-frame gColor, gPosition, gNormal, and the root stream (a hipStream_t as an
        int): work enqueued on it sees the whole last frame, and the next frame overwrites the surfaces only behind that work."""
        dc, dp, dn, s = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._call("rt_mgpu_get_surfaces", ctypes.byref(dc), ctypes.byref(dp), ctypes.byref(dn), ctypes.byref(s))
        return dc.value, dp.value, dn.value, s.value

    def context(self, slot):
        """Device slot `slot`'s context as a RayTracer that does not own it (rt_mgpu_context): for the debug_* read-outs of one
        device's share.  Valid while this handle is open; closing the view destroys nothing."""
        c = ctypes.c_void_p()
        self._call("rt_mgpu_context", int(slot), ctypes.byref(c))
        return _BorrowedRayTracer(self.lib, c)
