"""Byte layouts of the reference's SSBO records and uniform block.

These mirror, field for field, the host structs the reference uploads with
``glBufferData`` and the std430 view its shader has of them:

* ``Object``  176 B  -- /root/reference/src/Object.h:13-21, shader/raytracingCs.glsl:34-42
* ``Material`` 80 B  -- /root/reference/src/Material.h:11-23 (embedded at byte 64)
* ``AABB``     32 B  -- /root/reference/src/Object.h:8-11   (embedded at byte 144)
* ``Light``    96 B  -- /root/reference/src/Light.h:7-20, shader/raytracingCs.glsl:44-58

Offsets are SURVEY.md Appendix B (host ``offsetof`` == llvmpipe GL_OFFSET).  The C
side (include/rt_mi355.h) ``static_assert``s the same numbers.
"""
import ctypes

import numpy as np

OBJECT_STRIDE = 176
LIGHT_STRIDE = 96

# ObjectType  (/root/reference/src/Object.h:6)
SPHERE, PLANE = 0, 1
# LightType   (/root/reference/src/Light.h:5)
POINT, DIRECTIONAL, AREA = 0, 1, 2
# shadowType  (/root/reference/src/Light.h:16)
SHADOW_NONE, SHADOW_PCF, SHADOW_PCSS = 0, 1, 2
# MaterialType (/root/reference/src/Material.h:5-9) -- never read by the shader
MATERIAL_METALLIC, MATERIAL_DIELECTRIC, MATERIAL_PLASTIC = 0, 1, 2

OBJECT_DTYPE = np.dtype(
    {
        "names": [
            "type", "position", "radius", "normal", "size",
            "mat_type", "albedo", "metallic", "roughness", "diffuseStrength", "ior",
            "transparency", "specular", "subsurfaceScatter", "subsurfaceColor",
            "scatterDistance", "bounds_min", "bounds_max",
        ],
        "formats": [
            "<i4", ("<f4", 3), "<f4", ("<f4", 3), ("<f4", 2),
            "<i4", ("<f4", 3), "<f4", "<f4", "<f4", "<f4",
            "<f4", "<f4", "<f4", ("<f4", 3),
            "<f4", ("<f4", 3), ("<f4", 3),
        ],
        "offsets": [0, 16, 28, 32, 48, 64, 80, 92, 96, 100, 104, 108, 112, 116, 128, 140, 144, 160],
        "itemsize": OBJECT_STRIDE,
    }
)

LIGHT_DTYPE = np.dtype(
    {
        "names": [
            "type", "position", "direction", "color", "intensity", "radius", "samples",
            "shadowSoftness", "shadowType", "pcfSamples", "lightSize", "angularRadius",
        ],
        "formats": [
            "<i4", ("<f4", 3), ("<f4", 3), ("<f4", 3), "<f4", "<f4", "<i4",
            "<f4", "<i4", "<i4", "<f4", "<f4",
        ],
        "offsets": [0, 16, 32, 48, 60, 64, 68, 72, 76, 80, 84, 88],
        "itemsize": LIGHT_STRIDE,
    }
)

assert OBJECT_DTYPE.itemsize == 176 and LIGHT_DTYPE.itemsize == 96


def default_objects(n):
    """n Objects carrying the reference's member initialisers
    (/root/reference/src/Object.h:16-18, Material.h:12-22); diffuseStrength, which
    the reference leaves uninitialised, is set to the UI's value-initialised 0."""
    o = np.zeros(n, dtype=OBJECT_DTYPE)
    o["radius"] = 1.0
    o["normal"] = (0.0, 1.0, 0.0)
    o["size"] = (1.0, 1.0)
    o["mat_type"] = MATERIAL_PLASTIC
    o["albedo"] = 1.0
    o["roughness"] = 0.5
    o["ior"] = 1.0
    o["specular"] = 0.5
    o["subsurfaceColor"] = 1.0
    o["scatterDistance"] = 0.1
    return o


def default_lights(n):
    """n Lights carrying /root/reference/src/Light.h:8-19's initialisers."""
    l = np.zeros(n, dtype=LIGHT_DTYPE)
    l["direction"] = (0.0, -1.0, 0.0)
    l["color"] = 1.0
    l["intensity"] = 1.0
    l["radius"] = 0.5
    l["samples"] = 4
    l["shadowSoftness"] = 1.0
    l["shadowType"] = SHADOW_PCF
    l["pcfSamples"] = 4
    l["lightSize"] = 1.0
    return l


class RtParams(ctypes.Structure):
    """``rt_params`` of include/rt_mi355.h (identical to ``orc_params`` of
    oracle/rt_oracle.h): the shader's uniforms (raytracingCs.glsl:72-89, uploaded at
    /root/reference/src/ForwardShadingPipeline.cpp:155-166) + image size + window."""

    _fields_ = [
        ("camPos", ctypes.c_float * 3),
        ("camDir", ctypes.c_float * 3),
        ("camUp", ctypes.c_float * 3),
        ("camRight", ctypes.c_float * 3),
        ("fovDeg", ctypes.c_float),
        ("focalLength", ctypes.c_float),
        ("maxRayDistance", ctypes.c_float),
        ("noiseScale", ctypes.c_float * 2),
        ("frameCount", ctypes.c_int32),
        ("useSkybox", ctypes.c_int32),
        ("maxRayDepth", ctypes.c_int32),
        ("width", ctypes.c_int32),
        ("height", ctypes.c_int32),
        ("x0", ctypes.c_int32),
        ("y0", ctypes.c_int32),
        ("regionW", ctypes.c_int32),
        ("regionH", ctypes.c_int32),
        ("stripRows", ctypes.c_int32),
        ("stripCount", ctypes.c_int32),
        ("stripIndex", ctypes.c_int32),
        ("reserved0", ctypes.c_int32),
        ("stripCycleRows", ctypes.c_int32),
        ("stripOffsetRows", ctypes.c_int32),
    ]


assert ctypes.sizeof(RtParams) == 128


def make_params(width, height, max_ray_depth, cam_pos=(0.0, 0.0, 0.0), cam_dir=(0.0, 0.0, -1.0),
                cam_up=(0.0, 1.0, 0.0), cam_right=(1.0, 0.0, 0.0), fov_deg=45.0, focal_length=1.0,
                max_ray_distance=114514.0, noise_scale=(1.0 / 1024.0, 1.0 / 1024.0), frame_count=0,
                use_skybox=0, window=None, strips=None):
    """Uniform defaults follow the reference: camera /root/reference/src/Camera.h:9-20,
    focalLength/maxRayDistance raytracingCs.glsl:80,85, noiseScale
    ForwardShadingPipeline.cpp:164.  ``window`` = (x0, y0, w, h) in local-row space,
    ``strips`` = (stripRows, stripCount, stripIndex)."""
    p = RtParams()
    p.camPos[:] = cam_pos
    p.camDir[:] = cam_dir
    p.camUp[:] = cam_up
    p.camRight[:] = cam_right
    p.fovDeg = fov_deg
    p.focalLength = focal_length
    p.maxRayDistance = max_ray_distance
    p.noiseScale[:] = noise_scale
    p.frameCount = frame_count
    p.useSkybox = int(use_skybox)
    p.maxRayDepth = max_ray_depth
    p.width, p.height = width, height
    if window is None:
        window = (0, 0, width, height)
    p.x0, p.y0, p.regionW, p.regionH = window
    if strips is None:
        strips = (1, 1, 0)
    p.stripRows, p.stripCount, p.stripIndex = strips
    return p


def copy_params(p, **updates):
    q = RtParams.from_buffer_copy(bytes(p))
    for k, v in updates.items():
        if isinstance(v, (tuple, list)):
            getattr(q, k)[:] = v
        else:
            setattr(q, k, v)
    return q


# ---- ray queries (rt_trace_rays / rt_camera_rays / rt_pick, include/rt_mi355.h) ---------------
QUERY_CLOSEST, QUERY_ANY = 0, 1

RAY_DTYPE = np.dtype({"names": ["origin", "tMax", "direction", "reserved"],
                      "formats": [("<f4", 3), "<f4", ("<f4", 3), "<i4"],
                      "offsets": [0, 12, 16, 28], "itemsize": 32})
HIT_DTYPE = np.dtype({"names": ["position", "t", "normal", "object"],
                      "formats": [("<f4", 3), "<f4", ("<f4", 3), "<i4"],
                      "offsets": [0, 12, 16, 28], "itemsize": 32})


class RtRay(ctypes.Structure):
    """``rt_ray``: the ray origin + direction * t, 0 < t < tMax."""
    _fields_ = [("origin", ctypes.c_float * 3), ("tMax", ctypes.c_float), ("direction", ctypes.c_float * 3),
                ("reserved", ctypes.c_int32)]


class RtHit(ctypes.Structure):
    """``rt_hit``: closest hit (object -1 = miss, then t = tMax and position / normal 0)."""
    _fields_ = [("position", ctypes.c_float * 3), ("t", ctypes.c_float), ("normal", ctypes.c_float * 3),
                ("object", ctypes.c_int32)]


assert ctypes.sizeof(RtRay) == RAY_DTYPE.itemsize == 32 and ctypes.sizeof(RtHit) == HIT_DTYPE.itemsize == 32


# ---- the hierarchy behind the queries (rt_set_accel / rt_accel_info / rt_accel_build_host, include/rt_mi355.h) ----------------
ACCEL_AUTO, ACCEL_LANE, ACCEL_WAVE = 0, 1, 2
ACCEL_TRAVERSALS = {"auto": ACCEL_AUTO, "lane": ACCEL_LANE, "wave": ACCEL_WAVE}
ACCEL_INNER = 0xFFFFFFFF       # rt_accel_node.leaf of an inner node; else first << 4 | count into order[]

ACCEL_NODE_DTYPE = np.dtype({"names": ["lo", "skip", "hi", "leaf"], "formats": [("<f4", 3), "<u4", ("<f4", 3), "<u4"],
                             "offsets": [0, 12, 16, 28], "itemsize": 32})


class RtAccelDesc(ctypes.Structure):
    """``rt_accel_desc``: zero = the default of every field."""
    _fields_ = [("enable", ctypes.c_int32), ("leafSize", ctypes.c_int32), ("traversal", ctypes.c_int32), ("minObjects", ctypes.c_int32),
                ("largeFraction", ctypes.c_float), ("reserved", ctypes.c_int32 * 3)]


class RtAccelReport(ctypes.Structure):
    """``rt_accel_report``: what rt_accel_info and rt_accel_build_host answer."""
    _fields_ = [("built", ctypes.c_int32), ("nodes", ctypes.c_int32), ("leaves", ctypes.c_int32), ("depth", ctypes.c_int32),
                ("loose", ctypes.c_int32), ("reserved0", ctypes.c_int32), ("bytes", ctypes.c_uint64), ("buildMs", ctypes.c_double),
                ("builds", ctypes.c_uint64), ("launchesAccel", ctypes.c_uint64 * 2), ("launchesBrute", ctypes.c_uint64),
                ("reserved", ctypes.c_uint64 * 3)]


assert ctypes.sizeof(RtAccelDesc) == 32 and ctypes.sizeof(RtAccelReport) == 96 and ACCEL_NODE_DTYPE.itemsize == 32


def make_accel_desc(enable=True, leaf_size=0, traversal="auto", min_objects=0, large_fraction=0.0):
    """An rt_accel_desc; 0 keeps a field's default (leaf 4, minObjects 1024, largeFraction 0.5).  traversal: "auto", "lane", "wave" or a number."""
    d = RtAccelDesc()
    d.enable, d.leafSize, d.minObjects, d.largeFraction = int(bool(enable)), int(leaf_size), int(min_objects), float(large_fraction)
    d.traversal = int(ACCEL_TRAVERSALS.get(traversal, traversal))
    return d


# ---- who builds it (rt_set_accel_builder / rt_accel_build_info) ----
ACCEL_BUILD_HOST, ACCEL_BUILD_DEVICE = 0, 1
ACCEL_BUILDERS = {"host": ACCEL_BUILD_HOST, "device": ACCEL_BUILD_DEVICE}


class RtAccelBuildReport(ctypes.Structure):
    """``rt_accel_build_report``: what rt_accel_build_info answers."""
    _fields_ = [("builder", ctypes.c_int32), ("reserved0", ctypes.c_int32), ("buildsHost", ctypes.c_uint64), ("buildsDevice", ctypes.c_uint64),
                ("hostMs", ctypes.c_double), ("deviceMs", ctypes.c_double), ("reserved", ctypes.c_uint64 * 3)]


assert ctypes.sizeof(RtAccelBuildReport) == 64


class RtAccelShadeDesc(ctypes.Structure):
    """``rt_accel_shade_desc``: zero = the default of every field."""
    _fields_ = [("enable", ctypes.c_int32), ("traversal", ctypes.c_int32), ("minObjects", ctypes.c_int32), ("reserved", ctypes.c_int32 * 5)]


class RtAccelShadeReport(ctypes.Structure):
    """``rt_accel_shade_report``: what rt_accel_shading_info answers."""
    _fields_ = [("active", ctypes.c_int32), ("traversal", ctypes.c_int32), ("launchesAccel", ctypes.c_uint64 * 2),
                ("launchesBrute", ctypes.c_uint64), ("reserved", ctypes.c_uint64 * 2)]


assert ctypes.sizeof(RtAccelShadeDesc) == 32 and ctypes.sizeof(RtAccelShadeReport) == 48


def make_accel_shade_desc(enable=True, traversal="auto", min_objects=0):
    """An rt_accel_shade_desc; min_objects 0 keeps the default.  traversal: "auto", "lane", "wave" or a number."""
    d = RtAccelShadeDesc()
    d.enable, d.minObjects = int(bool(enable)), int(min_objects)
    d.traversal = int(ACCEL_TRAVERSALS.get(traversal, traversal))
    return d


# ---- the frames through the hierarchy (rt_set_accel_render / rt_accel_render_info) ----
ACCEL_RENDER_AUTO, ACCEL_RENDER_LANE, ACCEL_RENDER_WAVE, ACCEL_RENDER_SPLIT = 0, 1, 2, 3
ACCEL_RENDER_TRAVERSALS = {"auto": ACCEL_RENDER_AUTO, "lane": ACCEL_RENDER_LANE, "wave": ACCEL_RENDER_WAVE, "split": ACCEL_RENDER_SPLIT}
ACCEL_RENDER_DEFAULT_MIN_OBJECTS = 4098


class RtAccelRenderDesc(ctypes.Structure):
    """``rt_accel_render_desc``: zero = the default of every field."""
    _fields_ = [("enable", ctypes.c_int32), ("traversal", ctypes.c_int32), ("minObjects", ctypes.c_int32), ("reserved", ctypes.c_int32 * 5)]


class RtAccelRenderReport(ctypes.Structure):
    """``rt_accel_render_report``: what rt_accel_render_info answers."""
    _fields_ = [("active", ctypes.c_int32), ("traversal", ctypes.c_int32), ("minObjects", ctypes.c_int32), ("reserved0", ctypes.c_int32),
                ("launchesAccel", ctypes.c_uint64 * 3), ("launchesPacket", ctypes.c_uint64), ("reserved", ctypes.c_uint64 * 2)]


assert ctypes.sizeof(RtAccelRenderDesc) == 32 and ctypes.sizeof(RtAccelRenderReport) == 64


def make_accel_render_desc(enable=True, traversal="auto", min_objects=0):
    """An rt_accel_render_desc; min_objects 0 keeps the default.  traversal: "auto", "lane", "wave", "split" or a number."""
    d = RtAccelRenderDesc()
    d.enable, d.minObjects = int(bool(enable)), int(min_objects)
    d.traversal = int(ACCEL_RENDER_TRAVERSALS.get(traversal, traversal))
    return d


# ---- ray shading (rt_shade_rays, include/rt_mi355.h) ------------------------------------------
PIXEL_DTYPE = np.dtype({"names": ["x", "y"], "formats": ["<u4", "<u4"], "offsets": [0, 4], "itemsize": 8})


class RtPixel(ctypes.Structure):
    """``rt_pixel``: the gl_GlobalInvocationID.xy a shaded ray stands for."""
    _fields_ = [("x", ctypes.c_uint32), ("y", ctypes.c_uint32)]


assert ctypes.sizeof(RtPixel) == PIXEL_DTYPE.itemsize == 8


# ---- display packing and delivery (rt_display_pack / rt_present_*, include/rt_mi355.h) --------
DISPLAY_RGBA8_LINEAR, DISPLAY_RGBA8_SRGB = 0, 1
DISPLAY_FLIP_ROWS = 1


class RtDisplayDesc(ctypes.Structure):
    """``rt_display_desc``: size of the rgba32f surface, output format, flags, exposure."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("format", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("exposure", ctypes.c_float), ("reserved", ctypes.c_int32 * 3)]


assert ctypes.sizeof(RtDisplayDesc) == 32


def make_display_desc(width, height, format="linear", flip=False, exposure=1.0):
    f = {"linear": DISPLAY_RGBA8_LINEAR, "srgb": DISPLAY_RGBA8_SRGB}.get(format, format)
    d = RtDisplayDesc()
    d.width, d.height, d.format, d.flags, d.exposure = int(width), int(height), int(f), DISPLAY_FLIP_ROWS if flip else 0, float(exposure)
    return d


# ---- exposure metering and tone curves (rt_meter / rt_display_pack_toned, include/rt_mi355.h) --
TONE_NONE, TONE_REINHARD, TONE_ACES = 0, 1, 2
METER_EXPOSURE_OFFSET = 1060


class RtMeterDesc(ctypes.Structure):
    """``rt_meter_desc``: surface size, key, exposure limits, adaptation rate, trimmed shares."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("key", ctypes.c_float), ("minExposure", ctypes.c_float),
                ("maxExposure", ctypes.c_float), ("adapt", ctypes.c_float), ("lowPermille", ctypes.c_int32),
                ("highPermille", ctypes.c_int32), ("reserved", ctypes.c_int32 * 4)]


class RtToneDesc(ctypes.Structure):
    """``rt_tone_desc``: tone operator, Reinhard's white, the device float the exposure is multiplied by (or NULL)."""
    _fields_ = [("op", ctypes.c_int32), ("white", ctypes.c_float), ("dExposure", ctypes.c_void_p), ("reserved", ctypes.c_int32 * 4)]


# ``rt_meter_state``: what rt_meter leaves in device memory (a zeroed one starts a sequence)
METER_STATE_DTYPE = np.dtype({
    "names": ["hist", "nPixels", "nNonPositive", "nNaN", "nInf", "minLum", "maxLum", "nMetered", "meanLog2Q16", "target", "exposure",
              "frames", "reserved"],
    "formats": [("<u4", (256,)), "<u4", "<u4", "<u4", "<u4", "<f4", "<f4", "<u4", "<u4", "<f4", "<f4", "<u4", ("<u4", (5,))],
    "offsets": [0, 1024, 1028, 1032, 1036, 1040, 1044, 1048, 1052, 1056, 1060, 1064, 1068], "itemsize": 1088})

assert ctypes.sizeof(RtMeterDesc) == 48 and ctypes.sizeof(RtToneDesc) == 32 and METER_STATE_DTYPE.itemsize == 1088
assert METER_STATE_DTYPE.fields["exposure"][1] == METER_EXPOSURE_OFFSET


def make_meter_desc(width, height, key=0.18, min_exposure=2.0 ** -10, max_exposure=2.0 ** 10, adapt=1.0, low_permille=0, high_permille=0):
    d = RtMeterDesc()
    d.width, d.height, d.key, d.minExposure, d.maxExposure = int(width), int(height), float(key), float(min_exposure), float(max_exposure)
    d.adapt, d.lowPermille, d.highPermille = float(adapt), int(low_permille), int(high_permille)
    return d


def make_tone_desc(tone="none", white=1.0, d_exposure=None):
    """d_exposure: a device address (int) or None."""
    t = RtToneDesc()
    t.op = int({"none": TONE_NONE, "reinhard": TONE_REINHARD, "aces": TONE_ACES}.get(tone, tone))
    t.white = float(white)
    t.dExposure = d_exposure or None
    return t


# ---- YUV 4:2:0 video output (rt_display_pack_yuv / rt_present_submit_yuv, include/rt_mi355.h) --
YUV_NV12, YUV_I420 = 0, 1
YUV_BT709, YUV_BT601 = 0, 1
YUV_LIMITED, YUV_FULL = 0, 1


class RtYuvDesc(ctypes.Structure):
    """``rt_yuv_desc``: size of the rgba32f surface, plane format, matrix, range, transfer of the R'G'B' codes, flags, exposure."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("format", ctypes.c_int32), ("matrix", ctypes.c_int32),
                ("range", ctypes.c_int32), ("transfer", ctypes.c_int32), ("flags", ctypes.c_uint32), ("exposure", ctypes.c_float),
                ("reserved", ctypes.c_int32 * 4)]


assert ctypes.sizeof(RtYuvDesc) == 48


def make_yuv_desc(width, height, format="nv12", matrix="bt709", range="limited", transfer="srgb", flip=False, exposure=1.0):
    d = RtYuvDesc()
    d.width, d.height = int(width), int(height)
    d.format = int({"nv12": YUV_NV12, "i420": YUV_I420}.get(format, format))
    d.matrix = int({"bt709": YUV_BT709, "bt601": YUV_BT601}.get(matrix, matrix))
    d.range = int({"limited": YUV_LIMITED, "full": YUV_FULL}.get(range, range))
    d.transfer = int({"linear": DISPLAY_RGBA8_LINEAR, "srgb": DISPLAY_RGBA8_SRGB}.get(transfer, transfer))
    d.flags, d.exposure = DISPLAY_FLIP_ROWS if flip else 0, float(exposure)
    return d


# ---- baseline JPEG output (rt_jpeg_encode / rt_display_pack_jpeg / rt_present_submit_jpeg, include/rt_mi355.h) --
JPEG_HEADER_BYTES = 629
JPEG_STATE_BYTES = 64
JPEG_DEFAULT_INTERVAL = 8


class RtJpegDesc(ctypes.Structure):
    """``rt_jpeg_desc``: size of the frame, quality 1..100, MCUs per restart segment."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("quality", ctypes.c_int32), ("restartInterval", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 4)]


assert ctypes.sizeof(RtJpegDesc) == 32

# ``rt_jpeg_state``: what an encode leaves on the device, sixteen uint32
JPEG_STATE_DTYPE = np.dtype([("bytes", "<u4"), ("needed", "<u4"), ("overflow", "<u4"), ("nSegments", "<u4"), ("nMcu", "<u4"),
                             ("headerBytes", "<u4"), ("stuffedBytes", "<u4"), ("reserved", "<u4", (9,))])
assert JPEG_STATE_DTYPE.itemsize == JPEG_STATE_BYTES


def make_jpeg_desc(width, height, quality=90, restart_interval=None):
    """restart_interval None: JPEG_DEFAULT_INTERVAL MCUs -- segments are what the entropy coder runs in parallel, one wave each, and
    eight MCUs keep a 1080p frame at a thousand waves for 2 bytes of marker, three predictors and a padded byte per segment."""
    d = RtJpegDesc()
    d.width, d.height, d.quality = int(width), int(height), int(quality)
    d.restartInterval = int(restart_interval) if restart_interval is not None else JPEG_DEFAULT_INTERVAL
    return d


# ---- resampling in front of the display path (rt_display_resample / rt_resample_taps, include/rt_mi355.h) --
RESAMPLE_AREA, RESAMPLE_TRIANGLE, RESAMPLE_LANCZOS3 = 0, 1, 2
RESAMPLE_MAX_TAPS = 64
RESAMPLE_FILTERS = {"area": RESAMPLE_AREA, "triangle": RESAMPLE_TRIANGLE, "lanczos3": RESAMPLE_LANCZOS3}


class RtResampleDesc(ctypes.Structure):
    """``rt_resample_desc``: source and destination sizes of the rgba32f surfaces, filter, flags (zero)."""
    _fields_ = [("srcWidth", ctypes.c_int32), ("srcHeight", ctypes.c_int32), ("dstWidth", ctypes.c_int32), ("dstHeight", ctypes.c_int32),
                ("filter", ctypes.c_int32), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_int32 * 2)]


assert ctypes.sizeof(RtResampleDesc) == 32


def make_resample_desc(src_w, src_h, dst_w, dst_h, filter="lanczos3"):
    d = RtResampleDesc()
    d.srcWidth, d.srcHeight, d.dstWidth, d.dstHeight = int(src_w), int(src_h), int(dst_w), int(dst_h)
    d.filter = int(RESAMPLE_FILTERS.get(filter, filter))
    return d


# ---- progressive accumulation (rt_accum_*, include/rt_mi355.h) ---------------------------------------------
ACCUM_VIEW_RELERR, ACCUM_VIEW_COUNT, ACCUM_VIEW_CONVERGED = 0, 1, 2
ACCUM_VIEWS = {"relerr": ACCUM_VIEW_RELERR, "count": ACCUM_VIEW_COUNT, "converged": ACCUM_VIEW_CONVERGED}
ACCUM_BINS = 128
ACCUM_STATE_BYTES = 1024


class RtAccumDesc(ctypes.Structure):
    """``rt_accum_desc``: surface size, target relative error, luminance floor, least sample count, share of converged pixels."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("relError", ctypes.c_float), ("lumFloor", ctypes.c_float),
                ("minSamples", ctypes.c_int32), ("donePermille", ctypes.c_int32), ("reserved", ctypes.c_int32 * 4)]


class RtAccumState(ctypes.Structure):
    """``rt_accum_state``: the 1 KiB convergence report rt_accum_add leaves on the device."""
    _fields_ = [("hist", ctypes.c_uint32 * 128), ("nPixels", ctypes.c_uint32), ("nUnsampled", ctypes.c_uint32),
                ("nConverged", ctypes.c_uint32), ("nRejected", ctypes.c_uint32), ("minCount", ctypes.c_uint32),
                ("maxCount", ctypes.c_uint32), ("maxR2Bits", ctypes.c_uint32), ("medianBin", ctypes.c_uint32),
                ("p95Bin", ctypes.c_uint32), ("done", ctypes.c_uint32), ("frames", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 117)]


# the same record as a numpy dtype (what a read-back of the state is viewed as)
ACCUM_STATE_DTYPE = np.dtype({
    "names": ["hist", "nPixels", "nUnsampled", "nConverged", "nRejected", "minCount", "maxCount", "maxR2Bits", "medianBin", "p95Bin",
              "done", "frames", "reserved"],
    "formats": [("<u4", (128,))] + ["<u4"] * 11 + [("<u4", (117,))],
    "offsets": [0] + [512 + 4 * k for k in range(12)], "itemsize": 1024})
ACCUM_DONE_OFFSET = 548        # offsetof(rt_accum_state, done): the 4 bytes a frame loop reads every k frames

assert ctypes.sizeof(RtAccumDesc) == 40 and ctypes.sizeof(RtAccumState) == ACCUM_STATE_BYTES == ACCUM_STATE_DTYPE.itemsize
assert ACCUM_STATE_DTYPE.fields["done"][1] == ACCUM_DONE_OFFSET == RtAccumState.done.offset


def make_accum_desc(width, height, rel_error=0.02, lum_floor=2.0 ** -10, min_samples=16, done_permille=950):
    d = RtAccumDesc()
    d.width, d.height, d.relError, d.lumFloor = int(width), int(height), float(rel_error), float(lum_floor)
    d.minSamples, d.donePermille = int(min_samples), int(done_permille)
    return d


# ---- adaptive sampling (rt_accum_select / rt_camera_rays_at / rt_accum_add_at, include/rt_mi355.h) ----------------------------
SELECT_STATE_BYTES = 64
SELECT_TILE = 8                # the list's order: tiles of 8 x 8 pixels in raster order, raster order inside a tile
SELECT_MAX_SAMPLES = 1 << 24   # the largest budget cap


class RtSelectState(ctypes.Structure):
    """``rt_select_state``: the 64 bytes rt_accum_select leaves on the device."""
    _fields_ = [("nPixels", ctypes.c_uint32), ("nSelected", ctypes.c_uint32), ("nListed", ctypes.c_uint32), ("capacity", ctypes.c_uint32),
                ("overflow", ctypes.c_uint32), ("nCapped", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 10)]


# the same record as a numpy dtype (what a read-back of the select state is viewed as)
SELECT_STATE_DTYPE = np.dtype({
    "names": ["nPixels", "nSelected", "nListed", "capacity", "overflow", "nCapped", "reserved"],
    "formats": ["<u4"] * 6 + [("<u4", (10,))], "offsets": [4 * k for k in range(7)], "itemsize": 64})
SELECT_NSELECTED_OFFSET = 4    # offsetof(rt_select_state, nSelected): 8 bytes from here are nSelected and nListed, the loop's read

assert ctypes.sizeof(RtSelectState) == SELECT_STATE_BYTES == SELECT_STATE_DTYPE.itemsize
assert all(SELECT_STATE_DTYPE.fields[k][1] == getattr(RtSelectState, k).offset for k in SELECT_STATE_DTYPE.names)
assert RtSelectState.nSelected.offset == SELECT_NSELECTED_OFFSET and RtSelectState.nListed.offset == 8


# ---- first-hit-guided upsampling (rt_upsample / rt_image_put_at, include/rt_mi355.h) ---------------------------------------------
UPSAMPLE_DEFAULTS = dict(normal_log2_power=5, min_weight=0.25)


class RtUpsampleDesc(ctypes.Structure):
    """``rt_upsample_desc``: the output's size, the low-resolution size, the normal weight's power, the least 2 x 2 weight of an
    interpolated pixel."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("lowWidth", ctypes.c_int32), ("lowHeight", ctypes.c_int32),
                ("normalLog2Power", ctypes.c_int32), ("minWeight", ctypes.c_float), ("reserved", ctypes.c_int32 * 10)]


assert ctypes.sizeof(RtUpsampleDesc) == 64 and RtUpsampleDesc.minWeight.offset == 20 and RtUpsampleDesc.reserved.offset == 24


def make_upsample_desc(width, height, low_width, low_height, normal_log2_power=5, min_weight=0.25):
    d = RtUpsampleDesc()
    d.width, d.height, d.lowWidth, d.lowHeight = int(width), int(height), int(low_width), int(low_height)
    d.normalLog2Power, d.minWeight = int(normal_log2_power), float(min_weight)
    return d


# ---- denoising (rt_denoise_guide / rt_denoise, include/rt_mi355.h) ---------------------------------------------
# one pixel of the guide plane: the upper half of an rt_hit, the normal normalised
DENOISE_GUIDE_DTYPE = np.dtype({"names": ["n", "object"], "formats": [("<f4", 3), "<i4"], "offsets": [0, 12], "itemsize": 16})
DENOISE_DEFAULTS = dict(iterations=4, normal_log2_power=5, sigma_lum=4.0, lum_eps=2.0 ** -10, min_count=4)


class RtDenoiseDesc(ctypes.Structure):
    """``rt_denoise_desc``: surface size, a-trous iterations, the normal weight's power, the luminance weight's scale, the sample count
    below which the variance is estimated spatially."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("iterations", ctypes.c_int32), ("normalLog2Power", ctypes.c_int32),
                ("sigmaLum", ctypes.c_float), ("lumEps", ctypes.c_float), ("minCount", ctypes.c_int32), ("reserved", ctypes.c_int32 * 5)]


assert ctypes.sizeof(RtDenoiseDesc) == 48 and RtDenoiseDesc.sigmaLum.offset == 16 and RtDenoiseDesc.reserved.offset == 28
assert DENOISE_GUIDE_DTYPE.itemsize == 16 and DENOISE_GUIDE_DTYPE.fields["object"][1] == HIT_DTYPE.fields["object"][1] - 16


def make_denoise_desc(width, height, iterations=4, normal_log2_power=5, sigma_lum=4.0, lum_eps=2.0 ** -10, min_count=4):
    d = RtDenoiseDesc()
    d.width, d.height, d.iterations, d.normalLog2Power = int(width), int(height), int(iterations), int(normal_log2_power)
    d.sigmaLum, d.lumEps, d.minCount = float(sigma_lum), float(lum_eps), int(min_count)
    return d


# ---- reprojection (rt_accum_reproject, include/rt_mi355.h) ---------------------------------------------
REPROJECT_DEFAULTS = dict(normal_cos_min=0.9, plane_tol=0.01, max_history=32)
REPROJECT_REPORT_BYTES = 64


class RtReprojectDesc(ctypes.Structure):
    """``rt_reproject_desc``: surface size, the previous and the current view, the two tap tests' thresholds, the history cap."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("prev", RtParams), ("cur", RtParams),
                ("normalCosMin", ctypes.c_float), ("planeTol", ctypes.c_float), ("maxHistory", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 3)]


class RtReprojectReport(ctypes.Structure):
    """``rt_reproject_report``: the 64 bytes rt_accum_reproject leaves on the device."""
    _fields_ = [("nPixels", ctypes.c_uint32), ("nReused", ctypes.c_uint32), ("nRejected", ctypes.c_uint32),
                ("nOffscreen", ctypes.c_uint32), ("nMiss", ctypes.c_uint32), ("minCount", ctypes.c_uint32),
                ("maxCount", ctypes.c_uint32), ("reserved0", ctypes.c_uint32), ("sumCount", ctypes.c_uint64),
                ("reserved", ctypes.c_uint32 * 6)]


# the same record as a numpy dtype (what a read-back of the report is viewed as)
REPROJECT_REPORT_DTYPE = np.dtype({
    "names": ["nPixels", "nReused", "nRejected", "nOffscreen", "nMiss", "minCount", "maxCount", "reserved0", "sumCount", "reserved"],
    "formats": ["<u4"] * 8 + ["<u8", ("<u4", (6,))],
    "offsets": [4 * k for k in range(8)] + [32, 40], "itemsize": 64})

assert ctypes.sizeof(RtReprojectDesc) == 288 and RtReprojectDesc.cur.offset == 136 and RtReprojectDesc.normalCosMin.offset == 264
assert RtReprojectDesc.reserved.offset == 276
assert ctypes.sizeof(RtReprojectReport) == REPROJECT_REPORT_BYTES == REPROJECT_REPORT_DTYPE.itemsize
assert all(REPROJECT_REPORT_DTYPE.fields[k][1] == getattr(RtReprojectReport, k).offset for k in REPROJECT_REPORT_DTYPE.names)


def make_reproject_desc(prev, cur, normal_cos_min=0.9, plane_tol=0.01, max_history=32):
    """prev, cur: the RtParams of the two views; the surface size is the current view's."""
    d = RtReprojectDesc()
    d.width, d.height = int(cur.width), int(cur.height)
    d.prev, d.cur = prev, cur
    d.normalCosMin, d.planeTol, d.maxHistory = float(normal_cos_min), float(plane_tol), int(max_history)
    return d
