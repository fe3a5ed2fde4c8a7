#!/usr/bin/env python3
"""Generate the committed golden fixtures by running the REFERENCE's own shader
(/root/reference/shader/raytracingCs.glsl, read at run time, never copied) unmodified on
Mesa llvmpipe through oracle/_ref/gl_harness.

Runs only in the build container (needs /root/reference and Mesa's swrast_dri.so); the GPU box
and the CPU test-suite consume the .npz files this writes.  Usage:

    python tests/golden/make_golden.py [--only c1,c2,...] [--skip-fullres]

Per config the fixture holds
  * the inputs as bytes (objects, lights, params, noise/skybox flags) -- so a test never depends
    on the scene generator staying bit-stable,
  * `lowres_*`: a complete low-resolution frame of the config's scene (all three surfaces),
  * `win_*`: eight 32x32 windows cut from the FULL-resolution frame of the config
    (GL compute has no dispatch offset, so the full frame is rendered and cropped),
  * `tan_bits`: llvmpipe's own value of tan(radians(fov)*0.5) (probe mode), which lets a test
    feed the restatement the same constant and compare the rest bit-for-bit.
Also writes probes.npz: llvmpipe outputs of the GLSL built-ins / expression shapes whose
lowering the restatement depends on.

`--only refscenes` renders the three scene files the reference ships (tests/golden/scenes) into ref_default / ref_simple /
ref_performance_test, `--only ref_frame` the reference's post chain on its own frame of two of them into ref_frame_* (see
make_refscenes / make_ref_frame); these fixtures hold no timings, so two runs write identical arrays.
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from opengl_raytracing_amd import host, scenes  # noqa: E402
from opengl_raytracing_amd import layout as L  # noqa: E402
from oracle import binding as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SHARDS = {"c5_8k": [["objects", "lights", "params", "tan_bits", "frame_count", "max_ray_depth", "strip_dispatch_s",
                     "column_dispatch_s", "win8k_origins", "win8k_color", "renderer"], ["win8k_pos", "win8k_normal"]],
          "trig": [["trig_in", "trig_out"], ["fov_in", "fov_tan", "explog_in"], ["explog_out"]]}


# ---- the reference's own scene files (tests/golden/scenes, verbatim copies of res/Scene) --------------------------------------
REF_SCENES = {"ref_default": "default.scene", "ref_simple": "SIMPLE.scene", "ref_performance_test": "performance_test.scene"}
REF_FULL = 800                        # WIDTH = HEIGHT of the reference's window
REF_DEPTH = 3                         # MAX_RAY_DEPTH as shipped
# whole-frame size per view: 96 for every view would take the three fixtures past 4 MiB; `corner` keeps 96 because at 64 its
# frame of default.scene (23 % hits) holds 892 distinct red values, under the 1000 the case checks of the tests ask of a view
REF_VIEW_SIZES = {"shipped": 128, "corner": 96}
REF_VIEW_SIZE = 64
# view -> (position, yaw, pitch): Camera::UpdateVectors' angles (the shipped pose is yaw -90, pitch 0 at the origin)
REF_VIEWS = {"shipped": ((0.0, 0.0, 0.0), -90.0, 0.0), "down": ((0.0, 4.0, 2.0), -90.0, -60.0),
             "corner": ((-8.0, -8.0, 8.0), -45.0, 20.0), "inglass": ((0.0, 2.0, -3.0), -60.0, -15.0),
             "behind": ((0.0, 1.0, -9.0), 90.0, 0.0), "steep": ((1.0, 6.0, -4.0), -90.0, -89.0)}
# setting -> (MAX_RAY_DEPTH, shadowType written into every light); rendered for the views of REF_SETTING_VIEWS
REF_SETTINGS = {"noshadow": (1, 0), "pcss": (8, 2)}
REF_SETTING_VIEWS = ("shipped", "steep")
REF_CASES = list(REF_VIEWS) + [f"{v}_{s}" for v in REF_SETTING_VIEWS for s in REF_SETTINGS]
# One case more in ref_performance_test.  Every plane normal of the three files is of unit length ("LeftWall -10 0 0 1 1 0 0" is
# position, radius 1, normal (1, 0, 0)), so an intersectPlane that normalised its normal would pass all of the above.  `wall_tilted`
# is that file with LeftWall's / RightWall's normals set to (1, 1, 0) / (-1, -1, 0) and the AABBs regenerated, seen from a pose
# that faces LeftWall: half of the frame's last hits lie on the tilted walls.
REF_TILTED = ("ref_performance_test", "wall_tilted", ((-2.0, 3.0, 0.0), 180.0, -30.0), {"LeftWall": (1.0, 1.0, 0.0), "RightWall": (-1.0, -1.0, 0.0)})
REF_FRAME_SCENES = {"ref_frame_default": "default.scene", "ref_frame_performance_test": "performance_test.scene"}
REF_FRAME_SIZE = 128                  # the size at which all eleven bloom stages of the oracle equal llvmpipe's bit for bit


def _case_keys(case):
    return [f"{case}_{k}" for k in ("params", "color", "pos", "normal")]


def _ref_scene_shards(name):
    head = ["objects", "lights", "frame_count", "has_noise", "has_skybox", "full_size", "max_ray_depth", "tan_bits", "renderer",
            "cases", "shipped_fc7_params"] + [f"{s}_lights" for s in REF_SETTINGS]
    wins = ["win_params", "win_origins", "win_color", "win_pos", "win_normal"]
    views = [v for v in REF_VIEWS if v != "shipped"]
    extra = ["tilted_objects"] + _case_keys(REF_TILTED[1]) if name == REF_TILTED[0] else []
    return [head + _case_keys("shipped") + wins, sum((_case_keys(f"shipped_{s}") for s in REF_SETTINGS), []),
            sum((_case_keys(v) for v in views), []) + sum((_case_keys(f"steep_{s}") for s in REF_SETTINGS), []) + extra]


def _ref_frame_shards():
    head = ["objects", "lights", "frame_count", "has_noise", "has_skybox", "params", "renderer", "blend", "scene", "combined"]
    return [head, ["stages"]] + [[f"taa{k}_{n}" for n in ("params", "current", "history", "normal", "out")] for k in range(3)]


SHARDS.update({name: _ref_scene_shards(name) for name in REF_SCENES})
SHARDS.update({name: _ref_frame_shards() for name in REF_FRAME_SCENES})


def save_sharded(name, data):
    """<name>.part1.npz, <name>.part2.npz, ... with the keys of SHARDS[name] (conftest.load_golden joins them): every
    committed file stays under 1 MiB."""
    assert sorted(k for part in SHARDS[name] for k in part) == sorted(data)
    for i, keys in enumerate(SHARDS[name], 1):
        np.savez_compressed(os.path.join(OUT, f"{name}.part{i}.npz"), **{k: data[k] for k in keys})


WIN = 32
WINDOW_FRACS = [(0.10, 0.10), (0.50, 0.20), (0.80, 0.15), (0.30, 0.45),
                (0.60, 0.50), (0.45, 0.30), (0.20, 0.70), (0.70, 0.75)]
# config -> (low-res size, render full resolution?)
PLAN = {
    "c1": (1, (128, 128), True),
    "c2": (2, (240, 135), True),
    "c3": (3, (240, 135), True),
    "c4": (4, (160, 90), True),
    "c5": (5, (160, 90), False),   # 8K x 256 objects x depth 8 is ~2 h on 8 vCPUs: low-res + 1080p only
    "nan": ("nan", (96, 96), False),
}


def probe_tan(fov_deg):
    glsl = """#version 430 core
layout(local_size_x = 1) in;
layout(std430, binding = 0) buffer In { float xin[]; };
layout(std430, binding = 1) buffer Out { float xout[]; };
void main() { xout[0] = tan(radians(xin[0]) * 0.5); }
"""
    out = O.run_probe(glsl, np.array([fov_deg], dtype=np.float32), np.float32, 1, 1)
    return int(out.view(np.int32)[0])


def windows(w, h):
    res = []
    for fx, fy in WINDOW_FRACS:
        x0 = min(max(int(fx * w) - WIN // 2, 0), w - WIN)
        y0 = min(max(int(fy * h) - WIN // 2, 0), h - WIN)
        res.append((x0, y0))
    return res


def params_bytes(p):
    return np.frombuffer(bytes(p), dtype=np.uint8).copy()


def run(sc, p, tag):
    t = time.time()
    col, pos, nrm, info = O.run_reference(sc, p, repeat=0)
    print(f"  [{tag}] {p.width}x{p.height} depth {p.maxRayDepth}: llvmpipe {info['first_dispatch_s']:.2f}s "
          f"(wall {time.time() - t:.1f}s)", flush=True)
    return col, pos, nrm.astype(np.float16), info


def make_config(name, skip_fullres):
    cfg, lowres, full = PLAN[name]
    sc = scenes.nan_parity_scene(host.generate_aabb) if cfg == "nan" else scenes.make_scene(cfg, host.generate_aabb)
    data = {
        "objects": np.frombuffer(sc.objects.tobytes(), dtype=np.uint8).copy(),
        "lights": np.frombuffer(sc.lights.tobytes(), dtype=np.uint8).copy(),
        "frame_count": np.int32(sc.frame_count),
        "has_noise": np.int32(sc.noise is not None),
        "has_skybox": np.int32(bool(sc.use_skybox)),
        "full_size": np.array([sc.width, sc.height], dtype=np.int32),
        "max_ray_depth": np.int32(sc.max_ray_depth),
    }
    p = sc.params(width=lowres[0], height=lowres[1])
    data["tan_bits"] = np.int32(probe_tan(p.fovDeg))
    col, pos, nrm, info = run(sc, p, name + " lowres")
    data["lowres_params"] = params_bytes(p)
    data["lowres_color"], data["lowres_pos"], data["lowres_normal"] = col, pos, nrm
    data["renderer"] = np.array(info["renderer"] + " / " + info["version"])
    if full and not skip_fullres:
        p = sc.params()
        col, pos, nrm, info = run(sc, p, name + " full")
        wins = windows(sc.width, sc.height)
        data["win_params"] = params_bytes(p)
        data["win_origins"] = np.array(wins, dtype=np.int32)
        data["win_color"] = np.stack([col[y:y + WIN, x:x + WIN] for x, y in wins])
        data["win_pos"] = np.stack([pos[y:y + WIN, x:x + WIN] for x, y in wins])
        data["win_normal"] = np.stack([nrm[y:y + WIN, x:x + WIN] for x, y in wins])
        data["full_dispatch_s"] = np.float64(info["first_dispatch_s"])
    elif cfg == 5 and not skip_fullres:
        # C5's scene at 1920x1080 (chain the evidence through a downscale)
        p = sc.params(width=1920, height=1080)
        col, pos, nrm, info = run(sc, p, name + " 1080p")
        wins = windows(1920, 1080)
        data["win_params"] = params_bytes(p)
        data["win_origins"] = np.array(wins, dtype=np.int32)
        data["win_color"] = np.stack([col[y:y + WIN, x:x + WIN] for x, y in wins])
        data["win_pos"] = np.stack([pos[y:y + WIN, x:x + WIN] for x, y in wins])
        data["win_normal"] = np.stack([nrm[y:y + WIN, x:x + WIN] for x, y in wins])
    np.savez_compressed(os.path.join(OUT, f"{name}.npz"), **data)


PROBE_HEAD = """#version 430 core
layout(local_size_x = 64) in;
layout(std430, binding = 0) buffer In { vec4 xin[]; };
layout(std430, binding = 1) buffer Out { float xout[]; };
"""


def make_probes():
    """llvmpipe's outputs for the expression shapes whose lowering the oracle mirrors."""
    rng = np.random.default_rng(20250222)
    n = 1024
    out = {}
    # 1. scalar built-ins / shapes: rows of (a, b, c, d)
    x = rng.uniform(0, 1, (n, 4)).astype(np.float32)
    x[:, 1] = rng.uniform(-3, 3, n)
    glsl = PROBE_HEAD + """
float haltonSequence(int index, int base) {
    float result = 0.0; float f = 1.0 / base; int i = index;
    while(i > 0) { result += f * (i % base); i = i / base; f = f / base; }
    return result;
}
void main() {
    uint i = gl_GlobalInvocationID.x;
    float a = xin[i].x, b = xin[i].y, c = xin[i].z, d = xin[i].w;
    xout[i*8u+0u] = a + (1.0 - a) * c;               // F0 + (1-F0)*p     (:241)
    xout[i*8u+1u] = c * (1.0 - a) + a;               // NdotV*(1-k)+k     (:236)
    xout[i*8u+2u] = pow(a, 2.0) * (c * c - 1.0) + 1.0; // NDF inner       (:231)
    xout[i*8u+3u] = c * c / (3.14159265359 * pow(b, 2.0)); // PI*pow(x,2), x*x used once (:231)
    xout[i*8u+4u] = pow(b, 5.0);                     // negative base -> NaN
    xout[i*8u+5u] = haltonSequence(int(i), 2);
    xout[i*8u+6u] = haltonSequence(int(i), 3);
    xout[i*8u+7u] = 1.0 - a * (a * (1.0 - d * d));   // refract's k
}
"""
    out["scalar_in"] = x
    out["scalar_out"] = O.run_probe(glsl, x, np.float32, n * 8, n // 64).reshape(n, 8)
    # 2. vec3 built-ins: pairs of rows (a.xyz, t) (b.xyz, _)
    v = rng.uniform(-1, 1, (2 * n, 4)).astype(np.float32)
    v[0::2, 3] = rng.uniform(0, 1, n)
    for key, expr in [("mix_var", "mix(a, b, t)"), ("mix_const", "mix(vec3(0.04), b, t)"),
                      ("normalize", "normalize(a)"), ("reflect", "reflect(a, b)"),
                      ("refract", "refract(normalize(a), normalize(b), 0.3 + t)"), ("cross", "cross(a, b)")]:
        glsl = PROBE_HEAD + """
void main() {
    uint i = gl_GlobalInvocationID.x;
    vec3 a = xin[2u*i].xyz; float t = xin[2u*i].w; vec3 b = xin[2u*i+1u].xyz;
    vec3 m = %s;
    xout[i*4u+0u] = m.x; xout[i*4u+1u] = m.y; xout[i*4u+2u] = m.z; xout[i*4u+3u] = dot(a, b);
}
""" % expr
        out[key] = O.run_probe(glsl, v, np.float32, n * 4, n // 64).reshape(n, 4)
    out["vec_in"] = v
    np.savez_compressed(os.path.join(OUT, "probes.npz"), **out)
    print("  [probes] written", flush=True)


def make_taa():
    """TAA resolve fixture: the reference's taaFs.glsl + outputVs.glsl run on
    llvmpipe through gl_harness' postfx mode, fed with two consecutive oracle renders of the C2
    scene (the second with the objects moved, as history) and the first one's gNormal."""
    R = "/root/reference/shader/"
    sc = scenes.make_scene(2, host.generate_aabb)
    out = {}
    for tag, (W, H, fc, blend) in {"a": (96, 64, 5, 0.1), "b": (50, 37, 0, 0.5), "c": (64, 48, 3, 0.25)}.items():
        p = sc.params(width=W, height=H)
        cur, _, nrm, _ = O.render(sc, p)
        moved = scenes.make_scene(2, host.generate_aabb)
        moved.objects["position"][:, 0] += 0.07
        host.generate_aabb(moved.objects)
        hist, _, _, _ = O.render(moved, p)
        jx, jy = host.taa_jitter(fc, W, H)
        res = O.run_postfx(R + "outputVs.glsl", R + "taaFs.glsl", W, H,
                           [("uCurrentFrame", cur, dict(linear=True)), ("uHistory", hist, dict(linear=True, clamp=True)),
                            ("gNormal", nrm.astype(np.float32), dict(half=True))],
                           [("uBlendFactor", float(blend)), ("uJitterX", float(jx)), ("uJitterY", float(jy))])
        out[f"{tag}_current"], out[f"{tag}_history"], out[f"{tag}_normal"] = cur, hist, nrm
        out[f"{tag}_params"] = np.array([fc, blend, jx, jy], dtype=np.float64)
        out[f"{tag}_out"] = res
    np.savez_compressed(os.path.join(OUT, "taa.npz"), **out)
    print("  [taa] written", flush=True)


def make_bloom():
    """Bloom fixture: the reference's extract / blur / combine fragment shaders chained
    on llvmpipe exactly like ForwardShadingPipeline.cpp:189-228 (threshold 1.0, 10 alternating blur passes
    starting horizontal, strength 0.5), on an oracle render of the C2 scene scaled into HDR range."""
    R = "/root/reference/shader/"
    VS = R + "outputVs.glsl"
    sc = scenes.make_scene(2, host.generate_aabb)
    out = {}
    for tag, (W, H, gain) in {"a": (96, 64, 2.5), "b": (50, 37, 4.0)}.items():
        cur, _, _, _ = O.render(sc, sc.params(width=W, height=H))
        cur = (cur * np.float32(gain)).astype(np.float32)
        cur[..., 3] = 1.0
        tex = O.run_postfx(VS, R + "brightness_extractFS.glsl", W, H, [("hdrTexture", cur, dict(linear=True))],
                           [("threshold", 1.0)], out_half=True)
        stages = [tex]
        horizontal = True
        for _ in range(10):
            tex = O.run_postfx(VS, R + "gaussian_blurFs.glsl", W, H, [("image", tex, dict(half=True, linear=True, clamp=True))],
                               [("horizontal", int(horizontal))], out_half=True)
            stages.append(tex)
            horizontal = not horizontal
        comb = O.run_postfx(VS, R + "bloom_combineFs.glsl", W, H,
                            [("scene", cur, dict(linear=True)), ("bloomBlur", tex, dict(half=True, linear=True, clamp=True))],
                            [("bloomStrength", 0.5)])
        out[f"{tag}_scene"] = cur
        out[f"{tag}_stages"] = np.stack(stages).astype(np.float16)      # exact: the targets are rgba16f
        out[f"{tag}_combined"] = comb
    np.savez_compressed(os.path.join(OUT, "bloom.npz"), **out)
    print("  [bloom] written", flush=True)


def make_ssao():
    """SSAO fixture: ssaoFs.glsl and ssao_blurFs.glsl run unmodified on llvmpipe over oracle
    G-buffers (gPosition rgba32f, gNormal rgba16f, NEAREST / default REPEAT) with the glm view / projection
    matrices of Camera.h:36-42 and an AO.cpp:23-51-style kernel.  Also the llvmpipe lowering probes the
    restatement relies on (mat*vec association, projection*view*p = projection*(view*p), smoothstep).
    Image widths avoid W | 800*(x+0.5): there every pixel centre sits exactly on a rotation-texel boundary
    (TexCoords * 200 on a 4-texel REPEAT texture) and the reference's own result hangs on interpolation ulps."""
    R = "/root/reference/shader/"
    VS = R + "outputVs.glsl"
    samples, noise = host.ssao_kernel()
    out = {"samples": samples, "noise": noise}
    for tag, (cfg, W, H) in {"a": (2, 160, 90), "b": (5, 128, 64), "c": (1, 96, 54)}.items():
        sc = scenes.make_scene(cfg, host.generate_aabb)
        p = sc.params(width=W, height=H)
        _, pos, nrm, _ = O.render(sc, p)
        nrm = np.ascontiguousarray(nrm).view(np.float16).reshape(H, W, 4)
        if tag == "c":      # a patch of primary-miss texels: position 0, normal 0 (normalize -> NaN)
            pos[5:15, 10:30] = 0.0
            nrm[5:15, 10:30] = 0.0
        view, proj = host.camera_matrices(p.camPos[:], p.camDir[:], p.camUp[:], p.fovDeg, W / H)
        uni = [(f"samples[{i}]", tuple(samples[i])) for i in range(64)] + [("projection", tuple(proj)), ("view", tuple(view))]
        ao = O.run_postfx(VS, R + "ssaoFs.glsl", W, H, [("gPosition", pos, {}), ("gNormal", nrm.astype(np.float32), dict(half=True)),
                                                         ("texNoise", noise, {})], uni)[..., 0]
        rep = np.repeat(ao[..., None], 4, axis=2)
        blur_v = O.run_postfx(VS, R + "ssao_blurFs.glsl", W, H, [("ssaoInput", rep, {})], [("horizontal", 0)])[..., 0]
        blur_h = O.run_postfx(VS, R + "ssao_blurFs.glsl", W, H, [("ssaoInput", rep, {})], [("horizontal", 1)])[..., 0]
        out.update({f"{tag}_pos": pos, f"{tag}_nrm": nrm, f"{tag}_view": view, f"{tag}_proj": proj, f"{tag}_ao": ao,
                    f"{tag}_blur_v": blur_v, f"{tag}_blur_h": blur_h})
        print(f"  [ssao {tag}] cfg {cfg} {W}x{H}: mean ao {np.nanmean(ao):.4f}, NaN {np.isnan(ao).mean():.4f}", flush=True)
    # lowering probes (micro-kernels): M*v, A*B*w, smoothstep on random data
    n = 1024
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((n, 48)) * rng.choice([0.01, 1, 30], (n, 48))).astype(np.float32)
    glsl = """#version 430
layout(local_size_x=64) in;
layout(std430,binding=0) buffer I {float a[];};
layout(std430,binding=1) buffer Oo {float o[];};
void main(){ uint g=gl_GlobalInvocationID.x; uint b=g*48u;
 mat3 M=mat3(vec3(a[b],a[b+1],a[b+2]),vec3(a[b+3],a[b+4],a[b+5]),vec3(a[b+6],a[b+7],a[b+8]));
 vec3 v=vec3(a[b+9],a[b+10],a[b+11]);
 mat4 A,B; for(int c=0;c<4;c++){A[c]=vec4(a[b+12+c*4],a[b+13+c*4],a[b+14+c*4],a[b+15+c*4]);B[c]=vec4(a[b+28+c*4],a[b+29+c*4],a[b+30+c*4],a[b+31+c*4]);}
 vec4 w=vec4(a[b+44],a[b+45],a[b+46],1.0);
 vec3 r=M*v; vec4 q=A*B*w;
 float sm=smoothstep(0.0,1.0,0.5/abs(a[b+44]-a[b+45]));
 uint ob=g*8u; o[ob]=r.x;o[ob+1]=r.y;o[ob+2]=r.z; o[ob+3]=q.x;o[ob+4]=q.y;o[ob+5]=q.z;o[ob+6]=q.w; o[ob+7]=sm; }"""
    out["probe_in"] = x
    out["probe_out"] = O.run_probe(glsl, x, np.float32, n * 8, n // 64).reshape(n, 8)
    np.savez_compressed(os.path.join(OUT, "ssao.npz"), **out)
    print("  [ssao] written", flush=True)


def _look_at(eye, center, up):
    """glm::lookAtRH, column-major float32[16]."""
    f32 = np.float32
    eye, center, up = (np.asarray(a, f32) for a in (eye, center, up))
    nrm = lambda v: (v * (f32(1) / np.sqrt(np.dot(v, v).astype(f32)))).astype(f32)
    f = nrm(center - eye)
    s_ = nrm(np.cross(f, up).astype(f32))
    u = np.cross(s_, f).astype(f32)
    m = np.zeros((4, 4), f32)
    m[0][0], m[1][0], m[2][0] = s_
    m[0][1], m[1][1], m[2][1] = u
    m[0][2], m[1][2], m[2][2] = -f
    m[3][0], m[3][1], m[3][2], m[3][3] = -np.dot(s_, eye), -np.dot(u, eye), np.dot(f, eye), 1
    return m.ravel()


def _perspective(fovy, aspect, zn, zf):
    f32 = np.float32
    t = f32(np.tan(f32(fovy) / f32(2)))
    m = np.zeros((4, 4), f32)
    m[0][0], m[1][1] = f32(1) / (f32(aspect) * t), f32(1) / t
    m[2][2], m[2][3] = -(f32(zf) + f32(zn)) / (f32(zf) - f32(zn)), -1
    m[3][2] = -(f32(2) * f32(zf) * f32(zn)) / (f32(zf) - f32(zn))
    return m.ravel()


def make_cubemap():
    """Equirect -> cubemap fixture: skyboxVs.glsl + skyboxFs.glsl drawn over a unit cube with
    the six captureViews and the 90-degree captureProjection of TextureLoader.cpp:158-167, on a synthetic HDR
    panorama whose texels are fp16-representable (so the RGB16F upload is exact).  Face sizes are even: with an
    odd size the centre column of the -X face sits exactly on the atan seam (z = +-0) and the reference's own
    texels there flip between the panorama's two edges.  Plus probes of llvmpipe's atan(y,x) / asin lowering and
    of the float -> RGB16F upload rounding."""
    R = "/root/reference/shader/"
    f32 = np.float32
    W, H = 64, 32
    rng = np.random.default_rng(2)
    yy, xx = np.mgrid[0:H, 0:W]
    eqr = np.stack([1 + np.sin(xx / 5.0) + yy / 8.0, 2 + np.cos(yy / 3.0) * np.sin(xx / 7.0), (xx + yy) % 7 / 2.0], -1)
    eqr = ((eqr + rng.uniform(0, 0.3, (H, W, 3))) ** 2).astype(np.float16).astype(f32)
    tex = np.concatenate([eqr, np.ones((H, W, 1), f32)], -1)
    proj = _perspective(np.radians(f32(90.0)), 1.0, 0.1, 10.0)
    views = [((1, 0, 0), (0, -1, 0)), ((-1, 0, 0), (0, -1, 0)), ((0, 1, 0), (0, 0, 1)), ((0, -1, 0), (0, 0, -1)),
             ((0, 0, 1), (0, -1, 0)), ((0, 0, -1), (0, -1, 0))]
    out = {"equirect": eqr}
    for S in (32, 20, 128):
        faces = []
        for tg, up in views:
            ref = O.run_postfx(R + "skyboxVs.glsl", R + "skyboxFs.glsl", S, S,
                               [("equirectangularMap", tex, dict(half=True, linear=True, clamp=True))],
                               [("projection", tuple(proj)), ("view", tuple(_look_at((0, 0, 0), tg, up)))], out_half=True, cube=True)
            assert (ref[..., 3] == 1).all()
            faces.append(ref[..., :3].astype(np.float16))      # exact: the target is rgba16f
        out[f"faces_{S}"] = np.stack(faces)
        print(f"  [cubemap] S={S} done", flush=True)
    n = 4096
    v = rng.standard_normal((n, 3)).astype(f32)
    v[:48] = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [1, 1, 0], [1, 0, 1]] * 6, f32)
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)
    glsl = """#version 430
layout(local_size_x=64) in;
layout(std430,binding=0) buffer I {float a[];};
layout(std430,binding=1) buffer Oo {float o[];};
void main(){ uint g=gl_GlobalInvocationID.x; vec3 v=vec3(a[g*3u],a[g*3u+1u],a[g*3u+2u]);
 o[g*4u]=atan(v.z,v.x); o[g*4u+1u]=asin(v.y); vec2 uv=vec2(atan(v.z,v.x),asin(v.y)); uv*=vec2(0.1591,0.3183); uv+=0.5; o[g*4u+2u]=uv.x; o[g*4u+3u]=uv.y; }"""
    out["probe_v"] = v
    out["probe_out"] = O.run_probe(glsl, v, np.float32, n * 4, n // 64).reshape(n, 4)
    # upload rounding: arbitrary floats into an RGBA16F texture, read back texel-exact through the extract shader
    # (threshold -1: brightness_extractFS.glsl passes the colour through)
    up = np.abs(rng.standard_normal((16, 32, 4))).astype(f32) * rng.choice([1e-3, 1.0, 50.0], (16, 32, 1)).astype(f32)
    up[..., 3] = 1
    out["upload_in"] = up
    out["upload_out"] = O.run_postfx(R + "outputVs.glsl", R + "brightness_extractFS.glsl", 32, 16,
                                     [("hdrTexture", up, dict(half=True, linear=True))], [("threshold", -1.0)])
    np.savez_compressed(os.path.join(OUT, "cubemap.npz"), **out)
    print("  [cubemap] written", flush=True)


def make_c5_8k(strip_groups_y=24, column_groups_x=4, win=48):
    """C5 at its REAL size, 7680x4320 (VERDICT r1 'parity unpinned at 8K'): GL compute has no dispatch offset,
    but the group count is free -- glDispatchCompute(240, GY, 1) on the full-size images runs exactly the
    invocations the full dispatch runs for the bottom 32*GY rows (gl_GlobalInvocationID, imageSize() and hence uv
    and random()'s arguments are those of the 8K frame), and glDispatchCompute(GX, 135, 1) the left 32*GX columns
    over the whole height (gid.y up to 4319: the large random() arguments).  The fixture keeps `win`-pixel
    windows cut from the two regions; the raw strips stay in /tmp (tens of MB)."""
    sc = scenes.make_scene(5, host.generate_aabb)
    p = sc.params()
    W, H = p.width, p.height
    assert (W, H) == (7680, 4320)
    data = {"objects": np.frombuffer(sc.objects.tobytes(), dtype=np.uint8).copy(),
            "lights": np.frombuffer(sc.lights.tobytes(), dtype=np.uint8).copy(),
            "params": params_bytes(p), "tan_bits": np.int32(probe_tan(p.fovDeg)),
            "frame_count": np.int32(sc.frame_count), "max_ray_depth": np.int32(sc.max_ray_depth)}
    origins, cols, poss, nrms = [], [], [], []
    regions = [("strip", (W // 32, strip_groups_y), (0, 0, W, 32 * strip_groups_y)),
               ("column", (column_groups_x, (H + 31) // 32), (0, 0, 32 * column_groups_x, H))]
    rng = np.random.default_rng(58)
    for tag, groups, crop in regions:
        t = time.time()
        col, pos, nrm, info = O.run_reference(sc, p, repeat=0, groups=groups, crop=crop)
        nrm = nrm.astype(np.float16)
        print(f"  [c5_8k {tag}] groups {groups}: llvmpipe {info['first_dispatch_s']:.1f}s (wall {time.time() - t:.1f}s)", flush=True)
        np.savez_compressed(f"/tmp/c5_8k_{tag}.npz", color=col, pos=pos, normal=nrm)
        data[f"{tag}_dispatch_s"] = np.float64(info["first_dispatch_s"])
        rw, rh = crop[2], crop[3]
        # windows on a jittered grid over the region; keep those with content first (hits), then fill with the rest
        nx, ny = max(1, rw // 640), max(1, rh // 360)
        cand = []
        for gy_ in range(ny):
            for gx_ in range(nx):
                x0 = int(min(rw - win, gx_ * rw / nx + rng.integers(0, max(1, rw // nx - win))))
                y0 = int(min(rh - win, gy_ * rh / ny + rng.integers(0, max(1, rh // ny - win))))
                hits = float((pos[y0:y0 + win, x0:x0 + win, 3] == 1).mean())          # all pixels store alpha 1
                var = float(np.nanstd(col[y0:y0 + win, x0:x0 + win, :3]))
                cand.append((var, x0, y0))
        cand.sort(reverse=True)
        for var, x0, y0 in cand[:14]:
            origins.append((crop[0] + x0, crop[1] + y0))
            cols.append(col[y0:y0 + win, x0:x0 + win])
            poss.append(pos[y0:y0 + win, x0:x0 + win])
            nrms.append(nrm[y0:y0 + win, x0:x0 + win])
    data["win8k_origins"] = np.array(origins, dtype=np.int32)
    data["win8k_color"], data["win8k_pos"], data["win8k_normal"] = np.stack(cols), np.stack(poss), np.stack(nrms)
    data["renderer"] = np.array(info["renderer"] + " / " + info["version"])
    save_sharded("c5_8k", data)
    print(f"  [c5_8k] {len(origins)} windows of {win}x{win} written", flush=True)


def make_trig():
    """llvmpipe's sin / cos / tan / log2 / exp2 / pow(x,5) / exp, bitwise (trig.part*.npz).  Pins oracle/rt_oracle.c's
    mesa_* restatements (gallivm's cephes-style sincos with fused multiply-adds, polynomial log2 / exp2): the
    camera's tan(radians(fov)*0.5), cosineWeightedHemisphere's cos/sin(phi), random()'s sin(large), SSS's exp."""
    rng = np.random.default_rng(7)
    n = 1 << 16
    q = n // 8
    x = np.concatenate([rng.uniform(-8, 8, 2 * q), rng.uniform(-1e6, 1e6, 2 * q),
                        (np.arange(q) % 4096 - 2048) * np.float32(np.pi / 2) + rng.normal(0, 1e-3, q),
                        np.radians(np.linspace(0.01, 179.99, q)) * 0.5, rng.uniform(0, 1.6, q),
                        10.0 ** rng.uniform(-30, 9.0, q)]).astype(np.float32)
    x[:6] = [0, -0.0, np.inf, -np.inf, np.nan, 1e9]
    glsl = """#version 430 core
layout(local_size_x = 64) in;
layout(std430, binding = 0) buffer In { float xin[]; };
layout(std430, binding = 1) buffer Out { float xout[]; };
void main(){ uint i=gl_GlobalInvocationID.x; float a=xin[i]; xout[3u*i]=sin(a); xout[3u*i+1u]=cos(a); xout[3u*i+2u]=tan(a); }
"""
    out = {"trig_in": x, "trig_out": O.run_probe(glsl, x, np.float32, 3 * n, n // 64).reshape(n, 3)}
    # the exact expression of generateCameraRay (:209) over fov in (0, 180)
    fov = np.concatenate([np.linspace(0.05, 179.95, n - 64), np.array([20, 30, 45, 60, 75, 90, 100, 120] * 8)]).astype(np.float32)
    glsl = """#version 430 core
layout(local_size_x = 64) in;
layout(std430, binding = 0) buffer In { float xin[]; };
layout(std430, binding = 1) buffer Out { float xout[]; };
void main(){ uint i=gl_GlobalInvocationID.x; xout[i]=tan(radians(xin[i]) * 0.5); }
"""
    out["fov_in"] = fov
    out["fov_tan"] = O.run_probe(glsl, fov, np.float32, n, n // 64)
    y = np.concatenate([rng.uniform(0, 1, n // 2), rng.uniform(-20, 20, n // 4), 10.0 ** rng.uniform(-20, 10, n // 4)]).astype(np.float32)
    y[:6] = [0, -0.0, np.inf, -np.inf, np.nan, 1.0]
    glsl = """#version 430 core
layout(local_size_x = 64) in;
layout(std430, binding = 0) buffer In { float xin[]; };
layout(std430, binding = 1) buffer Out { float xout[]; };
void main(){ uint i=gl_GlobalInvocationID.x; float a=xin[i]; xout[4u*i]=log2(a); xout[4u*i+1u]=exp2(a); xout[4u*i+2u]=pow(a,5.0); xout[4u*i+3u]=exp(a); }
"""
    out["explog_in"] = y
    out["explog_out"] = O.run_probe(glsl, y, np.float32, 4 * n, n // 64).reshape(n, 4)
    save_sharded("trig", out)
    print("  [trig] written", flush=True)


def _ref_scene(fname, view="shipped", pose=None):
    """One of the reference's shipped scene files (tests/golden/scenes: the bytes of res/Scene) through host.parse_scene, with the
    camera of Camera::UpdateVectors at `view` and the reference's window and depth."""
    path = os.path.join(OUT, "scenes", fname)
    text = open(path).read()
    theirs = os.path.join("/root/reference/res/Scene", fname)
    assert open(theirs, "rb").read() == open(path, "rb").read(), f"{fname} is no longer the reference's file"
    objs, lts = host.parse_scene(text)
    pos, yaw, pitch = pose or REF_VIEWS[view]
    f, r, u = host.camera_vectors(yaw, pitch)
    cam = dict(cam_pos=pos, cam_dir=f, cam_right=r, cam_up=u, fov_deg=45.0)
    return scenes.Scene(fname, objs, lts, REF_FULL, REF_FULL, REF_DEPTH, cam)


def _same_surfaces(a, b):
    return all(np.array_equal(np.asarray(x, np.float32), np.asarray(y, np.float32), equal_nan=True) for x, y in zip(a[:3], b[:3]))


def make_refscenes(name):
    """ref_default / ref_simple / ref_performance_test: the scene files the reference ships, as its own shader draws them on
    llvmpipe -- six views (REF_VIEWS), `shipped` and `steep` also without shadows at depth 1 and with PCSS on every light at
    depth 8 (the NaN pixels stay in), and eight 32x32 windows of the real 800x800 frame.  Checked here and not stored: the shipped
    16x16 dispatch writes the bytes of the exact one, and frameCount 7 the bytes of frameCount 0 (no noise texture is bound, no
    object has a diffuseStrength)."""
    fname = REF_SCENES[name]
    sc = _ref_scene(fname)
    data = {"objects": np.frombuffer(sc.objects.tobytes(), dtype=np.uint8).copy(),
            "lights": np.frombuffer(sc.lights.tobytes(), dtype=np.uint8).copy(),
            "frame_count": np.int32(0), "has_noise": np.int32(0), "has_skybox": np.int32(0),
            "full_size": np.array([REF_FULL, REF_FULL], dtype=np.int32), "max_ray_depth": np.int32(REF_DEPTH),
            "tan_bits": np.int32(probe_tan(45.0)), "cases": np.array(REF_CASES)}
    for view in REF_VIEWS:
        sc = _ref_scene(fname, view)
        size = REF_VIEW_SIZES.get(view, REF_VIEW_SIZE)
        settings = [(view, None, REF_DEPTH, None)]
        if view in REF_SETTING_VIEWS:
            settings += [(f"{view}_{s}", s, depth, stype) for s, (depth, stype) in REF_SETTINGS.items()]
        for case, setting, depth, stype in settings:
            if setting is not None:
                sc.lights["shadowType"] = stype
                data[f"{setting}_lights"] = np.frombuffer(sc.lights.tobytes(), dtype=np.uint8).copy()
            p = sc.params(width=size, height=size, max_ray_depth=depth)
            col, pos, nrm, info = run(sc, p, f"{name} {case}")
            data[f"{case}_params"] = params_bytes(p)
            data[f"{case}_color"], data[f"{case}_pos"], data[f"{case}_normal"] = col, pos, nrm
            if case == "shipped":
                shipped = O.run_reference(sc, p, repeat=0, shipped_dispatch=True)
                assert _same_surfaces(shipped, (col, pos, nrm.astype(np.float32))), "16x16 dispatch differs from the exact one"
                p7 = L.copy_params(p, frameCount=7)
                fc7 = O.run_reference(sc, p7, repeat=0)
                assert _same_surfaces(fc7, (col, pos, nrm.astype(np.float32))), "frameCount 7 differs from frameCount 0"
                print(f"  [{name}] shipped 16x16 dispatch == exact dispatch; frameCount 7 == frameCount 0 (bytes)", flush=True)
                data["shipped_fc7_params"] = params_bytes(p7)
    if name == REF_TILTED[0]:
        _, case, pose, normals = REF_TILTED
        sc = _ref_scene(fname, pose=pose)
        names = [ln.split()[2] for ln in open(os.path.join(OUT, "scenes", fname)) if ln.startswith("OBJECT")]
        for wall, n in normals.items():
            sc.objects["normal"][names.index(wall)] = n
        host.generate_aabb(sc.objects)
        data["tilted_objects"] = np.frombuffer(sc.objects.tobytes(), dtype=np.uint8).copy()
        p = sc.params(width=REF_VIEW_SIZE, height=REF_VIEW_SIZE)
        col, pos, nrm, info = run(sc, p, f"{name} {case}")
        data[f"{case}_params"] = params_bytes(p)
        data[f"{case}_color"], data[f"{case}_pos"], data[f"{case}_normal"] = col, pos, nrm
        data["cases"] = np.array(REF_CASES + [case])
    data["renderer"] = np.array(info["renderer"] + " / " + info["version"])
    # the real frame: 800x800, shipped pose, the window's own 16x16 dispatch checked against the exact one
    sc = _ref_scene(fname)
    p = sc.params()
    col, pos, nrm, info = run(sc, p, f"{name} full")
    shipped = O.run_reference(sc, p, repeat=0, shipped_dispatch=True)
    assert _same_surfaces(shipped, (col, pos, nrm.astype(np.float32))), "800x800: 16x16 dispatch differs from the exact one"
    print(f"  [{name}] 800x800: shipped 16x16 dispatch == exact dispatch (bytes)", flush=True)
    wins = windows(REF_FULL, REF_FULL)
    data["win_params"] = params_bytes(p)
    data["win_origins"] = np.array(wins, dtype=np.int32)
    data["win_color"] = np.stack([col[y:y + WIN, x:x + WIN] for x, y in wins])
    data["win_pos"] = np.stack([pos[y:y + WIN, x:x + WIN] for x, y in wins])
    data["win_normal"] = np.stack([nrm[y:y + WIN, x:x + WIN] for x, y in wins])
    save_sharded(name, data)       # (no timings in these fixtures: two runs of the generator write identical arrays)


def _taa_blend_default():
    """m_TAABlendFactor's initialiser in the reference's UI header: the blend factor a user who touches nothing runs with."""
    import re
    m = re.search(r"m_TAABlendFactor\s*=\s*([0-9.]+)f", open("/root/reference/src/ImGUIManager.h", errors="replace").read())
    return float(np.float32(m.group(1)))


def make_ref_frame(name):
    """ref_frame_default / ref_frame_performance_test: the post chain of ForwardShadingPipeline.cpp:189-259 on llvmpipe's OWN
    raytraced frame of the shipped view at 128x128 -- extract (threshold 1.0), ten alternating blurs starting horizontal,
    combine (strength 0.5), then three TAA frames (frameCount 0, 1, 2; history ping-pong from zeros, the UI's default blend)."""
    R = "/root/reference/shader/"
    VS = R + "outputVs.glsl"
    W = H = REF_FRAME_SIZE
    sc = _ref_scene(REF_FRAME_SCENES[name])
    p = sc.params(width=W, height=H)
    cur, _, nrm, info = run(sc, p, name)
    out = {"objects": np.frombuffer(sc.objects.tobytes(), dtype=np.uint8).copy(),
           "lights": np.frombuffer(sc.lights.tobytes(), dtype=np.uint8).copy(),
           "frame_count": np.int32(0), "has_noise": np.int32(0), "has_skybox": np.int32(0), "params": params_bytes(p),
           "renderer": np.array(info["renderer"] + " / " + info["version"])}
    assert (cur[..., 3] == 1).all()
    tex = O.run_postfx(VS, R + "brightness_extractFS.glsl", W, H, [("hdrTexture", cur, dict(linear=True))],
                       [("threshold", 1.0)], out_half=True)
    stages = [tex]
    horizontal = True
    for _ in range(10):
        tex = O.run_postfx(VS, R + "gaussian_blurFs.glsl", W, H, [("image", tex, dict(half=True, linear=True, clamp=True))],
                           [("horizontal", int(horizontal))], out_half=True)
        stages.append(tex)
        horizontal = not horizontal
    out["scene"] = cur
    out["stages"] = np.stack(stages).astype(np.float16)      # exact: the targets are rgba16f
    out["combined"] = O.run_postfx(VS, R + "bloom_combineFs.glsl", W, H,
                                   [("scene", cur, dict(linear=True)), ("bloomBlur", tex, dict(half=True, linear=True, clamp=True))],
                                   [("bloomStrength", 0.5)])
    blend = _taa_blend_default()
    out["blend"] = np.float64(blend)
    hist = [np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)]
    for fc in range(3):
        pf = L.copy_params(p, frameCount=fc)
        cur, _, nrm, _ = run(sc, pf, f"{name} frameCount {fc}")
        jx, jy = host.taa_jitter(fc, W, H)
        k = fc % 2                                           # currentHistory (ForwardShadingPipeline.cpp:142)
        res = O.run_postfx(VS, R + "taaFs.glsl", W, H,
                           [("uCurrentFrame", cur, dict(linear=True)), ("uHistory", hist[1 - k], dict(linear=True, clamp=True)),
                            ("gNormal", nrm.astype(np.float32), dict(half=True))],
                           [("uBlendFactor", float(blend)), ("uJitterX", float(jx)), ("uJitterY", float(jy))])
        out[f"taa{fc}_params"] = np.array([fc, blend, jx, jy], dtype=np.float64)
        out[f"taa{fc}_current"], out[f"taa{fc}_history"], out[f"taa{fc}_normal"], out[f"taa{fc}_out"] = cur, hist[1 - k].copy(), nrm, res
        hist[k] = res
    save_sharded(name, out)
    print(f"  [{name}] written (blend {blend})", flush=True)


def make_surface_probes():
    """rgba16f imageStore rounding + cubemap sampling through a render-mode job with a tiny
    custom shader is not needed: both are exercised by the c5/nan fixtures.  (Kept as a hook.)"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--skip-fullres", action="store_true")
    args = ap.parse_args()
    if not O.harness_available():
        sys.exit("gl_harness or /root/reference is not available: goldens can only be generated in the build container")
    names = [s for s in args.only.split(",") if s] or list(PLAN) + ["probes", "taa", "bloom", "ssao", "cubemap", "c5_8k", "trig", "refscenes", "ref_frame"]
    for nme in names:
        print(f"== {nme}", flush=True)
        if nme == "probes":
            make_probes()
        elif nme == "taa":
            make_taa()
        elif nme == "bloom":
            make_bloom()
        elif nme == "ssao":
            make_ssao()
        elif nme == "cubemap":
            make_cubemap()
        elif nme == "c5_8k":
            make_c5_8k()
        elif nme == "trig":
            make_trig()
        elif nme == "refscenes":
            for ref in REF_SCENES:
                make_refscenes(ref)
        elif nme == "ref_frame":
            for ref in REF_FRAME_SCENES:
                make_ref_frame(ref)
        else:
            make_config(nme, args.skip_fullres)


if __name__ == "__main__":
    main()
