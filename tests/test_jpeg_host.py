"""CPU-only tests of the JPEG output's host side (include/rt_mi355.h): rt_jpeg_quant, rt_jpeg_dct_matrix, rt_jpeg_header and
rt_jpeg_layout against the definition restated in tests/jpeg_oracle.py, the byte layout of the two records, the refusals, the
coefficient bounds the definition states -- and, where Pillow is installed, that the oracle's streams are files: every one decodes at
the right size, with a luma error no more than 2 % plus 0.5 code above that of Pillow's own encoder on the same planes (the two
differ only in where the DCT rounds; the largest excesses measured are in DESIGN.md 29).  No GPU call is made."""
import ctypes
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import jpeg_oracle as JO
from opengl_raytracing_amd import layout as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, TOO_LARGE = -1, -4


@pytest.mark.parametrize("quality", range(1, 101))
def test_quant_matches_the_formula(host, quality):
    luma, chroma = host.jpeg_quant(quality)
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    for got, base in ((luma, JO.K1), (chroma, JO.K2)):
        assert got.dtype == np.uint8 and got.tolist() == [min(max((b * s + 50) // 100, 1), 255) for b in base]
    assert (luma.tolist(), chroma.tolist()) == JO.quant(quality)


def test_quant_end_points(host):
    assert host.jpeg_quant(50)[0].tolist() == JO.K1 and host.jpeg_quant(50)[1].tolist() == JO.K2
    assert set(host.jpeg_quant(100)[0].tolist()) == {1} and host.jpeg_quant(1)[0].max() == 255


def test_dct_matrix_is_the_double_precision_definition(host):
    m = host.jpeg_dct_matrix()
    assert m.dtype == np.int32 and m.shape == (8, 8)
    for u, x in itertools.product(range(8), repeat=2):
        exact = 16384.0 * (0.5 if u else 1.0 / (2.0 * math.sqrt(2.0))) * math.cos((2 * x + 1) * u * math.pi / 16.0)
        assert abs(abs(exact - math.floor(exact)) - 0.5) > 1e-3            # no entry near a tie: the rounding mode cannot matter
        assert m[u, x] == round(exact)
        assert m[u, 7 - x] == (-1) ** u * m[u, x]                            # the symmetry an even/odd split may use
    assert (m == JO.dct_matrix()).all()


@pytest.mark.parametrize("w,h,quality,interval", [(1, 1, 50, 1), (37, 19, 90, 3), (65535, 1, 1, 65535), (640, 360, 100, 40)])
def test_header_matches_the_oracle(host, w, h, quality, interval):
    got = host.jpeg_header(w, h, quality, interval)
    assert got.size == L.JPEG_HEADER_BYTES == 629
    assert (got == JO.header(w, h, quality, interval)).all()


@pytest.mark.parametrize("w,h,interval", [(1, 1, 1), (16, 16, 1), (17, 17, 3), (37, 19, 2), (1920, 1080, 120), (1920, 1080, 1), (65535, 1, 65535)])
def test_layout(host, w, h, interval):
    lay = host.jpeg_layout(w, h, 75, interval)
    mw, mh, n_mcu, n_seg = JO.geometry(w, h, interval)
    assert (lay.n_mcu, lay.n_segments) == (n_mcu, n_seg)
    assert lay.worst_bytes == 629 + n_mcu * 2488 + 2 * (n_seg - 1) + 2 == JO.worst_bytes(w, h, interval)
    assert lay.offset[0] == 0 and lay.offset[1] >= n_mcu * 6 * 64 * 2 and lay.offset[2] >= lay.offset[1] + 4 * (n_seg + 1)
    assert all(o % 16 == 0 for o in lay.offset) and lay.scratch_bytes % 16 == 0
    yuv = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
    assert lay.scratch_bytes >= lay.offset[2] + 8 * n_seg + yuv            # the private region: two words per segment, the planes


def test_record_layouts(tmp_path):
    assert ctypes.sizeof(L.RtJpegDesc) == 32 and L.JPEG_STATE_DTYPE.itemsize == 64
    for k, v in dict(width=0, height=4, quality=8, restartInterval=12, reserved=16).items():
        assert getattr(L.RtJpegDesc, k).offset == v, k
    names = ["bytes", "needed", "overflow", "nSegments", "nMcu", "headerBytes", "stuffedBytes", "reserved"]
    assert list(L.JPEG_STATE_DTYPE.names) == names and [L.JPEG_STATE_DTYPE.fields[n][1] for n in names] == [0, 4, 8, 12, 16, 20, 24, 28]
    src = tmp_path / "j.c"
    src.write_text('#include "rt_mi355.h"\n'
                   "int main(void){ rt_jpeg_desc d = {0}; rt_jpeg_state s = {0}; d.restartInterval = 1; s.stuffedBytes = 1;\n"
                   " return sizeof d == 32 && sizeof s == 64 ? 0 : 1; }\n")
    exe = tmp_path / "j"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
    d = L.make_jpeg_desc(1920, 1080)
    assert (d.width, d.height, d.quality, d.restartInterval, list(d.reserved)) == (1920, 1080, 90, L.JPEG_DEFAULT_INTERVAL, [0, 0, 0, 0])


def test_host_functions_refuse(host):
    lib = host.load_library()
    u8, sz = ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t
    luma, chroma = (ctypes.c_uint8 * 64)(*([7] * 64)), (ctypes.c_uint8 * 64)(*([7] * 64))
    for q in (0, -1, 101, 1000):
        assert lib.rt_jpeg_quant(q, luma, chroma) == INVALID
    assert lib.rt_jpeg_quant(50, None, chroma) == INVALID and lib.rt_jpeg_quant(50, luma, None) == INVALID
    assert list(luma) == [7] * 64 and list(chroma) == [7] * 64                # a refused call writes nothing
    assert lib.rt_jpeg_dct_matrix(None) == INVALID

    def desc(**kw):
        d = L.make_jpeg_desc(37, 19, 75, 2)
        for k, v in kw.items():
            if k == "reserved":
                d.reserved[v] = 1
            else:
                setattr(d, k, v)
        return d

    bad = [desc(width=0), desc(width=-1), desc(width=65536), desc(height=0), desc(height=65536), desc(quality=0), desc(quality=101),
           desc(quality=-5), desc(restartInterval=0), desc(restartInterval=65536), desc(restartInterval=-1)] + [desc(reserved=k) for k in range(4)]
    off, scratch, worst, n = (sz * 3)(), sz(5), sz(5), sz(5)
    buf = (ctypes.c_uint8 * 700)(*([9] * 700))
    for k, d in enumerate(bad):
        assert lib.rt_jpeg_layout(ctypes.byref(d), off, ctypes.byref(scratch), ctypes.byref(worst)) == INVALID, k
        assert lib.rt_jpeg_header(ctypes.byref(d), buf, 700, ctypes.byref(n)) == INVALID, k
    good = desc()
    assert lib.rt_jpeg_layout(None, off, ctypes.byref(scratch), ctypes.byref(worst)) == INVALID
    assert lib.rt_jpeg_layout(ctypes.byref(good), None, ctypes.byref(scratch), ctypes.byref(worst)) == INVALID
    assert lib.rt_jpeg_header(None, buf, 700, ctypes.byref(n)) == INVALID
    assert lib.rt_jpeg_header(ctypes.byref(good), None, 700, ctypes.byref(n)) == INVALID
    assert lib.rt_jpeg_header(ctypes.byref(good), buf, 700, None) == INVALID
    assert lib.rt_jpeg_header(ctypes.byref(good), buf, 628, ctypes.byref(n)) == INVALID
    assert (scratch.value, worst.value, n.value) == (5, 5, 5) and list(buf) == [9] * 700
    assert lib.rt_jpeg_layout(ctypes.byref(good), off, None, None) == 0          # the two sizes are optional
    assert lib.rt_jpeg_header(ctypes.byref(good), buf, 629, ctypes.byref(n)) == 0 and n.value == 629 and list(buf[629:]) == [9] * 71
    # 65535 x 65535 has 2^24 MCUs: the worst stream passes 2^32 - 1 bytes.  The largest square that does not: 1313 x 1313 MCUs
    huge = desc(width=65535, height=65535)
    assert lib.rt_jpeg_layout(ctypes.byref(huge), off, ctypes.byref(scratch), ctypes.byref(worst)) == TOO_LARGE
    assert lib.rt_jpeg_header(ctypes.byref(huge), buf, 700, ctypes.byref(n)) == TOO_LARGE
    edge = desc(width=1313 * 16, height=1313 * 16, restartInterval=65535)
    assert lib.rt_jpeg_layout(ctypes.byref(edge), off, ctypes.byref(scratch), ctypes.byref(worst)) == 0 and worst.value < 2 ** 32
    assert lib.rt_jpeg_layout(ctypes.byref(desc(width=1314 * 16, height=1314 * 16)), off, None, None) == TOO_LARGE


def test_coefficient_bounds_on_the_basis_sign_patterns(host):
    """The blocks that drive one coefficient hardest: sample 255 where a basis function is positive, 0 where it is negative, and the
    inverse -- 128 blocks.  |AC| <= 1020 and -1024 <= DC <= 1016, so AC categories stay <= 10, DC differences <= 11, unclamped."""
    m = host.jpeg_dct_matrix().astype(np.int64)
    assert (m == JO.dct_matrix()).all()
    blocks = []
    for v, u in itertools.product(range(8), repeat=2):
        basis = np.outer(m[v], m[u])
        blocks += [np.where(basis > 0, 255, 0), np.where(basis > 0, 0, 255)]
    F = JO.fdct(np.array(blocks))
    assert F.shape == (128, 8, 8)
    dc, ac = F[:, 0, 0], F.reshape(128, 64)[:, 1:]
    assert (dc.min(), dc.max()) == (-1024, 1016)
    assert np.abs(ac).max() <= 1020 and np.abs(ac).max() >= 900
    assert JO.category(int(np.abs(ac).max())) == 10 and JO.category(1016 + 1024) == 11


# ---- the oracle's streams are files (Pillow) -------------------------------------------------------------------------------------------
SIZES = [(1, 1, 1), (33, 17, 2), (37, 19, 1), (40, 24, 1), (64, 48, 1), (129, 65, 7)]
KINDS = ("ramp", "noise", "checker", "black", "white")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h,interval", SIZES, ids=[f"{w}x{h}" for w, h, _ in SIZES])
def test_oracle_streams_decode_as_well_as_pillows(w, h, interval, kind):
    pytest.importorskip("PIL")
    y, cb, cr = JO.content(kind, w, h, seed=100 * w + h)
    for quality in (1, 50, 90, 100):
        enc = JO.encode(y, cb, cr, quality, interval)
        planes = JO.decode_planes(enc.stream)
        assert planes[0].shape == (h, w) == planes[1].shape == planes[2].shape
        ours, theirs = JO.luma_rms(enc.stream, y), JO.luma_rms(JO.pillow_encode(y, cb, cr, quality), y)
        print(f"{kind} {w}x{h} q{quality}: rms {ours:.4f}, Pillow's {theirs:.4f}, excess {ours - theirs:+.4f}")
        assert ours <= theirs * 1.02 + 0.5, (quality, ours, theirs)
        assert enc.state[0] == enc.stream.size and enc.seg_offsets[-1] == enc.stream.size - 631
        assert enc.stats["rst"] == JO.geometry(w, h, interval)[3] - 1


def test_oracle_inputs_take_the_paths_the_device_tests_rely_on():
    """The statistics the device tests assert on exist and mean what they say."""
    e = JO.encode(*JO.content("black", 37, 19), quality=50, interval=1)
    assert e.stats["eob"] == e.coef.shape[0] and e.stats["zrl"] == 0 and e.stats["max_ac_cat"] == 0 and (e.coef != 0).sum() == 4 * 6
    e = JO.encode(*JO.content("checker", 64, 48), quality=1, interval=1)      # one coefficient survives, at the zigzag's far end
    assert e.stats["zrl"] > 0 and e.stats["rst"] == 11 >= 9
    e = JO.encode(*JO.content("binary", 64, 48, seed=1), quality=100, interval=2)
    assert e.stats["stuffed"] > 0 and e.stats["max_ac_cat"] == 10
    e = JO.encode(*JO.content("blocks", 64, 48), quality=100, interval=65535)
    assert e.stats["max_dc_cat"] == 11 and e.stats["rst"] == 0
