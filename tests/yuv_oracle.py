"""The definition of rt_display_pack_yuv (include/rt_mi355.h) restated in numpy: the oracle of tests/test_yuv_host.py and
tests/test_yuv.py.  Not a test module.  The R'G'B' codes are the toned pack's numpy formula (tests/meter_oracle.py::pack_toned, the
oracle of tests/test_tone.py); the coefficients are the header's formulas in Python floats (doubles; round() is round-half-even);
the 2x2 sums index with clamped coordinates; the integer matrix is numpy int64 with >> (floor, like the arithmetic shift of a
signed 32-bit sum -- and every sum is asserted to fit in 32 bits)."""
import numpy as np

import meter_oracle as MO

FORMATS = ("nv12", "i420")
MATRICES = {"bt709": (0.2126, 0.0722), "bt601": (0.299, 0.114)}       # Kr, Kb
RANGES = {"limited": (219.0 / 255.0, 224.0 / 255.0, 16), "full": (1.0, 1.0, 0)}      # sY, sC, yOff

# the four tables as DESIGN.md 16 lists them: Y (R, G, B), Cb (R, G, B), Cr (R, G, B)
PUBLISHED = {
    ("bt709", "limited"): ((11966, 40254, 4064), (-6596, -22188, 28784), (28784, -26145, -2639)),
    ("bt709", "full"): ((13933, 46871, 4732), (-7509, -25259, 32768), (32768, -29763, -3005)),
    ("bt601", "limited"): ((16829, 33039, 6416), (-9714, -19070, 28784), (28784, -24103, -4681)),
    ("bt601", "full"): ((19595, 38470, 7471), (-11058, -21710, 32768), (32768, -27439, -5329)),
}


def rne(x):
    """Round to nearest even, and check the header's claim that no coefficient is within 0.06 of a tie."""
    assert abs(abs(x - np.floor(x)) - 0.5) > 0.06, x
    return int(round(x))


def coeffs(matrix, rng):
    """-> the twelve words of rt_display_yuv_coeffs as Python ints."""
    Kr, Kb = MATRICES[matrix]
    sY, sC, yOff = RANGES[rng]
    cYR, cYB = rne(65536 * Kr * sY), rne(65536 * Kb * sY)
    cYG = rne(65536 * sY) - cYR - cYB
    cC = rne(32768 * sC)
    cBR = rne(-65536 * sC * Kr / (2 * (1 - Kb)))
    cRB = rne(-65536 * sC * Kb / (2 * (1 - Kr)))
    return [cYR, cYG, cYB, yOff, cBR, -cC - cBR, cC, 0, cC, -cC - cRB, cRB, 0]


def layout(w, h, fmt):
    """-> (offset[3], pitch[3], bytes) of the tightly packed frame."""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    if fmt == "nv12":
        return (0, w * h, w * h + 1), (w, 2 * cw, 2 * cw), w * h + 2 * cw * ch
    assert fmt == "i420"
    return (0, w * h, w * h + cw * ch), (w, cw, cw), w * h + 2 * cw * ch


def _i32(a):
    assert (np.abs(a) < 2 ** 31).all()
    return a


def matrix_unclamped(rgb, c):
    """rgb: integer codes [H, W, 3] in OUTPUT row order -> (Y[H, W], Cb[ch, cw], Cr[ch, cw]) as int64, chroma BEFORE the clamp."""
    rgb = np.asarray(rgb).astype(np.int64)
    assert rgb.min() >= 0 and rgb.max() <= 255
    h, w = rgb.shape[:2]
    cw, ch = (w + 1) // 2, (h + 1) // 2
    R, G, B = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    Y = c[3] + (_i32(c[0] * R + c[1] * G + c[2] * B + 32768) >> 16)
    S = np.zeros((ch, cw, 3), dtype=np.int64)
    for dy in (0, 1):                                          # the literal 2x2 sums, coordinates clamped to the frame
        for dx in (0, 1):
            ys = np.minimum(2 * np.arange(ch) + dy, h - 1)
            xs = np.minimum(2 * np.arange(cw) + dx, w - 1)
            S += rgb[ys][:, xs]
    Rs, Gs, Bs = S[..., 0], S[..., 1], S[..., 2]
    Cb = 128 + (_i32(c[4] * Rs + c[5] * Gs + c[6] * Bs + 131072) >> 18)
    Cr = 128 + (_i32(c[8] * Rs + c[9] * Gs + c[10] * Bs + 131072) >> 18)
    return Y, Cb, Cr


def matrix(rgb, c):
    """-> (Y, Cb, Cr) uint8: luma as computed (asserted to be a byte), chroma clamped to 0..255."""
    Y, Cb, Cr = matrix_unclamped(rgb, c)
    assert Y.min() >= 0 and Y.max() <= 255
    return Y.astype(np.uint8), np.clip(Cb, 0, 255).astype(np.uint8), np.clip(Cr, 0, 255).astype(np.uint8)


def frame(Y, Cb, Cr, fmt):
    """The planes as the flat uint8 frame of `fmt`."""
    if fmt == "nv12":
        return np.concatenate([Y.reshape(-1), np.stack([Cb, Cr], axis=-1).reshape(-1)])
    assert fmt == "i420"
    return np.concatenate([Y.reshape(-1), Cb.reshape(-1), Cr.reshape(-1)])


def frame_from_codes(rgb, fmt, matrix_name, rng):
    return frame(*matrix(rgb, coeffs(matrix_name, rng)), fmt)


def codes(img, transfer, exposure, table, tone="none", white=1.0, dev_exposure=None):
    """The R'G'B' codes [H, W, 3] of an [H, W, 4] float32 image, image row order: the toned pack's bytes."""
    return MO.pack_toned(img, transfer, False, exposure, table, tone, white, dev_exposure)[..., :3]


def pack_yuv(img, table, fmt="nv12", matrix_name="bt709", rng="limited", transfer="srgb", flip=False, exposure=1.0, tone="none",
             white=1.0, dev_exposure=None):
    """img float32 [H, W, 4] -> the flat uint8 frame rt_display_pack_yuv writes."""
    rgb = codes(img, transfer, exposure, table, tone, white, dev_exposure)
    return frame_from_codes(rgb[::-1] if flip else rgb, fmt, matrix_name, rng)
