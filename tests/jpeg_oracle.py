"""The baseline JPEG stream of rt_jpeg_encode (include/rt_mi355.h) restated in numpy: the oracle of tests/test_jpeg_host.py and
tests/test_jpeg.py.  Not a test module.  Planes in (Y, Cb, Cr as rt_display_pack_yuv lays them out, row 0 = top row of the file),
stream out: the integer DCT with the header's two roundings in int64 (every sum is asserted to fit in int32), the IJG-scaled Annex K
quantisers, the Annex K Huffman tables built from their BITS / HUFFVAL lists, restart segments, padding and byte stuffing.  encode()
also returns the coefficient plane, the segment offsets and what the symbols were, so that a test can assert that its input takes
a path (ZRL, EOB, the largest categories, stuffed bytes, the restart index wrapping) instead of hoping so."""
import collections
import math

import numpy as np

HEADER_BYTES = 629
BLOCK_WORST_BYTES = 2488           # 6 blocks of at most 20 + 63 * 26 bits, every byte stuffed

# Annex K.1 / K.2 in natural (row-major) order
K1 = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
K2 = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32

# Annex K.3 - K.6: BITS (codes of length 1..16) and HUFFVAL
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
assert all(sum(b) == len(v) for b, v in (DC_LUMA, DC_CHROMA, AC_LUMA, AC_CHROMA)) and len(AC_LUMA[1]) == len(AC_CHROMA[1]) == 162


def zigzag():
    """-> order[64]: the natural index of zigzag position k (the walk of the anti-diagonals, Figure A.6)."""
    out = []
    for s in range(15):
        cells = [(v, s - v) for v in range(8) if 0 <= s - v < 8]           # (row v, column u), v ascending
        out += [v * 8 + u for v, u in (cells if s % 2 else reversed(cells))]
    return out


ZIGZAG = zigzag()
assert ZIGZAG[:10] == [0, 1, 8, 16, 9, 2, 3, 10, 17, 24] and ZIGZAG[-3:] == [55, 62, 63] and sorted(ZIGZAG) == list(range(64))


def dct_matrix():
    """-> M[u][x] = rne(16384 * a(u) * cos((2x + 1) u pi / 16)) as int64 [8, 8]."""
    m = np.zeros((8, 8), dtype=np.int64)
    for u in range(8):
        a = 1.0 / (2.0 * math.sqrt(2.0)) if u == 0 else 0.5
        for x in range(8):
            m[u, x] = int(round(16384.0 * a * math.cos((2 * x + 1) * u * math.pi / 16.0)))
    return m


def quant(quality):
    """-> (luma[64], chroma[64]) in natural order, the IJG scaling of K.1 / K.2."""
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple([min(max((b * s + 50) // 100, 1), 255) for b in base] for base in (K1, K2))


def huff_codes(bits, vals):
    """-> {symbol: (code, length)} by Annex C."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = (huff_codes(*DC_LUMA), huff_codes(*DC_CHROMA))
AC_CODES = (huff_codes(*AC_LUMA), huff_codes(*AC_CHROMA))


def geometry(w, h, interval):
    mw, mh = (w + 15) // 16, (h + 15) // 16
    n_mcu = mw * mh
    return mw, mh, n_mcu, (n_mcu + interval - 1) // interval


def worst_bytes(w, h, interval):
    _, _, n_mcu, n_seg = geometry(w, h, interval)
    return HEADER_BYTES + n_mcu * BLOCK_WORST_BYTES + 2 * (n_seg - 1) + 2


def header(w, h, quality, interval):
    """-> the 629 bytes in front of the entropy-coded data."""
    be16 = lambda v: [v >> 8, v & 255]
    out = [0xFF, 0xD8]
    out += [0xFF, 0xE0] + be16(16) + list(b"JFIF\0") + [1, 1, 0] + be16(1) + be16(1) + [0, 0]
    for k, q in enumerate(quant(quality)):
        out += [0xFF, 0xDB] + be16(67) + [k] + [q[n] for n in ZIGZAG]
    out += [0xFF, 0xC0] + be16(17) + [8] + be16(h) + be16(w) + [3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]
    for tc_th, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += [0xFF, 0xC4] + be16(19 + len(vals)) + [tc_th] + bits + vals
    out += [0xFF, 0xDD] + be16(4) + be16(interval)
    out += [0xFF, 0xDA] + be16(12) + [3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]
    assert len(out) == HEADER_BYTES
    return np.array(out, dtype=np.uint8)


def blocks_of(y, cb, cr):
    """The planes cut into MCUs with replicated edges -> samples int64 [nMcu * 6, 8, 8] in stream order (Y00 Y01 Y10 Y11 Cb Cr)."""
    h, w = y.shape
    mw, mh = (w + 15) // 16, (h + 15) // 16
    yy = y[np.minimum(np.arange(mh * 16), h - 1)][:, np.minimum(np.arange(mw * 16), w - 1)].astype(np.int64)
    ch, cw = cb.shape
    assert (ch, cw) == ((h + 1) // 2, (w + 1) // 2) == cr.shape
    ri, ci = np.minimum(np.arange(mh * 8), ch - 1), np.minimum(np.arange(mw * 8), cw - 1)
    cbb, crr = cb[ri][:, ci].astype(np.int64), cr[ri][:, ci].astype(np.int64)
    ytiles = yy.reshape(mh, 2, 8, mw, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(mh * mw, 4, 8, 8)
    ctile = lambda p: p.reshape(mh, 8, mw, 8).transpose(0, 2, 1, 3).reshape(mh * mw, 1, 8, 8)
    return np.concatenate([ytiles, ctile(cbb), ctile(crr)], axis=1).reshape(mh * mw * 6, 8, 8)


def fdct(samples):
    """samples [..., 8 (y), 8 (x)] in 0..255 -> F [..., 8 (v), 8 (u)], the header's two passes with their roundings."""
    m = dct_matrix()
    f = samples.astype(np.int64) - 128
    rows = np.einsum("ux,...yx->...yu", m, f)
    assert np.abs(rows).max() < 2 ** 31 - 1024
    r = (rows + 1024) >> 11
    cols = np.einsum("vy,...yu->...vu", m, r)
    assert np.abs(cols).max() < 2 ** 31 - 65536
    return (cols + 65536) >> 17


def quantise(F, q):
    """F [..., 8, 8], q[64] natural -> sign(F) * ((|F| + (Q >> 1)) // Q)."""
    Q = np.array(q, dtype=np.int64).reshape(8, 8)
    return np.sign(F) * ((np.abs(F) + (Q >> 1)) // Q)


def coefficients(y, cb, cr, quality):
    """-> the coefficient plane: int16 [nMcu * 6, 64], zigzag order."""
    F = fdct(blocks_of(y, cb, cr)).reshape(-1, 6, 8, 8)
    ql, qc = quant(quality)
    qz = np.concatenate([quantise(F[:, :4], ql), quantise(F[:, 4:], qc)], axis=1).reshape(-1, 64)
    assert np.abs(qz).max() < 2 ** 15
    return qz[:, ZIGZAG].astype(np.int16)


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out, self.stuffed = 0, 0, bytearray(), 0

    def put(self, code, length):
        assert 0 <= code < (1 << length)
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            self._byte((self.acc >> self.n) & 255)
        self.acc &= (1 << self.n) - 1

    def _byte(self, b):
        self.out.append(b)
        if b == 0xFF:
            self.out.append(0)
            self.stuffed += 1

    def pad(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def category(v):
    return int(abs(int(v))).bit_length()


def magnitude(v, size):
    v = int(v)
    return v if v >= 0 else v + (1 << size) - 1


Encoded = collections.namedtuple("Encoded", "stream coef seg_offsets state stats")
Encoded.__doc__ = """encode()'s answer: the stream (uint8), the coefficient plane (int16 [nBlocks, 64], zigzag), the segment offsets
(uint32 [nSegments + 1], within the entropy-coded data, markers counted), the sixteen words of rt_jpeg_state for a capacity that
holds the stream, and stats: dict(zrl, eob, max_ac_cat, max_dc_cat, stuffed, rst)."""


def encode_coefficients(coef, w, h, quality, interval):
    """The entropy coder alone: coefficient plane (zigzag) -> Encoded."""
    _, _, n_mcu, n_seg = geometry(w, h, interval)
    assert coef.shape == (n_mcu * 6, 64)
    stats = dict(zrl=0, eob=0, max_ac_cat=0, max_dc_cat=0, stuffed=0, rst=0)
    body, offsets = bytearray(), [0]
    for seg in range(n_seg):
        bw, pred = BitWriter(), [0, 0, 0]
        for mcu in range(seg * interval, min((seg + 1) * interval, n_mcu)):
            for k in range(6):
                comp = 0 if k < 4 else k - 3
                t = 0 if comp == 0 else 1
                blk = coef[mcu * 6 + k].astype(np.int64)
                diff = int(blk[0]) - pred[comp]
                pred[comp] = int(blk[0])
                size = category(diff)
                assert size <= 11
                stats["max_dc_cat"] = max(stats["max_dc_cat"], size)
                bw.put(*DC_CODES[t][size])
                if size:
                    bw.put(magnitude(diff, size), size)
                run = 0
                for i in range(1, 64):
                    v = int(blk[i])
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        bw.put(*AC_CODES[t][0xF0])
                        stats["zrl"] += 1
                        run -= 16
                    size = category(v)
                    assert size <= 10
                    stats["max_ac_cat"] = max(stats["max_ac_cat"], size)
                    bw.put(*AC_CODES[t][(run << 4) | size])
                    bw.put(magnitude(v, size), size)
                    run = 0
                if run:
                    bw.put(*AC_CODES[t][0x00])
                    stats["eob"] += 1
        bw.pad()
        stats["stuffed"] += bw.stuffed
        body += bw.out
        if seg != n_seg - 1:
            body += bytes([0xFF, 0xD0 + (seg & 7)])
            stats["rst"] += 1
        offsets.append(len(body))
    stream = np.concatenate([header(w, h, quality, interval), np.frombuffer(bytes(body), dtype=np.uint8),
                             np.array([0xFF, 0xD9], dtype=np.uint8)])
    state = np.zeros(16, dtype=np.uint32)
    state[:7] = [stream.size, stream.size, 0, n_seg, n_mcu, HEADER_BYTES, stats["stuffed"]]
    return Encoded(stream, coef, np.array(offsets, dtype=np.uint32), state, stats)


def encode(y, cb, cr, quality=75, interval=1):
    """Planes (uint8 [H, W], [ch, cw], [ch, cw]; row 0 = the file's top row) -> Encoded."""
    h, w = y.shape
    return encode_coefficients(coefficients(y, cb, cr, quality), w, h, quality, interval)


def split_frame(frame, w, h, fmt):
    """A flat NV12 / I420 frame of rt_display_pack_yuv -> (y, cb, cr)."""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    frame = np.asarray(frame, dtype=np.uint8).reshape(-1)
    y = frame[:w * h].reshape(h, w)
    if fmt == "nv12":
        uv = frame[w * h:].reshape(ch, cw, 2)
        return y, uv[..., 0], uv[..., 1]
    return y, frame[w * h: w * h + cw * ch].reshape(ch, cw), frame[w * h + cw * ch:].reshape(ch, cw)


def join_frame(y, cb, cr, fmt):
    """(y, cb, cr) -> the flat frame in format fmt."""
    if fmt == "nv12":
        return np.concatenate([y.reshape(-1), np.stack([cb, cr], axis=-1).reshape(-1)]).astype(np.uint8)
    return np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)]).astype(np.uint8)


# ---- inputs the tests share -----------------------------------------------------------------------------------------------------------
def content(kind, w, h, seed=0):
    """-> (y, cb, cr) of a named picture: "ramp", "noise", "checker" ((x + y) & 1, in all three planes), "black", "white"."""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = np.mgrid[0:ch, 0:cw]
    if kind == "ramp":
        return (((xx * 255) // max(w - 1, 1) + yy) % 256).astype(np.uint8), ((cx * 7 + 16) % 256).astype(np.uint8), ((cy * 5 + 200) % 256).astype(np.uint8)
    if kind == "noise":
        r = np.random.default_rng(seed)
        return tuple(r.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (ch, cw), (ch, cw)))
    if kind == "binary":                                       # noise of 0 and 255 alone: the largest AC categories
        r = np.random.default_rng(seed)
        return tuple((r.integers(0, 2, s) * 255).astype(np.uint8) for s in ((h, w), (ch, cw), (ch, cw)))
    if kind == "blocks":                                       # 8x8 blocks black and white in turn: DC differences of category 11
        return ((((xx >> 3) + (yy >> 3)) & 1) * 255).astype(np.uint8), ((((cx >> 3) + (cy >> 3)) & 1) * 255).astype(np.uint8), \
            ((((cx >> 3) + (cy >> 3) + 1) & 1) * 255).astype(np.uint8)
    if kind == "checker":
        return (((xx + yy) & 1) * 255).astype(np.uint8), (((cx + cy) & 1) * 255).astype(np.uint8), (((cx + cy + 1) & 1) * 255).astype(np.uint8)
    v = {"black": 0, "white": 255}[kind]
    return np.full((h, w), v, np.uint8), np.full((ch, cw), 128, np.uint8), np.full((ch, cw), 128, np.uint8)


def decode_planes(stream):
    """Pillow's decoder without a colour conversion -> (y, cb, cr) at full resolution (chroma upsampled by the decoder)."""
    import io

    from PIL import Image
    im = Image.open(io.BytesIO(bytes(stream)))
    im.draft("YCbCr", im.size)
    assert im.mode == "YCbCr"
    a = np.asarray(im)
    return a[..., 0], a[..., 1], a[..., 2]


def pillow_encode(y, cb, cr, quality):
    """Pillow's own encoder on the same planes (chroma replicated 2x2, 4:2:0): the fidelity yardstick."""
    import io

    from PIL import Image
    h, w = y.shape
    up = lambda p: np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)[:h, :w]
    im = Image.fromarray(np.stack([y, up(cb), up(cr)], axis=-1), mode="YCbCr")
    buf = io.BytesIO()
    im.save(buf, format="JPEG", quality=quality, subsampling=2)
    return np.frombuffer(buf.getvalue(), dtype=np.uint8)


def luma_rms(stream, y):
    got = decode_planes(stream)[0].astype(np.float64)
    assert got.shape == y.shape
    return float(np.sqrt(np.mean((got - y.astype(np.float64)) ** 2)))
