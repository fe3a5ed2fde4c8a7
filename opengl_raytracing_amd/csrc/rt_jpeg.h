// rt_jpeg.h -- the baseline JPEG encoder's tables, kernel arguments and launch wrappers: what rt_jpeg.hip implements for the entry
// points in rt_jpeg.cpp (include/rt_mi355.h has the stream's definition, DESIGN.md 29 the design).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

constexpr unsigned kJpegHeaderBytes = 629;
constexpr unsigned kJpegMcuWorstBytes = 2488;       // 6 blocks of at most 20 + 63 * 26 bits, every byte stuffed

// ---- Annex K of ITU-T T.81: the quantisers in natural order, the Huffman tables as BITS (codes of length 1..16) and HUFFVAL
constexpr uint8_t kJpegQuantLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                        69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                                        81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99};
constexpr uint8_t kJpegQuantChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                          99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                          99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
struct RtJpegHuffSpec {
    uint8_t bits[16];
    uint8_t vals[162];
    int n;
};
constexpr RtJpegHuffSpec kJpegDcLuma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr RtJpegHuffSpec kJpegDcChroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr RtJpegHuffSpec kJpegAcLuma = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    162};
constexpr RtJpegHuffSpec kJpegAcChroma = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    162};

// natural index of zigzag position k, and its inverse
struct RtJpegZigzag {
    uint8_t order[64], position[64];
};
constexpr RtJpegZigzag rt_jpeg_zigzag() {
    RtJpegZigzag z{};
    int k = 0;
    for (int s = 0; s < 15; s++)
        for (int i = 0; i < 8; i++) {
            const int v = (s & 1) ? i : 7 - i, u = s - v;        // odd anti-diagonals walk down, even ones up
            if (u < 0 || u > 7) continue;
            z.order[k] = (uint8_t)(v * 8 + u);
            z.position[v * 8 + u] = (uint8_t)k;
            k++;
        }
    return z;
}
constexpr RtJpegZigzag kJpegZigzag = rt_jpeg_zigzag();
static_assert(kJpegZigzag.order[1] == 1 && kJpegZigzag.order[2] == 8 && kJpegZigzag.order[3] == 16 && kJpegZigzag.order[63] == 63 &&
                  kJpegZigzag.order[62] == 62 && kJpegZigzag.order[61] == 55,
              "Figure A.6");

// the codes of a table by Annex C: e[symbol] = length << 16 | code, 0 where the symbol has none
struct RtJpegCodes {
    uint32_t e[256];
};
constexpr RtJpegCodes rt_jpeg_codes(const RtJpegHuffSpec &h) {
    RtJpegCodes t{};
    unsigned code = 0;
    int k = 0;
    for (unsigned len = 1; len <= 16; len++) {
        for (int i = 0; i < h.bits[len - 1]; i++) t.e[h.vals[k++]] = len << 16 | code++;
        code <<= 1;
    }
    return t;
}

// ---- what the kernels take
// The transform's tables, built on the host: M[u * 8 + x] of rt_jpeg_dct_matrix; q[table][natural index] = Q << 21 | R with
// R = floor(2^20 / Q) + 1, so that (n * R) >> 20 == n / Q for every n < 2^11 (n * (R * Q - 2^20) <= 2047 * 255 < 2^20; n * R < 2^32)
struct RtJpegTables {
    int32_t M[64];
    uint32_t q[2][64];
};
struct RtJpegHeaderImage {
    uint32_t w[(kJpegHeaderBytes + 3) / 4];      // the header's bytes, little-endian in each word
};
// Where the planes lie (rt_display_yuv_layout) and how the frame divides
struct RtJpegGeom {
    int W, H, cw, ch;
    unsigned mw, nMcu, nSegments, interval;
    size_t planeOffset[3], planePitch[3];
    int chromaStep;                              // bytes from one Cb (Cr) sample to the next: 2 for NV12, 1 for I420
};

// The four launches of one encode on s: transform (planes -> coefficient plane), count (each segment's bytes), scan (segment
// offsets, the state record, and -- unless the stream overflows capBytes -- the header and EOI), emit (the entropy-coded data).
// segBytes / segStuffed: nSegments uint32 each, the private region of rt_jpeg_layout.
hipError_t rt_launch_jpeg_encode(const void *planes, const RtJpegGeom &g, const RtJpegTables &tab, const RtJpegHeaderImage &hdr, void *coef,
                                 void *segOffsets, void *segBytes, void *segStuffed, void *out, size_t capBytes, void *state, hipStream_t s);
