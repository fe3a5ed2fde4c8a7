// rt_jpeg.hip -- the baseline JPEG encoder's kernels (gfx950): integer DCT + quantiser, one wave per 8x8 block; the entropy coder,
// one wave per restart segment, the 64 lanes coding the 64 coefficients of a block together; the scan of the segments' sizes.
// include/rt_mi355.h defines the stream bit for bit, DESIGN.md 29 has the design and what was measured.
#include "rt_jpeg.h"

namespace {

__constant__ const RtJpegZigzag dZigzag = kJpegZigzag;
__constant__ const RtJpegCodes dDcCodes[2] = {rt_jpeg_codes(kJpegDcLuma), rt_jpeg_codes(kJpegDcChroma)};
__constant__ const RtJpegCodes dAcCodes[2] = {rt_jpeg_codes(kJpegAcLuma), rt_jpeg_codes(kJpegAcChroma)};

constexpr int kBlocksPerGroup = 4;       // transform: waves (blocks) per workgroup
constexpr int kTilePitch = 9;            // 8 + 1: the column pass reads down a column without a bank conflict

// ---- transform: lane = y * 8 + x of the samples, then v * 8 + u of the coefficients
__global__ __launch_bounds__(64 * kBlocksPerGroup) void rt_jpeg_transform(const uint8_t *__restrict__ planes, RtJpegGeom g, RtJpegTables tab,
                                                                           int16_t *__restrict__ coef) {
    __shared__ int tile[kBlocksPerGroup][2][8 * kTilePitch];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned nBlocks = g.nMcu * 6u;
    const unsigned blockRaw = blockIdx.x * kBlocksPerGroup + wave;
    const bool live = blockRaw < nBlocks;
    const unsigned block = live ? blockRaw : nBlocks - 1u;             // a spare wave of the last workgroup redoes the last block and stores nothing
    const unsigned mcu = block / 6u, k = block - mcu * 6u;
    const unsigned mx = mcu % g.mw, my = mcu / g.mw;
    const int hi = (int)(lane >> 3), lo = (int)(lane & 7u);
    int sample;
    if (k < 4u) {
        const int px = min((int)(mx * 16u + (k & 1u) * 8u) + lo, g.W - 1), py = min((int)(my * 16u + (k >> 1) * 8u) + hi, g.H - 1);
        sample = planes[g.planeOffset[0] + (size_t)py * g.planePitch[0] + (size_t)px];
    } else {
        const int c = (int)k - 3;
        const int px = min((int)(mx * 8u) + lo, g.cw - 1), py = min((int)(my * 8u) + hi, g.ch - 1);
        sample = planes[g.planeOffset[c] + (size_t)py * g.planePitch[c] + (size_t)px * (size_t)g.chromaStep];
    }
    int mRow[8], mCol[8];                                              // M[lo][.] for the row pass, M[hi][.] for the column pass
#pragma unroll
    for (int i = 0; i < 8; i++) {
        mRow[i] = tab.M[lo * 8 + i];
        mCol[i] = tab.M[hi * 8 + i];
    }
    int *f = tile[wave][0], *r = tile[wave][1];
    f[hi * kTilePitch + lo] = sample - 128;
    __syncthreads();
    int acc = 0;
#pragma unroll
    for (int x = 0; x < 8; x++) acc += mRow[x] * f[hi * kTilePitch + x];       // r[y = hi][u = lo]
    r[hi * kTilePitch + lo] = (acc + 1024) >> 11;
    __syncthreads();
    acc = 0;
#pragma unroll
    for (int y = 0; y < 8; y++) acc += mCol[y] * r[y * kTilePitch + lo];       // F[v = hi][u = lo]
    const int F = (acc + 65536) >> 17;
    const uint32_t qe = tab.q[k < 4u ? 0 : 1][lane];
    const uint32_t Q = qe >> 21, R = qe & 0x1fffffu;
    const uint32_t a = (uint32_t)(F < 0 ? -F : F);
    const int quot = (int)(((a + (Q >> 1)) * R) >> 20);
    if (live) coef[(size_t)block * 64u + dZigzag.position[lane]] = (int16_t)(F < 0 ? -quot : quot);
}

// ---- entropy coding
constexpr unsigned kWindowWords = 128;   // the wave's bit window: up to 2047 bits kept from the last flush + 1658 of a block + a deposit's two spare words
constexpr unsigned kFlushBits = 2048;    // one word per lane

// Inclusive prefix sum over the 64 lanes of a full wave in DPP steps: shifts by 1, 2, 4, 8 inside each row of 16 lanes (zeros come in
// at the row's start), then lane 15 of rows 0 and 2 into rows 1 and 3, then lane 31 into rows 2 and 3.
__device__ __forceinline__ unsigned wave_inclusive_scan(unsigned v) {
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);       // row_shr:1
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);       // row_shr:2
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);       // row_shr:4
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);       // row_shr:8
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);      // row_bcast:15 into rows 1 and 3
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);      // row_bcast:31 into rows 2 and 3
    return v;
}

// `len` (1..64) bits, the low ones of `bits`, to bit position `at` of the window (bit 0 = the top bit of word 0)
__device__ __forceinline__ void deposit(uint32_t *window, unsigned at, unsigned long long bits, unsigned len) {
    const unsigned long long top = bits << (64u - len);                // left-aligned
    const unsigned sh = at & 31u, w = at >> 5;
    const unsigned long long a = top >> sh;
    const uint32_t d0 = (uint32_t)(a >> 32), d1 = (uint32_t)a, d2 = sh ? (uint32_t)top << (32u - sh) : 0u;
    if (d0) atomicOr(&window[w], d0);
    if (d1) atomicOr(&window[w + 1], d1);
    if (d2) atomicOr(&window[w + 2], d2);
}

// The first nBytes (<= 256) bytes of the window leave it, a 0x00 behind every 0xFF: lane l takes bytes 4l .. 4l+3.  Returns the
// bytes written (wave-uniform); with EMIT false it only counts them.
template <bool EMIT>
__device__ __forceinline__ unsigned flush_bytes(const uint32_t *window, unsigned nBytes, uint8_t *dst, unsigned lane) {
    const uint32_t word = window[lane];
    const unsigned mine = nBytes > 4u * lane ? min(nBytes - 4u * lane, 4u) : 0u;
    unsigned count = 0;
#pragma unroll
    for (unsigned j = 0; j < 4u; j++) {
        const unsigned b = (word >> (24u - 8u * j)) & 255u;
        if (j < mine) count += b == 255u ? 2u : 1u;
    }
    const unsigned incl = wave_inclusive_scan(count);
    if (EMIT) {
        uint8_t *p = dst + (incl - count);
#pragma unroll
        for (unsigned j = 0; j < 4u; j++) {
            const unsigned b = (word >> (24u - 8u * j)) & 255u;
            if (j < mine) {
                *p++ = (uint8_t)b;
                if (b == 255u) *p++ = 0;
            }
        }
    }
    return (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
}

// One wave per restart segment.  EMIT false: the segment's size and stuffed bytes into segBytes / segStuffed.  EMIT true: the
// same walk again, the bytes to ecs + segOffsets[segment] (nothing when the scan found the stream larger than the output).
template <bool EMIT>
__global__ __launch_bounds__(64) void rt_jpeg_entropy(const int16_t *__restrict__ coef, unsigned nMcu, unsigned interval, unsigned nSegments,
                                                      uint32_t *__restrict__ segBytes, uint32_t *__restrict__ segStuffed,
                                                      const uint32_t *__restrict__ segOffsets, uint8_t *__restrict__ ecs,
                                                      const uint32_t *__restrict__ state) {
    __shared__ uint32_t window[kWindowWords];
    __shared__ uint32_t acCodes[2][256], dcCodes[2][16];                // the tables beside the window: a look-up per lane and block
    const unsigned lane = threadIdx.x, seg = blockIdx.x;
    if (EMIT && state[2]) return;                                      // overflow (wave-uniform): not one byte
    window[lane] = 0;
    window[lane + 64u] = 0;
#pragma unroll
    for (unsigned i = 0; i < 4u; i++) {
        acCodes[0][lane + 64u * i] = dAcCodes[0].e[lane + 64u * i];
        acCodes[1][lane + 64u * i] = dAcCodes[1].e[lane + 64u * i];
    }
    if (lane < 32u) dcCodes[lane >> 4][lane & 15u] = dDcCodes[lane >> 4].e[lane & 15u];
    uint8_t *dst = EMIT ? ecs + segOffsets[seg] : nullptr;
    const unsigned long long firstMcu = (unsigned long long)seg * interval;
    const unsigned mcuEnd = (unsigned)min(firstMcu + interval, (unsigned long long)nMcu);
    unsigned pos = 0, written = 0, dataBytes = 0;
    int pred[3] = {0, 0, 0};
    int next[6];
#pragma unroll
    for (unsigned k = 0; k < 6u; k++) next[k] = coef[((size_t)firstMcu * 6u + k) * 64u + lane];
    __syncthreads();
    for (unsigned mcu = (unsigned)firstMcu; mcu < mcuEnd; mcu++) {
        int cur[6];
#pragma unroll
        for (unsigned k = 0; k < 6u; k++) cur[k] = next[k];
        if (mcu + 1u < mcuEnd) {                                       // the next MCU's six blocks are in flight while this one is coded
#pragma unroll
            for (unsigned k = 0; k < 6u; k++) next[k] = coef[((size_t)(mcu + 1u) * 6u + k) * 64u + lane];
        }
#pragma unroll
        for (unsigned k = 0; k < 6u; k++) {
            const int c = cur[k];
            const unsigned comp = k < 4u ? 0u : k - 3u, t = comp ? 1u : 0u;
            const int dc = __builtin_amdgcn_readfirstlane(c);
            const int v = lane == 0u ? dc - pred[comp] : c;
            pred[comp] = dc;
            const unsigned mag = (unsigned)(v < 0 ? -v : v);
            const unsigned size = 32u - (unsigned)__clz((int)mag);     // the category: 0 for 0
            const unsigned extra = (unsigned)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);    // v, or v + 2^size - 1 for v < 0: the low `size` bits of v - 1
            const unsigned long long nonzero = __builtin_amdgcn_ballot_w64(lane != 0u && c != 0);
            const unsigned last = nonzero ? 63u - (unsigned)__builtin_clzll(nonzero) : 0u;
            unsigned long long bits = 0;
            unsigned len = 0;
            if (lane == 0u) {
                const uint32_t e = dcCodes[t][size];
                bits = (unsigned long long)(e & 0xffffu) << size | extra;
                len = (e >> 16) + size;
            } else if (c != 0) {
                const unsigned long long below = nonzero & ((1ull << lane) - 1ull);
                const unsigned prev = below ? 63u - (unsigned)__builtin_clzll(below) : 0u;
                const unsigned run = lane - prev - 1u;
                const uint32_t zrl = acCodes[t][0xf0], e = acCodes[t][(run & 15u) << 4 | size];
                for (unsigned i = 0; i < (run >> 4); i++) {            // at most three
                    bits = bits << (zrl >> 16) | (zrl & 0xffffu);
                    len += zrl >> 16;
                }
                bits = (bits << (e >> 16) | (e & 0xffffu)) << size | extra;
                len += (e >> 16) + size;
            }
            if (lane == last && last < 63u) {                          // zeros behind the last coefficient: EOB
                const uint32_t eob = acCodes[t][0];
                bits = bits << (eob >> 16) | (eob & 0xffffu);
                len += eob >> 16;
            }
            const unsigned incl = wave_inclusive_scan(len);
            if (len) deposit(window, pos + incl - len, bits, len);
            pos += (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
            __syncthreads();
            if (pos >= kFlushBits) {                                   // (wave-uniform) the first 64 words go, the rest moves down
                written += flush_bytes<EMIT>(window, kFlushBits / 8u, dst + written, lane);
                dataBytes += kFlushBits / 8u;
                const uint32_t upper = window[lane + 64u];
                __syncthreads();
                window[lane] = upper;
                window[lane + 64u] = 0;
                pos -= kFlushBits;
                __syncthreads();
            }
        }
    }
    const unsigned pad = (8u - (pos & 7u)) & 7u;                       // 1-bits up to the next byte
    if (pad && lane == 0u) deposit(window, pos, (1ull << pad) - 1ull, pad);
    pos += pad;
    __syncthreads();
    written += flush_bytes<EMIT>(window, pos >> 3, dst + written, lane);
    dataBytes += pos >> 3;
    const bool marker = seg + 1u != nSegments;
    if (lane == 0u) {
        if (EMIT) {
            if (marker) {
                dst[written] = 0xff;
                dst[written + 1u] = (uint8_t)(0xd0u + (seg & 7u));
            }
        } else {
            segBytes[seg] = written + (marker ? 2u : 0u);
            segStuffed[seg] = written - dataBytes;
        }
    }
}

// ---- the scan: one workgroup of 1024 lanes walks the segments' sizes, 1024 at a time
constexpr unsigned kScanLanes = 1024;

__global__ __launch_bounds__(kScanLanes) void rt_jpeg_scan(const uint32_t *__restrict__ segBytes, const uint32_t *__restrict__ segStuffed,
                                                           uint32_t *__restrict__ segOffsets, unsigned nSegments, unsigned nMcu,
                                                           unsigned long long capBytes, RtJpegHeaderImage hdr, uint8_t *__restrict__ out,
                                                           uint32_t *__restrict__ state) {
    __shared__ unsigned waveBytes[kScanLanes / 64], waveStuffed[kScanLanes / 64];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    unsigned carry = 0, stuffed = 0;                                   // the same in every lane
    for (unsigned base = 0; base < nSegments; base += kScanLanes) {    // (base is below 2^32 - 1024: nSegments <= nMcu < 2^21)
        const unsigned i = base + tid;
        const unsigned n = i < nSegments ? segBytes[i] : 0u, f = i < nSegments ? segStuffed[i] : 0u;
        const unsigned incl = wave_inclusive_scan(n), fsum = wave_inclusive_scan(f);
        if (lane == 63u) {
            waveBytes[wave] = incl;
            waveStuffed[wave] = fsum;
        }
        __syncthreads();
        unsigned before = 0, all = 0;
        for (unsigned w = 0; w < kScanLanes / 64u; w++) {
            if (w < wave) before += waveBytes[w];
            all += waveBytes[w];
            stuffed += waveStuffed[w];
        }
        if (i < nSegments) segOffsets[i] = carry + before + incl - n;
        carry += all;
        __syncthreads();
    }
    const unsigned long long needed = (unsigned long long)kJpegHeaderBytes + carry + 2ull;       // (rt_jpeg_layout: below 2^32)
    const bool overflow = needed > capBytes;
    if (tid == 0u) segOffsets[nSegments] = carry;
    if (tid < 16u) {
        const uint32_t words[7] = {overflow ? 0u : (uint32_t)needed, (uint32_t)needed, overflow ? 1u : 0u, nSegments, nMcu, kJpegHeaderBytes, stuffed};
        uint32_t w = 0;
#pragma unroll
        for (unsigned j = 0; j < 7u; j++)
            if (tid == j) w = words[j];
        state[tid] = w;
    }
    if (overflow) return;
    if (tid < kJpegHeaderBytes) out[tid] = (uint8_t)(hdr.w[tid >> 2] >> (8u * (tid & 3u)));
    if (tid == 0u) {
        out[kJpegHeaderBytes + carry] = 0xff;
        out[kJpegHeaderBytes + carry + 1u] = 0xd9;
    }
}

}  // namespace

hipError_t rt_launch_jpeg_encode(const void *planes, const RtJpegGeom &g, const RtJpegTables &tab, const RtJpegHeaderImage &hdr, void *coef,
                                 void *segOffsets, void *segBytes, void *segStuffed, void *out, size_t capBytes, void *state, hipStream_t s) {
    const unsigned nBlocks = g.nMcu * 6u;
    uint8_t *ecs = (uint8_t *)out + kJpegHeaderBytes;
    rt_jpeg_transform<<<(nBlocks + kBlocksPerGroup - 1) / kBlocksPerGroup, 64 * kBlocksPerGroup, 0, s>>>((const uint8_t *)planes, g, tab, (int16_t *)coef);
    rt_jpeg_entropy<false><<<g.nSegments, 64, 0, s>>>((const int16_t *)coef, g.nMcu, g.interval, g.nSegments, (uint32_t *)segBytes,
                                                      (uint32_t *)segStuffed, nullptr, nullptr, nullptr);
    rt_jpeg_scan<<<1, kScanLanes, 0, s>>>((const uint32_t *)segBytes, (const uint32_t *)segStuffed, (uint32_t *)segOffsets, g.nSegments, g.nMcu,
                                          (unsigned long long)capBytes, hdr, (uint8_t *)out, (uint32_t *)state);
    rt_jpeg_entropy<true><<<g.nSegments, 64, 0, s>>>((const int16_t *)coef, g.nMcu, g.interval, g.nSegments, nullptr, nullptr,
                                                     (const uint32_t *)segOffsets, ecs, (const uint32_t *)state);
    return hipGetLastError();
}
