// jpeg_encode.hip -- baseline JPEG files written on the device (resr_jpeg_encode, include/resr.h "JPEG encode"; the definition, rule by
// rule, is tests/jpeg_encode_ref.py and DESIGN "JPEG encode").  uint8 [n,h,w,3] frames in, n complete JFIF files and their lengths out.
//   jpeg_segment : one wave per restart segment (restart_interval MCUs).  Per MCU: the pixels of the MCU (edge-replicated) -> Y, Cb, Cr
//                  samples in LDS (4:2:0: a lane owns a 2x2 quad, sums R, G, B exactly and rounds the chroma once).  Per block: the two
//                  8x8 matrix passes through LDS, exact in integers (pass 1 int32, pass 2 int64); lane z computes the coefficient at
//                  zigzag position z, so the coefficients never leave registers.  Entropy coder: the nonzero mask is one ballot, a
//                  lane's zero run a count of leading zeros of the mask below it, its code comes from the (run, size) table in LDS, a
//                  wave prefix sum gives its bit offset, bits land in an LDS block buffer with atomicOr.  The finished bytes of the
//                  block are stuffed (a second prefix sum over the 0xFF count) and stored to the segment's worst-case slot of the
//                  workspace; less than a byte is carried to the next block.  The DC predictor is wave-uniform: nothing in a segment
//                  waits for anything but the previous block's bit count.
//   jpeg_scan    : one workgroup per image: the prefix sum of (segment length + 2 marker bytes) gives every segment's offset in the
//                  file and the file's length; an image that does not fit out_stride gets the negative of what it needs.
//   jpeg_copy    : one wave per segment copies it behind the header, followed by its RSTm (the last one: EOI); the wave of segment 0
//                  copies the header too.  The segments of an image that does not fit are not copied: nothing of it is written.
// Three launches per batch whatever n is; no allocation, no host read of device data: capture-safe.
#include <math.h>

#include "host_api.h"

namespace resr {
namespace {

// ---- the tables of ITU-T T.81 Annex K ----
constexpr uint8_t kJeBaseLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                     18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kJeBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                       99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// kJeZigzag[z]: the natural index (row = vertical frequency) of the z-th coefficient
constexpr uint8_t kJeZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
__constant__ uint8_t g_je_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                       35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};      // its device copy
struct JeHuffSpec {
    uint8_t bits[16];
    uint8_t vals[162];
};
constexpr JeHuffSpec kJeDcLuma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr JeHuffSpec kJeDcChroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr JeHuffSpec kJeAcLuma = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr JeHuffSpec kJeAcChroma = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// symbol -> code << 8 | length (0: the symbol has no code), the canonical assignment of Annex C.  [0]: luma, [1]: chroma.
struct JeCodes {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};
constexpr int kJeCodeWords = sizeof(JeCodes) / 4;

constexpr void je_assign(const JeHuffSpec& s, uint32_t* table) {
    uint32_t code = 0;
    int k = 0;
    for (int length = 1; length <= 16; ++length) {
        for (int i = 0; i < s.bits[length - 1]; ++i) table[s.vals[k++]] = code++ << 8 | (uint32_t)length;
        code <<= 1;
    }
}
constexpr JeCodes je_make_codes() {
    JeCodes c{};
    je_assign(kJeDcLuma, c.dc[0]);
    je_assign(kJeDcChroma, c.dc[1]);
    je_assign(kJeAcLuma, c.ac[0]);
    je_assign(kJeAcChroma, c.ac[1]);
    return c;
}
constexpr JeCodes kJeCodesHost = je_make_codes();
__constant__ JeCodes g_je_codes = je_make_codes();

// The longest a block can be.  A DC symbol of size s costs its code and s bits; an AC symbol (run, s) its code and s bits.  Every one of
// the 63 AC positions costs at most the dearest AC symbol: a ZRL (at most 11 bits) stands for 16 positions and the EOB (at most 4) for
// at least one.  Sizes: |DC difference| <= 2047 (size 11), |AC| <= 128 * 2.57 * 2.83 < 1024 (size 10).
constexpr int je_max_cost(const uint32_t* table, int n) {
    int m = 0;
    for (int i = 0; i < n; ++i)
        if (table[i] & 255) m = ((int)(table[i] & 255) + (i & 15)) > m ? (int)(table[i] & 255) + (i & 15) : m;
    return m;
}
constexpr int je_max2(int a, int b) { return a > b ? a : b; }
constexpr int kJeDcMaxBits = je_max2(je_max_cost(kJeCodesHost.dc[0], 12), je_max_cost(kJeCodesHost.dc[1], 12));      // 11 + 11 = 22 (chroma)
constexpr int kJeAcMaxBits = je_max2(je_max_cost(kJeCodesHost.ac[0], 256), je_max_cost(kJeCodesHost.ac[1], 256));    // 16 + 10 = 26
constexpr int kJeBlockMaxBits = kJeDcMaxBits + 63 * kJeAcMaxBits;                                                    // 1660
static_assert(kJeDcMaxBits == 22 && kJeAcMaxBits == 26, "the Annex K tables");
constexpr int kJeBufWords = 64;      // the block's bit buffer: 7 carried bits + a block, flushed four bytes per lane
static_assert(7 + kJeBlockMaxBits <= 8 * 4 * kJeBufWords - 64, "a block and the carry fit the bit buffer, with room for the second word of the last put");
constexpr int kJeHeaderBytes = 2 + 18 + (4 + 2 * 65) + 19 + (4 + 2 * 29 + 2 * 179) + 6 + 14;      // SOI APP0 DQT SOF0 DHT DRI SOS = 613
static_assert(kJeHeaderBytes == RESR_JPEG_HEADER_BYTES, "the header's length as include/resr.h states it");
constexpr int kJeCopyWaves = 4;

struct JeParams {
    int32_t dct[64];         // C[u][x], Q20
    uint16_t step[2][64];    // luma, chroma; ZIGZAG order
};

struct JePlan {
    int interval, blocks, mcu, mcus_x, mcus, nseg;
    int64_t seg_cap;         // bytes of a segment's slot in the workspace: no segment is longer
    int64_t segs;            // n * nseg
    size_t off_bytes, data_bytes, bytes;      // workspace: [seg_len int32 x segs | pad to 8][seg_off int64 x segs][segs x seg_cap]
};

__device__ __forceinline__ int je_scan_incl(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// `len` bits (1 .. 32, value below 2^len) at bit `off` of the MSB-first buffer
__device__ __forceinline__ void je_put(uint32_t* buf, int off, uint32_t value, int len) {
    const int pos = off & 31;
    const unsigned long long t = (unsigned long long)value << (64 - pos - len);
    atomicOr(&buf[off >> 5], (uint32_t)(t >> 32));
    if ((uint32_t)t) atomicOr(&buf[(off >> 5) + 1], (uint32_t)t);
}

__device__ __forceinline__ int je_size(int a) { return a ? 32 - __clz(a) : 0; }

__global__ __launch_bounds__(64) void jpeg_segment_kernel(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ seg_data, int* __restrict__ seg_len, const JeParams P, int H, int W,
                                                          int mcus_x, int mcus, int nseg, int interval, int sub420, long long seg_cap) {
    __shared__ uint32_t codes[kJeCodeWords];
    __shared__ int cmat[64];
    __shared__ int samp[6][64];
    __shared__ int tmp[64];
    __shared__ uint32_t bitbuf[kJeBufWords];
    const int lane = threadIdx.x;
    const long long g = blockIdx.x;
    const int img = (int)(g / nseg), seg = (int)(g % nseg);
    const uint8_t* __restrict__ src = rgb + (size_t)img * (size_t)H * (size_t)W * 3;
    uint8_t* __restrict__ dst = seg_data + (size_t)g * (size_t)seg_cap;

    for (int i = lane; i < kJeCodeWords; i += 64) codes[i] = ((const uint32_t*)&g_je_codes)[i];
    cmat[lane] = P.dct[lane];
    bitbuf[lane] = 0;
    const uint32_t* dc_codes = codes;             // [2][16]
    const uint32_t* ac_codes = codes + 32;        // [2][256]
    const int nat = g_je_zigzag[lane], fu = nat >> 3, fv = nat & 7;
    const int step_l = P.step[0][lane], step_c = P.step[1][lane];
    const int nb = sub420 ? 6 : 3;
    int pred0 = 0, pred1 = 0, pred2 = 0;
    int carry = 0;               // bits of the unfinished byte at the head of bitbuf
    long long written = 0;       // bytes of the segment stored so far
    __syncthreads();

    const int m_end = min((seg + 1) * interval, mcus);
    for (int m = seg * interval; m < m_end; ++m) {
        const int my = m / mcus_x, mx = m - my * mcus_x;
        if (sub420) {
            const int cy = lane >> 3, cx = lane & 7;
            int sr = 0, sg = 0, sb = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int yy = 2 * cy + (q >> 1), xx = 2 * cx + (q & 1);
                const int py = min(my * 16 + yy, H - 1), px = min(mx * 16 + xx, W - 1);
                const uint8_t* p = src + ((size_t)py * (size_t)W + (size_t)px) * 3;
                const int r = p[0], gg = p[1], b = p[2];
                sr += r, sg += gg, sb += b;
                samp[(yy >> 3) * 2 + (xx >> 3)][(yy & 7) * 8 + (xx & 7)] = ((19595 * r + 38470 * gg + 7471 * b + 32768) >> 16) - 128;
            }
            samp[4][lane] = ((-11059 * sr - 21709 * sg + 32768 * sb + (128 << 18) + 131071) >> 18) - 128;
            samp[5][lane] = ((32768 * sr - 27439 * sg - 5329 * sb + (128 << 18) + 131071) >> 18) - 128;
        } else {
            const int py = min(my * 8 + (lane >> 3), H - 1), px = min(mx * 8 + (lane & 7), W - 1);
            const uint8_t* p = src + ((size_t)py * (size_t)W + (size_t)px) * 3;
            const int r = p[0], gg = p[1], b = p[2];
            samp[0][lane] = ((19595 * r + 38470 * gg + 7471 * b + 32768) >> 16) - 128;
            samp[1][lane] = ((-11059 * r - 21709 * gg + 32768 * b + (128 << 16) + 32767) >> 16) - 128;
            samp[2][lane] = ((32768 * r - 27439 * gg - 5329 * b + (128 << 16) + 32767) >> 16) - 128;
        }
        __syncthreads();

        for (int b = 0; b < nb; ++b) {
            const int comp = b < nb - 2 ? 0 : b - (nb - 2) + 1, ti = comp ? 1 : 0;
            {   // pass 1: T[u][x] = sum_y C[u][y] s[y][x]
                const int u = lane >> 3, x = lane & 7;
                int t = 0;
#pragma unroll
                for (int y = 0; y < 8; ++y) t += cmat[u * 8 + y] * samp[b][y * 8 + x];
                tmp[lane] = t;
            }
            __syncthreads();
            long long F = 0;   // pass 2: F[u][v] = sum_x C[v][x] T[u][x], at this lane's zigzag position
#pragma unroll
            for (int x = 0; x < 8; ++x) F += (long long)cmat[fv * 8 + x] * (long long)tmp[fu * 8 + x];
            const int G = (int)((F + (1LL << 26)) >> 27);
            const unsigned step = (unsigned)(ti ? step_c : step_l);
            const int mag = (int)(((unsigned)abs(G) + (step << 12)) / (step << 13));
            const int q = G < 0 ? -mag : mag;

            // entropy: this lane's bits
            const int dcq = __shfl(q, 0, 64);
            const int pred = comp == 0 ? pred0 : comp == 1 ? pred1 : pred2;
            if (comp == 0) pred0 = dcq; else if (comp == 1) pred1 = dcq; else pred2 = dcq;
            const unsigned long long mask = __ballot(q != 0) & ~1ULL;
            const uint32_t zrl = ac_codes[ti * 256 + 0xF0];
            uint32_t value = 0;
            int nbits = 0, nzrl = 0;
            if (lane == 0) {
                const int diff = q - pred, size = je_size(abs(diff));
                const uint32_t e = dc_codes[ti * 16 + size];
                value = (e >> 8) << size | ((uint32_t)(diff > 0 ? diff : diff - 1) & ((1u << size) - 1));
                nbits = (int)(e & 255) + size;
            } else if (q != 0) {
                const unsigned long long below = mask & ((1ULL << lane) - 1);
                const int last = below ? 63 - __clzll((long long)below) : 0;
                const int run = lane - 1 - last, size = je_size(abs(q));
                nzrl = run >> 4;
                const uint32_t e = ac_codes[ti * 256 + ((run & 15) << 4 | size)];
                value = (e >> 8) << size | ((uint32_t)(q > 0 ? q : q - 1) & ((1u << size) - 1));
                nbits = (int)(e & 255) + size;
            } else if (lane == 63) {      // the block does not end in a coefficient: EOB
                const uint32_t e = ac_codes[ti * 256];
                value = e >> 8;
                nbits = (int)(e & 255);
            }
            const int mine = nzrl * (int)(zrl & 255) + nbits;
            const int incl = je_scan_incl(mine, lane);
            int off = carry + incl - mine;
            for (int i = 0; i < nzrl; ++i) {
                je_put(bitbuf, off, zrl >> 8, (int)(zrl & 255));
                off += (int)(zrl & 255);
            }
            if (nbits) je_put(bitbuf, off, value, nbits);
            const int total = carry + __shfl(incl, 63, 64);
            __syncthreads();

            // flush the finished bytes, four per lane, a zero byte behind every 0xFF
            const int nbytes = total >> 3;
            const uint32_t word = bitbuf[lane];
            const uint32_t part = (bitbuf[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 255;
            int count = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (4 * lane + i < nbytes) count += 1 + (((word >> (24 - 8 * i)) & 255) == 255);
            const int cincl = je_scan_incl(count, lane);
            uint8_t* o = dst + written + (cincl - count);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (4 * lane + i < nbytes) {
                    const uint32_t byte = (word >> (24 - 8 * i)) & 255;
                    *o++ = (uint8_t)byte;
                    if (byte == 255) *o++ = 0;
                }
            written += __shfl(cincl, 63, 64);
            carry = total & 7;
            __syncthreads();
            bitbuf[lane] = lane == 0 ? part << 24 : 0;
            __syncthreads();
        }
    }
    if (lane == 0) {
        if (carry) {             // the last byte of the segment, padded with 1-bits
            const uint32_t byte = (bitbuf[0] >> 24) | ((1u << (8 - carry)) - 1);
            dst[written++] = (uint8_t)byte;
            if (byte == 255) dst[written++] = 0;
        }
        seg_len[g] = (int)written;
    }
}

__global__ __launch_bounds__(256) void jpeg_scan_kernel(const int* __restrict__ seg_len, long long* __restrict__ seg_off, int nseg, int header_len, long long out_stride,
                                                        long long* __restrict__ lengths) {
    __shared__ long long wave_sum[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long base = (long long)blockIdx.x * nseg;
    long long running = header_len;
    for (int first = 0; first < nseg; first += 256) {
        const int i = first + t;
        const long long v = i < nseg ? (long long)seg_len[base + i] + 2 : 0;      // the segment and its RSTm (the last one: EOI)
        long long s = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long u = __shfl_up(s, d, 64);
            if (lane >= d) s += u;
        }
        if (lane == 63) wave_sum[wave] = s;
        __syncthreads();
        long long before = 0, all = 0;
        for (int k = 0; k < 4; ++k) {
            if (k < wave) before += wave_sum[k];
            all += wave_sum[k];
        }
        if (i < nseg) seg_off[base + i] = running + before + s - v;
        running += all;
        __syncthreads();
    }
    if (t == 0) lengths[blockIdx.x] = running <= out_stride ? running : -running;
}

__global__ __launch_bounds__(64 * kJeCopyWaves) void jpeg_copy_kernel(const uint8_t* __restrict__ seg_data, const int* __restrict__ seg_len, const long long* __restrict__ seg_off,
                                                                     const long long* __restrict__ lengths, const uint8_t* __restrict__ header, int header_len,
                                                                     uint8_t* __restrict__ out, long long out_stride, int nseg, long long segs, long long seg_cap) {
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * kJeCopyWaves + (threadIdx.x >> 6);
    if (g >= segs) return;
    const long long img = g / nseg;
    const int seg = (int)(g - img * nseg);
    if (lengths[img] < 0) return;      // the file does not fit its slot: not a byte of it is written
    uint8_t* __restrict__ file = out + (size_t)img * (size_t)out_stride;
    if (seg == 0)
        for (int i = lane; i < header_len; i += 64) file[i] = header[i];
    const uint8_t* __restrict__ s = seg_data + (size_t)g * (size_t)seg_cap;
    uint8_t* __restrict__ d = file + seg_off[g];
    const int len = seg_len[g];
    for (int i = lane; i < len; i += 64) d[i] = s[i];
    if (lane == 0) {
        d[len] = 0xFF;
        d[len + 1] = (uint8_t)(seg == nseg - 1 ? 0xD9 : 0xD0 + (seg & 7));
    }
}

bool je_plan(const ResrJpegEncDesc* d, JePlan* p) {
    if (!d) return fail(RESR_ERR_ARG, "jpeg_encode: null descriptor"), false;
    if (d->n < 1 || d->h < 1 || d->w < 1 || d->h > 65535 || d->w > 65535)
        return fail(RESR_ERR_ARG, "jpeg_encode: bad geometry (n=%d, frames %dx%d: n at least 1, h and w in 1..65535, the SOF0 fields)", d->n, d->h, d->w), false;
    if (d->quality < 1 || d->quality > 100) return fail(RESR_ERR_ARG, "jpeg_encode: quality %d is outside 1..100", d->quality), false;
    if (d->subsampling != RESR_JPEG_444 && d->subsampling != RESR_JPEG_420)
        return fail(RESR_ERR_ARG, "jpeg_encode: unknown subsampling %d (RESR_JPEG_444 or RESR_JPEG_420)", d->subsampling), false;
    if (d->restart_interval < 0 || d->restart_interval > 65535)
        return fail(RESR_ERR_ARG, "jpeg_encode: restart interval %d is outside 0..65535 (0 = the default, %d)", d->restart_interval, RESR_JPEG_DEFAULT_INTERVAL), false;
    p->interval = d->restart_interval ? d->restart_interval : RESR_JPEG_DEFAULT_INTERVAL;
    p->mcu = d->subsampling == RESR_JPEG_420 ? 16 : 8;
    p->blocks = d->subsampling == RESR_JPEG_420 ? 6 : 3;
    p->mcus_x = (d->w + p->mcu - 1) / p->mcu;
    p->mcus = p->mcus_x * ((d->h + p->mcu - 1) / p->mcu);      // at most 8192 * 8192
    p->nseg = (p->mcus + p->interval - 1) / p->interval;
    p->segs = (int64_t)d->n * p->nseg;
    if (p->segs > 0x7fffffffLL) return fail(RESR_ERR_ARG, "jpeg_encode: %d frames of %d segments do not fit the grid of a launch", d->n, p->nseg), false;
    // a segment before stuffing is at most ceil(blocks * kJeBlockMaxBits / 8) bytes, its padded last byte included; stuffing at most doubles it
    const int64_t seg_blocks = (int64_t)(p->interval < p->mcus ? p->interval : p->mcus) * p->blocks;
    p->seg_cap = (2 * ((seg_blocks * kJeBlockMaxBits + 7) / 8) + 15) / 16 * 16;
    p->off_bytes = ((size_t)p->segs * 4 + 7) / 8 * 8;
    p->data_bytes = p->off_bytes + (size_t)p->segs * 8;
    p->bytes = p->data_bytes + (size_t)p->segs * (size_t)p->seg_cap;
    return true;
}

void je_steps(int quality, int chroma, uint8_t* natural) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const int s = ((chroma ? kJeBaseChroma[i] : kJeBaseLuma[i]) * scale + 50) / 100;
        natural[i] = (uint8_t)(s < 1 ? 1 : s > 255 ? 255 : s);
    }
}

struct JeWriter {
    uint8_t* p;
    void byte(int v) { *p++ = (uint8_t)v; }
    void word(int v) { byte(v >> 8), byte(v & 255); }
    void marker(int m, int payload) { byte(0xFF), byte(m), word(payload + 2); }
};
}  // namespace

// no file of this geometry is longer: the header, and per segment its worst case (je_plan) and two marker bytes
size_t jpeg_encode_max_bytes(const ResrJpegEncDesc* d) {
    JePlan p;
    return je_plan(d, &p) ? (size_t)kJeHeaderBytes + (size_t)p.nseg * (size_t)(p.seg_cap + 2) : 0;
}

size_t jpeg_encode_workspace_bytes(const ResrJpegEncDesc* d) {
    JePlan p;
    return je_plan(d, &p) ? p.bytes : 0;
}

int jpeg_encode_header(const ResrJpegEncDesc* d, uint8_t* host_buf, size_t cap) {
    JePlan p;
    if (!je_plan(d, &p)) return RESR_ERR_ARG;
    if (!host_buf) return kJeHeaderBytes;
    if (cap < (size_t)kJeHeaderBytes) return fail(RESR_ERR_ARG, "jpeg_encode_header: a buffer of %zu bytes, %d needed", cap, kJeHeaderBytes);
    JeWriter w{host_buf};
    w.byte(0xFF), w.byte(0xD8);
    w.marker(0xE0, 14);
    for (int v : {0x4A, 0x46, 0x49, 0x46, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0}) w.byte(v);      // "JFIF" 0, version 1.01, no units, density 1:1, no thumbnail
    w.marker(0xDB, 2 * 65);
    for (int t = 0; t < 2; ++t) {
        uint8_t steps[64];
        je_steps(d->quality, t, steps);
        w.byte(t);
        for (int z = 0; z < 64; ++z) w.byte(steps[kJeZigzag[z]]);
    }
    w.marker(0xC0, 15);
    w.byte(8), w.word(d->h), w.word(d->w), w.byte(3);
    w.byte(1), w.byte(d->subsampling == RESR_JPEG_420 ? 0x22 : 0x11), w.byte(0);
    w.byte(2), w.byte(0x11), w.byte(1);
    w.byte(3), w.byte(0x11), w.byte(1);
    w.marker(0xC4, 2 * 29 + 2 * 179);
    const JeHuffSpec* specs[4] = {&kJeDcLuma, &kJeAcLuma, &kJeDcChroma, &kJeAcChroma};
    const int ids[4] = {0x00, 0x10, 0x01, 0x11};
    for (int t = 0; t < 4; ++t) {
        int count = 0;
        w.byte(ids[t]);
        for (int i = 0; i < 16; ++i) w.byte(specs[t]->bits[i]), count += specs[t]->bits[i];
        for (int i = 0; i < count; ++i) w.byte(specs[t]->vals[i]);
    }
    w.marker(0xDD, 2);
    w.word(p.interval);
    w.marker(0xDA, 10);
    for (int v : {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0}) w.byte(v);
    if (w.p - host_buf != kJeHeaderBytes) return fail(RESR_ERR_ARG, "jpeg_encode_header: wrote %d bytes, not %d", (int)(w.p - host_buf), kJeHeaderBytes);
    return kJeHeaderBytes;
}

int jpeg_encode_dispatch(const ResrJpegEncDesc* d, const uint8_t* rgb, uint8_t* out, int64_t out_stride, int64_t* lengths, const uint8_t* header_dev, int header_len, void* workspace,
                         size_t workspace_bytes, hipStream_t st) {
    JePlan p;
    if (!je_plan(d, &p)) return RESR_ERR_ARG;
    if (!rgb || !out || !lengths || !header_dev || !workspace) return fail(RESR_ERR_ARG, "jpeg_encode: null pointer");
    if (out_stride < 0) return fail(RESR_ERR_ARG, "jpeg_encode: out_stride %lld is negative", (long long)out_stride);
    if (header_len != kJeHeaderBytes) return fail(RESR_ERR_ARG, "jpeg_encode: a header of %d bytes, this descriptor's has %d (resr_jpeg_encode_header)", header_len, kJeHeaderBytes);
    if (((uintptr_t)workspace | (uintptr_t)lengths) & 7) return fail(RESR_ERR_ARG, "jpeg_encode: the workspace and lengths must be 8-byte aligned");
    if (workspace_bytes < p.bytes) return fail(RESR_ERR_ARG, "jpeg_encode: workspace of %zu bytes, %zu needed", workspace_bytes, p.bytes);

    static JeParams params_dct;      // the Q20 matrix, by the host's libm, once
    static const bool dct_made = [] {
        for (int u = 0; u < 8; ++u)
            for (int x = 0; x < 8; ++x) params_dct.dct[u * 8 + x] = (int32_t)nearbyint(0.5 * (u == 0 ? 1.0 / sqrt(2.0) : 1.0) * cos((2 * x + 1) * u * M_PI / 16) * 1048576.0);
        return true;
    }();
    (void)dct_made;
    JeParams P = params_dct;
    for (int t = 0; t < 2; ++t) {
        uint8_t steps[64];
        je_steps(d->quality, t, steps);
        for (int z = 0; z < 64; ++z) P.step[t][z] = steps[kJeZigzag[z]];
    }
    int* seg_len = (int*)workspace;
    long long* seg_off = (long long*)((uint8_t*)workspace + p.off_bytes);
    uint8_t* seg_data = (uint8_t*)workspace + p.data_bytes;
    const double px = (double)d->n * d->h * d->w;
    prof_before(st);
    hipLaunchKernelGGL(jpeg_segment_kernel, dim3((unsigned)p.segs), dim3(64), 0, st, rgb, seg_data, seg_len, P, d->h, d->w, p.mcus_x, p.mcus, p.nseg, p.interval,
                       d->subsampling == RESR_JPEG_420 ? 1 : 0, (long long)p.seg_cap);
    prof_after(st, 35000 + (d->subsampling == RESR_JPEG_420 ? 1 : 0), px * (d->subsampling == RESR_JPEG_420 ? 1.5 : 3.0) * 32.0, px * 3.0);
    RESR_CHECK_LAUNCH("jpeg_segment_kernel");
    prof_before(st);
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3((unsigned)d->n), dim3(256), 0, st, (const int*)seg_len, seg_off, p.nseg, header_len, (long long)out_stride, (long long*)lengths);
    prof_after(st, 35100, 0.0, (double)p.segs * 12.0);
    RESR_CHECK_LAUNCH("jpeg_scan_kernel");
    prof_before(st);
    hipLaunchKernelGGL(jpeg_copy_kernel, dim3((unsigned)((p.segs + kJeCopyWaves - 1) / kJeCopyWaves)), dim3(64 * kJeCopyWaves), 0, st, (const uint8_t*)seg_data, (const int*)seg_len,
                       (const long long*)seg_off, (const long long*)lengths, header_dev, header_len, out, (long long)out_stride, p.nseg, (long long)p.segs, (long long)p.seg_cap);
    prof_after(st, 35200, 0.0, 0.0);
    RESR_CHECK_LAUNCH("jpeg_copy_kernel");
    return RESR_OK;
}

}  // namespace resr
