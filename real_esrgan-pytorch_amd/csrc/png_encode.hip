// png_encode.hip -- PNG files written on the device (resr_png_encode, include/resr.h "PNG encode"; the definition, rule by rule, is
// tests/png_encode_ref.py and DESIGN "PNG encode").  uint8 / uint16 [n,h,w,c] images in, n complete files and their lengths out.
//   png_filter  : one wave per row: the five filter costs (sum of |int8|), lanes strided over the row, one reduction; the type byte
//                 of the row into the workspace.
//   png_segment : one wave per segment of the filtered stream F (segment_bytes of it).  The bytes of F are computed on the fly from the
//                 image and the rows' type bytes (left and up neighbours come from the image; 16-bit samples are byte-swapped).
//                 Pass 1: tokens (literals and distance-1 matches; a lane owns a position, run starts by ballot, the token is emitted
//                 by the lane at its LAST byte, so nothing looks further ahead than one byte), their histogram in LDS, the Adler
//                 partials.  Then the literal/length code, the code-length tokens and their code (pe_build_code: a rank sort over the
//                 wave, the two-queue merge and the repair in lane 0), the bit count and the stored / dynamic decision.  Pass 2: the
//                 same walk, codes through a wave prefix sum into an LDS bit buffer (LSB first), whole words to the segment's slot.
//                 Last: the CRC-32 of "IDAT" + the segment's bytes, a slice per lane, combined with x^(8L) mod P operators.
//   png_scan    : one workgroup per frame: chunk offsets (prefix sum), the Adler-32 of F from the partials, the file's length or, if
//                 it does not fit out_stride, its negative.
//   png_copy    : one wave per segment: length, "IDAT", bytes, CRC; the wave of segment 0 the header, the last one the Adler chunk and
//                 IEND.  A frame that does not fit is not touched.
// Four launches per batch whatever n is; no allocation, no host read of device data: capture-safe.  Plain C++ and vector stores only.
#include "host_api.h"

namespace resr {
namespace {

constexpr int kPeHeaderBytes = 47;
static_assert(kPeHeaderBytes == RESR_PNG_HEADER_BYTES, "the header's length as include/resr.h states it");
constexpr int kPeLitSyms = 286, kPeClSyms = 19, kPeLitLimit = 15, kPeClLimit = 7;
constexpr int kPeSymCap = 288;           // the arrays of a code: 286 symbols and the slot of the distance code behind them
constexpr int kPeBufWords = 68;          // the bit buffer: 31 carried bits + 63 lanes x 30 bits = 1921 bits = 61 words
constexpr int kPeCopyWaves = 4;
constexpr uint32_t kPePoly = 0xEDB88320u;

// ---- CRC-32 on the host and at compile time (the header; the constants of the device's combine) ----
constexpr uint32_t pe_crc_step(uint32_t crc, uint8_t byte) {
    crc ^= byte;
    for (int k = 0; k < 8; ++k) crc = crc & 1 ? kPePoly ^ (crc >> 1) : crc >> 1;
    return crc;
}
constexpr uint32_t pe_crc_raw(uint32_t crc, const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; ++i) crc = pe_crc_step(crc, p[i]);
    return crc;
}
constexpr uint8_t kPeIdat[4] = {'I', 'D', 'A', 'T'};
constexpr uint32_t kPeIdatState = pe_crc_raw(0xFFFFFFFFu, kPeIdat, 4);      // the register behind "IDAT", where a chunk's data starts

// a(x) b(x) mod P in the reflected representation (bit 31 = x^0)
__host__ __device__ constexpr uint32_t pe_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = b & 1 ? (b >> 1) ^ kPePoly : b >> 1;
    }
    return p;
}
struct PeX2n {
    uint32_t v[32];          // x^(2^k) mod P
};
constexpr PeX2n pe_make_x2n() {
    PeX2n t{};
    uint32_t p = 0x40000000u;          // x^1
    t.v[0] = p;
    for (int k = 1; k < 32; ++k) t.v[k] = p = pe_mulmod(p, p);
    return t;
}
__constant__ PeX2n g_pe_x2n = pe_make_x2n();
__constant__ uint8_t g_pe_cl_order[kPeClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct PePlan {
    int bpp, swap, S;
    uint32_t rb, rowlen;     // bytes of a row of samples; of a row of F (1 + rb)
    int64_t T;               // bytes of F of one frame
    int nseg;                // per frame
    int64_t segs, rows;      // n * nseg, n * h
    int64_t slot;            // bytes of a segment's slot in the workspace
    // workspace: [seg_len int32 x segs][seg_off int64 x segs][seg_crc uint32 x segs][seg_adler uint32 x 2 segs][frame uint32 x 2 n]
    //            [row type uint8 x rows][segs slots], every part padded to 16 bytes
    size_t off_off, crc_off, adler_off, frame_off, type_off, data_off, bytes;
};

// what the kernels need to compute a byte of F
struct PeSource {
    const uint8_t* base;     // the frame's samples (raw != 0: the frame's stream itself)
    const uint8_t* types;    // the frame's row type bytes
    uint32_t rb, rowlen;
    int bpp, swap, raw;
};

__device__ __forceinline__ int pe_paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int pe_filtered(int type, int x, int a, int b, int c) {
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : pe_paeth(a, b, c);
    return (x - pred) & 255;
}

// F[row][col] of the frame: col 0 is the row's type byte
__device__ __forceinline__ int pe_stream_byte(const PeSource& s, long long row, uint32_t col) {
    if (s.raw) return s.base[(size_t)row * s.rowlen + col];
    const int type = s.types[row];
    if (col == 0) return type;
    const uint32_t j = col - 1;
    const uint8_t* __restrict__ cur = s.base + (size_t)row * s.rb;
    const bool left = j >= (uint32_t)s.bpp, up = row > 0;
    const int x = cur[j ^ s.swap];
    const int a = left ? cur[(j - s.bpp) ^ s.swap] : 0;
    const int b = up ? (cur - s.rb)[j ^ s.swap] : 0;
    const int c = (left && up) ? (cur - s.rb)[(j - s.bpp) ^ s.swap] : 0;
    return pe_filtered(type, x, a, b, c);
}

__device__ __forceinline__ int pe_scan_incl(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

__device__ __forceinline__ int pe_wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ unsigned long long pe_wave_sum64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// ---- png_filter ----
__global__ __launch_bounds__(64) void png_filter_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ types, int h, uint32_t rb, int bpp, int swap) {
    const int lane = threadIdx.x;
    const long long g = blockIdx.x;
    const bool up = (g % h) != 0;
    const uint8_t* __restrict__ cur = src + (size_t)g * rb;
    const uint8_t* __restrict__ above = cur - rb;          // read only where `up`
    unsigned long long cost[5] = {0, 0, 0, 0, 0};
    for (uint32_t j = lane; j < rb; j += 64) {
        const bool left = j >= (uint32_t)bpp;
        const int x = cur[j ^ swap];
        const int a = left ? cur[(j - bpp) ^ swap] : 0;
        const int b = up ? above[j ^ swap] : 0;
        const int c = (left && up) ? above[(j - bpp) ^ swap] : 0;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const int v = pe_filtered(t, x, a, b, c);
            cost[t] += (unsigned)(v < 128 ? v : 256 - v);
        }
    }
    int best = 0;
    unsigned long long least = 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const unsigned long long total = pe_wave_sum64(cost[t]);
        if (t == 0 || total < least) least = total, best = t;      // ties to the lowest type
    }
    if (lane == 0) types[g] = (uint8_t)best;
}

// ---- the length-limited code ----
struct PeCodeScratch {
    uint16_t sorted[kPeSymCap];          // the used symbols, ascending by (count, symbol)
    uint32_t weight[kPeSymCap];          // their counts
    uint32_t node_weight[kPeSymCap];
    uint16_t leaf_parent[kPeSymCap], node_parent[kPeSymCap], node_depth[kPeSymCap];
    int per_length[16], next_code[16];
};

// counts[nsym] -> lengths[nsym] (tests/png_encode_ref.py build_lengths).  The sum of the counts must stay below 2^32.  The whole wave calls.
__device__ void pe_build_code(const uint32_t* counts, int nsym, int limit, uint8_t* lengths, PeCodeScratch& s, int lane) {
    int mine = 0;
    for (int a = lane; a < nsym; a += 64) {
        const uint32_t ca = counts[a];
        lengths[a] = 0;
        if (!ca) continue;
        ++mine;
        int rank = 0;
        for (int b = 0; b < nsym; ++b) {
            const uint32_t cb = counts[b];
            rank += (cb != 0) & ((cb < ca) | ((cb == ca) & (b < a)));
        }
        s.sorted[rank] = (uint16_t)a;
        s.weight[rank] = ca;
    }
    const int n = pe_wave_sum(mine);
    __syncthreads();
    if (lane == 0) {
        if (n == 1) lengths[s.sorted[0]] = 1;
        if (n >= 2) {
            int li = 0, ni = 0;
            for (int k = 0; k < n - 1; ++k) {          // two queues; of a leaf and a node of equal weight the leaf goes first
                uint32_t total = 0;
                for (int r = 0; r < 2; ++r) {
                    if (li < n && (ni >= k || s.weight[li] <= s.node_weight[ni])) {
                        total += s.weight[li];
                        s.leaf_parent[li++] = (uint16_t)k;
                    } else {
                        total += s.node_weight[ni];
                        s.node_parent[ni++] = (uint16_t)k;
                    }
                }
                s.node_weight[k] = total;
            }
            s.node_depth[n - 2] = 0;
            for (int j = n - 3; j >= 0; --j) s.node_depth[j] = (uint16_t)(s.node_depth[s.node_parent[j]] + 1);
            for (int i = 0; i <= limit; ++i) s.per_length[i] = 0;
            for (int i = 0; i < n; ++i) {
                const int d = s.node_depth[s.leaf_parent[i]] + 1;
                s.per_length[d < limit ? d : limit] += 1;
            }
            int total = 0;
            for (int i = 1; i <= limit; ++i) total += s.per_length[i] << (limit - i);
            while (total > (1 << limit)) {             // the repair: one unit of 2^-limit per round
                s.per_length[limit] -= 1;
                for (int i = limit - 1; i >= 1; --i)
                    if (s.per_length[i]) {
                        s.per_length[i] -= 1;
                        s.per_length[i + 1] += 2;
                        break;
                    }
                --total;
            }
            int j = n;
            for (int length = 1; length <= limit; ++length)
                for (int c = s.per_length[length]; c > 0; --c) lengths[s.sorted[--j]] = (uint8_t)length;
        }
    }
    __syncthreads();
}

// canonical codes (RFC 1951 3.2.2), bit-reversed for the LSB-first stream: codes[s] = reversed code << 8 | length.  Lane 0 works.
__device__ void pe_assign_codes(const uint8_t* lengths, int nsym, uint32_t* codes, PeCodeScratch& s, int lane) {
    if (lane == 0) {
        for (int i = 0; i < 16; ++i) s.per_length[i] = 0;
        for (int a = 0; a < nsym; ++a) s.per_length[lengths[a]] += 1;
        s.per_length[0] = 0;
        int code = 0;
        s.next_code[0] = 0;
        for (int bits = 1; bits < 16; ++bits) {
            code = (code + s.per_length[bits - 1]) << 1;
            s.next_code[bits] = code;
        }
        for (int a = 0; a < nsym; ++a) {
            const int length = lengths[a];
            uint32_t entry = 0;
            if (length) {
                const uint32_t c = (uint32_t)s.next_code[length]++;
                entry = (__brev(c) >> (32 - length)) << 8 | (uint32_t)length;
            }
            codes[a] = entry;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(64) void png_build_code_kernel(const uint32_t* __restrict__ counts, int nsym, int limit, uint8_t* __restrict__ lengths) {
    __shared__ uint32_t cnt[kPeSymCap];
    __shared__ uint8_t len[kPeSymCap];
    __shared__ PeCodeScratch scratch;
    const int lane = threadIdx.x;
    for (int a = lane; a < nsym; a += 64) cnt[a] = counts[a];
    __syncthreads();
    pe_build_code(cnt, nsym, limit, len, scratch, lane);
    for (int a = lane; a < nsym; a += 64) lengths[a] = len[a];
}

// ---- png_segment ----
// the symbol of a match length 3..258 and its extra bits
__device__ __forceinline__ void pe_length_symbol(int length, int* symbol, int* extra_bits, int* extra) {
    const int l = length - 3;
    if (length == 258) {
        *symbol = 285, *extra_bits = 0, *extra = 0;
    } else if (l < 8) {
        *symbol = 257 + l, *extra_bits = 0, *extra = 0;
    } else {
        const int eb = 29 - __clz(l);          // floor(log2 l) - 2
        *symbol = 265 + 4 * (eb - 1) + ((l >> eb) & 3);
        *extra_bits = eb;
        *extra = l & ((1 << eb) - 1);
    }
}

__device__ __forceinline__ int pe_length_extra_bits(int symbol) {      // of a symbol 257..285
    const int k = symbol - 257;
    return (k < 8 || k == 28) ? 0 : (k - 4) >> 2;
}

// `len` bits (at most 33, value below 2^len) at bit `off` of the LSB-first buffer
__device__ __forceinline__ void pe_put(uint32_t* buf, int off, unsigned long long value, int len) {
    if (!len) return;
    const unsigned long long t = value << (off & 31);
    atomicOr(&buf[off >> 5], (uint32_t)t);
    if (t >> 32) atomicOr(&buf[(off >> 5) + 1], (uint32_t)(t >> 32));
}

// the state of a walk over a segment's tokens, wave-uniform
struct PeWalk {
    int carry_byte;          // the byte before the tile's first
    int run_start;           // where the run that reaches into the tile began
};

// One tile of 63 positions (lane 63 looks one byte ahead).  The lane at the LAST byte of a token owns it:
//   symbol >= 0: `count` (1 or 2) literals of it; symbol < 0: a match of -symbol; count 0: nothing ends here.
__device__ __forceinline__ void pe_tile(const PeSource& src, long long row0, uint32_t col0, int base, int n, int lane, PeWalk& walk, int* byte_out, int* symbol, int* count) {
    const int i = base + lane;
    int byte = 0;
    if (i < n) {
        if (src.raw) {
            byte = src.base[(size_t)row0 * src.rowlen + col0 + (uint32_t)i];
        } else {
            const uint32_t cc = col0 + (uint32_t)i, q = cc / src.rowlen;
            byte = pe_stream_byte(src, row0 + q, cc - q * src.rowlen);
        }
    }
    int prev = __shfl_up(byte, 1, 64);
    if (lane == 0) prev = walk.carry_byte;
    const int next = __shfl_down(byte, 1, 64);
    const bool active = lane < 63 && i < n;
    const bool start = active && (i == 0 || byte != prev);
    const unsigned long long starts = __ballot(start);
    const unsigned long long below = starts & ((2ULL << lane) - 1);
    const int run_start = below ? base + 63 - __clzll((long long)below) : walk.run_start;
    const int k = i - run_start;
    const bool end = i == n - 1 || next != byte;
    *byte_out = active ? byte : 0;
    *symbol = byte;
    *count = 0;
    if (active) {
        if (k == 0) {
            *count = 1;
        } else {
            const int t = (k - 1) % 258;
            if (t == 257) {
                *symbol = -258, *count = 1;
            } else if (end) {
                if (t >= 2) *symbol = -(t + 1), *count = 1;
                else *count = t + 1;
            }
        }
    }
    walk.carry_byte = __shfl(byte, 62, 64);
    if (starts) walk.run_start = base + 63 - __clzll((long long)starts);
}

// the whole words of the bit buffer go to the slot; less than a word stays
__device__ __forceinline__ void pe_flush(uint32_t* buf, uint32_t* __restrict__ dst32, int* words, int* pending, int lane) {
    __syncthreads();
    const int nw = *pending >> 5;
    const uint32_t rest = buf[nw];
    if (lane < nw) dst32[*words + lane] = buf[lane];
    __syncthreads();
    buf[lane] = 0;
    if (lane < kPeBufWords - 64) buf[64 + lane] = 0;
    __syncthreads();
    if (lane == 0) buf[0] = rest;
    *words += nw;
    *pending &= 31;
    __syncthreads();
}

__global__ __launch_bounds__(64) void png_segment_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ types, uint8_t* seg_data, int* __restrict__ seg_len,
                                                         uint32_t* __restrict__ seg_crc, uint32_t* __restrict__ seg_adler, int h, uint32_t rb, uint32_t rowlen, int bpp, int swap,
                                                         int raw, long long T, int S, int nseg, long long slot) {
    __shared__ uint32_t cnt[kPeSymCap];
    __shared__ uint8_t len[kPeSymCap];
    __shared__ uint32_t codes[kPeSymCap];
    __shared__ uint32_t cl_cnt[kPeClSyms + 1];
    __shared__ uint8_t cl_len[kPeClSyms + 1];
    __shared__ uint32_t cl_codes[kPeClSyms + 1];
    __shared__ uint16_t cl_tok[kPeSymCap];          // symbol | extra value << 5
    __shared__ int shared_ints[4];                  // hlit, the number of code-length tokens, hclen
    __shared__ PeCodeScratch scratch;
    __shared__ uint32_t bitbuf[kPeBufWords];
    __shared__ uint32_t crc_table[256];
    const int lane = threadIdx.x;
    const long long g = blockIdx.x;
    const long long img = g / nseg;
    const int seg = (int)(g - img * nseg);
    const long long p0 = (long long)seg * S;
    const int n = (int)(T - p0 < S ? T - p0 : S);
    const bool last = seg == nseg - 1;
    PeSource source;
    source.base = src + (size_t)img * (raw ? (size_t)T : (size_t)h * rb);
    source.types = raw ? nullptr : types + (size_t)img * h;
    source.rb = rb, source.rowlen = rowlen, source.bpp = bpp, source.swap = swap, source.raw = raw;
    const long long row0 = p0 / rowlen;
    const uint32_t col0 = (uint32_t)(p0 - row0 * rowlen);
    uint8_t* dst = seg_data + (size_t)g * (size_t)slot;

    for (int a = lane; a < kPeSymCap; a += 64) cnt[a] = 0;
    if (lane < kPeClSyms + 1) cl_cnt[lane] = 0;
    bitbuf[lane] = 0;
    if (lane < kPeBufWords - 64) bitbuf[64 + lane] = 0;
    for (int a = lane; a < 256; a += 64) {
        uint32_t c = (uint32_t)a;
#pragma unroll
        for (int k = 0; k < 8; ++k) c = c & 1 ? kPePoly ^ (c >> 1) : c >> 1;
        crc_table[a] = c;
    }
    __syncthreads();

    // pass 1: the histogram of the tokens and the Adler partials  A = sum d_i, B = sum (n - i) d_i
    unsigned long long sum_a = 0, sum_b = 0;
    PeWalk walk{-1, 0};
    for (int base = 0; base < n; base += 63) {
        int byte, symbol, count;
        pe_tile(source, row0, col0, base, n, lane, walk, &byte, &symbol, &count);
        sum_a += (unsigned)byte;
        sum_b += (unsigned long long)byte * (unsigned)(n - base - lane);      // (byte is 0 where the lane owns no position)
        if (count) {
            int s = symbol, eb, ev;
            if (symbol < 0) pe_length_symbol(-symbol, &s, &eb, &ev);
            atomicAdd(&cnt[s], (uint32_t)count);
        }
    }
    sum_a = pe_wave_sum64(sum_a);
    sum_b = pe_wave_sum64(sum_b);
    if (lane == 0) {
        cnt[256] = 1;
        seg_adler[2 * g] = (uint32_t)(sum_a % 65521);
        seg_adler[2 * g + 1] = (uint32_t)(sum_b % 65521);
    }
    __syncthreads();

    // the two codes and the cost of the dynamic block
    pe_build_code(cnt, kPeLitSyms, kPeLitLimit, len, scratch, lane);
    pe_assign_codes(len, kPeLitSyms, codes, scratch, lane);
    if (lane == 0) {
        int hlit = kPeLitSyms;
        while (len[hlit - 1] == 0) --hlit;            // (>= 257: the end of block is always used)
        len[hlit] = 1;                                // the one distance code, symbol 0 of length 1, behind the literal/length lengths
        const int total = hlit + 1;
        int ntok = 0;
        for (int i = 0; i < total;) {                 // tests/png_encode_ref.py cl_tokens
            const int v = len[i];
            int run = 1;
            while (i + run < total && len[i + run] == v) ++run;
            int symbol = v, extra = 0;
            if (v == 0 && run >= 11) {
                run = run < 138 ? run : 138;
                symbol = 18, extra = run - 11;
            } else if (v == 0 && run >= 3) {
                symbol = 17, extra = run - 3;
            } else if (v != 0 && i > 0 && len[i - 1] == v && run >= 3) {
                run = run < 6 ? run : 6;
                symbol = 16, extra = run - 3;
            } else {
                run = 1;
            }
            cl_tok[ntok++] = (uint16_t)(symbol | extra << 5);
            cl_cnt[symbol] += 1;
            i += run;
        }
        shared_ints[0] = hlit;
        shared_ints[1] = ntok;
    }
    __syncthreads();
    pe_build_code(cl_cnt, kPeClSyms, kPeClLimit, cl_len, scratch, lane);
    pe_assign_codes(cl_len, kPeClSyms, cl_codes, scratch, lane);
    if (lane == 0) {
        int hclen = kPeClSyms;
        while (hclen > 4 && cl_len[g_pe_cl_order[hclen - 1]] == 0) --hclen;
        shared_ints[2] = hclen;
    }
    __syncthreads();
    const int hlit = shared_ints[0], ntok = shared_ints[1], hclen = shared_ints[2];
    int bits = 0;
    for (int t = lane; t < ntok; t += 64) {
        const int symbol = cl_tok[t] & 31;
        bits += cl_len[symbol] + (symbol == 16 ? 2 : symbol == 17 ? 3 : symbol == 18 ? 7 : 0);
    }
    for (int a = lane; a < kPeLitSyms; a += 64) bits += (int)cnt[a] * (len[a] + (a >= 257 ? pe_length_extra_bits(a) + 1 : 0));
    bits = pe_wave_sum(bits) + 17 + 3 * hclen;
    const int dynamic_bytes = last ? (bits + 7) >> 3 : ((bits + 3 + 7) >> 3) + 4;
    int length;

    if (dynamic_bytes >= 5 + n) {          // one stored block
        if (lane == 0) {
            dst[0] = last ? 1 : 0;
            dst[1] = (uint8_t)(n & 255), dst[2] = (uint8_t)(n >> 8);
            dst[3] = (uint8_t)(~n & 255), dst[4] = (uint8_t)((~n >> 8) & 255);
        }
        for (int i = lane; i < n; i += 64) {
            const uint32_t cc = col0 + (uint32_t)i, q = cc / rowlen;
            dst[5 + i] = (uint8_t)(raw ? source.base[(size_t)p0 + i] : pe_stream_byte(source, row0 + q, cc - q * rowlen));
        }
        length = 5 + n;
    } else {
        uint32_t* dst32 = (uint32_t*)dst;          // (the slot is 16-byte aligned)
        int words = 0, pending = 17 + 3 * hclen;
        if (lane == 0) {
            pe_put(bitbuf, 0, (unsigned)(last ? 1 : 0) | 2u << 1 | (unsigned)(hlit - 257) << 3 | (unsigned)(hclen - 4) << 13, 17);
            for (int k = 0; k < hclen; ++k) pe_put(bitbuf, 17 + 3 * k, cl_len[g_pe_cl_order[k]], 3);
        }
        pe_flush(bitbuf, dst32, &words, &pending, lane);
        for (int first = 0; first < ntok; first += 64) {
            unsigned long long value = 0;
            int nbits = 0;
            if (first + lane < ntok) {
                const int tok = cl_tok[first + lane], symbol = tok & 31;
                const uint32_t e = cl_codes[symbol];
                nbits = (int)(e & 255);
                value = (e >> 8) | (unsigned long long)(tok >> 5) << nbits;
                nbits += symbol == 16 ? 2 : symbol == 17 ? 3 : symbol == 18 ? 7 : 0;
            }
            const int incl = pe_scan_incl(nbits, lane);
            pe_put(bitbuf, pending + incl - nbits, value, nbits);
            pending += __shfl(incl, 63, 64);
            pe_flush(bitbuf, dst32, &words, &pending, lane);
        }
        // pass 2: the tokens again, now as codes
        walk = PeWalk{-1, 0};
        for (int base = 0; base < n; base += 63) {
            int byte, symbol, count;
            pe_tile(source, row0, col0, base, n, lane, walk, &byte, &symbol, &count);
            unsigned long long value = 0;
            int nbits = 0;
            if (count && symbol >= 0) {
                const uint32_t e = codes[symbol];
                nbits = (int)(e & 255);
                value = e >> 8;
                if (count == 2) value |= value << nbits, nbits *= 2;
            } else if (count) {
                int s, eb, ev;
                pe_length_symbol(-symbol, &s, &eb, &ev);
                const uint32_t e = codes[s];
                nbits = (int)(e & 255);
                value = (e >> 8) | (unsigned long long)ev << nbits;
                nbits += eb + 1;                    // the extra bits and the distance code: one 0 bit
            }
            const int incl = pe_scan_incl(nbits, lane);
            pe_put(bitbuf, pending + incl - nbits, value, nbits);
            pending += __shfl(incl, 63, 64);
            pe_flush(bitbuf, dst32, &words, &pending, lane);
        }
        if (lane == 0) pe_put(bitbuf, pending, codes[256] >> 8, (int)(codes[256] & 255));
        pending += (int)(codes[256] & 255);
        pe_flush(bitbuf, dst32, &words, &pending, lane);
        if (!last) {                                // an empty stored block: 000, pad to the byte, 00 00 FF FF
            pending = (pending + 3 + 7) & ~7;
            if (lane == 0) pe_put(bitbuf, pending, 0xFFFF0000u, 32);
            pending += 32;
            pe_flush(bitbuf, dst32, &words, &pending, lane);
        }
        const int tail = (pending + 7) >> 3;        // at most 4 bytes are left
        if (lane < tail) dst[4 * words + lane] = (uint8_t)(bitbuf[0] >> (8 * lane));
        length = 4 * words + tail;
    }
    __syncthreads();
    __threadfence_block();

    // the chunk's CRC-32 over "IDAT" + dst[0 .. length): zero bytes in front up to 64 slices of L bytes (they leave a zero register
    // zero), the register behind "IDAT" folded into the first four bytes, a table walk per slice, then the slices combined in a tree:
    // crc(A B) = crc(A) x^(8 |B|) + crc(B)
    const volatile uint8_t* data = dst;
    const int L = (length + 63) >> 6, pad = 64 * L - length;
    uint32_t crc = 0;
    for (int v = lane * L; v < (lane + 1) * L; ++v) {
        if (v < pad) continue;
        const int at = v - pad;
        uint32_t byte = data[at];
        if (at < 4) byte ^= (kPeIdatState >> (8 * at)) & 255;
        crc = crc_table[(crc ^ byte) & 255] ^ (crc >> 8);
    }
    uint32_t op = 0x80000000u;                      // x^(8 L): square and multiply over the bits of L, from x^8
    for (int bit = 0; (L >> bit) != 0; ++bit)
        if ((L >> bit) & 1) op = pe_mulmod(g_pe_x2n.v[(bit + 3) & 31], op);
#pragma unroll 1
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t other = __shfl_down(crc, d, 64);
        crc = pe_mulmod(op, crc) ^ other;
        op = pe_mulmod(op, op);
    }
    if (lane == 0) {
        seg_len[g] = length;
        seg_crc[g] = ~crc;
    }
}

// ---- png_scan ----
__global__ __launch_bounds__(256) void png_scan_kernel(const int* __restrict__ seg_len, const uint32_t* __restrict__ seg_adler, long long* __restrict__ seg_off,
                                                       uint32_t* __restrict__ frame, int nseg, long long T, int S, int header_len, int per_segment, int tail_len,
                                                       long long out_stride, long long* __restrict__ lengths) {
    __shared__ long long wave_sum[4], wave_a[4];
    __shared__ unsigned long long wave_b[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long base = (long long)blockIdx.x * nseg;
    long long running = header_len, running_a = 1;           // Adler-32 starts at A = 1, B = 0
    unsigned long long sum_b = 0;
    for (int first = 0; first < nseg; first += 256) {
        const int i = first + t;
        const bool in = i < nseg;
        const long long v = in ? (long long)seg_len[base + i] + per_segment : 0;
        const long long a = in ? (long long)seg_adler[2 * (base + i)] : 0;
        long long s = v, sa = a;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long u = __shfl_up(s, d, 64), ua = __shfl_up(sa, d, 64);
            if (lane >= d) s += u, sa += ua;
        }
        if (lane == 63) wave_sum[wave] = s, wave_a[wave] = sa;
        __syncthreads();
        long long before = 0, all = 0, before_a = 0, all_a = 0;
        for (int k = 0; k < 4; ++k) {
            if (k < wave) before += wave_sum[k], before_a += wave_a[k];
            all += wave_sum[k], all_a += wave_a[k];
        }
        if (in) {
            seg_off[base + i] = running + before + s - v;
            // B after the segment = B + n_k A + B_k, with A the sum before it (adler32_combine)
            const long long n_k = T - (long long)i * S < S ? T - (long long)i * S : S;
            const unsigned long long a_before = (unsigned long long)((running_a + before_a + sa - a) % 65521);
            sum_b += (unsigned long long)n_k * a_before % 65521 + seg_adler[2 * (base + i) + 1];
        }
        running += all;
        running_a = (running_a + all_a) % 65521;
        __syncthreads();
    }
    sum_b = pe_wave_sum64(sum_b);
    if (lane == 0) wave_b[wave] = sum_b;
    __syncthreads();
    if (t == 0) {
        const uint32_t adler = (uint32_t)((wave_b[0] + wave_b[1] + wave_b[2] + wave_b[3]) % 65521) << 16 | (uint32_t)running_a;
        uint32_t crc = kPeIdatState;
        for (int k = 3; k >= 0; --k) {
            crc ^= (adler >> (8 * k)) & 255;
            for (int j = 0; j < 8; ++j) crc = crc & 1 ? kPePoly ^ (crc >> 1) : crc >> 1;
        }
        frame[2 * blockIdx.x] = adler;
        frame[2 * blockIdx.x + 1] = ~crc;
        running += tail_len;
        lengths[blockIdx.x] = running <= out_stride ? running : -running;
    }
}

// ---- png_copy ----
__device__ __forceinline__ void pe_store_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v;
}

__global__ __launch_bounds__(64 * kPeCopyWaves) void png_copy_kernel(const uint8_t* __restrict__ seg_data, const int* __restrict__ seg_len, const long long* __restrict__ seg_off,
                                                                    const uint32_t* __restrict__ seg_crc, const uint32_t* __restrict__ frame,
                                                                    const long long* __restrict__ lengths, const uint8_t* __restrict__ header, int header_len, int framed,
                                                                    uint8_t* __restrict__ out, long long out_stride, int nseg, long long segs, long long slot) {
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * kPeCopyWaves + (threadIdx.x >> 6);
    if (g >= segs) return;
    const long long img = g / nseg;
    const int seg = (int)(g - img * nseg);
    if (lengths[img] < 0) return;      // the file does not fit its slot: not a byte of it is written
    uint8_t* __restrict__ file = out + (size_t)img * (size_t)out_stride;
    if (seg == 0) {
        if (framed) {
            for (int i = lane; i < header_len; i += 64) file[i] = header[i];
        } else if (lane < 2) {
            file[lane] = lane ? 0x01 : 0x78;      // the bare zlib stream of resr_png_debug_deflate
        }
    }
    const uint8_t* __restrict__ s = seg_data + (size_t)g * (size_t)slot;
    uint8_t* __restrict__ d = file + seg_off[g];
    const int len = seg_len[g];
    if (framed) {
        if (lane == 0) {
            pe_store_be32(d, (uint32_t)len);
            d[4] = 'I', d[5] = 'D', d[6] = 'A', d[7] = 'T';
            pe_store_be32(d + 8 + len, seg_crc[g]);
        }
        d += 8;
    }
    for (int i = lane; i < len; i += 64) d[i] = s[i];
    if (seg == nseg - 1 && lane == 0) {
        uint8_t* e = d + len + (framed ? 4 : 0);
        if (framed) {
            pe_store_be32(e, 4);
            e[4] = 'I', e[5] = 'D', e[6] = 'A', e[7] = 'T';
            pe_store_be32(e + 8, frame[2 * img]);
            pe_store_be32(e + 12, frame[2 * img + 1]);
            pe_store_be32(e + 16, 0);
            e[20] = 'I', e[21] = 'E', e[22] = 'N', e[23] = 'D';
            pe_store_be32(e + 24, 0xAE426082u);
        } else {
            pe_store_be32(e, frame[2 * img]);
        }
    }
}

size_t pe_pad16(size_t v) { return (v + 15) / 16 * 16; }

// the part of the plan that a byte stream alone has (resr_png_debug_deflate): n streams of T bytes in segments of S
bool pe_plan_stream(int n, int64_t T, int S, int64_t rows, PePlan* p, const char* who) {
    p->T = T, p->S = S, p->rows = rows;
    const int64_t nseg = (T + S - 1) / S;
    p->segs = (int64_t)n * nseg;
    if (nseg > 0x7fffffffLL || p->segs > 0x7fffffffLL || rows > 0x7fffffffLL)
        return fail(RESR_ERR_ARG, "%s: %d frames of %lld segments and %lld rows do not fit the grid of a launch", who, n, (long long)nseg, (long long)(rows / n)), false;
    p->nseg = (int)nseg;
    p->slot = (int64_t)pe_pad16((size_t)(T < S ? T : S) + 5);
    p->off_off = pe_pad16((size_t)p->segs * 4);
    p->crc_off = p->off_off + pe_pad16((size_t)p->segs * 8);
    p->adler_off = p->crc_off + pe_pad16((size_t)p->segs * 4);
    p->frame_off = p->adler_off + pe_pad16((size_t)p->segs * 8);
    p->type_off = p->frame_off + pe_pad16((size_t)n * 8);
    p->data_off = p->type_off + pe_pad16((size_t)rows);
    p->bytes = p->data_off + (size_t)p->segs * (size_t)p->slot;
    return true;
}

bool pe_plan(const ResrPngEncDesc* d, PePlan* p) {
    if (!d) return fail(RESR_ERR_ARG, "png_encode: null descriptor"), false;
    if (d->channels != 1 && d->channels != 3 && d->channels != 4) return fail(RESR_ERR_ARG, "png_encode: %d channels (1, 3 or 4: grey, RGB, RGBA)", d->channels), false;
    if (d->bit_depth != 8 && d->bit_depth != 16) return fail(RESR_ERR_ARG, "png_encode: bit depth %d (8 or 16)", d->bit_depth), false;
    p->bpp = d->channels * d->bit_depth / 8;
    p->swap = d->bit_depth == 16 ? 1 : 0;
    if (d->n < 1 || d->h < 1 || d->w < 1 || d->h > 0x7fffffff / p->bpp || d->w > 0x7fffffff / p->bpp)
        return fail(RESR_ERR_ARG, "png_encode: bad geometry (n=%d, images %dx%d of %d bytes a pixel: n at least 1, h and w in 1..(2^31-1)/bpp)", d->n, d->h, d->w, p->bpp), false;
    if (d->segment_bytes != 0 && (d->segment_bytes < 64 || d->segment_bytes > 65535))
        return fail(RESR_ERR_ARG, "png_encode: segment_bytes %d is outside 64..65535 (0 = the default, %d)", d->segment_bytes, RESR_PNG_DEFAULT_SEGMENT_BYTES), false;
    p->rb = (uint32_t)d->w * (uint32_t)p->bpp;
    p->rowlen = p->rb + 1;
    return pe_plan_stream(d->n, (int64_t)d->h * (int64_t)p->rowlen, d->segment_bytes ? d->segment_bytes : RESR_PNG_DEFAULT_SEGMENT_BYTES, (int64_t)d->n * d->h, p, "png_encode");
}

int pe_launch(const PePlan& p, int n, int h, int raw, const uint8_t* src, uint8_t* out, int64_t out_stride, int64_t* lengths, const uint8_t* header_dev, void* workspace,
              hipStream_t st) {
    uint8_t* ws = (uint8_t*)workspace;
    int* seg_len = (int*)ws;
    long long* seg_off = (long long*)(ws + p.off_off);
    uint32_t* seg_crc = (uint32_t*)(ws + p.crc_off);
    uint32_t* seg_adler = (uint32_t*)(ws + p.adler_off);
    uint32_t* frame = (uint32_t*)(ws + p.frame_off);
    uint8_t* types = ws + p.type_off;
    uint8_t* seg_data = ws + p.data_off;
    const double bytes = (double)n * (double)p.T;
    if (!raw) {
        prof_before(st);
        hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)p.rows), dim3(64), 0, st, src, types, h, p.rb, p.bpp, p.swap);
        prof_after(st, 35300, 0.0, 2.0 * bytes);
        RESR_CHECK_LAUNCH("png_filter_kernel");
    }
    prof_before(st);
    hipLaunchKernelGGL(png_segment_kernel, dim3((unsigned)p.segs), dim3(64), 0, st, src, (const uint8_t*)types, seg_data, seg_len, seg_crc, seg_adler, h, p.rb, p.rowlen, p.bpp, p.swap,
                       raw, (long long)p.T, p.S, p.nseg, (long long)p.slot);
    prof_after(st, 35400, 0.0, 3.0 * bytes);
    RESR_CHECK_LAUNCH("png_segment_kernel");
    prof_before(st);
    hipLaunchKernelGGL(png_scan_kernel, dim3((unsigned)n), dim3(256), 0, st, (const int*)seg_len, (const uint32_t*)seg_adler, seg_off, frame, p.nseg, (long long)p.T, p.S,
                       raw ? 2 : kPeHeaderBytes, raw ? 0 : 12, raw ? 4 : 28, (long long)out_stride, (long long*)lengths);
    prof_after(st, 35500, 0.0, (double)p.segs * 24.0);
    RESR_CHECK_LAUNCH("png_scan_kernel");
    prof_before(st);
    hipLaunchKernelGGL(png_copy_kernel, dim3((unsigned)((p.segs + kPeCopyWaves - 1) / kPeCopyWaves)), dim3(64 * kPeCopyWaves), 0, st, (const uint8_t*)seg_data, (const int*)seg_len,
                       (const long long*)seg_off, (const uint32_t*)seg_crc, (const uint32_t*)frame, (const long long*)lengths, header_dev, raw ? 2 : kPeHeaderBytes, raw ? 0 : 1, out,
                       (long long)out_stride, p.nseg, (long long)p.segs, (long long)p.slot);
    prof_after(st, 35600, 0.0, 2.0 * bytes);
    RESR_CHECK_LAUNCH("png_copy_kernel");
    return RESR_OK;
}

void pe_host_be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v; }

// length, type, data, CRC at p -> the byte behind the chunk
uint8_t* pe_host_chunk(uint8_t* p, const char* type, const uint8_t* data, uint32_t n) {
    pe_host_be32(p, n);
    for (int i = 0; i < 4; ++i) p[4 + i] = (uint8_t)type[i];
    for (uint32_t i = 0; i < n; ++i) p[8 + i] = data[i];
    pe_host_be32(p + 8 + n, ~pe_crc_raw(0xFFFFFFFFu, p + 4, 4 + n));
    return p + 12 + n;
}
}  // namespace

// no file of this geometry is longer: F stored (5 bytes a segment), 12 bytes of chunk framing a segment, the header and the two last chunks
size_t png_encode_max_bytes(const ResrPngEncDesc* d) {
    PePlan p;
    return pe_plan(d, &p) ? (size_t)p.T + 17 * (size_t)p.nseg + 75 : 0;
}

size_t png_encode_workspace_bytes(const ResrPngEncDesc* d) {
    PePlan p;
    return pe_plan(d, &p) ? p.bytes : 0;
}

int png_encode_header(const ResrPngEncDesc* d, uint8_t* host_buf, size_t cap) {
    PePlan p;
    if (!pe_plan(d, &p)) return RESR_ERR_ARG;
    if (!host_buf) return kPeHeaderBytes;
    if (cap < (size_t)kPeHeaderBytes) return fail(RESR_ERR_ARG, "png_encode_header: a buffer of %zu bytes, %d needed", cap, kPeHeaderBytes);
    const uint8_t signature[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    for (int i = 0; i < 8; ++i) host_buf[i] = signature[i];
    uint8_t ihdr[13];
    pe_host_be32(ihdr, (uint32_t)d->w);
    pe_host_be32(ihdr + 4, (uint32_t)d->h);
    ihdr[8] = (uint8_t)d->bit_depth;
    ihdr[9] = (uint8_t)(d->channels == 1 ? 0 : d->channels == 3 ? 2 : 6);      // colour type: grey, RGB, RGBA
    ihdr[10] = ihdr[11] = ihdr[12] = 0;                                          // deflate, the five filters, not interlaced
    uint8_t* at = pe_host_chunk(host_buf + 8, "IHDR", ihdr, 13);
    const uint8_t zlib_header[2] = {0x78, 0x01};
    at = pe_host_chunk(at, "IDAT", zlib_header, 2);
    if (at - host_buf != kPeHeaderBytes) return fail(RESR_ERR_ARG, "png_encode_header: wrote %d bytes, not %d", (int)(at - host_buf), kPeHeaderBytes);
    return kPeHeaderBytes;
}

int png_encode_dispatch(const ResrPngEncDesc* d, const void* src, uint8_t* out, int64_t out_stride, int64_t* lengths, const uint8_t* header_dev, int header_len, void* workspace,
                        size_t workspace_bytes, hipStream_t st) {
    PePlan p;
    if (!pe_plan(d, &p)) return RESR_ERR_ARG;
    if (!src || !out || !lengths || !header_dev || !workspace) return fail(RESR_ERR_ARG, "png_encode: null pointer");
    if (out_stride < 0) return fail(RESR_ERR_ARG, "png_encode: out_stride %lld is negative", (long long)out_stride);
    if (header_len != kPeHeaderBytes) return fail(RESR_ERR_ARG, "png_encode: a header of %d bytes, it has %d (resr_png_encode_header)", header_len, kPeHeaderBytes);
    if (((uintptr_t)workspace & 15) || ((uintptr_t)lengths & 7)) return fail(RESR_ERR_ARG, "png_encode: the workspace must be 16-byte and lengths 8-byte aligned");
    if (workspace_bytes < p.bytes) return fail(RESR_ERR_ARG, "png_encode: workspace of %zu bytes, %zu needed", workspace_bytes, p.bytes);
    return pe_launch(p, d->n, d->h, 0, (const uint8_t*)src, out, out_stride, lengths, header_dev, workspace, st);
}

size_t png_debug_deflate_workspace_bytes(int64_t stream_bytes, int segment_bytes) {
    PePlan p{};
    if (stream_bytes < 1 || segment_bytes < 64 || segment_bytes > 65535) return fail(RESR_ERR_ARG, "png_debug_deflate: %lld bytes in segments of %d", (long long)stream_bytes, segment_bytes), 0;
    return pe_plan_stream(1, stream_bytes, segment_bytes, 0, &p, "png_debug_deflate") ? p.bytes : 0;
}

int png_debug_deflate(const uint8_t* stream_dev, int64_t stream_bytes, int segment_bytes, uint8_t* out, int64_t out_capacity, int64_t* length, void* workspace, size_t workspace_bytes,
                      hipStream_t st) {
    PePlan p{};
    if (stream_bytes < 1 || segment_bytes < 64 || segment_bytes > 65535) return fail(RESR_ERR_ARG, "png_debug_deflate: %lld bytes in segments of %d", (long long)stream_bytes, segment_bytes);
    if (!pe_plan_stream(1, stream_bytes, segment_bytes, 0, &p, "png_debug_deflate")) return RESR_ERR_ARG;
    if (!stream_dev || !out || !length || !workspace || out_capacity < 0) return fail(RESR_ERR_ARG, "png_debug_deflate: null pointer or negative capacity");
    if (((uintptr_t)workspace & 15) || ((uintptr_t)length & 7)) return fail(RESR_ERR_ARG, "png_debug_deflate: the workspace must be 16-byte and length 8-byte aligned");
    if (workspace_bytes < p.bytes) return fail(RESR_ERR_ARG, "png_debug_deflate: workspace of %zu bytes, %zu needed", workspace_bytes, p.bytes);
    p.rb = 0, p.rowlen = (uint32_t)segment_bytes, p.bpp = 1, p.swap = 0;      // raw: F[row][col] is the stream itself
    return pe_launch(p, 1, 0, 1, stream_dev, out, out_capacity, length, nullptr, workspace, st);
}

int png_debug_build_code(const uint32_t* counts_dev, int nsym, int limit, uint8_t* lengths_dev, hipStream_t st) {
    if (!counts_dev || !lengths_dev || nsym < 1 || nsym > kPeLitSyms || limit < 1 || limit > 15 || (nsym > 1 && (1 << limit) < nsym))
        return fail(RESR_ERR_ARG, "png_debug_build_code: null pointer, or %d symbols (1..%d) at limit %d (1..15, 2^limit at least the symbols)", nsym, kPeLitSyms, limit);
    hipLaunchKernelGGL(png_build_code_kernel, dim3(1), dim3(64), 0, st, counts_dev, nsym, limit, lengths_dev);
    RESR_CHECK_LAUNCH("png_build_code_kernel");
    return RESR_OK;
}

}  // namespace resr
