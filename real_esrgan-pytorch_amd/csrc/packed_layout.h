// packed_layout.h -- THE definition of the packed weight format: what resr_pack_weights writes, how its buffers are sized, and the chunk
// tables that describe it.  Every planner (generator.hip, compact.hip, disc_native.hip), the launcher's group stride (conv3x3.hip), the
// pack kernels' block size (pack.hip) and the C ABI's table / size entries (api.hip) take it from here.
//
// The format.  The module keeps the reference's OIHW fp32 parameters; resr_pack_weights turns them (one launch for all convolutions, both
// the forward and the backward-data forms) into the order the convolution kernels stream them:
//     group (<= 64 M rows) -> chunk (32 K channels) -> tap (9) -> k-step -> M tile (mt = 1 or 2) -> lane (kh * 32 + m) -> 16 bytes
// so that a wave's A fragment is one contiguous, coalesced 1 KiB load.  One (group, chunk) BLOCK is 9 * mt * 1024 elements
// (packed_chunk_elems); the order inside a block is pack.hip's index decomposition.  A convolution of M x K padded channels is its M rows
// in groups of at most 64, group-major, each group holding its K / 32 chunks; m_count / k_count of a chunk are the REAL rows / channels,
// the rest of the block is zero.  Forward: M = cout, K = cin.  Backward-data chunks are gathered transposed (M = cin, K = cout) with
// flipped taps and an optional scale (the 0.2 residual scalings folded into the weights).  A 4x4 / stride-2 kernel enters as its virtual
// 3x3 kernel over the 2x2 space-to-depth image (ResrPackChunk.virtual4x4: 4 * cin virtual channels).
// RESR_F16X2 (exact16): a block becomes THREE consecutive f16 blocks of the plain block's size (packed_blocks), in the stage order of the
// conv kernel: W0 = f16(w * 2^12) (multiplies x_hi), W1 = f16(w * 2^12 - W0) (x_hi again), W2 = f16(W0 * 2^-12) (multiplies x_lo, which
// is stored times 2^12).  A table's dst_off counts elements of the PLAIN layout; the kernels triple it.
// Slack: every buffer ends in kPackedSlack bytes, because the one-role conv kernel prefetches two (chunk, tap) blocks past the end.
// MX stages (RESR_CONV_MX_PAIRS, resr_pack_weights_mx): behind the f16 blocks and their slack, 256-byte aligned (packed_mx_offset), lies
// a region that mirrors a plain f16 packing byte for byte -- chunk i is one block of 9 x (32 mt) x 64 bytes at 2 * dst_off: per tap and
// output row the bytes [bf8(W1[k]), k = 0..31 | bf8(W2[k])] of the exact16 split, as A fragments of v_mfma_scale_f32_32x32x64_f8f6f4.
// The kernels index this format on the device with their own constants and are NOT derived from this file: conv3x3.hip, conv3x3_ws.h,
// conv3x3_ws_chain.h.  tests/gpu_util.py (pack_conv) and tests/test_gpu_mx.py (_pack_mx) spell it once more, independently, on purpose.
#pragma once
#include <vector>

#include "common.h"

namespace resr {

constexpr int round32(int v) { return (v + 31) / 32 * 32; }

__host__ __device__ constexpr int packed_chunk_elems(int mt) { return 9 * mt * 1024; }   // one (group, chunk) block of mt M tiles
__host__ __device__ constexpr int packed_blocks(bool x2) { return x2 ? 3 : 1; }          // f16 blocks per block: exact16's W0, W1, W2
constexpr int packed_group_mt(int m_pad, int g0) { return (m_pad - g0 < 64 ? m_pad - g0 : 64) / 32; }   // M tiles of the group that starts at row g0
constexpr size_t packed_group_elems(int k_pad, int mt) { return (size_t)(k_pad / 32) * packed_chunk_elems(mt); }
constexpr int packed_conv_chunks(int m_pad, int k_pad) { return (m_pad + 63) / 64 * (k_pad / 32); }
inline size_t packed_conv_elems(int m_pad, int k_pad) {
    size_t e = 0;
    for (int g0 = 0; g0 < m_pad; g0 += 64) e += packed_group_elems(k_pad, packed_group_mt(m_pad, g0));
    return e;
}

inline size_t packed_elem_bytes(int dtype) { return elem_size(dtype) * packed_blocks(dtype == RESR_F16X2); }
constexpr size_t kPackedSlack = 16384;
inline size_t packed_buffer_bytes(size_t elems, int dtype) { return elems * packed_elem_bytes(dtype) + kPackedSlack; }
inline size_t packed_mx_offset(size_t elems) { return align_up(packed_buffer_bytes(elems, RESR_F16X2), 256); }
inline size_t packed_mx_buffer_bytes(size_t elems) { return packed_mx_offset(elems) + packed_buffer_bytes(elems, RESR_F16); }

inline ResrPackChunk pack_chunk(int64_t src_off, int64_t dst_off, int src_cout, int src_cin, int m_off, int m_count, int k_off, int k_count,
                                int mt, int transposed, float scale = 1.f, int virtual4x4 = 0, const float* scale_ptr = nullptr) {
    ResrPackChunk c;
    memset(&c, 0, sizeof(c));
    c.src_off = src_off; c.dst_off = dst_off; c.src_cout = src_cout; c.src_cin = src_cin;
    c.m_off = m_off; c.m_count = m_count; c.k_off = k_off; c.k_count = k_count;
    c.mt = mt; c.transposed = transposed; c.scale = scale; c.virtual4x4 = virtual4x4; c.scale_ptr = scale_ptr;
    return c;
}

// Appends the table of ONE convolution [src_cout][src_cin][3][3] (virtual4x4: [4][4]) at src_off in one orientation, packed from dst_off
// on; returns the elements it takes there (= packed_conv_elems of its padded M and K).
inline size_t emit_conv_chunks(std::vector<ResrPackChunk>& t, int64_t src_off, int src_cout, int src_cin, int transposed, int64_t dst_off,
                               float scale = 1.f, int virtual4x4 = 0, const float* scale_ptr = nullptr) {
    const int cin_v = virtual4x4 ? 4 * src_cin : src_cin;
    const int m_real = transposed ? cin_v : src_cout, k_real = transposed ? src_cout : cin_v;
    const int m_pad = round32(m_real), k_pad = round32(k_real);
    int64_t dst = dst_off;
    for (int g0 = 0; g0 < m_pad; g0 += 64) {
        const int mt = packed_group_mt(m_pad, g0);
        for (int k0 = 0; k0 < k_pad; k0 += 32) {
            t.push_back(pack_chunk(src_off, dst, src_cout, src_cin, g0, m_real - g0 < 64 ? m_real - g0 : 64, k0, k_real - k0 < 32 ? k_real - k0 : 32,
                                   mt, transposed, scale, virtual4x4, scale_ptr));
            dst += packed_chunk_elems(mt);
        }
    }
    return (size_t)(dst - dst_off);
}

// The tail of every *_pack_table entry: the count when `out` is null ("ask with (NULL, 0) for the length"), else the copy.
inline int64_t copy_pack_table(const std::vector<ResrPackChunk>& t, ResrPackChunk* out, int64_t cap, const char* who) {
    if (out) {
        if ((int64_t)t.size() > cap) return fail(RESR_ERR_ARG, "%s: capacity %lld < %zu", who, (long long)cap, t.size());
        memcpy(out, t.data(), t.size() * sizeof(ResrPackChunk));
    }
    return (int64_t)t.size();
}

}  // namespace resr
