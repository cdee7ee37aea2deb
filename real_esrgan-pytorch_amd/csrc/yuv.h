// yuv.h -- the integer YUV 4:2:0 <-> RGB definition of include/resr.h as device helpers, templates over bits per sample, and the two
// float conversions every end of the frame path uses (level -> unit float, float -> level), and the image modes' pixel load, grey and
// mode switch.  Shared by frames.hip (the heads, the tails at the network's own factor, the generic conversions) and image_resize.hip
// (the YUV and image ends of the outscale tail): one definition of each, hence the same bits everywhere.  frames.py holds the definition once more in numpy, which the tests compare with.
#pragma once
#include "common.h"

namespace resr {

// TOP: the highest level of a sample, 255 (8 bits), 1023 (10 bits) or 65535 (the 16-bit image modes)
template <int TOP>
__device__ __forceinline__ float unit_of(unsigned v) { return (float)v / (float)TOP; }

template <int TOP>
__device__ __forceinline__ unsigned quantise(float v) {
    v *= (float)TOP;
    v = v > 0.f ? v : 0.f;          // (a NaN compares false: 0)
    v = v < (float)TOP ? v : (float)TOP;
    return (unsigned)v;             // truncation, as astype(uint8) of a value in [0, 255]
}

// BITS per sample, 8 or 10 (every template below defaults to 8): the word a sample is stored in, the highest level, and the studio
// offsets 16 / 128, which scale with the depth (64 / 512 at 10 bits).  16: the image modes' full 16-bit word (RGB levels only: the
// YUV formulas below are not instantiated for it -- their int32 accumulators would overflow).
template <int BITS> struct Depth { typedef uint8_t word; };
template <> struct Depth<10> { typedef uint16_t word; };
template <> struct Depth<16> { typedef uint16_t word; };
template <int BITS> constexpr int kTop = (1 << BITS) - 1;
template <int BITS> constexpr int kLumaOff = 16 << (BITS - 8);
template <int BITS> constexpr int kChromaOff = 128 << (BITS - 8);

// Bits per sample of a layout: 8, 10, or 0 for a value that is no RESR_YUV_*
constexpr int yuv_bits(int layout) {
    return layout == RESR_YUV_I420 || layout == RESR_YUV_NV12 ? 8 : layout == RESR_YUV_I420P10 || layout == RESR_YUV_P010 ? 10 : 0;
}

// A runtime layout as a compile-time one, as with_scale: f(std::integral_constant<int, layout>()); false for any other value.
template <typename F>
inline bool with_yuv_layout(int layout, F&& f) {
    switch (layout) {
        case RESR_YUV_I420: f(std::integral_constant<int, RESR_YUV_I420>()); return true;
        case RESR_YUV_NV12: f(std::integral_constant<int, RESR_YUV_NV12>()); return true;
        case RESR_YUV_I420P10: f(std::integral_constant<int, RESR_YUV_I420P10>()); return true;
        case RESR_YUV_P010: f(std::integral_constant<int, RESR_YUV_P010>()); return true;
        default: return false;
    }
}

// NV12 and P010 hold one interleaved CbCr plane, I420 and I420P10 a Cb and a Cr plane
__device__ __forceinline__ constexpr bool semi_planar(int layout) { return layout == RESR_YUV_NV12 || layout == RESR_YUV_P010; }

// A 10-bit sample sits in the low bits of its 16-bit word (I420P10; the high 6 ignored on the way in, zero on the way out) or in the
// high bits (P010; the low 6 likewise).  A byte is its sample.
template <int BITS>
__device__ __forceinline__ int sample_of(unsigned word, int layout) {
    if constexpr (BITS == 8) return (int)word;
    else return (int)(layout == RESR_YUV_P010 ? word >> 6 : word & 1023u);
}

template <int BITS>
__device__ __forceinline__ unsigned word_of(unsigned sample, int layout) {
    if constexpr (BITS == 8) return sample;
    else return layout == RESR_YUV_P010 ? sample << 6 : sample;
}

// The three samples of pixel (y, x) of one image of luma size h x w (both even): chroma is replicated over its 2x2 block.
template <int BITS = 8>
__device__ __forceinline__ void yuv_load(const typename Depth<BITS>::word* __restrict__ img, int h, int w, int layout, int y, int x, int& Y,
                                         int& Cb, int& Cr) {
    const long luma = (long)h * w;
    Y = sample_of<BITS>(img[(long)y * w + x], layout);
    if (semi_planar(layout)) {
        const typename Depth<BITS>::word* c = img + luma + (long)(y >> 1) * w + (x & ~1);
        Cb = sample_of<BITS>(c[0], layout);
        Cr = sample_of<BITS>(c[1], layout);
    } else {
        const long o = (long)(y >> 1) * (w >> 1) + (x >> 1);
        Cb = sample_of<BITS>(img[luma + o], layout);
        Cr = sample_of<BITS>(img[luma + (luma >> 2) + o], layout);
    }
}

template <int BITS = 8>
__device__ __forceinline__ void yuv_to_rgb(const ResrYuvDesc& q, int Y, int Cb, int Cr, unsigned (&rgb)[3]) {
    const int y = Y - kLumaOff<BITS>, cb = Cb - kChromaOff<BITS>, cr = Cr - kChromaOff<BITS>;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int v = (q.iq[3 * c] * y + q.iq[3 * c + 1] * cb + q.iq[3 * c + 2] * cr + 32768) >> 16;
        v = v > 0 ? v : 0;
        rgb[c] = (unsigned)(v < kTop<BITS> ? v : kTop<BITS>);
    }
}

template <int BITS = 8>
__device__ __forceinline__ unsigned luma_of(const ResrYuvDesc& q, unsigned r, unsigned g, unsigned b) {
    return (unsigned)((q.fq[0] * (int)r + q.fq[1] * (int)g + q.fq[2] * (int)b + (kLumaOff<BITS> << 16) + 32768) >> 16) & (unsigned)kTop<BITS>;
}

// row = 1: Cb, row = 2: Cr; s: the sums of a 2x2 block's four pixels
template <int BITS = 8>
__device__ __forceinline__ unsigned chroma_of(const ResrYuvDesc& q, int row, const int (&s)[3]) {
    return (unsigned)((q.fq[3 * row] * s[0] + q.fq[3 * row + 1] * s[1] + q.fq[3 * row + 2] * s[2] + (kChromaOff<BITS> << 18) + (1 << 17)) >> 18) &
           (unsigned)kTop<BITS>;
}

// ---- image modes (include/resr.h: grey, RGB and RGBA images of 8 or 16 bits; frames.py holds the definition once more in numpy) ----

// cv2's fixed-point RGB2GRAY on integer levels: the coefficients sum to 2^14 (grey of (v, v, v) is v), the sum stays below 2^30 at 65535
__device__ __forceinline__ unsigned grey_of(const unsigned (&o)[3]) { return (4899u * o[0] + 9617u * o[1] + 1868u * o[2] + 8192u) >> 14; }

// The C levels of pixel p of an image batch [.,.,.,C]; an RGBA pixel is one load: a dword of four bytes, 8 bytes of four words.
template <int C, int BITS>
__device__ __forceinline__ void image_pixel(const typename Depth<BITS>::word* __restrict__ src, long p, unsigned (&lv)[4]) {
    if constexpr (C == 4 && BITS == 8) {
        const unsigned v = reinterpret_cast<const unsigned*>(src)[p];
#pragma unroll
        for (int c = 0; c < 4; ++c) lv[c] = (v >> (8 * c)) & 255u;
    } else if constexpr (C == 4) {
        const uint2 v = reinterpret_cast<const uint2*>(src)[p];
        lv[0] = v.x & 65535u; lv[1] = v.x >> 16; lv[2] = v.y & 65535u; lv[3] = v.y >> 16;
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) lv[c] = src[p * C + c];
    }
}

// A runtime image mode as a compile-time one, as with_scale: f(channels, bits), both std::integral_constant; false for any other mode.
template <typename F>
inline bool with_image_mode(const ResrImageDesc& m, F&& f) {
    auto depth = [&](auto C) {
        if (m.bits == 8) { f(C, std::integral_constant<int, 8>()); return true; }
        if (m.bits == 16) { f(C, std::integral_constant<int, 16>()); return true; }
        return false;
    };
    switch (m.channels) {
        case 1: return depth(std::integral_constant<int, 1>());
        case 3: return depth(std::integral_constant<int, 3>());
        case 4: return depth(std::integral_constant<int, 4>());
        default: return false;
    }
}

}  // namespace resr
