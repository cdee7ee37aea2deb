// frames.hip -- the frame path: images of integer levels in, images of integer levels out.
//
//   frame_head     : an image batch [N,H,W,C] (uint8 RGB frames: C = 3, bytes), or a YUV 4:2:0 frame [N,3H/2,W], -> the compact net's
//                    x_in [N,H,W,32] in the model's arithmetic (channels 3..31 zero): one kernel, the source of a pixel's RGB levels
//                    its parameter
//   compact_tail_image            : t [N,3S^2,H,W] fp32 + the input images -> images [N,H*S,W*S,C]   (pixel-shuffle + residual + quantise)
//   image_to_nchw, nchw_to_image  : images <-> fp32 [N,3,H,W]      (models whose first and last kernel are not ours to fuse: RRDB
//                                   Generator, the tiler); u8_to_nchw and nchw_to_u8 are their uint8 RGB entries
//   compact_tail_yuv              : the same tail with YUV 4:2:0 frames at both of its ends, of bytes or, as frame_head, of the
//                                   16-bit words of 10-bit samples (yuv420p10le / P010): one kernel, the layout of the source and
//                                   the layout of the destination its parameters (one format twice, or a mixed pair)
//   yuv420_to_rgb, rgb_to_yuv420  : the integer colour conversions on their own, u8 [N,3H/2,W] <-> u8 [N,H,W,3]
//   yuv420p10_to_nchw, nchw_to_yuv420p10: 10-bit YUV [N,3H/2,W] <-> fp32 [N,3,H,W], one launch each, no RGB frame in between
//   image modes                   : grey, RGB and RGBA images [N,H,W,C] of bytes or 16-bit words (255 or 65535 levels) at both ends; the
//                                   network's batch is the N colour or grey images, for RGBA the N alpha planes behind them, each level
//                                   thrice; grey and alpha leave through the fixed-point grey of their three levels.  uint8 RGB is the
//                                   (3, 8) mode (kRgb8): one template, one instance, under the profiling ids it has always had
//
// The result is DEFINED as what the float path followed by imgproc.tensor_to_image produces, bit for bit:
//   in : x = (float)u8 / 255.0f, one IEEE division (numpy's astype(float32) / 255.0), then converted to the model's type exactly
//        as nchw_to_nhwc_kernel converts a float (split_f16 / the rounding of common.h);
//   out: v = t + x (fp32, the single add of compact_tail_kernel; the generic kernel has no add), then v * 255.0f, clamp to
//        [0, 255], truncate -- in this order, nothing re-associated (t * 255 + x * 255 is another number).
// A NaN in v is outside the contract (the float path's astype(uint8) of a NaN is undefined too); here it quantises to 0.
// The YUV path is DEFINED as rgb_to_yuv420(the u8 path(yuv420_to_rgb(frame))), two integer functions of bytes (include/resr.h).
// The 10-bit YUV path is the same composition with 1023 levels: the integer functions with 64 / 512 / 1023 for 16 / 128 / 255,
// x = (float)rgb10 / 1023.0f on the way in and v * 1023.0f, clamp to [0, 1023], truncate on the way out (include/resr.h).
// The image modes are DEFINED as to_image(q(the float path(to_rgb(images) / top))) with top = 255 or 65535 (include/resr.h, "Image modes").
// Every index that can pass 2^31 is 64-bit.  Vector stores only.
#include "host_api.h"
#include "yuv.h"

namespace resr {

namespace {

// ---- YUV 4:2:0 (include/resr.h: the integer definition; frames.py holds it once more in numpy, which the tests compare with) ----

// (the integer conversions themselves: yuv.h, shared with the outscale tail of image_resize.hip)
// One dword of consecutive samples as their words, the first in the low bits (little-endian): four bytes, or two 16-bit words of a
// 10-bit layout.
template <int BITS = 8>
__device__ __forceinline__ unsigned pack_words(const unsigned* s, int layout = RESR_YUV_I420) {
    constexpr int WPD = 4 / (int)sizeof(typename Depth<BITS>::word);
    unsigned v = 0u;
#pragma unroll
    for (int i = 0; i < WPD; ++i) v |= word_of<BITS>(s[i], layout) << (32 / WPD * i);
    return v;
}

// Where frame_head_kernel and to_nchw_kernel take the three RGB levels of network pixel p from: a YUV 4:2:0 frame (images of luma
// size h x w; bytes, or 16-bit words of 10-bit samples: three 16-bit loads and a mask or a shift) yields them through the integer
// conversion, as levels of 255 or of 1023: `unit` is the division that goes with them.  (An image batch: ImageSrc, below.)
template <int BITS>
struct YuvSrc {
    const typename Depth<BITS>::word* __restrict__ src;
    int h, w;
    ResrYuvDesc q;
    __device__ __forceinline__ void operator()(long p, unsigned (&rgb)[3]) const {
        const long plane = (long)h * w;
        const long b = p / plane, r = p - b * plane;
        const int yy = (int)(r / w), xx = (int)(r - (long)yy * w);
        int Y, Cb, Cr;
        yuv_load<BITS>(src + b * (plane + (plane >> 1)), h, w, q.layout, yy, xx, Y, Cb, Cr);
        yuv_to_rgb<BITS>(q, Y, Cb, Cr, rgb);
    }
    static __device__ __forceinline__ float unit(unsigned v) { return unit_of<kTop<BITS>>(v); }
};

// One thread per 16-byte piece of an output pixel (as nchw_to_nhwc_kernel): only piece 0 holds the three real channels.
template <typename T, typename Src>
__global__ __launch_bounds__(256) void frame_head_kernel(Src src, T* __restrict__ dst, long px, long lo_off) {
    constexpr int E = 16 / (int)sizeof(T);
    constexpr int PIECES = 32 / E;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= px * PIECES) return;
    const long p = idx / PIECES;
    const int piece = (int)(idx - p * PIECES);
    uint4 out = make_uint4(0u, 0u, 0u, 0u), outl = make_uint4(0u, 0u, 0u, 0u);
    if (piece == 0) {
        unsigned rgb[3];
        src(p, rgb);
        T* o = reinterpret_cast<T*>(&out);
        T* ol = reinterpret_cast<T*>(&outl);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = Src::unit(rgb[c]);
            if constexpr (sizeof(T) == 2) {
                if (lo_off) split_f16(v, o[c], ol[c]);
                else o[c] = (T)v;
            } else {
                o[c] = (T)v;
            }
        }
    }
    *reinterpret_cast<uint4*>(dst + p * 32 + piece * E) = out;
    if (sizeof(T) == 2 && lo_off) *reinterpret_cast<uint4*>(dst + lo_off + p * 32 + piece * E) = outl;
}

// ---- image modes (include/resr.h: grey, RGB and RGBA images of 8 or 16 bits; frames.py holds the definition once more in numpy) ----

// (grey_of, image_pixel, with_image_mode: yuv.h, shared with the outscale tail of image_resize.hip)
// The other source of frame_head_kernel, an image batch of N images, `colour` = N * h * w pixels: network pixel p < colour is the colour of image pixel p (the grey
// level three times), network pixel p >= colour (RGBA only: the second N images of the network's batch) the alpha level of image pixel
// p - colour three times.  uint8 RGB frames are ImageSrc<3, 8>: three byte loads, a wavefront reads 192 contiguous bytes.
template <int C, int BITS>
struct ImageSrc {
    const typename Depth<BITS>::word* __restrict__ src;
    long colour;
    __device__ __forceinline__ void operator()(long p, unsigned (&rgb)[3]) const {
        const bool alpha = C == 4 && p >= colour;
        unsigned lv[4];
        image_pixel<C, BITS>(src, alpha ? p - colour : p, lv);
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = alpha ? lv[3] : C == 1 ? lv[0] : lv[c];
    }
    static __device__ __forceinline__ float unit(unsigned v) { return unit_of<kTop<BITS>>(v); }
};

// Output pixels a thread of the image tail owns: the fewest whose bytes are whole dwords, and a whole 16 bytes for RGBA
constexpr int image_group(int c, int bits) { return c == 1 ? 4 : 32 / bits; }
static_assert(image_group(1, 8) == 4 && image_group(1, 16) == 4 && image_group(3, 8) == 4 && image_group(3, 16) == 2 &&
              image_group(4, 8) == 4 && image_group(4, 16) == 2, "grey 4 pixels, 8-bit colour 4, 16-bit colour 2");

// The tail of every image mode, uint8 RGB frames (C = 3, BITS = 8) among them: t [planes * n, 3 S^2, h, w] fp32 + the input images
// x [n,h,w,C] -> y [n,hS,wS,C] of the same words.  The output is a flat array of n * hS * wS pixels; each pixel decodes its own (b, Y, X), and
// the 3 x S planes read for one (Y/S, X/S) are plane-strided but coalesced across lanes, as in compact_tail_kernel.  Per output pixel and channel v = t + unit(x level), quantise<top>(v): RGB stores the three levels; grey stores
// grey_of them (the residual is the grey level, thrice); RGBA stores the colour of image b's planes of t and, as the fourth word,
// grey_of the three levels of image n + b, whose residual is the alpha level.  A thread owns G = image_group consecutive output pixels
// = DW whole dwords, one store where DW is 1, 2 or 4 (grey8 a dword, grey16 8 bytes, RGBA 16 bytes) and three dword stores for RGB
// (12 bytes); y aligned to that store (compact_forward_ends / nchw_to_image_dispatch have checked it), a wavefront writes 64 * DW * 4
// contiguous bytes.  The last partial group falls back to single words.  RES = false, S = 1: the generic fp32 NCHW -> image conversion.
template <int S, int C, int BITS, bool RES>
__global__ __launch_bounds__(256) void compact_tail_image_kernel(const float* __restrict__ t, const typename Depth<BITS>::word* __restrict__ x,
                                                                 typename Depth<BITS>::word* __restrict__ y, int n, int h, int w) {
    typedef typename Depth<BITS>::word word;
    constexpr int TOP = kTop<BITS>, G = image_group(C, BITS), WPD = 32 / BITS, NW = G * C, DW = NW / WPD;
    static_assert(NW % WPD == 0 && (DW == 1 || DW == 2 || DW == 3 || DW == 4), "a group is 1 to 4 whole dwords");
    const int HS = h * S, WS = w * S;
    const long plane = (long)h * w;
    const long image = 3L * S * S * plane;     // floats of t per network image
    const long total = (long)n * HS * WS;
    const long q0 = ((long)blockIdx.x * 256 + threadIdx.x) * G;
    if (q0 >= total) return;
    const long row0 = q0 / WS;                 // b * HS + Y
    int X = (int)(q0 - row0 * WS);
    long b = row0 / HS;
    int Y = (int)(row0 - b * HS);
    unsigned words[NW];
#pragma unroll
    for (int k = 0; k < G; ++k) {
#pragma unroll
        for (int c = 0; c < C; ++c) words[k * C + c] = 0u;
        if (q0 + k < total) {
            const int yy = Y / S, sy = Y - yy * S, xx = X / S, sx = X - xx * S;
            unsigned lv[4] = {0u, 0u, 0u, 0u};
            if constexpr (RES) image_pixel<C, BITS>(x, (b * h + yy) * (long)w + xx, lv);
            const float* tp = t + (b * 3 * S * S + sy * S + sx) * plane + (long)yy * w + xx;
            unsigned o[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v = tp[(long)c * S * S * plane];
                if constexpr (RES) v = v + unit_of<TOP>(lv[C == 1 ? 0 : c]);
                o[c] = quantise<TOP>(v);
            }
            if constexpr (C == 1) {
                words[k] = grey_of(o);
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) words[k * C + c] = o[c];
            }
            if constexpr (C == 4) {
                const float* ta = tp + n * image;
                unsigned a[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float v = ta[(long)c * S * S * plane];
                    if constexpr (RES) v = v + unit_of<TOP>(lv[3]);
                    a[c] = quantise<TOP>(v);
                }
                words[k * 4 + 3] = grey_of(a);
            }
        }
        if (++X == WS) {
            X = 0;
            if (++Y == HS) { Y = 0; ++b; }
        }
    }
    word* out = y + q0 * C;
    if (q0 + G <= total) {
        unsigned dw[DW];
#pragma unroll
        for (int d = 0; d < DW; ++d) {
            dw[d] = 0u;
#pragma unroll
            for (int i = 0; i < WPD; ++i) dw[d] |= words[d * WPD + i] << (BITS * i);
        }
        if constexpr (DW == 1) *reinterpret_cast<unsigned*>(out) = dw[0];
        else if constexpr (DW == 2) *reinterpret_cast<uint2*>(out) = make_uint2(dw[0], dw[1]);
        else if constexpr (DW == 4) *reinterpret_cast<uint4*>(out) = make_uint4(dw[0], dw[1], dw[2], dw[3]);
        else {
#pragma unroll
            for (int d = 0; d < 3; ++d) reinterpret_cast<unsigned*>(out)[d] = dw[d];
        }
    } else {
        const int left = (int)(total - q0) * C;
#pragma unroll
        for (int i = 0; i < NW - C; ++i)
            if (i < left) out[i] = (word)words[i];
    }
}

// frames -> fp32 [.,3,H,W].  One thread per NETWORK pixel (an image batch: planes * n images): the pixel's levels through Src (an
// ImageSrc, or YuvSrc<10>: three 16-bit loads and the integer conversion), / top, one coalesced dword store per plane.
template <typename Src>
__global__ __launch_bounds__(256) void to_nchw_kernel(Src src, float* __restrict__ dst, long total, long plane) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    const long b = p / plane, r = p - b * plane;
    unsigned rgb[3];
    src(p, rgb);
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[(b * 3 + c) * plane + r] = Src::unit(rgb[c]);
}

// The image b, first row Y0 and first column X0 of the thread that owns 2 rows x COLS columns of n images of rows x cols pixels
// (rows even); false for a thread past the last such block.
template <int COLS>
__device__ __forceinline__ bool block_2xcols(int n, int rows, int cols, long& b, int& Y0, int& X0) {
    constexpr int SHIFT = COLS == 8 ? 3 : 2;
    static_assert(COLS == 1 << SHIFT, "4 or 8 columns");
    const int groups = (cols + COLS - 1) >> SHIFT;
    const long total = (long)n * (rows >> 1) * groups;
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return false;
    const long rp = gid / groups;              // b * rows / 2 + Y0 / 2
    X0 = (int)(gid - rp * groups) * COLS;
    b = rp / (rows >> 1);
    Y0 = (int)(rp - b * (rows >> 1)) * 2;
    return true;
}

// N sample words at p as one store of N words: 2, 4 or 8 bytes, p aligned to that.
template <int BITS, int N>
__device__ __forceinline__ void store_words(typename Depth<BITS>::word* p, const unsigned* s, int layout) {
    constexpr int WPD = 4 / (int)sizeof(typename Depth<BITS>::word);
    static_assert(N >= 2, "a single word is the narrow branch's");
    if constexpr (N * 2 == WPD) *reinterpret_cast<unsigned short*>(p) = (unsigned short)(s[0] | (s[1] << 8));
    else if constexpr (N == WPD) *reinterpret_cast<unsigned*>(p) = pack_words<BITS>(s, layout);
    else {
        static_assert(N == 2 * WPD, "2, 4 or 8 bytes");
        *reinterpret_cast<uint2*>(p) = make_uint2(pack_words<BITS>(s, layout), pack_words<BITS>(s + WPD, layout));
    }
}

// The 2 rows x COLS columns at (Y0, X0) of one 4:2:0 image (img; luma samples = rows x width, both even) from their samples: yb the
// two Y rows, cb / cr the COLS / 2 chroma samples.  wide (the caller's rule: every store below is aligned to its size): one store per
// Y row (COLS words), one of CbCr (COLS words; semi-planar) or one each of Cb and Cr (COLS / 2 words).  Else one sample word per store,
// the columns past the right edge skipped (rows always come in whole pairs).  Shared by the two generic writers, COLS = 4, whose
// registers it leaves as they were; compact_tail_yuv_kernel (COLS = 8, the layout a compile-time constant) keeps its stores in its own
// body: through this function five of its sixteen instances took one or two more VGPRs.
template <int BITS, int COLS>
__device__ __forceinline__ void store_yuv_block(typename Depth<BITS>::word* img, long luma, int width, int Y0, int X0, int layout, int wide,
                                                const unsigned (&yb)[2][COLS], const unsigned (&cb)[COLS / 2], const unsigned (&cr)[COLS / 2]) {
    typedef typename Depth<BITS>::word word;
    const bool semi = semi_planar(layout);
    word* row0 = img + (long)Y0 * width + X0;
    word* c0 = semi ? img + luma + (long)(Y0 >> 1) * width + X0 : img + luma + (long)(Y0 >> 1) * (width >> 1) + (X0 >> 1);
    if (wide) {
        store_words<BITS, COLS>(row0, yb[0], layout);
        store_words<BITS, COLS>(row0 + width, yb[1], layout);
        if (semi) {
            unsigned cc[COLS];
#pragma unroll
            for (int j = 0; j < COLS / 2; ++j) { cc[2 * j] = cb[j]; cc[2 * j + 1] = cr[j]; }
            store_words<BITS, COLS>(c0, cc, layout);
        } else {
            store_words<BITS, COLS / 2>(c0, cb, layout);
            store_words<BITS, COLS / 2>(c0 + (luma >> 2), cr, layout);
        }
    } else {
#pragma unroll
        for (int k = 0; k < COLS; ++k)
            if (X0 + k < width) {
                row0[k] = (word)word_of<BITS>(yb[0][k], layout);
                row0[width + k] = (word)word_of<BITS>(yb[1][k], layout);
            }
#pragma unroll
        for (int j = 0; j < COLS / 2; ++j)
            if (X0 + 2 * j < width) {
                if (semi) {
                    c0[2 * j] = (word)word_of<BITS>(cb[j], layout);
                    c0[2 * j + 1] = (word)word_of<BITS>(cr[j], layout);
                } else {
                    c0[j] = (word)word_of<BITS>(cb[j], layout);
                    c0[(luma >> 2) + j] = (word)word_of<BITS>(cr[j], layout);
                }
            }
    }
}

// compact_tail_image_kernel's job with YUV at both ends, of BITS = yuv_bits(LAYOUT) = 8 (bytes; RESR_YUV_I420 / RESR_YUV_NV12) or 10 bits per
// sample (16-bit words; RESR_YUV_I420P10 / RESR_YUV_P010).  A thread owns 2 rows x 8 columns of the output, i.e. four whole chroma
// samples; adjacent lanes are adjacent in x.  Per pixel: the residual level is recomputed from the YUV input (no RGB frame exists
// here), v = t + unit(rgb_in), quantise(v) unchanged (255 or 1023 levels), then the integer RGB -> YUV formula; the sums of the 2x2
// blocks stay in registers.  wide (the output width WS is a multiple of 8, y aligned to one Y store: then every plane row, both
// chroma bases and the per-image stride are aligned as the stores below need -- HS is even, so the luma plane is a
// multiple of 16 samples, a chroma row WS / 2 and a chroma plane HS / 2 * WS / 2 are multiples of 4, an image is 3 / 2 luma planes):
//   8 bits : two 8-byte Y stores and a dword each of Cb and Cr (I420) or one 8-byte CbCr store (NV12); a wavefront writes 512
//            contiguous bytes per Y row;
//   10 bits: two 16-byte Y stores and 8 bytes each of Cb and Cr (I420P10) or one 16-byte CbCr store (P010); 1 KiB per Y row.
// Every other even width: one sample word per store, the columns past the right edge skipped (rows always come in whole pairs).
// The two ends are separate: SRC is the layout of x (its word type, where its samples sit, and with qs.iq and unit_of<top of SRC> the
// residual level), LAYOUT that of y (quantise<top of LAYOUT>, qd.fq, the stores and the wide rule above).  SRC == LAYOUT with the same
// tables in qs and qd is the same-format path, instruction for instruction what it was with one descriptor; the twelve other pairs
// per S are the mixed tails (8 bits in and 10 out, NV12 in and I420 out, ...; BT.601 in and BT.709 out is a pair of tables, no instance).
template <int S, int SRC, int LAYOUT>
__global__ __launch_bounds__(256) void compact_tail_yuv_kernel(const float* __restrict__ t, const typename Depth<yuv_bits(SRC)>::word* __restrict__ x,
                                                               typename Depth<yuv_bits(LAYOUT)>::word* __restrict__ y, int n, int h, int w, int wide,
                                                               ResrYuvDesc qs, ResrYuvDesc qd) {
    constexpr int BITS = yuv_bits(LAYOUT), SBITS = yuv_bits(SRC);
    typedef typename Depth<BITS>::word word;
    const int HS = h * S, WS = w * S;
    long b;
    int Y0, X0;
    if (!block_2xcols<8>(n, HS, WS, b, Y0, X0)) return;
    const long plane = (long)h * w;
    const typename Depth<SBITS>::word* xin = x + b * (plane + (plane >> 1));
    const float* tb = t + b * 3 * S * S * plane;
    unsigned yb[2][8];
    int sum[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j) sum[j][0] = sum[j][1] = sum[j][2] = 0;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        // an even S keeps a row pair inside one LR row, a divisor of 8 keeps k / S a constant: the loads below then coincide
        const int yy = S % 2 == 0 ? Y0 / S : (Y0 + r) / S;
        const int sy = Y0 + r - yy * S;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int X = X0 + k;
            yb[r][k] = 0u;
            if (X < WS) {
                const int xx = 8 % S == 0 ? X0 / S + k / S : X / S;
                const int sx = X - xx * S;
                int Yi, Cb, Cr;
                yuv_load<SBITS>(xin, h, w, SRC, yy, xx, Yi, Cb, Cr);
                unsigned rgb_in[3], o[3];
                yuv_to_rgb<SBITS>(qs, Yi, Cb, Cr, rgb_in);
                const float* tp = tb + (long)(sy * S + sx) * plane + (long)yy * w + xx;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float v = tp[(long)c * S * S * plane] + unit_of<kTop<SBITS>>(rgb_in[c]);
                    o[c] = quantise<kTop<BITS>>(v);
                    sum[k >> 1][c] += (int)o[c];
                }
                yb[r][k] = luma_of<BITS>(qd, o[0], o[1], o[2]);
            }
        }
    }
    unsigned cb[4], cr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        cb[j] = chroma_of<BITS>(qd, 1, sum[j]);
        cr[j] = chroma_of<BITS>(qd, 2, sum[j]);
    }
    const long luma = (long)HS * WS;
    word* yo = y + b * (luma + (luma >> 1));
    word* row0 = yo + (long)Y0 * WS + X0;
    auto two = [](unsigned a0, unsigned a1) { return word_of<BITS>(a0, LAYOUT) | (word_of<BITS>(a1, LAYOUT) << 16); };
    word* c0 = semi_planar(LAYOUT) ? yo + luma + (long)(Y0 >> 1) * WS + X0 : yo + luma + (long)(Y0 >> 1) * (WS >> 1) + (X0 >> 1);
    if (wide) {
        if constexpr (BITS == 8) {
            *reinterpret_cast<uint2*>(row0) = make_uint2(pack_words<8>(yb[0]), pack_words<8>(yb[0] + 4));
            *reinterpret_cast<uint2*>(row0 + WS) = make_uint2(pack_words<8>(yb[1]), pack_words<8>(yb[1] + 4));
            if constexpr (semi_planar(LAYOUT)) {
                *reinterpret_cast<uint2*>(c0) =
                    make_uint2(cb[0] | (cr[0] << 8) | (cb[1] << 16) | (cr[1] << 24), cb[2] | (cr[2] << 8) | (cb[3] << 16) | (cr[3] << 24));
            } else {
                *reinterpret_cast<unsigned*>(c0) = pack_words<8>(cb);
                *reinterpret_cast<unsigned*>(c0 + (luma >> 2)) = pack_words<8>(cr);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 2; ++r)
                *reinterpret_cast<uint4*>(row0 + (long)r * WS) =
                    make_uint4(two(yb[r][0], yb[r][1]), two(yb[r][2], yb[r][3]), two(yb[r][4], yb[r][5]),
                               two(yb[r][6], yb[r][7]));
            if constexpr (semi_planar(LAYOUT)) {
                *reinterpret_cast<uint4*>(c0) =
                    make_uint4(two(cb[0], cr[0]), two(cb[1], cr[1]), two(cb[2], cr[2]), two(cb[3], cr[3]));
            } else {
                *reinterpret_cast<uint2*>(c0) = make_uint2(two(cb[0], cb[1]), two(cb[2], cb[3]));
                *reinterpret_cast<uint2*>(c0 + (luma >> 2)) = make_uint2(two(cr[0], cr[1]), two(cr[2], cr[3]));
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (X0 + k < WS) {
                row0[k] = (word)word_of<BITS>(yb[0][k], LAYOUT);
                row0[WS + k] = (word)word_of<BITS>(yb[1][k], LAYOUT);
            }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (X0 + 2 * j < WS) {
                if constexpr (semi_planar(LAYOUT)) {
                    c0[2 * j] = (word)word_of<BITS>(cb[j], LAYOUT);
                    c0[2 * j + 1] = (word)word_of<BITS>(cr[j], LAYOUT);
                } else {
                    c0[j] = (word)word_of<BITS>(cb[j], LAYOUT);
                    c0[(luma >> 2) + j] = (word)word_of<BITS>(cr[j], LAYOUT);
                }
            }
    }
}

// fp32 [N,3,H,W] (H, W even) -> 10-bit YUV [N,3H/2,W]: a thread owns 2 rows x 4 columns (two chroma samples), quantises its 8 pixels
// (v * 1023, clamp, truncate) and applies the integer formula.  wide (w a multiple of 4, src 16-byte and dst 8-byte aligned: then
// every row of every plane is): a 16-byte load per plane row, an 8-byte store per Y row, a dword each of Cb and Cr (I420P10) or 8
// bytes of CbCr (P010).  Every other even width moves single floats and words, the columns past the right edge skipped.
__global__ __launch_bounds__(256) void nchw_to_yuv420p10_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, int n, int h,
                                                                int w, int wide, ResrYuvDesc q) {
    long b;
    int Y0, X0;
    if (!block_2xcols<4>(n, h, w, b, Y0, X0)) return;
    const long plane = (long)h * w;
    unsigned yb[2][4];
    int sum[2][3] = {{0, 0, 0}, {0, 0, 0}};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const float* in = src + b * 3 * plane + (long)(Y0 + r) * w + X0;
        unsigned o[4][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (wide) {
                const float4 f = *reinterpret_cast<const float4*>(in + c * plane);
                v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (X0 + k < w) v[k] = in[c * plane + k];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k][c] = quantise<1023>(v[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            yb[r][k] = luma_of<10>(q, o[k][0], o[k][1], o[k][2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) sum[k >> 1][c] += (int)o[k][c];
        }
    }
    unsigned cb[2], cr[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        cb[j] = chroma_of<10>(q, 1, sum[j]);
        cr[j] = chroma_of<10>(q, 2, sum[j]);
    }
    store_yuv_block<10, 4>(dst + b * (plane + (plane >> 1)), plane, w, Y0, X0, q.layout, wide, yb, cb, cr);
}

// The generic conversions: a thread owns 2 rows x 4 columns (two chroma samples).  wide (w a multiple of 4, the HWC side 4-byte
// aligned): the 12 RGB bytes of a row are three dwords; the YUV side of rgb_to_yuv420 is a dword per Y row and a dword of CbCr
// (NV12) or two 2-byte stores (I420).  Every other even width moves bytes, the columns past the right edge skipped.
__global__ __launch_bounds__(256) void yuv420_to_rgb_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n, int h,
                                                            int w, int wide, ResrYuvDesc q) {
    long b;
    int Y0, X0;
    if (!block_2xcols<4>(n, h, w, b, Y0, X0)) return;
    const long plane = (long)h * w;
    const uint8_t* img = src + b * (plane + (plane >> 1));
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        unsigned bytes[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            unsigned rgb[3] = {0u, 0u, 0u};
            if (X0 + k < w) {
                int Y, Cb, Cr;
                yuv_load(img, h, w, q.layout, Y0 + r, X0 + k, Y, Cb, Cr);
                yuv_to_rgb(q, Y, Cb, Cr, rgb);
            }
            bytes[3 * k] = rgb[0];
            bytes[3 * k + 1] = rgb[1];
            bytes[3 * k + 2] = rgb[2];
        }
        uint8_t* o = dst + (b * plane + (long)(Y0 + r) * w + X0) * 3;
        if (wide) {
#pragma unroll
            for (int d = 0; d < 3; ++d) reinterpret_cast<unsigned*>(o)[d] = pack_words(bytes + 4 * d);
        } else {
            const int left = (w - X0 < 4 ? w - X0 : 4) * 3;
#pragma unroll
            for (int i = 0; i < 12; ++i)
                if (i < left) o[i] = (uint8_t)bytes[i];
        }
    }
}

__global__ __launch_bounds__(256) void rgb_to_yuv420_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n, int h,
                                                            int w, int wide, ResrYuvDesc q) {
    long b;
    int Y0, X0;
    if (!block_2xcols<4>(n, h, w, b, Y0, X0)) return;
    const long plane = (long)h * w;
    unsigned yb[2][4];
    int sum[2][3] = {{0, 0, 0}, {0, 0, 0}};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint8_t* in = src + (b * plane + (long)(Y0 + r) * w + X0) * 3;
        unsigned bytes[12];
        if (wide) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const unsigned v = reinterpret_cast<const unsigned*>(in)[d];
#pragma unroll
                for (int i = 0; i < 4; ++i) bytes[4 * d + i] = (v >> (8 * i)) & 255u;
            }
        } else {
            const int left = (w - X0 < 4 ? w - X0 : 4) * 3;
#pragma unroll
            for (int i = 0; i < 12; ++i) bytes[i] = i < left ? in[i] : 0u;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            yb[r][k] = luma_of(q, bytes[3 * k], bytes[3 * k + 1], bytes[3 * k + 2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) sum[k >> 1][c] += (int)bytes[3 * k + c];
        }
    }
    unsigned cb[2], cr[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        cb[j] = chroma_of(q, 1, sum[j]);
        cr[j] = chroma_of(q, 2, sum[j]);
    }
    store_yuv_block<8, 4>(dst + b * (plane + (plane >> 1)), plane, w, Y0, X0, q.layout, wide, yb, cb, cr);
}

bool grid_ok(long threads) { return threads > 0 && (threads + 255) / 256 <= 0x7fffffffL; }

// The refusals every YUV entry shares, in their order: a descriptor that is null or not of the entry's depth (bits = 0, the mixed
// entries: of no depth at all), then an odd frame.
int yuv_desc_check(const char* who, int h, int w, const ResrYuvDesc* q, int bits) {
    if (!q || !yuv_bits(q->layout) || (bits && yuv_bits(q->layout) != bits))
        return fail(RESR_ERR_ARG, "%s: the YUV descriptor is null or its layout is neither %s", who,
                    bits == 8 ? "RESR_YUV_I420 nor RESR_YUV_NV12" : bits ? "RESR_YUV_I420P10 nor RESR_YUV_P010" : "of these nor any other RESR_YUV_*");
    if ((h & 1) || (w & 1)) return fail(RESR_ERR_ARG, "%s: a 4:2:0 frame has an even height and width, got %dx%d", who, h, w);
    return RESR_OK;
}

// ... of the generic conversions, whose pointers and sizes come first; each dispatcher adds its own alignment rule
int yuv_frame_check(const char* who, const void* src, const void* dst, int n, int h, int w, const ResrYuvDesc* q, int bits) {
    if (!src || !dst || n <= 0 || h <= 0 || w <= 0) return fail(RESR_ERR_ARG, "%s: bad argument (n=%d h=%d w=%d)", who, n, h, w);
    return yuv_desc_check(who, h, w, q, bits);
}

// ---- image modes ----

long image_group_of(const ResrImageDesc* m) { return image_group(m->channels, m->bits); }
// The widest store of the tail (16 bytes of RGBA, 8 of 16-bit grey, else a dword) and the widest load of either end (an RGBA pixel is one
// load, every other level a word of its own): what y and x must be aligned to
size_t image_store_align(const ResrImageDesc* m) { return m->channels == 4 ? 16 : m->channels == 1 && m->bits == 16 ? 8 : 4; }
size_t image_load_align(const ResrImageDesc* m) { return (size_t)(m->channels == 4 ? m->bits / 2 : m->bits / 8); }

int image_desc_check(const char* who, const ResrImageDesc* m) {
    if (!m) return fail(RESR_ERR_ARG, "%s: null argument (the image descriptor)", who);
    if (m->channels != 1 && m->channels != 3 && m->channels != 4)
        return fail(RESR_ERR_ARG, "%s: channels must be 1 (grey), 3 (RGB) or 4 (RGBA), got %d", who, m->channels);
    if (m->bits != 8 && m->bits != 16) return fail(RESR_ERR_ARG, "%s: bits must be 8 or 16, got %d", who, m->bits);
    return RESR_OK;
}

int image_align_check(const char* who, const void* images_in, const void* images_out, const ResrImageDesc* m) {
    if (images_in && ((size_t)images_in & (image_load_align(m) - 1)) != 0)
        return fail(RESR_ERR_ARG, "%s: the source images must be %zu-byte aligned (%d channels of %d bits)", who, image_load_align(m), m->channels, m->bits);
    if (images_out && ((size_t)images_out & (image_store_align(m) - 1)) != 0)
        return fail(RESR_ERR_ARG, "%s: the output images must be %zu-byte aligned (%d channels of %d bits)", who, image_store_align(m), m->channels, m->bits);
    return RESR_OK;
}

// the pointers, the descriptor and the sizes of a generic conversion, in the order they are refused
int image_convert_check(const char* who, const void* src, const void* dst, int n_images, int h, int w, const ResrImageDesc* m) {
    if (!src || !dst) return fail(RESR_ERR_ARG, "%s: null argument", who);
    if (const int rc = image_desc_check(who, m)) return rc;
    if (n_images <= 0 || h <= 0 || w <= 0) return fail(RESR_ERR_ARG, "%s: bad argument (n_images=%d h=%d w=%d)", who, n_images, h, w);
    return RESR_OK;
}

template <int S, bool RES>
void launch_tail_image(const float* t, const void* x, void* y, int n, int h, int w, const ResrImageDesc* m, hipStream_t st) {
    const long groups = ((long)n * h * S * w * S + image_group_of(m) - 1) / image_group_of(m);
    with_image_mode(*m, [&](auto C, auto B) {
        typedef typename Depth<decltype(B)::value>::word word;
        hipLaunchKernelGGL((compact_tail_image_kernel<S, decltype(C)::value, decltype(B)::value, RES>), dim3((unsigned)((groups + 255) / 256)), dim3(256), 0,
                           st, t, (const word*)x, (word*)y, n, h, w);
    });
}

}  // namespace

// lo_off: the hi -> lo element offset of x_in (RESR_F16X2), as compact_forward passes it to nchw_to_nhwc_dispatch.
// q: the frames are YUV 4:2:0 [n,3h/2,w], of bytes or (a 10-bit layout) of 16-bit words.
// img (q null): the frames are images [n / planes,h,w,C] of that mode (image_forward_check has passed): the second half of an RGBA
// batch's n network images are the alpha planes.  Both null: uint8 RGB frames, the (3, 8) image mode.
int frame_head_dispatch(const void* src, void* dst, int n, int h, int w, int dtype, hipStream_t st, long lo_off, const ResrYuvDesc* q,
                        const ResrImageDesc* img) {
    if (!img && !q) img = &kRgb8;
    const int bits = q ? yuv_bits(q->layout) : 0;
    const bool ten = bits == 10;
    const char* who = ten ? "yuv10_head" : q ? "yuv_head" : image_id(img, 0, 1) ? "image_head" : "u8_head";
    if (!src || !dst || n <= 0 || h <= 0 || w <= 0 || (q && ((h & 1) || (w & 1) || !bits || img))) return fail(RESR_ERR_ARG, "%s: bad argument", who);
    const long px = (long)n * h * w;
    const int pieces = dtype != RESR_F32 ? 4 : 8;
    if (!grid_ok(px * pieces)) return fail(RESR_ERR_ARG, "%s: %ld pixels beyond the grid", who, px);
    const dim3 grid((unsigned)((px * pieces + 255) / 256));
    if (dtype != RESR_F16X2) lo_off = 0;
    auto launch = [&](auto from) {
        if (dtype != RESR_F32)
            hipLaunchKernelGGL((frame_head_kernel<half_t, decltype(from)>), grid, dim3(256), 0, st, from, (half_t*)dst, px, lo_off);
        else
            hipLaunchKernelGGL((frame_head_kernel<float, decltype(from)>), grid, dim3(256), 0, st, from, (float*)dst, px, 0L);
    };
    prof_before(st);
    if (ten) launch(YuvSrc<10>{(const uint16_t*)src, h, w, *q});
    else if (q) launch(YuvSrc<8>{(const uint8_t*)src, h, w, *q});
    else {
        const long colour = img->channels == 4 ? px / 2 : px;
        const bool ok = with_image_mode(*img, [&](auto C, auto B) {
            launch(ImageSrc<decltype(C)::value, decltype(B)::value>{(const typename Depth<decltype(B)::value>::word*)src, colour});
        });
        if (!ok) return fail(RESR_ERR_ARG, "%s: bad argument", who);
    }
    // an image pixel is read once per network pixel: an RGBA pixel twice, as colour and as alpha
    const double src_bytes = img ? img->channels * img->bits / 8.0 : ten ? 3.0 : 1.5;
    prof_after(st, ten ? 31022 : q ? 31021 : image_id(img, 31020, 31023), 0.0, (double)px * (src_bytes + 32.0 * (double)(elem_size(dtype) * act_tensors(dtype))));
    RESR_CHECK_LAUNCH("frame_head_kernel");
    return RESR_OK;
}

// ---- image modes ----

// Everything the image entry of compact_forward_ends has to refuse about its images, before its first launch.  n: the network's batch,
// planes * N.  The alignment rules are the widest load and store of the mode (image_load_align, image_store_align).
int image_forward_check(const char* who, int n, int h, int w, int s, const void* x, const void* y, const ResrImageDesc* img) {
    if (const int rc = image_desc_check(who, img)) return rc;
    if (img->channels == 4 && (n & 1))
        return fail(RESR_ERR_ARG, "%s: an RGBA batch is N colour images and N alpha images, the descriptor's n = %d is odd", who, n);
    if (const int rc = image_align_check(who, x, y, img)) return rc;
    const long out_px = (long)(img->channels == 4 ? n / 2 : n) * h * s * w * s, g = image_group_of(img);
    if (!grid_ok((out_px + g - 1) / g)) return fail(RESR_ERR_ARG, "%s: %dx%dx%d beyond the grid", who, n, h * s, w * s);
    return RESR_OK;
}

// x, y, n_images and img have passed image_forward_check: compact_forward_ends has called it.  Profiling id 31100 + s (uint8 RGB: 31010 + s).
int compact_tail_image(const float* t, const void* x, void* y, int n_images, int h, int w, int s, const ResrImageDesc* img, hipStream_t st) {
    prof_before(st);
    if (!with_scale(s, [&](auto S) { launch_tail_image<S(), true>(t, x, y, n_images, h, w, img, st); }))
        return fail(RESR_ERR_ARG, "compact_tail_image: upscale %d", s);
    // per LR pixel of a network image: 3 s^2 floats of t; per LR pixel of an image: its words in, s^2 times its words out
    const double pb = img->channels * img->bits / 8.0, planes = img->channels == 4 ? 2.0 : 1.0;
    prof_after(st, image_id(img, 31010, 31100) + s, 0.0, (double)n_images * h * w * (s * s * (12.0 * planes + pb) + pb));
    RESR_CHECK_LAUNCH("compact_tail_image_kernel");
    return RESR_OK;
}

namespace {

// The generic conversions once their entry (who) has checked its pointers, sizes and alignment: the grid, the launch, the mode's id
int image_to_nchw_launch(const char* who, const void* src, float* dst, int n_images, int h, int w, const ResrImageDesc* img, hipStream_t st) {
    const long plane = (long)h * w, colour = plane * n_images, total = img->channels == 4 ? 2 * colour : colour;
    if (!grid_ok(total)) return fail(RESR_ERR_ARG, "%s: %ld pixels beyond the grid", who, total);
    prof_before(st);
    with_image_mode(*img, [&](auto C, auto B) {
        typedef ImageSrc<decltype(C)::value, decltype(B)::value> Src;
        hipLaunchKernelGGL(to_nchw_kernel<Src>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                           Src{(const typename Depth<decltype(B)::value>::word*)src, colour}, dst, total, plane);
    });
    prof_after(st, image_id(img, 31030, 31036), 0.0, (double)total * (12.0 + img->channels * img->bits / 8.0));
    RESR_CHECK_LAUNCH("to_nchw_kernel");
    return RESR_OK;
}

int nchw_to_image_launch(const char* who, const float* src, void* dst, int n_images, int h, int w, const ResrImageDesc* img, hipStream_t st) {
    const long total = (long)n_images * h * w, g = image_group_of(img);
    if (!grid_ok((total + g - 1) / g)) return fail(RESR_ERR_ARG, "%s: %ld pixels beyond the grid", who, total);
    prof_before(st);
    launch_tail_image<1, false>(src, nullptr, dst, n_images, h, w, img, st);
    prof_after(st, image_id(img, 31031, 31037), 0.0, (double)total * ((img->channels == 4 ? 24.0 : 12.0) + img->channels * img->bits / 8.0));
    RESR_CHECK_LAUNCH("nchw_to_image_kernel");
    return RESR_OK;
}

}  // namespace

int image_to_nchw_dispatch(const void* src, float* dst, int n_images, int h, int w, const ResrImageDesc* img, hipStream_t st) {
    const char* who = "image_to_nchw";
    if (const int rc = image_convert_check(who, src, dst, n_images, h, w, img)) return rc;
    if (const int rc = image_align_check(who, src, nullptr, img)) return rc;
    if (((size_t)dst & 3) != 0) return fail(RESR_ERR_ARG, "%s: the float tensor must be 4-byte aligned", who);
    return image_to_nchw_launch(who, src, dst, n_images, h, w, img, st);
}

int nchw_to_image_dispatch(const float* src, void* dst, int n_images, int h, int w, const ResrImageDesc* img, hipStream_t st) {
    const char* who = "nchw_to_image";
    if (const int rc = image_convert_check(who, src, dst, n_images, h, w, img)) return rc;
    if (const int rc = image_align_check(who, nullptr, dst, img)) return rc;
    if (((size_t)src & 3) != 0) return fail(RESR_ERR_ARG, "%s: the float tensor must be 4-byte aligned", who);
    return nchw_to_image_launch(who, src, dst, n_images, h, w, img, st);
}

// The uint8-typed entries (include/resr.h: resr_u8_to_nchw, resr_nchw_to_u8): the (3, 8) image mode behind their own refusals.
int u8_to_nchw_dispatch(const uint8_t* src, float* dst, int n, int h, int w, hipStream_t st) {
    if (!src || !dst || n <= 0 || h <= 0 || w <= 0) return fail(RESR_ERR_ARG, "u8_to_nchw: bad argument (n=%d h=%d w=%d)", n, h, w);
    return image_to_nchw_launch("u8_to_nchw", src, dst, n, h, w, &kRgb8, st);
}

int nchw_to_u8_dispatch(const float* src, uint8_t* dst, int n, int h, int w, hipStream_t st) {
    if (!src || !dst || n <= 0 || h <= 0 || w <= 0) return fail(RESR_ERR_ARG, "nchw_to_u8: bad argument (n=%d h=%d w=%d)", n, h, w);
    if (((size_t)dst & 3) != 0) return fail(RESR_ERR_ARG, "nchw_to_u8: the output must be 4-byte aligned");
    return nchw_to_image_launch("nchw_to_u8", src, dst, n, h, w, &kRgb8, st);
}

// ---- YUV 4:2:0 ----

// Everything a YUV entry of compact_forward_ends has to refuse about its frames, before its first launch (d->h, d->w even: the
// output's are too).  bits: the entry's depth, 0 for the mixed entries (src and dst each of any depth; the same-format entries pass
// one descriptor twice).  The alignment of y is the wide store of the destination's depth (8 sample words) at an output width that
// is a multiple of 8, else one word.
int yuv_forward_check(const char* who, int n, int h, int w, int s, const void* y, const ResrYuvDesc* src, const ResrYuvDesc* dst, int bits) {
    if (const int rc = yuv_desc_check(who, h, w, src, bits)) return rc;
    if (dst != src)
        if (const int rc = yuv_desc_check(who, h, w, dst, bits)) return rc;
    const int word = yuv_bits(dst->layout) == 8 ? 1 : 2;
    if (((size_t)y & (size_t)(((w * s) % 8 == 0 ? 8 * word : word) - 1)) != 0)
        return fail(RESR_ERR_ARG, "%s: y_yuv must be %d-byte aligned at an output width of %d%s", who, 8 * word, w * s,
                    word > 1 ? " (2-byte at a width that is no multiple of 8)" : "");
    if (!grid_ok((long)n * (h * s / 2) * ((w * s + 7) / 8))) return fail(RESR_ERR_ARG, "%s: %dx%dx%d beyond the grid", who, n, h * s, w * s);
    return RESR_OK;
}

// the frames have passed yuv_forward_check: compact_forward_ends has called it.  x, y: bytes or 16-bit words, as qs->layout and
// qd->layout say.  Profiling ids name the instance: 31040 + s / 31060 + s where the two layouts are one (8 / 10 bits; another matrix
// on one side is the same instance), 31090 + s for the mixed tails.
// (31040 + s is also image_resize's 31040 + u8 at s = 1, u8 = 1: both are 31041.  Tests assert the values, so they stay.)
int compact_tail_yuv(const float* t, const void* x, void* y, int n, int h, int w, int s, const ResrYuvDesc* qs, const ResrYuvDesc* qd,
                     hipStream_t st) {
    const int wide = (w * s) % 8 == 0;
    const dim3 grid((unsigned)(((long)n * (h * s / 2) * ((w * s + 7) / 8) + 255) / 256));
    prof_before(st);
    const bool ok = with_scale(s, [&](auto S) {
        with_yuv_layout(qs->layout, [&](auto A) {
            with_yuv_layout(qd->layout, [&](auto L) {
                typedef typename Depth<yuv_bits(decltype(A)::value)>::word sword;
                typedef typename Depth<yuv_bits(decltype(L)::value)>::word word;
                hipLaunchKernelGGL((compact_tail_yuv_kernel<decltype(S)::value, decltype(A)::value, decltype(L)::value>), grid, dim3(256), 0, st, t,
                                   (const sword*)x, (word*)y, n, h, w, wide, *qs, *qd);
            });
        });
    });
    if (!ok) return fail(RESR_ERR_ARG, "compact_tail_yuv: upscale %d", s);
    // per LR pixel: 3 s^2 floats of t, 1.5 source words of x, 1.5 s^2 destination words out
    const bool ten = yuv_bits(qd->layout) == 10;
    const double wb = ten ? 2.0 : 1.0, sb = yuv_bits(qs->layout) == 10 ? 2.0 : 1.0;
    prof_after(st, (qs->layout != qd->layout ? 31090 : ten ? 31060 : 31040) + s, 0.0, (double)n * h * w * (s * s * (12.0 + 1.5 * wb) + 1.5 * sb));
    RESR_CHECK_LAUNCH("compact_tail_yuv_kernel");
    return RESR_OK;
}

// ---- the generic conversions ----

int yuv420p10_to_nchw_dispatch(const uint16_t* src, float* dst, int n, int h, int w, const ResrYuvDesc* q, hipStream_t st) {
    const char* who = "yuv420p10_to_nchw";
    if (const int rc = yuv_frame_check(who, src, dst, n, h, w, q, 10)) return rc;
    if ((((size_t)src & 1) | ((size_t)dst & 3)) != 0) return fail(RESR_ERR_ARG, "%s: 2-byte aligned frames, a 4-byte aligned float tensor", who);
    const long plane = (long)h * w, total = plane * n;
    if (!grid_ok(total)) return fail(RESR_ERR_ARG, "%s: %ld pixels beyond the grid", who, total);
    prof_before(st);
    hipLaunchKernelGGL(to_nchw_kernel<YuvSrc<10>>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, YuvSrc<10>{src, h, w, *q}, dst, total, plane);
    prof_after(st, 31034, 0.0, (double)total * 15.0);
    RESR_CHECK_LAUNCH("to_nchw_kernel");
    return RESR_OK;
}

int nchw_to_yuv420p10_dispatch(const float* src, uint16_t* dst, int n, int h, int w, const ResrYuvDesc* q, hipStream_t st) {
    const char* who = "nchw_to_yuv420p10";
    if (const int rc = yuv_frame_check(who, src, dst, n, h, w, q, 10)) return rc;
    const int wide = w % 4 == 0;
    if ((((size_t)src & (wide ? 15 : 3)) | ((size_t)dst & (wide ? 7 : 1))) != 0)
        return fail(RESR_ERR_ARG, "%s: at a width of %d the float tensor must be %d-byte and the frames %d-byte aligned", who, w, wide ? 16 : 4, wide ? 8 : 2);
    const long threads = (long)n * (h / 2) * ((w + 3) / 4);
    if (!grid_ok(threads)) return fail(RESR_ERR_ARG, "%s: %dx%dx%d beyond the grid", who, n, h, w);
    prof_before(st);
    hipLaunchKernelGGL(nchw_to_yuv420p10_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, src, dst, n, h, w, wide, *q);
    prof_after(st, 31035, 0.0, (double)n * h * w * 15.0);
    RESR_CHECK_LAUNCH("nchw_to_yuv420p10_kernel");
    return RESR_OK;
}

namespace {
int yuv420_convert_check(const char* who, const uint8_t* src, const uint8_t* dst, const uint8_t* hwc, int n, int h, int w,
                         const ResrYuvDesc* q) {
    if (const int rc = yuv_frame_check(who, src, dst, n, h, w, q, 8)) return rc;
    if (w % 4 == 0 && ((((size_t)dst | (size_t)hwc) & 3) != 0)) return fail(RESR_ERR_ARG, "%s: 4-byte aligned frames at a width of %d", who, w);
    if (!grid_ok((long)n * (h / 2) * ((w + 3) / 4))) return fail(RESR_ERR_ARG, "%s: %dx%dx%d beyond the grid", who, n, h, w);
    return RESR_OK;
}
}  // namespace

int yuv420_to_rgb_dispatch(const uint8_t* src, uint8_t* dst, int n, int h, int w, const ResrYuvDesc* q, hipStream_t st) {
    const int rc = yuv420_convert_check("yuv420_to_rgb", src, dst, dst, n, h, w, q);
    if (rc) return rc;
    const long threads = (long)n * (h / 2) * ((w + 3) / 4);
    prof_before(st);
    hipLaunchKernelGGL(yuv420_to_rgb_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, src, dst, n, h, w, (int)(w % 4 == 0), *q);
    prof_after(st, 31032, 0.0, (double)n * h * w * 4.5);
    RESR_CHECK_LAUNCH("yuv420_to_rgb_kernel");
    return RESR_OK;
}

int rgb_to_yuv420_dispatch(const uint8_t* src, uint8_t* dst, int n, int h, int w, const ResrYuvDesc* q, hipStream_t st) {
    const int rc = yuv420_convert_check("rgb_to_yuv420", src, dst, src, n, h, w, q);
    if (rc) return rc;
    const long threads = (long)n * (h / 2) * ((w + 3) / 4);
    prof_before(st);
    hipLaunchKernelGGL(rgb_to_yuv420_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, src, dst, n, h, w, (int)(w % 4 == 0), *q);
    prof_after(st, 31033, 0.0, (double)n * h * w * 4.5);
    RESR_CHECK_LAUNCH("rgb_to_yuv420_kernel");
    return RESR_OK;
}

}  // namespace resr
