// image_resize.hip -- the MATLAB-style antialiased bicubic resize of imgproc.image_resize as one tiled kernel, and the same
// kernel as the tail of the compact generator ("outscale": a final size that is not the network's own factor).
//
// DEFINITION.  For a model of factor s, an LR frame H x W and outscale o (a positive float, o != s):
//   sr  = model(x)                         fp32, not clamped: the float path
//   r   = o / s                            out_h = ceil(H * s * r), out_w = ceil(W * s * r)   (the reference's ceil(in * scale))
//   per axis a banded tap table            idx [out, P] int32, w [out, P] float32, P = ceil(4 / min(r, 1)) + 2: the non-zero band of
//                                          imgproc._resize_matrix with the symmetric reflection folded into idx, built on the host
//                                          in float32 (imgproc.resize_band_tables)
//   out = W-pass(H-pass(sr))               each pass acc = fmaf(v[idx[k]], w[k], acc) from acc = 0, k ascending, fp32; the
//                                          intermediate is fp32
//   u8  : out * 255.0f, clamp to [0, 255], truncate (imgproc.tensor_to_image, as everywhere on the frame path)
//
// KERNEL.  One workgroup of 256 threads per output tile (th x tw pixels, up to three channels).  It finds the source region its
// tile reads (rows min..max of the tile's idx_y entries by columns min..max of its idx_x entries), stages the tables and that
// region in LDS, runs the H pass LDS -> LDS (lanes along a source row: consecutive LDS words, no bank conflict whatever the row
// pitch), the W pass LDS -> registers (lanes along an output row: a stride of 1/r words, 2-way conflicts at r = 0.5; the pitch is
// odd so that the two rows a wavefront covers do not add to them) and stores.  resr_image_resize stages fp32 NCHW; the fused
// tail of resr_compact_forward_u8_scaled forms the staged value of HR pixel (Y, X), channel c, on the fly as
//   t[c*s*s + (Y%s)*s + X%s][Y/s][X/s] + x_u8[Y/s][X/s][c] / 255.0f        (the single fp32 add of compact_tail_image_kernel)
// so the HR frame exists as LDS tiles only.  Both call resize_tile(): fused and generic results are the same bits.
//
// The host picks the largest tile of a fixed list whose tables + region + intermediate (+ the u8 row buffer) stay within 64 KB:
// two workgroups or more per CU (160 KB of LDS) and no per-kernel LDS opt-in.  The region of t consecutive outputs is bounded by
// floor((t - 1) * in / (out - 1)) + 2 + P source pixels (the left tap moves 1/r < in / (out - 1) per output; reflection only
// folds the band inwards), at most `in`.  At r = 0.5 (P = 10) that is a 16 x 32 tile: 42 x 74 x 3 source floats + 16 x 74 x 3
// intermediate ~ 51 KB.  An r whose single-pixel footprint does not fit is RESR_ERR_ARG: there is no other path.
// A table entry outside the region bound (tables not built by the rule above) is clamped into it: never an access out of bounds.
// u8 rows leave as dword stores where the address is 4-byte aligned and byte stores at the row ends; every index that can pass
// 2^31 is 64-bit.  Vector stores only.
//
// YUV OUTSCALE.  The same tile with YUV 4:2:0 frames at both ends, 8 bits (I420 / NV12) or 10 (I420P10 / P010), the tail of
// resr_compact_forward_yuv420_scaled / _yuv420p10_scaled.  The staged value is t + unit(rgb_in), rgb_in the integer conversion of the
// YUV input pixel (yuv.h: what compact_tail_yuv of frames.hip adds; the input frames' own depth, layout and tables, which need not
// be the output's: resr_compact_forward_yuv420_mixed_scaled); after the W pass the three sums of a pixel are quantised to
// levels (255 or 1023) and staged in LDS as bytes or 16-bit words; after a barrier every Y row and every chroma row of the tile is
// written by the row writer of the image stage (dwords where the address is 4-byte aligned, single words at the row ends), each word
// formed on the fly from the staged levels: luma_of per pixel, chroma_of on the unrounded sum of a 2x2 block's four levels.  A
// thread owns a dword of an output row, not a block: adjacent lanes read adjacent staged pixels (a stride of 3 or 6 bytes per
// sample, odd in dwords: no bank conflict on the Y rows, 2-way on the chroma rows, whose lanes are two pixels apart) and write
// adjacent dwords; a block's levels are read once for Y and once per chroma plane, a few LDS reads against the 3 * taps of the W
// pass.  Tiles have an even height and width (resize_plan skips the odd entries of its list), so tile origins are even, the edge
// tile of an even output is even, and every chroma sample belongs to one workgroup.  The results are the compositions of
// include/resr.h bit for bit: the sums are those of the two stages above, the integer functions those of frames.hip.
//
// IMAGE-MODE OUTSCALE.  The same tile with an image batch [N,H,W,C] of bytes or 16-bit words at both ends (grey, RGB, RGBA; top = 255
// or 65535), the tail of resr_compact_forward_image_scaled.  The staged value is t + unit(level), the single add of
// compact_tail_image_kernel (frames.hip): the level is the image's own channel, the grey level thrice, or -- for the second half of an
// RGBA batch's network images -- the alpha word thrice; the pixel is read with image_pixel, an RGBA pixel as one load.  After the W pass
// the three sums of a pixel are quantised to levels of top and staged in LDS as C words per pixel: RGB the three levels, grey grey_of
// them, RGBA the three colour levels and one alpha word.  RGBA is ONE workgroup per output tile (two would each write part of a dword):
// it stages its tables once, runs region, H pass, W pass and quantisation for colour image b, then the same steps for alpha image N + b
// over the same region and the same LDS, takes grey_of the alpha levels into the fourth word, and stores; grid.z is N.  After a
// barrier a tile row leaves as tw * C contiguous words through store_row_slot.  uint8 RGB frames are the (3, 8) mode.  Tiles may be odd, as for uint8.  The
// sums are resize_tile's per channel and do not depend on the tile, so the result is to_image(resr_image_resize(float path)) bit for bit.
#include <limits.h>

#include "host_api.h"
#include "yuv.h"

namespace resr {

namespace {

constexpr int kResizeThreads = 256;
constexpr size_t kResizeLdsBudget = 64 * 1024;
constexpr int kResizeMaxTaps = 4096;

// What resize_tile stores: fp32 [N,C,oh,ow], a YUV 4:2:0 frame [N,3oh/2,ow] of BITS-bit samples in LAYOUT ...
struct OutF32 { static constexpr int kind = RESIZE_F32; };
template <int BITS, int LAYOUT>
struct OutYuv {
    static constexpr int kind = BITS == 8 ? RESIZE_YUV8 : RESIZE_YUV10;
    static constexpr int bits = BITS, layout = LAYOUT;
    const ResrYuvDesc* q;
};
// ... or an image batch [N,oh,ow,C] of bytes or 16-bit words, n = N images: grey and alpha leave through grey_of their three levels
// (uint8 RGB frames [N,oh,ow,3] are OutImage<3, 8>, whose kind is RESIZE_U8)
template <int C, int BITS>
struct OutImage {
    static constexpr int kind = resize_image_kind(C, BITS);
    static constexpr int channels = C, bits = BITS;
    int n;
};
// network images a workgroup of that output stage runs: the colour and the alpha image of an RGBA tile, else one
template <typename Out>
constexpr int image_planes() {
    if constexpr (resize_is_image(Out::kind)) return Out::channels == 4 ? 2 : 1;
    else return 1;
}

// fp32 [N,C,H,W]
struct PlanarSrc {
    static constexpr bool kTriple = false;
    const float* x;
    int c, h, w;
    __device__ __forceinline__ float load(long b, int ch, int Y, int X) const {
        return x[((b * c + ch) * h + Y) * (long)w + X];
    }
};

// The compact net's last conv t [N,3S^2,h,w] under pixel-shuffle: HR pixel (Y, X) of network image b is LR pixel (yy, xx), and its
// channel c the float at the returned pointer + c * S * S * h * w.  The one decode of the fused tails' sources below.
template <int S>
__device__ __forceinline__ const float* shuffle_decode(const float* t, int h, int w, long b, int Y, int X, int& yy, int& xx) {
    yy = Y / S;
    xx = X / S;
    const int sy = Y - yy * S, sx = X - xx * S;
    const long plane = (long)h * w;
    return t + (b * 3 * S * S + sy * S + sx) * plane + (long)yy * w + xx;
}

// t + the residual of its YUV 4:2:0 input frames [N,3h/2,w] of BITS-bit samples: the level of an LR pixel is the integer conversion
// of its three samples, so the three channels of HR pixel (Y, X) come together (kTriple: load3 in place of load)
template <int S, int BITS, int LAYOUT>
struct YuvShuffleSrc {
    static constexpr bool kTriple = true;
    const float* t;
    const typename Depth<BITS>::word* x;
    int h, w;             // LR
    ResrYuvDesc q;
    __device__ __forceinline__ void load3(long b, int Y, int X, float (&v)[3]) const {
        int yy, xx;
        const float* tp = shuffle_decode<S>(t, h, w, b, Y, X, yy, xx);
        const long plane = (long)h * w;
        int Yi, Cb, Cr;
        yuv_load<BITS>(x + b * (plane + (plane >> 1)), h, w, LAYOUT, yy, xx, Yi, Cb, Cr);
        unsigned rgb_in[3];
        yuv_to_rgb<BITS>(q, Yi, Cb, Cr, rgb_in);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = tp[(long)c * S * S * plane] + unit_of<kTop<BITS>>(rgb_in[c]);
    }
};

// t + the residual of its input images [n,h,w,C] of bytes or 16-bit words (frames.hip, image modes; uint8 RGB frames are C = 3, BITS = 8): the
// residual level of network image b < n is the colour of image b (the grey level three times), that of network image b >= n (RGBA
// only) the alpha word of image b - n three times.  The pixel is read with image_pixel, so an RGBA pixel stays one load.
template <int S, int C, int BITS>
struct ImageShuffleSrc {
    static constexpr bool kTriple = true;
    const float* t;
    const typename Depth<BITS>::word* x;
    int h, w;             // LR
    int n;                // images: the network's batch is n (RGBA: 2 n)
    __device__ __forceinline__ void load3(long b, int Y, int X, float (&v)[3]) const {
        int yy, xx;
        const float* tp = shuffle_decode<S>(t, h, w, b, Y, X, yy, xx);
        const long plane = (long)h * w;
        const bool alpha = C == 4 && b >= n;
        unsigned lv[4];
        image_pixel<C, BITS>(x, ((alpha ? b - n : b) * h + yy) * (long)w + xx, lv);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = tp[(long)c * S * S * plane] + unit_of<kTop<BITS>>(alpha ? lv[3] : C == 1 ? lv[0] : lv[c]);
    }
};

// Slot j of a row of `len` words that starts at gp (word-aligned): slot 0 writes the words before the first 4-byte boundary, slot
// j >= 1 one dword (or, at the row's end, the words that are left); at(k) is word k of the row.  len / WPD + 2 slots cover a row.
template <typename word, typename At>
__device__ __forceinline__ void store_row_slot(word* __restrict__ gp, int len, int j, At&& at) {
    constexpr int WPD = 4 / (int)sizeof(word);
    const int head = min((int)(((4 - ((size_t)gp & 3)) & 3) / sizeof(word)), len);
    if (j == 0) {
        for (int k = 0; k < head; ++k) gp[k] = (word)at(k);
    } else {
        const int off = head + WPD * (j - 1);
        if (off + WPD <= len) {
            unsigned v = 0u;
#pragma unroll
            for (int i = 0; i < WPD; ++i) v |= (unsigned)at(off + i) << (8 * (int)sizeof(word) * i);
            *reinterpret_cast<unsigned*>(gp + off) = v;
        } else {
            for (int k = off; k < len; ++k) gp[k] = (word)at(k);
        }
    }
}

// The W pass of output (c, ty, tx) of a tile, LDS -> a register: THE definition of that pass for every output stage -- acc from 0, the
// taps in ascending order, one fmaf each, fp32.  s_mid: the H pass's result; s_ix, s_wx: the tile's region-relative column tables.
__device__ __forceinline__ float w_pass(const float* s_mid, const int* s_ix, const float* s_wx, const ResizeGeom& g, int c, int ty, int tx) {
    const float* row = s_mid + (c * g.th + ty) * g.pitch;
    const int* ix = s_ix + tx * g.px;
    const float* wx = s_wx + tx * g.px;
    float acc = 0.f;
    for (int k = 0; k < g.px; ++k) acc = fmaf(row[ix[k]], wx[k], acc);
    return acc;
}

// The whole tile: region bounds, staging, both passes, quantisation and stores.  y: fp32 [N,C,oh,ow], a YUV 4:2:0 frame
// [N,3oh/2,ow] or an image batch [N,oh,ow,C] (Out).
template <typename Src, typename Out>
__device__ __forceinline__ void resize_tile(const Src& src, const Out& out, void* __restrict__ y, const int32_t* __restrict__ idx_y,
                                            const float* __restrict__ w_y, const int32_t* __restrict__ idx_x,
                                            const float* __restrict__ w_x, const ResizeGeom& g) {
    extern __shared__ __attribute__((aligned(16))) char resize_smem[];
    __shared__ int s_bounds[4];
    const int tid = threadIdx.x;
    const int ox0 = blockIdx.x * g.tw, oy0 = blockIdx.y * g.th;
    const int th = min(g.th, g.oh - oy0), tw = min(g.tw, g.ow - ox0);
    const long b = blockIdx.z / g.cgroups;
    const int c0 = (int)(blockIdx.z - b * g.cgroups) * 3;
    const int nc = min(3, g.c - c0);

    int* s_iy = reinterpret_cast<int*>(resize_smem);
    float* s_wy = reinterpret_cast<float*>(s_iy + g.th * g.py);
    int* s_ix = reinterpret_cast<int*>(s_wy + g.th * g.py);
    float* s_wx = reinterpret_cast<float*>(s_ix + g.tw * g.px);
    float* s_src = s_wx + g.tw * g.px;
    float* s_mid = s_src + 3 * g.rh * g.pitch;
    uint8_t* s_out = reinterpret_cast<uint8_t*>(s_mid + 3 * g.th * g.pitch);

    // ---- the region this tile reads -----------------------------------------------------------------------------------------
    if (tid == 0) { s_bounds[0] = INT_MAX; s_bounds[1] = INT_MIN; s_bounds[2] = INT_MAX; s_bounds[3] = INT_MIN; }
    __syncthreads();
    {
        int lo = INT_MAX, hi = INT_MIN;
        const int32_t* p = idx_y + (long)oy0 * g.py;
        for (int i = tid; i < th * g.py; i += kResizeThreads) { const int v = p[i]; lo = min(lo, v); hi = max(hi, v); }
        if (lo <= hi) { atomicMin(&s_bounds[0], lo); atomicMax(&s_bounds[1], hi); }
        lo = INT_MAX; hi = INT_MIN;
        p = idx_x + (long)ox0 * g.px;
        for (int i = tid; i < tw * g.px; i += kResizeThreads) { const int v = p[i]; lo = min(lo, v); hi = max(hi, v); }
        if (lo <= hi) { atomicMin(&s_bounds[2], lo); atomicMax(&s_bounds[3], hi); }
    }
    __syncthreads();
    const int ymin = min(max(s_bounds[0], 0), g.h - 1), xmin = min(max(s_bounds[2], 0), g.w - 1);
    const int rh = min(min(max(s_bounds[1], ymin), g.h - 1) - ymin + 1, g.rh);
    const int rw = min(min(max(s_bounds[3], xmin), g.w - 1) - xmin + 1, g.rw);

    // ---- tables (region-relative, clamped into the region) and the region itself ----------------------------------------------
    for (int i = tid; i < th * g.py; i += kResizeThreads) {
        s_iy[i] = min(max(idx_y[(long)oy0 * g.py + i] - ymin, 0), rh - 1);
        s_wy[i] = w_y[(long)oy0 * g.py + i];
    }
    for (int i = tid; i < tw * g.px; i += kResizeThreads) {
        s_ix[i] = min(max(idx_x[(long)ox0 * g.px + i] - xmin, 0), rw - 1);
        s_wx[i] = w_x[(long)ox0 * g.px + i];
    }
    // (an RGBA image runs from here to its quantised levels twice, over the same region and LDS: colour image b, then alpha image n + b;
    // every other kind once)
    constexpr int kPlanes = image_planes<Out>();
    const int region = rh * rw;
    for (int pl = 0; pl < kPlanes; ++pl) {
        long bn = b;
        if constexpr (kPlanes > 1) bn += (long)pl * out.n;
        if constexpr (Src::kTriple) {
            for (int i = tid; i < region; i += kResizeThreads) {
                const int ry = i / rw, rx = i - ry * rw;
                float v[3];
                src.load3(bn, ymin + ry, xmin + rx, v);
#pragma unroll
                for (int c = 0; c < 3; ++c) s_src[(c * g.rh + ry) * g.pitch + rx] = v[c];
            }
        } else {
            for (int c = 0; c < nc; ++c)
                for (int i = tid; i < region; i += kResizeThreads) {
                    const int ry = i / rw, rx = i - ry * rw;
                    s_src[(c * g.rh + ry) * g.pitch + rx] = src.load(bn, c0 + c, ymin + ry, xmin + rx);
                }
        }
        __syncthreads();   // (the second time round this also ends the first W pass, which read the s_mid that the H pass below overwrites)

        // ---- H pass: LDS -> LDS ---------------------------------------------------------------------------------------------------
        const int mid = th * rw;
        for (int c = 0; c < nc; ++c)
            for (int i = tid; i < mid; i += kResizeThreads) {
                const int ty = i / rw, col = i - ty * rw;
                const float* col_p = s_src + c * g.rh * g.pitch + col;
                const int* iy = s_iy + ty * g.py;
                const float* wy = s_wy + ty * g.py;
                float acc = 0.f;
                for (int k = 0; k < g.py; ++k) acc = fmaf(col_p[iy[k] * g.pitch], wy[k], acc);
                s_mid[(c * g.th + ty) * g.pitch + col] = acc;
            }
        __syncthreads();

        // ---- an image mode's W pass: LDS -> registers -> the levels of the tile in LDS, pixel by pixel as C words (RGB: the three levels;
        // grey: grey_of them; RGBA: the colour levels, then grey_of the alpha image's as the fourth word -- a thread fills the fourth word
        // of the pixels whose colour it wrote) ------------------------------------------------------------------------------------------
        if constexpr (resize_is_image(Out::kind)) {
            constexpr int C = Out::channels;
            typedef typename Depth<Out::bits>::word word;
            word* s_lv = reinterpret_cast<word*>(s_out);
            const int outs = th * tw;
            for (int i = tid; i < outs; i += kResizeThreads) {
                const int ty = i / tw, tx = i - ty * tw;
                unsigned o[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c] = quantise<kTop<Out::bits>>(w_pass(s_mid, s_ix, s_wx, g, c, ty, tx));
                if constexpr (C == 1) {
                    s_lv[i] = (word)grey_of(o);
                } else if (pl) {
                    s_lv[i * C + 3] = (word)grey_of(o);
                } else {
#pragma unroll
                    for (int c = 0; c < 3; ++c) s_lv[i * C + c] = (word)o[c];
                }
            }
        }
    }

    // ---- W pass: LDS -> registers, store --------------------------------------------------------------------------------------
    if constexpr (Out::kind == RESIZE_F32) {
        float* yf = reinterpret_cast<float*>(y);
        const int outs = th * tw;
        for (int c = 0; c < nc; ++c)
            for (int i = tid; i < outs; i += kResizeThreads) {
                const int ty = i / tw, tx = i - ty * tw;
                yf[((b * g.c + c0 + c) * g.oh + oy0 + ty) * (long)g.ow + ox0 + tx] = w_pass(s_mid, s_ix, s_wx, g, c, ty, tx);
            }
    } else if constexpr (resize_is_image(Out::kind)) {
        constexpr int C = Out::channels;
        typedef typename Depth<Out::bits>::word word;
        constexpr int WPD = 4 / (int)sizeof(word);
        const word* s_lv = reinterpret_cast<const word*>(s_out);
        __syncthreads();
        // a tile row is tw * C contiguous words of y
        word* yw = reinterpret_cast<word*>(y);
        const int len = tw * C;
        const int slots = len / WPD + 2;
        for (int i = tid; i < th * slots; i += kResizeThreads) {
            const int ty = i / slots, j = i - ty * slots;
            const word* sp = s_lv + ty * len;
            store_row_slot(yw + ((b * g.oh + oy0 + ty) * (long)g.ow + ox0) * C, len, j, [&](int k) { return sp[k]; });
        }
    } else {
        // YUV 4:2:0 (th, tw, oy0, ox0, g.oh, g.ow all even): the levels of the tile, pixel by pixel as (R, G, B) words
        constexpr int BITS = Out::bits, LAYOUT = Out::layout;
        typedef typename Depth<BITS>::word word;
        constexpr int WPD = 4 / (int)sizeof(word);
        const ResrYuvDesc& q = *out.q;
        word* s_lv = reinterpret_cast<word*>(s_out);
        const int outs = th * tw;
        for (int i = tid; i < outs; i += kResizeThreads) {
            const int ty = i / tw, tx = i - ty * tw;
#pragma unroll
            for (int c = 0; c < 3; ++c) s_lv[i * 3 + c] = (word)quantise<kTop<BITS>>(w_pass(s_mid, s_ix, s_wx, g, c, ty, tx));
        }
        __syncthreads();
        const long luma = (long)g.oh * g.ow;
        word* img = reinterpret_cast<word*>(y) + b * (luma + (luma >> 1));
        // a tile row of Y is tw contiguous words of the frame
        const int slots = tw / WPD + 2;
        for (int i = tid; i < th * slots; i += kResizeThreads) {
            const int ty = i / slots, j = i - ty * slots;
            const word* lv = s_lv + ty * tw * 3;
            store_row_slot(img + (long)(oy0 + ty) * g.ow + ox0, tw, j, [&](int k) {
                return word_of<BITS>(luma_of<BITS>(q, lv[3 * k], lv[3 * k + 1], lv[3 * k + 2]), LAYOUT);
            });
        }
        // the sums of block (cy, bx) of the tile: its four pixels' levels, unrounded
        auto block_sum = [&](int cy, int bx, int (&sum)[3]) {
            const word* p0 = s_lv + (2 * cy * tw + 2 * bx) * 3;
            const word* p1 = p0 + tw * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) sum[c] = (int)p0[c] + (int)p0[3 + c] + (int)p1[c] + (int)p1[3 + c];
        };
        if constexpr (semi_planar(LAYOUT)) {   // a tile row of CbCr pairs is tw contiguous words as well
            for (int i = tid; i < (th >> 1) * slots; i += kResizeThreads) {
                const int cy = i / slots, j = i - cy * slots;
                store_row_slot(img + luma + (long)((oy0 >> 1) + cy) * g.ow + ox0, tw, j, [&](int k) {
                    int sum[3];
                    block_sum(cy, k >> 1, sum);
                    const unsigned cb = chroma_of<BITS>(q, 1, sum), cr = chroma_of<BITS>(q, 2, sum);
                    return word_of<BITS>((k & 1) ? cr : cb, LAYOUT);
                });
            }
        } else {                               // ... of the Cb plane and of the Cr plane tw / 2
            const int cslots = (tw >> 1) / WPD + 2;
#pragma unroll
            for (int pl = 0; pl < 2; ++pl)
                for (int i = tid; i < (th >> 1) * cslots; i += kResizeThreads) {
                    const int cy = i / cslots, j = i - cy * cslots;
                    store_row_slot(img + luma + pl * (luma >> 2) + (long)((oy0 >> 1) + cy) * (g.ow >> 1) + (ox0 >> 1), tw >> 1, j, [&](int k) {
                        int sum[3];
                        block_sum(cy, k, sum);
                        return word_of<BITS>(chroma_of<BITS>(q, 1 + pl, sum), LAYOUT);
                    });
                }
        }
    }
}

template <bool U8>
__global__ __launch_bounds__(kResizeThreads) void image_resize_kernel(PlanarSrc src, void* __restrict__ y, const int32_t* __restrict__ idx_y,
                                                                      const float* __restrict__ w_y, const int32_t* __restrict__ idx_x,
                                                                      const float* __restrict__ w_x, ResizeGeom g) {
    resize_tile(src, std::conditional_t<U8, OutImage<3, 8>, OutF32>(), y, idx_y, w_y, idx_x, w_x, g);
}

// SRC: the layout of the input frames (the staged value is t + level / top of SRC, src.q the source's tables), LAYOUT that of the
// output stage (qd: the destination's).  SRC == LAYOUT with the same tables twice is the same-format tail; the other pairs are the
// mixed ones (frames.hip, compact_tail_yuv_kernel).
template <int S, int SRC, int LAYOUT>
__global__ __launch_bounds__(kResizeThreads) void compact_tail_yuv_scaled_kernel(YuvShuffleSrc<S, yuv_bits(SRC), SRC> src, ResrYuvDesc qd,
                                                                                 void* __restrict__ y, const int32_t* __restrict__ idx_y,
                                                                                 const float* __restrict__ w_y, const int32_t* __restrict__ idx_x,
                                                                                 const float* __restrict__ w_x, ResizeGeom g) {
    resize_tile(src, OutYuv<yuv_bits(LAYOUT), LAYOUT>{&qd}, y, idx_y, w_y, idx_x, w_x, g);
}

// The image modes' tail: grid.z = n images (an RGBA workgroup runs both of its network images: resize_tile)
template <int S, int C, int BITS>
__global__ __launch_bounds__(kResizeThreads) void compact_tail_image_scaled_kernel(ImageShuffleSrc<S, C, BITS> src, void* __restrict__ y,
                                                                                   const int32_t* __restrict__ idx_y, const float* __restrict__ w_y,
                                                                                   const int32_t* __restrict__ idx_x, const float* __restrict__ w_x,
                                                                                   ResizeGeom g) {
    resize_tile(src, OutImage<C, BITS>{src.n}, y, idx_y, w_y, idx_x, w_x, g);
}

// source pixels that t consecutive outputs of an axis (in -> out pixels, p taps) can reach
int span_bound(int t, int in, int out, int p) {
    long s = p;
    if (t > 1) s += (long)(t - 1) * in / (out - 1) + 2;
    return (int)(s < in ? s : in);
}

// tables + region + intermediate + the staging buffer of the output stage: three bytes (RESIZE_YUV8), three 16-bit words
// (RESIZE_YUV10) or the C words of an image mode (RESIZE_U8: three bytes) per pixel of the tile
size_t lds_bytes(const ResizeGeom& g, int out) {
    size_t floats = 2 * ((size_t)g.th * g.py + (size_t)g.tw * g.px) + 3 * ((size_t)g.rh + g.th) * g.pitch;
    const size_t pixel = out == RESIZE_F32 ? 0 : resize_is_image(out) ? resize_image_channels(out) * resize_image_word_bytes(out) : out == RESIZE_YUV10 ? 6 : 3;
    return floats * 4 + align_up((size_t)g.th * g.tw * pixel, 4);
}

// The largest tile of the list whose LDS fits the budget (g: everything but th, tw, rh, rw, pitch); a YUV 4:2:0 output takes the
// tiles of even height and width only (an image mode any, as uint8).  false: none fits.
bool choose_tile(ResizeGeom& g, int out) {
    static const int tiles[][2] = {{32, 32}, {16, 32}, {16, 16}, {8, 16}, {8, 8}, {4, 8}, {4, 4}, {2, 4}, {2, 2}, {1, 2}, {1, 1}};
    const bool yuv = out == RESIZE_YUV8 || out == RESIZE_YUV10;
    for (const auto& t : tiles) {
        if (yuv && ((t[0] | t[1]) & 1)) continue;
        g.th = t[0]; g.tw = t[1];
        g.rh = span_bound(g.th < g.oh ? g.th : g.oh, g.h, g.oh, g.py);
        g.rw = span_bound(g.tw < g.ow ? g.tw : g.ow, g.w, g.ow, g.px);
        g.pitch = g.rw | 1;
        if (lds_bytes(g, out) <= kResizeLdsBudget) return true;
    }
    return false;
}

}  // namespace

// Every check of a resize launch and the choice of its tile: no device work.  c, h, w: the source; who: the entry's name.
int resize_plan(const char* who, int n, int c, int h, int w, int oh, int ow, const void* idx_y, const void* w_y, int taps_y,
                const void* idx_x, const void* w_x, int taps_x, int kind, const void* y, ResizeGeom* out) {
    const bool yuv = kind == RESIZE_YUV8 || kind == RESIZE_YUV10, u8 = kind == RESIZE_U8, image = resize_is_image(kind);
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0)
        return fail(RESR_ERR_ARG, "%s: bad shape (n=%d c=%d h=%d w=%d oh=%d ow=%d)", who, n, c, h, w, oh, ow);
    if (!idx_y || !w_y || !idx_x || !w_x) return fail(RESR_ERR_ARG, "%s: null tap table", who);
    if (taps_y < 1 || taps_y > kResizeMaxTaps || taps_x < 1 || taps_x > kResizeMaxTaps)
        return fail(RESR_ERR_ARG, "%s: taps %d, %d outside [1, %d]", who, taps_y, taps_x, kResizeMaxTaps);
    if (yuv && (c != 3 || ((oh | ow) & 1))) return fail(RESR_ERR_ARG, "%s: a 4:2:0 output wants 3 channels and an even height and width, got %d, %dx%d", who, c, oh, ow);
    if (yuv && ((size_t)y & 3) != 0) return fail(RESR_ERR_ARG, "%s: the YUV output must be 4-byte aligned", who);
    if (image && c != 3) return fail(RESR_ERR_ARG, "%s: %s output wants 3 channels, got %d", who, u8 ? "uint8" : "an image", c);
    if (image && ((size_t)y & 3) != 0) return fail(RESR_ERR_ARG, "%s: the %s must be 4-byte aligned", who, u8 ? "uint8 output" : "output images");
    ResizeGeom g;
    g.c = c; g.h = h; g.w = w; g.oh = oh; g.ow = ow; g.py = taps_y; g.px = taps_x;
    g.cgroups = (c + 2) / 3;
    if ((long)n * g.cgroups > 65535) return fail(RESR_ERR_ARG, "%s: n * ceil(c / 3) = %ld beyond the grid", who, (long)n * g.cgroups);
    if (!choose_tile(g, kind))
        return fail(RESR_ERR_ARG, "%s: the footprint of one output %s (%d x %d taps) does not fit the LDS tile: scale too small", who,
                    yuv ? "2x2 block" : "pixel", taps_y, taps_x);
    if ((oh + g.th - 1) / g.th > 65535)
        return fail(RESR_ERR_ARG, "%s: %d x %d outputs in %d x %d tiles beyond the grid", who, oh, ow, g.th, g.tw);
    *out = g;
    return RESR_OK;
}

// resr_debug_resize_plan: what a launch of that plan asks for
size_t resize_lds_bytes(const ResizeGeom* gp, int kind) { return lds_bytes(*gp, kind); }

// resr_compact_yuv420_scaled_fits: would resize_plan find an even tile?  No device work, no error text.
int compact_yuv420_scaled_fits(int h, int w, int s, int oh, int ow, int taps_y, int taps_x, int bits) {
    if (h <= 0 || w <= 0 || s < 1 || s > 4 || oh <= 0 || ow <= 0 || ((h | w | oh | ow) & 1) || (bits != 8 && bits != 10)) return 0;
    if (taps_y < 1 || taps_y > kResizeMaxTaps || taps_x < 1 || taps_x > kResizeMaxTaps) return 0;
    if ((long)h * s > INT_MAX || (long)w * s > INT_MAX) return 0;
    ResizeGeom g;
    g.c = 3; g.h = h * s; g.w = w * s; g.oh = oh; g.ow = ow; g.py = taps_y; g.px = taps_x;
    g.cgroups = 1;
    return choose_tile(g, bits == 10 ? RESIZE_YUV10 : RESIZE_YUV8) ? 1 : 0;
}

// resr_compact_image_scaled_fits / resr_debug_image_resize_plan: the tile resize_plan would choose for an image mode's scaled tail
// (8-bit RGB: the uint8 tail's), without its pointer checks.  false: a bad argument or no tile.  No device work, no error text.
bool image_scaled_plan(int h, int w, int s, int oh, int ow, int taps_y, int taps_x, int channels, int bits, ResizeGeom* out, int* kind) {
    if (h <= 0 || w <= 0 || s < 1 || s > 4 || oh <= 0 || ow <= 0) return false;
    if ((channels != 1 && channels != 3 && channels != 4) || (bits != 8 && bits != 16)) return false;
    if (taps_y < 1 || taps_y > kResizeMaxTaps || taps_x < 1 || taps_x > kResizeMaxTaps) return false;
    if ((long)h * s > INT_MAX || (long)w * s > INT_MAX) return false;
    ResizeGeom g;
    g.c = 3; g.h = h * s; g.w = w * s; g.oh = oh; g.ow = ow; g.py = taps_y; g.px = taps_x;
    g.cgroups = 1;
    *kind = resize_image_kind(channels, bits);
    if (!choose_tile(g, *kind)) return false;
    *out = g;
    return true;
}

int image_resize_dispatch(const float* x, void* y, int n, int c, int h, int w, int oh, int ow, const int32_t* idx_y, const float* w_y,
                          int taps_y, const int32_t* idx_x, const float* w_x, int taps_x, int u8, hipStream_t st) {
    if (!x || !y) return fail(RESR_ERR_ARG, "image_resize: null argument");
    ResizeGeom g;
    const int rc = resize_plan("image_resize", n, c, h, w, oh, ow, idx_y, w_y, taps_y, idx_x, w_x, taps_x, u8 ? RESIZE_U8 : RESIZE_F32, y, &g);
    if (rc) return rc;
    const dim3 grid((unsigned)((ow + g.tw - 1) / g.tw), (unsigned)((oh + g.th - 1) / g.th), (unsigned)(n * g.cgroups));
    const PlanarSrc src{x, c, h, w};
    const size_t lds = lds_bytes(g, u8 ? RESIZE_U8 : RESIZE_F32);
    prof_before(st);
    if (u8)
        hipLaunchKernelGGL(image_resize_kernel<true>, grid, dim3(kResizeThreads), lds, st, src, y, idx_y, w_y, idx_x, w_x, g);
    else
        hipLaunchKernelGGL(image_resize_kernel<false>, grid, dim3(kResizeThreads), lds, st, src, y, idx_y, w_y, idx_x, w_x, g);
    // (31041 is also compact_tail_yuv's 31040 + s at s = 1, frames.hip.  Tests assert the values, so they stay.)
    prof_after(st, 31040 + (u8 ? 1 : 0), 2.0 * n * c * ((double)oh * w * taps_y + (double)oh * ow * taps_x),
               (double)n * c * ((double)h * w * 4.0 + (double)oh * ow * (u8 ? 1.0 : 4.0)));
    RESR_CHECK_LAUNCH("image_resize_kernel");
    return RESR_OK;
}

// The fused tail of the scaled YUV ends of compact_forward_ends: x, y frames of bytes or 16-bit words as qs->layout and qd->layout
// say (the caller has checked both), g planned by resize_plan for c = 3, h = H * s, w = W * s and the destination's RESIZE_YUV8 /
// RESIZE_YUV10.  Profiling ids name the instance: 31070 + s / 31080 + s where the two layouts are one, 31095 + s for the mixed tails.
int compact_tail_yuv420_scaled(const float* t, const void* x, void* y, int n, int h, int w, int s, const int32_t* idx_y, const float* w_y,
                               const int32_t* idx_x, const float* w_x, const ResrYuvDesc* qs, const ResrYuvDesc* qd, const ResizeGeom* gp,
                               hipStream_t st) {
    const ResizeGeom g = *gp;
    const bool ten = yuv_bits(qd->layout) == 10;
    const dim3 grid((unsigned)((g.ow + g.tw - 1) / g.tw), (unsigned)((g.oh + g.th - 1) / g.th), (unsigned)n);
    const size_t lds = lds_bytes(g, ten ? RESIZE_YUV10 : RESIZE_YUV8);
    prof_before(st);
    const bool ok = with_scale(s, [&](auto S) {
        with_yuv_layout(qs->layout, [&](auto A) {
            with_yuv_layout(qd->layout, [&](auto L) {
                constexpr int SBITS = yuv_bits(decltype(A)::value);
                const YuvShuffleSrc<decltype(S)::value, SBITS, decltype(A)::value> src{t, (const typename Depth<SBITS>::word*)x, h, w, *qs};
                hipLaunchKernelGGL((compact_tail_yuv_scaled_kernel<decltype(S)::value, decltype(A)::value, decltype(L)::value>), grid,
                                   dim3(kResizeThreads), lds, st, src, *qd, y, idx_y, w_y, idx_x, w_x, g);
            });
        });
    });
    if (!ok) return fail(RESR_ERR_ARG, "compact_tail_yuv420_scaled: upscale %d", s);
    // per LR pixel: 3 s^2 floats of t and 1.5 source words of x; per output pixel 1.5 destination words
    const double wb = ten ? 2.0 : 1.0, sb = yuv_bits(qs->layout) == 10 ? 2.0 : 1.0;
    prof_after(st, (qs->layout != qd->layout ? 31095 : ten ? 31080 : 31070) + s, 2.0 * n * 3 * ((double)g.oh * g.w * g.py + (double)g.oh * g.ow * g.px),
               (double)n * h * w * (s * s * 12.0 + 1.5 * sb) + (double)n * g.oh * g.ow * 1.5 * wb);
    RESR_CHECK_LAUNCH("compact_tail_yuv_scaled_kernel");
    return RESR_OK;
}

// The fused tail of the scaled image ends of compact_forward_ends: x, y image batches of n_images images in mode img (the caller has
// checked it), t the planes * n_images network images, g planned by resize_plan for n_images, c = 3, h = H * s, w = W * s and
// resize_image_kind of the mode.  Profiling id 31110 + s (uint8 RGB: 31050 + s).
int compact_tail_image_scaled(const float* t, const void* x, void* y, int n_images, int h, int w, int s, const int32_t* idx_y, const float* w_y,
                              const int32_t* idx_x, const float* w_x, const ResrImageDesc* img, const ResizeGeom* gp, hipStream_t st) {
    const ResizeGeom g = *gp;
    const dim3 grid((unsigned)((g.ow + g.tw - 1) / g.tw), (unsigned)((g.oh + g.th - 1) / g.th), (unsigned)n_images);
    const size_t lds = lds_bytes(g, resize_image_kind(img->channels, img->bits));
    prof_before(st);
    const bool ok = with_scale(s, [&](auto S) {
        with_image_mode(*img, [&](auto C, auto B) {
            typedef ImageShuffleSrc<decltype(S)::value, decltype(C)::value, decltype(B)::value> Src;
            hipLaunchKernelGGL((compact_tail_image_scaled_kernel<decltype(S)::value, decltype(C)::value, decltype(B)::value>), grid, dim3(kResizeThreads),
                               lds, st, (Src{t, (const typename Depth<decltype(B)::value>::word*)x, h, w, n_images}), y, idx_y, w_y, idx_x, w_x, g);
        });
    });
    if (!ok) return fail(RESR_ERR_ARG, "compact_tail_image_scaled: upscale %d", s);
    // per LR pixel of a network image: 3 s^2 floats of t and the image's pixel; per output pixel its words
    const double pb = img->channels * img->bits / 8.0, planes = img->channels == 4 ? 2.0 : 1.0;
    prof_after(st, image_id(img, 31050, 31110) + s, 2.0 * n_images * planes * 3 * ((double)g.oh * g.w * g.py + (double)g.oh * g.ow * g.px),
               (double)n_images * h * w * planes * (s * s * 12.0 + pb) + (double)n_images * g.oh * g.ow * pb);
    RESR_CHECK_LAUNCH("compact_tail_image_scaled_kernel");
    return RESR_OK;
}

}  // namespace resr
