// fullref.hip -- the full-reference metrics of image_quality_assessment.full_ref_native: PSNR and SSIM of the Y channel of sr against
// hr, one pass over the two images (resr_fullref, include/resr.h; that text states every order of summation and is the definition).
//   fullref_tile   : one workgroup owns one 32 x 32 tile of the SSIM map of one image.  It stages the tile plus the 10-pixel apron of
//                    both images from their own layout (three fp32 planes, or 3-byte HWC pixels: byte and dword loads only, nothing is
//                    assumed aligned), forms both luma levels in registers (luma_level.h) and keeps them in LDS as bytes.  H pass: the
//                    five 11-tap column sums (x, y, x^2, y^2, xy) of every staged column in float64 into LDS; W pass: the 11-tap row
//                    sums of those, the map value, the tile's map sum in a fixed order.  The squared differences of the pixels the
//                    tile owns (the last tile row / column own the 10 extra rows / columns) are summed as integers.  One
//                    (sse, ssim_sum) partial per tile; no atomics.
//   fullref_finish : one workgroup per image adds the partials in a fixed order and writes sse, psnr, ssim.
//   fullref_planes_tile (resr_fullref_planes: RGB channels, 16-bit images, the planes of YUV frames) is the same tile body
//                    (fr_tile_body) behind another Source: a level is taken out of a strided view of 1-, 2- or 4-byte words, levels up
//                    to 65535 lie in LDS as 16-bit words (+ 2 * 42 * 44 bytes: 61,216, still two workgroups per CU), the thread-private
//                    SSE is 64-bit, C1 and C2 are arguments; one workgroup per (image, plane, tile), the finish per (image, plane).
// LDS: lanes always walk a row of the float64 arrays.  The H pass writes consecutive words.  In the W pass a thread reads fourteen
// consecutive words as seven ds_read_b128 (rows are 336 bytes and a thread's first column a multiple of four, so every read is
// 16-byte aligned); eight threads share a row, 32 bytes apart, and the next row lies 84 dwords = 20 banks further, so the sixteen
// lanes of a quarter wave meet 64 different banks.  No float64 column walk exists, and the leading dimension is the plain 42.
// 5 * 32 * 42 * 8 + 2 * 42 * 44 + 64 = 57,520 bytes (57,536 as laid out): two workgroups fit a CU's 160 KiB.
#include <math.h>

#include "host_api.h"
#include "luma_level.h"

namespace resr {

constexpr int kFrTile = RESR_FULLREF_TILE, kFrTaps = 11, kFrApron = kFrTaps - 1, kFrReg = kFrTile + kFrApron;   // 32, 11, 10, 42
constexpr int kFrThreads = 256, kFrWaves = kFrThreads / 64, kFrBytePitch = 44, kFrMaps = 5;
constexpr int kFinThreads = RESR_FULLREF_FINISH_THREADS, kFinWaves = kFinThreads / 64;
static_assert(kFrTile * kFrTile == 4 * kFrThreads && kFrTile % 4 == 0, "the W pass gives every thread four adjacent map values of one row");

struct FullRefWindow { double k[kFrTaps]; };

// A source gives the tile body the two levels of pixel (y, x) of the cropped image the workgroup scores, the constants of the map and
// the types the levels and the thread-private SSE are kept in.  FrLumaSource: BT.601 luma of 8-bit RGB (resr_fullref).  FrPlaneSource:
// a level taken out of a view of the caller's memory (resr_fullref_planes).

// the level of image pixel `at` of one image (already offset to the image and to the crop's first pixel)
template <bool U8>
__device__ __forceinline__ uint8_t fr_level(const void* __restrict__ img, size_t plane, size_t at) {
    if (U8) {
        const uint8_t* p = (const uint8_t*)img + at * 3;
        return niqe_level(unit_of_byte(p[0]), unit_of_byte(p[1]), unit_of_byte(p[2]));
    }
    const float* p = (const float*)img + at;
    return niqe_level(p[0], p[plane], p[2 * plane]);
}

template <bool U8_SR, bool U8_HR>
struct FrLumaSource {
    typedef uint8_t level_t;
    typedef unsigned sse_t;          // thread-private: at most 42 * 42 / 256 < 7 terms of at most 65025
    const void *sr_img, *hr_img;     // the workgroup's image
    size_t plane;
    int W, crop;
    __device__ __forceinline__ FrLumaSource(const void* sr, const void* hr, int b, int H, int W_, int crop_) : plane((size_t)H * (size_t)W_), W(W_), crop(crop_) {
        sr_img = U8_SR ? (const void*)((const uint8_t*)sr + (size_t)b * plane * 3) : (const void*)((const float*)sr + (size_t)b * plane * 3);
        hr_img = U8_HR ? (const void*)((const uint8_t*)hr + (size_t)b * plane * 3) : (const void*)((const float*)hr + (size_t)b * plane * 3);
    }
    __device__ __forceinline__ void load(int y, int x, level_t& a, level_t& c) const {
        const size_t at = (size_t)(crop + y) * (size_t)W + (size_t)(crop + x);
        a = fr_level<U8_SR>(sr_img, plane, at);
        c = fr_level<U8_HR>(hr_img, plane, at);
    }
    __device__ __forceinline__ double c1() const { return 6.5025; }
    __device__ __forceinline__ double c2() const { return 58.5225; }
};

// one side of resr_fullref_planes as the kernel takes it: the descriptor's view with the base folded into the pointer
struct FrPlaneView {
    const void* base;
    long long pixel, row, plane, image;      // strides in words
    int word_bytes, shift, mask;
};

// the word at `at` of a view whose words have WB bytes, as loaded (fp32: its bits), and the level of such a word:
// (word >> shift) & mask of a 1- or 2-byte word; of an fp32 word quantise<peak> of yuv.h: trunc(clamp(v * peak, 0, peak)), NaN -> 0
template <int WB>
__device__ __forceinline__ unsigned fr_plane_word(const FrPlaneView& v, long long at) {
    return WB == 1 ? (unsigned)((const uint8_t*)v.base)[at] : WB == 2 ? (unsigned)((const uint16_t*)v.base)[at] : ((const unsigned*)v.base)[at];
}
template <int WB>
__device__ __forceinline__ uint16_t fr_plane_level(const FrPlaneView& v, unsigned word, float peak) {
    if (WB != 4) return (uint16_t)((word >> v.shift) & v.mask);
    float f = __uint_as_float(word) * peak;
    f = f > 0.f ? f : 0.f;          // (a NaN compares false: 0)
    f = f < peak ? f : peak;
    return (uint16_t)(unsigned)f;
}

struct FrPlaneSource {
    typedef uint16_t level_t;
    typedef unsigned long long sse_t;        // seven terms of 65535^2 do not fit 32 bits
    const FrPlaneView &sr, &hr;
    long long sr_at, hr_at;                  // the first pixel of the cropped plane of the workgroup's image, in words
    float peak;
    double k1, k2;
    __device__ __forceinline__ FrPlaneSource(const FrPlaneView& sr_, const FrPlaneView& hr_, int b, int pl, int crop, float peak_, double c1_, double c2_)
        : sr(sr_), hr(hr_), peak(peak_), k1(c1_), k2(c2_) {
        sr_at = (long long)b * sr.image + (long long)pl * sr.plane + (long long)crop * (sr.row + sr.pixel);
        hr_at = (long long)b * hr.image + (long long)pl * hr.plane + (long long)crop * (hr.row + hr.pixel);
    }
    // both loads of a pixel are issued in ONE block of straight-line code, chosen by the two (wave-uniform) word sizes: a branch per
    // side would put a wait behind each load and the tile would sit through two memory latencies per pixel instead of one
    template <int WS, int WH>
    __device__ __forceinline__ void load_as(long long s_at, long long h_at, level_t& a, level_t& c) const {
        const unsigned ws = fr_plane_word<WS>(sr, s_at), wh = fr_plane_word<WH>(hr, h_at);
        a = fr_plane_level<WS>(sr, ws, peak);
        c = fr_plane_level<WH>(hr, wh, peak);
    }
    __device__ __forceinline__ void load(int y, int x, level_t& a, level_t& c) const {
        const unsigned long long uy = (unsigned)y, ux = (unsigned)x;      // never negative: 32 x 64-bit products, not 64 x 64
        const long long s_at = sr_at + (long long)(uy * (unsigned long long)sr.row + ux * (unsigned long long)sr.pixel);
        const long long h_at = hr_at + (long long)(uy * (unsigned long long)hr.row + ux * (unsigned long long)hr.pixel);
        switch (sr.word_bytes * 8 + hr.word_bytes) {
            case 1 * 8 + 1: load_as<1, 1>(s_at, h_at, a, c); break;
            case 1 * 8 + 2: load_as<1, 2>(s_at, h_at, a, c); break;
            case 1 * 8 + 4: load_as<1, 4>(s_at, h_at, a, c); break;
            case 2 * 8 + 1: load_as<2, 1>(s_at, h_at, a, c); break;
            case 2 * 8 + 2: load_as<2, 2>(s_at, h_at, a, c); break;
            case 2 * 8 + 4: load_as<2, 4>(s_at, h_at, a, c); break;
            case 4 * 8 + 1: load_as<4, 1>(s_at, h_at, a, c); break;
            case 4 * 8 + 2: load_as<4, 2>(s_at, h_at, a, c); break;
            default: load_as<4, 4>(s_at, h_at, a, c); break;
        }
    }
    __device__ __forceinline__ double c1() const { return k1; }
    __device__ __forceinline__ double c2() const { return k2; }
};

// the map value from the five window sums (x, y, x^2, y^2, xy): every operation rounded once and none fused (the pragma: __dmul_rn and
// its kin are plain operators in this toolchain and would contract), so that with x == y numerator and denominator are the same bits
__device__ __forceinline__ double fr_map_value(const double* s, const double c1, const double c2) {
#pragma clang fp contract(off)
    const double m11 = s[0] * s[0], m22 = s[1] * s[1], m12 = s[0] * s[1];
    const double s11 = s[2] - m11, s22 = s[3] - m22, s12 = s[4] - m12;
    const double num = (2.0 * m12 + c1) * (2.0 * s12 + c2);
    const double den = ((m11 + m22) + c1) * ((s11 + s22) + c2);
    return num / den;
}

// THE tile: stage, H pass, W pass, map, the tile's (sse, map sum) partial to out[0 .. 1].  h x w is the cropped image.
template <class Source>
__device__ __forceinline__ void fr_tile_body(const Source& src, unsigned long long* __restrict__ out, int h, int w, int tiles_x, int tile, const FullRefWindow& win) {
    typedef typename Source::level_t level_t;
    typedef typename Source::sse_t sse_t;
    __shared__ double hp[kFrMaps][kFrTile][kFrReg];
    __shared__ __attribute__((aligned(4))) level_t lx[kFrReg * kFrBytePitch];
    __shared__ __attribute__((aligned(4))) level_t ly[kFrReg * kFrBytePitch];
    __shared__ double red_sum[kFrWaves];
    __shared__ unsigned long long red_sse[kFrWaves];
    const int tid = (int)threadIdx.x;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int mh = h - kFrApron, mw = w - kFrApron;                       // the map
    const int r0 = ty * kFrTile, c0 = tx * kFrTile;
    const int th = min(kFrTile, mh - r0), tw = min(kFrTile, mw - c0);     // map values of this tile: 1 .. 32 each way
    const int rh = th + kFrApron, rw = tw + kFrApron;                     // the staged region: r0 + rh <= h, c0 + rw <= w
    const int own_h = ty == (mh - 1) / kFrTile ? rh : th, own_w = tx == tiles_x - 1 ? rw : tw;   // the pixels whose SSE this tile owns
    // stage: levels of both images, and the SSE of the owned pixels (thread-private: at most 42 * 42 / 256 < 7 terms)
    sse_t sse = 0;
#pragma unroll 1
    for (int i = tid; i < rh * rw; i += kFrThreads) {
        const int ry = i / rw, rx = i - ry * rw;
        level_t a, c;
        src.load(r0 + ry, c0 + rx, a, c);
        lx[ry * kFrBytePitch + rx] = a;
        ly[ry * kFrBytePitch + rx] = c;
        const sse_t d = (sse_t)abs((int)a - (int)c);
        sse += (ry < own_h && rx < own_w) ? d * d : (sse_t)0;
    }
    __syncthreads();
    // H pass: for map row r and staged column c the five sums over k = 0 .. 10, ascending, of win.k[k] * value(r + k, c), one fused
    // multiply-add per tap from 0.0; the products x * x, y * y, x * y are integers and exact
    for (int i = tid; i < th * rw; i += kFrThreads) {
        const int r = i / rw, c = i - r * rw;
        double s[kFrMaps] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < kFrTaps; ++k) {
            const double x = (double)lx[(r + k) * kFrBytePitch + c], y = (double)ly[(r + k) * kFrBytePitch + c];
            const double g = win.k[k];
            s[0] = fma(g, x, s[0]);
            s[1] = fma(g, y, s[1]);
            s[2] = fma(g, __dmul_rn(x, x), s[2]);      // (integers below 2^16: the float64 products are exact)
            s[3] = fma(g, __dmul_rn(y, y), s[3]);
            s[4] = fma(g, __dmul_rn(x, y), s[4]);
        }
#pragma unroll
        for (int m = 0; m < kFrMaps; ++m) hp[m][r][c] = s[m];
    }
    __syncthreads();
    // W pass and the map: thread t has the four adjacent map values (t / 8, 4 (t % 8) + q), q = 0 .. 3 -- fourteen words of a row of
    // each H-pass array serve all four (44 if each value fetched its own eleven).  Words past the staged region are never written and
    // may hold anything: the values they reach lie outside the map and are dropped by the select below, never by arithmetic.
    const int r = tid / (kFrTile / 4), c4 = (tid % (kFrTile / 4)) * 4;
    double acc[4][kFrMaps];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int m = 0; m < kFrMaps; ++m) acc[q][m] = 0.0;
#pragma unroll
    for (int m = 0; m < kFrMaps; ++m) {
        double v[kFrTaps + 3];
#pragma unroll
        for (int k = 0; k < kFrTaps + 3; ++k) v[k] = hp[m][r][min(c4 + k, kFrReg - 1)];
#pragma unroll
        for (int k = 0; k < kFrTaps; ++k)      // taps ascending for every value, as in the H pass
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q][m] = fma(win.k[k], v[q + k], acc[q][m]);
    }
    double sum = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double value = fr_map_value(acc[q], src.c1(), src.c2());
        sum = __dadd_rn(sum, (r < th && c4 + q < tw) ? value : 0.0);       // q ascending; a value outside the map is an exact zero
    }
    // lanes meet in a fixed butterfly, waves are added in ascending order
    unsigned long long sse64 = sse;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum = __dadd_rn(sum, __shfl_xor(sum, off));
        sse64 += __shfl_xor(sse64, off);
    }
    if ((tid & 63) == 0) {
        red_sum[tid >> 6] = sum;
        red_sse[tid >> 6] = sse64;
    }
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        unsigned long long total_sse = 0;
        for (int wv = 0; wv < kFrWaves; ++wv) {
            total = __dadd_rn(total, red_sum[wv]);
            total_sse += red_sse[wv];
        }
        out[0] = total_sse;
        out[1] = (unsigned long long)__double_as_longlong(total);
    }
}

template <bool U8_SR, bool U8_HR>
__global__ __launch_bounds__(kFrThreads) void fullref_tile_kernel(const void* __restrict__ sr, const void* __restrict__ hr, unsigned long long* __restrict__ partials, int H, int W,
                                                                  int crop, int h, int w, int tiles_x, int tiles, FullRefWindow win) {
    const int tile = (int)(blockIdx.x % (unsigned)tiles), b = (int)(blockIdx.x / (unsigned)tiles);
    fr_tile_body(FrLumaSource<U8_SR, U8_HR>(sr, hr, b, H, W, crop), partials + (size_t)blockIdx.x * 2, h, w, tiles_x, tile, win);
}

// workgroup (image * planes + plane) * tiles + tile
__global__ __launch_bounds__(kFrThreads) void fullref_planes_tile_kernel(FrPlaneView sr, FrPlaneView hr, unsigned long long* __restrict__ partials, int planes, int crop, int h, int w,
                                                                         int tiles_x, int tiles, float peak, double c1, double c2, FullRefWindow win) {
    const int tile = (int)(blockIdx.x % (unsigned)tiles), ip = (int)(blockIdx.x / (unsigned)tiles);
    fr_tile_body(FrPlaneSource(sr, hr, ip / planes, ip % planes, crop, peak, c1, c2), partials + (size_t)blockIdx.x * 2, h, w, tiles_x, tile, win);
}

// thread t adds partials t, t + 256, ... of its image (of its plane of its image: resr_fullref_planes) in ascending order; lanes meet in the same butterfly, waves in ascending order
__global__ __launch_bounds__(kFinThreads) void fullref_finish_kernel(const unsigned long long* __restrict__ partials, int tiles, double pixels, double map_values, double peak2,
                                                                    int64_t* __restrict__ sse_out, double* __restrict__ psnr_out, double* __restrict__ ssim_out) {
    __shared__ double red_sum[kFinWaves];
    __shared__ unsigned long long red_sse[kFinWaves];
    const int tid = (int)threadIdx.x;
    const unsigned long long* p = partials + (size_t)blockIdx.x * (size_t)tiles * 2;
    double sum = 0.0;
    unsigned long long sse = 0;
    for (int i = tid; i < tiles; i += kFinThreads) {
        sse += p[(size_t)i * 2];
        sum = __dadd_rn(sum, __longlong_as_double((long long)p[(size_t)i * 2 + 1]));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum = __dadd_rn(sum, __shfl_xor(sum, off));
        sse += __shfl_xor(sse, off);
    }
    if ((tid & 63) == 0) {
        red_sum[tid >> 6] = sum;
        red_sse[tid >> 6] = sse;
    }
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        unsigned long long total_sse = 0;
        for (int wv = 0; wv < kFinWaves; ++wv) {
            total = __dadd_rn(total, red_sum[wv]);
            total_sse += red_sse[wv];
        }
        sse_out[blockIdx.x] = (int64_t)total_sse;
        psnr_out[blockIdx.x] = __dmul_rn(10.0, log10(peak2 / __dadd_rn((double)total_sse / pixels, 1e-8)));
        ssim_out[blockIdx.x] = total / map_values;
    }
}

namespace {
struct FullRefPlan {
    int h, w;            // after the crop
    int tiles_x, tiles;  // per image
    size_t bytes;
};

bool fullref_plan(const ResrFullRefDesc* d, FullRefPlan* p) {
    if (!d) return fail(RESR_ERR_ARG, "fullref: null descriptor"), false;
    if (d->n < 1 || d->h < 1 || d->w < 1 || d->crop < 0)
        return fail(RESR_ERR_ARG, "fullref: bad descriptor (n=%d, images %dx%d, crop %d: n, h, w at least 1, crop at least 0)", d->n, d->h, d->w, d->crop), false;
    const int64_t h = (int64_t)d->h - 2 * (int64_t)d->crop, w = (int64_t)d->w - 2 * (int64_t)d->crop;
    if (h < kFrTaps || w < kFrTaps)
        return fail(RESR_ERR_ARG, "fullref: a crop of %d leaves %lldx%lld of a %dx%d image, less than the 11x11 window", d->crop, (long long)h, (long long)w, d->h, d->w), false;
    const int64_t tiles_y = (h - kFrApron + kFrTile - 1) / kFrTile, tiles_x = (w - kFrApron + kFrTile - 1) / kFrTile;
    if (tiles_y * tiles_x > 0x7fffffffLL || (int64_t)d->n * tiles_y * tiles_x > 0x7fffffffLL)
        return fail(RESR_ERR_ARG, "fullref: %d images of %lld x %lld tiles do not fit the int32 tile index of a launch", d->n, (long long)tiles_y, (long long)tiles_x), false;
    p->h = (int)h;
    p->w = (int)w;
    p->tiles_x = (int)tiles_x;
    p->tiles = (int)(tiles_y * tiles_x);
    p->bytes = (size_t)d->n * (size_t)p->tiles * 16;
    return true;
}

// the 11 taps, by the host's libm
void fullref_window(FullRefWindow* win) {
    double total = 0.0;
    for (int i = 0; i < kFrTaps; ++i) {
        win->k[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
        total += win->k[i];
    }
    for (int i = 0; i < kFrTaps; ++i) win->k[i] /= total;
}
}  // namespace

size_t fullref_workspace_bytes(const ResrFullRefDesc* d) {
    FullRefPlan p;
    return fullref_plan(d, &p) ? p.bytes : 0;
}

int fullref_dispatch(const ResrFullRefDesc* d, const void* sr, const void* hr, int64_t* sse, double* psnr, double* ssim, hipStream_t st) {
    FullRefPlan p;
    if (!fullref_plan(d, &p)) return RESR_ERR_ARG;
    if (!sr || !hr || !sse || !psnr || !ssim || !d->workspace) return fail(RESR_ERR_ARG, "fullref: null pointer");
    if (((uintptr_t)d->workspace | (uintptr_t)sse | (uintptr_t)psnr | (uintptr_t)ssim) & 7)
        return fail(RESR_ERR_ARG, "fullref: the workspace, sse, psnr and ssim must be 8-byte aligned");
    if ((!d->sr_u8 && ((uintptr_t)sr & 3)) || (!d->hr_u8 && ((uintptr_t)hr & 3))) return fail(RESR_ERR_ARG, "fullref: a float image must be 4-byte aligned");
    if (d->workspace_bytes < p.bytes) return fail(RESR_ERR_ARG, "fullref: workspace of %zu bytes, %zu needed", d->workspace_bytes, p.bytes);
    FullRefWindow win;
    fullref_window(&win);
    unsigned long long* partials = (unsigned long long*)d->workspace;
    const dim3 grid((unsigned)((int64_t)d->n * p.tiles)), block(kFrThreads);
    const double px = (double)d->n * p.h * p.w;
    prof_before(st);
#define RESR_FULLREF_LAUNCH(A, B) \
    hipLaunchKernelGGL((fullref_tile_kernel<A, B>), grid, block, 0, st, sr, hr, partials, d->h, d->w, d->crop, p.h, p.w, p.tiles_x, p.tiles, win)
    if (d->sr_u8 && d->hr_u8) RESR_FULLREF_LAUNCH(true, true);
    else if (d->sr_u8) RESR_FULLREF_LAUNCH(true, false);
    else if (d->hr_u8) RESR_FULLREF_LAUNCH(false, true);
    else RESR_FULLREF_LAUNCH(false, false);
#undef RESR_FULLREF_LAUNCH
    prof_after(st, 34600 + (d->sr_u8 ? 1 : 0) + (d->hr_u8 ? 2 : 0), px * 2.0 * 5.0 * kFrTaps * 2.3, px * ((d->sr_u8 ? 3.0 : 12.0) + (d->hr_u8 ? 3.0 : 12.0)));
    RESR_CHECK_LAUNCH("fullref_tile_kernel");
    prof_before(st);
    hipLaunchKernelGGL(fullref_finish_kernel, dim3((unsigned)d->n), dim3(kFinThreads), 0, st, (const unsigned long long*)partials, p.tiles, (double)p.h * (double)p.w,
                       (double)(p.h - kFrApron) * (double)(p.w - kFrApron), 65025.0, sse, psnr, ssim);
    prof_after(st, 34700, 0.0, (double)d->n * p.tiles * 16.0);
    RESR_CHECK_LAUNCH("fullref_finish_kernel");
    return RESR_OK;
}

// ---- resr_fullref_planes: the same tile and finish over (image, plane), levels through a view of each side ----
namespace {
struct FullRefSide {
    const char* name;
    int word_bytes, shift, mask;
    int64_t base, pixel, row, plane, image;
};

bool fullref_planes_plan(const ResrFullRefPlanesDesc* d, FullRefPlan* p, FullRefSide* sides) {
    if (!d) return fail(RESR_ERR_ARG, "fullref_planes: null descriptor"), false;
    if (d->n < 1 || d->planes < 1 || d->planes > 4 || d->h < 1 || d->w < 1 || d->crop < 0)
        return fail(RESR_ERR_ARG, "fullref_planes: bad descriptor (n=%d, %d planes of %dx%d, crop %d: n, h, w at least 1, planes 1 .. 4, crop at least 0)", d->n, d->planes, d->h, d->w,
                    d->crop), false;
    if (d->peak != 255 && d->peak != 1023 && d->peak != 65535) return fail(RESR_ERR_ARG, "fullref_planes: peak %d is none of 255, 1023, 65535", d->peak), false;
    sides[0] = {"sr", d->sr_word_bytes, d->sr_shift, d->sr_mask, d->sr_base, d->sr_pixel_stride, d->sr_row_stride, d->sr_plane_stride, d->sr_image_stride};
    sides[1] = {"hr", d->hr_word_bytes, d->hr_shift, d->hr_mask, d->hr_base, d->hr_pixel_stride, d->hr_row_stride, d->hr_plane_stride, d->hr_image_stride};
    for (int i = 0; i < 2; ++i) {
        const FullRefSide& v = sides[i];
        if (v.word_bytes != 1 && v.word_bytes != 2 && v.word_bytes != 4) return fail(RESR_ERR_ARG, "fullref_planes: %s word_bytes %d is none of 1, 2, 4", v.name, v.word_bytes), false;
        if (v.shift < 0 || v.shift > 15 || v.mask < 0 || v.mask > d->peak)
            return fail(RESR_ERR_ARG, "fullref_planes: %s shift %d, mask %d (shift 0 .. 15, mask 0 .. the peak %d)", v.name, v.shift, v.mask, d->peak), false;
        if (v.pixel < 1 || v.row < 1 || v.plane < 0 || v.image < 0 || v.base < 0)
            return fail(RESR_ERR_ARG, "fullref_planes: %s strides pixel %lld, row %lld, plane %lld, image %lld, base %lld (pixel and row at least 1, the others at least 0)", v.name,
                        (long long)v.pixel, (long long)v.row, (long long)v.plane, (long long)v.image, (long long)v.base), false;
    }
    const int64_t h = (int64_t)d->h - 2 * (int64_t)d->crop, w = (int64_t)d->w - 2 * (int64_t)d->crop;
    if (h < kFrTaps || w < kFrTaps)
        return fail(RESR_ERR_ARG, "fullref_planes: a crop of %d leaves %lldx%lld of a %dx%d plane, less than the 11x11 window", d->crop, (long long)h, (long long)w, d->h, d->w), false;
    const int64_t tiles_y = (h - kFrApron + kFrTile - 1) / kFrTile, tiles_x = (w - kFrApron + kFrTile - 1) / kFrTile;
    if (tiles_y * tiles_x > 0x7fffffffLL || (int64_t)d->n * d->planes * tiles_y * tiles_x > 0x7fffffffLL)
        return fail(RESR_ERR_ARG, "fullref_planes: %d images of %d planes of %lld x %lld tiles do not fit the int32 tile index of a launch", d->n, d->planes, (long long)tiles_y,
                    (long long)tiles_x), false;
    p->h = (int)h;
    p->w = (int)w;
    p->tiles_x = (int)tiles_x;
    p->tiles = (int)(tiles_y * tiles_x);
    p->bytes = (size_t)d->n * (size_t)d->planes * (size_t)p->tiles * 16;
    return true;
}
}  // namespace

size_t fullref_planes_workspace_bytes(const ResrFullRefPlanesDesc* d) {
    FullRefPlan p;
    FullRefSide sides[2];
    return fullref_planes_plan(d, &p, sides) ? p.bytes : 0;
}

int fullref_planes_dispatch(const ResrFullRefPlanesDesc* d, const void* sr, const void* hr, int64_t* sse, double* psnr, double* ssim, hipStream_t st) {
    FullRefPlan p;
    FullRefSide sides[2];
    if (!fullref_planes_plan(d, &p, sides)) return RESR_ERR_ARG;
    if (!sr || !hr || !sse || !psnr || !ssim || !d->workspace) return fail(RESR_ERR_ARG, "fullref_planes: null pointer");
    if (((uintptr_t)d->workspace | (uintptr_t)sse | (uintptr_t)psnr | (uintptr_t)ssim) & 7)
        return fail(RESR_ERR_ARG, "fullref_planes: the workspace, sse, psnr and ssim must be 8-byte aligned");
    if (((uintptr_t)sr & (uintptr_t)(sides[0].word_bytes - 1)) || ((uintptr_t)hr & (uintptr_t)(sides[1].word_bytes - 1)))
        return fail(RESR_ERR_ARG, "fullref_planes: a base pointer must be aligned to its %d- / %d-byte word", sides[0].word_bytes, sides[1].word_bytes);
    if (d->workspace_bytes < p.bytes) return fail(RESR_ERR_ARG, "fullref_planes: workspace of %zu bytes, %zu needed", d->workspace_bytes, p.bytes);
    FullRefWindow win;
    fullref_window(&win);
    FrPlaneView views[2];
    const void* ptrs[2] = {sr, hr};
    for (int i = 0; i < 2; ++i) {
        const FullRefSide& v = sides[i];
        views[i] = {(const void*)((const char*)ptrs[i] + (size_t)v.base * (size_t)v.word_bytes), (long long)v.pixel, (long long)v.row, (long long)v.plane, (long long)v.image,
                    v.word_bytes, v.shift, v.mask};
    }
    const double peak2 = (double)((int64_t)d->peak * (int64_t)d->peak);
    unsigned long long* partials = (unsigned long long*)d->workspace;
    const int64_t maps = (int64_t)d->n * d->planes;
    const double px = (double)maps * p.h * p.w;
    prof_before(st);
    hipLaunchKernelGGL(fullref_planes_tile_kernel, dim3((unsigned)(maps * p.tiles)), dim3(kFrThreads), 0, st, views[0], views[1], partials, d->planes, d->crop, p.h, p.w, p.tiles_x,
                       p.tiles, (float)d->peak, peak2 / 10000.0, (9.0 * peak2) / 10000.0, win);
    prof_after(st, 34604, px * 2.0 * 5.0 * kFrTaps * 2.3, px * (double)(sides[0].word_bytes + sides[1].word_bytes));
    RESR_CHECK_LAUNCH("fullref_planes_tile_kernel");
    prof_before(st);
    hipLaunchKernelGGL(fullref_finish_kernel, dim3((unsigned)maps), dim3(kFinThreads), 0, st, (const unsigned long long*)partials, p.tiles, (double)p.h * (double)p.w,
                       (double)(p.h - kFrApron) * (double)(p.w - kFrApron), peak2, sse, psnr, ssim);
    prof_after(st, 34701, 0.0, (double)maps * p.tiles * 16.0);
    RESR_CHECK_LAUNCH("fullref_finish_kernel");
    return RESR_OK;
}

}  // namespace resr
