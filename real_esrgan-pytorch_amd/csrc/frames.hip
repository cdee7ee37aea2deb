// frames.hip -- the uint8 frame path: u8 HWC images in, u8 HWC images out.
//
//   u8_head        : u8 [N,H,W,3] -> the compact net's x_in [N,H,W,32] in the model's arithmetic (channels 3..31 zero)
//   compact_tail_u8: t [N,3S^2,H,W] fp32 + the u8 input frame -> u8 [N,H*S,W*S,3]   (pixel-shuffle + residual + quantise)
//   u8_to_nchw     : u8 [N,H,W,3] -> fp32 [N,3,H,W]                (models whose first kernel is not ours to fuse)
//   nchw_to_u8     : fp32 [N,3,H,W] -> u8 [N,H,W,3]                (... and whose last one is not: RRDB Generator, the tiler)
//
// The result is DEFINED as what the float path followed by imgproc.tensor_to_image produces, bit for bit:
//   in : x = (float)u8 / 255.0f, one IEEE division (numpy's astype(float32) / 255.0), then converted to the model's type exactly
//        as nchw_to_nhwc_kernel converts a float (split_f16 / the rounding of common.h);
//   out: v = t + x (fp32, the single add of compact_tail_kernel; the generic kernel has no add), then v * 255.0f, clamp to
//        [0, 255], truncate -- in this order, nothing re-associated (t * 255 + x * 255 is another number).
// A NaN in v is outside the contract (the float path's astype(uint8) of a NaN is undefined too); here it quantises to 0.
// Every index that can pass 2^31 is 64-bit.  Vector stores only.
#include "common.h"

namespace resr {

namespace {

__device__ __forceinline__ float u8_unit(unsigned v) { return (float)v / 255.0f; }

__device__ __forceinline__ unsigned quantise_u8(float v) {
    v *= 255.0f;
    v = v > 0.f ? v : 0.f;          // (a NaN compares false: 0)
    v = v < 255.f ? v : 255.f;
    return (unsigned)v;             // truncation, as astype(uint8) of a value in [0, 255]
}

// One thread per 16-byte piece of an output pixel (as nchw_to_nhwc_kernel): only piece 0 holds the three real channels.
template <typename T>
__global__ __launch_bounds__(256) void u8_head_kernel(const uint8_t* __restrict__ src, T* __restrict__ dst, long px, long lo_off) {
    constexpr int E = 16 / (int)sizeof(T);
    constexpr int PIECES = 32 / E;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= px * PIECES) return;
    const long p = idx / PIECES;
    const int piece = (int)(idx - p * PIECES);
    uint4 out = make_uint4(0u, 0u, 0u, 0u), outl = make_uint4(0u, 0u, 0u, 0u);
    if (piece == 0) {
        T* o = reinterpret_cast<T*>(&out);
        T* ol = reinterpret_cast<T*>(&outl);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = u8_unit(src[p * 3 + c]);
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

// The output is a flat array of n * hS * wS pixels of 3 bytes; a thread owns 4 consecutive pixels = 12 bytes = three dword
// stores (y is 4-byte aligned and 12 k is, whatever wS is), a wavefront writes 768 contiguous bytes.  Each pixel decodes its
// own (n, Y, X); the last partial group falls back to byte stores.  The 3 x S planes read for one (Y/S, X/S) are plane-strided
// but coalesced across lanes, as in compact_tail_kernel.  RES = false: the generic fp32 NCHW -> u8 HWC conversion (S = 1).
template <int S, bool RES>
__global__ __launch_bounds__(256) void compact_tail_u8_kernel(const float* __restrict__ t, const uint8_t* __restrict__ x,
                                                              uint8_t* __restrict__ y, int n, int h, int w) {
    const int HS = h * S, WS = w * S;
    const long plane = (long)h * w;
    const long total = (long)n * HS * WS;
    const long q0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (q0 >= total) return;
    const long row0 = q0 / WS;                 // b * HS + Y
    int X = (int)(q0 - row0 * WS);
    long b = row0 / HS;
    int Y = (int)(row0 - b * HS);
    unsigned bytes[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (q0 + k < total) {
            const int yy = Y / S, sy = Y - yy * S, xx = X / S, sx = X - xx * S;
            const float* tp = t + (b * 3 * S * S + sy * S + sx) * plane + (long)yy * w + xx;
            const long xo = ((b * h + yy) * (long)w + xx) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v = tp[(long)c * S * S * plane];
                if constexpr (RES) v = v + u8_unit(x[xo + c]);
                bytes[k * 3 + c] = quantise_u8(v);
            }
        } else {
            bytes[k * 3] = bytes[k * 3 + 1] = bytes[k * 3 + 2] = 0u;
        }
        if (++X == WS) {
            X = 0;
            if (++Y == HS) { Y = 0; ++b; }
        }
    }
    if (q0 + 4 <= total) {
        unsigned* o = reinterpret_cast<unsigned*>(y + q0 * 3);
#pragma unroll
        for (int d = 0; d < 3; ++d)
            o[d] = bytes[4 * d] | (bytes[4 * d + 1] << 8) | (bytes[4 * d + 2] << 16) | (bytes[4 * d + 3] << 24);
    } else {
        const int left = (int)(total - q0) * 3;
#pragma unroll
        for (int i = 0; i < 9; ++i)
            if (i < left) y[q0 * 3 + i] = (uint8_t)bytes[i];
    }
}

// One thread per pixel: 3 byte loads (a wavefront reads 192 contiguous bytes), one coalesced dword store per plane.
__global__ __launch_bounds__(256) void u8_to_nchw_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, long total, long plane) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    const long b = p / plane, r = p - b * plane;
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[(b * 3 + c) * plane + r] = u8_unit(src[p * 3 + c]);
}

bool grid_ok(long threads) { return threads > 0 && (threads + 255) / 256 <= 0x7fffffffL; }

template <int S, bool RES>
void launch_tail(const float* t, const uint8_t* x, uint8_t* y, int n, int h, int w, hipStream_t st) {
    const long groups = ((long)n * h * S * w * S + 3) / 4;
    hipLaunchKernelGGL((compact_tail_u8_kernel<S, RES>), dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, t, x, y, n, h, w);
}

}  // namespace

// lo_off: the hi -> lo element offset of x_in (RESR_F16X2), as compact_forward passes it to nchw_to_nhwc_dispatch
int u8_head_dispatch(const uint8_t* src, void* dst, int n, int h, int w, int dtype, hipStream_t st, long lo_off) {
    if (!src || !dst || n <= 0 || h <= 0 || w <= 0) return fail(RESR_ERR_ARG, "u8_head: bad argument");
    const long px = (long)n * h * w;
    const int pieces = dtype != RESR_F32 ? 4 : 8;
    if (!grid_ok(px * pieces)) return fail(RESR_ERR_ARG, "u8_head: %ld pixels beyond the grid", px);
    const dim3 grid((unsigned)((px * pieces + 255) / 256));
    if (dtype != RESR_F16X2) lo_off = 0;
    prof_before(st);
    if (dtype != RESR_F32)
        hipLaunchKernelGGL(u8_head_kernel<half_t>, grid, dim3(256), 0, st, src, (half_t*)dst, px, lo_off);
    else
        hipLaunchKernelGGL(u8_head_kernel<float>, grid, dim3(256), 0, st, src, (float*)dst, px, 0L);
    prof_after(st, 31020, 0.0, (double)px * (3.0 + 32.0 * (double)(elem_size(dtype) * act_tensors(dtype))));
    RESR_CHECK_LAUNCH("u8_head_kernel");
    return RESR_OK;
}

int compact_tail_u8(const float* t, const uint8_t* x, uint8_t* y, int n, int h, int w, int s, hipStream_t st) {
    if (((size_t)y & 3) != 0) return fail(RESR_ERR_ARG, "compact_tail_u8: the output must be 4-byte aligned");
    prof_before(st);
    switch (s) {
        case 1: launch_tail<1, true>(t, x, y, n, h, w, st); break;
        case 2: launch_tail<2, true>(t, x, y, n, h, w, st); break;
        case 3: launch_tail<3, true>(t, x, y, n, h, w, st); break;
        case 4: launch_tail<4, true>(t, x, y, n, h, w, st); break;
        default: return fail(RESR_ERR_ARG, "compact_tail_u8: upscale %d", s);
    }
    // per LR pixel: 3 s^2 floats of t, 3 bytes of x, 3 s^2 bytes out
    prof_after(st, 31010 + s, 0.0, (double)n * h * w * (s * s * 15.0 + 3.0));
    RESR_CHECK_LAUNCH("compact_tail_u8_kernel");
    return RESR_OK;
}

int u8_to_nchw_dispatch(const uint8_t* src, float* dst, int n, int h, int w, hipStream_t st) {
    if (!src || !dst || n <= 0 || h <= 0 || w <= 0) return fail(RESR_ERR_ARG, "u8_to_nchw: bad argument (n=%d h=%d w=%d)", n, h, w);
    const long plane = (long)h * w, total = plane * n;
    if (!grid_ok(total)) return fail(RESR_ERR_ARG, "u8_to_nchw: %ld pixels beyond the grid", total);
    prof_before(st);
    hipLaunchKernelGGL(u8_to_nchw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, dst, total, plane);
    prof_after(st, 31030, 0.0, (double)total * 15.0);
    RESR_CHECK_LAUNCH("u8_to_nchw_kernel");
    return RESR_OK;
}

int nchw_to_u8_dispatch(const float* src, uint8_t* dst, int n, int h, int w, hipStream_t st) {
    if (!src || !dst || n <= 0 || h <= 0 || w <= 0) return fail(RESR_ERR_ARG, "nchw_to_u8: bad argument (n=%d h=%d w=%d)", n, h, w);
    if (((size_t)dst & 3) != 0) return fail(RESR_ERR_ARG, "nchw_to_u8: the output must be 4-byte aligned");
    const long total = (long)n * h * w;
    if (!grid_ok((total + 3) / 4)) return fail(RESR_ERR_ARG, "nchw_to_u8: %ld pixels beyond the grid", total);
    prof_before(st);
    launch_tail<1, false>(src, nullptr, dst, n, h, w, st);
    prof_after(st, 31031, 0.0, (double)total * 15.0);
    RESR_CHECK_LAUNCH("nchw_to_u8_kernel");
    return RESR_OK;
}

}  // namespace resr
