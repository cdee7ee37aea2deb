// disc.hip -- kernels specific to the U-Net spectral-norm discriminator (reference model.py:135-203):
//   space_to_depth / depth_to_space   a 4x4 stride-2 pad-1 conv (model.py:140,144,148) is evaluated as a 3x3
//                                     pad-1 conv over the 2x2 space-to-depth image with a sparse virtual kernel
//                                     (pack.hip mode "virtual 4x4"), so it runs on the same MFMA conv kernel
//   bilinear_up2x (+ backward)        F.interpolate(scale_factor=2, mode="bilinear", align_corners=False)
//                                     (model.py:186,190,194)
//   spectral norm                     torch.nn.utils.spectral_norm's power iteration, sigma = u.(W v), and the
//                                     backward of W = W_orig / sigma
//   add_mask                          skip-connection gradient merge fused with the LeakyReLU backward
//   fold4x4                           virtual 3x3x4C weight gradient -> real 4x4xC layout
// All HBM-bound helpers; pixel-major (NHWC) activations of type T.
#include "host_api.h"

namespace resr {

// RESR_F16X2 (T = f16 with a non-zero hi -> lo element offset): every tensor is a (hi, lo) pair, value = hi + lo * 2^-12
// (include/resr.h); the helpers below read E values of a 16-byte piece as fp32 and store them split.
template <typename T>
__device__ __forceinline__ void ld_vals(const T* p, long lo, float* v) {
    constexpr int E = 16 / (int)sizeof(T);
    const uint4 raw = *reinterpret_cast<const uint4*>(p);
    const T* q = reinterpret_cast<const T*>(&raw);
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = (float)q[e];
    if constexpr (sizeof(T) == 2) {
        if (lo) {
            const uint4 rawl = *reinterpret_cast<const uint4*>(p + lo);
            const T* ql = reinterpret_cast<const T*>(&rawl);
#pragma unroll
            for (int e = 0; e < E; ++e) v[e] = __builtin_fmaf((float)ql[e], kLoInv, v[e]);
        }
    }
}
template <typename T>
__device__ __forceinline__ void st_vals(T* p, long lo, const float* v) {
    constexpr int E = 16 / (int)sizeof(T);
    uint4 o, ol;
    T* q = reinterpret_cast<T*>(&o);
    T* ql = reinterpret_cast<T*>(&ol);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        q[e] = (T)v[e];
        if constexpr (sizeof(T) == 2) ql[e] = (T)((v[e] - (float)q[e]) * kLoScale);
    }
    *reinterpret_cast<uint4*>(p) = o;
    if constexpr (sizeof(T) == 2) {
        if (lo) *reinterpret_cast<uint4*>(p + lo) = ol;
    }
}

// LeakyReLU-backward multipliers from a saved activation `pm` (8 / 4 values at `at`); RESR_F16X2 (lo != 0): a hi value that rounded to
// zero defers to the lo tensor, read only then (common.h pair_positive)
template <typename T>
__device__ __forceinline__ void mask_mult(const T* at, long lo, float slope, float* v) {
    constexpr int E = 16 / (int)sizeof(T);
    const uint4 rm = *reinterpret_cast<const uint4*>(at);
    const T* pm = reinterpret_cast<const T*>(&rm);
    bool pos[E];
    bool anyz = false;
#pragma unroll
    for (int e = 0; e < E; ++e) { pos[e] = (float)pm[e] > 0.f; anyz = anyz || (float)pm[e] == 0.f; }
    if constexpr (sizeof(T) == 2) {
        if (lo && anyz) {
            const uint4 rl = *reinterpret_cast<const uint4*>(at + lo);
            const T* pl = reinterpret_cast<const T*>(&rl);
#pragma unroll
            for (int e = 0; e < E; ++e) pos[e] = pair_positive(pm[e], pl[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        v[e] *= pos[e] ? 1.f : slope;
        // opaque: ONE fp32 product for every later use.  Left visible, the compiler folded the multiply into the f16 conversion of
        // some uses (v_fma_mixlo_f16: one rounding of the exact product) and not of others (multiply, then convert), and st_vals
        // stored the hi of one with the lo that belongs to the other: one f16 ulp apart where the fp32 product sits on an f16 tie
        if constexpr (sizeof(T) == 2) asm("" : "+v"(v[e]));
    }
}

// dst[Y][X][(i*2+j)*C + c] = src[2Y+i][2X+j][c]   (inverse: the other way round).  A pure permutation: RESR_F16X2 callers run it
// over hi and lo at once as a batch of 2n (the lo tensor directly follows the hi tensor in both operands).
template <typename T>
__global__ __launch_bounds__(256) void s2d_kernel(const T* __restrict__ src, T* __restrict__ dst, int n, int h, int w, int c,
                                                  int inverse) {
    constexpr int E = 16 / (int)sizeof(T);
    const unsigned groups = (unsigned)c / E;          // h, w = full-resolution dims
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= (unsigned)w * groups) return;
    const int x = (int)(idx / groups), g = (int)(idx - (unsigned)x * groups);
    const int y = (int)blockIdx.y, b = (int)blockIdx.z;
    const size_t full = (((size_t)b * h + y) * w + x) * c + g * E;
    const size_t packed = ((((size_t)b * (h / 2) + y / 2) * (w / 2) + x / 2) * 4 + (y & 1) * 2 + (x & 1)) * c + g * E;
    if (!inverse) *reinterpret_cast<uint4*>(dst + packed) = *reinterpret_cast<const uint4*>(src + full);
    else *reinterpret_cast<uint4*>(dst + full) = *reinterpret_cast<const uint4*>(src + packed);
}

// depth-to-space fused with the skip-gradient merge and the LeakyReLU backward that follow it in the discriminator's backward
// pass: out[full] = (src[packed] + add[full]) * (mask[full] > 0 ? 1 : slope)   (add, mask optional) -- the same roundings as
// s2d(inverse) followed by add_mask, one pass instead of two.  lo_* : RESR_F16X2 hi -> lo offsets of src / add / out (the mask is
// an activation of out's shape: its sign is its hi tensor's, or its lo tensor's where hi rounded to zero).
template <typename T>
__global__ __launch_bounds__(256) void d2s_add_mask_kernel(const T* __restrict__ src, const T* __restrict__ add, const T* __restrict__ mask,
                                                           T* __restrict__ out, int n, int h, int w, int c, float slope, long lo_src,
                                                           long lo_add, long lo_out) {
    constexpr int E = 16 / (int)sizeof(T);
    const unsigned groups = (unsigned)c / E;          // h, w = full-resolution dims
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= (unsigned)w * groups) return;
    const int x = (int)(idx / groups), g = (int)(idx - (unsigned)x * groups);
    const int y = (int)blockIdx.y, b = (int)blockIdx.z;
    const size_t full = (((size_t)b * h + y) * w + x) * c + g * E;
    const size_t packed = ((((size_t)b * (h / 2) + y / 2) * (w / 2) + x / 2) * 4 + (y & 1) * 2 + (x & 1)) * c + g * E;
    float v[E], va[E];
    ld_vals(src + packed, lo_src, v);
    if (add) {
        ld_vals(add + full, lo_add, va);
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] += va[e];
    }
    if (mask) mask_mult(mask + full, lo_out, slope, v);   // the mask has out's shape, hence its hi -> lo offset; the fp32 sum meets the
                                                          // multiplier unrounded, as in add_mask: ONE rounding to T, in st_vals
    st_vals(out + full, lo_out, v);
}

int d2s_add_mask_dispatch(const void* src, const void* add, const void* mask, void* out, int n, int h, int w, int c, int dtype, float slope,
                          hipStream_t st, long lo_src, long lo_add, long lo_out) {
    const int E = dtype == RESR_F32 ? 4 : 8;
    if (!src || !out || n <= 0 || h <= 0 || w <= 0 || (h & 1) || (w & 1) || c <= 0 || (c % E)) return fail(RESR_ERR_ARG, "d2s_add_mask: bad argument");
    if (h > 65535 || n > 65535) return fail(RESR_ERR_ARG, "d2s_add_mask: image too large");
    const dim3 blocks((unsigned)(((long)w * (c / E) + 255) / 256), (unsigned)h, (unsigned)n);
    if (dtype != RESR_F32)
        hipLaunchKernelGGL(d2s_add_mask_kernel<half_t>, blocks, dim3(256), 0, st, (const half_t*)src, (const half_t*)add, (const half_t*)mask, (half_t*)out, n, h, w, c, slope,
                           lo_src, lo_add, lo_out);
    else
        hipLaunchKernelGGL(d2s_add_mask_kernel<float>, blocks, dim3(256), 0, st, (const float*)src, (const float*)add, (const float*)mask, (float*)out, n, h, w, c, slope,
                           0L, 0L, 0L);
    RESR_CHECK_LAUNCH("d2s_add_mask_kernel");
    return RESR_OK;
}

int s2d_dispatch(const void* src, void* dst, int n, int h, int w, int c, int dtype, int inverse, hipStream_t st) {
    const int E = dtype == RESR_F32 ? 4 : 8;
    if (!src || !dst || n <= 0 || h <= 0 || w <= 0 || (h & 1) || (w & 1) || c <= 0 || (c % E))
        return fail(RESR_ERR_ARG, "space_to_depth: bad argument");
    if (dtype == RESR_F16X2) n *= 2;   // hi and lo as one batch (the lo tensor directly follows the hi tensor)
    if (h > 65535 || n > 65535) return fail(RESR_ERR_ARG, "space_to_depth: image too large");
    const dim3 blocks((unsigned)(((long)w * (c / E) + 255) / 256), (unsigned)h, (unsigned)n);
    if (dtype != RESR_F32) hipLaunchKernelGGL(s2d_kernel<half_t>, blocks, dim3(256), 0, st, (const half_t*)src, (half_t*)dst, n, h, w, c, inverse);
    else hipLaunchKernelGGL(s2d_kernel<float>, blocks, dim3(256), 0, st, (const float*)src, (float*)dst, n, h, w, c, inverse);
    RESR_CHECK_LAUNCH("s2d_kernel");
    return RESR_OK;
}

// torch upsample_bilinear2d, scale 2, align_corners=False: src = (o + 0.5) * 0.5 - 0.5, clamped at 0
__device__ __forceinline__ void bil_coord(int o, int n, int& i0, int& i1, float& l) {
    float f = (o + 0.5f) * 0.5f - 0.5f;
    if (f < 0.f) f = 0.f;
    i0 = (int)f;
    i1 = i0 + (i0 < n - 1 ? 1 : 0);
    l = f - i0;
}

// Index math of these helpers: rows and images come from blockIdx.y / blockIdx.z, (pixel, 16-byte group) inside the row from one
// 32-bit division -- decoded from one flat 64-bit thread index they were three emulated 64-bit divisions per 16 bytes of output,
// and the kernels ran at a quarter of the HBM rate.
template <typename T>
__global__ __launch_bounds__(256) void bilinear_up_kernel(const T* __restrict__ src, T* __restrict__ dst, int n, int h, int w,
                                                          int c, long lo_src, long lo_dst) {
    constexpr int E = 16 / (int)sizeof(T);
    const unsigned groups = (unsigned)c / E, ow = 2u * w;
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;      // (ox, g) inside the output row
    if (idx >= ow * groups) return;
    const unsigned ox = idx / groups, g = idx - ox * groups;
    const int oy = (int)blockIdx.y, b = (int)blockIdx.z, oh = 2 * h;
    int y0, y1, x0, x1;
    float ly, lx;
    bil_coord(oy, h, y0, y1, ly);
    bil_coord((int)ox, w, x0, x1, lx);
    const float hy = 1.f - ly, hx = 1.f - lx;
    const T* base = src + (size_t)b * h * w * c + g * E;
    float a[E], bq[E], cq[E], d[E], o[E];
    ld_vals(base + ((size_t)y0 * w + x0) * c, lo_src, a);
    ld_vals(base + ((size_t)y0 * w + x1) * c, lo_src, bq);
    ld_vals(base + ((size_t)y1 * w + x0) * c, lo_src, cq);
    ld_vals(base + ((size_t)y1 * w + x1) * c, lo_src, d);
#pragma unroll
    for (int e = 0; e < E; ++e) o[e] = hy * (hx * a[e] + lx * bq[e]) + ly * (hx * cq[e] + lx * d[e]);
    st_vals(dst + (((size_t)b * oh + oy) * ow + ox) * c + g * E, lo_dst, o);
}

// The same outputs, four per thread: the output quad rows {2y+1, 2y+2} x columns {2x+1, 2x+2} interpolates between the SAME four
// source pixels (y, y+1) x (x, x+1) with weights 0.25 / 0.75 -- four 16-byte loads for four 16-byte stores instead of four for one
// (the one-output kernel spent its time in the texture-address path: 2.8 TB/s on 335 MB).  Quads y = -1 / x = -1 (output row /
// column 0) and the quads of the last source row / column take the one-output path per pixel (their clamped coordinates); the
// interior arithmetic is bil_coord's, term for term: bit-identical outputs.
template <typename T>
__global__ __launch_bounds__(256) void bilinear_up_quad_kernel(const T* __restrict__ src, T* __restrict__ dst, int n, int h, int w,
                                                               int c, long lo_src, long lo_dst) {
    constexpr int E = 16 / (int)sizeof(T);
    const unsigned groups = (unsigned)c / E, ow = 2u * w;
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;      // (quad column + 1, g) inside the quad row
    if (idx >= (unsigned)(w + 1) * groups) return;
    const unsigned qx1 = idx / groups, g = idx - qx1 * groups;
    const int x = (int)qx1 - 1, y = (int)blockIdx.y - 1, b = (int)blockIdx.z, oh = 2 * h;
    const T* base = src + (size_t)b * h * w * c + g * E;
    T* obase = dst + (size_t)b * oh * ow * c + g * E;
    if (y >= 0 && y < h - 1 && x >= 0 && x < w - 1) {
        float a[E], bq[E], cq[E], d[E], o[E];
        ld_vals(base + ((size_t)y * w + x) * c, lo_src, a);
        ld_vals(base + ((size_t)y * w + x + 1) * c, lo_src, bq);
        ld_vals(base + ((size_t)(y + 1) * w + x) * c, lo_src, cq);
        ld_vals(base + ((size_t)(y + 1) * w + x + 1) * c, lo_src, d);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const float ly = r ? 0.75f : 0.25f, hy = 1.f - ly;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const float lx = q ? 0.75f : 0.25f, hx = 1.f - lx;
#pragma unroll
                for (int e = 0; e < E; ++e) o[e] = hy * (hx * a[e] + lx * bq[e]) + ly * (hx * cq[e] + lx * d[e]);
                st_vals(obase + ((size_t)(2 * y + 1 + r) * ow + (2 * x + 1 + q)) * c, lo_dst, o);
            }
        }
        return;
    }
#pragma unroll 1
    for (int r = 0; r < 2; ++r) {
        const int oy = 2 * y + 1 + r;
        if (oy < 0 || oy >= oh) continue;
#pragma unroll 1
        for (int q = 0; q < 2; ++q) {
            const int ox = 2 * x + 1 + q;
            if (ox < 0 || ox >= (int)ow) continue;
            int y0, y1, x0, x1;
            float ly, lx;
            bil_coord(oy, h, y0, y1, ly);
            bil_coord(ox, w, x0, x1, lx);
            const float hy = 1.f - ly, hx = 1.f - lx;
            float a[E], bq[E], cq[E], d[E], o[E];
            ld_vals(base + ((size_t)y0 * w + x0) * c, lo_src, a);
            ld_vals(base + ((size_t)y0 * w + x1) * c, lo_src, bq);
            ld_vals(base + ((size_t)y1 * w + x0) * c, lo_src, cq);
            ld_vals(base + ((size_t)y1 * w + x1) * c, lo_src, d);
#pragma unroll
            for (int e = 0; e < E; ++e) o[e] = hy * (hx * a[e] + lx * bq[e]) + ly * (hx * cq[e] + lx * d[e]);
            st_vals(obase + ((size_t)oy * ow + ox) * c, lo_dst, o);
        }
    }
}

// backward as a gather: input pixel (y,x) collects from the <= 4x4 outputs whose stencil touches it
// optional second output: gmasked = gin * (mask > 0 ? 1 : slope) (the LeakyReLU backward that follows in the discriminator; gin
// itself is kept, it is a skip gradient later) -- computed from the rounded gin, like a separate add_mask pass would
template <typename T>
__global__ __launch_bounds__(256) void bilinear_up_bwd_kernel(const T* __restrict__ g, T* __restrict__ gin, int n, int h, int w,
                                                              int c, const T* __restrict__ mask, T* __restrict__ gmasked,
                                                              float slope, long lo_g, long lo_gin) {
    constexpr int E = 16 / (int)sizeof(T);
    const unsigned groups = (unsigned)c / E;
    const int oh = 2 * h, ow = 2 * w;
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;      // (x, group) inside the input row
    if (idx >= (unsigned)w * groups) return;
    const int x = (int)(idx / groups), gi = (int)(idx - (unsigned)x * groups);
    const int y = (int)blockIdx.y, b = (int)blockIdx.z;
    // the outputs whose stencil touches (y, x): rows 2y-1 .. 2y+2, columns 2x-1 .. 2x+2 (the clamp at 0 and the repeated last
    // row / column only change their weights); weights once per row / column, same products and order as the 5 x 5 scan had
    float wy[4], wx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int oy = 2 * y - 1 + k, ox = 2 * x - 1 + k;
        int i0, i1;
        float l;
        wy[k] = 0.f;
        if (oy >= 0 && oy < oh) {
            bil_coord(oy, h, i0, i1, l);
            wy[k] = (i0 == y ? 1.f - l : 0.f) + (i1 == y ? l : 0.f);
        }
        wx[k] = 0.f;
        if (ox >= 0 && ox < ow) {
            bil_coord(ox, w, i0, i1, l);
            wx[k] = (i0 == x ? 1.f - l : 0.f) + (i1 == x ? l : 0.f);
        }
    }
    float acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.f;
    const T* base = g + (size_t)b * oh * ow * c + gi * E;
#pragma unroll
    for (int ky = 0; ky < 4; ++ky) {
        if (wy[ky] == 0.f) continue;
        const int oy = 2 * y - 1 + ky;
#pragma unroll
        for (int kx = 0; kx < 4; ++kx) {
            if (wx[kx] == 0.f) continue;
            const int ox = 2 * x - 1 + kx;
            float v[E];
            ld_vals(base + ((size_t)oy * ow + ox) * c, lo_g, v);
#pragma unroll
            for (int e = 0; e < E; ++e) acc[e] += wy[ky] * wx[kx] * v[e];
        }
    }
    const size_t po = (((size_t)b * h + y) * w + x) * c + gi * E;
    st_vals(gin + po, lo_gin, acc);
    if (gmasked) {
        float m[E];
#pragma unroll
        for (int e = 0; e < E; ++e) m[e] = lo_gin ? acc[e] : (float)(T)acc[e];
        mask_mult(mask + po, lo_gin, slope, m);
        st_vals(gmasked + po, lo_gin, m);   // the same shape as gin: the same hi -> lo offset
    }
}

int bilinear_up_bwd_mask_dispatch(const void* g, void* gin, const void* mask, void* gmasked, int n, int h, int w, int c, int dtype, float slope,
                                  hipStream_t st, long lo_g, long lo_gin) {
    const int E = dtype == RESR_F32 ? 4 : 8;
    if (!g || !gin || !mask || !gmasked || n <= 0 || h <= 0 || w <= 0 || c <= 0 || (c % E)) return fail(RESR_ERR_ARG, "bilinear_up_bwd_mask: bad argument");
    if (h > 32767 || n > 65535) return fail(RESR_ERR_ARG, "bilinear_up_bwd_mask: image too large");
    const dim3 grid((unsigned)(((long)w * (c / E) + 255) / 256), (unsigned)h, (unsigned)n);
    if (dtype != RESR_F32)
        hipLaunchKernelGGL(bilinear_up_bwd_kernel<half_t>, grid, dim3(256), 0, st, (const half_t*)g, (half_t*)gin, n, h, w, c, (const half_t*)mask, (half_t*)gmasked, slope,
                           lo_g, lo_gin);
    else
        hipLaunchKernelGGL(bilinear_up_bwd_kernel<float>, grid, dim3(256), 0, st, (const float*)g, (float*)gin, n, h, w, c, (const float*)mask, (float*)gmasked, slope,
                           0L, 0L);
    RESR_CHECK_LAUNCH("bilinear_up_bwd_kernel");
    return RESR_OK;
}

int bilinear_up_dispatch(const void* src, void* dst, int n, int h, int w, int c, int dtype, int backward, hipStream_t st, long lo_src, long lo_dst) {
    const int E = dtype == RESR_F32 ? 4 : 8;
    if (!src || !dst || n <= 0 || h <= 0 || w <= 0 || c <= 0 || (c % E)) return fail(RESR_ERR_ARG, "bilinear_up2x: bad argument");
    if (h > 32767 || n > 65535) return fail(RESR_ERR_ARG, "bilinear_up2x: image too large");
    const dim3 gf((unsigned)((2L * w * (c / E) + 255) / 256), (unsigned)(2 * h), (unsigned)n);   // forward: one thread per output piece
    const dim3 gb((unsigned)(((long)w * (c / E) + 255) / 256), (unsigned)h, (unsigned)n);       // backward: per input piece
    const dim3 gq((unsigned)(((long)(w + 1) * (c / E) + 255) / 256), (unsigned)(h + 1), (unsigned)n);   // forward: one thread per output quad piece
    static const bool one_px = getenv("RESR_BILINEAR_ONE_PX") != nullptr;                                 // the one-output-per-thread forward kernel (A/B)
    if (dtype != RESR_F32) {
        if (!backward && !one_px) hipLaunchKernelGGL(bilinear_up_quad_kernel<half_t>, gq, dim3(256), 0, st, (const half_t*)src, (half_t*)dst, n, h, w, c, lo_src, lo_dst);
        else if (!backward) hipLaunchKernelGGL(bilinear_up_kernel<half_t>, gf, dim3(256), 0, st, (const half_t*)src, (half_t*)dst, n, h, w, c, lo_src, lo_dst);
        else hipLaunchKernelGGL(bilinear_up_bwd_kernel<half_t>, gb, dim3(256), 0, st, (const half_t*)src, (half_t*)dst, n, h, w, c, (const half_t*)nullptr, (half_t*)nullptr, 0.f, lo_src, lo_dst);
    } else {
        if (!backward) hipLaunchKernelGGL(bilinear_up_kernel<float>, gf, dim3(256), 0, st, (const float*)src, (float*)dst, n, h, w, c, 0L, 0L);
        else hipLaunchKernelGGL(bilinear_up_bwd_kernel<float>, gb, dim3(256), 0, st, (const float*)src, (float*)dst, n, h, w, c, (const float*)nullptr, (float*)nullptr, 0.f, 0L, 0L);
    }
    RESR_CHECK_LAUNCH("bilinear_up_kernel");
    return RESR_OK;
}

// out = (a + b) * (mask > 0 ? 1 : slope)      (b, mask optional)
template <typename T>
__global__ __launch_bounds__(256) void add_mask_kernel(const T* __restrict__ a, const T* __restrict__ b, const T* __restrict__ mask,
                                                       T* __restrict__ out, long count, float slope, long lo) {
    constexpr int E = 16 / (int)sizeof(T);
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * E;
    if (i >= count) return;
    float v[E], vb[E];
    ld_vals(a + i, lo, v);
    if (b) {
        ld_vals(b + i, lo, vb);
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] += vb[e];
    }
    if (mask) mask_mult(mask + i, 0L, slope, v);   // hi tensor only: the C-ABI gives no lo offset for the mask (it may be a view of a larger batch)
    st_vals(out + i, lo, v);
}

// RESR_F16X2: a, b, out are pairs with the lo tensor `count` elements behind the hi tensor
int add_mask_dispatch(const void* a, const void* b, const void* mask, void* out, long count, int dtype, float slope, hipStream_t st) {
    const int E = dtype == RESR_F32 ? 4 : 8;
    if (!a || !out || count <= 0 || (count % E)) return fail(RESR_ERR_ARG, "add_mask: bad argument");
    const unsigned blocks = (unsigned)((count / E + 255) / 256);
    if (dtype != RESR_F32) hipLaunchKernelGGL(add_mask_kernel<half_t>, dim3(blocks), dim3(256), 0, st, (const half_t*)a, (const half_t*)b, (const half_t*)mask, (half_t*)out, count, slope,
                                              dtype == RESR_F16X2 ? count : 0L);
    else hipLaunchKernelGGL(add_mask_kernel<float>, dim3(blocks), dim3(256), 0, st, (const float*)a, (const float*)b, (const float*)mask, (float*)out, count, slope, 0L);
    RESR_CHECK_LAUNCH("add_mask_kernel");
    return RESR_OK;
}

// sum |a - b| over `count` elements as per-workgroup partial sums (fixed grid, fixed order: deterministic; the caller adds the
// partials): the L1 distance of two halves of a feature batch (perceptual loss, reference model.py:320-327) in one pass over the
// 16-bit tensors -- as torch ops it was two f16 -> f32 copies of the whole batch, a subtraction, an abs and a reduction per node.
template <typename T>
__global__ __launch_bounds__(256) void l1_partial_kernel(const T* __restrict__ a, const T* __restrict__ b, long count, long lo, float* __restrict__ partial) {
    constexpr int E = 16 / (int)sizeof(T);
    float acc = 0.f;
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * E; i < count; i += (long)gridDim.x * 256 * E) {
        float va[E], vb[E];
        ld_vals(a + i, lo, va);
        ld_vals(b + i, lo, vb);
#pragma unroll
        for (int e = 0; e < E; ++e) acc += fabsf(va[e] - vb[e]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    __shared__ float wsum[4];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

int l1_partial_dispatch(const void* a, const void* b, long count, int dtype, long lo, float* partial, int nblocks, hipStream_t st) {
    const int E = dtype == RESR_F32 ? 4 : 8;
    if (!a || !b || !partial || count <= 0 || (count % E) || nblocks <= 0) return fail(RESR_ERR_ARG, "l1_partial: bad argument");
    if (dtype != RESR_F32) hipLaunchKernelGGL(l1_partial_kernel<half_t>, dim3(nblocks), dim3(256), 0, st, (const half_t*)a, (const half_t*)b, count, dtype == RESR_F16X2 ? lo : 0L, partial);
    else hipLaunchKernelGGL(l1_partial_kernel<float>, dim3(nblocks), dim3(256), 0, st, (const float*)a, (const float*)b, count, 0L, partial);
    RESR_CHECK_LAUNCH("l1_partial_kernel");
    return RESR_OK;
}

// 2x2 / stride-2 max pooling on NHWC (VGG19 perceptual branch, reference model.py:296-298); arg (optional, uint8 per element):
// which of the four window positions (dy * 2 + dx, first maximum in that order -- ATen's max_pool2d picks the same) won, for the
// backward pass of a differentiable perceptual term
template <typename T>
__global__ __launch_bounds__(256) void maxpool2x2_kernel(const T* __restrict__ src, T* __restrict__ dst, int n, int ho, int wo, int c, long lo_src,
                                                         long lo_dst, uint8_t* __restrict__ arg) {
    constexpr int E = 16 / (int)sizeof(T);
    const int groups = c / E;
    const long total = (long)n * ho * wo * groups;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int g = (int)(t % groups);
    const long p = t / groups;
    const int x = (int)(p % wo), y = (int)((p / wo) % ho), b = (int)(p / ((long)wo * ho));
    const int wi = wo * 2;
    const T* s = src + (((size_t)b * ho * 2 + y * 2) * wi + x * 2) * c + g * E;
    float m[E];
    uint8_t am[E];
#pragma unroll
    for (int e = 0; e < E; ++e) { m[e] = -3.4e38f; am[e] = 0; }
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            float v[E];
            ld_vals(s + ((size_t)dy * wi + dx) * c, lo_src, v);
#pragma unroll
            for (int e = 0; e < E; ++e)
                if (v[e] > m[e]) { m[e] = v[e]; am[e] = (uint8_t)(dy * 2 + dx); }
        }
    st_vals(dst + p * c + g * E, lo_dst, m);
    if (arg) {
#pragma unroll
        for (int e = 0; e < E; ++e) arg[p * c + g * E + e] = am[e];
    }
}

int maxpool2x2_dispatch(const void* src, void* dst, int n, int ho, int wo, int c, int dtype, hipStream_t st, long lo_src, long lo_dst, uint8_t* arg) {
    const int E = dtype == RESR_F32 ? 4 : 8;
    if (!src || !dst || n <= 0 || ho <= 0 || wo <= 0 || c <= 0 || (c % E)) return fail(RESR_ERR_ARG, "maxpool2x2: bad argument");
    const long total = (long)n * ho * wo * (c / E);
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (dtype != RESR_F32) hipLaunchKernelGGL(maxpool2x2_kernel<half_t>, dim3(blocks), dim3(256), 0, st, (const half_t*)src, (half_t*)dst, n, ho, wo, c, lo_src, lo_dst, arg);
    else hipLaunchKernelGGL(maxpool2x2_kernel<float>, dim3(blocks), dim3(256), 0, st, (const float*)src, (float*)dst, n, ho, wo, c, 0L, 0L, arg);
    RESR_CHECK_LAUNCH("maxpool2x2_kernel");
    return RESR_OK;
}

// backward of maxpool2x2: the gradient of an output element goes to the window position that won (arg), zeros elsewhere
template <typename T>
__global__ __launch_bounds__(256) void maxpool2x2_bwd_kernel(const T* __restrict__ g, const uint8_t* __restrict__ arg, T* __restrict__ gin, int n,
                                                             int ho, int wo, int c, long lo_g, long lo_gin) {
    constexpr int E = 16 / (int)sizeof(T);
    const int groups = c / E;
    const long total = (long)n * ho * wo * groups;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int gq = (int)(t % groups);
    const long p = t / groups;
    const int x = (int)(p % wo), y = (int)((p / wo) % ho), b = (int)(p / ((long)wo * ho));
    const int wi = wo * 2;
    float v[E];
    ld_vals(g + p * c + gq * E, lo_g, v);
    uint8_t am[E];
#pragma unroll
    for (int e = 0; e < E; ++e) am[e] = arg[p * c + gq * E + e];
    T* d = gin + (((size_t)b * ho * 2 + y * 2) * wi + x * 2) * c + gq * E;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            float o[E];
#pragma unroll
            for (int e = 0; e < E; ++e) o[e] = am[e] == dy * 2 + dx ? v[e] : 0.f;
            st_vals(d + ((size_t)dy * wi + dx) * c, lo_gin, o);
        }
}

int maxpool2x2_bwd_dispatch(const void* g, const uint8_t* arg, void* gin, int n, int ho, int wo, int c, int dtype, hipStream_t st, long lo_g, long lo_gin) {
    const int E = dtype == RESR_F32 ? 4 : 8;
    if (!g || !arg || !gin || n <= 0 || ho <= 0 || wo <= 0 || c <= 0 || (c % E)) return fail(RESR_ERR_ARG, "maxpool2x2_bwd: bad argument");
    const long total = (long)n * ho * wo * (c / E);
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (dtype != RESR_F32) hipLaunchKernelGGL(maxpool2x2_bwd_kernel<half_t>, dim3(blocks), dim3(256), 0, st, (const half_t*)g, arg, (half_t*)gin, n, ho, wo, c, lo_g, lo_gin);
    else hipLaunchKernelGGL(maxpool2x2_bwd_kernel<float>, dim3(blocks), dim3(256), 0, st, (const float*)g, arg, (float*)gin, n, ho, wo, c, 0L, 0L);
    RESR_CHECK_LAUNCH("maxpool2x2_bwd_kernel");
    return RESR_OK;
}

// ---- spectral norm -----------------------------------------------------------------------------------------------
// W is [rows = cout][cols = cin*k*k] row-major fp32 (the OIHW parameter viewed as a matrix).  The power iteration of ALL
// normalised layers of a discriminator call runs as four launches (W^T u partials / normalise v / W v / normalise u + sigma),
// every launch covering up to kSnMaxLayers layers through a table in its arguments: one layer at a time it was 32 dependent
// launches of 5-10 us per call, three calls per GAN step (train_realesrgan.py:479,500,508).
// W^T u in row groups of kSnRows: part[g][k] = sum over the group's rows of W[r][k] * u[r] -- (cols / 256) x (rows / 32)
// workgroups per layer (a 512 x 4608 matrix as cols / 256 workgroups was 18 workgroups of 512 dependent loads each: 71 us);
// the groups are summed in a fixed order by the normalisation kernel -- no atomics, so every rank computes bit-identical v.
constexpr int kSnRows = 32;
constexpr int kSnMaxLayers = 8;
struct SnLayer {
    const float* W;
    float* u;
    float* v;
    float* sigma2;   // [2]: sigma, 1 / sigma
    float* wv;       // [rows] scratch
    float* vraw;     // [groups][cols] scratch
    int rows, cols, groups;
    int first_a, first_b;   // first workgroup of this layer in the W^T u launch / in the W v launch
    int first_c;            // ... in the launch that adds the groups' partial vectors
};
struct SnArgs {
    SnLayer l[kSnMaxLayers];
    int n;
    float eps;
};

__device__ __forceinline__ int sn_layer_of(const SnArgs& a, int block, bool wv_launch) {
    int li = 0;
    while (li + 1 < a.n && block >= (wv_launch ? a.l[li + 1].first_b : a.l[li + 1].first_a)) ++li;
    return li;
}

// vraw[0][k] = sum over the groups of vraw[g][k], one thread per column, groups in ascending order.  (As a loop inside the
// one-workgroup-per-layer normalisation this was 16 groups x 18 columns of dependent loads per thread: 62 us per call for the
// 512 x 4608 layer; the sums and everything after them are unchanged.)
__global__ __launch_bounds__(256) void sn_sum_groups_kernel(const SnArgs a) {
    int li = 0;
    while (li + 1 < a.n && (int)blockIdx.x >= a.l[li + 1].first_c) ++li;
    const SnLayer& L = a.l[li];
    const int k = ((int)blockIdx.x - L.first_c) * 256 + (int)threadIdx.x;
    if (k >= L.cols) return;
    float t = L.vraw[k];
    for (int g = 1; g < L.groups; ++g) t += L.vraw[(size_t)g * L.cols + k];
    L.vraw[k] = t;
}

__global__ __launch_bounds__(256) void sn_wt_u_kernel(const SnArgs a) {
    const int li = sn_layer_of(a, blockIdx.x, false);
    const SnLayer& L = a.l[li];
    const int local = blockIdx.x - L.first_a;
    const int bx = (L.cols + 255) / 256;
    const int k = (local % bx) * 256 + threadIdx.x, grp = local / bx;
    if (k >= L.cols) return;
    const float* __restrict__ W = L.W;
    const float* __restrict__ u = L.u;
    const int r0 = grp * kSnRows, r1 = min(L.rows, r0 + kSnRows);
    const int cols = L.cols;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int r = r0;
    for (; r + 4 <= r1; r += 4) {
        s0 += W[(size_t)r * cols + k] * u[r];
        s1 += W[(size_t)(r + 1) * cols + k] * u[r + 1];
        s2 += W[(size_t)(r + 2) * cols + k] * u[r + 2];
        s3 += W[(size_t)(r + 3) * cols + k] * u[r + 3];
    }
    for (; r < r1; ++r) s0 += W[(size_t)r * cols + k] * u[r];
    L.vraw[(size_t)grp * cols + k] = (s0 + s1) + (s2 + s3);
}

static __device__ float block_sum(float v, float* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
    return t;
}

// one workgroup per layer.  which = 0: src = W^T u (the groups' partial vectors already added by sn_sum_groups_kernel), v = src /
// max(||src||, eps).  which = 1: src = W v, u = src / max(||src||, eps), sigma = dot(u, src), sigma2 = (sigma, 1 / sigma).
__global__ __launch_bounds__(256) void sn_normalize_kernel(const SnArgs a, int which) {
    __shared__ float red[4];
    const SnLayer& L = a.l[blockIdx.x];
    float* src = which ? L.wv : L.vraw;
    float* dst = which ? L.u : L.v;
    const int n = which ? L.rows : L.cols;
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float t = src[i];
        s += t * t;
    }
    const float nrm = sqrtf(block_sum(s, red));
    const float inv = 1.f / fmaxf(nrm, a.eps);
    float d = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float v = src[i] * inv;
        dst[i] = v;
        d += v * src[i];
    }
    if (which) {
        const float dot = block_sum(d, red);
        if (threadIdx.x == 0) { L.sigma2[0] = dot; L.sigma2[1] = 1.f / dot; }
    }
}

__global__ __launch_bounds__(256) void sn_w_v_kernel(const SnArgs a) {
    __shared__ float red[4];
    const int li = sn_layer_of(a, blockIdx.x, true);
    const SnLayer& L = a.l[li];
    const int r = blockIdx.x - L.first_b;
    const float* __restrict__ W = L.W;
    const float* __restrict__ v = L.v;
    float s = 0.f;
    for (int k = threadIdx.x; k < L.cols; k += 256) s += W[(size_t)r * L.cols + k] * v[k];
    const float t = block_sum(s, red);
    if (threadIdx.x == 0) L.wv[r] = t;
}

// sigma = u . wv (eval mode: u, v are not updated); one workgroup per layer
__global__ __launch_bounds__(256) void sn_dot_kernel(const SnArgs a) {
    __shared__ float red[4];
    const SnLayer& L = a.l[blockIdx.x];
    float s = 0.f;
    for (int i = threadIdx.x; i < L.rows; i += 256) s += L.u[i] * L.wv[i];
    const float t = block_sum(s, red);
    if (threadIdx.x == 0) { L.sigma2[0] = t; L.sigma2[1] = 1.f / t; }
}

// `n` layers (<= kSnMaxLayers) at once: W[i] [rows[i]][cols[i]], u[i], v[i], sigma2[i] (2 floats), tmp[i] = rows + ceil(rows/32) * cols floats
int spectral_norm_batch_dispatch(int n, const float* const* W, float* const* u, float* const* v, const int* rows, const int* cols, int training,
                                 float eps, float* const* sigma2, float* const* tmp, hipStream_t st) {
    if (n <= 0 || n > kSnMaxLayers || !W || !u || !v || !rows || !cols || !sigma2 || !tmp) return fail(RESR_ERR_ARG, "spectral_norm: bad argument");
    SnArgs a;
    memset(&a, 0, sizeof(a));
    a.n = n; a.eps = eps;
    int na = 0, nb = 0, nc = 0;
    for (int i = 0; i < n; ++i) {
        if (!W[i] || !u[i] || !v[i] || !sigma2[i] || !tmp[i] || rows[i] <= 0 || cols[i] <= 0) return fail(RESR_ERR_ARG, "spectral_norm: bad argument");
        SnLayer& L = a.l[i];
        L.W = W[i]; L.u = u[i]; L.v = v[i]; L.sigma2 = sigma2[i];
        L.rows = rows[i]; L.cols = cols[i]; L.groups = (rows[i] + kSnRows - 1) / kSnRows;
        L.wv = tmp[i]; L.vraw = tmp[i] + rows[i];
        L.first_a = na; L.first_b = nb; L.first_c = nc;
        na += ((cols[i] + 255) / 256) * L.groups;
        nb += rows[i];
        nc += (cols[i] + 255) / 256;
    }
    if (training) {               // one power iteration, u and v updated in place (torch spectral_norm, training forward)
        hipLaunchKernelGGL(sn_wt_u_kernel, dim3(na), dim3(256), 0, st, a);
        hipLaunchKernelGGL(sn_sum_groups_kernel, dim3(nc), dim3(256), 0, st, a);
        hipLaunchKernelGGL(sn_normalize_kernel, dim3(n), dim3(256), 0, st, a, 0);
        hipLaunchKernelGGL(sn_w_v_kernel, dim3(nb), dim3(256), 0, st, a);
        hipLaunchKernelGGL(sn_normalize_kernel, dim3(n), dim3(256), 0, st, a, 1);   // sigma = u_new . (W v_new)
    } else {
        hipLaunchKernelGGL(sn_w_v_kernel, dim3(nb), dim3(256), 0, st, a);
        hipLaunchKernelGGL(sn_dot_kernel, dim3(n), dim3(256), 0, st, a);
    }
    RESR_CHECK_LAUNCH("spectral_norm kernels");
    return RESR_OK;
}

int spectral_norm_dispatch(const float* W, float* u, float* v, int rows, int cols, int training, float eps, float* sigma2,
                           float* tmp, hipStream_t st) {
    return spectral_norm_batch_dispatch(1, &W, &u, &v, &rows, &cols, training, eps, &sigma2, &tmp, st);
}

// backward of W = W_orig / sigma, sigma = u^T W_orig v (u, v constants):
//   dW_orig = G / sigma - (<G, W_orig> / sigma^2) * u v^T          (accumulated into dst when accumulate != 0)
__global__ __launch_bounds__(256) void sn_bwd_dot_kernel(const float* __restrict__ G, const float* __restrict__ W, long count,
                                                         float* __restrict__ dot) {
    __shared__ float red[4];
    float s = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256) s += G[i] * W[i];
    const float t = block_sum(s, red);
    if (threadIdx.x == 0) dot[blockIdx.x] = t;   // one partial per block, summed in a fixed order by the apply kernel (no atomics:
                                                 // the discriminator's gradients are bit-reproducible from run to run)
}

__global__ __launch_bounds__(256) void sn_bwd_apply_kernel(const float* __restrict__ G, const float* __restrict__ u,
                                                           const float* __restrict__ v, const float* __restrict__ sigma2,
                                                           const float* __restrict__ dot, int ndot, float* __restrict__ dst, int cols,
                                                           long count, int accumulate) {
    __shared__ float red[4];
    // <G, W>: every block adds the ndot (<= 512) partials in the same order
    float part = 0.f;
    for (int k = threadIdx.x; k < ndot; k += 256) part += dot[k];
    const float gw = block_sum(part, red);
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int r = (int)(i / cols), k = (int)(i % cols);
    const float inv = sigma2[1];
    const float val = G[i] * inv - gw * inv * inv * u[r] * v[k];
    dst[i] = accumulate ? dst[i] + val : val;
}

int spectral_norm_bwd_dispatch(const float* G, const float* W, const float* u, const float* v, const float* sigma2, float* dst,
                               int rows, int cols, int accumulate, float* tmp1, hipStream_t st) {
    if (!G || !W || !u || !v || !sigma2 || !dst || !tmp1 || rows <= 0 || cols <= 0) return fail(RESR_ERR_ARG, "spectral_norm_bwd: bad argument");
    const long count = (long)rows * cols;
    long blocks = (count + 255) / 256;
    if (blocks > 512) blocks = 512;
    hipLaunchKernelGGL(sn_bwd_dot_kernel, dim3((unsigned)blocks), dim3(256), 0, st, G, W, count, tmp1);
    hipLaunchKernelGGL(sn_bwd_apply_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, G, u, v, sigma2, tmp1, (int)blocks, dst,
                       cols, count, accumulate);
    RESR_CHECK_LAUNCH("spectral_norm_bwd kernels");
    return RESR_OK;
}

// The same two steps for ALL normalised layers of a discriminator backward pass in two launches (and the 4x4 folds in one): 38
// launches of 5-10 us per backward were 70 per RealESRGAN step.  Same per-layer block counts and summation orders as the
// single-layer kernels above: bit-identical results.
struct SnBwdLayer {
    const float* G; const float* W; const float* u; const float* v; const float* sigma2; float* dst;
    long count; int cols; int dot0, ndot;      // first partial / number of partials of this layer in `dot`
    long ablk0;                                // first workgroup of the apply launch that belongs to this layer
};
struct SnBwdBatch {
    SnBwdLayer l[8];
    int n;
    float* dot;
};

__global__ __launch_bounds__(256) void sn_bwd_dot_batch_kernel(const SnBwdBatch a) {
    __shared__ float red[4];
    int li = 0;
    while (li + 1 < a.n && (int)blockIdx.x >= a.l[li + 1].dot0) ++li;
    const SnBwdLayer& L = a.l[li];
    const int b = (int)blockIdx.x - L.dot0;
    float s = 0.f;
    for (long i = (long)b * 256 + threadIdx.x; i < L.count; i += (long)L.ndot * 256) s += L.G[i] * L.W[i];
    const float t = block_sum(s, red);
    if (threadIdx.x == 0) a.dot[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void sn_bwd_apply_batch_kernel(const SnBwdBatch a) {
    __shared__ float red[4];
    int li = 0;
    while (li + 1 < a.n && (long)blockIdx.x >= a.l[li + 1].ablk0) ++li;
    const SnBwdLayer& L = a.l[li];
    float part = 0.f;
    for (int k = threadIdx.x; k < L.ndot; k += 256) part += a.dot[L.dot0 + k];
    const float gw = block_sum(part, red);
    const long i = ((long)blockIdx.x - L.ablk0) * 256 + threadIdx.x;
    if (i >= L.count) return;
    const int r = (int)(i / L.cols), k = (int)(i % L.cols);
    const float inv = L.sigma2[1];
    L.dst[i] = L.G[i] * inv - gw * inv * inv * L.u[r] * L.v[k];
}

// n <= 8 layers; G[i] = gradient wrt W = W_orig / sigma of layer i ([rows][cols]), dst[i] = gradient wrt W_orig; dot: 8 x 512 floats
int spectral_norm_bwd_batch_dispatch(int n, const float* const* G, const float* const* W, const float* const* u, const float* const* v,
                                     const float* const* sigma2, float* const* dst, const int* rows, const int* cols, float* dot, hipStream_t st) {
    if (n <= 0 || n > 8 || !G || !W || !u || !v || !sigma2 || !dst || !rows || !cols || !dot) return fail(RESR_ERR_ARG, "spectral_norm_bwd_batch: bad argument");
    SnBwdBatch a;
    memset(&a, 0, sizeof(a));
    a.n = n; a.dot = dot;
    int dots = 0;
    long ablk = 0;
    for (int i = 0; i < n; ++i) {
        if (!G[i] || !W[i] || !u[i] || !v[i] || !sigma2[i] || !dst[i] || rows[i] <= 0 || cols[i] <= 0)
            return fail(RESR_ERR_ARG, "spectral_norm_bwd_batch: bad argument");
        SnBwdLayer& L = a.l[i];
        L.G = G[i]; L.W = W[i]; L.u = u[i]; L.v = v[i]; L.sigma2 = sigma2[i]; L.dst = dst[i];
        L.count = (long)rows[i] * cols[i]; L.cols = cols[i];
        long blocks = (L.count + 255) / 256;
        L.ndot = (int)(blocks > 512 ? 512 : blocks);
        L.dot0 = dots; dots += L.ndot;
        L.ablk0 = ablk; ablk += blocks;
    }
    hipLaunchKernelGGL(sn_bwd_dot_batch_kernel, dim3((unsigned)dots), dim3(256), 0, st, a);
    hipLaunchKernelGGL(sn_bwd_apply_batch_kernel, dim3((unsigned)ablk), dim3(256), 0, st, a);
    RESR_CHECK_LAUNCH("spectral_norm_bwd batch kernels");
    return RESR_OK;
}

struct FoldBatch {
    const float* src[4]; float* dst[4]; int cout[4], C[4]; long blk0[5]; int n;
};
__global__ __launch_bounds__(256) void fold4x4_batch_kernel(const FoldBatch a) {
    int li = 0;
    while (li + 1 < a.n && (long)blockIdx.x >= a.blk0[li + 1]) ++li;
    const int C = a.C[li];
    const long total = (long)a.cout[li] * C * 16;
    const long t = ((long)blockIdx.x - a.blk0[li]) * 256 + threadIdx.x;
    if (t >= total) return;
    const int kx = (int)(t % 4), ky = (int)((t / 4) % 4), c = (int)((t / 16) % C), co = (int)(t / (16L * C));
    const int ty = (ky + 1) >> 1, i = (ky + 1) & 1, tx = (kx + 1) >> 1, j = (kx + 1) & 1;
    a.dst[li][t] = a.src[li][(((size_t)co * 4 * C + (i * 2 + j) * C + c) * 3 + ty) * 3 + tx];
}
int fold4x4_batch_dispatch(int n, const float* const* src, float* const* dst, const int* cout, const int* C, hipStream_t st) {
    if (n <= 0 || n > 4 || !src || !dst || !cout || !C) return fail(RESR_ERR_ARG, "fold4x4_batch: bad argument");
    FoldBatch a;
    memset(&a, 0, sizeof(a));
    a.n = n;
    long blk = 0;
    for (int i = 0; i < n; ++i) {
        if (!src[i] || !dst[i] || cout[i] <= 0 || C[i] <= 0) return fail(RESR_ERR_ARG, "fold4x4_batch: bad argument");
        a.src[i] = src[i]; a.dst[i] = dst[i]; a.cout[i] = cout[i]; a.C[i] = C[i];
        a.blk0[i] = blk; blk += ((long)cout[i] * C[i] * 16 + 255) / 256;
    }
    a.blk0[n] = blk;
    hipLaunchKernelGGL(fold4x4_batch_kernel, dim3((unsigned)blk), dim3(256), 0, st, a);
    RESR_CHECK_LAUNCH("fold4x4_batch_kernel");
    return RESR_OK;
}

// virtual [cout][4C][3][3] gradient -> real [cout][C][4][4]:  ky = 2*ty + i - 1, kx = 2*tx + j - 1, virtual ci = (i*2+j)*C + c
__global__ __launch_bounds__(256) void fold4x4_kernel(const float* __restrict__ dw3, float* __restrict__ dw4, int cout, int C) {
    const long total = (long)cout * C * 16;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int kx = (int)(t % 4), ky = (int)((t / 4) % 4), c = (int)((t / 16) % C), co = (int)(t / (16L * C));
    const int ty = (ky + 1) >> 1, i = (ky + 1) & 1, tx = (kx + 1) >> 1, j = (kx + 1) & 1;
    dw4[t] = dw3[(((size_t)co * 4 * C + (i * 2 + j) * C + c) * 3 + ty) * 3 + tx];
}

int fold4x4_dispatch(const float* dw3, float* dw4, int cout, int C, hipStream_t st) {
    if (!dw3 || !dw4 || cout <= 0 || C <= 0) return fail(RESR_ERR_ARG, "fold4x4: bad argument");
    const long total = (long)cout * C * 16;
    hipLaunchKernelGGL(fold4x4_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, dw3, dw4, cout, C);
    RESR_CHECK_LAUNCH("fold4x4_kernel");
    return RESR_OK;
}

}  // namespace resr
