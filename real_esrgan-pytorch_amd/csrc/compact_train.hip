// compact_train.hip -- the three kernels of their own that training the compact generator needs (compact.hip owns the plan and the
// launch order; DESIGN, "Compact generator: training").  All three are HBM-bound and written for bandwidth:
//   act          a = z > 0 ? z : slope[c] * z                       z, a: [pixels][64] NHWC of T (the saved pre-activation / activation)
//   act_bwd      g_z = g_a * (z > 0 ? 1 : slope[c])                 in place or not; with a slope gradient:
//                dslope[c] = sum_pixels g_a * (z > 0 ? 0 : z)       per-thread fp32 partials -> per-block [64] -> a second, one-block launch
//   residual_bwd gx[n,c,y,x] += sum_{i,j<s} gy[n,c,sy+i,sx+j]      fp32, the adjoint of the nearest-upsampled residual
// One thread owns 16 bytes of a pixel record (8 f16 / 4 f32): a record is 128 / 256 bytes, so there is no scalar tail, consecutive lanes
// touch consecutive 16 bytes, and a thread's channels follow from its lane alone -- 256 and every grid stride are multiples of the 8 / 16
// pieces of a record -- so its slopes are loaded once.  The slopes come from a 64-float table: the PReLU parameters in the fp32 arena, or
// a constant table (0.1: LeakyReLU, 0: ReLU): one code path for the three activations.  Both expressions are evaluated in fp32 and rounded
// once to T.  No floating-point atomics: every sum has a fixed order, so a backward pass gives the same bits run to run.
// Every count is 64-bit, and a thread whose index lies past the end touches no memory.
#include "host_api.h"

namespace resr {

// the constant slope tables of LeakyReLU(0.1) and ReLU (read through hipGetSymbolAddress, as wgrad.hip's zero page)
#define RESR_R8(v) v, v, v, v, v, v, v, v
#define RESR_R64(v) RESR_R8(v), RESR_R8(v), RESR_R8(v), RESR_R8(v), RESR_R8(v), RESR_R8(v), RESR_R8(v), RESR_R8(v)
__device__ __attribute__((aligned(16))) float g_compact_slopes_lrelu[64] = {RESR_R64(0.1f)};
__device__ __attribute__((aligned(16))) float g_compact_slopes_relu[64] = {RESR_R64(0.f)};
#undef RESR_R64
#undef RESR_R8

namespace {

constexpr int kDslopeMaxBlocks = 1024;   // rows of the [blocks][64] partial buffer of a slope gradient

// One fp32 product that stays one: left to itself the compiler folds the f16 conversions around it into v_fma_mixlo_f16(a, b, +0),
// and the +0 addend loses the sign of a zero product (slope 0 times a negative z is -0).  The results are defined bit for bit.
__device__ __forceinline__ float mul_f32(float a, float b) {
    float p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}

// the thread's E slopes: channels (threadIdx.x % (64 / E)) * E ...
template <int E>
__device__ __forceinline__ void load_slopes(const float* __restrict__ slopes, float (&sl)[E]) {
    const float* p = slopes + (threadIdx.x % (64 / E)) * E;
#pragma unroll
    for (int e = 0; e < E; e += 4) {
        const float4 v = *reinterpret_cast<const float4*>(p + e);
        sl[e] = v.x; sl[e + 1] = v.y; sl[e + 2] = v.z; sl[e + 3] = v.w;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void compact_act_kernel(const T* __restrict__ z, T* __restrict__ a, const float* __restrict__ slopes, int64_t pieces) {
    constexpr int E = 16 / (int)sizeof(T);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= pieces) return;
    float sl[E];
    load_slopes<E>(slopes, sl);
    const uint4 raw = *reinterpret_cast<const uint4*>(z + i * E);
    const T* v = reinterpret_cast<const T*>(&raw);
    uint4 out;
    T* o = reinterpret_cast<T*>(&out);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const float f = (float)v[e];
        o[e] = (T)(f > 0.f ? f : mul_f32(sl[e], f));
    }
    *reinterpret_cast<uint4*>(a + i * E) = out;
}

// g and gz may be the same tensor (a thread reads its 16 bytes before it writes them): no __restrict__ on the two.
// DS: the grid strides over the pieces and leaves partial[blockIdx.x][c] = the block's share of dslope[c], summed in a fixed order.
template <typename T, bool DS>
__global__ __launch_bounds__(256) void compact_act_bwd_kernel(const T* g, const T* __restrict__ z, T* gz, const float* __restrict__ slopes, int64_t pieces,
                                                              float* __restrict__ partial) {
    constexpr int E = 16 / (int)sizeof(T), P = 64 / E;
    float sl[E], acc[E];
    load_slopes<E>(slopes, sl);
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pieces; i += (int64_t)gridDim.x * 256) {
        const uint4 rg = *reinterpret_cast<const uint4*>(g + i * E);
        const uint4 rz = *reinterpret_cast<const uint4*>(z + i * E);
        const T* vg = reinterpret_cast<const T*>(&rg);
        const T* vz = reinterpret_cast<const T*>(&rz);
        uint4 out;
        T* o = reinterpret_cast<T*>(&out);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const float fg = (float)vg[e], fz = (float)vz[e];
            const bool pos = fz > 0.f;
            o[e] = (T)mul_f32(fg, pos ? 1.f : sl[e]);
            if (DS) acc[e] += fg * (pos ? 0.f : fz);
        }
        *reinterpret_cast<uint4*>(gz + i * E) = out;
    }
    if constexpr (DS) {
        __shared__ float red[256][E];
#pragma unroll
        for (int e = 0; e < E; ++e) red[threadIdx.x][e] = acc[e];
        __syncthreads();
        if (threadIdx.x < 64) {   // channel c lives in the threads r, r + P, r + 2 P ... (r = c / E), element c % E
            const int c = (int)threadIdx.x, r = c / E, e = c % E;
            float s = 0.f;
            for (int j = 0; j < 256 / P; ++j) s += red[j * P + r][e];
            partial[(size_t)blockIdx.x * 64 + c] = s;
        }
    }
}

// dslope[c] = (sum over the blocks' partials, in a fixed order) / lift.  One block of 1024: thread (q, c) adds the rows q, q + 16, ... in
// that order (the loads of eight rows in flight: a loop of single dependent loads was a memory latency per row), then channel c's 16
// sums are added in the order of q.
__global__ __launch_bounds__(1024) void compact_dslope_reduce_kernel(const float* __restrict__ partial, int nblocks, const unsigned* __restrict__ amax, float* __restrict__ dslope) {
    __shared__ float red[16][64];
    const int c = (int)(threadIdx.x & 63u), q = (int)(threadIdx.x >> 6);
    float s = 0.f;
#pragma unroll 8
    for (int b = q; b < nblocks; b += 16) s += partial[(size_t)b * 64 + c];
    red[q][c] = s;
    __syncthreads();
    if (q == 0) {
        const float post = amax ? grad_prescale(*amax, true) : 1.f;   // (exact: a power of two)
        float t = red[0][c];
#pragma unroll
        for (int k = 1; k < 16; ++k) t += red[k][c];
        dslope[c] = t * post;
    }
}

// One thread per LR pixel column, rows (n, c, y) from the (strided) y grid; every index that can pass 2^31 is 64-bit.  The sum runs
// over (i, j) in this order and is ADDED to what gx holds: the backward pass calls it on the gx that nhwc_to_nchw has just stored.
template <int S>
__global__ __launch_bounds__(256) void compact_residual_bwd_kernel(const float* __restrict__ gy, float* __restrict__ gx, int64_t rows, int w) {
    const int x = (int)(blockIdx.x * 256u + threadIdx.x);
    if (x >= w) return;
    const int64_t WS = (int64_t)w * S;
    for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {   // row = (n * 3 + c) * h + y: its S source rows are row * S + i
        const float* src = gy + row * S * WS + (int64_t)x * S;
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < S; ++i)
#pragma unroll
            for (int j = 0; j < S; ++j) s += src[i * WS + j];
        gx[row * w + x] += s;
    }
}

}  // namespace

const float* compact_const_slopes(int act) {
    void* p = nullptr;
    const hipError_t e = act == RESR_COMPACT_LRELU ? hipGetSymbolAddress(&p, HIP_SYMBOL(g_compact_slopes_lrelu)) : hipGetSymbolAddress(&p, HIP_SYMBOL(g_compact_slopes_relu));
    return e == hipSuccess ? (const float*)p : nullptr;
}

static bool aligned16(const void* p) { return ((size_t)p & 15) == 0; }

int compact_act_dispatch(const void* z, void* a, const float* slopes, int64_t pixels, int dtype, hipStream_t st) {
    if (!z || !a || !slopes || pixels <= 0 || (dtype != RESR_F16 && dtype != RESR_F32) || !aligned16(z) || !aligned16(a) || !aligned16(slopes))
        return fail(RESR_ERR_ARG, "compact_act: bad argument");
    const int64_t pieces = pixels * (dtype == RESR_F32 ? 16 : 8), blocks = (pieces + 255) / 256;
    if (blocks > 0x7fffffffL) return fail(RESR_ERR_ARG, "compact_act: %lld pixels", (long long)pixels);
    prof_before(st);
    if (dtype == RESR_F32) hipLaunchKernelGGL(compact_act_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)z, (float*)a, slopes, pieces);
    else hipLaunchKernelGGL(compact_act_kernel<half_t>, dim3((unsigned)blocks), dim3(256), 0, st, (const half_t*)z, (half_t*)a, slopes, pieces);
    prof_after(st, 32000, 0.0, (double)pixels * 128.0 * elem_size(dtype));
    RESR_CHECK_LAUNCH("compact_act_kernel");
    return RESR_OK;
}

static int64_t dslope_blocks(int64_t pixels, int dtype) {
    const int64_t blocks = (pixels * (dtype == RESR_F32 ? 16 : 8) + 255) / 256;
    return blocks < kDslopeMaxBlocks ? blocks : kDslopeMaxBlocks;
}

size_t compact_dslope_partial_bytes(int64_t pixels, int dtype) { return pixels > 0 ? (size_t)dslope_blocks(pixels, dtype) * 64 * sizeof(float) : 0; }

int compact_act_bwd_dispatch(const void* g, const void* z, void* gz, const float* slopes, int64_t pixels, int dtype, float* dslope, float* partial,
                             size_t partial_bytes, const unsigned* amax, hipStream_t st) {
    if (!g || !z || !gz || !slopes || pixels <= 0 || (dtype != RESR_F16 && dtype != RESR_F32) || !aligned16(g) || !aligned16(z) || !aligned16(gz) ||
        !aligned16(slopes))
        return fail(RESR_ERR_ARG, "compact_act_bwd: bad argument");
    const int64_t pieces = pixels * (dtype == RESR_F32 ? 16 : 8), blocks = (pieces + 255) / 256;
    if (blocks > 0x7fffffffL) return fail(RESR_ERR_ARG, "compact_act_bwd: %lld pixels", (long long)pixels);
    const double bytes = (double)pixels * 192.0 * elem_size(dtype);
    if (!dslope) {
        prof_before(st);
        if (dtype == RESR_F32)
            hipLaunchKernelGGL((compact_act_bwd_kernel<float, false>), dim3((unsigned)blocks), dim3(256), 0, st, (const float*)g, (const float*)z, (float*)gz, slopes, pieces, (float*)nullptr);
        else
            hipLaunchKernelGGL((compact_act_bwd_kernel<half_t, false>), dim3((unsigned)blocks), dim3(256), 0, st, (const half_t*)g, (const half_t*)z, (half_t*)gz, slopes, pieces, (float*)nullptr);
        prof_after(st, 32100, 0.0, bytes);
        RESR_CHECK_LAUNCH("compact_act_bwd_kernel");
        return RESR_OK;
    }
    const int64_t nb = dslope_blocks(pixels, dtype);
    if (!partial || partial_bytes < (size_t)nb * 64 * sizeof(float)) return fail(RESR_ERR_WORKSPACE, "compact_act_bwd: partial buffer %zu < %zu", partial_bytes, (size_t)nb * 64 * sizeof(float));
    prof_before(st);
    if (dtype == RESR_F32)
        hipLaunchKernelGGL((compact_act_bwd_kernel<float, true>), dim3((unsigned)nb), dim3(256), 0, st, (const float*)g, (const float*)z, (float*)gz, slopes, pieces, partial);
    else
        hipLaunchKernelGGL((compact_act_bwd_kernel<half_t, true>), dim3((unsigned)nb), dim3(256), 0, st, (const half_t*)g, (const half_t*)z, (half_t*)gz, slopes, pieces, partial);
    prof_after(st, 32101, 0.0, bytes);
    RESR_CHECK_LAUNCH("compact_act_bwd_kernel");
    prof_before(st);
    hipLaunchKernelGGL(compact_dslope_reduce_kernel, dim3(1), dim3(1024), 0, st, (const float*)partial, (int)nb, amax, dslope);
    prof_after(st, 32200, 0.0, (double)nb * 256.0);
    RESR_CHECK_LAUNCH("compact_dslope_reduce_kernel");
    return RESR_OK;
}

int compact_residual_bwd_dispatch(const float* gy, float* gx, int n, int h, int w, int s, hipStream_t st) {
    if (!gy || !gx || n <= 0 || h <= 0 || w <= 0) return fail(RESR_ERR_ARG, "compact_residual_bwd: bad argument");
    const int64_t rows = (int64_t)n * 3 * h;
    const dim3 grid((unsigned)((w + 255) / 256), (unsigned)(rows > 65535 ? 65535 : rows));
    prof_before(st);
    if (!with_scale(s, [&](auto S) { hipLaunchKernelGGL(compact_residual_bwd_kernel<S()>, grid, dim3(256), 0, st, gy, gx, rows, w); }))
        return fail(RESR_ERR_ARG, "compact_residual_bwd: upscale %d", s);
    prof_after(st, 32300 + s, 0.0, (double)rows * w * (s * s * 4.0 + 8.0));
    RESR_CHECK_LAUNCH("compact_residual_bwd_kernel");
    return RESR_OK;
}

}  // namespace resr
