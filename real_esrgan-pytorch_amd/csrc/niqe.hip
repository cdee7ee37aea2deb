// niqe.hip -- the native form of image_quality_assessment.niqe: its 36 features per block (resr_niqe_luma_*, resr_niqe_features), and,
// as an entry of its own (resr_niqe_score, at the end of this file), the tail from the features to the score: NaN-aware mean,
// covariance, pseudo-inverse, distance.  float64 wherever the torch path is float64: the results are re-orderings of its sums.
//   niqe_luma   : fp32 [B,3,H,W] or uint8 [B,H,W,3] -> the luma LEVEL of every pixel of the cropped, block-trimmed image, uint8 [B,h,w]:
//                 t = r * 65.481f; t += g * 128.553f; t += b * 24.966f; t += 16.0f; level = rint(t) -- six fp32 operations, each
//                 rounded once, in this order (contraction off); a byte enters as (float)byte / 255.0f.  tests/niqe_ref.niqe_luma_np
//                 states the same chain in numpy and is the definition.
//   niqe_half   : MATLAB imresize(y / 255, 0.5) * 255 in float64 from the levels, H pass then W pass, through banded tap tables (the
//                 rows of imgproc._resize_matrix without their zeros).  One workgroup owns a 16 x 64 output tile; the H pass of the
//                 columns it needs lives in LDS, nothing in between reaches HBM.
//   niqe_mscn   : one workgroup owns one block.  It stages the block and a 3-pixel ring (replicate padding at the image edge), applies
//                 the 49 taps to y and y * y, forms the MSCN value, keeps the MSCN block in LDS and reduces the six moments of the five
//                 maps of _block_features (the block, its products with four circular shifts INSIDE the block) in a fixed order.
//   niqe_aggd   : one wave per (block, map): rhat_norm from the moments, the first minimum of |r_gam - rhat_norm| over the grid, the
//                 features of that map.
//   niqe_stats  : one workgroup per image: the NaN-aware column means, the two-pass covariance of the rows without a NaN (one triangle,
//                 mirrored) and A = (cov_prior + cov) / 2, the centred rows walked through LDS in chunks of 112, every sum in a fixed order.
//   niqe_eig    : one workgroup per image: cyclic Jacobi on A in LDS (round-robin ordering, 18 rotations at once), pinv's cut on the
//                 eigenvalues, the quadratic form and its square root.
#include <math.h>

#include "host_api.h"
#include "luma_level.h"

namespace resr {

// ---- luma ------------------------------------------------------------------------------------------------------------------------
// niqe_level, unit_of_byte: luma_level.h (shared with fullref.hip)
template <bool U8>
__global__ __launch_bounds__(256) void niqe_luma_kernel(const void* __restrict__ src, uint8_t* __restrict__ dst, int H, int W, int crop, int oh, int ow) {
    const int x = (int)(blockIdx.x * 256u + threadIdx.x), y = (int)blockIdx.y, b = (int)blockIdx.z;
    if (x >= ow) return;
    const size_t plane = (size_t)H * (size_t)W, at = (size_t)(y + crop) * (size_t)W + (size_t)(x + crop);
    float r, g, bl;
    if (U8) {
        const uint8_t* p = (const uint8_t*)src + ((size_t)b * plane + at) * 3;
        r = unit_of_byte(p[0]);
        g = unit_of_byte(p[1]);
        bl = unit_of_byte(p[2]);
    } else {
        const float* p = (const float*)src + (size_t)b * 3 * plane + at;
        r = p[0];
        g = p[plane];
        bl = p[2 * plane];
    }
    dst[((size_t)b * (size_t)oh + (size_t)y) * (size_t)ow + (size_t)x] = niqe_level(r, g, bl);
}

int niqe_luma_dispatch(const void* src, int u8, uint8_t* dst, int n, int h, int w, int crop, int oh, int ow, hipStream_t st) {
    if (!src || !dst || n < 1 || h < 1 || w < 1 || crop < 0 || oh < 1 || ow < 1 || (int64_t)crop * 2 + oh > h || (int64_t)crop * 2 + ow > w)
        return fail(RESR_ERR_ARG, "niqe_luma: bad argument (n=%d h=%d w=%d crop=%d out %dx%d: the output must lie inside the cropped image)", n, h, w, crop, oh, ow);
    if (n > 65535 || oh > 65535) return fail(RESR_ERR_ARG, "niqe_luma: grid overflow (n=%d or out_h=%d above 65535)", n, oh);
    prof_before(st);
    const dim3 grid((unsigned)((ow + 255) / 256), (unsigned)oh, (unsigned)n);
    if (u8) hipLaunchKernelGGL(niqe_luma_kernel<true>, grid, dim3(256), 0, st, src, dst, h, w, crop, oh, ow);
    else hipLaunchKernelGGL(niqe_luma_kernel<false>, grid, dim3(256), 0, st, src, dst, h, w, crop, oh, ow);
    prof_after(st, u8 ? 34001 : 34000, 0.0, (double)n * oh * ow * (u8 ? 4.0 : 13.0));
    RESR_CHECK_LAUNCH("niqe_luma_kernel");
    return RESR_OK;
}

// ---- half-size image -------------------------------------------------------------------------------------------------------------
constexpr int kHalfTH = 16, kHalfTW = 64, kHalfTapsMax = 16;
constexpr int kHalfRW = 2 * kHalfTW + 2 * kHalfTapsMax;   // columns of the H pass one tile may keep: 160

// a band's first source position, pinned so that its p taps stay inside the axis (tables that are no band of a resize give undefined
// values, never undefined accesses)
__device__ __forceinline__ int band_start(const int32_t* start, int i, int n, int p) { return min(max(start[i], 0), n - p); }

__global__ __launch_bounds__(256) void niqe_half_kernel(const uint8_t* __restrict__ luma, double* __restrict__ out, int H, int W, int H2, int W2,
                                                        const int32_t* __restrict__ sh, const double* __restrict__ wh, int ph,
                                                        const int32_t* __restrict__ sw, const double* __restrict__ ww, int pw) {
    __shared__ double tmp[kHalfTH * kHalfRW];
    __shared__ double unit[256];   // level / 255, one float64 division per level
    unit[threadIdx.x] = (double)threadIdx.x / 255.0;
    __syncthreads();
    const int b = (int)blockIdx.z, r0 = (int)blockIdx.y * kHalfTH, c0 = (int)blockIdx.x * kHalfTW;
    const int rows = min(kHalfTH, H2 - r0), cols = min(kHalfTW, W2 - c0);
    const int lo = band_start(sw, c0, W, pw);
    const int rw = min(max(band_start(sw, c0 + cols - 1, W, pw) + pw - lo, pw), kHalfRW);   // lo + rw <= W
    const uint8_t* src = luma + (size_t)b * (size_t)H * (size_t)W;
    for (int i = (int)threadIdx.x; i < rows * rw; i += 256) {
        const int r = i / rw, c = i - r * rw;
        const int s = band_start(sh, r0 + r, H, ph);
        const double* wr = wh + (size_t)(r0 + r) * ph;
        const uint8_t* p = src + (size_t)s * W + lo + c;
        double acc = 0.0;
        for (int k = 0; k < ph; ++k) acc = fma(wr[k], unit[p[(size_t)k * W]], acc);
        tmp[r * kHalfRW + c] = acc;
    }
    __syncthreads();
    double* dst = out + (size_t)b * (size_t)H2 * (size_t)W2;
    for (int i = (int)threadIdx.x; i < rows * cols; i += 256) {
        const int r = i / cols, c = i - r * cols;
        const int s = band_start(sw, c0 + c, W, pw) - lo;
        const double* wc = ww + (size_t)(c0 + c) * pw;
        double acc = 0.0;
        for (int k = 0; k < pw; ++k) acc = fma(tmp[r * kHalfRW + min(max(s + k, 0), rw - 1)], wc[k], acc);
        dst[(size_t)(r0 + r) * W2 + c0 + c] = acc * 255.0;
    }
}

// ---- MSCN + block moments --------------------------------------------------------------------------------------------------------
constexpr int kMscnThreads = 512, kMscnWaves = kMscnThreads / 64;
constexpr int kMaps = 5, kMoments = 6, kBlockWords = kMaps * kMoments;   // per block: [map][n_neg, n_pos, sq_neg, sq_pos, abs, sq]
constexpr size_t kLdsMax = 160 * 1024;

struct NiqeWindow { double w[49]; };

// LDS of one workgroup: the wave partials, the MSCN block, the halo tile of source words
inline size_t mscn_lds_bytes(int bh, int bw, size_t word) {
    return (size_t)kMscnWaves * kBlockWords * 8 + (size_t)bh * bw * 8 + align_up((size_t)(bh + 6) * (bw + 6) * word, 8);
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// S: uint8_t (scale 1: the levels) or double (scale 2: the half-size image)
template <typename S>
__global__ __launch_bounds__(kMscnThreads) void niqe_mscn_kernel(const S* __restrict__ plane, double* __restrict__ moments, int H, int W, int bh, int bw,
                                                                  int nbw, int nblk, NiqeWindow win) {
    extern __shared__ __attribute__((aligned(16))) unsigned char niqe_lds[];
    double* red = reinterpret_cast<double*>(niqe_lds);
    double* mscn = red + kMscnWaves * kBlockWords;
    S* tile = reinterpret_cast<S*>(mscn + bh * bw);
    const int blk = (int)(blockIdx.x % (unsigned)nblk), b = (int)(blockIdx.x / (unsigned)nblk);
    const int y0 = (blk / nbw) * bh, x0 = (blk % nbw) * bw;
    const int tw = bw + 6, th = bh + 6, tid = (int)threadIdx.x;
    const S* src = plane + (size_t)b * (size_t)H * (size_t)W;
    for (int i = tid; i < th * tw; i += kMscnThreads) {
        const int ty = i / tw, tx = i - ty * tw;
        const int y = min(max(y0 - 3 + ty, 0), H - 1), x = min(max(x0 - 3 + tx, 0), W - 1);
        tile[i] = src[(size_t)y * W + x];
    }
    __syncthreads();
    const int count = bh * bw;
    for (int i = tid; i < count; i += kMscnThreads) {
        const int py = i / bw, px = i - py * bw;
        const S* t = tile + py * tw + px;
        double mu = 0.0, sq = 0.0;
#pragma unroll
        for (int dy = 0; dy < 7; ++dy)
#pragma unroll
            for (int dx = 0; dx < 7; ++dx) {
                const double v = (double)t[dy * tw + dx], w = win.w[dy * 7 + dx];
                mu = fma(w, v, mu);
                sq = fma(w, __dmul_rn(v, v), sq);
            }
        const double sigma = sqrt(fabs(__dsub_rn(sq, __dmul_rn(mu, mu))) + 1e-8);
        mscn[i] = __dsub_rn((double)t[3 * tw + 3], mu) / (sigma + 1.0);
    }
    __syncthreads();
    // moments: thread t takes elements t, t + 512, ... in that order, lanes meet in a fixed butterfly, waves are added in ascending order
    int cnt[kMaps][2];
    double sum[kMaps][4];
#pragma unroll
    for (int m = 0; m < kMaps; ++m) {
        cnt[m][0] = cnt[m][1] = 0;
        sum[m][0] = sum[m][1] = sum[m][2] = sum[m][3] = 0.0;
    }
    for (int i = tid; i < count; i += kMscnThreads) {
        const int py = i / bw, px = i - py * bw;
        const int pu = py == 0 ? bh - 1 : py - 1, pl = px == 0 ? bw - 1 : px - 1, pr = px == bw - 1 ? 0 : px + 1;
        const double v = mscn[i];
        // torch.roll(blocks, (sy, sx)): the partner of (py, px) is ((py - sy) mod bh, (px - sx) mod bw); shifts (0,1) (1,0) (1,1) (1,-1)
        const double x[kMaps] = {v, v * mscn[py * bw + pl], v * mscn[pu * bw + px], v * mscn[pu * bw + pl], v * mscn[pu * bw + pr]};
#pragma unroll
        for (int m = 0; m < kMaps; ++m) {
            const double s = __dmul_rn(x[m], x[m]);
            const bool neg = x[m] < 0.0, pos = x[m] > 0.0;
            cnt[m][0] += neg;
            cnt[m][1] += pos;
            sum[m][0] = __dadd_rn(sum[m][0], neg ? s : 0.0);
            sum[m][1] = __dadd_rn(sum[m][1], pos ? s : 0.0);
            sum[m][2] = __dadd_rn(sum[m][2], fabs(x[m]));
            sum[m][3] = __dadd_rn(sum[m][3], s);
        }
    }
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int m = 0; m < kMaps; ++m) {
        const double c0 = (double)wave_sum(cnt[m][0]), c1 = (double)wave_sum(cnt[m][1]);
        const double s0 = wave_sum(sum[m][0]), s1 = wave_sum(sum[m][1]), s2 = wave_sum(sum[m][2]), s3 = wave_sum(sum[m][3]);
        if (lane == 0) {
            double* r = red + wave * kBlockWords + m * kMoments;
            r[0] = c0; r[1] = c1; r[2] = s0; r[3] = s1; r[4] = s2; r[5] = s3;
        }
    }
    __syncthreads();
    if (tid < kBlockWords) {
        double total = 0.0;
        for (int wv = 0; wv < kMscnWaves; ++wv) total = __dadd_rn(total, red[wv * kBlockWords + tid]);
        moments[(size_t)blockIdx.x * kBlockWords + tid] = total;
    }
}

// ---- AGGD fit --------------------------------------------------------------------------------------------------------------------
// grid (blocks of the batch, 5 maps, 2 scales), one wave each.  feats [B * nblk][36]: scale s fills columns 18 s .. 18 s + 17 in the
// order of _block_features: alpha, (bl + br) / 2, then per shifted map alpha, mean, bl, br.
__global__ __launch_bounds__(64) void niqe_aggd_kernel(const double* __restrict__ moments, double* __restrict__ feats, const double* __restrict__ grid,
                                                       const double* __restrict__ r_gam, int n_grid, int nfit, double count1, double count2) {
    const int blk = (int)blockIdx.x, map = (int)blockIdx.y, scale = (int)blockIdx.z, lane = (int)threadIdx.x;
    const double* m = moments + ((size_t)scale * nfit + blk) * kBlockWords + map * kMoments;
    const double count = scale ? count2 : count1;
    // n_neg + 1e-8 is a float32 sum in the torch path: the count itself, or 1e-8f for an empty side
    const double den_neg = m[0] > 0.0 ? m[0] : (double)1e-8f, den_pos = m[1] > 0.0 ? m[1] : (double)1e-8f;
    const double left = sqrt(m[2] / den_neg), right = sqrt(m[3] / den_pos);
    const double g = left / right;
    const double mean_abs = m[4] / count;
    const double rhat = __dmul_rn(mean_abs, mean_abs) / (m[5] / count);
    const double g2 = __dmul_rn(g, g), g2p1 = __dadd_rn(g2, 1.0);
    const double rhat_norm = __dmul_rn(__dmul_rn(rhat, __dadd_rn(__dmul_rn(g2, g), 1.0)), __dadd_rn(g, 1.0)) / __dmul_rn(g2p1, g2p1);
    double best = INFINITY;
    int arg = 0x7fffffff;
    for (int i = lane; i < n_grid; i += 64) {
        const double d = fabs(__dsub_rn(r_gam[i], rhat_norm));
        if (d < best) { best = d; arg = i; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ob = __shfl_xor(best, off);
        const int oa = __shfl_xor(arg, off);
        if (ob < best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    if (lane != 0) return;
    if (arg >= n_grid) arg = 0;   // every distance NaN or infinite: torch.argmin answers with the first entry
    const double alpha = grid[arg];
    const double sc = sqrt(exp(__dsub_rn(lgamma(1.0 / alpha), lgamma(3.0 / alpha))));
    const double bl = __dmul_rn(left, sc), br = __dmul_rn(right, sc);
    double* f = feats + (size_t)blk * 36 + scale * 18;
    if (map == 0) {
        f[0] = alpha;
        f[1] = __dadd_rn(bl, br) / 2.0;
    } else {
        f += 2 + 4 * (map - 1);
        f[0] = alpha;
        f[1] = __dmul_rn(__dsub_rn(br, bl), exp(__dsub_rn(lgamma(2.0 / alpha), lgamma(1.0 / alpha))));
        f[2] = bl;
        f[3] = br;
    }
}

// ---- the features entry ----------------------------------------------------------------------------------------------------------
namespace {
struct NiqePlan {
    int h2, w2, nbw, nblk;
    int64_t nfit;                  // n * nblk
    size_t half_bytes, bytes;      // the half-size image (256-byte aligned), the whole workspace
    size_t lds1, lds2;
};

bool niqe_plan(const ResrNiqeDesc* d, NiqePlan* p) {
    if (!d) return fail(RESR_ERR_ARG, "niqe_features: null descriptor"), false;
    if (d->n < 1 || d->h < 1 || d->w < 1 || d->bh < 2 || d->bw < 2 || (d->bh & 1) || (d->bw & 1) || d->h % d->bh || d->w % d->bw)
        return fail(RESR_ERR_ARG, "niqe_features: bad descriptor (n=%d luma %dx%d, blocks %dx%d: even block sides that divide the luma)", d->n, d->h, d->w, d->bh, d->bw), false;
    const bool huge = (int64_t)d->bh * d->bw > (int64_t)kLdsMax;   // (before the sizes below are formed)
    p->lds1 = huge ? ~(size_t)0 : mscn_lds_bytes(d->bh, d->bw, 1);
    p->lds2 = huge ? ~(size_t)0 : mscn_lds_bytes(d->bh / 2, d->bw / 2, 8);
    if (p->lds1 > kLdsMax || p->lds2 > kLdsMax)
        return fail(RESR_ERR_ARG, "niqe_features: a %dx%d block needs %zu bytes of LDS (the MSCN block in float64 and its halo tile), above the %zu of a CU", d->bh, d->bw,
                    p->lds1 > p->lds2 ? p->lds1 : p->lds2, kLdsMax), false;
    p->h2 = d->h / 2;
    p->w2 = d->w / 2;
    p->nbw = d->w / d->bw;
    p->nblk = (d->h / d->bh) * p->nbw;
    p->nfit = (int64_t)d->n * p->nblk;
    if (p->nfit > 0x7fffffffLL || d->n > 65535 || (p->h2 + kHalfTH - 1) / kHalfTH > 65535)
        return fail(RESR_ERR_ARG, "niqe_features: grid overflow (n=%d, %d blocks per image, %d half-size rows)", d->n, p->nblk, p->h2), false;
    p->half_bytes = align_up((size_t)d->n * p->h2 * p->w2 * 8, 256);
    p->bytes = p->half_bytes + (size_t)2 * p->nfit * kBlockWords * 8;
    return true;
}
}  // namespace

size_t niqe_workspace_bytes(const ResrNiqeDesc* d) {
    NiqePlan p;
    return niqe_plan(d, &p) ? p.bytes : 0;
}

int niqe_features_dispatch(const ResrNiqeDesc* d, const uint8_t* luma, double* feats, hipStream_t st) {
    NiqePlan p;
    if (!niqe_plan(d, &p)) return RESR_ERR_ARG;
    if (!luma || !feats || !d->start_h || !d->w_h || !d->start_w || !d->w_w || !d->grid || !d->r_gam || !d->workspace)
        return fail(RESR_ERR_ARG, "niqe_features: null pointer");
    if (d->taps_h < 1 || d->taps_w < 1 || d->taps_h > kHalfTapsMax || d->taps_w > kHalfTapsMax || d->taps_h > d->h || d->taps_w > d->w || d->n_grid < 1)
        return fail(RESR_ERR_ARG, "niqe_features: bad tables (taps %d x %d: 1 .. %d and no more than the axis; grid of %d entries)", d->taps_h, d->taps_w, kHalfTapsMax, d->n_grid);
    if (((uintptr_t)d->workspace & 7) || ((uintptr_t)feats & 7)) return fail(RESR_ERR_ARG, "niqe_features: workspace and feats must be 8-byte aligned");
    if (d->workspace_bytes < p.bytes) return fail(RESR_ERR_WORKSPACE, "niqe_features: workspace of %zu bytes, %zu needed", d->workspace_bytes, p.bytes);
    double* half = (double*)d->workspace;
    double* mom1 = (double*)((char*)d->workspace + p.half_bytes);
    double* mom2 = mom1 + (size_t)p.nfit * kBlockWords;
    NiqeWindow win;
    memcpy(win.w, d->win, sizeof(win.w));
    static bool attr_set[kMaxDevices] = {false};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev >= 0 && dev < kMaxDevices && !attr_set[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&niqe_mscn_kernel<uint8_t>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&niqe_mscn_kernel<double>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax);
        attr_set[dev] = true;
    }
    const double px = (double)d->n * d->h * d->w;
    prof_before(st);
    hipLaunchKernelGGL(niqe_half_kernel, dim3((unsigned)((p.w2 + kHalfTW - 1) / kHalfTW), (unsigned)((p.h2 + kHalfTH - 1) / kHalfTH), (unsigned)d->n), dim3(256), 0, st,
                       luma, half, d->h, d->w, p.h2, p.w2, d->start_h, d->w_h, d->taps_h, d->start_w, d->w_w, d->taps_w);
    prof_after(st, 34100, px * 0.25 * 2.0 * (d->taps_h * 2.2 + d->taps_w), px * 3.0);
    RESR_CHECK_LAUNCH("niqe_half_kernel");
    prof_before(st);
    hipLaunchKernelGGL(niqe_mscn_kernel<uint8_t>, dim3((unsigned)p.nfit), dim3(kMscnThreads), p.lds1, st, luma, mom1, d->h, d->w, d->bh, d->bw, p.nbw, p.nblk, win);
    prof_after(st, 34200, px * 196.0, px);
    RESR_CHECK_LAUNCH("niqe_mscn_kernel<u8>");
    prof_before(st);
    hipLaunchKernelGGL(niqe_mscn_kernel<double>, dim3((unsigned)p.nfit), dim3(kMscnThreads), p.lds2, st, (const double*)half, mom2, p.h2, p.w2, d->bh / 2, d->bw / 2, p.nbw,
                       p.nblk, win);
    prof_after(st, 34201, px * 49.0, px * 2.0);
    RESR_CHECK_LAUNCH("niqe_mscn_kernel<f64>");
    prof_before(st);
    hipLaunchKernelGGL(niqe_aggd_kernel, dim3((unsigned)p.nfit, kMaps, 2), dim3(64), 0, st, (const double*)mom1, feats, d->grid, d->r_gam, d->n_grid, (int)p.nfit,
                       (double)d->bh * d->bw, (double)(d->bh / 2) * (d->bw / 2));
    prof_after(st, 34300, 0.0, (double)p.nfit * 10.0 * (kMoments * 8.0 + d->n_grid * 8.0));
    RESR_CHECK_LAUNCH("niqe_aggd_kernel");
    return RESR_OK;
}

// ---- the tail: features -> score ---------------------------------------------------------------------------------------------------
// One workgroup per image in both kernels (16 waves for the sums, 4 for the sweeps); the orders of every sum, the sweep's ordering and
// the rotation are stated in include/resr.h (resr_niqe_score) and are the definition.  Matrices in LDS have the leading dimension 37:
// a column walk of float64 words then moves 74 dwords a row, which meets each of the 64 banks of a ds_read_b64 once per 32-lane half
// (72 would meet 8 of them).
constexpr int kF = 36, kLd = 37, kEigThreads = 256, kStatThreads = 1024, kStatWaves = kStatThreads / 64, kRowGroups = 5;
constexpr int kWaveRows = 7, kChunk = kWaveRows * kStatWaves;   // rows a wave has in flight; rows of the centred tile in LDS: 112
constexpr int kStrips = 180;       // strips (i, 4k .. 4k + 3) that reach the upper triangle: 4 (k + 1) rows for k = 0 .. 8
constexpr int kTri = kF * (kF + 1) / 2, kPairs = kF / 2, kSteps = kF - 1, kSweepCap = 30;

// A wave takes whole rows: lane c < 36 holds column c, so "the row has no NaN" is one vote of the wave and every load is one
// contiguous 288-byte row.
__global__ __launch_bounds__(kStatThreads) void niqe_stats_kernel(const double* __restrict__ feats, const double* __restrict__ cov_prior, double* __restrict__ mu_out,
                                                                   double* __restrict__ a_out, int blocks) {
    __shared__ double tile[kChunk * kF];          // (no column walks here: the plain leading dimension)
    __shared__ double partials[kRowGroups * kStrips * 4];
    double (*part)[kStatWaves][kF] = reinterpret_cast<double (*)[kStatWaves][kF]>(partials);        // pass 1, [4]: per wave the sum of the non-NaN entries, their count, the sum over ok rows, the ok rows
    double (*strip_part)[kStrips * 4] = reinterpret_cast<double (*)[kStrips * 4]>(partials);        // pass 2, [5]: per row group the sums of every strip
    static_assert(4 * kStatWaves * kF <= kRowGroups * kStrips * 4, "the pass-1 partials live in the pass-2 array");
    __shared__ double mean_ok[kF];
    __shared__ double m_ok;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool col = lane < kF;
    const double* x = feats + (size_t)blockIdx.x * (size_t)blocks * kF;
    // pass 1: the column sums; wave w takes rows w, w + 16, ..., seven loads in flight
    double s_all = 0.0, n_all = 0.0, s_ok = 0.0, n_ok = 0.0;
    for (int r = wave; r < blocks; r += kChunk) {
        double v[kWaveRows];
#pragma unroll
        for (int k = 0; k < kWaveRows; ++k) v[k] = (col && r + k * kStatWaves < blocks) ? x[(r + k * kStatWaves) * kF + lane] : 0.0;
#pragma unroll
        for (int k = 0; k < kWaveRows; ++k) {
            if (r + k * kStatWaves >= blocks) break;
            const bool nan = v[k] != v[k], good = !__any(nan);
            s_all = __dadd_rn(s_all, nan ? 0.0 : v[k]);
            n_all += nan ? 0.0 : 1.0;
            s_ok = __dadd_rn(s_ok, good ? v[k] : 0.0);
            n_ok += good ? 1.0 : 0.0;
        }
    }
    if (col) {
        part[0][wave][lane] = s_all;
        part[1][wave][lane] = n_all;
        part[2][wave][lane] = s_ok;
        part[3][wave][lane] = n_ok;
    }
    __syncthreads();
    if (tid < kF) {
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        for (int w = 0; w < kStatWaves; ++w)
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] = __dadd_rn(t[k], part[k][w][tid]);
        mu_out[(size_t)blockIdx.x * kF + tid] = t[0] / t[1];
        mean_ok[tid] = t[2] / t[3];
        if (tid == 0) m_ok = t[3];
    }
    __syncthreads();
    // pass 2: the rows, centred (an exact zero for a row that is not ok), pass through LDS 112 at a time; thread (g, s), s < 180, g < 5,
    // adds rows g, g + 5, ... of every chunk to its sums of (i, j0 .. j0 + 3); strips are numbered strip group by strip group, i ascending
    const int strip = tid % kStrips, grp = tid / kStrips;
    int jg = 0;
    while (jg < 8 && strip >= 2 * (jg + 1) * (jg + 2)) ++jg;
    const int si = strip - 2 * jg * (jg + 1), j0 = 4 * jg;
    const bool owner = grp < kRowGroups;
    const double mean = col ? mean_ok[lane] : 0.0;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    double next[kWaveRows];
#pragma unroll
    for (int k = 0; k < kWaveRows; ++k) next[k] = (col && wave + k * kStatWaves < blocks) ? x[(wave + k * kStatWaves) * kF + lane] : 0.0;
    for (int r0 = 0; r0 < blocks; r0 += kChunk) {
        const int rows = min(kChunk, blocks - r0);
#pragma unroll
        for (int k = 0; k < kWaveRows; ++k) {    // wave w stages rows w, w + 16, ..., w + 96 of the chunk
            const int r = wave + k * kStatWaves;
            if (r >= rows) break;
            const bool good = !__any(next[k] != next[k]);
            if (col) tile[r * kF + lane] = good ? __dsub_rn(next[k], mean) : 0.0;
        }
#pragma unroll
        for (int k = 0; k < kWaveRows; ++k) {    // the next chunk's rows travel while this one is summed
            const int r = r0 + kChunk + wave + k * kStatWaves;
            next[k] = (col && r < blocks) ? x[r * kF + lane] : 0.0;
        }
        __syncthreads();
        if (owner)
            for (int r = grp; r < rows; r += kRowGroups) {
                const double ci = tile[r * kF + si];
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = fma(ci, tile[r * kF + j0 + k], acc[k]);
            }
        __syncthreads();
    }
    if (owner)
#pragma unroll
        for (int k = 0; k < 4; ++k) strip_part[grp][strip * 4 + k] = acc[k];
    __syncthreads();
    if (tid < kStrips) {
        const double den = m_ok - 1.0;
        double* a = a_out + (size_t)blockIdx.x * kF * kF;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = j0 + k;
            if (j < si) continue;
            double sum = 0.0;
            for (int g = 0; g < kRowGroups; ++g) sum = __dadd_rn(sum, strip_part[g][strip * 4 + k]);
            const double v = __dadd_rn(cov_prior[si * kF + j], sum / den) / 2.0;
            a[si * kF + j] = v;
            a[j * kF + si] = v;
        }
    }
}

// the partner of index i in step `step` of a sweep: 35 meets `step`, every other pair (a, b) has a + b = 2 step (mod 35)
__device__ __forceinline__ int rr_partner(int i, int step) {
    if (i == kSteps) return step;
    if (i == step) return kSteps;
    int v = 2 * step - i;
    v += v < 0 ? kSteps : 0;
    v -= v >= kSteps ? kSteps : 0;
    return v;
}

__global__ __launch_bounds__(kEigThreads) void niqe_eig_kernel(const double* __restrict__ mu_prior, const double* __restrict__ mu_d, const double* __restrict__ a_in,
                                                                double* __restrict__ eig_out, double* __restrict__ kept_out, double* __restrict__ scores) {
    __shared__ double mat[2][kF * kLd];
    __shared__ double vec[kF * kLd];
    __shared__ double rot_c[kPairs], rot_s[kPairs], rot_t[kPairs];   // the step's rotations, pair by pair
    __shared__ int rot_p[kPairs], rot_q[kPairs];
    __shared__ double diff[kF], term[kF];
    __shared__ int keeps[kF];
    __shared__ int step_rotates[2];
    const int tid = (int)threadIdx.x, img = (int)blockIdx.x;
    const double* a = a_in + (size_t)img * kF * kF;
    int bad = 0;
    for (int e = tid; e < kF * kF; e += kEigThreads) {
        const int i = e / kF, j = e - i * kF;
        const double v = a[e];
        bad |= !(fabs(v) <= 1.7976931348623157e308);
        mat[0][i * kLd + j] = v;
        vec[i * kLd + j] = i == j ? 1.0 : 0.0;
    }
    if (tid < kF) diff[tid] = __dsub_rn(mu_prior[tid], mu_d[(size_t)img * kF + tid]);
    // what a thread owns for the whole loop: thread b < 171 the 2 x 2 block of J^T A J that pairs k1 <= k2 of a step meet in (b counts
    // the blocks row by row of the pair triangle); thread t < 252 rows t / 18, t / 18 + 14 and (below row 8) t / 18 + 28 of the two
    // eigenvector columns of pair t % 18
    int k1 = 0, k2 = tid;
    while (k1 < kPairs - 1 && k2 >= kPairs - k1) { k2 -= kPairs - k1; ++k1; }
    k2 = min(k1 + k2, kPairs - 1);                // (threads past the last block keep indices inside the arrays)
    const bool block_owner = tid < kPairs * (kPairs + 1) / 2, v_owner = tid < 14 * kPairs;
    const int vk = tid % kPairs, vr = min(tid / kPairs, 13);
    const bool third_v = vr + 28 < kF;
    if (__syncthreads_or(bad)) {                  // 0 / 0 of a single ok row, or a non-finite feature: no eigenvalues, no score
        if (tid < kF) eig_out[(size_t)img * kF + tid] = NAN;
        if (tid == 0) {
            kept_out[img] = 0.0;
            scores[img] = NAN;
        }
        return;
    }
    double* m = mat[0];
    double* out = mat[1];
    bool converged = false;
    for (int sweep = 0; sweep < kSweepCap && !converged; ++sweep) {
        int rotated = 0;
        for (int step = 0; step < kSteps; ++step) {
            if (tid < 64) {                       // the 18 rotations of the step, by the first wave
                bool rotates = false;
                if (tid < kPairs) {
                    const int x = tid == 0 ? kSteps : (step + tid >= kSteps ? step + tid - kSteps : step + tid), y = rr_partner(x, step);
                    const int p = min(x, y), q = max(x, y);
                    const double apq = m[p * kLd + q], app = m[p * kLd + p], aqq = m[q * kLd + q];
                    double c = 1.0, s = 0.0, t = 0.0;
                    if (__dmul_rn(apq, apq) > 0x1p-106 * fabs(__dmul_rn(app, aqq))) {
                        const double d = __dsub_rn(aqq, app), h = __dmul_rn(2.0, apq);
                        t = h / __dadd_rn(d, copysign(sqrt(fma(d, d, __dmul_rn(h, h))), d));
                        c = rsqrt(fma(t, t, 1.0));
                        s = __dmul_rn(t, c);
                        if (s == 0.0) { c = 1.0; t = 0.0; }   // a rotation too small to change anything is none
                        else rotates = true;
                    }
                    rot_p[tid] = p; rot_q[tid] = q;
                    rot_c[tid] = c; rot_s[tid] = s; rot_t[tid] = t;
                }
                const int any = __any(rotates);
                if (tid == 0) step_rotates[step & 1] = any;
            }
            __syncthreads();
            if (!step_rotates[step & 1]) continue;    // (the same word for every thread: the step leaves both matrices as they are)
            rotated = 1;
            // every load of the step first and without a branch, so that they travel together; then the stores
            // the block of pairs k1 <= k2: rows p1, q1, columns p2, q2 of J^T A J, pair k1's rotation outermost
            const int p1 = rot_p[k1], q1 = rot_q[k1], p2 = rot_p[k2], q2 = rot_q[k2];
            const double c1 = rot_c[k1], s1 = rot_s[k1], t1 = rot_t[k1], c2 = rot_c[k2], s2 = rot_s[k2];
            const double a_pp = m[p1 * kLd + p2], a_pq = m[p1 * kLd + q2], a_qp = m[q1 * kLd + p2], a_qq = m[q1 * kLd + q2];
            // the two eigenvector columns of pair vk
            const int vp = rot_p[vk], vq = rot_q[vk];
            const double vc = rot_c[vk], vs = rot_s[vk];
            double x0[3], x1[3];
#pragma unroll
            for (int n = 0; n < 3; ++n) {
                const int r = min(vr + 14 * n, kF - 1);
                x0[n] = vec[r * kLd + vp];
                x1[n] = vec[r * kLd + vq];
            }
            const double u_pp = fma(-s2, a_pq, __dmul_rn(c2, a_pp)), u_qp = fma(-s2, a_qq, __dmul_rn(c2, a_qp));   // columns rotated: (A J)
            const double u_pq = fma(s2, a_pp, __dmul_rn(c2, a_pq)), u_qq = fma(s2, a_qp, __dmul_rn(c2, a_qq));
            double n_pp = fma(-s1, u_qp, __dmul_rn(c1, u_pp)), n_pq = fma(-s1, u_qq, __dmul_rn(c1, u_pq));         // then rows: J^T (A J)
            double n_qp = fma(s1, u_pp, __dmul_rn(c1, u_qp)), n_qq = fma(s1, u_pq, __dmul_rn(c1, u_qq));
            if (k1 == k2) {                           // the pair's own block: a_pq is the element the rotation annihilates
                n_pp = fma(-t1, a_pq, a_pp);
                n_qq = fma(t1, a_pq, a_qq);
                n_pq = n_qp = s1 != 0.0 ? 0.0 : a_pq;
            }
            if (block_owner) {
                out[p1 * kLd + p2] = n_pp; out[p2 * kLd + p1] = n_pp;
                out[p1 * kLd + q2] = n_pq; out[q2 * kLd + p1] = n_pq;
                out[q1 * kLd + p2] = n_qp; out[p2 * kLd + q1] = n_qp;
                out[q1 * kLd + q2] = n_qq; out[q2 * kLd + q1] = n_qq;
            }
            if (v_owner)
#pragma unroll
                for (int n = 0; n < 3; ++n) {
                    if (n == 2 && !third_v) break;
                    const int r = vr + 14 * n;
                    vec[r * kLd + vp] = fma(-vs, x1[n], __dmul_rn(vc, x0[n]));
                    vec[r * kLd + vq] = fma(vs, x0[n], __dmul_rn(vc, x1[n]));
                }
            __syncthreads();
            double* was = m;
            m = out;
            out = was;
        }
        converged = rotated == 0;
    }
    if (tid < kF) {
        const double l = m[tid * kLd + tid];
        eig_out[(size_t)img * kF + tid] = l;
        double big = 0.0;
        for (int k = 0; k < kF; ++k) big = fmax(big, fabs(m[k * kLd + k]));
        double y = 0.0;
        for (int r = 0; r < kF; ++r) y = fma(vec[r * kLd + tid], diff[r], y);
        const bool keep = fabs(l) > __dmul_rn((double)kF * 0x1p-52, big);
        term[tid] = keep ? __dmul_rn(y, y) / l : 0.0;
        keeps[tid] = keep;
    }
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        int kept = 0;
        for (int k = 0; k < kF; ++k)
            if (keeps[k]) {
                sum = __dadd_rn(sum, term[k]);
                ++kept;
            }
        kept_out[img] = (double)kept;
        scores[img] = converged ? sqrt(sum) : NAN;
    }
}

namespace {
constexpr size_t kScoreWords = kF + kF * kF + kF + 1;   // per image: mu_d, A, eigenvalues, kept count

bool niqe_score_plan(const ResrNiqeScoreDesc* d, size_t* bytes) {
    if (!d) return fail(RESR_ERR_ARG, "niqe_score: null descriptor"), false;
    if (d->n < 1 || d->blocks < 1) return fail(RESR_ERR_ARG, "niqe_score: bad descriptor (n=%d, blocks=%d: both at least 1)", d->n, d->blocks), false;
    if ((int64_t)d->blocks * kF > 0x7fffffffLL)
        return fail(RESR_ERR_ARG, "niqe_score: %d blocks of 36 features do not fit the int32 offsets inside an image", d->blocks), false;
    *bytes = (size_t)d->n * kScoreWords * 8;
    return true;
}
}  // namespace

size_t niqe_score_workspace_bytes(const ResrNiqeScoreDesc* d) {
    size_t bytes = 0;
    return niqe_score_plan(d, &bytes) ? bytes : 0;
}

int niqe_score_dispatch(const ResrNiqeScoreDesc* d, const double* feats, double* scores, hipStream_t st) {
    size_t bytes = 0;
    if (!niqe_score_plan(d, &bytes)) return RESR_ERR_ARG;
    if (!feats || !scores || !d->mu_prior || !d->cov_prior || !d->workspace) return fail(RESR_ERR_ARG, "niqe_score: null pointer");
    if (((uintptr_t)feats | (uintptr_t)scores | (uintptr_t)d->mu_prior | (uintptr_t)d->cov_prior | (uintptr_t)d->workspace) & 7)
        return fail(RESR_ERR_ARG, "niqe_score: feats, scores, the priors and the workspace must be 8-byte aligned");
    if (d->workspace_bytes < bytes) return fail(RESR_ERR_ARG, "niqe_score: workspace of %zu bytes, %zu needed", d->workspace_bytes, bytes);
    const size_t n = (size_t)d->n;
    double* mu_d = (double*)d->workspace;
    double* a = mu_d + n * kF;
    double* eig = a + n * kF * kF;
    double* kept = eig + n * kF;
    prof_before(st);
    hipLaunchKernelGGL(niqe_stats_kernel, dim3((unsigned)d->n), dim3(kStatThreads), 0, st, feats, d->cov_prior, mu_d, a, d->blocks);
    prof_after(st, 34400, (double)n * d->blocks * (2.0 * kF * 4 + 2.0 * kStrips * 4), (double)n * d->blocks * kF * 8.0 * 2.0);
    RESR_CHECK_LAUNCH("niqe_stats_kernel");
    prof_before(st);
    hipLaunchKernelGGL(niqe_eig_kernel, dim3((unsigned)d->n), dim3(kEigThreads), 0, st, d->mu_prior, (const double*)mu_d, (const double*)a, eig, kept, scores);
    prof_after(st, 34500, 0.0, (double)n * kScoreWords * 8.0);
    RESR_CHECK_LAUNCH("niqe_eig_kernel");
    return RESR_OK;
}

}  // namespace resr
