// resample_u8.hip -- the multi-scale copies of the whole-image training source (device_data.ImageCropSource, scales / short_side): Pillow's
// 8-bit LANCZOS resize restated as an integer rule (device_data.resample_tables_np / resample_u8_np), its tables built on the host and its
// two passes run on the device in one launch.
//   resample_tables : (in, out) -> per output index (xmin, count) and `ksize` Q22 coefficients.  Plain host C++ in double with libm's sin,
//                     no contraction: the operations of the definition in its order.
//   resample_u8     : a table of jobs, each one HWC RGB uint8 image of an arena resampled into another place of the same arena: the
//                     horizontal pass (int32 multiply-adds, + 2^21, >> 22, clipped to a byte), then the vertical pass over those bytes.
//                     Bit for bit device_data.resample_u8_np.
#include <math.h>

#include <algorithm>
#include <vector>

#include "host_api.h"

namespace resr {

constexpr int kResampleBits = 22;                 // Q22 coefficients: 32 - 8 - 2
constexpr int kResampleMaxTaps = 4096;
constexpr double kResampleSupport = 3.0;          // Lanczos-3

// the taps of one table row: ceil(support * max(in / out, 1)) * 2 + 1, evaluated in double on the host and on the device alike (one IEEE
// division, one exact-rounded product, a ceil: nothing to contract)
__host__ __device__ inline int64_t resample_taps(int64_t in_size, int64_t out_size) {
    double fs = (double)in_size / (double)out_size;
    if (fs < 1.0) fs = 1.0;
    return (int64_t)ceil(kResampleSupport * fs) * 2 + 1;
}

// ---- the host table builder --------------------------------------------------------------------------------------------------------
static double sinc_pi(double x) {
#pragma clang fp contract(off)
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}

static double lanczos3(double x) {
#pragma clang fp contract(off)
    if (-3.0 <= x && x < 3.0) return sinc_pi(x) * sinc_pi(x / 3);
    return 0.0;
}

int resample_ksize(int64_t in_size, int64_t out_size) {
    if (in_size < 1 || out_size < 1 || in_size > 0x7fffffffLL || out_size > 0x7fffffffLL)
        return fail(RESR_ERR_ARG, "resample_ksize: in_size=%lld or out_size=%lld outside 1..2^31 - 1", (long long)in_size, (long long)out_size);
    const int64_t taps = resample_taps(in_size, out_size);
    return taps > 0x7fffffffLL ? 0x7fffffff : (int)taps;
}

int resample_tables(int64_t in_size, int64_t out_size, int32_t* bounds, int32_t* coeffs, int ksize_capacity) {
#pragma clang fp contract(off)
    if (!bounds || !coeffs) return fail(RESR_ERR_ARG, "resample_tables: a null pointer (bounds and coeffs are both needed)");
    const int ksize = resample_ksize(in_size, out_size);
    if (ksize < 0) return ksize;
    if (ksize_capacity < ksize)
        return fail(RESR_ERR_ARG, "resample_tables: ksize_capacity=%d below the %d taps of %lld -> %lld", ksize_capacity, ksize, (long long)in_size, (long long)out_size);
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = kResampleSupport * fs;
    const double ss = 1.0 / fs;
    std::vector<double> w((size_t)ksize);
    for (int64_t xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        int64_t xmin = (int64_t)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int64_t xmax = (int64_t)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        const int count = (int)(xmax - xmin);
        double ww = 0.0;
        for (int x = 0; x < count; ++x) {
            w[x] = lanczos3((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        int32_t* row = coeffs + (size_t)xx * (size_t)ksize_capacity;
        int64_t reach = 0;                                   // sum |coeff| of the row
        for (int x = 0; x < count; ++x) {
            if (ww != 0.0) w[x] /= ww;
            const double q = w[x] * (double)(1 << kResampleBits);
            row[x] = w[x] < 0 ? (int32_t)(-0.5 + q) : (int32_t)(0.5 + q);
            reach += row[x] < 0 ? -(int64_t)row[x] : (int64_t)row[x];
        }
        for (int x = count; x < ksize_capacity; ++x) row[x] = 0;
        if (255 * reach + (1LL << (kResampleBits - 1)) >= (1LL << 31))
            return fail(RESR_ERR_ARG, "resample_tables: row %lld of %lld -> %lld: 255 * sum|coeff| + 2^21 = %lld would overflow the int32 accumulator", (long long)xx,
                        (long long)in_size, (long long)out_size, (long long)(255 * reach + (1LL << (kResampleBits - 1))));
        bounds[2 * xx] = (int32_t)xmin;
        bounds[2 * xx + 1] = count;
    }
    return RESR_OK;
}

// ---- resample_u8 -------------------------------------------------------------------------------------------------------------------
// ONE fused launch; the only extra device memory is the launch's job and table buffers.  grid.y is the job, grid.x a kRsTW x kRsTH tile of its
// output (a workgroup past its job's tiles leaves at once).  The tile's output rows need the horizontally resampled rows r_lo .. r_hi - 1 of
// its 64 columns; they are made kRsRows at a time and never leave the CU:
//   stage   the source bytes of those rows, kRsSrcPx pixels a chunk, into LDS: consecutive lanes on consecutive bytes of a row;
//   H pass  thread (column, row group) holds 4 rows x 3 channels of int32 sums: one coefficient read serves 12 multiply-adds; the sums live
//           across the source chunks, so a row of any length (4096 taps) runs in the same LDS; four taps at a time come as four aligned LDS
//           dwords a row, the rest byte by byte; + 2^21, >> 22, clip -> bytes in LDS (`mid`);
//   V pass  a thread owns aligned dwords of output rows (4 bytes x 4 units of int32 sums, kept across the row chunks): per staged row one
//           coefficient and two LDS dwords, byte-aligned in a register.
// At the end a unit wholly inside its row is ONE dword store (the unit grid is shifted per row so that its addresses are 4-byte aligned
// wherever the row starts); the ragged ends of a row are byte stores.  Coefficient rows reach LDS once per workgroup: the tile's column rows
// when they have at most kRsTapCap taps (longer rows are read from the table, still once per column and 12 sums), the rows' coefficients of
// each row chunk.  An axis whose size does not change runs as the identity row (xmin = index, count = 1, coefficient 2^22), which returns the
// byte: (2^21 + b * 2^22) >> 22 = b, the skipped pass of the definition.
// Nothing of a table is trusted for addressing: xmin is clamped into 0 .. in - 1 and count into 0 .. min(ksize, in - xmin) where they are
// read.  The sums are formed in uint32 (two's complement, as numpy's int32).  Every offset is 64-bit.
constexpr int kRsThreads = 256;
constexpr int kRsTW = 64, kRsTH = 16;             // the output tile: pixels x rows
constexpr int kRsRows = 16;                       // intermediate rows a chunk
constexpr int kRsSrcPx = 256;                     // source pixels a staged chunk
constexpr int kRsSrcPitch = kRsSrcPx * 3 + 4;     // bytes per staged source row: 193 dwords, odd
constexpr int kRsMidWords = 52;                   // dwords per intermediate row: 4 bytes in front, 192 of the row, room for the last unit's pair
constexpr int kRsTapCap = 40;                     // staged taps per column (2040 -> 400 has 33)
constexpr int kRsUnits = kRsTW * 3 / 4 + 1;       // aligned dword units per output row
constexpr int kRsUnitsPerThread = (kRsTH * kRsUnits + kRsThreads - 1) / kRsThreads;
static_assert(kRsTH * kRsRows == kRsThreads && kRsThreads == 4 * kRsTW && kRsRows == 16, "the thread maps of resample_u8_kernel");
constexpr uint32_t kRsOne = 1u << kResampleBits, kRsHalf = 1u << (kResampleBits - 1);

__device__ __forceinline__ uint32_t resample_clip(uint32_t acc) {
    const int32_t v = (int32_t)(acc + kRsHalf) >> kResampleBits;
    return (uint32_t)min(max(v, 0), 255);
}

__global__ __launch_bounds__(kRsThreads) void resample_u8_kernel(uint8_t* arena, const int64_t* __restrict__ jobs, const int32_t* __restrict__ tables) {
    __shared__ __attribute__((aligned(16))) uint8_t src_lds[kRsRows * kRsSrcPitch];
    __shared__ uint32_t mid[kRsRows * kRsMidWords];
    __shared__ int32_t hc[kRsTW * kRsTapCap];
    __shared__ int32_t vc[kRsTH * kRsRows];
    __shared__ int32_t col_min[kRsTW], col_cnt[kRsTW], row_min[kRsTH], row_cnt[kRsTH];
    const int64_t* job = jobs + (size_t)blockIdx.y * 8;
    const int64_t h = job[1], w = job[2], oh = job[4], ow = job[5];
    const int64_t tiles_x = (ow + kRsTW - 1) / kRsTW, tiles_y = (oh + kRsTH - 1) / kRsTH;
    if ((int64_t)blockIdx.x >= tiles_x * tiles_y) return;
    const uint8_t* src = arena + job[0];
    const int64_t x0 = ((int64_t)blockIdx.x % tiles_x) * kRsTW, y0 = ((int64_t)blockIdx.x / tiles_x) * kRsTH;
    const int tw = (int)min((int64_t)kRsTW, ow - x0), th = (int)min((int64_t)kRsTH, oh - y0);
    const bool hpass = ow != w, vpass = oh != h;
    const int kx = hpass ? (int)min(resample_taps(w, ow), (int64_t)kResampleMaxTaps) : 1;
    const int ky = vpass ? (int)min(resample_taps(h, oh), (int64_t)kResampleMaxTaps) : 1;
    const int32_t* col_bounds = tables + job[7];
    const int32_t* col_coeffs = col_bounds + 2 * ow;
    const int32_t* row_bounds = tables + job[6];
    const int32_t* row_coeffs = row_bounds + 2 * oh;
    const int tid = (int)threadIdx.x;
    const bool staged_taps = hpass && kx <= kRsTapCap;

    // the tile's bounds, clamped into the source, and its column coefficients
    if (tid < kRsTW) {
        int64_t lo = x0 + tid, cnt = tid < tw ? 1 : 0;
        if (hpass && tid < tw) {
            lo = min(max((int64_t)col_bounds[2 * (x0 + tid)], (int64_t)0), w - 1);
            cnt = min(max((int64_t)col_bounds[2 * (x0 + tid) + 1], (int64_t)0), min((int64_t)kx, w - lo));
        }
        col_min[tid] = (int)lo;
        col_cnt[tid] = (int)cnt;
    } else if (tid < kRsTW + kRsTH) {
        const int yy = tid - kRsTW;
        int64_t lo = y0 + yy, cnt = yy < th ? 1 : 0;
        if (vpass && yy < th) {
            lo = min(max((int64_t)row_bounds[2 * (y0 + yy)], (int64_t)0), h - 1);
            cnt = min(max((int64_t)row_bounds[2 * (y0 + yy) + 1], (int64_t)0), min((int64_t)ky, h - lo));
        }
        row_min[yy] = (int)lo;
        row_cnt[yy] = (int)cnt;
    }
    if (staged_taps)
        for (int i = tid; i < tw * kx; i += kRsThreads) {
            const int xx = i / kx, k = i - xx * kx;
            hc[xx * kRsTapCap + k] = col_coeffs[(x0 + xx) * kx + k];
        }
    __syncthreads();
    int64_t s_lo = 0x7fffffff, s_hi = 0, r_lo = 0x7fffffff, r_hi = 0;  // the source columns and rows the tile reads (empty rows leave them out)
    for (int xx = 0; xx < tw; ++xx)
        if (col_cnt[xx] > 0) {
            s_lo = min(s_lo, (int64_t)col_min[xx]);
            s_hi = max(s_hi, (int64_t)col_min[xx] + col_cnt[xx]);
        }
    for (int yy = 0; yy < th; ++yy)
        if (row_cnt[yy] > 0) {
            r_lo = min(r_lo, (int64_t)row_min[yy]);
            r_hi = max(r_hi, (int64_t)row_min[yy] + row_cnt[yy]);
        }

    // H pass: this thread's column and its 4 rows of a chunk
    const int hx = tid & (kRsTW - 1), hrow = (tid >> 6) * 4;
    const int my_min = col_min[hx], my_cnt = hx < tw ? col_cnt[hx] : 0;
    const int32_t* my_coeffs = col_coeffs + (x0 + hx) * kx;
    // V pass: this thread's units
    uint8_t* const dst = arena + job[3];
    uint32_t vacc[kRsUnitsPerThread][4];
    int u_row[kRsUnitsPerThread], u_first[kRsUnitsPerThread];           // the unit's output row in the tile (-1: none); its first byte in the tile row
#pragma unroll
    for (int u = 0; u < kRsUnitsPerThread; ++u) {
        const int unit = tid + u * kRsThreads, yy = unit / kRsUnits, d = unit - yy * kRsUnits;
        u_row[u] = yy < th ? yy : -1;
        const int a = (int)((uintptr_t)(dst + ((y0 + yy) * ow + x0) * 3) & 3u);
        u_first[u] = 4 * d - a;
        if (u_first[u] >= tw * 3) u_row[u] = -1;
        vacc[u][0] = vacc[u][1] = vacc[u][2] = vacc[u][3] = 0u;
    }

    for (int64_t rc0 = r_lo; rc0 < r_hi; rc0 += kRsRows) {
        const int nrows = (int)min((int64_t)kRsRows, r_hi - rc0);
        uint32_t hacc[4][3];
#pragma unroll
        for (int r = 0; r < 4; ++r) hacc[r][0] = hacc[r][1] = hacc[r][2] = 0u;
        for (int64_t cs0 = s_lo; cs0 < s_hi; cs0 += kRsSrcPx) {
            const int nbytes = (int)min((int64_t)kRsSrcPx, s_hi - cs0) * 3;
            __syncthreads();                                            // the last readers of src_lds are through
            for (int r = 0; r < nrows; ++r) {
                const uint8_t* line = src + ((rc0 + r) * w + cs0) * 3;
                for (int b = tid; b < nbytes; b += kRsThreads) src_lds[r * kRsSrcPitch + b] = line[b];
            }
            __syncthreads();
            const int first = (int)(my_min - cs0);                      // this column's tap 0 in the chunk (may lie in front of it)
            const int k_lo = max(0, -first), k_hi = min(my_cnt, nbytes / 3 - first);
            int k = k_lo;
            for (; k + 4 <= k_hi; k += 4) {                             // four taps = 12 consecutive bytes a row: four aligned LDS dwords, shifted in registers
                uint32_t c[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) c[i] = (uint32_t)(staged_taps ? hc[hx * kRsTapCap + k + i] : my_coeffs[k + i]);      // (count >= 4: a real pass)
                const int at = (first + k) * 3;
                const uint32_t shift = (uint32_t)at & 3u;
                const uint32_t* q = reinterpret_cast<const uint32_t*>(src_lds + hrow * kRsSrcPitch + (at & ~3));
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint32_t* qr = q + r * (kRsSrcPitch / 4);
                    const uint32_t w0 = qr[0], w1 = qr[1], w2 = qr[2], w3 = qr[3];
                    const uint32_t d0 = __builtin_amdgcn_alignbyte(w1, w0, shift), d1 = __builtin_amdgcn_alignbyte(w2, w1, shift),
                                   d2 = __builtin_amdgcn_alignbyte(w3, w2, shift);
                    hacc[r][0] += (d0 & 255u) * c[0] + (d0 >> 24) * c[1] + ((d1 >> 16) & 255u) * c[2] + ((d2 >> 8) & 255u) * c[3];
                    hacc[r][1] += ((d0 >> 8) & 255u) * c[0] + (d1 & 255u) * c[1] + (d1 >> 24) * c[2] + ((d2 >> 16) & 255u) * c[3];
                    hacc[r][2] += ((d0 >> 16) & 255u) * c[0] + ((d1 >> 8) & 255u) * c[1] + (d2 & 255u) * c[2] + (d2 >> 24) * c[3];
                }
            }
            for (; k < k_hi; ++k) {
                const uint32_t c = !hpass ? kRsOne : (uint32_t)(staged_taps ? hc[hx * kRsTapCap + k] : my_coeffs[k]);
                const uint8_t* p = src_lds + hrow * kRsSrcPitch + (first + k) * 3;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    hacc[r][0] += (uint32_t)p[r * kRsSrcPitch] * c;
                    hacc[r][1] += (uint32_t)p[r * kRsSrcPitch + 1] * c;
                    hacc[r][2] += (uint32_t)p[r * kRsSrcPitch + 2] * c;
                }
            }
        }
        __syncthreads();                                                // the V pass of the chunk before is through with mid and vc
        if (hx < tw) {
            uint8_t* m = reinterpret_cast<uint8_t*>(mid) + 4 + hx * 3;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                uint8_t* o = m + (hrow + r) * (kRsMidWords * 4);
                o[0] = (uint8_t)resample_clip(hacc[r][0]);
                o[1] = (uint8_t)resample_clip(hacc[r][1]);
                o[2] = (uint8_t)resample_clip(hacc[r][2]);
            }
        }
        {
            const int yy = tid / kRsRows, rr = tid - yy * kRsRows;       // kRsTH * kRsRows == kRsThreads
            const int64_t k = rc0 + rr - row_min[yy];
            int32_t c = 0;
            if (yy < th && rr < nrows && k >= 0 && k < row_cnt[yy]) c = vpass ? row_coeffs[(y0 + yy) * ky + k] : (int32_t)kRsOne;
            vc[tid] = c;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kRsUnitsPerThread; ++u) {
            const int yy = u_row[u];
            if (yy < 0) continue;
            const int at = 4 + u_first[u];                              // >= 1: the unit's first byte in a mid row
            const int word = at >> 2, shift = at & 3;
            const int rr_lo = (int)max((int64_t)0, row_min[yy] - rc0), rr_hi = (int)min((int64_t)nrows, row_min[yy] + row_cnt[yy] - rc0);
            for (int rr = rr_lo; rr < rr_hi; ++rr) {
                const uint32_t c = (uint32_t)vc[yy * kRsRows + rr];
                const uint32_t lo = mid[rr * kRsMidWords + word], hi = mid[rr * kRsMidWords + word + 1];
                const uint32_t v = __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)shift);
                vacc[u][0] += (v & 255u) * c;
                vacc[u][1] += ((v >> 8) & 255u) * c;
                vacc[u][2] += ((v >> 16) & 255u) * c;
                vacc[u][3] += (v >> 24) * c;
            }
        }
    }
    const int row_bytes = tw * 3;
#pragma unroll
    for (int u = 0; u < kRsUnitsPerThread; ++u) {
        const int yy = u_row[u];
        if (yy < 0) continue;
        uint8_t* o = dst + ((y0 + yy) * ow + x0) * 3 + u_first[u];
        const uint32_t b0 = resample_clip(vacc[u][0]), b1 = resample_clip(vacc[u][1]), b2 = resample_clip(vacc[u][2]), b3 = resample_clip(vacc[u][3]);
        if (u_first[u] >= 0 && u_first[u] + 4 <= row_bytes) {
            *reinterpret_cast<uint32_t*>(o) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
        } else {
            const uint32_t b[4] = {b0, b1, b2, b3};
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (u_first[u] + i >= 0 && u_first[u] + i < row_bytes) o[i] = (uint8_t)b[i];
        }
    }
}

int resample_u8_dispatch(uint8_t* arena, int64_t arena_bytes, const int64_t* jobs_host, const int64_t* jobs_dev, int J, const int32_t* tables, int64_t table_words,
                         hipStream_t st) {
    if (!arena || !jobs_host || !jobs_dev || !tables) return fail(RESR_ERR_ARG, "resample_u8: a null pointer (arena, jobs_host, jobs_dev and tables are all needed)");
    if (J < 1 || J > 65535) return fail(RESR_ERR_ARG, "resample_u8: j=%d outside 1..65535 (the grid's y dimension)", J);
    if (arena_bytes < 1 || table_words < 0) return fail(RESR_ERR_ARG, "resample_u8: arena_bytes=%lld below 1 or table_words=%lld below 0", (long long)arena_bytes, (long long)table_words);
    struct Range { int64_t lo, hi; int dst, job; };
    std::vector<Range> ranges;
    ranges.reserve(2 * (size_t)J);
    int64_t tiles = 1;
    double bytes = 0.0;
    for (int j = 0; j < J; ++j) {
        const int64_t* q = jobs_host + (size_t)j * 8;
        const int64_t side[4] = {q[1], q[2], q[4], q[5]};
        for (int s = 0; s < 4; ++s)
            if (side[s] < 1 || side[s] > 0x7fffffffLL)
                return fail(RESR_ERR_ARG, "resample_u8: job %d: a side of %lldx%lld -> %lldx%lld (w x h) is below 1 or at or above 2^31", j, (long long)q[2], (long long)q[1],
                            (long long)q[5], (long long)q[4]);
        for (int axis = 0; axis < 2; ++axis) {                          // 0: rows (h -> oh, table q[6]); 1: columns (w -> ow, table q[7])
            const int64_t in = q[1 + axis], out = q[4 + axis], at = q[6 + axis];
            if (in == out) continue;
            const int64_t ksize = resample_taps(in, out);
            if (ksize < 1 || ksize > kResampleMaxTaps)
                return fail(RESR_ERR_ARG, "resample_u8: job %d: ksize=%lld of %lld -> %lld outside 1..%d", j, (long long)ksize, (long long)in, (long long)out, kResampleMaxTaps);
            if (at < 0 || at > table_words || out * (2 + ksize) > table_words - at)
                return fail(RESR_ERR_ARG, "resample_u8: job %d: its %s table at word %lld (%lld words) leaves the table buffer of %lld words", j, axis ? "column" : "row",
                            (long long)at, (long long)(out * (2 + ksize)), (long long)table_words);
        }
        const unsigned __int128 src_bytes = (unsigned __int128)q[1] * q[2] * 3, dst_bytes = (unsigned __int128)q[4] * q[5] * 3;
        if (q[0] < 0 || q[3] < 0 || q[0] > arena_bytes || q[3] > arena_bytes || src_bytes > (unsigned __int128)(arena_bytes - q[0]) || dst_bytes > (unsigned __int128)(arena_bytes - q[3]))
            return fail(RESR_ERR_ARG, "resample_u8: job %d: its source or destination leaves the arena of %lld bytes", j, (long long)arena_bytes);
        ranges.push_back({q[0], q[0] + (int64_t)src_bytes, 0, j});
        ranges.push_back({q[3], q[3] + (int64_t)dst_bytes, 1, j});
        tiles = std::max(tiles, ((q[5] + kRsTW - 1) / kRsTW) * ((q[4] + kRsTH - 1) / kRsTH));
        bytes += (double)src_bytes + (double)dst_bytes;
    }
    if (tiles > 0x7fffffffLL) return fail(RESR_ERR_ARG, "resample_u8: grid overflow (%lld tiles in one job)", (long long)tiles);
    // a destination shares no byte with any source or other destination of the launch (sources may share: they are only read)
    std::sort(ranges.begin(), ranges.end(), [](const Range& a, const Range& b) { return a.lo < b.lo; });
    int64_t end_any = -1, end_dst = -1;
    int job_any = 0, job_dst = 0;
    for (const Range& r : ranges) {
        if (r.dst ? r.lo < end_any : r.lo < end_dst)
            return fail(RESR_ERR_ARG, "resample_u8: overlapping source and destination: the %s of job %d and a range of job %d share bytes", r.dst ? "destination" : "source", r.job,
                        r.dst ? job_any : job_dst);
        if (r.hi > end_any) { end_any = r.hi; job_any = r.job; }
        if (r.dst && r.hi > end_dst) { end_dst = r.hi; job_dst = r.job; }
    }
    prof_before(st);
    hipLaunchKernelGGL(resample_u8_kernel, dim3((unsigned)tiles, (unsigned)J), dim3(kRsThreads), 0, st, arena, jobs_dev, tables);
    prof_after(st, 33004, 0.0, bytes);
    RESR_CHECK_LAUNCH("resample_u8_kernel");
    return RESR_OK;
}

}  // namespace resr
