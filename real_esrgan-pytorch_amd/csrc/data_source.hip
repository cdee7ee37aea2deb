// data_source.hip -- the device-resident training data sources (device_data.py): the two launches that make one batch of tiles, and
// the one launch that makes a batch of LR / HR pairs, and the one launch that exchanges a batch with the training pair pool.
//   tile_batch   : uint8 tiles [M,T,T,3] in HBM -> the batch's fp32 [B,3,T,T]: gather by index, right-angle rotation about the
//                  integer centre (zero fill where an even side loses a row / column), horizontal / vertical flip, / 255.0f,
//                  HWC -> CHW.  Bit for bit device_data.augment_np (the imgproc chain of dataset.py).
//   pair_batch   : uint8 images of any size, both sides of each pair in an arena -> fp32 LR [B,3,P,P] and HR [B,3,sP,sP]: crop, the
//                  same dihedral code on both sides, / 255.0f, HWC -> CHW.  Bit for bit device_data.paired_sample_np.
//   crop_batch   : uint8 images of any size in an arena -> fp32 [B,3,T,T]: the T x T window at (top, left), continued by reflection where
//                  the image is smaller, tile_batch's 16 codes, / 255.0f, HWC -> CHW.  Bit for bit device_data.crop_sample_np.
//   pool_exchange: fp32 batch LR [B,3,P,P] / HR [B,3,sP,sP] <-> slots of the resident pool [Q,...]: out[i] = pool[slots[i]], pool[slots[i]] =
//                  in[i], both sides, 32-bit words moved.  Bit for bit device_data.pool_exchange_np / pool_store_np.
//   blur_kernels : one record of RESR_BLUR_RECORD doubles per kernel (include/resr.h) -> fp32 [n,K,K]: the float64 synthesis of
//                  imgproc._kernel_of / generate_sinc_kernel, normalised, zero-padded to K, cast.  One workgroup per kernel.
#include <math.h>

#include "host_api.h"

namespace resr {

// ---- tile_batch ------------------------------------------------------------------------------------------------------------------
// A workgroup owns one TS x TS tile of one output image.  Under every one of the 16 codes the source pixels of such a tile are a
// TS x TS block of the source tile (rows and columns swap under 90 / 270), so the block is staged in LDS with row-contiguous
// reads -- consecutive lanes read consecutive bytes of the 3-byte pixels -- and the plane rows leave with consecutive lanes on
// consecutive floats; the permutation happens between the two, in LDS.  Source coordinates one past the tile (the column / row an
// even side loses) are staged as zeros: the fill of the rotation.
constexpr int kTileSide = 32;
constexpr int kTilePitch = kTileSide * 3 + 4;   // bytes per staged row: 25 dwords, odd, so a column walk spreads over the banks

// The 16-code permutation of one workgroup, shared by tile_batch and crop_batch: which block of the source the tile needs (block),
// and the tile's plane rows out of the staged block (store).
struct AugTile {
    int T, x0, y0, x_end, y_end;   // the side; the tile's first and last destination column / row
    int rot, c2;                   // angle / 90; cx + cy of the rotation about (T / 2, T / 2)
    bool hf, vf;
    int sx_lo, sy_lo;              // the source block: columns sx_lo.., rows sy_lo.. (>= 0 for every code; at most T, one past the side)

    // source coordinates of destination (x, y): rot 0: (x1, y1); 90: (c2 - y1, x1); 180: (c2 - x1, c2 - y1); 270: (y1, c2 - x1)
    __device__ __forceinline__ void source(int x1, int y1, int& sx, int& sy) const {
        switch (rot) {
            case 0: sx = x1; sy = y1; break;
            case 1: sx = c2 - y1; sy = x1; break;
            case 2: sx = c2 - x1; sy = c2 - y1; break;
            default: sx = y1; sy = c2 - x1; break;
        }
    }

    __device__ __forceinline__ AugTile(int code, int T_, int tile, int tiles_x) : T(T_) {
        x0 = (int)((unsigned)tile % (unsigned)tiles_x) * kTileSide;
        y0 = (int)((unsigned)tile / (unsigned)tiles_x) * kTileSide;
        rot = code & 3;
        hf = code & 4;
        vf = code & 8;
        x_end = min(x0 + kTileSide, T) - 1;
        y_end = min(y0 + kTileSide, T) - 1;
        // the tile's coordinates before the flips (x1, y1): an interval each
        const int x1_lo = hf ? T - 1 - x_end : x0, x1_hi = hf ? T - 1 - x0 : x_end;
        const int y1_lo = vf ? T - 1 - y_end : y0, y1_hi = vf ? T - 1 - y0 : y_end;
        c2 = 2 * (T / 2);
        switch (rot) {
            case 0: sx_lo = x1_lo; sy_lo = y1_lo; break;
            case 1: sx_lo = c2 - y1_hi; sy_lo = x1_lo; break;
            case 2: sx_lo = c2 - x1_hi; sy_lo = c2 - y1_hi; break;
            default: sx_lo = y1_lo; sy_lo = c2 - x1_hi; break;
        }
    }

    // after the barrier behind the staging: the tile of image `dst` [3, T, T], consecutive lanes on consecutive floats of a plane row
    __device__ __forceinline__ void store(const uint8_t* lds, float* __restrict__ dst) const {
        const int tx = (int)(threadIdx.x & 31u), x = x0 + tx;
        if (x > x_end) return;
        const int x1 = hf ? T - 1 - x : x;
        const size_t plane = (size_t)T * (size_t)T;
        for (int ty = (int)(threadIdx.x >> 5); ty < kTileSide; ty += 8) {
            const int y = y0 + ty;
            if (y > y_end) break;
            const int y1 = vf ? T - 1 - y : y;
            int sx, sy;
            source(x1, y1, sx, sy);
            const uint8_t* p = lds + (sy - sy_lo) * kTilePitch + (sx - sx_lo) * 3;
            float* o = dst + (size_t)y * T + x;
            o[0] = (float)p[0] / 255.0f;
            o[plane] = (float)p[1] / 255.0f;
            o[2 * plane] = (float)p[2] / 255.0f;
        }
    }
};

__global__ __launch_bounds__(256) void tile_batch_kernel(const uint8_t* __restrict__ tiles, const int32_t* __restrict__ index,
                                                         const uint8_t* __restrict__ aug, float* __restrict__ dst, int T, int tiles_x) {
    __shared__ uint8_t lds[kTileSide * kTilePitch];
    const int b = (int)blockIdx.y;
    const AugTile a(aug[b], T, (int)blockIdx.x, tiles_x);
    const uint8_t* src = tiles + (size_t)index[b] * (size_t)T * (size_t)T * 3;
    for (int i = (int)threadIdx.x; i < kTileSide * kTileSide * 3; i += 256) {
        const int r = i / (kTileSide * 3), k = i - r * (kTileSide * 3);
        const int sy = a.sy_lo + r, sx = a.sx_lo + k / 3;
        uint8_t v = 0;
        if (sy < T && sx < T) v = src[((size_t)sy * T + a.sx_lo) * 3 + k];
        lds[r * kTilePitch + k] = v;
    }
    __syncthreads();
    a.store(lds, dst + (size_t)b * 3 * (size_t)T * (size_t)T);
}

int tile_batch_dispatch(const uint8_t* tiles, const int32_t* index, const uint8_t* aug, int M, int B, int T, float* dst, hipStream_t st) {
    if (!tiles || !index || !aug || !dst || M < 1 || B < 1 || T < 1) return fail(RESR_ERR_ARG, "tile_batch: bad argument (M=%d B=%d T=%d)", M, B, T);
    const int64_t tiles_x = ((int64_t)T + kTileSide - 1) / kTileSide;
    if (tiles_x * tiles_x > 0x7fffffffLL || B > 65535) return fail(RESR_ERR_ARG, "tile_batch: grid overflow (B=%d above 65535, or T=%d)", B, T);
    prof_before(st);
    hipLaunchKernelGGL(tile_batch_kernel, dim3((unsigned)(tiles_x * tiles_x), (unsigned)B), dim3(256), 0, st, tiles, index, aug, dst, T, (int)tiles_x);
    prof_after(st, 33000, 0.0, (double)B * T * T * 15.0);
    RESR_CHECK_LAUNCH("tile_batch_kernel");
    return RESR_OK;
}

// ---- pair_batch ------------------------------------------------------------------------------------------------------------------
// The paired source (device_data.PairedDeviceSource): one launch crops, augments and converts BOTH sides of every sample.  grid.x
// runs over the 32 x 32 tiles of the LR patch [P, P] and then over those of the HR patch [sP, sP]; grid.y is the sample.  The three
// bits of the dihedral code are a horizontal flip, a vertical flip and a transpose of the crop, in that order, so -- as in tile_batch
// -- the source pixels of a tile are a block of at most 32 x 32 pixels of the crop (rows and columns swap under the transpose),
// staged through the same LDS tile.  Images have any size and start at any byte, so the arena is read byte by byte: consecutive
// lanes on consecutive bytes of a row.  Every offset is 64-bit.
__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

__global__ __launch_bounds__(256) void pair_batch_kernel(const uint8_t* __restrict__ hr_arena, const uint8_t* __restrict__ lr_arena,
                                                         const int64_t* __restrict__ table, const int32_t* __restrict__ records, int M, int P,
                                                         int scale, float* __restrict__ lr_dst, float* __restrict__ hr_dst, int lr_tiles_x,
                                                         int hr_tiles_x) {
    __shared__ uint8_t lds[kTileSide * kTilePitch];
    const int b = (int)blockIdx.y;
    const int32_t* rec = records + (size_t)b * 4;
    // nothing of a record is trusted (check_paired_records refuses a wrong one before upload): a clamped record reads inside its image
    const int image = min(max(rec[0], 0), M - 1);
    const int code = rec[3] & 7;
    const int64_t* row = table + (size_t)image * 4;
    const int64_t lr_h = row[2], lr_w = row[3];
    // (an image below the patch, which from_dirs refuses: the crop starts at 0 and the guard of the read keeps it inside)
    int64_t top = clamp64(rec[1], 0, lr_h > P ? lr_h - P : 0), left = clamp64(rec[2], 0, lr_w > P ? lr_w - P : 0);
    const unsigned lr_tiles = (unsigned)lr_tiles_x * (unsigned)lr_tiles_x;
    const bool is_hr = blockIdx.x >= lr_tiles;
    const unsigned tile = is_hr ? blockIdx.x - lr_tiles : blockIdx.x;
    const int tiles_x = is_hr ? hr_tiles_x : lr_tiles_x;
    const int s = is_hr ? scale : 1;
    const int N = s * P;                                                               // the side of this output
    const int64_t H = s * lr_h, W = s * lr_w;
    top *= s;
    left *= s;
    const uint8_t* src = is_hr ? hr_arena + row[0] : lr_arena + row[1];
    float* dst = (is_hr ? hr_dst : lr_dst) + (size_t)b * 3 * (size_t)N * (size_t)N;
    const bool hf = code & 1, vf = code & 2, tr = code & 4;
    const int x0 = (int)(tile % (unsigned)tiles_x) * kTileSide, y0 = (int)(tile / (unsigned)tiles_x) * kTileSide;
    const int x_end = min(x0 + kTileSide, N) - 1, y_end = min(y0 + kTileSide, N) - 1;  // last destination column / row of the tile
    // out[y][x] = crop[vf ? N-1-y2 : y2][hf ? N-1-x2 : x2] with (y2, x2) = tr ? (x, y) : (y, x): an interval of crop rows and one of columns
    const int r_lo = tr ? x0 : y0, r_hi = tr ? x_end : y_end, c_lo = tr ? y0 : x0, c_hi = tr ? y_end : x_end;
    const int cy_lo = vf ? N - 1 - r_hi : r_lo, cy_hi = vf ? N - 1 - r_lo : r_hi;
    const int cx_lo = hf ? N - 1 - c_hi : c_lo, cx_hi = hf ? N - 1 - c_lo : c_hi;
    for (int i = (int)threadIdx.x; i < kTileSide * kTileSide * 3; i += 256) {
        const int r = i / (kTileSide * 3), k = i - r * (kTileSide * 3);
        const int cy = cy_lo + r, cx = cx_lo + k / 3;
        const int64_t sy = top + cy, sx = left + cx;
        uint8_t v = 0;
        if (cy <= cy_hi && cx <= cx_hi && sy < H && sx < W) v = src[(sy * W + left + cx_lo) * 3 + k];
        lds[r * kTilePitch + k] = v;
    }
    __syncthreads();
    const int tx = (int)(threadIdx.x & 31u), x = x0 + tx;
    if (x > x_end) return;
    const size_t plane = (size_t)N * (size_t)N;
    for (int ty = (int)(threadIdx.x >> 5); ty < kTileSide; ty += 8) {
        const int y = y0 + ty;
        if (y > y_end) break;
        const int y2 = tr ? x : y, x2 = tr ? y : x;
        const int cy = vf ? N - 1 - y2 : y2, cx = hf ? N - 1 - x2 : x2;
        const uint8_t* p = lds + (cy - cy_lo) * kTilePitch + (cx - cx_lo) * 3;
        float* o = dst + (size_t)y * N + x;
        o[0] = (float)p[0] / 255.0f;
        o[plane] = (float)p[1] / 255.0f;
        o[2 * plane] = (float)p[2] / 255.0f;
    }
}

int pair_batch_dispatch(const uint8_t* hr_arena, const uint8_t* lr_arena, const int64_t* table, const int32_t* records, int M, int B, int P,
                        int scale, float* lr_dst, float* hr_dst, hipStream_t st) {
    if (!hr_arena || !lr_arena || !table || !records || !lr_dst || !hr_dst || M < 1 || B < 1 || P < 1 || scale < 1 || scale > 4)
        return fail(RESR_ERR_ARG, "pair_batch: bad argument (M=%d B=%d patch=%d scale=%d, scale in 1..4)", M, B, P, scale);
    const int64_t hr_side = (int64_t)scale * P;
    if (B > 65535 || hr_side > 0x7fffffffLL) return fail(RESR_ERR_ARG, "pair_batch: B=%d above 65535, or scale * patch = %lld above 2^31 - 1", B, (long long)hr_side);
    const int64_t lr_tiles_x = ((int64_t)P + kTileSide - 1) / kTileSide, hr_tiles_x = (hr_side + kTileSide - 1) / kTileSide;
    if (lr_tiles_x * lr_tiles_x + hr_tiles_x * hr_tiles_x > 0x7fffffffLL)
        return fail(RESR_ERR_ARG, "pair_batch: grid overflow (patch=%d scale=%d: %lld tiles a sample)", P, scale, (long long)(lr_tiles_x * lr_tiles_x + hr_tiles_x * hr_tiles_x));
    prof_before(st);
    hipLaunchKernelGGL(pair_batch_kernel, dim3((unsigned)(lr_tiles_x * lr_tiles_x + hr_tiles_x * hr_tiles_x), (unsigned)B), dim3(256), 0, st, hr_arena,
                       lr_arena, table, records, M, P, scale, lr_dst, hr_dst, (int)lr_tiles_x, (int)hr_tiles_x);
    prof_after(st, 33001, 0.0, (double)B * (double)P * P * 15.0 * (1.0 + (double)scale * scale));
    RESR_CHECK_LAUNCH("pair_batch_kernel");
    return RESR_OK;
}

// ---- crop_batch ------------------------------------------------------------------------------------------------------------------
// The whole-image source (device_data.ImageCropSource): images of any size in one arena, a sample the T x T window of its image at
// (top, left) under tile_batch's 16 codes.  An image below T in an axis is continued below / to the right by reflection about its last
// pixel (reflect101: the period is 2n - 2, so a pad of any width is defined).  The work split and the permutation are tile_batch's
// (AugTile); what differs is the staging.  A staged block that lies inside the image is read as pair_batch reads: row-contiguous bytes,
// consecutive lanes on consecutive bytes.  A block that reaches the padding maps every pixel through reflect101 in both axes; only
// those blocks pay for the two remainders.  Window coordinates one past T (the rotation's fill) are staged as zeros in both forms.
// Every offset is 64-bit.
__device__ __forceinline__ int64_t reflect101(uint32_t i, uint32_t n) {      // i < 2^31, 1 <= n < 2^31
    if (n == 1u) return 0;
    const uint32_t p = 2u * n - 2u, j = i % p;
    return j < n ? j : p - j;
}

__global__ __launch_bounds__(256) void crop_batch_kernel(const uint8_t* __restrict__ arena, const int64_t* __restrict__ table,
                                                         const int32_t* __restrict__ records, int M, int T, float* __restrict__ dst, int tiles_x) {
    __shared__ uint8_t lds[kTileSide * kTilePitch];
    const int b = (int)blockIdx.y;
    const int32_t* rec = records + (size_t)b * 4;
    // nothing of a record is trusted (check_crop_records refuses a wrong one before upload): a clamped record reads inside its image
    const int image = min(max(rec[0], 0), M - 1);
    const int64_t* row = table + (size_t)image * 3;
    const int64_t h = row[1], w = row[2];
    const int64_t top = clamp64(rec[1], 0, h > T ? h - T : 0), left = clamp64(rec[2], 0, w > T ? w - T : 0);
    const AugTile a(rec[3] & 15, T, (int)blockIdx.x, tiles_x);
    const uint8_t* src = arena + row[0];
    // the window rows and columns the block holds: sy_lo .. sy_hi, sx_lo .. sx_hi (the rest of the 32 x 32 is one past T, or unused)
    const int sy_hi = min(a.sy_lo + kTileSide, T) - 1, sx_hi = min(a.sx_lo + kTileSide, T) - 1;
    if (top + sy_hi < h && left + sx_hi < w) {
        for (int i = (int)threadIdx.x; i < kTileSide * kTileSide * 3; i += 256) {
            const int r = i / (kTileSide * 3), k = i - r * (kTileSide * 3);
            const int sy = a.sy_lo + r, sx = a.sx_lo + k / 3;
            uint8_t v = 0;
            if (sy <= sy_hi && sx <= sx_hi) v = src[((top + sy) * w + left + a.sx_lo) * 3 + k];
            lds[r * kTilePitch + k] = v;
        }
    } else {
        for (int i = (int)threadIdx.x; i < kTileSide * kTileSide * 3; i += 256) {
            const int r = i / (kTileSide * 3), k = i - r * (kTileSide * 3), px = k / 3;
            const int sy = a.sy_lo + r, sx = a.sx_lo + px;
            uint8_t v = 0;
            if (sy <= sy_hi && sx <= sx_hi) {
                const int64_t iy = reflect101((uint32_t)(top + sy), (uint32_t)h), ix = reflect101((uint32_t)(left + sx), (uint32_t)w);
                v = src[(iy * w + ix) * 3 + (k - px * 3)];
            }
            lds[r * kTilePitch + k] = v;
        }
    }
    __syncthreads();
    a.store(lds, dst + (size_t)b * 3 * (size_t)T * (size_t)T);
}

int crop_batch_dispatch(const uint8_t* arena, const int64_t* table, const int32_t* records, int M, int B, int T, float* dst, hipStream_t st) {
    if (!arena || !table || !records || !dst) return fail(RESR_ERR_ARG, "crop_batch: a null pointer (arena, table, records and dst are all needed)");
    if (M < 1 || B < 1 || T < 1) return fail(RESR_ERR_ARG, "crop_batch: m=%d, b=%d or t=%d below 1", M, B, T);
    if (B > 65535) return fail(RESR_ERR_ARG, "crop_batch: b=%d above 65535 (the grid's y dimension)", B);
    const int64_t tiles_x = ((int64_t)T + kTileSide - 1) / kTileSide;
    if (tiles_x * tiles_x > 0x7fffffffLL) return fail(RESR_ERR_ARG, "crop_batch: grid overflow (t=%d: %lld tiles a sample)", T, (long long)(tiles_x * tiles_x));
    prof_before(st);
    hipLaunchKernelGGL(crop_batch_kernel, dim3((unsigned)(tiles_x * tiles_x), (unsigned)B), dim3(256), 0, st, arena, table, records, M, T, dst, (int)tiles_x);
    prof_after(st, 33003, 0.0, (double)B * T * T * 15.0);
    RESR_CHECK_LAUNCH("crop_batch_kernel");
    return RESR_OK;
}

// ---- pool_exchange ---------------------------------------------------------------------------------------------------------------
// The training pair pool (device_data.PairPool): sample i of the batch changes places with slot slots[i] of the resident pool, on
// both sides, in ONE launch.  grid.y is the sample; grid.x runs over the chunks of the LR sample and then over those of the HR sample.
// A chunk is kPoolChunk 32-bit words: a thread owns kPoolVecs 16-byte vectors of it (consecutive lanes on consecutive vectors), loads
// them from in[i] and from pool[slot] -- every load before the first store, 2 * kPoolVecs * 16 bytes in flight per lane -- and stores
// them to out[i] and pool[slot].  A side whose sample is no multiple of 4 words, or one of whose base pointers is not 16-byte aligned,
// takes the scalar form of the same chunk: word by word, consecutive lanes on consecutive words, the same result.  The payload moves
// as 32-bit words, never as floats.  out == nullptr stores only (the fill of the pool).  out may be in itself: a thread has read
// every word it writes, and no other thread touches them.  Every offset is 64-bit.
constexpr int kPoolThreads = 256;
constexpr int kPoolVecs = 4;                                   // 16-byte vectors per thread and source
constexpr int kPoolChunk = kPoolThreads * kPoolVecs * 4;       // 32-bit words per chunk: 16 KiB of each tensor it touches

__global__ __launch_bounds__(kPoolThreads) void pool_exchange_kernel(uint32_t* pool_lr, uint32_t* pool_hr, const uint32_t* lr_in, const uint32_t* hr_in,
                                                                     uint32_t* lr_out, uint32_t* hr_out, const int32_t* __restrict__ slots, int Q,
                                                                     int64_t lr_elems, int64_t hr_elems, unsigned lr_chunks, int lr_vec, int hr_vec) {
    const int b = (int)blockIdx.y;
    // the slot is not trusted (check_pool_slots refuses a wrong one before upload): a clamped slot stays inside the pool
    const int slot = min(max(slots[b], 0), Q - 1);
    const bool is_hr = blockIdx.x >= lr_chunks;
    const int64_t chunk = is_hr ? blockIdx.x - lr_chunks : blockIdx.x;
    const int64_t elems = is_hr ? hr_elems : lr_elems;
    const bool vec = is_hr ? hr_vec : lr_vec;
    uint32_t* pool = (is_hr ? pool_hr : pool_lr) + (int64_t)slot * elems;
    const uint32_t* in = (is_hr ? hr_in : lr_in) + (int64_t)b * elems;
    uint32_t* out = is_hr ? hr_out : lr_out;
    const bool swap = out != nullptr;
    if (swap) out += (int64_t)b * elems;
    if (vec) {
        const int64_t count = elems >> 2, first = chunk * (kPoolThreads * kPoolVecs) + threadIdx.x;
        const uint4* in4 = reinterpret_cast<const uint4*>(in);
        uint4* pool4 = reinterpret_cast<uint4*>(pool);
        uint4* out4 = reinterpret_cast<uint4*>(out);
        uint4 a[kPoolVecs], p[kPoolVecs];
#pragma unroll
        for (int k = 0; k < kPoolVecs; ++k) {
            const int64_t i = first + k * kPoolThreads;
            a[k] = p[k] = make_uint4(0u, 0u, 0u, 0u);
            if (i < count) {
                a[k] = in4[i];
                if (swap) p[k] = pool4[i];
            }
        }
#pragma unroll
        for (int k = 0; k < kPoolVecs; ++k) {
            const int64_t i = first + k * kPoolThreads;
            if (i < count) {
                if (swap) out4[i] = p[k];
                pool4[i] = a[k];
            }
        }
    } else {
        constexpr int kWords = kPoolVecs * 4;
        const int64_t first = chunk * kPoolChunk + threadIdx.x;
        uint32_t a[kWords], p[kWords];
#pragma unroll
        for (int k = 0; k < kWords; ++k) {
            const int64_t i = first + k * kPoolThreads;
            a[k] = p[k] = 0u;
            if (i < elems) {
                a[k] = in[i];
                if (swap) p[k] = pool[i];
            }
        }
#pragma unroll
        for (int k = 0; k < kWords; ++k) {
            const int64_t i = first + k * kPoolThreads;
            if (i < elems) {
                if (swap) out[i] = p[k];
                pool[i] = a[k];
            }
        }
    }
}

// [p, p + bytes) and [q, q + bytes2) share a byte
static bool pool_overlap(const void* p, unsigned __int128 bytes, const void* q, unsigned __int128 bytes2) {
    const unsigned __int128 a = (uintptr_t)p, c = (uintptr_t)q;
    return a < c + bytes2 && c < a + bytes;
}

int pool_exchange_dispatch(float* pool_lr, float* pool_hr, const float* lr_in, const float* hr_in, float* lr_out, float* hr_out, const int32_t* slots,
                           int Q, int B, int64_t lr_elems, int64_t hr_elems, hipStream_t st) {
    if (!pool_lr || !pool_hr || !lr_in || !hr_in || !slots || (lr_out == nullptr) != (hr_out == nullptr))
        return fail(RESR_ERR_ARG, "pool_exchange: a null pointer (both outputs null = store only; exactly one null is refused)");
    if (Q < 1 || B < 1 || lr_elems < 1 || hr_elems < 1 || B > Q || B > 65535)
        return fail(RESR_ERR_ARG, "pool_exchange: bad argument (Q=%d B=%d lr_elems=%lld hr_elems=%lld; 1 <= B <= Q, B <= 65535)", Q, B, (long long)lr_elems,
                    (long long)hr_elems);
    // (rounded up without an addition that could overflow)
    const int64_t lr_chunks = lr_elems / kPoolChunk + (lr_elems % kPoolChunk != 0), hr_chunks = hr_elems / kPoolChunk + (hr_elems % kPoolChunk != 0);
    if (lr_chunks + hr_chunks > 0x7fffffffLL)
        return fail(RESR_ERR_ARG, "pool_exchange: grid overflow (lr_elems=%lld hr_elems=%lld: above 2^31 - 1 chunks of %d words a sample)", (long long)lr_elems,
                    (long long)hr_elems, kPoolChunk);
    int vec[2];
    for (int side = 0; side < 2; ++side) {
        const void* pool = side ? (const void*)pool_hr : pool_lr;
        const void* in = side ? (const void*)hr_in : lr_in;
        const void* out = side ? (const void*)hr_out : lr_out;
        const int64_t elems = side ? hr_elems : lr_elems;
        const unsigned __int128 pool_bytes = (unsigned __int128)Q * elems * 4, batch_bytes = (unsigned __int128)B * elems * 4;
        if (pool_overlap(pool, pool_bytes, in, batch_bytes) || (out && pool_overlap(pool, pool_bytes, out, batch_bytes)) ||
            (out && out != in && pool_overlap(in, batch_bytes, out, batch_bytes)))
            return fail(RESR_ERR_ARG, "pool_exchange: the %s pool, input and output overlap (an output may only be exactly its input)", side ? "hr" : "lr");
        vec[side] = elems % 4 == 0 && (((uintptr_t)pool | (uintptr_t)in | (uintptr_t)out) & 15u) == 0;
    }
    prof_before(st);
    hipLaunchKernelGGL(pool_exchange_kernel, dim3((unsigned)(lr_chunks + hr_chunks), (unsigned)B), dim3(kPoolThreads), 0, st, (uint32_t*)pool_lr,
                       (uint32_t*)pool_hr, (const uint32_t*)lr_in, (const uint32_t*)hr_in, (uint32_t*)lr_out, (uint32_t*)hr_out, slots, Q, lr_elems, hr_elems,
                       (unsigned)lr_chunks, vec[0], vec[1]);
    prof_after(st, 33002, 0.0, (double)B * ((double)lr_elems + (double)hr_elems) * (lr_out ? 16.0 : 8.0));
    RESR_CHECK_LAUNCH("pool_exchange_kernel");
    return RESR_OK;
}

// ---- blur_kernels ----------------------------------------------------------------------------------------------------------------
constexpr int kBlurMaxSide = RESR_BLUR_MAX_SIDE;
constexpr int kBlurThreads = 256;

// sum of v[0 .. count) in a fixed order: thread t adds v[t], v[t + 256], ... in that order, then the 256 partial sums halve in LDS.
// Every thread returns the same double; the bits do not depend on the launch.
__device__ __forceinline__ double fixed_sum(const double* v, int count, double* part) {
    double s = 0.0;
    for (int i = (int)threadIdx.x; i < count; i += kBlurThreads) s += v[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int half = kBlurThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) part[threadIdx.x] += part[threadIdx.x + half];
        __syncthreads();
    }
    const double total = part[0];
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(kBlurThreads) void blur_kernels_kernel(const double* __restrict__ params, float* __restrict__ dst, int K) {
    __shared__ double taps[kBlurMaxSide * kBlurMaxSide];
    __shared__ double part[kBlurThreads];
    const double* r = params + (size_t)blockIdx.x * RESR_BLUR_RECORD;
    const int family = (int)r[0];
    int side = (int)r[1];
    side = side < 1 ? 1 : side > K ? K : side;   // (refused before upload; never index past the LDS tile)
    const int count = side * side;
    const double half_side = (double)(side / 2);
    if (family == RESR_BLUR_DELTA) {
        for (int i = (int)threadIdx.x; i < count; i += kBlurThreads) taps[i] = i == count / 2 ? 1.0 : 0.0;
        __syncthreads();
    } else if (family == RESR_BLUR_SINC) {
        const double cutoff = r[7];
        for (int i = (int)threadIdx.x; i < count; i += kBlurThreads) {
            const double dy = (double)(i / side) - half_side, dx = (double)(i % side) - half_side;
            const double rad = sqrt(dy * dy + dx * dx);
            taps[i] = i == count / 2 ? cutoff * cutoff / (4.0 * M_PI) : cutoff * j1(cutoff * rad) / (2.0 * M_PI * rad);
        }
        __syncthreads();
        const double total = fixed_sum(taps, count, part);
        for (int i = (int)threadIdx.x; i < count; i += kBlurThreads) taps[i] = taps[i] / total;
        __syncthreads();
    } else {
        // inverse of cov = R diag(sx^2, sy^2) R^T in closed form (isotropic: diag(sx^2, sx^2))
        const double sx2 = r[2] * r[2], sy2 = r[3] * r[3], beta = r[5];
        double i00, i01, i10, i11;
        if (r[6] != 0.0) {
            const double c = cos(r[4]), s = sin(r[4]);
            const double a00 = c * sx2 * c + s * sy2 * s, a01 = c * sx2 * s - s * sy2 * c, a11 = s * sx2 * s + c * sy2 * c;
            const double det = a00 * a11 - a01 * a01;
            i00 = a11 / det; i01 = -a01 / det; i10 = i01; i11 = a00 / det;
        } else {
            i00 = i11 = 1.0 / sx2; i01 = i10 = 0.0;
        }
        for (int i = (int)threadIdx.x; i < count; i += kBlurThreads) {
            const double y = (double)(i / side) - half_side, x = (double)(i % side) - half_side;
            const double q = (x * i00 + y * i10) * x + (x * i01 + y * i11) * y;
            double v;
            if (family == RESR_BLUR_GAUSSIAN) v = exp(-0.5 * q);
            else if (family == RESR_BLUR_GENERALIZED) v = exp(-0.5 * pow(q, beta));
            else v = 1.0 / (pow(q, beta) + 1.0);
            taps[i] = v;
        }
        __syncthreads();
        for (int pass = 0; pass < 2; ++pass) {   // imgproc._kernel_of normalises, random_mixed_kernels normalises again
            const double total = fixed_sum(taps, count, part);
            for (int i = (int)threadIdx.x; i < count; i += kBlurThreads) taps[i] = taps[i] / total;
            __syncthreads();
        }
    }
    const int pad = (K - side) / 2;
    float* out = dst + (size_t)blockIdx.x * (size_t)K * (size_t)K;
    for (int i = (int)threadIdx.x; i < K * K; i += kBlurThreads) {
        const int y = i / K - pad, x = i % K - pad;
        out[i] = (y >= 0 && y < side && x >= 0 && x < side) ? (float)taps[y * side + x] : 0.f;
    }
}

int blur_kernels_dispatch(const double* params, int n, int K, float* dst, hipStream_t st) {
    if (!params || !dst || n < 1 || K < 1 || (K & 1) == 0 || K > kBlurMaxSide) return fail(RESR_ERR_ARG, "blur_kernels: bad argument (n=%d K=%d, K odd and at most %d)", n, K, kBlurMaxSide);
    prof_before(st);
    hipLaunchKernelGGL(blur_kernels_kernel, dim3((unsigned)n), dim3(kBlurThreads), 0, st, params, dst, K);
    prof_after(st, 33100, 0.0, (double)n * (RESR_BLUR_RECORD * 8.0 + 4.0 * K * K));
    RESR_CHECK_LAUNCH("blur_kernels_kernel");
    return RESR_OK;
}

}  // namespace resr
