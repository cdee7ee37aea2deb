// Shared host/device helpers for libresr_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "resr.h"
#include "resr_debug.h"

namespace resr {

typedef _Float16 half_t;
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float4v __attribute__((ext_vector_type(4)));
typedef unsigned uint2v __attribute__((ext_vector_type(2)));
typedef float float16v __attribute__((ext_vector_type(16)));

// thread-local error text for resr_last_error()
char* err_buf();
int fail(int code, const char* fmt, ...);

#define RESR_CHECK_LAUNCH(name)                                                        \
    do {                                                                               \
        hipError_t e_ = hipGetLastError();                                             \
        if (e_ != hipSuccess) return fail(RESR_ERR_LAUNCH, "%s: %s", name, hipGetErrorString(e_)); \
    } while (0)

// optional in-situ kernel timing (resr_profile_begin/end): HIP events around individual launches on the launch stream
bool prof_on();
void prof_before(hipStream_t st);
void prof_after(hipStream_t st, int kernel_id, double flop, double bytes = 0.0);

// bytes per stored element (RESR_F16X2: of one f16 tensor of the hi/lo pair) / tensors per activation
inline size_t elem_size(int dtype) { return dtype == RESR_F32 ? 4 : 2; }
inline size_t act_tensors(int dtype) { return dtype == RESR_F16X2 ? 2 : 1; }
// RESR_F16X2: value = hi + lo * kLoInv, lo = (value - hi) * kLoScale; packed weights carry the factor kLoScale
constexpr float kLoScale = 4096.f, kLoInv = 1.f / 4096.f;
constexpr int kMaxDevices = 16;   // per-device caches (occupancy, zero pages, CU counts) are indexed by hipGetDevice()
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// RESR_NO_PAD_SKIP in the environment (read per call; A/B arm and test control): the kernels that skip work on padding -- the few-channel
// nchw_to_nhwc (layout.hip) and the zero border of the 21 x 21 blur taps (degrade.hip) -- give way to the paths that compute on it
inline bool no_pad_skip() { return getenv("RESR_NO_PAD_SKIP") != nullptr; }
// RESR_DEGRADE_PARENT_KERNELS in the environment (read per call; A/B arm and test control): USMSharp and DiffJPEG run the kernels they
// had before usm51_stream_kernel / jpeg_run_kernel (degrade.hip) -- same bits, the older schedule
inline bool degrade_parent_kernels() { return getenv("RESR_DEGRADE_PARENT_KERNELS") != nullptr; }

// A runtime upscale factor s in {1, 2, 3, 4} as a compile-time one: f(std::integral_constant<int, s>()); false for any other s.
template <typename F>
inline bool with_scale(int s, F&& f) {
    switch (s) {
        case 1: f(std::integral_constant<int, 1>()); return true;
        case 2: f(std::integral_constant<int, 2>()); return true;
        case 3: f(std::integral_constant<int, 3>()); return true;
        case 4: f(std::integral_constant<int, 4>()); return true;
        default: return false;
    }
}

// RESR_F16X2 (lo_off != 0 with T = f16): every tensor of T is a (hi, lo) pair, lo at element offset lo_off; values are
// split / recombined in fp32 (see include/resr.h).  Shared by layout.hip and frames.hip: one rounding for every way in.
__device__ __forceinline__ void split_f16(float v, half_t& hi, half_t& lo) {
    hi = (half_t)v;
    lo = (half_t)((v - (float)hi) * kLoScale);
}

// Power-of-two gradient pre-scale of a backward pass (generator.hip, RESR_F16X2).  absmax_dispatch (layout.hip) leaves the bits of
// m = max |g_y| * 2^-t; when m < 1 the pass runs on g_y * s with s = 2^-floor(log2 m) -- max |g_y * s| in [2^t, 2^(t+1)): f16's
// normal range however small the caller's loss scale is -- and every result leaves through * 1/s.  Both factors are exact.  Gradients
// that are large enough already (m >= 1) are left alone (s = 1): a GradScaler that keeps doubling its scale still meets f16's
// overflow and settles below it, as it does without the pre-scale.  Zero, denormal or non-finite maxima give s = 1.
// The slot is a block of words in memory the caller zero-fills once (the head of a generator / discriminator workspace):
//   [0] the bits of m, rewritten by every pass (absmax_dispatch)
//   [1] back-off b (sticky): the lift aims 2^b lower -- m is stored times 2^b -- once a LIFTED pass has produced a non-finite weight
//       gradient: a gradient that grows by more than the 2^9 of headroom on its way back overflows f16 at EVERY loss scale when the lift
//       re-raises it each step, so a GradScaler backing off could no longer cure it (found_inf would fire until its scale decays to
//       nothing).  Every such pass lowers the target by 2^4 (up to 2^40: then the lift is effectively off and the caller's scale rules,
//       as before round 5); the pass that overflowed is the GradScaler's to skip, the next one runs with headroom.
//   [2] flag: set by the weight-gradient reductions of a lifted pass that wrote a non-finite value; consumed by the next absmax_dispatch
constexpr int kPrescaleBackoffStep = 4, kPrescaleBackoffMax = 40;
__host__ __device__ __forceinline__ bool grad_prescale_lifted(unsigned amax_bits) {
    const unsigned e = (amax_bits >> 23) & 0xffu;
    return e != 0u && e < 127u;
}
__host__ __device__ __forceinline__ float grad_prescale(unsigned amax_bits, bool inverse) {
    const unsigned e = (amax_bits >> 23) & 0xffu;          // biased exponent of m
    if (e == 0u || e >= 127u) return 1.f;
    const unsigned f = (inverse ? e : 254u - e) << 23;     // 2^(e - 127) or 2^(127 - e)
    return __builtin_bit_cast(float, f);
}

// RESR_F16X2: "is this saved activation positive" for a LeakyReLU-backward mask read from a (hi, lo) pair.  hi decides unless it
// rounded to zero (|v| < 2^-25, below f16's subnormals); then the lo tensor (v * 2^12) carries the sign.
__device__ __forceinline__ bool pair_positive(half_t hi, half_t lo) {
    return (float)hi > 0.f || ((float)hi == 0.f && (float)lo > 0.f);
}

// MI355X: blocks are dealt round-robin to the 8 XCDs (block b -> XCD b % 8).  Give every XCD a
// contiguous range of tiles so neighbouring tiles (shared halo rows, same weights) meet in one L2.
// Bijective for any grid size.
__device__ __forceinline__ int xcd_remap(int b, int nwg) {
    const int q = nwg >> 3, r = nwg & 7;
    const int xcd = b & 7, idx = b >> 3;
    const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

// image_resize.hip: one planned resize launch (resize_plan fills it on the host; the kernels take it by value)
struct ResizeGeom {
    int c, h, w;          // source: channels, rows, columns (of the HR frame on the fused path)
    int oh, ow;
    int py, px;           // taps per output row / column
    int th, tw;           // output tile
    int rh, rw, pitch;    // capacity of the staged region, LDS row pitch (floats)
    int cgroups;          // ceil(c / 3)
};
// ... and what it stores: fp32 NCHW, a YUV 4:2:0 frame of 8- or 10-bit samples (even tiles only, and a staging buffer of levels as
// wide as the sample's word), or an image batch [N,oh,ow,C] of bytes or 16-bit words, C words per pixel in the staging buffer:
// resize_image_kind.  RESIZE_U8 is the (3, 8) image kind, uint8 HWC frames; the others are RESIZE_IMAGE + 2 * C + (16 bits).
enum ResizeOut { RESIZE_F32 = 0, RESIZE_U8 = 1, RESIZE_YUV8 = 2, RESIZE_YUV10 = 3, RESIZE_IMAGE = 4 };
constexpr int resize_image_kind(int channels, int bits) { return channels == 3 && bits == 8 ? RESIZE_U8 : RESIZE_IMAGE + 2 * channels + (bits == 16); }
constexpr bool resize_is_image(int kind) { return kind == RESIZE_U8 || kind >= RESIZE_IMAGE; }
constexpr int resize_image_channels(int kind) { return kind == RESIZE_U8 ? 3 : (kind - RESIZE_IMAGE) >> 1; }
constexpr int resize_image_word_bytes(int kind) { return kind == RESIZE_U8 ? 1 : 1 + ((kind - RESIZE_IMAGE) & 1); }

// uint8 RGB frames [N,H,W,3] are the (3, 8) image mode: what the uint8-typed entries pass where an image entry passes its descriptor.
// Its launches keep the profiling ids they had before they were an image mode's (image_id: the id of that mode, of any other).
inline const ResrImageDesc kRgb8{3, 8};
inline int image_id(const ResrImageDesc* m, int rgb8, int other) { return m->channels == 3 && m->bits == 8 ? rgb8 : other; }

// compact.hip: the two ends of one forward pass (compact_forward_ends; api.hip builds one per entry): what x and y are, and what
// else that kind of end needs.
struct ScaledTail {
    int oh, ow, taps_y, taps_x;
    const int32_t *idx_y, *idx_x;
    const float *w_y, *w_x;
};
enum EndFormat {
    END_F32,    // x [N,3,H,W] fp32 -> y [N,3,sH,sW] fp32: layout.hip's head, compact_tail
    END_YUV,    // x [N,3H/2,W] -> y [N,3sH/2,sW], YUV 4:2:0 frames of bytes or 16-bit words (src->layout, dst->layout): the colour conversions too
    END_IMAGE,  // x [N,H,W,C] -> y [N,sH,sW,C], grey / RGB / RGBA images of bytes or 16-bit words (img; uint8 RGB frames: kRgb8): frames.hip, the
                // conversions fused into the head and the tail; the network's batch is planes * N
};
struct Ends {
    EndFormat format;
    bool scaled;             // END_YUV, END_IMAGE: y is the frame resized to sc.oh x sc.ow by the tail of image_resize.hip
    const void* x;
    void* y;
    ScaledTail sc;           // scaled
    const ResrYuvDesc* src;  // END_YUV: what the frames of x are (layout, matrix tables), else null
    const ResrYuvDesc* dst;  // END_YUV: what the frames of y are; the same-format entries pass src again
    int bits_expected;       // END_YUV: the depth the entry is for, 8 or 10 (a descriptor of another is refused); 0: the mixed
                             // entries, any depth on either side
    const ResrImageDesc* img;  // END_IMAGE: channels and bits of x and y, else null
};

}  // namespace resr
