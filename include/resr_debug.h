/*
 * resr_debug.h -- test and measurement aids of libresr_hip.so.  Exported, but NOT part of the drop-in contract of resr.h:
 * nothing in the product path (model.py, train.py, inference.py ...) needs them; tests/, tools/ and bench.py do.
 * Unlike the entry points of resr.h, resr_debug_chain_errors and resr_profile_end synchronise.
 */
#ifndef RESR_DEBUG_H_
#define RESR_DEBUG_H_

#include "resr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Debug: per-workgroup timeline of the fast-mode conv kernel (32 workgroups x 2 roles x 64 uint64 stamps, 100 MHz).  The stamps
 * are compiled in by a trace build only (-DRESR_TRACE=1, tools/build_variant.py); in the product build the buffer stays untouched. */
int resr_debug_conv_trace(void* dev_buf);
/* Debug / test: resr_chain_errors() after a hipDeviceSynchronize() (every launch enqueued so far has reported).
 * RESR_CONV_NO_CHAIN=1 in the environment disables chaining. */
int64_t resr_debug_chain_errors(void);
/* Test aid: `workgroups` single-wave workgroups that each hold `lds_bytes` of LDS and spin for `micros` microseconds -- what a
 * collective of another stream looks like to a chained launch that wants every CU. */
int resr_debug_occupy(int32_t workgroups, int32_t lds_bytes, int32_t micros, void* stream);
/* Host logic of the f16 weight-gradient launch, no GPU needed: how the (X chunk, G tile) products of `nconv` convolutions
 * that read one channel-prefix workspace (conv i: the first cin[i] channels; its own cout_pad[i] gradient channels) are
 * grouped into 2x2 jobs of the quad kernel.  out[q*4 + p] = index of the product computed by slot p of job q (products are
 * numbered conv-major, then G tile, then X chunk), -1 = slot unused.  Returns the number of jobs (<= max_jobs) or < 0. */
int resr_debug_wgrad_plan(const int32_t* cin, const int32_t* cout_pad, int32_t nconv, int32_t* out, int32_t max_jobs);
/* Measurement aid (tools/energy.py): the weight-gradient launch pair the generator's backward pass issues per RRDB -- the five
 * convolutions of `nblocks` (1..3) dense blocks, 26 products each, as ONE batched launch -- on caller-made f16 operands.
 * x_ws[b]: chunk-planar [6][n,h,w,32] (conv_k reads the first 2 + (k - 1) planes); g_ws[b]: chunk-planar [6][n,h,w,32] (planes
 * 0,1 = the closing convolution's 64 gradient channels, plane 1 + k = conv_k's 32); dw: nblocks * 26624 * 9 floats;
 * partial: `partial_bytes` of slab scratch (26 * nblocks * splits slabs of kSlab floats: csrc/wgrad.h, wgrad_slab_bytes). */
int resr_debug_wgrad_dense_blocks(int32_t nblocks, const void* const* x_ws, const void* const* g_ws, int32_t n, int32_t h, int32_t w,
                                  int32_t splits, float* partial, size_t partial_bytes, float* dw, void* stream);
/* test probe: lane/element map of ds_read_b64_tr_b16 (256 floats out) */
int resr_debug_tr_probe(float* out256, void* stream);

/* Test entries (tests/test_gpu_disc_helpers.py) of the discriminator helpers that the product reaches only from inside the native
 * passes (csrc/disc_native.hip): the existing dispatch functions, callable alone.  Shapes, types and RESR_F16X2 pairs as for the
 * helpers of resr.h -- every lo tensor directly behind its hi tensor.
 * resr_debug_d2s_add_mask: out[n,h,w,c] = (depth_to_space(src[n,h/2,w/2,4c]) + add) * (mask > 0 ? 1 : slope); add, mask optional,
 *   both of out's shape.  The sign of a RESR_F16X2 mask is its hi tensor's, or its lo tensor's where hi is zero.
 * resr_debug_bilinear_up2x_bwd_mask: gin[n,h,w,c] = resr_bilinear_up2x's backward of g[n,2h,2w,c], and in the same pass
 *   gmasked = gin * (mask > 0 ? 1 : slope); the mask (same sign rule) and gmasked have gin's shape. */
int resr_debug_d2s_add_mask(const void* src, const void* add, const void* mask, void* out, int32_t n, int32_t h, int32_t w, int32_t c,
                            int32_t dtype, float slope, void* stream);
int resr_debug_bilinear_up2x_bwd_mask(const void* g, void* gin, const void* mask, void* gmasked, int32_t n, int32_t h, int32_t w,
                                      int32_t c, int32_t dtype, float slope, void* stream);
/* The batched launches: `n` layers at once (<= 8; fold: <= 4) through HOST arrays of device pointers and of sizes; per layer the
 * operands of resr_spectral_norm / resr_spectral_norm_bwd (accumulate = 0) / resr_fold4x4, and bit-identical results.
 * tmp[i] = rows[i] + ceil(rows[i] / 32) * cols[i] floats; dot = 8 * 512 floats shared by the layers. */
int resr_debug_spectral_norm_batch(int32_t n, const float* const* w, float* const* u, float* const* v, const int32_t* rows,
                                   const int32_t* cols, int32_t training, float eps, float* const* sigma2, float* const* tmp,
                                   void* stream);
int resr_debug_spectral_norm_bwd_batch(int32_t n, const float* const* g, const float* const* w, const float* const* u,
                                       const float* const* v, const float* const* sigma2, float* const* dst, const int32_t* rows,
                                       const int32_t* cols, float* dot, void* stream);
int resr_debug_fold4x4_batch(int32_t n, const float* const* dw3, float* const* dw4, const int32_t* cout, const int32_t* c,
                             void* stream);

/* Test entry (tests/test_gpu_pad_skip.py): resr_nchw_to_nhwc with the gradient prescale the generator's backward pass applies to its
 * incoming gradient.  amax: device pointer to the bits of a float m (what the pass's absmax kernel leaves), or NULL: src is read times
 * 2^-floor(log2 m) where 2^-126 <= m < 1, times 1 otherwise.  RESR_NO_PAD_SKIP=1 in the environment (read per call) sends every
 * argument combination to the generic kernel, and the 21 x 21 taps of resr_filter2d through their zero border. */
int resr_debug_nchw_to_nhwc(const float* src, void* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t unshuffle, int32_t c_pad,
                            int32_t dtype, const uint8_t* mask, const void* amax, void* stream);

/* Test entries (tests/test_gpu_layout_kernels.py) of the layout kernels as the generator's passes call them (csrc/layout.hip): the
 * dispatch functions with every argument visible.  Offsets count elements of the tensor's type from the hi tensor; a negative lo offset
 * means "directly behind the hi tensor", the default of the entries of resr.h; 0 where the dtype is not RESR_F16X2.
 * resr_debug_absmax: slot[0] = the bits of m = max |src[i]| * 2^-target_log2 (|target_log2| <= 64; a NaN beats every number), after
 *   the sticky back-off (csrc/common.h, grad_prescale): slot[1] = b (clamped to 40, raised by 4 and slot[2] cleared when slot[2] != 0),
 *   and a normal m leaves times 2^b, its exponent clamped below infinity.  slot: three 32-bit words of device memory.
 * resr_debug_add_inplace: dst += src over `count` elements (a multiple of 16 bytes' worth); RESR_F16X2 needs both lo offsets > 0.
 * resr_debug_nchw_to_nhwc_q: resr_debug_nchw_to_nhwc with the lo offset named and, q_off != 0 (RESR_F16X2, c_pad % 32 == 0), the q
 *   tensor of ResrConvDesc written q_off elements behind dst.
 * resr_debug_nhwc_to_nchw: resr_nhwc_to_nchw with the lo offset named; amax != NULL: the result leaves times 2^floor(log2 m), the
 *   inverse of what resr_debug_nchw_to_nhwc applied for the same slot.
 * resr_debug_sumpool2x2: resr_sumpool2x2 with the lo offsets of src and of dst (and mask) named: one plane of a larger tensor. */
int resr_debug_absmax(const float* src, int64_t count, void* slot, int32_t target_log2, void* stream);
int resr_debug_add_inplace(void* dst, const void* src, int64_t count, int32_t dtype, int64_t dst_lo, int64_t src_lo, void* stream);
int resr_debug_nchw_to_nhwc_q(const float* src, void* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t unshuffle, int32_t c_pad,
                              int32_t dtype, const uint8_t* mask, int64_t lo_off, const void* amax, int64_t q_off, void* stream);
int resr_debug_nhwc_to_nchw(const void* src, float* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t shuffle, int32_t src_stride,
                            int32_t dtype, int64_t lo_off, const void* amax, void* stream);
int resr_debug_sumpool2x2(const void* src, void* dst, const void* mask, int32_t n, int32_t h_out, int32_t w_out, int32_t c, int32_t dtype,
                          float slope, int64_t src_lo, int64_t dst_lo, void* stream);

/* Test entry (tests/test_gpu_kernels.py) of the compact generator's body pass, which the product reaches only from inside
 * resr_compact_forward*: resr_conv3x3 on one input tensor with a plain epilogue (flags: RESR_CONV_NO_BIAS or 0; NHWC output of one
 * output group) followed by per-output-channel PReLU, v = v > 0 ? v : prelu[co] * v, `prelu` = d->cout floats.  bias may be NULL. */
int resr_debug_conv3x3_prelu(const ResrConvDesc* d, const void* in0, const void* w_packed, const float* bias, const float* prelu,
                             void* out, void* stream);

/* Test entries (tests/test_gpu_compact_train_kernels.py) of the three kernels of the compact generator's training pass, which the
 * product reaches only from inside resr_compact_forward_train / resr_compact_backward (csrc/compact_train.hip).  z, a, g, gz:
 * [pixels][64] NHWC tensors of `dtype` (RESR_F16 or RESR_F32), 16-byte aligned; slopes: 64 floats on the device.
 * resr_debug_compact_act: a = z > 0 ? z : slopes[c] * z, evaluated in fp32 and rounded once to the dtype.
 * resr_debug_compact_act_bwd: gz = g * (z > 0 ? 1 : slopes[c]), the same way; gz may be g.  dslope != NULL: also the 64 sums
 *   dslope[c] = sum_pixels g * (z > 0 ? 0 : z) in fp32, in a fixed order (the same bits run to run), through `partial`: at least
 *   min(1024, ceil(pixels * (dtype == RESR_F32 ? 16 : 8) / 256)) * 256 bytes of device scratch (else RESR_ERR_WORKSPACE); amax != NULL:
 *   they leave times 2^floor(log2 m) for the float m whose bits the slot holds, as resr_debug_nhwc_to_nchw's results do.
 * resr_debug_compact_residual_bwd: gx[n,c,y,x] += sum_{i,j < s} gy[n,c,s y + i,s x + j] for gy [n,3,h s,w s] fp32, s = 1..4: the adjoint
 *   of the nearest-upsampled residual, summed over (i, j) in this order and ADDED (one fp32 add) to what gx [n,3,h,w] holds. */
int resr_debug_compact_act(const void* z, void* a, const float* slopes, int64_t pixels, int32_t dtype, void* stream);
int resr_debug_compact_act_bwd(const void* g, const void* z, void* gz, const float* slopes, int64_t pixels, int32_t dtype, float* dslope,
                               float* partial, size_t partial_bytes, const void* amax, void* stream);
int resr_debug_compact_residual_bwd(const float* gy, float* gx, int32_t n, int32_t h, int32_t w, int32_t s, void* stream);

/* Test entry (tests/test_resize_surface.py, tests/test_gpu_resize_kernel.py): the launch plan of csrc/image_resize.hip, host only -- no
 * device work, no tables.  What resr_image_resize and the scaled frame entries would launch for n sources of c x h x w resized to
 * oh x ow through tables of taps_y / taps_x taps; kind: 0 fp32 NCHW output, 1 uint8 HWC, 2 / 3 a YUV 4:2:0 frame of 8- / 10-bit
 * samples.  plan: six int32 -- the output tile th, tw; the capacity rh, rw of the staged source region; its LDS row pitch in
 * floats; the LDS bytes of one workgroup.  Returns the status of that plan (RESR_ERR_ARG where the launch would be refused: a bad
 * shape, no tile that fits ...), then `plan` is untouched. */
int resr_debug_resize_plan(int32_t n, int32_t c, int32_t h, int32_t w, int32_t oh, int32_t ow, int32_t taps_y, int32_t taps_x,
                           int32_t kind, int32_t* plan);
/* ... and of the image modes' scaled tail (tests/test_image_outscale_surface.py, tests/test_gpu_image_outscale.py): what
 * resr_compact_forward_image_scaled launches for h x w images of `channels` x `bits` through a model of factor s resized to oh x ow --
 * the same six int32, the staging buffer `channels` words of bits / 8 bytes per pixel of the tile (8-bit RGB: the uint8 plan, kind 1
 * above).  RESR_ERR_ARG where resr_compact_image_scaled_fits says 0, then `plan` is untouched. */
int resr_debug_image_resize_plan(int32_t h, int32_t w, int32_t s, int32_t oh, int32_t ow, int32_t taps_y, int32_t taps_x, int32_t channels,
                                 int32_t bits, int32_t* plan);

/* What THIS board sustains once it sits at its power cap (bench.py's `roofline.vs_sustained`): 256 workgroups launched back to
 * back for `seconds` (last third timed) -- mode 1: an LDS-DMA stream over `src` (`bytes` >= 64 MB of readable device memory),
 * mode 2: eight waves per workgroup issuing v_mfma_f32_32x32x16_f16 on random f16 operands, mode 3: both at once.  Returns the
 * stream's TB/s and the matrix waves' executed PFLOP/s; counter8 = 8 bytes of device scratch.  Synchronises. */
int resr_debug_sustained(int32_t mode, double seconds, const void* src, size_t bytes, void* counter8, double* stream_tbs,
                         double* matrix_pflops, void* stream);

/* In-situ kernel timing for bench.py: between begin and end every conv3x3 / wgrad launch is bracketed by HIP events
 * on its launch stream.  kernel_id = dtype*10000 + MT*100 + NT*10 + NW for conv3x3_kernel<T,MT,NT,NW>,
 * 50000 + dtype*100 + RPW for wgrad_kernel<T,RPW>.  resr_profile_end synchronises the events (host-side, test/bench
 * only), fills up to `capacity` entries and returns the number recorded. */
typedef struct {
    int32_t kernel_id;
    float ms;
    double flop;  /* algorithmic FLOP of the launch: 2*9*cin*cout*pixels */
    double bytes; /* algorithmic HBM bytes of the launch: every operand plane read / written once (no halo, no re-reads) */
} ResrProfEntry;
int resr_profile_begin(void);
int64_t resr_profile_end(ResrProfEntry* out, int64_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* RESR_DEBUG_H_ */
