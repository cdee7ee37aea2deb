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
/* Host logic of a whole batched weight-gradient launch (csrc/wgrad.hip, wgrad_batch), no GPU needed and no HIP call made: the library's
 * planner runs on `nconv` (<= 16) convolutions whose operands lie at synthetic, never-dereferenced addresses, and the tables it would hand
 * to its kernels come back as integers (tests/test_wgrad_plan.py, tests/golden/gen_wgrad_plan_golden.py).  RESR_X2_WGRAD_PRODUCTS is read
 * per call, as by the launch.
 * convs: RESR_DEBUG_WGRAD_CONV_FIELDS int32 per convolution --
 *    0 cin   1 cin0 (< cin: channels [cin0, cin) come from a second X tensor)   2 cin_real   3 cout   4 cout_pad   5 has a bias
 *    6 X chunk-planar (else interleaved)   7 G chunk-planar   8 pixel stride of X   9 ... of the second X tensor   10 ... of G  (elements)
 *   11 buffer id of X   12 ... of the second X tensor   13 ... of G (0..63: convolutions that name one id read one tensor)
 *   14 first 32-channel tile of G inside its buffer (0..63)
 *   15 G has a lo tensor (0: single f16)   16 g_lo_bias_only   17 x_pair_chunks   18 x_single_g_hi   19 X and G carry q tensors
 *   20 x_s2d_c   21 id of the `unscale` pointer (0: none)          (15..19: RESR_F16X2, the fields of csrc/wgrad.h WgradConv)
 * dtype, n, h, w, flags (RESR_CONV_UPSAMPLE_IN or 0), splits: as wgrad_batch takes them.
 * totals: RESR_DEBUG_WGRAD_TOTALS int32 -- 0 tap-product jobs  1 algorithmic products  2 MX jobs  3 quads of the f16 launch (0: the pair
 *   kernel runs)  4 quads of the MX launch  5 splits_mx  6 splits_c  7 fast_addr  8 wgrad_batch_jobs  9 wgrad_batch_quads
 *   10 wgrad_batch_partial_bytes / 4 -- the last three as the planners ask them for the same batch.
 * jobs: RESR_DEBUG_WGRAD_JOB_FIELDS per job (room for 96) -- 0 X operand  1 G operand (each numbered in order of first appearance)
 *   2 part (0 (x_hi, g_hi)  1 (x_hi, g_lo)  2 (x_lo, g_hi)  3 MX)  3 slab_off  4 want_bias  5 xsub  6 mx  7 xstride_b  8 gstride_b.
 * reduce: RESR_DEBUG_WGRAD_REDUCE_FIELDS per product (room for 80) -- 0 slab_off  1 slab_b  2 slab_c (-1: none)  3 co_base  4 ci_base
 *   5 cout  6 cin_real  7 want_bias  8 c_bias  9 index of the convolution whose dw / db it writes  10 db present.
 * quads, quads_mx: RESR_DEBUG_WGRAD_QUAD_FIELDS per quad of the f16 / the MX launch (room for 40 each) -- 0..3 slab_off of the four
 *   slots (-1: unused)  4 bias_mask  5 xsub  6, 7 the X operands  8, 9 the G operands (numbered as in `jobs`, -1: none).
 * Returns RESR_OK, or the status with which wgrad_batch refuses the batch (resr_last_error has the text); the outputs are then undefined. */
#define RESR_DEBUG_WGRAD_CONV_FIELDS 22
#define RESR_DEBUG_WGRAD_TOTALS 11
#define RESR_DEBUG_WGRAD_JOB_FIELDS 9
#define RESR_DEBUG_WGRAD_REDUCE_FIELDS 11
#define RESR_DEBUG_WGRAD_QUAD_FIELDS 10
int resr_debug_wgrad_batch_plan(const int32_t* convs, int32_t nconv, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t flags,
                                int32_t splits, int32_t* totals, int32_t* jobs, int32_t* reduce, int32_t* quads, int32_t* quads_mx);
/* Measurement aid (tools/energy.py): the weight-gradient launch pair the generator's backward pass issues per RRDB -- the five
 * convolutions of `nblocks` (1..3) dense blocks, 26 products each, as ONE batched launch -- on caller-made f16 operands.
 * x_ws[b]: chunk-planar [6][n,h,w,32] (conv_k reads the first 2 + (k - 1) planes); g_ws[b]: chunk-planar [6][n,h,w,32] (planes
 * 0,1 = the closing convolution's 64 gradient channels, plane 1 + k = conv_k's 32); dw: nblocks * 26624 * 9 floats;
 * partial: `partial_bytes` of slab scratch (26 * nblocks * splits slabs of kSlab floats: csrc/wgrad.h, wgrad_slab_bytes). */
int resr_debug_wgrad_dense_blocks(int32_t nblocks, const void* const* x_ws, const void* const* g_ws, int32_t n, int32_t h, int32_t w,
                                  int32_t splits, float* partial, size_t partial_bytes, float* dw, void* stream);
/* Test entry (tests/test_gpu_sparse_taps.py) of the sparse-tap weight gradient, which the product reaches only from inside the native
 * discriminator passes (csrc/disc_native.hip, the 4x4 / stride-2 layers): resr_conv3x3_wgrad, every argument as there, on an X that is
 * the 2x2 space-to-depth image of x_s2d_c channels per sub-position (sub-position-major: channel sub * x_s2d_c + c).  x_s2d_c: a
 * positive multiple of 32 with d->cin == 4 * x_s2d_c, else RESR_ERR_ARG.  RESR_F16 / RESR_F16X2: an X chunk of sub-position (i, j)
 * contributes only the taps dy in {1,2} (i = 0) / {0,1} (i = 1), dx likewise by j -- the 16 of 36 (tap, sub-position) blocks where
 * the virtual kernel of csrc/pack.hip is non-zero; dw [cout, cin, 3, 3] holds zeros in the other 20 (the quad kernel; where the pair
 * kernel takes a launch -- RESR_WGRAD_PAIR_KERNEL, operands beyond 32-bit offsets -- it computes all taps).  RESR_F32: all taps. */
int resr_debug_conv3x3_wgrad_s2d(const ResrWgradDesc* d, const void* x0, const void* x1, const void* g, float* partial, float* dw,
                                 float* db, int32_t x_s2d_c, void* stream);
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
/* Test entry (tests/test_compact_train_surface.py, tests/test_gpu_compact_train_passes.py): where resr_compact_forward_train and
 * resr_compact_backward keep their tensors in the training workspace of `d` (resr.h, "Compact generator: training"), host only -- no
 * HIP call.  RESR_DEBUG_COMPACT_TRAIN_OFFSETS byte offsets from the workspace's start, in this order:
 *   0 the pre-scale slot   1 x_in [px][32]   2 z_0 [px][64]   3 a_0 [px][64]
 *   4 the byte stride from z_k to z_{k+1}, which is also the stride from a_k to a_{k+1} (k = 0 .. num_conv; no offset)
 *   5 t [N,3 s^2,H,W] fp32   6 g_t [px][cpl]   7 g0   8 g1 (the two ping-pong gradient tensors [px][64])   9 g_xin [px][32]
 * NHWC tensors of the descriptor's dtype.  Returns the count, or RESR_ERR_ARG for a descriptor the training entries refuse (RESR_F16X2
 * included), a null `out` or a capacity below the count. */
#define RESR_DEBUG_COMPACT_TRAIN_OFFSETS 10
int64_t resr_debug_compact_train_offsets(const ResrCompactDesc* d, int64_t* out, int64_t capacity);

/* Test entry (tests/test_generator_pass_ref.py, tests/test_gpu_generator_passes.py): where resr_generator_forward (training = 1) and
 * resr_generator_backward keep their tensors in the workspace of `d` (csrc/generator.hip has the plan), host only -- no HIP call.
 * resr_generator_buffer_offsets (resr.h) names ws[0] and gS[0] alone and neither the sign words nor the pre-scale slot; this entry names
 * all of them.  RESR_DEBUG_GENERATOR_TRAIN_OFFSETS values, byte offsets from the workspace's start unless called a stride, in this order
 * (px = N h w trunk pixels, h, w after the pixel-unshuffle; T = the descriptor's dtype; "planar" = chunk-planar [planes][pixels][32]):
 *    0 the gradient pre-scale slot (three 32-bit words; resr_generator_chain_state_bytes - 256)   1 x_in [px][ci_pad]
 *    2 ws[0], planar [6][px][32]: planes x (2) | o1 | o2 | o3 | o4 of dense block 0   3 the byte stride ws[r] -> ws[r + 1] (r < 3 n_blocks)
 *    4 bits[0]: the sign words of o1..o4 of dense block 0, uint32 [4][px]   5 the byte stride bits[r] -> bits[r + 1]
 *    6 bits_u2, 7 bits_c3: the sign words of u2 and c3, uint32 [16 px][2] (bit c of word m = channel 32 m + c)
 *    8 trunk_out, 9 feat: planar [2][px][32]   10 u1: planar [2][4 px][32]   11 u2, 12 c3: planar [2][16 px][32]
 *   13 ymask: uint8 [N][out_channels][4h][4w]   14 g4 [16 px][32]   15 gA, 16 gB: planar [2][16 px][32]   17 gM1: planar [2][4 px][32]
 *   18 gF: planar [2][px][32]   19 gT[0], planar [2][px][32]   20 the byte stride gT[i] -> gT[i + 1] (the ring's four slots)
 *   21 gS[0]: planar [4][px][32], planes g_o4 | g_o3 | g_o2 | g_o1   22 the byte stride gS[i] -> gS[i + 1] (one slab per dense block of an RRDB)
 *   23 g_xin [px][ci_pad]   24 the weight-gradient slabs (scratch; to the workspace's end)
 * Every offset is a multiple of 256; RESR_F16X2 tensors are followed by their lo (and q) tensors.  Returns the count, or RESR_ERR_ARG
 * for a descriptor the training entries refuse, for training == 0, a null `out` or a capacity below the count. */
#define RESR_DEBUG_GENERATOR_TRAIN_OFFSETS 25
int64_t resr_debug_generator_train_offsets(const ResrGeneratorDesc* d, int64_t* out, int64_t capacity);

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

/* Test entries of the PNG encoder (tests/test_gpu_png_encode.py; csrc/png_encode.hip).
 * resr_png_debug_deflate: the segment, scan and copy kernels of resr_png_encode over a given byte stream on the device (the filter
 *   stage skipped: the stream is F itself), segments of segment_bytes (64..65535).  out receives a bare zlib stream -- 78 01, the
 *   segments' blocks, the Adler-32 -- and *length its size, or the negative of it where out_capacity is too small (nothing written).
 *   workspace: resr_png_debug_deflate_workspace_bytes, 16-byte aligned.  Enqueued on `stream`, no synchronisation.
 * resr_png_debug_build_code: the device's length-limited code construction (one wave) on counts uint32 [nsym] (device memory, 1..286
 *   symbols, their sum below 2^32) with code lengths limited to `limit` (1..15, 2^limit >= nsym) -> lengths uint8 [nsym] (device). */
size_t resr_png_debug_deflate_workspace_bytes(int64_t stream_bytes, int32_t segment_bytes);
int resr_png_debug_deflate(const uint8_t* stream_dev, int64_t stream_bytes, int32_t segment_bytes, uint8_t* out, int64_t out_capacity,
                           int64_t* length, void* workspace, size_t workspace_bytes, void* stream);
int resr_png_debug_build_code(const uint32_t* counts_dev, int32_t nsym, int32_t limit, uint8_t* lengths_dev, void* stream);

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
