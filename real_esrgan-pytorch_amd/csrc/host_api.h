// host_api.h -- the host functions the translation units of libresr_hip.so call each other through, each declared ONCE.
// The rule: a function with external linkage is declared in exactly one header, and every file that defines or calls it includes that
// header -- so the compiler compares every definition and every call with the same declaration (tests/test_csrc_declarations.py keeps it
// so).  Grouped by defining file; the comments at the definitions say what each does.  Elsewhere: err_buf, fail, prof_* in common.h; the
// launchers that take ConvArgs / ChainJob / ChainArgs in conv3x3.h, next to those types (it includes this file; no other file needs the kernel headers).
// Shared parameter names: n, c, h, w tensor geometry; dtype RESR_F32 / RESR_F16 / RESR_F16X2; *lo* / lo_off the element offset hi -> lo
// tensor of a RESR_F16X2 pair (< 0 where the C ABI's default applies: lo right behind hi; ignored for other dtypes).
#pragma once
#include "common.h"
#include "wgrad.h"

namespace resr {
// ---- conv3x3.hip: the descriptor-level entries (include/resr.h).  prelu: per-output-channel slopes; block: njobs growth convolutions
// of a dense block (arrays of njobs) and, with d5, the closing one (the *5 arguments) ----
int conv3x3_dispatch(const ResrConvDesc* d, const void* in0, const void* in1, const void* w, const float* bias, const void* res0, const void* res1, const void* mask, void* out, void* aux,
                     hipStream_t stream);
int conv3x3_dispatch_prelu(const ResrConvDesc* d, const void* in0, const void* w, const float* bias, const float* prelu, void* out, hipStream_t stream);
int conv3x3_block_dispatch(int njobs, const ResrConvDesc* d, const void* in0, const void* in1, const void* const* w, const float* const* bias, const void* const* mask, void* const* out,
                           void* const* aux, const ResrConvDesc* d5, const void* w5, const float* bias5, const void* res0_5, const void* res1_5, void* out5, void* chain_state,
                           size_t chain_state_bytes, hipStream_t stream);
int conv3x3_chain_dispatch(int njobs, const ResrConvDesc* d, const void* in0, const void* in1, const void* const* w, const float* const* bias, const void* const* mask, void* const* out,
                           void* const* aux, void* chain_state, size_t chain_state_bytes, hipStream_t stream);
// ---- conv3x3_ws.hip ----
void conv_trace_set(void* p);   // p: device buffer of per-workgroup time stamps, or null
bool conv3x3_chain_device_ok();   // the current device is a whole MI355X (256 CUs)
long long conv3x3_chain_errors();   // time-outs | beyond-share << 32
size_t conv3x3_chain_state_bytes(int n, int h, int w);
// ---- wgrad.hip.  splits: pixel splits of the launch (one slab of partial sums each); partial: the slab scratch *_partial_bytes sizes;
// flags: RESR_CONV_* of the forward convolution (RESR_CONV_UPSAMPLE_IN) ----
int wgrad_tile_rows(int dtype);
int wgrad_default_splits(int dtype, int jobs, int n, int h, int w);
int wgrad_x2_products();   // tap-products per RESR_F16X2 weight gradient
int wgrad_batch_quads(const WgradConv* convs, int nconv, int dtype);
int wgrad_batch_jobs(const WgradConv* convs, int nconv, int dtype);
size_t wgrad_batch_partial_bytes(const WgradConv* convs, int nconv, int splits, int dtype);
size_t wgrad_layer_partial_bytes(int cin, int cout_pad, int splits, int dtype);
int wgrad_layer(const WgradConv* c, int n, int h, int w, int dtype, int flags, int splits, float* partial, hipStream_t stream);
int wgrad_batch(const WgradConv* convs, int nconv, int n, int h, int w, int dtype, int flags, int splits, float* partial, hipStream_t stream);
size_t wgrad_partial_bytes(const ResrWgradDesc* d);
int wgrad_dispatch(const ResrWgradDesc* d, const void* x0, const void* x1, const void* g, float* partial, float* dw, float* db, hipStream_t stream);
int wgrad_debug_s2d(const ResrWgradDesc* d, const void* x0, const void* x1, const void* g, float* partial, float* dw, float* db, int x_s2d_c, hipStream_t stream);
int wgrad_debug_plan(const int* cin, const int* cout_pad, int nconv, int* out, int max_jobs);
int wgrad_debug_batch_plan(const int* convs, int nconv, int dtype, int n, int h, int w, int flags, int splits, int* totals, int* jobs, int* reduce, int* quads, int* quads_mx);
int wgrad_debug_dense_blocks(int nblocks, const void* const* x, const void* const* g, int n, int h, int w, int splits, float* partial, size_t partial_bytes, float* dw, hipStream_t stream);
// ---- pack.hip ----
int pack_dispatch(const ResrPackChunk* chunks_dev, int n_chunks, const float* arena, void* packed, int dtype, hipStream_t stream);
int pack_mx_dispatch(const ResrPackChunk* chunks_dev, int n_chunks, const float* arena, void* packed_mx, hipStream_t stream);
int ema_dispatch(float* shadow, const float* params, long count, double decay, hipStream_t stream);
// ---- layout.hip.  r: pixel-(un)shuffle factor folded in (1 = none); c_pad / src_stride: channels per pixel of the NHWC tensor; mask: pass-mask
// bytes (the backward of a clamp) or, sumpool2x2, the producer's saved activation (its LeakyReLU backward, `slope`, fused in), or null; amax: device
// pointer to the bits of max |g| (absmax_dispatch; common.h grad_prescale), or null; q_off: != 0 = also write the q tensor at that element offset ----
int absmax_dispatch(const float* src, long count, unsigned* slot, int target_log2, hipStream_t stream);
int nchw_to_nhwc_dispatch(const float* src, void* dst, int n, int c, int h, int w, int r, int c_pad, int dtype, const uint8_t* mask, hipStream_t stream, long lo_off);
int nchw_to_nhwc_scaled_dispatch(const float* src, void* dst, int n, int c, int h, int w, int r, int c_pad, int dtype, const uint8_t* mask, hipStream_t stream, long lo_off,
                                 const unsigned* amax);
int nchw_to_nhwc_q_dispatch(const float* src, void* dst, int n, int c, int h, int w, int r, int c_pad, int dtype, const uint8_t* mask, hipStream_t stream, long lo_off, const unsigned* amax,
                            long q_off);
int nhwc_to_nchw_dispatch(const void* src, float* dst, int n, int c, int h, int w, int r, int src_stride, int dtype, hipStream_t stream, long lo_off);
int nhwc_to_nchw_scaled_dispatch(const void* src, float* dst, int n, int c, int h, int w, int r, int src_stride, int dtype, hipStream_t stream, long lo_off, const unsigned* amax);
int sumpool2x2_dispatch(const void* src, void* dst, const void* mask, int n, int ho, int wo, int c, int dtype, float slope, hipStream_t stream, long src_lo, long dst_lo);
int add_inplace_dispatch(void* dst, const void* src, long count, int dtype, hipStream_t stream, long dst_lo, long src_lo);
// ---- generator.hip.  events, n_events: the grad_ready_events of include/resr.h, or null / 0 ----
size_t generator_param_count(const ResrGeneratorDesc* d);
size_t generator_mx_offset(const ResrGeneratorDesc* d);
size_t generator_packed_bytes(const ResrGeneratorDesc* d, int backward);
size_t generator_chain_state_bytes(const ResrGeneratorDesc* d);
size_t generator_workspace_bytes(const ResrGeneratorDesc* d);
int64_t generator_buffer_offsets(const ResrGeneratorDesc* d, int64_t* out, int64_t cap);
int64_t generator_train_offsets(const ResrGeneratorDesc* d, int64_t* out, int64_t cap);
int64_t generator_pack_table(const ResrGeneratorDesc* d, int backward, ResrPackChunk* out, int64_t cap);
int generator_forward(const ResrGeneratorDesc* d, const float* x, const float* params, const void* packed, void* workspace, size_t workspace_bytes, float* y, hipStream_t st);
int generator_backward(const ResrGeneratorDesc* d, const float* gy, const float* params, const void* packed, void* workspace, size_t workspace_bytes, float* grad, float* gx, hipStream_t st,
                       void* const* events, int n_events);
// ---- compact.hip.  who: the entry's name, for error texts ----
size_t compact_param_count(const ResrCompactDesc* d);
size_t compact_packed_bytes(const ResrCompactDesc* d);
size_t compact_workspace_bytes(const ResrCompactDesc* d);
int64_t compact_pack_table(const ResrCompactDesc* d, ResrPackChunk* out, int64_t cap);
int compact_forward_ends(const ResrCompactDesc* d, const Ends& e, const float* params, const void* packed, void* workspace, size_t workspace_bytes, hipStream_t st, const char* who);
// training (fast / strict): the saved-activation forward and the backward pass; grad: the gradient arena (overwritten); gx: null = not wanted
size_t compact_train_packed_bytes(const ResrCompactDesc* d);
int64_t compact_train_pack_table(const ResrCompactDesc* d, ResrPackChunk* out, int64_t cap);
size_t compact_train_workspace_bytes(const ResrCompactDesc* d);
size_t compact_train_state_bytes(const ResrCompactDesc* d);
int64_t compact_train_offsets(const ResrCompactDesc* d, int64_t* out, int64_t cap);
int compact_forward_train(const ResrCompactDesc* d, const float* x, const float* params, const void* packed, void* workspace, size_t workspace_bytes, float* y, hipStream_t st);
int compact_backward(const ResrCompactDesc* d, const float* gy, const float* params, const void* packed, void* workspace, size_t workspace_bytes, float* grad, float* gx, hipStream_t st);
// ---- compact_train.hip: the element-wise kernels of that pass on [pixels][64] NHWC tensors (RESR_F16 / RESR_F32).  slopes: 64 floats on the
// device (compact_const_slopes: the table of RESR_COMPACT_LRELU / _RELU); dslope: the 64 slope gradients or null; partial: compact_dslope_partial_bytes
// of scratch for them; amax: the pre-scale slot they leave through, or null; residual_bwd: gx [n,3,h,w] += the s x s sums of gy [n,3,hs,ws] ----
const float* compact_const_slopes(int act);
int compact_act_dispatch(const void* z, void* a, const float* slopes, int64_t pixels, int dtype, hipStream_t st);
size_t compact_dslope_partial_bytes(int64_t pixels, int dtype);
int compact_act_bwd_dispatch(const void* g, const void* z, void* gz, const float* slopes, int64_t pixels, int dtype, float* dslope, float* partial, size_t partial_bytes, const unsigned* amax,
                             hipStream_t st);
int compact_residual_bwd_dispatch(const float* gy, float* gx, int n, int h, int w, int s, hipStream_t st);
// ---- frames.hip: the uint8 / YUV 4:2:0 ends of the compact generator.  t: the last convolution's output [n,3s^2,h,w] fp32; x: the source frames
// (the residual); s: upscale factor; q / qs / qd: what the (source / destination) frames are; bits: 8, 10 or 0 (Ends::bits_expected);
// img: the frames are images of that mode (then q is null; uint8 RGB frames are kRgb8), n of the head and of image_forward_check the network's batch
// planes * N, n_images N ----
int frame_head_dispatch(const void* src, void* dst, int n, int h, int w, int dtype, hipStream_t st, long lo_off, const ResrYuvDesc* q, const ResrImageDesc* img);
int u8_to_nchw_dispatch(const uint8_t* src, float* dst, int n, int h, int w, hipStream_t st);
int nchw_to_u8_dispatch(const float* src, uint8_t* dst, int n, int h, int w, hipStream_t st);
int yuv_forward_check(const char* who, int n, int h, int w, int s, const void* y, const ResrYuvDesc* src, const ResrYuvDesc* dst, int bits);
int compact_tail_yuv(const float* t, const void* x, void* y, int n, int h, int w, int s, const ResrYuvDesc* qs, const ResrYuvDesc* qd, hipStream_t st);
int yuv420p10_to_nchw_dispatch(const uint16_t* src, float* dst, int n, int h, int w, const ResrYuvDesc* q, hipStream_t st);
int nchw_to_yuv420p10_dispatch(const float* src, uint16_t* dst, int n, int h, int w, const ResrYuvDesc* q, hipStream_t st);
int yuv420_to_rgb_dispatch(const uint8_t* src, uint8_t* dst, int n, int h, int w, const ResrYuvDesc* q, hipStream_t st);
int rgb_to_yuv420_dispatch(const uint8_t* src, uint8_t* dst, int n, int h, int w, const ResrYuvDesc* q, hipStream_t st);
int image_forward_check(const char* who, int n, int h, int w, int s, const void* x, const void* y, const ResrImageDesc* img);
int compact_tail_image(const float* t, const void* x, void* y, int n_images, int h, int w, int s, const ResrImageDesc* img, hipStream_t st);
int image_to_nchw_dispatch(const void* src, float* dst, int n_images, int h, int w, const ResrImageDesc* img, hipStream_t st);
int nchw_to_image_dispatch(const float* src, void* dst, int n_images, int h, int w, const ResrImageDesc* img, hipStream_t st);
// ---- image_resize.hip.  idx_* / w_*: the resize tables (device), taps_* taps per output row / column; kind: a ResizeOut; c, h, w: the source;
// gp: the launch resize_plan made for the HR frame (c = 3, h * s, w * s) ----
int resize_plan(const char* who, int n, int c, int h, int w, int oh, int ow, const void* idx_y, const void* w_y, int taps_y, const void* idx_x, const void* w_x, int taps_x, int kind,
                const void* y, ResizeGeom* out);
size_t resize_lds_bytes(const ResizeGeom* gp, int kind);   // the dynamic LDS of one workgroup of that launch
int compact_yuv420_scaled_fits(int h, int w, int s, int oh, int ow, int taps_y, int taps_x, int bits);
int image_resize_dispatch(const float* x, void* y, int n, int c, int h, int w, int oh, int ow, const int32_t* idx_y, const float* w_y, int taps_y, const int32_t* idx_x, const float* w_x,
                          int taps_x, int u8, hipStream_t st);   // u8: y is uint8 HWC, else fp32 NCHW
int compact_tail_yuv420_scaled(const float* t, const void* x, void* y, int n, int h, int w, int s, const int32_t* idx_y, const float* w_y, const int32_t* idx_x, const float* w_x,
                               const ResrYuvDesc* qs, const ResrYuvDesc* qd, const ResizeGeom* gp, hipStream_t st);
// the image modes' scaled tail: x, y image batches of n_images images in mode img; image_scaled_plan: its tile without the pointer checks
// (false: a bad argument or none fits), *kind the ResizeOut of the mode
bool image_scaled_plan(int h, int w, int s, int oh, int ow, int taps_y, int taps_x, int channels, int bits, ResizeGeom* out, int* kind);
int compact_tail_image_scaled(const float* t, const void* x, void* y, int n_images, int h, int w, int s, const int32_t* idx_y, const float* w_y, const int32_t* idx_x, const float* w_x,
                              const ResrImageDesc* img, const ResizeGeom* gp, hipStream_t st);
// ---- disc_native.hip.  uv: the spectral-norm arena; table / n_chunks: discriminator_pack_table's, on the device ----
size_t discriminator_param_count();
size_t discriminator_uv_count();
size_t discriminator_workspace_bytes(const ResrDiscriminatorDesc* d);
int64_t discriminator_pack_table(const ResrDiscriminatorDesc* d, const void* workspace, ResrPackChunk* out, int64_t cap);
int discriminator_forward(const ResrDiscriminatorDesc* d, const float* x, const float* params, float* uv, const ResrPackChunk* table, int n_chunks, void* workspace, size_t workspace_bytes,
                          float* y, hipStream_t st);
int discriminator_backward(const ResrDiscriminatorDesc* d, const float* gy, const float* params, void* workspace, size_t workspace_bytes, float* grad, float* gx, hipStream_t st);
int discriminator_backward_f16(const ResrDiscriminatorDesc* d, const float* gy, const float* params, const ResrPackChunk* table, int n_chunks, void* workspace, size_t workspace_bytes,
                               float* grad, float* gx, hipStream_t st);
// ---- disc.hip: the discriminator's / VGG's helper kernels.  mask: a saved activation, its LeakyReLU backward (`slope`) fused in; ho, wo of the
// pools: the output's size; arg: the argmax bytes of resr_maxpool2x2_arg (or null) ----
int d2s_add_mask_dispatch(const void* src, const void* add, const void* mask, void* out, int n, int h, int w, int c, int dtype, float slope, hipStream_t st, long lo_src, long lo_add,
                          long lo_out);
int s2d_dispatch(const void* src, void* dst, int n, int h, int w, int c, int dtype, int inverse, hipStream_t st);
int bilinear_up_bwd_mask_dispatch(const void* g, void* gin, const void* mask, void* gmasked, int n, int h, int w, int c, int dtype, float slope, hipStream_t st, long lo_g, long lo_gin);
int bilinear_up_dispatch(const void* src, void* dst, int n, int h, int w, int c, int dtype, int backward, hipStream_t st, long lo_src, long lo_dst);
int add_mask_dispatch(const void* a, const void* b, const void* mask, void* out, long count, int dtype, float slope, hipStream_t st);
int l1_partial_dispatch(const void* a, const void* b, long count, int dtype, long lo, float* partial, int nblocks, hipStream_t st);
int maxpool2x2_dispatch(const void* src, void* dst, int n, int ho, int wo, int c, int dtype, hipStream_t st, long lo_src, long lo_dst, uint8_t* arg);
int maxpool2x2_bwd_dispatch(const void* g, const uint8_t* arg, void* gin, int n, int ho, int wo, int c, int dtype, hipStream_t st, long lo_g, long lo_gin);
// W [rows, cols]; u [rows], v [cols] updated in place; sigma2: [sigma, 1 / sigma]; the batch forms take n of each
int spectral_norm_dispatch(const float* W, float* u, float* v, int rows, int cols, int training, float eps, float* sigma2, float* tmp, hipStream_t st);
int spectral_norm_batch_dispatch(int n, const float* const* W, float* const* u, float* const* v, const int* rows, const int* cols, int training, float eps, float* const* sigma2,
                                 float* const* tmp, hipStream_t st);
int spectral_norm_bwd_dispatch(const float* G, const float* W, const float* u, const float* v, const float* sigma2, float* dst, int rows, int cols, int accumulate, float* tmp1,
                               hipStream_t st);
int spectral_norm_bwd_batch_dispatch(int n, const float* const* G, const float* const* W, const float* const* u, const float* const* v, const float* const* sigma2, float* const* dst,
                                     const int* rows, const int* cols, float* dot, hipStream_t st);
// dw3 [cout, 4C, 3, 3], the gradient of the virtual 3x3 kernel over the space-to-depth image -> dw4 [cout, C, 4, 4]
int fold4x4_dispatch(const float* dw3, float* dw4, int cout, int C, hipStream_t st);
int fold4x4_batch_dispatch(int n, const float* const* src, float* const* dst, const int* cout, const int* C, hipStream_t st);
// ---- degrade.hip: the fp32 degradation pipeline.  per_sample: one kernel per image, else one for all ----
int filter2d_dispatch(const float* src, float* dst, const float* kern, int n, int c, int h, int w, int kh, int kw, int per_sample, hipStream_t st);
int usm_dispatch(const float* src, float* dst, float* tmp, const float* k1d, int ksize, float weight, float threshold, int n, int c, int h, int w, hipStream_t st, int keep_for_backward);
int usm_bwd_dispatch(const float* x, const float* saved, const float* g, float* gx, float* tmp2, const float* k1d, int ksize, float weight, int n, int c, int h, int w, hipStream_t st);
int resize_dispatch(const float* src, float* dst, int n, int c, int h, int w, int oh, int ow, int mode, double scale_h, double scale_w, hipStream_t st);
int randn_dispatch(float* dst, long count, uint64_t seed, uint64_t stream, hipStream_t st);   // stream: which sequence of `seed`; st: the HIP stream
int gauss_noise_dispatch(const float* src, float* dst, const float* sigma, const float* gray, const float* fg, const float* fc, int n, int c, int h, int w, int clip, hipStream_t st);
int poisson_noise_dispatch(const float* src, float* dst, const float* scale, const float* gray, uint64_t seed, void* workspace, int n, int c, int h, int w, int clip, hipStream_t st);
int jpeg_dispatch(const float* src, float* dst, const float* quality, float* coeffs, int n, int h, int w, int flags, hipStream_t st);
int quantize_crop_dispatch(const float* lr, const float* hr, float* lr_out, float* hr_out, int n, int c, int lr_h, int lr_w, int hr_h, int hr_w, int hr_size, int upscale, int hr_top,
                           int hr_left, hipStream_t st);
// ---- degrade_int.hip: its bit-exact uint8 twin ----
int filter2d_u8_dispatch(const uint8_t* src, uint8_t* dst, const int32_t* taps, int n, int c, int h, int w, int kh, int kw, int per_sample, hipStream_t st);
int resize_u8_dispatch(const uint8_t* src, uint8_t* dst, int n, int c, int h, int w, int oh, int ow, int mode, const int32_t* idx_y, const int32_t* w_y, const int32_t* idx_x,
                       const int32_t* w_x, hipStream_t st);
int jpeg_u8_dispatch(const uint8_t* src, uint8_t* dst, const float* quality, int32_t* coeffs, int n, int h, int w, hipStream_t st);
// ---- data_source.hip: a batch of the device-resident training set.  tiles [M,T,T,3] bytes, index / aug [B] on the device; params n records ----
int tile_batch_dispatch(const uint8_t* tiles, const int32_t* index, const uint8_t* aug, int M, int B, int T, float* dst, hipStream_t st);
int blur_kernels_dispatch(const double* params, int n, int K, float* dst, hipStream_t st);
// a batch of LR / HR pairs: both arenas bytes, table [M,4] int64 (hr_offset, lr_offset, lr_h, lr_w), records [B,4] int32 (image, top, left, code)
int pair_batch_dispatch(const uint8_t* hr_arena, const uint8_t* lr_arena, const int64_t* table, const int32_t* records, int M, int B, int P, int scale,
                        float* lr_dst, float* hr_dst, hipStream_t st);
// a batch of windows of whole images: arena bytes, table [M,3] int64 (offset, h, w), records [B,4] int32 (image, top, left, code)
int crop_batch_dispatch(const uint8_t* arena, const int64_t* table, const int32_t* records, int M, int B, int T, float* dst, hipStream_t st);
// the training pair pool: pools [Q, *_elems], batches [B, *_elems] fp32, slots [B] int32 on the device; both outputs null = store only
int pool_exchange_dispatch(float* pool_lr, float* pool_hr, const float* lr_in, const float* hr_in, float* lr_out, float* hr_out, const int32_t* slots, int Q,
                           int B, int64_t lr_elems, int64_t hr_elems, hipStream_t st);
// ---- resample_u8.hip: the multi-scale copies of the whole-image source.  Tables: bounds [out,2] (xmin, count), coeffs [out,ksize_capacity] Q22 (host
// memory, no GPU call); jobs [J,8] int64 (src offset, h, w, dst offset, oh, ow, row table, column table), on the host for the checks and on the device ----
int resample_ksize(int64_t in_size, int64_t out_size);
int resample_tables(int64_t in_size, int64_t out_size, int32_t* bounds, int32_t* coeffs, int ksize_capacity);
int resample_u8_dispatch(uint8_t* arena, int64_t arena_bytes, const int64_t* jobs_host, const int64_t* jobs_dev, int J, const int32_t* tables, int64_t table_words,
                         hipStream_t st);
// ---- niqe.hip: the native NIQE stages (include/resr.h).  u8: src is uint8 [n,h,w,3], else fp32 [n,3,h,w] ----
int niqe_luma_dispatch(const void* src, int u8, uint8_t* dst, int n, int h, int w, int crop, int oh, int ow, hipStream_t st);
size_t niqe_workspace_bytes(const ResrNiqeDesc* d);
int niqe_features_dispatch(const ResrNiqeDesc* d, const uint8_t* luma, double* feats, hipStream_t st);
size_t niqe_score_workspace_bytes(const ResrNiqeScoreDesc* d);
int niqe_score_dispatch(const ResrNiqeScoreDesc* d, const double* feats, double* scores, hipStream_t st);
// ---- fullref.hip: PSNR / SSIM of sr against hr (include/resr.h) ----
size_t fullref_workspace_bytes(const ResrFullRefDesc* d);
int fullref_dispatch(const ResrFullRefDesc* d, const void* sr, const void* hr, int64_t* sse, double* psnr, double* ssim, hipStream_t st);
size_t fullref_planes_workspace_bytes(const ResrFullRefPlanesDesc* d);
int fullref_planes_dispatch(const ResrFullRefPlanesDesc* d, const void* sr, const void* hr, int64_t* sse, double* psnr, double* ssim, hipStream_t st);
// ---- jpeg_encode.hip: baseline JPEG files written on the device (include/resr.h) ----
size_t jpeg_encode_max_bytes(const ResrJpegEncDesc* d);
size_t jpeg_encode_workspace_bytes(const ResrJpegEncDesc* d);
int jpeg_encode_header(const ResrJpegEncDesc* d, uint8_t* host_buf, size_t cap);
int jpeg_encode_dispatch(const ResrJpegEncDesc* d, const uint8_t* rgb, uint8_t* out, int64_t out_stride, int64_t* lengths, const uint8_t* header_dev, int header_len, void* workspace,
                         size_t workspace_bytes, hipStream_t st);
// ---- png_encode.hip: PNG files written on the device (include/resr.h), and its test entries (include/resr_debug.h) ----
size_t png_encode_max_bytes(const ResrPngEncDesc* d);
size_t png_encode_workspace_bytes(const ResrPngEncDesc* d);
int png_encode_header(const ResrPngEncDesc* d, uint8_t* host_buf, size_t cap);
int png_encode_dispatch(const ResrPngEncDesc* d, const void* src, uint8_t* out, int64_t out_stride, int64_t* lengths, const uint8_t* header_dev, int header_len, void* workspace,
                        size_t workspace_bytes, hipStream_t st);
size_t png_debug_deflate_workspace_bytes(int64_t stream_bytes, int segment_bytes);
int png_debug_deflate(const uint8_t* stream_dev, int64_t stream_bytes, int segment_bytes, uint8_t* out, int64_t out_capacity, int64_t* length, void* workspace, size_t workspace_bytes,
                      hipStream_t st);
int png_debug_build_code(const uint32_t* counts_dev, int nsym, int limit, uint8_t* lengths_dev, hipStream_t st);
// ---- loss.hip. loss, grad: outputs (grad may be null) ----
int bce_logits_const_dispatch(const float* x, long count, float label, float weight, float* loss, float* grad, float* scratch, hipStream_t st);
int l1_mean_dispatch(const float* a, const float* b, long count, float weight, float* loss, float* grad, float* scratch, hipStream_t st);
int weighted_rows_dispatch(const float* partial, int rows, int cols, const float* coef, float* out, hipStream_t st);
// ---- sustained.hip ----
int sustained_run(int mode, double seconds, const void* src, size_t bytes, void* counter, double* tbs, double* pflops, hipStream_t st);

}  // namespace resr
