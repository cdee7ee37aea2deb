/*
 * resr.h -- C-ABI of libresr_hip.so: the MI355X (gfx950) Real-ESRGAN hot path.
 *
 * The reference (Lornatang/Real_ESRGAN-PyTorch) has no FFI: its device arithmetic is stock
 * PyTorch op call sites.  Each entry point below names the reference call site(s) it replaces
 * (file:line relative to the reference root).  All pointers are raw device pointers owned by the
 * caller (PyTorch's caching allocator); the library never allocates, frees or retains device
 * memory, never synchronises the stream or the device, and is graph-capture safe (chained dense-block launches inside a
 * captured graph: see resr_conv3x3_chain).  Test / measurement aids (resr_debug_*, resr_profile_*) are exported too but are NOT
 * part of this contract: they are declared in resr_debug.h.  What a launch needs beyond its operands -- scratch, slabs, the progress flags of the chained
 * dense-block launches -- is part of a workspace the caller passes in.  Every call enqueues on the
 * given hipStream_t (passed as void*) of the current device and returns 0 or a negative
 * resr_status; resr_last_error() returns a thread-local message.  No C++ exception crosses.
 *
 * Layouts.  Activations: NHWC ("pixel-major"), element type f16 (fast mode) or f32 (strict mode),
 * channels padded to a multiple of 32, addressed as base + pixel * pixel_stride + channel; a conv
 * reads a channel *prefix* of one or two such tensors, which is how the dense-block concat of
 * model.py:91-94 is served without materialising it.  Weights: packed MFMA A-fragments made by
 * resr_pack_weights from the module's OIHW fp32 parameters.
 */
#ifndef RESR_H_
#define RESR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: ResrWgradDesc gained x_chunk_stride / g_chunk_stride (round 4), ResrConvDesc.reserved_ became x2_pair_chunks and the struct gained mask_lo_offset,
 * ResrGeneratorDesc gained x2_plan.  A caller built against an older header passes shorter structs: compare resr_version() with the RESR_VERSION it was
 * compiled with and refuse on a mismatch.  New fields are appended (or replace reserved ones) and mean "as before" when zero, so
 * zero-initialise every descriptor (memset / = {0}) before filling it. */
/* 3 (round 6): ResrConvDesc gained in0_q_offset / in1_q_offset / out_q_offset / w_mx_offset (RESR_CONV_MX_PAIRS), ChainJob-level
 * counterparts follow from the per-job descriptors; resr_pack_weights_mx; RESR_X2_PLAN_MX_INFER. */
#define RESR_VERSION 3

typedef enum {
    RESR_OK = 0,
    RESR_ERR_ARG = -1,      /* bad descriptor / unsupported shape */
    RESR_ERR_LAUNCH = -2,   /* hipLaunchKernel failed */
    RESR_ERR_WORKSPACE = -3 /* workspace too small */
} resr_status;

/* RESR_F16X2 ("exact16" mode): every activation tensor is a PAIR of f16 tensors of identical shape and strides,
 *   value = hi + lo * 2^-12,   hi = f16(value),   lo = f16((value - hi) * 2^12)
 * (about 22 significand bits, the scaled lo keeps clear of the f16 subnormal range), addressed as `ptr` (hi) and
 * `ptr + *_lo_offset` elements (lo).  Packed weights hold three f16 blocks per 32-channel chunk -- f16(w*2^12),
 * its remainder, and f16(w) -- and a conv pass runs three v_mfma_f32_32x32x16_f16 per product into one fp32
 * accumulator (x_hi*W0 + x_hi*W1 + x_lo*W2, descaled by 2^-12 in the epilogue): fp32-class results on the f16
 * matrix pipe (the x_lo*w_lo term, 2^-22 relative, is dropped).  |w| must stay below 16. */
typedef enum { RESR_F16 = 0, RESR_F32 = 1, RESR_F16X2 = 2 } resr_dtype;

/* epilogue / gather flags of resr_conv3x3 */
enum {
    RESR_CONV_LRELU = 1 << 0,        /* v = v > 0 ? v : slope*v              (model.py:81,90-93,237,242,248) */
    RESR_CONV_UPSAMPLE_IN = 1 << 1,  /* input is nearest-upsampled x2 on load (model.py:264-265)            */
    RESR_CONV_CLAMP01 = 1 << 2,      /* v = min(max(v,0),1)                   (model.py:270)                */
    RESR_CONV_OUT_NCHW_F32 = 1 << 3, /* write planar fp32 [N,cout,H,W] (+ pass-mask bytes to aux)           */
    RESR_CONV_MASK = 1 << 4,         /* v *= (mask[p,c] > 0 ? 1 : slope): LeakyReLU backward (RESR_F16X2: mask_lo_offset) */
    RESR_CONV_NO_BIAS = 1 << 5,
    RESR_CONV_AUX_BEFORE_MASK = 1 << 6, /* aux_out (NHWC, out_stride) also receives v after bias, before the mask     */
    RESR_CONV_AUX_BEFORE_RES = 1 << 7,  /* aux_out (NHWC, out_stride) also receives v after LeakyReLU, before residuals */
    /* 1-bit LeakyReLU masks.  A sign tensor is uint32 [pixels][cout_pad/32]: bit c of word (p, m) = (out[p, 32m+c] > 0)
     * for the value as stored.  A forward pass can emit it (aux_out; no mask / residuals / other aux use in the same
     * pass); the matching backward-data pass reads it instead of re-reading the saved activation (64 B -> 4 B per
     * pixel and 32 channels in f16).  MASK_BITS goes together with RESR_CONV_MASK, without residuals. */
    RESR_CONV_WRITE_SIGNBITS = 1 << 8,
    RESR_CONV_MASK_BITS = 1 << 9,
    /* RESR_F16X2 only: the output is stored as ONE f16 tensor (the hi tensor; no lo tensor is written and out_lo_offset is
     * ignored).  A later pass reads such a tensor as a "single" chunk (x2_pair_chunks).  Ignored for other dtypes. */
    RESR_CONV_OUT_SINGLE = 1 << 10,
    /* RESR_F16X2 with x2_pair_chunks: the single chunks meet the f16 weights W0 alone -- ONE stage (x W0) instead of two (x W0 + x W1).
     * For operands that are the small ones of the sum (the growth planes of an inference forward next to the residual stream: forward
     * 1.4-2.1e-6 instead of 1.0-1.4e-6 at the reference's init, 2.4-2.9e-5 instead of 1.6-2.9e-5 with the dense weights x 4). */
    RESR_CONV_SINGLE_W16 = 1 << 11,
    /* RESR_F16X2 only: the PAIR chunks take TWO stages instead of three -- the main product x_hi W0 on the f16 matrix pipe, and BOTH
     * 2^-12-weighted corrections (x_hi W1 + x_lo W2) as ONE stage of nine v_mfma_scale_f32_32x32x64_f8f6f4 per output row on 8-bit
     * operands: B = the pixel's "q record" [bf8(x_hi) x 32 | bf8(x_lo) x 32] (64 B per pixel and chunk, K = 64 per tap), A = the
     * packed block [bf8(W1) | bf8(W2)] of resr_pack_weights_mx, unit scales (bf8 = e5m2 has f16's exponent range; the remainders
     * are stored times 2^12).  Every pair operand then needs its q tensor (in0_q_offset / in1_q_offset), the weights their MX blocks
     * (w_mx_offset); out_q_offset != 0 makes a pass EMIT the q tensor of its (pair) output for the passes behind it.  The
     * corrections need ~4 good bits, not 11: forward 0.8-1.2e-4 of the fp32 result over 23 blocks, 2/3 of the
     * matrix time of a pair chunk.  Inference epilogues only (bias / LeakyReLU / residuals) -- and, with MX_SIGNBITS, the sign words. */
    RESR_CONV_MX_PAIRS = 1 << 12,
    /* with MX_PAIRS: the pass may also WRITE_SIGNBITS (the training forward of RESR_X2_PLAN_MX_TRAIN_FORWARD: LeakyReLU with
     * 0 <= slope <= 1, no residuals, pair or single-f16 output).  Bit c of a sign word is taken from the fp32 value the stored
     * output is rounded from.  MX_PAIRS | WRITE_SIGNBITS without this flag is an argument error; the flag alone changes nothing. */
    RESR_CONV_MX_SIGNBITS = 1 << 13
};

/* One 3x3, stride 1, pad 1 convolution pass (forward conv or backward-data conv):
 *   v = sum_{tap,c} W[co][c][tap] * in[p + tap][c] + bias[co]
 *   v = mask / lrelu / (v*s0 + t0*res0[p,co]) / (v*s1 + t1*res1[p,co]) / clamp, in that order.
 * Replaces the F.conv2d + leaky_relu + torch.cat + mul/add call sites of model.py:87-98,
 * 123-132, 255-272 and their autograd backward-data counterparts. */
typedef struct {
    int32_t n, h, w;         /* output batch / height / width (input is h/2 x w/2 when UPSAMPLE_IN) */
    int32_t cin;             /* input channels, multiple of 32                                        */
    int32_t cin0;            /* channels [0,cin0) come from in0, [cin0,cin) from in1; multiple of 32  */
    int32_t in0_stride;      /* pixel strides in elements                                             */
    int32_t in1_stride;
    int32_t cout;            /* real output channels (<= cout_pad)                                    */
    int32_t cout_pad;        /* 32 or 64: rows of the packed weight tile                              */
    int32_t out_stride;      /* NHWC pixel stride of out (ignored for OUT_NCHW_F32)                   */
    int32_t res0_stride, res1_stride, mask_stride;
    int32_t dtype;           /* resr_dtype of activations and packed weights                          */
    int32_t flags;
    float s0, t0, s1, t1, slope;
    /* Chunk strides, in elements: distance between consecutive 32-channel chunks of an operand.  0 means 32, i.e. the
     * chunks of a pixel are interleaved (plain NHWC).  A chunk-planar tensor [C/32][N,H,W,32] has pixel stride 32 and
     * chunk stride N*H*W*32: every 64-byte (f16) piece a pass touches is then contiguous with its x-neighbours, so
     * HBM lines are consumed whole (the generator keeps its dense-block workspaces this way). */
    int32_t in0_chunk_stride, in1_chunk_stride, out_chunk_stride;
    int32_t res0_chunk_stride, res1_chunk_stride, mask_chunk_stride;
    /* RESR_F16X2 only: element offset from the hi tensor of an operand to its lo tensor (a mask given as an f16
     * activation: mask_lo_offset below; the aux tensor of AUX_BEFORE_* uses out's offset). */
    int64_t in0_lo_offset, in1_lo_offset, out_lo_offset, res0_lo_offset, res1_lo_offset;
    /* 4x4 / stride-2 convolutions (model.py:140-152) run as 3x3 convolutions over the 2x2 space-to-depth image with the
     * "virtual" kernel of ResrPackChunk.virtual4x4; 20 of its 36 (tap, sub-position) blocks are zero.  These two hints let
     * the kernel skip them (results are identical with or without; honoured for f16 / f16x2, 64-channel output groups and a
     * plain epilogue):  s2d_in_channels = C > 0: the input is the space-to-depth image, C channels per sub-position (cin = 4C,
     * forward pass);  s2d_out_channels = C > 0: the OUTPUT (all cout_groups * 64 = 4C channels of it) is the gradient of
     * such an image (backward-data pass).  0 = dense.
     * cout_groups = G > 1: ONE launch computes G consecutive 64-channel output groups of a convolution (f16 / f16x2, cout =
     * cout_pad = 64 per group, no bias, NHWC output): group g uses the packed weights at w_packed + g * (cin/32)*9*2*1024
     * elements (how resr_pack_weights lays out consecutive 64-row chunks tables) and writes / reads out, res0, res1, mask,
     * aux 64*g channels further inside the pixel.  The discriminator's 128..512-channel layers at 32^2..128^2 pixels
     * fill the 256 CUs only this way. */
    int32_t s2d_in_channels, s2d_out_channels, cout_groups;
    /* RESR_F16X2 only: P > 0 = only the FIRST P 32-channel input chunks are hi/lo pairs (three stages each: x_hi W0 + x_hi W1 +
     * x_lo W2); the chunks behind them are single f16 tensors -- no lo tensor is read, two stages each (x W0 + x W1: the weights
     * stay split, the activation carries 11 bits).  0 = every chunk is a pair.  The dense blocks use P = 2: the residual stream
     * (x0 x1 / g_y) as pairs, the growth planes (o1..o4 at inference, their gradients in backward) as single f16 -- the rungs of
     * DESIGN section 2 that keep the 1e-3 gate at 50 instead of 60 stages per block. */
    int32_t x2_pair_chunks;
    /* RESR_F16X2, RESR_CONV_MASK without _BITS: element offset from the mask's hi tensor to its lo tensor when the saved activation
     * is a pair of out's layout.  hi decides; the lo half is read only where hi rounded to zero (|value| < 2^-25: below f16's
     * subnormals), so that a LeakyReLU mask survives activations of any scale.  0 = the hi tensor alone (such values count as
     * "not positive"; the mask may then be any f16 tensor, e.g. a view of a larger batch). */
    int32_t reserved2_;
    int64_t mask_lo_offset;
    /* RESR_F16X2, RESR_CONV_MX_PAIRS (version 3): ELEMENT offsets (2 bytes each, like the lo offsets) from the hi tensor of a pair
     * operand to its q tensor -- same pixel / chunk strides as the hi tensor, 64 bytes per pixel and 32-channel chunk: byte c = bf8
     * (e5m2, round to nearest even) of hi[c], byte 32 + c = bf8 of lo[c].  out_q_offset != 0 (any pass with a pair output and a lean
     * epilogue): also write out's q tensor.  w_mx_offset: BYTE offset from w_packed to this convolution's MX blocks, one block of
     * 9 x cout_pad x 64 bytes per 32-channel input chunk in chunk order (resr_pack_weights_mx). */
    int64_t in0_q_offset, in1_q_offset, out_q_offset, w_mx_offset;
} ResrConvDesc;

int resr_conv3x3(const ResrConvDesc* d, const void* in0, const void* in1, const void* w_packed,
                 const float* bias, const void* res0, const void* res1, const void* mask,
                 void* out, void* aux_out, void* stream);

/* The growth convolutions of one dense block in ONE call (model.py:90-93: out_k = leaky_relu(conv_k(cat(x, out_1 ..
 * out_{k-1})))), or their mirrored backward-data passes: njobs (2..4) descriptors as for resr_conv3x3, all reading the
 * SAME in0 [/ in1] tensors -- job j the first descs[j].cin channels of them -- each with its own packed weights, bias (or
 * NULL), sign-word mask (or NULL), output and aux_out (or NULL); job j's output must be the tensor that job j+1 reads as
 * its last 32 channels.  Same results as njobs calls of resr_conv3x3 (to which it falls back); where the fast-mode kernel
 * supports it (f16 or f16x2, cout 32, chunk-planar operands, batch a multiple of 8, even width, LeakyReLU [+ sign words] or
 * the sign-word mask) the jobs run as one persistent launch that orders them through per-tile flags instead of kernel
 * boundaries.  bias / mask / aux_out may be NULL pointers to mean "no job has one".
 * chain_state: resr_conv3x3_chain_state_bytes(n, h, w) bytes of device memory OWNED BY THE CALLER (16-byte aligned), filled
 * with zeros once before its first use and then left alone: epoch, per-XCD tickets, per-tile flags and error words of the
 * chained launches live there (nothing is allocated, reset or synchronised by the library; consecutive launches on one
 * stream may share it, launches that can overlap in time must not).  NULL / too small: one launch per job.
 * A chained launch spins on its own workgroups, so only one runs at a time per device: a call from another stream first makes
 * that stream wait (hipStreamWaitEvent) for the previous chain.  A flag poll that gives up (~4 s: a lost workgroup) is never
 * silent -- the plane it waited for is read as NaNs, so the output (and a training loss) turns NaN, and resr_chain_errors()
 * counts it.
 * Under stream capture the call neither waits for, records, nor takes ownership of anything (none of it would mean anything at
 * replay time): inside one graph the chained launches are ordered by the capture itself, and the CALLER guarantees that a graph
 * holding chained launches is not replayed while another stream runs chained launches on the same device. */
size_t resr_conv3x3_chain_state_bytes(int32_t n, int32_t h, int32_t w);
int resr_conv3x3_chain(int32_t njobs, const ResrConvDesc* descs, const void* in0, const void* in1,
                       const void* const* packed_w, const float* const* bias, const void* const* mask,
                       void* const* out, void* const* aux_out, void* chain_state, size_t chain_state_bytes, void* stream);
/* Health of the chained launches on the current device: low 32 bits = flag polls that gave up, high 32 bits = workgroups an
 * XCD received beyond its share of the grid (tile ownership follows the XCD a workgroup really runs on and assumes the
 * dispatcher deals every XCD grid / 8 workgroups).  Both must be 0.  Reads two host-mapped words the kernels add to: no
 * synchronisation, cheap enough to call every few steps; it reflects the launches that have finished by then. */
int64_t resr_chain_errors(void);

/* Weight-gradient of the same convolution: dW[co][ci][tap] = sum_p G[p][co] * X[p + tap][ci]
 * (autograd backward of F.conv2d wrt weight, all conv call sites of model.py) and
 * db[co] = sum_p G[p][co].  Two launches: partial sums over pixel splits into `partial`
 * (fp32, resr_wgrad_partial_bytes), then a deterministic reduce that writes dW (OIHW fp32,
 * scaled by `scale`) and db.  cout_pad is 32 or 64 -- or, for RESR_F16 / RESR_F16X2, any multiple of 32: a convolution of
 * more than 80 (32-channel chunk x 32-channel tile) products (RESR_F16X2: more than 96 tap-products) runs as ONE "layer mode"
 * launch pair whose jobs follow from their grid position instead of a job table (the discriminator's 256..512-channel
 * layers, model.py:140-160). */
typedef struct {
    int32_t n, h, w;
    int32_t cin, cin0, in0_stride, in1_stride; /* X operand, same addressing as ResrConvDesc: cin0 < cin = channels [cin0, cin) come
                                                * from x1 (job-table launches only, not layer mode; RESR_F16X2: x1's lo tensor lies
                                                * x_lo_offset behind it too)                       */
    int32_t cin_real;                          /* rows of dW actually written (<= cin)            */
    int32_t cout, cout_pad, g_stride;          /* G operand: channels [0,cout_pad) of g           */
    int32_t dtype, flags;                      /* RESR_CONV_UPSAMPLE_IN honoured for X; RESR_CONV_OUT_SINGLE: G is a single f16 tensor */
    int32_t splits;                            /* pixel splits (partial slabs)                    */
    float scale;
    int64_t x_lo_offset, g_lo_offset;          /* RESR_F16X2: hi -> lo element offsets of X and G (both required).  A G that a
                                                * pass stored as ONE f16 tensor is selected explicitly by RESR_CONV_OUT_SINGLE in
                                                * flags (g_lo_offset is then ignored): dW = X_hi^T G + 2^-12 X_lo^T G; a zero
                                                * g_lo_offset without the flag is an argument error (version 3)                 */
    /* elements between consecutive 32-channel chunks of X / G (0 = 32: interleaved NHWC; a chunk-planar tensor
     * [C/32][N,H,W,32] has pixel stride 32 and chunk stride N*H*W*32 -- how the generator keeps its dense-block workspaces) */
    int64_t x_chunk_stride, g_chunk_stride;
} ResrWgradDesc;

size_t resr_wgrad_partial_bytes(const ResrWgradDesc* d);
int resr_conv3x3_wgrad(const ResrWgradDesc* d, const void* x0, const void* x1, const void* g,
                       float* partial, float* dw, float* db, void* stream);

/* Weight packing: a table of chunk descriptors turns the flat fp32 OIHW parameter arena into
 * MFMA A-fragment order (forward) or its transposed+flipped form (backward-data). */
typedef struct {
    int64_t src_off;     /* element offset of the source conv weight in the fp32 arena            */
    int64_t dst_off;     /* element offset of this chunk in the packed buffer                     */
    int32_t src_cout, src_cin;
    int32_t m_off, m_count; /* first row / number of real rows (rest zero) of this chunk's M      */
    int32_t k_off, k_count; /* first / number of real K channels of this chunk (<= 32)            */
    int32_t mt;          /* M tiles (1 or 2)                                                      */
    int32_t transposed;  /* 0: M = cout, K = cin;  1: M = cin, K = cout, taps flipped             */
    float scale;
    int32_t virtual4x4;  /* 1: source is a [cout][C=src_cin][4][4] stride-2 kernel seen as a 3x3 kernel
                            over the 2x2 space-to-depth image (4C virtual channels, (i*2+j)*C + c)       */
    const float* scale_ptr; /* optional device scalar multiplied in (1/sigma of spectral norm)           */
} ResrPackChunk;

int resr_pack_weights(const ResrPackChunk* chunks_dev, int32_t n_chunks, const float* arena,
                      void* packed, int32_t dtype, void* stream);
/* The MX blocks of RESR_CONV_MX_PAIRS from the SAME chunk table: chunk i becomes one block of 9 x (32 mt) x 64 bytes at
 * packed_mx + 2 * dst_off bytes (dst_off counts elements of the plain f16 layout, so the MX region mirrors a plain f16 packing byte for
 * byte): per tap and output row the bytes [bf8(W1[k]), k = 0..31 | bf8(W2[k])] of the exact16 split of resr_pack_weights (W0 =
 * f16(w 2^12), W1 = f16(w 2^12 - W0), W2 = f16(W0 2^-12)), in the A-fragment order of v_mfma_scale_f32_32x32x64_f8f6f4 (lane (row,
 * half h): K = 16 h .. 16 h + 15 of either block). */
int resr_pack_weights_mx(const ResrPackChunk* chunks_dev, int32_t n_chunks, const float* arena, void* packed_mx, void* stream);
/* Host helpers (no GPU needed) for a caller that packs convolutions of its own; the format itself is stated once, in csrc/packed_layout.h.
 * resr_conv_pack_table: the chunk table of ONE OIHW 3x3 convolution [cout][cin][3][3] at arena element offset src_off, in the forward
 *   (transposed = 0) or the backward-data orientation (1), packed from element dst_off on: output rows in groups of at most 64, each
 *   group holding its 32-channel input chunks.  A group starts at each chunk with k_off == 0; its dst_off and mt are what a launch of
 *   that group takes.  Returns the chunk count (`chunks` may be NULL to ask for it) or RESR_ERR_ARG.
 * resr_conv_packed_elems: the elements that table takes in the packed buffer (the same in both orientations): the next table's dst_off.
 * resr_packed_bytes: bytes of a packed buffer of `elems` elements of the plain layout in `dtype`, the slack the kernels' prefetch needs
 *   included.  resr_packed_mx_offset: byte offset of the MX region (resr_pack_weights_mx) behind an RESR_F16X2 packing of `elems`. */
int64_t resr_conv_pack_table(int32_t cout, int32_t cin, int32_t transposed, int64_t src_off, int64_t dst_off, float scale,
                             ResrPackChunk* chunks, int64_t capacity);
int64_t resr_conv_packed_elems(int32_t cout, int32_t cin);
size_t resr_packed_bytes(int64_t elems, int32_t dtype);
size_t resr_packed_mx_offset(int64_t elems);

/* Layout helpers around the generator (model.py:257 PixelUnshuffle, NCHW fp32 module surface). */
int resr_nchw_to_nhwc(const float* src, void* dst, int32_t n, int32_t c, int32_t h, int32_t w,
                      int32_t unshuffle, int32_t c_pad, int32_t dtype, const uint8_t* mask,
                      void* stream);
int resr_nhwc_to_nchw(const void* src, float* dst, int32_t n, int32_t c, int32_t h, int32_t w,
                      int32_t shuffle, int32_t src_stride, int32_t dtype, void* stream);
/* backward of nearest x2 upsample (+ optional LeakyReLU mask of the producer's output) */
int resr_sumpool2x2(const void* src, void* dst, const void* mask, int32_t n, int32_t h_out,
                    int32_t w_out, int32_t c, int32_t dtype, float slope, void* stream);

/* Whole-generator passes (model.py:255-272 and its autograd backward), enqueued natively so the
 * ~350 / ~1100 launches cost no Python time.  See real_esrgan-pytorch_amd/csrc/generator.hip. */
typedef struct {
    int32_t n, h, w;          /* input batch / height / width (before pixel-unshuffle)           */
    int32_t in_channels, out_channels, upscale; /* Generator(in, out, upscale) ctor args          */
    int32_t n_blocks;         /* RRDB count (23)                                                  */
    int32_t dtype;            /* RESR_F16 fast / RESR_F32 strict                                  */
    int32_t training;         /* keep activations for backward                                    */
    int32_t wgrad_splits;     /* 0 = auto                                                         */
    /* RESR_F16X2 only, bit set of RESR_X2_PLAN_*: which tensors of the dense blocks are single f16 instead of hi/lo pairs.  0 =
     * pairs everywhere (three stages per chunk in every pass: forward 1.8e-6, gradients 5.8e-6 vs float64). */
    int32_t x2_plan;
    int32_t reserved_;
} ResrGeneratorDesc;
/* Prerequisites of the x2_plan bits.  With dtype RESR_F16X2 a plan that breaks one is refused by every call that takes the descriptor,
 * whatever `training` says: the size queries return 0, resr_generator_forward / _backward / _pack_table / _buffer_offsets RESR_ERR_ARG, and
 * resr_last_error() names the rule.  Other dtypes ignore the field.
 *      bit                                needs
 *      GROWTH_GRAD_STORE_F16 (4)          GROWTH_GRAD_F16 (2)
 *      GROWTH_ACT_G_HI_WGRAD (16)         GROWTH_ACT_F16_WGRAD (8)
 *      GROWTH_W16_INFER (32)              GROWTH_F16_INFER (1)
 *      MX_INFER (64)                      1 + 32
 *      MX_WGRAD (512)                     MX_BWD (128) + GROWTH_ACT_F16_WGRAD (8)
 *      MX_TAIL (1024)                     512 + 128 + 8
 *      MX_TRAIN_FORWARD (2048)            1 + 32 + 64 + F16_BACKWARD (256)
 * MX_BWD (128) excludes GROWTH_GRAD_STORE_F16 (4); bits at or above 4096 are refused. */
enum {
    /* inference forward (training = 0) only: the growth planes o1..o4 of every dense block are single f16 tensors, the residual
     * stream and the HR tail stay pairs, weights stay split: 50 instead of 60 stages per block (forward 1e-6 at the reference's
     * init scale; a TRAINING forward ignores the bit -- a 2^-12 perturbation of a pre-activation flips LeakyReLU mask elements) */
    RESR_X2_PLAN_GROWTH_F16_INFER = 1,
    /* backward: the gradients of the growth planes (g_o1..g_o4) are READ as single f16 tensors (their hi tensor): their chunks
     * take two stages in the mirrored backward-data passes and conv1..conv4's weight gradients two tap-products instead of
     * three; they are still stored as pairs, and the BIAS gradients sum hi + lo (one extra tap-product per convolution).  Worst
     * gradient tensor 3-5e-4 vs float64 */
    RESR_X2_PLAN_GROWTH_GRAD_F16 = 2,
    /* with GROWTH_GRAD_F16: store the growth-plane gradients as single f16 tensors too (no lo store in the mirrored passes, no
     * bias job: 64 instead of 68 tap-products per block, ~4 % of an exact16 step).  The bias gradients of conv1..conv4 are then
     * sums of ROUNDED values: the emulation's worst bias tensor reaches 6.7e-4 at 1 x 128^2 (inside the 1e-3 gate, outside the
     * 5e-4 rule the default plan keeps): opt-in. */
    RESR_X2_PLAN_GROWTH_GRAD_STORE_F16 = 4,
    /* backward: the weight products read the growth planes o1..o4 (the X chunks behind the residual stream of conv2..conv5) as their
     * hi tensor: no (x_lo, g_hi) tap-product for them -- 14 fewer tap-products per dense block (54 instead of 68 next to
     * GROWTH_GRAD_F16).  The forward pass and backward-data still see the pairs.  What is dropped is a zero-mean residue of the
     * SMALL operand of conv5's products (the growth planes next to the stream): the worst gradient tensor does not move (emulation:
     * 3.0e-4 -> 3.0e-4 at the reference's init, 3.9e-4 -> 4.0e-4 with the dense weights x 4; conv5's own tensors 7e-7 -> 2.6e-5 / 1e-4) */
    RESR_X2_PLAN_GROWTH_ACT_F16_WGRAD = 8,
    /* with GROWTH_ACT_F16_WGRAD: conv5's products of the growth planes also take g_y's hi tensor alone -- one tap-product
     * (x_hi, g_hi) per growth chunk, 46 per dense block.  Both dropped residues belong to the small operand block of conv5's weight
     * tensor (emulation: conv5's tensors 2.6e-5 -> 3.8e-5, 1.0e-4 -> 1.5e-4 with the dense weights x 4; the worst tensor does not move) */
    RESR_X2_PLAN_GROWTH_ACT_G_HI_WGRAD = 16,
    /* with GROWTH_F16_INFER: the growth chunks of an inference forward take ONE stage (RESR_CONV_SINGLE_W16): 40 instead of 50 stages per
     * dense block */
    RESR_X2_PLAN_GROWTH_W16_INFER = 32,
    /* inference forward (training = 0) only, with GROWTH_F16_INFER + GROWTH_W16_INFER: the pair chunks (residual stream, HR tail) take
     * one f16 stage + one MX-fp8 stage (RESR_CONV_MX_PAIRS) instead of three f16 stages: 30 stage-equivalents per dense block
     * instead of 40.  The workspace grows by the q tensors, the packed weights by their MX region (resr_generator_packed_bytes,
     * resr_generator_mx_offset).  Forward 0.8-1.2e-4 of the fp32 oracle instead of 2e-6 (gate 2e-4). */
    RESR_X2_PLAN_MX_INFER = 64,
    /* backward (training = 1): the backward-data passes of the dense blocks (the four mirrored cout-32 passes and the g_x pass of every
     * block) read EVERY gradient chunk as a pair on one f16 stage + one MX stage (RESR_CONV_MX_PAIRS): 40 stage-equivalents per block
     * instead of 50 (GROWTH_GRAD_F16) or 60, and nothing is dropped -- the growth-plane gradients enter with both halves again: worst
     * gradient tensor 0.8-1.2e-4 vs float64 in the emulation (GROWTH_GRAD_F16: 3-5e-4).  The gradient planes gT / gS carry q tensors
     * (written by the passes that produce them), the packed buffer its MX region.  The forward pass and the weight gradients are
     * untouched (GROWTH_GRAD_F16 then only shapes the weight products); not together with GROWTH_GRAD_STORE_F16. */
    RESR_X2_PLAN_MX_BWD = 128,
    /* opt-in: the exact16 forward (all pairs: reference-exact masks, fp32-class losses) followed by FAST mode's backward pass -- plain f16
     * on the hi tensors, f16 weights: resr_generator_backward then takes a RESR_F16 packing of the same table as `packed`.  Most of fast
     * mode's gradient error is its own forward's mask flips, not its backward pass's roundings (emulation: median 4-6e-3 -> 5-7e-4 under the
     * L1 loss): a third operating point between fast and exact16.  Overrides the other backward bits. */
    RESR_X2_PLAN_F16_BACKWARD = 256,
    /* with MX_BWD + GROWTH_ACT_F16_WGRAD (the stream chunks are then the pair chunks): the weight gradients of the dense blocks take the two 2^-12-weighted tap-products (x_hi, g_lo) + (x_lo, g_hi) of every
     * STREAM chunk as ONE MX job -- K is pixels there: 8-bit transpose reads (ds_read_b64_tr_b8) of the staged q records feed one
     * v_mfma_scale_f32_32x32x64_f8f6f4 per output row and tap, block 0 = (g_lo, x_hi), block 1 = (g_hi, x_lo) -- half the staged bytes
     * and half the matrix time of the two f16 tap-products, and conv1..conv4 get their (x_hi, g_lo) term back (GROWTH_GRAD_F16 drops it).
     * The training forward then emits the q tensor of the residual stream (conv1 and every closing convolution: + 2 of 12 plane stores
     * per dense block), the workspace holds it, and g_lo's share of a bias gradient is summed by the MX job itself from the bf8 bytes of
     * its G fragments (a bias moves by 1-2e-5 against the f16 lo tensor's sum; gate 5e-5 in tests/test_gpu_mx.py). */
    RESR_X2_PLAN_MX_WGRAD = 512,
    /* with MX_WGRAD: the same treatment for the 4x-resolution tail (conv3, conv4, upsampling2 -- a third of an exact16 step's weight-gradient
     * work and a tenth of its backward-data work): the training forward emits the q tensors of u1, u2 and c3, the layout pass that brings the
     * incoming gradient in and the two masked tail passes emit those of the gradient tensors, the three tail passes that read them run one
     * f16 + one MX stage per chunk, and the three weight gradients take their correction tap-products as MX jobs.  upsampling1 keeps its f16
     * form (its gradient comes out of a 2 x 2 sum-pool). */
    RESR_X2_PLAN_MX_TAIL = 1024,
    /* opt-in, with GROWTH_F16_INFER + GROWTH_W16_INFER + MX_INFER + F16_BACKWARD (the named plan 2401, "output parity"): a TRAINING
     * forward runs the inference MX plan -- growth planes o1..o4 single f16 against f16 weights (one stage per growth chunk), pair
     * chunks on one f16 + one MX stage (RESR_CONV_MX_PAIRS | RESR_CONV_MX_SIGNBITS) --, every LeakyReLU still writes its sign words
     * (from the fp32 value the stored output is rounded from), and F16_BACKWARD's pass runs behind it on the hi tensors and the sign
     * words.  The training forward is bit-identical to an inference forward of plan 97 (output 0.9-1.1e-4 of the fp32 oracle, gate
     * 2e-4); the gradients are in fast mode's class (a fifth of its distance from the all-pairs plan: the MX forward's mask flips).
     * The workspace grows by the q tensors, the packed buffer holds its MX region. */
    RESR_X2_PLAN_MX_TRAIN_FORWARD = 2048
};

size_t resr_generator_param_count(const ResrGeneratorDesc* d);
size_t resr_generator_packed_bytes(const ResrGeneratorDesc* d, int32_t backward);
/* RESR_F16X2: byte offset of the MX region (resr_pack_weights_mx; RESR_X2_PLAN_MX_INFER) inside a packed buffer of
 * resr_generator_packed_bytes(d, *) bytes: pack the same chunk table there after resr_pack_weights.  0 for other dtypes. */
size_t resr_generator_mx_offset(const ResrGeneratorDesc* d);
size_t resr_generator_workspace_bytes(const ResrGeneratorDesc* d);
/* The first resr_generator_chain_state_bytes(d) bytes of a generator workspace are the chain state of its dense-block
 * launches (resr_conv3x3_chain) and, behind it, the 256-byte slot of the backward pass's gradient pre-scale (below): the caller
 * fills them with zeros once, when the workspace is allocated. */
size_t resr_generator_chain_state_bytes(const ResrGeneratorDesc* d);
/* fills `chunks` (host memory, capacity in elements) and returns the count; forward table first,
 * then (if backward) the backward-data table; dst offsets are relative to one packed buffer */
int64_t resr_generator_pack_table(const ResrGeneratorDesc* d, int32_t backward,
                                  ResrPackChunk* chunks, int64_t capacity);
/* test aid: byte offsets inside the workspace of {x_in, ws[0], out1, trunk_out, feat, u1, u2, c3,
 * ymask, g4, gA, gB, gM1, gF, gT0, gT1, gT2, gT3, gS, gxin, partial}; -1 = not allocated */
int64_t resr_generator_buffer_offsets(const ResrGeneratorDesc* d, int64_t* out, int64_t capacity);
int resr_generator_forward(const ResrGeneratorDesc* d, const float* x_nchw, const float* params,
                           const void* packed, void* workspace, size_t workspace_bytes,
                           float* y_nchw, void* stream);
/* grad_ready_events (optional, n_events = n_blocks + 2 hipEvent_t handles, else NULL / 0): recorded on `stream` as soon as a
 * range of the gradient arena is final, in backward order -- [0] the tail (conv2, upsampling1/2, conv3, conv4: the END of the
 * arena), [1 + j] RRDB n_blocks-1-j, [n_blocks + 1] conv1 (everything).  A data-parallel caller makes its communication
 * stream wait on them and all-reduces each range while the rest of the backward pass still runs.
 * RESR_F16 / RESR_F16X2: the pass does not depend on the scale of gy -- when max |gy| < 2^6 it runs on gy * 2^k (max in [2^6, 2^7)) and hands
 * grad / gx out times 2^-k, both exact, so its f16 tensors never see subnormals at small loss scales; an inf / NaN in gy turns the
 * lift off and reaches grad (resr_discriminator_backward does the same).  $RESR_X2_GRAD_PRESCALE_LOG2, RESR_X2_NO_GRAD_PRESCALE=1.
 * The lift leaves 2^9 of headroom to f16's maximum.  A gradient that grows by more than that on its way back overflows whatever the
 * caller's loss scale is -- a GradScaler halving its scale cannot cure an overflow the lift re-creates every step (the symptom would
 * be found_inf on every step and a scale decaying to nothing) -- so the pass backs off by itself: a lifted pass that writes a non-finite
 * weight gradient sets a flag in the workspace's pre-scale slot, and every later pass on that workspace aims 2^4 lower per such event
 * (sticky, up to 2^40 = lift off: the caller's scale rules again).  The overflowed step is the GradScaler's to skip, as ever. */
int resr_generator_backward(const ResrGeneratorDesc* d, const float* gy_nchw, const float* params,
                            const void* packed, void* workspace, size_t workspace_bytes,
                            float* grad_params, float* gx_nchw, void* stream,
                            void* const* grad_ready_events, int32_t n_events);

/* Compact generator (upstream Real-ESRGAN's SRVGGNetCompact: realesr-animevideov3, realesr-general-x4v3): the inference entries
 * below, and "Compact generator: training" behind them.
 * x [N,3,H,W] -> conv 3->64, act, num_conv x (conv 64->64, act), conv 64->3*s*s, pixel-shuffle(s), + nearest-upsampled x
 * -> y [N,3,sH,sW] fp32 NCHW, no clamp.  Any H, W >= 1 (no padding beyond each conv's own).  Parameters in the upstream
 * module's named_parameters() order: per conv k = 0 .. num_conv + 1 its weight [cout,cin,3,3] and bias [cout], and behind
 * every conv but the last, with act = RESR_COMPACT_PRELU, the 64 PReLU slopes.  Passes: the input as NHWC (channels padded to
 * 32), num_conv + 1 64-channel convolutions ping-ponging between two NHWC workspace buffers (bias + activation in the
 * epilogue: per-channel PReLU as v > 0 ? v : a[c] * v, LeakyReLU 0.1, ReLU), the last conv as an fp32 NCHW tensor, then one
 * launch for pixel-shuffle + residual.  See real_esrgan-pytorch_amd/csrc/compact.hip. */
enum { RESR_COMPACT_PRELU = 0, RESR_COMPACT_LRELU = 1, RESR_COMPACT_RELU = 2 };
typedef struct {
    int32_t n, h, w;          /* input batch / height / width                                     */
    int32_t num_conv;         /* 64->64 body convs (upstream num_conv: 16 or 32)                  */
    int32_t upscale;          /* 1, 2, 3 or 4                                                     */
    int32_t act;              /* RESR_COMPACT_*                                                   */
    int32_t dtype;            /* RESR_F16 fast / RESR_F16X2 exact16 (three-stage pairs) / RESR_F32 strict */
    int32_t reserved_;
} ResrCompactDesc;

/* Host planning calls (no GPU needed); 0 (or RESR_ERR_ARG from the pack table) for an invalid descriptor. */
size_t resr_compact_param_count(const ResrCompactDesc* d);
/* bytes of the packed-weight buffer resr_pack_weights fills from resr_compact_pack_table(d) (dst offsets relative to it) */
size_t resr_compact_packed_bytes(const ResrCompactDesc* d);
int64_t resr_compact_pack_table(const ResrCompactDesc* d, ResrPackChunk* chunks, int64_t capacity);
size_t resr_compact_workspace_bytes(const ResrCompactDesc* d);
/* Enqueues the whole network on `stream`: no allocation, no synchronisation, graph-capture safe (as resr_generator_forward). */
int resr_compact_forward(const ResrCompactDesc* d, const float* x_nchw, const float* params, const void* packed,
                         void* workspace, size_t workspace_bytes, float* y_nchw, void* stream);

/* Compact generator: training (csrc/compact.hip, compact_train.hip).  Same descriptor, RESR_F16 (fast) or RESR_F32 (strict);
 * RESR_F16X2 is refused by every entry below (0 / RESR_ERR_ARG: exact16 training is not built).
 * resr_compact_forward_train: resr_compact_forward's ends and result (strict: the same bits; fast: a negative activation is rounded
 *   twice, f16(slope * f16(z))), with every body convolution run on a plain (bias) epilogue that stores the pre-activation z_k and one
 *   element-wise launch that stores a_k = act(z_k); both stay in the workspace for the backward pass.
 * resr_compact_backward: gy_nchw [N,3,sH,sW] -> grad_params (the layout of the parameter arena, resr_compact_param_count floats,
 *   OVERWRITTEN) and, gx_nchw != NULL, gx_nchw [N,3,H,W].  It reads what the forward train call left in the SAME workspace, and the same
 *   packed buffer.  RESR_F16 lifts a small gy into f16's normal range and hands every result back unscaled, exactly as
 *   resr_generator_backward does (the pre-scale slot and its sticky back-off); RESR_F32 gets no lift.  No floating-point atomics: the
 *   same inputs give the same bits.
 * Packed weights: resr_compact_train_pack_table is resr_compact_pack_table's chunks followed by every convolution's transposed
 *   (backward-data) chunks in the same order; resr_compact_train_packed_bytes sizes the buffer.
 * Workspace (every buffer 256-byte aligned; es = 2 or 4 bytes, px = N H W, cpl = 3 s^2 rounded up to 32):
 *     256                          the gradient pre-scale slot: resr_compact_train_state_bytes, zero-filled ONCE by the caller
 *   + px * 32 * es                 the input as NHWC
 *   + 2 * (num_conv + 1) * px * 64 * es     z_k and a_k of every activation layer
 *   + px * 3 s^2 * 4               the last convolution's fp32 output
 *   + px * (cpl + 2 * 64 + 32) * es         the gradients g_t, two ping-pong 64-channel tensors, the input gradient
 *   + the slope-gradient partials (PReLU: at most 1024 * 256 bytes) + the weight-gradient slabs of the largest layer.
 * Refusals come before the first launch: RESR_ERR_ARG (a bad descriptor, RESR_F16X2, a null pointer other than gx_nchw),
 * RESR_ERR_WORKSPACE (workspace_bytes below resr_compact_train_workspace_bytes).  Both calls only enqueue. */
size_t resr_compact_train_packed_bytes(const ResrCompactDesc* d);
int64_t resr_compact_train_pack_table(const ResrCompactDesc* d, ResrPackChunk* chunks, int64_t capacity);
size_t resr_compact_train_workspace_bytes(const ResrCompactDesc* d);
size_t resr_compact_train_state_bytes(const ResrCompactDesc* d);
int resr_compact_forward_train(const ResrCompactDesc* d, const float* x_nchw, const float* params, const void* packed,
                               void* workspace, size_t workspace_bytes, float* y_nchw, void* stream);
int resr_compact_backward(const ResrCompactDesc* d, const float* gy_nchw, const float* params, const void* packed,
                          void* workspace, size_t workspace_bytes, float* grad_params, float* gx_nchw, void* stream);

/* The uint8 frame path (real_esrgan-pytorch_amd/csrc/frames.hip).  Images are uint8 HWC, contiguous: x_u8 [N,H,W,3] ->
 * y_u8 [N,sH,sW,3].  The result is defined as what the float path followed by the host's truncating uint8 conversion gives,
 * bit for bit: every input channel enters as (float)u8 / 255.0f (one IEEE division), converted to the model's arithmetic
 * exactly as resr_nchw_to_nhwc converts that float; every output channel leaves as v * 255.0f, clamped to [0, 255], truncated,
 * where v is the fp32 value the float path would have stored (for the compact net: t + x, one add).  A NaN in v is outside
 * the contract (the host's float -> uint8 cast of a NaN is undefined too).  y_u8 / dst_u8 must be 4-byte aligned (the kernels
 * store dwords); a misaligned pointer is RESR_ERR_ARG.
 *
 * resr_compact_forward_u8: the launch sequence of resr_compact_forward with the conversions fused into its first and last
 * kernel.  Same descriptor, packed weights and workspace (resr_compact_workspace_bytes: this path needs nothing more), same
 * checks and error codes, all before the first launch.  No fp32 copy of the frame exists on this path: the tail re-reads x_u8
 * for the residual, so x_u8 must stay valid until the call has run. */
int resr_compact_forward_u8(const ResrCompactDesc* d, const uint8_t* x_u8, const float* params, const void* packed,
                            void* workspace, size_t workspace_bytes, uint8_t* y_u8, void* stream);
/* The generic conversions, one launch each, for models whose first / last kernel is not fused (the RRDB generator, tiled
 * frames): u8 [N,H,W,3] -> fp32 [N,3,H,W] (/ 255.0f) and fp32 [N,3,H,W] -> u8 [N,H,W,3] (* 255.0f, clamp, truncate).
 * n, h, w <= 0 or a null pointer: RESR_ERR_ARG, before any launch. */
int resr_u8_to_nchw(const uint8_t* src_u8, float* dst_f32, int32_t n, int32_t h, int32_t w, void* stream);
int resr_nchw_to_u8(const float* src_f32, uint8_t* dst_u8, int32_t n, int32_t h, int32_t w, void* stream);

/* Outscale: a final size that is not the network's factor (real_esrgan-pytorch_amd/csrc/image_resize.hip).  The resampler is the
 * MATLAB-style bicubic of the reference's image_resize (a = -0.5, antialiased when shrinking, symmetric edges, output size
 * ceil(in * scale)), given per axis as a banded tap table on the device: idx [out, taps] int32 (0-based source positions, the
 * reflection folded in) and w [out, taps] float32, rows contiguous -- imgproc.resize_band_tables builds them.
 *   out = W-pass(H-pass(src)), each pass acc = fmaf(v[idx[k]], w[k], acc) from 0, k ascending, fp32 throughout.
 * An idx entry outside the source is clamped into it (never read out of bounds); tables whose rows are not the band of a resize
 * (a tile's entries further apart than floor((t - 1) * in / (out - 1)) + 2 + taps) give undefined VALUES, not undefined accesses.
 *
 * resr_image_resize: src fp32 [N,C,H,W] -> dst fp32 [N,C,oh,ow] (out_u8 = 0) or uint8 [N,oh,ow,3] (out_u8 = 1: C must be 3, dst
 * 4-byte aligned; * 255.0f, clamp, truncate as resr_nchw_to_u8; a NaN is outside the contract as above).
 * resr_compact_forward_u8_scaled: resr_compact_forward_u8 with the resize fused into its last kernel: y_u8 is [N,oh,ow,3], the
 * source of the resize is the [N,3,H*s,W*s] frame resr_compact_forward would have stored (t + x, one add), which is never written;
 * same descriptor, packed weights and workspace (resr_compact_workspace_bytes: nothing more).  Its result equals
 * resr_image_resize(out_u8 = 1) of that frame bit for bit.
 * Both: a null pointer, n, c, h, w, oh, ow <= 0, taps outside [1, 4096], N * ceil(C / 3) > 65535, or a scale so small that the taps
 * of ONE output pixel do not fit a 64 KB LDS tile are RESR_ERR_ARG; every check comes before the first launch.  The caller
 * guarantees the tables' lengths (oh * taps_y, ow * taps_x entries). */
int resr_image_resize(const float* src_f32, void* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t oh, int32_t ow,
                      const int32_t* idx_y, const float* w_y, int32_t taps_y, const int32_t* idx_x, const float* w_x, int32_t taps_x,
                      int32_t out_u8, void* stream);
int resr_compact_forward_u8_scaled(const ResrCompactDesc* d, const uint8_t* x_u8, const float* params, const void* packed,
                                   void* workspace, size_t workspace_bytes, uint8_t* y_u8, int32_t oh, int32_t ow,
                                   const int32_t* idx_y, const float* w_y, int32_t taps_y, const int32_t* idx_x, const float* w_x,
                                   int32_t taps_x, void* stream);

/* YUV 4:2:0 frames (real_esrgan-pytorch_amd/csrc/frames.hip): what video decoders deliver and encoders consume, 1.5 bytes per pixel.
 * A frame of luma size H x W (both even) is H * W * 3 / 2 bytes, seen as a uint8 array [3H/2, W]; batches are [N,3H/2,W], contiguous:
 *   RESR_YUV_I420: Y [H,W], then Cb [H/2,W/2], then Cr [H/2,W/2];      RESR_YUV_NV12: Y [H,W], then [H/2,W/2,2] interleaved Cb,Cr.
 * The path is DEFINED as a composition over the uint8 RGB path above, bit for bit, with no tolerance anywhere:
 *   resr_compact_forward_yuv420(f) == resr_rgb_to_yuv420(resr_compact_forward_u8(resr_yuv420_to_rgb(f)))
 * and the two colour conversions are integer functions of bytes (int32 throughout, >> arithmetic i.e. floor), studio range, with
 * the Q16 tables of the descriptor (rows of fq: Y, Cb, Cr over R, G, B; rows of iq: R, G, B over Y - 16, Cb - 128, Cr - 128;
 * frames.yuv420_tables computes them for BT.601 / BT.709):
 *   yuv420_to_rgb: pixel (y, x) takes Y[y,x], Cb[y/2,x/2], Cr[y/2,x/2] (chroma replicated over its 2x2 block);
 *                  rgb[c] = clamp((iq[c][0] * (Y - 16) + iq[c][1] * (Cb - 128) + iq[c][2] * (Cr - 128) + 32768) >> 16, 0, 255);
 *                  every byte value is legal input, values outside the studio range clamp.
 *   rgb_to_yuv420: Y = (fq[0] . rgb + (16 << 16) + 32768) >> 16 per pixel; with S the sum of a 2x2 block's four (R, G, B):
 *                  Cb = (fq[1] . S + (128 << 18) + (1 << 17)) >> 18, Cr likewise with fq[2] (a centre-sited box average of the
 *                  unrounded chroma).  The kernels do not clamp: with the tables of frames.yuv420_tables no RGB triple leaves
 *                  Y 16..235, Cb / Cr 16..240; a caller's own tables must keep every result within 0..255.
 * A NaN inside the net is outside the contract exactly as for resr_compact_forward_u8 (it quantises to the byte 0 here).
 *
 * resr_compact_forward_yuv420: resr_compact_forward_u8 with both conversions fused into its first and last kernel: x_yuv
 * [N, 3 d->h / 2, d->w] -> y_yuv [N, 3 s d->h / 2, s d->w], same layout both ways.  Same descriptor, packed weights and workspace
 * (resr_compact_workspace_bytes: nothing more), same checks and codes.  No RGB frame exists on this path: the tail recomputes the
 * residual from x_yuv, which must stay valid until the call has run.
 * resr_yuv420_to_rgb / resr_rgb_to_yuv420: the generic conversions, one launch each, [N,3H/2,W] <-> uint8 HWC [N,H,W,3], for every
 * case whose ends are not fused (the RRDB generator, tiled frames, an outscale the entries under "YUV outscale" do not take).
 * RESR_ERR_ARG before any launch: a null pointer; n, h, w <= 0; an odd h or w (d->h, d->w: then the output's are even too); a
 * layout other than RESR_YUV_*; a destination (for resr_rgb_to_yuv420 the source too) that is not aligned for the wide stores its
 * width selects: 8 bytes for y_yuv when s * d->w is a multiple of 8, 4 bytes for the generic conversions when w is a multiple of 4
 * (other even widths take byte stores and need no alignment). */
enum { RESR_YUV_I420 = 0, RESR_YUV_NV12 = 1 };
typedef struct {
    int32_t layout;           /* RESR_YUV_*                                                       */
    int32_t fq[9];            /* RGB -> YCbCr, Q16, row-major                                     */
    int32_t iq[9];            /* YCbCr -> RGB, Q16, row-major                                     */
} ResrYuvDesc;                /* host struct; the kernels take it by value                        */
int resr_compact_forward_yuv420(const ResrCompactDesc* d, const uint8_t* x_yuv, const float* params, const void* packed,
                                void* workspace, size_t workspace_bytes, uint8_t* y_yuv, const ResrYuvDesc* yuv, void* stream);
int resr_yuv420_to_rgb(const uint8_t* src, uint8_t* dst_hwc, int32_t n, int32_t h, int32_t w, const ResrYuvDesc* yuv, void* stream);
int resr_rgb_to_yuv420(const uint8_t* src_hwc, uint8_t* dst, int32_t n, int32_t h, int32_t w, const ResrYuvDesc* yuv, void* stream);

/* 10-bit YUV 4:2:0 frames (frames.hip): what decoders deliver for most HEVC / AV1 material, 1024 levels instead of 256 at both ends
 * of the network.  The geometry is that of the 8-bit frames with a little-endian 16-bit word per sample, 3 bytes per pixel: a frame
 * of luma size H x W (both even) is a uint16 array [3H/2, W], batches [N,3H/2,W], contiguous:
 *   RESR_YUV_I420P10 (yuv420p10le): planes as RESR_YUV_I420, the sample in the low 10 bits: read word & 1023, written with the
 *                                   high 6 bits zero;
 *   RESR_YUV_P010 (p010le):         planes as RESR_YUV_NV12, the sample in the high 10 bits: read word >> 6, written as
 *                                   sample << 6 with the low 6 bits zero.
 * Every 16-bit word is legal input.  The descriptor is ResrYuvDesc with one of these two layouts and the Q16 tables of the 10-bit
 * studio range (frames.yuv420p10_tables; rows of iq over Y - 64, Cb - 512, Cr - 512); the conversions are the 8-bit ones with 64 /
 * 512 / 1023 in place of 16 / 128 / 255, int32 throughout (the largest accumulator is below 2^28 with those tables):
 *   in : rgb10[c] = clamp((iq[c] . (Y - 64, Cb - 512, Cr - 512) + 32768) >> 16, 0, 1023), chroma replicated over its 2x2 block;
 *        the model's input is (float)rgb10 / 1023.0f, one IEEE division;
 *   out: q10(v) = trunc(clamp(v * 1023.0f, 0, 1023)) (a NaN gives 0); Y = (fq[0] . q10 + (64 << 16) + 32768) >> 16 per pixel;
 *        Cb = (fq[1] . S + (512 << 18) + (1 << 17)) >> 18 with S the sum of a 2x2 block's four q10 triples, Cr likewise with fq[2].
 *        The kernels mask the results to 10 bits and do not clamp: with the tables above Y stays in 64..940, Cb / Cr in 64..960.
 * The path is DEFINED as a composition, bit for bit:
 *   resr_compact_forward_yuv420p10(f) == resr_nchw_to_yuv420p10(resr_compact_forward(resr_yuv420p10_to_nchw(f)))
 * resr_compact_forward_yuv420p10: resr_compact_forward_yuv420 for these frames, both conversions inside the first and the last
 * kernel, x_yuv [N, 3 d->h / 2, d->w] -> y_yuv [N, 3 s d->h / 2, s d->w] in the same layout; same descriptor, packed weights and
 * workspace, same checks and codes.  Neither an RGB frame nor an fp32 copy of the input exists: the tail recomputes the residual
 * from x_yuv, which must stay valid until the call has run.
 * resr_yuv420p10_to_nchw / resr_nchw_to_yuv420p10: the generic conversions, one launch each, straight between the frames and fp32
 * [N,3,H,W], for every case whose ends are not fused (the RRDB generator, tiled frames, an outscale "YUV outscale" does not take).
 * RESR_ERR_ARG before any launch: a null pointer; n, h, w <= 0; an odd h or w; a layout other than these two (the 8-bit entries
 * refuse these two in turn); a misaligned end: y_yuv 16-byte aligned when s * d->w is a multiple of 8; for resr_nchw_to_yuv420p10
 * dst 8-byte and src_f32 16-byte aligned when w is a multiple of 4; 2 bytes per word and 4 per float everywhere else.
 * A source and a destination of different depth, layout or matrix: "Mixed frame formats" below.  12 / 16-bit samples, full range and
 * 4:2:2 / 4:4:4 are not provided. */
enum { RESR_YUV_I420P10 = 2, RESR_YUV_P010 = 3 };
int resr_compact_forward_yuv420p10(const ResrCompactDesc* d, const uint16_t* x_yuv, const float* params, const void* packed,
                                   void* workspace, size_t workspace_bytes, uint16_t* y_yuv, const ResrYuvDesc* yuv, void* stream);
int resr_yuv420p10_to_nchw(const uint16_t* src, float* dst_f32, int32_t n, int32_t h, int32_t w, const ResrYuvDesc* yuv, void* stream);
int resr_nchw_to_yuv420p10(const float* src_f32, uint16_t* dst, int32_t n, int32_t h, int32_t w, const ResrYuvDesc* yuv, void* stream);

/* YUV outscale: the YUV 4:2:0 ends (8 and 10 bits) on the resized tail of resr_compact_forward_u8_scaled (image_resize.hip).  x_yuv
 * [N, 3 d->h / 2, d->w] -> y_yuv [N, 3 oh / 2, ow] in the same layout; oh x ow and the tap tables as for resr_compact_forward_u8_scaled
 * (a resize of the s d->h x s d->w frame).  DEFINED by the compositions above, bit for bit:
 *   resr_compact_forward_yuv420_scaled(f)    == resr_rgb_to_yuv420(resr_compact_forward_u8_scaled(resr_yuv420_to_rgb(f)))
 *   resr_compact_forward_yuv420p10_scaled(f) == resr_nchw_to_yuv420p10(resr_image_resize(resr_compact_forward(resr_yuv420p10_to_nchw(f))))
 * One launch sequence: the YUV head, the convs, one tail.  The tail forms the frame resr_compact_forward would have stored tile by
 * tile in LDS (t + level / 255.0f or / 1023.0f, the level recomputed from x_yuv: neither an RGB nor an fp32 frame exists), resizes
 * it, quantises the three sums of every pixel (* 255.0f or * 1023.0f, clamp, truncate) and applies the integer RGB -> YUV formulas to
 * the levels of each 2x2 block.  Output tiles have an even height and width, so every chroma sample has one owner.
 * Same descriptor, packed weights and workspace as resr_compact_forward (resr_compact_workspace_bytes: nothing more).
 * RESR_ERR_ARG before any launch: a null pointer; an odd d->h, d->w, oh or ow; a descriptor of the other bit depth or an unknown
 * layout; y_yuv not 4-byte aligned (rows leave as dword stores); oh, ow <= 0, taps outside [1, 4096], N > 65535; a scale so small that
 * the taps of one 2x2 block of outputs do not fit a 64 KB LDS tile.
 * resr_compact_yuv420_scaled_fits: that last condition as a query with no device work -- 1 when a tile of even height and width
 * fits for an h x w frame through a model of factor s resized to oh x ow with these taps (bits: 8 or 10), else 0 (bad arguments
 * included).  A caller asks it to choose between these entries and the composition, which takes any scale the RGB tail takes. */
int resr_compact_forward_yuv420_scaled(const ResrCompactDesc* d, const uint8_t* x_yuv, const float* params, const void* packed,
                                       void* workspace, size_t workspace_bytes, uint8_t* y_yuv, int32_t oh, int32_t ow,
                                       const int32_t* idx_y, const float* w_y, int32_t taps_y, const int32_t* idx_x, const float* w_x,
                                       int32_t taps_x, const ResrYuvDesc* yuv, void* stream);
int resr_compact_forward_yuv420p10_scaled(const ResrCompactDesc* d, const uint16_t* x_yuv, const float* params, const void* packed,
                                          void* workspace, size_t workspace_bytes, uint16_t* y_yuv, int32_t oh, int32_t ow,
                                          const int32_t* idx_y, const float* w_y, int32_t taps_y, const int32_t* idx_x, const float* w_x,
                                          int32_t taps_x, const ResrYuvDesc* yuv, void* stream);
int resr_compact_yuv420_scaled_fits(int32_t h, int32_t w, int32_t s, int32_t oh, int32_t ow, int32_t taps_y, int32_t taps_x,
                                    int32_t bits);

/* Mixed frame formats: a source descriptor and a destination descriptor, each any of the four layouts above with its own tables --
 * 8 bits in and 10 out (or the reverse), NV12 / P010 in and planar out (or the reverse), BT.601 in and BT.709 out.  With top = 255
 * or 1023 for the depth of a side, DEFINED bit for bit by the functions above:
 *   y = rgb_to_yuv_dst(q_dst(float_path(yuv_to_rgb_src(x) / top_src)))            q(v) = trunc(clamp(v * top, 0, top)), fp32
 * float_path: resr_compact_forward on fp32 NCHW, for the scaled entry followed by resr_image_resize (fp32 out).  With src_yuv and
 * dst_yuv equal this is, term for term, the definition of the four same-format entries, and the same kernels run.
 * resr_compact_forward_yuv420_mixed: x_yuv [N, 3 d->h / 2, d->w] in src_yuv's layout -> y_yuv [N, 3 s d->h / 2, s d->w] in dst_yuv's;
 * bytes or 16-bit words on either side as that side's layout says.  One launch sequence: the head of the source's depth, the convs,
 * one tail that recomputes the residual from x_yuv with the source's word type, layout, iq and / top_src, and quantises, converts
 * and stores with the destination's top, fq and layout.  resr_compact_forward_yuv420_mixed_scaled: the same on the resized tail
 * of "YUV outscale" -> y_yuv [N, 3 oh / 2, ow].  Same descriptor, packed weights and workspace as resr_compact_forward.
 * RESR_ERR_ARG before any launch: a null pointer; a layout on either side that is no RESR_YUV_*; an odd d->h or d->w; y_yuv not
 * aligned as the destination's depth asks at its width (8-bit: 8 bytes when s * d->w is a multiple of 8; 10-bit: 16 bytes then,
 * else 2; the scaled entry: 4 bytes); for the scaled entry everything resr_compact_forward_yuv420_scaled refuses (an odd oh or ow,
 * a null table, taps outside [1, 4096], N > 65535, a scale with no even LDS tile: resr_compact_yuv420_scaled_fits with the
 * destination's bits).  An rgb24 frame on one side is not fused: compose resr_u8_to_nchw / resr_nchw_to_u8 with the generic
 * conversions above. */
int resr_compact_forward_yuv420_mixed(const ResrCompactDesc* d, const void* x_yuv, const ResrYuvDesc* src_yuv, const float* params,
                                      const void* packed, void* workspace, size_t workspace_bytes, void* y_yuv,
                                      const ResrYuvDesc* dst_yuv, void* stream);
int resr_compact_forward_yuv420_mixed_scaled(const ResrCompactDesc* d, const void* x_yuv, const ResrYuvDesc* src_yuv, const float* params,
                                             const void* packed, void* workspace, size_t workspace_bytes, void* y_yuv, int32_t oh,
                                             int32_t ow, const int32_t* idx_y, const float* w_y, int32_t taps_y, const int32_t* idx_x,
                                             const float* w_x, int32_t taps_x, const ResrYuvDesc* dst_yuv, void* stream);

/* Image modes (frames.hip): the still images upstream's RealESRGANer.enhance takes besides 8-bit RGB -- grey, RGBA and 16 bits per
 * channel.  An image batch is [N,H,W,C] of bytes (bits = 8, top = 255) or of little-endian 16-bit words (bits = 16, top = 65535), HWC,
 * contiguous; C = 1 grey, 3 RGB, 4 RGBA.  planes = 2 for RGBA, else 1: the network runs on planes * N three-channel images,
 *   to_rgb:   image b < N  is the colour of image b (grey: the level three times); image N + b (RGBA only) is the alpha plane of image b
 *             three times -- upstream's alpha_upsampler = "realesrgan": alpha goes through the network as a grey image;
 *   grey(r, g, b) = (4899 r + 9617 g + 1868 b + 8192) >> 14 on integer levels at both depths (cv2's fixed-point RGB2GRAY; the
 *             coefficients sum to 2^14, so grey(v, v, v) = v, and the sum stays below 2^31 at 65535);
 *   to_image: RGB the levels themselves; grey: grey of the three levels; RGBA: the colour of image b, and as the fourth channel
 *             grey of the three levels of image N + b.
 * DEFINED bit for bit, with q(v) = trunc(clamp(v * top, 0, top)) in fp32 (a NaN gives 0, outside the contract as everywhere):
 *   resr_compact_forward_image(x) == to_image(q(resr_compact_forward(to_rgb(x) / top)))        (/ top: one IEEE fp32 division)
 * resr_compact_forward_image: the launch sequence of resr_compact_forward with both conversions inside its first and last kernel;
 * x [N,H,W,C] -> y [N,sH,sW,C], same channels and depth.  d->n is the NETWORK's batch, planes * N; the descriptor's other fields, the
 * packed weights and the workspace are resr_compact_forward's (resr_compact_workspace_bytes: nothing more).  The tail re-reads x for
 * the residual, so x must stay valid until the call has run.  channels = 3, bits = 8 runs the kernels of resr_compact_forward_u8.
 * resr_image_to_nchw / resr_nchw_to_image: the generic conversions, one launch each, [n_images,H,W,C] <-> fp32 [planes * n_images,3,H,W]
 * (to_rgb / top, and to_image(q(.))), for every case whose ends are not fused (the RRDB generator, tiled frames).
 * Alignment, the widest access of each mode (a thread stores a group of output pixels whose bytes are whole dwords, and loads an RGBA
 * pixel as one word): y / dst 16 bytes for RGBA (either depth), 8 for 16-bit grey, 4 for 8-bit grey and for RGB (either depth);
 * x / src 4 bytes for 8-bit RGBA, 8 for 16-bit RGBA, 2 for the other 16-bit modes; the float tensor 4 bytes.
 * RESR_ERR_ARG before any launch, nothing written: a null pointer; channels not 1, 3 or 4; bits not 8 or 16; channels = 4 with an odd
 * d->n; a pointer not aligned as above; n_images, h, w <= 0 or more threads than a grid holds; a bad descriptor -- with RESR_F16X2 that
 * includes planes * N * H * W > 2^24, the cap of resr_compact_forward. */
typedef struct {
    int32_t channels;         /* 1 grey, 3 RGB, 4 RGBA                                            */
    int32_t bits;             /* 8 or 16 per channel                                              */
} ResrImageDesc;
int resr_compact_forward_image(const ResrCompactDesc* d, const void* x, const float* params, const void* packed, void* workspace,
                               size_t workspace_bytes, void* y, const ResrImageDesc* img, void* stream);
int resr_image_to_nchw(const void* src, float* dst_f32, int32_t n_images, int32_t h, int32_t w, const ResrImageDesc* img, void* stream);
int resr_nchw_to_image(const float* src_f32, void* dst, int32_t n_images, int32_t h, int32_t w, const ResrImageDesc* img, void* stream);

/* Image-mode outscale: the image ends on the resized tail of resr_compact_forward_u8_scaled (image_resize.hip).  x [N,H,W,C] -> y
 * [N,oh,ow,C], same channels and depth; oh x ow and the tap tables as for resr_compact_forward_u8_scaled (a resize of the s d->h x
 * s d->w frame).  DEFINED by the functions above, bit for bit, with no tolerance anywhere:
 *   resr_compact_forward_image_scaled(x) == resr_nchw_to_image(resr_image_resize(resr_compact_forward(resr_image_to_nchw(x))))
 * i.e. to_image(q(resize(float path(to_rgb(x) / top)))): the fp32 frame is resized before it is quantised, grey is taken of the three
 * quantised, resized levels, and the RGBA alpha is the grey of the resized alpha images' levels.
 * One launch sequence: the image head, the convs, one tail.  The tail forms the frame resr_compact_forward would have stored tile by
 * tile in LDS (t + level / top, the level read from x: neither the fp32 x4 frames of the planes * N network images nor their resized
 * fp32 frames exist), resizes it, quantises the three sums of every pixel and stores C words per pixel.  An RGBA tile is one workgroup,
 * which runs colour image b and then alpha image N + b over the same LDS; the sums are resr_image_resize's per channel and do not depend
 * on the tile.  d->n is the NETWORK's batch, planes * N, as for resr_compact_forward_image; same packed weights and workspace
 * (resr_compact_workspace_bytes: nothing more).  x must stay valid until the call has run.  channels = 3, bits = 8 runs the kernels of
 * resr_compact_forward_u8_scaled.
 * RESR_ERR_ARG before any launch, nothing written: everything resr_compact_forward_image refuses, with its rule for y replaced by 4-byte
 * alignment (rows leave as dword stores; x keeps the head's alignment); and what resr_compact_forward_u8_scaled refuses: a null table,
 * oh, ow <= 0, taps outside [1, 4096], N > 65535, a scale so small that the taps of one output pixel do not fit a 64 KB LDS tile.
 * resr_compact_image_scaled_fits: that last condition as a query with no device work and no error text -- 1 when a tile fits for an
 * h x w image of that mode through a model of factor s resized to oh x ow with these taps, else 0 (bad arguments included).  A caller
 * asks it to choose between this entry and the composition above. */
int resr_compact_forward_image_scaled(const ResrCompactDesc* d, const void* x, const float* params, const void* packed, void* workspace,
                                      size_t workspace_bytes, void* y, int32_t oh, int32_t ow, const int32_t* idx_y, const float* w_y,
                                      int32_t taps_y, const int32_t* idx_x, const float* w_x, int32_t taps_x, const ResrImageDesc* img,
                                      void* stream);
int resr_compact_image_scaled_fits(int32_t h, int32_t w, int32_t s, int32_t oh, int32_t ow, int32_t taps_y, int32_t taps_x,
                                   int32_t channels, int32_t bits);

/* ---- second-order degradation (imgproc.py device ops; call sites train_realesrnet.py:268-377) ----------
 * Images are planar fp32 [n,c,h,w] in [0,1].  No entry point synchronises or reads back. */

/* filter2d_torch (imgproc.py:1089-1121): reflect pad, correlation with a kh x kw kernel (odd sizes);
 * per_sample = 1: kernel is [n,kh,kw], else [kh,kw] shared. */
int resr_filter2d(const float* src, float* dst, const float* kernel, int32_t n, int32_t c, int32_t h, int32_t w,
                  int32_t kh, int32_t kw, int32_t per_sample, void* stream);
/* USMSharp.forward (imgproc.py:1526-1537) with the Gaussian given as its 1-D factor k1d[ksize];
 * tmp3 = 3*n*c*h*w floats of scratch, kept by a caller that will run resr_usm_sharp_bwd: [mask bytes / row pass | blur | soft].
 * ksize = 51 (USMSharp(50, 0), the only configuration the reference builds) runs as two fused launches -- blur + byte mask, soft
 * mask + combine: 26 B per value instead of the 60 B of six separate passes. */
int resr_usm_sharp(const float* src, float* dst, float* tmp3, const float* k1d, int32_t ksize, float weight,
                   float threshold, int32_t n, int32_t c, int32_t h, int32_t w, void* stream);
/* the same without the soft-mask store the backward pass needs (the degradation path, train_realesrnet.py:268: no graph) */
int resr_usm_sharp_forward_only(const float* src, float* dst, float* tmp3, const float* k1d, int32_t ksize, float weight,
                                float threshold, int32_t n, int32_t c, int32_t h, int32_t w, void* stream);
/* backward of resr_usm_sharp wrt its input (the GAN step differentiates through usm_sharpener(sr),
 * train_realesrgan.py:476): saved_tmp3 = the forward's tmp3 (kept), tmp2 = 2*n*c*h*w floats of scratch.  RESR_ERR_ARG, before
 * any launch, for what the forward refuses: n, c, h, w <= 0, an even ksize or one above 63, ksize / 2 >= h or w. */
int resr_usm_sharp_bwd(const float* x, const float* saved_tmp3, const float* g, float* gx, float* tmp2, const float* k1d,
                       int32_t ksize, float weight, int32_t n, int32_t c, int32_t h, int32_t w, void* stream);
/* F.interpolate (train_realesrnet.py:288,326-329,349-351,366-368): mode 0 area, 1 bilinear, 2 bicubic;
 * scale_h/scale_w > 0: the caller used scale_factor= (coordinates use 1/scale), else size= semantics. */
int resr_resize(const float* src, float* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t oh, int32_t ow,
                int32_t mode, double scale_h, double scale_w, void* stream);
/* standard-normal field, Philox4x32-10 (the device RNG draws of imgproc.py:854,858) */
int resr_randn_fill(float* dst, int64_t count, uint64_t seed, uint64_t stream_id, void* stream);
/* random_add_gaussian_noise_torch (imgproc.py:1029-1057) with the draws given: sigma[n], gray[n] (0/1),
 * field_gray[h*w] (ONE field for the batch, may be NULL when no sample is gray), field_color[n*c*h*w]. */
int resr_noise_gaussian(const float* src, float* dst, const float* sigma, const float* gray, const float* field_gray,
                        const float* field_color, int32_t n, int32_t c, int32_t h, int32_t w, int32_t clip, void* stream);
/* random_add_poisson_noise_torch (imgproc.py:1060-1086): per-sample unique-value counts on the device,
 * Poisson draws from Philox; scale[n], gray[n]. */
size_t resr_noise_poisson_workspace_bytes(int32_t n);
int resr_noise_poisson(const float* src, float* dst, const float* scale, const float* gray, uint64_t seed, void* workspace,
                       int32_t n, int32_t c, int32_t h, int32_t w, int32_t clip, void* stream);
/* DiffJPEG(differentiable=False).forward (imgproc.py:1462-1494); quality[n] (not mutated);
 * coeffs (optional) receives the rounded coefficients [n][Y blocks | Cb blocks | Cr blocks][64]. */
int resr_jpeg(const float* src, float* dst, const float* quality, float* coeffs, int32_t n, int32_t h, int32_t w,
              int32_t flags /* bit0: clamp the input to [0,1] first (train_realesrnet.py:308) */, void* stream);
/* clamp(round(x*255))/255 on lr + random_crop of both (train_realesrnet.py:374-377, imgproc.py:1894-1934).  hr_out = NULL is
 * allowed when the HR window is the whole image (hr_size == hr_h == hr_w): the caller keeps using `hr` instead of a copy of it. */
int resr_quantize_crop(const float* lr, const float* hr, float* lr_out, float* hr_out, int32_t n, int32_t c, int32_t lr_h,
                       int32_t lr_w, int32_t hr_h, int32_t hr_w, int32_t hr_size, int32_t upscale, int32_t hr_top,
                       int32_t hr_left, void* stream);

/* ---- integer mode of blur / resize / JPEG (north_star: "blur/resize/JPEG bit-exact in integer mode") --------------
 * uint8 planar images [n,c,h,w], fixed-point taps, integer accumulation: the CPU restatement (oracle/imgproc_int_ref.py)
 * and these kernels agree bit for bit.  They shadow the reference's float ops (imgproc.py:1089-1121 filter2d_torch; the
 * F.interpolate call sites train_realesrnet.py:288,326-329,349-351,366-368), to which the distance is <= 1 LSB.
 * resr_filter2d_u8: taps_q14 = the kernel in Q14 (int32, [kh*kw] or [n][kh*kw] with per_sample), summing to 2^14:
 *   dst = clamp((sum q*src[reflect] + 2^13) >> 14, 0, 255).
 * resr_resize_u8: mode 0 area (integer window means, round half up; tables unused), 1 bilinear (2 taps), 2 bicubic
 *   (4 taps): per-axis tables idx_* [out][taps] (clamped source indices) and w_* [out][taps] (Q11, summing to 2^11),
 *   made by the caller from ATen's coordinate map; dst = clamp((sum_y wy * (sum_x wx*src) + 2^21) >> 22, 0, 255). */
int resr_filter2d_u8(const uint8_t* src, uint8_t* dst, const int32_t* taps_q14, int32_t n, int32_t c, int32_t h, int32_t w,
                     int32_t kh, int32_t kw, int32_t per_sample, void* stream);
int resr_resize_u8(const uint8_t* src, uint8_t* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t oh, int32_t ow,
                   int32_t mode, const int32_t* idx_y, const int32_t* w_y, const int32_t* idx_x, const int32_t* w_x, void* stream);
/* resr_jpeg_u8: DiffJPEG(differentiable=False).forward (imgproc.py:1462-1494) as an integer round trip on uint8 RGB
 *   [n,3,h,w]: zero padding to multiples of 16, RGB -> YCbCr and the 8x8 DCT with Q20 constants and int64 accumulation,
 *   quantiser steps rint(table * factor * 2^20) (the reference's transposed tables, imgproc.py:40-49; factor from the
 *   float32 quality[n] as imgproc.py:1134-1139, evaluated in float64 on the device), round-half-even division (torch.round),
 *   inverse DCT, nearest chroma upsampling, YCbCr -> RGB, clamp.  `coeffs` (nullable): the quantised coefficients, int32,
 *   per image [Y blocks row-major | Cb blocks | Cr blocks] x 64 over the padded size -- the same layout as resr_jpeg's.
 *   `quality` is read, never written (the reference mutates its argument in place; the Python mirror does that). */
int resr_jpeg_u8(const uint8_t* src, uint8_t* dst, const float* quality, int32_t* coeffs, int32_t n, int32_t h, int32_t w,
                 void* stream);

/* ---- device-resident training data source (device_data.py; the host side of dataset.py:66-143 as two launches) ------------
 * resr_tile_batch: dst[b] = the augmented fp32 CHW image of tile index[b] under code aug[b] -- tiles uint8 [M,T,T,3] (RGB, HWC),
 *   index int32 [B] and aug uint8 [B] on the device, dst fp32 [B,3,T,T].  Code: bits 0-1 = angle / 90 of the rotation about the
 *   integer centre (T / 2, T / 2) (imgproc._rotate_right_angle: an exact pixel permutation; with an even T a 90 / 180 / 270
 *   rotation loses one row / column and gains a zero one), bit 2 = horizontal flip, bit 3 = vertical flip, applied in that order;
 *   then value / 255.0f.  Bit for bit device_data.augment_np.  One launch; 90 / 270 are staged through an LDS tile, so reads and
 *   writes are both row-contiguous; 64-bit offsets throughout.  The kernel TRUSTS index (0 <= index[b] < M: the caller checks before
 *   upload) and reads aug's low four bits.  RESR_ERR_ARG before any launch: a null pointer, M, B or T < 1, B > 65535 or
 *   ceil(T / 32)^2 >= 2^31 (the grid).
 * resr_blur_kernels: n blur kernels of the degradation stage from n records, one workgroup each -- params float64
 *   [n][RESR_BLUR_RECORD] on the device, dst fp32 [n,K,K].  A record (doubles):
 *     [0] family   RESR_BLUR_GAUSSIAN / _GENERALIZED / _PLATEAU / _SINC / _DELTA
 *     [1] side     odd, 1 <= side <= K: the kernel is side x side, centred in the K x K output, zeros around it (delta: side 1)
 *     [2] sigma_x  [3] sigma_y  [4] theta   Gaussian families: cov = R(theta) diag(sigma_x^2, sigma_y^2) R(theta)^T ...
 *     [5] beta     generalized: exp(-q^beta / 2); plateau: 1 / (q^beta + 1); gaussian: exp(-q / 2); q = (x, y) cov^-1 (x, y)^T
 *     [6] aniso    ... when != 0, else cov = diag(sigma_x^2, sigma_x^2) (sigma_y, theta unused)
 *     [7] cutoff   sinc: cutoff * J1(cutoff r) / (2 pi r), the centre tap cutoff^2 / (4 pi)
 *   Taps in float64 (closed-form 2x2 inverse), summed in LDS in a fixed order (the same bits run to run), divided by the sum --
 *   twice for the Gaussian families, as imgproc.random_mixed_kernels does --, zero-padded to K, cast to fp32.  The definition is
 *   device_data.blur_kernels_from_params_np (numpy's summation order and LAPACK's inverse differ in the last float64 bits: an fp32
 *   tap may differ by one ulp).  A family or side outside this definition is refused by the caller before upload (the kernel
 *   clamps side into [1, K] and never leaves its tile).  RESR_ERR_ARG before any launch: a null pointer, n < 1, K even,
 *   K < 1 or K > RESR_BLUR_MAX_SIDE. */
#define RESR_BLUR_RECORD 8
#define RESR_BLUR_MAX_SIDE 31
enum { RESR_BLUR_GAUSSIAN = 0, RESR_BLUR_GENERALIZED = 1, RESR_BLUR_PLATEAU = 2, RESR_BLUR_SINC = 3, RESR_BLUR_DELTA = 4 };
int resr_tile_batch(const uint8_t* tiles, const int32_t* index, const uint8_t* aug, int32_t m, int32_t b, int32_t t, float* dst,
                    void* stream);
int resr_blur_kernels(const double* params, int32_t n, int32_t k, float* dst, void* stream);

/* ---- paired training data source (device_data.PairedDeviceSource): LR / HR pairs resident as uint8, one launch a batch ------------
 * resr_pair_batch: for sample b with records[b] = (image, top, left, code): lr_dst[b] = the LR crop [top, top + patch) x [left, left + patch)
 *   of image's LR side, hr_dst[b] = the HR crop [scale * top, scale * top + scale * patch) x [scale * left, ...) of its HR side, both
 *   under the same dihedral code -- bit 0 = horizontal flip, bit 1 = vertical flip, bit 2 = transpose, applied in that order -- then
 *   value / 255.0f, HWC -> CHW.  Bit for bit device_data.paired_sample_np.
 *   hr_arena / lr_arena: the images of each side back to back, HWC RGB bytes, any size, sizes differing from image to image; table int64
 *   [m,4] = (hr_offset, lr_offset, lr_h, lr_w) in bytes / pixels, image i's HR side being (scale * lr_h, scale * lr_w); records int32
 *   [b,4]; lr_dst fp32 [b,3,patch,patch], hr_dst fp32 [b,3,scale * patch,scale * patch]; everything on the device.
 *   ONE launch writes both outputs (a workgroup owns one 32 x 32 tile of one output image, staged through LDS so that reads and
 *   writes are both row-contiguous); 64-bit offsets throughout, byte loads (a row starts at any address).  The kernel clamps image into
 *   0..m-1, top / left into the image and code to 3 bits: a wrong record gives wrong values, never an access outside the arenas; the
 *   caller refuses such records before upload (device_data.check_paired_records).  The table is trusted.
 *   RESR_ERR_ARG before any launch: a null pointer, m, b or patch < 1, scale outside 1..4, b > 65535, scale * patch > 2^31 - 1, or
 *   ceil(patch / 32)^2 + ceil(scale * patch / 32)^2 >= 2^31 (the grid). */
int resr_pair_batch(const uint8_t* hr_arena, const uint8_t* lr_arena, const int64_t* table, const int32_t* records, int32_t m, int32_t b,
                    int32_t patch, int32_t scale, float* lr_dst, float* hr_dst, void* stream);

/* ---- whole-image training data source (device_data.ImageCropSource): images of any size resident as uint8, the crop in the launch ----
 * resr_crop_batch: for sample b with records[b] = (image, top, left, code): dst[b] = the t x t window of that image at (top, left) under
 *   resr_tile_batch's 16 codes (bits 0-1 = angle / 90 about the integer centre with its zero row / column at an even t, bit 2 =
 *   horizontal flip, bit 3 = vertical flip), then value / 255.0f, HWC -> CHW.  The window is
 *     win[y][x] = image[reflect101(top + y, h)][reflect101(left + x, w)],   reflect101(i, n) = 0 for n = 1, else with p = 2n - 2 and
 *     j = i mod p: j below n, else p - j
 *   -- an image below t in an axis continues below / to the right by reflection about its last pixel, for a pad of any width.  Bit for bit
 *   device_data.crop_sample_np.
 *   arena: the images back to back, HWC RGB bytes, any size (h, w below 2^31), starting at any byte; table int64 [m,3] = (offset in bytes,
 *   h, w); records int32 [b,4]; dst fp32 [b,3,t,t]; everything on the device.  ONE launch (a workgroup owns one 32 x 32 tile of one
 *   sample, staged through LDS so that reads and writes are both row-contiguous; a staged block inside the image is read row by row, one
 *   that reaches the padding pixel by pixel through reflect101); 64-bit offsets throughout, byte loads.  The kernel clamps image into
 *   0..m-1, top into 0..max(h, t) - t, left into 0..max(w, t) - t and reads the code's low four bits: a wrong record gives wrong values,
 *   never an access outside the image; the caller refuses such records before upload (device_data.check_crop_records).  The table is
 *   trusted.  Profiling id 33003.
 *   RESR_ERR_ARG before any launch: a null pointer, m, b or t < 1, b > 65535, or ceil(t / 32)^2 >= 2^31 (the grid). */
int resr_crop_batch(const uint8_t* arena, const int64_t* table, const int32_t* records, int32_t m, int32_t b, int32_t t, float* dst,
                    void* stream);

/* ---- multi-scale copies of the whole-image source (device_data.ImageCropSource, scales / short_side): Pillow's 8-bit LANCZOS resize ----
 * The rule (device_data.resample_tables_np / resample_u8_np are the definition; they are checked against Pillow itself): per axis a table
 * of `out` rows, row xx = (xmin, count) and ksize Q22 integer coefficients, ksize = ceil(3 * max(in / out, 1)) * 2 + 1; a pass gives
 * clip((2^21 + sum_k pixel[xmin + k] * coeff[k]) >> 22, 0, 255) with an int32 sum; the horizontal pass is stored as bytes before the vertical
 * pass; a pass over an axis whose size does not change is skipped.
 * resr_resample_ksize: the row length of in_size -> out_size, or RESR_ERR_ARG for a size outside 1..2^31 - 1.  Host only.
 * resr_resample_tables: bounds int32 [out_size,2] and coeffs int32 [out_size,ksize_capacity] (a row's ksize coefficients, zeros behind them)
 *   of in_size -> out_size, HOST memory; plain host arithmetic in double with libm's sin and no contraction, no GPU call.  RESR_ERR_ARG: a
 *   size outside 1..2^31 - 1, a null pointer, ksize_capacity below resr_resample_ksize, and a row with 255 * sum|coeff| + 2^21 >= 2^31 (the
 *   int32 sum could overflow; never the case for this filter).
 * resr_resample_u8: j jobs in ONE launch, each one HWC RGB uint8 image of `arena` resampled into another place of the same arena.  A job is 8
 *   int64: (source offset, h, w, destination offset, oh, ow, row table, column table) -- offsets in bytes, the tables as word offsets into
 *   `tables` (int32 [table_words], device): at a table's offset `out` pairs (xmin, count), then `out` rows of resr_resample_ksize(in, out)
 *   coefficients, the row table for h -> oh, the column table for w -> ow; the table of an unchanged axis is not read.  The jobs are passed
 *   twice: jobs_host (host memory, read by the checks below) and jobs_dev (the same 8 * j words on the device, read by the kernel).  Bit for
 *   bit device_data.resample_u8_np.  A workgroup owns a 64 x 16 tile of one output, stages source rows in LDS (consecutive lanes on consecutive
 *   bytes), keeps the horizontal pass's bytes in LDS and stores whole aligned dwords wherever a row starts; int32 multiply-adds; no
 *   temporary buffer.  Images start at any byte; 64-bit offsets throughout.  The kernel clamps every xmin into 0..in - 1 and every count into
 *   0..min(ksize, in - xmin): a wrong table gives wrong values, never a read outside the image.  Profiling id 33004, its record's bytes the
 *   source plus destination bytes of the jobs.
 *   RESR_ERR_ARG before any launch: a null pointer; j < 1 or j > 65535; arena_bytes < 1; a side below 1 or at or above 2^31; ksize of a changed
 *   axis outside 1..4096; a table that leaves `tables`; a source or destination that leaves the arena; a destination that shares a byte with a
 *   source or another destination of the call ("overlapping source and destination"); more than 2^31 - 1 tiles in a job. */
int resr_resample_ksize(int64_t in_size, int64_t out_size);
int resr_resample_tables(int64_t in_size, int64_t out_size, int32_t* bounds, int32_t* coeffs, int32_t ksize_capacity);
int resr_resample_u8(uint8_t* arena, int64_t arena_bytes, const int64_t* jobs_host, const int64_t* jobs_dev, int32_t j, const int32_t* tables, int64_t table_words,
                     void* stream);

/* ---- training pair pool (device_data.PairPool): a resident queue of finished LR / HR pairs, one exchange launch a step ------------
 * resr_pool_exchange: for sample i < b with slot = slots[i]: lr_out[i] = pool_lr[slot], then pool_lr[slot] = lr_in[i]; the same for hr.
 *   pool_lr fp32 [q, lr_elems], pool_hr fp32 [q, hr_elems]; lr_in / lr_out fp32 [b, lr_elems], hr_in / hr_out fp32 [b, hr_elems]; slots int32
 *   [b]; everything on the device.  Bit for bit device_data.pool_exchange_np: the payload moves as 32-bit words, never as floats, so NaN
 *   payloads and subnormals keep their bits; there is no arithmetic.
 *   ONE launch moves both tensors (grid.y the sample, grid.x the 16 KiB chunks of its LR and then of its HR side; a thread issues all
 *   its loads before its stores).  16-byte loads and stores on a side whose sample size is a multiple of 4 floats and whose pool, input
 *   and output base pointers are 16-byte aligned; word by word otherwise, the same result.  64-bit offsets throughout.
 *   lr_out = hr_out = NULL: the stores only (device_data.pool_store_np, the fill of the pool); the pool is then not read.
 *   An output may be exactly its input (lr_out == lr_in: the swap in place).  The slots of a call must differ from each other; the
 *   kernel clamps a slot into 0..q-1: a wrong slot gives wrong values, never an access outside the pool, and the caller refuses such
 *   slots before upload (device_data.check_pool_slots).
 *   RESR_ERR_ARG before any launch: a null pointer (exactly one null output included), q, b, lr_elems or hr_elems < 1, b > q, b > 65535,
 *   ceil(lr_elems / 4096) + ceil(hr_elems / 4096) >= 2^31 (the grid), or, on either side, an overlap among the pool, the input and the
 *   output other than output == input. */
int resr_pool_exchange(float* pool_lr, float* pool_hr, const float* lr_in, const float* hr_in, float* lr_out, float* hr_out, const int32_t* slots,
                       int32_t q, int32_t b, int64_t lr_elems, int64_t hr_elems, void* stream);

/* ---- native NIQE (image_quality_assessment.niqe_native; csrc/niqe.hip): the metric up to its 36 features per block ---------
 * The tail of the score (NaN-aware mean, covariance, pinv, distance) is torch's, or resr_niqe_score's below.  float64 wherever the
 * torch path is float64.
 * resr_niqe_luma_f32 / _u8: src fp32 [n,3,h,w] in [0,1] / uint8 [n,h,w,3] (a byte enters as (float)byte / 255.0f) -> dst uint8
 *   [n,out_h,out_w]: the luma level of source pixel (crop + y, crop + x) -- crop_border and the trim to whole blocks fused into the
 *   read.  level = rint(t) (half to even, pinned into 0..255) of the fp32 chain, every operation rounded once, no contraction:
 *     t = r * 65.481f;  t = t + g * 128.553f;  t = t + b * 24.966f;  t = t + 16.0f
 *   (tests/niqe_ref.niqe_luma_np is the same chain in numpy).  One launch, profiling ids 34000 (fp32) / 34001 (uint8).
 *   RESR_ERR_ARG before any launch: a null pointer, n, h, w, out_h or out_w < 1, crop < 0, 2 crop + out_h > h or 2 crop + out_w > w,
 *   n or out_h above 65535.
 * resr_niqe_features: luma uint8 [n,h,w] -> feats float64 [n, blocks, 36], block (by, bx) at row by * (w / bw) + bx; columns
 *   0..17 are scale 1, 18..35 scale 2, each in the order of _block_features.  Four launches:
 *     34100  the half-size image imresize(y / 255, 0.5) * 255 in float64, H pass then W pass, from the banded tables below;
 *     34200 / 34201  MSCN + block moments at scale 1 (from the levels) / scale 2 (from the half-size image), one workgroup per block:
 *            mu and E[y^2] by the 49 taps of `win` with replicate padding at the IMAGE edge, sigma = sqrt(|E[y^2] - mu^2| + 1e-8),
 *            (y - mu) / (sigma + 1) kept in LDS only, and for each of five maps (the block; its products with the copies rolled by
 *            (0,1), (1,0), (1,1), (1,-1) inside the block) six float64 words: negatives, positives, sum of squares over the
 *            negatives, over the positives, sum of magnitudes, sum of squares -- summed in a fixed order: the same bits every call;
 *     34300  the AGGD fit of every (block, map): the first minimum of |r_gam[i] - rhat_norm| over the grid, then the features.
 *   Descriptor: n, h, w the luma batch and size (h, w multiples of bh, bw); bh, bw even; the tables on the device:
 *     start_h int32 [h / 2], w_h float64 [h / 2][taps_h]: output row i = sum_k w_h[i][k] * src[start_h[i] + k], k ascending (the
 *     non-zero band of imgproc._resize_matrix(h, h / 2, 0.5, True, float64)); start_w / w_w the same for the columns; a start that
 *     would leave the axis is pinned into it (undefined values, never undefined accesses); taps at most 16.
 *     grid / r_gam float64 [n_grid]: the shape grid and its ratio table, as _aggd computes them.  win: _gaussian_window() as float64.
 *   workspace: resr_niqe_workspace_bytes(d) bytes, 8-byte aligned, laid out [half-size image float64 [n, h / 2, w / 2], padded to
 *     256 bytes | moments float64 [2 scales][n * blocks][5][6]]; it needs no initialisation and holds these after the call (tests
 *     read them).  The query returns 0 for a descriptor the entry refuses (pointers and tables aside).
 *   RESR_ERR_ARG before any launch: a null pointer, a bad size, odd or non-dividing blocks, a block whose LDS tile (MSCN block in
 *   float64 + halo tile + 1920 bytes) exceeds 160 KiB at either scale, taps outside 1..16 or above the axis, misaligned workspace /
 *   feats; RESR_ERR_WORKSPACE: workspace_bytes too small. */
typedef struct {
    int32_t n, h, w;
    int32_t bh, bw;
    int32_t taps_h, taps_w;
    int32_t n_grid;
    const int32_t* start_h;
    const double* w_h;
    const int32_t* start_w;
    const double* w_w;
    const double* grid;
    const double* r_gam;
    void* workspace;
    size_t workspace_bytes;
    double win[49];
} ResrNiqeDesc;
int resr_niqe_luma_f32(const float* src, uint8_t* dst, int32_t n, int32_t h, int32_t w, int32_t crop, int32_t out_h, int32_t out_w,
                       void* stream);
int resr_niqe_luma_u8(const uint8_t* src, uint8_t* dst, int32_t n, int32_t h, int32_t w, int32_t crop, int32_t out_h, int32_t out_w,
                      void* stream);
size_t resr_niqe_workspace_bytes(const ResrNiqeDesc* d);
int resr_niqe_features(const ResrNiqeDesc* d, const uint8_t* luma, double* feats, void* stream);

/* ---- native NIQE tail (image_quality_assessment.niqe_score_native; csrc/niqe.hip): features -> score, batched, on the device --------
 * resr_niqe_score: feats float64 [n, blocks, 36] (the layout resr_niqe_features writes: the two chain with no copy) -> scores
 *   float64 [n], the tail of image_quality_assessment._score_from_features in float64 throughout.  Two launches whatever n is, one
 *   workgroup per image each (1024 threads, then 256); no host synchronisation, no allocation, no read-back.  Per image:
 *   34400  mean, covariance, A.
 *     mu_d[c] = (sum of the non-NaN entries of column c) / (their count); 0 / 0 = NaN for a column of NaNs.
 *     ok = the rows without a NaN, m of them.  Two passes: mean_ok[c] = sum over ok / m, then cov_d[i][j] = (sum over ok of
 *     (x[r][i] - mean_ok[i]) * (x[r][j] - mean_ok[j])) / (m - 1) -- so m = 1 gives 0 / 0 = NaN and m = 0 gives -0, as the torch tail.
 *     A = (cov_prior + cov_d) / 2.  Only i <= j is computed; A[j][i] is a copy of A[i][j]: A is exactly symmetric.
 *     Order of every sum (the same bits on every call): a wave takes whole rows, lane c column c.  A column sum is held by 16
 *     threads, one per wave: wave w adds rows w, w + 16, ... in ascending order, and the 16 partial sums are then added in ascending
 *     w.  A covariance sum is held by 5 threads (which own A[i][4k .. 4k + 3]): the centred rows pass through LDS 112 at a time,
 *     thread g adds rows g, g + 5, ... of chunk after chunk in ascending order, each term one fused multiply-add, and the 5 partial
 *     sums are then added in ascending g; a row that is not ok enters as an exact zero.
 *   34500  eigen-decomposition, cut, score.
 *     A with an entry that is not finite: the eigenvalues are NaN, the kept count 0, the score NaN.  Otherwise cyclic Jacobi on A
 *     in LDS (leading dimension 37, so that column walks meet no bank twice), the eigenvectors accumulated from the identity.
 *     Ordering: round robin, 35 steps per sweep, 18 disjoint pairs per step, rotated at once: in step s (0 .. 34) pair 0 is 35 with s
 *     and pair k = 1 .. 17 is (s + k) mod 35 with (s - k) mod 35; p is the smaller index of a pair, q the larger.
 *     Rotation of (p, q): none (c = 1, s = 0, t = 0) when a_pq^2 <= 2^-106 |a_pp a_qq| -- that is a_pq == 0, or |a_pq| <=
 *     2^-53 sqrt(|a_pp a_qq|) -- otherwise, with d = a_qq - a_pp and h = 2 a_pq,
 *       t = h / (d + sign(d) sqrt(d^2 + h^2))   (= sign(theta) / (|theta| + sqrt(theta^2 + 1)) for theta = d / h; sign(0) = +1),
 *       c = rsqrt(t^2 + 1) (the device library's reciprocal square root), s = t c, and none after all if s == 0.
 *     The step's J^T A J, every x y +- z w one multiplication and one fused multiply-add: in the pair's own block a_pp -= t a_pq,
 *     a_qq += t a_pq, a_pq = 0 (a_pq stays when there is no rotation); in the block of pairs k1 < k2 first the columns by pair k2,
 *       u[i][p2] = c2 a[i][p2] - s2 a[i][q2], u[i][q2] = s2 a[i][p2] + c2 a[i][q2]   for i = p1, q1,
 *     then the rows by pair k1, a'[p1][j] = c1 u[p1][j] - s1 u[q1][j], a'[q1][j] = s1 u[p1][j] + c1 u[q1][j] for j = p2, q2; a'[j][i]
 *     is a copy of a'[i][j].  Eigenvectors: v[r][p] = c v[r][p] - s v[r][q], v[r][q] = s v[r][p] + c v[r][q].
 *     The loop ends after the first sweep that applied no rotation, and is capped at 30 sweeps: a matrix still rotating then
 *     scores NaN (its eigenvalues as they stand are stored).
 *     Cut (torch.linalg.pinv's default): eigenvalue k is kept iff |lambda_k| > 36 * 2^-52 * max |lambda|.
 *     score = sqrt(sum over kept k, ascending, of (v_k . diff)^2 / lambda_k), diff = mu_prior - mu_d, each dot product summed in
 *     ascending row order by one thread; a negative sum gives NaN.
 *   workspace: resr_niqe_score_workspace_bytes(d) = n * (36 + 1296 + 36 + 1) * 8 bytes, 8-byte aligned, all float64, laid out
 *     [mu_d [n][36] | A [n][36][36] | eigenvalues [n][36], in the order the sweeps leave them on the diagonal | kept count [n], stored
 *     as a double]; it needs no initialisation and holds these after the call (tests read them).  The query needs no device and
 *     returns 0, with the reason in resr_last_error(), for a descriptor whose sizes the entry refuses.
 *   RESR_ERR_ARG before any launch, "niqe_score" in resr_last_error(): a null descriptor or pointer (feats, scores, mu_prior,
 *   cov_prior, workspace), n < 1, blocks < 1, blocks * 36 above 2^31 - 1 (offsets inside an image are int32), a workspace smaller
 *   than the query's answer, a pointer that is not 8-byte aligned. */
typedef struct {
    int32_t n, blocks;
    const double* mu_prior;    /* [36] */
    const double* cov_prior;   /* [36][36], row-major */
    void* workspace;
    size_t workspace_bytes;
} ResrNiqeScoreDesc;
size_t resr_niqe_score_workspace_bytes(const ResrNiqeScoreDesc* d);
int resr_niqe_score(const ResrNiqeScoreDesc* d, const double* feats, double* scores, void* stream);

/* ---- native PSNR / SSIM (image_quality_assessment.full_ref_native; csrc/fullref.hip): sr against its ground truth, on the device ----
 * resr_fullref: sr and hr, each fp32 [n,3,h,w] in [0,1] (sr_u8 / hr_u8 = 0) or uint8 [n,h,w,3] (= 1), independently -> per image
 *   sse int64 [n], psnr float64 [n], ssim float64 [n] of the Y channel.  Two launches whatever n is, no host synchronisation, no
 *   float64 map in memory.  crop >= 0 pixels leave on every side of both images; the rest, hc x wc = (h - 2 crop) x (w - 2 crop), must
 *   be at least 11 x 11.
 *   Levels: X (sr) and Y (hr) are the luma levels of resr_niqe_luma_* above (the same device function; a byte enters as
 *     (float)byte / 255.0f), uint8 in 0..255.
 *   PSNR: sse = sum of (X - Y)^2 over the hc * wc pixels, an exact integer; psnr = 10 * log10(65025 / (sse / (hc * wc) + 1e-8)) in
 *     float64, each operation rounded once (identical images: 128.13 dB).
 *   SSIM: k[i] = exp(-(i - 5)^2 / 4.5), i = 0 .. 10, divided by their sum (added for i ascending), float64, made by the host's libm.
 *     The map has (hc - 10) x (wc - 10) values; with x, y the levels as float64, at map position (r, c) the five window sums
 *       S_v = sum_b k[b] * (sum_a k[a] * v(r + a, c + b)),   v = x, y, x * x, y * y, x * y (exact integers),
 *     are taken in ONE order: the inner (H) sum over a ascending and then the outer (W) sum over b ascending, each from 0.0 with one
 *     fused multiply-add per tap.  Then, every operation rounded once and none fused,
 *       m11 = S_x * S_x, m22 = S_y * S_y, m12 = S_x * S_y;  s11 = S_xx - m11, s22 = S_yy - m22, s12 = S_xy - m12;
 *       value = ((2 * m12 + 6.5025) * (2 * s12 + 58.5225)) / (((m11 + m22) + 6.5025) * ((s11 + s22) + 58.5225)),
 *     so that sr == hr gives value == 1.0, and ssim == 1.0, exactly.
 *   34600 + sr_u8 + 2 hr_u8  fullref_tile_kernel: one workgroup of 256 threads per RESR_FULLREF_TILE x RESR_FULLREF_TILE tile of the
 *     map of one image, tile (ty, tx) at index ty * tiles_x + tx, tiles_x = ceil((wc - 10) / 32), tiles_y = ceil((hc - 10) / 32).
 *     Its map sum: thread t adds its values (t / 8, 4 (t % 8) + q) of the tile for q = 0 .. 3 ascending (a position outside the map
 *     is +0.0); the 64 lanes of a wave meet in the butterfly v += shuffle_xor(v, 32), 16, 8, 4, 2, 1; the four wave sums are added in
 *     ascending order.  Its sse: the pixels (r, c) of the cropped image with r / 32 == ty, or r >= 32 tiles_y for the last tile row, and
 *     the same for the columns: every pixel belongs to exactly one tile.
 *   34700  fullref_finish_kernel: one workgroup of RESR_FULLREF_FINISH_THREADS threads per image.  Thread t adds the map sums of tiles
 *     t, t + 256, ... in ascending order from 0.0; lanes meet in the same butterfly, the wave sums are added in ascending order;
 *     ssim = sum / ((hc - 10) * (wc - 10)).  The sse partials are added as integers.  The same input gives the same bits on every call.
 *   workspace: resr_fullref_workspace_bytes(d) = n * tiles_y * tiles_x * 16 bytes, 8-byte aligned: per image and tile [sse uint64 |
 *     map sum float64]; it needs no initialisation and holds these after the call (tests read them).  The query needs no device and
 *     returns 0, with the reason in resr_last_error(), for a descriptor whose sizes the entry refuses.
 *   RESR_ERR_ARG before any launch, "fullref" in resr_last_error(): a null descriptor or pointer (sr, hr, sse, psnr, ssim, workspace),
 *   n, h or w < 1, crop < 0, a crop that leaves less than 11 x 11, n * tiles_y * tiles_x above 2^31 - 1 (the launch's tile index is
 *   int32; every offset into the images is 64-bit), a workspace smaller than the query's answer, an output or workspace pointer that
 *   is not 8-byte aligned, a float image that is not 4-byte aligned (uint8 images need no alignment at any width).
 *   Not built: MS-SSIM, padding modes, windows other than 11 taps / sigma 1.5.  (RGB channels, 16-bit images and the planes of YUV
 *   frames: resr_fullref_planes below.) */
#define RESR_FULLREF_TILE 32
#define RESR_FULLREF_FINISH_THREADS 256
typedef struct {
    int32_t n, h, w;           /* the images as stored, before the crop */
    int32_t crop;
    int32_t sr_u8, hr_u8;
    void* workspace;
    size_t workspace_bytes;
} ResrFullRefDesc;
size_t resr_fullref_workspace_bytes(const ResrFullRefDesc* d);
int resr_fullref(const ResrFullRefDesc* d, const void* sr, const void* hr, int64_t* sse, double* psnr, double* ssim, void* stream);

/* ---- native PSNR / SSIM per plane (image_quality_assessment.full_ref_channels_native / full_ref_yuv_native; csrc/fullref.hip) ----
 * resr_fullref_planes: `planes` planes of h x w integer levels 0 .. peak in each of n images, on both sides -> sse int64, psnr float64,
 *   ssim float64, each [n][planes].  Two launches whatever n and planes are, no host synchronisation.  peak is 255, 1023 or 65535, one
 *   value per call.  crop as in resr_fullref: (h - 2 crop) x (w - 2 crop) = hc x wc, at least 11 x 11, is scored.
 *   A level comes out of a VIEW of the caller's memory, one view per side (the sr_ and hr_ fields), all strides and the base in WORDS:
 *     word(i, p, y, x) = memory[base + i * image_stride + p * plane_stride + y * row_stride + x * pixel_stride],
 *     word_bytes 1 or 2: an unsigned integer, level = (word >> shift) & mask;
 *     word_bytes 4: an fp32 value v, level = trunc(clamp(v * peak, 0, peak)) in fp32, a NaN gives 0 (the rule of every uint8 / uint16
 *       tail of this library); shift and mask are not used.
 *     Interleaved uint8 / uint16 pixels [n,h,w,C]: pixel C, row w C, plane 1, image h w C.  fp32 planes [n,C,h,w]: pixel 1, row w, plane
 *     h w, image C h w.  The chroma of a 4:2:0 frame of H x W luma: base H W, and planar pixel 1, row W / 2, plane H W / 4, or semi-planar
 *     pixel 2, row W, plane 1, with h = H / 2, w = W / 2.  10-bit words: mask 1023, shift 0 (low bits) or 6 (P010).
 *     The two sides may use different views.  THE KERNEL TRUSTS the strides and the base, as resr_tile_batch trusts its indices: every
 *     word a view names for 0 <= i < n, p < planes, y < h, x < w must lie inside the caller's allocation.  The Python layer builds
 *     views only from tensors whose shape it has checked.  Every offset is 64-bit; loads are byte, word or dword loads of one sample,
 *     and nothing is assumed aligned beyond the word itself.
 *   PSNR and SSIM are resr_fullref's, term for term, of the levels X (sr) and Y (hr), with 65025 replaced by peak * peak and
 *     C1 = (peak * peak) / 10000.0, C2 = (9 * peak * peak) / 10000.0, each ONE float64 division of exact integers (for peak 255 these are
 *     the bits of 6.5025 and 58.5225): the same window, H pass, W pass, unfused map expression, tile and finish orders; the same
 *     code.  A one-plane view of the uint8 luma levels of an RGB pair gives the bits of resr_fullref on the pair.  X == Y gives
 *     ssim == 1.0 exactly.  The thread-private squared differences are summed in 64 bits (seven of 65535^2 overflow 32).
 *   34604  fullref_planes_tile_kernel: workgroup (image * planes + plane) * tiles + tile; levels lie in LDS as 16-bit words
 *     (2 * 42 * 44 * 2 bytes; 61,216 bytes in all, two workgroups per CU as before).
 *   34701  fullref_finish_kernel (the same kernel, peak * peak an argument): one workgroup per (image, plane).
 *   workspace: resr_fullref_planes_workspace_bytes(d) = n * planes * tiles_y * tiles_x * 16 bytes, 8-byte aligned, [image][plane][tile]
 *     [sse uint64 | map sum float64] as resr_fullref's; no initialisation needed, readable after the call.  The query needs no device,
 *     ignores the workspace fields, and returns 0 with the reason in resr_last_error() for a descriptor the entry refuses.
 *   RESR_ERR_ARG before any launch, "fullref_planes" in resr_last_error(): a null descriptor or pointer; n, planes, h or w < 1;
 *   planes > 4; crop < 0; a peak other than 255, 1023, 65535; word_bytes not 1, 2 or 4; a mask above the peak or below 0; a shift
 *   outside 0 .. 15; a pixel or row stride < 1; a negative plane or image stride or base; a crop that leaves less than 11 x 11;
 *   n * planes * tiles above 2^31 - 1; a workspace smaller than the query's answer; a workspace or output pointer not 8-byte aligned;
 *   sr or hr not aligned to its word. */
typedef struct {
    int32_t n, planes, h, w;   /* the planes as stored, before the crop */
    int32_t crop, peak;
    int32_t sr_word_bytes, sr_shift, sr_mask;
    int32_t hr_word_bytes, hr_shift, hr_mask;
    int64_t sr_base, sr_pixel_stride, sr_row_stride, sr_plane_stride, sr_image_stride;
    int64_t hr_base, hr_pixel_stride, hr_row_stride, hr_plane_stride, hr_image_stride;
    void* workspace;
    size_t workspace_bytes;
} ResrFullRefPlanesDesc;
size_t resr_fullref_planes_workspace_bytes(const ResrFullRefPlanesDesc* d);
int resr_fullref_planes(const ResrFullRefPlanesDesc* d, const void* sr, const void* hr, int64_t* sse, double* psnr, double* ssim,
                        void* stream);

/* ---- JPEG encode (jpeg_encode.encode_jpeg; csrc/jpeg_encode.hip): finished frames leave the device as baseline JPEG files ----
 * resr_jpeg_encode: uint8 [n,h,w,3] RGB frames on the device -> n complete JFIF files (sequential DCT, 8 bits, YCbCr, Huffman) in device
 *   memory, file i at out + i * out_stride, and lengths int64 [n].  Three launches whatever n is, all on `stream`, no host synchronisation,
 *   no allocation, no host read of device data (safe under graph capture).  The bytes are a definition of this library's, stated rule by
 *   rule in DESIGN "JPEG encode" (colour in Q16 with one rounding; 4:2:0 as the colour rule on the exact 2x2 sums of R, G, B; edge
 *   replication up to the MCU; an exact integer 8x8 DCT with a Q20 matrix, rounded once to Q13; the Annex K tables scaled by the IJG
 *   quality rule, division half away from zero; the Annex K Huffman tables; restart segments): not libjpeg's bytes, and not the DiffJPEG
 *   round trip of resr_jpeg_u8 above (non-integer steps, transposed tables: a degradation, not a file format).
 *   subsampling: RESR_JPEG_444 (MCU 8x8) or RESR_JPEG_420 (MCU 16x16).  quality 1..100.  restart_interval: MCUs per restart segment,
 *   1..65535, 0 = RESR_JPEG_DEFAULT_INTERVAL; every file has a DRI segment and RSTm markers: the segments are what is encoded in
 *   parallel (one wave each).
 *   resr_jpeg_encode_header: HOST only, no GPU call: SOI APP0 DQT SOF0 DHT DRI SOS of the descriptor into host_buf (cap bytes); returns
 *     its length (RESR_JPEG_HEADER_BYTES; host_buf NULL: the length alone) or RESR_ERR_ARG.  The caller uploads it once per geometry and
 *     passes it as header_dev / header_len; a header_len that is not the descriptor's is refused.
 *   Overflow: out_stride is the caller's capacity per file and may be far below max_bytes.  A file that needs more gets lengths[i] =
 *     -(bytes it needs) and NOT ONE byte of its slot is written; the other files of the batch are unaffected.  No byte at or past
 *     out + (i + 1) * out_stride is ever written for file i.
 *   resr_jpeg_encode_max_bytes: a bound no file of this geometry exceeds.  A block costs at most 22 bits for its DC symbol (the longest
 *     code + size pair of the DC tables: 11 + 11, chroma) and 26 bits (16 + 10) for each of its 63 AC positions (a ZRL of at most 11 bits
 *     stands for 16 positions, the EOB for at least one): 1660 bits.  A segment of B blocks is at most ceil(1660 B / 8) bytes, its padded
 *     last byte included; 0xFF stuffing at most doubles it; every segment is followed by two marker bytes (RSTm or EOI).
 *     max_bytes = RESR_JPEG_HEADER_BYTES + segments * (round16(2 * ceil(1660 B / 8)) + 2): about 6.5 times the raw frame at 4:4:4, 3.2 at 4:2:0.
 *   workspace: resr_jpeg_encode_workspace_bytes(d) bytes, 8-byte aligned: [segment length int32 x S | pad to 8][segment offset int64 x S]
 *     [S slots of the segment bound], S = n * segments per frame.  Only the workspace has worst-case room; it needs no initialisation.
 *   35000 + (4:2:0)  jpeg_segment_kernel: one wave per segment: colour, DCT, quantisation and entropy coding; the coefficients stay in
 *     registers; stuffed bytes go to the segment's slot.   35100  jpeg_scan_kernel: one workgroup per frame: segment offsets, the
 *     length, the overflow verdict.   35200  jpeg_copy_kernel: one wave per segment: header, segment, marker into the file.
 *   The size queries need no device and return 0, with the reason in resr_last_error(), for a descriptor the entry refuses.
 *   RESR_ERR_ARG before any launch, "jpeg_encode" in resr_last_error(): a null descriptor or pointer; n, h or w < 1; h or w > 65535 (the
 *   SOF0 fields); quality outside 1..100; an unknown subsampling; a restart interval below 0 or above 65535; n * segments above
 *   2^31 - 1; a negative out_stride; a header_len other than the descriptor's; a workspace below the query's answer; a workspace or
 *   lengths pointer that is not 8-byte aligned.  rgb_hwc and out need no alignment (byte loads and stores), out_stride may be odd.
 *   Not built: progressive or arithmetic coding, optimised Huffman tables, 4:2:2, grey or CMYK files, EXIF / ICC, YUV frame formats as
 *   the source, byte equality with libjpeg. */
#define RESR_JPEG_444 0
#define RESR_JPEG_420 1
#define RESR_JPEG_DEFAULT_INTERVAL 8
#define RESR_JPEG_HEADER_BYTES 613
typedef struct {
    int32_t n, h, w;
    int32_t subsampling;          /* RESR_JPEG_444 / RESR_JPEG_420 */
    int32_t quality;              /* 1..100 */
    int32_t restart_interval;     /* MCUs per segment; 0 = RESR_JPEG_DEFAULT_INTERVAL */
} ResrJpegEncDesc;
size_t resr_jpeg_encode_max_bytes(const ResrJpegEncDesc* d);
size_t resr_jpeg_encode_workspace_bytes(const ResrJpegEncDesc* d);
int resr_jpeg_encode_header(const ResrJpegEncDesc* d, uint8_t* host_buf, size_t cap);
int resr_jpeg_encode(const ResrJpegEncDesc* d, const uint8_t* rgb_hwc, uint8_t* out, int64_t out_stride, int64_t* lengths,
                     const uint8_t* header_dev, int32_t header_len, void* workspace, size_t workspace_bytes, void* stream);

/* ---- PNG encode (png_encode.encode_png; csrc/png_encode.hip): finished images leave the device as PNG files, lossless ----
 * resr_png_encode: uint8 or uint16 [n,h,w,channels] images on the device (channels 1, 3, 4: PNG colour types 0, 2, 6; bit_depth 8 or 16,
 *   the samples in the device's own byte order) -> n complete PNG files in device memory, file i at out + i * out_stride, and lengths
 *   int64 [n].  Four launches whatever n is, all on `stream`, no host synchronisation, no allocation, no host read of device data (safe
 *   under graph capture).  The bytes are a definition of this library's, stated rule by rule in DESIGN "PNG encode" (numpy form:
 *   tests/png_encode_ref.py): per row the filter of libpng's heuristic (smallest sum of |int8|, ties to the lowest type); the filtered
 *   stream F, T = h (1 + w bpp) bytes, cut into segments of segment_bytes (64..65535, 0 = RESR_PNG_DEFAULT_SEGMENT_BYTES); per segment
 *   one deflate block of literals and distance-1 matches (zlib's Z_RLE) with its own length-limited Huffman codes, or a stored block
 *   where that is not smaller; every segment but the last is followed by an empty stored block (the Z_SYNC_FLUSH marker), so every
 *   segment is whole bytes; one IDAT chunk per segment with its own CRC-32; a last IDAT with the Adler-32 of F; IEND.  Any reader accepts
 *   the files; they are not libpng's bytes.
 *   resr_png_encode_header: HOST only, no GPU call: the signature, IHDR and an IDAT holding the zlib header 78 01 into host_buf (cap
 *     bytes); returns its length (RESR_PNG_HEADER_BYTES for every geometry; host_buf NULL: the length alone) or RESR_ERR_ARG.  The caller
 *     uploads it once per geometry and passes it as header_dev / header_bytes.
 *   Overflow: out_stride is the caller's capacity per file and may be below max_bytes.  A file that needs more gets lengths[i] = -(bytes
 *     it needs) and NOT ONE byte of its slot is written; the other files of the batch are unaffected.  No byte at or past
 *     out + (i + 1) * out_stride is ever written for file i.
 *   resr_png_encode_max_bytes: T + 17 K + 75 for K = ceil(T / segment_bytes) segments: a stored block is 5 + its bytes and no block is
 *     longer, 12 bytes frame a chunk, 47 + 28 bytes are the header and the two last chunks.
 *   workspace: resr_png_encode_workspace_bytes(d) bytes, 16-byte aligned, no initialisation needed: per segment its length, offset, CRC
 *     and Adler partials, per frame the Adler-32, per row its filter type, per segment a slot of round16(segment_bytes + 5) bytes.
 *   35300 png_filter_kernel (one wave per row)   35400 png_segment_kernel (one wave per segment: tokens, codes, bits, CRC)
 *   35500 png_scan_kernel (one workgroup per frame)   35600 png_copy_kernel (one wave per segment).
 *   The size queries need no device and return 0, with the reason in resr_last_error(), for a descriptor the entry refuses.
 *   RESR_ERR_ARG before any launch, "png_encode" in resr_last_error(): a null descriptor or pointer; n, h or w < 1; h or w above
 *   (2^31 - 1) / bpp; channels other than 1, 3, 4; a bit depth other than 8, 16; segment_bytes other than 0 or 64..65535; n * segments or
 *   n * h above 2^31 - 1; a negative out_stride; header_bytes other than RESR_PNG_HEADER_BYTES; a workspace below the query's answer or
 *   not 16-byte aligned; lengths not 8-byte aligned.  src needs the alignment of its samples, out none; out_stride may be odd.
 *   Not built: LZ77 matches beyond distance 1, fixed-Huffman blocks, palette and grey+alpha types, interlace, ancillary chunks, byte
 *   equality with libpng. */
#define RESR_PNG_DEFAULT_SEGMENT_BYTES 16384
#define RESR_PNG_HEADER_BYTES 47
typedef struct {
    int32_t n, h, w;
    int32_t channels;             /* 1, 3, 4 */
    int32_t bit_depth;            /* 8, 16 */
    int32_t segment_bytes;        /* bytes of the filtered stream per deflate block; 0 = RESR_PNG_DEFAULT_SEGMENT_BYTES */
} ResrPngEncDesc;
size_t resr_png_encode_max_bytes(const ResrPngEncDesc* d);
size_t resr_png_encode_workspace_bytes(const ResrPngEncDesc* d);
int resr_png_encode_header(const ResrPngEncDesc* d, uint8_t* host_buf, size_t cap);
int resr_png_encode(const ResrPngEncDesc* d, const void* src, uint8_t* out, int64_t out_stride, int64_t* lengths,
                    const uint8_t* header_dev, int32_t header_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* ---- discriminator helpers (model.py:135-203) -------------------------------------------------------- */
/* 2x2 space-to-depth of an NHWC tensor [n,h,w,c] -> [n,h/2,w/2,4c] (inverse != 0: depth-to-space) */
int resr_space_to_depth(const void* src, void* dst, int32_t n, int32_t h, int32_t w, int32_t c, int32_t dtype,
                        int32_t inverse, void* stream);
/* F.interpolate(scale_factor=2, mode="bilinear", align_corners=False) on NHWC [n,h,w,c] (model.py:186,190,194);
 * backward != 0: src is the gradient [n,2h,2w,c], dst the input gradient [n,h,w,c] */
int resr_bilinear_up2x(const void* src, void* dst, int32_t n, int32_t h, int32_t w, int32_t c, int32_t dtype,
                       int32_t backward, void* stream);
/* out = (a + b) * (mask > 0 ? 1 : slope); b and mask optional (RESR_F16X2: a, b, out are pairs with the lo tensor `count`
 * elements behind the hi tensor; the mask is an activation, read from its hi tensor) */
int resr_add_mask(const void* a, const void* b, const void* mask, void* out, int64_t count, int32_t dtype, float slope,
                  void* stream);
/* partial[k] = workgroup k's share of sum |a - b| over `count` elements (nblocks workgroups, fixed order: deterministic); the
 * caller adds the partials and divides: F.l1_loss of two feature tensors (model.py:320-327) without fp32 copies of them.
 * RESR_F16X2: a and b are pairs with the lo tensor lo_offset elements behind the hi tensor */
int resr_l1_partial(const void* a, const void* b, int64_t count, int32_t dtype, int64_t lo_offset, float* partial, int32_t nblocks,
                    void* stream);
/* ---- scalar losses of the train steps, forward value and unit gradient in ONE launch each --------------------------------
 * scratch: resr_loss_scratch_bytes() bytes of device memory owned by the caller, zero-filled once (an arrival counter + one
 * partial sum per workgroup; the last workgroup adds them in a fixed order and re-arms the counter: deterministic values).
 * Launches that may overlap in time need their own scratch.
 * resr_bce_logits_const: loss[0] = weight * mean_i BCEWithLogits(logits_i, label) against a CONSTANT label -- nn.BCEWithLogitsLoss
 *   on torch.full(..., 1.0 / 0.0) (train_realesrgan.py:460-461,478,500,509) without the label tensor; grad (nullable, [count]) =
 *   d loss / d logits_i = weight / count * (sigmoid(logits_i) - label).
 * resr_l1_mean: loss[0] = weight * mean_i |a_i - b_i| -- nn.L1Loss (train_realesrnet.py:385, train_realesrgan.py:475); grad_a
 *   (nullable) = weight / count * sign(a_i - b_i).  All tensors fp32, 16-byte aligned. */
size_t resr_loss_scratch_bytes(void);
int resr_bce_logits_const(const float* logits, int64_t count, float label, float weight, float* loss, float* grad, float* scratch,
                          void* stream);
int resr_l1_mean(const float* a, const float* b, int64_t count, float weight, float* loss, float* grad_a, float* scratch, void* stream);
/* out[r] = coef_host[r] * sum_k partial[r * cols + k] for r < rows (<= 8), out[rows] = their total: the weighted feature
 * distances of the perceptual term (model.py:320-335) from resr_l1_partial's partial sums, one launch; coef_host is HOST memory. */
int resr_weighted_row_sums(const float* partial, int32_t rows, int32_t cols, const float* coef_host, float* out, void* stream);

/* torch.nn.utils.spectral_norm forward (model.py:140-168): W [rows][cols] fp32; training: one power iteration
 * updating u[rows], v[cols] in place; sigma2[0] = sigma, sigma2[1] = 1/sigma; tmp = rows + ceil(rows/32) * cols floats
 * (W^T u is summed in 32-row groups, in a fixed order: bit-identical on every data-parallel rank) */
int resr_spectral_norm(const float* w, float* u, float* v, int32_t rows, int32_t cols, int32_t training, float eps,
                       float* sigma2, float* tmp, void* stream);
/* gradient wrt W_orig from the gradient wrt W = W_orig/sigma; tmp1 = 512 floats (block partials of <G, W>, added in a fixed
 * order: no atomics, the result is bit-reproducible) */
int resr_spectral_norm_bwd(const float* g, const float* w, const float* u, const float* v, const float* sigma2, float* dst,
                           int32_t rows, int32_t cols, int32_t accumulate, float* tmp1, void* stream);
/* 2x2 stride-2 max pooling on NHWC [n,2*h_out,2*w_out,c] (VGG19 of ContentLoss, model.py:296-298).  RESR_F16X2: src and dst
 * are (hi, lo) pairs, each lo tensor directly behind its hi tensor (this holds for every helper of this group). */
int resr_maxpool2x2(const void* src, void* dst, int32_t n, int32_t h_out, int32_t w_out, int32_t c, int32_t dtype,
                    void* stream);
/* ... also recording which window position won (arg: uint8 [n,h_out,w_out,c], value dy * 2 + dx, the first maximum in that order
 * like ATen's max_pool2d; may be NULL), and the backward pass through it: gin [n,2*h_out,2*w_out,c] receives g at the recorded
 * position of every window and zeros elsewhere (the differentiable perceptual term, model.py:311-335). */
int resr_maxpool2x2_arg(const void* src, void* dst, uint8_t* arg, int32_t n, int32_t h_out, int32_t w_out, int32_t c, int32_t dtype,
                        void* stream);
int resr_maxpool2x2_bwd(const void* g, const uint8_t* arg, void* gin, int32_t n, int32_t h_out, int32_t w_out, int32_t c, int32_t dtype,
                        void* stream);
/* virtual [cout][4C][3][3] weight gradient of a space-to-depth conv -> real [cout][C][4][4] */
int resr_fold4x4(const float* dw3, float* dw4, int32_t cout, int32_t c, void* stream);

/* Whole-discriminator passes (model.py:135-203, torch.nn.utils.spectral_norm included, and the autograd backward), enqueued
 * natively like the generator's: see real_esrgan-pytorch_amd/csrc/disc_native.hip for the parameter / spectral-norm arena
 * layouts (the reference's named_parameters() / named_buffers() orders) and the workspace plan.  The workspace holds the
 * activations kept for backward, THIS call's spectral-norm vectors, sigmas and packed weights (the module is called three
 * times per GAN step, train_realesrgan.py:479,500,508) and all scratch: nothing is allocated per tensor. */
typedef struct {
    int32_t n, h, w;       /* input [n,3,h,w], h and w multiples of 8                                  */
    int32_t dtype;         /* RESR_F16, RESR_F16X2 (hi/lo pairs: fp32-class results) or RESR_F32       */
    int32_t training;      /* keep activations for resr_discriminator_backward                         */
    int32_t sn_training;   /* module in training mode: one power iteration, u / v updated in place     */
} ResrDiscriminatorDesc;
size_t resr_discriminator_param_count(void);
size_t resr_discriminator_uv_count(void);
/* The first 256 bytes of a discriminator workspace (1 / sigma of the normalised layers + the gradient pre-scale slot of
 * resr_discriminator_backward, see resr_generator_backward) are filled with zeros by the caller once, when the workspace is allocated. */
size_t resr_discriminator_workspace_bytes(const ResrDiscriminatorDesc* d);
/* chunk table for the pack launch inside resr_discriminator_forward (host memory; returns the count, `chunks` may be NULL to
 * query it).  1/sigma of the normalised layers is read on the device from the head of `workspace`: one table per workspace. */
int64_t resr_discriminator_pack_table(const ResrDiscriminatorDesc* d, const void* workspace, ResrPackChunk* chunks, int64_t capacity);
int resr_discriminator_forward(const ResrDiscriminatorDesc* d, const float* x_nchw, const float* params, float* uv,
                               const ResrPackChunk* table_dev, int32_t n_chunks, void* workspace, size_t workspace_bytes,
                               float* y_nchw, void* stream);
/* grad_params = NULL: gradient wrt the input only (the generator's adversarial term, discriminator frozen); gx_nchw optional */
int resr_discriminator_backward(const ResrDiscriminatorDesc* d, const float* gy_nchw, const float* params, void* workspace,
                                size_t workspace_bytes, float* grad_params, float* gx_nchw, void* stream);
/* Output-parity backward (opt-in): after a RESR_F16X2 forward with training = 1 (d->dtype = RESR_F16X2, the same descriptor and
 * workspace), the backward pass in RESR_F16 arithmetic -- fast mode's kernels (backward-data conv, weight gradients, bilinear /
 * depth-to-space glue with their LeakyReLU masks, fold, spectral-norm backward with THIS call's u, v and sigma) on the hi halves
 * of the activations the forward stored (same pixel strides, lo offsets 0).  The forward and its outputs are exact16's, untouched;
 * the gradients are in fast mode's class.  LeakyReLU masks come from sign(hi): that is the sign of the forward's fp32 value
 * except where |value| < 2^-25 (hi rounds to a signed zero).  The f16 weights are packed inside this call, from the 1/sigma the
 * forward left at the head of the workspace, into the workspace's packed region (the next forward repacks its own form there);
 * `table_dev` / `n_chunks` are the forward's: resr_discriminator_pack_table does not depend on the dtype.  Same contract as
 * resr_discriminator_backward otherwise: grad_params = NULL gives the input gradient only, gx_nchw is optional, the gradient
 * lift and its sticky back-off use the same workspace slot; no allocation, no host synchronisation. */
int resr_discriminator_backward_f16(const ResrDiscriminatorDesc* d, const float* gy_nchw, const float* params,
                                    const ResrPackChunk* table_dev, int32_t n_chunks, void* workspace, size_t workspace_bytes,
                                    float* grad_params, float* gx_nchw, void* stream);

/* EMA.update (model.py:43-48) over the flat parameter arena, one launch. */
int resr_ema_update(float* shadow, const float* params, int64_t count, double decay, void* stream);

const char* resr_last_error(void);
int resr_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RESR_H_ */
