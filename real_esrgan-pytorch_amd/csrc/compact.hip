// compact.hip -- the compact generator (upstream Real-ESRGAN's SRVGGNetCompact) as one natively enqueued forward pass:
// the HBM plan, the launch order and the one kernel of its own (pixel-shuffle + nearest-upsampled residual).
//
//   x [N,3,H,W] fp32 -> x_in [N,H,W,32] (layout.hip, channels 3..31 zero)
//   conv 3->64 + act            x_in -> A      (act: per-channel PReLU -- conv3x3_dispatch_prelu --, LeakyReLU 0.1 or ReLU)
//   num_conv x conv 64->64 + act   A -> B -> A ...
//   conv 64->3*s*s              -> t [N,3s^2,H,W] fp32 NCHW (the conv's fp32 epilogue: exact16 keeps its fp32-class value)
//   y[n,c,Y,X] = t[n, c*s*s + (Y%s)*s + X%s, Y/s, X/s] + x[n,c,Y/s,X/s]      (one launch, 64-bit indexing)
// T = f16 (fast) / f32 (strict); RESR_F16X2 (exact16): every NHWC tensor is a hi/lo pair, the lo tensor right behind the hi one,
// three stages per chunk.  No padding beyond each conv's own pad = 1: any H, W >= 1.
// Every entry of the C ABI is this sequence with its own pair of ends (Ends of common.h: a format and a flag), same plan, same workspace:
//   END_YUV           YUV 4:2:0 frames [N,3H/2,W] of bytes or of 16-bit words holding 10-bit samples (yuv420p10le / P010: 1023
//                     levels): frames.hip's head reading YUV, and its YUV tail.  The source and the destination each have their
//                     own descriptor (Ends::src, Ends::dst): the head and the tail's residual follow the source's depth, layout
//                     and matrix, the tail's quantisation and stores the destination's; the same-format entries pass one twice;
//   END_IMAGE         grey, RGB or RGBA images [N,H,W,C] of bytes or 16-bit words (Ends::img): frames.hip's head reading them -- the
//                     network's batch is the N colour (or grey) images and, for RGBA, the N alpha planes behind them, each level
//                     three times -- and its image tail (grey: the fixed-point grey of the three levels; RGBA: the alpha images'
//                     grey as the fourth channel).  uint8 HWC frames (resr_compact_forward_u8) are the (3, 8) mode, kRgb8: the
//                     tail is pixel-shuffle + residual + * 255, clamp, truncate in place of compact_tail_kernel;
//   ... and scaled    ("outscale") image_resize.hip's fused tail in place of any of them: the HR frame is formed tile by tile in LDS
//                     and only the resized frame, uint8 [N,oh,ow,3], YUV 4:2:0 [N,3oh/2,ow] or images [N,oh,ow,C], is written.
// Training (compact_forward_train / compact_backward, at the end of this file; kernels of its own in compact_train.hip): the same
// convolutions with a plain epilogue, every pre-activation z_k and activation a_k kept -- TPlan below states the workspace.
#include <vector>

#include "conv3x3.h"
#include "packed_layout.h"
#include "yuv.h"

namespace resr {

namespace {

struct CConv {
    int cin, cin_pad, cout, cout_pad;
    size_t w_off, b_off;   // element offsets in the fp32 parameter arena
    long a_off;            // PReLU slopes (-1: none)
    size_t pk;             // element offset in the packed buffer
};

struct CPlan {
    ResrCompactDesc d;
    std::vector<CConv> convs;   // conv 0 (3 -> 64), num_conv body convs, the last conv (64 -> 3 s^2)
    size_t n_params, pk_elems;
    long px;                    // N * H * W
    size_t off_xin, off_a, off_b, off_t, total;
};

bool build_cplan(const ResrCompactDesc* d, CPlan& p) {
    if (!d) return false;
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->num_conv < 0 || d->num_conv > 4096 || d->upscale < 1 || d->upscale > 4 ||
        d->act < RESR_COMPACT_PRELU || d->act > RESR_COMPACT_RELU ||
        (d->dtype != RESR_F16 && d->dtype != RESR_F32 && d->dtype != RESR_F16X2))
        return false;
    p.d = *d;
    p.px = (long)d->n * d->h * d->w;
    // element offsets of a 64-channel NHWC tensor stay below 2^31; the pair kernels address at most 2^24 pixels per tensor
    if (p.px > 0x7fffffffL / 64 || (d->dtype == RESR_F16X2 && p.px > (1L << 24))) return false;
    const int s = d->upscale;
    size_t off = 0;
    auto add = [&](int cin, int cout, bool act) {
        CConv c;
        c.cin = cin; c.cin_pad = round32(cin); c.cout = cout; c.cout_pad = round32(cout);
        c.w_off = off; off += (size_t)cout * cin * 9;
        c.b_off = off; off += cout;
        c.a_off = -1;
        if (act && d->act == RESR_COMPACT_PRELU) { c.a_off = (long)off; off += cout; }
        c.pk = 0;
        p.convs.push_back(c);
    };
    add(3, 64, true);
    for (int i = 0; i < d->num_conv; ++i) add(64, 64, true);
    add(64, 3 * s * s, false);
    p.n_params = off;
    size_t pk = 0;
    for (auto& c : p.convs) {
        c.pk = pk;
        pk += packed_conv_elems(c.cout_pad, c.cin_pad);
    }
    p.pk_elems = pk;
    const size_t es = elem_size(d->dtype) * act_tensors(d->dtype);
    size_t ws = 0;
    auto carve = [&](size_t bytes) { const size_t o = ws; ws = align_up(ws + bytes, 256); return o; };
    p.off_xin = carve((size_t)p.px * 32 * es);
    p.off_a = carve((size_t)p.px * 64 * es);
    p.off_b = carve((size_t)p.px * 64 * es);
    p.off_t = carve((size_t)p.px * 3 * s * s * 4);
    p.total = ws;
    return true;
}

// The descriptor of conv `c` of the net on NHWC tensors of the plan's dtype (lo32 / lo64: exact16's hi -> lo element offsets of a 32- /
// 64-channel tensor, else 0), shared by the inference and the training forward.
ResrConvDesc cconv_desc(const ResrCompactDesc& d, const CConv& c, int flags, int64_t lo32, int64_t lo64) {
    ResrConvDesc cd = conv_desc_base(d.n, d.h, d.w, d.dtype, flags, d.act == RESR_COMPACT_LRELU ? 0.1f : 0.f);
    cd.cin = cd.cin0 = cd.in0_stride = c.cin_pad;
    cd.cout = c.cout; cd.cout_pad = c.cout_pad;
    cd.out_stride = (flags & RESR_CONV_OUT_NCHW_F32) ? 0 : c.cout_pad;
    cd.in0_lo_offset = c.cin_pad == 32 ? lo32 : lo64;
    cd.out_lo_offset = (flags & RESR_CONV_OUT_NCHW_F32) ? 0 : lo64;
    return cd;
}

// y [n,3,hS,wS] = pixel_shuffle(t [n,3S^2,h,w], S) + nearest_upsample(x [n,3,h,w], S): one output row per (grid-strided) y block,
// columns across x blocks; every index that can pass 2^31 is 64-bit
template <int S>
__global__ __launch_bounds__(256) void compact_tail_kernel(const float* __restrict__ t, const float* __restrict__ x,
                                                           float* __restrict__ y, int n, int h, int w) {
    const int HS = h * S, WS = w * S;
    const long rows = (long)n * 3 * HS;
    const long plane = (long)h * w;
    for (long row = blockIdx.y; row < rows; row += gridDim.y) {
        const int Y = (int)(row % HS);
        const long bc = row / HS;              // n * 3 + c
        const long b = bc / 3;
        const int c = (int)(bc - b * 3);
        const int yy = Y / S, sy = Y - yy * S;
        const float* trow = t + ((b * 3 * S * S + (long)c * S * S + sy * S) * plane) + (long)yy * w;
        const float* xrow = x + (bc * h + yy) * (long)w;
        float* yrow = y + row * (long)WS;
        for (int X = blockIdx.x * 256 + threadIdx.x; X < WS; X += gridDim.x * 256) {
            const int xx = X / S, sx = X - xx * S;
            yrow[X] = trow[sx * plane + xx] + xrow[xx];
        }
    }
}

int compact_tail(const float* t, const float* x, float* y, int n, int h, int w, int s, hipStream_t st) {
    const long rows = (long)n * 3 * h * s;
    const dim3 grid((unsigned)((w * s + 255) / 256), (unsigned)(rows > 65535 ? 65535 : rows));
    prof_before(st);
    if (!with_scale(s, [&](auto S) { hipLaunchKernelGGL(compact_tail_kernel<S()>, grid, dim3(256), 0, st, t, x, y, n, h, w); }))
        return fail(RESR_ERR_ARG, "compact_tail: upscale %d", s);
    prof_after(st, 31000 + s, 0.0, (double)n * 3 * h * w * (s * s * 8.0 + 4.0));
    RESR_CHECK_LAUNCH("compact_tail_kernel");
    return RESR_OK;
}

}  // namespace

size_t compact_param_count(const ResrCompactDesc* d) {
    CPlan p;
    return build_cplan(d, p) ? p.n_params : 0;
}

size_t compact_packed_bytes(const ResrCompactDesc* d) {
    CPlan p;
    return build_cplan(d, p) ? packed_buffer_bytes(p.pk_elems, d->dtype) : 0;
}

size_t compact_workspace_bytes(const ResrCompactDesc* d) {
    CPlan p;
    return build_cplan(d, p) ? p.total : 0;
}

int64_t compact_pack_table(const ResrCompactDesc* d, ResrPackChunk* out, int64_t cap) {
    CPlan p;
    if (!build_cplan(d, p)) return fail(RESR_ERR_ARG, "compact: bad descriptor");
    std::vector<ResrPackChunk> t;
    for (const auto& c : p.convs) emit_conv_chunks(t, (int64_t)c.w_off, c.cout, c.cin, 0, (int64_t)c.pk);
    return copy_pack_table(t, out, cap, "compact_pack_table");
}

namespace {

// Everything a call can be refused for after its descriptor, before the first launch.  Scaled ends: fills geom.
int check_ends(const CPlan& p, const Ends& e, const float* params, const void* packed, const void* workspace, size_t workspace_bytes,
               const char* who, ResizeGeom* geom) {
    const ResrCompactDesc& d = p.d;
    if (!e.x || !e.y || !params || !packed || !workspace) return fail(RESR_ERR_ARG, "%s: null argument", who);
    if (e.format == END_F32 && e.scaled) return fail(RESR_ERR_ARG, "%s: unknown kind of ends", who);
    // (the uint8-typed entries, which pass kRgb8 itself, name their y as they always have; scaled or not)
    if (e.img == &kRgb8 && ((size_t)e.y & 3) != 0) return fail(RESR_ERR_ARG, "%s: y_u8 must be 4-byte aligned", who);
    int rc = RESR_OK;
    // the descriptor and the LR frame; of scaled ends the output pointer's rule is the plan's (nullptr passes the unscaled tail's)
    if (e.format == END_YUV) rc = yuv_forward_check(who, d.n, d.h, d.w, d.upscale, e.scaled ? nullptr : e.y, e.src, e.dst, e.bits_expected);
    if (e.format == END_IMAGE) rc = image_forward_check(who, d.n, d.h, d.w, d.upscale, e.x, e.scaled ? nullptr : e.y, e.img);
    if (!rc && e.scaled) {
        // an image tail's workgroups own whole pixels: its grid counts the N images, not the planes * N of the network
        const int images = e.format == END_IMAGE && e.img->channels == 4 ? d.n / 2 : d.n;
        const int kind = e.format == END_IMAGE ? resize_image_kind(e.img->channels, e.img->bits) : yuv_bits(e.dst->layout) == 8 ? RESIZE_YUV8 : RESIZE_YUV10;
        rc = resize_plan(who, images, 3, d.h * d.upscale, d.w * d.upscale, e.sc.oh, e.sc.ow, e.sc.idx_y, e.sc.w_y, e.sc.taps_y, e.sc.idx_x,
                         e.sc.w_x, e.sc.taps_x, kind, e.y, geom);
    }
    if (rc) return rc;
    if (p.total > workspace_bytes) return fail(RESR_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, workspace_bytes, p.total);
    return RESR_OK;
}

}  // namespace

// The launch sequence every entry shares: plan, refusals, head, convs, tail.
int compact_forward_ends(const ResrCompactDesc* d, const Ends& e, const float* params, const void* packed, void* workspace,
                         size_t workspace_bytes, hipStream_t st, const char* who) {
    if ((e.format == END_YUV && (!e.src || !e.dst)) || (e.format == END_IMAGE && !e.img)) return fail(RESR_ERR_ARG, "%s: null argument", who);
    CPlan p;
    if (!build_cplan(d, p)) return fail(RESR_ERR_ARG, "%s: bad descriptor", who);
    ResizeGeom geom;
    int rc = check_ends(p, e, params, packed, workspace, workspace_bytes, who, &geom);
    if (rc) return rc;
    const bool x2 = d->dtype == RESR_F16X2;
    const size_t wes = packed_elem_bytes(d->dtype);   // bytes per element of the packed layout
    const char* pk = (const char*)packed;
    char* base = (char*)workspace;
    char* xin = base + p.off_xin;
    char* buf[2] = {base + p.off_a, base + p.off_b};
    float* t = reinterpret_cast<float*>(base + p.off_t);
    const int N = d->n, H = d->h, W = d->w;
    const int64_t lo32 = x2 ? (int64_t)p.px * 32 : 0, lo64 = x2 ? (int64_t)p.px * 64 : 0;   // hi -> lo element offsets
    if (e.format == END_F32) rc = nchw_to_nhwc_dispatch((const float*)e.x, xin, N, 3, H, W, 1, 32, d->dtype, nullptr, st, (long)lo32);
    else rc = frame_head_dispatch(e.x, xin, N, H, W, d->dtype, st, (long)lo32, e.src, e.img);   // src's layout: bytes or 16-bit words
    if (rc) return rc;
    auto desc = [&](const CConv& c, int flags) { return cconv_desc(*d, c, flags, lo32, lo64); };
    const int nbody = (int)p.convs.size() - 1;   // conv 0 + the num_conv body convs: 64 channels + activation
    const char* in = xin;
    for (int k = 0; k < nbody; ++k) {
        const CConv& c = p.convs[k];
        char* out = buf[k & 1];
        if (d->act == RESR_COMPACT_PRELU) {
            ResrConvDesc cd = desc(c, 0);
            rc = conv3x3_dispatch_prelu(&cd, in, pk + c.pk * wes, params + c.b_off, params + c.a_off, out, st);
        } else {
            ResrConvDesc cd = desc(c, RESR_CONV_LRELU);
            rc = conv3x3_dispatch(&cd, in, nullptr, pk + c.pk * wes, params + c.b_off, nullptr, nullptr, nullptr, out, nullptr, st);
        }
        if (rc) return rc;
        in = out;
    }
    {   // the last conv: fp32 NCHW [N, 3 s^2, H, W]
        const CConv& c = p.convs[nbody];
        ResrConvDesc cd = desc(c, RESR_CONV_OUT_NCHW_F32);
        rc = conv3x3_dispatch(&cd, in, nullptr, pk + c.pk * wes, params + c.b_off, nullptr, nullptr, nullptr, t, nullptr, st);
        if (rc) return rc;
    }
    const int s = d->upscale;
    switch (e.format) {
        case END_F32: return compact_tail(t, (const float*)e.x, (float*)e.y, N, H, W, s, st);
        case END_YUV:
            if (!e.scaled) return compact_tail_yuv(t, e.x, e.y, N, H, W, s, e.src, e.dst, st);
            return compact_tail_yuv420_scaled(t, e.x, e.y, N, H, W, s, e.sc.idx_y, e.sc.w_y, e.sc.idx_x, e.sc.w_x, e.src, e.dst, &geom, st);
        case END_IMAGE: {
            const int images = e.img->channels == 4 ? N / 2 : N;
            if (!e.scaled) return compact_tail_image(t, e.x, e.y, images, H, W, s, e.img, st);
            return compact_tail_image_scaled(t, e.x, e.y, images, H, W, s, e.sc.idx_y, e.sc.w_y, e.sc.idx_x, e.sc.w_x, e.img, &geom, st);
        }
    }
    return fail(RESR_ERR_ARG, "%s: unknown kind of ends", who);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Training: the saved-activation forward and the backward pass (include/resr.h, "Compact generator: training").  fast (f16) and strict
// (f32); exact16 training is not built.  No convolution kernel or epilogue of its own: conv3x3_dispatch with a plain (bias) epilogue
// writes z_k, one element-wise launch writes a_k = act(z_k), and both stay in the workspace -- the backward pass needs the sign of z_k
// (a trained PReLU slope may be negative, zero or above 1: a_k > 0 does not say z_k > 0), z_k itself for the slope gradient, and a_{k-1}
// for the weight gradient.  The backward pass is generator.hip's calling pattern: the convolutions on transposed packings, one
// weight-gradient launch pair per layer, the gradient pre-scale of common.h for f16.
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

// The workspace of a training graph, every buffer 256-byte aligned, es = 2 (fast) / 4 (strict) bytes, px = N H W:
//   slot    256 B            the gradient pre-scale slot (common.h: grad_prescale): the head the caller zero-fills once
//   x_in    px * 32 * es     the input as NHWC, channels 3..31 zero                                  (forward -> backward: X of conv 0)
//   z_k     px * 64 * es     k = 0 .. num_conv: pre-activations                                      (forward -> backward)
//   a_k     px * 64 * es     k = 0 .. num_conv: activations                                          (forward -> backward: X of conv k + 1)
//   t       px * 3 s^2 * 4   the last conv's fp32 NCHW output                                        (forward only)
//   g_t     px * cpl * es    the pixel-unshuffled output gradient, cpl = round32(3 s^2)              (backward)
//   g0, g1  px * 64 * es     g_a / g_z of the layer at hand, ping-pong (act_bwd runs in place)       (backward)
//   g_xin   px * 32 * es     the input gradient as NHWC                                              (backward, gx wanted)
//   dsp     <= 1024 * 256 B  per-block partial sums of a slope gradient                              (backward, PReLU)
//   slabs                    the weight-gradient slabs of the largest layer (wgrad_slab_bytes)       (backward)
struct TPlan {
    CPlan p;
    std::vector<size_t> pk_bwd;   // element offsets of the transposed (backward-data) packings, behind the forward ones
    size_t pk_total;
    size_t off_slot, off_xin, off_z, off_a, act_bytes, off_t, off_gt, off_g[2], off_gxin, off_dsp, dsp_bytes, off_slab, slab_bytes, total;
};

constexpr size_t kTrainStateBytes = 256;

// jobs of one layer's weight-gradient launch: (X chunks) x (G tiles)
int layer_jobs(const CConv& c) { return (c.cin_pad / 32) * (c.cout_pad / 32); }

bool build_tplan(const ResrCompactDesc* d, TPlan& t, const char* who) {
    if (!build_cplan(d, t.p)) return fail(RESR_ERR_ARG, "%s: bad descriptor", who), false;
    if (d->dtype == RESR_F16X2) return fail(RESR_ERR_ARG, "%s: exact16 training is not built (RESR_F16 or RESR_F32)", who), false;
    const CPlan& p = t.p;
    size_t pk = p.pk_elems;
    t.pk_bwd.clear();
    for (const auto& c : p.convs) {   // transposed: M = cin_pad, K = cout_pad
        t.pk_bwd.push_back(pk);
        pk += packed_conv_elems(c.cin_pad, c.cout_pad);
    }
    t.pk_total = pk;
    const size_t es = elem_size(d->dtype), px = (size_t)p.px;
    const int nbody = (int)p.convs.size() - 1, s = d->upscale;
    size_t ws = 0;
    auto carve = [&](size_t bytes) { const size_t o = ws; ws = align_up(ws + bytes, 256); return o; };
    t.off_slot = carve(kTrainStateBytes);
    t.off_xin = carve(px * 32 * es);
    t.act_bytes = align_up(px * 64 * es, 256);
    t.off_z = carve(t.act_bytes * nbody);
    t.off_a = carve(t.act_bytes * nbody);
    t.off_t = carve(px * 3 * s * s * 4);
    t.off_gt = carve(px * p.convs[nbody].cout_pad * es);
    t.off_g[0] = carve(px * 64 * es);
    t.off_g[1] = carve(px * 64 * es);
    t.off_gxin = carve(px * 32 * es);
    t.dsp_bytes = d->act == RESR_COMPACT_PRELU ? compact_dslope_partial_bytes((int64_t)px, d->dtype) : 0;
    t.off_dsp = carve(t.dsp_bytes);
    t.slab_bytes = 0;
    for (const auto& c : p.convs) {
        const int jobs = layer_jobs(c);
        const size_t b = wgrad_slab_bytes(jobs, wgrad_default_splits(d->dtype, jobs, d->n, d->h, d->w));
        if (b > t.slab_bytes) t.slab_bytes = b;
    }
    t.off_slab = carve(t.slab_bytes);
    t.total = ws;
    return true;
}

}  // namespace

size_t compact_train_packed_bytes(const ResrCompactDesc* d) {
    TPlan t;
    return build_tplan(d, t, "compact_train_packed_bytes") ? packed_buffer_bytes(t.pk_total, d->dtype) : 0;
}

size_t compact_train_workspace_bytes(const ResrCompactDesc* d) {
    TPlan t;
    return build_tplan(d, t, "compact_train_workspace_bytes") ? t.total : 0;
}

size_t compact_train_state_bytes(const ResrCompactDesc* d) {
    TPlan t;
    return build_tplan(d, t, "compact_train_state_bytes") ? kTrainStateBytes : 0;
}

// debug/test aid: byte offsets of the named buffers of a training workspace (order documented in include/resr_debug.h); host only
int64_t compact_train_offsets(const ResrCompactDesc* d, int64_t* out, int64_t cap) {
    TPlan t;
    if (!build_tplan(d, t, "compact_train_offsets")) return RESR_ERR_ARG;
    const size_t offs[] = {t.off_slot, t.off_xin, t.off_z, t.off_a, t.act_bytes, t.off_t, t.off_gt, t.off_g[0], t.off_g[1], t.off_gxin};
    const int64_t n = sizeof(offs) / sizeof(offs[0]);
    if (!out || cap < n) return fail(RESR_ERR_ARG, "compact_train_offsets: capacity %lld < %lld", (long long)cap, (long long)n);
    for (int64_t i = 0; i < n; ++i) out[i] = (int64_t)offs[i];
    return n;
}

// compact_pack_table's chunks, then every convolution's transposed chunks in the same order
int64_t compact_train_pack_table(const ResrCompactDesc* d, ResrPackChunk* out, int64_t cap) {
    TPlan t;
    if (!build_tplan(d, t, "compact_train_pack_table")) return RESR_ERR_ARG;
    std::vector<ResrPackChunk> v;
    for (const auto& c : t.p.convs) emit_conv_chunks(v, (int64_t)c.w_off, c.cout, c.cin, 0, (int64_t)c.pk);
    for (size_t i = 0; i < t.p.convs.size(); ++i) {
        const CConv& c = t.p.convs[i];
        emit_conv_chunks(v, (int64_t)c.w_off, c.cout, c.cin, 1, (int64_t)t.pk_bwd[i]);
    }
    return copy_pack_table(v, out, cap, "compact_train_pack_table");
}

// the slope table of activation layer k: the PReLU parameters in the arena, or the constant table of the activation
static const float* layer_slopes(const ResrCompactDesc* d, const CConv& c, const float* params, const float* const_slopes) {
    return d->act == RESR_COMPACT_PRELU ? params + c.a_off : const_slopes;
}

int compact_forward_train(const ResrCompactDesc* d, const float* x, const float* params, const void* packed, void* workspace, size_t workspace_bytes,
                          float* y, hipStream_t st) {
    TPlan t;
    if (!build_tplan(d, t, "compact_forward_train")) return RESR_ERR_ARG;
    if (!x || !params || !packed || !workspace || !y) return fail(RESR_ERR_ARG, "compact_forward_train: null argument");
    if (t.total > workspace_bytes) return fail(RESR_ERR_WORKSPACE, "compact_forward_train: workspace %zu < %zu", workspace_bytes, t.total);
    const float* const_slopes = d->act == RESR_COMPACT_PRELU ? nullptr : compact_const_slopes(d->act);
    if (d->act != RESR_COMPACT_PRELU && !const_slopes) return fail(RESR_ERR_LAUNCH, "compact_forward_train: slope table");
    const CPlan& p = t.p;
    const size_t wes = packed_elem_bytes(d->dtype);
    const char* pk = (const char*)packed;
    char* base = (char*)workspace;
    const int N = d->n, H = d->h, W = d->w, nbody = (int)p.convs.size() - 1;
    int rc = nchw_to_nhwc_dispatch(x, base + t.off_xin, N, 3, H, W, 1, 32, d->dtype, nullptr, st, 0L);
    if (rc) return rc;
    const char* in = base + t.off_xin;
    for (int k = 0; k < nbody; ++k) {   // z_k = conv_k(a_{k-1}) + bias, a_k = act(z_k): both kept
        const CConv& c = p.convs[k];
        char* z = base + t.off_z + (size_t)k * t.act_bytes;
        char* a = base + t.off_a + (size_t)k * t.act_bytes;
        ResrConvDesc cd = cconv_desc(*d, c, 0, 0, 0);
        rc = conv3x3_dispatch(&cd, in, nullptr, pk + c.pk * wes, params + c.b_off, nullptr, nullptr, nullptr, z, nullptr, st);
        if (rc) return rc;
        rc = compact_act_dispatch(z, a, layer_slopes(d, c, params, const_slopes), (int64_t)p.px, d->dtype, st);
        if (rc) return rc;
        in = a;
    }
    float* tt = reinterpret_cast<float*>(base + t.off_t);
    {   // the last conv and the tail: the inference ones
        const CConv& c = p.convs[nbody];
        ResrConvDesc cd = cconv_desc(*d, c, RESR_CONV_OUT_NCHW_F32, 0, 0);
        rc = conv3x3_dispatch(&cd, in, nullptr, pk + c.pk * wes, params + c.b_off, nullptr, nullptr, nullptr, tt, nullptr, st);
        if (rc) return rc;
    }
    return compact_tail(tt, x, y, N, H, W, d->upscale, st);
}

int compact_backward(const ResrCompactDesc* d, const float* gy, const float* params, const void* packed, void* workspace, size_t workspace_bytes,
                     float* grad, float* gx, hipStream_t st) {
    TPlan t;
    if (!build_tplan(d, t, "compact_backward")) return RESR_ERR_ARG;
    if (!gy || !params || !packed || !workspace || !grad) return fail(RESR_ERR_ARG, "compact_backward: null argument");
    if (t.total > workspace_bytes) return fail(RESR_ERR_WORKSPACE, "compact_backward: workspace %zu < %zu", workspace_bytes, t.total);
    const float* const_slopes = d->act == RESR_COMPACT_PRELU ? nullptr : compact_const_slopes(d->act);
    if (d->act != RESR_COMPACT_PRELU && !const_slopes) return fail(RESR_ERR_LAUNCH, "compact_backward: slope table");
    const CPlan& p = t.p;
    const int dt = d->dtype;
    const size_t wes = packed_elem_bytes(dt);
    const char* pk = (const char*)packed;
    char* base = (char*)workspace;
    const int N = d->n, H = d->h, W = d->w, s = d->upscale, nbody = (int)p.convs.size() - 1;
    const int64_t px = p.px;
    // f16: the pass runs on g_y * 2^k (max |g_y 2^k| in [2^6, 2^7): common.h grad_prescale, the slot protocol, target and back-off of
    // generator_backward) and every result leaves times 2^-k; strict gets no lift
    unsigned* slot = reinterpret_cast<unsigned*>(base + t.off_slot);
    const unsigned* gsc = dt != RESR_F32 ? slot : nullptr;
    char* gt = base + t.off_gt;
    char* g[2] = {base + t.off_g[0], base + t.off_g[1]};
    float* dsp = reinterpret_cast<float*>(base + t.off_dsp);
    float* slab = reinterpret_cast<float*>(base + t.off_slab);
    auto z_of = [&](int k) { return base + t.off_z + (size_t)k * t.act_bytes; };
    auto a_of = [&](int k) { return base + t.off_a + (size_t)k * t.act_bytes; };
    // weight and bias gradients of conv `c` from X (channels [0, cin_pad) at that stride) and G (cout_pad channels)
    auto wgrad = [&](const CConv& c, const void* xk, const void* gk) -> int {
        WgradConv wc;
        wc.x0 = xk; wc.cin = c.cin_pad; wc.in0_stride = c.cin_pad; wc.cin_real = c.cin;
        wc.g = gk; wc.cout = c.cout; wc.cout_pad = c.cout_pad; wc.g_stride = c.cout_pad;
        wc.x_chunk_stride = wc.g_chunk_stride = 0;
        wc.x_lo_off = wc.g_lo_off = 0; wc.x_s2d_c = 0; wc.g_lo_bias_only = 0;
        wc.dw = grad + c.w_off; wc.db = grad + c.b_off; wc.scale = 1.f;
        wc.unscale = gsc;
        const int splits = wgrad_default_splits(dt, wgrad_batch_jobs(&wc, 1, dt), N, H, W);
        if (wgrad_batch_partial_bytes(&wc, 1, splits, dt) > t.slab_bytes) return fail(RESR_ERR_WORKSPACE, "compact_backward: wgrad slab buffer too small");
        return wgrad_batch(&wc, 1, N, H, W, dt, 0, splits, slab, st);
    };
    // backward-data of conv `c` through its transposed packing: G (cout_pad channels) -> cout_pad_out channels at that stride
    auto dgrad = [&](int i, const void* gk, void* out) -> int {
        const CConv& c = p.convs[i];
        ResrConvDesc cd = conv_desc_base(N, H, W, dt, RESR_CONV_NO_BIAS, 0.f);
        cd.cin = cd.cin0 = cd.in0_stride = c.cout_pad;
        cd.cout = cd.cout_pad = cd.out_stride = c.cin_pad;   // (the rows behind the real input channels are zero weights)
        return conv3x3_dispatch(&cd, gk, nullptr, pk + t.pk_bwd[i] * wes, nullptr, nullptr, nullptr, nullptr, out, nullptr, st);
    };
    int rc;
#define STEP(expr) do { rc = (expr); if (rc) return rc; } while (0)
    if (gsc) STEP(absmax_dispatch(gy, (long)(px * 3 * s * s), slot, 6, st));
    // g_t = pixel_unshuffle_s(g_y) * lift: channel c s^2 + i s + j, PixelShuffle's order; the pad channels zero
    STEP(nchw_to_nhwc_scaled_dispatch(gy, gt, N, 3, H * s, W * s, s, p.convs[nbody].cout_pad, dt, nullptr, st, 0L, gsc));
    STEP(wgrad(p.convs[nbody], a_of(nbody - 1), gt));
    STEP(dgrad(nbody, gt, g[0]));
    int cur = 0;
    for (int k = nbody - 1; k >= 0; --k) {
        const CConv& c = p.convs[k];
        // g_z = g_a * act'(z_k), in place; PReLU: the slope gradient from the same pass
        STEP(compact_act_bwd_dispatch(g[cur], z_of(k), g[cur], layer_slopes(d, c, params, const_slopes), px, dt, c.a_off >= 0 ? grad + c.a_off : nullptr, dsp, t.dsp_bytes, gsc, st));
        STEP(wgrad(c, k > 0 ? a_of(k - 1) : base + t.off_xin, g[cur]));
        if (k > 0) {
            STEP(dgrad(k, g[cur], g[cur ^ 1]));
            cur ^= 1;
        } else if (gx) {   // gx = nhwc_to_nchw(g_xin) / lift + the residual's adjoint
            char* gxin = base + t.off_gxin;
            STEP(dgrad(0, g[cur], gxin));
            STEP(nhwc_to_nchw_scaled_dispatch(gxin, gx, N, 3, H, W, 1, 32, dt, st, 0L, gsc));
            STEP(compact_residual_bwd_dispatch(gy, gx, N, H, W, s, st));
        }
    }
#undef STEP
    return RESR_OK;
}

}  // namespace resr
