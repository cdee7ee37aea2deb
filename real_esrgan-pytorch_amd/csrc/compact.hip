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
//   END_RGB8          uint8 HWC frames: frames.hip's head in place of the layout kernel, its u8 tail (pixel-shuffle + residual +
//                     * 255, clamp, truncate) in place of compact_tail_kernel;
//   END_YUV           YUV 4:2:0 frames [N,3H/2,W] of bytes or of 16-bit words holding 10-bit samples (yuv420p10le / P010: 1023
//                     levels): frames.hip's head reading YUV, and its YUV tail.  The source and the destination each have their
//                     own descriptor (Ends::src, Ends::dst): the head and the tail's residual follow the source's depth, layout
//                     and matrix, the tail's quantisation and stores the destination's; the same-format entries pass one twice;
//   ... and scaled    ("outscale") image_resize.hip's fused tail in place of either: the HR frame is formed tile by tile in LDS and
//                     only the resized frame, uint8 [N,oh,ow,3] or YUV 4:2:0 [N,3oh/2,ow], is written.
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
    if (e.format == END_RGB8 && ((size_t)e.y & 3) != 0) return fail(RESR_ERR_ARG, "%s: y_u8 must be 4-byte aligned", who);
    int rc = RESR_OK;
    // the descriptor and the LR frame; of scaled ends the output pointer's rule is the plan's (nullptr passes the unscaled tail's)
    if (e.format == END_YUV) rc = yuv_forward_check(who, d.n, d.h, d.w, d.upscale, e.scaled ? nullptr : e.y, e.src, e.dst, e.bits_expected);
    if (!rc && e.scaled)
        rc = resize_plan(who, d.n, 3, d.h * d.upscale, d.w * d.upscale, e.sc.oh, e.sc.ow, e.sc.idx_y, e.sc.w_y, e.sc.taps_y, e.sc.idx_x,
                         e.sc.w_x, e.sc.taps_x, e.format == END_RGB8 ? RESIZE_U8 : yuv_bits(e.dst->layout) == 8 ? RESIZE_YUV8 : RESIZE_YUV10, e.y, geom);
    if (rc) return rc;
    if (p.total > workspace_bytes) return fail(RESR_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, workspace_bytes, p.total);
    return RESR_OK;
}

}  // namespace

// The launch sequence every entry shares: plan, refusals, head, convs, tail.
int compact_forward_ends(const ResrCompactDesc* d, const Ends& e, const float* params, const void* packed, void* workspace,
                         size_t workspace_bytes, hipStream_t st, const char* who) {
    if (e.format == END_YUV && (!e.src || !e.dst)) return fail(RESR_ERR_ARG, "%s: null argument", who);
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
    else rc = frame_head_dispatch(e.x, xin, N, H, W, d->dtype, st, (long)lo32, e.src);   // src null: RGB bytes; its layout: bytes or 16-bit words
    if (rc) return rc;
    auto desc = [&](const CConv& c, int flags) {
        ResrConvDesc cd = conv_desc_base(N, H, W, d->dtype, flags, d->act == RESR_COMPACT_LRELU ? 0.1f : 0.f);
        cd.cin = cd.cin0 = cd.in0_stride = c.cin_pad;
        cd.cout = c.cout; cd.cout_pad = c.cout_pad;
        cd.out_stride = (flags & RESR_CONV_OUT_NCHW_F32) ? 0 : c.cout_pad;
        cd.in0_lo_offset = c.cin_pad == 32 ? lo32 : lo64;
        cd.out_lo_offset = (flags & RESR_CONV_OUT_NCHW_F32) ? 0 : lo64;
        return cd;
    };
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
        case END_RGB8:
            if (!e.scaled) return compact_tail_u8(t, (const uint8_t*)e.x, (uint8_t*)e.y, N, H, W, s, st);
            return compact_tail_u8_scaled(t, (const uint8_t*)e.x, (uint8_t*)e.y, N, H, W, s, e.sc.idx_y, e.sc.w_y, e.sc.idx_x, e.sc.w_x, &geom, st);
        case END_YUV:
            if (!e.scaled) return compact_tail_yuv(t, e.x, e.y, N, H, W, s, e.src, e.dst, st);
            return compact_tail_yuv420_scaled(t, e.x, e.y, N, H, W, s, e.sc.idx_y, e.sc.w_y, e.sc.idx_x, e.sc.w_x, e.src, e.dst, &geom, st);
    }
    return fail(RESR_ERR_ARG, "%s: unknown kind of ends", who);
}

}  // namespace resr
