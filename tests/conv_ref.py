"""Plain references of resr_conv3x3 and resr_conv3x3_wgrad (csrc/conv3x3.hip, conv3x3_ws.h, wgrad.hip), CPU only, and the rule that
judges a kernel against them.  Also of the 4x4 / stride-2 convolution whose forward, backward-data and weight-gradient passes the library
runs as sparse-tap 3x3 passes over the space-to-depth image (correlate4x4s2 and below; tests/test_gpu_sparse_taps.py).

Every function restates the operation from its DEFINITION in include/resr.h on NCHW tensors -- a sum over the nine taps of a
zero-padded image, then the epilogue steps in the documented order -- and shares no index arithmetic with the kernels.  Each
evaluates in the precision it is asked for: float64 is the reference, float32 ON THE SAME INPUTS is the yardstick the allowance
is derived from.  tests/test_conv_ref.py checks the references against torch and shows that the rule rejects wrong kernels before
tests/test_gpu_kernels.py lets it judge a real one.

Values.  A case runs on exactly the values the kernel is given: f16 / f32 operands after tests/gpu_util.quant, exact16 operands as
hi + lo / 4096 (pair_value), weights as handed to resr_pack_weights (f16: their f16 rounding; exact16: the fp32 values).  Scalars
(slope, s0, t0, s1, t1, scale) are taken as float32 and then widened: the kernel's constant is the reference's constant.
"""
import numpy as np
import torch

F16_HALF_ULP = 2.0 ** -11 * 1.01    # half an f16 ulp relative to the value (11 significand bits), 1 % slack for the binade's lower end
F16_SUBNORMAL = 2.0 ** -24          # spacing of the f16 subnormals
PAIR_TENSOR_REL = 2e-6              # exact16 outputs: tests/test_gpu_x2_plan.py test_conv_reads_single_chunks_and_writes_single_output


def f32scalar(v, dtype):
    """A descriptor's float field: the float32 nearest to v, widened."""
    return torch.tensor(float(np.float32(v)), dtype=dtype)


def pair_split(t):
    """fp32 [..] -> (hi, lo) f16 tensors of an exact16 pair: hi = f16(v), lo = f16((v - hi) * 4096)."""
    hi = t.half()
    lo = ((t.double() - hi.double()) * 4096.0).half()
    return hi, lo


def pair_value(hi, lo):
    """The exact float64 value of a pair."""
    return hi.double() + lo.double() / 4096.0


def pair_lo_excess(hi, lo):
    """The structure of a STORED pair: lo is a remainder of hi, |lo| / 4096 <= 1.01 * max(2^-11 * |hi|, 2^-25) -- half an f16 ulp of hi
    (below the normal range: half the subnormal spacing), 1 % for lo's own rounding and the binade's lower end.  The passes behind
    rely on it: "hi decides" a sign, the q records take hi's exponent.  Returns the number of elements that break it."""
    hi, lo = hi.double().abs(), lo.double().abs()
    return int((~(lo / 4096.0 <= 1.01 * torch.clamp(2.0 ** -11 * hi, min=2.0 ** -25))).sum())


def split_weights(wt):
    """The three f16 blocks resr_pack_weights keeps of an exact16 weight (include/resr.h), as float64 in the weight's own scale:
    (W0, W1, W2) = (f16(w * 2^12), f16(w * 2^12 - W0), f16(W0 * 2^-12)) -> (W0 / 2^12, W1 / 2^12, W2).  A pair chunk computes
    x_hi (W0 + W1) + x_lo W2, a single chunk x (W0 + W1), with RESR_CONV_SINGLE_W16 x W0."""
    t = wt.float() * 4096.0
    w0 = t.half()
    w1 = (t - w0.float()).half()
    w2 = (w0.float() / 4096.0).half()
    return w0.double() / 4096.0, w1.double() / 4096.0, w2.double()


def upsample2(x):
    """Nearest x2: out[.., y, x] = in[.., y // 2, x // 2]."""
    n, c, h, w = x.shape
    return x.reshape(n, c, h, 1, w, 1).expand(n, c, h, 2, w, 2).reshape(n, c, 2 * h, 2 * w)


def _padded(x):
    n, c, h, w = x.shape
    xp = torch.zeros(n, c, h + 2, w + 2, dtype=x.dtype)
    xp[:, :, 1:h + 1, 1:w + 1] = x
    return xp


def correlate(x, wt, dtype=torch.float64, up=False):
    """acc[n,o,y,x] = sum_{c,dy,dx} W[o,c,dy,dx] * in[n,c,y+dy-1,x+dx-1], zero outside the image; `up`: in = nearest x2 of x.

    float32 is evaluated PLAINLY: one fp32 accumulator per output, the 9 * cin products added one after the other.  That is the
    yardstick the allowance needs.  A BLAS evaluation sums in blocks and in several accumulators per output, which no kernel's single
    chain of matrix instructions does; its error against float64 is several times below that of ANY single-accumulator order of the
    same sum (measured on the MI355X with the einsum below as the fp32 yardstick: the f32 kernel, one chain of 9 * cin / 2
    v_mfma_f32_32x32x2_f32 per output, reached 1.5 x A = 6 x e32 on 1e-4 of the elements of rdb_conv3_2seg).  "Another summation
    order" (the factor 4 of A) is meant between such chains.  float64 takes the einsum: its error is nothing at this scale."""
    x, wt = x.to(dtype), wt.to(dtype)
    if up:
        x = upsample2(x)
    n, c, h, w = x.shape
    xp = _padded(x)
    acc = torch.zeros(n, wt.shape[0], h, w, dtype=dtype)
    if dtype == torch.float32:
        for ci in range(c):
            for dy in range(3):
                for dx in range(3):
                    acc.addcmul_(xp[:, ci:ci + 1, dy:dy + h, dx:dx + w], wt[:, ci, dy, dx].view(1, -1, 1, 1))
        return acc
    for dy in range(3):
        for dx in range(3):
            acc += torch.einsum("oc,nchw->nohw", wt[:, :, dy, dx], xp[:, :, dy:dy + h, dx:dx + w])
    return acc


def epilogue(acc, dtype=torch.float64, bias=None, mask=None, slope=0.2, lrelu=False, prelu=None, res0=None, s0=1.0, t0=1.0,
             res1=None, s1=1.0, t1=1.0, clamp=False, with_aux=False):
    """include/resr.h: v = acc + bias; mask / lrelu / prelu / (v*s0 + t0*res0) / (v*s1 + t1*res1) / clamp, in that order.
    Returns (v, v before the clamp); with_aux: (v, v before the clamp, v after the bias and before the mask -- what
    RESR_CONV_AUX_BEFORE_MASK stores --, v after LeakyReLU / PReLU and before the residuals -- RESR_CONV_AUX_BEFORE_RES)."""
    v = acc.to(dtype)
    sl = f32scalar(slope, dtype)
    if bias is not None:
        v = v + bias.to(dtype).view(1, -1, 1, 1)
    before_mask = v
    if mask is not None:
        v = v * torch.where(mask > 0, torch.ones((), dtype=dtype), sl)
    if lrelu:
        v = torch.where(v > 0, v, v * sl)
    if prelu is not None:
        v = torch.where(v > 0, v, v * prelu.to(dtype).view(1, -1, 1, 1))
    before_res = v
    if res0 is not None:
        v = v * f32scalar(s0, dtype) + f32scalar(t0, dtype) * res0.to(dtype)
    if res1 is not None:
        v = v * f32scalar(s1, dtype) + f32scalar(t1, dtype) * res1.to(dtype)
    pre = v
    if clamp:
        v = v.clamp(0.0, 1.0)
    return (v, pre, before_mask, before_res) if with_aux else (v, pre)


def conv3x3(x, wt, dtype=torch.float64, up=False, **epi):
    return epilogue(correlate(x, wt, dtype, up), dtype, **epi)


def wgrad(x, g, scale, dtype=torch.float64, up=False):
    """dW[o,c,dy,dx] = scale * sum_{n,y,x} G[n,o,y,x] * in[n,c,y+dy-1,x+dx-1], db[o] = scale * sum_{n,y,x} G[n,o,y,x]."""
    x, g = x.to(dtype), g.to(dtype)
    if up:
        x = upsample2(x)
    n, c, h, w = x.shape
    xp = _padded(x)
    dw = torch.zeros(g.shape[1], c, 3, 3, dtype=dtype)
    for dy in range(3):
        for dx in range(3):
            dw[:, :, dy, dx] = torch.einsum("nohw,nchw->oc", g, xp[:, :, dy:dy + h, dx:dx + w])
    sc = f32scalar(scale, dtype)
    return dw * sc, g.sum(dim=(0, 2, 3)) * sc


# ---- the 4x4 / stride-2 / padding-1 convolution of the discriminator's DOWN layers (csrc/conv3x3_ws.h SP, csrc/wgrad.hip xsub) --------
# Stated on the ORIGINAL image [N,C,2h,2w] with the [cout,C,4,4] weight: out[Y,X] reads in[2Y + ky - 1, 2X + kx - 1].  Nothing here knows
# the space-to-depth image or the virtual 3x3 kernel the library computes through; s2d / d2s below only carry tensors between the views.
def _taps4(xp, h, w, ky, kx):
    """The h x w pixels in[2Y + ky - 1, 2X + kx - 1] of the image padded by one."""
    return xp[:, :, ky:ky + 2 * h:2, kx:kx + 2 * w:2]


def correlate4x4s2(x, w4, dtype=torch.float64):
    """acc[n,o,Y,X] = sum_{c,ky,kx} W[o,c,ky,kx] * in[n,c,2Y+ky-1,2X+kx-1], zero outside the image; x [N,C,2h,2w] -> [N,cout,h,w].
    float32: one accumulator per output, the 16 * C products one after the other (see correlate)."""
    x, w4 = x.to(dtype), w4.to(dtype)
    n, c, hh, ww = x.shape
    h, w = hh // 2, ww // 2
    xp = _padded(x)
    acc = torch.zeros(n, w4.shape[0], h, w, dtype=dtype)
    if dtype == torch.float32:
        for ci in range(c):
            for ky in range(4):
                for kx in range(4):
                    acc.addcmul_(_taps4(xp[:, ci:ci + 1], h, w, ky, kx), w4[:, ci, ky, kx].view(1, -1, 1, 1))
        return acc
    for ky in range(4):
        for kx in range(4):
            acc += torch.einsum("oc,nchw->nohw", w4[:, :, ky, kx], _taps4(xp, h, w, ky, kx))
    return acc


def conv4x4s2(x, w4, dtype=torch.float64, **epi):
    """conv2d(x, w4, stride 2, padding 1), then the epilogue of include/resr.h."""
    return epilogue(correlate4x4s2(x, w4, dtype), dtype, **epi)


def dgrad4x4s2(g, w4, dtype=torch.float64):
    """The adjoint, conv_transpose2d(g, w4, stride 2, padding 1): gin[n,c,2Y+ky-1,2X+kx-1] += g[n,o,Y,X] * W[o,c,ky,kx];
    g [N,cout,h,w] -> [N,C,2h,2w].  float32: one accumulator per output, its 4 * cout products one after the other."""
    g, w4 = g.to(dtype), w4.to(dtype)
    n, co, h, w = g.shape
    ginp = torch.zeros(n, w4.shape[1], 2 * h + 2, 2 * w + 2, dtype=dtype)
    for ky in range(4):
        for kx in range(4):
            dst = _taps4(ginp, h, w, ky, kx)
            if dtype == torch.float32:
                for o in range(co):
                    dst.addcmul_(g[:, o:o + 1], w4[o, :, ky, kx].view(1, -1, 1, 1))
            else:
                dst += torch.einsum("oc,nohw->nchw", w4[:, :, ky, kx], g)
    return ginp[:, :, 1:2 * h + 1, 1:2 * w + 1].contiguous()


def wgrad4x4s2(x, g, scale, dtype=torch.float64):
    """dW4[o,c,ky,kx] = scale * sum_{n,Y,X} G[n,o,Y,X] * in[n,c,2Y+ky-1,2X+kx-1]; x [N,C,2h,2w], g [N,cout,h,w]."""
    x, g = x.to(dtype), g.to(dtype)
    h, w = g.shape[2:]
    xp = _padded(x)
    dw = torch.zeros(g.shape[1], x.shape[1], 4, 4, dtype=dtype)
    for ky in range(4):
        for kx in range(4):
            dw[:, :, ky, kx] = torch.einsum("nohw,nchw->oc", g, _taps4(xp, h, w, ky, kx))
    return dw * f32scalar(scale, dtype)


def s2d(x):
    """[N,C,2h,2w] -> [N,4C,h,w] in the library's channel order (include/resr.h, resr_space_to_depth): sub-position-major,
    channel (i*2 + j) * C + c of pixel (Y, X) = x[c, 2Y+i, 2X+j]."""
    return torch.cat([x[:, :, i::2, j::2] for i in range(2) for j in range(2)], dim=1)


def d2s(p):
    """The inverse: [N,4C,h,w] -> [N,C,2h,2w]."""
    n, c4, h, w = p.shape
    c = c4 // 4
    x = torch.zeros(n, c, 2 * h, 2 * w, dtype=p.dtype)
    for i in range(2):
        for j in range(2):
            x[:, :, i::2, j::2] = p[:, (i * 2 + j) * c:(i * 2 + j + 1) * c]
    return x


def live_taps(sub, transposed=False):
    """The (ty, tx) taps of the virtual 3x3 kernel that are non-zero for sub-position sub = i*2 + j, from the definition: tap ty of
    sub-row i carries ky = 2 ty + i - 1 when that lies in 0..3.  transposed: the backward-data form (taps flipped, t -> 2 - t)."""
    def axis(i):
        ts = [t for t in range(3) if 0 <= 2 * t + i - 1 < 4]
        return [2 - t for t in ts] if transposed else ts
    return [(ty, tx) for ty in axis(sub >> 1) for tx in axis(sub & 1)]


def live_mask(c):
    """bool [4c,3,3]: True at the 16 live (tap, sub-position) blocks of a [cout,4c,3,3] virtual weight (gradient)."""
    m = torch.zeros(4 * c, 3, 3, dtype=torch.bool)
    for sub in range(4):
        for ty, tx in live_taps(sub):
            m[sub * c:(sub + 1) * c, ty, tx] = True
    return m


# ---- the rule (stated in the module docstring of tests/test_gpu_kernels.py) ------------------------------------------------------
def wgrad_lolo(x, g, scale, up=False):
    """The second term of the exact16 weight-gradient rule, per element of dW: 2^-22 * scale * wgrad(|X|, |G|).  The kernel issues
    three tap-products per product, dW = X_hi^T G_hi + 2^-12 (X_hi^T G_lo + X_lo^T G_hi), and drops X_lo^T G_lo; each lo half is at
    most 2^-11 of its operand (pair_lo_excess), so the dropped product of one pixel is at most 2^-22 |x| |g| and their sum at most
    this.  db has no such term: it is the plain sum of G's two halves."""
    return wgrad(x.abs(), g.abs(), abs(scale), torch.float64, up)[0] * 2.0 ** -22


def allowance(ref64, ref32):
    """(A, e32): e32 = max |ref32 - ref64|, A = max(4 * e32, one fp32 ulp of max |ref64|).  ref32 = None (a "pair" judgement, where A
    plays no part and nobody should pay for the plain fp32 evaluation): (0, 0)."""
    if ref32 is None:
        return 0.0, 0.0
    ref64 = ref64.double()
    e32 = float((ref32.double() - ref64).abs().max())
    floor = float(np.spacing(np.float32(float(ref64.abs().max()))))
    return max(4.0 * e32, floor), e32


def bound(ref64, A, kind, extra=None):
    """The per-element bound on |got - ref64|.  kind: "f32" (any fp32 output; `extra`: a per-element term on top of A -- wgrad_lolo
    for an exact16 dW), "f16" (an f16 store: + half an ulp of the element), "pair" (exact16 pair / exact16 fp32 outputs: the
    per-tensor bound of the x2-plan tests; A plays no part), "pair16" (the hi tensor of an exact16 pass stored alone,
    RESR_CONV_OUT_SINGLE: the pair bound for the value the store rounds + half an f16 ulp of the element for the store, as
    tests/test_gpu_x2_plan.py judges its single-f16 growth planes)."""
    ref64 = ref64.double()
    if kind == "f32":
        return torch.full_like(ref64, A) if extra is None else A + extra.double()
    if kind == "f16":
        return A + torch.clamp(F16_HALF_ULP * ref64.abs(), min=F16_SUBNORMAL)
    pair = PAIR_TENSOR_REL * max(1.0, float(ref64.abs().max()))
    if kind == "pair":
        return torch.full_like(ref64, pair)
    if kind == "pair16":
        return pair + torch.clamp(F16_HALF_ULP * ref64.abs(), min=F16_SUBNORMAL)
    raise ValueError(kind)


def judge(got, ref64, ref32, kind, extra=None):
    """Returns a record {cpu32_err, allowance, kernel_err, ratio, bad, worst}: ratio = max over the tensor of |got - ref64| / bound,
    bad = number of elements beyond their bound (NaNs count), allowance = A (f32, f16) or the tensor bound (pair)."""
    ref64 = ref64.double()
    A, e32 = allowance(ref64, ref32)
    b = bound(ref64, A, kind, extra)
    err = (got.double() - ref64).abs()
    bad = ~(err <= b)
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err / b)
    worst = int(ratio.argmax())
    return {"cpu32_err": e32, "allowance": float(b.min()) if kind.startswith("pair") else A, "kernel_err": float(err.max()), "ratio": float(ratio.max()),
            "bad": int(bad.sum()), "frac_bad": float(bad.double().mean()), "worst": worst, "got": float(got.reshape(-1)[worst]),
            "want": float(ref64.reshape(-1)[worst])}


def pass_mask_ok(got_mask, pre64, A):
    """RESR_CONV_CLAMP01's pass-mask (0 <= v <= 1 before the clamp) may differ from the reference's only where the reference's
    pre-clamp value lies within A of 0 or 1.  Returns the number of elements that differ anywhere else."""
    want = (pre64 >= 0) & (pre64 <= 1)
    near = (pre64.abs() <= A) | ((pre64 - 1.0).abs() <= A)
    return int(((got_mask.bool() != want) & ~near).sum())
