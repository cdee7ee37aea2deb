"""Plain references of the float degradation kernels (csrc/degrade.hip: filter2d, USM backward, resize, noise, JPEG), CPU only.

Every function restates the operation from its DEFINITION in include/resr.h and the reference's imgproc.py on NCHW tensors and shares
no index arithmetic with the kernels.  Each evaluates in the precision it is asked for: float64 is the reference, float32 ON THE
SAME INPUTS, evaluated plainly, is the yardstick tests/conv_ref.py's rule derives its allowance from.  "Plainly": one accumulator per
output, the terms added one after the other in the order the definition lists them (conv_ref.correlate says why no blocked sum will
do).  A kernel's float constants -- (float)(1.0 / scale), weight, the JPEG tables and factors -- are taken as float32 and then widened
(conv_ref.f32scalar): the kernel's constant is the reference's constant.  tests/test_degrade_ref.py checks these references against
torch and shows that the rule rejects wrong kernels before tests/test_gpu_degrade_kernels.py lets it judge a real one.

A few keyword arguments (`pad`, `cubic_a`, `clamp_at_zero`, `area_end`, `left` / `right`, `clip`) name a choice the definition makes;
their defaults ARE the definition, and tests/test_degrade_ref.py sets them wrong, one at a time, to make the kernels the rule has to
reject.
"""
import numpy as np
import torch

from tests.conv_ref import f32scalar

F64, F32 = torch.float64, torch.float32


# ---- filter2d (imgproc.py:1089-1121) -----------------------------------------------------------------------------------------------
def pad_index(n, r, pad="reflect"):
    """Source index of every position -r .. n - 1 + r of an axis of n pixels padded by r: numpy's own padding of 0 .. n - 1.
    "reflect" is the definition (d c b | a b c d | c b a); "edge" and "symmetric" are what a wrong kernel might do."""
    return torch.from_numpy(np.pad(np.arange(n), (r, r), mode=pad).astype(np.int64))


def correlate_reflect(x, k, dtype=F64, pad="reflect"):
    """out[n,c,y,x] = sum_{dy,dx} K[dy,dx] * P[n,c,y+dy,x+dx], P = x reflect-padded by (kh // 2, kw // 2); k: [kh,kw] or [1,kh,kw]
    shared, [N,kh,kw] per sample.  dy outer, dx inner, one accumulator."""
    x, k = x.to(dtype), k.to(dtype)
    if k.dim() == 2:
        k = k.unsqueeze(0)
    n, c, h, w = x.shape
    kh, kw = k.shape[-2:]
    assert k.shape[0] in (1, n)
    p = x.index_select(2, pad_index(h, kh // 2, pad)).index_select(3, pad_index(w, kw // 2, pad))
    acc = torch.zeros(n, c, h, w, dtype=dtype)
    for dy in range(kh):
        for dx in range(kw):
            acc.addcmul_(p[:, :, dy:dy + h, dx:dx + w], k[:, dy, dx].view(-1, 1, 1, 1))
    return acc


# ---- USMSharp backward -------------------------------------------------------------------------------------------------------------
def blur_matrix(n, k1d, dtype=F64, left=True, right=True):
    """The dense [n, n] matrix of "reflect-pad an axis of n by r = len(k1d) // 2, then correlate with k1d": C @ P with P [n + 2r, n]
    the padding (a one per row) and C [n, n + 2r] the band of taps.  Its transpose is the adjoint -- no second derivation of the
    reflection rule.  left / right = False leave the padded rows of that border out (an adjoint that forgets to fold them back)."""
    k1d = k1d.to(dtype)
    r = k1d.numel() // 2
    src = pad_index(n, r)
    P = torch.zeros(n + 2 * r, n, dtype=dtype)
    P[torch.arange(n + 2 * r), src] = 1.0
    if not left:
        P[:r] = 0.0
    if not right:
        P[n + r:] = 0.0
    C = torch.zeros(n, n + 2 * r, dtype=dtype)
    for t in range(k1d.numel()):
        C[torch.arange(n), torch.arange(n) + t] = k1d[t]
    return C @ P


def _apply(M, a, axis, dtype):
    """sum_j M[j, p] * a[.., j, ..] along `axis` (2: rows, 3: columns) = M^T applied to that axis; float32 term after term."""
    if dtype == F64:
        return torch.einsum("jp,ncjw->ncpw", M, a) if axis == 2 else torch.einsum("jp,nchj->nchp", M, a)
    out = torch.zeros_like(a)
    for j in range(M.shape[0]):
        if axis == 2:
            out.addcmul_(a[:, :, j:j + 1, :], M[j].view(1, 1, -1, 1))
        else:
            out.addcmul_(a[:, :, :, j:j + 1], M[j].view(1, 1, 1, -1))
    return out


def usm_backward(x, blur, soft, g, k1d, weight, dtype=F64, clip=True, matrices=None):
    """Gradient of out = soft * clip(x + w (x - B x), 0, 1) + (1 - soft) x with respect to x, soft held constant:
        a = soft * 1[0 <= x + w (x - blur) <= 1] * g,   gx = (1 - soft) g + (1 + w) a - w B^T a,
    B = blur_matrix per axis (columns, then rows), so B^T a = Mh^T a Mw.  matrices = (Mh, Mw) replaces them; clip=False drops the
    indicator."""
    x, blur, soft, g = (t.to(dtype) for t in (x, blur, soft, g))
    w = f32scalar(weight, dtype)
    pre = x + w * (x - blur)
    a = soft * g
    if clip:
        a = torch.where((pre >= 0) & (pre <= 1), a, torch.zeros((), dtype=dtype))
    Mh, Mw = matrices if matrices is not None else (blur_matrix(x.shape[2], k1d, dtype), blur_matrix(x.shape[3], k1d, dtype))
    bta = _apply(Mw.to(dtype), _apply(Mh.to(dtype), a, 2, dtype), 3, dtype)
    return ((1.0 - soft) * g + (1.0 + w) * a) - w * bta


# ---- resize (F.interpolate, align_corners=False, antialias=False) --------------------------------------------------------------------
def _coord_scale(n, on, scale, dtype):
    """1 / scale_factor when the caller gave one (the kernel's (float)(1.0 / scale)), else in / out in the working precision."""
    if scale:
        return f32scalar(1.0 / float(scale), dtype)
    return torch.tensor(float(n), dtype=dtype) / torch.tensor(float(on), dtype=dtype)


def _src(n, on, scale, dtype):
    return _coord_scale(n, on, scale, dtype) * (torch.arange(on, dtype=dtype) + 0.5) - 0.5


def _area_axis(n, on, area_end="ceil"):
    """Window [floor(o n / on), ceil((o + 1) n / on)) of every output, integer arithmetic: (start [on], length [on])."""
    o = np.arange(on, dtype=np.int64)
    start = (o * n) // on
    end = -((-(o + 1) * n) // on) if area_end == "ceil" else np.maximum(((o + 1) * n) // on, start + 1)
    return torch.from_numpy(start), torch.from_numpy(end - start)


def _cubic_weights(t, A):
    def c1(v):
        return ((A + 2.0) * v - (A + 3.0)) * v * v + 1.0

    def c2(v):
        return ((A * v - 5.0 * A) * v + 8.0 * A) * v - 4.0 * A
    return [c2(t + 1.0), c1(t), c1(1.0 - t), c2(2.0 - t)]


def _gather(x, iy, ix):
    return x.index_select(2, iy).index_select(3, ix)


def resize(x, oh, ow, mode, scale=None, dtype=F64, cubic_a=-0.75, clamp_at_zero=True, area_end="ceil"):
    """mode "area": the mean over the window of _area_axis (rows outer, columns inner, then one division by the count);
    "bilinear": source coordinate s (o + 0.5) - 0.5 clamped at 0, hy (hx p00 + lx p01) + ly (hx p10 + lx p11), the +1 neighbour
    clamped to the last pixel; "bicubic": A = -0.75, the four tap indices clamped, sum_a cy[a] (sum_b cx[b] p[a][b]).
    scale: the scale_factor the caller gave (coordinates use 1 / scale), None for size= (in / out)."""
    x = x.to(dtype)
    n, c, h, w = x.shape
    if mode == "area":
        (y0, ly), (x0, lx) = _area_axis(h, oh, area_end), _area_axis(w, ow, area_end)
        acc = torch.zeros(n, c, oh, ow, dtype=dtype)
        zero = torch.zeros((), dtype=dtype)
        for a in range(int(ly.max())):
            for b in range(int(lx.max())):
                inside = (a < ly).view(-1, 1) & (b < lx).view(1, -1)
                term = _gather(x, (y0 + a).clamp(max=h - 1), (x0 + b).clamp(max=w - 1))
                acc += torch.where(inside, term, zero)                 # (+0 leaves an accumulator as it is)
        return acc / (ly.view(-1, 1) * lx.view(1, -1)).to(dtype)
    fy, fx = _src(h, oh, scale, dtype), _src(w, ow, scale, dtype)
    if mode == "bilinear":
        if clamp_at_zero:
            fy, fx = fy.clamp(min=0), fx.clamp(min=0)
        iy, ix = fy.trunc(), fx.trunc()          # (the integer part as a C cast takes it; the floor, once the coordinate is clamped)
        ly, lx = (fy - iy).view(-1, 1), (fx - ix).view(1, -1)
        hy, hx = 1.0 - ly, 1.0 - lx
        iy, ix = iy.long(), ix.long()
        y0, x0 = iy.clamp(0, h - 1), ix.clamp(0, w - 1)
        y1, x1 = (iy + 1).clamp(0, h - 1), (ix + 1).clamp(0, w - 1)
        return hy * (hx * _gather(x, y0, x0) + lx * _gather(x, y0, x1)) + ly * (hx * _gather(x, y1, x0) + lx * _gather(x, y1, x1))
    if mode == "bicubic":
        iy, ix = fy.floor(), fx.floor()
        cy, cx = _cubic_weights(fy - iy, cubic_a), _cubic_weights(fx - ix, cubic_a)
        iy, ix = iy.long(), ix.long()
        out = torch.zeros(n, c, oh, ow, dtype=dtype)
        for a in range(4):
            row = torch.zeros(n, c, oh, ow, dtype=dtype)
            ya = (iy - 1 + a).clamp(0, h - 1)
            for b in range(4):
                row += cx[b].view(1, -1) * _gather(x, ya, (ix - 1 + b).clamp(0, w - 1))
            out += cy[a].view(-1, 1) * row
        return out
    raise ValueError(mode)


# ---- noise (imgproc.py:829-1086) -----------------------------------------------------------------------------------------------------
def pre_round(v, dtype=F64):
    """v * 255, the value modes 2 and 3 round."""
    return v.to(dtype) * 255.0


def finish(v, mode, dtype=F64):
    """imgproc.py:1050-1055: bit 0 = clip, bit 1 = rounds.  0: v; 1: clamp(v, 0, 1); 2: round(255 v) / 255; 3: clamp(round(255 v), 0, 255) / 255
    (round: half to even)."""
    v = v.to(dtype)
    if mode == 0:
        return v
    if mode == 1:
        return v.clamp(0.0, 1.0)
    if mode == 2:
        return torch.round(v * 255.0) / 255.0
    if mode == 3:
        return torch.round(v * 255.0).clamp(0.0, 255.0) / 255.0
    raise ValueError(mode)


def gaussian_noisy(x, sigma, gray, fg, fc, dtype=F64):
    """x + noise before the finish: noise = fc * sigma / 255, and where a gray field is given noise (1 - gray) + (fg * sigma / 255) gray
    with fg [h, w] ONE field for the whole batch (imgproc.py:854-861)."""
    x, fc = x.to(dtype), fc.to(dtype)
    b = x.shape[0]
    s, gr = sigma.to(dtype).view(b, 1, 1, 1), gray.to(dtype).view(b, 1, 1, 1)
    noise = fc * s / 255.0
    if fg is not None:
        noise = noise * (1.0 - gr) + (fg.to(dtype).view(1, 1, *x.shape[2:]) * s / 255.0) * gr
    return x + noise


def gaussian_noise(x, sigma, gray, fg, fc, mode, dtype=F64):
    return finish(gaussian_noisy(x, sigma, gray, fg, fc, dtype), mode, dtype)


def _coef(v):
    return float(np.float32(v))


def gray255(x, dtype=F64):
    """255 * (0.2989 r + 0.587 g + 0.114 b) of [N,3,H,W] -> [N,1,H,W], the value the gray branch rounds to its level."""
    x = x.to(dtype)
    return (_coef(0.2989) * x[:, 0:1] + _coef(0.587) * x[:, 1:2] + _coef(0.114) * x[:, 2:3]) * 255.0


def _level(v255):
    """clamp(round(.), 0, 255) / 255 as the kernel holds it: a float32, widened."""
    return (torch.round(v255).clamp(0.0, 255.0).float() / 255.0).double()


def poisson_decode(x, out, scale, gray, vals):
    """The counts a mode-0 resr_noise_poisson output holds.  out = x + scale * noise with, per sample, noise = P(q v) / v - q per
    channel (gray = 0) or P(gq vg) / vg - gq in all three (gray = 1); q, gq = the image's / its gray's 8-bit level, (v, vg) = vals[b].
    Returns (colour [N,3,H,W], gray [N,1,H,W]) in float64: ((out - x) / scale + q) v and ((out - x)[:, :1] / scale + gq) vg.  Only
    the one that belongs to a sample's gray flag holds its draws."""
    x, out = x.double(), out.double()
    b = x.shape[0]
    sc = scale.double().view(b, 1, 1, 1)
    v, vg = vals[:, 0].double().view(b, 1, 1, 1), vals[:, 1].double().view(b, 1, 1, 1)
    d = (out - x) / sc
    return (d + _level(x * 255.0)) * v, (d[:, 0:1] + _level(gray255(x))) * vg


# ---- DiffJPEG(differentiable=False) (imgproc.py:1195-1494) ------------------------------------------------------------------------------
def jpeg_factor(quality):
    """The kernel's float32 quality factor (imgproc.py:1134-1139), widened: [N] float64."""
    q = np.asarray(quality, dtype=np.float32)
    lo = (np.float32(5000.0) / q) / np.float32(100.0)
    hi = (np.float32(200.0) - q * np.float32(2.0)) / np.float32(100.0)
    return torch.from_numpy(np.where(q < 50, lo, hi).astype(np.float32)).double()


def jpeg_preround(x, quality):
    """The DCT coefficient over its quantisation step BEFORE the rounding, float64, in resr_jpeg's layout [N, blocks, 64]: per image
    the Y blocks (row-major over the size padded with zeros to multiples of 16), then Cb, then Cr (2 x 2 means), u * 8 + v inside.
    Tables, basis and colour matrix are those of oracle/imgproc_ref.py (float32, widened); step = float32(table * factor)."""
    from oracle import imgproc_ref as I
    import torch.nn.functional as F
    x = x.double()
    b, _, h, w = x.shape
    hp, wp = (16 - h % 16) % 16, (16 - w % 16) % 16
    p = F.pad(x, (0, wp, 0, hp)) * 255.0
    ycc = torch.tensordot(p.permute(0, 2, 3, 1), I._RGB2YCC.double(), dims=1) + torch.tensor([0.0, 128.0, 128.0], dtype=F64)
    planes = [ycc[..., 0]] + [F.avg_pool2d(ycc[..., i].unsqueeze(1), 2).squeeze(1) for i in (1, 2)]
    factor = jpeg_factor(quality).float().view(b, 1, 1, 1)
    out = []
    for plane, table in zip(planes, (I.Y_TABLE, I.C_TABLE, I.C_TABLE)):
        dct = I._DCT_SCALE.double() * torch.tensordot(I._blocks(plane) - 128.0, I._DCT_T.double(), dims=2)
        step = (table.view(1, 1, 8, 8) * factor).double()               # the float32 product, widened
        out.append((dct / step).reshape(b, -1, 64))
    return torch.cat(out, dim=1)


# ---- the cases both test modules run (tests/test_degrade_ref.py: the rule's power; tests/test_gpu_degrade_kernels.py: the kernels) ------
def signed_kernel(kh, kw, gen, count=None):
    """Taps with negative lobes (a sinc kernel has them), no symmetry of any kind, normalised to sum 1; [kh,kw] or [count,kh,kw]."""
    shape = (kh, kw) if count is None else (count, kh, kw)
    k = torch.rand(shape, generator=gen) + 0.05
    k = torch.where(torch.rand(shape, generator=gen) < 0.25, -0.3 * k, k)
    return k / k.sum(dim=(-2, -1), keepdim=True)


def core_kernel21(cores, gen):
    """[len(cores), 21, 21]: a signed core of cores[i] x cores[i] taps in a border of zeros (dataset.py:101-103 pads every blur kernel so)."""
    k = torch.zeros(len(cores), 21, 21)
    for i, s in enumerate(cores):
        lo = 10 - s // 2
        k[i, lo:lo + s, lo:lo + s] = signed_kernel(s, s, gen)
    return k


# name -> (image shape, kh, kw, per_sample, "dense" or the core sizes of a zero-padded 21 x 21)
FILTER_CASES = {
    "g1x1": ((2, 3, 5, 7), 1, 1, 0, "dense"),
    "g3x3": ((2, 3, 5, 7), 3, 3, 0, "dense"),
    "g1x3": ((2, 3, 5, 7), 1, 3, 0, "dense"),
    "g3x1": ((2, 3, 5, 7), 3, 1, 0, "dense"),
    "g5x9": ((1, 2, 33, 65), 5, 9, 0, "dense"),
    "g9x5": ((1, 2, 33, 65), 9, 5, 0, "dense"),
    "g9x5_per_sample": ((2, 1, 33, 65), 9, 5, 1, "dense"),
    "g7x7_pad_is_h_minus_1": ((1, 1, 4, 4), 7, 7, 0, "dense"),
    "g63x63": ((1, 1, 33, 40), 63, 63, 0, "dense"),
    "g1x51_per_sample": ((2, 1, 40, 56), 1, 51, 1, "dense"),        # per-sample: not the shared 51-tap kernel's case
    "g51x1_per_sample": ((2, 1, 56, 40), 51, 1, 1, "dense"),
    "row51_26x26": ((1, 1, 26, 26), 1, 51, 0, "dense"),
    "col51_26x26": ((1, 1, 26, 26), 51, 1, 0, "dense"),
    "row51_33x65": ((1, 2, 33, 65), 1, 51, 0, "dense"),
    "col51_33x65": ((1, 2, 33, 65), 51, 1, 0, "dense"),
    "row51_100x35": ((1, 1, 100, 35), 1, 51, 0, "dense"),
    "col51_100x35": ((1, 1, 100, 35), 51, 1, 0, "dense"),
}
for _tag, _shape in (("11x11", (1, 1, 11, 11)), ("one_tile", (2, 3, 32, 64)), ("33x65", (1, 2, 33, 65)), ("70x130", (1, 1, 70, 130))):
    for _ps in (0, 1):
        FILTER_CASES[f"k21_{_tag}_{'per_sample' if _ps else 'shared'}_dense"] = (_shape, 21, 21, _ps, "dense")
        FILTER_CASES[f"k21_{_tag}_{'per_sample' if _ps else 'shared'}_core"] = (_shape, 21, 21, _ps, (7, 13)[:_shape[0]] if _ps else (7,))


def filter_case(name):
    """(x [N,C,H,W], k [1 or N, kh, kw]) of a FILTER_CASES entry, fp32."""
    shape, kh, kw, per_sample, kind = FILTER_CASES[name]
    gen = torch.Generator().manual_seed(sorted(FILTER_CASES).index(name) + 100)
    x = torch.rand(shape, generator=gen)
    k = signed_kernel(kh, kw, gen, shape[0] if per_sample else 1) if kind == "dense" else core_kernel21(kind, gen)
    return x, k


# name -> (image shape, scale_factor or None, size or None); every case runs in all three modes
RESIZE_CASES = {
    "33x65_up3.7": ((1, 2, 33, 65), 3.7, None),
    "33x65_down0.15": ((1, 2, 33, 65), 0.15, None),
    "48x40_to_97x5": ((2, 3, 48, 40), None, (97, 5)),
    "48x40_to_1x1": ((2, 3, 48, 40), None, (1, 1)),
    "one_row_to_5x5": ((1, 1, 1, 7), None, (5, 5)),
    "one_column_to_5x5": ((1, 1, 7, 1), None, (5, 5)),
    "2x2_to_9x9": ((1, 1, 2, 2), None, (9, 9)),
    "seven_planes_9x11_to_4x13": ((7, 1, 9, 11), None, (4, 13)),
}
RESIZE_MODES = ("area", "bilinear", "bicubic")


def resize_case(name):
    """(x, oh, ow, scale) of a RESIZE_CASES entry; output size of a scale factor as F.interpolate takes it: floor(in * scale)."""
    import math
    shape, scale, size = RESIZE_CASES[name]
    x = torch.rand(shape, generator=torch.Generator().manual_seed(sorted(RESIZE_CASES).index(name) + 200))
    oh, ow = size if size is not None else (int(math.floor(shape[2] * scale)), int(math.floor(shape[3] * scale)))
    return x, oh, ow, scale


# name -> (image shape, ksize)
USM_BWD_CASES = {
    "26x26_k51": ((1, 1, 26, 26), 51),
    "40x56_k51": ((2, 3, 40, 56), 51),
    "33x65_k51": ((1, 2, 33, 65), 51),
    "100x27_k51": ((1, 1, 100, 27), 51),
    "3x9_k5": ((1, 1, 3, 9), 5),
}
USM_WEIGHT = 0.5


def usm_bwd_case(name):
    """(x, blur, soft, g, k1d) fp32: x in [0,1], soft in [0,1], and a blur chosen so that pre = x + w (x - blur) falls, a third of the
    elements each, into [-0.4, -0.01], [0.01, 0.99] and [1.01, 1.4] -- both sides of both clip edges, nowhere near one.  The taps are
    signed and asymmetric: an adjoint that runs them backwards is a different function."""
    shape, ksize = USM_BWD_CASES[name]
    gen = torch.Generator().manual_seed(sorted(USM_BWD_CASES).index(name) + 300)
    x, soft, g = torch.rand(shape, generator=gen), torch.rand(shape, generator=gen), torch.randn(shape, generator=gen)
    band = torch.randint(0, 3, shape, generator=gen)
    u = torch.rand(shape, generator=gen)
    pre = torch.where(band == 0, -0.4 + 0.39 * u, torch.where(band == 1, 0.01 + 0.98 * u, 1.01 + 0.39 * u))
    blur = x - (pre - x) / USM_WEIGHT
    return x, blur, soft, g, signed_kernel(1, ksize, gen).reshape(ksize)


def usm_pre(x, blur):
    """x + w (x - blur) in float64, the value whose position against 0 and 1 the backward's indicator reads."""
    w = f32scalar(USM_WEIGHT, F64)
    return x.double() + w * (x.double() - blur.double())
