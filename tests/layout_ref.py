"""Plain references of the layout, pool, pack, EMA and scalar-loss kernels (csrc/layout.hip, csrc/pack.hip, the first two kernels of
csrc/loss.hip), CPU only, the case tables of tests/test_gpu_layout_kernels.py, and the rule that judges a kernel against them.

Every reference restates an operation from its DEFINITION -- the comments of include/resr.h and csrc/common.h, the format text at the
top of csrc/packed_layout.h, torch's documentation of pixel_(un)shuffle -- on numpy arrays, with slices, reshapes and transposes where
the kernels do index arithmetic.  tests/test_layout_ref.py checks them against torch and shows, at the shapes listed here, that the
rule rejects wrong kernels before the GPU module lets it judge a real one.

The rule
  * a conversion, a permutation, a power-of-two scale, a maximum, a fixed two-products-one-sum: BIT FOR BIT (same_bits).  NaNs are
    compared as "is a NaN": the payload and sign a conversion or inf - inf leaves are the hardware's, not part of any definition here.
  * a sum (sumpool2x2, the pair add, the loss values): against float64 with tests/conv_ref.py's allowance A = max(4 e32, one fp32 ulp
    of max |ref64|), e32 the plain fp32 restatement's own error on the same inputs, and conv_ref.bound in kinds "f32", "f16", "pair".
  * BCE: the kernel evaluates exp(-|x|) as exp2(-|x| * log2 e) with a fast exp2 (by design).  Rounding the product moves the argument
    by at most |x| log2(e) 2^-24, i.e. t = exp(-|x|) by the relative |x| 2^-24; a one-ulp exp2 and the rounding of the result add
    2 * 2^-24: |dt| <= t (|x| + 2) 2^-24.  Through s = 1 / (1 + t) (or t / (1 + t)) that is |ds| <= s (1 - s) (|x| + 2) 2^-24, so a
    gradient element may lie A + gscale s (1 - s) (|x| + 2) 2^-24 from float64; through log1p(t) it is t / (1 + t) = sigmoid(-|x|)
    times the same, and the loss value gets weight * mean_i sigmoid(-|x_i|) (|x_i| + 2) 2^-24 on top of A.
"""
import math

import numpy as np
import torch

from tests import conv_ref as C
from tests import disc_helpers_ref as D

F32, F16, F64 = np.float32, np.float16, np.float64
LO = F32(4096.0)
LO_INV = F32(1.0 / 4096.0)
BACKOFF_STEP, BACKOFF_MAX = 4, 40          # csrc/common.h: "lowers the target by 2^4 (up to 2^40 ...)"
U32 = {2: np.uint16, 4: np.uint32, 1: np.uint8}


# ---- conversions -------------------------------------------------------------------------------------------------------------------
def f16_rne(v32):
    """fp32 -> f16, one rounding to nearest even (numpy's conversion; subnormals kept, beyond 65520 infinity)."""
    with np.errstate(over="ignore"):
        return np.asarray(v32, dtype=F32).astype(F16)


def pair_split(v32):
    """conv_ref.pair_split on a numpy fp32 array: hi = f16(v), lo = f16((v - hi) * 4096)."""
    hi, lo = C.pair_split(torch.from_numpy(np.ascontiguousarray(np.asarray(v32, dtype=F32))))
    return hi.numpy(), lo.numpy()


def pair_value(hi, lo):
    """conv_ref.pair_value: the exact float64 value."""
    return C.pair_value(torch.from_numpy(np.ascontiguousarray(hi)), torch.from_numpy(np.ascontiguousarray(lo))).numpy()


def pair_load32(hi, lo):
    """What a kernel loads from a pair: one fma, the single fp32 rounding of the exact value."""
    with np.errstate(invalid="ignore"):
        return pair_value(hi, lo).astype(F32)


def bf8_bits(h16):
    """e5m2 byte of an f16: the 16-bit pattern rounded to its upper byte, nearest, ties to the even byte."""
    p = np.ascontiguousarray(h16, dtype=F16).view(np.uint16).astype(np.uint32)
    upper, rest = p >> 8, p & 0xFF
    up = (rest > 0x80) | ((rest == 0x80) & ((upper & 1) == 1))
    return ((upper + up) & 0xFF).astype(np.uint8)


def store(kind, v32):
    """One rounding of fp32 results to the stored form: {"hi": ..} and for f16x2 {"hi", "lo"}."""
    v32 = np.asarray(v32, dtype=F32)
    if kind == "f32":
        return {"hi": v32}
    if kind == "f16":
        return {"hi": f16_rne(v32)}
    hi, lo = pair_split(v32)
    return {"hi": hi, "lo": lo}


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def bits_differ(got, want, sentinel=None):
    """Indices where got and want differ: in bits where want is a number, in NaN-ness where it is a NaN (a `sentinel` pattern, the
    pre-fill of an output buffer, never counts as that NaN)."""
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    assert got.dtype == want.dtype and got.size == want.size, (got.dtype, want.dtype, got.size, want.size)
    u = U32[got.dtype.itemsize]
    gb, wb = got.view(u), want.view(u)
    if got.dtype.kind != "f":
        return np.flatnonzero(gb != wb)
    wn, gn = np.isnan(want), np.isnan(got)
    if sentinel is not None:
        gn = gn & (gb != u(sentinel))
    return np.flatnonzero(np.where(wn, ~gn, gb != wb))


def judge(got, ref64, ref32, kind, extra=None):
    """conv_ref.judge on numpy arrays.  extra: a per-element (or scalar) term added to the bound (the BCE exp term); the record then
    holds `ratio` against the full bound and `ratio_plain` against the bound without it."""
    t = lambda a: torch.from_numpy(np.array(a, dtype=F64).reshape(-1))
    got, ref64, ref32 = t(got), t(ref64), t(ref32)
    rec = C.judge(got, ref64, ref32, kind)
    if extra is not None:
        A, _ = C.allowance(ref64, ref32)
        plain = C.bound(ref64, A, kind)
        b = plain + t(np.broadcast_to(np.asarray(extra, dtype=F64), tuple(ref64.shape)))
        err = (got - ref64).abs()
        rec["ratio_plain"] = rec["ratio"]
        rec["ratio"] = float(torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err / b).max())
        rec["bad"] = int((~(err <= b)).sum())
        rec["exp_term"] = float(b.max() - plain.max())
    return rec


# ---- pixel (un)shuffle, prescale, the layout passes ---------------------------------------------------------------------------------
def pixel_unshuffle(x, r):
    """torch.nn.PixelUnshuffle: [n,c,h,w] -> [n, c r^2, h/r, w/r], out[:, ch r^2 + i r + j, y, x] = in[:, ch, y r + i, x r + j]."""
    n, c, h, w = x.shape
    out = np.empty((n, c * r * r, h // r, w // r), dtype=x.dtype)
    for ch in range(c):
        for i in range(r):
            for j in range(r):
                out[:, ch * r * r + i * r + j] = x[:, ch, i::r, j::r]
    return out


def pixel_shuffle(x, r):
    """torch.nn.PixelShuffle, the inverse: [n, c r^2, h, w] -> [n, c, h r, w r]."""
    n, cr, h, w = x.shape
    c = cr // (r * r)
    out = np.empty((n, c, h * r, w * r), dtype=x.dtype)
    for ch in range(c):
        for i in range(r):
            for j in range(r):
                out[:, ch, i::r, j::r] = x[:, ch * r * r + i * r + j]
    return out


def bits_to_float(bits):
    return float(np.array([bits], dtype=np.uint32).view(F32)[0])


def float_to_bits(v):
    return int(np.array([v], dtype=F32).view(np.uint32)[0])


def grad_prescale(amax_bits, inverse=False):
    """csrc/common.h: with m the float whose bits the slot holds, s = 2^-floor(log2 m) when 2^-126 <= m < 1, else 1 (zero, subnormal,
    m >= 1, inf and NaN alike); inverse: 1 / s."""
    if amax_bits is None:
        return F32(1.0)
    m = bits_to_float(amax_bits & 0x7FFFFFFF)
    if not (2.0 ** -126 <= m < 1.0):
        return F32(1.0)
    _, e = math.frexp(m)                      # m = f * 2^e, 0.5 <= f < 1: floor(log2 m) = e - 1
    return F32(math.ldexp(1.0, e - 1 if inverse else 1 - e))


def nchw_to_nhwc(src, r, c_pad, kind, mask=None, amax_bits=None, q=False):
    """resr_nchw_to_nhwc: src [n,c,h,w] fp32 times the prescale, zero where the pass mask is zero, pixel-unshuffled by r, pixel-major
    with the channels padded with zeros to c_pad, converted once.  Returns {"hi", ["lo"], ["q"]}: [n, h/r, w/r, c_pad]; q (bytes):
    [n, h/r, w/r, c_pad/32, 64], per pixel and 32-channel chunk byte c = bf8(hi[c]), byte 32 + c = bf8(lo[c])."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.asarray(src, dtype=F32) * grad_prescale(amax_bits)
    if mask is not None:
        v = np.where(np.asarray(mask) != 0, v, F32(0.0))
    u = pixel_unshuffle(v, r)
    n, cr, ho, wo = u.shape
    full = np.zeros((n, ho, wo, c_pad), dtype=F32)
    full[..., :cr] = np.moveaxis(u, 1, 3)
    out = store(kind, full)
    if q:
        out["q"] = q_records(out["hi"], out["lo"])
    return out


def q_records(hi, lo):
    """The q tensor of a pair [.., c_pad] (include/resr.h, ResrConvDesc): [.., c_pad / 32, 64] bytes, per pixel and 32-channel chunk
    byte c = bf8(hi[c]), byte 32 + c = bf8(lo[c])."""
    chunks = hi.shape[-1] // 32
    rec = np.empty(hi.shape[:-1] + (chunks, 64), dtype=np.uint8)
    for k in range(chunks):
        rec[..., k, :32] = bf8_bits(hi[..., 32 * k:32 * k + 32])
        rec[..., k, 32:] = bf8_bits(lo[..., 32 * k:32 * k + 32])
    return rec


def nhwc_to_nchw(v32, c, r, amax_bits=None):
    """resr_nhwc_to_nchw: v32 [n,ho,wo,stride], the fp32 values the kernel loads; the first c r^2 channels, pixel-shuffled, times 1 / s."""
    x = np.moveaxis(np.asarray(v32, dtype=F32)[..., :c * r * r], 3, 1)
    with np.errstate(over="ignore", invalid="ignore"):
        return pixel_shuffle(x, r) * grad_prescale(amax_bits, inverse=True)


# ---- absmax ------------------------------------------------------------------------------------------------------------------------
def absmax_slot(values, target_log2, slot1=0, slot2=0):
    """The three slot words after absmax and its back-off, as (bits of m or "nan", b, flag).  m = max |v| * 2^-t in fp32 (a NaN beats
    every number); b = min(slot1, 40), raised by 4 (to 40 at most) when the flag is set, the flag consumed; a NORMAL m leaves times 2^b
    with its exponent field held at 254 (zero, subnormal, inf, NaN stay)."""
    v = np.abs(np.asarray(values, dtype=F32).reshape(-1))
    b = min(int(slot1), BACKOFF_MAX)
    if slot2:
        b = min(b + BACKOFF_STEP, BACKOFF_MAX)
    if np.isnan(v).any():
        return "nan", b, 0
    with np.errstate(over="ignore", under="ignore"):
        m = float(F32(v.max()) * F32(math.ldexp(1.0, -target_log2)))
    if b and 2.0 ** -126 <= m < math.inf:
        f, e = math.frexp(m)
        m = math.ldexp(f, min(e + b, 128))    # [2^127, 2^128): the largest finite binade
    return float_to_bits(m), b, 0


# ---- sumpool2x2, add_inplace, EMA --------------------------------------------------------------------------------------------------
def sumpool2x2(x, positive=None, slope=0.2, dtype=F64):
    """out[n,y,x,c] = sum of the 2 x 2 window of x [n,2ho,2wo,c] (the backward of nearest x2), times slope where the saved activation
    is not positive.  float32 is evaluated plainly: one accumulator, the four taps in reading order."""
    x = np.asarray(x, dtype=dtype)
    acc = np.zeros(x[:, 0::2, 0::2].shape, dtype=dtype)
    for dy in range(2):
        for dx in range(2):
            acc = acc + x[:, dy::2, dx::2]
    if positive is not None:
        acc = acc * np.where(positive, dtype(1.0), dtype(F32(slope)))
    return acc


def add_plain(a, b):
    """add_inplace, f32 / f16: the fp32 sum of the two stored values, rounded once to the tensor's type."""
    return (np.asarray(a).astype(F32) + np.asarray(b).astype(F32)).astype(np.asarray(a).dtype)


def add_pair32(ahi, alo, bhi, blo):
    """add_inplace on pairs in plain fp32: the sum of the hi parts plus 2^-12 times the sum of the lo parts."""
    f = lambda t: np.asarray(t).astype(F32)
    return (f(ahi) + f(bhi)) + (f(alo) + f(blo)) * LO_INV


def ema(shadow, p, decay):
    """EMA.update: (1 - decay) * p + decay * shadow as two rounded fp32 products and one rounded sum; decay is a double, its
    complement is taken in double, both are then fp32 constants."""
    om, d = F32(1.0 - float(decay)), F32(float(decay))
    a = om * np.asarray(p, dtype=F32)
    b = d * np.asarray(shadow, dtype=F32)
    return a + b


# ---- the scalar losses -------------------------------------------------------------------------------------------------------------
def seq_sum32(a):
    return np.cumsum(np.asarray(a, dtype=F32).reshape(-1), dtype=F32)[-1]


def gscale32(weight, count):
    """weight / count as the kernels hold it: one fp32 division of the two fp32 numbers."""
    return F32(weight) / F32(count)


def l1_mean(a, b, weight, dtype=F64, sign0=0.0):
    """(loss, grad): weight * mean |a - b| and weight / count * sign(a - b), sign(0) = 0.  float32: a plain left-to-right sum."""
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    d = a - b
    if dtype == F64:
        g = float(F32(weight)) / a.size
        return np.abs(d).sum() * g, np.where(d > 0, g, np.where(d < 0, -g, sign0 * g))
    g = gscale32(weight, a.size)
    return seq_sum32(np.abs(d)) * g, np.where(d > 0, g, np.where(d < 0, -g, F32(sign0) * g)).astype(F32)


def bce_const(x, label, weight, dtype=F64):
    """(loss, grad): weight * mean_i [max(x, 0) - x label + log1p(exp(-|x|))], weight / count * (sigmoid(x) - label)."""
    x = np.asarray(x, dtype=dtype)
    lab = dtype(label)
    t = np.exp(-np.abs(x))
    li = np.maximum(x, dtype(0)) - x * lab + np.log1p(t)
    s = np.where(x >= 0, dtype(1) / (dtype(1) + t), t / (dtype(1) + t))
    if dtype == F64:
        g = float(F32(weight)) / x.size
        return li.sum() * g, (s - lab) * g
    g = gscale32(weight, x.size)
    return seq_sum32(li) * g, ((s - lab) * g).astype(F32)


def bce_exp_terms(x, weight):
    """(per-element term of the gradient bound, term of the loss bound): module docstring."""
    x = np.asarray(x, dtype=F64)
    g = float(F32(weight)) / x.size
    t = np.exp(-np.abs(x))
    s = 1.0 / (1.0 + t)
    rel = (np.abs(x) + 2.0) * 2.0 ** -24
    return g * s * (1.0 - s) * rel, g * float(((1.0 - s) * rel).sum())


# ---- packed weights ----------------------------------------------------------------------------------------------------------------
class Chunk:
    """One row of a pack table (include/resr.h, ResrPackChunk); scale_value: what *scale_ptr holds, or None."""

    def __init__(self, src_off, dst_off, src_cout, src_cin, m_off, m_count, k_off, k_count, mt, transposed=0, scale=1.0, virtual4x4=0,
                 scale_value=None):
        self.src_off, self.dst_off, self.src_cout, self.src_cin = src_off, dst_off, src_cout, src_cin
        self.m_off, self.m_count, self.k_off, self.k_count, self.mt = m_off, m_count, k_off, k_count, mt
        self.transposed, self.scale, self.virtual4x4, self.scale_value = transposed, scale, virtual4x4, scale_value


def block_elems(mt):
    return 9 * mt * 1024


def chunk_weights(arena, ch, flip=True, exact_product=False):
    """The fp32 elements a chunk holds, [9 taps, 32 mt M rows, 32 K channels], zeros beyond the real rows / channels.  Forward: M = cout,
    K = cin.  Transposed: M = cin, K = cout, taps flipped (the convolution's adjoint).  virtual4x4: the source is [cout, C, 4, 4] and
    enters as its virtual 3 x 3 kernel over the space-to-depth image (disc_helpers_ref.virtual_ref).  Every element times
    scale * *scale_ptr, one fp32 product of the two, one fp32 product with the weight."""
    taps = 16 if ch.virtual4x4 else 9
    w = np.asarray(arena, dtype=F32)[ch.src_off:ch.src_off + ch.src_cout * ch.src_cin * taps]
    if ch.virtual4x4:
        w = D.virtual_ref(w.reshape(ch.src_cout, ch.src_cin, 4, 4)).reshape(ch.src_cout, 4 * ch.src_cin, 9)
    else:
        w = w.reshape(ch.src_cout, ch.src_cin, 9)
    if ch.transposed:
        w = np.swapaxes(w, 0, 1)
        if flip:
            w = w[:, :, ::-1]
    part = w[ch.m_off:ch.m_off + ch.m_count, ch.k_off:ch.k_off + ch.k_count]
    sc = F32(ch.scale) * (F32(ch.scale_value) if ch.scale_value is not None else F32(1.0))
    full = np.zeros((9, 32 * ch.mt, 32), dtype=F64 if exact_product else F32)
    full[:, :ch.m_count, :ch.k_count] = np.moveaxis(part, 2, 0).astype(full.dtype) * full.dtype.type(sc)   # (float64 holds the product of two fp32 exactly)
    return full


def exact16_blocks(v32):
    """W0 = f16(w 2^12), W1 = f16(w 2^12 - W0), W2 = f16(W0 2^-12), every step in fp32."""
    t = np.asarray(v32, dtype=F32) * LO
    w0 = f16_rne(t)
    return w0, f16_rne(t - w0.astype(F32)), f16_rne(w0.astype(F32) * LO_INV)


def unpack_block(flat, mt):
    """A packed block of 9 * mt * 1024 elements as [tap, M row, K channel].  The order (packed_layout.h): tap -> k-step -> M tile ->
    lane (kh * 32 + m) -> 16 bytes, a lane's 16 bytes holding E consecutive K channels and the two kh halves of a k-step 2 E."""
    flat = np.asarray(flat)
    e = 16 // flat.dtype.itemsize
    ks = 32 // (2 * e)
    a = flat.reshape(9, ks, mt, 2, 32, e)                   # tap, k-step, M tile, kh, m, element
    return a.transpose(0, 2, 4, 1, 3, 5).reshape(9, mt * 32, 32)


def unpack_mx_block(raw, mt):
    """An MX block of 9 * mt * 2048 bytes as [tap, M row, 64]: per tap and row [bf8(W1[k]), k = 0..31 | bf8(W2[k])].  The order
    (include/resr.h, resr_pack_weights_mx): 16-byte piece ((tap * 2 + p) * mt + tile) * 64 + h * 32 + row holds K = 16 h .. 16 h + 15
    of block p."""
    a = np.asarray(raw, dtype=np.uint8).reshape(9, 2, mt, 2, 32, 16)   # tap, p, tile, h, row, k
    return a.transpose(0, 2, 4, 1, 3, 5).reshape(9, mt * 32, 64)


def expected_blocks(arena, ch, kind, **mut):
    """What resr_pack_weights leaves for a chunk: a list of [9, 32 mt, 32] arrays (one; exact16: W0, W1, W2)."""
    v = chunk_weights(arena, ch, flip=mut.get("flip", True))
    if kind == "f32":
        return [v]
    if kind == "f16":
        return [f16_rne(v)]
    w0, w1, w2 = exact16_blocks(v)
    if mut.get("unscaled_w1"):
        w1 = f16_rne(v - w0.astype(F32))
    return [w0, w1, w2]


def expected_f16_fused(arena, ch):
    """The other legal evaluation of a plain f16 block: the EXACT product w * scale rounded once to f16.  The library is built with
    HIP's default -ffp-contract=fast, under which the compiler may fuse the fp32 product into the conversion (one rounding instead of
    two; an exact zero then leaves as +0 whatever its sign).  Both are "the f16 rounding of w * scale"; the formats' own consumers see
    no difference between the zeros.  f32 and exact16 blocks have no such freedom: their product is stored or reused in fp32."""
    with np.errstate(over="ignore"):
        return chunk_weights(arena, ch, exact_product=True).astype(F16)


def f16_block_differs(got, arena, ch):
    """Indices of a plain f16 block that equal neither evaluation (zeros compared by value), and how many elements tell the two apart."""
    a, b = expected_blocks(arena, ch, "f16")[0].reshape(-1), expected_f16_fused(arena, ch).reshape(-1)
    g = np.asarray(got, dtype=F16).reshape(-1)
    same = lambda w: (g.view(np.uint16) == w.view(np.uint16)) | ((g == 0) & (w == 0))
    return np.flatnonzero(~(same(a) | same(b))), int((a.view(np.uint16) != b.view(np.uint16)).sum())


def expected_mx(arena, ch):
    _, w1, w2 = exact16_blocks(chunk_weights(arena, ch))
    return np.concatenate([bf8_bits(w1), bf8_bits(w2)], axis=2)


# ---- case tables -------------------------------------------------------------------------------------------------------------------
DTYPES = ("f32", "f16", "f16x2")
AMAX_STATES = {"lifted": float_to_bits(1.5 * 2.0 ** -20), "unlifted": float_to_bits(3.0), "zero": 0}
# f16 ties (1 + 2^-11 -> 1, 1 + 3 2^-11 -> 1 + 2^-9), f16 subnormals and a subnormal tie, |v| < 2^-25 (hi = 0, lo carries the value), -0.0,
# the top of f16's range (65504 stays, 65519.996 falls back to it, 65520 is the tie that becomes inf), beyond it, inf, NaN
SPECIALS = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1.2345 * 2.0 ** -20, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 2.0 ** -26,
                     -1.3 * 2.0 ** -27, 2.0 ** -40, -0.0, 0.0, 65504.0, 65519.996, 65520.0, -70000.0, 1e6, np.inf, -np.inf, np.nan,
                     0.1, -2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12)], dtype=F32)


def planted(rng, shape, scale=1.0):
    """Standard normals times `scale` with SPECIALS planted at the start and (where the tensor is large enough) at the very end."""
    x = (rng.standard_normal(shape) * scale).astype(F32)
    f = x.reshape(-1)
    k = min(SPECIALS.size, f.size)
    f[:k] = SPECIALS[:k]
    if f.size >= 3 * SPECIALS.size:
        f[-SPECIALS.size:] = SPECIALS[::-1]
    return x


NCHW_CFG = [(3, 1, 8), (3, 1, 32), (3, 2, 32), (8, 2, 32), (3, 4, 64), (64, 1, 64)]          # (c, r, c_pad)


def nchw_cases():
    """name -> dict(kind, n, c, h, w, r, c_pad, mask, amax, lo, q).  lo: "default" (-1: directly behind) / "explicit"; q: write the q
    tensor.  Per (c, r, c_pad): 1 x 1 output, the 8 x 12 image with and without the mask, and at c_pad 32 a row of 70 output pixels
    (wo * pieces = 280 / 560 > 256 and no multiple of it) in a batch of 3."""
    cases = {}

    def add(kind, c, r, cp, n, h, w, mask=False, amax=None, lo=None, q=False):
        if kind == "f16x2" and lo is None:
            lo = "default"
        name = f"{kind}-c{c}r{r}p{cp}-{n}x{h}x{w}" + ("-mask" if mask else "") + (f"-{amax}" if amax else "") + \
               ("-lo" if lo == "explicit" else "") + ("-q" if q else "")
        cases[name] = dict(kind=kind, n=n, c=c, h=h, w=w, r=r, c_pad=cp, mask=mask, amax=amax, lo=lo, q=q)

    for kind in DTYPES:
        for c, r, cp in NCHW_CFG:
            add(kind, c, r, cp, 1, r, r)
            add(kind, c, r, cp, 2, 8, 12)
            add(kind, c, r, cp, 2, 8, 12, mask=True)
            if cp == 32:
                add(kind, c, r, cp, 3, 2 * r, 70 * r, mask=(r == 2))
        for amax in AMAX_STATES:
            add(kind, 3, 1, 32, 2, 8, 12, amax=amax)
            add(kind, 3, 2, 32, 2, 8, 12, mask=True, amax=amax)
    for amax in AMAX_STATES:
        add("f16", 3, 1, 8, 2, 8, 12, amax=amax, mask=True)
    for c, r, cp in NCHW_CFG[1:]:
        add("f16x2", c, r, cp, 2, 8, 12, lo="explicit")
        add("f16x2", c, r, cp, 2, 8, 12, q=True)
        add("f16x2", c, r, cp, 2, 8, 12, mask=True, lo="explicit", q=True)
    add("f16x2", 3, 2, 32, 3, 4, 140, mask=True, amax="lifted", lo="explicit", q=True)
    add("f16x2", 3, 1, 32, 1, 1, 1, q=True)
    return cases


def nchw_inputs(name, case):
    rng = np.random.default_rng(sum(map(ord, name)))
    shape = (case["n"], case["c"], case["h"], case["w"])
    # a lifted pass sees a tiny gradient: values around 2^-20, so that times 2^20 they fill f16's range
    src = planted(rng, shape, 2.0 ** -20 if case["amax"] == "lifted" else 1.0)
    mask = (rng.integers(0, 3, size=shape) > 0).astype(np.uint8) * rng.integers(1, 256, size=shape).astype(np.uint8) if case["mask"] else None
    return src, mask


def nhwc_cases():
    """name -> dict(kind, n, c, h, w, r, stride, amax, lo).  w = 1, 31 (wsh 5), 33 (6), 100 (7), 257 (8, two column blocks); h is no
    multiple of the 256 >> wsh rows of a workgroup."""
    cases = {}
    for kind in DTYPES:
        for (n, c, h, w, r, extra) in ((1, 3, 1, 1, 1, 0), (2, 3, 9, 31, 1, 5), (2, 3, 10, 33, 1, 29), (1, 2, 3, 100, 1, 6), (1, 3, 3, 257, 1, 0),
                                       (2, 3, 10, 34, 2, 20), (3, 3, 12, 32, 4, 16), (1, 3, 2, 514, 2, 4), (1, 1, 4, 4, 4, 0)):
            for amax in (None, "lifted") if (w in (31, 34)) else (None,):
                lo = None if kind != "f16x2" else ("explicit" if extra else "default")
                cases[f"{kind}-{n}x{c}x{h}x{w}-r{r}+{extra}" + (f"-{amax}" if amax else "")] = dict(
                    kind=kind, n=n, c=c, h=h, w=w, r=r, stride=c * r * r + extra, amax=amax, lo=lo)
        cases[f"{kind}-unlifted"] = dict(kind=kind, n=1, c=3, h=4, w=6, r=2, stride=16, amax="unlifted", lo=None if kind != "f16x2" else "default")
        cases[f"{kind}-zero"] = dict(kind=kind, n=1, c=3, h=4, w=6, r=2, stride=16, amax="zero", lo=None if kind != "f16x2" else "default")
    return cases


ABSMAX_COUNTS = (1, 3, 4, 5, 1023, 2048 * 1024 + 5)


def absmax_cases():
    """name -> dict(count, offset, where, fill, t, slot1, slot2).  where: index of the planted maximum (negative: from the end);
    fill: "normal" / "zeros" / "subnormal" / "inf" / "nan"."""
    cases = {}

    def add(count, where=0, fill="normal", t=0, slot1=0, slot2=0, offset=0, peak=-37.5):
        cases[f"n{count}-at{where}-{fill}-t{t}-b{slot1}f{slot2}-o{offset}-p{peak}"] = dict(count=count, offset=offset, where=where, fill=fill, t=t,
                                                                                           slot1=slot1, slot2=slot2, peak=peak)
    for count in ABSMAX_COUNTS:
        for where in (0, -1, -2 if count > 4 else 0):       # the first, the last, a tail element (count % 4 != 0: the last ones are tail)
            add(count, where)
        add(count, count // 2, offset=1)
    for fill in ("zeros", "subnormal", "inf", "nan"):
        for slot1, slot2 in ((0, 0), (8, 1)):
            add(1023, 511, fill, slot1=slot1, slot2=slot2)
        add(5, -1, fill)
    for t in (-64, 0, 6, 64):
        add(1023, 7, t=t, peak=2.0 ** -10 * 1.25)
        add(5, 4, t=t, peak=-3.0e4, slot1=4)
    for slot1, slot2 in ((0, 1), (4, 0), (4, 1), (36, 1), (38, 1), (40, 0), (40, 1), (100, 0), (100, 1)):
        add(1023, 100, t=6, slot1=slot1, slot2=slot2, peak=2.0 ** -30 * 1.75)
    add(5, 2, t=-64, slot1=40, peak=2.0 ** 50 * 1.5)        # exponent + 64 + 40 beyond 254: held at 254
    add(5, 2, t=0, slot1=40, peak=2.0 ** 100 * 1.5)
    add(4, 3, t=64, peak=2.0 ** -70, slot1=8)               # m becomes subnormal: left alone by the back-off
    return cases


def absmax_input(case):
    rng = np.random.default_rng(case["count"] % 9973 + len(case["fill"]))
    n = case["count"]
    x = rng.uniform(-1.0, 1.0, size=n).astype(F32)
    if case["fill"] == "zeros":
        x[:] = 0.0
        x[::2] = -0.0
        return x
    if case["fill"] == "subnormal":
        x = (x * F32(2.0 ** -127)).astype(F32)
        x[case["where"]] = -F32(2.0 ** -126) * F32(0.75)
        return x
    x[case["where"]] = F32(case["peak"])
    if case["fill"] == "inf":
        x[(case["where"] + n // 2) % n] = -np.inf
    if case["fill"] == "nan":
        x[(case["where"] + n // 2) % n] = np.nan
        x[0] = np.inf
    return x


def sumpool_cases():
    """name -> dict(kind, n, ho, wo, c, mask, plane).  wo * groups crosses 256 at (wo, c) = (65, 32) [f16: 260], (33, 64) [264], (129, 8)
    [f32 c 4: wo 257]; plane: the generator's form, one 32-channel plane of a chunk-planar pair tensor with explicit lo offsets."""
    cases = {}
    for kind in DTYPES:
        cs = (4,) if kind == "f32" else (8, 32, 64)
        for c in cs:
            wide = {4: 257, 8: 257, 32: 65, 64: 33}[c]
            for (n, ho, wo) in ((1, 1, 1), (2, 3, 5), (2, 2, wide)):
                for mask in (False, True):
                    cases[f"{kind}-{n}x{ho}x{wo}x{c}" + ("-mask" if mask else "")] = dict(kind=kind, n=n, ho=ho, wo=wo, c=c, mask=mask, plane=False)
    for mask in (False, True):
        cases["f16x2-plane" + ("-mask" if mask else "")] = dict(kind="f16x2", n=2, ho=3, wo=5, c=32, mask=mask, plane=True)
    return cases


def planted_pair_mask(rng, shape):
    """A pair mask with the sign rule's corner cases at the start and the end: (hi, lo) -> positive."""
    hi, lo = pair_split(rng.standard_normal(shape).astype(F32))
    hf, lf = hi.reshape(-1), lo.reshape(-1)
    tiny = F16(6e-8)
    corner = [(0.0, 0.5), (0.0, -0.5), (-0.0, 0.5), (-0.0, -0.5), (0.0, 0.0), (-0.0, -0.0), (tiny, -0.5), (-tiny, 0.5)]
    want = [True, False, True, False, False, False, True, False]
    idx = list(range(8)) + (list(range(hf.size - 8, hf.size)) if hf.size >= 32 else [])
    for k, i in enumerate(idx):
        hf[i], lf[i] = corner[k % 8]
    return hi, lo, idx, (want + want)[:len(idx)]


def nhwc_loaded(name, c):
    """(the fp32 values the kernel loads, hi, lo) of an nhwc case: shared by the CPU and the GPU module."""
    rng = np.random.default_rng(sum(map(ord, name)))
    shape = (c["n"], c["h"] // c["r"], c["w"] // c["r"], c["stride"])
    base = planted(rng, shape)
    base[~np.isfinite(base)] = 3.0
    if c["kind"] == "f32":
        return base, base, None
    if c["kind"] == "f16":
        hi = f16_rne(np.clip(base, -60000, 60000))
        return hi.astype(F32), hi, None
    hi, lo = pair_split(np.clip(base, -60000, 60000))
    return pair_load32(hi, lo), hi, lo


def sumpool_operands(name, c):
    """(x hi, x lo or None, mask hi, mask lo, positive) of a sumpool case."""
    rng = np.random.default_rng(sum(map(ord, name)))
    shape, oshape = (c["n"], 2 * c["ho"], 2 * c["wo"], c["c"]), (c["n"], c["ho"], c["wo"], c["c"])
    base = rng.standard_normal(shape).astype(F32)
    base = np.sign(base) * (F32(0.25) + np.abs(base))                  # no window sums to nearly nothing by a missing sign
    if c["mask"]:
        base = np.abs(base)                                            # every window sums to >= 1: the other LeakyReLU branch is >= 0.8 away
    if c["kind"] == "f16x2":
        xh, xl = pair_split(base)
        mh, ml, _, _ = planted_pair_mask(rng, oshape)
        return xh, xl, mh, ml, D.pair_positive(mh, ml)
    dt = F32 if c["kind"] == "f32" else F16
    m = rng.standard_normal(oshape).astype(dt)
    m.reshape(-1)[:4] = [0.0, -0.0, 1.0, -1.0][:min(4, m.size)] if m.size >= 4 else 0.0
    return base.astype(dt), None, m, None, m > 0


def judge_sumpool(c, got, xh, xl, pos):
    exact = xh.astype(F64) if xl is None else pair_value(xh, xl)
    v32 = xh.astype(F32) if xl is None else pair_load32(xh, xl)
    p = pos if c["mask"] else None
    return judge(got, sumpool2x2(exact, p), sumpool2x2(v32, p, dtype=F32), {"f32": "f32", "f16": "f16", "f16x2": "pair"}[c["kind"]])


ADD_COUNTS_E = (1, 257)                     # times E: one thread; two workgroups, the second with one thread
EMA_COUNTS = (1, 3, 4, 5, 100003, 2048 * 1024 + 7)
EMA_DECAYS = (0.999, 0.0, 1.0)
LOSS_COUNTS = (1, 2, 3, 4, 5, 6, 7, 1025, 4 * 1024 * 1024 + 131075)
BCE_SPECIALS = np.array([0.0, -0.0, 60.0, -60.0, 100.0, -100.0, 1e-3, -20.0], dtype=F32)


def loss_inputs(count):
    """(a, b, x): L1 operands with exact ties planted (a == b, +0 against -0), BCE logits with BCE_SPECIALS planted."""
    rng = np.random.default_rng(count)
    a, b = rng.standard_normal(count).astype(F32), rng.standard_normal(count).astype(F32)
    b[::5] = a[::5]
    if count > 2:
        a[2], b[2] = 0.0, -0.0
    x = (rng.standard_normal(count) * 4).astype(F32)
    k = min(count, BCE_SPECIALS.size)
    x[count - k:] = BCE_SPECIALS[:k]            # the specials sit in the tail (count % 4 elements) too
    return a, b, x


def pack_table():
    """(arena fp32, [Chunk], packed elements of the plain layout, scale_ptr value).  Five convolutions in one table:
       A forward [40, 20] (M 40 -> one group of mt 2, m_count 40 < 64; K 20 < 32)
       B forward [24, 40] (mt 1, m_count 24; two K chunks, the second with 8 real channels)
       C transposed [24, 40] with scale 0.2 (M = cin 40 -> mt 2; K = cout 24), taps flipped
       D virtual4x4 [16, C = 6, 4, 4] (24 virtual channels), forward, with a scale_ptr
       E forward [70, 33] with scale 0.5 AND the scale_ptr: two groups (mt 2 with 64 rows, mt 1 with 6), two K chunks (32 + 1)
    Between C and D the table leaves 512 elements of the packed buffer untouched."""
    rng = np.random.default_rng(20)
    sizes = [40 * 20 * 9, 24 * 40 * 9, 16 * 6 * 16, 70 * 33 * 9]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    arena = (rng.standard_normal(offs[-1]) * 0.3).astype(F32)
    arena[:8] = [0.0, -0.0, 2.0 ** -13, 1 + 2.0 ** -11, -(1 + 3 * 2.0 ** -11), 3e-6, -7e-9, 15.9]
    sv = float(F32(1.0 / 1.7))
    chunks, dst = [], 0
    chunks.append(Chunk(0, dst, 40, 20, 0, 40, 0, 20, 2)); dst += block_elems(2)
    for k0, kc in ((0, 32), (32, 8)):
        chunks.append(Chunk(int(offs[1]), dst, 24, 40, 0, 24, k0, kc, 1)); dst += block_elems(1)
    chunks.append(Chunk(int(offs[1]), dst, 24, 40, 0, 40, 0, 24, 2, transposed=1, scale=0.2)); dst += block_elems(2)
    dst += 512
    chunks.append(Chunk(int(offs[2]), dst, 16, 6, 0, 16, 0, 24, 1, virtual4x4=1, scale_value=sv)); dst += block_elems(1)
    for g0, mc, mt in ((0, 64, 2), (64, 6, 1)):
        for k0, kc in ((0, 32), (32, 1)):
            chunks.append(Chunk(int(offs[3]), dst, 70, 33, g0, mc, k0, kc, mt, scale=0.5, scale_value=sv)); dst += block_elems(mt)
    return arena, chunks, dst, sv
