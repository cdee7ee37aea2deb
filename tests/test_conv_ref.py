"""CPU: tests/conv_ref.py is right (against torch's own operators and float64 autograd), and the rule it carries has the power the
GPU tests rely on: the plain fp32 evaluation of every case passes with a ratio <= 0.25, every wrong kernel listed below is
rejected.  A "wrong kernel" is the float64 reference with ONE defect, stored as a correct kernel would store it.  The same for
exact16: pair_split leaves lo a remainder of hi; the pair rule rejects a lost lo tensor (in0, in1, res0, res1, one chunk of six), a
lost W1 block, a tap dropped at a seam and a mask decided by a zero hi half; the weight-gradient rule A + wgrad_lolo rejects X's or
G's lo tensor lost and one tap-product skipped in one pixel split -- while the exact16 arithmetic itself (x_lo (w - W2) and
X_lo^T G_lo dropped as documented) passes with room."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as R

F64, F32 = torch.float64, torch.float32


def _q(t, dtype_name):
    return t.half().float() if dtype_name == "f16" else t.float()


def _case(dtype_name, cin=192, cout=64, n=1, h=20, w=40, seed=5):
    """The shape of the dense block's closing convolution (rdb_conv5_res of tests/test_gpu_kernels.py) on an image that holds a tile
    seam in x (column 32) and two in y (rows 8 and 16)."""
    g = torch.Generator().manual_seed(seed)
    x = _q(torch.randn(n, cin, h, w, generator=g), dtype_name)
    wt = _q(torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5, dtype_name)
    bias = torch.randn(cout, generator=g) * 0.1
    r0 = _q(torch.randn(n, cout, h, w, generator=g), dtype_name)
    r1 = _q(torch.randn(n, cout, h, w, generator=g), dtype_name)
    mk = _q(torch.randn(n, cout, h, w, generator=g), dtype_name)
    return x, wt, bias, r0, r1, mk


def _store(v, dtype_name):
    """What a correct kernel stores of an fp32 result."""
    return v.float().half().double() if dtype_name == "f16" else v.float().double()


def _truncate_f16(v):
    """Round an fp32 tensor toward zero to f16 (normal range): clear the 13 low significand bits."""
    bits = v.float().contiguous().view(torch.int32) & ~0x1FFF
    return bits.view(torch.float32).half().double()


# ---- the reference is right -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up", [False, True])
def test_forward_reference_against_torch(up):
    x, wt, bias, r0, r1, mk = _case("f32", cin=40, cout=12, n=2, h=6, w=10)
    if up:
        x = x[:, :, :3, :5]
    xin = F.interpolate(x.double(), scale_factor=2, mode="nearest") if up else x.double()
    conv = F.conv2d(xin, wt.double(), bias.double(), padding=1)
    got, _ = R.conv3x3(x, wt, F64, up=up, bias=bias)
    assert (got - conv).abs().max().item() < 1e-13
    got, _ = R.conv3x3(x, wt, F64, up=up, bias=bias, lrelu=True, slope=0.1)
    assert (got - F.leaky_relu(conv, float(np.float32(0.1)))).abs().max().item() < 1e-13
    slopes = torch.rand(12) * 2 - 0.5
    got, _ = R.conv3x3(x, wt, F64, up=up, bias=bias, prelu=slopes)
    assert (got - F.prelu(conv, slopes.double())).abs().max().item() < 1e-13
    s0, t0, s1, t1, sl = (float(np.float32(v)) for v in (0.2, 1.0, 0.3, 0.5, 0.2))
    got, pre = R.conv3x3(x, wt, F64, up=up, mask=mk, slope=0.2, res0=r0, s0=0.2, t0=1.0, res1=r1, s1=0.3, t1=0.5, clamp=True)
    want = (F.conv2d(xin, wt.double(), None, padding=1) * torch.where(mk > 0, 1.0, sl) * s0 + t0 * r0.double()) * s1 + t1 * r1.double()
    assert (pre - want).abs().max().item() < 1e-13 and (got - want.clamp(0, 1)).abs().max().item() < 1e-13
    assert ((want < 0).any() and (want > 1).any()), "the clamp case clamps nothing"


@pytest.mark.parametrize("up", [False, True])
def test_wgrad_reference_against_autograd(up):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 7, 3 if up else 6, 5 if up else 10, generator=g)
    gy = torch.randn(2, 5, 6, 10, generator=g)
    wt = torch.zeros(5, 7, 3, 3, dtype=F64, requires_grad=True)
    bs = torch.zeros(5, dtype=F64, requires_grad=True)
    xin = F.interpolate(x.double(), scale_factor=2, mode="nearest") if up else x.double()
    (F.conv2d(xin, wt, bs, padding=1) * gy.double()).sum().backward()
    dw, db = R.wgrad(x, gy, 0.5, F64, up=up)
    assert (dw - 0.5 * wt.grad).abs().max().item() < 1e-13 and (db - 0.5 * bs.grad).abs().max().item() < 1e-13


def test_pairs_and_scalars():
    v = torch.randn(1000, generator=torch.Generator().manual_seed(1))
    hi, lo = R.pair_split(v)
    assert (R.pair_value(hi, lo) - v.double()).abs().max().item() <= 2.0 ** -22 * v.abs().max().item()
    assert R.f32scalar(0.2, F64).item() == float(np.float32(0.2)) != 0.2


# ---- the rule has power -----------------------------------------------------------------------------------------------------------
def _passes(ref64, ref32, dtype_name):
    """The unmutated fp32 evaluation, stored as the kernel stores it: ratio <= 0.25 against A alone by construction, inside the bound."""
    A, e32 = R.allowance(ref64, ref32)
    assert e32 <= 0.25 * A
    rec = R.judge(_store(ref32, dtype_name), ref64, ref32, dtype_name)
    assert rec["bad"] == 0, rec
    if dtype_name == "f32":
        assert rec["ratio"] <= 0.25, rec


def _rejected(mutant64, ref64, ref32, dtype_name, what, store=None):
    rec = R.judge(store(mutant64) if store else _store(mutant64, dtype_name), ref64, ref32, dtype_name)
    assert rec["bad"] > 0, (what, rec)
    return rec


@pytest.mark.parametrize("dtype_name", ["f32", "f16"])
def test_rule_rejects_wrong_epilogue_constants(dtype_name):
    x, wt, bias, r0, r1, mk = _case(dtype_name)
    kw = dict(bias=bias, res0=r0, s0=0.2, t0=1.0, res1=r1, s1=0.2, t1=0.5)
    acc64, acc32 = R.correlate(x, wt, F64), R.correlate(x, wt, F32)
    ref64, ref32 = R.epilogue(acc64, F64, **kw)[0], R.epilogue(acc32, F32, **kw)[0]
    _passes(ref64, ref32, dtype_name)
    for name in ("s0", "t0", "s1", "t1"):
        _rejected(R.epilogue(acc64, F64, **dict(kw, **{name: kw[name] * 1.01}))[0], ref64, ref32, dtype_name, name)
    # the existing per-tensor gates let all of these through (2e-2 / 2e-4 of the tensor's maximum)
    m = R.epilogue(acc64, F64, **dict(kw, s0=0.21))[0]
    if dtype_name == "f16":
        assert (m - ref64).abs().max().item() < 2e-2 * ref64.abs().max().item()
    # LeakyReLU / mask slope
    for kw2 in (dict(bias=bias, lrelu=True, slope=0.2), dict(mask=mk, slope=0.2), dict(bias=bias, lrelu=True, slope=0.1)):
        r64, r32 = R.epilogue(acc64, F64, **kw2)[0], R.epilogue(acc32, F32, **kw2)[0]
        _passes(r64, r32, dtype_name)
        _rejected(R.epilogue(acc64, F64, **dict(kw2, slope=kw2["slope"] * 1.01))[0], r64, r32, dtype_name, "slope")
    if dtype_name == "f32":   # a bias rounded to f16 in an fp32 result
        r64, r32 = R.epilogue(acc64, F64, bias=bias)[0], R.epilogue(acc32, F32, bias=bias)[0]
        _rejected(R.epilogue(acc64, F64, bias=bias.half().float())[0], r64, r32, "f32", "f16 bias")
    else:                     # a store that truncates instead of rounding to nearest
        rec = _rejected(ref32, ref64, ref32, "f16", "truncating store", store=_truncate_f16)
        assert rec["frac_bad"] > 0.1, rec


@pytest.mark.parametrize("dtype_name", ["f32", "f16"])
@pytest.mark.parametrize("where", ["col31", "col32", "row7", "row8", "row15", "row16"])
def test_rule_rejects_a_tap_dropped_at_a_tile_seam(dtype_name, where):
    """One tap of ONE input channel is missing for the outputs of one column / row next to a tile seam (tiles are 32 wide and
    8, 16 or 32 high): what a halo row or column staged one short looks like."""
    x, wt, bias, r0, r1, mk = _case(dtype_name)
    kw = dict(bias=bias, res0=r0, s0=0.2, t0=1.0, res1=r1, s1=0.2, t1=0.5)
    acc64, acc32 = R.correlate(x, wt, F64), R.correlate(x, wt, F32)
    ref64, ref32 = R.epilogue(acc64, F64, **kw)[0], R.epilogue(acc32, F32, **kw)[0]
    c = 17
    k = int(where[3:])
    m = acc64.clone()
    if where.startswith("col"):      # outputs of column k lose the tap that reads across the seam 31 | 32
        dx = 2 if k == 31 else 0
        m[:, :, :, k] -= wt[:, c, 1, dx].double().view(1, -1, 1) * x[:, c, :, k + dx - 1].double().unsqueeze(1)
    else:                             # outputs of row k lose the tap that reads across the seam k | k + 1 resp. k - 1 | k
        dy = 2 if k % 8 == 7 else 0
        m[:, :, k, :] -= wt[:, c, dy, 1].double().view(1, -1, 1) * x[:, c, k + dy - 1, :].double().unsqueeze(1)
    _rejected(R.epilogue(m, F64, **kw)[0], ref64, ref32, dtype_name, where)


@pytest.mark.parametrize("dtype_name", ["f32", "f16"])
def test_rule_rejects_a_padded_input_channel_read_as_nonzero(dtype_name):
    """cin = 3 in a 32-channel chunk: channel 3 of the buffer read as 2^-10 against a weight tap that should have been zero."""
    x, wt, bias, _, _, _ = _case(dtype_name, cin=3, cout=64, h=9, w=33)
    ref64, ref32 = R.conv3x3(x, wt, F64, bias=bias, lrelu=True, slope=0.1)[0], R.conv3x3(x, wt, F32, bias=bias, lrelu=True, slope=0.1)[0]
    _passes(ref64, ref32, dtype_name)
    x4 = torch.cat([x, torch.full_like(x[:, :1], 2.0 ** -10)], 1)
    w4 = torch.cat([wt, wt[:, :1]], 1)
    _rejected(R.conv3x3(x4, w4, F64, bias=bias, lrelu=True, slope=0.1)[0], ref64, ref32, dtype_name, "padded channel")
    # the sign of a zero is nothing to the rule: slope 0 stores -0.0 where torch's relu stores 0.0
    z64, z32 = R.conv3x3(x, wt, F64, bias=bias, lrelu=True, slope=0.0)[0], R.conv3x3(x, wt, F32, bias=bias, lrelu=True, slope=0.0)[0]
    assert (z64 == 0).any() and torch.signbit(z64[z64 == 0]).any()
    flipped = torch.where(z32 == 0, -z32, z32)
    assert R.judge(_store(flipped, dtype_name), z64, z32, dtype_name)["bad"] == 0
    assert R.judge(_store(z32, dtype_name), z64.clamp_min(0.0) + 0.0, z32, dtype_name)["bad"] == 0


def test_pass_mask_rule():
    x, wt, bias, _, _, _ = _case("f32", cin=64, cout=3, n=2)
    ref64, pre64 = R.conv3x3(x, wt, F64, bias=bias + 0.5, clamp=True)
    ref32, pre32 = R.conv3x3(x, wt, F32, bias=bias + 0.5, clamp=True)
    A, _ = R.allowance(ref64, ref32)
    assert R.pass_mask_ok((pre32 >= 0) & (pre32 <= 1), pre64, A) == 0
    wrong = (pre64 >= 0) & (pre64 <= 0.99)          # a kernel that compares against the wrong constant
    assert R.pass_mask_ok(wrong, pre64, A) > 0


@pytest.mark.parametrize("dtype_name", ["f32", "f16"])
@pytest.mark.parametrize("up", [False, True])
def test_rule_rejects_wrong_weight_gradients(dtype_name, up):
    g = torch.Generator().manual_seed(7)
    n, cin, cout, h, w = 2, 64, 32, 19, 45
    if up:
        h, w = 18, 44
    x = _q(torch.randn(n, cin, h // 2 if up else h, w // 2 if up else w, generator=g), dtype_name)
    gy = _q(torch.randn(n, cout, h, w, generator=g), dtype_name)
    dw64, db64 = R.wgrad(x, gy, 0.5, F64, up=up)
    dw32, db32 = R.wgrad(x, gy, 0.5, F32, up=up)
    _passes(dw64, dw32, "f32")
    _passes(db64, db32, "f32")
    # scale applied twice
    _rejected(dw64 * 0.5, dw64, dw32, "f32", "scale twice (dW)")
    _rejected(db64 * 0.5, db64, db32, "f32", "scale twice (db)")
    # the product of ONE border pixel (image 1, last row, last column) is missing from the centre tap / from db
    xin = R.upsample2(x) if up else x
    m = dw64.clone()
    m[:, :, 1, 1] -= 0.5 * gy[1, :, h - 1, w - 1].double().view(-1, 1) * xin[1, :, h - 1, w - 1].double().view(1, -1)
    _rejected(m, dw64, dw32, "f32", "border pixel (dW)")
    _rejected(db64 - 0.5 * gy[1, :, h - 1, w - 1].double(), db64, db32, "f32", "border pixel (db)")


# ---- the added epilogue values -------------------------------------------------------------------------------------------------------
def test_epilogue_aux_values_against_torch():
    """with_aux: the value after the bias and before the mask (RESR_CONV_AUX_BEFORE_MASK), the value after LeakyReLU and before the
    residuals (RESR_CONV_AUX_BEFORE_RES), on the discriminator's two uses and on a pass that has every step."""
    x, wt, bias, r0, r1, mk = _case("f32", cin=40, cout=12, n=2, h=6, w=10)
    sl, s0, s1, t1 = (float(np.float32(v)) for v in (0.2, 0.2, 0.3, 0.5))
    conv = F.conv2d(x.double(), wt.double(), bias.double(), padding=1)
    conv0 = F.conv2d(x.double(), wt.double(), None, padding=1)
    assert len(R.conv3x3(x, wt, F64, bias=bias)) == 2                       # the callers that do not ask keep their two values
    v, pre, bm, br = R.conv3x3(x, wt, F64, bias=bias, lrelu=True, slope=0.2, res0=r0, s0=0.2, t0=1.0, with_aux=True)
    act = F.leaky_relu(conv, sl)
    assert (bm - conv).abs().max().item() < 1e-13 and (br - act).abs().max().item() < 1e-13
    assert (v - (act * s0 + r0.double())).abs().max().item() < 1e-13 and torch.equal(v, pre)
    assert (br - v).abs().max().item() > 0.1                                   # it is not the output
    v, pre, bm, br = R.conv3x3(x, wt, F64, mask=mk, slope=0.2, with_aux=True)
    masked = conv0 * torch.where(mk > 0, 1.0, sl)
    assert (bm - conv0).abs().max().item() < 1e-13 and (v - masked).abs().max().item() < 1e-13 and torch.equal(br, v)
    assert (bm - v).abs().max().item() > 0.1
    v, pre, bm, br = R.conv3x3(x, wt, F64, bias=bias, mask=mk, lrelu=True, slope=0.2, res0=r0, s0=0.2, t0=1.0, res1=r1, s1=0.3, t1=0.5,
                               clamp=True, with_aux=True)
    want_br = F.leaky_relu(conv * torch.where(mk > 0, 1.0, sl), sl)
    want = (want_br * s0 + r0.double()) * s1 + t1 * r1.double()
    assert (bm - conv).abs().max().item() < 1e-13 and (br - want_br).abs().max().item() < 1e-13
    assert (pre - want).abs().max().item() < 1e-13 and (v - want.clamp(0, 1)).abs().max().item() < 1e-13
    slopes = torch.rand(12, generator=torch.Generator().manual_seed(1)) * 2 - 0.5
    v, pre, bm, br = R.conv3x3(x, wt, F64, bias=bias, prelu=slopes, res0=r0, s0=0.2, t0=1.0, with_aux=True)
    assert (br - F.prelu(conv, slopes.double())).abs().max().item() < 1e-13


# ---- exact16: the structure of a pair, the pair rule and the weight-gradient rule -----------------------------------------------------
def test_pair_split_leaves_lo_a_remainder_of_hi():
    """R.pair_lo_excess (what the GPU tests ask of every stored pair) holds for pair_split of fp32 data of every size -- normal,
    f16-subnormal, below the subnormals (hi = 0), zero, binade ends -- and notices a lo that is no remainder."""
    g = torch.Generator().manual_seed(4)
    v = torch.randn(20000, generator=g)
    edge = torch.tensor([0.0, -0.0, 1.0, 1.0 + 2.0 ** -11, 1.0 - 2.0 ** -12, 2.0 ** -14, 2.0 ** -14 * (1 + 2.0 ** -11), 2.0 ** -24, 2.0 ** -25,
                         2.0 ** -25 * 0.999, 1e-9, -1e-9, 60000.0, 2047.5, 0.1, 1.0 / 3.0])
    v = torch.cat([v, v * 100.0, v * 1e-3, v * 1e-5, v * 1e-7, v * 1e-9, torch.zeros(64), edge, -edge])
    hi, lo = R.pair_split(v)
    assert (hi == 0).sum() > 20000 and ((hi != 0) & (hi.abs() < 2.0 ** -14)).sum() > 1000      # both small ranges are in the data
    assert R.pair_lo_excess(hi, lo) == 0
    assert (R.pair_value(hi, lo) - v.double()).abs().max().item() <= 2.0 ** -22 * v.abs().max().item()
    # a hi half that was truncated instead of rounded leaves remainders of up to a whole ulp; a lo scaled wrongly is no remainder
    hi_t = _truncate_f16(v).half()
    lo_t = ((v.double() - hi_t.double()) * 4096.0).half()
    assert R.pair_lo_excess(hi_t, lo_t) > 1000
    assert R.pair_lo_excess(hi, (lo.float() * 4.0).half()) > 1000
    assert R.pair_lo_excess(torch.zeros(4).half(), torch.full((4,), 0.5).half()) == 4          # hi = 0: |value| must stay below 2^-25


class _Pair:
    """An exact16 operand: hi (float64), lo (float64, in the operand's own scale: the stored lo / 4096), value = hi + lo."""

    def __init__(self, t):
        hi, lo = R.pair_split(t)
        self.hi, self.lo = hi.double(), lo.double() / 4096.0
        self.value = self.hi + self.lo


def _x2_acc(xh, xl, wt, w1=True):
    """The exact16 accumulator in float64: x_hi (W0 + W1) + x_lo W2 -- everything the kernel computes; the documented drop is
    x_lo (w - W2)."""
    w0, w1_, w2 = R.split_weights(wt)
    return R.correlate(xh, w0 + w1_ if w1 else w0, F64) + R.correlate(xl, w2, F64)


def _store_pair(v):
    """What a correct kernel stores of an fp32 result as a pair, joined."""
    hi, lo = R.pair_split(v.float())
    assert R.pair_lo_excess(hi, lo) == 0
    return R.pair_value(hi, lo)


def _pair_judged(got, ref64, what, reject, below=0.25):
    """Judge `got`, stored as a pair, by the pair rule: a mutant must be rejected, an honest result pass with its ratio under `below`."""
    rec = R.judge(_store_pair(got), ref64, None, "pair")
    print(f"{what}: ratio {rec['ratio']:.3g} beyond {rec['frac_bad']:.2%}")
    if reject:
        assert rec["bad"] > 0, (what, rec)
    else:
        assert rec["bad"] == 0 and rec["ratio"] < below, (what, rec)
    return rec


def _x2_case(cin, cout, n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = _Pair(torch.randn(n, cin, h, w, generator=g))
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    r0, r1 = _Pair(torch.randn(n, cout, h, w, generator=g)), _Pair(torch.randn(n, cout, h, w, generator=g))
    return g, x, wt, bias, r0, r1


def test_pair_rule_rejects_a_lost_input_lo_or_weight_block():
    """rdb_conv3_2seg of tests/test_gpu_kernels.py (cin 128 in two segments of 64, cout 32, LeakyReLU, 1 x 33 x 32): the lo tensor
    of either segment lost, the W1 block lost.  The exact arithmetic -- x_lo (w - W2) dropped as documented -- and the plain fp32
    result stored as a pair pass with room."""
    _, x, wt, bias, _, _ = _x2_case(128, 32, 1, 33, 32, 21)
    kw = dict(bias=bias, lrelu=True, slope=0.2)
    ref64 = R.conv3x3(x.value, wt, F64, **kw)[0]
    _pair_judged(R.epilogue(_x2_acc(x.hi, x.lo, wt), F64, **kw)[0], ref64, "exact16 arithmetic", False)
    # (ONE fp32 accumulator over the 1152 products, the slowest-converging order there is: the yardstick of the f32 rule sits at 0.54 here)
    _pair_judged(R.conv3x3(x.value, wt, F32, **kw)[0], ref64, "plain fp32", False, below=1.0)
    for what, sl in (("in0 lo", slice(0, 64)), ("in1 lo", slice(64, 128))):
        xl = x.lo.clone()
        xl[:, sl] = 0.0
        rec = _pair_judged(R.epilogue(_x2_acc(x.hi, xl, wt), F64, **kw)[0], ref64, what + " dropped", True)
        assert rec["frac_bad"] > 0.2, rec
    _pair_judged(R.epilogue(_x2_acc(x.hi, x.lo, wt, w1=False), F64, **kw)[0], ref64, "W1 dropped", True)


@pytest.mark.parametrize("where", ["col31", "col32", "row7", "row8"])
def test_pair_rule_rejects_lost_residual_halves_chunks_and_seam_taps(where):
    """rdb_conv5_res (cin 192, cout 64, two residuals, 2 x 16 x 70): the lo tensor of either residual lost, the lo plane of ONE of
    the six input chunks lost (a pair chunk read as a single one), one tap of one channel lost next to a tile seam."""
    _, x, wt, bias, r0, r1 = _x2_case(192, 64, 2, 16, 70, 22)
    kw = dict(bias=bias, res0=r0.value, s0=0.2, t0=1.0, res1=r1.value, s1=0.2, t1=0.5)
    acc = _x2_acc(x.hi, x.lo, wt)
    ref64 = R.conv3x3(x.value, wt, F64, **kw)[0]
    _pair_judged(R.epilogue(acc, F64, **kw)[0], ref64, "exact16 arithmetic", False)
    if where == "col31":      # (the seam-independent mutants once)
        _pair_judged(R.epilogue(acc, F64, **dict(kw, res0=r0.hi))[0], ref64, "res0 lo dropped", True)
        _pair_judged(R.epilogue(acc, F64, **dict(kw, res1=r1.hi))[0], ref64, "res1 lo dropped", True)
        xl = x.lo.clone()
        xl[:, 96:128] = 0.0
        _pair_judged(R.epilogue(_x2_acc(x.hi, xl, wt), F64, **kw)[0], ref64, "lo of chunk 3 of 6 dropped", True)
    c, k = 17, int(where[3:])
    w0, w1, _ = R.split_weights(wt)
    m = acc.clone()
    if where.startswith("col"):
        dx = 2 if k == 31 else 0
        m[:, :, :, k] -= (w0 + w1)[:, c, 1, dx].view(1, -1, 1) * x.hi[:, c, :, k + dx - 1].unsqueeze(1)
    else:
        dy = 2 if k % 8 == 7 else 0
        m[:, :, k, :] -= (w0 + w1)[:, c, dy, 1].view(1, -1, 1) * x.hi[:, c, k + dy - 1, :].unsqueeze(1)
    _pair_judged(R.epilogue(m, F64, **kw)[0], ref64, "tap dropped at " + where, True)


def test_pair_rule_rejects_a_mask_decided_by_hi_alone_where_hi_is_zero():
    """mask_only (cin 64, cout 64, no bias, 1 x 40 x 72) with a saved activation a third of whose values are +-1e-9: their hi half is
    zero and their sign is the lo half's (include/resr.h, mask_lo_offset)."""
    g, x, wt, _, _, _ = _x2_case(64, 64, 1, 40, 72, 23)
    act = torch.randn(1, 64, 40, 72, generator=g)
    act = torch.where(torch.rand(act.shape, generator=g) < 0.33, act.sign() * 1e-9, act)
    mk = _Pair(act)
    assert ((mk.hi == 0) & (mk.lo > 0)).sum() > 1000
    acc = _x2_acc(x.hi, x.lo, wt)
    ref64 = R.conv3x3(x.value, wt, F64, mask=mk.value, slope=0.2)[0]
    _pair_judged(R.epilogue(acc, F64, mask=mk.value, slope=0.2)[0], ref64, "exact16 arithmetic", False)
    _pair_judged(R.epilogue(acc, F64, mask=mk.hi, slope=0.2)[0], ref64, "mask from hi alone", True)


def test_x2_wgrad_rule_rejects_lost_halves_and_a_skipped_tap_product():
    """w_64_32 (cin 64, cout 32, 2 x 19 x 45) under |got - ref64| <= A + wgrad_lolo: the three tap-products with X_lo^T G_lo dropped
    pass; X's lo tensor lost, G's lost (dW and db), and the (x_lo, g_hi) tap-product skipped in one of three pixel splits do not."""
    g = torch.Generator().manual_seed(7)
    n, cin, cout, h, w = 2, 64, 32, 19, 45
    x, gy = _Pair(torch.randn(n, cin, h, w, generator=g)), _Pair(torch.randn(n, cout, h, w, generator=g))
    dw64, db64 = R.wgrad(x.value, gy.value, 0.5, F64)
    dw32, db32 = R.wgrad(x.value, gy.value, 0.5, F32)
    extra = R.wgrad_lolo(x.value, gy.value, 0.5)

    def dw_of(*products):
        return sum(R.wgrad(a, b, 0.5, F64)[0] for a, b in products)
    three = ((x.hi, gy.hi), (x.hi, gy.lo), (x.lo, gy.hi))
    lolo = dw_of((x.lo, gy.lo))
    assert (lolo.abs() <= extra).all()                    # the term is what it claims to be: a bound of the dropped product
    rec = R.judge(dw_of(*three).float(), dw64, dw32, "f32", extra)
    print(f"three tap-products: ratio {rec['ratio']:.3g}; lo.lo / bound {float((lolo.abs() / R.bound(dw64, rec['allowance'], 'f32', extra)).max()):.3g}")
    assert rec["bad"] == 0 and rec["ratio"] < 0.5, rec
    assert R.judge(db64.float(), db64, db32, "f32")["bad"] == 0
    for what, products in (("X lo", three[:2]), ("G lo", (three[0], three[2]))):
        rec = R.judge(dw_of(*products).float(), dw64, dw32, "f32", extra)
        print(f"{what} dropped: ratio {rec['ratio']:.3g} beyond {rec['frac_bad']:.2%}")
        assert rec["bad"] > 0 and rec["frac_bad"] > 0.5, (what, rec)
    assert R.judge(R.wgrad(x.value, gy.hi, 0.5, F64)[1].float(), db64, db32, "f32")["bad"] > 0      # db from G's hi tensor alone
    band = torch.zeros(n, 1, h, w, dtype=F64)
    band[0, :, :13] = 1.0                                  # a third of the pixels: the first of three pixel splits
    skipped = dw_of(*three) - R.wgrad(x.lo, gy.hi * band, 0.5, F64)[0]
    rec = R.judge(skipped.float(), dw64, dw32, "f32", extra)
    print(f"(x_lo, g_hi) skipped in one split: ratio {rec['ratio']:.3g} beyond {rec['frac_bad']:.2%}")
    assert rec["bad"] > 0, rec


# ---- the 4x4 / stride-2 convolution and the virtual 3x3 kernel the library computes it through ------------------------------------
def _virtual(w4):
    """The virtual 3x3 kernel [cout,4C,3,3] of a [cout,C,4,4] weight by the formula csrc/pack.hip documents: virtual channel ci has
    sub = ci / C, and tap t = ty*3 + tx carries ky = 2*(t/3) + (sub>>1) - 1, kx = 2*(t%3) + (sub&1) - 1, zero outside [0,4)."""
    cout, c = w4.shape[:2]
    w3 = torch.zeros(cout, 4 * c, 3, 3, dtype=w4.dtype)
    for ci in range(4 * c):
        sub, ch = ci // c, ci % c
        for t in range(9):
            ky, kx = 2 * (t // 3) + (sub >> 1) - 1, 2 * (t % 3) + (sub & 1) - 1
            if 0 <= ky < 4 and 0 <= kx < 4:
                w3[:, ci, t // 3, t % 3] = w4[:, ch, ky, kx]
    return w3


def _case4(n=2, c=5, cout=7, h=5, w=6, seed=31):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, c, 2 * h, 2 * w, generator=g), torch.randn(cout, c, 4, 4, generator=g) * (2.0 / (c * 16)) ** 0.5,
            torch.randn(n, cout, h, w, generator=g))


def test_s2d_is_the_library_order_and_d2s_inverts_it():
    from tests import disc_helpers_ref as D
    x, _, _ = _case4()
    p = R.s2d(x)
    assert p.shape == (2, 20, 5, 6)
    assert float(p[1, 3 * 5 + 2, 4, 3]) == float(x[1, 2, 2 * 4 + 1, 2 * 3 + 1])          # sub = 3: (i, j) = (1, 1)
    assert float(p[0, 1 * 5 + 4, 2, 5]) == float(x[0, 4, 2 * 2 + 0, 2 * 5 + 1])          # sub = 1: (i, j) = (0, 1)
    assert np.array_equal(p.permute(0, 2, 3, 1).numpy(), D.s2d_ref(x.permute(0, 2, 3, 1).numpy()))
    assert torch.equal(R.d2s(p), x)


def test_4x4s2_references_against_torch():
    x, w4, gy = _case4()
    conv = F.conv2d(x.double(), w4.double(), stride=2, padding=1)
    assert (R.correlate4x4s2(x, w4, F64) - conv).abs().max().item() < 1e-13
    assert (R.correlate4x4s2(x, w4, F32).double() - conv).abs().max().item() < 1e-5
    got, _ = R.conv4x4s2(x, w4, F64, lrelu=True, slope=0.2)
    assert (got - F.leaky_relu(conv, float(np.float32(0.2)))).abs().max().item() < 1e-13
    tr = F.conv_transpose2d(gy.double(), w4.double(), stride=2, padding=1)
    assert tr.shape == x.shape and (R.dgrad4x4s2(gy, w4, F64) - tr).abs().max().item() < 1e-13
    assert (R.dgrad4x4s2(gy, w4, F32).double() - tr).abs().max().item() < 1e-5
    wt = w4.double().clone().requires_grad_(True)
    (F.conv2d(x.double(), wt, stride=2, padding=1) * gy.double()).sum().backward()
    assert (R.wgrad4x4s2(x, gy, 0.5, F64) - 0.5 * wt.grad).abs().max().item() < 1e-13
    assert (R.wgrad4x4s2(x, gy, 0.5, F32).double() - 0.5 * wt.grad).abs().max().item() < 1e-4
    # the adjoint pair: <conv(x), g> = <x, dgrad(g)>
    assert abs(float((conv * gy.double()).sum() - (x.double() * tr).sum())) < 1e-10


def test_virtual_kernel_over_s2d_equals_the_4x4s2_definition():
    """Forward, transposed pass and the fold of the 3x3 weight gradient: the dense 3x3 operation with the virtual kernel over the
    space-to-depth image IS the 4x4 / stride-2 operation on the original image (float64, to rounding)."""
    from tests import disc_helpers_ref as D
    x, w4, gy = _case4()
    w3 = _virtual(w4)
    assert np.array_equal(w3.numpy(), D.virtual_ref(w4.numpy()))
    assert (R.correlate(R.s2d(x), w3, F64) - R.correlate4x4s2(x, w4, F64)).abs().max().item() < 1e-13
    # backward-data: the 3x3 convolution of g with the transposed, tap-flipped virtual kernel gives the s2d image of the input gradient
    w3t = w3.permute(1, 0, 2, 3).flip(2, 3)
    assert (R.d2s(R.correlate(gy, w3t, F64)) - R.dgrad4x4s2(gy, w4, F64)).abs().max().item() < 1e-13
    # weight gradient: each real tap reads the one virtual tap that carries it
    dw3, _ = R.wgrad(R.s2d(x), gy, 0.5, F64)
    folded = torch.from_numpy(D.fold_ref(dw3.numpy()))
    assert (folded - R.wgrad4x4s2(x, gy, 0.5, F64)).abs().max().item() < 1e-13
    # ... and the 3x3 gradient is NOT zero in the blocks the virtual kernel leaves empty: a kernel that skips them stores something else
    assert (dw3[:, ~R.live_mask(5)].abs() > 1e-3).any()


def test_sixteen_of_36_blocks_are_live_and_they_are_the_ones_the_kernel_names():
    _, w4, _ = _case4()
    w4 = w4.abs() + 1.0                                      # no accidental zeros
    w3 = _virtual(w4)
    c = w4.shape[1]
    live = {(sub, ty, tx) for sub in range(4) for ty in range(3) for tx in range(3) if (w3[:, sub * c:(sub + 1) * c, ty, tx] != 0).any()}
    dead = {(sub, ty, tx) for sub in range(4) for ty in range(3) for tx in range(3) if (w3[:, sub * c:(sub + 1) * c, ty, tx] == 0).all()}
    assert len(live) == 16 and len(dead) == 20
    # csrc/conv3x3_ws.h, sparse_stage, SP = 1: i = 0 -> ty in {1,2}, i = 1 -> ty in {0,1}; tx by j alike
    rows = {0: (1, 2), 1: (0, 1)}
    assert live == {(i * 2 + j, ty, tx) for i in range(2) for j in range(2) for ty in rows[i] for tx in rows[j]}
    assert all(set(R.live_taps(sub)) == {(ty, tx) for s, ty, tx in live if s == sub} for sub in range(4))
    assert int(R.live_mask(c).sum()) == 16 * c and (w3[:, R.live_mask(c)] != 0).all() and (w3[:, ~R.live_mask(c)] == 0).all()
    # SP = 2 (backward-data, taps flipped: pack.hip t = 8 - tap): i = 0 -> {0,1}, i = 1 -> {1,2}
    w3t = w3.permute(1, 0, 2, 3).flip(2, 3)                 # [4C (M), cout (K), 3, 3]
    live_t = {(sub, ty, tx) for sub in range(4) for ty in range(3) for tx in range(3) if (w3t[sub * c:(sub + 1) * c, :, ty, tx] != 0).any()}
    rows_t = {0: (0, 1), 1: (1, 2)}
    assert live_t == {(i * 2 + j, ty, tx) for i in range(2) for j in range(2) for ty in rows_t[i] for tx in rows_t[j]}
    assert all(set(R.live_taps(sub, transposed=True)) == {(ty, tx) for s, ty, tx in live_t if s == sub} for sub in range(4))


def test_rule_rejects_an_index_mutation_of_the_sparse_stage():
    """What tests/test_gpu_sparse_taps.py must be able to see: the forward pass with the two column offsets of sub-position j exchanged
    (each sub-position multiplies its two live tap columns against the wrong pair of halo columns) -- every index still inside the
    3x3 window, no value out of place but the selection.  Both storage rules reject it; the unmutated evaluation passes."""
    g = torch.Generator().manual_seed(41)
    n, c, cout, h, w = 1, 32, 64, 9, 33
    x = _q(torch.randn(n, c, 2 * h, 2 * w, generator=g), "f16")
    w4 = _q(torch.randn(cout, c, 4, 4, generator=g) * (2.0 / (c * 16)) ** 0.5, "f16")
    ref64, _ = R.conv4x4s2(x, w4, F64, lrelu=True, slope=0.2)
    ref32, _ = R.conv4x4s2(x, w4, F32, lrelu=True, slope=0.2)
    w3 = _virtual(w4)
    xs = R.s2d(x)
    assert R.judge(_store(R.conv3x3(xs, w3, F64, lrelu=True, slope=0.2)[0], "f16"), ref64, ref32, "f16")["bad"] == 0
    xp = torch.zeros(n, 4 * c, h + 2, w + 2, dtype=F64)
    xp[:, :, 1:-1, 1:-1] = xs
    acc = torch.zeros(n, cout, h, w, dtype=F64)
    for sub in range(4):
        dx0 = 1 if (sub & 1) == 0 else 0
        wrong_dx0 = 1 - dx0                                  # the mutation
        for ty, tx in R.live_taps(sub):
            sx = wrong_dx0 + (tx - dx0)
            acc += torch.einsum("oc,nchw->nohw", w3[:, sub * c:(sub + 1) * c, ty, tx].double(), xp[:, sub * c:(sub + 1) * c, ty:ty + h, sx:sx + w])
    wrong = R.epilogue(acc, F64, lrelu=True, slope=0.2)[0]
    for kind in ("f16", "pair"):
        rec = R.judge(_store(wrong, "f16") if kind == "f16" else wrong, ref64, ref32, kind)
        assert rec["frac_bad"] > 0.9, (kind, rec)
