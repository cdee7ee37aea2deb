"""CPU: tests/conv_ref.py is right (against torch's own operators and float64 autograd), and the rule it carries has the power the
GPU tests rely on: the plain fp32 evaluation of every case passes with a ratio <= 0.25, every wrong kernel listed below is
rejected.  A "wrong kernel" is the float64 reference with ONE defect, stored as a correct kernel would store it."""
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
