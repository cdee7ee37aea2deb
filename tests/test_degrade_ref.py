"""CPU: tests/degrade_ref.py is right (against torch's own operators and float64 autograd), and the rule of tests/conv_ref.py has, at
the shapes tests/test_gpu_degrade_kernels.py runs, the power that module relies on: the plain fp32 evaluation of every case passes
with a ratio <= 0.25, every wrong kernel listed below is rejected.  A "wrong kernel" is the float64 reference with ONE defect, stored
as a correct kernel would store it (fp32)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as C
from tests import degrade_ref as R

F64, F32 = torch.float64, torch.float32


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- the references are right ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kh,kw,per_sample", [((2, 3, 9, 12), 3, 5, 0), ((2, 3, 9, 12), 5, 3, 1), ((1, 2, 11, 11), 21, 21, 0),
                                                    ((2, 1, 4, 4), 7, 7, 1), ((1, 1, 26, 30), 1, 51, 0), ((1, 1, 30, 26), 51, 1, 0)])
def test_correlate_reflect_against_torch(shape, kh, kw, per_sample):
    g = _gen(kh * 100 + kw)
    x = torch.rand(shape, generator=g, dtype=F64)
    k = R.signed_kernel(kh, kw, g, shape[0] if per_sample else 1).double()
    xp = F.pad(x, (kw // 2, kw // 2, kh // 2, kh // 2), mode="reflect")
    want = torch.cat([F.conv2d(xp[i:i + 1].transpose(0, 1), k[i if per_sample else 0].view(1, 1, kh, kw)).transpose(0, 1) for i in range(shape[0])])
    assert (R.correlate_reflect(x, k, F64) - want).abs().max().item() < 1e-13
    assert (R.correlate_reflect(x, k, F32).double() - want).abs().max().item() < 1e-5


@pytest.mark.parametrize("mode", R.RESIZE_MODES)
def test_resize_against_torch(mode):
    kw = {} if mode == "area" else {"align_corners": False}
    for name in R.RESIZE_CASES:
        x, oh, ow, scale = R.resize_case(name)
        if scale is not None:
            continue                     # (float32(1 / 3.7) is the kernel's constant, not torch's float64 one: the factors below are exact)
        want = F.interpolate(x.double(), size=(oh, ow), mode=mode, **kw)
        assert (R.resize(x, oh, ow, mode, None, F64) - want).abs().max().item() < 1e-13, name
    x = torch.rand(2, 3, 33, 65, generator=_gen(1))
    for scale in (0.25, 0.64, 1.6, 3.2, 4.0):         # 1 / scale is a float32: torch's coordinate scale is the reference's
        assert float(np.float32(1.0 / scale)) == 1.0 / scale
        want = F.interpolate(x.double(), scale_factor=scale, mode=mode, **kw)
        got = R.resize(x, want.shape[2], want.shape[3], mode, scale, F64)
        assert (got - want).abs().max().item() < 1e-12, scale
    same = R.resize(x, 33, 65, mode, None, F64)
    assert torch.equal(same, x.double())


@pytest.mark.parametrize("shape,ksize", [((2, 2, 12, 14), 5), ((1, 1, 26, 30), 51)])
def test_usm_backward_against_autograd(shape, ksize):
    from oracle import imgproc_ref as I
    g = _gen(ksize)
    k1d = (R.signed_kernel(1, ksize, g).reshape(ksize) if ksize == 5 else torch.from_numpy(I.gaussian_kernel_1d(51))).double()
    k2d = torch.outer(k1d, k1d).unsqueeze(0)
    x = torch.rand(shape, generator=g, dtype=F64)
    res = (x - I.filter2d(x, k2d)).abs() * 255
    assert (res - 10).abs().min().item() > 1e-3, "an element sits on the threshold: the mask is not locally constant"
    xr = x.clone().requires_grad_(True)
    gy = torch.randn(shape, generator=g, dtype=F64)
    w = float(np.float32(0.5))
    (I.usm_sharp(xr, k2d, w, 10) * gy).sum().backward()
    blur = I.filter2d(x, k2d)
    soft = I.filter2d((res > 10).double(), k2d)
    pre = x + w * (x - blur)
    assert ((pre < 0) | (pre > 1)).double().mean().item() > 0.02 and (soft > 0).double().mean().item() > 0.5, "nothing is clipped"
    got = R.usm_backward(x, blur, soft, gy, k1d, 0.5, F64)
    assert (got - xr.grad).abs().max().item() < 1e-12
    got32 = R.usm_backward(x.float(), blur.float(), soft.float(), gy.float(), k1d.float(), 0.5, F32)
    assert (got32.double() - xr.grad).abs().max().item() < 1e-4


def test_finish_and_gaussian_noise_against_the_oracle():
    from oracle import imgproc_ref as I
    g = _gen(3)
    x = torch.rand(3, 3, 6, 5, generator=g, dtype=F64) * 1.6 - 0.3
    for mode in range(4):
        assert torch.equal(R.finish(x, mode), I._finish(x, bool(mode & 1), bool(mode & 2))), mode
    sigma, gray = torch.rand(3, generator=g, dtype=F64) * 30, torch.tensor([1.0, 0.0, 1.0], dtype=F64)
    fg, fc = torch.randn(6, 5, generator=g, dtype=F64), torch.randn(3, 3, 6, 5, generator=g, dtype=F64)
    want = x + I.gaussian_noise_from_fields(x, sigma, gray, fg, fc)
    assert (R.gaussian_noisy(x, sigma, gray, fg, fc) - want).abs().max().item() < 1e-15
    want = x + I.gaussian_noise_from_fields(x, sigma, torch.zeros(3, dtype=F64), fg, fc)
    assert (R.gaussian_noisy(x, sigma, gray, None, fc) - want).abs().max().item() < 1e-15      # no gray field: colour noise for everyone


def test_poisson_decode_recovers_the_draws():
    from oracle import imgproc_ref as I
    g = _gen(4)
    x = torch.round(torch.rand(3, 3, 8, 9, generator=g) * 255) / 255
    x[1] = x[1, :1]                                                                    # r = g = b
    scale, gray = torch.tensor([0.5, 2.0, 1.0]), torch.tensor([0.0, 1.0, 0.0])
    v = I.poisson_vals(x).view(3)
    vg = I.poisson_vals(I.quantize(I.rgb_to_gray(x))).view(3)
    draws = torch.poisson(x * v.view(3, 1, 1, 1), generator=g)
    gdraws = torch.poisson(I.quantize(I.rgb_to_gray(x)) * vg.view(3, 1, 1, 1), generator=g)
    it = iter([gdraws, draws])
    out = x + I.poisson_noise(x, scale, gray, sampler=lambda lam: next(it))
    col, gr = R.poisson_decode(x, out, scale, gray, torch.stack([v, vg], dim=1))
    assert (col[[0, 2]] - draws[[0, 2]]).abs().max().item() < 1e-3 and (gr[1] - gdraws[1]).abs().max().item() < 1e-3


def test_jpeg_preround_rounds_to_the_oracles_coefficients():
    from oracle import imgproc_ref as I
    x = torch.rand(2, 3, 20, 37, generator=_gen(5))
    q = torch.tensor([30.0, 80.0])
    _, c = I.diff_jpeg(x, q, return_coeffs=True)
    want = torch.cat([c["y"], c["cb"], c["cr"]], dim=1).reshape(2, -1, 64)
    pre = R.jpeg_preround(x, q)
    assert pre.shape == want.shape
    safe = (pre - pre.floor() - 0.5).abs() > 1e-3
    assert safe.double().mean().item() > 0.99 and torch.equal(torch.round(pre)[safe], want.double()[safe])
    assert R.jpeg_factor([49.99, 50.0, 50.01]).tolist() == [float(np.float32(np.float32(5000.0) / np.float32(49.99)) / np.float32(100.0)), 1.0,
                                                            float((np.float32(200.0) - np.float32(50.01) * np.float32(2.0)) / np.float32(100.0))]


# ---- the rule has power -----------------------------------------------------------------------------------------------------------------
def _passes(ref64, ref32):
    """The unmutated fp32 evaluation: ratio <= 0.25 by construction."""
    rec = C.judge(ref32, ref64, ref32, "f32")
    assert rec["bad"] == 0 and rec["ratio"] <= 0.25, rec


def _rejected(mutant64, ref64, ref32, what):
    rec = C.judge(mutant64.float(), ref64, ref32, "f32")
    assert rec["bad"] > 0, (what, rec)


def _shifted(x, k, axis):
    """Correlation with the tap origin one pixel off along `axis`: the reflect-padded image grows by one replicated line at its far
    end and every window starts one line later."""
    x, k = x.double(), k.double()
    n, c, h, w = x.shape
    kh, kw = k.shape[-2:]
    p = x.index_select(2, R.pad_index(h, kh // 2)).index_select(3, R.pad_index(w, kw // 2))
    p = F.pad(p, (0, 1, 0, 0) if axis == 3 else (0, 0, 0, 1), mode="replicate")
    oy, ox = (0, 1) if axis == 3 else (1, 0)
    acc = torch.zeros(n, c, h, w, dtype=F64)
    for dy in range(kh):
        for dx in range(kw):
            acc += p[:, :, dy + oy:dy + oy + h, dx + ox:dx + ox + w] * k[:, dy, dx].view(-1, 1, 1, 1)
    return acc


@pytest.mark.parametrize("name", sorted(R.FILTER_CASES))
def test_rule_rejects_wrong_filters(name):
    x, k = R.filter_case(name)
    kh, kw = k.shape[-2:]
    ref64, ref32 = R.correlate_reflect(x, k, F64), R.correlate_reflect(x, k, F32)
    _passes(ref64, ref32)
    if kh * kw > 1:                                   # (a 1 x 1 kernel pads nothing and has no orientation)
        _rejected(R.correlate_reflect(x, k, F64, pad="edge"), ref64, ref32, "replicate padding")
        _rejected(R.correlate_reflect(x, k, F64, pad="symmetric"), ref64, ref32, "symmetric padding")
        _rejected(R.correlate_reflect(x, k.flip(-1, -2), F64), ref64, ref32, "convolution")
    if kh == kw and kh > 1:
        _rejected(R.correlate_reflect(x, k.transpose(-1, -2), F64), ref64, ref32, "kernel transposed")
    if kw > 1 or kh == 1:
        _rejected(_shifted(x, k, 3), ref64, ref32, "tap origin one column off")
    if kh > 1 or kw == 1:
        _rejected(_shifted(x, k, 2), ref64, ref32, "tap origin one row off")
    if k.shape[0] > 1:
        _rejected(R.correlate_reflect(x, k.flip(0), F64), ref64, ref32, "the other sample's kernel")
        _rejected(R.correlate_reflect(x, k[:1], F64), ref64, ref32, "sample 0's kernel for everyone")


# the cases where a defect changes the function at all: bilinear meets a negative source coordinate only when an axis with more
# than one pixel grows; an area window's end is an integer either way when out divides in; a scale factor exists in two cases
_UPSCALED = ["33x65_up3.7", "48x40_to_97x5", "2x2_to_9x9", "seven_planes_9x11_to_4x13"]
_RAGGED_WINDOWS = ["33x65_up3.7", "33x65_down0.15", "48x40_to_97x5", "one_row_to_5x5", "one_column_to_5x5", "2x2_to_9x9", "seven_planes_9x11_to_4x13"]
_WITH_FACTOR = ["33x65_up3.7", "33x65_down0.15"]


@pytest.mark.parametrize("name", sorted(R.RESIZE_CASES))
def test_rule_rejects_wrong_resizes(name):
    x, oh, ow, scale = R.resize_case(name)
    ref = {m: (R.resize(x, oh, ow, m, scale, F64), R.resize(x, oh, ow, m, scale, F32)) for m in R.RESIZE_MODES}
    for m in R.RESIZE_MODES:
        _passes(*ref[m])
    _rejected(R.resize(x, oh, ow, "bicubic", scale, F64, cubic_a=-0.5), *ref["bicubic"], "bicubic with A = -0.5")
    if name in _UPSCALED:
        _rejected(R.resize(x, oh, ow, "bilinear", scale, F64, clamp_at_zero=False), *ref["bilinear"], "bilinear without the clamp at 0")
    if name in _RAGGED_WINDOWS:
        _rejected(R.resize(x, oh, ow, "area", scale, F64, area_end="floor"), *ref["area"], "area window ending at floor")
    if name in _WITH_FACTOR:
        for m in ("bilinear", "bicubic"):
            _rejected(R.resize(x, oh, ow, m, None, F64), *ref[m], m + " with in / out for 1 / scale")
    if x.shape[0] * x.shape[1] > 1:
        _rejected(ref["bilinear"][0].flip(0).flip(1), *ref["bilinear"], "planes in the wrong order")


def test_every_resize_defect_meets_a_case():
    assert set(_UPSCALED) | set(_RAGGED_WINDOWS) | set(_WITH_FACTOR) <= set(R.RESIZE_CASES)
    assert set(R.RESIZE_CASES) - set(_RAGGED_WINDOWS) == {"48x40_to_1x1"}


@pytest.mark.parametrize("name", sorted(R.USM_BWD_CASES))
def test_rule_rejects_wrong_usm_backwards(name):
    x, blur, soft, g, k1d = R.usm_bwd_case(name)
    pre = R.usm_pre(x, blur)
    assert torch.minimum(pre.abs(), (pre - 1).abs()).min().item() > 1e-3
    assert min((pre < 0).double().mean().item(), ((pre > 0) & (pre < 1)).double().mean().item(), (pre > 1).double().mean().item()) >= 0.05
    w = R.USM_WEIGHT
    ref64, ref32 = R.usm_backward(x, blur, soft, g, k1d, w, F64), R.usm_backward(x, blur, soft, g, k1d, w, F32)
    _passes(ref64, ref32)
    h, wd = x.shape[2:]
    for axis, n in ((2, h), (3, wd)):
        for side in ("left", "right"):
            broken = R.blur_matrix(n, k1d, F64, **{side: False})
            mats = (broken, R.blur_matrix(wd, k1d)) if axis == 2 else (R.blur_matrix(h, k1d), broken)
            _rejected(R.usm_backward(x, blur, soft, g, k1d, w, F64, matrices=mats), ref64, ref32,
                      f"adjoint without its {'z(-p)' if side == 'left' else 'z(2(n-1)-p)'} term along axis {axis}")
    _rejected(R.usm_backward(x, blur, soft, g, k1d, w, F64, clip=False), ref64, ref32, "clip indicator dropped")
    _rejected(R.usm_backward(x, blur, soft, g, k1d.flip(0), w, F64), ref64, ref32, "taps run backwards")
    _rejected(R.usm_backward(x, blur, soft, g, k1d, w, F64, matrices=(R.blur_matrix(h, k1d).t(), R.blur_matrix(wd, k1d).t())), ref64, ref32,
              "the blur itself in place of its adjoint")
