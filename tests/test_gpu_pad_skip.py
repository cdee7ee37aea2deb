"""GPU: the kernels that skip work on padding against the paths that compute on it (RESR_NO_PAD_SKIP=1, read per call).

  layout   nchw_to_nhwc with r = 1, c <= 8, f16 takes the few-channel kernel (lane = pixel loads, 1 KB stores): the same bits as the
           generic kernel and as mask ? f16(g * pre) : 0 computed in torch.
  blur     the 21 x 21 taps of resr_filter2d run over the non-zero radius of each sample's kernel only: the same bits as the full
           441-tap loop (the skipped terms are +-0 * finite, the accumulator starts at +0), and the reflect-padded correlation in
           float64 within fp32 rounding of 441 terms.
"""
import math
import struct

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SWITCH = "RESR_NO_PAD_SKIP"


@pytest.fixture(scope="module")
def L():
    import real_esrgan_pytorch_amd as R
    return R._lib


# ---- layout ----------------------------------------------------------------------------------------------------------------------
def _layout(L, g, mask, slot, c_pad=32):
    n, c, h, w = g.shape
    out = torch.full((n, h, w, c_pad), -3.0, dtype=torch.float16, device="cuda")
    L.check(L.lib().resr_debug_nchw_to_nhwc(L.ptr(g), L.ptr(out), n, c, h, w, 1, c_pad, L.RESR_F16, L.ptr(mask) if mask is not None else None,
                                            L.ptr(slot) if slot is not None else None, L.stream_ptr()), "resr_debug_nchw_to_nhwc")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("prescale", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", [(1, 3, 1, 1), (2, 3, 5, 70), (3, 3, 33, 17), (2, 1, 5, 70), (1, 8, 9, 31)])
def test_few_channel_layout_is_the_generic_kernels_bits(L, monkeypatch, shape, masked, prescale):
    n, c, h, w = shape
    gen = torch.Generator().manual_seed(11 + n * 100 + c)
    # gradients as the backward pass meets them: small, some below f16's normal range (the prescale lifts them), some exact zeros
    g = torch.randn(shape, generator=gen) * 3e-4 * torch.pow(10.0, -3.0 * torch.rand(shape, generator=gen))
    g[torch.rand(shape, generator=gen) < 0.05] = 0.0
    mask = (torch.rand(shape, generator=gen) < 0.7).to(torch.uint8).cuda() if masked else None
    m = float(g.abs().max()) or 2.0 ** -12
    slot = torch.tensor([struct.unpack("<i", struct.pack("<f", m))[0], 0, 0], dtype=torch.int32).cuda() if prescale else None
    pre = 2.0 ** -math.floor(math.log2(m)) if prescale else 1.0     # m < 1 and normal: the lift is on (csrc/common.h grad_prescale)
    assert not prescale or (2.0 ** -126 <= m < 1.0 and pre > 1.0)
    gd = g.cuda()
    for c_pad in (32, 8, 24):
        got = _layout(L, gd, mask, slot, c_pad)
        monkeypatch.setenv(SWITCH, "1")
        generic = _layout(L, gd, mask, slot, c_pad)
        monkeypatch.delenv(SWITCH)
        want = torch.zeros(n, h, w, c_pad, dtype=torch.float16, device="cuda")
        v = gd * pre                                                # (exact: a power of two)
        if masked:
            v = torch.where(mask.bool(), v, torch.zeros_like(v))
        want[..., :c] = v.permute(0, 2, 3, 1).half()
        # bit patterns: torch.equal on the values would let -0 pass for +0
        assert torch.equal(got.view(torch.int16), generic.view(torch.int16)), (shape, c_pad, "vs the generic kernel")
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (shape, c_pad, "vs torch")


# ---- blur ------------------------------------------------------------------------------------------------------------------------
def _kernel21(kind, gen):
    k = torch.zeros(21, 21)
    if kind in (7, 13, 21):
        lo = 10 - kind // 2
        core = torch.rand(kind, kind, generator=gen) + 0.05          # no zero tap inside: the radius is the kernel's
        core[0, 0] = -core[0, 0]                                       # a sinc kernel's negative lobes
        k[lo:lo + kind, lo:lo + kind] = core / core.sum()
    elif kind == "centre":
        k[10, 10] = 1.0
    elif kind == "corner":
        k[20, 0] = 0.75
    return k


BLUR_CASES = [7, 13, 21, "centre", "corner"]


@pytest.fixture(scope="module")
def blur_image():
    return torch.rand(2, 3, 37, 70, generator=torch.Generator().manual_seed(5))


@pytest.mark.parametrize("case", range(len(BLUR_CASES)))
def test_blur_zero_border_skip_is_bit_identical(L, monkeypatch, blur_image, case):
    """Sample 0 carries the case's kernel, sample 1 the next case's: two radii in one launch."""
    gen = torch.Generator().manual_seed(40 + case)
    kern = torch.stack([_kernel21(BLUR_CASES[case], gen), _kernel21(BLUR_CASES[(case + 1) % len(BLUR_CASES)], gen)])
    x, kd = blur_image.cuda(), kern.cuda()

    def run():
        out = torch.full_like(x, -5.0)
        L.check(L.lib().resr_filter2d(L.ptr(x), L.ptr(out), L.ptr(kd), 2, 3, 37, 70, 21, 21, 1, L.stream_ptr()), "resr_filter2d")
        torch.cuda.synchronize()
        return out

    got = run()
    monkeypatch.setenv(SWITCH, "1")
    full = run()
    monkeypatch.delenv(SWITCH)
    assert torch.equal(got.view(torch.int32), full.view(torch.int32))
    # and the definition: reflect pad 10, correlation, in float64.  441 fused multiply-adds, each rounding a partial sum below 2
    xp = F.pad(blur_image.double(), (10, 10, 10, 10), mode="reflect")
    ref = torch.cat([F.conv2d(xp[i:i + 1].transpose(0, 1), kern[i].double().view(1, 1, 21, 21)).transpose(0, 1) for i in range(2)])
    assert (got.cpu().double() - ref).abs().max().item() < 441 * 2.0 ** -23
