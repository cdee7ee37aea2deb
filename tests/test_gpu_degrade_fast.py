"""GPU: USMSharp's and DiffJPEG's stream kernels (csrc/degrade.hip usm51_stream_kernel, jpeg_run_kernel) against the kernels they
replace (RESR_DEGRADE_PARENT_KERNELS=1, read per call): the same call twice through the entry points of tests/test_gpu_degrade.py,
and every tensor the call leaves must be the same bits -- torch.equal on the values and on their bit patterns, no tolerance.

  USM   out, the gradient of a backward pass (it reads the forward's blur and soft), and blur, soft and the mask bytes out of the
        tensor the forward saves for it ([mask bytes (+ unused) | blur | soft]).
  JPEG  dst and coeffs; qualities on both branches of the quality factor, with and without the folded input clamp, with and
        without a coefficient buffer, inputs slightly outside [0, 1].

The judgments against float64 and the goldens (tests/test_gpu_degrade_kernels.py, tests/test_gpu_degrade.py,
tests/test_gpu_pipeline_golden.py) run the stream kernels by default: they say the values are right, this file that none moved.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SWITCH = "RESR_DEGRADE_PARENT_KERNELS"


@pytest.fixture(scope="module")
def ip():
    from real_esrgan_pytorch_amd import imgproc
    return imgproc


def same_bits(a, b):
    return torch.equal(a, b) and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# (n, c, h, w): the smallest sizes at which each mechanism of the strip walk can go wrong
USM_SHAPES = [
    (1, 3, 26, 26),      # smallest size reflect padding allows; one ragged strip; one chunk
    (3, 1, 31, 97),      # two strips, the second 33 wide; h < 32
    (2, 3, 72, 64),      # exactly one strip; three row tiles, the last 8 rows; 16-byte aligned rows (float4 epilogue)
    (2, 3, 130, 67),     # a 3-column strip; odd width, so unaligned wide stores (scalar epilogue)
    (1, 2, 70, 130),     # three strips
    (1, 1, 500, 30),     # strip narrower than the halo; 4 segments
    (1, 1, 1000, 70),    # 8 segments: ring fill at every segment start
    (1, 2, 40, 132),     # aligned rows over three strips, the last one column group wide: the float4 epilogue at a strip's ragged end
]


@pytest.mark.parametrize("shape", USM_SHAPES)
def test_usm_stream_kernels_are_the_parent_kernels_bits(ip, monkeypatch, shape):
    n, c, h, w = shape
    gen = torch.Generator().manual_seed(h * w)
    # image-like, as in test_usm_two_launches_equal_six_passes: smooth structure plus noise, so that the mask fires
    x = F.interpolate(torch.rand(n, c, max(2, h // 8), max(2, w // 8), generator=gen), size=(h, w), mode="bicubic").clamp(0, 1)
    x = (0.8 * x + 0.2 * torch.rand(n, c, h, w, generator=gen)).clamp(0, 1)
    usm = ip.USMSharp(50, 0).cuda()
    gw = torch.rand(n, c, h, w, generator=gen).cuda()
    count = n * c * h * w

    def run():
        xd = x.cuda().requires_grad_(True)
        y = usm(xd, 0.5, 10)
        tmp = y.grad_fn.saved_tensors[1]          # [mask bytes (+ unused) | blur | soft], count floats each
        mask = tmp[:count].view(torch.uint8)[:count].clone()
        blur, soft = tmp[count:2 * count].clone(), tmp[2 * count:3 * count].clone()
        y.backward(gw)
        torch.cuda.synchronize()
        return {"out": y.detach().clone(), "grad": xd.grad.clone(), "blur": blur, "soft": soft, "mask": mask}

    monkeypatch.setenv(SWITCH, "1")
    want = run()
    monkeypatch.delenv(SWITCH)
    got = run()
    frac = ((got["out"].cpu() - x).abs() > 1e-6).float().mean().item()
    assert frac > 0.01, "the mask never fired: the test image is too smooth to exercise the sharpening branch"
    assert 0 < want["mask"].sum().item() < count
    assert torch.equal(got["mask"], want["mask"]), "mask bytes"
    for name in ("blur", "soft", "out", "grad"):
        assert same_bits(got[name], want[name]), (name, (got[name] - want[name]).abs().max().item())

    # without a graph the soft mask is not stored: the same output again
    with torch.no_grad():
        y = usm(x.cuda(), 0.5, 10)
    assert same_bits(y, want["out"])


JPEG_SHAPES = [
    (1, 3, 1, 1),        # everything is padding
    (2, 3, 7, 9),        # less than one macroblock
    (1, 3, 16, 16),      # exactly one macroblock
    (2, 3, 33, 17),      # ragged both ways; two images in one launch
    (3, 3, 40, 100),     # 7 macroblocks per row: a ragged run; three qualities
    (1, 3, 48, 272),     # 17 per row; exact multiples of 16
]
QUALITIES = [10.0, 49.5, 50.0, 95.0]   # both branches of the quality factor, and their border


@pytest.mark.parametrize("with_coeffs", [False, True])
@pytest.mark.parametrize("clamp_input", [False, True])
@pytest.mark.parametrize("shape", JPEG_SHAPES)
def test_jpeg_run_kernel_is_the_parent_kernels_bits(ip, monkeypatch, shape, clamp_input, with_coeffs):
    n, c, h, w = shape
    gen = torch.Generator().manual_seed(7 * h + w)
    x = F.interpolate(torch.rand(n, c, max(2, h // 4), max(2, w // 4), generator=gen), size=(h, w), mode="bilinear")
    x = 1.1 * (0.85 * x + 0.15 * torch.rand(n, c, h, w, generator=gen)) - 0.05   # in [-0.05, 1.05]
    x.view(-1)[0], x.view(-1)[-1] = -0.03, 1.04                                     # surely outside [0, 1], at any size
    x = x.cuda()
    first = int(torch.randint(0, 4, (1,), generator=gen))
    quality = torch.tensor([QUALITIES[(first + i) % 4] for i in range(n)])
    jpeg = ip.DiffJPEG(False).cuda()

    def run():
        r = jpeg(x, quality.clone(), return_coeffs=with_coeffs, clamp_input=clamp_input)
        torch.cuda.synchronize()
        return r if with_coeffs else (r, None)

    monkeypatch.setenv(SWITCH, "1")
    want, want_c = run()
    monkeypatch.delenv(SWITCH)
    got, got_c = run()
    assert same_bits(got, want), (got - want).abs().max().item()
    if with_coeffs:
        assert got_c.shape == (n, ((h + 15) // 16) * ((w + 15) // 16) * 6, 64)
        assert same_bits(got_c, want_c), (got_c - want_c).abs().max().item()
        assert got_c.abs().max().item() > 0 or h * w == 1
