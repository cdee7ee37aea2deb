"""-m gpu: the native NIQE end to end -- `niqe_native` from float and from uint8 input against `niqe()`, the golden scores, `validate()`
under config.niqe_backend = "native", `inference_frames --niqe`, and stream order.

Tolerance.  `niqe()` on the CPU and on the GPU are two float64 re-orderings of one definition; their difference on an input is that
definition's own order sensitivity there (the 36 x 36 pseudo-inverse amplifies the last bits of the features).  The native path is a
third ordering: it is held to 10 x that difference, measured here on the same inputs, with a floor of 1e-12.  The golden images are
repaired first (tests/niqe_ref.repair_ties), so that the native luma -- one stated fp32 order -- and torch's matmul round alike.
Measured on an MI355X: DESIGN.md, "Native NIQE"."""
import os
import types

import numpy as np
import pytest
import torch

from tests import niqe_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "niqe.npz"))
MODEL = os.path.join(HERE, "golden", "niqe_model.mat")
FLOOR = 1e-12


@pytest.fixture(scope="module")
def Q():
    from real_esrgan_pytorch_amd import image_quality_assessment
    return image_quality_assessment


def _score(t):
    return np.atleast_1d(t.detach().double().cpu().numpy())


@pytest.fixture(scope="module")
def golden(Q):
    """Per golden image: the repaired uint8 image [B,H,W,3], its float form, crop, niqe() on the CPU and on the GPU, and the tolerance."""
    out = []
    for i in (0, 1):
        img, nudged = R.repair_ties(np.ascontiguousarray(GOLDEN[f"img{i}"].transpose(0, 2, 3, 1)))
        crop = int(GOLDEN[f"crop{i}"])
        x = torch.from_numpy(R.unit_of_u8(img))
        m = Q.NIQE(crop, MODEL)
        cpu, gpu = _score(m(x)), _score(m.cuda()(x.cuda()))
        diff = float(np.abs(cpu - gpu).max())
        out.append({"img": img, "x": x, "crop": crop, "cpu": cpu, "gpu": gpu, "diff": diff, "tol": max(10 * diff, FLOOR), "nudged": nudged})
    return out


@pytest.mark.parametrize("i", [0, 1])
def test_score_from_float_and_from_uint8_equals_niqe_on_repaired_golden_images(Q, golden, i):
    g = golden[i]
    m = Q.NativeNIQE(g["crop"], MODEL).cuda()
    from_float, from_u8 = _score(m(g["x"].cuda())), _score(m(torch.from_numpy(g["img"]).cuda()))
    print(f"golden{i}: niqe() CPU {g['cpu']} GPU {g['gpu']} |CPU - GPU| {g['diff']:.3e} tolerance {g['tol']:.3e}; "
          f"native - CPU: float {np.abs(from_float - g['cpu']).max():.3e} uint8 {np.abs(from_u8 - g['cpu']).max():.3e}; "
          f"native - GPU: {np.abs(from_float - g['gpu']).max():.3e}; {g['nudged']} pixels repaired")
    assert np.array_equal(from_float, from_u8)                              # one luma, one set of kernels behind it
    assert from_float.shape == g["cpu"].shape and np.isfinite(from_float).all()
    assert np.abs(from_float - g["cpu"]).max() <= g["tol"] and np.abs(from_float - g["gpu"]).max() <= g["tol"]
    # the functional form with the priors the module passes
    mu, cov = m.mu_prisparam.float().double(), m.cov_prisparam.float().double()
    assert np.array_equal(_score(Q.niqe_native(g["x"].cuda(), g["crop"], mu, cov)), from_float)


@pytest.mark.parametrize("i", [0, 1])
def test_unrepaired_golden_images_against_the_reference_scores(Q, i):
    """The stored scores were recorded under ONE machine's matmul order for the luma; torch's order depends on the machine (and on the
    operand's shape and strides), so `niqe()` on the CPU of the machine at hand -- the torch path here -- is computed too.  Where the
    native luma equals the torch path's on every pixel, the native score is held to that torch path's at 10 x the CPU / GPU difference
    of `niqe()` on this image, and to the stored score at rtol 1e-6 whenever the torch path of this machine meets that itself (where
    it does not, its luma is not the one the score was recorded under, and no luma that equals it can be).  Otherwise the deviation is
    printed and not gated.  The case that ran is printed."""
    from real_esrgan_pytorch_amd import imgproc
    x = torch.from_numpy(GOLDEN[f"img{i}"]).float() / 255.0
    crop = int(GOLDEN[f"crop{i}"])
    stored = GOLDEN[f"score{i}"]
    got = _score(Q.NativeNIQE(crop, MODEL).cuda()(x.cuda()))
    dev = float(np.abs(got / stored - 1).max())
    b, _, h, w = x.shape
    lh, lw = (h - 2 * crop) // 96 * 96, (w - 2 * crop) // 96 * 96
    native = Q.niqe_luma_native(x.cuda(), crop, lh, lw).cpu().numpy()
    cropped = x[:, :, crop:-crop, crop:-crop] if crop else x               # as niqe() does: the crop first
    torch_luma = (imgproc.rgb2ycbcr_torch(cropped, only_use_y_channel=True) * 255.0).round()[:, 0, :lh, :lw].numpy()
    differing = int((native != torch_luma).sum())
    assert np.isfinite(got).all()
    if differing:
        print(f"golden{i} unrepaired: {differing} of {native.size} luma levels differ from the torch path's matmul (near-ties); "
              f"reported, not gated: relative deviation from the stored score {dev:.3e}")
        return
    m = Q.NIQE(crop, MODEL)
    here, here_gpu = _score(m(x)), _score(m.cuda()(x.cuda()))
    tol = max(10 * float(np.abs(here - here_gpu).max()), FLOOR)
    here_dev = float(np.abs(here / stored - 1).max())
    print(f"golden{i} unrepaired: the luma equals the torch path's on every pixel; native - niqe() of this machine "
          f"{np.abs(got - here).max():.3e} (tolerance {tol:.3e}); relative deviation from the stored score: native {dev:.3e}, niqe() of this "
          f"machine {here_dev:.3e} -> " + ("gated at rtol 1e-6" if here_dev <= 1e-6 else "the stored score is of another luma: not gated"))
    assert np.abs(got - here).max() <= tol
    if here_dev <= 1e-6:
        np.testing.assert_allclose(got, stored, rtol=1e-6)


class _RepairedOutput(torch.nn.Module):
    """The generator of the validation loop with its output made a repaired 8-bit image (tests/niqe_ref.repair_ties, on the CPU): the
    luma of a float network output lies within an fp32 rounding of a half at a pixel in 10^5 or so, where the native order and torch's
    matmul may round apart ("Native NIQE") -- the harness images are drawn anew in every process, so an unrepaired
    comparison would fail in some runs and pass in others."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, lr):
        sr = self.inner(lr).clamp(0, 1)
        fixed, _ = R.repair_ties((sr * 255).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy())
        return torch.from_numpy(R.unit_of_u8(fixed)).to(lr.device)


def test_validate_through_build_niqe_under_the_native_backend(Q, tmp_path, monkeypatch):
    """`validate()` with the module `config.build_niqe()` makes under either backend, on the harness dataset.  The float64 scores the
    loop feeds its (float32) meter are taken by a forward hook and compared image by image; the tolerance is the module docstring's,
    measured on these very images: 10 x |niqe() on the CPU - niqe() on the GPU|, floor 1e-12."""
    from real_esrgan_pytorch_amd import config
    from real_esrgan_pytorch_amd import train_realesrnet as T
    from tests.test_gpu_train_harness import _tiny_dataset
    _tiny_dataset(tmp_path, monkeypatch, g_arch="compact", compact_num_conv=4)
    torch.manual_seed(0)
    model, ema_model = T.build_model()
    _, _, test_prefetcher = T.load_dataset()
    writer = types.SimpleNamespace(add_scalar=lambda *a: None)
    seen = {"torch": [], "native": []}
    inputs = []
    averages = {}
    for backend, cls in (("torch", Q.NIQE), ("native", Q.NativeNIQE)):
        monkeypatch.setattr(config, "niqe_backend", backend)
        niqe_model = config.build_niqe()
        assert type(niqe_model) is cls and niqe_model.mu_prisparam.is_cuda

        def hook(module, args, output, backend=backend):
            seen[backend].append(_score(output))
            if backend == "torch":
                inputs.append(args[0].cpu())
        niqe_model.register_forward_hook(hook)
        averages[backend] = float(T.validate(_RepairedOutput(model), ema_model, test_prefetcher, 0, writer, niqe_model, "Test"))
    cpu_model = Q.NIQE(config.upscale_factor, config.niqe_model_path)
    assert len(inputs) == 2 and len(seen["native"]) == 2
    for k, sr in enumerate(inputs):
        tol = max(10 * float(np.abs(_score(cpu_model(sr)) - seen["torch"][k]).max()), FLOOR)
        diff = float(np.abs(seen["native"][k] - seen["torch"][k]).max())
        print(f"validate() image {k}: torch {seen['torch'][k]} native {seen['native'][k]} difference {diff:.3e} tolerance {tol:.3e}")
        assert np.isfinite(seen["native"][k]).all() and diff <= tol
    assert np.isfinite(averages["native"]) and abs(averages["native"] - averages["torch"]) < 1e-5     # the float32 meter's own resolution


def test_inference_frames_niqe_prints_the_scores_of_the_written_files(Q, tmp_path, monkeypatch, capsys):
    from PIL import Image
    from real_esrgan_pytorch_amd import config, inference_frames
    from real_esrgan_pytorch_amd.compact import SRVGGNetCompact
    from tests.test_gpu_train_harness import _smooth_png
    monkeypatch.setattr(config, "device", torch.device("cuda", 0))
    torch.manual_seed(0)
    torch.save({"params": SRVGGNetCompact(num_conv=4, upscale=4).state_dict()}, tmp_path / "w.pth")
    (tmp_path / "lr").mkdir()
    names = ["a.png", "b.png"]
    for k, name in enumerate(names):
        _smooth_png(str(tmp_path / "lr" / name), 56, 7 + k)
    inference_frames.main(types.SimpleNamespace(inputs_dir=str(tmp_path / "lr"), output_dir=str(tmp_path / "sr"), weights_path=str(tmp_path / "w.pth"),
                                                depth=2, model_type="compact", num_conv=4, act_type="prelu", precision="fast", niqe=True,
                                                niqe_model_path=MODEL))
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("NIQE ")]
    m = Q.NativeNIQE(config.upscale_factor, MODEL).cuda()
    want = [float(m(torch.from_numpy(np.asarray(Image.open(tmp_path / "sr" / name)))[None].cuda())) for name in names]
    assert np.isfinite(want).all()
    assert lines == [f"NIQE {name}: {v:.6f}" for name, v in zip(names, want)] + [f"NIQE mean: {sum(want) / len(want):.6f}"]


def test_score_follows_the_current_stream(Q, golden):
    """The producer and the metric on a side stream, nothing on the default stream and no host synchronisation in between: a stage
    enqueued anywhere but the current stream would read the frame before the copy behind the matrix products has filled it."""
    g = golden[0]
    m = Q.NativeNIQE(g["crop"], MODEL).cuda()
    frame = torch.from_numpy(g["img"]).cuda()
    want = _score(m(frame))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        late = torch.zeros_like(frame)
        a = torch.full((2048, 2048), 1.0 / 2048, device="cuda")
        for _ in range(50):
            a = a @ a
        late.copy_(frame)
        got = m(late)
    side.synchronize()
    assert np.array_equal(_score(got), want)
