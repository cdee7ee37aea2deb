"""-m gpu: the native PSNR / SSIM end to end -- `NativeFullRef` from float and from uint8 input, against the torch backend, inside
`validate()`, `test.main()` and `inference_frames --reference_dir`, and the errors that name a file.

The native luma is one stated fp32 order; torch's matmul may round a near-tie the other way, so the comparison with the torch backend
runs on images repaired with tests/niqe_ref.repair_ties.  Both backends are then held to the bound of tests/fullref_ref.py around the
longdouble reference (so they lie within twice that of each other)."""
import os
import types

import numpy as np
import pytest
import torch

from tests import fullref_ref as F
from tests import niqe_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL = os.path.join(HERE, "golden", "niqe_model.mat")
PSNR_GATE = 16 * 2.0 ** -52


@pytest.fixture(scope="module")
def Q():
    from real_esrgan_pytorch_amd import image_quality_assessment
    return image_quality_assessment


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def repaired():
    sr, hr = F.pair(77, 3, 61, 83)
    return R.repair_ties(sr)[0], R.repair_ties(hr)[0]


def test_module_from_float_and_from_uint8_gives_the_same_bits(Q, repaired):
    sr, hr = (torch.from_numpy(a).cuda() for a in repaired)
    sr_f, hr_f = (torch.from_numpy(R.unit_of_u8(a)).cuda() for a in repaired)
    m = Q.NativeFullRef(4).cuda()
    want = [_np(t) for t in m(sr, hr)]
    assert want[0].shape == (3,) and want[0].dtype == np.float64 and want[1].dtype == np.float64
    for a, b in ((sr_f, hr_f), (sr, hr_f), (sr_f, hr), (sr_f.double(), hr_f)):
        got = [_np(t) for t in m(a, b)]
        assert all(np.array_equal(g.view(np.int64), w.view(np.int64)) for g, w in zip(got, want))
    p, s = Q.full_ref_native(sr, hr, 4)
    assert np.array_equal(_np(p), want[0]) and np.array_equal(_np(s), want[1])


def test_native_against_the_torch_backend_on_repaired_images(Q, repaired):
    for crop in (0, 4):
        ref = F.reference(repaired[0], repaired[1], crop)
        sr, hr = (torch.from_numpy(a).cuda() for a in repaired)
        native = [_np(t) for t in Q.full_ref_native(sr, hr, crop)]
        both = [_np(t) for t in Q.TorchFullRef(crop).cuda()(sr, hr)]
        split = [_np(Q.PSNR(crop)(sr, hr)), _np(Q.SSIM(crop)(sr, hr))]
        assert np.array_equal(both[0], split[0]) and np.array_equal(both[1], split[1])
        on_cpu = _np(Q.ssim(torch.from_numpy(repaired[0]), torch.from_numpy(repaired[1]), crop))
        print(f"crop {crop}: ssim native {native[1]} torch {both[1]}; |native - reference| / gate {np.abs(native[1] - ref['ssim']) / ref['ssim_gate']}, "
              f"|torch (device) - reference| / gate {np.abs(both[1] - ref['ssim']) / ref['ssim_gate']}, |torch (CPU) - reference| / gate "
              f"{np.abs(on_cpu - ref['ssim']) / ref['ssim_gate']}; psnr native {native[0]} torch {both[0]}")
        for got in (native, both):
            assert (np.abs(got[1] - ref["ssim"]) <= ref["ssim_gate"]).all()
            assert (np.abs(got[0] - ref["psnr"]) <= PSNR_GATE * np.maximum(1.0, np.abs(ref["psnr"]))).all()
        assert native[1][2] == 1.0 and both[1][2] == 1.0                      # image 2: sr is hr


class _Pairs:
    """What validate() needs of a prefetcher, over fixed host batches."""

    def __init__(self, batches):
        self.batches, self.at = batches, 0

    def reset(self):
        self.at = 0

    def next(self):
        self.at += 1
        return self.batches[self.at - 1] if self.at <= len(self.batches) else None

    def __len__(self):
        return len(self.batches)


class _Writer:
    def __init__(self):
        self.seen = []

    def add_scalar(self, tag, value, step):
        self.seen.append((tag, value, step))


def _tiny_model():
    from real_esrgan_pytorch_amd.compact import SRVGGNetCompact
    torch.manual_seed(0)
    return SRVGGNetCompact(num_conv=4, upscale=4, precision="fast")


def test_validate_scores_against_the_batchs_ground_truth(Q, monkeypatch, capsys):
    from real_esrgan_pytorch_amd import config
    from real_esrgan_pytorch_amd import train_realesrnet as T
    monkeypatch.setattr(config, "device", torch.device("cuda", 0))
    model = _tiny_model().to(device=config.device, memory_format=torch.channels_last)
    ema = types.SimpleNamespace(apply_shadow=lambda: None, restore=lambda: None)
    g = torch.Generator().manual_seed(1)
    batches = [{"lr": torch.rand(1, 3, 12, 13, generator=g), "hr": torch.rand(1, 3, 48, 52, generator=g)} for _ in range(2)]
    outputs = []

    def quality(sr):                                   # stands where the NIQE module stands; keeps what validate() scored
        outputs.append(sr.clone())
        return sr.double().mean()

    monkeypatch.setattr(config, "full_ref", "native")
    full_ref = config.build_full_ref()
    assert type(full_ref) is Q.NativeFullRef and full_ref.crop_border == config.upscale_factor
    writer = _Writer()
    capsys.readouterr()
    with_ref = T.validate(model, ema, _Pairs(batches), 2, writer, quality, "Test", full_ref=full_ref)
    summary = capsys.readouterr().out
    scored = [Q.full_ref_native(sr, b["hr"].cuda(), config.upscale_factor) for sr, b in zip(outputs, batches)]
    assert all(sr.shape == (1, 3, 48, 52) for sr in outputs)
    want = [sum(s[k].float() for s in scored).item() / 2 for k in (0, 1)]     # the meters accumulate in float32 on the device
    assert [t for t, _, _ in writer.seen] == ["Test/NIQE", "Test/PSNR", "Test/SSIM"] and all(step == 3 for _, _, step in writer.seen)
    assert writer.seen[1][1] == want[0] and writer.seen[2][1] == want[1]
    assert np.isfinite(want).all() and 0 < want[0] < 60 and -1 <= want[1] < 1
    assert writer.seen[0][1] == with_ref and f"PSNR {want[0]:.2f}" in summary and f"SSIM {want[1]:.2f}" in summary
    # the torch backend through the same keyword
    monkeypatch.setattr(config, "full_ref", "torch")
    torch_writer = _Writer()
    assert T.validate(model, ema, _Pairs(batches), 2, torch_writer, quality, "Test", full_ref=config.build_full_ref()) == with_ref
    assert abs(torch_writer.seen[1][1] - want[0]) < 0.05 and abs(torch_writer.seen[2][1] - want[1]) < 1e-3   # (unrepaired outputs: a near-tie level may differ)
    # without it: the scalars and the line as they were, and the same NIQE
    plain = _Writer()
    capsys.readouterr()
    assert T.validate(model, ema, _Pairs(batches), 2, plain, quality, "Test") == with_ref
    assert plain.seen == [("Test/NIQE", with_ref, 3)]
    line = capsys.readouterr().out
    assert "PSNR" not in line and "SSIM" not in line and "NIQE" in line
    monkeypatch.setattr(config, "full_ref", "off")
    assert config.build_full_ref() is None


def _folders(tmp_path, count, lr_size):
    from tests.test_gpu_train_harness import _smooth_png
    names = [f"{k}.png" for k in range(count)]
    for sub, size in (("lr", lr_size), ("gt", 4 * lr_size)):
        (tmp_path / sub).mkdir()
        for k, name in enumerate(names):
            _smooth_png(str(tmp_path / sub / name), size, 11 + k + (100 if sub == "gt" else 0))
    return names


def test_directory_evaluation_prints_the_functional_forms_values(Q, tmp_path, monkeypatch, capsys):
    from PIL import Image
    from real_esrgan_pytorch_amd import config
    from real_esrgan_pytorch_amd import test as E
    names = _folders(tmp_path, 3, 32)
    torch.save({"ema_state_dict": {"model." + k: v for k, v in _tiny_model().state_dict().items()}}, tmp_path / "g.pth.tar")
    for k, v in dict(device=torch.device("cuda", 0), g_arch="compact", compact_num_conv=4, compact_act_type="prelu", inference_precision="fast",
                     niqe_backend="native", niqe_tail="native", niqe_model_path=MODEL, full_ref="native", lr_dir=str(tmp_path / "lr"),
                     sr_dir=str(tmp_path / "sr"), hr_dir=str(tmp_path / "gt"), model_path=str(tmp_path / "g.pth.tar")).items():
        monkeypatch.setattr(config, k, v, raising=False)
    build, seen = config.build_full_ref, []

    class Recorder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.inner = build()

        def forward(self, sr, hr):
            seen.append((sr.clone(), hr.clone()))
            return self.inner(sr, hr)

    monkeypatch.setattr(config, "build_full_ref", Recorder)
    niqe = E.main()
    out = capsys.readouterr().out.splitlines()
    assert len(seen) == 3 and isinstance(niqe, float)
    for name, (sr, hr) in zip(names, seen):
        assert sr.shape == (1, 3, 128, 128) and hr.dtype == torch.uint8
        assert np.array_equal(_np(hr)[0], np.asarray(Image.open(tmp_path / "gt" / name).convert("RGB")))
    scored = [Q.full_ref_native(sr, hr, config.upscale_factor) for sr, hr in seen]
    psnr, ssim = (float(torch.stack([s[k] for s in scored]).mean()) for k in (0, 1))
    at = [i for i, l in enumerate(out) if l.startswith("NIQE: ")][0]
    assert out[at + 1:at + 3] == [f"PSNR: {psnr:4.2f} dB", f"SSIM: {ssim:4.4f}"] and np.isfinite([psnr, ssim]).all()
    # off: the NIQE line is the last one, and the same NIQE
    monkeypatch.setattr(config, "build_full_ref", build)
    monkeypatch.setattr(config, "full_ref", "off")
    again = E.main()
    out = capsys.readouterr().out.splitlines()
    assert out[-1].startswith("NIQE: ") and not any(l.startswith(("PSNR", "SSIM")) for l in out)
    assert again == niqe or (np.isnan(again) and np.isnan(niqe))
    # a missing or differently sized ground truth names the file
    with pytest.raises(FileNotFoundError, match="9.png"):
        E.read_ground_truth(str(tmp_path / "gt"), "9.png", 128, 128)
    with pytest.raises(ValueError, match=r"0\.png.* is 128x128.*132x128"):
        E.read_ground_truth(str(tmp_path / "gt"), "0.png", 132, 128)
    os.remove(tmp_path / "gt" / "1.png")
    monkeypatch.setattr(config, "full_ref", "native")
    with pytest.raises(FileNotFoundError, match="1.png"):
        E.main()


def test_inference_frames_reference_dir_prints_the_scores_of_the_written_files(Q, tmp_path, monkeypatch, capsys):
    from PIL import Image
    from real_esrgan_pytorch_amd import config, inference_frames
    monkeypatch.setattr(config, "device", torch.device("cuda", 0))
    names = _folders(tmp_path, 3, 24)
    torch.save({"params": _tiny_model().state_dict()}, tmp_path / "w.pth")

    def args(**kw):
        base = dict(inputs_dir=str(tmp_path / "lr"), output_dir=str(tmp_path / "sr"), weights_path=str(tmp_path / "w.pth"), depth=2, model_type="compact",
                    num_conv=4, act_type="prelu", precision="fast", reference_dir=str(tmp_path / "gt"))
        base.update(kw)
        return types.SimpleNamespace(**base)

    inference_frames.main(args())
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("PSNR/SSIM ")]
    want = []
    for name in names:
        sr, hr = (torch.from_numpy(np.array(Image.open(tmp_path / sub / name).convert("RGB")))[None].cuda() for sub in ("sr", "gt"))
        want.append([float(t) for t in Q.full_ref_native(sr, hr, config.upscale_factor)])
    assert np.isfinite(want).all()
    assert lines == [f"PSNR/SSIM {name}: {p:.6f} {s:.6f}" for name, (p, s) in zip(names, want)] + \
        [f"PSNR/SSIM mean: {sum(w[0] for w in want) / 3:.6f} {sum(w[1] for w in want) / 3:.6f}"]
    # without the flag nothing of it is printed
    inference_frames.main(args(reference_dir=None))
    assert "PSNR" not in capsys.readouterr().out
    # an --outscale that does not lead to the reference's size, and a missing reference, name the file
    with pytest.raises(ValueError, match=r"0\.png.* is 96x96.*48x48"):
        inference_frames.main(args(outscale=2))
    os.remove(tmp_path / "gt" / "2.png")
    with pytest.raises(FileNotFoundError, match="2.png"):
        inference_frames.main(args())
