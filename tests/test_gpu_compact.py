"""GPU: the compact generator (SRVGGNetCompact, csrc/compact.hip) against a float64 CPU restatement of upstream's module, the
absence of torch fallbacks, tiling / hipGraph bit-equality, the autograd guard and the inference entry point (compact model and
upstream-format RRDBNet checkpoints)."""
import json
import os
import types

import numpy as np
import pytest
import torch

from tests.compact_oracle import compact_forward64

pytestmark = pytest.mark.gpu

# max |y - oracle| / max(1, max |oracle|) over the cases below: absolute at the init scale (|y| ~ 1), relative to the output's scale
# for the conv-weights-x4 cases (|y| up to ~3e4).  Measured on MI355X (diag JSON test_gpu_compact.json), worst case per mode:
# init scale strict 7.4e-8, exact16 9.8e-8, fast 2.2e-5; weights x4 strict 3.1e-6, exact16 2.3e-6, fast 2.0e-3.  Gates ~1.5x those.
GATES = {"strict": 1.2e-7, "exact16": 1.5e-7, "fast": 3.5e-5}
GATES_W4 = {"strict": 5e-6, "exact16": 3.5e-6, "fast": 3e-3}

# (num_conv, upscale, act, batch, (h, w), channels_last, init): every value of each axis at least once
CASES = [
    (16, 4, "prelu", 1, (37, 53), False, "slopes"),
    (32, 4, "prelu", 1, (128, 128), True, "default"),
    (16, 2, "leakyrelu", 3, (5, 7), False, "w4"),
    (16, 3, "relu", 1, (37, 53), True, "default"),
    (32, 3, "prelu", 3, (5, 7), False, "slopes"),
    (16, 2, "prelu", 1, (128, 128), False, "w4"),
    (32, 2, "leakyrelu", 1, (37, 53), False, "default"),
    (16, 4, "relu", 3, (5, 7), False, "w4"),
    (16, 1, "prelu", 1, (37, 53), True, "slopes"),
]


def _model(num_conv, upscale, act, precision, init="default", seed=0):
    import real_esrgan_pytorch_amd as R
    torch.manual_seed(seed)
    m = R.SRVGGNetCompact(3, 3, 64, num_conv, upscale, act, precision=precision)
    sd = m.state_dict()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, v in sd.items():
            if init == "w4" and v.dim() == 4:
                v.mul_(4)
            if init == "slopes" and v.dim() == 1 and int(k.split(".")[1]) % 2 == 1:   # PReLU slopes: negative and > 1 included
                v.copy_(torch.rand(v.shape, generator=g) * 2 - 0.5)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    return m.cuda().eval(), sd


def test_accuracy_against_float64(diag_dir):
    worst, worst_w4, rows = {p: 0.0 for p in GATES}, {p: 0.0 for p in GATES}, []
    for num_conv, s, act, n, (h, w), cl, init in CASES:
        x = torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(h * w + n))
        for precision in GATES:
            m, sd = _model(num_conv, s, act, precision, init)
            ref = compact_forward64(x, sd, num_conv, s, act)
            xi = x.cuda()
            if cl:
                xi = xi.to(memory_format=torch.channels_last)
            with torch.no_grad():
                y = m(xi)
            torch.cuda.synchronize()
            assert y.shape == (n, 3, h * s, w * s) and y.dtype == torch.float32 and y.is_contiguous()
            err = ((y.cpu().double() - ref).abs().max() / max(1.0, ref.abs().max().item())).item()
            rows.append(dict(num_conv=num_conv, upscale=s, act=act, n=n, h=h, w=w, channels_last=cl, init=init, precision=precision, err=err))
            bucket = worst_w4 if init == "w4" else worst
            bucket[precision] = max(bucket[precision], err)
    with open(os.path.join(diag_dir, "test_gpu_compact.json"), "w") as f:
        json.dump({"worst": worst, "worst_w4": worst_w4, "gates": GATES, "gates_w4": GATES_W4, "cases": rows}, f, indent=1)
    for precision in GATES:
        assert worst[precision] <= GATES[precision], (precision, worst[precision], rows)
        assert worst_w4[precision] <= GATES_W4[precision], (precision, worst_w4[precision], rows)


def test_no_torch_fallback():
    m, _ = _model(4, 4, "prelu", "fast")
    x = torch.rand(1, 3, 20, 24).cuda()
    with torch.no_grad():
        m(x)
        torch.cuda.synchronize()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            m(x)
            torch.cuda.synchronize()
    names = {e.key for e in prof.key_averages()}
    banned = {"aten::conv2d", "aten::convolution", "aten::_convolution", "aten::prelu", "aten::_prelu_kernel", "aten::pixel_shuffle",
              "aten::upsample_nearest2d", "aten::add", "aten::add_", "aten::leaky_relu", "aten::relu"}
    assert not names & banned, names & banned


def test_load_state_dict_is_seen_by_the_next_forward():
    m, sd = _model(2, 2, "prelu", "strict", "slopes")
    x = torch.rand(1, 3, 9, 11)
    with torch.no_grad():
        a = m(x.cuda()).cpu()
        sd2 = {k: v * 0.5 if v.dim() == 4 else v for k, v in sd.items()}
        m.load_state_dict(sd2)
        b = m(x.cuda()).cpu()
    assert (a.double() - compact_forward64(x, sd, 2, 2, "prelu")).abs().max() < 1e-5
    assert (b.double() - compact_forward64(x, sd2, 2, 2, "prelu")).abs().max() < 1e-5


@pytest.mark.parametrize("precision", ["fast", "exact16"])
def test_tiled_and_graph_equal_whole_frame(precision):
    from real_esrgan_pytorch_amd.tiling import TiledGenerator
    num_conv = 16
    m, _ = _model(num_conv, 4, "prelu", precision, "slopes")
    f1 = torch.rand(1, 3, 70, 90).cuda()
    f2 = torch.rand(1, 3, 70, 90).cuda()
    with torch.no_grad():
        w1, w2 = m(f1), m(f2)
        tg = TiledGenerator(m, tile=32, halo=num_conv + 2, use_graph=False)
        tiles, wh, ww = tg.plan(1, 70, 90)
        assert len(tiles) > 1 and (wh, ww) != (70, 90)
        assert torch.equal(tg(f1), w1)
        gr = TiledGenerator(m, tile=32, halo=num_conv + 2, use_graph=True)
        g1 = gr(f1)
        g2 = gr(f2)
    torch.cuda.synchronize()
    assert gr._graph is not None
    assert torch.equal(g1, w1) and torch.equal(g2, w2)


def test_autograd_guard():
    import real_esrgan_pytorch_amd as R
    m = R.SRVGGNetCompact(num_conv=2, precision="fast").cuda()
    x = torch.rand(1, 3, 8, 8).cuda()
    with pytest.raises(RuntimeError, match="backward"):
        m(x)                                                   # parameters require grad, grad mode on
    for p in m.parameters():
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match="backward"):
        m(x.clone().requires_grad_(True))
    y = m(x)                                                   # nothing requires grad: runs, no graph
    assert not y.requires_grad
    with pytest.raises(RuntimeError):
        m(x.cpu())


def _png(tmp_path, h, w):
    from PIL import Image
    lr = np.random.RandomState(0).randint(0, 256, size=(h, w, 3), dtype=np.uint8)
    Image.fromarray(lr).save(tmp_path / "lr.png")
    return lr


def test_inference_entry_point_compact(tmp_path):
    from PIL import Image
    from real_esrgan_pytorch_amd import inference
    num_conv = 8
    _, sd = _model(num_conv, 4, "prelu", "strict", "slopes")
    torch.save({"params": sd}, tmp_path / "c.pth")
    lr = _png(tmp_path, 24, 30)
    args = types.SimpleNamespace(inputs_path=str(tmp_path / "lr.png"), output_path=str(tmp_path / "sr.png"),
                                 weights_path=str(tmp_path / "c.pth"), precision=None, model_type="compact", num_conv=num_conv,
                                 act_type="prelu")
    inference.main(args)
    got = np.asarray(Image.open(tmp_path / "sr.png")).astype(np.int32)
    x = torch.from_numpy(lr.astype(np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0)
    ref = compact_forward64(x, sd, num_conv, 4, "prelu").clamp(0, 1).squeeze(0).permute(1, 2, 0).mul(255).numpy().astype("uint8")
    d = np.abs(got - ref.astype(np.int32))
    assert got.shape == (96, 120, 3) and d.max() <= 1 and (d == 0).mean() >= 0.999, (d.max(), (d == 0).mean())


def test_inference_entry_point_official_rrdb(tmp_path, monkeypatch):
    from PIL import Image
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import inference
    monkeypatch.setattr(R.Generator, "N_BLOCKS", 1)          # a 1-block trunk keeps the entry point's model small
    torch.manual_seed(0)
    sd = {k: v.clone() for k, v in R.Generator(3, 3, 4, n_blocks=1).state_dict().items()}
    sd["conv4.bias"] += 0.5
    from tests.test_compact_surface import _to_upstream
    torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}}, tmp_path / "ref.pth.tar")
    torch.save({"params_ema": {_to_upstream(k): v for k, v in sd.items()}}, tmp_path / "official.pth")
    _png(tmp_path, 20, 24)
    out = {}
    for name in ("ref.pth.tar", "official.pth"):
        args = types.SimpleNamespace(inputs_path=str(tmp_path / "lr.png"), output_path=str(tmp_path / f"{name}.png"),
                                     weights_path=str(tmp_path / name), model_type="rrdb")
        inference.main(args)
        out[name] = np.asarray(Image.open(tmp_path / f"{name}.png"))
    assert out["ref.pth.tar"].shape == (80, 96, 3)
    assert np.array_equal(out["ref.pth.tar"], out["official.pth"])
