"""GPU: the uint8 frame path (csrc/frames.hip, frames.py, inference_frames.py).  Its result is defined as the float path followed
by imgproc.tensor_to_image, so every comparison here is an equality (torch.equal / np.array_equal), never a tolerance."""
import types

import numpy as np
import pytest
import torch

from tests.frames_cases import CASES, ODD_WIDTHS, PRECISIONS, _model, float_reference, random_frames

pytestmark = pytest.mark.gpu


def _forward_u8(model, u8):
    with torch.no_grad():
        y = model.forward_u8(torch.from_numpy(u8).cuda())
    torch.cuda.synchronize()
    assert y.dtype == torch.uint8 and y.is_contiguous()
    return y.cpu().numpy()


def _check_definition(model, u8, channels_last=False):
    ref, y = float_reference(model, u8, channels_last)
    assert not torch.isnan(y).any(), "the float reference holds a NaN: equality is undefined"
    got = _forward_u8(model, u8)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bad = int((got != ref).sum())
    assert np.array_equal(got, ref), f"{bad} of {ref.size} bytes differ, first at {np.argwhere(got != ref)[:4].tolist()}"
    return ref


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-x{c[1]}-{c[2]}-n{c[3]}-{c[4][0]}x{c[4][1]}-{c[6]}")
def test_forward_u8_is_the_float_path_plus_tensor_to_image(case, precision):
    num_conv, s, act, n, (h, w), cl, init = case
    m, _ = _model(num_conv, s, act, precision, init)
    ref = _check_definition(m, random_frames(n, h, w, seed=h * w + n), cl)
    assert ref.shape == (n, h * s, w * s, 3)
    if init == "w4":      # weights x 4 drive the output far outside [0, 1]: the clamp works on both sides
        assert (ref == 0).any() and (ref == 255).any()
    flat = np.stack([np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)])      # an all-0 and an all-255 frame
    _check_definition(m, flat, cl)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("s,w", ODD_WIDTHS)
def test_output_widths_off_the_four_pixel_groups(s, w, precision):
    n, h = 3, 3
    assert (w * s) % 4 != 0 and (n * h * s * w * s) % 4 != 0
    m, _ = _model(2, s, "prelu", precision, "slopes")
    _check_definition(m, random_frames(n, h, w, seed=w * 10 + s))


def test_generic_conversions():
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import imgproc
    # fp32 -> u8: random values around and beyond [0, 1] ...
    y = (torch.rand(2, 3, 37, 53, generator=torch.Generator().manual_seed(0)) * 2 - 0.5).cuda()
    got = R.to_u8(y)
    assert got.shape == (2, 37, 53, 3) and got.dtype == torch.uint8
    ref = np.stack([imgproc.tensor_to_image(y[i:i + 1], False, False) for i in range(2)])
    assert np.array_equal(got.cpu().numpy(), ref)
    assert (ref == 0).any() and (ref == 255).any()
    # ... and the truncation edges: k / 255 and its two neighbours, for every k
    k = np.arange(256, dtype=np.float32) / np.float32(255.0)
    edges = np.concatenate([k, np.nextafter(k, np.float32(np.inf)), np.nextafter(k, np.float32(-np.inf))]).astype(np.float32)
    for shape in ((1, 3, 16, 16), (1, 3, 256, 1)):
        e = torch.from_numpy(edges.reshape(shape)).cuda()
        assert np.array_equal(R.to_u8(e)[0].cpu().numpy(), imgproc.tensor_to_image(e, False, False)), shape
    # channels_last input is normalised, not misread
    assert torch.equal(R.to_u8(y.to(memory_format=torch.channels_last)), got)
    # u8 -> fp32: numpy's division for all 256 values, in every channel
    u8 = (np.arange(3 * 256 * 2) % 256).astype(np.uint8).reshape(2, 16, 16, 3)
    x = R.from_u8(torch.from_numpy(u8).cuda())
    want = torch.from_numpy(np.ascontiguousarray((u8.astype(np.float32) / 255.0).transpose(0, 3, 1, 2)))
    assert x.dtype == torch.float32 and torch.equal(x.cpu(), want)
    # the round trip is the identity on bytes
    assert torch.equal(R.to_u8(x).cpu(), torch.from_numpy(u8))
    with pytest.raises(RuntimeError, match="uint8"):
        R.from_u8(torch.zeros(1, 4, 4, 3).cuda())
    with pytest.raises(RuntimeError, match="contiguous"):
        R.from_u8(torch.zeros(1, 4, 3, 4, dtype=torch.uint8).cuda().permute(0, 1, 3, 2))


def test_upscale_u8_rrdb_generator():
    import real_esrgan_pytorch_amd as R
    torch.manual_seed(0)
    g = R.Generator(3, 3, 4, precision="exact16", n_blocks=1)
    with torch.no_grad():
        g.conv4.bias += 0.5
    g = g.cuda().eval()
    assert not hasattr(g, "forward_u8")
    u8 = random_frames(2, 20, 24, seed=7)
    ref, y = float_reference(g, u8)
    assert not torch.isnan(y).any()
    got = R.upscale_u8(g, torch.from_numpy(u8).cuda())
    assert got.shape == (2, 80, 96, 3) and np.array_equal(got.cpu().numpy(), ref)
    assert len(np.unique(ref)) > 16


@pytest.mark.parametrize("precision", ["fast", "exact16"])
def test_upscale_u8_tiled_equals_whole_frame(precision, monkeypatch):
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import tiling
    num_conv = 4
    m, _ = _model(num_conv, 4, "prelu", precision, "slopes")
    u8 = random_frames(1, 70, 90, seed=3)
    frames = torch.from_numpy(u8).cuda()
    with torch.no_grad():
        whole = m.forward_u8(frames)
    assert torch.equal(R.upscale_u8(m, frames), whole)              # fits: the fused entry
    assert np.array_equal(whole.cpu().numpy(), float_reference(m, u8)[0])
    monkeypatch.setattr(tiling, "_MAX_OUT_PIXELS", 48 * 90)
    assert not tiling.fits_whole(m, 1, 70, 90)
    tiles, wh, ww = tiling.TiledGenerator(m, tile=None, halo=num_conv + 4, use_graph=False).plan(1, 70, 90)
    assert len(tiles) > 1 and (wh, ww) != (70, 90)
    tiled = R.upscale_u8(m, frames, halo=num_conv + 4)               # >= receptive_radius: equal to the whole frame
    assert torch.equal(tiled, whole)


def test_no_torch_fallback():
    m, _ = _model(4, 4, "prelu", "fast")
    frames = torch.from_numpy(random_frames(1, 20, 24, seed=1)).cuda()
    with torch.no_grad():
        m.forward_u8(frames)
        torch.cuda.synchronize()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            m.forward_u8(frames)
            torch.cuda.synchronize()
    names = {e.key for e in prof.key_averages()}
    banned = {"aten::conv2d", "aten::convolution", "aten::_convolution", "aten::prelu", "aten::_prelu_kernel", "aten::pixel_shuffle",
              "aten::upsample_nearest2d", "aten::add", "aten::add_", "aten::leaky_relu", "aten::relu",
              "aten::mul", "aten::clamp", "aten::permute", "aten::div", "aten::_to_copy"}
    assert not names & banned, names & banned


def test_forward_u8_argument_checks():
    import real_esrgan_pytorch_amd as R
    m, _ = _model(2, 2, "prelu", "fast")
    zeros = torch.zeros(1, 8, 8, 3, dtype=torch.uint8).cuda()
    # the guard of forward: parameters that require grad, grad mode on
    assert torch.is_grad_enabled() and any(p.requires_grad for p in m.parameters())
    with pytest.raises(RuntimeError, match="backward"):
        m.forward_u8(zeros)
    y = R.upscale_u8(m, zeros)                                 # the frame path runs it under no_grad itself
    assert y.shape == (1, 16, 16, 3) and not y.requires_grad
    with torch.no_grad():
        assert torch.equal(m.forward_u8(zeros), y)
        with pytest.raises(RuntimeError, match="uint8"):
            m.forward_u8(torch.zeros(1, 8, 8, 3).cuda())
        with pytest.raises(RuntimeError, match="uint8"):
            m.forward_u8(torch.zeros(1, 3, 8, 8, dtype=torch.uint8).cuda())
        with pytest.raises(RuntimeError, match="contiguous"):
            m.forward_u8(torch.zeros(1, 8, 3, 8, dtype=torch.uint8).cuda().permute(0, 1, 3, 2))
        with pytest.raises(RuntimeError, match="no CPU path"):
            m.forward_u8(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))


def _one_at_a_time(model, frames):
    import real_esrgan_pytorch_amd as R
    return [R.upscale_u8(model, torch.from_numpy(f)[None].cuda())[0].cpu().numpy() for f in frames]


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_frame_stream(depth):
    import real_esrgan_pytorch_amd as R
    m, _ = _model(2, 2, "prelu", "fast", "slopes")
    rs = np.random.RandomState(depth)
    frames = [rs.randint(0, 256, size=(12, 16, 3), dtype=np.uint8) for _ in range(7)]
    want = _one_at_a_time(m, frames)
    assert all(not np.array_equal(want[0], w) for w in want[1:])         # distinct contents: an order mix-up would show
    with R.FrameStream(m, depth=depth) as fs:
        got = list(fs.map(frames))
        assert len(got) == 7 and all(np.array_equal(g, w) for g, w in zip(got, want))
        # copy=True: the first result is the caller's own while the slots are reused
        it = fs.map(frames)                                              # (a second map on the same object)
        first = next(it)
        snapshot = first.copy()
        rest = list(it)
        assert np.array_equal(first, snapshot) and np.array_equal(first, want[0])
        assert all(np.array_equal(g, w) for g, w in zip(rest, want[1:]))
        assert not any(np.shares_memory(first, g) for g in rest)
        # copy=False: a view of the slot's pinned buffer, right at the moment it is handed out
        count = 0
        for i, view in enumerate(fs.map(frames, copy=False)):
            assert np.array_equal(view, want[i]), i
            count += 1
        assert count == 7
        # a change of frame size in the middle of the sequence
        mixed = frames[:3] + [rs.randint(0, 256, size=(9, 11, 3), dtype=np.uint8) for _ in range(2)] + frames[3:5]
        want_mixed = _one_at_a_time(m, mixed)
        got_mixed = list(fs.map(mixed))
        assert [g.shape for g in got_mixed] == [(24, 32, 3)] * 3 + [(18, 22, 3)] * 2 + [(24, 32, 3)] * 2
        assert all(np.array_equal(g, w) for g, w in zip(got_mixed, want_mixed))
        # submit / result by hand: oldest first, at most `depth` pending
        for f in frames[:depth]:
            fs.submit(f)
        assert len(fs) == depth
        with pytest.raises(RuntimeError, match="pending"):
            fs.submit(frames[0])
        for i in range(depth):
            assert np.array_equal(fs.result(), want[i])
        with pytest.raises(RuntimeError, match="no frame"):
            fs.result()
        with pytest.raises(ValueError, match="HxWx3 uint8"):
            fs.submit(frames[0].astype(np.float32))
    with pytest.raises(RuntimeError, match="closed"):
        fs.submit(frames[0])


def _write_pngs(d, sizes):
    from PIL import Image
    d.mkdir()
    rs = np.random.RandomState(5)
    names = []
    for i, (h, w) in enumerate(sizes):
        name = f"f{i:02d}.png"
        Image.fromarray(rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8)).save(d / name)
        names.append(name)
    return names


@pytest.mark.parametrize("model_type", ["compact", "rrdb"])
def test_directory_cli_equals_inference_per_image(model_type, tmp_path, monkeypatch):
    from PIL import Image
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import inference, inference_frames
    if model_type == "compact":
        _, sd = _model(8, 4, "prelu", "strict", "slopes")
        torch.save({"params": sd}, tmp_path / "w.pth")
        extra = dict(model_type="compact", num_conv=8, act_type="prelu", precision=None)
    else:
        monkeypatch.setattr(R.Generator, "N_BLOCKS", 1)          # a 1-block trunk keeps the entry point's model small
        torch.manual_seed(0)
        sd = {k: v.clone() for k, v in R.Generator(3, 3, 4, n_blocks=1).state_dict().items()}
        sd["conv4.bias"] += 0.5
        torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}}, tmp_path / "w.pth")
        extra = dict(model_type="rrdb", precision=None)
    names = _write_pngs(tmp_path / "lr", [(24, 30), (17, 21), (20, 26)])
    inference_frames.main(types.SimpleNamespace(inputs_dir=str(tmp_path / "lr"), output_dir=str(tmp_path / "sr"),
                                                weights_path=str(tmp_path / "w.pth"), depth=2, **extra))
    (tmp_path / "one").mkdir()
    for name in names:
        inference.main(types.SimpleNamespace(inputs_path=str(tmp_path / "lr" / name), output_path=str(tmp_path / "one" / name),
                                             weights_path=str(tmp_path / "w.pth"), **extra))
        a, b = np.asarray(Image.open(tmp_path / "sr" / name)), np.asarray(Image.open(tmp_path / "one" / name))
        assert a.shape == b.shape and a.shape[2] == 3 and np.array_equal(a, b), name
    assert sorted(p.name for p in (tmp_path / "sr").iterdir()) == names
