"""GPU: the device PNG encoder (csrc/png_encode.hip) against its numpy definition (tests/png_encode_ref.py), byte for byte: every case of
tests/png_encode_cases.py, batches, a slot past byte 2^31, the overflow contract with guarded slots and unaligned outputs, the two test
entries (code construction, deflate of a given stream), graph replay, FrameStream.png and the directory CLI's --ext png."""
import ctypes as C
import io
import types
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from tests import png_encode_cases as K
from tests import png_encode_ref as P
from tests.test_png_encode_ref import code_count_cases, fibonacci

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 64


def _lib():
    import real_esrgan_pytorch_amd as R
    return R._lib


def _tensor(image):
    """numpy uint8 / uint16 -> a device tensor of the same bits."""
    if image.dtype == np.uint16:
        return torch.from_numpy(image.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(image).cuda()


def _setup(n, h, w, c, depth, segment_bytes):
    L = _lib()
    d = L.PngEncDesc(n, h, w, c, depth, segment_bytes or 0)
    host = (C.c_uint8 * L.RESR_PNG_HEADER_BYTES)()
    assert L.lib().resr_png_encode_header(C.byref(d), host, len(host)) == len(host)
    header = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).cuda()
    ws_bytes = L.lib().resr_png_encode_workspace_bytes(C.byref(d))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device="cuda")
    return d, header, ws, ws_bytes


def _raw_encode(frames, segment_bytes, stride, offset=0):
    """resr_png_encode through the C ABI into guarded memory: `offset` sentinel bytes, n slots of `stride` bytes, GUARD sentinel bytes.
    -> (the whole buffer as numpy, lengths)."""
    L = _lib()
    n, h, w, c = frames.shape
    d, header, ws, ws_bytes = _setup(n, h, w, c, 8 * frames.dtype.itemsize, segment_bytes)
    out = torch.full((offset + n * stride + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    lengths = torch.zeros(n, dtype=torch.int64, device="cuda")
    dev = _tensor(np.ascontiguousarray(frames))
    L.check(L.lib().resr_png_encode(C.byref(d), L.ptr(dev), C.c_void_p(out.data_ptr() + offset), stride, L.ptr(lengths), L.ptr(header), header.numel(),
                                    L.ptr(ws), ws_bytes, L.stream_ptr(dev)), "resr_png_encode")
    torch.cuda.synchronize()
    return out.cpu().numpy(), lengths.cpu().tolist()


def _first_difference(got: bytes, want: bytes) -> str:
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return f"lengths {len(got)} / {len(want)}, first difference at byte {k}"


@pytest.mark.parametrize("name", list(K.CASES))
def test_bytes_equal_the_definition(name):
    import real_esrgan_pytorch_amd as R
    image, segment_bytes = K.CASES[name]
    want = K.reference(name)
    got = R.png_files(_tensor(image)[None], segment_bytes)
    assert len(got) == 1 and got[0] == want, _first_difference(got[0], want)
    got = R.png_files(_tensor(image)[None], segment_bytes, capacity=len(want))          # exactly the room it needs
    assert got[0] == want


def test_batch_of_three_different_frames():
    import real_esrgan_pytorch_amd as R
    frames = np.stack([K.noise(33, 47, seed=11), K.flat(33, 47), K.gradient(33, 47)])
    want = [P.encode_png_np(f, 512) for f in frames]
    assert len({len(w) for w in want}) == 3
    buf, lengths = R.encode_png(torch.from_numpy(frames).cuda(), 512)
    assert buf.shape == (3, R.png_max_bytes(frames.shape, "uint8", 512)) and buf.dtype == torch.uint8 and lengths.dtype == torch.int64 and buf.is_cuda and lengths.is_cuda
    assert lengths.cpu().tolist() == [len(w) for w in want]
    for i, w in enumerate(want):
        assert buf[i, :len(w)].cpu().numpy().tobytes() == w, (i, _first_difference(buf[i, :len(w)].cpu().numpy().tobytes(), w))
    assert R.png_files(torch.from_numpy(frames).cuda(), 512) == want


def test_a_slot_base_past_byte_2_31():
    L = _lib()
    frames = np.stack([K.gradient(16, 24), K.noise(16, 24, seed=3), K.speckled(16, 24)])
    want = [P.encode_png_np(f, 256) for f in frames]
    stride = (1 << 30) + 37          # slot 2 starts past byte 2^31, at an odd address
    d, header, ws, ws_bytes = _setup(3, 16, 24, 3, 8, 256)
    out = torch.empty(2 * stride + 4096, dtype=torch.uint8, device="cuda")          # (only the used part of the last slot exists)
    lengths = torch.zeros(3, dtype=torch.int64, device="cuda")
    dev = torch.from_numpy(frames).cuda()
    L.check(L.lib().resr_png_encode(C.byref(d), L.ptr(dev), L.ptr(out), stride, L.ptr(lengths), L.ptr(header), header.numel(), L.ptr(ws), ws_bytes,
                                    L.stream_ptr(dev)), "resr_png_encode")
    torch.cuda.synchronize()
    assert lengths.cpu().tolist() == [len(w) for w in want] and max(len(w) for w in want) <= 4096
    for i, w in enumerate(want):
        assert out[i * stride:i * stride + len(w)].cpu().numpy().tobytes() == w, i


@pytest.mark.parametrize("offset", [0, 1, 3])
def test_overflow_leaves_the_slot_and_every_guard_alone(offset):
    frames = np.stack([K.gradient(24, 40), K.noise(24, 40, seed=5), K.flat(24, 40)])
    want = [P.encode_png_np(f, 300) for f in frames]
    need = len(want[1])
    assert need > max(len(want[0]), len(want[2]))

    def slots(buf, stride):
        assert (buf[:offset] == SENTINEL).all() and (buf[offset + 3 * stride:] == SENTINEL).all(), "a guard outside the slots was written"
        return [buf[offset + i * stride:offset + (i + 1) * stride] for i in range(3)]
    # one byte short for the middle frame (the outputs start at `offset`, unaligned for 1 and 3)
    buf, lengths = _raw_encode(frames, 300, need - 1, offset)
    assert lengths == [len(want[0]), -need, len(want[2])]
    for i, slot in enumerate(slots(buf, need - 1)):
        if i == 1:
            assert (slot == SENTINEL).all(), "the slot of the frame that did not fit was written"
        else:
            assert slot[:len(want[i])].tobytes() == want[i] and (slot[len(want[i]):] == SENTINEL).all(), i
    # exactly the needed size: it fits
    buf, lengths = _raw_encode(frames, 300, need, offset)
    assert lengths == [len(w) for w in want]
    for i, slot in enumerate(slots(buf, need)):
        assert slot[:len(want[i])].tobytes() == want[i] and (slot[len(want[i]):] == SENTINEL).all(), i
    # no room at all: every length is the negative of the need, nothing is written
    buf, lengths = _raw_encode(frames, 300, 0, offset)
    assert lengths == [-len(w) for w in want] and (buf == SENTINEL).all()


def test_png_files_names_the_size_an_overflow_needs():
    import real_esrgan_pytorch_amd as R
    image = K.noise(24, 40, seed=5)
    need = len(P.encode_png_np(image))
    assert need > 24 * 40 * 3          # noise does not fit the raw frame's bytes
    with pytest.raises(RuntimeError, match=str(need)):
        R.png_files(torch.from_numpy(image)[None].cuda(), capacity=24 * 40 * 3)
    assert len(R.png_files(torch.from_numpy(image)[None].cuda())[0]) == need <= R.png_max_bytes((1, 24, 40, 3))


# ---- the test entries ----
@pytest.mark.parametrize("name", list(code_count_cases()))
def test_build_code_equals_numpy_element_by_element(name):
    L = _lib()
    counts, limit = code_count_cases()[name]
    want = P.build_lengths(counts, limit)
    dev = torch.from_numpy(np.asarray(counts, dtype=np.int64).astype(np.uint32).view(np.int32)).cuda()
    out = torch.full((len(counts),), 99, dtype=torch.uint8, device="cuda")
    L.check(L.lib().resr_png_debug_build_code(L.ptr(dev), len(counts), limit, L.ptr(out), L.stream_ptr(dev)), "resr_png_debug_build_code")
    got = out.cpu().tolist()
    assert got == want, [(s, g, w) for s, (g, w) in enumerate(zip(got, want)) if g != w][:8]
    used = [l for l in got if l]
    assert len(used) <= 1 and used in ([], [1]) or sum(1 << (limit - l) for l in used) == 1 << limit          # Kraft: exactly 1


def _deflate(stream, segment_bytes, capacity=None):
    L = _lib()
    dev = torch.from_numpy(stream).cuda()
    ws_bytes = L.lib().resr_png_debug_deflate_workspace_bytes(len(stream), segment_bytes)
    assert ws_bytes > 0
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device="cuda")
    capacity = len(stream) + 5 * (len(stream) // segment_bytes + 1) + 6 if capacity is None else capacity
    out = torch.full((capacity + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    length = torch.zeros(1, dtype=torch.int64, device="cuda")
    L.check(L.lib().resr_png_debug_deflate(L.ptr(dev), len(stream), segment_bytes, L.ptr(out), capacity, L.ptr(length), L.ptr(ws), ws_bytes, L.stream_ptr(dev)),
            "resr_png_debug_deflate")
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(length.item())


@pytest.mark.parametrize("name", list(K.STREAM_CASES))
def test_deflate_of_a_given_stream(name):
    stream, segment_bytes = K.STREAM_CASES[name]
    want = K.stream_reference(name)
    out, length = _deflate(stream, segment_bytes)
    got = out[:max(length, 0)].tobytes()
    assert length == len(want) and got == want, _first_difference(got, want)
    assert zlib.decompress(got) == stream.tobytes() and (out[length:] == SENTINEL).all()
    out, length = _deflate(stream, segment_bytes, len(want) - 1)
    assert length == -len(want) and (out == SENTINEL).all()


def test_deflate_of_a_fibonacci_histogram_in_one_segment():
    """Byte value i occurs F(i + 1) times, i < 22 (46,367 bytes, shuffled so that runs are rare): the unlimited literal code would be 21
    bits deep, the block must hold it to 15."""
    counts = fibonacci(22)
    stream = np.repeat(np.arange(22, dtype=np.uint8), counts)
    np.random.default_rng(8).shuffle(stream)
    assert len(stream) == 46367 and max(P.huffman_depths(sorted(counts))) > 15
    want = P.zlib_stream_np(stream, 65535)
    out, length = _deflate(stream, 65535)
    got = out[:max(length, 0)].tobytes()
    assert zlib.decompress(got) == stream.tobytes()
    assert got == want, _first_difference(got, want)


# ---- integration ----
def test_a_captured_graph_replays_to_the_same_bytes():
    L = _lib()
    first, second = K.gradient(40, 56, seed=2), K.noise(40, 56, seed=4)
    d, header, ws, ws_bytes = _setup(1, 40, 56, 3, 8, 1024)
    stride = P.max_bytes_np(40, 56, 3, 8, 1024)
    out = torch.zeros(stride, dtype=torch.uint8, device="cuda")
    lengths = torch.zeros(1, dtype=torch.int64, device="cuda")
    dev = torch.from_numpy(first)[None].cuda()

    def enqueue():
        L.check(L.lib().resr_png_encode(C.byref(d), L.ptr(dev), L.ptr(out), stride, L.ptr(lengths), L.ptr(header), header.numel(), L.ptr(ws), ws_bytes,
                                        L.stream_ptr(dev)), "resr_png_encode")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enqueue()          # once outside the capture: modules loaded, nothing left to initialise
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue()
    for image in (first, second, first):
        dev.copy_(torch.from_numpy(image)[None])
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want = P.encode_png_np(image, 1024)
        assert lengths.item() == len(want) and out[:len(want)].cpu().numpy().tobytes() == want


def _small_model():
    from tests.frames_cases import _model
    return _model(2, 2, "prelu", "fast", "slopes")[0]


def test_frame_stream_returns_the_files():
    import real_esrgan_pytorch_amd as R
    m = _small_model()
    shapes = ((24, 32), (24, 32), (20, 24), (24, 32))
    frames = [K.speckled(h, w, seed=i) for i, (h, w) in enumerate(shapes)]          # image-like: the files are far below the raw frames
    raw = [R.upscale_u8(m, torch.from_numpy(f)[None].cuda())[0].cpu().numpy() for f in frames]
    want = R.png_files(torch.stack([torch.from_numpy(r) for r in raw[:2]]).cuda()) + [R.png_files(torch.from_numpy(r)[None].cuda())[0] for r in raw[2:]]
    assert all(np.array_equal(np.asarray(Image.open(io.BytesIO(w))), r) for w, r in zip(want, raw))
    seen = []
    with R.FrameStream(m, depth=2) as fs:
        fs.png = dict()
        assert fs.png == dict(segment_bytes=None)
        fs.on_device = lambda frame: seen.append(tuple(frame.shape))          # still the raw frame
        got = list(fs.map(frames))
        assert all(g.ndim == 1 and g.dtype == np.uint8 for g in got)
        assert [g.tobytes() for g in got] == want and fs.png_fallbacks == 0
        assert seen == [(1,) + r.shape for r in raw]
        assert [g.tobytes() for g in fs.map(frames, copy=False)] == want
        # a noise frame's file is larger than the raw frame's pinned slot, a tiny capacity is below every file: the device writes
        # nothing, the frame comes down raw and Pillow encodes it
        noisy = [K.noise(24, 32, seed=7)]
        fs.png = None
        noisy_raw = list(fs.map(noisy))[0]
        fs.png = dict(segment_bytes=4096)
        fs.png_capacity = 100
        got = list(fs.map(frames[:3] + noisy))
        assert fs.png_fallbacks == 4
        for g, r in zip(got, raw[:3] + [noisy_raw]):
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(g.tobytes()))), r)
        fs.png_capacity = None
        assert [g.tobytes() for g in fs.map(frames)] == [R.png_files(torch.from_numpy(r)[None].cuda(), 4096)[0] for r in raw] and fs.png_fallbacks == 4
        fs.png = None          # switched off again on the same stream: raw frames
        assert all(np.array_equal(g, r) for g, r in zip(fs.map(frames), raw))


def _write_mixed(folder):
    """Tiny RGB, L, RGBA and I;16 files -> their names."""
    folder.mkdir()
    rs = np.random.RandomState(3)
    Image.fromarray(rs.randint(0, 256, (20, 26, 3), dtype=np.uint8)).save(folder / "a_rgb.png")
    Image.fromarray(K.speckled(17, 21, seed=2)).save(folder / "b_rgb.png")
    Image.fromarray(rs.randint(0, 256, (18, 22), dtype=np.uint8), "L").save(folder / "c_grey.png")
    Image.fromarray(rs.randint(0, 256, (16, 20, 4), dtype=np.uint8), "RGBA").save(folder / "d_rgba.png")
    Image.fromarray(rs.randint(0, 65536, (18, 18)).astype(np.uint16)).save(folder / "e_deep.png")
    return sorted(p.name for p in folder.iterdir())


def test_directory_cli_ext_png(tmp_path):
    from real_esrgan_pytorch_amd import inference_frames
    from tests.frames_cases import _model
    _, sd = _model(8, 4, "prelu", "strict", "slopes")
    torch.save({"params": sd}, tmp_path / "w.pth")
    names = _write_mixed(tmp_path / "lr")
    assert Image.open(tmp_path / "lr" / "e_deep.png").mode == "I;16"
    common = dict(inputs_dir=str(tmp_path / "lr"), weights_path=str(tmp_path / "w.pth"), depth=2, model_type="compact", num_conv=8, act_type="prelu", precision=None)
    for keep in (False, True):
        tag = "keep" if keep else "rgb"
        inference_frames.main(types.SimpleNamespace(output_dir=str(tmp_path / f"png_{tag}"), ext="png", keep_mode=keep, decode_workers=2, **common))
        inference_frames.main(types.SimpleNamespace(output_dir=str(tmp_path / f"same_{tag}"), keep_mode=keep, **common))
        assert sorted(p.name for p in (tmp_path / f"png_{tag}").iterdir()) == names == sorted(p.name for p in (tmp_path / f"same_{tag}").iterdir())
        for name in names:
            ours, theirs = Image.open(tmp_path / f"png_{tag}" / name), Image.open(tmp_path / f"same_{tag}" / name)
            assert ours.mode == theirs.mode and ours.size == theirs.size, (name, ours.mode, theirs.mode)
            assert np.array_equal(np.asarray(ours), np.asarray(theirs)), name
            Image.open(tmp_path / f"png_{tag}" / name).verify()
    assert {Image.open(tmp_path / "png_keep" / n).mode for n in names} == {"RGB", "L", "RGBA", "I;16"}
