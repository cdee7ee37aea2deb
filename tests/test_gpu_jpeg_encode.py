"""GPU: the device JPEG encoder (csrc/jpeg_encode.hip) against its numpy definition (tests/jpeg_encode_ref.py), byte for byte: every
case of tests/jpeg_encode_cases.py, batches, the overflow contract with guarded slots, unaligned outputs, graph replay, FrameStream.jpeg
and the directory CLI's --ext jpg."""
import ctypes as C
import io
import types

import numpy as np
import pytest
import torch
from PIL import Image

from tests import jpeg_encode_cases as K
from tests import jpeg_encode_ref as J

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 64


def _lib():
    import real_esrgan_pytorch_amd as R
    return R._lib


def _raw_encode(frames, quality, sub, interval, stride, offset=0):
    """resr_jpeg_encode through the C ABI into guarded memory: `offset` sentinel bytes, n slots of `stride` bytes, GUARD sentinel bytes.
    -> (the whole buffer as numpy, lengths)."""
    L = _lib()
    n, h, w = frames.shape[:3]
    d = L.JpegEncDesc(n, h, w, {"444": L.RESR_JPEG_444, "420": L.RESR_JPEG_420}[sub], quality, interval or 0)
    host = (C.c_uint8 * L.RESR_JPEG_HEADER_BYTES)()
    assert L.lib().resr_jpeg_encode_header(C.byref(d), host, len(host)) == len(host)
    header = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).cuda()
    ws_bytes = L.lib().resr_jpeg_encode_workspace_bytes(C.byref(d))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device="cuda")
    out = torch.full((offset + n * stride + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    lengths = torch.zeros(n, dtype=torch.int64, device="cuda")
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    L.check(L.lib().resr_jpeg_encode(C.byref(d), L.ptr(dev), C.c_void_p(out.data_ptr() + offset), stride, L.ptr(lengths), L.ptr(header), len(host),
                                     L.ptr(ws), ws_bytes, L.stream_ptr(dev)), "resr_jpeg_encode")
    torch.cuda.synchronize()
    return out.cpu().numpy(), lengths.cpu().tolist()


def _first_difference(got: bytes, want: bytes) -> str:
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return f"lengths {len(got)} / {len(want)}, first difference at byte {k}"


@pytest.mark.parametrize("name", list(K.CASES))
def test_bytes_equal_the_definition(name):
    import real_esrgan_pytorch_amd as R
    image, quality, sub, interval = K.CASES[name]
    want = K.reference(name)
    got = R.jpeg_files(torch.from_numpy(image)[None].cuda(), quality, sub, interval, capacity=len(want) + 7)
    assert len(got) == 1 and got[0] == want, _first_difference(got[0], want)


@pytest.mark.parametrize("sub", J.SUBSAMPLINGS)
def test_batch_of_three_different_frames(sub):
    import real_esrgan_pytorch_amd as R
    frames = np.stack([K.noise(33, 47, 11), K.flat(33, 47), K.gradient(33, 47)])
    want = [J.encode_jpeg_np(f, 90, sub) for f in frames]
    assert len({len(w) for w in want}) == 3
    buf, lengths = R.encode_jpeg(torch.from_numpy(frames).cuda(), 90, sub)
    assert buf.shape == (3, 33 * 47 * 3) and buf.dtype == torch.uint8 and lengths.dtype == torch.int64 and buf.is_cuda and lengths.is_cuda
    assert lengths.cpu().tolist() == [len(w) for w in want]
    for i, w in enumerate(want):
        assert buf[i, :len(w)].cpu().numpy().tobytes() == w, (i, _first_difference(buf[i, :len(w)].cpu().numpy().tobytes(), w))
    assert R.jpeg_files(torch.from_numpy(frames).cuda(), 90, sub) == want


@pytest.mark.parametrize("sub,offset", [("444", 0), ("420", 1), ("444", 3)])
def test_overflow_leaves_the_slot_and_every_guard_alone(sub, offset):
    frames = np.stack([K.gradient(24, 40), K.noise(24, 40, 5), K.flat(24, 40)])
    want = [J.encode_jpeg_np(f, 95, sub) for f in frames]
    need = len(want[1])
    assert need > max(len(want[0]), len(want[2]))

    def slots(buf, stride):
        assert (buf[:offset] == SENTINEL).all() and (buf[offset + 3 * stride:] == SENTINEL).all(), "a guard outside the slots was written"
        return [buf[offset + i * stride:offset + (i + 1) * stride] for i in range(3)]
    # one byte short for the middle frame (an odd or even stride as it comes; the outputs start at `offset`, unaligned for 1 and 3)
    buf, lengths = _raw_encode(frames, 95, sub, None, need - 1, offset)
    assert lengths == [len(want[0]), -need, len(want[2])]
    for i, slot in enumerate(slots(buf, need - 1)):
        if i == 1:
            assert (slot == SENTINEL).all(), "the slot of the frame that did not fit was written"
        else:
            assert slot[:len(want[i])].tobytes() == want[i] and (slot[len(want[i]):] == SENTINEL).all(), i
    # exactly the needed size: it fits
    buf, lengths = _raw_encode(frames, 95, sub, None, need, offset)
    assert lengths == [len(w) for w in want]
    for i, slot in enumerate(slots(buf, need)):
        assert slot[:len(want[i])].tobytes() == want[i] and (slot[len(want[i]):] == SENTINEL).all(), i
    # no room at all: every length is the negative of the need, nothing is written
    buf, lengths = _raw_encode(frames, 95, sub, None, 0, offset)
    assert lengths == [-len(w) for w in want] and (buf == SENTINEL).all()


def test_jpeg_files_names_the_size_an_overflow_needs():
    import real_esrgan_pytorch_amd as R
    image = K.noise(24, 40, 5)
    need = len(J.encode_jpeg_np(image, 100, "444"))
    assert need > 24 * 40 * 3          # noise at quality 100 does not fit the default capacity, the raw frame
    with pytest.raises(RuntimeError, match=str(need)):
        R.jpeg_files(torch.from_numpy(image)[None].cuda(), 100, "444")
    assert len(R.jpeg_files(torch.from_numpy(image)[None].cuda(), 100, "444", capacity=R.jpeg_encode.jpeg_max_bytes((1, 24, 40), 100, "444"))[0]) == need


def test_a_captured_graph_replays_to_the_same_bytes():
    L = _lib()
    first, second = K.gradient(40, 56, 2), K.noise(40, 56, 4)
    d = L.JpegEncDesc(1, 40, 56, L.RESR_JPEG_420, 90, 0)
    host = (C.c_uint8 * L.RESR_JPEG_HEADER_BYTES)()
    assert L.lib().resr_jpeg_encode_header(C.byref(d), host, len(host)) == len(host)
    header = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).cuda()
    ws_bytes = L.lib().resr_jpeg_encode_workspace_bytes(C.byref(d))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device="cuda")
    stride = 40 * 56 * 3
    out = torch.zeros(stride, dtype=torch.uint8, device="cuda")
    lengths = torch.zeros(1, dtype=torch.int64, device="cuda")
    dev = torch.from_numpy(first)[None].cuda()

    def enqueue():
        L.check(L.lib().resr_jpeg_encode(C.byref(d), L.ptr(dev), L.ptr(out), stride, L.ptr(lengths), L.ptr(header), len(host), L.ptr(ws), ws_bytes,
                                         L.stream_ptr(dev)), "resr_jpeg_encode")
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
        want = J.encode_jpeg_np(image, 90, "420")
        assert lengths.item() == len(want) and out[:len(want)].cpu().numpy().tobytes() == want


def _small_model():
    from tests.frames_cases import _model
    return _model(2, 2, "prelu", "fast", "slopes")[0]


def test_frame_stream_returns_the_files():
    import real_esrgan_pytorch_amd as R
    m = _small_model()
    rs = np.random.RandomState(2)
    frames = [rs.randint(0, 256, size=s + (3,), dtype=np.uint8) for s in ((24, 32), (24, 32), (20, 24), (24, 32))]
    raw = [R.upscale_u8(m, torch.from_numpy(f)[None].cuda())[0].cpu().numpy() for f in frames]
    want = [J.encode_jpeg_np(r, 90, "444") for r in raw]
    assert all(len(w) <= r.size for w, r in zip(want, raw))          # (frames large enough that the 613-byte header does not outweigh the raw frame)
    seen = []
    with R.FrameStream(m, depth=2) as fs:
        fs.jpeg = dict(quality=90, subsampling="444")
        fs.on_device = lambda frame: seen.append(tuple(frame.shape))          # still the raw frame
        got = list(fs.map(frames))
        assert all(g.ndim == 1 and g.dtype == np.uint8 for g in got)
        assert [g.tobytes() for g in got] == want and fs.jpeg_fallbacks == 0
        assert seen == [(1,) + r.shape for r in raw]
        assert [g.tobytes() for g in fs.map(frames, copy=False)] == want
        # a capacity below the files: the device writes nothing, the frame comes down raw and Pillow encodes it
        fs.jpeg_capacity = 620          # (the header alone is 613 bytes)
        assert min(len(w) for w in want) > 620
        got = list(fs.map(frames[:3]))
        assert fs.jpeg_fallbacks == 3
        for g, r in zip(got, raw):
            out = io.BytesIO()
            Image.fromarray(r).save(out, "JPEG", quality=90, subsampling=0)
            assert g.tobytes() == out.getvalue()
        fs.jpeg_capacity = None
        assert [g.tobytes() for g in fs.map(frames)] == want and fs.jpeg_fallbacks == 3
        # switched off and on again on the same stream: raw frames, then the defaults (quality 95, 4:2:0)
        fs.jpeg = None
        assert all(np.array_equal(g, r) for g, r in zip(fs.map(frames), raw))
    with R.FrameStream(m, depth=1) as fs:
        fs.jpeg = {}
        assert [g.tobytes() for g in fs.map(frames[:2])] == [J.encode_jpeg_np(r, 95, "420") for r in raw[:2]]


def test_directory_cli_ext_jpg(tmp_path):
    from real_esrgan_pytorch_amd import inference_frames
    from tests.frames_cases import _model
    from tests.test_gpu_frames import _write_pngs
    _, sd = _model(8, 4, "prelu", "strict", "slopes")
    torch.save({"params": sd}, tmp_path / "w.pth")
    names = _write_pngs(tmp_path / "lr", [(24, 30), (17, 21), (20, 26)])
    common = dict(inputs_dir=str(tmp_path / "lr"), weights_path=str(tmp_path / "w.pth"), depth=2, model_type="compact", num_conv=8, act_type="prelu", precision=None)
    inference_frames.main(types.SimpleNamespace(output_dir=str(tmp_path / "jpg"), ext="jpg", jpeg_quality=92, jpeg_subsampling="420", decode_workers=2, **common))
    inference_frames.main(types.SimpleNamespace(output_dir=str(tmp_path / "png"), **common))
    assert sorted(p.name for p in (tmp_path / "jpg").iterdir()) == [n[:-4] + ".jpg" for n in names]
    for name in names:
        raw = np.asarray(Image.open(tmp_path / "png" / name))
        data = (tmp_path / "jpg" / (name[:-4] + ".jpg")).read_bytes()
        assert data == J.encode_jpeg_np(raw, 92, "420")          # the file is the definition's, of the frame the PNG path writes
        with Image.open(io.BytesIO(data)) as image:
            image.load()
            assert image.size == (raw.shape[1], raw.shape[0]) and image.mode == "RGB"
