"""The JPEG encoder's surface without a device: the C entries (declared once, exported, every refusal before a launch, the host-side
header and the size bounds, on the cross-compiled library), the Python layer's ValueErrors, FrameStream.jpeg's checks
and the directory CLI's `--ext` / `--decode_workers` with a stub stream."""
import ctypes as C
import io
import os
import re
import types

import numpy as np
import pytest
import torch
from PIL import Image

import real_esrgan_pytorch_amd as R
from real_esrgan_pytorch_amd import _lib, inference_frames, jpeg_encode
from tests import jpeg_encode_cases as K
from tests import jpeg_encode_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("resr_jpeg_encode_max_bytes", "resr_jpeg_encode_workspace_bytes", "resr_jpeg_encode_header", "resr_jpeg_encode")
SUB = {"444": _lib.RESR_JPEG_444, "420": _lib.RESR_JPEG_420}


def _desc(n=1, h=16, w=16, sub="420", quality=75, interval=0):
    return _lib.JpegEncDesc(n, h, w, SUB.get(sub, sub), quality, interval)


def _header(d) -> bytes:
    buf = (C.c_uint8 * 1024)()
    got = _lib.lib().resr_jpeg_encode_header(C.byref(d), buf, len(buf))
    assert got > 0, _lib.lib().resr_last_error()
    return bytes(buf[:got])


def test_entries_are_declared_once_and_exported():
    with open(os.path.join(ROOT, "include", "resr.h")) as f:
        header = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)          # the declarations, without the comments that speak of them
    for name in ENTRIES:
        assert len(re.findall(rf"\b{name}\s*\(", header)) == 1, name
        assert callable(getattr(_lib.lib(), name)) and name in _lib.exported_symbols()
    assert [f[0] for f in _lib.JpegEncDesc._fields_] == ["n", "h", "w", "subsampling", "quality", "restart_interval"]
    assert _lib.RESR_JPEG_DEFAULT_INTERVAL == J.DEFAULT_RESTART_INTERVAL and (_lib.RESR_JPEG_444, _lib.RESR_JPEG_420) == (0, 1)
    for name in ("jpeg_encode", "encode_jpeg", "jpeg_files"):
        assert hasattr(R, name) and name in R.__all__, name
    assert R.encode_jpeg is jpeg_encode.encode_jpeg and set(jpeg_encode.JPEG_SUBSAMPLINGS) == set(J.SUBSAMPLINGS)


BAD_DESCS = [(dict(n=0), "geometry"), (dict(h=0), "geometry"), (dict(w=0), "geometry"), (dict(h=65536), "geometry"), (dict(w=65536), "geometry"),
             (dict(quality=0), "quality"), (dict(quality=101), "quality"), (dict(sub=2), "subsampling"), (dict(sub=-1), "subsampling"),
             (dict(interval=-1), "interval"), (dict(interval=65536), "interval")]


def test_every_refusal_comes_before_a_launch():
    """No device here: an entry that got as far as a launch would fail with RESR_ERR_LAUNCH or crash on the made-up pointers."""
    lib = _lib.lib()
    fake = C.c_void_p(0x10000)          # never dereferenced: every call below is refused first

    def encode(d, rgb=fake, out=fake, stride=1 << 20, lengths=fake, header=fake, header_len=_lib.RESR_JPEG_HEADER_BYTES, ws=fake, ws_bytes=1 << 40):
        return lib.resr_jpeg_encode(C.byref(d) if d is not None else None, rgb, out, stride, lengths, header, header_len, ws, ws_bytes, None)

    def refused(rc, word):
        assert rc == _lib.RESR_ERR_ARG, rc
        text = lib.resr_last_error().decode()
        assert "jpeg_encode" in text and word in text, text

    for kw, word in BAD_DESCS:
        d = _desc(**kw)
        refused(encode(d), word)
        assert lib.resr_jpeg_encode_max_bytes(C.byref(d)) == 0 and lib.resr_jpeg_encode_workspace_bytes(C.byref(d)) == 0
        refused(lib.resr_jpeg_encode_header(C.byref(d), (C.c_uint8 * 1024)(), 1024), word)
    refused(encode(None), "null descriptor")
    assert lib.resr_jpeg_encode_max_bytes(None) == 0 and lib.resr_jpeg_encode_workspace_bytes(None) == 0
    d = _desc()
    for which in ("rgb", "out", "lengths", "header", "ws"):
        refused(encode(d, **{which: None}), "null pointer")
    refused(encode(d, header_len=_lib.RESR_JPEG_HEADER_BYTES - 1), "header")
    refused(encode(d, header_len=0), "header")
    refused(encode(d, stride=-1), "out_stride")
    need = lib.resr_jpeg_encode_workspace_bytes(C.byref(d))
    assert need > 0
    refused(encode(d, ws_bytes=need - 1), "workspace")
    refused(encode(d, ws=C.c_void_p(0x10004)), "aligned")
    refused(encode(d, lengths=C.c_void_p(0x10004)), "aligned")
    refused(lib.resr_jpeg_encode_header(C.byref(d), (C.c_uint8 * 100)(), 100), "needed")
    assert lib.resr_jpeg_encode_header(C.byref(d), None, 0) == _lib.RESR_JPEG_HEADER_BYTES          # the length alone


@pytest.mark.parametrize("h,w,sub,quality,interval", [(16, 16, "420", 75, 0), (30, 38, "444", 95, 0), (1, 1, "444", 1, 1), (65535, 65535, "420", 100, 65535),
                                                      (47, 33, "420", 50, 5), (9, 17, "444", 10, 3)])
def test_header_is_the_definitions(h, w, sub, quality, interval):
    got = _header(_desc(1, h, w, sub, quality, interval))
    want = J.header_np(h, w, quality, sub, interval or J.DEFAULT_RESTART_INTERVAL)
    assert len(got) == _lib.RESR_JPEG_HEADER_BYTES == len(want) and got == want
    if h * w < 4096:
        image = K.noise(h, w)
        assert J.encode_jpeg_np(image, quality, sub, interval or None)[:len(got)] == got


@pytest.mark.parametrize("h,w,interval", [(8, 8, 0), (33, 47, 0), (24, 40, 1), (16, 72, 5), (17, 9, 65535)])
def test_max_bytes_covers_the_worst_file_the_definition_makes(h, w, interval):
    """Quality 100, uniform noise, 4:4:4: the longest codes there are.  The bound is derived from the code lengths (include/resr.h), so
    it is far above even this file -- and it must be."""
    for sub in J.SUBSAMPLINGS:
        worst = max(len(J.encode_jpeg_np(K.noise(h, w, seed), 100, sub, interval or None)) for seed in range(3))
        d = _desc(1, h, w, sub, 100, interval)
        bound = _lib.lib().resr_jpeg_encode_max_bytes(C.byref(d))
        assert bound >= worst, (sub, bound, worst)
        # the derivation, restated: header + segments * (round16(2 * ceil(1660 * blocks / 8)) + 2)
        mcu, blocks = (16, 6) if sub == "420" else (8, 3)
        mcus = -(-h // mcu) * -(-w // mcu)
        per = interval or J.DEFAULT_RESTART_INTERVAL
        seg = -(-2 * -(-1660 * min(per, mcus) * blocks // 8) // 16) * 16
        assert bound == _lib.RESR_JPEG_HEADER_BYTES + -(-mcus // per) * (seg + 2)
        assert _lib.lib().resr_jpeg_encode_workspace_bytes(C.byref(d)) >= -(-mcus // per) * (seg + 12)
    assert jpeg_encode.jpeg_max_bytes((1, h, w), 100, "444", interval or None) == _lib.lib().resr_jpeg_encode_max_bytes(C.byref(_desc(1, h, w, "444", 100, interval)))


def test_value_errors_of_the_python_layer_come_before_the_device():
    frames = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)          # on the CPU: any look at the device raises RuntimeError
    for kw, word in ((dict(quality=0), "quality"), (dict(quality=101), "quality"), (dict(quality=75.0), "quality"), (dict(quality=True), "quality"),
                     (dict(subsampling="422"), "subsampling"), (dict(subsampling=420), "subsampling"), (dict(restart_interval=0), "restart_interval"),
                     (dict(restart_interval=65536), "restart_interval"), (dict(restart_interval=-1), "restart_interval"), (dict(capacity=0), "capacity"),
                     (dict(capacity=1.5), "capacity")):
        for call in (R.encode_jpeg, R.jpeg_files):
            with pytest.raises(ValueError, match=word):
                call(frames, **kw)
    for bad in (torch.zeros(8, 8, 3, dtype=torch.uint8), torch.zeros(1, 8, 8, 4, dtype=torch.uint8), torch.zeros(1, 8, 8, 3), torch.zeros(0, 8, 8, 3, dtype=torch.uint8),
                torch.zeros(1, 3, 65536, 3, dtype=torch.uint8), np.zeros((1, 8, 8, 3), dtype=np.uint8)):
        with pytest.raises(ValueError, match="N,H,W,3|1..65535"):
            R.encode_jpeg(bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.encode_jpeg(frames)


class _FakeParam:
    is_cuda, device = True, torch.device("cuda", 0)


class _FakeModel:
    upscale_factor = 2

    def parameters(self):
        return iter([_FakeParam()])


def test_frame_stream_jpeg_argument_checks():
    """`jpeg` is an attribute of the stream (like `on_device`): the constructor's parameter list stays what it was."""
    import inspect
    assert "jpeg" not in inspect.signature(R.FrameStream.__init__).parameters and isinstance(R.FrameStream.jpeg, property)
    for kw in (dict(pix_fmt="nv12"), dict(pix_fmt="i420"), dict(pix_fmt="p010"), dict(out_pix_fmt="nv12"), dict(pix_fmt="nv12", out_pix_fmt="rgb24"),
               dict(out_pix_fmt="i420p10")):
        fs = R.FrameStream(_FakeModel(), 2, **kw)
        with pytest.raises(ValueError, match="rgb24"):
            fs.jpeg = dict(quality=90)
        assert fs.jpeg is None
        fs.jpeg = None          # (switching it off is always allowed)
    fs = R.FrameStream(_FakeModel(), 2)
    assert fs.jpeg is None and fs.jpeg_fallbacks == 0 and fs.jpeg_capacity is None
    for bad, word in ((dict(quality=0), "quality"), (dict(quality=101), "quality"), (dict(subsampling="411"), "subsampling"), (dict(restart_interval=0), "restart_interval"),
                      (dict(restart_interval=65536), "restart_interval"), (dict(qualty=90), "keys"), ("420", "dict")):
        with pytest.raises(ValueError, match=word):
            fs.jpeg = bad
        assert fs.jpeg is None
    fs.jpeg = {}
    assert fs.jpeg == dict(quality=95, subsampling="420", restart_interval=None)
    fs.jpeg = dict(quality=80, subsampling="444", restart_interval=4)
    assert fs.jpeg == dict(quality=80, subsampling="444", restart_interval=4)
    fs._ready.append(np.zeros(1, dtype=np.uint8))          # a result not yet taken: it was made under the old setting
    with pytest.raises(RuntimeError, match="outstanding"):
        fs.jpeg = None
    fs._ready.clear()
    fs.jpeg = None
    assert fs.jpeg is None
    # the slots keep the raw frame's layout, with or without jpeg; the formats are what they were
    plain = R.FrameStream(_FakeModel(), 2)
    fs.jpeg = {}
    assert fs.slot_layout(6, 10) == plain.slot_layout(6, 10) == (((6, 10, 3), np.uint8), ((12, 20, 3), np.uint8))
    assert R.FrameStream.PIX_FMTS == tuple(R.PIXEL_FORMATS) == ("rgb24", "i420", "nv12", "i420p10", "p010")


# ---- the directory CLI with a stub stream: what main() writes ----
class _StubStream:
    """FrameStream's surface as main() uses it; a result is the frame doubled by repetition, or with `jpeg` set Pillow's JPEG of that as bytes."""
    made = []

    def __init__(self, model, depth=2, outscale=None, **kw):
        self.kw, self.on_device, self.jpeg, self.seen = kw, None, None, []
        _StubStream.made.append(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return None

    @staticmethod
    def upscale(frame):
        return np.repeat(np.repeat(frame, 2, axis=0), 2, axis=1)

    def map(self, frames, copy=True):
        for frame in frames:
            self.seen.append(frame.shape)
            sr = self.upscale(frame)
            if self.jpeg is not None:
                out = io.BytesIO()
                Image.fromarray(sr).save(out, "JPEG", quality=self.jpeg["quality"])
                sr = np.frombuffer(out.getvalue(), dtype=np.uint8)
            yield sr


@pytest.fixture
def folder(tmp_path, monkeypatch):
    monkeypatch.setattr(inference_frames, "FrameStream", _StubStream)
    monkeypatch.setattr(inference_frames, "build_model", lambda args: _FakeModel())
    monkeypatch.setattr(torch.cuda, "set_device", lambda device: None)
    _StubStream.made.clear()
    (tmp_path / "lr").mkdir()
    rng = np.random.default_rng(3)
    frames = {}
    for i, (h, w) in enumerate([(6, 9), (5, 7), (6, 9), (8, 4), (3, 3)]):
        name = f"f{i}.{'png' if i != 1 else 'bmp'}"
        frames[name] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        Image.fromarray(frames[name]).save(tmp_path / "lr" / name)
    return tmp_path, frames


def _run(tmp_path, out, **extra):
    args = inference_frames.get_parser().parse_args(["--inputs_dir", str(tmp_path / "lr"), "--output_dir", str(tmp_path / out), "--weights_path", "none"])
    for k, v in extra.items():
        setattr(args, k, v)
    inference_frames.main(args)
    return {p.name: p.read_bytes() for p in (tmp_path / out).iterdir()}


def test_cli_defaults_are_todays_path(folder):
    args = inference_frames.get_parser().parse_args(["--inputs_dir", "a", "--output_dir", "b", "--weights_path", "c"])
    assert (args.ext, args.jpeg_quality, args.jpeg_subsampling, args.decode_workers) == ("same", 95, "420", 0)
    tmp_path, frames = folder

    def todays(name):          # what main() has always done with a result: PIL's encoder under the input's name
        out = io.BytesIO()
        Image.fromarray(_StubStream.upscale(frames[name])).save(out, format={"png": "PNG", "bmp": "BMP"}[name[-3:]])
        return out.getvalue()
    want = {name: todays(name) for name in frames}
    assert _run(tmp_path, "same") == want
    assert _StubStream.made[-1].kw == {}                                  # the stream is built with the arguments it always got
    # a namespace from before these options existed (no ext, no decode_workers attribute at all)
    inference_frames.main(types.SimpleNamespace(inputs_dir=str(tmp_path / "lr"), output_dir=str(tmp_path / "old"), weights_path="none"))
    assert {p.name: p.read_bytes() for p in (tmp_path / "old").iterdir()} == want and _StubStream.made[-1].kw == {}
    # the decode pool changes who decodes, not what is written or in which order
    assert _run(tmp_path, "pool", decode_workers=3) == want
    assert _StubStream.made[-1].seen == [frames[name].shape for name in sorted(frames)]
    assert _run(tmp_path, "pool64", decode_workers=64) == want


def test_cli_ext_jpg_writes_the_returned_bytes(folder):
    tmp_path, frames = folder
    got = _run(tmp_path, "jpg", ext="jpg", jpeg_quality=80, jpeg_subsampling="444", decode_workers=2)
    assert _StubStream.made[-1].kw == {} and _StubStream.made[-1].jpeg == dict(quality=80, subsampling="444")
    assert sorted(got) == [os.path.splitext(name)[0] + ".jpg" for name in sorted(frames)]
    for name, frame in frames.items():
        out = io.BytesIO()
        Image.fromarray(_StubStream.upscale(frame)).save(out, "JPEG", quality=80)
        assert got[os.path.splitext(name)[0] + ".jpg"] == out.getvalue(), name
    with pytest.raises(ValueError, match="--ext"):
        _run(tmp_path, "bad", ext="webp")
