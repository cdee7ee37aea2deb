"""The PNG encoder's surface without a device: the C entries (declared once, exported, every refusal before a launch, the host-side
header and the size bounds, on the cross-compiled library), the Python layer's ValueErrors, FrameStream.png's checks and the directory
CLI's `--ext png` with a stub stream."""
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
from real_esrgan_pytorch_amd import _lib, inference_frames, png_encode
from tests import png_encode_cases as K
from tests import png_encode_ref as P
from tests.test_jpeg_encode_surface import _FakeModel, _StubStream, _run, folder  # noqa: F401  (the fixture)

ENTRIES = ("resr_png_encode_max_bytes", "resr_png_encode_workspace_bytes", "resr_png_encode_header", "resr_png_encode",
           "resr_png_debug_deflate_workspace_bytes", "resr_png_debug_deflate", "resr_png_debug_build_code")


def _desc(n=1, h=16, w=16, c=3, depth=8, segment_bytes=0):
    return _lib.PngEncDesc(n, h, w, c, depth, segment_bytes)


def test_entries_are_declared_once_and_exported():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "resr.h")).read()
    text += open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "resr_debug.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)          # the declarations alone
    for name in ENTRIES:
        assert text.count(name + "(") == 1, name
        assert callable(getattr(_lib.lib(), name)) and name in _lib.exported_symbols()
    assert [f[0] for f in _lib.PngEncDesc._fields_] == ["n", "h", "w", "channels", "bit_depth", "segment_bytes"]
    assert _lib.RESR_PNG_DEFAULT_SEGMENT_BYTES == P.DEFAULT_SEGMENT_BYTES == 16384 and _lib.RESR_PNG_HEADER_BYTES == P.HEADER_BYTES == 47
    for name in ("png_encode", "encode_png", "png_files", "png_max_bytes"):
        assert hasattr(R, name) and name in R.__all__, name
    assert R.encode_png is png_encode.encode_png


BAD_DESCS = [(dict(n=0), "geometry"), (dict(h=0), "geometry"), (dict(w=0), "geometry"), (dict(w=2 ** 31 // 3 + 1), "geometry"), (dict(h=2 ** 30, c=4, depth=16), "geometry"),
             (dict(c=2), "channels"), (dict(c=0), "channels"), (dict(c=5), "channels"), (dict(depth=1), "depth"), (dict(depth=12), "depth"),
             (dict(segment_bytes=63), "segment_bytes"), (dict(segment_bytes=65536), "segment_bytes"), (dict(segment_bytes=-1), "segment_bytes"),
             (dict(n=2 ** 20, h=4096, w=4096, segment_bytes=64), "grid")]


def test_every_refusal_comes_before_a_launch():
    lib = _lib.lib()
    fake = C.c_void_p(0x10000)          # never dereferenced: every call below is refused first

    def encode(d, src=fake, out=fake, stride=1 << 20, lengths=fake, header=fake, header_bytes=_lib.RESR_PNG_HEADER_BYTES, ws=fake, ws_bytes=1 << 60):
        return lib.resr_png_encode(C.byref(d) if d is not None else None, src, out, stride, lengths, header, header_bytes, ws, ws_bytes, None)

    def refused(rc, word):
        assert rc == _lib.RESR_ERR_ARG, rc
        text = lib.resr_last_error().decode()
        assert "png_encode" in text and word in text, text
    for kw, word in BAD_DESCS:
        d = _desc(**kw)
        refused(encode(d), word)
        assert lib.resr_png_encode_max_bytes(C.byref(d)) == 0 and lib.resr_png_encode_workspace_bytes(C.byref(d)) == 0
        refused(lib.resr_png_encode_header(C.byref(d), (C.c_uint8 * 64)(), 64), word)
    refused(encode(None), "null descriptor")
    assert lib.resr_png_encode_max_bytes(None) == 0 and lib.resr_png_encode_workspace_bytes(None) == 0
    d = _desc()
    for which in ("src", "out", "lengths", "header", "ws"):
        refused(encode(d, **{which: None}), "null pointer")
    refused(encode(d, header_bytes=_lib.RESR_PNG_HEADER_BYTES - 1), "header")
    refused(encode(d, header_bytes=0), "header")
    refused(encode(d, stride=-1), "out_stride")
    need = lib.resr_png_encode_workspace_bytes(C.byref(d))
    assert need > 0
    refused(encode(d, ws_bytes=need - 1), "workspace")
    refused(encode(d, ws=C.c_void_p(0x10008)), "aligned")
    refused(encode(d, lengths=C.c_void_p(0x10004)), "aligned")
    refused(lib.resr_png_encode_header(C.byref(d), (C.c_uint8 * 46)(), 46), "needed")
    assert lib.resr_png_encode_header(C.byref(d), None, 0) == _lib.RESR_PNG_HEADER_BYTES          # the length alone
    # the test entries
    assert lib.resr_png_debug_deflate_workspace_bytes(0, 64) == 0 and lib.resr_png_debug_deflate_workspace_bytes(100, 63) == 0
    assert lib.resr_png_debug_deflate_workspace_bytes(100, 64) > 0
    for args in ((fake, 0, 64), (fake, 100, 65536), (None, 100, 64)):
        assert lib.resr_png_debug_deflate(args[0], args[1], args[2], fake, 1 << 20, fake, fake, 1 << 40, None) == _lib.RESR_ERR_ARG
        assert "png_debug_deflate" in lib.resr_last_error().decode()
    for args in ((None, 19, 7, fake), (fake, 0, 7, fake), (fake, 287, 15, fake), (fake, 19, 0, fake), (fake, 19, 16, fake), (fake, 19, 4, fake), (fake, 19, 7, None)):
        assert lib.resr_png_debug_build_code(*args, None) == _lib.RESR_ERR_ARG
        assert "png_debug_build_code" in lib.resr_last_error().decode()


@pytest.mark.parametrize("h,w,c,depth", [(16, 16, 3, 8), (38, 30, 4, 16), (1, 1, 1, 8), (7, 1, 1, 16), (2 ** 31 - 1, 1, 1, 8), (1, 2 ** 31 - 1, 1, 8), (1, (2 ** 31 - 1) // 8, 4, 16), (4320, 7680, 3, 8)])
def test_header_is_the_definitions(h, w, c, depth):
    buf = (C.c_uint8 * 64)()
    d = _desc(1, h, w, c, depth)
    assert _lib.lib().resr_png_encode_header(C.byref(d), buf, 64) == 47, _lib.lib().resr_last_error()
    assert bytes(buf[:47]) == P.header_np(h, w, c, depth)
    if h * w < 4096:
        image = K.noise(h, w, c, depth)
        assert P.encode_png_np(image)[:47] == bytes(buf[:47])


def test_bounds_hold_for_noise_and_grow_with_the_geometry():
    lib = _lib.lib()
    for (h, w), c, depth, s in (((33, 47), 3, 8, 64), ((33, 47), 4, 16, 100), ((64, 48), 1, 8, 0), ((1, 1), 1, 8, 0), ((7, 1), 3, 16, 65535)):
        d = _desc(1, h, w, c, depth, s)
        bound = lib.resr_png_encode_max_bytes(C.byref(d))
        t = h * (1 + w * c * depth // 8)
        k = -(-t // (s or 16384))
        assert bound == t + 17 * k + 75 == P.max_bytes_np(h, w, c, depth, s or None)
        assert bound >= max(len(P.encode_png_np(K.noise(h, w, c, depth, seed), s or None)) for seed in range(3))
        assert lib.resr_png_encode_workspace_bytes(C.byref(d)) >= k * (min(t, s or 16384) + 5 + 24) + h
        assert png_encode.png_max_bytes((1, h, w, c), np.dtype(f"uint{depth}"), s or None) == bound
    last = (0, 0)
    for h, w in ((8, 8), (8, 64), (64, 64), (1080, 1920), (4320, 7680)):
        d = _desc(1, h, w)
        now = (lib.resr_png_encode_max_bytes(C.byref(d)), lib.resr_png_encode_workspace_bytes(C.byref(d)))
        assert now[0] > last[0] and now[1] > last[1]
        last = now
        d2 = _desc(2, h, w)
        assert lib.resr_png_encode_max_bytes(C.byref(d2)) == now[0] and lib.resr_png_encode_workspace_bytes(C.byref(d2)) > now[1]
    assert lib.resr_png_encode_max_bytes(C.byref(_desc(1, 4320, 7680))) == 4320 * 23041 + 17 * 6076 + 75          # 6,076 segments at the default


def test_value_errors_of_the_python_layer_come_before_the_device():
    frames = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    for kw, word in ((dict(segment_bytes=63), "segment_bytes"), (dict(segment_bytes=65536), "segment_bytes"), (dict(segment_bytes=True), "segment_bytes"),
                     (dict(segment_bytes=100.0), "segment_bytes"), (dict(segment_bytes=0), "segment_bytes"), (dict(capacity=0), "capacity"), (dict(capacity=1.5), "capacity")):
        for call in (R.encode_png, R.png_files):
            with pytest.raises(ValueError, match=word):
                call(frames, **kw)
    for bad in (torch.zeros(8, 8, dtype=torch.uint8), torch.zeros(1, 8, 8, 2, dtype=torch.uint8), torch.zeros(1, 8, 8, 3), torch.zeros(0, 8, 8, 3, dtype=torch.uint8),
                torch.zeros(1, 8, 8, 3, dtype=torch.int16), np.zeros((1, 8, 8, 3), dtype=np.uint8)):
        with pytest.raises(ValueError, match="N,H,W,C|at least 1"):
            R.encode_png(bad)
    with pytest.raises(ValueError, match="segment_bytes"):
        R.png_max_bytes((1, 8, 8, 3), segment_bytes=10)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.encode_png(frames)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.encode_png(torch.zeros(2, 8, 8, dtype=torch.uint16))


def test_frame_stream_png_argument_checks():
    """`png` is an attribute of the stream (like `jpeg` and `on_device`): the constructor's parameter list stays what it was."""
    import inspect
    assert "png" not in inspect.signature(R.FrameStream.__init__).parameters and isinstance(R.FrameStream.png, property)
    for kw in (dict(pix_fmt="nv12"), dict(pix_fmt="i420"), dict(pix_fmt="p010"), dict(out_pix_fmt="nv12"), dict(pix_fmt="nv12", out_pix_fmt="rgb24"),
               dict(out_pix_fmt="i420p10")):
        fs = R.FrameStream(_FakeModel(), 2, **kw)
        with pytest.raises(ValueError, match="rgb24"):
            fs.png = {}
        assert fs.png is None
        fs.png = None          # (switching it off is always allowed)
    fs = R.FrameStream(_FakeModel(), 2)
    assert fs.png is None and fs.png_fallbacks == 0 and fs.png_capacity is None and fs.jpeg is None
    for bad, word in ((dict(segment_bytes=63), "segment_bytes"), (dict(segment_bytes=65536), "segment_bytes"), (dict(quality=90), "segment_bytes"), ("png", "dict")):
        with pytest.raises(ValueError, match=word):
            fs.png = bad
        assert fs.png is None
    fs.png = {}
    assert fs.png == dict(segment_bytes=None)
    with pytest.raises(ValueError, match="both"):
        fs.jpeg = {}
    assert fs.jpeg is None and fs.png == dict(segment_bytes=None)
    fs.png = dict(segment_bytes=4096)
    assert fs.png == dict(segment_bytes=4096)
    fs._ready.append(np.zeros(1, dtype=np.uint8))          # a result not yet taken: it was made under the old setting
    with pytest.raises(RuntimeError, match="outstanding"):
        fs.png = None
    fs._ready.clear()
    fs.png = None
    fs.jpeg = {}
    with pytest.raises(ValueError, match="both"):
        fs.png = {}
    assert fs.png is None and fs.jpeg is not None
    fs.jpeg = None
    plain = R.FrameStream(_FakeModel(), 2)
    fs.png = {}
    assert fs.slot_layout(6, 10) == plain.slot_layout(6, 10) == (((6, 10, 3), np.uint8), ((12, 20, 3), np.uint8))


class _PngStub(_StubStream):
    """... with `png` set, a result is Pillow's PNG of the doubled frame, marked by a text chunk no other path writes."""

    def __init__(self, model, depth=2, outscale=None, **kw):
        super().__init__(model, depth, outscale, **kw)
        self.png = None

    def map(self, frames, copy=True):
        if self.png is None:
            yield from super().map(frames, copy)
            return
        for frame in frames:
            out = io.BytesIO()
            Image.fromarray(self.upscale(frame)).save(out, "PNG", compress_level=1)
            yield np.frombuffer(out.getvalue(), dtype=np.uint8)


def test_cli_ext_png_writes_the_returned_bytes(folder, monkeypatch):  # noqa: F811
    args = inference_frames.get_parser().parse_args(["--inputs_dir", "a", "--output_dir", "b", "--weights_path", "c"])
    assert (args.ext, args.jpeg_quality, args.jpeg_subsampling, args.decode_workers, args.keep_mode) == ("same", 95, "420", 0, False)
    assert inference_frames.get_parser().parse_args(["--inputs_dir", "a", "--output_dir", "b", "--weights_path", "c", "--ext", "png"]).ext == "png"
    with pytest.raises(SystemExit):
        inference_frames.get_parser().parse_args(["--inputs_dir", "a", "--output_dir", "b", "--weights_path", "c", "--ext", "webp"])
    monkeypatch.setattr(inference_frames, "FrameStream", _PngStub)
    tmp_path, frames = folder
    stems = {os.path.splitext(name)[0] for name in frames}
    assert len(stems) == len(frames)
    got = _run(tmp_path, "png", ext="png", decode_workers=2)
    assert _StubStream.made[-1].kw == {} and _StubStream.made[-1].png == {} and _StubStream.made[-1].jpeg is None
    assert sorted(got) == sorted(stem + ".png" for stem in stems)
    for name, frame in frames.items():
        out = io.BytesIO()
        Image.fromarray(_StubStream.upscale(frame)).save(out, "PNG", compress_level=1)
        assert got[os.path.splitext(name)[0] + ".png"] == out.getvalue(), name          # the stream's bytes, not a second encode
    # `same` on the same stub: today's files, and the stream's png is never touched
    same = _run(tmp_path, "same")
    assert _StubStream.made[-1].png is None and sorted(same) == sorted(frames)
    with pytest.raises(ValueError, match="--ext"):
        _run(tmp_path, "bad", ext="webp")
    inference_frames.main(types.SimpleNamespace(inputs_dir=str(tmp_path / "lr"), output_dir=str(tmp_path / "old"), weights_path="none"))
    assert {p.name: p.read_bytes() for p in (tmp_path / "old").iterdir()} == same
