"""CPU: the surface of the mixed frame formats (frames.py, MIXED FRAME FORMATS) -- the definition as a numpy composition that, for one
format on both sides, is term for term the same-format definitions; every ValueError of `upscale_frames`, `forward_yuv420_mixed` and
`FrameStream(out_pix_fmt=...)` before the device is looked at; the output slots of a mixed stream; the rawvideo parser; the two C
entries (exported, declared, bound, refusals before any launch).  Nothing here touches a device."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("resr_compact_forward_yuv420_mixed", "resr_compact_forward_yuv420_mixed_scaled")
YUV = ("i420", "nv12", "i420p10", "p010")
MATRICES = ("bt601", "bt709")
ERR_ARG, ERR_WORKSPACE = -1, -3


@pytest.fixture(scope="module")
def R():
    import __graft_entry__
    __graft_entry__.build()
    import real_esrgan_pytorch_amd as R
    return R


def definition(R, f, src, dst, float_path):
    """encode_dst(q_dst(float_path(decode_src(f) / top_src))) in numpy: the definition of the module docstring of frames.py.
    `float_path`: fp32 NCHW -> fp32 NCHW."""
    a, b = R.frames.frame_format(src, "test"), R.frames.frame_format(dst, "test")
    if a.fmt.layout is None:
        rgb = np.asarray(f)
    else:
        rgb = (R.yuv420_to_rgb_np if a.fmt.bits == 8 else R.yuv420p10_to_rgb_np)(f, a.pix_fmt, a.matrix)
    x = np.ascontiguousarray((rgb.astype(np.float32) / np.float32(a.fmt.top)).transpose(0, 3, 1, 2))
    v = float_path(x)
    assert v.dtype == np.float32
    top = np.float32(b.fmt.top)
    q = np.clip(v * top, np.float32(0), top).astype(b.fmt.np_dtype).transpose(0, 2, 3, 1)
    if b.fmt.layout is None:
        return np.ascontiguousarray(q)
    return (R.rgb_to_yuv420_np if b.fmt.bits == 8 else R.rgb_to_yuv420p10_np)(q, b.pix_fmt, b.matrix)


def _random(R, name, n, h, w, seed):
    fmt = R.PIXEL_FORMATS[name]
    hi = 256 if fmt.bits == 8 else 65536
    return np.random.RandomState(seed).randint(0, hi, size=(n, h * 3 // 2, w)).astype(fmt.np_dtype)


def _stand_in(x):
    """A float path of factor 2 with a residual's shape: nearest upsample by 2 plus a constant."""
    return np.repeat(np.repeat(x, 2, axis=2), 2, axis=3) + np.float32(0.03125)


@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("name", YUV)
def test_same_format_is_the_existing_definition(R, name, matrix):
    fmt = R.PIXEL_FORMATS[name]
    f = _random(R, name, 2, 6, 10, seed=len(name) + fmt.bits)
    fmt_ = (name, matrix)
    if fmt.bits == 8:
        # the identity float path: the definition collapses to the two integer conversions back to back (v * 255 of u8 / 255 truncates to u8)
        want = R.rgb_to_yuv420_np(R.yuv420_to_rgb_np(f, name, matrix), name, matrix)
        assert np.array_equal(definition(R, f, fmt_, fmt_, lambda x: x), want)
        rgb = R.yuv420_to_rgb_np(f, name, matrix)
        v = _stand_in(np.ascontiguousarray((rgb.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2)))
        q = np.clip(v * np.float32(255.0), np.float32(0), np.float32(255.0)).astype(np.uint8).transpose(0, 2, 3, 1)
        want = R.rgb_to_yuv420_np(q, name, matrix)
    else:
        # tests/test_gpu_yuv420p10.py's composition, on the host: unit10, the float path, q10, the way out
        rgb = R.yuv420p10_to_rgb_np(f, name, matrix)
        v = _stand_in(np.ascontiguousarray((rgb.astype(np.float32) / np.float32(1023.0)).transpose(0, 3, 1, 2)))
        q = np.clip(v * np.float32(1023.0), np.float32(0), np.float32(1023.0)).astype(np.uint16).transpose(0, 2, 3, 1)
        want = R.rgb_to_yuv420p10_np(q, name, matrix)
    got = definition(R, f, fmt_, fmt_, _stand_in)
    assert got.dtype == fmt.np_dtype and got.shape == (2, 18, 20) and np.array_equal(got, want)
    # a mixed pair is the same terms with the other side's names: 8 -> 10 keeps levels the 8-bit result cannot hold
    other = "p010" if fmt.bits == 8 else "nv12"
    mixed = definition(R, f, fmt_, (other, matrix), _stand_in)
    assert mixed.dtype == R.PIXEL_FORMATS[other].np_dtype and mixed.shape == got.shape


def test_exports_and_signatures(R):
    for name in ("upscale_frames", "FrameFormat", "PIXEL_FORMATS", "YUV_MATRICES"):
        assert name in R.__all__ and getattr(R, name) is getattr(R.frames, name), name
    assert list(inspect.signature(R.upscale_frames).parameters) == ["model", "frames", "src", "dst", "halo", "outscale", "plan"]
    assert list(inspect.signature(R.SRVGGNetCompact.forward_yuv420_mixed).parameters) == ["self", "frames", "src", "dst", "outscale", "plan"]
    params = inspect.signature(R.FrameStream.__init__).parameters
    assert list(params) == ["self", "model", "depth", "outscale", "pix_fmt", "matrix", "out_pix_fmt", "out_matrix"]
    assert params["out_pix_fmt"].default is None and params["out_matrix"].default is None
    assert R.FrameFormat("rgb24") == ("rgb24", None) and R.FrameFormat("nv12", "bt709").fmt is R.PIXEL_FORMATS["nv12"]
    assert R.frames.frame_format(("p010", "bt601"), "t") == R.FrameFormat("p010", "bt601") and R.frames.frame_format("rgb24", "t").matrix is None


class _FakeParam:
    is_cuda, device = True, torch.device("cuda", 0)


class _FakeModel:
    """What FrameStream's constructor asks of a model, with nothing on a device behind it."""
    upscale_factor = 2

    def parameters(self):
        return iter([_FakeParam()])


BAD_FORMATS = [(("yuv420p", "bt601"), "pix_fmt"), (("nv21", "bt601"), "pix_fmt"), (("nv12", "bt2020"), "matrix"), (("p010", None), "matrix"),
               (("rgb24", "bt601"), "rgb24 takes no matrix")]


def test_value_errors_come_before_the_device(R):
    m = R.SRVGGNetCompact(num_conv=1, upscale=2, precision="fast")                     # on the CPU: any look at the device raises RuntimeError
    ok8, ok10 = ("nv12", "bt601"), ("p010", "bt709")
    f8 = torch.zeros(1, 12, 8, dtype=torch.uint8)                                       # 8 x 8 luma
    with torch.no_grad():
        for bad, word in BAD_FORMATS:
            for kw in (dict(src=bad, dst=ok10), dict(src=ok8, dst=bad)):
                with pytest.raises(ValueError, match=word):
                    R.upscale_frames(m, f8, **kw)
                with pytest.raises(ValueError, match=word):
                    m.forward_yuv420_mixed(f8, **kw)
        with pytest.raises(ValueError, match="rgb24 is not fused"):
            m.forward_yuv420_mixed(f8, ok8, "rgb24")
        # an odd input size for a YUV source: rows no multiple of 3, an odd width, too few rows, no batch
        for shape in ((1, 8, 8), (1, 12, 7), (1, 2, 8), (12, 8)):
            for call in (lambda f: R.upscale_frames(m, f, ok8, ok10), lambda f: m.forward_yuv420_mixed(f, ok8, ok10)):
                with pytest.raises(ValueError, match="3H/2"):
                    call(torch.zeros(*shape, dtype=torch.uint8))
        # an odd output size for a YUV destination: 12 x 18 through x2 at outscale 2.5 is 30 x 45; an rgb24 source of odd size
        f = torch.zeros(1, 18, 18, dtype=torch.uint8)
        assert R.output_size(12, 18, 2, 2.5) == (30, 45)
        for call in (lambda: R.upscale_frames(m, f, ok8, ok10, outscale=2.5), lambda: m.forward_yuv420_mixed(f, ok8, ok10, outscale=2.5),
                     lambda: R.upscale_frames(m, torch.zeros(1, 3, 4, 3, dtype=torch.uint8), "rgb24", ok8, outscale=1)):
            with pytest.raises(ValueError, match="even"):
                call()
        for bad in (0, -1.0, float("nan"), True):
            with pytest.raises(ValueError, match="outscale"):
                R.upscale_frames(m, f8, ok8, ok10, outscale=bad)
        # everything in order: the next check is the device's, for the same format, a mixed pair and rgb24 on a side
        for kw in (dict(src=ok8), dict(src=ok8, dst=ok8), dict(src=ok8, dst=ok10), dict(src=ok8, dst="rgb24"), dict(src=ok8, dst=ok10, outscale=3)):
            with pytest.raises(RuntimeError, match="no CPU path"):
                R.upscale_frames(m, f8, **kw)
        with pytest.raises(RuntimeError, match="no CPU path"):
            R.upscale_frames(m, torch.zeros(1, 4, 4, 3, dtype=torch.uint8), ("rgb24", None), ok10)
        with pytest.raises(RuntimeError, match="no CPU path"):
            m.forward_yuv420_mixed(f8, ok8, ok10)
    # FrameStream: its ValueErrors come before it asks where the model is (a model on the CPU is a RuntimeError)
    for kw, word in ((dict(out_pix_fmt="yuv420p"), "pix_fmt"), (dict(out_matrix="bt2020"), "matrix"), (dict(pix_fmt="nv12", out_matrix="smpte"), "matrix"),
                     (dict(pix_fmt="nv12", out_pix_fmt="rgb24", out_matrix="bt709"), "rgb24 takes no matrix"),
                     (dict(out_matrix="bt709"), "rgb24 takes no matrix")):
        with pytest.raises(ValueError, match=word):
            R.FrameStream(m, 2, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.FrameStream(m, 2, pix_fmt="nv12", out_pix_fmt="p010")
    fs = R.FrameStream(_FakeModel(), 2, pix_fmt="nv12", out_pix_fmt="p010", outscale=2.5)
    with pytest.raises(ValueError, match="even"):
        fs.slot_layout(12, 18)
    with pytest.raises(ValueError, match="uint8"):                                       # an odd frame, a frame of the output's words
        fs.submit(np.zeros((18, 17), np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        fs.submit(np.zeros((18, 18), np.uint16))


def test_frame_stream_output_slots(R):
    s, h, w = 2, 12, 16
    fs = R.FrameStream(_FakeModel(), 2, pix_fmt="nv12", out_pix_fmt="p010")
    assert (fs.pix_fmt, fs.matrix, fs.out_pix_fmt, fs.out_matrix) == ("nv12", "bt601", "p010", "bt601")
    assert fs.slot_layout(h, w) == (((h * 3 // 2, w), np.dtype(np.uint8)), ((3 * s * h // 2, s * w), np.dtype(np.uint16)))
    fs = R.FrameStream(_FakeModel(), 2, outscale=3, pix_fmt="p010", matrix="bt709", out_pix_fmt="i420")
    assert fs.out_matrix == "bt709" and fs.slot_layout(h, w) == (((18, 16), np.dtype(np.uint16)), ((54, 48), np.dtype(np.uint8)))
    fs = R.FrameStream(_FakeModel(), 2, pix_fmt="i420p10", out_pix_fmt="rgb24")
    assert fs.out_matrix is None and fs.slot_layout(h, w) == (((18, 16), np.dtype(np.uint16)), ((24, 32, 3), np.dtype(np.uint8)))
    fs = R.FrameStream(_FakeModel(), 2, out_pix_fmt="nv12", out_matrix="bt709")
    assert fs.slot_layout(h, w) == (((12, 16, 3), np.dtype(np.uint8)), ((36, 32), np.dtype(np.uint8)))
    # nothing given: the input's format, and the same-format path as before there was a destination
    for kw in (dict(), dict(pix_fmt="nv12", matrix="bt709"), dict(pix_fmt="p010", out_pix_fmt="p010"), dict(pix_fmt="i420", out_matrix="bt601")):
        fs = R.FrameStream(_FakeModel(), 2, **kw)
        assert fs.out_pix_fmt == fs.pix_fmt and not fs._fmt.mixed and fs._fmt.out_dtype == fs._fmt.dtype, kw
    assert R.FrameStream(_FakeModel(), 2, pix_fmt="i420", out_matrix="bt709")._fmt.mixed


def test_rawvideo_parser(R):
    from real_esrgan_pytorch_amd import inference_rawvideo as cli
    base = ["--input", "a", "--output", "b", "--size", "8x6", "--weights_path", "w"]
    args = cli.get_parser().parse_args(base + ["--pix_fmt", "nv12", "--matrix", "bt709"])
    assert args.out_pix_fmt is None and args.out_matrix is None
    assert cli.formats(args) == ("nv12", "bt709", "nv12", "bt709")                      # the output's default to the input's
    args = cli.get_parser().parse_args(base + ["--pix_fmt", "yuv420p", "--out_pix_fmt", "p010le", "--out_matrix", "bt709"])
    assert cli.formats(args) == ("yuv420p", "bt601", "p010le", "bt709")
    assert cli.formats(cli.get_parser().parse_args(base + ["--out_pix_fmt", "yuv420p10le"])) == ("yuv420p", "bt601", "yuv420p10le", "bt601")
    for bad in (["--out_pix_fmt", "rgb24"], ["--out_matrix", "bt2020"]):
        with pytest.raises(SystemExit):
            cli.get_parser().parse_args(base + bad)
    with pytest.raises(ValueError, match="--out_pix_fmt"):
        cli.formats(types.SimpleNamespace(pix_fmt="nv12", matrix="bt601", out_pix_fmt="rgb24"))
    assert cli.formats(types.SimpleNamespace(size="8x6")) == ("yuv420p", "bt601", "yuv420p", "bt601")     # the namespaces of older callers


def test_symbols_exported_declared_and_bound(R):
    lib = C.CDLL(R._lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "resr.h")).read()
    declared = set(re.findall(r"\b(resr_[a-z0-9_]+)\s*\(", hdr))
    Y = C.POINTER(R._lib.YuvDesc)
    for name, nargs in zip(ENTRIES, (10, 18)):
        assert hasattr(lib, name) and name in declared and name in R._lib.exported_symbols(), name
        protos = R._lib._PROTOS[name][1]
        assert len(protos) == nargs and protos[2] == Y and protos[-2] == Y, name
    assert R._lib.lib().resr_version() == 3 and R._lib.RESR_VERSION == 3          # nothing an existing caller reads has moved
    assert "Mixed depths" not in hdr and "not provided" in hdr


def _fake(nbytes=128):
    """A host buffer standing in for a device pointer: the calls below return before they would launch anything."""
    buf = (C.c_uint8 * nbytes)()
    return buf, C.c_void_p((C.addressof(buf) + 31) // 32 * 32)


@pytest.mark.parametrize("scaled", (False, True))
def test_c_abi_refusals_need_no_gpu(R, scaled):
    L = R._lib
    lib = L.lib()
    keep, p = _fake()
    fwd = getattr(lib, ENTRIES[scaled])
    a, b = R.frames.yuv_desc("nv12", "bt601"), R.frames.yuv10_desc("p010", "bt709")
    good = L.CompactDesc(1, 8, 8, 16, 2, 0, L.RESR_F16, 0)                       # 8 x 8 through x2: an output width of 16, the wide stores
    ws = lib.resr_compact_workspace_bytes(C.byref(good))
    assert ws > 0

    def call(desc=good, x=p, src=a, rest=(p, p, p), wsb=None, y=p, oh=8, ow=8, tabs=(p, p, p, p), ty=10, tx=10, dst=b):
        d = C.byref(desc) if desc is not None else None
        qa, qb = (C.byref(q) if q is not None else None for q in (src, dst))
        sc = (oh, ow, tabs[0], tabs[1], ty, tabs[2], tabs[3], tx) if scaled else ()
        return fwd(d, x, qa, rest[0], rest[1], rest[2], ws if wsb is None else wsb, y, *sc, qb, None)

    def refused(word, **kw):
        assert call(**kw) == ERR_ARG, kw
        msg = lib.resr_last_error()
        assert msg and word in msg, (kw, msg)

    refused(b"null", x=None)
    refused(b"null", y=None)
    refused(b"null", src=None)
    refused(b"null", dst=None)
    for hole in range(3):                                            # params, packed, workspace
        rest = [p] * 3
        rest[hole] = None
        refused(b"null", rest=rest)
    refused(b"descriptor", desc=None)
    for layout in (4, 7, -1):                                        # an unknown layout on either side
        refused(b"layout", src=L.YuvDesc(layout, a.fq, a.iq))
        refused(b"layout", dst=L.YuvDesc(layout, b.fq, b.iq))
    for h, w in ((7, 8), (8, 7)):                                    # odd sizes
        refused(b"even", desc=L.CompactDesc(1, h, w, 16, 2, 0, L.RESR_F16, 0), wsb=1 << 40)
    # the destination's alignment rule: 16 bytes for 10-bit words at a width of 16 (4 for the scaled entry's dword rows) ...
    for off in ((2,) if scaled else (2, 4, 8)):
        refused(b"aligned", y=C.c_void_p(p.value + off))
    # ... and the 8-bit rule when the destination is 8-bit: 8 bytes, so an offset of 8 passes it (and stops at the workspace)
    if not scaled:
        refused(b"aligned", src=b, dst=a, y=C.c_void_p(p.value + 4))
        assert call(src=b, dst=a, y=C.c_void_p(p.value + 8), wsb=0) == ERR_WORKSPACE
    if scaled:                                                       # what the existing scaled entries refuse
        for kw in (dict(oh=7), dict(ow=9)):
            refused(b"even", **kw)
        for hole in range(4):
            t = [p] * 4
            t[hole] = None
            refused(b"null", tabs=t)
        for kw in (dict(ty=0), dict(tx=4097), dict(ty=-3)):
            refused(b"taps", **kw)
        for kw in (dict(oh=0), dict(ow=-4)):
            refused(b"shape", **kw)
        big = L.CompactDesc(1, 200, 200, 16, 4, 0, L.RESR_F16, 0)    # r = 0.01 on an 800 x 800 frame: no even tile fits
        refused(b"footprint", desc=big, wsb=1 << 40, ty=402, tx=402, oh=8, ow=8)
    # everything in order, for a mixed pair and for one format twice: the last check is the workspace, as for every other entry
    assert call(wsb=ws - 1) == ERR_WORKSPACE and call(src=a, dst=a, wsb=0) == ERR_WORKSPACE and call(src=b, dst=b, wsb=0) == ERR_WORKSPACE
    del keep
