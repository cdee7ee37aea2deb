"""CPU: the YUV 4:2:0 frame path's definition and surface -- the Q16 tables pinned as literals and against the reference's printed
digits, the numpy definition against the float BT.601 conversion of imgproc (the reference's rgb2ycbcr), its ranges, round trip and
layouts, the three C-ABI entries (exported, declared, bound, argument checks before any launch), the package exports, FrameStream's
argument checks and the rawvideo CLI's parser.  Nothing here touches a device."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("resr_compact_forward_yuv420", "resr_yuv420_to_rgb", "resr_rgb_to_yuv420")
ERR_ARG, ERR_WORKSPACE = -1, -3
TABLES = {
    "bt601": ([[16829, 33039, 6416], [-9714, -19071, 28784], [28784, -24103, -4681]],
              [[76309, 0, 104597], [76309, -25675, -53279], [76309, 132201, 0]]),
    "bt709": ([[11966, 40254, 4064], [-6596, -22189, 28784], [28784, -26145, -2639]],
              [[76309, 0, 117489], [76309, -13975, -34925], [76309, 138438, 0]]),
}


@pytest.fixture(scope="module")
def R():
    import __graft_entry__
    __graft_entry__.build()
    import real_esrgan_pytorch_amd as R
    return R


@pytest.fixture(scope="module")
def lattice():
    """RGB triples [M,3] uint8: a 64^3 lattice over 0..255 (both ends included) plus 10^5 random ones."""
    g = np.rint(np.linspace(0, 255, 64)).astype(np.uint8)
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([grid, np.random.RandomState(0).randint(0, 256, size=(100000, 3), dtype=np.uint8)])


def _blocks(rgb):
    """[M,3] -> a frame [2, 2M, 3] of constant 2x2 blocks, one per triple."""
    return np.ascontiguousarray(np.broadcast_to(rgb[None, :, None, :], (2, len(rgb), 2, 3)).reshape(2, 2 * len(rgb), 3))


def _samples(yuv, m):
    """I420 [3, 2M] of `_blocks` -> (Y, Cb, Cr), each [M] (the four Y of a block are checked to be one value)."""
    y = yuv[:2].reshape(2, m, 2)
    assert (y == y[:1, :, :1]).all()
    c = yuv[2].reshape(2, m)
    return y[0, :, 0].astype(np.int64), c[0].astype(np.int64), c[1].astype(np.int64)


def test_tables_are_the_pinned_literals(R):
    for matrix, (fq, iq) in TABLES.items():
        got_fq, got_iq = R.yuv420_tables(matrix)
        assert got_fq.dtype == np.int32 and got_iq.dtype == np.int32 and got_fq.shape == got_iq.shape == (3, 3)
        assert got_fq.tolist() == fq and got_iq.tolist() == iq, matrix
    assert R.yuv420_tables()[0].tolist() == TABLES["bt601"][0]
    with pytest.raises(ValueError, match="matrix"):
        R.yuv420_tables("bt2020")


def test_bt601_float_tables_match_the_reference_digits(R):
    f, i = R.frames.yuv420_tables("bt601", quantised=False)
    assert f.dtype == np.float64 and i.dtype == np.float64
    # rgb2ycbcr: [[65.481, 128.553, 24.966], [-37.797, -74.203, 112.0], [112.0, -93.786, -18.214]] per unit of [0, 1] input
    want = np.array([[65.481, 128.553, 24.966], [-37.797, -74.203, 112.0], [112.0, -93.786, -18.214]])
    assert np.abs(f * 255 - want).max() <= 5e-4
    # ycbcr2rgb: [[0.00456621, 0.00456621, 0.00456621], [0, -0.00153632, 0.00791071], [0.00625893, -0.00318811, 0]] (columns R, G, B)
    want_i = np.array([[0.00456621, 0.0, 0.00625893], [0.00456621, -0.00153632, -0.00318811], [0.00456621, 0.00791071, 0.0]])
    assert np.abs(i / 255 - want_i).max() <= 5e-9
    # ... and its offsets, which fold the -16 / -128 into one constant per channel; the reference prints them cut off after three
    # decimals, not rounded (-222.92157 as -222.921), so they agree to one unit of the last printed digit
    off = -(i @ np.array([16.0, 128.0, 128.0]))
    assert np.abs(off - np.array([-222.921, 135.576, -276.836])).max() < 1e-3


def test_lattice_against_the_float_conversion(R, lattice):
    from real_esrgan_pytorch_amd import imgproc
    m = len(lattice)
    got = _samples(R.rgb_to_yuv420_np(_blocks(lattice), "i420", "bt601"), m)
    x = torch.from_numpy(lattice.astype(np.float64) / 255.0).t().reshape(1, 3, 1, m)
    ref = torch.floor(255.0 * imgproc.rgb2ycbcr_torch(x, False) + 0.5).reshape(3, m).numpy().astype(np.int64)
    for c, name in enumerate(("Y", "Cb", "Cr")):
        d = np.abs(got[c] - ref[c])
        share = float((d != 0).mean())
        print(f"{name}: max |Q16 - float| = {int(d.max())} level, {100 * share:.3f} % of {m} samples differ")
        assert d.max() <= 1, name                     # the Q16 rounding error is below 0.006 levels: only a rounding tie region differs
        assert share <= 0.005, (name, share)


@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_ranges_grey_and_equal_blocks(R, lattice, matrix):
    m = len(lattice)
    y, cb, cr = _samples(R.rgb_to_yuv420_np(_blocks(lattice), "i420", matrix), m)
    assert (y.min(), y.max()) == (16, 235)
    assert (cb.min(), cb.max()) == (16, 240) and (cr.min(), cr.max()) == (16, 240)
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    gy, gcb, gcr = _samples(R.rgb_to_yuv420_np(_blocks(grey), "i420", matrix), 256)
    assert (gcb == 128).all() and (gcr == 128).all()
    assert gy[0] == 16 and gy[255] == 235 and (np.diff(gy) >= 0).all()
    # a 2x2 block of equal pixels gives the chroma of the single pixel: (FQ . 4 rgb + (128 << 18) + (1 << 17)) >> 18 is the
    # per-pixel (FQ . rgb + (128 << 16) + 32768) >> 16
    fq = R.yuv420_tables(matrix)[0].astype(np.int64)
    one = ((lattice.astype(np.int64) @ fq[1:].T) + (128 << 16) + 32768) >> 16
    assert np.array_equal(one[:, 0], cb) and np.array_equal(one[:, 1], cr)


@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_round_trip_of_constant_blocks(R, lattice, matrix):
    frame = _blocks(lattice)
    for layout in ("i420", "nv12"):
        back = R.yuv420_to_rgb_np(R.rgb_to_yuv420_np(frame, layout, matrix), layout, matrix)
        assert back.shape == frame.shape and back.dtype == np.uint8
        d = np.abs(back.astype(np.int64) - frame.astype(np.int64)).reshape(-1, 3).max(0)
        print(f"{matrix} {layout}: round trip max |d| R, G, B = {d.tolist()}")
        assert d.max() <= 2


def test_layouts_hold_the_same_samples(R):
    rs = np.random.RandomState(1)
    rgb = rs.randint(0, 256, size=(2, 6, 10, 3), dtype=np.uint8)
    a, b = R.rgb_to_yuv420_np(rgb, "i420"), R.rgb_to_yuv420_np(rgb, "nv12")
    assert a.shape == b.shape == (2, 9, 10) and a.dtype == b.dtype == np.uint8
    assert np.array_equal(a[:, :6], b[:, :6])
    planes = a[:, 6:].reshape(2, 2, 3, 5)                                  # Cb, Cr planes
    pairs = b[:, 6:].reshape(2, 3, 5, 2)                                   # interleaved
    assert np.array_equal(planes[:, 0], pairs[..., 0]) and np.array_equal(planes[:, 1], pairs[..., 1])
    # the way in reads them the same: every byte value is legal, in either layout, with or without a batch axis
    f = rs.randint(0, 256, size=(2, 9, 10), dtype=np.uint8)
    g = f.copy()
    g[:, 6:] = np.stack([f[:, 6:].reshape(2, 2, 15)[:, 0], f[:, 6:].reshape(2, 2, 15)[:, 1]], -1).reshape(2, 3, 10)
    assert np.array_equal(R.yuv420_to_rgb_np(f, "i420"), R.yuv420_to_rgb_np(g, "nv12"))
    assert np.array_equal(R.yuv420_to_rgb_np(f[0], "i420"), R.yuv420_to_rgb_np(f, "i420")[0])
    assert R.yuv420_to_rgb_np(f, "i420").shape == (2, 6, 10, 3)
    # the formula, spelled out for one pixel: (y, x) = (3, 5) takes Y[3,5], Cb[1,2], Cr[1,2]
    iq = np.array(TABLES["bt601"][1], dtype=np.int64)
    v = np.array([int(f[0, 3, 5]) - 16, int(f[0, 6:].reshape(2, 3, 5)[0, 1, 2]) - 128, int(f[0, 6:].reshape(2, 3, 5)[1, 1, 2]) - 128])
    assert R.yuv420_to_rgb_np(f, "i420")[0, 3, 5].tolist() == np.clip((iq @ v + 32768) >> 16, 0, 255).tolist()
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((6, 5), np.uint8), np.zeros((6, 4), np.float32)):
        with pytest.raises(ValueError):
            R.yuv420_to_rgb_np(bad)
    for bad in (np.zeros((3, 4, 3), np.uint8), np.zeros((4, 5, 3), np.uint8), np.zeros((4, 4), np.uint8)):
        with pytest.raises(ValueError):
            R.rgb_to_yuv420_np(bad)
    with pytest.raises(ValueError, match="layout"):
        R.rgb_to_yuv420_np(rgb, "yv12")


def test_symbols_exported_declared_and_bound(R):
    lib = C.CDLL(R._lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "resr.h")).read()
    declared = set(re.findall(r"\b(resr_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in declared, name
        assert name in R._lib.exported_symbols(), name
    assert "RESR_YUV_I420 = 0" in hdr and "RESR_YUV_NV12 = 1" in hdr and "ResrYuvDesc" in hdr
    assert (R._lib.YUV_I420, R._lib.YUV_NV12) == (0, 1) and C.sizeof(R._lib.YuvDesc) == 19 * 4
    d = R.frames.yuv_desc("nv12", "bt709")
    assert d.layout == 1 and list(d.fq) == sum(TABLES["bt709"][0], []) and list(d.iq) == sum(TABLES["bt709"][1], [])


def test_package_exports(R):
    for name in ("yuv420_tables", "yuv420_to_rgb_np", "rgb_to_yuv420_np", "yuv420_to_rgb", "rgb_to_yuv420", "upscale_yuv420"):
        assert hasattr(R, name) and name in R.__all__ and name in R.frames.__all__, name
        assert getattr(R, name) is getattr(R.frames, name)
    assert callable(R.SRVGGNetCompact.forward_yuv420)


def _fake(nbytes=64):
    """A host buffer standing in for a device pointer: the calls below return before they would launch anything."""
    buf = (C.c_uint8 * nbytes)()
    base = C.addressof(buf)
    return buf, C.c_void_p((base + 15) // 16 * 16)


def test_c_abi_argument_checks_need_no_gpu(R):
    L = R._lib
    lib = L.lib()
    keep, p = _fake()
    ok = R.frames.yuv_desc("i420", "bt601")
    bad_layout = L.YuvDesc(2, ok.fq, ok.iq)
    for fn in (lib.resr_yuv420_to_rgb, lib.resr_rgb_to_yuv420):
        for n, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, 3, 4), (1, 4, 5), (1, 6, 2 + 1)):
            assert fn(p, p, n, h, w, C.byref(ok), None) == ERR_ARG, (n, h, w)
        assert fn(None, p, 1, 4, 4, C.byref(ok), None) == ERR_ARG
        assert fn(p, None, 1, 4, 4, C.byref(ok), None) == ERR_ARG
        assert fn(p, p, 1, 4, 4, None, None) == ERR_ARG
        assert fn(p, p, 1, 4, 4, C.byref(bad_layout), None) == ERR_ARG
        assert b"layout" in lib.resr_last_error()
    odd = C.c_void_p(p.value + 2)
    assert lib.resr_yuv420_to_rgb(p, odd, 1, 4, 4, C.byref(ok), None) == ERR_ARG          # w % 4 == 0: dword stores
    assert lib.resr_rgb_to_yuv420(p, odd, 1, 4, 4, C.byref(ok), None) == ERR_ARG
    assert lib.resr_rgb_to_yuv420(odd, p, 1, 4, 4, C.byref(ok), None) == ERR_ARG          # ... and dword loads of the HWC side
    good = L.CompactDesc(1, 8, 8, 16, 4, 0, L.RESR_F16, 0)
    ws = lib.resr_compact_workspace_bytes(C.byref(good))
    fwd = lib.resr_compact_forward_yuv420
    assert fwd(None, p, p, p, p, ws, p, C.byref(ok), None) == ERR_ARG
    for hole in range(5):                                          # x_yuv, params, packed, workspace, y_yuv
        a = [p] * 5
        a[hole] = None
        assert fwd(C.byref(good), a[0], a[1], a[2], a[3], ws, a[4], C.byref(ok), None) == ERR_ARG, hole
        assert b"null" in lib.resr_last_error()
    assert fwd(C.byref(good), p, p, p, p, ws, p, None, None) == ERR_ARG
    assert fwd(C.byref(good), p, p, p, p, ws, p, C.byref(bad_layout), None) == ERR_ARG
    for h, w in ((7, 8), (8, 7), (1, 1)):
        assert fwd(C.byref(L.CompactDesc(1, h, w, 16, 4, 0, L.RESR_F16, 0)), p, p, p, p, 1 << 40, p, C.byref(ok), None) == ERR_ARG
        assert b"even" in lib.resr_last_error()
    assert fwd(C.byref(good), p, p, p, p, ws, C.c_void_p(p.value + 4), C.byref(ok), None) == ERR_ARG    # output width 32: 8-byte stores
    assert b"aligned" in lib.resr_last_error()
    assert fwd(C.byref(good), p, p, p, p, ws - 1, p, C.byref(ok), None) == ERR_WORKSPACE   # nothing more than the u8 path's
    del keep


def test_frame_stream_argument_checks(R):
    cpu_model = R.SRVGGNetCompact(num_conv=1, precision="fast")
    for pix_fmt in ("yuv420p", "rgb", "I420", None):
        with pytest.raises(ValueError, match="pix_fmt"):
            R.FrameStream(cpu_model, pix_fmt=pix_fmt)
    with pytest.raises(ValueError, match="matrix"):
        R.FrameStream(cpu_model, pix_fmt="i420", matrix="bt2020")
    for pix_fmt in ("rgb24", "i420", "nv12"):
        with pytest.raises(RuntimeError, match="no CPU path"):
            R.FrameStream(cpu_model, pix_fmt=pix_fmt)
    ok = np.zeros((9, 8), np.uint8)
    R.FrameStream.check_frame_yuv420(ok)
    for bad in (np.zeros((8, 8), np.uint8), np.zeros((10, 8), np.uint8),        # rows not a multiple of 3
                np.zeros((9, 7), np.uint8),                                     # an odd W
                np.zeros((0, 8), np.uint8), ok.astype(np.float32), np.zeros((9, 8, 3), np.uint8), ok[None],
                torch.zeros(9, 8, dtype=torch.uint8), [[1, 2]]):
        with pytest.raises(ValueError, match="3H/2"):
            R.FrameStream.check_frame_yuv420(bad)
    R.FrameStream.check_frame(np.zeros((5, 7, 3), np.uint8))          # the RGB check is what it was


def test_device_functions_refuse_cpu_tensors(R):
    f = torch.zeros(1, 6, 4, dtype=torch.uint8)
    m = R.SRVGGNetCompact(num_conv=1, precision="fast")
    with torch.no_grad():
        for call in (lambda: R.yuv420_to_rgb(f), lambda: R.rgb_to_yuv420(torch.zeros(1, 4, 4, 3, dtype=torch.uint8)),
                     lambda: R.upscale_yuv420(m, f), lambda: m.forward_yuv420(f)):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call()
        with pytest.raises(ValueError, match="layout"):
            m.forward_yuv420(f, layout="yv12")
        with pytest.raises(ValueError, match="matrix"):
            R.upscale_yuv420(m, f, matrix="bt2020")
    with pytest.raises(RuntimeError, match="backward"):
        m.forward_yuv420(f)


def test_inference_rawvideo_parser_and_reader(R):
    from real_esrgan_pytorch_amd import inference_rawvideo as V
    p = V.get_parser()
    a = p.parse_args(["--input", "-", "--output", "O", "--size", "1920x1080", "--weights_path", "W"])
    assert (a.input, a.output, a.size, a.weights_path) == ("-", "O", "1920x1080", "W")
    assert (a.pix_fmt, a.matrix, a.model_type, a.num_conv, a.act_type, a.precision, a.depth, a.outscale) == \
        ("yuv420p", "bt601", "rrdb", 16, "prelu", None, 2, None)
    a = p.parse_args(["--input", "I", "--output", "-", "--size", "8x6", "--weights_path", "W", "--pix_fmt", "nv12", "--matrix", "bt709",
                      "--model_type", "compact", "--num_conv", "32", "--act_type", "relu", "--precision", "fast", "--depth", "3",
                      "--outscale", "2"])
    assert (a.pix_fmt, a.matrix, a.model_type, a.num_conv, a.act_type, a.precision, a.depth, a.outscale) == \
        ("nv12", "bt709", "compact", 32, "relu", "fast", 3, 2.0)
    for bad in (["--pix_fmt", "rgb24"], ["--matrix", "bt2020"], ["--model_type", "vgg"]):
        with pytest.raises(SystemExit):
            p.parse_args(["--input", "I", "--output", "O", "--size", "8x6", "--weights_path", "W"] + bad)
    with pytest.raises(SystemExit):
        p.parse_args(["--input", "I", "--output", "O", "--weights_path", "W"])          # --size is required
    assert V.parse_size("8x6") == (8, 6) and V.parse_size("1920X1080") == (1920, 1080)
    for bad in ("8", "8x", "7x6", "8x5", "0x0", "axb", ""):
        with pytest.raises(ValueError, match="size"):
            V.parse_size(bad)
    raw = bytes(range(72)) * 2                                      # two 8x6 frames of 72 bytes
    got = list(V.read_frames(io.BytesIO(raw), 8, 6))
    assert len(got) == 2 and got[0].shape == (9, 8) and got[0].dtype == np.uint8 and got[1].tobytes() == raw[72:]
    assert list(V.read_frames(io.BytesIO(b""), 8, 6)) == []
    with pytest.raises(ValueError, match="31 trailing bytes"):
        list(V.read_frames(io.BytesIO(raw + bytes(31)), 8, 6))
    assert hasattr(V, "main")
