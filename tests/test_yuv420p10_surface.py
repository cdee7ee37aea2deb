"""CPU: the 10-bit YUV 4:2:0 frame path's definition and surface -- the Q16 tables against quoted literals, the ranges and
accumulator bounds over the corner triples, both sample packings (ignored bits on the way in, zero bits on the way out), the grey ramp,
the integer conversions against rint of the float64 studio formula, the ValueErrors, the three C-ABI entries (exported, declared,
bound, argument checks before any launch), the package exports, FrameStream's and the rawvideo CLI's checks.  Nothing here touches a
device."""
import ctypes as C
import inspect
import io
import itertools
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("resr_compact_forward_yuv420p10", "resr_yuv420p10_to_nchw", "resr_nchw_to_yuv420p10")
LAYOUTS = ("i420p10", "p010")
MATRICES = ("bt601", "bt709")
ERR_ARG, ERR_WORKSPACE = -1, -3


@pytest.fixture(scope="module")
def R():
    import __graft_entry__
    __graft_entry__.build()
    import real_esrgan_pytorch_amd as R
    return R


def _blocks(rgb):
    """[M,3] -> a frame [2, 2M, 3] of constant 2x2 blocks, one per triple."""
    return np.ascontiguousarray(np.broadcast_to(rgb[None, :, None, :], (2, len(rgb), 2, 3)).reshape(2, 2 * len(rgb), 3))


def _samples(yuv, m):
    """i420p10 [3, 2M] of `_blocks` -> (Y, Cb, Cr), each [M] (the four Y of a block are checked to be one value)."""
    y = yuv[:2].reshape(2, m, 2)
    assert (y == y[:1, :, :1]).all()
    c = yuv[2].reshape(2, m)
    return y[0, :, 0].astype(np.int64), c[0].astype(np.int64), c[1].astype(np.int64)


def test_tables_reproduce_the_quoted_values(R):
    fq, iq = R.yuv420p10_tables("bt601")
    assert fq.dtype == np.int32 and iq.dtype == np.int32 and fq.shape == iq.shape == (3, 3)
    assert fq[0].tolist() == [16780, 32942, 6398] and iq[0].tolist() == [76533, 0, 104905]
    fq, iq = R.yuv420p10_tables("bt709")
    assert fq[0].tolist() == [11931, 40136, 4052] and iq[2].tolist() == [76533, 138846, 0]
    assert R.yuv420p10_tables()[0].tolist() == R.yuv420p10_tables("bt601")[0].tolist()
    # the float tables are the 8-bit ones rescaled: F per level * 1023 = 4 x (F8 per level * 255), I * 1023 = I8 * 255 / 4
    for matrix in MATRICES:
        f, i = R.yuv420p10_tables(matrix, quantised=False)
        f8, i8 = R.yuv420_tables(matrix, quantised=False)
        assert f.dtype == np.float64 and np.allclose(f * 1023, f8 * 255 * 4, rtol=1e-12, atol=0)
        assert np.allclose(i[:, 0], 1023 / 876) and np.allclose(i[:, 1:] * 896 / 1023, i8[:, 1:] * 224 / 255, rtol=1e-12, atol=0)
        assert np.array_equal(R.yuv420p10_tables(matrix)[0], np.rint(f * 65536).astype(np.int32))
    with pytest.raises(ValueError, match="matrix"):
        R.yuv420p10_tables("bt2020")


@pytest.mark.parametrize("matrix", MATRICES)
def test_ranges_and_accumulators_over_the_corners(R, matrix):
    """The conversions are linear, so the extremes sit at the 8 corner triples (x 4 for the block sums S)."""
    corners = np.array(list(itertools.product((0, 1023), repeat=3)), dtype=np.uint16)
    y, cb, cr = _samples(R.rgb_to_yuv420p10_np(_blocks(corners), "i420p10", matrix), 8)
    assert (y.min(), y.max()) == (64, 940)
    assert (cb.min(), cb.max()) == (64, 960) and (cr.min(), cr.max()) == (64, 960)
    fq, iq = (t.astype(np.int64) for t in R.yuv420p10_tables(matrix))
    c = corners.astype(np.int64)
    acc_y = c @ fq[0] + (64 << 16) + 32768
    acc_c = (4 * c) @ fq[1:].T + (512 << 18) + (1 << 17)
    assert 0 <= acc_y.min() and 0 <= acc_c.min()
    assert max(acc_y.max(), acc_c.max()) <= 251_789_200 < 2 ** 31
    # the way in, with 10-bit operands: every corner of (Y, Cb, Cr) in 0..1023
    ycc = c - np.array([64, 512, 512])
    acc_in = np.abs(ycc @ iq.T) + 32768
    assert acc_in.max() < 1.5e8 < 2 ** 31


@pytest.mark.parametrize("matrix", MATRICES)
def test_packings_ignore_and_zero_the_other_bits(R, matrix):
    rs = np.random.RandomState(5)
    samples = rs.randint(0, 1024, size=(2, 9, 10)).astype(np.uint16)
    garbage = rs.randint(0, 64, size=samples.shape).astype(np.uint16)
    clean = {"i420p10": samples, "p010": samples << 6}
    dirty = {"i420p10": samples | (garbage << 10), "p010": (samples << 6) | garbage}
    for layout in LAYOUTS:
        assert (dirty[layout] != clean[layout]).any()
        a, b = R.yuv420p10_to_rgb_np(clean[layout], layout, matrix), R.yuv420p10_to_rgb_np(dirty[layout], layout, matrix)
        assert a.dtype == np.uint16 and a.shape == (2, 6, 10, 3) and a.max() <= 1023 and np.array_equal(a, b)
    rgb = rs.randint(0, 1024, size=(2, 6, 10, 3)).astype(np.uint16)
    rgb.reshape(-1)[:2] = (0, 1023)
    lo, hi = R.rgb_to_yuv420p10_np(rgb, "i420p10", matrix), R.rgb_to_yuv420p10_np(rgb, "p010", matrix)
    assert lo.dtype == hi.dtype == np.uint16 and lo.shape == hi.shape == (2, 9, 10)
    assert (lo >> 10 == 0).all() and (hi & 63 == 0).all()
    # the two layouts hold the same samples: Y equal, the Cb / Cr planes of one the interleaved pairs of the other
    assert np.array_equal(lo[:, :6], hi[:, :6] >> 6)
    planes, pairs = lo[:, 6:].reshape(2, 2, 3, 5), (hi[:, 6:] >> 6).reshape(2, 3, 5, 2)
    assert np.array_equal(planes[:, 0], pairs[..., 0]) and np.array_equal(planes[:, 1], pairs[..., 1])
    # ... and are read the same, with or without a batch axis
    back = R.yuv420p10_to_rgb_np(lo, "i420p10", matrix)
    assert np.array_equal(back, R.yuv420p10_to_rgb_np(hi, "p010", matrix))
    assert np.array_equal(back[0], R.yuv420p10_to_rgb_np(lo[0], "i420p10", matrix))
    # the formula, spelled out for one pixel: (y, x) = (3, 5) takes Y[3,5], Cb[1,2], Cr[1,2]
    iq = R.yuv420p10_tables(matrix)[1].astype(np.int64)
    v = np.array([int(lo[0, 3, 5]) - 64, int(planes[0, 0, 1, 2]) - 512, int(planes[0, 1, 1, 2]) - 512])
    assert back[0, 3, 5].tolist() == np.clip((iq @ v + 32768) >> 16, 0, 1023).tolist()


@pytest.mark.parametrize("matrix", MATRICES)
def test_grey_ramp_round_trips_within_one_level(R, matrix):
    grey = np.repeat(np.arange(1024, dtype=np.uint16)[:, None], 3, 1)
    for layout in LAYOUTS:
        yuv = R.rgb_to_yuv420p10_np(_blocks(grey), layout, matrix)
        back = R.yuv420p10_to_rgb_np(yuv, layout, matrix)
        d = np.abs(back.astype(np.int64) - _blocks(grey).astype(np.int64))
        print(f"{matrix} {layout}: grey ramp round trip max |d| = {int(d.max())}")
        assert d.max() <= 1
    y, cb, cr = _samples(R.rgb_to_yuv420p10_np(_blocks(grey), "i420p10", matrix), 1024)
    assert (cb == 512).all() and (cr == 512).all() and y[0] == 64 and y[1023] == 940 and (np.diff(y) >= 0).all()


@pytest.mark.parametrize("matrix", MATRICES)
def test_integer_conversions_against_the_float64_studio_formula(R, matrix):
    """Coefficient error <= 2^-17 per Q16 entry x 3 terms x 1023 is about 0.02 level: against rint of the float64 formula the integer
    result differs by one level at most (only where the float value is within that distance of a rounding tie)."""
    f, i = R.yuv420p10_tables(matrix, quantised=False)
    rs = np.random.RandomState(2)
    rgb = rs.randint(0, 1024, size=(200000, 3)).astype(np.uint16)
    got = _samples(R.rgb_to_yuv420p10_np(_blocks(rgb), "i420p10", matrix), len(rgb))
    ref = np.rint(rgb.astype(np.float64) @ f.T + np.array([64.0, 512.0, 512.0])).astype(np.int64)
    for c, name in enumerate(("Y", "Cb", "Cr")):
        d = np.abs(got[c] - ref[:, c])
        print(f"{matrix} out {name}: max |Q16 - float64| = {int(d.max())} level, {100 * float((d != 0).mean()):.3f} % of {len(rgb)} samples differ")
        assert d.max() <= 1, name
    # the way in, on studio-range samples (outside it both sides clamp alike, which proves less)
    ycc = np.stack([rs.randint(64, 941, size=200000), rs.randint(64, 961, size=200000), rs.randint(64, 961, size=200000)], -1)
    frame = np.stack([np.repeat(ycc[:, 0], 2), np.repeat(ycc[:, 0], 2),
                      np.concatenate([ycc[:, 1], ycc[:, 2]])]).astype(np.uint16)                     # i420p10 [3, 2M]: one block per triple
    got_rgb = R.yuv420p10_to_rgb_np(frame, "i420p10", matrix)[0, ::2].astype(np.int64)                  # one pixel per block
    ref_rgb = np.clip(np.rint((ycc - np.array([64.0, 512.0, 512.0])) @ i.T), 0, 1023).astype(np.int64)
    d = np.abs(got_rgb - ref_rgb)
    print(f"{matrix} in: max |Q16 - float64| = {int(d.max())} level, {100 * float((d != 0).mean()):.3f} % of {d.size} samples differ")
    assert d.max() <= 1


def test_value_errors(R):
    ok = np.zeros((9, 8), np.uint16)
    assert R.yuv420p10_to_rgb_np(ok).shape == (6, 8, 3)
    for bad in (np.zeros((8, 8), np.uint16), np.zeros((9, 7), np.uint16), np.zeros((9, 8), np.uint8), np.zeros((9, 8), np.int16),
                np.zeros((9, 8), np.float32), np.zeros((8,), np.uint16)):
        with pytest.raises(ValueError):
            R.yuv420p10_to_rgb_np(bad)
    rgb = np.zeros((4, 6, 3), np.uint16)
    assert R.rgb_to_yuv420p10_np(rgb).shape == (6, 6)
    for bad in (np.zeros((3, 6, 3), np.uint16), np.zeros((4, 5, 3), np.uint16), np.zeros((4, 6), np.uint16), np.zeros((4, 6, 3), np.uint8),
                np.zeros((4, 6, 4), np.uint16)):
        with pytest.raises(ValueError):
            R.rgb_to_yuv420p10_np(bad)
    over = rgb.copy()
    over[1, 2, 0] = 1024
    with pytest.raises(ValueError, match="1023"):
        R.rgb_to_yuv420p10_np(over)
    for fn, arg in ((R.yuv420p10_to_rgb_np, ok), (R.rgb_to_yuv420p10_np, rgb)):
        for layout in ("i420", "nv12", "yuv420p10le", "P010"):                      # the 8-bit names are another path's
            with pytest.raises(ValueError, match="layout"):
                fn(arg, layout)
        with pytest.raises(ValueError, match="matrix"):
            fn(arg, "p010", "bt2020")


def test_symbols_exported_declared_and_bound(R):
    lib = C.CDLL(R._lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "resr.h")).read()
    declared = set(re.findall(r"\b(resr_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in declared, name
        assert name in R._lib.exported_symbols(), name
        assert R._lib._PROTOS[name][1][-2] == C.POINTER(R._lib.YuvDesc)
    assert "RESR_YUV_I420P10 = 2" in hdr and "RESR_YUV_P010 = 3" in hdr
    assert (R._lib.YUV_I420P10, R._lib.YUV_P010) == (2, 3) and C.sizeof(R._lib.YuvDesc) == 19 * 4       # the same 76-byte struct
    d = R.frames.yuv10_desc("p010", "bt709")
    fq, iq = R.yuv420p10_tables("bt709")
    assert d.layout == 3 and list(d.fq) == fq.reshape(-1).tolist() and list(d.iq) == iq.reshape(-1).tolist()
    assert R.frames.yuv10_desc("i420p10", "bt601").layout == 2


def test_package_exports(R):
    for name in ("yuv420p10_tables", "yuv420p10_to_rgb_np", "rgb_to_yuv420p10_np", "from_yuv420p10", "to_yuv420p10", "upscale_yuv420p10"):
        assert hasattr(R, name) and name in R.__all__ and name in R.frames.__all__, name
        assert getattr(R, name) is getattr(R.frames, name)
    assert callable(R.SRVGGNetCompact.forward_yuv420p10)


SIGNATURES = {        # recorded from the commit before the pixel-format table: the public surface did not move with it
    "yuv420_tables": "(matrix: 'str' = 'bt601', quantised: 'bool' = True) -> 'Tuple[np.ndarray, np.ndarray]'",
    "yuv420_to_rgb_np": "(frames: 'np.ndarray', layout: 'str' = 'i420', matrix: 'str' = 'bt601') -> 'np.ndarray'",
    "rgb_to_yuv420_np": "(rgb: 'np.ndarray', layout: 'str' = 'i420', matrix: 'str' = 'bt601') -> 'np.ndarray'",
    "yuv420_to_rgb": "(frames: 'torch.Tensor', layout: 'str' = 'i420', matrix: 'str' = 'bt601') -> 'torch.Tensor'",
    "rgb_to_yuv420": "(rgb: 'torch.Tensor', layout: 'str' = 'i420', matrix: 'str' = 'bt601') -> 'torch.Tensor'",
    "upscale_yuv420": "(model, frames: 'torch.Tensor', layout: 'str' = 'i420', matrix: 'str' = 'bt601', halo: 'Optional[int]' = None, "
                      "outscale: 'Optional[float]' = None, plan=None) -> 'torch.Tensor'",
    "yuv420p10_tables": "(matrix: 'str' = 'bt601', quantised: 'bool' = True) -> 'Tuple[np.ndarray, np.ndarray]'",
    "yuv420p10_to_rgb_np": "(frames: 'np.ndarray', layout: 'str' = 'i420p10', matrix: 'str' = 'bt601') -> 'np.ndarray'",
    "rgb_to_yuv420p10_np": "(rgb: 'np.ndarray', layout: 'str' = 'i420p10', matrix: 'str' = 'bt601') -> 'np.ndarray'",
    "from_yuv420p10": "(frames: 'torch.Tensor', layout: 'str' = 'i420p10', matrix: 'str' = 'bt601') -> 'torch.Tensor'",
    "to_yuv420p10": "(sr: 'torch.Tensor', layout: 'str' = 'i420p10', matrix: 'str' = 'bt601') -> 'torch.Tensor'",
    "upscale_yuv420p10": "(model, frames: 'torch.Tensor', layout: 'str' = 'i420p10', matrix: 'str' = 'bt601', halo: 'Optional[int]' = None, "
                         "outscale: 'Optional[float]' = None, plan=None) -> 'torch.Tensor'",
}
FORWARD_SIGNATURES = {
    "forward_u8": "(self, frames: 'torch.Tensor', outscale: 'Optional[float]' = None, plan=None) -> 'torch.Tensor'",
    "forward_yuv420": "(self, frames: 'torch.Tensor', layout: 'str' = 'i420', matrix: 'str' = 'bt601', outscale: 'Optional[float]' = None, "
                      "plan=None) -> 'torch.Tensor'",
    "forward_yuv420p10": "(self, frames: 'torch.Tensor', layout: 'str' = 'i420p10', matrix: 'str' = 'bt601', "
                         "outscale: 'Optional[float]' = None, plan=None) -> 'torch.Tensor'",
}


def test_pixel_formats_are_one_table(R):
    table = R.frames.PIXEL_FORMATS
    assert R.FrameStream.PIX_FMTS == tuple(table) == ("rgb24", "i420", "nv12", "i420p10", "p010")
    yuv = {name: f for name, f in table.items() if f.layout is not None}
    assert R.frames.YUV_LAYOUTS == {name: f.layout for name, f in yuv.items() if f.bits == 8} and list(R.frames.YUV_LAYOUTS) == ["i420", "nv12"]
    assert R.frames.YUV10_LAYOUTS == {name: f.layout for name, f in yuv.items() if f.bits == 10} and list(R.frames.YUV10_LAYOUTS) == list(LAYOUTS)
    hdr = open(os.path.join(ROOT, "include", "resr.h")).read()
    ids = {name: int(value) for name, value in re.findall(r"\b(RESR_YUV_[A-Z0-9]+) = (\d+)", hdr)}
    assert sorted(ids) == ["RESR_YUV_I420", "RESR_YUV_I420P10", "RESR_YUV_NV12", "RESR_YUV_P010"]
    for name, f in yuv.items():
        assert f.layout == ids["RESR_YUV_" + name.upper()], name
        assert (f.bits, f.top) == ((10, 1023) if name in LAYOUTS else (8, 255)), name
        assert f.semi_planar == (name in ("nv12", "p010")) and f.high_bits == (name == "p010"), name
        assert (f.np_dtype, f.torch_dtype) == ((np.uint16, torch.uint16) if f.bits == 10 else (np.uint8, torch.uint8)), name
    rgb = table["rgb24"]
    assert (rgb.layout, rgb.bits, rgb.top, rgb.np_dtype, rgb.torch_dtype) == (None, 8, 255, np.uint8, torch.uint8)
    with pytest.raises(AttributeError):                               # a record is immutable
        rgb.bits = 10
    for name, want in SIGNATURES.items():
        assert str(inspect.signature(getattr(R.frames, name))) == want, name
    for name, want in FORWARD_SIGNATURES.items():
        assert str(inspect.signature(getattr(R.SRVGGNetCompact, name))) == want, name


def _fake(nbytes=128):
    """A host buffer standing in for a device pointer: the calls below return before they would launch anything."""
    buf = (C.c_uint8 * nbytes)()
    base = C.addressof(buf)
    return buf, C.c_void_p((base + 31) // 32 * 32)


def test_c_abi_argument_checks_need_no_gpu(R):
    L = R._lib
    lib = L.lib()
    keep, p = _fake()
    ok = R.frames.yuv10_desc("i420p10", "bt601")
    for fn in (lib.resr_yuv420p10_to_nchw, lib.resr_nchw_to_yuv420p10):
        for n, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, 3, 4), (1, 4, 5), (1, 6, 3)):
            assert fn(p, p, n, h, w, C.byref(ok), None) == ERR_ARG, (n, h, w)
        assert fn(None, p, 1, 4, 4, C.byref(ok), None) == ERR_ARG
        assert fn(p, None, 1, 4, 4, C.byref(ok), None) == ERR_ARG
        assert fn(p, p, 1, 4, 4, None, None) == ERR_ARG
        for layout in (0, 1, 4, 7):                                   # the 8-bit layouts are not these entries'
            assert fn(p, p, 1, 4, 4, C.byref(L.YuvDesc(layout, ok.fq, ok.iq)), None) == ERR_ARG
            assert b"layout" in lib.resr_last_error()
    assert lib.resr_nchw_to_yuv420p10(p, C.c_void_p(p.value + 2), 1, 4, 4, C.byref(ok), None) == ERR_ARG     # w % 4 == 0: 8-byte stores
    assert b"aligned" in lib.resr_last_error()
    assert lib.resr_nchw_to_yuv420p10(C.c_void_p(p.value + 4), p, 1, 4, 4, C.byref(ok), None) == ERR_ARG     # ... and 16-byte loads
    assert lib.resr_nchw_to_yuv420p10(p, C.c_void_p(p.value + 1), 1, 4, 6, C.byref(ok), None) == ERR_ARG     # a word is 2 bytes
    # ... and the 8-bit entries refuse a 10-bit descriptor
    assert lib.resr_yuv420_to_rgb(p, p, 1, 4, 4, C.byref(ok), None) == ERR_ARG
    good = L.CompactDesc(1, 8, 8, 16, 4, 0, L.RESR_F16, 0)
    ws = lib.resr_compact_workspace_bytes(C.byref(good))
    assert lib.resr_compact_forward_yuv420(C.byref(good), p, p, p, p, ws, p, C.byref(ok), None) == ERR_ARG
    fwd = lib.resr_compact_forward_yuv420p10
    assert fwd(None, p, p, p, p, ws, p, C.byref(ok), None) == ERR_ARG
    for hole in range(5):                                          # x_yuv, params, packed, workspace, y_yuv
        a = [p] * 5
        a[hole] = None
        assert fwd(C.byref(good), a[0], a[1], a[2], a[3], ws, a[4], C.byref(ok), None) == ERR_ARG, hole
        assert b"null" in lib.resr_last_error()
    assert fwd(C.byref(good), p, p, p, p, ws, p, None, None) == ERR_ARG
    for layout in (0, 1, 7):
        assert fwd(C.byref(good), p, p, p, p, ws, p, C.byref(L.YuvDesc(layout, ok.fq, ok.iq)), None) == ERR_ARG
        assert b"layout" in lib.resr_last_error()
    for h, w in ((7, 8), (8, 7), (1, 1)):
        assert fwd(C.byref(L.CompactDesc(1, h, w, 16, 4, 0, L.RESR_F16, 0)), p, p, p, p, 1 << 40, p, C.byref(ok), None) == ERR_ARG
        assert b"even" in lib.resr_last_error()
    for off in (2, 8):                                             # output width 32: 16-byte stores; one sample off, half a store off
        assert fwd(C.byref(good), p, p, p, p, ws, C.c_void_p(p.value + off), C.byref(ok), None) == ERR_ARG
        assert b"aligned" in lib.resr_last_error()
    assert fwd(C.byref(good), p, p, p, p, ws - 1, p, C.byref(ok), None) == ERR_WORKSPACE   # nothing more than the float path's
    del keep


def test_frame_stream_argument_checks(R):
    cpu_model = R.SRVGGNetCompact(num_conv=1, precision="fast")
    assert R.FrameStream.PIX_FMTS == ("rgb24", "i420", "nv12", "i420p10", "p010")
    for pix_fmt in ("yuv420p10le", "p010le", "yuv420p10", "P010", "i420p12"):
        with pytest.raises(ValueError, match="pix_fmt"):
            R.FrameStream(cpu_model, pix_fmt=pix_fmt)
    with pytest.raises(ValueError, match="matrix"):
        R.FrameStream(cpu_model, pix_fmt="p010", matrix="bt2020")
    for pix_fmt in LAYOUTS:
        with pytest.raises(RuntimeError, match="no CPU path"):          # names accepted: the device is what is missing
            R.FrameStream(cpu_model, pix_fmt=pix_fmt)
    ok = np.zeros((9, 8), np.uint16)
    R.FrameStream.check_frame_yuv420p10(ok)
    for bad in (np.zeros((8, 8), np.uint16), np.zeros((9, 7), np.uint16), np.zeros((0, 8), np.uint16), ok.astype(np.uint8),
                ok.astype(np.float32), np.zeros((9, 8, 3), np.uint16), ok[None], torch.zeros(9, 8, dtype=torch.uint16), [[1, 2]]):
        with pytest.raises(ValueError, match="uint16"):
            R.FrameStream.check_frame_yuv420p10(bad)
    R.FrameStream.check_frame_yuv420(np.zeros((9, 8), np.uint8))      # the 8-bit check is what it was


def test_device_functions_refuse_cpu_tensors(R):
    f = torch.zeros(1, 6, 4, dtype=torch.uint16)
    m = R.SRVGGNetCompact(num_conv=1, precision="fast")
    with torch.no_grad():
        for call in (lambda: R.from_yuv420p10(f), lambda: R.to_yuv420p10(torch.zeros(1, 3, 4, 4)),
                     lambda: R.upscale_yuv420p10(m, f), lambda: m.forward_yuv420p10(f)):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call()
        with pytest.raises(ValueError, match="layout"):
            m.forward_yuv420p10(f, layout="nv12")
        with pytest.raises(ValueError, match="layout"):
            R.upscale_yuv420p10(m, f, layout="i420")
        with pytest.raises(ValueError, match="matrix"):
            R.upscale_yuv420p10(m, f, matrix="bt2020")
    with pytest.raises(RuntimeError, match="backward"):
        m.forward_yuv420p10(f)


def test_inference_rawvideo_parser_reader_and_byte_counts(R):
    from real_esrgan_pytorch_amd import inference_rawvideo as V
    p = V.get_parser()
    for name, layout in (("yuv420p10le", "i420p10"), ("p010le", "p010")):
        a = p.parse_args(["--input", "I", "--output", "O", "--size", "8x6", "--weights_path", "W", "--pix_fmt", name])
        assert a.pix_fmt == name and V.PIX_FMTS[name] == layout and V.WORD[layout].itemsize == 2
    for bad in ("yuv420p10", "p010", "yuv420p10be", "yuv420p12le"):
        with pytest.raises(SystemExit):
            p.parse_args(["--input", "I", "--output", "O", "--size", "8x6", "--weights_path", "W", "--pix_fmt", bad])
    # an unknown name is refused by main() before a device, a model or a file is touched
    args = types.SimpleNamespace(input="/nonexistent/in", output="/nonexistent/out", size="8x6", pix_fmt="yuv420p16le", matrix="bt601",
                                 weights_path="/nonexistent/w")
    with pytest.raises(ValueError, match="pix_fmt"):
        V.main(args)
    assert V.parse_size("1920x1080") == (1920, 1080)
    assert V.frame_bytes(8, 6) == 72 and V.frame_bytes(8, 6, V.WORD["i420p10"]) == 8 * 6 * 3 == 144
    assert V.frame_bytes(1920, 1080, V.WORD["p010"]) == 1920 * 1080 * 3 and V.frame_bytes(7680, 4320, V.WORD["p010"]) == 99532800
    words = np.arange(144, dtype="<u2") * 257                          # two 8x6 frames of 72 words = 144 bytes each
    raw = words.tobytes()
    got = list(V.read_frames(io.BytesIO(raw), 8, 6, V.WORD["i420p10"]))
    assert len(got) == 2 and got[0].shape == (9, 8) and got[0].dtype == np.uint16
    assert np.array_equal(np.concatenate(got).reshape(-1), words) and got[1].astype("<u2").tobytes() == raw[144:]
    assert raw[2:4] == bytes([1, 1]) and int(got[0][0, 1]) == 257 and int(got[0][0, 2]) == 514    # little-endian words
    assert list(V.read_frames(io.BytesIO(b""), 8, 6, V.WORD["p010"])) == []
    with pytest.raises(ValueError, match="frame 2: 31 trailing bytes.* has 144"):
        list(V.read_frames(io.BytesIO(raw + bytes(31)), 8, 6, V.WORD["p010"]))
    with pytest.raises(ValueError, match="72 trailing bytes"):          # one 8-bit frame is half a 10-bit one
        list(V.read_frames(io.BytesIO(raw[:72]), 8, 6, V.WORD["i420p10"]))
