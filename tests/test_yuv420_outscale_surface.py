"""CPU: the surface of the fused YUV outscale tail -- the two C-ABI entries and the query (exported, declared, bound), every refusal
before a launch, the query against the LDS arithmetic of csrc/image_resize.hip restated here, and the Python checks of the new
`outscale` argument of `SRVGGNetCompact.forward_yuv420` / `forward_yuv420p10`.  Nothing here touches a device."""
import ctypes as C
import inspect
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("resr_compact_forward_yuv420_scaled", "resr_compact_forward_yuv420p10_scaled")
QUERY = "resr_compact_yuv420_scaled_fits"
ERR_ARG, ERR_WORKSPACE = -1, -3          # include/resr.h resr_status
LDS_BUDGET = 64 * 1024


@pytest.fixture(scope="module")
def R():
    import __graft_entry__
    __graft_entry__.build()
    import real_esrgan_pytorch_amd as R
    return R


def test_symbols_exported_declared_and_bound(R):
    lib = C.CDLL(R._lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "resr.h")).read()
    declared = set(re.findall(r"\b(resr_[a-z0-9_]+)\s*\(", hdr))
    for name in ENTRIES + (QUERY,):
        assert hasattr(lib, name), name
        assert name in declared, name
        assert name in R._lib.exported_symbols(), name
    for name in ENTRIES:
        assert R._lib._PROTOS[name][1][-2] == C.POINTER(R._lib.YuvDesc) and len(R._lib._PROTOS[name][1]) == 17
    assert R._lib._PROTOS[QUERY] == (C.c_int, [C.c_int32] * 8)
    assert R._lib.lib().resr_version() == 3 and R._lib.RESR_VERSION == 3
    assert re.search(r"#define RESR_VERSION 3\b", hdr)
    for method in (R.SRVGGNetCompact.forward_yuv420, R.SRVGGNetCompact.forward_yuv420p10):
        params = inspect.signature(method).parameters
        assert params["outscale"].default is None and params["plan"].default is None


def _fake(nbytes=128):
    """A host buffer standing in for a device pointer: the calls below return before they would launch anything."""
    buf = (C.c_uint8 * nbytes)()
    base = C.addressof(buf)
    return buf, C.c_void_p((base + 31) // 32 * 32)


@pytest.mark.parametrize("bits", (8, 10))
def test_c_abi_refusals_need_no_gpu(R, bits):
    L = R._lib
    lib = L.lib()
    keep, p = _fake()
    fwd = getattr(lib, ENTRIES[bits == 10])
    ok = R.frames.yuv10_desc("p010", "bt601") if bits == 10 else R.frames.yuv_desc("nv12", "bt601")
    other = R.frames.yuv_desc("i420", "bt601") if bits == 10 else R.frames.yuv10_desc("i420p10", "bt601")
    good = L.CompactDesc(1, 8, 8, 16, 4, 0, L.RESR_F16, 0)
    ws = lib.resr_compact_workspace_bytes(C.byref(good))
    assert ws > 0

    def call(desc=good, a=(p, p, p, p), wsb=None, y=p, oh=16, ow=16, tabs=(p, p, p, p), ty=10, tx=10, yuv=ok):
        d = C.byref(desc) if desc is not None else None
        q = C.byref(yuv) if yuv is not None else None
        return fwd(d, a[0], a[1], a[2], a[3], ws if wsb is None else wsb, y, oh, ow, tabs[0], tabs[1], ty, tabs[2], tabs[3], tx, q, None)

    def refused(word, **kw):
        assert call(**kw) == ERR_ARG, kw
        msg = lib.resr_last_error()
        assert msg and word in msg, (kw, msg)

    for h, w in ((7, 8), (8, 7)):                                    # an odd LR frame
        refused(b"even", desc=L.CompactDesc(1, h, w, 16, 4, 0, L.RESR_F16, 0), wsb=1 << 40)
    for kw in (dict(oh=15), dict(ow=15), dict(oh=17, ow=17)):        # an odd result
        refused(b"even", **kw)
    refused(b"layout", yuv=other)                                    # a descriptor of the other bit depth
    for layout in (4, 7, -1):
        refused(b"layout", yuv=L.YuvDesc(layout, ok.fq, ok.iq))
    refused(b"null", yuv=None)
    refused(b"descriptor", desc=None)
    for hole in range(4):                                            # x_yuv, params, packed, workspace
        a = [p] * 4
        a[hole] = None
        refused(b"null", a=a)
    refused(b"null", y=None)
    for hole in range(4):                                            # idx_y, w_y, idx_x, w_x
        t = [p] * 4
        t[hole] = None
        refused(b"null", tabs=t)
    for off in (1, 2, 3) if bits == 8 else (2,):                     # rows leave as dwords
        refused(b"aligned", y=C.c_void_p(p.value + off))
    for kw in (dict(ty=0), dict(tx=0), dict(ty=4097), dict(tx=5000), dict(ty=-3)):
        refused(b"taps", **kw)
    for kw in (dict(oh=0), dict(ow=0), dict(oh=-4)):
        refused(b"shape", **kw)
    for bad in (L.CompactDesc(0, 8, 8, 16, 4, 0, 0, 0), L.CompactDesc(1, 8, 8, 16, 5, 0, 0, 0), L.CompactDesc(1, 8, 8, 16, 4, 0, 7, 0)):
        refused(b"descriptor", desc=bad, wsb=1 << 40)
    big = L.CompactDesc(1, 200, 200, 16, 4, 0, L.RESR_F16, 0)        # r = 0.01 on an 800 x 800 frame: 402 taps, no tile fits
    refused(b"footprint", desc=big, wsb=1 << 40, ty=402, tx=402, oh=8, ow=8)
    # everything in order: the last check is the workspace, as for every other entry (nothing is launched with fake pointers)
    assert call(wsb=ws - 1) == ERR_WORKSPACE and call(wsb=0) == ERR_WORKSPACE
    del keep


def _span_bound(t, n_in, n_out, p):
    s = p + ((t - 1) * n_in // (n_out - 1) + 2 if t > 1 else 0)
    return min(s, n_in)


def _lds_bytes(th, tw, n_in, n_out, taps, out_bytes_per_pixel):
    """csrc/image_resize.hip's lds_bytes for a square frame and one tile: tables + region + intermediate + the staging buffer."""
    rh = _span_bound(min(th, n_out), n_in, n_out, taps)
    rw = _span_bound(min(tw, n_out), n_in, n_out, taps)
    pitch = rw | 1
    floats = 2 * (th * taps + tw * taps) + 3 * (rh + th) * pitch
    return floats * 4 + (th * tw * out_bytes_per_pixel + 3) // 4 * 4


def test_query(R):
    L = R._lib
    lib = L.lib()
    fits = lib.resr_compact_yuv420_scaled_fits
    # 1080p through the x4 model at outscale 2: r = 0.5, 10 taps, the 16 x 32 tile of the RGB tail
    from real_esrgan_pytorch_amd import imgproc
    assert imgproc.resize_band_tables(4320, 2160, 0.5)[0].shape[1] == 10
    for bits in (8, 10):
        assert fits(1080, 1920, 4, 2160, 3840, 10, 10, bits) == 1
    assert _lds_bytes(16, 32, 4320, 2160, 10, 6) <= LDS_BUDGET < _lds_bytes(32, 32, 4320, 2160, 10, 6)
    # bad arguments are a plain no
    for args in ((1081, 1920, 4, 2160, 3840, 10, 10, 8), (1080, 1920, 4, 2161, 3840, 10, 10, 8), (1080, 1920, 4, 2160, 3840, 10, 10, 12),
                 (1080, 1920, 5, 2160, 3840, 10, 10, 8), (1080, 1920, 4, 2160, 3840, 0, 10, 8), (0, 1920, 4, 2160, 3840, 10, 10, 10)):
        assert fits(*args) == 0, args
    # an r whose 2x2 footprint exceeds 64 KB while one output pixel of the RGB tail still fits: found from the LDS arithmetic
    lr, s = 2000, 4
    hr = lr * s
    found = None
    for out in range(hr // 2, 2, -2):
        r = out / hr
        if math.ceil(hr * r) != out:
            continue
        taps = math.ceil(4 / r) + 2
        if _lds_bytes(2, 2, hr, out, taps, 3) > LDS_BUDGET and _lds_bytes(1, 1, hr, out, taps, 3) <= LDS_BUDGET:
            found = (out, taps)
            break
    assert found is not None
    out, taps = found
    assert _lds_bytes(2, 2, hr, out, taps, 6) > LDS_BUDGET
    for bits in (8, 10):
        assert fits(lr, lr, s, out, out, taps, taps, bits) == 0
    # ... the RGB entry plans it (it gets as far as the workspace check), the YUV entries refuse it
    keep, p = _fake()
    desc = L.CompactDesc(1, lr, lr, 16, s, 0, L.RESR_F16, 0)
    assert lib.resr_compact_forward_u8_scaled(C.byref(desc), p, p, p, p, 0, p, out, out, p, p, taps, p, p, taps, None) == ERR_WORKSPACE
    ok = R.frames.yuv_desc("i420", "bt601")
    assert lib.resr_compact_forward_yuv420_scaled(C.byref(desc), p, p, p, p, 0, p, out, out, p, p, taps, p, p, taps, C.byref(ok), None) == ERR_ARG
    assert b"footprint" in lib.resr_last_error() and b"2x2" in lib.resr_last_error()
    # one tap fewer per pixel row and the 2 x 2 tile is back: the query follows the arithmetic on both sides of the threshold
    for o2 in range(out + 2, out + 200, 2):
        t2 = math.ceil(4 / (o2 / hr)) + 2
        want = int(_lds_bytes(2, 2, hr, o2, t2, 6) <= LDS_BUDGET)
        assert fits(lr, lr, s, o2, o2, t2, t2, 10) == want, (o2, t2)
    del keep


def test_python_value_errors_come_first(R):
    m = R.SRVGGNetCompact(num_conv=1, precision="fast")
    f8, f10 = torch.zeros(1, 18, 18, dtype=torch.uint8), torch.zeros(1, 18, 18, dtype=torch.uint16)     # 12 x 18 luma
    assert R.output_size(12, 18, 4, 2.5) == (30, 45)
    with torch.no_grad():
        for fwd, up, f in ((m.forward_yuv420, R.upscale_yuv420, f8), (m.forward_yuv420p10, R.upscale_yuv420p10, f10)):
            for bad in (0, -2.0, float("nan"), float("inf"), True, "2"):
                with pytest.raises(ValueError, match="outscale"):
                    fwd(f, outscale=bad)
            with pytest.raises(ValueError, match="even"):            # 30 x 45: no 4:2:0 frame
                fwd(f, outscale=2.5)
            for o in (2, None, 4):                                   # a valid outscale reaches the device check
                with pytest.raises(RuntimeError, match="no CPU path"):
                    fwd(f, outscale=o)
                with pytest.raises(RuntimeError, match="no CPU path"):
                    up(m, f, outscale=o)
        with pytest.raises(ValueError, match="layout"):
            m.forward_yuv420(f8, "p010", outscale=2)
        with pytest.raises(ValueError, match="layout"):
            m.forward_yuv420p10(f10, "nv12", outscale=2)
