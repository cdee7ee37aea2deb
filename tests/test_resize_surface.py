"""CPU: the surface of outscale -- the two new C-ABI entries (exported, declared, argument checks before any launch), the banded
tap tables against `imgproc._resize_matrix` and against the reference's own outputs (tests/golden/image_resize_native.npz, written
by tests/golden/gen_resize_golden.py), `frames.output_size`, and the Python argument checks.  Nothing here touches a device."""
import ctypes as C
import hashlib
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("resr_image_resize", "resr_compact_forward_u8_scaled", "resr_compact_forward_u8")
ERR_ARG, ERR_WORKSPACE = -1, -3          # include/resr.h resr_status


@pytest.fixture(scope="module")
def R():
    import __graft_entry__
    __graft_entry__.build()
    import real_esrgan_pytorch_amd as R
    return R


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "image_resize_native.npz"))


def test_symbols_exported_declared_and_bound(R):
    lib = C.CDLL(R._lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "resr.h")).read()
    declared = set(re.findall(r"\b(resr_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in declared, name
        assert name in R._lib.exported_symbols(), name
    assert R._lib.lib().resr_version() == 3 and R._lib.RESR_VERSION == 3
    assert re.search(r"#define RESR_VERSION 3\b", hdr)


def test_package_exports(R):
    from real_esrgan_pytorch_amd import imgproc
    assert R.output_size is R.frames.output_size and "output_size" in R.__all__
    for name in ("image_resize_native", "resize_band_tables", "ResizePlan"):
        assert hasattr(imgproc, name) and name in imgproc.__all__, name
    import inspect
    assert "outscale" in inspect.signature(R.SRVGGNetCompact.forward_u8).parameters
    assert "outscale" in inspect.signature(R.upscale_u8).parameters
    assert "outscale" in inspect.signature(R.FrameStream.__init__).parameters
    assert inspect.signature(R.upscale_u8).parameters["outscale"].default is None


def _fake(nbytes=64):
    """A host buffer standing in for a device pointer: the calls below return before they would launch anything."""
    buf = (C.c_uint8 * nbytes)()
    return buf, C.cast(buf, C.c_void_p)


def test_image_resize_argument_checks_need_no_gpu(R):
    lib = R._lib.lib()
    keep, p = _fake()

    def call(src=p, dst=p, n=1, c=3, h=8, w=8, oh=4, ow=4, iy=p, wy=p, ty=10, ix=p, wx=p, tx=10, u8=0):
        return lib.resr_image_resize(src, dst, n, c, h, w, oh, ow, iy, wy, ty, ix, wx, tx, u8, None)

    for kw in (dict(src=None), dict(dst=None), dict(iy=None), dict(wy=None), dict(ix=None), dict(wx=None)):      # null pointers
        assert call(**kw) == ERR_ARG, kw
        assert b"null" in lib.resr_last_error()
    for kw in (dict(n=0), dict(c=0), dict(h=0), dict(w=-1), dict(oh=0), dict(ow=-3), dict(ty=0), dict(tx=0), dict(ty=4097), dict(tx=-2),
               dict(n=65536), dict(n=30000, c=7)):
        assert call(**kw) == ERR_ARG, kw
    assert call(c=4, u8=1) == ERR_ARG                                # uint8 output is HWC with 3 channels
    assert call(dst=C.c_void_p(p.value + 1), u8=1) == ERR_ARG        # ... stored as dwords
    assert b"aligned" in lib.resr_last_error()
    # a scale whose single-pixel footprint does not fit the LDS tile is refused, not routed elsewhere: r = 0.01 has 402 taps
    assert call(h=4000, w=4000, oh=40, ow=40, ty=402, tx=402) == ERR_ARG
    assert b"footprint" in lib.resr_last_error()
    del keep


def test_compact_forward_u8_scaled_argument_checks_need_no_gpu(R):
    L = R._lib
    lib = L.lib()
    keep, p = _fake()
    good = L.CompactDesc(1, 8, 8, 16, 4, 0, L.RESR_F16, 0)
    ws = lib.resr_compact_workspace_bytes(C.byref(good))
    assert ws > 0

    def call(desc=good, a=(p, p, p, p), wsb=None, y=p, oh=16, ow=16, tabs=(p, p, p, p), ty=10, tx=10):
        d = C.byref(desc) if desc is not None else None
        return lib.resr_compact_forward_u8_scaled(d, a[0], a[1], a[2], a[3], ws if wsb is None else wsb, y, oh, ow,
                                                  tabs[0], tabs[1], ty, tabs[2], tabs[3], tx, None)

    for bad in (L.CompactDesc(0, 8, 8, 16, 4, 0, 0, 0), L.CompactDesc(1, 8, 8, 16, 5, 0, 0, 0), L.CompactDesc(1, 8, 8, 16, 4, 3, 0, 0),
                L.CompactDesc(1, 8, 8, 16, 4, 0, 7, 0), L.CompactDesc(1, 8, 8, -1, 4, 0, 0, 0),
                L.CompactDesc(1, 8192, 4096, 16, 4, 0, L.RESR_F16X2, 0)):
        assert call(desc=bad, wsb=1 << 40) == ERR_ARG
        assert b"descriptor" in lib.resr_last_error()
    assert call(desc=None) == ERR_ARG
    for hole in range(4):                                            # x_u8, params, packed, workspace
        a = [p] * 4
        a[hole] = None
        assert call(a=a) == ERR_ARG, hole
        assert b"null" in lib.resr_last_error()
    assert call(y=None) == ERR_ARG
    for hole in range(4):                                            # idx_y, w_y, idx_x, w_x
        t = [p] * 4
        t[hole] = None
        assert call(tabs=t) == ERR_ARG, hole
        assert b"null" in lib.resr_last_error()
    for kw in (dict(oh=0), dict(ow=0), dict(oh=-4), dict(ty=0), dict(tx=0), dict(tx=5000)):
        assert call(**kw) == ERR_ARG, kw
    assert call(y=C.c_void_p(p.value + 2)) == ERR_ARG
    big = L.CompactDesc(1, 200, 200, 16, 4, 0, L.RESR_F16, 0)       # r = 0.01 on an 800 x 800 frame: 402 taps, no tile fits: refused
    assert call(desc=big, wsb=1 << 40, ty=402, tx=402, oh=8, ow=8) == ERR_ARG
    assert b"footprint" in lib.resr_last_error()
    assert call(wsb=ws - 1) == ERR_WORKSPACE and call(wsb=0) == ERR_WORKSPACE
    assert lib.resr_compact_workspace_bytes(C.byref(good)) == ws     # this path plans nothing of its own
    del keep


def _dense(idx, w, in_length):
    m = np.zeros((idx.shape[0], in_length), np.float32)
    np.add.at(m, (np.repeat(np.arange(idx.shape[0]), idx.shape[1]), idx.reshape(-1).astype(np.int64)), w.reshape(-1))
    return m


def test_band_tables_are_the_resize_matrix(R, golden):
    from real_esrgan_pytorch_amd import imgproc
    lengths = set()
    for h, w, r in golden["cases"]:
        lengths.update([(int(h), float(r)), (int(w), float(r))])
    assert len(lengths) >= 14
    for n, r in sorted(lengths):
        for aa in (True, False):
            out = math.ceil(n * r)
            idx, w = imgproc.resize_band_tables(n, out, r, aa)
            p = math.ceil(4 / min(r, 1) if aa else 4) + 2
            assert idx.shape == w.shape == (out, p) and idx.dtype == np.int32 and w.dtype == np.float32, (n, r, aa)
            assert idx.min() >= 0 and idx.max() < n
            m = imgproc._resize_matrix(n, out, r, aa)
            assert np.array_equal(_dense(idx, w, n), m), (n, r, aa)


def test_resize_matrix_kept_its_parent_values(R, golden):
    from real_esrgan_pytorch_amd import imgproc
    for (n, r, aa), sha in zip(golden["matrix_keys"], golden["matrix_sha256"]):
        n, aa = int(n), bool(aa)
        m = imgproc._resize_matrix(n, math.ceil(n * r), float(r), aa)
        assert m.dtype == np.float32 and hashlib.sha256(m.tobytes()).hexdigest() == str(sha), (n, r, aa)
    assert np.array_equal(imgproc._resize_matrix(8, 3, 0.375, True), golden["matrix_8_0375"])
    assert np.array_equal(imgproc._resize_matrix(4, 2, 0.5, True), golden["matrix_4_05"])
    m64 = imgproc._resize_matrix(16, 8, 0.5, True, np.float64)       # NIQE's form is still served
    assert m64.dtype == np.float64 and np.allclose(m64.sum(1), 1.0)


def test_builder_raises_exactly_where_the_reference_raises(R, golden):
    from real_esrgan_pytorch_amd import imgproc
    table = golden["raise_table"]
    assert len(table) >= 500 and 0 < table[:, 2].sum() < len(table)
    for n, r, raised in table:
        n, r = int(n), float(r)
        try:
            imgproc.resize_band_tables(n, math.ceil(n * r), r)
            got = False
        except ValueError:
            got = True
        assert got == bool(raised), (n, r, raised)
    for h, w, r in ((2, 8, 0.5), (3, 3, 0.5), (4, 12, 0.375)):      # the issue's examples, through the plan the launches use
        with pytest.raises(ValueError, match="shorter than the symmetric copy"):
            imgproc.ResizePlan(h, w, r, "cpu")


def _restate(x, r):
    """Section 1 of the definition in numpy: per axis sequential fp32 accumulation over the tables, H pass first."""
    from real_esrgan_pytorch_amd import imgproc
    _, h, w = x.shape
    iy, wy = imgproc.resize_band_tables(h, math.ceil(h * r), r)
    ix, wx = imgproc.resize_band_tables(w, math.ceil(w * r), r)
    mid = np.zeros((3, iy.shape[0], w), np.float32)
    for k in range(iy.shape[1]):
        mid = (mid + x[:, iy[:, k], :] * wy[None, :, k, None]).astype(np.float32)
    out = np.zeros((3, iy.shape[0], ix.shape[0]), np.float32)
    for k in range(ix.shape[1]):
        out = (out + mid[:, :, ix[:, k]] * wx[None, None, :, k]).astype(np.float32)
    return out


def test_definition_restated_in_numpy_meets_the_reference(R, golden):
    want = {(120, 152, 0.5), (117, 150, 0.75), (92, 100, 0.375), (60, 76, 0.625), (40, 52, 1.5), (4, 4, 0.5), (8, 8, 0.375), (2, 2, 1.5),
            (3, 40, 0.625)}
    assert want <= {(int(h), int(w), float(r)) for h, w, r in golden["cases"]}
    for i, (h, w, r) in enumerate(golden["cases"]):
        x, ref = golden[f"in_{i}"], golden[f"out_{i}"]
        assert x.dtype == np.float32 and x.shape == (3, int(h), int(w))
        got = _restate(x, float(r))
        assert got.shape == ref.shape
        err = float(np.abs(got - ref).max())
        print(f"case {int(h)}x{int(w)} x {r}: max |restatement - reference| = {err:.3e}")
        assert err <= 1e-6, (h, w, r, err)
    big = golden["in_0"]
    assert big.min() < -0.05 and big.max() > 1.05                    # the inputs overshoot [0, 1] as an unclamped SR output does


def test_output_size(R):
    for h, s, o in ((1080, 4, 2), (1080, 4, 1.5), (1080, 4, 3), (1080, 4, 2.5), (37, 3, 2), (37, 3, 1.5), (37, 3, 2.5), (5, 3, 4), (7, 2, 3),
                    (1, 4, 2), (53, 2, 1.5), (719, 3, 2.2)):
        assert R.output_size(h, 2 * h + 1, s, o) == (math.ceil(h * s * (o / s)), math.ceil((2 * h + 1) * s * (o / s))), (h, s, o)
    assert R.output_size(1080, 1920, 4, 2) == (2160, 3840)
    assert R.output_size(1080, 1920, 4) == R.output_size(1080, 1920, 4, None) == R.output_size(1080, 1920, 4, 4) == (4320, 7680)
    assert R.output_size(10, 10, 3, 3.0) == (30, 30)
    for bad in (0, -1, float("nan"), float("inf"), True, "2", [2]):
        with pytest.raises(ValueError, match="outscale"):
            R.output_size(10, 10, 4, bad)


def test_outscale_argument_checks_come_first(R):
    cpu_model = R.SRVGGNetCompact(num_conv=1, precision="fast")
    frames = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    for bad in (0, -2.0, float("nan"), float("inf"), True, False, "2"):
        with pytest.raises(ValueError, match="outscale"):
            R.FrameStream(cpu_model, depth=2, outscale=bad)
        with pytest.raises(ValueError, match="outscale"), torch.no_grad():
            cpu_model.forward_u8(frames, outscale=bad)
    with torch.no_grad():
        for o in (2, 2.5, None, 4):                                  # a valid outscale reaches the device check, as before
            with pytest.raises(RuntimeError, match="no CPU path"):
                cpu_model.forward_u8(frames, outscale=o)
            with pytest.raises(RuntimeError, match="no CPU path"):
                R.upscale_u8(cpu_model, frames, outscale=o)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.FrameStream(cpu_model, depth=2, outscale=2)
    from real_esrgan_pytorch_amd import imgproc
    with pytest.raises(RuntimeError, match="no CPU path"):
        imgproc.image_resize_native(torch.zeros(1, 3, 8, 8), 0.5)
    # tables of the wrong length, or for another size, never reach a launch
    plan = imgproc.ResizePlan(32, 32, 0.5, "cpu")
    assert (plan.out_h, plan.out_w, plan.taps_y, plan.taps_x) == (16, 16, 10, 10)
    plan.check("ok")
    plan.w_x = plan.w_x[:-1]
    with pytest.raises(ValueError, match="tap table"):
        plan.check("short")
    plan = imgproc.ResizePlan(32, 32, 0.5, "cpu")
    plan.out_h = 17                                                  # oh that disagrees with the tables
    with pytest.raises(ValueError, match="tap table"):
        plan.check("oh")
    for bad in (0, -0.5, float("nan"), True):
        with pytest.raises(ValueError, match="scale"):
            imgproc.ResizePlan(32, 32, bad, "cpu")


def test_inference_frames_parser_outscale(R):
    from real_esrgan_pytorch_amd import inference_frames
    p = inference_frames.get_parser()
    base = ["--inputs_dir", "D", "--output_dir", "O", "--weights_path", "W"]
    assert p.parse_args(base).outscale is None
    assert p.parse_args(base + ["--outscale", "2"]).outscale == 2.0
    assert p.parse_args(base + ["--outscale", "1.5"]).outscale == 1.5
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--outscale", "two"])
