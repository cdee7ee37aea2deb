"""CPU: the surface of the uint8 frame path -- the three C-ABI entries (exported, declared, argument checks before any launch),
the package exports, FrameStream's argument checks and the directory CLI's parser.  Nothing here touches a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("resr_compact_forward_u8", "resr_u8_to_nchw", "resr_nchw_to_u8")
ERR_ARG, ERR_WORKSPACE = -1, -3          # include/resr.h resr_status


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
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in declared, name
        assert name in R._lib.exported_symbols(), name
    assert "NaN" in hdr[hdr.index("resr_compact_forward_u8") - 2500:hdr.index("resr_compact_forward_u8")]   # the contract's edge is stated


def test_package_exports(R):
    for name in ("frames", "FrameStream", "upscale_u8", "to_u8", "from_u8"):
        assert hasattr(R, name) and name in R.__all__, name
    assert R.frames.FrameStream is R.FrameStream and R.frames.upscale_u8 is R.upscale_u8
    assert callable(R.SRVGGNetCompact.forward_u8)


def _fake(nbytes=64):
    """A host buffer standing in for a device pointer: the calls below return before they would launch anything."""
    buf = (C.c_uint8 * nbytes)()
    return buf, C.cast(buf, C.c_void_p)


def test_compact_forward_u8_argument_checks_need_no_gpu(R):
    L = R._lib
    lib = L.lib()
    keep, p = _fake()
    good = L.CompactDesc(1, 8, 8, 16, 4, 0, L.RESR_F16, 0)
    ws = lib.resr_compact_workspace_bytes(C.byref(good))
    assert ws > 0
    # the `bad` list of tests/test_compact_surface.py
    for bad in (L.CompactDesc(0, 8, 8, 16, 4, 0, 0, 0), L.CompactDesc(1, 8, 8, 16, 5, 0, 0, 0), L.CompactDesc(1, 8, 8, 16, 4, 3, 0, 0),
                L.CompactDesc(1, 8, 8, 16, 4, 0, 7, 0), L.CompactDesc(1, 8, 8, -1, 4, 0, 0, 0),
                L.CompactDesc(1, 8192, 4096, 16, 4, 0, L.RESR_F16X2, 0)):
        assert lib.resr_compact_forward_u8(C.byref(bad), p, p, p, p, 1 << 40, p, None) == ERR_ARG
        assert b"descriptor" in lib.resr_last_error()
    assert lib.resr_compact_forward_u8(None, p, p, p, p, 1 << 40, p, None) == ERR_ARG
    for hole in range(5):                                          # x_u8, params, packed, workspace, y_u8
        a = [p] * 5
        a[hole] = None
        assert lib.resr_compact_forward_u8(C.byref(good), a[0], a[1], a[2], a[3], ws, a[4], None) == ERR_ARG, hole
        assert b"null" in lib.resr_last_error()
    assert lib.resr_compact_forward_u8(C.byref(good), p, p, p, p, ws - 1, p, None) == ERR_WORKSPACE
    assert lib.resr_compact_forward_u8(C.byref(good), p, p, p, p, 0, p, None) == ERR_WORKSPACE
    # the same checks, the same codes as the float entry
    assert lib.resr_compact_forward(C.byref(good), p, p, p, p, ws - 1, p, None) == ERR_WORKSPACE
    # the dword stores of the tail want a 4-byte aligned output
    odd = C.c_void_p(p.value + 1)
    assert lib.resr_compact_forward_u8(C.byref(good), p, p, p, p, ws, odd, None) == ERR_ARG
    # this path plans nothing of its own
    assert lib.resr_compact_workspace_bytes(C.byref(good)) == ws
    del keep


@pytest.mark.parametrize("name", ["resr_u8_to_nchw", "resr_nchw_to_u8"])
def test_conversion_argument_checks_need_no_gpu(R, name):
    fn = getattr(R._lib.lib(), name)
    keep, p = _fake()
    for n, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -3, 4), (1, 4, -2)):
        assert fn(p, p, n, h, w, None) == ERR_ARG, (n, h, w)
    assert fn(None, p, 1, 4, 4, None) == ERR_ARG
    assert fn(p, None, 1, 4, 4, None) == ERR_ARG
    del keep


def test_frame_stream_argument_checks(R):
    cpu_model = R.SRVGGNetCompact(num_conv=1, precision="fast")
    for depth in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="depth"):
            R.FrameStream(cpu_model, depth=depth)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.FrameStream(cpu_model, depth=2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.FrameStream(R.Generator(3, 3, 4, n_blocks=1))
    ok = np.zeros((5, 7, 3), np.uint8)
    R.FrameStream.check_frame(ok)
    for bad in (ok.astype(np.float32), ok[:, :, :2], ok[:, :, 0], np.zeros((1, 5, 7, 3), np.uint8), np.zeros((0, 7, 3), np.uint8),
                torch.zeros(5, 7, 3, dtype=torch.uint8), [[1, 2, 3]]):
        with pytest.raises(ValueError, match="HxWx3 uint8"):
            R.FrameStream.check_frame(bad)


def test_device_functions_refuse_cpu_tensors(R):
    frames = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    m = R.SRVGGNetCompact(num_conv=1, precision="fast")
    with torch.no_grad():
        for call in (lambda: R.from_u8(frames), lambda: R.to_u8(torch.zeros(1, 3, 4, 4)), lambda: R.upscale_u8(m, frames),
                     lambda: m.forward_u8(frames)):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call()
    with pytest.raises(RuntimeError, match="backward"):      # the guard of forward: grad mode on, parameters that require grad
        m.forward_u8(frames)


def test_inference_frames_parser(R):
    from real_esrgan_pytorch_amd import inference_frames
    p = inference_frames.get_parser()
    a = p.parse_args(["--inputs_dir", "D", "--output_dir", "O", "--weights_path", "W"])
    assert (a.inputs_dir, a.output_dir, a.weights_path) == ("D", "O", "W")
    assert (a.model_type, a.num_conv, a.act_type, a.precision, a.depth) == ("rrdb", 16, "prelu", None, 2)
    a = p.parse_args(["--inputs_dir", "D", "--output_dir", "O", "--weights_path", "W", "--model_type", "compact", "--num_conv", "32",
                      "--act_type", "leakyrelu", "--precision", "fast", "--depth", "3"])
    assert (a.model_type, a.num_conv, a.act_type, a.precision, a.depth) == ("compact", 32, "leakyrelu", "fast", 3)
    for bad in (["--model_type", "vgg"], ["--precision", "bf16"], ["--act_type", "gelu"]):
        with pytest.raises(SystemExit):
            p.parse_args(["--inputs_dir", "D", "--output_dir", "O", "--weights_path", "W"] + bad)
    with pytest.raises(SystemExit):
        p.parse_args(["--inputs_dir", "D"])
    assert hasattr(inference_frames, "main")
    assert inference_frames.list_images(os.path.join(ROOT, "tests", "golden", "dataset_images")) == ["sample_38x30.png"]
