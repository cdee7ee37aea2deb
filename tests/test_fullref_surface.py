"""CPU: the host side of the native PSNR / SSIM -- the torch backend (`psnr`, `ssim`, `PSNR`, `SSIM`) against tests/fullref_ref.py
within its derived bound, the exact values of identical images, the declarations of the entry, `config.full_ref`, and everything the
Python layer refuses before it touches a device."""
import ctypes
import importlib
import math
import os
import random
import re

import numpy as np
import pytest
import torch

from tests import fullref_ref as F
from tests import niqe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def Q():
    import __graft_entry__
    __graft_entry__.build()
    from real_esrgan_pytorch_amd import image_quality_assessment
    return image_quality_assessment


def _flat(value, h, w):
    """A float image whose every level is 255 (value 2.0: the luma is pinned) or 0 (value -1.0)."""
    return np.full((1, 3, h, w), value, np.float32)


def _cases():
    rng = np.random.default_rng(11)
    noise = [R.repair_ties(rng.integers(0, 256, (1, 37, 53, 3), dtype=np.uint8))[0] for _ in range(2)]
    yield "noise 37x53", noise[0], noise[1]
    base = rng.integers(0, 256, (1, 40, 70, 3), dtype=np.uint8)
    near = np.clip(base.astype(np.int64) + rng.integers(-3, 4, base.shape), 0, 255).astype(np.uint8)
    yield "near copy 40x70", R.repair_ties(near)[0], R.repair_ties(base)[0]
    yield "all 255 11x11", _flat(2.0, 11, 11), _flat(2.0, 11, 11)
    yield "255 against 0 20x30", _flat(2.0, 20, 30), _flat(-1.0, 20, 30)


def _separable_f64(X, Y):
    """The kernel's order in float64 numpy (H pass, then W pass, taps ascending; numpy does not fuse): a third evaluation of the map."""
    k = F.window_1d()
    x, y = X.astype(np.float64), Y.astype(np.float64)

    def win(v):
        mh, mw = v.shape[1] - 10, v.shape[2] - 10
        t = np.zeros((v.shape[0], mh, v.shape[2]))
        for a in range(11):
            t += k[a] * v[:, a:a + mh, :]
        o = np.zeros((v.shape[0], mh, mw))
        for b in range(11):
            o += k[b] * t[:, :, b:b + mw]
        return o
    mu1, mu2 = win(x), win(y)
    m11, m22, m12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s11, s22, s12 = win(x * x) - m11, win(y * y) - m22, win(x * y) - m12
    return ((2 * m12 + F.C1) * (2 * s12 + F.C2)) / (((m11 + m22) + F.C1) * ((s11 + s22) + F.C2))


def test_torch_backend_lies_inside_the_bound_of_the_reference(Q):
    worst_bound = 0.0
    for name, sr, hr in _cases():
        ref = F.reference(sr, hr, 0)
        t_sr, t_hr = torch.from_numpy(sr), torch.from_numpy(hr)
        got_ssim, got_psnr = Q.ssim(t_sr, t_hr, 0).numpy(), Q.psnr(t_sr, t_hr, 0).numpy()
        assert got_ssim.dtype == np.float64 and got_psnr.dtype == np.float64 and got_ssim.shape == (1,)
        # the map itself, value by value: the separable float64 order, and torch's conv2d through the module's own helper
        sep = _separable_f64(ref["X"], ref["Y"])
        x, y = (torch.from_numpy(ref[k].astype(np.float64))[:, None] for k in ("X", "Y"))
        g = Q._ssim_window(x)
        conv = lambda v: torch.nn.functional.conv2d(v, g)
        m1, m2 = conv(x), conv(y)
        tmap = (((2 * m1 * m2 + F.C1) * (2 * (conv(x * y) - m1 * m2) + F.C2))
                / (((m1 * m1 + m2 * m2) + F.C1) * (((conv(x * x) - m1 * m1) + (conv(y * y) - m2 * m2)) + F.C2)))[:, 0].numpy()
        exact = np.asarray(ref["map"], np.float64)
        ratio = max(float((np.abs(sep - exact) / ref["bound"]).max()), float((np.abs(tmap - exact) / ref["bound"]).max()))
        worst_bound = max(worst_bound, float(ref["bound"].max()))
        print(f"{name}: bound {ref['bound'].min():.2e} .. {ref['bound'].max():.2e}, worst |error| / bound {ratio:.3f}; "
              f"ssim {got_ssim[0]!r} reference {ref['ssim'][0]!r} gate {ref['ssim_gate'][0]:.2e}; psnr {got_psnr[0]!r}")
        assert ratio <= F.GATE
        assert abs(got_ssim[0] - ref["ssim"][0]) <= ref["ssim_gate"][0]
        assert abs(got_psnr[0] - ref["psnr"][0]) <= 16 * 2.0 ** -52 * max(1.0, abs(ref["psnr"][0]))
    assert worst_bound < 1e-9                                               # the bound is no licence: 7e-10 on flat 255, 1e-12 otherwise


def test_identical_images_and_the_extremes_are_exact(Q):
    rng = np.random.default_rng(5)
    img = torch.from_numpy(rng.integers(0, 256, (2, 23, 31, 3), dtype=np.uint8))
    as_float = torch.from_numpy(R.unit_of_u8(img.numpy()))
    top = 10.0 * math.log10(65025.0 / 1e-8)
    for a, b in ((img, img), (as_float, as_float), (img, img.clone())):
        assert Q.ssim(a, b, 0).tolist() == [1.0, 1.0] and Q.ssim(a, b, 3).tolist() == [1.0, 1.0]
        assert Q.psnr(a, b, 0).tolist() == [top, top]
    assert abs(top - 128.13) < 0.005
    assert Q.SSIM(2)(img, img).tolist() == [1.0, 1.0] and Q.PSNR(2)(img, img).tolist() == [top, top]
    p, s = Q.TorchFullRef(2)(img, img)
    assert p.tolist() == [top, top] and s.tolist() == [1.0, 1.0]
    # 255 against 0: every squared difference is 65025
    sr, hr = _flat(2.0, 20, 30), _flat(-1.0, 20, 30)
    ref = F.reference(sr, hr, 0)
    assert ref["X"].min() == 255 and ref["Y"].max() == 0 and ref["sse"].tolist() == [65025 * 20 * 30]
    assert abs(Q.psnr(torch.from_numpy(sr), torch.from_numpy(hr), 0).item() - F.psnr_np(65025 * 600, 600)) <= 16 * 2.0 ** -52     # two libms
    assert F.reference(sr, hr, 4)["sse"].tolist() == [65025 * 12 * 22]
    # a uint8 image and its float form are one image; mixed kinds are accepted
    noise = torch.from_numpy(R.repair_ties(rng.integers(0, 256, (2, 23, 31, 3), dtype=np.uint8))[0])
    fixed = torch.from_numpy(R.repair_ties(img.numpy())[0])
    assert torch.equal(Q.ssim(fixed, noise, 1), Q.ssim(torch.from_numpy(R.unit_of_u8(fixed.numpy())), noise, 1))
    assert torch.equal(Q.psnr(noise, fixed, 1), Q.psnr(noise, torch.from_numpy(R.unit_of_u8(fixed.numpy())), 1))


def test_reference_tiles_cover_every_pixel_once():
    sr, hr = F.pair(3, 2, 11 + 40, 11 + 70)
    ref = F.reference(sr, hr, 0, tile=32)
    assert ref["tile_sse"].shape == (2, 2, 3) and np.array_equal(ref["tile_sse"].sum(axis=(1, 2)), ref["sse"])
    for i in range(2):
        assert abs(ref["tile_sum"][i].sum() / ref["map"][i].size - ref["ssim"][i]) <= ref["ssim_gate"][i]
    iy, ty = F.tile_index(41, 32)
    assert ty == 2 and len(iy) == 51 and iy[31] == 0 and iy[32] == 1 and iy[50] == 1
    ones = F.reference(_flat(2.0, 51, 81), _flat(-1.0, 51, 81), 0, tile=32)
    assert ones["tile_sse"].sum() == 65025 * 51 * 81 and ones["tile_sse"][0, 0, 0] == 65025 * 32 * 32 and ones["tile_sse"][0, 1, 2] == 65025 * 19 * 17


def test_header_declares_the_entry(Q):
    from real_esrgan_pytorch_amd import _lib
    text = open(os.path.join(ROOT, "include", "resr.h")).read()
    assert re.search(r"\bsize_t resr_fullref_workspace_bytes\(const ResrFullRefDesc\* d\);", text)
    assert re.search(r"\bint resr_fullref\(const ResrFullRefDesc\* d, const void\* sr, const void\* hr, int64_t\* sse, double\* psnr, double\* ssim,\s+void\* stream\);", text)
    for name in ("resr_fullref", "resr_fullref_workspace_bytes"):
        assert callable(getattr(_lib.lib(), name)) and name in _lib.exported_symbols()
    assert len(_lib._PROTOS["resr_fullref"][1]) == 7 and len(_lib._PROTOS["resr_fullref_workspace_bytes"][1]) == 1
    assert [f[0] for f in _lib.FullRefDesc._fields_] == ["n", "h", "w", "crop", "sr_u8", "hr_u8", "workspace", "workspace_bytes"]
    assert ctypes.sizeof(_lib.FullRefDesc) == 40
    t = _lib.RESR_FULLREF_TILE
    assert t >= 8 and _lib.RESR_FULLREF_FINISH_THREADS >= 64
    assert 2 * (5 * t * (t + 10) * 8 + 2 * (t + 10) * (t + 12)) <= 160 * 1024      # two workgroups' float64 rows and level bytes fit a CU
    # the size query needs no device: the layout the header states, and the refusals
    d = _lib.FullRefDesc()
    d.n, d.h, d.w, d.crop = 3, 2 * t + 10 + 1 + 6, t + 10 + 6, 3
    assert _lib.lib().resr_fullref_workspace_bytes(d) == 3 * 3 * 1 * 16 and Q.full_ref_tiles(2 * t + 11, t + 10) == (3, 1)
    for field, value in (("n", 0), ("crop", -1), ("crop", 4 + t), ("h", 16), ("w", 0)):
        bad = _lib.FullRefDesc()
        bad.n, bad.h, bad.w, bad.crop = 3, 2 * t + 17, t + 16, 3
        setattr(bad, field, value)
        assert _lib.lib().resr_fullref_workspace_bytes(bad) == 0 and b"fullref" in _lib.lib().resr_last_error(), (field, value)
    assert _lib.lib().resr_fullref_workspace_bytes(None) == 0
    huge = _lib.FullRefDesc()
    huge.n, huge.h, huge.w = 70000, 2 ** 20, 2 ** 20                       # n * tiles beyond an int32 tile index
    assert _lib.lib().resr_fullref_workspace_bytes(huge) == 0 and b"tile index" in _lib.lib().resr_last_error()
    # null pointers and a short workspace: RESR_ERR_ARG with no launch (no device is touched: the checks come first)
    ok = _lib.FullRefDesc()
    ok.n, ok.h, ok.w = 1, 11, 11
    one = ctypes.c_void_p(8)
    assert _lib.lib().resr_fullref(ctypes.byref(ok), one, one, one, one, one, None) == _lib.RESR_ERR_ARG     # workspace null
    assert b"null pointer" in _lib.lib().resr_last_error()


@pytest.fixture
def config(Q, monkeypatch):
    from real_esrgan_pytorch_amd import config as module
    state = (torch.get_rng_state(), random.getstate(), np.random.get_state())

    def reload(value=None):
        monkeypatch.delenv("RESR_FULL_REF", raising=False)
        if value is not None:
            monkeypatch.setenv("RESR_FULL_REF", value)
        return importlib.reload(module)
    yield reload
    monkeypatch.undo()
    importlib.reload(module)
    torch.set_rng_state(state[0])
    random.setstate(state[1])
    np.random.set_state(state[2])


def test_full_ref_defaults_to_off_and_refuses_other_names(Q, config):
    c = config()
    assert c.full_ref == "off" and c.build_full_ref() is None
    c = config("torch")
    c.device = torch.device("cpu")
    m = c.build_full_ref()
    assert c.full_ref == "torch" and type(m) is Q.TorchFullRef and m.crop_border == c.upscale_factor
    c = config("native")
    c.device = torch.device("cpu")
    m = c.build_full_ref()
    assert c.full_ref == "native" and type(m) is Q.NativeFullRef and m.crop_border == c.upscale_factor
    assert config("off").build_full_ref() is None
    with pytest.raises(ValueError, match="RESR_FULL_REF"):
        config("hip")
    c = config()
    c.full_ref = "fast"
    with pytest.raises(ValueError, match="full_ref"):
        c.build_full_ref()


def test_everything_refused_before_a_device_is_touched(Q):
    f = torch.rand(2, 3, 20, 24)
    u = torch.zeros(2, 20, 24, 3, dtype=torch.uint8)
    entries = (Q.psnr, Q.ssim, Q.full_ref_native, lambda a, b, c: Q.NativeFullRef(c)(a, b), lambda a, b, c: Q.TorchFullRef(c)(a, b))
    for fn in entries:
        with pytest.raises(ValueError, match="shapes must match"):
            fn(f, torch.rand(2, 3, 20, 25), 0)
        with pytest.raises(ValueError, match="shapes must match"):
            fn(f, torch.zeros(1, 20, 24, 3, dtype=torch.uint8), 0)
        for bad in (torch.rand(2, 4, 20, 24), torch.zeros(2, 3, 20, 24, dtype=torch.uint8), torch.zeros(2, 3, 20, 24, dtype=torch.int32), torch.rand(3, 20, 24),
                    np.zeros((2, 3, 20, 24), np.float32)):
            with pytest.raises(ValueError, match="float \\[B,3,H,W\\] or a uint8 \\[B,H,W,3\\]"):
                fn(bad, f, 0)
            with pytest.raises(ValueError, match="float \\[B,3,H,W\\] or a uint8 \\[B,H,W,3\\]"):
                fn(u, bad, 0)
        with pytest.raises(ValueError, match="one device"):
            fn(f, torch.empty(2, 3, 20, 24, device="meta"), 0)
        with pytest.raises(ValueError, match="11x11"):
            fn(f, u, 5)                                                     # 10 x 14 is left
        for crop in (-1, 1.0, True):
            with pytest.raises(ValueError, match="crop_border"):
                fn(f, u, crop)
    # the native entries have no torch fallback: a host tensor is an error, not a slow answer
    with pytest.raises(RuntimeError, match="MI355X"):
        Q.full_ref_native(f, u, 4)
    with pytest.raises(RuntimeError, match="MI355X"):
        Q.NativeFullRef(0)(u, u)
    with pytest.raises(ValueError, match="crop_border"):
        Q.NativeFullRef(-1)
    assert Q.psnr(f, u, 4).shape == (2,)                                    # 12 x 16 is enough


def test_names_are_exported_and_the_flag_parses(Q):
    assert {"PSNR", "SSIM", "psnr", "ssim", "NativeFullRef", "full_ref_native"} <= set(Q.__all__)
    assert {"NIQE", "niqe", "NativeNIQE", "niqe_native", "niqe_score_native"} <= set(Q.__all__)
    from real_esrgan_pytorch_amd import inference_frames
    base = ["--inputs_dir", "a", "--output_dir", "b", "--weights_path", "c"]
    assert inference_frames.get_parser().parse_args(base).reference_dir is None
    assert inference_frames.get_parser().parse_args(base + ["--reference_dir", "gt"]).reference_dir == "gt"


def test_validate_takes_the_keyword_and_advertises_the_reference_signature(Q):
    """`full_ref` is a keyword on top of the reference's seven parameters, which stay what the entry point advertises
    (tests/test_surface.py pins that list)."""
    import inspect
    from real_esrgan_pytorch_amd import train_realesrgan, train_realesrnet
    v = train_realesrnet.validate
    assert list(inspect.signature(v).parameters) == ["model", "ema_model", "data_prefetcher", "epoch", "writer", "niqe_model", "mode"]
    assert v.__code__.co_varnames[:v.__code__.co_argcount] == ("model", "ema_model", "data_prefetcher", "epoch", "writer", "niqe_model", "mode", "full_ref")
    assert v.__defaults__ == (None,) and train_realesrgan.validate is v
    with pytest.raises(ValueError, match="Unsupported mode"):                # the keyword is accepted: the call gets as far as its first check
        v(None, None, None, 0, None, None, "Train", full_ref=None)
