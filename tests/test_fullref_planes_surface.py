"""CPU: the host side of the native PSNR / SSIM per plane -- the declarations of resr_fullref_planes and what its size query refuses,
tests/fullref_planes_ref.py against tests/fullref_ref.py at peak 255, the constants, the torch twins (`full_ref_channels`,
`full_ref_yuv`) within the derived gates of the numpy reference at every peak, the views Python builds for every source kind against a
plain numpy slicing of the same array, `config.full_ref_channels`, and everything the Python layer refuses before it touches a device."""
import ctypes
import importlib
import os
import random
import re

import numpy as np
import pytest
import torch

from tests import fullref_planes_ref as P
from tests import fullref_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PSNR_GATE = 16 * 2.0 ** -52          # as tests/test_gpu_fullref_kernels.py: two libms, three roundings of the argument
FIELDS = ["n", "planes", "h", "w", "crop", "peak", "sr_word_bytes", "sr_shift", "sr_mask", "hr_word_bytes", "hr_shift", "hr_mask",
          "sr_base", "sr_pixel_stride", "sr_row_stride", "sr_plane_stride", "sr_image_stride",
          "hr_base", "hr_pixel_stride", "hr_row_stride", "hr_plane_stride", "hr_image_stride", "workspace", "workspace_bytes"]


@pytest.fixture(scope="module")
def Q():
    import __graft_entry__
    __graft_entry__.build()
    from real_esrgan_pytorch_amd import image_quality_assessment
    return image_quality_assessment


def _desc(L, **kw):
    """A valid descriptor: 2 images of 3 interleaved uint8 planes of 40 x 50 on both sides, crop 2."""
    d = L.FullRefPlanesDesc()
    d.n, d.planes, d.h, d.w, d.crop, d.peak = 2, 3, 40, 50, 2, 255
    for side in ("sr", "hr"):
        for k, v in (("word_bytes", 1), ("shift", 0), ("mask", 255), ("base", 0), ("pixel_stride", 3), ("row_stride", 150), ("plane_stride", 1), ("image_stride", 6000)):
            setattr(d, f"{side}_{k}", v)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


REFUSED = [("n", 0), ("planes", 0), ("planes", 5), ("h", 0), ("w", 0), ("crop", -1), ("crop", 15), ("peak", 256), ("peak", 0), ("peak", 4095),
           ("sr_word_bytes", 3), ("hr_word_bytes", 0), ("hr_word_bytes", 8), ("sr_mask", 256), ("hr_mask", -1), ("sr_shift", -1), ("hr_shift", 16),
           ("sr_pixel_stride", 0), ("hr_pixel_stride", -3), ("sr_row_stride", 0), ("hr_row_stride", -150), ("sr_plane_stride", -1), ("hr_image_stride", -1),
           ("sr_base", -1), ("hr_base", -1)]


def test_header_declares_the_entry_and_the_query_refuses_bad_sizes(Q):
    from real_esrgan_pytorch_amd import _lib
    lib = _lib.lib()
    text = open(os.path.join(ROOT, "include", "resr.h")).read()
    assert re.search(r"\bsize_t resr_fullref_planes_workspace_bytes\(const ResrFullRefPlanesDesc\* d\);", text)
    assert re.search(r"\bint resr_fullref_planes\(const ResrFullRefPlanesDesc\* d, const void\* sr, const void\* hr, int64_t\* sse, double\* psnr, double\* ssim,\s+void\* stream\);", text)
    for name in ("resr_fullref_planes", "resr_fullref_planes_workspace_bytes"):
        assert callable(getattr(lib, name)) and name in _lib.exported_symbols()
    assert len(_lib._PROTOS["resr_fullref_planes"][1]) == 7 and len(_lib._PROTOS["resr_fullref_planes_workspace_bytes"][1]) == 1
    assert [f[0] for f in _lib.FullRefPlanesDesc._fields_] == FIELDS
    assert ctypes.sizeof(_lib.FullRefPlanesDesc) == 12 * 4 + 10 * 8 + 16
    # the existing entry keeps its descriptor, and the header no longer lists RGB channels as missing
    assert ctypes.sizeof(_lib.FullRefDesc) == 40 and _lib.RESR_VERSION == 3
    assert "RGB-channel scoring" not in text
    t = _lib.RESR_FULLREF_TILE
    assert 2 * (5 * t * (t + 10) * 8 + 2 * (t + 10) * (t + 12) * 2 + 64) <= 160 * 1024     # 16-bit levels: two workgroups still fit a CU
    # the size query needs no device: n * planes * tiles * 16, and 0 with the reason for what the entry refuses
    ty, tx = Q.full_ref_tiles(36, 46)
    assert lib.resr_fullref_planes_workspace_bytes(_desc(_lib)) == 2 * 3 * ty * tx * 16
    assert lib.resr_fullref_planes_workspace_bytes(_desc(_lib, h=2 * t + 11, w=t + 10, crop=0, n=1, planes=4)) == 4 * 3 * 1 * 16
    for peak in P.PEAKS:
        assert lib.resr_fullref_planes_workspace_bytes(_desc(_lib, peak=peak, sr_mask=peak)) > 0
    for field, value in REFUSED:
        assert lib.resr_fullref_planes_workspace_bytes(_desc(_lib, **{field: value})) == 0, (field, value)
        assert b"fullref_planes" in lib.resr_last_error(), (field, value)
    assert lib.resr_fullref_planes_workspace_bytes(None) == 0 and b"fullref_planes" in lib.resr_last_error()
    assert lib.resr_fullref_planes_workspace_bytes(_desc(_lib, n=70000, planes=4, h=2 ** 20, w=2 ** 20)) == 0 and b"tile index" in lib.resr_last_error()
    # null pointers: RESR_ERR_ARG with no launch (no device is touched: the checks come first)
    one = ctypes.c_void_p(8)
    assert lib.resr_fullref_planes(ctypes.byref(_desc(_lib)), one, one, one, one, one, None) == _lib.RESR_ERR_ARG      # workspace null
    assert b"fullref_planes: null pointer" in lib.resr_last_error()
    assert lib.resr_fullref_planes(None, one, one, one, one, one, None) == _lib.RESR_ERR_ARG


def test_constants_are_the_literals_of_the_luma_kernel_at_255(Q):
    c1, c2 = P.constants(255)
    assert c1.hex() == (6.5025).hex() == F.C1.hex() and c2.hex() == (58.5225).hex() == F.C2.hex()
    assert Q.full_ref_constants(255) == (c1, c2)
    for peak in P.PEAKS:
        assert Q.full_ref_constants(peak) == P.constants(peak) == (peak * peak / 10000.0, 9 * peak * peak / 10000.0)
    assert P.constants(1023) == (104.6529, 941.8761) and P.constants(65535)[0] == 429483.6225
    assert Q.FULL_REF_PEAKS == P.PEAKS


def test_reference_at_255_is_the_luma_reference(Q):
    """Levels from fullref_ref.levels through fullref_planes_ref.reference: every entry of fullref_ref.reference, bit for bit."""
    for crop, (h, w) in ((0, (11 + 40, 11 + 70)), (3, (29, 60))):
        sr, hr = F.pair(7 + crop, 3, h, w)
        want = F.reference(sr, hr, crop, tile=32)
        got = P.reference(F.levels(sr, crop), F.levels(hr, crop), 255, tile=32)
        assert set(got) == set(want)
        for k in want:
            a, b = np.asarray(got[k]), np.asarray(want[k])
            assert a.dtype == b.dtype and a.shape == b.shape, k
            # (a longdouble carries padding bytes: its values are compared, every other array its bytes)
            assert np.array_equal(a, b) if a.dtype == np.longdouble and a.itemsize > 8 else a.tobytes() == b.tobytes(), k
    assert np.array_equal(P.psnr_np([0, 5, 10 ** 9], 600, 255), F.psnr_np([0, 5, 10 ** 9], 600))


def _noise(rng, peak, shape, dtype):
    return rng.integers(0, peak + 1, shape).astype(dtype)


def test_quantise_and_gather_follow_their_sentence():
    v = np.array([-1.0, -0.0, 0.0, 0.5, 1.0, 2.0, np.nan, np.inf, -np.inf, 254.5 / 255, 0.999999], np.float32)
    assert P.quantise(v, 255).tolist() == [0, 0, 0, 127, 255, 255, 0, 255, 0, 254, 254]
    assert P.quantise(v, 65535).tolist() == [0, 0, 0, 32767, 65535, 65535, 0, 65535, 0, int(np.float32(254.5 / 255) * np.float32(65535)), 65534]
    words = (np.arange(2 * 5 * 7 * 3) * 37 % 65536).astype(np.uint16)
    got = P.gather(words, P.View(2, 6, 1023, 1, 3, 21, 1, 105), 2, 2, 5, 6, 1023)
    img = words[1:].copy()
    for i in range(2):
        for p in range(2):
            for y in range(5):
                for x in range(6):
                    assert got[i, p, y, x] == (int(img[i * 105 + p + y * 21 + x * 3]) >> 6) & 1023


def test_views_of_every_source_kind(Q):
    """The views Python builds, read with the reference's gather (and with the torch backend's loader), against plain slicing."""
    rng = np.random.default_rng(3)
    n, h, w = 2, 6, 8
    for dtype, peak in ((np.uint8, 255), (np.uint16, 65535)):
        for c in (1, 3, 4):
            img = _noise(rng, peak, (n, h, w, c), dtype)
            view, *shape, got_peak = Q.image_plane_view(torch.from_numpy(img), "sr", "t")
            assert shape == [n, c, h, w] and got_peak == peak and view.word_bytes == img.itemsize
            want = img.transpose(0, 3, 1, 2).astype(np.int64)
            assert np.array_equal(P.gather(img, P.View(*view), n, c, h, w, peak), want)
            assert np.array_equal(Q.plane_levels(torch.from_numpy(img), view, n, c, h, w, peak).numpy(), want)
    for c in (1, 3):
        img = rng.uniform(-0.2, 1.2, (n, c, h, w)).astype(np.float32)
        img[0, 0, 0, 0] = np.nan
        view, *shape, got_peak = Q.image_plane_view(torch.from_numpy(img), "hr", "t")
        assert shape == [n, c, h, w] and got_peak is None and view.word_bytes == 4
        for peak in P.PEAKS:
            want = P.quantise(img, peak)
            assert want[0, 0, 0, 0] == 0 and want.min() == 0 and want.max() == peak
            assert np.array_equal(P.gather(img, P.View(*view), n, c, h, w, peak), want)
            assert np.array_equal(Q.plane_levels(torch.from_numpy(img), view, n, c, h, w, peak).numpy(), want)
    # 4:2:0 frames: planar and semi-planar chroma, 10 bits in the low or the high bits of the word (garbage in the other six)
    y = _noise(rng, 1023, (n, h, w), np.uint16)
    cb, cr = _noise(rng, 1023, (n, h // 2, w // 2), np.uint16), _noise(rng, 1023, (n, h // 2, w // 2), np.uint16)
    planar = np.concatenate([y.reshape(n, -1), cb.reshape(n, -1), cr.reshape(n, -1)], axis=1).reshape(n, 3 * h // 2, w)
    semi = np.concatenate([y.reshape(n, -1), np.stack([cb, cr], axis=-1).reshape(n, -1)], axis=1).reshape(n, 3 * h // 2, w)
    junk = rng.integers(0, 64, planar.shape).astype(np.uint16)
    frames = {"i420": ((planar >> 2).astype(np.uint8), 2, 255), "nv12": ((semi >> 2).astype(np.uint8), 2, 255),
              "i420p10": (planar | (junk << 10), 0, 1023), "p010": ((semi << 6) | junk, 0, 1023)}
    for name, (frame, drop, peak) in frames.items():
        luma, chroma, got_peak = Q.yuv_plane_views(name, h, w)
        assert got_peak == peak
        for loader in (lambda v, planes, ph, pw: P.gather(frame, P.View(*v), n, planes, ph, pw, peak),
                       lambda v, planes, ph, pw: Q.plane_levels(torch.from_numpy(frame), v, n, planes, ph, pw, peak).numpy()):
            assert np.array_equal(loader(luma, 1, h, w)[:, 0], y >> drop), name
            got = loader(chroma, 2, h // 2, w // 2)
            assert np.array_equal(got[:, 0], cb >> drop) and np.array_equal(got[:, 1], cr >> drop), name
    with pytest.raises(ValueError, match="pix_fmt"):
        Q.yuv_plane_views("rgb24", h, w)
    with pytest.raises(ValueError, match="even"):
        Q.yuv_plane_views("i420", 7, 8)


def _check_against(ref, sse, psnr, ssim, label):
    assert sse.dtype == np.int64 and psnr.dtype == np.float64 and ssim.dtype == np.float64
    assert np.array_equal(sse.reshape(-1), ref["sse"]), label
    ratio = np.abs(ssim.reshape(-1) - ref["ssim"]) / ref["ssim_gate"]
    want = ref["psnr"]
    pratio = np.abs(psnr.reshape(-1) - want) / (PSNR_GATE * np.maximum(1.0, np.abs(want)))
    print(f"{label}: ssim at {ratio.max():.3e} of its gate ({ref['ssim_gate'].max():.2e}), psnr at {pratio.max():.3f} of its")
    assert (ratio <= 1).all() and (pratio <= 1).all(), label


def test_torch_twin_of_the_channels_inside_the_gates(Q):
    rng = np.random.default_rng(17)
    b, h, w, crop = 2, 29, 40, 2
    for dtype, peak in ((np.uint8, 255), (np.uint16, 65535)):
        for c in (1, 3, 4):
            hr = _noise(rng, peak, (b, h, w, c), dtype)
            sr = hr.copy()
            sr[0] = _noise(rng, peak, (h, w, c), dtype)
            sr[1] = np.clip(hr[1].astype(np.int64) + rng.integers(-peak // 64, peak // 64 + 1, (h, w, c)), 0, peak).astype(dtype)
            X, Y = (P.crop(a.transpose(0, 3, 1, 2).astype(np.int64), crop).reshape(b * c, h - 2 * crop, w - 2 * crop) for a in (sr, hr))
            ref = P.reference(X, Y, peak)
            got = Q.full_ref_channels(torch.from_numpy(sr), torch.from_numpy(hr), crop)
            assert got.sse.shape == got.psnr.shape == got.ssim.shape == (b, c) and got.psnr_all.shape == got.ssim_mean.shape == (b,)
            _check_against(ref, got.sse.numpy(), got.psnr.numpy(), got.ssim.numpy(), f"{np.dtype(dtype).name} C={c}")
            psnr_all, mean, gate = P.channels_summary(ref, b, c, peak)
            assert (np.abs(got.psnr_all.numpy() - psnr_all) <= PSNR_GATE * np.maximum(1.0, np.abs(psnr_all))).all()
            assert (np.abs(got.ssim_mean.numpy() - mean) <= gate).all()
            if c == 3:                                                       # a float side is quantised to the other side's peak
                f = rng.uniform(-0.1, 1.1, (b, 3, h, w)).astype(np.float32)
                f[1, 2, 5, 5] = np.nan
                ref = P.reference(P.crop(P.quantise(f, peak), crop).reshape(b * 3, h - 2 * crop, w - 2 * crop), Y, peak)
                got = Q.full_ref_channels(torch.from_numpy(f), torch.from_numpy(hr), crop)
                _check_against(ref, got.sse.numpy(), got.psnr.numpy(), got.ssim.numpy(), f"float against {np.dtype(dtype).name}")
    # both sides float: 8 bits; identical sides: exact
    f = rng.uniform(0, 1, (b, 3, h, w)).astype(np.float32)
    g = rng.uniform(0, 1, (b, 3, h, w)).astype(np.float32)
    X, Y = (P.crop(P.quantise(a, 255), 0).reshape(b * 3, h, w) for a in (f, g))
    got = Q.full_ref_channels(torch.from_numpy(f), torch.from_numpy(g), 0)
    _check_against(P.reference(X, Y, 255), got.sse.numpy(), got.psnr.numpy(), got.ssim.numpy(), "float against float")
    same = Q.full_ref_channels(torch.from_numpy(f), torch.from_numpy(f.copy()), 3)
    assert same.sse.eq(0).all() and same.ssim.eq(1.0).all() and same.ssim_mean.tolist() == [1.0, 1.0]
    assert same.psnr_all.tolist() == [float(P.psnr_np(0, 1, 255))] * 2
    m = Q.TorchFullRefChannels(0)(torch.from_numpy(f), torch.from_numpy(g))
    assert torch.equal(m[0], got.psnr_all) and torch.equal(m[1], got.ssim_mean)


def _yuv_frames(rng, name, n, h, w, near=None):
    """n frames [3h/2, w] of the named format from random levels (or within +-3 levels of the frames `near` = (y, cb, cr))."""
    bits10 = name in ("i420p10", "p010")
    peak, dtype = (1023, np.uint16) if bits10 else (255, np.uint8)
    if near is None:
        y, cb, cr = _noise(rng, peak, (n, h, w), np.int64), _noise(rng, peak, (n, h // 2, w // 2), np.int64), _noise(rng, peak, (n, h // 2, w // 2), np.int64)
    else:
        y, cb, cr = (np.clip(a + rng.integers(-3, 4, a.shape), 0, peak) for a in near)
    chroma = np.stack([cb, cr], axis=-1).reshape(n, -1) if name in ("nv12", "p010") else np.concatenate([cb.reshape(n, -1), cr.reshape(n, -1)], axis=1)
    frame = np.concatenate([y.reshape(n, -1), chroma], axis=1).reshape(n, 3 * h // 2, w)
    if name == "p010":
        frame = (frame << 6) | rng.integers(0, 64, frame.shape)
    elif name == "i420p10":
        frame = frame | (rng.integers(0, 64, frame.shape) << 10)
    return frame.astype(dtype), (y, cb, cr), peak


def test_torch_twin_of_the_yuv_planes_inside_the_gates(Q):
    rng = np.random.default_rng(23)
    n, h, w = 2, 34, 46
    for name, other in (("i420", "nv12"), ("nv12", "nv12"), ("i420p10", "p010"), ("p010", "i420p10")):
        ref_frame, planes, peak = _yuv_frames(rng, other, n, h, w)
        frame, mine, _ = _yuv_frames(rng, name, n, h, w, near=planes)
        got = Q.full_ref_yuv(torch.from_numpy(frame), torch.from_numpy(ref_frame), name, other, 2)
        refs = [P.reference(P.crop(a, c), P.crop(b, c), peak) for a, b, c in zip(mine, planes, (2, 1, 1))]
        for r, psnr, ssim, label in zip(refs, (got.psnr_y, got.psnr_u, got.psnr_v), (got.ssim_y, got.ssim_u, got.ssim_v), "yuv"):
            _check_against(r, r["sse"], psnr.numpy(), ssim.numpy(), f"{name} against {other} {label}")
        samples = (h - 4) * (w - 4) + 2 * (h // 2 - 2) * (w // 2 - 2)
        want = P.psnr_np(sum(r["sse"] for r in refs), samples, peak)
        assert (np.abs(got.psnr_avg.numpy() - want) <= PSNR_GATE * np.maximum(1.0, np.abs(want))).all()
        same = Q.full_ref_yuv(torch.from_numpy(frame), torch.from_numpy(frame.copy()), name)
        assert all(t.tolist() == [1.0] * n for t in (same.ssim_y, same.ssim_u, same.ssim_v))
        assert same.psnr_avg.tolist() == [float(P.psnr_np(0, 1, peak))] * n


@pytest.fixture
def config(Q, monkeypatch):
    from real_esrgan_pytorch_amd import config as module
    state = (torch.get_rng_state(), random.getstate(), np.random.get_state())

    def reload(channels=None, backend=None):
        for name, value in (("RESR_FULL_REF_CHANNELS", channels), ("RESR_FULL_REF", backend)):
            monkeypatch.delenv(name, raising=False)
            if value is not None:
                monkeypatch.setenv(name, value)
        return importlib.reload(module)
    yield reload
    monkeypatch.undo()
    importlib.reload(module)
    torch.set_rng_state(state[0])
    random.setstate(state[1])
    np.random.set_state(state[2])


def test_full_ref_channels_defaults_to_y_and_refuses_other_names(Q, config):
    c = config()
    assert c.full_ref_channels == "y" and c.build_full_ref() is None
    c = config(None, "torch")
    c.device = torch.device("cpu")
    assert c.full_ref_channels == "y" and type(c.build_full_ref()) is Q.TorchFullRef
    c = config("rgb")
    assert c.full_ref_channels == "rgb" and c.build_full_ref() is None       # RESR_FULL_REF stays off: nothing is scored
    for backend, cls in (("torch", Q.TorchFullRefChannels), ("native", Q.NativeFullRefChannels)):
        c = config("rgb", backend)
        c.device = torch.device("cpu")
        m = c.build_full_ref()
        assert type(m) is cls and m.crop_border == c.upscale_factor
    c = config("y", "native")
    c.device = torch.device("cpu")
    assert type(c.build_full_ref()) is Q.NativeFullRef
    for bad in ("RGB", "yuv", ""):
        with pytest.raises(ValueError, match="RESR_FULL_REF_CHANNELS"):
            config(bad)
    c = config(None, "torch")
    c.full_ref_channels = "all"
    with pytest.raises(ValueError, match="full_ref_channels"):
        c.build_full_ref()


def test_everything_refused_before_a_device_is_touched(Q):
    f = torch.rand(2, 3, 20, 24)
    u = torch.zeros(2, 20, 24, 3, dtype=torch.uint8)
    u16 = torch.zeros(2, 20, 24, 3, dtype=torch.uint16)
    for fn in (Q.full_ref_channels, Q.full_ref_channels_native, lambda a, b, c: Q.TorchFullRefChannels(c)(a, b), lambda a, b, c: Q.NativeFullRefChannels(c)(a, b)):
        with pytest.raises(ValueError, match="shapes must match"):
            fn(f, torch.rand(2, 3, 20, 25), 0)
        with pytest.raises(ValueError, match="shapes must match"):
            fn(f, torch.zeros(2, 20, 24, 1, dtype=torch.uint8), 0)
        with pytest.raises(ValueError, match="one depth"):
            fn(u, u16, 0)
        for bad in (torch.rand(2, 4, 20, 24), torch.rand(2, 2, 20, 24), torch.zeros(2, 20, 24, 2, dtype=torch.uint8), torch.zeros(2, 20, 24, 3, dtype=torch.int32),
                    torch.rand(3, 20, 24), np.zeros((2, 3, 20, 24), np.float32)):
            with pytest.raises(ValueError, match="must be a float \\[B,C,H,W\\]"):
                fn(bad, f, 0)
            with pytest.raises(ValueError, match="must be a float \\[B,C,H,W\\]"):
                fn(u, bad, 0)
        with pytest.raises(ValueError, match="one device"):
            fn(f, torch.empty(2, 3, 20, 24, device="meta"), 0)
        with pytest.raises(ValueError, match="11x11"):
            fn(f, u, 5)
    for crop in (-1, 1.0, True):
        with pytest.raises(ValueError, match="crop_border"):
            Q.full_ref_channels(f, u, crop)
        with pytest.raises(ValueError, match="crop_border"):
            Q.NativeFullRefChannels(crop)
    with pytest.raises(RuntimeError, match="MI355X"):                       # no torch fallback behind the native entries
        Q.full_ref_channels_native(f, u16, 4)
    y8, y10 = torch.zeros(1, 48, 32, dtype=torch.uint8), torch.zeros(1, 48, 32, dtype=torch.uint16)
    for fn in (Q.full_ref_yuv, Q.full_ref_yuv_native):
        with pytest.raises(ValueError, match="even"):
            fn(y8, y8, "i420", None, 1)
        with pytest.raises(ValueError, match="one depth"):
            fn(y8, y10, "nv12", "p010")
        with pytest.raises(ValueError, match="pix_fmt"):
            fn(y8, y8, "rgb24")
        with pytest.raises(ValueError, match="pix_fmt"):
            fn(y8, y8, "i420", "yuv444p")
        with pytest.raises(ValueError, match="frames must be"):
            fn(y10, y8, "i420")
        with pytest.raises(ValueError, match="reference must be"):
            fn(y8, torch.zeros(1, 47, 32, dtype=torch.uint8), "i420")
        with pytest.raises(ValueError, match="shapes must match"):
            fn(y8, torch.zeros(2, 48, 32, dtype=torch.uint8), "i420")
        with pytest.raises(ValueError, match="11x11"):
            fn(y8, y8, "i420", None, 6)                                     # the 16 x 16 chroma planes keep 10 x 10
    with pytest.raises(RuntimeError, match="MI355X"):
        Q.full_ref_yuv_native(y8, y8, "i420")
    assert Q.full_ref_yuv(y8, y8, "i420", "nv12", 4).ssim_v.tolist() == [1.0]


def test_names_are_exported_and_the_flags_parse(Q):
    assert {"full_ref_channels", "full_ref_channels_native", "full_ref_yuv", "full_ref_yuv_native", "NativeFullRefChannels", "TorchFullRefChannels"} <= set(Q.__all__)
    assert Q.FULL_REF_BACKENDS == ("off", "torch", "native") and Q.FULL_REF_CHANNELS == ("y", "rgb")
    from real_esrgan_pytorch_amd import inference_frames, inference_rawvideo
    base = ["--inputs_dir", "a", "--output_dir", "b", "--weights_path", "c"]
    assert inference_frames.get_parser().parse_args(base).score_channels == "y"
    assert inference_frames.get_parser().parse_args(base + ["--reference_dir", "gt", "--score_channels", "rgb"]).score_channels == "rgb"
    base = ["--input", "a", "--output", "b", "--size", "16x24", "--weights_path", "c"]
    args = inference_rawvideo.get_parser().parse_args(base)
    assert args.reference is None and args.reference_pix_fmt is None and args.reference_size is None
    args = inference_rawvideo.get_parser().parse_args(base + ["--reference", "r.yuv", "--reference_pix_fmt", "nv12"])
    assert args.reference == "r.yuv" and args.reference_pix_fmt == "nv12"


def test_rawvideo_reference_is_checked_before_a_model_is_built(Q, tmp_path):
    """reference_plan: everything that can be known from the arguments and the files is refused with its cause; main() refuses an
    rgb24 output before it touches the device."""
    import argparse
    from real_esrgan_pytorch_amd import inference_rawvideo as V
    out_w, out_h = 96, 64
    inp, ref = tmp_path / "in.yuv", tmp_path / "ref.yuv"
    inp.write_bytes(bytes(V.frame_bytes(24, 16) * 3))
    ref.write_bytes(bytes(V.frame_bytes(out_w, out_h) * 3))
    args = argparse.Namespace(input=str(inp), reference=str(ref), reference_pix_fmt=None, reference_size=None)
    assert V.reference_plan(argparse.Namespace(input=str(inp), reference=None), "yuv420p", out_w, out_h, V.frame_bytes(24, 16)) is None
    assert V.reference_plan(args, "yuv420p", out_w, out_h, V.frame_bytes(24, 16)) == (str(ref), "i420", np.dtype(np.uint8))
    args.reference_pix_fmt = "nv12"
    assert V.reference_plan(args, "yuv420p", out_w, out_h, V.frame_bytes(24, 16))[1] == "nv12"
    ref.write_bytes(bytes(V.frame_bytes(out_w, out_h) * 2))
    with pytest.raises(ValueError, match="shorter than the input"):
        V.reference_plan(args, "yuv420p", out_w, out_h, V.frame_bytes(24, 16))
    ref.write_bytes(bytes(V.frame_bytes(out_w, out_h) * 3 + 10))
    with pytest.raises(ValueError, match="must have the output's size"):
        V.reference_plan(args, "yuv420p", out_w, out_h, V.frame_bytes(24, 16))
    args.reference_size = "96x60"
    with pytest.raises(ValueError, match="must have the output's size"):
        V.reference_plan(args, "yuv420p", out_w, out_h, V.frame_bytes(24, 16))
    args.reference_size, args.reference_pix_fmt = None, "p010le"
    with pytest.raises(ValueError, match="one bit depth"):
        V.reference_plan(args, "yuv420p", out_w, out_h, V.frame_bytes(24, 16))
    args.reference_pix_fmt = "rgb24"
    with pytest.raises(ValueError, match="--reference_pix_fmt"):
        V.reference_plan(args, "yuv420p", out_w, out_h, V.frame_bytes(24, 16))
    with pytest.raises(ValueError, match="rgb24 output"):
        V.main(argparse.Namespace(size="24x16", input=str(inp), output=str(tmp_path / "o"), reference=str(ref), pix_fmt="yuv420p", out_pix_fmt="rgb24"))
