"""CPU: the surface of the image modes (grey, RGBA and 16-bit images on the frame path) -- the numpy definition in frames.py, the
three C-ABI entries (exported, declared once, bound; every refusal before any launch), the package exports and the CLI switch.
Nothing here touches a device: a call that got as far as a launch would not return RESR_ERR_ARG."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("resr_compact_forward_image", "resr_image_to_nchw", "resr_nchw_to_image")
ERR_ARG, ERR_WORKSPACE = -1, -3          # include/resr.h resr_status
MODES = [(c, b) for c in (1, 3, 4) for b in (8, 16)]
# include/resr.h, "Image modes": the widest store of a mode's tail, the widest load of its head
STORE_ALIGN = {(1, 8): 4, (1, 16): 8, (3, 8): 4, (3, 16): 4, (4, 8): 16, (4, 16): 16}
LOAD_ALIGN = {(1, 8): 1, (1, 16): 2, (3, 8): 1, (3, 16): 2, (4, 8): 4, (4, 16): 8}


@pytest.fixture(scope="module")
def R():
    import __graft_entry__
    __graft_entry__.build()
    import real_esrgan_pytorch_amd as R
    return R


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def _float_grey(rgb):
    v = rgb.astype(np.float64)
    return np.rint(0.299 * v[..., 0] + 0.587 * v[..., 1] + 0.114 * v[..., 2])


def test_grey_is_exact_on_grey_triples(R):
    for dtype, levels in ((np.uint8, 256), (np.uint16, 65536)):
        v = np.arange(levels).astype(dtype)
        g = R.grey_np(np.stack([v, v, v], axis=-1))
        assert g.dtype == dtype and np.array_equal(g, v)


def test_grey_8_bits_exhaustively_within_one_level(R):
    gb = np.stack(np.meshgrid(np.arange(256), np.arange(256), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.uint8)
    worst, differ = 0, 0
    for r in range(256):
        rgb = np.concatenate([np.full((gb.shape[0], 1), r, np.uint8), gb], axis=1)
        d = np.abs(R.grey_np(rgb).astype(np.int64) - _float_grey(rgb).astype(np.int64))
        worst, differ = max(worst, int(d.max())), differ + int((d != 0).sum())
    assert worst == 1
    assert 0 < differ / 2 ** 24 < 0.01          # a fraction of a percent of the triples differ at all


def test_grey_16_bits_within_two_levels(R):
    top = 65535
    rgb = np.random.RandomState(16).randint(0, 65536, size=(1 << 20, 3)).astype(np.uint16)
    corners = np.array([[0, 0, 0], [top, 0, 0], [0, top, 0], [0, 0, top], [top, top, top]], np.uint16)
    rgb = np.concatenate([rgb, corners])
    g = R.grey_np(rgb)
    assert g.dtype == np.uint16
    assert int(np.abs(g.astype(np.int64) - _float_grey(rgb).astype(np.int64)).max()) <= 2
    assert list(g[-5:]) == [0, (4899 * top + 8192) >> 14, (9617 * top + 8192) >> 14, (1868 * top + 8192) >> 14, top]
    assert 4899 + 9617 + 1868 == 1 << 14 and (1 << 14) * top + 8192 < 1 << 31          # it fits int32
    for bad in (rgb.astype(np.int32), rgb[:, :2], np.float32(0)):
        with pytest.raises(ValueError):
            R.grey_np(bad)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_image_to_rgb_and_back(R, dtype):
    top = np.iinfo(dtype).max
    rs = np.random.RandomState(3)
    n, h, w = 3, 4, 5
    grey = rs.randint(0, top + 1, size=(n, h, w)).astype(dtype)
    for g in (grey, grey[..., None]):
        rgb = R.image_to_rgb_np(g)
        assert rgb.shape == (n, h, w, 3) and rgb.dtype == dtype
        assert all(np.array_equal(rgb[..., c], grey) for c in range(3))
        back = R.rgb_to_image_np(rgb, 1)
        assert back.shape == (n, h, w) and back.dtype == dtype and np.array_equal(back, grey)
    colour = rs.randint(0, top + 1, size=(n, h, w, 3)).astype(dtype)
    assert np.array_equal(R.image_to_rgb_np(colour), colour) and np.array_equal(R.rgb_to_image_np(colour, 3), colour)
    rgba = rs.randint(0, top + 1, size=(n, h, w, 4)).astype(dtype)
    rgb = R.image_to_rgb_np(rgba)
    assert rgb.shape == (2 * n, h, w, 3) and rgb.dtype == dtype
    assert np.array_equal(rgb[:n], rgba[..., :3])                                        # the N colour images ...
    assert all(np.array_equal(rgb[n:, :, :, c], rgba[..., 3]) for c in range(3))         # ... then the N alpha planes, thrice
    back = R.rgb_to_image_np(rgb, 4)
    assert back.shape == rgba.shape and back.dtype == dtype and np.array_equal(back, rgba)
    # the fourth channel is the grey of the LAST N images, not a copy of one of their channels
    mixed = rgb.copy()
    mixed[n:, :, :, 1] = top - mixed[n:, :, :, 1]
    assert np.array_equal(R.rgb_to_image_np(mixed, 4)[..., 3], R.grey_np(mixed[n:]))
    assert np.array_equal(R.rgb_to_image_np(mixed, 4)[..., :3], mixed[:n])
    for bad in (np.zeros((2, 3, 4, 2), dtype), np.zeros((2, 3, 4, 5), dtype), np.zeros((3, 4), dtype), np.zeros((1, 2, 3, 4, 1), dtype),
                np.zeros((2, 3, 4, 3), np.float32), np.zeros((0, 3, 4), dtype)):
        with pytest.raises(ValueError):
            R.image_to_rgb_np(bad)
    with pytest.raises(ValueError):
        R.rgb_to_image_np(rgb[:3], 4)             # an odd number of network images is no RGBA batch
    for channels in (0, 2, 5):
        with pytest.raises(ValueError):
            R.rgb_to_image_np(rgb, channels)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_symbols_exported_declared_once_and_bound(R):
    lib = C.CDLL(R._lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "resr.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert len(re.findall(r"\b%s\s*\(" % name, code)) == 1, name
        assert name in R._lib.exported_symbols(), name
    assert [f[0] for f in R._lib.ImageDesc._fields_] == ["channels", "bits"] and C.sizeof(R._lib.ImageDesc) == 8
    assert R._lib.lib().resr_version() == R._lib.RESR_VERSION == 3            # nothing an existing caller reads has moved
    about = hdr[hdr.index("Image modes (frames.hip)"):hdr.index("resr_nchw_to_image(")]
    for word in ("4899", "alpha_upsampler", "16 bytes for RGBA", "NaN", "before any launch"):
        assert word in about, word
    # each of the new host functions is declared once, in the internal header
    host = open(os.path.join(ROOT, "real_esrgan-pytorch_amd", "csrc", "host_api.h")).read()
    for name in ("image_forward_check", "compact_tail_image", "image_to_nchw_dispatch", "nchw_to_image_dispatch"):
        assert len(re.findall(r"\b%s\(" % name, host)) == 1, name


def test_package_exports(R):
    for name in ("image_to_rgb_np", "grey_np", "rgb_to_image_np", "from_image", "to_image", "upscale_image"):
        assert hasattr(R, name) and name in R.__all__ and name in R.frames.__all__, name
        assert getattr(R.frames, name) is getattr(R, name)
    assert callable(R.SRVGGNetCompact.forward_image)
    assert not hasattr(R.Generator, "forward_image") and not hasattr(R.Generator, "forward_u8")      # the RRDB model takes the composition
    # the pixel-format table of the streams is left alone
    assert tuple(R.PIXEL_FORMATS) == R.FrameStream.PIX_FMTS == ("rgb24", "i420", "nv12", "i420p10", "p010")


def _fake(nbytes=256):
    """A 64-byte aligned host buffer standing in for a device pointer: the calls below return before they would launch anything."""
    buf = (C.c_uint8 * (nbytes + 64))()
    base = (C.addressof(buf) + 63) // 64 * 64
    return buf, base


def _desc(L, n=2, h=8, w=8, dtype=None):
    return L.CompactDesc(n, h, w, 2, 4, 0, L.RESR_F16 if dtype is None else dtype, 0)


@pytest.mark.parametrize("channels,bits", MODES)
def test_forward_image_refusals_need_no_gpu(R, channels, bits):
    L = R._lib
    lib = L.lib()
    keep, base = _fake()
    p = C.c_void_p(base)
    good, img = _desc(L), L.ImageDesc(channels, bits)
    ws = lib.resr_compact_workspace_bytes(C.byref(good))
    assert ws > 0

    def call(d=good, x=p, params=p, packed=p, workspace=p, nbytes=ws, y=p, im=img):
        return lib.resr_compact_forward_image(C.byref(d) if d is not None else None, x, params, packed, workspace, nbytes, y,
                                              C.byref(im) if im is not None else None, None)

    # a null pointer, the image descriptor included
    for hole in ("x", "params", "packed", "workspace", "y", "im"):
        assert call(**{hole: None}) == ERR_ARG, hole
        assert b"null" in lib.resr_last_error(), hole
    assert call(d=None) == ERR_ARG
    # the descriptor's own refusals, exact16's 2^24-pixel cap on the NETWORK's batch among them: one 4096 x 4096 RGBA image is two
    for bad in (_desc(L, n=0), _desc(L, h=0), L.CompactDesc(2, 8, 8, 2, 5, 0, L.RESR_F16, 0), _desc(L, 2, 4096, 4096, L.RESR_F16X2)):
        assert call(d=bad) == ERR_ARG
        assert b"descriptor" in lib.resr_last_error()
    assert lib.resr_compact_workspace_bytes(C.byref(_desc(L, 1, 4096, 4096, L.RESR_F16X2))) > 0          # half of it is within the cap
    # channels and bits
    for c in (0, 2, 5, -1):
        assert call(im=L.ImageDesc(c, bits)) == ERR_ARG
        assert b"channels" in lib.resr_last_error()
    for b in (0, 10, 12, 32):
        assert call(im=L.ImageDesc(channels, b)) == ERR_ARG
        assert b"bits" in lib.resr_last_error()
    # RGBA: the network's batch is N colour and N alpha images
    odd = call(d=_desc(L, n=3), nbytes=0)
    if channels == 4:
        assert odd == ERR_ARG and b"odd" in lib.resr_last_error()
    else:
        assert odd == ERR_WORKSPACE
    # the alignment of y (the widest store) and of x (an RGBA pixel is one load): half the rule is refused, the rule passes on to the
    # next check, the workspace's
    sa, la = STORE_ALIGN[channels, bits], LOAD_ALIGN[channels, bits]
    assert call(y=C.c_void_p(base + sa // 2)) == ERR_ARG
    assert b"output images must be %d-byte aligned" % sa in lib.resr_last_error()
    assert call(y=C.c_void_p(base + sa), nbytes=0) == ERR_WORKSPACE
    if la > 1:
        assert call(x=C.c_void_p(base + la // 2)) == ERR_ARG
        assert b"source images must be %d-byte aligned" % la in lib.resr_last_error()
    assert call(x=C.c_void_p(base + la), nbytes=0) == ERR_WORKSPACE
    # the plan is the inference one: the same workspace, and too little of it is the float entry's code
    assert call(nbytes=ws - 1) == ERR_WORKSPACE
    assert lib.resr_compact_forward(C.byref(good), p, p, p, p, ws - 1, p, None) == ERR_WORKSPACE
    assert lib.resr_compact_workspace_bytes(C.byref(good)) == ws
    del keep


@pytest.mark.parametrize("name", ["resr_image_to_nchw", "resr_nchw_to_image"])
@pytest.mark.parametrize("channels,bits", MODES)
def test_conversion_refusals_need_no_gpu(R, name, channels, bits):
    L = R._lib
    lib = L.lib()
    fn = getattr(lib, name)
    keep, base = _fake()
    p = C.c_void_p(base)
    img = L.ImageDesc(channels, bits)
    assert fn(None, p, 1, 4, 4, C.byref(img), None) == ERR_ARG and b"null" in lib.resr_last_error()
    assert fn(p, None, 1, 4, 4, C.byref(img), None) == ERR_ARG and b"null" in lib.resr_last_error()
    assert fn(p, p, 1, 4, 4, None, None) == ERR_ARG and b"null" in lib.resr_last_error()
    for c, b, word in ((2, bits, b"channels"), (5, bits, b"channels"), (channels, 10, b"bits"), (channels, 0, b"bits")):
        assert fn(p, p, 1, 4, 4, C.byref(L.ImageDesc(c, b)), None) == ERR_ARG and word in lib.resr_last_error()
    for n, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -3, 4), (1, 4, -2)):
        assert fn(p, p, n, h, w, C.byref(img), None) == ERR_ARG, (n, h, w)
    # the image side's alignment: the load of image_to_nchw, the store of nchw_to_image; the float side's dword
    images_first = name == "resr_image_to_nchw"
    rule = (LOAD_ALIGN if images_first else STORE_ALIGN)[channels, bits]
    if rule > 1:
        off = C.c_void_p(base + rule // 2)
        assert (fn(off, p, 1, 4, 4, C.byref(img), None) if images_first else fn(p, off, 1, 4, 4, C.byref(img), None)) == ERR_ARG
        assert b"%d-byte aligned" % rule in lib.resr_last_error()
    off = C.c_void_p(base + 2)
    assert (fn(p, off, 1, 4, 4, C.byref(img), None) if images_first else fn(off, p, 1, 4, 4, C.byref(img), None)) == ERR_ARG
    assert b"float tensor" in lib.resr_last_error()
    # a grid that does not fit: 2^45 pixels
    assert fn(p, p, 32768, 32768, 32768, C.byref(img), None) == ERR_ARG and b"beyond the grid" in lib.resr_last_error()
    del keep


# ---- Python -----------------------------------------------------------------------------------------------------------------------
def test_device_functions_refuse_cpu_tensors(R):
    m = R.SRVGGNetCompact(num_conv=1, precision="fast")
    images = torch.zeros(1, 4, 4, 4, dtype=torch.uint8)
    with torch.no_grad():
        for call in (lambda: R.from_image(images), lambda: R.to_image(torch.zeros(2, 3, 4, 4), 4, torch.uint8),
                     lambda: R.upscale_image(m, images), lambda: m.forward_image(images),
                     lambda: R.upscale_image(R.Generator(3, 3, 4, n_blocks=1), images)):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call()
    with pytest.raises(RuntimeError, match="backward"):      # the guard of forward: grad mode on, parameters that require grad
        m.forward_image(images)
    for channels, dtype in ((2, torch.uint8), (5, torch.uint16), (3, torch.float32), (1, torch.int16)):
        with pytest.raises(ValueError):
            R.frames.image_desc(channels, dtype)


def test_keep_mode_parses_and_defaults_to_false(R):
    from real_esrgan_pytorch_amd import inference_frames
    p = inference_frames.get_parser()
    base = ["--inputs_dir", "D", "--output_dir", "O", "--weights_path", "W"]
    assert p.parse_args(base).keep_mode is False
    assert p.parse_args(base + ["--keep_mode"]).keep_mode is True
    assert inference_frames.KEPT_MODES == {"L": "L", "RGBA": "RGBA", "I;16": "I;16", "LA": "RGBA"}
    from PIL import Image
    for mode, kept in (("L", "L"), ("LA", "RGBA"), ("RGBA", "RGBA"), ("I;16", "I;16"), ("RGB", None), ("P", None), ("1", None), ("CMYK", None)):
        assert inference_frames.kept_mode(Image.new(mode, (3, 2))) == kept, mode
