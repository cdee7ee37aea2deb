"""GPU: the image modes of the frame path -- grey, RGB and RGBA images of 8 or 16 bits (csrc/frames.hip, frames.py, compact.py,
inference_frames.py --keep_mode).  The result is DEFINED in numpy (frames.image_to_rgb_np, grey_np, rgb_to_image_np around the
model's own fp32 forward), so every comparison here is an equality, never a tolerance."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests.frames_cases import ODD_WIDTHS, PRECISIONS, _model, float_reference, random_frames

pytestmark = pytest.mark.gpu

MODES = [(c, b) for c in (1, 3, 4) for b in (8, 16)]
MODE_IDS = {(1, 8): "grey8", (1, 16): "grey16", (3, 8): "rgb8", (3, 16): "rgb16", (4, 8): "rgba8", (4, 16): "rgba16"}
DTYPES = {8: np.uint8, 16: np.uint16}
GROUP = {(1, 8): 4, (1, 16): 4, (3, 8): 4, (3, 16): 2, (4, 8): 4, (4, 16): 2}      # output pixels per thread of the tail
SIZES = [(5, 7), (9, 12), (37, 53)]                                               # below a conv tile, ..., across tile edges


def _mode_id(m):
    return MODE_IDS[m]


def random_images(n, h, w, channels, bits, seed, squeeze=False):
    """[n,h,w,channels] (grey with squeeze: [n,h,w]) of uint8 / uint16, uniformly random, the levels 0 and top present."""
    top = (1 << bits) - 1
    a = np.random.RandomState(seed).randint(0, top + 1, size=(n, h, w, channels)).astype(DTYPES[bits])
    flat = a.reshape(-1)
    flat[0], flat[-1] = 0, top
    return a[..., 0] if squeeze and channels == 1 else a


def quantise_np(y, dtype):
    """q of the definition on an fp32 [B,3,H,W] tensor -> levels [B,H,W,3]: v * float32(top), clamp to [0, top], truncate."""
    top = np.float32(np.iinfo(dtype).max)
    v = y.detach().cpu().numpy().astype(np.float32) * top
    assert v.dtype == np.float32
    return np.ascontiguousarray(np.clip(v, np.float32(0), top).astype(dtype).transpose(0, 2, 3, 1))


def unit_np(images):
    """image_to_rgb_np(images) / top as fp32 NCHW: one IEEE division per level."""
    import real_esrgan_pytorch_amd as R
    rgb = R.image_to_rgb_np(images)
    x = rgb.astype(np.float32) / np.float32(np.iinfo(images.dtype).max)
    assert x.dtype == np.float32
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def definition(float_path, images):
    """THE DEFINITION: rgb_to_image_np(q(float_path(image_to_rgb_np(images) / top)), channels), in the shape the images came in."""
    import real_esrgan_pytorch_amd as R
    channels = 1 if images.ndim == 3 else images.shape[3]
    with torch.no_grad():
        y = float_path(torch.from_numpy(unit_np(images)).cuda())
    assert y.dtype == torch.float32 and not torch.isnan(y).any(), "the float reference holds a NaN: equality is undefined"
    out = R.rgb_to_image_np(quantise_np(y, images.dtype), channels)
    return out.reshape(out.shape[:3] + images.shape[3:])


def _same(got, ref, what=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = int((got != ref).sum())
    assert bad == 0, f"{what}: {bad} of {ref.size} words differ, first at {np.argwhere(got != ref)[:4].tolist()}"


def _forward_image(model, images):
    with torch.no_grad():
        y = model.forward_image(torch.from_numpy(images).cuda())
    torch.cuda.synchronize()
    assert y.is_contiguous()
    return y


# ---- 1. the definition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("mode", MODES, ids=_mode_id)
def test_forward_image_is_the_definition(mode, precision):
    channels, bits = mode
    top = (1 << bits) - 1
    for s, act, init in ((1, "prelu", "w4"), (2, "leakyrelu", "slopes"), (3, "relu", "default"), (4, "prelu", "w4")):
        m, _ = _model(2, s, act, precision, init)
        clamped = []
        for n in (1, 3):
            for h, w in SIZES:
                images = random_images(n, h, w, channels, bits, seed=h * w + n + s, squeeze=(n == 1))
                ref = definition(m, images)
                assert ref.shape == (n, h * s, w * s) + images.shape[3:]
                _same(_forward_image(m, images), ref, (s, n, h, w))
                clamped.append(ref.reshape(-1))
        if init == "w4":      # weights x 4 drive the output far outside [0, 1]: both clamps fire, in every channel grey is taken of
            seen = np.concatenate(clamped)
            assert (seen == 0).any() and (seen == top).any()
        # an all-0 and an all-top image; RGBA: a random colour under alpha all-0 and all-top
        h, w = 5, 7
        flat = np.stack([np.zeros((h, w, channels), DTYPES[bits]), np.full((h, w, channels), top, DTYPES[bits])])
        if channels == 4:
            under = random_images(2, h, w, 4, bits, seed=s)
            under[0, :, :, 3], under[1, :, :, 3] = 0, top
            flat = np.concatenate([flat, under])
        _same(_forward_image(m, flat), definition(m, flat), ("flat", s))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_uint8_rgb_is_forward_u8(precision):
    import real_esrgan_pytorch_amd as R
    m, _ = _model(2, 4, "prelu", precision, "slopes")
    u8 = random_frames(3, 9, 12, seed=2)
    frames = torch.from_numpy(u8).cuda()
    with torch.no_grad():
        want = m.forward_u8(frames)
        assert torch.equal(m.forward_image(frames), want)
    assert torch.equal(R.upscale_image(m, frames), want) and torch.equal(R.upscale_u8(m, frames), want)
    _same(want, float_reference(m, u8)[0])


def test_uint8_rgb_entries_are_the_3x8_image_mode():
    """The uint8-typed entries and the image entries at {3, 8} are one path: the same bytes and the same profiling ids, on the frames
    of ODD_WIDTHS (every partial 4-pixel group of the tail), through the scaled pair at outscale = s / 2 (an even and an odd output
    width) and through the generic conversions at 1x3x5."""
    import real_esrgan_pytorch_amd as R
    L = R._lib

    def both(a, b):
        """a() and b(): equal results (bit for bit), equal lists of profiling ids.  Returns (result, ids)."""
        with torch.no_grad():
            ya, yb = a(), b()
            ia, ib = _prof_ids_once(L, a), _prof_ids_once(L, b)
        assert ya.dtype == yb.dtype and ya.shape == yb.shape and torch.equal(ya.view(torch.uint8), yb.view(torch.uint8))
        assert ia == ib and len(ia) > 0, (ia, ib)
        return ya, ia

    n, h = 3, 3
    widths = set()
    for s, w in ODD_WIDTHS:
        m, _ = _model(2, s, "prelu", "fast", "slopes")
        frames = torch.from_numpy(random_frames(n, h, w, seed=w * 10 + s)).cuda()
        y, ids = both(lambda: m.forward_image(frames), lambda: m.forward_u8(frames))
        assert y.shape == (n, h * s, w * s, 3) and (ids[0], ids[-1]) == (31020, 31010 + s), ids
        if s == 1:         # (an HR frame of 3 rows is shorter than the symmetric copy r = 0.5 needs: the reference refuses it too)
            continue
        o = s / 2          # s = 3: the HR frame 9 x 9, 9 x 18, 9 x 15 -> 5 x 5, 5 x 9, 5 x 8
        y, ids = both(lambda: m.forward_image(frames, outscale=o), lambda: m.forward_u8(frames, outscale=o))
        assert y.shape == (n,) + tuple(R.output_size(h, w, s, o)) + (3,) and (ids[0], ids[-1]) == (31020, 31050 + s), ids
        widths.add(y.shape[2] % 2)
    assert widths == {0, 1}
    # the generic conversions
    frames = torch.from_numpy(random_frames(1, 3, 5, seed=1)).cuda()
    x, ids = both(lambda: R.from_image(frames), lambda: R.from_u8(frames))
    assert x.shape == (1, 3, 3, 5) and ids == [31030]
    sr = (torch.rand(1, 3, 3, 5, generator=torch.Generator().manual_seed(3)) * 2 - 0.5).cuda()
    y, ids = both(lambda: R.to_image(sr, 3, torch.uint8), lambda: R.to_u8(sr))
    assert y.shape == (1, 3, 5, 3) and ids == [31031]


# ---- 2. store groups --------------------------------------------------------------------------------------------------------------
def _odd_cases():
    """(mode, s, w) with n = 3, h = 3: neither the output width nor the output's pixel count is a multiple of the thread's group, so
    groups straddle rows and images and the last one is partial."""
    return [(mode, s, w) for mode in MODES for s, w in ODD_WIDTHS if (w * s) % GROUP[mode] and (3 * 3 * s * w * s) % GROUP[mode]]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("mode,s,w", _odd_cases(), ids=lambda v: _mode_id(v) if isinstance(v, tuple) else str(v))
def test_output_widths_off_the_store_groups(mode, s, w, precision):
    channels, bits = mode
    n, h = 3, 3
    assert (w * s) % GROUP[mode] != 0 and (n * h * s * w * s) % GROUP[mode] != 0
    m, _ = _model(2, s, "prelu", precision, "slopes")
    images = random_images(n, h, w, channels, bits, seed=w * 10 + s)
    _same(_forward_image(m, images), definition(m, images))


def test_every_mode_has_store_group_cases():
    for mode in MODES:
        cases = [c for c in _odd_cases() if c[0] == mode]
        assert len(cases) >= 4 and {s for _, s, _ in cases} == {1, 3}, (mode, cases)


# ---- 3. the generic conversions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=_mode_id)
def test_generic_conversions(mode):
    import real_esrgan_pytorch_amd as R
    channels, bits = mode
    dtype, tdtype, top = DTYPES[bits], {8: torch.uint8, 16: torch.uint16}[bits], (1 << bits) - 1
    planes = 2 if channels == 4 else 1
    n, h, w = 2, 37, 53
    images = random_images(n, h, w, channels, bits, seed=bits + channels)
    x = R.from_image(torch.from_numpy(images).cuda())
    assert x.shape == (planes * n, 3, h, w) and x.dtype == torch.float32 and x.is_contiguous()
    assert np.array_equal(x.cpu().numpy(), unit_np(images))
    if channels == 1:         # [N,H,W] is the same batch as [N,H,W,1]
        assert torch.equal(R.from_image(torch.from_numpy(images[..., 0].copy()).cuda()), x)
    # fp32 -> image: random values around and beyond [0, 1] ...
    y = (torch.rand(planes * n, 3, h, w, generator=torch.Generator().manual_seed(bits)) * 2 - 0.5).cuda()
    got = R.to_image(y, channels, tdtype)
    ref = R.rgb_to_image_np(quantise_np(y, dtype), channels)
    assert got.dtype == tdtype and got.is_contiguous()
    _same(got, ref, "to_image")
    assert (ref == 0).any() and (ref == top).any()
    # ... channels_last input is normalised, not misread ...
    assert torch.equal(R.to_image(y.to(memory_format=torch.channels_last), channels, tdtype).view(torch.uint8), got.view(torch.uint8))
    # ... and the truncation edges: k / top and its two float32 neighbours, for every k
    k = np.arange(top + 1, dtype=np.float32) / np.float32(top)
    edges = np.concatenate([k, np.nextafter(k, np.float32(np.inf)), np.nextafter(k, np.float32(-np.inf))]).astype(np.float32)
    side = 16 if bits == 8 else 256
    e = torch.from_numpy(edges.reshape(planes, 3, side // planes, side)).cuda()
    _same(R.to_image(e, channels, tdtype), R.rgb_to_image_np(quantise_np(e, dtype), channels), "edges")
    # the round trip is the identity on every level, in every channel (it holds in float32: trunc(fl(fl(k / top) * top)) == k)
    levels = np.arange((top + 1) * channels, dtype=np.int64).reshape(1, side, side, channels)
    levels = ((levels // channels + 7 * (levels % channels)) % (top + 1)).astype(dtype)
    assert all(len(np.unique(levels[..., c])) == top + 1 for c in range(channels))
    t = torch.from_numpy(levels).cuda()
    back = R.to_image(R.from_image(t), channels, tdtype)
    _same(back.reshape(levels.shape), levels, "round trip")


# ---- 4. the composition -----------------------------------------------------------------------------------------------------------
def test_upscale_image_rrdb_generator_rgba16():
    import real_esrgan_pytorch_amd as R
    torch.manual_seed(0)
    g = R.Generator(3, 3, 4, precision="exact16", n_blocks=1)
    with torch.no_grad():
        g.conv4.bias += 0.5
    g = g.cuda().eval()
    assert not hasattr(g, "forward_u8") and not hasattr(g, "forward_image")
    images = random_images(2, 20, 24, 4, 16, seed=7)
    ref = definition(g, images)
    got = R.upscale_image(g, torch.from_numpy(images).cuda())
    assert got.shape == (2, 80, 96, 4) and got.dtype == torch.uint16
    _same(got, ref)
    assert len(np.unique(ref[..., :3])) > 256 and len(np.unique(ref[..., 3])) > 256         # 16 bits are used, in colour and in alpha


@pytest.mark.parametrize("precision", ["fast", "exact16"])
def test_upscale_image_rgba8_tiled_equals_whole_frame(precision, monkeypatch):
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import tiling
    num_conv = 4
    m, _ = _model(num_conv, 4, "prelu", precision, "slopes")
    images = random_images(1, 70, 90, 4, 8, seed=3)
    t = torch.from_numpy(images).cuda()
    whole = _forward_image(m, images)
    assert torch.equal(R.upscale_image(m, t), whole)               # fits: the fused entry
    _same(whole, definition(m, images))
    monkeypatch.setattr(tiling, "_MAX_OUT_PIXELS", 48 * 90)
    assert not tiling.fits_whole(m, 2, 70, 90)
    halo = num_conv + 4
    assert halo >= m.receptive_radius
    tiles, wh, ww = tiling.TiledGenerator(m, tile=None, halo=halo, use_graph=False).plan(2, 70, 90)
    assert len(tiles) > 1 and (wh, ww) != (70, 90)
    assert torch.equal(R.upscale_image(m, t, halo=halo), whole)    # the composition, cut by the tiler


# ---- 5. fused means fused ---------------------------------------------------------------------------------------------------------
def _prof_ids_once(L, fn):
    """kernel ids of the instrumented launches of ONE call of fn()."""
    lib = L.lib()
    buf = (L.ProfEntry * 256)()
    lib.resr_profile_begin()
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        n = int(lib.resr_profile_end(C.cast(buf, C.c_void_p), 256))
    assert 0 <= n <= 256
    return [buf[k].kernel_id for k in range(n)]


@pytest.mark.parametrize("mode", MODES, ids=_mode_id)
def test_forward_image_is_one_fused_sequence(mode):
    import real_esrgan_pytorch_amd as R
    channels, bits = mode
    num_conv, s = 4, 4
    m, _ = _model(num_conv, s, "prelu", "fast")
    t = torch.from_numpy(random_images(2, 20, 24, channels, bits, seed=1)).cuda()
    with torch.no_grad():
        m.forward_image(t)
        torch.cuda.synchronize()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            m.forward_image(t)
            torch.cuda.synchronize()
        ids = _prof_ids_once(R._lib, lambda: m.forward_image(t))
    names = {e.key for e in prof.key_averages()}
    banned = {"aten::conv2d", "aten::convolution", "aten::_convolution", "aten::prelu", "aten::_prelu_kernel", "aten::pixel_shuffle",
              "aten::upsample_nearest2d", "aten::add", "aten::add_", "aten::leaky_relu", "aten::relu",
              "aten::mul", "aten::clamp", "aten::permute", "aten::div", "aten::_to_copy", "aten::cat", "aten::repeat", "aten::expand"}
    assert not names & banned, names & banned
    # the library's own records: one head, num_conv + 2 convolutions (kernel ids below 30000), one tail, and nothing else -- no
    # generic conversion (31030, 31031, 31036, 31037).  8-bit RGB runs the uint8 path's kernels, under their ids.
    head, tail = (31020, 31010 + s) if mode == (3, 8) else (31023, 31100 + s)
    assert ids[0] == head and ids[-1] == tail, ids
    assert all(k < 30000 for k in ids[1:-1]) and len(ids) == num_conv + 4, ids
    # ... while the composition shows the two generic launches around the float forward
    from real_esrgan_pytorch_amd import frames
    with torch.no_grad():
        ids = _prof_ids_once(R._lib, lambda: frames.to_image(m(frames.from_image(t)), channels, t.dtype))
    want = (31030, 31031) if mode == (3, 8) else (31036, 31037)
    assert ids[0] == want[0] and ids[-1] == want[1] and sum(1 for k in ids if k < 30000) == num_conv + 2, ids


# ---- 6. argument checks on the device ---------------------------------------------------------------------------------------------
def test_argument_checks():
    import real_esrgan_pytorch_amd as R
    m, _ = _model(2, 2, "prelu", "fast")
    ok = torch.zeros(1, 8, 8, 4, dtype=torch.uint8).cuda()
    # the guard of forward: parameters that require grad, grad mode on
    assert torch.is_grad_enabled() and any(p.requires_grad for p in m.parameters())
    with pytest.raises(RuntimeError, match="backward"):
        m.forward_image(ok)
    y = R.upscale_image(m, ok)                                 # the frame path runs it under no_grad itself
    assert y.shape == (1, 16, 16, 4) and y.dtype == torch.uint8 and not y.requires_grad
    for shape in ((2, 8, 8), (2, 8, 8, 1), (2, 8, 8, 3), (2, 8, 8, 4)):          # the trailing shape comes back as given
        for dtype in (torch.uint8, torch.uint16):
            out = R.upscale_image(m, torch.zeros(shape, dtype=dtype).cuda())
            assert out.shape == (2, 16, 16) + shape[3:] and out.dtype == dtype
    bad = [(torch.zeros(1, 8, 8, 4).cuda(), "uint8 or uint16"), (torch.zeros(1, 8, 8, 4, dtype=torch.int16).cuda(), "uint8 or uint16"),
           (torch.zeros(1, 8, 8, 2, dtype=torch.uint8).cuda(), "image batch is"), (torch.zeros(1, 8, 8, 5, dtype=torch.uint16).cuda(), "image batch is"),
           (torch.zeros(8, 8, dtype=torch.uint8).cuda(), "image batch is"),
           (torch.zeros(1, 8, 4, 8, dtype=torch.uint8).cuda().permute(0, 1, 3, 2), "contiguous"),
           (torch.zeros(1, 8, 8, 4, dtype=torch.uint8), "no CPU path")]
    with torch.no_grad():
        before = m(torch.zeros(1, 3, 8, 8).cuda()).clone()
        for images, match in bad:
            for call in (lambda: R.upscale_image(m, images), lambda: m.forward_image(images), lambda: R.from_image(images)):
                with pytest.raises(RuntimeError, match=match):
                    call()
        for sr, channels, dtype in ((torch.zeros(3, 3, 8, 8).cuda(), 4, torch.uint8), (torch.zeros(2, 4, 8, 8).cuda(), 4, torch.uint8),
                                    (torch.zeros(2, 3, 8, 8, dtype=torch.float16).cuda(), 1, torch.uint16)):
            with pytest.raises(RuntimeError, match="fp32"):
                R.to_image(sr, channels, dtype)
        for channels, dtype in ((2, torch.uint8), (5, torch.uint8), (3, torch.float32)):
            with pytest.raises(ValueError):
                R.to_image(torch.zeros(2, 3, 8, 8).cuda(), channels, dtype)
        assert torch.equal(m(torch.zeros(1, 3, 8, 8).cuda()), before)          # nothing was launched into the model's buffers
        # the uint8 RGB entries keep their own refusals
        with pytest.raises(RuntimeError, match="uint8"):
            R.upscale_u8(m, ok)
        with pytest.raises(RuntimeError, match="uint8"):
            m.forward_u8(ok)
        with pytest.raises(RuntimeError, match="uint8"):
            R.upscale_u8(m, torch.zeros(1, 8, 8, 3, dtype=torch.uint16).cuda())


def test_library_refuses_before_it_writes():
    """The refusals of the C entry with real device buffers: the output is untouched."""
    import real_esrgan_pytorch_amd as R
    L = R._lib
    m, _ = _model(2, 2, "prelu", "fast")
    images = torch.from_numpy(random_images(1, 8, 8, 4, 8, seed=0)).cuda()
    with torch.no_grad():
        m.forward_image(images)                        # packs the weights, makes the workspace of a batch of 2
    flat, ws = m.flat_parameters(), m._workspace(m._desc(2, 8, 8), images.device)
    y = torch.full((1, 16, 16, 4), 77, dtype=torch.uint8).cuda()
    base = torch.full((y.numel() + 64,), 77, dtype=torch.uint8).cuda()
    off = base[8:8 + y.numel()]                        # 8 bytes past an allocation: not 16-byte aligned
    assert off.data_ptr() % 16 == 8
    st = L.stream_ptr(images)

    def call(desc, out, img):
        return L.lib().resr_compact_forward_image(C.byref(desc), L.ptr(images), L.ptr(flat), L.ptr(m._packed), L.ptr(ws), ws.numel(), L.ptr(out),
                                                  C.byref(img), st)
    for desc, out, img in ((m._desc(2, 8, 8), y, L.ImageDesc(2, 8)), (m._desc(2, 8, 8), y, L.ImageDesc(4, 12)),
                           (m._desc(1, 8, 8), y, L.ImageDesc(4, 8)), (m._desc(2, 8, 8), off, L.ImageDesc(4, 8))):
        assert call(desc, out, img) == -1
        torch.cuda.synchronize()
        assert bool((y == 77).all()) and bool((base == 77).all())
    assert call(m._desc(2, 8, 8), y, L.ImageDesc(4, 8)) == 0
    with torch.no_grad():
        assert torch.equal(y, m.forward_image(images))


# ---- 7. the CLI -------------------------------------------------------------------------------------------------------------------
def test_directory_cli_keep_mode(tmp_path):
    from PIL import Image
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import inference_frames
    m, sd = _model(2, 4, "prelu", "strict", "slopes")
    torch.save({"params": sd}, tmp_path / "w.pth")
    lr = tmp_path / "lr"
    lr.mkdir()
    rs = np.random.RandomState(5)
    files = {"a_grey.png": rs.randint(0, 256, size=(17, 21)).astype(np.uint8),
             "b_rgb.png": rs.randint(0, 256, size=(24, 30, 3)).astype(np.uint8),
             "c_rgba.png": rs.randint(0, 256, size=(20, 26, 4)).astype(np.uint8),
             "d_grey16.png": rs.randint(0, 65536, size=(19, 23)).astype(np.uint16)}
    modes = {"a_grey.png": "L", "b_rgb.png": "RGB", "c_rgba.png": "RGBA", "d_grey16.png": "I;16"}
    for name, a in files.items():
        Image.fromarray(a).save(lr / name)
        assert Image.open(lr / name).mode == modes[name]
    args = dict(inputs_dir=str(lr), weights_path=str(tmp_path / "w.pth"), depth=2, model_type="compact", num_conv=2, act_type="prelu", precision="strict")
    inference_frames.main(types.SimpleNamespace(output_dir=str(tmp_path / "sr"), keep_mode=True, **args))
    assert sorted(p.name for p in (tmp_path / "sr").iterdir()) == sorted(files)
    for name, a in files.items():
        out = Image.open(tmp_path / "sr" / name)
        assert out.mode == modes[name], (name, out.mode)
        want = R.upscale_image(m, torch.from_numpy(a)[None].cuda())[0].cpu().numpy()
        _same(np.asarray(out), want, name)
    # without the switch nothing changes: every file leaves as RGB
    inference_frames.main(types.SimpleNamespace(output_dir=str(tmp_path / "rgb"), **args))
    for name in files:
        assert Image.open(tmp_path / "rgb" / name).mode == "RGB", name
    _same(np.asarray(Image.open(tmp_path / "rgb" / "b_rgb.png")), np.asarray(Image.open(tmp_path / "sr" / "b_rgb.png")), "rgb")
