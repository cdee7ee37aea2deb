"""GPU: outscale for the image modes -- grey, RGB and RGBA images of 8 or 16 bits through the resizing tail (csrc/image_resize.hip,
frames.py, compact.py, inference_frames.py --keep_mode --outscale).  The result is DEFINED in numpy: frames.image_to_rgb_np / top, the
model's own fp32 forward, tests/resize_ref.py's bit-exact restatement of the resize, q at top, frames.rgb_to_image_np.  Every
comparison here is an equality, never a tolerance."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import resize_ref
from tests.frames_cases import PRECISIONS, _model
from tests.test_gpu_image_modes import DTYPES, MODES, _mode_id, _prof_ids_once, _same, quantise_np, random_images, unit_np
from tests.test_gpu_outscale import OUTSCALES, SMALL_TILE_OUTSCALES, _admits
from tests.test_image_outscale_surface import _expected_plan
from tests.test_resize_surface import TILE_LIST

pytestmark = pytest.mark.gpu

FRAMES = ((37, 53), (3, 5), "smallest", (64, 96))
MODELS = {2: ("leakyrelu", "slopes"), 3: ("relu", "default"), 4: ("prelu", "w4")}      # factor -> activation, init (tests/test_gpu_compact.py)


def definition(float_path, images, s, o):
    """THE DEFINITION: rgb_to_image_np(q(resize(float_path(image_to_rgb_np(images) / top), o / s)), channels), in the shape the images
    came in.  The resize and q run in numpy."""
    import real_esrgan_pytorch_amd as R
    channels = 1 if images.ndim == 3 else images.shape[3]
    with torch.no_grad():
        y = float_path(torch.from_numpy(unit_np(images)).cuda())
    assert y.dtype == torch.float32 and not torch.isnan(y).any(), "the float reference holds a NaN: equality is undefined"
    y = y.cpu().numpy()
    r = o / s
    (iy, wy), (ix, wx) = resize_ref.band(y.shape[2], r), resize_ref.band(y.shape[3], r)
    z = resize_ref.resize_f32(y, iy, wy, ix, wx)
    assert z.dtype == np.float32 and not np.isnan(z).any()
    out = R.rgb_to_image_np(quantise_np(torch.from_numpy(z), images.dtype), channels)
    assert out.shape[1:3] == R.output_size(images.shape[1], images.shape[2], s, o)
    return out.reshape(out.shape[:3] + images.shape[3:])


def _fused(model, images, o, plan=None):
    with torch.no_grad():
        y = model.forward_image(torch.from_numpy(images).cuda(), outscale=o, plan=plan)
    torch.cuda.synchronize()
    assert y.is_contiguous()
    return y


def _equal(a, b):
    """Two image batches on the device hold the same words (grey: [N,H,W] and [N,H,W,1] are the same batch)."""
    return a.dtype == b.dtype and a.numel() == b.numel() and torch.equal(a.reshape(b.shape).view(torch.uint8), b.view(torch.uint8))


def _smallest(s, o):
    return next(h for h in range(1, 64) if _admits(h, h, s, o))


# ---- 1. the definition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("mode", MODES, ids=_mode_id)
def test_outscale_is_the_definition(mode, s, precision):
    import real_esrgan_pytorch_amd as R
    channels, bits = mode
    top = (1 << bits) - 1
    act, init = MODELS[s]
    m, _ = _model(2, s, act, precision, init)
    ran, seen = 0, []
    for o in OUTSCALES:
        if o == s:
            continue
        smallest = _smallest(s, o)
        for n in (1, 3):
            for frame in FRAMES:
                h, w = (smallest, smallest) if frame == "smallest" else frame
                assert _admits(h, w, s, o)                         # (frames the rule refuses: test_frames_below_the_rule_raise)
                images = random_images(n, h, w, channels, bits, seed=h * w + n + s, squeeze=(n == 1))
                ref = definition(m, images, s, o)
                if init == "w4":
                    seen.append(ref)
                _same(_fused(m, images, o), ref, ("forward_image", o, n, h, w))
                _same(R.upscale_image(m, torch.from_numpy(images).cuda(), outscale=o), ref, ("upscale_image", o, n, h, w))
                ran += 1
        # an all-0 and an all-top image; RGBA: a random colour under alpha all-0 and all-top
        h, w = max(5, smallest), max(7, smallest)
        flat = np.stack([np.zeros((h, w, channels), DTYPES[bits]), np.full((h, w, channels), top, DTYPES[bits])])
        if channels == 4:
            under = random_images(2, h, w, 4, bits, seed=s)
            under[0, :, :, 3], under[1, :, :, 3] = 0, top
            flat = np.concatenate([flat, under])
        _same(_fused(m, flat, o), definition(m, flat, s, o), ("flat", o))
    assert ran == len([o for o in OUTSCALES if o != s]) * 2 * len(FRAMES) >= 24
    if init == "w4":
        # asserted on the REFERENCE: weights x 4 drive the output far outside [0, 1], so both clamps fire; at 16 bits the levels are
        # 16-bit ones, in colour and in alpha
        words = np.concatenate([r.reshape(-1) for r in seen])
        assert (words == 0).any() and (words == top).any()
        colour = np.concatenate([r.reshape(r.shape[:3] + (-1,))[..., :min(channels, 3)].reshape(-1) for r in seen])
        assert bits == 8 or len(np.unique(colour)) > 256
        if channels == 4:
            assert bits == 8 or len(np.unique(np.concatenate([r[..., 3].reshape(-1) for r in seen]))) > 256


# ---- 2. small tiles: tile origins off the 4-byte grid, rows shorter than a dword -----------------------------------------------------
def _planned(h, w, s, o, channels, bits):
    """(th, tw), tiles per axis: resr_debug_image_resize_plan for LR images h x w, host only; and the restated plan it must equal."""
    import real_esrgan_pytorch_amd as R
    r = o / s
    oh, ow = R.output_size(h, w, s, o)
    ty, tx = resize_ref.band(h * s, r)[0].shape[1], resize_ref.band(w * s, r)[0].shape[1]
    out = (C.c_int32 * 6)()
    assert R._lib.lib().resr_debug_image_resize_plan(h, w, s, oh, ow, ty, tx, channels, bits, out) == 0
    assert tuple(out) == _expected_plan(h * s, w * s, oh, ow, ty, tx, channels, bits)
    return (out[0], out[1]), (-(-oh // out[0]), -(-ow // out[1]))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("mode", MODES, ids=_mode_id)
def test_small_tiles(mode, precision):
    import real_esrgan_pytorch_amd as R
    channels, bits = mode
    s = 4
    m, _ = _model(2, s, "prelu", precision, "slopes")
    tiles = set()
    for o, _ in SMALL_TILE_OUTSCALES:
        for n, h, w in ((1, 24, 24), (2, 25, 33)):
            assert _admits(h, w, s, o)
            tile, (gy, gx) = _planned(h, w, s, o, channels, bits)
            assert tile in TILE_LIST[3:] and gy >= 2 and gx >= 2, (o, h, w, tile, gy, gx)
            tiles.add(tile)
            images = random_images(n, h, w, channels, bits, seed=h * w + n)
            ref = definition(m, images, s, o)
            got = _fused(m, images, o)
            assert tuple(got.shape) == (n,) + R.output_size(h, w, s, o) + images.shape[3:]
            _same(got, ref, (o, n, h, w, tile))
    # the eight outscales reach the eight small entries of the plan's list, for this mode's staging buffer too
    assert tiles == set(TILE_LIST[3:]), sorted(tiles)


# ---- 3. fused equals composition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("mode", MODES, ids=_mode_id)
def test_fused_equals_composition(mode, precision):
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import frames, imgproc
    channels, bits = mode
    for s, o, (n, h, w) in ((4, 2, (2, 37, 53)), (4, 1.5, (1, 9, 12)), (2, 3, (3, 20, 24)), (3, 2.5, (1, 37, 53))):
        m, _ = _model(2, s, "prelu", precision, "slopes")
        images = random_images(n, h, w, channels, bits, seed=h + w + s)
        t = torch.from_numpy(images).cuda()
        plan = imgproc.ResizePlan(h * s, w * s, o / s, t.device)
        with torch.no_grad():
            want = frames.to_image(imgproc.resize_with_plan(m(frames.from_image(t)), plan), channels, t.dtype)
        got = _fused(m, images, o)
        assert tuple(got.shape) == (n, plan.out_h, plan.out_w, channels) and _equal(got, want), (s, o, n, h, w)
        assert _equal(_fused(m, images, o, plan), want)            # a caller's plan: the same call
        assert _equal(R.upscale_image(m, t, outscale=o, plan=plan), want)


@pytest.mark.parametrize("precision", ["fast", "exact16"])
def test_tiled_equals_whole_frame(precision, monkeypatch):
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import tiling
    num_conv = 4
    m, _ = _model(num_conv, 4, "prelu", precision, "slopes")
    images = random_images(1, 70, 90, 4, 8, seed=3)
    t = torch.from_numpy(images).cuda()
    whole = _fused(m, images, 2)
    assert tuple(whole.shape) == (1, 140, 180, 4)
    assert torch.equal(R.upscale_image(m, t, outscale=2), whole)               # fits: the fused entry
    _same(whole, definition(m, images, 4, 2))
    monkeypatch.setattr(tiling, "_MAX_OUT_PIXELS", 48 * 90)
    assert not tiling.fits_whole(m, 2, 70, 90)
    halo = num_conv + 4
    assert halo >= m.receptive_radius
    tiles, wh, ww = tiling.TiledGenerator(m, tile=None, halo=halo, use_graph=False).plan(2, 70, 90)
    assert len(tiles) > 1 and (wh, ww) != (70, 90)
    assert torch.equal(R.upscale_image(m, t, halo=halo, outscale=2), whole)    # the composition, cut by the tiler


def test_rrdb_generator_rgba16():
    import real_esrgan_pytorch_amd as R
    torch.manual_seed(0)
    g = R.Generator(3, 3, 4, precision="exact16", n_blocks=1)
    with torch.no_grad():
        g.conv4.bias += 0.5
    g = g.cuda().eval()
    assert not hasattr(g, "forward_u8") and not hasattr(g, "forward_image")
    images = random_images(2, 20, 24, 4, 16, seed=7)
    ref = definition(g, images, 4, 2)
    got = R.upscale_image(g, torch.from_numpy(images).cuda(), outscale=2)
    assert got.shape == (2, 40, 48, 4) and got.dtype == torch.uint16
    _same(got, ref)
    assert len(np.unique(ref[..., :3])) > 256 and len(np.unique(ref[..., 3])) > 256         # 16 bits are used, in colour and in alpha


# ---- 4. fused means fused ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=_mode_id)
def test_outscale_is_one_fused_sequence(mode):
    import real_esrgan_pytorch_amd as R
    channels, bits = mode
    num_conv, s = 4, 4
    m, _ = _model(num_conv, s, "prelu", "fast")
    t = torch.from_numpy(random_images(2, 20, 24, channels, bits, seed=1)).cuda()
    with torch.no_grad():
        m.forward_image(t, outscale=2)
        torch.cuda.synchronize()
        ids = _prof_ids_once(R._lib, lambda: m.forward_image(t, outscale=2))
    # one head, num_conv + 2 convolutions (kernel ids below 30000), one resizing tail, and nothing else: no generic conversion
    # (31036, 31037) and no resize launch of its own (31040).  8-bit RGB runs the uint8 path's kernels, under their ids.
    head, tail = (31020, 31050 + s) if mode == (3, 8) else (31023, 31110 + s)
    assert ids[0] == head and ids[-1] == tail, ids
    assert all(k < 30000 for k in ids[1:-1]) and len(ids) == num_conv + 4, ids
    # upscale_image takes the same sequence
    ids2 = _prof_ids_once(R._lib, lambda: R.upscale_image(m, t, outscale=2))
    assert ids2 == ids, (ids2, ids)


# ---- 5. pass-through -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=_mode_id)
def test_pass_through(mode):
    import real_esrgan_pytorch_amd as R
    channels, bits = mode
    s = 4
    m, _ = _model(2, s, "prelu", "fast", "slopes")
    t = torch.from_numpy(random_images(2, 9, 11, channels, bits, seed=4)).cuda()
    with torch.no_grad():
        base = m.forward_image(t)
        for o in (None, s, float(s)):                 # the unscaled call, bit for bit
            assert _equal(m.forward_image(t, outscale=o), base) and _equal(R.upscale_image(m, t, outscale=o), base), o
    assert _equal(R.upscale_image(m, t), base)
    if mode == (3, 8):                                # uint8 RGB with an outscale IS upscale_u8
        want = R.upscale_u8(m, t, outscale=2)
        assert torch.equal(R.upscale_image(m, t, outscale=2), want)
        with torch.no_grad():
            assert torch.equal(m.forward_image(t, outscale=2), want) and torch.equal(m.forward_u8(t, outscale=2), want)


# ---- 6. refusals on the device -----------------------------------------------------------------------------------------------------
def test_library_refuses_before_it_writes():
    """The refusals of the C entry with real device buffers: the output is untouched."""
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import imgproc
    L = R._lib
    m, _ = _model(2, 2, "prelu", "fast")
    images = torch.from_numpy(random_images(1, 8, 8, 4, 8, seed=0)).cuda()
    with torch.no_grad():
        want = m.forward_image(images, outscale=3)     # packs the weights, makes the workspace of a batch of 2
    plan = imgproc.ResizePlan(16, 16, 1.5, images.device)
    flat, ws = m.flat_parameters(), m._workspace(m._desc(2, 8, 8), images.device)
    y = torch.full((1, 24, 24, 4), 77, dtype=torch.uint8).cuda()
    base = torch.full((y.numel() + 64,), 77, dtype=torch.uint8).cuda()
    off = base[2:2 + y.numel()]                        # 2 bytes past an allocation: not 4-byte aligned
    assert off.data_ptr() % 4 == 2
    st = L.stream_ptr(images)

    def call(desc, out, img):
        return L.lib().resr_compact_forward_image_scaled(C.byref(desc), L.ptr(images), L.ptr(flat), L.ptr(m._packed), L.ptr(ws), ws.numel(),
                                                         L.ptr(out), *plan.args(), C.byref(img), st)
    for desc, out, img in ((m._desc(2, 8, 8), y, L.ImageDesc(2, 8)), (m._desc(2, 8, 8), y, L.ImageDesc(4, 12)),
                           (m._desc(1, 8, 8), y, L.ImageDesc(4, 8)), (m._desc(2, 8, 8), off, L.ImageDesc(4, 8))):
        assert call(desc, out, img) == -1
        torch.cuda.synchronize()
        assert bool((y == 77).all()) and bool((base == 77).all())
    assert call(m._desc(2, 8, 8), y, L.ImageDesc(4, 8)) == 0
    torch.cuda.synchronize()
    assert torch.equal(y, want)
    aligned4 = base[4:4 + y.numel()]                   # 4 bytes, not the unscaled tail's 16: the scaled tail's rule
    assert aligned4.data_ptr() % 16 == 4
    assert call(m._desc(2, 8, 8), aligned4, L.ImageDesc(4, 8)) == 0
    torch.cuda.synchronize()
    assert torch.equal(aligned4.view(1, 24, 24, 4), want) and bool((base[:4] == 77).all()) and bool((base[4 + y.numel():] == 77).all())


@pytest.mark.parametrize("mode", MODES, ids=_mode_id)
def test_frames_below_the_rule_raise(mode):
    import real_esrgan_pytorch_amd as R
    channels, bits = mode
    s, o = 4, 1.5
    m, _ = _model(2, s, "prelu", "fast")
    smallest = _smallest(s, o)
    assert smallest > 1
    tdtype = {8: torch.uint8, 16: torch.uint16}[bits]
    with torch.no_grad():
        before = m(torch.zeros(1, 3, 8, 8).cuda()).clone()
        for h in range(1, smallest):
            if _admits(h, 9, s, o):
                continue
            images = torch.zeros((1, h, 9, channels), dtype=tdtype).cuda()
            for call in (lambda: m.forward_image(images, outscale=o), lambda: R.upscale_image(m, images, outscale=o)):
                with pytest.raises(ValueError, match="symmetric copy"):
                    call()
        ok = torch.zeros((1, 8, 8, channels), dtype=tdtype).cuda()
        for bad in (0, -1, float("inf"), float("nan"), True, "2"):
            for call in (lambda: m.forward_image(ok, outscale=bad), lambda: R.upscale_image(m, ok, outscale=bad)):
                with pytest.raises(ValueError, match="outscale"):
                    call()
        assert torch.equal(m(torch.zeros(1, 3, 8, 8).cuda()), before)          # nothing was launched into the model's buffers


# ---- 7. the CLI --------------------------------------------------------------------------------------------------------------------
def test_directory_cli_keep_mode_outscale(tmp_path):
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
    inference_frames.main(types.SimpleNamespace(output_dir=str(tmp_path / "sr"), keep_mode=True, outscale=2, **args))
    assert sorted(p.name for p in (tmp_path / "sr").iterdir()) == sorted(files)
    for name, a in files.items():
        out = Image.open(tmp_path / "sr" / name)
        assert out.mode == modes[name], (name, out.mode)
        want = R.upscale_image(m, torch.from_numpy(a)[None].cuda(), outscale=2)[0].cpu().numpy()
        assert want.shape[:2] == (2 * a.shape[0], 2 * a.shape[1])
        _same(np.asarray(out), want, name)
