"""GPU: the fused YUV 4:2:0 outscale tail, 8 and 10 bits (csrc/image_resize.hip, compact.hip, frames.py).  The results are defined by
the compositions that tests/test_gpu_yuv420.py and tests/test_gpu_yuv420p10.py pin for the unfused path; here the composition is
computed in the test itself, from the numpy conversions and the existing device calls, and the fused call must give the same bytes /
words: every comparison is an equality, never a tolerance."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

from tests.frames_cases import PRECISIONS, _model
from tests.test_gpu_yuv420 import random_yuv
from tests.test_gpu_yuv420p10 import _launches, composition, random_yuv10

pytestmark = pytest.mark.gpu

LAYOUTS = {8: ("i420", "nv12"), 10: ("i420p10", "p010")}
MATRICES = ("bt601", "bt709")
ERR_ARG = -1
GENERIC_8 = {31032, 31033, 31040, 31041, 31051, 31052, 31053, 31054}      # the generic conversions, the resize, the RGB scaled tail
GENERIC_10 = {31034, 31035, 31040}

# (n, LR h, LR w, s, outscale): 3 x 3 tiles of 16 x 32 with a 4 x 4 corner and a width that is no multiple of 8; a width that is (dword
# stores all along); one tile of one 2 x 2 block pair, reflection inside it; upscaling; r = 2/3; r = 0.375 with 13 taps
ASKED = [(1, 18, 34, 4, 2), (2, 10, 12, 4, 2), (1, 2, 2, 4, 2), (3, 6, 10, 2, 3), (1, 12, 12, 3, 2), (1, 4, 12, 4, 1.5)]


def _accepted(case):
    """The reflection rule of the reference's resize (imgproc.resize_band_tables raises where it raises): a CPU check."""
    from real_esrgan_pytorch_amd import imgproc
    _, h, w, s, o = case
    try:
        for n_in in (h * s, w * s):
            imgproc.resize_band_tables(n_in, math.ceil(n_in * (o / s)), o / s)
    except ValueError:
        return False
    return True


CASES = [c for c in ASKED if _accepted(c)]


def test_enough_cases_ran():
    assert len(CASES) >= 5, CASES


def _plan(h, w, s, o):
    from real_esrgan_pytorch_amd import imgproc
    return imgproc.ResizePlan(h * s, w * s, o / s, torch.device("cuda", torch.cuda.current_device()))


def oracle(model, f, bits, layout, matrix, o, float_path=None, halo=None):
    """The composition, by the definition: numpy conversions around the RGB uint8 outscale path (8 bits) or around the float path and
    `resize_with_plan` (10 bits).  `float_path`: the model's forward unless given."""
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import imgproc
    s = model.upscale_factor
    if bits == 8:
        mid = R.upscale_u8(model, torch.from_numpy(R.yuv420_to_rgb_np(f, layout, matrix)).cuda(), halo, outscale=o)
        return R.rgb_to_yuv420_np(mid.cpu().numpy(), layout, matrix)
    h, w = f.shape[1] // 3 * 2, f.shape[2]
    plan = _plan(h, w, s, o)
    fp = float_path or model
    return composition(lambda x: imgproc.resize_with_plan(fp(x), plan), f, layout, matrix)


def _frames(bits, n, h, w, seed):
    return random_yuv(n, h, w, seed) if bits == 8 else random_yuv10(n, h, w, seed)


def _upscale(bits):
    import real_esrgan_pytorch_amd as R
    return R.upscale_yuv420 if bits == 8 else R.upscale_yuv420p10


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {want.size} samples differ, first at {np.argwhere(got != want)[:4].tolist()}"


# 1 ---- the fused call is the composition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("bits", (8, 10))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_%dx%d_x%d_o%s" % c)
def test_fused_is_the_composition(case, bits, precision):
    import real_esrgan_pytorch_amd as R
    n, h, w, s, o = case
    m, _ = _model(2, s, "prelu", precision, "slopes")
    oh, ow = R.output_size(h, w, s, o)
    f = _frames(bits, n, h, w, seed=h * w + n + s)
    assert int(f.min()) == 0 and int(f.max()) == (255 if bits == 8 else 65535)
    dev = torch.from_numpy(f).cuda()
    fwd = m.forward_yuv420 if bits == 8 else m.forward_yuv420p10
    for layout in LAYOUTS[bits]:
        for matrix in MATRICES:
            want = oracle(m, f, bits, layout, matrix, o)
            with torch.no_grad():
                got = fwd(dev, layout, matrix, outscale=o)
            torch.cuda.synchronize()
            assert got.is_contiguous() and tuple(got.shape) == (n, oh * 3 // 2, ow)
            _same(got, want, f"forward {layout} {matrix}")
            _same(_upscale(bits)(m, dev, layout, matrix, outscale=o), want, f"upscale {layout} {matrix}")     # the chooser takes this call
    # a plan the caller holds gives the same frame; one for another size is refused before any launch
    with torch.no_grad():
        held = fwd(dev, LAYOUTS[bits][1], "bt709", outscale=o, plan=_plan(h, w, s, o))
        _same(held, want, "held plan")
        with pytest.raises(ValueError, match="plan"):
            fwd(dev, outscale=o, plan=_plan(h + 2, w, s, o))


# (n, LR h, LR w, outscale of the x4 model, the even tile resize_plan chooses for the 4:2:0 tail): the small even entries of choose_tile's
# list, which the cases above (16 x 32 and larger) never reach; several tiles per axis and outputs that are no multiple of the tile
# (2 x 2 divides every 4:2:0 frame)
SMALL_TILES = [(1, 28, 30, 1.2, (8, 16)), (1, 24, 24, 0.8, (8, 8)), (1, 32, 36, 0.6, (4, 8)), (2, 24, 28, 0.5, (4, 4)), (1, 24, 24, 0.4, (2, 4)),
               (1, 24, 24, 0.32, (2, 2))]
SMALL_LAYOUT = {8: "nv12", 10: "i420p10"}      # one semi-planar, one planar


@pytest.mark.parametrize("bits", (8, 10))
@pytest.mark.parametrize("case", SMALL_TILES, ids=lambda c: "n%d_%dx%d_o%s_tile%dx%d" % (c[:4] + c[4]))
def test_fused_is_the_composition_on_the_small_tiles(case, bits):
    import real_esrgan_pytorch_amd as R
    from tests import resize_ref
    n, h, w, o, tile = case
    s = 4
    assert _accepted((n, h, w, s, o))
    oh, ow = R.output_size(h, w, s, o)
    ty, tx = (resize_ref.band(v * s, o / s)[0].shape[1] for v in (h, w))
    plan = resize_ref.plan_of(R._lib.lib(), n, 3, h * s, w * s, oh, ow, ty, tx, resize_ref.YUV8 if bits == 8 else resize_ref.YUV10)
    assert plan is not None and (plan.th, plan.tw) == tile, (case, bits, plan)
    assert -(-oh // plan.th) >= 2 and -(-ow // plan.tw) >= 2 and (tile == (2, 2) or oh % plan.th or ow % plan.tw)
    m, _ = _model(2, s, "prelu", "fast", "slopes")
    f = _frames(bits, n, h, w, seed=h * w + n + s)
    dev = torch.from_numpy(f).cuda()
    layout = SMALL_LAYOUT[bits]
    want = oracle(m, f, bits, layout, "bt709", o)
    with torch.no_grad():
        got = (m.forward_yuv420 if bits == 8 else m.forward_yuv420p10)(dev, layout, "bt709", outscale=o)      # the fused tail: the method has no other path
    torch.cuda.synchronize()
    assert got.is_contiguous() and tuple(got.shape) == (n, oh * 3 // 2, ow)
    _same(got, want, f"forward {layout} o={o} tile {tile}")
    assert len(np.unique(want)) > 16


# 2 ---- the fused kernels ran -----------------------------------------------------------------------------------------------------
def test_the_fused_kernels_ran():
    import real_esrgan_pytorch_amd as R
    m, _ = _model(2, 4, "prelu", "fast", "slopes")
    f = torch.from_numpy(random_yuv(1, 12, 18, seed=1)).cuda()
    n, ids = _launches(lambda: R.upscale_yuv420(m, f, outscale=2))
    # the YUV head, the convs, the x4 8-bit scaled YUV tail: one launch sequence
    assert n == len(ids) and ids[0] == 31021 and ids[-1] == 31074 and not GENERIC_8 & set(ids), ids
    n0, ids0 = _launches(lambda: R.upscale_yuv420(m, f))
    assert n == n0 and ids[:-1] == ids0[:-1] and ids0[-1] == 31044, (ids, ids0)          # the launches of the x4 call, another tail
    f10 = torch.from_numpy(random_yuv10(1, 12, 18, seed=1)).cuda()
    n, ids = _launches(lambda: R.upscale_yuv420p10(m, f10, "p010", outscale=2))
    assert n == len(ids) == n0 and ids[0] == 31022 and ids[-1] == 31084 and not GENERIC_10 & set(ids), ids
    m3, _ = _model(2, 3, "prelu", "fast", "slopes")
    assert _launches(lambda: R.upscale_yuv420p10(m3, f10, outscale=2))[1][-1] == 31083


# 3 ---- the composition is still taken where it must be ----------------------------------------------------------------------------
@pytest.mark.parametrize("bits", (8, 10))
def test_rrdb_generator_composes(bits):
    import real_esrgan_pytorch_amd as R
    torch.manual_seed(0)
    g = R.Generator(3, 3, 4, precision="exact16", n_blocks=1)
    with torch.no_grad():
        g.conv4.bias += 0.5
    g = g.cuda().eval()
    f = _frames(bits, 2, 20, 24, seed=7)
    dev = torch.from_numpy(f).cuda()
    first, resize, last = (31032, 31041, 31033) if bits == 8 else (31034, 31040, 31035)
    for layout in LAYOUTS[bits]:
        n, ids = _launches(lambda: _upscale(bits)(g, dev, layout, "bt709", outscale=2))
        assert ids[0] == first and ids[-1] == last and resize in ids, ids
        got = _upscale(bits)(g, dev, layout, "bt709", outscale=2)
        assert tuple(got.shape) == (2, 60, 48)
        _same(got, oracle(g, f, bits, layout, "bt709", 2), layout)


@pytest.mark.parametrize("bits", (8, 10))
def test_tiled_frame_composes(monkeypatch, bits):
    from real_esrgan_pytorch_amd import tiling
    m, _ = _model(2, 2, "prelu", "fast", "slopes")
    f = _frames(bits, 1, 40, 48, seed=5)
    dev = torch.from_numpy(f).cuda()
    up = _upscale(bits)
    layout = LAYOUTS[bits][1]
    whole = up(m, dev, layout, outscale=1)                                    # r = 0.5: fits one call, the fused tail
    assert tuple(whole.shape) == (1, 60, 48)
    _same(whole, oracle(m, f, bits, layout, "bt601", 1), "whole")
    monkeypatch.setattr(tiling, "_MAX_OUT_PIXELS", 28 * 48)                    # the frame no longer fits one call: the tiler cuts it
    assert not tiling.fits_whole(m, 1, 40, 48)
    halo = m.receptive_radius + 2
    first, resize, last = (31032, 31041, 31033) if bits == 8 else (31034, 31040, 31035)
    n, ids = _launches(lambda: up(m, dev, layout, halo=halo, outscale=1))
    assert ids[0] == first and ids[-1] == last and resize in ids and not {31021, 31022, 31072, 31082} & set(ids), ids
    got = up(m, dev, layout, halo=halo, outscale=1)
    _same(got, oracle(m, f, bits, layout, "bt601", 1, float_path=lambda x: tiling.super_resolve(m, x, halo), halo=halo), "tiled")
    # with the halo of the receptive field the tiled float frame is the whole one, hence the fused call's samples
    _same(got, whole.cpu().numpy(), "tiled == whole")


@pytest.mark.parametrize("bits", (8, 10))
def test_a_scale_without_an_even_tile_composes(bits):
    """36 x 36 through the x2 model to 4 x 4: r = 1/18, 74 taps.  The staged region is the whole 72 x 72 frame; with the two rows of
    intermediate of an even tile it passes 64 KB, with the one row of the RGB tail's 1 x 1 tile it does not."""
    import real_esrgan_pytorch_amd as R
    m, _ = _model(2, 2, "prelu", "fast", "slopes")
    o = 1 / 9
    assert R.output_size(36, 36, 2, o) == (4, 4)
    plan = _plan(36, 36, 2, o)
    assert (plan.taps_y, plan.taps_x) == (74, 74)
    assert R._lib.lib().resr_compact_yuv420_scaled_fits(36, 36, 2, 4, 4, 74, 74, bits) == 0
    f = _frames(bits, 1, 36, 36, seed=9)
    dev = torch.from_numpy(f).cuda()
    layout = LAYOUTS[bits][0]
    first, resize, last = (31032, 31052, 31033) if bits == 8 else (31034, 31040, 31035)    # (8 bits: the RGB scaled tail does fit)
    n, ids = _launches(lambda: _upscale(bits)(m, dev, layout, outscale=o))
    assert ids[0] == first and ids[-1] == last and resize in ids, ids
    got = _upscale(bits)(m, dev, layout, outscale=o)
    assert tuple(got.shape) == (1, 6, 4)
    _same(got, oracle(m, f, bits, layout, "bt601", o), "composed")
    fwd = m.forward_yuv420 if bits == 8 else m.forward_yuv420p10
    with pytest.raises(RuntimeError, match="footprint"), torch.no_grad():      # the method itself has no other path
        fwd(dev, layout, outscale=o)


# 4 ---- FrameStream ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pix_fmt", ("nv12", "p010"))
def test_frame_stream_outscale(pix_fmt):
    import real_esrgan_pytorch_amd as R
    bits = 8 if pix_fmt == "nv12" else 10
    m, _ = _model(2, 4, "prelu", "fast", "slopes")
    sizes = [(12, 16), (6, 10)]
    frames = [_frames(bits, 1, *sizes[i % 2], seed=i)[0] for i in range(5)]     # two alternating sizes: every submit reallocates
    want = [_upscale(bits)(m, torch.from_numpy(f)[None].cuda(), pix_fmt, "bt709", outscale=2)[0].cpu().numpy() for f in frames]
    for f, w in zip(frames[:2], want[:2]):
        _same(w[None], oracle(m, f[None], bits, pix_fmt, "bt709", 2), "single call")
    with R.FrameStream(m, depth=2, pix_fmt=pix_fmt, matrix="bt709", outscale=2) as fs:
        n, ids = _launches(lambda: list(fs.map(frames[:1])))
        assert ids[-1] == (31074 if bits == 8 else 31084), ids                 # the stream runs the fused call
        got = list(fs.map(frames))
        assert [g.shape for g in got] == [(36, 32), (18, 20)] * 2 + [(36, 32)]
        assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))
        views = [v.copy() for v in fs.map(frames, copy=False)]                 # (a view is valid until its slot is submitted to again)
        assert all(np.array_equal(g, w) for g, w in zip(views, want))


# 5 ---- the rawvideo CLI ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pix_fmt,layout", [("yuv420p", "i420"), ("p010le", "p010")])
def test_inference_rawvideo_outscale(tmp_path, pix_fmt, layout):
    from real_esrgan_pytorch_amd import inference_rawvideo
    bits = 8 if layout == "i420" else 10
    m, sd = _model(4, 4, "prelu", "strict", "slopes")
    torch.save({"params": sd}, tmp_path / "w.pth")
    frames = _frames(bits, 3, 6, 8, seed=11)                                    # three 8x6 frames
    word = "u1" if bits == 8 else "<u2"
    (tmp_path / "in.yuv").write_bytes(frames.astype(word).tobytes())
    args = types.SimpleNamespace(input=str(tmp_path / "in.yuv"), output=str(tmp_path / "out.yuv"), size="8x6", pix_fmt=pix_fmt,
                                 matrix="bt601", weights_path=str(tmp_path / "w.pth"), model_type="compact", num_conv=4,
                                 act_type="prelu", precision="strict", depth=2, outscale=2.0)
    assert inference_rawvideo.main(args) == 3
    want = b"".join(_upscale(bits)(m, torch.from_numpy(f)[None].cuda(), layout, outscale=2)[0].cpu().numpy().astype(word).tobytes()
                    for f in frames)
    got = (tmp_path / "out.yuv").read_bytes()
    assert len(got) == 3 * 16 * 12 * 3 // 2 * (bits // 8 + (bits > 8)) and got == want


# 6 ---- the C entries refuse before any launch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", (8, 10))
def test_c_abi_refuses_before_any_launch(bits):
    import real_esrgan_pytorch_amd as R
    L = R._lib
    lib = L.lib()
    m, _ = _model(2, 2, "prelu", "fast")
    dtype = torch.uint8 if bits == 8 else torch.uint16
    src = torch.zeros(4096, dtype=dtype).cuda()
    dst = torch.zeros(4096, dtype=dtype).cuda()
    ok = R.frames.yuv_desc("i420", "bt601") if bits == 8 else R.frames.yuv10_desc("i420p10", "bt601")
    other = R.frames.yuv10_desc("p010", "bt601") if bits == 8 else R.frames.yuv_desc("nv12", "bt601")
    bad_layout = L.YuvDesc(7, ok.fq, ok.iq)
    st = L.stream_ptr(src)
    fwd = getattr(lib, "resr_compact_forward_yuv420_scaled" if bits == 8 else "resr_compact_forward_yuv420p10_scaled")
    with torch.no_grad():
        (m.forward_yuv420 if bits == 8 else m.forward_yuv420p10)(torch.zeros(1, 12, 8, dtype=dtype).cuda(), outscale=1)   # packs, builds a workspace
    desc = m._desc(1, 8, 8)
    ws = m._workspace(desc, src.device)
    plan = _plan(8, 8, 2, 1)                                                   # 16 x 16 -> 8 x 8
    tabs = list(plan.args())                                                   # oh, ow, idx_y, w_y, taps_y, idx_x, w_x, taps_x

    def call(d=desc, ends=None, t=None, q=ok):
        e = ends or [L.ptr(src), L.ptr(m._flat), L.ptr(m._packed), L.ptr(ws), ws.numel(), L.ptr(dst)]
        return fwd(C.byref(d) if d is not None else None, *e, *(t or tabs), C.byref(q) if q is not None else None, st)

    def calls():
        for h, w in ((7, 8), (8, 7)):
            assert call(d=m._desc(1, h, w)) == ERR_ARG
        for i, v in ((0, 7), (1, 9)):                                          # an odd oh, an odd ow
            t = list(tabs)
            t[i] = v
            assert call(t=t) == ERR_ARG
            assert b"even" in lib.resr_last_error()
        assert call(q=other) == ERR_ARG and call(q=bad_layout) == ERR_ARG and call(q=None) == ERR_ARG and call(d=None) == ERR_ARG
        base = [L.ptr(src), L.ptr(m._flat), L.ptr(m._packed), L.ptr(ws), ws.numel(), L.ptr(dst)]
        for hole in (0, 1, 2, 3, 5):
            e = list(base)
            e[hole] = None
            assert call(ends=e) == ERR_ARG
        for hole in (2, 3, 5, 6):                                              # a null table
            t = list(tabs)
            t[hole] = None
            assert call(t=t) == ERR_ARG
        for i, v in ((4, 0), (7, 0), (4, 4097), (7, -1)):                      # bad taps
            t = list(tabs)
            t[i] = v
            assert call(t=t) == ERR_ARG
        e = list(base)
        e[5] = C.c_void_p(dst.data_ptr() + 2)                                  # rows leave as dwords
        assert call(ends=e) == ERR_ARG
        assert b"aligned" in lib.resr_last_error()
    assert _launches(calls)[0] == 0
    assert _launches(lambda: L.check(call(), "scaled"))[0] > 0                 # (the good call does launch, and the counter counts it)
