"""GPU: mixed frame formats -- a source and a destination pixel format of their own (csrc/frames.hip, image_resize.hip, compact.hip,
frames.py, compact.py, inference_rawvideo.py).  For a source A and a destination B the result is DEFINED as

    encode_B(q_B(float_path(decode_A(f) / top_A)))          q_B(v) = trunc(clamp(v * top_B, 0, top_B)) in fp32

with the numpy conversions of frames.py at both ends (tests/test_mixed_formats_surface.py holds the same helper on the host): every
comparison here is an equality, never a tolerance."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests.frames_cases import PRECISIONS, _model
from tests.test_gpu_yuv420 import random_yuv
from tests.test_gpu_yuv420_outscale import CASES, oracle
from tests.test_gpu_yuv420p10 import _launches, random_yuv10

pytestmark = pytest.mark.gpu

ERR_ARG = -1
# 8 -> 10 and 10 -> 8 across planar and semi-planar; the same depth with the layout changed; the same layout with the matrix changed
PAIRS = [(("nv12", "bt601"), ("i420p10", "bt601")), (("i420", "bt709"), ("p010", "bt709")), (("p010", "bt601"), ("i420", "bt601")),
         (("i420p10", "bt709"), ("nv12", "bt709")), (("nv12", "bt601"), ("i420", "bt601")), (("p010", "bt709"), ("i420p10", "bt709")),
         (("i420", "bt601"), ("i420", "bt709")), (("p010", "bt709"), ("p010", "bt601"))]
SCALED_PAIRS = [(("nv12", "bt601"), ("p010", "bt709")), (("i420p10", "bt601"), ("i420", "bt601"))]
GENERIC = {31030, 31031, 31032, 31033, 31034, 31035}                                   # the generic conversions
SAME_TAILS = {31040 + s for s in (1, 2, 3, 4)} | {31060 + s for s in (1, 2, 3, 4)} | {31070 + s for s in (1, 2, 3, 4)} | {31080 + s for s in (1, 2, 3, 4)}
HEAD = {8: 31021, 10: 31022}


def _fmt(pair):
    import real_esrgan_pytorch_amd as R
    return R.frames.frame_format(pair, "test")


def _random(pair, n, h, w, seed):
    """Frames of the pair's format, random over all words (random_yuv / random_yuv10); rgb24: random bytes [n,h,w,3]."""
    f = _fmt(pair).fmt
    if f.layout is None:
        return np.random.RandomState(seed).randint(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    return random_yuv(n, h, w, seed) if f.bits == 8 else random_yuv10(n, h, w, seed)


def dev(a):
    return torch.from_numpy(a).cuda()


def definition(float_path, f, src, dst):
    """The definition: numpy conversions around `float_path` (fp32 NCHW on the device -> fp32 NCHW)."""
    import real_esrgan_pytorch_amd as R
    a, b = _fmt(src), _fmt(dst)
    if a.fmt.layout is None:
        rgb = f
    else:
        rgb = (R.yuv420_to_rgb_np if a.fmt.bits == 8 else R.yuv420p10_to_rgb_np)(f, a.pix_fmt, a.matrix)
    x = np.ascontiguousarray((rgb.astype(np.float32) / np.float32(a.fmt.top)).transpose(0, 3, 1, 2))      # one IEEE division per sample
    with torch.no_grad():
        v = float_path(dev(x)).cpu().numpy()
    assert v.dtype == np.float32
    top = np.float32(b.fmt.top)
    q = np.ascontiguousarray(np.clip(v * top, np.float32(0), top).astype(b.fmt.np_dtype).transpose(0, 2, 3, 1))
    if b.fmt.layout is None:
        return q
    return (R.rgb_to_yuv420_np if b.fmt.bits == 8 else R.rgb_to_yuv420p10_np)(q, b.pix_fmt, b.matrix)


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {want.size} samples differ, first at {np.argwhere(got != want)[:4].tolist()}"


def _equal(a, b):
    """torch.equal for the frame dtypes (uint16 compared as its bits)."""
    if a.dtype == torch.uint16:
        a, b = a.view(torch.int16), b.view(torch.int16)
    return a.dtype == b.dtype and torch.equal(a, b)


def _plan(h, w, s, o):
    from real_esrgan_pytorch_amd import imgproc
    return imgproc.ResizePlan(h * s, w * s, o / s, torch.device("cuda", torch.cuda.current_device()))


# 1 ---- the fused entry is the composition --------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n,h,w,s", [(2, 4, 6, 4), (1, 6, 10, 3), (3, 2, 2, 1), (1, 4, 4, 2), (2, 2, 6, 2)],
                         ids=["wide24", "narrow30", "edge2", "wide8", "narrow12"])
def test_forward_yuv420_mixed_is_the_composition(n, h, w, s, precision):
    import real_esrgan_pytorch_amd as R
    m, _ = _model(2, s, "prelu", precision, "slopes")
    for src, dst in PAIRS:
        f = _random(src, n, h, w, seed=h * w + n + s)
        assert int(f.min()) == 0 and int(f.max()) == (255 if _fmt(src).fmt.bits == 8 else 65535)
        d = dev(f)
        with torch.no_grad():
            got = m.forward_yuv420_mixed(d, src, dst)
        torch.cuda.synchronize()
        assert got.is_contiguous() and got.dtype == _fmt(dst).fmt.torch_dtype and tuple(got.shape) == (n, h * s * 3 // 2, w * s)
        _same(got, definition(m, f, src, dst), f"forward_yuv420_mixed {src} -> {dst}")
        assert _equal(R.upscale_frames(m, d, src, dst), got), (src, dst)                  # fits: the chooser takes the fused entry


# 2 ---- with outscale -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_%dx%d_x%d_o%s" % c)
def test_outscale_is_the_composition(case, precision):
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import imgproc
    n, h, w, s, o = case
    m, _ = _model(2, s, "prelu", precision, "slopes")
    oh, ow = R.output_size(h, w, s, o)
    plan = _plan(h, w, s, o)
    for src, dst in SCALED_PAIRS:
        f = _random(src, n, h, w, seed=h * w + n + s)
        d = dev(f)
        want = definition(lambda x: imgproc.resize_with_plan(m(x), plan), f, src, dst)
        with torch.no_grad():
            got = m.forward_yuv420_mixed(d, src, dst, outscale=o)
        torch.cuda.synchronize()
        assert got.is_contiguous() and tuple(got.shape) == (n, oh * 3 // 2, ow)
        _same(got, want, f"forward_yuv420_mixed {src} -> {dst} outscale {o}")
        _same(R.upscale_frames(m, d, src, dst, outscale=o), want, "upscale_frames")
        with torch.no_grad():
            _same(m.forward_yuv420_mixed(d, src, dst, outscale=o, plan=plan), want, "held plan")
            with pytest.raises(ValueError, match="plan"):
                m.forward_yuv420_mixed(d, src, dst, outscale=o, plan=_plan(h + 2, w, s, o))


# 3 ---- the fused kernels ran -------------------------------------------------------------------------------------------------------
def test_the_fused_mixed_kernels_ran():
    import real_esrgan_pytorch_amd as R
    m, _ = _model(2, 4, "prelu", "fast", "slopes")
    f8, f10 = dev(random_yuv(1, 12, 18, seed=1)), dev(random_yuv10(1, 12, 18, seed=1))
    n0, ids0 = _launches(lambda: R.upscale_yuv420(m, f8, "nv12"))
    for f, src, dst in ((f8, ("nv12", "bt601"), ("p010", "bt709")), (f10, ("i420p10", "bt601"), ("i420", "bt601")),
                        (f8, ("nv12", "bt601"), ("i420", "bt601"))):
        bits = _fmt(src).fmt.bits
        n, ids = _launches(lambda: R.upscale_frames(m, f, src, dst))
        # the source's head, the convs of the same-format call, the x4 mixed tail: one launch sequence
        assert n == len(ids) == n0 and ids[0] == HEAD[bits] and ids[-1] == 31094 and ids[1:-1] == ids0[1:-1], (src, dst, ids)
        assert not (GENERIC | SAME_TAILS) & set(ids), ids
        n, ids = _launches(lambda: R.upscale_frames(m, f, src, dst, outscale=2))
        assert n == len(ids) == n0 and ids[0] == HEAD[bits] and ids[-1] == 31099 and not (GENERIC | SAME_TAILS | {31040, 31094}) & set(ids), ids
    m3, _ = _model(2, 3, "prelu", "fast", "slopes")
    assert _launches(lambda: R.upscale_frames(m3, f8, ("i420", "bt601"), ("i420p10", "bt601")))[1][-1] == 31093
    assert _launches(lambda: R.upscale_frames(m3, f10, ("p010", "bt601"), ("nv12", "bt601"), outscale=2))[1][-1] == 31098


# 4 ---- the same format through the new entry ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,n,h,w,s", [("i420", 2, 4, 6, 4), ("nv12", 1, 4, 4, 2), ("i420p10", 1, 6, 10, 3), ("p010", 2, 2, 6, 2)])
def test_same_format_through_the_mixed_entry(layout, n, h, w, s):
    import real_esrgan_pytorch_amd as R
    m, _ = _model(2, s, "prelu", "fast", "slopes")
    bits = R.PIXEL_FORMATS[layout].bits
    A = (layout, "bt709")
    f = _random(A, n, h, w, seed=h * w + n)
    d = dev(f)
    same = m.forward_yuv420 if bits == 8 else m.forward_yuv420p10
    with torch.no_grad():
        want = same(d, layout, "bt709")
        n0, ids0 = _launches(lambda: same(d, layout, "bt709"))
        got = m.forward_yuv420_mixed(d, A, A)
        n1, ids1 = _launches(lambda: m.forward_yuv420_mixed(d, A, A))
    assert _equal(got, want)
    # no new instance is reached: the launch ids are the same-format ones
    assert (n1, ids1) == (n0, ids0) and ids1[-1] == (31040 if bits == 8 else 31060) + s, (ids0, ids1)
    assert _equal(R.upscale_frames(m, d, A), want) and _equal(R.upscale_frames(m, d, A, A), want)
    # ... and with outscale (12 x 18, a result that stays even): the existing composition, the existing scaled tail
    o = s / 2 if s % 2 == 0 else 2 * s
    f2 = _random(A, 1, 12, 18, seed=s)
    d2 = dev(f2)
    with torch.no_grad():
        n2, ids2 = _launches(lambda: m.forward_yuv420_mixed(d2, A, A, outscale=o))
        _same(m.forward_yuv420_mixed(d2, A, A, outscale=o), oracle(m, f2, bits, layout, "bt709", o), "same format, outscale")
    assert ids2[-1] == (31070 if bits == 8 else 31080) + s, ids2


# 5 ---- the compositions ------------------------------------------------------------------------------------------------------------
def test_rrdb_generator_composes():
    import real_esrgan_pytorch_amd as R
    torch.manual_seed(0)
    g = R.Generator(3, 3, 4, precision="exact16", n_blocks=1)
    with torch.no_grad():
        g.conv4.bias += 0.5
    g = g.cuda().eval()
    assert not hasattr(g, "forward_yuv420_mixed")
    src, dst = ("nv12", "bt601"), ("p010", "bt709")
    f = _random(src, 2, 20, 24, seed=7)
    n, ids = _launches(lambda: R.upscale_frames(g, dev(f), src, dst))
    assert ids[0] == 31032 and ids[1] == 31030 and ids[-1] == 31035, ids                 # yuv420_to_rgb + from_u8 ... to_yuv420p10
    got = R.upscale_frames(g, dev(f), src, dst)
    assert tuple(got.shape) == (2, 120, 96) and got.dtype == torch.uint16
    _same(got, definition(g, f, src, dst), "RRDB 8 -> 10")


def test_tiled_frame_composes(monkeypatch):
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import imgproc, tiling
    m, _ = _model(2, 2, "prelu", "fast", "slopes")
    src, dst = ("p010", "bt601"), ("i420", "bt709")
    f = _random(src, 1, 40, 48, seed=5)
    d = dev(f)
    whole = R.upscale_frames(m, d, src, dst, outscale=1)                      # r = 0.5: fits one call, the fused mixed tail
    assert tuple(whole.shape) == (1, 60, 48)
    plan = _plan(40, 48, 2, 1)
    _same(whole, definition(lambda x: imgproc.resize_with_plan(m(x), plan), f, src, dst), "whole")
    monkeypatch.setattr(tiling, "_MAX_OUT_PIXELS", 28 * 48)                    # the frame no longer fits one call: the tiler cuts it
    assert not tiling.fits_whole(m, 1, 40, 48)
    halo = m.receptive_radius + 2
    n, ids = _launches(lambda: R.upscale_frames(m, d, src, dst, halo=halo, outscale=1))
    # from_yuv420p10 ... the resize with uint8 output, rgb_to_yuv420; neither head, no fused tail
    assert ids[0] == 31034 and ids[-2:] == [31041, 31033] and not {31021, 31022, 31092, 31097} & set(ids), ids
    got = R.upscale_frames(m, d, src, dst, halo=halo, outscale=1)
    _same(got, definition(lambda x: imgproc.resize_with_plan(tiling.super_resolve(m, x, halo), plan), f, src, dst), "tiled")
    _same(got, whole.cpu().numpy(), "tiled == whole")                          # the halo of the receptive field: the whole frame's floats
    n, ids = _launches(lambda: R.upscale_frames(m, d, src, dst, halo=halo))    # ... and without outscale
    assert ids[0] == 31034 and ids[-2:] == [31031, 31033], ids
    _same(R.upscale_frames(m, d, src, dst, halo=halo), definition(lambda x: tiling.super_resolve(m, x, halo), f, src, dst), "tiled x2")


def test_a_scale_without_an_even_tile_composes():
    """36 x 36 through the x2 model to 4 x 4: r = 1/18, 74 taps -- no even tile fits (tests/test_gpu_yuv420_outscale.py)."""
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import imgproc
    m, _ = _model(2, 2, "prelu", "fast", "slopes")
    o = 1 / 9
    plan = _plan(36, 36, 2, o)
    assert R.output_size(36, 36, 2, o) == (4, 4) and (plan.taps_y, plan.taps_x) == (74, 74)
    for src, dst, first, last in ((("i420", "bt601"), ("i420p10", "bt709"), [31032, 31030], [31040, 31035]),
                                  (("p010", "bt601"), ("nv12", "bt601"), [31034], [31041, 31033])):
        assert R._lib.lib().resr_compact_yuv420_scaled_fits(36, 36, 2, 4, 4, 74, 74, _fmt(dst).fmt.bits) == 0
        f = _random(src, 1, 36, 36, seed=9)
        d = dev(f)
        n, ids = _launches(lambda: R.upscale_frames(m, d, src, dst, outscale=o))
        assert ids[:len(first)] == first and ids[-2:] == last, ids
        got = R.upscale_frames(m, d, src, dst, outscale=o)
        assert tuple(got.shape) == (1, 6, 4)
        _same(got, definition(lambda x: imgproc.resize_with_plan(m(x), plan), f, src, dst), "composed")
        with pytest.raises(RuntimeError, match="footprint"), torch.no_grad():      # the method itself has no other path
            m.forward_yuv420_mixed(d, src, dst, outscale=o)


@pytest.mark.parametrize("src,dst,first,last", [("rgb24", ("nv12", "bt709"), 31030, 31033), (("p010", "bt601"), "rgb24", 31034, 31031)])
def test_rgb24_on_one_side_composes(src, dst, first, last):
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import imgproc
    m, _ = _model(2, 2, "prelu", "exact16", "slopes")
    f = _random(src, 2, 6, 10, seed=3)
    d = dev(f)
    n, ids = _launches(lambda: R.upscale_frames(m, d, src, dst))
    assert ids[0] == first and ids[-1] == last and not {31020, 31021, 31022} & set(ids), ids      # generic conversions at both ends
    got = R.upscale_frames(m, d, src, dst)
    assert tuple(got.shape) == ((2, 18, 20) if dst != "rgb24" else (2, 12, 20, 3)) and got.dtype == torch.uint8
    _same(got, definition(m, f, src, dst), "rgb24 on a side")
    plan = _plan(6, 10, 2, 3)
    n, ids = _launches(lambda: R.upscale_frames(m, d, src, dst, outscale=3))
    assert ids[0] == first and ids[-1] == (last if dst != "rgb24" else 31041), ids
    _same(R.upscale_frames(m, d, src, dst, outscale=3), definition(lambda x: imgproc.resize_with_plan(m(x), plan), f, src, dst), "outscale 3")


# 6 ---- FrameStream and the rawvideo CLI ------------------------------------------------------------------------------------------------
def test_frame_stream_mixed():
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import imgproc
    m, _ = _model(2, 4, "prelu", "fast", "slopes")
    src, dst = ("nv12", "bt601"), ("p010", "bt709")
    frames = [random_yuv(1, 12, 16, seed=i)[0] for i in range(3)]
    plan = _plan(12, 16, 4, 2)
    want = [definition(lambda x: imgproc.resize_with_plan(m(x), plan), f[None], src, dst)[0] for f in frames]
    with R.FrameStream(m, 2, outscale=2, pix_fmt="nv12", matrix="bt601", out_pix_fmt="p010", out_matrix="bt709") as fs:
        n, ids = _launches(lambda: list(fs.map(frames[:1])))
        assert ids[0] == 31021 and ids[-1] == 31099, ids                           # the stream runs the fused mixed call
        got = list(fs.map(frames))
        assert [g.shape for g in got] == [(36, 32)] * 3 and all(g.dtype == np.uint16 for g in got)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        views = [v.copy() for v in fs.map(frames, copy=False)]                     # (a view is valid until its slot is submitted to again)
        assert all(np.array_equal(g, w) for g, w in zip(views, want))
        with pytest.raises(ValueError, match="uint8"):                             # a frame of the output's words is no input
            fs.submit(np.zeros((18, 16), np.uint16))


def test_inference_rawvideo_mixed(tmp_path, capsys):
    from real_esrgan_pytorch_amd import inference_rawvideo
    m, sd = _model(4, 4, "prelu", "strict", "slopes")
    torch.save({"params": sd}, tmp_path / "w.pth")
    frames = random_yuv(2, 6, 8, seed=11)                                        # two 8x6 frames of 72 bytes
    (tmp_path / "in.yuv").write_bytes(frames.tobytes())
    args = types.SimpleNamespace(input=str(tmp_path / "in.yuv"), output=str(tmp_path / "out.yuv"), size="8x6", pix_fmt="yuv420p",
                                 matrix="bt601", out_pix_fmt="p010le", out_matrix=None, weights_path=str(tmp_path / "w.pth"),
                                 model_type="compact", num_conv=4, act_type="prelu", precision="strict", depth=2, outscale=None)
    assert inference_rawvideo.main(args) == 2
    assert f"Output size 32x24 (p010le, {32 * 24 * 3} bytes per frame)" in capsys.readouterr().out
    want = definition(m, frames, ("i420", "bt601"), ("p010", "bt601"))
    got = (tmp_path / "out.yuv").read_bytes()
    assert len(got) == 2 * 32 * 24 * 3 and got == want.astype("<u2").tobytes()


# 7 ---- the C ABI refuses before any launch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", (False, True))
def test_c_abi_refuses_before_any_launch(scaled):
    import real_esrgan_pytorch_amd as R
    L = R._lib
    lib = L.lib()
    m, _ = _model(2, 2, "prelu", "fast")
    src = torch.zeros(4096, dtype=torch.uint8).cuda()
    dst = torch.from_numpy(np.full(4096, 0x5a5a, np.uint16)).cuda()
    a, b = R.frames.yuv_desc("nv12", "bt601"), R.frames.yuv10_desc("p010", "bt709")
    st = L.stream_ptr(src)
    with torch.no_grad():
        m.forward_yuv420_mixed(torch.zeros(1, 12, 8, dtype=torch.uint8).cuda(), ("nv12", "bt601"), ("p010", "bt709"))     # packs, builds a workspace
    desc = m._desc(1, 8, 8)
    ws = m._workspace(desc, src.device)
    plan = _plan(8, 8, 2, 1)                                                   # 16 x 16 -> 8 x 8
    tabs = list(plan.args())                                                   # oh, ow, idx_y, w_y, taps_y, idx_x, w_x, taps_x
    fwd = lib.resr_compact_forward_yuv420_mixed_scaled if scaled else lib.resr_compact_forward_yuv420_mixed
    base = [L.ptr(src), L.ptr(m._flat), L.ptr(m._packed), L.ptr(ws), ws.numel(), L.ptr(dst)]

    def call(d=desc, ends=None, t=None, qa=a, qb=b):
        e = list(ends or base)
        ref = [C.byref(q) if q is not None else None for q in (qa, qb)]
        return fwd(C.byref(d) if d is not None else None, e[0], ref[0], *e[1:], *((t or tabs) if scaled else ()), ref[1], st)

    def calls():
        for hole in (0, 1, 2, 3, 5):                                           # a null pointer
            e = list(base)
            e[hole] = None
            assert call(ends=e) == ERR_ARG
        assert call(qa=None) == ERR_ARG and call(qb=None) == ERR_ARG and call(d=None) == ERR_ARG
        for layout in (4, -1):                                                 # an unknown layout on either side
            assert call(qa=L.YuvDesc(layout, a.fq, a.iq)) == ERR_ARG and b"layout" in lib.resr_last_error()
            assert call(qb=L.YuvDesc(layout, b.fq, b.iq)) == ERR_ARG and b"layout" in lib.resr_last_error()
        for h, w in ((7, 8), (8, 7)):                                          # odd sizes
            assert call(d=m._desc(1, h, w)) == ERR_ARG and b"even" in lib.resr_last_error()
        e = list(base)                                                         # the destination's alignment rule: 16-byte stores of 10-bit
        e[5] = C.c_void_p(dst.data_ptr() + 2)                                  # words at a width of 16; dword rows on the scaled tail
        assert call(ends=e) == ERR_ARG and b"aligned" in lib.resr_last_error()
        if not scaled:
            e[5] = C.c_void_p(dst.data_ptr() + 8)
            assert call(ends=e) == ERR_ARG and b"aligned" in lib.resr_last_error()
            return
        for i, v in ((0, 7), (1, 9)):                                          # what the existing scaled entries refuse: an odd oh, ow
            t = list(tabs)
            t[i] = v
            assert call(t=t) == ERR_ARG and b"even" in lib.resr_last_error()
        for hole in (2, 3, 5, 6):                                              # a null table
            t = list(tabs)
            t[hole] = None
            assert call(t=t) == ERR_ARG
        for i, v in ((4, 0), (7, 0), (4, 4097), (7, -1)):                      # bad taps
            t = list(tabs)
            t[i] = v
            assert call(t=t) == ERR_ARG
    assert _launches(calls)[0] == 0
    torch.cuda.synchronize()
    assert bool((dst.view(torch.int16) == 0x5a5a).all())                       # the output buffer is untouched
    assert _launches(lambda: L.check(call(), "mixed"))[0] > 0                  # (the good call does launch, and the counter counts it)
    torch.cuda.synchronize()
    assert not bool((dst.view(torch.int16)[:64] == 0x5a5a).all())
