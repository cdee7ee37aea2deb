"""GPU: the YUV 4:2:0 frame path (csrc/frames.hip, frames.py, compact.py, inference_rawvideo.py).  The path is defined as a
composition over the uint8 RGB path with two integer colour conversions, whose numpy versions in frames.py are the oracle
(tests/test_yuv420_surface.py pins those): every comparison here is an equality, never a tolerance."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests.frames_cases import PRECISIONS, _model

pytestmark = pytest.mark.gpu

LAYOUTS = ("i420", "nv12")
MATRICES = ("bt601", "bt709")
ERR_ARG = -1


def random_yuv(n, h, w, seed):
    """uint8 [n,3h/2,w], uniformly random over all 256 values (far outside the studio range: the clamp of the way in works on
    both sides), the values 0 and 255 present."""
    f = np.random.RandomState(seed).randint(0, 256, size=(n, h * 3 // 2, w), dtype=np.uint8)
    flat = f.reshape(-1)
    flat[0], flat[-1] = 0, 255
    return f


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {want.size} bytes differ, first at {np.argwhere(got != want)[:4].tolist()}"


def _launches(fn):
    """Launches the library records while `fn` runs (its in-situ profiler counts every one)."""
    import real_esrgan_pytorch_amd as R
    lib = R._lib.lib()
    lib.resr_profile_begin()
    try:
        fn()
    finally:
        torch.cuda.synchronize()
        buf = (R._lib.ProfEntry * 4096)()
        n = int(lib.resr_profile_end(C.cast(buf, C.c_void_p), 4096))
    return n, [buf[i].kernel_id for i in range(min(n, 4096))]


# 1 ---- the generic launches against the numpy definition ---------------------------------------------------------------------
@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,h,w", [(1, 2, 2), (3, 2, 6), (2, 4, 10), (1, 6, 8), (2, 8, 16), (1, 4, 24)])
def test_generic_conversions_are_the_numpy_definition(n, h, w, layout, matrix):
    import real_esrgan_pytorch_amd as R
    f = random_yuv(n, h, w, seed=h * w + n)
    rgb = R.yuv420_to_rgb(torch.from_numpy(f).cuda(), layout, matrix)
    assert rgb.is_contiguous() and tuple(rgb.shape) == (n, h, w, 3)
    want = R.yuv420_to_rgb_np(f, layout, matrix)
    _same(rgb, want, "yuv420_to_rgb")
    assert (want == 0).any() and (want == 255).any()                 # the clamp is exercised on both sides
    u8 = np.random.RandomState(w).randint(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    u8.reshape(-1)[0], u8.reshape(-1)[-1] = 0, 255
    yuv = R.rgb_to_yuv420(torch.from_numpy(u8).cuda(), layout, matrix)
    assert yuv.is_contiguous() and tuple(yuv.shape) == (n, h * 3 // 2, w)
    _same(yuv, R.rgb_to_yuv420_np(u8, layout, matrix), "rgb_to_yuv420")
    # ... and chained on the device as on the host
    _same(R.rgb_to_yuv420(rgb, layout, matrix), R.rgb_to_yuv420_np(want, layout, matrix), "rgb_to_yuv420(yuv420_to_rgb)")


# 2 ---- the fused entry is the composition --------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,h,w,s", [(2, 4, 6, 4), (1, 6, 10, 3), (3, 2, 2, 1), (1, 4, 4, 2), (2, 2, 6, 2)],
                         ids=["wide24", "narrow30", "edge2", "wide8", "narrow12"])
def test_forward_yuv420_is_the_composition(n, h, w, s, layout, precision):
    import real_esrgan_pytorch_amd as R
    m, _ = _model(2, s, "prelu", precision, "slopes")
    for matrix in MATRICES:
        f = random_yuv(n, h, w, seed=h * w + n + s)
        with torch.no_grad():
            got = m.forward_yuv420(torch.from_numpy(f).cuda(), layout, matrix)
            mid = m.forward_u8(torch.from_numpy(R.yuv420_to_rgb_np(f, layout, matrix)).cuda())
        torch.cuda.synchronize()
        assert got.is_contiguous() and tuple(got.shape) == (n, h * s * 3 // 2, w * s)
        _same(got, R.rgb_to_yuv420_np(mid.cpu().numpy(), layout, matrix), f"forward_yuv420 {matrix}")
        assert torch.equal(R.upscale_yuv420(m, torch.from_numpy(f).cuda(), layout, matrix), got)     # fits: the fused entry


def test_forward_yuv420_runs_its_own_kernels():
    m, _ = _model(2, 4, "prelu", "fast", "slopes")
    f = torch.from_numpy(random_yuv(1, 4, 6, seed=1)).cuda()
    with torch.no_grad():
        n, ids = _launches(lambda: m.forward_yuv420(f, "nv12"))
    # the YUV head and the x4 YUV tail, and neither the RGB ends nor the generic conversions
    assert n == len(ids) and 31021 in ids and ids[-1] == 31044 and not {31020, 31014, 31032, 31033} & set(ids), ids


# 3 ---- every case whose ends are not fused -------------------------------------------------------------------------------------
def test_upscale_yuv420_rrdb_generator():
    import real_esrgan_pytorch_amd as R
    torch.manual_seed(0)
    g = R.Generator(3, 3, 4, precision="exact16", n_blocks=1)
    with torch.no_grad():
        g.conv4.bias += 0.5
    g = g.cuda().eval()
    assert not hasattr(g, "forward_yuv420")
    f = random_yuv(2, 20, 24, seed=7)
    for layout in LAYOUTS:
        got = R.upscale_yuv420(g, torch.from_numpy(f).cuda(), layout, "bt709")
        mid = R.upscale_u8(g, torch.from_numpy(R.yuv420_to_rgb_np(f, layout, "bt709")).cuda())
        assert tuple(got.shape) == (2, 120, 96)
        _same(got, R.rgb_to_yuv420_np(mid.cpu().numpy(), layout, "bt709"), layout)


def test_upscale_yuv420_outscale():
    import real_esrgan_pytorch_amd as R
    m, _ = _model(2, 4, "prelu", "fast", "slopes")
    f = random_yuv(2, 12, 18, seed=3)
    dev = torch.from_numpy(f).cuda()
    for layout in LAYOUTS:
        got = R.upscale_yuv420(m, dev, layout, outscale=2)
        mid = R.upscale_u8(m, torch.from_numpy(R.yuv420_to_rgb_np(f, layout)).cuda(), outscale=2)
        assert tuple(mid.shape) == (2, 24, 36, 3) and tuple(got.shape) == (2, 36, 36)
        _same(got, R.rgb_to_yuv420_np(mid.cpu().numpy(), layout), layout)
    assert torch.equal(R.upscale_yuv420(m, dev, outscale=4), R.upscale_yuv420(m, dev))       # the model's own factor: the fused path
    # 12x18 x 2.5 = 30x45: an odd width cannot be a 4:2:0 frame -- refused before anything is launched
    assert R.output_size(12, 18, 4, 2.5) == (30, 45)
    def odd():
        with pytest.raises(ValueError, match="even"):
            R.upscale_yuv420(m, dev, outscale=2.5)
    assert _launches(odd)[0] == 0
    n, _ = _launches(lambda: R.upscale_yuv420(m, dev, outscale=2))
    assert n > 0                                                     # (the counter does count this path's launches)


# 4 ---- FrameStream ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pix_fmt", LAYOUTS)
def test_frame_stream_yuv420(pix_fmt):
    import real_esrgan_pytorch_amd as R
    m, _ = _model(2, 2, "prelu", "fast", "slopes")
    frames = [random_yuv(1, 12, 16, seed=i)[0] for i in range(5)]

    def one_at_a_time(fs_):
        return [R.upscale_yuv420(m, torch.from_numpy(f)[None].cuda(), pix_fmt, "bt709")[0].cpu().numpy() for f in fs_]
    want = one_at_a_time(frames)
    assert all(not np.array_equal(want[0], w) for w in want[1:])          # distinct contents: an order mix-up would show
    depth = 3
    with R.FrameStream(m, depth=depth, pix_fmt=pix_fmt, matrix="bt709") as fs:
        got = list(fs.map(frames))
        assert len(got) == 5 and all(g.shape == (36, 32) and g.dtype == np.uint8 for g in got)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        # a change of frame size in the middle drains and continues
        mixed = frames[:2] + [random_yuv(1, 6, 10, seed=9)[0], random_yuv(1, 6, 10, seed=10)[0]] + frames[2:4]
        got_mixed = list(fs.map(mixed))
        assert [g.shape for g in got_mixed] == [(36, 32)] * 2 + [(18, 20)] * 2 + [(36, 32)] * 2
        assert all(np.array_equal(g, w) for g, w in zip(got_mixed, one_at_a_time(mixed)))
        # copy=False: a view of the slot's pinned buffer, valid for depth - 1 further submits; the depth-th overwrites it
        fs.submit(frames[0])
        view = fs.result(copy=False)
        assert np.array_equal(view, want[0])
        for k in range(1, depth):
            fs.submit(frames[k])
            assert np.array_equal(fs.result(), want[k]) and np.array_equal(view, want[0]), k
        fs.submit(frames[depth])
        again = fs.result(copy=False)
        assert np.shares_memory(again, view) and np.array_equal(view, want[depth])
        # the frame checks: an RGB frame, rows not a multiple of 3, an odd width
        for bad in (np.zeros((12, 16, 3), np.uint8), np.zeros((16, 16), np.uint8), np.zeros((18, 15), np.uint8)):
            with pytest.raises(ValueError, match="3H/2"):
                fs.submit(bad)
    with R.FrameStream(m, depth=2, pix_fmt=pix_fmt, outscale=3) as fs:          # 12x16 x 3 = 36x48
        got = list(fs.map(frames[:3]))
        for g, f in zip(got, frames):
            assert np.array_equal(g, R.upscale_yuv420(m, torch.from_numpy(f)[None].cuda(), pix_fmt, outscale=3)[0].cpu().numpy())
    with R.FrameStream(m, depth=2, pix_fmt=pix_fmt, outscale=2.5) as fs:
        with pytest.raises(ValueError, match="even"):
            fs.submit(random_yuv(1, 6, 6, seed=0)[0])                        # 6x6 x 2.5 = 15x15
    with R.FrameStream(m, depth=2) as fs:                                       # rgb24 is what it was
        rgb = np.random.RandomState(0).randint(0, 256, size=(12, 16, 3), dtype=np.uint8)
        assert np.array_equal(next(iter(fs.map([rgb]))), R.upscale_u8(m, torch.from_numpy(rgb)[None].cuda())[0].cpu().numpy())


# 5 ---- argument checks ----------------------------------------------------------------------------------------------------------
def test_c_abi_refuses_before_any_launch():
    import real_esrgan_pytorch_amd as R
    L = R._lib
    lib = L.lib()
    m, _ = _model(2, 2, "prelu", "fast")
    src = torch.zeros(4096, dtype=torch.uint8).cuda()
    dst = torch.zeros(4096, dtype=torch.uint8).cuda()
    ok = R.frames.yuv_desc("i420", "bt601")
    bad_layout = L.YuvDesc(7, ok.fq, ok.iq)
    st = L.stream_ptr(src)
    with torch.no_grad():
        m.forward_yuv420(torch.zeros(1, 12, 8, dtype=torch.uint8).cuda())          # builds the packed weights and a workspace
    desc = m._desc(1, 8, 8)
    ws = m._workspace(desc, src.device)

    def calls():
        for fn in (lib.resr_yuv420_to_rgb, lib.resr_rgb_to_yuv420):
            assert fn(L.ptr(src), L.ptr(dst), 1, 7, 8, C.byref(ok), st) == ERR_ARG              # odd h
            assert fn(L.ptr(src), L.ptr(dst), 1, 8, 7, C.byref(ok), st) == ERR_ARG              # odd w
            assert fn(L.ptr(src), L.ptr(dst), 1, 8, 8, C.byref(bad_layout), st) == ERR_ARG
            assert fn(None, L.ptr(dst), 1, 8, 8, C.byref(ok), st) == ERR_ARG
            assert fn(L.ptr(src), None, 1, 8, 8, C.byref(ok), st) == ERR_ARG
            assert fn(L.ptr(src), L.ptr(dst), 1, 8, 8, None, st) == ERR_ARG
        fwd = lib.resr_compact_forward_yuv420
        args = [L.ptr(src), L.ptr(m._flat), L.ptr(m._packed), L.ptr(ws), ws.numel(), L.ptr(dst)]
        for h, w in ((7, 8), (8, 7)):
            assert fwd(C.byref(m._desc(1, h, w)), *args, C.byref(ok), st) == ERR_ARG
        assert fwd(C.byref(desc), *args, C.byref(bad_layout), st) == ERR_ARG
        assert fwd(C.byref(desc), *args, None, st) == ERR_ARG
        for hole in (0, 1, 2, 3, 5):
            a = list(args)
            a[hole] = None
            assert fwd(C.byref(desc), *a, C.byref(ok), st) == ERR_ARG
        assert fwd(C.byref(desc), *args[:5], C.c_void_p(dst.data_ptr() + 4), C.byref(ok), st) == ERR_ARG     # width 16: 8-byte stores
    assert _launches(calls)[0] == 0


def test_python_argument_checks():
    import real_esrgan_pytorch_amd as R
    m, _ = _model(2, 2, "prelu", "fast")
    good = torch.zeros(1, 12, 8, dtype=torch.uint8).cuda()
    with pytest.raises(RuntimeError, match="backward"):                  # the guard of forward: grad mode on, parameters that require grad
        m.forward_yuv420(good)
    assert tuple(R.upscale_yuv420(m, good).shape) == (1, 24, 16)
    with torch.no_grad():
        for call in (lambda f: m.forward_yuv420(f), lambda f: R.upscale_yuv420(m, f), lambda f: R.yuv420_to_rgb(f)):
            with pytest.raises(RuntimeError, match="uint8"):
                call(torch.zeros(1, 12, 8).cuda())                                              # dtype
            for shape in ((1, 8, 8), (1, 12, 7), (12, 8), (1, 8, 8, 3)):                        # rows % 3, odd W, no batch, RGB
                with pytest.raises(RuntimeError, match="3H/2"):
                    call(torch.zeros(*shape, dtype=torch.uint8).cuda())
            with pytest.raises(RuntimeError, match="contiguous"):
                call(torch.zeros(1, 8, 12, dtype=torch.uint8).cuda().permute(0, 2, 1))
        with pytest.raises(RuntimeError, match="uint8"):
            R.rgb_to_yuv420(torch.zeros(1, 4, 4, 3).cuda())
        for shape in ((1, 3, 4, 3), (1, 4, 5, 3)):
            with pytest.raises(RuntimeError, match="even"):
                R.rgb_to_yuv420(torch.zeros(*shape, dtype=torch.uint8).cuda())
        with pytest.raises(RuntimeError, match="contiguous"):
            R.rgb_to_yuv420(torch.zeros(1, 4, 3, 4, dtype=torch.uint8).cuda().permute(0, 1, 3, 2))
        with pytest.raises(ValueError, match="layout"):
            R.yuv420_to_rgb(good, "yv12")
        with pytest.raises(ValueError, match="matrix"):
            R.rgb_to_yuv420(torch.zeros(1, 4, 4, 3, dtype=torch.uint8).cuda(), "i420", "bt2020")


# 6 ---- the rawvideo CLI ---------------------------------------------------------------------------------------------------------
def test_inference_rawvideo_writes_upscale_yuv420(tmp_path):
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import inference_rawvideo
    m, sd = _model(4, 4, "prelu", "strict", "slopes")
    torch.save({"params": sd}, tmp_path / "w.pth")
    frames = random_yuv(3, 6, 8, seed=11)                                    # three 8x6 I420 frames of 72 bytes
    (tmp_path / "in.yuv").write_bytes(frames.tobytes())
    args = types.SimpleNamespace(input=str(tmp_path / "in.yuv"), output=str(tmp_path / "out.yuv"), size="8x6", pix_fmt="yuv420p",
                                 matrix="bt601", weights_path=str(tmp_path / "w.pth"), model_type="compact", num_conv=4,
                                 act_type="prelu", precision="strict", depth=2, outscale=None)
    assert inference_rawvideo.main(args) == 3
    want = b"".join(R.upscale_yuv420(m, torch.from_numpy(f)[None].cuda())[0].cpu().numpy().tobytes() for f in frames)
    got = (tmp_path / "out.yuv").read_bytes()
    assert len(got) == 3 * 32 * 24 * 3 // 2 and got == want
    # a trailing partial frame is an error that names the byte count
    (tmp_path / "cut.yuv").write_bytes(frames.tobytes()[:-5])
    args.input = str(tmp_path / "cut.yuv")
    with pytest.raises(ValueError, match="67 trailing bytes"):
        inference_rawvideo.main(args)
