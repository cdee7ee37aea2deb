"""GPU: the 10-bit YUV 4:2:0 frame path (csrc/frames.hip, frames.py, compact.py, inference_rawvideo.py).  The path is defined as a
composition -- the numpy conversions of frames.py (tests/test_yuv420p10_surface.py pins those) around the float path, with
x = rgb10 / 1023.0f on the way in and q10(v) = trunc(clamp(v * 1023.0f, 0, 1023)) on the way out: every comparison here is an equality,
never a tolerance."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests.frames_cases import PRECISIONS, _model

pytestmark = pytest.mark.gpu

LAYOUTS = ("i420p10", "p010")
MATRICES = ("bt601", "bt709")
ERR_ARG = -1


def random_yuv10(n, h, w, seed):
    """uint16 [n,3h/2,w], uniformly random over all 65536 words (the ignored bits set, samples far outside the studio range: the clamp
    of the way in works on both sides), the words 0 and 65535 present."""
    f = np.random.RandomState(seed).randint(0, 65536, size=(n, h * 3 // 2, w)).astype(np.uint16)
    flat = f.reshape(-1)
    flat[0], flat[-1] = 0, 65535
    return f


def dev(a):
    return torch.from_numpy(a).cuda()


def unit10(f, layout, matrix):
    """The model's input by the definition: yuv420p10_to_rgb_np(f) / 1023.0f as fp32 NCHW (one IEEE division per sample)."""
    import real_esrgan_pytorch_amd as R
    rgb = R.yuv420p10_to_rgb_np(f, layout, matrix)
    return np.ascontiguousarray((rgb.astype(np.float32) / np.float32(1023.0)).transpose(0, 3, 1, 2))


def q10(v):
    """fp32 NCHW -> uint16 [n,h,w,3]: v * 1023.0f in fp32, clamp to [0, 1023], truncate."""
    assert v.dtype == np.float32
    return np.clip(v * np.float32(1023.0), np.float32(0), np.float32(1023.0)).astype(np.uint16).transpose(0, 2, 3, 1)


def composition(float_path, f, layout, matrix):
    import real_esrgan_pytorch_amd as R
    with torch.no_grad():
        sr = float_path(dev(unit10(f, layout, matrix)))
    return R.rgb_to_yuv420p10_np(q10(sr.cpu().numpy()), layout, matrix)


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == np.uint16 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {want.size} words differ, first at {np.argwhere(got != want)[:4].tolist()}"


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
@pytest.mark.parametrize("n,h,w", [(1, 2, 2), (3, 2, 6), (2, 4, 10), (1, 6, 8), (2, 8, 16), (1, 4, 24), (1, 2, 12)])
def test_generic_conversions_are_the_numpy_definition(n, h, w, layout, matrix):
    import real_esrgan_pytorch_amd as R
    f = random_yuv10(n, h, w, seed=h * w + n)
    x = R.from_yuv420p10(dev(f), layout, matrix)
    assert x.is_contiguous() and x.dtype == torch.float32 and tuple(x.shape) == (n, 3, h, w)
    want = unit10(f, layout, matrix)
    assert np.array_equal(x.cpu().numpy(), want), "from_yuv420p10"
    assert (want == 0).any() and (want == 1).any()                      # the clamp is exercised on both sides
    # the way out: floats on and between levels, below 0 and above 1
    v = np.random.RandomState(w).uniform(-0.25, 1.25, size=(n, 3, h, w)).astype(np.float32)
    v.reshape(-1)[:4] = (-0.5, 1.5, 0.0, 1.0)
    levels = q10(v)
    assert (v < 0).any() and (v > 1).any() and levels.min() == 0 and levels.max() == 1023
    yuv = R.to_yuv420p10(dev(v), layout, matrix)
    assert yuv.is_contiguous() and yuv.dtype == torch.uint16 and tuple(yuv.shape) == (n, h * 3 // 2, w)
    _same(yuv, R.rgb_to_yuv420p10_np(levels, layout, matrix), "to_yuv420p10")
    # ... and chained on the device as on the host
    _same(R.to_yuv420p10(x, layout, matrix), R.rgb_to_yuv420p10_np(q10(want), layout, matrix), "to_yuv420p10(from_yuv420p10)")


# 2 ---- the fused entry is the composition --------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,h,w,s", [(2, 4, 6, 4), (1, 6, 10, 3), (3, 2, 2, 1), (1, 4, 4, 2), (2, 2, 6, 2)],
                         ids=["wide24", "narrow30", "edge2", "wide8", "narrow12"])
def test_forward_yuv420p10_is_the_composition(n, h, w, s, layout, precision):
    import real_esrgan_pytorch_amd as R
    m, _ = _model(2, s, "prelu", precision, "slopes")
    for matrix in MATRICES:
        f = random_yuv10(n, h, w, seed=h * w + n + s)
        with torch.no_grad():
            got = m.forward_yuv420p10(dev(f), layout, matrix)
        torch.cuda.synchronize()
        assert got.is_contiguous() and got.dtype == torch.uint16 and tuple(got.shape) == (n, h * s * 3 // 2, w * s)
        _same(got, composition(m, f, layout, matrix), f"forward_yuv420p10 {matrix}")
        assert torch.equal(R.upscale_yuv420p10(m, dev(f), layout, matrix).view(torch.int16), got.view(torch.int16))     # fits: the fused entry


def test_forward_yuv420p10_runs_its_own_kernels():
    m, _ = _model(2, 4, "prelu", "fast", "slopes")
    f = dev(random_yuv10(1, 4, 6, seed=1))
    with torch.no_grad():
        n, ids = _launches(lambda: m.forward_yuv420p10(f, "p010"))
    # the 10-bit head and the x4 10-bit tail; none of the 8-bit ends (RGB / YUV head, u8 / YUV tail), none of the generic conversions
    assert n == len(ids) and 31022 in ids and ids[-1] == 31064, ids
    assert not {31020, 31021, 31014, 31044, 31030, 31031, 31032, 31033, 31034, 31035} & set(ids), ids


# 3 ---- every case whose ends are not fused -------------------------------------------------------------------------------------
def test_upscale_yuv420p10_rrdb_generator():
    import real_esrgan_pytorch_amd as R
    torch.manual_seed(0)
    g = R.Generator(3, 3, 4, precision="exact16", n_blocks=1)
    with torch.no_grad():
        g.conv4.bias += 0.5
    g = g.cuda().eval()
    assert not hasattr(g, "forward_yuv420p10")
    f = random_yuv10(2, 20, 24, seed=7)
    for layout in LAYOUTS:
        n, ids = _launches(lambda: R.upscale_yuv420p10(g, dev(f), layout, "bt709"))
        assert ids[0] == 31034 and ids[-1] == 31035, ids                 # the generic conversions are its ends
        got = R.upscale_yuv420p10(g, dev(f), layout, "bt709")
        assert tuple(got.shape) == (2, 120, 96)
        _same(got, composition(g, f, layout, "bt709"), layout)


def test_upscale_yuv420p10_tiled(monkeypatch):
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import tiling
    m, _ = _model(2, 2, "prelu", "fast", "slopes")
    f = random_yuv10(1, 40, 48, seed=5)
    whole = R.upscale_yuv420p10(m, dev(f), "i420p10")
    monkeypatch.setattr(tiling, "_MAX_OUT_PIXELS", 28 * 48)                  # the frame no longer fits one call: the tiler cuts it
    assert not tiling.fits_whole(m, 1, 40, 48)
    halo = m.receptive_radius + 2
    tiles, wh, ww = tiling.TiledGenerator(m, tile=None, halo=halo, use_graph=False).plan(1, 40, 48)
    assert len(tiles) > 1 and (wh, ww) != (40, 48)
    for layout in LAYOUTS:
        n, ids = _launches(lambda: R.upscale_yuv420p10(m, dev(f), layout, halo=halo))
        assert ids[0] == 31034 and ids[-1] == 31035 and 31022 not in ids, ids
        got = R.upscale_yuv420p10(m, dev(f), layout, halo=halo)
        _same(got, composition(lambda x: tiling.super_resolve(m, x, halo), f, layout, "bt601"), layout)
    # with the halo of the receptive field the tiled float frame is the whole one, hence the same words
    _same(R.upscale_yuv420p10(m, dev(f), "i420p10", halo=halo), whole.cpu().numpy(), "tiled == whole")


def test_upscale_yuv420p10_outscale():
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import imgproc
    m, _ = _model(2, 4, "prelu", "fast", "slopes")
    f = random_yuv10(2, 12, 18, seed=3)
    plan = imgproc.ResizePlan(48, 72, 0.5, torch.device("cuda", torch.cuda.current_device()))
    for layout in LAYOUTS:
        got = R.upscale_yuv420p10(m, dev(f), layout, outscale=2)
        assert tuple(got.shape) == (2, 36, 36)
        _same(got, composition(lambda x: imgproc.resize_with_plan(m(x), plan), f, layout, "bt601"), layout)
    same = R.upscale_yuv420p10(m, dev(f), outscale=4)                         # the model's own factor: the fused path
    assert torch.equal(same.view(torch.int16), R.upscale_yuv420p10(m, dev(f)).view(torch.int16))
    # 12x18 x 2.5 = 30x45: an odd width cannot be a 4:2:0 frame -- refused before anything is launched
    assert R.output_size(12, 18, 4, 2.5) == (30, 45)
    d = dev(f)

    def odd():
        with pytest.raises(ValueError, match="even"):
            R.upscale_yuv420p10(m, d, outscale=2.5)
    assert _launches(odd)[0] == 0
    assert _launches(lambda: R.upscale_yuv420p10(m, d, outscale=2))[0] > 0     # (the counter does count this path's launches)


# 4 ---- FrameStream ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pix_fmt", LAYOUTS)
def test_frame_stream_yuv420p10(pix_fmt):
    import real_esrgan_pytorch_amd as R
    m, _ = _model(2, 2, "prelu", "fast", "slopes")
    sizes = [(12, 16), (6, 10)]
    frames = [random_yuv10(1, *sizes[i % 2], seed=i)[0] for i in range(5)]         # two alternating sizes: every submit reallocates

    want = [R.upscale_yuv420p10(m, dev(f)[None], pix_fmt, "bt709")[0].cpu().numpy() for f in frames]
    with R.FrameStream(m, depth=2, pix_fmt=pix_fmt, matrix="bt709") as fs:
        got = list(fs.map(frames))
        assert [g.shape for g in got] == [(36, 32), (18, 20)] * 2 + [(36, 32)] and all(g.dtype == np.uint16 for g in got)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        views = [v.copy() for v in fs.map(frames, copy=False)]                   # (a view is valid until its slot is submitted to again)
        assert all(np.array_equal(g, w) for g, w in zip(views, want))
        # one size, so that the slots are reused: copy=False hands out the slot's pinned buffer
        steady = [frames[0], frames[2], frames[4], frames[0]]
        out = [v.copy() for v in fs.map(steady, copy=False)]
        assert all(np.array_equal(g, want[i]) for g, i in zip(out, (0, 2, 4, 0)))
        fs.submit(frames[0])
        view = fs.result(copy=False)
        fs.submit(frames[2])
        assert np.array_equal(fs.result(), want[2]) and np.array_equal(view, want[0])
        fs.submit(frames[4])
        again = fs.result(copy=False)
        assert np.shares_memory(again, view) and np.array_equal(view, want[4])
        # the frame checks: an 8-bit frame, rows not a multiple of 3, an odd width
        for bad in (np.zeros((18, 16), np.uint8), np.zeros((16, 16), np.uint16), np.zeros((18, 15), np.uint16)):
            with pytest.raises(ValueError, match="uint16"):
                fs.submit(bad)
    with R.FrameStream(m, depth=2, pix_fmt=pix_fmt, outscale=3) as fs:          # 12x16 x 3 = 36x48
        got = list(fs.map(frames[:1]))
        assert np.array_equal(got[0], R.upscale_yuv420p10(m, dev(frames[0])[None], pix_fmt, outscale=3)[0].cpu().numpy())


# 5 ---- argument checks ----------------------------------------------------------------------------------------------------------
def test_c_abi_refuses_before_any_launch():
    import real_esrgan_pytorch_amd as R
    L = R._lib
    lib = L.lib()
    m, _ = _model(2, 2, "prelu", "fast")
    src = torch.zeros(4096, dtype=torch.uint16).cuda()
    dst = torch.zeros(4096, dtype=torch.uint16).cuda()
    flt = torch.zeros(4096, dtype=torch.float32).cuda()
    ok = R.frames.yuv10_desc("i420p10", "bt601")
    eight = R.frames.yuv_desc("i420", "bt601")
    bad_layout = L.YuvDesc(7, ok.fq, ok.iq)
    st = L.stream_ptr(src)
    with torch.no_grad():
        m.forward_yuv420p10(torch.zeros(1, 12, 8, dtype=torch.uint16).cuda())      # builds the packed weights and a workspace
    desc = m._desc(1, 8, 8)
    ws = m._workspace(desc, src.device)

    def calls():
        for fn, a, b in ((lib.resr_yuv420p10_to_nchw, src, flt), (lib.resr_nchw_to_yuv420p10, flt, dst)):
            assert fn(L.ptr(a), L.ptr(b), 1, 7, 8, C.byref(ok), st) == ERR_ARG              # odd h
            assert fn(L.ptr(a), L.ptr(b), 1, 8, 7, C.byref(ok), st) == ERR_ARG              # odd w
            assert fn(L.ptr(a), L.ptr(b), 1, 8, 8, C.byref(bad_layout), st) == ERR_ARG
            assert fn(L.ptr(a), L.ptr(b), 1, 8, 8, C.byref(eight), st) == ERR_ARG           # an 8-bit descriptor
            assert fn(None, L.ptr(b), 1, 8, 8, C.byref(ok), st) == ERR_ARG
            assert fn(L.ptr(a), None, 1, 8, 8, C.byref(ok), st) == ERR_ARG
            assert fn(L.ptr(a), L.ptr(b), 1, 8, 8, None, st) == ERR_ARG
        assert lib.resr_nchw_to_yuv420p10(L.ptr(flt), C.c_void_p(dst.data_ptr() + 2), 1, 8, 8, C.byref(ok), st) == ERR_ARG   # 8-byte stores
        fwd = lib.resr_compact_forward_yuv420p10
        args = [L.ptr(src), L.ptr(m._flat), L.ptr(m._packed), L.ptr(ws), ws.numel(), L.ptr(dst)]
        for h, w in ((7, 8), (8, 7)):
            assert fwd(C.byref(m._desc(1, h, w)), *args, C.byref(ok), st) == ERR_ARG
        assert fwd(C.byref(desc), *args, C.byref(bad_layout), st) == ERR_ARG
        assert fwd(C.byref(desc), *args, C.byref(eight), st) == ERR_ARG
        assert fwd(C.byref(desc), *args, None, st) == ERR_ARG
        assert fwd(None, *args, C.byref(ok), st) == ERR_ARG                                 # a null descriptor
        for hole in (0, 1, 2, 3, 5):
            a = list(args)
            a[hole] = None
            assert fwd(C.byref(desc), *a, C.byref(ok), st) == ERR_ARG
        # width 16, the wide stores of 16 bytes: a destination offset by one sample
        assert fwd(C.byref(desc), *args[:5], C.c_void_p(dst.data_ptr() + 2), C.byref(ok), st) == ERR_ARG
        assert b"aligned" in lib.resr_last_error()
        assert lib.resr_compact_forward_yuv420(C.byref(desc), *args, C.byref(ok), st) == ERR_ARG    # the 8-bit entry, a 10-bit descriptor
    assert _launches(calls)[0] == 0


def test_python_argument_checks():
    import real_esrgan_pytorch_amd as R
    m, _ = _model(2, 2, "prelu", "fast")
    good = torch.zeros(1, 12, 8, dtype=torch.uint16).cuda()
    with pytest.raises(RuntimeError, match="backward"):                  # the guard of forward: grad mode on, parameters that require grad
        m.forward_yuv420p10(good)
    assert tuple(R.upscale_yuv420p10(m, good).shape) == (1, 24, 16)
    with torch.no_grad():
        for call in (lambda f: m.forward_yuv420p10(f), lambda f: R.upscale_yuv420p10(m, f), lambda f: R.from_yuv420p10(f)):
            for dtype in (torch.uint8, torch.int16, torch.float32):                             # dtype
                with pytest.raises(RuntimeError, match="uint16"):
                    call(torch.zeros(1, 12, 8, dtype=dtype).cuda())
            for shape in ((1, 8, 8), (1, 12, 7), (12, 8), (1, 8, 8, 3)):                        # rows % 3, odd W, no batch, RGB
                with pytest.raises(RuntimeError, match="3H/2"):
                    call(torch.zeros(*shape, dtype=torch.uint16).cuda())
            with pytest.raises(RuntimeError, match="contiguous"):
                call(torch.zeros(1, 8, 12, dtype=torch.uint16).cuda().permute(0, 2, 1))
        with pytest.raises(RuntimeError, match="fp32"):
            R.to_yuv420p10(torch.zeros(1, 3, 4, 4, dtype=torch.float16).cuda())
        for shape in ((1, 3, 3, 4), (1, 3, 4, 5)):
            with pytest.raises(RuntimeError, match="even"):
                R.to_yuv420p10(torch.zeros(*shape).cuda())
        assert tuple(R.to_yuv420p10(torch.zeros(1, 3, 4, 6).cuda().permute(0, 1, 3, 2)).shape) == (1, 9, 4)    # made contiguous, as to_u8
        with pytest.raises(ValueError, match="layout"):
            R.from_yuv420p10(good, "nv12")
        with pytest.raises(ValueError, match="matrix"):
            R.to_yuv420p10(torch.zeros(1, 3, 4, 4).cuda(), "p010", "bt2020")


# 6 ---- the rawvideo CLI ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pix_fmt,layout", [("yuv420p10le", "i420p10"), ("p010le", "p010")])
def test_inference_rawvideo_writes_upscale_yuv420p10(tmp_path, capsys, pix_fmt, layout):
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import inference_rawvideo
    m, sd = _model(4, 4, "prelu", "strict", "slopes")
    torch.save({"params": sd}, tmp_path / "w.pth")
    frames = random_yuv10(3, 6, 8, seed=11)                                  # three 8x6 frames of 72 words = 144 bytes
    (tmp_path / "in.yuv").write_bytes(frames.astype("<u2").tobytes())
    args = types.SimpleNamespace(input=str(tmp_path / "in.yuv"), output=str(tmp_path / "out.yuv"), size="8x6", pix_fmt=pix_fmt,
                                 matrix="bt601", weights_path=str(tmp_path / "w.pth"), model_type="compact", num_conv=4,
                                 act_type="prelu", precision="strict", depth=2, outscale=None)
    assert inference_rawvideo.main(args) == 3
    assert f"Output size 32x24 ({pix_fmt}, {32 * 24 * 3} bytes per frame)" in capsys.readouterr().out
    want = b"".join(R.upscale_yuv420p10(m, dev(f)[None], layout)[0].cpu().numpy().astype("<u2").tobytes() for f in frames)
    got = (tmp_path / "out.yuv").read_bytes()
    assert len(got) == 3 * 32 * 24 * 3 and got == want
    # a trailing partial frame is an error that names the byte count
    (tmp_path / "cut.yuv").write_bytes(frames.astype("<u2").tobytes()[:-5])
    args.input = str(tmp_path / "cut.yuv")
    with pytest.raises(ValueError, match="frame 2: 139 trailing bytes.* has 144"):
        inference_rawvideo.main(args)
