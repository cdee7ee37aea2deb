"""GPU: outscale on the frame path (csrc/image_resize.hip, frames.py, imgproc.image_resize_native).

Correctness rests on the first two tests: the float kernel and its uint8 output against the reference's own `image_resize`
(tests/golden/image_resize_native.npz, written by tests/golden/gen_resize_golden.py), and on tests/test_gpu_resize_kernel.py, which
holds the kernel to its definition bit for bit at every tile size.  Everything after them is an equality between two paths of this tree: fused tail against generic kernel, tiler against whole frame, FrameStream against single calls."""
import math
import os
import types

import numpy as np
import pytest
import torch

from tests.frames_cases import PRECISIONS, _model, random_frames

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 1e-6                      # the project's gate for this function (tests/test_dataset_golden.py)
DELTA = 255e-6                   # ... scaled to the uint8 step
MAX_EXCLUDED = 0.005
OUTSCALES = (1.5, 2, 3, 2.5)
# outscale of a x4 model -> the tile resize_plan chooses for a 96 x 96 HR frame: the small entries of choose_tile's list, which the
# outscales above (r >= 0.375: 32 x 32, 16 x 32, 16 x 16) never reach
SMALL_TILE_OUTSCALES = ((1.2, (8, 16)), (0.8, (8, 8)), (0.6, (4, 8)), (0.5, (4, 4)), (0.4, (2, 4)), (0.32, (2, 2)), (0.28, (1, 2)),
                        (0.25, (1, 1)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "image_resize_native.npz"))


def _cases(golden):
    for i, (h, w, r) in enumerate(golden["cases"]):
        yield int(h), int(w), float(r), golden[f"in_{i}"], golden[f"out_{i}"]


def test_float_kernel_against_the_reference(golden):
    from real_esrgan_pytorch_amd import imgproc
    n = 0
    for h, w, r, x, ref in _cases(golden):
        got = imgproc.image_resize_native(torch.from_numpy(x)[None].cuda(), r)
        torch.cuda.synchronize()
        assert got.dtype == torch.float32 and tuple(got.shape) == (1,) + ref.shape
        err = float(np.abs(got[0].cpu().numpy() - ref).max())
        print(f"float {h}x{w} x {r}: max |kernel - reference| = {err:.3e}")
        assert err <= ATOL, (h, w, r, err)
        n += 1
    assert n >= 9
    # a batch, and more channels than one workgroup's three: every plane is resized on its own
    x = torch.from_numpy(np.stack([golden["in_3"], golden["in_3"][::-1].copy()])).cuda()          # [2,3,60,76]
    x7 = torch.cat([x, x[:, :1] * 0.5, x.flip(1)], 1)                                              # [2,7,60,76]
    got = imgproc.image_resize_native(x7, 0.625)
    one = imgproc.image_resize_native(x[:1], 0.625)
    assert tuple(got.shape) == (2, 7, 38, 48)
    assert torch.equal(got[0, :3], one[0]) and torch.equal(got[1, :3], one[0].flip(0)) and torch.equal(got[:, 4:], got[:, :3].flip(1))
    assert np.abs(got[0, :3].cpu().numpy() - golden["out_3"]).max() <= ATOL


def test_uint8_output_against_the_reference(golden):
    from real_esrgan_pytorch_amd import imgproc
    for h, w, r, x, ref in _cases(golden):
        v = 255.0 * ref.astype(np.float64)
        near = np.abs(v - np.rint(v)) <= DELTA
        share = float(near.mean())
        assert share <= MAX_EXCLUDED, (h, w, r, share)          # a condition on the fixture, before anything is compared
        want = np.trunc(np.clip(v, 0, 255)).astype(np.int64).transpose(1, 2, 0)
        got = imgproc.image_resize_native(torch.from_numpy(x)[None].cuda(), r, u8=True)
        torch.cuda.synchronize()
        assert got.dtype == torch.uint8 and tuple(got.shape) == (1,) + want.shape
        diff = np.abs(got[0].cpu().numpy().astype(np.int64) - want)
        far = ~near.transpose(1, 2, 0)
        print(f"u8 {h}x{w} x {r}: share within delta of an integer {share:.2e}, bytes off there {int((diff[~far] != 0).sum())}")
        assert (diff[far] == 0).all(), (h, w, r, int((diff[far] != 0).sum()))
        assert diff.max() <= 1
        # and it is the float output quantised as tensor_to_image quantises
        f = imgproc.image_resize_native(torch.from_numpy(x)[None].cuda(), r)
        assert np.array_equal(got[0].cpu().numpy(), imgproc.tensor_to_image(f, False, False))


def _admits(h, w, s, o):
    from real_esrgan_pytorch_amd import imgproc
    try:
        for n in (h * s, w * s):
            imgproc.resize_band_tables(n, math.ceil(n * (o / s)), o / s)
        return True
    except ValueError:
        return False


def _generic(m, u8, o):
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import imgproc
    with torch.no_grad():
        sr = m(R.from_u8(torch.from_numpy(u8).cuda()))
        return imgproc.image_resize_native(sr, o / m.upscale, u8=True)


def _planned_tile(h, w, s, o):
    """The tile of the fused uint8 tail for LR frames h x w: resr_debug_resize_plan on the HR frame, host only."""
    import real_esrgan_pytorch_amd as R
    from tests import resize_ref
    (hh, ww), r = (h * s, w * s), o / s
    oh, ow = R.output_size(h, w, s, o)
    ty, tx = resize_ref.band(hh, r)[0].shape[1], resize_ref.band(ww, r)[0].shape[1]
    plan = resize_ref.plan_of(R._lib.lib(), 1, 3, hh, ww, oh, ow, ty, tx, resize_ref.U8)
    return (plan.th, plan.tw), (-(-oh // plan.th), -(-ow // plan.tw))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("s", [2, 3, 4])
def test_fused_equals_generic_bit_for_bit(s, precision):
    import real_esrgan_pytorch_amd as R
    m, _ = _model(2, s, "prelu", precision, "slopes")
    ran = refused = 0
    for o in OUTSCALES:
        if o == s:
            continue
        smallest = next(h for h in range(1, 64) if _admits(h, h, s, o))
        for n in (1, 3):
            for h, w in ((37, 53), (3, 5), (smallest, smallest), (smallest, 41), (64, 96)):
                if not _admits(h, w, s, o):
                    continue
                u8 = random_frames(n, h, w, seed=h * w + n)
                with torch.no_grad():
                    got = m.forward_u8(torch.from_numpy(u8).cuda(), outscale=o)
                torch.cuda.synchronize()
                assert got.dtype == torch.uint8 and got.is_contiguous()
                assert tuple(got.shape) == (n,) + R.output_size(h, w, s, o) + (3,), (o, n, h, w)
                want = _generic(m, u8, o)
                bad = int((got != want).sum())
                assert bad == 0, f"s={s} o={o} n={n} {h}x{w}: {bad} of {want.numel()} bytes differ"
                ran += 1
        for h in range(1, smallest):          # frames the rule refuses: ValueError, as the reference raises
            with pytest.raises(ValueError, match="symmetric copy"), torch.no_grad():
                m.forward_u8(torch.zeros(1, h, 9, 3, dtype=torch.uint8).cuda(), outscale=o)
            refused += 1
    assert ran >= 20
    if s == 4:                                # the small tiles: tile origins off the 4-byte grid, rows shorter than a dword
        small = 0
        for o, tile in SMALL_TILE_OUTSCALES:
            for n, h, w in ((1, 24, 24), (2, 25, 33)):
                assert _admits(h, w, s, o)
                planned, (ty, tx) = _planned_tile(h, w, s, o)
                assert planned == tile and ty >= 2 and tx >= 2, (o, h, w, planned, ty, tx)
                u8 = random_frames(n, h, w, seed=h * w + n)
                with torch.no_grad():
                    got = m.forward_u8(torch.from_numpy(u8).cuda(), outscale=o)
                torch.cuda.synchronize()
                assert got.dtype == torch.uint8 and got.is_contiguous()
                assert tuple(got.shape) == (n,) + R.output_size(h, w, s, o) + (3,), (o, n, h, w)
                want = _generic(m, u8, o)
                bad = int((got != want).sum())
                assert bad == 0, f"s={s} o={o} n={n} {h}x{w} tile {tile}: {bad} of {want.numel()} bytes differ"
                assert len(torch.unique(got)) > 16
                small += 1
        assert small == 2 * len(SMALL_TILE_OUTSCALES)
        assert _admits(1, 1, 4, 2)            # 1 x 1 at s = 4, o = 2 is among the frames above (reflection inside a tile)
    with torch.no_grad():                     # outscale None / == s is the parent's call, bit for bit
        f = torch.from_numpy(random_frames(2, 9, 11, seed=4)).cuda()
        base = m.forward_u8(f)
        assert torch.equal(m.forward_u8(f, outscale=None), base) and torch.equal(m.forward_u8(f, outscale=s), base)
        assert torch.equal(m.forward_u8(f, outscale=float(s)), base) and torch.equal(R.upscale_u8(m, f, outscale=s), base)


def test_refused_frame_exists_somewhere():
    from real_esrgan_pytorch_amd import imgproc
    assert not _admits(1, 8, 2, 1) and _admits(4, 4, 2, 1)       # the issue's (2, 8, 0.5)
    with pytest.raises(ValueError, match="symmetric copy"):
        imgproc.image_resize_native(torch.zeros(1, 3, 3, 3).cuda(), 0.5)
    with pytest.raises(ValueError, match="symmetric copy"):
        imgproc.image_resize_native(torch.zeros(1, 3, 4, 12).cuda(), 0.375)


def test_every_route_agrees(monkeypatch):
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import imgproc, tiling
    # the fused entry, and the tiler over the same model
    num_conv = 4
    for precision in ("fast", "exact16"):
        m, _ = _model(num_conv, 4, "prelu", precision, "slopes")
        u8 = random_frames(1, 70, 90, seed=3)
        frames = torch.from_numpy(u8).cuda()
        whole = R.upscale_u8(m, frames, outscale=2)
        assert tuple(whole.shape) == (1, 140, 180, 3)
        with torch.no_grad():
            assert torch.equal(whole, m.forward_u8(frames, outscale=2))
        assert torch.equal(whole, _generic(m, u8, 2))
        with monkeypatch.context() as mp:
            mp.setattr(tiling, "_MAX_OUT_PIXELS", 48 * 90)
            assert not tiling.fits_whole(m, 1, 70, 90)
            tiles, wh, ww = tiling.TiledGenerator(m, tile=None, halo=num_conv + 4, use_graph=False).plan(1, 70, 90)
            assert len(tiles) > 1 and (wh, ww) != (70, 90)
            tiled = R.upscale_u8(m, frames, halo=num_conv + 4, outscale=2)
        assert torch.equal(tiled, whole)
        for o in (1.5, 3, 2.5):
            assert torch.equal(R.upscale_u8(m, frames, outscale=o), _generic(m, u8, o)), o
    # the RRDB Generator has no fused entry: super_resolve, then the generic kernel
    torch.manual_seed(0)
    g = R.Generator(3, 3, 4, precision="exact16", n_blocks=1)
    with torch.no_grad():
        g.conv4.bias += 0.5
    g = g.cuda().eval()
    u8 = random_frames(2, 20, 24, seed=7)
    frames = torch.from_numpy(u8).cuda()
    got = R.upscale_u8(g, frames, outscale=2)
    with torch.no_grad():
        sr = g(R.from_u8(frames))
    assert tuple(got.shape) == (2, 40, 48, 3)
    assert torch.equal(got, imgproc.image_resize_native(sr, 0.5, u8=True))
    assert np.array_equal(got[1].cpu().numpy(), imgproc.tensor_to_image(imgproc.image_resize_native(sr[1:], 0.5), False, False))
    assert len(np.unique(got.cpu().numpy())) > 16
    assert torch.equal(R.upscale_u8(g, frames, outscale=4), R.upscale_u8(g, frames))


def _one_at_a_time(model, frames, outscale):
    import real_esrgan_pytorch_amd as R
    return [R.upscale_u8(model, torch.from_numpy(f)[None].cuda(), outscale=outscale)[0].cpu().numpy() for f in frames]


def test_frame_stream_outscale():
    import real_esrgan_pytorch_amd as R
    m, _ = _model(2, 4, "prelu", "fast", "slopes")
    rs = np.random.RandomState(2)
    frames = [rs.randint(0, 256, size=(12, 16, 3), dtype=np.uint8) for _ in range(5)]
    mixed = frames[:3] + [rs.randint(0, 256, size=(9, 11, 3), dtype=np.uint8) for _ in range(2)] + frames[3:]
    want = _one_at_a_time(m, mixed, 2)
    assert [w.shape for w in want] == [(24, 32, 3)] * 3 + [(18, 22, 3)] * 2 + [(24, 32, 3)] * 2
    assert all(not np.array_equal(want[0], w) for w in want[1:3])
    depth = 2
    with R.FrameStream(m, depth, outscale=2) as fs:
        got = list(fs.map(mixed))
        assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
        plan = fs._plan
        assert plan is not None and (plan.in_h, plan.in_w) == (48, 64)        # the tables of the last frame size, kept with the slots
        list(fs.map(frames[:2]))
        assert fs._plan is plan                                                # same size: not rebuilt
        list(fs.map(mixed[3:4]))
        assert fs._plan is not plan and (fs._plan.in_h, fs._plan.in_w) == (36, 44)      # dropped on a change of size
        # copy=False: a view of the slot's pinned buffer, valid for depth - 1 further submits
        fs.submit(frames[0])
        view = fs.result(copy=False)
        assert np.array_equal(view, want[0])
        for k in range(depth - 1):
            fs.submit(frames[1 + k])
        assert np.array_equal(view, want[0])
        while len(fs):
            fs.result()
        for i, v in enumerate(fs.map(frames, copy=False)):
            assert np.array_equal(v, _one_at_a_time(m, [frames[i]], 2)[0]), i
    # outscale None and outscale == s: what the parent commit's call returns
    base = _one_at_a_time(m, mixed, None)
    with torch.no_grad():
        assert all(np.array_equal(b, m.forward_u8(torch.from_numpy(f)[None].cuda())[0].cpu().numpy()) for b, f in zip(base, mixed))
    for o in (None, 4, 4.0):
        with R.FrameStream(m, 2, outscale=o) as fs:
            assert fs.outscale is None
            got = list(fs.map(mixed))
            assert fs._plan is None
        assert all(np.array_equal(g, b) for g, b in zip(got, base)), o
    with R.FrameStream(m, 2) as fs:
        assert all(np.array_equal(g, b) for g, b in zip(fs.map(mixed), base))


def test_no_full_size_frame():
    import ctypes as C
    import real_esrgan_pytorch_amd as R
    m, _ = _model(2, 4, "prelu", "fast")
    h, w = 192, 256
    frames = torch.from_numpy(random_frames(1, h, w, seed=9)).cuda()
    desc = m._desc(1, h, w)
    planned = R._lib.lib().resr_compact_workspace_bytes(C.byref(desc))
    with torch.no_grad():
        m.forward_u8(frames)
        m.forward_u8(frames, outscale=2)                 # warm: workspace, packed weights, tables
        torch.cuda.synchronize()
        assert len(m._workspaces) == 1 and next(iter(m._workspaces.values())).numel() == planned     # one workspace, not grown
        peaks = {}
        for o in (None, 2):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            y = m.forward_u8(frames, outscale=o)
            torch.cuda.synchronize()
            peaks[o] = torch.cuda.max_memory_allocated() - before
            del y
    full_fp32 = 3 * h * 4 * w * 4 * 4
    print(f"peak allocation above the resident set: x4 u8 call {peaks[None]} B, outscale-2 call {peaks[2]} B, fp32 HR frame {full_fp32} B")
    assert peaks[2] < peaks[None]
    assert peaks[2] < full_fp32                          # no tensor of N*3*H*s*W*s elements was allocated


def _write_pngs(d, sizes):
    from PIL import Image
    d.mkdir()
    rs = np.random.RandomState(5)
    names = []
    for i, (h, w) in enumerate(sizes):
        name = f"f{i:02d}.png"
        Image.fromarray(rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8)).save(d / name)
        names.append(name)
    return names


def test_directory_cli_outscale(tmp_path):
    import subprocess
    import sys
    from PIL import Image
    import real_esrgan_pytorch_amd as R
    m, sd = _model(8, 4, "prelu", "strict", "slopes")
    torch.save({"params": sd}, tmp_path / "w.pth")
    sizes = [(24, 30), (17, 21)]
    names = _write_pngs(tmp_path / "lr", sizes)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "real_esrgan_pytorch_amd.inference_frames", "--inputs_dir", str(tmp_path / "lr"), "--output_dir",
           str(tmp_path / "sr"), "--weights_path", str(tmp_path / "w.pth"), "--model_type", "compact", "--num_conv", "8", "--precision",
           "strict", "--outscale", "2"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for name, (h, w) in zip(names, sizes):
        a = np.asarray(Image.open(tmp_path / "sr" / name))
        assert a.shape == R.output_size(h, w, 4, 2) + (3,) == (2 * h, 2 * w, 3)
        lr = np.asarray(Image.open(tmp_path / "lr" / name).convert("RGB"))
        want = R.upscale_u8(m, torch.from_numpy(lr.copy())[None].cuda(), outscale=2)[0].cpu().numpy()
        assert np.array_equal(a, want), name
    assert sorted(p.name for p in (tmp_path / "sr").iterdir()) == names
