"""CPU: the surface of outscale -- the two new C-ABI entries (exported, declared, argument checks before any launch), the banded
tap tables against `imgproc._resize_matrix` and against the reference's own outputs (tests/golden/image_resize_native.npz, written
by tests/golden/gen_resize_golden.py), `frames.output_size`, the Python argument checks, and the launch plan of the resize kernel
(`resr_debug_resize_plan`) swept over scales, lengths and output kinds: the staged region holds every tile's taps within 64 KB of LDS.
Nothing here touches a device."""
import ctypes as C
import hashlib
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("resr_image_resize", "resr_compact_forward_u8_scaled", "resr_compact_forward_u8")
ERR_ARG, ERR_WORKSPACE = -1, -3          # include/resr.h resr_status


@pytest.fixture(scope="module")
def R():
    import __graft_entry__
    __graft_entry__.build()
    import real_esrgan_pytorch_amd as R
    return R


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "image_resize_native.npz"))


def test_symbols_exported_declared_and_bound(R):
    lib = C.CDLL(R._lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "resr.h")).read()
    declared = set(re.findall(r"\b(resr_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in declared, name
        assert name in R._lib.exported_symbols(), name
    assert R._lib.lib().resr_version() == 3 and R._lib.RESR_VERSION == 3
    assert re.search(r"#define RESR_VERSION 3\b", hdr)


def test_package_exports(R):
    from real_esrgan_pytorch_amd import imgproc
    assert R.output_size is R.frames.output_size and "output_size" in R.__all__
    for name in ("image_resize_native", "resize_band_tables", "ResizePlan"):
        assert hasattr(imgproc, name) and name in imgproc.__all__, name
    import inspect
    assert "outscale" in inspect.signature(R.SRVGGNetCompact.forward_u8).parameters
    assert "outscale" in inspect.signature(R.upscale_u8).parameters
    assert "outscale" in inspect.signature(R.FrameStream.__init__).parameters
    assert inspect.signature(R.upscale_u8).parameters["outscale"].default is None


def _fake(nbytes=64):
    """A host buffer standing in for a device pointer: the calls below return before they would launch anything."""
    buf = (C.c_uint8 * nbytes)()
    return buf, C.cast(buf, C.c_void_p)


def test_image_resize_argument_checks_need_no_gpu(R):
    lib = R._lib.lib()
    keep, p = _fake()

    def call(src=p, dst=p, n=1, c=3, h=8, w=8, oh=4, ow=4, iy=p, wy=p, ty=10, ix=p, wx=p, tx=10, u8=0):
        return lib.resr_image_resize(src, dst, n, c, h, w, oh, ow, iy, wy, ty, ix, wx, tx, u8, None)

    for kw in (dict(src=None), dict(dst=None), dict(iy=None), dict(wy=None), dict(ix=None), dict(wx=None)):      # null pointers
        assert call(**kw) == ERR_ARG, kw
        assert b"null" in lib.resr_last_error()
    for kw in (dict(n=0), dict(c=0), dict(h=0), dict(w=-1), dict(oh=0), dict(ow=-3), dict(ty=0), dict(tx=0), dict(ty=4097), dict(tx=-2),
               dict(n=65536), dict(n=30000, c=7)):
        assert call(**kw) == ERR_ARG, kw
    assert call(c=4, u8=1) == ERR_ARG                                # uint8 output is HWC with 3 channels
    assert call(dst=C.c_void_p(p.value + 1), u8=1) == ERR_ARG        # ... stored as dwords
    assert b"aligned" in lib.resr_last_error()
    # a scale whose single-pixel footprint does not fit the LDS tile is refused, not routed elsewhere: r = 0.01 has 402 taps
    assert call(h=4000, w=4000, oh=40, ow=40, ty=402, tx=402) == ERR_ARG
    assert b"footprint" in lib.resr_last_error()
    del keep


def test_compact_forward_u8_scaled_argument_checks_need_no_gpu(R):
    L = R._lib
    lib = L.lib()
    keep, p = _fake()
    good = L.CompactDesc(1, 8, 8, 16, 4, 0, L.RESR_F16, 0)
    ws = lib.resr_compact_workspace_bytes(C.byref(good))
    assert ws > 0

    def call(desc=good, a=(p, p, p, p), wsb=None, y=p, oh=16, ow=16, tabs=(p, p, p, p), ty=10, tx=10):
        d = C.byref(desc) if desc is not None else None
        return lib.resr_compact_forward_u8_scaled(d, a[0], a[1], a[2], a[3], ws if wsb is None else wsb, y, oh, ow,
                                                  tabs[0], tabs[1], ty, tabs[2], tabs[3], tx, None)

    for bad in (L.CompactDesc(0, 8, 8, 16, 4, 0, 0, 0), L.CompactDesc(1, 8, 8, 16, 5, 0, 0, 0), L.CompactDesc(1, 8, 8, 16, 4, 3, 0, 0),
                L.CompactDesc(1, 8, 8, 16, 4, 0, 7, 0), L.CompactDesc(1, 8, 8, -1, 4, 0, 0, 0),
                L.CompactDesc(1, 8192, 4096, 16, 4, 0, L.RESR_F16X2, 0)):
        assert call(desc=bad, wsb=1 << 40) == ERR_ARG
        assert b"descriptor" in lib.resr_last_error()
    assert call(desc=None) == ERR_ARG
    for hole in range(4):                                            # x_u8, params, packed, workspace
        a = [p] * 4
        a[hole] = None
        assert call(a=a) == ERR_ARG, hole
        assert b"null" in lib.resr_last_error()
    assert call(y=None) == ERR_ARG
    for hole in range(4):                                            # idx_y, w_y, idx_x, w_x
        t = [p] * 4
        t[hole] = None
        assert call(tabs=t) == ERR_ARG, hole
        assert b"null" in lib.resr_last_error()
    for kw in (dict(oh=0), dict(ow=0), dict(oh=-4), dict(ty=0), dict(tx=0), dict(tx=5000)):
        assert call(**kw) == ERR_ARG, kw
    assert call(y=C.c_void_p(p.value + 2)) == ERR_ARG
    big = L.CompactDesc(1, 200, 200, 16, 4, 0, L.RESR_F16, 0)       # r = 0.01 on an 800 x 800 frame: 402 taps, no tile fits: refused
    assert call(desc=big, wsb=1 << 40, ty=402, tx=402, oh=8, ow=8) == ERR_ARG
    assert b"footprint" in lib.resr_last_error()
    assert call(wsb=ws - 1) == ERR_WORKSPACE and call(wsb=0) == ERR_WORKSPACE
    assert lib.resr_compact_workspace_bytes(C.byref(good)) == ws     # this path plans nothing of its own
    del keep


def _dense(idx, w, in_length):
    m = np.zeros((idx.shape[0], in_length), np.float32)
    np.add.at(m, (np.repeat(np.arange(idx.shape[0]), idx.shape[1]), idx.reshape(-1).astype(np.int64)), w.reshape(-1))
    return m


def test_band_tables_are_the_resize_matrix(R, golden):
    from real_esrgan_pytorch_amd import imgproc
    lengths = set()
    for h, w, r in golden["cases"]:
        lengths.update([(int(h), float(r)), (int(w), float(r))])
    assert len(lengths) >= 14
    for n, r in sorted(lengths):
        for aa in (True, False):
            out = math.ceil(n * r)
            idx, w = imgproc.resize_band_tables(n, out, r, aa)
            p = math.ceil(4 / min(r, 1) if aa else 4) + 2
            assert idx.shape == w.shape == (out, p) and idx.dtype == np.int32 and w.dtype == np.float32, (n, r, aa)
            assert idx.min() >= 0 and idx.max() < n
            m = imgproc._resize_matrix(n, out, r, aa)
            assert np.array_equal(_dense(idx, w, n), m), (n, r, aa)


def test_resize_matrix_kept_its_parent_values(R, golden):
    from real_esrgan_pytorch_amd import imgproc
    for (n, r, aa), sha in zip(golden["matrix_keys"], golden["matrix_sha256"]):
        n, aa = int(n), bool(aa)
        m = imgproc._resize_matrix(n, math.ceil(n * r), float(r), aa)
        assert m.dtype == np.float32 and hashlib.sha256(m.tobytes()).hexdigest() == str(sha), (n, r, aa)
    assert np.array_equal(imgproc._resize_matrix(8, 3, 0.375, True), golden["matrix_8_0375"])
    assert np.array_equal(imgproc._resize_matrix(4, 2, 0.5, True), golden["matrix_4_05"])
    m64 = imgproc._resize_matrix(16, 8, 0.5, True, np.float64)       # NIQE's form is still served
    assert m64.dtype == np.float64 and np.allclose(m64.sum(1), 1.0)


def test_builder_raises_exactly_where_the_reference_raises(R, golden):
    from real_esrgan_pytorch_amd import imgproc
    table = golden["raise_table"]
    assert len(table) >= 500 and 0 < table[:, 2].sum() < len(table)
    for n, r, raised in table:
        n, r = int(n), float(r)
        try:
            imgproc.resize_band_tables(n, math.ceil(n * r), r)
            got = False
        except ValueError:
            got = True
        assert got == bool(raised), (n, r, raised)
    for h, w, r in ((2, 8, 0.5), (3, 3, 0.5), (4, 12, 0.375)):      # the issue's examples, through the plan the launches use
        with pytest.raises(ValueError, match="shorter than the symmetric copy"):
            imgproc.ResizePlan(h, w, r, "cpu")


def _restate(x, r):
    """Section 1 of the definition in numpy: per axis sequential fp32 accumulation over the tables, H pass first."""
    from real_esrgan_pytorch_amd import imgproc
    _, h, w = x.shape
    iy, wy = imgproc.resize_band_tables(h, math.ceil(h * r), r)
    ix, wx = imgproc.resize_band_tables(w, math.ceil(w * r), r)
    mid = np.zeros((3, iy.shape[0], w), np.float32)
    for k in range(iy.shape[1]):
        mid = (mid + x[:, iy[:, k], :] * wy[None, :, k, None]).astype(np.float32)
    out = np.zeros((3, iy.shape[0], ix.shape[0]), np.float32)
    for k in range(ix.shape[1]):
        out = (out + mid[:, :, ix[:, k]] * wx[None, None, :, k]).astype(np.float32)
    return out


def test_definition_restated_in_numpy_meets_the_reference(R, golden):
    want = {(120, 152, 0.5), (117, 150, 0.75), (92, 100, 0.375), (60, 76, 0.625), (40, 52, 1.5), (4, 4, 0.5), (8, 8, 0.375), (2, 2, 1.5),
            (3, 40, 0.625)}
    assert want <= {(int(h), int(w), float(r)) for h, w, r in golden["cases"]}
    for i, (h, w, r) in enumerate(golden["cases"]):
        x, ref = golden[f"in_{i}"], golden[f"out_{i}"]
        assert x.dtype == np.float32 and x.shape == (3, int(h), int(w))
        got = _restate(x, float(r))
        assert got.shape == ref.shape
        err = float(np.abs(got - ref).max())
        print(f"case {int(h)}x{int(w)} x {r}: max |restatement - reference| = {err:.3e}")
        assert err <= 1e-6, (h, w, r, err)
    big = golden["in_0"]
    assert big.min() < -0.05 and big.max() > 1.05                    # the inputs overshoot [0, 1] as an unclamped SR output does


def test_output_size(R):
    for h, s, o in ((1080, 4, 2), (1080, 4, 1.5), (1080, 4, 3), (1080, 4, 2.5), (37, 3, 2), (37, 3, 1.5), (37, 3, 2.5), (5, 3, 4), (7, 2, 3),
                    (1, 4, 2), (53, 2, 1.5), (719, 3, 2.2)):
        assert R.output_size(h, 2 * h + 1, s, o) == (math.ceil(h * s * (o / s)), math.ceil((2 * h + 1) * s * (o / s))), (h, s, o)
    assert R.output_size(1080, 1920, 4, 2) == (2160, 3840)
    assert R.output_size(1080, 1920, 4) == R.output_size(1080, 1920, 4, None) == R.output_size(1080, 1920, 4, 4) == (4320, 7680)
    assert R.output_size(10, 10, 3, 3.0) == (30, 30)
    for bad in (0, -1, float("nan"), float("inf"), True, "2", [2]):
        with pytest.raises(ValueError, match="outscale"):
            R.output_size(10, 10, 4, bad)


def test_outscale_argument_checks_come_first(R):
    cpu_model = R.SRVGGNetCompact(num_conv=1, precision="fast")
    frames = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    for bad in (0, -2.0, float("nan"), float("inf"), True, False, "2"):
        with pytest.raises(ValueError, match="outscale"):
            R.FrameStream(cpu_model, depth=2, outscale=bad)
        with pytest.raises(ValueError, match="outscale"), torch.no_grad():
            cpu_model.forward_u8(frames, outscale=bad)
    with torch.no_grad():
        for o in (2, 2.5, None, 4):                                  # a valid outscale reaches the device check, as before
            with pytest.raises(RuntimeError, match="no CPU path"):
                cpu_model.forward_u8(frames, outscale=o)
            with pytest.raises(RuntimeError, match="no CPU path"):
                R.upscale_u8(cpu_model, frames, outscale=o)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.FrameStream(cpu_model, depth=2, outscale=2)
    from real_esrgan_pytorch_amd import imgproc
    with pytest.raises(RuntimeError, match="no CPU path"):
        imgproc.image_resize_native(torch.zeros(1, 3, 8, 8), 0.5)
    # tables of the wrong length, or for another size, never reach a launch
    plan = imgproc.ResizePlan(32, 32, 0.5, "cpu")
    assert (plan.out_h, plan.out_w, plan.taps_y, plan.taps_x) == (16, 16, 10, 10)
    plan.check("ok")
    plan.w_x = plan.w_x[:-1]
    with pytest.raises(ValueError, match="tap table"):
        plan.check("short")
    plan = imgproc.ResizePlan(32, 32, 0.5, "cpu")
    plan.out_h = 17                                                  # oh that disagrees with the tables
    with pytest.raises(ValueError, match="tap table"):
        plan.check("oh")
    for bad in (0, -0.5, float("nan"), True):
        with pytest.raises(ValueError, match="scale"):
            imgproc.ResizePlan(32, 32, bad, "cpu")


def test_inference_frames_parser_outscale(R):
    from real_esrgan_pytorch_amd import inference_frames
    p = inference_frames.get_parser()
    base = ["--inputs_dir", "D", "--output_dir", "O", "--weights_path", "W"]
    assert p.parse_args(base).outscale is None
    assert p.parse_args(base + ["--outscale", "2"]).outscale == 2.0
    assert p.parse_args(base + ["--outscale", "1.5"]).outscale == 1.5
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--outscale", "two"])


# ---- the launch plan (resr_debug_resize_plan): the staged region holds every tile's taps, within 64 KB --------------------------------
PLAN_SCALES = (0.75, 0.5, 0.4, 0.3, 0.2, 0.15, 0.125, 0.1, 0.08, 0.07, 0.0625, 0.05, 0.99, 1.0, 1.01, 1.5, 2, 3,
               1 / 3, 0.37, 0.45, 0.618, 0.7, 0.9, 0.11, 0.055, 1.25, 2.5, 3.7)
PLAN_LENGTHS = tuple(range(1, 140)) + (200, 257, 1000, 1920)
PLAN_MIXED = ((0.25, 1.5), (1.5, 0.25), (0.1, 0.75), (0.0625, 3), (0.3, 0.08), (2, 0.15), (0.07, 0.5))
TILE_LIST = ((32, 32), (16, 32), (16, 16), (8, 16), (8, 8), (4, 8), (4, 4), (2, 4), (2, 2), (1, 2), (1, 1))      # choose_tile's, in its order
LDS_BUDGET = 64 * 1024
KINDS = (0, 1, 2, 3)                     # csrc/common.h ResizeOut: fp32, uint8, YUV 8 bits, YUV 10 bits


class _Axis:
    """The tables of one axis, reduced to what the region check needs: per output the lowest and highest source index."""

    def __init__(self, n, r, aa):
        from real_esrgan_pytorch_amd import imgproc
        self.n, self.out = n, math.ceil(n * r)
        idx, _ = imgproc.resize_band_tables(n, self.out, r, aa)
        self.taps = idx.shape[1]
        self.lo, self.hi = idx.min(1), idx.max(1)
        self._span = {}

    def span(self, t):
        """The widest reach of any tile of t consecutive outputs: max(idx) - min(idx) + 1 over the tile's table rows."""
        if t not in self._span:
            starts = np.arange(0, self.out, t)
            self._span[t] = int((np.maximum.reduceat(self.hi, starts) - np.minimum.reduceat(self.lo, starts)).max()) + 1
        return self._span[t]


def _span_bound(t, n_in, n_out, p):
    """csrc/image_resize.hip span_bound, restated: what one axis alone implies."""
    s = p + ((t - 1) * n_in // (n_out - 1) + 2 if t > 1 else 0)
    return min(s, n_in)


def _lds_bytes(th, tw, rh, pitch, py, px, kind):
    staging = 0 if kind == 0 else (th * tw * 3 * (2 if kind == 3 else 1) + 3) // 4 * 4
    return 4 * (2 * (th * py + tw * px) + 3 * (rh + th) * pitch) + staging


def _expected_plan(y, x, kind):
    """The first tile of the list whose LDS fits, each axis sized on its own (None: none fits)."""
    for th, tw in TILE_LIST:
        if kind >= 2 and (th | tw) & 1:
            continue
        rh, rw = _span_bound(min(th, y.out), y.n, y.out, y.taps), _span_bound(min(tw, x.out), x.n, x.out, x.taps)
        lds = _lds_bytes(th, tw, rh, rw | 1, y.taps, x.taps, kind)
        if lds <= LDS_BUDGET:
            return (th, tw, rh, rw, rw | 1, lds)
    return None


def _check_plan(lib, out6, y, x, kind, tally):
    c = 3
    rc = lib.resr_debug_resize_plan(1, c, y.n, x.n, y.out, x.out, y.taps, x.taps, kind, out6)
    want = _expected_plan(y, x, kind)
    what = (y.n, x.n, y.out, x.out, y.taps, x.taps, kind)
    if kind >= 2 and ((y.out | x.out) & 1):
        assert rc == ERR_ARG, what                                 # a 4:2:0 frame has an even height and width
        return
    if want is None:
        assert rc == ERR_ARG, what
        tally["refused"] += 1
        return
    assert rc == 0 and tuple(out6) == want, (what, rc, tuple(out6), want)
    th, tw, rh, rw, pitch, lds = want
    # the condition under which the kernel's clamp into the staged region never acts
    assert y.span(th) <= rh and x.span(tw) <= rw, (what, want, y.span(th), x.span(tw))
    assert lds <= LDS_BUDGET and pitch >= rw and pitch & 1
    assert kind < 2 or not (th | tw) & 1, (what, want)
    tally["plans"] += 1
    tally["tiles"] += -(-y.out // th) * -(-x.out // tw)
    tally[(th, tw)] = tally.get((th, tw), 0) + 1


def test_resize_plan_regions_hold_every_tile(R):
    lib = R._lib.lib()
    out6 = (C.c_int32 * 6)()
    tally = {"plans": 0, "tiles": 0, "refused": 0}

    def axes(r, aa):
        got = {}
        for n in PLAN_LENGTHS:
            try:
                got[n] = _Axis(n, r, aa)
            except ValueError:
                pass                                               # a length the reflection rule refuses: no launch exists
        return got

    for aa in (True, False):
        for r in PLAN_SCALES:
            ax = axes(r, aa)
            names = sorted(ax)
            assert 1 in ax and len(names) > len(PLAN_LENGTHS) // 2, (r, aa, len(names))
            for i, n in enumerate(names):
                for m in {n, names[(7 * i + 3) % len(names)]}:     # the square source, and one of another length
                    for kind in KINDS:
                        _check_plan(lib, out6, ax[n], ax[m], kind, tally)
        for ry, rx in PLAN_MIXED:                                  # two axes with different tap counts
            ay, bx = axes(ry, aa), axes(rx, aa)
            for i, n in enumerate(sorted(ay)):
                ms = sorted(bx)
                m = ms[(5 * i + 1) % len(ms)]
                assert not aa or ay[n].taps != bx[m].taps
                for kind in KINDS:
                    _check_plan(lib, out6, ay[n], bx[m], kind, tally)
    print(f"resize plans checked: {tally['plans']} over {tally['tiles']} tiles, {tally['refused']} refused (no tile fits); "
          f"per tile {{th x tw: plans}}: { {k: v for k, v in tally.items() if isinstance(k, tuple)} }")
    assert tally["plans"] >= 40000 and tally["tiles"] >= 1000000 and tally["refused"] > 0
    assert all(tally.get(t, 0) > 0 for t in TILE_LIST), [t for t in TILE_LIST if not tally.get(t)]      # every entry of the list is reachable


def test_resize_plan_entry_argument_checks(R):
    lib = R._lib.lib()
    out6 = (C.c_int32 * 6)(*([-7] * 6))
    good = dict(n=1, c=3, h=96, w=96, oh=48, ow=48, ty=10, tx=10, kind=1)

    def call(out=out6, **kw):
        a = dict(good, **kw)
        return lib.resr_debug_resize_plan(a["n"], a["c"], a["h"], a["w"], a["oh"], a["ow"], a["ty"], a["tx"], a["kind"], out)

    for kw in (dict(n=0), dict(c=0), dict(h=0), dict(w=-1), dict(oh=0), dict(ow=-3), dict(ty=0), dict(tx=4097), dict(kind=-1), dict(kind=4),
               dict(c=4), dict(c=4, kind=2), dict(oh=47, kind=2), dict(ow=47, kind=3), dict(n=65536), dict(out=None),
               dict(h=4000, w=4000, oh=40, ow=40, ty=402, tx=402)):
        assert call(**kw) == ERR_ARG, kw
        assert list(out6) == [-7] * 6                              # a refused plan leaves the output untouched
    assert call(c=4, kind=0) == 0 and call(c=7, n=3, kind=0) == 0   # channels and batch do not enter the tile
    assert call() == 0 and list(out6) == [16, 32, 42, 75, 75, 56040 + 16 * 32 * 3]
    assert call(kind=0) == 0 and list(out6) == [16, 32, 42, 75, 75, 56040]
    assert call(kind=3) == 0 and list(out6) == [16, 32, 42, 75, 75, 56040 + 16 * 32 * 6]      # 16-bit words in the staging buffer
    assert call(h=6, w=6, oh=2, ow=2, ty=16, tx=16) == 0 and list(out6)[:5] == [32, 32, 6, 6, 7]   # a region is never larger than the source
