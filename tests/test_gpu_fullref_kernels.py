"""-m gpu: the two kernels of the native PSNR / SSIM (csrc/fullref.hip) against tests/fullref_ref.py, through `full_ref_native(keep=True)`.

Gates.  sse and every per-tile sse partial: the reference's integers, bit for bit.  Every per-tile map sum and the final ssim: inside
the bound fullref_ref derives (n = 124, u = 2^-53, first order through the quotient, SLACK 4; a sum adds N u sum|value|); the observed
worst fraction of the bound is printed.  ssim(x, x) == 1.0 exactly; two calls give the same bits; all four (sr kind, hr kind) pairs
give the same bits (one luma behind them).  psnr within 16 * 2^-52 * max(1, |psnr|) of numpy's evaluation of the formula on the same
sse (three roundings of the argument move log10 by under 2 * 2^-52, each libm is taken as within 2 ulp).
Shapes (after the crop; T = RESR_FULLREF_TILE, read from the library): one map value; one row / one column of map values; exactly one
tile; one tile + 1 each way (four tiles, three of them one value wide or high); 3 x 3 tiles with ragged edges; widths 13 and 27 for
3-byte pixels that are nowhere aligned; B = 3 (noise, near copy, identical); crop 0 and 3.  Measured on an MI355X: DESIGN.md."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import fullref_ref as F
from tests import niqe_ref as R

pytestmark = pytest.mark.gpu

PSNR_GATE = 16 * 2.0 ** -52


@pytest.fixture(scope="module")
def L():
    from real_esrgan_pytorch_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def Q():
    from real_esrgan_pytorch_amd import image_quality_assessment
    return image_quality_assessment


def _tile():
    from real_esrgan_pytorch_amd import _lib
    return _lib.RESR_FULLREF_TILE


def _shapes():
    t = _tile()
    return [(11, 11), (11, 75), (75, 11), (t + 10, t + 10), (t + 11, t + 11), (2 * t + 15, 2 * t + 27), (15, 13), (12, 27)]


@functools.lru_cache(maxsize=None)
def _case(h, w, crop, b=3):
    """The shared, read-only reference of one shape: the uint8 pair, its float forms, and fullref_ref.reference with the tiles."""
    sr, hr = F.pair(1000 * h + w + crop, b, h + 2 * crop, w + 2 * crop)
    return {"u8": (sr, hr), "float": (R.unit_of_u8(sr), R.unit_of_u8(hr)), "ref": F.reference(sr, hr, crop, tile=_tile())}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _run(Q, sr, hr, crop):
    out = Q.full_ref_native(torch.from_numpy(np.ascontiguousarray(sr)).cuda(), torch.from_numpy(np.ascontiguousarray(hr)).cuda(), crop, keep=True)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in zip(("psnr", "ssim", "sse", "tile_sse", "tile_sum"), out)}


def _gate(got, ref, label):
    """One call's outputs against the reference dict; -> the worst observed fraction of a bound."""
    assert got["sse"].dtype == np.int64 and got["tile_sse"].dtype == np.int64 and got["tile_sum"].dtype == np.float64
    assert np.array_equal(got["sse"], ref["sse"]), (label, got["sse"], ref["sse"])
    assert got["tile_sse"].shape == ref["tile_sse"].shape and np.array_equal(got["tile_sse"], ref["tile_sse"]), label
    assert np.array_equal(got["tile_sse"].sum(axis=(1, 2)), ref["sse"]), label
    tile_ratio = np.abs(got["tile_sum"] - ref["tile_sum"]) / ref["tile_gate"]
    ssim_ratio = np.abs(got["ssim"] - ref["ssim"]) / ref["ssim_gate"]
    want_psnr = F.psnr_np(got["sse"], ref["h"] * ref["w"])
    psnr_ratio = np.abs(got["psnr"] - want_psnr) / (PSNR_GATE * np.maximum(1.0, np.abs(want_psnr)))
    print(f"{label}: tile sums at {tile_ratio.max():.3e} of their bound, ssim at {ssim_ratio.max():.3e} of its ({ref['ssim_gate'].max():.2e}), "
          f"psnr at {psnr_ratio.max():.3f} of its gate; ssim {got['ssim']}, psnr {got['psnr']}")
    assert (tile_ratio <= 1).all(), (label, "tile sums", float(tile_ratio.max()))
    assert (ssim_ratio <= 1).all(), (label, "ssim", float(ssim_ratio.max()))
    assert (psnr_ratio <= 1).all(), (label, "psnr", float(psnr_ratio.max()))
    return float(max(tile_ratio.max(), ssim_ratio.max()))


@pytest.mark.parametrize("crop", [0, 3])
@pytest.mark.parametrize("shape", _shapes(), ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_shape_and_kind_against_the_reference(Q, shape, crop):
    c = _case(shape[0], shape[1], crop)
    ref = c["ref"]
    first = None
    for ks in ("u8", "float"):
        for kh in ("u8", "float"):
            got = _run(Q, c[ks][0], c[kh][1], crop)
            _gate(got, ref, f"{shape[0]}x{shape[1]} crop {crop} sr {ks} hr {kh}")
            assert got["ssim"][2] == 1.0 and got["sse"][2] == 0                     # image 2: sr is hr
            if first is None:
                first = got
                again = _run(Q, c[ks][0], c[kh][1], crop)
                for k in got:
                    assert np.array_equal(_bits(got[k]), _bits(again[k])), ("two calls", k)
            for k in got:
                assert np.array_equal(_bits(got[k]), _bits(first[k])), ("kinds", ks, kh, k)


def test_flat_extremes_every_pixel_belongs_to_one_tile(Q):
    """255 against 0 (float images outside [0,1]: the level is pinned): every squared difference is 65025, so a tile's sse counts the
    pixels it owns; and 255 against 255, where the bound is at its largest (7e-10) and the answer is 1.0 exactly."""
    t = _tile()
    h, w, crop = 2 * t + 15, 2 * t + 27, 1
    hi, lo = np.full((1, 3, h + 2, w + 2), 2.0, np.float32), np.full((1, 3, h + 2, w + 2), -1.0, np.float32)
    ref = F.reference(hi, lo, crop, tile=t)
    got = _run(Q, hi, lo, crop)
    _gate(got, ref, "255 against 0")
    assert got["sse"][0] == 65025 * h * w
    rows, cols = [t, t, h - 2 * t], [t, t, w - 2 * t]
    assert np.array_equal(got["tile_sse"][0], 65025 * np.outer(rows, cols))
    same = _run(Q, hi, hi, crop)
    _gate(same, F.reference(hi, hi, crop, tile=t), "255 against 255")
    assert same["ssim"][0] == 1.0 and same["sse"][0] == 0 and (same["tile_sse"] == 0).all()


def test_more_tiles_than_the_finish_kernel_has_threads(Q, L):
    t, threads = _tile(), L.RESR_FULLREF_FINISH_THREADS
    ty, tx = 16, threads // 16 + 1
    assert ty * tx > threads
    h, w = (ty - 1) * t + 5 + 10, (tx - 1) * t + 7 + 10
    c = _case(h, w, 0, b=1)
    got = _run(Q, c["u8"][0], c["float"][1], 0)
    assert got["tile_sum"].shape == (1, ty, tx)
    _gate(got, c["ref"], f"{h}x{w}: {ty * tx} tiles, {threads} threads")
    x = c["u8"][1]
    same = _run(Q, x, x, 0)
    assert same["ssim"].tolist() == [1.0] and same["sse"].tolist() == [0]


def _launch_ids(L, fn):
    lib = L.lib()
    lib.resr_profile_begin()
    try:
        out = fn()
    finally:
        torch.cuda.synchronize()
        buf = (L.ProfEntry * 64)()
        n = int(lib.resr_profile_end(C.cast(buf, C.c_void_p), 64))
    return out, [buf[i].kernel_id for i in range(n)]


def test_two_launches_with_their_own_ids(Q, L):
    c = _case(11, 75, 0)
    for ks, kh, first in (("float", "float", 34600), ("u8", "float", 34601), ("float", "u8", 34602), ("u8", "u8", 34603)):
        sr, hr = torch.from_numpy(c[ks][0]).cuda(), torch.from_numpy(c[kh][1]).cuda()
        _, ids = _launch_ids(L, lambda: Q.full_ref_native(sr, hr, 0))
        assert ids == [first, 34700], (ks, kh, ids)


def test_refused_descriptors_launch_nothing(Q, L):
    lib = L.lib()
    sr = torch.zeros((2, 3, 40, 50), dtype=torch.float32, device="cuda")
    hr = torch.zeros((2, 40, 50, 3), dtype=torch.uint8, device="cuda")
    ws = torch.zeros(64, dtype=torch.int64, device="cuda")
    sse = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = torch.zeros((2, 2), dtype=torch.float64, device="cuda")
    stream = L.stream_ptr(sr)

    def desc(**kw):
        d = L.FullRefDesc()
        d.n, d.h, d.w, d.crop, d.sr_u8, d.hr_u8 = 2, 40, 50, 2, 0, 1
        d.workspace, d.workspace_bytes = ws.data_ptr(), 64 * 8
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def call(d, **ptrs):
        p = {"sr": L.ptr(sr), "hr": L.ptr(hr), "sse": L.ptr(sse), "psnr": L.ptr(out[0]), "ssim": L.ptr(out[1])}
        p.update(ptrs)
        return lib.resr_fullref(C.byref(d) if d is not None else None, p["sr"], p["hr"], p["sse"], p["psnr"], p["ssim"], stream)

    need = int(lib.resr_fullref_workspace_bytes(desc()))
    ty, tx = Q.full_ref_tiles(36, 46)
    assert need == 2 * ty * tx * 16 and need <= 64 * 8
    refused = [("null descriptor", lambda: call(None)), ("n = 0", lambda: call(desc(n=0))), ("crop < 0", lambda: call(desc(crop=-1))),
               ("crop leaves 10 rows", lambda: call(desc(crop=15))), ("h = 0", lambda: call(desc(h=0))),
               ("short workspace", lambda: call(desc(workspace_bytes=need - 1))), ("null workspace", lambda: call(desc(workspace=None))),
               ("tile index", lambda: call(desc(n=70000, h=2 ** 20, w=2 ** 20))),
               ("misaligned psnr", lambda: call(desc(), psnr=C.c_void_p(out.data_ptr() + 4))),
               ("misaligned float image", lambda: call(desc(), sr=C.c_void_p(sr.data_ptr() + 2)))]
    refused += [(f"null {k}", lambda k=k: call(desc(), **{k: None})) for k in ("sr", "hr", "sse", "psnr", "ssim")]
    for label, fn in refused:
        rc, ids = _launch_ids(L, fn)
        assert rc == L.RESR_ERR_ARG and ids == [], (label, rc, ids)
        assert b"fullref" in lib.resr_last_error(), label
    rc, ids = _launch_ids(L, lambda: call(desc()))
    assert rc == L.RESR_OK and len(ids) == 2
    assert sse.tolist() == [0, 0] and out[1].tolist() == [1.0, 1.0]          # black against black
    with pytest.raises(ValueError, match="11x11"):
        Q.full_ref_native(sr, hr, 15)


def test_scores_follow_the_current_stream(Q):
    """The producer and the metric on a side stream, nothing on the default stream and no host synchronisation in between: a launch
    enqueued anywhere but the current stream would read the frame before the copy behind the matrix products has filled it."""
    c = _case(2 * _tile() + 15, 2 * _tile() + 27, 3)
    frame, truth = torch.from_numpy(c["u8"][0]).cuda(), torch.from_numpy(c["float"][1]).cuda()
    want = [t.cpu().numpy() for t in Q.full_ref_native(frame, truth, 3)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        late = torch.zeros_like(frame)
        a = torch.full((2048, 2048), 1.0 / 2048, device="cuda")
        for _ in range(50):
            a = a @ a
        late.copy_(frame)
        got = Q.full_ref_native(late, truth, 3)
    side.synchronize()
    for g, w in zip(got, want):
        assert np.array_equal(_bits(g.cpu().numpy()), _bits(w))
