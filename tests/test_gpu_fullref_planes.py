"""-m gpu: the native PSNR / SSIM per plane (csrc/fullref.hip, resr_fullref_planes) against tests/fullref_planes_ref.py, through
`full_ref_planes_native(keep=True)`, `full_ref_channels_native`, `full_ref_yuv_native` and the two tools.

Gates, as tests/test_gpu_fullref_kernels.py.  sse and every per-tile sse partial: the reference's integers, bit for bit.  Every per-tile
map sum and the final ssim: inside the bound fullref_ref derives (relative to the window sums, so at another peak only C1 and C2
change).  psnr within 16 * 2^-52 * max(1, |psnr|) of numpy's evaluation of the formula on the same sse.  X == Y: sse 0, ssim == 1.0,
psnr == 10 log10(peak^2 / 1e-8).  A one-plane view of the luma levels of an RGB pair: the bits of resr_fullref on the pair.
Plane sizes (T = 32): 11 x 11 is one map value; 12 x 43 has a 33-wide map, two tiles, the second one value wide and owner of the apron;
43 x 12 the same downwards; 75 x 53 is 3 x 2 tiles with ragged edges, at crop 0, 1 and 4 (4: 67 x 45, two tile rows)."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from tests import fullref_planes_ref as P
from tests import fullref_ref as F

pytestmark = pytest.mark.gpu

PSNR_GATE = 16 * 2.0 ** -52
TILE = 32
SIZES = [(11, 11, 0), (12, 43, 0), (43, 12, 0), (75, 53, 0), (75, 53, 1), (75, 53, 4)]
# name -> (numpy word, peak, shift, bits of garbage around the level)
KINDS = {"u8": (np.uint8, 255, 0, 0), "u16": (np.uint16, 65535, 0, 0), "10lo": (np.uint16, 1023, 0, 6), "10hi": (np.uint16, 1023, 6, 6)}


@pytest.fixture(scope="module")
def L():
    from real_esrgan_pytorch_amd import _lib
    assert _lib.RESR_FULLREF_TILE == TILE
    return _lib


@pytest.fixture(scope="module")
def Q():
    from real_esrgan_pytorch_amd import image_quality_assessment
    return image_quality_assessment


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _pair(seed, n, planes, h, w, peak):
    """Levels int64 [n,planes,h,w]: hr noise; sr of image 0 independent noise, of every further image hr +- peak / 64."""
    rng = np.random.default_rng(seed)
    hr = rng.integers(0, peak + 1, (n, planes, h, w))
    sr = np.clip(hr + rng.integers(-(peak // 64), peak // 64 + 1, hr.shape), 0, peak)
    sr[0] = rng.integers(0, peak + 1, (planes, h, w))
    return sr, hr


def _words(levels, kind, seed=0):
    """Levels [n,planes,h,w] as interleaved words [n,h,w,planes] of `kind` (garbage in the bits the mask drops) and their view."""
    word, peak, shift, junk = KINDS[kind]
    n, planes, h, w = levels.shape
    a = levels.transpose(0, 2, 3, 1) << shift
    if junk:
        g = np.random.default_rng(seed).integers(0, 1 << junk, a.shape)
        a = a | (g << 10 if shift == 0 else g)
    return np.ascontiguousarray(a.astype(word)), P.View(np.dtype(word).itemsize, shift, peak, 0, planes, w * planes, 1, h * w * planes)


def _floats(levels, peak, seed=0):
    """fp32 [n,planes,h,w] whose levels at `peak` are `levels` wherever these are not 0 or peak; there values below 0, above 1 and
    NaN are mixed in -> (array, view, the levels it has: NaN and negatives 0, above 1 peak)."""
    rng = np.random.default_rng(seed)
    v = ((levels.astype(np.float64) + 0.5) / peak).astype(np.float32)
    v[levels == 0] = rng.choice(np.array([-3.0, -0.0, np.nan, -np.inf], np.float32), int((levels == 0).sum()))
    v[levels == peak] = rng.choice(np.array([1.0, 1.5, np.inf], np.float32), int((levels == peak).sum()))
    v.reshape(-1)[:3] = (np.nan, -1.0, 2.0)
    n, planes, h, w = levels.shape
    return v, P.View(4, 0, 0, 0, 1, w, h * w, planes * h * w), P.quantise(v, peak)


def _run(Q, sr, sr_view, hr, hr_view, n, planes, h, w, crop, peak):
    out = Q.full_ref_planes_native(torch.from_numpy(np.ascontiguousarray(sr)).cuda(), Q.PlaneView(*sr_view), torch.from_numpy(np.ascontiguousarray(hr)).cuda(), Q.PlaneView(*hr_view),
                                   n, planes, h, w, crop, peak, keep=True)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in zip(("sse", "psnr", "ssim", "tile_sse", "tile_sum"), out)}


def _gate(got, X, Y, crop, peak, label):
    """One call's outputs [n,planes,...] against the reference of the levels X, Y [n,planes,h,w] (before the crop)."""
    n, planes = X.shape[:2]
    ref = P.reference(P.crop(X, crop).reshape((n * planes,) + P.crop(X, crop).shape[2:]), P.crop(Y, crop).reshape((n * planes,) + P.crop(Y, crop).shape[2:]), peak, tile=TILE)
    flat = {k: v.reshape((n * planes,) + v.shape[2:]) for k, v in got.items()}
    assert flat["sse"].dtype == np.int64 and flat["tile_sse"].dtype == np.int64 and flat["tile_sum"].dtype == np.float64 and got["sse"].shape == (n, planes)
    assert np.array_equal(flat["sse"], ref["sse"]), (label, flat["sse"], ref["sse"])
    assert flat["tile_sse"].shape == ref["tile_sse"].shape and np.array_equal(flat["tile_sse"], ref["tile_sse"]), label
    tile_ratio = np.abs(flat["tile_sum"] - ref["tile_sum"]) / ref["tile_gate"]
    ssim_ratio = np.abs(flat["ssim"] - ref["ssim"]) / ref["ssim_gate"]
    want_psnr = P.psnr_np(flat["sse"], ref["h"] * ref["w"], peak)
    psnr_ratio = np.abs(flat["psnr"] - want_psnr) / (PSNR_GATE * np.maximum(1.0, np.abs(want_psnr)))
    print(f"{label}: tile sums at {tile_ratio.max():.3e} of their bound, ssim at {ssim_ratio.max():.3e} of its ({ref['ssim_gate'].max():.2e}), "
          f"psnr at {psnr_ratio.max():.3f} of its gate")
    assert (tile_ratio <= 1).all(), (label, "tile sums", float(tile_ratio.max()))
    assert (ssim_ratio <= 1).all(), (label, "ssim", float(ssim_ratio.max()))
    assert (psnr_ratio <= 1).all(), (label, "psnr", float(psnr_ratio.max()))
    return ref


@pytest.mark.parametrize("planes", [1, 3, 4])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}-crop{s[2]}")
def test_every_size_and_source_kind_against_the_reference(Q, size, planes):
    h, w, crop = size
    n = 2
    for kind, (word, peak, shift, junk) in KINDS.items():
        X, Y = _pair(h * 1000 + w + crop + planes, n, planes, h, w, peak)
        sr, sv = _words(X, kind, 1)
        hr, hv = _words(Y, kind, 2)
        got = _run(Q, sr, sv, hr, hv, n, planes, h, w, crop, peak)
        _gate(got, X, Y, crop, peak, f"{h}x{w} crop {crop} C={planes} {kind}")
        again = _run(Q, sr, sv, hr, hv, n, planes, h, w, crop, peak)
        for k in got:
            assert np.array_equal(_bits(got[k]), _bits(again[k])), ("two calls", kind, k)
        same = _run(Q, hr, hv, hr.copy(), hv, n, planes, h, w, crop, peak)          # X == Y
        assert (same["sse"] == 0).all() and (same["tile_sse"] == 0).all() and (same["ssim"] == 1.0).all()
        top = 10.0 * np.log10(float(peak * peak) / 1e-8)                             # (two libms: the psnr gate, as everywhere)
        assert (np.abs(same["psnr"] - top) <= PSNR_GATE * top).all(), (same["psnr"], top)
        if kind != "10hi" and planes != 4:                                           # the fp32 side, quantised to the integer side's peak
            f, fv, Xf = _floats(X, peak, 3)
            got = _run(Q, f, fv, hr, hv, n, planes, h, w, crop, peak)
            _gate(got, Xf, Y, crop, peak, f"{h}x{w} crop {crop} C={planes} float against {kind}")
            swapped = _run(Q, hr, hv, f, fv, n, planes, h, w, crop, peak)
            assert np.array_equal(swapped["sse"], got["sse"]) and np.array_equal(swapped["tile_sse"], got["tile_sse"])


def test_checkerboard_at_65535_needs_the_64_bit_sse(Q):
    """0 / 65535 against its inverse: every squared difference is 65535^2 = 4,294,836,225, two of them overflow 32 bits."""
    h, w = 43, 53
    board = ((np.add.outer(np.arange(h), np.arange(w)) % 2) * 65535)[None, None]
    sr, sv = _words(board, "u16")
    hr, hv = _words(65535 - board, "u16")
    got = _run(Q, sr, sv, hr, hv, 1, 1, h, w, 0, 65535)
    _gate(got, board, 65535 - board, 0, 65535, "checkerboard")
    assert got["sse"].tolist() == [[65535 * 65535 * h * w]]
    assert np.array_equal(got["tile_sse"][0, 0], 65535 * 65535 * np.outer([32, 11], [32, 21]))


def test_strides_offsets_and_mixed_views(Q):
    h, w, n, peak = 23, 37, 2, 255
    X, Y = _pair(5, n, 4, h, w, peak)
    sr4, _ = _words(X, "u8")
    hr4, _ = _words(Y, "u8")
    # one plane out of 2, 3 or 4 interleaved ones: pixel strides 2, 3, 4; the plane chosen by the base
    for stride in (2, 3, 4):
        for p in range(stride):
            sr, hr = np.ascontiguousarray(sr4[..., :stride]), np.ascontiguousarray(hr4[..., :stride])
            v = P.View(1, 0, 255, p, stride, w * stride, 0, h * w * stride)
            got = _run(Q, sr, v, hr, v, n, 1, h, w, 1, peak)
            _gate(got, X[:, p:p + 1], Y[:, p:p + 1], 1, peak, f"pixel stride {stride} plane {p}")
    # planar against interleaved (mixed views), float against uint16, and bases that leave the plane at an odd byte (uint8) and at a
    # word that is not 4-byte aligned (uint16)
    planar = np.ascontiguousarray(X.astype(np.uint8))                        # [n,4,h,w]
    pad = np.concatenate([np.full(3, 77, np.uint8), planar.reshape(-1)])
    got = _run(Q, pad, P.View(1, 0, 255, 3, 1, w, h * w, 4 * h * w), hr4, P.View(1, 0, 255, 0, 4, 4 * w, 1, 4 * h * w), n, 4, h, w, 0, peak)
    _gate(got, X, Y, 0, peak, "planar at an odd address against interleaved")
    X16, Y16 = _pair(6, n, 3, h, w, 65535)
    hr16, hv16 = _words(Y16, "u16")
    pad16 = np.concatenate([np.full(5, 999, np.uint16), X16.astype(np.uint16).reshape(-1)])
    assert torch.from_numpy(pad16).cuda().data_ptr() % 4 == 0               # so word 5 is 2 bytes off a dword
    got = _run(Q, pad16, P.View(2, 0, 65535, 5, 1, w, h * w, 3 * h * w), hr16, hv16, n, 3, h, w, 2, 65535)
    _gate(got, X16, Y16, 2, 65535, "uint16 planar at a word off a dword against interleaved")
    f, fv, Xf = _floats(X16, 65535, 9)
    got = _run(Q, f, fv, hr16, hv16, n, 3, h, w, 0, 65535)
    _gate(got, Xf, Y16, 0, 65535, "float against uint16")


@pytest.mark.parametrize("bits", [8, 10])
def test_planar_and_semi_planar_chroma_give_the_same_numbers(Q, bits):
    n, h, w = 2, 34, 46
    names = ("i420", "nv12") if bits == 8 else ("i420p10", "p010")
    peak = (1 << bits) - 1
    rng = np.random.default_rng(bits)
    planes = [rng.integers(0, peak + 1, s) for s in ((n, h, w), (n, h // 2, w // 2), (n, h // 2, w // 2))]
    other = [np.clip(a + rng.integers(-5, 6, a.shape), 0, peak) for a in planes]
    other[0][0], other[1][0], other[2][0] = (rng.integers(0, peak + 1, a.shape[1:]) for a in planes)

    def frame(name, y, cb, cr):
        chroma = np.stack([cb, cr], axis=-1).reshape(n, -1) if name in ("nv12", "p010") else np.concatenate([cb.reshape(n, -1), cr.reshape(n, -1)], axis=1)
        f = np.concatenate([y.reshape(n, -1), chroma], axis=1).reshape(n, 3 * h // 2, w)
        if name == "p010":
            f = (f << 6) | rng.integers(0, 64, f.shape)
        elif name == "i420p10":
            f = f | (rng.integers(0, 64, f.shape) << 10)
        return torch.from_numpy(f.astype(np.uint8 if bits == 8 else np.uint16)).cuda()

    results = {}
    for a in names:
        for b in names:
            got = Q.full_ref_yuv_native(frame(a, *other), frame(b, *planes), a, b, 2)
            results[a, b] = np.stack([t.cpu().numpy() for t in got])
    first = results[names[0], names[0]]
    for key, value in results.items():
        assert np.array_equal(_bits(value), _bits(first)), key
    refs = [P.reference(P.crop(a, c), P.crop(b, c), peak) for a, b, c in zip(other, planes, (2, 1, 1))]
    for i, r in enumerate(refs):
        assert (np.abs(first[4 + i] - r["ssim"]) <= r["ssim_gate"]).all()
        assert (np.abs(first[i] - r["psnr"]) <= PSNR_GATE * np.maximum(1.0, np.abs(r["psnr"]))).all()
    want = P.psnr_np(sum(r["sse"] for r in refs), (h - 4) * (w - 4) + 2 * (h // 2 - 2) * (w // 2 - 2), peak)
    assert (np.abs(first[3] - want) <= PSNR_GATE * np.maximum(1.0, np.abs(want))).all()


def test_one_plane_view_of_the_luma_levels_is_resr_fullref(Q):
    """The tie to the existing kernel: same sse, tile partials, ssim and psnr bits as `full_ref_native(keep=True)` on the RGB pair."""
    crop, h, w = 3, 2 * TILE + 15, 2 * TILE + 27
    sr, hr = F.pair(77, 3, h + 2 * crop, w + 2 * crop)
    psnr, ssim, sse, tile_sse, tile_sum = (t.cpu().numpy() for t in Q.full_ref_native(torch.from_numpy(sr).cuda(), torch.from_numpy(hr).cuda(), crop, keep=True))
    X, Y = F.levels(sr, crop), F.levels(hr, crop)                           # uint8 [3,h,w], already cropped
    view = P.View(1, 0, 255, 0, 1, w, 0, h * w)
    got = _run(Q, X, view, Y, view, 3, 1, h, w, 0, 255)
    for mine, theirs in ((got["sse"][:, 0], sse), (got["tile_sse"][:, 0], tile_sse), (got["tile_sum"][:, 0], tile_sum), (got["ssim"][:, 0], ssim), (got["psnr"][:, 0], psnr)):
        assert mine.shape == theirs.shape and np.array_equal(_bits(mine), _bits(theirs))
    assert got["ssim"][2, 0] == 1.0


def test_last_image_past_two_gib(Q):
    """Image 1 starts at byte 2^31 + 5: an offset kept in 32 bits would read image 0 again (or fault)."""
    h = w = 13
    stride = 2 ** 31 + 5
    X, Y = _pair(31, 2, 1, h, w, 255)
    big = torch.empty(stride + h * w, dtype=torch.uint8, device="cuda")
    for i in range(2):
        big[i * stride:i * stride + h * w] = torch.from_numpy(X[i, 0].astype(np.uint8).reshape(-1)).cuda()
    hr, hv = _words(Y, "u8")
    out = Q.full_ref_planes_native(big, Q.PlaneView(1, 0, 255, 0, 1, w, 0, stride), torch.from_numpy(hr).cuda(), Q.PlaneView(*hv), 2, 1, h, w, 0, 255, keep=True)
    torch.cuda.synchronize()
    got = {k: t.cpu().numpy() for k, t in zip(("sse", "psnr", "ssim", "tile_sse", "tile_sum"), out)}
    _gate(got, X, Y, 0, 255, "image 1 past 2 GiB")
    assert got["sse"][0, 0] != got["sse"][1, 0]
    with pytest.raises(ValueError, match="reaches word"):                   # Python refuses a view that leaves its tensor
        Q.full_ref_planes_native(big, Q.PlaneView(1, 0, 255, 1, 1, w, 0, stride), torch.from_numpy(hr).cuda(), Q.PlaneView(*hv), 2, 1, h, w, 0, 255)


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


def test_two_launches_whatever_n_and_planes_are(Q, L):
    for n, planes in ((1, 1), (3, 4)):
        X, Y = _pair(1, n, planes, 12, 43, 255)
        sr, sv = _words(X, "u8")
        hr, hv = _words(Y, "u8")
        a, b = torch.from_numpy(sr).cuda(), torch.from_numpy(hr).cuda()
        _, ids = _launch_ids(L, lambda: Q.full_ref_planes_native(a, Q.PlaneView(*sv), b, Q.PlaneView(*hv), n, planes, 12, 43, 0, 255))
        assert ids == [34604, 34701], (n, planes, ids)
    frames = torch.zeros(2, 36, 24, dtype=torch.uint8, device="cuda")
    _, ids = _launch_ids(L, lambda: Q.full_ref_yuv_native(frames, frames, "i420", "nv12"))
    assert ids == [34604, 34701] * 2                                         # luma, chroma


def test_refused_descriptors_launch_nothing(Q, L):
    from tests.test_fullref_planes_surface import REFUSED, _desc
    lib = L.lib()
    sr = torch.zeros(2 * 40 * 50 * 3 + 8, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(64, dtype=torch.int64, device="cuda")
    sse = torch.zeros((2, 3), dtype=torch.int64, device="cuda")
    out = torch.zeros((2, 2, 3), dtype=torch.float64, device="cuda")
    stream = L.stream_ptr(sr)

    def desc(**kw):
        return _desc(L, **{"workspace": ws.data_ptr(), "workspace_bytes": 64 * 8, **kw})

    def call(d, **ptrs):
        p = {"sr": L.ptr(sr), "hr": L.ptr(sr), "sse": L.ptr(sse), "psnr": L.ptr(out[0]), "ssim": L.ptr(out[1])}
        p.update(ptrs)
        return lib.resr_fullref_planes(C.byref(d) if d is not None else None, p["sr"], p["hr"], p["sse"], p["psnr"], p["ssim"], stream)

    need = int(lib.resr_fullref_planes_workspace_bytes(desc()))
    assert need == 2 * 3 * 1 * 2 * 16 and need <= 64 * 8                     # 36 x 46 after the crop: 1 x 2 tiles
    refused = [("null descriptor", lambda: call(None))] + [(f"{k} = {v}", lambda k=k, v=v: call(desc(**{k: v}))) for k, v in REFUSED]
    refused += [("short workspace", lambda: call(desc(workspace_bytes=need - 1))), ("null workspace", lambda: call(desc(workspace=None))),
                ("misaligned workspace", lambda: call(desc(workspace=ws.data_ptr() + 4))),
                ("tile index", lambda: call(desc(n=70000, planes=4, h=2 ** 20, w=2 ** 20))),
                ("misaligned psnr", lambda: call(desc(), psnr=C.c_void_p(out.data_ptr() + 4))),
                ("misaligned sse", lambda: call(desc(), sse=C.c_void_p(sse.data_ptr() + 4))),
                ("uint16 words at an odd address", lambda: call(desc(sr_word_bytes=2, sr_pixel_stride=1, sr_row_stride=50, sr_plane_stride=0, sr_image_stride=0), sr=C.c_void_p(sr.data_ptr() + 1))),
                ("float words off a dword", lambda: call(desc(hr_word_bytes=4, hr_pixel_stride=1, hr_row_stride=50, hr_plane_stride=0, hr_image_stride=0), hr=C.c_void_p(sr.data_ptr() + 2)))]
    refused += [(f"null {k}", lambda k=k: call(desc(), **{k: None})) for k in ("sr", "hr", "sse", "psnr", "ssim")]
    for label, fn in refused:
        rc, ids = _launch_ids(L, fn)
        assert rc == L.RESR_ERR_ARG and ids == [], (label, rc, ids)
        assert b"fullref_planes" in lib.resr_last_error(), label
    rc, ids = _launch_ids(L, lambda: call(desc()))
    assert rc == L.RESR_OK and ids == [34604, 34701]
    assert sse.eq(0).all() and out[1].eq(1.0).all()                          # zeros against zeros
    rc, ids = _launch_ids(L, lambda: call(desc(), sr=C.c_void_p(sr.data_ptr() + 1)))      # uint8 words need no alignment
    assert rc == L.RESR_OK and len(ids) == 2
    torch.cuda.synchronize()


def test_channels_api_against_the_reference_and_the_twin(Q, monkeypatch):
    b, h, w, crop = 2, 34, 46, 2
    for kind, c in (("u8", 3), ("u16", 3), ("u8", 1), ("u16", 4)):
        peak = KINDS[kind][1]
        X, Y = _pair(41 + c, b, c, h, w, peak)
        sr, _ = _words(X, kind)
        hr, _ = _words(Y, kind)
        sides = [(torch.from_numpy(sr), X), (torch.from_numpy(hr), Y)]
        if c != 4:
            f, _, Xf = _floats(X, peak, 4)
            sides.append((torch.from_numpy(f), Xf))
        for (a, A), (t, T) in ((sides[0], sides[1]), (sides[-1], sides[1]), (sides[1], sides[-1])):
            got = Q.full_ref_channels_native(a.cuda(), t.cuda(), crop)
            twin = Q.full_ref_channels(a, t, crop)
            ref = P.reference(P.crop(A, crop).reshape(b * c, h - 2 * crop, w - 2 * crop), P.crop(T, crop).reshape(b * c, h - 2 * crop, w - 2 * crop), peak)
            psnr_all, mean, gate = P.channels_summary(ref, b, c, peak)
            for r in (got, twin):
                assert r.sse.dtype == torch.int64 and r.psnr_all.dtype == torch.float64 and tuple(r.ssim.shape) == (b, c) and tuple(r.ssim_mean.shape) == (b,)
                assert np.array_equal(r.sse.cpu().numpy().reshape(-1), ref["sse"])
                assert (np.abs(r.ssim.cpu().numpy().reshape(-1) - ref["ssim"]) <= ref["ssim_gate"]).all()
                assert (np.abs(r.psnr.cpu().numpy().reshape(-1) - ref["psnr"]) <= PSNR_GATE * np.maximum(1.0, np.abs(ref["psnr"]))).all()
                assert (np.abs(r.psnr_all.cpu().numpy() - psnr_all) <= PSNR_GATE * np.maximum(1.0, np.abs(psnr_all))).all()
                assert (np.abs(r.ssim_mean.cpu().numpy() - mean) <= gate).all()
    # both sides float: 8 bits; keep=True hands out the partials
    f, g = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(1)), torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(2))
    got, tile_sse, tile_sum = Q.full_ref_channels_native(f.cuda(), g.cuda(), 0, keep=True)
    assert tuple(tile_sse.shape) == tuple(tile_sum.shape) == (b, 3, 1, 2) and torch.equal(tile_sse.sum(dim=(2, 3)), got.sse)
    assert np.array_equal(got.sse.cpu().numpy(), Q.full_ref_channels(f, g, 0).sse.numpy())
    # config.build_full_ref() with RESR_FULL_REF_CHANNELS=rgb: (psnr_all, ssim_mean) through either backend
    from real_esrgan_pytorch_amd import config
    monkeypatch.setattr(config, "device", torch.device("cuda", 0))
    monkeypatch.setattr(config, "full_ref_channels", "rgb")
    crop = config.upscale_factor
    want = Q.full_ref_channels_native(f.cuda(), g.cuda(), crop)
    ref = P.reference(*(P.crop(P.quantise(t.numpy(), 255), crop).reshape(b * 3, h - 2 * crop, w - 2 * crop) for t in (f, g)), 255)
    psnr_all, mean, gate = P.channels_summary(ref, b, 3, 255)
    for backend, cls in (("native", Q.NativeFullRefChannels), ("torch", Q.TorchFullRefChannels)):
        monkeypatch.setattr(config, "full_ref", backend)
        m = config.build_full_ref()
        assert type(m) is cls
        p, s = m(f.cuda(), g.cuda())
        assert p.is_cuda and p.dtype == torch.float64 and tuple(p.shape) == (b,) and tuple(s.shape) == (b,)
        if backend == "native":
            assert torch.equal(p, want.psnr_all) and torch.equal(s, want.ssim_mean)
        assert (np.abs(p.cpu().numpy() - psnr_all) <= PSNR_GATE * np.maximum(1.0, np.abs(psnr_all))).all() and (np.abs(s.cpu().numpy() - mean) <= gate).all()


@functools.lru_cache(maxsize=None)
def _yuv_case(name, other, h, w):
    from tests.test_fullref_planes_surface import _yuv_frames
    rng = np.random.default_rng(h + w)
    ref_frame, planes, peak = _yuv_frames(rng, other, 2, h, w)
    frame, mine, _ = _yuv_frames(rng, name, 2, h, w, near=planes)
    return frame, ref_frame, mine, planes, peak


@pytest.mark.parametrize("name,other", [("i420", "nv12"), ("nv12", "i420"), ("i420p10", "p010"), ("p010", "i420p10")])
@pytest.mark.parametrize("size", [(64, 96), (34, 46)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_yuv_api_against_the_reference_and_the_twin(Q, size, name, other):
    """Luma 64 x 96 (what a 16 x 24 frame becomes at x4) and 34 x 46 (chroma 17 x 23: one tile, odd sizes), crop 0 and 2."""
    h, w = size
    frame, ref_frame, mine, planes, peak = _yuv_case(name, other, h, w)
    for crop in (0, 2):
        got = Q.full_ref_yuv_native(torch.from_numpy(frame).cuda(), torch.from_numpy(ref_frame).cuda(), name, other, crop)
        twin = Q.full_ref_yuv(torch.from_numpy(frame), torch.from_numpy(ref_frame), name, other, crop)
        refs = [P.reference(P.crop(a, c), P.crop(b, c), peak) for a, b, c in zip(mine, planes, (crop, crop // 2, crop // 2))]
        want = P.psnr_np(sum(r["sse"] for r in refs), (h - 2 * crop) * (w - 2 * crop) + 2 * (h // 2 - crop) * (w // 2 - crop), peak)
        for r in (got, twin):
            for i, ref in enumerate(refs):
                assert (np.abs(r[4 + i].cpu().numpy() - ref["ssim"]) <= ref["ssim_gate"]).all(), (crop, i)
                assert (np.abs(r[i].cpu().numpy() - ref["psnr"]) <= PSNR_GATE * np.maximum(1.0, np.abs(ref["psnr"]))).all(), (crop, i)
            assert (np.abs(r.psnr_avg.cpu().numpy() - want) <= PSNR_GATE * np.maximum(1.0, np.abs(want))).all()
    dev = torch.from_numpy(frame).cuda()
    with pytest.raises(ValueError, match="even"):
        Q.full_ref_yuv_native(dev, dev, name, None, 1)
    with pytest.raises(ValueError, match="11x11"):                          # the chroma planes of a 16 x 24 frame are 8 x 12
        Q.full_ref_yuv_native(dev[:, :24, :24].contiguous(), dev[:, :24, :24].contiguous(), name)


def _tiny_model():
    from real_esrgan_pytorch_amd.compact import SRVGGNetCompact
    torch.manual_seed(0)
    return SRVGGNetCompact(num_conv=2, upscale=4, precision="fast")


@pytest.mark.parametrize("pix_fmt,layout", [("yuv420p", "i420"), ("p010le", "p010")])
def test_inference_rawvideo_reference_lines(Q, tmp_path, capsys, monkeypatch, pix_fmt, layout):
    from real_esrgan_pytorch_amd import config, inference_rawvideo as V
    monkeypatch.setattr(config, "device", torch.device("cuda", 0))
    torch.save({"params": _tiny_model().state_dict()}, tmp_path / "w.pth")
    w, h, count = 24, 16, 3
    word = V.WORD[layout]
    rng = np.random.default_rng(3)
    top = 256 if word.itemsize == 1 else 65536
    (tmp_path / "in.yuv").write_bytes(rng.integers(0, top, (count, h * 3 // 2, w)).astype(word).tobytes())
    ref = rng.integers(0, top, (count + 1, 4 * h * 3 // 2, 4 * w)).astype(word)         # one frame more than the input: allowed
    (tmp_path / "ref.yuv").write_bytes(ref.tobytes())

    def args(**kw):
        base = dict(input=str(tmp_path / "in.yuv"), output=str(tmp_path / "out.yuv"), size=f"{w}x{h}", pix_fmt=pix_fmt, matrix="bt601", weights_path=str(tmp_path / "w.pth"),
                    model_type="compact", num_conv=2, act_type="prelu", precision="fast", depth=2, outscale=None, reference=str(tmp_path / "ref.yuv"))
        base.update(kw)
        return types.SimpleNamespace(**base)

    assert V.main(args()) == count
    lines = [l for l in capsys.readouterr().err.splitlines() if l.startswith(V.SCORE_LINE)]
    written = np.frombuffer((tmp_path / "out.yuv").read_bytes(), dtype=word).reshape(count, 4 * h * 3 // 2, 4 * w)
    want = torch.stack(Q.full_ref_yuv_native(torch.from_numpy(written.copy()).cuda(), torch.from_numpy(ref[:count]).cuda(), layout)).T.cpu().tolist()
    assert np.isfinite(want).all()
    assert lines == [f"{V.SCORE_LINE} {i}: " + " ".join(f"{v:.6f}" for v in row) for i, row in enumerate(want)] + \
        [f"{V.SCORE_LINE} mean: " + " ".join(f"{sum(r[i] for r in want) / count:.6f}" for i in range(7))]
    for line in lines:
        assert len(line.split(": ")[1].split()) == 7 and all(np.isfinite(float(t)) for t in line.split(": ")[1].split())
    # without the flag nothing of it is printed, and the video is the same
    first = (tmp_path / "out.yuv").read_bytes()
    assert V.main(args(reference=None)) == count and V.SCORE_LINE not in capsys.readouterr().err and (tmp_path / "out.yuv").read_bytes() == first
    # refused before any frame is computed, each with its cause
    (tmp_path / "short.yuv").write_bytes(ref[:count - 1].tobytes())
    with pytest.raises(ValueError, match="shorter than the input"):
        V.main(args(reference=str(tmp_path / "short.yuv")))
    (tmp_path / "small.yuv").write_bytes(ref[:, :-3, :].tobytes())            # frames of another height: not whole frames of the output
    with pytest.raises(ValueError, match="must have the output's size"):
        V.main(args(reference=str(tmp_path / "small.yuv")))
    with pytest.raises(ValueError, match="must have the output's size"):
        V.main(args(reference_size=f"{2 * w}x{2 * h}"))
    with pytest.raises(ValueError, match="one bit depth"):
        V.main(args(reference_pix_fmt="nv12" if word.itemsize == 2 else "p010le"))
    with pytest.raises(ValueError, match="rgb24 output"):
        V.main(args(out_pix_fmt="rgb24"))


def test_inference_frames_score_channels_rgb(Q, tmp_path, monkeypatch, capsys):
    from PIL import Image
    from real_esrgan_pytorch_amd import config, inference_frames
    monkeypatch.setattr(config, "device", torch.device("cuda", 0))
    torch.save({"params": _tiny_model().state_dict()}, tmp_path / "w.pth")
    rng = np.random.default_rng(8)
    names = ["0.png", "1.png"]
    for sub, (h, w) in (("lr", (16, 24)), ("gt", (64, 96))):
        (tmp_path / sub).mkdir()
        for name in names:
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(tmp_path / sub / name)

    def args(**kw):
        base = dict(inputs_dir=str(tmp_path / "lr"), output_dir=str(tmp_path / "sr"), weights_path=str(tmp_path / "w.pth"), depth=2, model_type="compact",
                    num_conv=2, act_type="prelu", precision="fast", reference_dir=str(tmp_path / "gt"), score_channels="rgb")
        base.update(kw)
        return types.SimpleNamespace(**base)

    def lines():
        return [l for l in capsys.readouterr().out.splitlines() if l.startswith("PSNR/SSIM ")]

    inference_frames.main(args())
    rgb = lines()
    want, want_y = [], []
    for name in names:
        sr, hr = (torch.from_numpy(np.array(Image.open(tmp_path / sub / name).convert("RGB")))[None].cuda() for sub in ("sr", "gt"))
        r = Q.full_ref_channels_native(sr, hr, config.upscale_factor)
        want.append([float(r.psnr_all), float(r.ssim_mean)])
        want_y.append([float(t) for t in Q.full_ref_native(sr, hr, config.upscale_factor)])
    expect = lambda rows: [f"PSNR/SSIM {name}: {p:.6f} {s:.6f}" for name, (p, s) in zip(names, rows)] + \
        [f"PSNR/SSIM mean: {sum(r[0] for r in rows) / 2:.6f} {sum(r[1] for r in rows) / 2:.6f}"]
    assert np.isfinite(want).all() and rgb == expect(want)
    for kw in ({"score_channels": "y"}, {"score_channels": None}):           # the default is today's output
        inference_frames.main(args(**kw))
        assert lines() == expect(want_y) != rgb
    with pytest.raises(ValueError, match="score_channels"):
        inference_frames.main(args(score_channels="yuv"))
