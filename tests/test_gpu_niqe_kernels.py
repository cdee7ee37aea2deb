"""-m gpu: every kernel of the native NIQE (csrc/niqe.hip) against its float64 restatement in tests/niqe_ref.py, element by element,
at the smallest shapes that can still go wrong:

    small    blocks 16 x 12 on a 2 x 3-block image of 41 x 43 with crop_border 2 (a trimmed remainder on both axes), batch 2
    default  blocks 96 x 96 on a 1 x 2-block image of 103 x 201 (remainders 7 and 9): the default block, 84 KB of LDS
    single   one 16 x 12 block: every replicate edge of the window and every reflected end of the half-size taps at once
    largest  one 132 x 132 block: the largest square block whose tile fits a CU's LDS (160,356 of 163,840 bytes)

The images are uniform random bytes, repaired on the CPU (niqe_ref.repair_ties) so that every fp32 order of the luma rounds alike.
Gates: the luma bit for bit niqe_luma_np, on these and on all 2^24 byte triples, unrepaired; the half-size image and the moments within niqe_ref's derived bounds (n 2^-53 sum|term| x 4,
propagated); the counts exact; alpha the reference's grid entry (one step away only where the reference's two best candidates lie
within 1e-12 of each other -- which no fit of these inputs shows, asserted); the other 17 features within the bounds derived from the
moments'; two calls the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gpu_util
from tests import niqe_ref as R

pytestmark = pytest.mark.gpu

CASES = {"small": ((2, 41, 43), 2, 16, 12), "default": ((1, 103, 201), 0, 96, 96), "single": ((1, 16, 12), 0, 16, 12),
         "largest": ((1, 132, 132), 0, 132, 132)}
IDS = [34100, 34200, 34201, 34300]


@pytest.fixture(scope="module")
def L():
    from real_esrgan_pytorch_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def Q():
    from real_esrgan_pytorch_amd import image_quality_assessment
    return image_quality_assessment


_CACHE = {}


def _case(Q, name):
    """The repaired image, its luma levels and the float64 reference of every stage, computed once per case and left unchanged."""
    if name not in _CACHE:
        from real_esrgan_pytorch_amd import imgproc
        (b, h, w), crop, bh, bw = CASES[name]
        img, _ = R.repair_ties(np.random.default_rng(0).integers(0, 256, (b, h, w, 3), dtype=np.uint8))
        lh, lw = (h - 2 * crop) // bh * bh, (w - 2 * crop) // bw * bw
        x = R.unit_of_u8(img)
        levels = R.niqe_luma_np(x, crop, lh, lw)
        grid, r_gam = (t.numpy() for t in Q._aggd_grid(torch.zeros((), dtype=torch.float64)))
        ref = R.reference(levels, bh, bw, Q._gaussian_window().double().numpy(), imgproc._resize_matrix(lh, lh // 2, 0.5, True, np.float64),
                          imgproc._resize_matrix(lw, lw // 2, 0.5, True, np.float64), grid, r_gam)
        _CACHE[name] = {"img": img, "x": x, "levels": levels, "ref": ref, "crop": crop, "bh": bh, "bw": bw}
    return _CACHE[name]


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


def _native(Q, c):
    """(features, half-size image, moments) of the case's levels as numpy, computed once per case."""
    if "native" not in c:
        out = Q.niqe_features_native(gpu_util.dev(c["levels"]), c["bh"], c["bw"], keep=True)
        torch.cuda.synchronize()
        c["native"] = tuple(t.cpu().numpy() for t in out)
    return c["native"]


@pytest.mark.parametrize("name", list(CASES))
def test_luma_is_the_definition_bit_for_bit(L, Q, name):
    c = _case(Q, name)
    b, lh, lw = c["levels"].shape
    _, h, w, _ = c["img"].shape
    for src, entry, want_id in ((gpu_util.dev(c["x"]), L.lib().resr_niqe_luma_f32, 34000), (gpu_util.dev(c["img"]), L.lib().resr_niqe_luma_u8, 34001)):
        out = gpu_util.Out(b * lh * lw, np.uint8)
        _, ids = _launch_ids(L, lambda: L.check(entry(L.ptr(src), C.c_void_p(out.ptr), b, h, w, c["crop"], lh, lw, L.stream_ptr()), "resr_niqe_luma"))
        assert ids == [want_id], ids
        got = out.read(written=False).reshape(b, lh, lw)                    # (0xA5 = 165 is a level: the guards are checked, not the body)
        assert np.array_equal(got, c["levels"]), (name, want_id, int((got != c["levels"]).sum()))
        again = Q.niqe_luma_native(src, c["crop"], lh, lw).cpu().numpy()    # the Python wrapper, the same bits
        assert np.array_equal(again, c["levels"])


def test_luma_of_every_byte_triple_is_the_definition(L, Q):
    """All 2^24 (r, g, b) byte triples as one 4096 x 4096 image, unrepaired: every near-tie a uint8 image can hold is in it (the
    nearest lies 4e-10 from a half), and the division of the uint8 entry meets every byte.  A chain with one contracted multiply-add
    misses 37 of them."""
    v = np.arange(1 << 24, dtype=np.uint32).reshape(1, 4096, 4096)
    img = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=-1).astype(np.uint8)
    x = R.unit_of_u8(img)
    want = R.niqe_luma_np(x, 0, 4096, 4096)
    assert want.min() == 16 and want.max() == 235
    from_u8 = Q.niqe_luma_native(gpu_util.dev(img), 0, 4096, 4096).cpu().numpy()
    from_f32 = Q.niqe_luma_native(gpu_util.dev(x), 0, 4096, 4096).cpu().numpy()
    assert np.array_equal(from_u8, want), int((from_u8 != want).sum())
    assert np.array_equal(from_f32, want), int((from_f32 != want).sum())


@pytest.mark.parametrize("name", list(CASES))
def test_half_size_image_and_moments_within_their_bounds(L, Q, name):
    c = _case(Q, name)
    ref = c["ref"]
    assert ref["min_abs"] >= R.SIGN_MARGIN, ref["min_abs"]                   # condition (b): no sign is summation noise
    _, half, mom = _native(Q, c)
    err = np.abs(half - ref["half"])
    print(f"{name}: half-size image worst error / bound {float((err / ref['half_bound']).max()):.3f} (bound up to {ref['half_bound'].max():.2e})")
    assert np.all(err <= ref["half_bound"])
    for s in (1, 2):
        r = ref[f"s{s}"]
        assert r["signed_margin"] > 0, r["signed_margin"]                    # no element's error bound reaches its magnitude: counts are exact
        got = mom[s - 1]
        assert np.array_equal(got[..., :2], r["mom"][..., :2]), (name, s, "counts")
        err = np.abs(got[..., 2:] - r["mom"][..., 2:])
        ratio = err / r["mom_bound"][..., 2:]
        print(f"{name}: scale {s} moments worst error / bound {float(ratio.max()):.3f} (relative bound up to {float((r['mom_bound'][..., 2:] / r['mom'][..., 2:]).max()):.2e})")
        assert np.all(err <= r["mom_bound"][..., 2:]), (name, s, float(ratio.max()))


@pytest.mark.parametrize("name", list(CASES))
def test_features_against_the_reference(L, Q, name):
    c = _case(Q, name)
    feats, _, _ = _native(Q, c)
    grid = Q._aggd_grid(torch.zeros((), dtype=torch.float64))[0].numpy()
    fits = near = 0
    for s in (1, 2):
        r = c["ref"][f"s{s}"]
        got = feats[..., 18 * (s - 1):18 * s]
        assert (r["gap"] > 1e-12).all()                                     # the reference alone shows no near-tie on these inputs
        got_alpha, want_alpha = got[..., R.ALPHA_COLUMNS], r["feats"][..., R.ALPHA_COLUMNS]
        differs = got_alpha != want_alpha
        for i in np.argwhere(differs):
            step = abs(int(np.argmin(np.abs(grid - got_alpha[tuple(i)]))) - int(r["idx"][tuple(i)]))
            assert step == 1 and r["gap"][tuple(i)] <= 1e-12, (name, s, tuple(i), got_alpha[tuple(i)], want_alpha[tuple(i)])
        fits += differs.size
        near += int(differs.sum())
        same = np.repeat(~differs, [2, 4, 4, 4, 4], axis=-1)               # the columns of a fit with another alpha are not comparable
        err = np.abs(got - r["feats"])
        ok = (err <= r["feats_bound"]) | ~same
        ratio = np.where(same & (r["feats_bound"] > 0), err / np.where(r["feats_bound"] > 0, r["feats_bound"], 1), 0)
        print(f"{name}: scale {s} features worst error / bound {float(ratio.max()):.3f} (relative bound up to "
              f"{float((r['feats_bound'] / np.abs(r['feats']).clip(1e-300)).max()):.2e})")
        assert ok.all(), (name, s, np.argwhere(~ok)[:4].tolist(), float(ratio.max()))
    assert near <= 0.01 * fits


def test_features_launch_under_their_ids_and_repeat_bit_for_bit(L, Q):
    c = _case(Q, "small")
    luma = gpu_util.dev(c["levels"])
    first, ids = _launch_ids(L, lambda: Q.niqe_features_native(luma, c["bh"], c["bw"], keep=True))
    assert ids == IDS, ids
    first = [t.cpu().numpy().copy() for t in first]
    second = Q.niqe_features_native(luma, c["bh"], c["bw"], keep=True)
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.int64), b.cpu().numpy().view(np.int64))
    for a, b in zip(first, _native(Q, c)):
        assert np.array_equal(a.view(np.int64), b.view(np.int64))


def test_refusals_follow_the_error_contract(L, Q):
    lib, st = L.lib(), L.stream_ptr()
    c = _case(Q, "single")
    x, img = gpu_util.dev(c["x"]), gpu_util.dev(c["img"])
    luma = torch.zeros(1, 16, 12, dtype=torch.uint8, device="cuda")
    for entry, src in ((lib.resr_niqe_luma_f32, x), (lib.resr_niqe_luma_u8, img)):
        for args in ((None, L.ptr(luma), 1, 16, 12, 0, 16, 12), (L.ptr(src), None, 1, 16, 12, 0, 16, 12), (L.ptr(src), L.ptr(luma), 0, 16, 12, 0, 16, 12),
                     (L.ptr(src), L.ptr(luma), 1, 16, 12, 1, 16, 12), (L.ptr(src), L.ptr(luma), 1, 16, 12, 0, 17, 12), (L.ptr(src), L.ptr(luma), 1, 16, 12, -1, 8, 8),
                     (L.ptr(src), L.ptr(luma), 1, 16, 12, 0, 0, 12)):
            rc = entry(*args, st)
            assert rc == L.RESR_ERR_ARG and b"niqe_luma" in lib.resr_last_error(), (args[2:], rc)
    t = Q._native_tables(16, 12, luma.device)
    feats = torch.zeros(1, 1, 36, dtype=torch.float64, device="cuda")
    ws = torch.zeros(4096, dtype=torch.float64, device="cuda")

    def desc(**change):
        d = L.NiqeDesc()
        d.n, d.h, d.w, d.bh, d.bw = 1, 16, 12, 16, 12
        d.taps_h, d.taps_w, d.n_grid = t["w_h"].shape[1], t["w_w"].shape[1], t["grid"].numel()
        for name in ("start_h", "w_h", "start_w", "w_w", "grid", "r_gam"):
            setattr(d, name, t[name].data_ptr())
        d.win[:] = t["win"]
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 8
        for k, v in change.items():
            setattr(d, k, v)
        return d
    need = int(lib.resr_niqe_workspace_bytes(desc()))
    assert need == 8 * 6 * 8 + 256 - (8 * 6 * 8) % 256 + 2 * 30 * 8
    for change, code in (({"bh": 15}, L.RESR_ERR_ARG), ({"bw": 8}, L.RESR_ERR_ARG), ({"n": 0}, L.RESR_ERR_ARG), ({"taps_h": 17}, L.RESR_ERR_ARG),
                         ({"taps_w": 0}, L.RESR_ERR_ARG), ({"taps_w": 13}, L.RESR_ERR_ARG), ({"n_grid": 0}, L.RESR_ERR_ARG), ({"grid": None}, L.RESR_ERR_ARG),
                         ({"workspace": None}, L.RESR_ERR_ARG), ({"workspace": ws.data_ptr() + 4}, L.RESR_ERR_ARG),
                         ({"workspace_bytes": need - 1}, L.RESR_ERR_WORKSPACE)):
        rc = lib.resr_niqe_features(C.byref(desc(**change)), L.ptr(luma), L.ptr(feats), st)
        assert rc == code and b"niqe_features" in lib.resr_last_error(), (change, rc)
    assert lib.resr_niqe_features(C.byref(desc()), None, L.ptr(feats), st) == L.RESR_ERR_ARG
    assert lib.resr_niqe_features(C.byref(desc()), L.ptr(luma), None, st) == L.RESR_ERR_ARG
    torch.cuda.synchronize()
    assert float(feats.abs().max()) == 0.0                                  # nothing was launched
    with pytest.raises(ValueError, match="whole number"):
        Q.niqe_features_native(torch.zeros(1, 17, 12, dtype=torch.uint8, device="cuda"), 16, 12)
    # the good call right behind the bad ones works
    got = Q.niqe_features_native(gpu_util.dev(c["levels"]), 16, 12).cpu().numpy()
    assert np.array_equal(got, _native(Q, c)[0])
