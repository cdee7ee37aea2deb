"""-m gpu: the native NIQE tail (csrc/niqe.hip, resr_niqe_score) stage by stage against tests/niqe_tail_ref.py, and end to end.

Features are synthetic rows mu_prior + 1.3 L z + 0.1 (L the Cholesky factor of the golden prior, fixed seeds).  A = (P + C) / 2 with C
positive semi-definite, so every eigenvalue of A is at least half the prior's smallest (7.07e-6) and cond(A) stays below about 5e5: no
eigenvalue is near pinv's cut.  Both facts are asserted on the reference A before anything is gated.

Gates.  mu_d and every element of A within the first-order bounds of niqe_tail_ref (n 2^-53 sum|term| x 4); A exactly symmetric; the
eigenvalues, sorted, within 36 * 2^-52 * max|lambda| of numpy's eigvalsh of the reference A; the kept count; the score within
4 * 36 * 2^-53 * cond(A), relative, of a 60-digit LU solve (niqe_tail_ref.score_bound states where that comes from).  The measured
fraction of the bound is printed, and so is the torch tail's own distance from the ground truth, which is not gated.
Measured on an MI355X: DESIGN.md, "Native NIQE tail"."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from tests import niqe_ref as R
from tests import niqe_tail_ref as T

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "niqe.npz"))
MODEL = os.path.join(HERE, "golden", "niqe_model.mat")
# a divisor of one; fewer rows than columns (and than the 16 waves and 5 row groups that share a sum); several rows per wave; a fifth
# row for the first wave; a second LDS chunk of one row (the centred rows pass through LDS 112 at a time); three chunks, the last partial
BLOCKS = [2, 5, 37, 65, 113, 300]
# With two or five rows one draw in a few has a row far enough out to lift the largest eigenvalue of A, and cond(A) with it, past 5e5;
# these seeds are the first from the block count on whose three reference matrices stay below it (a property of the input alone, asserted).
SEEDS = {2: 4, 5: 7, 37: 37, 65: 65, 113: 113, 300: 300}
IDS = [34400, 34500]


@pytest.fixture(scope="module")
def L():
    from real_esrgan_pytorch_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def Q():
    from real_esrgan_pytorch_amd import image_quality_assessment
    return image_quality_assessment


@pytest.fixture(scope="module")
def prior():
    import scipy.io
    model = scipy.io.loadmat(MODEL)
    mu, cov = np.ravel(model["mu_prisparam"]).astype(np.float64), np.asarray(model["cov_prisparam"], dtype=np.float64)
    assert np.array_equal(cov, cov.T)
    return {"mu": mu, "cov": cov, "chol": np.linalg.cholesky(cov), "min_eig": float(np.linalg.eigvalsh(cov).min()),
            "mu_dev": torch.from_numpy(mu).cuda(), "cov_dev": torch.from_numpy(cov).cuda()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _run(Q, prior, feats, cov=None):
    """The entry on float64 [B, blocks, 36] numpy features -> (scores [B], mu_d, A, eigenvalues, kept) as numpy."""
    cov_dev = prior["cov_dev"] if cov is None else torch.from_numpy(cov).cuda()
    out = Q.niqe_score_native(torch.from_numpy(feats).cuda(), prior["mu_dev"], cov_dev, keep=True)
    torch.cuda.synchronize()
    return tuple(np.atleast_1d(t.cpu().numpy()) for t in out)


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


def _check_reference(prior, s, a=None):
    """The two facts of the module docstring, on the reference A (or its non-zero block `a`); eigvalsh's own error, 36 eps ||A||, is
    allowed on the first.  -> (score bound, cond, eigenvalues)."""
    bound, cond, ev = T.score_bound(s["A"] if a is None else a)
    assert ev.min() >= 0.5 * prior["min_eig"] - T.F * T.EPS * ev.max(), (ev.min(), prior["min_eig"])
    assert cond < 5e5, cond
    return bound, cond, ev


def _gate_image(prior, s, got, i, label, cov=None):
    """Stages and score of image i of a call's outputs against the reference dict s of that image."""
    scores, mu_d, a, eig, kept = got
    bound, cond, ev = _check_reference(prior, s)
    assert (np.abs(mu_d[i] - s["mu_d"]) <= s["mu_bound"]).all(), (label, "mu_d", float((np.abs(mu_d[i] - s["mu_d"]) / s["mu_bound"]).max()))
    ratio = np.abs(a[i] - s["A"]) / s["A_bound"]
    assert (ratio <= 1).all(), (label, "A", float(ratio.max()))
    assert np.array_equal(_bits(a[i]), _bits(a[i].T)), (label, "A is not exactly symmetric")
    eig_err = float(np.abs(np.sort(eig[i]) - ev).max() / (T.F * T.EPS * np.abs(ev).max()))
    assert eig_err <= 1, (label, "eigenvalues", eig_err)
    assert kept[i] == 36, (label, kept[i])
    truth = T.truth_score(s["A"], s["diff"])
    rel = T.relative_distance(scores[i], truth)
    print(f"{label}: cond(A) {cond:.3e}, A at {float(ratio.max()):.3f} of its bound, eigenvalues at {eig_err:.3f} of theirs, "
          f"score {scores[i]:.15g} at {rel / bound:.3e} of its bound ({rel:.3e} of {bound:.3e})")
    assert np.isfinite(scores[i]) and rel <= bound, (label, "score", rel, bound)
    return truth, bound


_CASES = {}


def _case(Q, prior, blocks):
    """Per block count: a batch of 3, its reference stages and the entry's outputs, computed once and left unchanged."""
    if blocks not in _CASES:
        feats = T.synthetic_feats(prior["mu"], prior["chol"], 3, blocks, SEEDS[blocks])
        _CASES[blocks] = {"feats": feats, "ref": [T.stages_np(feats[i], prior["mu"], prior["cov"]) for i in range(3)], "got": _run(Q, prior, feats)}
    return _CASES[blocks]


@pytest.mark.parametrize("blocks", BLOCKS)
def test_stages_and_score_element_by_element(Q, prior, blocks):
    c = _case(Q, prior, blocks)
    assert c["got"][0].shape == (3,)
    for i in range(3):
        _gate_image(prior, c["ref"][i], c["got"], i, f"blocks={blocks} image {i}")
    # reported, not gated: the torch tail on the same features, on the device
    torch_tail = Q._score_from_features(torch.from_numpy(c["feats"]).cuda(), prior["mu_dev"], prior["cov_dev"]).cpu().numpy()
    for i in range(3):
        s = c["ref"][i]
        rel = T.relative_distance(torch_tail[i], T.truth_score(s["A"], s["diff"]))
        print(f"blocks={blocks} image {i}: the torch tail lies {rel:.3e} (relative) from the ground truth, {rel / T.score_bound(s['A'])[0]:.3e} of the bound")


def test_nan_semantics(Q, prior):
    """37 blocks.  Image 1: one NaN entry (the mean drops the entry, the covariance the row); image 2: a column of NaNs; image 3: a NaN
    in every row but one; images 0 and 4 clean -- and the same bits as in a call without the poisoned images."""
    clean = T.synthetic_feats(prior["mu"], prior["chol"], 5, 37, 1000)
    feats = clean.copy()
    feats[1, 11, 20] = np.nan
    feats[2, :, 5] = np.nan
    feats[3, np.arange(37) != 9, np.arange(37)[np.arange(37) != 9] % 36] = np.nan
    got = _run(Q, prior, feats)
    scores, mu_d, a, eig, kept = got
    s = T.stages_np(feats[1], prior["mu"], prior["cov"])
    assert s["m"] == 36 and np.isfinite(s["mu_d"]).all()
    _gate_image(prior, s, got, 1, "one NaN entry")
    full = T.stages_np(clean[1], prior["mu"], prior["cov"])               # (the gates can tell the two apart)
    assert np.abs(full["mu_d"][20] - s["mu_d"][20]) > 100 * s["mu_bound"][20] and (np.abs(full["A"] - s["A"]) > 100 * s["A_bound"]).any()
    assert np.isnan(scores[2]) and np.isnan(mu_d[2, 5]) and np.isfinite(np.delete(mu_d[2], 5)).all()
    assert np.isnan(scores[3]) and np.isfinite(mu_d[3]).all() and np.isnan(a[3]).all() and kept[3] == 0 and np.isnan(eig[3]).all()
    for i in (0, 4):
        _gate_image(prior, T.stages_np(feats[i], prior["mu"], prior["cov"]), got, i, f"clean image {i} beside the poisoned ones")
    alone = _run(Q, prior, np.ascontiguousarray(feats[[0, 4]]))
    for k, i in enumerate((0, 4)):
        for x, y in zip(got, alone):
            assert np.array_equal(_bits(x[i]), _bits(y[k]))
    single = _run(Q, prior, np.ascontiguousarray(clean[:2, :1]))            # blocks = 1: 0 / 0
    assert np.isnan(single[0]).all() and np.isfinite(single[1]).all() and np.isnan(single[2]).all()
    no_ok = feats[3:4].copy()
    no_ok[0, 9, 0] = np.nan                                                  # no row left: the torch tail's -0, and its score
    want = Q._score_from_features(torch.from_numpy(no_ok).cuda(), prior["mu_dev"], prior["cov_dev"]).cpu().numpy()
    got0 = _run(Q, prior, no_ok)
    assert np.array_equal(_bits(got0[2][0]), _bits(prior["cov"] / 2)) and np.isnan(want) == np.isnan(got0[0][0])
    if np.isfinite(want):
        s0 = T.stages_np(no_ok[0], prior["mu"], prior["cov"])
        assert T.relative_distance(got0[0][0], T.truth_score(prior["cov"] / 2, s0["diff"])) <= T.score_bound(prior["cov"] / 2)[0]


def test_the_cut_drops_an_exactly_zero_block(Q, prior):
    """8 blocks, a prior whose last 6 rows and columns are exactly 0, features that are one constant per column there (multiples of
    1/4, so that their sums are exact in every order): the mean is exact, A has an exactly zero block and diff is non-zero in it."""
    cov = prior["cov"].copy()
    cov[30:, :] = 0.0
    cov[:, 30:] = 0.0
    feats = T.synthetic_feats(prior["mu"], prior["chol"], 2, 8, 77)
    feats[:, :, 30:] = 0.25 * np.arange(1, 7)
    scores, mu_d, a, eig, kept = _run(Q, prior, feats, cov)
    for i in range(2):
        s = T.stages_np(feats[i], prior["mu"], cov)
        assert not s["A"][30:, :].any() and not s["A"][:, 30:].any() and (s["diff"][30:] != 0).all()
        block = s["A"][:30, :30]
        bound, cond, ev = _check_reference(prior, s, block)
        assert not a[i][30:, :].any() and not a[i][:, 30:].any() and np.array_equal(mu_d[i][30:], 0.25 * np.arange(1, 7))
        assert (np.abs(a[i] - s["A"]) <= s["A_bound"]).all()
        assert kept[i] == 30 and (np.sort(np.abs(eig[i]))[:6] == 0).all()
        rel = T.relative_distance(scores[i], T.truth_score(s["A"], s["diff"], keep=range(30)))
        print(f"cut, image {i}: cond of the 30 x 30 block {cond:.3e}, score {scores[i]:.15g} at {rel / bound:.3e} of its bound")
        assert np.isfinite(scores[i]) and rel <= bound


def test_same_bits_again_on_a_side_stream_and_two_launches_whatever_the_batch(L, Q, prior):
    c = _case(Q, prior, 65)
    again = _run(Q, prior, c["feats"])
    for x, y in zip(c["got"], again):
        assert np.array_equal(_bits(x), _bits(y))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    src = torch.from_numpy(c["feats"]).cuda()
    with torch.cuda.stream(side):
        feats = torch.zeros_like(src)
        m = torch.full((2048, 2048), 1.0 / 2048, device="cuda")
        for _ in range(50):
            m = m @ m
        feats.copy_(src)                                                    # the features appear late, on this stream only
        got = Q.niqe_score_native(feats, prior["mu_dev"], prior["cov_dev"])
    side.synchronize()
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(c["got"][0]))
    for b in (1, 3):
        f = torch.from_numpy(c["feats"][:b]).cuda()
        out, ids = _launch_ids(L, lambda: Q.niqe_score_native(f, prior["mu_dev"], prior["cov_dev"]))
        assert ids == IDS, (b, ids)
        assert out.shape == (() if b == 1 else (3,))                        # squeezed as _score_from_features squeezes
        assert np.array_equal(_bits(np.atleast_1d(out.cpu().numpy())), _bits(c["got"][0][:b]))


def test_refusals_follow_the_error_contract(L, Q, prior):
    lib, st = L.lib(), L.stream_ptr()
    feats = torch.from_numpy(T.synthetic_feats(prior["mu"], prior["chol"], 2, 5, 5)).cuda()
    scores = torch.zeros(2, dtype=torch.float64, device="cuda")
    ws = torch.zeros(2 * 1369 + 8, dtype=torch.float64, device="cuda")

    def desc(**change):
        d = L.NiqeScoreDesc()
        d.n, d.blocks, d.mu_prior, d.cov_prior = 2, 5, prior["mu_dev"].data_ptr(), prior["cov_dev"].data_ptr()
        d.workspace, d.workspace_bytes = ws.data_ptr(), 2 * 1369 * 8
        for k, v in change.items():
            setattr(d, k, v)
        return d
    assert int(lib.resr_niqe_score_workspace_bytes(desc())) == 2 * 1369 * 8

    def refused():
        for change in ({"n": 0}, {"n": -1}, {"blocks": 0}, {"blocks": (2 ** 31 - 1) // 36 + 1}, {"mu_prior": None}, {"cov_prior": None}, {"workspace": None},
                       {"workspace_bytes": 2 * 1369 * 8 - 1}, {"workspace": ws.data_ptr() + 4}):
            rc = lib.resr_niqe_score(C.byref(desc(**change)), L.ptr(feats), L.ptr(scores), st)
            assert rc == L.RESR_ERR_ARG and b"niqe_score" in lib.resr_last_error(), (change, rc)
        for args in ((None, L.ptr(feats), L.ptr(scores)), (C.byref(desc()), None, L.ptr(scores)), (C.byref(desc()), L.ptr(feats), None)):
            assert lib.resr_niqe_score(*args, st) == L.RESR_ERR_ARG and b"niqe_score" in lib.resr_last_error()
    _, ids = _launch_ids(L, refused)
    assert ids == []                                                        # nothing was launched
    assert float(scores.abs().max()) == 0.0 and float(ws.abs().max()) == 0.0
    for bad in (feats.float(), feats[:, :, :35], feats[0], feats[:, :0]):
        with pytest.raises(ValueError, match="niqe_score_native"):
            Q.niqe_score_native(bad, prior["mu_dev"], prior["cov_dev"])
    with pytest.raises(ValueError, match="priors"):
        Q.niqe_score_native(feats, prior["mu_dev"][:35], prior["cov_dev"])
    # the good call right behind the bad ones works
    assert lib.resr_niqe_score(C.byref(desc()), L.ptr(feats), L.ptr(scores), st) == L.RESR_OK
    torch.cuda.synchronize()
    assert np.array_equal(_bits(scores.cpu().numpy()), _bits(Q.niqe_score_native(feats, prior["mu_dev"], prior["cov_dev"]).cpu().numpy()))


def _score(t):
    return np.atleast_1d(t.detach().double().cpu().numpy())


@pytest.mark.parametrize("i", [0, 1])
def test_end_to_end_on_the_repaired_golden_images(Q, i):
    """`niqe_native(..., tail="native")` against `niqe_native(...)` of the same process -- the features are the same bits, only the tail
    differs: gated with the score bound, cond(A) from the reference A of those very features -- and against `niqe()` with the
    tolerance tests/test_gpu_niqe_native.py measures for that comparison: 10 x |niqe() on the CPU - niqe() on the GPU|, floor 1e-12."""
    img, _ = R.repair_ties(np.ascontiguousarray(GOLDEN[f"img{i}"].transpose(0, 2, 3, 1)))
    crop = int(GOLDEN[f"crop{i}"])
    x = torch.from_numpy(R.unit_of_u8(img))
    plain = Q.NIQE(crop, MODEL)
    cpu, gpu = _score(plain(x)), _score(plain.cuda()(x.cuda()))
    tol = max(10 * float(np.abs(cpu - gpu).max()), 1e-12)
    torch_tail, native_tail = Q.NativeNIQE(crop, MODEL).cuda(), Q.NativeNIQE(crop, MODEL, tail="native").cuda()
    frame = torch.from_numpy(img).cuda()
    want, got, from_u8 = _score(torch_tail(x.cuda())), _score(native_tail(x.cuda())), _score(native_tail(frame))
    assert got.shape == want.shape == cpu.shape and np.isfinite(got).all()
    assert np.array_equal(_bits(got), _bits(from_u8))                       # float and uint8 input: the same bits
    assert len(native_tail._tail_priors) == 1                               # the priors were made once for both calls
    mu, cov = (p.float().double() for p in (native_tail.mu_prisparam, native_tail.cov_prisparam))
    assert np.array_equal(_bits(_score(Q.niqe_native(frame, crop, mu, cov, tail="native"))), _bits(got))
    b, h, w = img.shape[:3]
    feats = Q.niqe_features_native(Q.niqe_luma_native(frame, crop, (h - 2 * crop) // 96 * 96, (w - 2 * crop) // 96 * 96)).cpu().numpy()
    for k in range(b):
        s = T.stages_np(feats[k], mu.cpu().numpy(), cov.cpu().numpy())
        bound, cond, _ = T.score_bound(s["A"])
        rel = abs(got[k] - want[k]) / abs(want[k])
        truth = T.truth_score(s["A"], s["diff"])
        print(f"golden{i} image {k}: {feats.shape[1]} blocks, cond(A) {cond:.3e}; native tail {got[k]:.15g}, torch tail {want[k]:.15g}: relative difference "
              f"{rel:.3e} of a bound of {bound:.3e}; from the ground truth: native {T.relative_distance(got[k], truth):.3e}, torch "
              f"{T.relative_distance(want[k], truth):.3e}; |native - niqe() CPU| {abs(got[k] - cpu[k]):.3e}, GPU {abs(got[k] - gpu[k]):.3e}, tolerance {tol:.3e}")
        assert rel <= bound
    assert np.abs(got - cpu).max() <= tol and np.abs(got - gpu).max() <= tol


def test_inference_frames_with_the_native_tail_prints_one_score_per_frame_in_input_order(Q, tmp_path, monkeypatch, capsys):
    from PIL import Image
    from real_esrgan_pytorch_amd import config, inference_frames
    from real_esrgan_pytorch_amd.compact import SRVGGNetCompact
    from tests.test_gpu_train_harness import _smooth_png
    monkeypatch.setattr(config, "device", torch.device("cuda", 0))
    torch.manual_seed(0)
    torch.save({"params": SRVGGNetCompact(num_conv=4, upscale=4).state_dict()}, tmp_path / "w.pth")
    (tmp_path / "lr").mkdir()
    names = ["a.png", "b.png", "c.png"]
    for k, name in enumerate(names):
        _smooth_png(str(tmp_path / "lr" / name), 56, 11 + k)
    inference_frames.main(types.SimpleNamespace(inputs_dir=str(tmp_path / "lr"), output_dir=str(tmp_path / "sr"), weights_path=str(tmp_path / "w.pth"),
                                                depth=2, model_type="compact", num_conv=4, act_type="prelu", precision="fast", niqe=True,
                                                niqe_model_path=MODEL, niqe_tail="native"))
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("NIQE ")]
    m = Q.NativeNIQE(config.upscale_factor, MODEL, tail="native").cuda()
    want = [float(m(torch.from_numpy(np.asarray(Image.open(tmp_path / "sr" / name)))[None].cuda())) for name in names]
    assert np.isfinite(want).all() and len(set(want)) == 3
    assert lines == [f"NIQE {name}: {v:.6f}" for name, v in zip(names, want)] + [f"NIQE mean: {sum(want) / len(want):.6f}"]
