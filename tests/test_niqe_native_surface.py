"""CPU: the native NIQE's host side -- the numpy restatements of tests/niqe_ref.py against the module's torch path, the banded
half-size tables, the declarations of the entries, `config.niqe_backend`, and what `NativeNIQE` refuses before it touches a device."""
import importlib
import os
import random
import re

import numpy as np
import pytest
import torch

from tests import niqe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "niqe.npz"))
MODEL = os.path.join(ROOT, "tests", "golden", "niqe_model.mat")


@pytest.fixture(scope="module")
def Q():
    import __graft_entry__
    __graft_entry__.build()
    from real_esrgan_pytorch_amd import image_quality_assessment
    return image_quality_assessment


def _images():
    """uint8 [B,H,W,3]: the seed-0 random 41 x 43 pair of the kernel tests and the two golden images."""
    yield "random", np.random.default_rng(0).integers(0, 256, (2, 41, 43, 3), dtype=np.uint8)
    for i in (0, 1):
        yield f"golden{i}", np.ascontiguousarray(GOLDEN[f"img{i}"].transpose(0, 2, 3, 1))


def test_luma_definition_is_the_modules_luma_on_repaired_images(Q):
    from real_esrgan_pytorch_amd import imgproc
    for name, img in _images():
        before = R.tie_distance(R.unit_of_u8(img))
        fixed, nudged = R.repair_ties(img)
        x = R.unit_of_u8(fixed)
        assert R.tie_distance(x) >= R.TIE_MARGIN
        print(f"{name}: nearest tie {before:.2e} before the repair, {nudged} pixels nudged")
        got = R.niqe_luma_np(x, 0, *x.shape[2:])
        t = torch.from_numpy(x)
        module32 = (imgproc.rgb2ycbcr_torch(t, only_use_y_channel=True) * 255.0).round()[:, 0].numpy()       # what niqe() rounds
        module64 = (imgproc.rgb2ycbcr_torch(t.double(), only_use_y_channel=True) * 255.0).round()[:, 0].numpy()
        assert np.array_equal(got, module32) and np.array_equal(got, module64), name
        assert got.min() >= 16 and got.max() <= 235
    # the crop and the trim are an index shift
    x = R.unit_of_u8(next(_images())[1])
    assert np.array_equal(R.niqe_luma_np(x, 2, 32, 36), R.niqe_luma_np(x, 0, 41, 43)[:, 2:34, 2:38])


@pytest.mark.parametrize("n", [8, 12, 16, 36, 41, 96, 192, 201])
def test_banded_tables_are_the_rows_of_the_resize_matrix(Q, n):
    from real_esrgan_pytorch_amd import imgproc
    m = imgproc._resize_matrix(n, -(-n // 2), 0.5, True, np.float64)
    start, w = Q.half_band_table(n)
    assert start.dtype == np.int32 and w.dtype == np.float64 and w.shape[1] <= 16
    assert start.min() >= 0 and (start + w.shape[1]).max() <= n and np.all(np.diff(start) >= 0)
    dense = np.zeros_like(m)
    for k in range(w.shape[1]):
        dense[np.arange(len(start)), start + k] = w[:, k]
    assert np.array_equal(dense, m)                                         # the same bits, zeros included
    y = np.random.default_rng(n).integers(16, 236, (1, n, n)).astype(np.float64)
    ref, bound = R.half_np(y, m, m)
    assert np.all(np.abs(R.banded_apply(y, start, w, start, w) - ref) <= bound)
    assert bound.max() < 1e-11


def test_reference_moments_and_features_are_the_modules(Q):
    """tests/niqe_ref.reference restates _block_features: on a repaired image its features equal the torch path's within their own
    bounds, and the AGGD index is the module's."""
    img, _ = R.repair_ties(np.random.default_rng(0).integers(0, 256, (2, 41, 43, 3), dtype=np.uint8))
    levels = R.niqe_luma_np(R.unit_of_u8(img), 2, 32, 36)
    from real_esrgan_pytorch_amd import imgproc
    grid, r_gam = (t.numpy() for t in Q._aggd_grid(torch.zeros((), dtype=torch.float64)))
    win = Q._gaussian_window().double().numpy()
    ref = R.reference(levels, 16, 12, win, imgproc._resize_matrix(32, 16, 0.5, True, np.float64),
                      imgproc._resize_matrix(36, 18, 0.5, True, np.float64), grid, r_gam)
    assert ref["min_abs"] >= R.SIGN_MARGIN
    y = torch.from_numpy(levels.astype(np.float64))[:, None]
    for s in (1, 2):
        mu = torch.nn.functional.conv2d(torch.nn.functional.pad(y, (3, 3, 3, 3), mode="replicate"), torch.from_numpy(win).view(1, 1, 7, 7))
        sq = torch.nn.functional.conv2d(torch.nn.functional.pad(y * y, (3, 3, 3, 3), mode="replicate"), torch.from_numpy(win).view(1, 1, 7, 7))
        mscn = (y - mu) / (torch.sqrt((sq - mu * mu).abs() + 1e-8) + 1)
        bh, bw = 16 // s, 12 // s
        blocks = torch.nn.functional.unfold(mscn, (bh, bw), stride=(bh, bw)).transpose(1, 2).reshape(-1, 1, bh, bw)
        want = Q._block_features(blocks).reshape(2, -1, 18).numpy()
        r = ref[f"s{s}"]
        assert (r["gap"] > 1e-12).all()
        assert np.array_equal(want[..., R.ALPHA_COLUMNS], r["feats"][..., R.ALPHA_COLUMNS])
        assert np.all(np.abs(want - r["feats"]) <= r["feats_bound"]), float((np.abs(want - r["feats"]) - r["feats_bound"]).max())
        assert r["feats_bound"].max() < 1e-9
        if s == 1:
            y = Q._resize_half(y / 255.0) * 255.0


def test_header_declares_the_entries(Q):
    from real_esrgan_pytorch_amd import _lib
    text = open(os.path.join(ROOT, "include", "resr.h")).read()
    names = ["resr_niqe_luma_f32", "resr_niqe_luma_u8", "resr_niqe_features", "resr_niqe_workspace_bytes"]
    for name in names:
        assert re.search(r"\b(int|size_t) %s\(" % name, text), name
        assert callable(getattr(_lib.lib(), name))
    assert set(names) <= set(_lib.exported_symbols())
    assert len(_lib._PROTOS["resr_niqe_luma_f32"][1]) == 9 and len(_lib._PROTOS["resr_niqe_luma_u8"][1]) == 9
    assert len(_lib._PROTOS["resr_niqe_features"][1]) == 4
    fields = [f[0] for f in _lib.NiqeDesc._fields_]
    assert fields[:8] == ["n", "h", "w", "bh", "bw", "taps_h", "taps_w", "n_grid"] and fields[-3:] == ["workspace", "workspace_bytes", "win"]
    # the size query needs no device: the default block, and the layout the header states
    d = _lib.NiqeDesc()
    d.n, d.h, d.w, d.bh, d.bw = 2, 192, 96, 96, 96
    assert _lib.lib().resr_niqe_workspace_bytes(d) == 2 * 96 * 48 * 8 + 2 * (2 * 2) * 30 * 8
    d.bh = 95
    assert _lib.lib().resr_niqe_workspace_bytes(d) == 0 and b"niqe_features" in _lib.lib().resr_last_error()


@pytest.fixture
def config(Q, monkeypatch):
    from real_esrgan_pytorch_amd import config as module
    state = (torch.get_rng_state(), random.getstate(), np.random.get_state())

    def reload(value=None):
        monkeypatch.delenv("RESR_NIQE", raising=False)
        if value is not None:
            monkeypatch.setenv("RESR_NIQE", value)
        return importlib.reload(module)
    yield reload
    monkeypatch.undo()
    importlib.reload(module)
    torch.set_rng_state(state[0])
    random.setstate(state[1])
    np.random.set_state(state[2])


def test_backend_defaults_to_torch_and_refuses_other_names(Q, config):
    c = config()
    assert c.niqe_backend == "torch"
    c.niqe_model_path, c.device = MODEL, torch.device("cpu")
    assert type(c.build_niqe()) is Q.NIQE
    c = config("native")
    assert c.niqe_backend == "native"
    c.niqe_model_path, c.device = MODEL, torch.device("cpu")
    assert type(c.build_niqe()) is Q.NativeNIQE
    assert config("torch").niqe_backend == "torch"
    with pytest.raises(ValueError, match="RESR_NIQE"):
        config("hip")


def test_native_refuses_bad_blocks_and_cpu_tensors(Q):
    for bh, bw in ((95, 96), (96, 97), (0, 96), (134, 134), (1024, 1024), (2, 100000)):   # 134^2 * 8 + 140^2 + 1920 = 165,168 bytes
        with pytest.raises(ValueError, match="native NIQE"):
            Q.NativeNIQE(0, MODEL, bh, bw)
    Q.NativeNIQE(0, MODEL, 132, 132)                                         # 132^2 * 8 + 138^2 + 1920 = 160,356 of 163,840 bytes: fits
    m = Q.NativeNIQE(0, MODEL)
    assert isinstance(m, Q.NIQE) and (m.block_size_height, m.block_size_width) == (96, 96)
    with pytest.raises(RuntimeError, match="MI355X"):
        m(torch.rand(1, 3, 128, 128))
    with pytest.raises(RuntimeError, match="MI355X"):
        m(torch.zeros(1, 128, 128, 3, dtype=torch.uint8))
    mu, cov = m.mu_prisparam, m.cov_prisparam
    with pytest.raises(ValueError, match="at least one"):
        Q.niqe_native(torch.rand(1, 3, 64, 64), 0, mu, cov)
    with pytest.raises(ValueError, match="crop_border"):
        Q.niqe_native(torch.rand(1, 3, 128, 128), -1, mu, cov)
    # NIQE itself is untouched: the golden score, through the shared tail
    x = torch.from_numpy(GOLDEN["img0"]).float() / 255.0
    np.testing.assert_allclose(np.atleast_1d(Q.NIQE(int(GOLDEN["crop0"]), MODEL)(x).numpy()), GOLDEN["score0"], rtol=1e-6)


def test_niqe_flag_parses(Q):
    from real_esrgan_pytorch_amd import inference_frames
    base = ["--inputs_dir", "a", "--output_dir", "b", "--weights_path", "c"]
    args = inference_frames.get_parser().parse_args(base)
    assert args.niqe is False and args.niqe_model_path is None
    args = inference_frames.get_parser().parse_args(base + ["--niqe", "--niqe_model_path", MODEL])
    assert args.niqe is True and args.niqe_model_path == MODEL
