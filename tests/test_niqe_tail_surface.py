"""CPU: the host side of the native NIQE tail -- the declarations of resr_niqe_score and its size query, `config.niqe_tail`, the
`tail` keyword of `niqe_native` / `NativeNIQE`, what `niqe_score_native` refuses before it touches a device, and the numpy
restatement of tests/niqe_tail_ref.py against the module's torch tail."""
import importlib
import os
import random
import re

import numpy as np
import pytest
import torch

from tests import niqe_tail_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = os.path.join(ROOT, "tests", "golden", "niqe_model.mat")


@pytest.fixture(scope="module")
def Q():
    import __graft_entry__
    __graft_entry__.build()
    from real_esrgan_pytorch_amd import image_quality_assessment
    return image_quality_assessment


def test_header_declares_the_entries_and_the_size_query_needs_no_device(Q):
    from real_esrgan_pytorch_amd import _lib
    text = open(os.path.join(ROOT, "include", "resr.h")).read()
    for name in ("resr_niqe_score", "resr_niqe_score_workspace_bytes"):
        assert re.search(r"\b(int|size_t) %s\(" % name, text), name
        assert callable(getattr(_lib.lib(), name)) and name in _lib.exported_symbols()
    assert len(_lib._PROTOS["resr_niqe_score"][1]) == 4 and len(_lib._PROTOS["resr_niqe_score_workspace_bytes"][1]) == 1
    assert [f[0] for f in _lib.NiqeScoreDesc._fields_] == ["n", "blocks", "mu_prior", "cov_prior", "workspace", "workspace_bytes"]
    d = _lib.NiqeScoreDesc()
    d.n, d.blocks = 2, 5
    assert _lib.lib().resr_niqe_score_workspace_bytes(d) == 2 * (36 + 36 * 36 + 36 + 1) * 8       # mu_d | A | eigenvalues | kept count
    d.blocks = 0
    assert _lib.lib().resr_niqe_score_workspace_bytes(d) == 0 and b"niqe_score" in _lib.lib().resr_last_error()
    d.n, d.blocks = 0, 5
    assert _lib.lib().resr_niqe_score_workspace_bytes(d) == 0 and b"niqe_score" in _lib.lib().resr_last_error()
    d.n, d.blocks = 1, (2 ** 31 - 1) // 36 + 1
    assert _lib.lib().resr_niqe_score_workspace_bytes(d) == 0 and b"niqe_score" in _lib.lib().resr_last_error()


@pytest.fixture
def config(Q, monkeypatch):
    from real_esrgan_pytorch_amd import config as module
    state = (torch.get_rng_state(), random.getstate(), np.random.get_state())

    def reload(backend=None, tail=None):
        for name, value in (("RESR_NIQE", backend), ("RESR_NIQE_TAIL", tail)):
            monkeypatch.delenv(name, raising=False)
            if value is not None:
                monkeypatch.setenv(name, value)
        return importlib.reload(module)
    yield reload
    monkeypatch.undo()
    importlib.reload(module)
    torch.set_rng_state(state[0])
    random.setstate(state[1])
    np.random.set_state(state[2])


def test_tail_defaults_to_torch_and_refuses_as_specified(Q, config):
    c = config()
    assert c.niqe_tail == "torch" and c.niqe_backend == "torch"
    c = config("native")
    assert c.niqe_tail == "torch"
    c.niqe_model_path, c.device = MODEL, torch.device("cpu")
    m = c.build_niqe()
    assert type(m) is Q.NativeNIQE and m.tail == "torch"
    c = config("native", "native")
    assert c.niqe_tail == "native" and c.niqe_backend == "native"
    c.niqe_model_path, c.device = MODEL, torch.device("cpu")
    m = c.build_niqe()
    assert type(m) is Q.NativeNIQE and m.tail == "native"
    assert config("native", "torch").niqe_tail == "torch" and config("torch", "torch").niqe_tail == "torch"
    with pytest.raises(ValueError, match="RESR_NIQE_TAIL"):
        config("native", "hip")
    with pytest.raises(ValueError, match="RESR_NIQE_TAIL"):
        config("torch", "native")
    with pytest.raises(ValueError, match="RESR_NIQE_TAIL"):
        config(None, "native")
    with pytest.raises(ValueError, match="RESR_NIQE"):                      # RESR_NIQE keeps accepting exactly its two names
        config("hip", "torch")
    c = config()
    c.niqe_model_path, c.device, c.niqe_tail = MODEL, torch.device("cpu"), "native"
    with pytest.raises(ValueError, match="niqe_tail"):                      # set behind the import: nothing would honour it
        c.build_niqe()


def test_tail_keyword_and_what_is_refused_before_a_device_is_touched(Q):
    m = Q.NativeNIQE(0, MODEL)
    assert m.tail == "torch" and Q.NativeNIQE(0, MODEL, tail="native").tail == "native"
    with pytest.raises(ValueError, match="tail"):
        Q.NativeNIQE(0, MODEL, tail="hip")
    mu, cov = m.mu_prisparam, m.cov_prisparam
    with pytest.raises(ValueError, match="tail"):
        Q.niqe_native(torch.rand(1, 3, 128, 128), 0, mu, cov, tail="hip")
    with pytest.raises(ValueError, match="on the device"):
        Q.niqe_score_native(torch.zeros(2, 5, 36, dtype=torch.float64), mu, cov)
    with pytest.raises(RuntimeError, match="MI355X"):                       # the native tail has no CPU path either
        Q.NativeNIQE(0, MODEL, tail="native")(torch.rand(1, 3, 128, 128))
    from real_esrgan_pytorch_amd import inference_frames
    base = ["--inputs_dir", "a", "--output_dir", "b", "--weights_path", "c"]
    assert inference_frames.get_parser().parse_args(base).niqe_tail == "torch"
    assert inference_frames.get_parser().parse_args(base + ["--niqe", "--niqe_tail", "native"]).niqe_tail == "native"
    with pytest.raises(SystemExit):
        inference_frames.get_parser().parse_args(base + ["--niqe_tail", "hip"])


def test_reference_restates_the_torch_tail(Q):
    """tests/niqe_tail_ref on the CPU against `_score_from_features`: the stages it restates give the torch tail's score, with and
    without NaNs, and its 60-digit ground truth lies within the score bound of it."""
    m = Q.NIQE(0, MODEL)
    mu, cov = m.mu_prisparam.numpy(), m.cov_prisparam.numpy()
    assert np.array_equal(cov, cov.T)
    feats = T.synthetic_feats(mu, np.linalg.cholesky(cov), 2, 37, 0)
    feats[1, 3, 7] = np.nan
    want = Q._score_from_features(torch.from_numpy(feats), m.mu_prisparam, m.cov_prisparam).numpy()
    for i in range(2):
        s = T.stages_np(feats[i], mu, cov)
        assert s["m"] == 37 - i and np.array_equal(s["A"], s["A"].T)
        bound, cond, ev = T.score_bound(s["A"])
        assert ev.min() > 0 and cond < 5e5
        truth = T.truth_score(s["A"], s["diff"])
        assert T.relative_distance(want[i], truth) <= bound
    one = T.stages_np(feats[0, :1], mu, cov)
    assert one["m"] == 1 and np.isnan(one["A"]).all()
