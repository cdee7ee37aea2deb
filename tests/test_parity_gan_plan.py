"""CPU: the output-parity GAN step -- exact16 forward, fast mode's f16 backward for the discriminator and ContentLoss, and the one
switch ($RESR_OUTPUT_PARITY) that puts the whole RealESRGAN step into that mode."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODES = ["features.2", "features.7", "features.16", "features.25", "features.34"]
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__
    __graft_entry__.build()
    import real_esrgan_pytorch_amd as R
    return R


def test_f16_backward_entry_point_declared_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "resr.h")).read()
    assert re.search(r"\bint resr_discriminator_backward_f16\s*\(", hdr)
    lib = ctypes.CDLL(built._lib.LIB_PATH)
    assert hasattr(lib, "resr_discriminator_backward_f16")
    assert "resr_discriminator_backward_f16" in built._lib.exported_symbols()
    assert lib.resr_version() == 3


def test_f16_backward_is_an_exact16_option(monkeypatch):
    import real_esrgan_pytorch_amd as R
    monkeypatch.delenv("RESR_X2_F16_BACKWARD", raising=False)
    assert R.Discriminator(precision="exact16", f16_backward=True).f16_backward
    assert R.ContentLoss(NODES, MEAN, STD, precision="exact16", f16_backward=True).f16_backward
    for precision in ("fast", "strict"):
        with pytest.raises(ValueError):
            R.Discriminator(precision=precision, f16_backward=True)
        with pytest.raises(ValueError):
            R.ContentLoss(NODES, MEAN, STD, precision=precision, f16_backward=True)
        assert not R.Discriminator(precision=precision, f16_backward=False).f16_backward
    assert not R.Discriminator(precision="exact16").f16_backward          # off by default
    assert not R.ContentLoss(NODES, MEAN, STD, precision="exact16").f16_backward


def test_env_default_reaches_exact16_modules_only(monkeypatch):
    import real_esrgan_pytorch_amd as R
    monkeypatch.setenv("RESR_X2_F16_BACKWARD", "1")
    assert R.Discriminator(precision="exact16").f16_backward
    assert R.ContentLoss(NODES, MEAN, STD, precision="exact16").f16_backward
    for precision in ("fast", "strict"):                                  # the env default is no error outside exact16: it does not apply
        assert not R.Discriminator(precision=precision).f16_backward
        assert not R.ContentLoss(NODES, MEAN, STD, precision=precision).f16_backward
    assert not R.Discriminator(precision="exact16", f16_backward=False).f16_backward   # an explicit argument wins
    monkeypatch.setenv("RESR_X2_F16_BACKWARD", "0")
    assert not R.Discriminator(precision="exact16").f16_backward


_PROBE = """
import json, sys
sys.path.insert(0, {root!r})
from real_esrgan_pytorch_amd import config, Discriminator, ContentLoss, Generator
g = Generator(3, 3, 4, n_blocks=1, **config.generator_options())
d = Discriminator(**config.backward_options())
c = ContentLoss(config.feature_model_extractor_nodes, config.feature_model_normalize_mean, config.feature_model_normalize_std,
                **config.backward_options())
print(json.dumps(dict(parity=config.output_parity, precision=config.train_precision(), g=[g.precision, g.x2_plan],
                      d=[d.precision, d.f16_backward], c=[c.precision, c.f16_backward, c.detached])))
"""


def _probe(env_extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("RESR_")}
    env.update(env_extra, RESR_MODE="train_realesrgan")
    r = subprocess.run([sys.executable, "-c", _PROBE.format(root=ROOT)], env=env, capture_output=True, text=True, timeout=300)
    return r


def test_output_parity_switch_configures_the_gan_step():
    r = _probe({"RESR_OUTPUT_PARITY": "1"})
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out == {"parity": True, "precision": "exact16", "g": ["exact16", 2401], "d": ["exact16", True],
                   "c": ["exact16", True, True]}
    r = _probe({})                                                        # off by default: fast, the generator's default plan
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["parity"] is False and out["precision"] == "fast" and out["d"] == ["fast", False] and out["c"][:2] == ["fast", False]
    r = _probe({"RESR_OUTPUT_PARITY": "1", "RESR_PRECISION": "fast"})    # a contradiction is an error, not a silent choice
    assert r.returncode != 0 and "RESR_OUTPUT_PARITY" in r.stderr
