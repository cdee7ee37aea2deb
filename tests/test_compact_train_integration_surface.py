"""CPU: the layers between the compact generator's native passes and the train scripts -- `config.g_arch` / `build_generator`,
`SRVGGNetCompact.flat_parameter()` / `flat_grad()` / `grad_hook`, and what `DataParallel.attach` refuses before it touches a device."""
import importlib

import pytest
import torch
from torch import nn


@pytest.fixture(scope="module")
def R():
    import __graft_entry__
    __graft_entry__.build()
    import real_esrgan_pytorch_amd as R
    return R


_NAMES = ("RESR_G_ARCH", "RESR_COMPACT_NUM_CONV", "RESR_COMPACT_ACT", "RESR_PRETRAINED_G", "RESR_OUTPUT_PARITY", "RESR_PRECISION",
          "RESR_INFERENCE_PRECISION", "RESR_MODE")


@pytest.fixture
def config(R, monkeypatch):
    """`reload(**env)`: the config module re-imported under exactly these RESR_* names; the environment's own module state is put
    back afterwards (config.py seeds the generators at import: the RNG state is kept too)."""
    from real_esrgan_pytorch_amd import config as module
    import random

    import numpy as np
    state = (torch.get_rng_state(), random.getstate(), np.random.get_state())

    def reload(**env):
        for k in _NAMES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        return importlib.reload(module)
    yield reload
    monkeypatch.undo()
    importlib.reload(module)
    torch.set_rng_state(state[0])
    random.setstate(state[1])
    np.random.set_state(state[2])


def test_g_arch_defaults_to_rrdb(R, config):
    c = config()
    assert c.g_arch == "rrdb" and c.compact_num_conv == 16 and c.compact_act_type == "prelu" and c.pretrained_g == ""
    g = c.build_generator(True)
    assert type(g) is R.Generator and len(g.state_dict()) == 702 and g.precision == c.train_precision()
    assert c.generator_options() == {"precision": "fast"} and c.backward_options() == {"precision": "fast"}


def test_g_arch_compact_builds_the_trainable_compact_generator(R, config):
    c = config(RESR_G_ARCH="compact", RESR_COMPACT_NUM_CONV="3", RESR_COMPACT_ACT="leakyrelu", RESR_PRETRAINED_G="/some/where.pth")
    assert c.g_arch == "compact" and c.pretrained_g == "/some/where.pth"
    g = c.build_generator(True)
    assert type(g) is R.SRVGGNetCompact and g.trainable is True
    assert (g.num_conv, g.act_type, g.upscale) == (3, "leakyrelu", c.upscale_factor) and g.precision == c.train_precision() == "fast"
    t = c.build_generator(False)
    assert type(t) is R.SRVGGNetCompact and t.trainable is False and t.precision == c.inference_precision == "exact16"
    assert (t.num_conv, t.act_type) == (3, "leakyrelu")
    c = config(RESR_G_ARCH="compact", RESR_PRECISION="strict")
    g = c.build_generator(True)
    assert g.precision == "strict" and g.num_conv == 16 and g.act_type == "prelu" and g.trainable is True


def test_g_arch_refusals(config):
    with pytest.raises(ValueError, match="RESR_G_ARCH"):
        config(RESR_G_ARCH="vgg")
    with pytest.raises(ValueError, match="exact16"):
        config(RESR_G_ARCH="compact", RESR_OUTPUT_PARITY="1")
    c = config(RESR_G_ARCH="compact", RESR_PRECISION="exact16")          # no parity mode, but exact16 training: the constructor refuses
    with pytest.raises(ValueError, match="exact16"):
        c.build_generator(True)
    assert c.build_generator(False).precision == "exact16"


def test_flat_parameter_of_the_compact_generator(R):
    torch.manual_seed(0)
    m = R.SRVGGNetCompact(num_conv=2, upscale=4, precision="fast", trainable=True)
    assert m.grad_hook is None and m.flat_grad() is None
    keys, n_params = list(m.state_dict()), len(list(m.parameters()))
    fp = m.flat_parameter()
    assert isinstance(fp, nn.Parameter) and fp.is_leaf and fp.requires_grad and fp.dtype == torch.float32
    assert fp.data_ptr() == m.flat_parameters().data_ptr() and fp.numel() == sum(p.numel() for p in m.parameters())
    assert m.flat_parameter() is fp
    assert all(p is not fp for p in m.parameters()) and len(list(m.parameters())) == n_params
    assert list(m.state_dict()) == keys and "_flat_param" not in dict(m.named_parameters())
    assert m.flat_grad() is None
    # the arena is rebuilt, the alias follows it: the same object on the new memory
    old = fp.data_ptr()
    m.double().float()
    flat = m.flat_parameters()
    assert m.flat_parameter() is fp and fp.data_ptr() == flat.data_ptr() != old
    assert next(m.parameters()).data_ptr() == fp.data_ptr()
    # zero_grad clears the alias's gradient too; requires_grad_ reaches it
    fp.grad = torch.ones_like(fp)
    assert m.flat_grad() is fp.grad
    m.zero_grad(set_to_none=False)
    assert fp.grad is not None and not fp.grad.any()
    m.zero_grad()
    assert fp.grad is None and m.flat_grad() is None
    m.requires_grad_(False)
    assert not fp.requires_grad
    m.requires_grad_(True)
    assert fp.requires_grad


def test_flat_parameter_leaves_the_inference_guard_alone(R):
    m = R.SRVGGNetCompact(num_conv=1, precision="fast")
    fp = m.flat_parameter()                              # allowed: an optimiser may hold it
    assert fp.requires_grad and m.trainable is False
    with pytest.raises(RuntimeError, match="backward pass is not implemented"):
        m(torch.zeros(1, 3, 8, 8))                       # grad mode on, parameters require grad: refused before the device is looked at


def test_attach_refuses_what_has_no_backward_to_hook(R):
    from real_esrgan_pytorch_amd.train import DataParallel
    dp = DataParallel()
    assert not dp.active
    with pytest.raises(ValueError, match="trainable=False"):
        dp.attach(R.SRVGGNetCompact(num_conv=1, precision="fast"))
    with pytest.raises(TypeError, match="grad_hook"):
        dp.attach(nn.Conv2d(3, 3, 3))
    m = R.SRVGGNetCompact(num_conv=1, precision="fast", trainable=True)
    with pytest.warns(RuntimeWarning, match="gradient-ready"):
        import real_esrgan_pytorch_amd.train as T
        T._OVERLAP_WARNED = False
        dp.attach(m, overlap=True)
    assert dp.overlap is False and m.grad_hook == dp.all_reduce_mean_ and not hasattr(m, "grad_ready_hook")
