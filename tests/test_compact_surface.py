"""CPU: the compact generator's module surface (upstream SRVGGNetCompact keys, shapes and init), its argument checks, the host
planning calls of resr_compact_* (no GPU needed) and the official-checkpoint loader."""
import ctypes as C

import pytest
import torch

from tests.compact_oracle import UpstreamCompact


@pytest.fixture(scope="module")
def R():
    import __graft_entry__
    __graft_entry__.build()
    import real_esrgan_pytorch_amd as R
    return R


@pytest.mark.parametrize("num_conv", [16, 32])
@pytest.mark.parametrize("act_type", ["prelu", "leakyrelu", "relu"])
@pytest.mark.parametrize("upscale", [1, 2, 3, 4])
def test_state_dict_matches_upstream(R, num_conv, act_type, upscale):
    torch.manual_seed(3)
    m = R.SRVGGNetCompact(3, 3, 64, num_conv, upscale, act_type, precision="strict")
    torch.manual_seed(3)
    u = UpstreamCompact(num_conv, upscale, act_type)
    a, b = m.state_dict(), u.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape, k
        assert torch.equal(a[k], b[k]), k        # same construction order: the same init under the same seed
    if act_type == "prelu":
        assert all(torch.all(a[f"body.{2 * k + 1}.weight"] == 0.25) for k in range(num_conv + 1))
    assert m.upscale_factor == upscale and m.pixel_unshuffle_factor == 1 and m.receptive_radius == num_conv + 2


def test_defaults_and_precision_rule(R, monkeypatch):
    monkeypatch.delenv("RESR_PRECISION", raising=False)
    m = R.SRVGGNetCompact()
    assert (m.num_conv, m.upscale, m.act_type, m.precision) == (16, 4, "prelu", "fast")
    monkeypatch.setenv("RESR_PRECISION", "exact16")
    assert R.SRVGGNetCompact().precision == "exact16"
    assert R.SRVGGNetCompact(precision="strict").precision == "strict"
    assert "SRVGGNetCompact" in R.__all__


@pytest.mark.parametrize("kw", [dict(act_type="gelu"), dict(upscale=5), dict(upscale=0), dict(num_feat=48), dict(num_in_ch=1),
                                dict(num_out_ch=4), dict(precision="bf16"), dict(num_conv=-1)])
def test_constructor_rejects_bad_arguments(R, kw):
    with pytest.raises(ValueError):
        R.SRVGGNetCompact(**kw)


def test_host_planning_calls_need_no_gpu(R):
    L = R._lib
    lib = L.lib()
    for num_conv, s, act, dtype in ((16, 4, L.COMPACT_PRELU, L.RESR_F16), (32, 3, L.COMPACT_LRELU, L.RESR_F16X2), (16, 1, L.COMPACT_RELU, L.RESR_F32)):
        d = L.CompactDesc(2, 37, 53, num_conv, s, act, dtype, 0)
        m = R.SRVGGNetCompact(3, 3, 64, num_conv, s, {0: "prelu", 1: "leakyrelu", 2: "relu"}[act])
        assert lib.resr_compact_param_count(C.byref(d)) == sum(p.numel() for p in m.parameters())
        n = lib.resr_compact_pack_table(C.byref(d), None, 0)
        assert n == 1 + 2 * num_conv + 2                       # conv 0: one chunk; every 64-input conv: two
        host = (L.PackChunk * n)()
        assert lib.resr_compact_pack_table(C.byref(d), C.cast(host, C.c_void_p), n) == n
        es = 4 if dtype == L.RESR_F32 else (6 if dtype == L.RESR_F16X2 else 2)
        last = host[n - 1]
        assert last.src_cout == 3 * s * s and last.mt == (1 if s <= 3 else 2)
        assert lib.resr_compact_packed_bytes(C.byref(d)) >= (last.dst_off + 9 * last.mt * 1024) * es
        px = 2 * 37 * 53
        pairs = 2 if dtype == L.RESR_F16X2 else 1
        act_es = 4 if dtype == L.RESR_F32 else 2
        assert lib.resr_compact_workspace_bytes(C.byref(d)) >= px * (32 + 64 + 64) * act_es * pairs + px * 3 * s * s * 4
    for bad in (L.CompactDesc(0, 8, 8, 16, 4, 0, 0, 0), L.CompactDesc(1, 8, 8, 16, 5, 0, 0, 0), L.CompactDesc(1, 8, 8, 16, 4, 3, 0, 0),
                L.CompactDesc(1, 8, 8, 16, 4, 0, 7, 0), L.CompactDesc(1, 8, 8, -1, 4, 0, 0, 0), L.CompactDesc(1, 8192, 4096, 16, 4, 0, L.RESR_F16X2, 0)):
        assert lib.resr_compact_param_count(C.byref(bad)) == 0
        assert lib.resr_compact_packed_bytes(C.byref(bad)) == 0
        assert lib.resr_compact_workspace_bytes(C.byref(bad)) == 0
        assert lib.resr_compact_pack_table(C.byref(bad), None, 0) < 0
    # exact16 takes at most 2^24 pixels per call (the pair kernels' addressing); fast mode routes such a frame to the one-role kernel
    big = dict(n=1, h=4096, w=4097, num_conv=16, upscale=4, act=0, reserved_=0)
    assert lib.resr_compact_workspace_bytes(C.byref(L.CompactDesc(dtype=L.RESR_F16X2, **big))) == 0
    assert lib.resr_compact_workspace_bytes(C.byref(L.CompactDesc(dtype=L.RESR_F16, **big))) > 0


_UPSTREAM = {"conv1": "conv_first", "conv2": "conv_body", "upsampling1.0": "conv_up1", "upsampling2.0": "conv_up2", "conv3.0": "conv_hr",
             "conv4": "conv_last"}


def _to_upstream(key):
    if key.startswith("trunk."):
        return "body." + key[len("trunk."):]
    head, _, leaf = key.rpartition(".")
    return _UPSTREAM[head] + "." + leaf


def test_rrdb_name_map_round_trips(R):
    torch.manual_seed(0)
    src = R.Generator(3, 3, 4, n_blocks=2)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    official = {_to_upstream(k): v for k, v in sd.items()}
    assert "conv_first.weight" in official and "body.1.rdb3.conv5.bias" in official and "conv_hr.weight" in official
    torch.manual_seed(1)
    dst = R.Generator(3, 3, 4, n_blocks=2)
    R.load_official_state_dict(dst, {"params_ema": official, "params": {k: v + 1 for k, v in official.items()}})
    for k, v in dst.state_dict().items():
        assert torch.equal(v, sd[k]), k                       # params_ema preferred over params
    R.load_official_state_dict(dst, {"params": official})
    R.load_official_state_dict(dst, official)                 # a bare state dict
    with pytest.raises(RuntimeError, match="conv_extra.weight"):
        R.load_official_state_dict(dst, {"params_ema": {**official, "conv_extra.weight": torch.zeros(1)}})
    missing = dict(official)
    del missing["conv_hr.bias"]
    with pytest.raises(RuntimeError, match="conv3.0.bias"):
        R.load_official_state_dict(dst, {"params_ema": missing})
    with pytest.raises(RuntimeError):                         # the reference's own names are not upstream's
        R.load_official_state_dict(dst, {"params": sd})


def test_compact_keys_pass_through(R):
    torch.manual_seed(0)
    u = UpstreamCompact(4, 2, "prelu")
    sd = {k: torch.randn_like(v) for k, v in u.state_dict().items()}
    m = R.SRVGGNetCompact(num_conv=4, upscale=2)
    m.load_official_state_dict({"params": sd})
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    with pytest.raises(RuntimeError, match="body.99.weight"):
        R.load_official_state_dict(m, {**sd, "body.99.weight": torch.zeros(1)})
