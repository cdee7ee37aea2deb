"""CPU: the training surface of the compact generator -- the host planning calls of resr_compact_train_* (no GPU needed), the
`trainable` keyword of SRVGGNetCompact, and the CPU evaluators of tests/compact_grad_ref.py against each other (the f16 emulation that
gates fast mode on the GPU gets a check of its own here)."""
import ctypes as C

import pytest
import torch

from tests import compact_grad_ref as G


@pytest.fixture(scope="module")
def R():
    import __graft_entry__
    __graft_entry__.build()
    import real_esrgan_pytorch_amd as R
    return R


def _table(L, call, d):
    n = call(C.byref(d), None, 0)
    assert n > 0
    host = (L.PackChunk * n)()
    assert call(C.byref(d), C.cast(host, C.c_void_p), n) == n
    return list(host)


_FIELDS = ("src_off", "dst_off", "src_cout", "src_cin", "m_off", "m_count", "k_off", "k_count", "mt", "transposed", "scale", "virtual4x4")


def test_host_planning_calls_need_no_gpu(R):
    L = R._lib
    lib = L.lib()
    px = 2 * 37 * 53
    for num_conv, s, act, dtype in ((16, 4, L.COMPACT_PRELU, L.RESR_F16), (32, 3, L.COMPACT_LRELU, L.RESR_F32), (2, 1, L.COMPACT_RELU, L.RESR_F16)):
        d = L.CompactDesc(2, 37, 53, num_conv, s, act, dtype, 0)
        fwd = _table(L, lib.resr_compact_pack_table, d)
        both = _table(L, lib.resr_compact_train_pack_table, d)
        # the forward table, chunk for chunk ...
        for a, b in zip(fwd, both):
            assert all(getattr(a, f) == getattr(b, f) for f in _FIELDS)
        # ... followed by the transposed chunks of as many convolutions, in the same order (the packed format gives a transposed
        # convolution K / 32 = cout_pad / 32 chunks: conv 0 two for its one forward chunk, the last conv one or two)
        bwd = both[len(fwd):]
        assert bwd and all(c.transposed == 1 and c.scale == 1.0 for c in bwd) and all(c.transposed == 0 for c in fwd)
        order = lambda t: list(dict.fromkeys((c.src_off, c.src_cout, c.src_cin) for c in t))
        assert order(bwd) == order(fwd) and len(order(fwd)) == num_conv + 2
        cpl = (3 * s * s + 31) // 32 * 32
        assert len(bwd) == 2 + 2 * num_conv + cpl // 32
        assert [c.dst_off for c in both] == sorted(c.dst_off for c in both) and len({c.dst_off for c in both}) == len(both)
        es = 4 if dtype == L.RESR_F32 else 2
        last = both[-1]
        assert lib.resr_compact_train_packed_bytes(C.byref(d)) >= (last.dst_off + 9 * last.mt * 1024) * es
        assert lib.resr_compact_train_packed_bytes(C.byref(d)) > lib.resr_compact_packed_bytes(C.byref(d))
        ws = lib.resr_compact_train_workspace_bytes(C.byref(d))
        assert ws >= px * (32 + 2 * 64 * (num_conv + 1) + 2 * 64 + cpl) * es
        more = L.CompactDesc(2, 37, 53, num_conv + 1, s, act, dtype, 0)
        assert lib.resr_compact_train_workspace_bytes(C.byref(more)) >= ws + 2 * px * 64 * es     # z and a of one more layer
        assert 0 < lib.resr_compact_train_state_bytes(C.byref(d)) < ws
    for bad in (L.CompactDesc(0, 8, 8, 16, 4, 0, 0, 0), L.CompactDesc(1, 8, 8, 16, 5, 0, 0, 0), L.CompactDesc(1, 8, 8, 16, 4, 3, 0, 0),
                L.CompactDesc(1, 8, 8, 16, 4, 0, 7, 0), L.CompactDesc(1, 8, 8, -1, 4, 0, 0, 0),
                L.CompactDesc(2, 37, 53, 16, 4, 0, L.RESR_F16X2, 0)):                             # exact16 training is not built
        assert lib.resr_compact_train_packed_bytes(C.byref(bad)) == 0
        assert lib.resr_compact_train_workspace_bytes(C.byref(bad)) == 0
        assert lib.resr_compact_train_state_bytes(C.byref(bad)) == 0
        assert lib.resr_compact_train_pack_table(C.byref(bad), None, 0) < 0
    for name in ("resr_compact_forward_train", "resr_compact_backward", "resr_debug_compact_act", "resr_debug_compact_act_bwd",
                 "resr_debug_compact_residual_bwd"):
        assert name in L.exported_symbols(), name


def test_train_offsets_describe_the_documented_workspace(R):
    """resr_debug_compact_train_offsets (host only): the buffers in the order include/resr_debug.h documents, each 256-byte aligned, each
    at least as large as include/resr.h ("Compact generator: training", Workspace) says, the last one inside the workspace."""
    L = R._lib
    lib = L.lib()
    count = L.RESR_DEBUG_COMPACT_TRAIN_OFFSETS
    assert count == 10 and "resr_debug_compact_train_offsets" in L.exported_symbols()
    n, h, w = 2, 9, 11
    px = n * h * w
    for s in (1, 2, 3, 4):
        for dtype, es in ((L.RESR_F16, 2), (L.RESR_F32, 4)):
            for num_conv, act in ((0, L.COMPACT_PRELU), (1, L.COMPACT_LRELU), (3, L.COMPACT_RELU)):
                d = L.CompactDesc(n, h, w, num_conv, s, act, dtype, 0)
                out = (C.c_int64 * (count + 1))(*([-7] * (count + 1)))
                assert lib.resr_debug_compact_train_offsets(C.byref(d), out, count) == count
                assert out[count] == -7
                slot, xin, z0, a0, stride, t, gt, g0, g1, gxin = list(out)[:count]
                assert all(v % 256 == 0 for v in out[:count])
                assert slot == 0 and slot < xin < z0 < a0 < t < gt < g0 < g1 < gxin                       # the documented order
                layers, cpl = num_conv + 1, (3 * s * s + 31) // 32 * 32
                assert xin - slot >= lib.resr_compact_train_state_bytes(C.byref(d)) == 256
                assert z0 - xin >= px * 32 * es
                assert stride >= px * 64 * es and a0 - z0 >= layers * stride and t - a0 >= layers * stride    # z_k, a_k: k = 0 .. num_conv
                assert gt - t >= px * 3 * s * s * 4
                assert g0 - gt >= px * cpl * es
                assert g1 - g0 >= px * 64 * es and gxin - g1 >= px * 64 * es
                assert gxin + px * 32 * es <= lib.resr_compact_train_workspace_bytes(C.byref(d))
                assert lib.resr_debug_compact_train_offsets(C.byref(d), out, count - 1) == L.RESR_ERR_ARG     # too small a capacity
                assert lib.resr_debug_compact_train_offsets(C.byref(d), None, count) == L.RESR_ERR_ARG
    out = (C.c_int64 * count)()
    for bad in (L.CompactDesc(n, h, w, 1, 2, 0, L.RESR_F16X2, 0), L.CompactDesc(n, h, w, 1, 5, 0, L.RESR_F16, 0), L.CompactDesc(0, h, w, 1, 2, 0, L.RESR_F16, 0),
                L.CompactDesc(n, h, w, -1, 2, 0, L.RESR_F32, 0)):                                          # what the training entries refuse
        assert lib.resr_debug_compact_train_offsets(C.byref(bad), out, count) == L.RESR_ERR_ARG
    assert lib.resr_debug_compact_train_offsets(None, out, count) == L.RESR_ERR_ARG


def test_trainable_keyword(R, monkeypatch):
    monkeypatch.delenv("RESR_PRECISION", raising=False)
    assert R.SRVGGNetCompact(num_conv=2).trainable is False
    assert R.SRVGGNetCompact(num_conv=2, trainable=True).trainable is True
    assert R.SRVGGNetCompact(num_conv=2, precision="strict", trainable=True).precision == "strict"
    with pytest.raises(ValueError, match="exact16"):
        R.SRVGGNetCompact(num_conv=2, precision="exact16", trainable=True)
    monkeypatch.setenv("RESR_PRECISION", "exact16")
    with pytest.raises(ValueError, match="exact16"):
        R.SRVGGNetCompact(num_conv=2, trainable=True)
    assert R.SRVGGNetCompact(num_conv=2).precision == "exact16"          # without the flag exact16 stays what it was
    for act in ("prelu", "leakyrelu", "relu"):
        torch.manual_seed(5)
        a = R.SRVGGNetCompact(num_conv=3, upscale=2, act_type=act, precision="fast").state_dict()
        torch.manual_seed(5)
        b = R.SRVGGNetCompact(num_conv=3, upscale=2, act_type=act, precision="fast", trainable=True).state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


# One case with identity slopes and one without (the gated sizes of the GPU test): the three evaluators against each other.
@pytest.mark.parametrize("case", [G.CASES[5], G.CASES[3]], ids=G.case_id)
def test_reference_evaluators_agree(case):
    sd, x, gy = G.make_case(case)
    nc, s, act = case[:3]
    y64, g64 = G.evaluate("f64", sd, x, gy, nc, s, act)
    y32, g32 = G.evaluate("f32", sd, x, gy, nc, s, act)
    y16, g16 = G.evaluate("emu16", sd, x, gy, nc, s, act)
    assert set(g64) == set(sd) | {"x"} and all(g64[k].shape == sd[k].shape for k in sd) and g64["x"].shape == x.shape
    w32, _ = G.worst_median(G.errors(g32, g64))
    w16, m16 = G.worst_median(G.errors(g16, g64))
    assert w32 < 1e-5 and G.error(y32, y64) < 1e-6, (w32, G.errors(g32, g64))
    assert 1e-4 < m16 <= w16 < 0.1, (w16, m16, G.errors(g16, g64))
    assert 1e-6 < G.error(y16, y64) < 1e-3
    # the emulation's roundings sit at the native pass's lift: a cotangent 2^-12 times as large gives the same gradients, scaled
    _, g16s = G.evaluate("emu16", sd, x, gy * 2.0 ** -12, nc, s, act)
    assert G.lift_of(gy * 2.0 ** -12) == G.lift_of(gy) * 2.0 ** 12
    assert all(torch.equal(g16s[k] * 2.0 ** 12, g16[k]) for k in g16)
