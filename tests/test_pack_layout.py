"""CPU: the packed weight layout did not move.  Every chunk table, size and offset the library reports -- generator, compact generator,
discriminator, the VGG19 table of ContentLoss -- equals tests/golden/pack_layout.json byte for byte (chunk count, SHA-256 of the table,
every size), a fixture written by tests/golden/gen_pack_layout_golden.py BEFORE the layout got its one definition
(csrc/packed_layout.h); and the one-convolution entries (resr_conv_pack_table, resr_conv_packed_elems, resr_packed_bytes,
resr_packed_mx_offset) equal the format written out here.  All host arithmetic: no GPU."""
import ctypes as C
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("gen_pack_layout_golden", os.path.join(HERE, "golden", "gen_pack_layout_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(gen.OUT) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def L():
    import __graft_entry__
    __graft_entry__.build()
    import real_esrgan_pytorch_amd as R
    return R._lib


@pytest.fixture(scope="module")
def reported(L):
    return gen.collect(L)


def test_the_fixture_covers_every_descriptor(reported):
    # generator: 3 upscales x (f16, f32, exact16 with three plans); compact: 4 x 2 x 3; discriminator: 3 x 2; the VGG table
    assert len(reported) == 3 * 5 + 4 * 2 * 3 + 3 * 2
    assert sorted(GOLDEN) == sorted(list(reported) + ["vgg19"])


@pytest.mark.parametrize("name", sorted(k for k in GOLDEN if k != "vgg19"))
def test_tables_and_sizes_did_not_move(reported, name):
    got = json.loads(json.dumps(reported[name]))
    assert got == GOLDEN[name]
    flat = json.dumps(got)
    assert '"chunks": 0' not in flat and '"workspace_bytes": 0' not in flat and '"param_count": 0' not in flat   # no refused descriptor


def test_vgg_table_of_content_loss_did_not_move(L):
    import real_esrgan_pytorch_amd as R
    m = R.ContentLoss(["features.35"], [0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    host, fwd, bwd, elems = m._table()          # no device: the host half of ContentLoss._pack
    assert gen.vgg_record(host, fwd, bwd, elems) == GOLDEN["vgg19"]
    old = gen.vgg_table(L)                      # ... and the loop ContentLoss used to hold, chunk by chunk
    assert bytes(host) == bytes(old[0]) and (fwd, bwd, elems) == old[1:]


def _r32(v):
    return (v + 31) // 32 * 32


@pytest.mark.parametrize("cout,cin", [(64, 3), (32, 160), (3, 64), (512, 256), (1, 64)])
@pytest.mark.parametrize("transposed", [0, 1])
def test_conv_pack_table_is_the_format(L, cout, cin, transposed):
    """M rows in groups of at most 64, group-major; each group its K chunks of 32; one (group, chunk) block = 9 * mt * 1024 elements;
    m_count / k_count clamped to the real counts."""
    src_off, dst_off, scale = 1234, 5 * 9216, 0.5
    m_real, k_real = (cin, cout) if transposed else (cout, cin)
    want, off = [], dst_off
    for g0 in range(0, _r32(m_real), 64):
        mt = min(64, _r32(m_real) - g0) // 32
        for k0 in range(0, _r32(k_real), 32):
            want.append((src_off, off, cout, cin, g0, min(64, m_real - g0), k0, min(32, k_real - k0), mt, transposed, scale, 0, None))
            off += 9 * mt * 1024
    lib = L.lib()
    assert lib.resr_conv_pack_table(cout, cin, transposed, src_off, dst_off, scale, None, 0) == len(want)
    host, elems = L.conv_pack_table(cout, cin, transposed, src_off, dst_off, scale)
    names = [f[0] for f in L.PackChunk._fields_]
    assert [tuple(getattr(c, n) for n in names) for c in host] == want
    assert bytes(host) == bytes((L.PackChunk * len(want))(*[L.PackChunk(*w) for w in want]))   # padding bytes zero
    assert elems == off - dst_off == lib.resr_conv_packed_elems(cout, cin) == 9 * 1024 * (_r32(cout) // 32) * (_r32(cin) // 32)
    # too small a capacity, and arguments that are no convolution, are refused
    small = (L.PackChunk * 1)()
    if len(want) > 1:
        assert lib.resr_conv_pack_table(cout, cin, transposed, 0, 0, 1.0, C.cast(small, C.c_void_p), 1) < 0
    assert lib.resr_conv_pack_table(0, cin, transposed, 0, 0, 1.0, None, 0) < 0
    assert lib.resr_conv_pack_table(cout, cin, 2, 0, 0, 1.0, None, 0) < 0
    for dtype, size in ((L.RESR_F16, 2), (L.RESR_F32, 4), (L.RESR_F16X2, 6)):
        assert lib.resr_packed_bytes(elems, dtype) == elems * size + 16384
    assert lib.resr_packed_mx_offset(elems) == (elems * 6 + 16384 + 255) // 256 * 256
