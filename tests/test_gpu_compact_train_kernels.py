"""-m gpu: the three kernels of the compact generator's training pass (csrc/compact_train.hip), each alone through its debug entry
(include/resr_debug.h), for f16 and f32, at 70 pixels (2 x 5 x 7: less than one block), 1961 (1 x 37 x 53: no multiple of the block)
and 2 x 64 x 65.

  * act, act_bwd: BIT FOR BIT the same expression evaluated on the CPU in fp32 and rounded once to the dtype.  The slopes hold
    negative values, 0, 1 and values above 1; z holds +0, -0 and f16 subnormals of both signs.
  * slope gradients: against float64 within n * 2^-24 * sum |term| per channel (the bound of any fp32 summation order over n terms),
    the same bits on two runs, and exactly the un-lifted value through a pre-scale slot.
  * residual_bwd, s = 1..4: against the float64 sum within s^2 * 2^-24 * sum |term|; exact for s = 1; onto a gx that holds something it
    is one fp32 add.
  * every output lies between guard elements that must survive, and is pre-filled with a sentinel that must be gone.
Every judgement goes to <diag_dir>/test_gpu_compact_train_kernels.json.
"""
import ctypes as C
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

PIXELS = [(70, "2x5x7"), (1961, "1x37x53"), (2 * 64 * 65, "2x64x65")]
GUARD = 64            # elements on either side of an output
SENT = 12345.0        # never a result of the cases below
RECORDS = {}


@pytest.fixture(scope="module")
def L():
    import real_esrgan_pytorch_amd as pkg
    pkg._lib.lib()
    return pkg._lib


@pytest.fixture(scope="module", autouse=True)
def _write_diag(diag_dir):
    yield
    with open(os.path.join(diag_dir, "test_gpu_compact_train_kernels.json"), "w") as f:
        json.dump(RECORDS, f, indent=1, sort_keys=True)


def _dt(L, kind):
    return (L.RESR_F16, torch.float16) if kind == "f16" else (L.RESR_F32, torch.float32)


def _ok(L, rc):
    assert rc == 0, (rc, L.lib().resr_last_error())


class Guarded:
    """A device tensor of `numel` elements between two guards, all of it the sentinel; `check()` returns the payload."""

    def __init__(self, numel, dtype):
        self.buf = torch.full((numel + 2 * GUARD,), SENT, dtype=dtype, device="cuda")
        self.numel = numel

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

    @property
    def payload(self):
        return self.buf[GUARD:GUARD + self.numel]

    def check(self):
        torch.cuda.synchronize()
        assert torch.all(self.buf[:GUARD] == SENT) and torch.all(self.buf[GUARD + self.numel:] == SENT), "a guard was overwritten"
        out = self.payload.clone()
        assert not torch.any(out == SENT), "an element was not written"
        return out


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _slopes():
    g = torch.Generator().manual_seed(7)
    s = torch.rand(64, generator=g) * 2.5 - 0.75          # negative ... above 1
    s[3], s[17], s[40], s[41], s[63] = 0.0, 1.0, -0.5, 1.75, 0.015625
    return s


def _inputs(pixels, tdtype, seed):
    """z and g [pixels, 64] as the dtype stores them (values every dtype of the test holds exactly), special values planted in z."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(pixels, 64, generator=g).to(torch.float16)
    gr = (torch.randn(pixels, 64, generator=g) * 3).to(torch.float16)
    flat = z.view(-1)
    sub = 2.0 ** -24     # the smallest f16 subnormal
    special = [0.0, -0.0, sub, -sub, 37 * sub, -37 * sub, 2.0 ** -14, -(2.0 ** -14), 1023 * sub, -1023 * sub]
    for i, v in enumerate(special * 13):                  # spread over the channels (130 is no multiple of 64)
        flat[(i * 97) % flat.numel()] = v
    return z.to(tdtype), gr.to(tdtype)


def _act_ref(z, slopes, tdtype):
    zf = z.float()
    return torch.where(zf > 0, zf, slopes.float() * zf).to(tdtype)


def _act_bwd_ref(g, z, slopes, tdtype):
    one = torch.ones(())
    return (g.float() * torch.where(z.float() > 0, one, slopes.float().expand_as(z))).to(tdtype)


@pytest.mark.parametrize("kind", ["f16", "f32"])
@pytest.mark.parametrize("pixels,name", PIXELS)
def test_act(L, kind, pixels, name):
    dt, tdtype = _dt(L, kind)
    slopes = _slopes()
    z, _ = _inputs(pixels, tdtype, pixels)
    out = Guarded(pixels * 64, tdtype)
    zd, sd = z.cuda(), slopes.cuda()
    _ok(L, L.lib().resr_debug_compact_act(L.ptr(zd), out.ptr, L.ptr(sd), pixels, dt, L.stream_ptr(zd)))
    got = out.check().cpu().view(pixels, 64)
    want = _act_ref(z, slopes, tdtype)
    differ = int((_bits(got) != _bits(want)).sum())
    RECORDS[f"act:{kind}:{name}"] = {"elements": pixels * 64, "differ": differ}
    assert differ == 0
    assert torch.equal(zd.cpu(), z)                       # the source is left alone


@pytest.mark.parametrize("kind", ["f16", "f32"])
@pytest.mark.parametrize("pixels,name", PIXELS)
def test_act_bwd_and_slope_gradient(L, kind, pixels, name):
    dt, tdtype = _dt(L, kind)
    lib = L.lib()
    slopes = _slopes()
    z, g = _inputs(pixels, tdtype, pixels + 1)
    zd, gd, sd = z.cuda(), g.cuda(), slopes.cuda()
    st = L.stream_ptr(zd)
    want = _act_bwd_ref(g, z, slopes, tdtype)
    partial = torch.zeros(1024 * 64, dtype=torch.float32, device="cuda")
    pbytes = partial.numel() * 4

    # without a slope gradient (LeakyReLU / ReLU layers), out of place
    out = Guarded(pixels * 64, tdtype)
    _ok(L, lib.resr_debug_compact_act_bwd(L.ptr(gd), L.ptr(zd), out.ptr, L.ptr(sd), pixels, dt, None, None, 0, None, st))
    d_plain = int((_bits(out.check().cpu().view(pixels, 64)) != _bits(want)).sum())

    # with it, twice, in place (what the backward pass does)
    runs = []
    for _ in range(2):
        io = Guarded(pixels * 64, tdtype)
        io.payload.copy_(gd.view(-1))
        ds = Guarded(64, torch.float32)
        _ok(L, lib.resr_debug_compact_act_bwd(io.ptr, L.ptr(zd), io.ptr, L.ptr(sd), pixels, dt, ds.ptr, L.ptr(partial), pbytes, None, st))
        runs.append((io.check().cpu().view(pixels, 64), ds.check().cpu()))
    d_inplace = int((_bits(runs[0][0]) != _bits(want)).sum())
    term = g.double() * torch.where(z.double() > 0, torch.zeros((), dtype=torch.float64), z.double())
    ref, bound = term.sum(0), pixels * 2.0 ** -24 * term.abs().sum(0)
    ratio = ((runs[0][1].double() - ref).abs() / bound).max().item()
    same = torch.equal(_bits(runs[0][1]), _bits(runs[1][1])) and torch.equal(_bits(runs[0][0]), _bits(runs[1][0]))

    # through a pre-scale slot: the slot holds m = 2^-3 (a pass lifted by 2^3), the gradients leave times 2^-3, exactly
    slot = torch.tensor([2.0 ** -3, 0.0, 0.0], dtype=torch.float32, device="cuda")
    io = Guarded(pixels * 64, tdtype)
    io.payload.copy_(gd.view(-1))
    ds = Guarded(64, torch.float32)
    _ok(L, lib.resr_debug_compact_act_bwd(io.ptr, L.ptr(zd), io.ptr, L.ptr(sd), pixels, dt, ds.ptr, L.ptr(partial), pbytes, L.ptr(slot), st))
    unlifted = torch.equal(ds.check().cpu(), runs[0][1] * 2.0 ** -3)

    RECORDS[f"act_bwd:{kind}:{name}"] = {"elements": pixels * 64, "differ": d_plain, "differ_in_place": d_inplace, "dslope_ratio": ratio,
                                         "same_bits_twice": same, "unlifted_exactly": unlifted}
    assert d_plain == 0 and d_inplace == 0
    assert ratio <= 1.0, ratio
    assert same and unlifted
    assert torch.equal(zd.cpu(), z) and torch.equal(gd.cpu(), g)


@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 37, 53)], ids=["2x3x5x7", "1x3x37x53"])
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_residual_bwd(L, s, shape):
    lib = L.lib()
    n, h, w = shape
    gen = torch.Generator().manual_seed(s * 100 + h)
    gy = torch.randn(n, 3, h * s, w * s, generator=gen)
    gyd = gy.cuda()
    st = L.stream_ptr(gyd)
    out = Guarded(n * 3 * h * w, torch.float32)
    out.payload.zero_()                                   # the kernel adds to what gx holds: onto zeros it is the sum itself
    _ok(L, lib.resr_debug_compact_residual_bwd(L.ptr(gyd), out.ptr, n, h, w, s, st))
    got = out.check().cpu().view(n, 3, h, w)
    terms = gy.double().view(n, 3, h, s, w, s)
    ref, bound = terms.sum((3, 5)), s * s * 2.0 ** -24 * terms.abs().sum((3, 5))
    ratio = ((got.double() - ref).abs() / bound).max().item()
    exact1 = torch.equal(got, gy) if s == 1 else None
    # onto a gx that holds something (what the backward pass does): one fp32 add
    base = torch.randn(n * 3 * h * w, generator=gen)
    out2 = Guarded(n * 3 * h * w, torch.float32)
    out2.payload.copy_(base.cuda())
    _ok(L, lib.resr_debug_compact_residual_bwd(L.ptr(gyd), out2.ptr, n, h, w, s, st))
    accumulated = torch.equal(out2.check().cpu(), base + got.view(-1))
    RECORDS[f"residual_bwd:s{s}:{n}x3x{h}x{w}"] = {"ratio": ratio, "exact_s1": exact1, "accumulated": accumulated}
    assert ratio <= 1.0, ratio
    assert exact1 is not False and accumulated
    assert torch.equal(gyd.cpu(), gy)


def test_refusals_launch_nothing(L):
    lib = L.lib()
    z = torch.zeros(70 * 64, dtype=torch.float16, device="cuda")
    out = Guarded(70 * 64, torch.float16)
    ds = Guarded(64, torch.float32)
    sl = torch.zeros(64, dtype=torch.float32, device="cuda")
    small = torch.zeros(64, dtype=torch.float32, device="cuda")
    st = L.stream_ptr(z)
    assert lib.resr_debug_compact_act(None, out.ptr, L.ptr(sl), 70, L.RESR_F16, st) == L.RESR_ERR_ARG
    assert lib.resr_debug_compact_act(L.ptr(z), out.ptr, L.ptr(sl), 70, L.RESR_F16X2, st) == L.RESR_ERR_ARG
    assert lib.resr_debug_compact_act(L.ptr(z), out.ptr, L.ptr(sl), 0, L.RESR_F16, st) == L.RESR_ERR_ARG
    assert lib.resr_debug_compact_act_bwd(L.ptr(z), L.ptr(z), out.ptr, None, 70, L.RESR_F16, None, None, 0, None, st) == L.RESR_ERR_ARG
    # 70 pixels of f16 are 3 blocks: 3 * 256 bytes of partials
    assert lib.resr_debug_compact_act_bwd(L.ptr(z), L.ptr(z), out.ptr, L.ptr(sl), 70, L.RESR_F16, ds.ptr, L.ptr(small), 256, None, st) == L.RESR_ERR_WORKSPACE
    assert lib.resr_debug_compact_act_bwd(L.ptr(z), L.ptr(z), out.ptr, L.ptr(sl), 70, L.RESR_F16, ds.ptr, None, 0, None, st) == L.RESR_ERR_WORKSPACE
    assert lib.resr_debug_compact_residual_bwd(L.ptr(z), out.ptr, 1, 5, 7, 5, st) == L.RESR_ERR_ARG
    assert lib.resr_debug_compact_residual_bwd(L.ptr(z), out.ptr, 1, 5, 7, 0, st) == L.RESR_ERR_ARG
    torch.cuda.synchronize()
    assert torch.all(out.buf == SENT) and torch.all(ds.buf == SENT)
