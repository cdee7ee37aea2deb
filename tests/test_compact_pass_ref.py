"""CPU: tests/compact_pass_ref.py before tests/test_gpu_compact_train_passes.py relies on it.

  * the definitions (pixel shuffle and its inverse, the transposed convolution, the residual's adjoint) against torch;
  * pinned_backward on float64's own forward IS float64 autograd: every tensor of every case within 1e-12 of its max-norm;
  * the per-pass rule accepts the CPU stand-in for the device (emulate_passes: float64 with the native pass's roundings) on every run
    of section 3a, fast and strict, and rejects it with each of six faults planted -- in the pass the fault sits in;
  * what the whole-network gate of tests/test_gpu_compact_train.py (worst and median tensor within 2 x the unpinned f16 emulation, its
    4e-2 class) says to the same faulty gradients, on the general case that test gates (2-x1-prelu-drawn-1x37x53);
  * section 3b's condition on the reference alone, and its gate, with the emulated forward standing in for the device.
The figures go to <diag_dir>/test_compact_pass_ref.json.

The old gate and the six faults (worst / median tensor against float64 autograd; the gate on this case is 6.2e-2 / 1.6e-2):
  one border column dropped from conv 0's backward-data pass   3.7e-2 / 8.1e-3   ACCEPTED -- the rule: g_xin, 111 elements
  one value in a pad channel of g_t                            3.1e-2 / 7.8e-3   ACCEPTED (no gradient changes) -- the rule: g_t_pad
  the same column dropped from the last conv's pass            1.0e-1 / 5.0e-2   rejected
  the top layer's mask from a > 0 under drawn slopes           8.4e-1 / 5.4e-1   rejected (layer 0's: 7.6e-1 / 8.1e-3, rejected too)
  dslope of the top layer from z_{k-1}                         1.6    / 8.1e-3   rejected
  1 / lift omitted from db of conv 0                           31     / 7.8e-3   rejected
  conv 0's weight gradient from the other ping-pong buffer     2.7    / 7.8e-3   rejected
A mask taken from a_k is wrong in every channel with a negative slope, a quarter of the drawn ones, on every pixel with z < 0: that is
no small fault and the old gate sees it.  What it lets through is what stays inside one tensor's 4e-2: a border column of the input
gradient, a pad channel.  On the general cases below 37 x 53 the old test gates nothing at all.
"""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from tests import compact_grad_ref as G
from tests import compact_pass_ref as P
from tests import conv_ref as R

F64 = torch.float64
RECORDS = {"old_gate": {}, "pinned": {}, "clean": {}}
OLD_GATE_CASE = G.CASES[3]          # the PReLU case tests/test_gpu_compact_train.py gates in fast mode
SMALL_CASE = P.CASES_3A[0]


@pytest.fixture(scope="module", autouse=True)
def _write_diag(diag_dir):
    yield
    with open(os.path.join(diag_dir, "test_compact_pass_ref.json"), "w") as f:
        json.dump(RECORDS, f, indent=1, sort_keys=True)


def test_definitions_against_torch():
    g = torch.Generator().manual_seed(3)
    for s in (1, 2, 3, 4):
        t = torch.randn(2, 3 * s * s, 5, 7, generator=g, dtype=F64)
        assert torch.equal(P.pixel_shuffle(t, s), F.pixel_shuffle(t, s))
        y = torch.randn(2, 3, 5 * s, 7 * s, generator=g, dtype=F64)
        assert torch.equal(P.pixel_unshuffle(y, s), F.pixel_unshuffle(y, s))
        assert torch.equal(P.pixel_unshuffle(P.pixel_shuffle(t, s), s), t)
        x = torch.randn(2, 3, 5, 7, generator=g, dtype=F64, requires_grad=True)
        assert torch.equal(P.nearest(x.detach(), s), F.interpolate(x.detach(), scale_factor=s, mode="nearest"))
        (gx,) = torch.autograd.grad(F.interpolate(x, scale_factor=s, mode="nearest"), x, y)
        assert (P.residual_adjoint(y, s, F64) - gx).abs().max() <= 1e-14 * gx.abs().max()
    for cout, cin in ((12, 64), (64, 3), (64, 64)):
        wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=F64)
        go = torch.randn(2, cout, 6, 9, generator=g, dtype=F64)
        want = F.conv_transpose2d(go, wt, padding=1)
        assert (P.dgrad(go, wt, F64) - want).abs().max() <= 1e-13 * want.abs().max()
        x = torch.randn(2, cin, 6, 9, generator=g, dtype=F64)
        wr = wt.clone().requires_grad_(True)
        (dw,) = torch.autograd.grad(F.conv2d(x, wr, padding=1), wr, go)
        assert (R.wgrad(x, go, 1.0, F64)[0] - dw).abs().max() <= 1e-13 * dw.abs().max()
    z = torch.tensor([[-2.0, -0.0, 0.0, 3.0]]).view(1, 4, 1, 1).half()
    sl = torch.tensor([-0.5, 0.25, 2.0, 7.0])
    assert torch.equal(P.act_fwd(z, sl, torch.float16).flatten(), torch.tensor([1.0, -0.0, 0.0, 3.0]).half())
    assert torch.equal(P.act_factor(z, sl).flatten(), torch.tensor([-0.5, 0.25, 2.0, 1.0], dtype=F64))


ALL_CASES = list(dict.fromkeys(G.CASES + P.CASES_3A + P.CASES_3B))


@pytest.mark.parametrize("case", ALL_CASES, ids=G.case_id)
def test_pinned_backward_is_autograd_on_its_own_forward(case):
    nc, s, act = case[:3]
    sd, x, gy = G.make_case(case)
    _, g64 = G.evaluate("f64", sd, x, gy, nc, s, act)
    x_in, z, a = P.forward64(sd, x, nc, act)
    got = P.pinned_backward(sd, x_in, z, a, gy, nc, s, act, round16=False)
    assert set(got) == set(g64)
    errs = G.errors(got, g64)
    assert max(errs.values()) <= 1e-12, errs
    # one linear map of g_y: the roundings sit at the lift, so a cotangent 2^-12 times as large gives the same gradients, scaled
    e = P.pinned_backward(sd, x_in, z, a, gy, nc, s, act, round16=True)
    es = P.pinned_backward(sd, x_in, z, a, gy * 2.0 ** -12, nc, s, act, round16=True)
    assert all(torch.equal(es[k] * 2.0 ** 12, e[k]) for k in e)


@pytest.mark.parametrize("fast", [True, False], ids=["fast", "strict"])
@pytest.mark.parametrize("run", P.RUNS_3A, ids=P.run_id)
def test_rule_accepts_the_emulated_passes(run, fast):
    case, shift = run
    nc, s, act = case[:3]
    sd, x, gy = G.make_case(case)
    gy = gy * 2.0 ** shift
    dev = P.emulate_passes(sd, x, gy, nc, s, act, fast)
    if fast:
        top = float(gy.abs().max()) * dev["lift"]
        assert (dev["lift"] == 1.0 and top >= 64.0) if shift == 7 else (dev["lift"] >= 16.0 * 2.0 ** -shift and 64.0 <= top < 128.0)
    rows = P.judge_passes(dev, sd, x, gy, nc, s, act, fast)
    names = [r["pass"] for r in rows]
    assert len(set(names)) == len(names)
    want = {"x_in", "t", "y", "g_t", "g_t_pad", "g_xin", "g_xin_pad", "gx", f"dW_{nc + 1}", f"db_{nc + 1}"}
    for k in range(nc + 1):
        want |= {f"z_{k}", f"a_{k}", f"g_z_{k}", f"dW_{k}", f"db_{k}"}
        want |= {f"dslope_{k}"} if act == "prelu" else set()
        want |= {f"g_z_{k}_where_z<=0"} if act == "relu" else set()
    assert set(names) == want
    RECORDS["clean"][f"{P.run_id(run)}:{'fast' if fast else 'strict'}"] = max(r["ratio"] for r in rows)
    assert not P.bad_passes(rows), P.bad_passes(rows)


# (fault, the passes the rule must name -- as a function of the top layer k): every fault sits in ONE pass, so nothing else may be named
def _expected(fault, top):
    name, at = fault if isinstance(fault, tuple) else (fault, None)
    return {
        "dgrad_drops_border_column": {"g_xin"} if at == 0 else {f"g_z_{top if at is None else at - 1}"},
        "mask_from_a": {f"g_z_{top if at is None else at}"},
        "g_t_pad_nonzero": {"g_t", "g_t_pad"},
        "dslope_reads_other_z": {f"dslope_{top}"},
        "db_without_unlift": {"db_0"},
        "ping_pong_swapped": {"dW_0", "db_0"},
    }[name]


FAULTS = [("dgrad_drops_border_column", 0), "dgrad_drops_border_column", ("dgrad_drops_border_column", 1), "mask_from_a", ("mask_from_a", 0),
          "g_t_pad_nonzero", "dslope_reads_other_z", "db_without_unlift", "ping_pong_swapped"]
_fid = lambda f: f if isinstance(f, str) else f"{f[0]}@{f[1]}"


@pytest.fixture(scope="module")
def old_gate():
    """The gate of tests/test_gpu_compact_train.py on OLD_GATE_CASE: (float64 autograd's gradients, 2 x the emulation's worst, ... median)."""
    nc, s, act = OLD_GATE_CASE[:3]
    sd, x, gy = G.make_case(OLD_GATE_CASE)
    _, g64 = G.evaluate("f64", sd, x, gy, nc, s, act)
    _, g16 = G.evaluate("emu16", sd, x, gy, nc, s, act)
    w, m = G.worst_median(G.errors(g16, g64))
    assert w < 0.1                                                   # the old test's own condition on its emulation
    return g64, 2.0 * w, 2.0 * m


@pytest.mark.parametrize("case", [SMALL_CASE, OLD_GATE_CASE], ids=G.case_id)
@pytest.mark.parametrize("fault", FAULTS, ids=_fid)
def test_rule_rejects_a_planted_fault(fault, case, old_gate):
    nc, s, act = case[:3]
    sd, x, gy = G.make_case(case)
    dev = P.emulate_passes(sd, x, gy, nc, s, act, True, fault)
    bad = P.bad_passes(P.judge_passes(dev, sd, x, gy, nc, s, act, True))
    want = _expected(fault, nc)
    # a wrong g_a also shows in the slope gradient computed from it: the one pass act_bwd is
    allowed = want | ({p.replace("g_z", "dslope") for p in want if p.startswith("g_z")})
    assert bad and want <= set(bad) <= allowed, (fault, bad)
    if case is OLD_GATE_CASE:
        g64, gate_worst, gate_median = old_gate
        errs = G.errors(P.device_grads(dev), g64)
        worst, median = G.worst_median(errs)
        RECORDS["old_gate"][_fid(fault)] = {"worst": worst, "median": median, "gate_worst": gate_worst, "gate_median": gate_median,
                                           "accepted": worst <= gate_worst and median <= gate_median, "worst_tensor": max(errs, key=errs.get),
                                           "rule_bad": bad}


def test_the_old_gate_accepts_some_of_the_faults(old_gate):
    """The evidence that the gap was real: faults the per-pass rule rejects (above) and the whole-network distance lets through."""
    nc, s, act = OLD_GATE_CASE[:3]
    sd, x, gy = G.make_case(OLD_GATE_CASE)
    g64, gate_worst, gate_median = old_gate
    accepted = {}
    for fault in FAULTS + [None]:
        worst, median = G.worst_median(G.errors(P.device_grads(P.emulate_passes(sd, x, gy, nc, s, act, True, fault)), g64))
        accepted[_fid(fault) if fault else "none"] = worst <= gate_worst and median <= gate_median
    assert accepted["none"]
    assert accepted["dgrad_drops_border_column@0"] and accepted["g_t_pad_nonzero"], accepted
    # recorded, not required: the old gate does see these (the module docstring has the figures)
    assert not accepted["db_without_unlift"] and not accepted["ping_pong_swapped"] and not accepted["dslope_reads_other_z"], accepted


@pytest.mark.parametrize("case", P.CASES_3B, ids=G.case_id)
def test_pinned_yardstick_condition_and_gate_on_the_emulated_forward(case):
    nc, s, act = case[:3]
    sd, x, gy = G.make_case(case)
    dev = P.emulate_passes(sd, x, gy, nc, s, act, True)
    rec = P.pinned_gate(P.device_grads(dev), sd, dev, gy, nc, s, act)
    RECORDS["pinned"][G.case_id(case)] = rec
    assert rec["condition"], rec                                      # section 3b's condition on the reference alone
    assert 2e-4 < rec["yardstick_median"] <= rec["yardstick_worst"] < 8e-4, rec    # f16's 2^-11, not the 4e-2 of flipped masks
    assert rec["ok"], rec
    # the unpinned distance of the same gradients is the old class: the pinning is what sharpens the judgement
    _, g64 = G.evaluate("f64", sd, x, gy, nc, s, act)
    unpinned, _ = G.worst_median(G.errors(P.device_grads(dev), g64))
    assert unpinned > 10.0 * rec["worst"], (unpinned, rec)
    # and a fault under the old gate's 4e-2 is far outside the pinned one
    bad = P.emulate_passes(sd, x, gy, nc, s, act, True, ("dgrad_drops_border_column", 0))
    assert not P.pinned_gate(P.device_grads(bad), sd, dev, gy, nc, s, act)["ok"]
