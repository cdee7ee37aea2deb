"""CPU: tests/generator_pass_ref.py before tests/test_gpu_generator_passes.py relies on it, and the host-only offsets entry that test
reads the workspace through.

  * the float64 forward of generator_pass_ref IS oracle.model_ref.generator_forward, and pinned_backward on that forward's own masks and
    values IS float64 autograd of it: every parameter and the input within 1e-10 of the tensor's max-norm, at upscale 4, 2 and 1 and
    with two RRDBs (the ring rotates past e);
  * the per-pass rule accepts the CPU stand-in for the device (emulate_passes: float64 with the native pass's roundings) on every run
    of section 3a, fast and strict -- with either legal f16 evaluation of the folded conv5 blocks --, and rejects it with each of the
    thirteen faults planted (fast: all; strict: one per kind of row): in the pass the fault sits in and in no other, because every later
    pass is judged on what the faulty one stored;
  * section 3b's condition on the reference alone (the pinned f16 yardstick's worst tensor below 5e-3) and its gate, with the emulated
    forward standing in for the device, for the seeds the GPU test uses;
  * resr_debug_generator_train_offsets against the public sizes.
The figures go to <diag_dir>/test_generator_pass_ref.json.
"""
import ctypes as C
import json
import os

import pytest
import torch

from oracle import model_ref as M
from tests import generator_pass_ref as P

F64 = torch.float64
RECORDS = {"clean": {}, "faults": {}, "pinned": {}, "autograd": {}}


@pytest.fixture(scope="module", autouse=True)
def _write_diag(diag_dir):
    yield
    with open(os.path.join(diag_dir, "test_generator_pass_ref.json"), "w") as f:
        json.dump(RECORDS, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("case", [P.CASES_3A[0], P.CASES_3A[2], P.CASES_3A[3], P.CASES_3B[0]], ids=P.case_id)
def test_references_composed_are_autograd(case):
    s, n, h, w, nb, _ = case
    sd, x, gy = P.make_case(case)
    p = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    xi = x.double().clone().requires_grad_(True)
    y = M.generator_forward(xi, p, s, nb)
    fw = P.forward64(sd, x, s, nb)
    assert (fw["y"] - y.detach()).abs().max() <= 1e-13
    assert 0 < int(fw["ymask"].sum()) < fw["ymask"].numel()                     # the clamp is active on some elements and not on all
    names = list(p)
    grads = torch.autograd.grad(y, [p[k] for k in names] + [xi], gy.double())
    want = dict(zip(names + ["x"], grads))
    got = P.pinned_backward(P.exact_weights(sd, nb), fw, gy, s, nb, sd, round16=False, consts=P.EXACT)
    assert set(got) == set(want)
    errs = {k: float((got[k] - want[k]).abs().max() / want[k].abs().max()) for k in want}
    RECORDS["autograd"][P.case_id(case)] = max(errs.values())
    assert max(errs.values()) <= 1e-10, errs
    # one linear map of g_y: the roundings sit at the lift, so a cotangent 2^-12 times as large gives the same gradients, scaled
    W = P.packed_weights(sd, nb, True)
    e = P.pinned_backward(W, fw, gy, s, nb, sd, round16=True)
    es = P.pinned_backward(W, fw, gy * 2.0 ** -12, s, nb, sd, round16=True)
    assert all(torch.equal(es[k] * 2.0 ** 12, e[k]) for k in e)


def _row_names(nb):
    names = ["x_in", "x_in pad", "conv1"]
    for key in P.rdb_keys(nb):
        for k in range(1, 5):
            names += [f"{key}.o{k}", f"{key}.sign{k}"]
        names.append(f"{key}.conv5")
    names += ["conv2+skip", "upsampling1", "upsampling2", "upsampling2 sign", "conv3", "conv3 sign", "conv4 -> y", "ymask"]
    fwd = len(names)
    names += ["slot", "g4", "g4 pad", "dW conv4", "db conv4", "gA = conv4^T g4, masked", "dW conv3.0", "db conv3.0", "gB = conv3^T gA, masked",
              "dW upsampling2.0", "db upsampling2.0", "gA = upsampling2^T gB", "gM1 = pool gA, masked", "dW upsampling1.0", "db upsampling1.0",
              "gA = upsampling1^T gM1", "gF = pool gA", "dW conv2", "db conv2", "gT = conv2^T gF"]
    for key in reversed(P.rdb_keys(nb)):
        names += [f"{key}.g_o{k}" for k in (4, 3, 2, 1)] + [f"{key}.g_x"]
        names += [f"{t} {key}.conv{k}" for k in range(1, 6) for t in ("dW", "db")]
    names += ["add_inplace gF", "dW conv1", "db conv1", "g_xin", "g_xin pad", "gx"]
    return names, fwd


@pytest.mark.parametrize("fast", [True, False], ids=["fast", "strict"])
@pytest.mark.parametrize("run", P.RUNS_3A, ids=P.run_id)
def test_rule_accepts_the_emulated_passes(run, fast):
    case, shift = run
    s, nb = case[0], case[4]
    sd, x, gy = P.make_case(case)
    gy = gy * 2.0 ** shift
    dev = P.emulate_passes(sd, x, gy, s, nb, fast)
    if fast:
        top = float(gy.abs().max()) * dev["lift"]
        assert (dev["lift"] == 1.0 and top >= 64.0) if shift == 7 else (dev["lift"] >= 16.0 * 2.0 ** -shift and 64.0 <= top < 128.0)
    else:
        assert dev["lift"] == 1.0
    rows = P.judge_passes(dev, sd, x, gy, s, nb, fast)
    want, _ = _row_names(nb)
    assert [r["pass"] for r in rows] == want                                      # one row per pass, in the order of the launches
    assert all(r["both_values"] for r in rows if "both_values" in r)             # every sign plane and ymask hold both values
    RECORDS["clean"][f"{P.run_id(run)}:{'fast' if fast else 'strict'}"] = max(r["ratio"] for r in rows)
    assert not P.bad_passes(rows), P.bad_passes(rows)
    if fast and shift == 0:
        # resr_pack_weights may hold either f16 evaluation of fold * w (generator_pass_ref.packed_weights): the rule accepts both, and
        # the term that lets it is the size of one f16 ulp of one small weight times the gradients around it
        W = P.packed_weights(sd, nb, True)
        assert any(bool((W[k + ".conv5@fold~"] != 0).any()) for k in P.rdb_keys(nb))
        rows = P.judge_passes(P.emulate_passes(sd, x, gy, s, nb, True, fused_pack=True), sd, x, gy, s, nb, True)
        assert not P.bad_passes(rows), P.bad_passes(rows)
        terms = [(r["weight_term"], r["kernel_err"]) for r in rows if "weight_term" in r]
        assert len(terms) == 15 and all(t <= 2.0 ** -20 for t, _ in terms) and max(e for _, e in terms) > 2.0 ** -14


# fault -> the rows that must name it (n_blocks = 1); nothing else may be named
_B = "trunk.0.rdb"
EXPECTED = {
    "rdb3_fold_0.2": {f"{_B}3.g_o4", f"{_B}3.g_o3", f"{_B}3.g_o2", f"{_B}3.g_o1", f"{_B}3.g_x"},
    "rdb3_t0_1": {f"{_B}3.g_x"},
    "rdb1_skip_from_newest_slot": {f"{_B}1.g_x"},
    "g_o4_mask_of_o3": {f"{_B}3.g_o4"},
    "g_o4_conv5_slice_of_o3": {f"{_B}3.g_o4"},
    "gM1_without_mask": {"gM1 = pool gA, masked"},
    "gF_with_mask": {"gF = pool gA"},
    "up2_wgrad_without_nearest": {"dW upsampling2.0"},
    "g4_ignores_ymask": {"g4"},
    "g4_pad_nonzero": {"g4 pad"},
    "hr_dgrad_drops_last_column": {"gA = conv4^T g4, masked"},
    "db_conv1_without_unlift": {"db conv1"},
    "conv5_forward_residual_1.0": {f"{_B}1.conv5"},
}


def test_every_fault_has_an_expectation():
    assert set(EXPECTED) == set(P.FAULTS) and len(P.FAULTS) == 13


# every fault in fast mode, the benchmarked one; in strict one fault per kind of row (a mirrored pass, a zero, an HR pass, a pool)
STRICT_TOO = ("rdb3_fold_0.2", "g4_pad_nonzero", "hr_dgrad_drops_last_column", "gM1_without_mask")


@pytest.mark.parametrize("fault,fast", [(f, True) for f in P.FAULTS] + [(f, False) for f in STRICT_TOO],
                         ids=lambda v: v if isinstance(v, str) else ("fast" if v else "strict"))
def test_rule_rejects_a_planted_fault(fault, fast):
    case = P.CASES_3A[0]
    s, nb = case[0], case[4]
    sd, x, gy = P.make_case(case)
    dev = P.emulate_passes(sd, x, gy, s, nb, fast, fault)
    bad = P.bad_passes(P.judge_passes(dev, sd, x, gy, s, nb, fast))
    RECORDS["faults"][f"{fault}:{'fast' if fast else 'strict'}"] = bad
    assert set(bad) == EXPECTED[fault], (fault, bad)


@pytest.mark.parametrize("case", P.CASES_3B, ids=P.case_id)
def test_pinned_yardstick_condition_and_gate_on_the_emulated_forward(case):
    s, nb = case[0], case[4]
    sd, x, gy = P.make_case(case)
    dev = P.emulate_passes(sd, x, gy, s, nb, True)
    rows = P.judge_passes(dev, sd, x, gy, s, nb, True, backward=False)
    names, fwd = _row_names(nb)
    assert [r["pass"] for r in rows] == names[:fwd] and not P.bad_passes(rows)
    rec = P.pinned_gate(P.device_grads(dev), sd, dev, gy, s, nb)
    RECORDS["pinned"][P.case_id(case)] = rec
    assert rec["condition"], rec                                      # section 3b's condition on the reference alone
    assert rec["ok"], rec
    # a wiring fault the whole-network gates let through is far outside the pinned one
    for fault in ("rdb3_t0_1", "rdb1_skip_from_newest_slot", "g_o4_mask_of_o3"):
        bad = P.emulate_passes(sd, x, gy, s, nb, True, fault)
        assert not P.pinned_gate(P.device_grads(bad), sd, dev, gy, s, nb)["ok"], fault


# ---- the offsets entry ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import __graft_entry__
    __graft_entry__.build()
    import real_esrgan_pytorch_amd as R
    return R._lib


def test_train_offsets_describe_the_documented_workspace(L):
    """resr_debug_generator_train_offsets (host only): the documented order, 256-byte alignment, room for every tensor, agreement with
    resr_generator_buffer_offsets where both name a buffer, everything inside resr_generator_workspace_bytes, the slot at the end of the
    zero-filled head, and the refusals."""
    lib = L.lib()
    count = L.RESR_DEBUG_GENERATOR_TRAIN_OFFSETS
    assert count == 25 and "resr_debug_generator_train_offsets" in L.exported_symbols()
    n, h, w = 2, 12, 20
    for upscale, r in ((4, 1), (2, 2), (1, 4)):
        for dtype, es in ((L.RESR_F16, 2), (L.RESR_F32, 4)):
            for nb in (1, 2):
                d = L.GeneratorDesc(n, h, w, 3, 3, upscale, nb, dtype, 1, 0, 0, 0)
                out = (C.c_int64 * (count + 1))(*([-7] * (count + 1)))
                assert lib.resr_debug_generator_train_offsets(C.byref(d), out, count) == count
                assert out[count] == -7
                o = list(out)[:count]
                (slot, xin, ws0, ws_stride, bits0, bits_stride, bits_u2, bits_c3, trunk_out, feat, u1, u2, c3, ymask, g4, gA, gB, gM1, gF,
                 gT0, gT_stride, gS0, gS_stride, gxin, partial) = o
                assert all(v % 256 == 0 for v in o)
                px, nrdb, ci_pad = n * (h // r) * (w // r), 3 * nb, (3 * r * r + 31) // 32 * 32
                total = lib.resr_generator_workspace_bytes(C.byref(d))
                head = lib.resr_generator_chain_state_bytes(C.byref(d))
                assert slot == head - 256 and xin == head                                              # the zero-filled head ends with the slot
                # the documented order, each buffer with room for its tensor
                assert ws0 - xin >= px * ci_pad * es
                assert ws_stride >= px * 192 * es and bits0 - ws0 >= nrdb * ws_stride
                assert bits_stride >= px * 4 * 4 and bits_u2 - bits0 >= nrdb * bits_stride
                assert bits_c3 - bits_u2 >= 16 * px * 2 * 4 and trunk_out - bits_c3 >= 16 * px * 2 * 4
                assert feat - trunk_out >= px * 64 * es and u1 - feat >= px * 64 * es
                assert u2 - u1 >= 4 * px * 64 * es and c3 - u2 >= 16 * px * 64 * es and ymask - c3 >= 16 * px * 64 * es
                assert g4 - ymask >= 16 * px * 3 and gA - g4 >= 16 * px * 32 * es
                assert gB - gA >= 16 * px * 64 * es and gM1 - gB >= 16 * px * 64 * es and gF - gM1 >= 4 * px * 64 * es
                assert gT0 - gF >= px * 64 * es and gT_stride >= px * 64 * es and gS0 - gT0 >= 4 * gT_stride
                assert gS_stride >= px * 128 * es and gxin - gS0 >= 3 * gS_stride
                assert partial - gxin >= px * ci_pad * es and partial < total                          # the last tensor, then the scratch
                # resr_generator_buffer_offsets names some of them too
                pub = (C.c_int64 * 32)()
                cnt = lib.resr_generator_buffer_offsets(C.byref(d), C.cast(pub, C.c_void_p), 32)
                names = ["x_in", "ws0", "out1", "trunk_out", "feat", "u1", "u2", "c3", "ymask", "g4", "gA", "gB", "gM1", "gF", "gT0", "gT1", "gT2",
                         "gT3", "gS", "gxin", "partial"]
                assert cnt == len(names)
                p = dict(zip(names, list(pub)[:cnt]))
                mine = {"x_in": xin, "ws0": ws0, "out1": ws0, "trunk_out": trunk_out, "feat": feat, "u1": u1, "u2": u2, "c3": c3, "ymask": ymask,
                        "g4": g4, "gA": gA, "gB": gB, "gM1": gM1, "gF": gF, "gT0": gT0, "gT1": gT0 + gT_stride, "gT2": gT0 + 2 * gT_stride,
                        "gT3": gT0 + 3 * gT_stride, "gS": gS0, "gxin": gxin, "partial": partial}
                assert p == mine
                assert lib.resr_debug_generator_train_offsets(C.byref(d), out, count - 1) == L.RESR_ERR_ARG     # too small a capacity
                assert lib.resr_debug_generator_train_offsets(C.byref(d), None, count) == L.RESR_ERR_ARG
                infer = L.GeneratorDesc(n, h, w, 3, 3, upscale, nb, dtype, 0, 0, 0, 0)
                assert lib.resr_debug_generator_train_offsets(C.byref(infer), out, count) == L.RESR_ERR_ARG     # training == 0
    out = (C.c_int64 * count)()
    for bad in (L.GeneratorDesc(n, h, w, 3, 3, 3, 1, L.RESR_F16, 1, 0, 0, 0), L.GeneratorDesc(0, h, w, 3, 3, 4, 1, L.RESR_F16, 1, 0, 0, 0),
                L.GeneratorDesc(n, 13, w, 3, 3, 2, 1, L.RESR_F32, 1, 0, 0, 0), L.GeneratorDesc(n, h, w, 3, 3, 4, 0, L.RESR_F16, 1, 0, 0, 0),
                L.GeneratorDesc(n, h, w, 3, 3, 4, 1, L.RESR_F16X2, 1, 0, 4096, 0)):                        # what the training entries refuse
        assert lib.resr_debug_generator_train_offsets(C.byref(bad), out, count) == L.RESR_ERR_ARG
    assert lib.resr_debug_generator_train_offsets(None, out, count) == L.RESR_ERR_ARG
