"""-m gpu: the compact generator's training graph judged PASS BY PASS on the device's own stored values (resr_compact_forward_train /
resr_compact_backward, csrc/compact.hip) -- as the host sequence wires the kernels: which buffer, which stride, which c_pad, which
slopes table, which 1 / lift.  tests/test_gpu_compact_train.py measures the distance to true float64 autograd, which in fast mode is
dominated by masks that flip (4e-2); here the reference is evaluated on the z_k and a_k the forward left in the workspace, so the
masks are the device's on both sides, the backward is one fixed linear map and only rounding is left.

The test drives the C ABI with buffers of its own -- resr_compact_train_pack_table, resr_pack_weights, a zero-filled state slot,
resr_compact_forward_train, resr_compact_backward with gx -- and reads the workspace through resr_debug_compact_train_offsets.  The
tensors of the workspace start as NaN patterns and the workspace lies between two guards: a buffer a pass did not fully write, or a
store beyond the workspace, shows.

  3a  num_conv 0 and 1, fast and strict: nothing the backward writes is overwritten before it returns (g_t; g0 = g_z of the top layer,
      g1 = g_z_0; g_xin), so EVERY pass is judged element by element with the rule of tests/compact_pass_ref.judge_passes
      (conv_ref.judge; A from the float32 evaluation of the reference on the same inputs, hu from f16's spacing; x_in, a_k, y and g_t
      bit for bit; pad channels and ReLU's dead elements exactly zero).  Every pass: bad == 0.  Strict: y is resr_compact_forward's bits.
  3b  the three deeper general cases, fast, all sizes gated: worst and median tensor of compact_grad_ref.error against the pinned
      float64 backward within 2 x the pinned f16 emulation's (compact_pass_ref.pinned_gate), whose own worst stays below 2e-3.
tests/test_compact_pass_ref.py shows on the CPU that the rule rejects planted faults and that the references are autograd.
Every row goes to <diag_dir>/test_gpu_compact_train_passes.json.

Measured on the MI355X (DESIGN, "Compact generator: training"): 3a, 248 judgements over the six runs and two precisions, bad = 0 in
all; largest |error| / bound per kind of pass, fast | strict: z_k 0.98 | 0.26, t 0.16 | 0.29, g_z_k 0.89 | 0.31, dslope_k 0.37 | 0.02,
dW 0.13 | 0.15, db 0.50 | 0.39, g_xin 0.94 | 0.34, gx 0.25 | 0.25 (an f16 store sits near 1 by construction: half an ulp is most of
its bound); lifts 1, 16, 32 and 2^18.  3b, worst tensor / median, native | yardstick: 2-x4-prelu-drawn-2x5x7 6.5e-4 / 3.7e-4 |
6.7e-4 / 3.7e-4; 3-x2-relu-2x18x33 6.5e-4 / 4.8e-4 | 6.8e-4 / 4.8e-4; 2-x1-prelu-drawn-1x37x53 5.7e-4 / 3.1e-4 | 5.5e-4 / 3.2e-4.
The fifteen tests take 3 s together, CPU references included.
"""
import ctypes as C
import json
import os

import pytest
import torch

from tests import compact_grad_ref as G
from tests import compact_pass_ref as P

pytestmark = pytest.mark.gpu
ROWS = {"passes": [], "pinned": {}}
GUARD = 256          # bytes on either side of the workspace
FILL = 0xFF          # f16 / f32 NaN patterns: a buffer that is read without having been written shows


@pytest.fixture(scope="module")
def L():
    import real_esrgan_pytorch_amd as pkg
    pkg._lib.lib()
    return pkg._lib


@pytest.fixture(scope="module", autouse=True)
def _write_diag(diag_dir):
    yield
    worst = {}
    for r in ROWS["passes"]:
        if r["kind"] not in ("bits", "zero"):
            key = f"{r['pass'].rstrip('0123456789').rstrip('_')}:{r['precision']}"
            worst[key] = max(worst.get(key, 0.0), r["ratio"])
    with open(os.path.join(diag_dir, "test_gpu_compact_train_passes.json"), "w") as f:
        json.dump({"worst_ratio_per_pass": worst, "pinned": ROWS["pinned"], "passes": ROWS["passes"]}, f, indent=1, sort_keys=True)


def _run(L, case, shift, fast):
    """One forward + backward of `case` through the C ABI on buffers of this test; returns (sd, x, gy, dev) with dev as
    compact_pass_ref.judge_passes takes it (gz: what g0 / g1 hold after the call -- the g_z of the LAST two layers the backward
    visited, which for num_conv <= 1 are all of them) and "y_inference" (strict: resr_compact_forward on the same weights)."""
    lib = L.lib()
    nc, s, act, _, n, (h, w), _ = case
    sd, x, gy = G.make_case(case)
    gy = gy * 2.0 ** shift
    dtype, tdt, es = (L.RESR_F16, torch.float16, 2) if fast else (L.RESR_F32, torch.float32, 4)
    d = L.CompactDesc(n, h, w, nc, s, {"prelu": L.COMPACT_PRELU, "leakyrelu": L.COMPACT_LRELU, "relu": L.COMPACT_RELU}[act], dtype, 0)
    ref = C.byref(d)
    flat = torch.cat([v.reshape(-1).float() for v in sd.values()]).cuda()        # named_parameters() order: the arena's
    assert flat.numel() == lib.resr_compact_param_count(ref)
    xd, gyd = x.cuda(), gy.cuda()
    st = L.stream_ptr(xd)

    def pack(table_fn, bytes_fn, what):
        host = L.fetch_pack_table(lambda out, cap: table_fn(ref, out, cap), what)
        table = L.upload_chunks(host, xd.device)
        packed = torch.zeros(bytes_fn(ref), dtype=torch.uint8, device="cuda")
        L.check(lib.resr_pack_weights(L.ptr(table), len(host), L.ptr(flat), L.ptr(packed), dtype, st), "resr_pack_weights")
        return packed

    packed = pack(lib.resr_compact_train_pack_table, lib.resr_compact_train_packed_bytes, "resr_compact_train_pack_table")
    nws = lib.resr_compact_train_workspace_bytes(ref)
    offs = (C.c_int64 * L.RESR_DEBUG_COMPACT_TRAIN_OFFSETS)()
    assert lib.resr_debug_compact_train_offsets(ref, offs, len(offs)) == len(offs)
    o_slot, o_xin, o_z, o_a, stride, o_t, o_gt, o_g0, o_g1, o_gxin = list(offs)
    px, c_t, cpl = n * h * w, 3 * s * s, (3 * s * s + 31) // 32 * 32
    assert o_gxin + px * 32 * es <= nws
    buf = torch.full((nws + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    ws = buf[GUARD:GUARD + nws]
    assert ws.data_ptr() % 256 == 0
    # the caller's one zero-fill: the state slot -- and, as the module does (_arena.Workspace has the reason), the scratch behind the
    # tensors (slope-gradient partials, weight-gradient slabs); the tensors themselves, x_in .. g_xin, start as NaN patterns
    assert lib.resr_compact_train_state_bytes(ref) <= o_xin
    ws[:o_xin] = 0
    ws[o_gxin + px * 32 * es:] = 0
    nan = float("nan")
    y = torch.full((n, 3, h * s, w * s), nan, device="cuda")
    grad = torch.full_like(flat, nan)
    gx = torch.full((n, 3, h, w), nan, device="cuda")
    L.check(lib.resr_compact_forward_train(ref, L.ptr(xd), L.ptr(flat), L.ptr(packed), L.ptr(ws), nws, L.ptr(y), st), "resr_compact_forward_train")
    L.check(lib.resr_compact_backward(ref, L.ptr(gyd), L.ptr(flat), L.ptr(packed), L.ptr(ws), nws, L.ptr(grad), L.ptr(gx), st), "resr_compact_backward")
    torch.cuda.synchronize()
    host = buf.cpu()
    assert torch.all(host[:GUARD] == FILL) and torch.all(host[GUARD + nws:] == FILL), "a pass wrote outside the workspace"
    body = host[GUARD:GUARD + nws]

    def nhwc(off, c):
        return body[off:off + px * c * es].view(tdt).view(n, h, w, c).permute(0, 3, 1, 2).contiguous()

    slot = body[o_slot:o_slot + 12].view(torch.int32).tolist()
    e = (slot[0] >> 23) & 0xFF                                                    # csrc/common.h grad_prescale: slot[0] = the bits of max |gy| 2^-6
    lift = 2.0 ** (127 - e) if fast and 0 < e < 127 else 1.0
    assert lift == (G.lift_of(gy) if fast else 1.0) and slot[1] == 0 and slot[2] == 0, (slot, lift)
    if not fast:
        assert slot[0] == 0                                                       # strict gets no lift and never touches the slot
    grad = grad.cpu()
    grads, at = {}, 0
    for name, v in sd.items():
        grads[name] = grad[at:at + v.numel()].view(v.shape)
        at += v.numel()
    held = [nhwc(o_g0, 64), nhwc(o_g1, 64)]            # the backward starts in g0 and swaps per layer: layer k's g_z lies in g[(nc - k) & 1],
    gz = [None] * (nc + 1)                             # and what survives the call is that of the two layers visited last, 1 and 0
    for k in range(min(nc, 1) + 1):
        gz[k] = held[(nc - k) & 1]
    dev = {"lift": lift, "x_in": nhwc(o_xin, 32), "z": [nhwc(o_z + k * stride, 64) for k in range(nc + 1)],
           "a": [nhwc(o_a + k * stride, 64) for k in range(nc + 1)], "t": body[o_t:o_t + px * c_t * 4].view(torch.float32).view(n, c_t, h, w).clone(),
           "y": y.cpu(), "g_t": nhwc(o_gt, cpl), "gz": gz, "g_xin": nhwc(o_gxin, 32), "grads": grads, "gx": gx.cpu()}
    if not fast:
        p_inf = pack(lib.resr_compact_pack_table, lib.resr_compact_packed_bytes, "resr_compact_pack_table")
        n_inf = lib.resr_compact_workspace_bytes(ref)
        ws_inf = torch.empty(n_inf, dtype=torch.uint8, device="cuda")
        y_inf = torch.full_like(y, nan)
        L.check(lib.resr_compact_forward(ref, L.ptr(xd), L.ptr(flat), L.ptr(p_inf), L.ptr(ws_inf), n_inf, L.ptr(y_inf), st), "resr_compact_forward")
        torch.cuda.synchronize()
        dev["y_inference"] = y_inf.cpu()
    return sd, x, gy, dev


@pytest.mark.parametrize("precision", ["fast", "strict"])
@pytest.mark.parametrize("run", P.RUNS_3A, ids=P.run_id)
def test_every_pass_on_the_device_s_own_values(L, run, precision):
    case, shift = run
    nc, s, act = case[:3]
    fast = precision == "fast"
    sd, x, gy, dev = _run(L, case, shift, fast)
    assert all(g is not None for g in dev["gz"])                                    # num_conv <= 1: every g_z is still there
    rows = P.judge_passes(dev, sd, x, gy, nc, s, act, fast)
    for r in rows:
        r.update(case=P.run_id(run), precision=precision, lift=dev["lift"])
        print(P.run_id(run), precision, "%-22s %-5s ratio %.3f bad %d allowance %.3e" % (r["pass"], r["kind"], r["ratio"], r["bad"], r["allowance"]))
    ROWS["passes"] += rows
    if not fast:
        assert torch.equal(dev["y"], dev["y_inference"])
    assert not P.bad_passes(rows), P.bad_passes(rows)


@pytest.mark.parametrize("case", P.CASES_3B, ids=G.case_id)
def test_deeper_graphs_end_to_end_with_the_masks_pinned(L, case):
    nc, s, act = case[:3]
    sd, x, gy, dev = _run(L, case, 0, True)
    grads = dict(dev["grads"])
    grads["x"] = dev["gx"]
    assert all(torch.isfinite(v).all() for v in grads.values())
    rec = P.pinned_gate(grads, sd, dev, gy, nc, s, act)
    ROWS["pinned"][G.case_id(case)] = rec
    print(G.case_id(case), "worst %.3e (yardstick %.3e) median %.3e (yardstick %.3e) %s" % (rec["worst"], rec["yardstick_worst"], rec["median"],
                                                                                          rec["yardstick_median"], rec["worst_tensor"]))
    assert rec["condition"], ("the pinned emulation itself is off on this seed: choose another", rec)
    assert rec["ok"], rec
