"""-m gpu: the RRDB generator's training step judged PASS BY PASS on the device's own stored values (resr_generator_forward with
training = 1, resr_generator_backward; csrc/generator.hip) -- as the host sequence wires the kernels: which workspace, which plane, which
sign plane, which fold, which ring slot, which 1 / lift.  tests/test_gpu_generator.py measures whole gradient tensors against float64
autograd, which in fast mode is dominated by masks that flip (4.6e-2 .. 1.25e-1); here every pass is judged on the tensors it READ, so
the masks are the device's on both sides and only that pass's rounding is left.

The test drives the C ABI with buffers of its own -- resr_generator_pack_table(backward = 1), resr_pack_weights, the zero-filled head of
resr_generator_chain_state_bytes, resr_generator_forward, resr_generator_backward with gx -- and reads the workspace through
resr_debug_generator_train_offsets.  Everything behind the head starts as a NaN pattern and the workspace lies between two guards: a
buffer a pass did not fully write, or a store beyond the workspace, shows.

  3a  n_blocks = 1, fast and strict: the forward keeps everything, the backward leaves everything but gA, which is written three times;
      RESR_DEBUG_STOP = 1, 2, 3 (each on a fresh forward + backward) shows it in each role, stop 4 shows gT3 before the add_inplace.
      EVERY pass is judged element by element with tests/generator_pass_ref.judge_passes (conv_ref.judge; A from the float32 evaluation
      of the reference on the same inputs, half an f16 ulp for an f16 store; layouts, the add and gx bit for bit; pad channels exactly
      zero; sign words = (stored > 0)).  Every pass: bad == 0.  Strict: y is an inference forward's bits.
  3b  n_blocks = 2, fast (the ring rotates past e): the forward judged pass by pass, the gradients gated end to end with the masks
      pinned: worst and median tensor (relative L2) against the pinned float64 backward within 2 x the pinned f16 yardstick's
      (generator_pass_ref.pinned_gate), whose own worst stays below 5e-3.
tests/test_generator_pass_ref.py shows on the CPU that the rule rejects thirteen planted wiring faults and that the references are autograd.
Every row goes to <diag_dir>/test_gpu_generator_passes.json.

Measured on the MI355X (DESIGN, "RRDB generator: training -- pass by pass"): 1438 judgements over the twelve 3a runs and 3b's two
forwards, bad = 0 in all; largest |error| / bound per kind of pass, fast | strict: the forward's f16 / f32 stores (conv1, o_k, conv5,
conv2 + skip, upsampling1, upsampling2, conv3) 0.99 | 0.44, y 0.38 | 0.32, the tail's backward-data passes 0.98 | 0.42, the pools 0.99 |
0.25, g_o_k 0.96 | 0.43, g_x 0.98 | 0.29, g_xin 0.96 | 0.29, dW 0.17 | 0.22, db 0.50 | 0.64 (an f16 store sits near 1 by construction:
half an ulp is most of its bound); lifts 1, 16, 32 and 2^19.  3b, worst tensor / median, native | yardstick: x4-2x5x7-b2 1.01e-3 /
6.7e-4 | 1.07e-3 / 6.9e-4; x4-1x9x33-b2 1.26e-3 / 7.1e-4 | 1.18e-3 / 7.0e-4.  The fourteen tests take 10 s together, CPU references
included.
"""
import ctypes as C
import json
import os

import pytest
import torch

from tests import generator_pass_ref as P

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
        if r["kind"] in ("f16", "f32"):
            name = r["pass"].split(".")[-1] if r["pass"].startswith("trunk.") else r["pass"]
            key = f"{name.split(' ')[0] if name.startswith(('dW', 'db')) else name}:{r['precision']}"
            worst[key] = max(worst.get(key, 0.0), r["ratio"])
    with open(os.path.join(diag_dir, "test_gpu_generator_passes.json"), "w") as f:
        json.dump({"worst_ratio_per_pass": worst, "judgements": len(ROWS["passes"]), "lifts": sorted({r["lift"] for r in ROWS["passes"]}),
                   "pinned": ROWS["pinned"], "passes": ROWS["passes"]}, f, indent=1, sort_keys=True)


class _Setup:
    """What the runs of one (case, cotangent, precision) share: the descriptor, the packed weights, the operands on the device."""

    def __init__(self, L, case, shift, fast):
        lib = L.lib()
        s, n, h, w, nb, _ = case
        self.L, self.case, self.fast = L, case, fast
        self.sd, self.x, gy = P.make_case(case)
        self.gy = gy * 2.0 ** shift
        self.dtype, self.tdt, self.es = (L.RESR_F16, torch.float16, 2) if fast else (L.RESR_F32, torch.float32, 4)
        self.d = L.GeneratorDesc(n, h, w, 3, 3, s, nb, self.dtype, 1, 0, 0, 0)
        ref = C.byref(self.d)
        self.flat = torch.cat([v.reshape(-1).float() for v in self.sd.values()]).cuda()      # conv1, the trunk, conv2 .. conv4: weight, bias
        assert self.flat.numel() == lib.resr_generator_param_count(ref)
        self.xd, self.gyd = self.x.cuda(), self.gy.cuda()
        self.st = L.stream_ptr(self.xd)
        host = L.fetch_pack_table(lambda out, cap: lib.resr_generator_pack_table(ref, 1, out, cap), "resr_generator_pack_table")
        table = L.upload_chunks(host, self.xd.device)
        self.packed = torch.zeros(lib.resr_generator_packed_bytes(ref, 1), dtype=torch.uint8, device="cuda")
        L.check(lib.resr_pack_weights(L.ptr(table), len(host), L.ptr(self.flat), L.ptr(self.packed), self.dtype, self.st), "resr_pack_weights")
        offs = (C.c_int64 * L.RESR_DEBUG_GENERATOR_TRAIN_OFFSETS)()
        assert lib.resr_debug_generator_train_offsets(ref, offs, len(offs)) == len(offs)
        self.offs = list(offs)

    def workspace(self, d):
        """A workspace of descriptor d between two guards: the head zero-filled, everything behind it a NaN pattern."""
        lib = self.L.lib()
        nws = lib.resr_generator_workspace_bytes(C.byref(d))
        head = lib.resr_generator_chain_state_bytes(C.byref(d))
        buf = torch.full((nws + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
        ws = buf[GUARD:GUARD + nws]
        assert ws.data_ptr() % 256 == 0 and 0 < head < nws
        ws[:head] = 0                                   # the caller's one zero-fill (include/resr.h): the chain state and the pre-scale slot
        return buf, ws, nws

    def run(self, stop=0):
        """One forward + backward on fresh buffers; returns the workspace's bytes on the host, y, the gradient arena, gx."""
        L, lib = self.L, self.L.lib()
        s, n, h, w, nb, _ = self.case
        ref = C.byref(self.d)
        buf, ws, nws = self.workspace(self.d)
        # ... and, as the module does (_arena.Workspace has the reason: the weight-gradient reduction looks at slab entries no launch
        # wrote when it decides whether a lifted pass overflowed), the slab scratch behind the tensors.  The tensors themselves, x_in ..
        # g_xin, the sign words and ymask included, start as NaN patterns.
        ws[self.offs[24]:] = 0
        nan = float("nan")
        y = torch.full((n, 3, h * s, w * s), nan, device="cuda")
        grad = torch.full_like(self.flat, nan)
        gx = torch.full((n, 3, h, w), nan, device="cuda")
        L.check(lib.resr_generator_forward(ref, L.ptr(self.xd), L.ptr(self.flat), L.ptr(self.packed), L.ptr(ws), nws, L.ptr(y), self.st), "resr_generator_forward")
        L.check(lib.resr_generator_backward(ref, L.ptr(self.gyd), L.ptr(self.flat), L.ptr(self.packed), L.ptr(ws), nws, L.ptr(grad), L.ptr(gx), self.st, None, 0),
                "resr_generator_backward")
        torch.cuda.synchronize()
        host = buf.cpu()
        assert torch.all(host[:GUARD] == FILL) and torch.all(host[GUARD + nws:] == FILL), f"a pass wrote outside the workspace (stop {stop})"
        return host[GUARD:GUARD + nws], y.cpu(), grad.cpu(), gx.cpu()

    def inference(self):
        """y of an inference forward (training = 0, the rotating-workspace plan) on the same packed weights."""
        L, lib = self.L, self.L.lib()
        s, n, h, w, nb, _ = self.case
        d = L.GeneratorDesc(n, h, w, 3, 3, s, nb, self.dtype, 0, 0, 0, 0)
        buf, ws, nws = self.workspace(d)
        y = torch.full((n, 3, h * s, w * s), float("nan"), device="cuda")
        L.check(lib.resr_generator_forward(C.byref(d), L.ptr(self.xd), L.ptr(self.flat), L.ptr(self.packed), L.ptr(ws), nws, L.ptr(y), self.st), "resr_generator_forward")
        torch.cuda.synchronize()
        host = buf.cpu()
        assert torch.all(host[:GUARD] == FILL) and torch.all(host[GUARD + nws:] == FILL)
        return y.cpu()

    # ---- reading a workspace: the tensor formats of include/resr_debug.h, nothing of the kernels' index arithmetic ----
    def geometry(self):
        s, n, h, w, nb, _ = self.case
        r = P.unshuffle_of(s)
        return n, h // r, w // r, (3 * r * r + 31) // 32 * 32

    def nhwc(self, body, off, c, hh, ww):
        n = self.case[1]
        return body[off:off + n * hh * ww * c * self.es].view(self.tdt).view(n, hh, ww, c).permute(0, 3, 1, 2).contiguous()

    def planar(self, body, off, planes, hh, ww):
        """[planes][N,hh,ww,32] -> [N, 32 planes, hh, ww]"""
        step = self.case[1] * hh * ww * 32 * self.es
        return torch.cat([self.nhwc(body, off + q * step, 32, hh, ww) for q in range(planes)], dim=1)

    def words(self, body, off, m, hh, ww):
        """uint32 [N,hh,ww][m] sign words -> bool [N, 32 m, hh, ww]: bit c of word j = channel 32 j + c"""
        n = self.case[1]
        wd = body[off:off + n * hh * ww * m * 4].view(torch.int32).view(n, hh, ww, m, 1)
        bits = (wd >> torch.arange(32, dtype=torch.int32)) & 1
        return bits.view(n, hh, ww, 32 * m).permute(0, 3, 1, 2).bool().contiguous()

    def forward_values(self, body, y):
        s, n, _, _, nb, _ = self.case
        _, h, w, ci_pad = self.geometry()
        (o_slot, o_xin, o_ws, ws_stride, o_bits, bits_stride, o_bu2, o_bc3, o_trunk, o_feat, o_u1, o_u2, o_c3, o_ymask) = self.offs[:14]
        px = n * h * w
        sign = [torch.cat([self.words(body, o_bits + r * bits_stride + k * px * 4, 1, h, w) for k in range(4)], dim=1) for r in range(3 * nb)]
        return {"x_in": self.nhwc(body, o_xin, ci_pad, h, w), "ws": [self.planar(body, o_ws + r * ws_stride, 6, h, w) for r in range(3 * nb)], "sign": sign,
                "trunk_out": self.planar(body, o_trunk, 2, h, w), "feat": self.planar(body, o_feat, 2, h, w), "u1": self.planar(body, o_u1, 2, 2 * h, 2 * w),
                "u2": self.planar(body, o_u2, 2, 4 * h, 4 * w), "c3": self.planar(body, o_c3, 2, 4 * h, 4 * w),
                "sign_u2": self.words(body, o_bu2, 2, 4 * h, 4 * w), "sign_c3": self.words(body, o_bc3, 2, 4 * h, 4 * w),
                "y": y, "ymask": body[o_ymask:o_ymask + 16 * px * 3].view(n, 3, 4 * h, 4 * w).clone()}

    def named_grads(self, grad):
        grads, at = {}, 0
        for name, v in self.sd.items():
            grads[name] = grad[at:at + v.numel()].view(v.shape)
            at += v.numel()
        return grads


def _slot(su, body):
    return body[su.offs[0]:su.offs[0] + 12].view(torch.int32).tolist()


@pytest.mark.parametrize("precision", ["fast", "strict"])
@pytest.mark.parametrize("run", P.RUNS_3A, ids=P.run_id)
def test_every_pass_on_the_device_s_own_values(L, run, precision, monkeypatch):
    case, shift = run
    s, nb = case[0], case[4]
    fast = precision == "fast"
    su = _Setup(L, case, shift, fast)
    _, h, w, ci_pad = su.geometry()
    o_g4, o_gA, o_gB, o_gM1, o_gF, o_gT, gT_stride, o_gS, gS_stride, o_gxin = su.offs[14:24]
    monkeypatch.delenv("RESR_DEBUG_STOP", raising=False)
    body, y, grad, gx = su.run()
    dev = su.forward_values(body, y)
    ring = lambda b, i: su.planar(b, o_gT + i * gT_stride, 2, h, w)
    slab = lambda b, i: su.planar(b, o_gS + i * gS_stride, 4, h, w)
    # one RRDB: the ring starts at slot 0 with conv2's backward-data result (e), the three blocks write slots 1, 2, 3 and never meet e
    dev.update(slot=_slot(su, body), g4=su.nhwc(body, o_g4, 32, 4 * h, 4 * w), gB=su.planar(body, o_gB, 2, 4 * h, 4 * w),
               gM1=su.planar(body, o_gM1, 2, 2 * h, 2 * w), gF=su.planar(body, o_gF, 2, h, w),
               gin=[ring(body, 2), ring(body, 1), ring(body, 0)], gsum=ring(body, 3),
               gS=[{4 - q: slab(body, r)[:, 32 * q:32 * q + 32] for q in range(4)} for r in range(3)],     # planes g_o4 | g_o3 | g_o2 | g_o1
               g_xin=su.nhwc(body, o_gxin, ci_pad, h, w), grads=su.named_grads(grad), gx=gx)
    # gA in its three roles and gT3 before the add: RESR_DEBUG_STOP is read per call and returns after the section named
    stopped = {}
    for stop in (1, 2, 3, 4):
        monkeypatch.setenv("RESR_DEBUG_STOP", str(stop))
        stopped[stop] = su.run(stop)[0]
    monkeypatch.delenv("RESR_DEBUG_STOP")
    dev.update(gA1=su.planar(stopped[1], o_gA, 2, 4 * h, 4 * w), gA2=su.planar(stopped[2], o_gA, 2, 4 * h, 4 * w),
               gA3=su.planar(stopped[3], o_gA, 2, 2 * h, 2 * w), g_out=ring(stopped[4], 3))
    # the runs are one computation: what a stopped run left behind its stop is what the complete run left there
    assert torch.equal(su.planar(stopped[1], o_gB, 2, 4 * h, 4 * w).view(torch.uint8), dev["gB"].view(torch.uint8))
    assert torch.equal(su.planar(stopped[2], o_gM1, 2, 2 * h, 2 * w).view(torch.uint8), dev["gM1"].view(torch.uint8))
    assert torch.equal(su.planar(stopped[3], o_gF, 2, h, w).view(torch.uint8), dev["gF"].view(torch.uint8))
    assert torch.equal(ring(stopped[4], 2).view(torch.uint8), dev["gin"][0].view(torch.uint8))
    if not fast:
        dev["y_inference"] = su.inference()
    rows = P.judge_passes(dev, su.sd, su.x, su.gy, s, nb, fast)
    lift = P.lift_of_slot(dev["slot"][0])
    for r in rows:
        r.update(case=P.run_id(run), precision=precision, lift=lift)
        print(P.run_id(run), precision, "%-28s %-5s ratio %.3f bad %d allowance %.3e worst %d" % (r["pass"], r["kind"], r["ratio"], r["bad"], r["allowance"], r["worst"]))
    ROWS["passes"] += rows
    if fast:
        assert (lift == 1.0) if shift == 7 else (lift >= 16.0 * 2.0 ** -shift)
    else:
        assert lift == 1.0 and torch.equal(dev["y"].view(torch.int32), dev["y_inference"].view(torch.int32))
    assert all(r["both_values"] for r in rows if "both_values" in r), [r["pass"] for r in rows if r.get("both_values") is False]
    assert not P.bad_passes(rows), P.bad_passes(rows)


@pytest.mark.parametrize("case", P.CASES_3B, ids=P.case_id)
def test_two_rrdbs_forward_by_pass_and_gradients_with_the_masks_pinned(L, case, monkeypatch):
    s, nb = case[0], case[4]
    monkeypatch.delenv("RESR_DEBUG_STOP", raising=False)
    su = _Setup(L, case, 0, True)
    body, y, grad, gx = su.run()
    dev = su.forward_values(body, y)
    rows = P.judge_passes(dev, su.sd, su.x, su.gy, s, nb, True, backward=False)
    lift = P.lift_of_slot(_slot(su, body)[0])
    for r in rows:
        r.update(case=P.case_id(case), precision="fast", lift=lift)
        print(P.case_id(case), "%-28s %-5s ratio %.3f bad %d allowance %.3e worst %d" % (r["pass"], r["kind"], r["ratio"], r["bad"], r["allowance"], r["worst"]))
    ROWS["passes"] += rows
    assert all(r["both_values"] for r in rows if "both_values" in r)
    assert not P.bad_passes(rows), P.bad_passes(rows)
    grads = su.named_grads(grad)
    grads["x"] = gx
    assert all(torch.isfinite(v).all() for v in grads.values())
    rec = P.pinned_gate(grads, su.sd, dev, su.gy, s, nb)
    ROWS["pinned"][P.case_id(case)] = rec
    print(P.case_id(case), "worst %.3e (yardstick %.3e) median %.3e (yardstick %.3e) %s" % (rec["worst"], rec["yardstick_worst"], rec["median"],
                                                                                          rec["yardstick_median"], rec["worst_tensor"]))
    assert rec["condition"], ("the pinned yardstick itself is off on this seed: choose another", rec)
    assert rec["ok"], rec
