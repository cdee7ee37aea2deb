"""-m gpu: training the compact generator natively (SRVGGNetCompact(trainable=True): resr_compact_forward_train /
resr_compact_backward, csrc/compact.hip + compact_train.hip) against the CPU evaluators of tests/compact_grad_ref.py.

Error of a tensor: max |g - g64| / max |g64| against float64 autograd; a case is judged on its worst tensor and on the median over its
tensors (every parameter, and x).  The gates come from the references' own errors on the same case, never from the code under test:
  strict           <= 4 x the float32 evaluator's error: two fp32 chains that differ in summation order.  The test also asserts that
                   the float32 evaluator stays below 1e-5 (a seed where fp32 itself flips a mask would be replaced, not gated wider).
  fast, identity   (PReLU slopes all 1: linear net, no mask can flip) <= 2 x the f16 emulation's error.
  fast, general    <= 2 x the emulation's, on cases of at least 37 x 53 pixels only: under a dense random cotangent the error is the
                   mask flips, the native pass flips another subset than the emulation, and the two counts agree within 2 only when
                   there are many.  The smaller general cases are measured and recorded, not gated.  The emulation's own worst
                   tensor must stay below 0.1 wherever it gates.
  training forward strict: the bits of the inference forward; fast: at most 2 x the inference forward's distance from float64 (a
                   negative activation is rounded twice).
Every figure goes to <diag_dir>/test_gpu_compact_train.json.

Measured on the MI355X (worst over the cases, worst tensor / median; DESIGN, "Compact generator: training"): strict 1.4e-6 / 6.5e-7
against float32's 1.8e-6 / 9.1e-7, the largest ratio on one case 2.5 / 2.0; fast with identity slopes 1.4e-3 / 4.8e-4 and general at
37 x 53 4.0e-2 / 3.1e-2, both within 1 % of the emulation; the smaller general cases 5.9e-2 / 2.8e-2 (the emulation: the same).  The fast
training forward sits at 0.93-1.06 x the inference forward's distance from float64 (worst 1.4e-4).

The unpinned general cases stay here as what they are: the distance of a fast-mode step to TRUE autograd, masks that flip included.
They cannot see a fault that fits inside one tensor's 4e-2.  The sharp judgement is tests/test_gpu_compact_train_passes.py: every pass
of the same graph on the z_k and a_k the device itself stored, element by element, and the deeper graphs end to end with the masks
pinned, within 2 x an emulation that sits at 7e-4 -- the small general cases included.
"""
import ctypes as C
import functools
import json
import os

import pytest
import torch

from tests import compact_grad_ref as G

pytestmark = pytest.mark.gpu
ROWS = {}


@pytest.fixture(scope="module", autouse=True)
def _write_diag(diag_dir):
    yield
    worst = {}
    for r in ROWS.values():
        w = worst.setdefault(r["precision"], {"worst": 0.0, "median": 0.0, "forward": 0.0})
        w["worst"], w["median"], w["forward"] = max(w["worst"], r["worst"]), max(w["median"], r["median"]), max(w["forward"], r["forward_train"])
    with open(os.path.join(diag_dir, "test_gpu_compact_train.json"), "w") as f:
        json.dump({"worst_per_mode": worst, "cases": ROWS}, f, indent=1, sort_keys=True)


@functools.lru_cache(maxsize=None)
def _refs(i):
    """The three CPU evaluations of case i, computed once and shared."""
    case = G.CASES[i]
    sd, x, gy = G.make_case(case)
    nc, s, act = case[:3]
    return {kind: G.evaluate(kind, sd, x, gy, nc, s, act) for kind in ("f64", "f32", "emu16")}


def _model(case, precision, trainable=True):
    import real_esrgan_pytorch_amd as R
    nc, s, act = case[:3]
    sd, x, gy = G.make_case(case)
    m = R.SRVGGNetCompact(3, 3, 64, nc, s, act, precision=precision, trainable=trainable)
    m.load_state_dict(sd)
    return m.cuda(), x.cuda(), gy.cuda()


def _grads(m, x, gy, x_grad=True):
    """One forward + backward from cleared gradients: (y, {name: grad} with "x")."""
    m.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(x_grad)
    y = m(xi)
    y.backward(gy)
    out = {n: (None if p.grad is None else p.grad.clone()) for n, p in m.named_parameters()}
    out["x"] = None if xi.grad is None else xi.grad.clone()
    torch.cuda.synchronize()
    return y.detach(), out


def _same_bits(a, b):
    return set(a) == set(b) and all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in a)


def _large(case):
    return case[5][0] * case[5][1] >= 37 * 53


@pytest.mark.parametrize("precision", ["strict", "fast"])
@pytest.mark.parametrize("i", range(len(G.CASES)), ids=[G.case_id(c) for c in G.CASES])
def test_gradients_and_training_forward(i, precision):
    case = G.CASES[i]
    refs = _refs(i)
    y64, g64 = refs["f64"]
    m, x, gy = _model(case, precision)
    y, g = _grads(m, x, gy)
    with torch.no_grad():
        y_inf = m(x)
    assert y.shape == y64.shape and y.dtype == torch.float32 and all(g[k] is not None and g[k].shape == g64[k].shape for k in g64)
    errs = G.errors(g, g64)
    worst, median = G.worst_median(errs)
    kind = "f32" if precision == "strict" else "emu16"
    ref_worst, ref_median = G.worst_median(G.errors(refs[kind][1], g64))
    factor = 4.0 if precision == "strict" else 2.0
    gated = precision == "strict" or case[3] == "identity" or _large(case)
    fwd, fwd_inf = G.error(y, y64), G.error(y_inf, y64)
    ROWS[f"{G.case_id(case)}:{precision}"] = dict(precision=precision, worst=worst, median=median, reference=kind, ref_worst=ref_worst,
                                                  ref_median=ref_median, factor=factor, gated=gated, forward_train=fwd, forward_inference=fwd_inf,
                                                  worst_tensor=max(errs, key=errs.get))
    print(G.case_id(case), precision, "worst %.3e (ref %.3e) median %.3e (ref %.3e) forward %.3e (inference %.3e)" % (worst, ref_worst, median, ref_median, fwd, fwd_inf))
    if precision == "strict":
        assert ref_worst < 1e-5, ("the float32 evaluator itself flips a mask on this seed: choose another", ref_worst)
        assert torch.equal(y, y_inf)
    else:
        assert fwd <= 2.0 * fwd_inf, (fwd, fwd_inf)
    if gated:
        if precision == "fast":
            assert ref_worst < 0.1, ("the emulation itself is off", ref_worst)
        assert worst <= factor * ref_worst, (worst, ref_worst, errs)
        assert median <= factor * ref_median, (median, ref_median, errs)


@pytest.mark.parametrize("i", [0, 3], ids=[G.case_id(G.CASES[0]), G.case_id(G.CASES[3])])
def test_fast_gradients_do_not_depend_on_the_loss_scale(i):
    m, x, gy = _model(G.CASES[i], "fast")
    assert gy.abs().max() < 2.0 ** 6
    _, a = _grads(m, x, gy)
    _, b = _grads(m, x, gy * 2.0 ** -12)
    assert all(torch.equal(a[k], b[k] * 2.0 ** 12) for k in a), [k for k in a if not torch.equal(a[k], b[k] * 2.0 ** 12)]


@pytest.mark.parametrize("precision", ["strict", "fast"])
def test_backward_is_deterministic(precision):
    m, x, gy = _model(G.CASES[1], precision)
    ya, a = _grads(m, x, gy)
    yb, b = _grads(m, x, gy)
    assert torch.equal(ya, yb) and _same_bits(a, b)


def test_autograd_semantics():
    import real_esrgan_pytorch_amd as R
    L = R._lib
    case = G.CASES[0]
    m, x, gy = _model(case, "strict")
    _, single = _grads(m, x, gy)
    params = dict(m.named_parameters())

    # two backward calls without zero_grad leave the sum
    m.zero_grad(set_to_none=True)
    for _ in range(2):
        m(x).backward(gy)
    assert all(torch.equal(p.grad, single[n] + single[n]) for n, p in params.items())

    # two live graphs, the backwards in either order: each matches its own single-graph gradients
    x2, gy2 = torch.flip(x, dims=[3]).contiguous(), torch.flip(gy, dims=[2]).contiguous()
    _, single2 = _grads(m, x2, gy2)
    for first in (0, 1):
        m.zero_grad(set_to_none=True)
        xs = [x.clone().requires_grad_(), x2.clone().requires_grad_()]
        ys = [m(xs[0]), m(xs[1])]
        assert len({id(ws) for pool in m._train_workspaces.values() for ws in pool if ws.busy}) == 2    # a workspace each
        got = {}
        for k in (first, 1 - first):
            m.zero_grad(set_to_none=True)
            ys[k].backward(gy if k == 0 else gy2)
            got[k] = {n: p.grad.clone() for n, p in params.items()}
            got[k]["x"] = xs[k].grad.clone()
        assert _same_bits(got[0], single) and _same_bits(got[1], single2)
        assert not any(ws.busy for pool in m._train_workspaces.values() for ws in pool)

    # a second backward through one graph is refused, not computed from a workspace another graph may own by then
    y = m(x)
    y.backward(gy, retain_graph=True)
    with pytest.raises(RuntimeError, match="backward has run already"):
        y.backward(gy)

    # parameters that do not require grad get none, the others are unchanged
    frozen = [n for n in params if n.startswith("body.2.") or n.endswith(".1.weight")]
    assert len(frozen) == 3
    for n in frozen:
        params[n].requires_grad_(False)
    _, part = _grads(m, x, gy)
    assert all(part[n] is None for n in frozen)
    assert all(torch.equal(part[n], single[n]) for n in single if n not in frozen)
    for n in frozen:
        params[n].requires_grad_(True)

    # x does not require grad: no gx, and the backward-data launch of conv 0 (a convolution: kernel id below 30000) is skipped
    _, nox = _grads(m, x, gy, x_grad=False)
    assert nox["x"] is None and all(torch.equal(nox[n], single[n]) for n in params)

    def run(x_grad):
        xi = x.clone().requires_grad_(x_grad)
        y = m(xi)
        return lambda: y.backward(gy)
    ids_x = _prof_counts_once(L, run(True))
    ids_nox = _prof_counts_once(L, run(False))
    convs = lambda ids: sum(1 for k in ids if k < 30000)
    nc = case[0]
    assert convs(ids_nox) == nc + 1 and convs(ids_x) == nc + 2, (ids_x, ids_nox)
    assert sum(1 for k in ids_x if 32300 <= k < 32400) == 1 and not any(32300 <= k < 32400 for k in ids_nox)    # the residual's adjoint
    assert sum(1 for k in ids_nox if k in (32100, 32101)) == nc + 1

    # under no_grad a trainable model is the inference model, bit for bit; the frame entries keep raising under grad mode
    twin, _, _ = _model(case, "strict", trainable=False)
    frames = (x.permute(0, 2, 3, 1) * 255).to(torch.uint8).contiguous()
    with torch.no_grad():
        assert torch.equal(m(x), twin(x))
        assert torch.equal(m.forward_u8(frames), twin.forward_u8(frames))
    with pytest.raises(RuntimeError, match="backward"):
        m.forward_u8(frames)
    with pytest.raises(RuntimeError, match="backward"):
        twin(x)                                            # without the flag: the guard of before
    for p in m.parameters():
        p.requires_grad_(False)
    y = m(x)                                               # nothing requires grad: the inference path, no graph
    with torch.no_grad():
        assert not y.requires_grad and torch.equal(y, twin(x))


def _prof_counts_once(L, fn):
    """kernel ids of the instrumented launches of ONE call of fn()."""
    lib = L.lib()
    buf = (L.ProfEntry * 256)()
    lib.resr_profile_begin()
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        n = int(lib.resr_profile_end(C.cast(buf, C.c_void_p), 256))
    assert 0 <= n <= 256
    return [buf[k].kernel_id for k in range(n)]


def test_steps_train_the_compact_generator():
    """fast, with a GradScaler: three RealESRNet steps with EMA, then one RealESRGAN step with the project's Discriminator."""
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd.train import RealESRGANStep, RealESRNetStep
    torch.manual_seed(11)
    g = R.SRVGGNetCompact(num_conv=2, upscale=4, act_type="prelu", precision="fast", trainable=True).cuda().train()
    gen = torch.Generator(device="cuda").manual_seed(3)
    hr = torch.rand(4, 3, 32, 32, device="cuda", generator=gen)
    lr = torch.nn.functional.interpolate(hr, scale_factor=0.25, mode="area")
    ema = R.EMA(g, 0.9)
    ema.register()
    opt = torch.optim.Adam(g.parameters(), 1e-3, (0.9, 0.99))
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    before = {n: p.detach().clone() for n, p in g.named_parameters()}
    shadow = {n: v.clone() for n, v in ema.shadow.items()}
    step = RealESRNetStep(g, ema, opt, scaler, None)
    losses = [step(hr, lr) for _ in range(3)]
    torch.cuda.synchronize()
    assert all(torch.isfinite(v) for v in losses)
    assert scaler.get_scale() == 1024.0                                            # no step was skipped
    assert all(not torch.equal(p.detach(), before[n]) for n, p in g.named_parameters()), [n for n, p in g.named_parameters() if torch.equal(p.detach(), before[n])]
    assert all(not torch.equal(ema.shadow[n], shadow[n]) for n in shadow)

    d = R.Discriminator().cuda().train()
    d_opt = torch.optim.Adam(d.parameters(), 1e-3, (0.9, 0.99))
    g_before = g.flat_parameters().clone()
    d_before = d.flat_parameters().clone()
    out = RealESRGANStep(g, d, ema, opt, d_opt, scaler, None)(hr, lr)
    torch.cuda.synchronize()
    assert set(out) == {"pixel_loss", "adversarial_loss", "d_loss_hr", "d_loss_sr"} and all(torch.isfinite(v) for v in out.values())
    assert not torch.equal(g.flat_parameters(), g_before) and not torch.equal(d.flat_parameters(), d_before)


def test_no_torch_fallback():
    m, x, gy = _model(G.CASES[0], "fast")
    _grads(m, x, gy)
    m.zero_grad(set_to_none=True)        # (a .grad left in place would be accumulated into: autograd's own aten::add_)
    xi = x.clone().requires_grad_()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        y = m(xi)
        y.backward(gy)
        torch.cuda.synchronize()
    names = {e.key for e in prof.key_averages()}
    banned = {"aten::conv2d", "aten::convolution", "aten::_convolution", "aten::prelu", "aten::_prelu_kernel", "aten::pixel_shuffle",
              "aten::upsample_nearest2d", "aten::add", "aten::add_", "aten::leaky_relu", "aten::relu",
              "aten::convolution_backward", "aten::_prelu_kernel_backward", "aten::prelu_backward", "aten::leaky_relu_backward",
              "aten::pixel_shuffle_backward", "aten::pixel_unshuffle", "aten::threshold_backward", "aten::upsample_nearest2d_backward"}
    assert not names & banned, names & banned
    assert xi.grad is not None and all(p.grad is not None for p in m.parameters())


def test_c_abi_refusals_launch_nothing():
    import real_esrgan_pytorch_amd as R
    L = R._lib
    lib = L.lib()
    d = L.CompactDesc(1, 9, 11, 2, 2, L.COMPACT_PRELU, L.RESR_F16, 0)
    nparam = lib.resr_compact_param_count(C.byref(d))
    nws = lib.resr_compact_train_workspace_bytes(C.byref(d))
    params = torch.zeros(nparam, device="cuda")
    packed = torch.zeros(lib.resr_compact_train_packed_bytes(C.byref(d)), dtype=torch.uint8, device="cuda")
    ws = torch.zeros(nws, dtype=torch.uint8, device="cuda")
    x = torch.zeros(1, 3, 9, 11, device="cuda")
    y = torch.full((1, 3, 18, 22), 7.0, device="cuda")
    grad = torch.full((nparam,), 7.0, device="cuda")
    st = L.stream_ptr(x)
    p = L.ptr
    x2 = L.CompactDesc(1, 9, 11, 2, 2, L.COMPACT_PRELU, L.RESR_F16X2, 0)
    bad = L.CompactDesc(1, 9, 11, 2, 5, L.COMPACT_PRELU, L.RESR_F16, 0)

    def calls():
        assert lib.resr_compact_forward_train(C.byref(d), p(x), p(params), p(packed), p(ws), nws - 1, p(y), st) == L.RESR_ERR_WORKSPACE
        assert lib.resr_compact_backward(C.byref(d), p(y), p(params), p(packed), p(ws), nws - 1, p(grad), None, st) == L.RESR_ERR_WORKSPACE
        assert lib.resr_compact_backward(C.byref(d), None, p(params), p(packed), p(ws), nws, p(grad), None, st) == L.RESR_ERR_ARG
        assert lib.resr_compact_backward(C.byref(d), p(y), p(params), p(packed), p(ws), nws, None, None, st) == L.RESR_ERR_ARG
        assert lib.resr_compact_forward_train(C.byref(d), None, p(params), p(packed), p(ws), nws, p(y), st) == L.RESR_ERR_ARG
        for dd in (x2, bad):
            assert lib.resr_compact_forward_train(C.byref(dd), p(x), p(params), p(packed), p(ws), nws * 4, p(y), st) == L.RESR_ERR_ARG
            assert lib.resr_compact_backward(C.byref(dd), p(y), p(params), p(packed), p(ws), nws * 4, p(grad), None, st) == L.RESR_ERR_ARG
        assert lib.resr_compact_backward(C.byref(x2), p(y), p(params), p(packed), p(ws), nws * 4, p(grad), None, st) == L.RESR_ERR_ARG
        assert b"exact16 training is not built" in lib.resr_last_error()
    assert _prof_counts_once(L, calls) == []
    assert torch.all(y == 7.0) and torch.all(grad == 7.0) and not torch.any(ws)
