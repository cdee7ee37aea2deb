"""-m gpu: the output-parity GAN step -- the discriminator and ContentLoss with f16_backward=True (exact16's forward, fast mode's
f16 backward pass on the hi halves of the saved activations), the generator on x2_plan 2401.  Forward bit-identical to exact16,
gradients no farther from the all-pairs exact16 pass than fast mode's, loss-scale independent, the pooled workspace reusable, the
golden RealESRGAN step inside the output tolerance, and the graph replay equal to the eager step.  Measured values go to diag_dir."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
NODES = ["features.2", "features.7", "features.16", "features.25", "features.34"]
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
CW = [0.1, 0.1, 1.0, 1.0, 1.0]                                  # config.py content_weight
MODES = {"exact16": ("exact16", False), "parity": ("exact16", True), "fast": ("fast", None)}


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _disc(mode, sd):
    import real_esrgan_pytorch_amd as R
    precision, f16 = MODES[mode]
    d = R.Discriminator(precision=precision, f16_backward=f16)
    d.load_state_dict(sd)
    return d.cuda().train()


def _three_calls(d, x, gw, scale=256.0):
    """train_realesrgan.py:479,500,508: three training-mode calls on one module (u / v move per call)."""
    out = []
    for _ in range(3):
        d.zero_grad(set_to_none=True)
        xt = x.clone().requires_grad_(True)
        y = d(xt)
        (y * gw).sum().mul(scale).backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach() / scale for n, p in d.named_parameters()}
        grads["gx"] = xt.grad.detach() / scale
        out.append((y.detach().clone(), d.flat_uv().detach().clone(), grads))
    return out


def _golden(name):
    z = np.load(os.path.join(G, name + ".npz"))
    return {k: torch.from_numpy(z[k]) if z[k].dtype.kind == "f" else z[k] for k in z.files}


def _content(mode, like=None):
    import real_esrgan_pytorch_amd as R
    precision, f16 = MODES[mode]
    torch.manual_seed(11)
    cl = R.ContentLoss(NODES, MEAN, STD, precision=precision, detached=False, f16_backward=f16)
    if like is not None:
        cl.load_state_dict(like.state_dict())
    return cl.cuda()


def _content_run(cl, sr, hr, scale=1024.0):
    srd = sr.clone().requires_grad_(True)
    losses = cl(srd, hr)
    (sum(w * l for w, l in zip(CW, losses)) * scale).backward()
    torch.cuda.synchronize()
    return torch.stack([l.detach() for l in losses]), srd.grad.detach() / scale


def test_forward_is_exact16_bit_for_bit():
    """Logits and the updated u / v of three training calls (each followed by its backward pass, which repacks the workspace's
    weights in f16) equal exact16's bit for bit; so do the five ContentLoss values."""
    from oracle import model_ref as M
    g = _golden("discriminator")
    sd = M.init_discriminator_state(int(g["seed"]))
    x, gw = g["x"].cuda(), g["gw"].cuda()
    ref = _three_calls(_disc("exact16", sd), x, gw)
    got = _three_calls(_disc("parity", sd), x, gw)
    for call, ((ya, uva, _), (yb, uvb, _)) in enumerate(zip(ref, got)):
        assert torch.equal(ya, yb), call
        assert torch.equal(uva, uvb), call
    gen = torch.Generator().manual_seed(5)
    sr, hr = torch.rand(2, 3, 64, 48, generator=gen).cuda(), torch.rand(2, 3, 64, 48, generator=gen).cuda()
    ce = _content("exact16")
    la, _ = _content_run(ce, sr, hr)
    lb, _ = _content_run(_content("parity", ce), sr, hr)
    assert torch.equal(la, lb)


@pytest.mark.parametrize("golden", ["discriminator_allgrads_240", "discriminator_allgrads_243"])
def test_gradients_no_farther_than_fast_mode(golden, diag_dir):
    """Every discriminator gradient tensor and gx of the three calls against the all-pairs exact16 pass: the worst and the median
    distance of the output-parity backward are no larger than fast mode's on the same inputs.  Measured (39 tensors): seed 240
    worst 9.0e-4 / median 7.1e-4, seed 243 1.8e-3 / 5.5e-4; fast mode 3.9-4.3e-2 / 2.0-2.5e-2.  Gates 1.5 x: 2.7e-3 / 1.1e-3."""
    from oracle import model_ref as M
    g = _golden(golden)
    sd = M.init_discriminator_state(int(g["seed"]))
    x, gw = g["x"].cuda(), g["gw"].cuda()
    runs = {m: _three_calls(_disc(m, sd), x, gw) for m in MODES}
    dist = {m: [] for m in ("parity", "fast")}
    for call in range(3):
        ref = runs["exact16"][call][2]
        for m in dist:
            dist[m] += [_rel(runs[m][call][2][k], ref[k]) for k in ref]
    rep = {m: {"worst": max(v), "median": float(np.median(v)), "n": len(v)} for m, v in dist.items()}
    with open(os.path.join(diag_dir, f"parity_gan_disc_grads_{golden[-3:]}.json"), "w") as f:
        json.dump(rep, f, indent=1)
    print(golden, rep)
    assert rep["parity"]["worst"] <= rep["fast"]["worst"], rep
    assert rep["parity"]["median"] <= rep["fast"]["median"], rep
    assert rep["parity"]["worst"] < 2.7e-3 and rep["parity"]["median"] < 1.1e-3, rep


def test_content_loss_input_gradient_no_farther_than_fast_mode(diag_dir):
    """ContentLoss(detached=False): d(weighted five L1 terms) / d(sr) against the exact16 pass.  Measured 1.1e-3 (fast mode 9.0e-2:
    its forward moves features across the L1 terms' sign ties and the ReLU masks); gate 1.5 x: 1.7e-3."""
    gen = torch.Generator().manual_seed(6)
    sr, hr = torch.rand(2, 3, 64, 48, generator=gen).cuda(), torch.rand(2, 3, 64, 48, generator=gen).cuda()
    ce = _content("exact16")
    _, g_ref = _content_run(ce, sr, hr)
    _, g_par = _content_run(_content("parity", ce), sr, hr)
    _, g_fast = _content_run(_content("fast", ce), sr, hr)
    rep = {"parity": _rel(g_par, g_ref), "fast": _rel(g_fast, g_ref)}
    with open(os.path.join(diag_dir, "parity_gan_content_gx.json"), "w") as f:
        json.dump(rep, f, indent=1)
    print(rep)
    assert rep["parity"] <= rep["fast"], rep
    assert rep["parity"] < 1.7e-3, rep


def test_backward_does_not_depend_on_the_loss_scale():
    """The gradient lift of the native pass: under the GAN step's BCE mean loss the unscaled gradients (spectral-norm backward and
    gx included) are the same bits at loss scales 2^0, 2^10 and 2^16."""
    import real_esrgan_pytorch_amd as R
    torch.manual_seed(6)
    d = R.Discriminator(precision="exact16", f16_backward=True).cuda().train()
    sd = {k: v.clone() for k, v in d.state_dict().items()}
    x = torch.rand(2, 3, 64, 64, device="cuda")

    def run(scale):
        d.load_state_dict(sd)                                  # the same u / v for every call
        d.zero_grad(set_to_none=True)
        xt = x.clone().requires_grad_(True)
        out = d(xt)
        (torch.nn.functional.binary_cross_entropy_with_logits(out, torch.ones_like(out)) * scale).backward()
        torch.cuda.synchronize()
        gr = {n: p.grad.detach() / scale for n, p in d.named_parameters()}
        gr["gx"] = xt.grad.detach() / scale
        return gr
    base = run(1.0)
    assert len(base) == 13
    for scale in (2.0 ** 10, 2.0 ** 16):
        got = run(scale)
        assert all(torch.equal(got[k], base[k]) for k in base), scale


def test_input_gradient_only_equals_full_backward():
    """grad_params = NULL (the generator's adversarial term: discriminator frozen) gives the gx of a full backward, bit for bit."""
    import real_esrgan_pytorch_amd as R
    torch.manual_seed(7)
    d = R.Discriminator(precision="exact16", f16_backward=True).cuda().train()
    sd = {k: v.clone() for k, v in d.state_dict().items()}
    x = torch.rand(2, 3, 64, 64, device="cuda")

    def run(weights):
        d.load_state_dict(sd)
        d.requires_grad_(weights)
        d.zero_grad(set_to_none=True)
        xt = x.clone().requires_grad_(True)
        out = d(xt)
        (torch.nn.functional.binary_cross_entropy_with_logits(out, torch.ones_like(out)) * 1024.0).backward()
        torch.cuda.synchronize()
        return xt.grad.detach().clone(), [p.grad for p in d.parameters()]
    gx_only, grads = run(False)
    assert all(g is None for g in grads)
    gx_full, grads = run(True)
    assert all(g is not None for g in grads)
    assert torch.equal(gx_only, gx_full)


def _bce(y, label, scale):
    return torch.nn.functional.binary_cross_entropy_with_logits(y, torch.full_like(y, label)) * scale


def _gan_sequence(d_for_call, sr, hr, scale=1024.0):
    """One GAN step's discriminator calls (train.RealESRGANStep): forward + gx-only backward on sr, forward + backward on hr,
    forward + backward on sr.detach().  `d_for_call(i)` hands out the module of call i."""
    res = []
    d = d_for_call(0)
    d.requires_grad_(False)
    srt = sr.clone().requires_grad_(True)
    y = d(srt)
    _bce(y, 1.0, scale).backward()
    res += [y.detach().clone(), srt.grad.detach().clone(), d.flat_uv().detach().clone()]
    for i, (x, label) in enumerate(((hr, 1.0), (sr, 0.0)), 1):
        d = d_for_call(i)
        d.requires_grad_(True)
        d.zero_grad(set_to_none=True)
        y = d(x)
        _bce(y, label, scale).backward()
        res += [y.detach().clone(), d.flat_uv().detach().clone()] + [p.grad.detach().clone() for p in d.parameters()]
    torch.cuda.synchronize()
    return res


def test_pooled_workspace_equals_fresh_modules():
    """The pooled workspace carries nothing from one call into the next: the GAN step's three discriminator calls on one module
    (one pooled workspace, f16 weights left in its packed region by every backward) equal the same calls on fresh modules."""
    import real_esrgan_pytorch_amd as R
    torch.manual_seed(8)
    sd = R.Discriminator().state_dict()
    gen = torch.Generator(device="cuda").manual_seed(3)
    sr, hr = torch.rand(2, 3, 64, 64, device="cuda", generator=gen), torch.rand(2, 3, 64, 64, device="cuda", generator=gen)
    pooled = _disc("parity", sd)
    a = _gan_sequence(lambda i: pooled, sr, hr)
    assert sum(len(v) for v in pooled._workspaces.values()) == 1          # all three calls on one workspace
    state = {"sd": sd}

    def fresh(i):
        d = _disc("parity", state["sd"] if i == 0 else state["prev"].state_dict())
        state["prev"] = d
        return d
    b = _gan_sequence(fresh, sr, hr)
    assert len(a) == len(b)
    for i, (p, q) in enumerate(zip(a, b)):
        assert torch.equal(p, q), i


def test_exact16_pass_after_f16_backward_on_the_same_workspace():
    """At the C-ABI: forward + resr_discriminator_backward_f16 on a workspace, then an exact16 forward + resr_discriminator_backward
    on it equal the same exact16 pair on a fresh workspace (logits, u / v, every gradient, gx)."""
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd.discriminator import _DWorkspace
    L, lib = R._lib, R._lib.lib()
    torch.manual_seed(9)
    d = R.Discriminator(precision="exact16").cuda().train()
    flat, uv0 = d.flat_parameters(), d.flat_uv().clone()
    n, h, w = 2, 64, 64
    desc = L.DiscriminatorDesc(n, h, w, L.RESR_F16X2, 1, 1)
    nbytes = lib.resr_discriminator_workspace_bytes(C.byref(desc))
    gen = torch.Generator(device="cuda").manual_seed(4)
    x1, x2 = torch.rand(n, 3, h, w, device="cuda", generator=gen), torch.rand(n, 3, h, w, device="cuda", generator=gen)
    gy = torch.randn(n, 1, h, w, device="cuda", generator=gen) * 1e-3
    st = L.stream_ptr(flat)

    def fwd(ws, x, uv):
        y = torch.empty(n, 1, h, w, device="cuda")
        L.check(lib.resr_discriminator_forward(C.byref(desc), L.ptr(x), L.ptr(flat), L.ptr(uv), L.ptr(ws.table), ws.n_chunks,
                                               L.ptr(ws.buf), ws.buf.numel(), L.ptr(y), st))
        return y

    def bwd(ws, f16):
        gp, gx = torch.zeros_like(flat), torch.empty(n, 3, h, w, device="cuda")
        if f16:
            L.check(lib.resr_discriminator_backward_f16(C.byref(desc), L.ptr(gy), L.ptr(flat), L.ptr(ws.table), ws.n_chunks,
                                                        L.ptr(ws.buf), ws.buf.numel(), L.ptr(gp), L.ptr(gx), st))
        else:
            L.check(lib.resr_discriminator_backward(C.byref(desc), L.ptr(gy), L.ptr(flat), L.ptr(ws.buf), ws.buf.numel(),
                                                    L.ptr(gp), L.ptr(gx), st))
        return gp, gx
    used = _DWorkspace(nbytes, flat.device, desc)
    uv_a = uv0.clone()
    fwd(used, x1, uv_a)
    gp16, gx16 = bwd(used, True)
    uv_b = uv_a.clone()
    ya = fwd(used, x2, uv_a)
    gpa, gxa = bwd(used, False)
    fresh = _DWorkspace(nbytes, flat.device, desc)
    yb = fwd(fresh, x2, uv_b)
    gpb, gxb = bwd(fresh, False)
    torch.cuda.synchronize()
    assert torch.isfinite(gp16).all() and gp16.abs().sum() > 0 and torch.isfinite(gx16).all()
    assert torch.equal(ya, yb) and torch.equal(uv_a, uv_b) and torch.equal(gpa, gpb) and torch.equal(gxa, gxb)
    # a wrong descriptor is refused: the pass needs an exact16 forward with training = 1
    bad = L.DiscriminatorDesc(n, h, w, L.RESR_F16, 1, 1)
    assert lib.resr_discriminator_backward_f16(C.byref(bad), L.ptr(gy), L.ptr(flat), L.ptr(fresh.table), fresh.n_chunks,
                                               L.ptr(fresh.buf), fresh.buf.numel(), L.ptr(gpb), L.ptr(gxb), st) != 0


def _gan_step_case(mode, z):
    import real_esrgan_pytorch_amd as R
    from oracle import model_ref as M
    from real_esrgan_pytorch_amd.train import RealESRGANStep
    seed = int(z["seed"])
    gsd = M.init_generator_state(60 + seed, 3, 3, 4, bias_noise=0.02)
    gsd["conv4.bias"] = gsd["conv4.bias"] + 0.5
    if mode == "parity":
        g = R.Generator(3, 3, 4, precision="exact16", x2_plan=R._lib.X2_PLAN_OUTPUT_PARITY)
        d = R.Discriminator(precision="exact16", f16_backward=True)
    else:
        g = R.Generator(3, 3, 4, precision="fast")
        d = R.Discriminator(precision="fast")
    g.load_state_dict(gsd)
    g = g.cuda().train()
    d.load_state_dict(M.init_discriminator_state(80 + seed))
    d = d.cuda().train()
    ema = R.EMA(g, 0.999)
    ema.register()
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=10 ** 9)
    step = RealESRGANStep(g, d, ema, torch.optim.SGD(g.parameters(), 0.0), torch.optim.SGD(d.parameters(), 0.0), scaler=scaler)
    srs = []
    hook = g.register_forward_hook(lambda m, i, o: srs.append(o.detach().clone()))
    out = step(torch.from_numpy(z["hr_crop"]).cuda(), torch.from_numpy(z["lr"]).cuda())
    torch.cuda.synchronize()
    hook.remove()
    rep = {k: abs(out[k].item() - float(z[k])) for k in ("pixel_loss", "adversarial_loss", "d_loss_hr", "d_loss_sr")}
    rep["sr"] = (srs[0].cpu() - torch.from_numpy(z["sr"])).abs().max().item()
    gn = torch.stack([p.grad.norm() for p in g.parameters()]).cpu()
    dn = torch.stack([p.grad.norm() for p in d.parameters()]).cpu()
    rg, rd = torch.from_numpy(z["g_grad_norms"]), torch.from_numpy(z["d_grad_norms"])
    rep["g_grad_norm_worst_rel"] = ((gn - rg).abs() / rg.clamp_min(1e-12)).max().item()
    rep["d_grad_norm_worst_rel"] = ((dn - rd).abs() / rd.clamp_min(1e-12)).max().item()
    sd = d.state_dict()
    rep["uv"] = max((sd[k[3:]].cpu() - torch.from_numpy(z[k])).abs().max().item() for k in z.files if k.startswith("uv_"))
    return rep


def test_golden_gan_step_in_output_parity_mode(diag_dir):
    """train.RealESRGANStep with the generator on plan 2401 and the discriminator on the f16 backward, on tests/golden/gan_step_seed5.npz
    against the reference's own values: the four losses within 1e-4, SR within 2e-4, and the worst relative gradient norm of both
    networks strictly better than fast mode's on the same case.  Measured: losses 0 .. 1.8e-7 (fast 2e-6 .. 8.6e-5), SR 1.07e-4
    (fast 2.6e-3), worst gradient norm G 1.29e-3 / D 2.5e-4 (fast 2.3e-3 / 1.9e-3).  Gates 1.5 x the measured value: SR 1.6e-4,
    G 1.9e-3, D 3.7e-4; the losses sit at the fp32 rounding of the values themselves: 1e-6."""
    z = np.load(os.path.join(G, "gan_step_seed5.npz"))
    rep = {m: _gan_step_case(m, z) for m in ("parity", "fast")}
    with open(os.path.join(diag_dir, "parity_gan_step_golden.json"), "w") as f:
        json.dump(rep, f, indent=1)
    print(json.dumps(rep, indent=1))
    p, fm = rep["parity"], rep["fast"]
    for k in ("pixel_loss", "adversarial_loss", "d_loss_hr", "d_loss_sr"):
        assert p[k] < 1e-6, (k, rep)
    assert p["sr"] < 1.6e-4, rep
    assert p["g_grad_norm_worst_rel"] < 1.9e-3 and p["d_grad_norm_worst_rel"] < 3.7e-4, rep
    assert p["uv"] < 1e-5, rep
    assert p["g_grad_norm_worst_rel"] < fm["g_grad_norm_worst_rel"], rep
    assert p["d_grad_norm_worst_rel"] < fm["d_grad_norm_worst_rel"], rep


def test_graphed_output_parity_gan_step_equals_eager_step():
    """train.GraphedStep replaying the output-parity GAN step (as test_gpu_train_harness.py's graphed-step test): losses of every
    step, the final weights of both networks and the EMA shadow bit-equal to the eager step."""
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd.train import GraphedStep, RealESRGANStep

    def run(graph):
        torch.manual_seed(0)
        g = R.Generator(3, 3, 4, n_blocks=2, precision="exact16", x2_plan=R._lib.X2_PLAN_OUTPUT_PARITY).cuda().train()
        with torch.no_grad():
            g.conv4.bias.add_(0.5)
        ema = R.EMA(g, 0.999)
        ema.register()
        go = torch.optim.Adam([g.flat_parameter()], 1e-4, (0.9, 0.99), fused=True, capturable=True)
        gen = torch.Generator(device="cuda").manual_seed(1)
        hr = torch.rand(8, 3, 128, 128, device="cuda", generator=gen)
        lr = torch.nn.functional.interpolate(hr, scale_factor=0.25, mode="area")
        scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
        d = R.Discriminator(precision="exact16", f16_backward=True).cuda().train()
        do = torch.optim.Adam([d.flat_parameter()], 1e-4, (0.9, 0.99), fused=True, capturable=True)
        step = RealESRGANStep(g, d, ema, go, do, scaler, None)
        if graph:
            step = GraphedStep(step, warmup=2)
        outs = []
        for _ in range(6):
            o = step(hr, lr)
            outs.append(torch.stack([o[k] for k in sorted(o)]).clone())
        torch.cuda.synchronize()
        return outs, [g.flat_parameters().detach().clone(), d.flat_parameters().detach().clone()], ema._flat_shadow.clone()
    oe, we, se = run(False)
    og, wg, sg = run(True)
    for a, b in zip(oe, og):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    for a, b in zip(we, wg):
        assert torch.equal(a, b)
    assert torch.equal(se, sg)
    assert int(R._lib.lib().resr_debug_chain_errors()) == 0


def test_train_realesrgan_in_output_parity_mode(tmp_path, monkeypatch):
    """`train_realesrgan.main()` with config.output_parity (what $RESR_OUTPUT_PARITY=1 sets): the generator on plan 2401, the
    discriminator and ContentLoss on the f16 backward, exact16 throughout; one epoch trains and logs finite losses."""
    import math
    from real_esrgan_pytorch_amd import config
    from real_esrgan_pytorch_amd import train_realesrgan as T
    from tests.test_gpu_train_harness import _tiny_dataset
    _tiny_dataset(tmp_path, monkeypatch, resume_d="", resume_g="", pixel_weight=1.0, adversarial_weight=0.1,
                  content_weight=[0.1, 0.1, 1.0, 1.0, 1.0], lr_scheduler_milestones=[1], lr_scheduler_gamma=0.5,
                  model_lr=1e-4, model_betas=(0.9, 0.99), ema_model_weight_decay=0.999, output_parity=True, precision="exact16",
                  feature_model_extractor_nodes=NODES, feature_model_normalize_mean=MEAN, feature_model_normalize_std=STD)
    built = {}
    build_model, define_loss = T.build_model, T.define_loss
    monkeypatch.setattr(T, "build_model", lambda: built.setdefault("models", build_model()))
    monkeypatch.setattr(T, "define_loss", lambda: built.setdefault("losses", define_loss()))
    T.main()
    d, g, _ = built["models"]
    content = built["losses"][1]
    assert (g.precision, g.x2_plan) == ("exact16", 2401)
    assert (d.precision, d.f16_backward) == ("exact16", True)
    assert (content.precision, content.f16_backward) == ("exact16", True)
    rows = [json.loads(l) for l in open(tmp_path / "samples" / "logs" / "harness_test" / "scalars.jsonl")]
    losses = [r["value"] for r in rows if r["tag"] in ("Train/D_Loss", "Train/G_Loss", "Train/Pixel_Loss", "Train/Adversarial_Loss")]
    assert losses and all(math.isfinite(v) for v in losses)
    assert (tmp_path / "results" / "harness_test" / "g_last.pth.tar").exists()
