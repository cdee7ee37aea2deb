"""-m gpu: the compact generator from its native passes up to the train scripts -- the gradient hook of its backward, the one-tensor
`flat_parameter()` mode under Adam / GradScaler / EMA, graph replay of both train steps, the data-parallel exchange (two gloo ranks on
the one GPU; a world-1 RCCL group), and `train_realesrnet.main()` / `train_realesrgan.main()` / `test.main()` with
`config.g_arch = "compact"`.

Every comparison here is `torch.equal`: both sides run the same launches on the same values (the backward pass is deterministic:
tests/test_gpu_compact_train.py), and the only arithmetic that differs between them is exact -- a multiplication by 0.5, one
two-term fp32 sum, the mean over one rank.

Shapes: SRVGGNetCompact(num_conv=2, upscale=4, trainable=True), batch 2, LR 16x16 (HR 64x64: two 32-column tiles of the HR tail, two
body layers to order) unless a test says otherwise.  Every process a test starts is joined with a time limit and killed past it.
"""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _model(precision, seed=0, trainable=True):
    import real_esrgan_pytorch_amd as R
    torch.manual_seed(seed)
    return R.SRVGGNetCompact(num_conv=2, upscale=4, act_type="prelu", precision=precision, trainable=trainable).cuda().train()


def _data(n=2, lr_size=16, seed=9):
    """(lr, hr) on the host: hr uniform, lr its 4x4 area mean."""
    g = torch.Generator().manual_seed(seed)
    hr = torch.rand(n, 3, 4 * lr_size, 4 * lr_size, generator=g)
    return torch.nn.functional.interpolate(hr, scale_factor=0.25, mode="area"), hr


def _flat_of_grads(m):
    return torch.cat([p.grad.reshape(-1) for p in m.parameters()])


# ---- 1. the hook ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["strict", "fast"])
def test_grad_hook_runs_once_per_backward_before_autograd_sees_the_gradients(precision):
    m = _model(precision)
    lr, hr = (t.cuda() for t in _data())
    gy = torch.randn(hr.shape, generator=torch.Generator().manual_seed(2)).cuda() * 1e-2

    def grads():
        m.zero_grad(set_to_none=True)
        m(lr).backward(gy)
        return {n: p.grad.clone() for n, p in m.named_parameters()}
    ref = grads()
    calls = []

    def hook(flat):
        calls.append((tuple(flat.shape), flat.dtype))
        flat.mul_(0.5)
    m.grad_hook = hook
    got = grads()
    assert calls == [((m.flat_parameters().numel(),), torch.float32)]
    assert all(torch.equal(got[n], 0.5 * ref[n]) for n in ref), [n for n in ref if not torch.equal(got[n], 0.5 * ref[n])]
    # one-tensor mode: the same hook, the same halved gradients, in the alias's .grad alone
    fp = m.flat_parameter()
    m.zero_grad(set_to_none=True)
    m(lr).backward(gy)
    assert len(calls) == 2 and all(p.grad is None for p in m.parameters())
    assert torch.equal(fp.grad, torch.cat([0.5 * ref[n].reshape(-1) for n in ref])) and m.flat_grad() is fp.grad
    # a backward that wants the input's gradient only does not call it
    m.requires_grad_(False)
    assert not fp.requires_grad
    x = lr.clone().requires_grad_()
    m(x).backward(gy)
    torch.cuda.synchronize()
    assert len(calls) == 2 and x.grad is not None and torch.isfinite(x.grad).all()


# ---- 2. one-tensor mode --------------------------------------------------------------------------------------------------
def _three_steps(precision, flat):
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd.train import RealESRNetStep
    m = _model(precision)
    ema = R.EMA(m, 0.999)
    ema.register()
    opt = torch.optim.Adam([m.flat_parameter()] if flat else m.parameters(), 1e-3, (0.9, 0.99), fused=True)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0) if precision == "fast" else None
    step = RealESRNetStep(m, ema, opt, scaler, None)
    lr, hr = (t.cuda() for t in _data())
    out = {"losses": [step(hr, lr).clone() for _ in range(3)]}
    out["weights"], out["shadow"] = m.flat_parameters().detach().clone(), ema._flat_shadow.clone()
    # two backward passes without zero_grad: autograd's own add, in either mode
    m.zero_grad(set_to_none=True)
    for k in range(2):
        (m(lr) - hr).abs().mean().mul(1024.0 if scaler else 1.0).backward()
    out["sum"] = (m.flat_grad() if flat else _flat_of_grads(m)).clone()
    assert (m.flat_grad() is None) == (not flat) and (not flat or all(p.grad is None for p in m.parameters()))
    # the arena is rebuilt under the optimiser (validate() of the train scripts): the alias follows it
    before = m.flat_parameters().data_ptr()
    ema.apply_shadow()
    with torch.no_grad():
        out["sr_ema"] = m(lr).clone()                    # a forward on the shadow's tensors builds a new arena, restore() leaves it again
    ema.restore()
    out["losses"].append(step(hr, lr).clone())
    assert m.flat_parameters().data_ptr() != before and (not flat or m.flat_parameter().data_ptr() == m.flat_parameters().data_ptr())
    out["weights_after"], out["shadow_after"] = m.flat_parameters().detach().clone(), ema._flat_shadow.clone()
    torch.cuda.synchronize()
    assert scaler is None or scaler.get_scale() == 1024.0                    # no step was skipped
    return out


@pytest.mark.parametrize("precision", ["strict", "fast"])
def test_flat_parameter_steps_equal_per_tensor_steps(precision):
    a, b = _three_steps(precision, False), _three_steps(precision, True)
    assert all(torch.isfinite(v) for v in a["losses"]) and not torch.equal(a["losses"][0], a["losses"][2])
    for x, y in zip(a["losses"], b["losses"]):
        assert torch.equal(x, y), (a["losses"], b["losses"])
    for k in ("weights", "shadow", "sum", "sr_ema", "weights_after", "shadow_after"):
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["weights"], a["weights_after"]) and a["sum"].abs().max() > 0


# ---- 3. EMA --------------------------------------------------------------------------------------------------------------
def test_ema_of_the_compact_generator_takes_the_flat_path_with_the_reference_rounding():
    import real_esrgan_pytorch_amd as R
    m = _model("fast")
    d = 0.999
    ema = R.EMA(m, d)
    ema.register()
    assert ema._flat_shadow is not None and ema._flat_shadow.numel() == m.flat_parameters().numel()
    with torch.no_grad():
        m.flat_parameters().add_(torch.randn(m.flat_parameters().shape, generator=torch.Generator().manual_seed(5)).cuda() * 1e-2)
    shadow = {n: v.clone() for n, v in ema.shadow.items()}
    ema.update()
    torch.cuda.synchronize()
    assert set(shadow) == {n for n, _ in m.named_parameters()}
    for n, p in m.named_parameters():
        want = (1.0 - d) * p.detach() + d * shadow[n]          # reference model.py: two rounded products, then their rounded sum
        assert not torch.equal(ema.shadow[n], shadow[n]) and torch.equal(ema.shadow[n], want), n
        assert ema.shadow[n].data_ptr() >= ema._flat_shadow.data_ptr()       # views of the one shadow arena


# ---- 4. graph replay -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gan", [False, True])
def test_graphed_compact_step_equals_eager_step(gan):
    """tests/test_gpu_train_harness.py::test_graphed_step_equals_eager_step with the compact generator."""
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd.train import GraphedStep, RealESRGANStep, RealESRNetStep

    def run(graph):
        g = _model("fast")
        ema = R.EMA(g, 0.999)
        ema.register()
        go = torch.optim.Adam([g.flat_parameter()], 1e-4, (0.9, 0.99), fused=True, capturable=True)
        lr, hr = (t.cuda() for t in (_data(4, 32) if gan else _data()))   # the discriminator wants H, W divisible by 8
        scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
        d = None
        if gan:
            torch.manual_seed(1)
            d = R.Discriminator(precision="fast").cuda().train()
            do = torch.optim.Adam([d.flat_parameter()], 1e-4, (0.9, 0.99), fused=True, capturable=True)
            step = RealESRGANStep(g, d, ema, go, do, scaler, None)
        else:
            step = RealESRNetStep(g, ema, go, scaler, None)
        if graph:
            step = GraphedStep(step, warmup=2)
        outs = []
        for _ in range(6):
            o = step(hr, lr)
            outs.append(torch.stack([o[k] for k in sorted(o)]).clone() if isinstance(o, dict) else o.clone())
        torch.cuda.synchronize()
        assert not graph or step._graph is not None
        return outs, [g.flat_parameters().detach().clone()] + ([d.flat_parameters().detach().clone()] if gan else []), ema._flat_shadow.clone()
    oe, we, se = run(False)
    og, wg, sg = run(True)
    assert all(torch.isfinite(o).all() for o in oe) and not torch.equal(oe[0], oe[5])
    for a, b in zip(oe, og):
        assert torch.equal(a, b), (oe, og)
    for a, b in zip(we, wg):
        assert torch.equal(a, b)
    assert torch.equal(se, sg)


# ---- processes -----------------------------------------------------------------------------------------------------------
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(target, world, limit=300):
    """`world` spawned processes of target(rank, world, port, queue): one result each, every process joined or killed."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=target, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in procs:
            res.append(q.get(timeout=limit))
    finally:
        for p in procs:
            p.join(timeout=60 if len(res) == world else 1)
            if p.is_alive():
                p.kill()
                p.join(timeout=30)
    for r in res:
        assert "error" not in r, r
    return {r["rank"]: r for r in res}


def _half_step(m, opt, lr, hr):
    from real_esrgan_pytorch_amd.train import RealESRNetStep
    return RealESRNetStep(m, None, opt, None, None)(hr.cuda(), lr.cuda())


def _adam(m):
    return torch.optim.Adam(m.parameters(), 1e-3, (0.9, 0.99))


# ---- 5. two ranks, one GPU -----------------------------------------------------------------------------------------------
def _two_rank_worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from real_esrgan_pytorch_amd.train import DataParallel
        torch.cuda.set_device(0)
        m = _model("strict")
        if rank == 1:                                   # replicas must be made identical by the broadcast of attach
            with torch.no_grad():
                m.flat_parameters().add_(1.0)
        dp = DataParallel()
        dp.attach(m)
        assert dp.active and dp.overlap is False and m.grad_hook is not None
        lr, hr = _data(4)
        half = slice(rank * 2, rank * 2 + 2)
        loss = _half_step(m, _adam(m), lr[half], hr[half])
        torch.cuda.synchronize()
        q.put({"rank": rank, "loss": float(loss), "weights": m.flat_parameters().detach().cpu().numpy()})   # by value
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        import traceback
        q.put({"rank": rank, "error": repr(e), "trace": traceback.format_exc()})


def test_two_rank_compact_step_matches_single_process():
    """gloo sums the two ranks' gradients and `_finish_mean_` multiplies by 0.5: a two-term fp32 sum has one order, so the weights
    after the step equal, bit for bit, those of one process that steps on (g0 + g1) * 0.5."""
    from real_esrgan_pytorch_amd import losses
    res = _run_ranks(_two_rank_worker, 2)
    w0, w1 = (torch.from_numpy(res[r]["weights"]) for r in (0, 1))
    assert torch.equal(w0, w1)
    m = _model("strict")
    start = m.flat_parameters().detach().cpu().clone()
    lr, hr = _data(4)
    grads, vals = [], []
    for r in (0, 1):
        half = slice(r * 2, r * 2 + 2)
        m.zero_grad(set_to_none=True)
        loss = losses.l1_loss(torch.nn.L1Loss(), m(lr[half].cuda()), hr[half].cuda())    # the step's own loss launch
        loss.backward()
        grads.append(_flat_of_grads(m).clone())
        vals.append(float(loss.detach()))
    assert [res[0]["loss"], res[1]["loss"]] == vals and not torch.equal(grads[0], grads[1])
    mean = (grads[0] + grads[1]) * 0.5
    off = 0
    for p in m.parameters():
        p.grad = mean[off:off + p.numel()].view_as(p).clone()
        off += p.numel()
    _adam(m).step()
    torch.cuda.synchronize()
    assert torch.equal(w0, m.flat_parameters().detach().cpu()) and not torch.equal(w0, start)


# ---- 6. world-1 RCCL -----------------------------------------------------------------------------------------------------
def _nccl_world1_worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        import warnings
        from real_esrgan_pytorch_amd.train import DataParallel, RealESRNetStep
        lr, hr = (t.cuda() for t in _data())
        res = {"rank": rank}
        runs = {}
        for attached in (False, True):
            m = _model("fast")
            calls = []
            if attached:
                dp = DataParallel(force=True)
                assert dp.active and dp.backend == "nccl" and dp._avg
                with warnings.catch_warnings(record=True) as seen:
                    warnings.simplefilter("always")
                    dp.attach(m, overlap=True)
                res["overlap"], res["warned"] = dp.overlap, [str(w.message) for w in seen if issubclass(w.category, RuntimeWarning)]
                inner = m.grad_hook

                def spy(flat, inner=inner, calls=calls):
                    calls.append(flat.numel())
                    return inner(flat)
                m.grad_hook = spy
            opt = torch.optim.Adam(m.parameters(), 1e-3, (0.9, 0.99), fused=True)
            loss = RealESRNetStep(m, None, opt, torch.amp.GradScaler("cuda", init_scale=1024.0), None)(hr, lr)
            torch.cuda.synchronize()
            runs[attached] = (loss.clone(), m.flat_parameters().detach().clone(), _flat_of_grads(m).clone())
            res["calls"] = calls
        res["bit_equal"] = all(torch.equal(a, b) for a, b in zip(runs[False], runs[True]))
        res["moved"] = bool(runs[True][2].abs().max() > 0)
        dist.destroy_process_group()
        q.put(res)
    except Exception as e:  # pragma: no cover
        import traceback
        q.put({"rank": rank, "error": repr(e), "trace": traceback.format_exc()})


def test_rccl_world1_exchange_is_the_identity_and_overlap_falls_back():
    res = _run_ranks(_nccl_world1_worker, 1)[0]
    assert res["bit_equal"] and res["moved"], res                     # ReduceOp.AVG over one rank: the gradient itself
    assert res["overlap"] is False and len(res["calls"]) == 1, res    # one message behind the backward pass


# ---- 7. the scripts ------------------------------------------------------------------------------------------------------
def _smooth_png(path, size, seed):
    from PIL import Image
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    x = F.interpolate(torch.rand(1, 3, size // 8, size // 8, generator=g), size=(size, size), mode="bicubic").clamp(0, 1)
    x = (0.85 * x + 0.15 * torch.rand(1, 3, size, size, generator=g)).clamp(0, 1)
    Image.fromarray((x[0].permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(path)


def _tiny_dataset(tmp_path, monkeypatch, **extra):
    """The tiny data set of tests/test_gpu_train_harness.py (224-pixel PNGs, image_size 208, batch 2, one epoch) with the compact
    generator configured."""
    from PIL import Image
    from real_esrgan_pytorch_amd import config, imgproc
    for k, (sub, n) in enumerate((("train", 4), ("valid", 2), ("test_hr", 2))):
        os.makedirs(tmp_path / sub)
        for i in range(n):
            _smooth_png(str(tmp_path / sub / f"{i}.png"), 224, 10 * k + i)
    os.makedirs(tmp_path / "test_lr")
    for i in range(2):
        hr = imgproc.read_image_rgb(str(tmp_path / "test_hr" / f"{i}.png"))
        lr = np.clip(imgproc.image_resize(hr, 0.25), 0, 1)
        Image.fromarray((lr * 255).round().astype(np.uint8)).save(str(tmp_path / "test_lr" / f"{i}.png"))
    here = os.path.dirname(os.path.abspath(__file__))
    settings = dict(train_image_dir=str(tmp_path / "train"), valid_image_dir=str(tmp_path / "valid"),
                    test_lr_image_dir=str(tmp_path / "test_lr"), test_hr_image_dir=str(tmp_path / "test_hr"),
                    image_size=208, batch_size=2, num_workers=0, epochs=1, print_frequency=1, resume="", pretrained_g="",
                    lr_scheduler_step_size=1, exp_name="compact_test", model_lr=2e-4, model_betas=(0.9, 0.99),
                    ema_model_weight_decay=0.999, niqe_model_path=os.path.join(here, "golden", "niqe_model.mat"),
                    device=torch.device("cuda", 0), g_arch="compact", compact_num_conv=2, compact_act_type="prelu",
                    precision="fast", output_parity=False, inference_precision="exact16", upscale_factor=4)
    settings.update(extra)
    for k, v in settings.items():
        monkeypatch.setattr(config, k, v, raising=False)
    monkeypatch.chdir(tmp_path)


def _compact_keys():
    import real_esrgan_pytorch_amd as R
    return list(R.SRVGGNetCompact(num_conv=2).state_dict())


def test_train_scripts_with_the_compact_generator(tmp_path, monkeypatch):
    """train_realesrnet.main(), its resume, train_realesrgan.main() from its checkpoint and test.main() on the result."""
    from PIL import Image
    from real_esrgan_pytorch_amd import config
    from real_esrgan_pytorch_amd import test as E
    from real_esrgan_pytorch_amd import train_realesrgan as TG
    from real_esrgan_pytorch_amd import train_realesrnet as T
    _tiny_dataset(tmp_path, monkeypatch)
    keys = _compact_keys()
    T.main()
    samples, results = tmp_path / "samples" / "compact_test", tmp_path / "results" / "compact_test"
    ck1 = samples / "g_epoch_1.pth.tar"
    assert ck1.exists() and (results / "g_last.pth.tar").exists()
    ck = torch.load(ck1, weights_only=False)
    assert set(ck) == {"epoch", "best_niqe", "state_dict", "ema_state_dict", "optimizer", "scheduler"}
    assert ck["epoch"] == 1 and list(ck["state_dict"]) == keys and keys[0] == "body.0.weight" and len(keys) == 2 * 4 + 3
    assert list(ck["ema_state_dict"]) == ["model." + k for k in keys]
    assert np.isfinite(ck["best_niqe"])
    tags = [json.loads(l)["tag"] for l in open(tmp_path / "samples" / "logs" / "compact_test" / "scalars.jsonl")]
    assert "Train/Loss" in tags and "Valid/NIQE" in tags and "Test/NIQE" in tags
    # resume for one more epoch: the optimiser state carries over
    monkeypatch.setattr(config, "resume", str(ck1))
    monkeypatch.setattr(config, "epochs", 2)
    T.main()
    ck2 = torch.load(samples / "g_epoch_2.pth.tar", weights_only=False)
    assert ck2["epoch"] == 2 and ck2["optimizer"]["state"][0]["step"] == 4               # 2 steps per epoch
    assert not torch.equal(ck2["state_dict"]["body.0.weight"], ck["state_dict"]["body.0.weight"])
    # the GAN script from the RealESRNet checkpoint
    for k, v in dict(exp_name="compact_gan", epochs=1, resume=str(ck1), resume_d="", resume_g="", pixel_weight=1.0, adversarial_weight=0.1,
                     content_weight=[0.1, 0.1, 1.0, 1.0, 1.0], lr_scheduler_milestones=[1], lr_scheduler_gamma=0.5, model_lr=1e-4,
                     feature_model_extractor_nodes=["features.2", "features.7", "features.16", "features.25", "features.34"],
                     feature_model_normalize_mean=[0.485, 0.456, 0.406], feature_model_normalize_std=[0.229, 0.224, 0.225]).items():
        monkeypatch.setattr(config, k, v, raising=False)
    TG.main()
    gan = tmp_path / "samples" / "compact_gan"
    d1 = torch.load(gan / "d_epoch_1.pth.tar", weights_only=False)
    g1 = torch.load(gan / "g_epoch_1.pth.tar", weights_only=False)
    assert set(d1) == {"epoch", "best_niqe", "state_dict", "optimizer", "scheduler"}
    assert list(g1["state_dict"]) == keys and list(g1["ema_state_dict"]) == ["model." + k for k in keys]
    w0, w1 = ck["state_dict"]["body.0.weight"].cpu(), g1["state_dict"]["body.0.weight"].cpu()
    assert not torch.equal(w0, w1) and (w0 - w1).abs().max() < 1e-2                      # started from the RealESRNet weights, then moved
    # directory evaluation with that checkpoint's EMA weights
    for k, v in dict(lr_dir=str(tmp_path / "test_lr"), sr_dir=str(tmp_path / "sr"), hr_dir=str(tmp_path / "test_hr"),
                     model_path=str(gan / "g_epoch_1.pth.tar")).items():
        monkeypatch.setattr(config, k, v, raising=False)
    score = E.main()
    assert np.isfinite(score) and 0 < score <= 100
    assert sorted(os.listdir(tmp_path / "sr")) == sorted(os.listdir(tmp_path / "test_lr")) == ["0.png", "1.png"]
    for name in ("0.png", "1.png"):
        w, h = Image.open(tmp_path / "test_lr" / name).size
        assert Image.open(tmp_path / "sr" / name).size == (4 * w, 4 * h)


def test_pretrained_g_starts_weights_and_ema_from_the_upstream_checkpoint(tmp_path, monkeypatch):
    """With a learning rate of 0 the weights must stay the checkpoint's, bit for bit, and so must the EMA -- which it can only when
    its shadow was registered again from the loaded weights.  The EMA decay here is 0.5: (1 - d) * p + d * p is then exact in fp32
    (two halvings and their sum), where 0.999 would move one element in six by an ulp; a shadow left on build_model()'s random
    init r would hold 0.75 p + 0.25 r after the epoch's two updates."""
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd import config
    from real_esrgan_pytorch_amd import train_realesrnet as T
    _tiny_dataset(tmp_path, monkeypatch, model_lr=0.0, ema_model_weight_decay=0.5)
    torch.manual_seed(77)
    sd = {k: v.clone() for k, v in R.SRVGGNetCompact(num_conv=2).state_dict().items()}
    torch.save({"params_ema": sd}, tmp_path / "upstream.pth")
    monkeypatch.setattr(config, "pretrained_g", str(tmp_path / "upstream.pth"))
    shadows, validate = [], T.validate

    def validate_and_keep(model, ema_model, *a, **k):      # (the checkpoint's "ema_state_dict" holds EMA.model, as the reference's: the shadow is read here)
        shadows.append(ema_model._flat_shadow.detach().cpu().clone())
        return validate(model, ema_model, *a, **k)
    monkeypatch.setattr(T, "validate", validate_and_keep)
    T.main()
    ck = torch.load(tmp_path / "samples" / "compact_test" / "g_epoch_1.pth.tar", weights_only=False)
    assert ck["optimizer"]["state"][0]["step"] == 2                                       # the steps ran
    assert list(ck["state_dict"]) == list(sd)
    for k in sd:
        assert torch.equal(ck["state_dict"][k].cpu(), sd[k]), k
        assert torch.equal(ck["ema_state_dict"]["model." + k].cpu(), sd[k]), k
    assert len(shadows) == 2 and all(torch.equal(s, torch.cat([v.reshape(-1) for v in sd.values()])) for s in shadows)
