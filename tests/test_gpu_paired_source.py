"""-m gpu: `device_data.PairedDeviceSource` against the loader path (`dataset.PairedPrefetcher` over `PairedImageDataset` at
num_workers=0) under the same seeds and sampler -- the same batches bit for bit, over two passes --, a consumer on another stream, two
compact training steps fed by either path, and one epoch of train_realesrnet and of train_realesrgan with config.data_source = "paired".

Nothing here has a tolerance: both paths evaluate device_data.paired_sample_np's arithmetic on the same bytes."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SCALE, PATCH, BATCH = 4, 16, 4
LR_SIZES = [(16, 16), (17, 23), (40, 16), (33, 33), (16, 37), (21, 18), (29, 35), (18, 18), (25, 16), (16, 31), (36, 20), (19, 27)]


@pytest.fixture(scope="module")
def D():
    from real_esrgan_pytorch_amd import device_data
    return device_data


def _write_pairs(root, lr_sizes, scale, seed):
    """Smooth colour fields plus noise (so a training step has something to fit): <root>/hr/<i>.png and its LR partner <root>/lr/<i>.png,
    the area mean of the HR side."""
    from PIL import Image
    hr_dir, lr_dir = os.path.join(root, "hr"), os.path.join(root, "lr")
    os.makedirs(hr_dir)
    os.makedirs(lr_dir)
    rng = np.random.default_rng(seed)
    for i, (h, w) in enumerate(lr_sizes):
        low = rng.random((h // 4 + 1, w // 4 + 1, 3))
        x = np.kron(low, np.ones((4 * scale, 4 * scale, 1)))[:scale * h, :scale * w]
        hr = (255 * (0.8 * x + 0.2 * rng.random(x.shape))).astype(np.uint8)
        lr = hr.reshape(h, scale, w, scale, 3).mean(axis=(1, 3)).round().astype(np.uint8)
        Image.fromarray(hr).save(os.path.join(hr_dir, f"{i}.png"))
        Image.fromarray(lr).save(os.path.join(lr_dir, f"{i}.png"))
    return hr_dir, lr_dir


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    return _write_pairs(str(tmp_path_factory.mktemp("pairs")), LR_SIZES, SCALE, 1)


def _sources(D, pairs, seed):
    """Both paths over the same directories, each started under the same `random` seed with a sampler of its own in the same state."""
    from torch.utils.data import DataLoader, RandomSampler
    from real_esrgan_pytorch_amd.dataset import PairedImageDataset, PairedPrefetcher
    device = torch.device("cuda", 0)
    data = PairedImageDataset(pairs[0], pairs[1], PATCH, SCALE)

    def loader():
        random.seed(seed)
        sampler = RandomSampler(data, generator=torch.Generator().manual_seed(seed))
        return PairedPrefetcher(DataLoader(data, batch_size=BATCH, sampler=sampler, num_workers=0, drop_last=True), device)

    def resident():
        random.seed(seed)
        sampler = RandomSampler(range(len(data)), generator=torch.Generator().manual_seed(seed))
        return D.PairedDeviceSource.from_dirs(pairs[0], pairs[1], BATCH, PATCH, SCALE, device, sampler=sampler)
    return loader, resident


def _two_passes(source):
    """What 2 x (3 batches + the None that ends a pass) of next() give, with `random`'s state after each call; reset() between the passes."""
    out = []
    for epoch in range(2):
        for _ in range(4):
            item = source.next()
            out.append((None if item is None else (item[0].clone(), item[1].clone(), dict(item[2])), random.getstate()))
        assert source.next() is None                                   # it stays ended
        if epoch == 0:
            source.reset()
    torch.cuda.synchronize()
    return out


def test_source_gives_the_loader_paths_batches_over_two_passes(D, pairs):
    from torch.utils.data import RandomSampler
    loader, resident = _sources(D, pairs, 11)
    want = _two_passes(loader())
    source = resident()
    assert len(source) == 3 and source.M == 12 and isinstance(source.original_dataloader.sampler, RandomSampler)
    files = os.listdir(pairs[0])
    assert [tuple(r) for r in source.table_host[:, 2:].tolist()] == [LR_SIZES[int(f.split(".")[0])] for f in files]     # os.listdir(hr_dir) order
    assert source.hr_arena.numel() == 16 * source.lr_arena.numel() == 16 * 3 * sum(h * w for h, w in LR_SIZES)
    got = _two_passes(source)
    seen = []
    for k, ((w, w_state), (g, g_state)) in enumerate(zip(want, got)):
        assert w_state == g_state, f"`random` differs after next() {k}"
        if k % 4 == 3:
            assert w is None and g is None                             # the fourth next() of a pass ends it
            continue
        (w_lr, w_hr, w_batch), (g_lr, g_hr, g_batch) = w, g
        assert g_lr.is_cuda and g_lr.dtype == g_hr.dtype == torch.float32
        assert g_lr.shape == (BATCH, 3, PATCH, PATCH) and g_hr.shape == (BATCH, 3, SCALE * PATCH, SCALE * PATCH)
        assert torch.equal(g_lr, w_lr) and torch.equal(g_hr, w_hr), k  # bit for bit, and so the order
        assert set(g_batch) == set(w_batch) == {"lr", "hr", "index"} and g_batch["index"] == w_batch["index"] == k % 4
        assert g_batch["lr"].data_ptr() != 0 and g_batch["hr"].shape == g_hr.shape
        seen.append(g_lr)
    assert not torch.equal(seen[0], seen[3])                            # the second pass is another draw, not the first again


def test_a_consumer_on_another_stream_reads_complete_pairs(D):
    """No device-wide synchronisation between the producer's launch and the consumer's reads: the event of next() alone orders them,
    and record_stream keeps the outputs alive.  48 samples with a 256 x 256 HR patch per batch, so the launch is still running when next()
    returns."""
    rng = np.random.default_rng(5)
    sizes = [(64, 64), (70, 65), (64, 91), (80, 80)]
    lr = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    hr = [rng.integers(0, 256, (4 * h, 4 * w, 3), dtype=np.uint8) for h, w in sizes]
    order = [i % 4 for i in range(96)]
    random.seed(21)
    plans = [[(i,) + D.sample_paired_draw(sizes[i][0], sizes[i][1], 64) for i in order[b * 48:(b + 1) * 48]] for b in range(2)]
    random.seed(21)                                                     # the source draws batch 0 now, batch 1 inside the first next()
    source = D.PairedDeviceSource.from_arrays(hr, lr, 48, 64, 4, torch.device("cuda", 0), sampler=order)
    consumer = torch.cuda.Stream()
    kept = []
    with torch.cuda.stream(consumer):
        for k in range(2):
            lr_b, hr_b, batch = source.next()
            assert batch["index"] == k
            kept.append((lr_b.clone(), hr_b.clone()))                   # enqueued on the consumer stream, right behind the event
            del lr_b, hr_b, batch                                       # the allocator may hand the outputs on: record_stream holds them
        assert source.next() is None
    consumer.synchronize()                                              # this stream only
    for plan, (lr_b, hr_b) in zip(plans, kept):
        lr_b, hr_b = lr_b.cpu().numpy(), hr_b.cpu().numpy()
        for b in (0, 1, 23, 47):
            i, top, left, code = plan[b]
            want_lr, want_hr = D.paired_sample_np(hr[i], lr[i], top, left, code, 64, 4)
            assert np.array_equal(lr_b[b], want_lr) and np.array_equal(hr_b[b], want_hr), b
    with pytest.raises(IndexError):
        D.PairedDeviceSource.from_arrays(hr, lr, 2, 64, 4, torch.device("cuda", 0), sampler=[0, 4])      # an index past the pairs never reaches the kernel


# ---- training --------------------------------------------------------------------------------------------------------------------
def _two_steps(make_source):
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd.train import RealESRNetStep
    torch.manual_seed(0)
    m = R.SRVGGNetCompact(num_conv=2, upscale=SCALE, act_type="prelu", precision="fast", trainable=True).cuda().train()
    ema = R.EMA(m, 0.999)
    ema.register()
    opt = torch.optim.Adam([m.flat_parameter()], 1e-3, (0.9, 0.99), fused=True)
    step = RealESRNetStep(m, ema, opt, torch.amp.GradScaler("cuda", init_scale=1024.0), None)
    source = make_source()
    losses = []
    for _ in range(2):
        lr, hr, _batch = source.next()
        losses.append(step(hr, lr).clone())
    torch.cuda.synchronize()
    return torch.stack(losses).cpu(), m.flat_parameters().detach().clone().cpu(), ema._flat_shadow.clone().cpu()


def test_two_steps_fed_by_either_path_end_with_the_same_weight_bits(D, pairs):
    loader, resident = _sources(D, pairs, 3)
    want = _two_steps(loader)
    got = _two_steps(resident)
    assert torch.isfinite(want[0]).all() and not torch.equal(want[0][0], want[0][1])
    assert torch.equal(got[0], want[0]), (got[0], want[0])
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)) and torch.equal(got[2].view(torch.int32), want[2].view(torch.int32))


def _smooth_png(path, size, seed):
    from PIL import Image
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    x = F.interpolate(torch.rand(1, 3, size // 8, size // 8, generator=g), size=(size, size), mode="bicubic").clamp(0, 1)
    x = (0.85 * x + 0.15 * torch.rand(1, 3, size, size, generator=g)).clamp(0, 1)
    Image.fromarray((x[0].permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(path)


def _tiny_paired_run(tmp_path, monkeypatch):
    """4 training pairs (LR sides 52..70, so image_size 208 gives the LR patch 52), 2 valid and 2 test images of 224, batch 2, one epoch,
    the compact generator, config.data_source = "paired"."""
    from PIL import Image
    from real_esrgan_pytorch_amd import config, imgproc
    hr_dir, lr_dir = _write_pairs(str(tmp_path / "train"), [(52, 52), (60, 56), (56, 64), (70, 53)], 4, 2)
    for k, (sub, n) in enumerate((("valid", 2), ("test_hr", 2))):
        os.makedirs(tmp_path / sub)
        for i in range(n):
            _smooth_png(str(tmp_path / sub / f"{i}.png"), 224, 10 * k + i)
    os.makedirs(tmp_path / "test_lr")
    for i in range(2):
        hr = imgproc.read_image_rgb(str(tmp_path / "test_hr" / f"{i}.png"))
        lr = np.clip(imgproc.image_resize(hr, 0.25), 0, 1)
        Image.fromarray((lr * 255).round().astype(np.uint8)).save(str(tmp_path / "test_lr" / f"{i}.png"))
    here = os.path.dirname(os.path.abspath(__file__))
    settings = dict(train_image_dir=hr_dir, paired_lr_image_dir=lr_dir, valid_image_dir=str(tmp_path / "valid"),
                    test_lr_image_dir=str(tmp_path / "test_lr"), test_hr_image_dir=str(tmp_path / "test_hr"),
                    image_size=208, batch_size=2, num_workers=0, epochs=1, print_frequency=1, resume="", pretrained_g="",
                    lr_scheduler_step_size=1, exp_name="paired_source_test", model_lr=2e-4, model_betas=(0.9, 0.99),
                    ema_model_weight_decay=0.999, niqe_model_path=os.path.join(here, "golden", "niqe_model.mat"),
                    device=torch.device("cuda", 0), g_arch="compact", compact_num_conv=2, compact_act_type="prelu",
                    precision="fast", output_parity=False, inference_precision="exact16", upscale_factor=4, data_source="paired")
    for k, v in settings.items():
        monkeypatch.setattr(config, k, v, raising=False)
    monkeypatch.chdir(tmp_path)


def test_train_realesrgan_epoch_from_the_paired_source(D, tmp_path, monkeypatch):
    """The GAN script takes its pairs the same way: one epoch of two steps from the resident source, the degradation stage untouched."""
    from real_esrgan_pytorch_amd import config, degrade
    from real_esrgan_pytorch_amd import train_realesrgan as G
    from real_esrgan_pytorch_amd import train_realesrnet as T
    _tiny_paired_run(tmp_path, monkeypatch)
    gan = dict(resume_d="", resume_g="", pixel_weight=1.0, adversarial_weight=0.1, content_weight=[0.1, 0.1, 1.0, 1.0, 1.0],
               lr_scheduler_milestones=[1], lr_scheduler_gamma=0.5, model_lr=1e-4,
               feature_model_extractor_nodes=["features.2", "features.7", "features.16", "features.25", "features.34"],
               feature_model_normalize_mean=[0.485, 0.456, 0.406], feature_model_normalize_std=[0.229, 0.224, 0.225])
    for k, v in gan.items():
        monkeypatch.setattr(config, k, v, raising=False)

    def never(*args, **kwargs):
        raise AssertionError("the degradation stage ran in paired mode")
    monkeypatch.setattr(T, "DegradationPrefetcher", never)
    monkeypatch.setattr(G, "DegradationPrefetcher", never)
    monkeypatch.setattr(degrade, "sample_plan", never)
    monkeypatch.setattr(degrade, "run_plan", never)
    G.main()
    g1 = torch.load(tmp_path / "samples" / "paired_source_test" / "g_epoch_1.pth.tar", weights_only=False)
    assert g1["epoch"] == 1 and g1["optimizer"]["state"][0]["step"] == 2 and np.isfinite(g1["best_niqe"])
    assert (tmp_path / "samples" / "paired_source_test" / "d_epoch_1.pth.tar").exists()
    scalars = [json.loads(l) for l in open(tmp_path / "samples" / "logs" / "paired_source_test" / "scalars.jsonl")]
    for tag in ("Train/G_Loss", "Train/D_Loss", "Train/Pixel_Loss"):
        values = [s["value"] for s in scalars if s["tag"] == tag]
        assert len(values) == 2 and all(np.isfinite(v) and v > 0 for v in values), (tag, values)


def test_train_realesrnet_epoch_from_the_paired_source(D, tmp_path, monkeypatch):
    """train() iterates the paired source itself: pair_batch launches, and nothing of the degradation stage -- not its prefetcher, not a
    plan, not a run of one, and none of the launches that feed it (tile_batch 33000, blur_kernels 33100).  The degradation kernels
    themselves carry no profiling ids, so the stage's Python entry points are watched next to the ids."""
    from real_esrgan_pytorch_amd import _lib as L
    from real_esrgan_pytorch_amd import config, degrade
    from real_esrgan_pytorch_amd import train_realesrnet as T
    _tiny_paired_run(tmp_path, monkeypatch)
    made, ids = [], []
    load, train = T.load_dataset, T.train

    def load_and_keep():
        made.extend(load())
        return made

    def profiled_train(*args, **kwargs):
        L.lib().resr_profile_begin()
        try:
            return train(*args, **kwargs)
        finally:
            torch.cuda.synchronize()
            buf = (L.ProfEntry * 8192)()
            n = int(L.lib().resr_profile_end(C.cast(buf, C.c_void_p), 8192))
            ids.extend(buf[i].kernel_id for i in range(n))

    def never(*args, **kwargs):
        raise AssertionError("the degradation stage ran in paired mode")
    monkeypatch.setattr(T, "load_dataset", load_and_keep)
    monkeypatch.setattr(T, "train", profiled_train)
    monkeypatch.setattr(T, "DegradationPrefetcher", never)
    monkeypatch.setattr(degrade, "sample_plan", never)
    monkeypatch.setattr(degrade, "run_plan", never)
    T.main()
    assert isinstance(made[0], D.PairedDeviceSource) and made[0].M == 4 and made[0].patch == 52 and made[0].scale == 4 and len(made[0]) == 2
    assert not isinstance(made[1], D.PairedDeviceSource) and not isinstance(made[2], D.PairedDeviceSource)
    # reset() of the epoch stages batch 0 again, next() of batch 0 stages batch 1: two launches inside train(), of this id alone in the 330xx block
    assert 0 < len(ids) < 8192 and ids.count(33001) == 2, ids.count(33001)
    assert not [i for i in ids if 33000 <= i < 34000 and i != 33001]
    ck = torch.load(tmp_path / "samples" / "paired_source_test" / "g_epoch_1.pth.tar", weights_only=False)
    assert ck["epoch"] == 1 and ck["optimizer"]["state"][0]["step"] == 2 and np.isfinite(ck["best_niqe"])
    scalars = [json.loads(l) for l in open(tmp_path / "samples" / "logs" / "paired_source_test" / "scalars.jsonl")]
    losses = [s["value"] for s in scalars if s["tag"] == "Train/Loss"]
    assert len(losses) == 2 and all(np.isfinite(v) and v > 0 for v in losses), losses
    # the loader path is built where the resident one is, and a missing LR directory is refused there too
    monkeypatch.setattr(T, "load_dataset", load)
    monkeypatch.setattr(config, "data_source", "paired_loader")
    from real_esrgan_pytorch_amd.dataset import PairedPrefetcher
    source = T.load_dataset()[0]
    assert isinstance(source, PairedPrefetcher) and len(source) == 2 and source.next()[1].shape == (2, 3, 208, 208)
    monkeypatch.setattr(config, "paired_lr_image_dir", "")
    with pytest.raises(ValueError, match="paired_lr_image_dir"):
        T.load_dataset()
