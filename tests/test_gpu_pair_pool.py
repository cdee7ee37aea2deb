"""-m gpu: `device_data.PairPool` against its CPU mirror `HostPairPool` (the same rule over `pool_exchange_np`) under the same seed --
the same batches bit for bit --, `reset()`, a consumer on another stream, the source's batches and `random`'s state with the pool on
and off, and one epoch of train_realesrnet and of train_realesrgan with config.pair_pool_size set: one launch of id 33002 per step.

Nothing here has a tolerance: the pool moves bits."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch

from tests.test_pair_pool_surface import Scripted

pytestmark = pytest.mark.gpu

POOL_EXCHANGE_ID = 33002


@pytest.fixture(scope="module")
def D():
    from real_esrgan_pytorch_amd import device_data
    return device_data


def _word_batches(count, B, seed, lr_shape=(3, 5, 5), hr_shape=(3, 20, 20)):
    """`count` batches of random 32-bit patterns as float32 (NaNs and subnormals among them)."""
    rng = np.random.default_rng(seed)
    words = lambda *shape: rng.integers(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32).view(np.float32)
    return [(words(B, *lr_shape), words(B, *hr_shape)) for _ in range(count)]


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def test_pair_pool_gives_its_cpu_mirrors_batches_bit_for_bit(D):
    Q, B = 8, 4
    steps = 3 * Q // B
    batches = _word_batches(steps, B, 17)
    device = torch.device("cuda", 0)
    pool, mirror = D.PairPool(Scripted(batches, device), Q, seed=6), D.HostPairPool(Scripted(batches), Q, seed=6)
    for step in range(steps):
        (g_lr, g_hr, g_batch), (w_lr, w_hr, w_batch) = pool.next(), mirror.next()
        assert g_lr.is_cuda and g_lr.shape == w_lr.shape and g_hr.shape == w_hr.shape and g_lr.dtype == g_hr.dtype == torch.float32
        assert np.array_equal(_bits(g_lr), _bits(w_lr)) and np.array_equal(_bits(g_hr), _bits(w_hr)), step
        assert g_batch["index"] == w_batch["index"] == step             # the incoming batch's dictionary, with the incoming tensors
        assert np.array_equal(_bits(g_batch["lr"]), batches[step][0].view(np.int32)) and np.array_equal(_bits(g_batch["hr"]), batches[step][1].view(np.int32))
        if step < Q // B:
            assert g_lr is g_batch["lr"] and g_hr is g_batch["hr"]      # the fill hands the source's own tensors out
        else:
            assert g_lr.data_ptr() != g_batch["lr"].data_ptr() and not np.array_equal(_bits(g_lr), batches[step][0].view(np.int32))
        assert pool.filled == mirror.filled == min(Q, (step + 1) * B)
    assert pool.next() is None and mirror.next() is None
    assert tuple(pool.pool_lr.shape) == (Q, 3, 5, 5) and tuple(pool.pool_hr.shape) == (Q, 3, 20, 20) and pool.pool_lr.device == device
    assert np.array_equal(_bits(pool.pool_lr), _bits(mirror.pool_lr)) and np.array_equal(_bits(pool.pool_hr), _bits(mirror.pool_hr))
    pool.attach(Scripted(_word_batches(1, B, 0, lr_shape=(3, 4, 4)), device))
    with pytest.raises(ValueError, match="after the pool was sized"):
        pool.next()
    for size, kwargs, word in ((6, {}, "not a multiple of the batch size 4"), (2, {}, "below the batch size 4"), (8, dict(max_bytes=1000), "above max_bytes=1000")):
        bad = D.PairPool(Scripted(batches, device), size, **kwargs)
        with pytest.raises(ValueError, match=word):
            bad.next()
        assert bad.pool_lr is None and bad.pool_hr is None              # refused before any allocation


def test_reset_keeps_the_contents_and_the_fill_pointer(D):
    Q, B = 8, 2
    batches = _word_batches(3, B, 23)
    device = torch.device("cuda", 0)
    source = Scripted(batches, device)
    pool = D.PairPool(source, Q, seed=0)
    for _ in range(3):
        pool.next()
    assert pool.next() is None and pool.filled == 6
    held = (_bits(pool.pool_lr[:6]).copy(), _bits(pool.pool_hr[:6]).copy())
    assert np.array_equal(held[0], np.concatenate([b[0] for b in batches]).view(np.int32))      # slots ptr..ptr+B-1, batch after batch
    pool.reset()
    assert source.resets == 1 and pool.filled == 6
    assert np.array_equal(_bits(pool.pool_lr[:6]), held[0]) and np.array_equal(_bits(pool.pool_hr[:6]), held[1])
    more = _word_batches(2, B, 24)
    pool.attach(Scripted(more, device))                                 # the next epoch's source: the fill goes on where it stopped
    lr, hr, _batch = pool.next()
    assert pool.filled == 8 and np.array_equal(_bits(lr), more[0][0].view(np.int32))
    assert np.array_equal(_bits(pool.pool_lr[:6]), held[0]) and np.array_equal(_bits(pool.pool_lr[6:]), more[0][0].view(np.int32))
    lr, hr, _batch = pool.next()                                        # full: an exchange
    slots = random.Random(0).sample(range(Q), B)
    everything = np.concatenate([held[1], more[0][1].view(np.int32)])
    assert np.array_equal(_bits(hr), everything[slots])


def test_a_consumer_on_another_stream_reads_complete_pairs(D):
    """No device-wide synchronisation between the source's launch, the pool's and the consumer's reads: the events alone order them.  16
    samples with a 256 x 256 HR patch per batch, so the launches are still running when next() returns.  Two batches fill the pool of 32,
    two are exchanged; what comes out is judged against the definition of the sample that the drawn slot held."""
    rng = np.random.default_rng(5)
    sizes = [(64, 64), (70, 65), (64, 91), (80, 80)]
    lr = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    hr = [rng.integers(0, 256, (4 * h, 4 * w, 3), dtype=np.uint8) for h, w in sizes]
    B, Q, seed = 16, 32, 9
    order = [i % 4 for i in range(4 * B)]
    random.seed(21)
    plans = [(i,) + D.sample_paired_draw(sizes[i][0], sizes[i][1], 64) for i in order]        # sample n's draw, n in the source's order
    random.seed(21)
    source = D.PairedDeviceSource.from_arrays(hr, lr, B, 64, 4, torch.device("cuda", 0), sampler=order)
    pool = D.PairPool(source, Q, seed=seed)
    consumer = torch.cuda.Stream()
    kept = []
    with torch.cuda.stream(consumer):
        for k in range(4):
            lr_b, hr_b, batch = pool.next()
            assert batch["index"] == k
            kept.append((lr_b.clone(), hr_b.clone()))                   # enqueued on the consumer stream, right behind the exchange
            del lr_b, hr_b, batch
        assert pool.next() is None
    consumer.synchronize()                                              # this stream only
    mirror, held = random.Random(seed), list(range(Q))                  # which sample each slot holds
    handed = [list(range(B)), list(range(B, 2 * B))]
    for k in (2, 3):
        slots = mirror.sample(range(Q), B)
        handed.append([held[s] for s in slots])
        for b, s in enumerate(slots):
            held[s] = k * B + b
    assert sorted([n for ids in handed[2:] for n in ids] + held) == list(range(4 * B))
    for k, (lr_b, hr_b) in enumerate(kept):
        lr_b, hr_b = lr_b.cpu().numpy(), hr_b.cpu().numpy()
        for b in (0, 1, 7, 15):
            i, top, left, code = plans[handed[k][b]]
            want_lr, want_hr = D.paired_sample_np(hr[i], lr[i], top, left, code, 64, 4)
            assert np.array_equal(lr_b[b], want_lr) and np.array_equal(hr_b[b], want_hr), (k, b)
    torch.cuda.synchronize()
    pool_hr = pool.pool_hr.cpu().numpy()
    for s in (0, 13, 31):
        i, top, left, code = plans[held[s]]
        assert np.array_equal(pool_hr[s], D.paired_sample_np(hr[i], lr[i], top, left, code, 64, 4)[1]), s


def test_the_source_hands_out_the_same_batches_with_the_pool_on_and_off(D):
    """The pool draws nothing from `random`: under one seed the resident paired source gives the same batches, and leaves `random` in the
    same state after every next(), whether or not a pool stands behind it."""
    from torch.utils.data import RandomSampler
    rng = np.random.default_rng(8)
    sizes = [(9, 9), (12, 10), (9, 15), (11, 11), (10, 9), (14, 9), (9, 12), (13, 13)]
    lr = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    hr = [rng.integers(0, 256, (2 * h, 2 * w, 3), dtype=np.uint8) for h, w in sizes]
    device = torch.device("cuda", 0)

    def source():
        random.seed(31)
        sampler = RandomSampler(range(len(sizes)), generator=torch.Generator().manual_seed(31))
        return D.PairedDeviceSource.from_arrays(hr, lr, 2, 9, 2, device, sampler=sampler)

    def passes(src):
        out = []
        for epoch in range(2):
            for _ in range(5):                                          # 4 batches and the None that ends the pass
                item = src.next()
                out.append((None if item is None else (_bits(item[2]["lr"]).copy(), _bits(item[2]["hr"]).copy(), item[2]["index"]), random.getstate()))
            src.reset()
        return out
    np_before, torch_before = np.random.get_state(), torch.get_rng_state()
    want = passes(source())
    pool = D.PairPool(source(), 4, seed=2)
    got = passes(pool)
    assert pool.filled == 4 and len(pool) == 4 and pool.original_dataloader is pool.source.original_dataloader
    for k, ((w, w_state), (g, g_state)) in enumerate(zip(want, got)):
        assert w_state == g_state, f"`random` differs after next() {k}"
        if k % 5 == 4:
            assert w is None and g is None
            continue
        assert np.array_equal(w[0], g[0]) and np.array_equal(w[1], g[1]) and w[2] == g[2] == k % 5, k      # what entered the pool
    now = np.random.get_state()
    assert now[0] == np_before[0] and np.array_equal(now[1], np_before[1]) and torch.equal(torch.get_rng_state(), torch_before)


# ---- the train scripts -------------------------------------------------------------------------------------------------------------
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


def _smooth_png(path, size, seed):
    from PIL import Image
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    x = F.interpolate(torch.rand(1, 3, size // 8, size // 8, generator=g), size=(size, size), mode="bicubic").clamp(0, 1)
    x = (0.85 * x + 0.15 * torch.rand(1, 3, size, size, generator=g)).clamp(0, 1)
    Image.fromarray((x[0].permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(path)


def _tiny_paired_run(tmp_path, monkeypatch, pool_size):
    """4 training pairs (LR sides 52..70, so image_size 208 gives the LR patch 52), 2 valid and 2 test images of 224, batch 2, one epoch of
    two steps, the compact generator, config.data_source = "paired", config.pair_pool_size = pool_size."""
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
                    lr_scheduler_step_size=1, exp_name="pair_pool_test", model_lr=2e-4, model_betas=(0.9, 0.99),
                    ema_model_weight_decay=0.999, niqe_model_path=os.path.join(here, "golden", "niqe_model.mat"),
                    device=torch.device("cuda", 0), g_arch="compact", compact_num_conv=2, compact_act_type="prelu",
                    precision="fast", output_parity=False, inference_precision="exact16", upscale_factor=4, data_source="paired",
                    pair_pool_size=pool_size,
                    resume_d="", resume_g="", pixel_weight=1.0, adversarial_weight=0.1, content_weight=[0.1, 0.1, 1.0, 1.0, 1.0],
                    lr_scheduler_milestones=[1], lr_scheduler_gamma=0.5,
                    feature_model_extractor_nodes=["features.2", "features.7", "features.16", "features.25", "features.34"],
                    feature_model_normalize_mean=[0.485, 0.456, 0.406], feature_model_normalize_std=[0.229, 0.224, 0.225])
    for k, v in settings.items():
        monkeypatch.setattr(config, k, v, raising=False)
    monkeypatch.chdir(tmp_path)


def _profiled(monkeypatch, module, ids, capacity=32768):
    """module.train under the profiling record: the kernel ids of every launch inside it go to `ids`."""
    from real_esrgan_pytorch_amd import _lib as L
    train = module.train

    def profiled_train(*args, **kwargs):
        L.lib().resr_profile_begin()
        try:
            return train(*args, **kwargs)
        finally:
            torch.cuda.synchronize()
            buf = (L.ProfEntry * capacity)()
            n = int(L.lib().resr_profile_end(C.cast(buf, C.c_void_p), capacity))
            assert 0 < n < capacity
            ids.extend(buf[i].kernel_id for i in range(n))
    monkeypatch.setattr(module, "train", profiled_train)


@pytest.mark.parametrize("pool_size", [2, 0])
def test_train_realesrnet_epoch_with_the_pool(D, tmp_path, monkeypatch, pool_size):
    """Batch 2, pool 2: step 1 fills the pool (the store form), step 2 exchanges -- one launch of id 33002 per step.  Pool 0: none."""
    from real_esrgan_pytorch_amd import train_realesrnet as T
    _tiny_paired_run(tmp_path, monkeypatch, pool_size)
    monkeypatch.setattr(T, "_PAIR_POOL", "a pool an earlier run left")  # main() clears it
    ids = []
    _profiled(monkeypatch, T, ids)
    T.main()
    assert ids.count(POOL_EXCHANGE_ID) == (2 if pool_size else 0), ids.count(POOL_EXCHANGE_ID)
    assert ids.count(33001) == 2                                        # the source's own launches, as with the pool off
    if pool_size:
        assert isinstance(T._PAIR_POOL, D.PairPool) and T._PAIR_POOL.filled == T._PAIR_POOL.size == 2
        assert tuple(T._PAIR_POOL.pool_lr.shape) == (2, 3, 52, 52) and tuple(T._PAIR_POOL.pool_hr.shape) == (2, 3, 208, 208)
        assert isinstance(T._PAIR_POOL.source, D.PairedDeviceSource)
    else:
        assert T._PAIR_POOL is None
    ck = torch.load(tmp_path / "samples" / "pair_pool_test" / "g_epoch_1.pth.tar", weights_only=False)
    assert ck["epoch"] == 1 and ck["optimizer"]["state"][0]["step"] == 2 and np.isfinite(ck["best_niqe"])
    assert all(torch.isfinite(v).all() for v in ck["state_dict"].values() if torch.is_tensor(v) and v.is_floating_point())
    scalars = [json.loads(l) for l in open(tmp_path / "samples" / "logs" / "pair_pool_test" / "scalars.jsonl")]
    losses = [s["value"] for s in scalars if s["tag"] == "Train/Loss"]
    assert len(losses) == 2 and all(np.isfinite(v) and v > 0 for v in losses), losses


@pytest.mark.parametrize("pool_size", [2, 0])
def test_train_realesrgan_epoch_with_the_pool(D, tmp_path, monkeypatch, pool_size):
    """The GAN script reaches the pool through train_realesrnet.train_pairs: the same count, one launch of id 33002 per step."""
    from real_esrgan_pytorch_amd import config
    from real_esrgan_pytorch_amd import train_realesrgan as G
    from real_esrgan_pytorch_amd import train_realesrnet as T
    _tiny_paired_run(tmp_path, monkeypatch, pool_size)
    monkeypatch.setattr(T, "_PAIR_POOL", "a pool an earlier run left")
    monkeypatch.setattr(config, "model_lr", 1e-4)
    ids = []
    _profiled(monkeypatch, G, ids)
    G.main()
    assert ids.count(POOL_EXCHANGE_ID) == (2 if pool_size else 0), ids.count(POOL_EXCHANGE_ID)
    assert ids.count(33001) == 2
    assert (isinstance(T._PAIR_POOL, D.PairPool) and T._PAIR_POOL.filled == 2) if pool_size else T._PAIR_POOL is None
    g1 = torch.load(tmp_path / "samples" / "pair_pool_test" / "g_epoch_1.pth.tar", weights_only=False)
    assert g1["epoch"] == 1 and g1["optimizer"]["state"][0]["step"] == 2 and np.isfinite(g1["best_niqe"])
    assert all(torch.isfinite(v).all() for v in g1["state_dict"].values() if torch.is_tensor(v) and v.is_floating_point())
    assert (tmp_path / "samples" / "pair_pool_test" / "d_epoch_1.pth.tar").exists()
    scalars = [json.loads(l) for l in open(tmp_path / "samples" / "logs" / "pair_pool_test" / "scalars.jsonl")]
    for tag in ("Train/G_Loss", "Train/D_Loss", "Train/Pixel_Loss"):
        values = [s["value"] for s in scalars if s["tag"] == tag]
        assert len(values) == 2 and all(np.isfinite(v) and v > 0 for v in values), (tag, values)
