"""-m gpu: `device_data.ImageCropSource` against its loader twin (`dataset.CropImageDataset` behind `CUDAPrefetcher` at num_workers=0)
under the same seeds and sampler -- the same windows bit for bit over two passes, the same host draws after every next() --, against
`DeviceTileSource` on a set of T x T tiles, and one epoch of train_realesrnet and of train_realesrgan with config.data_source = "images".

`hr` has no tolerance: both paths evaluate device_data.crop_sample_np's arithmetic on the same bytes.  The blur kernels come from the
unchanged resr_blur_kernels and meet the bound tests/test_gpu_device_data.py derives for it: one fp32 ulp of the host tap, with the
floor 2^-30 x the kernel's largest |tap|."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE, BATCH = 16, 4
# below the window in both axes, in one, exactly the window, and above it: 12 images, 3 batches a pass
SIZES = [(16, 16), (7, 5), (30, 38), (64, 64), (9, 40), (33, 12), (16, 37), (1, 1), (17, 16), (25, 31), (3, 70), (20, 20)]


@pytest.fixture(scope="module")
def D():
    from real_esrgan_pytorch_amd import device_data
    return device_data


def _seed(s):
    random.seed(s)
    np.random.seed(s)


def _host_state():
    a, b = random.getstate(), np.random.get_state()
    return a, (b[0], b[1].tolist(), b[2], b[3], b[4])


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from PIL import Image
    path = tmp_path_factory.mktemp("images")
    rng = np.random.default_rng(1)
    for i, (h, w) in enumerate(SIZES):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(str(path / f"{i}.png"))
    return str(path)


def _two_passes(source):
    """What 2 x (3 batches + the None that ends a pass) of next() give, with the host generators' state after each call."""
    out = []
    for epoch in range(2):
        for _ in range(4):
            batch = source.next()
            out.append((None if batch is None else {k: v.clone() for k, v in batch.items()}, _host_state()))
        assert source.next() is None                                   # it stays ended
        if epoch == 0:
            source.reset()
    torch.cuda.synchronize()
    return out


def _kernels_within_the_bound(got, want):
    g, w = got.cpu().numpy(), want.cpu().numpy()
    bound = np.maximum(np.spacing(np.abs(w)).astype(np.float64), 2.0 ** -30 * np.abs(w).max(axis=(1, 2), keepdims=True))
    return g.shape == w.shape and bool((np.abs(g.astype(np.float64) - w) <= bound).all())


def test_source_gives_the_loader_twins_batches_over_two_passes(D, folder):
    from torch.utils.data import DataLoader, RandomSampler
    from real_esrgan_pytorch_amd import config
    from real_esrgan_pytorch_amd.dataset import CropImageDataset, CUDAPrefetcher
    device = torch.device("cuda", 0)
    data = CropImageDataset(folder, TILE, config.degradation_model_parameters_dict)
    _seed(11)
    sampler = RandomSampler(data, generator=torch.Generator().manual_seed(11))
    want = _two_passes(CUDAPrefetcher(DataLoader(data, batch_size=BATCH, sampler=sampler, num_workers=0, drop_last=True), device))
    _seed(11)
    sampler = RandomSampler(range(len(data)), generator=torch.Generator().manual_seed(11))
    source = D.ImageCropSource.from_dir(folder, BATCH, TILE, device, sampler=sampler)
    assert len(source) == 3 and source.M == 12 and source.T == TILE and isinstance(source.original_dataloader.sampler, RandomSampler)
    files = os.listdir(folder)
    assert [tuple(r) for r in source.table_host[:, 1:].tolist()] == [SIZES[int(f.split(".")[0])] for f in files]      # os.listdir order
    assert source.arena.numel() == 3 * sum(h * w for h, w in SIZES) and source.table_host[0, 0] == 0
    got = _two_passes(source)
    seen = []
    for k, ((w, w_state), (g, g_state)) in enumerate(zip(want, got)):
        assert w_state == g_state, f"`random` / `np.random` differ after next() {k}"
        if k % 4 == 3:
            assert w is None and g is None                             # the fourth next() of a pass ends it
            continue
        assert set(g) == set(w) == {"hr", "kernel1", "kernel2", "sinc_kernel"}
        assert all(v.is_cuda and v.dtype == torch.float32 for v in g.values())
        assert g["hr"].shape == (BATCH, 3, TILE, TILE) and torch.equal(g["hr"].view(torch.int32), w["hr"].view(torch.int32)), k
        for name in ("kernel1", "kernel2", "sinc_kernel"):
            assert g[name].shape == (BATCH, 21, 21) and _kernels_within_the_bound(g[name], w[name]), (k, name)
        seen.append(g["hr"])
    assert len(seen) == 6 and not torch.equal(seen[0], seen[3])         # the second pass is another draw, not the first again


def test_on_a_tile_set_the_source_is_the_tile_source(D):
    """8 tiles of exactly the window: no crop draw is made, so the draw sequence, the windows and the kernels are DeviceTileSource's."""
    from torch.utils.data import RandomSampler
    device = torch.device("cuda", 0)
    tiles = np.random.default_rng(3).integers(0, 256, (8, TILE, TILE, 3), dtype=np.uint8)

    def take(make):
        _seed(5)
        source = make(RandomSampler(range(8), generator=torch.Generator().manual_seed(5)))
        out = []
        for _ in range(3):                                              # 2 batches and the None
            batch = source.next()
            out.append((None if batch is None else {k: v.clone() for k, v in batch.items()}, _host_state()))
        torch.cuda.synchronize()
        return out
    want = take(lambda sampler: D.DeviceTileSource.from_array(tiles, BATCH, device, sampler=sampler))
    got = take(lambda sampler: D.ImageCropSource.from_arrays(list(tiles), BATCH, TILE, device, sampler=sampler))
    for k, ((w, w_state), (g, g_state)) in enumerate(zip(want, got)):
        assert w_state == g_state, k
        if k == 2:
            assert w is None and g is None
            continue
        for name in ("hr", "kernel1", "kernel2", "sinc_kernel"):
            assert torch.equal(g[name].view(torch.int32), w[name].view(torch.int32)), (k, name)
    with pytest.raises(IndexError):
        D.ImageCropSource.from_arrays(list(tiles), 2, TILE, device, sampler=[0, 8])      # an index past the images never reaches the kernel


# ---- the train scripts -------------------------------------------------------------------------------------------------------------
def _smooth_png(path, h, w, seed):
    from PIL import Image
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    x = F.interpolate(torch.rand(1, 3, h // 8 + 1, w // 8 + 1, generator=g), size=(h, w), mode="bicubic").clamp(0, 1)
    x = (0.85 * x + 0.15 * torch.rand(1, 3, h, w, generator=g)).clamp(0, 1)
    Image.fromarray((x[0].permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(path)


TRAIN_SIZES = [(224, 224), (200, 260), (300, 240), (180, 190)]          # the window itself; padded below; larger; padded in both axes


def _tiny_image_run(tmp_path, monkeypatch, pool_size):
    """4 training images of mixed sizes around the window 224 (image_size 208: the sizes the degradation stage's own epoch tests use), 2
    valid and 2 test images of 224, batch 2, one epoch of two steps, the compact generator, config.data_source = "images"."""
    from PIL import Image
    from real_esrgan_pytorch_amd import config, imgproc
    os.makedirs(tmp_path / "train")
    for i, (h, w) in enumerate(TRAIN_SIZES):
        _smooth_png(str(tmp_path / "train" / f"{i}.png"), h, w, 30 + i)
    for k, (sub, n) in enumerate((("valid", 2), ("test_hr", 2))):
        os.makedirs(tmp_path / sub)
        for i in range(n):
            _smooth_png(str(tmp_path / sub / f"{i}.png"), 224, 224, 10 * k + i)
    os.makedirs(tmp_path / "test_lr")
    for i in range(2):
        hr = imgproc.read_image_rgb(str(tmp_path / "test_hr" / f"{i}.png"))
        lr = np.clip(imgproc.image_resize(hr, 0.25), 0, 1)
        Image.fromarray((lr * 255).round().astype(np.uint8)).save(str(tmp_path / "test_lr" / f"{i}.png"))
    here = os.path.dirname(os.path.abspath(__file__))
    settings = dict(train_image_dir=str(tmp_path / "train"), valid_image_dir=str(tmp_path / "valid"),
                    test_lr_image_dir=str(tmp_path / "test_lr"), test_hr_image_dir=str(tmp_path / "test_hr"),
                    image_size=208, train_tile=224, batch_size=2, num_workers=0, epochs=1, print_frequency=1, resume="", pretrained_g="",
                    lr_scheduler_step_size=1, exp_name="image_source_test", model_lr=2e-4, model_betas=(0.9, 0.99),
                    ema_model_weight_decay=0.999, niqe_model_path=os.path.join(here, "golden", "niqe_model.mat"),
                    device=torch.device("cuda", 0), g_arch="compact", compact_num_conv=2, compact_act_type="prelu",
                    precision="fast", output_parity=False, inference_precision="exact16", upscale_factor=4, data_source="images",
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


def _source_launches(ids, pool_size):
    """reset() of the epoch stages batch 0 again, next() of batch 0 stages batch 1: per training step one crop_batch and one blur_kernels
    launch inside train(), no tile_batch and no pair_batch; with the pool, one exchange launch per step on top."""
    assert ids.count(33003) == 2 and ids.count(33100) == 2, (ids.count(33003), ids.count(33100))
    assert ids.count(33000) == 0 and ids.count(33001) == 0
    assert ids.count(33002) == (2 if pool_size else 0), ids.count(33002)


@pytest.mark.parametrize("pool_size", [0, 2])
def test_train_realesrnet_epoch_from_the_image_source(D, tmp_path, monkeypatch, pool_size):
    from real_esrgan_pytorch_amd import config
    from real_esrgan_pytorch_amd import train_realesrnet as T
    from real_esrgan_pytorch_amd.dataset import CropImageDataset, CUDAPrefetcher
    _tiny_image_run(tmp_path, monkeypatch, pool_size)
    made, ids = [], []
    load = T.load_dataset

    def load_and_keep():
        made.extend(load())
        return made
    monkeypatch.setattr(T, "load_dataset", load_and_keep)
    _profiled(monkeypatch, T, ids)
    T.main()
    assert isinstance(made[0], D.ImageCropSource) and made[0].M == 4 and made[0].T == 224 and len(made[0]) == 2
    assert sorted(tuple(r) for r in made[0].table_host[:, 1:].tolist()) == sorted(TRAIN_SIZES)
    assert not isinstance(made[1], D.ImageCropSource) and not isinstance(made[2], D.ImageCropSource)
    _source_launches(ids, pool_size)
    assert (isinstance(T._PAIR_POOL, D.PairPool) and T._PAIR_POOL.filled == 2) if pool_size else T._PAIR_POOL is None
    ck = torch.load(tmp_path / "samples" / "image_source_test" / "g_epoch_1.pth.tar", weights_only=False)
    assert ck["epoch"] == 1 and ck["optimizer"]["state"][0]["step"] == 2 and np.isfinite(ck["best_niqe"])
    scalars = [json.loads(l) for l in open(tmp_path / "samples" / "logs" / "image_source_test" / "scalars.jsonl")]
    losses = [s["value"] for s in scalars if s["tag"] == "Train/Loss"]
    assert len(losses) == 2 and all(np.isfinite(v) and v > 0 for v in losses), losses
    if pool_size:
        return
    # the loader twin is built where the resident source is, and a window below image_size is refused there too
    monkeypatch.setattr(T, "load_dataset", load)
    monkeypatch.setattr(config, "data_source", "images_loader")
    source = T.load_dataset()[0]
    assert isinstance(source, CUDAPrefetcher) and isinstance(source.original_dataloader.dataset, CropImageDataset) and len(source) == 2
    assert source.next()["hr"].shape == (2, 3, 224, 224)
    monkeypatch.setattr(config, "train_tile", 207)
    for name in ("images", "images_loader"):
        monkeypatch.setattr(config, "data_source", name)
        with pytest.raises(ValueError, match="train_tile=207.*image_size=208"):
            T.load_dataset()


def test_train_realesrgan_epoch_from_the_image_source_with_the_pool(D, tmp_path, monkeypatch):
    """The GAN script takes the source through train_realesrnet's load_dataset / train_pairs: the same launches per step, and with
    config.pair_pool_size = the batch size on top, one exchange launch per step."""
    from real_esrgan_pytorch_amd import config
    from real_esrgan_pytorch_amd import train_realesrgan as G
    from real_esrgan_pytorch_amd import train_realesrnet as T
    _tiny_image_run(tmp_path, monkeypatch, 2)
    monkeypatch.setattr(config, "model_lr", 1e-4)
    ids = []
    _profiled(monkeypatch, G, ids)
    G.main()
    _source_launches(ids, 2)
    assert isinstance(T._PAIR_POOL, D.PairPool) and T._PAIR_POOL.filled == 2 and tuple(T._PAIR_POOL.pool_hr.shape) == (2, 3, 208, 208)
    g1 = torch.load(tmp_path / "samples" / "image_source_test" / "g_epoch_1.pth.tar", weights_only=False)
    assert g1["epoch"] == 1 and g1["optimizer"]["state"][0]["step"] == 2 and np.isfinite(g1["best_niqe"])
    assert (tmp_path / "samples" / "image_source_test" / "d_epoch_1.pth.tar").exists()
    scalars = [json.loads(l) for l in open(tmp_path / "samples" / "logs" / "image_source_test" / "scalars.jsonl")]
    for tag in ("Train/G_Loss", "Train/D_Loss", "Train/Pixel_Loss"):
        values = [s["value"] for s in scalars if s["tag"] == tag]
        assert len(values) == 2 and all(np.isfinite(v) and v > 0 for v in values), (tag, values)
