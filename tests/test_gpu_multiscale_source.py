"""-m gpu: `device_data.ImageCropSource` with multi-scale copies (scales / short_side) -- the arena against Pillow itself, the batches against
the loader twin (`dataset.CropImageDataset` with the same copies behind `CUDAPrefetcher` at num_workers=0) under the same seeds and
sampler over two passes, the source without copies against what it was, which launches happen when, and one epoch of train_realesrnet
with config.train_scales set.

Arena bytes and `hr` have no tolerance: the copies are Pillow's bytes (device_data.resample_u8_np restates its integer rule) and both paths
then evaluate device_data.crop_sample_np's arithmetic on them.  The blur kernels come from the unchanged resr_blur_kernels and meet the
bound tests/test_gpu_device_data.py derives for it: one fp32 ulp of the host tap, with the floor 2^-30 x the kernel's largest |tap|."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE, BATCH = 32, 4
SCALES, SHORT = (0.75, 1 / 3), 40
# below the window in both axes, in one, the window itself, above it, wider than one 64-column tile: 6 images, 24 table rows, 6 batches a pass
SIZES = [(32, 32), (7, 5), (50, 70), (96, 40), (33, 150), (121, 90)]
RESAMPLE_ID, CROP_ID, BLUR_ID = 33004, 33003, 33100


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
def images():
    rng = np.random.default_rng(1)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]


@pytest.fixture(scope="module")
def folder(tmp_path_factory, images):
    from PIL import Image
    path = tmp_path_factory.mktemp("multiscale")
    for i, a in enumerate(images):
        Image.fromarray(a).save(str(path / f"{i}.png"))
    return str(path)


def _profiled(fn, capacity=4096):
    """(fn(), the kernel ids of every launch inside it)."""
    from real_esrgan_pytorch_amd import _lib as L
    L.lib().resr_profile_begin()
    try:
        out = fn()
    finally:
        torch.cuda.synchronize()
        buf = (L.ProfEntry * capacity)()
        n = int(L.lib().resr_profile_end(C.cast(buf, C.c_void_p), capacity))
    assert n < capacity
    return out, [buf[i].kernel_id for i in range(n)]


def _passes(source, batches, passes=2):
    """What `passes` x (`batches` batches + the None that ends a pass) of next() give, with the host generators' state after each call."""
    out = []
    for epoch in range(passes):
        for _ in range(batches + 1):
            batch = source.next()
            out.append((None if batch is None else {k: v.clone() for k, v in batch.items()}, _host_state()))
        assert source.next() is None
        if epoch + 1 < passes:
            source.reset()
    torch.cuda.synchronize()
    return out


def _kernels_within_the_bound(got, want):
    g, w = got.cpu().numpy(), want.cpu().numpy()
    bound = np.maximum(np.spacing(np.abs(w)).astype(np.float64), 2.0 ** -30 * np.abs(w).max(axis=(1, 2), keepdims=True))
    return g.shape == w.shape and bool((np.abs(g.astype(np.float64) - w) <= bound).all())


def _same_batches(want, got, batches):
    for k, ((w, w_state), (g, g_state)) in enumerate(zip(want, got)):
        assert w_state == g_state, f"`random` / `np.random` differ after next() {k}"
        if k % (batches + 1) == batches:
            assert w is None and g is None
            continue
        assert g["hr"].shape == (BATCH, 3, TILE, TILE) and torch.equal(g["hr"].view(torch.int32), w["hr"].view(torch.int32)), k
        for name in ("kernel1", "kernel2", "sinc_kernel"):
            assert _kernels_within_the_bound(g[name], w[name]), (k, name)


def _check_arena(D, source, originals):
    """Rows 0..M-1 are the inputs' bytes, every copy row is Pillow's resize of its original; the table is the rule's."""
    from PIL import Image
    M = len(originals)
    table, arena = source.table_host, source.arena.cpu().numpy()
    assert table.shape == (M * 4, 3) and source.M == M * 4 and arena.size == int(table[-1, 0] + table[-1, 1] * table[-1, 2] * 3)
    assert np.array_equal(table, D._crop_table([a.shape[:2] for a in originals], [str(i) for i in range(M)], 10 ** 9, SCALES, SHORT))
    for row, (off, h, w) in enumerate(table.tolist()):
        original = originals[row % M]
        got = arena[off:off + h * w * 3].reshape(h, w, 3)
        if row < M:
            assert np.array_equal(got, original), row
            continue
        assert (h, w) == D.multiscale_sizes(original.shape[0], original.shape[1], SCALES, SHORT)[row // M - 1]
        assert np.array_equal(got, np.asarray(Image.fromarray(original).resize((w, h), Image.LANCZOS))), (row, h, w)


def test_from_arrays_holds_the_originals_and_pillows_copies(D, images):
    device = torch.device("cuda", 0)
    source, ids = _profiled(lambda: D.ImageCropSource.from_arrays(images, BATCH, TILE, device, scales=SCALES, short_side=SHORT))
    assert ids.count(RESAMPLE_ID) == 1 and ids.count(CROP_ID) == 1 and ids.count(BLUR_ID) == 1      # the copies: ONE launch; batch 0 is staged at once
    assert len(source) == 6 and source.T == TILE
    _check_arena(D, source, images)
    _, ids = _profiled(lambda: _passes(source, 6, passes=1))
    assert ids.count(RESAMPLE_ID) == 0 and ids.count(CROP_ID) == 5 and ids.count(BLUR_ID) == 5      # construction only; one crop launch a batch


def test_from_dir_makes_the_copies_in_bounded_groups(D, folder):
    """chunk_bytes of 2 KiB: the originals load in several chunks and the 18 copies go in several launches; the arena is the same."""
    from PIL import Image
    device = torch.device("cuda", 0)
    names = os.listdir(folder)
    originals = [np.asarray(Image.open(os.path.join(folder, n)).convert("RGB")) for n in names]
    source, ids = _profiled(lambda: D.ImageCropSource.from_dir(folder, BATCH, TILE, device, chunk_bytes=2048, scales=SCALES, short_side=SHORT))
    assert 2 <= ids.count(RESAMPLE_ID) <= 18
    _check_arena(D, source, originals)


def test_batches_are_the_loader_twins_over_two_passes(D, folder):
    from torch.utils.data import DataLoader, RandomSampler
    from real_esrgan_pytorch_amd import config
    from real_esrgan_pytorch_amd.dataset import CropImageDataset, CUDAPrefetcher
    device = torch.device("cuda", 0)
    data = CropImageDataset(folder, TILE, config.degradation_model_parameters_dict, SCALES, SHORT)
    assert len(data) == 24
    _seed(21)
    sampler = RandomSampler(data, generator=torch.Generator().manual_seed(21))
    want = _passes(CUDAPrefetcher(DataLoader(data, batch_size=BATCH, sampler=sampler, num_workers=0, drop_last=True), device), 6)
    _seed(21)
    sampler = RandomSampler(range(len(data)), generator=torch.Generator().manual_seed(21))
    source = D.ImageCropSource.from_dir(folder, BATCH, TILE, device, sampler=sampler, scales=SCALES, short_side=SHORT)
    assert len(source) == 6 and source.M == 24
    got = _passes(source, 6)
    _same_batches(want, got, 6)
    seen = [g["hr"] for g, _ in got if g is not None]
    assert len(seen) == 12 and not torch.equal(seen[0], seen[6])        # the second pass is another draw


def test_without_scales_the_source_is_what_it_was(D, folder, images):
    """No copies configured: the table is the originals', resr_resample_u8 is never launched, and draws and batches are the twin's without
    copies -- the same comparison tests/test_gpu_image_source.py makes."""
    from torch.utils.data import DataLoader, RandomSampler
    from real_esrgan_pytorch_amd import config
    from real_esrgan_pytorch_amd.dataset import CropImageDataset, CUDAPrefetcher
    device = torch.device("cuda", 0)
    data = CropImageDataset(folder, TILE, config.degradation_model_parameters_dict)
    _seed(22)
    sampler = RandomSampler(data, generator=torch.Generator().manual_seed(22))
    want = _passes(CUDAPrefetcher(DataLoader(data, batch_size=2, sampler=sampler, num_workers=0, drop_last=True), device), 3, passes=1)

    def make_and_run():
        _seed(22)
        sampler = RandomSampler(range(6), generator=torch.Generator().manual_seed(22))
        source = D.ImageCropSource.from_dir(folder, 2, TILE, device, sampler=sampler, scales=(), short_side=0)
        return source, _passes(source, 3, passes=1)
    (source, got), ids = _profiled(make_and_run)
    assert RESAMPLE_ID not in ids and ids.count(CROP_ID) == 3
    sizes = [tuple(r) for r in source.table_host[:, 1:].tolist()]
    assert source.M == 6 and sorted(sizes) == sorted(SIZES) and source.arena.numel() == 3 * sum(h * w for h, w in SIZES)
    assert np.array_equal(source.table_host, D._crop_table(sizes, [str(i) for i in range(6)], 10 ** 9))
    for k, ((w, w_state), (g, g_state)) in enumerate(zip(want, got)):
        assert w_state == g_state, k
        assert (w is None and g is None) or torch.equal(g["hr"].view(torch.int32), w["hr"].view(torch.int32)), k
    plain = D.ImageCropSource.from_arrays(images, 2, TILE, device)
    assert plain.M == 6 and plain.arena.numel() == source.arena.numel()


# ---- the train script ----------------------------------------------------------------------------------------------------------------
def test_train_realesrnet_epoch_with_train_scales(D, tmp_path, monkeypatch):
    """RESR_TRAIN_SCALES=0.5 (config.train_scales = "0.5"): 4 images and their 4 half-size copies, batch 2 -> M * 2 // 2 = 4 steps; the copies
    are made when the source is built, the training loop launches one crop_batch per step and no resample."""
    from real_esrgan_pytorch_amd import config
    from real_esrgan_pytorch_amd import train_realesrnet as T
    from tests.test_gpu_image_source import TRAIN_SIZES, _profiled as profiled_train, _tiny_image_run
    _tiny_image_run(tmp_path, monkeypatch, 0)
    monkeypatch.setattr(config, "train_scales", "0.5")
    monkeypatch.setattr(config, "exp_name", "multiscale_test")
    made, ids, built = [], [], []
    load = T.load_dataset

    def load_and_keep():
        out, seen = _profiled(load)
        built.extend(seen)
        made.extend(out)
        return made
    monkeypatch.setattr(T, "load_dataset", load_and_keep)
    profiled_train(monkeypatch, T, ids)
    T.main()
    M = len(TRAIN_SIZES)
    source = made[0]
    assert isinstance(source, D.ImageCropSource) and source.M == 2 * M and len(source) == M * 2 // 2
    assert [tuple(r) for r in source.table_host[M:, 1:].tolist()] == [(h // 2, w // 2) for h, w in (tuple(r) for r in source.table_host[:M, 1:].tolist())]
    assert built.count(RESAMPLE_ID) == 1 and ids.count(RESAMPLE_ID) == 0 and ids.count(CROP_ID) == 4 and ids.count(BLUR_ID) == 4
    ck = torch.load(tmp_path / "samples" / "multiscale_test" / "g_epoch_1.pth.tar", weights_only=False)
    assert ck["epoch"] == 1 and ck["optimizer"]["state"][0]["step"] == 4
    scalars = [json.loads(l) for l in open(tmp_path / "samples" / "logs" / "multiscale_test" / "scalars.jsonl")]
    losses = [s["value"] for s in scalars if s["tag"] == "Train/Loss"]
    assert len(losses) == 4 and all(np.isfinite(v) and v > 0 for v in losses), losses
    monkeypatch.setattr(T, "load_dataset", load)                        # the loader twin is sized the same way
    monkeypatch.setattr(config, "data_source", "images_loader")
    assert len(T.load_dataset()[0]) == 4
