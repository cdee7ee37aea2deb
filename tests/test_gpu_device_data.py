"""-m gpu: the device-resident data source -- resr_tile_batch and resr_blur_kernels against their host definitions
(device_data.augment_np, blur_kernels_from_params_np), `DeviceTileSource` against the loader path under the same seeds, and one
epoch of train_realesrnet fed by it.

The blur-kernel bound is derived, not measured: the kernel and the definition evaluate the same float64 formulas with different
summation orders, inverses and libm routines, about 1e-15 relative, so the two fp32 casts differ by at most one ulp of the host
tap; taps near the zeros of J1 get the floor 2^-30 x the kernel's largest |tap|, 64 times below one fp32 rounding of the largest
product in the filter that consumes the kernel.  Padding taps and the delta kernel are exact.

Measured on an MI355X (printed by test_blur_kernels_match_the_host_definition): see DESIGN.md, "Device-resident data source"."""
import ctypes as C
import json
import math
import os
import random

import numpy as np
import pytest
import torch

from tests import gpu_util

pytestmark = pytest.mark.gpu

PI = math.pi


@pytest.fixture(scope="module")
def D():
    from real_esrgan_pytorch_amd import device_data
    return device_data


@pytest.fixture(scope="module")
def L():
    from real_esrgan_pytorch_amd import _lib
    return _lib


def _seed(s):
    random.seed(s)
    np.random.seed(s)


def _host_state():
    a, b = random.getstate(), np.random.get_state()
    return a, (b[0], b[1].tolist(), b[2], b[3], b[4])


def _launch_ids(L, fn):
    lib = L.lib()
    lib.resr_profile_begin()
    try:
        fn()
    finally:
        torch.cuda.synchronize()
        buf = (L.ProfEntry * 64)()
        n = int(lib.resr_profile_end(C.cast(buf, C.c_void_p), 64))
    return [buf[i].kernel_id for i in range(n)]


# ---- resr_tile_batch -------------------------------------------------------------------------------------------------------------
M_TILES, BATCH = 5, 16
INDEX = [4, 0, 1, 4, 2, 3, 3, 0, 4, 1, 2, 2, 0, 4, 3, 1]      # repeated indices, M - 1 first and among them
CODES = [(7 * b + 3) % 16 for b in range(BATCH)]              # every one of the 16 codes, not in index order


@pytest.mark.parametrize("side", [5, 6, 33, 70])      # odd; even; one past the 32-pixel LDS tile; even and not a multiple of it
def test_tile_batch_is_augment_np_bit_for_bit(D, L, side):
    assert sorted(CODES) == list(range(16)) and max(INDEX) == M_TILES - 1
    tiles = np.random.default_rng(side).integers(0, 256, (M_TILES, side, side, 3), dtype=np.uint8)
    tiles[0, 0, 0] = (0, 255, 1)
    want = np.stack([D.augment_np(tiles[i], c).numpy() for i, c in zip(INDEX, CODES)])
    out = gpu_util.Out(BATCH * 3 * side * side, np.float32)
    t, idx, aug = gpu_util.dev(tiles), gpu_util.dev(np.asarray(INDEX, np.int32)), gpu_util.dev(np.asarray(CODES, np.uint8))
    ids = _launch_ids(L, lambda: L.check(L.lib().resr_tile_batch(L.ptr(t), L.ptr(idx), L.ptr(aug), M_TILES, BATCH, side, C.c_void_p(out.ptr),
                                                                   L.stream_ptr()), "resr_tile_batch"))
    assert ids == [33000], ids                                        # one launch, under its profiling id
    got = out.read().reshape(want.shape)
    bad = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
    assert bad.size == 0, (side, bad.size, np.unravel_index(bad[0], want.shape), got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])
    again = D.tile_batch(t, idx, aug)                                 # the Python wrapper, the same bits
    torch.cuda.synchronize()
    assert np.array_equal(again.cpu().numpy().view(np.int32), want.view(np.int32))


def test_tile_batch_reads_tiles_past_2_31_bytes(D):
    """M * T * T * 3 above 2^31 (a real set is): the last tile starts past the reach of a 32-bit offset."""
    side = 64
    M = 2 ** 31 // (side * side * 3) + 2
    tiles = torch.zeros(M, side, side, 3, dtype=torch.uint8, device="cuda")
    assert (M - 1) * side * side * 3 > 2 ** 31
    last = np.random.default_rng(1).integers(1, 256, (side, side, 3), dtype=np.uint8)
    tiles[M - 1] = gpu_util.dev(last)
    index, codes = [M - 1, 0, M - 1], [0, 5, 11]
    got = D.tile_batch(tiles, gpu_util.dev(np.asarray(index, np.int32)), gpu_util.dev(np.asarray(codes, np.uint8)))
    torch.cuda.synchronize()
    assert torch.equal(got[0].cpu(), D.augment_np(last, 0)) and torch.equal(got[2].cpu(), D.augment_np(last, 11))
    assert float(got[1].abs().max()) == 0.0


def test_tile_batch_refusals(D, L):
    t, idx, aug = torch.zeros(2, 4, 4, 3, dtype=torch.uint8, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.uint8, device="cuda")
    out = gpu_util.Out(2 * 3 * 16, np.float32)
    o = C.c_void_p(out.ptr)
    ok = dict(tiles=L.ptr(t), index=L.ptr(idx), aug=L.ptr(aug), m=2, b=2, t=4, dst=o)
    cases = [dict(tiles=None), dict(index=None), dict(aug=None), dict(dst=None), dict(t=0), dict(t=-4), dict(b=0), dict(m=0),
             dict(b=65536), dict(t=2 ** 31 - 1)]      # the last two: the grid's y / x dimension would overflow
    for change in cases:
        a = dict(ok, **change)
        rc = L.lib().resr_tile_batch(a["tiles"], a["index"], a["aug"], a["m"], a["b"], a["t"], a["dst"], L.stream_ptr())
        assert rc == L.RESR_ERR_ARG and b"tile_batch" in L.lib().resr_last_error(), (change, rc)
    out.read(written=False)                                           # nothing was launched
    assert (out.t.view(torch.int32) == out._sent()).all()
    with pytest.raises(ValueError):
        D.tile_batch(t, idx.long(), aug)
    with pytest.raises(ValueError):
        D.tile_batch(t.float(), idx, aug)


# ---- resr_blur_kernels -----------------------------------------------------------------------------------------------------------
def _records(D):
    """Hand-made records: every family, isotropic and anisotropic, sides 7 and 21, sigma 0.2 and 3, theta +-pi (and inside),
    generalized beta 0.5 and 4, plateau beta 1 and 2, sinc below and above side 13 (the padded final sinc is the same record: a side
    below K), the delta kernel."""
    rec, names = [], []
    for fam, betas in ((D.GAUSSIAN, (1.0,)), (D.GENERALIZED, (0.5, 4.0)), (D.PLATEAU, (1.0, 2.0))):
        for side in (7, 21):
            for beta in betas:
                for sx in (0.2, 3.0):
                    rec.append([fam, side, sx, sx, 0.0, beta, 0, 0.0])
                    names.append(f"{D.FAMILIES[fam]} iso side {side} sigma {sx} beta {beta}")
                    for sy, theta in ((3.0, PI), (0.2, -PI), (1.7, 0.6), (sx, -2.1)):
                        rec.append([fam, side, sx, sy, theta, beta, 1, 0.0])
                        names.append(f"{D.FAMILIES[fam]} aniso side {side} sigma {sx},{sy} theta {theta:.2f} beta {beta}")
    for side, cutoff in ((7, PI / 3), (7, PI), (11, 2.0), (13, PI / 5), (15, PI / 5), (19, 2.9), (21, PI / 3), (21, PI)):
        rec.append([D.SINC, side, 0.0, 0.0, 0.0, 1.0, 0, cutoff])
        names.append(f"sinc side {side} cutoff {cutoff:.3f}")
    rec.append([D.DELTA, 1, 0.0, 0.0, 0.0, 1.0, 0, 0.0])
    names.append("delta")
    return np.asarray(rec, dtype=np.float64), names


def _judge(D, got, want, rec):
    """Per tap: |got - want| <= max(one fp32 ulp of the host tap, 2^-30 x the kernel's largest |tap|); exact where the host tap is
    padding and in the delta kernel.  Returns (taps that differ at all, the worst difference in units of its bound, its place)."""
    K = want.shape[-1]
    differ, worst, where = 0, 0.0, None
    for i in range(want.shape[0]):
        side = int(rec[i][D.R_SIDE])
        pad = (K - side) // 2
        inside = np.zeros((K, K), bool)
        inside[pad:pad + side, pad:pad + side] = True
        g, w = got[i], want[i]
        exact = ~inside if int(rec[i][D.R_FAMILY]) != D.DELTA else np.ones((K, K), bool)
        assert np.array_equal(g[exact].view(np.int32), w[exact].view(np.int32)), ("padding / delta taps are exact", i)
        bound = np.maximum(np.spacing(np.abs(w)).astype(np.float64), 2.0 ** -30 * float(np.abs(w).max()))
        err = np.abs(g.astype(np.float64) - w.astype(np.float64))
        differ += int((g.view(np.int32) != w.view(np.int32)).sum())
        ratio = err / bound
        if ratio.max() > worst:
            worst, where = float(ratio.max()), (i, int(ratio.argmax()))
    return differ, worst, where


def test_blur_kernels_match_the_host_definition(D, L, diag_dir):
    rec, names = _records(D)
    want = D.blur_kernels_from_params_np(rec)
    out = gpu_util.Out(rec.shape[0] * 21 * 21, np.float32)
    r = gpu_util.dev(rec)
    ids = _launch_ids(L, lambda: L.check(L.lib().resr_blur_kernels(L.ptr(r), rec.shape[0], 21, C.c_void_p(out.ptr), L.stream_ptr()), "resr_blur_kernels"))
    assert ids == [33100], ids
    got = out.read().reshape(want.shape)
    assert np.isfinite(got).all()
    differ, worst, where = _judge(D, got, want, rec)
    line = {"kernels": int(rec.shape[0]), "taps": int(want.size), "taps_that_differ": differ, "worst_over_bound": worst,
            "worst_case": names[where[0]] if where else None}
    print("blur_kernels vs host definition:", json.dumps(line))
    with open(os.path.join(diag_dir, "test_gpu_device_data_blur.json"), "w") as f:
        json.dump(line, f)
    assert worst <= 1.0, line
    assert np.allclose(got.reshape(rec.shape[0], -1).sum(1), 1.0, atol=1e-5)
    # two calls, the same bits (the sums run in a fixed order); through the wrapper, and with a smaller K for the 7-tap records
    again = D.blur_kernels(r)
    torch.cuda.synchronize()
    assert np.array_equal(again.cpu().numpy().view(np.int32), got.view(np.int32))
    small = np.flatnonzero(rec[:, D.R_SIDE] <= 7)
    got7 = D.blur_kernels(gpu_util.dev(rec[small]), K=7).cpu().numpy()
    d7, w7, _ = _judge(D, got7, D.blur_kernels_from_params_np(rec[small], K=7), rec[small])
    assert w7 <= 1.0 and np.array_equal(got7.view(np.int32), got[small][:, 7:14, 7:14].view(np.int32))


def test_blur_kernels_refusals(D, L):
    rec, _ = _records(D)
    r = gpu_util.dev(rec[:2])
    out = gpu_util.Out(2 * 31 * 31, np.float32)
    o = C.c_void_p(out.ptr)
    for args in ((None, 2, 21, o), (L.ptr(r), 2, 21, None), (L.ptr(r), 0, 21, o), (L.ptr(r), -1, 21, o), (L.ptr(r), 2, 20, o), (L.ptr(r), 2, 0, o),
                 (L.ptr(r), 2, L.RESR_BLUR_MAX_SIDE + 2, o)):
        rc = L.lib().resr_blur_kernels(*args, L.stream_ptr())
        assert rc == L.RESR_ERR_ARG and b"blur_kernels" in L.lib().resr_last_error(), (args[1:3], rc)
    out.read(written=False)
    assert (out.t.view(torch.int32) == out._sent()).all()
    assert L.RESR_BLUR_MAX_SIDE >= 21
    L.check(L.lib().resr_blur_kernels(L.ptr(r), 2, L.RESR_BLUR_MAX_SIDE, o, L.stream_ptr()))      # the limit itself runs
    out.read()
    with pytest.raises(ValueError, match="blur kernels"):      # a side above K never reaches the device
        D.check_blur_records(rec, K=7)


# ---- the source against the loader ---------------------------------------------------------------------------------------------
def _png_dir(path, count, side, seed):
    from PIL import Image
    os.makedirs(path)
    rng = np.random.default_rng(seed)
    for i in range(count):
        Image.fromarray(rng.integers(0, 256, (side, side, 3), dtype=np.uint8)).save(os.path.join(path, f"{i}.png"))
    return path


def _take(source, count):
    out = []
    for _ in range(count):
        batch = source.next()
        state = _host_state()
        out.append((None if batch is None else {k: v.clone() for k, v in batch.items()}, state))
    torch.cuda.synchronize()
    return out


def test_source_gives_the_loader_paths_batches(D, tmp_path):
    from torch.utils.data import DataLoader, SequentialSampler
    from real_esrgan_pytorch_amd import config
    from real_esrgan_pytorch_amd.dataset import CUDAPrefetcher, TrainValidImageDataset
    path = _png_dir(str(tmp_path / "tiles"), 6, 24, 3)
    dataset = TrainValidImageDataset(path, 16, 4, "Train", config.degradation_model_parameters_dict)
    _seed(11)
    loader = CUDAPrefetcher(DataLoader(dataset, batch_size=2, sampler=SequentialSampler(dataset), num_workers=0, drop_last=True), torch.device("cuda", 0))
    want = _take(loader, 4)
    _seed(11)
    source = D.DeviceTileSource.from_dir(path, 2, torch.device("cuda", 0), sampler=SequentialSampler(range(6)))
    assert len(source) == len(loader) == 3 and source.tiles.shape == (6, 24, 24, 3)
    assert isinstance(source.original_dataloader.sampler, SequentialSampler)
    got = _take(source, 4)
    for k, ((wb, ws), (gb, gs)) in enumerate(zip(want, got)):
        assert ws == gs, f"`random` / `np.random` differ after next() {k}"
        if k == 3:
            assert wb is None and gb is None                      # the fourth next() ends the epoch
            continue
        assert set(gb) == set(wb) == {"hr", "kernel1", "kernel2", "sinc_kernel"}
        assert all(v.is_cuda and v.dtype == torch.float32 for v in gb.values())
        assert gb["hr"].shape == (2, 3, 24, 24) and torch.equal(gb["hr"], wb["hr"]), k
        for name in ("kernel1", "kernel2", "sinc_kernel"):
            g, w = gb[name].cpu().numpy(), wb[name].cpu().numpy()
            assert g.shape == (2, 21, 21)
            bound = np.maximum(np.spacing(np.abs(w)).astype(np.float64), 2.0 ** -30 * np.abs(w).max(axis=(1, 2), keepdims=True))
            assert (np.abs(g.astype(np.float64) - w) <= bound).all(), (k, name)
    assert source.next() is None                                      # and stays ended
    _seed(11)
    source.reset()                                                    # ... until reset() starts over
    first = _take(source, 1)[0]
    assert first[1] == got[0][1] and all(torch.equal(first[0][k], got[0][0][k]) for k in first[0])


def test_a_consumer_on_another_stream_reads_complete_batches(D):
    """No device-wide synchronisation between the producer's launches and the consumer's reads: the event of next() alone orders
    them.  64 tiles of 256 x 256 per batch, so the launches are still running when next() returns."""
    from torch.utils.data import SequentialSampler
    tiles = np.random.default_rng(5).integers(0, 256, (8, 256, 256, 3), dtype=np.uint8)
    order = [i % 8 for i in range(128)]
    _seed(21)
    plans = [[(i, D.sample_augment(), D.sample_blur_params()) for i in order[b * 64:(b + 1) * 64]] for b in range(2)]
    _seed(21)                                                          # the source draws batch 0 now, batch 1 inside the first next()
    source = D.DeviceTileSource.from_array(tiles, 64, torch.device("cuda", 0), sampler=order)
    consumer = torch.cuda.Stream()
    kept = []
    with torch.cuda.stream(consumer):
        for _ in range(2):
            batch = source.next()
            kept.append({k: v.clone() for k, v in batch.items()})      # enqueued on the consumer stream, right behind the event
        assert source.next() is None
    consumer.synchronize()                                             # this stream only
    for plan, batch in zip(plans, kept):
        hr = batch["hr"].cpu()
        for b in (0, 1, 31, 63):
            i, code, rec = plan[b]
            assert torch.equal(hr[b], D.augment_np(tiles[i], code)), b
            want = D.blur_kernels_from_params_np(rec)
            got = np.stack([batch[n][b].cpu().numpy() for n in ("kernel1", "kernel2", "sinc_kernel")])
            assert _judge(D, got, want, rec)[1] <= 1.0
    with pytest.raises(IndexError):
        D.DeviceTileSource.from_array(tiles, 2, torch.device("cuda", 0), sampler=[0, 8])      # an index past the tiles never reaches the kernel


# ---- the train script ------------------------------------------------------------------------------------------------------------
def _smooth_png(path, size, seed):
    from PIL import Image
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    x = F.interpolate(torch.rand(1, 3, size // 8, size // 8, generator=g), size=(size, size), mode="bicubic").clamp(0, 1)
    x = (0.85 * x + 0.15 * torch.rand(1, 3, size, size, generator=g)).clamp(0, 1)
    Image.fromarray((x[0].permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(path)


def _tiny_dataset(tmp_path, monkeypatch):
    """224-pixel PNGs (4 train, 2 valid, 2 test pairs), image_size 208, batch 2, one epoch, the compact generator, the device source."""
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
                    lr_scheduler_step_size=1, exp_name="device_source_test", model_lr=2e-4, model_betas=(0.9, 0.99),
                    ema_model_weight_decay=0.999, niqe_model_path=os.path.join(here, "golden", "niqe_model.mat"),
                    device=torch.device("cuda", 0), g_arch="compact", compact_num_conv=2, compact_act_type="prelu",
                    precision="fast", output_parity=False, inference_precision="exact16", upscale_factor=4, data_source="device")
    for k, v in settings.items():
        monkeypatch.setattr(config, k, v, raising=False)
    monkeypatch.chdir(tmp_path)


def test_train_realesrnet_epoch_from_the_device_source(D, tmp_path, monkeypatch):
    from real_esrgan_pytorch_amd import config
    from real_esrgan_pytorch_amd import train_realesrnet as T
    _tiny_dataset(tmp_path, monkeypatch)
    made = []
    load = T.load_dataset

    def load_and_keep():
        made.extend(load())
        return made
    monkeypatch.setattr(T, "load_dataset", load_and_keep)
    T.main()
    assert isinstance(made[0], D.DeviceTileSource) and made[0].tiles.shape == (4, 224, 224, 3) and len(made[0]) == 2
    assert not isinstance(made[1], D.DeviceTileSource) and not isinstance(made[2], D.DeviceTileSource)
    ck = torch.load(tmp_path / "samples" / "device_source_test" / "g_epoch_1.pth.tar", weights_only=False)
    assert ck["epoch"] == 1 and ck["optimizer"]["state"][0]["step"] == 2 and np.isfinite(ck["best_niqe"])
    assert (tmp_path / "results" / "device_source_test" / "g_last.pth.tar").exists()
    scalars = [json.loads(l) for l in open(tmp_path / "samples" / "logs" / "device_source_test" / "scalars.jsonl")]
    losses = [s["value"] for s in scalars if s["tag"] == "Train/Loss"]
    assert len(losses) == 2 and all(np.isfinite(v) and v > 0 for v in losses), losses
    # an unknown source is refused where the sources are built
    monkeypatch.setattr(config, "data_source", "hbm")
    monkeypatch.setattr(T, "load_dataset", load)
    with pytest.raises(ValueError, match="data_source"):
        T.load_dataset()
