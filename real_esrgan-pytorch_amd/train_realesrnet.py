"""RealESRNet training entry point behind the reference's `train_realesrnet.py` surface: same
function names, epoch loop, checkpoint dictionary and file names, NIQE validation with the EMA weights applied.

    python -m real_esrgan_pytorch_amd.train_realesrnet          # reads real_esrgan_pytorch_amd.config

The step itself is `train.RealESRNetStep` (degradation -> generator forward/backward on the HIP kernels -> Adam ->
EMA); the degradation uses the blur kernels the dataset sampled for each image (reference train_realesrnet.py:258-413).
TensorBoard is absent from the image: scalars go to `samples/logs/<exp>/scalars.jsonl` through the same `add_scalar`.
"""
from __future__ import annotations

import inspect
import json
import os
import shutil
import time
from typing import Any, List, Optional

import numpy as np
import torch
from torch import nn, optim
from torch.optim import lr_scheduler
from torch.utils.data import DataLoader

from . import config, imgproc
from . import _lib
from .dataset import CUDAPrefetcher, TestImageDataset, TrainValidImageDataset
from .degrade import DegradationPrefetcher
from .meters import AverageMeter, ProgressMeter, Summary  # noqa: F401  (the reference's script-level names)
from .compact import SRVGGNetCompact
from .model import EMA, Generator, load_official_state_dict  # noqa: F401  (Generator: the reference's script-level name)
from .train import DataParallel, RealESRNetStep, setup_distributed


class ScalarWriter:
    """`SummaryWriter.add_scalar` stand-in: one JSON line per scalar (rank 0 only under data parallelism)."""

    def __init__(self, log_dir: str, enabled: bool = True) -> None:
        self.enabled = enabled
        if enabled:
            os.makedirs(log_dir, exist_ok=True)
        self.path = os.path.join(log_dir, "scalars.jsonl")

    def add_scalar(self, tag: str, value: float, step: int) -> None:
        if not self.enabled:
            return
        with open(self.path, "a") as f:
            f.write(json.dumps({"tag": tag, "value": float(value), "step": int(step)}) + "\n")


_RANK, _WORLD = 0, 1     # set by main() through train.setup_distributed()


def seed_rank(rank: int, world: int, base: int = 0) -> None:
    """Data-parallel ranks must not draw the same degradation plans, sigma / quality values and crop offsets: the host and
    device generators of rank r restart at base + r (rank 0 keeps the reference's seeds, config.py:64-66)."""
    if world > 1:
        import random
        random.seed(base + rank)
        np.random.seed(base + rank)
        torch.manual_seed(base + rank)


def load_dataset() -> List[CUDAPrefetcher]:
    """Reference train_realesrnet.py:131-172."""
    valid_datasets = TrainValidImageDataset(config.valid_image_dir, config.image_size, config.upscale_factor, "Valid",
                                            config.degradation_model_parameters_dict)
    test_datasets = TestImageDataset(config.test_lr_image_dir, config.test_hr_image_dir)
    workers = config.num_workers
    valid_dataloader = DataLoader(valid_datasets, batch_size=1, shuffle=False, num_workers=min(1, workers),
                                  pin_memory=True, drop_last=False, persistent_workers=workers > 0)
    test_dataloader = DataLoader(test_datasets, batch_size=1, shuffle=False, num_workers=min(1, workers),
                                 pin_memory=True, drop_last=False, persistent_workers=workers > 0)
    if config.data_source in config.PAIRED_DATA_SOURCES:
        train_source = _paired_source()
    elif config.data_source in ("loader", "device") + config.IMAGE_DATA_SOURCES:
        train_source = _synthesised_source()
    else:
        raise ValueError(f"config.data_source={config.data_source!r}: expected one of {config.DATA_SOURCES}")
    return [train_source, CUDAPrefetcher(valid_dataloader, config.device), CUDAPrefetcher(test_dataloader, config.device)]


def _synthesised_source():
    """The train source of "loader" / "device" / "images" / "images_loader": HR tiles and their blur kernels, for
    `DegradationPrefetcher` to make the pairs from."""
    if config.data_source in config.IMAGE_DATA_SOURCES:
        return _image_source()
    train_datasets = TrainValidImageDataset(config.train_image_dir, config.image_size, config.upscale_factor, "Train",
                                            config.degradation_model_parameters_dict)
    workers = config.num_workers
    # data parallel: every rank draws its own shard of each epoch (batch_size is per GPU, as in the reference's per-process config)
    sampler = torch.utils.data.distributed.DistributedSampler(train_datasets, _WORLD, _RANK, shuffle=True) if _WORLD > 1 else None
    train_dataloader = DataLoader(train_datasets, batch_size=config.batch_size, shuffle=sampler is None, sampler=sampler,
                                  num_workers=workers, pin_memory=True, drop_last=True, persistent_workers=workers > 0)
    if config.data_source == "device":
        # the training tiles resident in HBM, augmentation and kernel synthesis on the device (device_data.py): the same batch
        # dictionary, draws and sampler classes; the DataLoader above is never iterated (no workers start)
        from .device_data import DeviceTileSource
        count = len(train_datasets)
        sampler = torch.utils.data.distributed.DistributedSampler(range(count), _WORLD, _RANK, shuffle=True) if _WORLD > 1 else None
        return DeviceTileSource.from_dir(config.train_image_dir, config.batch_size, config.device, sampler=sampler,
                                         P=config.degradation_model_parameters_dict)
    return CUDAPrefetcher(train_dataloader, config.device)


def _image_source():
    """The train source of "images" / "images_loader": whole images of any size in config.train_image_dir, a sample a random
    config.train_tile window of its image -- the batch dictionary of the tile sources, so the degradation stage takes it unchanged."""
    from .dataset import CropImageDataset
    from .device_data import ImageCropSource
    tile = config.train_window()      # (checked against image_size again: both may have been set after import)
    scales, short_side = config.train_copies()      # the multi-scale copies: every image enters the set 1 + K times
    if config.data_source == "images":
        count = len(os.listdir(config.train_image_dir)) * (1 + len(scales) + (short_side > 0))
        sampler = torch.utils.data.distributed.DistributedSampler(range(count), _WORLD, _RANK, shuffle=True) if _WORLD > 1 else None
        return ImageCropSource.from_dir(config.train_image_dir, config.batch_size, tile, config.device, sampler=sampler,
                                        P=config.degradation_model_parameters_dict, scales=scales, short_side=short_side)
    train_datasets = CropImageDataset(config.train_image_dir, tile, config.degradation_model_parameters_dict, scales, short_side)
    workers = config.num_workers
    sampler = torch.utils.data.distributed.DistributedSampler(train_datasets, _WORLD, _RANK, shuffle=True) if _WORLD > 1 else None
    train_dataloader = DataLoader(train_datasets, batch_size=config.batch_size, shuffle=sampler is None, sampler=sampler,
                                  num_workers=workers, pin_memory=True, drop_last=True, persistent_workers=workers > 0)
    return CUDAPrefetcher(train_dataloader, config.device)


def _paired_source():
    """The train source of "paired" / "paired_loader": LR / HR pairs of the user's own (HR in config.train_image_dir, LR in
    config.paired_lr_image_dir), handed out as (lr, hr, batch) -- what train() iterates, with no degradation stage in between."""
    from .dataset import PairedImageDataset, PairedPrefetcher
    from .device_data import PairedDeviceSource, paired_files
    if not getattr(config, "paired_lr_image_dir", ""):
        raise ValueError(f"config.data_source={config.data_source!r} needs config.paired_lr_image_dir (RESR_PAIRED_LR_DIR)")
    patch, scale = config.paired_patch(), config.upscale_factor
    if config.data_source == "paired":
        count = len(paired_files(config.train_image_dir, config.paired_lr_image_dir)[0])
        sampler = torch.utils.data.distributed.DistributedSampler(range(count), _WORLD, _RANK, shuffle=True) if _WORLD > 1 else None
        return PairedDeviceSource.from_dirs(config.train_image_dir, config.paired_lr_image_dir, config.batch_size, patch, scale, config.device,
                                            sampler=sampler)
    train_datasets = PairedImageDataset(config.train_image_dir, config.paired_lr_image_dir, patch, scale)
    workers = config.num_workers
    sampler = torch.utils.data.distributed.DistributedSampler(train_datasets, _WORLD, _RANK, shuffle=True) if _WORLD > 1 else None
    train_dataloader = DataLoader(train_datasets, batch_size=config.batch_size, shuffle=sampler is None, sampler=sampler,
                                  num_workers=workers, pin_memory=True, drop_last=True, persistent_workers=workers > 0)
    return PairedPrefetcher(train_dataloader, config.device)


def train_pairs(train_prefetcher):
    """What train() of both scripts iterates: (lr, hr, batch) items.  A paired source hands them out itself; every other source gets the
    second-order degradation attached (reference train_realesrnet.py:262-377: host draws in the reference's order, blur kernels from
    the dataset batch), which runs ONE BATCH AHEAD on a side stream: batch i+1's kernels are enqueued before step i is issued and run
    under it.  No degradation kernel is launched and no degradation draw is made for a paired source.  With config.pair_pool_size > 0
    either one stands behind the process's training pair pool (`_pooled`); with 0, the default, nothing changes."""
    if config.data_source in config.PAIRED_DATA_SOURCES:
        return _pooled(train_prefetcher)
    jpeg_operation = imgproc.DiffJPEG(False)
    usm_sharpener = imgproc.USMSharp(50, 0).to(device=config.device)
    return _pooled(DegradationPrefetcher(train_prefetcher, usm_sharpener, jpeg_operation, config.upscale_factor, config.image_size, config.device))


_PAIR_POOL = None     # the process's training pair pool: train() asks for its pairs once per epoch, and the pool must outlive the epoch


def _pooled(source):
    """`source` itself with the pool off; else the process's `device_data.PairPool` re-attached to this epoch's source, made at the
    first call.  Its draws come from a generator of its own, seeded with the rank (seed_rank's spirit: no two ranks draw the same
    slots), so the source's and the degradation stage's draws are the ones they make with the pool off.  main() of either script
    clears it when it starts: two runs in one process are independent."""
    global _PAIR_POOL
    size = config.pair_pool()      # (checked against the batch size again: both may have been set after import)
    if size <= 0:
        return source
    from .device_data import PairPool
    if _PAIR_POOL is None:
        _PAIR_POOL = PairPool(source, size, seed=_RANK)
    else:
        _PAIR_POOL.attach(source)
    return _PAIR_POOL


def build_model() -> List[nn.Module]:
    """Reference train_realesrnet.py:175-183."""
    model = config.build_generator(True).to(device=config.device)      # config.g_arch: Generator or SRVGGNetCompact (output parity: config.py)
    ema_model = EMA(model, config.ema_model_weight_decay).to(device=config.device)
    ema_model.register()
    return [model, ema_model]


def load_pretrained(path: str, model: nn.Module, ema_model: EMA) -> None:
    """`config.pretrained_g`: an upstream checkpoint into the generator (model.load_official_state_dict), and the EMA shadow
    registered again from the loaded weights -- a fine-tune must not average from the random init of build_model()."""
    load_official_state_dict(model, torch.load(path, map_location=lambda storage, loc: storage, weights_only=False))
    ema_model.register()
    print(f"Loaded pretrained generator weights `{os.path.abspath(path)}`.")


def define_loss() -> nn.L1Loss:
    return nn.L1Loss().to(device=config.device)


def define_optimizer(model) -> optim.Adam:
    return optim.Adam(model.parameters(), config.model_lr, config.model_betas)


def define_scheduler(optimizer) -> lr_scheduler.StepLR:
    return lr_scheduler.StepLR(optimizer, config.lr_scheduler_step_size, config.lr_scheduler_gamma)


def load_checkpoint(path: str, model: nn.Module, ema_model: nn.Module, optimizer, scheduler) -> List[Any]:
    """Reference train_realesrnet.py:60-83: keys present in the current modules are taken, the rest ignored."""
    checkpoint = torch.load(path, map_location=lambda storage, loc: storage, weights_only=False)
    for module, key in ((model, "state_dict"), (ema_model, "ema_state_dict")):
        current = module.state_dict()
        current.update({k: v for k, v in checkpoint[key].items() if k in current})
        module.load_state_dict(current)
    optimizer.load_state_dict(checkpoint["optimizer"])
    scheduler.load_state_dict(checkpoint["scheduler"])
    return [checkpoint["epoch"], checkpoint["best_niqe"]]


def save_checkpoint(epoch: int, best_niqe: float, is_best: bool, model, ema_model, optimizer, scheduler,
                    samples_dir: str, results_dir: str) -> str:
    """Reference train_realesrnet.py:117-129: same dictionary, same file names."""
    path = os.path.join(samples_dir, f"g_epoch_{epoch + 1}.pth.tar")
    torch.save({"epoch": epoch + 1, "best_niqe": best_niqe, "state_dict": model.state_dict(),
                "ema_state_dict": ema_model.state_dict(), "optimizer": optimizer.state_dict(),
                "scheduler": scheduler.state_dict()}, path)
    if is_best:
        shutil.copyfile(path, os.path.join(results_dir, "g_best.pth.tar"))
    if (epoch + 1) == config.epochs:
        shutil.copyfile(path, os.path.join(results_dir, "g_last.pth.tar"))
    return path


def main() -> None:
    global _RANK, _WORLD, _PAIR_POOL
    _PAIR_POOL = None                                    # a run starts with no training pair pool: it is made at the first epoch
    _RANK, _WORLD, device = setup_distributed()          # one process per GPU: cuda:LOCAL_RANK, RCCL group when WORLD_SIZE > 1
    config.device = device
    seed_rank(_RANK, _WORLD)
    start_epoch, best_niqe = 0, 100.0
    train_prefetcher, valid_prefetcher, test_prefetcher = load_dataset()
    model, ema_model = build_model()
    if config.pretrained_g:                              # before the broadcast below and before `resume`
        load_pretrained(config.pretrained_g, model, ema_model)
    dp = DataParallel()
    dp.attach(model)                                     # broadcast of the initial weights + all-reduce of the gradient arena per step
    dp.attach_ema(ema_model)                             # ... and of the EMA shadow (registered from each rank's own init above)
    pixel_criterion = define_loss()
    optimizer = define_optimizer(model)
    scheduler = define_scheduler(optimizer)
    if config.resume:
        start_epoch, best_niqe = load_checkpoint(config.resume, model, ema_model, optimizer, scheduler)
        print("Loaded pretrained model weights.")
        dp.broadcast_(model.flat_parameters())           # every rank read the same file; keep the replicas bit-identical anyway
        dp.attach_ema(ema_model)
    samples_dir = os.path.join("samples", config.exp_name)
    results_dir = os.path.join("results", config.exp_name)
    os.makedirs(samples_dir, exist_ok=True)
    os.makedirs(results_dir, exist_ok=True)
    writer = ScalarWriter(os.path.join("samples", "logs", config.exp_name), enabled=_RANK == 0)
    scaler = torch.amp.GradScaler("cuda") if config.train_precision() != "strict" else None
    niqe_model = config.build_niqe()
    full_ref = config.build_full_ref()
    for epoch in range(start_epoch, config.epochs):
        sampler = getattr(train_prefetcher.original_dataloader, "sampler", None)
        if hasattr(sampler, "set_epoch"):
            sampler.set_epoch(epoch)
        train(model, ema_model, train_prefetcher, pixel_criterion, optimizer, epoch, scaler, writer)
        _lib.chain_health(sync=True)   # fail loudly if a chained conv launch ever gave up on a neighbouring tile
        _ = validate(model, ema_model, valid_prefetcher, epoch, writer, niqe_model, "Valid", full_ref=full_ref)
        niqe = validate(model, ema_model, test_prefetcher, epoch, writer, niqe_model, "Test", full_ref=full_ref)
        print("\n")
        scheduler.step()
        is_best = niqe < best_niqe
        best_niqe = min(niqe, best_niqe)
        if _RANK == 0:       # weights, EMA shadow and optimiser state are identical on every rank: one writer
            save_checkpoint(epoch, best_niqe, is_best, model, ema_model, optimizer, scheduler, samples_dir, results_dir)


def train(model: nn.Module, ema_model: nn.Module, train_prefetcher: CUDAPrefetcher, pixel_criterion: nn.L1Loss,
          optimizer: optim.Adam, epoch: int, scaler: Optional["torch.amp.GradScaler"], writer: ScalarWriter) -> None:
    """Reference train_realesrnet.py:218-413."""
    batches = len(train_prefetcher)
    batch_time = AverageMeter("Time", ":6.3f", Summary.NONE)            # :219-224
    data_time = AverageMeter("Data", ":6.3f", Summary.NONE)
    losses = AverageMeter("Loss", ":6.6f", Summary.NONE)
    progress = ProgressMeter(batches, [batch_time, data_time, losses], prefix=f"Epoch: [{epoch + 1}]")
    model.train()

    degraded = train_pairs(train_prefetcher)     # the degradation stage over the source, or the paired source itself
    step = RealESRNetStep(model, ema_model, optimizer, scaler, None)
    step.criterion = pixel_criterion
    batch_index = 0
    degraded.reset()
    item = degraded.next()
    end = time.time()
    while item is not None:
        data_time.update(time.time() - end)
        lr, hr, _ = item
        loss = step(hr, lr)
        losses.update(loss, hr.size(0))                    # :397 -- every batch counts; accumulated on the device, no read-back
        batch_time.update(time.time() - end)
        if batch_index % config.print_frequency == 0:      # the only host read-back of the loop
            writer.add_scalar("Train/Loss", losses.val, batch_index + epoch * batches + 1)
            _lib.chain_health()                            # two host-mapped counters, no synchronisation: a broken chained launch aborts here
            if _RANK == 0:
                progress.display(batch_index)
        end = time.time()
        item = degraded.next()
        batch_index += 1


def validate(model: nn.Module, ema_model: nn.Module, data_prefetcher: CUDAPrefetcher, epoch: int, writer: ScalarWriter,
             niqe_model: Any, mode: str, full_ref: Any = None) -> float:
    """Reference train_realesrnet.py:416-488: EMA weights applied for the evaluation, restored afterwards.  full_ref
    (`config.build_full_ref()`; None = off): a module forward(sr, hr) -> (psnr, ssim) that also scores sr against the batch's ground
    truth; `{mode}/PSNR` and `{mode}/SSIM` then go to the writer and the summary line (of the Y channel, or with
    `config.full_ref_channels` = "rgb" of the RGB channels, under the same names).  The NIQE average alone is returned."""
    if mode not in ("Valid", "Test"):
        raise ValueError("Unsupported mode, please use `Valid` or `Test`.")
    batch_time = AverageMeter("Time", ":6.3f", Summary.NONE)
    niqe_metrics = AverageMeter("NIQE", ":4.2f", Summary.AVERAGE)
    psnr_metrics = AverageMeter("PSNR", ":4.2f", Summary.AVERAGE)
    ssim_metrics = AverageMeter("SSIM", ":4.4f", Summary.AVERAGE)
    ema_model.apply_shadow()
    model.eval()
    batch_index = 0
    data_prefetcher.reset()
    batch_data = data_prefetcher.next()
    end = time.time()
    with torch.no_grad():
        while batch_data is not None:
            lr = batch_data["lr"].to(device=config.device, non_blocking=True)
            sr = model(lr)
            if isinstance(model, SRVGGNetCompact):
                sr.clamp_(0, 1)     # the compact module does not clamp (Generator does, inside); upstream's inference does, and NIQE quantises to 0..255
            niqe = niqe_model(sr)
            niqe_metrics.update(niqe.reshape(()), lr.size(0))
            if full_ref is not None:
                psnr, ssim = full_ref(sr, batch_data["hr"].to(device=config.device, non_blocking=True))
                psnr_metrics.update(psnr.mean(), lr.size(0))
                ssim_metrics.update(ssim.mean(), lr.size(0))
            batch_time.update(time.time() - end)
            end = time.time()
            batch_data = data_prefetcher.next()
            batch_index += 1
    ema_model.restore()
    avg_niqe = niqe_metrics.avg     # the meters accumulate on the device: THIS read-back is the evaluation's first synchronisation
    _lib.chain_health()             # ... after which every launch of the evaluation has reported
    meters = [batch_time, niqe_metrics] + ([psnr_metrics, ssim_metrics] if full_ref is not None else [])
    if _RANK == 0:
        ProgressMeter(len(data_prefetcher), meters, prefix=f"{mode}: ").display_summary()
    writer.add_scalar(f"{mode}/NIQE", avg_niqe, epoch + 1)
    if full_ref is not None:
        writer.add_scalar(f"{mode}/PSNR", psnr_metrics.avg, epoch + 1)
        writer.add_scalar(f"{mode}/SSIM", ssim_metrics.avg, epoch + 1)
    return avg_niqe


# The reference's validate() has exactly the seven positional parameters above, and the entry points keep the reference's
# signatures for whatever introspects them (tests/test_surface.py pins that list); `full_ref` is this project's keyword on top of it,
# so the advertised signature stays the reference's.
validate.__signature__ = inspect.Signature([p for p in inspect.signature(validate).parameters.values() if p.name != "full_ref"],
                                           return_annotation=float)


if __name__ == "__main__":
    main()
