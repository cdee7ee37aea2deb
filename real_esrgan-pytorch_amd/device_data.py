"""A device-resident training data source: the tiles of the training set live in HBM as uint8, and a batch -- gather, rotate / flip
augmentation, /255, HWC -> CHW, and the 3 x B blur / sinc kernels of the degradation stage -- is two launches on a side stream
(csrc/data_source.hip: resr_tile_batch, resr_blur_kernels).  The host keeps only the random draws, made in the loader path's order
(dataset.py `TrainValidImageDataset.__getitem__` at num_workers=0: the augmentation, then the kernel parameters), so a fixed seed gives
the loader path's batches.  `DeviceTileSource` has `dataset.CUDAPrefetcher`'s contract and sits in its place under
`degrade.DegradationPrefetcher` (config.data_source = "device").

Host definitions (numpy, float64 where the loader path's are): `sample_blur_params` / `blur_kernels_from_params_np` split
`degrade.sample_blur_kernels` into its draws and its arithmetic, `sample_augment` / `augment_np` do the same for the
`imgproc.random_rotate` / `random_horizontally_flip` / `random_vertically_flip` chain.  The kernels are judged against them.

The paired source (config.data_source = "paired") feeds LR / HR pairs of the user's own instead of synthesised ones: both sides of
every pair resident as uint8 in two arenas, a batch -- crop, dihedral augmentation, /255, HWC -> CHW of both sides -- ONE launch
(resr_pair_batch).  `paired_sample_np` is the definition, `sample_paired_draw` the host's draws, `PairedDeviceSource` the source; it
has `degrade.DegradationPrefetcher`'s contract, because it stands in its place in the train scripts.  The loader path over the same
two directories is `dataset.PairedImageDataset` / `PairedPrefetcher`.

The whole-image source (config.data_source = "images") lifts the tile source's one limit, that every file is a square tile of one size:
images of any size resident in one arena, a batch -- random T x T window, reflect padding of an image below T, the tile source's
rotation and flips, /255, HWC -> CHW -- ONE launch (resr_crop_batch) in front of resr_blur_kernels.  `reflect101` / `crop_sample_np` are
the definition, `sample_crop_draw` the host's extra draw, `ImageCropSource` the source, with `DeviceTileSource`'s contract; the loader
path over the same directory is `dataset.CropImageDataset`.  With `scales` / `short_side` the set also holds upstream's multi-scale copies of
every image, made on the device at construction (resr_resample_u8, one launch per group of copies): Pillow's 8-bit LANCZOS resize as an
integer rule -- `resample_tables_np` / `resample_u8_np` are the definition, `multiscale_sizes` the sizes -- which the loader twin makes with
Pillow itself, to the same bits.

The training pair pool (config.pair_pool_size > 0) stands behind whichever source hands out (lr, hr, batch): a resident queue of
finished pairs that a step's batch is exchanged with, so that a batch mixes samples of many degradation plans.  `pool_exchange_np` /
`pool_store_np` are the definition, `sample_pool_slots` the host's draw (from a `random.Random` of the pool's own), `PairPool` the
wrapper; an exchange is ONE launch (resr_pool_exchange) on the consumer's stream.
"""
from __future__ import annotations

import math
import os
import random
import types
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, imgproc
from .config import check_train_copies, degradation_model_parameters_dict as MODEL_P

__all__ = ["sample_blur_params", "blur_kernels_from_params_np", "check_blur_records", "sample_augment", "augment_np",
           "tile_batch", "blur_kernels", "DeviceTileSource", "RECORD", "FAMILIES",
           "paired_sample_np", "sample_paired_draw", "check_paired_records", "paired_files", "pair_batch", "PairedDeviceSource",
           "reflect101", "crop_sample_np", "sample_crop_draw", "check_crop_records", "crop_batch", "ImageCropSource",
           "resample_ksize", "resample_tables_np", "resample_tables", "resample_u8_np", "multiscale_sizes", "resample_jobs", "resample_u8",
           "pool_exchange_np", "pool_store_np", "sample_pool_slots", "check_pool_slots", "pool_exchange", "pool_store", "PairPool",
           "HostPairPool"]

# One blur-kernel record: RECORD float64 words, the layout include/resr.h documents (resr_blur_kernels).
RECORD = 8
R_FAMILY, R_SIDE, R_SIGMA_X, R_SIGMA_Y, R_THETA, R_BETA, R_ANISO, R_CUTOFF = range(RECORD)
FAMILIES = ("gaussian", "generalized", "plateau", "sinc", "delta")
GAUSSIAN, GENERALIZED, PLATEAU, SINC, DELTA = range(5)
KERNEL_SIDE = 21             # K of the degradation stage (config: sinc_kernel_size, the last gaussian_kernel_range entry)
DEFAULT_MAX_BYTES = 64 << 30


def _record(family, side, sigma_x=0.0, sigma_y=0.0, theta=0.0, beta=1.0, aniso=0.0, cutoff=0.0):
    return [float(family), float(side), sigma_x, sigma_y, theta, beta, float(aniso), cutoff]


def _mixed_params(kernel_type, kernel_prob, size, sigma_range, rotation_range, gen_beta_range, plateau_beta_range):
    """The draws of imgproc.random_mixed_kernels (noise_range=None), in its order."""
    kind = random.choices(kernel_type, kernel_prob)[0]
    family = GENERALIZED if kind.startswith("generalized") else (PLATEAU if kind.startswith("plateau") else GAUSSIAN)
    isotropic = not kind.endswith("anisotropic")
    sigma_x = np.random.uniform(sigma_range[0], sigma_range[1])
    if isotropic:
        sigma_y, theta = sigma_x, 0.0
    else:
        sigma_y = np.random.uniform(sigma_range[0], sigma_range[1])
        theta = np.random.uniform(rotation_range[0], rotation_range[1])
    beta = 1.0
    if family != GAUSSIAN:
        rng = gen_beta_range if family == GENERALIZED else plateau_beta_range
        beta = np.random.uniform(rng[0], 1) if np.random.uniform() < 0.5 else np.random.uniform(1, rng[1])
    return _record(family, size, sigma_x, sigma_y, theta, beta, not isotropic)


def sample_blur_params(P: dict = MODEL_P) -> np.ndarray:
    """The host draws of `degrade.sample_blur_kernels` (ONE sample: kernel1, kernel2, the final sinc kernel), in its order from
    `random` and `np.random`, as three records [3, RECORD] float64 instead of three kernels.  Both generators are left in the
    state `sample_blur_kernels` leaves them in."""
    out = []
    kr = P["gaussian_kernel_range"]
    for tag in ("1", "2"):
        size = random.choice(kr)
        if np.random.uniform() < P["sinc_kernel_probability" + tag]:
            lo = np.pi / 3 if size < int(np.median(kr)) else np.pi / 5
            out.append(_record(SINC, size, cutoff=np.random.uniform(lo, np.pi)))
        else:
            out.append(_mixed_params(P["gaussian_kernel_type"], P["gaussian_kernel_probability" + tag], size,
                                     P["gaussian_sigma_range" + tag], [-math.pi, math.pi], P["generalized_kernel_beta_range" + tag],
                                     P["plateau_kernel_beta_range" + tag]))
    if np.random.uniform() < P["sinc_kernel_probability3"]:
        size = random.choice(kr)
        out.append(_record(SINC, size, cutoff=np.random.uniform(np.pi / 3, np.pi)))
    else:
        out.append(_record(DELTA, 1))
    return np.asarray(out, dtype=np.float64)


def check_blur_records(records: np.ndarray, K: int = KERNEL_SIDE) -> np.ndarray:
    """`records` as a float64 [n, RECORD] array, or ValueError for what the record's definition excludes: a family outside 0..4, a
    side that is not an odd integer in [1, K] (a delta kernel's side is 1), a non-positive sigma of a Gaussian family."""
    rec = np.ascontiguousarray(np.asarray(records, dtype=np.float64).reshape(-1, RECORD))
    if K < 1 or K % 2 == 0:
        raise ValueError(f"blur kernels: K={K} must be odd")
    fam, side = rec[:, R_FAMILY], rec[:, R_SIDE]
    if rec.shape[0] < 1 or not np.isfinite(rec).all():
        raise ValueError("blur kernels: no record, or a record that is not finite")
    if not (np.isin(fam, np.arange(len(FAMILIES)))).all():
        raise ValueError(f"blur kernels: family outside 0..{len(FAMILIES) - 1}: {sorted(set(fam.tolist()))}")
    if not ((side == np.floor(side)) & (side >= 1) & (side <= K) & (side % 2 == 1)).all():
        raise ValueError(f"blur kernels: a side must be an odd integer in [1, {K}]: {sorted(set(side.tolist()))}")
    if not (side[fam == DELTA] == 1).all():
        raise ValueError("blur kernels: the delta kernel's side is 1")
    gauss = fam <= PLATEAU
    if not ((rec[gauss, R_SIGMA_X] > 0) & (rec[gauss, R_SIGMA_Y] > 0)).all():
        raise ValueError("blur kernels: sigma_x and sigma_y of a Gaussian family must be positive")
    return rec


def blur_kernels_from_params_np(records: np.ndarray, K: int = KERNEL_SIDE) -> np.ndarray:
    """THE definition of a record's kernel: float32 [n, K, K], bit for bit what `degrade.sample_blur_kernels` returns for the same
    draws (the same imgproc._kernel_of / generate_sinc_kernel / np.pad calls, the second normalisation of random_mixed_kernels)."""
    rec = check_blur_records(records, K)
    out = np.zeros((rec.shape[0], K, K), dtype=np.float32)
    for i, r in enumerate(rec):
        family, side = int(r[R_FAMILY]), int(r[R_SIDE])
        if family == DELTA:
            k = np.ones((1, 1))
        elif family == SINC:
            k = imgproc.generate_sinc_kernel(r[R_CUTOFF], side, padding=False)
        else:
            k = imgproc._kernel_of(FAMILIES[family], side, r[R_SIGMA_X], r[R_SIGMA_Y], r[R_THETA], r[R_BETA], not r[R_ANISO])
            k = k / np.sum(k)
        pad = (K - side) // 2
        out[i] = np.pad(k, ((pad, pad), (pad, pad))).astype(np.float32)
    return out


def sample_augment() -> int:
    """The draws of random_rotate(..., [0, 90, 180, 270]), random_horizontally_flip(..., 0.5) and random_vertically_flip(..., 0.5),
    in that order, as one code: bits 0-1 = angle / 90, bit 2 = horizontal flip, bit 3 = vertical flip."""
    code = random.choice([0, 90, 180, 270]) // 90
    code |= (random.random() < 0.5) << 2
    code |= (random.random() < 0.5) << 3
    return int(code)


def augment_np(tile_u8: np.ndarray, code: int) -> torch.Tensor:
    """uint8 [T, T, 3] -> float32 [3, T, T]: image_to_tensor(vflip(hflip(_rotate_right_angle(u8 / 255.0f)))) for that code, the zero
    row / column an even side gains under 90 / 180 / 270 included."""
    tile_u8 = np.asarray(tile_u8)
    if tile_u8.dtype != np.uint8 or tile_u8.ndim != 3 or tile_u8.shape[0] != tile_u8.shape[1] or tile_u8.shape[2] != 3:
        raise ValueError(f"augment_np: expected a uint8 [T, T, 3] tile, got {tile_u8.dtype} {tile_u8.shape}")
    if not 0 <= int(code) < 16:
        raise ValueError(f"augment_np: code {code} outside 0..15")
    image = imgproc._rotate_right_angle(tile_u8.astype(np.float32) / 255.0, 90 * (code & 3))
    if code & 4:
        image = image[:, ::-1].copy()
    if code & 8:
        image = image[::-1].copy()
    return imgproc.image_to_tensor(image, False, False)


# ---- the two launches ------------------------------------------------------------------------------------------------------------
def tile_batch(tiles: torch.Tensor, index: torch.Tensor, aug: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """resr_tile_batch on the current stream: tiles uint8 [M,T,T,3], index int32 [B], aug uint8 [B], all on the device (the indices
    were checked by the caller) -> float32 [B,3,T,T]."""
    _lib.require_cuda(tiles, "tile_batch")
    M, T = int(tiles.shape[0]), int(tiles.shape[1])
    B = int(index.numel())
    if tiles.dtype != torch.uint8 or tiles.dim() != 4 or tiles.shape[2] != T or tiles.shape[3] != 3 or not tiles.is_contiguous():
        raise ValueError(f"tile_batch: tiles must be a contiguous uint8 [M,T,T,3] tensor, got {tiles.dtype} {tuple(tiles.shape)}")
    if index.dtype != torch.int32 or aug.dtype != torch.uint8 or aug.numel() != B or index.device != tiles.device or aug.device != tiles.device:
        raise ValueError("tile_batch: index int32 [B] and aug uint8 [B] on the tiles' device")
    if out is None:
        out = torch.empty(B, 3, T, T, dtype=torch.float32, device=tiles.device)
    _lib.check(_lib.lib().resr_tile_batch(_lib.ptr(tiles), _lib.ptr(index), _lib.ptr(aug), M, B, T, _lib.ptr(out), _lib.stream_ptr(tiles)),
               "resr_tile_batch")
    return out


def blur_kernels(records_dev: torch.Tensor, K: int = KERNEL_SIDE, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """resr_blur_kernels on the current stream: float64 [n, RECORD] records on the device (checked by check_blur_records before
    they were uploaded) -> float32 [n, K, K]."""
    _lib.require_cuda(records_dev, "blur_kernels")
    if records_dev.dtype != torch.float64 or records_dev.dim() != 2 or records_dev.shape[1] != RECORD or not records_dev.is_contiguous():
        raise ValueError(f"blur_kernels: records must be a contiguous float64 [n,{RECORD}] tensor")
    n = int(records_dev.shape[0])
    if out is None:
        out = torch.empty(n, K, K, dtype=torch.float32, device=records_dev.device)
    _lib.check(_lib.lib().resr_blur_kernels(_lib.ptr(records_dev), n, K, _lib.ptr(out), _lib.stream_ptr(records_dev)), "resr_blur_kernels")
    return out


# ---- the source ------------------------------------------------------------------------------------------------------------------
def _read_tile(path: str) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)      # the bytes imgproc.read_image_rgb divides by 255


def _tile_size(path: str):
    from PIL import Image
    with Image.open(path) as im:      # the header only: nothing is decoded
        return im.size


class DeviceTileSource:
    """`dataset.CUDAPrefetcher`'s contract (`next()` -> batch dict or None, `reset()`, `len()`, `original_dataloader.sampler`) over
    a training set held on the device as uint8 tiles [M,T,T,3].

    `next()` returns {"hr": f32 [B,3,T,T], "kernel1", "kernel2", "sinc_kernel": f32 [B,21,21]}, all on the device.  As in
    CUDAPrefetcher, batch i+1 is drawn and enqueued inside `next()` of batch i: per sample the augmentation code, then the three
    kernel records -- `TrainValidImageDataset.__getitem__`'s order, so next to `degrade.sample_plan` the global draw sequence of
    `random` / `np.random` is the loader path's at num_workers=0.  Per batch: one pinned upload (records, indices, codes) and two
    launches on the source's side stream; the consumer is ordered behind them by an event, and the caching allocator is told of the
    consumer stream.  Nothing synchronises with the host.

    The order of a pass is `sampler`'s (default: torch's RandomSampler over range(M); a DistributedSampler for world > 1), batched
    with drop_last=True."""

    def __init__(self, tiles: torch.Tensor, batch_size: int, sampler=None, P: dict = MODEL_P) -> None:
        _lib.require_cuda(tiles, "DeviceTileSource")
        if tiles.dtype != torch.uint8 or tiles.dim() != 4 or tiles.shape[1] != tiles.shape[2] or tiles.shape[3] != 3:
            raise ValueError(f"DeviceTileSource: tiles must be uint8 [M,T,T,3], got {tiles.dtype} {tuple(tiles.shape)}")
        if batch_size < 1:
            raise ValueError(f"DeviceTileSource: batch_size {batch_size}")
        self.tiles = tiles.contiguous()
        self.device = tiles.device
        self.batch_size = int(batch_size)
        self.parameters = P
        self.M, self.T = int(tiles.shape[0]), int(tiles.shape[1])
        if sampler is None:
            sampler = torch.utils.data.RandomSampler(range(self.M))
        self._batches = torch.utils.data.BatchSampler(sampler, self.batch_size, drop_last=True)
        # what the epoch loops of the train scripts look at: `original_dataloader.sampler.set_epoch`
        self.original_dataloader = types.SimpleNamespace(sampler=sampler, batch_size=self.batch_size, drop_last=True)
        self._side = torch.cuda.Stream(device=self.device)
        self._side.wait_stream(torch.cuda.current_stream(self.device))      # the upload of the tiles
        B = self.batch_size
        self._rec_bytes, self._idx_bytes = 3 * B * RECORD * 8, B * 4
        self._it = None
        self._staged = None
        self.reset()

    # -- construction --
    @staticmethod
    def _budget(M: int, T: int, max_bytes: int) -> None:
        if M * T * T * 3 > max_bytes:
            raise ValueError(f"device data source: {M} tiles of {T}x{T}x3 bytes are {M * T * T * 3} bytes, above max_bytes={max_bytes}")

    @classmethod
    def from_array(cls, tiles_u8, batch_size: int, device, sampler=None, max_bytes: int = DEFAULT_MAX_BYTES, P: dict = MODEL_P):
        """uint8 [M,T,T,3] (numpy or a host tensor) -> a source on `device`."""
        a = tiles_u8.numpy() if torch.is_tensor(tiles_u8) else np.asarray(tiles_u8)
        if a.dtype != np.uint8 or a.ndim != 4 or a.shape[1] != a.shape[2] or a.shape[3] != 3 or a.shape[0] < 1:
            raise ValueError(f"device data source: expected uint8 [M,T,T,3] tiles, got {a.dtype} {a.shape}")
        cls._budget(a.shape[0], a.shape[1], max_bytes)
        host = torch.from_numpy(np.ascontiguousarray(a)).pin_memory()
        return cls(host.to(torch.device(device), non_blocking=True), batch_size, sampler, P)

    @classmethod
    def from_dir(cls, image_dir: str, batch_size: int, device, sampler=None, max_bytes: int = DEFAULT_MAX_BYTES, P: dict = MODEL_P,
                 chunk: int = 64):
        """Every file of `image_dir` (in `TrainValidImageDataset`'s order: os.listdir) decoded once with PIL on a thread pool and
        moved through two pinned staging buffers of `chunk` tiles into one uint8 [M,T,T,3] device tensor."""
        from concurrent.futures import ThreadPoolExecutor
        device = torch.device(device)
        paths = [os.path.join(image_dir, name) for name in os.listdir(image_dir)]
        if not paths:
            raise ValueError(f"device data source: no files in {image_dir}")
        workers = max(1, min(16, os.cpu_count() or 1))
        with ThreadPoolExecutor(max_workers=workers) as pool:      # the headers first: every refusal comes before any device work
            sizes = list(pool.map(_tile_size, paths))
        T = sizes[0][0]
        for path, (w, h) in zip(paths, sizes):
            if w != h:
                raise ValueError(f"device data source: {path} is {w}x{h}, not a square tile")
            if w != T:
                raise ValueError(f"device data source: {path} is {w}x{h}, expected the {T}x{T} tile of {paths[0]}")
        M = len(paths)
        cls._budget(M, T, max_bytes)
        tiles = torch.empty(M, T, T, 3, dtype=torch.uint8, device=device)
        chunk = max(1, min(chunk, M))
        staging = [torch.empty(chunk, T, T, 3, dtype=torch.uint8).pin_memory() for _ in range(2)]
        free = [None, None]      # the event behind the last copy out of each staging buffer

        def decode(job):
            slot, path = job
            a = _read_tile(path)
            if a.shape != (T, T, 3):
                raise ValueError(f"device data source: {path} is {a.shape[1]}x{a.shape[0]}, expected the {T}x{T} tile of {paths[0]}")
            np.copyto(slot.numpy(), a)

        with ThreadPoolExecutor(max_workers=workers) as pool:
            for k, start in enumerate(range(0, M, chunk)):
                buf, n = staging[k % 2], min(chunk, M - start)
                if free[k % 2] is not None:
                    free[k % 2].synchronize()       # start-up only: the buffer is read by an earlier copy
                list(pool.map(decode, [(buf[i], paths[start + i]) for i in range(n)]))
                tiles[start:start + n].copy_(buf[:n], non_blocking=True)
                free[k % 2] = torch.cuda.Event()
                free[k % 2].record(torch.cuda.current_stream(device))
        for e in free:
            if e is not None:
                e.synchronize()                     # the staging buffers go back to the allocator after this
        return cls(tiles, batch_size, sampler, P)

    # -- the batch source --
    def _stage(self) -> None:
        try:
            indices = next(self._it)
        except StopIteration:
            self._staged = None
            return
        B = self.batch_size
        if len(indices) != B or min(indices) < 0 or max(indices) >= self.M:
            raise IndexError(f"device data source: the sampler gave {indices} for {self.M} tiles and batch size {B}")
        host = torch.empty(self._rec_bytes + self._idx_bytes + B, dtype=torch.uint8, pin_memory=True)
        raw = host.numpy()
        rec = raw[:self._rec_bytes].view(np.float64).reshape(3, B, RECORD)      # kernel-major: [kernel1 | kernel2 | sinc_kernel] x B
        idx = raw[self._rec_bytes:self._rec_bytes + self._idx_bytes].view(np.int32)
        aug = raw[self._rec_bytes + self._idx_bytes:]
        for b, i in enumerate(indices):
            idx[b] = i
            aug[b] = sample_augment()
            rec[:, b] = sample_blur_params(self.parameters)
        check_blur_records(rec, KERNEL_SIDE)
        with torch.cuda.stream(self._side):
            dev = host.to(self.device, non_blocking=True)
            records = dev[:self._rec_bytes].view(torch.float64).view(3 * B, RECORD)
            index = dev[self._rec_bytes:self._rec_bytes + self._idx_bytes].view(torch.int32)
            codes = dev[self._rec_bytes + self._idx_bytes:]
            hr = tile_batch(self.tiles, index, codes)
            kernels = blur_kernels(records, KERNEL_SIDE)
            done = torch.cuda.Event()
            done.record(self._side)
        batch = {"hr": hr, "kernel1": kernels[:B], "kernel2": kernels[B:2 * B], "sinc_kernel": kernels[2 * B:]}
        self._staged = (batch, done)

    def next(self):
        if self._staged is None:
            return None
        batch, done = self._staged
        consumer = torch.cuda.current_stream(self.device)
        consumer.wait_event(done)
        for v in batch.values():
            v.record_stream(consumer)
        self._stage()
        return batch

    def reset(self) -> None:
        self._it = iter(self._batches)
        self._stage()

    def __len__(self) -> int:
        return len(self._batches)


# ---- the paired source: the definition -------------------------------------------------------------------------------------------
PAIR_SCALES = (1, 2, 3, 4)


def paired_sample_np(hr_u8: np.ndarray, lr_u8: np.ndarray, top: int, left: int, code: int, patch: int, scale: int):
    """THE definition of one paired sample: hr uint8 [s*h, s*w, 3] and lr uint8 [h, w, 3] -> (lr float32 [3, P, P], hr float32
    [3, s*P, s*P]), P = patch, s = scale.  The LR crop is lr[top:top+P, left:left+P], the HR crop its `scale`-times block; both get
    the same dihedral code -- bit 0 a horizontal flip, bit 1 a vertical flip, bit 2 a transpose, in that order --, then
    astype(float32) / float32(255) and HWC -> CHW."""
    hr_u8, lr_u8 = np.asarray(hr_u8), np.asarray(lr_u8)
    top, left, code, P, s = int(top), int(left), int(code), int(patch), int(scale)
    for name, a in (("hr", hr_u8), ("lr", lr_u8)):
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"paired_sample_np: {name} must be uint8 [H, W, 3], got {a.dtype} {a.shape}")
    h, w = lr_u8.shape[:2]
    if s not in PAIR_SCALES or P < 1:
        raise ValueError(f"paired_sample_np: scale {scale} outside 1..4, or patch {patch} below 1")
    if hr_u8.shape[:2] != (s * h, s * w):
        raise ValueError(f"paired_sample_np: hr is {hr_u8.shape[0]}x{hr_u8.shape[1]}, not {s} x the {h}x{w} lr")
    if not (0 <= top <= h - P and 0 <= left <= w - P):
        raise ValueError(f"paired_sample_np: the {P}x{P} crop at (top {top}, left {left}) leaves the {h}x{w} lr image")
    if not 0 <= code < 8:
        raise ValueError(f"paired_sample_np: code {code} outside 0..7")
    out = []
    for a in (lr_u8[top:top + P, left:left + P], hr_u8[s * top:s * top + s * P, s * left:s * left + s * P]):
        if code & 1:
            a = a[:, ::-1]
        if code & 2:
            a = a[::-1]
        if code & 4:
            a = a.transpose(1, 0, 2)
        out.append(np.ascontiguousarray((a.astype(np.float32) / np.float32(255)).transpose(2, 0, 1)))
    return out[0], out[1]


def sample_paired_draw(h: int, w: int, patch: int):
    """The host's draws of one paired sample, five from `random` in this order: top, left, then the three bits of the code."""
    top = random.randint(0, h - patch)
    left = random.randint(0, w - patch)
    code = 0
    for bit in range(3):
        code |= (random.random() < 0.5) << bit
    return top, left, int(code)


def check_paired_records(records, table, patch: int) -> np.ndarray:
    """`records` as an int32 [B, 4] array of (image, top, left, code) rows, or ValueError for what the definition excludes: an image
    index outside 0..M-1, a crop that leaves its image, a code above 7.  `table` is the source's int64 [M, 4] = (hr_offset, lr_offset,
    lr_h, lr_w)."""
    rec = np.asarray(records)
    table = np.asarray(table).reshape(-1, 4)
    if rec.size < 4 or rec.size % 4 or not np.issubdtype(rec.dtype, np.integer):
        raise ValueError(f"paired records: expected integer (image, top, left, code) rows, got {rec.dtype} {rec.shape}")
    rec = rec.reshape(-1, 4).astype(np.int64)
    M = table.shape[0]
    image, top, left, code = rec.T
    bad = np.flatnonzero((image < 0) | (image >= M))
    if bad.size:
        raise ValueError(f"paired records: image index {int(image[bad[0]])} of record {int(bad[0])} outside 0..{M - 1}")
    h, w = table[image, 2], table[image, 3]
    bad = np.flatnonzero((top < 0) | (top > h - patch))
    if bad.size:
        k = int(bad[0])
        raise ValueError(f"paired records: top {int(top[k])} of record {k} takes the {patch}-row crop out of image {int(image[k])} ({int(h[k])}x{int(w[k])})")
    bad = np.flatnonzero((left < 0) | (left > w - patch))
    if bad.size:
        k = int(bad[0])
        raise ValueError(f"paired records: left {int(left[k])} of record {k} takes the {patch}-column crop out of image {int(image[k])} ({int(h[k])}x{int(w[k])})")
    bad = np.flatnonzero((code < 0) | (code > 7))
    if bad.size:
        raise ValueError(f"paired records: code {int(code[bad[0]])} of record {int(bad[0])} outside 0..7")
    return np.ascontiguousarray(rec.astype(np.int32))


def paired_files(hr_dir: str, lr_dir: str):
    """The pairs of two directories: files of the same name, in os.listdir(hr_dir) order, as (hr paths, lr paths).  A file of either
    directory without its partner is a ValueError that names it."""
    names = os.listdir(hr_dir)
    if not names:
        raise ValueError(f"paired data source: no files in {hr_dir}")
    theirs = set(os.listdir(lr_dir))
    for name in names:
        if name not in theirs:
            raise ValueError(f"paired data source: {os.path.join(hr_dir, name)} has no partner {os.path.join(lr_dir, name)}")
    orphans = sorted(theirs - set(names))
    if orphans:
        raise ValueError(f"paired data source: {os.path.join(lr_dir, orphans[0])} has no partner {os.path.join(hr_dir, orphans[0])}")
    return [os.path.join(hr_dir, n) for n in names], [os.path.join(lr_dir, n) for n in names]


def _pair_table(hr_sizes, lr_sizes, names, patch: int, scale: int, max_bytes: int) -> np.ndarray:
    """(h, w) of both sides of every pair -> the int64 [M, 4] table (hr_offset, lr_offset, lr_h, lr_w), images back to back; every
    refusal of a set (host only) is made here and names the pair."""
    if scale not in PAIR_SCALES or patch < 1:
        raise ValueError(f"paired data source: scale {scale} outside 1..4, or patch {patch} below 1")
    if not names:
        raise ValueError("paired data source: no pairs")
    table = np.zeros((len(names), 4), dtype=np.int64)
    hr_off = lr_off = 0
    for i, ((H, W), (h, w), name) in enumerate(zip(hr_sizes, lr_sizes, names)):
        if (H, W) != (scale * h, scale * w):
            raise ValueError(f"paired data source: {name}: the HR side is {W}x{H}, not {scale} x the {w}x{h} LR side")
        if h < patch or w < patch:
            raise ValueError(f"paired data source: {name}: the {w}x{h} LR side is below the patch {patch}")
        table[i] = (hr_off, lr_off, h, w)
        hr_off += H * W * 3
        lr_off += h * w * 3
    if hr_off + lr_off > max_bytes:
        raise ValueError(f"paired data source: {len(names)} pairs are {hr_off} + {lr_off} bytes, above max_bytes={max_bytes}")
    return table


def pair_batch(hr_arena: torch.Tensor, lr_arena: torch.Tensor, table: torch.Tensor, records: torch.Tensor, patch: int, scale: int, out=None):
    """resr_pair_batch on the current stream: both arenas uint8 [bytes], table int64 [M,4], records int32 [B,4] (checked by
    check_paired_records before they were uploaded), all on one device -> (lr float32 [B,3,P,P], hr float32 [B,3,sP,sP]); `out` is
    such a pair to write into."""
    _lib.require_cuda(hr_arena, "pair_batch")
    for name, a in (("hr_arena", hr_arena), ("lr_arena", lr_arena)):
        if a.dtype != torch.uint8 or a.dim() != 1 or not a.is_contiguous() or a.device != hr_arena.device:
            raise ValueError(f"pair_batch: {name} must be a contiguous uint8 [bytes] tensor on the device, got {a.dtype} {tuple(a.shape)}")
    if table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != 4 or not table.is_contiguous() or table.device != hr_arena.device:
        raise ValueError("pair_batch: table must be a contiguous int64 [M,4] tensor on the arenas' device")
    if records.dtype != torch.int32 or records.dim() != 2 or records.shape[1] != 4 or not records.is_contiguous() or records.device != hr_arena.device:
        raise ValueError("pair_batch: records must be a contiguous int32 [B,4] tensor on the arenas' device")
    M, B, P, s = int(table.shape[0]), int(records.shape[0]), int(patch), int(scale)
    if out is None:
        out = (torch.empty(B, 3, P, P, dtype=torch.float32, device=hr_arena.device),
               torch.empty(B, 3, s * P, s * P, dtype=torch.float32, device=hr_arena.device))
    lr, hr = out
    for t, side in ((lr, P), (hr, s * P)):
        if t.dtype != torch.float32 or tuple(t.shape) != (B, 3, side, side) or not t.is_contiguous() or t.device != hr_arena.device:
            raise ValueError(f"pair_batch: out must be contiguous float32 [B,3,{P},{P}] and [B,3,{s * P},{s * P}] tensors on the arenas' device")
    _lib.check(_lib.lib().resr_pair_batch(_lib.ptr(hr_arena), _lib.ptr(lr_arena), _lib.ptr(table), _lib.ptr(records), M, B, P, s, _lib.ptr(lr),
                                          _lib.ptr(hr), _lib.stream_ptr(hr_arena)), "resr_pair_batch")
    return lr, hr


# ---- the paired source -----------------------------------------------------------------------------------------------------------
def _image_size(path: str):
    w, h = _tile_size(path)
    return h, w


def _load_arenas(jobs: dict, device, chunk_bytes: int, workers: int, who: str, arena_bytes: Optional[dict] = None) -> dict:
    """The loader of the arena sources (`PairedDeviceSource.from_dirs`, `ImageCropSource.from_dir`).  `jobs`: arena name -> its images as
    (path, byte offset, (h, w)), back to back in offset order.  Every file is decoded once with PIL on a thread pool of `workers` and
    moved through two pinned staging buffers of `chunk_bytes` (or of the largest image) into one uint8 device tensor per arena;
    `arena_bytes`: arena name -> the size to allocate where an arena is to hold more than these images (the rest is left unwritten)."""
    from concurrent.futures import ThreadPoolExecutor
    totals = {side: jobs[side][-1][1] + jobs[side][-1][2][0] * jobs[side][-1][2][1] * 3 for side in jobs}
    largest = max(h * w * 3 for side in jobs for _, _, (h, w) in jobs[side])
    room = max(largest, min(int(chunk_bytes), max(totals.values())))
    arenas = {side: torch.empty(max(totals[side], (arena_bytes or {}).get(side, 0)), dtype=torch.uint8, device=device) for side in jobs}
    staging = [torch.empty(room, dtype=torch.uint8).pin_memory() for _ in range(2)]
    free = [None, None]      # the event behind the last copy out of each staging buffer

    def decode(job):
        view, path, (h, w) = job
        a = _read_tile(path)
        if a.shape != (h, w, 3):
            raise ValueError(f"{who}: {path} decodes to {a.shape[1]}x{a.shape[0]}, its header said {w}x{h}")
        np.copyto(view.numpy().reshape(h, w, 3), a)

    k = 0
    with ThreadPoolExecutor(max_workers=workers) as pool:
        for side, todo in jobs.items():
            first = 0
            while first < len(todo):
                start = todo[first][1]      # a chunk: consecutive images of the arena, as many as the staging buffer holds
                last = first
                while last < len(todo) and todo[last][1] + todo[last][2][0] * todo[last][2][1] * 3 - start <= room:
                    last += 1
                end = todo[last - 1][1] + todo[last - 1][2][0] * todo[last - 1][2][1] * 3
                buf = staging[k % 2]
                if free[k % 2] is not None:
                    free[k % 2].synchronize()       # start-up only: the buffer is read by an earlier copy
                list(pool.map(decode, [(buf[off - start:off - start + h * w * 3], path, (h, w)) for path, off, (h, w) in todo[first:last]]))
                arenas[side][start:end].copy_(buf[:end - start], non_blocking=True)
                free[k % 2] = torch.cuda.Event()
                free[k % 2].record(torch.cuda.current_stream(device))
                first, k = last, k + 1
    for e in free:
        if e is not None:
            e.synchronize()                         # the staging buffers go back to the allocator after this
    return arenas


class PairedDeviceSource:
    """`degrade.DegradationPrefetcher`'s contract -- `next()` -> (lr, hr, batch) or None, `reset()`, `len()`,
    `original_dataloader.sampler` -- over LR / HR pairs held on the device as uint8: the train scripts iterate it directly
    (config.data_source = "paired"), no degradation stage in between.

    `next()` returns lr f32 [B,3,P,P], hr f32 [B,3,sP,sP] and the dict {"lr", "hr", "index"}, index being the number of the batch
    within the pass.  Batch i+1 is drawn and enqueued inside `next()` of batch i: per sample `sample_paired_draw`, in the batch's
    order -- `dataset.PairedImageDataset.__getitem__`'s draws, so a fixed seed gives the loader path's batches at num_workers=0.
    Per batch: one pinned upload of the records and ONE launch on the source's side stream; the consumer is ordered behind them by
    an event, and the caching allocator is told of the consumer stream.  Nothing synchronises with the host.

    The order of a pass is `sampler`'s (default: torch's RandomSampler over range(M); a DistributedSampler for world > 1), batched
    with drop_last=True."""

    def __init__(self, hr_arena: torch.Tensor, lr_arena: torch.Tensor, table: np.ndarray, batch_size: int, patch: int, scale: int, sampler=None) -> None:
        _lib.require_cuda(hr_arena, "PairedDeviceSource")
        _lib.require_cuda(lr_arena, "PairedDeviceSource")
        if batch_size < 1:
            raise ValueError(f"PairedDeviceSource: batch_size {batch_size}")
        self.table_host = np.ascontiguousarray(np.asarray(table, dtype=np.int64).reshape(-1, 4))
        self.hr_arena, self.lr_arena = hr_arena, lr_arena
        self.device = hr_arena.device
        self.batch_size, self.patch, self.scale = int(batch_size), int(patch), int(scale)
        self.M = int(self.table_host.shape[0])
        self.table = torch.from_numpy(self.table_host).to(self.device)
        if sampler is None:
            sampler = torch.utils.data.RandomSampler(range(self.M))
        self._batches = torch.utils.data.BatchSampler(sampler, self.batch_size, drop_last=True)
        # what the epoch loops of the train scripts look at: `original_dataloader.sampler.set_epoch`
        self.original_dataloader = types.SimpleNamespace(sampler=sampler, batch_size=self.batch_size, drop_last=True)
        self._side = torch.cuda.Stream(device=self.device)
        self._side.wait_stream(torch.cuda.current_stream(self.device))      # the upload of the arenas and the table
        self._it = None
        self._staged = None
        self._count = 0
        self.reset()

    # -- construction --
    @classmethod
    def from_arrays(cls, hr_list, lr_list, batch_size: int, patch: int, scale: int, device, sampler=None, max_bytes: int = DEFAULT_MAX_BYTES):
        """Two lists of uint8 [H,W,3] arrays, hr_list[i] being `scale` x lr_list[i] -> a source on `device`."""
        hr_list, lr_list = [np.asarray(a) for a in hr_list], [np.asarray(a) for a in lr_list]
        if len(hr_list) != len(lr_list):
            raise ValueError(f"paired data source: {len(hr_list)} HR images for {len(lr_list)} LR images")
        for i, a in enumerate(hr_list + lr_list):
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"paired data source: image {i % max(1, len(hr_list))} must be uint8 [H,W,3], got {a.dtype} {a.shape}")
        table = _pair_table([a.shape[:2] for a in hr_list], [a.shape[:2] for a in lr_list], [f"pair {i}" for i in range(len(hr_list))],
                            patch, scale, max_bytes)
        device = torch.device(device)
        arenas = []
        for images in (hr_list, lr_list):
            host = torch.from_numpy(np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in images])).pin_memory()
            arenas.append(host.to(device, non_blocking=True))
        return cls(arenas[0], arenas[1], table, batch_size, patch, scale, sampler)

    @classmethod
    def from_dirs(cls, hr_dir: str, lr_dir: str, batch_size: int, patch: int, scale: int, device, sampler=None,
                  max_bytes: int = DEFAULT_MAX_BYTES, chunk_bytes: int = 64 << 20):
        """The pairs of two directories (`paired_files`) decoded once with PIL on a thread pool and moved through two pinned staging
        buffers into the two arenas.  The headers are read first: a missing partner, an HR size that is not `scale` x the LR size, an
        LR side below `patch` and a total above `max_bytes` are refused, by file name, before any device work."""
        from concurrent.futures import ThreadPoolExecutor
        device = torch.device(device)
        hr_paths, lr_paths = paired_files(hr_dir, lr_dir)
        workers = max(1, min(16, os.cpu_count() or 1))
        with ThreadPoolExecutor(max_workers=workers) as pool:
            hr_sizes, lr_sizes = list(pool.map(_image_size, hr_paths)), list(pool.map(_image_size, lr_paths))
        table = _pair_table(hr_sizes, lr_sizes, hr_paths, patch, scale, max_bytes)
        M = len(hr_paths)
        arenas = _load_arenas({"hr": [(hr_paths[i], int(table[i, 0]), hr_sizes[i]) for i in range(M)],
                               "lr": [(lr_paths[i], int(table[i, 1]), lr_sizes[i]) for i in range(M)]}, device, chunk_bytes, workers,
                              "paired data source")
        return cls(arenas["hr"], arenas["lr"], table, batch_size, patch, scale, sampler)

    # -- the batch source --
    def _stage(self) -> None:
        try:
            indices = next(self._it)
        except StopIteration:
            self._staged = None
            return
        B = self.batch_size
        if len(indices) != B or min(indices) < 0 or max(indices) >= self.M:
            raise IndexError(f"paired data source: the sampler gave {indices} for {self.M} pairs and batch size {B}")
        host = torch.empty(B, 4, dtype=torch.int32, pin_memory=True)
        rec = host.numpy()
        for b, i in enumerate(indices):
            rec[b, 0] = i
            rec[b, 1:] = sample_paired_draw(int(self.table_host[i, 2]), int(self.table_host[i, 3]), self.patch)
        check_paired_records(rec, self.table_host, self.patch)
        with torch.cuda.stream(self._side):
            records = host.to(self.device, non_blocking=True)
            lr, hr = pair_batch(self.hr_arena, self.lr_arena, self.table, records, self.patch, self.scale)
            done = torch.cuda.Event()
            done.record(self._side)
        self._staged = (lr, hr, {"lr": lr, "hr": hr, "index": self._count}, done)
        self._count += 1

    def next(self):
        if self._staged is None:
            return None
        lr, hr, batch, done = self._staged
        consumer = torch.cuda.current_stream(self.device)
        consumer.wait_event(done)
        lr.record_stream(consumer)
        hr.record_stream(consumer)
        self._stage()
        return lr, hr, batch

    def reset(self) -> None:
        self._it = iter(self._batches)
        self._count = 0
        self._stage()

    def __len__(self) -> int:
        return len(self._batches)


# ---- the whole-image source: the definition ----------------------------------------------------------------------------------------
CROP_TABLE_COLUMNS = 3       # (byte offset, h, w)


def reflect101(i: int, n: int) -> int:
    """Index i >= 0 mapped into an axis of length n >= 1 by reflection about the last pixel, period 2n - 2: np.pad(..., mode="reflect") below
    / to the right for a pad of any width, cv2's BORDER_REFLECT_101 for a pad below n."""
    i, n = int(i), int(n)
    if i < 0 or n < 1:
        raise ValueError(f"reflect101: index {i} below 0, or length {n} below 1")
    if n == 1:
        return 0
    p = 2 * n - 2
    j = i % p
    return j if j < n else p - j


def _crop_range(h: int, w: int, T: int):
    """The last legal (top, left) of a T x T window of an h x w image: padding exists only below and to the right."""
    return max(h, T) - T, max(w, T) - T


def crop_sample_np(image_u8: np.ndarray, top: int, left: int, code: int, T: int) -> torch.Tensor:
    """THE definition of one sample of the whole-image source: uint8 [h, w, 3] -> float32 [3, T, T], `augment_np(win, code)` of the window
    win[y, x] = image[reflect101(top + y, h), reflect101(left + x, w)], y, x < T.  Legal: 0 <= top <= max(h, T) - T, 0 <= left <=
    max(w, T) - T -- a window never starts inside the padding of an image that is large enough."""
    image_u8 = np.asarray(image_u8)
    top, left, T = int(top), int(left), int(T)
    if image_u8.dtype != np.uint8 or image_u8.ndim != 3 or image_u8.shape[2] != 3 or image_u8.shape[0] < 1 or image_u8.shape[1] < 1:
        raise ValueError(f"crop_sample_np: expected a uint8 [h, w, 3] image, got {image_u8.dtype} {image_u8.shape}")
    if T < 1:
        raise ValueError(f"crop_sample_np: window side {T} below 1")
    h, w = image_u8.shape[:2]
    top_max, left_max = _crop_range(h, w, T)
    if not (0 <= top <= top_max and 0 <= left <= left_max):
        raise ValueError(f"crop_sample_np: the {T}x{T} window at (top {top}, left {left}) is outside 0..{top_max}, 0..{left_max} of the {h}x{w} image")
    rows = [reflect101(top + y, h) for y in range(T)]
    cols = [reflect101(left + x, w) for x in range(T)]
    return augment_np(np.ascontiguousarray(image_u8[np.ix_(rows, cols)]), code)


def sample_crop_draw(h: int, w: int, T: int):
    """The host's crop draw of one sample, from `random`: top = randint(0, max(h, T) - T) only when h > T, else 0 and NO draw; left the
    same.  On T x T tiles nothing is drawn."""
    top = random.randint(0, h - T) if h > T else 0
    left = random.randint(0, w - T) if w > T else 0
    return top, left


def check_crop_records(records, table, T: int) -> np.ndarray:
    """`records` as an int32 [B, 4] array of (image, top, left, code) rows, or ValueError for what the definition excludes: a wrong shape
    or dtype, an image index outside 0..M-1, a top or left outside the legal range of its image, a code outside 0..15.  `table` is the
    source's int64 [M, 3] = (offset, h, w)."""
    rec = np.asarray(records)
    table = np.asarray(table).reshape(-1, CROP_TABLE_COLUMNS)
    if rec.size < 4 or rec.size % 4 or not np.issubdtype(rec.dtype, np.integer):
        raise ValueError(f"crop records: expected integer (image, top, left, code) rows, got {rec.dtype} {rec.shape}")
    rec = rec.reshape(-1, 4).astype(np.int64)
    M = table.shape[0]
    image, top, left, code = rec.T
    bad = np.flatnonzero((image < 0) | (image >= M))
    if bad.size:
        raise ValueError(f"crop records: image index {int(image[bad[0]])} of record {int(bad[0])} outside 0..{M - 1}")
    h, w = table[image, 1], table[image, 2]
    for name, value, side in (("top", top, h), ("left", left, w)):
        last = np.maximum(side, T) - T
        bad = np.flatnonzero((value < 0) | (value > last))
        if bad.size:
            k = int(bad[0])
            raise ValueError(f"crop records: {name} {int(value[k])} of record {k} outside 0..{int(last[k])}, the legal range of a {T}-pixel window "
                             f"of image {int(image[k])} ({int(h[k])}x{int(w[k])})")
    bad = np.flatnonzero((code < 0) | (code > 15))
    if bad.size:
        raise ValueError(f"crop records: code {int(code[bad[0]])} of record {int(bad[0])} outside 0..15")
    return np.ascontiguousarray(rec.astype(np.int32))


def _crop_table(sizes, names, max_bytes: int, scales=(), short_side: int = 0) -> np.ndarray:
    """(h, w) of every image -> the int64 [M * (1 + K), 3] table (offset, h, w), images back to back: rows 0..M-1 the originals, row
    M * (1 + k) + i copy k of image i (`multiscale_sizes`: the scale copies in the order given, the short-side copy last); every refusal of
    a set (host only) is made here and names the image."""
    scales, short_side = check_train_copies(scales, short_side)
    if not names:
        raise ValueError("image data source: no images")
    M = len(names)
    for (h, w), name in zip(sizes, names):
        if h < 1 or w < 1 or h >= 2 ** 31 or w >= 2 ** 31:
            raise ValueError(f"image data source: {name} is {w}x{h}; a side must be in 1..2^31 - 1")
    copies = [multiscale_sizes(h, w, scales, short_side) for h, w in sizes]
    K = len(scales) + (short_side > 0)
    table = np.zeros((M * (1 + K), CROP_TABLE_COLUMNS), dtype=np.int64)
    off = 0
    for k in range(1 + K):
        for i in range(M):
            h, w = sizes[i] if k == 0 else copies[i][k - 1]
            if h >= 2 ** 31 or w >= 2 ** 31:
                raise ValueError(f"image data source: copy {k - 1} of {names[i]} is {w}x{h}; a side must be in 1..2^31 - 1")
            table[M * k + i] = (off, h, w)
            off += h * w * 3
    if off > max_bytes:
        what = f"{M} images" + (f" and their {K} copies each" if K else "")
        raise ValueError(f"image data source: {what} are {off} bytes, above max_bytes={max_bytes}")
    return table


def crop_batch(arena: torch.Tensor, table: torch.Tensor, records: torch.Tensor, T: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """resr_crop_batch on the current stream: arena uint8 [bytes], table int64 [M,3], records int32 [B,4] (checked by check_crop_records
    before they were uploaded), all on one device -> float32 [B,3,T,T]; `out` is such a tensor to write into."""
    _lib.require_cuda(arena, "crop_batch")
    if arena.dtype != torch.uint8 or arena.dim() != 1 or not arena.is_contiguous():
        raise ValueError(f"crop_batch: arena must be a contiguous uint8 [bytes] tensor on the device, got {arena.dtype} {tuple(arena.shape)}")
    if table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != CROP_TABLE_COLUMNS or not table.is_contiguous() or table.device != arena.device:
        raise ValueError("crop_batch: table must be a contiguous int64 [M,3] tensor on the arena's device")
    if records.dtype != torch.int32 or records.dim() != 2 or records.shape[1] != 4 or not records.is_contiguous() or records.device != arena.device:
        raise ValueError("crop_batch: records must be a contiguous int32 [B,4] tensor on the arena's device")
    M, B, T = int(table.shape[0]), int(records.shape[0]), int(T)
    if T < 1:
        raise ValueError(f"crop_batch: window side {T} below 1")
    if out is None:
        out = torch.empty(B, 3, T, T, dtype=torch.float32, device=arena.device)
    if out.dtype != torch.float32 or tuple(out.shape) != (B, 3, T, T) or not out.is_contiguous() or out.device != arena.device:
        raise ValueError(f"crop_batch: out must be a contiguous float32 [B,3,{T},{T}] tensor on the arena's device")
    _lib.check(_lib.lib().resr_crop_batch(_lib.ptr(arena), _lib.ptr(table), _lib.ptr(records), M, B, T, _lib.ptr(out), _lib.stream_ptr(arena)),
               "resr_crop_batch")
    return out


# ---- multi-scale copies: the definition --------------------------------------------------------------------------------------------
# Pillow's 8-bit `Image.resize(..., LANCZOS)` restated (tests/test_multiscale_surface.py holds it to Pillow itself, bit for bit): per axis a
# table of integer coefficients rounded once to Q22, int32 accumulation, the horizontal pass stored as bytes before the vertical pass, a pass
# over an unchanged axis skipped.
RESAMPLE_BITS = 22
RESAMPLE_MAX_TAPS = 4096
RESAMPLE_JOB_COLUMNS = 8     # (source offset, h, w, destination offset, oh, ow, row table, column table)


def _lanczos3(t: float) -> float:
    if not -3.0 <= t < 3.0:
        return 0.0
    out = 1.0
    for x in (t, t / 3):
        if x != 0.0:
            x = x * math.pi
            out = out * (math.sin(x) / x)
    return out


def resample_ksize(in_size: int, out_size: int, support: float = 3.0) -> int:
    """The taps of one table row: ceil(support * max(in / out, 1)) * 2 + 1."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"resample tables: in_size={in_size} or out_size={out_size} below 1")
    return int(math.ceil(support * max(in_size / out_size, 1.0))) * 2 + 1


def resample_tables_np(in_size: int, out_size: int, support: float = 3.0):
    """THE definition of one axis's table: bounds int32 [out, 2] = (xmin, count) and coeffs int32 [out, ksize], all in Python floats (libm's
    sin): center = (xx + 0.5) * scale, xmin = max(0, int(center - sup + 0.5)), xmax = min(in, int(center + sup + 0.5)), weights
    lanczos((x + xmin - center + 0.5) * (1 / fs)) summed in index order and each divided by the sum, then int(+-0.5 + w * 2^22), truncating.  A
    row with 255 * sum|coeff| + 2^21 >= 2^31 (an int32 sum could overflow) is a ValueError."""
    ksize = resample_ksize(in_size, out_size, support)
    in_size, out_size = int(in_size), int(out_size)
    scale = in_size / out_size
    fs = max(scale, 1.0)
    sup, ss = support * fs, 1.0 / fs
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coeffs = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - sup + 0.5))
        xmax = min(in_size, int(center + sup + 0.5))
        weights = [_lanczos3((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        total = 0.0
        for v in weights:
            total += v
        reach = 0
        for x, v in enumerate(weights):
            if total != 0.0:
                v = v / total
            q = int(-0.5 + v * (1 << RESAMPLE_BITS)) if v < 0 else int(0.5 + v * (1 << RESAMPLE_BITS))
            coeffs[xx, x] = q
            reach += abs(q)
        if 255 * reach + (1 << (RESAMPLE_BITS - 1)) >= 2 ** 31:
            raise ValueError(f"resample tables: row {xx} of {in_size} -> {out_size}: 255 * sum|coeff| + 2^21 would overflow the int32 accumulator")
        bounds[xx] = (xmin, xmax - xmin)
    return bounds, coeffs


def resample_tables(in_size: int, out_size: int):
    """`resample_tables_np` by the library's host builder (resr_resample_tables: the same arithmetic in C++, no GPU call)."""
    lib = _lib.lib()
    ksize = int(lib.resr_resample_ksize(int(in_size), int(out_size)))
    if ksize < 1:
        _lib.check(ksize, "resr_resample_ksize")
    bounds = np.zeros((int(out_size), 2), dtype=np.int32)
    coeffs = np.zeros((int(out_size), ksize), dtype=np.int32)
    _lib.check(lib.resr_resample_tables(int(in_size), int(out_size), bounds.ctypes.data, coeffs.ctypes.data, ksize), "resr_resample_tables")
    return bounds, coeffs


def _resample_axis_np(a: np.ndarray, bounds: np.ndarray, coeffs: np.ndarray) -> np.ndarray:
    """One pass along axis 0 of a uint8 array.  As on the device nothing of `bounds` is trusted for addressing: xmin is clamped into
    0..n - 1, count into 0..min(ksize, n - xmin); the sum is int32 (two's complement)."""
    n, ksize = a.shape[0], coeffs.shape[1]
    out = np.empty((bounds.shape[0],) + a.shape[1:], dtype=np.uint8)
    wide = a.astype(np.int32)
    for xx in range(bounds.shape[0]):
        xmin = min(max(int(bounds[xx, 0]), 0), n - 1)
        count = min(max(int(bounds[xx, 1]), 0), min(ksize, n - xmin))
        acc = np.full(a.shape[1:], 1 << (RESAMPLE_BITS - 1), dtype=np.int32)
        for k in range(count):
            acc += wide[xmin + k] * coeffs[xx, k]
        out[xx] = np.clip(acc >> RESAMPLE_BITS, 0, 255)
    return out


def resample_u8_np(image_u8: np.ndarray, oh: int, ow: int, tables=None) -> np.ndarray:
    """THE definition of a copy: uint8 [h, w, 3] -> uint8 [oh, ow, 3].  The horizontal pass runs when ow != w -- acc = 2^21 + sum_x pixel *
    coeff in int32, out = clip(acc >> 22, 0, 255) --, then the vertical pass on the BYTES of the horizontal result when oh != h; an axis whose
    size does not change is skipped.  `tables` = ((row bounds, row coeffs), (column bounds, column coeffs)) stands in for
    `resample_tables_np(h, oh)` / `(w, ow)` (the table of a skipped axis is not read)."""
    image_u8 = np.asarray(image_u8)
    oh, ow = int(oh), int(ow)
    if image_u8.dtype != np.uint8 or image_u8.ndim != 3 or image_u8.shape[2] != 3 or image_u8.shape[0] < 1 or image_u8.shape[1] < 1:
        raise ValueError(f"resample_u8_np: expected a uint8 [h, w, 3] image, got {image_u8.dtype} {image_u8.shape}")
    if oh < 1 or ow < 1:
        raise ValueError(f"resample_u8_np: output {ow}x{oh} below 1")
    h, w = image_u8.shape[:2]
    out = image_u8
    if ow != w:
        bounds, coeffs = tables[1] if tables is not None else resample_tables_np(w, ow)
        out = _resample_axis_np(out.transpose(1, 0, 2), np.asarray(bounds), np.asarray(coeffs)).transpose(1, 0, 2)
    if oh != h:
        bounds, coeffs = tables[0] if tables is not None else resample_tables_np(h, oh)
        out = _resample_axis_np(out, np.asarray(bounds), np.asarray(coeffs))
    return out.copy() if out is image_u8 else np.ascontiguousarray(out)


def multiscale_sizes(h: int, w: int, scales=(), short_side: int = 0):
    """The (h, w) of the copies of an h x w image, in the order given: a scale s gives (max(1, int(h * s)), max(1, int(w * s))); short_side =
    S > 0 one more, last: the shorter side becomes S and the other max(1, int(S * (longer / shorter)))."""
    h, w = int(h), int(w)
    out = [(max(1, int(h * s)), max(1, int(w * s))) for s in scales]
    S = int(short_side)
    if S > 0:
        out.append((S, max(1, int(S * (w / h)))) if h <= w else (max(1, int(S * (h / w))), S))
    return out


def resample_jobs(pairs, place=None):
    """(source offset, h, w, destination offset, oh, ow) rows -> (jobs int64 [J, 8], tables int32 [words]) for `resample_u8`: the tables of the
    library's host builder, one per distinct (in, out) pair of a changed axis.  `place(words) -> int32 array` hands out the table buffer
    (default: a new array); the builds run wherever `place.map` says (default: here, one after the other)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 6)
    jobs = np.zeros((pairs.shape[0], RESAMPLE_JOB_COLUMNS), dtype=np.int64)
    jobs[:, :6] = pairs
    where, words = {}, 0
    for j, (_, h, w, _, oh, ow) in enumerate(pairs.tolist()):
        for column, (n, out) in ((6, (h, oh)), (7, (w, ow))):
            if n != out and (n, out) not in where:
                where[(n, out)] = words
                words += out * (2 + _native_ksize(n, out))
            jobs[j, column] = where.get((n, out), 0)
    tables = place(max(words, 1)) if place is not None else np.zeros(max(words, 1), dtype=np.int32)
    base = tables.ctypes.data
    lib = _lib.lib()

    def build(item):
        (n, out), at = item
        _lib.check(lib.resr_resample_tables(n, out, base + 4 * at, base + 4 * (at + 2 * out), _native_ksize(n, out)), "resr_resample_tables")
    list(getattr(place, "map", map)(build, where.items()))
    return jobs, tables


def _native_ksize(in_size: int, out_size: int) -> int:
    ksize = int(_lib.lib().resr_resample_ksize(int(in_size), int(out_size)))
    if ksize < 1:
        _lib.check(ksize, "resr_resample_ksize")
    if ksize > RESAMPLE_MAX_TAPS:
        raise ValueError(f"resample tables: {in_size} -> {out_size} takes {ksize} taps a row, above {RESAMPLE_MAX_TAPS}")
    return ksize


def resample_u8(arena: torch.Tensor, jobs, tables: torch.Tensor, jobs_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """resr_resample_u8 on the current stream: arena uint8 [bytes] and tables int32 [words] on one device, jobs int64 [J, 8] on the HOST
    (numpy or a CPU tensor: the library checks them before the launch -- sizes, tables and ranges inside their buffers, no destination
    overlapping a source or another destination); `jobs_dev` is their copy on the device where the caller has made one already.  Every job's
    image is resampled inside the arena; returns the arena."""
    _lib.require_cuda(arena, "resample_u8")
    if arena.dtype != torch.uint8 or arena.dim() != 1 or not arena.is_contiguous():
        raise ValueError(f"resample_u8: arena must be a contiguous uint8 [bytes] tensor on the device, got {arena.dtype} {tuple(arena.shape)}")
    if tables.dtype != torch.int32 or tables.dim() != 1 or not tables.is_contiguous() or tables.device != arena.device:
        raise ValueError("resample_u8: tables must be a contiguous int32 [words] tensor on the arena's device")
    host = jobs.numpy() if torch.is_tensor(jobs) and not jobs.is_cuda else jobs
    if not isinstance(host, np.ndarray) or host.dtype != np.int64 or host.ndim != 2 or host.shape[1] != RESAMPLE_JOB_COLUMNS:
        raise ValueError(f"resample_u8: jobs must be an int64 [J,{RESAMPLE_JOB_COLUMNS}] array on the host")
    host = np.ascontiguousarray(host)
    if jobs_dev is None:
        jobs_dev = torch.from_numpy(host).to(arena.device)
    if (jobs_dev.dtype != torch.int64 or tuple(jobs_dev.shape) != host.shape or not jobs_dev.is_contiguous() or jobs_dev.device != arena.device):
        raise ValueError(f"resample_u8: jobs_dev must be a contiguous int64 {list(host.shape)} tensor on the arena's device")
    _lib.check(_lib.lib().resr_resample_u8(_lib.ptr(arena), int(arena.numel()), host.ctypes.data, _lib.ptr(jobs_dev), int(host.shape[0]), _lib.ptr(tables),
                                           int(tables.numel()), _lib.stream_ptr(arena)), "resr_resample_u8")
    return arena


class _Staged:
    """`resample_jobs`'s `place`: the tables go straight into a pinned staging buffer, behind the jobs' words, and are built on a thread pool."""

    def __init__(self, buffer: torch.Tensor, skip: int, pool) -> None:
        self.buffer, self.skip, self.map = buffer, skip, pool.map

    def __call__(self, words: int) -> np.ndarray:
        return self.buffer.numpy()[self.skip:self.skip + 4 * words].view(np.int32)


def _make_copies(arena: torch.Tensor, table: np.ndarray, M: int, chunk_bytes: int, workers: int) -> None:
    """The copies of a whole-image arena whose rows 0..M-1 are in place: row r >= M is the resample of row r % M.  Bounded groups of jobs;
    per group the tables are built on a thread pool of `workers` straight into one of two pinned staging buffers of `chunk_bytes` (or of the
    largest job), one upload and ONE launch on the current stream.  The host waits only for a staging buffer's earlier upload."""
    from concurrent.futures import ThreadPoolExecutor
    rows = table.shape[0]
    if rows == M:
        return
    pairs = [(int(table[r % M, 0]), int(table[r % M, 1]), int(table[r % M, 2]), int(table[r, 0]), int(table[r, 1]), int(table[r, 2])) for r in range(M, rows)]

    def need(h, w, oh, ow, seen):      # bytes a job adds to a group that holds the tables `seen`
        new = {(n, out) for n, out in ((h, oh), (w, ow)) if n != out and (n, out) not in seen}
        return 8 * RESAMPLE_JOB_COLUMNS + 4 * sum(out * (2 + _native_ksize(n, out)) for n, out in new), new
    room = max([int(chunk_bytes)] + [need(h, w, oh, ow, set())[0] + 4 for _, h, w, _, oh, ow in pairs])
    groups, seen, used = [[]], set(), 4
    for job in pairs:
        cost, new = need(*job[1:3], *job[4:6], seen)
        if groups[-1] and (used + cost > room or len(groups[-1]) == 65535):
            groups.append([])
            seen, used = set(), 4
            cost, new = need(*job[1:3], *job[4:6], seen)
        groups[-1].append(job)
        seen |= new
        used += cost
    staging = [torch.empty(room, dtype=torch.uint8).pin_memory() for _ in range(min(2, len(groups)))]
    free = [None, None]      # the event behind the last upload out of each staging buffer
    with ThreadPoolExecutor(max_workers=workers) as pool:
        for k, group in enumerate(groups):
            buf = staging[k % 2]
            if free[k % 2] is not None:
                free[k % 2].synchronize()       # start-up only: the buffer is read by an earlier upload
            head = 8 * RESAMPLE_JOB_COLUMNS * len(group)
            jobs, tables = resample_jobs(group, _Staged(buf, head, pool))
            buf.numpy()[:head].view(np.int64)[:] = jobs.reshape(-1)
            dev = buf[:head + 4 * tables.size].to(arena.device, non_blocking=True)
            free[k % 2] = torch.cuda.Event()
            free[k % 2].record(torch.cuda.current_stream(arena.device))
            resample_u8(arena, jobs, dev[head:].view(torch.int32), jobs_dev=dev[:head].view(torch.int64).view(len(group), RESAMPLE_JOB_COLUMNS))
    for e in free:
        if e is not None:
            e.synchronize()                     # the staging buffers go back to the allocator after this


# ---- the whole-image source --------------------------------------------------------------------------------------------------------
class ImageCropSource:
    """`DeviceTileSource`'s contract -- `next()` -> {"hr": f32 [B,3,T,T], "kernel1", "kernel2", "sinc_kernel": f32 [B,21,21]} or None,
    `reset()`, `len()`, `original_dataloader.sampler` -- over training images of ANY size held on the device as uint8 in one arena
    (config.data_source = "images"): a sample is a random T x T window of its image, reflect-padded below / to the right where the image
    is smaller (`crop_sample_np`), so a folder of whole images needs no offline tiling.

    Batch i+1 is drawn and enqueued inside `next()` of batch i: per sample `sample_crop_draw`, `sample_augment`, then
    `sample_blur_params` -- `dataset.CropImageDataset.__getitem__`'s order, so a fixed seed gives that loader path's batches at
    num_workers=0; on a set of T x T tiles no crop draw is made and the draws and batches are `DeviceTileSource`'s.  Per batch: one pinned
    upload (blur records, crop records) and two launches on the source's side stream (resr_crop_batch, resr_blur_kernels); the consumer is
    ordered behind them by an event, and the caching allocator is told of the consumer stream.  Nothing synchronises with the host.

    The order of a pass is `sampler`'s (default: torch's RandomSampler over range(M); a DistributedSampler for world > 1), batched with
    drop_last=True.  M counts the table's rows: with multi-scale copies (`from_dir` / `from_arrays`, `scales` / `short_side`) every copy is
    an image of the set like any other, made once at construction; a batch is the same launch over a longer table."""

    def __init__(self, arena: torch.Tensor, table: np.ndarray, batch_size: int, tile: int, sampler=None, P: dict = MODEL_P) -> None:
        _lib.require_cuda(arena, "ImageCropSource")
        if batch_size < 1 or int(tile) < 1:
            raise ValueError(f"ImageCropSource: batch_size {batch_size} or tile {tile} below 1")
        self.table_host = np.ascontiguousarray(np.asarray(table, dtype=np.int64).reshape(-1, CROP_TABLE_COLUMNS))
        self.arena = arena
        self.device = arena.device
        self.batch_size, self.T = int(batch_size), int(tile)
        self.parameters = P
        self.M = int(self.table_host.shape[0])
        self.table = torch.from_numpy(self.table_host).to(self.device)
        if sampler is None:
            sampler = torch.utils.data.RandomSampler(range(self.M))
        self._batches = torch.utils.data.BatchSampler(sampler, self.batch_size, drop_last=True)
        # what the epoch loops of the train scripts look at: `original_dataloader.sampler.set_epoch`
        self.original_dataloader = types.SimpleNamespace(sampler=sampler, batch_size=self.batch_size, drop_last=True)
        self._side = torch.cuda.Stream(device=self.device)
        self._side.wait_stream(torch.cuda.current_stream(self.device))      # the upload of the arena and the table
        self._rec_bytes = 3 * self.batch_size * RECORD * 8
        self._it = None
        self._staged = None
        self.reset()

    # -- construction --
    @classmethod
    def from_arrays(cls, images, batch_size: int, tile: int, device, sampler=None, max_bytes: int = DEFAULT_MAX_BYTES, P: dict = MODEL_P,
                    scales=(), short_side: int = 0):
        """A list of uint8 [h,w,3] arrays of any sizes -> a source on `device`; `scales` / `short_side`: as `from_dir`."""
        if int(tile) < 1:
            raise ValueError(f"image data source: tile {tile} below 1")
        images = [np.asarray(a) for a in images]
        for i, a in enumerate(images):
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"image data source: image {i} must be uint8 [h,w,3], got {a.dtype} {a.shape}")
        table = _crop_table([a.shape[:2] for a in images], [f"image {i}" for i in range(len(images))], max_bytes, scales, short_side)
        host = torch.from_numpy(np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in images])).pin_memory()
        if table.shape[0] == len(images):
            return cls(host.to(torch.device(device), non_blocking=True), table, batch_size, tile, sampler, P)
        arena = torch.empty(int(table[-1, 0] + table[-1, 1] * table[-1, 2] * 3), dtype=torch.uint8, device=torch.device(device))
        arena[:host.numel()].copy_(host, non_blocking=True)
        _make_copies(arena, table, len(images), 64 << 20, max(1, min(16, os.cpu_count() or 1)))
        return cls(arena, table, batch_size, tile, sampler, P)

    @classmethod
    def from_dir(cls, image_dir: str, batch_size: int, tile: int, device, sampler=None, max_bytes: int = DEFAULT_MAX_BYTES, P: dict = MODEL_P,
                 chunk_bytes: int = 64 << 20, scales=(), short_side: int = 0):
        """Every file of `image_dir` (os.listdir order, `.convert("RGB")`), of any size from 1 x 1, through `PairedDeviceSource.from_dirs`'s
        loader into one arena.  The headers are read first: an empty directory and a total above `max_bytes` are refused before any device
        work.

        `scales` (each in (0, 1)) and `short_side` (S > 0) add the multi-scale copies of upstream's data preparation to the set, made on the
        device once the originals are resident (`multiscale_sizes`, `resample_u8_np`: Pillow's LANCZOS resize, bit for bit): table rows
        0..M-1 stay the originals, row M * (1 + k) + i is copy k of image i.  The total that `max_bytes` bounds includes the copies."""
        from concurrent.futures import ThreadPoolExecutor
        if int(tile) < 1:
            raise ValueError(f"image data source: tile {tile} below 1")
        device = torch.device(device)
        paths = [os.path.join(image_dir, name) for name in os.listdir(image_dir)]
        if not paths:
            raise ValueError(f"image data source: no files in {image_dir}")
        workers = max(1, min(16, os.cpu_count() or 1))
        with ThreadPoolExecutor(max_workers=workers) as pool:
            sizes = list(pool.map(_image_size, paths))
        table = _crop_table(sizes, paths, max_bytes, scales, short_side)
        arenas = _load_arenas({"images": [(paths[i], int(table[i, 0]), sizes[i]) for i in range(len(paths))]}, device, chunk_bytes, workers,
                              "image data source", {"images": int(table[-1, 0] + table[-1, 1] * table[-1, 2] * 3)})
        _make_copies(arenas["images"], table, len(paths), chunk_bytes, workers)
        return cls(arenas["images"], table, batch_size, tile, sampler, P)

    # -- the batch source --
    def _stage(self) -> None:
        try:
            indices = next(self._it)
        except StopIteration:
            self._staged = None
            return
        B = self.batch_size
        if len(indices) != B or min(indices) < 0 or max(indices) >= self.M:
            raise IndexError(f"image data source: the sampler gave {indices} for {self.M} images and batch size {B}")
        host = torch.empty(self._rec_bytes + B * 16, dtype=torch.uint8, pin_memory=True)
        raw = host.numpy()
        rec = raw[:self._rec_bytes].view(np.float64).reshape(3, B, RECORD)      # kernel-major: [kernel1 | kernel2 | sinc_kernel] x B
        crops = raw[self._rec_bytes:].view(np.int32).reshape(B, 4)
        for b, i in enumerate(indices):
            top, left = sample_crop_draw(int(self.table_host[i, 1]), int(self.table_host[i, 2]), self.T)
            crops[b] = (i, top, left, sample_augment())
            rec[:, b] = sample_blur_params(self.parameters)
        check_crop_records(crops, self.table_host, self.T)
        check_blur_records(rec, KERNEL_SIDE)
        with torch.cuda.stream(self._side):
            dev = host.to(self.device, non_blocking=True)
            records = dev[:self._rec_bytes].view(torch.float64).view(3 * B, RECORD)
            hr = crop_batch(self.arena, self.table, dev[self._rec_bytes:].view(torch.int32).view(B, 4), self.T)
            kernels = blur_kernels(records, KERNEL_SIDE)
            done = torch.cuda.Event()
            done.record(self._side)
        batch = {"hr": hr, "kernel1": kernels[:B], "kernel2": kernels[B:2 * B], "sinc_kernel": kernels[2 * B:]}
        self._staged = (batch, done)

    def next(self):
        if self._staged is None:
            return None
        batch, done = self._staged
        consumer = torch.cuda.current_stream(self.device)
        consumer.wait_event(done)
        for v in batch.values():
            v.record_stream(consumer)
        self._stage()
        return batch

    def reset(self) -> None:
        self._it = iter(self._batches)
        self._stage()

    def __len__(self) -> int:
        return len(self._batches)


# ---- the training pair pool: the definition ----------------------------------------------------------------------------------------
# The rule (upstream Real-ESRGAN's training pair pool, restated): finished (lr, hr) pairs go into a queue of Q samples.  While fewer
# than Q samples are stored, a batch of B is written to slots ptr..ptr+B-1, ptr += B, and handed out unchanged.  Once the pool is full,
# every step hands out B pooled samples and stores the incoming ones in their slots.  Upstream permutes the whole pool and takes its
# first B; the first B positions of a uniform permutation are a uniformly random ordered B-subset, which is what `sample_pool_slots`
# draws -- so the pool here never moves, and only the B slots drawn are touched.
POOL_DEFAULT_MAX_BYTES = 8 << 30


def _pool_views(who: str, pool_lr, pool_hr, lr, hr, slots):
    """The four arrays as int32 views (bits are moved) and the checked slots."""
    arrays = []
    for name, a in (("pool_lr", pool_lr), ("pool_hr", pool_hr), ("lr", lr), ("hr", hr)):
        if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim < 2 or not a.flags["C_CONTIGUOUS"]:
            raise ValueError(f"{who}: {name} must be a C-contiguous float32 array [n, ...]")
        arrays.append(a.view(np.int32))
    p_lr, p_hr, b_lr, b_hr = arrays
    if p_lr.shape[0] != p_hr.shape[0] or b_lr.shape[0] != b_hr.shape[0] or p_lr.shape[1:] != b_lr.shape[1:] or p_hr.shape[1:] != b_hr.shape[1:]:
        raise ValueError(f"{who}: pools {pool_lr.shape} / {pool_hr.shape} do not hold samples of the batch {lr.shape} / {hr.shape}")
    return p_lr, p_hr, b_lr, b_hr, check_pool_slots(slots, p_lr.shape[0], b_lr.shape[0])


def pool_exchange_np(pool_lr: np.ndarray, pool_hr: np.ndarray, lr: np.ndarray, hr: np.ndarray, slots):
    """THE definition of an exchange: for i < B, out_lr[i] = pool_lr[slots[i]], then pool_lr[slots[i]] = lr[i]; the same for hr.  Returns
    (out_lr, out_hr) and updates the pools in place.  float32 arrays [Q, ...] and [B, ...]; bits are moved, there is no arithmetic."""
    p_lr, p_hr, b_lr, b_hr, slots = _pool_views("pool_exchange_np", pool_lr, pool_hr, lr, hr, slots)
    out_lr, out_hr = np.empty_like(b_lr), np.empty_like(b_hr)
    for i, s in enumerate(slots.tolist()):
        out_lr[i] = p_lr[s]
        p_lr[s] = b_lr[i]
        out_hr[i] = p_hr[s]
        p_hr[s] = b_hr[i]
    return out_lr.view(np.float32), out_hr.view(np.float32)


def pool_store_np(pool_lr: np.ndarray, pool_hr: np.ndarray, lr: np.ndarray, hr: np.ndarray, slots) -> None:
    """The fill form of `pool_exchange_np`: the stores only."""
    p_lr, p_hr, b_lr, b_hr, slots = _pool_views("pool_store_np", pool_lr, pool_hr, lr, hr, slots)
    for i, s in enumerate(slots.tolist()):
        p_lr[s] = b_lr[i]
        p_hr[s] = b_hr[i]


def sample_pool_slots(rng: random.Random, Q: int, B: int):
    """The host's draw of one exchange: B different slots of 0..Q-1 in a random order, from `rng` -- a `random.Random` the pool owns,
    so `random`, `numpy.random` and torch's generators are never touched."""
    return rng.sample(range(Q), B)


def check_pool_slots(slots, Q: int, B: int) -> np.ndarray:
    """`slots` as an int32 [B] array, or ValueError for what the definition excludes: a count other than B, a slot outside 0..Q-1, a
    slot named twice.  Called before every upload."""
    s = np.asarray(slots)
    if s.ndim != 1 or not np.issubdtype(s.dtype, np.integer) or s.size != B:
        raise ValueError(f"pool slots: expected {B} integer slots, got {s.dtype} {s.shape}")
    s = s.astype(np.int64)
    bad = np.flatnonzero((s < 0) | (s >= Q))
    if bad.size:
        raise ValueError(f"pool slots: slot {int(s[bad[0]])} of entry {int(bad[0])} outside 0..{Q - 1}")
    order = np.argsort(s, kind="stable")
    twice = np.flatnonzero(np.diff(s[order]) == 0)
    if twice.size:
        j, k = sorted((int(order[twice[0]]), int(order[twice[0] + 1])))
        raise ValueError(f"pool slots: slot {int(s[j])} repeated (entries {j} and {k}): two samples of a batch cannot share a slot")
    return np.ascontiguousarray(s.astype(np.int32))


# ---- the training pair pool: the launch --------------------------------------------------------------------------------------------
def _pool_launch(who: str, pool_lr, pool_hr, lr, hr, slots, out):
    _lib.require_cuda(pool_lr, who)
    dev = pool_lr.device
    for name, t in (("pool_lr", pool_lr), ("pool_hr", pool_hr), ("lr", lr), ("hr", hr)) + ((("out[0]", out[0]), ("out[1]", out[1])) if out else ()):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() < 2 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{who}: {name} must be a contiguous float32 [n, ...] tensor on the pool's device")
    Q, B = int(pool_lr.shape[0]), int(lr.shape[0])
    if pool_hr.shape[0] != Q or hr.shape[0] != B or pool_lr.shape[1:] != lr.shape[1:] or pool_hr.shape[1:] != hr.shape[1:]:
        raise ValueError(f"{who}: pools {tuple(pool_lr.shape)} / {tuple(pool_hr.shape)} do not hold samples of the batch {tuple(lr.shape)} / {tuple(hr.shape)}")
    if out and (out[0].shape != lr.shape or out[1].shape != hr.shape):
        raise ValueError(f"{who}: out must be a pair of the batch's shapes {tuple(lr.shape)} / {tuple(hr.shape)}")
    if slots.dtype != torch.int32 or slots.dim() != 1 or slots.numel() != B or not slots.is_contiguous() or slots.device != dev:
        raise ValueError(f"{who}: slots must be a contiguous int32 [{B}] tensor on the pool's device")
    _lib.check(_lib.lib().resr_pool_exchange(_lib.ptr(pool_lr), _lib.ptr(pool_hr), _lib.ptr(lr), _lib.ptr(hr), _lib.ptr(out[0]) if out else None,
                                             _lib.ptr(out[1]) if out else None, _lib.ptr(slots), Q, B, lr[0].numel(), hr[0].numel(),
                                             _lib.stream_ptr(pool_lr)), "resr_pool_exchange")


def pool_exchange(pool_lr: torch.Tensor, pool_hr: torch.Tensor, lr: torch.Tensor, hr: torch.Tensor, slots: torch.Tensor, out=None):
    """resr_pool_exchange on the current stream: pools float32 [Q, ...], the batch float32 [B, ...] of the same sample shapes, slots
    int32 [B] (checked by check_pool_slots before they were uploaded), all contiguous and on one device -> (out_lr, out_hr), what the
    slots held; the pools now hold the batch there.  `out` is such a pair to write into; (lr, hr) itself swaps in place."""
    if out is None:
        out = (torch.empty_like(lr), torch.empty_like(hr))
    _pool_launch("pool_exchange", pool_lr, pool_hr, lr, hr, slots, tuple(out))
    return out[0], out[1]


def pool_store(pool_lr: torch.Tensor, pool_hr: torch.Tensor, lr: torch.Tensor, hr: torch.Tensor, slots: torch.Tensor) -> None:
    """The fill form of `pool_exchange`, the same launch with no outputs: the batch is stored in its slots, the pools are not read."""
    _pool_launch("pool_store", pool_lr, pool_hr, lr, hr, slots, None)


# ---- the training pair pool: the wrapper -------------------------------------------------------------------------------------------
class PairPool:
    """The training pair pool around a source of (lr, hr, batch) items -- `degrade.DegradationPrefetcher`, `PairedDeviceSource`,
    `dataset.PairedPrefetcher` --, with that contract: `next()` -> (lr, hr, batch) or None, `reset()`, `len()`, and the source's
    `original_dataloader` when it has one.

    `size` samples (Q) are held on the device as fp32 [Q,3,P,P] and [Q,3,sP,sP], allocated at the first batch from that batch's shapes;
    a later batch of another shape is a ValueError.  A size that is no multiple of the batch, a size below the batch and a byte count
    above `max_bytes` are ValueErrors before anything is allocated.  While the pool fills, `next()` stores the source's batch in slots
    ptr..ptr+B-1 and hands the source's own tensors out.  Once it is full, `next()` draws B slots (`sample_pool_slots`), hands out what
    they held and stores the incoming batch there: per step one pinned upload of the checked slots and ONE launch, in line on the
    consumer's current stream, behind the source's own hand-over.  Nothing synchronises with the host.

    The third item is always the INCOMING batch's dictionary, unchanged: it describes what entered the pool in this step, not the
    tensors handed out next to it.  A source's None ends the pass; the pool is not drained.  `reset()` resets the source and keeps the
    pool's contents and fill pointer, `attach(source)` swaps the wrapped source and keeps them too (the train scripts make a new source
    object every epoch).  The pool is not saved in a checkpoint.

    The draws come from the pool's own `random.Random(seed)` (the train scripts pass seed + rank): `random`, `numpy.random` and
    torch's generators are never touched, so under a fixed seed the source, and the degradation stage behind it, produce the same
    sequence with the pool on or off."""

    def __init__(self, source, size: int, seed: int = 0, max_bytes: int = POOL_DEFAULT_MAX_BYTES) -> None:
        if int(size) < 1:
            raise ValueError(f"pair pool: size {size} below 1")
        self.source, self.size, self.max_bytes = source, int(size), int(max_bytes)
        self.filled = 0                      # the fill pointer: samples stored so far, Q once the pool is full
        self.pool_lr = self.pool_hr = None
        self._rng = random.Random(seed)
        self._shapes = None
        self._home = self._last = None

    @property
    def original_dataloader(self):
        return self.source.original_dataloader      # (AttributeError where the source has none)

    def attach(self, source) -> None:
        self.source = source

    def reset(self) -> None:
        self.source.reset()

    def __len__(self) -> int:
        return len(self.source)

    # -- the rule --
    def _admit(self, lr, hr) -> int:
        """The batch size of a batch the pool can take; the first batch sizes the pool (every refusal before the allocation)."""
        shapes = (tuple(lr.shape), tuple(hr.shape))
        if lr.dtype != torch.float32 or hr.dtype != torch.float32 or len(shapes[0]) < 2 or len(shapes[1]) < 2 or shapes[0][0] != shapes[1][0] or shapes[0][0] < 1:
            raise ValueError(f"pair pool: a batch must be float32 [B, ...] on both sides, got {lr.dtype} {shapes[0]} and {hr.dtype} {shapes[1]}")
        B = shapes[0][0]
        if self._shapes is None:
            if self.size < B:
                raise ValueError(f"pair pool: size {self.size} below the batch size {B}")
            if self.size % B:
                raise ValueError(f"pair pool: size {self.size} is not a multiple of the batch size {B}")
            count = self.size * 4 * (math.prod(shapes[0][1:]) + math.prod(shapes[1][1:]))
            if count > self.max_bytes:
                raise ValueError(f"pair pool: {self.size} pairs of {shapes[0][1:]} and {shapes[1][1:]} float32 are {count} bytes, above max_bytes={self.max_bytes}")
            self._allocate(lr, hr)
            self._shapes = shapes
        elif shapes != self._shapes:
            raise ValueError(f"pair pool: a batch of {shapes[0]} / {shapes[1]} after the pool was sized for {self._shapes[0]} / {self._shapes[1]}")
        return B

    def next(self):
        item = self.source.next()
        if item is None:
            return None
        lr, hr, batch = item
        B = self._admit(lr, hr)
        if self.filled < self.size:
            self._store(lr, hr, check_pool_slots(np.arange(self.filled, self.filled + B), self.size, B))
            self.filled += B
            return lr, hr, batch
        out_lr, out_hr = self._exchange(lr, hr, check_pool_slots(sample_pool_slots(self._rng, self.size, B), self.size, B))
        return out_lr, out_hr, batch

    # -- the device: what HostPairPool replaces --
    def _allocate(self, lr, hr) -> None:
        _lib.require_cuda(lr, "PairPool")
        _lib.require_cuda(hr, "PairPool")
        self._home = torch.cuda.current_stream(lr.device)
        self.pool_lr = torch.empty((self.size,) + tuple(lr.shape[1:]), dtype=torch.float32, device=lr.device)
        self.pool_hr = torch.empty((self.size,) + tuple(hr.shape[1:]), dtype=torch.float32, device=hr.device)

    def _launch(self, lr, hr, slots: np.ndarray, swap: bool):
        device = self.pool_lr.device
        consumer = torch.cuda.current_stream(device)
        if self._last is not None:
            consumer.wait_event(self._last)          # the pool's last exchange, on whichever stream it ran
        if consumer != self._home:
            self.pool_lr.record_stream(consumer)
            self.pool_hr.record_stream(consumer)
        host = torch.empty(slots.size, dtype=torch.int32, pin_memory=True)
        host.numpy()[:] = slots
        slots_dev = host.to(device, non_blocking=True)
        lr, hr = lr.contiguous(), hr.contiguous()
        out = pool_exchange(self.pool_lr, self.pool_hr, lr, hr, slots_dev) if swap else pool_store(self.pool_lr, self.pool_hr, lr, hr, slots_dev)
        self._last = torch.cuda.Event()
        self._last.record(consumer)
        return out

    def _store(self, lr, hr, slots: np.ndarray) -> None:
        self._launch(lr, hr, slots, False)

    def _exchange(self, lr, hr, slots: np.ndarray):
        return self._launch(lr, hr, slots, True)


class HostPairPool(PairPool):
    """`PairPool`'s rule -- the same draws, fill and refusals -- over CPU tensors, by `pool_exchange_np` / `pool_store_np`: the mirror
    the device pool is judged against."""

    def _allocate(self, lr, hr) -> None:
        self.pool_lr = torch.zeros((self.size,) + tuple(lr.shape[1:]), dtype=torch.float32)
        self.pool_hr = torch.zeros((self.size,) + tuple(hr.shape[1:]), dtype=torch.float32)

    def _store(self, lr, hr, slots: np.ndarray) -> None:
        pool_store_np(self.pool_lr.numpy(), self.pool_hr.numpy(), lr.contiguous().numpy(), hr.contiguous().numpy(), slots)

    def _exchange(self, lr, hr, slots: np.ndarray):
        out_lr, out_hr = pool_exchange_np(self.pool_lr.numpy(), self.pool_hr.numpy(), lr.contiguous().numpy(), hr.contiguous().numpy(), slots)
        return torch.from_numpy(out_lr), torch.from_numpy(out_hr)
