"""A device-resident training data source: the tiles of the training set live in HBM as uint8, and a batch -- gather, rotate / flip
augmentation, /255, HWC -> CHW, and the 3 x B blur / sinc kernels of the degradation stage -- is two launches on a side stream
(csrc/data_source.hip: resr_tile_batch, resr_blur_kernels).  The host keeps only the random draws, made in the loader path's order
(dataset.py `TrainValidImageDataset.__getitem__` at num_workers=0: the augmentation, then the kernel parameters), so a fixed seed gives
the loader path's batches.  `DeviceTileSource` has `dataset.CUDAPrefetcher`'s contract and sits in its place under
`degrade.DegradationPrefetcher` (config.data_source = "device").

Host definitions (numpy, float64 where the loader path's are): `sample_blur_params` / `blur_kernels_from_params_np` split
`degrade.sample_blur_kernels` into its draws and its arithmetic, `sample_augment` / `augment_np` do the same for the
`imgproc.random_rotate` / `random_horizontally_flip` / `random_vertically_flip` chain.  The kernels are judged against them.
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
from .config import degradation_model_parameters_dict as MODEL_P

__all__ = ["sample_blur_params", "blur_kernels_from_params_np", "check_blur_records", "sample_augment", "augment_np",
           "tile_batch", "blur_kernels", "DeviceTileSource", "RECORD", "FAMILIES"]

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
