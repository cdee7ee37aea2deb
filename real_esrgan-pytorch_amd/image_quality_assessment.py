"""No-reference quality metric of the reference's validation loop: `NIQE`, the module
`train_realesrnet.py:102,430-466` / `train_realesrgan.py` evaluate on every validation batch
(reference image_quality_assessment.py:803-1032, MATLAB NIQE semantics).

`niqe` / `NIQE` are plain torch in float64 on whatever device the SR batch lives on.  `niqe_native` / `NativeNIQE` (opt-in:
`config.niqe_backend`) compute the same 36 features per block with the kernels of csrc/niqe.hip -- from a float [B,3,H,W] batch or
straight from a uint8 [B,H,W,3] frame -- and share the tail of the score (`_score_from_features`) with `niqe`, or, with
`tail="native"` (`config.niqe_tail`), run it as two more launches for the whole batch (`niqe_score_native`): no host round trip.
The prior (mean / covariance of the 36 natural-scene features) is the reference's `results/pretrained_models/niqe_model.mat`; a copy of that data file is kept as a test fixture
(`tests/golden/niqe_model.mat`).

Full-reference metrics ("Native PSNR / SSIM"; the reference has none, include/resr.h is the specification): `psnr` / `ssim` /
`PSNR` / `SSIM` score an SR batch against its ground truth on the Y channel in plain torch float64 (the "torch" backend of
`config.full_ref`); `full_ref_native` / `NativeFullRef` compute both in one pass of csrc/fullref.hip, from float [B,3,H,W] or uint8
[B,H,W,3] tensors on either side.  Not built: MS-SSIM, padding modes, windows other than 11 taps / sigma 1.5.
Per plane ("Native PSNR / SSIM per plane"; resr_fullref_planes): `full_ref_channels_native` scores every channel of a float,
uint8 or uint16 image batch (BasicSR's RGB PSNR / SSIM: `psnr_all`, `ssim_mean`), `full_ref_yuv_native` the stored Y, Cb and Cr planes
of 8- and 10-bit 4:2:0 frames; `full_ref_channels` / `full_ref_yuv` are their torch float64 twins.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import imgproc

__all__ = ["NIQE", "niqe", "NativeNIQE", "niqe_native", "niqe_score_native",
           "PSNR", "SSIM", "psnr", "ssim", "NativeFullRef", "full_ref_native",
           "full_ref_channels", "full_ref_channels_native", "full_ref_yuv", "full_ref_yuv_native", "NativeFullRefChannels", "TorchFullRefChannels"]


def _gaussian_window(size: int = 7, sigma: float = 7.0 / 6.0) -> torch.Tensor:
    """MATLAB fspecial('gaussian'); the reference stores it as float32 before use (iqa.py:215-242)."""
    m = (size - 1) / 2.0
    y, x = np.ogrid[-m:m + 1, -m:m + 1]
    h = np.exp(-(x * x + y * y) / (2.0 * sigma * sigma))
    h[h < np.finfo(h.dtype).eps * h.max()] = 0
    h /= h.sum()
    return torch.from_numpy(h.astype(np.float32))


def _aggd_grid(like: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The shape grid 0.2:0.001:10 and its ratio table r(alpha), in `like`'s dtype and on its device."""
    grid = torch.arange(0.2, 10 + 0.001, 0.001).to(like)                    # float32 grid values, as in the reference
    r_gam = (2 * torch.lgamma(2.0 / grid) - (torch.lgamma(1.0 / grid) + torch.lgamma(3.0 / grid))).exp()
    return grid, r_gam


def _aggd(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Asymmetric generalised Gaussian fit of every block x[n,1,h,w] by moment matching on the grid 0.2:0.001:10
    (iqa.py:803-851, the `get_sigma=True` form): shape alpha, left / right scale."""
    grid, r_gam = _aggd_grid(x)
    neg, pos = x < 0, x > 0
    n_neg = neg.sum(dim=(-1, -2), dtype=torch.float32)
    n_pos = pos.sum(dim=(-1, -2), dtype=torch.float32)
    left = torch.sqrt((x * neg).pow(2).sum(dim=(-1, -2)) / (n_neg + 1e-8))
    right = torch.sqrt((x * pos).pow(2).sum(dim=(-1, -2)) / (n_pos + 1e-8))
    g = left / right
    rhat = x.abs().mean(dim=(-1, -2)).pow(2) / x.pow(2).mean(dim=(-1, -2))
    rhat_norm = rhat * (g.pow(3) + 1) * (g + 1) / (g.pow(2) + 1).pow(2)
    alpha = grid[(r_gam.unsqueeze(0) - rhat_norm).abs().argmin(dim=-1)]     # [n]
    scale = (torch.lgamma(1 / alpha) - torch.lgamma(3 / alpha)).exp().sqrt()
    return alpha, left.squeeze(-1) * scale, right.squeeze(-1) * scale


def _block_features(blocks: torch.Tensor) -> torch.Tensor:
    """18 features of every MSCN block [n,1,h,w] (iqa.py:854-883): AGGD of the block and of its products with the four
    circularly shifted copies (right, down, both diagonals)."""
    alpha, bl, br = _aggd(blocks)
    feats: List[torch.Tensor] = [alpha, (bl + br) / 2]
    for shift in ((0, 1), (1, 0), (1, 1), (1, -1)):
        alpha, bl, br = _aggd(blocks * torch.roll(blocks, shift, dims=(2, 3)))
        mean = (br - bl) * (torch.lgamma(2 / alpha) - torch.lgamma(1 / alpha)).exp()
        feats += [alpha, mean, bl, br]
    return torch.stack(feats, dim=-1)                                       # [n, 18]


def _resize_half(y: torch.Tensor) -> torch.Tensor:
    """MATLAB imresize(., 0.5) with antialiasing, in the tensor's own precision (iqa.py:726-800 for scale 0.5)."""
    _, _, h, w = y.shape
    mh = torch.from_numpy(imgproc._resize_matrix(h, math.ceil(h * 0.5), 0.5, True, np.float64)).to(y)
    mw = torch.from_numpy(imgproc._resize_matrix(w, math.ceil(w * 0.5), 0.5, True, np.float64)).to(y)
    return torch.matmul(torch.matmul(mh, y), mw.t())


def niqe(tensor: torch.Tensor, crop_border: int, mu_prior: torch.Tensor, cov_prior: torch.Tensor,
         block_size_height: int = 96, block_size_width: int = 96) -> torch.Tensor:
    """NIQE score of every image of an RGB batch [B,3,H,W] in [0,1] (iqa.py:886-998)."""
    if crop_border > 0:
        tensor = tensor[:, :, crop_border:-crop_border, crop_border:-crop_border]
    y = (imgproc.rgb2ycbcr_torch(tensor.float(), only_use_y_channel=True) * 255.0).round().to(torch.float64)
    b, _, h, w = y.shape
    nbh, nbw = h // block_size_height, w // block_size_width
    if nbh == 0 or nbw == 0:
        raise ValueError(f"NIQE needs at least one {block_size_height}x{block_size_width} block, got {h}x{w}")
    y = y[..., :nbh * block_size_height, :nbw * block_size_width]
    win = _gaussian_window().to(y).view(1, 1, 7, 7)
    feats = []
    for scale in (1, 2):
        mu = F.conv2d(F.pad(y, (3, 3, 3, 3), mode="replicate"), win)
        sq = F.conv2d(F.pad(y * y, (3, 3, 3, 3), mode="replicate"), win)
        sigma = torch.sqrt((sq - mu * mu).abs() + 1e-8)
        mscn = (y - mu) / (sigma + 1)
        bh, bw = block_size_height // scale, block_size_width // scale
        blocks = F.unfold(mscn, (bh, bw), stride=(bh, bw))                  # [b, bh*bw, nblocks]
        nblk = blocks.shape[-1]
        blocks = blocks.transpose(1, 2).reshape(b * nblk, 1, bh, bw)
        feats.append(_block_features(blocks).reshape(b, nblk, 18))
        if scale == 1:
            y = _resize_half(y / 255.0) * 255.0
    dist = torch.cat(feats, dim=-1)                                         # [b, nblocks, 36]
    return _score_from_features(dist, mu_prior, cov_prior)


def _score_from_features(dist: torch.Tensor, mu_prior: torch.Tensor, cov_prior: torch.Tensor) -> torch.Tensor:
    """The score of every image from its block features [b, nblocks, 36] (iqa.py:960-998): the tail `niqe` and `niqe_native` share."""
    scores = []
    for i in range(dist.shape[0]):                                          # blocks with a NaN feature are dropped
        rows = dist[i]
        nan = torch.isnan(rows)
        mu_d = torch.where(nan, torch.zeros_like(rows), rows).sum(0) / (~nan).to(rows.dtype).sum(0)
        ok = rows[~nan.any(dim=1)]
        c = ok - ok.mean(dim=0, keepdim=True)
        cov_d = c.t() @ c / (ok.shape[0] - 1)
        diff = (mu_prior.to(rows) - mu_d).unsqueeze(0)
        inv = torch.linalg.pinv((cov_prior.to(rows) + cov_d) / 2)
        scores.append(torch.sqrt((diff @ inv @ diff.t()).squeeze()))
    return torch.stack(scores).squeeze()


class NIQE(nn.Module):
    """Same constructor and call as the reference's `NIQE` (iqa.py:1001-1032): `NIQE(crop_border, niqe_model_path)`,
    `forward(sr) -> score` (scalar for a batch of one, else one score per image)."""

    def __init__(self, crop_border: int, niqe_model_path: str, block_size_height: int = 96,
                 block_size_width: int = 96) -> None:
        super().__init__()
        self.crop_border = crop_border
        self.niqe_model_path = niqe_model_path
        self.block_size_height = block_size_height
        self.block_size_width = block_size_width
        import scipy.io
        model = scipy.io.loadmat(niqe_model_path)
        self.register_buffer("mu_prisparam", torch.from_numpy(np.ravel(model["mu_prisparam"]).astype(np.float64)), persistent=False)
        self.register_buffer("cov_prisparam", torch.from_numpy(np.asarray(model["cov_prisparam"], dtype=np.float64)), persistent=False)

    def forward(self, raw_tensor: torch.Tensor) -> torch.Tensor:
        # the reference moves the priors to the image's dtype first (iqa.py:980-984)
        mu = self.mu_prisparam.to(raw_tensor.dtype).to(torch.float64)
        cov = self.cov_prisparam.to(raw_tensor.dtype).to(torch.float64)
        return niqe(raw_tensor, self.crop_border, mu, cov, self.block_size_height, self.block_size_width)


# ---- native backend (csrc/niqe.hip) ----------------------------------------------------------------------------------------------
def half_band_table(n: int) -> Tuple[np.ndarray, np.ndarray]:
    """The non-zero band of `imgproc._resize_matrix(n, ceil(n / 2), 0.5, True, float64)` as (start int32 [out], w float64 [out, P]):
    row i of the matrix is zero outside columns start[i] .. start[i] + P - 1 and equals w[i] there, bit for bit -- the taps are
    accumulated in the order `_resize_matrix` accumulates them, without the dense matrix ever being built."""
    out = math.ceil(n * 0.5)
    idx, w = imgproc._resize_taps(n, out, 0.5, True, np.float64)
    idx = imgproc._reflect_symmetric(idx, n) - 1
    if idx.min() < 0 or idx.max() >= n:
        raise ValueError(f"half_band_table: an axis of {n} pixels is shorter than the symmetric copy its taps reach for")
    p = min(int((idx.max(1) - idx.min(1)).max()) + 1, n)
    start = np.minimum(idx.min(1), n - p)
    band = np.zeros((out, p), np.float64)
    np.add.at(band, (np.repeat(np.arange(out), idx.shape[1]), (idx - start[:, None]).reshape(-1)), w.reshape(-1))
    return start.astype(np.int32), band


_NATIVE_TABLES: dict = {}


def _native_tables(h: int, w: int, device: torch.device) -> dict:
    """Device tables of one luma size, built once: the banded half-size taps, the AGGD grid and ratio table (the module's own torch
    expression, evaluated on the host in float64), the window."""
    key = (h, w, str(device))
    t = _NATIVE_TABLES.get(key)
    if t is None:
        shared = _NATIVE_TABLES.get(("grid", str(device)))
        if shared is None:
            grid, r_gam = _aggd_grid(torch.zeros((), dtype=torch.float64))
            shared = _NATIVE_TABLES[("grid", str(device))] = (grid.to(device), r_gam.to(device))
        sh, wh = half_band_table(h)
        sw, ww = half_band_table(w)
        if len(_NATIVE_TABLES) > 16:                                        # a handful of validation sizes live here, not a history
            for k in [k for k in _NATIVE_TABLES if k[0] != "grid"]:
                del _NATIVE_TABLES[k]
        t = _NATIVE_TABLES[key] = {"start_h": torch.from_numpy(sh).to(device), "w_h": torch.from_numpy(wh).to(device),
                                   "start_w": torch.from_numpy(sw).to(device), "w_w": torch.from_numpy(ww).to(device),
                                   "grid": shared[0], "r_gam": shared[1], "win": _gaussian_window().double().reshape(-1).tolist()}
    return t


def check_native_blocks(bh: int, bw: int) -> None:
    """ValueError for a block size the kernels refuse: an odd side, or an LDS tile (the float64 MSCN block and its halo) beyond a CU's
    160 KiB.  There is no fallback onto the torch path."""
    from . import _lib
    if isinstance(bh, bool) or isinstance(bw, bool) or not isinstance(bh, int) or not isinstance(bw, int) or bh < 2 or bw < 2 or bh % 2 or bw % 2:
        raise ValueError(f"native NIQE needs even block sides of at least 2, got {bh}x{bw}")
    d = _lib.NiqeDesc()
    d.n, d.h, d.w, d.bh, d.bw = 1, bh, bw, bh, bw
    if not _lib.lib().resr_niqe_workspace_bytes(d):
        raise ValueError(f"native NIQE: {_lib.lib().resr_last_error().decode()}")


def niqe_luma_native(tensor: torch.Tensor, crop_border: int, out_h: int, out_w: int) -> torch.Tensor:
    """The luma levels uint8 [B, out_h, out_w] of a float [B,3,H,W] batch in [0,1] or a uint8 [B,H,W,3] batch, read from
    `crop_border` pixels inside the image (resr_niqe_luma_f32 / _u8, on the current stream)."""
    from . import _lib
    _lib.require_cuda(tensor, "niqe_native")
    if tensor.dtype == torch.uint8:
        if tensor.dim() != 4 or tensor.shape[-1] != 3:
            raise ValueError(f"niqe_native: a uint8 batch is [B,H,W,3], got {tuple(tensor.shape)}")
        b, h, w = tensor.shape[:3]
        entry, name = _lib.lib().resr_niqe_luma_u8, "resr_niqe_luma_u8"
    else:
        if tensor.dim() != 4 or tensor.shape[1] != 3 or not tensor.is_floating_point():
            raise ValueError(f"niqe_native: a float batch is [B,3,H,W], got {tensor.dtype} {tuple(tensor.shape)}")
        b, _, h, w = tensor.shape
        tensor = tensor.float()
        entry, name = _lib.lib().resr_niqe_luma_f32, "resr_niqe_luma_f32"
    tensor = tensor.contiguous()
    luma = torch.empty((b, out_h, out_w), dtype=torch.uint8, device=tensor.device)
    _lib.check(entry(_lib.ptr(tensor), _lib.ptr(luma), b, h, w, crop_border, out_h, out_w, _lib.stream_ptr(tensor)), name)
    return luma


def niqe_features_native(luma: torch.Tensor, bh: int = 96, bw: int = 96, keep: bool = False):
    """resr_niqe_features on the current stream: luma uint8 [B,h,w] (h, w multiples of bh, bw) -> float64 [B, blocks, 36].
    keep=True also returns the workspace's contents as views: (features, half-size image [B,h/2,w/2], moments [2,B,blocks,5,6])."""
    from . import _lib
    import ctypes as C
    _lib.require_cuda(luma, "niqe_features_native")
    if luma.dtype != torch.uint8 or luma.dim() != 3 or not luma.is_contiguous():
        raise ValueError(f"niqe_features_native: luma must be a contiguous uint8 [B,h,w] tensor, got {luma.dtype} {tuple(luma.shape)}")
    check_native_blocks(bh, bw)
    b, h, w = luma.shape
    if h < bh or w < bw or h % bh or w % bw:
        raise ValueError(f"niqe_features_native: a luma of {h}x{w} is no whole number of {bh}x{bw} blocks")
    t = _native_tables(h, w, luma.device)
    d = _lib.NiqeDesc()
    d.n, d.h, d.w, d.bh, d.bw = b, h, w, bh, bw
    d.taps_h, d.taps_w, d.n_grid = t["w_h"].shape[1], t["w_w"].shape[1], t["grid"].numel()
    for name in ("start_h", "w_h", "start_w", "w_w", "grid", "r_gam"):
        setattr(d, name, t[name].data_ptr())
    d.win[:] = t["win"]
    need = int(_lib.lib().resr_niqe_workspace_bytes(d))
    if not need:
        raise ValueError(f"native NIQE: {_lib.lib().resr_last_error().decode()}")
    ws = torch.empty(need // 8, dtype=torch.float64, device=luma.device)
    d.workspace, d.workspace_bytes = ws.data_ptr(), need
    nblk = (h // bh) * (w // bw)
    feats = torch.empty((b, nblk, 36), dtype=torch.float64, device=luma.device)
    _lib.check(_lib.lib().resr_niqe_features(C.byref(d), _lib.ptr(luma), _lib.ptr(feats), _lib.stream_ptr(luma)), "resr_niqe_features")
    if not keep:
        return feats
    n_half = b * (h // 2) * (w // 2)
    return feats, ws[:n_half].view(b, h // 2, w // 2), ws[need // 8 - 2 * b * nblk * 30:].view(2, b, nblk, 5, 6)


def niqe_score_native(feats: torch.Tensor, mu_prior: torch.Tensor, cov_prior: torch.Tensor, keep: bool = False):
    """`_score_from_features` as resr_niqe_score on the current stream: feats float64 [B, blocks, 36] on the device -> scores [B],
    squeezed as `_score_from_features` squeezes them.  Two launches for the whole batch, no host synchronisation.  The priors are
    float64 [36] and [36, 36]; tensors already on feats' device in float64 are used as they are.
    keep=True also returns the workspace's contents as views: (scores, mu_d [B,36], A [B,36,36], eigenvalues [B,36], kept count [B])."""
    from . import _lib
    import ctypes as C
    if not isinstance(feats, torch.Tensor) or not feats.is_cuda:
        raise ValueError(f"niqe_score_native: the features must be a tensor on the device, got {getattr(feats, 'device', type(feats))}")
    if feats.dtype != torch.float64 or feats.dim() != 3 or feats.shape[2] != 36 or feats.shape[0] < 1 or feats.shape[1] < 1:
        raise ValueError(f"niqe_score_native: the features must be float64 [B, blocks, 36], got {feats.dtype} {tuple(feats.shape)}")
    if mu_prior.numel() != 36 or tuple(cov_prior.shape) != (36, 36):
        raise ValueError(f"niqe_score_native: the priors must be [36] and [36, 36], got {tuple(mu_prior.shape)} and {tuple(cov_prior.shape)}")
    feats = feats.contiguous()
    mu = mu_prior.to(device=feats.device, dtype=torch.float64).reshape(36).contiguous()
    cov = cov_prior.to(device=feats.device, dtype=torch.float64).contiguous()
    b, blocks, _ = feats.shape
    d = _lib.NiqeScoreDesc()
    d.n, d.blocks, d.mu_prior, d.cov_prior = b, blocks, mu.data_ptr(), cov.data_ptr()
    need = int(_lib.lib().resr_niqe_score_workspace_bytes(d))
    if not need:
        raise ValueError(f"native NIQE: {_lib.lib().resr_last_error().decode()}")
    ws = torch.empty(need // 8, dtype=torch.float64, device=feats.device)
    d.workspace, d.workspace_bytes = ws.data_ptr(), need
    scores = torch.empty(b, dtype=torch.float64, device=feats.device)
    _lib.check(_lib.lib().resr_niqe_score(C.byref(d), _lib.ptr(feats), _lib.ptr(scores), _lib.stream_ptr(feats)), "resr_niqe_score")
    if not keep:
        return scores.squeeze()
    o = (0, 36 * b, (36 + 1296) * b, (36 + 1296 + 36) * b)
    return scores.squeeze(), ws[o[0]:o[1]].view(b, 36), ws[o[1]:o[2]].view(b, 36, 36), ws[o[2]:o[3]].view(b, 36), ws[o[3]:]


TAILS = ("torch", "native")


def niqe_native(tensor: torch.Tensor, crop_border: int, mu_prior: torch.Tensor, cov_prior: torch.Tensor,
                bh: int = 96, bw: int = 96, tail: str = "torch") -> torch.Tensor:
    """`niqe` with the features computed by the kernels of csrc/niqe.hip: a float [B,3,H,W] batch in [0,1], or a uint8 [B,H,W,3]
    batch scored without a float image ever existing.  Everything is enqueued on the current stream; the tail is `niqe`'s
    (`_score_from_features`, tail="torch") or `niqe_score_native` (tail="native": two launches for the batch, no host round trip).
    The luma is the kernel's stated fp32 order (include/resr.h), which may differ from the
    torch path's matmul at a pixel whose luma lies within an fp32 rounding of a half ("Native NIQE")."""
    if tail not in TAILS:
        raise ValueError(f"niqe_native: tail must be 'torch' or 'native', got {tail!r}")
    check_native_blocks(bh, bw)
    if isinstance(crop_border, bool) or not isinstance(crop_border, int) or crop_border < 0:
        raise ValueError(f"niqe_native: crop_border must be a non-negative int, got {crop_border!r}")
    if tensor.dim() != 4:
        raise ValueError(f"niqe_native: expected a 4-D batch, got {tuple(tensor.shape)}")
    h, w = (tensor.shape[1:3] if tensor.dtype == torch.uint8 else tensor.shape[2:])
    nbh, nbw = (h - 2 * crop_border) // bh, (w - 2 * crop_border) // bw
    if nbh <= 0 or nbw <= 0:
        raise ValueError(f"NIQE needs at least one {bh}x{bw} block, got {h - 2 * crop_border}x{w - 2 * crop_border}")
    luma = niqe_luma_native(tensor, crop_border, nbh * bh, nbw * bw)
    feats = niqe_features_native(luma, bh, bw)
    if tail == "native":
        return niqe_score_native(feats, mu_prior, cov_prior)
    return _score_from_features(feats, mu_prior, cov_prior)


class NativeNIQE(NIQE):
    """`NIQE` on the native backend: same constructor and call; also takes uint8 [B,H,W,3] frames.  Block sizes the kernels refuse
    are a ValueError here, at construction.  tail="native" scores through `niqe_score_native`; its priors are made once per device and
    input precision and kept."""

    def __init__(self, crop_border: int, niqe_model_path: str, block_size_height: int = 96, block_size_width: int = 96,
                 tail: str = "torch") -> None:
        if tail not in TAILS:
            raise ValueError(f"NativeNIQE: tail must be 'torch' or 'native', got {tail!r}")
        check_native_blocks(block_size_height, block_size_width)
        super().__init__(crop_border, niqe_model_path, block_size_height, block_size_width)
        self.tail = tail
        self._tail_priors: dict = {}

    def forward(self, raw_tensor: torch.Tensor) -> torch.Tensor:
        as_float = raw_tensor.dtype if raw_tensor.is_floating_point() else torch.float32
        if self.tail == "native":
            key = (str(raw_tensor.device), as_float)
            priors = self._tail_priors.get(key)
            if priors is None:
                priors = self._tail_priors[key] = tuple(p.to(as_float).to(device=raw_tensor.device, dtype=torch.float64).contiguous()
                                                        for p in (self.mu_prisparam, self.cov_prisparam))
            return niqe_native(raw_tensor, self.crop_border, priors[0], priors[1], self.block_size_height, self.block_size_width, tail="native")
        mu = self.mu_prisparam.to(as_float).to(torch.float64)
        cov = self.cov_prisparam.to(as_float).to(torch.float64)
        return niqe_native(raw_tensor, self.crop_border, mu, cov, self.block_size_height, self.block_size_width)


# ---- full-reference metrics: PSNR and SSIM of the Y channel ------------------------------------------------------------------------
FULL_REF_WINDOW = 11       # the SSIM window: 11 taps, sigma 1.5 (Wang et al.; MATLAB / BasicSR on the Y channel)
FULL_REF_SIGMA = 1.5
FULL_REF_C1, FULL_REF_C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2      # 6.5025, 58.5225
FULL_REF_BACKENDS = ("off", "torch", "native")


def _full_ref_kind(t, name: str, who: str) -> str:
    """"u8" for a uint8 [B,H,W,3] tensor, "float" for a floating [B,3,H,W] one; ValueError for anything else."""
    if not isinstance(t, torch.Tensor) or t.dim() != 4:
        raise ValueError(f"{who}: {name} must be a float [B,3,H,W] or a uint8 [B,H,W,3] tensor, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
    if t.dtype == torch.uint8 and t.shape[3] == 3:
        return "u8"
    if t.is_floating_point() and t.shape[1] == 3:
        return "float"
    raise ValueError(f"{who}: {name} must be a float [B,3,H,W] or a uint8 [B,H,W,3] tensor, got {t.dtype} {tuple(t.shape)}")


def _full_ref_check(sr, hr, crop_border, who: str):
    """The checks every full-reference entry makes before any device work -> (kind of sr, kind of hr, B, H, W)."""
    kinds = _full_ref_kind(sr, "sr", who), _full_ref_kind(hr, "hr", who)
    if isinstance(crop_border, bool) or not isinstance(crop_border, int) or crop_border < 0:
        raise ValueError(f"{who}: crop_border must be a non-negative int, got {crop_border!r}")
    sizes = [(t.shape[0],) + (tuple(t.shape[1:3]) if k == "u8" else tuple(t.shape[2:])) for t, k in zip((sr, hr), kinds)]
    if sizes[0] != sizes[1]:
        raise ValueError(f"{who}: sr is {sizes[0][0]} images of {sizes[0][1]}x{sizes[0][2]}, hr {sizes[1][0]} of {sizes[1][1]}x{sizes[1][2]}: the shapes must match")
    if sr.device != hr.device:
        raise ValueError(f"{who}: sr is on {sr.device}, hr on {hr.device}: both must be on one device")
    b, h, w = sizes[0]
    if b < 1 or h - 2 * crop_border < FULL_REF_WINDOW or w - 2 * crop_border < FULL_REF_WINDOW:
        raise ValueError(f"{who}: a crop of {crop_border} leaves {h - 2 * crop_border}x{w - 2 * crop_border} of {b} images of {h}x{w}; the window needs at least 11x11")
    return kinds[0], kinds[1], b, h, w


def _y_levels(t: torch.Tensor, kind: str, crop_border: int) -> torch.Tensor:
    """The luma levels float64 [B,1,h,w] of the cropped batch: the luma as `niqe()` takes it, rounded to levels.  A uint8 frame enters
    as (float)byte / 255.0f."""
    if kind == "u8":
        # (a tensor divisor: a Python scalar may be turned into a multiplication by its reciprocal, which is not that division)
        t = (t.to(torch.float32) / torch.full((), 255.0, dtype=torch.float32, device=t.device)).permute(0, 3, 1, 2)
    if crop_border > 0:
        t = t[:, :, crop_border:-crop_border, crop_border:-crop_border]
    return (imgproc.rgb2ycbcr_torch(t.float(), only_use_y_channel=True) * 255.0).round().clamp(0, 255).to(torch.float64)


def _ssim_window(like: torch.Tensor) -> torch.Tensor:
    k = torch.exp(-(torch.arange(FULL_REF_WINDOW, dtype=torch.float64) - FULL_REF_WINDOW // 2) ** 2 / (2 * FULL_REF_SIGMA ** 2))
    k = k / k.sum()
    return torch.outer(k, k).to(like).view(1, 1, FULL_REF_WINDOW, FULL_REF_WINDOW)


def _psnr_of_levels(x: torch.Tensor, y: torch.Tensor, peak2: float = 65025.0) -> torch.Tensor:
    mse = ((x - y) ** 2).sum(dim=(1, 2, 3)) / (x.shape[2] * x.shape[3])     # integers below 2^53: the sum is exact
    return 10.0 * torch.log10(peak2 / (mse + 1e-8))


def _ssim_of_levels(x: torch.Tensor, y: torch.Tensor, c1: float = FULL_REF_C1, c2: float = FULL_REF_C2) -> torch.Tensor:
    g = _ssim_window(x)
    mu1, mu2 = F.conv2d(x, g), F.conv2d(y, g)
    m11, m22, m12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s11, s22, s12 = F.conv2d(x * x, g) - m11, F.conv2d(y * y, g) - m22, F.conv2d(x * y, g) - m12
    value = ((2 * m12 + c1) * (2 * s12 + c2)) / (((m11 + m22) + c1) * ((s11 + s22) + c2))
    return value.mean(dim=(1, 2, 3))


def psnr(sr: torch.Tensor, hr: torch.Tensor, crop_border: int) -> torch.Tensor:
    """PSNR [B] (float64) of the Y levels of sr against hr, each float [B,3,H,W] in [0,1] or uint8 [B,H,W,3]:
    10 log10(65025 / (mean (X - Y)^2 + 1e-8)) over the image without `crop_border` pixels on every side."""
    ks, kh, *_ = _full_ref_check(sr, hr, crop_border, "psnr")
    return _psnr_of_levels(_y_levels(sr, ks, crop_border), _y_levels(hr, kh, crop_border))


def ssim(sr: torch.Tensor, hr: torch.Tensor, crop_border: int) -> torch.Tensor:
    """SSIM [B] (float64) of the Y levels of sr against hr: the mean of the 11 x 11 / sigma 1.5 Gaussian-window map, valid
    convolution, C1 = 6.5025, C2 = 58.5225 (the MATLAB / BasicSR form)."""
    ks, kh, *_ = _full_ref_check(sr, hr, crop_border, "ssim")
    return _ssim_of_levels(_y_levels(sr, ks, crop_border), _y_levels(hr, kh, crop_border))


class PSNR(nn.Module):
    def __init__(self, crop_border: int) -> None:
        super().__init__()
        self.crop_border = crop_border

    def forward(self, sr: torch.Tensor, hr: torch.Tensor) -> torch.Tensor:
        return psnr(sr, hr, self.crop_border)


class SSIM(nn.Module):
    def __init__(self, crop_border: int) -> None:
        super().__init__()
        self.crop_border = crop_border

    def forward(self, sr: torch.Tensor, hr: torch.Tensor) -> torch.Tensor:
        return ssim(sr, hr, self.crop_border)


class TorchFullRef(nn.Module):
    """`forward(sr, hr) -> (psnr [B], ssim [B])` on the torch backend: one luma of each image for both metrics."""

    def __init__(self, crop_border: int) -> None:
        super().__init__()
        self.crop_border = crop_border

    def forward(self, sr: torch.Tensor, hr: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        ks, kh, *_ = _full_ref_check(sr, hr, self.crop_border, "full_ref")
        x, y = _y_levels(sr, ks, self.crop_border), _y_levels(hr, kh, self.crop_border)
        return _psnr_of_levels(x, y), _ssim_of_levels(x, y)


def full_ref_tiles(h: int, w: int) -> Tuple[int, int]:
    """Tile rows and columns of the SSIM map of a cropped h x w image (include/resr.h, resr_fullref)."""
    from . import _lib
    t = _lib.RESR_FULLREF_TILE
    return -(-(h - FULL_REF_WINDOW + 1) // t), -(-(w - FULL_REF_WINDOW + 1) // t)


def full_ref_native(sr: torch.Tensor, hr: torch.Tensor, crop_border: int, keep: bool = False):
    """(psnr [B], ssim [B]) in float64 by resr_fullref on the current stream: two launches for the batch, no host round trip.  sr and
    hr are each float [B,3,H,W] in [0,1] or uint8 [B,H,W,3].  The luma is the native NIQE's (one stated fp32 order).  There is no
    fallback onto torch: tensors that are not on the device are an error.
    keep=True also returns sse int64 [B] and the per-tile partials as views of the workspace: (psnr, ssim, sse, tile sse int64
    [B, tiles_y, tiles_x], tile map sums float64 [B, tiles_y, tiles_x])."""
    from . import _lib
    import ctypes as C
    ks, kh, b, h, w = _full_ref_check(sr, hr, crop_border, "full_ref_native")
    _lib.require_cuda(sr, "full_ref_native")
    sr = (sr if ks == "u8" else sr.float()).contiguous()
    hr = (hr if kh == "u8" else hr.float()).contiguous()
    d = _lib.FullRefDesc()
    d.n, d.h, d.w, d.crop, d.sr_u8, d.hr_u8 = b, h, w, crop_border, ks == "u8", kh == "u8"
    need = int(_lib.lib().resr_fullref_workspace_bytes(d))
    if not need:
        raise ValueError(f"full_ref_native: {_lib.lib().resr_last_error().decode()}")
    ws = torch.empty(need // 8, dtype=torch.int64, device=sr.device)
    d.workspace, d.workspace_bytes = ws.data_ptr(), need
    sse = torch.empty(b, dtype=torch.int64, device=sr.device)
    out = torch.empty((2, b), dtype=torch.float64, device=sr.device)
    _lib.check(_lib.lib().resr_fullref(C.byref(d), _lib.ptr(sr), _lib.ptr(hr), _lib.ptr(sse), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.stream_ptr(sr)),
               "resr_fullref")
    if not keep:
        return out[0], out[1]
    ty, tx = full_ref_tiles(h - 2 * crop_border, w - 2 * crop_border)
    parts = ws.view(b, ty, tx, 2)
    return out[0], out[1], sse, parts[..., 0], parts.view(torch.float64)[..., 1]


class NativeFullRef(nn.Module):
    """`forward(sr, hr) -> (psnr [B], ssim [B])` through `full_ref_native`: both metrics in one pass over the two images."""

    def __init__(self, crop_border: int) -> None:
        super().__init__()
        if isinstance(crop_border, bool) or not isinstance(crop_border, int) or crop_border < 0:
            raise ValueError(f"NativeFullRef: crop_border must be a non-negative int, got {crop_border!r}")
        self.crop_border = crop_border

    def forward(self, sr: torch.Tensor, hr: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return full_ref_native(sr, hr, self.crop_border)


# ---- full-reference metrics per plane: RGB channels, 16-bit images, the planes of YUV 4:2:0 frames ---------------------------------
# ("Native PSNR / SSIM per plane"; include/resr.h, resr_fullref_planes, is the specification.)
FULL_REF_PEAKS = (255, 1023, 65535)
FULL_REF_CHANNELS = ("y", "rgb")


class PlaneView(NamedTuple):
    """How the levels of `planes` planes of h x w lie in a flat tensor of 1-, 2- or 4-byte words (include/resr.h, resr_fullref_planes):
    word(i, p, y, x) = flat[base + i * image_stride + p * plane_stride + y * row_stride + x * pixel_stride]; an integer word gives the
    level (word >> shift) & mask, an fp32 word trunc(clamp(v * peak, 0, peak))."""
    word_bytes: int
    shift: int
    mask: int
    base: int
    pixel_stride: int
    row_stride: int
    plane_stride: int
    image_stride: int


class FullRefChannels(NamedTuple):
    """Per-channel sse int64, psnr, ssim float64 [B,C]; psnr_all [B] from the summed sse over C * hc * wc samples (BasicSR's RGB PSNR),
    ssim_mean [B] the channel mean (BasicSR's RGB SSIM)."""
    sse: torch.Tensor
    psnr: torch.Tensor
    ssim: torch.Tensor
    psnr_all: torch.Tensor
    ssim_mean: torch.Tensor


class FullRefYuv(NamedTuple):
    """PSNR and SSIM [N] float64 of the Y, Cb and Cr planes as stored; psnr_avg over all 1.5 H W samples (ffmpeg's "average")."""
    psnr_y: torch.Tensor
    psnr_u: torch.Tensor
    psnr_v: torch.Tensor
    psnr_avg: torch.Tensor
    ssim_y: torch.Tensor
    ssim_u: torch.Tensor
    ssim_v: torch.Tensor


def full_ref_constants(peak: int) -> Tuple[float, float]:
    """(C1, C2) of the SSIM map at `peak`: one float64 division of exact integers each (6.5025, 58.5225 at 255)."""
    return (peak * peak) / 10000.0, (9 * peak * peak) / 10000.0


_WORD_DTYPES = {torch.uint8: 1, torch.uint16: 2, torch.float32: 4}


def image_plane_view(t, name: str, who: str):
    """(view, B, C, H, W, peak or None) of one side of `full_ref_channels*`: a uint8 / uint16 [B,H,W,C] image batch, C in {1, 3, 4}
    (peak 255 / 65535), or a float [B,C,H,W] batch, C in {1, 3} (peak None: the other side's).  ValueError for anything else."""
    what = f"{who}: {name} must be a float [B,C,H,W] tensor, C 1 or 3, or a uint8 / uint16 [B,H,W,C] tensor, C 1, 3 or 4"
    if not isinstance(t, torch.Tensor) or t.dim() != 4:
        raise ValueError(f"{what}, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
    if t.dtype in (torch.uint8, torch.uint16) and t.shape[3] in (1, 3, 4):
        b, h, w, c = t.shape
        return PlaneView(t.element_size(), 0, 255 if t.dtype == torch.uint8 else 65535, 0, c, w * c, 1, h * w * c), b, c, h, w, 255 if t.dtype == torch.uint8 else 65535
    if t.is_floating_point() and t.shape[1] in (1, 3):
        b, c, h, w = t.shape
        return PlaneView(4, 0, 0, 0, 1, w, h * w, c * h * w), b, c, h, w, None
    raise ValueError(f"{what}, got {t.dtype} {tuple(t.shape)}")


def yuv_plane_views(pix_fmt: str, h: int, w: int):
    """(luma view, chroma view, peak) of a 4:2:0 frame [N,3h/2,w] in one of the YUV names of `frames.PIXEL_FORMATS`; the luma view has
    one h x w plane, the chroma view the two (Cb, Cr) h/2 x w/2 planes."""
    from .frames import PIXEL_FORMATS
    f = PIXEL_FORMATS.get(pix_fmt) if isinstance(pix_fmt, str) else None
    if f is None or f.layout is None:
        raise ValueError(f"full_ref_yuv: pix_fmt must be one of {tuple(n for n, p in PIXEL_FORMATS.items() if p.layout is not None)}, got {pix_fmt!r}")
    if h < 2 or w < 2 or h % 2 or w % 2:
        raise ValueError(f"full_ref_yuv: a 4:2:0 frame needs an even height and width, got {h}x{w}")
    word, shift, frame = f.bits // 8 if f.bits == 8 else 2, (16 - f.bits if f.high_bits else 0), 3 * h * w // 2
    luma = PlaneView(word, shift, f.top, 0, 1, w, 0, frame)
    chroma = (PlaneView(word, shift, f.top, h * w, 2, w, 1, frame) if f.semi_planar
              else PlaneView(word, shift, f.top, h * w, 1, w // 2, h * w // 4, frame))
    return luma, chroma, f.top


def _check_crop(crop_border, who: str):
    if isinstance(crop_border, bool) or not isinstance(crop_border, int) or crop_border < 0:
        raise ValueError(f"{who}: crop_border must be a non-negative int, got {crop_border!r}")


def _channels_check(sr, hr, crop_border, who: str):
    """The checks of `full_ref_channels*` before any device work -> (sr view, hr view, B, C, H, W, peak)."""
    vs, *ss, ps = image_plane_view(sr, "sr", who)
    vh, *sh, ph = image_plane_view(hr, "hr", who)
    _check_crop(crop_border, who)
    if ss != sh:
        raise ValueError(f"{who}: sr is {ss[0]} images of {ss[1]} channels of {ss[2]}x{ss[3]}, hr {sh[0]} of {sh[1]} of {sh[2]}x{sh[3]}: the shapes must match")
    if ps is not None and ph is not None and ps != ph:
        raise ValueError(f"{who}: sr is {sr.dtype}, hr {hr.dtype}: two integer sides must have one depth")
    if sr.device != hr.device:
        raise ValueError(f"{who}: sr is on {sr.device}, hr on {hr.device}: both must be on one device")
    b, c, h, w = ss
    if b < 1 or h - 2 * crop_border < FULL_REF_WINDOW or w - 2 * crop_border < FULL_REF_WINDOW:
        raise ValueError(f"{who}: a crop of {crop_border} leaves {h - 2 * crop_border}x{w - 2 * crop_border} of {b} images of {h}x{w}; the window needs at least 11x11")
    return vs, vh, b, c, h, w, (ps or ph or 255)


def _yuv_check(frames, reference, pix_fmt, ref_pix_fmt, crop_border, who: str):
    """The checks of `full_ref_yuv*` -> (views of frames, views of the reference, N, H, W, peak)."""
    from .frames import PIXEL_FORMATS
    ref_pix_fmt = pix_fmt if ref_pix_fmt is None else ref_pix_fmt
    for t, name, fmt in ((frames, "frames", pix_fmt), (reference, "reference", ref_pix_fmt)):
        f = PIXEL_FORMATS.get(fmt) if isinstance(fmt, str) else None
        if f is None or f.layout is None:
            raise ValueError(f"{who}: pix_fmt must be one of {tuple(n for n, p in PIXEL_FORMATS.items() if p.layout is not None)}, got {fmt!r}")
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.dtype != f.torch_dtype or t.shape[1] % 3 or t.shape[2] % 2:
            raise ValueError(f"{who}: {name} must be a {f.torch_dtype} [N,3H/2,W] tensor of {fmt!r} frames, H and W even, got "
                             f"{(t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t)}")
    if PIXEL_FORMATS[pix_fmt].bits != PIXEL_FORMATS[ref_pix_fmt].bits:
        raise ValueError(f"{who}: {pix_fmt!r} frames have {PIXEL_FORMATS[pix_fmt].bits} bits, the {ref_pix_fmt!r} reference {PIXEL_FORMATS[ref_pix_fmt].bits}: both sides must have one depth")
    _check_crop(crop_border, who)
    if crop_border % 2:
        raise ValueError(f"{who}: crop_border must be even (the chroma planes are cropped by half of it), got {crop_border}")
    if frames.shape != reference.shape:
        raise ValueError(f"{who}: frames are {tuple(frames.shape)}, the reference {tuple(reference.shape)}: the shapes must match")
    if frames.device != reference.device:
        raise ValueError(f"{who}: frames are on {frames.device}, the reference on {reference.device}: both must be on one device")
    n, h, w = frames.shape[0], frames.shape[1] // 3 * 2, frames.shape[2]
    if n < 1 or h // 2 - crop_border < FULL_REF_WINDOW or w // 2 - crop_border < FULL_REF_WINDOW:
        raise ValueError(f"{who}: a crop of {crop_border} leaves {h // 2 - crop_border}x{w // 2 - crop_border} of the {h // 2}x{w // 2} chroma planes; the window needs at least 11x11")
    fl, fc, peak = yuv_plane_views(pix_fmt, h, w)
    rl, rc, _ = yuv_plane_views(ref_pix_fmt, h, w)
    return (fl, fc), (rl, rc), n, h, w, peak


def _psnr_from_sse(sse: torch.Tensor, samples: int, peak: int) -> torch.Tensor:
    """10 log10(peak^2 / (sse / samples + 1e-8)) in float64 on sse's device (sse: exact integers below 2^53)."""
    return 10.0 * torch.log10(float(peak * peak) / (sse.to(torch.float64) / float(samples) + 1e-8))


def _channels_result(sse, psnr, ssim, samples: int, peak: int) -> FullRefChannels:
    """The [B,C] results plus psnr_all and ssim_mean (channels added in ascending order), all on the device, no host sync."""
    c = sse.shape[1]
    total = ssim[:, 0]
    for i in range(1, c):
        total = total + ssim[:, i]
    return FullRefChannels(sse, psnr, ssim, _psnr_from_sse(sse.sum(dim=1), c * samples, peak), total / float(c))


def _yuv_result(sse_y, psnr_y, ssim_y, sse_c, psnr_c, ssim_c, hc: int, wc: int, peak: int) -> FullRefYuv:
    total = sse_y[:, 0] + sse_c[:, 0] + sse_c[:, 1]
    return FullRefYuv(psnr_y[:, 0], psnr_c[:, 0], psnr_c[:, 1], _psnr_from_sse(total, hc * wc + 2 * (hc // 2) * (wc // 2), peak), ssim_y[:, 0], ssim_c[:, 0], ssim_c[:, 1])


def plane_levels(t: torch.Tensor, view: PlaneView, n: int, planes: int, h: int, w: int, peak: int) -> torch.Tensor:
    """The levels int64 [n,planes,h,w] a view names in the contiguous tensor `t`, in plain torch: the torch backend's loader."""
    flat = t.contiguous().reshape(-1)
    ax = lambda count, stride, shape: (torch.arange(count, device=t.device, dtype=torch.int64) * stride).view(shape)
    at = view.base + ax(n, view.image_stride, (n, 1, 1, 1)) + ax(planes, view.plane_stride, (1, planes, 1, 1)) + ax(h, view.row_stride, (1, 1, h, 1)) + ax(w, view.pixel_stride, (1, 1, 1, w))
    words = flat[at.reshape(-1)].view(n, planes, h, w)
    if view.word_bytes == 4:
        v = words.float() * torch.full((), float(peak), dtype=torch.float32, device=t.device)
        v = torch.where(v > 0, v, torch.zeros_like(v))                      # a NaN compares false: 0
        v = torch.where(v < float(peak), v, torch.full_like(v, float(peak)))
        return v.to(torch.int64)
    return (words.to(torch.int64) >> view.shift) & view.mask


def full_ref_planes(sr, sr_view: PlaneView, hr, hr_view: PlaneView, n: int, planes: int, h: int, w: int, crop: int, peak: int):
    """The torch float64 twin of `full_ref_planes_native`: (sse int64, psnr, ssim float64), each [n,planes]."""
    x, y = (plane_levels(t, v, n, planes, h, w, peak)[:, :, crop:h - crop, crop:w - crop].to(torch.float64).reshape(n * planes, 1, h - 2 * crop, w - 2 * crop)
            for t, v in ((sr, sr_view), (hr, hr_view)))
    c1, c2 = full_ref_constants(peak)
    sse = ((x - y) ** 2).sum(dim=(1, 2, 3)).to(torch.int64)
    return sse.view(n, planes), _psnr_of_levels(x, y, float(peak * peak)).view(n, planes), _ssim_of_levels(x, y, c1, c2).view(n, planes)


def full_ref_planes_native(sr, sr_view: PlaneView, hr, hr_view: PlaneView, n: int, planes: int, h: int, w: int, crop: int, peak: int, keep: bool = False):
    """resr_fullref_planes on the current stream: (sse int64, psnr, ssim float64), each [n,planes]; two launches, no host round trip.
    sr and hr are contiguous uint8 / uint16 / float32 device tensors whose words the views index; a view that names a word outside
    its tensor is refused here (the kernel trusts it).  keep=True adds the per-tile partials as views of the workspace: tile sse int64
    and tile map sums float64, each [n,planes,tiles_y,tiles_x]."""
    from . import _lib
    import ctypes as C
    d = _lib.FullRefPlanesDesc()
    d.n, d.planes, d.h, d.w, d.crop, d.peak = n, planes, h, w, crop, peak
    for side, t, v in (("sr", sr, sr_view), ("hr", hr, hr_view)):
        _lib.require_cuda(t, "full_ref_planes_native")
        if _WORD_DTYPES.get(t.dtype) != v.word_bytes or not t.is_contiguous():
            raise ValueError(f"full_ref_planes_native: {side} must be a contiguous tensor of {v.word_bytes}-byte words, got {t.dtype}")
        for field in PlaneView._fields:
            setattr(d, f"{side}_{field}", getattr(v, field))
    need = int(_lib.lib().resr_fullref_planes_workspace_bytes(d))
    if not need:
        raise ValueError(f"full_ref_planes_native: {_lib.lib().resr_last_error().decode()}")
    for side, t, v in (("sr", sr, sr_view), ("hr", hr, hr_view)):           # after the query: every stride is known non-negative
        last = v.base + (n - 1) * v.image_stride + (planes - 1) * v.plane_stride + (h - 1) * v.row_stride + (w - 1) * v.pixel_stride
        if last >= t.numel():
            raise ValueError(f"full_ref_planes_native: the {side} view reaches word {last} of a tensor of {t.numel()}")
    if sr.device != hr.device:
        raise ValueError(f"full_ref_planes_native: sr is on {sr.device}, hr on {hr.device}: both must be on one device")
    ws = torch.empty(need // 8, dtype=torch.int64, device=sr.device)
    d.workspace, d.workspace_bytes = ws.data_ptr(), need
    sse = torch.empty((n, planes), dtype=torch.int64, device=sr.device)
    out = torch.empty((2, n, planes), dtype=torch.float64, device=sr.device)
    _lib.check(_lib.lib().resr_fullref_planes(C.byref(d), _lib.ptr(sr), _lib.ptr(hr), _lib.ptr(sse), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.stream_ptr(sr)),
               "resr_fullref_planes")
    if not keep:
        return sse, out[0], out[1]
    ty, tx = full_ref_tiles(h - 2 * crop, w - 2 * crop)
    parts = ws.view(n, planes, ty, tx, 2)
    return sse, out[0], out[1], parts[..., 0], parts.view(torch.float64)[..., 1]


def _word_tensor(t: torch.Tensor) -> torch.Tensor:
    return (t if t.dtype in (torch.uint8, torch.uint16) else t.float()).contiguous()


def _full_ref_channels(planes_fn, who, sr, hr, crop_border, keep):
    vs, vh, b, c, h, w, peak = _channels_check(sr, hr, crop_border, who)
    got = planes_fn(_word_tensor(sr), vs, _word_tensor(hr), vh, b, c, h, w, crop_border, peak, **({"keep": True} if keep else {}))
    result = _channels_result(*got[:3], (h - 2 * crop_border) * (w - 2 * crop_border), peak)
    return (result,) + tuple(got[3:]) if keep else result


def full_ref_channels(sr: torch.Tensor, hr: torch.Tensor, crop_border: int) -> FullRefChannels:
    """PSNR / SSIM of every channel of sr against hr in torch float64 (the "torch" backend of RESR_FULL_REF_CHANNELS=rgb).  Each side
    is float [B,C,H,W] (quantised to the other side's depth; 8 bits when both are float) or uint8 / uint16 [B,H,W,C]."""
    return _full_ref_channels(full_ref_planes, "full_ref_channels", sr, hr, crop_border, False)


def full_ref_channels_native(sr: torch.Tensor, hr: torch.Tensor, crop_border: int, keep: bool = False):
    """`full_ref_channels` by resr_fullref_planes: one call, two launches for the batch and all channels, no host round trip and no
    fallback onto torch.  keep=True returns (result, tile sse int64 [B,C,tiles_y,tiles_x], tile map sums float64 of that shape)."""
    return _full_ref_channels(full_ref_planes_native, "full_ref_channels_native", sr, hr, crop_border, keep)


def _full_ref_yuv(planes_fn, who, frames, reference, pix_fmt, ref_pix_fmt, crop_border):
    (fl, fc), (rl, rc), n, h, w, peak = _yuv_check(frames, reference, pix_fmt, ref_pix_fmt, crop_border, who)
    frames, reference = frames.contiguous(), reference.contiguous()
    luma = planes_fn(frames, fl, reference, rl, n, 1, h, w, crop_border, peak)
    chroma = planes_fn(frames, fc, reference, rc, n, 2, h // 2, w // 2, crop_border // 2, peak)
    return _yuv_result(*luma[:3], *chroma[:3], h - 2 * crop_border, w - 2 * crop_border, peak)


def full_ref_yuv(frames: torch.Tensor, reference: torch.Tensor, pix_fmt: str, ref_pix_fmt=None, crop_border: int = 0) -> FullRefYuv:
    """PSNR / SSIM of the stored Y, Cb and Cr planes of 4:2:0 frames [N,3H/2,W] against a reference of the same size and depth, in
    torch float64.  pix_fmt / ref_pix_fmt (default: pix_fmt): "i420", "nv12", "i420p10" or "p010".  crop_border must be even."""
    return _full_ref_yuv(full_ref_planes, "full_ref_yuv", frames, reference, pix_fmt, ref_pix_fmt, crop_border)


def full_ref_yuv_native(frames: torch.Tensor, reference: torch.Tensor, pix_fmt: str, ref_pix_fmt=None, crop_border: int = 0) -> FullRefYuv:
    """`full_ref_yuv` by two resr_fullref_planes calls, luma and chroma, on the frames where they lie: no conversion to RGB."""
    return _full_ref_yuv(full_ref_planes_native, "full_ref_yuv_native", frames, reference, pix_fmt, ref_pix_fmt, crop_border)


class TorchFullRefChannels(nn.Module):
    """`forward(sr, hr) -> (psnr_all [B], ssim_mean [B])` of the RGB channels on the torch backend (RESR_FULL_REF_CHANNELS=rgb)."""
    score = staticmethod(full_ref_channels)

    def __init__(self, crop_border: int) -> None:
        super().__init__()
        _check_crop(crop_border, type(self).__name__)
        self.crop_border = crop_border

    def forward(self, sr: torch.Tensor, hr: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        r = self.score(sr, hr, self.crop_border)
        return r.psnr_all, r.ssim_mean


class NativeFullRefChannels(TorchFullRefChannels):
    """The same through `full_ref_channels_native`."""
    score = staticmethod(full_ref_channels_native)
