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
[B,H,W,3] tensors on either side.  Not built: RGB-channel scoring, MS-SSIM, padding modes, windows other than 11 taps / sigma 1.5.
"""
from __future__ import annotations

import math
from typing import List, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import imgproc

__all__ = ["NIQE", "niqe", "NativeNIQE", "niqe_native", "niqe_score_native",
           "PSNR", "SSIM", "psnr", "ssim", "NativeFullRef", "full_ref_native"]


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


def _psnr_of_levels(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    mse = ((x - y) ** 2).sum(dim=(1, 2, 3)) / (x.shape[2] * x.shape[3])     # integers below 2^53: the sum is exact
    return 10.0 * torch.log10(65025.0 / (mse + 1e-8))


def _ssim_of_levels(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    g = _ssim_window(x)
    mu1, mu2 = F.conv2d(x, g), F.conv2d(y, g)
    m11, m22, m12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s11, s22, s12 = F.conv2d(x * x, g) - m11, F.conv2d(y * y, g) - m22, F.conv2d(x * y, g) - m12
    value = ((2 * m12 + FULL_REF_C1) * (2 * s12 + FULL_REF_C2)) / (((m11 + m22) + FULL_REF_C1) * ((s11 + s22) + FULL_REF_C2))
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
