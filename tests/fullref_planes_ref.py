"""numpy restatement of the native PSNR / SSIM per plane (csrc/fullref.hip; include/resr.h, resr_fullref_planes, is the specification)
with the error bound its tests hold the kernel and the torch twins to.  No GPU, no library.

Definition.  A plane is an h x w array of integer levels 0 .. peak, peak one of 255, 1023, 65535.  For planes X (sr), Y (hr):
SSE = sum (X - Y)^2 in int64, exact; psnr = 10 log10(peak^2 / (SSE / (h w) + 1e-8)) in float64; SSIM is tests/fullref_ref.py's, term for
term, with C1 = (peak peak) / 10000.0 and C2 = (9 peak peak) / 10000.0, each ONE float64 division of exact integers (at 255 the bits of
6.5025 and 58.5225; (0.01 peak)^2 is not).  At peak 255 every function here returns what its namesake of fullref_ref returns.

Bound: fullref_ref's derivation, unchanged -- it is relative to the window sums, so only C1 and C2 (which enter A1, A2, B1, B2) differ.

A level comes out of a VIEW of the caller's words (`View`; strides and base in words): integer words give (word >> shift) & mask, fp32
words trunc(clamp(v * peak, 0, peak)) in fp32 with NaN -> 0.  `gather` is that sentence in numpy.
"""
from collections import namedtuple

import numpy as np

from tests import fullref_ref as F

PEAKS = (255, 1023, 65535)
View = namedtuple("View", "word_bytes shift mask base pixel_stride row_stride plane_stride image_stride")


def constants(peak):
    return (peak * peak) / 10000.0, (9 * peak * peak) / 10000.0


def quantise(v, peak):
    """fp32 values -> levels int64: trunc(clamp(v * peak, 0, peak)) in fp32, NaN -> 0."""
    with np.errstate(invalid="ignore"):
        t = np.asarray(v, np.float32) * np.float32(peak)
        t = np.where(t > 0, t, np.float32(0))
        t = np.where(t < np.float32(peak), t, np.float32(peak))
    return t.astype(np.int64)


def gather(words, view, n, planes, h, w, peak):
    """The levels int64 [n,planes,h,w] `view` names in the flat array `words` (uint8, uint16 or float32)."""
    words = np.ascontiguousarray(words).reshape(-1)
    assert words.dtype.itemsize == view.word_bytes
    out = np.empty((n, planes, h, w), np.int64)
    for i in range(n):
        for p in range(planes):
            for y in range(h):
                at = view.base + i * view.image_stride + p * view.plane_stride + y * view.row_stride
                row = words[at:at + (w - 1) * view.pixel_stride + 1:view.pixel_stride]
                out[i, p, y] = quantise(row, peak) if view.word_bytes == 4 else (row.astype(np.int64) >> view.shift) & view.mask
    return out


def sse_np(X, Y):
    return F.sse_np(X, Y)


def psnr_np(sse, pixels, peak):
    return 10.0 * np.log10(float(peak * peak) / (np.asarray(sse, dtype=np.float64) / float(pixels) + 1e-8))


def ssim_map_np(X, Y, peak, real=F.REAL):
    """X, Y integer [B,h,w] -> (map [B,h-10,w-10] in `real`, bound float64): fullref_ref.ssim_map_np with the constants of `peak`."""
    c1, c2 = constants(peak)
    k = F.window_1d().astype(real)
    g = np.outer(k, k)
    x, y = X.astype(real), Y.astype(real)
    mu1, mu2 = F._window_sums(x, g), F._window_sums(y, g)
    exx, eyy, exy = F._window_sums(x * x, g), F._window_sums(y * y, g), F._window_sums(x * y, g)
    s11, s22, s12 = exx - mu1 * mu1, eyy - mu2 * mu2, exy - mu1 * mu2
    a1, a2 = 2 * mu1 * mu2 + real(c1), 2 * s12 + real(c2)
    b1, b2 = mu1 * mu1 + mu2 * mu2 + real(c1), s11 + s22 + real(c2)
    value = a1 * a2 / (b1 * b2)
    nu = F.N_TERMS * F.U
    f = lambda t: np.asarray(t, dtype=np.float64)
    mu1, mu2, exx, eyy, exy, a1, a2, b1, b2, v = map(f, (mu1, mu2, exx, eyy, exy, a1, a2, b1, b2, value))
    d_mu1, d_mu2 = nu * mu1, nu * mu2
    d_s11, d_s22 = nu * exx + 2 * mu1 * d_mu1, nu * eyy + 2 * mu2 * d_mu2
    d_s12 = nu * exy + mu1 * d_mu2 + mu2 * d_mu1
    d_a1, d_a2 = 2 * (mu1 * d_mu2 + mu2 * d_mu1), 2 * d_s12
    d_b1, d_b2 = 2 * (mu1 * d_mu1 + mu2 * d_mu2), d_s11 + d_s22
    bound = F.SLACK * ((d_a1 * np.abs(a2) + np.abs(a1) * d_a2) / (b1 * b2) + np.abs(v) * (d_b1 / b1 + d_b2 / b2))
    return value, bound


def reference(X, Y, peak, tile=None):
    """Everything the tests compare with, from the cropped levels X, Y integer [B,h,w] (B = images x planes): the dict of
    fullref_ref.reference -- sse [B] int64, psnr, ssim and ssim_gate [B], the map and its bound; with `tile`, also the per-tile sse,
    map sums and their gates [B,ty,tx]."""
    X, Y = np.asarray(X), np.asarray(Y)
    assert X.shape == Y.shape and X.ndim == 3 and peak in PEAKS and 0 <= min(X.min(), Y.min()) and max(X.max(), Y.max()) <= peak
    b, h, w = X.shape
    value, bound = ssim_map_np(X, Y, peak)
    sse = sse_np(X, Y)
    out = {"X": X, "Y": Y, "h": h, "w": w, "sse": sse, "psnr": psnr_np(sse, h * w, peak), "map": value, "bound": bound,
           "ssim": np.array([float(value[i].mean()) for i in range(b)]),
           "ssim_gate": np.array([F.sum_gate(np.asarray(value[i], np.float64), bound[i]) / value[i].size for i in range(b)])}
    if tile:
        (iy, ty), (ix, tx) = F.tile_index(h - F.WINDOW + 1, tile), F.tile_index(w - F.WINDOW + 1, tile)
        d = (X.astype(np.int64) - Y.astype(np.int64)) ** 2
        out["tile_sse"] = np.zeros((b, ty, tx), np.int64)
        out["tile_sum"] = np.zeros((b, ty, tx))
        out["tile_gate"] = np.zeros((b, ty, tx))
        for i in range(ty):
            for j in range(tx):
                out["tile_sse"][:, i, j] = d[:, iy == i][:, :, ix == j].sum(axis=(1, 2))
                v = value[:, i * tile:(i + 1) * tile, j * tile:(j + 1) * tile]
                e = bound[:, i * tile:(i + 1) * tile, j * tile:(j + 1) * tile]
                for k in range(b):
                    out["tile_sum"][k, i, j] = float(v[k].sum())
                    out["tile_gate"][k, i, j] = F.sum_gate(np.asarray(v[k], np.float64), e[k])
    return out


def crop(levels, c):
    """[..., h, w] -> [..., h - 2c, w - 2c]."""
    return levels[..., c:levels.shape[-2] - c, c:levels.shape[-1] - c]


def channels_summary(ref, b, c, peak):
    """(psnr_all [b], ssim_mean [b], its gate [b]) from a `reference` over b * c planes: the PSNR of the summed sse over c h w samples,
    the channel mean of the ssim added in ascending order (gate: the mean of the channels' gates plus the c additions' roundings)."""
    sse, ssim, gate = ref["sse"].reshape(b, c), ref["ssim"].reshape(b, c), ref["ssim_gate"].reshape(b, c)
    mean = np.zeros(b)
    for i in range(c):
        mean = mean + ssim[:, i]
    return psnr_np(sse.sum(axis=1), c * ref["h"] * ref["w"], peak), mean / c, gate.sum(axis=1) / c + F.SLACK * c * F.U * np.abs(ssim).sum(axis=1) / c


def yuv_planes(frame_words, view_luma, view_chroma, n, h, w, peak):
    """(Y [n,1,h,w], CbCr [n,2,h/2,w/2]) levels of 4:2:0 frames through their two views."""
    return gather(frame_words, view_luma, n, 1, h, w, peak), gather(frame_words, view_chroma, n, 2, h // 2, w // 2, peak)
