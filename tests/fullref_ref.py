"""numpy restatement of the native PSNR / SSIM (csrc/fullref.hip; include/resr.h, resr_fullref, is the specification) with the error
bound its tests hold the kernels and the torch backend to.  No GPU, no library.

Definition.  Levels X, Y uint8 [B,h,w] through tests/niqe_ref.niqe_luma_np.  SSE = sum (X - Y)^2 in int64, exact.
psnr = 10 log10(65025 / (SSE / (h w) + 1e-8)) in float64.  SSIM: k[i] = exp(-(i - 5)^2 / 4.5) / sum in float64, the window g = k k^T,
valid convolution; the map (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s11 + s22 + C2)) is evaluated here with the 2-D window
in np.longdouble (64-bit mantissa on x86), or, where the host's longdouble is no wider than float64, in float64 with twice the gate.

Bound (as tests/niqe_ref.py derives its own).  u = 2^-53.  A float64 sum of n non-negative terms lies within n u sum|t| of the exact
sum; n = 124: the 121 taps of a window sum, plus the roundings of the taps themselves (each k[i] a quotient of a rounded exponential,
each g[a][b] a product, or the value passing through two 11-tap passes).  Every window sum here has non-negative terms, so
    d_mu  = n u mu                                  for mu1 = g * x and mu2 = g * y
    d_s11 = n u E[x^2] + 2 mu1 d_mu1                (s11 = E[x^2] - mu1^2), d_s22 likewise, d_s12 = n u E[xy] + mu1 d_mu2 + mu2 d_mu1
and to first order through the quotient, with A1 = 2 mu1 mu2 + C1, A2 = 2 s12 + C2, B1 = mu1^2 + mu2^2 + C1, B2 = s11 + s22 + C2:
    d_map = (dA1 |A2| + |A1| dA2) / (B1 B2) + |map| (dB1 / B1 + dB2 / B2),
    dA1 = 2 (mu1 d_mu2 + mu2 d_mu1), dA2 = 2 d_s12, dB1 = 2 (mu1 d_mu1 + mu2 d_mu2), dB2 = d_s11 + d_s22
(the absolute form for the numerator: A2 may pass through zero), times SLACK = 4.  A sum of N map values is gated by the sum of their
bounds plus SLACK N u sum|value|; the mean by that over N.
"""
import numpy as np

from tests import niqe_ref

U = 2.0 ** -53
N_TERMS = 124
SLACK = 4.0
WINDOW, SIGMA = 11, 1.5
C1, C2 = 6.5025, 58.5225
WIDE = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
REAL = np.longdouble if WIDE else np.float64
GATE = 1.0 if WIDE else 2.0      # a float64 reference carries the error it is meant to judge: twice the gate


def window_1d():
    k = np.exp(-(np.arange(WINDOW, dtype=np.float64) - WINDOW // 2) ** 2 / (2 * SIGMA ** 2))
    return k / k.sum()


def levels(img, crop):
    """img: uint8 [B,H,W,3] or float32 [B,3,H,W] -> the luma levels uint8 [B,h,w] of the image without `crop` pixels on every side."""
    x = niqe_ref.unit_of_u8(img) if img.dtype == np.uint8 else np.ascontiguousarray(img, dtype=np.float32)
    h, w = x.shape[2] - 2 * crop, x.shape[3] - 2 * crop
    return niqe_ref.niqe_luma_np(x, crop, h, w)


def sse_np(X, Y):
    d = X.astype(np.int64) - Y.astype(np.int64)
    return (d * d).sum(axis=(1, 2))


def psnr_np(sse, pixels):
    return 10.0 * np.log10(65025.0 / (np.asarray(sse, dtype=np.float64) / float(pixels) + 1e-8))


def _window_sums(v, g):
    mh, mw = v.shape[1] - WINDOW + 1, v.shape[2] - WINDOW + 1
    acc = np.zeros((v.shape[0], mh, mw), dtype=g.dtype)
    for a in range(WINDOW):
        for b in range(WINDOW):
            acc += g[a, b] * v[:, a:a + mh, b:b + mw]
    return acc


def ssim_map_np(X, Y, real=REAL):
    """X, Y uint8 [B,h,w] -> (map [B,h-10,w-10] in `real`, bound float64 of the same shape: the distance a float64 evaluation in any
    order may lie from the exact map, SLACK included, the reference's GATE not)."""
    k = window_1d().astype(real)
    g = np.outer(k, k)
    x, y = X.astype(real), Y.astype(real)
    mu1, mu2 = _window_sums(x, g), _window_sums(y, g)
    exx, eyy, exy = _window_sums(x * x, g), _window_sums(y * y, g), _window_sums(x * y, g)
    s11, s22, s12 = exx - mu1 * mu1, eyy - mu2 * mu2, exy - mu1 * mu2
    a1, a2 = 2 * mu1 * mu2 + real(C1), 2 * s12 + real(C2)
    b1, b2 = mu1 * mu1 + mu2 * mu2 + real(C1), s11 + s22 + real(C2)
    value = a1 * a2 / (b1 * b2)
    nu = N_TERMS * U
    f = lambda t: np.asarray(t, dtype=np.float64)
    mu1, mu2, exx, eyy, exy, a1, a2, b1, b2, v = map(f, (mu1, mu2, exx, eyy, exy, a1, a2, b1, b2, value))
    d_mu1, d_mu2 = nu * mu1, nu * mu2
    d_s11, d_s22 = nu * exx + 2 * mu1 * d_mu1, nu * eyy + 2 * mu2 * d_mu2
    d_s12 = nu * exy + mu1 * d_mu2 + mu2 * d_mu1
    d_a1, d_a2 = 2 * (mu1 * d_mu2 + mu2 * d_mu1), 2 * d_s12
    d_b1, d_b2 = 2 * (mu1 * d_mu1 + mu2 * d_mu2), d_s11 + d_s22
    bound = SLACK * ((d_a1 * np.abs(a2) + np.abs(a1) * d_a2) / (b1 * b2) + np.abs(v) * (d_b1 / b1 + d_b2 / b2))
    return value, bound


def sum_gate(values, bounds):
    """The gate of a float64 sum of `values` (any order) against their exact sum: the values' own bounds plus the sum's roundings."""
    return GATE * (float(np.sum(bounds)) + SLACK * values.size * U * float(np.sum(np.abs(values))))


def tile_index(n, tile):
    """Pixel / map index -> tile index along an axis of n map values (n + 10 pixels): the last tile owns the extra 10."""
    tiles = -(-n // tile)
    return np.minimum(np.arange(n + WINDOW - 1) // tile, tiles - 1), tiles


def reference(sr, hr, crop, tile=None):
    """Everything the tests compare with, from the two images (uint8 [B,H,W,3] or float32 [B,3,H,W], independently): a dict with the
    levels, sse [B] int64, psnr [B], ssim [B] float64 and its gate [B], the map and its bound; with `tile`, also the per-tile sse
    [B,ty,tx] int64, map sums [B,ty,tx] float64 and their gates."""
    X, Y = levels(sr, crop), levels(hr, crop)
    b, h, w = X.shape
    value, bound = ssim_map_np(X, Y)
    sse = sse_np(X, Y)
    out = {"X": X, "Y": Y, "h": h, "w": w, "sse": sse, "psnr": psnr_np(sse, h * w), "map": value, "bound": bound,
           "ssim": np.array([float(value[i].mean()) for i in range(b)]),
           "ssim_gate": np.array([sum_gate(np.asarray(value[i], np.float64), bound[i]) / value[i].size for i in range(b)])}
    if tile:
        (iy, ty), (ix, tx) = tile_index(h - WINDOW + 1, tile), tile_index(w - WINDOW + 1, tile)
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
                    out["tile_gate"][k, i, j] = sum_gate(np.asarray(v[k], np.float64), e[k])
    return out


def pair(seed, b, h, w):
    """A test pair of uint8 [b,h,w,3] images: hr noise; sr of image 0 independent noise, of image 1 a near copy (hr +- 3 levels), of
    every further image hr itself."""
    rng = np.random.default_rng(seed)
    hr = rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)
    sr = hr.copy()
    sr[0] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if b > 1:
        sr[1] = np.clip(hr[1].astype(np.int64) + rng.integers(-3, 4, (h, w, 3)), 0, 255).astype(np.uint8)
    return sr, hr
