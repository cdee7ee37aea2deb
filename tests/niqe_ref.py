"""numpy / float64 restatement of every stage of the native NIQE (csrc/niqe.hip), with the error bounds its tests hold the kernels to,
and the repair of test images.  No GPU, no library: tests/test_niqe_native_surface.py checks these against the module's torch path on
the CPU, tests/test_gpu_niqe_kernels.py checks the kernels against these.

Bounds.  u = 2^-53.  A float64 sum of n terms t_k, in any order and with or without fused multiply-adds, lies within n u sum|t_k| of
the exact sum (to first order); two such sums lie within twice that of each other.  Every bound below is that expression, propagated
through the stage's formula to first order, times SLACK = 4 (the factor 2 between two computed sums, and 2 for the second-order terms and
the handful of single roundings that are not written out).
"""
import math

import numpy as np

U = 2.0 ** -53
SLACK = 4.0
TIE_MARGIN = 2e-4      # condition (a): every float64 luma at least this far from a half
SIGN_MARGIN = 1e-9     # condition (b): no MSCN value of the float64 reference smaller than this
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))   # torch.roll shifts of _block_features, after the block itself
_C = (np.float32(65.481), np.float32(128.553), np.float32(24.966))


# ---- luma --------------------------------------------------------------------------------------------------------------------------
def unit_of_u8(img_u8):
    """uint8 [B,H,W,3] -> float32 [B,3,H,W]: (float)byte / 255.0f, one IEEE division (yuv.h's unit_of)."""
    return np.ascontiguousarray((img_u8.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))


def niqe_luma_np(x, crop, out_h, out_w):
    """THE definition of the native luma: x float32 [B,3,H,W] -> uint8 levels [B,out_h,out_w] of the pixels from (crop, crop) on.
    Six fp32 operations, each rounded once, in this order; rint is half to even."""
    assert x.dtype == np.float32
    v = x[:, :, crop:crop + out_h, crop:crop + out_w]
    t = v[:, 0] * _C[0]
    t = t + v[:, 1] * _C[1]
    t = t + v[:, 2] * _C[2]
    t = t + np.float32(16.0)
    assert t.dtype == np.float32
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def luma_f64(x):
    """The exact value (float64: 24-bit constants times 24-bit inputs, four terms) of the sum the fp32 chain rounds: [B,H,W]."""
    v = x.astype(np.float64)
    return v[:, 0] * float(_C[0]) + v[:, 1] * float(_C[1]) + v[:, 2] * float(_C[2]) + 16.0


def tie_distance(x):
    """min over pixels of |frac(luma) - 1/2|."""
    y = luma_f64(x)
    return float(np.abs(y - np.floor(y) - 0.5).min())


def repair_ties(img_u8, margin=TIE_MARGIN):
    """Condition (a).  uint8 [B,H,W,3] -> a copy in which every pixel's float64 luma is at least `margin` from a half: a pixel that
    violates it is nudged by one level on one channel (the first of R+1, R-1, G+1, ... that cures it).  A four-operation fp32 chain
    on values up to 255 errs by less than 1e-4 (four half-ulps of 2^-17 at most), so every fp32 order then rounds alike."""
    out = img_u8.copy()
    y = luma_f64(unit_of_u8(out))
    bad = np.argwhere(np.abs(y - np.floor(y) - 0.5) < margin)
    for b, i, j in bad:
        for ch, step in ((0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1)):
            px = out[b, i, j].astype(np.int64)
            px[ch] += step
            if not 0 <= px[ch] <= 255:
                continue
            cand = px.astype(np.uint8).reshape(1, 1, 1, 3)
            if tie_distance(unit_of_u8(cand)) >= margin:
                out[b, i, j] = cand.reshape(3)
                break
        else:
            raise AssertionError(f"no one-level nudge cures the tie at {(b, i, j)}")
    assert tie_distance(unit_of_u8(out)) >= margin
    return out, len(bad)


# ---- half-size image ---------------------------------------------------------------------------------------------------------------
def half_np(y, mh, mw):
    """_resize_half(y / 255) * 255 for y float64 [B,h,w] with the dense matrices mh [h/2,h], mw [w/2,w]; and its bound."""
    v = y / 255.0
    ref = np.einsum("ih,bhw,jw->bij", mh, v, mw) * 255.0
    terms = int((mh != 0).sum(1).max() + (mw != 0).sum(1).max()) + 2
    bound = SLACK * terms * U * np.einsum("ih,bhw,jw->bij", np.abs(mh), np.abs(v), np.abs(mw)) * 255.0
    return ref, bound


def banded_apply(y, start_h, w_h, start_w, w_w):
    """The kernel's own summation: H pass, then W pass, k ascending, through the banded tables (numpy, no fma)."""
    v = y / 255.0
    ph, pw = w_h.shape[1], w_w.shape[1]
    t = np.zeros((y.shape[0], len(start_h), y.shape[2]))
    for k in range(ph):
        t += w_h[None, :, k, None] * v[:, start_h + k, :]
    o = np.zeros((y.shape[0], len(start_h), len(start_w)))
    for k in range(pw):
        o += t[:, :, start_w + k] * w_w[None, None, :, k]
    return o * 255.0


# ---- MSCN + block moments ----------------------------------------------------------------------------------------------------------
def mscn_np(y, win, y_err=0.0):
    """y float64 [B,h,w], win float64 [7,7] -> (mscn [B,h,w], err [B,h,w]): the locally normalised plane with replicate padding, and
    the first-order bound of the distance between two float64 evaluations of it whose inputs differ by at most y_err."""
    p = np.pad(y, ((0, 0), (3, 3), (3, 3)), mode="edge")
    h, w = y.shape[1:]
    mu = np.zeros_like(y)
    sq = np.zeros_like(y)
    amu = np.zeros_like(y)
    asq = np.zeros_like(y)
    for dy in range(7):
        for dx in range(7):
            v = p[:, dy:dy + h, dx:dx + w]
            mu += win[dy, dx] * v
            sq += win[dy, dx] * (v * v)
            amu += win[dy, dx] * np.abs(v)
            asq += win[dy, dx] * (v * v)
    var = sq - mu * mu
    sigma = np.sqrt(np.abs(var) + 1e-8)
    x = (y - mu) / (sigma + 1)
    ymax = np.abs(p).max()
    d_mu = 49 * U * amu + y_err
    d_sq = 50 * U * asq + 2 * ymax * y_err
    d_var = d_sq + 2 * np.abs(mu) * d_mu + 2 * U * (sq + mu * mu)
    d_sigma = d_var / (2 * sigma) + 2 * U * sigma          # sigma >= 1e-4: the 1e-8 under the root
    err = (d_mu + y_err + U * np.abs(y - mu)) / (sigma + 1) + np.abs(x) * (d_sigma / (sigma + 1) + 2 * U)
    return x, SLACK * err


def block_moments_np(x, err, bh, bw):
    """x, err [B,h,w] -> (moments [B,blocks,5,6], bound [B,blocks,5,6], min_abs): per block and map (the block, its products with the
    four rolled copies) the six words of the kernel -- negatives, positives, sum of squares over negatives / positives, sum of
    magnitudes, sum of squares -- with their bounds (0 for the counts: they are exact when no element can change sign, which min_abs,
    the smallest |element| minus its own error bound over all maps, shows), n u sum|term| + sum of the propagated element errors."""
    b, h, w = x.shape
    nbh, nbw = h // bh, w // bw
    blk = x.reshape(b, nbh, bh, nbw, bw).transpose(0, 1, 3, 2, 4).reshape(b, nbh * nbw, bh, bw)
    eblk = err.reshape(b, nbh, bh, nbw, bw).transpose(0, 1, 3, 2, 4).reshape(b, nbh * nbw, bh, bw)
    n = bh * bw
    out = np.zeros((b, nbh * nbw, 5, 6))
    bound = np.zeros_like(out)
    min_abs = math.inf
    for m in range(5):
        if m == 0:
            v, e = blk, eblk
        else:
            r = np.roll(blk, SHIFTS[m - 1], axis=(2, 3))
            er = np.roll(eblk, SHIFTS[m - 1], axis=(2, 3))
            v = blk * r
            e = np.abs(blk) * er + np.abs(r) * eblk + U * np.abs(v)
        min_abs = min(min_abs, float((np.abs(v) - e).min()))
        neg, pos = v < 0, v > 0
        s = v * v
        es = 2 * np.abs(v) * e + U * s
        out[:, :, m, 0] = neg.sum((2, 3))
        out[:, :, m, 1] = pos.sum((2, 3))
        out[:, :, m, 2] = (s * neg).sum((2, 3))
        out[:, :, m, 3] = (s * pos).sum((2, 3))
        out[:, :, m, 4] = np.abs(v).sum((2, 3))
        out[:, :, m, 5] = s.sum((2, 3))
        bound[:, :, m, 2] = SLACK * n * U * out[:, :, m, 2] + (es * neg).sum((2, 3))
        bound[:, :, m, 3] = SLACK * n * U * out[:, :, m, 3] + (es * pos).sum((2, 3))
        bound[:, :, m, 4] = SLACK * n * U * out[:, :, m, 4] + e.sum((2, 3))
        bound[:, :, m, 5] = SLACK * n * U * out[:, :, m, 5] + es.sum((2, 3))
    return out, bound, min_abs


# ---- AGGD fit ------------------------------------------------------------------------------------------------------------------------
_lgamma = np.vectorize(math.lgamma)


def aggd_np(mom, bound, n, grid, r_gam):
    """mom, bound [..., 6] of one map, n elements per block -> dict of alpha's grid index, the gap between the two best grid candidates,
    (bl, br, mean) and their bounds.  grid / r_gam: the module's tables as float64 numpy."""
    den_neg = np.where(mom[..., 0] > 0, mom[..., 0], float(np.float32(1e-8)))
    den_pos = np.where(mom[..., 1] > 0, mom[..., 1], float(np.float32(1e-8)))
    left, right = np.sqrt(mom[..., 2] / den_neg), np.sqrt(mom[..., 3] / den_pos)
    g = left / right
    rhat = (mom[..., 4] / n) ** 2 / (mom[..., 5] / n)
    rhat_norm = rhat * (g ** 3 + 1) * (g + 1) / (g ** 2 + 1) ** 2
    d = np.abs(r_gam[None, :] - rhat_norm.reshape(-1, 1))
    idx = d.argmin(1)
    two = np.partition(d, 1, axis=1)[:, :2]
    gap = (two[:, 1] - two[:, 0]).reshape(rhat_norm.shape)
    idx = idx.reshape(rhat_norm.shape)
    alpha = grid[idx]
    l1, l2, l3 = _lgamma(1 / alpha), _lgamma(2 / alpha), _lgamma(3 / alpha)
    scale = np.sqrt(np.exp(l1 - l3))
    ratio = np.exp(l2 - l1)
    bl, br = left * scale, right * scale
    # relative bounds: half the moment's (a square root), plus the special functions -- lgamma, exp and sqrt of either side are allowed
    # 16 u of their own value each, and an error dz of an exponent is a relative error dz of its exponential
    with np.errstate(divide="ignore", invalid="ignore"):
        rl = 0.5 * bound[..., 2] / mom[..., 2] + 8 * U
        rr = 0.5 * bound[..., 3] / mom[..., 3] + 8 * U
    r_scale = 0.5 * (16 * U * (np.abs(l1) + np.abs(l3) + 2)) + 16 * U
    r_ratio = 16 * U * (np.abs(l1) + np.abs(l2) + 2)
    e_bl, e_br = bl * (rl + r_scale), br * (rr + r_scale)
    mean = (br - bl) * ratio
    e_mean = (e_bl + e_br) * ratio + np.abs(mean) * (r_ratio + 4 * U)
    return {"idx": idx, "gap": gap, "alpha": alpha, "bl": bl, "br": br, "mean": mean, "e_bl": e_bl, "e_br": e_br, "e_mean": e_mean}


def features_np(mom, bound, n, grid, r_gam):
    """mom, bound [B,blocks,5,6] -> (feats [B,blocks,18], bound [B,blocks,18], idx [B,blocks,5], gap [B,blocks,5]) in the column order
    of _block_features; the alpha columns carry a bound of 0 (they are judged through idx and gap)."""
    f = np.zeros(mom.shape[:2] + (18,))
    e = np.zeros_like(f)
    idx = np.zeros(mom.shape[:2] + (5,), np.int64)
    gap = np.zeros(mom.shape[:2] + (5,))
    for m in range(5):
        a = aggd_np(mom[:, :, m], bound[:, :, m], n, grid, r_gam)
        idx[:, :, m], gap[:, :, m] = a["idx"], a["gap"]
        if m == 0:
            f[:, :, 0], f[:, :, 1] = a["alpha"], (a["bl"] + a["br"]) / 2
            e[:, :, 1] = (a["e_bl"] + a["e_br"]) / 2 + 2 * U * f[:, :, 1]
        else:
            c = 2 + 4 * (m - 1)
            f[:, :, c], f[:, :, c + 1], f[:, :, c + 2], f[:, :, c + 3] = a["alpha"], a["mean"], a["bl"], a["br"]
            e[:, :, c + 1], e[:, :, c + 2], e[:, :, c + 3] = a["e_mean"], a["e_bl"], a["e_br"]
    return f, e, idx, gap


ALPHA_COLUMNS = (0, 2, 6, 10, 14)


def reference(levels, bh, bw, win, mh, mw, grid, r_gam):
    """Every stage of the float64 reference from the luma levels uint8 [B,h,w]: a dict with the half-size image, the moments and the
    features of both scales, each with its bound, and min_abs of condition (b)."""
    y1 = levels.astype(np.float64)
    half, half_bound = half_np(y1, mh, mw)
    out = {"half": half, "half_bound": half_bound, "min_abs": math.inf}
    for s, (y, y_err) in enumerate(((y1, 0.0), (half, float(half_bound.max())))):
        x, err = mscn_np(y, win, y_err)
        out["min_abs"] = min(out["min_abs"], float(np.abs(x).min()))
        hb, wb = bh // (s + 1), bw // (s + 1)
        mom, mb, min_abs = block_moments_np(x, err, hb, wb)
        f, fe, idx, gap = features_np(mom, mb, hb * wb, grid, r_gam)
        out[f"s{s + 1}"] = {"mscn": x, "mom": mom, "mom_bound": mb, "signed_margin": min_abs, "feats": f, "feats_bound": fe, "idx": idx, "gap": gap}
    return out
