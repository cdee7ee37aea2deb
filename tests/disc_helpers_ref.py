"""Plain float64 references of the discriminator / VGG helper operations (csrc/disc.hip, the tail of csrc/loss.hip), CPU only.

Every function restates the operation from its DEFINITION (include/resr.h, torch's documentation), on numpy float64 arrays in the
library's layouts -- activations NHWC, weights OIHW -- and shares no index arithmetic with the kernels.  tests/test_disc_helpers_ref.py
checks these references against torch before tests/test_gpu_disc_helpers.py lets them judge a kernel.
"""
import numpy as np

LO_SCALE = 4096.0            # include/resr.h, RESR_F16X2: value = hi + lo * 2^-12
PAIR_REL = 2.0 ** -22        # round trip of a value through a (hi, lo) pair, see pair_bound
PAIR_ABS = 2.0 ** -37


# ---- exact16 pairs ---------------------------------------------------------------------------------------------------------------
def pair_split(v):
    """hi = f16(v), lo = f16((v - hi) * 4096); numpy rounds float64 -> float16 once, to nearest even."""
    v = np.asarray(v, dtype=np.float64)
    hi = v.astype(np.float16)
    lo = ((v - hi.astype(np.float64)) * LO_SCALE).astype(np.float16)
    return hi, lo


def pair_join(hi, lo):
    """The exact value of a pair: float64 holds hi + lo * 2^-12 of two f16 numbers without rounding (at most 11 + 11 significand bits
    no more than 40 binary places apart)."""
    return np.asarray(hi, dtype=np.float64) + np.asarray(lo, dtype=np.float64) / LO_SCALE


def pair_bound(v):
    """|pair_join(pair_split(v)) - v| <= max(2^-22 |v|, 2^-37) for |v| < 2^15.

    hi = f16(v) is off by at most 2^-11 |v| (11 significand bits; 2^-25 absolutely where hi is subnormal), so the remainder
    r = (v - hi) * 2^12 has |r| <= 2 |v|: no overflow.  lo = f16(r) is off by at most 2^-11 |r| <= 2^-11 * 2^-11 |v| * 2^12 =
    2^-10 |v| while lo is normal, and by at most 2^-25 (half the subnormal spacing 2^-24) otherwise.  The join descales that by
    2^-12: 2^-22 |v|, or 2^-37.  For |v| >= 2^-6 the first term is at least 2^-28 and decides alone."""
    return np.maximum(PAIR_REL * np.abs(np.asarray(v, dtype=np.float64)), PAIR_ABS)


def pair_positive(hi, lo):
    """The documented sign of a saved activation held as a pair: hi decides unless it is zero, then lo does."""
    hi = np.asarray(hi, dtype=np.float64)
    lo = np.asarray(lo, dtype=np.float64)
    return (hi > 0) | ((hi == 0) & (lo > 0))


# ---- space to depth and the virtual kernel ---------------------------------------------------------------------------------------
def s2d_ref(x):
    """[n,h,w,c] -> [n,h/2,w/2,4c]: pixel (2Y+i, 2X+j) becomes the channel block i*2+j of pixel (Y, X)."""
    n, h, w, c = x.shape
    blocks = [x[:, i::2, j::2, :] for i in range(2) for j in range(2)]
    return np.concatenate(blocks, axis=3)


def d2s_ref(p):
    """The inverse: [n,h/2,w/2,4c] -> [n,h,w,c]."""
    n, h2, w2, c4 = p.shape
    c = c4 // 4
    x = np.zeros((n, 2 * h2, 2 * w2, c), dtype=p.dtype)
    for i in range(2):
        for j in range(2):
            x[:, i::2, j::2, :] = p[..., (i * 2 + j) * c:(i * 2 + j + 1) * c]
    return x


def virtual_ref(w4):
    """A 4x4 stride-2 pad-1 kernel [cout,C,4,4] as the 3x3 pad-1 kernel [cout,4C,3,3] over the space-to-depth image.

    Output pixel (Y, X) of the 4x4 conv reads input rows 2Y - 1 + ky.  Row 2(Y + ty - 1) + i of the input is row Y + ty - 1, block
    row i of the packed image, which a 3x3 pad-1 kernel reaches with tap ty: so tap (ty, i) carries ky = 2 ty + i - 1 when that lies
    in 0..3, and zero otherwise (columns alike)."""
    cout, C = w4.shape[:2]
    w3 = np.zeros((cout, 4 * C, 3, 3), dtype=w4.dtype)
    for ty in range(3):
        for i in range(2):
            ky = 2 * ty + i - 1
            if not 0 <= ky < 4:
                continue
            for tx in range(3):
                for j in range(2):
                    kx = 2 * tx + j - 1
                    if 0 <= kx < 4:
                        w3[:, (i * 2 + j) * C:(i * 2 + j + 1) * C, ty, tx] = w4[:, :, ky, kx]
    return w3


def fold_ref(w3):
    """The virtual [cout,4C,3,3] weight (gradient) back as [cout,C,4,4]: each real tap reads the one virtual tap that carries it."""
    cout, C4 = w3.shape[:2]
    C = C4 // 4
    w4 = np.zeros((cout, C, 4, 4), dtype=w3.dtype)
    for ty in range(3):
        for i in range(2):
            ky = 2 * ty + i - 1
            if not 0 <= ky < 4:
                continue
            for tx in range(3):
                for j in range(2):
                    kx = 2 * tx + j - 1
                    if 0 <= kx < 4:
                        w4[:, :, ky, kx] = w3[:, (i * 2 + j) * C:(i * 2 + j + 1) * C, ty, tx]
    return w4


# ---- bilinear x2 -----------------------------------------------------------------------------------------------------------------
def bilinear_matrix(n):
    """[2n, n] interpolation matrix of torch's bilinear upsampling by 2 with align_corners=False: output o samples the input at
    max((o + 0.5) / 2 - 0.5, 0), between floor(s) and min(floor(s) + 1, n - 1)."""
    m = np.zeros((2 * n, n), dtype=np.float64)
    for o in range(2 * n):
        s = max((o + 0.5) / 2.0 - 0.5, 0.0)
        i0 = int(np.floor(s))
        i1 = min(i0 + 1, n - 1)
        lam = s - i0
        m[o, i0] += 1.0 - lam
        m[o, i1] += lam
    return m


def bilinear_up_ref(x, dtype=np.float64):
    """[n,h,w,c] -> [n,2h,2w,c], evaluated in `dtype` (the weights 0, 0.25, 0.75, 1 are exact in either)."""
    x = np.asarray(x, dtype=dtype)
    my, mx = bilinear_matrix(x.shape[1]).astype(dtype), bilinear_matrix(x.shape[2]).astype(dtype)
    return np.einsum("oy,nyxc,px->nopc", my, x, mx)


def bilinear_up_bwd_ref(g, dtype=np.float64):
    """The adjoint: [n,2h,2w,c] -> [n,h,w,c]."""
    g = np.asarray(g, dtype=dtype)
    my, mx = bilinear_matrix(g.shape[1] // 2).astype(dtype), bilinear_matrix(g.shape[2] // 2).astype(dtype)
    return np.einsum("oy,nopc,px->nyxc", my, g, mx)


# ---- add + LeakyReLU backward ----------------------------------------------------------------------------------------------------
def add_mask_ref(a, b, positive, slope):
    """(a + b) * (positive ? 1 : slope); b and positive (a boolean array: "the saved activation is > 0") may be None."""
    v = np.asarray(a, dtype=np.float64)
    if b is not None:
        v = v + np.asarray(b, dtype=np.float64)
    if positive is not None:
        v = v * np.where(positive, 1.0, float(slope))
    return v


# ---- 2x2 max pooling -------------------------------------------------------------------------------------------------------------
def maxpool_ref(x):
    """[n,2ho,2wo,c] -> (max [n,ho,wo,c], arg uint8): arg = dy*2+dx of the FIRST maximum in that order (np.argmax returns the first)."""
    win = np.stack([x[:, dy::2, dx::2, :] for dy in range(2) for dx in range(2)])
    arg = np.argmax(win, axis=0)
    return np.take_along_axis(win, arg[None], axis=0)[0], arg.astype(np.uint8)


def maxpool_bwd_ref(g, arg):
    """g [n,ho,wo,c] goes to the recorded window position of gin [n,2ho,2wo,c]; zeros elsewhere."""
    n, ho, wo, c = g.shape
    gin = np.zeros((n, 2 * ho, 2 * wo, c), dtype=g.dtype)
    for dy in range(2):
        for dx in range(2):
            gin[:, dy::2, dx::2, :] = np.where(arg == dy * 2 + dx, g, 0)
    return gin


# ---- reductions ------------------------------------------------------------------------------------------------------------------
def l1_sum_ref(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).sum())


def weighted_rows_ref(partial, coef):
    """out[r] = coef[r] * sum_k partial[r][k], out[rows] = their total."""
    rows = np.asarray(coef, dtype=np.float64) * np.asarray(partial, dtype=np.float64).sum(axis=1)
    return np.concatenate([rows, [rows.sum()]])


# ---- spectral norm ---------------------------------------------------------------------------------------------------------------
def _normalize(x, eps):
    return x / max(float(np.sqrt((x * x).sum())), eps)


def spectral_norm_ref(w, u, v, training, eps, dtype=np.float64):
    """torch.nn.utils.spectral_norm's forward on the weight as a [rows, cols] matrix: in training one power iteration
    v = normalize(W^T u), u = normalize(W v) with normalize(x) = x / max(||x||, eps); then sigma = u . (W v).  Returns (u, v, sigma)
    evaluated in `dtype` (float64: the reference; float32: the plain evaluation whose error sets the GPU tests' allowance)."""
    w, u, v = (np.asarray(t, dtype=dtype) for t in (w, u, v))
    if training:
        v = _normalize(w.T @ u, dtype(eps)).astype(dtype)
        u = _normalize(w @ v, dtype(eps)).astype(dtype)
    sigma = dtype(u @ (w @ v))
    return u, v, sigma


def spectral_norm_bwd_ref(g, w, u, v, sigma, dtype=np.float64):
    """Gradient wrt W_orig of W = W_orig / sigma, sigma = u^T W_orig v with u, v constant: G / sigma - (<G, W_orig> / sigma^2) u v^T."""
    g, w, u, v = (np.asarray(t, dtype=dtype) for t in (g, w, u, v))
    sigma = dtype(sigma)
    return (g / sigma - ((g * w).sum(dtype=dtype) / (sigma * sigma)) * np.outer(u, v)).astype(dtype)
