"""The bit-exact reference of csrc/image_resize.hip (its DEFINITION, lines 4-12) in numpy, and the cases the kernel is judged on.

`fmaf32` is the correctly rounded fp32 fused multiply-add; `resize_f32` / `resize_u8` restate the definition with it: per axis
acc = fmaf(v[idx[k]], w[k], acc) from acc = 0, k ascending, H pass first, fp32 intermediate; uint8 is `* 255.0f` rounded to fp32,
NaN and negatives to 0, clamp to 255, truncate.  tests/test_resize_ref.py proves the reference on the CPU (against libm's fmaf, the
nine goldens, and a list of mutations bit equality must reject); tests/test_gpu_resize_kernel.py holds the kernel to it bit for bit.
Nothing here touches a device."""
import ctypes as C
import math
from collections import namedtuple

import numpy as np


# ---- fmaf ---------------------------------------------------------------------------------------------------------------------
def fmaf32(a, b, c):
    """round_fp32(a * b + c), one rounding, elementwise on fp32 arrays (broadcast).

    The product of two fp32 is exact in float64 (48 significant bits).  s = p + c is rounded once to float64; TwoSum gives the exact
    error e of that sum.  Where e != 0 the true value lies strictly between s and its neighbour on e's side, and s is replaced by
    whichever of the two has an odd last bit (round to odd).  A float64 rounded to odd carries 53 >= 24 + 2 bits, so the final
    rounding to fp32 (normal or subnormal) is the rounding of the exact value: no double rounding.  Non-finite s (an inf or NaN
    operand, inf - inf, 0 * inf) is what IEEE gives for the fused operation too, and is cast as it is."""
    a, b, c = (np.asarray(v, dtype=np.float32) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c = c.astype(np.float64)
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        s, e = np.broadcast_arrays(s, e)
        bits = s.copy().view(np.int64)
        # s even and inexact: step one float64 towards the true value (magnitude up where e has the sign of s, else down)
        fix = np.isfinite(s) & (e != 0) & ((bits & 1) == 0)
        up = (e > 0) == (s > 0)
        bits = np.where(fix, np.where(up, bits + 1, bits - 1), bits)
        return bits.view(np.float64).astype(np.float32)


def libm_fmaf():
    """The C library's fmaf as a function of three Python floats, or None where no libm can be loaded."""
    import ctypes.util
    for name in (ctypes.util.find_library("m"), "libm.so.6"):
        if not name:
            continue
        try:
            f = C.CDLL(name).fmaf
        except (OSError, AttributeError):
            continue
        f.restype = C.c_float
        f.argtypes = [C.c_float] * 3
        return f
    return None


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def axis_pass(v, idx, w, axis, fma=fmaf32, order=None):
    """One pass of the definition along `axis` (-2: H, -1: W) of v [..., H, W]: out[..., i, ...] = the fma chain over the taps of
    output i, from acc = 0, in `order` (ascending unless given)."""
    idx = np.asarray(idx)
    w = np.asarray(w, dtype=np.float32)
    out_len, taps = idx.shape
    shape = list(v.shape)
    shape[axis] = out_len
    acc = np.zeros(shape, np.float32)
    for k in (range(taps) if order is None else order):
        if axis == -2:
            acc = fma(v[..., idx[:, k], :], w[:, k][:, None], acc)
        else:
            acc = fma(v[..., idx[:, k]], w[:, k], acc)
    return acc


def resize_f32(x, idx_y, w_y, idx_x, w_x):
    """fp32 [..., H, W] -> fp32 [..., oh, ow]: W-pass(H-pass(x))."""
    x = np.asarray(x, dtype=np.float32)
    return axis_pass(axis_pass(x, idx_y, w_y, -2), idx_x, w_x, -1)


def quantise_u8(v):
    """quantise<255> of csrc/yuv.h in fp32 steps: v * 255.0f rounded to fp32; NaN and negatives to 0; clamp; truncate."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(v, dtype=np.float32) * np.float32(255.0)
        v = np.where(v > 0, v, np.float32(0))
        v = np.where(v < 255, v, np.float32(255))
    return v.astype(np.uint8)


def resize_u8(x, idx_y, w_y, idx_x, w_x):
    """fp32 [N, 3, H, W] -> uint8 [N, oh, ow, 3]."""
    out = resize_f32(x, idx_y, w_y, idx_x, w_x)
    assert out.ndim == 4 and out.shape[1] == 3
    return np.ascontiguousarray(quantise_u8(out).transpose(0, 2, 3, 1))


# ---- the launch plan ----------------------------------------------------------------------------------------------------------------
F32, U8, YUV8, YUV10 = 0, 1, 2, 3       # csrc/common.h ResizeOut, the `kind` of resr_debug_resize_plan
Plan = namedtuple("Plan", "th tw rh rw pitch lds")


def plan_of(lib, n, c, h, w, oh, ow, taps_y, taps_x, kind):
    """resr_debug_resize_plan: the Plan of that launch, or None where the library refuses it."""
    out = (C.c_int32 * 6)()
    rc = lib.resr_debug_resize_plan(n, c, h, w, oh, ow, taps_y, taps_x, kind, out)
    return Plan(*out) if rc == 0 else None


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def band(n_in, r, aa=True):
    from real_esrgan_pytorch_amd import imgproc
    return imgproc.resize_band_tables(n_in, math.ceil(n_in * r), r, aa)


def admitted(n_in, r, aa=True):
    try:
        band(n_in, r, aa)
        return True
    except ValueError:
        return False


def shortest_admitted(r, aa=True, above=1):
    """The shortest axis longer than `above` that the rule admits (a one-pixel axis is always admitted: every tap reads that pixel)."""
    return next(n for n in range(above + 1, 4096) if admitted(n, r, aa))


def source(n, c, h, w, seed):
    """Seeded fp32 [n,c,h,w] overshooting [0, 1] as an unclamped SR output does; every value normal (no zero, no subnormal)."""
    x = np.random.RandomState(seed).uniform(-0.25, 1.25, size=(n, c, h, w)).astype(np.float32)
    x = np.where(np.abs(x) < 1e-6, np.float32(0.5), x)
    assert x.min() < -0.05 and x.max() > 1.05 or x.size < 64
    return np.ascontiguousarray(x)


class Case:
    """One launch of resr_image_resize: the source [n,c,h,w], the four tables, the tile the plan must choose (None: whatever it is,
    the case is not about the tile).  u8: also judged with uint8 output (c = 3)."""

    def __init__(self, name, x, ty, tx, tile=None, u8=None):
        self.name, self.x = name, np.ascontiguousarray(x, dtype=np.float32)
        (self.idx_y, self.w_y), (self.idx_x, self.w_x) = ty, tx
        self.tile = tile
        self.n, self.c, self.h, self.w = self.x.shape
        self.oh, self.ow = self.idx_y.shape[0], self.idx_x.shape[0]
        self.taps_y, self.taps_x = self.idx_y.shape[1], self.idx_x.shape[1]
        assert self.idx_y.dtype == self.idx_x.dtype == np.int32 and self.w_y.dtype == self.w_x.dtype == np.float32
        assert 0 <= self.idx_y.min() and self.idx_y.max() < self.h and 0 <= self.idx_x.min() and self.idx_x.max() < self.w
        self.u8 = (self.c == 3) if u8 is None else u8
        self._ref = None

    def tables(self):
        return self.idx_y, self.w_y, self.idx_x, self.w_x

    def ref_f32(self):
        """Computed once, shared, never modified."""
        if self._ref is None:
            self._ref = resize_f32(self.x, *self.tables())
            self._ref.setflags(write=False)
        return self._ref

    def ref_u8(self):
        return np.ascontiguousarray(quantise_u8(self.ref_f32()).transpose(0, 2, 3, 1))

    def plan(self, lib, kind=F32):
        return plan_of(lib, self.n, self.c, self.h, self.w, self.oh, self.ow, self.taps_y, self.taps_x, kind)

    def tiles_per_axis(self, plan):
        return -(-self.oh // plan.th), -(-self.ow // plan.tw)

    def __repr__(self):
        return self.name


def scaled(name, n, c, h, w, ry, rx=None, aa=True, tile=None, seed=0, x=None):
    rx = ry if rx is None else rx
    x = source(n, c, h, w, seed) if x is None else x
    return Case(name, x, band(h, ry, aa), band(w, rx, aa), tile)


def one_tap(idx, weights):
    return (np.ascontiguousarray(np.asarray(idx, np.int32)[:, None]), np.ascontiguousarray(np.asarray(weights, np.float32)[:, None]))


# r -> the tile a 96 x 96 source selects (fp32 and uint8 output alike): every entry of choose_tile's list
TILE_OF = {0.75: (32, 32), 0.5: (16, 32), 0.4: (16, 16), 0.3: (8, 16), 0.2: (8, 8), 0.15: (4, 8), 0.125: (4, 4), 0.1: (2, 4), 0.08: (2, 2),
           0.07: (1, 2), 0.0625: (1, 1)}
# a ragged, non-square source per tile: the same tile, outputs that are no multiple of it, several tiles per axis
RAGGED = {0.75: (97, 131), 0.5: (97, 131), 0.4: (97, 131), 0.3: (97, 131), 0.2: (97, 131), 0.15: (97, 131), 0.125: (97, 131),
          0.1: (103, 131), 0.08: (103, 131), 0.07: (97, 127), 0.0625: (97, 131)}
SMALL_SCALES = (0.3, 0.125, 0.0625)      # "three of the small scales": their shortest admitted lengths


def tile_cases():
    out = []
    for i, (r, tile) in enumerate(TILE_OF.items()):
        out.append(scaled(f"tile{tile[0]}x{tile[1]}_96x96_r{r}", 1, 3, 96, 96, r, tile=tile, seed=100 + i))
        h, w = RAGGED[r]
        out.append(scaled(f"tile{tile[0]}x{tile[1]}_{h}x{w}_r{r}", 1, 3, h, w, r, tile=tile, seed=200 + i))
    return out


def enlarge_cases():
    return [scaled(f"r{r}_{h}x{w}", 1, 3, h, w, r, seed=300 + i)
            for i, (r, h, w) in enumerate(((0.99, 41, 67), (1.01, 41, 67), (1.5, 29, 47), (2, 23, 37), (3, 13, 21)))]


def smallest_cases():
    out = [scaled("1x1_r1.5", 1, 3, 1, 1, 1.5, seed=400), scaled("1x9_r1.5", 1, 3, 1, 9, 1.5, seed=401),
           scaled("9x1_r1.5", 1, 3, 9, 1, 1.5, seed=402), scaled("2x2_r1.5", 1, 3, 2, 2, 1.5, seed=403),
           scaled("1x1_r0.5", 1, 3, 1, 1, 0.5, seed=404)]
    for i, r in enumerate(SMALL_SCALES):
        n = shortest_admitted(r)
        out.append(scaled(f"shortest{n}x{n}_r{r}", 1, 3, n, n, r, seed=410 + i))
        m = shortest_admitted(r, above=n)
        out.append(scaled(f"shortest{n}x{m}_r{r}", 1, 3, n, m, r, seed=420 + i))
        out.append(scaled(f"shortest1x{n}_r{r}", 1, 3, 1, n, r, seed=430 + i))
    return out


def channel_cases():
    """c in 1, 2, 3, 4, 7 with n in 1, 3 at r = 0.4 on 67 x 83 (2 x 3 ragged tiles of 16 x 16): the last channel group is partial."""
    return [scaled(f"n{n}_c{c}_67x83_r0.4", n, c, 67, 83, 0.4, tile=(16, 16), seed=500 + 10 * n + c) for n in (1, 3) for c in (1, 2, 3, 4, 7)]


def table_cases():
    out = [scaled("y0.25_x1.5_44x31", 1, 3, 44, 31, 0.25, 1.5, seed=600), scaled("y1.5_x0.25_31x44", 1, 3, 31, 44, 1.5, 0.25, seed=601)]
    h, w = 19, 23
    x = source(2, 3, h, w, 602)
    ident = lambda n: one_tap(np.arange(n), np.ones(n))
    out.append(Case("one_tap_identity", x, ident(h), ident(w)))
    out.append(Case("one_tap_reversal", x, one_tap(np.arange(h)[::-1], np.ones(h)), one_tap(np.arange(w)[::-1], np.ones(w))))
    rs = np.random.RandomState(603)
    out.append(Case("one_tap_negative_weight", x, one_tap(rs.randint(0, h, 27), np.full(27, -0.7)),
                    one_tap(rs.randint(0, w, 14), -rs.uniform(0.5, 1.5, 14))))
    for i, r in enumerate((0.5, 0.3, 0.125)):
        out.append(scaled(f"no_antialias_r{r}_96x83", 1, 3, 96, 83, r, aa=False, seed=610 + i))
    return out


def constant_cases():
    """uint8: values on integers and on both clamps.  (The weights of a row sum to 1 only up to rounding: what the bytes are is the
    reference's business.)"""
    out = []
    for i, v in enumerate((0.0, 1.0, 128 / 255, 1.2, -0.2)):
        x = np.full((1, 3, 21, 26), v, np.float32)
        out.append(scaled(f"constant_{v:.4g}_r0.75", 1, 3, 21, 26, 0.75, x=x))
        out.append(scaled(f"constant_{v:.4g}_r2", 1, 3, 7, 9, 2, x=x[:, :, :7, :9]))
    return out


def nonfinite_case():
    x = source(1, 3, 30, 34, 700)
    x[0, 0, 7, 9] = np.inf
    x[0, 1, 20, 25] = np.nan
    x[0, 2, 3, 30] = -np.inf
    return scaled("nonfinite_30x34_r0.4", 1, 3, 30, 34, 0.4, x=x)


def all_cases():
    return tile_cases() + enlarge_cases() + smallest_cases() + channel_cases() + table_cases() + constant_cases() + [nonfinite_case()]


# the small ones the mutations of tests/test_resize_ref.py are tried on
MUTATION_CASES = ("tile2x4_96x96_r0.1", "r1.5_29x47", "n1_c3_67x83_r0.4")


def mutation_cases():
    by_name = {c.name: c for c in all_cases()}
    return [by_name[name] for name in MUTATION_CASES]
