"""-m gpu: the discriminator / VGG helper kernels (csrc/disc.hip, weighted_row_sums of csrc/loss.hip) one at a time through the C ABI,
against the float64 references of tests/disc_helpers_ref.py (validated on the CPU by tests/test_disc_helpers_ref.py).

How a result is judged
  * order-free arithmetic (permutations, max, one add followed by one multiply, fold): BIT FOR BIT against a CPU restatement in the
    documented precision -- fp32 arithmetic on the values the kernel loads (a RESR_F16X2 pair loads as the fp32 rounding of the exact
    hi + lo * 2^-12, one fma), stored by one rounding to the tensor's type (a pair: hi = f16(v), lo = f16((v - hi) * 4096)).
  * sums in a fixed but unspecified order (spectral norm, l1_partial, weighted_row_sums, the bilinear gathers): against float64.  The
    allowance is 4 x the error a plain fp32 CPU evaluation of the same reference on the same inputs shows against float64 -- the
    factor covers another summation order, nothing else -- with a floor of one fp32 ulp of the result; both are maxima over the
    output tensor.  exact16 outputs are joined in float64 and get the pair round trip (disc_helpers_ref.pair_bound) on top.
    Every such judgement is written to <diag_dir>/test_gpu_disc_helpers.json: cpu32_err, allowance, kernel_err.
  * every output lies between two sentinel-filled guards of 64 elements and is itself pre-filled with the sentinel: the guards must
    survive and every element in range must have been written.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import disc_helpers_ref as ref
from tests.gpu_util import GUARD, INT, SENT, TINT, TORCH, Operand, Out, dev, np_type

pytestmark = pytest.mark.gpu

SLOPE = float(np.float32(0.2))
DIAG = {}


@pytest.fixture(scope="module")
def L():
    import real_esrgan_pytorch_amd as R
    R._lib.lib()
    return R._lib


@pytest.fixture(scope="module", autouse=True)
def _write_diag(diag_dir):
    yield
    worst = max(DIAG.items(), key=lambda kv: kv[1]["ratio"], default=None)
    with open(os.path.join(diag_dir, "test_gpu_disc_helpers.json"), "w") as f:
        json.dump({"worst": None if worst is None else {"case": worst[0], **worst[1]}, "cases": DIAG}, f, indent=1, sort_keys=True)


def ok(L, rc):
    assert rc == 0, (rc, L.lib().resr_last_error())


RESR_ERR_ARG = -1             # include/resr.h


def refused(L, rc, word="bad argument"):
    assert rc == RESR_ERR_ARG, rc
    assert word in (L.lib().resr_last_error() or b"").decode()


def E_of(L, dtype):
    return 4 if dtype == L.RESR_F32 else 8


# ---- device buffers --------------------------------------------------------------------------------------------------------------
def store(L, dtype, v32):
    """One rounding of fp32 results to the stored form (flat; pair: hi then lo).  v - hi and its scaling by 4096 are exact in fp32."""
    v32 = np.asarray(v32, dtype=np.float32)
    if dtype == L.RESR_F32:
        return v32.reshape(-1)
    hi = v32.astype(np.float16)
    if dtype == L.RESR_F16:
        return hi.reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        lo = ((v32 - hi.astype(np.float32)) * np.float32(4096)).astype(np.float16)
    return np.concatenate([hi.reshape(-1), lo.reshape(-1)])


def value(L, dtype, flat, shape):
    """float64 value of a stored result."""
    n = int(np.prod(shape))
    if dtype == L.RESR_F16X2:
        return ref.pair_join(flat[:n], flat[n:]).reshape(shape)
    return flat.astype(np.float64).reshape(shape)


def same_bits(got, want, what=""):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.dtype == want.dtype and got.size == want.size, (what, got.dtype, want.dtype, got.size, want.size)
    bad = np.flatnonzero(got.view(INT[got.dtype]) != want.view(INT[want.dtype]))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} elements differ in bits, first at {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}"


def judge(case, got, want, cpu32, pair=False):
    """The sums rule (module docstring)."""
    got, want, cpu32 = (np.asarray(a, dtype=np.float64) for a in (got, want, cpu32))
    cpu_err = float(np.abs(cpu32 - want).max())
    floor = float(np.spacing(np.float32(np.abs(want).max())))
    allowance = max(4.0 * cpu_err, floor) + (float(ref.pair_bound(want).max()) if pair else 0.0)
    kernel_err = float(np.abs(got - want).max())
    worst = int(np.argmax(np.abs(got - want)))
    print(f"{case}: worst element {worst}: got {got.reshape(-1)[worst]!r} want {want.reshape(-1)[worst]!r} cpu32 {cpu32.reshape(-1)[worst]!r}")
    DIAG[case] = {"cpu32_err": cpu_err, "floor_ulp": floor, "allowance": allowance, "kernel_err": kernel_err,
                  "ratio": kernel_err / allowance}
    print(f"{case}: cpu32_err {cpu_err:.3e} allowance {allowance:.3e} kernel_err {kernel_err:.3e}")
    assert kernel_err <= allowance, (case, DIAG[case])


def seq_sum32(a):
    """A plain left-to-right fp32 sum."""
    a = np.asarray(a, dtype=np.float32).reshape(-1)
    return np.cumsum(a, dtype=np.float32)[-1]


def planted_mask(rng, L, shape):
    """A RESR_F16X2 mask with the sign rule's corner cases planted twice: at the start (one 16-byte piece holds several) and in the
    last piece.  Returns (Operand, positive, planted flat indices)."""
    hi, lo = ref.pair_split(rng.standard_normal(shape).astype(np.float32).astype(np.float64))
    hf, lf = hi.reshape(-1), lo.reshape(-1)
    tiny = np.float16(6e-8)                                                   # the smallest positive f16
    cases = [(0.0, 0.5), (0.0, -0.5), (-0.0, 0.5), (0.0, 0.0), (tiny, -0.5)]   # (hi, lo)
    want = [True, False, True, False, True]                                   # hi > 0 or (hi == 0 and lo > 0)
    idx = list(range(5)) + (list(range(hf.size - 5, hf.size)) if hf.size >= 16 else [])
    for k, i in enumerate(idx):
        hf[i], lf[i] = cases[k % 5]
    m = Operand(L, L.RESR_F16X2, hi=hi, lo=lo)
    pos = ref.pair_positive(m.hi, m.lo)
    assert [bool(pos.reshape(-1)[i]) for i in idx] == (want + want)[:len(idx)]
    return m, pos, idx


S2D_SHAPES = [(1, 2, 2, 8), (3, 6, 10, 24), (2, 4, 172, 24)]
DTYPES = ["f16", "f32", "f16x2"]


def dt_of(L, name):
    return {"f16": L.RESR_F16, "f32": L.RESR_F32, "f16x2": L.RESR_F16X2}[name]


# ---- space to depth --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DTYPES)
@pytest.mark.parametrize("shape", S2D_SHAPES)
def test_space_to_depth_and_inverse(L, shape, dname):
    dtype, (n, h, w, c) = dt_of(L, dname), shape
    rng = np.random.default_rng(h * 1000 + w)
    x = Operand(L, dtype, rng.standard_normal(shape))
    nb = 2 * n if dtype == L.RESR_F16X2 else n                    # hi and lo travel as one batch of 2n
    full = x.flat.reshape(nb, h, w, c)
    out = Out(x.flat.size, x.flat.dtype)
    ok(L, L.lib().resr_space_to_depth(x.ptr, out.ptr, n, h, w, c, dtype, 0, None))
    packed = out.read()
    same_bits(packed, ref.s2d_ref(full), "space_to_depth")
    back = Out(x.flat.size, x.flat.dtype)
    ok(L, L.lib().resr_space_to_depth(out.ptr, back.ptr, n, h, w, c, dtype, 1, None))
    same_bits(back.read(), x.flat, "depth_to_space(space_to_depth)")
    same_bits(ref.d2s_ref(packed.reshape(nb, h // 2, w // 2, 4 * c)), x.flat, "reference inverse")


@pytest.mark.parametrize("dname", DTYPES)
def test_space_to_depth_refusals(L, dname):
    dtype = dt_of(L, dname)
    e = E_of(L, dtype)
    buf = torch.zeros(2 * 2 * 4 * 4 * 2 * e, dtype=TORCH[np_type(L, dtype)], device="cuda")     # [2n, 4, 4, 2E]: every shape below rounded up
    dst = torch.zeros_like(buf)
    for n, h, w, c in ((2, 3, 4, e), (2, 4, 3, e), (2, 4, 4, e + e // 2), (2, 4, 4, 0), (0, 4, 4, e)):
        for inverse in (0, 1):
            refused(L, L.lib().resr_space_to_depth(buf.data_ptr(), dst.data_ptr(), n, h, w, c, dtype, inverse, None))
    refused(L, L.lib().resr_space_to_depth(None, dst.data_ptr(), 2, 4, 4, e, dtype, 0, None))
    torch.cuda.synchronize()
    assert not dst.any()


# ---- depth to space + add + mask -------------------------------------------------------------------------------------------------
def strong(rng, shape):
    """|value| >= 0.5: a wrong LeakyReLU branch moves a result by at least 0.4."""
    v = rng.standard_normal(shape)
    return np.sign(v) * (0.5 + np.abs(v))


@pytest.mark.parametrize("dname", ["f16", "f32"])
@pytest.mark.parametrize("shape", S2D_SHAPES)
def test_d2s_add_mask_equals_two_passes(L, shape, dname):
    """csrc/disc.hip: "the same roundings as s2d(inverse) followed by add_mask, one pass instead of two" -- bit for bit, and both equal
    to fp32 (src + add) * (mask > 0 ? 1 : slope) rounded ONCE to the tensor's type.

    Regression: the fused kernel used to round the f16 sum to f16 BEFORE the multiplier and again after it; with add and mask both
    present about one element in ten differed from the two passes it replaced (3252 of 33024 at (2, 4, 172, 24))."""
    dtype, (n, h, w, c) = dt_of(L, dname), shape
    rng = np.random.default_rng(h * 1000 + w + 1)
    packed_shape = (n, h // 2, w // 2, 4 * c)
    src = Operand(L, dtype, strong(rng, packed_shape))
    add = Operand(L, dtype, rng.standard_normal(shape) * 3)
    mbase = rng.standard_normal(shape)
    mbase.reshape(-1)[:4] = [0.0, -0.0, 1.0, -1.0]
    mask = Operand(L, dtype, mbase)
    count = n * h * w * c
    for use_add in (False, True):
        for use_mask in (False, True):
            what = f"d2s_add_mask[{dname},{shape},add={use_add},mask={use_mask}]"
            a, m = (add if use_add else None), (mask if use_mask else None)
            fused = Out(count, src.flat.dtype)
            ok(L, L.lib().resr_debug_d2s_add_mask(src.ptr, a and a.ptr, m and m.ptr, fused.ptr, n, h, w, c, dtype, SLOPE, None))
            got = fused.read()
            tmp, two = Out(count, src.flat.dtype), Out(count, src.flat.dtype)
            ok(L, L.lib().resr_space_to_depth(src.ptr, tmp.ptr, n, h, w, c, dtype, 1, None))
            ok(L, L.lib().resr_add_mask(tmp.ptr, a and a.ptr, m and m.ptr, two.ptr, count, dtype, SLOPE, None))
            two_pass = two.read()
            v = ref.d2s_ref(src.v32)
            if use_add:
                v = v + add.v32
            if use_mask:
                v = v * np.where(mask.v32 > 0, np.float32(1), np.float32(SLOPE))
            assert v.dtype == np.float32
            same_bits(two_pass, store(L, dtype, v), what + " two passes vs restatement")
            same_bits(got, store(L, dtype, v), what + " fused vs restatement")
            same_bits(got, two_pass, what + " fused vs two passes")


@pytest.mark.parametrize("shape", S2D_SHAPES)
def test_d2s_add_mask_exact16(L, shape):
    dtype, (n, h, w, c) = L.RESR_F16X2, shape
    rng = np.random.default_rng(h * 1000 + w + 2)
    src = Operand(L, dtype, strong(rng, (n, h // 2, w // 2, 4 * c)))
    mask, pos, idx = planted_mask(rng, L, shape)
    abase = rng.standard_normal(shape)
    abase.reshape(-1)[idx] = 8.0                                      # |src + add| >= 4 where the mask's corner cases sit
    add = Operand(L, dtype, abase)
    count = n * h * w * c
    for use_add in (False, True):
        for use_mask in (False, True):
            case = f"d2s_add_mask[f16x2,{shape},add={use_add},mask={use_mask}]"
            a, m = (add if use_add else None), (mask if use_mask else None)
            out = Out(2 * count, np.float16)
            ok(L, L.lib().resr_debug_d2s_add_mask(src.ptr, a and a.ptr, m and m.ptr, out.ptr, n, h, w, c, dtype, SLOPE, None))
            got = value(L, dtype, out.read(), shape)
            want = ref.add_mask_ref(ref.d2s_ref(src.exact), add.exact if use_add else None, pos if use_mask else None, SLOPE)
            v = ref.d2s_ref(src.v32)
            if use_add:
                v = v + add.v32
            if use_mask:
                v = v * np.where(pos, np.float32(1), np.float32(SLOPE))
            judge(case, got, want, v, pair=True)
            if use_mask:                                              # the planted elements one by one: the other branch is >= 0.4 away
                assert np.abs(want.reshape(-1)[idx]).min() >= 0.1
                assert np.abs(got.reshape(-1)[idx] - want.reshape(-1)[idx]).max() <= 1e-5


# ---- bilinear x2 -----------------------------------------------------------------------------------------------------------------
BIL_SHAPES = [(2, 7, 5, 64), (1, 1, 9, 8), (3, 6, 1, 16), (2, 16, 24, 128), (1, 2, 2, 8), (1, 1, 1, 8)]


def run_bilinear(L, dtype, op, n, h, w, c, backward):
    count = n * h * w * c * (1 if backward else 4) * (2 if dtype == L.RESR_F16X2 else 1)
    out = Out(count, op.flat.dtype)
    ok(L, L.lib().resr_bilinear_up2x(op.ptr, out.ptr, n, h, w, c, dtype, backward, None))
    return out.read()


@pytest.mark.parametrize("shape", BIL_SHAPES)
def test_bilinear_up2x_all_types(L, shape):
    n, h, w, c = shape
    up_shape = (n, 2 * h, 2 * w, c)
    rng = np.random.default_rng(h * 100 + w)
    xb, gb = rng.standard_normal(shape), rng.standard_normal(up_shape)
    res = {}
    for dname in DTYPES:
        dtype = dt_of(L, dname)
        x, g = Operand(L, dtype, xb), Operand(L, dtype, gb)
        up = value(L, dtype, run_bilinear(L, dtype, x, n, h, w, c, 0), up_shape)
        gin_flat = run_bilinear(L, dtype, g, n, h, w, c, 1)
        gin = value(L, dtype, gin_flat, shape)
        res[dname] = (x, g, up, gin, gin_flat)
        if dname != "f16":                                            # f16 results: judged through the f32 kernel below
            pair = dname == "f16x2"
            judge(f"bilinear_fwd[{dname},{shape}]", up, ref.bilinear_up_ref(x.exact), ref.bilinear_up_ref(x.v32, np.float32), pair)
            judge(f"bilinear_bwd[{dname},{shape}]", gin, ref.bilinear_up_bwd_ref(g.exact), ref.bilinear_up_bwd_ref(g.v32, np.float32), pair)
    # f16: the f32 kernel on the same f16 values, rounded once to f16 -- forward and backward
    for backward, k in ((0, 2), (1, 3)):
        op16 = res["f16"][backward]
        op32 = Operand(L, L.RESR_F32, op16.exact)
        r32 = run_bilinear(L, L.RESR_F32, op32, n, h, w, c, backward)
        same_bits(res["f16"][k].astype(np.float16), r32.astype(np.float16), f"bilinear f16 vs rounded f32, backward={backward}")
    # adjoint identity from the f32 outputs, in float64: each side is off by at most (its allowance) x (the 1-norm of the other factor)
    x, g, up, gin, _ = res["f32"]
    lhs, rhs = float((up * g.exact).sum()), float((x.exact * gin).sum())
    tol = (DIAG[f"bilinear_fwd[f32,{shape}]"]["allowance"] * np.abs(g.exact).sum()
           + DIAG[f"bilinear_bwd[f32,{shape}]"]["allowance"] * np.abs(x.exact).sum())
    assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)


@pytest.mark.parametrize("dname", DTYPES)
@pytest.mark.parametrize("shape", BIL_SHAPES)
def test_bilinear_bwd_mask(L, shape, dname):
    """gin is the plain backward bit for bit; gmasked = gin * (mask > 0 ? 1 : slope), for plain tensors from the ROUNDED gin like a
    separate add_mask pass, for pairs from the fp32 value.

    Regression (RESR_F16X2, the two shapes with c >= 64): where the fp32 product gin * slope sat exactly on an f16 tie, gmasked's hi
    came from one rounding of it and its lo from another -- an error of one f16 ulp of hi, 9.77e-4 against an allowance of 1.0e-5."""
    dtype, (n, h, w, c) = dt_of(L, dname), shape
    pairs = 2 if dtype == L.RESR_F16X2 else 1
    rng = np.random.default_rng(h * 100 + w + 7)
    g = Operand(L, dtype, 1.0 + np.abs(rng.standard_normal((n, 2 * h, 2 * w, c))))       # positive: every gin is >= 1
    count = n * h * w * c
    if dtype == L.RESR_F16X2:
        mask, pos, idx = planted_mask(rng, L, shape)
    else:
        mbase = rng.standard_normal(shape)
        mbase.reshape(-1)[:4] = [0.0, -0.0, 1.0, -1.0]
        mask = Operand(L, dtype, mbase)
    plain = run_bilinear(L, dtype, g, n, h, w, c, 1)
    gin, gm = Out(pairs * count, g.flat.dtype), Out(pairs * count, g.flat.dtype)
    ok(L, L.lib().resr_debug_bilinear_up2x_bwd_mask(g.ptr, gin.ptr, mask.ptr, gm.ptr, n, h, w, c, dtype, SLOPE, None))
    gin_flat, gm_flat = gin.read(), gm.read()
    same_bits(gin_flat, plain, "gin of bwd_mask vs the plain backward")
    if dtype != L.RESR_F16X2:
        two = Out(count, g.flat.dtype)
        ok(L, L.lib().resr_add_mask(gin.ptr, None, mask.ptr, two.ptr, count, dtype, SLOPE, None))
        same_bits(gm_flat, two.read(), "gmasked vs add_mask(gin, NULL, mask)")
        v = value(L, dtype, gin_flat, shape).astype(np.float32) * np.where(mask.v32 > 0, np.float32(1), np.float32(SLOPE))
        same_bits(gm_flat, store(L, dtype, v), "gmasked vs restatement")
    else:
        mult = np.where(pos, 1.0, SLOPE)
        want = ref.bilinear_up_bwd_ref(g.exact) * mult
        cpu32 = ref.bilinear_up_bwd_ref(g.v32, np.float32) * mult.astype(np.float32)
        got = value(L, dtype, gm_flat, shape)
        k = int(np.argmax(np.abs(got - want)))
        print(f"worst {k}: gmasked (hi, lo) = ({gm_flat[k]!r}, {gm_flat[count + k]!r}), gin (hi, lo) = ({gin_flat[k]!r}, {gin_flat[count + k]!r}), "
              f"mask (hi, lo) = ({mask.hi.reshape(-1)[k]!r}, {mask.lo.reshape(-1)[k]!r})")
        judge(f"bilinear_bwd_mask[f16x2,{shape}]", got, want, cpu32, pair=True)
        assert np.abs(want.reshape(-1)[idx]).min() >= 0.1
        assert np.abs(got.reshape(-1)[idx] - want.reshape(-1)[idx]).max() <= 1e-4


def test_bilinear_refusals(L):
    buf = torch.zeros(4096, device="cuda")
    for fn in (lambda *a: L.lib().resr_debug_bilinear_up2x_bwd_mask(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), *a, SLOPE, None),
               lambda *a: L.lib().resr_debug_d2s_add_mask(buf.data_ptr(), None, None, buf.data_ptr(), *a, SLOPE, None)):
        refused(L, fn(1, 2, 2, 6, L.RESR_F32))
        refused(L, fn(1, 2, 2, 12, L.RESR_F16))
        refused(L, fn(0, 2, 2, 8, L.RESR_F16))
    refused(L, L.lib().resr_debug_d2s_add_mask(buf.data_ptr(), None, None, buf.data_ptr(), 1, 3, 2, 8, L.RESR_F32, SLOPE, None))
    refused(L, L.lib().resr_debug_bilinear_up2x_bwd_mask(buf.data_ptr(), buf.data_ptr(), None, buf.data_ptr(), 1, 2, 2, 8, L.RESR_F32, SLOPE, None))


# ---- add_mask --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DTYPES)
def test_add_mask(L, dname):
    """Bit for bit: fp32 (a + b) * (mask > 0 ? 1 : slope), one rounding.  RESR_F16X2: a, b, out are pairs with the lo tensor `count`
    behind; the mask is read from its hi tensor ALONE (include/resr.h) -- a mask with hi == 0 and lo > 0 takes the slope."""
    dtype = dt_of(L, dname)
    e = E_of(L, dtype)
    for count in (e, 256 * e, 256 * e + e):                           # one thread / one full block / one thread of a second block
        rng = np.random.default_rng(count)
        a, b = Operand(L, dtype, rng.standard_normal(count)), Operand(L, dtype, rng.standard_normal(count))
        mbase = rng.standard_normal(count)
        mbase[:4] = [0.0, -0.0, 1.0, -1.0]
        mbase[-1] = 0.0
        if dtype == L.RESR_F16X2:
            mhi = mbase.astype(np.float16)
            mask = Operand(L, dtype, hi=mhi, lo=np.where(mhi == 0, np.float16(0.5), np.float16(-0.5)))   # lo says the opposite of hi > 0
            assert ref.pair_positive(mask.hi, mask.lo)[0] and not (mask.hi > 0)[0]
        else:
            mask = Operand(L, dtype, mbase)
        positive = mask.hi.astype(np.float32) > 0
        for use_b in (False, True):
            for use_mask in (False, True):
                for slope in (SLOPE, 0.0):
                    out = Out(a.flat.size, a.flat.dtype)
                    ok(L, L.lib().resr_add_mask(a.ptr, b.ptr if use_b else None, mask.ptr if use_mask else None, out.ptr, count, dtype,
                                                slope, None))
                    v = a.v32 + b.v32 if use_b else a.v32
                    if use_mask:
                        v = v * np.where(positive, np.float32(1), np.float32(slope))
                    same_bits(out.read(), store(L, dtype, v), f"add_mask[{dname},count={count},b={use_b},mask={use_mask},slope={slope}]")
    buf = torch.zeros(64, dtype=TORCH[np_type(L, dtype)], device="cuda")
    refused(L, L.lib().resr_add_mask(buf.data_ptr(), None, None, buf.data_ptr(), e + 1, dtype, SLOPE, None))
    refused(L, L.lib().resr_add_mask(buf.data_ptr(), None, None, buf.data_ptr(), 0, dtype, SLOPE, None))


# ---- max pooling -----------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 1, 1, 8), (2, 3, 5, 24), (1, 7, 37, 64)]


def tie_rich(rng, shape):
    """Integers 0..3; a quarter of the windows all equal (2), a quarter all zero (as after ReLU)."""
    n, h, w, c = shape
    x = rng.integers(0, 4, size=shape).astype(np.float64)
    win = rng.integers(0, 4, size=(n, h // 2, w // 2, c))
    for dy in range(2):
        for dx in range(2):
            v = x[:, dy::2, dx::2, :]
            v[win == 0] = 2.0
            v[win == 1] = 0.0
    return x


def tied_windows(x):
    """Fraction of windows whose maximum occurs more than once."""
    win = np.sort(np.stack([x[:, dy::2, dx::2, :] for dy in range(2) for dx in range(2)]), axis=0)
    return float((win[-1] == win[-2]).mean())


@pytest.mark.parametrize("kind", ["random", "ties"])
@pytest.mark.parametrize("dname", DTYPES)
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool2x2_arg_and_backward(L, shape, dname, kind):
    dtype, (n, ho, wo, c) = dt_of(L, dname), shape
    in_shape = (n, 2 * ho, 2 * wo, c)
    rng = np.random.default_rng(ho * 100 + wo + (kind == "ties"))
    if kind == "random":
        src = Operand(L, dtype, rng.standard_normal(in_shape))
    elif dtype != L.RESR_F16X2:
        src = Operand(L, dtype, tie_rich(rng, in_shape))
    else:
        # hi ties everywhere (integers 0..3, equal / zero windows); lo in {0, 1, 2} decides some windows and ties the whole pair in others
        hi = tie_rich(rng, in_shape).astype(np.float16)
        lo = rng.integers(0, 3, size=in_shape).astype(np.float16)
        lo[rng.integers(0, 2, size=in_shape) == 0] = 0
        src = Operand(L, dtype, hi=hi, lo=lo)
        if src.exact.size > 32:
            assert (ref.maxpool_ref(src.exact)[1] != ref.maxpool_ref(hi.astype(np.float64))[1]).any()      # somewhere lo decides
    want_max, want_arg = ref.maxpool_ref(src.v32)
    if kind == "ties" and src.exact.size > 32:
        assert tied_windows(src.exact) > 0.2                        # the maximum of the full value occurs twice
    pairs = 2 if dtype == L.RESR_F16X2 else 1
    count = n * ho * wo * c
    dst, dst2, arg = Out(pairs * count, src.flat.dtype), Out(pairs * count, src.flat.dtype), Out(count, np.uint8)
    ok(L, L.lib().resr_maxpool2x2_arg(src.ptr, dst.ptr, arg.ptr, n, ho, wo, c, dtype, None))
    ok(L, L.lib().resr_maxpool2x2(src.ptr, dst2.ptr, n, ho, wo, c, dtype, None))
    got = dst.read()
    same_bits(got, store(L, dtype, want_max), "maxpool dst")
    same_bits(dst2.read(), got, "resr_maxpool2x2 vs resr_maxpool2x2_arg")
    got_arg = arg.read()
    assert np.array_equal(got_arg.reshape(want_arg.shape), want_arg), f"{(got_arg.reshape(want_arg.shape) != want_arg).sum()} wrong winners"
    g = Operand(L, dtype, rng.standard_normal(shape))
    gin = Out(pairs * 4 * count, src.flat.dtype)
    ok(L, L.lib().resr_maxpool2x2_bwd(g.ptr, arg.ptr, gin.ptr, n, ho, wo, c, dtype, None))
    same_bits(gin.read(), store(L, dtype, ref.maxpool_bwd_ref(g.v32, want_arg)), "maxpool backward (zeros included)")


def test_maxpool_refusals(L):
    buf = torch.zeros(4096, device="cuda")
    arg = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    for dtype, c in ((L.RESR_F32, 6), (L.RESR_F16, 12), (L.RESR_F16X2, 4), (L.RESR_F32, 0)):
        refused(L, L.lib().resr_maxpool2x2(p, p, 1, 1, 1, c, dtype, None))
        refused(L, L.lib().resr_maxpool2x2_arg(p, p, arg.data_ptr(), 1, 1, 1, c, dtype, None))
        refused(L, L.lib().resr_maxpool2x2_bwd(p, arg.data_ptr(), p, 1, 1, 1, c, dtype, None))
    refused(L, L.lib().resr_maxpool2x2_bwd(p, None, p, 1, 1, 1, 8, L.RESR_F32, None))


# ---- l1_partial / weighted_row_sums ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DTYPES)
def test_l1_partial(L, dname):
    dtype = dt_of(L, dname)
    e = E_of(L, dtype)
    for count in (e, 256 * e + e, 5 * 256 * e + 3 * e):
        rng = np.random.default_rng(count + 1)
        a, b = Operand(L, dtype, rng.standard_normal(count)), Operand(L, dtype, rng.standard_normal(count))
        lo_offset = 0
        if dtype == L.RESR_F16X2:                                     # a view into a larger batch: NaNs between the hi and the lo tensor
            pad = np.full(24, np.nan, dtype=np.float16)
            lo_offset = count + pad.size
            ta, tb = (dev(np.concatenate([o.hi, pad, o.lo])) for o in (a, b))
            pa, pb = ta.data_ptr(), tb.data_ptr()
        else:
            pa, pb = a.ptr, b.ptr
        want = ref.l1_sum_ref(a.exact, b.exact)
        cpu32 = seq_sum32(np.abs(a.v32 - b.v32))
        for nblocks in (1, 3, 64):
            runs = []
            for _ in range(2):
                part = Out(nblocks, np.float32)
                ok(L, L.lib().resr_l1_partial(pa, pb, count, dtype, lo_offset, part.ptr, nblocks, None))
                runs.append(part.read())                              # every workgroup wrote, the idle ones too
            same_bits(runs[0], runs[1], "l1_partial, two runs")
            idle = np.arange(nblocks) * 256 * e >= count
            assert (runs[0][idle] == 0).all() and (runs[0][~idle] > 0).all()
            judge(f"l1_partial[{dname},count={count},nblocks={nblocks}]", runs[0].astype(np.float64).sum(), want, cpu32)
    buf = torch.zeros(64, device="cuda")
    refused(L, L.lib().resr_l1_partial(buf.data_ptr(), buf.data_ptr(), e + 1, dtype, 0, buf.data_ptr(), 1, None))
    refused(L, L.lib().resr_l1_partial(buf.data_ptr(), buf.data_ptr(), e, dtype, 0, buf.data_ptr(), 0, None))


@pytest.mark.parametrize("rows", [1, 4, 5, 8])
def test_weighted_row_sums(L, rows):
    for cols in (1, 63, 64, 65, 1000):
        rng = np.random.default_rng(rows * 10000 + cols)
        partial = np.abs(rng.standard_normal((rows, cols))).astype(np.float32) * 50
        coef = (rng.uniform(0.1, 1.0, size=rows)).astype(np.float32)
        tp = dev(partial)
        out = Out(rows + 1, np.float32)
        ok(L, L.lib().resr_weighted_row_sums(tp.data_ptr(), rows, cols, (C.c_float * rows)(*coef.tolist()), out.ptr, None))
        got = out.read()
        want = ref.weighted_rows_ref(partial, coef)
        r32 = np.array([coef[r] * seq_sum32(partial[r]) for r in range(rows)], dtype=np.float32)
        cpu32 = np.concatenate([r32, [seq_sum32(r32)]])
        judge(f"weighted_row_sums[rows={rows},cols={cols}]", got, want, cpu32)
    tp = torch.zeros(64, device="cuda")
    coef9 = (C.c_float * 9)(*([1.0] * 9))
    refused(L, L.lib().resr_weighted_row_sums(tp.data_ptr(), 0, 4, coef9, tp.data_ptr(), None))
    refused(L, L.lib().resr_weighted_row_sums(tp.data_ptr(), 9, 4, coef9, tp.data_ptr(), None))
    refused(L, L.lib().resr_weighted_row_sums(tp.data_ptr(), 4, 0, coef9, tp.data_ptr(), None))


# ---- spectral norm ---------------------------------------------------------------------------------------------------------------
def unit(rng, n):
    v = rng.standard_normal(n)
    return (v / np.linalg.norm(v)).astype(np.float32)


def sn_inputs(rows, cols, scale=None):
    rng = np.random.default_rng(rows * 7919 + cols)
    w = (rng.standard_normal((rows, cols)) * (scale or 1 / np.sqrt(cols))).astype(np.float32)
    return w, unit(rng, rows), unit(rng, cols)


def tmp_floats(rows, cols):
    return rows + (rows + 31) // 32 * cols            # include/resr.h


class SnRun:
    """Buffers of one layer: u in place (it is read), v pre-filled with the sentinel in training (it is only written there)."""

    def __init__(self, w, u0, v0, training):
        rows, cols = w.shape
        self.rows, self.cols, self.training = rows, cols, training
        self.w = dev(w)
        self.u = Out(rows, np.float32).load(u0)
        self.v = Out(cols, np.float32)
        if not training:
            self.v.load(v0)
        self.sigma2 = Out(2, np.float32)
        self.tmp = Out(tmp_floats(rows, cols), np.float32)

    def read(self):
        self.tmp.read(written=False)
        return self.u.read(), self.v.read(), self.sigma2.read()


def sn_single(L, w, u0, v0, training, eps):
    r = SnRun(w, u0, v0, training)
    ok(L, L.lib().resr_spectral_norm(r.w.data_ptr(), r.u.ptr, r.v.ptr, r.rows, r.cols, training, eps, r.sigma2.ptr, r.tmp.ptr, None))
    return r.read()


def judge_sn(case, got, w, u0, v0, training, eps):
    u, v, s2 = got
    ru, rv, rs = ref.spectral_norm_ref(w, u0, v0, training, eps)
    with np.errstate(all="ignore"):
        cu, cv, cs = ref.spectral_norm_ref(w, u0, v0, training, eps, np.float32)
        cinv = np.float32(1) / cs
    if training:
        judge(case + ".u", u, ru, cu)
        judge(case + ".v", v, rv, cv)
    else:
        same_bits(u, u0, case + ": eval mode leaves u alone")
        same_bits(v, v0, case + ": eval mode leaves v alone")
    judge(case + ".sigma", s2[0], rs, cs)
    judge(case + ".inv_sigma", s2[1], 1.0 / rs, cinv)


SN_SHAPES = [(1, 1), (30, 600), (33, 257), (128, 1024), (512, 4608)]


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("shape", SN_SHAPES)
def test_spectral_norm_single(L, shape, training):
    w, u0, v0 = sn_inputs(*shape)
    first = sn_single(L, w, u0, v0, training, 1e-12)
    second = sn_single(L, w, u0, v0, training, 1e-12)
    for a, b in zip(first, second):
        same_bits(a, b, "spectral_norm, two runs")
    judge_sn(f"spectral_norm[{shape},training={training}]", first, w, u0, v0, training, 1e-12)


def test_spectral_norm_eps_branch(L):
    """||W^T u|| < eps: v = W^T u / eps, not a unit vector; ||W v|| < eps as well.  On the largest layer, where sigma ~ 1e-37 is still a
    normal fp32 number."""
    w, u0, v0 = sn_inputs(512, 4608, scale=1e-20)
    got = sn_single(L, w, u0, v0, 1, 1e-12)
    assert np.linalg.norm(w.astype(np.float64).T @ u0) < 1e-12 and 0 < np.linalg.norm(got[1].astype(np.float64)) < 1e-6
    judge_sn("spectral_norm[eps branch (512, 4608) * 1e-20]", got, w, u0, v0, 1, 1e-12)


def ptr_array(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def int_array(v):
    return (C.c_int32 * len(v))(*v)


BATCH_LAYERS = [(33, 257), (128, 1024), (30, 600), (64, 300), (1, 1), (512, 4608), (7, 1000), (40, 40)]   # mixed, not monotone, 1 x 1 inside


@pytest.mark.parametrize("training", [1, 0])
def test_spectral_norm_batch_equals_single(L, training):
    """csrc/disc.hip: the batched launches the product runs promise the single-layer results bit for bit."""
    ins = [sn_inputs(r, c) for r, c in BATCH_LAYERS]
    singles = [sn_single(L, w, u0, v0, training, 1e-12) for w, u0, v0 in ins]
    runs = [SnRun(w, u0, v0, training) for w, u0, v0 in ins]
    rc = L.lib().resr_debug_spectral_norm_batch(
        len(runs), ptr_array([r.w.data_ptr() for r in runs]), ptr_array([r.u.ptr for r in runs]), ptr_array([r.v.ptr for r in runs]),
        int_array([r.rows for r in runs]), int_array([r.cols for r in runs]), training, 1e-12, ptr_array([r.sigma2.ptr for r in runs]),
        ptr_array([r.tmp.ptr for r in runs]), None)
    ok(L, rc)
    for shape, r, single in zip(BATCH_LAYERS, runs, singles):
        for name, a, b in zip(("u", "v", "sigma2"), r.read(), single):
            same_bits(a, b, f"batched spectral_norm layer {shape} {name}")


# ---- spectral norm backward ------------------------------------------------------------------------------------------------------
def snb_inputs(rows, cols):
    """The kernel's formula is linear algebra on ANY u, v and 1 / sigma: unit random vectors and an unrelated 1 / sigma keep the two
    terms from cancelling (with the power iteration's own values a 1 x 1 layer's gradient is pure rounding noise)."""
    rng = np.random.default_rng(rows * 104729 + cols)
    g = rng.standard_normal((rows, cols)).astype(np.float32)
    w = (rng.standard_normal((rows, cols)) / np.sqrt(cols)).astype(np.float32)
    sigma2 = np.array([1.7, 1 / 1.7], dtype=np.float32)
    d0 = rng.standard_normal((rows, cols)).astype(np.float32)
    return g, w, unit(rng, rows), unit(rng, cols), sigma2, d0


def snb_single(L, ins, accumulate):
    g, w, u, v, sigma2, d0 = ins
    rows, cols = g.shape
    dst = Out(rows * cols, np.float32)
    if accumulate:
        dst.load(d0)
    tmp1 = Out(512, np.float32)
    keep = [dev(a) for a in (g, w, u, v, sigma2)]
    ok(L, L.lib().resr_spectral_norm_bwd(*[t.data_ptr() for t in keep], dst.ptr, rows, cols, accumulate, tmp1.ptr, None))
    tmp1.read(written=False)
    return dst.read()


SNB_SHAPES = [(1, 1), (33, 257), (129, 1024)]                        # the last: > 512 * 256 elements, the dot's grid-stride loop wraps


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", SNB_SHAPES)
def test_spectral_norm_bwd_single(L, shape, accumulate):
    ins = snb_inputs(*shape)
    g, w, u, v, sigma2, d0 = ins
    first, second = snb_single(L, ins, accumulate), snb_single(L, ins, accumulate)
    same_bits(first, second, "spectral_norm_bwd, two runs")
    sigma = 1.0 / float(sigma2[1])                                    # the kernel reads sigma2[1] = 1 / sigma
    want = ref.spectral_norm_bwd_ref(g, w, u, v, sigma)
    cpu32 = ref.spectral_norm_bwd_ref(g, w, u, v, np.float32(1) / sigma2[1], np.float32)
    if accumulate:
        want, cpu32 = want + d0, cpu32 + d0
    judge(f"spectral_norm_bwd[{shape},accumulate={accumulate}]", first.reshape(shape), want, cpu32)


SNB_BATCH = [(33, 257), (129, 1024), (1, 1), (64, 300), (7, 1000), (256, 600), (30, 600), (40, 40)]


def test_spectral_norm_bwd_batch_equals_single(L):
    ins = [snb_inputs(r, c) for r, c in SNB_BATCH]
    singles = [snb_single(L, i, 0) for i in ins]
    keep = [[dev(a) for a in i[:5]] for i in ins]
    dsts = [Out(r * c, np.float32) for r, c in SNB_BATCH]
    dot = Out(8 * 512, np.float32)
    cols = [ptr_array([k[j].data_ptr() for k in keep]) for j in range(5)]
    ok(L, L.lib().resr_debug_spectral_norm_bwd_batch(len(ins), *cols, ptr_array([d.ptr for d in dsts]), int_array([r for r, _ in SNB_BATCH]),
                                                     int_array([c for _, c in SNB_BATCH]), dot.ptr, None))
    dot.read(written=False)
    for shape, d, single in zip(SNB_BATCH, dsts, singles):
        same_bits(d.read(), single, f"batched spectral_norm_bwd layer {shape}")


# ---- fold4x4 ---------------------------------------------------------------------------------------------------------------------
FOLD_SHAPES = [(1, 1), (3, 5), (5, 7), (128, 64)]


def fold_single(L, dw3):
    cout, c = dw3.shape[0], dw3.shape[1] // 4
    src, dst = dev(dw3), Out(cout * c * 16, np.float32)
    ok(L, L.lib().resr_fold4x4(src.data_ptr(), dst.ptr, cout, c, None))
    return dst.read()


def fold_input(cout, c):
    return np.random.default_rng(cout * 100 + c).standard_normal((cout, 4 * c, 3, 3)).astype(np.float32)


@pytest.mark.parametrize("shape", FOLD_SHAPES)
def test_fold4x4(L, shape):
    dw3 = fold_input(*shape)
    same_bits(fold_single(L, dw3), ref.fold_ref(dw3), f"fold4x4{shape}")


def test_fold4x4_batch_equals_single(L):
    shapes = [(5, 7), (3, 5), (128, 64), (1, 1)]                      # the 240-element layer second
    ins = [fold_input(*s) for s in shapes]
    singles = [fold_single(L, i) for i in ins]
    srcs = [dev(i) for i in ins]
    dsts = [Out(co * c * 16, np.float32) for co, c in shapes]
    ok(L, L.lib().resr_debug_fold4x4_batch(len(shapes), ptr_array([s.data_ptr() for s in srcs]), ptr_array([d.ptr for d in dsts]),
                                           int_array([s[0] for s in shapes]), int_array([s[1] for s in shapes]), None))
    for shape, d, single, i in zip(shapes, dsts, singles, ins):
        got = d.read()
        same_bits(got, single, f"batched fold4x4 layer {shape}")
        same_bits(got, ref.fold_ref(i), f"batched fold4x4 layer {shape} vs reference")


# ---- argument validation of the backward / batched dispatchers -------------------------------------------------------------------
def test_zero_sizes_and_null_layers_are_refused(L):
    """A zero dimension used to reach the runtime as a zero-sized grid.  Host-side checks only: every buffer below is large enough for
    the largest shape named (4 x 4 / cout 1, C 1), so no call could run past one if it were accepted."""
    buf = torch.zeros(4096, device="cuda")
    p = buf.data_ptr()
    lib = L.lib()
    for rows, cols in ((0, 4), (4, 0), (-1, 4)):
        refused(L, lib.resr_spectral_norm_bwd(p, p, p, p, p, p, rows, cols, 0, p, None))
        refused(L, lib.resr_spectral_norm(p, p, p, rows, cols, 1, 1e-12, p, p, None))
    two, good = ptr_array([p, p]), int_array([4, 4])
    hole = ptr_array([p, None])
    for rows, cols in ((int_array([4, 0]), good), (good, int_array([0, 4]))):
        refused(L, lib.resr_debug_spectral_norm_bwd_batch(2, two, two, two, two, two, two, rows, cols, p, None))
        refused(L, lib.resr_debug_spectral_norm_batch(2, two, two, two, rows, cols, 1, 1e-12, two, two, None))
    for k in range(6):
        args = [two] * 6
        args[k] = hole
        refused(L, lib.resr_debug_spectral_norm_bwd_batch(2, *args, good, good, p, None))
    refused(L, lib.resr_debug_spectral_norm_bwd_batch(0, two, two, two, two, two, two, good, good, p, None))
    refused(L, lib.resr_debug_spectral_norm_bwd_batch(9, two, two, two, two, two, two, good, good, p, None))
    refused(L, lib.resr_debug_spectral_norm_bwd_batch(2, two, two, two, two, two, two, good, good, None, None))
    one = int_array([1, 1])
    refused(L, lib.resr_debug_fold4x4_batch(2, two, two, int_array([1, 0]), one, None))
    refused(L, lib.resr_debug_fold4x4_batch(2, two, two, one, int_array([0, 1]), None))
    refused(L, lib.resr_debug_fold4x4_batch(2, hole, two, one, one, None))
    refused(L, lib.resr_debug_fold4x4_batch(2, two, hole, one, one, None))
    refused(L, lib.resr_debug_fold4x4_batch(5, two, two, one, one, None))
    refused(L, lib.resr_fold4x4(p, p, 0, 1, None))
    refused(L, lib.resr_fold4x4(p, p, 1, 0, None))
    torch.cuda.synchronize()
    assert not buf.any()
