"""CPU: the bit-exact reference of the resize kernel (tests/resize_ref.py) is itself right, and bit equality is a gate that sees what
the 1e-6 gate cannot.  `fmaf32` against the C library's fmaf; the restatement against the reference project's own outputs (the nine
goldens); and a list of wrong kernels -- each a small change of the restatement -- that equality with the reference must reject on
at least one of the small cases tests/test_gpu_resize_kernel.py runs.  Nothing here touches a device."""
import os

import numpy as np
import pytest

from tests import resize_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_bits(got, want):
    """Equal int32 views, NaN where NaN is due (a NaN's payload is not part of the result)."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


# ---- fmaf32 -------------------------------------------------------------------------------------------------------------------
def _operands():
    rs = np.random.RandomState(1)
    n = 40000
    groups = {}
    # random: normal values, and magnitudes spread over the exponent range (results down to subnormals and up to overflow)
    groups["random"] = tuple(rs.standard_normal(n).astype(F) for _ in range(3))
    spread = lambda: (rs.standard_normal(n) * np.exp2(rs.randint(-70, 70, n))).astype(F)
    groups["spread"] = (spread(), spread(), spread())
    tiny = lambda: (rs.standard_normal(n) * np.exp2(rs.randint(-80, -55, n))).astype(F)
    groups["subnormal results"] = (tiny(), tiny(), (rs.standard_normal(n) * np.exp2(-140.0)).astype(F))
    # products that cancel c: c = -round(a * b), and a neighbour of it
    a, b = rs.standard_normal(n).astype(F), rs.standard_normal(n).astype(F)
    c = -(a * b)
    groups["cancelling"] = (a, b, c)
    groups["cancelling, one ulp off"] = (a, b, np.nextafter(c, F(np.inf) * np.where(rs.rand(n) < 0.5, F(-1), F(1))).astype(F))
    # ties: a * b is exactly half an ulp of c, added or subtracted; and a hair more or less than half
    c = (rs.uniform(1, 2, n) * np.exp2(rs.randint(-20, 20, n)) * np.where(rs.rand(n) < 0.5, -1, 1)).astype(F)
    half_ulp = (np.spacing(np.abs(c)) / 2).astype(F)
    k = np.exp2(rs.randint(-10, 10, n)).astype(F)
    sign = np.where(rs.rand(n) < 0.5, F(-1), F(1))
    groups["ties"] = (k * sign, half_ulp / k, c)
    # (2^46 + 1 = 8392705 * 8384513 and 2^46 - 1 = (2^23 + 1)(2^23 - 1): half an ulp times 1 +- 2^-46, a hair float64's sum cannot hold)
    scale = (half_ulp * F(2.0 ** -46)) / k
    groups["ties, a hair above"] = (k * sign * F(8392705), F(8384513) * scale, c)
    groups["ties, a hair below"] = (k * sign * F(2 ** 23 + 1), F(2 ** 23 - 1) * scale, c)
    # powers of two in c: the ulp below is half the ulp above
    p2 = np.exp2(rs.randint(-20, 20, n)).astype(F)
    groups["ties at a power of two"] = (k * sign, (np.spacing(p2) / 4).astype(F) / k, p2)
    special = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 3e38, -3e38, 1e-45, -1e-45, 1.17549435e-38], F)
    g = np.stack(np.meshgrid(special, special, special, indexing="ij"), -1).reshape(-1, 3)
    groups["special values"] = (g[:, 0].copy(), g[:, 1].copy(), g[:, 2].copy())
    return groups


def test_fmaf32_is_the_c_librarys_fmaf():
    fmaf = rr.libm_fmaf()
    if fmaf is None:
        pytest.skip("no C math library could be loaded: fmaf32 has nothing to be compared with")
    total = 0
    for name, (a, b, c) in _operands().items():
        got = rr.fmaf32(a, b, c)
        assert got.dtype == np.float32 and got.shape == a.shape
        want = np.array([fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], F)
        nan = np.isnan(want)
        bad = (np.isnan(got) != nan) | (~nan & (_bits(got) != _bits(want)))
        print(f"fmaf32 against libm, {name}: {int(bad.sum())} of {a.size} differ")
        assert not bad.any(), (name, [(float(a[i]), float(b[i]), float(c[i]), float(got[i]), float(want[i])) for i in np.flatnonzero(bad)[:4]])
        if name.startswith("ties, a hair"):      # the crafted operands are what they claim: float64 a * b + c rounds twice on them
            twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)
            assert np.isfinite(want).all() and (_bits(twice) != _bits(want)).mean() > 0.2, name
        total += a.size
    assert total >= 350000


def test_fmaf32_is_not_the_two_roundings():
    """The two near-misses the reference must not be: float64 a * b + c cast to fp32, and fp32 product then fp32 sum."""
    a, b, c = _operands()["ties, a hair above"]
    want = rr.fmaf32(a, b, c)
    twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)
    split = (a * b + c).astype(F)
    assert (_bits(twice) != _bits(want)).any() and (_bits(split) != _bits(want)).any()
    assert rr.fmaf32(F(3), F(5), F(-15)).tobytes() == F(0).tobytes() and float(rr.fmaf32(F(2), F(3), F(4))) == 10.0
    assert rr.fmaf32(np.ones((2, 3), F), F(2), np.zeros(3, F)).shape == (2, 3)              # broadcasts


# ---- the restatement against the reference project's outputs ------------------------------------------------------------------------
def test_restatement_meets_the_goldens():
    golden = np.load(os.path.join(ROOT, "tests", "golden", "image_resize_native.npz"))
    assert len(golden["cases"]) == 9
    for i, (h, w, r) in enumerate(golden["cases"]):
        x, ref = golden[f"in_{i}"], golden[f"out_{i}"]
        got = rr.resize_f32(x, *rr.band(int(h), float(r)), *rr.band(int(w), float(r)))
        assert got.dtype == np.float32 and got.shape == ref.shape
        err = float(np.abs(got.astype(np.float64) - ref).max())
        print(f"golden {int(h)}x{int(w)} x {r}: max |restatement - reference| = {err:.3e}")
        assert err <= 1e-6, (h, w, r, err)


def test_quantise_u8_steps():
    v = np.array([0.0, -0.0, -1e-3, 1.0, 1.0 + 1e-6, 128 / 255, 0.999999, 0.5, np.nan, np.inf, -np.inf, 254.5 / 255, 3.0], F)
    assert rr.quantise_u8(v).tolist() == [0, 0, 0, 255, 255, 128, 254, 127, 0, 255, 0, 254, 255]
    # the multiply is an fp32 multiply: the byte is the truncation of the fp32 product
    v = np.random.RandomState(2).uniform(-0.1, 1.1, 100000).astype(F)
    assert np.array_equal(rr.quantise_u8(v), np.floor(np.clip(v * F(255), 0, 255)).astype(np.uint8))


# ---- bit equality rejects wrong kernels ---------------------------------------------------------------------------------------------
def _split_fma(a, b, c):
    return ((a * b).astype(F) + c).astype(F)


def _w_then_h(case):
    return rr.axis_pass(rr.axis_pass(case.x, case.idx_x, case.w_x, -1), case.idx_y, case.w_y, -2)


def _product_rounded(case):
    return rr.axis_pass(rr.axis_pass(case.x, case.idx_y, case.w_y, -2, _split_fma), case.idx_x, case.w_x, -1, _split_fma)


def _descending(case):
    mid = rr.axis_pass(case.x, case.idx_y, case.w_y, -2, order=range(case.taps_y - 1, -1, -1))
    return rr.axis_pass(mid, case.idx_x, case.w_x, -1, order=range(case.taps_x - 1, -1, -1))


def _tap_dropped(case):
    w_y = case.w_y.copy()
    row = case.oh // 2
    last = np.flatnonzero(w_y[row])[-1]
    w_y[row, last] = 0                                            # fmaf(v, 0, acc) = acc: the tap is not accumulated
    return rr.resize_f32(case.x, case.idx_y, w_y, case.idx_x, case.w_x)


def _region_one_short(case, lib):
    """Every tile's table entries clamped into a region one pixel smaller than the tile's span, as the kernel clamps them into a
    region of `rh` x `rw` pixels: what a span_bound one too small would do to a tile that fills the bound."""
    plan = case.plan(lib)

    def clamp(idx, t):
        idx = idx.copy()
        for o in range(0, idx.shape[0], t):
            lo, hi = idx[o:o + t].min(), idx[o:o + t].max()
            idx[o:o + t] = lo + np.clip(idx[o:o + t] - lo, 0, max(hi - lo - 1, 0))
        return idx
    return rr.resize_f32(case.x, clamp(case.idx_y, plan.th), case.w_y, clamp(case.idx_x, plan.tw), case.w_x)


def _u8_rounded(case):
    with np.errstate(invalid="ignore"):
        v = np.clip(np.nan_to_num(case.ref_f32() * F(255), nan=0.0), 0, 255)
    return np.ascontiguousarray(np.rint(v).astype(np.uint8).transpose(0, 2, 3, 1))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import real_esrgan_pytorch_amd as R
    return R._lib.lib()


@pytest.fixture(scope="module")
def cases():
    out = rr.mutation_cases()
    assert [c.name for c in out] == list(rr.MUTATION_CASES) and all(c.c == 3 and c.x.size <= 3 * 96 * 96 for c in out)
    return out


FLOAT_MUTATIONS = {"W pass before H pass": _w_then_h, "product rounded before the add": _product_rounded,
                   "taps accumulated in descending order": _descending, "last non-zero tap of one row dropped": _tap_dropped}


@pytest.mark.parametrize("name", list(FLOAT_MUTATIONS))
def test_bit_equality_rejects_float_mutation(cases, name):
    rejected = []
    for case in cases:
        got, ref = FLOAT_MUTATIONS[name](case), case.ref_f32()
        assert got.shape == ref.shape
        differ = int((_bits(got) != _bits(ref)).sum())
        within = float(np.abs(got.astype(np.float64) - ref).max()) <= 1e-6
        print(f"{name} on {case.name}: {differ} of {ref.size} elements differ in bits; within 1e-6 everywhere: {within}")
        if not _same_bits(got, ref):
            rejected.append(case.name)
    assert rejected, f"mutation '{name}' gives the reference's bits on every case: bit equality would not see it"


def test_bit_equality_rejects_undersized_region(cases, lib):
    name = "a tile's indices clamped to a region one pixel smaller than its span"
    rejected = []
    for case in cases:
        got, ref = _region_one_short(case, lib), case.ref_f32()
        differ = int((_bits(got) != _bits(ref)).sum())
        print(f"{name} on {case.name}: {differ} of {ref.size} elements differ in bits")
        if not _same_bits(got, ref):
            rejected.append(case.name)
    assert rejected, f"mutation '{name}' gives the reference's bits on every case: bit equality would not see it"


def test_byte_equality_rejects_rounding_in_the_uint8_stage(cases):
    name = "truncation replaced by rounding in the uint8 stage"
    rejected = []
    for case in cases:
        got, ref = _u8_rounded(case), case.ref_u8()
        assert got.shape == ref.shape == (case.n, case.oh, case.ow, 3)
        print(f"{name} on {case.name}: {int((got != ref).sum())} of {ref.size} bytes differ")
        if not np.array_equal(got, ref):
            rejected.append(case.name)
    assert rejected, f"mutation '{name}' gives the reference's bytes on every case: byte equality would not see it"


def test_the_reference_is_the_definition_unmutated(cases):
    """The helpers above with nothing changed are the reference: a mutation is rejected for what it changes, not for how it is written."""
    for case in cases:
        same = rr.axis_pass(rr.axis_pass(case.x, case.idx_y, case.w_y, -2, order=range(case.taps_y)), case.idx_x, case.w_x, -1,
                            order=range(case.taps_x))
        assert _same_bits(same, case.ref_f32())
        assert np.array_equal(rr.resize_u8(case.x, *case.tables()), case.ref_u8())


# ---- the case table is what it claims -------------------------------------------------------------------------------------------------
def test_the_cases_reach_every_tile_of_the_list(lib):
    """Every entry of choose_tile's list is selected by a 96 x 96 case and by a ragged one, for fp32 and for uint8 output; the ragged
    outputs are no multiple of the tile (where the tile is wider than one pixel) and span several tiles per axis."""
    tile_list = [(32, 32), (16, 32), (16, 16), (8, 16), (8, 8), (4, 8), (4, 4), (2, 4), (2, 2), (1, 2), (1, 1)]
    assert list(rr.TILE_OF.values()) == tile_list
    seen = {}
    for case in rr.tile_cases():
        for kind in (rr.F32, rr.U8):
            plan = case.plan(lib, kind)
            assert plan is not None and (plan.th, plan.tw) == case.tile, (case.name, kind, plan)
        ty, tx = case.tiles_per_axis(plan)
        assert ty >= 2 and tx >= 2, (case.name, ty, tx)
        if (case.h, case.w) != (96, 96):
            assert (plan.th == 1 or case.oh % plan.th) and (plan.tw == 1 or case.ow % plan.tw), (case.name, case.oh, case.ow)
            assert case.h != case.w
        seen.setdefault(case.tile, []).append(case.name)
    assert sorted(seen) == sorted(tile_list) and all(len(v) == 2 for v in seen.values()), seen
    # uint8 rows off the 4-byte grid: an odd output width, and tile origins of 3, 6 and 12 bytes
    assert any(c.ow & 1 for c in rr.tile_cases()) and {1, 2, 4} <= {c.tile[1] for c in rr.tile_cases()}


def test_every_case_is_admitted_and_small(lib):
    cases = rr.all_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names) >= 70
    for case in cases:
        assert case.c <= 7 and case.h <= 131 and case.w <= 131, case.name
        assert case.plan(lib, rr.F32) is not None, case.name
        finite = case.x[np.isfinite(case.x)]
        assert (np.abs(finite) >= np.finfo(F).tiny).all() or case.name.startswith("constant_0"), case.name      # no subnormal, no zero
        # within the region bound: the kernel's clamp never acts on these tables (tables that exceed it are out of scope)
        plan = case.plan(lib, rr.U8 if case.u8 else rr.F32)
        for kind_plan in {plan, case.plan(lib, rr.F32)}:
            for idx, t, cap in ((case.idx_y, kind_plan.th, kind_plan.rh), (case.idx_x, kind_plan.tw, kind_plan.rw)):
                for o in range(0, idx.shape[0], t):
                    assert idx[o:o + t].max() - idx[o:o + t].min() + 1 <= cap, (case.name, o, t, cap)
    for group in ("tile", "r0.99", "r3", "1x1", "shortest", "n1_c7", "n3_c4", "y0.25_x1.5", "one_tap", "no_antialias", "constant", "nonfinite"):
        assert any(name.startswith(group) for name in names), group
