"""-m gpu: the sparse-tap kernels of the discriminator's 4x4 / stride-2 layers, one launch at a time, element by element.

Three pieces of device code run these layers as 3x3 passes over the 2x2 space-to-depth image and skip the 20 of 36 (tap, sub-position)
blocks in which the virtual kernel of csrc/pack.hip is zero:
  * conv3x3_ws_kernel<.., SP = 1> (csrc/conv3x3_ws.h, instantiated in conv3x3_ws_sp.hip): the forward pass, chosen by
    ResrConvDesc.s2d_in_channels; the sub-position comes from the input chunk, (chunk * 32) / s2d_c;
  * conv3x3_ws_kernel<.., SP = 2>: backward-data with flipped taps, chosen by s2d_out_channels; the sub-position comes from the tile's
    output group, ((tile / ntiles_sp) * 64) / tap_c;
  * the weight-gradient quad kernel's xsub / x_s2d_c path (csrc/wgrad.hip), reached through resr_debug_conv3x3_wgrad_s2d, then resr_fold4x4.
The references are the float64 definitions of tests/conv_ref.py ON THE ORIGINAL IMAGE -- conv2d / conv_transpose2d with a [cout,C,4,4]
weight, stride 2, padding 1, and the weight gradient of that -- which know neither the space-to-depth image nor the virtual kernel
(tests/test_conv_ref.py ties the two views together on the CPU).  They get the values the kernel gets: operands after gpu_util.quant
(exact16: hi + lo / 4096), weights as resr_pack_weights sees them (f16: their f16 rounding).  Judged by the rule of
tests/test_gpu_kernels.py (conv_ref.judge): f16 outputs "f16", exact16 pair outputs "pair" and conv_ref.pair_lo_excess, fp32 dW within A,
exact16 dW within A + conv_ref.wgrad_lolo.  Outputs lie between guards.  Every sparse launch is bracketed by resr_profile_begin /
resr_profile_end and must record the sparse instantiation's kernel id, every fallback a dense one: a route whose conditions stop
matching would otherwise compute the right values on the dense kernel and nobody would see the speed go.
Every judgement goes to <diag_dir>/test_gpu_sparse_taps.json: cpu32_err, allowance, kernel_err, ratio; "worst" holds the worst ratio per
dtype and path."""
import ctypes as C
import json
import os
import zlib

import pytest
import torch

from tests import conv_ref as R
from tests.test_gpu_kernels import Guarded, Operand   # the guard helpers of the kernel tests, as they are

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
DIAG = {}
SLOPE = 0.2


@pytest.fixture(scope="module")
def U():
    import tests.gpu_util as U
    return U


@pytest.fixture(scope="module", autouse=True)
def _write_diag(diag_dir):
    yield
    worst = {}
    for name, rec in DIAG.items():
        if "ratio" not in rec:
            continue
        key = f"{rec['dtype']}/{rec['path']}"
        if key not in worst or rec["ratio"] > worst[key]["ratio"]:
            worst[key] = {"case": name, "ratio": rec["ratio"]}
    with open(os.path.join(diag_dir, "test_gpu_sparse_taps.json"), "w") as f:
        json.dump({"worst": worst, "cases": DIAG}, f, indent=1, sort_keys=True)


def judge(case, dtype_name, path, got, ref64, ref32, kind, extra=None):
    rec = R.judge(got, ref64, ref32, kind, extra)
    rec.update(dtype=dtype_name, kind=kind, path=path)
    DIAG[case] = rec
    print(f"{case}: cpu32_err {rec['cpu32_err']:.3e} allowance {rec['allowance']:.3e} kernel_err {rec['kernel_err']:.3e} "
          f"ratio {rec['ratio']:.3f} bad {rec['bad']} worst element {rec['worst']} of shape {tuple(ref64.shape)}: got {rec['got']!r} "
          f"want {rec['want']!r}")
    assert rec["bad"] == 0, (case, rec)


def _dt(L, name):
    return {"f32": L.RESR_F32, "f16": L.RESR_F16, "exact16": L.RESR_F16X2}[name]


def _td(L, dtype):
    return torch.float32 if dtype == L.RESR_F32 else torch.float16


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) % 100000)


def _weight(g, cout, c):
    return torch.randn(cout, c, 4, 4, generator=g) * (2.0 / (c * 16)) ** 0.5


# ---- which kernel ran -------------------------------------------------------------------------------------------------------------
def sparse_id(x2):
    """The kernel id resr_profile_end reports for a sparse-tap launch: csrc/conv3x3_ws.h, launch_ws_epi, the prof_after call --
    (X2 ? 25000 : 20000) + (SP ? 2000 : 0) + MT * 100 + NT * 10 + NWC -- with the one shape csrc/conv3x3_ws_sp.hip instantiates,
    launch_ws_epi<half_t, MT = 2, NT = 2, NWC = 4, ..>."""
    return (25000 if x2 else 20000) + 2000 + 2 * 100 + 2 * 10 + 4


def is_dense_conv_id(kid):
    """A conv3x3 launch that is none of the sparse ones: the one-role kernel (csrc/conv3x3.hip: 0 / 10000 + ..) or the
    producer/consumer kernel without the SP term (20000 / 25000 + MT * 100 + NT * 10 + NWC < 1000)."""
    return 0 < kid < 30000 and kid % 5000 < 1000


def profiled(L, call):
    """(status, kernel ids recorded) of one library call."""
    lib = L.lib()
    lib.resr_profile_begin()
    try:
        rc = call()
    finally:
        buf = (L.ProfEntry * 16)()
        k = int(lib.resr_profile_end(C.cast(buf, C.c_void_p), 16))
    return rc, [buf[i].kernel_id for i in range(min(k, 16))]


# ---- packing ----------------------------------------------------------------------------------------------------------------------
def pack4x4(U, w4, dtype, transposed):
    """resr_pack_weights of a [cout,C,4,4] weight from a chunk table with virtual4x4 = 1 (and transposed = 1 for backward-data), as
    tests/test_gpu_layout_kernels.py builds one: M = cout (transposed: the 4C virtual channels) in consecutive groups of 64 rows, each
    group holding its K / 32 chunks of mt = 2 -- the order ResrConvDesc.cout_groups documents."""
    L = U.L
    cout, c = w4.shape[:2]
    m_real, k_real = (4 * c, cout) if transposed else (cout, 4 * c)
    assert m_real % 64 == 0 and k_real % 32 == 0
    rows, dst = [], 0
    for g0 in range(0, m_real, 64):
        for k0 in range(0, k_real, 32):
            rows.append(L.PackChunk(0, dst, cout, c, g0, 64, k0, 32, 2, 1 if transposed else 0, 1.0, 1, None))
            dst += 9 * 2 * 1024
    table = L.upload_chunks((L.PackChunk * len(rows))(*rows), "cuda")
    arena = w4.reshape(-1).float().cuda()
    es = {L.RESR_F16: 2, L.RESR_F32: 4, L.RESR_F16X2: 6}[dtype]
    packed = torch.zeros(dst * es + 16384, dtype=torch.uint8, device="cuda")
    L.check(L.lib().resr_pack_weights(L.ptr(table), len(rows), L.ptr(arena), L.ptr(packed), dtype, L.stream_ptr()), "resr_pack_weights")
    return packed, (U.quant(w4, dtype) if dtype == L.RESR_F16 else w4)


# ---- one conv launch --------------------------------------------------------------------------------------------------------------
def run_conv(U, dtype, x_ptr, x_lo, packed, n, h, w, cin, groups, flags, slope, s2d_in=0, s2d_out=0, res0=None):
    """One resr_conv3x3 launch of `groups` 64-channel output groups on an NHWC input of `cin` channels (x_lo: its hi -> lo offset) into
    a guarded NHWC output.  Returns (the NCHW float64 value [n, 64 groups, h, w], the kernel ids recorded)."""
    L = U.L
    pair = dtype == L.RESR_F16X2
    ct = 64 * groups
    out = Guarded(n * h * w * ct * (2 if pair else 1), _td(L, dtype))
    d = L.ConvDesc(n, h, w, cin, cin, cin, 0, 64, 64, ct, 0, 0, 0, dtype, flags, 1.0, 1.0, 1.0, 1.0, slope)
    d.in0_lo_offset = x_lo
    d.out_lo_offset = n * h * w * ct if pair else 0
    d.cout_groups, d.s2d_in_channels, d.s2d_out_channels = groups, s2d_in, s2d_out
    if res0 is not None:
        d.res0_stride, d.s0, d.t0, d.res0_lo_offset = 64, 0.5, 0.25, res0.lo_offset
    rc, ids = profiled(L, lambda: L.lib().resr_conv3x3(C.byref(d), x_ptr, None, L.ptr(packed), None, L.ptr(res0.t) if res0 is not None else None,
                                                       None, None, L.ptr(out.body), None, L.stream_ptr()))
    L.check(rc, "resr_conv3x3")
    flat = out.read()
    if pair:
        hi, lo = flat[:flat.numel() // 2], flat[flat.numel() // 2:]
        assert R.pair_lo_excess(hi, lo) == 0, "a stored lo is no remainder of its hi"
        v = R.pair_value(hi, lo)
    else:
        v = flat.double()
    return v.reshape(n, h, w, ct).permute(0, 3, 1, 2), ids


def _kind(L, dtype):
    return {L.RESR_F16: "f16", L.RESR_F32: "f32", L.RESR_F16X2: "pair"}[dtype]


# ---- forward (SP = 1) -------------------------------------------------------------------------------------------------------------
FWD_CASES = [
    # name, C = s2d_in_channels, cout groups of 64, (n, h, w) of the OUTPUT, LeakyReLU
    ("c32_1x1x1", 32, 1, (1, 1, 1), True),              # cin 128: one chunk per sub-position
    ("c32_1x1x5", 32, 1, (1, 1, 5), True),
    ("c32_1x9x33", 32, 1, (1, 9, 33), True),            # two tile rows and two tile columns of the 8 x 32 tile, both ragged
    ("c32_1x9x33_linear", 32, 1, (1, 9, 33), False),    # NO_BIAS alone
    ("c64_g2_2x17x40", 64, 2, (2, 17, 40), True),       # two chunks per sub-position, cout 128: the network's DOWN1
    ("c96_1x9x33", 96, 1, (1, 9, 33), True),            # three chunks per sub-position: the chunk -> sub-position division is no shift
    # More tiles than the launch has workgroups, so that a workgroup walks several tiles and output groups.  launch_ws_epi
    # (csrc/conv3x3_ws.h) launches min(ntiles, resident) workgroups, resident = (workgroups per CU by the occupancy query) x 256 CUs;
    # this kernel asks for WsCfg::LDS_BYTES, which takes every weight buffer that fits into the 160 KB of a CU, so one workgroup per CU:
    # 256.  (4, 72, 72) is 3 x 9 x 4 = 108 spatial tiles x 8 groups = 864 tiles: three to four per workgroup (and still more than
    # two per CU would hold).
    ("c32_g8_many_tiles", 32, 8, (4, 72, 72), True),
]


def _fwd_inputs(name, c, groups, geo):
    n, h, w = geo
    g = _gen(name)
    return torch.randn(n, c, 2 * h, 2 * w, generator=g), _weight(g, 64 * groups, c)


def _fwd_refs(L, dtype, xv, wv, **epi):
    ref64 = R.conv4x4s2(xv, wv, F64, **epi)[0]
    ref32 = None if dtype == L.RESR_F16X2 else R.conv4x4s2(xv, wv, F32, **epi)[0]
    return ref64, ref32


@pytest.mark.parametrize("dtype_name", ["f16", "exact16"])
@pytest.mark.parametrize("case", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_forward_sparse(U, case, dtype_name):
    """conv2d(x [N,C,2h,2w], w [cout,C,4,4], stride 2, padding 1) + LeakyReLU 0.2 through SP = 1, on the Python space-to-depth of x."""
    L = U.L
    dtype = _dt(L, dtype_name)
    name, c, groups, (n, h, w), lrelu = case
    x, w4 = _fwd_inputs(name, c, groups, (n, h, w))
    xo = Operand(L, R.s2d(x), dtype, 4 * c)
    xv = R.d2s(xo.value)                                   # what the kernel is given, back on the original image
    packed, wv = pack4x4(U, w4, dtype, False)
    flags = L.CONV_NO_BIAS | (L.CONV_LRELU if lrelu else 0)
    got, ids = run_conv(U, dtype, L.ptr(xo.t), xo.lo_offset, packed, n, h, w, 4 * c, groups, flags, SLOPE, s2d_in=c)
    assert ids == [sparse_id(dtype == L.RESR_F16X2)], ids
    ref64, ref32 = _fwd_refs(L, dtype, xv, wv, lrelu=lrelu, slope=SLOPE)
    judge(f"fwd_{name}_{dtype_name}", dtype_name, "forward", got, ref64, ref32, _kind(L, dtype))


@pytest.mark.parametrize("dtype_name", ["f16", "exact16"])
def test_forward_input_from_space_to_depth_kernel(U, dtype_name):
    """The input tensor comes from resr_space_to_depth on an NHWC image (exact16: hi and lo as one batch of 2n), not from the Python
    s2d: the conv kernel's, the pack kernel's and the s2d kernel's sub-position orders against each other and against the definition."""
    L = U.L
    dtype = _dt(L, dtype_name)
    name, c, groups, (n, h, w) = "s2d_kernel_c64", 64, 1, (2, 9, 33)
    x, w4 = _fwd_inputs(name, c, groups, (n, h, w))
    img = Operand(L, x, dtype, c)                          # NHWC [n, 2h, 2w, C]; a pair: [2][n, 2h, 2w, C]
    nb = 2 * n if dtype == L.RESR_F16X2 else n
    xs = Guarded(nb * h * w * 4 * c, torch.float16)
    L.check(L.lib().resr_space_to_depth(L.ptr(img.t), L.ptr(xs.body), n, 2 * h, 2 * w, c, dtype, 0, L.stream_ptr()), "resr_space_to_depth")
    xs.read()
    packed, wv = pack4x4(U, w4, dtype, False)
    got, ids = run_conv(U, dtype, L.ptr(xs.body), n * h * w * 4 * c if dtype == L.RESR_F16X2 else 0, packed, n, h, w, 4 * c, groups,
                        L.CONV_NO_BIAS | L.CONV_LRELU, SLOPE, s2d_in=c)
    assert ids == [sparse_id(dtype == L.RESR_F16X2)], ids
    ref64, ref32 = _fwd_refs(L, dtype, img.value, wv, lrelu=True, slope=SLOPE)
    judge(f"fwd_{name}_{dtype_name}", dtype_name, "forward", got, ref64, ref32, _kind(L, dtype))


# ---- backward-data (SP = 2) -------------------------------------------------------------------------------------------------------
BWD_CASES = [
    # name, C = s2d_out_channels (4C / 64 output groups), (n, h, w) of G; K = 64 channels of G
    ("c64_1x1x1", 64, (1, 1, 1)),                       # 4 groups, one per sub-position
    ("c64_1x9x33", 64, (1, 9, 33)),
    ("c128_2x17x40", 128, (2, 17, 40)),                 # 8 groups, two per sub-position
    ("c192_1x9x33", 192, (1, 9, 33)),                   # 12 groups, three per sub-position
    ("c128_many_tiles", 128, (4, 72, 72)),              # 108 spatial tiles x 8 groups = 864 tiles on 256 workgroups (see FWD_CASES)
]
K_BWD = 64


def _bwd_inputs(name, c, geo):
    n, h, w = geo
    g = _gen(name)
    return torch.randn(n, K_BWD, h, w, generator=g), _weight(g, K_BWD, c)


def _run_bwd(U, dtype, name, c, geo, s2d_out):
    L = U.L
    n, h, w = geo
    gy, w4 = _bwd_inputs(name, c, geo)
    go = Operand(L, gy, dtype, K_BWD)
    packed, wv = pack4x4(U, w4, dtype, True)
    got, ids = run_conv(U, dtype, L.ptr(go.t), go.lo_offset, packed, n, h, w, K_BWD, 4 * c // 64, L.CONV_NO_BIAS, 0.0, s2d_out=s2d_out)
    return R.d2s(got), ids, go.value, wv


@pytest.mark.parametrize("dtype_name", ["f16", "exact16"])
@pytest.mark.parametrize("case", BWD_CASES, ids=[c[0] for c in BWD_CASES])
def test_backward_data_sparse(U, case, dtype_name):
    """conv_transpose2d(g [N,64,h,w], w [64,C,4,4], stride 2, padding 1) through SP = 2: the output [N,h,w,4C] is the space-to-depth
    image of the input gradient, compared after depth-to-space."""
    L = U.L
    dtype = _dt(L, dtype_name)
    name, c, geo = case
    got, ids, gv, wv = _run_bwd(U, dtype, name, c, geo, c)
    assert ids == [sparse_id(dtype == L.RESR_F16X2)], ids
    ref32 = None if dtype == L.RESR_F16X2 else R.dgrad4x4s2(gv, wv, F32)
    judge(f"bwd_{name}_{dtype_name}", dtype_name, "backward_data", got, R.dgrad4x4s2(gv, wv, F64), ref32, _kind(L, dtype))


# ---- fallbacks stay right and visible ---------------------------------------------------------------------------------------------
FALLBACKS = [
    # name, runs sparse?, changes to the base forward case c32_1x9x33 (C = 32, cout 64, NO_BIAS | LRELU 0.2)
    ("base", True, {}),
    ("hints0", False, {"s2d_in": 0}),
    ("slope1.5", False, {"slope": 1.5}),
    ("residual", False, {"res0": True}),
    ("slope0.0", True, {"slope": 0.0}),
    ("slope1.0", True, {"slope": 1.0}),
]


@pytest.mark.parametrize("dtype_name", ["f16", "exact16"])
def test_forward_fallbacks(U, dtype_name):
    """The same descriptor with one condition of the route (csrc/conv3x3_ws.hip, conv3x3_ws_f16) changed: the hint dropped, a slope
    outside [0, 1], a residual -- the dense kernel runs over the virtual kernel's zeros, and its result passes the same judgement;
    slopes 0 and 1 stay sparse.  Sparse and dense accumulate in different orders (ks, dx, dy against tap-major), so they are not
    compared bit for bit: the largest difference goes to the diag file."""
    L = U.L
    dtype = _dt(L, dtype_name)
    x2 = dtype == L.RESR_F16X2
    c, (n, h, w) = 32, (1, 9, 33)
    x, w4 = _fwd_inputs("c32_1x9x33", c, 1, (n, h, w))
    r0 = torch.randn(n, 64, h, w, generator=_gen("fallback_res0"))
    xo, ro = Operand(L, R.s2d(x), dtype, 4 * c), Operand(L, r0, dtype, 64)
    xv = R.d2s(xo.value)
    packed, wv = pack4x4(U, w4, dtype, False)
    results = {}
    for name, sparse, ch in FALLBACKS:
        slope, res0 = ch.get("slope", SLOPE), ro if ch.get("res0") else None
        got, ids = run_conv(U, dtype, L.ptr(xo.t), xo.lo_offset, packed, n, h, w, 4 * c, 1, L.CONV_NO_BIAS | L.CONV_LRELU, slope,
                            s2d_in=ch.get("s2d_in", c), res0=res0)
        assert len(ids) == 1 and ((ids[0] == sparse_id(x2)) if sparse else is_dense_conv_id(ids[0])), (name, ids)
        epi = dict(lrelu=True, slope=slope, **({"res0": ro.value, "s0": 0.5, "t0": 0.25} if res0 is not None else {}))
        ref64, ref32 = _fwd_refs(L, dtype, xv, wv, **epi)
        judge(f"fallback_fwd_{name}_{dtype_name}", dtype_name, "forward" if sparse else "dense_fallback", got, ref64, ref32, _kind(L, dtype))
        results[name] = got
    DIAG[f"sparse_vs_dense_fwd_{dtype_name}"] = {"max_abs_diff": float((results["base"] - results["hints0"]).abs().max())}


def test_forward_fallback_f32(U):
    """RESR_F32 with the hint set: strict mode has no sparse kernel, the one-role kernel takes all nine taps of the virtual kernel."""
    L = U.L
    dtype = L.RESR_F32
    c, (n, h, w) = 32, (1, 9, 33)
    x, w4 = _fwd_inputs("c32_1x9x33", c, 1, (n, h, w))
    xo = Operand(L, R.s2d(x), dtype, 4 * c)
    packed, wv = pack4x4(U, w4, dtype, False)
    got, ids = run_conv(U, dtype, L.ptr(xo.t), 0, packed, n, h, w, 4 * c, 1, L.CONV_NO_BIAS | L.CONV_LRELU, SLOPE, s2d_in=c)
    assert len(ids) == 1 and is_dense_conv_id(ids[0]), ids
    ref64, ref32 = _fwd_refs(L, dtype, R.d2s(xo.value), wv, lrelu=True, slope=SLOPE)
    judge("fallback_fwd_f32", "f32", "dense_fallback", got, ref64, ref32, "f32")


@pytest.mark.parametrize("dtype_name", ["f16", "exact16"])
def test_backward_data_fallback_without_hint(U, dtype_name):
    L = U.L
    dtype = _dt(L, dtype_name)
    name, c, geo = BWD_CASES[1]
    dense, ids, gv, wv = _run_bwd(U, dtype, name, c, geo, 0)
    assert len(ids) == 1 and is_dense_conv_id(ids[0]), ids
    ref32 = None if dtype == L.RESR_F16X2 else R.dgrad4x4s2(gv, wv, F32)
    judge(f"fallback_bwd_hints0_{dtype_name}", dtype_name, "dense_fallback", dense, R.dgrad4x4s2(gv, wv, F64), ref32, _kind(L, dtype))
    sparse, ids, _, _ = _run_bwd(U, dtype, name, c, geo, c)
    assert ids == [sparse_id(dtype == L.RESR_F16X2)], ids
    DIAG[f"sparse_vs_dense_bwd_{dtype_name}"] = {"max_abs_diff": float((sparse - dense).abs().max())}


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
REFUSALS = [
    # name, dtype, cin, s2d_in, s2d_out, cout_groups, extra flags, what the error text names
    ("s2d_in_not_multiple_of_32", "f16", 192, 48, 0, 1, 0, "s2d_in_channels"),
    ("cin_is_not_4_s2d_in", "f16", 96, 32, 0, 1, 0, "s2d_in_channels"),
    ("s2d_out_not_multiple_of_64", "f16", 64, 0, 32, 2, 0, "s2d_out_channels"),
    ("both_hints", "f16", 128, 32, 64, 4, 0, "s2d_out_channels"),
    ("groups_do_not_cover_s2d_out", "f16", 64, 0, 64, 2, 0, "s2d_out_channels"),
    ("mx_pairs_with_s2d_in", "exact16", 128, 32, 0, 1, "mx", "RESR_CONV_MX_PAIRS"),
    ("mx_pairs_with_s2d_out", "exact16", 64, 0, 64, 4, "mx", "RESR_CONV_MX_PAIRS"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals(U, case):
    """conv3x3_args / conv3x3_route (csrc/conv3x3.hip) refuse the descriptor with the argument error: no launch is recorded and the
    output keeps its sentinel."""
    L = U.L
    name, dtype_name, cin, s2d_in, s2d_out, groups, extra, text = case
    dtype = _dt(L, dtype_name)
    n, h, w = 1, 9, 33
    # operands large enough for whatever the descriptor names, should a kernel run after all
    x = torch.zeros(2 * n * h * w * 256 + 64, dtype=torch.float16, device="cuda")
    packed = torch.zeros(8 * 8 * 9 * 2 * 1024 * 6 * 2 + 16384, dtype=torch.uint8, device="cuda")
    out = Guarded(2 * n * h * w * 64 * groups, torch.float16)
    d = L.ConvDesc(n, h, w, cin, cin, cin, 0, 64, 64, 64 * groups, 0, 0, 0, dtype, L.CONV_NO_BIAS | L.CONV_LRELU, 1.0, 1.0, 1.0, 1.0, SLOPE)
    d.cout_groups, d.s2d_in_channels, d.s2d_out_channels = groups, s2d_in, s2d_out
    if dtype == L.RESR_F16X2:
        d.in0_lo_offset, d.out_lo_offset = n * h * w * cin, n * h * w * 64 * groups
    if extra == "mx":      # everything RESR_CONV_MX_PAIRS itself asks for is there: the hint alone is what is refused
        d.flags |= L.CONV_MX_PAIRS
        d.in0_q_offset, d.w_mx_offset = 2 * n * h * w * cin, 8 * 9 * 2 * 1024 * 6
    rc, ids = profiled(L, lambda: L.lib().resr_conv3x3(C.byref(d), L.ptr(x), None, L.ptr(packed), None, None, None, None, L.ptr(out.body),
                                                       None, L.stream_ptr()))
    assert rc == L.RESR_ERR_ARG and text in L.lib().resr_last_error().decode(), (name, rc, L.lib().resr_last_error())
    assert ids == [], (name, ids)
    torch.cuda.synchronize()
    assert (out.t.view(out.idt) == out.sent).all(), "a refused descriptor wrote its output"


# ---- the weight gradient ----------------------------------------------------------------------------------------------------------
WG_CASES = [
    # name, C = x_s2d_c, cout, (n, h, w) of G
    ("c32_1x1x1", 32, 64, (1, 1, 1)),                   # the job-table launch: 4 chunks x 2 G tiles = 8 products
    ("c32_1x1x5", 32, 64, (1, 1, 5)),
    ("c32_1x9x33", 32, 64, (1, 9, 33)),
    ("c64_layer_2x17x40", 64, 128, (2, 17, 40)),        # cout_pad > 64: layer mode
    ("c96_1x9x33", 96, 64, (1, 9, 33)),                 # three chunks per sub-position
]
WG_SCALE = 0.5


def _wgrad_launch(U, dtype, xo, go, n, h, w, cin, cout, splits, x_s2d_c):
    """dW [cout, cin, 3, 3] of one launch between guards (f32 with cout > 64: one launch per 64-channel group of G, as strict mode
    issues them -- the job-table launch takes cout_pad 32 or 64 and f32 has no layer mode), and the kernel ids."""
    L = U.L
    lib = L.lib()
    dw = Guarded(cout * cin * 9, torch.float32)
    step = 64 if dtype == L.RESR_F32 and cout > 64 else cout
    ids = []
    for q in range(cout // step):
        d = L.WgradDesc(n, h, w, cin, cin, cin, 0, cin, step, step, cout, dtype, 0, splits, WG_SCALE)
        d.x_lo_offset, d.g_lo_offset = xo.lo_offset, go.lo_offset
        partial = torch.empty(lib.resr_wgrad_partial_bytes(C.byref(d)) // 4, device="cuda")
        args = (C.byref(d), L.ptr(xo.t), None, U.sptr(go.t.reshape(-1), q * step), L.ptr(partial), U.sptr(dw.body, q * step * cin * 9), None)
        if x_s2d_c:
            rc, k = profiled(L, lambda: lib.resr_debug_conv3x3_wgrad_s2d(*args, x_s2d_c, L.stream_ptr()))
        else:
            rc, k = profiled(L, lambda: lib.resr_conv3x3_wgrad(*args, L.stream_ptr()))
        L.check(rc, "wgrad")
        torch.cuda.synchronize()
        ids += k
    return dw.read().reshape(cout, cin, 3, 3), ids


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("dtype_name", ["f16", "exact16", "f32"])
@pytest.mark.parametrize("case", WG_CASES, ids=[c[0] for c in WG_CASES])
def test_wgrad_sparse(U, case, dtype_name, splits):
    """dW4[co,c,ky,kx] = scale * sum_p g[co,p] * xpad[c, 2p + k - 1] through resr_debug_conv3x3_wgrad_s2d on the space-to-depth image of
    x, then resr_fold4x4; no db.  Three judgements per launch:
      * the folded [cout,C,4,4] result against the float64 4x4 gradient;
      * the raw [cout,4C,3,3] tensor at the 16 live (tap, sub-position) blocks against the float64 dense 3x3 gradient over the s2d image;
      * the 20 skipped blocks.  What csrc/wgrad.hip leaves there: ZEROS.  The quad kernel's skipped taps never touch their
        accumulators, it writes all nine taps of every slab all the same, and the reduction kernels store every element of
        [cout,cin,3,3] -- so a destination filled with a sentinel comes back fully written, with 0.0 in those blocks (f16, exact16).
        f32 ignores the hint (xsub = 4): there the whole raw tensor is the dense gradient, and is judged as such.
    The same operands through resr_conv3x3_wgrad (x_s2d_c = 0) pass the first two judgements too."""
    L = U.L
    dtype = _dt(L, dtype_name)
    name, c, cout, (n, h, w) = case
    g = _gen("wg_" + name)
    x = torch.randn(n, c, 2 * h, 2 * w, generator=g)
    gy = torch.randn(n, cout, h, w, generator=g)
    xo, go = Operand(L, R.s2d(x), dtype, 4 * c), Operand(L, gy, dtype, cout)
    xs, gv = xo.value, go.value
    xv = R.d2s(xs)
    lolo = dtype == L.RESR_F16X2
    ref4, ref4_32 = R.wgrad4x4s2(xv, gv, WG_SCALE, F64), R.wgrad4x4s2(xv, gv, WG_SCALE, F32)
    ref3, ref3_32 = R.wgrad(xs, gv, WG_SCALE, F64)[0], R.wgrad(xs, gv, WG_SCALE, F32)[0]
    extra4 = R.wgrad4x4s2(xv.abs(), gv.abs(), WG_SCALE, F64) * 2.0 ** -22 if lolo else None
    extra3 = R.wgrad_lolo(xs, gv, WG_SCALE) if lolo else None
    live = R.live_mask(c)
    for hint in (c, 0):
        tag = f"wgrad_{name}_s{splits}_{dtype_name}" + ("" if hint else "_nohint")
        path = "wgrad" if hint and dtype != L.RESR_F32 else "wgrad_dense"
        raw, ids = _wgrad_launch(U, dtype, xo, go, n, h, w, 4 * c, cout, splits, hint)
        if dtype != L.RESR_F32:      # the quad kernel (table mode 50200 / 50500, layer mode 50200: csrc/wgrad.hip prof_after) -- the one with the xsub path
            assert ids and all(k in (50200, 50500) for k in ids), ids
        dw4, raw_d = Guarded(cout * c * 16, torch.float32), raw.cuda()
        L.check(L.lib().resr_fold4x4(L.ptr(raw_d), L.ptr(dw4.body), cout, c, L.stream_ptr()), "resr_fold4x4")
        judge(tag + "_folded", dtype_name, path, dw4.read().reshape(cout, c, 4, 4), ref4, ref4_32, "f32", extra4)
        judge(tag + "_live", dtype_name, path, raw[:, live], ref3[:, live], ref3_32[:, live], "f32", extra3[:, live] if lolo else None)
        if hint and dtype != L.RESR_F32:
            assert (raw[:, ~live] == 0).all(), "a skipped (tap, sub-position) block holds something other than zero"
        else:
            judge(tag + "_rest", dtype_name, path, raw[:, ~live], ref3[:, ~live], ref3_32[:, ~live], "f32", extra3[:, ~live] if lolo else None)


def test_wgrad_s2d_refusals(U):
    """x_s2d_c that is no positive multiple of 32, or cin != 4 * x_s2d_c: the argument error, nothing launched, dW untouched."""
    L = U.L
    n, h, w, cin, cout = 1, 4, 8, 128, 64
    x = torch.zeros(n * h * w * cin, dtype=torch.float16, device="cuda")
    gy = torch.zeros(n * h * w * cout, dtype=torch.float16, device="cuda")
    d = L.WgradDesc(n, h, w, cin, cin, cin, 0, cin, cout, cout, cout, L.RESR_F16, 0, 1, 1.0)
    partial = torch.empty(L.lib().resr_wgrad_partial_bytes(C.byref(d)) // 4, device="cuda")
    dw = Guarded(cout * cin * 9, torch.float32)
    for bad in (0, -32, 16, 48, 64):
        rc, ids = profiled(L, lambda: L.lib().resr_debug_conv3x3_wgrad_s2d(C.byref(d), L.ptr(x), None, L.ptr(gy), L.ptr(partial), L.ptr(dw.body),
                                                                           None, bad, L.stream_ptr()))
        assert rc == L.RESR_ERR_ARG and ids == [], (bad, rc, ids)
    torch.cuda.synchronize()
    assert (dw.t.view(dw.idt) == dw.sent).all()
