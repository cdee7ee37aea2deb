"""-m gpu parity tests of the individual kernels, through the C-ABI, on seeded inputs.

How a convolution or weight-gradient result is judged (test_conv3x3*, test_wgrad*, the torch comparison of
test_output_groups_with_bias_equal_one_launch_per_group) -- the "sums rule" of tests/test_gpu_disc_helpers.py, extended by the
store's rounding; implemented once in tests/conv_ref.py (validated on the CPU by tests/test_conv_ref.py):
  * the reference is the float64 evaluation of the definition in include/resr.h (tests/conv_ref.py) on exactly the values the
    kernel is given: operands after gpu_util.quant (exact16: hi + lo / 4096), the weights handed to resr_pack_weights (f16: their
    f16 rounding), scalars as float32.
  * e32 = max over the tensor of |ref32 - ref64|, ref32 = the CPU fp32 evaluation of the same reference on the same inputs;
    A = max(4 * e32, one fp32 ulp of max |ref64|).  The factor 4 covers another summation order, nothing else.
  * fp32 outputs (f32 NHWC, any NCHW output, dW, db): every element has |got - ref64| <= A.
  * f16 outputs: every element has |got - ref64| <= A + max(2^-11 * 1.01 * |ref64|, 2^-24): half an ulp of EACH element (the f16
    subnormal spacing as a floor), not of the tensor's maximum.
  * exact16 pair outputs and exact16 fp32 NCHW outputs: joined in float64, every element within 2e-6 * max(1, max |ref64|), as
    test_conv_reads_single_chunks_and_writes_single_output (tests/test_gpu_x2_plan.py) judges its pair case ("pair": e32 and A play no
    part, so the exact16-only tests do not compute the fp32 yardstick); an exact16 output stored as its hi tensor alone
    (RESR_CONV_OUT_SINGLE): that bound + half an f16 ulp of the element ("pair16").
  * every stored exact16 pair: |lo| / 4096 <= 1.01 * max(2^-11 * |hi|, 2^-25) -- lo is a remainder of hi (conv_ref.pair_lo_excess).
  * exact16 dW: every element within A + 2^-22 * scale * wgrad(|X|, |G|)[element] (conv_ref.wgrad_lolo: the worst case of the dropped
    X_lo^T G_lo product; A from the plain fp32 evaluation on the pair values); exact16 db: within A.  With RESR_CONV_OUT_SINGLE G is
    its hi tensor, in the reference too.
  * sign words equal (stored > 0) exactly (a pair: hi + lo / 4096; a single-f16 output: its hi tensor).
  * the RESR_CONV_CLAMP01 pass-mask may differ from the reference's only where the reference's pre-clamp value lies within A (exact16:
    within the pair bound) of 0 or 1.
  * RESR_CONV_AUX_BEFORE_MASK / _RES: the aux tensor against conv_ref.epilogue's value at that point, by its dtype's rule, like out.
What runs as a single exact16 pass: the compact net's passes (test_conv3x3_prelu, test_conv3x3_cin3_forward, test_conv3x3_nchw_tail),
every epilogue form of launch_ws, partial cout tiles, pair / single chunks across two segments, chunk-planar operands and 16-row tiles
(test_exact16_conv_pass), the aux-before forms (test_aux_before_forms, all three dtypes), the job-table weight gradients
(test_exact16_wgrad*) and the layer-mode ones (test_wgrad_layer_mode_exact16).  Outputs of these tests lie between guards: every
element in range written, nothing outside it -- the channels between cout and the pixel stride and the gap between a pair's halves
included.
Every judgement is written to <diag_dir>/test_gpu_conv_kernels.json: case, cpu32_err, allowance, kernel_err, ratio (the re-runs
of the fallback kernels in a subprocess add theirs under their knob's name).  Everything else here compares against plain fp32
torch on the CPU."""
import ctypes as C
import json
import os

import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as R

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
DIAG = {}
_KNOBS = ("RESR_CONV_ONE_ROLE", "RESR_WGRAD_PAIR_KERNEL", "RESR_WGRAD_GENERIC_ADDR")
VARIANT = "+".join(k for k in _KNOBS if os.environ.get(k))   # "" in the main run; the subprocess re-runs carry their knobs


@pytest.fixture(scope="module")
def U():
    import tests.gpu_util as U
    return U


@pytest.fixture(scope="module", autouse=True)
def _write_diag(diag_dir):
    import tests.gpu_util as U
    if not VARIANT:
        U.merge_conv_diag(diag_dir, {}, restart=True)   # the main run starts the file, its re-runs (which end before it does) add to it
    yield
    U.merge_conv_diag(diag_dir, DIAG)


def judge(case, dtype_name, got, ref64, ref32, kind, extra=None):
    """The rule of the module docstring; returns the allowance (A, or the tensor bound of a pair).  extra: tests/conv_ref.wgrad_lolo."""
    rec = R.judge(got, ref64, ref32, kind, extra)
    rec.update(dtype=dtype_name, kind=kind)
    name = (VARIANT + "/" if VARIANT else "") + case
    DIAG[name] = rec
    print(f"{name}: cpu32_err {rec['cpu32_err']:.3e} allowance {rec['allowance']:.3e} kernel_err {rec['kernel_err']:.3e} "
          f"ratio {rec['ratio']:.3f} bad {rec['bad']} worst element {rec['worst']}: got {rec['got']!r} want {rec['want']!r}")
    assert rec["bad"] == 0, (name, rec)
    return rec["allowance"]


def refs(x, wt, up=False, **epi):
    """(ref64, its pre-clamp value, ref32) of one pass."""
    r64, pre = R.conv3x3(x, wt, F64, up, **epi)
    return r64, pre, R.conv3x3(x, wt, F32, up, **epi)[0]


def test_tr_probe(U, diag_dir):
    out = torch.zeros(256, device="cuda")
    U.L.check(U.L.lib().resr_debug_tr_probe(U.L.ptr(out), U.L.stream_ptr()))
    got = out.cpu().view(64, 4).long()
    with open(os.path.join(diag_dir, "tr_probe.json"), "w") as f:
        json.dump(got.tolist(), f)
    # assumed semantics (wgrad.hip): within a 16-lane group whose lanes point at consecutive
    # 8-byte pieces of a row-major [4][16] block, lane n receives column n: elements n + 16*j
    exp = torch.tensor([[(l & 15) + 16 * j + (l >> 4) * 64 for j in range(4)] for l in range(64)])
    assert torch.equal(got, exp), got[:20].tolist()


CONV_CASES = [
    # name, cin, cin0, cout, flags(str), n, h, w
    ("rdb_conv1", 64, 64, 32, "lrelu", 2, 19, 45),
    ("rdb_conv3_2seg", 128, 64, 32, "lrelu", 1, 33, 32),
    ("rdb_conv5_res", 192, 192, 64, "res0,res1", 2, 16, 70),
    ("up_conv", 64, 64, 64, "lrelu,up", 1, 36, 40),
    ("conv4_nchw", 64, 64, 3, "nchw,clamp", 2, 21, 37),
    ("dgrad_mask", 96, 64, 32, "mask,nobias,res0", 1, 17, 64),
    ("big_tiles", 64, 64, 32, "lrelu", 1, 256, 64),
    # fast-mode persistent kernel: more tiles than resident workgroups (several tiles per workgroup), and the
    # epilogue kinds it instantiates (mask only / residual 0 only / two-segment input with 5 chunks)
    ("persist_multi", 64, 64, 32, "lrelu", 4, 320, 256),
    ("persist_multi64", 64, 64, 64, "lrelu", 2, 272, 256),
    ("mask_only", 64, 64, 64, "mask,nobias", 1, 40, 72),
    ("res0_only", 192, 192, 64, "res0", 1, 33, 40),
    ("two_seg_5chunks", 160, 64, 32, "lrelu", 1, 50, 33),
    # 1-bit LeakyReLU masks: a forward pass emits the sign tensor, the backward-data pass reads it instead of the activation
    ("signbits32", 64, 64, 32, "lrelu,signbits", 2, 37, 45),
    ("signbits64", 96, 96, 64, "lrelu,signbits", 1, 40, 70),
    ("maskbits32", 128, 64, 32, "mask,nobias,maskbits", 1, 33, 64),
    ("maskbits64", 64, 64, 64, "mask,nobias,maskbits", 2, 20, 36),
    # 16-row tile shapes (three halo buffers for cout <= 32) with ragged last tile row / column and several tiles per workgroup
    ("rows16_ragged32", 96, 96, 32, "lrelu,signbits", 8, 200, 200),
    ("rows16_ragged64", 64, 64, 64, "res0", 8, 200, 200),
    ("rows16_maskbits_2seg", 160, 64, 32, "mask,nobias,maskbits", 6, 184, 216),
    # partial output tiles of the lean epilogue: 8-channel pieces beyond cout are neither read nor stored
    ("cout8", 64, 64, 8, "lrelu", 1, 20, 40),
    ("cout16", 96, 96, 16, "lrelu", 2, 18, 34),
    ("cout24", 64, 64, 24, "lrelu", 1, 33, 32),
    ("cout48", 64, 64, 48, "lrelu", 1, 20, 36),
    ("cout24_res", 64, 64, 24, "res0", 1, 17, 40),      # residual with cout % 16 != 0: the general epilogue
    ("cout48_res", 64, 64, 48, "res0,res1", 1, 17, 40),
]


@pytest.mark.parametrize("dtype_name", ["f32", "f16"])
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv3x3(U, case, dtype_name):
    L = U.L
    dtype = L.RESR_F16 if dtype_name == "f16" else L.RESR_F32
    name, cin, cin0, cout, fl, n, h, w = case
    fl = set(fl.split(","))
    g = torch.Generator().manual_seed(hash(name) % 1000)
    hs, ws = (h // 2, w // 2) if "up" in fl else (h, w)
    x = U.quant(torch.randn(n, cin, hs, ws, generator=g), dtype)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    cout_pad = (cout + 31) // 32 * 32
    # two-segment input: channels [0,cin0) in tensor A (stride cin0+32, offset 0), rest in tensor B
    a = U.to_nhwc(x[:, :cin0], dtype, stride=cin0 + 32)
    b = U.to_nhwc(x[:, cin0:], dtype, stride=cin - cin0 + 64, offset=32) if cin0 < cin else None
    packed = U.pack_conv(wt, dtype)
    flags = 0
    d = L.ConvDesc(n, h, w, cin, cin0, cin0 + 32, (cin - cin0 + 64) if b is not None else 0, cout, cout_pad,
                   cout_pad + 32, 0, 0, 0, dtype, 0, 1.0, 1.0, 1.0, 1.0, 0.2)
    epi = {"slope": 0.2}                      # the reference's epilogue arguments (tests/conv_ref.py)
    if "nobias" not in fl:
        epi["bias"] = bias
    res0 = res1 = mask = None
    if "up" in fl:
        flags |= L.CONV_UPSAMPLE_IN
    if "nobias" in fl:
        flags |= L.CONV_NO_BIAS
    if "mask" in fl:
        mk = U.quant(torch.randn(n, cout, h, w, generator=g), dtype)
        if "maskbits" in fl:   # sign tensor: uint32 [pixels][cout/32], bit c of word m = (mask[32m + c] > 0)
            bits = (mk > 0).permute(0, 2, 3, 1).reshape(n, h, w, cout // 32, 32).to(torch.int64)
            words = (bits << torch.arange(32)).sum(-1)
            mask = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).cuda().contiguous()
            flags |= L.CONV_MASK_BITS
        else:
            mask = U.to_nhwc(mk, dtype, stride=cout + 32)
            d.mask_stride = cout + 32
        flags |= L.CONV_MASK
        epi["mask"] = mk
    if "lrelu" in fl:
        flags |= L.CONV_LRELU
        epi["lrelu"] = True
    if "res0" in fl:
        r0 = U.quant(torch.randn(n, cout, h, w, generator=g), dtype)
        res0 = U.to_nhwc(r0, dtype, stride=cout + 64)
        d.res0_stride, d.s0, d.t0 = cout + 64, 0.2, 1.0
        epi.update(res0=r0, s0=0.2, t0=1.0)
    if "res1" in fl:
        r1 = U.quant(torch.randn(n, cout, h, w, generator=g), dtype)
        res1 = U.to_nhwc(r1, dtype, stride=cout)
        d.res1_stride, d.s1, d.t1 = cout, 0.2, 0.5
        epi.update(res1=r1, s1=0.2, t1=0.5)
    aux = None
    if "nchw" in fl:
        flags |= L.CONV_OUT_NCHW_F32
        out = torch.full((n, cout, h, w), -7.0, device="cuda")
        if "clamp" in fl:
            flags |= L.CONV_CLAMP01
            aux = torch.full((n, cout, h, w), 9, dtype=torch.uint8, device="cuda")
            epi["clamp"] = True
    else:
        out = torch.full((n, h, w, cout_pad + 32), -7.0, dtype=U.tdtype(dtype), device="cuda")
    if "signbits" in fl:
        flags |= L.CONV_WRITE_SIGNBITS
        aux = torch.zeros((n, h, w, cout_pad // 32), dtype=torch.int32, device="cuda")
    d.flags = flags
    bias_d = bias.cuda()
    L.check(L.lib().resr_conv3x3(C.byref(d), L.ptr(a), L.ptr(b) if b is None else U.sptr(b, 32), L.ptr(packed),
                                 L.ptr(bias_d), L.ptr(res0), L.ptr(res1), L.ptr(mask), L.ptr(out), L.ptr(aux),
                                 L.stream_ptr()), "resr_conv3x3")
    torch.cuda.synchronize()
    if "nchw" in fl:
        got = out.cpu()
    else:
        got = U.from_nhwc(out, cout)
        assert (out[..., cout_pad:].float() == -7.0).all(), "wrote outside its channel slice"
    ref, pre, ref32 = refs(x, U.quant(wt, dtype), "up" in fl, **epi)
    A = judge(f"conv_{name}_{dtype_name}", dtype_name, got, ref, ref32, "f32" if "nchw" in fl else dtype_name)
    if "signbits" in fl:
        words = aux.cpu().to(torch.int64) & 0xFFFFFFFF
        got_bits = ((words.unsqueeze(-1) >> torch.arange(32)) & 1).reshape(n, h, w, cout_pad)[..., :cout].permute(0, 3, 1, 2).bool()
        assert torch.equal(got_bits, got > 0), "sign tensor disagrees with the stored activation"
    elif aux is not None:
        # the pass-mask may differ only where the reference's pre-clamp value is within A of 0 or 1
        assert set(aux.unique().tolist()) <= {0, 1}, "pass-mask bytes never written, or not 0 / 1"
        assert R.pass_mask_ok(aux.cpu(), pre, A) == 0


PLANAR_CASES = [
    # name, cin, cout, residual, n, h, w -- operands laid out chunk-planar [C/32][N,H,W,32] as the generator's workspaces are
    ("planar_rdb_conv3", 128, 32, False, 5, 120, 100),
    ("planar_rdb_conv5", 192, 64, True, 3, 100, 72),
    ("planar_small", 64, 32, False, 1, 20, 24),
]


@pytest.mark.parametrize("dtype_name", ["f32", "f16"])
@pytest.mark.parametrize("case", PLANAR_CASES, ids=[c[0] for c in PLANAR_CASES])
def test_conv3x3_chunk_planar(U, case, dtype_name):
    """`ResrConvDesc.*_chunk_stride`: input, output, residual and the emitted sign tensor in the chunk-planar layout
     -- the addressing every dense-block pass of the generator uses."""
    L = U.L
    dtype = L.RESR_F16 if dtype_name == "f16" else L.RESR_F32
    name, cin, cout, with_res, n, h, w = case
    g = torch.Generator().manual_seed(len(name))
    x = U.quant(torch.randn(n, cin, h, w, generator=g), dtype)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1

    def planar(t):   # [N,C,H,W] cpu -> [C/32][N,H,W,32] device
        nn_, c, hh, ww = t.shape
        return t.reshape(nn_, c // 32, 32, hh, ww).permute(1, 0, 3, 4, 2).contiguous().to(U.tdtype(dtype)).cuda()

    def unplanar(t, c):
        return t.float().cpu().permute(1, 0, 4, 2, 3).reshape(n, c, h, w)

    plane = n * h * w * 32
    xin = planar(x)
    out = torch.full((cout // 32, n, h, w, 32), -7.0, dtype=U.tdtype(dtype), device="cuda")
    d = L.ConvDesc(n, h, w, cin, cin, 32, 0, cout, cout, 32, 0, 0, 0, dtype, 0, 1.0, 1.0, 1.0, 1.0, 0.2)
    d.in0_chunk_stride = plane
    d.out_chunk_stride = plane
    epi = {"bias": bias, "slope": 0.2}
    res0 = aux = None
    if with_res:
        r0 = U.quant(torch.randn(n, cout, h, w, generator=g), dtype)
        res0 = planar(r0)
        d.res0_stride, d.res0_chunk_stride, d.s0, d.t0 = 32, plane, 0.2, 1.0
        epi.update(res0=r0, s0=0.2, t0=1.0)
        d.flags = 0
    else:
        epi["lrelu"] = True
        aux = torch.zeros((n, h, w, cout // 32), dtype=torch.int32, device="cuda")
        d.flags = L.CONV_LRELU | L.CONV_WRITE_SIGNBITS
    packed = U.pack_conv(wt, dtype)
    bias_d = bias.cuda()
    L.check(L.lib().resr_conv3x3(C.byref(d), L.ptr(xin), None, L.ptr(packed), L.ptr(bias_d), L.ptr(res0), None, None,
                                 L.ptr(out), L.ptr(aux), L.stream_ptr()), "resr_conv3x3")
    torch.cuda.synchronize()
    got = unplanar(out, cout)
    ref, _, ref32 = refs(x, U.quant(wt, dtype), **epi)
    judge(f"conv_{name}_{dtype_name}", dtype_name, got, ref, ref32, dtype_name)
    if aux is not None:
        words = aux.cpu().to(torch.int64) & 0xFFFFFFFF
        bits = ((words.unsqueeze(-1) >> torch.arange(32)) & 1).reshape(n, h, w, cout).permute(0, 3, 1, 2).bool()
        assert torch.equal(bits, got > 0), "sign tensor disagrees with the stored activation"


def test_conv3x3_one_role_and_wgrad_pair_kernel_fallbacks():
    """The register-staged f16 conv kernel (used when the producer/consumer kernel's preconditions fail) and the f16 weight-gradient
    pair kernel (used when the quad kernel's grouping fails) stay correct: re-run the f16 conv cases and the wgrad cases in ONE
    subprocess with RESR_CONV_ONE_ROLE=1 and RESR_WGRAD_PAIR_KERNEL=1 (the knobs are read once per process; one interpreter start-up
    instead of two: the suite's time box)."""
    import subprocess, sys
    env = dict(os.environ, RESR_CONV_ONE_ROLE="1", RESR_WGRAD_PAIR_KERNEL="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_kernels.py"), "-q", "-x", "-m", "gpu",
                        "-k", "(test_conv3x3 and f16 and not fallback and not persist) or (test_wgrad and not fallback and not layer)"], env=env, cwd=root,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def judge_wgrad(case, dtype_name, dw, db, x, gy, scale, up, lolo=False):
    """dW and db of one launch against tests/conv_ref.wgrad on the values the kernel was given (both are fp32 outputs).  lolo: the
    exact16 rule -- dW's bound is A + conv_ref.wgrad_lolo, the worst case of the dropped X_lo^T G_lo product."""
    ref_w, ref_b = R.wgrad(x, gy, scale, F64, up)
    w32, b32 = R.wgrad(x, gy, scale, F32, up)
    judge(case + "_dW", dtype_name, dw.cpu(), ref_w, w32, "f32", R.wgrad_lolo(x, gy, scale, up) if lolo else None)
    judge(case + "_db", dtype_name, db.cpu(), ref_b, b32, "f32")


WGRAD_CASES = [
    ("w_64_32", 64, 32, 0, 2, 19, 45),
    ("w_192_64", 192, 64, 0, 1, 24, 40),
    ("w_up", 64, 64, 1, 1, 16, 64),
    ("w_cout3", 64, 3, 0, 1, 17, 33),
    ("w_cin3", 3, 64, 0, 2, 12, 36),
    ("w_160_32", 160, 32, 0, 1, 21, 70),      # odd chunk count: 2 full quad jobs + a half one
    ("w_many_tiles", 64, 64, 0, 3, 40, 96),   # several tiles per workgroup (double-buffer reuse)
]


@pytest.mark.parametrize("dtype_name", ["f32", "f16"])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_wgrad(U, case, dtype_name):
    L = U.L
    dtype = L.RESR_F16 if dtype_name == "f16" else L.RESR_F32
    name, cin, cout, up, n, h, w = case
    g = torch.Generator().manual_seed(7)
    hs, ws = (h // 2, w // 2) if up else (h, w)
    x = U.quant(torch.randn(n, cin, hs, ws, generator=g), dtype)
    gy = U.quant(torch.randn(n, cout, h, w, generator=g), dtype)
    cin_pad, cout_pad = (cin + 31) // 32 * 32, (cout + 31) // 32 * 32
    xb = U.to_nhwc(x, dtype, c_pad=cin_pad, stride=cin_pad + 32)
    gb = U.to_nhwc(gy, dtype, c_pad=cout_pad, stride=cout_pad + 32)
    splits = 3
    d = L.WgradDesc(n, h, w, cin_pad, cin_pad, cin_pad + 32, 0, cin, cout, cout_pad, cout_pad + 32, dtype,
                    L.CONV_UPSAMPLE_IN if up else 0, splits, 0.5)
    nbytes = L.lib().resr_wgrad_partial_bytes(C.byref(d))
    partial = torch.empty(nbytes // 4, device="cuda")
    dw = torch.full((cout, cin, 3, 3), -7.0, device="cuda")
    db = torch.full((cout,), -7.0, device="cuda")
    L.check(L.lib().resr_conv3x3_wgrad(C.byref(d), L.ptr(xb), None, L.ptr(gb), L.ptr(partial), L.ptr(dw), L.ptr(db),
                                       L.stream_ptr()), "resr_conv3x3_wgrad")
    torch.cuda.synchronize()
    judge_wgrad(f"wgrad_{name}_{dtype_name}", dtype_name, dw, db, x, gy, 0.5, up)


LAYER_CASES = [
    ("layer_odd", 352, 288, 0, 2, 16, 40, 3),        # 11 chunks x 9 tiles = 99 products: odd counts (half-filled quad jobs on both edges)
    ("layer_wide", 512, 256, 0, 4, 16, 32, 2),       # the discriminator's 512 -> 256 layer: 128 products, two pixel splits
    ("layer_up_bias", 128, 200, 1, 1, 24, 64, 12),   # cout not a multiple of 32 (rows of the last tile masked), upsampled input, > 8 splits
]


@pytest.mark.parametrize("case", LAYER_CASES, ids=[c[0] for c in LAYER_CASES])
def test_wgrad_layer_mode(U, case):
    """Weight gradients in layer mode (wgrad.hip WgradLayer: an output wider than 64 channels or more than 80 products; quad jobs and
    slabs from the grid position, work spread over all XCDs, <= 8 splits through the wide reduction) through the public entry
    against float64 (the rule of the module docstring)."""
    L = U.L
    dtype = L.RESR_F16
    name, cin, cout, up, n, h, w, splits = case
    g = torch.Generator().manual_seed(11)
    hs, ws = (h // 2, w // 2) if up else (h, w)
    x = U.quant(torch.randn(n, cin, hs, ws, generator=g), dtype)
    gy = U.quant(torch.randn(n, cout, h, w, generator=g), dtype)
    cin_pad, cout_pad = (cin + 31) // 32 * 32, (cout + 31) // 32 * 32
    xb = U.to_nhwc(x, dtype, c_pad=cin_pad, stride=cin_pad + 32)
    gb = U.to_nhwc(gy, dtype, c_pad=cout_pad, stride=cout_pad + 32)
    d = L.WgradDesc(n, h, w, cin_pad, cin_pad, cin_pad + 32, 0, cin, cout, cout_pad, cout_pad + 32, dtype,
                    L.CONV_UPSAMPLE_IN if up else 0, splits, 1.0)
    partial = torch.empty(L.lib().resr_wgrad_partial_bytes(C.byref(d)) // 4, device="cuda")
    dw = torch.full((cout, cin, 3, 3), -7.0, device="cuda")
    db = torch.full((cout,), -7.0, device="cuda")
    L.check(L.lib().resr_conv3x3_wgrad(C.byref(d), L.ptr(xb), None, L.ptr(gb), L.ptr(partial), L.ptr(dw), L.ptr(db), L.stream_ptr()),
            "resr_conv3x3_wgrad")
    torch.cuda.synchronize()
    judge_wgrad(f"wgrad_{name}", "f16", dw, db, x, gy, 1.0, up)


@pytest.mark.parametrize("products", [3, 1])
@pytest.mark.parametrize("case", LAYER_CASES, ids=[c[0] for c in LAYER_CASES])
def test_wgrad_layer_mode_exact16(U, case, products, diag_dir):
    """Layer mode on RESR_F16X2 operands ((hi, lo) f16 pairs, value = hi + lo * 2^-12): the three tap-products (hi, hi), (hi, lo),
    (lo, hi) of every product as three rounds of quad jobs with their own slab regions, combined by the reduction -- fp32-class
    gradients against a float64 autograd of the SAME fp32 inputs (1e-3 is the path's tolerance; measured ~1e-6); with
    RESR_X2_WGRAD_PRODUCTS=1 (hi tensors only) the f16-class error of one rounding per operand."""
    L = U.L
    name, cin, cout, up, n, h, w, splits = case
    g = torch.Generator().manual_seed(12)
    hs, ws = (h // 2, w // 2) if up else (h, w)
    x = torch.randn(n, cin, hs, ws, generator=g)
    gy = torch.randn(n, cout, h, w, generator=g)
    cin_pad, cout_pad = (cin + 31) // 32 * 32, (cout + 31) // 32 * 32

    def pair(t, c_pad):          # [2][n,h,w,stride] f16: the hi tensor, directly behind it the lo tensor
        hi = t.half()
        lo = ((t - hi.float()) * 4096.0).half()
        stride = c_pad + 32
        buf = torch.zeros(2, t.shape[0], t.shape[2], t.shape[3], stride, dtype=torch.float16, device="cuda")
        buf[0, ..., :t.shape[1]] = hi.permute(0, 2, 3, 1).cuda()
        buf[1, ..., :t.shape[1]] = lo.permute(0, 2, 3, 1).cuda()
        value = hi.double() + lo.double() / 4096.0
        return buf, buf[0].numel(), value
    xb, x_lo, xv = pair(x, cin_pad)
    gb, g_lo, gv = pair(gy, cout_pad)
    d = L.WgradDesc(n, h, w, cin_pad, cin_pad, cin_pad + 32, 0, cin, cout, cout_pad, cout_pad + 32, L.RESR_F16X2,
                    L.CONV_UPSAMPLE_IN if up else 0, splits, 1.0)
    d.x_lo_offset, d.g_lo_offset = x_lo, g_lo
    os.environ["RESR_X2_WGRAD_PRODUCTS"] = str(products)
    try:
        partial = torch.empty(L.lib().resr_wgrad_partial_bytes(C.byref(d)) // 4, device="cuda")
        dw = torch.full((cout, cin, 3, 3), -7.0, device="cuda")
        db = torch.full((cout,), -7.0, device="cuda")
        L.check(L.lib().resr_conv3x3_wgrad(C.byref(d), L.ptr(xb), None, L.ptr(gb), L.ptr(partial), L.ptr(dw), L.ptr(db), L.stream_ptr()),
                "resr_conv3x3_wgrad")
        torch.cuda.synchronize()
    finally:
        os.environ.pop("RESR_X2_WGRAD_PRODUCTS", None)
    xin = F.interpolate(xv, scale_factor=2, mode="nearest") if up else xv
    wt = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    bs = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    (F.conv2d(xin, wt, bs, padding=1) * gv).sum().backward()
    rel_w = ((dw.cpu().double() - wt.grad).norm() / wt.grad.norm()).item()
    rel_b = ((db.cpu().double() - bs.grad).norm() / bs.grad.norm()).item()
    with open(os.path.join(diag_dir, f"wgrad_x2_{name}_{products}.json"), "w") as f:
        json.dump({"rel_w": rel_w, "rel_b": rel_b}, f)
    if products == 3:
        assert rel_w < 5e-6 and rel_b < 5e-6, (rel_w, rel_b)
        judge_wgrad(f"wgrad_x2_{name}", "exact16", dw, db, xv, gv, 1.0, up, lolo=True)     # and element by element
    else:
        assert 1e-5 < rel_w < 2e-3 and rel_b < 2e-3, (rel_w, rel_b)    # the hi-only form drops the 2^-12 terms: visibly coarser, still a gradient


@pytest.mark.parametrize("knob", ["RESR_WGRAD_GENERIC_ADDR"])
def test_wgrad_fallback_kernels(knob):
    """The f16 pair kernel's 64-bit addressing path (taken when the 32-bit addressing preconditions fail; with 32-bit addressing it
    runs in test_conv3x3_one_role_and_wgrad_pair_kernel_fallbacks) stays correct: re-run the wgrad cases in a subprocess with the
    knob set (read once per process)."""
    import subprocess, sys
    env = dict(os.environ, **{knob: "1"})
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_kernels.py"), "-q", "-x", "-m", "gpu",
                        "-k", "test_wgrad and not fallback and not layer"], env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_layout_and_pool(U):
    L = U.L
    g = torch.Generator().manual_seed(3)
    for dtype in (L.RESR_F32, L.RESR_F16):
        x = torch.rand(2, 3, 8, 12, generator=g)
        for r, cpad in ((1, 32), (2, 32), (4, 64)):
            dst = torch.full((2, 8 // r, 12 // r, cpad), -1.0, dtype=U.tdtype(dtype), device="cuda")
            xd = x.cuda()
            L.check(L.lib().resr_nchw_to_nhwc(L.ptr(xd), L.ptr(dst), 2, 3, 8, 12, r, cpad, dtype, None,
                                              L.stream_ptr()))
            torch.cuda.synchronize()
            ref = F.pixel_unshuffle(x, r) if r > 1 else x
            got = U.from_nhwc(dst, 3 * r * r)
            assert torch.allclose(got, U.quant(ref, dtype), atol=0), (r, dtype)
            assert (dst[..., 3 * r * r:] == 0).all()
            back = torch.empty(2, 3, 8, 12, device="cuda")
            L.check(L.lib().resr_nhwc_to_nchw(L.ptr(dst), L.ptr(back), 2, 3, 8, 12, r, cpad, dtype, L.stream_ptr()))
            assert torch.allclose(back.cpu(), U.quant(x, dtype), atol=0)
        src = U.quant(torch.randn(2, 64, 12, 20, generator=g), dtype)
        mk = U.quant(torch.randn(2, 64, 6, 10, generator=g), dtype)
        out = torch.empty(2, 6, 10, 64, dtype=U.tdtype(dtype), device="cuda")
        src_d, mk_d = U.to_nhwc(src, dtype), U.to_nhwc(mk, dtype)   # keep alive while the kernel runs
        L.check(L.lib().resr_sumpool2x2(L.ptr(src_d), L.ptr(out), L.ptr(mk_d), 2, 6, 10, 64, dtype, 0.2,
                                        L.stream_ptr()))
        torch.cuda.synchronize()
        ref = F.avg_pool2d(src, 2) * 4 * torch.where(mk > 0, 1.0, 0.2)
        assert (U.from_nhwc(out, 64) - ref).abs().max().item() < (2e-2 if dtype == L.RESR_F16 else 1e-5)


@pytest.mark.parametrize("n,c,h,w", [(128, 512, 4, 6), (2, 40, 70, 64), (1, 3, 300, 33), (1, 8, 66000, 2)])
def test_layout_helpers_beyond_the_grid_limits(U, n, c, h, w):
    """resr_nhwc_to_nchw with n * c > 65535 (128 x 512-channel feature maps), narrow images (several rows per workgroup) and
    h > 65535: rows / (image, channel) pairs beyond a grid dimension loop instead of failing."""
    L = U.L
    g = torch.Generator().manual_seed(7)
    src = torch.randn(n, h, w, c, generator=g).half().cuda()
    out = torch.full((n, c, h, w), -7.0, device="cuda")
    L.check(L.lib().resr_nhwc_to_nchw(L.ptr(src), L.ptr(out), n, c, h, w, 1, c, L.RESR_F16, L.stream_ptr()), "resr_nhwc_to_nchw")
    torch.cuda.synchronize()
    assert torch.equal(out, src.float().permute(0, 3, 1, 2))
    if c <= 32:   # and back (rows from the grid, strided)
        back = torch.full((n, h, w, 32), -1.0, dtype=torch.float16, device="cuda")
        L.check(L.lib().resr_nchw_to_nhwc(L.ptr(out), L.ptr(back), n, c, h, w, 1, 32, L.RESR_F16, None, L.stream_ptr()), "resr_nchw_to_nhwc")
        torch.cuda.synchronize()
        assert torch.equal(back[..., :c], src) and (back[..., c:] == 0).all()


def test_ema_bit_exact(U):
    L = U.L
    g = torch.Generator().manual_seed(5)
    p = torch.randn(100003, generator=g)
    s = torch.randn(100003, generator=g)
    sd, pd = s.cuda(), p.cuda()
    ref = s.clone()
    for _ in range(3):
        L.check(L.lib().resr_ema_update(L.ptr(sd), L.ptr(pd), sd.numel(), 0.999, L.stream_ptr()))
        ref = (1.0 - 0.999) * p + 0.999 * ref     # reference model.py:47
    assert torch.equal(sd.cpu(), ref)


# ---- fused scalar losses (csrc/loss.hip, losses.py): value + unit gradient in one launch -----------------------------------
@pytest.mark.parametrize("shape", [(16, 1, 64, 64), (3, 1, 17, 23), (1, 3, 5, 7)])
@pytest.mark.parametrize("label,weight", [(1.0, 0.1), (0.0, 1.0)])
def test_fused_bce_with_logits_const_vs_torch(shape, label, weight):
    """nn.BCEWithLogitsLoss against torch.full(..., label) (train_realesrgan.py:460-461,478,500,509): value, gradient (through a
    loss scale like GradScaler's), determinism, and the generic path for a non-stock criterion."""
    from real_esrgan_pytorch_amd import losses
    gen = torch.Generator().manual_seed(3)
    x = (torch.randn(*shape, generator=gen) * 4).cuda()
    x.view(-1)[:3] = torch.tensor([60.0, -60.0, 0.0]).cuda()              # saturated logits: no overflow in sigmoid / log1p
    crit = torch.nn.BCEWithLogitsLoss()
    xr = x.clone().requires_grad_(True)
    ref = weight * crit(xr, torch.full_like(xr, label))
    (ref * 512.0).backward()
    xf = x.clone().requires_grad_(True)
    got = losses.bce_with_logits_const(crit, xf, label, weight)
    (got * 512.0).backward()
    assert got.shape == () and abs(got.item() - ref.item()) <= 2e-6 * max(1.0, abs(ref.item()))
    assert (xf.grad - xr.grad).abs().max().item() <= 1e-6 * xr.grad.abs().max().item() + 1e-12
    again = losses.bce_with_logits_const(crit, x.clone().requires_grad_(True), label, weight)
    assert again.item() == got.item()                                        # fixed-order partial sums: bit-reproducible
    with torch.no_grad():
        assert abs(losses.bce_with_logits_const(crit, x, label, weight).item() - ref.item()) <= 2e-6 * max(1.0, abs(ref.item()))
    summed = losses.bce_with_logits_const(torch.nn.BCEWithLogitsLoss(reduction="sum"), x, label, weight)   # not the stock form: called as is
    assert abs(summed.item() - weight * torch.nn.functional.binary_cross_entropy_with_logits(x, torch.full_like(x, label), reduction="sum").item()) < 1e-2


@pytest.mark.parametrize("shape", [(16, 3, 256, 256), (2, 3, 33, 17)])
def test_fused_l1_mean_vs_torch(shape):
    from real_esrgan_pytorch_amd import losses
    gen = torch.Generator().manual_seed(4)
    a, b = torch.rand(*shape, generator=gen).cuda(), torch.rand(*shape, generator=gen).cuda()
    b.view(-1)[:5] = a.view(-1)[:5]                                           # ties: gradient 0 like ATen's sgn
    crit = torch.nn.L1Loss()
    ar = a.clone().requires_grad_(True)
    ref = 0.7 * crit(ar, b)
    (ref * 1024.0).backward()
    af = a.clone().requires_grad_(True)
    got = losses.l1_loss(crit, af, b, 0.7)
    (got * 1024.0).backward()
    assert abs(got.item() - ref.item()) <= 2e-6 * abs(ref.item())
    assert torch.equal(af.grad, ar.grad) or (af.grad - ar.grad).abs().max().item() <= 1e-6 * ar.grad.abs().max().item()
    bf = b.clone().requires_grad_(True)                                       # gradient wrt the second operand as well
    losses.l1_loss(crit, a, bf).backward()
    br = b.clone().requires_grad_(True)
    crit(a, br).backward()
    assert (bf.grad - br.grad).abs().max().item() <= 1e-6 * br.grad.abs().max().item()
    sm = losses.l1_loss(torch.nn.SmoothL1Loss(), a, b, 0.5)                   # not nn.L1Loss: the criterion is simply called
    assert abs(sm.item() - 0.5 * torch.nn.functional.smooth_l1_loss(a, b).item()) < 1e-6


@pytest.mark.parametrize("cin,cout,n,h,w", [(64, 128, 2, 24, 40), (128, 512, 4, 16, 16), (256, 256, 1, 33, 20)])
def test_output_groups_with_bias_equal_one_launch_per_group(cin, cout, n, h, w):
    """ResrConvDesc.cout_groups with a BIAS (VGG19's 128..512-channel layers, model.py:296-298, as one launch instead of one per
    64-channel group): bit-equal to the per-group launches, and right against float64 (the rule of the module docstring)."""
    import ctypes as C
    import torch.nn.functional as F
    from tests import gpu_util as U
    L = U.L
    lib = L.lib()
    g = torch.Generator().manual_seed(cin + cout + h)
    x = U.quant(torch.randn(n, cin, h, w, generator=g), L.RESR_F16)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    bias = torch.randn(cout, generator=g)
    xd = U.to_nhwc(x, L.RESR_F16)
    groups = cout // 64
    packed = torch.cat([U.pack_conv(wt[q * 64:(q + 1) * 64], L.RESR_F16)[:(cin // 32) * 9 * 2 * 1024 * 2] for q in range(groups)]
                       + [torch.zeros(16384, dtype=torch.uint8, device="cuda")])
    bd = bias.cuda()
    per_group = (cin // 32) * 9 * 2 * 1024 * 2          # bytes of one group's packed weights
    outs = []
    for grouped in (True, False):
        y = torch.zeros(n, h, w, cout, dtype=torch.float16, device="cuda")
        if grouped:
            d = L.ConvDesc(n, h, w, cin, cin, cin, 0, 64, 64, cout, 0, 0, 0, L.RESR_F16, L.CONV_LRELU, 1.0, 1.0, 1.0, 1.0, 0.0)
            d.cout_groups = groups
            L.check(lib.resr_conv3x3(C.byref(d), L.ptr(xd), None, L.ptr(packed), L.ptr(bd), None, None, None, L.ptr(y), None, L.stream_ptr()),
                    "resr_conv3x3")
        else:
            for q in range(groups):
                d = L.ConvDesc(n, h, w, cin, cin, cin, 0, 64, 64, cout, 0, 0, 0, L.RESR_F16, L.CONV_LRELU, 1.0, 1.0, 1.0, 1.0, 0.0)
                L.check(lib.resr_conv3x3(C.byref(d), L.ptr(xd), None, C.c_void_p(packed.data_ptr() + q * per_group), U.sptr(bd, q * 64), None, None,
                                         None, U.sptr(y, q * 64), None, L.stream_ptr()), "resr_conv3x3")
        torch.cuda.synchronize()
        outs.append(y)
    assert torch.equal(outs[0], outs[1])
    ref, _, ref32 = refs(x, U.quant(wt, L.RESR_F16), bias=bias, lrelu=True, slope=0.0)   # LeakyReLU with slope 0: ReLU
    judge(f"conv_groups_{cin}_{cout}_f16", "f16", U.from_nhwc(outs[0], cout), ref, ref32, "f16")
    # more groups with a bias than the kernel keeps in LDS: refused loudly, not computed wrongly
    d = L.ConvDesc(n, h, w, cin, cin, cin, 0, 64, 64, 64 * 9, 0, 0, 0, L.RESR_F16, L.CONV_LRELU, 1.0, 1.0, 1.0, 1.0, 0.0)
    d.cout_groups = 9
    assert lib.resr_conv3x3(C.byref(d), L.ptr(xd), None, L.ptr(packed), L.ptr(bd), None, None, None, L.ptr(outs[0]), None, L.stream_ptr()) != 0


# ---- the compact generator's kernel paths (csrc/compact.hip), one pass at a time ----------------------------------------------------
# (n, h, w): one pixel, one row, one column, a second tile that holds a single column, exact tile width, one short of it, and a ragged
# interior -- the smallest shapes at which tile seams, halo rows and ragged tails exist (tiles are 32 wide and 8, 16 or 32 high).
GEOMETRIES = [(1, 1, 1), (3, 1, 40), (2, 40, 1), (1, 2, 33), (2, 17, 32), (1, 33, 31), (1, 37, 53)]
GEO_IDS = ["x".join(map(str, g)) for g in GEOMETRIES]
GUARD = 64
SENT = {torch.float16: (torch.int16, 0x7E5A), torch.float32: (torch.int32, 0x7FC5A5A5)}   # NaN payloads no kernel produces


def _dtype(L, dtype_name):
    return {"f32": L.RESR_F32, "f16": L.RESR_F16, "exact16": L.RESR_F16X2}[dtype_name]


def _tdtype(L, dtype):
    return torch.float32 if dtype == L.RESR_F32 else torch.float16   # exact16 tensors are pairs of f16 tensors


class Guarded:
    """`count` elements between two guards of GUARD elements, everything pre-filled with a sentinel: the guards must survive and
    every element in range must have been written."""

    def __init__(self, count, tdtype):
        self.count, (self.idt, self.sent) = count, SENT[tdtype]
        self.t = torch.empty(count + 2 * GUARD, dtype=tdtype, device="cuda")
        self.t.view(self.idt).fill_(self.sent)
        self.body = self.t[GUARD:GUARD + count]

    def read(self):
        torch.cuda.synchronize()
        bits = self.t.view(self.idt).cpu()
        assert (bits[:GUARD] == self.sent).all(), "the guard in front of the output was written"
        assert (bits[GUARD + self.count:] == self.sent).all(), "the guard behind the output was written"
        missed = (bits[GUARD:GUARD + self.count] == self.sent).nonzero()
        assert missed.numel() == 0, f"{missed.numel()} elements in range never written, first at {int(missed[0])}"
        return self.body.cpu()


class Operand:
    """An NHWC input [n,h,w,stride] holding c real channels, as the layout kernel leaves it (channels beyond c zero, or `fill`).
    exact16: plain interleaved NHWC pairs as compact.hip lays them out -- the hi tensor, directly behind it the lo tensor
    (lo_offset = pixels * stride) -- where the x2-plan tests use chunk-planar operands only; the exact16 cases of
    test_conv3x3_prelu[cin64] and test_conv3x3_nchw_tail[48] are that network's 64 -> 64 and 64 -> 48 passes.
    value: the NCHW float64 value of the real channels -- what the kernel is given."""

    def __init__(self, L, x, dtype, stride, fill=0.0):
        n, c, h, w = x.shape
        nhwc = x.permute(0, 2, 3, 1)
        if dtype == L.RESR_F16X2:
            hi, lo = R.pair_split(nhwc)
            self.value = R.pair_value(hi, lo).permute(0, 3, 1, 2)
            buf = torch.full((2, n, h, w, stride), fill, dtype=torch.float16)
            buf[0, ..., :c], buf[1, ..., :c] = hi, lo
            self.lo_offset = n * h * w * stride
        else:
            td = torch.float16 if dtype == L.RESR_F16 else torch.float32
            q = nhwc.to(td)
            self.value = q.double().permute(0, 3, 1, 2)
            buf = torch.full((n, h, w, stride), fill, dtype=td)
            buf[..., :c] = q
            self.lo_offset = 0
        self.t = buf.cuda()


def _conv_case(seed, cin, cout, n, h, w):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    return g, x, wt, bias


def _weights(U, wt, dtype):
    """(packed weights, the values they carry): f16 packs the f16 rounding, f32 and exact16 the fp32 values."""
    return U.pack_conv(wt, dtype), (U.quant(wt, dtype) if dtype == U.L.RESR_F16 else wt)


def _nhwc_result(L, out, dtype, n, h, w, c):
    """A Guarded NHWC output [n,h,w,c] (exact16: hi then lo) as the NCHW float64 value."""
    flat = out.read()
    if dtype == L.RESR_F16X2:
        v = R.pair_value(flat[:flat.numel() // 2], flat[flat.numel() // 2:])
    else:
        v = flat.double()
    return v.reshape(n, h, w, c).permute(0, 3, 1, 2)


def _desc(L, n, h, w, cin_pad, cout, dtype, flags, slope, x, nchw=False):
    cout_pad = (cout + 31) // 32 * 32
    d = L.ConvDesc(n, h, w, cin_pad, cin_pad, cin_pad, 0, cout, cout_pad, 0 if nchw else cout_pad, 0, 0, 0, dtype, flags,
                   1.0, 1.0, 1.0, 1.0, slope)
    d.in0_lo_offset = x.lo_offset
    d.out_lo_offset = 0 if nchw or dtype != L.RESR_F16X2 else n * h * w * cout_pad
    return d


@pytest.mark.parametrize("dtype_name", ["f32", "f16", "exact16"])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=GEO_IDS)
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("cin", [64, 3], ids=["cin64", "cin3"])
def test_conv3x3_prelu(U, cin, with_bias, geo, dtype_name):
    """conv3x3_dispatch_prelu (the compact generator's body and, with 3 real channels in a 32-channel chunk, its first conv) through
    resr_debug_conv3x3_prelu: per-channel slopes from [-0.5, 1.5) -- negative ones and ones above 1 included."""
    L = U.L
    dtype = _dtype(L, dtype_name)
    n, h, w = geo
    g, x, wt, bias = _conv_case(cin + n + h + w, cin, 64, n, h, w)
    slopes = torch.rand(64, generator=g) * 2.0 - 0.5
    assert (slopes < 0).any() and (slopes > 1).any()
    xo = Operand(L, x, dtype, 64 if cin == 64 else 32)
    packed, wv = _weights(U, wt, dtype)
    d = _desc(L, n, h, w, xo.t.shape[-1], 64, dtype, 0 if with_bias else L.CONV_NO_BIAS, 0.0, xo)
    out = Guarded(n * h * w * 64 * (2 if dtype == L.RESR_F16X2 else 1), _tdtype(L, dtype))
    bias_d, slopes_d = bias.cuda(), slopes.cuda()
    L.check(L.lib().resr_debug_conv3x3_prelu(C.byref(d), L.ptr(xo.t), L.ptr(packed), L.ptr(bias_d) if with_bias else None,
                                             L.ptr(slopes_d), L.ptr(out.body), L.stream_ptr()), "resr_debug_conv3x3_prelu")
    got = _nhwc_result(L, out, dtype, n, h, w, 64)
    epi = dict(prelu=slopes, **({"bias": bias} if with_bias else {}))
    ref, _, ref32 = refs(xo.value, wv, **epi)
    judge(f"conv_prelu_cin{cin}_{'bias' if with_bias else 'nobias'}_{GEO_IDS[GEOMETRIES.index(geo)]}_{dtype_name}", dtype_name, got, ref,
          ref32, "pair" if dtype == L.RESR_F16X2 else dtype_name)


@pytest.mark.parametrize("dtype_name", ["f32", "f16", "exact16"])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=GEO_IDS)
@pytest.mark.parametrize("slope", [0.1, 0.0], ids=["slope0.1", "slope0"])
def test_conv3x3_cin3_forward(U, slope, geo, dtype_name):
    """The first conv of both generators: 3 real channels in a 32-channel chunk, LeakyReLU 0.1 (the compact generator's) and slope 0
    (its ReLU; -0.0 where torch stores 0.0 is nothing to the rule).  The 29 padded channels contribute nothing twice over -- the
    buffer holds zeros there and so do the packed weights: filling the buffer's padding with a finite sentinel changes no bit."""
    L = U.L
    dtype = _dtype(L, dtype_name)
    n, h, w = geo
    g, x, wt, bias = _conv_case(3 + n + h + w, 3, 64, n, h, w)
    packed, wv = _weights(U, wt, dtype)
    bias_d = bias.cuda()
    flat = []
    for fill in (0.0, 3.0):
        xo = Operand(L, x, dtype, 32, fill=fill)
        d = _desc(L, n, h, w, 32, 64, dtype, L.CONV_LRELU, slope, xo)
        out = Guarded(n * h * w * 64 * (2 if dtype == L.RESR_F16X2 else 1), _tdtype(L, dtype))
        L.check(L.lib().resr_conv3x3(C.byref(d), L.ptr(xo.t), None, L.ptr(packed), L.ptr(bias_d), None, None, None, L.ptr(out.body),
                                     None, L.stream_ptr()), "resr_conv3x3")
        flat.append(out.read())
        if fill == 0.0:
            got = _nhwc_result(L, out, dtype, n, h, w, 64)
    ref, _, ref32 = refs(xo.value, wv, bias=bias, lrelu=True, slope=slope)
    judge(f"conv_cin3_slope{slope}_{GEO_IDS[GEOMETRIES.index(geo)]}_{dtype_name}", dtype_name, got, ref, ref32,
          "pair" if dtype == L.RESR_F16X2 else dtype_name)
    idt = SENT[_tdtype(L, dtype)][0]
    assert torch.equal(flat[0].view(idt), flat[1].view(idt)), "the padded input channels reached the result"


@pytest.mark.parametrize("dtype_name", ["f32", "f16", "exact16"])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=GEO_IDS)
@pytest.mark.parametrize("cout", [12, 27, 48])
def test_conv3x3_nchw_tail(U, cout, geo, dtype_name):
    """The compact generator's last conv for x2, x3 and x4: 64 -> 3 s^2 channels as planar fp32 [N,cout,H,W], no activation, no
    clamp.  27 leaves a ragged quad of output channels.  Every element in range is written, nothing outside."""
    L = U.L
    dtype = _dtype(L, dtype_name)
    n, h, w = geo
    g, x, wt, bias = _conv_case(cout + n + h + w, 64, cout, n, h, w)
    xo = Operand(L, x, dtype, 64)
    packed, wv = _weights(U, wt, dtype)
    d = _desc(L, n, h, w, 64, cout, dtype, L.CONV_OUT_NCHW_F32, 0.0, xo, nchw=True)
    out = Guarded(n * cout * h * w, torch.float32)
    bias_d = bias.cuda()
    L.check(L.lib().resr_conv3x3(C.byref(d), L.ptr(xo.t), None, L.ptr(packed), L.ptr(bias_d), None, None, None, L.ptr(out.body),
                                 None, L.stream_ptr()), "resr_conv3x3")
    got = out.read().double().reshape(n, cout, h, w)
    ref, _, ref32 = refs(xo.value, wv, bias=bias)
    judge(f"conv_nchw{cout}_{GEO_IDS[GEOMETRIES.index(geo)]}_{dtype_name}", dtype_name, got, ref, ref32,
          "pair" if dtype == L.RESR_F16X2 else "f32")


WGRAD_SMALL = [
    # name, cin, cout, n, h, w, dtypes -- the coarsest U-Net level of the discriminator on a 64 x 64 crop is 8 x 8 (discriminator.py:
    # up_block1, 512 -> 256; f16 runs it in layer mode, strict mode one 64-channel output group at a time), then one pixel, one row, one column
    ("w_unet8x8", 512, 256, 2, 8, 8, ("f16",)),
    ("w_unet8x8_group", 512, 64, 2, 8, 8, ("f32",)),
    ("w_1x1", 64, 32, 1, 1, 1, ("f32", "f16")),
    ("w_row", 64, 32, 2, 1, 40, ("f32", "f16")),
    ("w_col", 64, 32, 2, 40, 1, ("f32", "f16")),
]


WGRAD_SMALL_PARAMS = [(c, dt) for c in WGRAD_SMALL for dt in c[6]]


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("case,dtype_name", WGRAD_SMALL_PARAMS, ids=[f"{c[0]}-{dt}" for c, dt in WGRAD_SMALL_PARAMS])
def test_wgrad_small_geometry(U, case, dtype_name, splits):
    """Weight gradients at the smallest geometries: fewer tiles than pixel splits (a split without a tile still owes its slab),
    images narrower or shorter than a tile's halo."""
    L = U.L
    name, cin, cout, n, h, w, _ = case
    dtype = _dtype(L, dtype_name)
    g = torch.Generator().manual_seed(cin + h + w)
    x = U.quant(torch.randn(n, cin, h, w, generator=g), dtype)
    gy = U.quant(torch.randn(n, cout, h, w, generator=g), dtype)
    xb = U.to_nhwc(x, dtype, stride=cin + 32)
    gb = U.to_nhwc(gy, dtype, stride=cout + 32)
    d = L.WgradDesc(n, h, w, cin, cin, cin + 32, 0, cin, cout, cout, cout + 32, dtype, 0, splits, 0.5)
    partial = torch.empty(L.lib().resr_wgrad_partial_bytes(C.byref(d)) // 4, device="cuda")
    dw, db = Guarded(cout * cin * 9, torch.float32), Guarded(cout, torch.float32)
    L.check(L.lib().resr_conv3x3_wgrad(C.byref(d), L.ptr(xb), None, L.ptr(gb), L.ptr(partial), L.ptr(dw.body), L.ptr(db.body),
                                       L.stream_ptr()), "resr_conv3x3_wgrad")
    judge_wgrad(f"wgrad_{name}_s{splits}_{dtype_name}", dtype_name, dw.read().reshape(cout, cin, 3, 3), db.read(), x, gy, 0.5, False)


# ---- exact16 (RESR_F16X2), one pass at a time: conv3x3_ws_x2_mt1.hip / conv3x3_ws_x2_mt2.hip and the three tap-products of wgrad.hip ----
class GuardedWhere(Guarded):
    """Guarded, for an output that owns only part of its range (the real channels of a padded pixel stride; the hi tensor of a
    single-f16 output): `owned` (bool, one per element) says which.  Every owned element must have been written and no other --
    the channels between cout and the pixel stride, the gap between the hi and the lo tensor, a lo tensor nobody asked for."""

    def __init__(self, owned, tdtype):
        super().__init__(owned.numel(), tdtype)
        self.owned = owned.reshape(-1)

    def read(self):
        torch.cuda.synchronize()
        bits = self.t.view(self.idt).cpu()
        assert (bits[:GUARD] == self.sent).all(), "the guard in front of the output was written"
        assert (bits[GUARD + self.count:] == self.sent).all(), "the guard behind the output was written"
        wrote = bits[GUARD:GUARD + self.count] != self.sent
        missed = (self.owned & ~wrote).nonzero()
        assert missed.numel() == 0, f"{missed.numel()} elements in range never written, first at {int(missed[0])}"
        stray = (wrote & ~self.owned).nonzero()
        assert stray.numel() == 0, f"{stray.numel()} elements outside the output's channels written, first at {int(stray[0])}"
        return self.body.cpu()


# elements between an operand's hi tensor and its lo tensor, on top of the hi tensor's size: every operand of a pass gets a hi -> lo
# offset of its own, so that a kernel that takes one operand's offset for another's reads (or writes) the wrong data
GAP = {"in0": 8, "in1": 24, "res0": 40, "res1": 56, "mask": 72, "out": 88}


class Layout:
    """Where the elements of an [n,h,w,c] operand or output sit in device memory: interleaved NHWC with a padded pixel stride and the
    channels at `offset` inside the pixel, or chunk-planar [c/32][n,h,w,32].  exact16: the hi tensor, behind it (after `gap`
    elements of nobody's) the lo tensor; single: an exact16 output stored as its hi tensor alone (the lo tensor must stay untouched).
    index[n,h,w,c]: the element's position in the hi tensor."""

    def __init__(self, L, dtype, n, h, w, c, stride=0, offset=0, gap=0, planar=False, single=False):
        px = n * h * w
        pix, ch = torch.arange(px).view(n, h, w, 1), torch.arange(c)
        if planar:
            assert c % 32 == 0 and offset == 0
            self.index, self.size = (ch // 32) * (px * 32) + pix * 32 + ch % 32, (c // 32) * px * 32
            self.pixel_stride, self.chunk_stride = 32, px * 32
        else:
            self.index, self.size = pix * stride + offset + ch, px * stride
            self.pixel_stride, self.chunk_stride = stride, 0
        self.pair, self.single, self.offset = dtype == L.RESR_F16X2, single, offset
        self.tdtype = _tdtype(L, dtype)
        self.lo_offset = self.size + gap if self.pair else 0
        self.total = self.lo_offset + self.size if self.pair else self.size

    def upload(self, x, poison_lo=None):
        """x: NCHW fp32 (cpu).  Sets .t (device, flat), .value and .hi (NCHW float64: what the kernel is given, and its hi half);
        poison_lo: a channel slice whose lo elements hold garbage (single chunks: never to be read)."""
        nhwc = x.permute(0, 2, 3, 1)
        buf = torch.zeros(self.total, dtype=self.tdtype)
        if self.pair:
            hi, lo = R.pair_split(nhwc)
            self.value, self.hi = R.pair_value(hi, lo).permute(0, 3, 1, 2), hi.double().permute(0, 3, 1, 2)
            if poison_lo is not None:
                lo = lo.clone()
                lo[..., poison_lo] = 777.0
            buf[self.index], buf[self.index + self.lo_offset] = hi, lo
        else:
            q = nhwc.to(self.tdtype)
            self.value = self.hi = q.double().permute(0, 3, 1, 2)
            buf[self.index] = q
        self.t = buf.cuda()
        return self

    def ptr(self, U):
        return U.sptr(self.t, self.offset)

    def guarded(self):
        owned = torch.zeros(self.total, dtype=torch.bool)
        owned[self.index] = True
        if self.pair and not self.single:
            owned[self.index + self.lo_offset] = True
        self.out = GuardedWhere(owned, self.tdtype)
        return self.out

    def out_ptr(self):
        return C.c_void_p(self.out.body.data_ptr() + self.offset * self.out.body.element_size())

    def result(self):
        """The stored output as its NCHW float64 value (a pair joined, after the check that its lo half is a remainder of its hi
        half: conv_ref.pair_lo_excess)."""
        flat = self.out.read()
        hi = flat[self.index]
        if self.pair and not self.single:
            lo = flat[self.index + self.lo_offset]
            assert R.pair_lo_excess(hi, lo) == 0, "a stored lo half is no remainder of its hi half"
            return R.pair_value(hi, lo).permute(0, 3, 1, 2)
        return hi.double().permute(0, 3, 1, 2)


def _sign_words(n, h, w, cout):
    return Guarded(n * h * w * ((cout + 31) // 32), torch.float32)     # (read as uint32 words; the sentinel is no word a test meets)


def _sign_bits(words, n, h, w, cout):
    wd = words.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    cp = (cout + 31) // 32 * 32
    return ((wd.unsqueeze(-1) >> torch.arange(32)) & 1).reshape(n, h, w, cp)[..., :cout].permute(0, 3, 1, 2).bool()


_CC = {c[0]: c[1:] for c in CONV_CASES}
X2_CONV_CASES = [
    # id, form of launch_ws (conv3x3_ws.h), (cin, cin0, cout, flags, n, h, w) -- by name: the shape of that CONV_CASES entry --, options
    ("rdb_conv1", 0, "rdb_conv1", {}),
    ("up_conv", 0, "up_conv", {}),
    ("rdb_conv3_2seg", 0, "rdb_conv3_2seg", {}),
    ("two_seg_5chunks", 0, "two_seg_5chunks", {}),
    ("mask_only", 1, "mask_only", {}),
    ("mask_only_hi_alone", 1, "mask_only", {"mask_lo0": True}),        # mask_lo_offset = 0: the mask's hi tensor decides alone
    ("dgrad_mask", 3, "dgrad_mask", {}),
    ("res0_only", 2, "res0_only", {}),
    ("rdb_conv5_res", 6, "rdb_conv5_res", {}),
    ("signbits32", 16, "signbits32", {}),
    ("signbits64", 16, "signbits64", {}),
    ("signbits32_single", 16, "signbits32", {"out_single": True}),     # RESR_CONV_OUT_SINGLE: the lo tensor stays untouched
    ("maskbits32", 33, "maskbits32", {}),
    ("maskbits64", 33, "maskbits64", {}),
    ("conv4_nchw", 15, "conv4_nchw", {}),
    ("cout24_res", 15, "cout24_res", {}),
    ("cout48_res", 15, "cout48_res", {}),
    ("lrelu_slope1.5", 15, "rdb_conv1", {"slope": 1.5}),               # a slope outside [0, 1]: no max(v, slope v) form
    ("cout8", 0, "cout8", {}),
    ("cout16", 0, "cout16", {}),
    ("cout24", 0, "cout24", {}),
    ("cout48", 0, "cout48", {}),
    # x2_pair_chunks across the segments: chunks 0-2 pairs, chunk 3 single -- in1 holds one of each, the single one's lo plane poisoned
    ("pair_chunks3_2seg", 0, (128, 64, 32, "lrelu", 1, 33, 32), {"pair_chunks": 3}),
    ("pair_chunks3_2seg_w16", 0, (128, 64, 32, "lrelu", 1, 33, 32), {"pair_chunks": 3, "single_w16": True}),
    ("planar_small", 16, (64, 64, 32, "lrelu,signbits", 1, 20, 24), {"planar": True}),
    # 16-row tiles (chosen when the launch has at least as many of them as the device has CUs): 7 x 5 x 8 = 280 tiles, the last tile
    # row 8 of 16 rows, the last tile column 8 of 32 columns
    ("rows16_32", 16, (64, 64, 32, "lrelu,signbits", 8, 72, 200), {}),
    ("rows16_64", 2, (64, 64, 64, "res0", 8, 72, 200), {}),
]


@pytest.mark.parametrize("case", X2_CONV_CASES, ids=[c[0] for c in X2_CONV_CASES])
def test_exact16_conv_pass(U, case):
    """One exact16 pass per epilogue form of launch_ws, on the shapes of CONV_CASES (8-row tiles with seams and ragged edges) and on
    16-row tiles.  Operands are interleaved NHWC pairs with padded pixel strides (planar_small: chunk-planar), each with its own
    hi -> lo offset; the output is guarded element by element; the reference is conv_ref.conv3x3 in float64 on the pair values that
    were uploaded and the fp32 weights, the judgement the pair rule (no fp32 yardstick is computed)."""
    import zlib
    L = U.L
    dt = L.RESR_F16X2
    ident, form, shape, opt = case
    cin, cin0, cout, fl, n, h, w = _CC[shape] if isinstance(shape, str) else shape
    fl = set(fl.split(","))
    slope, planar, out_single = opt.get("slope", 0.2), opt.get("planar", False), opt.get("out_single", False)
    g = torch.Generator().manual_seed(zlib.crc32(ident.encode()) % 1000)
    up = "up" in fl
    hs, ws = (h // 2, w // 2) if up else (h, w)
    x = torch.randn(n, cin, hs, ws, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    cout_pad, c1 = (cout + 31) // 32 * 32, cin - cin0
    pc = opt.get("pair_chunks", 0) * 32 or cin                  # channels [0, pc) are pairs, the rest single f16 tensors

    def singles(first, count):                                   # the channel slice of a segment that holds single chunks
        return slice(max(pc - first, 0), count) if pc < first + count else None
    a = Layout(L, dt, n, hs, ws, cin0, cin0 + 32, gap=GAP["in0"], planar=planar).upload(x[:, :cin0], singles(0, cin0))
    b = Layout(L, dt, n, hs, ws, c1, c1 + 64, offset=32, gap=GAP["in1"]).upload(x[:, cin0:], singles(cin0, c1)) if c1 else None
    xv = torch.cat([a.value, b.value], 1) if b else a.value
    xh = torch.cat([a.hi, b.hi], 1) if b else a.hi
    x_eff = torch.cat([xv[:, :pc], xh[:, pc:]], 1)
    w_eff = wt.double()
    flags = 0
    if opt.get("single_w16"):                                    # the single chunks meet W0 = f16(w 2^12) alone
        flags |= L.CONV_SINGLE_W16
        w_eff = torch.cat([w_eff[:, :pc], R.split_weights(wt)[0][:, pc:]], 1)
    nchw = "nchw" in fl
    o = None if nchw else Layout(L, dt, n, h, w, cout, cout_pad + 32, gap=GAP["out"], planar=planar, single=out_single)
    d = L.ConvDesc(n, h, w, cin, cin0, a.pixel_stride, b.pixel_stride if b else 0, cout, cout_pad, 0 if nchw else o.pixel_stride, 0, 0, 0, dt, 0,
                   1.0, 1.0, 1.0, 1.0, slope)
    d.in0_chunk_stride, d.in0_lo_offset = a.chunk_stride, a.lo_offset
    d.x2_pair_chunks = opt.get("pair_chunks", 0)
    if b:
        d.in1_lo_offset = b.lo_offset
    if o:
        d.out_chunk_stride, d.out_lo_offset = o.chunk_stride, 0 if out_single else o.lo_offset
    epi = {"slope": slope}
    if "nobias" in fl:
        flags |= L.CONV_NO_BIAS
    else:
        epi["bias"] = bias
    if up:
        flags |= L.CONV_UPSAMPLE_IN
    if out_single:
        flags |= L.CONV_OUT_SINGLE
    mask = res0 = res1 = aux = None
    offsets = [a.lo_offset] + ([b.lo_offset] if b else []) + ([o.lo_offset] if o else [])
    if "mask" in fl:
        flags |= L.CONV_MASK
        mk = torch.randn(n, cout, h, w, generator=g)
        if "maskbits" in fl:
            bits = (mk > 0).permute(0, 2, 3, 1).reshape(n, h, w, cout // 32, 32).to(torch.int64)
            words = (bits << torch.arange(32)).sum(-1)
            mask_t = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).cuda().contiguous()
            mask = L.ptr(mask_t)
            flags |= L.CONV_MASK_BITS
            epi["mask"] = mk
        else:
            # a saved activation, itself a pair; a fifth of it +-1e-9: the hi half is zero there and the lo half holds the sign
            mk = torch.where(torch.rand(mk.shape, generator=g) < 0.2, mk.sign() * 1e-9, mk)
            m = Layout(L, dt, n, h, w, cout, cout + 32, gap=GAP["mask"]).upload(mk)
            assert ((m.hi == 0) & (m.value > 0)).sum() > 100
            mask, d.mask_stride = m.ptr(U), m.pixel_stride
            d.mask_lo_offset = 0 if opt.get("mask_lo0") else m.lo_offset
            epi["mask"] = m.hi if opt.get("mask_lo0") else m.value
            offsets.append(m.lo_offset)
    if "lrelu" in fl:
        flags |= L.CONV_LRELU
        epi["lrelu"] = True
    if "res0" in fl:
        r0 = Layout(L, dt, n, h, w, cout, cout + 64, gap=GAP["res0"]).upload(torch.randn(n, cout, h, w, generator=g))
        res0, d.res0_stride, d.res0_lo_offset, d.s0, d.t0 = r0.ptr(U), r0.pixel_stride, r0.lo_offset, 0.2, 1.0
        epi.update(res0=r0.value, s0=0.2, t0=1.0)
        offsets.append(r0.lo_offset)
    if "res1" in fl:
        r1 = Layout(L, dt, n, h, w, cout, cout, gap=GAP["res1"]).upload(torch.randn(n, cout, h, w, generator=g))
        res1, d.res1_stride, d.res1_lo_offset, d.s1, d.t1 = r1.ptr(U), r1.pixel_stride, r1.lo_offset, 0.2, 0.5
        epi.update(res1=r1.value, s1=0.2, t1=0.5)
        offsets.append(r1.lo_offset)
    assert len(set(offsets)) == len(offsets), "two operands share a hi -> lo offset"
    if nchw:
        flags |= L.CONV_OUT_NCHW_F32
        out = Guarded(n * cout * h * w, torch.float32)
        out_ptr = L.ptr(out.body)
        if "clamp" in fl:
            flags |= L.CONV_CLAMP01
            passed = torch.full((n, cout, h, w), 9, dtype=torch.uint8, device="cuda")
            aux = L.ptr(passed)
            epi["clamp"] = True
    else:
        o.guarded()
        out_ptr = o.out_ptr()
    if "signbits" in fl:
        flags |= L.CONV_WRITE_SIGNBITS
        sw = _sign_words(n, h, w, cout)
        aux = L.ptr(sw.body)
    d.flags = flags
    packed, bias_d = U.pack_conv(wt, dt), bias.cuda()
    L.check(L.lib().resr_conv3x3(C.byref(d), a.ptr(U), b.ptr(U) if b else None, L.ptr(packed), L.ptr(bias_d), res0, res1, mask, out_ptr, aux,
                                 L.stream_ptr()), "resr_conv3x3")
    got = out.read().double().reshape(n, cout, h, w) if nchw else o.result()
    ref, pre = R.conv3x3(x_eff, w_eff, F64, up, **epi)
    bound = judge(f"conv_x2_form{form}_{ident}", "exact16", got, ref, None, "pair16" if out_single else "pair")
    if "signbits" in fl:
        assert torch.equal(_sign_bits(sw.read(), n, h, w, cout), got > 0), "sign tensor disagrees with the stored activation"
    if "clamp" in fl:
        assert set(passed.unique().tolist()) <= {0, 1}, "pass-mask bytes never written, or not 0 / 1"
        assert R.pass_mask_ok(passed.cpu(), pre, bound) == 0


AUX_CASES = [
    # id, flags, output groups -- the discriminator's calls (disc_native.hip): an up block's convolution keeps its activation from before
    # the skip connection is added; a backward-data pass keeps the gradient from before the LeakyReLU mask
    ("before_res", "lrelu,res0,aux_res", 1),
    ("before_mask", "mask,nobias,aux_mask", 1),
    ("before_res_groups2", "lrelu,res0,aux_res,nobias", 2),
]
AUX_PARAMS = [(c, dt) for c in AUX_CASES for dt in ("f32", "f16", "exact16") if not (c[2] > 1 and dt == "f32")]


@pytest.mark.parametrize("geo", [(2, 20, 36), (1, 33, 31)], ids=["2x20x36", "1x33x31"])
@pytest.mark.parametrize("case,dtype_name", AUX_PARAMS, ids=[f"{c[0]}-{dt}" for c, dt in AUX_PARAMS])
def test_aux_before_forms(U, case, dtype_name, geo):
    """RESR_CONV_AUX_BEFORE_RES and RESR_CONV_AUX_BEFORE_MASK, cin 64 -> 64 channels per output group: f16 takes the specialised
    epilogues 66 and 65 of launch_ws, exact16 the general one, f32 the one-role kernel.  out and aux are both guarded and both judged
    by their dtype's rule; the exact16 aux is a pair of out's layout at out's hi -> lo offset."""
    L = U.L
    dtype = _dtype(L, dtype_name)
    ident, fl, groups = case
    fl = set(fl.split(","))
    n, h, w = geo
    cin, cout = 64, 64 * groups
    g, x, wt, bias = _conv_case(len(ident) + n + h + w, cin, cout, n, h, w)
    a = Layout(L, dtype, n, h, w, cin, cin + 32, gap=GAP["in0"]).upload(x)
    o = Layout(L, dtype, n, h, w, cout, cout + 32, gap=GAP["out"])
    ax = Layout(L, dtype, n, h, w, cout, cout + 32, gap=GAP["out"])
    d = L.ConvDesc(n, h, w, cin, cin, a.pixel_stride, 0, 64, 64, o.pixel_stride, 0, 0, 0, dtype, 0, 1.0, 1.0, 1.0, 1.0, 0.2)
    d.in0_lo_offset, d.out_lo_offset, d.cout_groups = a.lo_offset, o.lo_offset, groups if groups > 1 else 0
    epi, flags = {"slope": 0.2}, 0
    mask = res0 = None
    if "nobias" in fl:
        flags |= L.CONV_NO_BIAS
    else:
        epi["bias"] = bias
    if "mask" in fl:
        mk = torch.randn(n, cout, h, w, generator=g)
        m = Layout(L, dtype, n, h, w, cout, cout + 64, gap=GAP["mask"]).upload(mk)
        mask, d.mask_stride, d.mask_lo_offset = m.ptr(U), m.pixel_stride, m.lo_offset
        flags |= L.CONV_MASK | L.CONV_AUX_BEFORE_MASK
        epi["mask"] = m.value
    if "lrelu" in fl:
        flags |= L.CONV_LRELU
        epi["lrelu"] = True
    if "res0" in fl:
        r0 = Layout(L, dtype, n, h, w, cout, cout + 96, gap=GAP["res0"]).upload(torch.randn(n, cout, h, w, generator=g))
        res0, d.res0_stride, d.res0_lo_offset, d.s0, d.t0 = r0.ptr(U), r0.pixel_stride, r0.lo_offset, 1.0, 1.0
        flags |= L.CONV_AUX_BEFORE_RES
        epi.update(res0=r0.value, s0=1.0, t0=1.0)
    d.flags = flags
    if groups > 1:   # consecutive 64-row chunk tables, as resr_pack_weights lays them out (include/resr.h, cout_groups)
        per_group = (cin // 32) * 9 * 2 * 1024 * {L.RESR_F16: 2, L.RESR_F16X2: 6}[dtype]
        packed = torch.cat([U.pack_conv(wt[q * 64:(q + 1) * 64], dtype)[:per_group] for q in range(groups)]
                           + [torch.zeros(16384, dtype=torch.uint8, device="cuda")])
    else:
        packed = U.pack_conv(wt, dtype)
    wv = U.quant(wt, dtype) if dtype == L.RESR_F16 else wt
    o.guarded()
    ax.guarded()
    bias_d = bias.cuda()
    L.check(L.lib().resr_conv3x3(C.byref(d), a.ptr(U), None, L.ptr(packed), L.ptr(bias_d), res0, None, mask, o.out_ptr(), ax.out_ptr(),
                                 L.stream_ptr()), "resr_conv3x3")
    got, got_aux = o.result(), ax.result()
    pair = dtype == L.RESR_F16X2
    r64 = R.conv3x3(a.value, wv, F64, with_aux=True, **epi)
    r32 = (None,) * 4 if pair else R.conv3x3(a.value, wv, F32, with_aux=True, **epi)
    which = 3 if "aux_res" in fl else 2
    name = f"conv_aux_{ident}_{'x'.join(map(str, geo))}_{dtype_name}"
    judge(name + "_out", dtype_name, got, r64[0], r32[0], "pair" if pair else dtype_name)
    judge(name + "_aux", dtype_name, got_aux, r64[which], r32[which], "pair" if pair else dtype_name)


def _x2_wgrad(U, name, cin, cout, up, n, h, w, splits, single_g=False, cin0=None):
    """One exact16 weight-gradient launch (the job-table one for these sizes) on interleaved NHWC pairs with padded strides and guarded
    dW / db; |got - ref64| <= A + conv_ref.wgrad_lolo for dW, <= A for db."""
    L = U.L
    dt = L.RESR_F16X2
    g = torch.Generator().manual_seed(7)
    hs, ws = (h // 2, w // 2) if up else (h, w)
    x = torch.randn(n, cin, hs, ws, generator=g)
    gy = torch.randn(n, cout, h, w, generator=g)
    cin_pad, cout_pad = (cin + 31) // 32 * 32, (cout + 31) // 32 * 32
    cin0 = cin0 or cin_pad
    xa = Layout(L, dt, n, hs, ws, min(cin, cin0), cin0 + 32, gap=GAP["in0"]).upload(x[:, :cin0])
    xb = None
    if cin0 < cin_pad:   # the second segment shares X's one hi -> lo offset: its gap makes up for its narrower pixel stride
        stride1 = cin_pad - cin0 + 16
        xb = Layout(L, dt, n, hs, ws, cin - cin0, stride1, gap=xa.lo_offset - n * hs * ws * stride1).upload(x[:, cin0:])
        assert xb.lo_offset == xa.lo_offset and stride1 < xa.pixel_stride
    gb = Layout(L, dt, n, h, w, cout, cout_pad + 32, gap=GAP["out"], single=single_g).upload(gy)
    xv = torch.cat([xa.value, xb.value], 1) if xb else xa.value
    gv = gb.hi if single_g else gb.value
    d = L.WgradDesc(n, h, w, cin_pad, cin0, xa.pixel_stride, xb.pixel_stride if xb else 0, cin, cout, cout_pad, gb.pixel_stride, dt,
                    (L.CONV_UPSAMPLE_IN if up else 0) | (L.CONV_OUT_SINGLE if single_g else 0), splits, 0.5)
    d.x_lo_offset, d.g_lo_offset = xa.lo_offset, 0 if single_g else gb.lo_offset
    partial = torch.empty(L.lib().resr_wgrad_partial_bytes(C.byref(d)) // 4, device="cuda")
    dw, db = Guarded(cout * cin * 9, torch.float32), Guarded(cout, torch.float32)
    L.check(L.lib().resr_conv3x3_wgrad(C.byref(d), xa.ptr(U), xb.ptr(U) if xb else None, gb.ptr(U), L.ptr(partial), L.ptr(dw.body),
                                       L.ptr(db.body), L.stream_ptr()), "resr_conv3x3_wgrad")
    judge_wgrad(f"wgrad_x2_{name}", "exact16", dw.read().reshape(cout, cin, 3, 3), db.read(), xv, gv, 0.5, up, lolo=True)


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_exact16_wgrad(U, case):
    """The plain (job-table) exact16 weight-gradient launch -- what every 64 -> 32 and 64 -> 64 layer of the generator uses -- element
    by element, at the shapes of test_wgrad."""
    name, cin, cout, up, n, h, w = case
    _x2_wgrad(U, name, cin, cout, up, n, h, w, 3)


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("case", [c for c in WGRAD_SMALL if c[0] in ("w_1x1", "w_row", "w_col")], ids=["w_1x1", "w_row", "w_col"])
def test_exact16_wgrad_small_geometry(U, case, splits):
    name, cin, cout, n, h, w, _ = case
    _x2_wgrad(U, f"{name}_s{splits}", cin, cout, 0, n, h, w, splits)


def test_exact16_wgrad_two_segment_x(U):
    """X in two segments (cin 128, cin0 64, x1 given): both share the descriptor's one x_lo_offset."""
    _x2_wgrad(U, "w_2seg", 128, 32, 0, 1, 21, 38, 3, cin0=64)
    # refused loudly, not computed wrongly: a second segment in layer mode (an output wider than 64 channels), x1 without cin0 < cin
    L = U.L
    t = torch.zeros(1 << 16, dtype=torch.float16, device="cuda")
    dw = torch.zeros(128 * 128 * 9, device="cuda")
    for cout, cin0, x1 in ((128, 64, t), (32, 128, t), (32, 64, None)):
        d = L.WgradDesc(1, 8, 8, 128, cin0, 96, 80, 128, cout, cout, cout + 32, L.RESR_F16X2, 0, 1, 1.0)
        d.x_lo_offset = d.g_lo_offset = 20000
        partial = torch.zeros(L.lib().resr_wgrad_partial_bytes(C.byref(d)) // 4, device="cuda")
        assert L.lib().resr_conv3x3_wgrad(C.byref(d), L.ptr(t), L.ptr(x1), L.ptr(t), L.ptr(partial), L.ptr(dw), None, L.stream_ptr()) != 0


def test_exact16_wgrad_single_g(U):
    """RESR_CONV_OUT_SINGLE: G enters as its hi tensor (the lo tensor behind it is there and must not be read), in the reference too."""
    _x2_wgrad(U, "w_single_g", 96, 32, 0, 1, 21, 38, 3, single_g=True)
