"""-m gpu: the float degradation kernels of csrc/degrade.hip, one by one, against the plain references of tests/degrade_ref.py.

The rule (tests/conv_ref.py, shown to reject wrong kernels at these very shapes by tests/test_degrade_ref.py).  Per case
A = max(4 * e32, one fp32 ulp of max |ref64|), e32 = the plain fp32 restatement's own distance to float64 on the same inputs; no
element of the kernel's output may lie beyond A.  Nothing about A is fixed in advance, nothing is taken from the kernel's output.
Every judgement is written to <diag_dir>/degrade_kernels.json: cpu32_err, allowance, kernel_err, ratio.

Where an operation is exact the test says torch.equal instead: a one-hot blur kernel moves pixels, an identity resize copies them, an
area mean over 4 x 4 dyadic values has no rounding, a rounded noise output is a multiple of 1 / 255, the crop copies.

The samplers are judged by their law: a Poisson draw is decoded from the output and its counts are set against the Poisson pmf
(mean, variance, chi-square per level at 1e-6, correlations at 5 sigma), the normals against the normal cdf (Kolmogorov-Smirnov at 1e-6).
The limits come from the laws, none from the kernels; the seeds are fixed.

Worst ratio kernel_err / A per kernel, measured on the MI355X:
  filter2d_kernel 0.250 (11 cases)   filter2d21_kernel 0.267 (16)   filter1d_kernel 0.250 (6)   usm_bwd 0.250 (5)
  resize_kernel 0.290 (24)           gauss_noise_kernel 0.250 (8)
0.25 is the yardstick's own ratio (e32 / 4 e32): these kernels add their terms in the definition's order and land on the plain fp32
evaluation's error, not merely near it.  Poisson per level: |z| of the mean <= 1.2, of the variance <= 2.8, chi-square 8.6 .. 79.6
against limits of 38.3 .. 191.4; Kolmogorov-Smirnov distance of 2^20 normals 6.9e-4 against 2.63e-3.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import conv_ref as C
from tests import degrade_ref as R

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
SENTINEL = -777.25
GENERIC = os.environ.get("RESR_FILTER_GENERIC") is not None      # (read once per process by the library: not toggled here)
RECORDS = {}


@pytest.fixture(scope="module")
def L():
    import real_esrgan_pytorch_amd as pkg
    return pkg._lib


@pytest.fixture(scope="module")
def ip():
    from real_esrgan_pytorch_amd import imgproc
    return imgproc


@pytest.fixture(scope="module", autouse=True)
def _write_diag(diag_dir):
    yield
    worst = {}
    for rec in RECORDS.values():
        worst[rec["kernel"]] = max(worst.get(rec["kernel"], 0.0), rec["ratio"])
    with open(os.path.join(diag_dir, "degrade_kernels.json"), "w") as f:
        json.dump({"worst": worst, "cases": RECORDS}, f, indent=1, sort_keys=True)


def judge(kernel, case, got, ref64, ref32):
    rec = C.judge(got.cpu(), ref64, ref32, "f32")
    rec["kernel"] = kernel
    RECORDS[f"{kernel}:{case}"] = rec
    print(f"{kernel}:{case} cpu32_err {rec['cpu32_err']:.3e} allowance {rec['allowance']:.3e} kernel_err {rec['kernel_err']:.3e} "
          f"ratio {rec['ratio']:.3f}")
    assert rec["bad"] == 0, (kernel, case, rec)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- filters ------------------------------------------------------------------------------------------------------------------------------
def filter_kernel_name(kh, kw, per_sample):
    if GENERIC:
        return "filter2d_kernel"
    if kh == 21 and kw == 21:
        return "filter2d21_kernel"
    if not per_sample and (kh, kw) in ((1, 51), (51, 1)):
        return "filter1d_kernel"
    return "filter2d_kernel"


def run_filter(L, x, k, per_sample):
    """resr_filter2d into a buffer full of sentinels; every element must come back written."""
    n, c, h, w = x.shape
    kh, kw = k.shape[-2:]
    assert k.shape[0] == (n if per_sample else 1)
    xd, kd = x.contiguous().cuda(), k.contiguous().cuda()
    out = torch.full_like(xd, SENTINEL)
    L.check(L.lib().resr_filter2d(L.ptr(xd), L.ptr(out), L.ptr(kd), n, c, h, w, kh, kw, per_sample, L.stream_ptr()), "resr_filter2d")
    torch.cuda.synchronize()
    out = out.cpu()
    assert not (out == SENTINEL).any(), "an output element was never written"
    return out


def _nine_taps(kh, kw):
    """The four corners, the four edge midpoints and the centre (fewer where an axis has one tap)."""
    return sorted({(dy, dx) for dy in (0, kh // 2, kh - 1) for dx in (0, kw // 2, kw - 1)})


def _one_hot_check(L, x, kh, kw, per_sample, taps):
    n, c, h, w = x.shape
    p = x.index_select(2, R.pad_index(h, kh // 2)).index_select(3, R.pad_index(w, kw // 2))     # reflect(y + dy - ry), reflect(x + dx - rx)
    for i, (dy, dx) in enumerate(taps):
        mine = [(dy, dx)] * n
        if per_sample and n > 1:
            mine[1:] = [taps[(i + j) % len(taps)] for j in range(1, n)]          # another tap per sample in one launch
        k = torch.zeros(n if per_sample else 1, kh, kw)
        for s in range(k.shape[0]):
            k[s, mine[s][0], mine[s][1]] = 1.0
        got = run_filter(L, x, k, per_sample)
        want = torch.stack([p[s, :, mine[s][0]:mine[s][0] + h, mine[s][1]:mine[s][1] + w] for s in range(n)])
        assert torch.equal(got, want), (tuple(x.shape), kh, kw, per_sample, mine)


@pytest.mark.parametrize("per_sample", [0, 1])
@pytest.mark.parametrize("shape", [(1, 1, 11, 11), (1, 2, 33, 65), (2, 3, 32, 64)])
def test_one_hot_21x21_moves_pixels(L, shape, per_sample):
    """Every other term is 0 * finite: orientation, correlation against convolution and the reflection rule with no tolerance."""
    _one_hot_check(L, torch.rand(shape, generator=_gen(1)), 21, 21, per_sample, _nine_taps(21, 21))


@pytest.mark.parametrize("shape,k", [((1, 2, 33, 65), 7), ((2, 3, 32, 64), 7), ((1, 1, 33, 40), 63)])
def test_one_hot_generic_moves_pixels(L, shape, k):
    _one_hot_check(L, torch.rand(shape, generator=_gen(2)), k, k, 0, _nine_taps(k, k))


@pytest.mark.parametrize("per_sample", [0, 1])
@pytest.mark.parametrize("kh,kw", [(1, 51), (51, 1)])
@pytest.mark.parametrize("shape", [(1, 2, 33, 65), (2, 3, 32, 64)])
def test_one_hot_51_taps_moves_pixels(L, shape, kh, kw, per_sample):
    taps = [(0, t) if kh == 1 else (t, 0) for t in (0, 25, 50)]
    _one_hot_check(L, torch.rand(shape, generator=_gen(3)), kh, kw, per_sample, taps)


@pytest.mark.parametrize("name", sorted(R.FILTER_CASES))
def test_dense_filter_against_float64(L, name):
    x, k = R.filter_case(name)
    per_sample = R.FILTER_CASES[name][3]
    got = run_filter(L, x, k, per_sample)
    judge(filter_kernel_name(k.shape[-2], k.shape[-1], per_sample), name, got, R.correlate_reflect(x, k, F64), R.correlate_reflect(x, k, F32))


# ---- USM -------------------------------------------------------------------------------------------------------------------------------
def _usm(L, fn, x, k1d, weight=0.5, threshold=10.0):
    n, c, h, w = x.shape
    xd, kd = x.cuda(), k1d.cuda()
    dst = torch.full_like(xd, SENTINEL)
    tmp = torch.full((3 * xd.numel(),), SENTINEL, device="cuda")
    L.check(fn(L.ptr(xd), L.ptr(dst), L.ptr(tmp), L.ptr(kd), k1d.numel(), weight, threshold, n, c, h, w, L.stream_ptr()), "resr_usm_sharp")
    torch.cuda.synchronize()
    return dst.cpu(), tmp.cpu().view(3, n, c, h, w)


def test_usm_forward_only_gives_the_same_bits(L, ip):
    """resr_usm_sharp_forward_only leaves the soft-mask store out and nothing else: dst and the blur third of tmp3 are the same bits."""
    import torch.nn.functional as F
    g = _gen(7)
    x = F.interpolate(torch.rand(1, 2, 9, 17, generator=g), size=(70, 130), mode="bicubic").clamp(0, 1)
    x = (0.8 * x + 0.2 * torch.rand(1, 2, 70, 130, generator=g)).clamp(0, 1)
    k1d = ip.USMSharp(50, 0).k1d
    full, tmp_full = _usm(L, L.lib().resr_usm_sharp, x, k1d)
    fwd, tmp_fwd = _usm(L, L.lib().resr_usm_sharp_forward_only, x, k1d)
    assert not (full == SENTINEL).any() and not (tmp_full[1:] == SENTINEL).any()
    assert torch.equal(full.view(torch.int32), fwd.view(torch.int32))
    assert torch.equal(tmp_full[1].view(torch.int32), tmp_fwd[1].view(torch.int32))
    assert ((full - x).abs() > 1e-6).float().mean().item() > 0.01, "the mask never fired"


def _usm_bwd(L, x, saved, g, k1d, ksize=None, shape=None):
    n, c, h, w = shape or x.shape
    gx = torch.full(x.shape, SENTINEL, device="cuda")
    tmp2 = torch.empty(2 * x.numel(), device="cuda")
    ops = [t.contiguous().cuda() for t in (x, saved, g, k1d)]
    rc = L.lib().resr_usm_sharp_bwd(L.ptr(ops[0]), L.ptr(ops[1]), L.ptr(ops[2]), L.ptr(gx), L.ptr(tmp2), L.ptr(ops[3]),
                                    k1d.numel() if ksize is None else ksize, R.USM_WEIGHT, n, c, h, w, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, gx.cpu()


@pytest.mark.parametrize("name", sorted(R.USM_BWD_CASES))
def test_usm_backward_against_float64(L, name):
    """usm_bwd_prep_kernel + filter1d_adjoint_kernel on a constructed saved_tmp3 = [NaN: never read | blur | soft]; the forward's mask
    discontinuity plays no part."""
    x, blur, soft, g, k1d = R.usm_bwd_case(name)
    pre = R.usm_pre(x, blur)
    assert torch.minimum(pre.abs(), (pre - 1).abs()).min().item() > 1e-3
    assert min((pre < 0).double().mean().item(), ((pre > 0) & (pre < 1)).double().mean().item(), (pre > 1).double().mean().item()) >= 0.05
    saved = torch.stack([torch.full_like(x, float("nan")), blur, soft])
    rc, gx = _usm_bwd(L, x, saved, g, k1d)
    assert rc == L.RESR_OK, L.lib().resr_last_error()
    assert not (gx == SENTINEL).any()
    judge("usm_bwd", name, gx, R.usm_backward(x, blur, soft, g, k1d, R.USM_WEIGHT, F64), R.usm_backward(x, blur, soft, g, k1d, R.USM_WEIGHT, F32))


@pytest.mark.parametrize("what,shape,ksize", [("n = 0", (0, 1, 8, 8), 5), ("c = 0", (1, 0, 8, 8), 5), ("h = 0", (1, 1, 0, 8), 5),
                                              ("w < 0", (1, 1, 8, -8), 5), ("even ksize", (1, 1, 8, 8), 4), ("ksize 0", (1, 1, 8, 8), 0),
                                              ("ksize above 63", (1, 1, 80, 80), 65), ("pad = h", (1, 1, 25, 40), 51),
                                              ("pad = w", (1, 1, 40, 25), 51), ("pad > h", (1, 1, 2, 9), 7)])
def test_usm_backward_refuses_what_the_forward_refuses(L, what, shape, ksize):
    """Return codes only: both calls are rejected before any launch (the buffers are far larger than any of these geometries)."""
    x = torch.rand(1, 1, 80, 80)
    saved = torch.rand(3, 1, 1, 80, 80)
    k1d = torch.full((65,), 1.0 / 65)
    rc, gx = _usm_bwd(L, x, saved, x, k1d, ksize=ksize, shape=shape)
    assert rc == L.RESR_ERR_ARG, (what, rc)
    assert (gx == SENTINEL).all(), "a refused call wrote its output"
    n, c, h, w = shape
    for fn in (L.lib().resr_usm_sharp, L.lib().resr_usm_sharp_forward_only):          # the forward, for the same geometry
        xd, kd = x.cuda(), k1d.cuda()
        dst, tmp = torch.empty_like(xd), torch.empty(3 * xd.numel(), device="cuda")
        assert fn(L.ptr(xd), L.ptr(dst), L.ptr(tmp), L.ptr(kd), ksize, 0.5, 10.0, n, c, h, w, L.stream_ptr()) == L.RESR_ERR_ARG


# ---- resize -----------------------------------------------------------------------------------------------------------------------------
def run_resize(L, x, oh, ow, mode, scale):
    n, c, h, w = x.shape
    xd = x.contiguous().cuda()
    out = torch.full((n, c, oh, ow), SENTINEL, device="cuda")
    s = float(scale) if scale else 0.0
    L.check(L.lib().resr_resize(L.ptr(xd), L.ptr(out), n, c, h, w, oh, ow, R.RESIZE_MODES.index(mode), s, s, L.stream_ptr()), "resr_resize")
    torch.cuda.synchronize()
    out = out.cpu()
    assert not (out == SENTINEL).any(), "an output element was never written"
    return out


@pytest.mark.parametrize("mode", R.RESIZE_MODES)
@pytest.mark.parametrize("name", sorted(R.RESIZE_CASES))
def test_resize_against_float64(L, ip, name, mode):
    x, oh, ow, scale = R.resize_case(name)
    got = run_resize(L, x, oh, ow, mode, scale)
    judge("resize_kernel", f"{name}:{mode}", got, R.resize(x, oh, ow, mode, scale, F64), R.resize(x, oh, ow, mode, scale, F32))
    kw = {"scale_factor": scale} if scale else {"size": (oh, ow)}
    assert torch.equal(ip.interpolate(x.cuda(), mode=mode, **kw).cpu(), got)          # the module surface passes the same arguments


@pytest.mark.parametrize("mode", R.RESIZE_MODES)
def test_resize_to_the_same_size_is_the_identity(L, mode):
    """The bilinear coordinate is an integer there, the bicubic weights are exactly 0, 1, 0, 0, an area window holds one pixel."""
    x = torch.rand(2, 3, 33, 65, generator=_gen(11))
    assert torch.equal(run_resize(L, x, 33, 65, mode, None), x)
    assert torch.equal(run_resize(L, x, 33, 65, mode, 1.0), x)


def test_area_at_an_integer_factor_is_exact(L):
    x = torch.randint(0, 256, (2, 3, 64, 64), generator=_gen(12)).float() / 256
    want = x.double().view(2, 3, 16, 4, 16, 4).mean(dim=(3, 5))          # sums of 16 values with 8 fractional bits: no rounding anywhere
    assert torch.equal(run_resize(L, x, 16, 16, "area", None).double(), want)


# ---- Gaussian noise ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gauss_inputs():
    out = {}
    for c in (1, 3):
        g = _gen(20 + c)
        x = torch.rand(4, c, 24, 20, generator=g)
        sigma = torch.rand(4, generator=g) * 29 + 1
        gray = torch.tensor([1.0, 0.0, 1.0, 0.0])
        out[c] = (x, sigma, gray, torch.randn(24, 20, generator=g), torch.randn(4, c, 24, 20, generator=g))
    return out


@pytest.mark.parametrize("with_gray_field", [True, False])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_gaussian_noise_every_finish_mode(L, gauss_inputs, mode, c, with_gray_field):
    x, sigma, gray, fg, fc = gauss_inputs[c]
    fg = fg if with_gray_field else None
    dev = [t.cuda() if t is not None else None for t in (x, sigma, gray, fg, fc)]
    out = torch.full_like(dev[0], SENTINEL)
    L.check(L.lib().resr_noise_gaussian(L.ptr(dev[0]), L.ptr(out), L.ptr(dev[1]), L.ptr(dev[2]), L.ptr(dev[3]), L.ptr(dev[4]), 4, c, 24, 20, mode,
                                        L.stream_ptr()), "resr_noise_gaussian")
    torch.cuda.synchronize()
    got = out.cpu()
    assert not (got == SENTINEL).any()
    ref64 = R.gaussian_noise(x, sigma, gray, fg, fc, mode, F64)
    if mode < 2:
        judge("gauss_noise_kernel", f"mode{mode}:c{c}:{'gray_field' if with_gray_field else 'no_gray_field'}", got, ref64,
              R.gaussian_noise(x, sigma, gray, fg, fc, mode, F32))
        if mode == 1:
            assert got.min().item() >= 0.0 and got.max().item() <= 1.0 and (got == 0).any() and (got == 1).any()
        return
    # a rounded output is k / 255: the float64 reference's bits, except where the value it rounds sits on a half-integer
    p = R.pre_round(R.gaussian_noisy(x, sigma, gray, fg, fc, F64))
    tie = ((p - p.floor()) - 0.5).abs() <= 1e-4
    assert tie.double().mean().item() <= 1e-3, "too many elements of this seed's reference sit on a rounding tie"
    assert torch.equal(got[~tie], ref64.float()[~tie])
    assert ((got[tie].double() - ref64[tie]).abs() <= 1.0 / 255 + 1e-7).all()
    if mode == 2:
        assert got.min().item() < 0.0 and got.max().item() > 1.0, "nothing left [0, 1]: mode 2 was not told from mode 3"


# ---- Poisson noise ----------------------------------------------------------------------------------------------------------------------
def test_poisson_structure_element_wise(ip):
    g = _gen(30)
    x = torch.randint(0, 256, (3, 3, 40, 36), generator=g).float() / 255
    x[0, :, :4] = 0.0                                                              # level 0 always draws 0
    x[1] = (torch.randint(0, 64, (1, 40, 36), generator=g).float() * 4 / 255).expand(3, 40, 36)      # the gray sample: r = g = b
    x[1, :, :4] = 0.0
    scale, gray = torch.tensor([0.5, 2.0, 1.0]), torch.tensor([0.0, 1.0, 0.0])
    g255 = R.gray255(x[1:2])
    assert ((g255 - g255.floor()) - 0.5).abs().min().item() > 1e-3, "a gray level of the input sits on a rounding tie"

    def run(seed, mode):
        out, vals = ip.add_poisson_noise(x.cuda(), scale.cuda(), gray.cuda(), seed, bool(mode & 1), bool(mode & 2), return_vals=True)
        return out.cpu(), vals.cpu()
    out, vals = run(1234, 0)
    col, gr = R.poisson_decode(x, out, scale, gray, vals)
    for b in (0, 2):
        assert (col[b] - col[b].round()).abs().max().item() < 1e-3 and col[b].min().item() > -1e-3
        assert col[b].max().item() > 2 * vals[b, 0].item() / 256, "no draw of any size: nothing was decoded"
    assert torch.equal(out[0, :, :4], x[0, :, :4])
    d = out[1] - x[1]                                                              # the gray sample: one noise term for the three channels
    ulp = torch.from_numpy(np.spacing(d[0].abs().numpy()))
    assert ((d[1] - d[0]).abs() <= 2 * ulp).all() and ((d[2] - d[0]).abs() <= 2 * ulp).all()
    assert (gr[1] - gr[1].round()).abs().max().item() < 1e-3 and gr[1].min().item() > -1e-3 and gr[1].max().item() > 2
    assert torch.equal(out[1, :, :4], x[1, :, :4])
    again, _ = run(1234, 0)
    other, _ = run(1235, 0)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    assert (other != out).float().mean().item() > 0.5
    for mode in (1, 2, 3):
        got, _ = run(1234, mode)
        assert torch.equal(got, R.finish(out, mode, F32)), mode
    assert out.min().item() < 0.0 and out.max().item() > 1.0, "mode 0 clipped nothing: modes 1 and 3 were not exercised"


LAW_LEVELS = (0, 1, 5, 9, 10, 11, 60, 255)


@pytest.fixture(scope="module")
def poisson_draws(ip):
    """Draws of one 2 x 3 x 256 x 256 launch: (levels [2,3,255,256] int, counts [2,3,255,256] int).  Row 0 holds the levels 0 .. 255,
    so that v = 256 and lam = float32(L / 255) * 256 -- up to 256, on both sides of the sampler's switch at 10."""
    g = _gen(31)
    lv = torch.tensor(LAW_LEVELS)[torch.randint(0, len(LAW_LEVELS), (2, 3, 256, 256), generator=g)]
    lv[:, :, 0, :] = torch.arange(256)
    x = lv.float() / 255
    one = torch.ones(2)
    out, vals = ip.add_poisson_noise(x.cuda(), one.cuda(), torch.zeros(2).cuda(), 20240607, False, False, return_vals=True)
    assert torch.equal(vals[:, 0].cpu(), torch.tensor([256.0, 256.0]))
    col, _ = R.poisson_decode(x, out.cpu(), one, torch.zeros(2), vals.cpu())
    assert (col - col.round()).abs().max().item() < 1e-3 and col.min().item() > -1e-3
    return lv[:, :, 1:].numpy(), col.round().long()[:, :, 1:].numpy()


def _lam(level):
    return float(np.float32(level) / np.float32(255.0)) * 256.0


def _pooled_cells(lam, n):
    """Cells {0..lo}, {lo+1}, .., {hi-1}, {hi..} of the Poisson(lam) pmf with both tails pooled until each expects at least 5 of n:
    (lo, hi, probabilities)."""
    from scipy import stats
    top = int(lam + 12 * math.sqrt(lam) + 30)
    ks = np.arange(top + 1)
    cdf, sf = stats.poisson.cdf(ks, lam), stats.poisson.sf(ks - 1, lam)         # P(X <= k), P(X >= k)
    pmf = stats.poisson.pmf(ks, lam)
    lo = int(np.argmax((n * cdf[:-1] >= 5) & (n * pmf[1:] >= 5)))               # (the pmf has one mode: every cell between the two is larger)
    hi = int(np.max(np.nonzero((n * sf[1:] >= 5) & (n * pmf[:-1] >= 5))[0])) + 1
    assert lo < hi
    p = np.concatenate([[cdf[lo]], stats.poisson.pmf(np.arange(lo + 1, hi), lam), [sf[hi]]])
    assert abs(p.sum() - 1) < 1e-9 and (n * p).min() >= 5 - 1e-9
    return lo, hi, p


@pytest.mark.parametrize("level", LAW_LEVELS)
def test_poisson_law_per_level(poisson_draws, level, diag_dir):
    from scipy import stats
    levels, counts = poisson_draws
    d = counts[levels == level].astype(np.float64)
    n, lam = d.size, _lam(level)
    assert 45000 < n < 53000
    if level == 0:
        assert (d == 0).all()
        return
    z_mean = (d.mean() - lam) / math.sqrt(lam / n)
    z_var = (d.var(ddof=1) - lam) / math.sqrt((lam + 2 * lam * lam) / n)
    lo, hi, p = _pooled_cells(lam, n)
    obs = np.bincount(np.clip(d.astype(np.int64), lo, hi) - lo, minlength=hi - lo + 1)
    chi = float(((obs - n * p) ** 2 / (n * p)).sum())
    limit = float(stats.chi2.isf(1e-6, len(p) - 1))
    print(f"poisson level {level} lam {lam:.4f} n {n}: z_mean {z_mean:.2f} z_var {z_var:.2f} chi2 {chi:.1f} (dof {len(p) - 1}, limit {limit:.1f})")
    with open(os.path.join(diag_dir, f"poisson_law_{level}.json"), "w") as f:
        json.dump({"lam": lam, "n": int(n), "z_mean": z_mean, "z_var": z_var, "chi2": chi, "dof": len(p) - 1, "limit": limit}, f)
    assert abs(z_mean) <= 5 and abs(z_var) <= 5 and chi <= limit


def test_poisson_draws_are_uncorrelated(poisson_draws):
    levels, counts = poisson_draws
    lam = (levels.astype(np.float32) / np.float32(255.0)).astype(np.float64) * 256.0
    ok = levels > 0
    z = np.where(ok, (counts - lam) / np.sqrt(np.where(ok, lam, 1.0)), 0.0)          # standardised: mean 0, variance 1 whatever the level

    def corr(a, b, both):
        a, b = a[both], b[both]
        return float(np.corrcoef(a, b)[0, 1]), a.size
    for i, j in ((0, 1), (0, 2), (1, 2)):                                           # one thread draws a pixel's three channels in a row
        r, n = corr(z[:, i], z[:, j], ok[:, i] & ok[:, j])
        assert n > 90000 and abs(r) <= 5 / math.sqrt(n), ("channels", i, j, r, n)
    r, n = corr(z[..., :-1], z[..., 1:], ok[..., :-1] & ok[..., 1:])               # neighbouring threads: neighbouring Philox counters
    assert n > 250000 and abs(r) <= 5 / math.sqrt(n), ("neighbours", r, n)


# ---- resr_randn_fill -----------------------------------------------------------------------------------------------------------------------
def _randn(L, count, seed, stream, tail=8):
    buf = torch.full((count + tail,), SENTINEL, device="cuda")
    L.check(L.lib().resr_randn_fill(L.ptr(buf), count, seed, stream, L.stream_ptr()), "resr_randn_fill")
    torch.cuda.synchronize()
    return buf.cpu()


@pytest.mark.parametrize("count", [1, 2, 3, 5, 1023, 1025])
def test_randn_fill_writes_exactly_count_elements(L, count):
    buf = _randn(L, count, 77, 3)
    assert (buf[count:] == SENTINEL).all(), "wrote past the count"
    assert torch.isfinite(buf[:count]).all() and not (buf[:count] == SENTINEL).any()
    assert torch.equal(buf.view(torch.int32), _randn(L, count, 77, 3).view(torch.int32))
    whole = _randn(L, 1028, 77, 3)
    assert torch.equal(buf[:count], whole[:count])                                  # the count cuts the field, it does not change it
    if count > 3:
        assert (buf[:count] != _randn(L, count, 77, 4)[:count]).float().mean().item() > 0.9


def test_randn_fill_is_normal(L):
    from scipy import stats
    n = 1 << 20
    z = _randn(L, n, 2024, 0, tail=0).double().numpy()
    d = stats.kstest(z, "norm").statistic
    print(f"randn KS distance {d:.3e}, limit {stats.kstwobign.isf(1e-6) / math.sqrt(n):.3e}")
    assert d <= stats.kstwobign.isf(1e-6) / math.sqrt(n)
    q = z.reshape(-1, 4)
    for a, b in ((0, 1), (2, 3)):                                                   # the two outputs of one Box-Muller pair
        assert abs(np.corrcoef(q[:, a], q[:, b])[0, 1]) <= 5 / math.sqrt(n // 4)
    assert abs(np.corrcoef(z[:-1], z[1:])[0, 1]) <= 5 / math.sqrt(n - 1)
    other = _randn(L, n, 2024, 1, tail=0).double().numpy()
    assert abs(np.corrcoef(z, other)[0, 1]) <= 5 / math.sqrt(n)


# ---- JPEG -------------------------------------------------------------------------------------------------------------------------------
def test_jpeg_fused_clamp_is_the_clamp(ip):
    x = torch.rand(2, 3, 20, 37, generator=_gen(40)) * 1.6 - 0.3
    assert (x < 0).any() and (x > 1).any()
    jpeg, q = ip.DiffJPEG(False), torch.tensor([30.0, 80.0])
    y0, c0 = jpeg(x.cuda(), q.clone().cuda(), return_coeffs=True, clamp_input=True)
    y1, c1 = jpeg(x.clamp(0, 1).cuda(), q.clone().cuda(), return_coeffs=True)
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32)) and torch.equal(c0.view(torch.int32), c1.view(torch.int32))
    y2 = jpeg(x.cuda(), q.clone().cuda())
    assert not torch.equal(y2, y0), "the unclamped input gave the same image: the flag was not exercised"


def _macroblock_pixels(bad, h, w):
    """[N, blocks, 64] mask of coefficients -> [N, 1, h, w] mask of the pixels of every 16 x 16 macroblock that holds one."""
    n = bad.shape[0]
    mby, mbx = (h + 15) // 16, (w + 15) // 16
    blk = bad.any(dim=2)
    ny = mby * 2 * mbx * 2
    ymask = blk[:, :ny].view(n, mby, 2, mbx, 2).any(dim=4).any(dim=2)
    cmask = blk[:, ny:].view(n, 2, mby, mbx).any(dim=1)
    mb = ymask | cmask
    return mb.repeat_interleave(16, dim=1).repeat_interleave(16, dim=2)[:, None, :h, :w]


@pytest.mark.parametrize("shape,qualities", [((3, 3, 5, 7), (49.99, 50.0, 50.01)), ((1, 3, 16, 23), (10.0,)), ((1, 3, 16, 23), (95.0,))])
def test_jpeg_coefficients_round_the_float64_dct(ip, shape, qualities):
    """Images smaller than a macroblock, a quality on either side of the factor's switch at 50, the coarsest and the finest tables."""
    from oracle import imgproc_ref as I
    x = torch.rand(shape, generator=_gen(41))
    q = torch.tensor(qualities)
    pre = R.jpeg_preround(x, q)
    tie = ((pre - pre.floor()) - 0.5).abs() <= 1e-3
    assert int(tie.sum()) <= 2, "this seed's reference has too many coefficients on a rounding tie"
    y, c = ip.DiffJPEG(False)(x.cuda(), q.clone().cuda(), return_coeffs=True)
    y, c = y.cpu(), c.cpu()
    assert c.shape == pre.shape
    assert torch.equal(c.double()[~tie], torch.round(pre)[~tie])
    assert ((c.double() - pre).abs()[tie] <= 0.5 + 1e-3).all()
    assert (c != 0).float().mean().item() > 0.02, "every coefficient is zero: nothing was quantised"
    want, oc = I.diff_jpeg(x, q, return_coeffs=True)
    differ = c != torch.cat([oc["y"], oc["cb"], oc["cr"]], dim=1).reshape(c.shape)
    same = ~_macroblock_pixels(differ, shape[2], shape[3]).expand(shape)
    assert same.float().mean().item() > 0.5
    assert ((y - want).abs()[same] <= 1.0 / 255).all()


# ---- quantise + crop ------------------------------------------------------------------------------------------------------------------------
def _crop_values(shape, g):
    """[-0.5, 1.5] with -0.0 and values whose product with 255 is exactly k + 0.5 in float32 (round-half-even decides them)."""
    v = torch.rand(shape, generator=g) * 2 - 0.5
    flat = v.view(-1)
    k = torch.arange(-3, 259).float()
    ties = ((k + 0.5) / 255).float()
    ties = ties[(ties * 255) == (k + 0.5)]
    assert ties.numel() > 60 and flat.numel() > 2 * ties.numel() + 4
    flat[1:1 + ties.numel()] = ties
    flat[-ties.numel():] = ties
    flat[0] = -0.0
    flat[1 + ties.numel()] = -0.0
    return v


@pytest.mark.parametrize("upscale,lr_hw", [(2, (18, 22)), (4, (9, 11))])
def test_quantize_crop_is_the_host_formula(ip, upscale, lr_hw):
    """Odd HR offsets (the LR window starts at offset // upscale), both windows ending on their image's last row and column."""
    g = _gen(50 + upscale)
    lr, hr = _crop_values((2, 3) + lr_hw, g), _crop_values((2, 3, 37, 45), g)
    top, left, size = 21, 29, 16
    assert top + size == 37 and left + size == 45 and top // upscale + size // upscale == lr_hw[0] and left // upscale + size // upscale == lr_hw[1]
    plr, phr = ip.quantize_crop(lr.cuda(), hr.cuda(), size, upscale, top, left)
    lt, ll, ls = top // upscale, left // upscale, size // upscale
    want = (torch.round(lr * 255.0).clamp(0, 255) / 255.0)[:, :, lt:lt + ls, ll:ll + ls]
    assert torch.equal(plr.cpu(), want) and (want == 0).any() and (want == 1).any()
    assert torch.equal(phr.cpu().view(torch.int32), hr[:, :, top:top + size, left:left + size].contiguous().view(torch.int32))


def test_quantize_crop_identity_window_and_refusals(ip):
    lr, hr = torch.rand(1, 3, 8, 8).cuda(), torch.rand(1, 3, 32, 32).cuda()
    plr, phr = ip.quantize_crop(lr, hr, 32, 4, 0, 0)
    assert phr is hr and torch.equal(plr.cpu(), torch.round(lr.cpu() * 255.0).clamp(0, 255) / 255.0)
    for top, left, size in ((17, 0, 16), (0, 17, 16), (-1, 0, 16), (0, -4, 16), (0, 0, 36)):       # rejected before any launch
        with pytest.raises(RuntimeError, match="window outside the image"):
            ip.quantize_crop(lr, hr, size, 4, top, left)
    small = torch.rand(1, 3, 3, 8).cuda()                                                             # the HR window fits, the LR window does not
    with pytest.raises(RuntimeError, match="window outside the image"):
        ip.quantize_crop(small, hr, 16, 4, 0, 0)
