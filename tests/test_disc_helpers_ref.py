"""CPU: the float64 references of tests/disc_helpers_ref.py against torch, before they judge a kernel (tests/test_gpu_disc_helpers.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import disc_helpers_ref as ref


def _nchw(x_nhwc):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(x_nhwc, (0, 3, 1, 2))))


def _nhwc(t_nchw):
    return t_nchw.permute(0, 2, 3, 1).contiguous().numpy()


@pytest.mark.parametrize("n,h,w,c,cout", [(1, 2, 2, 1, 1), (2, 6, 10, 3, 5), (1, 8, 4, 4, 2)])
def test_s2d_conv_identity_and_fold(n, h, w, c, cout):
    """What justifies space-to-depth and fold4x4: the 4x4 stride-2 pad-1 conv IS the 3x3 pad-1 conv of the packed image with the
    virtual kernel, and folding the virtual kernel gives the real one back exactly."""
    rng = np.random.default_rng(h * 10 + w)
    x = rng.standard_normal((n, h, w, c))
    w4 = rng.standard_normal((cout, c, 4, 4))
    direct = F.conv2d(_nchw(x), torch.from_numpy(w4), stride=2, padding=1)
    w3 = ref.virtual_ref(w4)
    packed = F.conv2d(_nchw(ref.s2d_ref(x)), torch.from_numpy(w3), padding=1)
    assert direct.shape == packed.shape
    assert (direct - packed).abs().max().item() <= 1e-12
    assert np.array_equal(ref.fold_ref(w3), w4)
    assert np.array_equal(ref.d2s_ref(ref.s2d_ref(x)), x)
    # every virtual tap that carries a real one carries exactly one: 16 of the 36 (tap, block) slots per channel
    assert np.count_nonzero(ref.virtual_ref(np.ones((1, 1, 4, 4)))) == 16


def _tie_rich(rng, shape):
    """Integers 0..3, with some windows all equal and some all zero (as after a ReLU)."""
    n, h, w, c = shape
    x = rng.integers(0, 4, size=shape).astype(np.float64)
    win = rng.integers(0, 4, size=(n, h // 2, w // 2, c))
    for dy in range(2):
        for dx in range(2):
            v = x[:, dy::2, dx::2, :]
            v[win == 0] = 2.0
            v[win == 1] = 0.0
    return x


@pytest.mark.parametrize("shape", [(1, 2, 2, 1), (2, 6, 10, 3), (1, 14, 6, 8)])
def test_maxpool_ref_matches_torch_on_ties(shape):
    rng = np.random.default_rng(shape[1])
    for x in (_tie_rich(rng, shape), rng.standard_normal(shape)):
        dst, arg = ref.maxpool_ref(x)
        tdst, tidx = F.max_pool2d(_nchw(x), 2, 2, return_indices=True)
        assert np.array_equal(dst, _nhwc(tdst))
        n, h, w, c = shape
        iy, ix = _nhwc(tidx // w), _nhwc(tidx % w)
        yy = np.arange(h // 2)[None, :, None, None]
        xx = np.arange(w // 2)[None, None, :, None]
        assert np.array_equal(arg, (iy - 2 * yy) * 2 + (ix - 2 * xx))
        # the scatter backward against autograd
        g = rng.standard_normal(dst.shape)
        xt = _nchw(x).requires_grad_(True)
        torch.max_pool2d(xt, 2, 2).backward(_nchw(g))
        assert np.array_equal(ref.maxpool_bwd_ref(g, arg), _nhwc(xt.grad))
    assert (ref.maxpool_ref(np.zeros(shape))[1] == 0).all()


@pytest.mark.parametrize("rows,cols", [(1, 1), (5, 7), (33, 257)])
def test_spectral_norm_ref_matches_torch_module(rows, cols):
    """One training forward of a float64 torch.nn.utils.spectral_norm module: u, v and the normalised weight; then the eval-mode
    sigma from the same u, v; and the backward formula against autograd through W / sigma with u, v constant."""
    torch.manual_seed(rows)
    lin = torch.nn.Linear(cols, rows, bias=False).double()
    m = torch.nn.utils.spectral_norm(lin, eps=1e-12)
    w = m.weight_orig.detach().numpy().copy()
    u0, v0 = m.weight_u.numpy().copy(), m.weight_v.numpy().copy()
    m.train()
    m(torch.zeros(1, cols, dtype=torch.float64))
    u, v, sigma = ref.spectral_norm_ref(w, u0, v0, True, 1e-12)
    assert np.abs(u - m.weight_u.numpy()).max() <= 1e-14
    assert np.abs(v - m.weight_v.numpy()).max() <= 1e-14
    assert np.abs(w / sigma - m.weight.detach().numpy()).max() <= 1e-13 * np.abs(w / sigma).max()
    ue, ve, sigma_e = ref.spectral_norm_ref(w, u, v, False, 1e-12)
    assert np.array_equal(ue, u) and np.array_equal(ve, v) and abs(sigma_e - sigma) <= 1e-15 * abs(sigma)
    # backward: d/dW_orig of <G, W_orig / (u^T W_orig v)>
    g = np.random.default_rng(cols).standard_normal((rows, cols))
    wt = torch.from_numpy(w).requires_grad_(True)
    ut, vt = torch.from_numpy(u), torch.from_numpy(v)
    ((wt / (ut @ (wt @ vt))) * torch.from_numpy(g)).sum().backward()
    mine = ref.spectral_norm_bwd_ref(g, w, u, v, sigma)
    # measured against the terms, not the result: for 1 x 1 the two terms cancel to rounding noise
    assert np.abs(mine - wt.grad.numpy()).max() <= 1e-12 * np.abs(g / sigma).max()


def test_spectral_norm_ref_eps_branch():
    rng = np.random.default_rng(0)
    w = rng.standard_normal((5, 7)) * 1e-20
    u0 = rng.standard_normal(5)
    u0 /= np.linalg.norm(u0)
    u, v, _ = ref.spectral_norm_ref(w, u0, np.zeros(7), True, 1e-12)
    assert np.allclose(v, (w.T @ u0) / 1e-12, rtol=1e-15, atol=0) and np.linalg.norm(v) < 1e-6


@pytest.mark.parametrize("shape", [(2, 7, 5, 3), (1, 1, 9, 2), (3, 6, 1, 1), (1, 1, 1, 2), (1, 2, 2, 1)])
def test_bilinear_ref_matches_torch_and_adjoint(shape):
    rng = np.random.default_rng(shape[1] * 10 + shape[2])
    x = rng.standard_normal(shape)
    xt = _nchw(x).requires_grad_(True)
    up = F.interpolate(xt, scale_factor=2, mode="bilinear", align_corners=False)
    mine = ref.bilinear_up_ref(x)
    assert mine.shape == (shape[0], 2 * shape[1], 2 * shape[2], shape[3])
    assert np.abs(mine - _nhwc(up.detach())).max() <= 1e-14
    g = rng.standard_normal(mine.shape)
    up.backward(_nchw(g))
    back = ref.bilinear_up_bwd_ref(g)
    assert np.abs(back - _nhwc(xt.grad)).max() <= 1e-14
    assert abs((mine * g).sum() - (x * back).sum()) <= 1e-12 * max(1.0, abs((mine * g).sum()))
    assert np.allclose(ref.bilinear_matrix(shape[1]).sum(axis=1), 1.0, rtol=0, atol=1e-15)      # every output is an average


def test_add_mask_ref():
    a, b = np.array([1.0, -2.0, 3.0, 0.5]), np.array([0.5, 0.5, -4.0, 0.0])
    m = np.array([1.0, 0.0, -0.0, -3.0])
    assert np.array_equal(ref.add_mask_ref(a, b, m > 0, 0.25), np.array([1.5, -0.375, -0.25, 0.125]))
    assert np.array_equal(ref.add_mask_ref(a, None, None, 0.25), a)
    mt = torch.from_numpy(m).requires_grad_(True)
    F.leaky_relu(mt, 0.25).backward(torch.from_numpy(a + b))
    assert np.array_equal(ref.add_mask_ref(a, b, m > 0, 0.25), mt.grad.numpy())


def test_pair_round_trip_bound():
    """pair_join(pair_split(v)) is within 2^-22 |v| of v for |v| in [2^-6, 2^6].

    hi = f16(v) has 11 significand bits: |v - hi| <= 2^-11 |v|.  The remainder times 2^12 is at most 2 |v| <= 2^7 in magnitude -- no f16
    overflow -- and lo = f16(remainder * 2^12) loses at most 2^-11 of it while normal (>= 2^-14), at most 2^-25 absolutely below that.
    Divided by 2^12 again: 2^-11 * 2^-11 |v| = 2^-22 |v|, or 2^-37, which for |v| >= 2^-6 is below 2^-22 |v| >= 2^-28."""
    rng = np.random.default_rng(3)
    mag = 2.0 ** rng.uniform(-6, 6, size=200_000)
    v = np.concatenate([mag * rng.choice([-1.0, 1.0], size=mag.size), [2.0 ** -6, -2.0 ** -6, 2.0 ** 6, -2.0 ** 6, 1.0, 1.0 + 2.0 ** -11,
                                                                       1.0 + 2.0 ** -10 + 2.0 ** -23]])
    hi, lo = ref.pair_split(v)
    assert hi.dtype == np.float16 and lo.dtype == np.float16
    err = np.abs(ref.pair_join(hi, lo) - v)
    assert (err <= 2.0 ** -22 * np.abs(v)).all(), (err / np.abs(v)).max()
    assert (err <= ref.pair_bound(v)).all()
    assert (err / np.abs(v)).max() > 2.0 ** -25            # the bound is not vacuous: the worst case sits within 8x of it
    # below the range the absolute term takes over, and the general bound still holds
    small = 2.0 ** rng.uniform(-30, -6, size=20_000)
    hs, ls = ref.pair_split(small)
    assert (np.abs(ref.pair_join(hs, ls) - small) <= ref.pair_bound(small)).all()
    # fp32 values split the way the kernels split them (fp32 subtraction and scaling are exact here): the same pair
    v32 = v.astype(np.float32)
    h32 = v32.astype(np.float16)
    l32 = ((v32 - h32.astype(np.float32)) * np.float32(4096)).astype(np.float16)
    h64, l64 = ref.pair_split(v32.astype(np.float64))
    assert np.array_equal(h32, h64) and np.array_equal(l32, l64)


def test_pair_sign_rule():
    f = np.float16
    hi = np.array([0.0, 0.0, -0.0, 0.0, 6e-8, 1.0, -1.0, -0.0], dtype=f)
    lo = np.array([0.5, -0.5, 0.5, 0.0, -0.5, -8.0, 8.0, -0.0], dtype=f)
    assert ref.pair_positive(hi, lo).tolist() == [True, False, True, False, True, True, False, False]


def test_reductions_ref():
    p = np.arange(12, dtype=np.float64).reshape(3, 4)
    assert np.array_equal(ref.weighted_rows_ref(p, [1.0, 0.5, 2.0]), np.array([6.0, 11.0, 76.0, 93.0]))
    assert ref.l1_sum_ref([1.0, -2.0, 3.0], [0.5, 2.0, 3.0]) == 4.5
