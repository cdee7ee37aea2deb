"""numpy / float64 restatement of the native NIQE tail (csrc/niqe.hip, resr_niqe_score) stage by stage -- NaN-aware mean, the rows
without a NaN, two-pass covariance, A = (cov_prior + cov) / 2 -- with the first-order bounds the tests hold the kernels to, and a
60-digit ground truth of the score.  No GPU, no library.

Bounds, in the form of tests/niqe_ref.py: u = 2^-53; a float64 sum of n terms lies within n u sum|term| of the exact sum in any order,
with or without fused multiply-adds; every bound below is that expression propagated to first order, times SLACK = 4.
"""
import numpy as np

from tests.niqe_ref import SLACK, U

F = 36
EPS = 2.0 ** -52


def synthetic_feats(mu_prior, chol, b, blocks, seed):
    """[b, blocks, 36]: rows mu_prior + 1.3 L z + 0.1 with z standard normal under a fixed seed."""
    z = np.random.default_rng(seed).standard_normal((b, blocks, F))
    return mu_prior + 1.3 * z @ chol.T + 0.1


def stages_np(rows, mu_prior, cov_prior):
    """One image's features [blocks, 36] (NaNs allowed) -> dict: mu_d and its bound, the ok mask and m, cov_d, A and its bound
    (element-wise), diff.  With m <= 1 the covariance is what the torch tail computes: 0 / 0 (m = 1) or -0 (m = 0)."""
    nan = np.isnan(rows)
    clean = np.where(nan, 0.0, rows)
    cnt = (~nan).sum(0).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mu_d = clean.sum(0) / cnt
        mu_bound = SLACK * (cnt * U * np.abs(clean).sum(0) / cnt + U * np.abs(mu_d))
        ok = ~nan.any(1)
        x = rows[ok]
        m = x.shape[0]
        mean_ok = x.sum(0) / m
        c = x - mean_ok
        cov_d = c.T @ c / (m - 1)
        a = (cov_prior + cov_d) / 2
        # the error of a centred element: that of the column mean (m u sum|x| / m) and the subtraction's own rounding
        e_c = m * U * np.abs(x).sum(0) / max(m, 1) + U * np.abs(c)
        e_sum = m * U * (np.abs(c).T @ np.abs(c)) + np.abs(c).T @ e_c + e_c.T @ np.abs(c)
        a_bound = SLACK * (e_sum / (m - 1) + U * (np.abs(cov_prior) + np.abs(cov_d))) / 2
    return {"mu_d": mu_d, "mu_bound": mu_bound, "ok": ok, "m": m, "cov_d": cov_d, "A": a, "A_bound": a_bound, "diff": mu_prior - mu_d}


def truth_score(a, diff, keep=None):
    """sqrt(d^T A^-1 d) by an LU solve at 60 digits, restricted to the indices `keep` (default: all) -> mpmath number."""
    import mpmath as mp
    idx = list(range(F)) if keep is None else list(keep)
    with mp.workdps(60):
        am = mp.matrix([[mp.mpf(float(a[i, j])) for j in idx] for i in idx])
        dm = mp.matrix([mp.mpf(float(diff[i])) for i in idx])
        return mp.sqrt((dm.T * mp.lu_solve(am, dm))[0])


def relative_distance(score, truth):
    import mpmath as mp
    with mp.workdps(60):
        return float(abs(mp.mpf(float(score)) - truth) / truth)


def score_bound(a):
    """(bound, cond, eigenvalues): the relative distance from the ground truth a score may show, 4 * 36 * u * cond(A): the first-order
    effect of a backward error of 36 eps ||A|| on d^T A^-1 d, halved by the square root, doubled for the mean and covariance stages."""
    ev = np.linalg.eigvalsh(a)
    cond = float(np.abs(ev).max() / np.abs(ev).min())
    return 4 * F * U * cond, cond, ev
