"""GP.cv_predict without a device: a NumPy restatement of leave-fold-out prediction on Posterior fields (cv_numpy:
with P = (K + Sigma)^-1 the held-out set I has covariance (P_II)^-1 and mean y_I - (P_II)^-1 alpha_I), checked
against brute force through the oracle (a posterior on the data without the fold, its predictive mean, full covariance
and joint density at the fold) and against values the reference itself produced (tests/golden/cv_cases.npz); the
fold normalisation and the host assembly of GP.cv_predict behind a stand-in for the device.
test_gpu_cv.py compares the device against the same restatement."""

import os
import warnings

import numpy as np
import pytest
from scipy.linalg import cholesky, solve_triangular

from gp_stubs import _NoDevice, _se_gp
from test_quad_grad_cpu import _counts, solve_posterior

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-8  # the project's fp64 parity bound


def cv_numpy(posts, y, folds=None):
    """gpc_cv restated on Posterior fields (alpha, L, sW, L_chol), P read as oracle.predict reads them:
    (dmu, s2 (N, S), NaN at points in no fold; quad, logdet (F, S)).  ``folds`` None: leave-one-out."""
    N, S = np.size(y), len(posts)
    folds = [np.array([i]) for i in range(N)] if folds is None else [np.sort(np.asarray(f)) for f in folds]
    dmu, s2 = np.full((N, S), np.nan), np.full((N, S), np.nan)
    quad, logdet = np.zeros((len(folds), S)), np.zeros((len(folds), S))
    for s, p in enumerate(posts):
        P = solve_posterior(p, np.eye(N))
        P = 0.5 * (P + P.T)
        a = np.asarray(p.alpha).reshape(-1)
        for f, I in enumerate(folds):
            R = cholesky(P[np.ix_(I, I)], lower=True)
            Wf = solve_triangular(R, np.eye(I.size), lower=True)
            u = Wf @ a[I]
            dmu[I, s] = Wf.T @ u
            s2[I, s] = np.sum(Wf * Wf, 0)
            quad[f, s] = u @ u
            logdet[f, s] = -2 * np.sum(np.log(np.diag(R)))
    return dmu, s2, quad, logdet


def lpd_fold_of(quad, logdet, folds, N):
    k = np.ones((N, 1)) if folds is None else np.array([[np.size(f)] for f in folds], dtype=float)
    return -0.5 * quad - 0.5 * logdet - 0.5 * k * np.log(2 * np.pi)


def cv_bruteforce(model, hyps, X, y, s2, folds, mults):
    """What a user does without cv_predict, through the oracle: for every fold the posteriors on the data without it
    (at the full posterior's jitter multiplier), the predictive mean and the full noisy covariance at the fold, and the
    joint log density of the fold's targets: (mu, s2 (N, S), lpd_fold (F, S))."""
    from oracle import gp_oracle as orc

    N, D = X.shape
    S = hyps.shape[0]
    cov_N, noise_N, mean_N = _counts(model, D)
    folds = [np.array([i]) for i in range(N)] if folds is None else folds
    mu, v = np.full((N, S), np.nan), np.full((N, S), np.nan)
    lpd = np.zeros((len(folds), S))
    for f, I in enumerate(folds):
        keep = np.setdiff1d(np.arange(N), I)
        posts = orc.posteriors(model, hyps, X[keep], y[keep], None if s2 is None else s2[keep], force_mult=mults)
        for s, p in enumerate(posts):
            h = p.hyp
            m = np.reshape(orc.mean(model["mean"], h[cov_N + noise_N:cov_N + noise_N + mean_N], X[I]), (-1,))
            Ks = orc.covariance(model["kernel"], h[:cov_N], X[keep], X[I], degree=model.get("degree", 0))
            Kss = orc.covariance(model["kernel"], h[:cov_N], X[I], degree=model.get("degree", 0))
            mf = m + Ks.T @ p.alpha[:, 0]
            if p.L_chol:
                V = solve_triangular(p.L, np.reshape(p.sW, (-1, 1)) * Ks, trans=1)
                C = Kss - V.T @ V
            else:
                C = Kss + Ks.T @ (p.L @ Ks)
            sn2 = orc.noise(model["noise"], h[cov_N:cov_N + noise_N], X[I], y[I], None if s2 is None else s2[I])
            C = C + np.diag(np.ravel(np.broadcast_to(sn2, (I.size, 1)))) * p.sn2_mult
            mu[I, s], v[I, s] = mf, np.diag(C)
            R = cholesky(0.5 * (C + C.T), lower=True)
            u = solve_triangular(R, y[I, 0] - mf, lower=True)
            lpd[f, s] = -0.5 * u @ u - np.sum(np.log(np.diag(R))) - 0.5 * I.size * np.log(2 * np.pi)
    return mu, v, lpd


def cv_data(kernel="se", degree=0, mean="const", N=200, D=3, S=3, seed=1, s2=False, sn2=None):
    """The generator of tests/test_gpu_quad_grad.py's ``_problem`` (same draws in the same order), without the GP."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (N, D))
    y = np.sin(X.sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1))
    model = dict(kernel=kernel, degree=degree, mean=mean, noise=(1, 1 if s2 else 0, 0))
    cov_N, noise_N, mean_N = _counts(model, D)
    hyp = np.zeros((S, cov_N + noise_N + mean_N))
    hyp[:, :cov_N - 1] = np.log(1.2)
    hyp[:, cov_N] = np.log(0.1)
    if mean != "zero":
        hyp[:, cov_N + noise_N] = 0.3
    hyp += 0.05 * rng.standard_normal(hyp.shape)
    if sn2 is not None:
        hyp[:, cov_N] = 0.5 * np.log(sn2)
    s2v = 0.01 * (1 + rng.uniform(0, 1, (N, 1))) if s2 else None
    return model, X, y, s2v, hyp


def scattered_folds(N, sizes, seed=5):
    """Disjoint scattered folds of the given sizes from a seeded permutation, each sorted."""
    perm = np.random.default_rng(seed).permutation(N)
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    assert cuts[-1] <= N
    return [np.sort(perm[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]


def check_against(ref, got, folds, N, label=""):
    """The issue's bounds: mu per fold (max over the fold), s2 per element, the density per fold, all 1e-8 relative."""
    mu_r, s2_r, lpd_r = ref
    mu_g, s2_g, lpd_g = got
    fl = [np.array([i]) for i in range(N)] if folds is None else folds
    worst = 0.0
    for f, I in enumerate(fl):
        for s in range(mu_r.shape[1]):
            e = np.abs(mu_g[I, s] - mu_r[I, s]).max() / np.abs(mu_r[I, s]).max()
            worst = max(worst, e)
            assert e <= RTOL, (label, "mu", f, s, e)
            e = np.abs(lpd_g[f, s] - lpd_r[f, s]) / abs(lpd_r[f, s])
            worst = max(worst, e)
            assert e <= RTOL, (label, "lpd_fold", f, s, e)
    cov = np.concatenate(fl)
    e = (np.abs(s2_g[cov] - s2_r[cov]) / np.abs(s2_r[cov])).max()
    assert e <= RTOL, (label, "s2", e)
    return max(worst, e)


def restated(model, hyps, X, y, s2, folds):
    from oracle import gp_oracle as orc

    posts = orc.posteriors(model, hyps, X, y, s2)
    dmu, v, quad, logdet = cv_numpy(posts, y, folds)
    return posts, (y - dmu, v, lpd_fold_of(quad, logdet, folds, X.shape[0]))


@pytest.mark.parametrize("case", ["se", "matern5", "s2"])
def test_restatement_matches_brute_force(case):
    kw = dict(se=dict(N=200, S=2), matern5=dict(kernel="matern", degree=5, N=120, S=2), s2=dict(N=120, S=2, s2=True))[case]
    model, X, y, s2, hyp = cv_data(**kw)
    N = X.shape[0]
    for folds in (None, scattered_folds(N, [1, 15, 17, N // 3]), list(np.array_split(np.arange(N), 5))):
        posts, got = restated(model, hyp, X, y, s2, folds)
        assert all(p.L_chol for p in posts)
        ref = cv_bruteforce(model, hyp, X, y, s2, folds, [p.sn2_mult for p in posts])
        worst = check_against(ref, got, folds, N, case)
        print(case, "LOO" if folds is None else len(folds), "worst relative error %.2e" % worst)


def test_restatement_and_oracle_match_the_reference_fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "cv_cases.npz"), allow_pickle=False)
    model = dict(kernel="se", degree=0, mean="const", noise=(1, 0, 0))
    X, y, hyp = g["X"], g["y"], g["hyp"]
    for name in g["names"]:
        ptr, idx = g[f"{name}_ptr"], g[f"{name}_idx"]
        folds = [idx[a:b] for a, b in zip(ptr[:-1], ptr[1:])]
        ref = g[f"{name}_mu"], g[f"{name}_s2"], g[f"{name}_lpd_fold"]
        posts, got = restated(model, hyp, X, y, None, folds)
        check_against(ref, got, folds, X.shape[0], f"{name} restatement")
        brute = cv_bruteforce(model, hyp, X, y, None, folds, [p.sn2_mult for p in posts])
        check_against(ref, brute, folds, X.shape[0], f"{name} oracle")


def test_fold_normalisation_and_its_errors():
    from gpyreg_amd.gaussian_process import _cv_folds

    assert _cv_folds(None, 10) is None
    fl = _cv_folds(3, 10)
    assert [f.tolist() for f in fl] == [[0, 1, 2, 3], [4, 5, 6], [7, 8, 9]]
    fl = _cv_folds([[5, 2], np.array([9]), (0, 7, 1)], 10)
    assert [f.tolist() for f in fl] == [[2, 5], [9], [0, 1, 7]] and all(f.dtype == np.int64 for f in fl)
    for bad, msg in ((1, r"must lie in \[2, N = 10\]"), (11, r"must lie in \[2, N = 10\]"), ([], "empty sequence"),
                     ([[1], []], "fold 1 is empty"), ([[0, 10]], r"fold 0 has index 10 out of range \[0, 10\)"),
                     ([[1], [-1, 2]], "fold 1 has index -1 out of range"), ([[1, 2], [3, 2]], "fold 1 overlaps fold 0 at index 2"),
                     ([[4, 4]], "fold 0 repeats index 4"), ([list(range(10))], "fold 0 holds all 10 points"),
                     ([[0.5]], "fold 0 must hold integer indices"), (2.5, "None, an int or a sequence")):
        with pytest.raises(ValueError, match=msg):
            _cv_folds(bad, 10)


class _Handle:
    """Stands in for the device posteriors: PostHandle.cv from the restatement."""

    def __init__(self, posts, y, bad=None):
        self.posts, self.y, self.bad = posts, y, bad

    def cv(self, folds):
        dmu, s2, quad, logdet = cv_numpy(self.posts, self.y, folds)
        info = np.zeros(quad.shape, dtype=np.int32)
        if self.bad is not None:
            f, s = self.bad
            info[f, s] = 3
            quad[f, s] = logdet[f, s] = np.nan
            I = np.array([f]) if folds is None else folds[f]
            dmu[I, s] = s2[I, s] = np.nan
        return dmu, s2, quad, logdet, info

    def free(self):
        pass


def _host_gp(monkeypatch, S=3, bad=None):
    from gpyreg_amd import _lib
    from oracle import gp_oracle as orc

    monkeypatch.setattr(_lib, "context", lambda device=None: _NoDevice())
    model, X, y, _, hyp = cv_data(N=40, D=2, S=S)
    posts = orc.posteriors(model, hyp, X, y, None)
    gp = _se_gp(D=2)
    gp.update(X_new=X, y_new=y, hyp=hyp, compute_posterior=False)
    monkeypatch.setattr(gp, "_ctx", lambda: None)
    gp._post_handle = _Handle(posts, y, bad)
    return gp, model, posts, X, y, hyp


def test_host_assembly_mixture_lpd_and_uncovered_points(monkeypatch):
    from gpyreg_amd.gaussian_process import _mix_samples

    gp, model, posts, X, y, hyp = _host_gp(monkeypatch)
    try:
        N, S = X.shape[0], hyp.shape[0]
        folds = scattered_folds(N, [1, 7, 12])
        covered = np.concatenate(folds)
        rest = np.setdiff1d(np.arange(N), covered)
        dmu, v, quad, logdet = cv_numpy(posts, y, folds)
        sn2 = np.exp(2 * hyp[:, 3])[None, :]
        mu, s2, lpd, lpf = gp.cv_predict(folds, separate_samples=True, return_lpd=True)
        assert mu.shape == s2.shape == lpd.shape == (N, S) and lpf.shape == (3, S)
        assert np.array_equal(mu[covered], (y - dmu)[covered]) and np.array_equal(s2[covered], np.maximum(v - sn2, 0)[covered])
        assert np.all(np.isnan(mu[rest])) and np.all(np.isnan(s2[rest])) and np.all(np.isnan(lpd[rest]))
        assert np.allclose(lpd[covered], (-0.5 * dmu**2 / v - 0.5 * np.log(2 * np.pi * v))[covered], rtol=1e-14)
        assert np.array_equal(lpf, lpd_fold_of(quad, logdet, folds, N))
        assert np.array_equal(gp.cv_predict(folds, add_noise=True, separate_samples=True)[1][covered], v[covered])
        # the mixture over samples, as predict forms it
        m1, s1, l1, f1 = gp.cv_predict(folds, return_lpd=True)
        mm, sm, between = _mix_samples(y - dmu, np.maximum(v - sn2, 0))
        assert m1.shape == s1.shape == l1.shape == (N, 1) and f1.shape == (3, 1)
        assert np.array_equal(m1[covered], mm[covered]) and np.array_equal(s1[covered], sm[covered])
        noisy = np.reshape(np.sum(v, 1) / S + between, (-1, 1))
        assert np.allclose(l1[covered], (-0.5 * (y - mm) ** 2 / noisy - 0.5 * np.log(2 * np.pi * noisy))[covered], rtol=1e-14)
        assert np.allclose(f1[:, 0], np.log(np.mean(np.exp(lpf), 1)), rtol=1e-13)  # the exact equal-weight mixture
        m2, s2n, l2, _ = gp.cv_predict(folds, add_noise=True, return_lpd=True)
        assert np.allclose(s2n[covered], noisy[covered], rtol=1e-14) and np.allclose(l2[covered], l1[covered], rtol=1e-13)
        # leave-one-out, an int, and the single fold of the 1-point form
        mu_l, s2_l, lpd_l, lpf_l = gp.cv_predict(None, add_noise=True, separate_samples=True, return_lpd=True)
        assert lpf_l.shape == (N, S) and np.allclose(lpf_l, lpd_l, rtol=1e-12)
        assert not np.any(np.isnan(mu_l))
        mu_k = gp.cv_predict(4, separate_samples=True)[0]
        ref_k = y - cv_numpy(posts, y, list(np.array_split(np.arange(N), 4)))[0]
        assert np.array_equal(mu_k, ref_k)
        one = gp.cv_predict([[folds[0][0]]], add_noise=True, separate_samples=True)
        assert np.allclose(one[0][folds[0]], mu_l[folds[0]], rtol=1e-12) and np.allclose(one[1][folds[0]], s2_l[folds[0]], rtol=1e-12)
        with pytest.raises(ValueError, match="fold 1 overlaps fold 0"):
            gp.cv_predict([[1, 2], [2, 3]])
    finally:
        gp._post_handle = None


def test_host_assembly_warns_once_for_a_failed_fold(monkeypatch):
    gp, model, posts, X, y, hyp = _host_gp(monkeypatch, bad=(1, 2))
    try:
        folds = scattered_folds(X.shape[0], [3, 5, 4])
        with warnings.catch_warnings(record=True) as wl:
            warnings.simplefilter("always")
            mu, s2, lpd, lpf = gp.cv_predict(folds, separate_samples=True, return_lpd=True)
        assert len(wl) == 1 and "fold 1" in str(wl[0].message) and "sample 2" in str(wl[0].message)
        assert np.all(np.isnan(mu[folds[1], 2])) and np.isnan(lpf[1, 2]) and not np.any(np.isnan(mu[folds[1], :2]))
        assert not np.any(np.isnan(mu[folds[0]])) and not np.any(np.isnan(lpf[[0, 2]]))
    finally:
        gp._post_handle = None


def test_refusals_before_device_work(monkeypatch):
    from gpyreg_amd import _lib

    monkeypatch.setattr(_lib, "context", lambda device=None: _NoDevice())
    gp = _se_gp()
    with pytest.raises(ValueError, match="no training data"):
        gp.cv_predict()
    rng = np.random.default_rng(0)
    gp.update(X_new=rng.uniform(-1, 1, (10, 2)), y_new=rng.uniform(-1, 1, (10, 1)), hyp=np.zeros((1, 5)), compute_posterior=False)
    with pytest.raises(ValueError, match="posteriors have been cleaned"):
        gp.cv_predict()
    with pytest.raises(ValueError, match="fold 0 has index 10 out of range"):
        gp.cv_predict([[10]])
