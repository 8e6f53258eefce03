#!/usr/bin/env python3
"""Generate tests/golden/cv_cases.npz by running the REFERENCE itself (build container only; see make_golden.py):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg PYTHONPATH=<reference> python3 <repo>/tests/golden/make_cv_golden.py

Two small cases (N = 60, D = 2, S = 2, SE kernel, constant mean, constant noise): leave-one-out and four unequal,
scattered folds.  For every fold the reference's own ``update`` on the data without the fold and its ``predict`` /
``predict_full`` at the fold, with ``add_noise``; the joint log density of the fold is computed here from the mean and
covariance that ``predict_full`` returned.  The file holds inputs and recorded outputs only."""

import os

import numpy as np
import scipy.linalg as sla

import gpyreg as gpr  # the reference

HERE = os.path.dirname(os.path.abspath(__file__))


def make_gp(D):
    return gpr.GP(D=D, covariance=gpr.covariance_functions.SquaredExponential(), mean=gpr.mean_functions.ConstantMean(),
                  noise=gpr.noise_functions.GaussianNoise(constant_add=True))


def main():
    N, D, S = 60, 2, 2
    rng = np.random.default_rng(23000)
    X = rng.uniform(-2, 2, (N, D))
    y = np.sin(X.sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1))
    hyp = np.zeros((S, D + 3))
    hyp[:, :D + 1] = np.log(1.2)
    hyp[:, D + 1] = np.log(0.1)
    hyp[:, D + 2] = 0.3
    hyp += 0.05 * rng.standard_normal(hyp.shape)
    perm = rng.permutation(N)
    cases = {"loo": [np.array([i]) for i in range(N)],
             "folds4": [np.sort(perm[a:b]) for a, b in ((0, 1), (1, 8), (8, 25), (25, 60))]}
    out = dict(X=X, y=y, hyp=hyp, names=np.array(list(cases)))
    full = make_gp(D)
    full.update(X_new=X, y_new=y, hyp=hyp)
    assert all(p.sn2_mult == 1 and p.L_chol for p in full.posteriors)
    for name, folds in cases.items():
        mu, s2 = np.full((N, S), np.nan), np.full((N, S), np.nan)
        lpd = np.zeros((len(folds), S))
        for f, I in enumerate(folds):
            keep = np.setdiff1d(np.arange(N), I)
            gp = make_gp(D)
            gp.update(X_new=X[keep], y_new=y[keep], hyp=hyp)
            assert all(p.sn2_mult == 1 for p in gp.posteriors)
            m1, v1 = gp.predict(X[I], add_noise=True, separate_samples=True)
            mf, cf = gp.predict_full(X[I], add_noise=True)
            assert np.allclose(m1, mf, rtol=1e-12, atol=1e-14)
            mu[I], s2[I] = m1, v1
            for s in range(S):
                R = sla.cholesky(cf[:, :, s], lower=True)
                u = sla.solve_triangular(R, y[I, 0] - mf[:, s], lower=True)
                lpd[f, s] = -0.5 * u @ u - np.sum(np.log(np.diag(R))) - 0.5 * I.size * np.log(2 * np.pi)
        out[name + "_ptr"] = np.concatenate([[0], np.cumsum([I.size for I in folds])]).astype(np.int64)
        out[name + "_idx"] = np.concatenate(folds).astype(np.int64)
        out[name + "_mu"], out[name + "_s2"], out[name + "_lpd_fold"] = mu, s2, lpd
        print(name, "folds", len(folds), "lpd_fold sum", lpd.sum(0))
    np.savez_compressed(os.path.join(HERE, "cv_cases.npz"), **out)


if __name__ == "__main__":
    main()
