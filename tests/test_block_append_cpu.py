"""CPU-side checks of the block append (GP.update(block_append=True), gpc_post_append_block): a NumPy restatement of
its algebra (include/gpcore.h, both parametrisations) against the oracle's full recompute on the extended data, the
k = 1 case against the oracle's rank-one update, the declarations and bindings, and the parts of ``update`` that
need no device."""

import copy
import os
import re

import numpy as np
import pytest
import scipy.linalg as sla

from oracle import gp_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "rank1_cases.npz"), allow_pickle=False)


def parse(name):
    tag, kname, mname, npar, N, D, flav = str(name).split("|")
    degree, kernel = 0, kname
    if kname.startswith("matern"):
        kernel, degree = "matern", int(kname[6:])
    return tag, dict(kernel=kernel, degree=degree, mean=mname, noise=tuple(int(c) for c in npar)), int(N), int(D), flav


def seeded_rows(X, y, k, seed):
    """k new rows in the cloud of the training inputs (a training row plus a perturbation of half the per-column
    spread, so that no new point coincides with an old one) and observations with the spread of y."""
    rng = np.random.default_rng(seed)
    base = X[rng.integers(0, X.shape[0], k)]
    Xn = base + 0.5 * X.std(0, keepdims=True) * rng.standard_normal((k, X.shape[1]))
    yn = y.mean() + y.std() * rng.standard_normal((k, 1))
    return Xn, yn


def new_rows(g, tag, k):
    """The fixture's own three rows for k = 3, seeded rows otherwise."""
    if k == 3:
        return g[tag + "_Xn"], g[tag + "_yn"]
    return seeded_rows(g[tag + "_X"], g[tag + "_y"], k, 100 + k)


def block_append_numpy(model, posts, X, y, Xn, yn, schur_min_eig=None):
    """The block append of include/gpcore.h restated in NumPy on the oracle's posterior records (high noise:
    ``L`` is the UPPER factor U, U^T U = K / sl + I; low noise: ``L`` = -(K + Sigma)^-1).  Returns new records on
    the extended data; ``schur_min_eig`` (a list) receives the smallest eigenvalue of every sample's Schur block."""
    kernel, degree = model["kernel"], model.get("degree", 0)
    n, d = X.shape
    k = Xn.shape[0]
    cov_N, noise_N = orc.cov_count(kernel, d), orc.noise_count(model["noise"])
    out = []
    for p in posts:
        h = p.hyp
        sn2 = orc.noise(model["noise"], h[cov_N:cov_N + noise_N], Xn, yn, 0)
        assert np.isscalar(sn2) or np.ndim(sn2) == 0
        sn2_eff = float(sn2) * p.sn2_mult
        m_new = np.reshape(orc.mean(model["mean"], h[cov_N + noise_N:], Xn), (k, 1))
        B = orc.covariance(kernel, h[0:cov_N], X, Xn, degree=degree)
        Knn = orc.covariance(kernel, h[0:cov_N], Xn, degree=degree)
        e = (yn - m_new) - B.T @ p.alpha
        if p.L_chol:
            sl = sn2_eff
            Lo = p.L.T
            W = sla.solve_triangular(Lo, np.eye(n), lower=True, check_finite=False)
            V = W @ B
            L21 = V.T / sl
            S = Knn / sl + np.eye(k) - L21 @ L21.T
            if schur_min_eig is not None:
                schur_min_eig.append(np.linalg.eigvalsh(S).min())
            L22 = np.linalg.cholesky(S)
            W22 = sla.solve_triangular(L22, np.eye(k), lower=True, check_finite=False)
            W21 = -W22 @ (L21 @ W)
            u2 = W22 @ e
            alpha = np.concatenate([p.alpha + W21.T @ u2 / sl, W22.T @ u2 / sl])
            Lo_new = np.block([[Lo, np.zeros((n, k))], [L21, L22]])
            L_new = Lo_new.T
        else:
            Ainv = -p.L
            G = Ainv @ B
            S = Knn + sn2_eff * np.eye(k) - B.T @ G
            if schur_min_eig is not None:
                schur_min_eig.append(np.linalg.eigvalsh(S).min())
            L22 = np.linalg.cholesky(S)
            W22 = sla.solve_triangular(L22, np.eye(k), lower=True, check_finite=False)
            Si = W22.T @ W22
            GS = G @ Si
            a2 = Si @ e
            alpha = np.concatenate([p.alpha - G @ a2, a2])
            L_new = -np.block([[Ainv + GS @ G.T, -GS], [-GS.T, Si]])
        sW = np.concatenate([p.sW, np.full((k, 1), 1.0 / np.sqrt(sn2_eff))])
        out.append(orc.OraclePosterior(h, alpha, sW, L_new, p.sn2_mult, p.L_chol))
    return out


def rel(a, ref):
    return np.abs(np.asarray(a) - np.asarray(ref)).max() / max(np.abs(ref).max(), 1e-300)


@pytest.mark.parametrize("k", [3, 40, 200])
def test_restatement_equals_the_full_recompute(k):
    g = golden()
    for name in g["names"]:
        tag, model, N, D, flav = parse(name)
        X, y, hyp, xs = g[tag + "_X"], g[tag + "_y"], g[tag + "_hyp"], g[tag + "_xs"]
        Xn, yn = new_rows(g, tag, k)
        posts = orc.posteriors(model, hyp, X, y, None)
        eig = []
        app = block_append_numpy(model, posts, X, y, Xn, yn, eig)
        assert len(eig) == len(posts) and min(eig) > 0.0, (name, eig)  # every Schur block is positive definite
        X2, y2 = np.concatenate([X, Xn]), np.concatenate([y, yn])
        full = orc.posteriors(model, hyp, X2, y2, None)
        for s, (a, f) in enumerate(zip(app, full)):
            assert a.L_chol == f.L_chol == (flav == "high") and a.sn2_mult == f.sn2_mult, (name, s)
            assert a.alpha.shape == (N + k, 1) and a.L.shape == (N + k, N + k) and a.sW.shape == (N + k, 1)
            assert rel(a.alpha, f.alpha) <= 1e-8, (name, s, rel(a.alpha, f.alpha))
            assert rel(a.L, f.L) <= 1e-8, (name, s, rel(a.L, f.L))
            assert np.allclose(a.sW, f.sW, rtol=1e-12), (name, s)
        mu, s2 = orc.predict(model, app, X2, y2, xs, separate_samples=True)
        rm, rs = orc.predict(model, full, X2, y2, xs, separate_samples=True)
        assert np.abs(mu - rm).max() <= 1e-8 * max(1.0, np.abs(rm).max()), name
        assert np.abs(s2 - rs).max() <= 1e-8 * max(1.0, np.abs(rs).max()), name


def test_restatement_with_one_row_equals_the_rank_one_update():
    g = golden()
    for name in g["names"]:
        tag, model, N, D, flav = parse(name)
        X, y, hyp = g[tag + "_X"], g[tag + "_y"], g[tag + "_hyp"]
        Xn, yn = g[tag + "_Xn"][:1], g[tag + "_yn"][:1]
        posts = orc.posteriors(model, hyp, X, y, None)
        app = block_append_numpy(model, posts, X, y, Xn, yn)
        r1, _, _, redone = orc.rank_one_update(model, copy.deepcopy(posts), X, y, Xn, yn)
        assert redone == [], name
        for s, (a, f) in enumerate(zip(app, r1)):
            assert rel(a.alpha, f.alpha) <= 1e-8 and rel(a.L, f.L) <= 1e-8, (name, s)
            assert np.allclose(a.sW, f.sW, rtol=1e-12), (name, s)


def _params(text, fn):
    m = re.search(r"\b%s\s*\(([^)]*)\)" % fn, text)
    assert m, fn + " is not declared in include/gpcore.h"
    return [a for a in m.group(1).split(",") if a.strip()]


def test_block_append_entry_points_are_declared_and_bound():
    from gpyreg_amd import _lib

    header = open(os.path.join(ROOT, "include", "gpcore.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for fn, nargs in (("gpc_post_append_block", 6), ("gpc_post_append_block_K", 8)):
        assert len(_params(header, fn)) == nargs, fn
        assert fn in _lib.SIGNATURES and len(_lib.SIGNATURES[fn][1]) == nargs, fn
    assert callable(_lib.PostHandle.append_block) and callable(_lib.PostHandle.append_block_K)


def _small_gp():
    import gpyreg_amd as gpr

    return gpr.GP(2, gpr.covariance_functions.SquaredExponential(), gpr.mean_functions.ConstantMean(),
                  gpr.noise_functions.GaussianNoise(constant_add=True))


def test_update_without_posteriors_ignores_the_keyword():
    """No posterior is computed: X, y are stored and the records are empty, exactly as without the keyword."""
    rng = np.random.default_rng(0)
    X, y = rng.standard_normal((6, 2)), rng.standard_normal((6, 1))
    hyp = np.array([[0.1, -0.1, 0.05, np.log(0.2), 0.1], [0.3, 0.2, -0.1, np.log(0.1), -0.2]])
    gps = []
    for kw in ({}, {"block_append": True}):
        gp = _small_gp()
        gp.update(X_new=X[:4], y_new=y[:4], hyp=hyp, compute_posterior=False, **kw)  # a GP without data
        gp.update(X_new=X[4:], y_new=y[4:], compute_posterior=False, **kw)           # ... and one with
        gps.append(gp)
    a, b = gps
    assert np.array_equal(a.X, X) and np.array_equal(b.X, X) and np.array_equal(a.y, b.y)
    assert a.posteriors.shape == b.posteriors.shape == (2,)
    for p, q in zip(a.posteriors, b.posteriors):
        assert np.array_equal(p.hyp, q.hyp)
        assert p.alpha is None and q.alpha is None and p.L is None and q.L is None and p.sW is None and q.sW is None
    assert a._post_handle is None and b._post_handle is None


def test_update_refuses_bad_shapes_before_any_device_work():
    """The shape checks of ``update`` come before the dispatch: the same exception type and message with the keyword
    as without it, and nothing is stored."""
    rng = np.random.default_rng(1)
    # (D = 5 for a GP of D = 2: _convert_shapes' own assertion; 3 rows of X and 4 of y: its reshape)
    cases = [(AssertionError, dict(X_new=rng.standard_normal((3, 5)), y_new=rng.standard_normal((3, 1)))),
             (ValueError, dict(X_new=rng.standard_normal((3, 2)), y_new=rng.standard_normal((4, 1))))]
    for exc, args in cases:
        seen = []
        for kw in ({}, {"block_append": True}):
            gp = _small_gp()
            with pytest.raises(exc) as e:
                gp.update(compute_posterior=False, **args, **kw)
            assert gp.X is None and gp.y is None
            seen.append((type(e.value), str(e.value)))
        assert seen[0] == seen[1] and seen[0][1], seen
