"""GP.predict_cov / GP.lookahead_variance without a device: NumPy restatements of the cross covariance between two query
sets and of the look-ahead reduction (both L_chol forms written out) against the reference's own predict_full numbers
(tests/golden/full_cases.npz) and against the identity they stand for -- the variance at the reference points drops by
exactly the reduction when the candidate is appended to the data -- on the oracle's posteriors; the prior paths of a GP
without data; the refusals that come before any device work.  test_gpu_lookahead.py compares the device against the
same restatements."""

import os

import numpy as np
import pytest
from scipy.linalg import solve_triangular

from conftest import parse_core_name

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _counts(model, D):
    from oracle import gp_oracle as orc

    return orc.cov_count(model["kernel"], D), orc.noise_count(model["noise"]), orc.mean_count(model["mean"], D)


def predict_cov_numpy(model, posts, X, xa, xb):
    """(cov (Ma, Mb, S), fs2b (Mb, S)): the posterior covariance between the rows of xa and of xb and predict's
    unclamped variance of xb, per posterior record (hyp, sW, L, L_chol):
      L_chol     (L upper, L^T L = I + sW K sW):  V = L^-T (sW o K*),  C = K_ab - V_a^T V_b,  fs2 = kss - sum V_b o V_b
      otherwise  (L = -(K + Sigma)^-1):           C = K_ab + K_a^T (L K_b),                  fs2 = kss + sum K_b o (L K_b)"""
    from oracle import gp_oracle as orc

    k, d = model["kernel"], model.get("degree", 0)
    cov_N = orc.cov_count(k, X.shape[1])
    cov = np.zeros((xa.shape[0], xb.shape[0], len(posts)))
    fs2b = np.zeros((xb.shape[0], len(posts)))
    for s, p in enumerate(posts):
        h = p.hyp[:cov_N]
        Kab = orc.covariance(k, h, xa, xb, degree=d)
        Ka = orc.covariance(k, h, X, xa, degree=d)
        Kb = orc.covariance(k, h, X, xb, degree=d)
        kss = orc.covariance(k, h, xb, compute_diag=True, degree=d)[:, 0]
        if p.L_chol:
            sW = np.reshape(p.sW, (-1, 1))
            Va = solve_triangular(p.L, sW * Ka, trans=1)
            Vb = solve_triangular(p.L, sW * Kb, trans=1)
            cov[:, :, s] = Kab - Va.T @ Vb
            fs2b[:, s] = kss - np.sum(Vb * Vb, 0)
        else:
            G = p.L @ Kb
            cov[:, :, s] = Kab + Ka.T @ G
            fs2b[:, s] = kss + np.sum(Kb * G, 0)
    return cov, fs2b


def reduce_numpy(cov, weights, den):
    """sum_r w_rs cov[r, c, s]^2 / den[c, s], 0 where den <= 0: (Mc, S).  weights None, (Mr,) or (Mr, S)."""
    Mr, Mc, S = cov.shape
    w = np.full(Mr, 1.0 / Mr) if weights is None else np.asarray(weights, float)
    w = w if w.ndim == 2 else np.repeat(w[:, None], S, axis=1)
    wsq = np.einsum("rs,rcs->cs", w, cov * cov)
    return np.where(den > 0, wsq / np.where(den > 0, den, 1.0), 0.0)


def lookahead_numpy(model, posts, X, x_cand, x_ref, weights=None, y_cand=None, s2_cand=None):
    """GP.lookahead_variance(separate_samples=True) restated: (Mc, S)."""
    from oracle import gp_oracle as orc

    cov_N, noise_N, _ = _counts(model, X.shape[1])
    cov, fs2 = predict_cov_numpy(model, posts, X, x_ref, x_cand)
    den = np.empty_like(fs2)
    for s, p in enumerate(posts):
        sn2 = orc.noise(model["noise"], p.hyp[cov_N:cov_N + noise_N], x_cand, y_cand, s2_cand)
        den[:, s:s + 1] = np.maximum(fs2[:, s:s + 1], 0) + sn2 * (1 if p.sn2_mult is None else p.sn2_mult)
    return reduce_numpy(cov, weights, den)


def test_restatement_equals_the_reference_block():
    """The five models of full_cases.npz, the 9 query points split 4 / 5 (and 5 / 4): the restated block equals the
    reference's predict_full block within 1e-7 of its largest entry, the bound of test_gpu_full.py.  (Measured: 1.1e-10
    of that scale for the low-noise model u002, 3e-12 for u004, below 5e-15 for the others.)"""
    from oracle import gp_oracle as orc

    g = np.load(os.path.join(ROOT, "tests", "golden", "full_cases.npz"), allow_pickle=False)
    assert len(g["names"]) == 5
    for name in g["names"]:
        tag, model, N, D, _ = parse_core_name(str(name) + "|plain")
        X, y, hyp, xs = g[tag + "_X"], g[tag + "_y"], g[tag + "_hyp"], g[tag + "_xs"]
        s2 = g[tag + "_s2"] if tag + "_s2" in g.files else None
        ref = g[tag + "_pf_cov"]
        assert xs.shape[0] == 9
        posts = orc.posteriors(model, hyp, X, y, s2)
        scale = np.abs(ref).max()
        for k in (4, 5):
            C, fs2b = predict_cov_numpy(model, posts, X, xs[:k], xs[k:])
            err = np.abs(C - ref[:k, k:, :]).max()
            print(tag, k, "block error / scale", err / scale)
            assert err <= 1e-7 * scale, (name, k)
            assert np.abs(fs2b - np.einsum("iis->is", ref)[k:]).max() <= 1e-7 * scale, (name, k)


def _problem(kernel, N=200, D=3, S=3, seed=1):
    """Laid out like the _problem of test_gpu_quad_grad.py, with a constant mean and scalar noise."""
    from oracle import gp_oracle as orc

    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (N, D))
    y = np.sin(X.sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1))
    model = dict(kernel=kernel, degree=5 if kernel.startswith("matern") else 0, mean="const", noise=(1, 0, 0))
    cov_N = orc.cov_count(kernel, D)
    hyp = np.zeros((S, cov_N + 2))
    hyp[:, :cov_N - 1] = np.log(1.2)
    hyp[:, cov_N] = np.log(0.1)
    hyp[:, cov_N + 1] = 0.3
    if kernel == "rq":
        hyp[:, cov_N - 1] = 0.5
        hyp[:, cov_N - 2] = 0.0
    hyp += 0.05 * rng.standard_normal(hyp.shape)
    return model, X, y, hyp


@pytest.mark.parametrize("kernel", ["se", "matern", "rq", "se_iso"])
def test_lookahead_identity_on_the_oracle(kernel):
    """Append candidate c to the data (any y: the variance does not depend on it), recompute the oracle's posteriors:
    the mean drop of the predictive variance over the reference points is the restated reduction.  L_chol samples only
    (a low-noise refactorization is conditioned too badly to show the identity: 1e-7).  Measured 3e-15 .. 1e-14 of the
    largest reduction; bound 1e-10."""
    from oracle import gp_oracle as orc

    model, X, y, hyp = _problem(kernel)
    rng = np.random.default_rng(5)
    xr, xc = rng.uniform(-2.5, 2.5, (40, 3)), rng.uniform(-2.5, 2.5, (6, 3))
    posts = orc.posteriors(model, hyp, X, y, None)
    assert all(p.L_chol for p in posts)
    rho = lookahead_numpy(model, posts, X, xc, xr)
    assert rho.shape == (6, 3) and rho.min() > 0
    _, v0 = orc.predict(model, posts, X, y, xr, separate_samples=True)
    worst = 0.0
    for c in range(xc.shape[0]):
        X1, y1 = np.vstack([X, xc[c:c + 1]]), np.vstack([y, [[0.7]]])
        p1 = orc.posteriors(model, hyp, X1, y1, None)
        assert [p.sn2_mult for p in p1] == [p.sn2_mult for p in posts]
        _, v1 = orc.predict(model, p1, X1, y1, xr, separate_samples=True)
        worst = max(worst, np.abs((v0 - v1).mean(0) - rho[c]).max() / np.abs(rho).max())
    print(kernel, "identity error / largest reduction", worst)
    assert worst <= 1e-10


def _prior_gp(D=2, S=3):
    import gpyreg_amd as gpr

    gp = gpr.GP(D, gpr.covariance_functions.Matern(5), gpr.mean_functions.NegativeQuadratic(),
                gpr.noise_functions.GaussianNoise(constant_add=True))
    rng = np.random.default_rng(0)
    hyp = np.concatenate([0.2 * rng.standard_normal((S, D)), np.zeros((S, 1)), np.full((S, 1), np.log(0.1)),
                          0.3 * rng.standard_normal((S, 1 + 2 * D))], axis=1)
    hyp[:, D + 1] += 0.1 * np.arange(S)
    gp.update(hyp=hyp)

    def host_compute(h, X, X_star=None, compute_diag=False, compute_grad=False):
        from oracle import gp_oracle as orc

        return orc.covariance("matern", h, X, X_star, compute_diag, degree=5)

    gp.covariance.compute = host_compute  # (the built-in compute is a device kernel)
    return gp, hyp


def test_gp_without_data_returns_the_prior():
    gp, hyp = _prior_gp()
    D, S = 2, 3
    rng = np.random.default_rng(1)
    xa, xb = rng.uniform(-2, 2, (7, D)), rng.uniform(-2, 2, (4, D))
    C = gp.predict_cov(xa, xb)
    assert C.shape == (7, 4, S)
    for s in range(S):
        assert np.array_equal(C[:, :, s], gp.covariance.compute(hyp[s, :D + 1], xa, xb))
    assert np.array_equal(gp.predict_cov(xa[0], xb)[:, :, 0], C[:1, :, 0])  # one point as a flat vector
    sn2 = np.exp(2 * hyp[:, D + 1])
    kss = np.stack([gp.covariance.compute(hyp[s, :D + 1], xb, compute_diag=True)[:, 0] for s in range(S)], 1)
    den = kss + sn2[None, :]
    w1, w2 = rng.uniform(0, 1, 7), rng.uniform(0, 1, (7, S))
    for w in (None, w1, w2):
        r = gp.lookahead_variance(xb, xa, weights=w, separate_samples=True)
        assert r.shape == (4, S)
        assert np.allclose(r, reduce_numpy(C, w, den), rtol=1e-13, atol=0)
        m = gp.lookahead_variance(xb, xa, weights=w)
        assert m.shape == (4, 1) and np.allclose(m[:, 0], r.mean(1), rtol=1e-14, atol=0)
    # per-point noise at the candidates enters the denominator
    gp2 = _prior_gp()[0]
    import gpyreg_amd as gpr

    gp2.noise = gpr.noise_functions.GaussianNoise(constant_add=True, user_provided_add=True)
    s2c = 0.3 * np.ones((4, 1))
    r = gp2.lookahead_variance(xb, xa, s2_cand=s2c, separate_samples=True)
    assert np.allclose(r, reduce_numpy(C, None, den + 0.3), rtol=1e-13, atol=0)


def test_refusals():
    import gpyreg_amd as gpr

    gp, hyp = _prior_gp()
    xa, xb = np.zeros((5, 2)), np.ones((3, 2))
    for bad in (np.ones(4), np.ones((5, 2)), np.ones((3,)), np.ones((5, 3, 1)), np.ones((3, 5))):
        with pytest.raises(ValueError, match="weights must be"):
            gp.lookahead_variance(xb, xa, weights=bad)
    for bad in (np.nan, np.inf, -np.inf):
        w = np.ones(5)
        w[2] = bad
        with pytest.raises(ValueError, match="finite"):
            gp.lookahead_variance(xb, xa, weights=w)
    with pytest.raises(AssertionError, match="input dimension"):
        gp.predict_cov(np.zeros((5, 3)), xb)
    with pytest.raises(AssertionError, match="input dimension"):
        gp.lookahead_variance(xb, np.zeros((5, 3)))

    class MyKernel(gpr.covariance_functions.SquaredExponential):
        _gpc_kernel_id = None  # a kernel of the caller's own: its compute is not a device kernel

    user = gpr.GP(2, MyKernel(), gpr.mean_functions.ZeroMean(), gpr.noise_functions.GaussianNoise(constant_add=True))
    user.update(hyp=np.zeros((1, 4)))
    with pytest.raises(NotImplementedError, match="MyKernel"):
        user.predict_cov(xa, xb)
    with pytest.raises(NotImplementedError, match="MyKernel"):
        user.lookahead_variance(xb, xa)


def test_the_symbol_is_bound():
    from gpyreg_amd import _lib

    assert "gpc_predict_cov" in _lib.SIGNATURES and hasattr(_lib.PostHandle, "predict_cov")
