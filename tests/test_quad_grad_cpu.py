"""GP.quad_grad without a device: a NumPy restatement of the gradient formulas (per-pair z, q = (K + Sigma)^-1 z and
the host terms) against 5-point differences of a NumPy restatement of GP.quad, on the oracle's posteriors; the mixture
gradients with quad's shapes; the refusals that come before any device work.  test_gpu_quad_grad.py compares the device
against the same restatement."""

import numpy as np
import pytest
from scipy.linalg import solve_triangular

from gp_stubs import _NoDevice, _se_gp


def _counts(model, D):
    from oracle import gp_oracle as orc

    return orc.cov_count(model["kernel"], D), orc.noise_count(model["noise"]), orc.mean_count(model["mean"], D)


def _kernel_scales(model, hyp, D):
    """(ell (D,), sf2) of an SE kernel's hyperparameters, ARD or isotropic."""
    iso = model["kernel"] == "se_iso"
    ell = np.exp(hyp[0]) * np.ones(D) if iso else np.exp(hyp[:D])
    return ell, np.exp(2 * hyp[1 if iso else D])


def kernel_means(X, mu, sigma, ell, sf2):
    """z (N, M) per pair as quad_z_kernel forms it, with d = mu - X (N, M, D) and tau (M, D)."""
    tau = np.sqrt(sigma**2 + ell**2)
    d = mu[None, :, :] - X[:, None, :]
    nf = sf2 * np.prod(ell / tau, 1)
    return nf[None, :] * np.exp(-0.5 * np.sum((d / tau[None]) ** 2, 2)), d, tau


def solve_posterior(p, z):
    """q = (K + Sigma)^-1 z through the posterior record: sW o L^-1 (L^-T (sW o z)) (L_chol; L upper, L^T L =
    I + sW K sW) as predict solves, or -(L z) (L = -(K + Sigma)^-1)."""
    if p.L_chol:
        sW = np.reshape(p.sW, (-1, 1))
        return sW * solve_triangular(p.L, solve_triangular(p.L, sW * z, trans="T"))
    return -(p.L @ z)


def _mean_part(model, hm, mu, sigma):
    """The mean function's part of F and its gradients: (nu (M,), dnu_dmu, dnu_dsigma (M, D))."""
    M, D = mu.shape
    zero = np.zeros((M, D))
    if model["mean"] == "zero":
        return np.zeros(M), zero, zero
    if model["mean"] == "const":
        return hm[0] * np.ones(M), zero, zero
    xm, om2 = hm[1:1 + D], np.exp(2 * hm[1 + D:1 + 2 * D])
    nu = hm[0] - 0.5 * np.sum((mu**2 + sigma**2 - 2 * mu * xm + xm**2) / om2, 1)
    return nu, -(mu - xm) / om2, -sigma / om2


def quad_numpy(model, posts, X, mu, sigma):
    """GP.quad restated, per sample: F, F_var (M, S)."""
    D = X.shape[1]
    cov_N, noise_N, mean_N = _counts(model, D)
    F, V = [], []
    for p in posts:
        h = p.hyp
        ell, sf2 = _kernel_scales(model, h[:cov_N], D)
        z, _, _ = kernel_means(X, mu, sigma, ell, sf2)
        nu, _, _ = _mean_part(model, h[cov_N + noise_N:cov_N + noise_N + mean_N], mu, sigma)
        F.append(z.T @ p.alpha[:, 0] + nu)
        nf_kk = sf2 * np.prod(ell / np.sqrt(2 * sigma**2 + ell**2), 1)
        V.append(np.maximum(np.spacing(1), nf_kk - np.sum(z * solve_posterior(p, z), 0)))
    return np.stack(F, 1), np.stack(V, 1)


def quad_grad_numpy(model, posts, X, mu, sigma, parts=False):
    """The formulas of GP.quad_grad, per sample: dF_dmu, dF_dsigma, dFvar_dmu, dFvar_dsigma (M, D, S).  With
    ``parts`` the device's share instead: dza_dmu, dza_dsigma, dzkz_dmu, dzkz_dsigma (gpc_quad_grad's convention)."""
    M, D = mu.shape
    cov_N, noise_N, mean_N = _counts(model, D)
    out = np.zeros((4, M, D, len(posts)))
    for s, p in enumerate(posts):
        h = p.hyp
        ell, sf2 = _kernel_scales(model, h[:cov_N], D)
        z, d, tau = kernel_means(X, mu, sigma, ell, sf2)
        dz_mu = -z[:, :, None] * d / tau**2
        dz_sg = z[:, :, None] * sigma * (d**2 / tau**2 - 1) / tau**2
        q = solve_posterior(p, z)
        g = [np.einsum("i,ijl->jl", p.alpha[:, 0], dz_mu), np.einsum("i,ijl->jl", p.alpha[:, 0], dz_sg),
             2 * np.einsum("ij,ijl->jl", q, dz_mu), 2 * np.einsum("ij,ijl->jl", q, dz_sg)]
        if not parts:
            _, nmu, nsg = _mean_part(model, h[cov_N + noise_N:cov_N + noise_N + mean_N], mu, sigma)
            nf_kk = sf2 * np.prod(ell / np.sqrt(2 * sigma**2 + ell**2), 1)
            held = nf_kk - np.sum(z * q, 0) <= np.spacing(1)
            g = [g[0] + nmu, g[1] + nsg, -g[2], -nf_kk[:, None] * 2 * sigma / (2 * sigma**2 + ell**2) - g[3]]
            g[2][held] = g[3][held] = 0
        for k in range(4):
            out[k, :, :, s] = g[k]
    return tuple(out)


def five_point(f, x, h):
    """d f / d x[j, l] for every (j, l) of a function of the rows of x (M, D) -> (M, S): (M, D, S).  Rows are
    independent, so one column l of the perturbation moves every row at once."""
    M, D = x.shape
    out = None
    for l in range(D):
        e = np.zeros_like(x)
        e[:, l] = h
        g = (-f(x + 2 * e) + 8 * f(x + e) - 8 * f(x - e) + f(x - 2 * e)) / (12 * h)
        out = np.zeros((M, D) + g.shape[1:]) if out is None else out
        out[:, l] = g
    return out


def _problem(kernel, mean, lchol=True, N=30, D=3, S=2, seed=0):
    from oracle import gp_oracle as orc

    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (N, D))
    y = np.sin(X.sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1))
    model = dict(kernel=kernel, degree=0, mean=mean, noise=(1, 0, 0))
    cov_N, noise_N, mean_N = _counts(model, D)
    hyp = np.zeros((S, cov_N + noise_N + mean_N))
    hyp[:, :cov_N - 1] = np.log(0.8)
    hyp[:, cov_N] = np.log(0.1) if lchol else 0.5 * np.log(1e-7)
    if mean != "zero":
        hyp[:, cov_N + noise_N] = 0.3
    if mean == "negquad":
        hyp[:, cov_N + noise_N + 1 + D:] = np.log(2.0)
    hyp += 0.05 * rng.standard_normal(hyp.shape)
    posts = orc.posteriors(model, hyp, X, y, None)
    assert all(bool(p.L_chol) == lchol for p in posts)
    mu = rng.uniform(-2.5, 2.5, (6, D))
    sigma = rng.uniform(0.2, 1.5, (6, D))
    sigma[0] = 0.0  # a point measure
    sigma[1, 0] = 0.0
    return model, posts, X, mu, sigma


@pytest.mark.parametrize("kernel", ["se", "se_iso"])
@pytest.mark.parametrize("mean", ["zero", "const", "negquad"])
@pytest.mark.parametrize("lchol", [True, False])
def test_formulas_match_five_point_differences_of_quad(kernel, mean, lchol):
    model, posts, X, mu, sigma = _problem(kernel, mean, lchol)
    F, V = quad_numpy(model, posts, X, mu, sigma)
    assert np.all(V > np.spacing(1))  # no clamp in these cases: the variance is smooth in mu and sigma
    dF_mu, dF_sg, dV_mu, dV_sg = quad_grad_numpy(model, posts, X, mu, sigma)
    h = 1e-3
    for got, f, x in ((dF_mu, lambda m: quad_numpy(model, posts, X, m, sigma)[0], mu),
                      (dF_sg, lambda g: quad_numpy(model, posts, X, mu, g)[0], sigma),
                      (dV_mu, lambda m: quad_numpy(model, posts, X, m, sigma)[1], mu),
                      (dV_sg, lambda g: quad_numpy(model, posts, X, mu, g)[1], sigma)):
        fd = five_point(f, x, h)
        # the stencil's error is h^4 f^(5) / 30 (~1e-13 here) plus ~eps |f| / h (~1e-13): 1e-8 of the largest entry
        # is far above both and far below any wrong term
        assert np.abs(got - fd).max() <= 1e-8 * np.abs(fd).max()
    assert np.all(dF_sg[0] == 0) and np.all(dV_sg[0] == 0) and np.all(dF_sg[1, 0] == 0) and np.all(dV_sg[1, 0] == 0)


def test_posterior_solve_is_the_direct_solve():
    from oracle import gp_oracle as orc

    for lchol in (True, False):
        model, posts, X, mu, sigma = _problem("se", "const", lchol)
        for p in posts:
            ell, sf2 = _kernel_scales(model, p.hyp, X.shape[1])
            z, _, _ = kernel_means(X, mu, sigma, ell, sf2)
            K = orc.covariance("se", p.hyp[:X.shape[1] + 1], X)
            sn2 = np.exp(2 * p.hyp[X.shape[1] + 1]) * p.sn2_mult
            q = np.linalg.solve(K + sn2 * np.eye(X.shape[0]), z)
            assert np.abs(solve_posterior(p, z) - q).max() <= 1e-6 * np.abs(q).max()


def test_kernel_means_are_the_gaussian_integrals():
    """z_ij = E_{x ~ N(mu_j, diag sigma_j^2)} k(x, X_i), checked by Gauss-Hermite quadrature in D = 2."""
    rng = np.random.default_rng(3)
    X = rng.uniform(-1, 1, (4, 2))
    mu, sigma = np.array([[0.3, -0.2]]), np.array([[0.5, 0.8]])
    ell, sf2 = np.array([0.7, 1.1]), 1.7
    z, _, _ = kernel_means(X, mu, sigma, ell, sf2)
    t, w = np.polynomial.hermite_e.hermegauss(40)
    w = w / w.sum()
    x0, x1 = mu[0, 0] + sigma[0, 0] * t[:, None], mu[0, 1] + sigma[0, 1] * t[None, :]
    for i in range(4):
        k = sf2 * np.exp(-0.5 * ((x0 - X[i, 0]) ** 2 / ell[0] ** 2 + (x1 - X[i, 1]) ** 2 / ell[1] ** 2))
        assert abs(w @ k @ w - z[i, 0]) <= 1e-13


def test_mixture_gradients_with_quad_shapes():
    """quad_grad mixes with _mix_sample_grads, once for mu and once for sigma: against 5-point differences of quad's own
    mixture (_mix_samples) of the restated per-sample values."""
    from gpyreg_amd.gaussian_process import _mix_sample_grads, _mix_samples

    model, posts, X, mu, sigma = _problem("se", "negquad", True, S=3)
    F, V = quad_numpy(model, posts, X, mu, sigma)
    dF_mu, dF_sg, dV_mu, dV_sg = quad_grad_numpy(model, posts, X, mu, sigma)
    gm = _mix_sample_grads(F, dF_mu, dV_mu)
    gs = _mix_sample_grads(F, dF_sg, dV_sg)
    assert gm[0].shape == gm[1].shape == mu.shape
    h = 1e-3
    for k in range(2):
        fm = five_point(lambda m: _mix_samples(*quad_numpy(model, posts, X, m, sigma))[k], mu, h)[:, :, 0]
        fs = five_point(lambda g: _mix_samples(*quad_numpy(model, posts, X, mu, g))[k], sigma, h)[:, :, 0]
        assert np.abs(gm[k] - fm).max() <= 1e-8 * np.abs(fm).max()
        assert np.abs(gs[k] - fs).max() <= 1e-8 * np.abs(fs).max()


def test_refusals_before_device_work(monkeypatch):
    import gpyreg_amd as gpr
    from gpyreg_amd import _lib

    monkeypatch.setattr(_lib, "context", lambda device=None: _NoDevice())
    rng = np.random.default_rng(0)
    X = rng.uniform(-1, 1, (10, 2))
    y = X[:, :1]
    for cov in (gpr.covariance_functions.Matern(5), gpr.covariance_functions.RationalQuadraticARD()):
        gp = gpr.GP(2, cov, gpr.mean_functions.ConstantMean(), gpr.noise_functions.GaussianNoise(constant_add=True))
        with pytest.raises(ValueError, match="only supports the squared exponential kernel"):
            gp.quad_grad(np.zeros((3, 2)), 1.0)
    gp = _se_gp()
    gp.update(X_new=X, y_new=y, hyp=np.zeros((1, 5)), compute_posterior=False)
    with pytest.raises(ValueError, match="posteriors have been cleaned"):
        gp.quad_grad(np.zeros((3, 2)), 1.0, compute_var=True)
    with pytest.raises(ValueError):  # quad's broadcast of sigma to mu's shape
        gp.quad_grad(np.zeros((3, 2)), np.ones((2, 2)))
    with pytest.raises(ValueError, match="dimensions"):
        gp.quad_grad(np.zeros((3, 3)), np.ones((3, 3)))
    # quirks with an isotropic kernel at D > 1: quad builds a misread z on the host; nothing on the device matches it
    gp = _se_gp(iso=True, quirks=True)
    gp.update(X_new=X, y_new=y, hyp=np.zeros((1, 4)), compute_posterior=False)
    gp._post_handle = object()  # (posteriors present; the refusal must come before they are touched)
    try:
        with pytest.raises(NotImplementedError, match="reference_quirks"):
            gp.quad_grad(np.zeros((3, 2)), 1.0)
    finally:
        gp._post_handle = None
