"""GP.quad_cov / GP.quad_mixture without a device: a NumPy restatement of the covariance between Gaussian-measure
integrals, of the mixture mean and variance and of every gradient, on the oracle's posteriors; checked against a
Gauss-Hermite double integral of the posterior covariance (D = 1), against the restatement of GP.quad, and against
5-point differences; the host assembly of GP.quad_mixture behind a stand-in for the device; the refusals that come before
any device work.  test_gpu_quad_mixture.py compares the device against the same restatement."""

import numpy as np
import pytest

from gp_stubs import _NoDevice, _se_gp
from test_quad_grad_cpu import (_counts, _kernel_scales, _mean_part, _problem, kernel_means, quad_numpy,
                                solve_posterior)


def gamma_matrix(mu, sigma, ell, sf2):
    """Gamma (M, M), the pair differences d (M, M, D) and t (M, M, D) = ell^2 + sigma_j^2 + sigma_k^2."""
    t = ell**2 + sigma[:, None, :] ** 2 + sigma[None, :, :] ** 2
    d = mu[:, None, :] - mu[None, :, :]
    return sf2 * np.prod(ell / np.sqrt(t), 2) * np.exp(-0.5 * np.sum(d**2 / t, 2)), d, t


def quad_cov_numpy(model, posts, X, mu, sigma):
    """GP.quad_cov restated, per sample: F (M, S) and C (M, M, S) = Gamma - Z^T (K + Sigma)^-1 Z, not clamped."""
    D = X.shape[1]
    cov_N, noise_N, mean_N = _counts(model, D)
    F, C = [], []
    for p in posts:
        h = p.hyp
        ell, sf2 = _kernel_scales(model, h[:cov_N], D)
        z, _, _ = kernel_means(X, mu, sigma, ell, sf2)
        nu, _, _ = _mean_part(model, h[cov_N + noise_N:cov_N + noise_N + mean_N], mu, sigma)
        F.append(z.T @ p.alpha[:, 0] + nu)
        c = gamma_matrix(mu, sigma, ell, sf2)[0] - z.T @ solve_posterior(p, z)
        C.append(0.5 * (c + c.T))
    return np.stack(F, 1), np.stack(C, 2)


def quad_mixture_numpy(model, posts, X, mu, sigma, w, terms=False):
    """GP.quad_mixture restated, per sample: a dict with E, V (S,), dE_dmu, dE_dsigma, dV_dmu, dV_dsigma (M, D, S) and
    dE_dw, dV_dw (M, S); V without the clamp in "V_raw".  With ``terms`` the dict also holds, for V and each of its
    gradients, the Gamma term and the solve term whose difference it is ("V|gamma", "V|solve", "dV_dmu|gamma", ...)."""
    M, D = mu.shape
    S = len(posts)
    cov_N, noise_N, mean_N = _counts(model, D)
    r = {k: np.zeros(S) for k in ("E", "V", "V_raw", "V|gamma", "V|solve")}
    for k in ("dE_dmu", "dE_dsigma", "dV_dmu", "dV_dsigma", "dV_dmu|gamma", "dV_dmu|solve", "dV_dsigma|gamma",
              "dV_dsigma|solve"):
        r[k] = np.zeros((M, D, S))
    for k in ("dE_dw", "dV_dw", "dV_dw|gamma", "dV_dw|solve"):
        r[k] = np.zeros((M, S))
    for s, p in enumerate(posts):
        h = p.hyp
        ell, sf2 = _kernel_scales(model, h[:cov_N], D)
        z, d, tau = kernel_means(X, mu, sigma, ell, sf2)
        dz_mu = -z[:, :, None] * d / tau**2
        dz_sg = z[:, :, None] * sigma * (d**2 / tau**2 - 1) / tau**2
        nu, nmu, nsg = _mean_part(model, h[cov_N + noise_N:cov_N + noise_N + mean_N], mu, sigma)
        a = p.alpha[:, 0]
        F = z.T @ a + nu
        r["E"][s] = w @ F
        r["dE_dw"][:, s] = F
        r["dE_dmu"][:, :, s] = w[:, None] * (np.einsum("i,ijl->jl", a, dz_mu) + nmu)
        r["dE_dsigma"][:, :, s] = w[:, None] * (np.einsum("i,ijl->jl", a, dz_sg) + nsg)
        G, dd, t = gamma_matrix(mu, sigma, ell, sf2)
        zbar = z @ w
        q = solve_posterior(p, zbar[:, None])[:, 0]
        r["V|gamma"][s], r["V|solve"][s] = w @ G @ w, zbar @ q
        r["dV_dw|gamma"][:, s], r["dV_dw|solve"][:, s] = 2 * G @ w, 2 * z.T @ q
        d1_mu = -G[:, :, None] * dd / t
        d1_sg = G[:, :, None] * sigma[:, None, :] * (dd**2 / t - 1) / t
        r["dV_dmu|gamma"][:, :, s] = 2 * w[:, None] * np.einsum("k,jkl->jl", w, d1_mu)
        r["dV_dsigma|gamma"][:, :, s] = 2 * w[:, None] * np.einsum("k,jkl->jl", w, d1_sg)
        r["dV_dmu|solve"][:, :, s] = 2 * w[:, None] * np.einsum("i,ijl->jl", q, dz_mu)
        r["dV_dsigma|solve"][:, :, s] = 2 * w[:, None] * np.einsum("i,ijl->jl", q, dz_sg)
    for k in ("V", "dV_dw", "dV_dmu", "dV_dsigma"):
        r[k] = r[k + "|gamma"] - r[k + "|solve"]
    r["V_raw"] = r["V"].copy()
    held = r["V_raw"] <= np.spacing(1)
    r["V"] = np.maximum(np.spacing(1), r["V_raw"])
    for k in ("dV_dw", "dV_dmu", "dV_dsigma"):
        r[k][..., held] = 0
    return r if terms else {k: v for k, v in r.items() if "|" not in k}


def device_share_numpy(model, posts, X, mu, sigma, w):
    """What gpc_quad_mix returns (both flags), from the restatement: the dict of GaussianProcess' handle.quad_mix."""
    M, D = mu.shape
    S = len(posts)
    cov_N = _counts(model, D)[0]
    out = {k: np.zeros((M, S)) for k in ("za", "gw", "zq")}
    out["zbkzb"] = np.zeros(S)
    for k in ("dza_dmu", "dza_dsigma", "dzq_dmu", "dzq_dsigma", "dgw_dmu", "dgw_dsigma"):
        out[k] = np.zeros((M, D, S))
    for s, p in enumerate(posts):
        ell, sf2 = _kernel_scales(model, p.hyp[:cov_N], D)
        z, d, tau = kernel_means(X, mu, sigma, ell, sf2)
        dz_mu = -z[:, :, None] * d / tau**2
        dz_sg = z[:, :, None] * sigma * (d**2 / tau**2 - 1) / tau**2
        G, dd, t = gamma_matrix(mu, sigma, ell, sf2)
        zbar = z @ w
        q = solve_posterior(p, zbar[:, None])[:, 0]
        a = p.alpha[:, 0]
        out["za"][:, s], out["gw"][:, s], out["zq"][:, s], out["zbkzb"][s] = z.T @ a, G @ w, z.T @ q, zbar @ q
        out["dza_dmu"][:, :, s] = np.einsum("i,ijl->jl", a, dz_mu)
        out["dza_dsigma"][:, :, s] = np.einsum("i,ijl->jl", a, dz_sg)
        out["dzq_dmu"][:, :, s] = np.einsum("i,ijl->jl", q, dz_mu)
        out["dzq_dsigma"][:, :, s] = np.einsum("i,ijl->jl", q, dz_sg)
        out["dgw_dmu"][:, :, s] = np.einsum("k,jkl->jl", w, -G[:, :, None] * dd / t)
        out["dgw_dsigma"][:, :, s] = np.einsum("k,jkl->jl", w, G[:, :, None] * sigma[:, None, :] * (dd**2 / t - 1) / t)
    return out


def _weights(M, seed=7):
    w = np.random.default_rng(seed).uniform(0.2, 1.0, M)
    w[1] = -0.4  # any finite reals: a negative weight
    return w


def test_covariance_is_the_double_integral_of_the_posterior_covariance():
    """D = 1: C_jk = E_{x ~ N_j} E_{x' ~ N_k} cov(f(x), f(x')) with cov the posterior covariance predict_full returns,
    k(x, x') - k(x, X) (K + Sigma)^-1 k(X, x'), formed from the oracle's kernel and posterior record at the nodes of an
    80-node Gauss-Hermite rule per measure.  The integrand is a sum of Gaussians of width >= ell ~ 0.8 against measures
    of width <= 0.8: the rule converges far below the bound, 1e-10 of max |C| (the formula itself reaches ~1e-13).
    L_chol posteriors only: with the low-noise parametrisation of _problem (sn2 = 1e-7, cond(K + Sigma) ~1e7 at D = 1)
    BOTH sides carry a solve error of ~1e-9 of Gamma, above the bound; that branch of the restatement is checked
    against quad's below."""
    from oracle import gp_oracle as orc

    model, posts, X, mu, sigma = _problem("se", "const", True, N=20, D=1)
    sigma = np.minimum(sigma, 0.8)
    _, C = quad_cov_numpy(model, posts, X, mu, sigma)
    t, wt = np.polynomial.hermite_e.hermegauss(80)
    wt = wt / wt.sum()
    M = mu.shape[0]
    nodes = (mu + sigma * t[None, :]).reshape(-1, 1)  # (M * 80, 1): measure-major
    for s, p in enumerate(posts):
        Kss = orc.covariance("se", p.hyp[:2], nodes)
        Ks = orc.covariance("se", p.hyp[:2], X, nodes)
        cov = Kss - Ks.T @ solve_posterior(p, Ks)
        ref = np.einsum("a,jakb,b->jk", wt, cov.reshape(M, 80, M, 80), wt)
        assert np.abs(C[:, :, s] - ref).max() <= 1e-10 * np.abs(ref).max()


@pytest.mark.parametrize("kernel,mean,lchol", [("se", "negquad", True), ("se_iso", "const", False), ("se", "zero", True)])
def test_diagonal_and_unit_weights_reproduce_quad(kernel, mean, lchol):
    model, posts, X, mu, sigma = _problem(kernel, mean, lchol)
    F0, V0 = quad_numpy(model, posts, X, mu, sigma)
    F, C = quad_cov_numpy(model, posts, X, mu, sigma)
    assert np.abs(F - F0).max() <= 1e-14 * np.abs(F0).max()
    diag = np.einsum("jjs->js", C)
    assert np.abs(diag - V0).max() <= 1e-13 * np.abs(V0).max()
    for j in range(mu.shape[0]):
        r = quad_mixture_numpy(model, posts, X, mu, sigma, np.eye(mu.shape[0])[j])
        assert np.abs(r["E"] - F0[j]).max() <= 1e-14 * np.abs(F0).max()
        assert np.abs(r["V"] - V0[j]).max() <= 1e-12 * np.abs(V0).max()


def test_mixture_variance_is_the_quadratic_form_of_the_covariance():
    for lchol in (True, False):
        model, posts, X, mu, sigma = _problem("se", "negquad", lchol)
        w = _weights(mu.shape[0])
        F, C = quad_cov_numpy(model, posts, X, mu, sigma)
        r = quad_mixture_numpy(model, posts, X, mu, sigma, w, terms=True)
        assert np.abs(r["E"] - w @ F).max() <= 1e-14 * np.abs(F).max()
        # V is the difference of two terms that nearly cancel: the bound is relative to the larger, w^T Gamma w
        assert np.abs(r["V_raw"] - np.einsum("j,jks,k->s", w, C, w)).max() <= 1e-13 * r["V|gamma"].max()


def _fd(f, x, h):
    """5-point d f / d x[j, l] of a function of the whole array x (M, D) -> (S,): (M, D, S)."""
    out = np.zeros(x.shape + f(x).shape)
    for idx in np.ndindex(*x.shape):
        e = np.zeros_like(x)
        e[idx] = h
        out[idx] = (-f(x + 2 * e) + 8 * f(x + e) - 8 * f(x - e) + f(x - 2 * e)) / (12 * h)
    return out


@pytest.mark.parametrize("kernel,mean,lchol", [("se", "negquad", True), ("se_iso", "const", True), ("se", "zero", False),
                                               ("se_iso", "negquad", False)])
def test_gradients_match_five_point_differences(kernel, mean, lchol):
    """Every gradient plane against 5-point differences of the restatement, step h = 1e-5 and bound 1e-6 of the plane's
    largest entry as reasoned in test_gpu_quad_grad.py (truncation h^4 f^(5) / 30 is negligible, rounding ~eps |f| / h
    ~1e-11 of the scale)."""
    model, posts, X, mu, sigma = _problem(kernel, mean, lchol, N=20)
    mu, sigma = mu[:4], sigma[:4]
    w = _weights(4)
    r = quad_mixture_numpy(model, posts, X, mu, sigma, w)
    assert np.all(r["V_raw"] > np.spacing(1))
    h = 1e-5
    for q in ("E", "V"):
        fd_mu = _fd(lambda m: quad_mixture_numpy(model, posts, X, m, sigma, w)[q], mu, h)
        fd_sg = _fd(lambda g: quad_mixture_numpy(model, posts, X, mu, g, w)[q], sigma, h)
        fd_w = _fd(lambda v: quad_mixture_numpy(model, posts, X, mu, sigma, v[:, 0])[q], w[:, None], h)[:, 0]
        for got, fd in ((r[f"d{q}_dmu"], fd_mu), (r[f"d{q}_dsigma"], fd_sg), (r[f"d{q}_dw"], fd_w)):
            assert np.abs(got - fd).max() <= 1e-6 * np.abs(fd).max(), q
    assert np.all(r["dE_dsigma"][0] == 0) and np.all(r["dV_dsigma"][0] == 0)  # a point measure (sigma = 0)


# ---- the host assembly of GP.quad_mixture / GP.quad_cov behind a stand-in for the device


class _Handle:
    """Stands in for the device posteriors: returns the device's share from the restatement."""

    def __init__(self, model, posts, X, shift=None):
        self.model, self.posts, self.X, self.shift = model, posts, X, shift

    def quad_mix(self, mu, sigma, w, compute_var, compute_grad):
        r = device_share_numpy(self.model, self.posts, self.X, mu, sigma, w)
        if self.shift is not None:
            r["zbkzb"] = r["zbkzb"] + self.shift
        for k in r:
            on = (k == "za" or (compute_var and k in ("gw", "zq", "zbkzb")) or (compute_grad and k.startswith("dza")) or
                  (compute_var and compute_grad and k[:3] in ("dzq", "dgw")))
            r[k] = r[k] if on else None
        return r

    def quad_cov(self, mu, sigma):
        cov_N = _counts(self.model, mu.shape[1])[0]
        za, C = [], []
        for p in self.posts:
            ell, sf2 = _kernel_scales(self.model, p.hyp[:cov_N], mu.shape[1])
            z, _, _ = kernel_means(self.X, mu, sigma, ell, sf2)
            za.append(z.T @ p.alpha[:, 0])
            C.append(gamma_matrix(mu, sigma, ell, sf2)[0] - z.T @ solve_posterior(p, z))
        return np.stack(za, 1), np.stack(C, 0)

    def free(self):
        pass


def _host_gp(monkeypatch, kernel, mean, S=3, shift=None):
    import gpyreg_amd as gpr
    from gpyreg_amd import _lib

    monkeypatch.setattr(_lib, "context", lambda device=None: _NoDevice())
    model, posts, X, mu, sigma = _problem(kernel, mean, True, S=S)
    means = {"zero": gpr.mean_functions.ZeroMean, "const": gpr.mean_functions.ConstantMean,
             "negquad": gpr.mean_functions.NegativeQuadratic}
    gp = _se_gp(D=X.shape[1], iso=kernel == "se_iso", mean=means[mean]())
    gp.update(X_new=X, y_new=np.zeros((X.shape[0], 1)), hyp=np.stack([p.hyp for p in posts]), compute_posterior=False)
    monkeypatch.setattr(gp, "_ctx", lambda: None)
    gp._post_handle = _Handle(model, posts, X, shift)
    return gp, model, posts, X, mu, sigma


@pytest.mark.parametrize("kernel,mean", [("se", "zero"), ("se_iso", "const"), ("se", "negquad")])
def test_host_assembly_mean_terms_and_shapes(monkeypatch, kernel, mean):
    from gpyreg_amd.gaussian_process import _mix_sample_grads, _mix_samples

    gp, model, posts, X, mu, sigma = _host_gp(monkeypatch, kernel, mean)
    try:
        M, D = mu.shape
        S = len(posts)
        w = _weights(M)
        ref = quad_mixture_numpy(model, posts, X, mu, sigma, w)
        keys = ("E", "V", "dE_dmu", "dE_dsigma", "dE_dw", "dV_dmu", "dV_dsigma", "dV_dw")
        got = gp.quad_mixture(mu, sigma, w, compute_var=True, compute_grad=True, separate_samples=True)
        assert len(got) == 8
        for k, g in zip(keys, got):
            assert g.shape == ref[k].shape
            assert np.abs(g - ref[k]).max() <= 1e-12 * max(np.abs(ref[k]).max(), 1e-300), k
        assert got[0].shape == (S,) and got[2].shape == (M, D, S) and got[4].shape == (M, S)
        # fewer outputs: the same numbers
        E = gp.quad_mixture(mu, sigma, w, separate_samples=True)
        assert np.array_equal(E, got[0])
        E, V = gp.quad_mixture(mu, sigma, w, compute_var=True, separate_samples=True)
        assert np.array_equal(E, got[0]) and np.array_equal(V, got[1])
        E, g_mu, g_sg, g_w = gp.quad_mixture(mu, sigma, w, compute_grad=True, separate_samples=True)
        assert np.array_equal(g_mu, got[2]) and np.array_equal(g_sg, got[3]) and np.array_equal(g_w, got[4])
        # the mixture over samples: _mix_samples and _mix_sample_grads of the per-sample values
        mixed = gp.quad_mixture(mu, sigma, w, compute_var=True, compute_grad=True)
        Em, Vm, _ = _mix_samples(got[0][None, :], got[1][None, :])
        assert isinstance(mixed[0], float) and isinstance(mixed[1], float)
        assert mixed[0] == Em[0, 0] and mixed[1] == Vm[0, 0]
        for i, shape in ((2, (M, D)), (3, (M, D)), (4, (M,))):
            de, dv = _mix_sample_grads(got[0][None, :], got[i].reshape(1, -1, S), got[i + 3].reshape(1, -1, S))
            assert mixed[i].shape == shape and mixed[i + 3].shape == shape
            assert np.array_equal(mixed[i], de.reshape(shape)) and np.array_equal(mixed[i + 3], dv.reshape(shape))
        # quad_cov: per sample, and the law of total covariance
        F0, C0 = quad_cov_numpy(model, posts, X, mu, sigma)
        F, C = gp.quad_cov(mu, sigma, separate_samples=True)
        assert F.shape == (M, S) and C.shape == (M, M, S)
        assert np.abs(F - F0).max() <= 1e-13 * np.abs(F0).max() and np.abs(C - C0).max() <= 1e-13 * np.abs(C0).max()
        assert np.array_equal(C, C.transpose(1, 0, 2))
        Fm, Cm = gp.quad_cov(mu, sigma)
        assert Fm.shape == (M, 1) and Cm.shape == (M, M)
        total = C0.mean(2) + np.cov(F0, ddof=1)
        assert np.abs(Cm - total).max() <= 1e-12 * np.abs(total).max()
        assert np.abs(Fm[:, 0] - F0.mean(1)).max() <= 1e-14 * np.abs(F0).max()
    finally:
        gp._post_handle = None


def test_host_assembly_clamp(monkeypatch):
    """Where V = max(eps, .) holds the variance its gradients are 0, per sample and in the mixture; the mean's are not."""
    shift = np.array([0.0, 1e3, 0.0])  # the solve term of sample 1 raised far above w^T Gamma w
    gp, model, posts, X, mu, sigma = _host_gp(monkeypatch, "se", "const", shift=shift)
    try:
        w = _weights(mu.shape[0])
        ref = quad_mixture_numpy(model, posts, X, mu, sigma, w)
        E, V, dE_mu, dE_sg, dE_w, dV_mu, dV_sg, dV_w = gp.quad_mixture(mu, sigma, w, True, True, separate_samples=True)
        assert V[1] == np.spacing(1) and V[0] > np.spacing(1) and V[2] > np.spacing(1)
        for g, k in ((dV_mu, "dV_dmu"), (dV_sg, "dV_dsigma"), (dV_w, "dV_dw")):
            assert np.all(g[..., 1] == 0)
            assert np.abs(g[..., [0, 2]] - ref[k][..., [0, 2]]).max() <= 1e-12 * np.abs(ref[k]).max()
        assert np.any(dE_mu[..., 1] != 0) and np.any(dE_w[..., 1] != 0)
    finally:
        gp._post_handle = None


def test_refusals_before_device_work(monkeypatch):
    import gpyreg_amd as gpr
    from gpyreg_amd import _lib

    monkeypatch.setattr(_lib, "context", lambda device=None: _NoDevice())
    rng = np.random.default_rng(0)
    X = rng.uniform(-1, 1, (10, 2))
    y = X[:, :1]
    calls = (lambda g, m, s: g.quad_mixture(m, s, np.ones(np.atleast_2d(m).shape[0]), compute_var=True),
             lambda g, m, s: g.quad_cov(m, s))
    for call in calls:
        for cov in (gpr.covariance_functions.Matern(5), gpr.covariance_functions.RationalQuadraticARD()):
            gp = gpr.GP(2, cov, gpr.mean_functions.ConstantMean(), gpr.noise_functions.GaussianNoise(constant_add=True))
            with pytest.raises(ValueError, match="only supports the squared exponential kernel"):
                call(gp, np.zeros((3, 2)), 1.0)
        gp = _se_gp()
        gp.update(X_new=X, y_new=y, hyp=np.zeros((1, 5)), compute_posterior=False)
        with pytest.raises(ValueError, match="posteriors have been cleaned"):
            call(gp, np.zeros((3, 2)), 1.0)
        with pytest.raises(ValueError):  # quad's broadcast of sigma to mu's shape
            call(gp, np.zeros((3, 2)), np.ones((2, 2)))
        with pytest.raises(ValueError, match="dimensions"):
            call(gp, np.zeros((3, 3)), np.ones((3, 3)))
        gp = _se_gp(iso=True, quirks=True)
        gp.update(X_new=X, y_new=y, hyp=np.zeros((1, 4)), compute_posterior=False)
        gp._post_handle = object()  # (posteriors present; the refusal must come before they are touched)
        try:
            with pytest.raises(NotImplementedError, match="reference_quirks"):
                call(gp, np.zeros((3, 2)), 1.0)
        finally:
            gp._post_handle = None
    gp = _se_gp()
    gp.update(X_new=X, y_new=y, hyp=np.zeros((1, 5)), compute_posterior=False)
    gp._post_handle = object()
    try:
        with pytest.raises(ValueError, match="3 measures but 2 weights"):
            gp.quad_mixture(np.zeros((3, 2)), 1.0, np.ones(2))
        with pytest.raises(ValueError, match="finite"):
            gp.quad_mixture(np.zeros((3, 2)), 1.0, np.array([1.0, np.nan, 1.0]))
    finally:
        gp._post_handle = None
