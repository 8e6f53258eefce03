"""gpyreg_amd._gradpost, the NumPy restatement of GP.gradient_posterior (the oracle of the GPU tests): the prior block H
and the derivative operand G against central differences of the oracle's covariance functions, the joint covariance
against the finite-difference transform of the oracle's full predictive covariance on a stencil, the identities with
predict and predict_grad, the mixture, and the host-side refusals.  No device: the covariance values come from
oracle.gp_oracle.covariance (the package's covariance classes evaluate on the device; tests/test_gpu_gradient_posterior.py
repeats the H check on them)."""

import numpy as np
import pytest
import scipy.linalg as sla

from gpyreg_amd import _gradpost as gpm
from oracle import gp_oracle as orc

KID = {"se": 0, "matern": 1, "rq": 2, "se_iso": 3, "matern_iso": 4}
FAMILIES = [("se", 0), ("matern", 3), ("matern", 5), ("rq", 0), ("se_iso", 0), ("matern_iso", 3), ("matern_iso", 5)]


def _hyp_cov(kernel, D, rng, ell=1.2):
    n = orc.cov_count(kernel, D)
    h = np.zeros(n)
    nl = 1 if kernel.endswith("_iso") else D
    h[:nl] = np.log(ell) + 0.1 * rng.standard_normal(nl)
    h[nl] = np.log(1.3)  # sf
    if kernel == "rq":
        h[nl + 1] = np.log(1.7)
    return h


def _ells(kernel, h, D):
    return np.exp(h[0]) * np.ones(D) if kernel.endswith("_iso") else np.exp(h[:D])


@pytest.mark.parametrize("kernel,degree", FAMILIES)
@pytest.mark.parametrize("D", [1, 3])
def test_prior_block_against_second_differences(kernel, degree, D):
    """H[1 + l, 1 + l] = d^2 k(x, x') / dx_l dx'_l at x = x' by the four-point central difference with h = 1e-4 ell:
    truncation O(h^2) for SE / Matern 5 / RQ (1e-5 of the value asserted), O(h) for Matern 3 (third-derivative kink at
    0: 4 h c / 3 = 2.3e-4 sqrt(3), 1e-3 asserted); rounding eps / (4 h^2) ~ 2e-9.  The off-diagonal second differences
    and the first differences (the value / derivative cross terms) vanish."""
    rng = np.random.default_rng(3)
    h_cov = _hyp_cov(kernel, D, rng)
    ell = _ells(kernel, h_cov, D)
    H = gpm.prior_block(KID[kernel], degree, h_cov, D)
    x = rng.uniform(-1, 1, (1, D))

    def k(a, b):
        return orc.covariance(kernel, h_cov, a, b, degree=degree)[0, 0]

    assert abs(H[0] - k(x, x)) <= 1e-14 * H[0]
    tol = 1e-3 if degree == 3 else 1e-5
    for l in range(D):
        e = np.zeros((1, D))
        e[0, l] = 1e-4 * ell[l]
        hh = e[0, l]
        d2 = (k(x + e, x + e) - k(x + e, x - e) - k(x - e, x + e) + k(x - e, x - e)) / (4 * hh * hh)
        assert abs(d2 - H[1 + l]) <= tol * H[1 + l], (l, d2, H[1 + l])
        assert abs(k(x + e, x) - k(x - e, x)) / (2 * hh) <= 1e-9 * H[0] / ell[l]
        for m in range(l):
            g = np.zeros((1, D))
            g[0, m] = 1e-4 * ell[m]
            d2o = (k(x + e, x + g) - k(x + e, x - g) - k(x - e, x + g) + k(x - e, x - g)) / (4 * hh * g[0, m])
            assert abs(d2o) <= 1e-6 * np.sqrt(H[1 + l] * H[1 + m])


@pytest.mark.parametrize("kernel,degree", FAMILIES)
@pytest.mark.parametrize("D", [1, 3])
def test_operand_against_central_differences(kernel, degree, D):
    """Slot 0 is the oracle's cross covariance (1e-13); slot 1 + l its central difference in x*_l with h = 1e-5 ell
    (truncation ~h^2 = 1e-10, rounding eps / h ~ 1e-11 of the scale: 1e-7 of the largest entry asserted).  Queries off
    the training points, plus one that IS a training point: its own pair has derivative entries exactly 0."""
    rng = np.random.default_rng(4)
    h_cov = _hyp_cov(kernel, D, rng)
    ell = _ells(kernel, h_cov, D)
    X = rng.uniform(-2, 2, (40, D))
    xs = np.vstack([rng.uniform(-2, 2, (6, D)), X[7:8]])
    B = gpm.operand(KID[kernel], degree, h_cov, X, xs)
    Ks = orc.covariance(kernel, h_cov, X, xs, degree=degree)
    assert np.abs(B[:, 0, :] - Ks).max() <= 1e-13 * Ks.max()
    assert np.all(B[7, 1:, 6] == 0)
    for l in range(D):
        e = np.zeros(D)
        e[l] = 1e-5 * ell[l]
        fd = (orc.covariance(kernel, h_cov, X, xs + e, degree=degree)
              - orc.covariance(kernel, h_cov, X, xs - e, degree=degree)) / (2 * e[l])
        fd[7, 6] = 0  # (the coincident pair: the convention, not the limit of the difference quotient)
        assert np.abs(B[:, 1 + l, :] - fd).max() <= 1e-7 * np.abs(fd).max(), (l, np.abs(B[:, 1 + l, :] - fd).max())


def _problem(kernel, degree, N, D, sn, seed=1, S=2):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (N, D))
    y = np.sin(X.sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1))
    model = dict(kernel=kernel, degree=degree, mean="const", noise=(1, 0, 0))
    cov_N = orc.cov_count(kernel, D)
    hyp = np.zeros((S, cov_N + 2))
    hyp[:, :1 if kernel.endswith("_iso") else D] = np.log(1.2)
    hyp[:, cov_N] = np.log(sn)
    hyp += 0.05 * rng.standard_normal(hyp.shape)
    hyp[:, cov_N] = np.log(sn)
    xs = rng.uniform(-1.8, 1.8, (12, D))
    return model, X, y, hyp, xs


def _full_cov(model, p, X, pts):
    """The oracle's full predictive covariance of the latent function at pts under posterior p (reference :1561-1661)."""
    D = X.shape[1]
    h = p.hyp[:orc.cov_count(model["kernel"], D)]
    Ks = orc.covariance(model["kernel"], h, X, pts, degree=model["degree"])
    Kss = orc.covariance(model["kernel"], h, pts, degree=model["degree"])
    if p.L_chol:
        V = sla.solve_triangular(p.L, p.sW * Ks, trans=1, check_finite=False)
        return Kss - V.T @ V
    return Kss + Ks.T @ (p.L @ Ks)


def _joint(model, p, X, xs):
    D = X.shape[1]
    h = p.hyp[:orc.cov_count(model["kernel"], D)]
    return gpm.joint(KID[model["kernel"]], model["degree"], h, X, xs, p.alpha, p.sW, p.L, p.L_chol)


# L_chol = 1: the problem of the tolerance measurement (N = 200, D = 3, ell ~ 1.2, sn2 = 0.01).  L_chol = 0 needs
# sn2 < 1e-6; the stencil's rounding enters as eps cond(K + sn2 I) / (4 h^2), so that case takes N = 25 points (cond
# ~1e6: ~1e-16 1e6 / 6e-6 = 2e-5 of the scale, under the 1e-4 asserted).
@pytest.mark.parametrize("kernel,degree,tol", [("se", 0, 1e-4), ("matern", 5, 1e-4), ("rq", 0, 1e-4), ("matern", 3, 1e-2),
                                               ("matern_iso", 5, 1e-4)])
@pytest.mark.parametrize("lchol", [1, 0])
def test_joint_covariance_against_stencil(kernel, degree, tol, lchol):
    D = 3
    model, X, y, hyp, xs = _problem(kernel, degree, 200 if lchol else 25, D, 0.1 if lchol else 9e-4)
    posts = orc.posteriors(model, hyp, X, y, None)
    for p in posts:
        assert bool(p.L_chol) == bool(lchol)
        ell = _ells(kernel, p.hyp, D)
        hs = 1e-3 * ell
        mean, C = _joint(model, p, X, xs)
        assert np.array_equal(C, np.transpose(C, (0, 2, 1))) or np.abs(C - np.transpose(C, (0, 2, 1))).max() < 1e-12
        for j in range(xs.shape[0]):
            pts = np.vstack([xs[j:j + 1]] + [xs[j] + s * hs[l] * np.eye(D)[l] for l in range(D) for s in (1, -1)])
            T = np.zeros((D + 1, 2 * D + 1))
            T[0, 0] = 1
            for l in range(D):
                T[1 + l, 1 + 2 * l], T[1 + l, 2 + 2 * l] = 0.5 / hs[l], -0.5 / hs[l]
            fd = T @ _full_cov(model, p, X, pts) @ T.T
            err = np.abs(C[j] - fd).max()
            assert err <= tol * np.abs(C[j]).max(), (kernel, degree, lchol, j, err / np.abs(C[j]).max())


@pytest.mark.parametrize("kernel,degree", [("se", 0), ("matern", 3), ("matern", 5), ("rq", 0), ("se_iso", 0)])
@pytest.mark.parametrize("lchol", [1, 0])
def test_identities_with_predict_and_predict_grad(kernel, degree, lchol):
    """[0, 0] is the oracle's fs2, [0, 1:] half the variance gradient of test_gpu_predict_grad._numpy_grads, the mean
    its dmu and the oracle's fmu: 1e-12 of the largest entry each (L_chol = 0: the two sides share L = -inv and
    differ by the order of the products only)."""
    from test_gpu_predict_grad import _numpy_grads

    D = 3
    model, X, y, hyp, xs = _problem(kernel, degree, 60 if lchol else 25, D, 0.1 if lchol else 9e-4)
    posts = orc.posteriors(model, hyp, X, y, None)
    mu, s2 = orc.predict(model, posts, X, y, xs, separate_samples=True)
    rdmu, rds2 = _numpy_grads(model, posts, X, xs, mu, s2)
    cov_N = orc.cov_count(kernel, D)
    for s, p in enumerate(posts):
        assert bool(p.L_chol) == bool(lchol)
        mean, C = _joint(model, p, X, xs)
        assert np.all(s2[:, s] > 0)
        assert np.abs(C[:, 0, 0] - s2[:, s]).max() <= 1e-12 * np.abs(C).max()
        assert np.abs(C[:, 0, 1:] - 0.5 * rds2[:, :, s]).max() <= 1e-12 * max(np.abs(C).max(), np.abs(rds2).max())
        assert np.abs(mean[:, 1:] - rdmu[:, :, s]).max() <= 1e-12 * np.abs(rdmu).max()
        m0 = p.hyp[cov_N + 1]  # the constant mean
        assert np.abs(mean[:, 0] + m0 - mu[:, s]).max() <= 1e-12 * np.abs(mu).max()


def test_mixture_moments():
    """The equal-weight mixture of S Gaussians N(m_s, C_s) has mean = mean_s m_s and covariance mean_s C_s + the
    POPULATION covariance of the m_s (closed form: E[x x^T] - E[x] E[x]^T); the library's convention (predict's) uses
    divisor S - 1 for the spread, so mix = mean_s C_s + np.cov(m, ddof=1) exactly, and its spread term is S / (S - 1)
    times the closed form's.  S = 1 returns the sample."""
    rng = np.random.default_rng(5)
    M, P, S = 4, 3, 5
    mean = rng.standard_normal((M, P, S))
    A = rng.standard_normal((M, P, P, S))
    cov = np.einsum("mabs,mcbs->macs", A, A)
    mm, mc = gpm.mix(mean, cov)
    for j in range(M):
        second = np.mean([cov[j, :, :, s] + np.outer(mean[j, :, s], mean[j, :, s]) for s in range(S)], axis=0)
        true_cov = second - np.outer(mm[j], mm[j])
        spread = true_cov - cov[j].mean(2)
        assert np.allclose(mm[j], mean[j].mean(1), rtol=0, atol=1e-15)
        assert np.allclose(mc[j] - cov[j].mean(2), spread * S / (S - 1), rtol=1e-12, atol=1e-14)
        assert np.allclose(mc[j], cov[j].mean(2) + np.cov(mean[j], ddof=1), rtol=1e-13, atol=1e-15)
    dm, dv = gpm.mix_diag(mean, np.einsum("maas->mas", cov))
    assert np.array_equal(dm, mm) and np.allclose(dv, np.einsum("maa->ma", mc), rtol=1e-13, atol=1e-15)
    one_m, one_c = gpm.mix(mean[:, :, :1], cov[:, :, :, :1])
    assert np.array_equal(one_m, mean[:, :, 0]) and np.array_equal(one_c, cov[:, :, :, 0])
    one_m, one_v = gpm.mix_diag(mean[:, :, :1], mean[:, :, :1] ** 2)
    assert np.array_equal(one_m, mean[:, :, 0]) and np.array_equal(one_v, mean[:, :, 0] ** 2)


def test_host_side_refusals():
    import gpyreg_amd as gpr

    for kid in (KID["matern"], KID["matern_iso"]):
        with pytest.raises(NotImplementedError, match="degree 1"):
            gpm.check_kind(kid, 1)
        with pytest.raises(NotImplementedError, match="degree 1"):
            gpm.prior_block(kid, 1, np.zeros(3), 2)
    assert gpm.f0(KID["matern"], 1, 1.0) == np.inf  # (why: the functor's F at distance 0)

    class MyMean(gpr.mean_functions.ConstantMean):
        pass

    # (GP.gradient_posterior itself holds the device context's lock, as its neighbours do: the refusals through the GP
    # are in tests/test_gpu_gradient_posterior.py; here the host functions it calls)
    from gpyreg_amd.gaussian_process import _mean_grad_x

    with pytest.raises(NotImplementedError, match=r"gradient_posterior: .*MyMean"):
        _mean_grad_x(MyMean(), np.zeros(1), np.zeros((3, 2)), "gradient_posterior")
    assert np.array_equal(_mean_grad_x(gpr.mean_functions.ConstantMean(), np.zeros(1), np.zeros((3, 2)),
                                       "gradient_posterior"), np.zeros((3, 2)))
