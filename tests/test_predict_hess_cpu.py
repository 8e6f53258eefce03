"""gpyreg_amd._hess, the NumPy restatement of GP.predict_hess (the oracle of the GPU tests): the per-record Hessians of
the predictive mean and variance against automatic differentiation of an independent torch.float64 statement, the
mixture formula against autograd of _mix_samples' moments, a query ON a training point, the refusals and the prior's
pieces.  No device: the GP method holds the device context's lock, so here it is entered below the lock (its refusals
and the prior's mean-only path never reach the device); the prior WITH its variance -- the covariance object's own diagonal,
evaluated on the device -- is in tests/test_gpu_predict_hess.py."""

import numpy as np
import pytest
import torch

from gpyreg_amd import _hess as hm
from oracle import gp_oracle as orc

KID = {"se": 0, "matern": 1, "rq": 2, "se_iso": 3, "matern_iso": 4}
FAMILIES = [("se", 0), ("matern", 3), ("matern", 5), ("rq", 0), ("se_iso", 0), ("matern_iso", 3), ("matern_iso", 5)]
N, M = 40, 7


def _problem(kernel, degree, D, sn, S=1, seed=5):
    """Well-spread points (about one lengthscale apart in every D, so that K + Sigma stays well conditioned at any
    noise) and queries at least 0.1 lengthscale from every one of them."""
    rng = np.random.default_rng(seed + D)
    half = {1: 20.0, 3: 3.0, 10: 3.0}[D]
    X = rng.uniform(-half, half, (N, D))
    y = np.sin(X.sum(1, keepdims=True) / np.sqrt(D))
    model = dict(kernel=kernel, degree=degree, mean="const", noise=(1, 0, 0))
    cov_N = orc.cov_count(kernel, D)
    nl = 1 if kernel.endswith("_iso") else D
    hyp = np.zeros((S, cov_N + 2))
    hyp[:, :nl] = np.log(1.1 * (np.sqrt(D) if D > 1 else 1.0))
    hyp[:, nl] = np.log(1.3)
    if kernel == "rq":
        hyp[:, nl + 1] = np.log(1.7)
    hyp[:, :cov_N] += 0.05 * rng.standard_normal((S, cov_N))
    hyp[:, cov_N] = np.log(sn)
    hyp[:, cov_N + 1] = 0.1
    ell = np.exp(hyp[:, :nl]).max()
    cand = rng.uniform(-half, half, (40 * M, D))
    dist = np.sqrt(((cand[:, None, :] - X[None, :, :]) ** 2).sum(2)).min(1)
    xs = cand[dist >= 0.12 * ell][:M]
    assert xs.shape[0] == M
    posts = orc.posteriors(model, hyp, X, y, None)
    return model, X, hyp, xs, posts


def _kinv(p):
    """(K + Sigma)^-1 of a posterior record, dense."""
    if p.L_chol:
        sW = p.sW[:, 0]
        return sW[:, None] * np.linalg.inv(p.L.T @ p.L) * sW[None, :]
    return -p.L


def _torch_kernel(kernel, degree, h, D):
    """x (D,), X (N, D) -> k(X, x) (N,): the textbook formula straight from the lengthscales, not through F / G."""
    nl = 1 if kernel.endswith("_iso") else D
    ell = torch.tensor(np.exp(h[:nl]) * np.ones(D))
    sf2 = float(np.exp(2 * h[nl]))

    def k(x, X):
        r2 = (((x[None, :] - X) / ell) ** 2).sum(1)
        if kernel.startswith("se"):
            return sf2 * torch.exp(-r2 / 2)
        if kernel.startswith("matern"):
            r = torch.sqrt(degree * r2)
            poly = 1 + r if degree == 3 else 1 + r + r * r / 3
            return sf2 * poly * torch.exp(-r)
        a = float(np.exp(h[nl + 1]))
        return sf2 * (1 + r2 / (2 * a)) ** (-a)

    return k, sf2


def _torch_moments(kernel, degree, D, X, p):
    """x -> (mu, s2) of one posterior record, without the mean function."""
    cov_N = orc.cov_count(kernel, D)
    k, sf2 = _torch_kernel(kernel, degree, p.hyp[:cov_N], D)
    Xt, al, Ki = torch.tensor(X), torch.tensor(p.alpha[:, 0]), torch.tensor(_kinv(p))

    def mu(x):
        return k(x, Xt) @ al

    def s2(x):
        kx = k(x, Xt)
        return sf2 - kx @ (Ki @ kx)

    return mu, s2


def _hessians(f, xs):
    return np.stack([torch.autograd.functional.hessian(f, torch.tensor(x)).numpy() for x in xs])


# (largest deviation seen over all cases: 1.9e-14 of the largest entry for Hmu, 7.3e-11 for Hs2)
@pytest.mark.parametrize("kernel,degree", FAMILIES)
@pytest.mark.parametrize("D", [1, 3, 10])
@pytest.mark.parametrize("sn", [0.1, 1e-4])
def test_record_against_automatic_differentiation(kernel, degree, D, sn, record_property):
    """Hmu and Hs2 of one record (sn = 0.1: L_chol; sn = 1e-4: low noise, L = -(K + Sigma)^-1) against torch's double
    backward of an independent statement of the predictive mean and variance, to 1e-8 of the largest entry of each
    Hessian (the project's fp64 parity figure; autograd is exact to rounding).  The values and gradients ride along."""
    model, X, hyp, xs, posts = _problem(kernel, degree, D, sn)
    p = posts[0]
    assert bool(p.L_chol) == (sn > 1e-3)
    cov_N = orc.cov_count(kernel, D)
    mu, s2, dmu, ds2, Hmu, Hs2 = hm.record(KID[kernel], degree, p.hyp[:cov_N], X, xs, p.alpha, p.sW, p.L, p.L_chol)
    fm, fv = _torch_moments(kernel, degree, D, X, p)
    rHmu, rHs2 = _hessians(fm, xs), _hessians(fv, xs)
    e_mu = np.abs(Hmu - rHmu).max() / np.abs(rHmu).max()
    e_s2 = np.abs(Hs2 - rHs2).max() / np.abs(rHs2).max()
    print(f"predict_hess autograd deviation {kernel}{degree} D={D} sn={sn}: Hmu {e_mu:.2e} Hs2 {e_s2:.2e}")
    record_property("deviation", (e_mu, e_s2))
    assert e_mu <= 1e-8 and e_s2 <= 1e-8, (e_mu, e_s2)
    assert np.array_equal(Hmu, np.transpose(Hmu, (0, 2, 1))) and np.array_equal(Hs2, np.transpose(Hs2, (0, 2, 1)))
    for j, x in enumerate(xs):
        xt = torch.tensor(x, requires_grad=True)
        m, v = fm(xt), fv(xt)
        gm, = torch.autograd.grad(m, xt)
        gv, = torch.autograd.grad(fv(xt), xt)
        assert abs(mu[j] - m.item()) <= 1e-10 * np.abs(mu).max() and abs(s2[j] - v.item()) <= 1e-10 * np.abs(s2).max()
        assert np.abs(dmu[j] - gm.numpy()).max() <= 1e-9 * np.abs(dmu).max()
        assert np.abs(ds2[j] - gv.numpy()).max() <= 1e-9 * np.abs(ds2).max()


@pytest.mark.parametrize("kernel,degree", [("matern", 5), ("rq", 0)])
def test_mixture_against_autograd_of_the_mixed_moments(kernel, degree):
    """S = 3: the Hessians of _mix_samples' moments -- mean of the means; mean of the variances plus the spread of the
    means with divisor S - 1 -- by autograd, against mix() of the per-record results; 1e-8 of the largest entry."""
    from gpyreg_amd.gaussian_process import _mix_samples

    D, S = 3, 3
    model, X, hyp, xs, posts = _problem(kernel, degree, D, 0.1, S=S)
    cov_N = orc.cov_count(kernel, D)
    recs = [hm.record(KID[kernel], degree, p.hyp[:cov_N], X, xs, p.alpha, p.sW, p.L, p.L_chol) for p in posts]
    mu, s2, dmu, ds2, Hmu, Hs2 = [np.stack([r[i] for r in recs], -1) for i in range(6)]
    fs = [_torch_moments(kernel, degree, D, X, p) for p in posts]

    def mixed_mean(x):
        return sum(f[0](x) for f in fs) / S

    def mixed_var(x):
        ms = torch.stack([f[0](x) for f in fs])
        return sum(f[1](x) for f in fs) / S + ((ms - ms.mean()) ** 2).sum() / (S - 1)

    # (the torch statement is _mix_samples': same numbers at the queries)
    centre, total, _ = _mix_samples(mu, s2)
    x0 = torch.tensor(xs[0])
    assert abs(mixed_mean(x0).item() - centre[0, 0]) <= 1e-12 * abs(centre[0, 0])
    assert abs(mixed_var(x0).item() - total[0, 0]) <= 1e-10 * abs(total[0, 0])
    gHmu, gHs2 = hm.mix(mu, dmu, Hmu, Hs2)
    rHmu, rHs2 = _hessians(mixed_mean, xs), _hessians(mixed_var, xs)
    assert np.abs(gHmu - rHmu).max() <= 1e-8 * np.abs(rHmu).max()
    assert np.abs(gHs2 - rHs2).max() <= 1e-8 * np.abs(rHs2).max()
    assert np.array_equal(gHs2, np.transpose(gHs2, (0, 2, 1)))
    # one sample is returned as it is; without the variance there is no variance Hessian
    a, b = hm.mix(mu[:, :1], dmu[..., :1], Hmu[..., :1], Hs2[..., :1])
    assert np.array_equal(a, Hmu[..., 0]) and np.array_equal(b, Hs2[..., 0])
    a, b = hm.mix(mu, dmu, Hmu, None)
    assert np.array_equal(a, gHmu) and b is None


@pytest.mark.parametrize("kernel,degree", [("se", 0), ("matern", 3), ("matern", 5), ("rq", 0)])
@pytest.mark.parametrize("sn", [0.1, 1e-4])
def test_query_on_a_training_point(kernel, degree, sn):
    """x* = X[3]: finite; equal to the engine's value at x* + 1e-7 e_1 to 1e-5 of the largest entry (continuity: the
    Hessians are Lipschitz with constant O(1) in lengthscale units -- Matern 3 included, whose G is infinite at the
    coincident pair while G d_a d_b -> 0); symmetric to the bit."""
    D = 3
    model, X, hyp, xs, posts = _problem(kernel, degree, D, sn)
    p = posts[0]
    cov_N = orc.cov_count(kernel, D)
    e1 = np.zeros(D)
    e1[0] = 1e-7
    at = hm.record(KID[kernel], degree, p.hyp[:cov_N], X, X[3:4], p.alpha, p.sW, p.L, p.L_chol)
    near = hm.record(KID[kernel], degree, p.hyp[:cov_N], X, X[3:4] + e1, p.alpha, p.sW, p.L, p.L_chol)
    for i in (4, 5):
        assert np.all(np.isfinite(at[i]))
        assert np.abs(at[i] - near[i]).max() <= 1e-5 * np.abs(near[i]).max(), (i, np.abs(at[i] - near[i]).max())
        assert np.array_equal(at[i], np.transpose(at[i], (0, 2, 1)))
    # the coincident pair: nothing from the G term, the whole -F(0) on the diagonal
    c, diff, k, F, G = hm.pair_terms(KID[kernel], degree, p.hyp[:cov_N], X, X[3:4])
    _, sf2, rqa = hm.scaling(KID[kernel], degree, p.hyp[:cov_N], D)
    assert G[3, 0] == 0 and F[3, 0] == hm._gpm.f0(KID[kernel], degree, sf2, rqa)


def _host(gp, *a, **k):
    """GP.predict_hess without the device context's lock: everything up to the first device call runs on the host."""
    import gpyreg_amd as gpr

    return gpr.GP.predict_hess.__wrapped__(gp, *a, **k)


def test_refusals():
    """Matern 1, a user-defined covariance and a user-defined mean are refused before anything touches the device."""
    import gpyreg_amd as gpr
    from gpyreg_amd.covariance_functions import AbstractKernel

    for kind in (1, 4):
        with pytest.raises(NotImplementedError, match="predict_hess: the Matern kernel of degree 1 has no second derivative"):
            hm.check_kind(kind, 1)
    with pytest.raises(ValueError, match="unknown kernel id"):
        hm.check_kind(7, 0)
    noise = gpr.noise_functions.GaussianNoise(constant_add=True)
    xs = np.zeros((3, 2))
    for cov_obj, n in ((gpr.covariance_functions.Matern(1), 3), (gpr.isotropic_covariance_functions.MaternIsotropic(1), 2)):
        g1 = gpr.GP(2, cov_obj, gpr.mean_functions.ConstantMean(), noise)
        g1.update(hyp=np.zeros((1, n + 2)))
        with pytest.raises(NotImplementedError, match="predict_hess: the Matern kernel of degree 1"):
            _host(g1, xs)

    class MyMean(gpr.mean_functions.ConstantMean):
        pass

    with pytest.raises(NotImplementedError, match="predict_hess: the mean function .*MyMean.* is user-defined"):
        hm.mean_hess(MyMean(), np.zeros(1), np.zeros((2, 3)))
    gm = gpr.GP(2, gpr.covariance_functions.SquaredExponential(), MyMean(), noise)
    gm.update(hyp=np.zeros((1, 5)))
    with pytest.raises(NotImplementedError, match="predict_hess: the mean function .*MyMean"):
        _host(gm, xs)

    class MyCov(AbstractKernel):
        """A covariance without a device kernel."""

        def hyperparameter_count(self, D):
            return D + 1

        def compute(self, hyp, X, X_star=None, compute_diag=False, compute_grad=False):
            raise AssertionError("predict_hess must refuse before it evaluates a user-defined covariance")

    gk = gpr.GP(2, MyCov(), gpr.mean_functions.ConstantMean(), noise)
    gk.posteriors = np.empty(0, dtype=object)
    with pytest.raises(NotImplementedError, match="predict_hess: the covariance function .*MyCov.* is user-defined"):
        _host(gk, xs)


def test_prior_pieces_without_data():
    """A GP without data returns the mean function's Hessian and Hs2 = 0: the stock means' Hessians against autograd of
    their formulas, and the mixture of constant per-sample priors."""
    import gpyreg_amd as gpr

    Dd = 3
    xs = np.random.default_rng(2).uniform(-1, 1, (4, Dd))
    assert np.all(hm.mean_hess(gpr.mean_functions.ZeroMean(), np.zeros(0), xs) == 0)
    assert np.all(hm.mean_hess(gpr.mean_functions.ConstantMean(), np.zeros(1), xs) == 0)
    h = np.r_[0.3, 0.1, -0.2, 0.4, 0.2, -0.1, 0.3]  # m0, xm (D), omega (D)
    H = hm.mean_hess(gpr.mean_functions.NegativeQuadratic(), h, xs)
    xm, om = torch.tensor(h[1:1 + Dd]), torch.tensor(np.exp(h[1 + Dd:]))
    ref = _hessians(lambda x: h[0] - 0.5 * (((x - xm) / om) ** 2).sum(), xs)
    assert H.shape == (4, Dd, Dd) and np.abs(H - ref).max() <= 1e-14
    m = np.reshape(gpr.mean_functions.NegativeQuadratic().compute(h, xs), (-1,))
    assert np.abs(m - np.array([(h[0] - 0.5 * (((x - h[1:4]) / np.exp(h[4:])) ** 2).sum()) for x in xs])).max() <= 1e-14
    # two prior samples: Hs2 = 0 per sample, the mixture adds the spread of the mean functions alone
    mu = np.stack([m, m + 1.0], 1)
    dmu = np.zeros((4, Dd, 2))
    Hm = np.stack([H, H], 3)
    a, b = hm.mix(mu, dmu, Hm, np.zeros((4, Dd, Dd, 2)))
    assert np.array_equal(a, H) and np.all(b == 0)
    # through the method, without the variance (the prior variance is the covariance object's, evaluated on the device)
    gp = gpr.GP(Dd, gpr.covariance_functions.Matern(5), gpr.mean_functions.NegativeQuadratic(),
                gpr.noise_functions.GaussianNoise(constant_add=True))
    hyp = np.stack([np.r_[0.1, -0.2, 0.3, 0.2, np.log(0.1), h], np.r_[0.0, 0.2, 0.1, 0.1, np.log(0.1), h + 0.1]])
    gp.update(hyp=hyp)
    mu_s, s2_s, dmu_s, ds2_s, Hmu_s, Hs2_s = _host(gp, xs, compute_var=False, separate_samples=True)
    assert s2_s is None and ds2_s is None and Hs2_s is None
    assert mu_s.shape == (4, 2) and dmu_s.shape == (4, Dd, 2) and Hmu_s.shape == (4, Dd, Dd, 2)
    assert np.array_equal(Hmu_s[..., 0], H) and np.array_equal(mu_s[:, 0], m)
    assert np.array_equal(Hmu_s[..., 1], hm.mean_hess(gp.mean, h + 0.1, xs))
    out = _host(gp, xs, compute_var=False)
    assert [None if o is None else o.shape for o in out] == [(4,), None, (4, Dd), None, (4, Dd, Dd), None]
    assert np.allclose(out[4], (Hmu_s[..., 0] + Hmu_s[..., 1]) / 2, rtol=1e-15)
