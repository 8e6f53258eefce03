"""gpyreg_amd._nllhess, the NumPy restatement of GP.nll_hess_batch (the oracle of the GPU tests): value, gradient and
Hessian of the negative log marginal likelihood against torch.autograd of an independent torch.float64 statement
written from the textbook kernels, for every family, mean and noise variant; the plugins' and the priors' second
derivatives against central differences of their own first derivatives; the longdouble path; symmetry; the refusals
that never reach the device; the new ABI symbols.  No device."""

import os
import re

import numpy as np
import pytest
import torch

import gpyreg_amd as gpr
from gpyreg_amd import _nllhess as nh
from gpyreg_amd import priors as pr

KID = {"se": 0, "matern": 1, "rq": 2, "se_iso": 3, "matern_iso": 4}
FAMILIES = [("se", 0), ("matern", 3), ("matern", 5), ("rq", 0), ("se_iso", 0), ("matern_iso", 3), ("matern_iso", 5)]
N, D = 40, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(seed=3):
    """Points about one lengthscale apart, one of them duplicated, and smooth observations."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-3.0, 3.0, (N, D))
    X[7] = X[3]
    y = np.sin(X.sum(1) / np.sqrt(D)) + 0.1 * rng.standard_normal(N)
    s2 = rng.uniform(0.005, 0.02, N)
    return X, y, s2


def _cov_hyp(kernel, rng):
    nl = 1 if kernel.endswith("_iso") else D
    h = [np.log(1.9) + 0.1 * rng.standard_normal(nl), [np.log(1.3)]]
    if kernel == "rq":
        h.append([np.log(1.7)])
    return np.concatenate(h)


MEANS = {"zero": (gpr.mean_functions.ZeroMean, 0), "const": (gpr.mean_functions.ConstantMean, 1),
         "negquad": (gpr.mean_functions.NegativeQuadratic, 1 + 2 * D)}
NOISES = {"const": (dict(constant_add=True), 1),
          "scaled": (dict(constant_add=True, user_provided_add=True, scale_user_provided=True), 2),
          "rect": (dict(constant_add=True, rectified_linear_output_dependent_add=True), 3)}


def _mean_hyp(name, rng):
    if name == "zero":
        return np.zeros(0)
    if name == "const":
        return np.array([0.2])
    return np.concatenate([[0.3], 0.3 * rng.standard_normal(D), np.log(4.0) + 0.1 * rng.standard_normal(D)])


def _noise_hyp(name, y):
    if name == "const":
        return np.array([np.log(0.1)])
    if name == "scaled":
        return np.array([np.log(0.1), np.log(1.5)])
    return np.array([np.log(0.1), float(np.median(y)), np.log(0.2)])  # threshold at the median: both signs of gap


def _torch_nll(h, kernel, degree, mean, noise, X, y, s2):
    """The textbook statement: K from the lengthscales, m and sn2 from the hyperparameters, a Cholesky-based NLL."""
    X, y, s2 = torch.tensor(X), torch.tensor(y), torch.tensor(s2)
    nl = 1 if kernel.endswith("_iso") else D
    cov_N = nh.cov_count(KID[kernel], D)
    ell = torch.exp(h[:nl]) * torch.ones(D, dtype=torch.float64)
    sf2 = torch.exp(2 * h[nl])
    diff = (X[:, None, :] - X[None, :, :]) / ell
    r2 = (diff**2).sum(2)
    if kernel.startswith("se"):
        K = sf2 * torch.exp(-r2 / 2)
    elif kernel == "rq":
        a = torch.exp(h[nl + 1])
        K = sf2 * (1 + r2 / (2 * a)) ** (-a)
    else:
        pos = r2 > 0  # (a masked square root: its derivatives at 0 are infinite, the chain rule's other factor is 0)
        t = torch.where(pos, torch.sqrt(degree * torch.where(pos, r2, torch.ones_like(r2))), torch.zeros_like(r2))
        K = sf2 * torch.exp(-t) * ((1 + t) if degree == 3 else (1 + t + t * t / 3))
    hn = h[cov_N:cov_N + NOISES[noise][1]]
    sn2 = torch.exp(2 * hn[0]) * torch.ones(N, dtype=torch.float64)
    if noise == "scaled":
        sn2 = sn2 + torch.exp(hn[1]) * s2
    if noise == "rect":
        sn2 = sn2 + torch.exp(2 * hn[2]) * torch.relu(hn[1] - y) ** 2
    hm = h[cov_N + NOISES[noise][1]:]
    m = torch.zeros(N, dtype=torch.float64)
    if mean == "const":
        m = m + hm[0]
    if mean == "negquad":
        m = hm[0] - 0.5 * (((X - hm[1:1 + D]) / torch.exp(hm[1 + D:])) ** 2).sum(1)
    L = torch.linalg.cholesky(K + torch.diag(sn2))
    z = torch.linalg.solve_triangular(L, (y - m)[:, None], upper=False)[:, 0]
    return 0.5 * (z @ z) + torch.log(torch.diagonal(L)).sum() + 0.5 * N * np.log(2 * np.pi)


def _restated(hyp, kernel, degree, mean, noise, X, y, s2, dtype=np.float64, plugins=True):
    cov_N = nh.cov_count(KID[kernel], D)
    nN = NOISES[noise][1]
    nobj = gpr.noise_functions.GaussianNoise(**NOISES[noise][0])
    mobj = MEANS[mean][0]()
    s2a = s2 if noise == "scaled" else None
    hn, hm = hyp[cov_N:cov_N + nN], hyp[cov_N + nN:]
    sn2, dsn2 = nobj.values(hn[None], X, y, s2a, True)
    if mobj.hyperparameter_count(D):
        m, dm = mobj.values(hm[None], X, True)
        dm = dm[0]
    else:
        m, dm = np.zeros((1, N)), None
    vec = nobj.per_point(y, s2a)
    ds = dsn2[0] if vec else dsn2[0, :1]
    return nh.nll_hess(KID[kernel], degree, hyp[:cov_N], X, y - m[0], sn2[0], 1.0, dm, ds,
                       nh.noise_d2(nobj, hn, X, y, s2a) if plugins else None,
                       nh.mean_d2(mobj, hm, X) if plugins else None, dtype=dtype)


def _case(kernel, mean, noise, seed=11):
    rng = np.random.default_rng(seed)
    X, y, s2 = _data()
    hyp = np.concatenate([_cov_hyp(kernel, rng), _noise_hyp(noise, y), _mean_hyp(mean, rng)])
    return X, y, s2, hyp


def _check_against_autograd(kernel, degree, mean, noise):
    X, y, s2, hyp = _case(kernel, mean, noise)
    h = torch.tensor(hyp, requires_grad=True)
    f = lambda v: _torch_nll(v, kernel, degree, mean, noise, X, y, s2)  # noqa: E731
    val = f(h)
    grad = torch.autograd.grad(val, h)[0].numpy()
    Href = torch.autograd.functional.hessian(f, h).numpy()
    nlz, g, H = _restated(hyp, kernel, degree, mean, noise, X, y, s2)
    scale = np.abs(Href).max()
    print(f"{kernel}{degree} {mean} {noise}: |dH| / max|H| = {np.abs(H - Href).max() / scale:.2e}, "
          f"|dg| / max|g| = {np.abs(g - grad).max() / np.abs(grad).max():.2e}")
    assert abs(nlz - val.item()) <= 1e-11 * abs(val.item())
    assert np.abs(g - grad).max() <= 1e-10 * np.abs(grad).max()
    assert np.abs(H - Href).max() <= 1e-10 * scale
    assert np.array_equal(H, H.T)


@pytest.mark.parametrize("mean", ["zero", "const", "negquad"])
@pytest.mark.parametrize("kernel,degree", FAMILIES)
def test_restatement_matches_autograd(kernel, degree, mean):
    _check_against_autograd(kernel, degree, mean, "const")


@pytest.mark.parametrize("noise", ["scaled", "rect"])
@pytest.mark.parametrize("kernel,degree", [("se", 0), ("rq", 0), ("matern_iso", 5)])
def test_noise_variants_match_autograd(kernel, degree, noise):
    X, y, _, hyp = _case(kernel, "const", noise)
    if noise == "rect":
        gap = hyp[nh.cov_count(KID[kernel], D) + 1] - y
        assert (gap > 0).any() and (gap < 0).any()
    _check_against_autograd(kernel, degree, "const", noise)


def test_longdouble_agrees_with_float64():
    X, y, s2, hyp = _case("matern", "negquad", "rect")
    _, g, H = _restated(hyp, "matern", 5, "negquad", "rect", X, y, s2)
    _, gl, Hl = _restated(hyp, "matern", 5, "negquad", "rect", X, y, s2, dtype=np.longdouble)
    assert Hl.dtype == np.longdouble
    assert np.abs(H - Hl).max() <= 1e-11 * np.abs(H).max()
    assert np.abs(g - gl).max() <= 1e-11 * np.abs(g).max()


def test_plugin_terms_are_separable():
    """What the device returns (no plugin second derivatives) plus the two plugin terms is the full Hessian."""
    X, y, s2, hyp = _case("se", "negquad", "rect")
    cov_N, nN = D + 1, 3
    _, _, Hfull = _restated(hyp, "se", 0, "negquad", "rect", X, y, s2)
    _, _, Hbare = _restated(hyp, "se", 0, "negquad", "rect", X, y, s2, plugins=False)
    diff = Hfull - Hbare
    assert np.abs(diff[:cov_N]).max() == 0 and np.abs(diff[cov_N:cov_N + nN, cov_N + nN:]).max() == 0
    assert np.abs(diff[cov_N:cov_N + nN, cov_N:cov_N + nN]).max() > 0 and np.abs(diff[cov_N + nN:, cov_N + nN:]).max() > 0


def _central(f, x, step=1e-5):
    cols = []
    for i in range(x.size):
        e = np.zeros(x.size)
        e[i] = step
        cols.append((f(x + e) - f(x - e)) / (2 * step))
    return np.stack(cols, axis=-1)


@pytest.mark.parametrize("noise", ["const", "scaled", "rect"])
def test_noise_second_derivatives(noise):
    X, y, s2 = _data()
    s2a = s2 if noise == "scaled" else None
    nobj = gpr.noise_functions.GaussianNoise(**NOISES[noise][0])
    h = _noise_hyp(noise, y) + (0.013 if noise == "rect" else 0.0)  # (no observation exactly at the threshold)
    d2 = nh.noise_d2(nobj, h, X, y, s2a)
    fd = _central(lambda v: nobj.values(v[None], X, y, s2a, True)[1][0], h)
    fd = fd if nobj.per_point(y, s2a) else fd[:1]
    assert d2.shape == fd.shape
    assert np.abs(d2 - fd).max() <= 1e-8 * max(1.0, np.abs(d2).max())
    assert np.array_equal(d2, np.transpose(d2, (0, 2, 1)))


@pytest.mark.parametrize("mean", ["zero", "const", "negquad"])
def test_mean_second_derivatives(mean):
    X, _, _ = _data()
    mobj = MEANS[mean][0]()
    h = _mean_hyp(mean, np.random.default_rng(2))
    d2 = nh.mean_d2(mobj, h, X)
    assert d2.shape == (N, h.size, h.size)
    if h.size:
        fd = _central(lambda v: mobj.values(v[None], X, True)[1][0], h)
        assert np.abs(d2 - fd).max() <= 1e-8 * max(1.0, np.abs(d2).max())


def test_prior_second_derivatives():
    """The four families (Gaussian, Student-t, smooth box, smooth box with Student-t shoulders), inside and outside the
    boxes on either side, and a uniform dimension: the diagonal against central differences of log_priors' gradient.
    (One dimension per smooth-box class: log_priors reproduces the reference's broadcasting over a class's dimensions,
    which raises for several of them in different regions.)"""
    P = 5
    hp = pr.empty_priors(P)
    hp["mu"][0], hp["sigma"][0], hp["df"][0] = 0.3, 0.7, 0
    hp["mu"][1], hp["sigma"][1], hp["df"][1] = -0.2, 1.1, 3
    hp["a"][2], hp["b"][2], hp["sigma"][2], hp["df"][2] = -1.0, 1.0, 0.5, 0
    hp["a"][3], hp["b"][3], hp["sigma"][3], hp["df"][3] = -1.0, 1.0, 0.5, 4
    lb, ub = np.full(P, -10.0), np.full(P, 10.0)
    nc = pr.normalization_constants(hp, lb, ub)
    for box, box_t in ((-1.7, 1.9), (0.2, -0.3), (1.6, -1.4)):
        hyp = np.array([0.9, 0.8, box, box_t, 0.4])
        d2 = nh.prior_d2(hyp, hp, lb, ub)
        fd = _central(lambda v: pr.log_priors(v, hp, lb, ub, nc, True)[1], hyp)
        assert np.abs(fd - np.diag(np.diag(fd))).max() == 0  # the priors are products over the dimensions
        assert np.abs(d2 - np.diag(fd)).max() <= 1e-8
        inside = abs(box) < 1
        assert d2[4] == 0 and (d2[2] == 0) == inside and (d2[3] == 0) == inside and d2[0] != 0 and d2[1] != 0


def test_refusals_without_device():
    with pytest.raises(NotImplementedError, match="degree 1"):
        nh.check_kind(1, 1)

    class MyNoise(gpr.noise_functions.GaussianNoise):
        pass

    class MyMean(gpr.mean_functions.ConstantMean):
        pass

    X, y, _ = _data()
    with pytest.raises(NotImplementedError, match="user-defined"):
        nh.noise_d2(MyNoise(constant_add=True), np.zeros(1), X, y)
    with pytest.raises(NotImplementedError, match="user-defined"):
        nh.mean_d2(MyMean(), np.zeros(1), X)
    # the GP's own refusals come before anything touches the device
    zero, const = gpr.mean_functions.ZeroMean(), gpr.noise_functions.GaussianNoise(constant_add=True)
    se = gpr.covariance_functions.SquaredExponential
    h = np.zeros((1, D + 2))

    class MyCov(se):
        _gpc_kernel_id = None

    for gp, msg in ((gpr.GP(D, gpr.covariance_functions.Matern(1), zero, const), "degree 1"),
                    (gpr.GP(D, se(), zero, const, dtype="f32"), "fp64 only"),
                    (gpr.GP(D, se(), zero, MyNoise(constant_add=True)), "noise function"),
                    (gpr.GP(D, se(), MyMean(), const), "mean function"),
                    (gpr.GP(D, MyCov(), zero, const), "covariance function")):
        for call in (lambda: gp.nll_hess_batch(h), lambda: gp.log_posterior_hess(h[0]),
                     lambda: gp.laplace_approximation(h[0])):
            with pytest.raises(NotImplementedError, match=msg):
                call()


def test_abi_declares_and_binds_the_new_entry_points():
    from gpyreg_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpcore.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gpc_\w+)\s*\(", header))
    for name in ("gpc_nll_hess", "gpc_debug_nll_plane", "gpc_debug_nll_d2", "gpc_debug_nll_gram"):
        assert name in declared and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["gpc_nll_hess"][1]) == 10
