"""gpyreg_amd._cvgrad, the NumPy restatement of GP.cv_nll_batch (the oracle of the GPU tests): value and gradient of the
leave-one-out objective against torch.autograd of an independent textbook statement (for every point, condition on the
other N - 1 by a solve and evaluate the Gaussian log density or the squared error of y_i), for every family, mean,
noise variant and loss; against sixth-order differences of its own value in longdouble; the identities; the refusals
that never reach the device; the new ABI symbols.  No device."""

import os
import re

import numpy as np
import pytest
import torch

import gpyreg_amd as gpr
from gpyreg_amd import _cvgrad as cg
from gpyreg_amd import _nllhess as nh

KID = {"se": 0, "matern": 1, "rq": 2, "se_iso": 3, "matern_iso": 4}
FAMILIES = [("se", 0), ("matern", 3), ("matern", 5), ("rq", 0), ("se_iso", 0), ("matern_iso", 3), ("matern_iso", 5)]
N, D = 30, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEANS = {"zero": (gpr.mean_functions.ZeroMean, 0), "const": (gpr.mean_functions.ConstantMean, 1),
         "negquad": (gpr.mean_functions.NegativeQuadratic, 1 + 2 * D)}
NOISES = {"scalar": (dict(constant_add=True), 1),
          "per_point": (dict(constant_add=True, user_provided_add=True, scale_user_provided=True), 2)}


def _data(n=N, seed=3):
    """Points about one lengthscale apart, one of them duplicated, and smooth observations."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-3.0, 3.0, (n, D))
    X[7] = X[3]
    y = np.sin(X.sum(1) / np.sqrt(D)) + 0.1 * rng.standard_normal(n)
    s2 = rng.uniform(0.005, 0.02, n)
    return X, y, s2


def _cov_hyp(kernel, rng):
    nl = 1 if kernel.endswith("_iso") else D
    h = [np.log(1.9) + 0.1 * rng.standard_normal(nl), [np.log(1.3)]]
    if kernel == "rq":
        h.append([np.log(1.7)])
    return np.concatenate(h)


def _mean_hyp(name, rng):
    if name == "zero":
        return np.zeros(0)
    if name == "const":
        return np.array([0.2])
    return np.concatenate([[0.3], 0.3 * rng.standard_normal(D), np.log(4.0) + 0.1 * rng.standard_normal(D)])


def _noise_hyp(name):
    return np.array([np.log(0.1)]) if name == "scalar" else np.array([np.log(0.1), np.log(1.5)])


def _case(kernel, mean, noise, seed=11):
    rng = np.random.default_rng(seed)
    X, y, s2 = _data()
    return X, y, s2, np.concatenate([_cov_hyp(kernel, rng), _noise_hyp(noise), _mean_hyp(mean, rng)])


def _torch_loo(h, kernel, degree, mean, noise, loss, X, y, s2, w):
    """The textbook statement: for each i the Gaussian conditional of y_i given the other points, by a solve."""
    X, y, s2, w = torch.tensor(X), torch.tensor(y), torch.tensor(s2), torch.tensor(w)
    n = X.shape[0]
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
    sn2 = torch.exp(2 * hn[0]) * torch.ones(n, dtype=torch.float64)
    if noise == "per_point":
        sn2 = sn2 + torch.exp(hn[1]) * s2
    hm = h[cov_N + NOISES[noise][1]:]
    m = torch.zeros(n, dtype=torch.float64)
    if mean == "const":
        m = m + hm[0]
    if mean == "negquad":
        m = hm[0] - 0.5 * (((X - hm[1:1 + D]) / torch.exp(hm[1 + D:])) ** 2).sum(1)
    Sig = K + torch.diag(sn2)
    total = torch.zeros((), dtype=torch.float64)
    for i in range(n):
        o = [j for j in range(n) if j != i]
        sol = torch.linalg.solve(Sig[o][:, o], torch.stack([(y - m)[o], Sig[o, i]], 1))
        mu = m[i] + Sig[i, o] @ sol[:, 0]
        var = Sig[i, i] - Sig[i, o] @ sol[:, 1]
        if loss == "lpd":
            total = total + w[i] * (0.5 * torch.log(2 * np.pi * var) + 0.5 * (y[i] - mu) ** 2 / var)
        else:
            total = total + w[i] * (y[i] - mu) ** 2
    return total


def _restated(hyp, kernel, degree, mean, noise, loss, X, y, s2, weights=None, dtype=np.float64, **kw):
    cov_N = nh.cov_count(KID[kernel], D)
    nN = NOISES[noise][1]
    nobj = gpr.noise_functions.GaussianNoise(**NOISES[noise][0])
    mobj = MEANS[mean][0]()
    s2a = s2 if noise == "per_point" else None
    hn, hm = hyp[cov_N:cov_N + nN], hyp[cov_N + nN:]
    sn2, dsn2 = nobj.values(hn[None], X, y, s2a, True)
    if mobj.hyperparameter_count(D):
        m, dm = mobj.values(hm[None], X, True)
        dm = dm[0]
    else:
        m, dm = np.zeros((1, X.shape[0])), None
    ds = dsn2[0] if nobj.per_point(y, s2a) else dsn2[0, :1]
    return cg.cv_nll(KID[kernel], degree, hyp[:cov_N], X, y - m[0], sn2[0], 1.0, dm, ds, loss, weights, dtype=dtype, **kw)


def _bound(ref):
    return 1e-10 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("loss", ["lpd", "mse"])
@pytest.mark.parametrize("noise", ["scalar", "per_point"])
@pytest.mark.parametrize("mean", ["zero", "const", "negquad"])
@pytest.mark.parametrize("kernel,degree", FAMILIES)
def test_restatement_matches_textbook_autograd(kernel, degree, mean, noise, loss):
    X, y, s2, hyp = _case(kernel, mean, noise)
    weighted = (kernel, mean, noise) == ("matern", "negquad", "per_point")  # non-uniform weights, a zero among them
    w = np.random.default_rng(5).uniform(0.2, 2.0, N) if weighted else np.ones(N)
    if weighted:
        w[4] = 0.0
    h = torch.tensor(hyp, requires_grad=True)
    val = _torch_loo(h, kernel, degree, mean, noise, loss, X, y, s2, w)
    grad = torch.autograd.grad(val, h)[0].numpy()
    L, g = _restated(hyp, kernel, degree, mean, noise, loss, X, y, s2, w if weighted else None)
    print(f"{kernel}{degree} {mean} {noise} {loss}: |dL| = {abs(L - val.item()):.2e}, |dg| = {np.abs(g - grad).max():.2e}, "
          f"max|g| = {np.abs(grad).max():.2e}")
    assert abs(L - val.item()) <= _bound(val.item())
    assert np.abs(g - grad).max() <= _bound(grad)


# sixth-order central differences: f'(x) h = sum_k c_k (f(x + k h) - f(x - k h))
_FD6 = ((1, 3 / 4), (2, -3 / 20), (3, 1 / 60))


def _value_ld(hyp, kernel, degree, loss, X, y, w=None):
    """L in longdouble, constant mean and scalar noise formed in longdouble as well: hyp = [cov | log sn | m0]."""
    ld = np.longdouble
    cov_N = nh.cov_count(KID[kernel], D)
    hyp = np.asarray(hyp, dtype=ld)
    sn2 = np.exp(2 * hyp[cov_N])
    return cg.cv_nll(KID[kernel], degree, hyp[:cov_N], X, np.asarray(y, dtype=ld) - hyp[cov_N + 1], sn2, 1.0, loss=loss,
                     weights=w, dtype=ld, compute_grad=False)[0]


@pytest.mark.parametrize("loss", ["lpd", "mse"])
@pytest.mark.parametrize("log_sn", [-1.0, -4.0])
@pytest.mark.parametrize("kernel,degree", [("se", 0), ("matern", 3), ("matern", 5), ("rq", 0), ("se_iso", 0),
                                           ("matern_iso", 5)])
def test_restatement_matches_longdouble_differences(kernel, degree, log_sn, loss):
    ld = np.longdouble
    X, y, _ = _data(40)
    rng = np.random.default_rng(11)
    hyp = np.concatenate([_cov_hyp(kernel, rng), [log_sn], [0.2]])
    cov_N = nh.cov_count(KID[kernel], D)
    n = X.shape[0]
    L, g = cg.cv_nll(KID[kernel], degree, hyp[:cov_N], X, y - hyp[-1], np.exp(2 * log_sn), 1.0, np.ones((n, 1)),
                     np.array([[2 * np.exp(2 * log_sn)]]), loss)
    assert abs(L - float(_value_ld(hyp, kernel, degree, loss, X, y))) <= _bound(L)
    step = ld(1) / 256  # truncation ~ step^6 f^(7) / 140; rounding ~ 1e-19 cond(Sigma) / step
    fd = np.zeros(hyp.size, dtype=ld)
    for p in range(hyp.size):
        e = np.zeros(hyp.size, dtype=ld)
        e[p] = step
        for k, ck in _FD6:
            fd[p] += ld(ck) * (_value_ld(hyp + k * e, kernel, degree, loss, X, y)
                               - _value_ld(hyp - k * e, kernel, degree, loss, X, y))
    fd = (fd / step).astype(float)
    err = np.abs(g - fd).max() / max(1.0, np.abs(fd).max())
    print(f"{kernel}{degree} log sn = {log_sn} {loss}: {err:.2e} of max(1, largest entry {np.abs(fd).max():.2e})")
    assert err <= 1e-8


def test_longdouble_agrees_with_float64():
    X, y, s2, hyp = _case("matern", "negquad", "per_point")
    L, g = _restated(hyp, "matern", 5, "negquad", "per_point", "lpd", X, y, s2)
    Ll, gl = _restated(hyp, "matern", 5, "negquad", "per_point", "lpd", X, y, s2, dtype=np.longdouble)
    assert gl.dtype == np.longdouble
    assert abs(L - Ll) <= 1e-11 * abs(L) and np.abs(g - gl).max() <= 1e-11 * np.abs(g).max()


@pytest.mark.parametrize("loss", ["lpd", "mse"])
@pytest.mark.parametrize("iso,ard,degree", [("se_iso", "se", 0), ("matern_iso", "matern", 5)])
def test_isotropic_is_tied_ard(iso, ard, degree, loss):
    X, y, s2 = _data()
    tail = np.array([np.log(1.3), np.log(0.1), 0.2])
    Li, gi = _restated(np.r_[np.log(1.9), tail], iso, degree, "const", "scalar", loss, X, y, s2)
    La, ga = _restated(np.r_[np.full(D, np.log(1.9)), tail], ard, degree, "const", "scalar", loss, X, y, s2)
    tied = np.r_[ga[:D].sum(), ga[D:]]
    assert abs(Li - La) <= 1e-12 * max(1.0, abs(La))
    assert np.abs(gi - tied).max() <= 1e-12 * max(1.0, np.abs(tied).max())


@pytest.mark.parametrize("kernel,degree", FAMILIES)
def test_mse_is_invariant_to_a_common_scale(kernel, degree):
    """Scaling sf^2 and sn^2 together scales Sigma and leaves the leave-one-out means where they are."""
    X, y, s2, hyp = _case(kernel, "const", "scalar")
    cov_N = nh.cov_count(KID[kernel], D)
    sf = 1 if kernel.endswith("_iso") else D
    _, g = _restated(hyp, kernel, degree, "const", "scalar", "mse", X, y, s2)
    assert abs(g[sf]) > 1e-3  # (not a vacuous cancellation)
    assert abs(g[sf] + g[cov_N]) <= 1e-10 * max(1.0, np.abs(g).max())


@pytest.mark.parametrize("loss", ["lpd", "mse"])
def test_unit_weights_are_no_weights(loss):
    X, y, s2, hyp = _case("rq", "negquad", "per_point")
    L0, g0 = _restated(hyp, "rq", 0, "negquad", "per_point", loss, X, y, s2)
    L1, g1 = _restated(hyp, "rq", 0, "negquad", "per_point", loss, X, y, s2, np.ones(N))
    assert L0 == L1 and np.array_equal(g0, g1)


def test_refusals_without_device():
    with pytest.raises(NotImplementedError, match="degree 1"):
        cg.check_kind(1, 1)
    with pytest.raises(NotImplementedError, match="degree 1"):
        cg.cv_nll(4, 1, np.zeros(2), np.zeros((3, D)), np.zeros(3), 0.01)

    class MyNoise(gpr.noise_functions.GaussianNoise):
        pass

    class MyMean(gpr.mean_functions.ConstantMean):
        pass

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
        for call in (lambda: gp.cv_nll_batch(h), lambda: gp.cv_nll_batch(), lambda: gp.log_pseudo_likelihood(h[0]),
                     lambda: gp.log_pseudo_likelihood(h[0], compute_grad=True)):
            with pytest.raises(NotImplementedError, match=msg):
                call()
    gp = gpr.GP(D, se(), zero, const)
    X, y, _ = _data()
    gp.update(X_new=X, y_new=y[:, None], hyp=h, compute_posterior=False)
    for kw, msg in ((dict(loss="nlpd"), "loss must be one of"),
                    (dict(weights=np.ones(N - 1)), "weights must have shape"),
                    (dict(weights=np.ones((N, 1))), "weights must have shape"),
                    (dict(weights=-np.ones(N)), "finite and >= 0"),
                    (dict(weights=np.r_[np.nan, np.ones(N - 1)]), "finite and >= 0"),
                    (dict(weights=np.r_[np.inf, np.ones(N - 1)]), "finite and >= 0")):
        with pytest.raises(ValueError, match=msg):
            gp.cv_nll_batch(h, **kw)
    assert gp._cv_grad_check("cv_nll_batch", "mse", list(range(N))).dtype == np.float64


def test_abi_declares_and_binds_the_new_entry_points():
    from gpyreg_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpcore.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gpc_\w+)\s*\(", header))
    for name in ("gpc_cv_grad", "gpc_debug_cv_trace", "gpc_debug_cv_weights"):
        assert name in declared and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["gpc_cv_grad"][1]) == 9
    for method in ("cv_nll_batch", "log_pseudo_likelihood", "_cv_grad_check"):
        assert callable(getattr(gpr.GP, method))
