"""gpyreg_amd._hypgrad, the NumPy restatement of GP.predict_hyp_grad (the oracle of the GPU tests): predict's values on
the golden core cases, central differences of its own prediction at a fixed multiplier for every family, mean and
noise variant in both noise regimes, the scaling identities at rounding level, the delta-method assembly of
GP.predict_laplace on a stubbed GP, the refusals that never reach the device and the new ABI symbols.  No device."""

import os
import re

import numpy as np
import pytest

import gpyreg_amd as gpr
from conftest import parse_core_name
from gpyreg_amd import _hypgrad as hg
from gpyreg_amd import _nllhess as nh

KID = {"se": 0, "matern": 1, "rq": 2, "se_iso": 3, "matern_iso": 4}
FAMILIES = [("se", 0), ("matern", 3), ("matern", 5), ("rq", 0), ("se_iso", 0), ("matern_iso", 3), ("matern_iso", 5)]
D = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEANS = {"zero": gpr.mean_functions.ZeroMean, "const": gpr.mean_functions.ConstantMean,
         "negquad": gpr.mean_functions.NegativeQuadratic}


def _noise_obj(p):
    return gpr.noise_functions.GaussianNoise(constant_add=p[0] == 1, user_provided_add=p[1] >= 1,
                                             scale_user_provided=p[1] == 2,
                                             rectified_linear_output_dependent_add=p[2] == 1)


def _restated(kind, degree, mobj, nobj, hyp, X, y, s2, xs, mult=1.0, dtype=np.float64, var=True):
    """_hypgrad.hyp_grad at one hyperparameter vector with the stock plugins' values and derivatives, in ``dtype``.
    Returns (fmu, fs2, dfmu, dfs2) of the LATENT prediction without the mean function."""
    N, Dx = X.shape
    hyp = np.asarray(hyp, dtype=dtype)
    cov_N, nN = nh.cov_count(kind, Dx), nobj.hyperparameter_count()
    hn, hm = hyp[cov_N:cov_N + nN], hyp[cov_N + nN:]
    sn2, dsn2 = nobj.values(hn[None], X, y, s2, True)
    vec = nobj.per_point(y, s2)
    ds = None if nN == 0 else (dsn2[0] if vec else dsn2[0, :1])
    if mobj.hyperparameter_count(Dx):
        m, dm = mobj.values(hm[None], X, True)
        dm = dm[0]
    else:
        m, dm = np.zeros((1, N), dtype=dtype), None
    return hg.hyp_grad(kind, degree, hyp[:cov_N], X, xs, np.reshape(y, (-1,)) - m[0], sn2[0], mult, dm, ds, var, dtype=dtype)


# ---- 1. predict's values on the golden core cases ---------------------------------------------------------------------


def test_reproduces_predict_on_the_golden_core_cases(core_golden):
    """fmu + m(x*) and max(fs2, 0) against the stored per-sample predictions of every golden model but Matern 1, at the
    stored multipliers, to (1e-8 + 1e-14 cond(K + Sigma)) of max(1, largest entry): the project's fp64 bound, plus what
    two different factorizations of an ill-conditioned matrix may differ by (the low-noise and jitter flavours).  A
    sample whose bound exceeds 1 % is not compared; every plain case is."""
    g = core_golden
    done = plain = 0
    for name in g["names"]:
        tag, model, N, Dx, flavour = parse_core_name(name)
        if model["kernel"].startswith("matern") and model["degree"] == 1:
            continue
        kind = KID[model["kernel"]]
        X, y, hyp, xs = g[tag + "_X"], g[tag + "_y"], g[tag + "_hyp"], g[tag + "_xs"]
        s2 = g[tag + "_s2"] if tag + "_s2" in g.files else None
        mobj, nobj = MEANS[model["mean"]](), _noise_obj(model["noise"])
        cov_N, nN = nh.cov_count(kind, Dx), nobj.hyperparameter_count()
        for s in range(hyp.shape[0]):
            mult = g[tag + "_sn2_mult"][s]
            sn2 = np.broadcast_to(nobj.values(hyp[s:s + 1, cov_N:cov_N + nN], X, y, s2)[0], (N,))
            K = nh.cov_derivatives(kind, model["degree"], hyp[s, :cov_N], X)[0]
            tol = 1e-8 + 1e-14 * np.linalg.cond(K + np.diag(mult * sn2))
            if tol > 1e-2:
                assert flavour != "plain", name
                continue
            fmu, fs2, dfmu, dfs2 = _restated(kind, model["degree"], mobj, nobj, hyp[s], X, y, s2, xs, mult=mult)
            mu = fmu + mobj.values(hyp[s:s + 1, cov_N + nN:], xs)[0]
            want_mu, want_s2 = g[tag + "_mu_sep"][:, s], g[tag + "_s2_sep"][:, s]
            assert np.abs(mu - want_mu).max() <= tol * max(1.0, np.abs(want_mu).max()), (name, s)
            assert np.abs(np.maximum(fs2, 0) - want_s2).max() <= tol * max(1.0, np.abs(want_s2).max()), (name, s)
            assert dfmu.shape == (xs.shape[0], hyp.shape[1]) and dfs2.shape == dfmu.shape
            assert np.all(np.isfinite(dfmu)) and np.all(np.isfinite(dfs2))
            done += 1
            plain += flavour == "plain"
    assert plain >= 26 and done > plain, (done, plain)


# ---- 2. central differences of its own prediction ---------------------------------------------------------------------


def _problem(kernel, N, sn, mean, per_point, seed=5):
    """D = 3, X uniform in [-2, 2], lengthscales about 1; one query ON a training point."""
    rng = np.random.default_rng(seed + N)
    X = rng.uniform(-2.0, 2.0, (N, D))
    y = np.sin(X.sum(1) / np.sqrt(D)) + 0.1 * rng.standard_normal(N)
    xs = rng.uniform(-2.0, 2.0, (6, D))
    xs[0] = X[N // 2]
    nl = 1 if kernel.endswith("_iso") else D
    hc = [0.1 * rng.standard_normal(nl), [np.log(1.3)]]
    if kernel == "rq":
        hc.append([np.log(1.7)])
    if per_point:
        nobj = _noise_obj((1, 2, 0))
        hn, s2 = [np.log(sn), np.log(1.5)], rng.uniform(0.5, 2.0, N) * sn**2
    else:
        nobj, hn, s2 = _noise_obj((1, 0, 0)), [np.log(sn)], None
    hm = [0.2] if mean == "const" else np.r_[0.3, 0.3 * rng.standard_normal(D), np.log(4.0) + 0.1 * rng.standard_normal(D)]
    return X, y, s2, xs, nobj, MEANS[mean](), np.concatenate(hc + [hn, hm])


@pytest.mark.parametrize("sn", [0.3, 3e-4])
@pytest.mark.parametrize("mean,per_point,N", [("const", False, 40), ("negquad", True, 40), ("const", True, 130),
                                              ("negquad", False, 130)])
@pytest.mark.parametrize("kernel,degree", FAMILIES)
def test_central_differences_of_its_own_prediction(kernel, degree, mean, per_point, N, sn):
    """Every column of dfmu and dfs2 against central differences of (fmu, fs2) at the multiplier held at 1, to 1e-6 of the
    column's largest entry.  The differences are the sixth-order central stencil
    (f(3h) - 9 f(2h) + 45 f(h) - 45 f(-h) + 9 f(-2h) - f(-3h)) / 60h at h = 1e-2, formed in extended precision; the
    closed form under test runs in fp64.  Why not the plain two-point difference in fp64: at sn = 3e-4 several columns
    are tiny against the values they differentiate -- d fs2 / d log sn is 4e-6 where fs2 is 1e-2, and the log sf and
    log sn columns of the mean are differences of nearly equal terms that vanish with the noise -- so the rounding of
    the differences, (error of f) / h, is measured against a column 1e4 times smaller than f.  With the values good
    to ~2e-14 in longdouble (cond(K + Sigma) up to 1e7 here) that needs h near 1e-2 to stay below 1e-6 of such a column;
    the stencil's truncation, h^6 / 140 times a seventh derivative whose ratio to the first is a few hundred on log
    scales, is then ~1e-12.  The two-point difference at h = 1e-4 leaves a truncation error of 1e-5 in the log sn
    columns (measured against the closed form evaluated in longdouble, which the fp64 closed form matches to 1e-7).
    (A zero column -- the variance against a mean hyperparameter -- must be matched by zero differences.)"""
    kind = KID[kernel]
    X, y, s2, xs, nobj, mobj, th = _problem(kernel, N, sn, mean, per_point)
    fmu, fs2, dfmu, dfs2 = _restated(kind, degree, mobj, nobj, th, X, y, s2, xs)
    h = np.longdouble(1e-2)
    worst = 0.0
    thl = th.astype(np.longdouble)
    for p in range(th.size):
        e = np.zeros(th.size, dtype=np.longdouble)
        e[p] = h
        f = {k: _restated(kind, degree, mobj, nobj, thl + k * e, X, y, s2, xs, dtype=np.longdouble)
             for k in (-3, -2, -1, 1, 2, 3)}
        for which, an, i in (("dfmu", dfmu[:, p], 0), ("dfs2", dfs2[:, p], 1)):
            fd = ((f[3][i] - 9 * f[2][i] + 45 * f[1][i] - 45 * f[-1][i] + 9 * f[-2][i] - f[-3][i]) / (60 * h)).astype(float)
            scale = np.abs(an).max()
            if scale == 0:
                assert np.abs(fd).max() <= 1e-12, (which, p)
                continue
            err = np.abs(fd - an).max() / scale
            worst = max(worst, err)
            assert err <= 1e-6, (kernel, degree, mean, per_point, N, sn, which, p, err)
    print(f"{kernel}{degree} {mean} per_point={per_point} N={N} sn={sn}: worst column error {worst:.2e}")


# ---- 3. identities at rounding level ----------------------------------------------------------------------------------


@pytest.mark.parametrize("kernel,degree", FAMILIES)
def test_scaling_identities(kernel, degree):
    """With constant noise alone, scaling sf and sn together scales K + Sigma: the mean does not move and the latent
    variance scales with sf^2 -- dmu/dlog sf + dmu/dlog sn = 0 and ds2/dlog sf + ds2/dlog sn = 2 s2, to 1e-12 of the
    larger term."""
    kind = KID[kernel]
    X, y, s2, xs, nobj, mobj, th = _problem(kernel, 40, 0.3, "const", False)
    fmu, fs2, dfmu, dfs2 = _restated(kind, degree, mobj, nobj, th, X, y, s2, xs)
    cov_N, sfc = nh.cov_count(kind, D), hg.sf_col(kind, D)
    a, b = dfmu[:, sfc], dfmu[:, cov_N]
    assert np.abs(a + b).max() <= 1e-12 * np.abs(a).max()
    a, b = dfs2[:, sfc], dfs2[:, cov_N]
    assert np.abs(a + b - 2 * fs2).max() <= 1e-12 * max(np.abs(a).max(), np.abs(b).max(), np.abs(fs2).max())


@pytest.mark.parametrize("iso,ard,degree", [("se_iso", "se", 0), ("matern_iso", "matern", 3), ("matern_iso", "matern", 5)])
def test_isotropic_equals_tied_ard(iso, ard, degree):
    """The isotropic lengthscale column is the sum of the ARD columns at tied lengthscales; every other column and the
    values agree, to 1e-12 of the largest entry."""
    X, y, s2, xs, nobj, mobj, th = _problem(iso, 40, 0.3, "negquad", True)
    a = _restated(KID[iso], degree, mobj, nobj, th, X, y, s2, xs)
    tied = np.r_[np.full(D, th[0]), th[1:]]
    b = _restated(KID[ard], degree, mobj, nobj, tied, X, y, s2, xs)
    for i in (0, 1):
        assert np.abs(a[i] - b[i]).max() <= 1e-12 * np.abs(b[i]).max()
    for i in (2, 3):
        folded = np.c_[b[i][:, :D].sum(1), b[i][:, D:]]
        assert np.abs(a[i] - folded).max() <= 1e-12 * max(np.abs(folded).max(), np.abs(b[i][:, :D]).max())


# ---- 4. predict_laplace's assembly ------------------------------------------------------------------------------------


def test_predict_laplace_assembly_on_a_stub(monkeypatch):
    """g^T Sigma g over the free coordinates only, from the first sample's gradients; the ValueError without a
    covariance."""
    from gp_stubs import _se_gp

    gp = _se_gp(D=2)
    rng = np.random.default_rng(3)
    M, P, S = 4, 5, 2
    mu, s2 = rng.standard_normal((M, S)), rng.uniform(0.1, 1.0, (M, S))
    dmu, ds2 = rng.standard_normal((M, P, S)), rng.standard_normal((M, P, S))
    seen = {}

    def stub(x_star, compute_var=True, add_noise=False, s2_star=None):
        seen.update(var=compute_var, noise=add_noise)
        return mu, s2, dmu, ds2

    monkeypatch.setattr(gp, "predict_hyp_grad", stub)
    free = np.array([0, 2, 3])
    A = rng.standard_normal((3, 3))
    cov = A @ A.T
    lap = dict(cov=cov, free=free, is_pd=True)
    out = gp.predict_laplace(np.zeros((M, 2)), lap, add_noise=True)
    assert seen == dict(var=True, noise=True)
    assert set(out) == {"mu", "s2", "var_mu", "var_s2", "s2_total"}
    for j in range(M):
        gm, gs = dmu[j, free, 0], ds2[j, free, 0]
        assert abs(out["var_mu"][j] - gm @ cov @ gm) <= 1e-13 * abs(gm @ cov @ gm)
        assert abs(out["var_s2"][j] - gs @ cov @ gs) <= 1e-13 * abs(gs @ cov @ gs)
    assert np.array_equal(out["mu"], mu[:, 0]) and np.array_equal(out["s2"], s2[:, 0])
    assert np.array_equal(out["s2_total"], s2[:, 0] + out["var_mu"])
    assert np.all(out["var_mu"] >= 0)
    with pytest.raises(ValueError, match="is_pd"):
        gp.predict_laplace(np.zeros((M, 2)), dict(cov=None, free=free, is_pd=False))


# ---- the refusals that need no device, the ABI ------------------------------------------------------------------------


def test_refusals_without_device():
    with pytest.raises(NotImplementedError, match="degree 1"):
        hg.check_kind(1, 1)

    class MyNoise(gpr.noise_functions.GaussianNoise):
        pass

    class MyMean(gpr.mean_functions.ConstantMean):
        pass

    zero, const = gpr.mean_functions.ZeroMean(), gpr.noise_functions.GaussianNoise(constant_add=True)
    se = gpr.covariance_functions.SquaredExponential

    class MyCov(se):
        _gpc_kernel_id = None

    xs = np.zeros((2, D))
    for gp, msg in ((gpr.GP(D, gpr.covariance_functions.Matern(1), zero, const), "predict_hyp_grad: .*degree 1"),
                    (gpr.GP(D, se(), zero, const, dtype="f32"), "predict_hyp_grad: .*fp64 only"),
                    (gpr.GP(D, se(), zero, MyNoise(constant_add=True)), "predict_hyp_grad: the noise function .*MyNoise"),
                    (gpr.GP(D, se(), MyMean(), const), "predict_hyp_grad: the mean function .*MyMean"),
                    (gpr.GP(D, MyCov(), zero, const), "predict_hyp_grad: the covariance function .*user-defined")):
        with pytest.raises(NotImplementedError, match=msg):
            gp.predict_hyp_grad(xs)
        with pytest.raises(NotImplementedError, match=msg):
            gp.predict_laplace(xs, dict(cov=np.eye(1), free=np.array([0])))


def test_abi_declares_and_binds_the_new_entry_points():
    from gpyreg_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpcore.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gpc_\w+)\s*\(", header))
    for name in ("gpc_predict_hyp_grad", "gpc_debug_hyp_cross"):
        assert name in declared and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["gpc_predict_hyp_grad"][1]) == 14
    assert len(_lib.SIGNATURES["gpc_debug_hyp_cross"][1]) == 14
