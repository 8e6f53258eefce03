"""Hyperparameter gradients of the gradient-observation likelihood on the device: gobs_trace_kernel alone
(gpc_debug_gobs_trace) against the extended-precision planes of tests/gradobs_grad_ref.py, then
GP.nll_batch_grad_obs(compute_grad=True) end to end against gpyreg_amd._gradobs.nll_grad, the same answer as the
planes-through-nll_batch_K route, invariance, and the Python layer (log_posterior_grad_obs, L-BFGS, refusals)."""

import numpy as np
import pytest

import gradobs_grad_ref as ggr
import gradobs_ref as gr
from test_cov_functors_cpu import LD
from test_gpu_gradobs import KID, _problem, _reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from gpyreg_amd import _lib

    return _lib.context(0)


# ---- the kernel alone --------------------------------------------------------------------------------------------------
SHAPES = [
    (3, 2, 1),
    (70, 37, 3),   # partial tiles of both kinds
    (64, 64, 2),   # exact tiles
    (5, 70, 2),    # gradient blocks that straddle a tile edge
    (6, 3, 33),    # D above DCH
]


@pytest.mark.parametrize("N,Ng,D", SHAPES)
@pytest.mark.parametrize("name,alpha", gr.FAMILIES)
def test_kernel_alone(ctx, name, alpha, N, Ng, D):
    """out_p = sum_IJ (Ainv / sl - alpha alpha^T)_IJ dK_IJ / dtheta_p against the longdouble sum of weight x plane, every
    output within 1e-12 sum |weight| |terms of the entry| (the bound of the sibling contraction test in
    test_gpu_cv_grad.py).  Data: gradobs_ref.setup's ladder -- X_g repeats rows of X and of itself, so r2 = 0 off the
    diagonal in every kind of block, for Matern 3 and 5 too.  The strict upper triangle of the supplied matrix is NaN:
    the kernel reads the lower triangle only.  Two calls give identical bits."""
    case = gr.setup(name, alpha, N, Ng, D, 0.0)
    kind, degree, hyp, X, Xg = (case[k] for k in ("kind", "degree", "hyp", "X", "Xg"))
    n = N + Ng * D
    rng = np.random.default_rng(100 * N + Ng + D)
    A = rng.standard_normal((n, n))
    A = A + A.T
    al = rng.standard_normal(n)
    sl = 0.37
    given = A.copy()
    given[np.triu_indices(n, 1)] = np.nan
    got = ctx.debug_gobs_trace(kind, degree, hyp, X, Xg, given, al, sl)
    again = ctx.debug_gobs_trace(kind, degree, hyp, X, Xg, given, al, sl)
    dK, mag = ggr.planes_ld(case)
    W = A.astype(LD) / LD(sl) - np.outer(al.astype(LD), al.astype(LD))
    want = np.array([np.sum(W * dK[p]) for p in range(dK.shape[0])])
    bound = 1e-12 * np.array([np.sum(np.abs(W).astype(np.float64) * mag[p]) for p in range(dK.shape[0])])
    assert got.shape == want.shape and np.all(np.isfinite(got))
    err = np.abs(got.astype(LD) - want).astype(np.float64)
    print(f"{name} {alpha} ({N},{Ng},{D}): worst error / bound {np.max(err / bound):.3e}")
    assert np.all(err <= bound), (name, alpha, got, want.astype(np.float64), err / bound)
    assert np.array_equal(got, again)
    assert ctx.get_option("gobs_trace_us") >= 0


# ---- end to end --------------------------------------------------------------------------------------------------------
def _joint_derivative_rows(gp, X, Xg, h, counts, mean):
    """(dm (n, mean_N) | None, dsn2 (n, 1)) of one hyperparameter vector, put together HERE from the stock plugins."""
    from gpyreg_amd import _gradobs as go

    cov_N, noise_N, mean_N = counts
    N, D = X.shape
    Ng = Xg.shape[0]
    hm = h[cov_N + noise_N:]
    dm = None
    if mean_N:
        dm = go.joint_dm(gp.mean.values(hm[None, :], X, True)[1][0], go.mean_xgrad_dhyp(mean, hm, Xg))
    dsn2 = np.zeros((N + Ng * D, 1))
    dsn2[:N] = 2 * np.exp(2 * h[cov_N])  # GaussianNoise(constant_add): sn2 = exp(2 theta)
    return dm, dsn2


def _close(a, b, rtol):
    """|a - b| <= rtol max(1, largest entry of b)."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return a.shape == b.shape and np.all(np.isfinite(a)) and np.abs(a - b).max() <= rtol * max(1.0, np.abs(b).max())


# joint orders n = 70 (one leaf), 190 and 360
E2E = [(40, 10, 3, "rq", 0), (100, 30, 3, "matern", 5), (120, 80, 3, "matern_iso", 3)]


@pytest.mark.parametrize("mean", ["zero", "const", "negquad"])
@pytest.mark.parametrize("N,Ng,D,kernel,degree", E2E)
def test_end_to_end_against_numpy(N, Ng, D, kernel, degree, mean):
    """nll_batch_grad_obs(compute_grad=True) against _gradobs.nll_grad on _gradobs.posterior's record, per sample within
    1e-8 max(1, largest entry); S = 3 with the middle sample on the low-noise branch (value noise 5e-7 < 1e-6); nlZ is
    the compute_grad=False result bit for bit."""
    from gpyreg_amd import _gradobs as go

    gp, model, X, y, Xg, dy, hyp, counts = _problem(N, Ng, D, kernel, degree, mean, seed=21,
                                                    sn_rows=np.array([0.1, np.sqrt(5e-7), 0.1]))
    cov_N = counts[0]
    s2g = 0.01
    posts = _reference(gp, model, X, y, Xg, dy, hyp, counts, s2g)
    assert [p["L_chol"] for p in posts] == [True, False, True] and all(p["sn2_mult"] == 1 for p in posts)
    nlz0 = gp.nll_batch_grad_obs(hyp, Xg, dy, s2g)
    nlz, g = gp.nll_batch_grad_obs(hyp, Xg, dy, s2g, compute_grad=True)
    assert np.array_equal(nlz, nlz0) and g.shape == hyp.shape
    for s, p in enumerate(posts):
        dm, dsn2 = _joint_derivative_rows(gp, X, Xg, hyp[s], counts, mean)
        want = go.nll_grad(KID[kernel], degree, hyp[s, :cov_N], X, Xg, p, dm, dsn2)
        err = np.abs(g[s] - want).max() / max(1.0, np.abs(want).max())
        print(f"n = {N + Ng * D} {kernel} {mean} sample {s}: {err:.2e} (largest entry {np.abs(want).max():.3e})")
        assert _close(g[s], want, 1e-8), (s, g[s], want)


def test_same_answer_as_the_planes_route(ctx):
    """The model's joint matrix and derivative planes through nll_batch_K with a dK callback (the route a user had
    before) at n = 190: gradients agree to 1e-8."""
    from gpyreg_amd import _gradobs as go
    from gpyreg_amd import _lib

    rng = np.random.default_rng(12)
    N, Ng, D, S = 100, 30, 3, 2
    X, Xg = rng.uniform(-2, 2, (N, D)), rng.uniform(-2, 2, (Ng, D))
    y, dy = np.sin(X.sum(1)), rng.standard_normal((Ng, D))
    n = N + Ng * D
    kid, degree = KID["rq"], 0
    hyp_cov = np.log(1.5) + 0.1 * rng.standard_normal((S, D + 2))
    m = 0.1 * rng.standard_normal((S, n))
    sn2 = 0.01 * rng.uniform(0.5, 2, (S, n))
    dm = rng.standard_normal((S, n, 2))
    dsn2 = rng.uniform(size=(S, n, 1)) * sn2[:, :, None]
    ctx.set_data_gobs(X, y, Xg, dy)
    nlz1, g1, mult1, lchol1, info1 = ctx.nll_batch_gobs_grad(kid, degree, _lib.F64, hyp_cov, m, sn2, dm, dsn2)
    K = np.stack([go.joint_cov(kid, degree, h, X, Xg) for h in hyp_cov])
    dK = [go.joint_cov_dhyp(kid, degree, h, X, Xg) for h in hyp_cov]
    ctx.set_data(np.zeros((n, D)), go.to_joint(y, dy))
    nlz2, g2, mult2, lchol2, info2 = ctx.nll_batch_K(_lib.F64, K, lambda s, p: np.ascontiguousarray(dK[s][p]), D + 2, m,
                                                     sn2, True, True, dm, dsn2)
    assert np.all(info1 == 0) and np.all(info2 == 0) and np.array_equal(mult1, mult2)
    assert g1.shape == g2.shape == (S, D + 2 + 1 + 2)
    for s in range(S):
        assert _close(g1[s], g2[s], 1e-8), (s, g1[s], g2[s])
    assert _close(nlz1, nlz2, 1e-8)
    with pytest.raises(RuntimeError, match="fp64 only"):
        ctx.set_data_gobs(X, y, Xg, dy)
        ctx.nll_batch_gobs_grad(kid, degree, _lib.F32, hyp_cov, m, sn2, dm, dsn2)


# ---- invariance ----------------------------------------------------------------------------------------------------------
def test_rows_alone_and_reordered_give_the_same_bits_and_the_gp_is_untouched():
    gp, model, X, y, Xg, dy, hyp, counts = _problem(70, 20, 3, "se", 0, "negquad", S=3, seed=9)
    rows = np.concatenate([hyp, hyp[:1] + 0.05])
    xs = np.random.default_rng(5).uniform(-2, 2, (33, 3))
    before = (gp.predict(xs, separate_samples=True), gp.nll_batch(hyp, compute_grad=True),
              [np.array(p.alpha) for p in gp.posteriors])
    nlz, g = gp.nll_batch_grad_obs(rows, Xg, dy, 0.01, compute_grad=True)
    for s in range(rows.shape[0]):
        z1, g1 = gp.nll_batch_grad_obs(rows[s], Xg, dy, 0.01, compute_grad=True)
        assert np.array_equal(z1, nlz[s:s + 1]) and np.array_equal(g1[0], g[s]), s
    perm = np.array([2, 0, 3, 1])
    zp, gp_ = gp.nll_batch_grad_obs(rows[perm], Xg, dy, 0.01, compute_grad=True)
    assert np.array_equal(zp, nlz[perm]) and np.array_equal(gp_, g[perm])
    after = (gp.predict(xs, separate_samples=True), gp.nll_batch(hyp, compute_grad=True),
             [np.array(p.alpha) for p in gp.posteriors])
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0]))
    assert all(np.array_equal(a, b) for a, b in zip(before[1], after[1]))
    assert all(np.array_equal(a, b) for a, b in zip(before[2], after[2]))
    assert np.array_equal(gp.X, X) and np.array_equal(gp.y, y) and len(gp.posteriors) == 3


# ---- the Python layer ----------------------------------------------------------------------------------------------------
def _with_priors(gp):
    """A Student-t prior on the first block of hyperparameters, Gaussian ones on the others, inside wide bounds."""
    P = gp._hyp_N()
    gp.set_bounds(gp.bounds_to_dict(np.full(P, -8.0), np.full(P, 8.0)))
    pri = {}
    for i, (name, cnt) in enumerate(gp._hyper_info()):
        z, two = np.zeros(cnt), np.full(cnt, 2.0)
        pri[name] = ("student_t", (z, two, np.full(cnt, 3.0))) if i == 0 else ("gaussian", (z, two))
    gp.set_priors(pri)
    return gp.hyper_priors


def test_log_posterior_grad_obs_and_lbfgs():
    """log_posterior_grad_obs = -(nll_batch_grad_obs) + log prior, value and gradient, array or dict; its gradient
    agrees with central differences of its value (1e-6 max(1, largest entry)); twenty L-BFGS-B steps from a perturbed
    start lower the objective."""
    import scipy.optimize as so

    from gpyreg_amd import priors as pr

    gp, model, X, y, Xg, dy, hyp, counts = _problem(60, 15, 2, "matern", 5, "const", S=1, seed=31)
    hp = _with_priors(gp)
    h = hyp[0]
    nlz, g = gp.nll_batch_grad_obs(h, Xg, dy, 0.01, compute_grad=True)
    lp, dlp = pr.log_priors(h, hp, gp.lower_bounds, gp.upper_bounds, gp.normalization_constants, True)
    val, grad = gp.log_posterior_grad_obs(h, Xg, dy, 0.01, compute_grad=True)
    assert val == -(nlz[0] - lp) and np.array_equal(grad, -(g[0] - dlp))
    assert gp.log_posterior_grad_obs(h, Xg, dy, 0.01) == val
    lz, dlz = gp.log_likelihood_grad_obs(h, Xg, dy, 0.01, compute_grad=True)
    assert lz == -nlz[0] and np.array_equal(dlz, -g[0]) and gp.log_likelihood_grad_obs(h, Xg, dy, 0.01) == lz
    as_dict = gp.hyperparameters_to_dict(h[None, :])[0]
    assert gp.log_posterior_grad_obs(as_dict, Xg, dy, 0.01) == val
    fd = np.empty(h.size)
    for p in range(h.size):
        e = np.zeros(h.size)
        e[p] = 1e-5
        fd[p] = (gp.log_posterior_grad_obs(h + e, Xg, dy, 0.01) - gp.log_posterior_grad_obs(h - e, Xg, dy, 0.01)) / 2e-5
    assert np.abs(grad - fd).max() <= 1e-6 * max(1.0, np.abs(fd).max()), (grad, fd)

    obj = lambda t: tuple(-v for v in gp.log_posterior_grad_obs(t, Xg, dy, 0.01, compute_grad=True))
    start = h + 0.5 * np.random.default_rng(2).standard_normal(h.size)
    res = so.minimize(obj, start, jac=True, method="L-BFGS-B", options={"maxiter": 20})
    assert np.isfinite(res.fun) and res.fun < obj(start)[0] - 1e-3, (res.fun, obj(start)[0])


def test_refusals():
    import gpyreg_amd as gpr

    gp, model, X, y, Xg, dy, hyp, counts = _problem(30, 8, 2, "matern", 5, "const", S=1, seed=10, dtype="f32")
    assert np.all(np.isfinite(gp.nll_batch_grad_obs(hyp, Xg, dy, 0.01)))  # (the value alone has no such limit)
    with pytest.raises(NotImplementedError, match="fp64"):
        gp.nll_batch_grad_obs(hyp, Xg, dy, 0.01, compute_grad=True)
    with pytest.raises(NotImplementedError, match="fp64"):
        gp.log_posterior_grad_obs(hyp[0], Xg, dy, 0.01, compute_grad=True)

    gp, model, X, y, Xg, dy, hyp, counts = _problem(30, 8, 2, "matern", 1, "const", S=1, seed=10)
    with pytest.raises(NotImplementedError, match="degree 1"):
        gp.nll_batch_grad_obs(hyp, Xg, dy, 0.01, compute_grad=True)

    class MyMean(gpr.mean_functions.ConstantMean):
        pass

    class MyNoise(gpr.noise_functions.GaussianNoise):
        pass

    class MyCov(gpr.covariance_functions.SquaredExponential):
        _gpc_kernel_id = None  # (what makes a covariance object user-defined: it goes through its own compute())

    rng = np.random.default_rng(0)
    X, Xg = rng.uniform(-2, 2, (20, 2)), rng.uniform(-2, 2, (5, 2))
    y, dy = np.sin(X.sum(1, keepdims=True)), rng.standard_normal((5, 2))
    parts = dict(cov=gpr.covariance_functions.SquaredExponential, mean=gpr.mean_functions.ConstantMean,
                 noise=lambda: gpr.noise_functions.GaussianNoise(constant_add=True))
    for swap, make, match in (("mean", MyMean, "mean function"), ("noise", lambda: MyNoise(constant_add=True), "noise function"),
                              ("cov", MyCov, "covariance function")):
        p = dict(parts, **{swap: make})
        gp = gpr.GP(2, p["cov"](), p["mean"](), p["noise"]())
        h = np.zeros((1, 2 + 1 + 1 + 1))
        gp.update(X_new=X, y_new=y, hyp=h, compute_posterior=False)
        with pytest.raises(NotImplementedError, match=match):
            gp.nll_batch_grad_obs(h, Xg, dy, 0.01, compute_grad=True)
