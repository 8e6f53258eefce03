"""GP.predict_grad / gpc_predict_grad: gradients of the predictive mean and variance with respect to the query
inputs, against a NumPy restatement of the formulas on the oracle's posteriors, against central differences of the
GP's own predict, and against predict itself; batch and sharding invariance bit for bit."""

import os
import socket
import sys

import numpy as np
import pytest

from conftest import parse_core_name

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gp(model, D, dtype="f64"):
    from test_gpu_api import _gp as make

    return make(model, D, dtype)


def _counts(model, D):
    from oracle import gp_oracle as orc

    return orc.cov_count(model["kernel"], D), orc.noise_count(model["noise"]), orc.mean_count(model["mean"], D)


def _dk_dxstar(model, hyp, X, xs):
    """dK(X, xs)_ij / dxs_jl (N, M, D), written out per family; pairs at distance 0 contribute 0."""
    kernel, degree = model["kernel"], model["degree"]
    D = X.shape[1]
    iso = kernel.endswith("_iso")
    ell = np.exp(hyp[0]) * np.ones(D) if iso else np.exp(hyp[:D])
    sf2 = np.exp(2 * hyp[1 if iso else D])
    c = (np.sqrt(degree) if kernel.startswith("matern") else 1.0) / ell
    diff = (xs * c)[None, :, :] - (X * c)[:, None, :]  # xs*_jl - xs_il, scaled
    r2 = np.sum(diff**2, 2)
    with np.errstate(all="ignore"):
        if kernel.startswith("se"):
            F = sf2 * np.exp(-r2 / 2)
        elif kernel.startswith("matern"):
            t = np.sqrt(r2)
            df = {1: 1 / t, 3: np.ones_like(t), 5: (1 + t) / 3}[degree]
            F = sf2 * df * np.exp(-t)
        else:
            a = np.exp(hyp[D + 1])
            F = sf2 * (1 + r2 / (2 * a)) ** (-a - 1)
    F = np.where(r2 > 0, F, 0.0)
    return -F[:, :, None] * diff * c


def _numpy_grads(model, posts, X, xs, mu_sep, s2_sep, bounds=False):
    """Per-sample dmu, ds2 (M, D, S) from alpha and (K + Sigma)^-1 of the oracle's posteriors.  With ``bounds``: also
    the first-order sensitivity of each to a relative perturbation of the solve, per sample -- cond((K + Sigma)^-1) times
    max_jl |alpha| |dk_:jl| (mean) and 2 max_jl |Q_:j| |dk_:jl| (variance), 2-norms: a backward-stable solve of
    relative accuracy u changes the result by at most u times that (Cauchy-Schwarz on the perturbed alpha / Q)."""
    from oracle import gp_oracle as orc

    M, D = xs.shape
    cov_N, noise_N, mean_N = _counts(model, D)
    S = len(posts)
    dmu = np.zeros((M, D, S))
    ds2 = np.zeros((M, D, S))
    sens = np.zeros((2, S))
    for s, p in enumerate(posts):
        h = p.hyp
        Ks = orc.covariance(model["kernel"], h[:cov_N], X, xs, degree=model["degree"])
        dk = _dk_dxstar(model, h[:cov_N], X, xs)
        if p.L_chol:
            sW = p.sW[:, 0]
            Kinv = sW[:, None] * np.linalg.inv(p.L.T @ p.L) * sW[None, :]
        else:
            Kinv = -p.L
        Q = Kinv @ Ks
        dmu[:, :, s] = np.einsum("i,ijl->jl", p.alpha[:, 0], dk)
        ds2[:, :, s] = -2 * np.einsum("ij,ijl->jl", Q, dk)
        if model["mean"] == "negquad":
            hm = h[cov_N + noise_N:cov_N + noise_N + mean_N]
            dmu[:, :, s] += -(xs - hm[1:1 + D]) / np.exp(2 * hm[1 + D:])
        ds2[s2_sep[:, s] <= 0, :, s] = 0
        if bounds:
            dkn = np.sqrt(np.sum(dk**2, 0))  # (M, D)
            cond = np.linalg.cond(Kinv)
            sens[0, s] = cond * np.linalg.norm(p.alpha) * dkn.max()
            sens[1, s] = cond * 2 * (np.sqrt(np.sum(Q**2, 0))[:, None] * dkn).max()
    return (dmu, ds2, sens) if bounds else (dmu, ds2)


def _mix(mu_sep, dmu, ds2):
    S = mu_sep.shape[1]
    if S == 1:
        return dmu[:, :, 0], ds2[:, :, 0]
    dev = mu_sep - mu_sep.mean(1, keepdims=True)
    return dmu.mean(2), ds2.mean(2) + 2 * np.einsum("ms,mds->md", dev, dmu) / (S - 1)


def _close(a, b, rtol):
    scale = max(np.abs(b).max(), 1e-300)
    return np.abs(a - b).max() <= rtol * scale


# (dtype, rtol of the well-conditioned cases, u = relative accuracy of a solve in that arithmetic with some margin:
# ~45 ulp of fp64, ~16 ulp of fp32)
@pytest.mark.parametrize("dtype,rtol,u", [("f64", 1e-8, 1e-14), ("f32", 1e-3, 1e-6)])
def test_analytic_parity_with_numpy_formulas(core_golden, dtype, rtol, u):
    """Every golden model, both L_chol kinds: the `plain` cases (all L_chol = 1, well conditioned) to rtol of the
    largest entry; the lownoise / tiny_s2 / jitter cases (L_chol = 0 except jitter_high) to rtol plus u times the
    solve's sensitivity (_numpy_grads), the oracle evaluated at the device's jitter level.  A case whose sensitivity
    bound exceeds 1 % of the largest entry carries no information and is not compared: in fp64 the lownoise g014 and
    g020 (L_chol = 0) are compared, g007 / g008 and the jitter cases (cond 1e9 ... 1e18) are not; in fp32 none of them
    (test_low_noise_and_mixed_batches covers L_chol = 0 in fp32 on a well-conditioned problem)."""
    from oracle import gp_oracle as orc

    g = core_golden
    done, lchol0 = 0, 0
    for name in g["names"]:
        tag, model, N, D, flavour = parse_core_name(name)
        X, y, hyp = g[tag + "_X"], g[tag + "_y"], g[tag + "_hyp"]
        s2 = g[tag + "_s2"] if tag + "_s2" in g.files else None
        xs = g[tag + "_xs"]
        gp = _gp(model, D, dtype)
        try:
            gp.update(X_new=X, y_new=y, s2_new=s2, hyp=hyp)
        except np.linalg.LinAlgError:
            if dtype == "f32" and flavour != "plain":  # fp32 factorization of a matrix of cond 1e7 ... 1e18
                continue
            raise
        mult = [p.sn2_mult for p in gp.posteriors]
        try:
            posts = orc.posteriors(model, hyp, X, y, s2, force_mult=mult)
        except np.linalg.LinAlgError:  # LAPACK fails at the device's jitter level: a jitter case of cond ~1e17
            if flavour != "plain":
                continue
            raise
        assert [p.L_chol for p in posts] == [p.L_chol for p in gp.posteriors], name
        mu_sep, s2_sep = orc.predict(model, posts, X, y, xs, separate_samples=True)
        rdmu, rds2, sens = _numpy_grads(model, posts, X, xs, mu_sep, s2_sep, bounds=True)
        if flavour != "plain":
            if np.any(u * sens[0] > 1e-2 * np.abs(rdmu).max()) or np.any(u * sens[1] > 1e-2 * np.abs(rds2).max()):
                continue
        else:
            sens[:] = 0
        mu, v, dmu, ds2 = gp.predict_grad(xs, separate_samples=True)
        assert dmu.shape == (xs.shape[0], D, hyp.shape[0]) and ds2.shape == dmu.shape
        for s in range(hyp.shape[0]):
            e_m = np.abs(dmu[:, :, s] - rdmu[:, :, s]).max()
            e_v = np.abs(ds2[:, :, s] - rds2[:, :, s]).max()
            assert e_m <= rtol * np.abs(rdmu[:, :, s]).max() + u * sens[0, s], (name, s, "dmu", e_m)
            assert e_v <= rtol * np.abs(rds2[:, :, s]).max() + u * sens[1, s], (name, s, "ds2", e_v)
        _, _, mdmu, mds2 = gp.predict_grad(xs)
        emu, eds2 = _mix(mu_sep, rdmu, rds2)
        assert mdmu.shape == (xs.shape[0], D)
        slack = u * sens.max(1) * 2  # the spread term: dmu_s times deviations of the means
        assert np.abs(mdmu - emu).max() <= rtol * np.abs(emu).max() + u * sens[0].max(), name
        assert np.abs(mds2 - eds2).max() <= rtol * np.abs(eds2).max() + slack[1] + slack[0] * np.abs(mu_sep).max(), name
        done += 1
        lchol0 += not gp.posteriors[0].L_chol
    assert done >= 25
    assert lchol0 >= (2 if dtype == "f64" else 0), lchol0


def _problem(kernel, degree, mean="const", N=200, D=3, S=3, seed=1):
    import gpyreg_amd as gpr

    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (N, D))
    y = np.sin(X.sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1))
    model = dict(kernel=kernel, degree=degree, mean=mean, noise=(1, 0, 0))
    cov_N, noise_N, mean_N = _counts(model, D)
    hyp = np.zeros((S, cov_N + noise_N + mean_N))
    hyp[:, :D if not kernel.endswith("_iso") else 1] = np.log(1.2)
    hyp[:, cov_N] = np.log(0.1)
    if mean == "negquad":
        hyp[:, cov_N + noise_N + 1 + D:] = np.log(3.0)
    hyp += 0.05 * rng.standard_normal(hyp.shape)
    gp = _gp(model, D)
    gp.update(X_new=X, y_new=y, hyp=hyp)
    del gpr
    return gp, model, X, y, hyp


@pytest.mark.parametrize("kernel,degree,mean", [("se", 0, "negquad"), ("matern", 5, "const"), ("matern", 3, "zero"),
                                                ("rq", 0, "const"), ("matern_iso", 5, "negquad")])
def test_central_differences_of_predict(kernel, degree, mean):
    gp, model, X, y, hyp = _problem(kernel, degree, mean)
    rng = np.random.default_rng(7)
    xs = np.concatenate([rng.uniform(-2, 2, (12, X.shape[1])), X[:3]])  # the last three ON training points
    mu, v, dmu, ds2 = gp.predict_grad(xs, separate_samples=True)
    mmu, mv, mdmu, mds2 = gp.predict_grad(xs)
    assert np.all(np.isfinite(dmu)) and np.all(np.isfinite(ds2))
    h = 1e-5 * (X.max(0) - X.min(0))
    for l in range(X.shape[1]):
        e = np.zeros(X.shape[1])
        e[l] = h[l]
        mp, vp = gp.predict(xs + e, separate_samples=True)
        mm, vm = gp.predict(xs - e, separate_samples=True)
        assert _close(dmu[:, l, :], (mp - mm) / (2 * h[l]), 1e-5), ("dmu", l)
        assert _close(ds2[:, l, :], (vp - vm) / (2 * h[l]), 1e-5), ("ds2", l)
        mp, vp = gp.predict(xs + e)
        mm, vm = gp.predict(xs - e)
        assert _close(mdmu[:, l:l + 1], (mp - mm) / (2 * h[l]), 1e-5), ("mix dmu", l)
        assert _close(mds2[:, l:l + 1], (vp - vm) / (2 * h[l]), 1e-5), ("mix ds2", l)


def _lownoise_problem(sn2s, N=40, D=3, seed=11, dtype="f64"):
    """Matern 5 on well-spread points, one noise variance per hyperparameter row: rows below 1e-6 give L_chol = 0
    posteriors (Posterior.L = -(K + Sigma)^-1), the others L_chol = 1; cond(K + Sigma) stays near 1e2 either way."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-3, 3, (N, D))
    y = np.sin(X.sum(1, keepdims=True))
    model = dict(kernel="matern", degree=5, mean="const", noise=(1, 0, 0))
    hyp = np.array([np.r_[0.05 * rng.standard_normal(D), 0.0, 0.5 * np.log(v), 0.1] for v in sn2s])
    gp = _gp(model, D, dtype)
    gp.update(X_new=X, y_new=y, hyp=hyp)
    assert [p.L_chol for p in gp.posteriors] == [v >= 1e-6 for v in sn2s]
    return gp, model, X, y, hyp


@pytest.mark.parametrize("dtype,rtol", [("f64", 1e-8), ("f32", 1e-3)])
@pytest.mark.parametrize("sn2s", [(1e-7, 1e-8), (1e-2, 1e-7, 1e-7, 1e-2, 1e-7, 1e-2)])
def test_low_noise_and_mixed_batches(sn2s, dtype, rtol):
    """L_chol = 0 samples (Q = -(A K*) from the product predict forms) alone, and interleaved with L_chol = 1 samples so
    that one call runs several launches with nonzero sample offsets: NumPy parity, central differences of predict, and
    each sample bitwise equal to its own single-sample GP (central differences in fp64 only)."""
    from oracle import gp_oracle as orc

    gp, model, X, y, hyp = _lownoise_problem(sn2s, dtype=dtype)
    xs = np.random.default_rng(12).uniform(-3, 3, (50, X.shape[1]))
    mu, v, dmu, ds2 = gp.predict_grad(xs, separate_samples=True)
    posts = orc.posteriors(model, hyp, X, y, None)
    mu_sep, s2_sep = orc.predict(model, posts, X, y, xs, separate_samples=True)
    rdmu, rds2 = _numpy_grads(model, posts, X, xs, mu_sep, s2_sep)
    for s in range(len(sn2s)):
        assert _close(dmu[:, :, s], rdmu[:, :, s], rtol) and _close(ds2[:, :, s], rds2[:, :, s], rtol), s
    h = 1e-5 * (X.max(0) - X.min(0))
    _, _, mdmu, mds2 = gp.predict_grad(xs)
    for l in range(X.shape[1] if dtype == "f64" else 0):
        e = np.zeros(X.shape[1])
        e[l] = h[l]
        mp, vp = gp.predict(xs + e, separate_samples=True)
        mm, vm = gp.predict(xs - e, separate_samples=True)
        assert _close(dmu[:, l, :], (mp - mm) / (2 * h[l]), 1e-5), ("dmu", l)
        assert _close(ds2[:, l, :], (vp - vm) / (2 * h[l]), 1e-5), ("ds2", l)
        mp, vp = gp.predict(xs + e)
        mm, vm = gp.predict(xs - e)
        assert _close(mdmu[:, l:l + 1], (mp - mm) / (2 * h[l]), 1e-5) and _close(mds2[:, l:l + 1], (vp - vm) / (2 * h[l]), 1e-5)
    for s in range(len(sn2s)):
        one = _gp(model, X.shape[1], dtype)
        one.update(X_new=X, y_new=y, hyp=hyp[s:s + 1])
        _, _, d1, v1 = one.predict_grad(xs, separate_samples=True)
        assert np.array_equal(d1[:, :, 0], dmu[:, :, s]) and np.array_equal(v1[:, :, 0], ds2[:, :, s]), s


def test_clamp_zeroes_the_variance_gradient(monkeypatch):
    """Where predict's clamp s2 = max(s2, 0) holds the variance at 0 (s2 <= 0 before it) the variance gradient is 0, per
    sample and in the mixture; elsewhere it is the device's.  The device results are shifted below 0 on chosen rows."""
    gp, model, X, y, hyp = _lownoise_problem((1e-2, 1e-7, 1e-2))
    xs = np.random.default_rng(13).uniform(-3, 3, (20, X.shape[1]))
    h = gp._post_handle
    real = h.predict_grad
    ref = real(xs)

    def shifted(x):
        fmu, fs2, dfmu, dfs2 = real(x)
        fs2 = fs2.copy()
        fs2[0:5, 0] = -1e-3
        fs2[5, 1] = 0.0
        fs2[6:9, :] = -1e-9
        return fmu, fs2, dfmu, dfs2

    monkeypatch.setattr(h, "predict_grad", shifted)
    mu, v, dmu, ds2 = gp.predict_grad(xs, separate_samples=True)
    held = np.zeros((20, 3), bool)
    held[0:5, 0] = held[5, 1] = True
    held[6:9, :] = True
    assert np.all(v[held] == 0)
    assert np.all(ds2.transpose(0, 2, 1)[held] == 0)
    assert np.array_equal(ds2.transpose(0, 2, 1)[~held], ref[3].transpose(0, 2, 1)[~held])
    _, _, mdmu, mds2 = gp.predict_grad(xs)
    emu, eds2 = _mix(mu, dmu, ds2)
    assert np.allclose(mds2, eds2, rtol=1e-13, atol=0) and np.allclose(mdmu, emu, rtol=1e-13, atol=0)


def test_chunked_samples_bitwise(monkeypatch):
    """A memory budget that holds only a few samples of the gradient scratch per chunk (non-resident constants, several
    chunks, runs split at chunk borders): the same bits as one chunk."""
    gp, model, X, y, hyp = _lownoise_problem((1e-2, 1e-7) * 5, N=300, D=4)
    xs = np.random.default_rng(14).uniform(-3, 3, (300, 4))
    whole = gp.predict_grad(xs, separate_samples=True)
    monkeypatch.setenv("GPC_MEM_BUDGET_MB", "16")  # ~3.7 MB of scratch per sample at npad = mpad = 384: 3 per chunk
    chunked = gp.predict_grad(xs, separate_samples=True)
    monkeypatch.delenv("GPC_MEM_BUDGET_MB")
    for a, b in zip(whole, chunked):
        assert np.array_equal(a, b)
    # ... and the chunk is the one that the scratch's closed form gives
    from gpyreg_amd import _lib
    from scratch_sizes import planned_chunk, rhs_per, rhs_shared

    want = planned_chunk(10, 16, rhs_per(384, 384, False, 8, 4, "cross", True, grad=True), rhs_shared(300, 300, 4, 10))
    assert want == 3 and _lib.context(gp.device).get_option("last_chunk") == want


def test_matern1_on_training_points_is_finite_and_the_convention():
    from oracle import gp_oracle as orc

    gp, model, X, y, hyp = _problem("matern", 1, "const")
    xs = np.concatenate([X[:5], X[5:8] + 0.3])
    mu, v, dmu, ds2 = gp.predict_grad(xs, separate_samples=True)
    assert np.all(np.isfinite(dmu)) and np.all(np.isfinite(ds2))
    posts = orc.posteriors(model, hyp, X, y, None)
    mu_sep, s2_sep = orc.predict(model, posts, X, y, xs, separate_samples=True)
    rdmu, rds2 = _numpy_grads(model, posts, X, xs, mu_sep, s2_sep)
    assert _close(dmu, rdmu, 1e-8) and _close(ds2, rds2, 1e-8)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mean_and_variance_match_predict(dtype):
    gp, model, X, y, hyp = _problem("matern", 5, "negquad")
    if dtype == "f32":
        gp = _gp(model, X.shape[1], "f32")
        gp.update(X_new=X, y_new=y, hyp=hyp)
    xs = np.random.default_rng(3).uniform(-2.5, 2.5, (300, X.shape[1]))
    for kw in (dict(separate_samples=True), dict(), dict(add_noise=True), dict(add_noise=True, separate_samples=True)):
        mu, v = gp.predict(xs, **kw)
        gmu, gv, _, _ = gp.predict_grad(xs, **kw)
        assert gmu.shape == mu.shape and gv.shape == v.shape
        assert np.abs(gmu - mu).max() <= 1e-12 * np.abs(mu).max(), kw
        assert np.abs(gv - v).max() <= 1e-12 * np.abs(v).max(), kw


@pytest.mark.parametrize("kernel,degree", [("matern", 5), ("rq", 0)])
def test_batch_equals_single_and_query_subsets_bitwise(kernel, degree):
    gp, model, X, y, hyp = _problem(kernel, degree, "const", N=300, D=4, S=16, seed=4)
    xs = np.random.default_rng(5).uniform(-2, 2, (300, 4))
    _, _, dmu, ds2 = gp.predict_grad(xs, separate_samples=True)
    for s in (0, 7, 15):
        one = _gp(model, 4)
        one.update(X_new=X, y_new=y, hyp=hyp[s:s + 1])
        _, _, d1, v1 = one.predict_grad(xs, separate_samples=True)
        assert np.array_equal(d1[:, :, 0], dmu[:, :, s]) and np.array_equal(v1[:, :, 0], ds2[:, :, s]), s
    for lo, hi in ((0, 70), (130, 300)):  # other query counts: other padded widths and tile counts
        _, _, d2, v2 = gp.predict_grad(xs[lo:hi], separate_samples=True)
        assert np.array_equal(d2, dmu[lo:hi]) and np.array_equal(v2, ds2[lo:hi]), (lo, hi)


def test_no_data_gp_is_the_mean_function():
    import gpyreg_amd as gpr

    D = 2
    gp = gpr.GP(D, gpr.covariance_functions.SquaredExponential(), gpr.mean_functions.NegativeQuadratic(),
                gpr.noise_functions.GaussianNoise(constant_add=True))
    hyp = np.array([[0.1, -0.2, 0.0, np.log(0.1), 1.0, 0.3, -0.4, 0.2, 0.5]])
    gp.update(hyp=hyp)
    xs = np.array([[0.5, 1.0], [-1.0, 2.0]])
    mu, v, dmu, ds2 = gp.predict_grad(xs)
    emu, ev = gp.predict(xs)
    assert np.array_equal(mu, emu) and np.array_equal(v, ev)
    assert np.allclose(dmu, -(xs - hyp[0, 5:7]) / np.exp(2 * hyp[0, 7:9]), rtol=1e-14) and np.all(ds2 == 0)


def test_refusals_name_the_object():
    import gpyreg_amd as gpr
    from test_gpu_user_kernel import PySquaredExponential

    rng = np.random.default_rng(0)
    X = rng.uniform(-1, 1, (40, 2))
    y = np.sin(X[:, :1])
    hyp = np.array([[0.0, 0.0, 0.0, np.log(0.1), 0.0]])

    class MyMean(gpr.mean_functions.ConstantMean):
        pass

    class MyNoise(gpr.noise_functions.GaussianNoise):
        pass

    gp = gpr.GP(2, PySquaredExponential(), gpr.mean_functions.ConstantMean(),
                gpr.noise_functions.GaussianNoise(constant_add=True))
    gp.update(X_new=X, y_new=y, hyp=hyp)
    with pytest.raises(NotImplementedError, match="PySquaredExponential"):
        gp.predict_grad(X[:3])
    gp = gpr.GP(2, gpr.covariance_functions.SquaredExponential(), MyMean(),
                gpr.noise_functions.GaussianNoise(constant_add=True))
    gp.update(X_new=X, y_new=y, hyp=hyp)
    with pytest.raises(NotImplementedError, match="MyMean"):
        gp.predict_grad(X[:3])
    gp = gpr.GP(2, gpr.covariance_functions.SquaredExponential(), gpr.mean_functions.ConstantMean(),
                MyNoise(constant_add=True))
    gp.update(X_new=X, y_new=y, hyp=hyp)
    gp.predict_grad(X[:3])  # without add_noise the noise object is not needed
    with pytest.raises(NotImplementedError, match="MyNoise"):
        gp.predict_grad(X[:3], add_noise=True)


# ---- sharding: the pattern of test_gpu_sharding.py::test_sharded_gp_equals_unsharded_bitwise_two_ranks_one_gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      GPYREG_AMD_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist

    import bench

    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    try:
        bench.CONFIGS[3] = dict(bench.CONFIGS[3], N=700)
        for S in (1, 5, 16):
            X, y, hyp = bench.synthetic_problem(3, S)
            xs = X[:40] + 0.05
            ref = bench.make_gp(3, "f64")
            ref.shard = False
            ref.update(X_new=X, y_new=y, hyp=hyp)
            gp = bench.make_gp(3, "f64")
            gp.update(X_new=X, y_new=y, hyp=hyp)
            ok = {}
            for kw in (dict(separate_samples=True), dict(), dict(add_noise=True)):
                a = ref.predict_grad(xs, **kw)
                b = gp.predict_grad(xs, **kw)
                ok[str(kw)] = all(np.array_equal(u, v) for u, v in zip(a, b))
            out[S] = ok
    except Exception as e:  # noqa: BLE001 - reported to the parent
        out["exception"] = repr(e)
    finally:
        dist.destroy_process_group()
    q.put((rank, out))


def test_sharded_predict_grad_equals_unsharded_bitwise_two_ranks_one_gpu():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for rank in (0, 1):
        r = res[rank]
        assert "exception" not in r, r.get("exception")
        for S in (1, 5, 16):
            assert all(r[S].values()), (rank, S, r[S])
