"""GP.condition_on_gradients / gpc_posterior_batch_gobs: conditioning on values AND gradients on the device.

The two new kernels entry by entry through their hooks (gpc_debug_gobs_cov, gpc_debug_gobs_cross) against the
extended-precision reference of tests/gradobs_ref.py, then the pipeline: parity with the NumPy restatement
(gpyreg_amd._gradobs), the same bits as the caller-provided-K pipeline fed with the device's own matrix, the identity
with GP.gradient_posterior, properties (no variance increase, the large-noise limit, better held-out predictions),
invariance, the GP left untouched, refusals and errors, and nll_batch_grad_obs."""

import numpy as np
import pytest

import gradobs_ref as gr
import test_cov_functors_cpu as cf
from test_gpu_api import _gp

pytestmark = pytest.mark.gpu
KID = {"se": 0, "matern": 1, "rq": 2, "se_iso": 3, "matern_iso": 4}
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def ctx():
    from gpyreg_amd import _lib

    return _lib.context(0)


def _close(a, b, rtol):
    """The project's scale-relative metric: |a - b| / max(|b|, |b|_inf) <= rtol everywhere."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return a.shape == b.shape and np.all(np.isfinite(a)) and np.abs(a - b).max() <= rtol * max(np.abs(b).max(), 1e-300)


# ---- the two kernels, per entry ------------------------------------------------------------------------------------


@pytest.mark.parametrize("N,Ng,D", [(70, 37, 1), (70, 37, 3), (129, 65, 3), (20, 64, 33)])
@pytest.mark.parametrize("name,alpha", gr.FAMILIES)
def test_kernels_per_entry(ctx, name, alpha, N, Ng, D):
    """gobs_cov_kernel and gobs_cross_tile_kernel against np.longdouble on the same fp64 scaled coordinates, on the
    functor tests' ladder and shifts, within the per-entry bounds of tests/gradobs_ref.py.  Also: the joint matrix is
    symmetric to the bit; a duplicate pair gives exactly 0 for value / gradient and c_a^2 F0 delta_ab for gradient /
    gradient (exactly 0 off the diagonal; on it the entry the point has with itself, to the bit, which is c_a^2 F0
    within the three roundings of the product and one of F0); the operand's padding is exactly 0; its fused column
    sums equal the sums of the stored values within 64 eps sum|terms|."""
    M = 70
    rng = np.random.default_rng(N + D)
    for shift in cf.SHIFTS:
        case = gr.setup(name, alpha, N, Ng, D, shift, M=M)
        kind, degree, hyp, X, Xg, Xq = (case[k] for k in ("kind", "degree", "hyp", "X", "Xg", "Xq"))
        n = N + Ng * D
        K = ctx.debug_gobs_cov(kind, degree, hyp, X, Xg)
        want, bound = gr.joint_cov_ld(case)
        r = gr.worst(K, want, bound)
        print(f"{name} {alpha} ({N},{Ng},{D}) shift {shift:g}: cov worst error / bound {r:.3f}")
        assert r <= 1.0, (name, alpha, shift, r)
        assert np.array_equal(K, K.T), (name, shift, "the joint matrix is not symmetric to the bit")
        # duplicates: Xg[:half] repeat X[:half]; Xg[Ng - 1] repeats Xg[0]
        idx = np.arange(N, n).reshape(D, Ng).T  # idx[g, l] = N + l Ng + g
        half = min(Ng // 2, N)
        for g in range(half):
            assert np.all(K[idx[g], g] == 0) and np.all(K[g, idx[g]] == 0), (name, shift, g)
        if Ng > 1:
            blk = K[np.ix_(idx[Ng - 1], idx[0])]
            own = K[np.ix_(idx[0], idx[0])]
            assert np.array_equal(blk, own) and np.all(blk[~np.eye(D, dtype=bool)] == 0), (name, shift)
            f0 = np.float64(gr.with_g(kind, degree, cf.reference(kind, degree, case["xsg"][:1], case["xsg"][:1],
                                                                 case["sf2"], case["rqa"]), case["sf2"], case["rqa"])["F"][0, 0])
            c = case["c"]
            assert np.all(np.abs(np.diag(blk) - c * c * f0) <= 4 * EPS * c * c * f0), (name, shift)
        alpha_v = rng.standard_normal(n)
        B, panel, col = ctx.debug_gobs_cross(kind, degree, hyp, X, Xg, Xq, alpha_v)
        wantb, boundb = gr.joint_cross_ld(case)
        rb = gr.worst(B, wantb, boundb)
        print(f"{name} {alpha} ({N},{Ng},{D}) shift {shift:g}: cross worst error / bound {rb:.3f}")
        assert rb <= 1.0, (name, alpha, shift, rb)
        assert panel.shape[0] % 128 == 0 and panel.shape[1] % 128 == 0
        assert np.all(panel[n:] == 0) and np.all(panel[:, M:] == 0), (name, shift, "padding is not exactly 0")
        terms = B * alpha_v[:, None]
        assert np.all(np.abs(col - terms.sum(0)) <= 64 * EPS * np.abs(terms).sum(0)), (name, shift)
        # a query ON a training row: that row's value column of the joint matrix, to the bit
        assert np.array_equal(Xq[0], X[7]) and np.array_equal(B[:, 0], K[:, 7]), (name, shift)


# ---- the pipeline against the NumPy restatement --------------------------------------------------------------------


def _problem(N, Ng, D, kernel, degree, mean, S=3, seed=0, dtype="f64", sn_val=0.1, repeat=0, sn_rows=None):
    """A GP with S resident samples on y = sin(sum x / sqrt(D)), and gradient data dy = cos(.) / sqrt(D) + noise at Ng
    points, the first ``repeat`` of them rows of X."""
    from oracle import gp_oracle as orc

    rng = np.random.default_rng(1000 * N + 10 * Ng + D + seed)
    X, Xg = rng.uniform(-2, 2, (N, D)), rng.uniform(-2, 2, (Ng, D))
    Xg[:repeat] = X[:repeat]
    f = lambda Z: np.sin(Z.sum(1, keepdims=True) / np.sqrt(D))
    y = f(X) + 0.05 * rng.standard_normal((N, 1))
    dy = np.cos(Xg.sum(1, keepdims=True) / np.sqrt(D)) / np.sqrt(D) * np.ones((1, D)) + 0.05 * rng.standard_normal((Ng, D))
    model = dict(kernel=kernel, degree=degree, mean=mean, noise=(1, 0, 0))
    cov_N, noise_N, mean_N = orc.cov_count(kernel, D), orc.noise_count(model["noise"]), orc.mean_count(mean, D)
    hyp = np.zeros((S, cov_N + noise_N + mean_N))
    hyp[:, :1 if kernel.endswith("_iso") else D] = np.log(1.2 * np.sqrt(D))
    if kernel == "rq":
        hyp[:, D + 1] = np.log(2.0)
    hyp[:, cov_N] = np.log(sn_val)
    if mean == "negquad":
        hyp[:, cov_N + noise_N + 1 + D:] = np.log(3.0)
    hyp += 0.05 * rng.standard_normal(hyp.shape)
    if sn_rows is not None:
        hyp[:, cov_N] = np.log(sn_rows)
    gp = _gp(model, D, dtype)
    gp.update(X_new=X, y_new=y, hyp=hyp)
    return gp, model, X, y, Xg, dy, hyp, (cov_N, noise_N, mean_N)


def _reference(gp, model, X, y, Xg, dy, hyp, counts, s2g):
    """_gradobs.posterior of every sample: the joint rows are put together HERE, not by the code under test."""
    from gpyreg_amd import _gradobs as go
    from gpyreg_amd.gaussian_process import _mean_grad_x

    cov_N, noise_N, mean_N = counts
    N, D = X.shape
    Ng = Xg.shape[0]
    kid, degree = KID[model["kernel"]], model["degree"]
    s2 = np.broadcast_to(np.asarray(s2g, dtype=float)[:, None] if np.ndim(s2g) == 1 else np.asarray(s2g, dtype=float), (Ng, D))
    posts = []
    for h in hyp:
        hm = h[cov_N + noise_N:]
        m = go.to_joint(np.reshape(gp.mean.compute(hm, X), (-1,)), _mean_grad_x(gp.mean, hm, Xg))
        sn2 = go.to_joint(np.full(N, np.exp(2 * h[cov_N])), s2)
        posts.append(go.posterior(kid, degree, h[:cov_N], X, Xg, go.to_joint(y, dy), m, sn2))
    return posts


PIPELINE = [
    # N, Ng, D, kernel, degree, mean, s2_grad form, dtype, repeated rows
    (70, 37, 3, "matern", 5, "const", "scalar", "f64", 18),   # half of X_g repeats rows of X
    (130, 65, 2, "se", 0, "negquad", "vector", "f64", 0),     # three and two point tiles, n_pad = 384
    (20, 64, 1, "rq", 0, "zero", "matrix", "f64", 0),
    (50, 9, 33, "matern", 3, "const", "vector", "f64", 0),    # more than one staged chunk of dimensions
    (1, 1, 2, "se", 0, "zero", "scalar", "f64", 0),
    (70, 37, 3, "se", 0, "const", "matrix", "f32", 18),
    (130, 65, 2, "matern", 5, "negquad", "scalar", "f32", 0),
]


def _s2_grad(form, Ng, D, rng):
    if form == "scalar":
        return 0.01
    if form == "vector":
        return 0.01 * rng.uniform(0.5, 2.0, Ng)
    return 0.01 * rng.uniform(0.5, 2.0, (Ng, D))


def _check_against_reference(gp, cp, posts, model, X, Xg, hyp, counts, rtol, lchol):
    from gpyreg_amd import _gradobs as go

    cov_N, noise_N, _ = counts
    N, D = X.shape
    Ng = Xg.shape[0]
    kid, degree = KID[model["kernel"]], model["degree"]
    S = len(posts)
    xs = np.random.default_rng(9).uniform(-2, 2, (70, D))
    xs[:2] = X[:2] if N >= 2 else xs[:2]
    xs[2] = Xg[0]
    mu, s2 = cp.predict(xs, separate_samples=True)
    assert mu.shape == (70, S) and s2.shape == (70, S)
    assert list(cp.L_chol) == lchol and np.all(cp.sn2_mult == 1)
    assert _close(cp.nlZ, [p["nlZ"] for p in posts], rtol), (cp.nlZ, [p["nlZ"] for p in posts])
    for s, p in enumerate(posts):
        assert p["L_chol"] == lchol[s] and p["sn2_mult"] == 1
        av, ag = cp.alpha[s]
        assert av.shape == (N,) and ag.shape == (Ng, D)
        assert _close(go.to_joint(av, ag), p["alpha"], rtol), (s, "alpha")
        _, sW, L = cp._handle.fetch(s)
        assert _close(L, p["L"].T if lchol[s] else p["L"], rtol), (s, "L")
        assert np.allclose(sW, p["sW"], rtol=1e-14, atol=0), (s, "sW")  # (inf on both sides when the joint minimum is 0)
        rmu, rs2 = go.predict(kid, degree, hyp[s, :cov_N], X, Xg, xs, p)
        rmu = rmu + np.reshape(gp.mean.compute(hyp[s, cov_N + noise_N:], xs), (-1,))
        assert _close(mu[:, s], rmu, rtol), (s, "mean", np.abs(mu[:, s] - rmu).max())
        assert _close(s2[:, s], np.maximum(rs2, 0), rtol), (s, "variance", np.abs(s2[:, s] - rs2).max())


@pytest.mark.parametrize("N,Ng,D,kernel,degree,mean,form,dtype,repeat", PIPELINE)
def test_pipeline_against_numpy(N, Ng, D, kernel, degree, mean, form, dtype, repeat):
    """alpha, nlZ, L (gpc_post_fetch), the predictive mean and variance at 70 queries, S = 3 samples, against
    gpyreg_amd._gradobs: the project's parity bar, 1e-8 in the scale-relative metric in fp64, 1e-3 for fp32 posteriors.
    Value noise 0.1^2 and gradient noise ~ 0.1^2."""
    gp, model, X, y, Xg, dy, hyp, counts = _problem(N, Ng, D, kernel, degree, mean, dtype=dtype, repeat=repeat)
    s2g = _s2_grad(form, Ng, D, np.random.default_rng(4))
    posts = _reference(gp, model, X, y, Xg, dy, hyp, counts, s2g)
    with gp.condition_on_gradients(Xg, dy, s2g) as cp:
        _check_against_reference(gp, cp, posts, model, X, Xg, hyp, counts, 1e-8 if dtype == "f64" else 1e-3, [True] * 3)
    with pytest.raises(ValueError, match="closed"):
        cp.predict(X[:1])


def test_pipeline_low_noise_and_mixed_batch():
    """s2_grad = 0 at distinct points: min of the joint noise is 0, the reference's low-noise branch (L = -inv) by its
    own rule; and a batch whose samples take different branches (value noise 0.1^2 | 1e-7 | 0.1^2 with gradient noise
    0.1^2: the middle sample's joint minimum is below 1e-6)."""
    gp, model, X, y, Xg, dy, hyp, counts = _problem(40, 12, 3, "matern", 5, "const", seed=3)
    posts = _reference(gp, model, X, y, Xg, dy, hyp, counts, 0.0)
    with gp.condition_on_gradients(Xg, dy, 0.0) as cp:
        _check_against_reference(gp, cp, posts, model, X, Xg, hyp, counts, 1e-8, [False] * 3)
    gp, model, X, y, Xg, dy, hyp, counts = _problem(40, 12, 3, "se", 0, "const", seed=4,
                                                    sn_rows=np.array([0.1, np.sqrt(1e-7), 0.1]))
    posts = _reference(gp, model, X, y, Xg, dy, hyp, counts, 0.01)
    with gp.condition_on_gradients(Xg, dy, 0.01) as cp:
        _check_against_reference(gp, cp, posts, model, X, Xg, hyp, counts, 1e-8, [True, False, True])


# ---- nothing downstream was forked ---------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [cf.F64, cf.F32])
def test_same_bits_as_the_caller_provided_K_pipeline(ctx, dtype):
    """The posterior built from the device's joint matrix equals BIT FOR BIT (alpha, L, sn2_mult; nlZ of the
    likelihood-only evaluation) the one posterior_batch_K / nll_batch_K build from the matrix fetched through
    debug_gobs_cov with the same joint targets and noise: both go through the same staging buffer and load_K_kernel."""
    from gpyreg_amd import _gradobs as go

    rng = np.random.default_rng(8)
    N, Ng, D, S = 70, 37, 3, 3
    X, Xg = rng.uniform(-2, 2, (N, D)), rng.uniform(-2, 2, (Ng, D))
    y, dy = np.sin(X.sum(1)), rng.standard_normal((Ng, D))
    n = N + Ng * D
    hyp_cov = np.log(1.5) + 0.1 * rng.standard_normal((S, D + 1))
    m = 0.1 * rng.standard_normal((S, n))
    sn2 = 0.01 * rng.uniform(0.5, 2, (S, n))
    sn2[1, 5] = 0.0  # a low-noise sample in the middle
    kid, degree = KID["matern"], 5
    ctx.set_data_gobs(X, y, Xg, dy)
    h1, nlz_post, mult1, lchol1, info1 = ctx.posterior_batch_gobs(kid, degree, dtype, hyp_cov, m, sn2)
    nlz1, mult1n, lchol1n, info1n = ctx.nll_batch_gobs(kid, degree, dtype, hyp_cov, m, sn2)
    K = np.stack([ctx.debug_gobs_cov(kid, degree, h, X, Xg) for h in hyp_cov])
    ctx.set_data(np.zeros((n, D)), go.to_joint(y, dy))
    h2, mult2, lchol2, info2 = ctx.posterior_batch_K(dtype, K, m, sn2, True)
    nlz2, _, mult2n, lchol2n, info2n = ctx.nll_batch_K(dtype, K, None, 0, m, sn2, True)
    assert np.all(info1 == 0) and np.all(info2 == 0) and list(lchol1) == [True, False, True]
    assert np.array_equal(mult1, mult2) and np.array_equal(lchol1, lchol2)
    assert np.array_equal(nlz1, nlz2) and np.array_equal(mult1n, mult2n)
    assert _close(nlz_post, nlz1, 1e-8 if dtype == cf.F64 else 1e-3)  # (the pipeline with the inverse: the parity bar)
    for s in range(S):
        a1, w1, L1 = h1.fetch(s)
        a2, w2, L2 = h2.fetch(s)
        assert np.array_equal(a1, a2) and np.array_equal(w1, w2) and np.array_equal(L1, L2), s
    h1.free()
    h2.free()


def test_identity_with_gradient_posterior():
    """Ng = 1 and x* = x_g with the device on both sides: conditioning gp.gradient_posterior's joint Gaussian of
    (f, grad f) at x_g on the observed gradient equals condition_on_gradients(...).predict(x_g), 1e-8 relative."""
    for kernel, degree, mean in [("matern", 5, "const"), ("se", 0, "negquad"), ("rq", 0, "zero")]:
        gp, model, X, y, Xg, dy, hyp, counts = _problem(60, 1, 3, kernel, degree, mean, seed=6)
        mean_j, cov_j = gp.gradient_posterior(Xg, with_value=True, separate_samples=True)
        s2g = 0.02
        with gp.condition_on_gradients(Xg, dy, s2g) as cp:
            mu, s2 = cp.predict(Xg, separate_samples=True)
        for s in range(hyp.shape[0]):
            m, C = mean_j[0, :, s], cov_j[0, :, :, s]
            Sg = C[1:, 1:] + s2g * np.eye(3)
            want_mu = m[0] + C[0, 1:] @ np.linalg.solve(Sg, dy[0] - m[1:])
            want_s2 = C[0, 0] - C[0, 1:] @ np.linalg.solve(Sg, C[1:, 0])
            assert abs(mu[0, s] - want_mu) <= 1e-8 * max(abs(want_mu), np.abs(y).max()), (kernel, s, mu[0, s], want_mu)
            assert abs(s2[0, s] - want_s2) <= 1e-8 * np.exp(2 * hyp[s, counts[0] - (2 if kernel == "rq" else 1)]), (kernel, s)


# ---- properties ------------------------------------------------------------------------------------------------------


def test_properties():
    """The variance with gradient observations is <= the GP's own at every query (up to 1e-10 kss); s2_grad = 1e12
    reproduces the GP's own predict to 1e-6 relative (the gradient rows then carry relative weight <= kss / s2_grad ~
    1e-12; the margin is for the rescaled, jitter-free system); on y = sin(sum x / sqrt D) with its analytic gradient
    the held-out RMSE at 200 points is smaller with gradients than without."""
    rng = np.random.default_rng(2)
    gp, model, X, y, Xg, dy, hyp, counts = _problem(40, 40, 3, "matern", 5, "const", seed=7, repeat=40)
    xs = rng.uniform(-2, 2, (200, 3))
    kss = np.exp(2 * hyp[:, 3])
    mu0, s20 = gp.predict(xs, separate_samples=True)
    dy_true = np.cos(Xg.sum(1, keepdims=True) / np.sqrt(3)) / np.sqrt(3) * np.ones((1, 3))
    with gp.condition_on_gradients(Xg, dy_true, 1e-4) as cp:
        mu1, s21 = cp.predict(xs, separate_samples=True)
        mu1m, s21m = cp.predict(xs)
    assert mu1m.shape == (200, 1) and s21m.shape == (200, 1)
    assert np.all(s21 <= s20 + 1e-10 * kss[None, :])
    truth = np.sin(xs.sum(1) / np.sqrt(3))
    rmse = lambda m: np.sqrt(np.mean((m - truth) ** 2))
    mu0m, _ = gp.predict(xs)
    print("held-out RMSE without / with gradients:", rmse(mu0m[:, 0]), rmse(mu1m[:, 0]))
    assert rmse(mu1m[:, 0]) < rmse(mu0m[:, 0])
    with gp.condition_on_gradients(Xg, dy, 1e12) as cp:
        mu2, s22 = cp.predict(xs, separate_samples=True)
    assert _close(mu2, mu0, 1e-6) and _close(s22, s20, 1e-6)


def test_invariance():
    """A sample alone or in a batch of 3, and two calls: the same bits.  predict in one block of queries or in two:
    equal to rounding (1e-13 relative)."""
    gp, model, X, y, Xg, dy, hyp, counts = _problem(70, 37, 3, "matern", 5, "const", seed=8)
    xs = np.random.default_rng(3).uniform(-2, 2, (70, 3))
    cp = gp.condition_on_gradients(Xg, dy, 0.01)
    cp2 = gp.condition_on_gradients(Xg, dy, 0.01)
    mu, s2 = cp.predict(xs, separate_samples=True)
    mu2, s22 = cp2.predict(xs, separate_samples=True)
    assert np.array_equal(mu, mu2) and np.array_equal(s2, s22) and np.array_equal(cp.nlZ, cp2.nlZ)
    for s in range(3):
        assert all(np.array_equal(a, b) for a, b in zip(cp.alpha[s], cp2.alpha[s]))
    gp1 = _gp(model, 3)
    gp1.update(X_new=X, y_new=y, hyp=hyp[1:2])
    with gp1.condition_on_gradients(Xg, dy, 0.01) as c1:
        m1, v1 = c1.predict(xs, separate_samples=True)
        assert np.array_equal(m1[:, 0], mu[:, 1]) and np.array_equal(v1[:, 0], s2[:, 1])
        assert c1.nlZ[0] == cp.nlZ[1] and all(np.array_equal(a, b) for a, b in zip(c1.alpha[0], cp.alpha[1]))
    ma, va = cp.predict(xs[:30], separate_samples=True)
    mb, vb = cp.predict(xs[30:], separate_samples=True)
    assert _close(np.concatenate([ma, mb]), mu, 1e-13) and _close(np.concatenate([va, vb]), s2, 1e-13)
    cp.close()
    cp2.close()


def test_the_gp_is_untouched():
    """gp.predict, gp.nll_batch and Posterior.alpha are bit-identical before and after condition_on_gradients +
    predict + close (the context's resident data go to the joint system and come back through the data token)."""
    gp, model, X, y, Xg, dy, hyp, counts = _problem(70, 20, 3, "se", 0, "negquad", seed=9)
    xs = np.random.default_rng(5).uniform(-2, 2, (33, 3))
    before = (gp.predict(xs, separate_samples=True), gp.nll_batch(hyp, compute_grad=True),
              [np.array(p.alpha) for p in gp.posteriors])
    cp = gp.condition_on_gradients(Xg, dy, 0.01)
    cp.predict(xs)
    mid = gp.predict(xs, separate_samples=True)  # (while the object is alive)
    cp.predict(xs)
    cp.close()
    after = (gp.predict(xs, separate_samples=True), gp.nll_batch(hyp, compute_grad=True),
             [np.array(p.alpha) for p in gp.posteriors])
    assert all(np.array_equal(a, b) for a, b in zip(before[0], mid))
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0]))
    assert all(np.array_equal(a, b) for a, b in zip(before[1], after[1]))
    assert all(np.array_equal(a, b) for a, b in zip(before[2], after[2]))
    assert np.array_equal(gp.X, X) and np.array_equal(gp.y, y) and len(gp.posteriors) == 3


# ---- refusals and errors ---------------------------------------------------------------------------------------------


def test_refusals_and_errors():
    import gpyreg_amd as gpr
    from numpy.linalg import LinAlgError

    gp, model, X, y, Xg, dy, hyp, counts = _problem(30, 8, 2, "matern", 5, "const", seed=10)
    cp = gp.condition_on_gradients(Xg, dy, 0.01)
    h = cp._handle
    x = X[:3]
    calls = [lambda: h.predict(x), lambda: h.predict_grad(x), lambda: h.grad_post(x), lambda: h.predict_full(x),
             lambda: h.predict_hess(x), lambda: h.predict_cov(x, x), lambda: h.draw(x, 1, 0), lambda: h.cv(),
             lambda: h.quad(np.zeros((1, 2)), np.ones((1, 2)), False)]
    for call in calls:
        with pytest.raises(RuntimeError, match="gradient observations"):
            call()
    mu, _ = cp.predict(x)  # (the handle still works)
    assert np.all(np.isfinite(mu))
    cp.close()
    # bad arguments
    for bad, exc in [(lambda: gp.condition_on_gradients(Xg[:, :1], dy, 0.01), ValueError),
                     (lambda: gp.condition_on_gradients(Xg, dy[:-1], 0.01), ValueError),
                     (lambda: gp.condition_on_gradients(Xg, dy, -0.01), ValueError),
                     (lambda: gp.condition_on_gradients(Xg, dy, np.ones(3)), ValueError),
                     (lambda: gp.condition_on_gradients(Xg, dy, None), ValueError),
                     (lambda: gp.condition_on_gradients(Xg, dy * np.nan, 0.01), ValueError),
                     (lambda: gp.nll_batch_grad_obs(hyp[:, :-1], Xg, dy, 0.01), ValueError)]:
        with pytest.raises(exc):
            bad()
    m1 = _gp(dict(kernel="matern", degree=1, mean="const", noise=(1, 0, 0)), 2)
    m1.update(X_new=X, y_new=y, hyp=hyp[:1])
    with pytest.raises(NotImplementedError, match="mean-square derivative"):
        m1.condition_on_gradients(Xg, dy, 0.01)

    class Mine:  # the squared exponential as a user-defined object: no device kernel id
        def __init__(self):
            self._k = gpr.covariance_functions.SquaredExponential()

        def __getattr__(self, name):
            if name == "_gpc_kernel_id":
                raise AttributeError(name)
            return getattr(self._k, name)

    user = gpr.GP(2, Mine(), gpr.mean_functions.ConstantMean(), gpr.noise_functions.GaussianNoise(constant_add=True))
    assert not user._builtin
    user.update(X_new=X, y_new=y, hyp=hyp[:1])
    with pytest.raises(NotImplementedError, match="user-defined"):
        user.condition_on_gradients(Xg, dy, 0.01)
    empty = _gp(model, 2)
    with pytest.raises(ValueError):
        empty.condition_on_gradients(Xg, dy, 0.01)
    nopost = _gp(model, 2)
    nopost.update(X_new=X, y_new=y, hyp=hyp[:1], compute_posterior=False)
    with pytest.raises(ValueError, match="posteriors"):
        nopost.condition_on_gradients(Xg, dy, 0.01)
    # exactly duplicated gradient points without noise: a singular joint matrix no multiplier of a zero noise repairs
    Xd, dyd = np.concatenate([Xg, Xg[:2]]), np.concatenate([dy, dy[:2]])
    try:
        with gp.condition_on_gradients(Xd, dyd, 0.0) as cd:
            assert np.all(cd.sn2_mult > 1), cd.sn2_mult
    except LinAlgError:
        pass


def test_nll_batch_grad_obs():
    """Equal to the object's nlZ at the resident hyperparameters, bit for bit; equal to _gradobs at three perturbed rows
    to 1e-8."""
    gp, model, X, y, Xg, dy, hyp, counts = _problem(70, 37, 3, "matern", 5, "negquad", seed=11, repeat=5)
    s2g = _s2_grad("matrix", 37, 3, np.random.default_rng(1))
    with gp.condition_on_gradients(Xg, dy, s2g) as cp:
        nl = gp.nll_batch_grad_obs(hyp, Xg, dy, s2g)
        assert nl.shape == (3,) and np.array_equal(nl, cp.nlZ)
    hyp2 = hyp + 0.1 * np.random.default_rng(2).standard_normal(hyp.shape)
    posts = _reference(gp, model, X, y, Xg, dy, hyp2, counts, s2g)
    assert _close(gp.nll_batch_grad_obs(hyp2, Xg, dy, s2g), [p["nlZ"] for p in posts], 1e-8)
