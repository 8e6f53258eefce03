"""GradientConditionedPosterior.gradient_posterior / predict_grad (gpc_grad_post_gobs): the posterior of the gradient
under gradient observations on the device.

The new operand kernel entry by entry through its hook (gpc_debug_gobs_grad_operand) against the extended-precision
reference of tests/gradobs_ref.py and bit for bit against its two siblings, then the pipeline: parity with the NumPy
model (gpyreg_amd._gradobs.gradient_joint), identities with the object's own predict, properties (a noisily observed
gradient, no variance increase, the large-noise limit, positive semi-definiteness), invariance (batch, chunk, query
block), refusals, and the GP left untouched."""

import numpy as np
import pytest

import gradobs_ref as gr
import scratch_sizes as ss
import test_cov_functors_cpu as cf
from test_gpu_api import _gp
from test_gpu_gradobs import KID, _close, _problem, _reference, _s2_grad

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from gpyreg_amd import _lib

    return _lib.context(0)


# ---- the operand kernel, per entry -----------------------------------------------------------------------------------


def _operand_reference(case):
    """(want (n, D + 1, M) longdouble, bound (n, D + 1, M)) of the operand of one ``gradobs_ref.setup`` case with
    queries: the blocks between the data rows and the rows of the appended queries in the joint covariance of
    [X; X*] and [X_g; X*] (gradobs_ref.joint_cov_ld, with that file's bounds)."""
    (N, D), Ng, M = case["xs"].shape, case["xsg"].shape[0], case["xss"].shape[0]
    ext = dict(case, xs=np.vstack([case["xs"], case["xss"]]), xsg=np.vstack([case["xsg"], case["xss"]]))
    K2, B2 = gr.joint_cov_ld(ext)
    N2, Ng2 = N + M, Ng + M
    rows = np.r_[np.arange(N), [N2 + a * Ng2 + g for a in range(D) for g in range(Ng)]].astype(int)
    want, bound = np.empty((len(rows), D + 1, M), cf.LD), np.empty((len(rows), D + 1, M))
    for slot in range(D + 1):
        cols = N + np.arange(M) if slot == 0 else N2 + (slot - 1) * Ng2 + Ng + np.arange(M)
        want[:, slot], bound[:, slot] = K2[np.ix_(rows, cols)], B2[np.ix_(rows, cols)]
    return want, bound


@pytest.mark.parametrize("N,Ng,D,M", [(70, 37, 1, 70), (70, 37, 3, 128), (129, 65, 3, 64), (20, 64, 33, 7), (65, 1, 1, 3)])
@pytest.mark.parametrize("name,alpha", gr.FAMILIES)
def test_operand_per_entry(ctx, name, alpha, N, Ng, D, M):
    """gobs_grad_operand_tile_kernel against np.longdouble on the same fp64 scaled coordinates, at the origin and 1e4
    length scales away from it, within the per-entry bounds of tests/gradobs_ref.py: worst ratio <= 1.  No NaN is left
    of the preset panel; the rows >= n and the queries >= M are exactly 0; the fused sums equal panel^T alpha recomputed
    from the returned panel within 1e-13 sum |panel| |alpha| per column.  (20, 64, 33, 7) stages more than one chunk of
    dimensions; at (65, 1, 1, 3) the point list has 3 tiles of 64 where the panel has 2."""
    rng = np.random.default_rng(N + D)
    n = N + Ng * D
    for shift in (0.0, 1e4):
        case = gr.setup(name, alpha, N, Ng, D, shift, M=M)
        kind, degree, hyp, X, Xg, Xq = (case[k] for k in ("kind", "degree", "hyp", "X", "Xg", "Xq"))
        alpha_v = rng.standard_normal(n)
        B, panel, col = ctx.debug_gobs_grad_operand(kind, degree, hyp, X, Xg, Xq, alpha_v)
        assert B.shape == (n, D + 1, M) and panel.shape == (-(-n // 128) * 128, D + 1, 128) and col.shape == (D + 1, M)
        assert np.all(np.isfinite(panel)), (name, shift, "an entry nobody wrote")
        assert np.all(panel[n:] == 0) and np.all(panel[:, :, M:] == 0), (name, shift, "padding is not exactly 0")
        want, bound = _operand_reference(case)
        r = gr.worst(B, want, bound)
        print(f"{name} {alpha} ({N},{Ng},{D},{M}) shift {shift:g}: operand worst error / bound {r:.3f}")
        assert r <= 1.0, (name, alpha, shift, r)
        terms = np.abs(B) * np.abs(alpha_v)[:, None, None]
        err = np.abs(col - np.einsum("iaj,i->aj", B, alpha_v))
        assert np.all(err <= 1e-13 * terms.sum(0)), (name, shift, (err / np.maximum(terms.sum(0), 1e-300)).max())


def test_operand_same_bits_as_the_siblings(ctx):
    """N = 70, Ng = 37, D = 3, M = 128: the rows [0, N) of every slot are the plain GP's grad_operand_tile_kernel panel
    (Context.debug_cov "grad_operand") and slot 0 of all n rows is gobs_cross_tile_kernel's panel, bit for bit."""
    N, Ng, D, M = 70, 37, 3, 128
    n = N + Ng * D
    for name, alpha in gr.FAMILIES:
        for shift in (0.0, 1e2):
            case = gr.setup(name, alpha, N, Ng, D, shift, M=M)
            kind, degree, hyp, X, Xg, Xq = (case[k] for k in ("kind", "degree", "hyp", "X", "Xg", "Xq"))
            al = np.random.default_rng(3).standard_normal(n)
            B, _, _ = ctx.debug_gobs_grad_operand(kind, degree, hyp, X, Xg, Xq, al)
            plain = ctx.debug_cov("grad_operand", kind, degree, hyp, X, X_star=Xq, vec=al[:N])[0]
            assert plain.shape == (128, D + 1, 128)
            assert np.array_equal(B[:N], plain[:N, :, :M]), (name, shift, "value rows")
            cross, _, _ = ctx.debug_gobs_cross(kind, degree, hyp, X, Xg, Xq, al)
            assert np.array_equal(B[:, 0], cross), (name, shift, "slot 0")


# ---- the pipeline against the NumPy model ----------------------------------------------------------------------------


def _model(gp, model, X, Xg, hyp, counts, posts, xs):
    """(mean (M, D + 1, S), cov (M, D + 1, D + 1, S)) of _gradobs.gradient_joint with the mean function added here."""
    from gpyreg_amd import _gradobs as go
    from gpyreg_amd.gaussian_process import _mean_grad_x

    cov_N, noise_N, _ = counts
    kid, degree = KID[model["kernel"]], model["degree"]
    D = X.shape[1]
    mean, cov = np.empty((xs.shape[0], D + 1, len(posts))), np.empty((xs.shape[0], D + 1, D + 1, len(posts)))
    for s, p in enumerate(posts):
        mean[:, :, s], cov[:, :, :, s] = go.gradient_joint(kid, degree, hyp[s, :cov_N], X, Xg, xs, p)
        hm = hyp[s, cov_N + noise_N:]
        mean[:, 0, s] += np.reshape(gp.mean.compute(hm, xs), (-1,))
        mean[:, 1:, s] += _mean_grad_x(gp.mean, hm, xs)
    return mean, cov


def _queries(X, Xg, M, seed=9):
    xs = np.random.default_rng(seed).uniform(-2, 2, (M, X.shape[1]))
    xs[0] = X[0]    # a query ON a training row
    xs[1] = Xg[0]   # ... and on a gradient point
    return xs


def _check_pipeline(gp, cp, posts, model, X, Xg, hyp, counts, xs, rtol):
    S, P = len(posts), X.shape[1] + 1
    want_mean, want_cov = _model(gp, model, X, Xg, hyp, counts, posts, xs)
    mean, cov = cp.gradient_posterior(xs, with_value=True, separate_samples=True)
    assert mean.shape == (xs.shape[0], P, S) and cov.shape == (xs.shape[0], P, P, S)
    for s in range(S):
        assert _close(mean[..., s], want_mean[..., s], rtol), (s, "mean", np.abs(mean[..., s] - want_mean[..., s]).max())
        assert _close(cov[..., s], want_cov[..., s], rtol), (s, "cov", np.abs(cov[..., s] - want_cov[..., s]).max())
    assert np.array_equal(cov, cov.transpose(0, 2, 1, 3)), "a per-sample matrix is not symmetric to the bit"
    mean_d, var = cp.gradient_posterior(xs, cov="diag", with_value=True, separate_samples=True)
    full_d = np.einsum("maas->mas", cov)
    assert var.shape == (xs.shape[0], P, S) and np.array_equal(mean_d, mean)
    assert np.abs(var - full_d).max() <= 1e-10 * np.abs(full_d).max() if rtol < 1e-6 else _close(var, full_d, rtol)
    # without the value: the trailing block
    dm, dc = cp.gradient_posterior(xs, separate_samples=True)
    assert np.array_equal(dm, mean[:, 1:]) and np.array_equal(dc, cov[:, 1:, 1:])


PIPELINE = [
    # N, Ng, D, M, S, kernel, degree, mean, dtype, repeated rows
    (70, 37, 3, 130, 3, "matern", 5, "const", "f64", 18),    # two query blocks, the second of 2 queries
    (70, 37, 3, 130, 3, "se", 0, "negquad", "f32", 18),
    (70, 37, 3, 130, 3, "se_iso", 0, "zero", "f64", 0),
    (20, 5, 9, 7, 2, "rq", 0, "zero", "f64", 0),             # D + 1 = 10 > GTB = 8: more than one register-tile pair
    (20, 5, 9, 7, 2, "matern", 3, "const", "f64", 0),
    (20, 5, 9, 7, 2, "matern_iso", 5, "negquad", "f32", 0),
    (600, 150, 3, 5, 1, "se", 0, "const", "f64", 0),         # n = 1050, npad = 1152: gram_segments = 2
    (600, 150, 3, 5, 1, "matern", 5, "negquad", "f32", 0),
]


@pytest.mark.parametrize("N,Ng,D,M,S,kernel,degree,mean,dtype,repeat", PIPELINE)
def test_pipeline_against_numpy(N, Ng, D, M, S, kernel, degree, mean, dtype, repeat):
    """Mean and covariance of (f, grad f) per sample against gpyreg_amd._gradobs.gradient_joint: the project's parity
    bar, 1e-8 in the scale-relative metric for fp64 handles, 1e-3 for fp32.  cov="diag" against the diagonal of "full"
    (1e-10 relative in fp64); every per-sample matrix equals its transpose to the bit."""
    gp, model, X, y, Xg, dy, hyp, counts = _problem(N, Ng, D, kernel, degree, mean, S=S, dtype=dtype, repeat=repeat)
    s2g = _s2_grad("vector", Ng, D, np.random.default_rng(4))
    posts = _reference(gp, model, X, y, Xg, dy, hyp, counts, s2g)
    with gp.condition_on_gradients(Xg, dy, s2g) as cp:
        assert list(cp.L_chol) == [True] * S
        _check_pipeline(gp, cp, posts, model, X, Xg, hyp, counts, _queries(X, Xg, M), 1e-8 if dtype == "f64" else 1e-3)


def test_pipeline_low_noise_and_mixed_batch():
    """s2_grad = 0 (every sample on the low-noise branch, L = -inv) and a batch whose samples take different branches
    [L_chol, low, L_chol]: the shapes of test_gpu_gradobs.py's test of the same name."""
    gp, model, X, y, Xg, dy, hyp, counts = _problem(40, 12, 3, "matern", 5, "const", seed=3)
    posts = _reference(gp, model, X, y, Xg, dy, hyp, counts, 0.0)
    with gp.condition_on_gradients(Xg, dy, 0.0) as cp:
        assert list(cp.L_chol) == [False] * 3
        _check_pipeline(gp, cp, posts, model, X, Xg, hyp, counts, _queries(X, Xg, 40), 1e-8)
    gp, model, X, y, Xg, dy, hyp, counts = _problem(40, 12, 3, "se", 0, "const", seed=4,
                                                    sn_rows=np.array([0.1, np.sqrt(1e-7), 0.1]))
    posts = _reference(gp, model, X, y, Xg, dy, hyp, counts, 0.01)
    with gp.condition_on_gradients(Xg, dy, 0.01) as cp:
        assert list(cp.L_chol) == [True, False, True]
        _check_pipeline(gp, cp, posts, model, X, Xg, hyp, counts, _queries(X, Xg, 40), 1e-8)


# ---- identities with the object's own methods ------------------------------------------------------------------------


def test_identities_against_the_shipped_methods():
    """Slot 0 of with_value=True is cp.predict (1e-10: the same operand rows through another product form);
    predict_grad's dmu is the gradient slots to the bit and its ds2 is 2 C[0, 1:] (1e-9); mu and s2 of predict_grad are
    predict's; the mixture is _gradpost.mix of the separate samples (rtol 1e-13); add_noise adds the noise times the
    multiplier and leaves the gradients alone."""
    from gpyreg_amd import _gradpost as gpm

    gp, model, X, y, Xg, dy, hyp, counts = _problem(70, 37, 3, "matern", 5, "negquad", seed=12, repeat=5)
    xs = _queries(X, Xg, 40)
    with gp.condition_on_gradients(Xg, dy, 0.01) as cp:
        mean, cov = cp.gradient_posterior(xs, with_value=True, separate_samples=True)
        mu, s2 = cp.predict(xs, separate_samples=True)
        assert np.abs(mean[:, 0] - mu).max() <= 1e-10 * np.abs(mu).max()
        assert np.abs(cov[:, 0, 0] - s2).max() <= 1e-10 * np.abs(s2).max()
        pmu, ps2, dmu, ds2 = cp.predict_grad(xs, separate_samples=True)
        assert pmu.shape == (40, 3) and ps2.shape == (40, 3) and dmu.shape == (40, 3, 3) and ds2.shape == (40, 3, 3)
        assert np.array_equal(dmu, mean[:, 1:]) and np.array_equal(pmu, mean[:, 0])
        assert np.array_equal(ps2, np.maximum(cov[:, 0, 0], 0))
        assert np.abs(ds2 - 2 * cov[:, 0, 1:]).max() <= 1e-9 * np.abs(2 * cov[:, 0, 1:]).max()
        mm, mc = cp.gradient_posterior(xs, with_value=True)
        wm, wc = gpm.mix(mean, cov)
        assert mm.shape == (40, 4) and mc.shape == (40, 4, 4)
        assert np.allclose(mm, wm, rtol=1e-13, atol=0) and np.allclose(mc, wc, rtol=1e-13, atol=1e-13 * np.abs(wc).max())
        dd, dv = cp.gradient_posterior(xs, cov="diag")
        wd, wv = gpm.mix_diag(mean[:, 1:], np.einsum("maas->mas", cov)[:, 1:])
        assert dd.shape == (40, 3) and np.allclose(dd, wd, rtol=1e-13, atol=0) and np.allclose(dv, wv, rtol=1e-9, atol=0)
        # the mixed predict_grad: predict's mixture and the gradients of its moments
        qmu, qs2, qdmu, qds2 = cp.predict_grad(xs)
        rmu, rs2 = cp.predict(xs)
        assert qmu.shape == (40, 1) and qdmu.shape == (40, 3) and qds2.shape == (40, 3)
        assert np.abs(qmu - rmu).max() <= 1e-10 * np.abs(rmu).max() and np.abs(qs2 - rs2).max() <= 1e-10 * np.abs(rs2).max()
        assert np.allclose(qdmu, dmu.mean(2), rtol=1e-13, atol=0)
        nmu, ns2, ndmu, nds2 = cp.predict_grad(xs, add_noise=True, separate_samples=True)
        rmu2, rs22 = cp.predict(xs, add_noise=True, separate_samples=True)
        assert np.abs(ns2 - rs22).max() <= 1e-10 * np.abs(rs22).max() and np.array_equal(nmu, pmu)
        assert np.array_equal(ndmu, dmu) and np.array_equal(nds2, ds2)


# ---- properties ------------------------------------------------------------------------------------------------------


def test_properties():
    """With s2_grad = 1e-6 the posterior variance of d_l f at a gradient point is <= s2_grad + 1e-10 F0 c_l^2 (the
    posterior variance of a noisily observed quantity cannot exceed its noise); every diagonal entry is <= the plain
    GP's + 1e-10 H (conditioning on more data cannot raise a variance); s2_grad = 1e12 reproduces GP.gradient_posterior
    to 1e-6 (test_gpu_gradobs.py's bar and reasoning: the gradient rows carry relative weight ~1e-12); the smallest
    eigenvalue of every (D + 1) x (D + 1) matrix is >= -1e-10 x its largest entry."""
    from gpyreg_amd import _gradpost as gpm

    gp, model, X, y, Xg, dy, hyp, counts = _problem(40, 40, 3, "matern", 5, "const", seed=7, repeat=20)
    rng = np.random.default_rng(2)
    xs = np.concatenate([Xg[:25], rng.uniform(-2, 2, (60, 3))])
    H = np.stack([gpm.prior_block(KID["matern"], 5, h[:counts[0]], 3) for h in hyp], axis=1)  # (D + 1, S)
    m0, c0 = gp.gradient_posterior(xs, with_value=True, separate_samples=True)
    with gp.condition_on_gradients(Xg, dy, 1e-6) as cp:
        m1, c1 = cp.gradient_posterior(xs, with_value=True, separate_samples=True)
        v1 = cp.gradient_posterior(xs, cov="diag", with_value=True, separate_samples=True)[1]
    d0, d1 = np.einsum("maas->mas", c0), np.einsum("maas->mas", c1)
    assert np.all(d1[:25, 1:] <= 1e-6 + 1e-10 * H[None, 1:]), (d1[:25, 1:].max(), "a gradient point's variance")
    assert np.all(v1[:25, 1:] <= 1e-6 + 1e-10 * H[None, 1:])
    assert np.all(d1 <= d0 + 1e-10 * H[None]) and np.all(v1 <= d0 + 1e-10 * H[None])
    for c in (c0, c1):
        w = np.linalg.eigvalsh(c.transpose(0, 3, 1, 2))
        assert np.all(w[..., 0] >= -1e-10 * np.abs(c).max(axis=(1, 2))), w[..., 0].min()
    with gp.condition_on_gradients(Xg, dy, 1e12) as cp:
        m2, c2 = cp.gradient_posterior(xs, with_value=True, separate_samples=True)
        v2 = cp.gradient_posterior(xs, cov="diag", with_value=True, separate_samples=True)[1]
    assert _close(m2, m0, 1e-6) and _close(c2, c0, 1e-6) and _close(v2, d0, 1e-6)


# ---- invariance ------------------------------------------------------------------------------------------------------


def test_sample_alone_in_a_batch_and_chunked_bitwise(monkeypatch):
    """A sample's results are the same bits alone, in a batch of 3 (one of them on the low-noise branch), and under a
    memory budget that forces one sample per chunk (non-resident constants: the point lists are scaled per chunk);
    full and diag."""
    from gpyreg_amd import _lib

    gp, model, X, y, Xg, dy, hyp, counts = _problem(70, 37, 3, "se", 0, "const", seed=8,
                                                    sn_rows=np.array([0.1, np.sqrt(1e-7), 0.1]))
    xs = _queries(X, Xg, 70, seed=14)
    get = lambda cp: (cp.gradient_posterior(xs, with_value=True, separate_samples=True)
                      + cp.gradient_posterior(xs, cov="diag", with_value=True, separate_samples=True))
    cp = gp.condition_on_gradients(Xg, dy, 0.01)
    whole = get(cp)
    for s in range(3):
        one = _gp(model, 3)
        one.update(X_new=X, y_new=y, hyp=hyp[s:s + 1])
        with one.condition_on_gradients(Xg, dy, 0.01) as c1:
            for a, b in zip(get(c1), whole):
                assert np.array_equal(a[..., 0], b[..., s]), s
    # n = 181, npad = 256, D = 3: the smallest budget that holds one sample's scratch and not two
    w = 8
    per = [ss.grad_post_per(256, 3, diag, w) + (((128 + 64) // 64) - 256 // 64) * 4 * 128 * 8 for diag in (False, True)]
    mb = ss.budget_for_chunk(3, 1, max(per), 70 * 3 * 8)
    assert mb is not None and ss.planned_chunk(3, mb, min(per), 70 * 3 * 8) == 1
    monkeypatch.setenv("GPC_MEM_BUDGET_MB", str(mb))
    chunked, chunks = [], []
    for diag in ("full", "diag"):
        chunked += list(cp.gradient_posterior(xs, cov=diag, with_value=True, separate_samples=True))
        chunks.append(_lib.context(gp.device).get_option("last_chunk"))
    monkeypatch.delenv("GPC_MEM_BUDGET_MB")
    assert chunks == [1, 1], chunks
    for a, b in zip(whole, chunked):
        assert np.array_equal(a, b)
    cp.close()


def test_query_alone_or_among_150_to_rounding():
    """150 queries span two query blocks of 128: a query's results alone, in the first and in the second block agree to
    1e-12 relative (the blocks are separate launches of the same forms)."""
    gp, model, X, y, Xg, dy, hyp, counts = _problem(70, 37, 3, "matern", 5, "const", seed=8)
    xs = _queries(X, Xg, 150, seed=15)
    with gp.condition_on_gradients(Xg, dy, 0.01) as cp:
        mean, cov = cp.gradient_posterior(xs, with_value=True, separate_samples=True)
        for j in (0, 1, 77, 127, 128, 149):
            m1, c1 = cp.gradient_posterior(xs[j:j + 1], with_value=True, separate_samples=True)
            assert np.abs(m1[0] - mean[j]).max() <= 1e-12 * np.abs(mean).max(), j
            assert np.abs(c1[0] - cov[j]).max() <= 1e-12 * np.abs(cov).max(), j


# ---- refusals; the GP is left alone ----------------------------------------------------------------------------------


def test_refusals_and_the_gp_is_untouched():
    import gpyreg_amd as gpr

    gp, model, X, y, Xg, dy, hyp, counts = _problem(30, 8, 2, "matern", 5, "const", seed=10)
    xs = np.random.default_rng(5).uniform(-2, 2, (9, 2))
    before = ([np.array(p.alpha) for p in gp.posteriors], gp.predict(xs, separate_samples=True))
    with pytest.raises(RuntimeError, match="no gradient observations"):
        gp._post_handle.grad_post_gobs(xs)
    cp = gp.condition_on_gradients(Xg, dy, 0.01)
    for bad in (np.zeros((3, 3)), np.full((2, 2), np.nan), np.array([[0.0, np.inf]])):
        for call in (cp.gradient_posterior, cp.predict_grad):
            with pytest.raises(ValueError, match="x_star"):
                call(bad)
    with pytest.raises(ValueError, match="cov must be"):
        cp.gradient_posterior(xs, cov="both")
    mu, _ = cp.predict(xs)  # the handle still predicts
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(cp.gradient_posterior(xs)[1]))
    cp.close()
    for call in (cp.gradient_posterior, cp.predict_grad):
        with pytest.raises(ValueError, match="closed"):
            call(xs)

    class MyMean(gpr.mean_functions.ConstantMean):  # a user-defined mean: its x-gradient is unknown
        pass

    user = gpr.GP(2, gpr.covariance_functions.Matern(5), MyMean(), gpr.noise_functions.GaussianNoise(constant_add=True))
    user.update(X_new=X, y_new=y, hyp=hyp[:1])
    with pytest.raises(NotImplementedError, match="user-defined"):
        user.condition_on_gradients(Xg, dy, 0.01)  # (the joint mean rows already need the gradient)
    with gp.condition_on_gradients(Xg, dy, 0.01) as cp2:
        cp2._mean = MyMean()
        for call in (cp2.gradient_posterior, cp2.predict_grad):
            with pytest.raises(NotImplementedError, match="user-defined"):
                call(xs)
        assert np.all(np.isfinite(cp2.predict(xs)[0]))  # the handle still predicts
        cp2._mean = gp.mean
        assert np.all(np.isfinite(cp2.predict_grad(xs)[3]))
    after = ([np.array(p.alpha) for p in gp.posteriors], gp.predict(xs, separate_samples=True))
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0]))
    assert all(np.array_equal(a, b) for a, b in zip(before[1], after[1]))
    assert np.array_equal(gp.X, X) and np.array_equal(gp.y, y) and len(gp.posteriors) == 3
