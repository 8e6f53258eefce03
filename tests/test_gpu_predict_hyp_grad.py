"""GP.predict_hyp_grad / gpc_predict_hyp_grad and GP.predict_laplace: derivatives of the prediction with respect to the
hyperparameters.

The fused cross kernel entry by entry through its hook (gpc_debug_hyp_cross), then the pipeline: parity with the NumPy
restatement (gpyreg_amd._hypgrad) on the golden core cases and at sizes that cross the tiles and the query blocks,
low-noise and mixed batches, per-point noise, inputs far from the origin, appended posteriors; invariance bit for bit
(batch, chunking, compute_var, sharding) and to rounding (query blocks); central differences of predict on the device;
predict_laplace against sigma points; the clamp, the refusals and the budget failure."""

import os
import socket
import sys

import numpy as np
import pytest

from conftest import parse_core_name
from test_gpu_predict_grad import _counts, _gp, _lownoise_problem, _problem
from test_gpu_predict_hess import FAMILIES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KID = {"se": 0, "matern": 1, "rq": 2, "se_iso": 3, "matern_iso": 4}


@pytest.fixture(scope="module")
def ctx():
    from gpyreg_amd import _lib

    return _lib.context(0)


# ---- the cross kernel, per entry -------------------------------------------------------------------------------------

_CROSS_CASES = {}


def _cross_case(name, N, M, D):
    """One problem per (family, shape): inputs, weights and the NumPy sums with their sums of absolute terms, on the
    device's own scaling of the inputs (x mul / dv, operation for operation).  Query 0 equals a training point; P covers
    the covariance hyperparameters and two more weight vectors."""
    from gpyreg_amd import _hypgrad as hg

    key = (name, N, M, D)
    if key not in _CROSS_CASES:
        kid, degree, iso, extra = FAMILIES[name]
        rng = np.random.default_rng(1000 * N + 10 * M + D)
        X = rng.uniform(-2, 2, (N, D))
        xs = rng.uniform(-2, 2, (M, D))
        xs[0] = X[N // 2]
        ell = np.log(1.2 * np.sqrt(D)) + 0.1 * rng.standard_normal(1 if iso else D)
        hyp = np.r_[ell, 0.2] if extra is None else np.r_[ell, 0.2, np.log(extra)]
        cov_N = hyp.size
        alpha = rng.standard_normal(N)
        W = rng.standard_normal((cov_N + 2, N))
        Q = rng.standard_normal((N, M))
        nl = 1 if iso else D
        snu = np.sqrt(float(degree)) if kid in (1, 4) else 1.0
        dv = np.exp(hyp[:nl]) * np.ones(D)
        mul, div = ((snu * np.ones(D), dv) if iso or kid == 0 else (snu / dv, np.ones(D)))
        with np.errstate(all="ignore"):
            k, dk = hg.cross_planes(kid, degree, hyp, X, xs, xs=X * mul / div, xss=xs * mul / div)
        dk[hg.sf_col(kid, D)] = k  # the kernel leaves k itself in log sf's column; the caller doubles it
        dk = np.stack(dk)  # (cov_N, N, M)
        adk = np.abs(dk)
        if kid == 2:
            # Ka = K (r2 / (2 m) - alpha log m) is a DIFFERENCE of terms that nearly cancel at small r2 (both ~ r2 / 2): its
            # own terms count among the absolute terms, as in test_gpu_nll_hess's plane test
            xa, xb = X * mul / div, xs * mul / div
            r2 = np.zeros((N, M))
            for l in range(D):
                r2 += (xb[None, :, l] - xa[:, None, l]) ** 2
            rqa = np.exp(hyp[D + 1])
            m = 1 + r2 / (2 * rqa)
            adk[D + 1] = k * (r2 / (2 * m) + rqa * np.log(m))
        ref = dict(B=(W @ k).T, A=np.einsum("cij,i->jc", dk, alpha), C=np.einsum("cij,ij->jc", dk, Q))
        mag = dict(B=(np.abs(W) @ np.abs(k)).T, A=np.einsum("cij,i->jc", adk, np.abs(alpha)),
                   C=np.einsum("cij,ij->jc", adk, np.abs(Q)))
        _CROSS_CASES[key] = (kid, degree, hyp, X, xs, alpha, W, Q, ref, mag)
    return _CROSS_CASES[key]


@pytest.mark.parametrize("name", list(FAMILIES))
def test_cross_kernel_per_entry(ctx, name):
    """Every reduced sum -- k w_p for the P weight vectors, d_c k alpha and d_c k Q for the covariance columns -- against
    NumPy within 1e-12 times the sum of the absolute values of its terms (the bound and rationale of
    test_gpu_predict_hess.test_contraction_kernel_per_entry: the same closed form on the same inputs, differing in the
    rounding of exp / sqrt / log and in the order).  N and M cross the 64-tile and the 128-query block and include the
    single-row case; D crosses the 32-dimension staging of the distances; query 0 lies ON a training point (nothing to
    a lengthscale sum).  The mean-only kernel gives the same bits for the sums it forms."""
    for N in (1, 64, 65, 130):
        for M in (1, 64, 65, 129):
            for D in (1, 2, 10, 17, 33):
                kid, degree, hyp, X, xs, alpha, W, Q, ref, mag = _cross_case(name, N, M, D)
                B, A, C = ctx.debug_hyp_cross(kid, degree, hyp, X, xs, alpha, W, Q)
                for tag, got in (("B", B), ("A", A), ("C", C)):
                    assert got.shape == ref[tag].shape, (name, N, M, D, tag)
                    err = np.abs(got - ref[tag])
                    assert np.all(err <= 1e-12 * mag[tag]), (name, N, M, D, tag, (err / np.maximum(mag[tag], 1e-300)).max())
                if D in (2, 17) and M in (1, 129):
                    B0, A0, none = ctx.debug_hyp_cross(kid, degree, hyp, X, xs, alpha, W, None)
                    assert none is None and np.array_equal(B0, B) and np.array_equal(A0, A), (name, N, M, D, "mean-only")


# ---- the pipeline ----------------------------------------------------------------------------------------------------


def _restated(gp, xs, var=True, s2_star=None, add_noise=False):
    """GP.predict_hyp_grad restated on the host from _hypgrad.hyp_grad, per resident sample, at the samples' own
    multipliers: (mu, s2, dmu, ds2) with the mean function, unclamped."""
    from gpyreg_amd import _hypgrad as hg
    from gpyreg_amd.gaussian_process import _mean_hyp, _sn2_mult

    kid, degree = gp._kid()
    cov_N, noise_N, mean_N = counts = gp._counts()
    hyp = np.stack([p.hyp for p in gp.posteriors])
    pv = gp._plugin_values(hyp, True)
    out = []
    for s in range(hyp.shape[0]):
        mult = float(_sn2_mult(gp.posteriors[s]))
        fmu, fs2, dfmu, dfs2 = hg.hyp_grad(kid, degree, hyp[s, :cov_N], gp.X, xs, gp.y[:, 0] - pv["m"][s], pv["sn2"][s], mult,
                                           None if pv["dm"] is None else pv["dm"][s],
                                           None if pv["dsn2"] is None else pv["dsn2"][s], var)
        hm = _mean_hyp(hyp[s:s + 1], counts)
        m = gp.mean.values(hm, xs, mean_N > 0)
        if mean_N > 0:
            m, dm = m
            dfmu[:, cov_N + noise_N:] += dm[0]
        fmu = fmu + m[0]
        if add_noise:
            ns, dns = gp.noise.values(hyp[s:s + 1, cov_N:cov_N + noise_N], xs, None, s2_star, True)
            fs2 = fs2 + mult * np.broadcast_to(ns[0], (xs.shape[0],))
            dfs2[:, cov_N:cov_N + noise_N] += mult * np.broadcast_to(dns[0], (xs.shape[0], noise_N))
        out.append((fmu, fs2, dfmu, dfs2))
    return [None if out[0][i] is None else np.stack([o[i] for o in out], -1) for i in range(4)]


def _assert_parity(got, ref, tol, what, keep=None):
    """Each of (mu, s2, dmu, ds2) per sample to tol[s] of max(1, largest reference entry); ``keep`` (M, S): the queries
    whose variance entries are compared (the clamp has a test of its own)."""
    for i, which in enumerate(("mu", "s2", "dmu", "ds2")):
        assert got[i].shape == ref[i].shape, (what, which)
        assert np.all(np.isfinite(got[i])), (what, which)
        for s in range(ref[i].shape[-1]):
            rows = np.ones(ref[i].shape[0], bool) if keep is None or i % 2 == 0 else keep[:, s]
            if not rows.any():
                continue
            e = np.abs(got[i][rows, ..., s] - ref[i][rows, ..., s]).max()
            assert e <= tol[s] * max(1.0, np.abs(ref[i][..., s]).max()), (what, which, s, e)


def test_parity_on_the_golden_core_cases(core_golden):
    """Every golden model but Matern 1 at its own data, hyperparameters and queries: 1e-8 of max(1, largest reference
    entry), the project's fp64 bound, for the plain cases; the ill-conditioned flavours (low noise, jitter) to
    1e-8 + 1e-14 cond(K + Sigma) -- what two factorizations of such a matrix may differ by -- and not compared where
    that exceeds 1 %.  Queries whose latent variance is 0 to the bound keep their variance entries out (the clamp)."""
    from gpyreg_amd import _nllhess as nh

    g = core_golden
    done, lchol0 = 0, 0
    for name in g["names"]:
        tag, model, N, D, flavour = parse_core_name(name)
        if model["kernel"].startswith("matern") and model["degree"] == 1:
            continue
        X, y, hyp, xs = g[tag + "_X"], g[tag + "_y"], g[tag + "_hyp"], g[tag + "_xs"]
        s2 = g[tag + "_s2"] if tag + "_s2" in g.files else None
        gp = _gp(model, D)
        gp.update(X_new=X, y_new=y, s2_new=s2, hyp=hyp)
        tol = np.full(hyp.shape[0], 1e-8)
        if flavour != "plain":
            cov_N = _counts(model, D)[0]
            pv = gp._plugin_values(hyp, False)
            for s in range(hyp.shape[0]):
                K = nh.cov_derivatives(KID[model["kernel"]], model["degree"], hyp[s, :cov_N], X)[0]
                sn2 = np.broadcast_to(pv["sn2"][s], (N,)) * float(gp.posteriors[s].sn2_mult)
                tol[s] += 1e-14 * np.linalg.cond(K + np.diag(sn2))
            if np.any(tol > 1e-2):
                continue
        ref = _restated(gp, xs)
        keep = ref[1] > tol[None, :] * np.maximum(1.0, np.abs(ref[1]).max(0))[None, :]
        ref[1], ref[3] = np.maximum(ref[1], 0), ref[3]
        got = gp.predict_hyp_grad(xs)
        _assert_parity(got, ref, tol, name, keep)
        done += 1
        lchol0 += not gp.posteriors[0].L_chol
    assert done >= 27, done


@pytest.mark.parametrize("kernel,degree,mean", [("se", 0, "negquad"), ("rq", 0, "const"), ("matern_iso", 5, "zero")])
def test_parity_across_tiles_and_query_blocks(kernel, degree, mean):
    """N in {65, 130, 300} (one row past a 64-tile, past a 128-tile, several tiles) and M in {1, 129, 260} (one query, one
    past a block, three blocks) at three samples: 1e-8 of max(1, largest reference entry)."""
    for N in (65, 130, 300):
        gp, model, X, y, hyp = _problem(kernel, degree, mean, N=N)
        for M in (1, 129, 260):
            xs = np.random.default_rng(N + M).uniform(-2, 2, (M, X.shape[1]))
            ref = _restated(gp, xs)
            assert np.all(ref[1] > 1e-6)
            _assert_parity(gp.predict_hyp_grad(xs), ref, [1e-8] * 3, (kernel, N, M))
            mean_only = gp.predict_hyp_grad(xs, compute_var=False)
            assert mean_only[1] is None and mean_only[3] is None
            _assert_parity([mean_only[0], ref[1], mean_only[2], ref[3]], ref, [1e-8] * 3, (kernel, N, M, "mean only"))


@pytest.mark.parametrize("sn2s", [(1e-7, 1e-8), (1e-2,), (1e-2, 1e-7, 1e-7, 1e-2, 1e-7, 1e-2)])
def test_low_noise_lchol_and_mixed_batches(sn2s):
    """L_chol = 0 samples alone, an L_chol = 1 sample alone, and both interleaved (several runs with nonzero sample
    offsets in one call): parity with the restatement at 1e-8 of max(1, largest entry) (cond(K + Sigma) ~ 1e2 by the
    problem's construction), and each sample bitwise equal to its own single-sample GP."""
    gp, model, X, y, hyp = _lownoise_problem(sn2s)
    xs = np.random.default_rng(12).uniform(-3, 3, (50, X.shape[1]))
    got = gp.predict_hyp_grad(xs)
    ref = _restated(gp, xs)
    assert np.all(ref[1] > 0)
    _assert_parity(got, ref, [1e-8] * len(sn2s), sn2s)
    for s in range(len(sn2s)):
        one = _gp(model, X.shape[1])
        one.update(X_new=X, y_new=y, hyp=hyp[s:s + 1])
        for a, b in zip(one.predict_hyp_grad(xs), got):
            assert np.array_equal(a[..., 0], b[..., s]), s


def _per_point_problem(kernel="matern", degree=5, N=130, D=3, S=2, noise=(1, 2, 0), seed=4):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (N, D))
    y = np.sin(X.sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1))
    s2 = rng.uniform(0.5, 2.0, (N, 1)) * 0.01
    model = dict(kernel=kernel, degree=degree, mean="negquad", noise=noise)
    cov_N, noise_N, mean_N = _counts(model, D)
    hyp = np.zeros((S, cov_N + noise_N + mean_N))
    hyp[:, :D] = np.log(1.2)
    hyp[:, cov_N] = np.log(0.1)
    if noise[2]:
        hyp[:, cov_N + noise_N - 2] = float(np.median(y))
        hyp[:, cov_N + noise_N - 1] = np.log(0.2)
    hyp[:, cov_N + noise_N + 1 + D:] = np.log(3.0)
    hyp += 0.05 * rng.standard_normal(hyp.shape)
    gp = _gp(model, D)
    gp.update(X_new=X, y_new=y, s2_new=s2, hyp=hyp)
    return gp, X, y, s2, hyp


@pytest.mark.parametrize("noise", [(1, 2, 0), (1, 1, 1)])
def test_per_point_noise_and_noise_at_the_queries(noise):
    """Noise per training point (a scaled provided term; a provided term plus the output-dependent one): the weighted
    column sums of squares take the vectors sn2 and d_n sn2 instead of scalars.  Parity at 1e-8 of max(1, largest
    entry), with and without noise at x* (``s2_star`` provided per query)."""
    gp, X, y, s2, hyp = _per_point_problem(noise=noise)
    xs = np.random.default_rng(5).uniform(-2, 2, (70, X.shape[1]))
    s2s = np.random.default_rng(6).uniform(0.005, 0.02, (70, 1))
    assert gp._plugin_values(hyp, True)["vec"]
    _assert_parity(gp.predict_hyp_grad(xs), _restated(gp, xs), [1e-8] * 2, noise)
    got = gp.predict_hyp_grad(xs, add_noise=True, s2_star=s2s)
    _assert_parity(got, _restated(gp, xs, s2_star=s2s, add_noise=True), [1e-8] * 2, (noise, "add_noise"))
    with pytest.raises(ValueError, match="add_noise needs compute_var"):
        gp.predict_hyp_grad(xs, compute_var=False, add_noise=True)


@pytest.mark.parametrize("kernel,degree", [("se", 0), ("matern", 3), ("rq", 0), ("matern_iso", 5)])
def test_far_from_the_origin(kernel, degree):
    """X and x* shifted by 1e4 lengthscales against the restatement of the UNSHIFTED problem (the same function) at
    1e-8 of max(1, largest entry).  The shift rounds the scaled coordinates at 1e4 2^-53 ~ 1e-12; the differences are
    taken first, so that is what reaches d and the radial factors; through the solves it is amplified by
    cond(K + Sigma) ~ 1e3 at most here (N = 150, noise sd 0.3)."""
    rng = np.random.default_rng(31)
    N, D, S = 150, 3, 2
    X = rng.uniform(-2, 2, (N, D))
    y = np.sin(X.sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1))
    model = dict(kernel=kernel, degree=degree, mean="const", noise=(1, 0, 0))
    cov_N, noise_N, mean_N = _counts(model, D)
    hyp = np.zeros((S, cov_N + noise_N + mean_N))
    hyp[:, :D] = np.log(1.2)
    hyp[:, cov_N] = np.log(0.3)
    hyp += 0.05 * rng.standard_normal(hyp.shape)
    xs = rng.uniform(-2, 2, (20, D))
    shift = 1e4 * 1.2 * np.array([1.0, -1.0, 0.5])
    near = _gp(model, D)
    near.update(X_new=X, y_new=y, hyp=hyp)
    ref = _restated(near, xs)
    far = _gp(model, D)
    far.update(X_new=X + shift, y_new=y, hyp=hyp)
    _assert_parity(far.predict_hyp_grad(xs + shift), ref, [1e-8] * S, kernel)


def test_after_block_append_and_one_point_append():
    """Posteriors extended in place -- ten points by update(..., block_append=True), then one by the rank-one path --
    against the restatement on the extended data at the records' own multipliers: 1e-8 of max(1, largest entry)."""
    gp, model, X, y, hyp = _problem("matern", 5, "const", N=141)
    inc = _gp(model, X.shape[1])
    inc.update(X_new=X[:130], y_new=y[:130], hyp=hyp)
    h0 = inc._post_handle
    xs = np.random.default_rng(8).uniform(-2, 2, (40, X.shape[1]))
    inc.update(X_new=X[130:140], y_new=y[130:140], block_append=True)
    assert inc._post_handle is h0 and h0.N == 140
    _assert_parity(inc.predict_hyp_grad(xs), _restated(inc, xs), [1e-8] * 3, "block append")
    inc.update(X_new=X[140:], y_new=y[140:])
    assert inc._post_handle is h0 and h0.N == 141
    _assert_parity(inc.predict_hyp_grad(xs), _restated(inc, xs), [1e-8] * 3, "one-point append")
    _assert_parity(inc.predict_hyp_grad(xs), gp.predict_hyp_grad(xs), [1e-8] * 3, "against the full recompute")


# ---- invariance ------------------------------------------------------------------------------------------------------


def test_sample_alone_in_a_batch_chunked_and_mean_only_bitwise(monkeypatch):
    """A sample's results are the same bits alone, in a batch of 5 that mixes L_chol runs, and under a memory budget that
    forces one sample per chunk (non-resident constants, runs cut at the chunk borders); compute_var=False leaves mu
    and dmu with the same bits, launches no product (gpc_last_timing's ms_factor is 0 with the timing events on; with
    the variance it is positive)."""
    gp, model, X, y, hyp = _lownoise_problem((1e-2, 1e-7, 1e-2, 1e-2, 1e-7), N=100, D=3)
    xs = np.random.default_rng(14).uniform(-3, 3, (70, 3))
    c = gp._post_handle.ctx
    c.set_option("small_timing", 1)
    try:
        whole = gp.predict_hyp_grad(xs)
        assert c.last_timing()[1] > 0
        mean_only = gp.predict_hyp_grad(xs, compute_var=False)
        total, factor = c.last_timing()
        assert factor == 0 and total > 0
    finally:
        c.set_option("small_timing", 0)
    assert mean_only[1] is None and mean_only[3] is None
    assert np.array_equal(mean_only[0], whole[0]) and np.array_equal(mean_only[2], whole[2])
    for s in range(5):
        one = _gp(model, 3)
        one.update(X_new=X, y_new=y, hyp=hyp[s:s + 1])
        for a, b in zip(one.predict_hyp_grad(xs), whole):
            assert np.array_equal(a[..., 0], b[..., s]), s
    # scratch of one sample at npad = 128, D = 3, P = 6, one block of 128 queries: the plane, three panels and the
    # partials, 74753 doubles = 0.6 MB; 80 % of 1 MB holds one sample, not two.  Without the variance a sample needs 6273
    # doubles and all five fit: that call runs the forced path in one chunk.  The library reports the chunk it planned
    from scratch_sizes import hyp_grad_per, planned_chunk

    per_var, per_mean = hyp_grad_per(128, 3, 6, 1, 3, 128, True, 6 + 2 * 4), hyp_grad_per(128, 3, 6, 1, 3, 128, False, 6 + 4)
    assert (per_var, per_mean) == (74753 * 8, 6273 * 8)
    assert (planned_chunk(5, 1, per_var), planned_chunk(5, 1, per_mean)) == (1, 5)
    monkeypatch.setenv("GPC_MEM_BUDGET_MB", "1")
    chunked = gp.predict_hyp_grad(xs)
    assert c.get_option("last_chunk") == planned_chunk(5, 1, per_var)
    chunked_mean = gp.predict_hyp_grad(xs, compute_var=False)
    assert c.get_option("last_chunk") == planned_chunk(5, 1, per_mean)
    monkeypatch.delenv("GPC_MEM_BUDGET_MB")
    for a, b in zip(whole, chunked):
        assert np.array_equal(a, b)
    assert np.array_equal(whole[0], chunked_mean[0]) and np.array_equal(whole[2], chunked_mean[2])


def test_query_blocks_to_rounding(monkeypatch):
    """260 queries against their three pieces of 128, 128 and 4, and against the same call under a budget that splits
    the queries into super-blocks of 128 (1 MB: the scratch of one sample with all 384 padded queries is 1.5 MB, with
    256 it is 1.05 MB): 1e-12 of each array's largest entry per query.  Not asserted bitwise: the products are
    launches of other widths."""
    gp, model, X, y, hyp = _problem("matern", 5, "const", N=100, S=2)
    xs = np.random.default_rng(15).uniform(-2, 2, (260, X.shape[1]))
    whole = gp.predict_hyp_grad(xs)
    pieces = [gp.predict_hyp_grad(xs[a:b]) for a, b in ((0, 128), (128, 256), (256, 260))]
    # the planner refuses the blocks of 384 and 256 padded queries and halves down to 128, of which one sample fits
    from scratch_sizes import hyp_grad_per, planned_chunk

    fit = [planned_chunk(2, 1, hyp_grad_per(128, 3, 6, 1, 3, msb, True, 6 + 2 * 4)) for msb in (384, 256, 128)]
    assert fit[:2] == [0, 0] and fit[2] >= 1
    monkeypatch.setenv("GPC_MEM_BUDGET_MB", "1")
    split = gp.predict_hyp_grad(xs)
    assert gp._post_handle.ctx.get_option("last_chunk") == fit[2]
    monkeypatch.delenv("GPC_MEM_BUDGET_MB")
    for i in range(4):
        joined = np.concatenate([p[i] for p in pieces], axis=0)
        for other in (joined, split[i]):
            for j in range(260):
                assert np.abs(other[j] - whole[i][j]).max() <= 1e-12 * np.abs(whole[i][j]).max(), (i, j)


# ---- against the shipped methods -------------------------------------------------------------------------------------


@pytest.mark.parametrize("kernel,degree,mean", [("se", 0, "negquad"), ("matern", 5, "const"), ("rq", 0, "zero"),
                                                ("se_iso", 0, "const")])
def test_central_differences_of_predict_on_the_device(kernel, degree, mean):
    """dmu and ds2 against central differences of predict(separate_samples=True) after update(hyp=theta +- h e_p), all
    2 P shifted vectors in one batch: sn = 0.3, N = 130 (cond(K + Sigma) ~ 1e3, every multiplier 1), h = 1e-4, to 1e-6
    of the column's largest entry (truncation ~ h^2 = 1e-8, rounding ~ cond 2^-53 / h = 1e-9).  Measured on an MI355X,
    worst column per case: se / negquad 2.2e-8, matern5 / const 7.4e-9, rq / zero 8.5e-9, se_iso / const 4.0e-8."""
    rng = np.random.default_rng(21)
    N, D = 130, 3
    X = rng.uniform(-2, 2, (N, D))
    y = np.sin(X.sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1))
    model = dict(kernel=kernel, degree=degree, mean=mean, noise=(1, 0, 0))
    cov_N, noise_N, mean_N = _counts(model, D)
    P = cov_N + noise_N + mean_N
    th = np.zeros(P)
    th[:1 if kernel.endswith("_iso") else D] = np.log(1.1)
    th[cov_N] = np.log(0.3)
    if mean == "negquad":
        th[cov_N + noise_N + 1 + D:] = np.log(3.0)
    th += 0.05 * rng.standard_normal(P)
    xs = rng.uniform(-2, 2, (30, D))
    gp = _gp(model, D)
    gp.update(X_new=X, y_new=y, hyp=th[None])
    assert gp.posteriors[0].sn2_mult == 1
    mu, s2, dmu, ds2 = gp.predict_hyp_grad(xs)
    h = 1e-4
    shifted = np.concatenate([th[None] + h * np.eye(P), th[None] - h * np.eye(P)])
    gp.update(hyp=shifted)
    assert all(p.sn2_mult == 1 for p in gp.posteriors)
    pm, ps2 = gp.predict(xs, separate_samples=True)
    worst = 0.0
    for which, an, f in (("dmu", dmu[..., 0], pm), ("ds2", ds2[..., 0], ps2)):
        fd = (f[:, :P] - f[:, P:]) / (2 * h)
        for p in range(P):
            scale = np.abs(an[:, p]).max()
            if scale == 0:
                assert np.abs(fd[:, p]).max() <= 1e-9, (which, p)
                continue
            err = np.abs(fd[:, p] - an[:, p]).max() / scale
            worst = max(worst, err)
            assert err <= 1e-6, (kernel, which, p, err)
    print(f"{kernel}{degree} {mean}: worst column against central differences {worst:.2e}")


def test_predict_laplace_against_sigma_points():
    """At a mode found by a few Newton steps on log_posterior_hess (no fit), where laplace_approximation reports
    is_pd: var_mu = g^T Sigma g equals sum_i ((mu(theta + sqrt(eps) L e_i) - mu(theta - sqrt(eps) L e_i)) / 2)^2 / eps with
    Sigma = L L^T and eps = 1e-8 -- the same central difference in rotated directions -- to 1e-6 relative; the 2 k sigma
    points are evaluated in one update(hyp=...) batch.  Measured on an MI355X: 3.3e-9."""
    rng = np.random.default_rng(23)
    N, D = 130, 2
    X = rng.uniform(-2, 2, (N, D))
    y = np.sin(1.3 * X[:, :1]) * np.cos(0.7 * X[:, 1:]) + 0.3 * rng.standard_normal((N, 1))
    model = dict(kernel="se", degree=0, mean="const", noise=(1, 0, 0))
    gp = _gp(model, D)
    th = np.array([0.0, 0.3, -0.3, np.log(0.3), 0.0])
    gp.update(X_new=X, y_new=y, hyp=th[None])
    for _ in range(12):
        val, g, H = gp.log_posterior_hess(th)
        w, V = np.linalg.eigh(-H)
        step = V @ ((V.T @ g) / np.maximum(np.abs(w), 1e-3 * np.abs(w).max()))
        th = th + step * min(1.0, 1.0 / np.abs(step).max())
    gp.update(hyp=th[None])
    assert gp.posteriors[0].sn2_mult == 1
    lap = gp.laplace_approximation()
    assert lap["is_pd"] and np.array_equal(lap["free"], np.arange(5))
    xs = rng.uniform(-2, 2, (25, D))
    out = gp.predict_laplace(xs, lap)
    mu, s2, dmu, ds2 = gp.predict_hyp_grad(xs)
    assert np.array_equal(out["mu"], mu[:, 0]) and np.array_equal(out["s2"], s2[:, 0])
    assert np.array_equal(out["s2_total"], out["s2"] + out["var_mu"]) and np.all(out["var_s2"] >= 0)
    L = np.linalg.cholesky(lap["cov"])
    eps = 1e-8
    pts = np.concatenate([th[None] + np.sqrt(eps) * L.T, th[None] - np.sqrt(eps) * L.T])
    gp.update(hyp=pts)
    assert all(p.sn2_mult == 1 for p in gp.posteriors)
    pm, _ = gp.predict(xs, separate_samples=True)
    want = np.sum(((pm[:, :5] - pm[:, 5:]) / 2) ** 2, 1) / eps
    err = np.abs(out["var_mu"] - want) / want
    print(f"predict_laplace: var_mu against sigma points, worst relative error {err.max():.2e}")
    assert np.all(err <= 1e-6), err.max()


# ---- behaviour -------------------------------------------------------------------------------------------------------


def test_clamp_zeroes_the_variance_gradient(monkeypatch):
    """Where the device's latent variance is <= 0 the clamp holds s2 at 0 and ds2 is 0 in every column; elsewhere they are
    the device's; noise at x* is added after the clamp."""
    gp, model, X, y, hyp = _lownoise_problem((1e-2,), N=40, D=3)
    h = gp._post_handle
    real = h.predict_hyp_grad
    xs = np.random.default_rng(17).uniform(-3, 3, (12, 3))
    cov_N = _counts(model, 3)[0]
    raw = []

    def shifted(*a, **k):
        out = list(real(*a, **k))
        raw[:] = out
        out[1] = out[1].copy()
        out[1][0:5, 0] = -1e-3
        out[1][5, 0] = 0.0
        return tuple(out)

    monkeypatch.setattr(h, "predict_hyp_grad", shifted)
    mu, s2, dmu, ds2 = gp.predict_hyp_grad(xs)
    assert np.all(s2[:6] == 0) and np.all(ds2[:6] == 0) and np.all(s2[6:] > 0)
    assert np.array_equal(ds2[6:], raw[3][6:]) and np.array_equal(s2[6:], raw[1][6:])
    _, s2n, _, ds2n = gp.predict_hyp_grad(xs, add_noise=True)
    assert np.allclose(s2n[:6, 0], 1e-2, rtol=1e-12) and np.allclose(ds2n[:6, cov_N, 0], 2e-2, rtol=1e-12)
    assert np.all(ds2n[:6, :cov_N] == 0)


def test_refusals(ctx):
    import gpyreg_amd as gpr
    from gpyreg_amd import _lib
    from test_gpu_user_kernel import PySquaredExponential

    rng = np.random.default_rng(0)
    X = rng.uniform(-1, 1, (40, 2))
    y = np.sin(X[:, :1])
    hyp = np.array([[0.0, 0.0, 0.0, np.log(0.1), 0.0]])
    noise = gpr.noise_functions.GaussianNoise(constant_add=True)
    const = gpr.mean_functions.ConstantMean()
    lib = _lib.load()
    p = _lib._ptr
    xs = np.zeros((3, 2))
    o = dict(fmu=np.empty((3, 1)), fs2=np.empty((3, 1)), dfmu=np.empty((3, 5, 1)), dfs2=np.empty((3, 5, 1)))
    sn2, dsn2, dm = np.array([[1e-2]]), np.array([[[2e-2]]]), np.ones((1, 40, 1))

    def raw(gp, M=3, var=1, x=xs, rows=1, sn=sn2, **drop):
        h = gp._post_handle
        a = {k: (None if k in drop else p(v)) for k, v in o.items()}
        rc = lib.gpc_predict_hyp_grad(h._h, None if x is None else p(x), M, var, None if sn is None else p(sn), p(dsn2), rows,
                                      1, p(dm), 1, a["fmu"], a["fs2"], a["dfmu"], a["dfs2"])
        return rc, lib.gpc_last_error(h.ctx._h).decode()

    gp = gpr.GP(2, gpr.covariance_functions.SquaredExponential(), const, noise)
    gp.update(X_new=X, y_new=y, hyp=hyp)
    assert raw(gp)[0] == 0
    for r in (raw(gp, M=0), raw(gp, x=None), raw(gp, sn=None), raw(gp, rows=7), raw(gp, fmu=True), raw(gp, dfmu=True),
              raw(gp, fs2=True), raw(gp, dfs2=True), raw(gp, var=0, fmu=True)):
        assert r[0] == -2 and r[1].startswith("gpc_predict_hyp_grad: bad arguments"), r
    assert raw(gp, var=0, fs2=True, dfs2=True)[0] == 0  # the variance outputs may be NULL without it
    # Matern 1
    for cov_obj in (gpr.covariance_functions.Matern(1), gpr.isotropic_covariance_functions.MaternIsotropic(1)):
        g1 = gpr.GP(2, cov_obj, const, noise)
        g1.update(X_new=X, y_new=y, hyp=hyp[:, :g1.covariance.hyperparameter_count(2) + 2])
        rc, msg = raw(g1)
        assert rc == -2 and msg.startswith("gpc_predict_hyp_grad: the Matern kernel of degree 1")
        with pytest.raises(NotImplementedError, match="predict_hyp_grad: the Matern kernel of degree 1"):
            g1.predict_hyp_grad(xs)
    # fp32
    g32 = gpr.GP(2, gpr.covariance_functions.SquaredExponential(), const, noise, dtype="f32")
    g32.update(X_new=X, y_new=y, hyp=hyp)
    rc, msg = raw(g32)
    assert rc == -2 and msg == "gpc_predict_hyp_grad: the hyperparameter gradients are fp64 only; this posterior is " \
                               "stored in fp32"
    with pytest.raises(NotImplementedError, match="predict_hyp_grad: .*fp64 only; this GP's dtype is 'f32'"):
        g32.predict_hyp_grad(xs)
    # user-defined plugins
    gk = gpr.GP(2, PySquaredExponential(), const, noise)
    gk.update(X_new=X, y_new=y, hyp=hyp)
    rc, msg = raw(gk)
    assert rc == -2 and msg.startswith("gpc_predict_hyp_grad: this posterior was built from caller-provided K")
    with pytest.raises(NotImplementedError, match="predict_hyp_grad: the covariance function .*PySquaredExponential"):
        gk.predict_hyp_grad(xs)

    class MyMean(gpr.mean_functions.ConstantMean):
        pass

    class MyNoise(gpr.noise_functions.GaussianNoise):
        pass

    gm = gpr.GP(2, gpr.covariance_functions.SquaredExponential(), MyMean(), noise)
    gm.update(X_new=X, y_new=y, hyp=hyp)
    with pytest.raises(NotImplementedError, match="predict_hyp_grad: the mean function .*MyMean"):
        gm.predict_hyp_grad(xs)
    gn = gpr.GP(2, gpr.covariance_functions.SquaredExponential(), const, MyNoise(constant_add=True))
    gn.update(X_new=X, y_new=y, hyp=hyp)
    with pytest.raises(NotImplementedError, match="predict_hyp_grad: the noise function .*MyNoise"):
        gn.predict_hyp_grad(xs)
    # a cleaned GP
    gp.clean()
    with pytest.raises(ValueError, match="posteriors have been cleaned"):
        gp.predict_hyp_grad(xs)
    # a failed factorization
    ctx.set_data(X, y)
    handle, mult, lchol, info = ctx.posterior_batch(0, 0, _lib.F64, np.zeros((2, 3)), np.zeros((2, 40)),
                                                    np.array([[1e-2], [-1e12]]), False)
    try:
        assert info[0] == 0 and info[1] != 0
        with pytest.raises(RuntimeError, match="gpc_predict_hyp_grad: posterior contains a failed factorization"):
            handle.predict_hyp_grad(xs, 3, np.full((2, 1), 1e-2))
    finally:
        handle.free()
    # the hook's own argument checks
    with pytest.raises(RuntimeError, match="gpc_debug_hyp_cross: the Matern kernel of degree 1"):
        ctx.debug_hyp_cross(1, 1, np.zeros(3), X, xs, np.zeros(40), np.zeros((3, 40)))
    with pytest.raises(RuntimeError, match="gpc_debug_hyp_cross: P must cover"):
        ctx.debug_hyp_cross(0, 0, np.zeros(3), X, xs, np.zeros(40), np.zeros((2, 40)))


def test_budget_failure_names_the_sizes(monkeypatch):
    gp, model, X, y, hyp = _lownoise_problem((1e-2,), N=300, D=3)
    xs = np.zeros((5, 3))
    # at N_pad = 384 the dense plane alone is 1.2 MB; the message carries the scratch's bytes, to the byte what the
    # closed form gives (P = 6, one noise vector, three planes, 6 + 2 * 4 sums per query)
    from scratch_sizes import hyp_grad_per

    per = hyp_grad_per(384, 3, 6, 1, 3, 128, True, 6 + 2 * 4)
    monkeypatch.setenv("GPC_MEM_BUDGET_MB", "1")
    with pytest.raises(RuntimeError, match=r"gpc_predict_hyp_grad: the scratch of one sample with one query block \(%d " % per +
                                           r"bytes: N_pad = 384, planes = 3, block = 128 queries\) exceeds the device "
                                           r"memory budget \(\d+ bytes\)"):
        gp.predict_hyp_grad(xs)
    monkeypatch.delenv("GPC_MEM_BUDGET_MB")
    gp.predict_hyp_grad(xs)  # and the context is usable afterwards


# ---- sharding: the pattern of test_gpu_predict_hess.py ---------------------------------------------------------------


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
        bench.CONFIGS[3] = dict(bench.CONFIGS[3], N=300)
        for S in (1, 5):
            X, y, hyp = bench.synthetic_problem(3, S)
            xs = X[:20] + 0.05
            ref = bench.make_gp(3, "f64")
            ref.shard = False
            ref.update(X_new=X, y_new=y, hyp=hyp)
            gp = bench.make_gp(3, "f64")
            gp.update(X_new=X, y_new=y, hyp=hyp)
            ok = {}
            for kw in (dict(), dict(compute_var=False), dict(add_noise=True)):
                a = ref.predict_hyp_grad(xs, **kw)
                b = gp.predict_hyp_grad(xs, **kw)
                ok[str(kw)] = all((u is None and v is None) or np.array_equal(u, v) for u, v in zip(a, b))
            out[S] = ok
    except Exception as e:  # noqa: BLE001 - reported to the parent
        out["exception"] = repr(e)
    finally:
        dist.destroy_process_group()
    q.put((rank, out))


def test_sharded_equals_unsharded_bitwise_two_ranks_one_gpu():
    import torch.multiprocessing as mp

    mctx = mp.get_context("spawn")
    q = mctx.Queue()
    port = _free_port()
    procs = [mctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for rank in (0, 1):
        r = res[rank]
        assert "exception" not in r, r.get("exception")
        for S in (1, 5):
            assert all(r[S].values()), (rank, S, r[S])
