"""GP.predict_hess / gpc_predict_hess: Hessians of the predictive mean and variance with respect to the query point.

The contraction kernel entry by entry through its hook (gpc_debug_hess_contract), then the pipeline: parity with the
NumPy restatement (gpyreg_amd._hess) on the golden core cases, low-noise and mixed batches, inputs far from the origin,
predict_grad's values and central differences of its analytic gradients, invariance bit for bit (symmetry, batch,
chunking, compute_var, sharding) and to rounding (query blocks), the clamp, the refusals and the budget failure."""

import os
import socket
import sys

import numpy as np
import pytest

from conftest import parse_core_name
from test_cov_functors_cpu import F32, F64
from test_gpu_gradient_posterior import KID, _solve_sensitivity
from test_gpu_predict_grad import _counts, _gp, _lownoise_problem, _problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (kernel id, degree, isotropic, extra hyperparameter)
FAMILIES = {"se": (0, 0, False, None), "matern3": (1, 3, False, None), "matern5": (1, 5, False, None),
            "rq": (2, 0, False, 0.7), "se_iso": (3, 0, True, None), "matern_iso3": (4, 3, True, None),
            "matern_iso5": (4, 5, True, None)}


@pytest.fixture(scope="module")
def ctx():
    from gpyreg_amd import _lib

    return _lib.context(0)


def _tri(sG):
    """(M, D, D) -> (M, D (D + 1) / 2): entry a (a + 1) / 2 + b = [a, b], a >= b."""
    D = sG.shape[1]
    a, b = np.tril_indices(D)
    return sG[:, a, b]


# ---- the contraction kernel, per entry -------------------------------------------------------------------------------

_CONTRACT_CASES = {}


def _contract_case(name, N, M, D):
    """One problem per (family, shape), shared by the fp64 and the fp32 test: inputs, weights and the NumPy sums with
    their sums of absolute terms.  Query 0 equals a training point; Q is exactly representable in fp32."""
    from gpyreg_amd import _hess as hm

    key = (name, N, M, D)
    if key not in _CONTRACT_CASES:
        kid, degree, iso, extra = FAMILIES[name]
        rng = np.random.default_rng(1000 * N + 10 * M + D)
        X = rng.uniform(-2, 2, (N, D))
        xs = rng.uniform(-2, 2, (M, D))
        xs[0] = X[N // 2]
        ell = np.log(1.2 * np.sqrt(D)) + 0.1 * rng.standard_normal(1 if iso else D)
        hyp = np.r_[ell, 0.2] if extra is None else np.r_[ell, 0.2, np.log(extra)]
        alpha = rng.standard_normal(N)
        Q = rng.standard_normal((N, M)).astype(np.float32).astype(np.float64)
        # the device's own scaling of the inputs, operation for operation (x mul / dv: _hess scales by c = mul / dv, one
        # rounding more, which a difference d ~ 1e-5 shows at 1e-11 relative): the same closed form on the same inputs
        nl = 1 if iso else D
        snu = np.sqrt(float(degree)) if kid in (1, 4) else 1.0
        dv = np.exp(hyp[:nl]) * np.ones(D)
        mul, div = ((snu * np.ones(D), dv) if iso or kid == 0 else (snu / dv, np.ones(D)))
        sf2, rqa = np.exp(2 * hyp[nl]), (np.exp(hyp[nl + 1]) if extra is not None else 1.0)
        diff = (xs * mul / div)[None, :, :] - (X * mul / div)[:, None, :]
        r2 = np.zeros((N, M))
        for l in range(D):
            r2 += diff[:, :, l] ** 2
        with np.errstate(all="ignore"):
            _, F, G = hm.radial2(kid, degree, r2, sf2, rqa)
        G = np.where(r2 > 0, G, 0.0)
        ref = {}
        for tag, w in (("alpha", alpha[:, None] * np.ones((1, M))), ("q", Q)):
            sF, sG = hm.contract(w, F, G, diff)
            aF, aG = hm.contract(np.abs(w), np.abs(F), np.abs(G), np.abs(diff))
            ref[tag] = (np.c_[sF, _tri(sG)], np.c_[aF, _tri(aG)])
        _CONTRACT_CASES[key] = (kid, degree, hyp, X, xs, alpha, Q, ref)
    return _CONTRACT_CASES[key]


@pytest.mark.parametrize("dtype,rtol", [(F64, 1e-12), (F32, 1e-6)])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_contraction_kernel_per_entry(ctx, name, dtype, rtol):
    """Every reduced sum -- w F and w G d_a d_b, a >= b, for the weights alpha and a dense Q -- against NumPy within
    rtol times the sum of the absolute values of its terms: both sides evaluate the same closed form and differ in the
    rounding of exp / sqrt and in the order.  N and M cross the 64-tile and the 128-query block and include the
    single-row case; D crosses the 8-dimension blocks of the pairs and the 32-dimension staging of the distances;
    query 0 lies ON a training point (G term 0, F term whole).  The mean-only kernel gives the alpha sums' bits."""
    for N in (1, 64, 65, 130):
        for M in (1, 64, 65, 129):
            for D in (1, 2, 10, 17, 33):
                kid, degree, hyp, X, xs, alpha, Q, ref = _contract_case(name, N, M, D)
                got_a, got_q = ctx.debug_hess_contract(kid, degree, hyp, X, xs, alpha, Q, dtype=dtype)
                for tag, got in (("alpha", got_a), ("q", got_q)):
                    want, mag = ref[tag]
                    assert got.shape == want.shape
                    err = np.abs(got - want)
                    assert np.all(err <= rtol * mag), (name, N, M, D, tag, (err / np.maximum(mag, 1e-300)).max())
                if D in (2, 17) and M in (1, 129):
                    only_a, none = ctx.debug_hess_contract(kid, degree, hyp, X, xs, alpha, None, dtype=dtype)
                    assert none is None and np.array_equal(only_a, got_a), (name, N, M, D, "mean-only kernel")


# ---- the pipeline ----------------------------------------------------------------------------------------------------


def _restated(model, posts, X, xs):
    """Per-sample (mu, s2, dmu, ds2, Hmu, Hs2) stacked on a trailing axis, without the mean function, from the oracle's
    posterior records."""
    from gpyreg_amd import _hess as hm
    from oracle import gp_oracle as orc

    cov_N = orc.cov_count(model["kernel"], X.shape[1])
    out = [hm.record(KID[model["kernel"]], model["degree"], p.hyp[:cov_N], X, xs, p.alpha, p.sW, p.L, p.L_chol)
           for p in posts]
    return [np.stack([o[i] for o in out], -1) for i in range(6)]


def _mean_parts(model, hyp, xs):
    """The mean function's value (M, S), gradient (M, D, S) and Hessian (M, D, D, S)."""
    from oracle import gp_oracle as orc

    M, D = xs.shape
    cov_N, noise_N, _ = _counts(model, D)
    m, dm, Hm = np.zeros((M, len(hyp))), np.zeros((M, D, len(hyp))), np.zeros((M, D, D, len(hyp)))
    for s, h in enumerate(hyp):
        hmn = h[cov_N + noise_N:]
        m[:, s] = np.reshape(orc.mean(model["mean"], hmn, xs), (-1,))
        if model["mean"] == "negquad":
            dm[:, :, s] = -(xs - hmn[1:1 + D]) / np.exp(2 * hmn[1 + D:])
            Hm[:, :, :, s] = -np.diag(np.exp(-2 * hmn[1 + D:]))
    return m, dm, Hm


def _extended_operands(model, posts, X, xs):
    """Per sample the N x (1 + D + D^2) x M stack [k | dk/dx* | d^2 k / dx* dx*]: what the solves of the Hessians act
    on, for _solve_sensitivity."""
    from gpyreg_amd import _hess as hm
    from oracle import gp_oracle as orc

    D = X.shape[1]
    cov_N = orc.cov_count(model["kernel"], D)
    Bs = []
    for p in posts:
        c, diff, k, F, G = hm.pair_terms(KID[model["kernel"]], model["degree"], p.hyp[:cov_N], X, xs)
        dk = -F[:, :, None] * diff * c
        d2 = (G[:, :, None, None] * diff[:, :, :, None] * diff[:, :, None, :] - F[:, :, None, None] * np.eye(D)) \
            * (c[:, None] * c[None, :])
        B = np.concatenate([k[:, :, None], dk, d2.reshape(d2.shape[0], d2.shape[1], D * D)], axis=2)
        Bs.append(np.transpose(B, (0, 2, 1)))
    return Bs


@pytest.mark.parametrize("dtype,rtol,u", [("f64", 1e-8, 1e-14), ("f32", 1e-3, 1e-6)])
def test_parity_with_numpy_restatement(core_golden, dtype, rtol, u):
    """Every golden model whose kernel has a second derivative, with the bound of
    test_gpu_gradient_posterior.test_parity_with_numpy_restatement: the plain cases to rtol of the largest entry, the
    ill-conditioned flavours to rtol plus u times the solve's sensitivity (here of the stack [k | dk | d^2 k]); a case
    whose bound exceeds 1 % of the largest entry is not compared."""
    from gpyreg_amd import _hess as hm
    from oracle import gp_oracle as orc

    g = core_golden
    done, lchol0, matern1 = 0, 0, 0
    for name in g["names"]:
        tag, model, N, D, flavour = parse_core_name(name)
        if model["kernel"].startswith("matern") and model["degree"] == 1:
            matern1 += 1
            continue
        X, y, hyp = g[tag + "_X"], g[tag + "_y"], g[tag + "_hyp"]
        s2 = g[tag + "_s2"] if tag + "_s2" in g.files else None
        xs = g[tag + "_xs"]
        gp = _gp(model, D, dtype)
        try:
            gp.update(X_new=X, y_new=y, s2_new=s2, hyp=hyp)
        except np.linalg.LinAlgError:
            if dtype == "f32" and flavour != "plain":
                continue
            raise
        mult = [p.sn2_mult for p in gp.posteriors]
        try:
            posts = orc.posteriors(model, hyp, X, y, s2, force_mult=mult)
        except np.linalg.LinAlgError:
            if flavour != "plain":
                continue
            raise
        assert [p.L_chol for p in posts] == [p.L_chol for p in gp.posteriors], name
        ref = _restated(model, posts, X, xs)
        sens = _solve_sensitivity(posts, _extended_operands(model, posts, X, xs))
        if flavour != "plain":
            if np.any(u * sens[0] > 1e-2 * np.abs(ref[5]).max()) or np.any(u * sens[1] > 1e-2 * np.abs(ref[4]).max()):
                continue
        else:
            sens[:] = 0
        m, dm, Hm = _mean_parts(model, hyp, xs)
        ref[0], ref[2], ref[4] = ref[0] + m, ref[2] + dm, ref[4] + Hm
        # (the clamp has a test of its own: where the variance is 0 to the bound, the variance entries are not compared)
        amb = ref[1] <= rtol * np.abs(ref[1]).max() + u * sens[0][None, :]
        got = gp.predict_hess(xs, separate_samples=True)
        for i, which in enumerate(("mu", "s2", "dmu", "ds2", "Hmu", "Hs2")):
            assert got[i].shape == ref[i].shape, (name, which)
            assert np.all(np.isfinite(got[i])), (name, which)
            for s in range(hyp.shape[0]):
                keep = ~amb[:, s] if i % 2 else np.ones(xs.shape[0], bool)
                if not keep.any():
                    continue
                e = np.abs(got[i][keep, ..., s] - ref[i][keep, ..., s]).max()
                assert e <= rtol * np.abs(ref[i][..., s]).max() + u * sens[1 - i % 2, s], (name, s, which, e)
        Hmu, Hs2 = gp.predict_hess(xs)[4:]
        eHmu, eHs2 = hm.mix(ref[0], ref[2], ref[4], ref[5])
        assert np.abs(Hmu - eHmu).max() <= rtol * np.abs(eHmu).max() + u * sens[1].max(), name
        if not amb.any():
            spread = 4 * u * sens[1].max() * (np.abs(ref[2]).max() + np.abs(ref[0]).max() + np.abs(ref[4]).max())
            assert np.abs(Hs2 - eHs2).max() <= rtol * np.abs(eHs2).max() + u * sens[0].max() + spread, name
        done += 1
        lchol0 += not gp.posteriors[0].L_chol
    assert done >= 25 - matern1, (done, matern1)
    assert lchol0 >= (1 if dtype == "f64" else 0), lchol0


@pytest.mark.parametrize("dtype,rtol", [("f64", 1e-8), ("f32", 1e-3)])
@pytest.mark.parametrize("sn2s", [(1e-7, 1e-8), (1e-2, 1e-7, 1e-7, 1e-2, 1e-7, 1e-2)])
def test_low_noise_and_mixed_batches(sn2s, dtype, rtol):
    """L_chol = 0 samples alone, and interleaved with L_chol = 1 samples (several runs with nonzero sample offsets in
    one call): parity with the restatement, and each sample bitwise equal to its own single-sample GP."""
    from oracle import gp_oracle as orc

    gp, model, X, y, hyp = _lownoise_problem(sn2s, dtype=dtype)
    xs = np.random.default_rng(12).uniform(-3, 3, (50, X.shape[1]))
    got = gp.predict_hess(xs, separate_samples=True)
    posts = orc.posteriors(model, hyp, X, y, None)
    ref = _restated(model, posts, X, xs)
    m, dm, Hm = _mean_parts(model, hyp, xs)
    ref[0], ref[2], ref[4] = ref[0] + m, ref[2] + dm, ref[4] + Hm
    assert np.all(ref[1] > 0)
    for i, which in enumerate(("mu", "s2", "dmu", "ds2", "Hmu", "Hs2")):
        for s in range(len(sn2s)):
            e = np.abs(got[i][..., s] - ref[i][..., s]).max()
            assert e <= rtol * np.abs(ref[i][..., s]).max(), (which, s, e)
    for s in range(len(sn2s)):
        one = _gp(model, X.shape[1], dtype)
        one.update(X_new=X, y_new=y, hyp=hyp[s:s + 1])
        g1 = one.predict_hess(xs, separate_samples=True)
        for a, b in zip(g1, got):
            assert np.array_equal(a[..., 0], b[..., s]), s


def _spread_queries(X, ell, M, seed, lo=-1.8, hi=1.8):
    """M queries at least 0.1 lengthscale (0.12 of the smallest) from every training point."""
    rng = np.random.default_rng(seed)
    cand = rng.uniform(lo, hi, (8 * M, X.shape[1]))
    dist = np.sqrt(((cand[:, None, :] - X[None, :, :]) ** 2).sum(2)).min(1)
    cand = cand[dist >= 0.12 * np.max(ell)]
    assert cand.shape[0] >= M
    return cand[:M]


@pytest.mark.parametrize("kernel,degree", [("se", 0), ("matern", 3), ("matern", 5), ("rq", 0)])
def test_far_from_the_origin(kernel, degree):
    """The same problem with X and x* shifted by 1e4 lengthscales: every Hessian entry agrees with the unshifted run to
    1e-8 of the largest entry.  The shift rounds the scaled coordinates at 1e4 2^-53 ~ 1e-12; the differences are
    taken first, so that is what reaches d, F and G; through the solves it is amplified by cond(K + Sigma) ~ 1e3 at
    most here (N = 150, noise sd 0.3).  A products-first contraction sum w x_a x_b - ... loses 1e8 2^-53 ~ 1e-8 of
    terms 1e8 times the result's size."""
    from test_gpu_api import _gp as make

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
    xs = _spread_queries(X, np.exp(hyp[:, :D]), 20, 32)
    shift = 1e4 * 1.2 * np.array([1.0, -1.0, 0.5])
    res = []
    for off in (np.zeros(D), shift):
        gp = make(model, D, "f64")
        gp.update(X_new=X + off, y_new=y, hyp=hyp)
        res.append(gp.predict_hess(xs + off, separate_samples=True))
    for i in (4, 5):
        for s in range(S):
            a, b = res[0][i][..., s], res[1][i][..., s]
            assert np.abs(a - b).max() <= 1e-8 * np.abs(a).max(), (kernel, i, s, np.abs(a - b).max() / np.abs(a).max())


@pytest.mark.parametrize("kernel,degree,mean", [("se", 0, "negquad"), ("matern", 3, "const"), ("rq", 0, "zero")])
def test_against_the_shipped_methods(kernel, degree, mean):
    """mu, s2, dmu, ds2 against predict_grad's to 1e-10 of the largest entry -- to rounding, not to the bit: they come
    from the operand panel and the Gram matrix of gradient_posterior, not from predict_grad's kernels.  Hmu and Hs2, per
    sample and mixed, against central differences of predict_grad's analytic gradients at h = 1e-4 lengthscales to 1e-6
    of the largest entry (truncation ~ h^2 = 1e-8, rounding ~ 1e-12 / h = 1e-8)."""
    gp, model, X, y, hyp = _problem(kernel, degree, mean, N=150)
    D, S = X.shape[1], hyp.shape[0]
    ell = np.exp(hyp[:, :D])
    xs = _spread_queries(X, ell, 20, 41)
    for sep in (True, False):
        got = gp.predict_hess(xs, separate_samples=sep)
        pg = gp.predict_grad(xs, separate_samples=sep)
        for i, which in enumerate(("mu", "s2", "dmu", "ds2")):
            a, b = got[i], np.reshape(pg[i], got[i].shape)
            assert np.abs(a - b).max() <= 1e-10 * np.abs(b).max(), (which, sep, np.abs(a - b).max() / np.abs(b).max())
        fd_mu, fd_s2 = np.empty_like(got[4]), np.empty_like(got[5])
        for b in range(D):
            h = 1e-4 * ell[:, b].mean()
            e = np.zeros(D)
            e[b] = h
            _, _, dmp, dsp = gp.predict_grad(xs + e, separate_samples=sep)
            _, _, dmm, dsm = gp.predict_grad(xs - e, separate_samples=sep)
            fd_mu[:, :, b] = (dmp - dmm) / (2 * h)
            fd_s2[:, :, b] = (dsp - dsm) / (2 * h)
        for which, a, f in (("Hmu", got[4], fd_mu), ("Hs2", got[5], fd_s2)):
            for s in range(S if sep else 1):
                av, fv = (a[..., s], f[..., s]) if sep else (a, f)
                err = np.abs(av - fv).max() / np.abs(av).max()
                assert err <= 1e-6, (kernel, which, sep, s, err)


def test_symmetric_and_sample_alone_in_a_batch_and_chunked_bitwise(monkeypatch):
    """Every matrix is symmetric to the bit; a sample's results are the same bits alone, in a batch of 3, and under a
    memory budget that forces one sample per chunk (non-resident constants, runs cut at the chunk borders)."""
    gp, model, X, y, hyp = _lownoise_problem((1e-2, 1e-7, 1e-2), N=100, D=3)
    xs = np.random.default_rng(14).uniform(-3, 3, (70, 3))
    whole = gp.predict_hess(xs, separate_samples=True)
    for H in whole[4:]:
        assert np.array_equal(H, np.transpose(H, (0, 2, 1, 3)))
    for H in gp.predict_hess(xs)[4:]:
        assert np.array_equal(H, np.transpose(H, (0, 2, 1)))
    for s in range(3):
        one = _gp(model, 3)
        one.update(X_new=X, y_new=y, hyp=hyp[s:s + 1])
        for a, b in zip(one.predict_hess(xs, separate_samples=True), whole):
            assert np.array_equal(a[..., 0], b[..., s]), s
    # scratch of one sample at npad = 128, D = 3: two 128 x 512 panels and Q, 128 x 128, of doubles = 1.1 MB, the
    # partials and small vectors; 80 % of 2 MB holds one sample, not two
    from gpyreg_amd import _lib
    from scratch_sizes import planned_chunk, predict_hess_per

    monkeypatch.setenv("GPC_MEM_BUDGET_MB", "2")
    chunked = gp.predict_hess(xs, separate_samples=True)
    chunks = [_lib.context(gp.device).get_option("last_chunk")]
    chunked_mean = gp.predict_hess(xs, compute_var=False, separate_samples=True)
    chunks.append(_lib.context(gp.device).get_option("last_chunk"))
    monkeypatch.delenv("GPC_MEM_BUDGET_MB")
    # the chunks that the scratch's closed form gives (shared: the raw queries): without the variance there is one
    # panel and no Q, and two samples fit
    want = [planned_chunk(3, 2, predict_hess_per(128, 3, var, 8), 70 * 3 * 8) for var in (True, False)]
    assert chunks == want == [1, 2], (chunks, want)
    for a, b in zip(whole, chunked):
        assert np.array_equal(a, b)
    for i in (0, 2, 4):
        assert np.array_equal(whole[i], chunked_mean[i])


def test_query_alone_or_among_150_to_rounding():
    """150 queries span two query blocks of 128: a query's results alone, in the first and in the second block agree to
    1e-12 relative (the blocks are separate launches of the same forms)."""
    gp, model, X, y, hyp = _problem("matern", 5, "const")
    xs = np.random.default_rng(15).uniform(-2, 2, (150, X.shape[1]))
    whole = gp.predict_hess(xs, separate_samples=True)
    for j in (0, 127, 128, 149):
        one = gp.predict_hess(xs[j:j + 1], separate_samples=True)
        for a, b in zip(one, whole):
            assert np.abs(a[0] - b[j]).max() <= 1e-12 * np.abs(b[j]).max(), j


def test_mean_only_mode():
    """compute_var=False: Hmu, mu and dmu carry the same bits, the variance outputs are None, and no product is timed
    (gpc_last_timing's ms_factor is 0, with the timing events on; with the variance it is positive)."""
    gp, model, X, y, hyp = _problem("matern", 5, "negquad")
    xs = np.random.default_rng(16).uniform(-2, 2, (150, X.shape[1]))
    c = gp._post_handle.ctx
    c.set_option("small_timing", 1)
    try:
        for sep in (True, False):
            full = gp.predict_hess(xs, separate_samples=sep)
            assert c.last_timing()[1] > 0
            mean = gp.predict_hess(xs, compute_var=False, separate_samples=sep)
            total, factor = c.last_timing()
            assert factor == 0 and total > 0
            assert mean[1] is None and mean[3] is None and mean[5] is None
            for i in (0, 2, 4):
                assert np.array_equal(mean[i], full[i]), (sep, i)
    finally:
        c.set_option("small_timing", 0)


def test_clamp_zeroes_gradient_and_hessian(monkeypatch):
    """Queries ON the training points of a near-noiseless posterior: wherever the device's variance is <= 0 the clamp
    holds s2 at 0 and ds2 and Hs2 are 0, per sample and (one sample) in the mixture; elsewhere they are the device's.
    Then with the device's variance pushed below 0 on chosen rows, so that the clamp is certain to act."""
    gp, model, X, y, hyp = _lownoise_problem((1e-12,), N=40, D=3)
    h = gp._post_handle
    real = h.predict_hess
    xs = np.concatenate([X[:30], np.random.default_rng(17).uniform(-3, 3, (10, 3))])
    raw = real(xs)

    def check(raw, held):
        mu, s2, dmu, ds2, Hmu, Hs2 = gp.predict_hess(xs, separate_samples=True)
        assert np.all(s2[held] == 0) and np.all(s2 >= 0)
        assert np.all(ds2[held[:, 0]] == 0) and np.all(Hs2[held[:, 0]] == 0)
        assert np.array_equal(ds2[~held[:, 0]], raw[3][~held[:, 0]])
        assert np.array_equal(Hs2[~held[:, 0]], raw[5][~held[:, 0]])
        assert np.all(np.isfinite(Hmu)) and np.all(np.isfinite(Hs2))
        m = gp.predict_hess(xs)
        assert np.array_equal(m[5], Hs2[..., 0]) and np.array_equal(m[3], ds2[..., 0])

    check(raw, raw[1] <= 0)

    def shifted(x, compute_var=True):
        out = list(real(x, compute_var))
        out[1] = out[1].copy()
        out[1][0:5, 0] = -1e-3
        out[1][5, 0] = 0.0
        return tuple(out)

    monkeypatch.setattr(h, "predict_hess", shifted)
    held = raw[1] <= 0
    held[0:6, 0] = True
    check(raw, held)


def test_abi_refusals(ctx):
    import gpyreg_amd as gpr
    from gpyreg_amd import _lib

    rng = np.random.default_rng(0)
    X = rng.uniform(-1, 1, (40, 2))
    y = np.sin(X[:, :1])
    hyp = np.array([[0.0, 0.0, 0.0, np.log(0.1), 0.0]])
    noise = gpr.noise_functions.GaussianNoise(constant_add=True)
    lib = _lib.load()
    p = _lib._ptr
    xs = np.zeros((3, 2))
    o = dict(fmu=np.empty((3, 1)), fs2=np.empty((3, 1)), dfmu=np.empty((3, 2, 1)), dfs2=np.empty((3, 2, 1)),
             hmu=np.empty((3, 2, 2, 1)), hs2=np.empty((3, 2, 2, 1)))

    def raw(gp, M=3, var=1, x=xs, **drop):
        h = gp._post_handle
        a = {k: (None if k in drop else p(v)) for k, v in o.items()}
        rc = lib.gpc_predict_hess(h._h, None if x is None else p(x), M, var, a["fmu"], a["fs2"], a["dfmu"], a["dfs2"],
                                  a["hmu"], a["hs2"])
        return rc, lib.gpc_last_error(h.ctx._h).decode()

    gp = gpr.GP(2, gpr.covariance_functions.SquaredExponential(), gpr.mean_functions.ConstantMean(), noise)
    gp.update(X_new=X, y_new=y, hyp=hyp)
    bad = (-2, "gpc_predict_hess: bad arguments")
    assert raw(gp, M=0) == bad and raw(gp, M=-1) == bad and raw(gp, x=None) == bad
    for k in o:
        assert raw(gp, **{k: True}) == bad, k
    for k in ("fmu", "dfmu", "hmu"):
        assert raw(gp, var=0, **{k: True}) == bad, k
    assert raw(gp, var=0, fs2=True, dfs2=True, hs2=True)[0] == 0  # the variance outputs may be NULL without it
    assert lib.gpc_predict_hess(None, p(xs), 3, 1, *[p(v) for v in o.values()]) == -2
    for cov_obj in (gpr.covariance_functions.Matern(1), gpr.isotropic_covariance_functions.MaternIsotropic(1)):
        g1 = gpr.GP(2, cov_obj, gpr.mean_functions.ConstantMean(), noise)
        g1.update(X_new=X, y_new=y, hyp=hyp[:, :g1.covariance.hyperparameter_count(2) + 2])
        rc, msg = raw(g1)
        assert rc == -2 and msg == "gpc_predict_hess: the Matern kernel of degree 1 has no second derivative with " \
                                   "respect to x*"
        with pytest.raises(NotImplementedError, match="degree 1"):
            g1.predict_hess(xs)
    from test_gpu_user_kernel import PySquaredExponential

    gk = gpr.GP(2, PySquaredExponential(), gpr.mean_functions.ConstantMean(), noise)
    gk.update(X_new=X, y_new=y, hyp=hyp)
    rc, msg = raw(gk)
    assert rc == -2 and msg.startswith("gpc_predict_hess: this posterior was built from caller-provided K")
    with pytest.raises(NotImplementedError, match="predict_hess: .*PySquaredExponential"):
        gk.predict_hess(xs)

    class MyMean(gpr.mean_functions.ConstantMean):
        pass

    gm = gpr.GP(2, gpr.covariance_functions.SquaredExponential(), MyMean(), noise)
    gm.update(X_new=X, y_new=y, hyp=hyp)
    with pytest.raises(NotImplementedError, match="predict_hess: .*MyMean"):
        gm.predict_hess(xs)
    # the hook's own argument checks
    with pytest.raises(RuntimeError, match="gpc_debug_hess_contract: the Matern kernel of degree 1"):
        ctx.debug_hess_contract(1, 1, np.zeros(3), X, xs, np.zeros(40))


def test_failed_factorization_is_refused(ctx):
    """A device-kernel posterior batch that holds a failed factorization (K - 1e12 I is not positive definite at any
    jitter multiplier: info != 0) is refused, with and without the variance."""
    rng = np.random.default_rng(1)
    X = rng.uniform(-1, 1, (40, 2))
    y = np.sin(X[:, :1])
    ctx.set_data(X, y)
    hyp_cov = np.zeros((2, 3))
    handle, mult, lchol, info = ctx.posterior_batch(0, 0, F64, hyp_cov, np.zeros((2, 40)), np.array([[1e-2], [-1e12]]), False)
    try:
        assert info[0] == 0 and info[1] != 0
        for var in (True, False):
            with pytest.raises(RuntimeError, match="gpc_predict_hess: posterior contains a failed factorization"):
                handle.predict_hess(np.zeros((3, 2)), var)
    finally:
        handle.free()


def test_budget_failure_names_the_sizes(monkeypatch):
    gp, model, X, y, hyp = _lownoise_problem((1e-2,), N=100, D=3)
    xs = np.zeros((5, 3))
    monkeypatch.setenv("GPC_MEM_BUDGET_MB", "1")  # one sample with one query block needs > 1 MB at npad = 128, D = 3
    with pytest.raises(RuntimeError, match=r"gpc_predict_hess: the scratch of one sample with one query block \(\d+ bytes: "
                                           r"N_pad = 128, D = 3, block = 128 queries\) exceeds the device memory budget "
                                           r"\(\d+ bytes\)"):
        gp.predict_hess(xs)
    monkeypatch.delenv("GPC_MEM_BUDGET_MB")
    gp.predict_hess(xs)  # and the context is usable afterwards


def test_prior_without_data_on_the_device_classes():
    """No data: the prior -- the mean function's Hessian, Hs2 = 0, s2 the package covariance's own diagonal."""
    import gpyreg_amd as gpr

    D = 2
    gp = gpr.GP(D, gpr.covariance_functions.Matern(5), gpr.mean_functions.NegativeQuadratic(),
                gpr.noise_functions.GaussianNoise(constant_add=True))
    hyp = np.array([[0.1, -0.2, 0.3, np.log(0.1), 1.0, 0.3, -0.4, 0.2, 0.5],
                    [0.0, 0.2, 0.1, np.log(0.1), 0.5, 0.1, 0.4, 0.1, 0.3]])
    gp.update(hyp=hyp)
    xs = np.array([[0.5, 1.0], [-1.0, 2.0], [0.0, 0.0]])
    mu, s2, dmu, ds2, Hmu, Hs2 = gp.predict_hess(xs, separate_samples=True)
    pm, ps2, pdm, pds2 = gp.predict_grad(xs, separate_samples=True)
    assert np.array_equal(mu, pm) and np.array_equal(s2, ps2) and np.array_equal(dmu, pdm) and np.array_equal(ds2, pds2)
    for s in range(2):
        assert np.array_equal(Hmu[..., s], np.broadcast_to(-np.diag(np.exp(-2 * hyp[s, 7:9])), (3, D, D)))
    assert np.all(Hs2 == 0) and Hs2.shape == (3, D, D, 2)
    out = gp.predict_hess(xs)
    assert [o.shape for o in out] == [(3,), (3,), (3, D), (3, D), (3, D, D), (3, D, D)]


# ---- sharding: the pattern of test_gpu_gradient_posterior.py


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
            for kw in (dict(separate_samples=True), dict(), dict(compute_var=False)):
                a = ref.predict_hess(xs, **kw)
                b = gp.predict_hess(xs, **kw)
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
