"""GPU tests of the block append (GP.update(block_append=True), gpc_post_append_block / _K): k new points appended
to the resident posteriors in one device call, against the oracle's full recompute on the extended data (the
reference has no block path: it recomputes) and against the NumPy restatement of tests/test_block_append_cpu.py.
Every parity case also asserts, through the get-only options "block_appended" / "block_stale", that its samples
were appended and did not reach the expected values through the per-sample fallback."""

import os
import socket
import sys

import numpy as np
import pytest

from oracle import gp_oracle as orc
from test_block_append_cpu import golden, new_rows, parse

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _counts():
    from gpyreg_amd import _lib

    ctx = _lib.context(0)
    return ctx.get_option("block_appended"), ctx.get_option("block_stale")


def _check_against_oracle(gp, model, hyp, X2, y2, xs, name, tol=1e-8):
    full = orc.posteriors(model, hyp, X2, y2, None)
    rm, rs = orc.predict(model, full, X2, y2, xs, separate_samples=True)
    mu, s2 = gp.predict(xs, separate_samples=True)
    assert np.abs(mu - rm).max() <= tol * max(1.0, np.abs(rm).max()), (name, "mu", np.abs(mu - rm).max())
    assert np.abs(s2 - rs).max() <= tol * max(1.0, np.abs(rs).max()), (name, "s2", np.abs(s2 - rs).max())
    N2 = X2.shape[0]
    for s, (p, f) in enumerate(zip(gp.posteriors, full)):
        assert p.alpha.shape == (N2, 1) and p.sW.shape == (N2, 1) and p.L.shape == (N2, N2), (name, s)
        assert np.abs(p.alpha - f.alpha).max() <= tol * np.abs(f.alpha).max(), (name, s, "alpha")
        assert np.abs(np.asarray(p.L) - f.L).max() <= tol * np.abs(f.L).max(), (name, s, "L")
        assert np.allclose(p.sW, f.sW, rtol=1e-12), (name, s, "sW")
        assert bool(p.L_chol) == bool(f.L_chol) and p.sn2_mult == f.sn2_mult, (name, s)
    return full


@pytest.mark.parametrize("k", [3, 40, 200])
def test_block_append_matches_the_full_recompute_on_every_fixture_model(k):
    """n = 126, 127, 128 cross a tile boundary and grow the storage by one (k = 3, 40) and two (k = 200) tiles; both
    parametrisations; every kernel family of the fixture."""
    from test_gpu_api import _gp as mk

    g = golden()
    for name in g["names"]:
        tag, model, N, D, flav = parse(name)
        X, y, hyp, xs = g[tag + "_X"], g[tag + "_y"], g[tag + "_hyp"], g[tag + "_xs"]
        Xn, yn = new_rows(g, tag, k)
        gp = mk(model, D)
        gp.update(X_new=X, y_new=y, hyp=hyp)
        h0 = gp._post_handle
        a0, s0 = _counts()
        gp.update(X_new=Xn, y_new=yn, block_append=True)
        a1, s1 = _counts()
        assert gp._post_handle is h0, (name, "the resident posteriors must be extended, not rebuilt")
        assert (a1 - a0, s1 - s0) == (hyp.shape[0], 0), (name, "every sample must be appended, none recomputed")
        assert gp.X.shape[0] == N + k and h0.N == N + k
        assert all(bool(p.L_chol) == (flav == "high") for p in gp.posteriors)
        _check_against_oracle(gp, model, hyp, np.concatenate([X, Xn]), np.concatenate([y, yn]), xs, (name, k))


def _mk(kernel="se", dtype="float64"):
    import gpyreg_amd as gpr

    cov = gpr.covariance_functions.SquaredExponential() if kernel == "se" else gpr.covariance_functions.Matern(5)
    return gpr.GP(2, cov, gpr.mean_functions.ConstantMean(), gpr.noise_functions.GaussianNoise(constant_add=True),
                  dtype=dtype)


def _data(N, seed):  # (the seeded data of test_gpu_rank1.py)
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, 2))
    y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
    hyp = np.array([[0.1, -0.1, 0.05, np.log(0.2), 0.1], [0.3, 0.2, -0.1, np.log(0.1), -0.2]])
    return X, y, hyp


def _model(kernel):
    return dict(kernel="se" if kernel == "se" else "matern", degree=0 if kernel == "se" else 5, mean="const",
                noise=(1, 0, 0))


def _property(inc, one_go, model, hyp, X, y, xs, start):
    N = X.shape[0]
    inc.update(X_new=X[:start], y_new=y[:start], hyp=hyp)
    h0 = inc._post_handle
    a0, s0 = _counts()
    inc.update(X_new=X[start:], y_new=y[start:], block_append=True)
    a1, s1 = _counts()
    assert inc._post_handle is h0 and (a1 - a0, s1 - s0) == (hyp.shape[0], 0)
    assert np.array_equal(inc.X, X) and np.array_equal(inc.y, y)
    full = orc.posteriors(model, hyp, X, y, None)
    for a, b in zip(inc.posteriors, full):
        assert np.array_equal(a.hyp, b.hyp) and a.sn2_mult == b.sn2_mult == 1 and a.L_chol and b.L_chol
        assert a.alpha.shape == (N, 1) and a.L.shape == (N, N) and a.sW.shape == (N, 1)
        assert np.allclose(a.alpha, b.alpha, rtol=1e-7, atol=1e-9 * np.abs(b.alpha).max())
        assert np.allclose(a.sW, b.sW, rtol=1e-12)
        assert np.allclose(a.L, b.L, rtol=1e-8, atol=1e-10)
    m1, v1 = inc.predict(xs, separate_samples=True)
    m2, v2 = orc.predict(model, full, X, y, xs, separate_samples=True)
    assert np.allclose(m1, m2, atol=1e-8) and np.allclose(v1, v2, atol=1e-8)
    one_go.update(X_new=X, y_new=y, hyp=hyp)
    n1, g1 = inc.nll_batch(hyp, compute_grad=True)  # (does not use the posteriors: the same bits)
    n2, g2 = one_go.nll_batch(hyp, compute_grad=True)
    assert np.array_equal(n1, n2) and np.array_equal(g1, g2)


@pytest.mark.parametrize("N,start,kernel", [(20, 10, "se"), (140, 120, "matern5"), (260, 255, "se"), (700, 100, "se")])
def test_one_block_append_equals_the_full_recompute(N, start, kernel):
    X, y, hyp = _data(N, N)
    xs = np.random.default_rng(1).standard_normal((30, 2))
    _property(_mk(kernel), _mk(kernel), _model(kernel), hyp, X, y, xs, start)


@pytest.mark.parametrize("N,start", [(2100, 1500), (2048, 2043)])
def test_block_append_at_benchmark_scale(N, start):
    """The benchmark's problem (D = 10, Matern-5) with S = 2: 600 rows at once, and 5 rows across a tile boundary."""
    from test_gpu_api import _gp as mk

    model, X, y, hyp = orc.synthetic_problem(3, N=N, S=2)
    _property(mk(model, X.shape[1]), mk(model, X.shape[1]), model, hyp, X, y, X[:30] + 0.05, start)


@pytest.mark.parametrize("engine", [1, 2])
def test_both_engines_of_the_products_with_W_agree_with_the_oracle(engine):
    """The skinny kernel (1) and the padded MFMA GEMM (2), forced through the test option "block_engine", on the same
    inputs: k = 40 on every fixture model (both parametrisations) and 1500 + 600 at benchmark scale."""
    from gpyreg_amd import _lib
    from test_gpu_api import _gp as mk

    ctx = _lib.context(0)
    ctx.set_option("block_engine", engine)
    try:
        assert ctx.get_option("block_engine") == engine
        g = golden()
        for name in g["names"]:
            tag, model, N, D, flav = parse(name)
            X, y, hyp, xs = g[tag + "_X"], g[tag + "_y"], g[tag + "_hyp"], g[tag + "_xs"]
            Xn, yn = new_rows(g, tag, 40)
            gp = mk(model, D)
            gp.update(X_new=X, y_new=y, hyp=hyp)
            h0 = gp._post_handle
            a0, s0 = _counts()
            gp.update(X_new=Xn, y_new=yn, block_append=True)
            a1, s1 = _counts()
            assert gp._post_handle is h0 and (a1 - a0, s1 - s0) == (hyp.shape[0], 0), name
            _check_against_oracle(gp, model, hyp, np.concatenate([X, Xn]), np.concatenate([y, yn]), xs, (name, engine))
        model, X, y, hyp = orc.synthetic_problem(3, N=2100, S=2)
        _property(mk(model, X.shape[1]), mk(model, X.shape[1]), model, hyp, X, y, X[:30] + 0.05, 1500)
    finally:
        ctx.set_option("block_engine", 0)


def test_a_sample_declared_unstable_is_recomputed_alone():
    from gpyreg_amd import _lib
    from test_gpu_api import _gp as mk

    g = golden()
    ctx = _lib.context(0)
    ran = 0
    for name in g["names"]:
        tag, model, N, D, flav = parse(name)
        if N not in (33, 128):
            continue
        ran += 1
        X, y, hyp, xs = g[tag + "_X"], g[tag + "_y"], g[tag + "_hyp"], g[tag + "_xs"]
        assert hyp.shape[0] == 3
        Xn, yn = g[tag + "_Xn"], g[tag + "_yn"]
        gp = mk(model, D)
        gp.update(X_new=X, y_new=y, hyp=hyp)
        h0 = gp._post_handle
        a0, s0 = _counts()
        ctx.set_option("append_fail_mask", 0b010)
        try:
            gp.update(X_new=Xn, y_new=yn, block_append=True)
        finally:
            ctx.set_option("append_fail_mask", 0)
        a1, s1 = _counts()
        assert gp._post_handle is h0 and (a1 - a0, s1 - s0) == (2, 1), name
        # sample 1: the full recompute; samples 0 and 2: the appended values -- all equal the oracle's full recompute
        _check_against_oracle(gp, model, hyp, np.concatenate([X, Xn]), np.concatenate([y, yn]), xs, name)
    assert ran >= 1


def _py_se_gp():
    import gpyreg_amd as gpr
    from test_gpu_user_kernel import PySquaredExponential

    gp = gpr.GP(2, PySquaredExponential(), gpr.mean_functions.ConstantMean(),
                gpr.noise_functions.GaussianNoise(constant_add=True))
    assert not gp._builtin
    return gp


def test_a_block_unstable_by_construction_is_left_stale_and_recomputed():
    """Through append_block_K with the true cross covariances of new points that COINCIDE with training points and
    Kss = 0: every diagonal entry of the Schur complement is 1 - |W b_j|^2 / sl^2 < 0 (about -26 and -81 for the two
    hyperparameter rows), not a matter of rounding.  ok is all 0, nothing non-finite reaches alpha / A / W, and
    recompute_K with the true K gives the oracle's full recompute."""
    N, k = 60, 4
    X, y, hyp = _data(N, N)
    model = _model("se")
    gp = _py_se_gp()
    gp.update(X_new=X, y_new=y, hyp=hyp)
    h = gp._post_handle
    cov = gp.covariance
    Xn, yn = X[:k].copy(), y[:k] + 0.05
    Ks = np.stack([cov.compute(hh[:3], X, Xn) for hh in hyp])
    Kss = np.zeros((2, k, k))
    # the Schur diagonal on the CPU
    for s, hh in enumerate(hyp):
        sl = np.exp(2 * hh[3])
        A = cov.compute(hh[:3], X) / sl + np.eye(N)
        d = 1.0 - np.einsum("ij,ij->j", Ks[s], np.linalg.solve(A, Ks[s])) / sl**2
        assert d.max() < -10.0, d
    old = [h.fetch(s) for s in range(2)]
    X2, y2 = np.concatenate([X, Xn]), np.concatenate([y, yn])
    gp.X, gp.y = X2, y2
    gp._token = None
    gp._ctx()  # uploads the extended data
    a0, s0 = _counts()
    ok = h.append_block_K(Ks, Kss, np.tile(hyp[:, 4:5], (1, k)), np.exp(2 * hyp[:, 3]), yn)
    a1, s1 = _counts()
    assert not ok.any() and (a1 - a0, s1 - s0) == (0, 2) and h.N == N + k
    for s in range(2):  # stale: the old rows untouched, the new ones the identity padding -- and finite
        al, sw, L = h.fetch(s)
        assert np.isfinite(al).all() and np.isfinite(L).all()
        assert np.array_equal(al[:N], old[s][0]) and np.array_equal(L[:N, :N], old[s][2])
    pv = gp._plugin_values(hyp, False)
    K = gp._user_cov(hyp[:, :3], False)[0]
    mult, lchol, info = h.recompute(np.arange(2), hyp[:, :3], pv["m"], pv["sn2"], pv["vec"], K=K)
    assert (info == 0).all()
    full = orc.posteriors(model, hyp, X2, y2, None)
    for s in range(2):
        al, sw, L = h.fetch(s)
        assert mult[s] == full[s].sn2_mult and bool(lchol[s]) == bool(full[s].L_chol)
        assert np.abs(al - full[s].alpha[:, 0]).max() <= 1e-8 * np.abs(full[s].alpha).max()
        Lp = L.T if lchol[s] else L  # (the device holds the lower factor, the record SciPy's upper one)
        assert np.abs(Lp - full[s].L).max() <= 1e-8 * np.abs(full[s].L).max()
    # W (the inverse factor, which no fetch returns) enters every predictive variance: finite and right
    for p, f, m, lc in zip(gp.posteriors, full, mult, lchol):
        p.sn2_mult, p.L_chol = f.sn2_mult, bool(lc)
        p._alpha = p._sW = p._L = None
        p._have = {"alpha": False, "sW": False, "L": False}
    xs = np.random.default_rng(8).standard_normal((25, 2))
    mu, s2 = gp.predict(xs, separate_samples=True)
    rm, rs = orc.predict(model, full, X2, y2, xs, separate_samples=True)
    assert np.isfinite(mu).all() and np.isfinite(s2).all()
    assert np.abs(mu - rm).max() <= 1e-8 * max(1.0, np.abs(rm).max())
    assert np.abs(s2 - rs).max() <= 1e-8 * max(1.0, np.abs(rs).max())


def test_block_append_with_a_user_defined_kernel():
    """A Python SE kernel (cross covariances from its own compute(), gpc_post_append_block_K) against the oracle's
    full recompute of the built-in SE fixtures, and the per-sample fallback from the object's own K."""
    import gpyreg_amd as gpr
    from gpyreg_amd import _lib
    from test_gpu_user_kernel import PySquaredExponential

    g = golden()
    ctx = _lib.context(0)
    ran = 0
    for name in g["names"]:
        tag, model, N, D, flav = parse(name)
        if model["kernel"] != "se" or model["noise"] != (1, 0, 0):
            continue
        ran += 1
        Mean = {"const": gpr.mean_functions.ConstantMean, "negquad": gpr.mean_functions.NegativeQuadratic,
                "zero": gpr.mean_functions.ZeroMean}[model["mean"]]
        X, y, hyp, xs = g[tag + "_X"], g[tag + "_y"], g[tag + "_hyp"], g[tag + "_xs"]
        for k, mask, want in ((3, 0, (hyp.shape[0], 0)), (40, 0b010, (hyp.shape[0] - 1, 1))):
            Xn, yn = new_rows(g, tag, k)
            gp = gpr.GP(D, PySquaredExponential(), Mean(), gpr.noise_functions.GaussianNoise(constant_add=True))
            assert not gp._builtin
            gp.update(X_new=X, y_new=y, hyp=hyp)
            h0 = gp._post_handle
            a0, s0 = _counts()
            ctx.set_option("append_fail_mask", mask)
            try:
                gp.update(X_new=Xn, y_new=yn, block_append=True)
            finally:
                ctx.set_option("append_fail_mask", 0)
            a1, s1 = _counts()
            assert gp._post_handle is h0 and (a1 - a0, s1 - s0) == want, (name, k)
            _check_against_oracle(gp, model, hyp, np.concatenate([X, Xn]), np.concatenate([y, yn]), xs, (name, k))
    assert ran >= 2


@pytest.mark.parametrize("k,engine", [(3, 0), (12, 0), (40, 1), (40, 2)])
def test_block_append_of_fp32_posteriors(k, engine):
    """fp32 posteriors append in fp32: predictions within 1e-3 of the fp64 oracle (the project's fp32 figure) on every
    fixture model, every sample appended and none recomputed.  k = 3 and 12 run the skinny kernel's float
    instantiations (k <= 16), k = 40 both engines forced.  The oracle escalates the jitter exactly like the device
    does in fp64; where fp32 settles on another (sn2_mult, L_chol) than the oracle, the expected values are the
    oracle's at the multiplier the device settled on (``force_mult``) -- no model is left out."""
    from gpyreg_amd import _lib
    from test_gpu_api import _gp as mk

    ctx = _lib.context(0)
    g = golden()
    ctx.set_option("block_engine", engine)
    try:
        for name in g["names"]:
            tag, model, N, D, flav = parse(name)
            X, y, hyp, xs = g[tag + "_X"], g[tag + "_y"], g[tag + "_hyp"], g[tag + "_xs"]
            Xn, yn = new_rows(g, tag, k)
            gp = mk(model, D, dtype="float32")
            gp.update(X_new=X, y_new=y, hyp=hyp)
            h0 = gp._post_handle
            a0, s0 = _counts()
            gp.update(X_new=Xn, y_new=yn, block_append=True)
            a1, s1 = _counts()
            assert gp._post_handle is h0 and h0.N == N + k, name
            assert (a1 - a0, s1 - s0) == (hyp.shape[0], 0), (name, "every fp32 sample must be appended, none recomputed")
            X2, y2 = np.concatenate([X, Xn]), np.concatenate([y, yn])
            full = orc.posteriors(model, hyp, X2, y2, None)
            for s, p in enumerate(gp.posteriors):
                if p.sn2_mult != full[s].sn2_mult:
                    full[s] = orc.core(model, hyp[s], X2, y2, None, 0, 0, force_mult=p.sn2_mult)
                assert bool(p.L_chol) == bool(full[s].L_chol), (name, s)
            rm, rs = orc.predict(model, full, X2, y2, xs, separate_samples=True)
            mu, s2 = gp.predict(xs, separate_samples=True)
            assert np.abs(mu - rm).max() <= 1e-3 * max(1.0, np.abs(rm).max()), (name, np.abs(mu - rm).max())
            assert np.abs(s2 - rs).max() <= 1e-3 * max(1.0, np.abs(rs).max()), (name, np.abs(s2 - rs).max())
    finally:
        ctx.set_option("block_engine", 0)


def _budget_worker(budget_mb, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        from gpyreg_amd import _lib

        N, k, S = 700, 100, 5
        X, y, _ = _data(N + k, 3)
        rng = np.random.default_rng(4)
        hyp = np.array([0.1, -0.1, 0.05, np.log(0.2), 0.1]) + 0.05 * rng.standard_normal((S, 5))
        gp = _mk("matern5")
        gp.update(X_new=X[:N], y_new=y[:N], hyp=hyp)
        ctx = _lib.context(0)
        a0, s0 = ctx.get_option("block_appended"), ctx.get_option("block_stale")
        os.environ["GPC_MEM_BUDGET_MB"] = str(budget_mb)  # (the library reads it at every call: the append alone is budgeted)
        try:
            gp.update(X_new=X[N:], y_new=y[N:], block_append=True)
        except Exception as e:  # noqa: BLE001
            q.put(dict(error=str(e)))
            return
        finally:
            del os.environ["GPC_MEM_BUDGET_MB"]
        chunk = ctx.get_option("last_chunk")
        mu, s2 = gp.predict(X[:20] + 0.05, separate_samples=True)
        q.put(dict(chunk=chunk, mu=mu, s2=s2, alpha=[p.alpha for p in gp.posteriors], L=[np.asarray(p.L) for p in gp.posteriors],
                   counts=(ctx.get_option("block_appended") - a0, ctx.get_option("block_stale") - s0)))
    except Exception:  # noqa: BLE001
        import traceback

        q.put(dict(exception=traceback.format_exc()))


def _run_budgeted(budget_mb):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_budget_worker, args=(budget_mb, q))
    p.start()
    r = q.get(timeout=300)
    p.join(60)
    assert p.exitcode == 0
    assert "exception" not in r, r.get("exception")
    return r


def test_scratch_budget_chunks_over_the_samples_and_refuses_one_sample_that_does_not_fit():
    """GPC_MEM_BUDGET_MB (set in a fresh child process, for the append alone) budgets the scratch.  N = 700 + 100 in fp64
    with the MFMA engine needs 4 x 896 x 112 x 8 + 3 x 896 x 128 x 8 + ... = 6.5 MB per sample, and 80 % of the budget
    is used: 20 MB hold two samples of five (chunks of 2, 2, 1), 4 MB hold none.  The chunked result carries the bits of the unchunked one, and the refusal
    names the sizes."""
    big, small = _run_budgeted(4096), _run_budgeted(20)
    assert "error" not in big and "error" not in small, (big.get("error"), small.get("error"))
    assert big["counts"] == (5, 0) and small["counts"] == (5, 0)
    from scratch_sizes import append_block_per, planned_chunk

    want = planned_chunk(5, 20, append_block_per(896, 100, 8, 2))  # (k = 100: the MFMA engine)
    assert (big["chunk"], small["chunk"]) == (5, want) and want == 2, (big["chunk"], small["chunk"], want)
    assert np.array_equal(big["mu"], small["mu"]) and np.array_equal(big["s2"], small["s2"])
    for a, b in zip(big["alpha"] + big["L"], small["alpha"] + small["L"]):
        assert np.array_equal(a, b)
    model = _model("matern5")
    X, y, _ = _data(800, 3)
    hyp = np.array([0.1, -0.1, 0.05, np.log(0.2), 0.1]) + 0.05 * np.random.default_rng(4).standard_normal((5, 5))
    full = orc.posteriors(model, hyp, X, y, None)
    rm, rs = orc.predict(model, full, X, y, X[:20] + 0.05, separate_samples=True)
    assert np.allclose(small["mu"], rm, atol=1e-8) and np.allclose(small["s2"], rs, atol=1e-8)
    none = _run_budgeted(4)
    assert "error" in none, none.keys()
    assert "gpc_post_append_block" in none["error"] and "exceeds the device memory budget" in none["error"], none["error"]
    assert "N_pad = 896" in none["error"] and "k = 100" in none["error"], none["error"]


def _bits(gp, xs):
    out = list(gp.predict(xs, separate_samples=True))
    for p in gp.posteriors:
        out += [p.alpha, np.asarray(p.L), p.sW, np.array([float(p.sn2_mult), float(p.L_chol)])]
    return out


def test_the_keyword_changes_nothing_where_the_block_path_does_not_apply():
    X, y, hyp = _data(40, 7)
    xs = np.random.default_rng(2).standard_normal((10, 2))
    # k = 1: the rank-one path, same bits
    a, b = _mk(), _mk()
    for gp, kw in ((a, {}), (b, {"block_append": True})):
        gp.update(X_new=X[:39], y_new=y[:39], hyp=hyp)
        h0 = gp._post_handle
        gp.update(X_new=X[39:], y_new=y[39:], **kw)
        assert gp._post_handle is h0
    assert all(np.array_equal(u, v) for u, v in zip(_bits(a, xs), _bits(b, xs)))
    # new hyperparameters with the points: the full recompute, same bits
    a, b = _mk(), _mk()
    for gp, kw in ((a, {}), (b, {"block_append": True})):
        gp.update(X_new=X[:30], y_new=y[:30], hyp=hyp)
        h0 = gp._post_handle
        gp.update(X_new=X[30:], y_new=y[30:], hyp=hyp + 0.01, **kw)
        assert gp._post_handle is not h0
    assert all(np.array_equal(u, v) for u, v in zip(_bits(a, xs), _bits(b, xs)))
    # user-provided noise for the new points: the full recompute, same bits
    import gpyreg_amd as gpr

    def mk2():
        return gpr.GP(2, gpr.covariance_functions.SquaredExponential(), gpr.mean_functions.ConstantMean(),
                      gpr.noise_functions.GaussianNoise(constant_add=True, user_provided_add=True))

    s2 = np.full((40, 1), 0.01)
    a, b = mk2(), mk2()
    for gp, kw in ((a, {}), (b, {"block_append": True})):
        gp.update(X_new=X[:30], y_new=y[:30], s2_new=s2[:30], hyp=hyp)
        h0 = gp._post_handle
        gp.update(X_new=X[30:], y_new=y[30:], s2_new=s2[30:], **kw)
        assert gp._post_handle is not h0
    assert all(np.array_equal(u, v) for u, v in zip(_bits(a, xs), _bits(b, xs)))


def test_appends_of_both_kinds_in_turn_then_every_predictor():
    """Block append, one-point append, block append on one GP; predict, predict_full, predict_cov and draw_functions
    afterwards match a GP built in one go (the device-resident constants must have been refreshed)."""
    N = 300
    X, y, hyp = _data(N, 11)
    xs = np.random.default_rng(3).standard_normal((12, 2))
    inc, ref = _mk("matern5"), _mk("matern5")
    inc.update(X_new=X[:120], y_new=y[:120], hyp=hyp)
    h0 = inc._post_handle
    inc.predict(xs)  # (puts the constants of the 120-point posterior on the device)
    inc.update(X_new=X[120:130], y_new=y[120:130], block_append=True)
    assert inc._post_handle is h0
    inc.predict(xs)
    inc.update(X_new=X[130:131], y_new=y[130:131])
    inc.update(X_new=X[131:], y_new=y[131:], block_append=True)
    assert inc._post_handle is h0 and h0.N == N
    ref.update(X_new=X, y_new=y, hyp=hyp)
    model = _model("matern5")
    _check_against_oracle(inc, model, hyp, X, y, xs, "chain")
    for a, b in zip(inc.predict(xs, separate_samples=True), ref.predict(xs, separate_samples=True)):
        assert np.abs(a - b).max() <= 1e-8 * max(1.0, np.abs(b).max())
    for a, b in zip(inc.predict_full(xs), ref.predict_full(xs)):
        assert np.abs(a - b).max() <= 1e-8 * max(1.0, np.abs(b).max())
    a, b = inc.predict_cov(xs[:5], xs[5:]), ref.predict_cov(xs[:5], xs[5:])
    assert np.abs(a - b).max() <= 1e-8 * max(1.0, np.abs(b).max())
    a, b = inc.draw_functions(xs, n_draws=3, seed=5), ref.draw_functions(xs, n_draws=3, seed=5)
    assert np.abs(a - b).max() <= 1e-8 * max(1.0, np.abs(b).max())


def test_refusals_of_the_entry_point():
    from gpyreg_amd import _lib

    X, y, hyp = _data(30, 5)
    gp = _mk()
    gp.update(X_new=X[:20], y_new=y[:20], hyp=hyp)
    h = gp._post_handle
    S = hyp.shape[0]
    sn2 = np.exp(2 * hyp[:, 3])
    for k, needle in ((0, "k must be at least 1"), (3, "extended"), (_lib.load().gpc_max_n(_lib.F64), "gpc_max_n")):
        with pytest.raises(Exception) as e:
            h.append_block(np.zeros((S, k)), sn2, np.zeros(k))
        assert needle in str(e.value), (k, str(e.value))
        assert h.N == 20
    mu, _ = gp.predict(X[:3])  # the posteriors are unharmed
    assert np.isfinite(mu).all()


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
    from gpyreg_amd import sharding

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        bench.CONFIGS[3] = dict(bench.CONFIGS[3], N=700)
        S, k = 5, 9
        X, y, hyp = bench.synthetic_problem(3, S)
        xs = X[:40] + 0.05
        ref = bench.make_gp(3, "f64")
        ref.shard = False  # rank-local: the unsharded answer
        ref.update(X_new=X[:-k], y_new=y[:-k], hyp=hyp)
        ref.update(X_new=X[-k:], y_new=y[-k:], block_append=True)
        gp = bench.make_gp(3, "f64")
        gp.update(X_new=X[:-k], y_new=y[:-k], hyp=hyp)
        h0 = gp._post_handle
        gp.update(X_new=X[-k:], y_new=y[-k:], block_append=True)
        lo, hi = sharding.shard_bounds(S, rank, world)
        mu, s2 = gp.predict(xs, separate_samples=True)
        rmu, rs2 = ref.predict(xs, separate_samples=True)
        q.put((rank, dict(
            kept=bool(gp._post_handle is h0 and gp._post_range == (lo, hi, S) and h0.N == X.shape[0]),
            ref_kept=bool(ref._post_handle.N == X.shape[0]),
            pred=bool(np.array_equal(mu, rmu) and np.array_equal(s2, rs2)),
            flags=bool(all(a.sn2_mult == b.sn2_mult and a.L_chol == b.L_chol
                           for a, b in zip(gp.posteriors, ref.posteriors))),
            alpha=bool(all(np.array_equal(gp.posteriors[i].alpha, ref.posteriors[i].alpha) for i in range(lo, hi))))))
    except Exception:  # noqa: BLE001
        import traceback

        q.put((rank, {"exception": traceback.format_exc()}))
    finally:
        dist.destroy_process_group()


def test_sharded_block_append_equals_the_unsharded_one_bitwise():
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
        assert all(r.values()), (rank, r)
