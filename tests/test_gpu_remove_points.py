"""GPU tests of the point removal (GP.remove_points, gpc_post_remove): the panel and the apply kernel alone against
the NumPy restatement (gpyreg_amd/_remove.py), and the whole call against the ORACLE's recompute on the reduced data
(never the library's own), through gpc_post_fetch and through the posterior consumers.  Tolerances are the project's:
1e-8 relative in fp64, 1e-3 in fp32.  Every parity case also asserts through the get-only options "removed" /
"remove_stale" that its samples took the fast path and did not reach the expected values through the fallback."""

import os

import numpy as np
import pytest

from gpyreg_amd import _remove as rm
from oracle import gp_oracle as orc
from test_block_append_cpu import golden, parse
from test_gpu_block_append import _data, _mk, _model, _py_se_gp

pytestmark = pytest.mark.gpu


def _ctx():
    from gpyreg_amd import _lib

    return _lib.context(0)


@pytest.fixture(autouse=True)
def _sweep_whatever_the_length():
    """GP.remove_points gives the device path only sweeps of at most RM_SWEEP_MAX_PANELS panels that keep more than
    RM_MIN_KEPT_ROWS rows (the rest loses to the recompute, remove.h); the tests are about the device path: the test
    option lifts both limits.  The production routing is the subject of one test below."""
    _ctx().set_option("remove_force", 1)
    yield
    _ctx().set_option("remove_force", 0)


def _counts():
    ctx = _ctx()
    return ctx.get_option("removed"), ctx.get_option("remove_stale")


def _rel(a, ref):
    return np.abs(np.asarray(a) - np.asarray(ref)).max() / max(np.abs(ref).max(), 1e-300)


def _orth(t):
    return np.abs(t.T @ t - np.eye(t.shape[0])).sum(1).max()


# ---- the panel kernel alone ----------------------------------------------------------------------------------------
def _panel_inputs(k, zero_rows=0, seed=0):
    rng = np.random.default_rng(100 * k + seed)
    D = np.tril(rng.standard_normal((64, 64))) + 8.0 * np.eye(64)
    Vp = rng.standard_normal((64, k))
    Vp[:zero_rows] = 0.0
    return D, Vp


@pytest.mark.parametrize("k,zero_rows", [(1, 0), (16, 0), (17, 0), (64, 0), (5, 20)])
def test_panel_kernel_equals_the_restatement(k, zero_rows):
    """k on both sides of a 16-boundary of Theta's padded order and the largest; a carrier whose first 20 rows are
    zero, as when only some of the removed rows lie above the panel (those reflections are the identity)."""
    D, Vp = _panel_inputs(k, zero_rows)
    theta, Dn = _ctx().debug_remove_panel(D, Vp)
    rt, rD = rm.panel_theta(D, Vp)
    scale = np.abs(D).max()
    print("k = %d: Theta %.3g, D' %.3g, orthogonality %.3g" % (k, np.abs(theta - rt).max(), np.abs(Dn - rD).max() / scale,
                                                               _orth(theta)))
    # both are backward-stable Householder constructions of the same reflections in fp64, summed in different orders:
    # 64 + k terms of size <= 1 per entry, a few ulp each
    assert np.abs(theta - rt).max() <= 1e-12
    assert np.abs(Dn - rD).max() <= 1e-12 * scale
    assert _orth(theta) <= 1e-12
    assert np.array_equal(Dn, np.tril(Dn)) and np.all(np.diag(Dn) > 0)
    out = np.hstack([D, Vp]) @ theta
    assert np.abs(out[:, :64] - Dn).max() <= 1e-12 * scale and np.abs(out[:, 64:]).max() <= 1e-12 * scale
    if zero_rows:
        assert np.array_equal(Dn[:zero_rows], D[:zero_rows])
        assert np.array_equal(theta[:zero_rows, :zero_rows], np.eye(zero_rows))


def test_panel_kernel_on_an_identity_block_with_a_zero_carrier_is_the_identity_exactly():
    theta, Dn = _ctx().debug_remove_panel(np.eye(64), np.zeros((64, 7)))
    assert np.array_equal(theta, np.eye(71)) and np.array_equal(Dn, np.eye(64))


def test_panel_kernel_in_fp32_storage_reads_and_writes_the_cast_block():
    from gpyreg_amd import _lib

    D, Vp = _panel_inputs(9)
    theta, Dn = _ctx().debug_remove_panel(D, Vp, dtype=_lib.F32)
    D32 = D.astype(np.float32).astype(np.float64)
    rt, rD = rm.panel_theta(D32, Vp)
    assert np.abs(theta - rt).max() <= 1e-12 and _orth(theta) <= 1e-12
    assert np.array_equal(Dn, Dn.astype(np.float32).astype(np.float64))
    assert np.abs(Dn - rD).max() <= 2.0**-23 * np.abs(rD).max()  # one fp32 rounding of the fp64 result


# ---- the apply kernel alone ----------------------------------------------------------------------------------------
def _random_theta(k, seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((64 + k, 64 + k)))
    return q


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("k,a,rows", [(1, 0, 1), (16, 64, 100), (17, 0, 64), (64, 128, 131)])
def test_apply_kernel_L_side_equals_numpy(dtype, k, a, rows):
    """[P | Cr] Theta on rows below the panel: one row, a multiple of 64, and counts that are none (two and three
    blocks); fp64 accumulation whatever the storage."""
    from gpyreg_amd import _lib

    rng = np.random.default_rng(k + rows)
    theta = _random_theta(k, k)
    P, Cr = rng.standard_normal((rows, 64)), rng.standard_normal((rows, k))
    f32 = dtype == "f32"
    P2, C2 = _ctx().debug_remove_apply("L", a, theta, P, Cr, dtype=_lib.F32 if f32 else _lib.F64)
    Pin = P.astype(np.float32).astype(np.float64) if f32 else P
    ref = np.hstack([Pin, Cr]) @ theta
    # 64 + k <= 128 products of entries of size ~1 with |Theta| <= 1, accumulated in fp64: 128 ulp of the largest entry
    tol = 128 * 2.0**-52 * np.abs(ref).max()
    assert np.abs(C2 - ref[:, 64:]).max() <= tol
    if f32:
        assert np.array_equal(P2, P2.astype(np.float32).astype(np.float64))
        assert np.abs(P2 - ref[:, :64]).max() <= tol + 2.0**-24 * np.abs(ref).max()  # + the store's rounding
    else:
        assert np.abs(P2 - ref[:, :64]).max() <= tol


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("k,a,n", [(1, 0, 64), (16, 64, 128), (17, 64, 100), (64, 128, 259), (5, 0, 30)])
def test_apply_kernel_W_side_equals_numpy(dtype, k, a, n):
    """Theta^T [W[a:a+64, :n] ; C]: column counts that are and are not multiples of 64, a last panel that is cut by n
    (its rows >= n are neither read nor written), C updated over all n columns, W on and below the diagonal only."""
    from gpyreg_amd import _lib

    rng = np.random.default_rng(k + n)
    theta = _random_theta(k, k + 1)
    rows = np.arange(a, a + 64)
    live = (np.arange(n)[None, :] <= rows[:, None]) & (rows[:, None] < n)
    P = rng.standard_normal((64, n))
    Cr = rng.standard_normal((k, n))
    f32 = dtype == "f32"
    P2, C2 = _ctx().debug_remove_apply("W", a, theta, P, Cr, dtype=_lib.F32 if f32 else _lib.F64)
    Pin = np.where(live, P.astype(np.float32).astype(np.float64) if f32 else P, 0.0)
    ref = theta.T @ np.vstack([Pin, Cr])
    tol = 128 * 2.0**-52 * np.abs(ref).max()
    assert np.abs(C2 - ref[64:]).max() <= tol
    store = 2.0**-24 * np.abs(ref).max() if f32 else 0.0
    assert np.abs(P2 - ref[:64])[live].max() <= tol + store
    keep = P.astype(np.float32).astype(np.float64) if f32 else P
    assert np.array_equal(P2[~live], keep[~live])  # what lies above the diagonal or beyond n comes back as given


# ---- the whole call --------------------------------------------------------------------------------------------------
def _fetch_check(h, full, name, tol=1e-8):
    worst = 0.0
    for s, f in enumerate(full):
        al, sw, L = h.fetch(s)
        Lp = L.T if f.L_chol else L  # (the device holds the lower factor, the record SciPy's upper one)
        ea, eL = _rel(al, f.alpha[:, 0]), _rel(Lp, f.L)
        worst = max(worst, ea, eL)
        assert ea <= tol and eL <= tol, (name, s, ea, eL)
        assert np.allclose(sw, f.sW[:, 0], rtol=1e-12), (name, s)
        if f.L_chol:
            assert np.all(np.diag(L) > 0), (name, s)
    return worst


def _remove_and_check(gp, model, hyp, X, y, idx, name, tol=1e-8, want=None):
    S = hyp.shape[0]
    h0 = gp._post_handle
    r0, s0 = _counts()
    gp.remove_points(idx)
    r1, s1 = _counts()
    keep = np.setdiff1d(np.arange(X.shape[0]), np.arange(X.shape[0])[idx])
    assert gp._post_handle is h0, (name, "the resident posteriors must be shrunk, not rebuilt")
    assert (r1 - r0, s1 - s0) == (want or (S, 0)), (name, "fast path / fallback counts", r1 - r0, s1 - s0)
    assert h0.N == keep.size and np.array_equal(gp.X, X[keep]) and np.array_equal(gp.y, y[keep])
    full = orc.posteriors(model, hyp, X[keep], y[keep], None)
    for p, f in zip(gp.posteriors, full):
        assert bool(p.L_chol) == bool(f.L_chol) and p.sn2_mult == f.sn2_mult, name
    worst = _fetch_check(h0, full, name, tol)
    xs = np.random.default_rng(1).standard_normal((20, X.shape[1]))
    mu, s2 = gp.predict(xs, separate_samples=True)  # (the variance is the only reader of W here)
    rmu, rs2 = orc.predict(model, full, X[keep], y[keep], xs, separate_samples=True)
    em, es = np.abs(mu - rmu).max() / max(1.0, np.abs(rmu).max()), np.abs(s2 - rs2).max() / max(1.0, np.abs(rs2).max())
    print("%s: alpha / L %.3g, mean %.3g, variance %.3g" % (name, worst, em, es))
    assert em <= tol and es <= tol, (name, em, es)
    return full


CASES = {
    "one tile, one panel": (20, [7]),
    "storage shrinks 256 -> 128": (130, [5, 64, 129]),
    "tile and panel boundaries": (260, [0, 63, 64, 128, 259]),
    "last rows: truncation only": (260, [256, 257, 258, 259]),
    "64 rows, one sweep": (700, None),
    "65 rows, two sweeps": (700, None),
}


@pytest.mark.parametrize("case", list(CASES))
def test_remove_points_equals_the_oracle_on_the_reduced_data(case):
    N, idx = CASES[case]
    if idx is None:
        idx = np.sort(np.random.default_rng(N).choice(N, 64 if case.startswith("64") else 65, replace=False))
    idx = np.asarray(idx)
    X, y, hyp = _data(N, N)
    gp = _mk("se")
    gp.update(X_new=X, y_new=y, hyp=hyp)
    _remove_and_check(gp, _model("se"), hyp, X, y, idx, case)


def test_last_rows_leave_the_bits_of_the_old_leading_block():
    N, k = 260, 4
    X, y, hyp = _data(N, N)
    gp = _mk("se")
    gp.update(X_new=X, y_new=y, hyp=hyp)
    h = gp._post_handle
    old = [h.fetch(s) for s in range(hyp.shape[0])]
    gp.remove_points(np.arange(N - k, N))
    for s in range(hyp.shape[0]):
        al, sw, L = h.fetch(s)
        assert np.array_equal(L, old[s][2][:N - k, :N - k]), s


def test_high_and_low_noise_samples_in_one_batch_and_a_stale_low_noise_sample():
    """The fixture's low-noise Matern models with sample 1 moved to high noise: both branches in one call.  Then, on
    the unchanged (all low-noise) hyperparameters, sample 1 is declared stale through the test option: it alone is
    recomputed, the others keep what the rank-k correction gave them."""
    from test_gpu_api import _gp as mk

    g = golden()
    ran = 0
    for name in g["names"]:
        tag, model, N, D, flav = parse(name)
        if flav != "low" or N < 100:
            continue
        ran += 1
        X, y, hyp = g[tag + "_X"], g[tag + "_y"], g[tag + "_hyp"]
        cov_N = orc.cov_count(model["kernel"], D)
        mixed = hyp.copy()
        mixed[1, cov_N] = np.log(0.3)
        idx = np.array([0, 63, 64, N - 1])
        gp = mk(model, D)
        gp.update(X_new=X, y_new=y, hyp=mixed)
        assert [bool(p.L_chol) for p in gp.posteriors] == [False, True, False]
        _remove_and_check(gp, model, mixed, X, y, idx, (name, "mixed"))
        gp = mk(model, D)
        gp.update(X_new=X, y_new=y, hyp=hyp)
        ref = mk(model, D)
        ref.update(X_new=X, y_new=y, hyp=hyp)
        ref.remove_points(idx)
        untouched = [ref._post_handle.fetch(s) for s in (0, 2)]
        _ctx().set_option("remove_fail_mask", 0b010)
        try:
            _remove_and_check(gp, model, hyp, X, y, idx, (name, "stale"), want=(2, 1))
        finally:
            _ctx().set_option("remove_fail_mask", 0)
        for (al, sw, L), s in zip(untouched, (0, 2)):  # the other samples: the bits of a call without the option
            bl, bw, BL = gp._post_handle.fetch(s)
            assert np.array_equal(al, bl) and np.array_equal(L, BL), (name, s)
    assert ran >= 2


def test_remove_points_with_a_user_defined_kernel():
    """No covariance is evaluated: a posterior built from a Python kernel's own K takes the same call.  The first
    removal shrinks the storage (130 -> 127 rows: two tiles to one) with sample 0 declared stale: its recompute from the
    object's own K must find a fresh posterior's layout."""
    N, idx = 130, np.array([3, 70, 129])
    X, y, hyp = _data(N, N)
    gp = _py_se_gp()
    gp.update(X_new=X, y_new=y, hyp=hyp)
    _ctx().set_option("remove_fail_mask", 0b01)
    try:
        _remove_and_check(gp, _model("se"), hyp, X, y, idx, "python kernel, stale", want=(1, 1))
    finally:
        _ctx().set_option("remove_fail_mask", 0)
    keep = np.setdiff1d(np.arange(N), idx)
    _remove_and_check(gp, _model("se"), hyp, X[keep], y[keep], np.array([0, 100]), "python kernel")


@pytest.mark.parametrize("N,idx", [(130, [5, 64, 129]), (300, list(range(100, 170, 2)))])
def test_remove_points_of_fp32_posteriors(N, idx):
    idx = np.asarray(idx)
    X, y, hyp = _data(N, N)
    gp = _mk("se", dtype="float32")
    gp.update(X_new=X, y_new=y, hyp=hyp)
    h0 = gp._post_handle
    r0, s0 = _counts()
    gp.remove_points(idx)
    r1, s1 = _counts()
    assert gp._post_handle is h0 and (r1 - r0, s1 - s0) == (hyp.shape[0], 0)
    keep = np.setdiff1d(np.arange(N), idx)
    model = _model("se")
    full = [orc.core(model, hyp[s], X[keep], y[keep], None, 0, 0, force_mult=p.sn2_mult) for s, p in enumerate(gp.posteriors)]
    xs = np.random.default_rng(1).standard_normal((20, 2))
    mu, s2 = gp.predict(xs, separate_samples=True)
    rmu, rs2 = orc.predict(model, full, X[keep], y[keep], xs, separate_samples=True)
    em, es = np.abs(mu - rmu).max() / max(1.0, np.abs(rmu).max()), np.abs(s2 - rs2).max() / max(1.0, np.abs(rs2).max())
    print("fp32 N = %d: mean %.3g, variance %.3g" % (N, em, es))
    assert em <= 1e-3 and es <= 1e-3


def test_the_bits_of_a_sample_do_not_depend_on_the_batch():
    N, idx = 260, np.array([0, 63, 64, 128, 259])
    X, y, hyp2 = _data(N, N)
    hyp = np.concatenate([hyp2, hyp2[::-1] + 0.01])
    out = []
    for rows in (hyp, hyp[:1]):
        gp = _mk("se")
        gp.update(X_new=X, y_new=y, hyp=rows)
        gp.remove_points(idx)
        al, sw, L = gp._post_handle.fetch(0)
        mu, s2 = gp.predict(X[:7] + 0.01, separate_samples=True)
        out.append((al, L, mu[:, 0], s2[:, 0]))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_append_five_rows_and_remove_them_three_times_over():
    from test_gpu_block_append import _check_against_oracle

    N = 200
    X, y, hyp = _data(N + 5, 21)
    gp = _mk("matern5")
    gp.update(X_new=X[:N], y_new=y[:N], hyp=hyp)
    h0 = gp._post_handle
    for _ in range(3):
        gp.update(X_new=X[N:], y_new=y[N:], block_append=True)
        gp.remove_points(np.arange(N, N + 5))
        assert gp._post_handle is h0 and h0.N == N
    xs = np.random.default_rng(2).standard_normal((15, 2))
    _check_against_oracle(gp, _model("matern5"), hyp, X[:N], y[:N], xs, "round trips")


def test_consumers_after_remove_points_agree_with_a_fresh_gp_on_the_reduced_data():
    N, idx = 300, np.array([2, 64, 65, 190, 299])
    X, y, hyp = _data(N, 13)
    keep = np.setdiff1d(np.arange(N), idx)
    gp, ref = _mk("se"), _mk("se")
    gp.update(X_new=X, y_new=y, hyp=hyp)
    gp.predict(X[:3])  # (puts the constants of the 300-point posterior on the device)
    r0, s0 = _counts()
    gp.remove_points(idx)
    assert tuple(np.subtract(_counts(), (r0, s0))) == (2, 0)
    ref.update(X_new=X[keep], y_new=y[keep], hyp=hyp)
    xs = np.random.default_rng(3).standard_normal((12, 2))

    def same(a, b, what):
        for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            e = np.abs(np.asarray(u) - np.asarray(v)).max() / max(1.0, np.abs(v).max())
            assert e <= 1e-8, (what, e)

    same(gp.predict(xs, separate_samples=True), ref.predict(xs, separate_samples=True), "predict")
    same(gp.predict_full(xs), ref.predict_full(xs), "predict_full")
    same(gp.cv_predict(separate_samples=True), ref.cv_predict(separate_samples=True), "cv_predict")
    same(gp.lookahead_variance(xs[:5], xs[5:], separate_samples=True),
         ref.lookahead_variance(xs[:5], xs[5:], separate_samples=True), "lookahead_variance")
    mu, sigma = np.zeros((2, 2)), np.ones((2, 2))
    same(gp.quad(mu, sigma, compute_var=True, separate_samples=True),
         ref.quad(mu, sigma, compute_var=True, separate_samples=True), "quad")


def test_without_the_test_option_only_short_sweeps_above_one_tile_take_the_device_path():
    ctx = _ctx()
    ctx.set_option("remove_force", 0)
    limit, rows = ctx.get_option("remove_max_panels"), ctx.get_option("remove_min_rows")
    assert 0 <= limit < 1 << 30 and rows >= 0
    for N, idx in ((260, [0, 259]), (260, [258, 259]), (100, [98, 99]), (131, [128, 129, 130])):
        idx = np.array(idx)
        X, y, hyp = _data(N, N)
        fast = rm.swept_panels(N, idx) <= limit and N - idx.size > rows
        gp = _mk("se")
        gp.update(X_new=X, y_new=y, hyp=hyp)
        h0 = gp._post_handle
        r0, s0 = _counts()
        gp.remove_points(idx)
        assert tuple(np.subtract(_counts(), (r0, s0))) == ((hyp.shape[0], 0) if fast else (0, 0)), (N, idx)
        assert (gp._post_handle is h0) == fast, (N, idx)
        keep = np.setdiff1d(np.arange(N), idx)
        _fetch_check(gp._post_handle, orc.posteriors(_model("se"), hyp, X[keep], y[keep], None), ("routing", N, fast))
    assert limit == 1 and rows == 128  # (remove.h's constants as measured: of the four cases only the second is fast)


# ---- refusals and the scratch budget ---------------------------------------------------------------------------------
def _state(h, S):
    return [h.fetch(s) for s in range(S)]


def test_every_refusal_leaves_the_posterior_untouched():
    N = 140
    X, y, hyp = _data(N, 5)
    S = hyp.shape[0]
    gp = _mk("se")
    gp.update(X_new=X, y_new=y, hyp=hyp)
    h = gp._post_handle
    before = _state(h, S)

    def refused(idx, ym, needle):
        with pytest.raises(Exception) as e:
            h.remove(idx, ym)
        assert needle in str(e.value), (idx, str(e.value))
        assert h.N == N
        for (a, w, L), (a0, w0, L0) in zip(_state(h, S), before):
            assert np.array_equal(a, a0) and np.array_equal(L, L0)

    refused(np.array([3, 4]), np.zeros((S, N - 2)), "reduced")            # the data still has N rows
    gp.X, gp.y = X[:-2], y[:-2]
    gp._token = None
    gp._ctx()  # uploads N - 2 rows: what a removal of two rows expects
    refused(np.array([4, 3]), np.zeros((S, N - 2)), "sorted")
    refused(np.array([3, 3]), np.zeros((S, N - 2)), "sorted")
    refused(np.array([3, N]), np.zeros((S, N - 2)), "sorted")
    refused(np.array([-1, 3]), np.zeros((S, N - 2)), "sorted")
    refused(np.array([3, 4, 5]), np.zeros((S, N - 3)), "reduced")         # three rows, data reduced by two
    refused(np.zeros(0, dtype=np.int32), np.zeros((S, N)), "at least 1")
    refused(np.arange(N), np.zeros((S, 0)), "less than N")
    lib = _ctx()._lib
    assert lib.gpc_post_remove(h._h, 2, None, None, None) == -2            # null arguments
    os.environ["GPC_MEM_BUDGET_MB"] = "0"  # (read at every call) one sample's scratch is 0.5 MB: no room for it
    try:
        refused(np.array([3, 4]), np.zeros((S, N - 2)), "exceeds the device memory budget")
    finally:
        del os.environ["GPC_MEM_BUDGET_MB"]
    # ... and after all that the same handle still takes the removal it was prepared for
    ym = np.ravel(y[:-2])[None, :] - hyp[:, 4:5]
    assert h.remove(np.array([N - 2, N - 1]), ym).all() and h.N == N - 2


def test_a_scratch_budget_too_small_for_all_samples_chunks_with_the_same_bits():
    """N = 700 - 40: per sample three 768 x 48 fp64 panels (0.84 MB), Theta (112^2 x 8) and the three 128^2 slabs of the
    k x k factorization (0.38 MB): 1.4 MB.  80 % of 4 MB hold two of the five samples: chunks of 2, 2, 1."""
    N, S = 700, 5
    X, y, _ = _data(N, 3)
    hyp = np.array([0.1, -0.1, 0.05, np.log(0.2), 0.1]) + 0.05 * np.random.default_rng(4).standard_normal((S, 5))
    idx = np.sort(np.random.default_rng(5).choice(N, 40, replace=False))
    out = []
    for mb in (None, 4):
        gp = _mk("matern5")
        gp.update(X_new=X, y_new=y, hyp=hyp)
        if mb is not None:
            os.environ["GPC_MEM_BUDGET_MB"] = str(mb)
        try:
            r0, s0 = _counts()
            gp.remove_points(idx)
            assert tuple(np.subtract(_counts(), (r0, s0))) == (S, 0)
            chunk = _ctx().get_option("last_chunk")
        finally:
            os.environ.pop("GPC_MEM_BUDGET_MB", None)
        out.append([a for s in range(S) for a in gp._post_handle.fetch(s)])
        per = (3 * 768 * 48 + 112 * 112 + 3 * 48) * 8 + 3 * 128 * 128 * 8
        assert chunk == (S if mb is None else min(S, int((mb << 20) * 0.8) // per)), (mb, chunk)
    assert out and _ctx().get_option("last_chunk") == 2
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    keep = np.setdiff1d(np.arange(N), idx)
    _fetch_check(gp._post_handle, orc.posteriors(_model("matern5"), hyp, X[keep], y[keep], None), "chunked")
