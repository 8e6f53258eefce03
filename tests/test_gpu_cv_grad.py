"""GP.cv_nll_batch on the device (gpc_cv_grad) against gpyreg_amd._cvgrad: the contraction and the per-point kernel through
their debug hooks, the pipeline's parity in fp64, agreement with cv_predict, the gradient against differences of the
device's own value, bit identities (batch, chunking, resident posteriors), the budget refusal and log_pseudo_likelihood."""

import os
import subprocess
import sys

import numpy as np
import pytest

import gpyreg_amd as gpr
from gpyreg_amd import _cvgrad as cg
from gpyreg_amd import _nllhess as nh
from test_gpu_nll_hess import _device_scaled, _problem  # the sibling objective's problems and scaled inputs

pytestmark = pytest.mark.gpu

KID = {"se": 0, "matern": 1, "rq": 2, "se_iso": 3, "matern_iso": 4}
FAMILIES = [("se", 0), ("matern", 3), ("matern", 5), ("rq", 0), ("se_iso", 0), ("matern_iso", 3), ("matern_iso", 5)]
LOSSES = ("lpd", "mse")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from gpyreg_amd import _lib

    return _lib.context(0)


# ---- the kernels, through the hooks ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", [(n, d) for n in (1, 2, 64, 65, 130) for d in (1, 3, 33)])
@pytest.mark.parametrize("kernel,degree", FAMILIES)
def test_trace_kernel_per_entry(ctx, kernel, degree, N, D):
    """<d_p K, G> for every covariance hyperparameter against NumPy on the same scaled inputs, each within 1e-12 of the
    sum of the absolute values of its terms (|M| + |beta alpha^T| / 2 + |alpha beta^T| / 2 for the weight, the sum of
    the absolute terms of the rational quadratic's Ka, a difference inside the functor), and diag(G) per entry.  M is
    handed over as its lower triangle alone.  N crosses the 64-tile and includes one row; D = 33 crosses the
    32-dimension staging; the last point duplicates the first (r2 = 0 off the diagonal); the inputs lie 1e4 lengthscales
    from the origin."""
    kid = KID[kernel]
    rng = np.random.default_rng(100 * N + D)
    nl = 1 if kernel.endswith("_iso") else D
    ell = 1.2 * np.sqrt(D) * np.exp(0.1 * rng.standard_normal(nl))
    X = 1e4 * ell * np.ones(D) + rng.uniform(-2, 2, (N, D)) * np.sqrt(D)
    if N > 1:
        X[N - 1] = X[0]
    hyp = np.r_[np.log(ell), 0.2] if kernel != "rq" else np.r_[np.log(ell), 0.2, np.log(0.7)]
    alpha, beta = rng.standard_normal(N), rng.standard_normal(N)
    M = rng.standard_normal((N, N))
    M = (M + M.T) / 2
    xs = _device_scaled(kid, degree, hyp, X)
    _, dK, _ = nh.cov_derivatives(kid, degree, hyp, X, xs=xs)
    ba = np.outer(beta, alpha)
    G = M - (ba + ba.T) / 2
    Gmag = np.abs(M) + (np.abs(ba) + np.abs(ba.T)) / 2
    gsum, diagG = ctx.debug_cv_trace(kid, degree, hyp, X, np.tril(M), alpha, beta)
    assert gsum.shape == (len(dK),) and diagG.shape == (N,)
    for p, plane in enumerate(dK):
        mag = np.abs(plane)
        if kernel == "rq" and p == D + 1:
            _, r2, _, rqa = nh.scaled_sq_diffs(kid, degree, hyp, X, xs=xs)
            Mv = 1 + r2 / (2 * rqa)
            mag = nh.radial(kid, degree, r2, np.exp(2 * hyp[D]), rqa)["K"] * (r2 / (2 * Mv) + rqa * np.log(Mv))
        want, bound = np.sum(plane * G), 1e-12 * np.sum(mag * Gmag)
        assert abs(gsum[p] - want) <= bound, (p, gsum[p], want, abs(gsum[p] - want) / max(bound, 1e-300))
    assert np.all(np.abs(diagG - np.diag(G)) <= 1e-15 * np.diag(Gmag))


@pytest.mark.parametrize("loss", LOSSES)
def test_weights_kernel_per_entry(ctx, loss):
    rng = np.random.default_rng(17)
    N = 300  # (two blocks of the launch)
    alpha, q, w = rng.standard_normal(N), rng.uniform(0.05, 40.0, N), rng.uniform(0.0, 3.0, N)
    w[5] = 0.0
    alpha[9] = 0.0
    for weights in (w, None):
        c, b = ctx.debug_cv_weights(cg.LOSSES.index(loss), alpha, q, weights)
        rc, rb = cg.loo_weights(alpha, q, loss, weights)
        assert np.all(np.abs(c - rc) <= 1e-14 * np.abs(rc)) and np.all(np.abs(b - rb) <= 1e-14 * np.abs(rb))
        assert b[9] == 0 and (c[9] == 0) == (loss == "mse")
    c, b = ctx.debug_cv_weights(cg.LOSSES.index(loss), alpha, q, w)
    assert c[5] == 0 and b[5] == 0


# ---- the pipeline ----------------------------------------------------------------------------------------------------
def _reference(gp, hyp, loss, weights=None, mult=None, dtype=np.float64):
    """The restatement for every row of hyp: (L (S,), dL (S, P))."""
    cov_N = gp._counts()[0]
    kid, deg = gp._kid()
    pv = gp._plugin_values(hyp, True)
    out = [cg.cv_nll(kid, deg, hyp[s, :cov_N], gp.X, gp.y[:, 0] - pv["m"][s], pv["sn2"][s],
                     1.0 if mult is None else mult[s], None if pv["dm"] is None else pv["dm"][s], pv["dsn2"][s], loss,
                     weights, dtype=dtype) for s in range(hyp.shape[0])]
    return np.array([float(o[0]) for o in out]), np.stack([np.asarray(o[1], dtype=float) for o in out])


def _assert_parity(L, dL, rL, rdL, tol=1e-8, what=""):
    for s in range(L.shape[0]):
        eg, sg = np.abs(dL[s] - rdL[s]).max(), max(1.0, np.abs(rdL[s]).max())
        ev, sv = abs(L[s] - rL[s]), max(1.0, abs(rL[s]))
        print(f"{what} sample {s}: |dL_dev - dL_ref| = {eg / sg:.2e}, |L_dev - L_ref| = {ev / sv:.2e} of max(1, largest)")
        assert eg <= tol * sg and ev <= tol * sv, (what, s, eg / sg, ev / sv)


@pytest.mark.parametrize("per_point", [False, True])
@pytest.mark.parametrize("mean", ["zero", "const", "negquad"])
@pytest.mark.parametrize("kernel,degree", FAMILIES)
def test_pipeline_parity(kernel, degree, mean, per_point):
    """Value and gradient within 1e-8 max(1, largest entry) per sample of the float64 restatement -- the project's fp64
    parity bound -- for N in {50, 65, 130, 200} x D in {1, 3}, every family, each mean, scalar and per-point noise, both
    losses (N = 65 with non-uniform weights, a zero among them)."""
    for N in (50, 65, 130, 200):
        for D in (1, 3):
            gp, X, y, s2, hyp = _problem(kernel, degree, mean, N, D, per_point=per_point)
            w = None
            if N == 65:
                w = np.random.default_rng(N + D).uniform(0.2, 2.0, N)
                w[11] = 0.0
            for loss in LOSSES:
                L, dL = gp.cv_nll_batch(hyp, loss=loss, weights=w)
                rL, rdL = _reference(gp, hyp, loss, w)
                _assert_parity(L, dL, rL, rdL, what=f"{kernel}{degree} {mean} N={N} D={D} {loss}")


def test_mixed_batch_with_a_low_noise_sample():
    """An L_chol = 0 sample (sn2 = 1e-7 < 1e-6: the posterior holds -(K + Sigma)^-1) between two L_chol = 1 samples:
    one path after Q is formed.  The L_chol samples are held to the float64 restatement, the low-noise one to the
    restatement in longdouble on the same sample, all at 1e-8 max(1, largest entry)."""
    gp, X, y, s2, hyp = _problem("matern", 5, "const", 50, 3, S=3)
    cov_N = gp._counts()[0]
    hyp[1, cov_N] = 0.5 * np.log(1e-7)
    gp.update(hyp=hyp)
    assert [p.L_chol for p in gp.posteriors] == [True, False, True]
    mult = [float(p.sn2_mult) for p in gp.posteriors]
    for loss in LOSSES:
        L, dL = gp.cv_nll_batch(loss=loss)
        rL, rdL = _reference(gp, hyp, loss, mult=mult)
        _assert_parity(L[[0, 2]], dL[[0, 2]], rL[[0, 2]], rdL[[0, 2]], what=f"L_chol {loss}")
        lL, ldL = _reference(gp, hyp[1:2], loss, mult=mult[1:2], dtype=np.longdouble)
        _assert_parity(L[1:2], dL[1:2], lL, ldL, what=f"low noise against longdouble {loss}")
        one = gp.cv_nll_batch(hyp[1:2], loss=loss)  # the low-noise sample alone: the same bits
        assert one[0][0] == L[1] and np.array_equal(one[1][0], dL[1])


def test_value_agrees_with_cv_predict():
    """loss = "lpd" is the negated sum of cv_predict's single-point folds, at 1e-10 (of max(1, |L|)): on resident
    posteriors, after a block append, from the gradient call and from the value-only call."""
    gp, X, y, s2, hyp = _problem("se", 0, "const", 130, 3, S=2)
    gp.X, gp.y = X[:120], y[:120]
    gp.update(hyp=hyp)
    for stage in ("resident", "appended"):
        if stage == "appended":
            gp.update(X_new=X[120:], y_new=y[120:], block_append=True)
            assert gp.X.shape[0] == 130
        _, _, _, lpd_fold = gp.cv_predict(return_lpd=True, separate_samples=True)
        want = -lpd_fold.sum(0)
        for grad in (True, False):
            L, dL = gp.cv_nll_batch(compute_grad=grad)
            err = np.abs(L - want) / np.maximum(1.0, np.abs(want))
            print(f"{stage}, compute_grad={grad}: |L + sum lpd| = {err.max():.2e} of max(1, |L|)")
            assert np.all(err <= 1e-10) and (dL is None) == (not grad)
    gp2, *_ = _problem("se", 0, "const", 130, 3, S=2)
    L2, dL2 = gp2.cv_nll_batch(hyp)  # the appended posteriors against fresh ones: rounding apart
    L, dL = gp.cv_nll_batch()
    assert np.all(np.abs(L - L2) <= 1e-8 * np.maximum(1.0, np.abs(L2)))
    assert np.all(np.abs(dL - dL2) <= 1e-8 * np.maximum(1.0, np.abs(dL2).max()))


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("kernel,degree,mean,per_point", [("se", 0, "negquad", False), ("matern", 5, "const", True),
                                                          ("rq", 0, "zero", False), ("matern_iso", 3, "const", False)])
def test_gradient_against_device_differences(kernel, degree, mean, per_point, loss):
    """Central differences of cv_nll_batch(hyp +- h, compute_grad=False) -- the device's own value, by the leave-one-out
    pass -- at 1e-6 max(1, largest entry); all 2 P rows of a sample in one batch."""
    gp, X, y, s2, hyp = _problem(kernel, degree, mean, 130, 3, S=2)
    _, dL = gp.cv_nll_batch(hyp, loss=loss)
    P = hyp.shape[1]
    step = 1e-4
    for s in range(hyp.shape[0]):
        rows = np.repeat(hyp[s:s + 1], 2 * P, 0)
        rows[np.arange(P), np.arange(P)] += step
        rows[P + np.arange(P), np.arange(P)] -= step
        v, none = gp.cv_nll_batch(rows, compute_grad=False, loss=loss)
        assert none is None
        fd = (v[:P] - v[P:]) / (2 * step)
        err = np.abs(dL[s] - fd).max() / max(1.0, np.abs(fd).max())
        print(f"{kernel}{degree} {mean} {loss} sample {s}: |dL - fd| = {err:.2e} of max(1, largest entry)")
        assert err <= 1e-6


def test_bit_identities():
    """A sample alone or in a batch of five; resident posteriors (hyp=None) or the same hyp passed; unit weights."""
    gp, X, y, s2, hyp = _problem("rq", 0, "negquad", 130, 3, S=5)
    for loss in LOSSES:
        L, dL = gp.cv_nll_batch(hyp, loss=loss)
        for s in range(5):
            L1, dL1 = gp.cv_nll_batch(hyp[s:s + 1], loss=loss)
            assert L1[0] == L[s] and np.array_equal(dL1[0], dL[s])
        Lw, dLw = gp.cv_nll_batch(hyp, loss=loss, weights=np.ones(130))
        assert np.array_equal(Lw, L) and np.array_equal(dLw, dL)
    gp.update(hyp=hyp)
    Lr, dLr = gp.cv_nll_batch(loss="mse")
    assert np.array_equal(Lr, L) and np.array_equal(dLr, dL)


_CHILD = """
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from test_gpu_cv_grad import _problem
gp, X, y, s2, hyp = _problem("matern", 3, "const", 130, 3, S=5)
try:
    L, dL = gp.cv_nll_batch(hyp)
    np.save(sys.argv[1], np.c_[L, dL])
except RuntimeError as e:
    print("REFUSED:", e)
from gpyreg_amd import _lib
print("LAST_CHUNK", _lib.context().get_option("last_chunk"))
"""


def test_chunking_changes_no_bit_and_the_budget_refusal(tmp_path):
    """GPC_MEM_BUDGET_MB in child processes: budgets that fit one and two samples per chunk (a sample's scratch at
    N_pad = 256 is 3 N_pad^2 doubles = 1.6 MB and vectors; the planner takes 80 %) give the bits of the unchunked call;
    1 MB fits no sample and is refused with the sizes in the message.  Each child reports the chunk the library planned
    ("last_chunk"): it is the one that the scratch's closed form (scratch_sizes.cv_grad_per) gives."""
    from scratch_sizes import cv_grad_per, planned_chunk

    gp, X, y, s2, hyp = _problem("matern", 3, "const", 130, 3, S=5)
    L, dL = gp.cv_nll_batch(hyp)
    per, shared = cv_grad_per(256, gp._counts()[0]), 256 * 8
    assert [planned_chunk(5, mb, per, shared) for mb in (3, 5, 1)] == [1, 2, 0]
    script = tmp_path / "child.py"
    script.write_text(_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests")))
    for mb, refused in ((3, False), (5, False), (1, True)):
        out = tmp_path / f"l{mb}.npy"
        env = dict(os.environ, GPC_MEM_BUDGET_MB=str(mb))
        r = subprocess.run([sys.executable, str(script), str(out)], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert f"LAST_CHUNK {planned_chunk(5, mb, per, shared)}\n" in r.stdout, r.stdout
        if refused:
            # (with the scratch's size to the byte: the closed form pins every array of the layout, not only the chunk)
            assert "REFUSED" in r.stdout and f"gpc_cv_grad: the scratch of one sample ({per} bytes:" in r.stdout
            assert "N_pad = 256" in r.stdout
        else:
            assert np.array_equal(np.load(out), np.c_[L, dL]), mb


def test_log_pseudo_likelihood():
    """-L of the "lpd" loss for one vector, as an array or as a dict; the pair with compute_grad."""
    gp, X, y, s2, hyp = _problem("matern", 5, "const", 65, 3, S=1)
    L, dL = gp.cv_nll_batch(hyp)
    v, g = gp.log_pseudo_likelihood(hyp[0], compute_grad=True)
    assert v == -L[0] and np.array_equal(g, -dL[0])
    v0 = gp.log_pseudo_likelihood(hyp[0])
    assert isinstance(v0, float) and abs(v0 - v) <= 1e-10 * max(1.0, abs(v))
    as_dict = gp.hyperparameters_to_dict(hyp)[0]
    vd, gd = gp.log_pseudo_likelihood(as_dict, compute_grad=True)
    assert vd == v and np.array_equal(gd, g)
    gp.update(hyp=hyp)
    _, _, lpd, _ = gp.cv_predict(return_lpd=True, separate_samples=True)
    assert abs(v - lpd.sum()) <= 1e-10 * max(1.0, abs(v))  # (a log density summed, not negated)


def test_device_refusals(ctx):
    gp, X, y, s2, hyp = _problem("se", 0, "const", 50, 3, S=1)
    gp.update(hyp=hyp)
    h = gp._post_handle
    with pytest.raises(ValueError, match="loss must be one of"):
        h.cv_grad(4, "nlpd")
    with pytest.raises(RuntimeError, match="gpc_cv_grad: the weights must be finite"):
        h.cv_grad(4, "lpd", -np.ones(50))
    rc = ctx._lib.gpc_cv_grad(h._h, 2, None, None, None, None, None, None, None)
    assert rc == -2 and b"gpc_cv_grad: bad arguments" in ctx._lib.gpc_last_error(ctx._h)
    with pytest.raises(RuntimeError, match="gpc_debug_cv_trace: bad arguments"):
        ctx.debug_cv_trace(1, 1, np.zeros(4), X, np.zeros((50, 50)), np.zeros(50), np.zeros(50))
    gp32 = gpr.GP(3, gpr.covariance_functions.SquaredExponential(), gpr.mean_functions.ConstantMean(),
                  gpr.noise_functions.GaussianNoise(constant_add=True), dtype="f32")
    gp32.X, gp32.y = X, y
    gp32.update(hyp=hyp)
    with pytest.raises(RuntimeError, match="gpc_cv_grad: the cross-validation gradient is fp64 only"):
        gp32._post_handle.cv_grad(4)
