"""GP.nll_hess_batch on the device (gpc_nll_hess) against gpyreg_amd._nllhess: every kernel through its debug hook, the
pipeline's parity in fp64, bit identities, the gradient against nll_batch, central differences, the Python layer
(log_posterior_hess, laplace_approximation) and the refusals."""

import os
import subprocess
import sys

import numpy as np
import pytest

import gpyreg_amd as gpr
from gpyreg_amd import _nllhess as nh

pytestmark = pytest.mark.gpu

KID = {"se": 0, "matern": 1, "rq": 2, "se_iso": 3, "matern_iso": 4}
FAMILIES = [("se", 0), ("matern", 3), ("matern", 5), ("rq", 0), ("se_iso", 0), ("matern_iso", 3), ("matern_iso", 5)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from gpyreg_amd import _lib

    return _lib.context(0)


def _cov(kernel, degree):
    c, i = gpr.covariance_functions, gpr.isotropic_covariance_functions
    return {"se": c.SquaredExponential, "rq": c.RationalQuadraticARD, "se_iso": i.SquaredExponentialIsotropic,
            "matern": lambda: c.Matern(degree), "matern_iso": lambda: i.MaternIsotropic(degree)}[kernel]()


def _mean(name):
    m = gpr.mean_functions
    return {"zero": m.ZeroMean, "const": m.ConstantMean, "negquad": m.NegativeQuadratic}[name]()


# ---- the kernels, through the hooks ----------------------------------------------------------------------------------
def _device_scaled(kid, degree, hyp, X):
    """The scaled inputs as the device forms them, operation for operation (x mul / dv), the lengthscales from the C
    library's exp as the host code takes them (math.exp: NumPy's own exp may differ in the last bit, and 1e4 lengthscales
    from the origin one ulp of a scaled coordinate is 2e-12 of a difference of order one)."""
    import math

    D = X.shape[1]
    iso = kid in (3, 4)
    nl = 1 if iso else D
    snu = np.sqrt(float(degree)) if kid in (1, 4) else 1.0
    dv = np.array([math.exp(h) for h in hyp[:nl]]) * np.ones(D)
    mul, div = ((snu * np.ones(D), dv) if iso or kid == 0 else (snu / dv, np.ones(D)))
    return X * mul / div


_HOOK_CASES = {}


def _hook_case(kernel, degree, N, D):
    """Inputs 1e4 lengthscales from the origin with a duplicated point, weights alpha and a symmetric Q, and the NumPy
    planes, second factors and contraction sums on the device's own scaled inputs."""
    key = (kernel, degree, N, D)
    if key not in _HOOK_CASES:
        kid = KID[kernel]
        rng = np.random.default_rng(100 * N + D)
        nl = 1 if kernel.endswith("_iso") else D
        ell = 1.2 * np.sqrt(D) * np.exp(0.1 * rng.standard_normal(nl))
        X = 1e4 * ell * np.ones(D) + rng.uniform(-2, 2, (N, D)) * np.sqrt(D)
        if N > 1:
            X[N - 1] = X[0]
        hyp = np.r_[np.log(ell), 0.2] if kernel != "rq" else np.r_[np.log(ell), 0.2, np.log(0.7)]
        alpha = rng.standard_normal(N)
        Q = rng.standard_normal((N, N))
        Q = (Q + Q.T) / 2
        xs = _device_scaled(kid, degree, hyp, X)
        K, dK, second = nh.cov_derivatives(kid, degree, hyp, X, xs=xs)
        d2, r2, sf2, rqa = nh.scaled_sq_diffs(kid, degree, hyp, X, xs=xs)
        R = nh.radial(kid, degree, r2, sf2, rqa)
        if kernel == "rq":
            # Ka = K (r2 / (2 M) - alpha log M) and its relatives are DIFFERENCES of terms that nearly cancel at small
            # r2 (both ~ r2 / 2): the closed form's own error is relative to the sum of the absolute terms, kept here
            M = 1 + r2 / (2 * rqa)
            t = r2 / (2 * M) + rqa * np.log(M)
            R["mag_Ka"] = R["K"] * t
            R["mag_Fa"] = R["F"] * (t + r2 / (2 * rqa * M))
            R["mag_Kaa"] = R["K"] * (t * t + t + r2 * r2 / (4 * rqa * M * M))
        _HOOK_CASES[key] = (kid, hyp, X, alpha, Q, dK, d2, r2, R)
    return _HOOK_CASES[key]


@pytest.mark.parametrize("N,D", [(1, 1), (2, 3), (64, 1), (65, 3), (130, 3), (65, 33)])
@pytest.mark.parametrize("kernel,degree", FAMILIES)
def test_plane_kernel_per_entry(ctx, kernel, degree, N, D):
    """Every plane entry, every u and both fused sums against NumPy on the same scaled inputs: both sides evaluate the
    same closed form and differ in the rounding of exp / sqrt / log and in the order of the sums, so an entry is held to
    1e-12 of its size (of the sum of the absolute terms of the rational quadratic's alpha-derivatives, which are
    differences inside the functor) and a sum to 1e-12 of the sum of the absolute values of its terms.  N crosses the 64-tile and
    includes one row; D = 33 crosses the 32-dimension staging (the plane's own chunk is staged again); the last point
    duplicates the first (r2 = 0 off the diagonal); the inputs lie 1e4 lengthscales from the origin."""
    kid, hyp, X, alpha, Q, dK, d2, r2, R = _hook_case(kernel, degree, N, D)
    Qm = Q - np.outer(alpha, alpha)
    iso = kernel.endswith("_iso")
    planes = range(len(dK)) if D < 33 or iso else [0, 31, 32, D] + ([D + 1] if kernel == "rq" else [])
    for p in planes:
        plane, u, g = ctx.debug_nll_plane(kid, degree, hyp, X, p, alpha, Q)
        want = dK[p]
        mag = R["mag_Ka"] if kernel == "rq" and p == D + 1 else np.abs(want)
        assert np.all(np.abs(plane - want) <= 1e-12 * mag), (p, np.abs(plane - want).max())
        assert np.all(np.abs(u - want @ alpha) <= 1e-12 * (mag @ np.abs(alpha))), p
        if iso and p == 0:
            sec = R["G"] * r2 * r2
        elif kernel == "rq" and p < D:
            sec = R["Fa"] * d2[p]
        elif kernel == "rq" and p == D + 1:
            sec = R["Kaa"]
        else:
            sec = np.zeros_like(want)
        smag = (R["mag_Fa"] * d2[p] if p < D else R["mag_Kaa"]) if kernel == "rq" and p != D else np.abs(sec)
        for got, term, tmag in ((g[0], Qm * want, np.abs(Qm) * mag), (g[1], Qm * sec, np.abs(Qm) * smag)):
            assert abs(got - term.sum()) <= 1e-12 * tmag.sum(), (p, got, term.sum())
    if N > 1:  # the duplicated pair: nothing in any lengthscale plane
        plane, _, _ = ctx.debug_nll_plane(kid, degree, hyp, X, 0, alpha, Q)
        assert plane[0, N - 1] == 0 and plane[N - 1, 0] == 0 and np.all(np.diag(plane) == 0)


@pytest.mark.parametrize("N,D", [(1, 1), (2, 3), (64, 1), (65, 3), (130, 3), (65, 33)])
@pytest.mark.parametrize("kernel,degree", [f for f in FAMILIES if not f[0].endswith("_iso")])
def test_second_derivative_sums_per_entry(ctx, kernel, degree, N, D):
    """sum Qm G d_a^2 d_b^2 over the lower triangle (weight 2 off the diagonal) for every a >= b, each within 1e-12 of
    the sum of the absolute values of its terms.  D = 33 takes the path that reads coordinates beyond the staged 32."""
    kid, hyp, X, alpha, Q, dK, d2, r2, R = _hook_case(kernel, degree, N, D)
    W = (Q - np.outer(alpha, alpha)) * R["G"]  # symmetric: the full sum is the weighted lower-triangle sum
    got = ctx.debug_nll_d2(kid, degree, hyp, X, alpha, Q)
    a, b = np.tril_indices(D)
    assert got.shape == (a.size,)
    for k in range(a.size):
        term = W * d2[a[k]] * d2[b[k]]
        assert abs(got[k] - term.sum()) <= 1e-12 * np.abs(term).sum(), (a[k], b[k], got[k], term.sum())


@pytest.mark.parametrize("npad", [128, 192])
@pytest.mark.parametrize("P", [1, 2, 13, 35])
def test_gram_kernel_exact_on_integer_planes(ctx, P, npad):
    """tr(B_p B_q) for every q <= p on planes of small integers -- every product and partial sum is an integer below
    2^53, so the expected value is exact and the comparison is ==; nothing is written around the output."""
    rng = np.random.default_rng(P * 1000 + npad)
    planes = rng.integers(-3, 4, (P, npad, npad)).astype(float)
    n = P * (P + 1) // 2
    buf = np.full(n + 16, -777.0)
    out = ctx.debug_nll_gram(planes, buf[8:8 + n])
    want = np.einsum("pab,qba->pq", planes, planes)
    i, j = np.tril_indices(P)
    assert np.array_equal(out, want[i, j])
    assert np.all(buf[:8] == -777.0) and np.all(buf[8 + n:] == -777.0)


# ---- the pipeline ----------------------------------------------------------------------------------------------------
def _problem(kernel, degree, mean, N, D, S=2, per_point=False, sn=0.1, seed=1):
    """Points about a lengthscale apart, noise standard deviation >= 0.03 of the signal's: the restatement and autograd
    agree below 1e-10 there (tests/test_nll_hess_cpu.py)."""
    rng = np.random.default_rng(seed + N + D)
    half = {1: 0.25 * N, 3: 3.0}[D]
    X = rng.uniform(-half, half, (N, D))
    y = np.sin(X.sum(1, keepdims=True) / np.sqrt(D)) + sn * rng.standard_normal((N, 1))
    s2 = rng.uniform(0.5, 2.0, (N, 1)) * sn**2 if per_point else None
    noise = gpr.noise_functions.GaussianNoise(constant_add=True, user_provided_add=per_point, scale_user_provided=per_point)
    gp = gpr.GP(D, _cov(kernel, degree), _mean(mean), noise)
    cov_N, noise_N, mean_N = gp._counts()
    nl = 1 if kernel.endswith("_iso") else D
    hyp = np.zeros((S, cov_N + noise_N + mean_N))
    hyp[:, :nl] = np.log(1.5)
    hyp[:, nl] = np.log(1.2)
    if kernel == "rq":
        hyp[:, nl + 1] = np.log(1.7)
    hyp[:, cov_N] = np.log(sn)
    if mean == "negquad":
        hyp[:, cov_N + noise_N + 1 + D:] = np.log(2.0 * half)
    hyp += 0.05 * rng.standard_normal(hyp.shape)
    gp.X, gp.y, gp.s2 = X, y, s2
    return gp, X, y, s2, hyp


def _reference(gp, hyp, mult=None, dtype=np.float64):
    """The restatement for every row of hyp, plugin terms included: (nlZ, g, H)."""
    cov_N, noise_N, mean_N = gp._counts()
    kid, deg = gp._kid()
    pv = gp._plugin_values(hyp, True)
    out = []
    for s in range(hyp.shape[0]):
        hn, hm = hyp[s, cov_N:cov_N + noise_N], hyp[s, cov_N + noise_N:]
        out.append(nh.nll_hess(kid, deg, hyp[s, :cov_N], gp.X, gp.y[:, 0] - pv["m"][s], pv["sn2"][s],
                               1.0 if mult is None else mult[s], None if pv["dm"] is None else pv["dm"][s], pv["dsn2"][s],
                               nh.noise_d2(gp.noise, hn, gp.X, gp.y, gp.s2), nh.mean_d2(gp.mean, hm, gp.X), dtype=dtype))
    return [np.stack([np.asarray(o[i], dtype=float) for o in out]) for i in range(3)]


def _assert_parity(H, Href, tol=1e-8, what=""):
    for s in range(H.shape[0]):
        err, scale = np.abs(H[s] - Href[s]).max(), np.abs(Href[s]).max()
        print(f"{what} sample {s}: max|H_dev - H_ref| / max|H_ref| = {err / scale:.2e}")
        assert err <= tol * scale, (what, s, err / scale)
        assert np.array_equal(H[s], H[s].T)


@pytest.mark.parametrize("mean,per_point", [("zero", False), ("const", True), ("negquad", False)])
@pytest.mark.parametrize("kernel,degree", FAMILIES)
def test_pipeline_parity(kernel, degree, mean, per_point):
    """max|H_dev - H_ref| <= 1e-8 max|H_ref| per sample against the float64 restatement -- the project's fp64 parity
    figure -- for N in {50, 130, 200} x D in {1, 3}, every family, each mean, scalar and per-point noise; the gradient
    and the value against the same restatement."""
    for N in (50, 130, 200):
        for D in (1, 3):
            gp, X, y, s2, hyp = _problem(kernel, degree, mean, N, D, per_point=per_point)
            nlz, g, H = gp.nll_hess_batch(hyp)
            rz, rg, rH = _reference(gp, hyp)
            _assert_parity(H, rH, what=f"{kernel}{degree} {mean} N={N} D={D}")
            assert np.all(np.abs(g - rg) <= 1e-8 * np.abs(rg).max(1, keepdims=True))
            assert np.all(np.abs(nlz - rz) <= 1e-9 * np.abs(rz))


LOW_NOISE_F64_VS_LONGDOUBLE = 1.7e-15


def test_mixed_batch_with_a_low_noise_sample():
    """An L_chol = 0 sample (sn2 = 1e-7 < 1e-6: the posterior holds -(K + Sigma)^-1) between two L_chol = 1 samples:
    one path after Q is formed.  The L_chol samples are held to 1e-8; the low-noise one is not conditioned for that, its
    yardstick is the restatement in longdouble on the same sample.  Measured on the CPU: the float64 restatement
    deviates from the longdouble one by 1.7e-15 max|H| on this sample (well-spread points: K itself is well conditioned,
    so the tiny noise does not hurt); the device is allowed ten times that, floored at 1e-8 -- here the floor."""
    gp, X, y, s2, hyp = _problem("matern", 5, "const", 50, 3, S=3)
    cov_N = gp._counts()[0]
    hyp[1, cov_N] = 0.5 * np.log(1e-7)
    gp.update(hyp=hyp)
    assert [p.L_chol for p in gp.posteriors] == [True, False, True]
    mult = [float(p.sn2_mult) for p in gp.posteriors]
    nlz, g, H = gp.nll_hess_batch()
    _, _, rH = _reference(gp, hyp, mult)
    _assert_parity(H[[0, 2]], rH[[0, 2]], what="L_chol")
    _, _, lH = _reference(gp, hyp[1:2], mult[1:2], dtype=np.longdouble)
    dev64 = np.abs(rH[1] - lH[0]).max() / np.abs(lH[0]).max()
    err = np.abs(H[1] - lH[0]).max() / np.abs(lH[0]).max()
    print(f"low-noise sample: float64 restatement vs longdouble {dev64:.2e}, device vs longdouble {err:.2e}")
    assert err <= max(10 * LOW_NOISE_F64_VS_LONGDOUBLE, 1e-8)
    assert np.array_equal(H[1], H[1].T)
    one = gp.nll_hess_batch(hyp[1:2])  # the low-noise sample alone: the same bits
    assert np.array_equal(one[2][0], H[1]) and np.array_equal(one[1][0], g[1])


def test_after_block_append_equals_fresh_posterior():
    gp, X, y, s2, hyp = _problem("se", 0, "const", 130, 3, S=2)
    gp2, *_ = _problem("se", 0, "const", 130, 3, S=2)
    gp.X, gp.y = X[:120], y[:120]
    gp.update(hyp=hyp)
    gp.update(X_new=X[120:], y_new=y[120:], block_append=True)
    assert gp.X.shape[0] == 130
    nlz, g, H = gp.nll_hess_batch()
    gp2.update(hyp=hyp)
    nlz2, g2, H2 = gp2.nll_hess_batch()
    _, _, rH = _reference(gp2, hyp)
    _assert_parity(H, rH, what="appended")
    _assert_parity(H2, rH, what="fresh")
    assert np.all(np.abs(H - H2) <= 1e-8 * np.abs(H2).max())


def test_bit_identities():
    """H == H^T; a sample alone or in a batch of three; resident posteriors (hyp=None) or the same hyp passed."""
    gp, X, y, s2, hyp = _problem("rq", 0, "negquad", 130, 3, S=3)
    nlz, g, H = gp.nll_hess_batch(hyp)
    for s in range(3):
        assert np.array_equal(H[s], H[s].T)
        z1, g1, H1 = gp.nll_hess_batch(hyp[s:s + 1])
        assert np.array_equal(H1[0], H[s]) and np.array_equal(g1[0], g[s]) and z1[0] == nlz[s]
    gp.update(hyp=hyp)
    zr, gr, Hr = gp.nll_hess_batch()
    assert np.array_equal(Hr, H) and np.array_equal(gr, g) and np.array_equal(zr, nlz)


_CHILD = """
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from test_gpu_nll_hess import _problem
from gpyreg_amd import _lib
device_call = _lib.PostHandle.nll_hess
def reporting(self, *args):  # the chunk gpc_nll_hess planned (nll_hess_batch evaluates nlZ after it, which plans again)
    try:
        return device_call(self, *args)
    finally:
        print("LAST_CHUNK", self.ctx.get_option("last_chunk"))
_lib.PostHandle.nll_hess = reporting
gp, X, y, s2, hyp = _problem("matern", 3, "const", 130, 3, S=3)
try:
    nlz, g, H = gp.nll_hess_batch(hyp)
    np.save(sys.argv[1], H)
except RuntimeError as e:
    print("REFUSED:", e)
"""


def test_chunking_changes_no_bit_and_the_budget_refusal(tmp_path):
    """GPC_MEM_BUDGET_MB in child processes: budgets that fit one and two samples per chunk (a sample's scratch at
    N_pad = 256 with 5 planes is 7 N_pad^2 doubles = 3.7 MB and vectors; the planner takes 80 %) give the bits of the
    unchunked call; 2 MB fits no sample and is refused with the sizes in the message.  Each child reports the chunk the
    library planned ("last_chunk"): it is the one that the scratch's closed form (scratch_sizes.nll_hess_per) gives."""
    from scratch_sizes import nll_hess_per, planned_chunk

    gp, X, y, s2, hyp = _problem("matern", 3, "const", 130, 3, S=3)
    _, _, H = gp.nll_hess_batch(hyp)
    cov_N, noise_N, mean_N = gp._counts()
    per = nll_hess_per(256, cov_N, noise_N, mean_N, 3 * 4 // 2)
    assert [planned_chunk(3, mb, per) for mb in (6, 11, 2)] == [1, 2, 0]
    script = tmp_path / "child.py"
    script.write_text(_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests")))
    for mb, refused in ((6, False), (11, False), (2, True)):
        out = tmp_path / f"h{mb}.npy"
        env = dict(os.environ, GPC_MEM_BUDGET_MB=str(mb))
        r = subprocess.run([sys.executable, str(script), str(out)], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert f"LAST_CHUNK {planned_chunk(3, mb, per)}\n" in r.stdout, r.stdout
        if refused:
            # (with the scratch's size to the byte: the closed form pins every array of the layout, not only the chunk)
            assert "REFUSED" in r.stdout and f"gpc_nll_hess: the scratch of one sample ({per} bytes:" in r.stdout
            assert "N_pad = 256" in r.stdout and "planes = 5" in r.stdout
        else:
            assert np.array_equal(np.load(out), H), mb


@pytest.mark.parametrize("kernel,degree,mean,per_point", [("se", 0, "negquad", False), ("matern", 5, "const", True),
                                                          ("rq", 0, "zero", False), ("matern_iso", 3, "const", False)])
def test_gradient_and_central_differences(kernel, degree, mean, per_point):
    """dnlZ against nll_batch(compute_grad=True) at 1e-10 relative (to the gradient's largest entry), and H against
    central differences of those gradients at the differences' own accuracy: 1e-5 max|H| with step 1e-4 (a sanity
    check, not the parity test)."""
    gp, X, y, s2, hyp = _problem(kernel, degree, mean, 130, 3, S=2)
    nlz, g, H = gp.nll_hess_batch(hyp)
    z0, g0 = gp.nll_batch(hyp, compute_grad=True)
    assert np.all(np.abs(g - g0) <= 1e-10 * np.abs(g0).max(1, keepdims=True)), np.abs(g - g0).max()
    assert np.all(np.abs(nlz - z0) <= 1e-12 * np.abs(z0))
    P = hyp.shape[1]
    step = 1e-4
    for s in range(hyp.shape[0]):
        rows = np.repeat(hyp[s:s + 1], 2 * P, 0)
        rows[np.arange(P), np.arange(P)] += step
        rows[P + np.arange(P), np.arange(P)] -= step
        _, gg = gp.nll_batch(rows, compute_grad=True)
        fd = (gg[:P] - gg[P:]) / (2 * step)
        assert np.abs(H[s] - fd).max() <= 1e-5 * np.abs(H[s]).max(), np.abs(H[s] - fd).max() / np.abs(H[s]).max()


# ---- the Python layer ------------------------------------------------------------------------------------------------
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


def test_log_posterior_hess_with_priors():
    from gpyreg_amd import priors as pr

    gp, X, y, s2, hyp = _problem("matern", 5, "const", 50, 3, S=1)
    hp = _with_priors(gp)
    val, grad, hess = gp.log_posterior_hess(hyp[0])
    rz, rg, rH = _reference(gp, hyp)
    lp, dlp = pr.log_priors(hyp[0], hp, gp.lower_bounds, gp.upper_bounds, gp.normalization_constants, True)
    want = -rH[0] + np.diag(nh.prior_d2(hyp[0], hp, gp.lower_bounds, gp.upper_bounds))
    assert np.abs(hess - want).max() <= 1e-8 * np.abs(want).max()
    assert np.abs(grad - (-rg[0] + dlp)).max() <= 1e-8 * np.abs(rg[0]).max()
    assert abs(val - gp.log_posterior(hyp[0])) <= 1e-10 * abs(val)
    assert abs(val - (-rz[0] + lp)) <= 1e-9 * abs(val)
    assert np.array_equal(hess, hess.T)


def _map_problem():
    rng = np.random.default_rng(4)
    X = rng.uniform(-2, 2, (60, 2))
    y = np.sin(X[:, :1]) + 0.5 * np.cos(2 * X[:, 1:]) + 0.1 * rng.standard_normal((60, 1))
    gp = gpr.GP(2, gpr.covariance_functions.SquaredExponential(), gpr.mean_functions.ConstantMean(),
                gpr.noise_functions.GaussianNoise(constant_add=True))
    return gp, X, y


def test_laplace_at_a_fit_map():
    gp, X, y = _map_problem()
    gp.fit(X, y, options={"n_samples": 0, "opts_N": 2, "init_N": 256})
    la = gp.laplace_approximation()
    assert la["is_pd"] and la["cov"] is not None and np.isfinite(la["log_evidence"])
    k = la["free"].size
    assert np.array_equal(la["mean"], gp.posteriors[0].hyp) and la["hess"].shape == (k, k)
    assert np.abs(la["cov"] @ la["hess"] - np.eye(k)).max() <= 1e-8
    val, _, hess = gp.log_posterior_hess(la["mean"])
    assert np.array_equal(la["hess"], -hess[np.ix_(la["free"], la["free"])])
    sign, logdet = np.linalg.slogdet(la["hess"])
    assert sign > 0 and abs(la["log_evidence"] - (val + 0.5 * k * np.log(2 * np.pi) - 0.5 * logdet)) <= 1e-9 * abs(val)


def test_laplace_on_a_ridge_is_not_repaired():
    """Lengthscales far beyond the data's extent and a tiny signal variance: the kernel is all but constant, the
    objective is nearly flat along both lengthscales and the signal variance and curves the wrong way there (the float64
    restatement's eigenvalues: -1.1e-1, -1.0e-2, -4.4e-4, 2.2e2, 4.2e2), so the Hessian is not positive definite and
    nothing is returned in place of a covariance."""
    gp, X, y = _map_problem()
    gp.X, gp.y = X, y
    hyp = np.array([np.log(30.0), np.log(30.0), np.log(0.01), np.log(0.5), 0.0])  # tiny signal, long lengthscales
    la = gp.laplace_approximation(hyp)
    w = np.linalg.eigvalsh(la["hess"])
    print("ridge eigenvalues:", w)
    assert w.min() <= 0
    assert la["is_pd"] is False and la["cov"] is None and la["log_evidence"] is None


def test_refusals(ctx):
    gp, X, y, s2, hyp = _problem("se", 0, "const", 50, 3, S=1)
    zero, const = gpr.mean_functions.ZeroMean(), gpr.noise_functions.GaussianNoise(constant_add=True)

    class MyCov(gpr.covariance_functions.SquaredExponential):
        _gpc_kernel_id = None

    class MyNoise(gpr.noise_functions.GaussianNoise):
        pass

    class MyMean(gpr.mean_functions.ConstantMean):
        pass

    se = gpr.covariance_functions.SquaredExponential
    for other, msg in ((gpr.GP(3, gpr.covariance_functions.Matern(1), zero, const), "degree 1"),
                       (gpr.GP(3, se(), zero, const, dtype="f32"), "fp64 only"),
                       (gpr.GP(3, se(), zero, MyNoise(constant_add=True)), "noise function"),
                       (gpr.GP(3, se(), MyMean(), const), "mean function"),
                       (gpr.GP(3, MyCov(), zero, const), "covariance function")):
        other.X, other.y = X, y
        with pytest.raises(NotImplementedError, match=msg):
            other.nll_hess_batch(np.zeros((1, other._hyp_N())))
    # the library's own refusals, each with its message
    from gpyreg_amd import _lib

    gp.update(hyp=hyp)
    h = gp._post_handle
    with pytest.raises(ValueError, match="dsn2"):
        h.nll_hess(4, np.zeros((1, 50, 1)), np.zeros((1, 7, 1)))
    rc = ctx._lib.gpc_nll_hess(h._h, None, 1, None, 1, 0, None, None, None, None)  # mean_N = 1 without dm, no outputs
    assert rc == -2 and b"gpc_nll_hess: bad arguments" in ctx._lib.gpc_last_error(ctx._h)
    for kid, deg, dtype, msg in ((_lib.K_MATERN, 1, _lib.F64, "Matern kernel of degree 1"), (_lib.K_SE, 0, _lib.F32, "fp64 only")):
        cn = 4
        hh, _, _, info = ctx.posterior_batch(kid, deg, dtype, hyp[:, :cn], np.zeros((1, 50)), np.full((1, 1), 0.01), False)
        assert info[0] == 0
        with pytest.raises(RuntimeError, match=msg):
            hh.nll_hess(cn, None, np.full((1, 1, 1), 0.02))
        hh.free()
    K = gp.covariance.compute(hyp[0, :4], X)
    hk, _, _, _ = ctx.posterior_batch_K(_lib.F64, K[None], np.zeros((1, 50)), np.full((1, 1), 0.01), False)
    with pytest.raises(RuntimeError, match="caller-provided K"):
        hk.nll_hess(4, None, np.full((1, 1, 1), 0.02))
    hk.free()
