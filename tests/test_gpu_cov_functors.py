"""The covariance kernels of the evaluation and prediction paths, entry by entry, against np.longdouble.

``cov.compute`` runs the generic functor (covfun.h: pair_eval, library exp / sqrt / pow); the matrices the device
factors, contracts and predicts from come from build_kernel, small_front_kernel, trace_kernel and cross_tile_kernel
with the hand-written functors (pair_eval_t: Cody-Waite exp, rsq-based sqrt, exp(-a log M); pair_eval32 in fp32 mode:
hardware exp2 / log2 / rcp / sqrt on packed-fp32 distances).  gpc_debug_cov launches those kernels themselves on one
sample; every output is compared elementwise with the extended-precision reference, the distance ladder and the bound
of tests/test_cov_functors_cpu.py (derived there; its constants are not tuned), on every family and degree, both
dtypes, N in {70, 129, 200}, D in {1, 3, 33}, M in {1, 70}, and with every input shifted by 0, 1e2 and 1e4 length
scales.  The second half runs fp32 mode end to end through the public API on shifted inputs.

Measured on the MI355X, worst |error| / bound over all shapes and shifts (printed by the tests):

    family        dtype  build  front  cross  mu     sums: sf     ell    alpha  trace  diagQ
    se            f64    0.442  0.426  0.460  0.023        0.001  0.058  -      0.002  0.069
    se            f32    0.997  0.993  0.020  0.026        0.002  0.023  -      0.004  0.029
    se_iso        f64    0.438  0.414  0.463  0.024        0.001  0.010  -      0.002  0.069
    se_iso        f32    0.997  0.993  0.020  0.026        0.002  0.020  -      0.004  0.029
    matern1       f64    0.259  0.259  0.244  0.027        0.002  NaN    -      0.002  0.069
    matern1       f32    0.107  0.096  0.020  0.012        0.006  NaN    -      0.004  0.029
    matern3       f64    0.253  0.253  0.250  0.015        0.003  0.009  -      0.002  0.069
    matern3       f32    0.104  0.089  0.018  0.016        0.002  0.009  -      0.004  0.029
    matern5       f64    0.274  0.246  0.233  0.014        0.002  0.006  -      0.002  0.069
    matern5       f32    0.102  0.087  0.018  0.008        0.006  0.012  -      0.004  0.029
    matern_iso1   f64    0.259  0.259  0.257  0.027        0.002  NaN    -      0.002  0.069
    matern_iso1   f32    0.107  0.096  0.020  0.012        0.006  NaN    -      0.004  0.029
    matern_iso3   f64    0.253  0.253  0.213  0.015        0.003  0.005  -      0.002  0.069
    matern_iso3   f32    0.104  0.089  0.018  0.016        0.002  0.005  -      0.004  0.029
    matern_iso5   f64    0.245  0.245  0.233  0.014        0.004  0.001  -      0.002  0.069
    matern_iso5   f32    0.102  0.087  0.018  0.008        0.006  0.001  -      0.004  0.029
    rq  a = 0.7   f64    0.108  0.105  0.106  0.008        0.001  0.003  0.000  0.002  0.069
    rq  a = 0.7   f32    0.072  0.072  0.014  0.005        0.000  0.001  0.000  0.004  0.029
    rq  a = 150   f64    0.171  0.162  0.172  0.025        0.004  0.032  0.075  0.002  0.069
    rq  a = 150   f32    0.999  0.970  0.000  0.017        0.001  0.007  0.012  0.004  0.029

(The fp32 build entries at 0.97 - 0.999 for se and rq are values just below sf2 2^-126 that the hardware flushes to
zero: their error is their own size, which the floor term allows by construction; everywhere else fp32 stays below
0.11.  The fp64 figures of se are the rounding of r2 over D = 33 dimensions: NumPy's own evaluation measures 0.442.)
End to end (second half), fp32 mode, the same at every shift c in {0, 1e2, 1e4, 1e5}: se nlZ 5.9e-5, dnlZ 1.3e-5;
matern5 3.1e-6, 4.7e-6; rq 6.3e-5, 9.4e-6; predictions <= 1.7e-5.  fp64 control: <= 7e-13.
Before stage_x32 centred the coordinates and sqrt_fast scaled tiny arguments, these tests failed as follows: fp32
build entries at 2.5 (se, matern1) times the bound at a shift of 1e2 and 335 (se), 405 (matern1), 129 (rq 0.7), 119
(matern3) times at 1e4; NaN in the fp64 matrices of every Matern degree at shift 0 (the pair with r2 = 1e-320);
end to end at c = 1e4 nlZ off by 4.5e-3 (se) and 1.6e-2 (rq), predictive means by 1.8e-2.
"""

import functools

import numpy as np
import pytest

import test_cov_functors_cpu as cf
from test_cov_functors_cpu import F32, F64, LD

pytestmark = pytest.mark.gpu

DT_NAME = {F64: "f64", F32: "f32"}
KSCALE = 0.02  # sl = sn2 * mult of a sample with sigma_n ~ 0.14
WORST = {}


@pytest.fixture(scope="module")
def ctx():
    from gpyreg_amd import _lib

    return _lib.context(0)


def _note(what, name, alpha, dtype, ratio):
    key = (what, name if alpha is None else "%s(a=%g)" % (name, alpha), DT_NAME[dtype])
    WORST[key] = max(WORST.get(key, 0.0), ratio)


@functools.lru_cache(maxsize=2)
def _problem(name, alpha, N, D, shift):
    kind, degree = cf.FAMILIES[name]
    hyp = cf.make_hyp(kind, D, alpha)
    mul, dv, sf2, rqa = cf.scaling(kind, degree, D, hyp)
    X = cf.ladder_inputs(kind, degree, N, D, hyp, shift)
    xs = cf.scale(X, mul, dv)
    ref = cf.reference(kind, degree, xs, xs, sf2, rqa)
    dr2, pieces = cf.stage_dr2(xs, xs, xs[0])
    return dict(kind=kind, degree=degree, hyp=hyp, mul=mul, dv=dv, sf2=sf2, rqa=rqa, X=X, xs=xs, ref=ref, dr2=dr2,
                pieces=pieces)


def _scaled(ref, s):
    return dict(ref, K=ref["K"] / LD(s), F=ref["F"] / LD(s))


def _check_xs(xs_dev, xs):
    N = xs.shape[0]
    assert np.array_equal(xs_dev[:N], xs), "the device's scaled inputs are not NumPy's X * mul / dv to the bit"
    assert not xs_dev[N:].any()


def _check_build(A, p, N, dtype, dvec, name, alpha, what):
    kind, ref = p["kind"], _scaled(p["ref"], KSCALE)
    npad = A.shape[0]
    assert np.isfinite(A).all(), (what, name, "NaN / inf in the matrix")
    pad = np.zeros((npad, npad), bool)
    pad[N:, :] = pad[:, N:] = True
    eye = np.eye(npad, dtype=bool)
    assert (A[pad & ~eye] == 0).all() and (A[pad & eye] == 1).all(), (what, name, "padding is not the identity")
    bound = cf.entry_bound(kind, ref, p["sf2"] / KSCALE, p["rqa"], dtype, p["dr2"] if dtype == F32 else None)
    got = A[:N, :N].copy()
    d = np.arange(N)
    # the diagonal carries dvec: remove it in extended precision, its own rounding (one eps of the stored sum) allowed
    diag_slack = cf.EPS[dtype] * np.abs(got[d, d])
    low = np.tril(np.ones((N, N), bool), -1)
    err = np.abs(got.astype(LD) - ref["K"]).astype(np.float64)
    r_off = float((err[low] / bound[low]).max())
    err_d = np.abs(got[d, d].astype(LD) - dvec.astype(LD) - ref["K"][d, d]).astype(np.float64)
    r_diag = float((err_d / (bound[d, d] + diag_slack)).max())
    _note(what, name, alpha, dtype, max(r_off, r_diag))
    assert r_off <= 1.0 and r_diag <= 1.0, (what, name, alpha, DT_NAME[dtype], r_off, r_diag,
                                            np.argwhere(low & (err > bound))[:5].tolist())


def _check_cross(ctx, p, N, D, M, dtype, shift, name, alpha, A1):
    kind, degree = p["kind"], p["degree"]
    Xq, same = cf.query_inputs(kind, degree, p["X"], M, p["hyp"], shift)
    rng = np.random.default_rng(N + M)
    al = rng.standard_normal(N)
    Ks, mu, (xs_dev, xss_dev) = ctx.debug_cov("cross", kind, degree, p["hyp"], p["X"], dtype=dtype, X_star=Xq, vec=al)
    xss = cf.scale(Xq, p["mul"], p["dv"])
    _check_xs(xs_dev, p["xs"])
    _check_xs(xss_dev, xss)
    assert np.isfinite(Ks).all() and np.isfinite(mu).all(), (name, "NaN / inf in the cross covariance")
    assert not Ks[N:].any() and not Ks[:, M:].any() and not mu[M:].any(), (name, "cross padding is not zero")
    ref = cf.reference(kind, degree, p["xs"], xss, p["sf2"], p["rqa"])
    bound = cf.entry_bound(kind, ref, p["sf2"], p["rqa"], dtype)
    r = cf.worst_ratio(Ks[:N, :M], ref["K"], bound)
    _note("cross", name, alpha, dtype, r)
    assert r <= 1.0, ("cross", name, alpha, DT_NAME[dtype], N, D, M, r)
    # the fused mean product, from the STORED values: a sum of N terms in a tree of depth < 64
    terms = Ks[:N, :M].astype(LD) * al.astype(LD)[:, None]
    mu_ref = terms.sum(0)
    mu_bound = 64 * cf.EPS[F64] * np.abs(terms).sum(0).astype(np.float64) + 2.0 ** -1022
    r_mu = float((np.abs(mu[:M].astype(LD) - mu_ref).astype(np.float64) / mu_bound).max())
    _note("cross mu", name, alpha, dtype, r_mu)
    assert r_mu <= 1.0, ("cross mu", name, alpha, DT_NAME[dtype], r_mu)
    if dtype == F64:  # a query point that is a training point gets the training matrix's value, to the bit
        for j, r0 in enumerate(same):
            col = np.where(np.arange(N) > r0, A1[:N, r0], A1[r0, :N])
            off = np.arange(N) != r0
            assert np.array_equal(Ks[:N, j][off], col[off]), ("cross vs build bits", name, alpha, N, D, j, r0)


def _check_trace(ctx, p, N, D, dtype, name, alpha):
    kind, degree, ref = p["kind"], p["degree"], p["ref"]
    rng = np.random.default_rng(3 * N + D)
    T = rng.standard_normal((N, N))
    T = (T + T.T) / 2
    a = rng.standard_normal(N)
    if dtype == F32:  # T is stored, and a is read, as float: the reference uses the rounded values
        T, a = T.astype(np.float32).astype(np.float64), a.astype(np.float32).astype(np.float64)
    sl = KSCALE
    sums, diagq, xs_dev = ctx.debug_cov("trace", kind, degree, p["hyp"], p["X"], dtype=dtype, sl=sl, mat=T, vec=a)
    _check_xs(xs_dev, p["xs"])
    eps, C = cf.EPS[dtype], cf.CBOUND[dtype]
    Q = T.astype(LD) / LD(sl) - np.outer(a.astype(LD), a.astype(LD))
    Qmag = np.abs(T) / sl + np.abs(np.outer(a, a))  # Q's own rounding is relative to its two terms
    w = np.tril(np.full((N, N), 2.0), -1) + np.eye(N)  # lower triangle, off-diagonal pairs twice
    d = np.arange(N)
    # diag(Q) and its trace
    assert not diagq[N:].any()
    r_dq = float((np.abs(diagq[:N].astype(LD) - Q[d, d]).astype(np.float64) / (C * eps * Qmag[d, d])).max())
    _note("trace diagQ", name, alpha, dtype, r_dq)
    assert r_dq <= 1.0, ("diagQ", name, alpha, DT_NAME[dtype], r_dq)
    rel = cf.rel_bound(kind, ref, p["rqa"], dtype)
    tail = (64 * eps) if dtype == F64 else 16 * eps
    floor = cf.floor_of(p["sf2"], dtype)
    dr2 = p["dr2"] if dtype == F32 else np.zeros((N, N))
    K, F = np.abs(ref["K"]).astype(np.float64), np.abs(ref["F"]).astype(np.float64)
    r2 = ref["r2"].astype(np.float64)

    def check(slot, terms_ld, mag, stage, label):
        """terms_ld: the signed terms w Q dK/dtheta (longdouble); mag >= |dK/dtheta| per entry; stage: its fp32 staging
        error per entry.  |sum_dev - sum_ld| <= sum_ij w |Q|_ij (rel_ij mag_ij + stage_ij + floor) + tail sum w |Q| mag."""
        wq = w * Qmag
        bound = float((wq * (rel * mag + stage + floor)).sum() + tail * (wq * mag).sum())
        err = float(abs(LD(sums[slot]) - terms_ld.sum()))
        _note("trace " + label, name, alpha, dtype, err / bound)
        assert np.isfinite(sums[slot]) and err <= bound, ("trace " + label, name, alpha, DT_NAME[dtype], N, D, err / bound)

    iso = cf.is_iso(kind)
    P = cf.cov_count(kind, D) + 1
    assert sums.shape == (P,)
    wQ = LD(1) * w * Q
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        half_f_dr2 = np.where(dr2 > 0, F / 2 * dr2, 0.0)
        # dF/dr2 relative to F: 1/2 (SE, Matern 5), 1/(2t) (Matern 3), (1 + 1/a)/2 (rq)
        g = 0.5 + (np.where(r2 > 0, 0.5 / np.sqrt(r2), 0.0) if degree == 3 else 0.0) + (0.5 / p["rqa"] if kind == cf.K_RQ else 0.0)
        f_stage = np.where(dr2 > 0, F * g * dr2, 0.0)
    sf_slot = 1 if iso else D
    check(sf_slot, wQ * 2 * ref["K"], 2 * K, 2 * half_f_dr2, "sf")
    tr_err = float(abs(LD(sums[P - 1]) - Q[d, d].sum()))
    tr_bound = float((C * eps + tail) * Qmag[d, d].sum())
    _note("trace trQ", name, alpha, dtype, tr_err / tr_bound)
    assert tr_err <= tr_bound, ("trace(Q)", name, alpha, DT_NAME[dtype], tr_err / tr_bound)
    if kind == cf.K_RQ:
        al = p["rqa"]
        M = 1 + r2 / (2 * al)
        hmag = r2 / (2 * M) + al * np.log1p(r2 / (2 * al))  # the two terms of Ka / K cancel: the error is relative to them
        ka_stage = (F / 2 * hmag + K * r2 / (4 * al * M * M)) * dr2
        check(D + 1, wQ * ref["Ka"], K * hmag, ka_stage, "alpha")
    ls_slots = [0] if iso else list(range(D))
    if degree == 1:  # F = 1/t is +inf on the diagonal and inf * 0 = NaN, by the reference's definition
        assert np.isnan(sums[ls_slots]).all(), (name, "Matern-1 length-scale sums must be NaN, as the reference's are")
    else:
        for l in ls_slots:
            d2 = ref["r2"] if iso else ref["d2"][:, :, l]
            d2_stage = dr2 if iso else p["pieces"][:, :, l]
            d2f = d2.astype(np.float64)
            stage = (f_stage * d2f + F * d2_stage) if dtype == F32 else np.zeros((N, N))
            check(l, wQ * ref["F"] * d2, F * d2f, stage, "ell")
    others = np.ones(P, bool)
    if degree == 1:
        others[ls_slots] = False
    assert np.isfinite(sums[others]).all() and np.isfinite(diagq).all(), (name, "NaN outside Matern-1's length-scale sums")


def _cases():
    return [pytest.param(name, alpha, id=name if alpha is None else "%s-a%g" % (name, alpha))
            for name, _, _, alpha in cf.family_cases()]


@pytest.mark.parametrize("shift", cf.SHIFTS)
@pytest.mark.parametrize("name,alpha", _cases())
def test_production_covariance_kernels_elementwise(ctx, name, alpha, shift):
    for N, D in cf.SHAPES:
        p = _problem(name, alpha, N, D, shift)
        kind, degree = p["kind"], p["degree"]
        dvec = np.random.default_rng(N).uniform(1.0, 2.0, N)
        A1 = None
        for dtype in (F64, F32):
            A, xs_dev = ctx.debug_cov("build", kind, degree, p["hyp"], p["X"], dtype=dtype, kscale=KSCALE, dvec=dvec)
            _check_xs(xs_dev, p["xs"])
            _check_build(A, p, N, dtype, dvec, name, alpha, "build")
            if N <= 128:  # the one-leaf front builds the same tiles from inputs it scales itself
                Af, xs_f = ctx.debug_cov("front", kind, degree, p["hyp"], p["X"], dtype=dtype, kscale=KSCALE, dvec=dvec)
                _check_xs(xs_f, p["xs"])
                _check_build(Af, p, N, dtype, dvec, name, alpha, "front")
                assert np.array_equal(Af, A), ("front vs build bits", name, alpha, DT_NAME[dtype])
            if dtype == F64:
                A1, _ = ctx.debug_cov("build", kind, degree, p["hyp"], p["X"], dtype=F64, kscale=1.0, dvec=np.zeros(N))
            for M in (1, 70):
                _check_cross(ctx, p, N, D, M, dtype, shift, name, alpha, A1)
            _check_trace(ctx, p, N, D, dtype, name, alpha)
    mine = {k: v for k, v in WORST.items() if k[1] == (name if alpha is None else "%s(a=%g)" % (name, alpha))}
    for k in sorted(mine):
        print("worst err/bound so far  %-12s %-16s %s  %.3f" % (k[0], k[1], k[2], mine[k]))


# ---- end to end: fp32 mode through the public API on shifted inputs ------------------------------------------------

E2E = {"se": ("se", 0), "matern5": ("matern", 5), "rq": ("rq", 0)}


def _gp(kernel, dtype):
    import gpyreg_amd as gpr

    cov = {"se": gpr.covariance_functions.SquaredExponential, "matern5": lambda: gpr.covariance_functions.Matern(5),
           "rq": gpr.covariance_functions.RationalQuadraticARD}[kernel]()
    return gpr.GP(2, cov, gpr.mean_functions.ConstantMean(), gpr.noise_functions.GaussianNoise(constant_add=True),
                  dtype=dtype)


@functools.lru_cache(maxsize=None)
def _e2e_reference(kernel, c):
    from oracle import gp_oracle as orc

    rng = np.random.default_rng(11)
    N, D, S = 300, 2, 2
    X0 = rng.uniform(-3, 3, (N, D))
    y = np.sin(X0.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
    X = X0 + c
    xq = rng.uniform(-3, 3, (9, D)) + c
    kname, degree = E2E[kernel]
    cov = [np.log(0.5)] * D + [0.0] + ([np.log(2.0)] if kname == "rq" else [])
    hyp = np.array(cov + [np.log(0.1), 0.3])
    hyp = hyp + 0.05 * rng.standard_normal((S, hyp.size))
    model = dict(kernel=kname, degree=degree, mean="const", noise=(1, 0, 0))
    core = [orc.core(model, hyp[s], X, y, None, 1, 1) for s in range(S)]
    posts = orc.posteriors(model, hyp, X, y, None)
    rmu, rs2 = orc.predict(model, posts, X, y, xq, separate_samples=True)
    return X, y, xq, hyp, core, rmu, rs2, len(cov)


@pytest.mark.parametrize("dtype,bar", [("f32", 1e-3), ("f64", 1e-8)])
@pytest.mark.parametrize("kernel", list(E2E))
def test_shifted_inputs_through_the_public_api(kernel, dtype, bar):
    """nll_batch and predict on inputs uniform in c + [-3, 3] (ell = 0.5) against the fp64 reference implementation on
    the same inputs: fp32 mode at the project's 1e-3 bar, flat in c; fp64 at 1e-8 as the control."""
    for c in (0.0, 1e2, 1e4, 1e5):
        X, y, xq, hyp, core, rmu, rs2, cov_N = _e2e_reference(kernel, c)
        gp = _gp(kernel, dtype)
        gp.update(X_new=X, y_new=y, hyp=hyp)
        nlz, dnlz = gp.nll_batch(hyp, compute_grad=True)
        mu, s2 = gp.predict(xq, separate_samples=True)
        e_n = e_d = 0.0
        for s in range(hyp.shape[0]):
            rn, rd = core[s]
            e_n = max(e_n, abs(nlz[s] - rn) / max(1.0, abs(rn)))
            e_d = max(e_d, (np.abs(dnlz[s] - rd) / np.maximum(np.abs(rd), np.abs(rd).max())).max())
        sf2 = np.exp(2 * hyp[:, 2]).max()
        e_mu = np.abs(mu - rmu).max() / max(1.0, np.abs(rmu).max())
        e_s2 = np.abs(np.maximum(s2, 0) - rs2).max() / sf2
        print("%s %s c = %-6g nlZ %.1e  dnlZ %.1e  mu %.1e  s2 %.1e" % (kernel, dtype, c, e_n, e_d, e_mu, e_s2))
        assert e_n <= bar and e_d <= bar and e_mu <= bar and e_s2 <= bar, (kernel, dtype, c, e_n, e_d, e_mu, e_s2)
