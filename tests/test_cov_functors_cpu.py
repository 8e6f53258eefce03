"""The distance ladder, the extended-precision reference and the per-entry error bound of the covariance functors
that build the matrices the device factors (covfun.h: pair_eval_t in fp64, pair_eval32 in fp32 mode), and CPU checks
that the bound is sound.  tests/test_gpu_cov_functors.py imports everything here and applies it to the device.

Reference: np.longdouble (64-bit mantissa) arithmetic on the SAME fp64 scaled coordinates the device uses --
``X * mul / dv`` in scale_x_kernel's order is reproducible to the bit, so the rounding of the scaling is not part of
the error under test.

Bound for one entry K_ij (C = 8, eps = 2^-52 in fp64; C = 16, eps = 2^-23 in fp32):

    |K_dev - K_ld| <= C eps (1 + a_rq + |arg|) |K_ld|  +  |dK/dr2| dr2_stage  +  floor

  * arg is the argument of the final exponential (-r2/2, -t, -alpha log M): a relative error delta of it is a
    relative error |arg| delta of K, and r2 itself carries a few eps from the differences and the sum;
  * a_rq = alpha for the rational quadratic (0 otherwise): rounding M = 1 + r2/(2 alpha) to eps moves
    alpha log M by up to alpha eps;
  * dr2_stage (fp32 mode only) = sum_l 2 |d_l| ulp32(|xs_l - centre_l|): the scaled coordinates are rounded to float
    AFTER the sample's row 0 is subtracted (stage_x32), each to half an ulp, so d_l moves by at most one ulp of the
    larger of its two staged coordinates; dK/dr2 = -F/2 for every family;
  * floor: a few of the smallest subnormals times sf2 in fp64 (gradual underflow of the last product); sf2 2^-126 in
    fp32, where results below the smallest normal may be flushed to zero.

The CPU checks: NumPy's own fp64 evaluation and an fp32 emulation of the staged path stay below HALF that bound on
every family, shape and shift of the ladder (so the bound has room for a correct implementation and none for a wrong
one), and the emulation of uncentred fp32 staging documents why the staging is centred: at c / ell = 2e4 it alone costs
more than the project's 1e-3 fp32 bar.
"""

import math

import numpy as np
import pytest

LD = np.longdouble
K_SE, K_MATERN, K_RQ, K_SE_ISO, K_MATERN_ISO = range(5)
F64, F32 = 0, 1

# name -> (kernel id, Matern degree)
FAMILIES = {
    "se": (K_SE, 0), "se_iso": (K_SE_ISO, 0), "rq": (K_RQ, 0),
    "matern1": (K_MATERN, 1), "matern3": (K_MATERN, 3), "matern5": (K_MATERN, 5),
    "matern_iso1": (K_MATERN_ISO, 1), "matern_iso3": (K_MATERN_ISO, 3), "matern_iso5": (K_MATERN_ISO, 5),
}
RQ_ALPHAS = (0.7, 150.0)
SHIFTS = (0.0, 1e2, 1e4)  # c / ell
# scaled offsets of the first rows from row 0 along dimension 0: an exact duplicate, subnormal r2 (1e-160), tiny r2,
# the bulk, SE's K in the subnormal range (38.5) and at exactly 0 (39.2), and every family's K at exactly 0 (1e3)
LADDER = (0.0, 1e-160, 1e-150, 1e-8, 1e-3, 0.1, 1.0, 5.0, 12.0, 27.0, 37.5, 38.5, 39.2, 1e3)
SHAPES = ((70, 1), (70, 3), (129, 3), (200, 3), (70, 33), (200, 33))  # N in {70, 129, 200} x D in {1, 3, 33}

EPS = {F64: 2.0 ** -52, F32: 2.0 ** -23}
CBOUND = {F64: 8.0, F32: 16.0}


def is_iso(kind):
    return kind in (K_SE_ISO, K_MATERN_ISO)


def cov_count(kind, D):
    return 2 if is_iso(kind) else (D + 2 if kind == K_RQ else D + 1)


def make_hyp(kind, D, alpha=None):
    """log length scales (spread over a factor 1.6 around 0.5), log sf (sf2 = 1.69), log alpha."""
    if is_iso(kind):
        return np.array([math.log(0.5), math.log(1.3)])
    ell = [0.5 * (0.8 + 0.8 * h / max(D - 1, 1)) for h in range(D)]
    tail = [math.log(1.3)] + ([math.log(alpha)] if kind == K_RQ else [])
    return np.array([math.log(e) for e in ell] + tail)


def scaling(kind, degree, D, hyp):
    """mul, dv, sf2, alpha as the library derives them (gpcore.hip: scaling_of) -- math.exp and the C library's exp
    are the same function, so these are the library's values to the bit."""
    snu = math.sqrt(float(degree))
    if is_iso(kind):
        ell = math.exp(hyp[0])
        return (np.full(D, snu if kind == K_MATERN_ISO else 1.0), np.full(D, ell), math.exp(2 * hyp[1]), 1.0)
    sf2 = math.exp(2 * hyp[D])
    rqa = math.exp(hyp[D + 1]) if kind == K_RQ else 1.0
    ell = np.array([math.exp(h) for h in hyp[:D]])
    if kind == K_SE:
        return np.ones(D), ell, sf2, rqa
    if kind == K_MATERN:
        return snu / ell, np.ones(D), sf2, rqa
    return 1.0 / ell, np.ones(D), sf2, rqa


def scale(X, mul, dv):
    return X * mul / dv  # scale_x_kernel: (X * mul) / dv


def ladder_inputs(kind, degree, N, D, hyp, shift, seed=0):
    """X (N, D): row 0 at the origin, rows 1 .. len(LADDER)-1 equal to it except along dimension 0, where their SCALED
    offsets are LADDER; the other rows uniform in +-3 length scales; rows 63 and 64 an exact duplicate across the border
    of the first two 64-tiles.  Then every input is shifted by ``shift`` length scales in every dimension."""
    mul, dv, _, _ = scaling(kind, degree, D, hyp)
    unit = dv / mul  # one scaled unit, in input units
    rng = np.random.default_rng(1000 * N + D + seed)
    X = rng.uniform(-3, 3, (N, D)) * unit
    X[:len(LADDER)] = 0.0
    X[:len(LADDER), 0] = np.array(LADDER) * unit[0]
    X[64] = X[63]
    return X + shift * unit


def query_inputs(kind, degree, X, M, hyp, shift, seed=0):
    """X* (M, D): the first rows ARE training rows (the ladder's 5.0 row, then -- M permitting -- its duplicate row, its
    subnormal-offset row, a bulk row and the row behind the tile border), the rest uniform in +-3 length scales."""
    N, D = X.shape
    mul, dv, _, _ = scaling(kind, degree, D, hyp)
    unit = dv / mul
    rng = np.random.default_rng(77 * M + D + seed)
    Xq = rng.uniform(-3, 3, (M, D)) * unit + shift * unit
    same = [7, 0, 1, 40, 64][:min(M, 5)]
    Xq[:len(same)] = X[same]
    return Xq, same


def reference(kind, degree, xa, xb, sf2, rqa):
    """Extended-precision functor on fp64 scaled coordinates xa (n, D), xb (m, D): dict of (n, m) longdouble arrays
    K, F (dK/dlog ell_l = F d_l), Ka (rq), r2, arg, and d2 (n, m, D) = the squared differences."""
    a, b = xa.astype(LD), xb.astype(LD)
    d = a[:, None, :] - b[None, :, :]
    d2 = d * d
    r2 = d2.sum(-1)
    sf2, al = LD(sf2), LD(rqa)
    Ka = np.zeros_like(r2)
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind in (K_SE, K_SE_ISO):
            arg = -r2 / 2
            K = sf2 * np.exp(arg)
            F = K
        elif kind in (K_MATERN, K_MATERN_ISO):
            t = np.sqrt(r2)
            arg = -t
            e = sf2 * np.exp(arg)
            if degree == 1:
                K, F = e, e / t  # +inf where r2 = 0, as the reference implementation defines it
            elif degree == 3:
                K, F = e * (1 + t), e
            else:
                K, F = e * (1 + t + t * t / 3), e * (1 + t) / 3
        else:
            lM = np.log1p(r2 / (2 * al))
            M = 1 + r2 / (2 * al)
            arg = -al * lM
            K = sf2 * np.exp(arg)
            F = K / M
            Ka = K * (r2 / (2 * M) - al * lM)
    return dict(K=K, F=F, Ka=Ka, r2=r2, arg=arg, d2=d2, d=d)


def ulp32(v):
    """Spacing of float32 at |v| (fp64 in, fp64 out); below the smallest normal a conversion may flush: 2^-126."""
    return np.maximum(np.spacing(np.abs(v).astype(np.float32)).astype(np.float64), 2.0 ** -126)


def stage_dr2(xa, xb, centre):
    """(dr2_stage (n, m), per-dimension pieces (n, m, D)) of centred fp32 staging."""
    ua, ub = ulp32(xa - centre), ulp32(xb - centre)
    d = np.abs(xa[:, None, :] - xb[None, :, :])
    pieces = 2 * d * np.maximum(ua[:, None, :], ub[None, :, :])
    return pieces.sum(-1), pieces


def rel_bound(kind, ref, rqa, dtype):
    """The relative part C eps (1 + a_rq + |arg|) of the entry bound, (n, m) fp64."""
    a_rq = rqa if kind == K_RQ else 0.0
    return CBOUND[dtype] * EPS[dtype] * (1.0 + a_rq + np.abs(ref["arg"]).astype(np.float64))


def floor_of(sf2, dtype):
    return 4 * 2.0 ** -1074 * max(sf2, 1.0) if dtype == F64 else max(sf2, 1.0) * 2.0 ** -126


def entry_bound(kind, ref, sf2, rqa, dtype, dr2=None):
    """Bound on |K_dev - K_ld| per entry (fp64 array); ``dr2``: the staging term's dr2_stage (fp32 staged paths)."""
    b = rel_bound(kind, ref, rqa, dtype) * np.abs(ref["K"]).astype(np.float64) + floor_of(sf2, dtype)
    if dr2 is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            half_f = np.abs(ref["F"]).astype(np.float64) / 2
            b = b + np.where(dr2 > 0, half_f * dr2, 0.0)
    return b


def worst_ratio(got, ref_K, bound):
    """max |got - ref| / bound over the finite reference entries (NaN / inf patterns are asserted separately)."""
    fin = np.isfinite(ref_K.astype(np.float64))
    err = np.abs(got.astype(LD) - ref_K)[fin].astype(np.float64)
    return float((err / bound[fin]).max()) if fin.any() else 0.0


# ---- CPU evaluations that must themselves stay inside the bound ---------------------------------------------------

def numpy_functor64(kind, degree, xa, xb, sf2, rqa):
    """The generic fp64 functor (covfun.h: pair_eval) in NumPy: squared differences summed in ascending dimension."""
    r2 = np.zeros((xa.shape[0], xb.shape[0]))
    for h in range(xa.shape[1]):
        d = xa[:, None, h] - xb[None, :, h]
        r2 = r2 + d * d
    if kind in (K_SE, K_SE_ISO):
        return sf2 * np.exp(-r2 / 2)
    if kind in (K_MATERN, K_MATERN_ISO):
        t = np.sqrt(r2)
        f = {1: 1.0, 3: 1 + t, 5: 1 + t * (1 + t / 3)}[degree]
        return sf2 * f * np.exp(-t)
    return sf2 * np.power(1 + r2 * (0.5 / rqa), -rqa)


def emulate_functor32(kind, degree, xs, sf2, rqa, centre):
    """fp32 mode's build in float32 NumPy: centred staging, even and odd dimensions summed separately, exp2 / log2."""
    f = np.float32
    st = (xs - centre).astype(f)
    acc = [np.zeros((xs.shape[0],) * 2, f), np.zeros((xs.shape[0],) * 2, f)]
    for h in range(xs.shape[1]):
        d = st[:, None, h] - st[None, :, h]
        acc[h & 1] = d * d + acc[h & 1]
    r2 = acc[0] + acc[1]
    log2e = f(1.4426950408889634)
    sf2 = f(sf2)
    with np.errstate(under="ignore"):
        if kind in (K_SE, K_SE_ISO):
            return sf2 * np.exp2(r2 * (f(-0.5) * log2e))
        if kind in (K_MATERN, K_MATERN_ISO):
            t = np.sqrt(r2)
            e = sf2 * np.exp2(t * -log2e)
            return {1: e, 3: t * e + e, 5: e * (t * (t * f(1 / 3) + f(1)) + f(1))}[degree]
        Mv = r2 * f(0.5 / rqa) + f(1)
        return sf2 * np.exp2(-f(rqa) * np.log2(Mv))


def family_cases():
    for name, (kind, degree) in FAMILIES.items():
        for alpha in (RQ_ALPHAS if kind == K_RQ else (None,)):
            yield name, kind, degree, alpha


def test_longdouble_is_wider_than_double():
    assert np.finfo(LD).eps <= 2.0 ** -63, "the reference of these tests needs an extended-precision long double"


def test_ladder_reaches_the_ends_of_the_functors_domain():
    kind, degree = FAMILIES["se"]
    hyp = make_hyp(kind, 3)
    mul, dv, sf2, rqa = scaling(kind, degree, 3, hyp)
    xs = scale(ladder_inputs(kind, degree, 70, 3, hyp, 0.0), mul, dv)
    ref = reference(kind, degree, xs, xs, sf2, rqa)
    r2, K = ref["r2"][0].astype(np.float64), ref["K"][0].astype(np.float64)
    assert r2[0] == 0 and 0 < r2[1] < 2.0 ** -1022 and r2[1] == np.float64(ref["r2"][0, 1])  # exact duplicate; subnormal r2
    assert 0 < K[11] < 2.0 ** -1022 and K[12] == 0 and K[13] == 0  # subnormal K, then exactly 0
    assert np.array_equal(xs[63], xs[64]) and ref["r2"][63, 64] == 0


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("N,D", SHAPES)
def test_numpy_evaluations_stay_inside_half_the_bound(N, D, shift):
    """NumPy fp64, and the float32 emulation of fp32 mode with centred staging, against longdouble on the ladder:
    the bound the device is held to leaves a correct implementation a factor two."""
    for name, kind, degree, alpha in family_cases():
        hyp = make_hyp(kind, D, alpha)
        mul, dv, sf2, rqa = scaling(kind, degree, D, hyp)
        xs = scale(ladder_inputs(kind, degree, N, D, hyp, shift), mul, dv)
        ref = reference(kind, degree, xs, xs, sf2, rqa)
        with np.errstate(under="ignore"):
            k64 = numpy_functor64(kind, degree, xs, xs, sf2, rqa)
        r64 = worst_ratio(k64, ref["K"], entry_bound(kind, ref, sf2, rqa, F64))
        dr2, _ = stage_dr2(xs, xs, xs[0])
        k32 = emulate_functor32(kind, degree, xs, sf2, rqa, xs[0])
        r32 = worst_ratio(k32, ref["K"], entry_bound(kind, ref, sf2, rqa, F32, dr2))
        assert np.isfinite(k64).all() and np.isfinite(k32).all(), (name, alpha)
        assert r64 <= 0.5 and r32 <= 0.5, (name, alpha, r64, r32)


def _nll_and_grad(K, dKs, y, sn2):
    A = K + sn2 * np.eye(len(y))
    L = np.linalg.cholesky(A)
    a = np.linalg.solve(A, y)
    nll = 0.5 * y @ a + np.log(np.diag(L)).sum() + 0.5 * len(y) * np.log(2 * np.pi)
    Q = np.linalg.inv(A) - np.outer(a, a)
    return nll, np.array([0.5 * (Q * dK).sum() for dK in dKs] + [sn2 * np.trace(Q)])


def _staged_se(xs, dt, centre):
    """SE (sf2 = 1) from coordinates rounded to ``dt`` after ``centre`` is subtracted; differences and r2 in ``dt``,
    everything after in fp64: the cost of the staging alone."""
    st = (xs - centre).astype(dt)
    d = st[:, None, :] - st[None, :, :]
    d2 = (d * d).astype(dt)
    K = np.exp(-0.5 * d2.sum(-1, dtype=dt).astype(np.float64))
    return K, [K * d2[:, :, l].astype(np.float64) for l in range(xs.shape[1])] + [2 * K]


def test_uncentred_fp32_staging_breaks_translation_invariance_and_centred_staging_does_not():
    """Why stage_x32 subtracts the sample's row 0 before it rounds to float: SE, D = 2, N = 300, ell = 0.5,
    sigma_n = 0.1, inputs uniform in c + [-3, 3].  Rounding the scaled coordinates themselves costs 1e-3 of nlZ or of
    its gradient at c / ell = 2e4 (the whole fp32 budget, before the fp32 factorization adds its own error); rounding
    them relative to row 0 costs the same ~1e-6 at every c."""
    rng = np.random.default_rng(0)
    N, D, ell, sn = 300, 2, 0.5, 0.1
    X0 = rng.uniform(-3, 3, (N, D))
    y = np.sin(X0.sum(1)) + sn * rng.standard_normal(N)

    def errs(n, g, n64, g64):
        return abs(n - n64) / max(1.0, abs(n64)), (np.abs(g - g64) / np.maximum(np.abs(g64), np.abs(g64).max())).max()

    for c in (0.0, 1e4):
        xs = (X0 + c) / ell
        n64, g64 = _nll_and_grad(*_staged_se(xs, np.float64, 0.0), y, sn ** 2)
        plain = errs(*_nll_and_grad(*_staged_se(xs, np.float32, 0.0), y, sn ** 2), n64, g64)
        centred = errs(*_nll_and_grad(*_staged_se(xs, np.float32, xs[0]), y, sn ** 2), n64, g64)
        print("c / ell = %g: uncentred nlZ %.1e dnlZ %.1e | centred nlZ %.1e dnlZ %.1e" % ((c / ell,) + plain + centred))
        assert max(centred) <= 1e-5, (c, centred)
        if c:
            assert max(plain) >= 1e-3, (c, plain)
