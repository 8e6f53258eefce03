"""Shared by tests/test_gradobs_cpu.py and tests/test_gpu_gradobs.py: the extended-precision reference of the joint
covariance of values and gradients (gradobs.h) and its per-entry error bounds, on the distance ladder, shifts and fp64
scaled coordinates of tests/test_cov_functors_cpu.py.

Bounds (C, eps, a_rq, arg, floor as defined there for fp64; c = mul / dv; d = xs_p - xs_q):
  value / value        that file's entry_bound;
  value / gradient     (C eps (1 + a_rq + |arg|) + 4 eps) |entry| + floor max(c_l, 1) max(|d_l|, 1)
                       -- F carries the functor's relative bound; the difference, the two products and the store round
                       once each; F's absolute floor is multiplied by c_l |d_l| like F itself (the bound
                       tests/test_gpu_gradient_posterior.py uses for its derivative slots);
  gradient / gradient  (C eps (1 + a_rq + |arg|) + 8 eps) c_a c_b (|F| delta_ab + |G d_a d_b|)
                       + floor max(c_a c_b, 1) max(|d_a d_b|, 1)
                       -- relative to the SUM of the two terms' magnitudes: their difference cancels on a = b.
"""

import numpy as np

import test_cov_functors_cpu as cf
from test_cov_functors_cpu import F64, LD

# (family name of test_cov_functors_cpu.FAMILIES, rational-quadratic alpha)
FAMILIES = [("se", None), ("se_iso", None), ("matern3", None), ("matern5", None), ("matern_iso3", None),
            ("matern_iso5", None), ("rq", 0.7), ("rq", 150.0)]


def setup(name, alpha, N, Ng, D, shift, M=0):
    """One ladder case: hyp, the raw inputs X (N, D), Xg (Ng, D), Xq (M, D) and their fp64 scaled copies.  X is the
    functor tests' ladder (duplicates, subnormal and huge r2, a duplicate across a tile border when N > 64); Xg repeats
    rows of X in its first half (r2 = 0 between a value and a gradient point) and row 0 in its last row (a duplicated
    gradient point when Ng > 1); the queries start ON training rows."""
    kind, degree = cf.FAMILIES[name]
    hyp = cf.make_hyp(kind, D, alpha)
    mul, dv, sf2, rqa = cf.scaling(kind, degree, D, hyp)
    X = cf.ladder_inputs(kind, degree, max(N, 65), D, hyp, shift)[:N]
    Xg = cf.ladder_inputs(kind, degree, max(Ng, 65), D, hyp, shift, seed=5)[:Ng]
    half = min(Ng // 2, N)
    Xg[:half] = X[:half]
    if Ng > 1:
        Xg[Ng - 1] = Xg[0]
    out = dict(kind=kind, degree=degree, hyp=hyp, X=X, Xg=Xg, c=mul / dv, sf2=sf2, rqa=rqa,
               xs=cf.scale(X, mul, dv), xsg=cf.scale(Xg, mul, dv))
    if M:
        Xq, _ = cf.query_inputs(kind, degree, np.concatenate([X, Xg]), M, hyp, shift)
        if M > 6:
            Xq[5] = Xg[Ng - 1]
        out.update(Xq=Xq, xss=cf.scale(Xq, mul, dv))
    return out


def with_g(kind, degree, ref, sf2, rqa):
    """test_cov_functors_cpu.reference's dict extended by G = -2 dF/d(r2) (longdouble; set to 0 at r2 = 0, where the
    kernels drop the G term)."""
    r2 = ref["r2"]
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind in (cf.K_SE, cf.K_SE_ISO):
            G = ref["K"]
        elif kind in (cf.K_MATERN, cf.K_MATERN_ISO):
            t = np.sqrt(r2)
            e = LD(sf2) * np.exp(-t)
            G = e / t if degree == 3 else e / 3
        else:
            al = LD(rqa)
            G = (al + 1) / al * ref["F"] / (1 + r2 / (2 * al))
    ref["G"] = np.where(r2 > 0, G, LD(0))
    return ref


def _vg(kind, ref, c, sf2, rqa, sign):
    """value / gradient entries (P, Q, D) = sign c_l F d_l (0 at r2 = 0) and their bounds."""
    F, d = ref["F"][:, :, None], ref["d"]
    live = (ref["r2"] > 0)[:, :, None]
    want = np.where(live, sign * c.astype(LD) * F * d, LD(0))
    rel = cf.rel_bound(kind, ref, rqa, F64)[:, :, None] + 4 * cf.EPS[F64]
    bound = rel * np.abs(want).astype(np.float64) + cf.floor_of(sf2, F64) * np.maximum(c, 1.0) * np.maximum(
        np.abs(d).astype(np.float64), 1.0)
    return want, bound


def joint_cov_ld(case):
    """(K (n, n) longdouble, bound (n, n) fp64) of the joint covariance of one ``setup`` case, in joint order."""
    kind, degree, c, sf2, rqa = (case[k] for k in ("kind", "degree", "c", "sf2", "rqa"))
    xs, xsg = case["xs"], case["xsg"]
    (N, D), Ng = xs.shape, xsg.shape[0]
    n = N + Ng * D
    K, B = np.zeros((n, n), LD), np.zeros((n, n))
    vv = cf.reference(kind, degree, xs, xs, sf2, rqa)
    K[:N, :N], B[:N, :N] = vv["K"], cf.entry_bound(kind, vv, sf2, rqa, F64)
    gv = cf.reference(kind, degree, xsg, xs, sf2, rqa)
    w, b = _vg(kind, gv, c, sf2, rqa, -1)
    gg = with_g(kind, degree, cf.reference(kind, degree, xsg, xsg, sf2, rqa), sf2, rqa)
    rel = cf.rel_bound(kind, gg, rqa, F64) + 8 * cf.EPS[F64]
    F, G, d = gg["F"], gg["G"], gg["d"]
    for a in range(D):
        ra = slice(N + a * Ng, N + (a + 1) * Ng)
        K[ra, :N], B[ra, :N] = w[:, :, a], b[:, :, a]
        K[:N, ra], B[:N, ra] = w[:, :, a].T, b[:, :, a].T
        for bb in range(D):
            rb = slice(N + bb * Ng, N + (bb + 1) * Ng)
            dd = d[:, :, a] * d[:, :, bb]
            cab = LD(c[a]) * LD(c[bb])
            K[ra, rb] = cab * ((F if a == bb else LD(0)) - G * dd)
            mag = float(c[a] * c[bb]) * ((np.abs(F) if a == bb else 0) + np.abs(G * dd)).astype(np.float64)
            B[ra, rb] = rel * mag + cf.floor_of(sf2, F64) * max(c[a] * c[bb], 1.0) * np.maximum(
                np.abs(dd).astype(np.float64), 1.0)
    return K, B


def joint_cross_ld(case):
    """(B (n, M) longdouble, bound (n, M) fp64) of the joint cross operand of one ``setup`` case (with queries)."""
    kind, degree, c, sf2, rqa = (case[k] for k in ("kind", "degree", "c", "sf2", "rqa"))
    xs, xsg, xss = case["xs"], case["xsg"], case["xss"]
    (N, D), Ng, M = xs.shape, xsg.shape[0], xss.shape[0]
    K, B = np.zeros((N + Ng * D, M), LD), np.zeros((N + Ng * D, M))
    v = cf.reference(kind, degree, xs, xss, sf2, rqa)
    K[:N], B[:N] = v["K"], cf.entry_bound(kind, v, sf2, rqa, F64)
    w, b = _vg(kind, cf.reference(kind, degree, xsg, xss, sf2, rqa), c, sf2, rqa, -1)
    for a in range(D):
        K[N + a * Ng:N + (a + 1) * Ng], B[N + a * Ng:N + (a + 1) * Ng] = w[:, :, a], b[:, :, a]
    return K, B


def worst(got, want, bound):
    """max |got - want| / bound over all entries (every reference entry of these families is finite)."""
    assert np.all(np.isfinite(want.astype(np.float64))) and np.all(np.isfinite(got))
    return float((np.abs(got.astype(LD) - want).astype(np.float64) / bound).max())
