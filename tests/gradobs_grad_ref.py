"""Shared by tests/test_gpu_gradobs_grad.py: the extended-precision reference of the hyperparameter-derivative planes of
the joint covariance of values and gradients (gradobs.h: gobs_trace_kernel), on the cases of tests/gradobs_ref.py
(``setup``: the functor tests' distance ladder, duplicated points, the same fp64 scaled coordinates the device sees).

``planes_ld(case)`` returns the planes dK (cov_N, n, n) in np.longdouble and, entry by entry, the sum of the MAGNITUDES
of the terms each entry is made of (fp64) -- what a bound relative to "the terms of the entry" needs: the entries
cancel (delta_ab (G d_l^2 - 2 F) against d_a d_b (H d_l^2 - 4 G) on a = b = l).  Formulas: gpyreg_amd._gradobs.

The rational quadratic's log-alpha entries are Ka = K h, Fa = F (h + q), Ga = G (-1 / (alpha + 1) + h + 2 q) with
h = r2 / (2 M) - alpha log M, q = (M - 1) / M and M = 1 + r2 / (2 alpha).  Their terms are taken one level down -- h
cancels to O(r2^2) at small distances -- and the term 1 of M counts as tests/test_cov_functors_cpu.py counts it for the
functor these factors are built from (its a_rq): rounding M to eps moves alpha log M by up to alpha eps whatever r2
is, so alpha C eps / 1e-12 (C = 8) of the factor is added to the magnitude of its terms."""

import numpy as np

import gradobs_ref as gr
import test_cov_functors_cpu as cf
from test_cov_functors_cpu import LD


def _factors(kind, degree, xa, xb, sf2, rqa):
    """cf.reference's dict with G, H (0 at r2 = 0, where the kernels drop their terms) and the rational quadratic's
    (Fa, Ga), all longdouble."""
    ref = gr.with_g(kind, degree, cf.reference(kind, degree, xa, xb, sf2, rqa), sf2, rqa)
    r2, F, G = ref["r2"], ref["F"], ref["G"]
    zero = np.zeros_like(r2)
    ref["Fa"], ref["Ga"], ref["Ka_mag"], ref["Fa_mag"], ref["Ga_mag"] = zero, zero, zero, zero, zero
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if kind in (cf.K_SE, cf.K_SE_ISO):
            H = ref["K"]
        elif kind in (cf.K_MATERN, cf.K_MATERN_ISO):
            t = np.sqrt(r2)
            e = LD(sf2) * np.exp(-t)
            H = e * (1 + t) / t**3 if degree == 3 else e / (3 * t)
        else:
            al = LD(rqa)
            M = 1 + r2 / (2 * al)
            H = (al + 2) / al * G / M
            h, q = ref["Ka"] / ref["K"], (M - 1) / M
            ref["Fa"] = F * (h + q)
            ref["Ga"] = G * (-1 / (al + 1) + (h + q) + q)
            hm = r2 / (2 * M) + al * np.log1p(r2 / (2 * al)) + al * LD(cf.CBOUND[cf.F64] * cf.EPS[cf.F64] / 1e-12)
            ref["Ka_mag"] = np.abs(ref["K"]) * hm
            ref["Fa_mag"] = np.abs(F) * (hm + q)
            ref["Ga_mag"] = np.abs(G) * (1 / (al + 1) + hm + 2 * q)
    ref["H"] = np.where(r2 > 0, H, LD(0))
    return ref


def planes_ld(case):
    """(dK (cov_N, n, n) longdouble, mag (cov_N, n, n) fp64) of one ``gradobs_ref.setup`` case, in joint order."""
    kind, degree, c, sf2, rqa = (case[k] for k in ("kind", "degree", "c", "sf2", "rqa"))
    xs, xsg = case["xs"], case["xsg"]
    (N, D), Ng = xs.shape, xsg.shape[0]
    n = N + Ng * D
    iso = cf.is_iso(kind)
    nl = 1 if iso else D
    P = cf.cov_count(kind, D)
    dK, mag = np.zeros((P, n, n), LD), np.zeros((P, n, n))
    cl = c.astype(LD)
    rows = [slice(N + a * Ng, N + (a + 1) * Ng) for a in range(D)]

    def add(p, ri, rj, term, mirror=False, m=None):
        m = (np.abs(term) if m is None else m).astype(np.float64)
        dK[p, ri, rj] += term
        mag[p, ri, rj] += m
        if mirror:
            dK[p, rj, ri] += term.T
            mag[p, rj, ri] += m.T

    vv = _factors(kind, degree, xs, xs, sf2, rqa)
    gv = _factors(kind, degree, xsg, xs, sf2, rqa)
    gg = _factors(kind, degree, xsg, xsg, sf2, rqa)
    V = slice(0, N)
    # log sf (twice the entry) and log alpha
    sf = {"K": 2 * vv["K"], "Fv": 2 * gv["F"], "F": 2 * gg["F"], "G": 2 * gg["G"]}
    sf.update({k + "m": np.abs(v) for k, v in list(sf.items())})
    sh = {"K": vv["Ka"], "Fv": gv["Fa"], "F": gg["Fa"], "G": gg["Ga"],
          "Km": vv["Ka_mag"], "Fvm": gv["Fa_mag"], "Fm": gg["Fa_mag"], "Gm": gg["Ga_mag"]}
    for p, f in ((nl, sf), (D + 1, sh)):
        if p == D + 1 and kind != cf.K_RQ:
            continue
        add(p, V, V, f["K"], m=f["Km"])
        for a in range(D):
            da = cl[a] * gv["d"][:, :, a]
            add(p, rows[a], V, -da * f["Fv"], mirror=True, m=np.abs(da) * f["Fvm"])
            for b in range(D):
                if a == b:
                    add(p, rows[a], rows[b], cl[a] * cl[b] * f["F"], m=cl[a] * cl[b] * f["Fm"])
                dab = cl[a] * cl[b] * gg["d"][:, :, a] * gg["d"][:, :, b]
                add(p, rows[a], rows[b], -dab * f["G"], m=np.abs(dab) * f["Gm"])
    # log ell_l
    for l in range(D):
        p = 0 if iso else l
        add(p, V, V, vv["F"] * vv["d"][:, :, l] ** 2)
        dl2 = gv["d"][:, :, l] ** 2
        for a in range(D):
            add(p, rows[a], V, -cl[a] * gv["d"][:, :, a] * gv["G"] * dl2, mirror=True)
            if a == l:
                add(p, rows[a], V, 2 * cl[a] * gv["d"][:, :, a] * gv["F"], mirror=True)
        dl2 = gg["d"][:, :, l] ** 2
        for a in range(D):
            for b in range(D):
                cab = cl[a] * cl[b]
                dab = gg["d"][:, :, a] * gg["d"][:, :, b]
                if a == b:
                    add(p, rows[a], rows[b], cab * gg["G"] * dl2)
                    if a == l:
                        add(p, rows[a], rows[b], -2 * cab * gg["F"])
                add(p, rows[a], rows[b], -cab * dab * gg["H"] * dl2)
                k = (a == l) + (b == l)
                if k:
                    add(p, rows[a], rows[b], 2 * k * cab * dab * gg["G"])
    return dK, mag
