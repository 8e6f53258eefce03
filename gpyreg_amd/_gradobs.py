"""Gradient observations (``GP.condition_on_gradients``), restated in vectorised NumPy.

The data are values y at X (N, D) and gradients dy (Ng, D) at X_g (Ng, D).  With xs the kernel family's scaled inputs,
c_l = d xs_l / d x_l (``_gradpost.scaling``), and for a pair (p, q) d = xs_p - xs_q, r2 = |d|^2 (differences first,
dimensions summed in ascending order) and (k, F, G) the covariance and its two radial factors at r2::

    cov(f(x_p), f(x_q))         = k
    cov(d_a f(x_p), f(x_q))     = -c_a F d_a                          (0 at r2 = 0)
    cov(d_a f(x_p), d_b f(x_q)) = c_a c_b (F delta_ab - G d_a d_b)    (c_a^2 F0 delta_ab at r2 = 0: the G term is dropped)

F is ``_gradpost.radial``'s (dk/dxs*_l = -F (xs*_l - xs_l)); G = -2 dF/d(r2) is added here (``radial_g``).  The joint
system has order n = N + Ng D: the values first, then the gradient rows DIMENSION-MAJOR, row N + l Ng + g =
d f / dx_l at X_g[g] (``order``).  From the joint matrix on it is the reference's computation on a per-row noise vector:
the branch rule min(sn2) >= 1e-6, the scaling by min(sn2), the x 10 jitter ladder, alpha, L and nlZ
(``posterior``), and ``predict``'s two variance formulas on the n x M operand (``joint_cross``, ``predict``).

HYPERPARAMETER DERIVATIVES (``joint_cov_dhyp``, ``nll_grad``; the device: gobs_trace_kernel).  With the third radial
factor H = -2 dG/d(r2) (``radial_h``; infinite at r2 = 0 for both Matern kernels, where every term that carries it tends
to 0 and is dropped, as G's are) and theta_l = log ell_l of an ARD kernel::

    d_l k    = F d_l^2
    d_l E_a  = -c_a d_a (G d_l^2 - 2 delta_al F)                                           (gradient_a / value)
    d_l E_ab = c_a c_b [delta_ab (G d_l^2 - 2 delta_al F) - d_a d_b (H d_l^2 - 2 (delta_al + delta_bl) G)]

An isotropic kernel's one length scale is the sum over l; log sf gives twice the entry; the rational quadratic's
log alpha the entries with (Ka, Fa, Ga) = d(k, F, G)/d log alpha in place of (k, F, G) (``radial_alpha``).  Contracted
with a pair's D x D weight block W (u_a = c_a d_a)::

    sum_ab W_ab d_l E_ab = d_l^2 (G T1 - H T2) - 2 F W_ll c_l^2 + 2 G u_l R_l
    T1 = sum_a W_aa c_a^2,   T2 = sum_ab W_ab u_a u_b,   R_l = sum_b (W_lb + W_bl) u_b

and with a gradient / value pair's weight vector w:  sum_a w_a d_l E_a = -G d_l^2 sum_a w_a u_a + 2 F w_l u_l.
dnlZ / dtheta_p = 1/2 sum_ij ((K + mult Sigma)^-1 - alpha alpha^T)_ij d_p K_ij at the record's fixed jitter multiplier.

THE POSTERIOR OF THE GRADIENT (``joint_operand``, ``gradient_joint``; the device: gobs_grad_operand_tile_kernel and
gpc_grad_post_gobs).  For a query x*, slot 0 = f(x*) and slot 1 + l = d f / dx*_l, the n x (D + 1) operand has, with
d = xs_i - xs* on a value row i and d = xs_g - xs* on the gradient rows of X_g[g]::

    value row i              slot 0: k              slot 1 + l: -c_l F (xs*_l - xs_il)           (0 at r2 = 0)
    gradient row N + a Ng + g  slot 0: -c_a F d_a   slot 1 + l: c_a c_l (F delta_al - G d_a d_l)
                             (slot 0: 0 at r2 = 0;  slot 1 + l: c_a^2 F0 delta_al at r2 = 0, the G term dropped)

The value rows are ``_gradpost.operand``'s, slot 0 is ``joint_cross``, and the gradient rows' slots 1 + l are the
gradient / gradient block of ``joint_cov`` with p = g and q = *.  From the operand on it is ``_gradpost.joint``'s
algebra: mean = B^T alpha, C = H - V^T V (V = L^-T (sW B)) or H + B^T (L B), H = diag(kss, F0 c_l^2).

The module is the model the device (gradobs.h) is tested against; nothing of it runs in the product's hot path.
"""

import numpy as np

from ._gradpost import _MATERN, K_MATERN_ISO, K_RQ, K_SE, K_SE_ISO, check_kind, operand, prior_block, radial, scaling


def order(N, Ng, D):
    """idx (Ng, D): the joint row of dy[g, l], N + l Ng + g.  ``v[order(N, Ng, D)]`` brings a joint vector's gradient
    part into the user's (Ng, D) layout; ``j[order(N, Ng, D)] = dy`` writes it back."""
    g, l = np.meshgrid(np.arange(Ng), np.arange(D), indexing="ij")
    return N + l * Ng + g


def to_joint(y, dy):
    """[y | dy in joint order] (n,) from y (N,) and dy (Ng, D)."""
    y, dy = np.asarray(y, dtype=float).ravel(), np.asarray(dy, dtype=float)
    Ng, D = dy.shape
    out = np.empty(y.size + Ng * D)
    out[:y.size] = y
    out[order(y.size, Ng, D)] = dy
    return out


def from_joint(v, N, Ng, D):
    """(values (N,), gradients (Ng, D)) of a joint vector (n,)."""
    v = np.asarray(v).ravel()
    return v[:N].copy(), v[order(N, Ng, D)]


def radial_g(kind, degree, r2, sf2, rqa=1.0):
    """G = -2 dF/d(r2) at squared scaled distance r2: d^2 k / dxs_a dxs_b = G d_a d_b - F delta_ab.
    SE: k;  Matern 3: e / t (infinite at 0);  Matern 5: e / 3;  RQ: (alpha + 1) / alpha F / m."""
    r2 = np.asarray(r2, dtype=float)
    if kind in (K_SE, K_SE_ISO):
        return sf2 * np.exp(-r2 / 2)
    if kind in _MATERN:
        t = np.sqrt(r2)
        e = sf2 * np.exp(-t)
        if degree == 3:
            with np.errstate(divide="ignore"):
                return e / t
        return e / 3
    m = 1 + r2 / (2 * rqa)
    return (rqa + 1) / rqa * (sf2 * m ** (-rqa) / m) / m


def radial_h(kind, degree, r2, sf2, rqa=1.0):
    """H = -2 dG/d(r2), the third radial factor.  SE: k;  Matern 3: e (1 + t) / t^3;  Matern 5: e / (3 t) (both infinite
    at 0);  RQ: (alpha + 2) / alpha G / m."""
    r2 = np.asarray(r2, dtype=float)
    if kind in (K_SE, K_SE_ISO):
        return sf2 * np.exp(-r2 / 2)
    if kind in _MATERN:
        t = np.sqrt(r2)
        e = sf2 * np.exp(-t)
        with np.errstate(divide="ignore"):
            return e * (1 + t) / t**3 if degree == 3 else e / (3 * t)
    m = 1 + r2 / (2 * rqa)
    return (rqa + 2) / rqa * radial_g(kind, degree, r2, sf2, rqa) / m


def radial_alpha(r2, sf2, rqa):
    """(Ka, Fa, Ga) = d(k, F, G) / d log alpha of the rational quadratic kernel at squared scaled distance r2:
    Ka = k (r2 / (2 m) - alpha log m),  Fa = F (Ka / k + (m - 1) / m),  Ga = G (-1 / (alpha + 1) + Fa / F + (m - 1) / m)."""
    r2 = np.asarray(r2, dtype=float)
    m = 1 + r2 / (2 * rqa)
    k = sf2 * m ** (-rqa)
    h = r2 / (2 * m) - rqa * np.log(m)
    q = (m - 1) / m
    F = k / m
    G = (rqa + 1) / rqa * F / m
    return k * h, F * (h + q), G * (-1 / (rqa + 1) + (h + q) + q)


def _pairs(kind, degree, sf2, rqa, A, B):
    """diff (P, Q, D) = a - b, r2, k, F, G of all pairs of the rows of the SCALED inputs A and B (G zeroed at r2 = 0)."""
    diff = A[:, None, :] - B[None, :, :]
    r2 = np.zeros(diff.shape[:2])
    for l in range(diff.shape[2]):  # ascending l, as the device sums
        r2 += diff[:, :, l] ** 2
    with np.errstate(all="ignore"):
        k, F = radial(kind, degree, r2, sf2, rqa)
        G = np.where(r2 > 0, radial_g(kind, degree, r2, sf2, rqa), 0.0)
    return diff, r2, k, F, G


def joint_cov_scaled(kind, degree, xs, xsg, c, sf2, rqa=1.0):
    """``joint_cov`` from the scaled inputs xs (N, D), xsg (Ng, D) and the scaling itself (c (D,), sf2, rq alpha)."""
    check_kind(kind, degree)
    X, Xg = xs, xsg
    N, D = X.shape
    Ng = Xg.shape[0]
    n = N + Ng * D
    K = np.empty((n, n))
    K[:N, :N] = _pairs(kind, degree, sf2, rqa, X, X)[2]
    d_gv, r2_gv, _, F_gv, _ = _pairs(kind, degree, sf2, rqa, Xg, X)
    d_vg, r2_vg, _, F_vg, _ = _pairs(kind, degree, sf2, rqa, X, Xg)
    d_gg, _, _, F_gg, G_gg = _pairs(kind, degree, sf2, rqa, Xg, Xg)
    for a in range(D):
        ra = slice(N + a * Ng, N + (a + 1) * Ng)
        K[ra, :N] = np.where(r2_gv > 0, -((c[a] * F_gv) * d_gv[:, :, a]), 0.0)
        K[:N, ra] = np.where(r2_vg > 0, (c[a] * F_vg) * d_vg[:, :, a], 0.0)
        for b in range(D):
            rb = slice(N + b * Ng, N + (b + 1) * Ng)
            K[ra, rb] = (c[a] * c[b]) * ((F_gg if a == b else 0.0) - G_gg * (d_gg[:, :, a] * d_gg[:, :, b]))
    return K


def joint_cov(kind, degree, hyp_cov, X, Xg):
    """The n x n joint covariance of [f(X) ; grad f(X_g)] in joint order, without noise.  Every block is evaluated from
    its own pairs (d -> -d between a block and its mirror image only flips signs): symmetric to the bit."""
    X, Xg = np.atleast_2d(np.asarray(X, dtype=float)), np.atleast_2d(np.asarray(Xg, dtype=float))
    c, sf2, rqa = scaling(kind, degree, hyp_cov, X.shape[1])
    return joint_cov_scaled(kind, degree, X * c, Xg * c, c, sf2, rqa)


def joint_cross_scaled(kind, degree, xs, xsg, xss, c, sf2, rqa=1.0):
    """``joint_cross`` from the scaled inputs xs (N, D), xsg (Ng, D), xss (M, D) and the scaling itself."""
    check_kind(kind, degree)
    N, D = xs.shape
    Ng = xsg.shape[0]
    B = np.empty((N + Ng * D, xss.shape[0]))
    B[:N] = _pairs(kind, degree, sf2, rqa, xs, xss)[2]
    d, r2, _, F, _ = _pairs(kind, degree, sf2, rqa, xsg, xss)
    for a in range(D):
        B[N + a * Ng:N + (a + 1) * Ng] = np.where(r2 > 0, -((c[a] * F) * d[:, :, a]), 0.0)
    return B


def joint_cross(kind, degree, hyp_cov, X, Xg, x_star):
    """The n x M operand of a prediction at x_star (M, D): rows [k(X, x*) ; dk(X_g, x*) / dx_g], the gradient rows
    -c_l F (xs_g - xs*)_l (0 at r2 = 0), in joint order."""
    X, Xg = np.atleast_2d(np.asarray(X, dtype=float)), np.atleast_2d(np.asarray(Xg, dtype=float))
    x_star = np.atleast_2d(np.asarray(x_star, dtype=float))
    c, sf2, rqa = scaling(kind, degree, hyp_cov, X.shape[1])
    return joint_cross_scaled(kind, degree, X * c, Xg * c, x_star * c, c, sf2, rqa)


def _is_iso(kind):
    return kind in (K_SE_ISO, K_MATERN_ISO)


def cov_count(kind, D):
    """The number of covariance hyperparameters: [log ell (D, or 1 isotropic) | log sf | log alpha (RQ)]."""
    return (1 if _is_iso(kind) else D) + 1 + (1 if kind == K_RQ else 0)


def _pairs_h(kind, degree, sf2, rqa, A, B):
    """``_pairs`` with H and, for the rational quadratic, (Ka, Fa, Ga) (else zeros).  H is zeroed at r2 = 0, as G, and
    -- as on the device -- below r2 = 1e-200, where Matern 3's t^3 leaves the fp64 range: its terms carry d_a d_b d_l^2
    <= r2^2 and are below 1e-100 there."""
    diff, r2, k, F, G = _pairs(kind, degree, sf2, rqa, A, B)
    with np.errstate(all="ignore"):
        H = np.where(r2 > 1e-200, radial_h(kind, degree, r2, sf2, rqa), 0.0)
    al = radial_alpha(r2, sf2, rqa) if kind == K_RQ else (np.zeros_like(r2),) * 3
    return diff, r2, k, F, G, H, al


def joint_cov_dhyp(kind, degree, hyp_cov, X, Xg):
    """dK (cov_N, n, n): the derivative of ``joint_cov`` with respect to every covariance hyperparameter, in the
    module's formulas; symmetric.  For tests: the device never forms a plane."""
    check_kind(kind, degree)
    X, Xg = np.atleast_2d(np.asarray(X, dtype=float)), np.atleast_2d(np.asarray(Xg, dtype=float))
    N, D = X.shape
    Ng = Xg.shape[0]
    n = N + Ng * D
    c, sf2, rqa = scaling(kind, degree, hyp_cov, D)
    xs, xsg = X * c, Xg * c
    iso = _is_iso(kind)
    nl = 1 if iso else D
    dK = np.zeros((cov_count(kind, D), n, n))
    dK[nl] = 2 * joint_cov_scaled(kind, degree, xs, xsg, c, sf2, rqa)
    d_vv, _, _, F_vv, _, _, al_vv = _pairs_h(kind, degree, sf2, rqa, xs, xs)
    d_gv, r2_gv, _, F_gv, G_gv, _, al_gv = _pairs_h(kind, degree, sf2, rqa, xsg, xs)
    d_gg, _, _, F_gg, G_gg, H_gg, al_gg = _pairs_h(kind, degree, sf2, rqa, xsg, xsg)
    live = r2_gv > 0
    rows = [slice(N + a * Ng, N + (a + 1) * Ng) for a in range(D)]
    for l in range(D):
        P = dK[0 if iso else l]
        P[:N, :N] += F_vv * d_vv[:, :, l] ** 2
        for a in range(D):
            e = np.where(live, -(c[a] * d_gv[:, :, a]) * (G_gv * d_gv[:, :, l] ** 2 - (2 * F_gv if a == l else 0.0)), 0.0)
            P[rows[a], :N] += e
            P[:N, rows[a]] += e.T
            for b in range(D):
                t1 = (G_gg * d_gg[:, :, l] ** 2 - (2 * F_gg if a == l else 0.0)) if a == b else 0.0
                t2 = (d_gg[:, :, a] * d_gg[:, :, b]) * (H_gg * d_gg[:, :, l] ** 2 - ((a == l) + (b == l)) * 2 * G_gg)
                P[rows[a], rows[b]] += (c[a] * c[b]) * (t1 - t2)
    if kind == K_RQ:
        P = dK[D + 1]
        P[:N, :N] = al_vv[0]
        for a in range(D):
            e = np.where(live, -(c[a] * d_gv[:, :, a]) * al_gv[1], 0.0)
            P[rows[a], :N] = e
            P[:N, rows[a]] = e.T
            for b in range(D):
                P[rows[a], rows[b]] = (c[a] * c[b]) * ((al_gg[1] if a == b else 0.0)
                                                      - al_gg[2] * (d_gg[:, :, a] * d_gg[:, :, b]))
    return dK


def mean_xgrad_dhyp(mean, hyp_mean, Xg):
    """(Ng, D, mean_N): the derivatives of d m(x) / dx_l at the rows of Xg with respect to the mean hyperparameters of
    a stock mean function, ``mean`` in ("zero", "const", "negquad").  The negative quadratic's
    d m / dx_l = -(x_l - xm_l) / omega_l^2 depends on xm_l (1 / omega_l^2) and log omega_l (2 (x_l - xm_l) / omega_l^2)."""
    Xg = np.atleast_2d(np.asarray(Xg, dtype=float))
    Ng, D = Xg.shape
    hyp_mean = np.asarray(hyp_mean, dtype=float).ravel()
    if mean == "zero":
        return np.zeros((Ng, D, 0))
    if mean == "const":
        return np.zeros((Ng, D, 1))
    if mean != "negquad":
        raise ValueError(f"unknown stock mean {mean!r}")
    out = np.zeros((Ng, D, 1 + 2 * D))
    w2 = np.exp(2 * hyp_mean[1 + D:1 + 2 * D])
    for l in range(D):
        out[:, l, 1 + l] = 1.0 / w2[l]
        out[:, l, 1 + D + l] = 2 * (Xg[:, l] - hyp_mean[1 + l]) / w2[l]
    return out


def joint_dm(dm_X, dmg):
    """dm (n, mean_N) in joint order from the mean's derivatives at X (N, mean_N) and those of its x-gradient at X_g
    (Ng, D, mean_N: ``mean_xgrad_dhyp``)."""
    dm_X, dmg = np.asarray(dm_X, dtype=float), np.asarray(dmg, dtype=float)
    N, (Ng, D, P) = dm_X.shape[0], dmg.shape
    out = np.empty((N + Ng * D, P))
    out[:N] = dm_X.reshape(N, P)
    out[order(N, Ng, D)] = dmg
    return out


def joint_dsn2(dsn2_X, N, Ng, D):
    """dsn2 (n, noise_N) in joint order: the noise function's derivatives (N or 1, noise_N) on the N value rows, zeros
    on the gradient rows (s2_grad is data, not a hyperparameter)."""
    dsn2_X = np.asarray(dsn2_X, dtype=float)
    out = np.zeros((N + Ng * D, dsn2_X.shape[-1]))
    out[:N] = np.broadcast_to(dsn2_X.reshape(-1, dsn2_X.shape[-1]), (N, dsn2_X.shape[-1]))
    return out


def weight(post):
    """Wt (n, n) = (K + mult Sigma)^-1 - alpha alpha^T of a ``posterior`` record: dnlZ = 1/2 sum Wt o dK."""
    import scipy.linalg as sla

    if post["L_chol"]:
        n = post["L"].shape[0]
        Li = sla.solve_triangular(post["L"], np.eye(n), check_finite=False)  # A^-1 = Li Li^T, K + mult Sigma = sl A
        Q = (Li @ Li.T) / post["sl"]
    else:
        Q = -post["L"]
    Q = (Q + Q.T) / 2
    return Q - np.outer(post["alpha"], post["alpha"])


def trace_contract(kind, degree, hyp_cov, X, Xg, Wt):
    """(cov_N,): sum_ij Wt_ij d_p K_ij for a SYMMETRIC weight Wt (n, n), in the contracted form of the module's header
    (O(D^2) sums per pair, no plane): what gobs_trace_kernel computes from the lower triangle."""
    check_kind(kind, degree)
    X, Xg = np.atleast_2d(np.asarray(X, dtype=float)), np.atleast_2d(np.asarray(Xg, dtype=float))
    N, D = X.shape
    Ng = Xg.shape[0]
    c, sf2, rqa = scaling(kind, degree, hyp_cov, D)
    xs, xsg = X * c, Xg * c
    iso = _is_iso(kind)
    nl = 1 if iso else D
    idx = order(N, Ng, D)  # (Ng, D)
    out = np.zeros(cov_count(kind, D))
    # value / value
    d, _, k, F, _, _, al = _pairs_h(kind, degree, sf2, rqa, xs, xs)
    W = Wt[:N, :N]
    ell = np.einsum("pq,pql->l", W * F, d ** 2)
    out[nl] += 2 * np.sum(W * k)
    if kind == K_RQ:
        out[D + 1] += np.sum(W * al[0])
    # gradient / value, counted twice (its mirror image value / gradient)
    d, r2, _, F, G, _, al = _pairs_h(kind, degree, sf2, rqa, xsg, xs)
    w = 2 * np.where((r2 > 0)[:, :, None], Wt[idx][:, :, :N].transpose(0, 2, 1), 0.0)  # (Ng, N, D)
    u = d * c
    A = np.sum(w * u, 2)
    ell += np.einsum("pq,pql->l", -G * A, d ** 2) + 2 * np.einsum("pq,pql->l", F, w * u)
    out[nl] += 2 * np.sum(-F * A)
    if kind == K_RQ:
        out[D + 1] += np.sum(-al[1] * A)
    # gradient / gradient
    d, _, _, F, G, H, al = _pairs_h(kind, degree, sf2, rqa, xsg, xsg)
    W = Wt[idx[:, :, None, None], idx[None, None, :, :]].transpose(0, 2, 1, 3)  # (Ng, Ng, D, D): [p, q, a, b]
    u = d * c
    T1 = np.einsum("pqaa,a->pq", W, c * c)
    T2 = np.einsum("pqab,pqa,pqb->pq", W, u, u)
    R = np.einsum("pqlb,pqb->pql", W, u) + np.einsum("pqbl,pqb->pql", W, u)
    ell += (np.einsum("pq,pql->l", G * T1 - H * T2, d ** 2) - 2 * np.einsum("pq,pqll,l->l", F, W, c * c)
            + 2 * np.einsum("pq,pql,pql->l", G, u, R))
    out[nl] += 2 * np.sum(F * T1 - G * T2)
    if kind == K_RQ:
        out[D + 1] += np.sum(al[1] * T1 - al[2] * T2)
    out[:nl] = np.sum(ell) if iso else ell
    return out


def nll_grad(kind, degree, hyp_cov, X, Xg, post, dm=None, dsn2=None, sn2_mult=None):
    """dnlZ ([cov | noise | mean],) of ``posterior``'s nlZ from its record ``post`` at the record's fixed jitter
    multiplier: 1/2 sum Wt o d_p K for the covariance part (``trace_contract``), 1/2 mult sum_i Wt_ii dsn2_ip for the
    noise function's hyperparameters and -sum_i alpha_i dm_ip for the mean's, with dm (n, mean_N) and dsn2
    (n, noise_N) in joint order (``joint_dm``, ``joint_dsn2``; None: no such hyperparameters)."""
    Wt = weight(post)
    mult = post["sn2_mult"] if sn2_mult is None else sn2_mult
    parts = [trace_contract(kind, degree, hyp_cov, X, Xg, Wt) / 2]
    if dsn2 is not None and np.size(dsn2):
        parts.append(0.5 * mult * (np.diag(Wt) @ np.asarray(dsn2, dtype=float)))
    if dm is not None and np.size(dm):
        parts.append(-(post["alpha"] @ np.asarray(dm, dtype=float)))
    return np.concatenate(parts)


def posterior(kind, degree, hyp_cov, X, Xg, target, m, sn2):
    """The reference's ``__core_computation`` on the joint system: target, m, sn2 (n,) in joint order (the observations,
    the mean function with its x-gradient, the per-row noise variances).  Returns a dict with alpha (n,), L (n, n: the
    UPPER Cholesky factor of K / sl + diag(sn2 / min sn2) when L_chol, else -(K + mult diag(sn2))^-1), sW (n,),
    sn2_mult, L_chol, sl and nlZ.  Raises LinAlgError after ten failed factorizations."""
    import scipy.linalg as sla

    K = joint_cov(kind, degree, hyp_cov, X, Xg)
    n = K.shape[0]
    target, m, sn2 = (np.asarray(v, dtype=float).ravel() for v in (target, m, sn2))
    sn2_mult, L = 1.0, None
    L_chol = bool(np.min(sn2) >= 1e-6)
    sn2_div = np.min(sn2)
    for _ in range(10):
        try:
            if L_chol:
                L = sla.cholesky(K / (sn2_div * sn2_mult) + np.diag(sn2 / sn2_div), check_finite=False)
            else:
                L = sla.cholesky(K + sn2_mult * np.diag(sn2), check_finite=False)
        except sla.LinAlgError:
            sn2_mult *= 10
            continue
        break
    if L is None:
        raise np.linalg.LinAlgError("Singular matrix for L Cholesky decomposition")
    sl = sn2_div * sn2_mult if L_chol else 1.0
    r = target - m
    tri = lambda trans, v: sla.solve_triangular(L, v, trans=trans, check_finite=False)
    alpha = tri(0, tri(1, r)) / sl
    nlZ = float(r @ alpha / 2 + np.sum(np.log(np.diag(L))) + n * np.log(2 * np.pi * sl) / 2)
    pL = L if L_chol else tri(0, tri(1, np.eye(n))) * -1.0
    with np.errstate(divide="ignore"):
        sW = np.full(n, 1.0 / np.sqrt(sn2_div * sn2_mult))
    return {"alpha": alpha, "L": pL, "sW": sW, "sn2_mult": sn2_mult, "L_chol": L_chol, "sl": sl, "nlZ": nlZ}


def predict(kind, degree, hyp_cov, X, Xg, x_star, post):
    """(mu (M,), s2 (M,)) at x_star under one ``posterior`` record, without the mean function and unclamped:
    mu = B^T alpha; s2 = kss - colsum(V^2), V = L^-T (sW B), or kss + colsum(B o (L B)) on the low-noise branch."""
    import scipy.linalg as sla

    B = joint_cross(kind, degree, hyp_cov, X, Xg, x_star)
    D = np.atleast_2d(np.asarray(X)).shape[1]
    kss = scaling(kind, degree, hyp_cov, D)[1]
    mu = B.T @ post["alpha"]
    if post["L_chol"]:
        V = sla.solve_triangular(post["L"], post["sW"][:, None] * B, trans=1, check_finite=False)
        s2 = kss - np.sum(V * V, 0)
    else:
        s2 = kss + np.sum(B * (post["L"] @ B), 0)
    return mu, s2


def joint_operand(kind, degree, hyp_cov, X, Xg, x_star):
    """B (n, D + 1, M): the operand of the joint posterior of (f, grad f) at x_star (M, D) under values at X and
    gradients at X_g, rows in joint order; slot 0 = ``joint_cross``, slot 1 + l the derivative with respect to x*_l
    (the header's formulas: zeros at r2 = 0 but for c_a^2 F0 on a gradient row's own dimension)."""
    check_kind(kind, degree)
    X, Xg = np.atleast_2d(np.asarray(X, dtype=float)), np.atleast_2d(np.asarray(Xg, dtype=float))
    x_star = np.atleast_2d(np.asarray(x_star, dtype=float))
    N, D = X.shape
    Ng, M = Xg.shape[0], x_star.shape[0]
    c, sf2, rqa = scaling(kind, degree, hyp_cov, D)
    xsg, xss = Xg * c, x_star * c
    B = np.empty((N + Ng * D, D + 1, M))
    B[:N] = operand(kind, degree, hyp_cov, X, x_star)  # the value rows are the plain GP's operand
    d, r2, _, F, G = _pairs(kind, degree, sf2, rqa, xsg, xss)  # d = xs_g - xs*: (Ng, M, D)
    for a in range(D):
        ra = slice(N + a * Ng, N + (a + 1) * Ng)
        B[ra, 0] = np.where(r2 > 0, -((c[a] * F) * d[:, :, a]), 0.0)
        for l in range(D):
            B[ra, 1 + l] = (c[a] * c[l]) * ((F if a == l else 0.0) - G * (d[:, :, a] * d[:, :, l]))
    return B


def gradient_joint(kind, degree, hyp_cov, X, Xg, x_star, post):
    """(mean (M, D + 1), cov (M, D + 1, D + 1)) of (f, grad f) at every row of x_star under ONE ``posterior`` record,
    without the mean function: ``_gradpost.joint``'s algebra on ``joint_operand``.  The matrix is returned as computed."""
    import scipy.linalg as sla

    B = joint_operand(kind, degree, hyp_cov, X, Xg, x_star)
    n, P, M = B.shape
    H = np.diag(prior_block(kind, degree, hyp_cov, P - 1))
    mean = np.einsum("iaj,i->ja", B, np.asarray(post["alpha"], dtype=float).ravel())
    flat = B.reshape(n, P * M)
    if post["L_chol"]:
        V = sla.solve_triangular(post["L"], post["sW"][:, None] * flat, trans=1, check_finite=False).reshape(n, P, M)
        cov = H[None] - np.einsum("iaj,ibj->jab", V, V)
    else:
        Z = (post["L"] @ flat).reshape(n, P, M)
        cov = H[None] + np.einsum("iaj,ibj->jab", B, Z)
    return mean, cov
