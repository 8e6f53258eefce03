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

The module is the model the device (gradobs.h) is tested against; nothing of it runs in the product's hot path.
"""

import numpy as np

from ._gradpost import _MATERN, K_SE, K_SE_ISO, check_kind, radial, scaling


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
