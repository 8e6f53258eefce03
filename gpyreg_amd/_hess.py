"""Hessians of the predictive mean and variance with respect to the query point (``GP.predict_hess``), restated in
vectorised NumPy.

Notation of ``_gradpost``: xs = x c the kernel family's scaled inputs, d = xs* - xs_i, r2 = |d|^2, F the radial factor
(dk/dx*_a = -c_a F d_a).  With the second radial factor G = -2 dF/d(r2)::

    d^2 k / dx*_a dx*_b = c_a c_b (G d_a d_b - F delta_ab)

    G:  SE  k      Matern 3  e / t      Matern 5  e / 3      RQ  (alpha + 1) / alpha F / m
        (t = sqrt(r2), e = sf2 exp(-t), m = 1 + r2 / (2 alpha))

and for one posterior record, alpha the posterior weights and Q = (K + Sigma)^-1 k*::

    Hmu[a, b]  = c_a c_b ( sum_i alpha_i G_i d_a d_b - delta_ab sum_i alpha_i F_i )
    Hs2[a, b]  = -2 ( P[a, b] + c_a c_b ( sum_i Q_i G_i d_a d_b - delta_ab sum_i Q_i F_i ) )
    P[a, b]    = (d_a k*)^T (K + Sigma)^-1 (d_b k*)

A pair at distance 0 contributes 0 to the G term (the limit: Matern 3 has G = infinity there, but G d_a d_b -> 0) and
its full -F(0) delta_ab to the diagonal term.  The Matern kernel of degree 1 has no second derivative.  kss is constant.

The module is the product's path for a GP without data, holds the mixture over samples, and is the model the device
(``gpc_predict_hess``) is tested against.
"""

import numpy as np

from . import _gradpost as _gpm
from ._gradpost import K_MATERN, K_MATERN_ISO, K_RQ, K_SE, K_SE_ISO, scaling  # noqa: F401  (the shared notation)

_MATERN = (K_MATERN, K_MATERN_ISO)


def check_kind(kind, degree):
    if kind not in (K_SE, K_MATERN, K_RQ, K_SE_ISO, K_MATERN_ISO):
        raise ValueError(f"unknown kernel id {kind}")
    if kind in _MATERN and degree not in (1, 3, 5):
        raise ValueError(f"Matern degree must be 1, 3 or 5, got {degree}")
    if kind in _MATERN and degree == 1:
        raise NotImplementedError("predict_hess: the Matern kernel of degree 1 has no second derivative with respect "
                                  "to x_star")


def radial2(kind, degree, r2, sf2, rqa=1.0):
    """(k, F, G) at squared scaled distance r2: ``_gradpost.radial`` and the second radial factor G = -2 dF/d(r2)
    (Matern 3: +inf at r2 = 0)."""
    r2 = np.asarray(r2, dtype=float)
    k, F = _gpm.radial(kind, degree, r2, sf2, rqa)
    if kind in (K_SE, K_SE_ISO):
        return k, F, k
    if kind in _MATERN:
        t = np.sqrt(r2)
        e = sf2 * np.exp(-t)
        if degree == 3:
            with np.errstate(divide="ignore"):
                return k, F, e / t
        if degree == 5:
            return k, F, e / 3
        raise NotImplementedError("the Matern kernel of degree 1 has no second derivative")
    m = 1 + r2 / (2 * rqa)
    return k, F, (rqa + 1) / rqa * F / m


def pair_terms(kind, degree, hyp_cov, X, x_star):
    """(c (D,), diff (N, M, D), k, F, G (N, M)): differences before products, r2 summed in ascending dimension (as the
    device sums); G is 0 at r2 = 0 (the limit of G d_a d_b), F is not."""
    X, x_star = np.asarray(X, dtype=float), np.asarray(x_star, dtype=float)
    D = X.shape[1]
    c, sf2, rqa = scaling(kind, degree, hyp_cov, D)
    diff = (x_star * c)[None, :, :] - (X * c)[:, None, :]
    r2 = np.zeros(diff.shape[:2])
    for l in range(D):
        r2 += diff[:, :, l] ** 2
    with np.errstate(all="ignore"):
        k, F, G = radial2(kind, degree, r2, sf2, rqa)
    return c, diff, k, F, np.where(r2 > 0, G, 0.0)


def contract(w, F, G, diff):
    """(sum_i w F (M,), sum_i w G d_a d_b (M, D, D)) for weights w (N,) or (N, M): the two sums the device kernel forms;
    as there, the lower triangle is computed and mirrored (symmetric to the bit)."""
    w = np.asarray(w, dtype=float)
    if w.ndim == 1:
        w = w[:, None]
    sG = np.einsum("ij,ija,ijb->jab", w * G, diff, diff)
    low = np.tril(np.ones(sG.shape[1:], bool))
    return np.sum(w * F, 0), np.where(low, sG, np.transpose(sG, (0, 2, 1)))


def kernel_hess(c, sF, sG):
    """c_a c_b (sG[a, b] - delta_ab sF) per query: (M, D, D)."""
    D = c.size
    return (c[:, None] * c[None, :])[None] * (sG - np.eye(D)[None] * sF[:, None, None])


def record(kind, degree, hyp_cov, X, x_star, alpha, sW, L, L_chol):
    """(mu (M,), s2 (M,), dmu (M, D), ds2 (M, D), Hmu (M, D, D), Hs2 (M, D, D)) at every row of x_star under ONE
    posterior record (alpha (N, 1), sW (N, 1), L (N, N), L_chol), without the mean function, unclamped."""
    import scipy.linalg as sla

    check_kind(kind, degree)
    X = np.asarray(X, dtype=float)
    N, D = X.shape
    c, diff, k, F, G = pair_terms(kind, degree, hyp_cov, X, x_star)
    M = diff.shape[1]
    _, sf2, rqa = scaling(kind, degree, hyp_cov, D)
    kss = float(_gpm.radial(kind, degree, 0.0, sf2, rqa)[0])
    dk = -F[:, :, None] * diff * c  # (N, M, D): dk_i / dx*_a (a coincident pair: d = 0 and F finite, so 0)
    al = np.asarray(alpha, dtype=float).ravel()
    B = np.concatenate([k[:, :, None], dk], axis=2).reshape(N, M * (D + 1))
    if L_chol:
        sw = np.asarray(sW, dtype=float).reshape(N, 1)
        V = sla.solve_triangular(L, sw * B, trans=1, check_finite=False)
        KiB = sw * sla.solve_triangular(L, V, trans=0, check_finite=False)  # (K + Sigma)^-1 B
    else:
        KiB = -(np.asarray(L, dtype=float) @ B)
    KiB = KiB.reshape(N, M, D + 1)
    Q = KiB[:, :, 0]
    mu = k.T @ al
    dmu = np.einsum("ija,i->ja", dk, al)
    s2 = kss - np.einsum("ij,ij->j", k, Q)
    ds2 = -2 * np.einsum("ija,ij->ja", dk, Q)
    P = np.einsum("ija,ijb->jab", dk, KiB[:, :, 1:])
    P = (P + np.transpose(P, (0, 2, 1))) / 2
    Hmu = kernel_hess(c, *contract(al, F, G, diff))
    Hs2 = -2 * (P + kernel_hess(c, *contract(Q, F, G, diff)))
    return mu, s2, dmu, ds2, Hmu, Hs2


def mean_hess(mean, hyp, x_star):
    """d^2 m(x) / dx dx^T (M, D, D) of a stock mean function; exact types only, as ``_mean_grad_x``."""
    from .mean_functions import ConstantMean, NegativeQuadratic, ZeroMean

    M, D = x_star.shape
    if type(mean) in (ZeroMean, ConstantMean):
        return np.zeros((M, D, D))
    if type(mean) is NegativeQuadratic:
        return np.broadcast_to(-np.diag(np.exp(-2 * np.asarray(hyp)[1 + D:1 + 2 * D])), (M, D, D)).copy()
    raise NotImplementedError(f"predict_hess: the mean function {mean!r} ({type(mean).__name__}) is user-defined; its "
                              "Hessian with respect to x_star is unknown")


def mix(mu, dmu, Hmu, Hs2):
    """Hessians of the equal-weight mixture's moments (``_mix_samples``: spread with divisor S - 1).  mu (M, S),
    dmu (M, D, S), Hmu, Hs2 (M, D, D, S; Hs2 may be None) -> (Hmu (M, D, D), Hs2 (M, D, D) | None)::

        Hmu = mean_s Hmu_s
        Hs2 = mean_s Hs2_s + 2 / (S - 1) sum_s [ (dmu_s - dmu)(dmu_s - dmu)^T + (mu_s - mu)(Hmu_s - Hmu) ]

    One sample is returned as it is."""
    S = mu.shape[1]
    if S == 1:
        return Hmu[..., 0], None if Hs2 is None else Hs2[..., 0]
    Hbar = np.sum(Hmu, 3) / S
    if Hs2 is None:
        return Hbar, None
    dm = mu - np.sum(mu, 1, keepdims=True) / S
    dg = dmu - np.sum(dmu, 2, keepdims=True) / S
    dH = Hmu - Hbar[..., None]
    spread = np.einsum("mas,mbs->mab", dg, dg) + np.einsum("ms,mabs->mab", dm, dH)
    return Hbar, np.sum(Hs2, 3) / S + 2 * spread / (S - 1)
