"""Derivatives of the latent predictive mean and variance with respect to the hyperparameters
(``GP.predict_hyp_grad``), restated in vectorised NumPy.

Notation of ``_nllhess``: Sigma = K + mult diag(sn2) at a FIXED jitter multiplier, Q = Sigma^-1, alpha = Q (y - m),
hyperparameters ordered [cov | noise | mean], P of them.  For query j: k_j = k(X, x*_j), q_j = Q k_j and::

    fmu_j = k_j . alpha                     fs2_j = k** - k_j . q_j

Every hyperparameter p has a weight vector w_p (N,)::

    lengthscale, RQ shape    w_p = Q (d_p K alpha)
    log sf                   w_p = 2 alpha - 2 mult Q (sn2 o alpha)        (= Q (2 K alpha))
    noise n                  w_p = mult Q (dsn2_n o alpha)
    mean k                   w_p = Q d_k m

and with the cross planes d_p k (N, M) -- F d_a^2 (isotropic: F r2), 2 k for log sf, Ka for the RQ shape, the planes
of ``_nllhess.cov_derivatives`` between training points and queries -- ::

    dfmu_j / dtheta_p = sum_i d_p k_ij alpha_i - sum_i k_ij w_p,i               (first sum: covariance p only)
    dfs2_j / dtheta_p = -2 sum_i d_p k_ij q_ij + q_j^T (d_p K) q_j              lengthscale, RQ shape
                      = 2 fs2_j - 2 mult sum_i sn2_i q_ij^2                     log sf  (Sigma q_j = k_j)
                      = mult sum_i dsn2_n,i q_ij^2                              noise n;     0 for a mean hyperparameter

k** does not depend on a lengthscale or the shape (stationary kernels).  A pair at r2 = 0 contributes nothing to a
lengthscale term.  The caller adds the mean function, d_k m(x*_j) and, with noise at x*, its value and derivative.

The module is the model the device (``gpc_predict_hyp_grad``) is tested against, and holds the delta-method sums of
``GP.predict_laplace``.
"""

import numpy as np

from . import _nllhess as _nh
from ._gradpost import K_MATERN, K_MATERN_ISO, K_RQ, K_SE, K_SE_ISO  # noqa: F401  (the shared notation)

_MATERN = (K_MATERN, K_MATERN_ISO)
_ISO = (K_SE_ISO, K_MATERN_ISO)


def check_kind(kind, degree, who="predict_hyp_grad"):
    if kind not in (K_SE, K_MATERN, K_RQ, K_SE_ISO, K_MATERN_ISO):
        raise ValueError(f"unknown kernel id {kind}")
    if kind in _MATERN and degree not in (1, 3, 5):
        raise ValueError(f"Matern degree must be 1, 3 or 5, got {degree}")
    if kind in _MATERN and degree == 1:
        raise NotImplementedError(f"{who}: the Matern kernel of degree 1 has an infinite radial factor on the diagonal; "
                                  "its lengthscale planes are not formed")


def sf_col(kind, D):
    """The column of log sf among the covariance hyperparameters."""
    return 1 if kind in _ISO else D


def scales(kind, degree, hyp_cov, D, dtype=np.float64):
    """(c (D,): xs = x c, sf2, rq_alpha), as ``_nllhess.scaled_sq_diffs`` scales."""
    h = np.asarray(hyp_cov, dtype=dtype).ravel()
    snu = np.sqrt(dtype(degree)) if kind in _MATERN else dtype(1)
    if kind in _ISO:
        return np.full(D, snu / np.exp(h[0]), dtype=dtype), np.exp(2 * h[1]), dtype(1)
    return snu / np.exp(h[:D]), np.exp(2 * h[D]), (np.exp(h[D + 1]) if kind == K_RQ else dtype(1))


def cross_planes(kind, degree, hyp_cov, X, x_star, dtype=np.float64, xs=None, xss=None):
    """(k (N, M), dk: list of the cov_N cross planes (N, M)): differences before products, r2 summed in ascending
    dimension.  ``xs`` / ``xss``: the scaled inputs, when the caller has formed them itself."""
    X, x_star = np.asarray(X, dtype=dtype), np.asarray(x_star, dtype=dtype)
    D = X.shape[1]
    c, sf2, rqa = scales(kind, degree, hyp_cov, D, dtype)
    xs = X * c if xs is None else np.asarray(xs, dtype=dtype)
    xss = x_star * c if xss is None else np.asarray(xss, dtype=dtype)
    d2 = np.empty((D, X.shape[0], x_star.shape[0]), dtype=dtype)
    r2 = np.zeros(d2.shape[1:], dtype=dtype)
    for a in range(D):
        d = xss[None, :, a] - xs[:, None, a]
        d2[a] = d * d
        r2 += d2[a]
    R = _nh.radial(kind, degree, r2, sf2, rqa)
    k, F = R["K"], np.where(r2 > 0, R["F"], 0)
    if kind in _ISO:
        return k, [F * r2, 2 * k]
    dk = [F * d2[a] for a in range(D)] + [2 * k]
    if kind == K_RQ:
        dk.append(R["Ka"])
    return k, dk


def hyp_grad(kind, degree, hyp_cov, X, x_star, resid, sn2, mult=1.0, dm=None, dsn2=None, compute_var=True,
             dtype=np.float64):
    """(fmu (M,), fs2 (M,), dfmu (M, P), dfs2 (M, P)) for ONE hyperparameter vector: the latent prediction without the
    mean function, unclamped, and its derivatives at a fixed multiplier.

    resid = y - m (N,); sn2 (N,) or a scalar; dm (N, mean_N) | None; dsn2 (N | 1, noise_N) | None.  Without
    ``compute_var`` fs2 and dfs2 are None."""
    check_kind(kind, degree)
    X = np.asarray(X, dtype=dtype)
    N, D = X.shape
    r = np.asarray(resid, dtype=dtype).ravel()
    sn2 = np.broadcast_to(np.asarray(sn2, dtype=dtype).ravel(), (N,))
    mult = dtype(mult)
    K, dK, _ = _nh.cov_derivatives(kind, degree, hyp_cov, X, dtype)
    k, dk = cross_planes(kind, degree, hyp_cov, X, x_star, dtype)
    cov_N, sfc = len(dK), sf_col(kind, D)
    dm = np.zeros((N, 0), dtype=dtype) if dm is None else np.asarray(dm, dtype=dtype).reshape(N, -1)
    noise_N = 0 if dsn2 is None else np.shape(dsn2)[-1]
    e = np.zeros((noise_N, N), dtype=dtype)
    if noise_N:
        e[:] = np.broadcast_to(np.asarray(dsn2, dtype=dtype).reshape(-1, noise_N), (N, noise_N)).T
    mean_N = dm.shape[1]
    P, M = cov_N + noise_N + mean_N, k.shape[1]
    Q, _ = _nh.spd_inverse(K + np.diag(mult * sn2))
    Q = (Q + Q.T) / 2
    alpha = Q @ r
    w = []
    for p in range(cov_N):
        w.append(2 * alpha - 2 * mult * (Q @ (sn2 * alpha)) if p == sfc else Q @ (dK[p] @ alpha))
    w += [mult * (Q @ (e[n] * alpha)) for n in range(noise_N)]
    w += [Q @ dm[:, kk] for kk in range(mean_N)]
    fmu = k.T @ alpha
    dfmu = np.empty((M, P), dtype=dtype)
    for p in range(P):
        dfmu[:, p] = -(k.T @ w[p])
        if p < cov_N:
            dfmu[:, p] += dk[p].T @ alpha
    if not compute_var:
        return fmu, None, dfmu, None
    _, sf2, _ = scales(kind, degree, hyp_cov, D, dtype)
    q = Q @ k
    fs2 = sf2 - np.sum(k * q, 0)
    dfs2 = np.zeros((M, P), dtype=dtype)
    for p in range(cov_N):
        if p == sfc:
            dfs2[:, p] = 2 * fs2 - 2 * mult * (sn2 @ (q * q))
        else:
            dfs2[:, p] = -2 * np.sum(dk[p] * q, 0) + np.sum(q * (dK[p] @ q), 0)
    for n in range(noise_N):
        dfs2[:, cov_N + n] = mult * (e[n] @ (q * q))
    return fmu, fs2, dfmu, dfs2


def delta_variance(g, cov, free):
    """g^T Sigma g per query for gradients g (M, P) restricted to the coordinates ``free`` the covariance ``cov``
    (k, k) lives on: the first-order (delta-method) variance of a function of the hyperparameters."""
    gf = np.asarray(g, dtype=float)[:, np.asarray(free, dtype=int)]
    return np.einsum("ma,ab,mb->m", gf, np.asarray(cov, dtype=float), gf)
