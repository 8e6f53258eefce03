"""The posterior of the gradient (``GP.gradient_posterior``), restated in vectorised NumPy.

For hyperparameter sample s and query x*, the joint Gaussian of (f(x*), grad f(x*)) -- slot 0 = f, slot 1 + l = d/dx_l::

    B      = [ k(X, x*) | G ],   G[i, l] = dk(x*, X_i) / dx*_l = -c_l F_i (xs*_l - xs_il)
    H      = diag(kss, F0 c_1^2, ..., F0 c_D^2)
    mean   = B^T alpha                                        (+ the mean function's value and gradient: the caller's)
    C      = H - V^T V,   V = L^-T (sW B)                     (L_chol: L the upper Cholesky factor of sW K sW + I)
    C      = H + B^T (L B)                                    (low noise: L = -(K + Sigma)^-1)

``xs`` are the kernel family's scaled inputs (the device's ``mul / dv`` scaling, the Matern sqrt(degree) inside),
c_l = d xs_l / d x_l, and F the radial factor dk/dlog(ell_l) = F (xs_l - xs'_l)^2, so dk/dxs*_l = -F (xs*_l - xs_l).
A pair at distance 0 contributes 0 to G.  H is diagonal because the kernels are stationary: dk(x, x')/dx vanishes at
x = x', and d^2 k / dx_l dx'_l at x = x' is F0 c_l^2 with F0 = F at distance 0 (``f0``: the same radial function
evaluated at 0, not a table).  The Matern kernel of degree 1 has F0 = infinity: no mean-square derivative.

The module is the product's path for a GP without data (the prior: H), holds the mixture over samples, and is the
model the device (``gpc_grad_post``) is tested against.
"""

import numpy as np

K_SE, K_MATERN, K_RQ, K_SE_ISO, K_MATERN_ISO = 0, 1, 2, 3, 4
_MATERN = (K_MATERN, K_MATERN_ISO)


def check_kind(kind, degree):
    if kind not in (K_SE, K_MATERN, K_RQ, K_SE_ISO, K_MATERN_ISO):
        raise ValueError(f"unknown kernel id {kind}")
    if kind in _MATERN and degree not in (1, 3, 5):
        raise ValueError(f"Matern degree must be 1, 3 or 5, got {degree}")
    if kind in _MATERN and degree == 1:
        raise NotImplementedError("gradient_posterior: the Matern kernel of degree 1 has no mean-square derivative "
                                  "(the prior variance of its gradient is infinite)")


def scaling(kind, degree, hyp_cov, D):
    """(c (D,), sf2, rq_alpha): c_l = d xs_l / d x_l of the kernel family's scaled inputs xs = x c."""
    hyp_cov = np.asarray(hyp_cov, dtype=float).ravel()
    snu = np.sqrt(float(degree)) if kind in _MATERN else 1.0
    if kind in (K_SE_ISO, K_MATERN_ISO):
        return np.full(D, snu / np.exp(hyp_cov[0])), np.exp(2 * hyp_cov[1]), 1.0
    rqa = np.exp(hyp_cov[D + 1]) if kind == K_RQ else 1.0
    return snu / np.exp(hyp_cov[:D]), np.exp(2 * hyp_cov[D]), rqa


def radial(kind, degree, r2, sf2, rqa=1.0):
    """(k, F) at squared scaled distance r2: the covariance and its radial factor (dk/dxs*_l = -F (xs*_l - xs_l))."""
    r2 = np.asarray(r2, dtype=float)
    if kind in (K_SE, K_SE_ISO):
        k = sf2 * np.exp(-r2 / 2)
        return k, k
    if kind in _MATERN:
        t = np.sqrt(r2)
        e = sf2 * np.exp(-t)
        if degree == 1:
            with np.errstate(divide="ignore"):
                return e, e / t
        if degree == 3:
            return e * (1 + t), e
        return e * (1 + t * (1 + t / 3)), e * (1 + t) / 3
    m = 1 + r2 / (2 * rqa)
    k = sf2 * m ** (-rqa)
    return k, k / m


def f0(kind, degree, sf2, rqa=1.0):
    """F at distance 0: d^2 k / dxs_l dxs'_l at coincident points."""
    return float(radial(kind, degree, 0.0, sf2, rqa)[1])


def prior_block(kind, degree, hyp_cov, D):
    """diag(H) (D + 1,): the prior variances of f and of its D partial derivatives."""
    check_kind(kind, degree)
    c, sf2, rqa = scaling(kind, degree, hyp_cov, D)
    return np.concatenate([[float(radial(kind, degree, 0.0, sf2, rqa)[0])], f0(kind, degree, sf2, rqa) * c * c])


def operand(kind, degree, hyp_cov, X, x_star):
    """B (N, D + 1, M): slot 0 = k(X_i, x*_j), slot 1 + l = dk(x*_j, X_i) / dx*_jl."""
    X, x_star = np.asarray(X, dtype=float), np.asarray(x_star, dtype=float)
    D = X.shape[1]
    c, sf2, rqa = scaling(kind, degree, hyp_cov, D)
    diff = (x_star * c)[None, :, :] - (X * c)[:, None, :]  # xs*_jl - xs_il (N, M, D): differences before products
    r2 = np.zeros(diff.shape[:2])
    for l in range(D):  # ascending l, as the device sums
        r2 += diff[:, :, l] ** 2
    with np.errstate(all="ignore"):
        k, F = radial(kind, degree, r2, sf2, rqa)
    F = np.where(r2 > 0, F, 0.0)
    B = np.empty((X.shape[0], D + 1, x_star.shape[0]))
    B[:, 0, :] = k
    B[:, 1:, :] = np.transpose(-F[:, :, None] * diff * c, (0, 2, 1))
    return B


def joint(kind, degree, hyp_cov, X, x_star, alpha, sW, L, L_chol):
    """(mean (M, D + 1), cov (M, D + 1, D + 1)) of (f, grad f) at every row of x_star under ONE posterior record
    (alpha (N, 1), sW (N, 1), L (N, N), L_chol), without the mean function.  The matrix is returned as computed."""
    import scipy.linalg as sla

    check_kind(kind, degree)
    X = np.asarray(X, dtype=float)
    N, D = X.shape
    B = operand(kind, degree, hyp_cov, X, x_star)
    M = B.shape[2]
    H = np.diag(prior_block(kind, degree, hyp_cov, D))
    mean = np.einsum("iaj,i->ja", B, np.asarray(alpha, dtype=float).ravel())
    flat = B.reshape(N, (D + 1) * M)
    if L_chol:
        V = sla.solve_triangular(L, np.asarray(sW, dtype=float).reshape(N, 1) * flat, trans=1, check_finite=False)
        V = V.reshape(N, D + 1, M)
        cov = H[None] - np.einsum("iaj,ibj->jab", V, V)
    else:
        Z = (np.asarray(L, dtype=float) @ flat).reshape(N, D + 1, M)
        cov = H[None] + np.einsum("iaj,ibj->jab", B, Z)
    return mean, cov


def mix(mean, cov):
    """Moments of the equal-weight mixture of the per-sample Gaussians: mean (M, P, S), cov (M, P, P, S) ->
    (M, P), (M, P, P): the mean of the means, and the mean of the covariances plus the between-sample covariance of
    the mean vectors with divisor S - 1 (``GP.predict``'s convention).  One sample is returned as it is."""
    S = mean.shape[2]
    if S == 1:
        return mean[:, :, 0], cov[:, :, :, 0]
    centre = np.sum(mean, 2) / S
    dev = mean - centre[:, :, None]
    return centre, np.sum(cov, 3) / S + np.einsum("mas,mbs->mab", dev, dev) / (S - 1)


def mix_diag(mean, var):
    """``mix`` for the diagonal alone: mean (M, P, S), var (M, P, S) -> (M, P), (M, P)."""
    S = mean.shape[2]
    if S == 1:
        return mean[:, :, 0], var[:, :, 0]
    centre = np.sum(mean, 2) / S
    return centre, np.sum(var, 2) / S + np.sum((mean - centre[:, :, None]) ** 2, 2) / (S - 1)
