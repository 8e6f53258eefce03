"""Pathwise posterior samples (``GP.sample_paths``), restated in vectorised NumPy on top of ``_philox``.

Matheron's rule with random Fourier features.  Per hyperparameter sample s (global index) and path r::

    f_{s,r}(x) = m_s(x) + p_{s,r}(x) + k_s(x, X) v_{s,r}
    p_{s,r}(x) = sqrt(2 sf2_s / F) sum_{f<F} wt_s[f][r] cos(theta_s[f] . xs(x) + b_s[f])
    v_{s,r}    = (K_s + Sigma_s)^-1 (y - m_s(X) - p_{s,r}(X) - eps_{s,r}),   eps_{s,r}[i] = sqrt(sn2_s[i] sn2_mult_s) e_s[i][r]

``xs`` are the kernel family's scaled inputs (``scale_inputs``: the device's ``mul / dv`` scaling, the Matern
sqrt(degree) inside).  On scaled inputs the spectral draw is theta[f][l] = z[f][l] for the squared exponential and
z[f][l] / sqrt(c[f]), c[f] = sum_{q<d} g[f][q]^2, for Matern of degree d (the multivariate Student-t with d degrees
of freedom).  Streams of the Philox key (seed, stream), all through ``_philox.normals(seed, stream, s, r, j)``:

    2  z[f][l]  = normals(r=l, j=f)        3  g[f][q] = normals(r=q, j=f)
    4  b[f]     = 2 pi (word(r=0, j=f) >> 11) 2^-53
    5  wt[f][r] = normals(r=r, j=f)        6  e[i][r] = normals(r=r, j=i)

so path r of sample s does not depend on the number of paths, the batch of samples, the chunking or the sharding.

The module is the product's path for a GP without data (prior paths, v = 0) and the model the device
(``gpc_paths_create`` / ``gpc_paths_eval``) is tested against.  The mean function is the caller's.
"""

import numpy as np

from . import _philox

K_SE, K_MATERN, K_RQ, K_SE_ISO, K_MATERN_ISO = 0, 1, 2, 3, 4
_MATERN = (K_MATERN, K_MATERN_ISO)
_SUPPORTED = (K_SE, K_MATERN, K_SE_ISO, K_MATERN_ISO)


def _check_kind(kind, degree):
    if kind not in _SUPPORTED:
        raise NotImplementedError("sample_paths: the spectral draw is defined for the squared-exponential and Matern "
                                  f"kernels only (kernel id {kind})")
    if kind in _MATERN and degree not in (1, 3, 5):
        raise ValueError(f"Matern degree must be 1, 3 or 5, got {degree}")


def features(kind, degree, D, F, seed, s):
    """(theta (F, D), b (F,)) of sample ``s``: the spectral draw on SCALED inputs and the phases."""
    _check_kind(kind, degree)
    f = np.arange(F).reshape(-1, 1)
    theta = _philox.normals(seed, 2, s, np.arange(D).reshape(1, -1), f)
    if kind in _MATERN:
        g = _philox.normals(seed, 3, s, np.arange(degree).reshape(1, -1), f)
        theta = theta / np.sqrt(np.sum(g * g, axis=1, keepdims=True))
    w = _philox.words(seed, 4, s, 0, np.arange(F))
    b = 2.0 * np.pi * ((w >> np.uint64(11)).astype(np.float64) * 2.0**-53)
    return theta, b


def weights(F, R, seed, s):
    """wt (F, R): the feature weights of the R paths of sample ``s``."""
    return _philox.normals(seed, 5, s, np.arange(R).reshape(1, -1), np.arange(F).reshape(-1, 1))


def noise(N, R, seed, s):
    """e (N, R): the standard normals behind the observation-noise draws eps of sample ``s``."""
    return _philox.normals(seed, 6, s, np.arange(R).reshape(1, -1), np.arange(N).reshape(-1, 1))


def scale_inputs(kind, degree, hyp_cov, X):
    """(xs (N, D), c (D,), sf2): the scaled inputs x mul / dv of the kernel family, c_l = mul_l / dv_l = d xs_l / d x_l."""
    _check_kind(kind, degree)
    X = np.asarray(X, dtype=float)
    hyp_cov = np.asarray(hyp_cov, dtype=float).ravel()
    D = X.shape[1]
    snu = np.sqrt(float(degree)) if kind in _MATERN else 1.0
    if kind in (K_SE_ISO, K_MATERN_ISO):
        ell = np.exp(hyp_cov[0])
        mul, dv, sf2 = np.full(D, snu), np.full(D, ell), np.exp(2 * hyp_cov[1])
    elif kind == K_SE:
        mul, dv, sf2 = np.ones(D), np.exp(hyp_cov[:D]), np.exp(2 * hyp_cov[D])
    else:
        mul, dv, sf2 = snu / np.exp(hyp_cov[:D]), np.ones(D), np.exp(2 * hyp_cov[D])
    return X * mul / dv, mul / dv, sf2


def pair(kind, degree, r2, sf2):
    """(K, Fr) of squared scaled distances ``r2``: the covariance and its radial factor, dK / dx*_l =
    Fr (xs_l - xs*_l) c_l.  A pair at distance 0 has Fr = 0 (the limit; Matern 1: the convention)."""
    _check_kind(kind, degree)
    r2 = np.asarray(r2, dtype=float)
    if kind in (K_SE, K_SE_ISO):
        K = sf2 * np.exp(-0.5 * r2)
        Fr = K
    else:
        t = np.sqrt(r2)
        e = sf2 * np.exp(-t)
        if degree == 1:
            K = e
            with np.errstate(divide="ignore", invalid="ignore"):
                Fr = e / t
        elif degree == 3:
            K, Fr = e * (1 + t), e
        else:
            K, Fr = e * (1 + t * (1 + t / 3)), e * (1 + t) / 3
    return K, np.where(r2 > 0, Fr, 0.0)


def prior_part(xs, c, sf2, theta, b, wt, compute_grad=False):
    """p (M, R) at scaled inputs ``xs`` (M, D) and, with the gradient, dp / dx (M, D, R)."""
    F = theta.shape[0]
    scale = np.sqrt(2.0 * sf2 / F)
    arg = xs @ theta.T + b
    p = scale * (np.cos(arg) @ wt)
    if not compute_grad:
        return p
    sw = np.sin(arg)
    dp = -scale * np.einsum("mf,fl,fr->mlr", sw, theta, wt, optimize=True) * c[None, :, None]
    return p, dp


def evaluate(kind, degree, hyp_cov, X, v, theta, b, wt, x_star, compute_grad=False):
    """f (M, R) = p(x*) + k(x*, X) v without the mean function and, with the gradient, df / dx* (M, D, R).
    ``X`` (N, D) the unscaled training inputs (None or N = 0: the prior part alone), ``v`` (N, R)."""
    x_star = np.atleast_2d(np.asarray(x_star, dtype=float))
    xq, c, sf2 = scale_inputs(kind, degree, hyp_cov, x_star)
    out = prior_part(xq, c, sf2, theta, b, wt, compute_grad)
    f, df = out if compute_grad else (out, None)
    if X is not None and len(X):
        xt, _, _ = scale_inputs(kind, degree, hyp_cov, X)
        diff = xq[:, None, :] - xt[None, :, :]  # (M, N, D)
        K, Fr = pair(kind, degree, np.sum(diff * diff, axis=2), sf2)
        f = f + K @ v
        if compute_grad:  # dK_ji / dx*_jl = -c_l Fr_ji (xs*_jl - xs_il)
            df = df - np.einsum("mn,mnl,nr->mlr", Fr, diff, v, optimize=True) * c[None, :, None]
    return (f, df) if compute_grad else f
