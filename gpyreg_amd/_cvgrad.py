"""The leave-one-out cross-validation objective and its gradient with respect to the hyperparameters
(``GP.cv_nll_batch``), restated in vectorised NumPy.

Sigma = K + mult diag(sn2) at a FIXED jitter multiplier, Q = Sigma^-1, alpha = Q (y - m), q_i = Q_ii.  Leaving point i
out, the hyperparameters held fixed, predicts y_i with mean mu_i = y_i - alpha_i / q_i and variance 1 / q_i (Rasmussen &
Williams 5.4.2).  With per-point weights w_i >= 0 (default 1)::

    loss "lpd":  L = -sum_i w_i (1/2 log q_i - alpha_i^2 / (2 q_i) - 1/2 log 2 pi)
                 c_i = w_i (1 + alpha_i^2 / q_i) / (2 q_i)         b_i = w_i alpha_i / q_i
    loss "mse":  L =  sum_i w_i (alpha_i / q_i)^2
                 c_i = 2 w_i alpha_i^2 / q_i^3                     b_i = 2 w_i alpha_i / q_i^2

c = -dL/dq and b = dL/dalpha.  With d_p Q = -Q d_p Sigma Q and d_p alpha = -Q d_p Sigma alpha every derivative of L is a
contraction with ONE symmetric weight matrix::

    beta = Q b
    G = Q diag(c) Q - 1/2 (beta alpha^T + alpha beta^T)

    dL / d theta_p = <d_p K, G>                     covariance hyperparameter p (``_nllhess.cov_derivatives``' planes)
                   = mult sum_i G_ii d_n sn2_i      noise hyperparameter n
                   = -beta . d_k m                  mean hyperparameter k

"lpd" is the negative leave-one-out log predictive density (the log pseudo-likelihood of R&W 5.4.2, negated).
Hyperparameters are ordered [cov | noise | mean].  A pair at r2 = 0 contributes nothing to a lengthscale term.  The
Matern kernel of degree 1 is refused: its radial factor F is infinite on the diagonal.

Every function takes ``dtype`` (float64 or longdouble).  The module is the model the device (``gpc_cv_grad``) is tested
against.
"""

import numpy as np

from ._nllhess import _MATERN, cov_derivatives, spd_inverse

LOSSES = ("lpd", "mse")


def check_kind(kind, degree, who="cv_nll_batch"):
    if kind in _MATERN and degree == 1:
        raise NotImplementedError(f"{who}: the Matern kernel of degree 1 has an infinite radial factor on the diagonal; "
                                  "its lengthscale planes are not formed")


def check_loss(loss, who="cv_nll_batch"):
    if loss not in LOSSES:
        raise ValueError(f"{who}: loss must be one of {LOSSES}, got {loss!r}")


def check_weights(weights, N=None, who="cv_nll_batch"):
    """``weights`` as a float64 vector (None stays None): (N,), finite and >= 0."""
    if weights is None:
        return None
    w = np.asarray(weights, dtype=float)
    if w.ndim != 1 or (N is not None and w.size != N):
        raise ValueError(f"{who}: weights must have shape (N,)" + ("" if N is None else f" = ({N},)") + f", got {w.shape}")
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError(f"{who}: weights must be finite and >= 0")
    return w


def loo_weights(alpha, q, loss, weights=None):
    """(c, b) of the module's header for the vectors alpha, q."""
    w = 1 if weights is None else weights
    if loss == "lpd":
        return w * (1 + alpha * alpha / q) / (2 * q), w * alpha / q
    return 2 * w * alpha * alpha / (q * q * q), 2 * w * alpha / (q * q)


def loo_value(alpha, q, loss, weights=None):
    """L of the module's header from alpha, q (the last axis is summed)."""
    w = 1 if weights is None else weights
    if loss == "lpd":
        two_pi = 2 * np.asarray(q).dtype.type(np.pi)
        return -np.sum(w * (np.log(q) / 2 - alpha * alpha / (2 * q) - np.log(two_pi) / 2), axis=-1)
    return np.sum(w * (alpha / q) ** 2, axis=-1)


def assemble(gsum, diagG, beta, mult, dsn2=None, dm=None):
    """dL (P,) ordered [cov | noise | mean] from one sample's contraction sums gsum (cov_N,), diag(G) (N,) and beta
    (N,): dsn2 (N | 1, noise_N) | None without the multiplier, dm (N, mean_N) | None."""
    parts = [np.asarray(gsum)]
    N = diagG.shape[0]
    if dsn2 is not None and np.shape(dsn2)[-1]:
        ds = np.broadcast_to(np.asarray(dsn2, dtype=diagG.dtype).reshape(-1, np.shape(dsn2)[-1]), (N, np.shape(dsn2)[-1]))
        parts.append(mult * (diagG @ ds))
    if dm is not None and np.shape(dm)[-1]:
        parts.append(-(beta @ np.asarray(dm, dtype=diagG.dtype).reshape(N, -1)))
    return np.concatenate(parts)


def cv_nll(kind, degree, hyp_cov, X, resid, sn2, mult=1.0, dm=None, dsn2=None, loss="lpd", weights=None,
           dtype=np.float64, compute_grad=True, parts=False):
    """(L, dL (P,) | None) for ONE hyperparameter vector.

    resid = y - m (N,); sn2 (N,) or a scalar; mult the jitter multiplier; dm (N, mean_N) | None; dsn2 (N | 1, noise_N)
    | None; weights (N,) | None.  ``parts``: also the dict of (Q, alpha, q, c, b, beta, G)."""
    check_kind(kind, degree)
    check_loss(loss)
    X = np.asarray(X, dtype=dtype)
    N = X.shape[0]
    r = np.asarray(resid, dtype=dtype).ravel()
    sn2 = np.broadcast_to(np.asarray(sn2, dtype=dtype).ravel(), (N,))
    mult = dtype(mult)
    w = None if weights is None else np.asarray(check_weights(weights, N), dtype=dtype)
    K, dK, _ = cov_derivatives(kind, degree, hyp_cov, X, dtype)
    Q, _ = spd_inverse(K + np.diag(mult * sn2))
    Q = (Q + Q.T) / 2
    alpha = Q @ r
    q = np.diag(Q).copy()
    L = loo_value(alpha, q, loss, w)
    if not compute_grad:
        return (L, None, dict(Q=Q, alpha=alpha, q=q)) if parts else (L, None)
    c, b = loo_weights(alpha, q, loss, w)
    beta = Q @ b
    ba = np.outer(beta, alpha)
    G = (Q * c[None, :]) @ Q - (ba + ba.T) / 2
    gsum = np.array([np.sum(dK[p] * G) for p in range(len(dK))], dtype=dtype)
    g = assemble(gsum, np.diag(G).copy(), beta, mult, dsn2, dm)
    if parts:
        return L, g, dict(Q=Q, alpha=alpha, q=q, c=c, b=b, beta=beta, G=G, gsum=gsum)
    return L, g
