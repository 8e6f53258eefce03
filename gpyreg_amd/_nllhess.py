"""The Hessian of the negative log marginal likelihood with respect to the hyperparameters (``GP.nll_hess_batch``),
restated in vectorised NumPy.

Sigma = K + mult diag(sn2) at a FIXED jitter multiplier, Q = Sigma^-1, alpha = Q (y - m), Qm = Q - alpha alpha^T,
hyperparameters ordered [cov | noise | mean].  Every covariance and noise hyperparameter p is a plane d_p Sigma; with
B_p = Q d_p Sigma, u_p = d_p Sigma alpha, w_p = Q u_p and, for mean hyperparameter k, v_k = Q d_k m::

    nlZ    = 1/2 (y - m)^T alpha + 1/2 log det Sigma + N/2 log 2 pi
    g[p]   = 1/2 <Qm, d_p Sigma>                       g[k] = -alpha . d_k m
    H[p,q] = -1/2 tr(B_p B_q) + u_p . w_q + 1/2 <Qm, d2_pq Sigma>          planes p, q
    H[p,k] =  w_p . d_k m                                                   plane p, mean k
    H[k,l] =  d_k m . v_l - alpha . d2_kl m                                 mean k, l

On log scales, with xs the kernel family's scaled inputs, d_a the difference of coordinate a, r2 = sum_a d_a^2, F the
radial factor (dK / d log ell_a = F d_a^2) and G = -2 dF/d(r2) (``_hess.radial2``)::

    d K / d log ell_a = F d_a^2 (isotropic: F r2)      d K / d log sf = 2 K      d K / d log alpha_RQ = Ka
    ell_a x ell_b   G d_a^2 d_b^2 - 2 delta_ab F d_a^2          (isotropic: G r2^2 - 2 F r2)
    sf x ell_a      2 F d_a^2         sf x sf   4 K            sf x shape   2 Ka
    shape x ell_a   Fa d_a^2          Fa  = dF / d log alpha  = F (h + r2 / (2 alpha M))
    shape x shape   Kaa               Kaa = dKa / d log alpha = K (h^2 + h + r2^2 / (4 alpha M^2))
                    (M = 1 + r2 / (2 alpha),  h = r2 / (2 M) - alpha log M,  Ka = K h)

A pair at r2 = 0 contributes nothing to a lengthscale term (Matern 3 has G = infinity there; G d^2 d^2 -> 0).  The
Matern kernel of degree 1 has no G.  Noise planes are mult diag(d_n sn2), their second derivatives
mult diag(d2_nn' sn2); both plugin second derivatives (``noise_d2``, ``mean_d2``) and the priors' (``prior_d2``) live
here too.

Every function takes ``dtype`` (float64 or longdouble: the factorisation is then a plain NumPy loop, since LAPACK has
no extended precision).  The module is the model the device (``gpc_nll_hess``) is tested against.
"""

import numpy as np

from ._gradpost import K_MATERN, K_MATERN_ISO, K_RQ, K_SE, K_SE_ISO

_MATERN = (K_MATERN, K_MATERN_ISO)
_ISO = (K_SE_ISO, K_MATERN_ISO)


def check_kind(kind, degree, who="nll_hess_batch"):
    if kind not in (K_SE, K_MATERN, K_RQ, K_SE_ISO, K_MATERN_ISO):
        raise ValueError(f"unknown kernel id {kind}")
    if kind in _MATERN and degree not in (1, 3, 5):
        raise ValueError(f"Matern degree must be 1, 3 or 5, got {degree}")
    if kind in _MATERN and degree == 1:
        raise NotImplementedError(f"{who}: the Matern kernel of degree 1 has no second derivative with respect to its "
                                  "lengthscales (no second radial factor G)")


def cov_count(kind, D):
    return 2 if kind in _ISO else (D + 2 if kind == K_RQ else D + 1)


def scaled_sq_diffs(kind, degree, hyp_cov, X, dtype=np.float64, xs=None):
    """(d2 (D, N, N): squared differences of the scaled coordinates -- differences before products --, r2 (N, N) summed
    in ascending dimension, sf2, rq_alpha).  ``xs``: the scaled inputs, when the caller has formed them itself (the
    device scales as x mul / dv, one rounding apart from x c)."""
    X = np.asarray(X, dtype=dtype)
    h = np.asarray(hyp_cov, dtype=dtype).ravel()
    D = X.shape[1]
    snu = np.sqrt(dtype(degree)) if kind in _MATERN else dtype(1)
    if kind in _ISO:
        c, sf2, rqa = np.full(D, snu / np.exp(h[0]), dtype=dtype), np.exp(2 * h[1]), dtype(1)
    else:
        c, sf2 = snu / np.exp(h[:D]), np.exp(2 * h[D])
        rqa = np.exp(h[D + 1]) if kind == K_RQ else dtype(1)
    xs = X * c if xs is None else np.asarray(xs, dtype=dtype)
    d2 = np.empty((D,) + (X.shape[0],) * 2, dtype=dtype)
    r2 = np.zeros((X.shape[0],) * 2, dtype=dtype)
    for a in range(D):
        d = xs[:, None, a] - xs[None, :, a]
        d2[a] = d * d
        r2 += d2[a]
    return d2, r2, sf2, rqa


def radial(kind, degree, r2, sf2, rqa):
    """dict of the radial functions at r2: K, F, G (0 where r2 = 0) and, for the rational quadratic, Ka, Fa, Kaa."""
    one = r2.dtype.type(1)
    out = {}
    if kind in (K_SE, K_SE_ISO):
        K = sf2 * np.exp(-r2 / 2)
        out.update(K=K, F=K, G=K)
    elif kind in _MATERN:
        t = np.sqrt(r2)
        e = sf2 * np.exp(-t)
        if degree == 3:
            with np.errstate(divide="ignore", invalid="ignore"):
                out.update(K=e * (1 + t), F=e, G=e / t)
        elif degree == 5:
            out.update(K=e * (1 + t * (1 + t / 3)), F=e * (1 + t) / 3, G=e / 3)
        else:
            raise NotImplementedError("the Matern kernel of degree 1 has no second radial factor")
    else:
        M = one + r2 / (2 * rqa)
        lM = np.log(M)
        K = sf2 * np.exp(-rqa * lM)
        F = K / M
        h = r2 / (2 * M) - rqa * lM
        out.update(K=K, F=F, G=(rqa + 1) / rqa * F / M, Ka=K * h, Fa=F * (h + r2 / (2 * rqa * M)),
                   Kaa=K * (h * h + h + r2 * r2 / (4 * rqa * M * M)))
    out["G"] = np.where(r2 > 0, out["G"], 0)
    return out


def cov_derivatives(kind, degree, hyp_cov, X, dtype=np.float64, xs=None):
    """(K, dK: list of cov_N planes (N, N), second(p, q) -> (N, N) for p >= q)."""
    D = np.shape(X)[1]
    d2, r2, sf2, rqa = scaled_sq_diffs(kind, degree, hyp_cov, X, dtype, xs)
    R = radial(kind, degree, r2, sf2, rqa)
    K, F, G = R["K"], R["F"], R["G"]
    if kind in _ISO:
        dK = [F * r2, 2 * K]

        def second(p, q):
            if p == 0:
                return G * r2 * r2 - 2 * F * r2
            return 2 * F * r2 if q == 0 else 4 * K
        return K, dK, second
    dK = [F * d2[a] for a in range(D)] + [2 * K]
    if kind == K_RQ:
        dK.append(R["Ka"])

    def second(p, q):
        if p < D:
            return G * d2[p] * d2[q] - (2 * F * d2[p] if p == q else 0)
        if p == D:
            return 2 * F * d2[q] if q < D else 4 * K
        if q < D:
            return R["Fa"] * d2[q]
        return 2 * R["Ka"] if q == D else R["Kaa"]
    return K, dK, second


def spd_inverse(A):
    """(A^-1, log det A) of a symmetric positive definite matrix in A's own dtype: LAPACK for float64, a NumPy Cholesky
    loop for longdouble."""
    A = np.asarray(A)
    n = A.shape[0]
    if A.dtype == np.float64:
        L = np.linalg.cholesky(A)
        Li = np.linalg.solve(L, np.eye(n))
        return Li.T @ Li, 2 * np.sum(np.log(np.diag(L)))
    L = np.zeros_like(A)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise np.linalg.LinAlgError("matrix is not positive definite")
        L[j:, j] = v / np.sqrt(v[0])
    Li = np.zeros_like(A)
    for i in range(n):  # row i of L^-1 by forward substitution
        e = np.zeros(n, dtype=A.dtype)
        e[i] = 1
        Li[i] = (e - L[i, :i] @ Li[:i]) / L[i, i]
    return Li.T @ Li, 2 * np.sum(np.log(np.diag(L)))


def nll_hess(kind, degree, hyp_cov, X, resid, sn2, mult=1.0, dm=None, dsn2=None, d2sn2=None, d2m=None,
             dtype=np.float64, parts=False):
    """(nlZ, g (P,), H (P, P)) for ONE hyperparameter vector.

    resid = y - m (N,); sn2 (N,) or a scalar; mult the jitter multiplier; dm (N, mean_N) | None; dsn2 (N | 1, noise_N)
    | None; d2sn2 (N | 1, noise_N, noise_N) and d2m (N, mean_N, mean_N): the plugins' second derivatives, None leaves
    their terms out (what ``gpc_nll_hess`` returns).  ``parts``: also the dict of (Q, alpha, diagq)."""
    check_kind(kind, degree)
    X = np.asarray(X, dtype=dtype)
    N = X.shape[0]
    r = np.asarray(resid, dtype=dtype).ravel()
    sn2 = np.broadcast_to(np.asarray(sn2, dtype=dtype).ravel(), (N,))
    mult = dtype(mult)
    K, dK, second = cov_derivatives(kind, degree, hyp_cov, X, dtype)
    cov_N = len(dK)
    dm = np.zeros((N, 0), dtype=dtype) if dm is None else np.asarray(dm, dtype=dtype).reshape(N, -1)
    noise_N = 0 if dsn2 is None else np.shape(dsn2)[-1]
    e = np.zeros((noise_N, N), dtype=dtype)
    if noise_N:
        e[:] = mult * np.broadcast_to(np.asarray(dsn2, dtype=dtype).reshape(-1, noise_N), (N, noise_N)).T
    mean_N = dm.shape[1]
    ppl, P = cov_N + noise_N, cov_N + noise_N + mean_N
    Q, logdet = spd_inverse(K + np.diag(mult * sn2))
    Q = (Q + Q.T) / 2
    alpha = Q @ r
    Qm = Q - np.outer(alpha, alpha)
    diagq = np.diag(Qm).copy()
    B = [Q @ dK[p] for p in range(cov_N)] + [Q * e[n][None, :] for n in range(noise_N)]
    u = [dK[p] @ alpha for p in range(cov_N)] + [e[n] * alpha for n in range(noise_N)]
    w = [Q @ up for up in u]
    v = [Q @ dm[:, k] for k in range(mean_N)]
    g = np.zeros(P, dtype=dtype)
    H = np.zeros((P, P), dtype=dtype)
    for p in range(ppl):
        g[p] = np.sum(Qm * dK[p]) / 2 if p < cov_N else np.sum(diagq * e[p - cov_N]) / 2
        for q in range(p + 1):
            val = -np.sum(B[p] * B[q].T) / 2 + u[p] @ w[q]
            if p < cov_N:
                val += np.sum(Qm * second(p, q)) / 2
            elif q >= cov_N and d2sn2 is not None:
                dd = np.broadcast_to(np.asarray(d2sn2, dtype=dtype).reshape(-1, noise_N, noise_N), (N, noise_N, noise_N))
                val += mult * np.sum(diagq * dd[:, p - cov_N, q - cov_N]) / 2
            H[p, q] = H[q, p] = val
    for k in range(mean_N):
        g[ppl + k] = -(alpha @ dm[:, k])
        for p in range(ppl):
            H[ppl + k, p] = H[p, ppl + k] = w[p] @ dm[:, k]
        for l in range(k + 1):
            val = dm[:, k] @ v[l]
            if d2m is not None:
                val -= alpha @ np.asarray(d2m, dtype=dtype)[:, k, l]
            H[ppl + k, ppl + l] = H[ppl + l, ppl + k] = val
    nlz = (r @ alpha) / 2 + logdet / 2 + N * np.log(2 * dtype(np.pi)) / 2
    if parts:
        return nlz, g, H, dict(Q=Q, alpha=alpha, diagq=diagq)
    return nlz, g, H


# ---- the plugins' second derivatives ----------------------------------------------------------------------------------
def noise_d2(noise, hyp_noise, X, y, s2=None):
    """d^2 sn2 / d theta d theta' of the stock ``GaussianNoise``: (R, noise_N, noise_N), R = N when the noise is per
    point (``noise.per_point``) else 1, for one hyperparameter vector.  Exact type only."""
    from .noise_functions import GaussianNoise

    if type(noise) is not GaussianNoise:
        raise NotImplementedError(f"nll_hess_batch: the noise function {noise!r} ({type(noise).__name__}) is user-defined; "
                                  "its second derivatives with respect to the hyperparameters are unknown")
    h = np.asarray(hyp_noise, dtype=float).ravel()
    N = X.shape[0]
    const, provided, rect = noise.parameters
    nN = noise.hyperparameter_count()
    wide = noise.per_point(y, s2)
    out = np.zeros((N if wide else 1, nN, nN))
    col = 0
    if const == 1:
        out[:, col, col] = 4 * np.exp(2 * h[col])
        col += 1
    if provided == 2:
        given = 0 if s2 is None else (s2 if np.isscalar(s2) else np.reshape(s2, (N,)))
        out[:, col, col] = np.exp(h[col]) * given
        col += 1
    if rect == 1:
        if y is not None:
            w2 = np.exp(2 * h[col + 1])
            gap = h[col] - np.reshape(y, (N,))
            below = np.maximum(0, gap)
            on = (below > 0).astype(float)
            out[:, col, col] = 2 * w2 * on
            out[:, col, col + 1] = out[:, col + 1, col] = 4 * w2 * gap * on
            out[:, col + 1, col + 1] = 4 * w2 * below**2
        col += 2
    return out


def mean_d2(mean, hyp_mean, X):
    """d^2 m / d theta d theta' (N, mean_N, mean_N) of a stock mean function for one hyperparameter vector."""
    from .mean_functions import ConstantMean, NegativeQuadratic, ZeroMean

    N, D = X.shape
    if type(mean) is ZeroMean:
        return np.zeros((N, 0, 0))
    if type(mean) is ConstantMean:
        return np.zeros((N, 1, 1))
    if type(mean) is NegativeQuadratic:
        h = np.asarray(hyp_mean, dtype=float).ravel()
        om2 = np.exp(2 * h[1 + D:1 + 2 * D])
        delta = X - h[1:1 + D]
        out = np.zeros((N, 1 + 2 * D, 1 + 2 * D))
        for d in range(D):
            i, j = 1 + d, 1 + D + d
            out[:, i, i] = -1 / om2[d]
            out[:, i, j] = out[:, j, i] = -2 * delta[:, d] / om2[d]
            out[:, j, j] = -2 * delta[:, d] ** 2 / om2[d]
        return out
    raise NotImplementedError(f"nll_hess_batch: the mean function {mean!r} ({type(mean).__name__}) is user-defined; its "
                              "second derivatives with respect to the hyperparameters are unknown")


def prior_d2(hyp, hp, lb, ub):
    """The diagonal (P,) of the Hessian of ``priors.log_priors`` (the four families are products over dimensions):
    Gaussian -1 / sigma^2; Student-t -(df + 1) / (df sigma^2) (1 - s) / (1 + s)^2, s = z^2 / df; the smooth boxes the
    same about the nearer edge outside [a, b] and 0 inside; uniform 0; a fixed dimension NaN, as its gradient."""
    from . import priors as _pr

    hyp = np.asarray(hyp, dtype=float)
    mu, sigma, df, a, b = hp["mu"], np.abs(hp["sigma"]), hp["df"], hp["a"], hp["b"]
    ix = _pr.classify(hp, lb, ub)
    out = np.zeros(hyp.shape)

    def student(x, sel):
        s = (x / sigma[sel]) ** 2 / df[sel]
        return -(df[sel] + 1) / (df[sel] * sigma[sel] ** 2) * (1 - s) / (1 + s) ** 2

    for cls, t in (("sb", False), ("sb_t", True)):
        for edge, side in ((a, hyp < a), (b, hyp > b)):
            sel = ix[cls] & side
            if np.any(sel):
                out[sel] = student(hyp[sel] - edge[sel], sel) if t else -1 / sigma[sel] ** 2
    g, t = ix["gauss"], ix["stud"]
    out[g] = -1 / sigma[g] ** 2
    if np.any(t):
        out[t] = student(hyp[t] - mu[t], t)
    out[ix["fixed"]] = np.nan
    return out
