"""NumPy restatement of the point removal (``GP.remove_points``, ``gpc_post_remove``; csrc/remove.h has the kernels,
DESIGN.md "Point removal" the derivation): the same 64-column panels, the same Householder construction of every
panel's orthogonal Theta and the same two applications as the device path, for both parametrisations of a posterior.
It is what the tests compare the kernels with, panel by panel, and it needs no device.

Per sample, I = the sorted removed rows, R = the kept rows in order, n = N - k:

high noise (``Lo`` lower triangular with Lo Lo^T = K / sl + I, ``W`` = Lo^-1)
    Lr = Lo[R, R], Wr = W[R, R] (still lower triangular), V = Lo[R, I], C = W[I, R]; the new factor has
    L' L'^T = Lr Lr^T + V V^T.  For every panel [a, b) from the one that holds the first removed row on:
    [D | Vp] Theta = [D' | 0] with D = Lr[a:b, a:b], Vp = V[a:b, :], then
    [Lr[b:, a:b] | V[b:, :]] <- [...] Theta   and   [Wr[a:b, :b] ; C] <- Theta^T [Wr[a:b, :b] ; C].
    alpha' = W'^T (W' (y_R - m_R)) / sl, from the new factor.
low noise (``A`` = -(K + Sigma)^-1 = -Q, full symmetric)
    Q_II = Lq Lq^T,  H = A[R, I] Lq^-T:   A' = A[R, R] + H H^T,   alpha' = alpha_R + A[R, I] Q_II^-1 alpha_I.
"""

import numpy as np
import scipy.linalg as sla

PANEL = 64   # columns of a panel (remove.h: RM_P)
SWEEP = 64   # rows one sweep removes (remove.h: RM_KMAX); a larger k goes in consecutive sweeps


def check_indices(idx, N):
    """``idx`` as a sorted int array: an integer array or a boolean mask over the N rows.  Raises for anything that
    gpc_post_remove refuses (empty, all rows, repeated, out of range)."""
    idx = np.asarray(idx)
    if idx.dtype == bool:
        if idx.shape != (N,):
            raise ValueError("remove_points: a boolean mask must have one entry per training row (%d)" % N)
        idx = np.flatnonzero(idx)
    else:
        if idx.size and not np.issubdtype(idx.dtype, np.integer):
            raise ValueError("remove_points: idx must be an integer array or a boolean mask")
        idx = np.ravel(idx).astype(np.int64)
        if np.any(idx < -N) or np.any(idx >= N):
            raise IndexError("remove_points: index out of range for %d training rows" % N)
        idx = np.sort(np.where(idx < 0, idx + N, idx))
        if np.any(np.diff(idx) == 0):
            raise ValueError("remove_points: repeated index")
    if idx.size < 1:
        raise ValueError("remove_points: no row to remove")
    if idx.size >= N:
        raise ValueError("remove_points: at least one training row must remain")
    return idx


def swept_panels(N, idx):
    """The 64-column panels a removal of the sorted rows ``idx`` from N sweeps, summed over its sweeps of at most 64
    rows: each starts at the panel that holds its first removed row (rows removed from the end visit at most the last
    panel, with a zero carrier)."""
    idx = np.asarray(idx, dtype=int)
    panels = 0
    for j0 in range(0, idx.size, SWEEP):
        grp = idx[j0:j0 + SWEEP] - j0
        n = N - j0 - grp.size
        panels += max(0, -(-(n - (int(grp[0]) // PANEL) * PANEL) // PANEL))
    return panels


def panel_theta(D, Vp):
    """Theta (orthogonal, order p + k) with [D | Vp] Theta = [D' | 0], D (p x p) lower triangular, D' lower triangular
    with a positive diagonal.  Householder QR of [D | Vp]^T whose column j is (D[j, j], zeros, Vp[j, :]) below the
    diagonal: H_j = I - tau_j u_j u_j^T with u_j = e_j + [0 ; vn_j]; beta = +sqrt(d^2 + sigma), u1 = d - beta formed as
    -sigma / (d + beta); sigma = 0: H_j = I exactly.  Theta = H_0 H_1 ... H_{p-1}.  Returns (Theta, D')."""
    p, k = Vp.shape
    Dt = np.tril(np.asarray(D, dtype=float)).T.copy()   # Dt[j, c] = D[c, j]
    Vt = np.asarray(Vp, dtype=float).T.copy()           # Vt[i, c] = Vp[c, i]
    tau = np.zeros(p)
    for j in range(p):
        sigma = float(Vt[:, j] @ Vt[:, j])
        if sigma == 0.0:
            continue
        d = Dt[j, j]
        beta = np.sqrt(d * d + sigma)
        u1 = -sigma / (d + beta)
        inv, tau[j] = 1.0 / u1, -u1 / beta
        w = Dt[j, j + 1:] + inv * (Vt[:, j] @ Vt[:, j + 1:])
        tw = tau[j] * w
        Dt[j, j + 1:] -= tw
        Vt[:, j + 1:] -= np.outer(Vt[:, j] * inv, tw)
        Vt[:, j] *= inv          # vn_j, kept for the backward pass
        Dt[j, j] = beta
    theta = np.eye(p + k)
    for j in range(p - 1, -1, -1):
        if tau[j] == 0.0:
            continue
        vn = Vt[:, j]
        w = theta[j, :] + vn @ theta[p:, :]   # (row j is still e_j)
        tw = tau[j] * w
        theta[j, :] -= tw
        theta[p:, :] -= np.outer(vn, tw)
    return theta, Dt.T.copy()


def sweep_high(Lo, W, idx, thetas=None):
    """One sweep (k <= 64 rows) on a high-noise sample: (L', W').  ``thetas`` (a list) receives every panel's Theta."""
    N = Lo.shape[0]
    idx = np.asarray(idx, dtype=int)
    k = idx.size
    assert 1 <= k <= SWEEP and k < N
    keep = np.setdiff1d(np.arange(N), idx)
    n = keep.size
    Lr, Wr = np.tril(Lo[np.ix_(keep, keep)]), np.tril(W[np.ix_(keep, keep)])
    V = np.where(keep[:, None] > idx[None, :], Lo[np.ix_(keep, idx)], 0.0)
    C = np.where(keep[None, :] < idx[:, None], W[np.ix_(idx, keep)], 0.0)
    for a in range((int(idx[0]) // PANEL) * PANEL, n, PANEL):
        b = min(a + PANEL, n)
        p = b - a
        theta, Dn = panel_theta(Lr[a:b, a:b], V[a:b, :])
        if thetas is not None:
            thetas.append(theta)
        Lr[a:b, a:b] = Dn
        V[a:b, :] = 0.0
        low = np.hstack([Lr[b:, a:b], V[b:, :]]) @ theta
        Lr[b:, a:b], V[b:, :] = low[:, :p], low[:, p:]
        top = theta.T @ np.vstack([Wr[a:b, :], C])
        Wr[a:b, :b] = np.tril(top[:p, :b], a)   # (on and below the diagonal: the rest is structurally zero)
        C = top[p:, :]
    return Lr, Wr


def remove_high(Lo, W, idx, ym, sl, thetas=None):
    """High-noise sample: (L', W', alpha') after the rows ``idx`` (sorted) have left, in sweeps of at most 64."""
    idx = np.asarray(idx, dtype=int)
    for j0 in range(0, idx.size, SWEEP):
        Lo, W = sweep_high(Lo, W, idx[j0:j0 + SWEEP] - j0, thetas)
    r = np.reshape(ym, (-1, 1))
    return Lo, W, W.T @ (W @ r) / sl


def remove_low(A, alpha, idx):
    """Low-noise sample (A = -(K + Sigma)^-1): (A', alpha', ok); ok False (Q_II not positive definite in one of the
    sweeps) returns the inputs of the failing sweep."""
    idx = np.asarray(idx, dtype=int)
    alpha = np.reshape(alpha, (-1, 1))
    for j0 in range(0, idx.size, SWEEP):
        I = idx[j0:j0 + SWEEP] - j0
        keep = np.setdiff1d(np.arange(A.shape[0]), I)
        try:
            Lq = np.linalg.cholesky(-A[np.ix_(I, I)])
        except np.linalg.LinAlgError:
            return A, alpha, False
        Wq = sla.solve_triangular(Lq, np.eye(I.size), lower=True, check_finite=False)
        V = A[np.ix_(keep, I)]
        H = V @ Wq.T
        alpha = alpha[keep] + V @ (Wq.T @ (Wq @ alpha[I]))
        A = A[np.ix_(keep, keep)] + H @ H.T
    return A, alpha, True
