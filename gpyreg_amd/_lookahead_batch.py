"""The greedy look-ahead batch (``GP.lookahead_batch``), restated in NumPy.

A Gaussian posterior's covariance after conditioning on a new observation does not depend on the observed value, so the
greedy choice of q candidates by the weighted integrated variance is closed.  Per hyperparameter sample s the state is

    C_s  (Mr + Mc, Mc)   the posterior covariance of [x_ref; x_cand] (rows) against x_cand (columns)
    v_s  (Mc,)           the unclamped posterior variance of the candidates (``predict``'s fs2)
    n_s  (Mc,)           the predictive noise of the candidates, sn2_s(x_c) * sn2_mult_s
    w_s  (Mr,)           the weights of the reference points

and step t = 0 .. q-1 is::

    den_s(c)  = max(v_s(c), 0) + n_s(c)
    gain_s(c) = sum_r w_rs C_s(r, c)^2 / den_s(c)            (0 where den_s(c) <= 0)
    score(c)  = (1/S) sum_s gain_s(c)                         (samples added in ascending order; NaN counts as -inf)
    c_t       = argmax over the candidates not yet chosen; ties go to the lowest index
    l_s(a)    = C_s(a, c_t) / sqrt(den_s(c_t))                for every row a; 0 if den_s(c_t) <= 0
    C_s(a, b) -= l_s(a) l_s(Mr + b),    v_s(b) -= l_s(Mr + b)^2

Step 0's gain is ``GP.lookahead_variance(..., separate_samples=True)``.  The module is the model the device
(``gpc_lookahead_batch``) is tested against, and what a GP without data runs on its prior.
"""

import numpy as np


def greedy_batch(C0, v0, noise, w, q, replay=None, return_scores=False):
    """q greedy steps: (idx (q,), gain (q, S)), with ``return_scores`` also scores (q, Mc) -- every step's score, -inf
    at the candidates chosen before it.

    C0 (S, Mr + Mc, Mc), v0 (Mc, S), noise (Mc, S), w (Mr, S).  ``replay``: an index sequence (q,) to condition on
    instead of the argmax (each step's gain and scores are still the recurrence's own)."""
    C = np.array(C0, dtype=float)
    v = np.array(v0, dtype=float)
    noise = np.asarray(noise, dtype=float)
    w = np.asarray(w, dtype=float)
    S, Ma, Mc = C.shape
    Mr = Ma - Mc
    if not 1 <= q <= Mc:
        raise ValueError(f"q must be in [1, {Mc}], got {q}")
    if v.shape != (Mc, S) or noise.shape != (Mc, S) or w.shape != (Mr, S):
        raise ValueError("greedy_batch: C0 (S, Mr + Mc, Mc), v0 (Mc, S), noise (Mc, S), w (Mr, S) expected")
    idx = np.empty(q, dtype=np.int64)
    gain = np.empty((q, S))
    scores = np.empty((q, Mc))
    chosen = np.zeros(Mc, bool)
    for t in range(q):
        den = np.maximum(v, 0) + noise
        g = np.empty((Mc, S))
        for s in range(S):
            wsq = np.sum(w[:, s:s + 1] * C[s, :Mr, :] * C[s, :Mr, :], axis=0)
            g[:, s] = np.where(den[:, s] > 0, wsq / np.where(den[:, s] > 0, den[:, s], 1.0), 0.0)
        score = np.zeros(Mc)
        for s in range(S):
            score = score + g[:, s]
        score = score / S
        score = np.where(np.isnan(score), -np.inf, score)
        masked = np.where(chosen, -np.inf, score)
        scores[t] = masked
        if replay is None:
            free = np.flatnonzero(~chosen)
            c = int(free[np.argmax(score[free])])  # (argmax returns the first maximum: the lowest index)
        else:
            c = int(replay[t])
            if chosen[c]:
                raise ValueError(f"replay chooses candidate {c} twice")
        idx[t] = c
        gain[t] = g[c]
        chosen[c] = True
        for s in range(S):
            if den[c, s] > 0:
                l = C[s, :, c] / np.sqrt(den[c, s])
                C[s] -= np.outer(l, l[Mr:])
                v[:, s] -= l[Mr:] ** 2
    return (idx, gain, scores) if return_scores else (idx, gain)
