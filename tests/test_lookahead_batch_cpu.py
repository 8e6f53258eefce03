"""GP.lookahead_batch without a device: the NumPy restatement of the greedy recurrence (gpyreg_amd/_lookahead_batch.py)
against a naive loop that re-fits the oracle's posteriors with every chosen candidate appended; the prior path of a GP
without data; the refusals that come before any device work; the symbol's binding.  test_gpu_lookahead_batch.py compares
the device against the same restatement."""

import numpy as np
import pytest

from test_lookahead_cpu import _counts, _prior_gp, _problem, lookahead_numpy, predict_cov_numpy


def restated_inputs(model, posts, X, xr, xc, weights=None, y_cand=None, s2_cand=None):
    """(C0 (S, Mr + Mc, Mc), v0 (Mc, S), noise (Mc, S), w (Mr, S)) of greedy_batch from posterior records."""
    from oracle import gp_oracle as orc

    cov_N, noise_N, _ = _counts(model, X.shape[1])
    S, Mr, Mc = len(posts), xr.shape[0], xc.shape[0]
    C0, v0 = predict_cov_numpy(model, posts, X, np.vstack([xr, xc]), xc)
    noise = np.empty((Mc, S))
    for s, p in enumerate(posts):
        sn2 = orc.noise(model["noise"], p.hyp[cov_N:cov_N + noise_N], xc, y_cand, s2_cand)
        noise[:, s:s + 1] = sn2 * (1 if p.sn2_mult is None else p.sn2_mult)
    w = np.full(Mr, 1.0 / Mr) if weights is None else np.asarray(weights, float)
    w = w if w.ndim == 2 else np.repeat(w[:, None], S, axis=1)
    return C0.transpose(2, 0, 1), v0, noise, w


@pytest.mark.parametrize("kernel", ["se", "matern"])
def test_restatement_against_a_naive_refit(kernel):
    """N = 60, Mr = 20, Mc = 15, q = 4: at every step the oracle's posteriors are recomputed with the candidates chosen
    so far appended (target 0.7: the variance does not depend on it) and the step's scores are lookahead_numpy's on that
    fit.  Same selection, gains within 1e-10 of gain[0]."""
    from oracle import gp_oracle as orc

    from gpyreg_amd._lookahead_batch import greedy_batch

    model, X, y, hyp = _problem(kernel, N=60)
    rng = np.random.default_rng(5)
    xr, xc = rng.uniform(-2.5, 2.5, (20, 3)), rng.uniform(-2.5, 2.5, (15, 3))
    posts = orc.posteriors(model, hyp, X, y, None)
    idx, gain = greedy_batch(*restated_inputs(model, posts, X, xr, xc), 4)
    assert idx.shape == (4,) and gain.shape == (4, hyp.shape[0]) and len(set(idx.tolist())) == 4
    Xt, yt, chosen = X, y, []
    for t in range(4):
        pt = orc.posteriors(model, hyp, Xt, yt, None)
        assert [p.sn2_mult for p in pt] == [p.sn2_mult for p in posts]
        rho = lookahead_numpy(model, pt, Xt, xc, xr)
        score = rho.mean(1)
        score[chosen] = -np.inf
        c = int(np.argmax(score))
        err = np.abs(rho[c] - gain[t]).max() / np.abs(gain[0]).max()
        print(kernel, "step", t, "naive choice", c, "restated", idx[t], "gain error / gain[0]", err)
        assert c == idx[t]
        assert err <= 1e-10
        chosen.append(c)
        Xt, yt = np.vstack([Xt, xc[c:c + 1]]), np.vstack([yt, [[0.7]]])


def test_replay_and_scores_of_the_restatement():
    """``replay`` conditions on a given sequence; the scores of a step are -inf exactly at the candidates chosen
    before it, and a replay of the greedy sequence is the greedy run."""
    from gpyreg_amd._lookahead_batch import greedy_batch

    rng = np.random.default_rng(0)
    S, Mr, Mc = 2, 6, 5
    A = rng.standard_normal((S, Mr + Mc, Mr + Mc + 3))
    K = A @ A.transpose(0, 2, 1)
    C0, v0 = K[:, :, Mr:], np.stack([np.diag(K[s])[Mr:] for s in range(S)], 1)
    noise, w = np.full((Mc, S), 0.1), rng.uniform(0, 1, (Mr, S))
    idx, gain, scores = greedy_batch(C0, v0, noise, w, Mc, return_scores=True)
    assert sorted(idx.tolist()) == list(range(Mc))
    for t in range(Mc):
        assert np.array_equal(np.isneginf(scores[t]), np.isin(np.arange(Mc), idx[:t]))
        assert scores[t, idx[t]] == scores[t].max() and np.isclose(scores[t, idx[t]], gain[t].mean(), rtol=1e-14)
    i2, g2 = greedy_batch(C0, v0, noise, w, Mc, replay=idx)
    assert np.array_equal(i2, idx) and np.array_equal(g2, gain)
    with pytest.raises(ValueError, match="twice"):
        greedy_batch(C0, v0, noise, w, 2, replay=[1, 1])
    with pytest.raises(ValueError, match="q must be"):
        greedy_batch(C0, v0, noise, w, Mc + 1)


def test_gp_without_data_runs_the_recurrence_on_the_prior():
    from gpyreg_amd._lookahead_batch import greedy_batch

    gp, hyp = _prior_gp()
    D, S = 2, 3
    rng = np.random.default_rng(1)
    xr, xc = rng.uniform(-2, 2, (7, D)), rng.uniform(-2, 2, (5, D))
    C0 = np.stack([gp.covariance.compute(hyp[s, :D + 1], np.vstack([xr, xc]), xc) for s in range(S)])
    v0 = np.stack([gp.covariance.compute(hyp[s, :D + 1], xc, compute_diag=True)[:, 0] for s in range(S)], 1)
    noise = np.repeat(np.exp(2 * hyp[:, D + 1])[None, :], 5, axis=0)
    for w in (None, rng.uniform(0, 1, 7), rng.uniform(0, 1, (7, S))):
        w2 = np.full((7, S), 1 / 7) if w is None else (w if w.ndim == 2 else np.repeat(w[:, None], S, 1))
        ref_idx, ref_gain = greedy_batch(C0, v0, noise, w2, 3)
        idx, gain = gp.lookahead_batch(xc, xr, 3, weights=w, separate_samples=True)
        assert idx.shape == (3,) and gain.shape == (3, S)
        assert np.array_equal(idx, ref_idx) and np.array_equal(gain, ref_gain)
        i1, g1 = gp.lookahead_batch(xc, xr, 3, weights=w)
        assert np.array_equal(i1, idx) and g1.shape == (3, 1) and np.allclose(g1[:, 0], gain.mean(1), rtol=1e-14, atol=0)
        # step 0 is lookahead_variance
        R = gp.lookahead_variance(xc, xr, weights=w, separate_samples=True)
        assert idx[0] == np.argmax(R.mean(1)) and np.allclose(gain[0], R[idx[0]], rtol=1e-13, atol=0)
    # q = Mc: every candidate once
    idx, _ = gp.lookahead_batch(xc, xr, 5)
    assert sorted(idx.tolist()) == list(range(5))


def test_refusals():
    import gpyreg_amd as gpr

    gp, hyp = _prior_gp()
    xr, xc = np.zeros((5, 2)), np.arange(6.0).reshape(3, 2)
    for q in (0, 4, -1, 1.5, True):
        with pytest.raises(ValueError, match="q must be"):
            gp.lookahead_batch(xc, xr, q)
    for bad in (np.ones(4), np.ones((5, 2)), np.ones((3,)), np.ones((5, 3, 1)), np.ones((3, 5))):
        with pytest.raises(ValueError, match="lookahead_batch: weights must be"):
            gp.lookahead_batch(xc, xr, 2, weights=bad)
    for bad in (np.nan, np.inf, -np.inf):
        w = np.ones(5)
        w[2] = bad
        with pytest.raises(ValueError, match="finite"):
            gp.lookahead_batch(xc, xr, 2, weights=w)
    with pytest.raises(AssertionError, match="input dimension"):
        gp.lookahead_batch(xc, np.zeros((5, 3)), 2)

    class MyKernel(gpr.covariance_functions.SquaredExponential):
        _gpc_kernel_id = None  # a kernel of the caller's own: its compute is not a device kernel

    user = gpr.GP(2, MyKernel(), gpr.mean_functions.ZeroMean(), gpr.noise_functions.GaussianNoise(constant_add=True))
    user.update(hyp=np.zeros((1, 4)))
    with pytest.raises(NotImplementedError, match="MyKernel"):
        user.lookahead_batch(xc, xr, 2)


def test_the_symbol_is_bound():
    from gpyreg_amd import _lib

    assert "gpc_lookahead_batch" in _lib.SIGNATURES and hasattr(_lib.PostHandle, "lookahead_batch")
