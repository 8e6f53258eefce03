"""Host parts of GP.predict_grad (no GPU): the gradient of the mixture over hyperparameter samples and the mean
functions' gradients with respect to the query inputs, against central differences of _mix_samples and of the mean
functions' values."""

import numpy as np
import pytest


def test_mixture_gradient_matches_differences_of_mix_samples():
    from gpyreg_amd.gaussian_process import _mix_sample_grads, _mix_samples

    rng = np.random.default_rng(0)
    M, D, S = 5, 3, 4
    A, B = rng.standard_normal((M, S, D)), rng.standard_normal((M, S, D))
    x0 = rng.standard_normal((M, D))

    def moments(x):  # per-sample means and variances as smooth functions of the row's inputs
        mu = np.sin(np.einsum("msd,md->ms", A, x))
        var = np.exp(np.einsum("msd,md->ms", B, x))
        return mu, var

    mu, var = moments(x0)
    dmu = np.einsum("ms,msd->mds", np.cos(np.einsum("msd,md->ms", A, x0)), A)
    dvar = np.einsum("ms,msd->mds", var, B)
    gm, gv = _mix_sample_grads(mu, dmu, dvar)
    h = 1e-6
    for l in range(D):
        e = np.zeros((M, D))
        e[:, l] = h
        mp, vp, _ = _mix_samples(*moments(x0 + e))
        mm, vm, _ = _mix_samples(*moments(x0 - e))
        assert np.allclose(gm[:, l], (mp - mm)[:, 0] / (2 * h), rtol=1e-7, atol=1e-9)
        assert np.allclose(gv[:, l], (vp - vm)[:, 0] / (2 * h), rtol=1e-7, atol=1e-9)


def test_mixture_of_one_sample_is_the_sample():
    from gpyreg_amd.gaussian_process import _mix_sample_grads

    rng = np.random.default_rng(1)
    dmu, dvar = rng.standard_normal((4, 2, 1)), rng.standard_normal((4, 2, 1))
    gm, gv = _mix_sample_grads(rng.standard_normal((4, 1)), dmu, dvar)
    assert np.array_equal(gm, dmu[:, :, 0]) and np.array_equal(gv, dvar[:, :, 0])


def test_mean_gradients_match_differences_of_values():
    from gpyreg_amd import mean_functions as mf
    from gpyreg_amd.gaussian_process import _mean_grad_x

    rng = np.random.default_rng(2)
    D = 3
    X = rng.uniform(-2, 2, (6, D))
    hyp = np.concatenate([[0.7], rng.standard_normal(D), 0.3 * rng.standard_normal(D)])
    nq = mf.NegativeQuadratic()
    g = _mean_grad_x(nq, hyp, X)
    h = 1e-6
    for l in range(D):
        e = np.zeros(D)
        e[l] = h
        fd = (nq.values(hyp[None], X + e) - nq.values(hyp[None], X - e))[0] / (2 * h)
        assert np.allclose(g[:, l], fd, rtol=1e-7, atol=1e-9)
    assert np.array_equal(_mean_grad_x(mf.ZeroMean(), np.zeros(0), X), np.zeros(X.shape))
    assert np.array_equal(_mean_grad_x(mf.ConstantMean(), np.array([1.5]), X), np.zeros(X.shape))


def test_user_mean_has_no_gradient():
    from gpyreg_amd import mean_functions as mf
    from gpyreg_amd.gaussian_process import _mean_grad_x

    class Shifted(mf.ConstantMean):
        pass

    with pytest.raises(NotImplementedError, match="Shifted"):
        _mean_grad_x(Shifted(), np.array([0.0]), np.zeros((2, 2)))
