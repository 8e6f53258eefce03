"""GP.sample_paths without a device: the host model gpyreg_amd/_paths.py -- the spectral draws against the kernels they
stand for, prior paths of a GP without data, the refusals, and the model's analytic gradient against its own central
differences."""

import functools
import pickle

import numpy as np
import pytest

from gpyreg_amd import _paths

KINDS = [(_paths.K_SE, 0), (_paths.K_MATERN, 1), (_paths.K_MATERN, 3), (_paths.K_MATERN, 5), (_paths.K_SE_ISO, 0),
         (_paths.K_MATERN_ISO, 1), (_paths.K_MATERN_ISO, 3), (_paths.K_MATERN_ISO, 5)]
F_SPECTRAL = 200_000


@functools.lru_cache(maxsize=None)
def _theta(matern_degree):
    """theta of F_SPECTRAL features at D = 3 (the draw depends on the family through the Matern degree only)."""
    kind = _paths.K_MATERN if matern_degree else _paths.K_SE
    return _paths.features(kind, matern_degree, 3, F_SPECTRAL, 17, 2)[0]


@pytest.mark.parametrize("kind,degree", KINDS)
def test_spectral_draw_reproduces_the_kernel(kind, degree):
    """mean_f cos(theta_f . delta) = k(delta) / sf2 on scaled inputs.  The summands are bounded by 1, so their mean over
    F features lies within 5 / sqrt(F) of its expectation at 5 sigma."""
    theta = _theta(degree if kind in (_paths.K_MATERN, _paths.K_MATERN_ISO) else 0)
    assert np.array_equal(theta, _paths.features(kind, degree, 3, F_SPECTRAL, 17, 2)[0])
    bound = 5.0 / np.sqrt(F_SPECTRAL)
    for delta in ([0.3, -0.2, 0.5], [1.0, 0.7, -1.2], [0.0, 0.0, 2.5], [0.05, 0.0, 0.0]):
        delta = np.array(delta)
        est = np.mean(np.cos(theta @ delta))
        k = _paths.pair(kind, degree, float(delta @ delta), 1.0)[0]
        assert abs(est - k) <= bound, (kind, degree, delta, est, float(k))


def test_phases_and_streams():
    theta, b = _paths.features(_paths.K_MATERN, 3, 2, 50, 5, 4)
    assert theta.shape == (50, 2) and b.shape == (50,) and np.all((b >= 0) & (b < 2 * np.pi))
    # a feature is its own function of (seed, sample, index): prefixes agree, other samples and seeds do not
    t2, b2 = _paths.features(_paths.K_MATERN, 3, 2, 20, 5, 4)
    assert np.array_equal(t2, theta[:20]) and np.array_equal(b2, b[:20])
    assert not np.array_equal(_paths.features(_paths.K_MATERN, 3, 2, 50, 5, 3)[0], theta)
    assert not np.array_equal(_paths.features(_paths.K_MATERN, 3, 2, 50, 6, 4)[0], theta)
    assert np.array_equal(_paths.weights(50, 7, 5, 4)[:, :3], _paths.weights(50, 3, 5, 4))
    assert np.array_equal(_paths.noise(33, 7, 5, 4)[:, :3], _paths.noise(33, 3, 5, 4))


def _prior_gp(cov=None, D=2, S=3):
    import gpyreg_amd as gpr

    cov = cov or gpr.covariance_functions.Matern(5)
    gp = gpr.GP(D, cov, gpr.mean_functions.NegativeQuadratic(), gpr.noise_functions.GaussianNoise(constant_add=True))
    rng = np.random.default_rng(0)
    cov_N = cov.hyperparameter_count(D)
    hyp = np.concatenate([0.2 * rng.standard_normal((S, cov_N)), np.full((S, 1), np.log(0.1)),
                          0.3 * rng.standard_normal((S, 1 + 2 * D))], axis=1)
    gp.update(hyp=hyp)
    return gp, hyp


def test_prior_paths_of_a_gp_without_data():
    gp, hyp = _prior_gp()
    D = 2
    x = np.random.default_rng(1).uniform(-2, 2, (13, D))
    paths = gp.sample_paths(n_paths=5, n_features=64, seed=11)
    assert (paths.n_paths, paths.n_features, paths.seed) == (5, 64, 11)
    f = paths(x)
    f2, df = paths(x, compute_grad=True)
    assert f.shape == (13, 5, 3) and df.shape == (13, D, 5, 3) and np.array_equal(f, f2)
    for s in range(3):
        theta, b = _paths.features(_paths.K_MATERN, 5, D, 64, 11, s)
        wt = _paths.weights(64, 5, 11, s)
        m = gp.mean.compute(hyp[s, D + 2:], x).ravel()
        ref = _paths.evaluate(_paths.K_MATERN, 5, hyp[s, :D + 1], None, None, theta, b, wt, x)
        assert np.allclose(f[:, :, s], m[:, None] + ref, rtol=1e-13, atol=1e-13)
    # a path is a function: the same rows in another call, and it does not depend on n_paths
    assert np.array_equal(paths(x[3:9]), f[3:9])
    wide = gp.sample_paths(n_paths=9, n_features=64, seed=11)(x)
    assert np.allclose(wide[:, :5], f, rtol=1e-13, atol=1e-13)
    assert not np.allclose(gp.sample_paths(n_paths=5, n_features=64, seed=12)(x), f)
    paths.close()
    with pytest.raises(ValueError, match="closed"):
        paths(x)


def test_refusals():
    import gpyreg_amd as gpr

    gp, _ = _prior_gp()
    for name in ("n_paths", "n_features"):
        for bad in (0, -1, 1.5, True):
            with pytest.raises(ValueError, match=name):
                gp.sample_paths(**{name: bad})
    for bad in (-1, 2**64, 0.5, True):
        with pytest.raises(ValueError, match="seed"):
            gp.sample_paths(seed=bad)
    paths = gp.sample_paths(seed=2**64 - 1, n_features=8)
    with pytest.raises(ValueError, match="x_star"):
        paths(np.zeros((3, 5)))
    with pytest.raises(TypeError, match="cannot be pickled"):
        pickle.dumps(paths)
    import copy

    with pytest.raises(TypeError, match="cannot be pickled or copied"):
        copy.deepcopy(paths)

    rq, _ = _prior_gp(gpr.covariance_functions.RationalQuadraticARD())
    with pytest.raises(NotImplementedError, match="rational-quadratic"):
        rq.sample_paths()

    class MyKernel(gpr.covariance_functions.SquaredExponential):
        _gpc_kernel_id = None  # a kernel of the caller's own

    user = gpr.GP(2, MyKernel(), gpr.mean_functions.ZeroMean(), gpr.noise_functions.GaussianNoise(constant_add=True))
    user.update(hyp=np.zeros((1, 4)))
    with pytest.raises(NotImplementedError, match="MyKernel"):
        user.sample_paths()
    with pytest.raises(NotImplementedError):
        _paths.features(_paths.K_RQ, 0, 2, 4, 0, 0)


@pytest.mark.parametrize("kind,degree", KINDS)
def test_model_gradient_equals_central_differences(kind, degree):
    rng = np.random.default_rng(3)
    N, D, F, R, M = 17, 3, 40, 4, 6
    X = rng.uniform(-1.5, 1.5, (N, D))
    iso = kind in (_paths.K_SE_ISO, _paths.K_MATERN_ISO)
    hyp = np.concatenate([np.log(rng.uniform(0.6, 1.4, 1 if iso else D)), [np.log(1.3)]])
    v = rng.standard_normal((N, R))
    theta, b = _paths.features(kind, degree, D, F, 9, 1)
    # (the step of the differences must resolve the fastest feature: the heavy-tailed Matern-1 draws are clipped)
    theta = np.clip(theta, -6.0, 6.0)
    wt = _paths.weights(F, R, 9, 1)
    # query points off the training points: the Matern-1 kernel has a kink there
    x = rng.uniform(-1.5, 1.5, (M, D))
    assert np.min(np.linalg.norm(x[:, None] - X[None], axis=2)) > 0.05
    f, df = _paths.evaluate(kind, degree, hyp, X, v, theta, b, wt, x, compute_grad=True)
    assert np.array_equal(f, _paths.evaluate(kind, degree, hyp, X, v, theta, b, wt, x))
    h = 1e-5
    scale = np.max(np.abs(df))
    for l in range(D):
        e = np.zeros(D)
        e[l] = h
        num = (_paths.evaluate(kind, degree, hyp, X, v, theta, b, wt, x + e) -
               _paths.evaluate(kind, degree, hyp, X, v, theta, b, wt, x - e)) / (2 * h)
        assert np.max(np.abs(num - df[:, l])) <= 1e-6 * scale, (kind, degree, l)
