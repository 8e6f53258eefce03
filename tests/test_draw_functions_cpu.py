"""GP.draw_functions without a device: the random stream's NumPy restatement (gpyreg_amd/_philox.py) against
numpy.random.Philox, the Box-Muller formulas, prior draws of a GP without data, and the argument refusals.  The prior
path factors and multiplies on the host; its K** comes from the covariance object, which the tests here back with the
oracle's NumPy covariance (the built-in ``compute`` is a device kernel)."""

import numpy as np
import pytest

from gpyreg_amd import _philox


@pytest.mark.parametrize("seed,stream,s,r,q", [(0, 0, 0, 0, 0), (1, 1, 0, 0, 0), (123, 0, 7, 3, 5), (5, 1, 2**40, 9, 1000),
                                                (2**63, 0, 3, 1, 0), (2**63 + 12345, 1, 15, 63, 17),
                                                (2**64 - 1, 0, 2**62, 2**31, 2**33)])
def test_words_equal_numpy_philox(seed, stream, s, r, q):
    key = np.array([seed, stream], dtype=np.uint64)
    ctr = np.array([q, r, s, 0], dtype=np.uint64)
    ref = np.random.Philox(key=key, counter=ctr).random_raw(4)
    got = _philox.words(seed, stream, s, r, np.arange(4 * q, 4 * q + 4))
    assert np.array_equal(got, ref)


def test_words_vectorised_over_samples_and_draws():
    j = np.arange(10).reshape(-1, 1, 1)
    r = np.arange(3).reshape(1, -1, 1)
    s = np.array([0, 4]).reshape(1, 1, -1)
    w = _philox.words(99, 1, s, r, j)
    for jj, rr, ss in ((0, 0, 0), (9, 2, 1), (5, 1, 1)):
        key = np.array([99, 1], dtype=np.uint64)
        ref = np.random.Philox(key=key, counter=np.array([jj // 4, rr, s.ravel()[ss], 0], dtype=np.uint64)).random_raw(4)
        assert w[jj, rr, ss] == ref[jj % 4]


def test_box_muller_formulas():
    seed, stream, s, r = 2024, 0, 3, 5
    M = 9  # odd: the last row's partner word is computed and not used
    z = _philox.normals(seed, stream, s, r, np.arange(M))
    w = [int(x) for x in _philox.words(seed, stream, s, r, np.arange(M + 1))]
    for t in range((M + 1) // 2):
        u1 = ((w[2 * t] >> 11) + 1) * 2.0**-53
        u2 = (w[2 * t + 1] >> 11) * 2.0**-53
        rad = np.sqrt(-2.0 * np.log(u1))
        assert z[2 * t] == rad * np.cos(2 * np.pi * u2)
        if 2 * t + 1 < M:
            assert z[2 * t + 1] == rad * np.sin(2 * np.pi * u2)


def test_stream_does_not_depend_on_the_block_shape():
    a = _philox.normals_block(7, 0, 11, 4, [2, 5])
    b = _philox.normals_block(7, 0, 30, 9, [5, 0, 2])
    assert np.array_equal(a[:, :, 0], b[:11, :4, 2]) and np.array_equal(a[:, :, 1], b[:11, :4, 0])
    z = _philox.normals_block(0, 0, 20000, 1, [0]).ravel()
    assert abs(z.mean()) < 0.05 and abs(z.std() - 1) < 0.05


def _prior_gp(D=2, S=3):
    import gpyreg_amd as gpr

    gp = gpr.GP(D, gpr.covariance_functions.Matern(5), gpr.mean_functions.NegativeQuadratic(),
                gpr.noise_functions.GaussianNoise(constant_add=True))
    rng = np.random.default_rng(0)
    hyp = np.concatenate([0.2 * rng.standard_normal((S, D)), np.zeros((S, 1)), np.full((S, 1), np.log(0.1)),
                          0.3 * rng.standard_normal((S, 1 + 2 * D))], axis=1)
    gp.update(hyp=hyp)

    def host_compute(h, X, X_star=None, compute_diag=False, compute_grad=False):
        from oracle import gp_oracle as orc

        return orc.covariance("matern", h, X, X_star, compute_diag, degree=5)

    gp.covariance.compute = host_compute
    return gp, hyp


def test_prior_draws_are_m_plus_chol_z():
    gp, hyp = _prior_gp()
    D = 2
    xs = np.random.default_rng(1).uniform(-2, 2, (13, D))
    f, tau = gp.draw_functions(xs, n_draws=5, seed=11, return_jitter=True)
    assert f.shape == (13, 5, 3) and tau.shape == (3,)
    for s in range(3):
        K = gp.covariance.compute(hyp[s, :D + 1], xs)
        L = np.linalg.cholesky(K + tau[s] * np.eye(13))
        m = gp.mean.compute(hyp[s, D + 2:], xs).ravel()
        z = _philox.normals_block(11, 0, 13, 5, [s])[:, :, 0]
        assert np.allclose(f[:, :, s], m[:, None] + L @ z, rtol=1e-13, atol=1e-13)
    noisy = gp.draw_functions(xs, n_draws=5, seed=11, add_noise=True)
    for s in range(3):
        sn = np.sqrt(np.exp(2 * hyp[s, D + 1]))
        zn = _philox.normals_block(11, 1, 13, 5, [s])[:, :, 0]
        assert np.allclose(noisy[:, :, s], f[:, :, s] + sn * zn, rtol=1e-13, atol=1e-13)
    # prefix of rows and draws (host BLAS: the product's order may change with the shape)
    assert np.allclose(gp.draw_functions(xs[:6], n_draws=2, seed=11), f[:6, :2], rtol=1e-13, atol=1e-13)


def test_prior_jitter_ladder_on_duplicated_points():
    gp, hyp = _prior_gp(S=1)
    xs = np.repeat(np.random.default_rng(2).uniform(-1, 1, (4, 2)), 3, axis=0)  # K** singular: rank 4 of 12
    f, tau = gp.draw_functions(xs, n_draws=3, seed=1, return_jitter=True)
    assert np.all(np.isfinite(f)) and tau[0] > 0
    K = gp.covariance.compute(hyp[0, :3], xs)
    t = tau[0] / np.mean(np.diag(K))
    assert any(np.isclose(t, 10.0**e, rtol=1e-12) for e in range(-12, -5))


def test_refusals():
    import gpyreg_amd as gpr

    gp, hyp = _prior_gp()
    xs = np.zeros((3, 2))
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="n_draws"):
            gp.draw_functions(xs, n_draws=bad)
    for bad in (-1, 2**64, 0.5):
        with pytest.raises(ValueError, match="seed"):
            gp.draw_functions(xs, seed=bad)
    gp.draw_functions(xs, seed=2**64 - 1)

    class MyKernel(gpr.covariance_functions.SquaredExponential):
        _gpc_kernel_id = None  # a kernel of the caller's own: its compute is not a device kernel

    user = gpr.GP(2, MyKernel(), gpr.mean_functions.ZeroMean(), gpr.noise_functions.GaussianNoise(constant_add=True))
    user.update(hyp=np.zeros((1, 4)))
    with pytest.raises(NotImplementedError, match="MyKernel"):
        user.draw_functions(xs)
