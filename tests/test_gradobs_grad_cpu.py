"""The NumPy model of the hyperparameter gradient of the gradient-observation likelihood (gpyreg_amd._gradobs:
radial_h, radial_alpha, joint_cov_dhyp, trace_contract, nll_grad, the joint rows of dm and dsn2), without a device:
every formula against central differences of the functions it differentiates."""

import numpy as np
import pytest

from gpyreg_amd import _gradobs as go
from gpyreg_amd import mean_functions as mf
from gpyreg_amd.gaussian_process import _mean_grad_x

LD = np.longdouble
# (kernel id, Matern degree): all five families, both Matern degrees that have a mean-square derivative
KINDS = [(0, 0), (1, 3), (1, 5), (2, 0), (3, 0), (4, 3), (4, 5)]
MEANS = {"zero": mf.ZeroMean, "const": mf.ConstantMean, "negquad": mf.NegativeQuadratic}


def _central(f, x, h):
    """(f(x + h) - f(x - h)) / (2 h) with the difference and the quotient in longdouble."""
    return (np.asarray(f(x + h), dtype=LD) - np.asarray(f(x - h), dtype=LD)) / (2 * LD(h))


@pytest.mark.parametrize("kind,degree", KINDS)
def test_radial_factors_against_central_differences(kind, degree):
    """H = -2 dG/d(r2) against the central difference of radial_g, and (Ka, Fa, Ga) against those of (k, F, G) in
    log alpha.  Step 1e-4 r2 (1e-4 in log alpha): truncation ~ 1e-8 relative, rounding 2^-52 / 1e-4 ~ 2e-12; bound 1e-6
    of the value.  At r2 = 0 the Matern kernels' H is infinite -- the caller drops the term, _pairs_h returns 0."""
    sf2, rqa = 1.7, 0.9
    r2 = np.array([1e-3, 0.04, 0.5, 1.0, 3.0, 9.0, 40.0])
    H = go.radial_h(kind, degree, r2, sf2, rqa)
    fd = -2 * np.array([_central(lambda v: go.radial_g(kind, degree, v, sf2, rqa), r, 1e-4 * r) for r in r2])
    assert np.all(np.abs(H - fd) <= 1e-6 * np.abs(H)), (H, fd)
    h0 = go.radial_h(kind, degree, 0.0, sf2, rqa)
    assert np.isinf(h0) if kind in (1, 4) else np.isfinite(h0)
    A = np.zeros((2, 2))
    d, r2z, k, F, G, Hz, al = go._pairs_h(kind, degree, sf2, rqa, A, A)
    assert np.all(r2z == 0) and np.all(G == 0) and np.all(Hz == 0) and np.all(np.isfinite(F))
    if kind != 2:
        return
    la = np.log(rqa)
    Ka, Fa, Ga = go.radial_alpha(r2, sf2, rqa)
    from gpyreg_amd._gradpost import radial

    for got, f in ((Ka, lambda t: radial(kind, degree, r2, sf2, np.exp(t))[0]),
                   (Fa, lambda t: radial(kind, degree, r2, sf2, np.exp(t))[1]),
                   (Ga, lambda t: go.radial_g(kind, degree, r2, sf2, np.exp(t)))):
        fd = _central(f, la, 1e-4)
        assert np.all(np.abs(got - fd) <= 1e-6 * np.abs(fd).max()), (got, fd)
    assert np.all(np.isfinite(np.array(go.radial_alpha(0.0, sf2, rqa))))


def _points(rng, N, Ng, D, repeat=True):
    X, Xg = rng.uniform(-2, 2, (N, D)), rng.uniform(-2, 2, (Ng, D))
    if repeat:  # rows of X_g repeating rows of X and of X_g: r2 = 0 in every kind of block, off the diagonal too
        Xg[0] = X[1]
        Xg[Ng - 1] = Xg[1]
    return X, Xg


def _hyp_cov(rng, kind, D):
    h = np.log(1.3) + 0.2 * rng.standard_normal(go.cov_count(kind, D))
    return h


@pytest.mark.parametrize("kind,degree", KINDS)
def test_joint_cov_dhyp_against_central_differences(kind, degree):
    """Every plane against the central difference of joint_cov (step 1e-5), within 1e-8 of the plane's largest entry;
    coincident points included; every plane symmetric to the bit."""
    rng = np.random.default_rng(10 * kind + degree)
    N, Ng, D = 6, 5, 3
    X, Xg = _points(rng, N, Ng, D)
    hyp = _hyp_cov(rng, kind, D)
    dK = go.joint_cov_dhyp(kind, degree, hyp, X, Xg)
    n = N + Ng * D
    assert dK.shape == (hyp.size, n, n) and np.all(np.isfinite(dK))
    for p in range(hyp.size):
        e = np.zeros(hyp.size)
        e[p] = 1e-5
        fd = (go.joint_cov(kind, degree, hyp + e, X, Xg) - go.joint_cov(kind, degree, hyp - e, X, Xg)) / 2e-5
        err = np.abs(fd - dK[p]).max() / np.abs(dK[p]).max()
        print(f"kind {kind} degree {degree} plane {p}: {err:.2e}")
        assert err <= 1e-8, (kind, degree, p, err)
        assert np.array_equal(dK[p], dK[p].T)


def _joint_rows(mean_name, N, Ng, D, X, Xg, hyp, counts, s2g):
    """(m, sn2, dm, dsn2) in joint order for ONE hyperparameter vector: stock mean, GaussianNoise(constant_add)."""
    cov_N, noise_N, mean_N = counts
    mean = MEANS[mean_name]()
    hm = hyp[cov_N + noise_N:]
    mX, dmX = mean.values(hm[None, :], X, True)
    m = go.to_joint(mX[0], _mean_grad_x(mean, hm, Xg))
    sn2 = go.to_joint(np.full(N, np.exp(2 * hyp[cov_N])), np.full((Ng, D), s2g))
    dm = go.joint_dm(dmX[0], go.mean_xgrad_dhyp(mean_name, hm, Xg))
    dsn2 = go.joint_dsn2(np.full((1, 1), 2 * np.exp(2 * hyp[cov_N])), N, Ng, D)
    return m, sn2, dm, dsn2


@pytest.mark.parametrize("mean_name", ["zero", "const", "negquad"])
@pytest.mark.parametrize("s2g,lchol", [(0.01, True), (0.0, False)])
@pytest.mark.parametrize("kind,degree", [(0, 0), (1, 5), (2, 0), (4, 3)])
def test_nll_grad_against_central_differences(kind, degree, s2g, lchol, mean_name):
    """nll_grad against central differences of posterior(...)["nlZ"] over covariance, noise and mean hyperparameters,
    on the L_chol branch and on the low-noise branch (s2_grad = 0): 1e-6 max(1, largest entry), the bound of the
    project's other difference checks.  Also: nll_grad is 1/2 sum (Q - alpha alpha^T) o joint_cov_dhyp's planes to
    1e-12 sum |terms| (the contracted form against the planes)."""
    rng = np.random.default_rng(100 * kind + degree + (7 if lchol else 0))
    N, Ng, D = 9, 4, 2
    X, Xg = _points(rng, N, Ng, D, repeat=False)
    y, dy = np.sin(X.sum(1)), 0.5 * np.cos(Xg.sum(1))[:, None] * np.ones((1, D))
    cov_N, noise_N, mean_N = counts = go.cov_count(kind, D), 1, MEANS[mean_name].hyperparameter_count(D)
    hyp = np.concatenate([_hyp_cov(rng, kind, D), [np.log(0.2)], 0.3 * rng.standard_normal(mean_N)])
    target = go.to_joint(y, dy)

    def nlz(h):
        m, sn2, _, _ = _joint_rows(mean_name, N, Ng, D, X, Xg, h, counts, s2g)
        p = go.posterior(kind, degree, h[:cov_N], X, Xg, target, m, sn2)
        assert p["sn2_mult"] == 1.0 and p["L_chol"] == lchol
        return p["nlZ"]

    m, sn2, dm, dsn2 = _joint_rows(mean_name, N, Ng, D, X, Xg, hyp, counts, s2g)
    post = go.posterior(kind, degree, hyp[:cov_N], X, Xg, target, m, sn2)
    g = go.nll_grad(kind, degree, hyp[:cov_N], X, Xg, post, dm, dsn2)
    assert g.shape == hyp.shape
    fd = np.empty(hyp.size)
    for p in range(hyp.size):
        e = np.zeros(hyp.size)
        e[p] = 1e-5
        fd[p] = (nlz(hyp + e) - nlz(hyp - e)) / 2e-5
    err = np.abs(g - fd).max()
    print(f"kind {kind} degree {degree} {mean_name} L_chol {lchol}: {err:.2e} of {np.abs(fd).max():.2e}")
    assert err <= 1e-6 * max(1.0, np.abs(fd).max()), (g, fd)
    Wt = go.weight(post)
    dK = go.joint_cov_dhyp(kind, degree, hyp[:cov_N], X, Xg)
    want = 0.5 * np.einsum("pij,ij->p", dK, Wt)
    scale = 0.5 * np.einsum("pij,ij->p", np.abs(dK), np.abs(Wt))
    assert np.all(np.abs(g[:cov_N] - want) <= 1e-12 * scale), (g[:cov_N], want)


def test_joint_rows_of_dm_and_dsn2():
    """dm: the theta-derivatives of the mean at X and of its x-gradient at X_g (central differences of the stock
    means' values and of _mean_grad_x); dsn2: the noise function's rows on the values, zeros on the gradient rows."""
    rng = np.random.default_rng(3)
    N, Ng, D = 5, 3, 2
    X, Xg = _points(rng, N, Ng, D)
    for name, cls in MEANS.items():
        mean = cls()
        P = cls.hyperparameter_count(D)
        hm = 0.4 * rng.standard_normal(P)
        dm = go.joint_dm(mean.values(hm[None, :], X, True)[1][0], go.mean_xgrad_dhyp(name, hm, Xg))
        assert dm.shape == (N + Ng * D, P)
        joint = lambda h: go.to_joint(mean.values(h[None, :], X)[0], _mean_grad_x(mean, h, Xg))
        for p in range(P):
            e = np.zeros(P)
            e[p] = 1e-6
            fd = (joint(hm + e) - joint(hm - e)) / 2e-6
            assert np.abs(fd - dm[:, p]).max() <= 1e-8 * max(1.0, np.abs(fd).max()), (name, p)
    d = go.joint_dsn2(np.array([[0.3, 0.1]]), N, Ng, D)
    assert d.shape == (N + Ng * D, 2) and np.all(d[:N] == [0.3, 0.1]) and np.all(d[N:] == 0)
    rows = rng.uniform(size=(N, 1))
    d = go.joint_dsn2(rows, N, Ng, D)
    assert np.array_equal(d[:N], rows) and np.all(d[N:] == 0)
    with pytest.raises(ValueError):
        go.mean_xgrad_dhyp("other", np.zeros(1), Xg)


def test_the_partials_are_a_declared_scratch_layout():
    """scratch.h's GobsTraceScratch (the "gobs_trace" layout of gpc_debug_scratch_bytes) against its closed form: one
    row of `pst` doubles per block of the contraction's three grids -- the value / value tiles of the lower triangle,
    the gradient / value tiles, and D per gradient / gradient tile -- and nothing shared.  Host only."""
    import ctypes as C

    from gpyreg_amd import _lib

    lib = _lib.load()
    tiles = lambda v: -(-v // 64)
    for N, Ng, D, pst in ((3, 2, 1, 2), (70, 37, 3, 5), (2000, 200, 10, 12)):
        vt, gt = tiles(N), tiles(Ng)
        rows = vt * (vt + 1) // 2 + vt * gt + gt * gt * D
        dims = (C.c_int * 4)(N, Ng, D, pst)
        per, shared, mis = C.c_ulonglong(), C.c_ulonglong(), C.c_int(-1)
        for dtype in (0, 1):
            assert lib.gpc_debug_scratch_bytes(b"gobs_trace", dtype, dims, 4, C.byref(per), C.byref(shared), C.byref(mis)) == 0
            assert (per.value, shared.value, mis.value) == (rows * pst * 8, 0, 0)
