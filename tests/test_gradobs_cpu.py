"""Gradient observations on the CPU: the NumPy restatement (gpyreg_amd._gradobs) that the device is tested against.

The closed forms against torch autograd of the scalar kernels written out here, the structure of the joint matrix
(symmetry to the bit, positive semi-definiteness, the cross operand as a column of it), the conditioning identity against
the already-tested gradient posterior (_gradpost), the soundness of the per-entry bounds the device is held to
(tests/gradobs_ref.py), and the row order."""

import numpy as np
import pytest

import gradobs_ref as gr
import test_cov_functors_cpu as cf
from gpyreg_amd import _gradobs as go
from gpyreg_amd import _gradpost as gp

# (kernel id, degree, rq alpha): SE, SE iso, Matern 3 / 5 (ARD and iso), RQ at alpha = 0.7 and 150
KERNELS = [(0, 0, None), (3, 0, None), (1, 3, None), (1, 5, None), (4, 3, None), (4, 5, None), (2, 0, 0.7),
           (2, 0, 150.0)]
# the shapes of the device's pipeline test (tests/test_gpu_gradobs.py)
PIPELINE_SHAPES = [(70, 37, 3), (130, 65, 2), (20, 64, 1), (50, 9, 33), (1, 1, 2)]


def _hyp(kind, D, alpha, rng):
    if kind in (3, 4):
        return np.array([0.1, 0.2])
    h = np.r_[0.3 * rng.standard_normal(D), 0.2]
    return np.r_[h, np.log(alpha)] if kind == 2 else h


def _torch_kernel(kind, degree, hyp, D):
    import torch

    hyp = torch.tensor(hyp, dtype=torch.float64)
    iso = kind in (3, 4)
    ell = torch.exp(hyp[0]).expand(D) if iso else torch.exp(hyp[:D])
    sf2 = torch.exp(2 * hyp[1 if iso else D])

    def k(x, z):
        d = (x - z) / ell
        r2 = (d * d).sum()
        if kind in (0, 3):
            return sf2 * torch.exp(-r2 / 2)
        if kind in (1, 4):
            t = torch.sqrt(degree * r2)
            return sf2 * ((1 + t) if degree == 3 else (1 + t + t * t / 3)) * torch.exp(-t)
        a = torch.exp(hyp[D + 1])
        return sf2 * (1 + r2 / (2 * a)) ** (-a)

    return k


@pytest.mark.parametrize("kind,degree,alpha", KERNELS)
def test_joint_cov_against_autograd(kind, degree, alpha):
    """First derivatives for the value / gradient entries and the mixed second derivative for the gradient / gradient
    entries at distinct points, against torch fp64 autograd of the kernel written out above; the coincident-point
    blocks against c_a^2 F0 delta_ab and 0.  Bound: 1e-13 max|entry| -- 200 x the 5e-16 measured when the formulas were
    fixed; autograd and the closed form share no code, 5e-16 is a few ulp of the largest entry, so the factor leaves
    room for round-off to accumulate in either chain and none for a wrong sign or factor (an error of order 1)."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(3)
    N, Ng, D = 5, 6, 3
    X, Xg = rng.standard_normal((N, D)), rng.standard_normal((Ng, D))
    Xg[0] = X[1]  # a gradient point ON a value point
    Xg[5] = Xg[2]  # a duplicated gradient point
    hyp = _hyp(kind, D, alpha, rng)
    K = go.joint_cov(kind, degree, hyp, X, Xg)
    tol = 1e-13 * np.abs(K).max()
    idx = go.order(N, Ng, D)
    k = _torch_kernel(kind, degree, hyp, D)
    c, sf2, rqa = gp.scaling(kind, degree, hyp, D)
    F0 = gp.f0(kind, degree, sf2, rqa)
    t = lambda v, g=False: torch.tensor(v, dtype=torch.float64, requires_grad=g)
    for p in range(N):
        for q in range(N):
            assert abs(K[p, q] - float(k(t(X[p]), t(X[q])))) <= tol
    for p in range(Ng):
        for q in range(N):
            if np.array_equal(Xg[p], X[q]):
                assert np.all(K[idx[p], q] == 0) and np.all(K[q, idx[p]] == 0)
                continue
            x = t(Xg[p], True)
            g, = torch.autograd.grad(k(x, t(X[q])), x)
            assert np.abs(K[idx[p], q] - g.numpy()).max() <= tol, (p, q)
            assert np.abs(K[q, idx[p]] - g.numpy()).max() <= tol, (p, q)
        for q in range(Ng):
            blk = K[np.ix_(idx[p], idx[q])]
            if np.array_equal(Xg[p], Xg[q]):
                assert np.abs(blk - np.diag(c * c * F0)).max() <= tol and np.all(blk[~np.eye(D, dtype=bool)] == 0)
                continue
            x, z = t(Xg[p], True), t(Xg[q], True)
            g, = torch.autograd.grad(k(x, z), x, create_graph=True)
            H = torch.stack([torch.autograd.grad(g[a], z, retain_graph=True)[0] for a in range(D)]).numpy()
            assert np.abs(blk - H).max() <= tol, (p, q)


def _pipeline_points(N, Ng, D, seed=0):
    rng = np.random.default_rng(100 * N + Ng + D + seed)
    X, Xg = rng.uniform(-2, 2, (N, D)), rng.uniform(-2, 2, (Ng, D))
    if (N, Ng, D) == (70, 37, 3):
        Xg[:18] = X[:18]  # half of X_g repeats rows of X
    return X, Xg


@pytest.mark.parametrize("N,Ng,D", PIPELINE_SHAPES)
def test_joint_cov_structure(N, Ng, D):
    """Symmetric to the bit; smallest eigenvalue >= -1e-12 x the largest (it was >= -5e-15 with largest eigenvalues of
    order n when the formulas were fixed); the cross operand at a training point, or at a gradient point that repeats
    one, is that point's value column of the joint matrix, to the bit."""
    X, Xg = _pipeline_points(N, Ng, D)
    rng = np.random.default_rng(1)
    for kind, degree, alpha in KERNELS:
        hyp = _hyp(kind, D, alpha, rng)
        K = go.joint_cov(kind, degree, hyp, X, Xg)
        assert K.shape == (N + Ng * D,) * 2 and np.array_equal(K, K.T), (kind, degree)
        w = np.linalg.eigvalsh(K)
        assert w[0] >= -1e-12 * w[-1], (kind, degree, w[0], w[-1])
        cols = [0, N - 1, N // 2]
        B = go.joint_cross(kind, degree, hyp, X, Xg, X[cols])
        assert np.array_equal(B, K[:, cols]), (kind, degree)
        if (N, Ng, D) == (70, 37, 3):
            assert np.array_equal(go.joint_cross(kind, degree, hyp, X, Xg, Xg[[3, 17]]), K[:, [3, 17]])


@pytest.mark.parametrize("s2_val,s2_grad", [(0.01, 0.01), (1e-8, 0.0)])
@pytest.mark.parametrize("kind,degree,alpha", [(0, 0, None), (1, 5, None), (1, 3, None), (2, 0, 0.7)])
def test_conditioning_identity_against_gradient_posterior(kind, degree, alpha, s2_val, s2_grad):
    """Ng = 1, query x* = x_g: conditioning the value-only posterior's joint Gaussian (m, C) of (f, grad f) at x_g
    (_gradpost.joint) on the observed gradient gives m_f + C_fg (C_gg + s2_grad I)^-1 (dy - m_g) and the matching
    variance; _gradobs.posterior + predict must equal it to 1e-10 relative (both sides are fp64 dense solves at
    cond ~ 1e3: round-off ~ 1e-13, margin 1e3).  High-noise and low-noise (L = -inv) branches."""
    import scipy.linalg as sla

    rng = np.random.default_rng(5)
    N, D = 30, 3
    X = rng.uniform(-2, 2, (N, D))
    y = np.sin(X.sum(1))
    xg = rng.uniform(-1, 1, (1, D))
    dy = rng.standard_normal((1, D))
    hyp = _hyp(kind, D, alpha, rng)
    if s2_val < 1e-6:  # (low noise: keep K + Sigma well conditioned without the noise's help)
        hyp[:D] -= 1.0
    # the value-only posterior, by the same rules
    Kvv = go.joint_cov(kind, degree, hyp, X, xg)[:N, :N]
    lch = s2_val >= 1e-6
    if lch:
        L = sla.cholesky(Kvv / s2_val + np.eye(N))
        alpha_v = sla.cho_solve((L, False), y) / s2_val
        sW = np.full((N, 1), 1 / np.sqrt(s2_val))
    else:
        L = -np.linalg.inv(Kvv + s2_val * np.eye(N))
        alpha_v = -L @ y
        sW = None
    mean, cov = gp.joint(kind, degree, hyp, X, xg, alpha_v, sW, L, lch)
    m, C = mean[0], cov[0]
    S = C[1:, 1:] + s2_grad * np.eye(D)
    want_mu = m[0] + C[0, 1:] @ np.linalg.solve(S, dy[0] - m[1:])
    want_s2 = C[0, 0] - C[0, 1:] @ np.linalg.solve(S, C[1:, 0])
    sn2 = np.r_[np.full(N, s2_val), np.full(D, s2_grad)]
    post = go.posterior(kind, degree, hyp, X, xg, go.to_joint(y, dy), np.zeros(N + D), sn2)
    assert post["L_chol"] == (min(s2_val, s2_grad) >= 1e-6) and post["sn2_mult"] == 1
    mu, s2 = go.predict(kind, degree, hyp, X, xg, xg, post)
    assert abs(mu[0] - want_mu) <= 1e-10 * max(abs(want_mu), np.abs(y).max()), (mu[0], want_mu)
    assert abs(s2[0] - want_s2) <= 1e-10 * C[0, 0], (s2[0], want_s2)


@pytest.mark.parametrize("shift", cf.SHIFTS)
@pytest.mark.parametrize("N,Ng,D", [(70, 37, 1), (70, 37, 3), (129, 65, 3), (20, 64, 33)])
def test_numpy_evaluation_stays_inside_half_the_device_bounds(N, Ng, D, shift):
    """NumPy's fp64 evaluation of the three entry kinds (joint_cov_scaled, joint_cross_scaled on the device's scaled
    coordinates) against the extended-precision reference on the functor tests' ladder and shifts: below HALF the
    per-entry bounds the device is held to (the convention of test_cov_functors_cpu)."""
    for name, alpha in gr.FAMILIES:
        case = gr.setup(name, alpha, N, Ng, D, shift, M=9)
        with np.errstate(under="ignore"):
            K = go.joint_cov_scaled(case["kind"], case["degree"], case["xs"], case["xsg"], case["c"], case["sf2"], case["rqa"])
            B = go.joint_cross_scaled(case["kind"], case["degree"], case["xs"], case["xsg"], case["xss"], case["c"],
                                      case["sf2"], case["rqa"])
        want, bound = gr.joint_cov_ld(case)
        r = gr.worst(K, want, bound)
        wantb, boundb = gr.joint_cross_ld(case)
        rb = gr.worst(B, wantb, boundb)
        assert r <= 0.5 and rb <= 0.5, (name, alpha, r, rb)


def test_row_order_round_trips():
    rng = np.random.default_rng(0)
    for N, Ng, D in [(1, 1, 1), (5, 6, 3), (0, 4, 2), (7, 1, 33)]:
        idx = go.order(N, Ng, D)
        assert idx.shape == (Ng, D) and sorted(idx.ravel()) == list(range(N, N + Ng * D))
        assert all(idx[g, l] == N + l * Ng + g for g in range(Ng) for l in range(D))
        y, dy = rng.standard_normal(N), rng.standard_normal((Ng, D))
        j = go.to_joint(y, dy)
        y2, dy2 = go.from_joint(j, N, Ng, D)
        assert np.array_equal(y, y2) and np.array_equal(dy, dy2)
        assert np.array_equal(j[N:].reshape(D, Ng).T, dy)  # dimension-major
