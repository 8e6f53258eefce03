"""The posterior of the gradient under gradient observations on the CPU: the NumPy model the device is tested against
(gpyreg_amd._gradobs.joint_operand / gradient_joint) and the scratch layout of gpc_grad_post_gobs.

The model against brute-force conditioning of the joint covariance extended by the query (every sign and both r2 = 0
rules, independently of the operand's formulas), against central differences of _gradobs.predict (the code the project
had before), and the layout's closed form, including the shape whose point list has more 64-tiles than the panel."""

import ctypes as C

import numpy as np
import pytest

import gradobs_ref as gr
import scratch_sizes as ss
import test_cov_functors_cpu as cf
from gpyreg_amd import _gradobs as go
from gpyreg_amd import _gradpost as gpm

F64, F32 = 0, 1
N, NG, D, M = 12, 5, 3, 4


def _case(name, alpha, seed=0):
    """Points in +-2 (length scales ~0.5: a well-conditioned joint matrix), the family's hyperparameters, M queries of
    which the first lies ON a training row and the second ON a gradient point."""
    kind, degree = cf.FAMILIES[name]
    rng = np.random.default_rng(11 + seed)
    X, Xg = rng.uniform(-2, 2, (N, D)), rng.uniform(-2, 2, (NG, D))
    xq = rng.uniform(-2, 2, (M, D))
    xq[0], xq[1] = X[3], Xg[2]
    y, dy = np.sin(X.sum(1)), np.cos(Xg.sum(1))[:, None] * np.ones((1, D))
    return kind, degree, cf.make_hyp(kind, D, alpha), X, Xg, xq, go.to_joint(y, dy)


@pytest.mark.parametrize("sn2_value,s2_grad", [(1e-2, 1e-2), (1e-8, 0.0)], ids=["lchol", "low-noise"])
@pytest.mark.parametrize("name,alpha", gr.FAMILIES)
def test_model_against_brute_force_conditioning(name, alpha, sn2_value, s2_grad):
    """K' = joint_cov of [X; x*] and [X_g; x*] holds every block among the data values, the data gradients, f(x*) and
    grad f(x*); conditioning it in NumPy on the data rows gives the joint posterior of (f, grad f) at x* without the
    operand's formulas.  Mean and covariance agree with gradient_joint to 1e-10 of the largest entry, on both branches
    of the factorization, also where x* is a training row or a gradient point (the r2 = 0 rules)."""
    kind, degree, hyp, X, Xg, xq, target = _case(name, alpha)
    n = N + NG * D
    sn2 = go.to_joint(np.full(N, sn2_value), np.full((NG, D), s2_grad))
    post = go.posterior(kind, degree, hyp, X, Xg, target, np.zeros(n), sn2)
    assert post["L_chol"] == (s2_grad > 0) and post["sn2_mult"] == 1
    mean, cov = go.gradient_joint(kind, degree, hyp, X, Xg, xq, post)
    assert mean.shape == (M, D + 1) and cov.shape == (M, D + 1, D + 1)
    data = np.r_[np.arange(N), (N + 1 + go.order(0, NG + 1, D)[:NG].T).ravel()]  # dimension-major, as the joint order
    for j in range(M):
        Kp = go.joint_cov(kind, degree, hyp, np.vstack([X, xq[j:j + 1]]), np.vstack([Xg, xq[j:j + 1]]))
        tgt = np.r_[N, N + 1 + go.order(0, NG + 1, D)[NG]]
        A = Kp[np.ix_(data, data)] + post["sn2_mult"] * np.diag(sn2)
        Ktd = Kp[np.ix_(tgt, data)]
        want_mean = Ktd @ np.linalg.solve(A, target)
        want_cov = Kp[np.ix_(tgt, tgt)] - Ktd @ np.linalg.solve(A, Ktd.T)
        em = np.abs(mean[j] - want_mean).max() / np.abs(want_mean).max()
        ec = np.abs(cov[j] - want_cov).max() / np.abs(Kp[np.ix_(tgt, tgt)]).max()
        print(f"{name} {alpha} query {j}: mean {em:.2e} cov {ec:.2e}")
        assert em <= 1e-10 and ec <= 1e-10, (name, alpha, j, em, ec)
    assert np.array_equal(xq[0], X[3]) and np.array_equal(xq[1], Xg[2])


def test_operand_is_made_of_the_siblings():
    """Slot 0 is joint_cross, the value rows are _gradpost.operand, to the bit (the same expressions)."""
    for name, alpha in gr.FAMILIES:
        kind, degree, hyp, X, Xg, xq, _ = _case(name, alpha)
        B = go.joint_operand(kind, degree, hyp, X, Xg, xq)
        assert B.shape == (N + NG * D, D + 1, M)
        assert np.array_equal(B[:, 0], go.joint_cross(kind, degree, hyp, X, Xg, xq)), name
        assert np.array_equal(B[:N], gpm.operand(kind, degree, hyp, X, xq)), name


# measured disagreement between gradient_joint and central differences of _gradobs.predict at h = 1e-3 ell, relative to
# the largest analytic entry, (dmu, ds2) per family: the stencil's own error, h^2 / 6 times a third derivative ~ 1e-6,
# dominates (the model agrees with brute-force conditioning to 1e-15 above).  At these 6 random queries no family stands
# apart; the plain GP's test (tests/test_gpu_gradient_posterior.py) records 1e-6 .. 7e-6, and 3e-3 for Matern 3.
FD_MEASURED = {
    ("se", None): (3.54e-7, 4.27e-7), ("se_iso", None): (2.97e-7, 4.76e-7), ("matern3", None): (2.86e-7, 4.10e-7),
    ("matern5", None): (2.62e-7, 3.78e-7), ("matern_iso3", None): (9.90e-8, 4.27e-7),
    ("matern_iso5", None): (1.32e-7, 2.55e-7), ("rq", 0.7): (3.31e-7, 3.10e-7), ("rq", 150.0): (3.54e-7, 4.25e-7),
}


@pytest.mark.parametrize("name,alpha", gr.FAMILIES)
def test_model_against_central_differences(name, alpha):
    """dmu and ds2 = 2 C[0, 1 + l] of gradient_joint against central differences of _gradobs.predict (the parent's
    code) with h = 1e-3 ell_l, at 6 random queries, value noise 1e-2 and gradient noise 1e-2.  The tolerance is 10 x the
    disagreement measured on the CPU when the model was written (FD_MEASURED: (mean, variance gradient) per family;
    the stencil's own error varies with the draw).  Measured: 1e-7 .. 3.5e-7 for dmu and 2.6e-7 .. 4.8e-7 for ds2, every
    family alike.  Slot 0 equals _gradobs.predict to 1e-12 (the same operand rows, another order of the sums)."""
    kind, degree, hyp, X, Xg, _, target = _case(name, alpha)
    n = N + NG * D
    sn2 = go.to_joint(np.full(N, 1e-2), np.full((NG, D), 1e-2))
    post = go.posterior(kind, degree, hyp, X, Xg, target, np.zeros(n), sn2)
    xq = np.random.default_rng(5).uniform(-2, 2, (6, D))
    mean, cov = go.gradient_joint(kind, degree, hyp, X, Xg, xq, post)
    ell = np.exp(hyp[0]) * np.ones(D) if cf.is_iso(kind) else np.exp(hyp[:D])
    dmu, ds2 = np.empty((6, D)), np.empty((6, D))
    for l in range(D):
        e = np.zeros(D)
        e[l] = 1e-3 * ell[l]
        mp, sp = go.predict(kind, degree, hyp, X, Xg, xq + e, post)
        mm, sm = go.predict(kind, degree, hyp, X, Xg, xq - e, post)
        dmu[:, l], ds2[:, l] = (mp - mm) / (2 * e[l]), (sp - sm) / (2 * e[l])
    em = np.abs(mean[:, 1:] - dmu).max() / np.abs(mean[:, 1:]).max()
    es = np.abs(2 * cov[:, 0, 1:] - ds2).max() / np.abs(2 * cov[:, 0, 1:]).max()
    print(f"FD {name} {alpha}: dmu {em:.2e} ds2 {es:.2e}")
    m0, s0 = go.predict(kind, degree, hyp, X, Xg, xq, post)
    assert np.abs(mean[:, 0] - m0).max() <= 1e-12 * np.abs(m0).max() and np.abs(cov[:, 0, 0] - s0).max() <= 1e-12 * np.abs(s0).max()
    tm, ts = FD_MEASURED[(name, alpha)]
    assert em <= 10 * tm and es <= 10 * ts, (name, alpha, em, es)


# ---- the scratch layout ------------------------------------------------------------------------------------------------


def _measured(lib, name, dtype, *dims):
    arr = (C.c_int * len(dims))(*[int(d) for d in dims])
    per, shared, mis = C.c_ulonglong(), C.c_ulonglong(), C.c_int(-1)
    rc = lib.gpc_debug_scratch_bytes(name.encode(), dtype, arr, len(dims), C.byref(per), C.byref(shared), C.byref(mis))
    assert rc == 0 and mis.value == 0, (name, dims, rc, mis.value)
    return per.value, shared.value


def _grad_post_gobs_per(N_, Ng, D_, diag, w):
    """grad_post's closed form at the joint order, its npad / 64 tile rows of partials replaced by the point list's
    (pad64(N) + pad64(Ng)) / 64."""
    npad = ss.pad(N_ + Ng * D_)
    rows = (ss.pad(N_, 64) + ss.pad(Ng, 64)) // 64
    return ss.grad_post_per(npad, D_, diag, w) + (rows - npad // 64) * (D_ + 1) * 128 * 8


@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
def test_scratch_layout(dtype):
    """The "grad_post_gobs" layout (N, Ng, D, diag) against its closed form -- at (65, 1, 1) the partials have 3 tile rows
    where the panel has 2, and the layout must count 3 -- and "grad_post"'s own counts unchanged from
    tests/scratch_sizes.py at three shapes."""
    from gpyreg_amd import _lib

    lib = _lib.load()
    w = 8 if dtype == F64 else 4
    for N_, Ng, D_ in [(65, 1, 1), (70, 37, 3), (129, 65, 3), (20, 64, 33), (600, 150, 3), (300, 100, 10)]:
        for diag in (0, 1):
            got = _measured(lib, "grad_post_gobs", dtype, N_, Ng, D_, diag)
            assert got == (_grad_post_gobs_per(N_, Ng, D_, bool(diag), w), 0), (N_, Ng, D_, diag, got)
    assert _grad_post_gobs_per(65, 1, 1, False, 8) == ss.grad_post_per(128, 1, False, 8) + 2 * 128 * 8
    for N_, M_, D_ in [(90, 70, 3), (300, 129, 1), (1100, 1, 3)]:
        for diag in (0, 1):
            assert _measured(lib, "grad_post", dtype, N_, M_, D_, diag) == \
                (ss.grad_post_per(ss.pad(N_), D_, bool(diag), w), M_ * D_ * 8), (N_, M_, D_, diag)
