"""GP.gradient_posterior / gpc_grad_post: the joint posterior of (f, grad f) at the query points.

The two new kernels entry by entry through their hooks (gpc_debug_block_gram, gpc_debug_cov which = 4), then the
pipeline: parity with the NumPy restatement (gpyreg_amd._gradpost) on the golden core cases, finite differences of the
GP's own predict_full on a stencil, the identities with predict / predict_grad, positive semi-definiteness, low-noise
and mixed batches, fp32, invariance bit for bit (batch, chunking, sharding) and to rounding (query blocks), the budget
failure, the refusals and the prior."""

import os
import socket
import sys

import numpy as np
import pytest

import test_cov_functors_cpu as cf
from conftest import parse_core_name
from test_cov_functors_cpu import F32, F64, LD
from test_gpu_predict_grad import _gp, _lownoise_problem, _problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KID = {"se": 0, "matern": 1, "rq": 2, "se_iso": 3, "matern_iso": 4}


@pytest.fixture(scope="module")
def ctx():
    from gpyreg_amd import _lib

    return _lib.context(0)


# ---- the block Gram kernel, per element ----------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [F64, F32])
def test_block_gram_kernel_per_element(ctx, dtype):
    """Every entry against einsum on the STORED values (fp32: the inputs rounded to fp32 first, so the products are
    exact in fp64) within 8 n u sum_i |y_ia| |z_ib|, u = 2^-53 the unit round-off of the fp64 accumulation.  The kernel
    forms a >= b and mirrors it: [a, b] = [b, a] = sum_i Y[i, a] Z[i, b], symmetric to the bit.  n = 1100 takes the
    two-segment path (gram_segments), Dp = 17 and 33 more than one register tile."""
    u = 2.0 ** -53
    rng = np.random.default_rng(21)
    shapes = [(n, Dp, M) for n in (1, 63, 64, 65, 200) for Dp in (1, 2, 11, 16, 17, 33) for M in (1, 3, 70)]
    shapes += [(1100, 11, 70), (1100, 17, 3)]
    for n, Dp, M in shapes:
        Y = rng.standard_normal((n, Dp, M)) * np.exp(rng.uniform(-3, 3, (1, Dp, 1)))
        Z = rng.standard_normal((n, Dp, M))
        if dtype == F32:
            Y, Z = Y.astype(np.float32).astype(np.float64), Z.astype(np.float32).astype(np.float64)
        low = np.tril(np.ones((Dp, Dp), bool))
        for Zarg, Zv in ((None, Y), (Z, Z)):
            want = np.einsum("iaj,ibj->jab", Y, Zv)
            want = np.where(low, want, np.transpose(want, (0, 2, 1)))
            bound = 8 * n * u * np.einsum("iaj,ibj->jab", np.abs(Y), np.abs(Zv))
            bound = np.where(low, bound, np.transpose(bound, (0, 2, 1)))
            got = ctx.debug_block_gram(Y, Zarg, dtype=dtype)
            assert got.shape == (M, Dp, Dp)
            assert np.all(np.abs(got - want) <= bound), (n, Dp, M, Zarg is None, np.abs(got - want).max())
            assert np.array_equal(got, np.transpose(got, (0, 2, 1))), (n, Dp, M, "not symmetric to the bit")
            gd = ctx.debug_block_gram(Y, Zarg, dtype=dtype, diag_only=True)
            dwant = np.einsum("iaj,iaj->ja", Y, Zv)
            dbound = 8 * n * u * np.einsum("iaj,iaj->ja", np.abs(Y), np.abs(Zv))
            assert gd.shape == (M, Dp) and np.all(np.abs(gd - dwant) <= dbound), (n, Dp, M, "diag")


# ---- the derivative operand kernel, per entry ------------------------------------------------------------------------

OPERAND_FAMILIES = [("se", None), ("se_iso", None), ("matern3", None), ("matern5", None), ("matern_iso3", None),
                    ("matern_iso5", None), ("rq", 0.7), ("rq", 150.0)]


@pytest.mark.parametrize("name,alpha", OPERAND_FAMILIES)
def test_operand_kernel_per_entry(ctx, name, alpha):
    """gpc_debug_cov(which = 4) against the extended-precision functor of test_cov_functors_cpu and against
    gpyreg_amd._gradpost.operand, per entry, on the distance ladder of that file (duplicates, subnormal and huge r2).
    Bound of slot 0: the functor tests' entry bound C eps (1 + a_rq + |arg|) |k| + floor.  Slot 1 + l is
    -c_l F (xs*_l - xs_l): F carries the same relative bound, the difference of two fp64 coordinates, the two products
    and the store round once each (4 eps more), and the absolute floor of F (its underflow: a subnormal F has few bits) is
    multiplied by c_l |d_l| like F itself: (C eps (1 + a_rq + |arg|) + 4 eps) |G| + floor max(c_l, 1) max(|d_l|, 1).
    Against _gradpost (fp64, its own scaling of the inputs): twice that bound plus its coordinate rounding.  Padding is exactly
    0; a query that IS a training point has value sf2 and derivative entries 0 for that pair; the fused column sums
    are the sums of the stored values (64 eps sum |terms|, as the cross kernel's mu)."""
    from gpyreg_amd import _gradpost as gpm

    kind, degree = cf.FAMILIES[name]
    worst = 0.0
    for dtype in (F64, F32):
        for D in (1, 3, 17, 33):
            hyp = cf.make_hyp(kind, D, alpha)
            mul, dv, sf2, rqa = cf.scaling(kind, degree, D, hyp)
            c = mul / dv
            Xall = cf.ladder_inputs(kind, degree, 200, D, hyp, 0.0)
            for N in (1, 65, 200):
                X = Xall[:N]
                xs = cf.scale(X, mul, dv)
                for M in (1, 70):
                    rng = np.random.default_rng(100 * N + M + D)
                    Xq = rng.uniform(-3, 3, (M, D)) * (dv / mul)
                    same = min(7, N - 1)
                    Xq[0] = X[same]  # a query ON a training point (the ladder's 5.0 row when N > 7)
                    al = rng.standard_normal(N)
                    panel, sums, xs_dev = ctx.debug_cov("grad_operand", kind, degree, hyp, X, dtype=dtype, X_star=Xq, vec=al)
                    npad, mpad = panel.shape[0], panel.shape[2]
                    assert panel.shape == (npad, D + 1, mpad) and sums.shape == (D + 1, mpad)
                    assert np.array_equal(xs_dev[:N], xs)
                    assert np.isfinite(panel).all() and np.isfinite(sums).all()
                    assert not panel[N:].any() and not panel[:, :, M:].any() and not sums[:, M:].any(), "padding"
                    xss = cf.scale(Xq, mul, dv)
                    ref = cf.reference(kind, degree, xs, xss, sf2, rqa)
                    rel = cf.rel_bound(kind, ref, rqa, dtype)
                    floor = cf.floor_of(sf2, dtype)
                    pos = (ref["r2"] > 0)
                    with np.errstate(invalid="ignore"):
                        G = np.where(pos[:, :, None], ref["F"][:, :, None] * ref["d"] * c.astype(LD), LD(0))
                    want = np.concatenate([ref["K"][:, None, :], np.transpose(G, (0, 2, 1))], axis=1)
                    bound = np.empty(want.shape)
                    bound[:, 0, :] = rel * np.abs(ref["K"]).astype(np.float64) + floor
                    bound[:, 1:, :] = ((rel + 4 * cf.EPS[dtype])[:, None, :] * np.abs(want[:, 1:, :]).astype(np.float64)
                                       + floor * np.maximum(c, 1.0)[None, :, None]
                                       * np.maximum(np.abs(np.transpose(ref["d"], (0, 2, 1))).astype(np.float64), 1.0))
                    err = np.abs(panel[:N, :, :M].astype(LD) - want).astype(np.float64)
                    worst = max(worst, float((err / bound).max()))
                    assert np.all(err <= bound), (name, alpha, dtype, N, M, D, float((err / bound).max()))
                    assert panel[same, 0, 0] == (np.float32(sf2) if dtype == F32 else sf2)
                    assert not panel[same, 1:, 0].any()
                    if dtype == F64:
                        # _gradpost scales the inputs itself (x c_l, c_l rounded once more than mul and dv): its
                        # coordinates differ from the device's by <= 2 eps |xs|, which moves an entry by at most
                        # |dB/dxs| = c_l |F| (1 + r2) per coordinate (k: |F| sqrt(r2)) -- added to the bound for it
                        B = gpm.operand(kind, degree, hyp, X, Xq)
                        Ff = np.where(pos, np.abs(ref["F"]).astype(np.float64), 0.0)
                        r2f = ref["r2"].astype(np.float64)
                        dx = 8 * cf.EPS[F64] * (np.abs(xs).max() + np.abs(xss).max()) * D
                        coord = np.empty(want.shape)
                        coord[:, 0, :] = dx * Ff * np.sqrt(r2f)
                        coord[:, 1:, :] = dx * (Ff * (1 + r2f))[:, None, :] * c[None, :, None]
                        eb = np.abs(panel[:N, :, :M] - B)
                        assert np.all(eb <= 2 * bound + coord), ("device vs _gradpost", name, N, M, D)
                    terms = panel[:N, :, :M].astype(LD) * al.astype(LD)[:, None, None]
                    sb = 64 * cf.EPS[F64] * np.abs(terms).sum(0).astype(np.float64) + 2.0 ** -1022
                    assert np.all(np.abs(sums[:, :M].astype(LD) - terms.sum(0)).astype(np.float64) <= sb), (name, N, M, D)
    print("operand worst |error| / bound", name, alpha, worst)


# ---- the pipeline ----------------------------------------------------------------------------------------------------


def _restated(model, posts, X, xs):
    """(mean (M, P, S) without the mean function, cov (M, P, P, S)) from the oracle's posteriors."""
    from gpyreg_amd import _gradpost as gpm
    from oracle import gp_oracle as orc

    D = X.shape[1]
    cov_N = orc.cov_count(model["kernel"], D)
    out = [gpm.joint(KID[model["kernel"]], model["degree"], p.hyp[:cov_N], X, xs, p.alpha, p.sW, p.L, p.L_chol)
           for p in posts]
    return np.stack([o[0] for o in out], 2), np.stack([o[1] for o in out], 3)


def _mean_part(model, hyp, xs):
    """The mean function's value and gradient (M, P, S)."""
    from oracle import gp_oracle as orc

    D = xs.shape[1]
    cov_N, noise_N = orc.cov_count(model["kernel"], D), orc.noise_count(model["noise"])
    out = np.zeros((xs.shape[0], D + 1, hyp.shape[0]))
    for s, h in enumerate(hyp):
        hm = h[cov_N + noise_N:]
        out[:, 0, s] = np.reshape(orc.mean(model["mean"], hm, xs), (-1,))
        if model["mean"] == "negquad":
            out[:, 1:, s] = -(xs - hm[1:1 + D]) / np.exp(2 * hm[1 + D:])
    return out


def _solve_sensitivity(posts, B):
    """Per sample: first-order bound on the change of the joint covariance and of the mean under a relative
    perturbation of the solve, cond((K + Sigma)^-1) max_j |B_j|_F^2 |(K + Sigma)^-1|_2 and cond |alpha| max |B_:aj|."""
    sens = np.zeros((2, len(posts)))
    for s, p in enumerate(posts):
        if p.L_chol:
            sW = p.sW[:, 0]
            Kinv = sW[:, None] * np.linalg.inv(p.L.T @ p.L) * sW[None, :]
        else:
            Kinv = -p.L
        cond = np.linalg.cond(Kinv)
        sens[0, s] = cond * np.linalg.norm(Kinv, 2) * np.sum(B[s] ** 2, axis=(0, 1)).max()
        sens[1, s] = cond * np.linalg.norm(p.alpha) * np.sqrt(np.sum(B[s] ** 2, axis=0)).max()
    return sens


@pytest.mark.parametrize("dtype,rtol,u", [("f64", 1e-8, 1e-14), ("f32", 1e-3, 1e-6)])
def test_parity_with_numpy_restatement(core_golden, dtype, rtol, u):
    """Every golden model whose kernel has a mean-square derivative, in the manner of
    test_gpu_predict_grad.test_analytic_parity_with_numpy_formulas: the plain cases to rtol of the largest entry, the
    ill-conditioned flavours to rtol plus u times the solve's sensitivity; a case whose bound exceeds 1 % of the
    largest entry is not compared."""
    from gpyreg_amd import _gradpost as gpm
    from oracle import gp_oracle as orc

    g = core_golden
    done, lchol0, matern1 = 0, 0, 0
    for name in g["names"]:
        tag, model, N, D, flavour = parse_core_name(name)
        if model["kernel"].startswith("matern") and model["degree"] == 1:
            matern1 += 1
            continue
        X, y, hyp = g[tag + "_X"], g[tag + "_y"], g[tag + "_hyp"]
        s2 = g[tag + "_s2"] if tag + "_s2" in g.files else None
        xs = g[tag + "_xs"]
        gp = _gp(model, D, dtype)
        try:
            gp.update(X_new=X, y_new=y, s2_new=s2, hyp=hyp)
        except np.linalg.LinAlgError:
            if dtype == "f32" and flavour != "plain":
                continue
            raise
        mult = [p.sn2_mult for p in gp.posteriors]
        try:
            posts = orc.posteriors(model, hyp, X, y, s2, force_mult=mult)
        except np.linalg.LinAlgError:
            if flavour != "plain":
                continue
            raise
        assert [p.L_chol for p in posts] == [p.L_chol for p in gp.posteriors], name
        rmean, rcov = _restated(model, posts, X, xs)
        cov_N = orc.cov_count(model["kernel"], D)
        Bs = [gpm.operand(KID[model["kernel"]], model["degree"], p.hyp[:cov_N], X, xs) for p in posts]
        sens = _solve_sensitivity(posts, Bs)
        if flavour != "plain":
            if np.any(u * sens[0] > 1e-2 * np.abs(rcov).max()) or np.any(u * sens[1] > 1e-2 * np.abs(rmean).max()):
                continue
        else:
            sens[:] = 0
        rmean = rmean + _mean_part(model, hyp, xs)
        mean, cov = gp.gradient_posterior(xs, with_value=True, separate_samples=True)
        assert mean.shape == rmean.shape and cov.shape == rcov.shape
        for s in range(hyp.shape[0]):
            e_c = np.abs(cov[..., s] - rcov[..., s]).max()
            e_m = np.abs(mean[..., s] - rmean[..., s]).max()
            assert e_c <= rtol * np.abs(rcov[..., s]).max() + u * sens[0, s], (name, s, "cov", e_c)
            assert e_m <= rtol * np.abs(rmean[..., s]).max() + u * sens[1, s], (name, s, "mean", e_m)
        mm, mc = gp.gradient_posterior(xs, with_value=True)
        em, ec = gpm.mix(rmean, rcov)
        assert np.abs(mm - em).max() <= rtol * np.abs(em).max() + u * sens[1].max(), name
        assert np.abs(mc - ec).max() <= rtol * np.abs(ec).max() + u * sens[0].max() \
            + 4 * u * sens[1].max() * np.abs(rmean).max(), name
        done += 1
        lchol0 += not gp.posteriors[0].L_chol
    assert done >= 25 - matern1, (done, matern1)
    assert lchol0 >= (1 if dtype == "f64" else 0), lchol0


@pytest.mark.parametrize("kernel,degree,mean,tol", [("se", 0, "negquad", 1e-4), ("matern", 3, "const", 1e-2),
                                                   ("matern", 5, "const", 1e-4), ("rq", 0, "const", 1e-4),
                                                   ("matern_iso", 5, "negquad", 1e-4)])
def test_finite_differences_of_predict_full(kernel, degree, mean, tol):
    """The joint covariance against T C T^T, C the GP's own predict_full covariance on the stencil (x*, x* +- h_l e_l),
    h = 1e-3 ell (the CPU test's h and tolerances: the stencil is off by 1e-6 ... 7e-6, Matern 3 by 3e-3; the device's
    rounding enters as eps / (4 h^2) ~ 1e-10).  The mean against the same transform of predict_full's mean."""
    gp, model, X, y, hyp = _problem(kernel, degree, mean)
    D = X.shape[1]
    xs = np.random.default_rng(7).uniform(-1.8, 1.8, (12, D))
    mean_j, cov_j = gp.gradient_posterior(xs, with_value=True, separate_samples=True)
    S = hyp.shape[0]
    nl = 1 if kernel.endswith("_iso") else D
    for j in range(xs.shape[0]):
        for s in range(S):
            hs = 1e-3 * np.exp(hyp[s, :nl]) * np.ones(D)
            pts = np.vstack([xs[j:j + 1]] + [xs[j] + sg * hs[l] * np.eye(D)[l] for l in range(D) for sg in (1, -1)])
            T = np.zeros((D + 1, 2 * D + 1))
            T[0, 0] = 1
            for l in range(D):
                T[1 + l, 1 + 2 * l], T[1 + l, 2 + 2 * l] = 0.5 / hs[l], -0.5 / hs[l]
            mu, C = gp.predict_full(pts)
            fd = T @ C[:, :, s] @ T.T
            err = np.abs(cov_j[j, :, :, s] - fd).max() / np.abs(cov_j[j, :, :, s]).max()
            assert err <= tol, (kernel, j, s, err)
            fm = T @ mu[:, s]
            assert np.abs(mean_j[j, :, s] - fm).max() <= tol * max(np.abs(mean_j[j, :, s]).max(), 1.0), (kernel, j, s)


@pytest.mark.parametrize("kernel,degree,mean", [("matern", 5, "negquad"), ("se", 0, "const"), ("rq", 0, "zero")])
def test_identities_against_the_shipped_methods(kernel, degree, mean):
    gp, model, X, y, hyp = _problem(kernel, degree, mean)
    xs = np.random.default_rng(8).uniform(-2, 2, (40, X.shape[1]))
    mean_j, cov_j = gp.gradient_posterior(xs, with_value=True, separate_samples=True)
    mu, s2 = gp.predict(xs, separate_samples=True)
    _, s2g, dmu, ds2 = gp.predict_grad(xs, separate_samples=True)
    assert np.all(s2 > 0)
    assert np.abs(cov_j[:, 0, 0, :] - s2).max() <= 1e-10 * np.abs(s2).max()
    assert np.abs(mean_j[:, 0, :] - mu).max() <= 1e-10 * np.abs(mu).max()
    assert np.abs(cov_j[:, 0, 1:, :] - 0.5 * ds2).max() <= 1e-9 * np.abs(ds2).max()
    assert np.abs(mean_j[:, 1:, :] - dmu).max() <= 1e-10 * np.abs(dmu).max()
    dmean, dvar = gp.gradient_posterior(xs, cov="diag", with_value=True, separate_samples=True)
    assert np.array_equal(dmean, mean_j)
    full_diag = np.einsum("maas->mas", cov_j)
    assert np.abs(dvar - full_diag).max() <= 1e-10 * np.abs(full_diag).max()
    # without the value: the trailing block; the mixtures: the restated mixture of the per-sample results
    from gpyreg_amd import _gradpost as gpm

    g_mean, g_cov = gp.gradient_posterior(xs, separate_samples=True)
    assert np.array_equal(g_mean, mean_j[:, 1:]) and np.array_equal(g_cov, cov_j[:, 1:, 1:])
    mm, mc = gp.gradient_posterior(xs)
    em, ec = gpm.mix(g_mean, g_cov)
    assert mm.shape == (40, X.shape[1]) and mc.shape == (40, X.shape[1], X.shape[1])
    assert np.allclose(mm, em, rtol=1e-13, atol=0) and np.allclose(mc, ec, rtol=1e-13, atol=1e-300)
    dm, dv = gp.gradient_posterior(xs, cov="diag")
    assert np.allclose(dv, np.einsum("maa->ma", ec), rtol=1e-9, atol=0) and np.allclose(dm, em, rtol=1e-13, atol=0)


@pytest.mark.parametrize("kernel,degree", [("se", 0), ("matern", 3), ("matern", 5), ("rq", 0), ("se_iso", 0)])
def test_per_sample_joint_matrices_are_psd(kernel, degree):
    """On the well-conditioned problem the smallest eigenvalue of every per-sample joint matrix is +3e-2 ... +3e-1 of
    its scale in NumPy; asserted: >= -1e-10 times the largest entry.  Symmetric to the bit."""
    gp, model, X, y, hyp = _problem(kernel, degree, "const")
    xs = np.random.default_rng(9).uniform(-2, 2, (60, X.shape[1]))
    _, cov_j = gp.gradient_posterior(xs, with_value=True, separate_samples=True)
    assert np.array_equal(cov_j, np.transpose(cov_j, (0, 2, 1, 3)))
    for s in range(hyp.shape[0]):
        for j in range(xs.shape[0]):
            lam = np.linalg.eigvalsh(cov_j[j, :, :, s])
            assert lam[0] >= -1e-10 * np.abs(cov_j[j, :, :, s]).max(), (j, s, lam[0])


@pytest.mark.parametrize("dtype,rtol", [("f64", 1e-8), ("f32", 1e-3)])
@pytest.mark.parametrize("sn2s", [(1e-7, 1e-8), (1e-2, 1e-7, 1e-7, 1e-2, 1e-7, 1e-2)])
def test_low_noise_and_mixed_batches(sn2s, dtype, rtol):
    """L_chol = 0 samples alone, and interleaved with L_chol = 1 samples (several runs with nonzero sample offsets in
    one call): parity with the restatement, full and diag, and each sample bitwise equal to its own single-sample GP."""
    from oracle import gp_oracle as orc

    gp, model, X, y, hyp = _lownoise_problem(sn2s, dtype=dtype)
    xs = np.random.default_rng(12).uniform(-3, 3, (50, X.shape[1]))
    mean_j, cov_j = gp.gradient_posterior(xs, with_value=True, separate_samples=True)
    _, var_j = gp.gradient_posterior(xs, cov="diag", with_value=True, separate_samples=True)
    posts = orc.posteriors(model, hyp, X, y, None)
    rmean, rcov = _restated(model, posts, X, xs)
    rmean = rmean + _mean_part(model, hyp, xs)
    assert np.array_equal(cov_j, np.transpose(cov_j, (0, 2, 1, 3)))
    for s in range(len(sn2s)):
        assert np.abs(cov_j[..., s] - rcov[..., s]).max() <= rtol * np.abs(rcov[..., s]).max(), s
        assert np.abs(mean_j[..., s] - rmean[..., s]).max() <= rtol * np.abs(rmean[..., s]).max(), s
        rd = np.einsum("maa->ma", rcov[..., s])
        assert np.abs(var_j[..., s] - rd).max() <= rtol * np.abs(rd).max(), s
    for s in range(len(sn2s)):
        one = _gp(model, X.shape[1], dtype)
        one.update(X_new=X, y_new=y, hyp=hyp[s:s + 1])
        m1, c1 = one.gradient_posterior(xs, with_value=True, separate_samples=True)
        _, v1 = one.gradient_posterior(xs, cov="diag", with_value=True, separate_samples=True)
        assert np.array_equal(m1[..., 0], mean_j[..., s]) and np.array_equal(c1[..., 0], cov_j[..., s]), s
        assert np.array_equal(v1[..., 0], var_j[..., s]), s


def test_sample_alone_in_a_batch_and_chunked_bitwise(monkeypatch):
    """A sample's results are the same bits alone, in a batch of 3, and under a memory budget that forces one sample
    per chunk (non-resident constants, runs cut at the chunk borders); full and diag."""
    gp, model, X, y, hyp = _lownoise_problem((1e-2, 1e-7, 1e-2), N=100, D=3)
    xs = np.random.default_rng(14).uniform(-3, 3, (70, 3))
    whole = gp.gradient_posterior(xs, with_value=True, separate_samples=True)
    whole_d = gp.gradient_posterior(xs, cov="diag", with_value=True, separate_samples=True)
    for s in range(3):
        one = _gp(model, 3)
        one.update(X_new=X, y_new=y, hyp=hyp[s:s + 1])
        m1, c1 = one.gradient_posterior(xs, with_value=True, separate_samples=True)
        assert np.array_equal(m1[..., 0], whole[0][..., s]) and np.array_equal(c1[..., 0], whole[1][..., s]), s
    # scratch of one sample at npad = 128, D = 3: two 128 x 512 panels of doubles = 1 MB and small vectors; 80 % of
    # 2 MB holds one sample, not two
    from gpyreg_amd import _lib
    from scratch_sizes import grad_post_per, planned_chunk

    monkeypatch.setenv("GPC_MEM_BUDGET_MB", "2")
    chunked = gp.gradient_posterior(xs, with_value=True, separate_samples=True)
    chunks = [_lib.context(gp.device).get_option("last_chunk")]
    chunked_d = gp.gradient_posterior(xs, cov="diag", with_value=True, separate_samples=True)
    chunks.append(_lib.context(gp.device).get_option("last_chunk"))
    monkeypatch.delenv("GPC_MEM_BUDGET_MB")
    for a, b in zip(whole + whole_d, chunked + chunked_d):
        assert np.array_equal(a, b)
    # ... in the chunks that the scratch's closed form gives (shared: the raw queries)
    want = [planned_chunk(3, 2, grad_post_per(128, 3, diag, 8), 70 * 3 * 8) for diag in (False, True)]
    assert chunks == want == [1, 1], (chunks, want)


def test_budget_failure_names_the_sizes(monkeypatch):
    gp, model, X, y, hyp = _lownoise_problem((1e-2,), N=100, D=3)
    xs = np.zeros((5, 3))
    monkeypatch.setenv("GPC_MEM_BUDGET_MB", "1")  # one sample with one query block needs > 1 MB at npad = 128, D = 3
    with pytest.raises(RuntimeError, match=r"gpc_grad_post: the scratch of one sample with one query block \(\d+ bytes: "
                                           r"N_pad = 128, D = 3, block = 128 queries\) exceeds the device memory budget"):
        gp.gradient_posterior(xs)
    monkeypatch.delenv("GPC_MEM_BUDGET_MB")
    gp.gradient_posterior(xs)  # and the context is usable afterwards


def test_query_alone_or_among_150_to_rounding():
    """150 queries span two query blocks of 128: a query's results alone, in the first and in the second block agree to
    1e-12 relative (the blocks are separate launches of the same forms)."""
    gp, model, X, y, hyp = _problem("matern", 5, "const")
    xs = np.random.default_rng(15).uniform(-2, 2, (150, X.shape[1]))
    mean_j, cov_j = gp.gradient_posterior(xs, with_value=True, separate_samples=True)
    for j in (0, 127, 128, 149):
        m1, c1 = gp.gradient_posterior(xs[j:j + 1], with_value=True, separate_samples=True)
        assert np.abs(m1[0] - mean_j[j]).max() <= 1e-12 * np.abs(mean_j[j]).max(), j
        assert np.abs(c1[0] - cov_j[j]).max() <= 1e-12 * np.abs(cov_j[j]).max(), j


def test_abi_refusals(ctx):
    import gpyreg_amd as gpr
    from gpyreg_amd import _lib

    rng = np.random.default_rng(0)
    X = rng.uniform(-1, 1, (40, 2))
    y = np.sin(X[:, :1])
    hyp = np.array([[0.0, 0.0, 0.0, np.log(0.1), 0.0]])
    noise = gpr.noise_functions.GaussianNoise(constant_add=True)
    lib = _lib.load()

    def raw(gp, xs_ptr, M, fmu, dfmu, cov):
        h = gp._post_handle
        rc = lib.gpc_grad_post(h._h, xs_ptr, M, 0, fmu, dfmu, cov)
        return rc, lib.gpc_last_error(h.ctx._h).decode()

    xs = np.zeros((3, 2))
    fmu, dfmu, cov = np.empty((3, 1)), np.empty((3, 2, 1)), np.empty((3, 3, 3, 1))
    p = _lib._ptr
    gp = gpr.GP(2, gpr.covariance_functions.SquaredExponential(), gpr.mean_functions.ConstantMean(), noise)
    gp.update(X_new=X, y_new=y, hyp=hyp)
    assert raw(gp, p(xs), 0, p(fmu), p(dfmu), p(cov)) == (-2, "gpc_grad_post: bad arguments")
    assert raw(gp, p(xs), -1, p(fmu), p(dfmu), p(cov)) == (-2, "gpc_grad_post: bad arguments")
    for args in ((None, 3, p(fmu), p(dfmu), p(cov)), (p(xs), 3, None, p(dfmu), p(cov)),
                 (p(xs), 3, p(fmu), None, p(cov)), (p(xs), 3, p(fmu), p(dfmu), None)):
        assert raw(gp, *args) == (-2, "gpc_grad_post: bad arguments")
    assert lib.gpc_grad_post(None, p(xs), 3, 0, p(fmu), p(dfmu), p(cov)) == -2
    for cov_obj in (gpr.covariance_functions.Matern(1), gpr.isotropic_covariance_functions.MaternIsotropic(1)):
        g1 = gpr.GP(2, cov_obj, gpr.mean_functions.ConstantMean(), noise)
        g1.update(X_new=X, y_new=y, hyp=hyp[:, :g1.covariance.hyperparameter_count(2) + 2])
        rc, msg = raw(g1, p(xs), 3, p(fmu), p(dfmu), p(cov))
        assert rc == -2 and "Matern kernel of degree 1 has no mean-square derivative" in msg
        with pytest.raises(NotImplementedError, match="degree 1"):
            g1.gradient_posterior(xs)
    # a posterior from caller-provided K
    from test_gpu_user_kernel import PySquaredExponential

    gk = gpr.GP(2, PySquaredExponential(), gpr.mean_functions.ConstantMean(), noise)
    gk.update(X_new=X, y_new=y, hyp=hyp)
    rc, msg = raw(gk, p(xs), 3, p(fmu), p(dfmu), p(cov))
    assert rc == -2 and "caller-provided K" in msg
    with pytest.raises(NotImplementedError, match="PySquaredExponential"):
        gk.gradient_posterior(xs)

    class MyMean(gpr.mean_functions.ConstantMean):
        pass

    gm = gpr.GP(2, gpr.covariance_functions.SquaredExponential(), MyMean(), noise)
    gm.update(X_new=X, y_new=y, hyp=hyp)
    with pytest.raises(NotImplementedError, match="gradient_posterior: .*MyMean"):
        gm.gradient_posterior(xs)
    with pytest.raises(ValueError, match="cov must be"):
        gp.gradient_posterior(xs, cov="lower")


def test_failed_factorization_is_refused(ctx):
    """A device-kernel posterior batch that holds a failed factorization (K - 1e12 I is not positive definite at any
    jitter multiplier: info != 0) is refused."""
    rng = np.random.default_rng(1)
    X = rng.uniform(-1, 1, (40, 2))
    y = np.sin(X[:, :1])
    ctx.set_data(X, y)
    hyp_cov = np.zeros((2, 3))
    handle, mult, lchol, info = ctx.posterior_batch(0, 0, F64, hyp_cov, np.zeros((2, 40)), np.array([[1e-2], [-1e12]]), False)
    try:
        assert info[0] == 0 and info[1] != 0
        with pytest.raises(RuntimeError, match="gpc_grad_post: posterior contains a failed factorization"):
            handle.grad_post(np.zeros((3, 2)))
    finally:
        handle.free()


def test_prior_without_data():
    import gpyreg_amd as gpr
    from gpyreg_amd import _gradpost as gpm

    D = 2
    gp = gpr.GP(D, gpr.covariance_functions.Matern(5), gpr.mean_functions.NegativeQuadratic(),
                gpr.noise_functions.GaussianNoise(constant_add=True))
    hyp = np.array([[0.1, -0.2, 0.3, np.log(0.1), 1.0, 0.3, -0.4, 0.2, 0.5],
                    [0.0, 0.2, 0.1, np.log(0.1), 0.5, 0.1, 0.4, 0.1, 0.3]])
    gp.update(hyp=hyp)
    xs = np.array([[0.5, 1.0], [-1.0, 2.0], [0.0, 0.0]])
    mean_j, cov_j = gp.gradient_posterior(xs, with_value=True, separate_samples=True)
    mu, s2 = gp.predict(xs, separate_samples=True)
    for s in range(2):
        H = gpm.prior_block(1, 5, hyp[s, :3], D)
        assert np.allclose(H[1:], np.exp(2 * hyp[s, 2]) / 3 * (np.sqrt(5) / np.exp(hyp[s, :2])) ** 2, rtol=1e-14)
        for j in range(3):
            assert np.array_equal(cov_j[j, :, :, s], np.diag(H))
        assert np.allclose(mean_j[:, 1:, s], -(xs - hyp[s, 5:7]) / np.exp(2 * hyp[s, 7:9]), rtol=1e-14)
        assert np.array_equal(mean_j[:, 0, s], mu[:, s]) and np.allclose(cov_j[:, 0, 0, s], s2[:, s], rtol=1e-14)
    dm, dv = gp.gradient_posterior(xs, cov="diag")
    assert dm.shape == (3, D) and dv.shape == (3, D)
    em, ec = gpm.mix(mean_j[:, 1:], cov_j[:, 1:, 1:])
    assert np.allclose(dm, em) and np.allclose(dv, np.einsum("maa->ma", ec))


def test_prior_block_against_the_package_covariance_classes():
    """H[1 + l] by the four-point second difference of the package's own covariance classes at coincident points
    (h = 1e-4 ell; 1e-5 of the value, Matern 3: 1e-3 -- the CPU file's check, on the device's generic functor)."""
    import gpyreg_amd as gpr
    from gpyreg_amd import _gradpost as gpm

    cases = [(gpr.covariance_functions.SquaredExponential(), 0), (gpr.covariance_functions.Matern(3), 3),
             (gpr.covariance_functions.Matern(5), 5), (gpr.covariance_functions.RationalQuadraticARD(), 0),
             (gpr.isotropic_covariance_functions.SquaredExponentialIsotropic(), 0),
             (gpr.isotropic_covariance_functions.MaternIsotropic(5), 5)]
    rng = np.random.default_rng(3)
    for cov, degree in cases:
        for D in (1, 3):
            n = cov.hyperparameter_count(D)
            iso = n == 2
            h = np.zeros(n)
            nl = 1 if iso else D
            h[:nl] = np.log(1.2) + 0.1 * rng.standard_normal(nl)
            h[nl] = np.log(1.3)
            ell = np.exp(h[0]) * np.ones(D) if iso else np.exp(h[:D])
            H = gpm.prior_block(cov._gpc_kernel_id, degree, h, D)
            x = rng.uniform(-1, 1, (1, D))
            for l in range(D):
                e = np.zeros((1, D))
                e[0, l] = 1e-4 * ell[l]
                k0 = cov.compute(h, x, x)[0, 0]
                k2 = cov.compute(h, x + e, x - e)[0, 0]
                d2 = (2 * k0 - 2 * k2) / (4 * e[0, l] ** 2)
                assert abs(d2 - H[1 + l]) <= (1e-3 if degree == 3 else 1e-5) * H[1 + l], (type(cov).__name__, D, l)


# ---- sharding: the pattern of test_gpu_predict_grad.py


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      GPYREG_AMD_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist

    import bench

    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    try:
        bench.CONFIGS[3] = dict(bench.CONFIGS[3], N=300)
        for S in (1, 5):
            X, y, hyp = bench.synthetic_problem(3, S)
            xs = X[:20] + 0.05
            ref = bench.make_gp(3, "f64")
            ref.shard = False
            ref.update(X_new=X, y_new=y, hyp=hyp)
            gp = bench.make_gp(3, "f64")
            gp.update(X_new=X, y_new=y, hyp=hyp)
            ok = {}
            for kw in (dict(separate_samples=True, with_value=True), dict(), dict(cov="diag", separate_samples=True)):
                a = ref.gradient_posterior(xs, **kw)
                b = gp.gradient_posterior(xs, **kw)
                ok[str(kw)] = all(np.array_equal(u, v) for u, v in zip(a, b))
            out[S] = ok
    except Exception as e:  # noqa: BLE001 - reported to the parent
        out["exception"] = repr(e)
    finally:
        dist.destroy_process_group()
    q.put((rank, out))


def test_sharded_equals_unsharded_bitwise_two_ranks_one_gpu():
    import torch.multiprocessing as mp

    mctx = mp.get_context("spawn")
    q = mctx.Queue()
    port = _free_port()
    procs = [mctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for rank in (0, 1):
        r = res[rank]
        assert "exception" not in r, r.get("exception")
        for S in (1, 5):
            assert all(r[S].values()), (rank, S, r[S])
