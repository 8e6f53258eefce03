"""GP.quad_grad / gpc_quad_grad: gradients of Bayesian quadrature with respect to the measures' means and widths,
against the NumPy restatement of test_quad_grad_cpu.py on the GP's own fetched posteriors, against central differences
of the GP's own quad, and against quad and predict / predict_grad themselves; bitwise invariance over batches, measure
subsets, chunking and sharding."""

import os
import socket
import sys

import numpy as np
import pytest

from conftest import parse_core_name
from test_quad_grad_cpu import _counts, quad_grad_numpy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gp(model, D, dtype="f64"):
    from test_gpu_api import _gp as make

    return make(model, D, dtype)


def _problem(kernel="se", mean="const", N=200, D=3, S=3, seed=1, dtype="f64", s2=False, quirks=False, lo=-2.0, hi=2.0,
             sn2s=None, shift=0.0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(lo, hi, (N, D))
    y = np.sin(X.sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1))
    model = dict(kernel=kernel, degree=0, mean=mean, noise=(1, 1 if s2 else 0, 0))
    cov_N, noise_N, mean_N = _counts(model, D)
    S = S if sn2s is None else len(sn2s)
    hyp = np.zeros((S, cov_N + noise_N + mean_N))
    hyp[:, :cov_N - 1] = np.log(1.2)
    hyp[:, cov_N] = np.log(0.1)
    if mean != "zero":
        hyp[:, cov_N + noise_N] = 0.3
    if mean == "negquad":
        hyp[:, cov_N + noise_N + 1 + D:] = np.log(3.0)
    hyp += 0.05 * rng.standard_normal(hyp.shape)
    if sn2s is not None:
        hyp[:, cov_N] = 0.5 * np.log(sn2s)
    s2v = 0.01 * (1 + rng.uniform(0, 1, (N, 1))) if s2 else None
    gp = _gp(model, D, dtype)
    gp.reference_quirks = quirks
    gp.update(X_new=X + shift, y_new=y, s2_new=s2v, hyp=hyp)
    if sn2s is not None:
        assert [p.L_chol for p in gp.posteriors] == [v >= 1e-6 for v in sn2s]
    return gp, model, X + shift, hyp


def _measures(D, M=20, seed=2, shift=0.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-2.5, 2.5, (M, D)) + shift, rng.uniform(0.2, 1.5, (M, D))


def _close(a, b, rtol):
    return np.abs(a - b).max() <= rtol * max(np.abs(b).max(), 1e-300)


def _parity(gp, model, X, mu, sigma, rtol):
    """Every gradient plane of every sample against the restatement on the GP's fetched posteriors."""
    F, V, *g = gp.quad_grad(mu, sigma, compute_var=True, separate_samples=True)
    ref = quad_grad_numpy(model, list(gp.posteriors), X, mu, sigma)
    for k in range(4):
        for s in range(g[k].shape[2]):
            assert _close(g[k][:, :, s], ref[k][:, :, s], rtol), (k, s, np.abs(g[k][:, :, s] - ref[k][:, :, s]).max())
    return g


def test_analytic_parity_golden_and_fresh_models():
    g = np.load(os.path.join(ROOT, "tests", "golden", "full_cases.npz"), allow_pickle=False)
    done = 0
    for name in g["names"]:
        tag, model, N, D, _ = parse_core_name(str(name) + "|plain")
        if tag + "_qm" not in g.files:
            continue
        X, y, hyp = g[tag + "_X"], g[tag + "_y"], g[tag + "_hyp"]
        s2 = g[tag + "_s2"] if tag + "_s2" in g.files else None
        gp = _gp(model, D)
        gp.update(X_new=X, y_new=y, s2_new=s2, hyp=hyp)
        _parity(gp, model, X, g[tag + "_qm"], np.broadcast_to(g[tag + "_qs"], g[tag + "_qm"].shape), 1e-8)
        done += 1
    assert done >= 3
    for kernel, mean in (("se", "const"), ("se_iso", "negquad"), ("se", "zero")):
        gp, model, X, hyp = _problem(kernel, mean)
        _parity(gp, model, X, *_measures(X.shape[1]), 1e-8)


def _central(f, x, l, h):
    e = np.zeros_like(x)
    e[:, l] = h
    return [(a - b) / (2 * h) for a, b in zip(f(x + e), f(x - e))]


@pytest.mark.parametrize("kernel,mean,s2,quirks", [("se", "negquad", False, False), ("se_iso", "const", False, False),
                                                   ("se", "zero", True, True), ("se_iso", "negquad", True, False)])
def test_central_differences_of_quad(kernel, mean, s2, quirks):
    """The whole host assembly end to end (mean terms, self-term, quirks scale, mixture) against central differences of
    gp.quad.  Step h = 1e-5: the stencil's truncation error h^2 f''' / 6 is ~1e-11 of the scale here and its rounding
    error ~eps |f| / h ~1e-11; 1e-6 of each plane's largest entry bounds both with room and catches any wrong term."""
    gp, model, X, hyp = _problem(kernel, mean, s2=s2, quirks=quirks)
    mu, sigma = _measures(X.shape[1], M=12)
    h = 1e-5
    for sep in (True, False):
        F, V, dF_mu, dF_sg, dV_mu, dV_sg = gp.quad_grad(mu, sigma, compute_var=True, separate_samples=sep)
        F1, g_mu, g_sg = gp.quad_grad(mu, sigma, separate_samples=sep)
        assert np.array_equal(F1, F)
        assert _close(g_mu, dF_mu, 1e-13) and _close(g_sg, dF_sg, 1e-13)
        for l in range(X.shape[1]):
            fm, vm = _central(lambda m: gp.quad(m, sigma, compute_var=True, separate_samples=sep), mu, l, h)
            fs, vs = _central(lambda s: gp.quad(mu, s, compute_var=True, separate_samples=sep), sigma, l, h)
            for got, fd in ((dF_mu, fm), (dF_sg, fs), (dV_mu, vm), (dV_sg, vs)):
                assert _close(got[:, l], fd if sep else fd[:, 0], 1e-6), (sep, l)


@pytest.mark.parametrize("N,M,S", [(200, 20, 3), (1000, 1000, 2)])
def test_values_match_quad(N, M, S):
    """F is quad's to the bit, F_var to 1e-12 (at N = M = 1000 quad takes the column-square epilogue, quad_grad writes
    V: another order of the sums), and quad returns the same bits after a quad_grad call."""
    gp, model, X, hyp = _problem("se", "negquad", N=N, S=S)
    mu, sigma = _measures(X.shape[1], M=M)
    for sep in (True, False):
        F0, V0 = gp.quad(mu, sigma, compute_var=True, separate_samples=sep)
        F, V, *_ = gp.quad_grad(mu, sigma, compute_var=True, separate_samples=sep)
        F1, *_ = gp.quad_grad(mu, sigma, separate_samples=sep)
        assert np.array_equal(F, F0) and np.array_equal(F1, F0)
        assert F.shape == F0.shape and V.shape == V0.shape
        assert np.abs(V - V0).max() <= 1e-12 * np.abs(V0).max()
        F2, V2 = gp.quad(mu, sigma, compute_var=True, separate_samples=sep)
        assert np.array_equal(F2, F0) and np.array_equal(V2, V0)


@pytest.mark.parametrize("dtype,rtol", [("f64", 1e-8), ("f32", 1e-3)])
@pytest.mark.parametrize("sn2s", [(1e-7, 1e-8), (1e-2, 1e-7, 1e-7, 1e-2, 1e-7, 1e-2)])
def test_low_noise_and_mixed_batches(sn2s, dtype, rtol):
    """L_chol = 0 samples (q = -(L z) from the product quad forms) alone and interleaved with L_chol = 1 samples
    (several launches at nonzero sample offsets), on well-spread inputs (cond(K + Sigma) ~1e2): parity with the
    restatement, and each sample bitwise equal to its own single-sample GP."""
    gp, model, X, hyp = _problem("se", "const", N=40, lo=-3, hi=3, sn2s=sn2s, dtype=dtype, seed=11)
    mu, sigma = _measures(X.shape[1], M=30)
    g = _parity(gp, model, X, mu, sigma, rtol)
    for s in range(len(sn2s)):
        one = _gp(model, X.shape[1], dtype)
        one.update(X_new=X, y_new=gp.y, hyp=hyp[s:s + 1])
        _, _, *g1 = one.quad_grad(mu, sigma, compute_var=True, separate_samples=True)
        for k in range(4):
            assert np.array_equal(g1[k][:, :, 0], g[k][:, :, s]), (s, k)


def test_offset_measures_far_from_the_origin():
    """Training inputs and measures shifted by 1e5 in every dimension: the per-pair differences keep full accuracy
    (a moment expansion would lose eps * 1e10 against the 1e-8 bound); against the unshifted problem only loosely,
    since the factorization builds K from the rounded shifted inputs."""
    shift = 1e5
    gp, model, X, hyp = _problem("se", "const", shift=shift)
    mu, sigma = _measures(X.shape[1], shift=shift)
    g = _parity(gp, model, X, mu, sigma, 1e-8)
    gp0, _, _, _ = _problem("se", "const")
    mu0, _ = _measures(X.shape[1])
    _, _, *g0 = gp0.quad_grad(mu0, sigma, compute_var=True, separate_samples=True)
    for k in range(4):
        assert _close(g[k], g0[k], 1e-5), k


def test_point_measures_are_predict():
    """sigma = 0: z_j = k(X, mu_j), so F is predict's mean (ConstantMean), the sigma gradients are exactly 0 and the mu
    gradients are predict_grad's."""
    gp, model, X, hyp = _problem("se", "const")
    mu, _ = _measures(X.shape[1])
    sigma = np.zeros_like(mu)
    F, V, dF_mu, dF_sg, dV_mu, dV_sg = gp.quad_grad(mu, sigma, compute_var=True, separate_samples=True)
    assert np.all(dF_sg == 0) and np.all(dV_sg == 0)
    m, v, dm, dv = gp.predict_grad(mu, separate_samples=True)
    assert np.abs(F - m).max() <= 1e-10 * np.abs(m).max()
    assert _close(dF_mu, dm, 1e-8) and _close(dV_mu, dv, 1e-8)


def test_clamp_zeroes_the_variance_gradient(monkeypatch):
    """Where quad's clamp F_var = max(eps, .) holds the variance (nf_kk - zkz <= eps) the variance gradient is 0, per
    sample and in the mixture; elsewhere it is the device's.  The device's zkz is raised on chosen rows."""
    gp, model, X, hyp = _problem("se", "const")
    mu, sigma = _measures(X.shape[1])
    h = gp._post_handle
    real = h.quad_grad
    ref = gp.quad_grad(mu, sigma, compute_var=True, separate_samples=True)

    def shifted(m, s, cv):
        out = list(real(m, s, cv))
        out[1] = out[1].copy()
        out[1][0:5, 0] += 10.0
        out[1][6:9, :] += 10.0
        return tuple(out)

    monkeypatch.setattr(h, "quad_grad", shifted)
    F, V, dF_mu, dF_sg, dV_mu, dV_sg = gp.quad_grad(mu, sigma, compute_var=True, separate_samples=True)
    held = np.zeros((mu.shape[0], 3), bool)
    held[0:5, 0] = True
    held[6:9, :] = True
    assert np.all(V[held] == np.spacing(1))
    for got, r in ((dV_mu, ref[4]), (dV_sg, ref[5])):
        assert np.all(got.transpose(0, 2, 1)[held] == 0)
        assert np.array_equal(got.transpose(0, 2, 1)[~held], r.transpose(0, 2, 1)[~held])
    from gpyreg_amd.gaussian_process import _mix_sample_grads

    _, _, mF_mu, mF_sg, mV_mu, mV_sg = gp.quad_grad(mu, sigma, compute_var=True)
    for mf, mv, d, dv in ((mF_mu, mV_mu, dF_mu, dV_mu), (mF_sg, mV_sg, dF_sg, dV_sg)):
        ef, ev = _mix_sample_grads(F, d, dv)
        assert np.array_equal(mf, ef) and np.array_equal(mv, ev)


def test_batch_single_subsets_chunks_bitwise(monkeypatch):
    gp, model, X, hyp = _problem("se", "const", N=300, D=4, S=16, seed=4)
    mu, sigma = _measures(4, M=300, seed=5)
    whole = gp.quad_grad(mu, sigma, compute_var=True, separate_samples=True)
    again = gp.quad_grad(mu, sigma, compute_var=True, separate_samples=True)
    assert all(np.array_equal(a, b) for a, b in zip(whole, again))
    for s in (0, 7, 15):
        one = _gp(model, 4)
        one.update(X_new=X, y_new=gp.y, hyp=hyp[s:s + 1])
        r = one.quad_grad(mu, sigma, compute_var=True, separate_samples=True)
        assert all(np.array_equal(a[..., 0], b[..., s]) for a, b in zip(r[2:], whole[2:])), s
        r = one.quad_grad(mu, sigma, separate_samples=True)
        assert all(np.array_equal(a[..., 0], b[..., s]) for a, b in zip(r[1:], whole[2:4])), s
    for lo, hi in ((0, 70), (130, 300)):  # other measure counts: other padded widths and tile counts
        r = gp.quad_grad(mu[lo:hi], sigma[lo:hi], compute_var=True, separate_samples=True)
        assert all(np.array_equal(a, b[lo:hi]) for a, b in zip(r, whole)), (lo, hi)
    # a budget that holds a few samples of the scratch per chunk (~4 MB each at npad = mpad = 384): several chunks,
    # non-resident constants; mixed L_chol kinds so that runs split at chunk borders
    gp, model, X, hyp = _problem("se", "const", N=300, D=4, lo=-3, hi=3, sn2s=(1e-2, 1e-7) * 5, seed=6)
    from gpyreg_amd import _lib
    from scratch_sizes import planned_chunk, rhs_per, rhs_shared

    whole = [gp.quad_grad(mu, sigma, compute_var=cv, separate_samples=True) for cv in (True, False)]
    monkeypatch.setenv("GPC_MEM_BUDGET_MB", "16")
    chunked, chunks = [], []
    for cv in (True, False):
        chunked.append(gp.quad_grad(mu, sigma, compute_var=cv, separate_samples=True))
        chunks.append(_lib.context(gp.device).get_option("last_chunk"))
    monkeypatch.delenv("GPC_MEM_BUDGET_MB")
    for w, c in zip(whole, chunked):
        assert all(np.array_equal(a, b) for a, b in zip(w, c))
    # ... in the chunks that the scratch's closed form gives (without the variance there is no Q and no product)
    want = [planned_chunk(10, 16, rhs_per(384, 384, False, 8, 4, "quad", cv, grad=True, qg=True),
                          rhs_shared(300, 300, 4, 10, "quad", qg=True)) for cv in (True, False)]
    assert chunks == want and want[0] < 10, (chunks, want)


def test_refusals():
    import gpyreg_amd as gpr

    rng = np.random.default_rng(0)
    X = rng.uniform(-1, 1, (40, 2))
    y = np.sin(X[:, :1])
    noise = gpr.noise_functions.GaussianNoise(constant_add=True)
    for cov, hyp in ((gpr.covariance_functions.Matern(5), [0.0, 0.0, 0.0, np.log(0.1), 0.0]),
                     (gpr.covariance_functions.RationalQuadraticARD(), [0.0, 0.0, 0.0, 0.0, np.log(0.1), 0.0])):
        gp = gpr.GP(2, cov, gpr.mean_functions.ConstantMean(), noise)
        gp.update(X_new=X, y_new=y, hyp=np.array([hyp]))
        with pytest.raises(ValueError) as e:
            gp.quad(X[:3], 1.0)
        with pytest.raises(ValueError, match=str(e.value)):
            gp.quad_grad(X[:3], 1.0)
    gp = gpr.GP(2, gpr.isotropic_covariance_functions.SquaredExponentialIsotropic(), gpr.mean_functions.ConstantMean(),
                noise, reference_quirks=True)
    gp.update(X_new=X, y_new=y, hyp=np.array([[0.0, 0.0, np.log(0.1), 0.0]]))
    with pytest.raises(NotImplementedError, match="reference_quirks"):
        gp.quad_grad(X[:3], 1.0)
    gp.reference_quirks = False
    assert len(gp.quad_grad(X[:3], 1.0)) == 3
    gp.clean()
    with pytest.raises(ValueError, match="posteriors have been cleaned"):
        gp.quad_grad(X[:3], 1.0)


# ---- sharding: the pattern of test_gpu_predict_grad.py::test_sharded_predict_grad_equals_unsharded_bitwise_two_ranks_one_gpu


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

    import gpyreg_amd as gpr

    import bench

    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    try:
        bench.CONFIGS[3] = dict(bench.CONFIGS[3], N=700)
        for S in (1, 5, 16):
            X, y, hyp = bench.synthetic_problem(3, S)
            mu, sigma = X[:40] + 0.05, 0.3 * np.ones((40, X.shape[1]))

            def make():
                return gpr.GP(X.shape[1], gpr.covariance_functions.SquaredExponential(),
                              gpr.mean_functions.ConstantMean(), gpr.noise_functions.GaussianNoise(constant_add=True))

            ref = make()
            ref.shard = False
            ref.update(X_new=X, y_new=y, hyp=hyp)
            gp = make()
            gp.update(X_new=X, y_new=y, hyp=hyp)
            ok = {}
            for kw in (dict(separate_samples=True), dict(), dict(compute_var=True),
                       dict(compute_var=True, separate_samples=True)):
                a = ref.quad_grad(mu, sigma, **kw)
                b = gp.quad_grad(mu, sigma, **kw)
                ok[str(kw)] = all(np.array_equal(u, v) for u, v in zip(a, b))
            out[S] = ok
    except Exception as e:  # noqa: BLE001 - reported to the parent
        out["exception"] = repr(e)
    finally:
        dist.destroy_process_group()
    q.put((rank, out))


def test_sharded_quad_grad_equals_unsharded_bitwise_two_ranks_one_gpu():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for rank in (0, 1):
        r = res[rank]
        assert "exception" not in r, r.get("exception")
        for S in (1, 5, 16):
            assert all(r[S].values()), (rank, S, r[S])
