"""GP.quad_mixture / GP.quad_cov (gpc_quad_mix, gpc_quad_cov): quadrature against a mixture of Gaussian measures and the
covariance between the single integrals, against the NumPy restatement of test_quad_mixture_cpu.py on the GP's own
fetched posteriors, against quad itself, against central differences of the GP's own quad_mixture; odd shapes; bitwise
invariance over batches, chunking and sharding; no MFMA GEMM launch; the budget message.

V and every variance gradient are differences of a Gamma term and a solve term that nearly cancel (V / w^T Gamma w was
0.017 on the CPU check), so their error is bounded relative to the LARGER of the two terms -- w^T Gamma w for V, the
larger plane maximum for a plane -- never relative to the difference."""

import os
import sys

import numpy as np
import pytest

from conftest import parse_core_name
from test_gpu_quad_grad import _close, _free_port, _gp, _measures, _problem
from test_quad_grad_cpu import _counts, _kernel_scales
from test_quad_mixture_cpu import _weights, gamma_matrix, quad_cov_numpy, quad_mixture_numpy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("E", "V", "dE_dmu", "dE_dsigma", "dE_dw", "dV_dmu", "dV_dsigma", "dV_dw")


def _gemms(gp):
    from gpyreg_amd import _lib

    return _lib.context(gp.device).get_option("quad_mix_gemms")


def _parity(gp, model, X, mu, sigma, w, rtol):
    """quad_mixture and quad_cov of every sample against the restatement on the GP's fetched posteriors."""
    posts = list(gp.posteriors)
    got = dict(zip(KEYS, gp.quad_mixture(mu, sigma, w, compute_var=True, compute_grad=True, separate_samples=True)))
    ref = quad_mixture_numpy(model, posts, X, mu, sigma, w, terms=True)
    assert np.all(ref["V_raw"] > 10 * rtol * ref["V|gamma"])  # (clear of the clamp: device and restatement agree on it)
    for s in range(len(posts)):
        for k in KEYS:
            g, r = got[k][..., s], ref[k][..., s]
            scale = np.abs(r).max()
            if k.startswith("dV") or k == "V":
                scale = max(np.abs(ref[k + "|gamma"][..., s]).max(), np.abs(ref[k + "|solve"][..., s]).max())
            err = np.abs(g - r).max()
            print(f"parity {k} sample {s}: err {err:.3e} scale {scale:.3e} ratio {err / max(scale, 1e-300):.3e}")
            assert err <= rtol * max(scale, 1e-300), (k, s, err, scale)
    F, C = gp.quad_cov(mu, sigma, separate_samples=True)
    F0, C0 = quad_cov_numpy(model, posts, X, mu, sigma)
    cov_N = _counts(model, X.shape[1])[0]
    for s, p in enumerate(posts):
        gmax = np.abs(gamma_matrix(mu, sigma, *_kernel_scales(model, p.hyp[:cov_N], X.shape[1]))[0]).max()
        err = np.abs(C[:, :, s] - C0[:, :, s]).max()
        print(f"parity C sample {s}: err {err:.3e} scale {gmax:.3e}")
        assert err <= rtol * gmax, (s, err, gmax)
        assert np.abs(F[:, s] - F0[:, s]).max() <= rtol * np.abs(F0[:, s]).max()
    return got


def test_parity_golden_and_fresh_models():
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
        mu = g[tag + "_qm"]
        before = _gemms(gp)
        _parity(gp, model, X, mu, np.broadcast_to(g[tag + "_qs"], mu.shape), _weights(mu.shape[0]), 1e-8)
        assert _gemms(gp) == before == 0
        done += 1
    assert done >= 3
    for kernel, mean, s2 in (("se", "const", False), ("se_iso", "negquad", False), ("se", "zero", False),
                             ("se", "negquad", True), ("se_iso", "const", True)):
        gp, model, X, hyp = _problem(kernel, mean, s2=s2)
        mu, sigma = _measures(X.shape[1])
        _parity(gp, model, X, mu, sigma, _weights(mu.shape[0]), 1e-8)
    assert _gemms(gp) == 0


@pytest.mark.parametrize("dtype,rtol", [("f64", 1e-8), ("f32", 1e-3)])
@pytest.mark.parametrize("sn2s", [(1e-7, 1e-8), (1e-2, 1e-7, 1e-7, 1e-2, 1e-7, 1e-2)])
def test_low_noise_and_mixed_batches(sn2s, dtype, rtol):
    """L_chol = 0 samples (q = -(L zbar)) alone and interleaved with L_chol = 1 samples (several launches at nonzero
    sample offsets), on well-spread inputs: parity, and each sample bitwise equal to its own single-sample GP."""
    gp, model, X, hyp = _problem("se", "const", N=40, lo=-3, hi=3, sn2s=sn2s, dtype=dtype, seed=11)
    mu, sigma = _measures(X.shape[1], M=30)
    w = _weights(30)
    got = _parity(gp, model, X, mu, sigma, w, rtol)
    F, C = gp.quad_cov(mu, sigma, separate_samples=True)
    for s in range(len(sn2s)):
        one = _gp(model, X.shape[1], dtype)
        one.update(X_new=X, y_new=gp.y, hyp=hyp[s:s + 1])
        r = one.quad_mixture(mu, sigma, w, compute_var=True, compute_grad=True, separate_samples=True)
        for k, a in zip(KEYS, r):
            assert np.array_equal(a[..., 0], got[k][..., s]), (s, k)
        F1, C1 = one.quad_cov(mu, sigma, separate_samples=True)
        assert np.array_equal(F1[:, 0], F[:, s]) and np.array_equal(C1[:, :, 0], C[:, :, s])


@pytest.mark.parametrize("N,M", [(200, 20), (1000, 300)])
def test_consistency_with_quad(N, M):
    """quad_cov's diagonal is quad's variance, w^T quad_cov w is quad_mixture's V, dE_dw is quad's F.  The variances are
    differences of cancelling terms formed in different orders: bounded at 1e-10 of the Gamma term."""
    gp, model, X, hyp = _problem("se", "negquad", N=N, S=3)
    mu, sigma = _measures(X.shape[1], M=M)
    w = _weights(M)
    ref = quad_mixture_numpy(model, list(gp.posteriors), X, mu, sigma, w, terms=True)
    cov_N = _counts(model, X.shape[1])[0]
    gmax = max(gamma_matrix(mu, sigma, *_kernel_scales(model, p.hyp[:cov_N], X.shape[1]))[0].max() for p in gp.posteriors)
    for sep in (True, False):
        F0, V0 = gp.quad(mu, sigma, compute_var=True, separate_samples=sep)
        F, C = gp.quad_cov(mu, sigma, separate_samples=sep)
        assert F.shape == F0.shape and _close(F, F0, 1e-12)
        diag = np.einsum("jj...->j...", C).reshape(V0.shape)
        print("diag", np.abs(diag - V0).max(), "gamma", gmax)
        assert np.abs(diag - V0).max() <= 1e-10 * gmax
        assert np.array_equal(C, np.swapaxes(C, 0, 1))
    F0 = gp.quad(mu, sigma, separate_samples=True)
    _, C = gp.quad_cov(mu, sigma, separate_samples=True)
    E, V, _, _, dE_dw, *_ = gp.quad_mixture(mu, sigma, w, compute_var=True, compute_grad=True, separate_samples=True)
    assert _close(dE_dw, F0, 1e-12) and _close(E, w @ F0, 1e-12)
    wCw = np.einsum("j,jks,k->s", w, C, w)
    print("V", V, "wCw", wCw, "gamma term", ref["V|gamma"])
    assert np.all(np.abs(V - wCw) <= 1e-10 * ref["V|gamma"])


def _central(f, x, h):
    """Central differences of f: x-shaped array -> tuple of (S,) or scalar values, one entry of x at a time."""
    outs = None
    for idx in np.ndindex(*x.shape):
        e = np.zeros_like(x)
        e[idx] = h
        d = [(np.asarray(a) - np.asarray(b)) / (2 * h) for a, b in zip(f(x + e), f(x - e))]
        if outs is None:
            outs = [np.zeros(x.shape + v.shape) for v in d]
        for o, v in zip(outs, d):
            o[idx] = v
    return outs


@pytest.mark.parametrize("kernel,mean,s2,quirks", [("se", "negquad", False, False), ("se_iso", "const", False, False),
                                                   ("se", "zero", True, True), ("se", "negquad", True, True)])
def test_central_differences_of_quad_mixture(kernel, mean, s2, quirks):
    """The whole assembly end to end (device share, mean terms, quirks scale, mixture) against central differences of
    gp.quad_mixture itself in mu, sigma and w, one entry at a time.  Step h = 1e-5 and 1e-6 of each plane's largest
    entry, as reasoned in test_gpu_quad_grad.py: truncation h^2 f''' / 6 ~1e-11 of the scale; the rounding error of V is
    ~eps w^T Gamma w / h ~1e-11 of the Gamma term, ~1e-9 of V's own gradients here."""
    gp, model, X, hyp = _problem(kernel, mean, s2=s2, quirks=quirks)
    mu, sigma = _measures(X.shape[1], M=5)
    if quirks:
        # the reference's rescaling doubles the solve term here (sl / exp(2 hyp[cov_N]) ~ 2 with the per-point noise):
        # measures spread beyond the data keep that term below w^T Gamma w (restatement: V = 0.10 .. 0.16), so that the
        # clamp does not hold V and its gradients are the ones under test
        mu = 2.0 * mu
    w = _weights(5)
    h = 1e-5
    for sep in (True, False):
        E, V, dE_mu, dE_sg, dE_w, dV_mu, dV_sg, dV_w = gp.quad_mixture(mu, sigma, w, True, True, separate_samples=sep)
        assert np.all(np.asarray(V) > 1e-3)
        f = lambda m, s, v: gp.quad_mixture(m, s, v, compute_var=True, separate_samples=sep)
        fd_mu = _central(lambda m: f(m, sigma, w), mu, h)
        fd_sg = _central(lambda s: f(mu, s, w), sigma, h)
        fd_w = _central(lambda v: f(mu, sigma, v), w, h)
        for name, got, fd in (("dE_dmu", dE_mu, fd_mu[0]), ("dV_dmu", dV_mu, fd_mu[1]), ("dE_dsigma", dE_sg, fd_sg[0]),
                              ("dV_dsigma", dV_sg, fd_sg[1]), ("dE_dw", dE_w, fd_w[0]), ("dV_dw", dV_w, fd_w[1])):
            err, scale = np.abs(got - fd).max(), np.abs(fd).max()
            print(f"central {name} sep={sep}: err {err:.3e} scale {scale:.3e} ")
            assert got.shape == fd.shape and scale > 0 and err <= 1e-6 * scale, (name, sep)


@pytest.mark.parametrize("N,M,D", [(200, 1, 3), (200, 70, 3), (333, 130, 2), (150, 20, 40)])
def test_shapes(N, M, D):
    """M = 1, M not a multiple of 64, N not a multiple of 128, D above the staging chunk of 32; negative weights."""
    gp, model, X, hyp = _problem("se", "const", N=N, D=D, S=2, lo=-1.0 if D > 30 else -2.0, hi=1.0 if D > 30 else 2.0)
    rng = np.random.default_rng(M)
    mu = rng.uniform(-1, 1, (M, D)) if D > 30 else rng.uniform(-2.5, 2.5, (M, D))
    sigma = rng.uniform(0.2, 1.5, (M, D))
    w = rng.uniform(-1.0, 1.0, M)
    before = _gemms(gp)
    _parity(gp, model, X, mu, sigma, w, 1e-8)
    assert _gemms(gp) == before


def test_batch_single_chunks_bitwise_and_budget_message(monkeypatch):
    gp, model, X, hyp = _problem("se", "const", N=300, D=4, S=16, seed=4)
    mu, sigma = _measures(4, M=300, seed=5)
    w = _weights(300)
    kw = dict(compute_var=True, compute_grad=True, separate_samples=True)
    whole = gp.quad_mixture(mu, sigma, w, **kw)
    again = gp.quad_mixture(mu, sigma, w, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(whole, again))
    for s in (0, 7, 15):
        one = _gp(model, 4)
        one.update(X_new=X, y_new=gp.y, hyp=hyp[s:s + 1])
        r = one.quad_mixture(mu, sigma, w, **kw)
        assert all(np.array_equal(a[..., 0], b[..., s]) for a, b in zip(r, whole)), s
        r = one.quad_mixture(mu, sigma, w, compute_grad=True, separate_samples=True)
        assert all(np.array_equal(a[..., 0], b[..., s]) for a, b in zip(r, (whole[0],) + whole[2:5])), s
        r = one.quad_mixture(mu, sigma, w, compute_var=True, separate_samples=True)
        assert all(np.array_equal(a[..., 0], b[..., s]) for a, b in zip(r, whole[:2])), s
    # budgets that hold one and two samples of the scratch (~0.65 MB each at npad = mpad = 384): several chunks; mixed
    # L_chol kinds so that runs split at chunk borders
    gp, model, X, hyp = _problem("se", "const", N=300, D=4, lo=-3, hi=3, sn2s=(1e-2, 1e-7) * 5, seed=6)
    flags = ((True, True), (True, False), (False, True), (False, False))
    whole = [gp.quad_mixture(mu, sigma, w, cv, cg, separate_samples=True) for cv, cg in flags]
    cov = gp.quad_cov(mu, sigma, separate_samples=True)
    from gpyreg_amd import _lib
    from scratch_sizes import planned_chunk, quad_mix_per, quad_mix_shared

    ctx, shared = _lib.context(gp.device), quad_mix_shared(300, 384, 4)
    # (the chunk the library reports is the one that the scratch's closed form gives: with variance and gradient, one
    # sample under 1 MB and two under 2 MB)
    assert [planned_chunk(10, mb, quad_mix_per(384, 384, 4, True, True), shared) for mb in (1, 2)] == [1, 2]
    for mb in ("1", "2"):
        monkeypatch.setenv("GPC_MEM_BUDGET_MB", mb)
        chunked = []
        for cv, cg in flags:
            chunked.append(gp.quad_mixture(mu, sigma, w, cv, cg, separate_samples=True))
            assert ctx.get_option("last_chunk") == planned_chunk(10, int(mb), quad_mix_per(384, 384, 4, cv, cg), shared), (mb, cv, cg)
        monkeypatch.delenv("GPC_MEM_BUDGET_MB")
        for a, b in zip(whole, chunked):
            a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
            assert all(np.array_equal(u, v) for u, v in zip(a, b)), mb
    monkeypatch.setenv("GPC_MEM_BUDGET_MB", "8")
    cov_c = gp.quad_cov(mu, sigma, separate_samples=True)
    monkeypatch.delenv("GPC_MEM_BUDGET_MB")
    assert all(np.array_equal(u, v) for u, v in zip(cov, cov_c))
    assert _gemms(gp) == 0
    # one sample's scratch above the budget: -2 with the sizes in the message
    mu2, sigma2 = _measures(4, M=1000, seed=8)
    monkeypatch.setenv("GPC_MEM_BUDGET_MB", "1")
    with pytest.raises(RuntimeError, match=r"gpc_quad_mix.*rc=-2.*N_pad = 384, M_pad = 1024, D = 4.*budget"):
        gp.quad_mixture(mu2, sigma2, np.ones(1000), compute_var=True, compute_grad=True)
    monkeypatch.delenv("GPC_MEM_BUDGET_MB")
    assert len(gp.quad_mixture(mu2, sigma2, np.ones(1000), compute_var=True, compute_grad=True)) == 8


def test_refusals():
    import gpyreg_amd as gpr

    rng = np.random.default_rng(0)
    X = rng.uniform(-1, 1, (40, 2))
    y = np.sin(X[:, :1])
    noise = gpr.noise_functions.GaussianNoise(constant_add=True)
    gp = gpr.GP(2, gpr.covariance_functions.Matern(5), gpr.mean_functions.ConstantMean(), noise)
    gp.update(X_new=X, y_new=y, hyp=np.array([[0.0, 0.0, 0.0, np.log(0.1), 0.0]]))
    with pytest.raises(ValueError) as e:
        gp.quad(X[:3], 1.0)
    with pytest.raises(ValueError, match=str(e.value)):
        gp.quad_mixture(X[:3], 1.0, np.ones(3))
    with pytest.raises(ValueError, match=str(e.value)):
        gp.quad_cov(X[:3], 1.0)
    with pytest.raises(RuntimeError, match="squared exponential"):  # the library's own refusal
        gp._post_handle.quad_mix(X[:3], np.ones((3, 2)), np.ones(3), True, True)
    with pytest.raises(RuntimeError, match="squared exponential"):
        gp._post_handle.quad_cov(X[:3], np.ones((3, 2)))
    gp = gpr.GP(2, gpr.isotropic_covariance_functions.SquaredExponentialIsotropic(), gpr.mean_functions.ConstantMean(),
                noise, reference_quirks=True)
    gp.update(X_new=X, y_new=y, hyp=np.array([[0.0, 0.0, np.log(0.1), 0.0]]))
    with pytest.raises(NotImplementedError, match="reference_quirks"):
        gp.quad_mixture(X[:3], 1.0, np.ones(3))
    gp.reference_quirks = False
    assert len(gp.quad_mixture(X[:3], 1.0, np.ones(3), compute_grad=True)) == 4
    gp.clean()
    with pytest.raises(ValueError, match="posteriors have been cleaned"):
        gp.quad_mixture(X[:3], 1.0, np.ones(3))
    with pytest.raises(ValueError, match="posteriors have been cleaned"):
        gp.quad_cov(X[:3], 1.0)


# ---- sharding: the pattern of test_gpu_quad_grad.py::test_sharded_quad_grad_equals_unsharded_bitwise_two_ranks_one_gpu


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
            w = np.linspace(-0.5, 1.5, 40)

            def make():
                return gpr.GP(X.shape[1], gpr.covariance_functions.SquaredExponential(),
                              gpr.mean_functions.ConstantMean(), gpr.noise_functions.GaussianNoise(constant_add=True))

            ref = make()
            ref.shard = False
            ref.update(X_new=X, y_new=y, hyp=hyp)
            gp = make()
            gp.update(X_new=X, y_new=y, hyp=hyp)
            ok = {}
            for kw in (dict(separate_samples=True), dict(compute_grad=True), dict(compute_var=True),
                       dict(compute_var=True, compute_grad=True), dict(compute_var=True, compute_grad=True, separate_samples=True)):
                a = ref.quad_mixture(mu, sigma, w, **kw)
                b = gp.quad_mixture(mu, sigma, w, **kw)
                a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
                ok[str(kw)] = all(np.array_equal(u, v) for u, v in zip(a, b))
            for sep in (True, False):
                a = ref.quad_cov(mu, sigma, separate_samples=sep)
                b = gp.quad_cov(mu, sigma, separate_samples=sep)
                ok[f"cov {sep}"] = all(np.array_equal(u, v) for u, v in zip(a, b))
            out[S] = ok
    except Exception as e:  # noqa: BLE001 - reported to the parent
        out["exception"] = repr(e)
    finally:
        dist.destroy_process_group()
    q.put((rank, out))


def test_sharded_quad_mixture_equals_unsharded_bitwise_two_ranks_one_gpu():
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
