"""GP.draw_functions / gpc_draw: joint posterior draws on the device.  The device stream against its NumPy restatement
(gpyreg_amd/_philox.py), the draws against NumPy's mu + chol(C + tau I) z on the oracle's posteriors, bitwise
invariance over batches, chunks, sharding and repeated calls, prefix consistency, the empirical moments, the jitter
ladder, the noise and the refusals."""

import copy
import os
import socket
import sys

import numpy as np
import pytest

from conftest import parse_core_name
from gpyreg_amd import _philox

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gp(model, D, dtype="f64"):
    from test_gpu_api import _gp as make

    return make(model, D, dtype)


def _oracle_moments(model, posts, X, y, xs):
    """Per sample: mu_s = m_s + fmu_s (M,) and C_s = K** - K*^T (K + Sigma)^-1 K* (M, M), from the oracle's posteriors."""
    from oracle import gp_oracle as orc

    D = X.shape[1]
    cov_N = orc.cov_count(model["kernel"], D)
    mu_sep, _ = orc.predict(model, posts, X, y, xs, separate_samples=True)
    Cs = []
    for p in posts:
        h = p.hyp[:cov_N]
        Ks = orc.covariance(model["kernel"], h, X, xs, degree=model["degree"])
        Kss = orc.covariance(model["kernel"], h, xs, degree=model["degree"])
        if p.L_chol:
            sW = p.sW[:, 0]
            V = np.linalg.solve(p.L.T, sW[:, None] * Ks)
            C = Kss - V.T @ V
        else:
            C = Kss + Ks.T @ (p.L @ Ks)
        Cs.append((C + C.T) / 2)
    return mu_sep, Cs


def _numpy_draws(mu, C, tau, seed, s, R, stream=0):
    z = _philox.normals_block(seed, stream, C.shape[0], R, [s])[:, :, 0]
    L = np.linalg.cholesky(C + tau * np.eye(C.shape[0]))
    return mu[:, None] + L @ z, L, z


def test_device_stream_equals_host_restatement():
    from gpyreg_amd import _lib

    ctx = _lib.context()
    for seed, stream, s, r, j0, count in [(0, 0, 0, 0, 0, 4096), (2**63 + 7, 1, 17, 5, 3, 1001),
                                          (2**64 - 1, 0, 2**31 - 1, 2**31 - 1, 12345, 777), (99, 1, 3, 64, 1, 9)]:
        dev = ctx.debug_normals(seed, stream, s, r, j0, count)
        host = _philox.normals(seed, stream, s, r, np.arange(j0, j0 + count))
        assert np.all(np.abs(dev - host) <= 1e-14 * np.maximum(1.0, np.abs(host))), (seed, stream, s, r, j0)


def test_golden_models_match_numpy(core_golden):
    """Every golden model, both L_chol kinds: f = mu + chol(C + tau I) z with C and mu from the oracle's posteriors, to a
    tolerance bounded by conditioning: a relative perturbation d of C moves L z by about cond(C + tau I) d |L z|, with d
    the factorization's eps plus the distance between the device's C (predict_full) and the oracle's -- large for the
    low-noise cases, where C = K** - K*^T (K + Sigma)^-1 K* inherits cond(K + Sigma) -- and the mean enters with the
    distance between the device's predictive mean and the oracle's (1e-4 relative on the jitter cases).  Cases where
    the covariance bound exceeds 1 % are not compared."""
    from oracle import gp_oracle as orc

    g = core_golden
    done, lchol0 = 0, 0
    seed, R = 5, 8
    for name in g["names"]:
        tag, model, N, D, flavour = parse_core_name(name)
        X, y, hyp = g[tag + "_X"], g[tag + "_y"], g[tag + "_hyp"]
        s2 = g[tag + "_s2"] if tag + "_s2" in g.files else None
        xs = g[tag + "_xs"]
        gp = _gp(model, D)
        gp.update(X_new=X, y_new=y, s2_new=s2, hyp=hyp)
        mult = [p.sn2_mult for p in gp.posteriors]
        try:
            posts = orc.posteriors(model, hyp, X, y, s2, force_mult=mult)
        except np.linalg.LinAlgError:
            continue
        try:
            f, tau = gp.draw_functions(xs, n_draws=R, seed=seed, return_jitter=True)
        except np.linalg.LinAlgError:
            assert flavour != "plain", name
            continue
        assert f.shape == (xs.shape[0], R, hyp.shape[0]) and np.all(np.isfinite(f)), name
        mu, Cs = _oracle_moments(model, posts, X, y, xs)
        dev_mu, dev_cov = gp.predict_full(xs)
        for s in range(hyp.shape[0]):
            try:
                ref, L, z = _numpy_draws(mu[:, s], Cs[s], tau[s], seed, s, R)
            except np.linalg.LinAlgError:
                continue
            Cj = Cs[s] + tau[s] * np.eye(xs.shape[0])
            cond = np.linalg.cond(Cj)
            dev = ref - mu[:, s:s + 1]
            scale = max(np.abs(dev).max(), 1e-300)
            d = 1e-15 + np.abs(dev_cov[:, :, s] - Cs[s]).max() / np.abs(Cs[s]).max()
            if 2 * d * cond > 1e-2:
                continue
            e_mu = np.abs(dev_mu[:, s] - mu[:, s]).max()
            tol = (1e-10 + 2 * d * cond) * scale + 1e-12 * np.abs(mu[:, s]).max() + 2 * e_mu
            err = np.abs(f[:, :, s] - ref).max()
            assert err <= tol, (name, s, err, tol, cond)
            done += 1
            lchol0 += not gp.posteriors[s].L_chol
    assert done >= 25 and lchol0 >= 2, (done, lchol0)


def _lownoise_problem(sn2s, N=40, D=3, seed=11, dtype="f64"):
    from test_gpu_predict_grad import _lownoise_problem as make

    return make(sn2s, N=N, D=D, seed=seed, dtype=dtype)


@pytest.mark.parametrize("dtype,rtol", [("f64", 1e-10), ("f32", 1e-3)])
@pytest.mark.parametrize("sn2s", [(1e-2,), (1e-7, 1e-8), (1e-2, 1e-7, 1e-7, 1e-2, 1e-7, 1e-2)])
@pytest.mark.parametrize("M", [37, 300])
def test_well_conditioned_parity_and_mixed_batches(sn2s, dtype, rtol, M):
    """Query points away from the data (C_s well conditioned): rtol of the largest entry against NumPy, for L_chol = 1,
    L_chol = 0 and batches interleaving both; no jitter needed; every sample the bits of its own single-sample GP.
    M = 300 spreads the points over a larger box (C stays well conditioned) and factors in three leaves."""
    from oracle import gp_oracle as orc

    gp, model, X, y, hyp = _lownoise_problem(sn2s, dtype=dtype)
    xs = np.random.default_rng(12).uniform(-3, 3, (M, X.shape[1])) * (1 if M < 100 else 4)
    seed, R = 123, 10
    f, tau = gp.draw_functions(xs, n_draws=R, seed=seed, return_jitter=True)
    assert np.all(tau == 0)
    posts = orc.posteriors(model, hyp, X, y, None)
    mu, Cs = _oracle_moments(model, posts, X, y, xs)
    for s in range(len(sn2s)):
        ref, _, _ = _numpy_draws(mu[:, s], Cs[s], 0.0, seed, s, R)
        assert np.abs(f[:, :, s] - ref).max() <= rtol * np.abs(ref).max(), s
    # a single-sample GP draws with stream index 0; the ABI's s_offset keys it as sample s of the batch
    for s in range(len(sn2s)):
        one = _gp(model, X.shape[1], dtype)
        one.update(X_new=X, y_new=y, hyp=hyp[s:s + 1])
        f1, t1 = one._post_handle.draw(xs, R, seed, s_offset=s)
        m = gp.mean.compute(hyp[s, 5:], xs).ravel()
        assert np.array_equal(f1[:, :, 0] + m[:, None], f[:, :, s]) and t1[0] == 0, s


def test_subset_chunks_repeats_and_deepcopy_bitwise(monkeypatch):
    gp, model, X, y, hyp = _lownoise_problem((1e-2, 1e-7) * 5, N=300, D=4)
    xs = np.random.default_rng(14).uniform(-3, 3, (300, 4))
    seed, R = 2**63 + 3, 20
    whole = gp.draw_functions(xs, n_draws=R, seed=seed)
    assert np.array_equal(gp.draw_functions(xs, n_draws=R, seed=seed), whole)
    assert np.array_equal(copy.deepcopy(gp).draw_functions(xs, n_draws=R, seed=seed), whole)
    # a subset of the samples at the ABI, keyed by s_offset
    sub = _gp(model, 4)
    sub.update(X_new=X, y_new=y, hyp=hyp[3:7])
    fs, _ = sub._post_handle.draw(xs, R, seed, s_offset=3)
    fw, _ = gp._post_handle.draw(xs, R, seed)
    assert np.array_equal(fs, fw[:, :, 3:7])
    # ~7 MB of draw scratch per sample at mpad = 384: a few samples per chunk
    monkeypatch.setenv("GPC_MEM_BUDGET_MB", "40")
    chunked = gp.draw_functions(xs, n_draws=R, seed=seed)
    from gpyreg_amd import _lib
    from scratch_sizes import planned_chunk, rhs_per, rhs_shared

    # ... in the chunks that the scratch's closed form gives (the factor's three slabs count as the scratch they are)
    want = planned_chunk(10, 40, rhs_per(384, 384, True, 8, 4, "cross", False, M=300, R=R),
                         rhs_shared(300, 300, 4, 10, full=True, R=R))
    assert 1 < want < 10 and _lib.context(gp.device).get_option("last_chunk") == want
    monkeypatch.setenv("GPC_MEM_BUDGET_MB", "1")
    with pytest.raises(RuntimeError, match="exceeds the device memory budget"):
        gp.draw_functions(xs, n_draws=R, seed=seed)
    monkeypatch.delenv("GPC_MEM_BUDGET_MB")
    assert np.array_equal(chunked, whole)


@pytest.mark.parametrize("dtype,tol", [("f64", 1e-10), ("f32", 1e-4)])
def test_prefix_consistency(dtype, tol):
    gp, model, X, y, hyp = _lownoise_problem((1e-2, 1e-7, 1e-2), dtype=dtype)
    xs = np.random.default_rng(15).uniform(-3, 3, (150, X.shape[1]))
    f = gp.draw_functions(xs, n_draws=12, seed=9)
    scale = np.abs(f).max()
    for k in (1, 7, 64, 129):
        fk = gp.draw_functions(xs[:k], n_draws=12, seed=9)
        assert np.abs(fk - f[:k]).max() <= tol * scale, k
    f5 = gp.draw_functions(xs, n_draws=5, seed=9)
    assert np.abs(f5 - f[:, :5]).max() <= tol * scale


def test_empirical_moments_match_the_covariance():
    from oracle import gp_oracle as orc

    gp, model, X, y, hyp = _lownoise_problem((1e-2, 1e-7))
    xs = np.random.default_rng(16).uniform(-3, 3, (6, X.shape[1]))
    R = 20000
    f = gp.draw_functions(xs, n_draws=R, seed=31)
    posts = orc.posteriors(model, hyp, X, y, None)
    mu, Cs = _oracle_moments(model, posts, X, y, xs)
    for s in range(2):
        d = f[:, :, s] - mu[:, s:s + 1]
        C = Cs[s]
        se_mean = np.sqrt(np.diag(C) / R)
        assert np.all(np.abs(d.mean(1)) <= 5 * se_mean), s
        emp = d @ d.T / R
        se_cov = np.sqrt((np.outer(np.diag(C), np.diag(C)) + C**2) / R)
        assert np.all(np.abs(emp - C) <= 5 * se_cov), s


def test_jitter_on_duplicated_query_points():
    """Query points that repeat low-noise training points (and each other): C_s is singular, the first attempt fails and
    the ladder finds tau > 0; the draws are finite and match NumPy at that tau, to a bound of eps |C| / sqrt(tau)."""
    from oracle import gp_oracle as orc

    gp, model, X, y, hyp = _lownoise_problem((1e-7, 1e-8))
    rng = np.random.default_rng(17)
    xs = np.concatenate([X[:6], X[:6], rng.uniform(-3, 3, (10, X.shape[1]))])
    R = 6
    f, tau = gp.draw_functions(xs, n_draws=R, seed=4, return_jitter=True)
    assert np.all(np.isfinite(f)) and np.all(tau > 0), tau
    posts = orc.posteriors(model, hyp, X, y, None)
    mu, Cs = _oracle_moments(model, posts, X, y, xs)
    for s in range(2):
        t = tau[s] / np.mean(np.diag(Cs[s]))
        assert any(np.isclose(t, 10.0**e, rtol=1e-6) for e in range(-12, -5)), t
        ref, L, z = _numpy_draws(mu[:, s], Cs[s], tau[s], 4, s, R)
        bound = 100 * np.finfo(float).eps * np.abs(Cs[s]).max() / np.sqrt(tau[s]) * np.abs(z).max() * xs.shape[0]
        assert np.abs(f[:, :, s] - ref).max() <= bound + 1e-10 * np.abs(ref).max(), s


def test_add_noise_uses_stream_one():
    gp, model, X, y, hyp = _lownoise_problem((1e-2, 1e-7, 1e-2))
    xs = np.random.default_rng(18).uniform(-3, 3, (33, X.shape[1]))
    f = gp.draw_functions(xs, n_draws=7, seed=77)
    fn = gp.draw_functions(xs, n_draws=7, seed=77, add_noise=True)
    for s in range(3):
        mult = gp.posteriors[s].sn2_mult
        sd = np.sqrt(np.exp(2 * hyp[s, 4]) * (1 if mult is None else mult))
        zn = _philox.normals_block(77, 1, 33, 7, [s])[:, :, 0]
        assert np.allclose(fn[:, :, s], f[:, :, s] + sd * zn, rtol=0, atol=1e-13 * max(1.0, np.abs(f).max()))


def test_no_data_gp_draws_from_the_prior():
    import gpyreg_amd as gpr

    D = 2
    gp = gpr.GP(D, gpr.covariance_functions.SquaredExponential(), gpr.mean_functions.ZeroMean(),
                gpr.noise_functions.GaussianNoise(constant_add=True))
    hyp = np.array([[0.1, -0.2, 0.0, np.log(0.1)]])
    gp.update(hyp=hyp)
    xs = np.random.default_rng(19).uniform(-1, 1, (9, D))
    f, tau = gp.draw_functions(xs, n_draws=4, seed=3, return_jitter=True)
    K = gp.covariance.compute(hyp[0, :3], xs)
    ref = np.linalg.cholesky(K + tau[0] * np.eye(9)) @ _philox.normals_block(3, 0, 9, 4, [0])[:, :, 0]
    assert np.allclose(f[:, :, 0], ref, rtol=1e-13, atol=1e-13)


def test_refusals():
    import gpyreg_amd as gpr
    from test_gpu_user_kernel import PySquaredExponential

    rng = np.random.default_rng(0)
    X = rng.uniform(-1, 1, (40, 2))
    y = np.sin(X[:, :1])
    hyp = np.array([[0.0, 0.0, 0.0, np.log(0.1), 0.0]])
    gp = gpr.GP(2, PySquaredExponential(), gpr.mean_functions.ConstantMean(),
                gpr.noise_functions.GaussianNoise(constant_add=True))
    gp.update(X_new=X, y_new=y, hyp=hyp)
    with pytest.raises(NotImplementedError, match="PySquaredExponential"):
        gp.draw_functions(X[:3])
    gp = gpr.GP(2, gpr.covariance_functions.SquaredExponential(), gpr.mean_functions.ConstantMean(),
                gpr.noise_functions.GaussianNoise(constant_add=True))
    gp.update(X_new=X, y_new=y, hyp=hyp)
    gp.draw_functions(X[:3])
    gp.clean()
    with pytest.raises(ValueError, match="cleaned"):
        gp.draw_functions(X[:3])


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
        bench.CONFIGS[3] = dict(bench.CONFIGS[3], N=700)
        for S in (1, 5, 16):
            X, y, hyp = bench.synthetic_problem(3, S)
            xs = X[:40] + 0.05
            ref = bench.make_gp(3, "f64")
            ref.shard = False
            ref.update(X_new=X, y_new=y, hyp=hyp)
            gp = bench.make_gp(3, "f64")
            gp.update(X_new=X, y_new=y, hyp=hyp)
            ok = {}
            for kw in (dict(), dict(add_noise=True), dict(return_jitter=True)):
                a = ref.draw_functions(xs, n_draws=9, seed=5, **kw)
                b = gp.draw_functions(xs, n_draws=9, seed=5, **kw)
                a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
                ok[str(kw)] = all(np.array_equal(u, v) for u, v in zip(a, b))
            out[S] = ok
    except Exception as e:  # noqa: BLE001 - reported to the parent
        out["exception"] = repr(e)
    finally:
        dist.destroy_process_group()
    q.put((rank, out))


def test_sharded_draws_equal_unsharded_bitwise_two_ranks_one_gpu():
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
