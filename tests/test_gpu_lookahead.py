"""GP.predict_cov / GP.lookahead_variance / gpc_predict_cov on the device: against the reference's predict_full block
(tests/golden/full_cases.npz), against the NumPy restatement of test_lookahead_cpu.py on the GP's own fetched
posteriors, against predict_full and predict themselves, the fused (epilogue) form against the stored one, the
look-ahead identity end to end through update's rank-one append, bitwise invariance over batches, chunking and
sharding, edge cases and refusals."""

import copy
import os
import socket
import sys

import numpy as np
import pytest

from conftest import parse_core_name
from test_lookahead_cpu import _counts, lookahead_numpy, predict_cov_numpy, reduce_numpy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gp(model, D, dtype="f64"):
    from test_gpu_api import _gp as make

    return make(model, D, dtype)


def _problem(kernel="se", degree=0, mean="const", N=200, D=3, S=3, seed=1, dtype="f64", s2=False, lo=-2.0, hi=2.0,
             sn2s=None, noise_sd=0.1):
    """Laid out like the _problem of test_gpu_quad_grad.py."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(lo, hi, (N, D))
    y = np.sin(X.sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1))
    model = dict(kernel=kernel, degree=degree, mean=mean, noise=(1, 1 if s2 else 0, 0))
    cov_N, noise_N, mean_N = _counts(model, D)
    S = S if sn2s is None else len(sn2s)
    hyp = np.zeros((S, cov_N + noise_N + mean_N))
    hyp[:, :cov_N - 1] = np.log(1.2)
    hyp[:, cov_N] = np.log(noise_sd)
    if kernel == "rq":
        hyp[:, cov_N - 1] = 0.5
        hyp[:, cov_N - 2] = 0.0
    if mean != "zero":
        hyp[:, cov_N + noise_N] = 0.3
    if mean == "negquad":
        hyp[:, cov_N + noise_N + 1 + D:] = np.log(3.0)
    hyp += 0.05 * rng.standard_normal(hyp.shape)
    if sn2s is not None:
        hyp[:, cov_N] = 0.5 * np.log(sn2s)
    s2v = 0.01 * (1 + rng.uniform(0, 1, (N, 1))) if s2 else None
    gp = _gp(model, D, dtype)
    gp.update(X_new=X, y_new=y, s2_new=s2v, hyp=hyp)
    if sn2s is not None:
        assert [p.L_chol for p in gp.posteriors] == [v >= 1e-6 for v in sn2s]
    return gp, model, X, hyp


def _points(D, Mr, Mc, seed=5):
    rng = np.random.default_rng(seed)
    return rng.uniform(-2.5, 2.5, (Mr, D)), rng.uniform(-2.5, 2.5, (Mc, D))


def _fused_calls(gp):
    from gpyreg_amd import _lib

    return _lib.context(gp.device).get_option("cov_fused")


def _err(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# ---- 1. golden parity


def test_golden_parity_and_transpose():
    g = np.load(os.path.join(ROOT, "tests", "golden", "full_cases.npz"), allow_pickle=False)
    assert len(g["names"]) == 5
    for name in g["names"]:
        tag, model, N, D, _ = parse_core_name(str(name) + "|plain")
        X, y, hyp, xs = g[tag + "_X"], g[tag + "_y"], g[tag + "_hyp"], g[tag + "_xs"]
        s2 = g[tag + "_s2"] if tag + "_s2" in g.files else None
        ref = g[tag + "_pf_cov"]
        scale = np.abs(ref).max()
        gp = _gp(model, D)
        gp.update(X_new=X, y_new=y, s2_new=s2, hyp=hyp)
        for k in (4, 5):
            C = gp.predict_cov(xs[:k], xs[k:])
            assert C.shape == (k, 9 - k, hyp.shape[0])
            print(tag, k, "golden block error / scale", np.abs(C - ref[:k, k:, :]).max() / scale)
            assert np.abs(C - ref[:k, k:, :]).max() <= 1e-7 * scale, (name, k)
            Ct = gp.predict_cov(xs[k:], xs[:k])
            assert np.abs(Ct.transpose(1, 0, 2) - C).max() <= 1e-7 * scale, (name, k)


# ---- 2. parity with the restatement on the GP's own posteriors


def _parity(gp, model, X, xr, xc, rtol, s2_cand=None, weights=None):
    posts = list(gp.posteriors)
    C = gp.predict_cov(xr, xc)
    Cref, _ = predict_cov_numpy(model, posts, X, xr, xc)
    for s in range(C.shape[2]):
        e = _err(C[:, :, s], Cref[:, :, s])
        print("cov parity", model["kernel"], model["degree"], gp.dtype if hasattr(gp, "dtype") else "", s, e)
        assert e <= rtol, (s, e)
    R = gp.lookahead_variance(xc, xr, weights=weights, s2_cand=s2_cand, separate_samples=True)
    Rref = lookahead_numpy(model, posts, X, xc, xr, weights=weights, s2_cand=s2_cand)
    for s in range(R.shape[1]):
        e = _err(R[:, s], Rref[:, s])
        print("look-ahead parity", model["kernel"], model["degree"], s, e)
        assert e <= rtol, (s, e)
    return C, R


@pytest.mark.parametrize("dtype,rtol", [("f64", 1e-8), ("f32", 1e-3)])
@pytest.mark.parametrize("kernel,degree,mean,s2", [
    ("se", 0, "const", False), ("se_iso", 0, "negquad", True), ("matern", 1, "zero", False),
    ("matern", 3, "const", True), ("matern", 5, "negquad", False), ("matern_iso", 5, "const", False),
    ("rq", 0, "const", True)])
def test_parity_with_the_restatement(kernel, degree, mean, s2, dtype, rtol):
    gp, model, X, hyp = _problem(kernel, degree, mean, s2=s2, dtype=dtype)
    xr, xc = _points(3, 40, 17)
    s2c = 0.02 * np.ones((17, 1)) if s2 else None
    w = np.random.default_rng(3).uniform(0, 1, (40, hyp.shape[0]))
    _parity(gp, model, X, xr, xc, rtol, s2_cand=s2c, weights=w)


@pytest.mark.parametrize("dtype,rtol", [("f64", 1e-8), ("f32", 1e-3)])
@pytest.mark.parametrize("sn2s", [(1e-7, 1e-8), (1e-2, 1e-7, 1e-7, 1e-2, 1e-7, 1e-2)])
def test_low_noise_and_mixed_batches(sn2s, dtype, rtol):
    """L_chol = 0 samples alone and interleaved with L_chol = 1 samples (several launches at nonzero sample offsets), on
    well-spread inputs: parity with the restatement, and each sample bitwise equal to its own single-sample GP."""
    gp, model, X, hyp = _problem("se", N=40, lo=-3, hi=3, sn2s=sn2s, dtype=dtype, seed=11)
    xr, xc = _points(3, 30, 12)
    C, R = _parity(gp, model, X, xr, xc, rtol)
    for s in range(len(sn2s)):
        one = _gp(model, 3, dtype)
        one.update(X_new=X, y_new=gp.y, hyp=hyp[s:s + 1])
        assert np.array_equal(one.predict_cov(xr, xc)[:, :, 0], C[:, :, s]), s
        assert np.array_equal(one.lookahead_variance(xc, xr, separate_samples=True)[:, 0], R[:, s]), s


# ---- 3. consistency with predict_full and predict


@pytest.mark.parametrize("N,Ma,Mb", [(200, 37, 300), (1000, 1000, 1000)])
def test_block_of_predict_full_and_variance_of_predict(N, Ma, Mb):
    gp, model, X, hyp = _problem("matern", 5, N=N, S=2)
    xa, xb = _points(3, Ma, Mb)
    C = gp.predict_cov(xa, xb)
    _, full = gp.predict_full(np.vstack([xa, xb]))
    e = np.abs(C - full[:Ma, Ma:, :]).max() / np.abs(full).max()
    print("block of predict_full", N, Ma, Mb, e)
    assert e <= 1e-12
    h = gp._post_handle
    _, _, fs2b = h.predict_cov(xa, xb, np.ones(Ma), want_cov=False, want_fs2=True)
    _, fs2 = h.predict(xb)
    cov_N = _counts(model, 3)[0]
    kss = max(np.exp(2 * p.hyp[cov_N - 1]) for p in gp.posteriors)
    print("fs2b against predict", N, Ma, Mb, np.abs(fs2b - fs2).max() / kss)
    assert np.abs(fs2b - fs2).max() <= 1e-12 * kss


# ---- 4. the fused form against the stored one


@pytest.mark.parametrize("N,Mr,Mc,fused", [(200, 300, 50, False), (1000, 1000, 1000, True)])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_fused_against_stored(N, Mr, Mc, fused, dtype):
    """lookahead_variance (no covariance leaves the device; from 64 128-tiles on the reduction runs in the product's
    epilogue) against the stored covariance of the same GP reduced in NumPy, within 1e-12 of the largest value (the
    sums run in fp64 in both precisions).  The library's counter says which form ran."""
    gp, model, X, hyp = _problem("se", N=N, S=3, dtype=dtype)
    xr, xc = _points(3, Mr, Mc)
    cov_N, noise_N, _ = _counts(model, 3)
    rng = np.random.default_rng(9)
    for w in (None, rng.uniform(0, 1, Mr), rng.uniform(0, 1, (Mr, 3))):
        n0 = _fused_calls(gp)
        R = gp.lookahead_variance(xc, xr, weights=w, separate_samples=True)
        assert _fused_calls(gp) - n0 == (1 if fused else 0)
        n0 = _fused_calls(gp)
        cov, _, fs2b = gp._post_handle.predict_cov(xr, xc, None, want_cov=True, want_fs2=True)
        assert _fused_calls(gp) == n0  # a covariance was asked for: stored
        den = np.maximum(fs2b, 0) + np.array([np.exp(2 * p.hyp[cov_N]) * p.sn2_mult for p in gp.posteriors])[None, :]
        ref = reduce_numpy(cov.transpose(1, 2, 0), w, den)
        print("fused" if fused else "stored", dtype, "against the NumPy reduction", _err(R, ref))
        assert _err(R, ref) <= 1e-12
        assert np.array_equal(cov.transpose(1, 2, 0), gp.predict_cov(xr, xc))


# ---- 5. the identity end to end


@pytest.mark.parametrize("kernel,degree", [("se", 0), ("matern", 5), ("rq", 0), ("se_iso", 0)])
def test_identity_through_the_rank_one_append(kernel, degree):
    """Append candidate c (update's rank-one path) to a copy of the GP: the drop of the weighted predictive variance at
    the reference points is lookahead_variance's value for c, within 1e-8 of the largest reduction (the fp64 parity
    figure; the CPU reference holds 1e-14 on these inputs)."""
    gp, model, X, hyp = _problem(kernel, degree)
    S = hyp.shape[0]
    xr, xc = _points(3, 40, 6)
    assert all(p.sn2_mult == 1 for p in gp.posteriors)
    rng = np.random.default_rng(4)
    for w in (None, rng.uniform(0, 1, 40), rng.uniform(0, 1, (40, S))):
        R = gp.lookahead_variance(xc, xr, weights=w, separate_samples=True)
        wm = np.full((40, S), 1.0 / 40) if w is None else (w if w.ndim == 2 else np.repeat(w[:, None], S, 1))
        _, v0 = gp.predict(xr, separate_samples=True)
        worst = 0.0
        for c in range(xc.shape[0]):
            g2 = copy.deepcopy(gp)
            g2.update(X_new=xc[c:c + 1], y_new=np.array([[0.7]]))
            assert g2.X.shape[0] == X.shape[0] + 1 and all(p.sn2_mult == 1 for p in g2.posteriors)
            _, v1 = g2.predict(xr, separate_samples=True)
            worst = max(worst, np.abs(np.sum(wm * (v0 - v1), 0) - R[c]).max())
        print(kernel, "identity error / largest reduction", worst / np.abs(R).max())
        assert worst <= 1e-8 * np.abs(R).max()
        assert np.allclose(gp.lookahead_variance(xc, xr, weights=w)[:, 0], R.mean(1), rtol=1e-14, atol=0)


# ---- 6. bitwise invariance


@pytest.mark.parametrize("Mr,Mc", [(300, 200), (1000, 1000)])
def test_repeats_copies_and_sample_subsets_bitwise(Mr, Mc):
    gp, model, X, hyp = _problem("se", N=300, D=4, S=16, seed=4)
    xr, xc = _points(4, Mr, Mc)
    w = np.random.default_rng(2).uniform(0, 1, (Mr, 16))
    R = gp.lookahead_variance(xc, xr, weights=w, separate_samples=True)
    C = gp.predict_cov(xr, xc)
    assert np.array_equal(gp.lookahead_variance(xc, xr, weights=w, separate_samples=True), R)
    assert np.array_equal(gp.predict_cov(xr, xc), C)
    g2 = copy.deepcopy(gp)
    assert np.array_equal(g2.lookahead_variance(xc, xr, weights=w, separate_samples=True), R)
    assert np.array_equal(g2.predict_cov(xr, xc), C)
    for s in (0, 7, 15):
        one = _gp(model, 4)
        one.update(X_new=X, y_new=gp.y, hyp=hyp[s:s + 1])
        assert np.array_equal(one.lookahead_variance(xc, xr, weights=w[:, s:s + 1], separate_samples=True)[:, 0], R[:, s])
        assert np.array_equal(one.predict_cov(xr, xc)[:, :, 0], C[:, :, s])
    # candidate subsets: other padded widths and tile counts, to rounding
    for lo, hi in ((0, 70), (130, Mc)):
        r = gp.lookahead_variance(xc[lo:hi], xr, weights=w, separate_samples=True)
        assert np.abs(r - R[lo:hi]).max() <= 1e-12 * np.abs(R).max()


@pytest.mark.parametrize("Mr,Mc,budget", [(300, 200, "16"), (1000, 1000, "64")])
def test_forced_chunks_on_a_mixed_batch_bitwise(monkeypatch, Mr, Mc, budget):
    """A budget that holds two samples of the scratch per chunk: several chunks, non-resident constants, runs of equal
    L_chol split at the chunk borders."""
    gp, model, X, hyp = _problem("se", N=300, D=4, lo=-3, hi=3, sn2s=(1e-2, 1e-7) * 3 + (1e-2,), seed=6)
    xr, xc = _points(4, Mr, Mc)
    w = np.random.default_rng(2).uniform(0, 1, (Mr, 7))
    whole = gp.lookahead_variance(xc, xr, weights=w, separate_samples=True), gp.predict_cov(xr, xc)
    from gpyreg_amd import _lib
    from scratch_sizes import cov_per, cov_shared, pad, planned_chunk

    monkeypatch.setenv("GPC_MEM_BUDGET_MB", budget)
    look = gp.lookahead_variance(xc, xr, weights=w, separate_samples=True)
    chunks = [_lib.context(gp.device).get_option("last_chunk")]
    chunked = look, gp.predict_cov(xr, xc)
    chunks.append(_lib.context(gp.device).get_option("last_chunk"))
    monkeypatch.delenv("GPC_MEM_BUDGET_MB")
    assert np.array_equal(whole[0], chunked[0]) and np.array_equal(whole[1], chunked[1])
    # ... in the chunks that the scratch's closed form gives: the look-ahead is reduced in the product's epilogue from 64
    # 128-tiles on, the covariance is always stored (and staged on its way out)
    fused = (pad(Mr) // 128) * (pad(Mc) // 128) >= 64
    want = [planned_chunk(7, int(budget), cov_per(384, pad(Mr), pad(Mc), 4, 8, f), cov_shared(Mr, Mc, 4, c))
            for f, c in ((fused, False), (False, True))]
    assert chunks == want and 0 < want[0] < 7, (chunks, want)


def test_other_entry_points_keep_their_bits():
    gp, model, X, hyp = _problem("se", N=300, D=4, S=4, seed=4)
    xr, xc = _points(4, 300, 200)
    mu, sigma = xc[:30], 0.4 * np.ones((30, 4))
    before = gp.predict(xc, separate_samples=True), gp.predict_full(xc[:50]), gp.quad(mu, sigma, compute_var=True)
    gp.lookahead_variance(xc, xr)
    gp.predict_cov(xr, xc)
    after = gp.predict(xc, separate_samples=True), gp.predict_full(xc[:50]), gp.quad(mu, sigma, compute_var=True)
    for b, a in zip(before, after):
        assert all(np.array_equal(u, v) for u, v in zip(b, a))


# ---- 7. edge cases


def test_edge_cases(monkeypatch):
    gp, model, X, hyp = _problem("matern", 5, noise_sd=0.01)
    posts = list(gp.posteriors)
    xr, xc = _points(3, 40, 6)
    # a candidate equal to a training point (small noise) and one equal to a reference point
    xc2 = np.vstack([X[3:4], xr[7:8], xc])
    R = gp.lookahead_variance(xc2, xr, separate_samples=True)
    ref = lookahead_numpy(model, posts, X, xc2, xr)
    assert np.all(np.isfinite(R)) and _err(R, ref) <= 1e-8
    # zero weights
    assert np.all(gp.lookahead_variance(xc, xr, weights=np.zeros(40), separate_samples=True) == 0)
    # one reference point, one candidate
    R1 = gp.lookahead_variance(xc[:1], xr[:1], separate_samples=True)
    assert R1.shape == (1, 3) and _err(R1, lookahead_numpy(model, posts, X, xc[:1], xr[:1])) <= 1e-8
    assert gp.predict_cov(xr[0], xc[0]).shape == (1, 1, 3)
    # odd sizes: the padding contributes nothing
    xa, xb = _points(3, 129, 127, seed=8)
    Ra = gp.lookahead_variance(xb, xa, separate_samples=True)
    assert _err(Ra, lookahead_numpy(model, posts, X, xb, xa)) <= 1e-8
    assert _err(gp.predict_cov(xa, xb), predict_cov_numpy(model, posts, X, xa, xb)[0]) <= 1e-8
    # a reduction of 0 where den <= 0: the device's variance is lowered on chosen rows and the noise taken away
    h = gp._post_handle
    real = h.predict_cov
    base = real(xr, xc, np.full(40, 1.0 / 40), want_cov=False, want_fs2=True)

    def lowered(*a, **k):
        cov, wsq, fs2 = real(*a, **k)
        fs2 = fs2.copy()
        fs2[0:2, 0] = -1.0
        fs2[4, :] = 0.0
        return cov, wsq, fs2

    monkeypatch.setattr(h, "predict_cov", lowered)
    monkeypatch.setattr(gp.noise, "compute", lambda *a, **k: 0.0)
    R0 = gp.lookahead_variance(xc, xr, separate_samples=True)
    held = np.zeros((6, 3), bool)
    held[0:2, 0] = True
    held[4, :] = True
    assert np.all(R0[held] == 0)
    assert np.array_equal(R0[~held], (base[1] / base[2])[~held])


# ---- 8. refusals and the -2 path


def test_refusals(monkeypatch):
    import gpyreg_amd as gpr

    gp, model, X, hyp = _problem("se", N=300, D=4)
    xr, xc = _points(4, 300, 300)
    monkeypatch.setenv("GPC_MEM_BUDGET_MB", "1")
    for call in (lambda: gp.predict_cov(xr, xc), lambda: gp.lookahead_variance(xc, xr)):
        with pytest.raises(RuntimeError) as e:
            call()
        msg = str(e.value)
        assert "scratch of one sample" in msg and "N_pad = 384" in msg and "Ma_pad = 384" in msg and "Mb_pad = 384" in msg
    monkeypatch.delenv("GPC_MEM_BUDGET_MB")
    assert gp.predict_cov(xr, xc).shape == (300, 300, 3)
    with pytest.raises(ValueError, match="weights must be"):
        gp.lookahead_variance(xc, xr, weights=np.ones(299))
    with pytest.raises(ValueError, match="finite"):
        gp.lookahead_variance(xc, xr, weights=np.full(300, np.nan))
    with pytest.raises(ValueError, match="nothing to compute"):
        gp._post_handle.predict_cov(xr, xc, None, want_cov=False)
    with pytest.raises(AssertionError, match="input dimension"):
        gp.predict_cov(xr[:, :3], xc)
    with pytest.raises(RuntimeError, match="bad arguments"):
        gp.predict_cov(np.zeros((0, 4)), xc)
    gp.clean()
    with pytest.raises(ValueError, match="posteriors have been cleaned"):
        gp.predict_cov(xr, xc)
    with pytest.raises(ValueError, match="posteriors have been cleaned"):
        gp.lookahead_variance(xc, xr)

    from test_gpu_user_kernel import PySquaredExponential

    user = gpr.GP(4, PySquaredExponential(), gpr.mean_functions.ZeroMean(),
                  gpr.noise_functions.GaussianNoise(constant_add=True))
    user.update(X_new=X, y_new=gp.y, hyp=np.r_[np.zeros(5), np.log(0.1)][None, :])
    assert user.predict(xc)[0].shape == (300, 1)
    with pytest.raises(NotImplementedError, match="PySquaredExponential"):
        user.predict_cov(xr, xc)
    with pytest.raises(NotImplementedError, match="PySquaredExponential"):
        user.lookahead_variance(xc, xr)


# ---- sharding: the pattern of test_gpu_quad_grad.py::test_sharded_quad_grad_equals_unsharded_bitwise_two_ranks_one_gpu


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
            xr, xc = X[:60] + 0.05, X[100:130] - 0.03
            w = np.random.default_rng(1).uniform(0, 1, (60, S))

            def make():
                return gpr.GP(X.shape[1], gpr.covariance_functions.Matern(5),
                              gpr.mean_functions.ConstantMean(), gpr.noise_functions.GaussianNoise(constant_add=True))

            ref = make()
            ref.shard = False
            ref.update(X_new=X, y_new=y, hyp=hyp)
            gp = make()
            gp.update(X_new=X, y_new=y, hyp=hyp)
            ok = {"cov": np.array_equal(ref.predict_cov(xr, xc), gp.predict_cov(xr, xc))}
            for kw in (dict(separate_samples=True), dict(), dict(weights=w, separate_samples=True), dict(weights=w[:, 0])):
                ok[str(sorted(kw))] = np.array_equal(ref.lookahead_variance(xc, xr, **kw),
                                                     gp.lookahead_variance(xc, xr, **kw))
            out[S] = ok
    except Exception as e:  # noqa: BLE001 - reported to the parent
        out["exception"] = repr(e)
    finally:
        dist.destroy_process_group()
    q.put((rank, out))


def test_sharded_equals_unsharded_bitwise_two_ranks_one_gpu():
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
