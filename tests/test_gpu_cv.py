"""GP.cv_predict / gpc_cv on the device: leave-fold-out predictions from the resident posterior against the NumPy
restatement of test_cv_cpu.py on the GP's own fetched posteriors, against brute force through the oracle and the
reference's fixture; both engines of the fold Gram; bitwise invariance over folds, batches, chunking and sharding;
posteriors from a Python kernel and from appends; consistency with the GP's own update + predict; the refusals."""

import os
import socket
import sys

import numpy as np
import pytest

from test_cv_cpu import (check_against, cv_bruteforce, cv_data, cv_numpy, lpd_fold_of, scattered_folds)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 15, 17, 63, 65, 129, 130]  # unequal folds, tile borders on both sides, a multi-leaf factorization (k > 128)


def _gp(model, D, dtype="f64"):
    from test_gpu_api import _gp as make

    return make(model, D, dtype)


def _fit(dtype="f64", **kw):
    model, X, y, s2, hyp = cv_data(**kw)
    gp = _gp(model, X.shape[1], dtype)
    gp.update(X_new=X, y_new=y, s2_new=s2, hyp=hyp)
    return gp, model, X, y, s2, hyp


def _folds_with_ends(N, sizes):
    """Scattered disjoint folds of the given sizes; fold 3 holds index 0 and the last fold index N - 1."""
    folds = scattered_folds(N, sizes)
    for want, f in ((0, 3), (N - 1, len(sizes) - 1)):
        owner = {int(i): g for g, I in enumerate(folds) for i in I}
        if owner.get(want) == f:
            continue
        give = int(folds[f][folds[f].size // 2])  # (neither end point: both are placed on purpose)
        assert give not in (0, N - 1)
        folds[f] = np.sort(np.append(folds[f][folds[f] != give], want))
        g = owner.get(want)
        if g is not None:
            folds[g] = np.sort(np.append(folds[g][folds[g] != want], give))
    assert 0 in folds[3] and N - 1 in folds[-1] and [f.size for f in folds] == list(sizes)
    assert np.unique(np.concatenate(folds)).size == sum(sizes)
    return folds


def _sizes_for(N):
    """The longest prefix of SIZES that leaves some of the N points uncovered (all seven need N > 420)."""
    k = max(i for i in range(1, len(SIZES) + 1) if sum(SIZES[:i]) < N)
    return SIZES[:k]


def _device(gp, folds, **kw):
    mu, s2, lpd, lpf = gp.cv_predict(folds, add_noise=True, separate_samples=True, return_lpd=True, **kw)
    return mu, s2, lpf


def _restated(gp, folds):
    y = gp.y
    dmu, v, quad, logdet = cv_numpy(list(gp.posteriors), y, folds)
    return y - dmu, v, lpd_fold_of(quad, logdet, folds, y.shape[0])


def _engine(gp, which=None):
    ctx = gp._ctx()
    if which is None:
        return ctx.get_option("cv_engine_ran")
    ctx.set_option("cv_engine", which)


@pytest.mark.parametrize("N", [200, 333, 460])
def test_parity_with_the_restatement(N):
    """N no multiple of 64 or 128.  Leave-one-out; scattered unequal folds in one call -- sizes 1, 15, 17, 63, 65 at
    N = 200, with 129 at N = 333, all seven (420 points) at N = 460 -- one of which holds index 0 and one index N - 1;
    contiguous folds; folds that cover a part only."""
    gp, model, X, y, s2, hyp = _fit(N=N, S=3)
    cases = dict(loo=None, scattered=_folds_with_ends(N, _sizes_for(N)), contiguous=list(np.array_split(np.arange(N), 4)),
                 partial=[np.arange(5, 40), np.array([N - 1])])
    for name, folds in cases.items():
        got, ref = _device(gp, folds), _restated(gp, folds)
        worst = check_against(ref, got, folds, N, f"N={N} {name}")
        print(f"N={N} {name}: worst relative error {worst:.2e}, engine {_engine(gp)}")
        if folds is not None:
            covered = np.concatenate(folds)
            rest = np.setdiff1d(np.arange(N), covered)
            assert np.all(np.isnan(got[0][rest])) and np.all(np.isnan(got[1][rest]))
            assert not np.any(np.isnan(got[0][covered]))
            assert name == "contiguous" or rest.size > 0


def test_parity_with_the_oracle_brute_force_and_the_reference_fixture():
    for kw in (dict(N=200, S=2), dict(kernel="matern", degree=5, N=120, S=2), dict(N=120, S=2, s2=True)):
        gp, model, X, y, s2, hyp = _fit(**kw)
        N = X.shape[0]
        mults = [p.sn2_mult for p in gp.posteriors]
        for folds in (None, scattered_folds(N, [1, 15, 17, N // 3]), list(np.array_split(np.arange(N), 5))):
            ref = cv_bruteforce(model, hyp, X, y, s2, folds, mults)
            check_against(ref, _device(gp, folds), folds, N, str(kw))
    g = np.load(os.path.join(ROOT, "tests", "golden", "cv_cases.npz"), allow_pickle=False)
    model = dict(kernel="se", degree=0, mean="const", noise=(1, 0, 0))
    gp = _gp(model, 2)
    gp.update(X_new=g["X"], y_new=g["y"], hyp=g["hyp"])
    for name in g["names"]:
        ptr, idx = g[f"{name}_ptr"], g[f"{name}_idx"]
        folds = [idx[a:b] for a, b in zip(ptr[:-1], ptr[1:])]
        ref = g[f"{name}_mu"], g[f"{name}_s2"], g[f"{name}_lpd_fold"]
        check_against(ref, _device(gp, folds), folds, 60, f"fixture {name}")
        if name == "loo":
            check_against(ref, _device(gp, None), None, 60, "fixture loo as None")


@pytest.mark.parametrize("sn2s", [(1e-7, 1e-8), (1e-2, 1e-7, 1e-7, 1e-2, 1e-7, 1e-2)])
def test_low_noise_and_mixed_batches(sn2s):
    from test_gpu_quad_grad import _problem

    gp, model, X, hyp = _problem("se", "const", N=40, lo=-3, hi=3, sn2s=sn2s, seed=11)
    cases = (None, scattered_folds(40, [1, 7, 12]), list(np.array_split(np.arange(40), 3)))
    got = [_device(gp, f) for f in cases]
    for folds, g in zip(cases, got):
        check_against(_restated(gp, folds), g, folds, 40, f"{sn2s} {None if folds is None else len(folds)}")
    for s in range(len(sn2s)):
        one = _gp(model, X.shape[1])
        one.update(X_new=X, y_new=gp.y, hyp=hyp[s:s + 1])
        for folds, g in zip(cases, got):
            r = _device(one, folds)
            assert all(np.array_equal(a[:, 0], b[:, s], equal_nan=True) for a, b in zip(r, g)), s


def test_fp32_posteriors():
    """fp32 storage, fp64 after the load: 1e-3, the project's fp32 bound, against the restatement in fp64 on the fetched
    (fp32) factor.  A float32-factor emulation of this case (N = 200 generator, sn2 = 1e-2) gave 2.7e-4 for the
    leave-one-out mean and ~5e-6 for folds: more than a factor 3 inside the bound, so the case stays at sn2 = 1e-2.
    A held-out point has no scale of its own (a mean may cross 0), so mean and density errors are taken relative to
    the largest magnitude over the covered points / folds; the variance per element."""
    gp, model, X, y, s2, hyp = _fit("f32", N=200, S=3)
    for folds in (None, scattered_folds(200, [1, 15, 17, 63, 65]), list(np.array_split(np.arange(200), 4))):
        got, ref = _device(gp, folds), _restated(gp, folds)
        cov = np.arange(200) if folds is None else np.concatenate(folds)
        e_mu = np.abs(got[0][cov] - ref[0][cov]).max() / np.abs(ref[0][cov]).max()
        e_s2 = (np.abs(got[1][cov] - ref[1][cov]) / ref[1][cov]).max()
        e_lpd = np.abs(got[2] - ref[2]).max() / np.abs(ref[2]).max()
        print("fp32", "LOO" if folds is None else len(folds), "mu %.2e s2 %.2e lpd_fold %.2e" % (e_mu, e_s2, e_lpd))
        assert max(e_mu, e_s2, e_lpd) <= 1e-3


def test_engines_agree_to_rounding():
    perm = np.random.default_rng(9).permutation(700)
    for N, folds in ((333, _folds_with_ends(333, _sizes_for(333))),
                     (700, [np.sort(perm[:300]), np.sort(perm[300:365])])):  # N_pad = 768: several row slabs and tiles
        gp, model, X, y, s2, hyp = _fit(N=N, S=2)
        try:
            _engine(gp, 1)
            h = gp._post_handle
            a = h.cv(folds)
            assert _engine(gp) == 1
            _engine(gp, 2)
            b = h.cv(folds)
            assert _engine(gp) == 2
        finally:
            _engine(gp, 0)
        cov = np.concatenate(folds)
        assert np.array_equal(a[4], b[4]) and not a[4].any()
        for k, (u, v) in enumerate(zip(a[:4], b[:4])):
            u, v = (u[cov], v[cov]) if k < 2 else (u, v)
            e = np.abs(u - v).max() / max(np.abs(u).max(), np.abs(v).max())
            print(f"N={N} output {k}: engines differ by {e:.2e}")
            assert e <= 1e-12, (N, k, e)
        check_against(_restated(gp, folds), _device(gp, folds), folds, N, f"N={N}")
        gp.cv_predict()
        assert _engine(gp) == 0  # the leave-one-out pass has no engine


def test_bitwise_invariance_over_folds_batches_and_spellings():
    gp, model, X, y, s2, hyp = _fit(N=333, S=3)
    folds = _folds_with_ends(333, _sizes_for(333))
    whole = _device(gp, folds)
    for f in (1, 3, 5):  # a fold alone against the same fold among others (another F, another k_max)
        alone = _device(gp, [folds[f]])
        I = folds[f]
        assert np.array_equal(alone[0][I], whole[0][I]) and np.array_equal(alone[1][I], whole[1][I])
        assert np.array_equal(alone[2][0], whole[2][f])
    loo = gp.cv_predict(None, add_noise=True, separate_samples=True, return_lpd=True)
    single = gp.cv_predict([[i] for i in range(333)], add_noise=True, separate_samples=True, return_lpd=True)
    assert all(np.array_equal(a, b) for a, b in zip(loo, single))
    some = [np.array([7]), np.array([0]), np.array([332])]
    part = gp.cv_predict(some, add_noise=True, separate_samples=True, return_lpd=True)
    for f, I in enumerate(some):
        assert np.array_equal(part[0][I], loo[0][I]) and np.array_equal(part[3][f], loo[3][I[0]])
    assert np.isnan(part[0][1]).all()
    for s in range(3):
        one = _gp(model, 3)
        one.update(X_new=X, y_new=y, hyp=hyp[s:s + 1])
        r = _device(one, folds)
        assert all(np.array_equal(a[:, 0], b[:, s], equal_nan=True) for a, b in zip(r, whole)), s
        r = one.cv_predict(None, add_noise=True, separate_samples=True)
        assert np.array_equal(r[0][:, 0], loo[0][:, s]) and np.array_equal(r[1][:, 0], loo[1][:, s])


def test_chunks_bitwise_and_budget_message(monkeypatch):
    from test_gpu_quad_grad import _problem

    gp, model, X, hyp = _problem("se", "const", N=300, D=4, lo=-3, hi=3, sn2s=(1e-2, 1e-7) * 3, seed=6)
    folds = scattered_folds(300, [1, 40, 100])
    whole, loo = gp._post_handle.cv(folds), gp._post_handle.cv(None)
    # one sample's scratch: 3 folds x 3 x 128^2 doubles = 1.1 MB (+ panels for engine 2): budgets of one and two samples
    from gpyreg_amd import _lib
    from scratch_sizes import cv_fold_per, cv_loo_per, planned_chunk

    ctx = _lib.context(gp.device)
    for mb in ("2", "4"):
        monkeypatch.setenv("GPC_MEM_BUDGET_MB", mb)
        chunked = gp._post_handle.cv(folds)
        chunks, engine = [ctx.get_option("last_chunk")], ctx.get_option("cv_engine_ran")
        loo_c = gp._post_handle.cv(None)
        chunks.append(ctx.get_option("last_chunk"))
        monkeypatch.delenv("GPC_MEM_BUDGET_MB")
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(whole, chunked)), mb
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(loo, loo_c)), mb
        # ... in the chunks that the scratch's closed forms give (the leave-one-out pass holds all six samples)
        want = [planned_chunk(6, int(mb), cv_fold_per(384, 3, 100, engine)),
                planned_chunk(6, int(mb), cv_loo_per(384))]
        assert chunks == want and want[1] == 6 and 0 < want[0] < 6, (mb, chunks, want)
    monkeypatch.setenv("GPC_MEM_BUDGET_MB", "1")
    with pytest.raises(RuntimeError, match=r"gpc_cv.*rc=-2.*N_pad = 384, F = 3, k_max = 100.*budget"):
        gp._post_handle.cv(folds)
    monkeypatch.delenv("GPC_MEM_BUDGET_MB")


def test_other_posterior_origins():
    from test_gpu_user_kernel import PySquaredExponential, _mk

    gp, model, X, y, s2, hyp = _fit(N=200, S=2)
    folds = scattered_folds(200, [1, 15, 65])
    user = _mk(PySquaredExponential(), 3)
    user.update(X_new=X, y_new=y, hyp=hyp)
    for fl in (None, folds):
        check_against(_device(gp, fl), _device(user, fl), fl, 200, "python kernel")
    # after a block append of 5 points and a one-point append: against a freshly recomputed posterior
    rng = np.random.default_rng(4)
    Xn = rng.uniform(-2, 2, (6, 3))
    yn = np.sin(Xn.sum(1, keepdims=True))
    gp.update(X_new=Xn[:5], y_new=yn[:5], block_append=True)
    gp.update(X_new=Xn[5:], y_new=yn[5:])
    fresh = _gp(model, 3)
    fresh.update(X_new=np.vstack([X, Xn]), y_new=np.vstack([y, yn]), hyp=hyp)
    folds = folds + [np.array([200, 201, 203, 205])]  # (a fold of appended points)
    for fl in (None, folds):
        check_against(_device(fresh, fl), _device(gp, fl), fl, 206, "appended")


def test_consistency_with_loo_lpd_and_the_gps_own_refit():
    gp, model, X, y, s2, hyp = _fit(N=200, S=3)
    mu, v, lpd, lpf = gp.cv_predict(None, add_noise=True, separate_samples=True, return_lpd=True)
    assert np.allclose(lpf, lpd, rtol=1e-11, atol=0)  # each fold of leave-one-out is its point
    _engine(gp, 1)
    one = gp.cv_predict([[17], [4, 9]], add_noise=True, separate_samples=True, return_lpd=True)  # the fold path, k = 1
    assert np.allclose(one[0][17], mu[17], rtol=1e-11) and np.allclose(one[1][17], v[17], rtol=1e-11)
    assert np.allclose(one[3][0], lpf[17], rtol=1e-11)
    _engine(gp, 0)
    halves = [np.arange(0, 200, 2), np.arange(1, 200, 2)]
    m2, v2 = gp.cv_predict(halves, add_noise=True, separate_samples=True)
    for I, J in (halves, halves[::-1]):
        ref = _gp(model, 3)
        ref.update(X_new=X[J], y_new=y[J], hyp=hyp)
        mr, vr = ref.predict(X[I], add_noise=True, separate_samples=True)
        assert np.abs(m2[I] - mr).max() <= 1e-8 * np.abs(mr).max()
        assert (np.abs(v2[I] - vr) / vr).max() <= 1e-8
    # the mixture, the latent variance and predict's lpd conventions on the whole path
    m, s = gp.cv_predict(halves)
    assert m.shape == s.shape == (200, 1) and np.all(s >= 0)
    lat = gp.cv_predict(halves, separate_samples=True)[1]
    sn2 = np.exp(2 * hyp[:, 4])[None, :]
    assert np.allclose(lat, np.maximum(v2 - sn2, 0), rtol=1e-13)


def test_refusals():
    gp, model, X, y, s2, hyp = _fit(N=40, D=2, S=2)
    h = gp._post_handle
    i32 = lambda *a: np.array(a, dtype=np.int32)
    for folds, msg in (([i32(1, 40)], r"fold 0 has index 40 out of range \[0, 40\)"), ([i32(3), i32(-1)], "fold 1 has index -1 out of range"),
                       ([i32(2, 1)], "fold 0 is unsorted"), ([i32(2, 2)], "fold 0 is unsorted"),
                       ([i32(1, 2), i32(2, 3)], "fold 1 overlaps fold 0 at index 2"), ([i32(1), i32()], "fold 1 is empty"),
                       ([np.arange(40, dtype=np.int32)], "fold 0 holds all 40 points")):
        with pytest.raises(RuntimeError, match=r"gpc_cv.*rc=-2.*" + msg):
            h.cv(folds)
    with pytest.raises(ValueError, match="fold 1 overlaps fold 0"):
        gp.cv_predict([[1, 2], [2, 3]])
    # a posterior with a failed factorization
    from gpyreg_amd import _lib

    ctx = gp._ctx()
    K = -1e12 * np.eye(40)[None]
    bad, mult, lchol, info = ctx.posterior_batch_K(_lib.F64, K, np.zeros((1, 40)), np.full((1, 1), 1e-2), False)
    try:
        assert info[0] != 0
        with pytest.raises(RuntimeError, match="gpc_cv: posterior contains a failed factorization"):
            bad.cv(None)
    finally:
        bad.free()
    gp.clean()
    with pytest.raises(ValueError, match="posteriors have been cleaned"):
        gp.cv_predict()


# ---- sharding: the pattern of test_gpu_quad_mixture.py's two-rank test


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      GPYREG_AMD_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist

    import gpyreg_amd as gpr

    from test_cv_cpu import cv_data, scattered_folds

    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    try:
        for S in (1, 5):
            model, X, y, _, hyp = cv_data(N=200, S=S)

            def make():
                return gpr.GP(3, gpr.covariance_functions.SquaredExponential(), gpr.mean_functions.ConstantMean(),
                              gpr.noise_functions.GaussianNoise(constant_add=True))

            ref = make()
            ref.shard = False
            ref.update(X_new=X, y_new=y, hyp=hyp)
            gp = make()
            gp.update(X_new=X, y_new=y, hyp=hyp)
            ok = {}
            for name, folds in (("loo", None), ("folds", scattered_folds(200, [1, 15, 65]))):
                for sep in (True, False):
                    a = ref.cv_predict(folds, separate_samples=sep, return_lpd=True)
                    b = gp.cv_predict(folds, separate_samples=sep, return_lpd=True)
                    ok[f"{name} {sep}"] = all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))
            out[S] = ok
    except Exception as e:  # noqa: BLE001 - reported to the parent
        out["exception"] = repr(e)
    finally:
        dist.destroy_process_group()
    q.put((rank, out))


def test_sharded_cv_predict_equals_unsharded_bitwise_two_ranks_one_gpu():
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
        for S in (1, 5):
            assert all(r[S].values()), (rank, S, r[S])
