"""GP.lookahead_batch / gpc_lookahead_batch on the device: against the NumPy restatement (gpyreg_amd/_lookahead_batch.py)
on the GP's own fetched posteriors in both precisions and both parametrisations, against lookahead_variance at step 0,
against the host loop it replaces (lookahead_variance, argmax, update), exhaustion and ties, bitwise determinism over
repeats and over the chunking of the formation, the budget refusal, denominators <= 0, and the bits of the neighbouring
entry points.

Shapes (Mr, Mc, q): (70, 150, 12) -- two row slabs of 64, the second partial, three column blocks of 64 in a padded
width of 256; (300, 150, 12) -- five slabs; (5, 129, 8) -- one partial slab, a candidate count one past a tile."""

import copy
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_lookahead import _err, _points, _problem
from test_lookahead_batch_cpu import restated_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(70, 150, 12), (300, 150, 12), (5, 129, 8)]
KERNELS = [("se", 0, "const", False), ("se_iso", 0, "negquad", False), ("matern", 3, "const", True),
           ("matern", 5, "negquad", False), ("rq", 0, "const", False)]
MIXED = dict(kernel="se", lo=-6.0, hi=6.0, sn2s=(1e-2, 1e-7, 1e-7, 1e-2), seed=11)  # well-spread inputs: see test 3
MIN_GAP = 1e-5


def weight_cases(Mr, S):
    rng = np.random.default_rng(3)
    return [None, rng.uniform(0, 1, Mr), rng.uniform(0, 1, (Mr, S))]


def gaps(scores):
    """Relative gap between the best and the second-best score of every step that had a choice."""
    out = []
    for row in scores:
        f = np.sort(row[np.isfinite(row)])[::-1]
        if f.size >= 2:
            out.append((f[0] - f[1]) / abs(f[0]))
    return np.array(out)


def _restated(gp, model, X, xr, xc, w, q, s2_cand=None, replay=None):
    from gpyreg_amd._lookahead_batch import greedy_batch

    args = restated_inputs(model, list(gp.posteriors), X, xr, xc, weights=w, s2_cand=s2_cand)
    return greedy_batch(*args, q, replay=replay, return_scores=True)


def _check_fp64(gp, model, X, xr, xc, q, s2_cand=None, tag=""):
    """Test 1's assertions for the three kinds of weights: the restatement's selection is decided by at least MIN_GAP
    at every step (asserted on the restatement alone), the device picks the same candidates, gains within 1e-8 of
    gain[0]."""
    S = gp.posteriors.size
    for w in weight_cases(xr.shape[0], S):
        ref_idx, ref_gain, scores = _restated(gp, model, X, xr, xc, w, q, s2_cand)
        g = gaps(scores)
        print(tag, xr.shape[0], xc.shape[0], q, "weights", None if w is None else w.shape, "smallest gap", g.min())
        assert g.min() >= MIN_GAP
        idx, gain = gp.lookahead_batch(xc, xr, q, weights=w, s2_cand=s2_cand, separate_samples=True)
        assert idx.shape == (q,) and gain.shape == (q, S) and len(set(idx.tolist())) == q
        err = np.abs(gain - ref_gain).max() / np.abs(ref_gain[0]).max()
        print(tag, "idx equal", np.array_equal(idx, ref_idx), "gain error / gain[0]", err)
        assert np.array_equal(idx, ref_idx)
        assert err <= 1e-8
        m_idx, m_gain = gp.lookahead_batch(xc, xr, q, weights=w, s2_cand=s2_cand)
        assert np.array_equal(m_idx, idx) and m_gain.shape == (q, 1)
        assert np.allclose(m_gain[:, 0], gain.mean(1), rtol=1e-14, atol=0)


# ---- 1. parity with the restatement, fp64


@pytest.mark.parametrize("Mr,Mc,q", SHAPES)
@pytest.mark.parametrize("kernel,degree,mean,s2", KERNELS)
def test_parity_with_the_restatement(kernel, degree, mean, s2, Mr, Mc, q):
    gp, model, X, hyp = _problem(kernel, degree, mean, s2=s2)
    xr, xc = _points(3, Mr, Mc)
    s2c = 0.02 * np.ones((Mc, 1)) if s2 else None
    _check_fp64(gp, model, X, xr, xc, q, s2c, tag=f"{kernel}{degree}")


# ---- 2. fp32 posteriors


@pytest.mark.parametrize("Mr,Mc,q", SHAPES)
@pytest.mark.parametrize("kernel,degree", [("se", 0), ("matern", 5)])
def test_fp32_posteriors(kernel, degree, Mr, Mc, q):
    """The products that form C^0 run in fp32, the step loop in fp64.  No index equality: the device's selection is
    replayed through the restatement (on the fetched fp32 posteriors); every chosen candidate's restated score is within
    1e-3, relative, of the restated maximum of its step, and the gains agree with the replay's within 1e-3 of their
    largest entry (the fp32 figure of the project's parity tests)."""
    gp, model, X, hyp = _problem(kernel, degree, dtype="f32")
    xr, xc = _points(3, Mr, Mc)
    w = weight_cases(Mr, hyp.shape[0])[2]
    idx, gain = gp.lookahead_batch(xc, xr, q, weights=w, separate_samples=True)
    assert len(set(idx.tolist())) == q and idx.min() >= 0 and idx.max() < Mc
    _, ref_gain, scores = _restated(gp, model, X, xr, xc, w, q, replay=idx)
    short = np.array([(scores[t].max() - scores[t, idx[t]]) / abs(scores[t].max()) for t in range(q)])
    print(kernel, Mr, Mc, "fp32: largest shortfall of a chosen score", short.max(), "gain error", _err(gain, ref_gain))
    assert short.max() <= 1e-3
    assert _err(gain, ref_gain) <= 1e-3


# ---- 3. low-noise and mixed parametrisations


@pytest.mark.parametrize("Mr,Mc,q", SHAPES)
def test_low_noise_and_mixed_batches(Mr, Mc, q):
    """sn2 = (1e-2, 1e-7, 1e-7, 1e-2): L_chol samples around two low-noise ones (runs of the formation at nonzero sample
    offsets).  The 200 inputs are spread over [-6, 6]^3, about as far apart as the 40 of test_gpu_lookahead.py's
    test_low_noise_and_mixed_batches are in [-3, 3]^3: the low-noise factor -(K + Sigma)^-1 then has moderate entries
    and the cross product does not cancel its way out of the fp64 parity figure."""
    gp, model, X, hyp = _problem(**MIXED)
    assert [bool(p.L_chol) for p in gp.posteriors] == [True, False, False, True]
    xr, xc = _points(3, Mr, Mc)
    _check_fp64(gp, model, X, xr, xc, q, tag="mixed")


# ---- 4. step 0 is lookahead_variance


@pytest.mark.parametrize("Mr,Mc", [(70, 150), (300, 150), (5, 129)])
def test_step_zero_is_lookahead_variance(Mr, Mc):
    gp, model, X, hyp = _problem("matern", 5)
    xr, xc = _points(3, Mr, Mc)
    S = hyp.shape[0]
    for w in weight_cases(Mr, S):
        R = gp.lookahead_variance(xc, xr, weights=w, separate_samples=True)
        score = np.zeros(Mc)
        for s in range(S):
            score = score + R[:, s]
        idx, gain = gp.lookahead_batch(xc, xr, 3, weights=w, separate_samples=True)
        err = np.abs(gain[0] - R[idx[0]]).max() / np.abs(R[idx[0]]).max()
        print("step 0 against lookahead_variance", Mr, Mc, err)
        assert idx[0] == np.argmax(score / S)
        assert err <= 1e-12


# ---- 5. the host loop it replaces


def test_identity_through_update():
    """q = 4, Mr = 40, Mc = 6: lookahead_variance, masked argmax and update (target 0.7) on a deep copy reproduce idx and,
    within 1e-8 of gain[0], gain; the GP that lookahead_batch was called on predicts the same bits afterwards."""
    gp, model, X, hyp = _problem("se")
    S = hyp.shape[0]
    xr, xc = _points(3, 40, 6)
    assert all(p.sn2_mult == 1 for p in gp.posteriors)
    for w in weight_cases(40, S):
        before = gp.predict(xr, separate_samples=True)
        idx, gain = gp.lookahead_batch(xc, xr, 4, weights=w, separate_samples=True)
        after = gp.predict(xr, separate_samples=True)
        assert all(np.array_equal(b, a) for b, a in zip(before, after)) and gp.X.shape[0] == X.shape[0]
        g2 = copy.deepcopy(gp)
        chosen = []
        for t in range(4):
            R = g2.lookahead_variance(xc, xr, weights=w, separate_samples=True)
            score = R.mean(1)
            score[chosen] = -np.inf
            c = int(np.argmax(score))
            err = np.abs(R[c] - gain[t]).max() / np.abs(gain[0]).max()
            print("host loop step", t, "choice", c, idx[t], "gain error / gain[0]", err)
            assert c == idx[t]
            assert err <= 1e-8
            chosen.append(c)
            g2.update(X_new=xc[c:c + 1], y_new=np.array([[0.7]]))
            assert g2.X.shape[0] == X.shape[0] + t + 1 and all(p.sn2_mult == 1 for p in g2.posteriors)


# ---- 6. exhaustion and exclusion


def test_exhaustion_and_identical_candidates():
    gp, model, X, hyp = _problem("matern", 5)
    xr, xc = _points(3, 40, 5)
    idx, gain = gp.lookahead_batch(xc, xr, 5, separate_samples=True)
    assert sorted(idx.tolist()) == list(range(5)) and np.all(np.isfinite(gain))
    xc = xc.copy()
    xc[3] = xc[1]  # the same point twice: the same scores to the bit until one of them is chosen
    idx, gain = gp.lookahead_batch(xc, xr, 5, separate_samples=True)
    order = idx.tolist()
    assert sorted(order) == list(range(5))
    assert order.index(1) < order.index(3)
    # ... and with fewer steps than candidates the twin is still a candidate: it is picked or left on its merits
    R = gp.lookahead_variance(xc, xr, separate_samples=True)
    assert np.array_equal(R[1], R[3])
    xc2 = np.vstack([xc[1:2], xc[1:2]])
    idx2, gain2 = gp.lookahead_batch(xc2, xr, 2, separate_samples=True)
    assert idx2.tolist() == [0, 1] and np.all(gain2[1] < gain2[0]) and np.all(gain2[1] > 0)


# ---- 7. determinism, chunked formation, the budget refusal

_CHILD = """
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
from test_gpu_lookahead import _points, _problem
from test_gpu_lookahead_batch import MIXED
from gpyreg_amd import _lib
gp, model, X, hyp = _problem(**MIXED)
xr, xc = _points(3, 70, 150)
w = np.random.default_rng(2).uniform(0, 1, (70, 4))
out = {{}}
for mb in ("4", "8"):
    os.environ["GPC_MEM_BUDGET_MB"] = mb
    idx, gain = gp.lookahead_batch(xc, xr, 12, weights=w, separate_samples=True)
    print("LAST_CHUNK", mb, _lib.context(gp.device).get_option("last_chunk"))
    out["idx" + mb], out["gain" + mb] = idx, gain
os.environ["GPC_MEM_BUDGET_MB"] = "1"
try:
    gp.lookahead_batch(xc, xr, 12, weights=w)
    print("NOT REFUSED")
except RuntimeError as e:
    print("REFUSED", e)
np.savez(sys.argv[1], **out)
"""


def test_repeats_chunked_formation_and_the_budget_refusal(tmp_path):
    """Two calls give the same bits.  In a child process GPC_MEM_BUDGET_MB = 4 and 8 hold the resident state (2 MB at
    S = 4, Mr = 70, Mc_pad = 256, q = 12) and one or two samples of the formation's scratch (2.6 MB each; the planner takes
    80 %): the formation runs in chunks, with the bits of the unchunked call.  1 MB does not hold the resident state:
    refused, the sizes in the message."""
    gp, model, X, hyp = _problem(**MIXED)
    xr, xc = _points(3, 70, 150)
    w = np.random.default_rng(2).uniform(0, 1, (70, 4))
    idx, gain = gp.lookahead_batch(xc, xr, 12, weights=w, separate_samples=True)
    idx2, gain2 = gp.lookahead_batch(xc, xr, 12, weights=w, separate_samples=True)
    assert np.array_equal(idx, idx2) and np.array_equal(gain, gain2)
    g2 = copy.deepcopy(gp)
    idx3, gain3 = g2.lookahead_batch(xc, xr, 12, weights=w, separate_samples=True)
    assert np.array_equal(idx, idx3) and np.array_equal(gain, gain3)
    script = tmp_path / "child.py"
    script.write_text(_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests")))
    out = tmp_path / "chunked.npz"
    env = {k: v for k, v in os.environ.items() if k != "GPC_MEM_BUDGET_MB"}
    r = subprocess.run([sys.executable, str(script), str(out)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "LAST_CHUNK 4 1\n" in r.stdout and "LAST_CHUNK 8 2\n" in r.stdout, r.stdout
    z = np.load(out)
    for mb in ("4", "8"):
        assert np.array_equal(z["idx" + mb], idx) and np.array_equal(z["gain" + mb], gain), mb
    assert "REFUSED" in r.stdout and "NOT REFUSED" not in r.stdout, r.stdout
    msg = r.stdout[r.stdout.index("REFUSED"):]
    assert "gpc_lookahead_batch: the resident state" in msg and "exceeds the device memory budget" in msg
    assert "S = 4" in msg and "Mr = 70" in msg and "Mc_pad = 256" in msg and "q = 12" in msg


# ---- 8. denominators <= 0


def test_nonpositive_denominators():
    """The ABI takes the candidates' noise as an array: lowering it below -max(v, 0) gives den <= 0, the way test_edge_cases
    lowers the variance and takes the noise away.  The candidate `a` that the plain run picks first gets den <= 0 under
    sample 0 only: it still wins step 0 through the other samples, gains 0 under sample 0 and leaves that sample's state
    alone (the next gain of sample 0 is the unconditioned one, well above the plain run's).  The candidate `z` that the
    plain run picks last gets den <= 0 under every sample: score 0, chosen last.  Parity with the restatement on the
    same noise."""
    from gpyreg_amd._lookahead_batch import greedy_batch

    gp, model, X, hyp = _problem("matern", 5, noise_sd=0.01)
    xr, xc = _points(3, 40, 6)
    C0, v0, noise, w = restated_inputs(model, list(gp.posteriors), X, xr, xc)
    plain_idx, plain_gain = greedy_batch(C0, v0, noise, w, 6)
    a, z = plain_idx[0], plain_idx[-1]
    noise = noise.copy()
    noise[a, 0] = -np.maximum(v0[a, 0], 0) - 1.0
    noise[z, :] = -np.maximum(v0[z, :], 0) - 1.0
    ref_idx, ref_gain, scores = greedy_batch(C0, v0, noise, w, 6, return_scores=True)
    assert gaps(scores).min() >= MIN_GAP
    assert ref_idx[0] == a and ref_gain[0, 0] == 0 and ref_idx[-1] == z and np.all(ref_gain[-1] == 0)
    # sample 0 was not conditioned on `a`: its next gain is the unconditioned one, 1e-3 of gain[0] away from the plain
    # run's -- a device that applied the downdate all the same would miss the parity bound below by five orders
    assert ref_idx[1] == plain_idx[1] and ref_gain[1, 0] - plain_gain[1, 0] > 1e-4 * ref_gain[0].max()
    idx, gain = gp._post_handle.lookahead_batch(xr, xc, 6, w, noise)
    assert np.array_equal(idx, ref_idx)
    assert gain[0, 0] == 0 and np.all(gain[-1] == 0)
    assert np.all(np.isfinite(gain))
    err = np.abs(gain - ref_gain).max() / np.abs(ref_gain[0]).max()
    print("den <= 0: gain error / gain[0]", err)
    assert err <= 1e-8


# ---- 9. the neighbouring entry points keep their bits; refusals on the device path


def test_predict_cov_and_lookahead_variance_keep_their_bits():
    gp, model, X, hyp = _problem("se", N=300, D=4, S=4, seed=4)
    xr, xc = _points(4, 300, 200)
    before = gp.predict_cov(xr, xc), gp.lookahead_variance(xc, xr, separate_samples=True), gp.predict(xc, separate_samples=True)
    gp.lookahead_batch(xc, xr, 5)
    after = gp.predict_cov(xr, xc), gp.lookahead_variance(xc, xr, separate_samples=True), gp.predict(xc, separate_samples=True)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert all(np.array_equal(b, a) for b, a in zip(before[2], after[2]))


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      GPYREG_AMD_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    try:
        import gpyreg_amd as gpr

        rng = np.random.default_rng(1)
        X = rng.uniform(-2, 2, (200, 3))
        y = np.sin(X.sum(1, keepdims=True)) + 0.05 * rng.standard_normal((200, 1))
        hyp = np.r_[np.log(1.2) * np.ones(3), 0.0, np.log(0.1), 0.3] + 0.05 * rng.standard_normal((5, 6))
        xr, xc = _points(3, 70, 150)
        w = rng.uniform(0, 1, (70, 5))

        def make(shard):
            gp = gpr.GP(3, gpr.covariance_functions.Matern(5), gpr.mean_functions.ConstantMean(),
                        gpr.noise_functions.GaussianNoise(constant_add=True))
            gp.shard = shard
            gp.update(X_new=X, y_new=y, hyp=hyp)
            return gp

        ref, gp = make(False), make(True)
        out["sharded"] = bool(ref._post_range is None and gp._post_range is not None)
        r_idx, r_gain = ref.lookahead_batch(xc, xr, 8, weights=w, separate_samples=True)
        # (the call exchanges nothing: the ranks need not make it together -- rank 1 makes it twice)
        for _ in range(1 + rank):
            idx, gain = gp.lookahead_batch(xc, xr, 8, weights=w, separate_samples=True)
        out["idx"] = bool(np.array_equal(idx, r_idx))
        out["gain"] = float(np.abs(gain - r_gain).max() / np.abs(r_gain[0]).max())
        out["kept"] = bool(gp._post_range is not None)
    except Exception:  # noqa: BLE001 - reported to the parent
        import traceback

        out["exception"] = traceback.format_exc()
    finally:
        dist.destroy_process_group()
    q.put((rank, out))


def test_under_a_process_group_the_call_runs_on_the_calling_rank():
    """Two ranks on one GPU, the resident posteriors sharded 3 + 2: every rank's call rebuilds all five samples as
    temporaries and returns the unsharded GP's selection, gains within 1e-8 of gain[0], without an exchange; the sharded posteriors stay as they were."""
    import torch.multiprocessing as mp

    from test_gpu_lookahead import _free_port

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
        print("rank", rank, r)
        assert r["sharded"] and r["idx"] and r["kept"] and r["gain"] <= 1e-8, (rank, r)


def test_refusals_with_data():
    gp, model, X, hyp = _problem("se")
    xr, xc = _points(3, 40, 6)
    for q in (0, 7):
        with pytest.raises(ValueError, match="q must be"):
            gp.lookahead_batch(xc, xr, q)
    with pytest.raises(ValueError, match="weights must be"):
        gp.lookahead_batch(xc, xr, 2, weights=np.ones(39))
    with pytest.raises(RuntimeError, match="bad arguments"):
        gp._post_handle.lookahead_batch(xr, xc, 7, np.ones(40), np.ones((6, 3)))
    gp.clean()
    with pytest.raises(ValueError, match="posteriors have been cleaned"):
        gp.lookahead_batch(xc, xr, 2)
