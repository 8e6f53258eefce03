"""gpc_predict, gpc_predict_full, gpc_quad and gpc_predict_K -- the four calls that go through rhs_products / RhsCall
of gpcore.hip -- against the 80-bit reference of tests/rhs_ref.py, per sample and per output, at the shapes where the
engine changes path (tests/rhs_ref.py: SHAPES), for both posterior forms in one batch (L_chol runs [1], [0, 0], [1],
[0]) and both storage types; then the invariants the engine's comments promise, to the bit: batch = single, chunked =
whole, polled = stream-waited completion, and columns that do not couple.

Every error is stated in the unit eps_T cond_2(K_s + sn2_s I) max |reference| of that output and sample: the device
builds its own K to an ulp or two per entry, which alone moves the answer by about one unit."""

import numpy as np
import pytest

import rhs_ref as rr
from scratch_sizes import budget_for_chunk, pad, planned_chunk, rhs_per, rhs_shared

pytestmark = pytest.mark.gpu

F64, F32 = 0, 1
KID = {"se": (0, 0), "matern5": (1, 5), "rq": (2, 0)}
EPS = {F64: float(np.finfo(np.float64).eps), F32: float(np.finfo(np.float32).eps)}
# the project's contract for these calls (test_gpu_full.py, test_gpu_core_abi.py), relative to max |reference|
CONTRACT = {F64: 1e-8, F32: 1e-3}
# The tight bound: err <= C_TIGHT eps_T cond_2(A_s) max |reference|, never beyond the contract.  The device carries an
# explicit inverse, not a solve, and sums up to 384 terms per column: each is worth a small factor over the unit.
# Worst err / (eps_T cond scale) measured on the MI355X, per (call, form, dtype) over all outputs and cases below:
#                        fp64 L_chol   fp64 low-noise   fp32 L_chol   fp32 low-noise
#   predict                 16.2           0.60            0.28           0.48
#   predict_full            16.2           0.63            0.36           0.48
#   quad                     7.6           5.6             1.25           0.53
#   predict_K (3 forms)      0.55          0.72            0.65           0.64
# Every ratio above 1 belongs to N <= 2, where cond = 1, and every one above 4 to (N, M) = (1, 1): the whole output is
# ONE far-tail kernel value (fmu = k(x*, X) alpha with r2 / 2 = 26 .. 30, or one z), so `scale` is that value, and a
# kernel value carries the rounding of its exponent's argument, |arg| eps relative (the bound of
# test_cov_functors_cpu.py: tile_r2_ab forms r2 from the fp64 scaled coordinates, pair_eval_t takes exp(-r2 / 2)).  The
# oracle's own fp64 value of that entry is 0.2 .. 21 eps from the 80-bit one; predict_K, which is handed the oracle's Ks,
# shows none of it.  With N >= 100 no ratio exceeds 0.75.  The start value 8 was too small for (1, 1) alone: the next
# power of two above twice the worst ratio (2 x 16.2) is 64.
C_TIGHT = 64.0


@pytest.fixture(scope="module")
def ctx():
    from gpyreg_amd import _lib

    yield _lib.context(0)
    for key in sorted(WORST):  # (under -s) the worst err / (eps cond scale) per (call, output, form, dtype) of this run
        print("WORST %-14s %-4s %-9s %s  %.3g" % (key + (WORST[key],)))


class Device:
    """The device posteriors of one case: `h` from the device kernel, `hk` from NumPy's K (gpc_posterior_batch_K), for
    the hyperparameter rows `rows` (default: the whole mixed batch)."""

    def __init__(self, ctx, ref, dtype, rows=None):
        p = ref["problem"]
        self.ctx, self.ref, self.p, self.dtype = ctx, ref, p, dtype
        self.rows = list(range(rr.S)) if rows is None else list(rows)
        kid, deg = KID[p["kernel"]]
        N = p["N"]
        ctx.set_data(p["X"], p["y"])
        m = np.repeat(p["m0"][self.rows, None], N, axis=1)
        sn2 = p["sn2"][self.rows, None]
        self.h = self.hk = None
        self.h, mult, lchol, info = ctx.posterior_batch(kid, deg, dtype, p["hyp_cov"][self.rows], m, sn2, False)
        want_lchol = [rr.LCHOL[s] for s in self.rows]
        assert np.all(info == 0) and np.all(mult == 1) and list(lchol) == want_lchol, (info, mult, lchol)
        self.hk, mult, lchol, info = ctx.posterior_batch_K(dtype, ref["K"][self.rows], m, sn2, False)
        assert np.all(info == 0) and np.all(mult == 1) and list(lchol) == want_lchol, (info, mult, lchol)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for h in (self.h, self.hk):
            if h is not None:
                h.free()

    def calls(self, M=None, which=None):
        """{call: tuple of outputs} for the first M queries / measures (default all), every output (M, S) or
        (S, M, M).  `which`: a subset of the call names."""
        p, ref = self.p, self.ref
        M = p["M"] if M is None else M
        xs, Ks, Kss = p["xs"][:M], ref["Ks"][self.rows][:, :, :M], ref["Kss"][self.rows][:, :M, :M]
        todo = {
            "predict": lambda: self.h.predict(xs),
            "predict_full": lambda: self.h.predict_full(xs),
            "predict_K": lambda: self.hk.predict_K(Ks)[:2],
            "predict_K+Kss": lambda: self.hk.predict_K(Ks, Kss),
            "predict_K-var": lambda: self.hk.predict_K(Ks, Kss, want_var=False)[::2],
        }
        if p["kernel"] == "se":
            todo["quad"] = lambda: self.h.quad(p["mu"][:M], p["sigma"][:M], True)
            todo["quad-var"] = lambda: self.h.quad(p["mu"][:M], p["sigma"][:M], False)[:1]
        return {k: f() for k, f in todo.items() if which is None or k in which}


# which reference array each output of each call is compared with
OUTPUTS = {
    "predict": ("fmu", "fs2"),
    "predict_full": ("fmu", "C"),
    "quad": ("za", "zkz"),
    "quad-var": ("za",),
    "predict_K": ("fmu", "fq"),
    "predict_K+Kss": ("fmu", "fq", "C"),
    "predict_K-var": ("fmu", "C"),
}
WORST = {}


def _sample(a, s):
    return a[s] if a.ndim == 3 else a[:, s]


def _check(case, dtype, call, out, got, want, cond):
    """Every sample of one output against the reference at both bounds; returns nothing, records the worst ratio."""
    assert got.shape == want.shape and np.all(np.isfinite(got)), (case, call, out)
    for s in range(rr.S):
        g, w = _sample(got, s), _sample(want, s)
        scale = float(np.abs(w).max())
        err = float(np.abs(g.astype(rr.LD) - w).max())
        ratio = err / (EPS[dtype] * cond[s] * scale)
        key = (call, out, "L_chol" if rr.LCHOL[s] else "low-noise", "fp64" if dtype == F64 else "fp32")
        WORST[key] = max(WORST.get(key, 0.0), ratio)
        print("RATIO %-14s %-4s %-9s %s %s s=%d cond=%.3g err/scale=%.3g ratio=%.3g" % (key + (case, s, cond[s], err / scale, ratio)))
        assert err <= CONTRACT[dtype] * scale, ("contract", case, call, out, s, err / scale)
        assert err <= min(C_TIGHT * EPS[dtype] * cond[s], CONTRACT[dtype]) * scale, ("tight", case, call, out, s, ratio)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("case", rr.CASES, ids=lambda c: "%s-%d-%d" % c)
def test_every_output_against_the_80_bit_reference(ctx, case, dtype):
    """predict, predict_full, quad (with and without compute_var) and predict_K (with and without Kss, with and without
    want_var) of the mixed batch, per sample, within the contract (1e-8 / 1e-3 of the largest reference entry) and within
    C_TIGHT eps cond of it; the full covariance symmetric and its diagonal equal to predict's variance within the same."""
    ref = rr.reference(*case)
    cond = ref["cond"]
    with Device(ctx, ref, dtype) as dev:
        res = dev.calls()
    assert set(res) == {c for c in OUTPUTS if case[0] == "se" or not c.startswith("quad")}
    for call, outs in res.items():
        assert len(outs) == len(OUTPUTS[call])
        for name, got in zip(OUTPUTS[call], outs):
            _check(case, dtype, call, name, got, ref[name], cond)
    # what the variants of one call share comes back the same whatever else is asked for
    assert np.array_equal(res["predict"][0], res["predict_full"][0])
    assert np.array_equal(res["predict_K"][0], res["predict_K+Kss"][0]) and np.array_equal(res["predict_K"][1], res["predict_K+Kss"][1])
    assert np.array_equal(res["predict_K+Kss"][2], res["predict_K-var"][1])
    if "quad" in res:
        assert np.array_equal(res["quad"][0], res["quad-var"][0])
    fs2 = res["predict"][1]
    for call, C in (("predict_full", res["predict_full"][1]), ("predict_K+Kss", res["predict_K+Kss"][2])):
        for s in range(rr.S):
            scale = float(np.abs(ref["C"][s]).max())
            tight = min(C_TIGHT * EPS[dtype] * cond[s], CONTRACT[dtype]) * scale
            asym = np.abs(C[s] - C[s].T).max()
            dg = np.abs(np.diag(C[s]) - fs2[:, s]).max()
            print("SYMM %s %s s=%d |C - C^T|/scale=%.3g |diag C - fs2|/scale=%.3g" % (call, case, s, asym / scale, dg / scale))
            # (each side is within `tight` of the reference, which is symmetric and whose diagonal is fs2)
            assert asym <= 2 * tight and dg <= 2 * tight, (call, case, s, asym, dg, tight)


# ---- bit for bit -----------------------------------------------------------------------------------------------------


def _same(a, b, what):
    assert set(a) == set(b)
    for call in a:
        for name, x, y in zip(OUTPUTS[call], a[call], b[call]):
            assert np.array_equal(x, y), (what, call, name, np.abs(x - y).max())


@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("N,M", rr.BIG)
def test_batch_equals_single(ctx, N, M, dtype):
    """Every sample of the mixed batch carries the bits of its own single-sample posterior, in all four calls."""
    ref = rr.reference("se", N, M)
    with Device(ctx, ref, dtype) as dev:
        batch = dev.calls()
    for s in range(rr.S):
        with Device(ctx, ref, dtype, rows=[s]) as dev:
            one = dev.calls()
        _same(one, {c: tuple(o[s:s + 1] if o.ndim == 3 else o[:, s:s + 1] for o in outs) for c, outs in batch.items()},
              ("sample", s))


@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
def test_chunked_equals_whole(ctx, monkeypatch, dtype):
    """GPC_MEM_BUDGET_MB chosen from the scratch's closed forms (scratch_sizes.rhs_per, rhs_shared) so that two samples fit: chunks
    of 2, 2 and 1 -- the partial last chunk (RhsCall::download's two-copy branch), constants that are not resident and
    L_chol runs cut at the chunk borders -- give the bits of the call that holds all five."""
    N, M = 300, 300
    ref = rr.reference("se", N, M)
    w = 8 if dtype == F64 else 4
    with Device(ctx, ref, dtype) as dev:
        whole = dev.calls()
        assert ctx.get_option("last_chunk") == rr.S
        for call in whole:
            kind = "given" if call.startswith("predict_K") else "quad" if call.startswith("quad") else "cross"
            full, want_quad = call in ("predict_full", "predict_K+Kss", "predict_K-var"), call in ("predict", "quad", "predict_K", "predict_K+Kss")
            per = rhs_per(pad(N), pad(M), full, w, rr.D, kind, want_quad)
            shared = rhs_shared(N, M, rr.D, rr.S, kind, full)
            mb = budget_for_chunk(rr.S, 2, per, shared)
            assert mb is not None and planned_chunk(rr.S, mb, per, shared) == 2
            monkeypatch.setenv("GPC_MEM_BUDGET_MB", str(mb))
            part = dev.calls(which=(call,))
            chunk = ctx.get_option("last_chunk")
            monkeypatch.delenv("GPC_MEM_BUDGET_MB")
            assert chunk == 2, (call, mb, chunk)
            _same(part, {call: whole[call]}, ("budget", mb))


@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
def test_polled_equals_stream_waited(ctx, dtype):
    """small_poll 1 against 0: the same bits, and the completion counters move as the `poll` condition of
    RhsCall::chunk_steps says -- a call without the full covariance whose one chunk holds all samples ends on the polled
    word (small_polled, or small_synced when the word was not seen in time); predict_full never does, and nothing
    does with small_poll = 0."""
    ref = rr.reference("se", 129, 129)
    eligible = {"predict", "quad", "quad-var", "predict_K"}

    def count():
        return ctx.get_option("small_polled") + ctx.get_option("small_synced")

    before = ctx.get_option("small_poll")
    try:
        with Device(ctx, ref, dtype) as dev:
            res = {}
            for poll in (1, 0):
                ctx.set_option("small_poll", poll)
                res[poll] = {}
                for call in OUTPUTS:
                    c0 = count()
                    res[poll].update(dev.calls(which=(call,)))
                    assert count() - c0 == (1 if poll and call in eligible else 0), (call, poll)
            _same(res[1], res[0], "small_poll")
    finally:
        ctx.set_option("small_poll", before)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("N,M,M1,M2", [(128, 128, 65, 128), (300, 300, 129, 200)])
def test_columns_do_not_couple(ctx, N, M, M1, M2, dtype):
    """Within one padded width the results for xs[:M1] are the prefix of the results for xs[:M2]: every step works per
    column in an order fixed by the padded shape."""
    assert pad(M1) == pad(M2)
    ref = rr.reference("se", N, M)
    with Device(ctx, ref, dtype) as dev:
        a, b = dev.calls(M=M1), dev.calls(M=M2)
    _same(a, {c: tuple(o[:, :M1, :M1] if o.ndim == 3 else o[:M1] for o in outs) for c, outs in b.items()}, (M1, M2))


def test_quad_refuses_a_failed_factorization(ctx):
    """A batch that holds a failed factorization (K - 1e12 I is not positive definite at any jitter multiplier:
    info != 0) is refused by gpc_quad as by every other posterior consumer."""
    rng = np.random.default_rng(1)
    X = rng.uniform(-1, 1, (40, 2))
    ctx.set_data(X, np.sin(X[:, :1]))
    handle, mult, lchol, info = ctx.posterior_batch(0, 0, F64, np.zeros((2, 3)), np.zeros((2, 40)),
                                                    np.array([[1e-2], [-1e12]]), False)
    try:
        assert info[0] == 0 and info[1] != 0
        for var in (False, True):
            with pytest.raises(RuntimeError, match="gpc_quad: posterior contains a failed factorization"):
                handle.quad(np.zeros((3, 2)), np.ones((3, 2)), var)
    finally:
        handle.free()
