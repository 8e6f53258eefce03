"""The blocked factorization plan (plan.h: potrf_inv, potrf_nll, trsm_nll, the forward solves, lauum; leaf.h; gemm.h)
per matrix, in every mode the product runs it in, through gpc_debug_factor_plan: fast and stable mode, fp64 and fp32,
full inverse / NLL-only / blocked NLL-only with nll_block 128 and 256, keep_L on and off, batches, failed samples inside
a batch, both leaf versions and both launch forms of the small nodes.  The buffers go in NaN-poisoned (tests/factor_ref.py)
and come back whole, so the header of plan.h -- "strictly-upper tiles are never read", no launch reads what no launch
wrote -- is tested together with the arithmetic.  Expectations (a) - (f) and their bars: tests/factor_ref.py; the same
cases run through the NumPy model in tests/test_factor_plan_cpu.py, which also shows that every bar bites.

Measured on the MI355X, worst over the cases of each row (printed by test_zz_report).  rho_F as defined -- in fast mode
the row's worst is a printed-only family (neardup in fp64 and fp32); rho_F/model = the device's rho_F over the model's on
the families where fast mode asserts it (bar: 4, or rho_F <= 1); the other columns are measured / bar:

    plan    mode    dtype  rho_F        rho_F/model  rho_I        logdet       solve        ainv
    p0      fast    f32    12.3         2.52         0.0107       0.00543      0.00996      0.0724
    p0      fast    f64    9.99e+05     2.66         0.00619      0.0121       0.0136       0.109
    p0      stable  f32    0.0864       -            0.00766      0.00797      0.00864      0.0766
    p0      stable  f64    0.0875       -            0.00869      0.00749      0.0094       0.106
    p1      fast    f32    12.3         2.28         0.00598      0.0145       0.00754      -
    p1      fast    f64    6.27e+06     0.59         0.00904      0.00769      0.0137       -
    p1      stable  f32    0.0834       -            0.00627      0.0162       0.00816      -
    p1      stable  f64    0.0743       -            0.00608      0.00871      0.0131       -
    p2b128  fast    f32    12.3         2.28         0.00467      0.00448      0.00664      -
    p2b128  fast    f64    9.99e+05     0.59         0.00451      0.00509      0.00658      -
    p2b128  stable  f32    0.0633       -            0.00465      0.0162       0.00664      -
    p2b128  stable  f64    0.0722       -            0.00448      0.00519      0.00658      -
    p2b256  fast    f32    12.3         1.55         0.00727      0.00448      0.00687      -
    p2b256  fast    f64    9.99e+05     0.59         0.00474      0.00769      0.0057       -
    p2b256  stable  f32    0.0474       -            0.00528      0.00528      0.00777      -
    p2b256  stable  f64    0.0722       -            0.00501      0.00753      0.00645      -
    neardup n=300 fp64: rho_F stable 0.0668, fast 9.99e+05
    neardup n=640 fp64: rho_F stable 0.0452, fast 6.73e+06
    printed only (scaled, neardup) p0 fast f32: rho_F / model 1.76
    printed only (scaled, neardup) p0 fast f64: rho_F / model 0.178
    printed only (scaled, neardup) p1 fast f32: rho_F / model 2
    printed only (scaled, neardup) p1 fast f64: rho_F / model 0.524
    printed only (scaled, neardup) p2b128 fast f32: rho_F / model 1.62
    printed only (scaled, neardup) p2b128 fast f64: rho_F / model 0.0318
    printed only (scaled, neardup) p2b256 fast f32: rho_F / model 1.62
    printed only (scaled, neardup) p2b256 fast f64: rho_F / model 0.0318

No case exceeded 4 rho_model, and the poison found no read that the header of plan.h rules out.  One expectation was
wrong and is mended in factor_ref.ainv_check: a lower-only launch in 64-tiles leaves the upper 64 x 64 quarter of a
diagonal 128-tile unwritten, so Ainv is the lower triangle, not the lower tiles.
"""

import functools

import numpy as np
import pytest

import factor_ref as fr
from factor_ref import F32, F64

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module")
def ctx():
    from gpyreg_amd import _lib

    return _lib.context(0)


def _note(plan, blk, stable, dtype, ratios):
    key = ("p%d%s" % (plan, "b%d" % blk if plan == 2 else ""), "stable" if stable else "fast", fr.DT_NAME[dtype])
    row = WORST.setdefault(key, {})
    for k, v in ratios.items():
        if v == v:
            row[k] = max(row.get(k, 0.0), v)


def _sample(out, s):
    """Sample s of a batched result, in the form factor_ref.verify takes."""
    return dict(A=out["A"][s], W=out["W"][s], T=out["T"][s], z=None if out["z"] is None else out["z"][s],
                Ainv=None if out["Ainv"] is None else out["Ainv"][s], logdet=float(out["logdet"][s]),
                info=int(out["info"][s]))


def _run(ctx, mats, n, plan, blk, stable, keep_L, dtype, rs=None, want_inv=False):
    """One call on the poisoned, identity-padded matrices `mats` (all of order n)."""
    P = [fr.poisoned(A0) for A0 in mats]
    A, W, T = (np.stack([p[k] for p in P]) for k in range(3))
    return ctx.debug_factor_plan(A, W, T, n, plan=plan, nll_block=blk, stable=bool(stable), keep_L=bool(keep_L),
                                 want_inv=want_inv, r=None if rs is None else np.stack(rs), dtype=dtype)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else np.uint32)


def _same(a, b, what):
    for k in ("A", "W", "T", "z", "logdet", "info"):
        if a[k] is None and b[k] is None:
            continue
        x, y = np.atleast_1d(np.asarray(a[k])), np.atleast_1d(np.asarray(b[k]))
        assert np.array_equal(_bits(x), _bits(y)), "%s: %s differs" % (what, k)


def _verify(out, A0, fam, n, plan, blk, stable, keep_L, dtype, r):
    rho_model = None if stable else fr.model_rho_F(fam, n, plan, blk, stable, keep_L, dtype)
    asserted = bool(stable) or fam in fr.FAST_ASSERTED
    ratios, fails = fr.verify(out, A0, plan, blk, stable, keep_L, dtype, r=r, rho_model=rho_model, assert_fast=asserted)
    if "rho_F/model" in ratios and not asserted:
        ratios["rho_F/model (printed)"] = ratios.pop("rho_F/model")
    return ratios, fails


@pytest.mark.parametrize("case", fr.cases(), ids=fr.case_id)
def test_the_device_stays_inside_every_bar(ctx, case):
    fam, n, plan, blk, stable, keep_L, dtype = case
    A0, r = fr.matrix(fam, n, dtype), fr.rhs(n)
    out = _sample(_run(ctx, [A0], n, plan, blk, stable, keep_L, dtype, rs=[r], want_inv=plan == 0), 0)
    ratios, fails = _verify(out, A0, fam, n, plan, blk, stable, keep_L, dtype, r)
    print(fr.case_id(case), " ".join("%s %.3g" % kv for kv in ratios.items()))
    _note(plan, blk, stable, dtype, ratios)
    assert not fails, fails


BATCH_N = 300
BATCH_FAMILIES = ("gp", "scaled", "lownoise", "neardup", "extreme")


@functools.lru_cache(maxsize=None)
def _batch_inputs(dtype):
    return ([fr.matrix(f, BATCH_N, dtype) for f in BATCH_FAMILIES], [fr.rhs(BATCH_N, seed=s) for s in range(5)])


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("stable", [0, 1], ids=["fast", "stable"])
@pytest.mark.parametrize("plan,blk,keep_L", [(0, 0, 0), (0, 0, 1), (1, 0, 0), (2, 128, 0), (2, 256, 0)])
def test_a_batch_is_its_samples_one_by_one(ctx, plan, blk, keep_L, stable, dtype):
    """Five different matrices in one call (every batch stride, logdet and info slot): each sample to the bit what its
    own batch = 1 call gives, and inside the bars."""
    mats, rs = _batch_inputs(dtype)
    n = BATCH_N
    out = _run(ctx, mats, n, plan, blk, stable, keep_L, dtype, rs=rs)
    for s, fam in enumerate(BATCH_FAMILIES):
        one = _sample(_run(ctx, [mats[s]], n, plan, blk, stable, keep_L, dtype, rs=[rs[s]]), 0)
        got = _sample(out, s)
        _same(got, one, "sample %d (%s)" % (s, fam))
        ratios, fails = _verify(got, mats[s], fam, n, plan, blk, stable, keep_L, dtype, rs[s])
        _note(plan, blk, stable, dtype, ratios)
        assert not fails, (fam, fails)


@pytest.mark.parametrize("leaf", [5, 3])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("p", [0, 15, 16, 17, 127, 128, 129, BATCH_N - 1])
def test_failed_samples_inside_a_batch(ctx, p, dtype, leaf):
    """The inputs of the jitter path: samples 1 and 3 are not positive definite (A[p, p] = -1; sample 3 has a second bad
    pivot and reports the first), sample 2 has a NaN pivot.  info[s] = first bad pivot + 1 exactly, in the sample's own
    slot; the healthy samples 0 and 4 are what their single runs give, with nothing of the neighbours in them."""
    mats, rs = _batch_inputs(dtype)
    n = BATCH_N
    mats = [np.array(M) for M in mats]
    q = (p + 130) % n
    mats[1][p, p] = -1.0
    mats[3][p, p] = -1.0
    mats[3][q, q] = -1.0
    mats[2][p, p] = np.nan
    old = ctx.get_option("leaf")
    try:
        ctx.set_option("leaf", leaf)
        out = _run(ctx, mats, n, 0, 0, 0, 1, dtype, rs=rs)
        singles = {s: _sample(_run(ctx, [mats[s]], n, 0, 0, 0, 1, dtype, rs=[rs[s]]), 0) for s in (0, 4)}
    finally:
        ctx.set_option("leaf", old)
    assert list(out["info"]) == [0, p + 1, p + 1, min(p, q) + 1, 0]
    for s in (0, 4):
        got = _sample(out, s)
        _same(got, singles[s], "healthy sample %d" % s)
        assert not fr.check_layout(got, n, 0, 0, False, True)  # (finite wherever the plan writes: no NaN came over)
        assert np.isfinite(got["z"]).all() and np.isfinite(got["logdet"])


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("plan", [0, 1])
def test_launch_forms_and_leaf_versions_are_bit_identical(ctx, plan, dtype):
    """dual_launch 0 / 1 (syrk and U of a small node in one launch or two) and leaf 3 / 5 at n = 640, batch 3, fast mode."""
    n = 640
    mats = [fr.matrix(f, n, dtype) for f in ("gp", "lownoise", "extreme")]
    rs = [fr.rhs(n, seed=s) for s in range(3)]
    old = {k: ctx.get_option(k) for k in ("dual_launch", "leaf")}
    outs = {}
    try:
        for dual in (0, 1):
            for leaf in (3, 5):
                ctx.set_option("dual_launch", dual)
                ctx.set_option("leaf", leaf)
                outs[dual, leaf] = _run(ctx, mats, n, plan, 0, 0, 0, dtype, rs=rs)
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)
    base = outs[1, 5]
    assert list(base["info"]) == [0, 0, 0]
    for key, o in outs.items():
        _same(o, base, "dual_launch %d, leaf %d" % key)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("stable", [0, 1], ids=["fast", "stable"])
@pytest.mark.parametrize("plan,blk", [(0, 0), (1, 0), (2, 256)])
def test_the_plan_in_128_tiles(ctx, plan, blk, stable, dtype):
    """Every launch of the sizes above is below gemm.h's small-launch threshold and runs in 64-tiles (the deep levels of
    a production factorization); its upper levels run in 128-tiles.  With the threshold at 1 the same plan runs in
    128-tiles throughout (which also takes the dual launch away): the same bars, batch 2 at n = 640."""
    n = 640
    fams = ("gp", "neardup" if stable else "lownoise")
    mats, rs = [fr.matrix(f, n, dtype) for f in fams], [fr.rhs(n, seed=s) for s in range(2)]
    old = ctx.get_option("small_blocks")
    try:
        ctx.set_option("small_blocks", 1)
        out = _run(ctx, mats, n, plan, blk, stable, 0, dtype, rs=rs, want_inv=plan == 0)
    finally:
        ctx.set_option("small_blocks", old)
    for s, fam in enumerate(fams):
        ratios, fails = _verify(_sample(out, s), mats[s], fam, n, plan, blk, stable, 0, dtype, rs[s])
        print("128-tiles", fam, " ".join("%s %.3g" % kv for kv in ratios.items()))
        _note(plan, blk, stable, dtype, ratios)
        assert not fails, (fam, fails)


@pytest.mark.parametrize("n", [300, 640])
def test_stable_mode_really_refines(ctx, n):
    """neardup in fp64: stable mode inside Higham's bound, fast mode far outside it (the model: >= 4e4).  A stable mode
    that ran the fast arithmetic fails the first assertion; if the second fails, the family no longer separates the
    modes or fast mode is not what runs."""
    A0 = fr.matrix("neardup", n, F64)
    rho = {}
    for stable in (1, 0):
        out = _sample(_run(ctx, [A0], n, 0, 0, stable, 1, F64), 0)
        assert out["info"] == 0
        assert not fr.check_layout(out, n, 0, 0, stable, True)
        rho[stable] = fr.rho_F(A0, fr.assemble_L(out), F64)
    print("neardup n = %d: rho_F stable %.3g, fast %.3g (model, fast: %.3g)"
          % (n, rho[1], rho[0], fr.model_rho_F("neardup", n, 0, 0, 0, 1, F64)))
    WORST.setdefault(("refine", "n=%d" % n, "f64"), {}).update(stable=rho[1], fast=rho[0])
    assert rho[1] <= 1.0
    assert rho[0] > 1.0


@pytest.mark.parametrize("stable,leaf", [(0, 5), (0, 3), (1, 3)], ids=["fast-leaf5", "fast-leaf3", "stable"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_a_padded_panel_never_reaches_logdet(ctx, dtype, stable, leaf):
    """With identity padding a padded panel that was factored adds log 1 = 0 and cannot show.  The leaf skips the panels
    that start at or beyond nvalid whatever they hold: a diagonal of 4 in panel 7 (rows 112 .. 127, nvalid = 100) must
    stay out of logdet (it would add 16 log 2)."""
    n = 100
    A0 = fr.matrix("gp", n, dtype)
    A, W, T = fr.poisoned(A0)
    A[np.arange(112, 128), np.arange(112, 128)] = 4.0
    old = ctx.get_option("leaf")
    try:
        ctx.set_option("leaf", leaf)
        out = _sample(ctx.debug_factor_plan(A[None], W[None], T[None], n, stable=bool(stable), dtype=dtype), 0)
    finally:
        ctx.set_option("leaf", old)
    assert out["info"] == 0
    L = np.tril(out["A"])
    assert fr.logdet_ratio(L, n, out["logdet"]) <= 1.0


def test_refusals(ctx):
    A = np.ones((1, 128, 128))

    def call(**kw):
        a = kw.pop("A", A)
        return ctx.debug_factor_plan(a, a, a, kw.pop("nvalid", 128), **kw)

    with pytest.raises(RuntimeError, match="multiple of 128"):
        call(A=np.ones((1, 100, 100)))
    with pytest.raises(RuntimeError, match="multiple of 128"):
        call(A=np.ones((1, 2176, 2176)))
    with pytest.raises(RuntimeError, match="batch"):
        call(A=np.ones((17, 128, 128)))
    for blk in (0, 64, 192, 256):
        with pytest.raises(RuntimeError, match="nll_block"):
            call(plan=2, nll_block=blk)
    for plan in (1, 2):
        with pytest.raises(RuntimeError, match="bit 2"):
            call(plan=plan, nll_block=128, want_inv=True)
    with pytest.raises(RuntimeError, match="dtype"):
        call(dtype=7)
    with pytest.raises(RuntimeError, match="plan"):
        call(plan=3)


def test_zz_report():
    """Prints the table of the docstring (run the whole module)."""
    cols = ("rho_F", "rho_F/model", "rho_I", "logdet", "solve", "ainv")
    print("\n    plan    mode    dtype  " + "  ".join("%-11s" % c for c in cols))
    for key in sorted(k for k in WORST if k[0] != "refine"):
        row = WORST[key]
        print("    %-7s %-7s %-5s  " % key + "  ".join("%-11s" % ("%.3g" % row[c] if c in row else "-") for c in cols))
    for key in sorted(k for k in WORST if k[0] == "refine"):
        print("    neardup %s fp64: rho_F stable %.3g, fast %.3g" % (key[1], WORST[key]["stable"], WORST[key]["fast"]))
    printed = {k: v.get("rho_F/model (printed)") for k, v in WORST.items() if "rho_F/model (printed)" in v}
    for key in sorted(printed):
        print("    printed only (scaled, neardup) %s %s %s: rho_F / model %.3g" % (key + (printed[key],)))
