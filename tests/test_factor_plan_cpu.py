"""The ground tests/test_gpu_factor_plan.py stands on, without a device: gpc_debug_factor_plan is declared and bound, the
NumPy model of the plan (tests/blocked_model.py) stays inside every bar of tests/factor_ref.py on every case the GPU test
runs -- the reference alone does not use up the bars -- and the bars bite: a model with one seeded defect of the kind
the device could have (a refinement that does not run, a stale tile of T21, a wrong k-range, a flipped sign, a padded
panel that reaches logdet, a forward solve that reads the wrong buffer) fails the check that is there to catch it."""

import os
import re

import numpy as np
import pytest

import blocked_model as bm
import factor_ref as fr
from factor_ref import F32, F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_and_binds_the_hook():
    from gpyreg_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpcore.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+gpc_debug_factor_plan\s*\(([^)]*)\)\s*;", header)
    assert m, "include/gpcore.h does not declare gpc_debug_factor_plan"
    assert "gpc_debug_factor_plan" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["gpc_debug_factor_plan"][1]) == len(m.group(1).split(",")) == 16
    assert callable(_lib.Context.debug_factor_plan)
    assert (_lib.F64, _lib.F32) == (F64, F32)


def test_owning_blocks_mirror_the_plan():
    assert fr.owning_blocks(0, 640, 0) == [(0, 640)]
    assert fr.owning_blocks(1, 128, 0) == [(0, 128)]
    assert fr.owning_blocks(1, 640, 0) == [(0, 256), (256, 128), (384, 128), (512, 128)]
    assert fr.owning_blocks(2, 640, 128) == [(o, 128) for o in range(0, 640, 128)]
    assert fr.owning_blocks(2, 640, 256) == [(0, 256), (256, 128), (384, 256)]
    assert fr.owning_blocks(2, 384, 256) == [(0, 128), (128, 256)]
    # the model leaves W finite exactly there (NaN poison everywhere else below the diagonal)
    A0 = fr.matrix("gp", 640, F64)
    for plan, blk in ((1, 0), (2, 256)):
        out = fr.run_model(*fr.poisoned(A0), 640, plan, blk)
        fin = np.isfinite(out["W"]).reshape(5, 128, 5, 128).all(axis=(1, 3))
        exp = np.zeros((5, 5), dtype=bool)
        for off, n in fr.owning_blocks(plan, 640, blk):
            exp[off // 128:(off + n) // 128, off // 128:(off + n) // 128] = True
        assert np.array_equal(fin, np.tril(exp))


def test_cases_cover_every_mode_size_and_family():
    cs = fr.cases()
    assert len(set(cs)) == len(cs)
    for stable in (0, 1):
        for dtype in (F64, F32):
            sel = [c for c in cs if c[4] == stable and c[6] == dtype]
            assert {c[2] for c in sel} == {0, 1, 2} and {c[3] for c in sel if c[2] == 2} == {128, 256}
            assert {c[1] for c in sel} == set(fr.SIZES) and {c[0] for c in sel} == set(fr.FAMILIES)
            assert {c[5] for c in sel if c[2] < 2} == ({0} if stable else {0, 1})
            assert {c[1] for c in sel if c[2] == 2} >= {384, 640}
            assert len({c[0] for c in sel if c[1] == 640}) == 1


@pytest.mark.parametrize("case", fr.cases(), ids=fr.case_id)
def test_the_model_stays_inside_every_bar(case):
    fam, n, plan, blk, stable, keep_L, dtype = case
    A0, r = fr.matrix(fam, n, dtype), fr.rhs(n)
    out = fr.run_model(*fr.poisoned(A0), n, plan, blk, stable, keep_L, want_inv=plan == 0, r=r, dtype=dtype)
    ratios, fails = fr.verify(out, A0, plan, blk, stable, keep_L, dtype, r=r)
    print(fr.case_id(case), " ".join("%s %.3g" % kv for kv in ratios.items()))
    assert not fails, fails
    assert np.isfinite(ratios["rho_F"])


# ---- the bars bite ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,floor", [(F64, 1e6), (F32, 5.0)])
@pytest.mark.parametrize("n", [300, 640])
def test_defect_stable_mode_without_the_refinement(n, dtype, floor):
    """A stable mode that ran the fast arithmetic: measured here rho_F >= 1e6 (fp64), >= 5 (fp32) against the bar 1."""
    A0 = fr.matrix("neardup", n, dtype)
    good = fr.run_model(*fr.poisoned(A0), n, 0, 0, True, dtype=dtype)
    bad = fr.run_model(*fr.poisoned(A0), n, 0, 0, False, True, dtype=dtype)
    assert fr.rho_F(A0, fr.assemble_L(good), dtype) <= 1.0
    rf = fr.rho_F(A0, fr.assemble_L(bad), dtype)
    print("neardup n = %d %s: rho_F without the refinement %.3g" % (n, fr.DT_NAME[dtype], rf))
    assert rf >= floor
    # with the zeros of stable mode above the diagonal of A's diagonal tiles the layout is the same: the factor check
    # alone tells the two apart
    for o in range(0, fr.npad_of(n), fr.TILE):
        bad["A"][o:o + fr.TILE, o:o + fr.TILE][np.triu_indices(fr.TILE, 1)] = 0.0
    assert set(fr.verify(bad, A0, 0, 0, True, False, dtype)[1]) == {"factor"}


@pytest.mark.parametrize("dtype", [F64, F32])
def test_defect_a_tile_of_T21_from_before_the_syrk(dtype):
    """One 128-tile of the root's T21 as step 2 found it (the entries of A21) instead of as the syrk read it."""
    n = 300
    A0 = fr.matrix("gp", n, dtype)
    inp = fr.poisoned(A0)
    out = fr.run_model(*inp, n, 0, 0, False, True, dtype=dtype)
    ratios, fails = fr.verify(out, A0, 0, 0, False, True, dtype)
    assert not fails
    for M in (out["T"], out["A"]):  # (keep_L: A carries the same tile)
        M[256:384, 0:128] = inp[0][256:384, 0:128]
    assert "factor" in fr.verify(out, A0, 0, 0, False, True, dtype, rho_model=ratios["rho_F"])[1]


@pytest.mark.parametrize("stable", [0, 1])
def test_defect_khi_full_in_step_2_reads_poison(stable):
    """T21 = A21 W11^T over the full k-range reads W11's tiles above the diagonal, which nothing wrote: NaN in T."""
    n = 640
    A0 = fr.matrix("gp", n, F64)

    def hook(kw):
        if kw["beta"] == 0.0 and kw.get("khi") == bm.KHI_COL:
            kw["khi"] = bm.KHI_FULL
        return kw

    out = fr.run_model(*fr.poisoned(A0), n, 0, 0, stable, gemm_hook=hook)
    fails = fr.verify(out, A0, 0, 0, stable, False, F64)[1]
    assert "layout" in fails or "info" in fails, fails


@pytest.mark.parametrize("plan,n", [(0, 300), (1, 640)])
def test_defect_sign_of_W21(plan, n):
    A0, r = fr.matrix("gp", n, F64), fr.rhs(n)

    def hook(kw):
        if kw.get("khi") == bm.KHI_ROW:
            kw["alpha"] = -kw["alpha"]
        return kw

    out = fr.run_model(*fr.poisoned(A0), n, plan, 0, r=r, gemm_hook=hook)
    fails = fr.verify(out, A0, plan, 0, False, False, F64, r=r, rho_model=fr.model_rho_F("gp", n, plan, 0, 0, 0, F64))[1]
    # (the forward solve multiplies by W as stored: its identity holds for any W, the inverse check is what sees the sign)
    # In plan 1 the flipped W21 belongs to the root's left child, whose inverse the root's panel solve multiplies by:
    # the factorization itself goes wrong from there on.
    assert set(fails) == {"inverse"} if plan == 0 else set(fails) & {"info", "factor"}, fails


@pytest.mark.parametrize("dtype", [F64, F32])
def test_defect_a_padded_panel_reaches_logdet(dtype):
    """With identity padding a factored padded panel adds log 1 = 0 and cannot show; the leaf skips the panels that
    start at or beyond nvalid whatever they hold, so a non-unit diagonal there makes the skip observable."""
    n = 100
    A0 = fr.matrix("gp", n, dtype)
    A, W, T = fr.poisoned(A0)
    A[np.arange(112, 128), np.arange(112, 128)] = 4.0  # panel 7, beyond nvalid = 100 (panel 6 holds rows 96 .. 111)
    good = fr.run_model(A, W, T, n, 0, 0, dtype=dtype)
    bad = fr.run_model(A, W, T, n, 0, 0, dtype=dtype, leaf_nvalid=False)
    assert fr.logdet_ratio(fr.assemble_L(good), n, good["logdet"]) <= 1.0
    assert abs(bad["logdet"] - good["logdet"] - 16 * np.log(2.0)) < 1e-9
    assert fr.logdet_ratio(fr.assemble_L(bad), n, bad["logdet"]) > 1e10


@pytest.mark.parametrize("n", [300, 640])
def test_defect_forward_solve_reads_A_without_keep_L(n):
    """Without keep_L the spine's L21 exists in the scratch alone; A21 still holds the entries of the matrix."""
    A0, r = fr.matrix("gp", n, F64), fr.rhs(n)
    good = fr.run_model(*fr.poisoned(A0), n, 1, 0, r=r)
    bad = fr.run_model(*fr.poisoned(A0), n, 1, 0, r=r, solve_from_A=True)
    assert not fr.verify(good, A0, 1, 0, False, False, F64, r=r)[1]
    fails = fr.verify(bad, A0, 1, 0, False, False, F64, r=r)[1]
    assert set(fails) == {"solve"}, fails
    # with keep_L the two buffers hold the same L21: reading A is then no defect, and the check agrees
    kept = fr.run_model(*fr.poisoned(A0), n, 1, 0, keep_L=True, r=r, solve_from_A=True)
    assert not fr.verify(kept, A0, 1, 0, False, True, F64, r=r)[1]
