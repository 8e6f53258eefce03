"""The ground the direct tests of blas1.h stand on, without a device: the hook is declared and bound, and the inputs
and the derived bound of tests/test_gpu_blas1.py are consistent -- a plain NumPy fp64 emulation of each reduction's
documented summation order (lane-strided partial sums, xor butterfly, four-wave sum, chunk sums; no FMA), run on the
exact inputs of the GPU test, stays inside the bound against the longdouble reference.  The emulation indexes only what
the kernels' comments allow, so the NaN-poisoned storage around every operand never enters it: a NaN in its result would
mean the test's own inputs poison the contract region."""

import os
import re

import numpy as np
import pytest

import blas1_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_and_binds_the_hook():
    from gpyreg_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpcore.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+gpc_debug_blas1\s*\(([^)]*)\)\s*;", header)
    assert m, "include/gpcore.h does not declare gpc_debug_blas1"
    assert "gpc_debug_blas1" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["gpc_debug_blas1"][1]) == len(m.group(1).split(",")) == 8
    assert callable(_lib.Context.debug_blas1)
    assert len(_lib.BLAS1) == 22 and sorted(_lib.BLAS1.values()) == list(range(22))
    assert _lib.BLAS1_GUARD == br.GUARD
    # every kernel of the header but the two utility probes has a `which`
    src = open(os.path.join(ROOT, "gpyreg_amd", "csrc", "blas1.h")).read()
    kernels = set(re.findall(r"\bvoid\s+(\w+)_kernel\s*\(", src)) - {"mfma_peak", "valu_peak"}
    assert kernels == set(_lib.BLAS1), kernels ^ set(_lib.BLAS1)


def test_summation_helpers_add_every_term_once():
    """Integers add exactly in any order: each emulated order must return the plain sum."""
    rng = np.random.default_rng(1)
    for n in (1, 63, 128, 255, 256, 257, 640):
        t = rng.integers(-1000, 1000, (3, n)).astype(np.float64)
        assert np.array_equal(br.block_sum(t), t.sum(-1))
        for vec in (2, 4):
            assert np.array_equal(br.lane_strided(t, vec), t.sum(-1))
    for rows in (1, 3, 4, 130):
        t = rng.integers(-1000, 1000, (2, rows, 57)).astype(np.float64)
        assert np.array_equal(br.four_waves(t), t.sum(1))
    v = rng.integers(-1000, 1000, (5, 64)).astype(np.float64)
    assert np.array_equal(br.wave_sum(v), np.repeat(v.sum(-1, keepdims=True), 64, axis=1))


@pytest.mark.parametrize("dtype", [br.F64, br.F32], ids=["f64", "f32"])
def test_emulated_summation_orders_stay_inside_the_derived_bound(dtype):
    worst = {}
    for case in br.reduction_cases(dtype):
        got = case.emu()
        ratio = br.check(case, got, guard=False)
        worst[case.which] = max(worst.get(case.which, 0.0), ratio)
    print("\nfp64 emulation, worst |error| / bound (%s): " % br.DT_NAME[dtype]
          + "  ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert set(worst) == {"trmv", "trmv_low", "gemv_sub", "trmv_t_part", "trmv_t_part_low", "trmv_t_sum", "dot",
                          "mat_t_vec", "grad_tail", "colsum_prod", "colsum_vec", "diagq", "trace_plane"}


@pytest.mark.parametrize("dtype", [br.F64, br.F32], ids=["f64", "f32"])
def test_every_case_is_self_consistent(dtype):
    """The moves and the append cases: operands of the announced sizes, expectations of the outputs' sizes, and nothing
    expected of an entry both to the bit and within a bound."""
    for case in list(br.copy_cases(dtype)) + list(br.append_cases(dtype)):
        for o in case.outs:
            assert not (o.tol & o.skip).any()
            if o.tol.any():
                assert np.isfinite(o.ref[o.tol].astype(np.float64)).all() and (o.bnd[o.tol] >= 0).all(), case.name
            assert np.isfinite(o.exact[~o.tol & ~o.skip]).all(), (case.name, "a move never produces a NaN here")
