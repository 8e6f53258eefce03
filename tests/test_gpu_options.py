"""gpc_set_option / gpc_get_option walk one table (gpcore.hip: OPTIONS).  Every name the two else-if ladders knew before
the table, with the value each ladder stored for -1, 0, 1, 2, 3, 100 and 4096, written down here from those ladders:
the names are still accepted, set-then-get returns the same clamped value, the counters stay get-only, the three
test hooks that could never be read back stay set-only, and an unknown name is refused by both.  (A context needs a
device, so this is a GPU test; nothing is computed while the options are off their defaults.)"""

import pytest

pytestmark = pytest.mark.gpu

VALUES = (-1, 0, 1, 2, 3, 100, 4096)
RAW = VALUES
FLAG = (1, 0, 1, 1, 1, 1, 1)  # value != 0
ENGINE = (0, 0, 1, 2, 0, 0, 0)  # 1 and 2 force an engine, anything else is "by default"

# name -> what get returns after set(name, v) for v in VALUES
SETTABLE = {
    "groups": (1, 1, 1, 2, 3, 8, 8),  # 1 .. MAXG = 8
    "small_blocks": RAW,
    "dual_launch": FLAG,
    "leaf": (5, 5, 5, 5, 3, 5, 5),  # 3 or the default 5
    "defer_min": RAW,
    "defer_reserve": RAW,
    "nll_block": (-1, 0, 128, 128, 128, 128, 4096),  # negative: automatic; else a multiple of 128, at least 128
    "solves_beside_lauum": FLAG,
    "stable": FLAG,
    "small_path": FLAG,
    "check_queues": FLAG,
    "small_poll": FLAG,
    "small_timing": FLAG,
    "block_engine": ENGINE,
    "paths_engine": ENGINE,
    "paths_solve_engine": ENGINE,
}
SET_ONLY = {"leaf_fault": 0, "start_mult_log10": 0, "append_fail_mask": 0}  # name -> the default to put back
GET_ONLY = ("small_polled", "small_synced", "cov_fused", "quad_mix_gemms", "block_engine_ran", "paths_engine_ran",
            "paths_solve_engine_ran", "block_appended", "block_stale", "last_chunk", "experiments")
EXPERIMENTS = {
    "rect_min": RAW,
    "rect_mode": FLAG,
    "indep": RAW,
    "indep_max": (2, 2, 2, 2, 3, 8, 8),  # 2 .. MAXG
    "indep_min_tiles": (1, 1, 1, 2, 3, 100, 4096),
    "rl_ahead_max": RAW,
    "rl_panel": (0, 0, 128, 128, 128, 128, 4096),
    "dag": RAW,
    "dag_small_tiles": RAW,
    "dag_lauum": RAW,
    "dag_leaf_blocks": RAW,
    "dag_aborts": RAW,
    "dag_runs": RAW,
    "dag_urgent_cus": (0, 0, 1, 2, 3, 15, 15),
    "dag_gate": RAW,
    "dag_gate_pct": (0, 0, 1, 2, 3, 100, 100),
    "dag_crit_pct": (0, 0, 1, 2, 3, 100, 100),
    "dag_timeout_ms": (1, 1, 1, 2, 3, 100, 4096),
}


def _roundtrip(ctx, table):
    for name, want in table.items():
        before = ctx.get_option(name)
        try:
            got = []
            for v in VALUES:
                ctx.set_option(name, v)
                got.append(ctx.get_option(name))
            assert tuple(got) == tuple(want), (name, got)
        finally:
            ctx.set_option(name, before)
        assert ctx.get_option(name) == before, name


def test_every_option_keeps_its_name_and_its_clamp():
    from gpyreg_amd import _lib

    ctx = _lib.context()
    _roundtrip(ctx, SETTABLE)
    for name, default in SET_ONLY.items():
        try:
            for v in VALUES:
                ctx.set_option(name, v)
            with pytest.raises(RuntimeError, match="gpc_get_option: unknown option"):
                ctx.get_option(name)
        finally:
            ctx.set_option(name, default)
    for name in GET_ONLY:
        before = ctx.get_option(name)
        with pytest.raises(RuntimeError, match="gpc_set_option: unknown option"):
            ctx.set_option(name, 1)
        assert ctx.get_option(name) == before, name
    assert ctx.get_option("experiments") == int(_lib.is_experiments_build())
    for call in (lambda: ctx.set_option("no_such_option", 1), lambda: ctx.get_option("no_such_option")):
        with pytest.raises(RuntimeError, match="rc=-2.*unknown option"):
            call()
    if not _lib.is_experiments_build():  # the product library does not know the experiments' names
        for name in EXPERIMENTS:
            with pytest.raises(RuntimeError, match="unknown option"):
                ctx.get_option(name)


@pytest.mark.experiments
def test_every_experiments_option_keeps_its_name_and_its_clamp():
    from gpyreg_amd import _lib

    _roundtrip(_lib.context(), EXPERIMENTS)
