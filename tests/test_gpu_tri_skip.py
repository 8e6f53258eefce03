"""Zero skipping in the fp64 128-tile GEMM (gemm.h: GemmArgs::tri, option "tri_skip"): with the guarantee given, a
launch computes the same BITS as without it, writes nothing it is not entitled to, and -- small integers -- the exact
product.  Single launches go through gpc_debug_gemm_form (bits 8-11 of its flags carry the guarantee), the plan through
gpc_debug_factor_plan, the pipeline through nll_batch, each with the option on and off in one process.

The product runs launches of fewer than `small_blocks` (1100) 128-tiles as 64-tiles, which ignore the guarantee: at the
sizes of a quick test nothing would reach the new instantiations.  The plan and pipeline tests therefore run every case
twice, at the default and with small_blocks = 1 (every launch in 128-tiles), and put the option back."""

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A_FIRST, A_LAST, B_FIRST, B_LAST, DIAG = 1, 2, 3, 4, 8
SENT = -1048576.5
# name -> (tri, a_kmajor, b_kmajor, klo, khi, lower_only, beta): the launches of plan.h that give a guarantee
LAUNCHES = {
    "wtw_a_first": (A_FIRST, 1, 1, 1, 0, 1, 0),
    "wtw_a_first_diag": (A_FIRST | DIAG, 1, 1, 1, 0, 1, 0),
    "w21_a_last": (A_LAST, 0, 1, 0, 1, 0, 0),
    "u_b_first": (B_FIRST, 0, 1, 2, 0, 0, 0),
    "t21_b_last": (B_LAST, 0, 0, 0, 2, 0, 0),
    "t21_b_last_beta1": (B_LAST, 0, 0, 0, 2, 0, 1),
    "syrk_diag": (DIAG, 0, 0, 0, 0, 1, 1),
}


@pytest.fixture(scope="module")
def ctx():
    from gpyreg_amd import _lib

    c = _lib.context(0)
    before = {k: c.get_option(k) for k in ("tri_skip", "small_blocks")}
    yield c
    for k, v in before.items():
        c.set_option(k, v)


@functools.lru_cache(maxsize=None)
def _operands(name, n, batch, integer, both_tri=False):
    """Aop (batch, n, n) [m, k], Bop (batch, n, n) [k, n], C0 (batch, n, n): the operand the kind speaks of is zero in
    the half of every diagonal 128-block the caller vouches for (and random elsewhere, the blocks outside the k-range
    included).  both_tri (W^T W proper): Bop = W, Aop = W^T for one lower triangular W."""
    tri = LAUNCHES[name][0]
    rng = np.random.default_rng([n, batch, int(integer), sum(map(ord, name))])
    draw = (lambda: rng.integers(-4, 5, (batch, n, n)).astype(float)) if integer else (lambda: rng.uniform(-1, 1, (batch, n, n)))
    A, B, C0 = draw(), draw(), (rng.integers(-100, 101, (batch, n, n)).astype(float) if integer else rng.uniform(-1, 1, (batch, n, n)))
    idx = np.arange(n)
    same = (idx[:, None] // 128) == (idx[None, :] // 128)
    r, c = idx[:, None], idx[None, :]
    kind = tri & 7
    if both_tri:
        W = np.where(r >= c, B, 0.0)  # W[k][n], zero above the diagonal
        A, B = W.transpose(0, 2, 1).copy(), W
    elif kind == A_FIRST:
        A[:, same & (c < r)] = 0.0  # A(m, k) = 0 for k < m
    elif kind == A_LAST:
        A[:, same & (c > r)] = 0.0  # A(m, k) = 0 for k > m
    elif kind == B_FIRST:
        B[:, same & (r < c)] = 0.0  # B(k, n) = 0 for k < n
    elif kind == B_LAST:
        B[:, same & (r > c)] = 0.0  # B(k, n) = 0 for k > n
    for a in (A, B, C0):
        a.setflags(write=False)
    return A, B, C0


def _entitled(n, lower, diag):
    """Elements a launch may write: its tiles, and of the diagonal tiles of a diag-lower launch the 16 x 16 fragments
    with fragment row >= fragment column."""
    idx = np.arange(n)
    ti, tj = idx[:, None] // 128, idx[None, :] // 128
    m = (tj <= ti) if lower else np.ones((n, n), dtype=bool)
    if diag:
        m &= (ti != tj) | (idx[:, None] // 16 >= idx[None, :] // 16)
    return m


def _reference(A, B, C0, klo, khi, lower, beta, alpha):
    """The product over each 128-tile's own k-range (exact for small integers)."""
    n = A.shape[1]
    out = C0.copy()
    for ti in range(n // 128):
        for tj in range(n // 128):
            if lower and tj > ti:
                continue
            k0 = {0: 0, 1: ti, 2: tj}[klo] * 128
            k1 = {0: n // 128, 1: ti + 1, 2: tj + 1}[khi] * 128
            r, c = slice(ti * 128, ti * 128 + 128), slice(tj * 128, tj * 128 + 128)
            acc = A[:, r, k0:k1] @ B[:, k0:k1, c]
            out[:, r, c] = alpha * acc + (C0[:, r, c] if beta else 0)
    return out


def _launch(ctx, name, n, batch, form, on, integer, both_tri=False):
    from gpyreg_amd import _lib

    tri, akm, bkm, klo, khi, lower, beta = LAUNCHES[name]
    A, B, C0 = _operands(name, n, batch, integer, both_tri)
    Cin = C0.copy()
    ent = _entitled(n, lower, False)
    Cin[:, ~ent] = SENT  # the tiles a lower_only launch leaves alone
    if not beta:
        Cin[:] = SENT
    As = A.transpose(0, 2, 1) if akm else A
    Bs = B if bkm else B.transpose(0, 2, 1)
    alpha = -1.0 if beta else 1.0
    prod = _lib.GemmProduct(np.ascontiguousarray(As), np.ascontiguousarray(Bs), Cin, n, n, n, akm, bkm, alpha, beta, klo, khi,
                            lower, s_a=n * n, s_b=n * n, s_c=n * n)
    flags = 24 | ((tri if on else 0) << _lib.TRI_FLAGS_SHIFT)
    r = ctx.debug_gemm_form(form, prod, batch=batch, tile=128, flags=flags, block_slots=1 if form == "persist" else 0)
    return r["C"][0].reshape(batch, n, n), Cin, _reference(A, B, C0, klo, khi, lower, beta, alpha)


@pytest.mark.parametrize("form", ["plain", "persist"])
@pytest.mark.parametrize("name", sorted(LAUNCHES))
def test_single_launches_same_bits_and_nothing_else_written(ctx, name, form):
    """Tests 1 and 2 of the design: n = 128 (the boundary block is the whole k-range), 256 (a boundary block and a plain
    one: the seam between the masked sequence and the plain loop, in the order the kind has them) and 384; batch 1 and
    3; the plain grid and the persistent kernel with ONE block slot, so that a block runs tile after tile."""
    tri, _, _, _, _, lower, beta = LAUNCHES[name]
    for n in (128, 256, 384):
        for batch in (1, 3):
            what = (name, form, n, batch)
            ent = _entitled(n, lower, bool(tri & DIAG))
            # operands that ARE triangular, random non-integer entries: flag on == flag off, bit for bit
            on, Cin, _ = _launch(ctx, name, n, batch, form, True, False)
            off, _, _ = _launch(ctx, name, n, batch, form, False, False)
            assert np.array_equal(on[:, ent].view(np.uint64), off[:, ent].view(np.uint64)), what
            # nothing else is written: the sentinel (beta = 0) or the old value (beta = 1) is still there
            assert np.array_equal(on[:, ~ent].view(np.uint64), Cin[:, ~ent].view(np.uint64)), what
            # small integers: NumPy's exact product
            on, Cin, ref = _launch(ctx, name, n, batch, form, True, True)
            assert np.array_equal(on[:, ent], ref[:, ent]), what
            assert np.array_equal(on[:, ~ent], Cin[:, ~ent]), what


@pytest.mark.parametrize("form", ["plain", "persist"])
@pytest.mark.parametrize("name", ["wtw_a_first", "w21_a_last", "u_b_first", "t21_b_last"])
def test_the_masked_instantiation_is_what_runs(ctx, name, form):
    """The bits of flag on and flag off agree by construction, so the tests above would pass if the launcher ran the plain
    kernel.  Here the caller LIES: the operand is full (integers, no zero half) and the flag is given.  The masked kernel
    never issues the fragments it was told are zero, so the result is the exact product with exactly those zeroed -- and
    differs from the plain launch's."""
    from gpyreg_amd import _lib

    tri, akm, bkm, klo, khi, lower, beta = LAUNCHES[name]
    n, batch = 256, 3
    rng = np.random.default_rng([tri, 9])
    A = rng.integers(1, 5, (batch, n, n)).astype(float)  # no zeros at all
    B = rng.integers(1, 5, (batch, n, n)).astype(float)
    idx = np.arange(n)
    same, r, c = (idx[:, None] // 128) == (idx[None, :] // 128), idx[:, None], idx[None, :]
    # what is skipped is whole fragments per slab under the busier wave's mask: i > s // 2 of the fragments 2 i + w in
    # slab s (FIRST), i < s // 2 (LAST) -- in elements, the 32 x 32 sub-blocks strictly on the zero side of the diagonal
    r32, c32 = (r % 128) // 32, (c % 128) // 32
    Az, Bz = A.copy(), B.copy()
    if tri == A_FIRST:
        Az[:, same & (r32 > c32)] = 0.0  # A[m, k]
    elif tri == A_LAST:
        Az[:, same & (r32 < c32)] = 0.0
    elif tri == B_FIRST:
        Bz[:, same & (c32 > r32)] = 0.0  # B[k, n]
    else:
        Bz[:, same & (c32 < r32)] = 0.0
    C0 = np.zeros((batch, n, n))
    ent = _entitled(n, lower, False)
    got = {}
    for on in (True, False):
        prod = _lib.GemmProduct(np.ascontiguousarray(A.transpose(0, 2, 1) if akm else A),
                                np.ascontiguousarray(B if bkm else B.transpose(0, 2, 1)), np.full((batch, n, n), SENT), n, n, n,
                                akm, bkm, 1.0, 0, klo, khi, lower, s_a=n * n, s_b=n * n, s_c=n * n)
        flags = 24 | ((tri if on else 0) << _lib.TRI_FLAGS_SHIFT)
        got[on] = ctx.debug_gemm_form(form, prod, batch=batch, tile=128, flags=flags,
                                      block_slots=1 if form == "persist" else 0)["C"][0].reshape(batch, n, n)
    assert np.array_equal(got[True][:, ent], _reference(Az, Bz, C0, klo, khi, lower, 0, 1.0)[:, ent]), name
    assert np.array_equal(got[False][:, ent], _reference(A, B, C0, klo, khi, lower, 0, 1.0)[:, ent]), name
    assert not np.array_equal(got[True][:, ent], got[False][:, ent])


@pytest.mark.parametrize("form", ["plain", "persist"])
def test_wtw_proper_with_both_operands_triangular(ctx, form):
    """W^T W as the pipeline launches it: ONE lower triangular W as both operands (B is triangular too where ti = tj)."""
    for name in ("wtw_a_first", "wtw_a_first_diag"):
        for n, batch in ((128, 1), (256, 3), (384, 3)):
            ent = _entitled(n, True, name.endswith("diag"))
            on, Cin, _ = _launch(ctx, name, n, batch, form, True, False, both_tri=True)
            off, _, _ = _launch(ctx, name, n, batch, form, False, False, both_tri=True)
            assert np.array_equal(on[:, ent].view(np.uint64), off[:, ent].view(np.uint64)), (name, n, batch)
            assert np.array_equal(on[:, ~ent].view(np.uint64), Cin[:, ~ent].view(np.uint64)), (name, n, batch)
            on, _, ref = _launch(ctx, name, n, batch, form, True, True, both_tri=True)
            assert np.array_equal(on[:, ent], ref[:, ent]), (name, n, batch)


def test_fp32_ignores_the_guarantee(ctx):
    from gpyreg_amd import _lib

    tri, akm, bkm, klo, khi, lower, beta = LAUNCHES["wtw_a_first_diag"]
    A, B, _ = _operands("wtw_a_first_diag", 256, 3, False)
    out = []
    for on in (True, False):
        Cin = np.full((3, 256, 256), SENT)
        prod = _lib.GemmProduct(np.ascontiguousarray(A.transpose(0, 2, 1)), B, Cin, 256, 256, 256, akm, bkm, 1.0, beta, klo, khi,
                                lower, s_a=256 * 256, s_b=256 * 256, s_c=256 * 256)
        flags = 24 | ((tri if on else 0) << _lib.TRI_FLAGS_SHIFT)
        out.append(ctx.debug_gemm_form("plain", prod, batch=3, tile=128, flags=flags, dtype=_lib.F32)["C"][0])
    assert np.array_equal(out[0].view(np.uint64), out[1].view(np.uint64))
    ent = _entitled(256, True, False)  # the whole diagonal tiles: fp32 knows no diag-lower
    assert (out[0].reshape(3, 256, 256)[:, ent] != SENT).all()


# ---- the factorization plan ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _spd(npad, batch):
    rng = np.random.default_rng([npad, batch, 41])
    Q = rng.standard_normal((batch, npad, 48))
    A = Q @ Q.transpose(0, 2, 1) + 60.0 * np.eye(npad)
    idx = np.arange(npad)
    up = ((idx[:, None] // 128) == (idx[None, :] // 128)) & (idx[None, :] > idx[:, None])
    A[:, up] = np.nan  # the upper triangles of the diagonal tiles: nobody may read them
    A.setflags(write=False)
    return A


def _plan_both_ways(ctx, npad, batch, what, **kw):
    A = _spd(npad, batch)
    W = np.zeros_like(A)
    T = np.full_like(A, np.nan)
    res = []
    for on in (1, 0):
        ctx.set_option("tri_skip", on)
        res.append(ctx.debug_factor_plan(A, W, T, npad, **kw))
    ctx.set_option("tri_skip", 1)
    on, off = res
    assert np.array_equal(on["info"], off["info"]) and not on["info"].any(), what
    assert np.array_equal(on["logdet"].view(np.uint64), off["logdet"].view(np.uint64)), what
    low = np.tril(np.ones((npad, npad), dtype=bool))
    for key in ("A", "W") + (("Ainv",) if kw.get("want_inv") else ()):
        assert np.array_equal(on[key][:, low].view(np.uint64), off[key][:, low].view(np.uint64)), what + (key,)
    assert np.isfinite(on["W"][:, low]).all(), what


@pytest.mark.parametrize("small_blocks", [1100, 1])
@pytest.mark.parametrize("npad,batch", [(256, 1), (256, 4), (384, 1), (384, 4), (1024, 1), (1024, 4), (2304, 1), (2304, 4)])
def test_factor_plan_same_bits(ctx, npad, batch, small_blocks):
    """L, W, A^-1 (lower), log det and info with the option on and off, fast and stable mode, the upper triangles of A's
    diagonal tiles and the whole scratch NaN on entry."""
    ctx.set_option("small_blocks", small_blocks)
    try:
        for stable in (False, True):
            _plan_both_ways(ctx, npad, batch, (npad, batch, stable, small_blocks), plan=0, stable=stable, want_inv=True)
        if npad == 1024:  # the NLL-only plan: blocked panel solves against inverses of 256 rows
            _plan_both_ways(ctx, npad, batch, (npad, batch, "nll", small_blocks), plan=2, nll_block=256)
            _plan_both_ways(ctx, npad, batch, (npad, batch, "nll stable", small_blocks), plan=2, nll_block=256, stable=True)
    finally:
        ctx.set_option("small_blocks", 1100)


# ---- the pipeline -------------------------------------------------------------------------------------------------------
def _gp(N, D, seed):
    import gpyreg_amd as gpr

    rng = np.random.default_rng(seed)
    X = rng.uniform(-3, 3, (N, D))
    y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
    gp = gpr.GP(D, gpr.covariance_functions.Matern(5), gpr.mean_functions.ConstantMean(),
                gpr.noise_functions.GaussianNoise(constant_add=True))
    hyp0 = np.concatenate([np.log(1.5) * np.ones(D), [0.0], [np.log(0.2)], [0.3]])
    gp.update(X_new=X, y_new=y, hyp=hyp0[None, :], compute_posterior=False)
    return gp, hyp0, rng


def _nll_both_ways(ctx, gp, hyp):
    from gpyreg_amd.gaussian_process import _DTYPES

    cov_N, _, _ = gp._counts()
    gp._ctx()
    pv = gp._plugin_values(hyp, True)
    kid, deg = gp._kid()
    res = []
    for on in (1, 0):
        ctx.set_option("tri_skip", on)
        res.append(ctx.nll_batch(kid, deg, _DTYPES[gp.dtype], hyp[:, :cov_N], pv["m"], pv["sn2"], pv["vec"], True, pv["dm"],
                                 pv["dsn2"]))
    ctx.set_option("tri_skip", 1)
    return res


@pytest.mark.parametrize("small_blocks", [1100, 1])
@pytest.mark.parametrize("N,S", [(300, 3), (1000, 16), (2304, 4)])
def test_pipeline_same_bits(ctx, N, S, small_blocks):
    ctx.set_option("small_blocks", small_blocks)
    try:
        gp, hyp0, rng = _gp(N, 3, N)
        hyp = hyp0 + 0.1 * rng.standard_normal((S, hyp0.size))
        on, off = _nll_both_ways(ctx, gp, hyp)
        assert np.isfinite(on[0]).all() and np.isfinite(on[1]).all()
        assert np.array_equal(on[0].view(np.uint64), off[0].view(np.uint64)), "nlZ"
        assert np.array_equal(on[1].view(np.uint64), off[1].view(np.uint64)), "dnlZ"
        assert np.array_equal(on[2], off[2]) and np.array_equal(on[4], off[4])
    finally:
        ctx.set_option("small_blocks", 1100)


@pytest.mark.parametrize("small_blocks", [1100, 1])
def test_pipeline_with_a_failed_first_factorization(ctx, small_blocks):
    """One sample of the batch is singular at the first jitter level (duplicated inputs, noise 1e-9): the same samples
    fail, the same retry level succeeds and every sample's bits are the same with the option on and off."""
    import gpyreg_amd as gpr

    ctx.set_option("small_blocks", small_blocks)
    try:
        # (the construction of tests/test_gpu_boundary_cm.py: test_constant_mean_entry_through_a_jitter_retry)
        rng = np.random.default_rng(3)
        N, D = 200, 2
        X = rng.uniform(-3, 3, (N, D))
        X[100:] = X[:100]
        y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
        gp = gpr.GP(D, gpr.covariance_functions.SquaredExponential(), gpr.mean_functions.ConstantMean(),
                    gpr.noise_functions.GaussianNoise(constant_add=True))
        hyp = np.array([[np.log(1.0), np.log(1.5), 0.1, np.log(0.1), 0.0], [np.log(2.0), np.log(2.0), 0.0, np.log(1e-9), 0.2],
                        [np.log(1.2), np.log(1.4), 0.0, np.log(0.2), 0.1]])
        gp.update(X_new=X, y_new=y, hyp=hyp[:1], compute_posterior=False)
        on, off = _nll_both_ways(ctx, gp, hyp)
        assert on[2][1] > 1 and on[2][0] == 1 and on[2][2] == 1, on[2]  # sample 1 needed jitter, the others did not
        for a, b in zip(on, off):
            assert np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))
    finally:
        ctx.set_option("small_blocks", 1100)
