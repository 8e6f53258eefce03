"""Every launch form of gemm.h at small shapes, per element, through gpc_debug_gemm_form: plain gemm_kernel (with and
without the XCD-aware order), gemm_persist_kernel with the flat queue, with the eight XCD-affine queues (both regimes)
and behind cu_reserve_bail, gemm_dual_kernel, and the two non-storing epilogues (EPI 1 colsq, EPI 2 wsq).

The structural tests use small integers, so every partial sum is exact in fp64 and in fp32 and the comparison with the
int64 reference is array_equal: a tile handed out twice under beta = 1, a tile nobody computed, a wrong stride, leading
dimension, offset or column shows as a wrong element at a known place.

What the product cannot launch is not tested as if it could: a 64-tile launch without a reservation is always plain
(launch_gemm_bt), so "persist" at tile 64 checks that plain launch and that no counter moved; the dual launch exists
for 64-tiles and one pair of orientations only; launch_gemm_wsq has no persistent form, so EPI 2 runs plain only."""

import functools

import numpy as np
import pytest
from numpy.lib.stride_tricks import as_strided

pytestmark = pytest.mark.gpu

ORIENT = [(0, 0), (0, 1), (1, 1), (1, 0)]
MODES = [  # (klo, khi, lower_only): the k-range modes of test_gemm_modes_fp64
    (0, 0, 0), (0, 0, 1), (0, 2, 0), (2, 0, 0), (0, 1, 0), (1, 0, 1),
]
BATCHES = [1, 2, 3, 5, 7, 8, 9, 13]
SQUARE, RECT = (384, 384, 384), (256, 384, 256)
SENT = -1048576.5  # exact in fp32; any read-modify-write or store changes it


@pytest.fixture(scope="module")
def ctx():
    from gpyreg_amd import _lib

    return _lib.context(0)


# ---- inputs and references, computed once and shared ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _int_ops(shape, s):
    """Sample s of a shape: Aop (M, K) and Bop (K, N) integers in [-4, 4], C0 (M, N) integers in [-100, 100]."""
    M, N, K = shape
    rng = np.random.default_rng([M, N, K, s, 77])
    ops = rng.integers(-4, 5, (M, K)), rng.integers(-4, 5, (K, N)), rng.integers(-100, 101, (M, N))
    for o in ops:
        o.setflags(write=False)
    return ops


@functools.lru_cache(maxsize=None)
def _int_slabs(shape, sa, sb):
    """Aop[sa][:, slab] @ Bop[sb][slab, :] per 128-wide k-slab, int64: a tile's k-range is a sum of whole slabs."""
    A, B = _int_ops(shape, sa)[0], _int_ops(shape, sb)[1]
    out = np.stack([A[:, k:k + 128] @ B[k:k + 128, :] for k in range(0, shape[2], 128)])
    out.setflags(write=False)
    return out


def _tiles(M, N, K, klo, khi, lower, bt):
    """(rows, cols, first slab, end slab) of every tile a launch with tile size bt computes; k-ranges are 128-granular."""
    for ti in range(M // bt):
        for tj in range(N // bt):
            if lower and tj > ti:
                continue
            m128, n128 = ti * bt // 128, tj * bt // 128
            k0 = {0: 0, 1: m128, 2: n128}[klo]
            k1 = min({0: K // 128, 1: m128 + 1, 2: n128 + 1}[khi], K // 128)
            yield slice(ti * bt, (ti + 1) * bt), slice(tj * bt, (tj + 1) * bt), k0, max(k1, k0)


def _ntiles(M, N, lower, bt):
    tm, tn = M // bt, N // bt
    return tm * (tm + 1) // 2 if lower else tm * tn


@functools.lru_cache(maxsize=None)
def _int_prefix(shape, sa, sb):
    """Prefix sums of _int_slabs over the slabs, with a leading zero: a k-range is a difference of two of them."""
    slabs = _int_slabs(shape, sa, sb)
    out = np.concatenate([np.zeros_like(slabs[:1]), np.cumsum(slabs, axis=0)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _krange_maps(M, N, K, klo, khi, lower, bt):
    """Per element: first and end slab of its tile's k-range, and whether a launch with tile size bt computes it."""
    k0m, k1m = np.zeros((1, M, N), dtype=np.intp), np.zeros((1, M, N), dtype=np.intp)
    mask = np.zeros((M, N), dtype=bool)
    for r, c, k0, k1 in _tiles(M, N, K, klo, khi, lower, bt):
        k0m[0, r, c], k1m[0, r, c], mask[r, c] = k0, k1, True
    for a in (k0m, k1m, mask):
        a.setflags(write=False)
    return k0m, k1m, mask


def _acc_exact(shape, sa, sb, klo, khi, lower, bt):
    """int64 accumulators of the launched tiles (Aop of sample sa, Bop of sample sb) over each tile's own k-range, and
    the mask of the elements they cover."""
    k0m, k1m, mask = _krange_maps(*shape, klo, khi, lower, bt)
    pre = _int_prefix(shape, sa, sb)
    return (np.take_along_axis(pre, k1m, 0) - np.take_along_axis(pre, k0m, 0))[0], mask


# ---- embedding of the operands in their allocations ---------------------------------------------------------------------
DENSE = dict(pad=0, off=(0, 0, 0), gap=0, shared_b=False)


def _alloc(mats, ld, off, stride, fill):
    """One flat allocation filled by `fill(n)`, with mats[b] (rows x cols) at element off + b * stride, rows ld apart."""
    rows, cols = mats[0].shape
    n = off + (len(mats) - 1) * stride + (rows - 1) * ld + cols + 40
    a = fill(n)
    v = as_strided(a[off:], (len(mats), rows, cols), (stride * 8, ld * 8, 8))
    for b, m in enumerate(mats):
        v[b] = m
    return a


def _block_mask(n, rows, cols, ld, off, stride, batch):
    m = np.zeros(n, dtype=bool)
    as_strided(m[off:], (batch, rows, cols), (stride, ld, 1))[...] = True
    return m


class Case:
    """One product: the GemmProduct for the hook, the C allocation as uploaded, and where the samples' blocks are."""

    def __init__(self, shape, ops, akm, bkm, alpha, beta, klo, khi, lower, batch, emb=DENSE, seed=0):
        from gpyreg_amd import _lib

        M, N, K = shape
        self.shape, self.batch, self.mode, self.alpha, self.beta = shape, batch, (klo, khi, lower), alpha, beta
        rng = np.random.default_rng([seed, 5])
        junk = lambda n: rng.integers(5, 9, n).astype(np.float64)  # outside the operands' range: a misread shows
        sent = lambda n: np.full(n, SENT)
        nb = 1 if emb["shared_b"] else batch
        As = [ops(b)[0].T if akm else ops(b)[0] for b in range(batch)]
        Bs = [ops(b)[1] if bkm else ops(b)[1].T for b in range(nb)]
        self.C0 = [np.array(ops(b)[2], dtype=np.float64) for b in range(batch)]
        pad, (oa, ob, oc), gap = emb["pad"], emb["off"], emb["gap"]
        lda, ldb, self.ldc = As[0].shape[1] + pad, Bs[0].shape[1] + pad, N + pad
        s_a = (As[0].shape[0] - 1) * lda + As[0].shape[1] + gap
        s_b = 0 if emb["shared_b"] else (Bs[0].shape[0] - 1) * ldb + Bs[0].shape[1] + gap
        self.s_c, self.off_c = (M - 1) * self.ldc + N + gap, oc
        A = _alloc(As, lda, oa, s_a, junk)
        B = _alloc(Bs, ldb, ob, s_b, junk)
        self.C = _alloc(self.C0, self.ldc, oc, self.s_c, sent)
        self.prod = _lib.GemmProduct(A, B, self.C, M, N, K, akm, bkm, alpha, beta, klo, khi, lower, lda, ldb, self.ldc,
                                     oa, ob, oc, s_a, s_b, self.s_c)

    def blocks(self, alloc):
        M, N, _ = self.shape
        return as_strided(alloc[self.off_c:], (self.batch, M, N), (self.s_c * 8, self.ldc * 8, 8))

    def outside(self):
        M, N, _ = self.shape
        return ~_block_mask(self.C.size, M, N, self.ldc, self.off_c, self.s_c, self.batch)


def _exact_case(shape, akm, bkm, alpha, beta, mode, batch, bt, emb=DENSE):
    """An integer product and its exact expectation: the whole C allocation after the launch."""
    klo, khi, lower = mode
    M, N, K = shape
    case = Case(shape, lambda b: _int_ops(shape, b), akm, bkm, alpha, beta, klo, khi, lower, batch, emb)
    if lower:  # the tiles a lower_only launch leaves alone hold the sentinel too
        _, mask = _acc_exact(shape, 0, 0, klo, khi, lower, bt)
        for b in range(batch):
            case.C0[b][~mask] = SENT
            case.blocks(case.C)[b] = case.C0[b]
        case.prod.C = case.C
    want = case.C.copy()
    for b in range(batch):
        acc, mask = _acc_exact(shape, b, 0 if emb["shared_b"] else b, klo, khi, lower, bt)
        ref = case.C0[b].copy()
        old = np.where(mask, case.C0[b], 0).astype(np.int64)
        ref[mask] = (int(alpha) * acc + (old if beta else 0))[mask]
        case.blocks(want)[b] = ref
    return case, want


def _assert_exact(case, got, want, what):
    out = case.outside()
    assert np.array_equal(got.view(np.uint64)[out], case.C.view(np.uint64)[out]), ("bytes outside the blocks", what)
    bad = np.argwhere(case.blocks(got) != case.blocks(want))
    assert bad.size == 0, (what, "first wrong (sample, row, col):", bad[:4].tolist(), "of", len(bad))


def _slots_just_below(items, bt):
    """Block slots that make the cap the largest one still below the launch's items (64-tiles: two slots each)."""
    return items - 1 if bt == 128 else (items - 1) // 2


def _check_counters(lib, form, bt, counters, ntiles, batch, flags, what):
    """verify_queues' rule: every queue counter reached its queue's total, and capped at the totals they sum to the
    launch's items.  A launch that is not persistent moves no counter."""
    persistent = form == "persist_reserved" or (form in ("persist", "colsq") and bt == 128)
    if not persistent:
        assert not counters.any(), (what, counters)
        return
    _, totals, _, _ = lib.gemm_queues(ntiles, batch, flags)
    assert (counters >= totals).all(), (what, counters, totals)
    assert int(np.minimum(counters, totals).sum()) == ntiles * batch, (what, counters, totals)


def _launch(ctx, form, cases, batch, bt, flags, slots, dtype):
    r = ctx.debug_gemm_form(form, [c.prod for c in cases], batch=batch, tile=bt, flags=flags, block_slots=slots,
                            dtype=dtype)
    if r is None:
        pytest.skip("this context has no table of reserved CUs")
    return r


def _run_exact(ctx, form, bt, batch, shape, orient, mode, alpha, beta, flags, small_slots, dtype, emb=DENSE):
    from gpyreg_amd import _lib

    M, N, _ = shape
    ntiles = _ntiles(M, N, mode[2], bt)
    slots = 4 if small_slots else _slots_just_below(ntiles * batch, bt)
    what = (form, bt, batch, shape, orient, mode, alpha, beta, flags, slots, dtype)
    case, want = _exact_case(shape, orient[0], orient[1], alpha, beta, mode, batch, bt, emb)
    r = _launch(ctx, form, [case], batch, bt, flags, slots, dtype)
    _assert_exact(case, r["C"][0], want, what)
    _check_counters(_lib, form, bt, r["counters"], ntiles, batch, flags, what)


def _run_exact_dual(ctx, batch, mode1, mode2, alpha, beta, flags, dtype, emb=DENSE):
    """The dual launch as plan.h uses it: a syrk-like product (m-major x m-major) beside an m-major x k-major one."""
    what = ("dual", batch, mode1, mode2, alpha, beta, flags, dtype)
    c1, w1 = _exact_case(SQUARE, 0, 0, alpha, beta, mode1, batch, 64, emb)
    c2, w2 = _exact_case(SQUARE if mode2[2] else RECT, 0, 1, -alpha, beta, mode2, batch, 64, emb)
    r = _launch(ctx, "dual", [c1, c2], batch, 64, flags, 0, dtype)
    _assert_exact(c1, r["C"][0], w1, what + (1,))
    _assert_exact(c2, r["C"][1], w2, what + (2,))
    assert not r["counters"].any()


# ---- a. exact structural test ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("bt", [128, 64])
@pytest.mark.parametrize("form", ["plain", "persist", "persist_reserved"])
def test_exact_every_form_tile_batch(ctx, form, bt, batch):
    """Every form x tile size x batch, each with the four flag values {0, 8, 16, 24}; orientation, k-range mode, shape,
    alpha, precision and the block-slot override (4: stealing is certain; just below the launch's items) rotate with
    the case.  beta = 1 in every persistent launch: a tile executed twice is invisible under beta = 0."""
    from gpyreg_amd import _lib

    i = ["plain", "persist", "persist_reserved"].index(form) * 16 + (bt == 64) * 8 + BATCHES.index(batch)
    for j, flags in enumerate([0, 8, 16, 24]):
        mode = MODES[(i + 2 * j) % 6]
        shape = RECT if (not mode[2] and (i + j) % 3 == 0) else SQUARE
        if shape == RECT and mode[0] == 1:  # (no product launches k >= row tile on a non-square grid)
            shape = SQUARE
        _run_exact(ctx, form, bt, batch, shape, ORIENT[(i + j) % 4], mode, alpha=1 - 2 * ((i + j) % 2),
                   beta=1 if form != "plain" else (i + j) // 2 % 2, flags=flags, small_slots=j % 2 == 0,
                   dtype=_lib.F32 if (i // 4 + j) % 2 else _lib.F64)


@pytest.mark.parametrize("batch", BATCHES)
def test_exact_dual_every_batch(ctx, batch):
    from gpyreg_amd import _lib

    i = BATCHES.index(batch)
    for j, flags in enumerate([0, 8, 16, 24]):
        _run_exact_dual(ctx, batch, (0, 0, 1), MODES[(i + j) % 6], alpha=1 - 2 * ((i + j) % 2), beta=(i + j + 1) // 2 % 2,
                        flags=flags, dtype=_lib.F32 if (i + j) % 3 == 0 else _lib.F64)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", ["plain", "persist", "persist_reserved", "dual"])
def test_exact_every_kmode_form(ctx, form, mode):
    """Every k-range mode x form, the four orientations and both tile sizes, beta = 1, at batches 3 (two queue classes of
    a sample) and 9 (uneven queues; 9 x 9 tiles leave one item outside the XCD-aware order)."""
    from gpyreg_amd import _lib

    if form == "dual":
        for batch in (3, 9):
            _run_exact_dual(ctx, batch, mode if mode[2] else (0, 0, 1), mode, alpha=-1, beta=1, flags=24, dtype=_lib.F64)
            _run_exact_dual(ctx, batch, (1, 0, 1), mode, alpha=1, beta=1, flags=16, dtype=_lib.F32)
        return
    for n, orient in enumerate(ORIENT):
        for bt in (128, 64):
            _run_exact(ctx, form, bt, (3, 9)[(n + (bt == 64)) % 2], SQUARE, orient, mode, alpha=(-1, 1)[n % 2], beta=1,
                       flags=24 if n < 2 else 8, small_slots=n % 2 == 0, dtype=_lib.F64 if n % 2 else _lib.F32)


@pytest.mark.parametrize("bt", [128, 64])
def test_exact_xcd_order_with_a_remainder(ctx, bt):
    """Plain launches under flag 16 whose grid is no multiple of 8: 9 tiles x 9 samples = 81 (128-tiles), 36 x 9 and
    21 x 13 (64-tiles), the dual grid (21 + 24) x 9 -- the last total % 8 workgroups keep their own item."""
    from gpyreg_amd import _lib

    for flags in (16, 24):
        _run_exact(ctx, "plain", bt, 9, SQUARE, (0, 1), (0, 0, 0), -1, 1, flags, True, _lib.F64)
        _run_exact(ctx, "plain", bt, 13, SQUARE, (0, 0), (0, 0, 1), 1, 1, flags, True, _lib.F32)
    _run_exact_dual(ctx, 9, (0, 0, 1), (0, 0, 0), alpha=-1, beta=1, flags=16, dtype=_lib.F64)


# ---- b. embedding ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [128, 24])
@pytest.mark.parametrize("form", ["plain", "persist", "persist_reserved", "dual"])
def test_embedded_operands(ctx, form, pad):
    """Leading dimensions of extent + 128 and extent + 24, operands that start inside their allocations (offsets that
    are multiples of the 16-byte vector), a gap between the samples and one B for all samples (sB = 0).  The C
    allocation holds a sentinel everywhere outside the addressed blocks, and in the tiles a lower_only launch leaves
    alone: every sentinel must come back bit-identical, every addressed element exact."""
    from gpyreg_amd import _lib

    emb = dict(pad=pad, off=(8, 20, 12), gap=44, shared_b=True)
    for n, (batch, mode) in enumerate([(3, (0, 0, 0)), (9, (0, 0, 1)), (9, (0, 2, 0)), (3, (1, 0, 1))]):
        dtype = _lib.F32 if n % 2 else _lib.F64
        if form == "dual":
            _run_exact_dual(ctx, batch, (0, 0, 1), mode, alpha=-1, beta=1, flags=24, dtype=dtype, emb=emb)
            continue
        for bt in (128, 64):
            _run_exact(ctx, form, bt, batch, SQUARE, ORIENT[(n + (bt == 64)) % 4], mode, alpha=(-1, 1)[n % 2], beta=1,
                       flags=24, small_slots=True, dtype=dtype, emb=emb)
    if form != "dual":  # the rectangular shape, both leading orientations of the padded rows
        for orient in ORIENT:
            _run_exact(ctx, form, 128, 5, RECT, orient, (0, 0, 0), alpha=1, beta=1, flags=8, small_slots=True,
                       dtype=_lib.F64, emb=emb)


# ---- c. queue accounting -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 8])
@pytest.mark.parametrize("form", ["persist", "persist_reserved"])
def test_queue_counters_reach_their_totals(ctx, form, flags):
    """Every returned queue counter is at least its queue's total as gpc_debug_gemm_queues reports it, and capped at the
    totals the counters sum to ntiles * batch (the rule of verify_queues) -- for every batch, lower and full tile sets,
    both block-slot overrides.  (_run_exact asserts it; the structural tests above do so for all their launches too.)"""
    from gpyreg_amd import _lib

    for n, batch in enumerate(BATCHES):
        for bt in (128, 64) if form == "persist_reserved" else (128,):
            _run_exact(ctx, form, bt, batch, SQUARE, (0, 1), MODES[n % 2], alpha=1, beta=1, flags=flags,
                       small_slots=n % 2 == 1, dtype=_lib.F64)


# ---- d. epilogues --------------------------------------------------------------------------------------------------------------
def _tile_rows(v):
    """(M, N) -> (M / 128, N): sums over the 128 rows of every tile row."""
    return v.reshape(v.shape[0] // 128, 128, v.shape[1]).sum(axis=1)


@pytest.mark.parametrize("batch", [1, 3, 9])
@pytest.mark.parametrize("persistent", [False, True])
def test_colsq_epilogue_exact(ctx, persistent, batch):
    """EPI 1 (launch_gemm_colsq): colsq[(b tiles_m + ti) N + col] = sum over the 128 rows of tile row ti of
    (alpha acc)^2, exact for the integer inputs (below 2^38); C is not stored.  M = 256, N = 384: tile rows and columns
    cannot be swapped unnoticed.  Plain, and persistent with both queue kinds."""
    from gpyreg_amd import _lib

    M, N, K = RECT
    for n, (alpha, flags, dtype) in enumerate([(-1, 24, _lib.F64), (2, 0, _lib.F32), (-2, 8, _lib.F64)]):
        what = (persistent, batch, alpha, flags, dtype)
        case = Case(RECT, lambda b: _int_ops(RECT, b), 0, 1, alpha, 0, 0, 0, 0, batch,
                    dict(pad=24 * (n % 2), off=(0, 0, 0), gap=0, shared_b=False))
        slots = (4 if n % 2 == 0 else _slots_just_below(6 * batch, 128)) if persistent else 0
        r = ctx.debug_gemm_form("colsq", case.prod, batch=batch, flags=flags, block_slots=slots, dtype=dtype)
        want = np.stack([_tile_rows((alpha * _acc_exact(RECT, b, b, 0, 0, 0, 128)[0]) ** 2)
                         for b in range(batch)])
        assert np.array_equal(r["colsq"], want.astype(np.float64)), (what, np.argwhere(r["colsq"] != want)[:4].tolist())
        assert np.array_equal(r["C"][0].view(np.uint64), case.C.view(np.uint64)), what
        if persistent:
            _check_counters(_lib, "colsq", 128, r["counters"], 6, batch, flags, what)
        else:
            assert not r["counters"].any()


@pytest.mark.parametrize("batch", [1, 3, 9])
def test_wsq_epilogue_exact(ctx, batch):
    """EPI 2 (launch_gemm_wsq; a plain launch -- the product has no persistent one): with v = C + ep_alpha[b] acc,
    colsq[(b tiles_m + ti) N + col] = sum over the 128 rows of tile row ti of ep_w[b ep_sw + row] v^2.  Integer C,
    dyadic weights 2^-3 .. 2^3 and an integer factor that differs per sample: exact.  C is only read."""
    from gpyreg_amd import _lib

    M, N, K = RECT
    rng = np.random.default_rng(batch)
    for flags, dtype, ep_sw in ((24, _lib.F64, M + 8), (0, _lib.F32, M), (16, _lib.F64, 0)):
        what = (batch, flags, dtype, ep_sw)
        case = Case(RECT, lambda b: _int_ops(RECT, b), 1, 1, 1.0, 1, 0, 0, 0, batch)
        w = 2.0 ** rng.integers(-3, 4, (batch - 1) * ep_sw + M)
        al = np.array([(-1) ** b * (b % 3 + 1) for b in range(batch)], dtype=np.float64)
        r = ctx.debug_gemm_form("wsq", case.prod, batch=batch, flags=flags, dtype=dtype, ep_w=w, ep_sw=ep_sw, ep_alpha=al)
        want = []
        for b in range(batch):
            acc = _acc_exact(RECT, b, b, 0, 0, 0, 128)[0]
            v = (_int_ops(RECT, b)[2] + int(al[b]) * acc).astype(np.float64)
            want.append(_tile_rows(w[b * ep_sw:b * ep_sw + M, None] * v * v))
        want = np.stack(want)
        assert np.array_equal(r["colsq"], want), (what, np.argwhere(r["colsq"] != want)[:4].tolist())
        assert np.array_equal(r["C"][0].view(np.uint64), case.C.view(np.uint64)), what
        assert not r["counters"].any()


# ---- e. rounding, f. bit identity across forms -----------------------------------------------------------------------------------
RSHAPE = (256, 384, 384)


@functools.lru_cache(maxsize=None)
def _real_ops(s, fp32):
    M, N, K = RSHAPE
    rng = np.random.default_rng([s, 1234])
    ops = [rng.standard_normal((M, K)), rng.standard_normal((K, N)), rng.standard_normal((M, N))]
    if fp32:
        ops = [o.astype(np.float32).astype(np.float64) for o in ops]
    for o in ops:
        o.setflags(write=False)
    return tuple(ops)


@functools.lru_cache(maxsize=None)
def _real_slabs(s, fp32):
    """Per 128-wide k-slab: the product in np.longdouble, and |A| |B|."""
    A, B, _ = _real_ops(s, fp32)
    Al, Bl = A.astype(np.longdouble), B.astype(np.longdouble)
    ks = range(0, RSHAPE[2], 128)
    return (np.stack([Al[:, k:k + 128] @ Bl[k:k + 128, :] for k in ks]),
            np.stack([np.abs(A[:, k:k + 128]) @ np.abs(B[k:k + 128, :]) for k in ks]))


@pytest.mark.parametrize("bt", [128, 64])
@pytest.mark.parametrize("fp32", [False, True])
def test_rounding_of_the_plain_batched_launch(ctx, fp32, bt):
    """Standard-normal A, B, C0, batch 2, M = 256, N = 384, K = 384, alpha = -0.75, beta = 1, against np.longdouble over
    each tile's k-range (fp32: on the fp32-rounded operands).  Bound, per element:
        2 (k_len + 2) u (|alpha| (|A| |B|)_ij + beta |C0_ij|),   u = 2^-53 (fp64) or 2^-24 (fp32)
    -- the bound of a sequential dot product of k_len terms, plus the scaling and the addition of C0, doubled for the
    higher-order terms (the construction of _gemm_fp32_bound).  The bound is derived, not measured."""
    from gpyreg_amd import _lib

    M, N, K = RSHAPE
    u = 2.0 ** (-24 if fp32 else -53)
    alpha, beta = -0.75, 1
    for (akm, bkm), (klo, khi) in zip(ORIENT, [(0, 0), (0, 2), (2, 0), (0, 1)]):
        case = Case(RSHAPE, lambda b: _real_ops(b, fp32), akm, bkm, alpha, beta, klo, khi, 0, 2)
        r = ctx.debug_gemm_form("plain", case.prod, batch=2, tile=bt, dtype=_lib.F32 if fp32 else _lib.F64)
        got = case.blocks(r["C"][0])
        worst = 0.0
        for b in range(2):
            prod, absprod = _real_slabs(b, fp32)
            C0 = _real_ops(b, fp32)[2]
            ref = np.zeros((M, N), dtype=np.longdouble)
            bound = np.zeros((M, N))
            for rs, cs, k0, k1 in _tiles(M, N, K, klo, khi, 0, bt):
                ref[rs, cs] = alpha * prod[k0:k1, rs, cs].sum(axis=0) + beta * C0[rs, cs].astype(np.longdouble)
                bound[rs, cs] = 2 * ((k1 - k0) * 128 + 2) * u * (abs(alpha) * absprod[k0:k1, rs, cs].sum(axis=0)
                                                              + beta * np.abs(C0[rs, cs]))
            err = np.abs(got[b].astype(np.longdouble) - ref).astype(np.float64)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), ((akm, bkm), (klo, khi), b, float((err / bound).max()))
        print(f"rounding fp32={fp32} tile={bt} orient={(akm, bkm)} k-range={(klo, khi)}: worst error / bound = {worst:.3g}")
    out = case.outside()
    assert np.array_equal(r["C"][0].view(np.uint64)[out], case.C.view(np.uint64)[out])


@pytest.mark.parametrize("batch", [3, 9])
@pytest.mark.parametrize("fp32", [False, True])
def test_every_form_gives_the_bits_of_the_plain_launch(ctx, fp32, batch):
    """The inputs of the rounding test at batches 3 and 9: for each tile size every sample of every other form equals
    the plain launch bit for bit, and every sample equals its own batch = 1 launch -- persist with the flat queue and
    with the XCD-affine queues, persist_reserved, plain in the XCD-aware order, and the two products of a dual launch
    against their own plain 64-tile launches.  Tile sizes 64 and 128 are not asserted equal; whether they are is
    printed."""
    from gpyreg_amd import _lib

    dtype = _lib.F32 if fp32 else _lib.F64
    ops = lambda b: _real_ops(b, fp32)
    mk = lambda akm, bkm, n, first=0: Case(RSHAPE, lambda b: ops(first + b), akm, bkm, -0.75, 1, 0, 0, 0, n)
    base = {}
    for bt in (128, 64):
        for akm, bkm in ((0, 1), (0, 0)):
            if (akm, bkm) == (0, 0) and bt == 128:
                continue  # (the m-major x m-major baseline serves the dual launch: 64-tiles only)
            case = mk(akm, bkm, batch)
            items = _ntiles(RSHAPE[0], RSHAPE[1], 0, bt) * batch
            plain = case.blocks(ctx.debug_gemm_form("plain", case.prod, batch=batch, tile=bt, flags=0, dtype=dtype)["C"][0])
            base[bt, akm, bkm] = plain
            for b in range(batch):
                one = mk(akm, bkm, 1, first=b)
                got = one.blocks(ctx.debug_gemm_form("plain", one.prod, batch=1, tile=bt, flags=0, dtype=dtype)["C"][0])
                assert np.array_equal(got[0].view(np.uint64), plain[b].view(np.uint64)), ("batch of one", bt, akm, bkm, b)
            others = [("plain", 16, 0), ("persist", 0, 4), ("persist", 8, 4), ("persist", 8, _slots_just_below(items, bt)),
                      ("persist_reserved", 8, 4), ("persist_reserved", 0, _slots_just_below(items, bt))]
            for form, flags, slots in others:
                r = ctx.debug_gemm_form(form, case.prod, batch=batch, tile=bt, flags=flags, block_slots=slots, dtype=dtype)
                if r is None:
                    print("persist_reserved: this context has no table of reserved CUs, not compared")
                    continue
                got = case.blocks(r["C"][0])
                assert np.array_equal(got.view(np.uint64), plain.view(np.uint64)), (form, flags, slots, bt, akm, bkm)
    for flags in (0, 16):
        c1, c2 = mk(0, 0, batch), mk(0, 1, batch)
        r = ctx.debug_gemm_form("dual", [c1.prod, c2.prod], batch=batch, flags=flags, dtype=dtype)
        assert np.array_equal(c1.blocks(r["C"][0]).view(np.uint64), base[64, 0, 0].view(np.uint64)), ("dual", 1, flags)
        assert np.array_equal(c2.blocks(r["C"][1]).view(np.uint64), base[64, 0, 1].view(np.uint64)), ("dual", 2, flags)
    same = np.array_equal(base[64, 0, 1].view(np.uint64), base[128, 0, 1].view(np.uint64))
    print(f"fp32={fp32} batch={batch}: 64-tiles and 128-tiles give {'the same' if same else 'different'} bits")
