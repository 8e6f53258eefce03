"""The index arithmetic of the GEMM launch forms enumerated on the host through gpc_debug_gemm_queues -- no device
needed.

Two kinds of arithmetic are pinned here (gemm.h):
  * tile_of_bx (gemm_tile's map bx -> (ti, tj)) and xcd_order (the XCD-aware order of gemm_kernel / gemm_dual_kernel)
    are __host__ __device__ inlines that the kernels call: the dispatch-order and XCD-order tests below check the
    arithmetic the device runs.
  * queue_nclass / queue_of / queue_total / queue_item / flat_queue_item RESTATE gemm_persist_kernel's queue arithmetic
    for the host (the kernel's text is untouched: calling them changed its register allocation).  The queue test below
    pins the restatement, which verify_queues uses too.  It cannot see the restatement drifting from the kernel; these
    tests of tests/test_gpu_gemm_forms.py would: test_queue_counters_reach_their_totals (every counter of a launch
    against the totals computed here), and the exact structural tests test_exact_every_form_tile_batch /
    test_exact_every_kmode_form (a (tile, sample) the kernel's queues drop or hand out twice is a wrong element under
    beta = 1)."""

import numpy as np
import pytest

NQ = 8
MODES = [  # (klo, khi, lower_only) the product launches: the cases of test_gemm_modes_fp64
    (0, 0, 0), (0, 0, 1), (0, 2, 0), (2, 0, 0), (0, 1, 0), (1, 0, 1),
]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from gpyreg_amd import _lib

    return _lib


def _documented_queues(ntiles, batch, affine):
    """The rule as gemm.h states it in words, written out independently: one flat queue, tile-major; or queue q =
    samples q, q + 8, ... (sample-major, tiles ascending) when batch >= 8, else sample q % batch and every nclass-th
    tile from tile q // batch, nclass = 8 // batch."""
    if not affine:
        return [[(i // batch, i % batch) for i in range(ntiles * batch)]] + [[] for _ in range(NQ - 1)]
    out = []
    for q in range(NQ):
        if batch >= NQ:
            out.append([(t, s) for s in range(q, batch, NQ) for t in range(ntiles)])
        else:
            nclass = NQ // batch
            out.append([(t, q % batch) for t in range(q // batch, ntiles, nclass)] if q < batch * nclass else [])
    return out


@pytest.mark.parametrize("flags", [0, 8])
def test_queues_hand_out_every_item_once_longest_first(lib, flags):
    """batch 1..20 x ntiles 1..40: the union of the queues is every (tile, sample) exactly once, every queue's tiles
    of one sample ascend (tile index = dispatch order = longest first), the totals the kernel compares its counter
    with are the queue lengths, and the queues are the ones gemm.h documents."""
    for batch in range(1, 21):
        for ntiles in range(1, 41):
            queues, totals, _, _ = lib.gemm_queues(ntiles, batch, flags)
            assert len(queues) == NQ
            items = [tuple(it) for q in queues for it in q]
            assert len(items) == ntiles * batch == int(totals.sum()), (batch, ntiles, totals)
            assert set(items) == {(t, s) for t in range(ntiles) for s in range(batch)}, (batch, ntiles)
            assert len(set(items)) == len(items), (batch, ntiles)
            for q, qi in enumerate(queues):
                assert len(qi) == totals[q], (batch, ntiles, q)
                for s in set(qi[:, 1].tolist()):
                    t = qi[qi[:, 1] == s, 0]
                    assert (np.diff(t) > 0).all(), (batch, ntiles, q, s)
            assert [[tuple(it) for it in q] for q in queues] == _documented_queues(ntiles, batch, flags & 8), \
                (batch, ntiles)
            if flags & 8 and batch < NQ:  # unused queues and classes: 8 = nclass * batch + the queues left idle
                used = sum(len(q) > 0 for q in queues)
                assert used == min(ntiles, NQ // batch) * batch, (batch, ntiles, used)


def _k_len(klo, khi, ti, tj, K):
    k0 = {0: 0, 1: ti * 128, 2: tj * 128}[klo]
    k1 = min({0: K, 1: (ti + 1) * 128, 2: (tj + 1) * 128}[khi], K)
    return max(k1 - k0, 0)


GRIDS = [(n, n) for n in range(1, 13)] + [(2, 5), (5, 2), (1, 7), (7, 1), (3, 12), (12, 3)]


@pytest.mark.parametrize("klo", [0, 1, 2])
@pytest.mark.parametrize("khi", [0, 1, 2])
@pytest.mark.parametrize("lower", [0, 1])
def test_dispatch_order_is_a_bijection_onto_the_launched_tiles(lib, klo, khi, lower):
    """bx -> (ti, tj) for every ordering mode: each launched tile exactly once (lower_only: the tiles with tj <= ti),
    on square grids up to 12 x 12 and rectangular ones; for the modes the product launches the k-length never grows
    along the dispatch order (longest first)."""
    for tm, tn in GRIDS:
        if lower and tm != tn:
            continue
        want = {(i, j) for i in range(tm) for j in range(tn) if not lower or j <= i}
        _, _, tiles, _ = lib.gemm_queues(len(want), 1, 0, tm, tn, klo, khi, lower, want_tiles=True)
        got = [tuple(t) for t in tiles]
        assert len(got) == len(want) and set(got) == want, (tm, tn, got)
        if (klo, khi, lower) in MODES:
            K = max(tm, tn) * 128
            lens = [_k_len(klo, khi, ti, tj, K) for ti, tj in got]
            assert all(a >= b for a, b in zip(lens, lens[1:])), (tm, tn, lens)


def test_dispatch_order_refuses_a_tile_count_that_is_not_the_launchs(lib):
    with pytest.raises(RuntimeError):
        lib.gemm_queues(7, 1, 0, 3, 3, 0, 0, 0, want_tiles=True)
    with pytest.raises(RuntimeError):
        lib.gemm_queues(9, 1, 0, 3, 3, 0, 0, 1, want_tiles=True)


def test_xcd_order_is_a_bijection_with_one_contiguous_range_per_xcd(lib):
    """Grids (x, y), x in 1..40, y in 8..20, flag 16: the map L -> (bx, by) is a bijection on [0, x y); workgroup L
    (on XCD L % 8) takes item (L % 8) * (x y // 8) + L // 8 of the sample-major item list, so every XCD works through
    one contiguous range; the x y % 8 items at the end keep their place.  Below 8 samples, or without the flag, the
    order is the identity."""
    for x in range(1, 41):
        for y in range(8, 21):
            _, _, _, xcd = lib.gemm_queues(x, y, 16, want_xcd=True)
            wk = (xcd[:, :, 1].astype(np.int64) * x + xcd[:, :, 0]).ravel()  # item taken by workgroup L, L ascending
            assert (xcd[:, :, 0] >= 0).all() and (xcd[:, :, 0] < x).all() and (xcd[:, :, 1] < y).all()
            assert np.array_equal(np.sort(wk), np.arange(x * y)), (x, y)
            per = x * y // 8
            L = np.arange(x * y)
            want = np.where(L < 8 * per, (L % 8) * per + L // 8, L)
            assert np.array_equal(wk, want), (x, y)
    for x, y, flags in ((5, 7, 16), (5, 7, 24), (5, 9, 0), (5, 9, 8)):
        _, _, _, xcd = lib.gemm_queues(x, y, flags, want_xcd=True)
        bx, by = np.meshgrid(np.arange(x), np.arange(y))
        assert np.array_equal(xcd[:, :, 0], bx) and np.array_equal(xcd[:, :, 1], by), (x, y, flags)
