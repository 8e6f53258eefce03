"""The zero-skipping masks of the fp64 128-tile GEMM (gemm.h: GemmArgs::tri) enumerated on the host through
gpc_debug_tri_masks -- no device needed -- against a brute-force triangular predicate over the ELEMENTS of a diagonal
128-block: for each kind and each of the eight k-slabs no product that can be non-zero is dropped, the four waves
together own every 16 x 16 fragment of the tile exactly once, and the executed share is the one the design states.

Shares.  A triangular kind issues 1,1,2,2,3,3,4,4 (FIRST) or 4,4,3,3,2,2,1,1 (LAST) of a wave's four fragment rows or
columns over the slabs, the same in every wave: 20 of 32.  A diagonal output tile of a diag-lower launch needs the
fragments with fragment row >= fragment column: 10, 10, 10 and 6 of a wave's 16, and exactly those are stored.  Every
wave ISSUES the 10 with i >= j, though: the wave (wr, wc) = (0, 1) computes its four i = j fragments with the others
and drops them -- the block is as slow as its busiest wave either way, and one mask for all waves keeps every wave on
the same barrier sequence.  So the issued share of such a tile is 40 of 64, the stored and needed share 36 of 64."""

import numpy as np
import pytest

A_FIRST, A_LAST, B_FIRST, B_LAST, DIAG = 1, 2, 3, 4, 8


@pytest.fixture(scope="module")
def lib():
    from gpyreg_amd import _lib

    return _lib


def _needed_fragment(kind, f, s):
    """Brute force over the elements: can operand fragment f (rows of A / columns of B: 16 f .. 16 f + 15) hold a
    non-zero in slab s (k = 16 s .. 16 s + 15) of a lower triangular diagonal block?"""
    idx, k = np.arange(16 * f, 16 * f + 16)[:, None], np.arange(16 * s, 16 * s + 16)[None, :]
    nonzero = (k >= idx) if kind in (A_FIRST, B_FIRST) else (k <= idx)
    return bool(nonzero.any())


def test_waves_own_every_fragment_once(lib):
    rows, cols, _, _ = lib.tri_masks(A_FIRST, 0, 0)
    owned = np.zeros((8, 8), dtype=int)
    for w in range(4):
        for i in range(4):
            for j in range(4):
                owned[rows[w, i], cols[w, j]] += 1
    assert (owned == 1).all()
    for w in range(4):  # cyclic: wave row wr owns 2 i + wr, wave column wc owns 2 j + wc
        assert rows[w].tolist() == [2 * i + w // 2 for i in range(4)]
        assert cols[w].tolist() == [2 * j + w % 2 for j in range(4)]


@pytest.mark.parametrize("kind", [A_FIRST, A_LAST, B_FIRST, B_LAST])
def test_triangular_kinds_drop_nothing_and_issue_20_of_32(lib, kind):
    issued_total, needed_by_wave = 0, np.zeros(4, dtype=int)
    per_slab = []
    for s in range(8):
        rows, cols, issued, stored = lib.tri_masks(kind, 0, s)
        assert stored.all()
        for w in range(4):
            own = rows[w] if kind in (A_FIRST, A_LAST) else cols[w]
            for i in range(4):
                for j in range(4):
                    f = own[i] if kind in (A_FIRST, A_LAST) else own[j]
                    need = _needed_fragment(kind, int(f), s)
                    needed_by_wave[w] += need
                    assert issued[w, i, j] or not need, (kind, s, w, i, j)
        assert (issued == issued[0]).all(), "one mask for all waves"
        per_slab.append(int(issued[0].sum()) // 4)
        issued_total += int(issued.sum())
    want = [1, 1, 2, 2, 3, 3, 4, 4] if kind in (A_FIRST, B_FIRST) else [4, 4, 3, 3, 2, 2, 1, 1]
    assert per_slab == want
    assert issued_total * 32 == 20 * (4 * 16 * 8)
    # the busier wave row / column needs all it issues: 20 x 4 of its 128 fragment-slabs, the other one 16 x 4
    assert sorted(needed_by_wave.tolist()) == [64, 64, 80, 80]


@pytest.mark.parametrize("tri", [DIAG, A_FIRST | DIAG])
def test_diag_lower_stores_what_is_needed(lib, tri):
    for s in range(8):
        rows, cols, issued, stored = lib.tri_masks(tri, 1, s)
        need = rows[:, :, None] >= cols[:, None, :]
        assert np.array_equal(stored.astype(bool), need)
        assert not (need & ~issued.astype(bool)).any()
        assert sorted(int(x) for x in need.sum(axis=(1, 2))) == [6, 10, 10, 10]
        assert int(stored.sum()) == 36 and int(issued.sum()) == 40
        assert (issued.sum(axis=(1, 2)) == 10).all()
    # an off-diagonal tile of the same launch: the triangular kind alone, everything stored
    for s in range(8):
        _, _, issued, stored = lib.tri_masks(tri, 0, s)
        _, _, issued_kind, _ = lib.tri_masks(tri & 7, 0, s)
        assert stored.all() and np.array_equal(issued, issued_kind)


def test_nothing_guaranteed_issues_everything(lib):
    for s in range(8):
        _, _, issued, stored = lib.tri_masks(0, 0, s)
        assert issued.all() and stored.all()
    with pytest.raises(RuntimeError):
        lib.tri_masks(5, 0, 0)
    with pytest.raises(RuntimeError):
        lib.tri_masks(1, 0, 8)


def test_the_launches_of_the_plan_get_their_instantiation(lib):
    """gemm.h: tri_usable, the function launch_gemm_bt calls, for the (orientation, k-range, guarantee) of every launch of
    plan.h that names a triangular operand: each gets the instantiation of its kind -- a launcher that quietly ran the
    plain kernel would return 0 here -- and nothing else gets one."""
    n = 1024
    # (tri, a_kmajor, b_kmajor, klo, khi, lower_only): W^T W (with and without diag-lower), W21, U, T21, syrk
    plan = [(A_FIRST, 1, 1, 1, 0, 1), (A_FIRST | DIAG, 1, 1, 1, 0, 1), (A_LAST, 0, 1, 0, 1, 0), (B_FIRST, 0, 1, 2, 0, 0),
            (B_LAST, 0, 0, 0, 2, 0), (DIAG, 0, 0, 0, 0, 1)]
    for tri, akm, bkm, klo, khi, lower in plan:
        assert lib.tri_usable(tri, akm, bkm, klo, khi, lower, n, n, n) == tri
        assert lib.tri_usable(tri, akm, bkm, klo, khi, lower, n, n, n, tile=64) == 0  # the 64-tile kernels know no masks
        assert lib.tri_usable(tri, akm, bkm, klo, khi, lower, n, n, n, dtype=lib.F32) == 0  # nor does fp32
        assert lib.tri_usable(0, akm, bkm, klo, khi, lower, n, n, n) == 0  # nothing guaranteed, nothing skipped
    # a kind beside a k-range that does not put its triangular block at that end, or in another orientation: unused
    assert lib.tri_usable(A_FIRST, 1, 1, 0, 0, 1, n, n, n) == 0
    assert lib.tri_usable(B_FIRST, 0, 1, 0, 0, 0, n, n, n) == 0
    assert lib.tri_usable(A_LAST, 0, 1, 0, 0, 0, n, n, n) == 0
    assert lib.tri_usable(B_LAST, 0, 0, 0, 0, 0, n, n, n) == 0
    assert lib.tri_usable(B_LAST, 1, 0, 0, 2, 0, n, n, n) == 0
    assert lib.tri_usable(A_LAST, 0, 1, 0, 1, 0, n, n, n - 128) == 0  # K cut short of the last tile row's diagonal block
    assert lib.tri_usable(B_LAST, 0, 0, 0, 2, 0, n, n, n - 128) == 0
    assert lib.tri_usable(DIAG, 0, 0, 0, 0, 0, n, n, n) == 0  # diag-lower needs a lower_only launch
    assert lib.tri_usable(A_FIRST | DIAG, 1, 1, 1, 0, 0, n, n, n) == A_FIRST
