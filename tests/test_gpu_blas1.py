"""Every kernel of gpyreg_amd/csrc/blas1.h on its own: ONE launch through gpc_debug_blas1, with the grid and block of
the production call site, against the defining formula of the kernel's comment in np.longdouble (tests/blas1_ref.py:
the inputs, the references and the derived bound; tests/test_blas1_cpu.py shows the three consistent without a device).

What these tests see that the end-to-end tests cannot: every operand is surrounded by NaN wherever the kernel's
contract says it does not read (the tiles of W above the diagonal, the columns left of a diagonal block, the rows past
nrows, vector entries past n), every output buffer starts as NaN and is followed by a NaN guard, and kernels that update
in place start from distinct values -- an unmasked read, a skipped entry, a write outside the contract each change a
checked value.  Pure moves, casts, negation and mirroring are held to the bit; arithmetic to the derived bound, with no
constant added; the forms that claim the same bits (low-register = chip-filling, with = without the fused z.z, the
fused z.z = dot_kernel, grad_tail's mean / noise slots = mat_t_vec_kernel) are compared with np.array_equal.

Both dtypes; the shapes are the smallest at which each piece of index arithmetic changes behaviour (blas1_ref.NPADS
and the case generators there).  Each test prints the worst |error| / bound per kernel; test_report prints the table.

Measured on the MI355X, worst |error| / bound over all cases (the pure moves -- extract, neg_sym, pad_load, pad_rect,
rect_copy, grow_copy -- have no bound: to the bit):

    kernel            f64    f32        kernel            f64    f32
    trmv              0.468  0.428      colsum_prod       0.491  0.316
    trmv_low          0.468  0.376      colsum_vec        0.481  0.492
    gemv_sub          0.007  0.007      diagq             0.291  0.237
    trmv_t_part       0.015  0.014      trace_plane       <1e-3  <1e-3
    trmv_t_part_low   0.015  0.014      load_K            0.486  0.999
    trmv_t_sum        0.271  0.271      append_row        0.489  0.970
    dot               0.210  0.210      append_low        0.278  0.996
    mat_t_vec         0.210  0.210      grad_tail         0.225  0.225

(The figures near 0.5 are single products or sums of one term, m = 1: half an ulp against a bound of one.  The fp32
figures near 1 of load_K and the append kernels are the storage rounding of a result kept in fp32, half an ulp of a
value just above a power of two against 2^-24 |ref|.)  No kernel needed a change.
"""

import numpy as np
import pytest

import blas1_ref as br
from blas1_ref import F32, F64

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
WORST = {}


@pytest.fixture(scope="module")
def ctx():
    from gpyreg_amd import _lib

    return _lib.context(0)


def _run(ctx, case):
    got = case.run(ctx)
    ratio = br.check(case, got)
    key = (case.which, br.DT_NAME[case.dtype])
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    return got


def _show(*kernels):
    print("\nworst |error| / bound: " + "  ".join("%s/%s %.3g" % (k[0], k[1], v) for k, v in sorted(WORST.items())
                                                   if k[0] in kernels))


def _same(a, b, what):
    assert np.array_equal(a, b, equal_nan=True), (what, np.flatnonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))[:5].tolist())


@DTYPES
@pytest.mark.parametrize("batch", br.BATCHES)
@pytest.mark.parametrize("npad", br.NPADS)
def test_triangular_products_and_their_forms(ctx, dtype, npad, batch):
    # z = W r: the chip-filling and the low-register kernel, the same bits
    (z,) = _run(ctx, br.trmv(dtype, npad, batch))
    (zl,) = _run(ctx, br.trmv(dtype, npad, batch, low=True))
    _same(z, zl, "trmv_low_kernel = trmv_kernel(row0 = 0)")
    # W^T z, pass 1: UNR = 8 and UNR = 3, with and without the fused z.z
    c8 = br.trmv_t_part(dtype, npad, batch, quad=True)
    p8, q8 = _run(ctx, c8)
    p3, q3 = _run(ctx, br.trmv_t_part(dtype, npad, batch, quad=True, low=True))
    _same(p8, p3, "trmv_t_part_low_kernel = trmv_t_part_kernel<T, 8>: partials")
    _same(q8, q3, "trmv_t_part_low_kernel = trmv_t_part_kernel<T, 8>: z.z")
    (p8n,) = _run(ctx, br.trmv_t_part(dtype, npad, batch, quad=False))
    (p3n,) = _run(ctx, br.trmv_t_part(dtype, npad, batch, quad=False, low=True))
    _same(p8, p8n, "trmv_t_part with and without quad")
    _same(p3, p3n, "trmv_t_part_low with and without quad")
    (qd,) = _run(ctx, br.dot_self(dtype, c8.ins[1]))
    _same(q8, qd, "the fused z.z of trmv_t_part = dot_kernel(z, z, npad, npad)")
    # pass 2
    for scale in (True, False):
        _run(ctx, br.trmv_t_sum(dtype, npad, batch, scale))
    _show("trmv", "trmv_low", "trmv_t_part", "trmv_t_part_low", "trmv_t_sum")


@DTYPES
@pytest.mark.parametrize("batch", br.BATCHES)
def test_blocked_forward_solve_pieces(ctx, dtype, batch):
    for row0, rows in br.TRMV_BLOCKS:
        _run(ctx, br.trmv(dtype, 640, batch, row0, rows))
    for blk in br.GEMV_BLOCKS:
        _run(ctx, br.gemv_sub(dtype, 640, batch, *blk))
    _show("trmv", "gemv_sub")


@DTYPES
def test_reductions(ctx, dtype):
    names = set()
    for case in br.reduction_cases(dtype):
        if case.which in ("dot", "mat_t_vec", "colsum_prod", "colsum_vec", "diagq", "trace_plane"):
            _run(ctx, case)
            names.add(case.which)
    assert len(names) == 6
    _show(*names)


@DTYPES
def test_grad_tail_and_its_slots_against_mat_t_vec(ctx, dtype):
    for case in br.grad_tail_cases(dtype):
        got = _run(ctx, case)
        n, batch = case.ip[2], case.ip[6]
        for k, Mat, vec in ((1, case.dm1, case.alpha), (2, case.dsn2, case.diagq)):
            if Mat is None:  # (no such slots: the buffer is its guard alone, which _run has checked)
                continue
            (ref,) = _run(ctx, br.mat_t_vec(dtype, n, Mat.shape[2], batch, vstride=case.vstride, Mat=Mat, vec=vec))
            _same(got[k], ref, "grad_tail slot = mat_t_vec_kernel: " + case.name)
    _show("grad_tail", "mat_t_vec")


@DTYPES
def test_layout_and_copies(ctx, dtype):
    for case in br.copy_cases(dtype):
        _run(ctx, case)
    _show("load_K")


@DTYPES
def test_rank_one_append(ctx, dtype):
    for case in br.append_cases(dtype):
        _run(ctx, case)
    _show("append_row", "append_low")


def test_the_hook_keeps_nothing_between_calls(ctx):
    """Buffers live for one call: a call of another size between two runs of a case changes nothing, and what the case
    does not write is the NaN fill, not the other call's data."""
    small = br.trmv(F64, 640, 1, 128, 128)  # writes 128 of 640 outputs
    first = _run(ctx, small)
    _run(ctx, br.grow_copy(F64, 128, 256, 2))
    _run(ctx, br.trmv(F64, 256, 3))
    again = _run(ctx, small)
    _same(first[0], again[0], "the same call after calls of other sizes")
    assert np.isnan(again[0][:128]).all() and np.isnan(again[0][256:]).all()


@DTYPES
def test_unmasked_tile_reads_need_a_finite_vector_and_nothing_more(ctx, dtype):
    """trmv reads a row to the end of its diagonal tile and trmv_t_part the whole diagonal tile: the exact zeros of W
    above the diagonal meet vector entries the formula never names.  Their VALUES change no bit of the rows that do not
    own them (here: the padding entries of r against the rows before the padding); a NaN there would poison the tile,
    which is why blas1.h asks for a finite vector and the hook refuses another."""
    npad, pad = 384, 5
    case = br.trmv(dtype, npad, 2)
    W, r = case.ins
    (z,) = case.run(ctx)
    r2 = r.copy()
    r2[:, npad - pad:] = [7.5, -1e30, 0.0, 3e-300, -2.0]
    (z2,) = ctx.debug_blas1("trmv", case.ip, [W, r2], case.out_sizes, dtype=dtype)
    z, z2 = z[:2 * npad].reshape(2, npad), z2[:2 * npad].reshape(2, npad)
    _same(z[:, :npad - pad], z2[:, :npad - pad], "the padding entries of r reach no row before the padding")
    assert np.array_equal(z2[:, npad - pad:], r2[:, npad - pad:]), "identity rows on the padding"
    r2[1, npad - 1] = np.nan
    with pytest.raises(RuntimeError, match="finite"):
        ctx.debug_blas1("trmv", case.ip, [W, r2], case.out_sizes, dtype=dtype)
    with pytest.raises(RuntimeError, match="finite"):
        ctx.debug_blas1("trmv_t_part", [npad, 2, 0], [W, r2], [2 * (npad // 128) * npad], dtype=dtype)


def test_the_hook_refuses_launches_outside_its_buffers(ctx):
    W = np.zeros((1, 128, 128))
    for ip, ins, sizes in (([128, 1, 0, 128], [W, np.zeros(127)], [128]),  # r too short
                           ([128, 1, 0, 128], [W, np.zeros(128)], [127]),  # z too short
                           ([128, 1, 64, 64], [W, np.zeros(128)], [128]),  # a block off the tile grid
                           ([128, 1, 128, 128], [W, np.zeros(128)], [128])):  # rows past npad
        with pytest.raises(RuntimeError, match="gpc_debug_blas1"):
            ctx.debug_blas1("trmv", ip, ins, sizes)
    with pytest.raises(RuntimeError, match="gpc_debug_blas1"):
        ctx.debug_blas1("append_row", [128, 128, 1], [W, W, np.zeros(128), np.zeros(128), np.zeros(5), np.zeros(128)],
                        [128 * 128, 128 * 128, 128])  # row n = npad


def test_report():
    kernels = sorted({k for k, _ in WORST})
    print("\nworst |error| / derived bound per kernel (0: exact results only)\n%-18s %8s %8s" % ("kernel", "f64", "f32"))
    for k in kernels:
        print("%-18s %8.3g %8.3g" % (k, WORST.get((k, "f64"), float("nan")), WORST.get((k, "f32"), float("nan"))))
