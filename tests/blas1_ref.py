"""References, inputs and bounds for the direct tests of gpyreg_amd/csrc/blas1.h (tests/test_gpu_blas1.py runs the
kernels through gpc_debug_blas1, tests/test_blas1_cpu.py runs a NumPy emulation of their summation orders on the same
inputs).

Every case is built by a function of this module: the operands of one launch (seeded, distinct per position and batch
member, mixed signs, magnitudes over three decades, never symmetric; whatever lies outside a kernel's contract is NaN),
the expected result of every output buffer and how it is compared:

* ``exact``: the expected contents, compared with ``np.array_equal`` (NaN = NaN: "still the hook's fill");
* ``tol``: where the result is arithmetic, the mask of the entries held to a DERIVED bound against the defining formula
  of the kernel's comment, evaluated in np.longdouble over exactly the index set the comment states:

      |device - ref| <= m 2^-52 sum |a_i b_i|  +  k 2^-52 |ref|  +  [stored as float] 2^-24 |ref|

  m products accumulated in fp64 in any order, with or without FMA contraction (gamma_m at u = 2^-53, doubled); k
  further roundings of the result (a division, a subtraction from the operand updated in place); the storage rounding
  of a result kept in fp32.  Operands that live on the device as T are rounded to float32 beforehand, so the upload is
  exact and there is no storage term for the inputs.  The longdouble reference's own error (2^-11 of the bound) is
  ignored.  Nothing else is added.
* ``skip``: entries no assertion is made about (the padding columns of the column sums).
"""

import zlib

import numpy as np

LD = np.longdouble
F64, F32 = 0, 1
DT_NAME = {F64: "f64", F32: "f32"}
VEC = {F64: 2, F32: 4}  # MM<T>::VEC: elements per 16-byte load
GUARD = 128
U52, U24 = LD(2.0) ** -52, LD(2.0) ** -24
TILE = 128
NAN = np.nan


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def rnd(rng, *shape):
    return rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-1.5, 1.5, shape)


def as_T(a, dtype):
    """What the device holds of an operand stored as T: the upload of these values is exact."""
    with np.errstate(invalid="ignore"):
        return a.astype(np.float32).astype(np.float64) if dtype == F32 else a


def store(ref, dtype):
    """The NumPy cast of a result stored as T (pure moves: the expected bits)."""
    return as_T(np.asarray(ref, dtype=np.float64), dtype)


def bound(m, sabs, ref, extra=0, stored=F64):
    b = np.asarray(m, dtype=LD) * U52 * sabs + LD(extra) * U52 * np.abs(ref)
    return b + U24 * np.abs(ref) if stored == F32 else b


class Out:
    """One output buffer of a case: expected contents and how to compare (module docstring)."""

    def __init__(self, exact, tol=None, ref=None, bnd=None, skip=None):
        self.exact = np.asarray(exact, dtype=np.float64).ravel()
        n = self.exact.size
        self.tol = np.zeros(n, bool) if tol is None else np.broadcast_to(tol, np.shape(exact)).ravel()
        self.ref = None if ref is None else np.broadcast_to(ref, np.shape(exact)).astype(LD).ravel()
        self.bnd = None if bnd is None else np.broadcast_to(bnd, np.shape(exact)).astype(LD).ravel()
        self.skip = np.zeros(n, bool) if skip is None else np.broadcast_to(skip, np.shape(exact)).ravel()

    @property
    def size(self):
        return self.exact.size


class Case:
    def __init__(self, which, dtype, ip, ins, outs, name, emu=None):
        self.which, self.dtype, self.ip, self.ins, self.outs, self.name, self.emu = which, dtype, ip, ins, outs, name, emu

    @property
    def out_sizes(self):
        return [o.size for o in self.outs]

    def run(self, ctx):
        return ctx.debug_blas1(self.which, self.ip, self.ins, self.out_sizes, dtype=self.dtype)


def check(case, got, guard=True):
    """Compare the buffers ``got`` with the case's expectation; returns the worst |error| / bound (0 without one)."""
    assert len(got) == len(case.outs), (case.name, "number of outputs")
    worst = 0.0
    for k, (o, g) in enumerate(zip(case.outs, got)):
        g = np.asarray(g).ravel()
        if guard:
            assert g.size == o.size + GUARD, (case.name, k, "the buffer comes back with its guard")
            assert np.isnan(g[o.size:]).all(), (case.name, k, "written past the end of the buffer",
                                                np.flatnonzero(~np.isnan(g[o.size:]))[:5].tolist())
            g = g[:o.size]
        assert g.size == o.size
        ex = ~o.tol & ~o.skip
        bad = ex & ~((g == o.exact) | (np.isnan(g) & np.isnan(o.exact)))
        assert not bad.any(), (case.name, k, "entries that must match to the bit (or stay untouched) differ",
                               np.flatnonzero(bad)[:5].tolist(), g[bad][:5].tolist(), o.exact[bad][:5].tolist())
        if o.tol.any():
            t = o.tol
            assert np.isfinite(g[t]).all(), (case.name, k, "NaN / inf in a result: storage outside the contract was read",
                                             np.flatnonzero(t & ~np.isfinite(g))[:5].tolist())
            err = np.abs(g[t].astype(LD) - o.ref[t])
            b = o.bnd[t]
            assert (err[b == 0] == 0).all(), (case.name, k, "an empty or exact sum is not exact")
            ratio = float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
            worst = max(worst, ratio)
            assert ratio <= 1.0, (case.name, k, "outside the derived bound: ratio", ratio,
                                  np.flatnonzero(t)[np.flatnonzero(err > b)[:5]].tolist())
    return worst


# ---- the summation orders of blas1.h in fp64 (no FMA), for tests/test_blas1_cpu.py -----------------------------------
def _seq(terms, axis):
    """Left-to-right sum along ``axis``, starting from 0.0 as the kernels do."""
    terms = np.moveaxis(terms, axis, 0)
    s = np.zeros(terms.shape[1:])
    for t in terms:
        s = s + t
    return s


def _pad_last(terms, mult):
    n = terms.shape[-1]
    extra = (-n) % mult
    if extra:  # (the lanes without a term add nothing)
        terms = np.concatenate([terms, np.zeros(terms.shape[:-1] + (extra,))], axis=-1)
    return terms


def wave_sum(v):
    """wave_sum of common.h: the xor butterfly over the last axis (64 lanes); every lane ends with the total."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v


def lane_strided(terms, vec):
    """trmv / gemv_sub: lane l takes elements [l vec, l vec + vec) of every stretch of 64 vec, in order; then wave_sum."""
    t = _pad_last(terms, 64 * vec)
    t = t.reshape(t.shape[:-1] + (-1, 64, vec))
    t = np.moveaxis(t, -2, -3)  # (..., 64, stretches, vec)
    s = _seq(t.reshape(t.shape[:-2] + (-1,)), -1)
    return wave_sum(s)[..., 0]


def block_sum(terms):
    """dot / mat_t_vec / grad_tail / diagq / trace_plane: thread t takes every 256th term, then block_sum_256."""
    t = _pad_last(terms, 256)
    t = t.reshape(t.shape[:-1] + (-1, 256))
    s = _seq(t, -2)  # (..., 256)
    w = wave_sum(s.reshape(s.shape[:-1] + (4, 64)))[..., 0]  # (..., 4)
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def four_waves(terms):
    """colsum_* / trmv_t_part: rows on axis -2; wave w takes every fourth row from w, then red[0] + .. + red[3]."""
    w = [_seq(terms[..., q::4, :], -2) if terms.shape[-2] > q else np.zeros(terms.shape[:-2] + terms.shape[-1:])
         for q in range(4)]
    return ((w[0] + w[1]) + w[2]) + w[3]


# ---- operands -----------------------------------------------------------------------------------------------------------
def make_W(rng, batch, npad, dtype, pad_rows=5):
    """W = L^-1 as the factorization leaves it: the lower triangle arbitrary, exact zeros above the diagonal inside each
    diagonal tile, identity rows on the padding -- and NaN in every tile strictly above the diagonal (storage the
    factorization never writes: in a workspace shared by all problem sizes it holds another problem's leftovers)."""
    W = rnd(rng, batch, npad, npad)
    i, j = np.indices((npad, npad))
    W[:, j > i] = 0.0
    pad = i >= npad - pad_rows
    W[:, pad & (j < i)] = 0.0
    W[:, pad & (i == j)] = 1.0
    W[:, (j // TILE) > (i // TILE)] = NAN
    return as_T(W, dtype)


def _masked(a, mask):
    """``a`` in longdouble with everything outside ``mask`` (NaNs included) replaced by 0."""
    return np.where(mask, a, 0.0).astype(LD)


# ---- triangular mat-vecs ---------------------------------------------------------------------------------------------------
def trmv(dtype, npad, batch, row0=0, rows=None, low=False):
    rows = npad if rows is None else rows
    rng = _rng("trmv", dtype, npad, batch, row0, rows)
    W, r = make_W(rng, batch, npad, dtype), rnd(rng, batch, npad)
    i, j = np.indices((npad, npad))
    blk = (np.arange(npad) >= row0) & (np.arange(npad) < row0 + rows)
    if row0 > 0 or rows < npad:
        W[:, ~blk, :] = NAN
        W[:, :, :row0] = NAN
        r[:, ~blk] = NAN
    use = (j <= i) & (j >= row0) & blk[:, None]
    Wl, rl = _masked(W, use), _masked(r, blk)
    ref = (Wl * rl[:, None, :]).sum(-1)
    sabs = np.abs(Wl * rl[:, None, :]).sum(-1)
    m = (np.arange(npad) - row0 + 1).clip(1)
    exact = np.where(blk, 0.0, NAN) * np.ones((batch, 1))
    out = Out(exact, tol=blk[None, :] & np.ones((batch, 1), bool), ref=ref, bnd=bound(m, sabs, ref))

    def emu():
        z = np.full((batch, npad), NAN)
        for t0 in range(row0, row0 + rows, TILE):  # the rows of one tile read the same columns: row0 .. the tile's end
            kend = t0 + TILE
            z[:, t0:kend] = lane_strided(W[:, t0:kend, row0:kend] * r[:, None, row0:kend], VEC[dtype])
        return [z]

    if low:
        return Case("trmv_low", dtype, [npad, batch], [W, r], [out], "trmv_low %s npad=%d b=%d" % (DT_NAME[dtype], npad, batch),
                    emu)
    return Case("trmv", dtype, [npad, batch, row0, rows], [W, r], [out],
                "trmv %s npad=%d b=%d block=(%d,%d)" % (DT_NAME[dtype], npad, batch, row0, rows), emu)


def gemv_sub(dtype, npad, batch, row0, nrows, col0, ncols):
    rng = _rng("gemv_sub", dtype, npad, batch, row0, nrows, col0, ncols)
    A = np.full((batch, npad, npad), NAN)
    A[:, row0:row0 + nrows, col0:col0 + ncols] = as_T(rnd(rng, batch, nrows, ncols), dtype)
    z = np.full((batch, npad), NAN)
    z[:, col0:col0 + ncols] = rnd(rng, batch, ncols)
    r = rnd(rng, batch, npad)
    rows = np.zeros(npad, bool)
    rows[row0:row0 + nrows] = True
    prod = A[:, row0:row0 + nrows, col0:col0 + ncols].astype(LD) * z[:, None, col0:col0 + ncols].astype(LD)
    ref = r.astype(LD)
    ref[:, rows] = ref[:, rows] - prod.sum(-1)
    sabs = np.zeros((batch, npad), LD)
    sabs[:, rows] = np.abs(prod).sum(-1)
    out = Out(r, tol=rows[None, :] & np.ones((batch, 1), bool), ref=ref, bnd=bound(ncols, sabs, ref, extra=1))

    def emu():
        o = r.copy()
        s = lane_strided(A[:, row0:row0 + nrows, col0:col0 + ncols] * z[:, None, col0:col0 + ncols], VEC[dtype])
        o[:, rows] = o[:, rows] - s
        return [o]

    return Case("gemv_sub", dtype, [npad, batch, row0, nrows, col0, ncols], [A, z, r], [out],
                "gemv_sub %s npad=%d b=%d (%d,%d,%d,%d)" % (DT_NAME[dtype], npad, batch, row0, nrows, col0, ncols), emu)


def trmv_t_part(dtype, npad, batch, quad=True, low=False):
    rng = _rng("trmv_t_part", dtype, npad, batch)  # (the same operands for every form: they are compared to the bit)
    W, z = make_W(rng, batch, npad, dtype), rnd(rng, batch, npad)
    nch = npad // TILE
    ch, k = np.indices((nch, npad))
    live = ch >= k // TILE  # the chunks at or below the diagonal tile of column k; the others are empty sums
    ref = np.zeros((batch, nch, npad), LD)
    sabs = np.zeros((batch, nch, npad), LD)
    for c in range(nch):
        cols = (c + 1) * TILE
        p = W[:, c * TILE:cols, :cols].astype(LD) * z[:, c * TILE:cols, None].astype(LD)
        ref[:, c, :cols], sabs[:, c, :cols] = p.sum(1), np.abs(p).sum(1)
    outs = [Out(np.zeros((batch, nch, npad)), tol=live[None] & np.ones((batch, 1, 1), bool), ref=ref,
                bnd=bound(TILE, sabs, ref))]
    if quad:
        zz = z.astype(LD) ** 2
        outs.append(Out(np.zeros(batch), tol=np.ones(batch, bool), ref=zz.sum(-1), bnd=bound(npad, zz.sum(-1), zz.sum(-1))))

    def emu():
        part = np.zeros((batch, nch, npad))
        for c in range(nch):
            cols = (c + 1) * TILE
            part[:, c, :cols] = four_waves(W[:, c * TILE:cols, :cols] * z[:, c * TILE:cols, None])
        return [part] + ([block_sum(z * z)] if quad else [])

    return Case("trmv_t_part_low" if low else "trmv_t_part", dtype, [npad, batch, int(quad)], [W, z], outs,
                "trmv_t_part%s %s npad=%d b=%d quad=%d" % ("_low" if low else "", DT_NAME[dtype], npad, batch, quad), emu)


def trmv_t_sum(dtype, npad, batch, scale):
    rng = _rng("trmv_t_sum", npad, batch)
    nch = npad // TILE
    part = rnd(rng, batch, nch, npad)
    ch, k = np.indices((nch, npad))
    live = ch >= k // TILE
    part[:, ~live] = NAN  # what pass 1 leaves above the diagonal is not this kernel's to read
    sp = rnd(rng, batch, 4)
    pl = _masked(part, live[None])
    div = sp[:, 3:4].astype(LD) if scale else LD(1)
    ref, sabs = pl.sum(1) / div, np.abs(pl).sum(1) / np.abs(div)
    m = nch - np.arange(npad) // TILE
    out = Out(np.zeros((batch, npad)), tol=np.ones((batch, npad), bool), ref=ref, bnd=bound(m, sabs, ref, extra=int(scale)))

    def emu():
        o = np.zeros((batch, npad))
        for t in range(nch):  # column tile t: the chunks t .. nch - 1, in order
            o[:, t * TILE:(t + 1) * TILE] = _seq(part[:, t:, t * TILE:(t + 1) * TILE], 1)
        return [o / sp[:, 3:4] if scale else o]

    return Case("trmv_t_sum", dtype, [npad, batch, 4, 3], [part, sp if scale else None], [out],
                "trmv_t_sum npad=%d b=%d scale=%d" % (npad, batch, scale), emu)


# ---- reductions ------------------------------------------------------------------------------------------------------------
def _vec(rng, batch, n, stride):
    v = np.full((batch, stride), NAN)
    v[:, :n] = rnd(rng, batch, n)
    return v


def dot(dtype, n, batch):
    stride = n + 7
    rng = _rng("dot", n, batch, stride)
    return _dot_case(dtype, n, batch, stride, _vec(rng, batch, n, stride), _vec(rng, batch, n, stride))


def _dot_case(dtype, n, batch, stride, x, y):
    p = x[:, :n].astype(LD) * y[:, :n].astype(LD)
    out = Out(np.zeros(batch), tol=np.ones(batch, bool), ref=p.sum(-1), bnd=bound(n, np.abs(p).sum(-1), p.sum(-1)))
    return Case("dot", dtype, [n, stride, batch], [x, y], [out], "dot n=%d b=%d stride=%d" % (n, batch, stride),
                lambda: [block_sum(x[:, :n] * y[:, :n])])


def dot_self(dtype, z):
    """dot_kernel(z, z, n = npad, stride = npad): what the fused z.z of trmv_t_part must equal to the bit."""
    batch, npad = z.shape
    return _dot_case(dtype, npad, batch, npad, z, z)


def _mtv(Mat, v, n):
    """out[b][p] = sum_i Mat[b][i][p] v[b][i] over i < n in longdouble, and the sum of the magnitudes."""
    p = Mat.astype(LD) * v[:, :n, None].astype(LD)
    return p.sum(1), np.abs(p).sum(1)


def mat_t_vec(dtype, n, P, batch, vstride=None, Mat=None, vec=None):
    vstride = n + 5 if vstride is None else vstride
    rng = _rng("mat_t_vec", n, P, batch, vstride)
    Mat = rnd(rng, batch, n, P) if Mat is None else Mat
    vec = _vec(rng, batch, n, vstride) if vec is None else vec
    ref, sabs = _mtv(Mat, vec, n)
    out = Out(np.zeros((batch, P)), tol=np.ones((batch, P), bool), ref=ref, bnd=bound(n, sabs, ref))
    return Case("mat_t_vec", dtype, [n, P, vstride, batch], [Mat, vec], [out],
                "mat_t_vec n=%d P=%d b=%d" % (n, P, batch),
                lambda: [block_sum(np.swapaxes(Mat * vec[:, :n, None], 1, 2))])


def grad_tail(dtype, ntiles, P, mean_N, noise_N, with_dm, n, batch):
    rng = _rng("grad_tail", ntiles, P, mean_N, noise_N, with_dm, n, batch)
    vstride = n + 3
    part = rnd(rng, batch, ntiles, P)
    dm = rnd(rng, batch, n, mean_N) if (mean_N and with_dm) else None
    alpha = _vec(rng, batch, n, vstride)  # (alpha and diagq are always passed, as the production call passes them)
    dsn2 = rnd(rng, batch, n, noise_N) if noise_N else None
    diagq = _vec(rng, batch, n, vstride)
    pl = part.astype(LD)
    outs = [Out(np.zeros((batch, P)), tol=np.ones((batch, P), bool), ref=pl.sum(1),
                bnd=bound(ntiles, np.abs(pl).sum(1), pl.sum(1)))]
    dm1 = None
    if mean_N:
        dm1 = dm if dm is not None else np.ones((batch, n, mean_N))  # (the derivative of a constant mean)
        ref, sabs = _mtv(dm1, alpha, n)
        outs.append(Out(np.zeros((batch, mean_N)), tol=np.ones((batch, mean_N), bool), ref=ref, bnd=bound(n, sabs, ref)))
    else:
        outs.append(Out(np.zeros(0)))
    if noise_N:
        ref, sabs = _mtv(dsn2, diagq, n)
        outs.append(Out(np.zeros((batch, noise_N)), tol=np.ones((batch, noise_N), bool), ref=ref, bnd=bound(n, sabs, ref)))
    else:
        outs.append(Out(np.zeros(0)))

    def emu():
        return [block_sum(np.swapaxes(part, 1, 2)),
                block_sum(np.swapaxes(dm1 * alpha[:, :n, None], 1, 2)) if mean_N else np.zeros(0),
                block_sum(np.swapaxes(dsn2 * diagq[:, :n, None], 1, 2)) if noise_N else np.zeros(0)]

    c = Case("grad_tail", dtype, [ntiles, P, n, mean_N, noise_N, vstride, batch], [part, dm, alpha, dsn2, diagq],
             [o for o in outs], "grad_tail ntiles=%d P=%d mean=%d noise=%d dm=%d n=%d b=%d"
             % (ntiles, P, mean_N, noise_N, with_dm, n, batch), emu)
    c.dm1, c.alpha, c.dsn2, c.diagq, c.vstride = dm1, alpha, dsn2, diagq, vstride
    return c


def _colsum_mats(rng, dtype, batch, nrows, mpad, ld, count):
    """Matrices of nrows + 3 rows, ld columns: rows >= nrows and columns >= M = mpad - 7 hold NaN."""
    mats = []
    for _ in range(count):
        A = np.full((batch, nrows + 3, ld), NAN)
        A[:, :nrows, :mpad - 7] = as_T(rnd(rng, batch, nrows, mpad - 7), dtype)
        mats.append(A)
    return mats


def colsum_prod(dtype, nrows, mpad, batch):
    ld, M = mpad + 64, mpad - 7
    rng = _rng("colsum_prod", dtype, nrows, mpad, batch)
    A, B = _colsum_mats(rng, dtype, batch, nrows, mpad, ld, 2)
    p = A[:, :nrows, :M].astype(LD) * B[:, :nrows, :M].astype(LD)
    ref, sabs = np.zeros((batch, mpad), LD), np.zeros((batch, mpad), LD)
    ref[:, :M], sabs[:, :M] = p.sum(1), np.abs(p).sum(1)
    real = (np.arange(mpad) < M)[None, :] & np.ones((batch, 1), bool)
    out = Out(np.zeros((batch, mpad)), tol=real, ref=ref, bnd=bound(nrows, sabs, ref), skip=~real)

    def emu():
        o = np.full((batch, mpad), NAN)
        o[:, :M] = four_waves(A[:, :nrows, :M] * B[:, :nrows, :M])
        return [o]

    return Case("colsum_prod", dtype, [ld, nrows, mpad, batch], [A, B], [out],
                "colsum_prod %s nrows=%d mpad=%d b=%d" % (DT_NAME[dtype], nrows, mpad, batch), emu)


def colsum_vec(dtype, nrows, mpad, batch):
    ld, M, vstride = mpad + 64, mpad - 7, nrows + 2
    rng = _rng("colsum_vec", dtype, nrows, mpad, batch)
    (A,) = _colsum_mats(rng, dtype, batch, nrows, mpad, ld, 1)
    v = _vec(rng, batch, nrows, vstride)
    p = A[:, :nrows, :M].astype(LD) * v[:, :nrows, None].astype(LD)
    ref, sabs = np.zeros((batch, mpad), LD), np.zeros((batch, mpad), LD)
    ref[:, :M], sabs[:, :M] = p.sum(1), np.abs(p).sum(1)
    real = (np.arange(mpad) < M)[None, :] & np.ones((batch, 1), bool)
    out = Out(np.zeros((batch, mpad)), tol=real, ref=ref, bnd=bound(nrows, sabs, ref), skip=~real)

    def emu():
        o = np.full((batch, mpad), NAN)
        o[:, :M] = four_waves(A[:, :nrows, :M] * v[:, :nrows, None])
        return [o]

    return Case("colsum_vec", dtype, [ld, nrows, mpad, vstride, batch], [A, v], [out],
                "colsum_vec %s nrows=%d mpad=%d b=%d" % (DT_NAME[dtype], nrows, mpad, batch), emu)


def diagq(dtype, n, ld, P, batch):
    """diagQ_i = Ainv_ii / sl - alpha_i^2: two products and a subtraction; out[P - 1] = their sum over i < n."""
    rng = _rng("diagq", dtype, n, ld, P, batch)
    Ainv = np.full((batch, ld, ld), NAN)
    Ainv[:, :n, :n] = as_T(rnd(rng, batch, n, n), dtype)
    alpha = _vec(rng, batch, n, ld)
    sp = np.abs(rnd(rng, batch, 4))
    d = np.arange(n)
    t1, t2 = Ainv[:, d, d].astype(LD) / sp[:, 3:4].astype(LD), alpha[:, :n].astype(LD) ** 2
    q, qabs = t1 - t2, np.abs(t1) + t2
    real = (np.arange(ld) < n)[None, :] & np.ones((batch, 1), bool)
    qref, qa = np.zeros((batch, ld), LD), np.zeros((batch, ld), LD)
    qref[:, :n], qa[:, :n] = q, qabs
    o0 = Out(np.where(real, 0.0, NAN), tol=real, ref=qref, bnd=bound(2, qa, qref, extra=1))
    last = (np.arange(P) == P - 1)[None, :] & np.ones((batch, 1), bool)
    tr, tra = q.sum(-1, keepdims=True), qabs.sum(-1, keepdims=True)
    o1 = Out(np.where(last, 0.0, NAN), tol=last, ref=tr * np.ones((1, P)), bnd=bound(2 * n, tra, tr, extra=1) * np.ones((1, P)))

    def emu():
        qq = Ainv[:, d, d] * (1.0 / sp[:, 3:4]) - alpha[:, :n] * alpha[:, :n]
        dq = np.full((batch, ld), NAN)
        dq[:, :n] = qq
        o = np.full((batch, P), NAN)
        o[:, P - 1] = block_sum(qq)
        return [dq, o]

    return Case("diagq", dtype, [n, ld, P, batch], [Ainv, alpha, sp], [o0, o1],
                "diagq %s n=%d ld=%d P=%d b=%d" % (DT_NAME[dtype], n, ld, P, batch), emu)


def trace_plane(dtype, n, ld, nblk):
    """part[block] = sum over the block's entries idx = i n + j (grid-stride) of (Ainv_ij / sl - alpha_i alpha_j) dK_ij,
    Ainv read from its lower triangle: two products per entry."""
    rng = _rng("trace_plane", dtype, n, ld, nblk)
    i, j = np.indices((n, n))
    Ainv = np.full((ld, ld), NAN)
    low = as_T(rnd(rng, n, n), dtype)
    Ainv[:n, :n] = np.where(j <= i, low, NAN)  # the upper triangle is not part of the operand
    alpha = _vec(rng, 1, n, ld)[0]
    sp = np.abs(rnd(rng, 4))
    dK = rnd(rng, n, n)
    sym = np.where(j <= i, low, low.T)
    t1 = sym.astype(LD) / LD(sp[3]) * dK.astype(LD)
    t2 = alpha[:n, None].astype(LD) * alpha[None, :n].astype(LD) * dK.astype(LD)
    term, tabs = (t1 - t2).ravel(), (np.abs(t1) + np.abs(t2)).ravel()
    own = (np.arange(n * n) // 256) % nblk  # idx = block 256 + thread, stride grid 256
    ref = np.array([term[own == b].sum() for b in range(nblk)], LD)
    sabs = np.array([tabs[own == b].sum() for b in range(nblk)], LD)
    cnt = np.array([(own == b).sum() for b in range(nblk)])
    out = Out(np.zeros(nblk), tol=np.ones(nblk, bool), ref=ref, bnd=bound(2 * cnt, sabs, ref, extra=1))

    def emu():
        t = ((sym * (1.0 / sp[3]) - alpha[:n, None] * alpha[None, :n]) * dK).ravel()
        flat = np.zeros(-(-n * n // (256 * nblk)) * 256 * nblk)
        flat[:n * n] = t
        flat = flat.reshape(-1, nblk, 256)  # [trip][block][thread]
        return [np.array([block_sum(flat[:, b, :].ravel()) for b in range(nblk)])]

    return Case("trace_plane", dtype, [n, ld, nblk], [Ainv, alpha, sp, dK], [out],
                "trace_plane %s n=%d ld=%d blocks=%d" % (DT_NAME[dtype], n, ld, nblk), emu)


# ---- layout and copies ---------------------------------------------------------------------------------------------------
def _pad128(n):
    return -(-n // TILE) * TILE


def extract(dtype, n, mode):
    ld = _pad128(n)
    rng = _rng("extract", dtype, n, mode)
    src = np.full((ld, ld), NAN)
    full = as_T(rnd(rng, n, n), dtype)
    i, j = np.indices((n, n))
    src[:n, :n] = full if mode == 2 else np.where(j <= i, full, NAN)
    exp = {0: np.where(j <= i, full, 0.0), 1: -np.where(j <= i, full, full.T), 2: full}[mode]
    return Case("extract", dtype, [n, ld, mode], [src], [Out(exp)], "extract %s n=%d mode=%d" % (DT_NAME[dtype], n, mode))


def neg_sym(dtype, npad, batch):
    ld = npad + 64
    rng = _rng("neg_sym", dtype, npad, batch)
    buf = as_T(rnd(rng, batch, npad, ld), dtype)
    i, j = np.indices((npad, npad))
    sq = buf[:, :, :npad].copy()
    low = np.where(j <= i, sq, 0.0)
    exp = buf.copy()
    exp[:, :, :npad] = -np.where(j <= i, low, np.swapaxes(low, 1, 2))
    buf[:, :, :npad] = np.where(j <= i, sq, NAN)  # the upper triangle is overwritten, never read
    return Case("neg_sym", dtype, [npad, ld, batch], [buf], [Out(exp)], "neg_sym %s npad=%d b=%d" % (DT_NAME[dtype], npad, batch))


def pad_load(dtype, n, npad):
    src = rnd(_rng("pad_load", n, npad), n, n)
    exp = np.eye(npad)
    exp[:n, :n] = store(src, dtype)
    return Case("pad_load", dtype, [n, npad], [src], [Out(exp)], "pad_load %s %d -> %d" % (DT_NAME[dtype], n, npad))


def pad_rect(dtype, r, c, rpad, cpad):
    src = rnd(_rng("pad_rect", r, c), r, c)
    exp = np.zeros((rpad, cpad))
    exp[:r, :c] = store(src, dtype)
    return Case("pad_rect", dtype, [r, c, rpad, cpad], [src], [Out(exp)],
                "pad_rect %s %dx%d -> %dx%d" % (DT_NAME[dtype], r, c, rpad, cpad))


def load_K(dtype, n, npad, kscale):
    """A = K / sp[2] + diag(dvec), identity padding.  sp[2] = 1: the entries off the diagonal are the cast of K."""
    rng = _rng("load_K", n, npad, kscale)
    K, dvec = rnd(rng, n, n), np.abs(rnd(rng, n))
    sp = np.array([NAN, NAN, kscale, NAN])
    eye = np.eye(n, dtype=bool)
    q = K.astype(LD) / LD(kscale)
    ref = q + np.where(eye, dvec[:, None].astype(LD), 0)
    sabs = np.abs(q) + np.where(eye, dvec[:, None], 0.0)
    bnd = np.where(eye, bound(2, sabs, ref, extra=1, stored=dtype), bound(0, sabs, ref, extra=1, stored=dtype))
    exp, tol = np.eye(npad), np.zeros((npad, npad), bool)
    refp, bndp = np.zeros((npad, npad), LD), np.zeros((npad, npad), LD)
    refp[:n, :n], bndp[:n, :n] = ref, bnd
    if kscale == 1.0:
        exp[:n, :n] = store(K, dtype)
        tol[:n, :n] = eye
    else:
        tol[:n, :n] = True
    return Case("load_K", dtype, [n, npad], [K, sp, dvec], [Out(exp, tol=tol, ref=refp, bnd=bndp)],
                "load_K %s %d -> %d kscale=%g" % (DT_NAME[dtype], n, npad, kscale))


def rect_copy(dtype, rows, cols, batch):
    lds, ldd = cols + 64, cols + 128
    rng = _rng("rect_copy", dtype, rows, cols, batch)
    src = as_T(rnd(rng, batch, rows + 4, lds), dtype)
    dst = as_T(rnd(rng, batch, rows + 8, ldd), dtype)
    exp = dst.copy()
    exp[:, :rows, :cols] = src[:, :rows, :cols]
    return Case("rect_copy", dtype, [rows, cols, lds, ldd, batch], [src, dst], [Out(exp)],
                "rect_copy %s %dx%d b=%d" % (DT_NAME[dtype], rows, cols, batch))


def grow_copy(dtype, np_, npn, batch):
    src = as_T(rnd(_rng("grow_copy", dtype, np_, npn, batch), batch, np_, np_), dtype)
    exp = np.eye(npn)[None].repeat(batch, 0)
    exp[:, :np_, :np_] = src
    return Case("grow_copy", dtype, [np_, npn, batch], [src], [Out(exp)],
                "grow_copy %s %d -> %d b=%d" % (DT_NAME[dtype], np_, npn, batch))


# ---- rank-one append -------------------------------------------------------------------------------------------------------
def append_row(dtype, npad, n, batch):
    rng = _rng("append_row", dtype, npad, n, batch)
    A, W = as_T(rnd(rng, batch, npad, npad), dtype), as_T(rnd(rng, batch, npad, npad), dtype)
    l, au = _vec(rng, batch, n, npad), _vec(rng, batch, n, npad)
    coef, alpha = rnd(rng, batch, 5), rnd(rng, batch, npad)
    cl, dl, cw, ca, cau = (coef[:, q:q + 1].astype(LD) for q in range(5))
    row = np.zeros((batch, npad, npad), bool)
    row[:, n, :n + 1] = True
    k = np.arange(npad)
    refA, refW = A.astype(LD), W.astype(LD)
    refA[:, n, :n], refW[:, n, :n] = l[:, :n].astype(LD) * cl, au[:, :n].astype(LD) * cw
    refA[:, n, n], refW[:, n, n] = dl[:, 0], 1 / dl[:, 0]
    expA, expW = A.copy(), W.copy()
    expA[:, n, n] = store(coef[:, 1], dtype)  # a cast
    tolA = row & (k < n)[None, None, :]
    oA = Out(expA, tol=tolA, ref=refA, bnd=bound(1, np.abs(refA), refA, stored=dtype))
    oW = Out(expW, tol=row, ref=refW, bnd=bound(1, np.abs(refW), refW, stored=dtype))
    upd = ca * au[:, :n].astype(LD) * cau
    refal, sab = alpha.astype(LD), np.zeros((batch, npad), LD)
    sab[:, :n] = np.abs(refal[:, :n]) + np.abs(upd)
    refal[:, :n] = refal[:, :n] + upd
    expal = alpha.copy()
    expal[:, n] = -coef[:, 3]
    oal = Out(expal, tol=(k < n)[None, :] & np.ones((batch, 1), bool), ref=refal, bnd=bound(2, sab, refal, extra=1))
    return Case("append_row", dtype, [npad, n, batch], [A, W, l, au, coef, alpha], [oA, oW, oal],
                "append_row %s npad=%d n=%d b=%d" % (DT_NAME[dtype], npad, n, batch))


def append_low(dtype, n, ld):
    rng = _rng("append_low", dtype, n, ld)
    A = as_T(rnd(rng, ld, ld), dtype)
    au = _vec(rng, 1, n, ld)[0]
    coef, alpha = rnd(rng, 5), rnd(rng, ld)
    cv, ca = LD(coef[0]), LD(coef[3])
    aul = au[:n].astype(LD)
    ref, sab = A.astype(LD), np.zeros((ld, ld), LD)
    outer = aul[:, None] * cv * aul[None, :]
    sab[:n, :n] = np.abs(ref[:n, :n]) + np.abs(outer)
    ref[:n, :n] = ref[:n, :n] - outer
    ref[:n, n] = ref[n, :n] = aul * cv
    sab[:n, n] = sab[n, :n] = np.abs(aul * cv)
    exp = A.copy()
    exp[n, n] = store(-coef[0], dtype)
    tol = np.zeros((ld, ld), bool)
    tol[:n + 1, :n + 1] = True
    tol[n, n] = False
    oA = Out(exp, tol=tol, ref=ref, bnd=bound(2, sab, ref, extra=1, stored=dtype))
    refal, sal = alpha.astype(LD), np.zeros(ld, LD)
    sal[:n] = np.abs(refal[:n]) + np.abs(ca * aul)
    refal[:n] = refal[:n] + ca * aul
    expal = alpha.copy()
    expal[n] = -coef[3]
    oal = Out(expal, tol=np.arange(ld) < n, ref=refal, bnd=bound(2, sal, refal))
    return Case("append_low", dtype, [ld, n], [A, au, coef, alpha], [oA, oal], "append_low %s n=%d ld=%d" % (DT_NAME[dtype], n, ld))


# ---- the shapes: the smallest at which each piece of index arithmetic changes behaviour --------------------------------------
NPADS = (128, 256, 384, 640)  # 128, 384: the fp32 trmv_t_part block hangs over the edge by a tile; 384, 640: odd tile
#                               counts, a third chunk; 640 > 512: two trips of trmv's 64 VEC stride loop in fp32
TRMV_BLOCKS = ((0, 640), (128, 128), (128, 256), (256, 384))  # (row0, rows) in npad = 640
GEMV_BLOCKS = ((128, 128, 0, 128), (256, 384, 0, 256), (384, 256, 256, 128))  # (row0, nrows, col0, ncols) in npad = 640
BATCHES = (1, 3)
GRAD_TAIL_SLOTS = ((0, 0), (1, 0), (3, 2), (0, 1))  # (mean_N, noise_N)


def reduction_cases(dtype):
    """Every case whose result is arithmetic with a summation order (the CPU emulation covers exactly these)."""
    for b in BATCHES:
        for npad in NPADS:
            yield trmv(dtype, npad, b)
            yield trmv(dtype, npad, b, low=True)
            for quad in (True, False):
                yield trmv_t_part(dtype, npad, b, quad)
                yield trmv_t_part(dtype, npad, b, quad, low=True)
            for scale in (True, False):
                yield trmv_t_sum(dtype, npad, b, scale)
        for row0, rows in TRMV_BLOCKS[1:]:
            yield trmv(dtype, 640, b, row0, rows)
        for blk in GEMV_BLOCKS:
            yield gemv_sub(dtype, 640, b, *blk)
        for n in (1, 255, 256, 257, 640):
            yield dot(dtype, n, b)
        for n in (5, 256, 300):
            for P in (1, 4):
                yield mat_t_vec(dtype, n, P, b)
        for nrows in (1, 3, 4, 130):
            for mpad in (64, 192):
                yield colsum_prod(dtype, nrows, mpad, b)
                yield colsum_vec(dtype, nrows, mpad, b)
        yield diagq(dtype, 130, 256, 3, b)
    for cs in grad_tail_cases(dtype):
        yield cs
    for nblk in (1, 7):
        yield trace_plane(dtype, 130, 256, nblk)


def grad_tail_cases(dtype):
    for b in BATCHES:
        for ntiles in (1, 3, 300):  # 300: more than one pass of the 256 threads
            for P in (1, 4):
                for mN, nN in GRAD_TAIL_SLOTS:
                    for with_dm in ((True, False) if mN else (True,)):
                        for n in (5, 300):
                            yield grad_tail(dtype, ntiles, P, mN, nN, with_dm, n, b)


def copy_cases(dtype):
    for n in (1, 63, 65, 130):
        for mode in (0, 1, 2):
            yield extract(dtype, n, mode)
    for npad in (128, 256):
        yield neg_sym(dtype, npad, 2)
    yield pad_load(dtype, 130, 256)
    yield pad_rect(dtype, 130, 70, 256, 128)
    for kscale in (1.0, 0.37):
        yield load_K(dtype, 130, 256, kscale)
    for rows in (32, 96):
        for cols in (128, 384):
            yield rect_copy(dtype, rows, cols, 2)
    yield grow_copy(dtype, 128, 256, 2)


def append_cases(dtype):
    for n in (0, 5, 255, 256, 257):
        yield append_row(dtype, 384, n, 2)
    for n in (3, 63, 64, 130):
        yield append_low(dtype, n, 256)
