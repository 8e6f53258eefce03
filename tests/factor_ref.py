"""What tests/test_factor_plan_cpu.py and tests/test_gpu_factor_plan.py share: the matrix families, the NaN poison, the
NumPy model of every plan (tests/blocked_model.py, driven as gpc_debug_factor_plan drives plan.h) and the expectations
(a) - (f) with their bars.  Test helper, CPU only; nothing here touches a device.

Symbols: u = 2^-53 (fp64) or 2^-24 (fp32), n = the order of the matrix (nvalid), npad = n rounded up to 128.

  rho_F = max over the lower triangle of |A - L L^T| / (n u |L||L^T|)           Higham's componentwise Cholesky bound
  rho_I = max over the 128-tiles of an owning block of ||(L W - I)_tile||_F / (n u ||(|L||W|)_tile||_F)

Bars (none is tuned against a device): stable mode rho_F <= 1; fast mode rho_F <= max(1, 4 rho_model) on the families
whose fast-mode error the explicit-inverse panel solves leave bounded (gp, lownoise, extreme), rho_model being the
model's own rho_F on the same matrix, plan and precision, and 4 a margin for two summation orders of one algorithm;
rho_I <= 1 everywhere; logdet, forward solve and Ainv as written at their checks below.  The residuals are formed in
np.longdouble for fp64 (x86: 64-bit mantissa, so the reference's own error is 2^-11 of the bar) and in float64 for fp32
(2^-29 of it); the |.||.| products of the denominators are taken in float64, whose error of n 2^-53 relative is far
below anything a bar could notice."""

import functools

import numpy as np

import blocked_model as bm

TILE = 128
F64, F32 = 0, 1  # gpyreg_amd._lib.F64 / F32
NP_DT = {F64: np.float64, F32: np.float32}
U = {F64: 2.0 ** -53, F32: 2.0 ** -24}
DT_NAME = {F64: "f64", F32: "f32"}
LD = np.longdouble

FAMILIES = ("gp", "scaled", "lownoise", "neardup", "extreme")
SIZES = (100, 128, 129, 144, 145, 300, 384, 640)
NLL_SIZES = (129, 300, 384, 640)  # potrf_nll: two, three, three and five tiles
FAST_ASSERTED = ("gp", "lownoise", "extreme")  # fast mode: rho_F asserted here, printed on scaled and neardup
FAST_MARGIN = 4.0


def npad_of(n):
    return -(-n // TILE) * TILE


# ---- inputs ----------------------------------------------------------------------------------------------------------
def _sqdist(X):
    return ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)


@functools.lru_cache(maxsize=64)
def matrix(family, n, dtype):
    """The n x n SPD matrix of a family (fixed seed per family and size); fp32: rounded to float32, returned as float64."""
    rng = np.random.default_rng(1000 * FAMILIES.index(family) + n)
    X = rng.uniform(-3, 3, (n, 2))
    gp = np.exp(-0.5 * _sqdist(X) / 2) / 0.01 + np.eye(n)  # _spd of tests/test_gpu_kernels.py
    if family == "gp":
        A = gp
    elif family == "scaled":
        d = 10.0 ** rng.uniform(-3, 3, n)
        A = d[:, None] * gp * d[None, :]
    elif family == "lownoise":
        A = np.exp(-0.5 * _sqdist(X)) + (1e-6 if dtype == F64 else 1e-2) * np.eye(n)
    elif family == "neardup":
        h = n // 2
        X[h:] = X[:n - h] + 1e-7 * rng.standard_normal((n - h, 2))
        A = np.exp(-0.5 * _sqdist(X)) + (1e-9 if dtype == F64 else 1e-3) * np.eye(n)
    elif family == "extreme":
        e = 200 if dtype == F64 else 40
        A = gp * 2.0 ** (e if n % 2 == 0 else -e)
    else:
        raise KeyError(family)
    A = 0.5 * (A + A.T)
    if dtype == F32:
        A = A.astype(np.float32).astype(np.float64)
    A.setflags(write=False)
    return A


def rhs(n, seed=0):
    """The right-hand side of the forward solve: finite everywhere, the padding included (blas1.h: trmv_kernel)."""
    return np.random.default_rng(77 + n + seed).standard_normal(npad_of(n))


def poisoned(A0):
    """(A, W, T) as the hook gets them: A identity-padded with its whole strict upper triangle NaN, W and T all NaN."""
    A = bm.pad_identity(np.asarray(A0), TILE)
    npad = A.shape[0]
    A[np.triu_indices(npad, 1)] = np.nan
    return A, np.full((npad, npad), np.nan), np.full((npad, npad), np.nan)


# ---- the cases -------------------------------------------------------------------------------------------------------
# (plan, nll_block, keep_L); stable mode keeps L anyway, so keep_L is swept in fast mode only
PLANS = ((0, 0, 0), (0, 0, 1), (1, 0, 0), (1, 0, 1), (2, 128, 0), (2, 256, 0))


def cases():
    """(family, n, plan, nll_block, stable, keep_L, dtype): every plan x mode x precision, every size, the families
    rotating over the sizes so that each (plan, mode, precision) meets all five; n = 640 in one family per mode."""
    out = []
    for stable in (0, 1):
        for dtype in (F64, F32):
            for ci, (plan, blk, keep_L) in enumerate(PLANS):
                if stable and keep_L:
                    continue
                for si, n in enumerate(NLL_SIZES if plan == 2 else SIZES):
                    fam = FAMILIES[(si + ci + dtype) % 5]
                    if n == 640:
                        fam = "neardup" if stable else "gp"
                    out.append((fam, n, plan, blk, stable, keep_L, dtype))
    return out


def case_id(c):
    fam, n, plan, blk, stable, keep_L, dtype = c
    return "%s-%d-p%d%s%s-%s-%s" % (fam, n, plan, "b%d" % blk if plan == 2 else "", "k" if keep_L else "",
                                   "stable" if stable else "fast", DT_NAME[dtype])


def owning_blocks(plan, npad, blk):
    """The diagonal blocks (off, n) that own their whole inverse -- a recursion that mirrors plan.h: plan 0 the matrix,
    plan 1 the left child of every node on the right spine (and the last leaf), plan 2 the blocks of at most blk rows."""
    if plan == 0:
        return [(0, npad)]
    out = []
    if plan == 1:
        off, n = 0, npad
        while n > TILE:
            n1 = (n // TILE // 2) * TILE
            out.append((off, n1))
            off, n = off + n1, n - n1
        out.append((off, n))
        return out

    def rec(off, n):
        if n <= blk or n == TILE:
            out.append((off, n))
            return
        n1 = (n // TILE // 2) * TILE
        rec(off, n1)
        rec(off + n1, n - n1)

    rec(0, npad)
    return out


# ---- the model, driven as the hook drives the device -------------------------------------------------------------------
def run_model(A, W, T, nvalid, plan=0, nll_block=0, stable=False, keep_L=False, want_inv=False, r=None, dtype=F64,
              gemm_hook=None, leaf_nvalid=True, solve_from_A=False):
    """One sample through tests/blocked_model.py; same arguments and the same dict as Context.debug_factor_plan gives per
    sample.  The last three arguments seed defects (test_factor_plan_cpu.py): gemm_hook(kwargs) may alter the
    arguments of every product, leaf_nvalid = False factors the padded panels too, solve_from_A reads L21 out of A."""
    dt = NP_DT[dtype]
    A, W, T = (np.array(x, dtype=dt) for x in (A, W, T))
    npad = A.shape[0]
    ld = [0.0]
    leaves = [0]

    def leaf_fn(a, w):  # the plan visits the leaves once each, left to right
        off = leaves[0] * TILE
        leaves[0] += 1
        nv = max(0, min(TILE, nvalid - off)) if leaf_nvalid else None
        return bm.leaf_panels(a, w, 16, refine=bool(stable), nvalid=nv, logdet=ld)

    real = bm.tiled_gemm

    def hooked(C, A_, B_, M, N, K, tile, **kw):
        return real(C, A_, B_, M, N, K, tile, **gemm_hook(dict(kw)))

    if gemm_hook is not None:
        bm.tiled_gemm = hooked
    try:
        with np.errstate(all="ignore"):
            if plan == 2:
                info = bm.potrf_nll(A, W, T, 0, npad, TILE, nll_block, None, bool(stable), leaf_fn)
            else:
                info = bm.potrf_inv(A, W, T, 0, npad, TILE, plan == 0, bool(keep_L), None, bool(stable), leaf_fn)
            z = None
            if r is not None:
                z = np.array(r, dtype=np.float64)
                src = A if solve_from_A else T
                if plan == 2:
                    bm.forward_solve_nll(src, W, z, 0, npad, TILE, nll_block)
                else:
                    bm.forward_solve(src, W, z, 0, npad, TILE, plan == 0)
            out = dict(A=A.astype(np.float64), W=W.astype(np.float64), T=T.astype(np.float64), z=z, Ainv=None,
                       logdet=ld[0], info=int(info))
            if want_inv:
                bm.lauum(T, W, npad, TILE)
                out["Ainv"] = T.astype(np.float64)
    finally:
        bm.tiled_gemm = real
    return out


# ---- the expectations ------------------------------------------------------------------------------------------------
def _tiles(npad):
    q = npad // TILE
    return [(i, j) for i in range(q) for j in range(q)]


def _t(M, i, j):
    return M[i * TILE:(i + 1) * TILE, j * TILE:(j + 1) * TILE]


def assemble_L(out):
    """The factor, valid for every plan: the lower triangles of A's diagonal tiles and the strictly-lower tiles of T."""
    A, T = out["A"], out["T"]
    npad = A.shape[0]
    L = np.zeros((npad, npad))
    for i, j in _tiles(npad):
        if i == j:
            _t(L, i, j)[:] = np.tril(_t(A, i, j))
        elif j < i:
            _t(L, i, j)[:] = _t(T, i, j)
    return L


def lower_tiles(M, blocks=None):
    """M with every tile strictly above the diagonal -- or outside `blocks` -- replaced by zeros (they hold poison)."""
    npad = M.shape[0]
    out = np.zeros_like(M)
    for off, n in (blocks or [(0, npad)]):
        for i in range(off // TILE, (off + n) // TILE):
            for j in range(off // TILE, i + 1):
                _t(out, i, j)[:] = _t(M, i, j)
    return out


def check_layout(out, nvalid, plan, blk, stable, keep_L):
    """(a): the list of what is wrong with where the plan wrote and what it left alone."""
    A, W, T = out["A"], out["W"], out["T"]
    npad = A.shape[0]
    bad = []
    own = np.zeros((npad // TILE, npad // TILE), dtype=bool)
    for off, n in owning_blocks(plan, npad, blk):
        own[off // TILE:(off + n) // TILE, off // TILE:(off + n) // TILE] = True
    iu = np.triu_indices(TILE, 1)
    keep = stable or (keep_L and plan != 2)  # (potrf_nll takes no keep_L)
    for i, j in _tiles(npad):
        a, w, t = _t(A, i, j), _t(W, i, j), _t(T, i, j)
        if j > i:
            for name, x in (("A", a), ("W", w), ("T", t)):
                if not np.isnan(x).all():
                    bad.append("%s tile (%d, %d) above the diagonal was written" % (name, i, j))
        elif i == j:
            if not np.isnan(t).all():
                bad.append("T diagonal tile %d was written" % i)
            if not np.isfinite(np.tril(a)).all():
                bad.append("A diagonal tile %d: L is not finite" % i)
            if stable and not (a[iu] == 0).all():
                bad.append("A diagonal tile %d: stable mode left no exact zeros above the diagonal" % i)
            if not stable and not np.isnan(a[iu]).all():
                bad.append("A diagonal tile %d was written above the diagonal in fast mode" % i)
            if not np.isfinite(w).all() or not (w[iu] == 0).all():
                bad.append("W diagonal tile %d is not finite with exact zeros above the diagonal" % i)
        else:
            if not np.isfinite(t).all():
                bad.append("T tile (%d, %d) is not finite" % (i, j))
            if not np.isfinite(a).all():
                bad.append("A tile (%d, %d) is not finite" % (i, j))
            if own[i, j] and not np.isfinite(w).all():
                bad.append("W tile (%d, %d) of an owning block is not finite" % (i, j))
            if not own[i, j] and not np.isnan(w).all():
                bad.append("W tile (%d, %d) outside the owning blocks was written" % (i, j))
            # (potrf_nll keeps L inside the blocks it hands to potrf_inv -- in stable mode -- and nowhere above them:
            # there A21 holds what the blocked solve left, in stable mode the refinement's residual)
            if keep and (plan != 2 or own[i, j]) and not np.array_equal(a, t):
                bad.append("A tile (%d, %d) is not T's to the bit although L is kept" % (i, j))
    # identity padding: exact
    if nvalid < npad and not bad:
        L = assemble_L(out)
        Wl = lower_tiles(W, owning_blocks(plan, npad, blk))
        eye = np.eye(npad)
        for name, M in (("L", L), ("W", Wl)):
            if not (np.array_equal(M[nvalid:, :], eye[nvalid:, :]) and np.array_equal(M[:, nvalid:], eye[:, nvalid:])):
                bad.append("%s is not exactly the identity in the rows and columns >= nvalid" % name)
    return bad


def _ratio(num, den):
    """max num / den with 0 / 0 = 0 and x / 0 = inf; NaN anywhere gives inf."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    with np.errstate(all="ignore"):
        q = np.where(num == 0, 0.0, num / den)
    if q.size == 0:
        return 0.0
    m = q.max()
    return float("inf") if np.isnan(m) else float(m)


def _wide(dtype):
    return LD if dtype == F64 else np.float64


def rho_F(A0, L, dtype):
    """(b) on the n valid rows (the padding is checked exactly by the layout)."""
    n = A0.shape[0]
    wt = _wide(dtype)
    Lw = L[:n, :n].astype(wt)
    res = np.abs(np.asarray(A0, dtype=wt) - Lw @ Lw.T)
    aL = np.abs(L[:n, :n])
    il = np.tril_indices(n)
    return _ratio(res[il], (n * U[dtype]) * (aL @ aL.T)[il])


def rho_I(L, W, blocks, n, dtype):
    """(c): the right residual L W - I per 128-tile of every owning block."""
    wt = _wide(dtype)
    worst = 0.0
    Wl = lower_tiles(W, blocks)
    for off, nb in blocks:
        s = slice(off, off + nb)
        Lb, Wb = L[s, s], Wl[s, s]
        res = np.abs(Lb.astype(wt) @ Wb.astype(wt) - np.eye(nb, dtype=wt)).astype(np.float64)
        den = np.abs(Lb) @ np.abs(Wb)
        for i in range(nb // TILE):
            for j in range(i + 1):
                worst = max(worst, _ratio(np.linalg.norm(_t(res, i, j)), n * U[dtype] * np.linalg.norm(_t(den, i, j))))
    return worst


def logdet_ratio(L, nvalid, logdet):
    """(d): |logdet - sum_{i < nvalid} log L_ii| / ((nvalid + 4) 2^-53 sum |log L_ii|); the accumulation is in double in
    both precisions (one rounding per log, nvalid additions in some order, the wave reduction)."""
    lg = np.log(np.diag(L)[:nvalid].astype(LD))
    return _ratio(abs(LD(logdet) - lg.sum()), (nvalid + 4) * 2.0 ** -53 * np.abs(lg).sum())


def solve_ratio(L, W, blocks, r, z, n):
    """(e): z = W_bd (r - L_off z) as the device evaluates it, in double for both precisions."""
    Wbd = lower_tiles(W, blocks)
    Loff = L - lower_tiles(L, blocks)
    zw, rw = z.astype(LD), r.astype(LD)
    res = np.abs(zw - Wbd.astype(LD) @ (rw - Loff.astype(LD) @ zw))
    den = 2 * n * 2.0 ** -53 * (np.abs(Wbd) @ (np.abs(r) + np.abs(Loff) @ np.abs(z)))
    return _ratio(res, den)


def ainv_check(W, Ainv, n, dtype):
    """(f): (ratio on the lower tiles, strictly-upper tiles untouched).  The result is the lower TRIANGLE.  Above the
    diagonal inside a diagonal 128-tile an entry is either the mirrored value, held to the same bound (a launch of
    128-tiles, and the model, write the whole tile), or untouched (a launch of 64-tiles, which every launch below
    gemm.h's small-launch threshold is, leaves the upper 64 x 64 quarter alone): never anything else."""
    npad = W.shape[0]
    wt = _wide(dtype)
    Wl = lower_tiles(W)
    ref = Wl.T.astype(wt) @ Wl.astype(wt)
    den = n * U[dtype] * (np.abs(Wl).T @ np.abs(Wl))
    iu = np.triu_indices(TILE, 1)
    worst, untouched = 0.0, True
    for i, j in _tiles(npad):
        if j > i:
            untouched = untouched and bool(np.isnan(_t(Ainv, i, j)).all())
            continue
        got = _t(Ainv, i, j)
        err = np.abs(got.astype(wt) - _t(ref, i, j))
        if i == j:
            err[iu] = np.where(np.isnan(got[iu]), 0, err[iu])
        worst = max(worst, _ratio(err, _t(den, i, j)))
    return worst, untouched


def verify(out, A0, plan, blk, stable, keep_L, dtype, r=None, rho_model=None, assert_fast=True):
    """All of (a) - (f) on one sample with info == 0.  Returns (ratios, failures): every ratio is measured / bar except
    rho_F, which is reported as defined; `failures` lists what misses its bar, keyed "layout", "factor", "inverse",
    "logdet", "solve", "ainv".  rho_model: the model's rho_F of the same case (fast mode's bar); None in the model's own
    run, where it stands in for itself."""
    n = A0.shape[0]
    npad = out["A"].shape[0]
    fails = {}
    ratios = {}
    if out["info"] != 0:
        return ratios, {"info": "info = %d on a positive definite matrix" % out["info"]}
    lay = check_layout(out, n, plan, blk, stable, keep_L)
    if lay:
        fails["layout"] = "; ".join(lay[:4])
        return ratios, fails  # the assembled factor would be poison
    blocks = owning_blocks(plan, npad, blk)
    L = assemble_L(out)
    ratios["rho_F"] = rf = rho_F(A0, L, dtype)
    if stable:
        bar = 1.0
    else:
        bar = max(1.0, FAST_MARGIN * (rf if rho_model is None else rho_model))
        ratios["rho_F/model"] = rf / rho_model if rho_model else float("nan")
    if (stable or assert_fast) and not rf <= bar:
        fails["factor"] = "rho_F = %.3g > %.3g" % (rf, bar)
    ratios["rho_I"] = ri = rho_I(L, out["W"], blocks, n, dtype)
    if not ri <= 1.0:
        fails["inverse"] = "rho_I = %.3g > 1" % ri
    ratios["logdet"] = rl = logdet_ratio(L, n, out["logdet"])
    if not rl <= 1.0:
        fails["logdet"] = "logdet misses its bound by %.3g" % rl
    if r is not None:
        ratios["solve"] = rs = solve_ratio(L, out["W"], blocks, r, out["z"], n)
        if not rs <= 1.0:
            fails["solve"] = "the forward solve misses its bound by %.3g" % rs
    if out.get("Ainv") is not None:
        ra, untouched = ainv_check(out["W"], out["Ainv"], n, dtype)
        ratios["ainv"] = ra
        if not ra <= 1.0 or not untouched:
            fails["ainv"] = "Ainv misses its bound by %.3g%s" % (ra, "" if untouched else "; upper tiles written")
    return ratios, fails


@functools.lru_cache(maxsize=None)
def model_rho_F(family, n, plan, blk, stable, keep_L, dtype):
    """rho_model: the model's rho_F on the matrix of a case (the bar of fast mode on the device)."""
    A0 = matrix(family, n, dtype)
    out = run_model(*poisoned(A0), n, plan, blk, stable, keep_L, dtype=dtype)
    assert out["info"] == 0, "the model fails on %s n = %d" % (family, n)
    return rho_F(A0, assemble_L(out), dtype)
