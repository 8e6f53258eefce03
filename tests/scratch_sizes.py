"""The scratch of one sample of the chunked posterior consumers, in bytes, as closed forms, and the chunk that the
library's planner derives from them under GPC_MEM_BUDGET_MB.

These are the formulas that gpcore.hip carried by hand (`per_sample(...)`, then one `per` expression per call) before
its scratch blocks were declared once through ScratchCarver, restated here so that the chunking tests can say which chunk
a budget must give: the library reports the chunk it planned as the option "last_chunk", and a layout that lost or gained
an array shows up as a different chunk (or as the same chunk at a budget chosen near a border).  Where a call's hand-written
formula left out arrays it allocated, or counted bytes that live elsewhere, the form here is that formula plus or minus
the terms DESIGN.md lists ("Posterior consumers share their host scaffolding"), each named where it is added.  Nothing
here is read from the library; test_scratch_layout_cpu.py compares the library's own count (gpc_debug_scratch_bytes)
against these forms."""


def pad(n, t=128):
    return -(-n // t) * t


def planned_chunk(S, mb, per, shared=0):
    """plan_chunk under a forced budget of `mb` megabytes: 80 % of it, less `shared`, divided by `per`; 0 = refused."""
    budget = int((mb << 20) * 0.8)
    return 0 if budget < shared + per else min(S, (budget - shared) // per)


def rhs_per(npad, mpad, full, w, D, kind="cross", want_quad=True, grad=False, qg=False, M=0, R=0, gobs_pts=0):
    """rhs_products: gpc_predict (kind "cross"), gpc_predict_full (full, no want_quad), gpc_quad ("quad"), gpc_predict_K
    ("given"), gpc_predict_gobs ("gobs"), gpc_predict_grad (grad), gpc_quad_grad (grad and qg), gpc_draw (full, R draws
    of M points).  The hand-written formula -- the right-hand side and the product, npad x mpad each, with `full` the
    mpad x mpad covariance, with a gradient pass that reads it Q, in the storage type (w bytes); the gradient pass's
    partials and planes and quad_grad's constants; a draw's three slabs, Z, F and the draws -- plus what that formula
    left out."""
    gq = grad and (not qg or want_quad)
    gpl = (4 if qg and want_quad else 2) if grad else 0
    per = (2 * npad * mpad + (mpad * mpad if full else 0) + (npad * mpad if gq else 0)) * w
    per += (npad // 64) * gpl * D * mpad * 8 + gpl * mpad * D * 8 + ((D + 1) * mpad * 8 if qg else 0)
    if R:
        per += (3 * mpad * mpad + 2 * mpad * pad(R)) * w + M * R * 8
    per += 2 * mpad * 8                                   # + [mu | v]
    if kind != "given":
        per += mpad * D * 8                               # + the scaled queries
    if kind in ("cross", "gobs"):
        per += ((npad if kind == "cross" else gobs_pts) // 64) * mpad * 8  # + the builder's cross-tile partials
    if want_quad and not full and not grad and (npad // 128) * (mpad // 128) >= 64:
        per += (npad // 128) * mpad * 8                   # + the tile rows' column sums of squares (large products)
    if R:
        per += 16                                         # + a draw's logdet and info
    return per


def rhs_shared(N, M, D, S, kind="cross", full=False, qg=False, R=0):
    """rhs_products, once per call (the hand-written plan had no shared part): quad_grad's transposed means, the staging
    of gpc_predict_K's uploads and of the full covariance's download, the raw queries, a draw's noise deviations."""
    d = D * pad(M) if qg else 0
    if kind == "given":
        d += max(N, M) * M
    else:
        d += 2 * M * D
    if full and not R:
        d += M * M
    if R:
        d += M * S
    return d * 8


def cov_per(npad, mapad, mbpad, D, w, fused=False):
    """gpc_predict_cov / the look-ahead's C^0: both right-hand sides and products, K_ab, the partials, the scaled queries,
    the weights and factors, [v | q] -- the hand-written formula, which was complete."""
    part = (npad // 64) * max(mapad, mbpad) * 8 + ((mapad // 128) * mbpad * 8 if fused else 0)
    return (2 * npad * (mapad + mbpad) + mapad * mbpad) * w + part + ((mapad + mbpad) * D + mapad + 1 + 2 * mbpad) * 8


def cov_shared(Ma, Mb, D, want_cov):
    """... once per call (not planned for by hand): the raw queries and one sample's covariance on its way out."""
    return ((Ma + Mb) * D + (Ma * Mb if want_cov else 0)) * 8


def _chunk_consts(npad, D):
    """What grad_post and predict_hess counted although it lives in the buffers of ChunkConsts: the scaled training
    inputs, SP_STRIDE = 4 scalars and the two scale vectors."""
    return (npad * D + 4 + 2 * D) * 8


def grad_post_per(npad, D, diag, w, qb=128):
    """gpc_grad_post with one block of 128 queries (shared: the raw queries, M D 8)."""
    dp, nt64, nseg = D + 1, npad // 64, max(1, min(16, npad // 512))
    ld, gper = dp * qb, qb * dp * (1 if diag else dp)
    hand = 2 * npad * ld * w + (nt64 * ld + ((npad // 128) * ld if diag else 0) + (nseg if nseg > 1 else 0) * gper + gper
                                + ld + 1 + qb * D) * 8 + _chunk_consts(npad, D)
    return hand - _chunk_consts(npad, D)


def predict_hess_per(npad, D, var, w, qb=128):
    """gpc_predict_hess with one block of 128 queries (shared: the raw queries, M D 8)."""
    dp, nt64, nseg = D + 1, npad // 64, max(1, min(16, npad // 512))
    ld, gper, hper = dp * qb, (qb * dp * dp if var else 0), (2 if var else 1) * (1 + D * (D + 1) // 2) * qb
    hand = ((2 if var else 1) * npad * ld + (npad * qb if var else 0)) * w + \
        (nt64 * ld + nt64 * hper + hper + (nseg if nseg > 1 else 0) * gper + gper + ld + 1 + qb * D) * 8 + _chunk_consts(npad, D)
    return hand - _chunk_consts(npad, D)


def append_block_per(npn, k, w, engine):
    """gpc_post_append_block: four fp64 panels of pad16(k) columns, the k x k products, three vectors, the three slabs of
    the k x k factorization and (engine 2) three panels of pad128(k) columns in the storage type; the hand-written
    formula less its 64 bytes of slack."""
    kq, kp = pad(k, 16), pad(k)
    hand = 4 * npn * kq * 8 + (3 * npn * kp * w if engine == 2 else 0) + kq * kq * 8 + 3 * kq * 8 + 3 * kp * kp * w + 64
    return hand - 64


def remove_per(N, k, w):
    """gpc_post_remove, the first sweep (shared: its row maps, (npn + kk) ints, which the hand-written plan left out)."""
    kk = min(k, 64)
    npn, kq, kp = pad(N - kk), pad(kk, 16), pad(kk)
    return (3 * npn * kq + (64 + kq) ** 2 + 3 * kq) * 8 + 3 * kp * kp * w


def cv_loo_per(npad):
    return 5 * npad * 8


def cv_fold_per(npad, F, kmax, engine):
    """gpc_cv with folds: per fold three k_pad^2 slabs, one vector and [quad | logdet | ld | info], engine 2's gathered
    panels, two output planes; the hand-written formula less its 64 bytes of slack."""
    kp = pad(kmax)
    hand = F * (3 * kp * kp + kp) * 8 + (F * npad * kp * 8 if engine == 2 else 0) + 2 * npad * 8 + F * 32 + 64
    return hand - 64


def budget_for_chunk(S, chunk, per, shared=0):
    """The smallest GPC_MEM_BUDGET_MB under which the planner gives `chunk` samples per chunk (None: no whole number of
    megabytes does)."""
    return next((mb for mb in range(1, 4096) if planned_chunk(S, mb, per, shared) == chunk), None)


def nll_hess_per(npad, cov_N, noise_N, mean_N, nd2):
    """gpc_nll_hess: Q, one B per plane and the operand; the vectors; the partials of the Gram and d2 passes."""
    n2, ppl, nt = npad * npad, cov_N + noise_N, npad // 64
    ntl = nt * (nt + 1) // 2
    return ((ppl + 2) * n2 + (2 * (ppl + mean_N) + noise_N + 1 + nt) * npad + nt * nt * 2 + 2 * cov_N
            + (nt * nt + 1) * (ppl * (ppl + 1) // 2) + (ntl + 1) * nd2) * 8


def cv_grad_per(npad, cov_N):
    """gpc_cv_grad: Q, Q diag(c) and their product, seven vectors, the contraction's partials (shared: npad * 8)."""
    nt = npad // 64
    ntl = nt * (nt + 1) // 2
    return (3 * npad * npad + 7 * npad + (ntl + 1) * cov_N) * 8


def hyp_grad_per(npad, D, P, nvv, ngp, msb, var, nout):
    """gpc_predict_hyp_grad with one block of `msb` padded queries."""
    n2, nt, nch = npad * npad, npad // 64, npad // 128
    d = (2 * P + 1 + nch + nt) * npad + (nt + 1) * nout * msb + msb * D + 1
    if var:
        d += n2 + 3 * npad * msb + nvv * npad + nt * msb + nt * (1 + nvv) * msb + (ngp + nvv) * msb
    return d * 8


def quad_mix_per(npad, mpad, D, var, grad):
    """gpc_quad_mix: (per sample, shared) without the M-dependent part of the shared block (see quad_mix_shared)."""
    gnt, mnt, nch = npad // 64, mpad // 64, npad // 128
    gpl = (4 if var else 2) if grad else 0
    gnq = (1 + 2 * D if grad else 1) if var else 0
    npl = gpl + (2 if var and grad else 0)
    ss = mpad * D
    d = (D + 1) * mpad + gnt * mpad + mnt * npad + npad + gnt * gpl * D * mpad + mnt * gnq * mpad + 3 * mpad + 2 + npl * ss
    if var:
        d += 2 * npad + nch * npad + gnt * mpad
    return d * 8


def quad_mix_shared(M, mpad, D):
    return (2 * mpad * D + mpad + 2 * M * D + M) * 8


def paths_create_per(npad, R, w, solve_engine):
    """gpc_paths_create: three fp64 panels of pad16(R) columns, for the MFMA solve three of pad128(R) in the storage type."""
    return 3 * npad * pad(R, 16) * 8 + (3 * npad * pad(R) * w if solve_engine == 2 else 0) + 64


def paths_eval_per(npad, mpad, fpad, R, D, engine):
    """gpc_paths_eval (shared: the results, M R S 8 (1 + D) bytes with gradients)."""
    rp = pad(R)
    eng = (max(npad, fpad) * mpad + mpad * rp + npad * rp + fpad * rp) * 8 if engine == 2 else 0
    return mpad * D * 8 + eng


def paths_eval_shared(M, R, S, D, grad):
    """... once per call: the results, and the raw queries (M D 8, which the hand-written plan left out)."""
    return M * R * S * 8 * (1 + D if grad else 1) + M * D * 8
