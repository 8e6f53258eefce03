"""The scratch of one sample of the chunked posterior consumers, in bytes, as closed forms, and the chunk that the
library's planner derives from them under GPC_MEM_BUDGET_MB.

These are the formulas that gpcore.hip carried as `per_sample(...)` before its scratch blocks were declared once through
ScratchCarver, restated here so that the chunking tests can say which chunk a budget must give: the library reports the
chunk it planned as the option "last_chunk", and a layout that lost or gained an array shows up as a different chunk (or
as the same chunk at a budget chosen near a border).  Nothing here is read from the library."""


def pad(n, t=128):
    return -(-n // t) * t


def planned_chunk(S, mb, per, shared=0):
    """plan_chunk under a forced budget of `mb` megabytes: 80 % of it, less `shared`, divided by `per`; 0 = refused."""
    budget = int((mb << 20) * 0.8)
    return 0 if budget < shared + per else min(S, (budget - shared) // per)


def rhs_per(npad, mpad, full, w):
    """gpc_predict, gpc_predict_full, gpc_quad, gpc_predict_K (rhs_products without gradients or draws): the right-hand
    side and the product, npad x mpad each, and with `full` the mpad x mpad covariance, in the storage type (w bytes)."""
    return (2 * npad * mpad + (mpad * mpad if full else 0)) * w


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
