"""GP.gradient_posterior against the only route a caller has without it, on the cfg3 problem (N = 4096, D = 10,
Matern-5, S = 16; bench.synthetic_problem(3, 16)) for M in {100, 1000} queries (GPU box).

    python tools/gradient_posterior_bench.py [--out profiles/gradient_posterior_cfg3.json] [--reps 5] [--ms 100,1000]
                                             [--stencil-block 48]

Routes, alternating inside one process (a warm-up round first; every call ends in a synchronise):
  (a) full     gradient_posterior(xs, with_value=True, separate_samples=True)
  (b) diag     gradient_posterior(xs, cov="diag", with_value=True, separate_samples=True)
  (c) stencil  predict_full on the (2 D + 1)-point stencil (x*, x* +- h_l e_l), h = 1e-3 ell, and the NumPy transform
               T C T^T per query and sample -- in blocks of --stencil-block queries, because predict_full returns the
               whole (M (2 D + 1))^2 covariance per sample (M = 1000 in one call would be 3.5 GB per sample)
Recorded: wall time per route (median, min, max), the device time of (a) and (b) (gpc_last_timing: ms_total = the device
sections, ms_factor = the products with W; "grad_post_gram_us" = the Gram passes) and of (c) summed over its calls, the
bytes the Gram pass reads (S M_pad (D + 1) N_pad 8) and its achieved bytes/s against the HBM figure of the MI355X,
and the largest relative difference between (a) and (c)."""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import bench  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X: 8 TB/s HBM3E peak


def _stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), n=len(v))


def _stencil(gp, ctx, xs, hyp, block):
    """(cov (M, D + 1, D + 1, S), device ms) by finite differences of predict_full."""
    M, D = xs.shape
    S = hyp.shape[0]
    out = np.empty((M, D + 1, D + 1, S))
    hs = 1e-3 * np.exp(hyp[:, :D]).mean(0)  # one stencil for all samples: h = 1e-3 of the mean length scale
    T = np.zeros((D + 1, 2 * D + 1))
    T[0, 0] = 1
    for l in range(D):
        T[1 + l, 1 + 2 * l], T[1 + l, 2 + 2 * l] = 0.5 / hs[l], -0.5 / hs[l]
    P = 2 * D + 1
    dev = 0.0
    for q0 in range(0, M, block):
        q = xs[q0:q0 + block]
        pts = np.repeat(q, P, axis=0)
        for l in range(D):
            pts[1 + 2 * l::P, l] += hs[l]
            pts[2 + 2 * l::P, l] -= hs[l]
        _, C = gp.predict_full(pts)
        dev += ctx.last_timing()[0]
        for j in range(q.shape[0]):
            Cj = C[j * P:(j + 1) * P, j * P:(j + 1) * P, :]
            out[q0 + j] = np.einsum("ap,pqs,bq->abs", T, Cj, T)
    return out, dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/gradient_posterior_cfg3.json")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ms", default="100,1000")
    ap.add_argument("--stencil-block", type=int, default=48)
    args = ap.parse_args()
    from gpyreg_amd import _lib

    S = 16
    X, y, hyp = bench.synthetic_problem(3, S)
    N, D = X.shape
    gp = bench.make_gp(3, "f64")
    gp.shard = False
    gp.update(X_new=X, y_new=y, hyp=hyp)
    ctx = _lib.context(0)
    npad = -(-N // 128) * 128
    rows = []
    for M in [int(m) for m in args.ms.split(",")]:
        rng = np.random.default_rng(M)
        xs = X[rng.integers(0, N, M)] + 0.3 * X.std(0, keepdims=True) * rng.standard_normal((M, D))
        mpad = -(-M // 128) * 128
        gram_bytes = float(S) * mpad * (D + 1) * npad * 8
        wall = {"full": [], "diag": [], "stencil": []}
        dev = {"full": [], "diag": [], "stencil": []}
        prod = {"full": [], "diag": []}
        gram = {"full": [], "diag": []}
        worst = None
        for rep in range(args.reps + 1):
            res = {}
            for route, kw in (("full", {}), ("diag", dict(cov="diag"))):
                t0 = time.perf_counter()
                res[route] = gp.gradient_posterior(xs, with_value=True, separate_samples=True, **kw)
                t1 = time.perf_counter()
                tot, fac = ctx.last_timing()
                if rep:
                    wall[route].append(1e3 * (t1 - t0))
                    dev[route].append(tot)
                    prod[route].append(fac)
                    gram[route].append(1e-3 * ctx.get_option("grad_post_gram_us"))
            t0 = time.perf_counter()
            fd, fd_dev = _stencil(gp, ctx, xs, hyp, args.stencil_block)
            t1 = time.perf_counter()
            if rep:
                wall["stencil"].append(1e3 * (t1 - t0))
                dev["stencil"].append(fd_dev)
            c = res["full"][1]
            worst = float((np.abs(c - fd).max(axis=(1, 2)) / np.abs(c).max(axis=(1, 2))).max())
        g_ms = float(np.median(gram["full"]))
        row = dict(M=M, M_pad=mpad, wall_ms={k: _stats(v) for k, v in wall.items()},
                   device_ms={k: _stats(v) for k, v in dev.items()},
                   products_ms={k: _stats(v) for k, v in prod.items()},
                   gram_ms={k: _stats(v) for k, v in gram.items()},
                   gram_bytes=gram_bytes, gram_bytes_per_s=gram_bytes / (1e-3 * g_ms) if g_ms > 0 else None,
                   gram_fraction_of_hbm=gram_bytes / (1e-3 * g_ms) / HBM_BYTES_PER_S if g_ms > 0 else None,
                   product_flops=2.0 * S * npad * npad * mpad * (D + 1) / 2,  # (W is lower triangular)
                   speedup_full_vs_stencil=float(np.median(wall["stencil"]) / np.median(wall["full"])),
                   speedup_diag_vs_stencil=float(np.median(wall["stencil"]) / np.median(wall["diag"])),
                   stencil_vs_full_max_rel=worst)
        rows.append(row)
        print(json.dumps(row))
    rec = dict(problem=dict(cfg=3, N=N, D=D, S=S, kernel="matern5", dtype="f64"), device=ctx.device_info(),
               reps=args.reps, stencil_block=args.stencil_block, hbm_bytes_per_s=HBM_BYTES_PER_S, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
