"""Removing k points from resident posteriors: GP.remove_points (gpc_post_remove) against the full recompute on the
reduced data, on the cfg3 problem (N = 4096, D = 10, Matern-5, S = 16; bench.synthetic_problem(3, 16)) and the
PyVBMC-sized problem of tools/lookahead_bench.py (N = 400, D = 6, S = 8) and its first 100 rows (one 128-tile, where
the recompute is the two-launch small path), for k in {1, 5, 16, 64, 128} (k < N / 2) and three places of the removed
rows (GPU box):

    python tools/remove_points_bench.py [--out profiles/remove_points_cfg3.json] [--reps 3] [--ks 1,5,16] [--no-small]

  first    rows 0 .. k-1: every panel is swept, the worst case
  middle   k rows around N / 2: half the panels
  last     rows N-k .. N-1: no sweep, truncation only
Routes, alternating inside one process (a warm-up round first); every repeat of every route starts from a freshly
built posterior set of size N whose construction is outside the timed window:
  (a) remove      remove_points(idx), always the device path (the test option "remove_force": without it sweeps of
                  more than RM_SWEEP_MAX_PANELS panels are routed to (b), remove.h)
  (b) recompute   X, y assigned the kept rows, then update(hyp=...): the full recompute through the existing path
Wall time per route (median, min, max; every call ends in a synchronise) and device time (gpc_last_timing): of (a) the
whole device section and the panel sweep alone, of (b) the recompute's.  Also the shape-derived flops: a full sweep is
about 2 N^2 (64 + k)^2 / 64 per sample, the recompute about N^3.  --dry-run prints the plan and those figures without a
device."""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import bench  # noqa: E402
from block_append_bench import _gp, _stats  # noqa: E402
from lookahead_bench import _pyvbmc_problem  # noqa: E402

PLACES = ("first", "middle", "last")


def rows_to_remove(N, k, place):
    if place == "first":
        return np.arange(k)
    if place == "last":
        return np.arange(N - k, N)
    lo = N // 2 - k // 2
    return np.arange(lo, lo + k)


def flops(N, k, S, place):
    """Shape-derived: the sweeps' panels (rows below and columns left of each, 64 + kk wide, in sweeps of kk <= 64
    rows) against the recompute's factorization, inverse and W^T W of the reduced matrix."""
    n, first = N - k, int(rows_to_remove(N, k, place)[0])
    sweep = 0.0
    for j0 in range(0, k, 64):
        kk = min(64, k - j0)
        nn = N - j0 - kk
        for a in range((first // 64) * 64, nn, 64):
            sweep += 2.0 * (64 + kk) ** 2 * (max(nn - a - 64, 0) + nn)
    return dict(sweep_flops=S * sweep, recompute_flops=S * 1.0 * n**3)


def _row(X, y, hyp, k, place, reps, tag):
    from gpyreg_amd import _lib

    S, N = hyp.shape[0], X.shape[0]
    idx = rows_to_remove(N, k, place)
    keep = np.setdiff1d(np.arange(N), idx)
    routes = ("remove", "recompute")
    wall = {r: [] for r in routes}
    dev = {r: [] for r in routes}
    sweep, preds, counts = [], {}, None
    for rep in range(-1, reps):  # (-1: the warm-up round)
        for route in routes:
            gp = _gp(X, y, hyp)  # outside the timed window
            ctx = _lib.context(gp.device)
            ctx.set_option("small_timing", 1)
            ctx.set_option("remove_force", 1)  # (the device path whatever the length of the sweep: it is what is measured)
            c0 = (ctx.get_option("removed"), ctx.get_option("remove_stale"))
            t0 = time.perf_counter()
            if route == "remove":
                gp.remove_points(idx)
            else:
                gp.X, gp.y = X[keep], y[keep]
                gp.update(hyp=hyp)
            dt = (time.perf_counter() - t0) * 1e3
            if route == "remove":
                counts = (ctx.get_option("removed") - c0[0], ctx.get_option("remove_stale") - c0[1])
            if rep >= 0:
                wall[route].append(dt)
                tot, part = ctx.last_timing()
                dev[route].append(tot)
                if route == "remove":
                    sweep.append(part)
            if rep == reps - 1:
                preds[route] = gp.predict(X[:64] + 0.05, separate_samples=True)
            del gp
    row = dict(case=tag, N=N, D=X.shape[1], S=S, k=k, place=place, removed_stale=counts,
               wall_ms={r: _stats(wall[r]) for r in routes}, device_ms={r: _stats(dev[r]) for r in routes},
               device_sweep_ms=_stats(sweep), **flops(N, k, S, place),
               wall_remove_over_recompute=float(np.median(wall["remove"]) / np.median(wall["recompute"])),
               predictions_remove_against_recompute=float(max(np.abs(preds["remove"][i] - preds["recompute"][i]).max()
                                                              for i in (0, 1))))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ks", default="1,5,16,64,128")
    ap.add_argument("--no-small", action="store_true")
    ap.add_argument("--no-cfg3", action="store_true")
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    ks = [int(v) for v in a.ks.split(",") if v]
    problems = []
    if not a.no_cfg3:
        problems.append(("cfg3",) + tuple(bench.synthetic_problem(3, 16)))
    if not a.no_small:
        X, y, hyp = _pyvbmc_problem()
        problems.append(("pyvbmc", X, y, hyp))
        problems.append(("pyvbmc100", X[:100], y[:100], hyp))
    plan = [(p, k, place) for p in problems for k in ks for place in PLACES if 2 * k < p[1].shape[0]]
    if a.dry_run:
        for (tag, X, y, hyp), k, place in plan:
            print(json.dumps(dict(case=tag, N=X.shape[0], D=X.shape[1], S=hyp.shape[0], k=k, place=place,
                                  **flops(X.shape[0], k, hyp.shape[0], place))))
        return
    from gpyreg_amd import _lib

    try:
        rows = [_row(X, y, hyp, k, place, a.reps, tag) for (tag, X, y, hyp), k, place in plan]
    finally:  # (_row lifts the limit on the length of the sweep on the shared context)
        _lib.context(0).set_option("remove_force", 0)
    out = dict(device=_lib.context(0).device_info(), rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
