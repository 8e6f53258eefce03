"""lookahead_batch against the host loop it replaces -- lookahead_variance, masked argmax, update with a fantasy target on
a deep copy, q times -- on the cfg3 problem (N = 4096, D = 10, Matern-5, S = 16; bench.synthetic_problem(3, 16)) at
(M_ref, M_cand) = (1000, 1000) and (1000, 4096), q = 5, 16, 64 (GPU box).

    python tools/lookahead_batch_bench.py [--out profiles/lookahead_batch_cfg3.json] [--reps 3] [--loop-reps 1]
                                          [--sizes 1000x1000,1000x4096] [--qs 5,16,64]

Both routes run in one process on the same problem and the same points.  Per (size, q): wall time of lookahead_batch
(median, min and max of --reps after one warm-up call; every call ends in a synchronise), its device time (gpc_last_timing:
the formation of C^0; "lookahead_batch_loop_us": the q steps), the bytes the step kernel moves (S Mr Mc_pad 8 bytes read
per step, and written from step 1 on) over the device time of the WHOLE step loop -- a lower bound on the step kernel's
achieved bytes/s, the loop also holds the score, pick and column launches -- and the wall time of the host loop
(--loop-reps runs; the deep copy is timed apart).  The two selections are compared.  --dry-run prints the plan without a
device."""

import argparse
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import bench  # noqa: E402
from tools.lookahead_bench import _gp, _points, _stats  # noqa: E402


def step_bytes(S, Mr, Mc, q):
    ld = -(-Mc // 128) * 128
    return float(S) * Mr * ld * 8 * (2 * q - 1)


def resident_bytes(S, Mr, Mc, q):
    ld = -(-Mc // 128) * 128
    return float(S) * ((Mr + Mc) * ld + q * (Mr + ld)) * 8


def host_loop(gp, xr, xc, q):
    """The parent commit's way: (idx, gain (q, 1), seconds of the copy, seconds of the loop)."""
    t0 = time.perf_counter()
    g2 = copy.deepcopy(gp)
    g2.predict(xr[:1])  # (the copy rebuilds its device posteriors on first use)
    t1 = time.perf_counter()
    idx, gain, chosen = [], [], np.zeros(xc.shape[0], bool)
    for _ in range(q):
        r = g2.lookahead_variance(xc, xr)[:, 0]
        c = int(np.argmax(np.where(chosen, -np.inf, r)))
        idx.append(c)
        gain.append(r[c])
        chosen[c] = True
        g2.update(X_new=xc[c:c + 1], y_new=np.array([[0.7]]))
    return np.array(idx), np.array(gain), t1 - t0, time.perf_counter() - t1


def _row(gp, X, Mr, Mc, q, reps, loop_reps):
    from gpyreg_amd import _lib

    ctx = _lib.context(gp.device)
    xr, xc = _points(X, Mr, Mc)
    S = len(gp.posteriors)
    wall, form, loop = [], [], []
    for rep in range(-1, reps):  # (-1: the warm-up call)
        t0 = time.perf_counter()
        idx, gain = gp.lookahead_batch(xc, xr, q)
        dt = (time.perf_counter() - t0) * 1e3
        if rep >= 0:
            wall.append(dt)
            form.append(ctx.last_timing()[0])
            loop.append(ctx.get_option("lookahead_batch_loop_us") / 1e3)
    hl = [host_loop(gp, xr, xc, q) for _ in range(loop_reps)]
    h_idx, h_gain = hl[-1][0], hl[-1][1]
    same = int(np.sum(np.cumprod(h_idx == idx)))  # steps until the two selections part (rounding near a tie)
    loop_ms = float(np.median(loop))
    row = dict(case="cfg3", N=X.shape[0], D=X.shape[1], S=S, M_ref=Mr, M_cand=Mc, q=q,
               wall_ms=_stats(wall), device_formation_ms=_stats(form), device_loop_ms=_stats(loop),
               device_loop_ms_per_step=loop_ms / q, resident_bytes=resident_bytes(S, Mr, Mc, q),
               step_kernel_bytes=step_bytes(S, Mr, Mc, q),
               step_kernel_bytes_per_s_lower_bound=step_bytes(S, Mr, Mc, q) / (loop_ms * 1e-3) if loop_ms > 0 else None,
               host_loop_wall_ms=_stats([1e3 * h[3] for h in hl]), host_loop_copy_ms=_stats([1e3 * h[2] for h in hl]),
               host_loop_over_batch_wall=float(np.median([1e3 * h[3] for h in hl]) / np.median(wall)),
               steps_with_the_same_choice=same,
               gain_rel_difference_over_those=float(np.abs(h_gain[:same] - gain[:same, 0]).max() / abs(gain[0, 0])) if same else None)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-reps", type=int, default=1)
    ap.add_argument("--sizes", default="1000x1000,1000x4096")
    ap.add_argument("--qs", default="5,16,64")
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",") if s]
    qs = [int(v) for v in a.qs.split(",") if v]
    X, y, hyp = bench.synthetic_problem(3, 16)
    if a.dry_run:
        for Mr, Mc in sizes:
            for q in qs:
                print(json.dumps(dict(N=X.shape[0], D=X.shape[1], S=16, M_ref=Mr, M_cand=Mc, q=q,
                                      resident_bytes=resident_bytes(16, Mr, Mc, q), step_kernel_bytes=step_bytes(16, Mr, Mc, q))))
        return
    from gpyreg_amd import _lib

    gp = _gp(X, y, hyp)
    _lib.context(gp.device).set_option("small_timing", 1)
    rows = [_row(gp, X, Mr, Mc, q, a.reps, a.loop_reps) for Mr, Mc in sizes for q in qs]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=_lib.context(gp.device).device_info(), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
