"""Where the wall time of cv_grad_bench.py's small problem (N = 500, S = 8) goes, and how it is distributed.

    GPYREG_AMD_LIB=<some build of libgpcore.so> python tools/cv_wall_phases.py [reps]

The bench's own loop (cv_nll_batch, nll_batch with gradient, the central differences) with the quantiles of the timed
call's wall time instead of its median alone, then the same loop with the call taken apart into its phases: the plugins'
values, posterior_batch, the device call gpc_cv_grad, and freeing the temporary posteriors.  One JSON line, milliseconds,
[min p10 p25 p50 p75 p90 max].  For an A/B of two builds run it in fresh processes that alternate between them
(profiles/consumer_scaffold_cv_wall.txt): the median of a process moves by 10 % and more from one process to the next
on one build, most of it in posterior_batch, so two or three processes per build decide nothing."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

from nll_hess_bench import _vbmc  # noqa: E402

from gpyreg_amd import _lib  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
gp, X, y, hyp = _vbmc()
gp.shard = False
gp.X, gp.y = X, y
S, P = hyp.shape
ctx = _lib.context(0)
ctx.set_option("small_timing", 1)
cov_N = gp._counts()[0]
step = 1e-4


def differences():
    for s in range(S):
        rows = np.repeat(hyp[s:s + 1], 2 * P, 0)
        rows[np.arange(P), np.arange(P)] += step
        rows[P + np.arange(P), np.arange(P)] -= step
        gp.cv_nll_batch(rows, compute_grad=False)


def q(v):
    return [round(float(np.percentile(v, p)), 4) for p in (0, 10, 25, 50, 75, 90, 100)]


wall = []
for rep in range(reps + 1):
    t0 = time.perf_counter()
    gp.cv_nll_batch(hyp)
    t1 = time.perf_counter()
    gp.nll_batch(hyp, compute_grad=True)
    differences()
    if rep:
        wall.append(1e3 * (t1 - t0))
ph = {k: [] for k in ("plugins", "post", "cv_grad", "free")}
kid, deg = gp._kid()
for rep in range(reps + 1):
    t0 = time.perf_counter()
    pv = gp._plugin_values(hyp, True)
    t1 = time.perf_counter()
    handle, _, _, info = ctx.posterior_batch(kid, deg, _lib.F64, hyp[:, :cov_N], pv["m"], pv["sn2"], pv["vec"])
    t2 = time.perf_counter()
    handle.cv_grad(cov_N, "lpd")
    t3 = time.perf_counter()
    handle.free()
    t4 = time.perf_counter()
    gp.nll_batch(hyp, compute_grad=True)
    differences()
    if rep:
        for k, a, b in (("plugins", t0, t1), ("post", t1, t2), ("cv_grad", t2, t3), ("free", t3, t4)):
            ph[k].append(1e3 * (b - a))
print(json.dumps(dict(lib=os.path.basename(_lib.LIB_PATH), quantiles="min p10 p25 p50 p75 p90 max", wall=q(wall),
                      **{k: q(v) for k, v in ph.items()})))
