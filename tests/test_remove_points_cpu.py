"""CPU-side checks of the point removal (GP.remove_points, gpc_post_remove): the NumPy restatement of the blocked
algorithm (gpyreg_amd/_remove.py: the panels and the Householder construction of csrc/remove.h) against a fresh
factorization of the reduced matrix on the models of rank1_cases.npz, the round trip with the block append, the
orthogonality of every panel's Theta, the declarations and bindings, and the parts of ``remove_points`` that need no
device."""

import os
import re

import numpy as np
import pytest
import scipy.linalg as sla

from gpyreg_amd import _remove as rm
from oracle import gp_oracle as orc
from gp_stubs import _NoDevice, _se_gp
from test_block_append_cpu import block_append_numpy, golden, parse, rel, seeded_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10


def index_sets(N):
    """name -> sorted rows to remove, for a model of N rows: the sets the issue lists, where N allows them."""
    sets = {"first": np.array([0]), "last4": np.arange(N - 4, N)}
    edges = np.array([i for i in (63, 64, 127, 128) if i < N])
    if edges.size:
        sets["edges"] = edges
    rng = np.random.default_rng(N)
    for k in (64, 65):
        if k < N - 8:
            sets["k%d" % k] = np.sort(rng.choice(N, k, replace=False))
    return sets


def sample_state(model, p, X, y):
    """(sl, m, Lo, W) of an oracle record: the fitted noise, the mean at X, and for a high-noise record the lower
    factor and its inverse."""
    d = X.shape[1]
    cov_N, noise_N = orc.cov_count(model["kernel"], d), orc.noise_count(model["noise"])
    sn2 = float(orc.noise(model["noise"], p.hyp[cov_N:cov_N + noise_N], X, y, 0))
    m = np.reshape(orc.mean(model["mean"], p.hyp[cov_N + noise_N:], X), (-1, 1))
    if not p.L_chol:
        return sn2 * p.sn2_mult, m, None, None
    Lo = p.L.T
    return sn2 * p.sn2_mult, m, Lo, sla.solve_triangular(Lo, np.eye(Lo.shape[0]), lower=True, check_finite=False)


def reduced_condition(model, p, X, sl):
    d = X.shape[1]
    K = orc.covariance(model["kernel"], p.hyp[0:orc.cov_count(model["kernel"], d)], X, degree=model.get("degree", 0))
    return np.linalg.cond(K / sl + np.eye(X.shape[0]) if p.L_chol else K + sl * np.eye(X.shape[0]))


def remove_numpy(model, posts, X, y, idx, thetas=None):
    """The removal restated on the oracle's records: new records on the reduced data (None for a stale sample)."""
    keep = np.setdiff1d(np.arange(X.shape[0]), idx)
    out = []
    for p in posts:
        sl, m, Lo, W = sample_state(model, p, X, y)
        if p.L_chol:
            L2, W2, alpha = rm.remove_high(Lo, W, idx, (y - m)[keep], sl, thetas)
            rec = orc.OraclePosterior(p.hyp, alpha, p.sW[keep], L2.T, p.sn2_mult, True)
            rec.W = W2
        else:
            A2, alpha, ok = rm.remove_low(p.L, p.alpha, idx)
            rec = orc.OraclePosterior(p.hyp, alpha, p.sW[keep], A2, p.sn2_mult, False) if ok else None
        out.append(rec)
    return out


def test_restatement_equals_a_fresh_factorization_of_the_reduced_matrix():
    g = golden()
    names = list(g["names"])
    skipped, flavours, sets_seen, worst = 0, set(), set(), 0.0
    for name in names:
        tag, model, N, D, flav = parse(name)
        X, y, hyp = g[tag + "_X"], g[tag + "_y"], g[tag + "_hyp"]
        posts = orc.posteriors(model, hyp, X, y, None)
        model_ok = True
        for sname, idx in index_sets(N).items():
            keep = np.setdiff1d(np.arange(N), idx)
            conds = [reduced_condition(model, p, X[keep], sample_state(model, p, X, y)[0]) for p in posts]
            if max(conds) >= 1e8:
                model_ok = False
                break
            thetas = []
            got = remove_numpy(model, posts, X, y, idx, thetas)
            full = orc.posteriors(model, hyp, X[keep], y[keep], None, force_mult=[p.sn2_mult for p in posts])
            for s, (a, f, p) in enumerate(zip(got, full, posts)):
                assert a is not None and a.L_chol == f.L_chol == (flav == "high"), (name, sname, s)
                errs = [rel(a.alpha, f.alpha), rel(a.L, f.L)]
                if a.L_chol:
                    Wf = sla.solve_triangular(f.L.T, np.eye(keep.size), lower=True, check_finite=False)
                    errs.append(rel(a.W, Wf))
                    assert np.array_equal(a.L, np.triu(a.L)) and np.array_equal(a.W, np.tril(a.W))
                    assert np.all(np.diag(a.L) > 0)
                    if sname == "last4":  # nothing but truncation: the bits of the old leading block
                        _, _, Lo, W = sample_state(model, p, X, y)
                        assert np.array_equal(a.L.T, Lo[:N - 4, :N - 4]) and np.array_equal(a.W, W[:N - 4, :N - 4])
                worst = max(worst, *errs)
                assert max(errs) <= TOL, (name, sname, s, errs)
            for t in thetas:  # every panel's Theta is orthogonal
                assert np.abs(t.T @ t - np.eye(t.shape[0])).sum(1).max() <= 1e-12, (name, sname)
            flavours.add(flav)
            sets_seen.add(sname)
        skipped += not model_ok
    print("worst relative error %.3g, %d of %d models skipped" % (worst, skipped, len(names)))
    assert 4 * skipped <= len(names), skipped
    assert flavours == {"high", "low"}  # both parametrisations were covered ...
    assert sets_seen == {"first", "last4", "edges", "k64", "k65"}  # ... and every index set


def test_append_five_rows_then_remove_them_gives_the_original_back():
    g = golden()
    for name in g["names"]:
        tag, model, N, D, flav = parse(name)
        X, y, hyp = g[tag + "_X"], g[tag + "_y"], g[tag + "_hyp"]
        Xn, yn = seeded_rows(X, y, 5, 105)
        posts = orc.posteriors(model, hyp, X, y, None)
        app = block_append_numpy(model, posts, X, y, Xn, yn)
        back = remove_numpy(model, app, np.concatenate([X, Xn]), np.concatenate([y, yn]), np.arange(N, N + 5))
        for s, (a, p) in enumerate(zip(back, posts)):
            assert a is not None, (name, s)
            assert rel(a.alpha, p.alpha) <= TOL and rel(a.L, p.L) <= TOL, (name, s, rel(a.alpha, p.alpha), rel(a.L, p.L))


def test_panel_theta_special_cases():
    rng = np.random.default_rng(3)
    # an identity block with a zero carrier: Theta is the identity, exactly
    theta, Dn = rm.panel_theta(np.eye(64), np.zeros((64, 7)))
    assert np.array_equal(theta, np.eye(71)) and np.array_equal(Dn, np.eye(64))
    # zero rows of the carrier (only some removed rows lie above): those reflections are the identity
    D = np.tril(rng.standard_normal((64, 64))) + 8 * np.eye(64)
    Vp = rng.standard_normal((64, 5))
    Vp[:20] = 0.0
    theta, Dn = rm.panel_theta(D, Vp)
    assert np.array_equal(Dn[:20], D[:20]) and np.array_equal(theta[:20, :20], np.eye(20))
    out = np.hstack([D, Vp]) @ theta
    assert np.abs(out[:, :64] - Dn).max() <= 1e-13 * np.abs(D).max() and np.abs(out[:, 64:]).max() <= 1e-13 * np.abs(D).max()
    assert np.array_equal(Dn, np.tril(Dn)) and np.all(np.diag(Dn) > 0)
    assert np.abs(Dn @ Dn.T - (D @ D.T + Vp @ Vp.T)).max() <= 1e-12 * np.abs(D @ D.T).max()


def _params(text, fn):
    m = re.search(r"\b%s\s*\(([^)]*)\)" % fn, text)
    assert m, fn + " is not declared in include/gpcore.h"
    return [a for a in m.group(1).split(",") if a.strip()]


def test_remove_entry_points_are_declared_and_bound():
    from gpyreg_amd import _lib

    header = open(os.path.join(ROOT, "include", "gpcore.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for fn, nargs in (("gpc_post_remove", 5), ("gpc_debug_remove_panel", 7), ("gpc_debug_remove_apply", 9)):
        assert len(_params(header, fn)) == nargs, fn
        assert fn in _lib.SIGNATURES and len(_lib.SIGNATURES[fn][1]) == nargs, fn
    assert callable(_lib.PostHandle.remove)
    assert callable(_lib.Context.debug_remove_panel) and callable(_lib.Context.debug_remove_apply)


# ---- remove_points without a device ------------------------------------------------------------------------------
HYP = np.array([[0.1, -0.1, 0.05, np.log(0.2), 0.1], [0.3, 0.2, -0.1, np.log(0.1), -0.2]])


def _gp_with_data(n=9, s2=False):
    rng = np.random.default_rng(n)
    gp = _se_gp()
    X, y = rng.standard_normal((n, 2)), rng.standard_normal((n, 1))
    gp.update(X_new=X, y_new=y, s2_new=np.full((n, 1), 0.01) + np.arange(n)[:, None] if s2 else None, hyp=HYP,
              compute_posterior=False)
    return gp, X, y


@pytest.mark.parametrize("form", ["index", "negative", "mask", "list"])
def test_remove_points_shrinks_the_data(form):
    gp, X, y = _gp_with_data(s2=True)
    s2 = gp.s2.copy()
    rows = [1, 4, 8]
    idx = {"index": np.array([4, 1, 8]), "negative": np.array([-1, 1, 4]), "list": rows,
           "mask": np.isin(np.arange(9), rows)}[form]
    gp.remove_points(idx)
    keep = np.setdiff1d(np.arange(9), rows)
    assert np.array_equal(gp.X, X[keep]) and np.array_equal(gp.y, y[keep]) and np.array_equal(gp.s2, s2[keep])
    assert gp.posteriors.shape == (2,) and np.array_equal(gp.get_hyperparameters(as_array=True), HYP)
    assert all(p.alpha is None and p.L is None for p in gp.posteriors) and gp._post_handle is None


@pytest.mark.parametrize("bad, exc", [(np.array([], dtype=int), ValueError), (np.arange(9), ValueError),
                                      (np.array([2, 2]), ValueError), (np.array([9]), IndexError),
                                      (np.array([-10]), IndexError), (np.array([0.5]), ValueError),
                                      (np.ones(8, dtype=bool), ValueError), (np.ones(9, dtype=bool), ValueError),
                                      (np.zeros(9, dtype=bool), ValueError)])
def test_remove_points_refuses_bad_indices_and_changes_nothing(bad, exc):
    gp, X, y = _gp_with_data()
    with pytest.raises(exc):
        gp.remove_points(bad)
    assert np.array_equal(gp.X, X) and np.array_equal(gp.y, y)


def test_remove_points_without_data_raises():
    with pytest.raises(ValueError):
        _se_gp().remove_points([0])


class _Handle:
    """Stands in for the resident posterior set: nothing on it may be called before the dispatch."""

    def free(self):
        pass


def _resident(gp, monkeypatch, calls, pays=True):
    """Make ``gp`` look as if its posteriors were resident and record which path remove_points takes; ``pays``: what
    the library's limit on the length of the sweep (remove.h: RM_SWEEP_MAX_PANELS) is taken to say."""
    from gpyreg_amd import _lib, gaussian_process as gpm

    monkeypatch.setattr(_lib, "context", lambda device: _NoDevice)
    for p in gp.posteriors:
        p.sn2_mult, p.L_chol = 1, True
    gp._post_handle = _Handle()
    monkeypatch.setattr(gpm.GP, "_remove_pays", lambda self, idx: pays)
    monkeypatch.setattr(gpm.GP, "_remove_resident", lambda self, idx: calls.append(("fast", tuple(idx))))
    monkeypatch.setattr(gpm.GP, "_compute_posteriors",
                        lambda self, hyp, shard=None: calls.append(("recompute", hyp.shape[0], self.X.shape[0])))


def test_remove_points_takes_the_fast_path_when_its_conditions_hold(monkeypatch):
    gp, X, y = _gp_with_data()
    calls = []
    _resident(gp, monkeypatch, calls)
    gp.remove_points(np.array([7, 2]))
    assert calls == [("fast", (2, 7))] and gp.X.shape == (7, 2)


def test_swept_panels_counts_the_panels_from_the_first_removed_row_on_per_sweep():
    assert rm.swept_panels(4096, np.arange(1)) == 64 and rm.swept_panels(4096, np.array([2048])) == 32
    assert rm.swept_panels(4096, np.arange(4032, 4096)) == 0 and rm.swept_panels(4096, np.array([4095])) == 1
    assert rm.swept_panels(130, np.array([5, 64, 129])) == 2 and rm.swept_panels(400, np.arange(336, 400)) == 1
    assert rm.swept_panels(4096, np.arange(3968, 4096)) == 1 and rm.swept_panels(400, np.arange(272, 400)) == 3
    # the sweep of the restatement visits exactly that many panels
    rng = np.random.default_rng(0)
    for N, idx in ((200, np.array([70, 199])), (150, np.sort(rng.choice(150, 70, replace=False)))):
        M = rng.standard_normal((N, N))
        Lo = np.linalg.cholesky(M @ M.T / N + np.eye(N))
        thetas = []
        rm.remove_high(Lo, np.linalg.inv(Lo), idx, np.zeros(N - idx.size), 1.0, thetas)
        assert len(thetas) == rm.swept_panels(N, idx), (N, len(thetas))


def test_the_device_path_pays_inside_both_of_the_librarys_limits_only(monkeypatch):
    from gpyreg_amd import _lib

    class _Limits(_NoDevice):
        @staticmethod
        def get_option(name):
            return {"remove_max_panels": 1, "remove_min_rows": 128}[name]

    monkeypatch.setattr(_lib, "context", lambda device: _Limits)
    gp = _se_gp()
    for N, idx, pays in ((260, [258, 259], True), (260, [0, 259], False), (260, [255], False), (260, [256], True),
                         (131, [129, 130], True), (131, [128, 129, 130], False), (100, [99], False)):
        gp.X = np.zeros((N, 2))
        assert gp._remove_pays(np.array(idx)) == pays, (N, idx)


@pytest.mark.parametrize("why", ["keyword", "s2", "sharded", "group", "vector_noise", "not_resident", "long_sweep"])
def test_every_fallback_of_remove_points_takes_the_recompute(monkeypatch, why):
    from gpyreg_amd import sharding as sh

    gp, X, y = _gp_with_data(s2=why == "s2")
    calls = []
    _resident(gp, monkeypatch, calls, pays=why != "long_sweep")
    kw = {}
    if why == "keyword":
        kw["recompute"] = True
    elif why == "sharded":
        gp._post_range = (0, 1, 2)
    elif why == "group":
        monkeypatch.setattr(sh, "active_group", lambda group: (0, 2))
    elif why == "vector_noise":
        monkeypatch.setattr(type(gp.noise), "compute", lambda self, hyp, X, y, s2, compute_grad=False: np.ones((X.shape[0], 1)))
    elif why == "not_resident":
        gp._post_handle = None
    gp.remove_points([0, 3], **kw)
    assert calls == [("recompute", 2, 7)], calls
    assert gp.X.shape == (7, 2) and gp.y.shape == (7, 1) and gp._post_handle is None
    if why == "s2":
        assert gp.s2.shape == (7, 1)
