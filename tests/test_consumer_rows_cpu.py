"""The per-sample row protocol of the posterior consumers (GP._device_rows), without a device.

First the helper alone, behind a stand-in handle: what an unsharded GP hands on, what a rank without a sample
contributes, the refusal of a cleaned GP.  Then every public consumer over gloo: a GP whose samples are sharded over
the ranks must return, to the bit, what an unsharded GP returns from the same per-sample device values.  The values
come from a stand-in for ``_lib.PostHandle`` that draws arrays of the documented shapes from seeded generators for all
S samples and hands out this rank's columns; they mean nothing: what is under test is packing, gather order and
unpacking.  The second part uses the public methods and the attributes ``_post_handle`` / ``_post_range`` / ``_ctx``
only, so it describes the behaviour of the consumers and not of the helper."""

import os
import socket
import sys

import numpy as np
import pytest

from gp_stubs import _NoDevice, _se_gp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, M, MB, R = 12, 2, 3, 4, 2  # training points, dimensions, query points, points of the second set, draws
MULT = (1, 10, 100)  # sn2_mult of the samples
LCHOL = (True, False, True)  # their L_chol: reference_quirks rescales the quadrature's solve term of the True ones only


class _Handle:
    """Quacks like ``_lib.PostHandle`` for the samples [lo, hi) of S: every consumer method returns arrays of the
    documented shapes, drawn for ALL S samples from a generator seeded per method and cut to this block."""

    def __init__(self, S, lo, hi):
        self.S, self.lo, self.hi = S, lo, hi

    def _last(self, seed, *shape):  # sample axis last
        return np.random.default_rng(seed).uniform(0.5, 1.5, shape + (self.S,))[..., self.lo:self.hi].copy()

    def _first(self, seed, *shape):  # sample axis first
        return np.random.default_rng(seed).uniform(0.5, 1.5, (self.S,) + shape)[self.lo:self.hi].copy()

    def predict(self, x_star):
        m = x_star.shape[0]
        return self._last(1, m), self._last(2, m)

    def predict_grad(self, x_star):
        m, d = x_star.shape
        return self._last(3, m), self._last(4, m), self._last(5, m, d), self._last(6, m, d)

    def grad_post(self, x_star, diag_only=False):
        m, d = x_star.shape
        return self._last(7, m), self._last(8, m, d), self._last(9, *((m, d + 1) if diag_only else (m, d + 1, d + 1)))

    def predict_hess(self, x_star, compute_var=True):
        m, d = x_star.shape
        var = [self._last(13, m), self._last(14, m, d), self._last(15, m, d, d)] if compute_var else [None] * 3
        return self._last(10, m), var[0], self._last(11, m, d), var[1], self._last(12, m, d, d), var[2]

    def predict_full(self, x_star):
        m = x_star.shape[0]
        return self._last(16, m), self._first(17, m, m)

    def predict_cov(self, x_a, x_b, weights=None, want_cov=True, want_fs2=False):
        ma, mb = x_a.shape[0], x_b.shape[0]
        cov = self._first(18, ma, mb) if want_cov else None
        wsq = None
        if weights is not None:  # (the first row of the weights: per sample, this block's columns must have come)
            assert weights.shape in ((ma,), (ma, self.hi - self.lo))
            wsq = self._last(19, mb) * weights[0]
        return cov, wsq, self._last(20, mb) if want_fs2 else None

    def draw(self, x_star, n_draws, seed, s_offset=0, noise_sd=None):
        assert s_offset == self.lo
        f = self._last(21 + seed, x_star.shape[0], n_draws)
        if noise_sd is not None:
            assert noise_sd.shape == (x_star.shape[0], self.hi - self.lo)
            f += noise_sd[:, None, :]
        return f, self._last(22)

    def cv(self, folds=None):
        f = N if folds is None else len(folds)
        info = np.zeros((f, self.hi - self.lo), dtype=np.int32)
        return self._last(23, N), self._last(24, N), self._last(25, f), self._last(26, f), info

    def quad(self, mu, sigma, compute_var):
        m = mu.shape[0]
        return self._last(27, m), self._last(28, m) if compute_var else None

    def quad_grad(self, mu, sigma, compute_var):
        m, d = mu.shape
        var = [self._last(32, m), self._last(33, m, d), self._last(34, m, d)] if compute_var else [None] * 3
        return self._last(29, m), var[0], self._last(30, m, d), self._last(31, m, d), var[1], var[2]

    def quad_cov(self, mu, sigma):
        m = mu.shape[0]
        return self._last(35, m), self._first(36, m, m)

    def quad_mix(self, mu, sigma, w, compute_var, compute_grad):
        m, d = mu.shape
        both = compute_var and compute_grad
        row = lambda seed, on: self._last(seed, m) if on else None  # noqa: E731
        plane = lambda seed, on: self._last(seed, m, d) if on else None  # noqa: E731
        return dict(za=row(37, True), zbkzb=self._last(38) if compute_var else None, gw=row(39, compute_var),
                    zq=row(40, compute_var), dza_dmu=plane(41, compute_grad), dza_dsigma=plane(42, compute_grad),
                    dzq_dmu=plane(43, both), dzq_dsigma=plane(44, both), dgw_dmu=plane(45, both),
                    dgw_dsigma=plane(46, both))

    def free(self):
        pass


def _gp(S, block=None, quirks=False):
    """A GP with S hyperparameter samples and no device: the stand-in handle over all samples, or -- ``block`` =
    (lo, hi) -- sharded, holding that block (no handle at all when the block is empty).  Every record has its own
    ``sn2_mult``, ``L_chol`` and ``sW``, which is what the ``reference_quirks`` rescaling reads."""
    rng = np.random.default_rng(0)
    X = rng.uniform(-1, 1, (N, D))
    y = np.sin(X.sum(1, keepdims=True))
    hyp = 0.1 * rng.standard_normal((S, D + 3))
    gp = _se_gp(D=D, quirks=quirks)
    gp.update(X_new=X, y_new=y, hyp=hyp, compute_posterior=False)
    gp._ctx = lambda: None
    for s, p in enumerate(gp.posteriors):
        p.sn2_mult, p.L_chol, p.sW = MULT[s], LCHOL[s], np.full((N, 1), 3.0 + s)
    if block is None:
        gp._post_handle = _Handle(S, 0, S)
    else:
        lo, hi = block
        gp._post_handle = _Handle(S, lo, hi) if hi > lo else None
        gp._post_range = (lo, hi, S)
    return gp


# ---------------------------------------------------------------- the helper alone
def _layout_and_fields(k, with_optional):
    rng = np.random.default_rng(5)
    layout = [("scalar", ()), ("row", (M,)), ("plane", (M, D)), ("cube", (M, D, D))]
    if with_optional:
        layout.append(("optional", (M,)))
    return layout, [rng.standard_normal(tuple(shape) + (k,)) for _, shape in layout]


@pytest.mark.parametrize("with_optional", [False, True])
def test_unsharded_fields_pass_through_untouched(monkeypatch, with_optional):
    from gpyreg_amd import _lib

    monkeypatch.setattr(_lib, "context", lambda device=None: _NoDevice())
    gp = _gp(3)
    layout, fields = _layout_and_fields(3, with_optional)
    seen = []

    def call(handle, local_posts, lo):
        seen.append((handle, len(local_posts), lo))
        return fields

    got = gp._device_rows(call, layout, np.zeros(2))
    assert seen == [(gp._post_handle, 3, 0)]
    assert list(got) == [n for n, _ in layout] and ("optional" in got) == with_optional
    assert all(got[n] is f for (n, _), f in zip(layout, fields))  # the very objects: no concatenate, no copy


def test_unsharded_predict_cov_is_a_view_of_the_device_result(monkeypatch):
    """The handle's covariance is sample-first; unsharded, ``predict_cov`` hands out its (Ma, Mb, S) view, no copy."""
    from gpyreg_amd import _lib

    monkeypatch.setattr(_lib, "context", lambda device=None: _NoDevice())
    gp = _gp(3)
    made = []
    inner = gp._post_handle.predict_cov
    monkeypatch.setattr(gp._post_handle, "predict_cov", lambda *a, **k: made.append(inner(*a, **k)) or made[-1])
    rng = np.random.default_rng(2)
    cov = gp.predict_cov(rng.uniform(-1, 1, (M, D)), rng.uniform(-1, 1, (MB, D)))
    assert cov.shape == (M, MB, 3) and np.shares_memory(cov, made[0][0])
    assert cov.strides == (MB * 8, 8, M * MB * 8) and np.array_equal(cov, made[0][0].transpose(1, 2, 0))


def test_a_rank_without_a_sample_contributes_empty_fields(monkeypatch):
    """``_post_handle = None`` with ``_post_range = (2, 2, 2)``: ``call`` does not run, and what goes into the gather
    has shape + (0,) per field of the layout."""
    from gpyreg_amd import _lib

    monkeypatch.setattr(_lib, "context", lambda device=None: _NoDevice())
    gp = _gp(2, block=(2, 2))
    layout, full = _layout_and_fields(2, True)
    heights = [int(np.prod(shape)) for _, shape in layout]
    sent = []

    def gather(rows, *key):  # stands in for the exchange: the other ranks' columns arrive
        sent.append((rows, key))
        return np.concatenate([f.reshape(h, 2) for f, h in zip(full, heights)], axis=0)

    monkeypatch.setattr(gp, "_gather_samples", gather)

    def call(handle, local_posts, lo):
        raise AssertionError("call must not run on a rank without samples")

    key = (np.ones(3), 7)
    got = gp._device_rows(call, layout, *key)
    assert len(sent) == 1 and sent[0][0].shape == (sum(heights), 0) and sent[0][1] == key
    for (n, shape), f in zip(layout, full):
        assert got[n].shape == tuple(shape) + (2,) and np.array_equal(got[n], f)


def test_a_cleaned_gp_is_refused_before_call(monkeypatch):
    from gpyreg_amd import _lib

    monkeypatch.setattr(_lib, "context", lambda device=None: _NoDevice())
    gp = _gp(2)
    gp.clean()
    ran = []
    with pytest.raises(ValueError, match="posteriors have been cleaned"):
        gp._device_rows(lambda handle, local_posts, lo: ran.append(1), [("row", (M,))])
    assert not ran


# ---------------------------------------------------------------- every consumer, sharded against unsharded, over gloo
def _arguments(S, perturb=False):
    """The consumers' arguments; ``perturb``: one entry of each differs (a rank that was called with something else)."""
    rng = np.random.default_rng(1)
    a = dict(x=rng.uniform(-1, 1, (M, D)), xb=rng.uniform(-1, 1, (MB, D)), y=rng.uniform(-1, 1, (M, 1)),
             mu=rng.uniform(-1, 1, (2, D)), sigma=rng.uniform(0.3, 1.0, (2, D)), wm=rng.uniform(0.5, 1.5, 2),
             w1=rng.uniform(0.5, 1.5, M), ws=rng.uniform(0.5, 1.5, (M, S)), seed=3,
             folds=[np.array([0, 5, 7]), np.array([2, 3])])
    if perturb:
        for k in ("x", "xb", "mu", "wm", "w1", "ws"):
            a[k].flat[0] += 0.25
        a["seed"] = 4
        a["folds"] = [np.array([0, 5, 8]), np.array([2, 3])]
    return a


def _consumers(a):
    """name -> call on a GP, for every public consumer and every switch that changes what is packed."""
    c = {}
    for sep in (True, False):
        t = " separate" if sep else " mixture"
        c["predict" + t] = lambda gp, sep=sep: gp.predict(a["x"], a["y"], separate_samples=sep, return_lpd=True)
        c["predict_grad" + t] = lambda gp, sep=sep: gp.predict_grad(a["x"], add_noise=True, separate_samples=sep)
        for cov in ("full", "diag"):
            for val in (False, True):
                c[f"gradient_posterior {cov} {val}" + t] = lambda gp, sep=sep, cov=cov, val=val: \
                    gp.gradient_posterior(a["x"], cov=cov, with_value=val, separate_samples=sep)
        for var in (True, False):
            c[f"predict_hess {var}" + t] = lambda gp, sep=sep, var=var: \
                gp.predict_hess(a["x"], compute_var=var, separate_samples=sep)
            c[f"quad {var}" + t] = lambda gp, sep=sep, var=var: \
                gp.quad(a["mu"], a["sigma"], compute_var=var, separate_samples=sep)
            c[f"quad_grad {var}" + t] = lambda gp, sep=sep, var=var: \
                gp.quad_grad(a["mu"], a["sigma"], compute_var=var, separate_samples=sep)
            for grad in (True, False):
                c[f"quad_mixture {var} {grad}" + t] = lambda gp, sep=sep, var=var, grad=grad: \
                    gp.quad_mixture(a["mu"], a["sigma"], a["wm"], compute_var=var, compute_grad=grad,
                                    separate_samples=sep)
        c["lookahead_variance 1-D weights" + t] = lambda gp, sep=sep: \
            gp.lookahead_variance(a["xb"], a["x"], weights=a["w1"], separate_samples=sep)
        c["lookahead_variance per-sample weights" + t] = lambda gp, sep=sep: \
            gp.lookahead_variance(a["xb"], a["x"], weights=a["ws"], separate_samples=sep)
        c["cv_predict loo" + t] = lambda gp, sep=sep: gp.cv_predict(None, separate_samples=sep, return_lpd=True)
        c["cv_predict folds" + t] = lambda gp, sep=sep: gp.cv_predict(a["folds"], separate_samples=sep, return_lpd=True)
        c["quad_cov" + t] = lambda gp, sep=sep: gp.quad_cov(a["mu"], a["sigma"], separate_samples=sep)
    c["predict_full"] = lambda gp: gp.predict_full(a["x"], add_noise=True)
    c["predict_cov"] = lambda gp: gp.predict_cov(a["x"], a["xb"])
    c["draw_functions"] = lambda gp: gp.draw_functions(a["x"], n_draws=R, add_noise=True, seed=a["seed"],
                                                       return_jitter=True)
    return c


def _same(got, want):
    got, want = (list(v) if isinstance(v, tuple) else [v] for v in (got, want))
    return len(got) == len(want) and all(
        (g is None and w is None) or (g is not None and w is not None and np.shape(g) == np.shape(w)
                                      and np.array_equal(np.asarray(g), np.asarray(w)))
        for g, w in zip(got, want))


def _worker(rank, world, port, S, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist

    from gpyreg_amd import _lib, sharding

    _lib.context = lambda device=None: _NoDevice()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        lo, hi = sharding.shard_bounds(S, rank, world)
        sharded, whole = _gp(S, block=(lo, hi)), _gp(S)
        a = _arguments(S)
        differ = []  # the consumers whose sharded result is not the unsharded one, to the bit
        for name, call in _consumers(a).items():
            want = call(whole)
            assert all(np.all(np.isfinite(v)) for v in (want if isinstance(want, tuple) else [want]) if v is not None)
            if not _same(call(sharded), want):
                differ.append(name)
        # the quadrature calls again under reference_quirks, whose per-sample rescaling acts on the local block
        sharded_q, whole_q = _gp(S, block=(lo, hi), quirks=True), _gp(S, quirks=True)
        for name, call in _consumers(a).items():
            if name.startswith("quad"):
                want, plain = call(whole_q), call(whole)
                if name.split()[1] != "False":  # (with a variance: the rescaling must have changed it)
                    assert not _same(want, plain), name
                if not _same(call(sharded_q), want):
                    differ.append(name + " quirks")
        # rank 1 is called with other arguments: ShardError on EVERY rank, for every consumer's own key
        silent = []
        for name, call in _consumers(_arguments(S, perturb=(rank == 1))).items():
            if name.startswith("cv_predict loo"):  # (leave-one-out has no argument that could differ)
                continue
            try:
                call(sharded)
                silent.append(name)
            except sharding.ShardError:
                pass
        q.put((rank, differ, silent))
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("world, S", [(2, 3), (3, 2)])  # blocks of 2 + 1; one rank holds nothing
def test_sharded_consumers_equal_unsharded_to_the_bit(world, S):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, S, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert [r[0] for r in res] == list(range(world))
    for rank, differ, silent in res:
        assert differ == [], (rank, differ)
        assert silent == [], (rank, silent)
