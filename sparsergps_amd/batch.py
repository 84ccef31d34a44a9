"""Batched small-knot VI fits: many independent problems per launch.

  SparseGPBatch                B problems (row ranges of one resident X / y / mu), each with its own
                               theta and at most 64 knots: sgp_batch_* of include/sgp.h
  norm_grad_ascent_vi_batch    B norm_grad_ascent_vi runs (R/vi_functions.R:606-1218) in lockstep,
                               one batch evaluation per iteration
  optimize_gp_batch            optimize_gp(family = "gaussian", sparse = TRUE, vi = TRUE,
                               xu_opt = "fixed") for a list of problems
  SparseGPBatch.set_test / predict / score
                               predict_vi (R/vi_functions.R:1222-1336) and score_gp's figures for
                               every problem's held-out rows, from the posteriors the batch holds
                               on the device
  cross_validate_gp            k-fold cross-validation: the folds fitted in lockstep and scored on
                               one batch

Per problem the semantics are the single fit's (drivers._ascent with the knots fixed); a problem
that meets its stop rule is retired through the evaluation's `active` mask while the others go
on.  The path is opt-in: nothing else in the package routes to it.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import numpy as np

from . import _lib
from .covariance import theta_vector
from .drivers import _opts
from .vi import param_names

MMAX = _lib.SGP_BATCH_MMAX


def _mat(xy, n):
    return np.asarray(xy, dtype=np.float64).reshape(n, -1)


class SparseGPBatch:
    """B independent problems on rows of one device-resident X / y / mu.

    xy (n x d), y (n); mu: n values, a scalar, or None for each problem's own mean(y) (quirk Q14;
    with overlapping ranges the later problem's mean stands on the shared rows).  row0 / nrow: the
    problems' row ranges (None: one problem of all rows); ranges may overlap or coincide."""

    def __init__(self, xy, y, mu=None, row0=None, nrow=None, device=None):
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
        X = np.asfortranarray(_mat(xy, y.size))
        n, d = X.shape
        if row0 is None and nrow is None:
            row0, nrow = [0], [n]
        self.row0 = np.ascontiguousarray(np.asarray(row0, dtype=np.int64).reshape(-1))
        self.nrow = np.ascontiguousarray(np.asarray(nrow, dtype=np.int64).reshape(-1))
        if self.row0.size != self.nrow.size:
            raise ValueError("SparseGPBatch: row0 and nrow differ in length")
        self.B, self.n, self.d = int(self.row0.size), n, d
        self.X, self.y = X, y
        self.mu = self._mu(mu, y)
        self._lib = _lib.lib()
        self._h = C.c_void_p()
        self._state = [None] * self.B      # knot count of the last successful evaluation
        i64 = lambda a: a.ctypes.data_as(_lib.c_int64_p)   # noqa: E731
        _lib.check(self._lib.sgp_batch_create(
            C.byref(self._h), 0 if device is None else int(device), _lib.dptr(X), n, n, d,
            _lib.dptr(y), _lib.dptr(self.mu), i64(self.row0), i64(self.nrow), self.B))

    def _mu(self, mu, y):
        if mu is None or (np.ndim(mu) == 0 and not np.isfinite(mu)):
            out = np.empty_like(y)
            for r0, nr in zip(self.row0, self.nrow):
                if 0 <= r0 and nr >= 1 and r0 + nr <= y.size:
                    out[r0:r0 + nr] = y[r0:r0 + nr].mean()
            return out
        return np.ascontiguousarray(np.broadcast_to(np.asarray(mu, dtype=np.float64), y.shape))

    @classmethod
    def from_problems(cls, problems, device=None):
        """problems: [(xy_b, y_b, mu_b), ...] (mu_b may be None: mean(y_b)); rows concatenated."""
        xs, ys, mus, row0, nrow = [], [], [], [], []
        at = 0
        for prob in problems:
            xy, y = prob[0], np.asarray(prob[1], dtype=np.float64).reshape(-1)
            mu = prob[2] if len(prob) > 2 else None
            if mu is None or (np.ndim(mu) == 0 and not np.isfinite(mu)):
                mu = y.mean()
            xs.append(_mat(xy, y.size))
            ys.append(y)
            mus.append(np.broadcast_to(np.asarray(mu, dtype=np.float64), y.shape))
            row0.append(at)
            nrow.append(y.size)
            at += y.size
        if len({x.shape[1] for x in xs}) != 1:
            raise ValueError("SparseGPBatch.from_problems: the problems differ in dimension")
        return cls(np.vstack(xs), np.concatenate(ys), np.concatenate(mus), row0, nrow, device)

    # ------------------------------------------------------------------ data of one problem
    def rows(self, b):
        r0, nr = int(self.row0[b]), int(self.nrow[b])
        return self.X[r0:r0 + nr], self.y[r0:r0 + nr], self.mu[r0:r0 + nr]

    def set_data(self, y, mu=None):
        self._need()
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
        if y.size != self.n:
            raise ValueError(f"set_data: {y.size} values for {self.n} rows")
        mu = self._mu(mu, y)
        _lib.check(self._lib.sgp_batch_set_data(self._h, _lib.dptr(y), _lib.dptr(mu)))
        self.y, self.mu = y, mu
        self._state = [None] * self.B

    # ------------------------------------------------------------------ evaluation
    def eval_raw(self, cov_fun, theta, xus, delta, flags, active, obj, grad, status):
        """sgp_batch_eval_vi on caller-owned arrays: theta (B x P, row b = problem b), xus a list
        of m_b x d knot arrays (entries of inactive problems may be None), active a uint8 array
        or None, obj (B), grad (B x P, or None with SGP_FLAG_OBJ_ONLY), status (B, int32).
        Slots of inactive problems are left as they are."""
        self._need()
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        on = [active is None or bool(active[b]) for b in range(self.B)]
        packs = [np.asfortranarray(_mat(xus[b], np.shape(xus[b])[0])).reshape(-1, order="F")
                 if on[b] else np.zeros(0) for b in range(self.B)]
        m = np.array([np.shape(xus[b])[0] if on[b] else 0 for b in range(self.B)], dtype=np.int64)
        for b in range(self.B):
            if on[b] and packs[b].size != m[b] * self.d:
                raise ValueError(f"problem {b}: knots are not m x {self.d}")
        uoff = np.concatenate([[0], np.cumsum([p.size for p in packs])[:-1]]).astype(np.int64)
        U = np.concatenate(packs + [np.zeros(1)])
        act = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
        i64 = lambda a: a.ctypes.data_as(_lib.c_int64_p)   # noqa: E731
        st = self._lib.sgp_batch_eval_vi(
            self._h, _lib.KERNELS.get(cov_fun, -1), _lib.dptr(theta), theta.shape[1], _lib.dptr(U),
            i64(uoff), i64(m), float(delta), int(flags),
            None if act is None else act.ctypes.data_as(_lib.c_ubyte_p), _lib.dptr(obj),
            None if grad is None else _lib.dptr(grad), 0 if grad is None else grad.shape[1],
            status.ctypes.data_as(_lib.c_int_p))
        _lib.check(st)
        for b in range(self.B):
            if on[b] and status[b] == 0:
                self._state[b] = int(m[b])

    def eval_vi(self, cov_pars, cov_fun, xus, delta=1e-6, active=None, obj_only=False,
                r_det=False):
        """One evaluation of the batch.  cov_pars: B dicts, xus: B knot arrays (entries of
        inactive problems are not read).  Returns (obj[B], grad, status[B]): grad a list of
        OrderedDicts in each cov_par's key order (None for inactive problems and with
        obj_only); a problem with status != 0 has NaN obj and grad (chol()'s leading-minor order:
        > 0 for Sigma22, < 0 for Sigma22 + t(Sigma12) %*% ZSig12).  Inactive slots are NaN / 0."""
        P = (self.d if cov_fun == "ard" else 1) + 2
        theta = np.ones((self.B, P))
        on = [active is None or bool(active[b]) for b in range(self.B)]
        for b in range(self.B):
            if on[b]:
                theta[b] = theta_vector(cov_pars[b], cov_fun, self.d)
        obj = np.full(self.B, np.nan)
        g = None if obj_only else np.full((self.B, P), np.nan)
        status = np.zeros(self.B, dtype=np.int32)
        flags = (_lib.SGP_FLAG_OBJ_ONLY if obj_only else 0) | (_lib.SGP_FLAG_R_DET if r_det else 0)
        self.eval_raw(cov_fun, theta, xus, delta, flags, active, obj, g, status)
        names = param_names(cov_fun, self.d)
        grads = []
        for b in range(self.B):
            if g is None or not on[b]:
                grads.append(None)
                continue
            byname = dict(zip(names, g[b]))
            grads.append(OrderedDict((k, float(byname[k])) for k in cov_pars[b].keys()))
        return obj, grads, status

    def posterior_u(self, muus):
        """(u_mean list, u_var list): the knot posterior of each problem's last successful
        evaluation (None for a problem that has none)."""
        self._need()
        ms = [0 if s is None else s for s in self._state]
        muu = np.concatenate([np.broadcast_to(np.asarray(muus[b], dtype=np.float64), (ms[b],))
                              if ms[b] else np.zeros(0) for b in range(self.B)] + [np.zeros(1)])
        um = np.zeros(sum(ms) + 1)
        uv = np.zeros(sum(k * k for k in ms) + 1)
        _lib.check(self._lib.sgp_batch_posterior_u(self._h, _lib.dptr(muu), _lib.dptr(um),
                                                   _lib.dptr(uv)))
        means, covs, o1, o2 = [], [], 0, 0
        for k, s in zip(ms, self._state):
            means.append(None if s is None else um[o1:o1 + k].copy())
            covs.append(None if s is None else uv[o2:o2 + k * k].reshape(k, k, order="F").copy())
            o1 += k
            o2 += k * k
        return means, covs

    def stage_ms(self, enable=True):
        """HIP-event times (ms) of the last evaluation's four stages; records from the next on."""
        self._need()
        out = np.zeros(4)
        _lib.check(self._lib.sgp_diag_batch_timing(self._h, int(bool(enable)), _lib.dptr(out)))
        return out

    # ------------------------------------------------------------------ held-out prediction
    def set_test(self, x_test, y_test=None, mu_test=None, row0=None, nrow=None):
        """The held-out rows (sgp_batch_set_test): x_test (nt x d), y_test (nt, or None: predict
        only), mu_test (nt values, a scalar, or None for zeros: score_gp's rule for mu_pred);
        problem b's test rows are [row0[b], row0[b] + nrow[b]) (None: all rows for every
        problem).  Ranges may overlap; nrow[b] = 0 is allowed.  A repeated call replaces them."""
        self._need()
        X = np.asarray(x_test, dtype=np.float64)
        X = np.asfortranarray(X.reshape(-1, self.d) if X.ndim != 2 else X)
        nt = X.shape[0]
        if X.shape[1] != self.d:
            raise ValueError(f"set_test: x_test has {X.shape[1]} columns, the batch {self.d}")
        yt = None if y_test is None else \
            np.ascontiguousarray(np.asarray(y_test, dtype=np.float64).reshape(-1))
        if yt is not None and yt.size != nt:
            raise ValueError(f"set_test: {yt.size} y_test values for {nt} rows")
        mut = np.zeros(nt) if mu_test is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(mu_test, dtype=np.float64), (nt,)))
        if row0 is None and nrow is None:
            row0, nrow = [0] * self.B, [nt] * self.B
        r0 = np.ascontiguousarray(np.asarray(row0, dtype=np.int64).reshape(-1))
        nr = np.ascontiguousarray(np.asarray(nrow, dtype=np.int64).reshape(-1))
        if r0.size != self.B or nr.size != self.B:
            raise ValueError(f"set_test: row0 and nrow must have one entry per problem ({self.B})")
        i64 = lambda a: a.ctypes.data_as(_lib.c_int64_p)   # noqa: E731
        _lib.check(self._lib.sgp_batch_set_test(
            self._h, _lib.dptr(X), nt, nt, None if yt is None else _lib.dptr(yt), _lib.dptr(mut),
            i64(r0), i64(nr)))
        self._test = (r0, nr, np.concatenate([[0], np.cumsum(nr)]).astype(np.int64), yt)

    def set_test_problems(self, tests):
        """tests: [(x_b, y_b, mu_b), ...], one per problem (y_b None in all of them: predict only;
        mu_b None: zeros), concatenated as from_problems concatenates the training rows."""
        if len(tests) != self.B:
            raise ValueError(f"set_test_problems: {len(tests)} test sets for {self.B} problems")
        xs, ys, mus, row0, nrow = [], [], [], [], []
        at = 0
        for t in tests:
            x = np.asarray(t[0], dtype=np.float64)
            x = x.reshape(-1, self.d) if x.ndim != 2 else x
            y = t[1] if len(t) > 1 else None
            mu = t[2] if len(t) > 2 else None
            xs.append(x)
            ys.append(None if y is None else np.asarray(y, dtype=np.float64).reshape(-1))
            mus.append(np.broadcast_to(np.asarray(0.0 if mu is None else mu, dtype=np.float64),
                                       (x.shape[0],)))
            row0.append(at)
            nrow.append(x.shape[0])
            at += x.shape[0]
        if any(y is None for y in ys) and not all(y is None for y in ys):
            raise ValueError("set_test_problems: y is given for some problems and not for others")
        self.set_test(np.vstack(xs), None if ys[0] is None else np.concatenate(ys),
                      np.concatenate(mus), row0, nrow)

    def predict_raw(self, active, pred_mean, pred_var, nlp=None, stats=None):
        """sgp_batch_predict on caller-owned arrays: pred_mean, pred_var (and nlp) of sum nrow
        values, packed per problem in problem order, stats (B x 4); nlp and stats both or
        neither.  Slots of inactive problems are left as they are."""
        self._need()
        act = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
        _lib.check(self._lib.sgp_batch_predict(
            self._h, None if act is None else act.ctypes.data_as(_lib.c_ubyte_p),
            _lib.dptr(pred_mean), _lib.dptr(pred_var), None if nlp is None else _lib.dptr(nlp),
            None if stats is None else _lib.dptr(stats)))

    def _run_predict(self, active, score):
        self._need()
        test = getattr(self, "_test", None)
        tot = int(test[2][-1]) if test else 0
        pm, pv = np.full(tot + 1, np.nan), np.full(tot + 1, np.nan)
        nlp = np.full(tot + 1, np.nan) if score else None
        stats = np.zeros((self.B, 4)) if score else None
        self.predict_raw(active, pm, pv, nlp, stats)
        return test, pm, pv, nlp, stats

    def predict(self, active=None):
        """predict_vi for every active problem on its test rows, from the posterior of its last
        successful evaluation: a list of {"pred_mean": (n_b, 1), "pred_var": (n_b,)}, None for
        inactive problems."""
        (_, nr, off, _), pm, pv, _, _ = self._run_predict(active, False)
        return [None if active is not None and not active[b] else
                {"pred_mean": pm[off[b]:off[b] + nr[b]].reshape(-1, 1).copy(),
                 "pred_var": pv[off[b]:off[b] + nr[b]].copy()} for b in range(self.B)]

    def score(self, active=None):
        """score_gp(vi = True) for every active problem on its test rows: a list of {"pred",
        "nlp", "median_nlp", "mean_nlp", "rmse", "srmse", "n_nan"} dicts (None for inactive
        problems), the nlp with each problem's own tau."""
        self._need()
        test = getattr(self, "_test", None)
        if test is not None and test[3] is None:
            raise ValueError("SparseGPBatch.score: set_test was given no y_test")
        (r0, nr, off, yt), pm, pv, nlp, stats = self._run_predict(active, True)
        out = []
        for b in range(self.B):
            if active is not None and not active[b]:
                out.append(None)
                continue
            n, o = int(nr[b]), int(off[b])
            st = stats[b] if n else np.zeros(4)
            y = yt[r0[b]:r0[b] + n]
            v = nlp[o:o + n].copy()
            rmse = float(np.sqrt(st[3] / n)) if n else float("nan")
            sd = float(np.std(y, ddof=1)) if n > 1 else float("nan")
            fin = v[np.isfinite(v)]
            out.append({"pred": {"pred_mean": pm[o:o + n].reshape(-1, 1).copy(),
                                 "pred_var": pv[o:o + n].copy()},
                        "nlp": v,
                        "median_nlp": float(np.median(fin)) if fin.size else float("nan"),
                        "mean_nlp": float(st[0] / st[1]) if st[1] > 0 else float("nan"),
                        "rmse": rmse, "srmse": rmse / sd, "n_nan": int(st[2])})
        return out

    def predict_stage_ms(self, enable=True):
        """HIP-event times (ms) of the last predict / score's three stages (the m x m stage, the
        row pass, the finish); records from the next call on."""
        self._need()
        out = np.zeros(3)
        _lib.check(self._lib.sgp_diag_batch_predict_timing(self._h, int(bool(enable)),
                                                           _lib.dptr(out)))
        return out

    # ------------------------------------------------------------------ lifetime
    def _need(self):
        if not self._h:
            raise RuntimeError("SparseGPBatch is closed")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sgp_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _not_pd(status):
    which = "Sigma22" if status > 0 else "Sigma22 + t(Sigma12) %*% ZSig12"
    return _lib.NotPositiveDefinite(
        _lib.SGP_ENOTPD, f"chol(): the leading minor of order {abs(int(status))} of {which} is "
                         "not positive definite")


def norm_grad_ascent_vi_batch(cov_par_starts, cov_fun, xus, batch, muus=None, opt=None,
                              dcov_fun_dknot=None):
    """B norm_grad_ascent_vi runs in lockstep on one batch: every iteration is one
    batch.eval_vi call over the problems still running.  batch: a SparseGPBatch, or a list of
    (xy, y, mu) problems to build one from.  Returns a list of the dicts norm_grad_ascent_vi
    returns; a problem whose evaluation is not positive definite retires with that error under
    "error" (the R error the single fit raises) and u_mean = u_var = None."""
    if not (dcov_fun_dknot is None or dcov_fun_dknot is False or
            (isinstance(dcov_fun_dknot, float) and np.isnan(dcov_fun_dknot))):
        raise ValueError("norm_grad_ascent_vi_batch: knot gradients are not supported "
                         "(dcov_fun_dknot must be None)")
    o = _opts(opt)
    own = not hasattr(batch, "eval_vi")
    if own:
        batch = SparseGPBatch.from_problems(batch)
    try:
        return _lockstep(cov_par_starts, cov_fun, xus, batch, muus, o)
    finally:
        if own:
            batch.close()


def _lockstep(cov_par_starts, cov_fun, xus, batch, muus, o):
    B = batch.B
    if len(cov_par_starts) != B or len(xus) != B:
        raise ValueError(f"norm_grad_ascent_vi_batch: {B} problems, {len(cov_par_starts)} "
                         f"cov_par_starts, {len(xus)} knot sets")
    data = [batch.rows(b) for b in range(B)]
    d = data[0][0].shape[1]
    xus = [np.array(np.asarray(xus[b], dtype=np.float64).reshape(-1, d), copy=True)
           for b in range(B)]
    if muus is None:
        muus = [None] * B
    muus = [np.full(xus[b].shape[0], data[b][1].mean())                      # quirk Q14
            if muus[b] is None or (np.ndim(muus[b]) == 0 and not np.isfinite(muus[b]))
            else muus[b] for b in range(B)]
    names = [list(cp.keys()) for cp in cov_par_starts]
    cur = [np.array([float(cov_par_starts[b][k]) for k in names[b]]) for b in range(B)]
    log_t = [np.log(c) for c in cur]
    zeros = lambda b: np.zeros(len(names[b]))   # noqa: E731
    sg2, sd2, sc = ([zeros(b) for b in range(B)] for _ in range(3))
    tr_obj, tr_grad, tr_cov = ([[] for _ in range(B)] for _ in range(3))
    gt, obj, it = [None] * B, [None] * B, [1] * B
    error = [None] * B
    active = np.ones(B, dtype=np.uint8)
    adadelta = o["optim_method"] == "adadelta"

    def evaluate(first):
        pars = [OrderedDict(zip(names[b], cur[b])) for b in range(B)]
        ob, gr, st = batch.eval_vi(pars, cov_fun, xus, o["delta"], active=active)
        for b in range(B):
            if not active[b]:
                continue
            if st[b] != 0:
                error[b] = _not_pd(st[b])
                active[b] = 0
                continue
            gnew = np.array([gr[b][k] for k in names[b]], dtype=np.float64)
            if not first and adadelta:
                sc[b] = o["decay"] * sc[b] + (1 - o["decay"]) * np.abs(np.sign(gnew) -
                                                                      np.sign(gt[b])) / 2
            obj[b], gt[b] = float(ob[b]), gnew
            tr_obj[b].append(obj[b])
            tr_cov[b].append(cur[b].copy())
            tr_grad[b].append(gnew)
            log_t[b] = np.log(cur[b])

    evaluate(True)
    while True:
        for b in range(B):
            if not active[b]:
                continue
            k = it[b]
            if not (k < o["maxit"] and (
                    bool(np.any(np.abs(gt[b]) > o["grad_tol"])) or
                    (abs(obj[b] - tr_obj[b][k - 2]) > o["obj_tol"] if k > 1 else True))):
                active[b] = 0                       # retired: never evaluated again
                continue
            it[b] += 1
            if adadelta:
                sg2[b] = o["decay"] * sg2[b] + (1 - o["decay"]) * gt[b] ** 2
                step = ((1 / o["eta"]) ** sc[b]) * (np.sqrt(sd2[b] + o["epsilon"]) /
                                                    np.sqrt(sg2[b] + o["epsilon"])) * gt[b]
                sd2[b] = o["decay"] * sd2[b] + (1 - o["decay"]) * step ** 2
            else:
                step = o["learn_rate"] * gt[b]
            log_t[b] = log_t[b] + step
            cur[b] = np.exp(log_t[b])
        if not active.any():
            break
        evaluate(False)

    u_means, u_vars = [None] * B, [None] * B
    if any(e is None for e in error):
        u_means, u_vars = batch.posterior_u(muus)
    out = []
    for b in range(B):
        xy, _, mu = data[b]
        res = {"cov_par": OrderedDict(zip(names[b], cur[b])), "xu": xus[b], "iter": it[b],
               "obj_fun": np.array(tr_obj[b]), "grad": np.array(tr_grad[b]),
               "cov_par_history": np.array(tr_cov[b]), "knot_grad": 0, "knot_history": xus[b],
               "cov_fun": cov_fun, "xy": np.array(xy), "mu": np.array(mu), "muu": muus[b],
               "u_mean": None if error[b] else u_means[b],
               "u_var": None if error[b] else u_vars[b]}
        if error[b] is not None:
            res["error"] = error[b]
        out.append(res)
    return out


def _per_problem(B, cov_par_start, xu, muu, who, unit):
    """cov_par_start, xu and muu as B-lists: each is one value for all or a list with one per
    problem (a list of numbers is one knot set / one muu)."""
    per = lambda v, one: list(v) if isinstance(v, (list, tuple)) and not one(v) else [v] * B  # noqa: E731
    starts = per(cov_par_start, lambda v: False)
    is_arr = lambda v: len(v) > 0 and np.ndim(v[0]) == 0   # noqa: E731
    xus = [xu] * B if isinstance(xu, np.ndarray) else per(xu, is_arr)
    muus = [muu] * B if muu is None or isinstance(muu, np.ndarray) else per(muu, is_arr)
    if len(starts) != B or len(xus) != B or len(muus) != B:
        raise ValueError(f"{who}: cov_par_start, xu and muu must be one value or one "
                         f"per {unit}")
    return starts, xus, muus


def _knots_and_muu(xu, muu):
    """(m x d knots, muu): a muu that is None or not of m values is zeros."""
    u = np.asarray(xu, dtype=np.float64)
    u = u.reshape(-1, 1) if u.ndim == 1 else u
    if muu is None or np.size(muu) != u.shape[0]:
        muu = np.zeros(u.shape[0])
    return u, np.asarray(muu, dtype=np.float64).reshape(-1)


def optimize_gp_batch(problems, cov_fun, cov_par_start, xu, muu=None, opt=None):
    """optimize_gp(y, xy, cov_fun, cov_par_start, mu, family = "gaussian", sparse = TRUE,
    xu_opt = "fixed", xu, muu, vi = TRUE, opt) for each (xy, y, mu) of `problems`, fitted in
    lockstep on one batch.  cov_par_start, xu and muu: one value for all problems or a list with
    one per problem.  Returns a list of optimize_gp's {"results", "sparse", "family", "delta",
    "xu_init"} dicts (or its error strings), which predict_gp, predictor_gp and score_gp take."""
    from .optimize import ERR_COV, ERR_GA, ERR_MAXKNOT, OPT_MASTER
    B = len(problems)
    o = {k: (dict(v) if isinstance(v, dict) else v) for k, v in OPT_MASTER.items()}
    for k, v in (opt or {}).items():
        if k in o:
            o[k] = dict(v) if isinstance(v, dict) else v
    if o["optim_method"] == "ga":
        return [ERR_GA] * B
    if cov_fun not in ("sqexp", "ard"):
        return [ERR_COV] * B
    starts, xus, muus = _per_problem(B, cov_par_start, xu, muu, "optimize_gp_batch", "problem")
    out, keep = [None] * B, []
    for b, prob in enumerate(problems):
        n = np.asarray(prob[1]).size
        if o["maxknot"] >= n:
            out[b] = ERR_MAXKNOT
            continue
        xy = _mat(prob[0], n)
        u, mb = _knots_and_muu(xus[b], muus[b])
        keep.append((b, (xy, prob[1], prob[2] if len(prob) > 2 else None), u, mb))
    if keep:
        res = norm_grad_ascent_vi_batch([starts[b] for b, *_ in keep], cov_fun,
                                        [u for _, _, u, _ in keep], [p for _, p, _, _ in keep],
                                        [mb for *_, mb in keep], o)
        for (b, _, u, _), r in zip(keep, res):
            out[b] = {"results": r, "sparse": True, "family": "gaussian", "delta": o["delta"],
                      "xu_init": u}
    return out


def cross_validate_gp(y, xy, cov_fun, cov_par_start, xu, folds=5, mu=None, muu=None, opt=None,
                      rng=None):
    """k-fold cross-validation of optimize_gp(family = "gaussian", sparse = TRUE, vi = TRUE,
    xu_opt = "fixed"): every fold's fit runs in lockstep on one batch and every fold's held-out
    rows are scored on it (SparseGPBatch.score), without the posteriors leaving the device.

    folds: an integer (a random partition from rng, default np.random.default_rng(0)) or an
    integer array of fold ids, one per row.  Fold f trains on the rows of every other fold and
    holds its own out.  mu = None takes each fold's training mean(y) for its training rows and
    its held-out rows; an array mu is split by rows.  cov_par_start, xu and muu: one value for
    all folds or a list with one per fold.  The refusals are optimize_gp_batch's and come back as
    its error string.

    Returns {"folds": [{"model": an optimize_gp-shaped dict (predict_gp / score_gp take it),
    "score": score_gp's dict for the held-out rows, or the fit's error, "test_rows": indices}],
    "mean_nlp", "median_nlp" (over all held-out rows' finite nlp), "rmse" (over all held-out
    rows), "fold_id"}; the pooled figures cover the folds that were scored."""
    from .optimize import ERR_COV, ERR_GA, ERR_MAXKNOT, OPT_MASTER
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n = y.size
    xy = _mat(xy, n)
    o = {k: (dict(v) if isinstance(v, dict) else v) for k, v in OPT_MASTER.items()}
    for k, v in (opt or {}).items():
        if k in o:
            o[k] = dict(v) if isinstance(v, dict) else v
    if o["optim_method"] == "ga":
        return ERR_GA
    if cov_fun not in ("sqexp", "ard"):
        return ERR_COV
    if np.ndim(folds) == 0:
        k = int(folds)
        if not 2 <= k <= n:
            raise ValueError(f"cross_validate_gp: folds={k} outside [2, {n}]")
        g = np.random.default_rng(0) if rng is None else rng
        fold_id = np.empty(n, dtype=np.int64)
        fold_id[g.permutation(n)] = np.arange(n) % k
    else:
        fold_id = np.asarray(folds, dtype=np.int64).reshape(-1)
        if fold_id.size != n:
            raise ValueError(f"cross_validate_gp: {fold_id.size} fold ids for {n} rows")
    ids = np.unique(fold_id)
    B = ids.size
    if B < 2:
        raise ValueError("cross_validate_gp: fewer than two folds")
    test_rows = [np.flatnonzero(fold_id == f) for f in ids]
    train_rows = [np.flatnonzero(fold_id != f) for f in ids]
    if any(o["maxknot"] >= tr.size for tr in train_rows):
        return ERR_MAXKNOT
    starts, xus, muus = _per_problem(B, cov_par_start, xu, muu, "cross_validate_gp", "fold")
    mu_all = None if mu is None else np.broadcast_to(np.asarray(mu, dtype=np.float64), (n,))
    problems, tests, us, mbs = [], [], [], []
    for b in range(B):
        tr, te = train_rows[b], test_rows[b]
        mu_tr = np.full(tr.size, y[tr].mean()) if mu_all is None else mu_all[tr]
        mu_te = np.full(te.size, y[tr].mean()) if mu_all is None else mu_all[te]
        problems.append((xy[tr], y[tr], mu_tr))
        tests.append((xy[te], y[te], mu_te))
        u, mb = _knots_and_muu(xus[b], muus[b])
        us.append(u)
        mbs.append(mb)
    batch = SparseGPBatch.from_problems(problems)
    try:
        res = norm_grad_ascent_vi_batch(starts, cov_fun, us, batch, mbs, o)
        ok = np.array(["error" not in r for r in res], dtype=np.uint8)
        scores = [None] * B
        if ok.any():
            batch.set_test_problems(tests)
            scores = batch.score(ok)
    finally:
        batch.close()
    out, nlps, errs = [], [], []
    for b in range(B):
        model = {"results": res[b], "sparse": True, "family": "gaussian", "delta": o["delta"],
                 "xu_init": us[b]}
        out.append({"model": model, "score": scores[b] if ok[b] else res[b]["error"],
                    "test_rows": test_rows[b]})
        if ok[b]:
            nlps.append(scores[b]["nlp"])
            errs.append(scores[b]["pred"]["pred_mean"].reshape(-1) - tests[b][1])
    nlp = np.concatenate(nlps) if nlps else np.zeros(0)
    err = np.concatenate(errs) if errs else np.zeros(0)
    fin = nlp[np.isfinite(nlp)]
    return {"folds": out,
            "mean_nlp": float(fin.mean()) if fin.size else float("nan"),
            "median_nlp": float(np.median(fin)) if fin.size else float("nan"),
            "rmse": float(np.sqrt(np.mean(err ** 2))) if err.size else float("nan"),
            "fold_id": fold_id}
