"""Batched small-knot VI fits: many independent problems per launch.

  SparseGPBatch                B problems (row ranges of one resident X / y / mu), each with its own
                               theta and at most 64 knots: sgp_batch_* of include/sgp.h
  norm_grad_ascent_vi_batch    B norm_grad_ascent_vi runs (R/vi_functions.R:606-1218) in lockstep,
                               one batch evaluation per iteration
  optimize_gp_batch            optimize_gp(family = "gaussian", sparse = TRUE, vi = TRUE,
                               xu_opt = "fixed") for a list of problems

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
    per = lambda v, one: list(v) if isinstance(v, (list, tuple)) and not one(v) else [v] * B  # noqa: E731
    starts = per(cov_par_start, lambda v: False)
    is_arr = lambda v: len(v) > 0 and np.ndim(v[0]) == 0   # noqa: E731
    xus = [xu] * B if isinstance(xu, np.ndarray) else per(xu, is_arr)
    muus = [muu] * B if muu is None or isinstance(muu, np.ndarray) else per(muu, is_arr)
    if len(starts) != B or len(xus) != B or len(muus) != B:
        raise ValueError("optimize_gp_batch: cov_par_start, xu and muu must be one value or one "
                         "per problem")
    out, keep = [None] * B, []
    for b, prob in enumerate(problems):
        n = np.asarray(prob[1]).size
        if o["maxknot"] >= n:
            out[b] = ERR_MAXKNOT
            continue
        xy = _mat(prob[0], n)
        u = np.asarray(xus[b], dtype=np.float64)
        u = u.reshape(-1, 1) if u.ndim == 1 else u
        mb = muus[b]
        if mb is None or np.size(mb) != u.shape[0]:
            mb = np.zeros(u.shape[0])
        keep.append((b, (xy, prob[1], prob[2] if len(prob) > 2 else None), u,
                     np.asarray(mb, dtype=np.float64).reshape(-1)))
    if keep:
        res = norm_grad_ascent_vi_batch([starts[b] for b, *_ in keep], cov_fun,
                                        [u for _, _, u, _ in keep], [p for _, p, _, _ in keep],
                                        [mb for *_, mb in keep], o)
        for (b, _, u, _), r in zip(keep, res):
            out[b] = {"results": r, "sparse": True, "family": "gaussian", "delta": o["delta"],
                      "xu_init": u}
    return out
