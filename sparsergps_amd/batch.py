"""Batched small-knot VI and FITC fits: many independent problems per launch (DESIGN.md sec. 0n,
0q).

  SparseGPBatch                B problems (row ranges of one resident X / y / mu), each with its own
                               theta and at most 64 knots: sgp_batch_* of include/sgp.h
  norm_grad_ascent_vi_batch    B norm_grad_ascent_vi runs (R/vi_functions.R:606-1218) in lockstep,
                               one batch evaluation per iteration
  optimize_gp_batch            optimize_gp(family = "gaussian", sparse = TRUE, vi = TRUE,
                               xu_opt = "fixed") for a list of problems
  SparseGPBatch.eval_vi_knots  the evaluation with every problem's knot gradient (delbo_dcov_par's
                               knot branch, R/vi_functions.R:425-593), which
                               xu_opt = "simultaneous" of the three functions above ascends on
  SparseGPBatch.set_test / predict / score
                               predict_vi (R/vi_functions.R:1222-1336) and score_gp's figures for
                               every problem's held-out rows, from the posteriors the batch holds
                               on the device
  cross_validate_gp            k-fold cross-validation: the folds fitted in lockstep and scored on
                               one batch
  SparseGPBatch.eval_fitc      the other Gaussian objective (obj_fun_norm / dlogp_dcov_par;
                               DESIGN.md sec. 0q), which norm_grad_ascent_batch ascends on and
                               vi = False of optimize_gp_batch / cross_validate_gp fits; predict and
                               score then give predict_laplace(family = "gaussian")

  SparseGPBatch.lap_init / set_f / get_f / eval_laplace
                               Poisson and Bernoulli problems (newtrap_sparseGP and dlogq_dcov_par per
                               problem), which laplace_grad_ascent_batch ascends
                               on and family = "poisson" / "bernoulli" of optimize_gp_batch /
                               cross_validate_gp fit; predict and score then give
                               predict_laplace(family != "gaussian") and that family's my_nlp

Per problem the semantics are the single fit's (drivers._ascent, the knots fixed or moved with
theta: optimize_gp's xu_opt = "fixed" / "simultaneous", R/optimize_gp.R:299-333, 378-412); a problem
that meets its stop rule is retired through the evaluation's `active` mask while the others go
on.  The path is opt-in: nothing else in the package routes to it.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import numpy as np

from . import _lib
from .covariance import theta_vector
from .drivers import _opts, _unbounded
from .vi import knot_bounds, param_names

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
        self._kind = [None] * self.B       # and whether it was a Gaussian or a Laplace one
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
        self._kind = [None] * self.B

    # ------------------------------------------------------------------ evaluation
    def eval_raw(self, cov_fun, theta, xus, delta, flags, active, obj, grad, status):
        """sgp_batch_eval_vi on caller-owned arrays: theta (B x P, row b = problem b), xus a list
        of m_b x d knot arrays (entries of inactive problems may be None), active a uint8 array
        or None, obj (B), grad (B x P, or None with SGP_FLAG_OBJ_ONLY), status (B, int32).
        Slots of inactive problems are left as they are."""
        self._eval(cov_fun, theta, xus, delta, flags, active, obj, grad, status)

    def _eval(self, cov_fun, theta, xus, delta, flags, active, obj, grad, status, knots=False,
              bounds=None, fitc=False, laplace=None):
        """sgp_batch_eval_vi, with knots sgp_batch_eval_vi_knots (bounds: B x 2d or None), with
        fitc sgp_batch_eval_fitc, with laplace = (tol, maxit, nr_iters) sgp_batch_eval_laplace;
        returns (grad_knot packed like U, uoff, m) with knots."""
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
        args = (self._h, _lib.KERNELS.get(cov_fun, -1), _lib.dptr(theta), theta.shape[1],
                _lib.dptr(U), i64(uoff), i64(m), float(delta), int(flags),
                None if act is None else act.ctypes.data_as(_lib.c_ubyte_p), _lib.dptr(obj),
                None if grad is None else _lib.dptr(grad), 0 if grad is None else grad.shape[1],
                status.ctypes.data_as(_lib.c_int_p))
        gk = None
        if knots:
            gk = np.full(U.size, np.nan)
            bd = None if bounds is None else np.ascontiguousarray(bounds, dtype=np.float64)
            st = self._lib.sgp_batch_eval_vi_knots(*args, None if bd is None else _lib.dptr(bd),
                                                   _lib.dptr(gk))
        elif laplace is not None:
            st = self._lib.sgp_batch_eval_laplace(*args, laplace[0], laplace[1],
                                                  laplace[2].ctypes.data_as(_lib.c_int_p))
        elif fitc:
            st = self._lib.sgp_batch_eval_fitc(*args)
        else:
            st = self._lib.sgp_batch_eval_vi(*args)
        _lib.check(st)
        for b in range(self.B):
            if on[b] and status[b] == 0 and not (fitc and np.isnan(obj[b])):
                self._state[b] = int(m[b])
                self._kind[b] = "laplace" if laplace is not None else "gaussian"
        return gk, uoff, m

    def eval_vi(self, cov_pars, cov_fun, xus, delta=1e-6, active=None, obj_only=False,
                r_det=False):
        """One evaluation of the batch.  cov_pars: B dicts, xus: B knot arrays (entries of
        inactive problems are not read).  Returns (obj[B], grad, status[B]): grad a list of
        OrderedDicts in each cov_par's key order (None for inactive problems and with
        obj_only); a problem with status != 0 has NaN obj and grad (chol()'s leading-minor order:
        > 0 for Sigma22, < 0 for Sigma22 + t(Sigma12) %*% ZSig12).  Inactive slots are NaN / 0."""
        return self._eval_pars(self.eval_raw, cov_pars, cov_fun, xus, delta, active, obj_only,
                               r_det)

    def _eval_pars(self, run, cov_pars, cov_fun, xus, delta, active, obj_only, r_det):
        """eval_vi / eval_fitc on run = eval_raw / eval_fitc_raw."""
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
        run(cov_fun, theta, xus, delta, flags, active, obj, g, status)
        return obj, self._named(cov_pars, cov_fun, g, on), status

    def eval_fitc_raw(self, cov_fun, theta, xus, delta, flags, active, obj, grad, status):
        """sgp_batch_eval_fitc on caller-owned arrays, as eval_raw."""
        self._eval(cov_fun, theta, xus, delta, flags, active, obj, grad, status, fitc=True)

    def eval_fitc(self, cov_pars, cov_fun, xus, delta=1e-6, active=None, obj_only=False,
                  r_det=False):
        """One FITC evaluation of the batch (sgp_batch_eval_fitc: obj_fun_norm and
        dlogp_dcov_par per problem, as SparseGPContext.eval_fitc gives them for one).  The
        arguments and the return value are eval_vi's: (obj[B], grad, status[B]); status < 0 names
        Sigma22 + t(Sigma12) %*% ZSig12.  posterior_u, predict and score afterwards are
        laplace_gradient_ascent.R:1635-1655 and predict_laplace(family = "gaussian") for the
        problems this call evaluated."""
        return self._eval_pars(self.eval_fitc_raw, cov_pars, cov_fun, xus, delta, active,
                               obj_only, r_det)

    def fitc_stage_ms(self, enable=True):
        """HIP-event times (ms) of the last eval_fitc's five stages (K22's stage, the weighted
        pass 1, Bm's stage, the gradient pass, the G22 stage); records from the next one on."""
        self._need()
        out = np.zeros(5)
        _lib.check(self._lib.sgp_diag_batch_fitc_timing(self._h, int(bool(enable)),
                                                        _lib.dptr(out)))
        return out

    # ------------------------------------------------------------------ Laplace (sec. 0s)
    def lap_init(self, family, expo=None):
        """sgp_batch_lap_init: family "poisson" or "bernoulli"; expo: n positive values (the
        reference's m, read by Poisson only), a scalar, or None for 1 on every row.  Allocates
        what eval_laplace needs and sets every problem's latent f to 0; may be repeated."""
        self._need()
        if family not in _lib.FAMILIES:
            raise ValueError(f"family must be one of {sorted(_lib.FAMILIES)}, not {family!r}")
        ex = None if expo is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(expo, dtype=np.float64), (self.n,)))
        _lib.check(self._lib.sgp_batch_lap_init(self._h, _lib.FAMILIES[family],
                                                None if ex is None else _lib.dptr(ex)))
        self.family, self.expo = family, ex
        self._foff = np.concatenate([[0], np.cumsum(self.nrow)]).astype(np.int64)

    def _need_lap(self):
        self._need()
        if getattr(self, "family", None) is None:
            raise RuntimeError("SparseGPBatch: call lap_init first")

    def set_f(self, f=None, fill=None):
        """The problems' latent vectors (sgp_batch_lap_set_f): f a list of B arrays (n_b values
        each) or one packed array of sum n_b values; or fill, one value per problem (the
        reference starts Poisson at log(mean y) - log(expo) and Bernoulli at 0)."""
        self._need_lap()
        if (f is None) == (fill is None):
            raise ValueError("set_f: give f or fill")
        if f is not None:
            if isinstance(f, (list, tuple)):
                f = np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in f])
            v = np.ascontiguousarray(np.asarray(f, dtype=np.float64).reshape(-1))
            if v.size != self._foff[-1]:
                raise ValueError(f"set_f: {v.size} values for {self._foff[-1]} rows")
            _lib.check(self._lib.sgp_batch_lap_set_f(self._h, _lib.dptr(v), None))
        else:
            v = np.ascontiguousarray(np.broadcast_to(np.asarray(fill, dtype=np.float64),
                                                     (self.B,)))
            _lib.check(self._lib.sgp_batch_lap_set_f(self._h, None, _lib.dptr(v)))

    def get_f(self):
        """The problems' latent vectors, a list of B arrays (after eval_laplace: the modes)."""
        self._need_lap()
        v = np.zeros(int(self._foff[-1]) + 1)
        _lib.check(self._lib.sgp_batch_lap_get_f(self._h, _lib.dptr(v)))
        return [v[self._foff[b]:self._foff[b + 1]].copy() for b in range(self.B)]

    def eval_laplace_raw(self, cov_fun, theta, xus, delta, flags, active, obj, grad, status, tol,
                         maxit, nr_iters):
        """sgp_batch_eval_laplace on caller-owned arrays, as eval_raw, with nr_iters (B, int32)."""
        self._need_lap()
        self._eval(cov_fun, theta, xus, delta, flags, active, obj, grad, status,
                   laplace=(float(tol), int(maxit), nr_iters))

    def eval_laplace(self, cov_pars, cov_fun, xus, delta=1e-6, active=None, obj_only=False,
                     tol=1e-6, maxit=1000):
        """One Laplace evaluation of the batch (sgp_batch_eval_laplace): per problem
        newtrap_sparseGP warm-started from its resident f, then dlogq_dcov_par at the mode, as
        SparseGPContext.eval_laplace gives them for one.  Returns what eval_vi returns plus
        nr_iters: (obj[B], grad, status[B], nr_iters[B]); obj is the last NR objective; status < 0
        names Sigma22 + t(Sigma12) %*% ZSig12 or the B-weighted one.  The resident f is left at the
        mode (unspecified for a problem with status != 0 until set_f).  posterior_u, predict and
        score afterwards are laplace_posterior_u and predict_laplace(family != "gaussian")."""
        nr = np.zeros(self.B, dtype=np.int32)

        def run(cov_fun, theta, xus, delta, flags, active, obj, g, status):
            self.eval_laplace_raw(cov_fun, theta, xus, delta, flags, active, obj, g, status, tol,
                                  maxit, nr)
        obj, grads, status = self._eval_pars(run, cov_pars, cov_fun, xus, delta, active, obj_only,
                                             False)
        return obj, grads, status, nr

    def lap_objective_values(self, b):
        """newtrap_sparseGP's objective_function_values of problem b in the last eval_laplace
        that evaluated it (the first 256 of them)."""
        self._need_lap()
        out, cnt = np.zeros(_lib.SGP_BATCH_LAP_NOBJ), C.c_int(0)
        _lib.check(self._lib.sgp_diag_batch_lap_objective_values(
            self._h, int(b), _lib.dptr(out), out.size, C.byref(cnt)))
        return out[:min(cnt.value, out.size)].copy()

    def laplace_stage_ms(self, enable=True):
        """HIP-event times (ms) of the last eval_laplace's eleven stages (K22, the Z pass, the
        K22 + S_Z stage | summed over the Newton iterations: the objective pass, the C stage, NR's
        part a, x2 | the gradient's part a, its vector stage, part b, the G22 stage); records
        from the next one on."""
        self._need()
        out = np.zeros(11)
        _lib.check(self._lib.sgp_diag_batch_laplace_timing(self._h, int(bool(enable)),
                                                           _lib.dptr(out)))
        return out

    def _named(self, cov_pars, cov_fun, g, on):
        names = param_names(cov_fun, self.d)
        grads = []
        for b in range(self.B):
            if g is None or not on[b]:
                grads.append(None)
                continue
            byname = dict(zip(names, g[b]))
            grads.append(OrderedDict((k, float(byname[k])) for k in cov_pars[b].keys()))
        return grads

    def knot_bounds(self):
        """knot_bounds (vi_functions.R:175-178) of each problem's own rows: B arrays of d x 2.
        Computed once; set_data replaces y and mu only, so it does not invalidate them."""
        if getattr(self, "_kb", None) is None:
            self._kb = [knot_bounds(self.rows(b)[0]) for b in range(self.B)]
        return self._kb

    def eval_vi_knots(self, cov_pars, cov_fun, xus, delta=1e-6, active=None, bounds="data",
                      r_det=False):
        """eval_vi with every active problem's knot gradient (sgp_batch_eval_vi_knots).  Returns
        (obj, grads, knot_grads, status): obj, grads and status are eval_vi's, bit for bit;
        knot_grads[b] is the (m_b d,) knot-major vector (entry k d + c: knot k, coordinate c) of
        dsqexp_dx2 / dsqexp_dx2_ard following cov_fun, None for an inactive problem and NaN for
        one that is not positive definite.  bounds: "data" for knot_bounds of each problem's own
        rows (the drivers' choice), None for the plain dELBO/du, or a list of B d x 2 arrays
        (entries of inactive problems may be None)."""
        P = (self.d if cov_fun == "ard" else 1) + 2
        theta = np.ones((self.B, P))
        on = [active is None or bool(active[b]) for b in range(self.B)]
        for b in range(self.B):
            if on[b]:
                theta[b] = theta_vector(cov_pars[b], cov_fun, self.d)
        if isinstance(bounds, str):
            if bounds != "data":
                raise ValueError(f'eval_vi_knots: bounds must be "data", None or a list, not '
                                 f"{bounds!r}")
            bounds = self.knot_bounds()
        bd = None
        if bounds is not None:
            if len(bounds) != self.B:
                raise ValueError(f"eval_vi_knots: {len(bounds)} bounds for {self.B} problems")
            bd = np.zeros((self.B, 2 * self.d))
            for b in range(self.B):
                if on[b]:
                    bb = np.asarray(bounds[b], dtype=np.float64)
                    if bb.shape != (self.d, 2):
                        raise ValueError(f"problem {b}: bounds are not {self.d} x 2")
                    bd[b] = bb.reshape(-1, order="F")
        obj = np.full(self.B, np.nan)
        g = np.full((self.B, P), np.nan)
        status = np.zeros(self.B, dtype=np.int32)
        flags = _lib.SGP_FLAG_R_DET if r_det else 0
        gk, uoff, m = self._eval(cov_fun, theta, xus, delta, flags, active, obj, g, status,
                                 knots=True, bounds=bd)
        kg = [gk[uoff[b]:uoff[b] + m[b] * self.d].copy() if on[b] else None
              for b in range(self.B)]
        return obj, self._named(cov_pars, cov_fun, g, on), kg, status

    def knot_stage_ms(self, enable=True):
        """HIP-event times (ms) of the last eval_vi_knots' knot pass and knot finish; records from
        the next one on (stage_ms covers its first four stages)."""
        self._need()
        out = np.zeros(2)
        _lib.check(self._lib.sgp_diag_batch_knot_timing(self._h, int(bool(enable)),
                                                        _lib.dptr(out)))
        return out

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
        """predict_vi (predict_laplace(family = "gaussian") where that evaluation was eval_fitc)
        for every active problem on its test rows, from the posterior of its last successful
        evaluation: a list of {"pred_mean": (n_b, 1), "pred_var": (n_b,)}, None for
        inactive problems."""
        (_, nr, off, _), pm, pv, _, _ = self._run_predict(active, False)
        return [None if active is not None and not active[b] else
                {"pred_mean": pm[off[b]:off[b] + nr[b]].reshape(-1, 1).copy(),
                 "pred_var": pv[off[b]:off[b] + nr[b]].copy()} for b in range(self.B)]

    def score(self, active=None, par=None):
        """score_gp(vi = True) (vi = False after eval_fitc) for every active problem on its test
        rows: a list of {"pred",
        "nlp", "median_nlp", "mean_nlp", "rmse", "srmse", "n_nan"} dicts (None for inactive
        problems), the nlp with each problem's own tau.  Where the active problems' posteriors are
        Laplace ones (eval_laplace) the dicts are score_gp's for that family: predict, then one
        call of the quadrature (my_nlp's, sgp_nlp) over the packed rows.  par: one entry per
        problem as score_gp's par ({"m": ...} for Poisson; None: m = 1), read by Laplace problems
        only."""
        self._need()
        test = getattr(self, "_test", None)
        if test is not None and test[3] is None:
            raise ValueError("SparseGPBatch.score: set_test was given no y_test")
        on = [active is None or bool(active[b]) for b in range(self.B)]
        kinds = {self._kind[b] for b in range(self.B) if on[b]}
        if "laplace" in kinds:
            if kinds != {"laplace"}:
                raise ValueError("SparseGPBatch.score: the active problems mix Gaussian and "
                                 "Laplace posteriors; score them in two calls")
            return self._score_laplace(active, on, par)
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

    def _score_laplace(self, active, on, par):
        from .evaluation import _nlp, _score_par
        (r0, nr, off, yt), pm, pv, _, _ = self._run_predict(active, False)
        if par is not None and len(par) != self.B:
            raise ValueError(f"SparseGPBatch.score: {len(par)} par entries for {self.B} problems")
        idx = [b for b in range(self.B) if on[b] and nr[b] > 0]
        ys, expo = [], []
        for b in idx:
            n = int(nr[b])
            ys.append(yt[r0[b]:r0[b] + n])
            p, ex = _score_par(self.family, None if par is None else par[b])
            expo.append(np.full(n, p) if ex is None else ex)
            if expo[-1].size != n:
                raise ValueError(f"problem {b}: par['m'] has {expo[-1].size} values for {n} rows")
        nlp_all = np.zeros(0)
        if idx:
            rows = np.concatenate([np.arange(off[b], off[b] + nr[b]) for b in idx])
            nlp_all, _ = _nlp(self.family, np.concatenate(ys), pm[rows], pv[rows], 1.0,
                              np.concatenate(expo) if self.family == "poisson" else None)
        out, at = [], 0
        for b in range(self.B):
            if not on[b]:
                out.append(None)
                continue
            n, o = int(nr[b]), int(off[b])
            v = nlp_all[at:at + n].copy()
            at += n
            y = yt[r0[b]:r0[b] + n]
            mean = pm[o:o + n]
            fin = v[np.isfinite(v)]
            rmse = float(np.sqrt(np.sum((mean - y) ** 2) / n)) if n else float("nan")
            sd = float(np.std(y, ddof=1)) if n > 1 else float("nan")
            out.append({"pred": {"pred_mean": mean.reshape(-1, 1).copy(),
                                 "pred_var": pv[o:o + n].copy()},
                        "nlp": v,
                        "median_nlp": float(np.median(fin)) if fin.size else float("nan"),
                        "mean_nlp": float(fin.mean()) if fin.size else float("nan"),
                        "rmse": rmse, "srmse": rmse / sd, "n_nan": int(np.sum(np.isnan(v)))})
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


def _xu_opt(xu_opt, who):
    """True for "simultaneous", False for "fixed"; optimize_gp's refusals otherwise."""
    if xu_opt == "fixed":
        return False
    if xu_opt in ("oat", "random"):
        raise ValueError(f'{who}: batches do not support xu_opt = "{xu_opt}" (the knot search '
                         'adds and removes knots problem by problem); use optimize_gp')
    if xu_opt != "simultaneous":
        raise ValueError(f'{who}: xu_opt must be "fixed" or "simultaneous", not {xu_opt!r}')
    return True


def norm_grad_ascent_vi_batch(cov_par_starts, cov_fun, xus, batch, muus=None, opt=None,
                              dcov_fun_dknot=None, xu_opt="fixed", knot_opt=None):
    """B norm_grad_ascent_vi runs in lockstep on one batch: every iteration is one
    batch.eval_vi call over the problems still running (one batch.eval_vi_knots call with
    xu_opt = "simultaneous").  batch: a SparseGPBatch, or a list of (xy, y, mu) problems to build
    one from.  Returns a list of the dicts norm_grad_ascent_vi returns; a problem whose evaluation
    is not positive definite retires with that error under "error" (the R error the single fit
    raises) and u_mean = u_var = None.

    xu_opt = "simultaneous" moves every problem's knots with its theta as drivers._ascent does
    (the knot derivative kind follows cov_fun, the bounded transform is on knot_bounds of the
    problem's own rows); knot_opt: the 1-based knots that move, one list for all problems or one
    per problem (None: all), the others' gradient being zero."""
    if not (dcov_fun_dknot is None or dcov_fun_dknot is False or
            (isinstance(dcov_fun_dknot, float) and np.isnan(dcov_fun_dknot))):
        raise ValueError("norm_grad_ascent_vi_batch: knot gradients are not supported through "
                         'dcov_fun_dknot (it must be None); pass xu_opt = "simultaneous"')
    simul = _xu_opt(xu_opt, "norm_grad_ascent_vi_batch")
    o = _opts(opt)
    own = not hasattr(batch, "eval_vi")
    if own:
        batch = SparseGPBatch.from_problems(batch)
    try:
        return _lockstep(cov_par_starts, cov_fun, xus, batch, muus, o, simul, knot_opt)
    finally:
        if own:
            batch.close()


_ERR_FITC_KNOTS = ('xu_opt = "simultaneous" with vi = False: FITC batches have no knot gradient '
                   'yet; use xu_opt = "fixed", vi = True, or optimize_gp')


def norm_grad_ascent_batch(cov_par_starts, cov_fun, xus, batch, muus=None, opt=None,
                           dcov_fun_dknot=None, xu_opt="fixed", knot_opt=None):
    """B norm_grad_ascent runs (R/laplace_gradient_ascent.R:1111-1693, the FITC objective) in
    lockstep on one batch: every iteration is one batch.eval_fitc call over the problems still
    running.  The arguments and the return value are norm_grad_ascent_vi_batch's, the dicts being
    those norm_grad_ascent returns (u_mean / u_var from laplace_gradient_ascent.R:1635-1655);
    status < 0 of a problem that is not positive definite names
    Sigma22 + t(Sigma12) %*% ZSig12.  xu_opt = "simultaneous" is refused: FITC batches have no
    knot gradient yet."""
    if not (dcov_fun_dknot is None or dcov_fun_dknot is False or
            (isinstance(dcov_fun_dknot, float) and np.isnan(dcov_fun_dknot))):
        raise ValueError("norm_grad_ascent_batch: knot gradients are not supported "
                         "(dcov_fun_dknot must be None)")
    if _xu_opt(xu_opt, "norm_grad_ascent_batch"):
        raise ValueError("norm_grad_ascent_batch: " + _ERR_FITC_KNOTS)
    o = _opts(opt)
    own = not hasattr(batch, "eval_fitc")
    if own:
        batch = SparseGPBatch.from_problems(batch)
    try:
        return _lockstep(cov_par_starts, cov_fun, xus, batch, muus, o, objective="fitc")
    finally:
        if own:
            batch.close()


_ERR_LAP_KNOTS = ('Laplace batches have no knot gradient: xu_opt must be "fixed" '
                  '(use laplace_grad_ascent or optimize_gp to move knots)')


def laplace_grad_ascent_batch(cov_par_starts, cov_fun, xus, batch, muus=None, opt=None,
                              dcov_fun_dknot=None, xu_opt="fixed", knot_opt=None,
                              family="poisson", expo=None, ff=None):
    """B laplace_grad_ascent runs (R/laplace_gradient_ascent.R:10-623, Poisson or Bernoulli) in
    lockstep on one batch: every iteration is one batch.eval_laplace call over the problems still
    running, each problem's Newton iteration warm-started from its previous mode on the device.
    The arguments are norm_grad_ascent_batch's, then family ("poisson" / "bernoulli"), expo (the
    exposure of the batch's rows, as SparseGPBatch.lap_init takes it; for a list of problems one
    entry per problem) and ff, the per-problem starts of the latent f (a list of B arrays or
    scalars; None: 0); opt's tol_nr / maxit_nr (1e-6 / 1000) bound the Newton iteration.  Returns
    a list of the dicts laplace_grad_ascent returns ("fmax", "u_mean", "u_var", "nr_iter", ...).
    xu_opt other than "fixed" is refused: Laplace batches have no knot gradient."""
    if family not in _lib.FAMILIES:
        raise ValueError(f"family must be one of {sorted(_lib.FAMILIES)}, not {family!r}")
    if not (dcov_fun_dknot is None or dcov_fun_dknot is False or
            (isinstance(dcov_fun_dknot, float) and np.isnan(dcov_fun_dknot))):
        raise ValueError("laplace_grad_ascent_batch: knot gradients are not supported "
                         "(dcov_fun_dknot must be None)")
    if xu_opt != "fixed":
        raise ValueError("laplace_grad_ascent_batch: " + _ERR_LAP_KNOTS)
    o = _opts(opt, {"maxit_nr": 1000, "tol_nr": 1e-6})
    own = not hasattr(batch, "eval_laplace")
    if own:
        if expo is not None and isinstance(expo, (list, tuple)):
            expo = np.concatenate([np.broadcast_to(np.asarray(e, dtype=np.float64),
                                                   (np.asarray(p[1]).size,))
                                   for e, p in zip(expo, batch)])
        batch = SparseGPBatch.from_problems(batch)
    try:
        if own or getattr(batch, "family", None) != family or expo is not None:
            batch.lap_init(family, expo)
        if ff is not None:
            batch.set_f([np.broadcast_to(np.asarray(ff[b], dtype=np.float64),
                                         (int(batch.nrow[b]),)) for b in range(batch.B)])
        return _lockstep(cov_par_starts, cov_fun, xus, batch, muus, o, objective="laplace")
    finally:
        if own:
            batch.close()


def _bounded(t, bounds):
    """drivers._bounded in the reference's order of operations, a product with the reciprocal
    (trans_fun, covariance_function_derivatives.R:191-197): a last-bit difference in a knot shows
    at 1e-11 in the knot gradient's small entries.  t: d values or m x d."""
    return bounds[:, 1] * (1 / (1 + np.exp(-t))) + bounds[:, 0] * (1 / (1 + np.exp(t)))


def _knot_keep(knot_opt, B, ms, d):
    """Per problem the 0 / 1 factor of its knot-major gradient, or None where every knot moves."""
    if knot_opt is None:
        return [None] * B
    ko = list(knot_opt)
    nested = any(k is None or np.ndim(k) > 0 for k in ko)   # one list per problem
    per = ko if nested else [ko] * B
    if len(per) != B:
        raise ValueError(f"norm_grad_ascent_vi_batch: {len(per)} knot_opt lists for {B} problems")
    out = []
    for b in range(B):
        if per[b] is None:
            out.append(None)
            continue
        keep = np.zeros(ms[b], dtype=bool)
        keep[np.asarray(list(per[b]), dtype=int) - 1] = True
        out.append(np.repeat(keep, d).astype(np.float64))
    return out


def _lockstep(cov_par_starts, cov_fun, xus, batch, muus, o, simul=False, knot_opt=None,
              objective="vi"):
    """objective: "vi" (batch.eval_vi / eval_vi_knots), "fitc" (batch.eval_fitc, knots fixed) or
    "laplace" (batch.eval_laplace with o's tol_nr / maxit_nr, knots fixed)."""
    if objective not in ("vi", "fitc", "laplace"):
        raise ValueError(f'_lockstep: objective must be "vi", "fitc" or "laplace", not '
                         f'{objective!r}')
    if simul and objective == "fitc":
        raise ValueError(_ERR_FITC_KNOTS)
    if simul and objective == "laplace":
        raise ValueError(_ERR_LAP_KNOTS)
    nr_iter = [[] for _ in range(batch.B)]
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
    # the knot state of drivers._ascent, per problem
    gk = [np.zeros(0)] * B
    if simul:
        bounds = [knot_bounds(data[b][0]) for b in range(B)]
        keep = _knot_keep(knot_opt, B, [u.shape[0] for u in xus], d)
        xu_t = [_unbounded(xus[b], bounds[b]) for b in range(B)]
        sg2k, sd2k, sck = ([np.zeros(xus[b].size) for b in range(B)] for _ in range(3))
        tr_kg = [[] for _ in range(B)]
        tr_xu = [[xus[b].copy()] for b in range(B)]

    def evaluate(first):
        pars = [OrderedDict(zip(names[b], cur[b])) for b in range(B)]
        if simul:
            ob, gr, kg, st = batch.eval_vi_knots(pars, cov_fun, xus, o["delta"], active=active,
                                                 bounds=bounds)
        elif objective == "laplace":
            ob, gr, st, nr = batch.eval_laplace(pars, cov_fun, xus, o["delta"], active=active,
                                                tol=o["tol_nr"], maxit=o["maxit_nr"])
            for b in range(B):
                if active[b] and st[b] == 0:
                    nr_iter[b].append(int(nr[b]))
        elif objective == "fitc":
            ob, gr, st = batch.eval_fitc(pars, cov_fun, xus, o["delta"], active=active)
        else:
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
            if simul:
                gknew = np.asarray(kg[b], dtype=np.float64)
                if keep[b] is not None:
                    gknew = gknew * keep[b]
                if not first and adadelta:      # not halved, unlike theta's (drivers._ascent)
                    sck[b] = o["decay"] * sck[b] + (1 - o["decay"]) * np.abs(np.sign(gknew) -
                                                                            np.sign(gk[b]))
                gk[b] = gknew
                tr_kg[b].append(gknew)
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
                    bool(np.any(np.abs(np.concatenate([gt[b], gk[b]])) > o["grad_tol"])) or
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
            if simul:
                if adadelta:
                    sg2k[b] = o["decay"] * sg2k[b] + (1 - o["decay"]) * gk[b] ** 2
                    step_k = ((1 / o["eta"]) ** sck[b]) * (np.sqrt(sd2k[b] + o["epsilon"]) /
                                                           np.sqrt(sg2k[b] + o["epsilon"])) * gk[b]
                    sd2k[b] = o["decay"] * sd2k[b] + (1 - o["decay"]) * step_k ** 2
                else:
                    step_k = o["learn_rate"] * gk[b]
                xu_t[b] = xu_t[b] + step_k.reshape(xus[b].shape)     # knot-major (Q16)
                xus[b] = _bounded(xu_t[b], bounds[b])                # every knot row at once
                tr_xu[b].append(xus[b].copy())
            cur[b] = np.exp(log_t[b])
        if not active.any():
            break
        evaluate(False)

    u_means, u_vars = [None] * B, [None] * B
    if any(e is None for e in error):
        u_means, u_vars = batch.posterior_u(muus)
    fmax = batch.get_f() if objective == "laplace" else None
    out = []
    for b in range(B):
        xy, _, mu = data[b]
        res = {"cov_par": OrderedDict(zip(names[b], cur[b])), "xu": xus[b], "iter": it[b],
               "obj_fun": np.array(tr_obj[b]), "grad": np.array(tr_grad[b]),
               "cov_par_history": np.array(tr_cov[b]),
               "knot_grad": np.array(tr_kg[b]) if simul else 0,
               "knot_history": np.stack(tr_xu[b], axis=2) if simul else xus[b],
               "cov_fun": cov_fun, "xy": np.array(xy), "mu": np.array(mu), "muu": muus[b],
               "u_mean": None if error[b] else u_means[b],
               "u_var": None if error[b] else u_vars[b]}
        if objective == "laplace":       # laplace_grad_ascent's dict (drivers.py)
            res["fmax"] = None if error[b] else fmax[b]
            res["nr_iter"] = np.array(nr_iter[b])
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


_ERR_Q10 = ('xu_opt = "simultaneous" passes cov_fun = "sqexp" to the driver '
            '(R/optimize_gp.R:320, 399), which cannot take an "ard" fit\'s cov_par; use "fixed"')


def _family_check(family, vi, xu_opt, who):
    """The refusals of a non-Gaussian family: optimize_gp's for vi = TRUE, and the knots fixed."""
    from .optimize import ERR_VI
    if family not in ("gaussian", "poisson", "bernoulli"):
        raise ValueError(f"family must be gaussian, poisson or bernoulli, not {family!r}")
    if family != "gaussian":
        if vi:
            raise ValueError(f'{who}: family = "{family}" needs vi = False ({ERR_VI})')
        if xu_opt != "fixed":
            raise ValueError(f"{who}: " + _ERR_LAP_KNOTS)


def _lap_starts(family, ys, expos):
    """optimize_gp's starts of the latent f: log(mean y) - log(expo) for Poisson
    (R/optimize_gp.R:480), 0 for Bernoulli (l.583)."""
    if family == "poisson":
        return [np.full(y.size, np.log(y.mean())) - np.log(e) for y, e in zip(ys, expos)]
    return [np.zeros(y.size) for y in ys]


def optimize_gp_batch(problems, cov_fun, cov_par_start, xu, muu=None, opt=None, xu_opt="fixed",
                      vi=True, family="gaussian", expo=None):
    """optimize_gp(y, xy, cov_fun, cov_par_start, mu, family = "gaussian", sparse = TRUE,
    xu_opt, xu, muu, vi, opt) for each (xy, y, mu) of `problems`, fitted in lockstep on
    one batch.  vi: True (the default here, as before) for the Titsias ELBO; False for FITC, the
    fit of optimize_gp(vi = FALSE) -- the reference's own default is vi = FALSE -- whose models
    predict_gp(mod, ..., vi=False), predictor_gp and score_gp(vi=False) take; with vi = False
    xu_opt = "simultaneous" raises a ValueError (FITC batches have no knot gradient yet).  xu_opt: "fixed" or "simultaneous" (all knots move, R/optimize_gp.R:396-412; with
    cov_fun = "ard" optimize_gp's quirk-Q10 ValueError); "oat" and "random" are refused.  cov_par_start, xu and muu: one value for all problems or a list with
    one per problem.  Returns a list of optimize_gp's {"results", "sparse", "family", "delta",
    "xu_init"} dicts (or its error strings), which predict_gp, predictor_gp and score_gp take.

    family: "gaussian" (the default, as before), or "poisson" / "bernoulli" for
    optimize_gp(family, sparse = TRUE, xu_opt = "fixed")'s Laplace fits: these
    need vi = False (vi = True raises a ValueError with optimize_gp's message) and
    xu_opt = "fixed"; expo: the Poisson exposure, one entry (a scalar or n_b values) per problem
    or one scalar for all (optimize_gp's a; None: 1); the latent f starts where optimize_gp
    starts it."""
    from .optimize import ERR_COV, ERR_GA, ERR_MAXKNOT, OPT_MASTER
    _family_check(family, vi, xu_opt, "optimize_gp_batch")
    simul = _xu_opt(xu_opt, "optimize_gp_batch")
    if simul and not vi:
        raise ValueError("optimize_gp_batch: " + _ERR_FITC_KNOTS)
    B = len(problems)
    o = {k: (dict(v) if isinstance(v, dict) else v) for k, v in OPT_MASTER.items()}
    for k, v in (opt or {}).items():
        if k in o:
            o[k] = dict(v) if isinstance(v, dict) else v
    if o["optim_method"] == "ga":
        return [ERR_GA] * B
    if cov_fun not in ("sqexp", "ard"):
        return [ERR_COV] * B
    if simul and cov_fun == "ard":
        raise ValueError(_ERR_Q10)
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
    if keep and family != "gaussian":
        ys = [np.asarray(p[1], dtype=np.float64).reshape(-1) for _, p, _, _ in keep]
        per = expo if isinstance(expo, (list, tuple)) else [expo] * B
        if len(per) != B:
            raise ValueError("optimize_gp_batch: expo must be one value or one per problem")
        expos = [np.broadcast_to(np.asarray(1.0 if per[b] is None else per[b], dtype=np.float64),
                                 (y.size,)) for (b, *_), y in zip(keep, ys)]
        res = laplace_grad_ascent_batch(
            [starts[b] for b, *_ in keep], cov_fun, [u for _, _, u, _ in keep],
            [p for _, p, _, _ in keep], [mb for *_, mb in keep], o, family=family, expo=expos,
            ff=_lap_starts(family, ys, expos))
    elif keep:
        driver = norm_grad_ascent_vi_batch if vi else norm_grad_ascent_batch
        res = driver([starts[b] for b, *_ in keep], cov_fun, [u for _, _, u, _ in keep],
                     [p for _, p, _, _ in keep], [mb for *_, mb in keep], o, xu_opt=xu_opt)
    if keep:
        for (b, _, u, _), r in zip(keep, res):
            out[b] = {"results": r, "sparse": True, "family": family, "delta": o["delta"],
                      "xu_init": u}
    return out


def cross_validate_gp(y, xy, cov_fun, cov_par_start, xu, folds=5, mu=None, muu=None, opt=None,
                      rng=None, xu_opt="fixed", vi=True, family="gaussian", expo=None):
    """k-fold cross-validation of optimize_gp(family = "gaussian", sparse = TRUE, vi,
    xu_opt): every fold's fit runs in lockstep on one batch and every fold's held-out rows are
    scored on it (SparseGPBatch.score), without the posteriors leaving the device.  vi: True (the
    default here, as before) for the Titsias ELBO and score_gp(vi = True)'s figures; False for
    FITC -- the reference's own default is vi = FALSE -- and score_gp(vi = False)'s figures, with
    xu_opt = "simultaneous" then refused by a ValueError (FITC batches have no knot gradient yet).  xu_opt is
    optimize_gp_batch's: "fixed", or "simultaneous" for folds whose knots move (each on
    knot_bounds of its own training rows); the scores then use the moved knots.

    folds: an integer (a random partition from rng, default np.random.default_rng(0)) or an
    integer array of fold ids, one per row.  Fold f trains on the rows of every other fold and
    holds its own out.  mu = None takes each fold's training mean(y) for its training rows and
    its held-out rows; an array mu is split by rows.  cov_par_start, xu and muu: one value for
    all folds or a list with one per fold.  The refusals are optimize_gp_batch's and come back as
    its error string.

    Returns {"folds": [{"model": an optimize_gp-shaped dict (predict_gp / score_gp take it),
    "score": score_gp's dict for the held-out rows, or the fit's error, "test_rows": indices}],
    "mean_nlp", "median_nlp" (over all held-out rows' finite nlp), "rmse" (over all held-out
    rows), "fold_id"}; the pooled figures cover the folds that were scored.

    family: "gaussian" (the default, as before), or "poisson" / "bernoulli" for the Laplace fits
    of optimize_gp_batch(family = ...) (vi = False and xu_opt = "fixed" are needed) scored by
    score_gp's figures for that family; expo: the Poisson exposure of the n rows (a scalar or n
    values; None: 1), split by rows like y and passed to the score as par = {"m": ...}."""
    from .optimize import ERR_COV, ERR_GA, ERR_MAXKNOT, OPT_MASTER
    _family_check(family, vi, xu_opt, "cross_validate_gp")
    simul = _xu_opt(xu_opt, "cross_validate_gp")
    if simul and not vi:
        raise ValueError("cross_validate_gp: " + _ERR_FITC_KNOTS)
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
    if simul and cov_fun == "ard":
        raise ValueError(_ERR_Q10)
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
        pars = None
        if family != "gaussian":
            ex = np.broadcast_to(np.asarray(1.0 if expo is None else expo, dtype=np.float64), (n,))
            batch.lap_init(family, np.concatenate([ex[tr] for tr in train_rows]))
            res = laplace_grad_ascent_batch(
                starts, cov_fun, us, batch, mbs, o, family=family,
                ff=_lap_starts(family, [y[tr] for tr in train_rows],
                               [ex[tr] for tr in train_rows]))
            if family == "poisson":
                pars = [{"m": ex[te]} for te in test_rows]
        else:
            driver = norm_grad_ascent_vi_batch if vi else norm_grad_ascent_batch
            res = driver(starts, cov_fun, us, batch, mbs, o, xu_opt=xu_opt)
        ok = np.array(["error" not in r for r in res], dtype=np.uint8)
        scores = [None] * B
        if ok.any():
            batch.set_test_problems(tests)
            scores = batch.score(ok) if pars is None else batch.score(ok, par=pars)
    finally:
        batch.close()
    out, nlps, errs = [], [], []
    for b in range(B):
        model = {"results": res[b], "sparse": True, "family": family, "delta": o["delta"],
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
