"""A resident predictor on the MI355X (sgp_predictor_*, include/sgp.h).

`predict_vi` / `predict_laplace` / `predict_gp_full` / `predict_laplace_full` redo the fit's
m x m stage and allocate their work space on every call, and hold K(x_pred, xu) in full.  A
``Predictor`` does the m x m stage once and then streams any number of batches of any size
through a fixed chunk work space (full_cov stays with the predict_* functions):

    with Predictor("laplace", u_mean, u_var, xu, cov_fun, cov_par, muu, family) as p:
        for x, mu in batches:
            out = p.predict(x, mu)              # {"pred_mean": (np, 1), "pred_var": (np,)}

`predictor_gp(mod, vi)` builds one from a fit object with predict_gp's dispatch
(R/laplace_approx_prediction.R:408-542).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .covariance import theta_vector
from .vi import _device

METHODS = {"vi": _lib.SGP_PRED_VI, "laplace": _lib.SGP_PRED_LAPLACE, "full": _lib.SGP_PRED_FULL,
           "laplace_full": _lib.SGP_PRED_LAPLACE_FULL}


class Predictor:
    """method: "vi" (predict_vi), "laplace" (predict_laplace), "full" (predict_gp_full: xu = xy,
    u_mean = y, muu = mu, u_var = None) or "laplace_full" (predict_laplace_full: xu = xy, u_mean =
    grad_log_py_ff, muu = W, u_var = None).  The other arguments are the predict_* functions'."""

    def __init__(self, method, u_mean, u_var, xu, cov_fun, cov_par, muu, family="gaussian",
                 delta=1e-6, device=None):
        if method not in METHODS:
            raise ValueError(f"method must be one of {sorted(METHODS)}, not {method!r}")
        self._lib = _lib.lib()
        self._h = None
        self.method, self.family = method, family
        self.device = _device() if device is None else int(device)
        U = np.asarray(xu, dtype=np.float64)
        if U.ndim == 1:
            U = U.reshape(-1, 1)
        U = np.asfortranarray(U)
        self.m, self.d = U.shape
        m, d = self.m, self.d
        lnames = [f"l{c + 1}" for c in range(d)] if cov_fun == "ard" else None
        theta = np.ascontiguousarray(theta_vector(cov_par, cov_fun, d, lnames))
        um = np.ascontiguousarray(np.asarray(u_mean, dtype=np.float64).reshape(-1)[:m])
        mu_u = np.ascontiguousarray(np.broadcast_to(
            np.asarray(muu, dtype=np.float64).reshape(-1)[:m] if np.ndim(muu) else
            np.asarray(muu, dtype=np.float64), (m,)))
        uv = (None if u_var is None
              else np.asfortranarray(np.asarray(u_var, dtype=np.float64).reshape(m, m)))
        if cov_fun not in _lib.KERNELS:
            raise ValueError(f"unknown covariance function {cov_fun!r}")
        args = (_lib.KERNELS[cov_fun], _lib.dptr(theta), float(delta), METHODS[method],
                1 if family == "gaussian" else 0, _lib.dptr(U), m, m)
        tail = (_lib.dptr(um), _lib.dptr(mu_u), None if uv is None else _lib.dptr(uv), m)
        # the argument checks need no device; everything after them does (no CPU fallback)
        _lib.check(self._lib.sgp_diag_predictor_args(d, *args, *tail))
        try:
            _lib.require_gpu()
        except RuntimeError as e:
            raise _lib.SGPError(_lib.SGP_EHIP, str(e)) from None
        h = C.c_void_p()
        _lib.check(self._lib.sgp_predictor_create(C.byref(h), self.device, *args, d, *tail))
        self._h = h

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            _lib.check(self._lib.sgp_predictor_destroy(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._h is None:
            raise _lib.SGPError(_lib.SGP_EINVAL, "the predictor is closed")
        return self._h

    def _inputs(self, x_pred, mu_pred):
        x = np.asarray(x_pred, dtype=np.float64)
        if x.ndim == 1:
            x = x.reshape(-1, 1)
        if x.shape[1] != self.d:
            raise ValueError(f"x_pred has {x.shape[1]} columns; the knots have {self.d}")
        x = np.asfortranarray(x)
        n = x.shape[0]
        mu = np.ascontiguousarray(np.broadcast_to(np.asarray(mu_pred, dtype=np.float64).reshape(-1)
                                                  if np.ndim(mu_pred) else
                                                  np.asarray(mu_pred, dtype=np.float64), (n,)))
        return x, mu, n

    def predict(self, x_pred, mu_pred, chunk_rows=0, route=0, stage_ms=None):
        """{"pred_mean": (np, 1), "pred_var": (np,)}.  chunk_rows / route other than 0 and
        stage_ms (an array of 4 doubles to fill) go through sgp_diag_predictor_run."""
        x, mu, n = self._inputs(x_pred, mu_pred)
        pm, pv = np.zeros(n), np.zeros(n)
        if chunk_rows or route or stage_ms is not None:
            _lib.check(self._lib.sgp_diag_predictor_run(
                self._handle(), int(chunk_rows), int(route), _lib.dptr(x), n, n, _lib.dptr(mu),
                _lib.dptr(pm), _lib.dptr(pv), None if stage_ms is None else _lib.dptr(stage_ms)))
        else:
            _lib.check(self._lib.sgp_predictor_run(self._handle(), _lib.dptr(x), n, n,
                                                   _lib.dptr(mu), _lib.dptr(pm), _lib.dptr(pv)))
        return {"pred_mean": pm.reshape(-1, 1), "pred_var": pv}

    def score(self, x_test, y_test, mu_pred, family=None, par=None, expo=None):
        """predict(x_test, mu_pred) scored against y_test on the device (my_nlp's rule): adds
        "nlp" (np values) and "stats" = [sum of the finite nlp, their count, NaN rows,
        sum (pred_mean - y)^2].  par: tau (gaussian) or the scalar exposure (poisson), or the
        reference's par list ({"tau": ..} / {"m": ..}); expo: one poisson exposure per row."""
        from .evaluation import _score_par
        family = self.family if family is None else family
        if family not in _lib.SCORE_FAMILIES:
            raise ValueError(f"family must be one of {sorted(_lib.SCORE_FAMILIES)}, not {family!r}")
        x, mu, n = self._inputs(x_test, mu_pred)
        y = np.ascontiguousarray(np.asarray(y_test, dtype=np.float64).reshape(-1))
        if y.size != n:
            raise ValueError(f"y has {y.size} values for {n} prediction rows")
        if par is None or isinstance(par, dict):
            p, ex = _score_par(family, par)
        else:
            p, ex = float(par), None
        if expo is not None:
            ex = np.ascontiguousarray(np.broadcast_to(np.asarray(expo, dtype=np.float64), (n,)))
        if ex is not None and ex.size != n:
            raise ValueError(f"the exposure has {ex.size} values for {n} rows")
        pm, pv, nlp, stats = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(4)
        _lib.check(self._lib.sgp_predictor_run_nlp(
            self._handle(), _lib.dptr(x), n, n, _lib.dptr(mu), _lib.dptr(pm), _lib.dptr(pv),
            _lib.SCORE_FAMILIES[family], _lib.dptr(y), p, None if ex is None else _lib.dptr(ex),
            _lib.dptr(nlp), _lib.dptr(stats)))
        return {"pred_mean": pm.reshape(-1, 1), "pred_var": pv, "nlp": nlp, "stats": stats}

    def predict_torch(self, x, mu, box=None):
        """x: (np, d) float64 torch tensor on this predictor's device, mu: (np,) or a scalar.
        Returns {"pred_mean": (np, 1), "pred_var": (np,)} device tensors, queued on the current
        torch stream with no host round trip.  box = (lo, hi), d values each bounding x's
        columns, lets the K builder use its matrix-core form (with x's exact column range the
        result is bit-identical to predict's); None: the exact-difference form."""
        import torch
        h = self._handle()
        if x.dim() == 1:
            x = x.reshape(-1, 1)
        dev = torch.device("cuda", self.device)
        if x.device != dev or x.dtype != torch.float64 or x.shape[1] != self.d:
            raise ValueError(f"x must be a float64 (np, {self.d}) tensor on {dev}")
        n = x.shape[0]
        xt = x.t().contiguous()   # d x np row-major = np x d column-major, ld np
        mu_t = torch.as_tensor(mu, dtype=torch.float64, device=dev).reshape(-1)
        mu_t = mu_t.expand(n).contiguous()
        pm = torch.empty(n, dtype=torch.float64, device=dev)
        pv = torch.empty(n, dtype=torch.float64, device=dev)
        lo = hi = None
        if box is not None:
            lo = np.ascontiguousarray(np.asarray(box[0], dtype=np.float64).reshape(-1))
            hi = np.ascontiguousarray(np.asarray(box[1], dtype=np.float64).reshape(-1))
            if lo.size != self.d or hi.size != self.d:
                raise ValueError(f"box needs {self.d} values per side")
        stream = torch.cuda.current_stream(dev)
        _lib.check(self._lib.sgp_predictor_run_dev(
            h, xt.data_ptr(), n, n, mu_t.data_ptr(), pm.data_ptr(), pv.data_ptr(),
            None if lo is None else _lib.dptr(lo), None if hi is None else _lib.dptr(hi),
            stream.cuda_stream))
        # xt and mu_t are temporaries the queued work still reads: tie them to the stream
        xt.record_stream(stream)
        mu_t.record_stream(stream)
        return {"pred_mean": pm.reshape(-1, 1), "pred_var": pv}


def predictor_gp(mod, vi=False):
    """A Predictor for the fit object `mod` with predict_gp's dispatch
    (R/laplace_approx_prediction.R:408-542): sparse fits (vi: predict_vi, else predict_laplace),
    the full Gaussian GP and full Poisson / Bernoulli fits.  As there, vi with a non-Gaussian
    family returns the reference's error string."""
    family = mod["family"]
    res = mod["results"]
    delta = mod.get("delta", 1e-6)
    if vi and family != "gaussian":
        return "Error: VI not supported for non-gaussian data."
    if not mod.get("sparse", True):
        if family != "gaussian":
            return Predictor("laplace_full", res["grad_log_py_ff"], None, res["xy"],
                             res["cov_fun"], res["cov_par"], res["W"], family, delta)
        y = np.asarray(res["y"], dtype=np.float64).reshape(-1)
        mu = np.broadcast_to(np.asarray(res["mu"], dtype=np.float64), y.shape)
        xy = np.asarray(res["xy"], dtype=np.float64).reshape(y.size, -1)
        return Predictor("full", y, None, xy, res["cov_fun"], res["cov_par"], mu, family, delta)
    m = np.asarray(res["xu"]).shape[0]
    if vi:
        return Predictor("vi", res["u_mean"], res["u_var"], res["xu"], res["cov_fun"],
                         res["cov_par"], res["muu"], family, delta)
    return Predictor("laplace", np.asarray(res["u_mean"])[:m], res["u_var"], res["xu"],
                     res["cov_fun"], res["cov_par"], np.asarray(res["muu"])[:m], family, delta)
