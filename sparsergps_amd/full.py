"""Full (non-sparse) GPs on the MI355X: the Gaussian family (config 1 of SURVEY.md sec. 8, rank 4
of 8(f)) and, in the second half of this module, the Laplace approximation for Poisson and
Bernoulli responses.

Host-side mirror of the reference's full-GP Gaussian path:
  obj_fun_norm_full      R/laplace_approx_obj_funs.R:56-61   (mvtnorm::dmvnorm, log = TRUE)
  dlogp_dcov_par_full    R/laplace_approx_gradient.R:1140-1269
  norm_grad_ascent_full  R/laplace_gradient_ascent.R:1700-2011
  predict_gp_full        R/laplace_approx_prediction.R:281-405
Sigma11 = k(xy, xy) + (tau^2 + delta) I is built, inverted (Gauss-Jordan, MFMA) and contracted
against dSigma11/dlog(theta) on the device (sgp_eval_full); the n x n system lives in a
SparseGPContext whose "knots" are its own rows.  Quirk kept: the gradient's alpha is
Sigma11^-1 y, not Sigma11^-1 (y - mu) (laplace_approx_gradient.R:1186).
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from . import _lib
from .covariance import theta_vector
from .drivers import _ascent, _opts
from .predict import _predict
from .vi import SparseGPContext, param_names

_CTX = {}


def _ctx_for(xy, y, mu):
    xy = np.asarray(xy, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    xy = xy.reshape(y.size, -1)
    mu = np.broadcast_to(np.asarray(mu, dtype=np.float64), y.shape)
    key = (xy.shape, xy.tobytes(), y.tobytes(), mu.tobytes())
    ctx = _CTX.get(key)
    if ctx is None:
        _CTX.clear()
        ctx = SparseGPContext(xy, y, mu, m_max=y.size)
        _CTX[key] = ctx
    return ctx, xy.shape[1]


def full_eval(cov_par, cov_fun, xy, y, mu, delta=1e-6, ctx=None, obj_only=False):
    """(log dmvnorm(y; mu, Sigma11), OrderedDict d/dlog(theta) in names(cov_par) order)."""
    if ctx is None:
        ctx, d = _ctx_for(xy, y, mu)
    else:
        d = ctx.d
    lnames = [f"l{c + 1}" for c in range(d)] if cov_fun == "ard" else None
    theta = theta_vector(cov_par, cov_fun, d, lnames)
    obj, g = ctx.eval_full(theta, cov_fun, delta, obj_only)
    if obj_only:
        return obj, None
    byname = dict(zip(param_names(cov_fun, d, lnames), g))
    return obj, OrderedDict((k, float(byname[k])) for k in cov_par.keys())


def obj_fun_norm_full(cov_par, cov_fun, xy, y, mu, delta=1e-6, ctx=None):
    """R/laplace_approx_obj_funs.R:56-61 at Sigma11(cov_par)."""
    return full_eval(cov_par, cov_fun, xy, y, mu, delta, ctx, obj_only=True)[0]


def dlogp_dcov_par_full(cov_par, cov_fun, dcov_fun_dtheta=True, xy=None, y=None, mu=None,
                        transform=True, delta=1e-6, ctx=None):
    """R/laplace_approx_gradient.R:1140-1269: {"gradient", "trans_par"}."""
    if mu is None:
        mu = np.mean(np.asarray(y, dtype=np.float64))
    _, grad = full_eval(cov_par, cov_fun, xy, y, mu, delta, ctx)
    trans_par = OrderedDict((k, float(np.log(v))) for k, v in cov_par.items())
    return {"gradient": grad if dcov_fun_dtheta else 0, "trans_par": trans_par}


def norm_grad_ascent_full(cov_par_start, cov_fun, dcov_fun_dtheta=True, xy=None, y=None,
                          mu=None, opt=None, verbose=False, ctx=None):
    """R/laplace_gradient_ascent.R:1700-2011 (obj_fun = obj_fun_norm_full): the drivers'
    Adadelta / "ga" loop with one fused device evaluation per iteration."""
    o = _opts(opt)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    if mu is None or (np.ndim(mu) == 0 and not np.isfinite(mu)):
        mu = np.full(y.size, y.mean())
    mu = np.broadcast_to(np.asarray(mu, dtype=np.float64), y.shape)
    if ctx is None:
        ctx, _ = _ctx_for(xy, y, mu)

    def evaluate(cov_par, _xu):
        obj, g = full_eval(cov_par, cov_fun, xy, y, mu, o["delta"], ctx)
        return obj, [g[k] for k in cov_par.keys()], None

    out = _ascent(evaluate, cov_par_start, np.zeros((1, 1)), None, bool(dcov_fun_dtheta), False,
                  o, verbose)
    return {"cov_par": out["cov_par"], "cov_fun": cov_fun, "xy": np.asarray(xy), "y": y,
            "mu": mu, "iter": out["iter"], "obj_fun": out["obj_fun"], "grad": out["grad"],
            "cov_par_history": out["cov_par_history"]}


def predict_gp_full(xy, y, x_pred, cov_fun, cov_par, mu, mu_pred, full_cov=False, delta=1e-6):
    """R/laplace_approx_prediction.R:281-405: mean mu_pred + Sigma12 Sigma22^-1 (y - mu),
    variance Sigma11 - Sigma12 Sigma22^-1 Sigma21 (diagonal unless full_cov)."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    xy = np.asarray(xy, dtype=np.float64).reshape(y.size, -1)
    mu = np.broadcast_to(np.asarray(mu, dtype=np.float64), y.shape)
    return _predict(_lib.SGP_PRED_FULL, True, y, None, xy, x_pred, cov_fun, cov_par, mu_pred, mu,
                    full_cov, delta)


# ------------------------------------------------------------------ full-GP Laplace
# family = "poisson" / "bernoulli" with sparse = FALSE (R/optimize_gp.R:687-732):
#   newtrapGP                 R/newtrapGP.R:6-177
#   obj_fun_pois_full         R/laplace_approx_obj_funs.R:67-102
#   obj_fun_bern_full         R/laplace_approx_obj_funs.R:346-397
#   dlogq_dcov_par_full       R/laplace_approx_gradient.R:558-711
#   laplace_grad_ascent_full  R/laplace_gradient_ascent.R:630-1016
#   predict_laplace_full      R/laplace_approx_prediction.R:128-214
# One device evaluation (sgp_eval_full_laplace) is newtrapGP warm-started from the resident mode
# followed by dlogq_dcov_par_full there.  The Bernoulli family keeps the reference's W (quirk
# Q19), does not read the exposure `m` and has no default mean.


def _lap_ctx(xy, y, mu, family, ctx):
    if family not in _lib.FAMILIES:
        raise ValueError(f"family must be one of {sorted(_lib.FAMILIES)}, not {family!r}")
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    if mu is None:
        if family != "poisson":
            raise ValueError(f'mu=None is a Poisson convention; pass mu with family="{family}"')
        mu = np.log(np.mean(y))
    if ctx is None:
        ctx, _ = _ctx_for(xy, y, mu)
    ctx.lap_set_family(family)
    return ctx


def _theta(cov_par, cov_fun, d):
    lnames = [f"l{c + 1}" for c in range(d)] if cov_fun == "ard" else None
    return theta_vector(cov_par, cov_fun, d, lnames), param_names(cov_fun, d, lnames)


def full_laplace_eval(cov_par, cov_fun, xy, y, mu, ff=None, m=1.0, delta=1e-6, tol=1e-6,
                      maxit=1000, ctx=None, family="poisson", obj_only=False):
    """newtrapGP from `ff` (None: the context's resident mode), then dlogq_dcov_par_full at the
    mode: dict(objective, gradient (names(cov_par) order; None with obj_only), gp,
    objective_function_values, nr_iter).  maxit is the C ABI's: 0 = at ff as given, no NR step."""
    ctx = _lap_ctx(xy, y, mu, family, ctx)
    theta, names = _theta(cov_par, cov_fun, ctx.d)
    if ff is not None:
        ctx.lap_set_f(ff)
    obj, g, it = ctx.eval_full_laplace(theta, cov_fun, delta, m, tol, maxit, obj_only)
    grad = None
    if not obj_only:
        byname = dict(zip(names, g))
        grad = OrderedDict((k, float(byname[k])) for k in cov_par.keys())
    return {"objective": obj, "gradient": grad, "gp": ctx.lap_get_f(),
            "objective_function_values": ctx.lap_objective_values(), "nr_iter": it}


def newtrapGP(start_vals, cov_par, cov_fun, xy, y, mu, m=1.0, delta=1e-6, maxit=10000, tol=1e-6,
              ctx=None, family="poisson"):
    """R/newtrapGP.R:6-177: {"gp", "objective_function_values", "gradient" (grad psi),
    "grad_log_py_ff", "W"}; the last three at the iterate the last update started from, as the
    reference's loop leaves them.  The reference's "L" (chol of I + sqrt(-W) Sigma sqrt(-W)) is
    not returned: predict_laplace_full rebuilds it from W."""
    ctx = _lap_ctx(xy, y, mu, family, ctx)
    theta, _ = _theta(cov_par, cov_fun, ctx.d)
    if start_vals is not None:
        ctx.lap_set_f(start_vals)
    ctx.eval_full_laplace(theta, cov_fun, delta, m, tol, max(int(maxit), 1), obj_only=True)
    W, g = ctx.full_laplace_state()
    return {"gp": ctx.lap_get_f(), "objective_function_values": ctx.lap_objective_values(),
            "gradient": ctx.lap_get_grad_psi(), "grad_log_py_ff": g, "W": W}


def obj_fun_pois_full(ff, cov_par, cov_fun, xy, y, mu, m=1.0, delta=1e-6, ctx=None):
    """R/laplace_approx_obj_funs.R:67-102 at ff, Sigma = Sigma11(cov_par)."""
    return full_laplace_eval(cov_par, cov_fun, xy, y, mu, ff, m, delta, 0.0, 0, ctx, "poisson",
                             obj_only=True)["objective"]


def obj_fun_bern_full(ff, cov_par, cov_fun, xy, y, mu, delta=1e-6, ctx=None):
    """R/laplace_approx_obj_funs.R:346-397 at ff, Sigma = Sigma11(cov_par)."""
    return full_laplace_eval(cov_par, cov_fun, xy, y, mu, ff, 1.0, delta, 0.0, 0, ctx,
                             "bernoulli", obj_only=True)["objective"]


def dlogq_dcov_par_full(cov_par, cov_fun, dcov_fun_dtheta=True, xy=None, y=None, ff=None,
                        mu=None, m=1.0, transform=True, delta=1e-6, ctx=None, family="poisson"):
    """R/laplace_approx_gradient.R:558-711 at the given ff (no NR step): {"gradient",
    "trans_par"}."""
    r = full_laplace_eval(cov_par, cov_fun, xy, y, mu, ff, m, delta, 0.0, 0, ctx, family)
    trans_par = OrderedDict((k, float(np.log(v))) for k, v in cov_par.items())
    return {"gradient": r["gradient"] if dcov_fun_dtheta else 0, "trans_par": trans_par}


def laplace_grad_ascent_full(cov_par_start, cov_fun, dcov_fun_dtheta=True, xy=None, y=None,
                             ff=None, mu=None, m=1.0, opt=None, verbose=False, ctx=None,
                             family="poisson"):
    """R/laplace_gradient_ascent.R:630-1016: the drivers' Adadelta / "ga" loop with one fused
    device evaluation (newtrapGP warm-started from the previous mode + dlogq_dcov_par_full) per
    iteration.  ff=None takes optimize_gp's start values: log(mean(y)) - log(m) for Poisson
    (R/optimize_gp.R:702), 0 for Bernoulli (l.722).  A non-numeric mu is mean(y) (l.722-725 of
    the driver).  Returns the reference's list, with fmax, W and grad_log_py_ff."""
    o = _opts(opt, {"maxit_nr": 1000, "tol_nr": 1e-6})
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    xy_m = np.asarray(xy, dtype=np.float64).reshape(y.size, -1)
    if mu is None or (np.ndim(mu) == 0 and not np.isfinite(mu)):
        mu = np.full(y.size, y.mean())
    mu = np.broadcast_to(np.asarray(mu, dtype=np.float64), y.shape)
    if ff is None:
        ff = (np.full(y.size, np.log(y.mean())) - np.log(m)) if family == "poisson" \
            else np.zeros(y.size)
    ctx = _lap_ctx(xy_m, y, mu, family, ctx)
    ctx.lap_set_f(ff)
    nr_iter = []

    def evaluate(cov_par, _xu):
        theta, names = _theta(cov_par, cov_fun, ctx.d)
        obj, g, it = ctx.eval_full_laplace(theta, cov_fun, o["delta"], m, o["tol_nr"],
                                           max(int(o["maxit_nr"]), 1))
        nr_iter.append(it)
        byname = dict(zip(names, g))
        return obj, [byname[k] for k in cov_par.keys()], None

    out = _ascent(evaluate, cov_par_start, np.zeros((1, 1)), None, bool(dcov_fun_dtheta), False,
                  o, verbose)
    W, g = ctx.full_laplace_state()
    return {"cov_par": out["cov_par"], "cov_fun": cov_fun, "xy": xy_m, "y": y, "mu": mu,
            "fmax": ctx.lap_get_f(), "iter": out["iter"], "obj_fun": out["obj_fun"],
            "grad": out["grad"], "cov_par_history": out["cov_par_history"], "W": W,
            "grad_log_py_ff": g, "nr_iter": np.array(nr_iter)}


def predict_laplace_full(ff=None, xy=None, x_pred=None, W=None, cov_par=None, cov_fun=None,
                         grad_log_py_ff=None, mu=None, mu_pred=None, full_cov=False, delta=1e-6):
    """R/laplace_approx_prediction.R:128-214: mean mu_pred + Sigma12 grad_log_py_ff, variance
    Sigma11 - Sigma12 R Sigma21 with R = sqrt(-W) (I + sqrt(-W) Sigma sqrt(-W))^-1 sqrt(-W)
    (diagonal unless full_cov).  ff and mu are accepted as the reference accepts them and, as
    there, not used.  The mean is returned with full_cov too (the reference leaves it undefined
    there and fails: DESIGN.md Q20)."""
    W = np.asarray(W, dtype=np.float64).reshape(-1)
    xy = np.asarray(xy, dtype=np.float64).reshape(W.size, -1)
    return _predict(_lib.SGP_PRED_LAPLACE_FULL, False, grad_log_py_ff, None, xy, x_pred, cov_fun,
                    cov_par, mu_pred, W, full_cov, delta)
