"""One-at-a-time (OAT) knot selection: the reference's ``xu_opt = "oat"`` fits

  oat_knot_selection_norm_vi   R/vi_functions.R:1340-1579        (VI, norm_grad_ascent_vi)
  oat_knot_selection_norm      R/oat_knot_selection.R:311-548    (FITC, norm_grad_ascent)
  oat_knot_selection           R/oat_knot_selection.R:14-306     (Laplace, laplace_grad_ascent)

All three are one loop (``oat_core``): fit the covariance parameters with the starting knots
fixed; then, while there is room for a knot (and, with chooseK, while the last knot paid off),
propose a knot, refit with it appended -- the ascent moves only the appended knot when cov_diff
-- and keep it if the objective rose by more than tol_knot (always, without chooseK).  The core
takes the fit and the proposal as callables, so it runs over any drivers; the wrappers bind this
package's drivers and proposals to ONE SparseGPContext with room for maxknot knots, so the rows
are uploaded once per OAT run, not once per added knot.

Reproduced as written: each function's opt_master; unknown opt names
skipped; the whole merged opt handed to the driver and to the proposal, each of which merges it
by name into its own defaults (so OAT's grad_tol = 1 and ego_cov_par$tau = 1e-3 reach them);
muu grows by muu[1]; the two return shapes (``upost`` with u_mean = upost[[iter]] when the
loop ended on maxknot, ``u_post`` with upost[[iter - 1]] otherwise).
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np

from . import proposals as P
from ._lib import NotPositiveDefinite

_EGO = {"ego_cov_par": {"sigma": 3.0, "l": 1.0, "tau": 1e-3}, "ego_cov_fun": "exp"}
_COMMON = {"optim_method": "adadelta", "decay": 0.95, "epsilon": 1e-6, "learn_rate": 1e-2,
           "eta": 1e3, "maxit": 1000, "grad_tol": 1.0, "maxit_nr": 1000, "delta": 1e-6,
           "maxknot": 30, "TTmin": 10, **_EGO, "cov_diff": True, "chooseK": True}
# R/vi_functions.R:1383-1393
OPT_OAT_NORM_VI = {**_COMMON, "obj_tol": 1e-3, "tol_knot": 1e-3, "TTmax": 40}
# R/oat_knot_selection.R:354-362
OPT_OAT_NORM = {**_COMMON, "obj_tol": 1e-3, "tol_knot": 1e-3, "TTmax": 40}
# R/oat_knot_selection.R:67-75
OPT_OAT = {**_COMMON, "obj_tol": 1e-2, "tol_knot": 1e-1, "tol_nr": 1e-5, "TTmax": 30}


def merge_opt(master, opt):
    """The reference's loop over names(opt): unknown names are skipped silently."""
    return P._merge_opt(master, opt)


def oat_core(fit, propose, cov_par_start, xu_start, muu_start, o, laplace=False, ff=None,
             verbose=False):
    """The loop of the three OAT functions (R/vi_functions.R:1447-1577;
    R/oat_knot_selection.R:131-304).

    fit(cov_par, xu, knot_opt, dknot, muu, ff) -> the driver's result (cov_par, xu, obj_fun,
    iter, u_mean, u_var and, for Laplace, fmax and muu); knot_opt is None or the 1-based indices
    the ascent may move, dknot says whether knots move at all.  propose(fit_result) -> the 1 x d
    knot.  o: the merged opt (maxknot, tol_knot, chooseK, cov_diff).  laplace=True adds the
    Laplace variant's warm start from the accepted fmax, its try-error branch (a
    NotPositiveDefinite ascent leaves the previous fit in place) and the ``success`` flag."""
    chooseK, cov_diff = bool(o["chooseK"]), bool(o["cov_diff"])
    tol_knot, maxknot = float(o["tol_knot"]), int(o["maxknot"])
    xu = np.array(xu_start, dtype=np.float64)
    xu = xu.reshape(xu.shape[0], -1)
    muu = np.array(muu_start, dtype=np.float64).reshape(-1)
    obj_fun_vals, ga_steps = [], []
    cov_par_vals = [np.array([float(v) for v in cov_par_start.values()])]

    opt = fit(cov_par_start, xu, None, False, muu, ff)      # knots fixed
    current = float(np.asarray(opt["obj_fun"]).reshape(-1)[-1])
    obj_fun_vals.append(current)
    cov_par_vals.append(np.array([float(v) for v in opt["cov_par"].values()]))
    cov_par = OrderedDict(opt["cov_par"])
    ga_steps.append(int(opt["iter"]))
    fmax = None
    if laplace:                                             # oat_knot_selection.R:180-182
        fmax = opt["fmax"]
        muu = np.array(opt["muu"], dtype=np.float64).reshape(-1)
        xu = np.array(opt["xu"], dtype=np.float64)
    upost = {1: {"mean": opt["u_mean"], "var": opt["u_var"]}}
    numknots = np.asarray(xu_start).reshape(xu.shape[0], -1).shape[0]
    it = 1
    success = True

    def go_on():
        if numknots >= maxknot:
            return False
        if not chooseK or len(obj_fun_vals) == 1:
            return True
        return current - obj_fun_vals[-2] > tol_knot

    while go_on():
        it += 1
        if verbose:
            print(it)
        knot_prop = np.asarray(propose(opt), dtype=np.float64).reshape(1, -1)
        if verbose:
            print(knot_prop)
        m = xu.shape[0]
        knot_opt = list(range(m + 1, m + 2)) if cov_diff else None     # 1-based, as the drivers
        muu_try = np.append(muu, muu[0])
        if laplace:
            success = False
            try:
                opt = fit(cov_par, np.vstack([xu, knot_prop]), knot_opt, cov_diff, muu_try, fmax)
                success = True
            except NotPositiveDefinite:     # class(opt_temp) == "try-error": opt stays
                pass
        else:
            opt = fit(cov_par, np.vstack([xu, knot_prop]), knot_opt, cov_diff, muu_try, None)
        ga_steps.append(int(opt["iter"]))
        current = float(np.asarray(opt["obj_fun"]).reshape(-1)[-1])
        obj_fun_vals.append(current)
        if (current - obj_fun_vals[-2] > tol_knot) if chooseK else True:
            cov_par_vals.append(np.array([float(v) for v in opt["cov_par"].values()]))
            if laplace:
                fmax = opt["fmax"]
            upost[it] = {"mean": opt["u_mean"], "var": opt["u_var"]}
            xu = np.array(opt["xu"], dtype=np.float64)
            muu = muu_try
            cov_par = OrderedDict(opt["cov_par"])
            numknots = xu.shape[0]

    # the two return shapes (vi_functions.R:1550-1577): on maxknot the posterior of iteration
    # iter under "upost"; otherwise the one of iter - 1 under "u_post"
    on_max = numknots == maxknot
    pick = it if on_max else it - 1
    if pick not in upost:
        raise ValueError(f"the reference reads upost[[{pick}]], which this run never stored "
                         f"({numknots} knots, maxknot = {maxknot})")
    out = {"cov_par": cov_par, "xu": xu, "obj_fun": np.array(obj_fun_vals),
           "u_mean": upost[pick]["mean"], "muu": muu, "u_var": upost[pick]["var"],
           "cov_par_history": np.vstack(cov_par_vals), "ga_steps": np.array(ga_steps),
           ("upost" if on_max else "u_post"): [upost.get(k) for k in range(1, it + 1)]}
    if laplace:
        out["fmax"] = fmax
        out["success"] = success
    return out


# ------------------------------------------------------------------ the three wrappers
_PROPOSAL_NAMES = ("knot_prop_ego_norm_vi", "knot_prop_ego_norm", "knot_prop_ego",
                   "knot_prop_random_norm_vi", "knot_prop_random_norm", "knot_prop_random",
                   "knot_prop_var", "knot_prop_error")


def _resolve_proposal(proposal_fun):
    if isinstance(proposal_fun, str):
        if proposal_fun not in _PROPOSAL_NAMES:
            raise ValueError(f"proposal_fun must be callable or one of {_PROPOSAL_NAMES}")
        return getattr(P, proposal_fun)
    if not callable(proposal_fun):
        raise ValueError("proposal_fun must be callable")
    return proposal_fun


def _dknot(cov_fun):
    return "ard" if cov_fun == "ard" else "sqexp"       # dsqexp_dx2_ard / dsqexp_dx2


def _prepare(xy, y, mu, xu_start, muu_start, default_mean):
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    xy = np.asarray(xy, dtype=np.float64).reshape(y.size, -1)
    xu = np.asarray(xu_start, dtype=np.float64).reshape(-1, xy.shape[1])
    if mu is None:
        mu = np.full(y.size, default_mean(y))
    if muu_start is None:
        muu_start = np.full(xu.shape[0], default_mean(y))
    mu = np.ascontiguousarray(np.broadcast_to(np.asarray(mu, dtype=np.float64), y.shape))
    muu = np.broadcast_to(np.asarray(muu_start, dtype=np.float64), (xu.shape[0],)).copy()
    return xy, y, mu, xu, muu


def _own_context(ctx, xy, y, mu, o, xu):
    from .vi import SparseGPContext
    need = max(int(o["maxknot"]), xu.shape[0] + 1)
    if ctx is not None:
        if ctx.m_max < need:
            raise ValueError(f"the context holds {ctx.m_max} knots; this OAT run needs {need}")
        return ctx
    return SparseGPContext(xy, y, mu, m_max=need)


def _gaussian_oat(driver, master, cov_par_start, cov_fun, xu_start, proposal_fun, xy, y, mu,
                  muu_start, opt, verbose, ctx, rng, proposal_kw):
    o = merge_opt(master, opt)
    xy, y, mu, xu, muu = _prepare(xy, y, mu, xu_start, muu_start, np.mean)
    ctx = _own_context(ctx, xy, y, mu, o, xu)
    prop = _resolve_proposal(proposal_fun)
    kw = dict(proposal_kw or {})
    if rng is not None:
        kw.setdefault("rng", rng)

    def fit(cov_par, U, knot_opt, dknot, muu_now, _ff):
        res = driver(cov_par, cov_fun, True, _dknot(cov_fun) if dknot else None, knot_opt, U, xy,
                     y, mu, muu_now, o, verbose, ctx)
        res["muu"] = np.asarray(muu_now, dtype=np.float64)
        return res

    def propose(fit_res):
        return prop(fit_res, o, y=y, ctx=ctx, **kw)

    out = oat_core(fit, propose, OrderedDict(cov_par_start), xu, muu, o, verbose=verbose)
    out.update({"cov_fun": cov_fun, "mu": mu})
    return out


def oat_knot_selection_norm_vi(cov_par_start, cov_fun, xu_start, proposal_fun, xy, y, mu=None,
                               muu_start=None, opt=None, verbose=False, ctx=None, rng=None,
                               proposal_kw=None):
    """oat_knot_selection_norm_vi (R/vi_functions.R:1340-1579): OAT knot selection for the
    Titsias-ELBO fit.  proposal_fun: one of this package's proposals (the function or its name)
    or a callable (fit, opt, y=, ctx=, **proposal_kw) -> 1 x d knot; rng (a numpy Generator) is
    forwarded to it.  mu / muu_start default to mean(y) (l.1437-1444)."""
    from .drivers import norm_grad_ascent_vi
    return _gaussian_oat(norm_grad_ascent_vi, OPT_OAT_NORM_VI, cov_par_start, cov_fun, xu_start,
                         proposal_fun, xy, y, mu, muu_start, opt, verbose, ctx, rng, proposal_kw)


def oat_knot_selection_norm(cov_par_start, cov_fun, xu_start, proposal_fun, xy, y, mu=None,
                            muu_start=None, opt=None, verbose=False, ctx=None, rng=None,
                            proposal_kw=None):
    """oat_knot_selection_norm (R/oat_knot_selection.R:311-548): the same for the FITC fit."""
    from .drivers import norm_grad_ascent
    return _gaussian_oat(norm_grad_ascent, OPT_OAT_NORM, cov_par_start, cov_fun, xu_start,
                         proposal_fun, xy, y, mu, muu_start, opt, verbose, ctx, rng, proposal_kw)


def oat_knot_selection(cov_par_start, cov_fun, xu_start, proposal_fun, xy, y, ff, mu, muu_start,
                       m=1.0, family="poisson", opt=None, verbose=False, ctx=None, rng=None,
                       proposal_kw=None):
    """oat_knot_selection (R/oat_knot_selection.R:14-306): the same for the Laplace fit of a
    Poisson (exposure m) or Bernoulli response.  ff: the first fit's start for the mode; later
    fits start from the accepted fmax (l.230).  A NotPositiveDefinite ascent is the reference's
    try-error branch (l.241-246): the previous fit stays and ``success`` is False."""
    from .drivers import laplace_grad_ascent
    o = merge_opt(OPT_OAT, opt)
    xy, y, mu, xu, muu = _prepare(xy, y, mu, xu_start, muu_start, np.mean)
    ctx = _own_context(ctx, xy, y, mu, o, xu)
    prop = _resolve_proposal(proposal_fun)
    kw = dict(proposal_kw or {})
    if rng is not None:
        kw.setdefault("rng", rng)
    takes_family = prop in (P.knot_prop_ego, P.knot_prop_random)

    def fit(cov_par, U, knot_opt, dknot, muu_now, ff_now):
        return laplace_grad_ascent(cov_par, cov_fun, True, _dknot(cov_fun) if dknot else None,
                                   knot_opt, U, xy, y, ff_now, mu, muu_now, m, o, verbose, ctx,
                                   family)

    def propose(fit_res):
        extra = {"m": m, "family": family} if takes_family else {}
        return prop(fit_res, o, y=y, ctx=ctx, **extra, **kw)

    out = oat_core(fit, propose, OrderedDict(cov_par_start), xu, muu, o, laplace=True, ff=ff,
                   verbose=verbose)
    out.update({"cov_fun": cov_fun, "mu": mu})
    return out
