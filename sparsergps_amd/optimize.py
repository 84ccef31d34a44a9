"""optimize_gp (R/optimize_gp.R:147-753): the reference's public entry -- one call that
dispatches a fit by family x sparse x vi x xu_opt onto the drivers, the full-GP fits and the OAT
knot selection, and returns the ``mod`` that predict_gp / score_gp take.

Quirks:
  Q11  the reference's maxknot check (l.214, 225) reads a GLOBAL ``maxknot``, not opt$maxknot;
       here opt["maxknot"] is read.
  Q10  xu_opt = "simultaneous" passes cov_fun = "sqexp" to the driver whatever the fit's cov_fun
       is (l.320, 399), which fails for "ard" (the cov_par names do not match).  Kept failing,
       with a clear error instead of R's subscript error.
nugget = FALSE (derivative lists without tau, l.242-260) and optim_method = "ga" are refused.
"""
from __future__ import annotations

import math
import pickle

import numpy as np

from . import drivers as _D
from . import full as _F
from . import knot_selection as _K
from . import proposals as _P

# R/optimize_gp.R:166-177
OPT_MASTER = {"optim_method": "adadelta", "decay": 0.95, "epsilon": 1e-6, "learn_rate": 1e-2,
              "eta": 1e3, "maxit": 1000, "obj_tol": 1e-3, "grad_tol": math.inf, "maxit_nr": 1000,
              "delta": 1e-6, "tol_nr": 1e-5, "maxknot": 15, "tol_knot": 1e-3,
              "ego_cov_par": {"sigma": 3.0, "l": 1.0, "tau": 0.0}, "ego_cov_fun": "exp",
              "TTmax": 30, "TTmin": 10, "cov_diff": True, "chooseK": True}
XU_OPTS = ("fixed", "simultaneous", "oat", "random")
ERR_GA = "Error: Basic gradient ascent no longer supported."
ERR_VI = "Error: VI not supported for non-gaussian data."
ERR_MAXKNOT = "Error: Maximum number of knots must be less than the number of data points."
ERR_TT = ("Error: Must adhere to 0 < TTmin < TTmax < N - maxknot. Recommend setting both TTmax "
          "and maxknot < N / 2 or using a full GP.")
ERR_COV = "Error: invalid covariance function"


def optimize_gp(y, xy, cov_fun="sqexp", cov_par_start=None, mu=None, family="gaussian",
                nugget=True, sparse=False, xu_opt=None, xu=None, muu=None, vi=False, opt=None,
                verbose=False, file_path=None, a=None, rng=None, ctx=None, proposal_kw=None):
    """Fit a GP as the reference's optimize_gp does and return {"results", "sparse", "family",
    "delta", "xu_init"} (also pickled to file_path when given).  Error conditions the reference
    reports as strings are returned as those strings.  a: the Poisson exposure (default 1);
    rng: a numpy Generator forwarded to the knot proposals; ctx: a SparseGPContext to reuse."""
    o = {k: (dict(v) if isinstance(v, dict) else v) for k, v in OPT_MASTER.items()}
    if vi and family != "gaussian":                # l.186-189
        return ERR_VI
    for k, v in (opt or {}).items():               # l.192-207: unknown names warned about
        if k in o:
            o[k] = dict(v) if isinstance(v, dict) else v
        elif verbose:
            print("Warning: you supplied an argument to opt() not utilized by this function.")
    # l.180-183: the reference tests this before the merge, where it can never be true; its
    # message says what is meant, so the merged value is tested here
    if o["optim_method"] == "ga":
        return ERR_GA
    if not nugget:
        raise ValueError("nugget = False is not supported: every fit here carries tau")
    if family not in ("gaussian", "poisson", "bernoulli"):
        raise ValueError(f"family must be gaussian, poisson or bernoulli, not {family!r}")
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n = y.size
    if sparse and o["maxknot"] >= n:               # l.214-219, Q11
        return ERR_MAXKNOT
    if xu_opt is not None and xu_opt in ("random", "oat") and (
            o["TTmin"] <= 0 or o["TTmax"] <= o["TTmin"] or o["TTmax"] >= n - o["maxknot"]):
        return ERR_TT                              # l.220-232
    if cov_fun not in ("sqexp", "ard"):            # l.264-268
        return ERR_COV
    xy = np.asarray(xy, dtype=np.float64)
    if xy.ndim == 1:                               # l.270-274
        xy = xy.reshape(-1, 1)
    if cov_par_start is None:
        raise ValueError("cov_par_start is required")
    m_expo = 1.0 if a is None else a               # l.461-468
    if family == "poisson":
        ff0 = np.full(n, math.log(y.mean())) - np.log(m_expo)      # l.480
    else:
        ff0 = np.zeros(n)                                          # l.583

    if sparse:
        if xu_opt not in XU_OPTS:
            raise ValueError(f"xu_opt must be one of {XU_OPTS}, not {xu_opt!r}")
        xu = np.asarray(xu, dtype=np.float64)
        if xu.ndim == 1:                           # l.279-283
            xu = xu.reshape(-1, 1)
        if muu is None or np.size(muu) != xu.shape[0]:             # l.285-289
            muu = np.zeros(xu.shape[0])
        muu = np.asarray(muu, dtype=np.float64).reshape(-1)
        if xu_opt == "simultaneous" and cov_fun == "ard":          # Q10
            raise ValueError('xu_opt = "simultaneous" passes cov_fun = "sqexp" to the driver '
                             '(R/optimize_gp.R:320, 399), which cannot take an "ard" fit\'s '
                             "cov_par; use \"oat\" or \"fixed\"")
        results = _sparse(y, xy, cov_fun, cov_par_start, mu, family, xu_opt, xu, muu, vi, o,
                          verbose, m_expo, ff0, rng, ctx, proposal_kw)
    elif family == "gaussian":                     # l.673-685
        results = _F.norm_grad_ascent_full(cov_par_start, cov_fun, True, xy, y, mu, o, verbose)
    else:                                          # l.687-732
        results = _F.laplace_grad_ascent_full(cov_par_start, cov_fun, True, xy, y, ff0, mu, m_expo,
                                              o, verbose, None, family)
    mod = {"results": results, "sparse": bool(sparse), "family": family, "delta": o["delta"],
           "xu_init": xu}
    if isinstance(file_path, str):                 # l.738-746
        with open(file_path, "wb") as fh:
            pickle.dump(mod, fh)
    return mod


def _sparse(y, xy, cov_fun, cov_par_start, mu, family, xu_opt, xu, muu, vi, o, verbose, m_expo,
            ff0, rng, ctx, proposal_kw):
    dknot = "ard" if cov_fun == "ard" else "sqexp"
    all_knots = list(range(1, xu.shape[0] + 1))
    if family == "gaussian":
        driver = _D.norm_grad_ascent_vi if vi else _D.norm_grad_ascent
        if xu_opt == "fixed":                      # l.299-315, 378-394
            return driver(cov_par_start, cov_fun, True, None, None, xu, xy, y, mu, muu, o, verbose,
                          ctx)
        if xu_opt == "simultaneous":               # l.317-333, 396-412: cov_fun = "sqexp"
            return driver(cov_par_start, "sqexp", True, dknot, all_knots, xu, xy, y, mu, muu, o,
                          verbose, ctx)
        oat = _K.oat_knot_selection_norm_vi if vi else _K.oat_knot_selection_norm
        if xu_opt == "oat":                        # l.335-353, 414-432
            prop = _P.knot_prop_ego_norm_vi if vi else _P.knot_prop_ego_norm
        else:                                      # l.355-373, 434-452
            prop = _P.knot_prop_random_norm_vi if vi else _P.knot_prop_random_norm
        return oat(cov_par_start, cov_fun, xu, prop, xy, y, mu, muu, o, verbose, ctx, rng,
                   proposal_kw)
    if xu_opt == "fixed":                          # l.469-492, 572-594
        return _D.laplace_grad_ascent(cov_par_start, cov_fun, True, None, None, xu, xy, y, ff0, mu,
                                      muu, m_expo, o, verbose, ctx, family)
    if xu_opt == "simultaneous":                   # l.494-516, 596-617
        return _D.laplace_grad_ascent(cov_par_start, "sqexp", True, dknot, all_knots, xu, xy, y,
                                      ff0, mu, muu, m_expo, o, verbose, ctx, family)
    prop = _P.knot_prop_ego if xu_opt == "oat" else _P.knot_prop_random   # l.518-565, 619-665
    return _K.oat_knot_selection(cov_par_start, cov_fun, xu, prop, xy, y, ff0, mu, muu, m_expo,
                                 family, o, verbose, ctx, rng, proposal_kw)
