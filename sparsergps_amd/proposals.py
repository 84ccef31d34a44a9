"""Knot proposals: the reference's ``xu_opt = "oat"`` / ``"random"`` proposal functions

  knot_prop_ego_norm_vi   R/vi_functions.R:1584-2104              (VI, scorer = the ELBO)
  knot_prop_ego_norm      R/knot_proposal_functions.R:498-999     (FITC, obj_fun_norm)
  knot_prop_ego           R/knot_proposal_functions.R:46-495      (Laplace, newtrap_sparseGP)
  knot_prop_random*       R/vi_functions.R:2108-2311; R/knot_proposal_functions.R:1001-1365
  knot_prop_var / _error  R/knot_proposal_functions.R:4-42        (at the end of this module)

The EGO proposals first.

All three are the same loop (``_ego_core``): score TTmin random data rows as an added knot, fit a
small meta-model GP to (candidate, objective) pairs, scan every data row outside the knots for
the largest expected improvement, score that row, refit, ... until TTmax candidates are scored;
the best scored candidate is returned.  The two O(n) steps run on the device: the scorers are
``SparseGPContext.vi_candidates`` / ``fitc_candidates`` / ``lap_candidates`` and the scan is
``SparseGPContext.ego_scan`` (sgp_ego_scan).  The T <= 128 point meta-model fit runs on the host.

Differences from the reference, all deliberate:
  * randomness is injected (``rng``, a numpy Generator, for the reference's sample.int / rnorm
    draws; ``init_rows`` may fix the first TTmin rows) -- never global state, and the draws are
    numpy's, not R's;
  * the meta-model fit is a ``meta_fit`` callable; the default minimises the reference's
    meta_mod_obj_fun with its meta_mod_grad by BFGS through scipy.  Iterate-for-iterate parity
    with R's optim() is NOT claimed: both are BFGS on the same function and gradient, but their
    line searches and stopping rules differ;
  * data rows that duplicate earlier data rows stay in the pool the first TTmin rows are drawn
    from (the reference's duplicated() drops them); the winner's coordinates cannot depend on it;
  * the scan after the last refit, whose result the reference never reads
    (vi_functions.R:2074-2097 at iter = TTmax - 1), is not run.
"""
from __future__ import annotations

import math

import numpy as np

# the reference's opt defaults (vi_functions.R:1606-1616; knot_proposal_functions.R:522-528, 74-80)
_OPT_COMMON = {"optim_method": "adadelta", "decay": 0.95, "epsilon": 1e-6, "learn_rate": 1e-2,
               "eta": 0.8, "maxit": 1000, "obj_tol": 1e-3, "maxit_nr": 1000, "delta": 1e-6,
               "maxknot": 30, "TTmin": 10, "TTmax": 40,
               "ego_cov_par": {"sigma": 3.0, "l": 1.0, "tau": 0.0}, "ego_cov_fun": "exp"}
OPT_EGO_NORM_VI = {**_OPT_COMMON, "grad_tol": math.inf, "tol_knot": 1e-3, "tol_nr": 1e-5}
OPT_EGO_NORM = dict(OPT_EGO_NORM_VI)
OPT_EGO = {**_OPT_COMMON, "grad_tol": 1e-1, "tol_knot": 1e-1, "tol_nr": 1e-4}


def _merge_opt(master, opt):
    """The reference's loop over names(opt): unknown names are skipped silently."""
    o = {k: (dict(v) if isinstance(v, dict) else v) for k, v in master.items()}
    for k, v in (opt or {}).items():
        if k in o:
            o[k] = dict(v) if isinstance(v, dict) else v
    return o


# ------------------------------------------------------------------ the meta-model's likelihood
def _meta_dists(x):
    diff = x[:, None, :] - x[None, :, :]
    return np.abs(diff).sum(axis=2), np.sqrt((diff * diff).sum(axis=2))


def _meta_sigma(x, sigma, l, tau, delta, cov_fun):
    """make_cov_matC(x, x_pred = matrix()): k(x, x) + (tau^2 + delta) I
    (src/covariance_functionsC.cpp:72-169; "exp" is the L1 form, l.45-52)."""
    l1, l2 = _meta_dists(x)
    if cov_fun == "exp":
        K = sigma * sigma * np.exp(-l1 / l)
    elif cov_fun == "sqexp":
        K = sigma * sigma * np.exp(-(l2 * l2) / (2.0 * l * l))
    else:
        raise ValueError(f"ego_cov_fun must be 'exp' or 'sqexp', not {cov_fun!r}")
    return K + (tau * tau + delta) * np.eye(x.shape[0])


def meta_mod_obj_fun(par, x, vals, cov_fun, tau, delta):
    """meta_mod_obj_fun (R/vi_functions.R:1791-1828): the meta-model GP's negative log
    likelihood at par = (log sigma, log l), mean mu = vals[0], tau fixed:
    sum(log(diag(L))) + 1/2 |L^-1 (vals - mu)|^2 with L = t(chol(Sig))."""
    x = np.asarray(x, dtype=np.float64).reshape(len(vals), -1)
    vals = np.asarray(vals, dtype=np.float64)
    sigma, l = math.exp(par[0]), math.exp(par[1])
    L = np.linalg.cholesky(_meta_sigma(x, sigma, l, tau, delta, cov_fun))
    w = np.linalg.solve(L, vals - vals[0])
    return float(np.sum(np.log(np.diag(L))) + 0.5 * (w @ w))


def meta_mod_grad(par, x, vals, cov_fun, tau, delta):
    """meta_mod_grad (R/vi_functions.R:1849-1905) with dexp_dsigma / dexp_dl as
    ego_cov_fun_dtheta (transform = TRUE): d nll / d (log sigma, log l).

    Quirk Q12, second appearance: for the "exp" kernel the VALUES use the L1 distance
    (covariance_functionsC.cpp:45-52) but the reference's derivative functions use the L2
    distance sqrt(sum((x1 - x2)^2)) (R/covariance_function_derivatives.R:326-432):
        dSig/dlog sigma = 2 sigma^2 exp(-|.|_2 / l),  dSig/dlog l = sigma^2 exp(-|.|_2 / l) |.|_2 / l
    so this is the gradient of the objective only at d = 1.  Reproduced as written."""
    x = np.asarray(x, dtype=np.float64).reshape(len(vals), -1)
    vals = np.asarray(vals, dtype=np.float64)
    sigma, l = math.exp(par[0]), math.exp(par[1])
    Sig = _meta_sigma(x, sigma, l, tau, delta, cov_fun)
    L = np.linalg.cholesky(Sig)
    _, l2 = _meta_dists(x)
    if cov_fun == "exp":
        e = sigma * sigma * np.exp(-l2 / l)
        dS = (2.0 * e, e * l2 / l)
    else:   # dsqexp_dsigma / dsqexp_dl (covariance_function_derivatives.R:7-155)
        e = sigma * sigma * np.exp(-(l2 * l2) / (2.0 * l * l))
        dS = (2.0 * e, e * (l2 * l2) / (l * l))
    a = np.linalg.solve(L.T, np.linalg.solve(L, vals - vals[0]))
    g = np.zeros(2)
    for p in range(2):
        tr = np.trace(np.linalg.solve(L.T, np.linalg.solve(L, dS[p])))
        g[p] = -(-0.5 * tr + 0.5 * (a @ dS[p] @ a))
    return g


def meta_fit_fallback(x, vals):
    """The reference's values when optim() fails (vi_functions.R:1915-1920):
    (log(max v - min v), log((max x - min x) / 1000))."""
    x, vals = np.asarray(x, dtype=np.float64), np.asarray(vals, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.array([np.log(vals.max() - vals.min()), np.log((x.max() - x.min()) / 1000.0)])


def meta_fit_bfgs(x, vals, start, cov_fun, tau, delta):
    """optim(par = start, fn = meta_mod_obj_fun, gr = meta_mod_grad, method = "BFGS")
    (vi_functions.R:1908-1911) through scipy.optimize.minimize.  Not iterate-for-iterate R's
    optim: the same function and gradient, another line search and stopping rule."""
    from scipy.optimize import minimize   # lazy: only the default fit needs scipy
    res = minimize(meta_mod_obj_fun, np.asarray(start, dtype=np.float64), jac=meta_mod_grad,
                   args=(x, vals, cov_fun, tau, delta), method="BFGS")
    return res.x


def _fit_meta(meta_fit, x, vals, start, cov_fun, tau, delta):
    """One refit; any failure or non-finite result takes the reference's fallback."""
    try:
        par = np.asarray(meta_fit(x, vals, start, cov_fun, tau, delta), dtype=np.float64)
        if par.shape != (2,) or not np.all(np.isfinite(par)) or not np.all(np.isfinite(np.exp(par))):
            raise FloatingPointError("non-finite meta-model parameters")
    except Exception:   # R: class(temp_opt) == "try-error"
        par = meta_fit_fallback(x, vals)
    return par


# ------------------------------------------------------------------ the shared loop
def rows_outside_knots(xy, xu):
    """Indices of the rows of xy that equal no row of xu in all coordinates (the reference's
    xy_setminus_xu, vi_functions.R:1679-1687, without its removal of repeated data rows)."""
    xy = np.asarray(xy, dtype=np.float64)
    xu = np.asarray(xu, dtype=np.float64).reshape(-1, xy.shape[1])
    hit = np.flatnonzero(np.isin(xy[:, 0], xu[:, 0]))
    if hit.size:
        same = (xy[hit][:, None, :] == xu[None, :, :]).all(axis=2).any(axis=1)
        keep = np.ones(xy.shape[0], dtype=bool)
        keep[hit[same]] = False
        return np.flatnonzero(keep)
    return np.arange(xy.shape[0])


def ego_proposal(xy, xu, scorer, scan, o, rng=None, init_rows=None, meta_fit=None, trace=None):
    """The loop shared by the three proposals.  scorer(cand) -> objective values of the k x d
    candidate knots (NaN = the reference's try-error); scan(cov_par, cov_fun, x, vals) -> the
    0-based data row of largest expected improvement outside the knots.  ``trace`` (a list)
    receives one dict per scan: the row, the meta-model's parameters and its size."""
    xy = np.asarray(xy, dtype=np.float64)
    xy = xy.reshape(xy.shape[0], -1)
    d = xy.shape[1]
    xu = np.asarray(xu, dtype=np.float64).reshape(-1, d)
    TTmin, TTmax = int(o["TTmin"]), int(o["TTmax"])
    if not 1 <= TTmin <= TTmax <= 128:
        raise ValueError(f"need 1 <= TTmin <= TTmax <= 128 (TTmin={TTmin}, TTmax={TTmax})")
    cov_fun = o["ego_cov_fun"]
    par = dict(o["ego_cov_par"])
    tau, delta = float(par["tau"]), float(o["delta"])
    meta_fit = meta_fit or meta_fit_bfgs
    pool = None

    def resample():
        # xy_setminus_xu[sample.int(n, 1), ] + rnorm(d, 0, 1e-6)  (vi_functions.R:1738-1739)
        nonlocal pool
        if rng is None:
            raise ValueError("the scorer failed on a candidate and no rng was given to resample")
        if pool is None:
            pool = rows_outside_knots(xy, xu)
        return xy[pool[rng.integers(pool.size)]] + rng.normal(0.0, 1e-6, size=d)

    def score_one(prop):
        val = float(np.asarray(scorer(prop.reshape(1, d))).reshape(-1)[0])
        while math.isnan(val):
            prop = resample()
            val = float(np.asarray(scorer(prop.reshape(1, d))).reshape(-1)[0])
        return prop, val

    if init_rows is None:
        if rng is None:
            raise ValueError("give rng (a numpy Generator) or init_rows")
        pool = rows_outside_knots(xy, xu)
        if pool.size < TTmin:
            raise ValueError(f"{pool.size} data rows outside the knots, TTmin = {TTmin}")
        init_rows = rng.choice(pool, size=TTmin, replace=False)   # sample.int, l.1690
    init_rows = np.asarray(init_rows, dtype=np.int64).reshape(-1)
    if init_rows.size != TTmin:
        raise ValueError(f"init_rows has {init_rows.size} rows, TTmin = {TTmin}")
    obj_x = xy[init_rows].copy()
    vals = np.asarray(scorer(obj_x), dtype=np.float64).reshape(-1).copy()
    for i in np.flatnonzero(np.isnan(vals)):   # in order, as the reference's loop resamples
        obj_x[i], vals[i] = score_one(resample())

    it = TTmin
    while True:
        start = np.log([par["sigma"], par["l"]])
        fit = _fit_meta(meta_fit, obj_x, vals, start, cov_fun, tau, delta)
        par = {"sigma": float(np.exp(fit[0])), "l": float(np.exp(fit[1])), "tau": tau}
        if it >= TTmax:
            break
        row = int(scan(par, cov_fun, obj_x, vals))
        if trace is not None:
            trace.append({"row": row, "cov_par": dict(par), "T": int(vals.size)})
        prop, val = score_one(xy[row].copy())
        obj_x = np.vstack([obj_x, prop])
        vals = np.append(vals, val)
        it += 1
    # obj_fun_x[which.max(obj_fun_vals), ] as a 1 x d matrix (vi_functions.R:2101-2102)
    return obj_x[int(np.argmax(vals))].reshape(1, d).copy()


def _fit_parts(fit):
    from .covariance import theta_vector
    xy = np.asarray(fit["xy"], dtype=np.float64)
    xy = xy.reshape(xy.shape[0], -1)
    d = xy.shape[1]
    xu = np.asarray(fit["xu"], dtype=np.float64).reshape(-1, d)
    cov_fun = fit["cov_fun"]
    lnames = [f"l{c + 1}" for c in range(d)] if cov_fun == "ard" else None
    return xy, xu, cov_fun, theta_vector(fit["cov_par"], cov_fun, d, lnames)


def _context(ctx, fit, xy, xu, y):
    if ctx is not None:
        if ctx.m_max < xu.shape[0] + 1:
            raise ValueError(f"the context holds {ctx.m_max} knots; a proposal scores "
                             f"{xu.shape[0] + 1}")
        return ctx
    if y is None:
        raise ValueError("give y or a SparseGPContext over (xy, y, mu)")
    from .vi import SparseGPContext
    return SparseGPContext(xy, y, fit["mu"], m_max=xu.shape[0] + 1)


def _run(fit, master, opt, ctx, y, make_scorer, rng, init_rows, meta_fit, trace):
    o = _merge_opt(master, opt)
    xy, xu, cov_fun, theta = _fit_parts(fit)
    ctx = _context(ctx, fit, xy, xu, y)
    scorer = make_scorer(ctx, o, theta, cov_fun, xu)

    def scan(par, ego_cov_fun, x, vals):
        return ctx.ego_scan(par, ego_cov_fun, x, vals, excl=xu, delta=o["delta"], want=())["row"]

    return ego_proposal(xy, xu, scorer, scan, o, rng, init_rows, meta_fit, trace)


def knot_prop_ego_norm_vi(norm_opt, opt=None, *, y=None, ctx=None, rng=None, init_rows=None,
                          meta_fit=None, trace=None):
    """knot_prop_ego_norm_vi (R/vi_functions.R:1584-2104): the EGO proposal of one more knot
    for a VI fit.  norm_opt: the fit (``norm_grad_ascent_vi``'s result: xu, cov_par, cov_fun, xy,
    mu); opt: overrides of OPT_EGO_NORM_VI; y or ctx (a SparseGPContext over the fit's xy, y, mu
    with room for one more knot).  Returns the 1 x d proposed knot."""
    def make(ctx, o, theta, cov_fun, xu):
        return lambda cand: ctx.vi_candidates(theta, cov_fun, xu, cand, o["delta"])
    return _run(norm_opt, OPT_EGO_NORM_VI, opt, ctx, y, make, rng, init_rows, meta_fit, trace)


def knot_prop_ego_norm(norm_opt, opt=None, *, y=None, ctx=None, rng=None, init_rows=None,
                       meta_fit=None, trace=None):
    """knot_prop_ego_norm (R/knot_proposal_functions.R:498-999): the same for a FITC fit
    (``norm_grad_ascent``; scorer obj_fun_norm at [xu; candidate])."""
    def make(ctx, o, theta, cov_fun, xu):
        return lambda cand: ctx.fitc_candidates(theta, cov_fun, xu, cand, o["delta"])
    return _run(norm_opt, OPT_EGO_NORM, opt, ctx, y, make, rng, init_rows, meta_fit, trace)


def knot_prop_ego(laplace_opt, opt=None, *, y=None, ctx=None, m=1.0, family="poisson", rng=None,
                  init_rows=None, meta_fit=None, trace=None):
    """knot_prop_ego (R/knot_proposal_functions.R:46-495): the same for a Laplace fit
    (``laplace_grad_ascent``; scorer = the last objective value of newtrap_sparseGP at
    [xu; candidate] started from the fit's fmax, with opt's tol_nr / maxit_nr).  m: the Poisson
    exposure; family: "poisson" or "bernoulli"."""
    def make(ctx, o, theta, cov_fun, xu):
        ctx.lap_set_family(family)
        ctx.lap_set_f(laplace_opt["fmax"])
        return lambda cand: ctx.lap_candidates(theta, cov_fun, xu, cand, o["delta"], m,
                                               o["tol_nr"], o["maxit_nr"])
    return _run(laplace_opt, OPT_EGO, opt, ctx, y, make, rng, init_rows, meta_fit, trace)


# ------------------------------------------------------------------ the random proposals
# knot_prop_random_norm_vi (R/vi_functions.R:2108-2311), knot_prop_random_norm and
# knot_prop_random (R/knot_proposal_functions.R:1176-1365, 1001-1171): TTmax random data rows
# outside the knots, each scored as an added knot; no meta-model, and no TTmin.
# opt defaults: vi_functions.R:2132-2135; knot_proposal_functions.R:1200-1203, 1030-1033
_OPT_RANDOM = {"optim_method": "adadelta", "decay": 0.95, "epsilon": 1e-6, "learn_rate": 1e-2,
               "eta": 0.8, "maxit": 1000, "obj_tol": 1e-3, "grad_tol": 1e-1, "maxit_nr": 1000,
               "delta": 1e-6, "tol_knot": 1e-1, "maxknot": 30, "TTmax": 40}
OPT_RANDOM_NORM_VI = dict(_OPT_RANDOM)
OPT_RANDOM_NORM = dict(_OPT_RANDOM)
OPT_RANDOM = {**_OPT_RANDOM, "tol_nr": 1e-4}


def random_proposal(xy, xu, scorer, last_obj, o, rng=None, init_rows=None, trace=None):
    """The loop shared by the three random proposals.  scorer(cand) -> objective values of the
    k x d candidate knots (NaN = the reference's try-error); last_obj: the fit's last objective
    value.  All TTmax first draws are scored in one scorer call; a NaN is resampled as the
    reference resamples it (a random row outside the knots plus N(0, 1e-6^2) noise).

    The return value is the reference's, quirk included (vi_functions.R:2188, 2302-2309): the
    value vector starts with m copies of last_obj and obj_fun_x = rbind(xu, pseudo_prop), so
    which.max returns the best candidate only if it beats the current objective strictly --
    otherwise index 1, the FIRST EXISTING KNOT xu[0].  ``trace`` (a list) receives
    {"rows", "vals", "best"}."""
    xy = np.asarray(xy, dtype=np.float64)
    xy = xy.reshape(xy.shape[0], -1)
    d = xy.shape[1]
    xu = np.asarray(xu, dtype=np.float64).reshape(-1, d)
    TTmax = int(o["TTmax"])
    pool = rows_outside_knots(xy, xu)
    if init_rows is None:
        if rng is None:
            raise ValueError("give rng (a numpy Generator) or init_rows")
        if pool.size < TTmax:
            raise ValueError(f"{pool.size} data rows outside the knots, TTmax = {TTmax}")
        init_rows = rng.choice(pool, size=TTmax, replace=False)   # sample.int, l.2209
    init_rows = np.asarray(init_rows, dtype=np.int64).reshape(-1)
    if init_rows.size != TTmax:
        raise ValueError(f"init_rows has {init_rows.size} rows, TTmax = {TTmax}")
    prop = xy[init_rows].copy()
    vals = np.asarray(scorer(prop), dtype=np.float64).reshape(-1).copy()
    for i in np.flatnonzero(np.isnan(vals)):   # in order, as the reference's loop resamples
        while math.isnan(vals[i]):             # l.2254-2297
            if rng is None:
                raise ValueError("the scorer failed on a candidate and no rng was given to resample")
            prop[i] = xy[pool[rng.integers(pool.size)]] + rng.normal(0.0, 1e-6, size=d)
            vals[i] = float(np.asarray(scorer(prop[i].reshape(1, d))).reshape(-1)[0])
    all_vals = np.concatenate([np.full(xu.shape[0], float(last_obj)), vals])   # l.2188, 2300
    all_x = np.vstack([xu, prop])                                              # l.2302
    best = int(np.argmax(all_vals))                                            # which.max
    if trace is not None:
        trace.append({"rows": init_rows.copy(), "vals": vals.copy(), "best": best})
    return all_x[best].reshape(1, d).copy()


def _run_random(fit, master, opt, ctx, y, make_scorer, rng, init_rows, trace):
    o = _merge_opt(master, opt)
    xy, xu, cov_fun, theta = _fit_parts(fit)
    ctx = _context(ctx, fit, xy, xu, y)
    scorer = make_scorer(ctx, o, theta, cov_fun, xu)
    last = np.asarray(fit["obj_fun"], dtype=np.float64).reshape(-1)[-1]
    return random_proposal(xy, xu, scorer, last, o, rng, init_rows, trace)


def knot_prop_random_norm_vi(norm_opt, opt=None, *, y=None, ctx=None, rng=None, init_rows=None,
                             trace=None):
    """knot_prop_random_norm_vi (R/vi_functions.R:2108-2311): the best of TTmax random data rows
    as one more knot of a VI fit (scorer = the ELBO at [xu; candidate]); see random_proposal for
    the return value.  norm_opt needs xu, cov_par, cov_fun, xy, mu and obj_fun."""
    def make(ctx, o, theta, cov_fun, xu):
        return lambda cand: ctx.vi_candidates(theta, cov_fun, xu, cand, o["delta"])
    return _run_random(norm_opt, OPT_RANDOM_NORM_VI, opt, ctx, y, make, rng, init_rows, trace)


def knot_prop_random_norm(norm_opt, opt=None, *, y=None, ctx=None, rng=None, init_rows=None,
                          trace=None):
    """knot_prop_random_norm (R/knot_proposal_functions.R:1176-1365): the same for a FITC fit
    (scorer obj_fun_norm at [xu; candidate])."""
    def make(ctx, o, theta, cov_fun, xu):
        return lambda cand: ctx.fitc_candidates(theta, cov_fun, xu, cand, o["delta"])
    return _run_random(norm_opt, OPT_RANDOM_NORM, opt, ctx, y, make, rng, init_rows, trace)


def knot_prop_random(laplace_opt, opt=None, *, y=None, ctx=None, m=1.0, family="poisson",
                     rng=None, init_rows=None, trace=None):
    """knot_prop_random (R/knot_proposal_functions.R:1001-1171): the same for a Laplace fit
    (scorer = the last objective value of newtrap_sparseGP at [xu; candidate] started from the
    fit's fmax, with opt's tol_nr / maxit_nr)."""
    def make(ctx, o, theta, cov_fun, xu):
        ctx.lap_set_family(family)
        ctx.lap_set_f(laplace_opt["fmax"])
        return lambda cand: ctx.lap_candidates(theta, cov_fun, xu, cand, o["delta"], m,
                                               o["tol_nr"], o["maxit_nr"])
    return _run_random(laplace_opt, OPT_RANDOM, opt, ctx, y, make, rng, init_rows, trace)


# ------------------------------------------------------------------ the variance / error proposals
def _scan_proposal(fit, mode, ctx, y, exclude_knots, trace):
    xy = np.asarray(fit["xy"], dtype=np.float64)
    xy = xy.reshape(xy.shape[0], -1)
    xu = np.asarray(fit["xu"], dtype=np.float64).reshape(-1, xy.shape[1])
    if ctx is None:
        if y is None:
            raise ValueError("give y or a SparseGPContext over (xy, y, mu)")
        from .vi import SparseGPContext
        ctx = SparseGPContext(xy, y, fit["mu"], m_max=xu.shape[0])
    # the reference's call passes neither family nor delta (knot_proposal_functions.R:10-17,
    # 30-37): predict_laplace's defaults, family = "gaussian" and delta = 1e-6, apply to every fit
    res = ctx.fit_scan(fit["cov_par"], fit["cov_fun"], xu, fit["u_mean"], fit["u_var"], fit["muu"],
                       mode, "gaussian", f=fit["fmax"] if mode == "error" else None,
                       excl=xu if exclude_knots else None, delta=1e-6)
    if trace is not None:
        trace.append(dict(res))
    return xy[res["row"]].reshape(1, -1).copy()


def knot_prop_var(laplace_opt, opt=None, *, y=None, ctx=None, exclude_knots=False, trace=None,
                  **_):
    """knot_prop_var (R/knot_proposal_functions.R:4-20): the data row of the largest predictive
    variance of the fit, as a 1 x d matrix, from one pass over the context's resident rows
    (SparseGPContext.fit_scan).  The fit needs xu, cov_par, cov_fun, xy, mu, muu, u_mean, u_var.

    Reference bug, not reproduced: pred_var is an n-vector there and l.18 takes
    diag() of it, which builds an n x n matrix (n^2 doubles) whose which.max index is out of range
    for xy unless row 1 wins.  Here: the row of largest variance, what the code intends.
    exclude_knots=True leaves out rows that are knots already (the reference does not)."""
    return _scan_proposal(laplace_opt, "var", ctx, y, exclude_knots, trace)


def knot_prop_error(laplace_opt, opt=None, *, y=None, ctx=None, exclude_knots=False, trace=None,
                    **_):
    """knot_prop_error (R/knot_proposal_functions.R:24-42): the data row of the largest
    |exp(fmax) - exp(pred_mean)| (l.38, written so for every family), as a 1 x d matrix.  The
    fit also needs fmax."""
    return _scan_proposal(laplace_opt, "error", ctx, y, exclude_knots, trace)
