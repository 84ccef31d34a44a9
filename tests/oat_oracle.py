"""numpy oracle for the OAT knot selection layer: the variance / error scan of knot_prop_var and
knot_prop_error (R/knot_proposal_functions.R:4-42), the random proposals
(R/vi_functions.R:2108-2311) and the OAT loop (R/vi_functions.R:1340-1579,
R/oat_knot_selection.R:14-548), composed from oracle/sgp_oracle.py::predict_laplace,
oracle/drivers.py and tests/ego_oracle.py.  numpy only."""
import math

import numpy as np

import ego_oracle as E
from oracle import sgp_oracle as O


# ------------------------------------------------------------------ the variance / error scan
def fit_scan(xy, mu, cov_par, cov_fun, xu, u_mean, u_var, muu, mode, family, f=None, excl=None,
             delta=1e-6):
    """predict_laplace(full_cov = FALSE) at x_pred = xy, mu = the fit's mean
    (R/knot_proposal_functions.R:10-17, 30-37), the key (l.18: the variance; l.38:
    |exp(f) - exp(mean)|) and which.max over the rows not in excl (the reference excludes none)."""
    xy = np.asarray(xy, dtype=np.float64)
    pr = O.predict_laplace(u_mean, u_var, xu, xy, cov_fun, cov_par, mu, muu, full_cov=False,
                           family=family, delta=delta)
    mean = np.asarray(pr["pred_mean"], dtype=np.float64).reshape(-1)
    var = np.asarray(pr["pred_var"], dtype=np.float64).reshape(-1)
    key = np.abs(np.exp(np.asarray(f, dtype=np.float64)) - np.exp(mean)) if mode == "error" else var
    ex = E.excluded_rows(xy, excl)
    return {"mean": mean, "var": var, "key": np.where(ex, np.nan, key), "key_all": key,
            "excluded": ex, "row": E.which_max(key, ex)}


def _cross(x, u, cov_par, cov_fun):
    sig2 = float(cov_par["sigma"]) ** 2
    if cov_fun == "ard":
        ls = np.array([float(cov_par[f"l{c + 1}"]) for c in range(x.shape[1])])
    else:
        ls = np.full(x.shape[1], float(cov_par["l"]))
    diff = (x[:, None, :] - u[None, :, :]) / ls[None, None, :]
    return sig2 * np.exp(-0.5 * (diff * diff).sum(axis=2))


def fit_scan_dense(xy, mu, cov_par, cov_fun, xu, u_mean, u_var, muu, family, delta=1e-6):
    """The same mean and variance written out densely through a Cholesky factor of K22:
    mean = mu + K12 w, var_i = sigma^2 + tau^2 - k_i^T (K22^-1 - K22^-1 u_var K22^-1) k_i."""
    xy, xu = np.asarray(xy, dtype=np.float64), np.asarray(xu, dtype=np.float64)
    m = xu.shape[0]
    sig2, tau2 = float(cov_par["sigma"]) ** 2, float(cov_par["tau"]) ** 2
    K22 = _cross(xu, xu, cov_par, cov_fun)
    K22[np.diag_indices(m)] = sig2 + (delta if family == "gaussian" else tau2 + delta)
    K12 = _cross(xy, xu, cov_par, cov_fun)
    L = np.linalg.cholesky(K22)
    B = np.linalg.solve(L.T, np.linalg.solve(L, K12.T))          # K22^-1 K21, m x n
    w = np.linalg.solve(L.T, np.linalg.solve(L, np.asarray(u_mean) - np.asarray(muu)))
    mean = np.asarray(mu, dtype=np.float64) + K12 @ w
    var = sig2 + tau2 - (K12.T * B).sum(axis=0) + (B * (np.asarray(u_var) @ B)).sum(axis=0)
    return {"mean": mean, "var": var}


def scan_recipe(n, d, m, cov_fun, seed=0):
    """The scan tests' data: X ~ U(0, 10)^(n x d) with rng = default_rng(1000 n + 10 m + seed);
    knots = the first min(m, n) rows of X (uniform points beyond n); length scales of order the
    mean knot spacing so that K22 stays well conditioned; a smooth mean function, a random
    u_mean near it and an SPD u_var."""
    rng = np.random.default_rng(1000 * n + 10 * m + seed)
    X = rng.uniform(0.0, 10.0, size=(n, d))
    xu = X[:m].copy() if m <= n else np.vstack([X, rng.uniform(0.0, 10.0, size=(m - n, d))])
    base = 1.2 * math.sqrt(d) * 10.0 / (2.0 * max(m, 2) ** (1.0 / d))
    base = min(max(base, 0.3), 4.0 * math.sqrt(d))
    if cov_fun == "ard":
        cov_par = {"sigma": 1.3, **{f"l{c + 1}": base * (0.7 + 0.6 * c / max(d - 1, 1))
                                    for c in range(d)}, "tau": 0.4}
    else:
        cov_par = {"sigma": 1.3, "l": base, "tau": 0.4}
    mu = 0.3 + 0.1 * np.cos(X[:, 0])
    muu = np.full(m, 0.3)
    u_mean = muu + np.sin(xu).sum(axis=1) / math.sqrt(d) + rng.normal(0.0, 0.05, size=m)
    Bm = rng.normal(size=(m, m))
    u_var = 0.05 * (Bm @ Bm.T) / m + 0.01 * np.eye(m)
    f = mu + np.sin(X).sum(axis=1) / math.sqrt(d) + rng.normal(0.0, 0.3, size=n)
    return {"X": X, "xu": xu, "cov_par": cov_par, "mu": mu, "muu": muu, "u_mean": u_mean,
            "u_var": u_var, "f": f}


# ------------------------------------------------------------------ proposals
def scan_proposal(fit, mode):
    """knot_prop_var / knot_prop_error as the code intends (R/knot_proposal_functions.R:4-42):
    predict_laplace with ITS defaults family = "gaussian", delta = 1e-6 (the call passes
    neither), and the data row of the largest key.  Returns (1 x d row, the scan)."""
    xy = np.asarray(fit["xy"], dtype=np.float64)
    res = fit_scan(xy, fit["mu"], fit["cov_par"], fit["cov_fun"], fit["xu"], fit["u_mean"],
                   fit["u_var"], fit["muu"], mode, "gaussian", f=fit.get("fmax"), delta=1e-6)
    return xy[res["row"]].reshape(1, -1).copy(), res


def make_scorer(kind, fit, y, delta, m=1.0, tol_nr=1e-5, maxit_nr=1000):
    """The objective at knots [xu; candidate] for each candidate row: the ELBO ("vi",
    vi_functions.R:2246-2251), obj_fun_norm ("fitc") or newtrap_sparseGP's last objective value
    started from the fit's fmax ("laplace", knot_proposal_functions.R:1120-1133, 1162).  NaN =
    the reference's try-error."""
    xy, xu, cp, cf, mu = fit["xy"], np.asarray(fit["xu"]), fit["cov_par"], fit["cov_fun"], fit["mu"]

    def score(cand):
        out = []
        for c in np.asarray(cand, dtype=np.float64).reshape(-1, xu.shape[1]):
            U = np.vstack([xu, c])
            try:
                if kind == "vi":
                    v = O.elbo_eval(cp, cf, U, xy, y, mu, delta)
                elif kind == "fitc":
                    v = O.fitc_obj_eval(cp, cf, U, xy, y, mu, delta)
                else:
                    muu = np.append(fit["muu"], np.asarray(fit["muu"]).reshape(-1)[0])
                    nr = O.newtrap_sparseGP(np.asarray(fit["fmax"]).copy(), cp, cf, xy, U, y, mu,
                                            m, delta, maxit_nr, tol_nr, muu=muu)
                    v = nr["objective_function_values"][-1]
            except np.linalg.LinAlgError:
                v = math.nan
            out.append(float(v))
        return np.array(out)
    return score


def random_proposal(xy, xu, scorer, last_obj, TTmax, rng=None, init_rows=None, trace=None):
    """knot_prop_random_norm_vi's body (vi_functions.R:2188-2309): TTmax rows outside the knots,
    each scored; values = c(rep(last_obj, m), scores), x = rbind(xu, rows), which.max -- so the
    FIRST KNOT comes back when no candidate beats the current objective strictly."""
    xy, xu = np.asarray(xy, dtype=np.float64), np.asarray(xu, dtype=np.float64)
    d = xy.shape[1]
    pool = np.flatnonzero(~E.excluded_rows(xy, xu))                                  # l.2199-2207
    if init_rows is None:
        init_rows = rng.choice(pool, size=TTmax, replace=False)                      # l.2209
    prop = xy[np.asarray(init_rows)].copy()
    vals = np.zeros(TTmax)
    first = scorer(prop)
    for i in range(TTmax):                                                           # l.2213
        v = float(first[i])
        while math.isnan(v):                                                         # l.2254
            prop[i] = xy[pool[rng.integers(pool.size)]] + rng.normal(0.0, 1e-6, size=d)
            v = float(scorer(prop[i].reshape(1, d))[0])
        vals[i] = v
    all_vals = np.concatenate([np.full(xu.shape[0], last_obj), vals])                # l.2188, 2300
    all_x = np.vstack([xu, prop])                                                    # l.2302
    if trace is not None:
        s = np.sort(vals)
        trace.append({"vals": vals.copy(), "last": float(last_obj),
                      "gap": float(min(abs(s[-1] - last_obj), s[-1] - s[-2] if TTmax > 1 else math.inf))})
    return all_x[int(np.argmax(all_vals))].reshape(1, d)                             # l.2308-2309


# ------------------------------------------------------------------ the OAT loop
def oracle_fit(kind, cov_fun, xy, y, mu, o, m=1.0):
    """fit(cov_par, xu, knot_opt, dknot, muu, ff) over oracle/drivers.py; the whole merged opt o
    goes to the driver, which merges it by name into its own defaults."""
    from oracle import drivers as OD
    dk = "ard" if cov_fun == "ard" else "sqexp"

    def fit(cov_par, xu, knot_opt, dknot, muu, ff):
        kw = {"dcov_fun_dknot": dk if dknot else None, "knot_opt": knot_opt, "opt": o}
        if kind == "vi":
            return OD.norm_grad_ascent_vi(cov_par, cov_fun, xu, xy, y, mu, muu, **kw)
        if kind == "fitc":
            return OD.norm_grad_ascent(cov_par, cov_fun, xu, xy, y, mu, muu, **kw)
        return OD.laplace_grad_ascent(cov_par, cov_fun, xu, xy, y, ff, mu, muu, m, **kw)
    return fit


def oat_loop(fit, propose, cov_par_start, xu_start, muu_start, o, laplace=False, ff=None,
             margins=None):
    """The reference's loop, line by line in R's 1-based bookkeeping (vi_functions.R:1447-1577;
    oat_knot_selection.R:131-304).  margins (a list) receives every accept / reject margin
    (current - previous - tol_knot)."""
    chooseK, cov_diff, tol_knot, maxknot = o["chooseK"], o["cov_diff"], o["tol_knot"], o["maxknot"]
    obj_fun_vals, ga_steps = {}, {}
    cov_par_vals = [np.array(list(cov_par_start.values()), dtype=np.float64)]        # l.1451
    xu, muu = np.array(xu_start, dtype=np.float64), np.array(muu_start, dtype=np.float64)
    opt = fit(cov_par_start, xu, None, False, muu, ff)                               # l.1460-1470
    current = opt["obj_fun"][-1]                                                     # l.1472
    obj_fun_vals[1] = current
    cov_par_vals.append(np.array(list(opt["cov_par"].values()), dtype=np.float64))   # l.1474
    cov_par = opt["cov_par"]
    ga_steps[1] = opt["iter"]
    fmax = None
    if laplace:                                                  # oat_knot_selection.R:180-182
        fmax, muu, xu = opt["fmax"], np.asarray(opt["muu"], dtype=np.float64), opt["xu"]
    upost = {1: (opt["u_mean"], opt["u_var"])}                                       # l.1480
    numknots, it, success = np.shape(xu_start)[0], 1, True
    while (numknots < maxknot and (len(obj_fun_vals) == 1 or
                                   current - obj_fun_vals[len(obj_fun_vals) - 1] > tol_knot)
           if chooseK else numknots < maxknot):                                      # l.1485-1489
        it += 1
        knot_prop = propose(opt)                                                     # l.1500
        knot_opt = [xu.shape[0] + 1] if cov_diff else None                           # l.1516-1518
        try:
            new = fit(cov_par, np.vstack([xu, knot_prop]), knot_opt, bool(cov_diff),
                      np.append(muu, muu[0]), fmax)                                  # l.1509-1525
            opt, success = new, True
        except np.linalg.LinAlgError:
            if not laplace:
                raise
            success = False                                      # oat_knot_selection.R:241-246
        ga_steps[it] = opt["iter"]                                                   # l.1526
        current = opt["obj_fun"][-1]
        obj_fun_vals[it] = current
        margin = current - obj_fun_vals[len(obj_fun_vals) - 1]
        if margins is not None:
            margins.append(float(margin - tol_knot))
        if (margin > tol_knot) if chooseK else True:                                 # l.1531-1534
            cov_par_vals.append(np.array(list(opt["cov_par"].values()), dtype=np.float64))
            if laplace:
                fmax = opt["fmax"]
            upost[it] = (opt["u_mean"], opt["u_var"])
            xu = opt["xu"]
            muu = np.append(muu, muu[0])                                             # l.1542
            cov_par = opt["cov_par"]
            numknots = xu.shape[0]
    on_max = numknots == maxknot                                                     # l.1550
    um, uv = upost[it] if on_max else upost[it - 1]
    out = {"cov_par": cov_par, "xu": xu, "obj_fun": np.array([obj_fun_vals[k] for k in range(1, it + 1)]),
           "u_mean": um, "u_var": uv, "muu": muu, "cov_par_history": np.vstack(cov_par_vals),
           "ga_steps": np.array([ga_steps[k] for k in range(1, it + 1)]),
           "shape": "upost" if on_max else "u_post"}
    if laplace:
        out.update({"fmax": fmax, "success": success})
    return out
