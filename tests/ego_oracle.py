"""numpy restatement of the reference's EGO knot proposal (test helper, no GPU, no product code).

The scan: R/vi_functions.R:1927-1950 (repeated at 2074-2097 and in
R/knot_proposal_functions.R:355-379, 457-478, 832-855, 964-985).  The loop around it:
R/vi_functions.R:1584-2104.  ``scan_literal`` follows the reference's per-row solve loop line by
line; ``scan`` is the vectorised form the GPU tests compare against, with the magnitude budgets
their tolerances are built from.
"""
import math

import numpy as np

_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def cross_cov(x, xp, sigma, l, cov_fun):
    """make_cov_matC(x, x_pred) in cross mode: no nugget, even on a coincident pair
    (src/covariance_functionsC.cpp:72-169; "exp" = L1 distance, l.45-52; "sqexp" l.5-20)."""
    diff = x[:, None, :] - xp[None, :, :]
    if cov_fun == "exp":
        return sigma ** 2 * np.exp(-np.abs(diff).sum(axis=2) / l)
    if cov_fun == "sqexp":
        return sigma ** 2 * np.exp(-(diff * diff).sum(axis=2) / (2.0 * l * l))
    raise ValueError(cov_fun)


def sym_cov(x, sigma, l, tau, delta, cov_fun):
    """make_cov_matC(x, x_pred = matrix()): tau^2 + delta added to the diagonal."""
    return cross_cov(x, x, sigma, l, cov_fun) + (tau ** 2 + delta) * np.eye(x.shape[0])


def pnorm(z):
    """Phi(z) = erfc(-z / sqrt 2) / 2 (accurate in the lower tail, unlike (1 + erf) / 2)."""
    return 0.5 * _erfc(-np.asarray(z, dtype=np.float64) / math.sqrt(2.0))


def dnorm(z):
    z = np.asarray(z, dtype=np.float64)
    return np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def expected_improvement(mean, var, vmax, tau):
    """vi_functions.R:1938-1943: EI where var > tau^2 (strictly; false for NaN), else 0."""
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    ei = np.zeros_like(mean)
    with np.errstate(invalid="ignore"):
        on = var > tau ** 2
    sd = np.sqrt(var[on])
    z = (mean[on] - vmax) / sd
    ei[on] = sd * (z * pnorm(z) + dnorm(z))
    return ei


def excluded_rows(X, excl):
    """xy_setminus_xu's complement (vi_functions.R:1679-1687): rows of X equal (==) to a row of
    excl in every coordinate."""
    out = np.zeros(X.shape[0], dtype=bool)
    if excl is None or len(excl) == 0:
        return out
    excl = np.asarray(excl, dtype=np.float64).reshape(-1, X.shape[1])
    for u in excl:
        out |= (X == u[None, :]).all(axis=1)
    return out


def which_max(ei, excluded=None):
    """R's which.max over the non-excluded rows, as a 0-based index into all rows: NaN is
    ignored, the first of equal maxima wins, all zero gives the first row.  -1: nothing left."""
    ei = np.asarray(ei, dtype=np.float64)
    ok = ~np.isnan(ei)
    if excluded is not None:
        ok &= ~excluded
    idx = np.flatnonzero(ok)
    if idx.size == 0:
        return -1
    return int(idx[np.argmax(ei[idx])])   # argmax: first occurrence


def scan_literal(X, xm, vals, par, cov_fun, delta, excl=None):
    """The reference's text, row by row (vi_functions.R:1927-1950); delta is the caller's,
    delta / 1000 goes to K22 (l.1927-1928)."""
    sigma, l, tau = par["sigma"], par["l"], par["tau"]
    K12 = cross_cov(X, xm, sigma, l, cov_fun)                                        # l.1927
    K22 = sym_cov(xm, sigma, l, tau, delta / 1000.0, cov_fun)                        # l.1928
    pred = vals[0] + K12 @ np.linalg.solve(K22, vals - vals[0])                      # l.1930
    n = X.shape[0]
    var, ei = np.zeros(n), np.zeros(n)
    for i in range(n):                                                               # l.1934
        var[i] = sigma ** 2 + tau ** 2 - K12[i] @ np.linalg.solve(K22, K12[i])       # l.1936
        if var[i] > tau ** 2:                                                        # l.1938
            z = (pred[i] - vals.max()) / math.sqrt(var[i])                           # l.1940
            ei[i] = math.sqrt(var[i]) * (z * 0.5 * math.erfc(-z / math.sqrt(2.0))
                                         + math.exp(-0.5 * z * z) / math.sqrt(2 * math.pi))
        else:
            ei[i] = 0.0                                                              # l.1943
    ex = excluded_rows(X, excl)
    return {"mean": pred, "var": var, "ei": np.where(ex, np.nan, ei), "excluded": ex,
            "row": which_max(ei, ex)}                                                # l.1950


def scan(X, xm, vals, par, cov_fun, delta, excl=None):
    """The same, vectorised, plus what the GPU tests' bounds need: A = K22^-1, alpha, cond(K22)
    and the magnitude budgets s_mean = |v1| + sum |k_ij| |alpha_j|,
    s_var = sigma^2 + tau^2 + sum |k_ij| |A_jk| |k_ik|."""
    X = np.asarray(X, dtype=np.float64)
    xm = np.asarray(xm, dtype=np.float64).reshape(-1, X.shape[1])
    vals = np.asarray(vals, dtype=np.float64)
    sigma, l, tau = par["sigma"], par["l"], par["tau"]
    K12 = cross_cov(X, xm, sigma, l, cov_fun)
    K22 = sym_cov(xm, sigma, l, tau, delta / 1000.0, cov_fun)
    A = np.linalg.inv(K22)
    A = 0.5 * (A + A.T)
    alpha = np.linalg.solve(K22, vals - vals[0])
    mean = vals[0] + K12 @ alpha
    var = sigma ** 2 + tau ** 2 - np.einsum("ij,jk,ik->i", K12, A, K12)
    ei = expected_improvement(mean, var, vals.max(), tau)
    ex = excluded_rows(X, excl)
    aK = np.abs(K12)
    return {"mean": mean, "var": var, "ei": np.where(ex, np.nan, ei), "ei_all": ei,
            "excluded": ex, "row": which_max(ei, ex), "cond": float(np.linalg.cond(K22)),
            "s_mean": abs(vals[0]) + aK @ np.abs(alpha),
            "s_var": sigma ** 2 + tau ** 2 + np.einsum("ij,jk,ik->i", aK, np.abs(A), aK),
            "z": (mean - vals.max()) / np.sqrt(np.where(var > 0, var, np.nan))}


def ei_bound(ref, sigma, rel=1e-8):
    """Per-row bound on |EI - EI_ref| for mean and var within rel * budget: the propagated
    Phi(z) rel s_mean + phi(z) / (2 sqrt var) rel s_var + rel max EI_ref, and the mask of rows
    it applies to (var_ref >= 1e-3 sigma^2, not excluded)."""
    on = (ref["var"] >= 1e-3 * sigma ** 2) & ~ref["excluded"]
    z = np.where(on, ref["z"], 0.0)
    sd = np.sqrt(np.where(on, ref["var"], 1.0))
    b = pnorm(z) * rel * ref["s_mean"] + dnorm(z) / (2.0 * sd) * rel * ref["s_var"] \
        + rel * np.nanmax(ref["ei"])
    return b, on


def top_two_gap(ei):
    """(best - second) / best over the finite entries (inf with fewer than two)."""
    v = np.sort(ei[~np.isnan(ei)])
    if v.size < 2 or v[-1] == 0.0:
        return math.inf if v.size < 2 else 0.0
    return float((v[-1] - v[-2]) / v[-1])


def recipe(n, d, T):
    """The GPU tests' data: rng = default_rng(1000 n + T); X ~ U(0, 10)^(n x d); Xm = T distinct
    rows of X (uniform points when T > n); v = -50 + 3 sum_c sin(xm_c) / sqrt d + N(0, 0.1)."""
    rng = np.random.default_rng(1000 * n + T)
    X = rng.uniform(0.0, 10.0, size=(n, d))
    xm = X[rng.choice(n, size=T, replace=False)] if T <= n else rng.uniform(0.0, 10.0, size=(T, d))
    v = -50.0 + 3.0 * np.sin(xm).sum(axis=1) / math.sqrt(d) + rng.normal(0.0, 0.1, size=T)
    return X, xm.copy(), v


# ------------------------------------------------------------------ the meta-model fit
def meta_nll(par, x, vals, cov_fun, tau, delta):
    """meta_mod_obj_fun (vi_functions.R:1791-1828): mu = vals[1] (R index), delta not / 1000."""
    sigma, l = math.exp(par[0]), math.exp(par[1])                                    # l.1803
    L = np.linalg.cholesky(sym_cov(x, sigma, l, tau, delta, cov_fun))                # l.1817-1822
    w = np.linalg.solve(L, vals - vals[0])
    return float(np.log(np.diag(L)).sum() + 0.5 * w @ w)                             # l.1825


def meta_grad(par, x, vals, cov_fun, tau, delta):
    """meta_mod_grad (vi_functions.R:1849-1905) with dexp_dsigma / dexp_dl, transform = TRUE
    (R/covariance_function_derivatives.R:326-357, 401-432): L2 distance inside, against the L1
    values of the "exp" kernel (quirk Q12)."""
    sigma, l = math.exp(par[0]), math.exp(par[1])
    L = np.linalg.cholesky(sym_cov(x, sigma, l, tau, delta, cov_fun))                # l.1885
    diff = x[:, None, :] - x[None, :, :]
    r = np.sqrt((diff * diff).sum(axis=2))
    if cov_fun == "exp":
        dS = [2 * sigma * np.exp(-r / l) * sigma,                                    # R l.344
              sigma ** 2 * np.exp(-r / l) * (r / l ** 2) * l]                        # R l.419
    else:
        e = sigma ** 2 * np.exp(-r * r / (2 * l * l))
        dS = [2 * e, e * r * r / l ** 3 * l]
    a = np.linalg.solve(L.T, np.linalg.solve(L, vals - vals[0]))
    g = np.zeros(2)
    for p in range(2):                                                               # l.1888
        g[p] = -(-0.5 * np.trace(np.linalg.solve(L.T, np.linalg.solve(L, dS[p])))
                 + 0.5 * a @ dS[p] @ a)                                              # l.1898-1900
    return g


def fallback(x, vals):
    """vi_functions.R:1919."""
    return np.array([math.log(vals.max() - vals.min()), math.log((x.max() - x.min()) / 1000.0)])


# ------------------------------------------------------------------ the proposal loop
def proposal_loop(xy, xu, scorer, o, rng=None, init_rows=None, meta_fit=None, trace=None):
    """knot_prop_ego_norm_vi's body (vi_functions.R:1679-2102) with the scorer, the meta fit and
    the randomness passed in: scorer(k x d candidates) -> values (NaN = try-error);
    meta_fit(x, vals, start, cov_fun, tau, delta) -> (log sigma, log l), an exception or a
    non-finite value = try-error.  Every scan the reference runs is run (TTmax - TTmin + 1; the
    last one's result is never read) and recorded in trace."""
    d = xy.shape[1]
    TTmin, TTmax, delta = o["TTmin"], o["TTmax"], o["delta"]
    par = dict(o["ego_cov_par"])
    cov_fun = o["ego_cov_fun"]
    pool = np.flatnonzero(~excluded_rows(xy, xu))                                    # l.1679-1687

    def resample():                                                                  # l.1738-1739
        return xy[pool[rng.integers(pool.size)]] + rng.normal(0.0, 1e-6, size=d)

    def score(prop):                                                                 # l.1729-1778
        val = float(np.asarray(scorer(prop.reshape(1, d))).reshape(-1)[0])
        while math.isnan(val):
            prop = resample()
            val = float(np.asarray(scorer(prop.reshape(1, d))).reshape(-1)[0])
        return prop, val

    if init_rows is None:
        init_rows = rng.choice(pool, size=TTmin, replace=False)                      # l.1690
    obj_x = xy[np.asarray(init_rows)].copy()
    vals = np.zeros(TTmin)
    for i in range(TTmin):                                                           # l.1694
        obj_x[i], vals[i] = score(obj_x[i].copy())

    def refit_and_scan():
        nonlocal par
        start = np.log([par["sigma"], par["l"]])                                     # l.1908
        try:
            p = np.asarray(meta_fit(obj_x, vals, start, cov_fun, par["tau"], delta), dtype=float)
            if not np.all(np.isfinite(p)):
                raise FloatingPointError
        except Exception:                                                            # l.1915-1920
            p = fallback(obj_x, vals)
        par = {"sigma": math.exp(p[0]), "l": math.exp(p[1]), "tau": par["tau"]}      # l.1922-1924
        res = scan(xy, obj_x, vals, par, cov_fun, delta, excl=xu)                    # l.1927-1945
        if trace is not None:
            trace.append({"row": res["row"], "cov_par": dict(par), "T": vals.size,
                          "gap": top_two_gap(res["ei"])})
        return res["row"]

    row = refit_and_scan()
    it = TTmin                                                                       # l.1946
    while it < TTmax:                                                                # l.1947
        prop, val = score(xy[row].copy())                                            # l.1950-2049
        vals = np.append(vals, val)                                                  # l.2051
        obj_x = np.vstack([obj_x, prop])                                             # l.2054
        row = refit_and_scan()                                                       # l.2057-2092
        it += 1                                                                      # l.2096
    return obj_x[int(np.argmax(vals))].reshape(1, d)                                 # l.2101-2102
