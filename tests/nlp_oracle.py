"""Oracles for the held-out scores (sparsergps_amd.evaluation, sgp_nlp).

Three independent statements of the reference's my_nlp (R/evaluation_functions.R:12-145):

* ``model_nlp``: a numpy model of the algorithm of sparsergps_amd/csrc/sgp_quad.h (mode by
  bracketed Newton, level-set end points, 128-point midpoint rule in log space);
* ``mp_nlp``: the integral at 50 digits with mpmath, the range split at the mode +- {0.1, 1, 3,
  10, 60} s, mpmath's own error estimate checked;
* ``literal_nlp``: my_nlp as written -- the integrand in linear space (dbinom / dpois times dnorm)
  handed to QUADPACK's QAGI through scipy.integrate.quad with R integrate()'s tolerances
  (rel.tol = abs.tol = .Machine$double.eps^0.25, subdivisions = 100), and norm.logpdf for the
  gaussian family -- together with my_kl and my_rmse as written (the n x n diag included).
"""
import math

import numpy as np

N_QUAD = 128
C_LEVEL = 36.0
MODE_ITERS = 60
EDGE_ITERS = 80
R_TOL = np.finfo(np.float64).eps ** 0.25   # integrate()'s rel.tol = abs.tol


# ------------------------------------------------------------------ numpy model of sgp_quad.h
def _delta(pois, ysg, mu, is2, f0, aux0, t, want_slope=False):
    """h(f0 + t) - h(f0) (and its derivative in t); ysg = y (poisson) or +-1 (bernoulli)."""
    gq = -t * (t + 2.0 * (f0 - mu)) * (0.5 * is2)
    gs = -(t + (f0 - mu)) * is2
    with np.errstate(over="ignore", invalid="ignore"):
        em = np.expm1(t)
        dp = ysg * t - aux0 * em + gq
        z = ysg * (f0 + t)
        e = np.exp(-np.abs(z))
        db = (np.minimum(z, 0.0) - np.log1p(e)) - aux0 + gq
        d = np.where(pois, dp, db)
        if not want_slope:
            return d
        sp = ysg - aux0 * (em + 1.0) + gs
        sb = ysg * np.where(z >= 0.0, e, 1.0) / (1.0 + e) + gs
    return d, np.where(pois, sp, sb)


def _dh(pois, ysg, mu, is2, logm, f):
    with np.errstate(over="ignore", invalid="ignore"):
        lam = np.exp(f + logm)
        z = ysg * f
        e = np.exp(-np.abs(z))
        q = 1.0 / (1.0 + e)
        d1 = np.where(pois, ysg - lam, ysg * np.where(z >= 0.0, e * q, q)) - (f - mu) * is2
        d2 = np.where(pois, -lam, -e * q * q) - is2
    return d1, d2


def model_nlp(family, y, pred_mean, pred_var, par=1.0, expo=None):
    """nlp per row by the algorithm of sgp_quad.h.  par: tau (gaussian) / exposure m (poisson)."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    mu = np.asarray(pred_mean, dtype=np.float64).reshape(-1)
    s2 = np.asarray(pred_var, dtype=np.float64).reshape(-1)
    n = y.size
    if family == "gaussian":
        v = s2 + par * par
        ok = np.isfinite(mu) & np.isfinite(v) & (v > 0)
        vv = np.where(ok, v, 1.0)
        z = (y - np.where(ok, mu, 0.0)) / np.sqrt(vv)
        return np.where(ok, 0.5 * np.log(2.0 * np.pi * vv) + 0.5 * z * z, np.nan)
    pois = np.full(n, family == "poisson")
    ok = np.isfinite(mu) & np.isfinite(s2) & (s2 > 0)
    mu_ = np.where(ok, mu, 0.0)
    s2_ = np.where(ok, s2, 1.0)
    is2 = 1.0 / s2_
    if family == "poisson":
        m = np.broadcast_to(np.asarray(par if expo is None else expo, dtype=np.float64), (n,))
        logm = np.log(m)
        ysg = y
        lconst = -np.array([math.lgamma(v + 1.0) for v in y])
        with np.errstate(divide="ignore"):
            fy = np.log(y) - logm
        lo = np.where(y > 0, np.minimum(mu_, fy), mu_ - s2_ * np.exp(mu_ + logm))
        hi = np.where(y > 0, np.maximum(mu_, fy), mu_)
    else:
        logm = np.zeros(n)
        ysg = np.where(y > 0.5, 1.0, -1.0)
        lconst = np.zeros(n)
        lo, hi = mu_ - s2_, mu_ + s2_
    # (a) the mode
    f = np.clip(mu_, lo, hi)
    lo, hi = lo.copy(), hi.copy()
    live = np.ones(n, dtype=bool)
    for _ in range(MODE_ITERS):
        d1, d2 = _dh(pois, ysg, mu_, is2, logm, f)
        live &= d1 != 0.0
        up = live & (d1 > 0.0)
        dn = live & ~(d1 > 0.0)
        lo = np.where(up, f, lo)
        hi = np.where(dn, f, hi)
        fn = f - d1 / d2
        fn = np.where((fn > lo) & (fn < hi), fn, 0.5 * (lo + hi))
        step = np.abs(fn - f)
        f = np.where(live, fn, f)
        live &= ~((step <= 1e-14 * (1.0 + np.abs(f))) | ~(hi > lo))
        if not live.any():
            break
    f0 = f
    with np.errstate(over="ignore"):
        z0 = ysg * f0
        lp0 = np.where(pois, ysg * (f0 + logm) - np.exp(f0 + logm),
                       np.minimum(z0, 0.0) - np.log1p(np.exp(-np.abs(z0))))
        aux0 = np.where(pois, np.exp(f0 + logm), lp0)
    h0 = lp0 + lconst - (f0 - mu_) * (f0 - mu_) * (0.5 * is2)
    span = np.sqrt(2.0 * C_LEVEL * s2_)

    # (b) the level-set points
    def edge(t0):
        t = t0.copy()
        live = np.ones(n, dtype=bool)
        for _ in range(EDGE_ITERS):
            d, sl = _delta(pois, ysg, mu_, is2, f0, aux0, t, True)
            g = d + C_LEVEL
            live &= (g < -1e-3) & (sl != 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                tn = t - g / sl
            inward = np.where(t0 > 0, (tn < t) & (tn > 0), (tn > t) & (tn < 0))
            live &= inward
            t = np.where(live, tn, t)
            if not live.any():
                break
        return t

    ta, tb = edge(-span), edge(span)
    w = (tb - ta) / N_QUAD
    total = np.zeros(n)
    for k in range(N_QUAD):
        total += np.exp(_delta(pois, ysg, mu_, is2, f0, aux0, ta + (k + 0.5) * w))
    nlp = -(h0 + np.log(total) + np.log(w) - 0.5 * np.log(2.0 * np.pi * s2_))
    return np.where(ok, nlp, np.nan)


# ------------------------------------------------------------------ 50-digit truth
def mp_nlp(family, y, mu, s2, m=1.0, tau=0.0, rel_bar=1e-25):
    """One row's nlp at 50 digits; raises if mpmath's error estimate exceeds rel_bar."""
    import mpmath as mp
    with mp.workdps(50):
        y, mu, s2, m, tau = (mp.mpf(float(v)) for v in (y, mu, s2, m, tau))
        if family == "gaussian":
            v = s2 + tau * tau
            return float(mp.log(2 * mp.pi * v) / 2 + (y - mu) ** 2 / (2 * v))
        if family == "poisson":
            def lp(f):
                return y * (f + mp.log(m)) - m * mp.exp(f) - mp.loggamma(y + 1)

            def dh(f):
                return y - m * mp.exp(f) - (f - mu) / s2
        else:
            sg = 1 if y > 0.5 else -1

            def lp(f):
                return -mp.log1p(mp.exp(-sg * f))

            def dh(f):
                return sg / (1 + mp.exp(sg * f)) - (f - mu) / s2

        def h(f):
            return lp(f) - (f - mu) ** 2 / (2 * s2)

        # the mode: bisection on the decreasing h' inside a generous bracket
        s = mp.sqrt(s2)
        lo, hi = mu - s2 * (1 + y) - 1, mu + s2 * (1 + y) + 1
        for _ in range(400):
            mid = (lo + hi) / 2
            if dh(mid) > 0:
                lo = mid
            else:
                hi = mid
        fh = (lo + hi) / 2
        h0 = h(fh)
        offs = [0.1, 1, 3, 10, 60]
        pts = [fh - k * s for k in reversed(offs)] + [fh] + [fh + k * s for k in offs]
        val, err = mp.quad(lambda f: mp.exp(h(f) - h0), pts, error=True, maxdegree=14)
        if not err <= rel_bar * val:
            raise ArithmeticError(f"mpmath quad error estimate {err} (value {val}) for "
                                  f"{family} y={y} mu={mu} s2={s2} m={m}")
        # tails beyond 60 s: below exp(-1800) of the peak (h'' <= -1/s2)
        return float(-(h0 + mp.log(val) - mp.log(2 * mp.pi * s2) / 2))


# ------------------------------------------------------------------ the reference as written
def my_logistic(x):
    return 1.0 / (1.0 + np.exp(-x))


def literal_nlp(family, y, pred_mean, pred_var, par=None):
    """my_nlp(mc = FALSE, mv = FALSE) as written; returns the nlp vector (non-finite where
    integrate()'s rule returns 0 or a negative value)."""
    from scipy import integrate, stats
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    pred_mean = np.asarray(pred_mean, dtype=np.float64).reshape(-1)
    pred_var = np.asarray(pred_var, dtype=np.float64).reshape(-1)
    if family == "gaussian":
        return -stats.norm.logpdf(y, loc=pred_mean, scale=np.sqrt(pred_var + par["tau"] ** 2))
    nlp = np.empty(y.size)
    for i in range(y.size):
        if family == "bernoulli":
            def g(ff, i=i):
                ll = stats.binom.pmf(y[i], 1, my_logistic(ff))
                return ll * stats.norm.pdf(ff, loc=pred_mean[i], scale=math.sqrt(pred_var[i]))
        else:
            def g(ff, i=i):
                lam = np.exp(ff) * par["m"]
                # R: exp(ff) overflows to Inf and dpois(x, Inf) is 0
                ll = stats.poisson.pmf(y[i], lam) if np.isfinite(lam) else 0.0
                return ll * stats.norm.pdf(ff, loc=pred_mean[i], scale=math.sqrt(pred_var[i]))
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with np.errstate(all="ignore"):
                val = integrate.quad(g, -np.inf, np.inf, epsabs=R_TOL, epsrel=R_TOL, limit=100)[0]
                nlp[i] = -np.log(val) if val == val else np.nan
    return nlp


def literal_rmse(pred, actual):
    pred, actual = np.asarray(pred, dtype=np.float64), np.asarray(actual, dtype=np.float64)
    return math.sqrt(np.mean((pred - actual) ** 2))


def literal_kl(mean1, mean2, sigma1, sigma2):
    """my_kl(mv = FALSE) as written (R/evaluation_functions.R:165-173)."""
    mean1, mean2, sigma1, sigma2 = (np.asarray(v, dtype=np.float64).reshape(-1)
                                    for v in (mean1, mean2, sigma1, sigma2))
    dm = (mean2 - mean1).reshape(-1, 1)
    quad = (dm.T @ (np.diag(1.0 / sigma2) @ dm))[0, 0]
    return 0.5 * (np.sum(sigma1 / sigma2) + quad - mean1.size + np.sum(np.log(sigma2))
                  - np.sum(np.log(sigma1)))


# ------------------------------------------------------------------ the fixture's grid
GRID_MU = (-6.0, -2.0, -0.3, 0.0, 1.5, 6.0)
GRID_S2 = (1e-6, 1e-3, 0.05, 0.7, 4.0, 25.0)


def grid_cases():
    """The 612-case grid followed by the three named rows: arrays fam (0 poisson, 1 bernoulli),
    y, mu, s2, m."""
    rows = []
    for mu in GRID_MU:
        for s2 in GRID_S2:
            for yv in (0.0, 1.0):
                rows.append((1, yv, mu, s2, 1.0))
    for mu in GRID_MU:
        for s2 in GRID_S2:
            for yv in (0.0, 1.0, 3.0, 17.0, 200.0):
                for m in (0.5, 1.0, 20.0):
                    rows.append((0, yv, mu, s2, m))
    assert len(rows) == 612
    rows.append((1, 1.0, -0.3, 1e-6, 1.0))      # the confident bernoulli row
    rows.append((0, 200.0, -6.0, 0.7, 1.0))     # nlp 96.516468834...
    rows.append((0, 5000.0, 0.0, 1.0, 1.0))     # the integral underflows a double
    a = np.array(rows, dtype=np.float64)
    return a[:, 0].astype(np.int64), a[:, 1], a[:, 2], a[:, 3], a[:, 4]


FAMILY_NAMES = {0: "poisson", 1: "bernoulli", 2: "gaussian"}
