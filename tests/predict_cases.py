"""Shared inputs of the prediction tests -- TEST INFRASTRUCTURE ONLY (not a test module).

``mp_fixture(name)``: the two small problems on which prediction is pinned to 50-digit mpmath
(tests/test_mpmath.py holds the fp64 oracle to them, tests/test_gpu_predict_edges.py the GPU):
m = 24 knots, 8 prediction rows of which rows 0 and 1 equal knots exactly, d = 3 sqexp and d = 2
ARD.  The knot posteriors are the oracle's own: ``vi_posterior_u`` of a 60-row Gaussian
regression (VI and the gaussian family of predict_laplace) and ``newtrap_sparseGP``'s posterior
of a 60-row Poisson regression (any other family); the full GP is the 24 knots as data.

``mp_predict(name, method, full_cov)``: the mpmath result (oracle/mp_ref.py), computed once.
``METHODS``: the four prediction calls, as (name, oracle / GPU dispatcher).
"""
import math
from collections import OrderedDict

import numpy as np

from oracle import sgp_oracle as O

DELTA = 1e-6
MP_FIXTURES = {
    "sqexp_d3": ("sqexp", 3, OrderedDict(sigma=1.2, l=1.9, tau=0.6)),
    "ard_d2": ("ard", 2, OrderedDict(sigma=1.1, l1=1.6, l2=2.4, tau=0.5)),
}
METHODS = ("vi", "lap_gauss", "lap_nongauss", "gp_full")
_FIX, _MP = {}, {}


def mp_fixture(name, n=60, m=24, npred=8):
    if name in _FIX:
        return _FIX[name]
    cov_fun, d, cp = MP_FIXTURES[name]
    rng = np.random.default_rng(4 + d)
    X = rng.uniform(0, 10, (n, d))
    U = rng.uniform(0, 10, (m, d))
    xp = rng.uniform(-1, 11, (npred, d))            # some rows outside the knots' box
    xp[0], xp[1] = U[5], U[17]
    y = np.sin(X).sum(1) / math.sqrt(d) + rng.normal(0, 0.3, n)
    mu = np.full(n, y.mean())
    muu = np.full(m, y.mean())
    um, uv = O.vi_posterior_u(cp, cov_fun, U, X, y, mu, muu, DELTA)
    lam = np.exp(0.5 * np.sin(X).sum(1) / math.sqrt(d) + math.log(2))
    yp = rng.poisson(lam).astype(float)
    mup = np.full(n, math.log(yp.mean()))
    muu_p = np.full(m, mup[0])
    nr = O.newtrap_sparseGP(mup.copy(), cp, cov_fun, X, U, yp, mup, 1.0, DELTA, tol=1e-8,
                            muu=muu_p)
    yu = np.sin(U).sum(1) / math.sqrt(d) + rng.normal(0, 0.3, m)   # full GP: data at the knots
    _FIX[name] = dict(
        cov_fun=cov_fun, cov_par=cp, U=U, xp=xp, delta=DELTA,
        mu_pred=0.2 + 0.1 * np.cos(np.arange(npred)),
        gauss=dict(u_mean=um, u_var=uv, muu=muu),
        nongauss=dict(u_mean=nr["u_posterior_mean"], u_var=nr["u_posterior_variance"], muu=muu_p),
        full=dict(y=yu, mu=np.full(m, yu.mean())))
    return _FIX[name]


def call(mod, method, F, full_cov, family_name="poisson"):
    """One prediction of fixture / case F (keys as mp_fixture's) by `mod`, which is the fp64
    oracle, oracle.mp_ref or the sparsergps_amd package (their signatures agree but for where
    delta sits, hence keywords)."""
    cf, cp, U, xp, mup, dl = (F["cov_fun"], F["cov_par"], F["U"], F["xp"], F["mu_pred"],
                              F["delta"])
    if method == "gp_full":
        return mod.predict_gp_full(U, F["full"]["y"], xp, cf, cp, F["full"]["mu"], mup,
                                   full_cov=full_cov, delta=dl)
    P = F["nongauss" if method == "lap_nongauss" else "gauss"]
    if method == "vi":
        return mod.predict_vi(P["u_mean"], P["u_var"], U, xp, cf, cp, mup, P["muu"],
                              full_cov=full_cov, delta=dl)
    fam = "gaussian" if method == "lap_gauss" else family_name
    return mod.predict_laplace(P["u_mean"], P["u_var"], U, xp, cf, cp, mup, P["muu"],
                               full_cov=full_cov, family=fam, delta=dl)


def mp_predict(name, method, full_cov):
    from oracle import mp_ref as M
    key = (name, method, bool(full_cov))
    if key not in _MP:
        _MP[key] = call(M, method, mp_fixture(name), full_cov)
    return _MP[key]
