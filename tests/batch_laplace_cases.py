"""The problems the batched Laplace tests share (tests/test_batch_laplace_model.py,
tests/test_batch_laplace_abi.py, tests/test_gpu_batch_laplace.py): tests/batch_fitc_cases.py's
shapes (MIXED and the two coincident-knot cases) with Poisson counts and Bernoulli classes drawn
from a latent sin surface of moderate amplitude, each drawn once, and the reference results
(newtrap_sparseGP with its stop trace, dlogq_dcov_par, the knot posterior), each computed once.

The seeds are chosen so that, with the oracle's stop trace at TOL from the reference's start, both
stop margins (bern_oracle.stop_margins) of every case are >= 1e-3 and every case takes at least
three NR iterations: a device sum that differs from the oracle's in its last bits then cannot
change an iteration count.  tests/test_batch_laplace_model.py asserts both for every case."""
import functools
import math
from collections import OrderedDict

import numpy as np

import batch_fitc_cases as FC
import bern_oracle as BO
from oracle import sgp_oracle as O

TOL = 1e-6
MAXIT = 1000
FAMILIES = ("poisson", "bernoulli")
# (family, case name) -> seed, where the default (600 + the case's index) does not satisfy the
# rule above
SEEDS = {("poisson", "mixed0"): 900}     # n = 1: seed 600 stops after two updates


def _shapes():
    out = [(f"mixed{i}", n, m, d, cf, False) for i, (n, m, d, cf) in enumerate(FC.MIXED)]
    out += [(f"coincident{m}", n, m, d, cf, True) for n, m, d, cf, _ in FC.COINCIDENT]
    return out


NAMES = [s[0] for s in _shapes()]


@functools.lru_cache(maxsize=None)
def problem(family, name, seed=None):
    """X, U, y, mu, expo (Poisson: not all 1; Bernoulli: None), f0 (the reference's start:
    R/optimize_gp.R:480, 583), cov_par, cov_fun, delta."""
    idx = NAMES.index(name)
    _, n, m, d, cf, coinc = _shapes()[idx]
    if seed is None:
        seed = SEEDS.get((family, name), 600 + idx)
    G = FC.gauss(n, m, d, cf, seed)                  # X, U and theta by the shared recipe
    g = np.random.Generator(np.random.PCG64(seed + 7000))
    X, U = G["X"], G["U"].copy()
    if coinc:
        U = X[:m].copy()
        U[1::2] = G["U"][1::2]                       # half the knots copied from rows
    lat = 0.8 * np.sin(X).sum(axis=1) / math.sqrt(d)
    if family == "poisson":
        expo = g.uniform(0.5, 2.0, size=n)
        y = g.poisson(expo * np.exp(0.7 + lat)).astype(np.float64)
        f0 = np.full(n, math.log(y.mean())) - np.log(expo) if y.mean() > 0 else None
        mu = np.full(n, 0.5)
    else:
        expo = None
        y = (g.uniform(size=n) < 1.0 / (1.0 + np.exp(-2.0 * lat))).astype(np.float64)
        f0 = np.zeros(n)
        mu = np.zeros(n)
    return dict(X=X, U=U, y=y, mu=mu, expo=expo, f0=f0, cov_par=G["cov_par"], cov_fun=cf,
                delta=1e-6, family=family, name=name)


def newtrap(P, f0=None, tol=TOL, maxit=MAXIT, muu=None):
    """The oracle's newtrap_sparseGP for P's family with "stop_trace" (per loop test
    (|obj step|, max |grad psi|)) and "W" (the last update's start W)."""
    f0 = P["f0"] if f0 is None else f0
    cp, cf, X, U, y, mu, dl = (P[k] for k in ("cov_par", "cov_fun", "X", "U", "y", "mu", "delta"))
    if P["family"] == "bernoulli":
        return BO.newtrap_sparseGP(f0, cp, cf, X, U, y, mu, dl, maxit, tol, muu=muu, trace=True)
    # O.newtrap_sparseGP's loop (newtrap_sparseGP.R:6-186) with the stop quantities recorded
    m = P["expo"]
    S12, S22, Z = O.laplace_mats(cp, cf, U, X, dl)
    ff = np.asarray(f0, dtype=np.float64).copy()
    obj = [O.obj_fun_pois(ff, mu, Z, S12, S22, y, m)]
    stops = []
    it = 1
    while True:
        it += 1
        W = O.d2log_py_dff_pois(ff, m)
        gp = O.grad_loglik_fn_pois(ff, y, mu, S12, S22, Z, m)
        ff = O.newtrap_sparseGP_update(ff, W, Z, S12, S22, gp, y, mu, m)
        obj.append(O.obj_fun_pois(ff, mu, Z, S12, S22, y, m))
        stops.append((abs(obj[it - 1] - obj[it - 2]), float(np.max(np.abs(gp)))))
        if not (it < maxit and (abs(obj[it - 1] - obj[it - 2]) > tol or np.any(np.abs(gp) > tol))):
            break
    out = {"gp": ff, "objective_function_values": np.array(obj), "gradient": gp, "W": W,
           "stop_trace": np.array(stops)}
    if muu is not None:
        out["u_posterior_mean"], out["u_posterior_variance"] = O.laplace_posterior_u(
            cp, cf, U, X, y, mu, muu, ff, W, dl)
    return out


def gradient(P, ff):
    """dlogq_dcov_par at ff, in cov_par's key order."""
    cp, cf, X, U, y, mu, dl = (P[k] for k in ("cov_par", "cov_fun", "X", "U", "y", "mu", "delta"))
    if P["family"] == "bernoulli":
        g = BO.dlogq_dcov_par(cp, cf, U, X, y, ff, mu, dl)["gradient"]
    else:
        g = O.dlogq_dcov_par(cp, cf, U, X, y, ff, mu, P["expo"], dl)["gradient"]
    return np.array([g[k] for k in cp])


@functools.lru_cache(maxsize=None)
def reference(family, name):
    """newtrap (muu = 0) from the reference's start, and the gradient at its mode; shared and
    left unchanged by the tests."""
    P = problem(family, name)
    nr = newtrap(P, muu=np.zeros(P["U"].shape[0]))
    return P, nr, gradient(P, nr["gp"])


def all_cases():
    return [(fam, name) for fam in FAMILIES for name in NAMES]
