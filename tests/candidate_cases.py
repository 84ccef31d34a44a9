"""The inputs and CPU references the OAT candidate-scoring edge tests share
(tests/test_candidate_cases.py, which runs without a GPU and checks the inputs themselves, and
tests/test_gpu_candidate_edges.py): fixed PCG64 seeds, every case built once (lru_cache) and left
unchanged by the tests.

A scorer returns, per candidate x*, the objective at the knot set [U; x*]
(sgp_vi_candidates / sgp_fitc_candidates / sgp_lap_candidates, include/sgp.h).  References, in
their order of authority:
  * the literal rebuild: O.elbo_eval / O.fitc_obj_eval / newtrap_sparseGP's last objective at
    np.vstack([U, x*]).  Where the literal Gaussian objective is R's det() underflow (-inf, quirk
    Q4) the adjoint model (oracle.adjoint_ref.eval_vi / eval_fitc) at the same knots stands in;
    the case keeps the literal value ("lit") so the substitution stays visible;
  * oracle.adjoint_ref.vi_candidates, the numpy model of the bordered algebra ("model"), which
    covers every entry of the large-T cases cheaply;
  * oracle.mp_ref.vi_objective (50 digits) for the candidate next to a knot, where both fp64
    routes lose digits (NEAR_KNOT_MODEL_ERR below).
"""
import functools
import math
from collections import OrderedDict

import numpy as np

import batch_fitc_cases as FC
import batch_laplace_cases as LC
import bern_oracle as BO
from oracle import adjoint_ref as A
from oracle import sgp_oracle as O
from sparsergps_amd.workloads import (make_bernoulli_problem, make_gaussian_problem,
                                      make_poisson_problem)

VI_RTOL = 1e-9          # tests/test_gpu_candidates.py's bar for the VI scorer
EVAL_RTOL = 1e-6        # tests/test_gpu_objonly_candidates.py's bar for FITC and Laplace
LAP_TOL = 1e-5          # tol_nr of the Laplace candidate runs
MARGIN_MIN = 1e-3       # both stop margins of every Laplace candidate run

VI_TILE_M = (1, 127, 128, 129, 255, 256, 257)
FITC_TILE_M = (128, 255, 256)
LAP_TILE_M = (127, 128)
ROW_N = (1, 128, 129)
CHUNK_T = (1, 127, 128, 129, 257)
CHUNK_LITERAL = (0, 126, 127, 128, 256)
# (cov_fun, d, n, m): tests/test_gpu_edges.py's high-d shapes and its one-dimensional knot grid
DIMS = (("ard", 12, 600, 40), ("ard", 20, 500, 33), ("ard", 32, 300, 20),
        ("sqexp", 12, 600, 40), ("sqexp", 1, 500, 20))


def theta_of(P):
    return np.array(list(P["cov_par"].values()), dtype=np.float64)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def objective(mode, P, U):
    """(reference, literal) objective of mode "vi" / "fitc" at knots U: the literal oracle's value,
    or the adjoint model's where the literal one is not finite (the callers assert it is -inf)."""
    args = (P["cov_par"], P["cov_fun"], U, P["X"], P["y"], P["mu"], P["delta"])
    lit = O.elbo_eval(*args) if mode == "vi" else O.fitc_obj_eval(*args)
    if np.isfinite(lit):
        return lit, lit
    ev = A.eval_vi if mode == "vi" else A.eval_fitc
    return ev(P["cov_fun"], theta_of(P), P["X"], P["y"], P["mu"], U, P["delta"])[0], lit


def _scored(mode, P, cand, check=None, bad=()):
    """One scorer call's case: ref / lit hold the rebuild at the entries in `check` (all by
    default; NaN elsewhere and at the `bad` entries, the try-errors); VI cases add the bordered
    model at every entry that is not bad."""
    cand = np.asarray(cand, dtype=np.float64).reshape(-1, P["X"].shape[1])
    T = cand.shape[0]
    check = tuple(range(T) if check is None else check)
    ref, lit = np.full(T, np.nan), np.full(T, np.nan)
    for t in check:
        if t not in bad:
            ref[t], lit[t] = objective(mode, P, np.vstack([P["U"], cand[t]]))
    out = dict(P=P, theta=theta_of(P), cand=cand, ref=ref, lit=lit, check=check, bad=tuple(bad))
    if mode == "vi":
        good = [t for t in range(T) if t not in bad]
        model = np.full(T, np.nan)
        model[good] = A.vi_candidates(P["cov_fun"], out["theta"], P["X"], P["y"], P["mu"], P["U"],
                                      cand[good], P["delta"])
        out["model"] = model
    return out


# ----------------------------------------------------------------------------- a. knot tiles
@functools.lru_cache(maxsize=None)
def vi_tile(m):
    """C2-style sqexp, d = 3, n = 300: two candidates from X and one uniform off-data point."""
    P = make_gaussian_problem("C2", n=300, m=m)
    g = _rng(1000 + m)
    cand = np.vstack([P["X"][g.choice(300, size=2, replace=False)], g.uniform(0.0, 10.0, size=(1, 3))])
    return _scored("vi", P, cand)


@functools.lru_cache(maxsize=None)
def fitc_tile(m):
    P = make_gaussian_problem("C2", n=300, m=m)
    out = _scored("fitc", P, P["X"][_rng(1100 + m).choice(300, size=2, replace=False)])
    out["base"], out["base_lit"] = objective("fitc", P, P["U"])
    return out


def _lap_problem(family, n, m, seed=None):
    if family == "poisson":
        P = make_poisson_problem(n=n, m=m)
        P["expo"] = P.pop("a")
    else:
        P = make_bernoulli_problem(n, m, d=2, seed=seed,
                                   cov_par=OrderedDict([("sigma", 1.0), ("l", 2.0), ("tau", 0.1)]))
        P["expo"] = None
    P["family"] = family
    return P


def _lap_scored(P, cand, bad=()):
    """fmax: the oracle's mode at U from the reference's start (the warm start of every candidate);
    per candidate the last NR objective at [U; x*] from fmax and both stop margins."""
    cand = np.asarray(cand, dtype=np.float64).reshape(-1, P["X"].shape[1])
    T = cand.shape[0]
    fmax = LC.newtrap(P, tol=LAP_TOL)["gp"]
    ref, margins = np.full(T, np.nan), np.full((T, 2), np.nan)
    for t in range(T):
        if t in bad:
            continue
        nr = LC.newtrap(dict(P, U=np.vstack([P["U"], cand[t]])), f0=fmax, tol=LAP_TOL)
        ref[t] = nr["objective_function_values"][-1]
        margins[t] = BO.stop_margins(nr["stop_trace"], LAP_TOL)
    return dict(P=P, theta=theta_of(P), cand=cand, ref=ref, fmax=fmax, margins=margins,
                check=tuple(range(T)), bad=tuple(bad))


# candidate rows of X per Laplace case: the first draws (PCG64 seed 1200 + m) whose NR runs keep
# both stop margins >= MARGIN_MIN; tests/test_candidate_cases.py asserts they still do
@functools.lru_cache(maxsize=None)
def lap_tile(family, m):
    n = 300
    P = _lap_problem(family, n, m, seed=14)
    rows = _rng(1200 + m + (0 if family == "poisson" else 50)).choice(n, size=2, replace=False)
    return _lap_scored(P, P["X"][rows])


# ----------------------------------------------------------------------------- b. row edges
@functools.lru_cache(maxsize=None)
def row_edge(mode, n):
    """tests/test_gpu_edges.py's _gauss recipe at m = 7, d = 3; at n = 1 one candidate is the row
    itself and one is not."""
    P = FC.gauss(n, 7, 3, "sqexp", 1300 + n)
    g = _rng(1310 + n)
    if n == 1:
        cand = np.vstack([P["X"][0], g.uniform(0.0, 10.0, size=(1, 3))])
    else:
        cand = P["X"][g.choice(n, size=2, replace=False)]
    return _scored(mode, P, cand)


# ----------------------------------------------------------------------------- c. chunk edges
@functools.lru_cache(maxsize=None)
def _chunk_pool():
    P = make_gaussian_problem("C2", n=200, m=9)
    c = P["X"][_rng(1400).choice(200, size=257, replace=True)].copy()
    c[128] = c[256] = P["X"][_rng(1401).choice(200)]   # the T = 1 call's candidate ends T = 129, 257
    c[130] = c[3]                                      # one candidate twice, in two chunks
    return P, c


@functools.lru_cache(maxsize=None)
def chunk(T):
    """n = 200, m = 9: the first T rows of one pool of candidates drawn from X (T = 1: the row
    that ends the T = 129 and T = 257 calls)."""
    P, c = _chunk_pool()
    cand = c[256:257] if T == 1 else c[:T]
    return _scored("vi", P, cand, check=[t for t in CHUNK_LITERAL if t < T])


# ----------------------------------------------------------------------------- d. dimensions
@functools.lru_cache(maxsize=None)
def dims(mode, cov_fun, d, n, m):
    P = FC.gauss(n, m, d, cov_fun, 1500 + d)          # _gauss_hd's length scales at d > 8
    g = _rng(1510 + d)
    cand = np.vstack([P["X"][g.choice(n, size=2, replace=False)], g.uniform(0.0, 10.0, size=(1, d))])
    return _scored(mode, P, cand)


# ----------------------------------------------------------------------------- e. try-error
TRY_DELTA = -1e-3
TRY_DUP = 3           # the knot the poisoned candidate copies
TRY_BAD = 1           # its position among the candidates


@functools.lru_cache(maxsize=None)
def _try_inputs():
    """The ingredients of test_gpu_edges.py::test_not_positive_definite_order at m = 40: knots
    uniform on [0, 10]^3 at l = 0.3 (K22 nearly diagonal), jitter delta = -1e-3."""
    g = _rng(77)
    n, m, d = 500, 40, 3
    U = g.uniform(0.0, 10.0, size=(m, d))
    X = g.uniform(0.0, 10.0, size=(n, d))
    noise = g.normal(0.0, 0.5, size=n)
    return X, U, noise


def border_margins(P, laplace=False):
    """(smallest eigenvalue of the base K22, of K22 bordered by a copy of knot TRY_DUP, and the
    bordered model's Schur complement sK of that candidate).  K22 = Kuu + e I with e = delta (VI,
    FITC) or tau^2 + delta (Laplace, quirk Q1); for an exact copy of knot j,
    sK = 2 e - e^2 (K22^-1)_jj."""
    th = theta_of(P)
    sigma, ls, tau = th[0], th[1:-1], th[-1]
    e = P["delta"] + (tau ** 2 if laplace else 0.0)
    U2 = np.vstack([P["U"], P["U"][TRY_DUP]])
    Kb = A._kmat(P["cov_fun"], U2, U2, sigma, ls)[0] + e * np.eye(U2.shape[0])
    m = P["U"].shape[0]
    K22, k = Kb[:m, :m], Kb[:m, m]
    sK = Kb[m, m] - k @ np.linalg.solve(K22, k)
    return np.linalg.eigvalsh(K22)[0], np.linalg.eigvalsh(Kb)[0], sK, e


@functools.lru_cache(maxsize=None)
def try_error(mode):
    """Candidates [good_0, a copy of knot TRY_DUP, good_1].  VI / FITC: the good ones are rows of
    X.  Laplace (Poisson): K22 carries tau^2 + delta (quirk Q1), so tau = 0.01 makes it
    -9e-4; a row of X as a knot would then have Z_i = 2 e - ... < 0 (the same Schur complement), so
    the good candidates are rows of X moved by 0.1 in every coordinate."""
    X, U, noise = _try_inputs()
    n = X.shape[0]
    rows = _rng(1600).choice(n, size=2, replace=False)
    if mode == "laplace":
        f = 0.5 * np.sin(X).sum(axis=1) / math.sqrt(3.0) + math.log(2.0)
        y = _rng(1601).poisson(np.exp(f)).astype(np.float64)
        mu = np.full(n, math.log(y.mean()))
        P = dict(X=X, U=U, y=y, mu=mu, f0=mu.copy(), expo=1.0, family="poisson",
                 cov_par=OrderedDict([("sigma", 1.0), ("l", 0.3), ("tau", 0.01)]),
                 cov_fun="sqexp", delta=TRY_DELTA)
        good = X[rows] + 0.1
        return _lap_scored(P, np.vstack([good[0], U[TRY_DUP], good[1]]), bad=(TRY_BAD,))
    y = np.sin(X).sum(axis=1) + noise
    P = dict(X=X, U=U, y=y, mu=np.full(n, y.mean()),
             cov_par=OrderedDict([("sigma", 1.0), ("l", 0.3), ("tau", 0.5)]), cov_fun="sqexp",
             delta=TRY_DELTA)
    out = _scored(mode, P, np.vstack([X[rows[0]], U[TRY_DUP], X[rows[1]]]), bad=(TRY_BAD,))
    out["base"], out["base_lit"] = objective(mode, P, U)
    return out


# ----------------------------------------------------------------------------- f. near a knot
NEAR_DIST = (0.5, 0.05)      # candidate distances from knot 0, in length scales
# relative error of oracle.adjoint_ref.vi_candidates (plain fp64 numpy, the scorer's algebra)
# against oracle.mp_ref.vi_objective (50 digits) for the candidates [0.5 l, 0.05 l, far].
# Measured (tests/test_candidate_cases.py prints them): 0, 1.1e-14, 1.6e-16 -- the constants
# leave a few ulps for another BLAS's summation order, and that test asserts the model still
# meets them.  The device is held to max(1e-9, 100 x the constant) per candidate: tau = 0.5
# keeps Bm well conditioned here, so the cancellation in sK and sB costs two digits at most
NEAR_KNOT_MODEL_ERR = (1e-15, 5e-14, 1e-15)


@functools.lru_cache(maxsize=None)
def near_knot():
    """n = 60, m = 8, d = 2, sqexp, delta = 1e-6: "truth" is the 50-digit dense ELBO at the
    augmented knots."""
    import mpmath as mp

    from oracle import mp_ref as M
    P = FC.gauss(60, 8, 2, "sqexp", 1700)
    l = P["cov_par"]["l"]
    u0 = P["U"][0]
    dirn = np.array([0.6, 0.8])
    dist = np.linalg.norm(P["X"][:, None, :] - P["U"][None, :, :], axis=2).min(axis=1)
    far = P["X"][np.argmax(dist)]                      # the row farthest from every knot
    cand = np.vstack([u0 + NEAR_DIST[0] * l * dirn, u0 + NEAR_DIST[1] * l * dirn, far])
    out = _scored("vi", P, cand)
    truth = []
    with mp.workdps(M.DPS):
        th, Xm, r = M._theta(P["cov_par"]), M._mat(P["X"]), M._vec(P["y"] - P["mu"])
        for x in cand:
            v = M.vi_objective(th, "sqexp", Xm, M._mat(np.vstack([P["U"], x])), r,
                               mp.mpf(P["delta"]))
            truth.append(float(v))
    out["truth"] = np.array(truth)
    return out


# ----------------------------------------------------------------------------- g. outside the box
@functools.lru_cache(maxsize=None)
def outside(mode):
    """n = 1500, m = 40, d = 2, X uniform on [0, 10]^2, l = 0.7.  Candidates [x_in, x_edge, x_far]:
    x_edge a tenth of the range outside the data box in its first coordinate (the reference's
    knot bounds, Q9), x_far = (400, 400)."""
    g = _rng(1800)
    n, m, d = 1500, 40, 2
    X = g.uniform(0.0, 10.0, size=(n, d))
    U = g.uniform(0.0, 10.0, size=(m, d))
    y = np.sin(X).sum(axis=1) / math.sqrt(d) + g.normal(0.0, 0.5, size=n)
    P = dict(X=X, U=U, y=y, mu=np.full(n, y.mean()),
             cov_par=OrderedDict([("sigma", 1.2), ("l", 0.7), ("tau", 0.5)]), cov_fun="sqexp",
             delta=1e-6)
    b = O.knot_bounds_of(X)
    x_in = g.uniform(2.0, 8.0, size=d)
    x_edge = np.array([b[0, 1], 0.5 * (X[:, 1].min() + X[:, 1].max())])
    out = _scored(mode, P, np.vstack([x_in, x_edge, [400.0, 400.0]]))
    out["base"], out["base_lit"] = objective(mode, P, U)
    return out


# ----------------------------------------------------------------------------- i. context state
@functools.lru_cache(maxsize=None)
def state_gauss():
    """C2, n = 300: knots U (m = 20) and U' (m = 21), theta' != theta, two candidates from X, and
    the oracle's knot posteriors at (theta, U) with muu = mean(y)."""
    P = make_gaussian_problem("C2", n=300, m=20)
    U21 = make_gaussian_problem("C2", n=300, m=21)["U"]
    muu = np.full(20, P["y"].mean())
    args = (P["cov_par"], "sqexp", P["U"], P["X"], P["y"], P["mu"], muu, P["delta"])
    return dict(P=P, theta=theta_of(P), theta2=theta_of(P) * np.array([1.1, 0.9, 1.2]), U21=U21,
                cand=P["X"][_rng(1900).choice(300, size=2, replace=False)], muu=muu,
                post_vi=O.vi_posterior_u(*args), post_fitc=O.fitc_posterior_u(*args))


@functools.lru_cache(maxsize=None)
def state_laplace():
    """Poisson, n = 300, m = 20: the oracle's Newton run from the reference's start with its knot
    posterior (muu = mu)."""
    P = _lap_problem("poisson", 300, 20)
    muu = np.full(20, P["mu"][0])
    nr = LC.newtrap(P, tol=LAP_TOL, muu=muu)
    return dict(P=P, theta=theta_of(P), muu=muu, nr=nr,
                cand=P["X"][_rng(1901).choice(300, size=2, replace=False)])


@functools.lru_cache(maxsize=None)
def state_try(mode):
    """3e's inputs: an evaluation at U succeeds, one at [U; U[TRY_DUP]] is not positive
    definite; the oracle's posterior of the first (muu = mean(y))."""
    P = try_error(mode)["P"]
    muu = np.full(P["U"].shape[0], P["y"].mean())
    post = (O.vi_posterior_u if mode == "vi" else O.fitc_posterior_u)(
        P["cov_par"], "sqexp", P["U"], P["X"], P["y"], P["mu"], muu, P["delta"])
    return dict(P=P, theta=theta_of(P), muu=muu, post=post,
                U_bad=np.vstack([P["U"], P["U"][TRY_DUP]]))


@functools.lru_cache(maxsize=None)
def state_knots():
    """tests/test_gpu_knots.py's VI shape (n = 90, m = 7): the oracle's knot gradient at theta."""
    P = make_gaussian_problem("C2", n=90, m=7)
    ref = O.delbo_dcov_par(P["cov_par"], "sqexp", P["U"], P["X"], P["y"], P["mu"], P["delta"],
                           dcov_fun_dknot="sqexp")
    return dict(P=P, theta=theta_of(P), theta2=theta_of(P) * np.array([1.1, 0.9, 1.2]),
                cand=P["X"][:2].copy(), bounds=O.knot_bounds_of(P["X"]),
                knot_gradient=np.ravel(ref["knot_gradient"]))
