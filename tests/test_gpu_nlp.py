"""Held-out scoring on the MI355X: sgp_nlp, sgp_predict_nlp, my_nlp, predict_prob, score_gp.

* the whole fixture tests/golden/nlp_grid.npz (the 612-case grid, the confident bernoulli row, the
  far-tail and the y = 5000 poisson rows), one call per family, against the 50-digit truth at
  1e-10 max(1, |nlp|) (GPU against mpmath); every row finite;
* n in {1, 63, 64, 65, 255, 256, 257, 100 003} random rows of the box mu in [-6, 6], s2 in
  [1e-6, 25] per family against the numpy model of sgp_quad.h at 1e-11 max(1, |nlp|); stats against
  math.fsum of the returned rows at 1e-12 relative with exact counts; a second call and a call on
  a grid of 7 workgroups bit-identical;
* invalid rows (pred_var 0, -1, NaN; pred_mean NaN) among good ones at n = 130: NaN, counted,
  every other row's bits untouched;
* a constant per-row exposure gives the scalar call's bits;
* sgp_predict_nlp for every prediction method at np in {1, 129}, m in {5, 130}: pred_mean and
  pred_var bit-identical to sgp_predict, nlp and stats to sgp_nlp on those vectors;
* score_gp on a small VI fit and a small bernoulli fit (golden fixtures) against predict_gp plus
  the oracle's model, my_rmse and the median.
"""
import math
import os
from collections import OrderedDict

import numpy as np
import pytest

import nlp_oracle as NO
import predict_cases as PC
from oracle import sgp_oracle as O

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAMS = ("poisson", "bernoulli", "gaussian")
TAU, M_EXPO = 0.3, 1.7


@pytest.fixture(scope="module")
def sgp():
    import sparsergps_amd as S
    from sparsergps_amd import _lib
    _lib.require_gpu()
    return S


def _call(family, y, pm, pv, par=1.0, expo=None, max_blocks=None):
    """sgp_nlp (or sgp_diag_nlp with a grid cap): (nlp, stats)."""
    from sparsergps_amd import _lib
    lib = _lib.lib()
    y, pm, pv = (np.ascontiguousarray(v, dtype=np.float64) for v in (y, pm, pv))
    ex = None if expo is None else np.ascontiguousarray(expo, dtype=np.float64)
    nlp, st = np.zeros(y.size), np.zeros(4)
    head = (0, _lib.SCORE_FAMILIES[family])
    tail = (_lib.dptr(y), _lib.dptr(pm), _lib.dptr(pv), y.size, float(par),
            None if ex is None else _lib.dptr(ex), _lib.dptr(nlp), _lib.dptr(st))
    if max_blocks is None:
        _lib.check(lib.sgp_nlp(*head, *tail))
    else:
        _lib.check(lib.sgp_diag_nlp(*head, max_blocks, *tail, None))
    return nlp, st


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


def _rel(got, ref):
    return np.abs(got - ref) / np.maximum(1.0, np.abs(ref))


# ------------------------------------------------------------------ the fixture
@pytest.mark.parametrize("family", ["poisson", "bernoulli"])
def test_fixture_against_truth(sgp, family):
    g = np.load(os.path.join(GOLD, "nlp_grid.npz"))
    k = g["fam"] == {"poisson": 0, "bernoulli": 1}[family]
    assert k.sum() == {"poisson": 542, "bernoulli": 73}[family]
    par = {"m": g["m"][k]} if family == "poisson" else None
    got = sgp.my_nlp(g["y"][k], g["mu"][k], g["s2"][k], family=family, par=par)["nlp"]
    err = _rel(got, g["nlp"][k])
    print(family, "against mpmath: max %.3g at row %d" % (err.max(), err.argmax()))
    assert np.all(np.isfinite(got))          # the confident and the far-tail rows included
    assert err.max() <= 1e-10


def test_predict_prob(sgp):
    pm = np.array([-0.3, 0.0, 2.0, -6.0])
    pv = np.array([1e-6, 0.7, 4.0, 25.0])
    p = sgp.predict_prob(pm, pv)
    ref = np.exp(-NO.model_nlp("bernoulli", np.ones(4), pm, pv))
    assert np.all((p > 0) & (p < 1)) and np.max(np.abs(p - ref)) <= 1e-12
    assert abs(p[1] - 0.5) <= 1e-13          # symmetric integrand


# ------------------------------------------------------------------ random rows in the box
_RAND = {}


def _random_rows(family, n):
    """Inputs and the numpy model's nlp, computed once per (family, n)."""
    if (family, n) not in _RAND:
        rng = np.random.default_rng(1000 * FAMS.index(family) + n % 997)
        mu = rng.uniform(-6.0, 6.0, n)
        s2 = 10.0 ** rng.uniform(-6.0, math.log10(25.0), n)
        if family == "poisson":
            y = rng.integers(0, 201, n).astype(np.float64)
            y[rng.random(n) < 0.3] = 0.0
            par = M_EXPO
        elif family == "bernoulli":
            y = (rng.random(n) < 0.5).astype(np.float64)
            par = 0.0
        else:
            y = mu + rng.normal(0.0, 2.0, n)
            par = TAU
        ref = NO.model_nlp(family, y, mu, s2, par=par)
        ref.setflags(write=False)
        _RAND[(family, n)] = (y, mu, s2, par, ref)
    return _RAND[(family, n)]


def _check_stats(st, nlp, y, pm):
    fin = np.isfinite(nlp)
    ref0 = math.fsum(nlp[fin])
    ref3 = math.fsum((pm - y) ** 2)
    assert abs(st[0] - ref0) <= 1e-12 * abs(ref0)
    assert st[1] == fin.sum() and st[2] == np.isnan(nlp).sum()
    assert abs(st[3] - ref3) <= 1e-12 * abs(ref3)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 100003])
@pytest.mark.parametrize("family", FAMS)
def test_random_rows(sgp, family, n):
    y, mu, s2, par, ref = _random_rows(family, n)
    nlp, st = _call(family, y, mu, s2, par)
    err = _rel(nlp, ref)
    print(family, n, "against the model: max %.3g" % err.max())
    assert np.all(np.isfinite(nlp)) and err.max() <= 1e-11
    _check_stats(st, nlp, y, mu)
    nlp2, st2 = _call(family, y, mu, s2, par)
    assert np.array_equal(_bits(nlp), _bits(nlp2)) and np.array_equal(_bits(st), _bits(st2))
    # independent of the grid: 7 workgroups take the tiles in rounds
    nlp3, st3 = _call(family, y, mu, s2, par, max_blocks=7)
    assert np.array_equal(_bits(nlp), _bits(nlp3)) and np.array_equal(_bits(st), _bits(st3))


@pytest.mark.parametrize("family", FAMS)
def test_invalid_rows_do_not_touch_their_neighbours(sgp, family):
    n = 130
    y, mu, s2, par, _ = _random_rows(family, 257)
    y, mu, s2 = y[:n].copy(), mu[:n].copy(), s2[:n].copy()
    if family == "gaussian":
        par = 0.0                     # the variance tested is pred_var + tau^2
    clean, _ = _call(family, y, mu, s2, par)
    bad_var = {3: 0.0, 64: -1.0, 65: float("nan"), 129: 0.0, 0: -1.0}
    bad_mean = {17: float("nan"), 63: float("nan"), 128: float("nan")}
    mu2, s22 = mu.copy(), s2.copy()
    for i, v in bad_var.items():
        s22[i] = v
    for i, v in bad_mean.items():
        mu2[i] = v
    bad = sorted({**bad_var, **bad_mean})
    nlp, st = _call(family, y, mu2, s22, par)
    assert np.all(np.isnan(nlp[bad])) and st[2] == len(bad) and st[1] == n - len(bad)
    good = np.setdiff1d(np.arange(n), bad)
    assert np.array_equal(_bits(nlp[good]), _bits(clean[good]))
    assert abs(st[0] - math.fsum(clean[good])) <= 1e-12 * abs(math.fsum(clean[good]))
    if family == "gaussian":          # pred_var = 0 is a usable row once tau > 0
        v, _ = _call(family, y[:4], mu[:4], np.zeros(4), TAU)
        assert np.all(np.isfinite(v))


def test_constant_exposure_vector_is_the_scalar_call(sgp):
    y, mu, s2, par, _ = _random_rows("poisson", 257)
    a, sa = _call("poisson", y, mu, s2, par)
    b, sb = _call("poisson", y, mu, s2, 1.0, expo=np.full(y.size, par))
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(sa), _bits(sb))
    c, _ = _call("poisson", y, mu, s2, 1.0, expo=np.where(np.arange(y.size) % 2, par, 2 * par))
    odd = np.arange(y.size) % 2 == 1
    assert np.array_equal(_bits(a[odd]), _bits(c[odd])) and not np.array_equal(a[~odd], c[~odd])


# ------------------------------------------------------------------ sgp_predict_nlp
PRED_METHODS = PC.METHODS + ("lap_full",)
_PCASE = {}


def _pred_case(m, npred):
    """Inputs keyed as tests/predict_cases.py's fixtures (its `call` consumes them)."""
    if (m, npred) not in _PCASE:
        d = 3
        g = np.random.Generator(np.random.PCG64(900 + 7 * m + npred))
        U = g.uniform(0.0, 10.0, size=(m, d))
        xp = g.uniform(-1.0, 11.0, size=(npred, d))
        xp[0] = U[m - 1]
        cp = OrderedDict(sigma=1.2, l=1.2 if m > 128 else 1.7, tau=0.5)
        A = g.normal(0.0, 1.0, size=(m, m))
        post = dict(u_mean=0.3 + g.normal(0.0, 0.5, size=m),
                    u_var=0.05 * 1.2 ** 2 * (A @ A.T) / m, muu=np.full(m, 0.3))
        yu = np.sin(U).sum(axis=1) / math.sqrt(d) + g.normal(0.0, 0.5, size=m)
        _PCASE[(m, npred)] = dict(
            cov_fun="sqexp", cov_par=cp, U=U, xp=xp, delta=PC.DELTA,
            mu_pred=0.25 + 0.1 * np.sin(np.arange(npred)), gauss=post, nongauss=post,
            full=dict(y=yu, mu=np.full(m, yu.mean())),
            lapfull=dict(W=-g.uniform(0.05, 0.25, size=m), grad=g.normal(0.0, 0.4, size=m)),
            y_gauss=g.normal(0.3, 1.0, size=npred),
            y_pois=g.integers(0, 9, size=npred).astype(np.float64),
            y_bern=(g.random(npred) < 0.5).astype(np.float64))
    return _PCASE[(m, npred)]


@pytest.mark.parametrize("m", [5, 130])
@pytest.mark.parametrize("npred", [1, 129])
@pytest.mark.parametrize("method", PRED_METHODS)
def test_predict_nlp_is_predict_then_nlp(sgp, method, npred, m):
    from sparsergps_amd import _lib
    from sparsergps_amd.predict import _predict
    F = _pred_case(m, npred)
    cf, cp, U, xp, mup, dl = (F[k] for k in ("cov_fun", "cov_par", "U", "xp", "mu_pred", "delta"))
    if method == "lap_full":
        L = F["lapfull"]
        plain = sgp.predict_laplace_full(None, U, xp, L["W"], cp, cf, L["grad"], None, mup,
                                         False, dl)
        args = (_lib.SGP_PRED_LAPLACE_FULL, False, L["grad"], None, U, xp, cf, cp, mup, L["W"])
        score = ("bernoulli", F["y_bern"], 0.0, None)
    else:
        plain = PC.call(sgp, method, F, False)
        if method == "gp_full":
            args = (_lib.SGP_PRED_FULL, True, F["full"]["y"], None, U, xp, cf, cp, mup,
                    F["full"]["mu"])
        else:
            P = F["nongauss" if method == "lap_nongauss" else "gauss"]
            args = (_lib.SGP_PRED_VI if method == "vi" else _lib.SGP_PRED_LAPLACE,
                    method != "lap_nongauss", P["u_mean"], P["u_var"], U, xp, cf, cp, mup,
                    P["muu"])
        score = (("poisson", F["y_pois"], M_EXPO, None) if method == "lap_nongauss"
                 else ("gaussian", F["y_gauss"], cp["tau"], None))
    got = _predict(*args, False, dl, score)
    assert np.array_equal(_bits(got["pred_mean"]), _bits(plain["pred_mean"]))
    assert np.array_equal(_bits(got["pred_var"]), _bits(plain["pred_var"]))
    nlp, st = _call(score[0], score[1], plain["pred_mean"].reshape(-1), plain["pred_var"],
                    score[2])
    assert np.array_equal(_bits(got["nlp"]), _bits(nlp))
    assert np.array_equal(_bits(got["stats"]), _bits(st))
    assert np.all(np.asarray(plain["pred_var"]) > 0) and np.all(np.isfinite(nlp))


# ------------------------------------------------------------------ score_gp
def _check_score(sgp, mod, sc, x, y, mu_pred, family, par, vi):
    pred = sgp.predict_gp(mod, x, mu_pred, full_cov=False, vi=vi)["pred"]
    assert np.array_equal(_bits(sc["pred"]["pred_mean"]), _bits(pred["pred_mean"]))
    assert np.array_equal(_bits(sc["pred"]["pred_var"]), _bits(pred["pred_var"]))
    pm = pred["pred_mean"].reshape(-1)
    ref = NO.model_nlp(family, y, pm, pred["pred_var"], par=par)
    assert np.all(np.isfinite(ref)) and _rel(sc["nlp"], ref).max() <= 1e-11
    assert abs(sc["median_nlp"] - np.median(ref)) <= 1e-11 * max(1.0, abs(np.median(ref)))
    assert abs(sc["mean_nlp"] - np.mean(ref)) <= 1e-11 * max(1.0, abs(np.mean(ref)))
    rmse = NO.literal_rmse(pm, y)
    assert abs(sc["rmse"] - rmse) <= 1e-13 * rmse
    assert abs(sc["srmse"] - rmse / np.std(y, ddof=1)) <= 1e-13 * sc["srmse"]
    assert sc["n_nan"] == 0


def test_score_gp_vi_fit(sgp):
    z = np.load(os.path.join(GOLD, "gauss_c2_small.npz"))
    cp = OrderedDict(zip([str(s) for s in z["names"]], (float(v) for v in z["theta"])))
    cf, dl = str(z["cov_fun"]), float(z["delta"])
    X, y, mu, U = z["X"], z["y"], z["mu"], z["U"]
    tr, te = slice(0, 150), slice(150, 200)
    muu = np.full(U.shape[0], mu[0])
    um, uv = O.vi_posterior_u(cp, cf, U, X[tr], y[tr], mu[tr], muu, dl)
    mod = {"family": "gaussian", "sparse": True, "delta": dl,
           "results": {"u_mean": um, "u_var": uv, "xu": U, "cov_fun": cf, "cov_par": cp,
                       "muu": muu}}
    sc = sgp.score_gp(mod, X[te], y[te], mu_pred=mu[te], vi=True)
    _check_score(sgp, mod, sc, X[te], y[te], mu[te], "gaussian", cp["tau"], True)
    assert sgp.score_gp(dict(mod, family="poisson"), X[te], np.ones(50), vi=True) == \
        "Error: VI not supported for non-gaussian data."


def test_score_gp_bernoulli_fit(sgp):
    z = np.load(os.path.join(GOLD, "bernoulli_small.npz"))
    cp = OrderedDict(zip(("sigma", "l", "tau"), (float(v) for v in z["theta"])))
    dl, U = float(z["delta"]), z["U"]
    muu = np.zeros(U.shape[0])
    with sgp.SparseGPContext(z["X"], z["y"], z["mu"], m_max=U.shape[0]) as ctx:
        sgp.newtrap_sparseGP(z["f0"], cp, "sqexp", z["X"], U, z["y"], z["mu"], 1.0, dl,
                             tol=float(z["tol"]), ctx=ctx, family="bernoulli")
        um, uv = ctx.posterior_u(muu)
    mod = {"family": "bernoulli", "sparse": True, "delta": dl,
           "results": {"u_mean": um, "u_var": uv, "xu": U, "cov_fun": "sqexp", "cov_par": cp,
                       "muu": muu}}
    x, y = z["X"][:60], z["y"][:60]
    mu_pred = np.zeros(60)
    sc = sgp.score_gp(mod, x, y, mu_pred=mu_pred)
    _check_score(sgp, mod, sc, x, y, mu_pred, "bernoulli", 0.0, False)
    # the averaged class probability scores a 1 exactly as my_nlp does
    p = sgp.predict_prob(sc["pred"]["pred_mean"], sc["pred"]["pred_var"])
    assert np.array_equal(_bits(p[y == 1]), _bits(np.exp(-sc["nlp"][y == 1])))
