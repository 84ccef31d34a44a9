"""The EGO proposal's numpy oracle (tests/ego_oracle.py) against the reference's literal text,
mpmath and finite differences, and the product's host-side half (sparsergps_amd.proposals)
against that oracle.  No GPU."""
import math

import mpmath
import numpy as np
import pytest

import ego_oracle as E
from sparsergps_amd import proposals as P


@pytest.mark.parametrize("n,d,T,cov_fun,l,tau", [(60, 3, 7, "exp", 1.0, 0.0),
                                                 (41, 1, 5, "exp", 2.0, 0.0),
                                                 (33, 2, 9, "sqexp", 1.5, 0.3),
                                                 (17, 4, 1, "exp", 1.0, 0.2)])
def test_vectorised_scan_is_the_literal_loop(n, d, T, cov_fun, l, tau):
    X, xm, v = E.recipe(n, d, T)
    par = {"sigma": 3.0, "l": l, "tau": tau}
    excl = np.vstack([X[[2, n - 1]], X[5] + np.r_[0.5, np.zeros(d - 1)]])
    lit = E.scan_literal(X, xm, v, par, cov_fun, 1e-6, excl)
    vec = E.scan(X, xm, v, par, cov_fun, 1e-6, excl)
    # both are double-precision evaluations of the same formula: they differ by the rounding
    # of solve() against inv(), cond(K22) * eps * the entry's magnitude budget
    tol = 16 * vec["cond"] * np.finfo(float).eps
    assert np.all(np.abs(lit["mean"] - vec["mean"]) <= tol * vec["s_mean"])
    assert np.all(np.abs(lit["var"] - vec["var"]) <= tol * vec["s_var"])
    assert list(np.flatnonzero(lit["excluded"])) == [2, n - 1]
    assert np.array_equal(np.isnan(lit["ei"]), lit["excluded"])
    b, on = E.ei_bound(vec, par["sigma"], rel=tol)
    assert np.all(np.abs(lit["ei"] - vec["ei"])[on] <= b[on])
    if E.top_two_gap(vec["ei"]) > 1e-9:
        assert lit["row"] == vec["row"]
    assert lit["row"] not in (2, n - 1)


def test_pnorm_and_ei_against_mpmath():
    mpmath.mp.dps = 60
    zs = np.concatenate([np.linspace(-35.0, 8.0, 173), [-1e-9, 0.0, 1e-9]])
    for z in zs:
        zz = mpmath.mpf(float(z))
        Phi = mpmath.erfc(-zz / mpmath.sqrt(2)) / 2
        phi = mpmath.exp(-zz * zz / 2) / mpmath.sqrt(2 * mpmath.pi)
        # erfc and exp are good to a few ulp; their arguments carry one rounding, which the
        # functions amplify by |d log f / d log x| <= z^2 + 1
        rel = 8 * (z * z + 1) * np.finfo(float).eps
        assert abs(E.pnorm(z) - Phi) <= rel * Phi
        # z Phi + phi cancels for z < 0 down to ~ phi / z^2: absolute error rel * (|z| Phi + phi)
        h = zz * Phi + phi
        got = float(E.expected_improvement(np.array([float(z)]), np.array([1.0]), 0.0, 0.0)[0])
        assert abs(got - h) <= rel * (abs(zz) * Phi + phi), (z, got, h)
        assert got >= 0.0 or abs(got) <= rel * phi


def test_ei_is_zero_unless_var_exceeds_tau2():
    ei = E.expected_improvement(np.zeros(4), np.array([0.25, 0.25 + 1e-12, np.nan, -1.0]), 0.0, 0.5)
    assert ei[0] == 0.0 and ei[1] > 0.0 and ei[2] == 0.0 and ei[3] == 0.0


def test_which_max_rules():
    assert E.which_max(np.array([0.1, 0.7, 0.7, 0.2])) == 1                  # first of equals
    assert E.which_max(np.array([np.nan, 0.3, np.nan, 0.3])) == 1            # a NaN never wins
    assert E.which_max(np.zeros(5)) == 0                                     # all zero: first
    ex = np.array([True, True, False, False, False])
    assert E.which_max(np.zeros(5), ex) == 2                                 # first non-excluded
    assert E.which_max(np.array([9.0, 1.0, 2.0, 5.0, 5.0]), ex) == 3
    assert E.which_max(np.array([1.0, 2.0]), np.array([True, True])) == -1
    assert E.which_max(np.array([np.nan, np.nan])) == -1                     # R: integer(0)


def _fd(par, *args, h=1e-5):
    g = np.zeros(2)
    for p in range(2):
        e = np.zeros(2)
        e[p] = h
        g[p] = (E.meta_nll(par + e, *args) - E.meta_nll(par - e, *args)) / (2 * h)
    return g


def test_meta_gradient_is_the_objectives_at_d1_and_not_at_d2():
    rng = np.random.default_rng(3)
    par = np.log([2.0, 0.8])
    for cov_fun in ("exp", "sqexp"):
        x = rng.uniform(0, 10, size=(9, 1))
        v = -40 + np.sin(x[:, 0]) + rng.normal(0, 0.1, 9)
        args = (x, v, cov_fun, 0.1, 1e-6)
        g, fd = E.meta_grad(par, *args), _fd(par, *args)
        # central differences with h = 1e-5: truncation h^2 |f'''| / 6 + rounding eps |f| / h
        assert np.all(np.abs(g - fd) <= 1e-6 * (1 + np.abs(fd))), (cov_fun, g, fd)
    x = rng.uniform(0, 10, size=(9, 2))
    v = -40 + np.sin(x).sum(axis=1) + rng.normal(0, 0.1, 9)
    args = (x, v, "exp", 0.1, 1e-6)
    g, fd = E.meta_grad(par, *args), _fd(par, *args)
    # quirk Q12: L2-distance derivatives against L1-distance values -- not the gradient
    assert np.max(np.abs(g - fd) / (1 + np.abs(fd))) > 1e-2, (g, fd)
    gs, fds = E.meta_grad(par, x, v, "sqexp", 0.1, 1e-6), _fd(par, x, v, "sqexp", 0.1, 1e-6)
    assert np.all(np.abs(gs - fds) <= 1e-6 * (1 + np.abs(fds)))             # sqexp has no quirk


def test_product_meta_functions_are_the_oracles():
    rng = np.random.default_rng(11)
    for d, cov_fun, tau in ((1, "exp", 0.0), (3, "exp", 0.2), (2, "sqexp", 0.0)):
        x = rng.uniform(0, 10, size=(12, d))
        v = -50 + rng.normal(0, 1, 12)
        par = np.log([3.0, 1.0]) + rng.normal(0, 0.3, 2)
        a, b = P.meta_mod_obj_fun(par, x, v, cov_fun, tau, 1e-6), E.meta_nll(par, x, v, cov_fun, tau, 1e-6)
        assert abs(a - b) <= 1e-12 * abs(b)
        ga, gb = P.meta_mod_grad(par, x, v, cov_fun, tau, 1e-6), E.meta_grad(par, x, v, cov_fun, tau, 1e-6)
        assert np.all(np.abs(ga - gb) <= 1e-10 * (1 + np.abs(gb)))
        assert np.array_equal(P.meta_fit_fallback(x, v), E.fallback(x, v))


def test_reference_opt_defaults():
    for o in (P.OPT_EGO_NORM_VI, P.OPT_EGO_NORM, P.OPT_EGO):
        assert o["TTmin"] == 10 and o["TTmax"] == 40 and o["delta"] == 1e-6
        assert o["ego_cov_par"] == {"sigma": 3.0, "l": 1.0, "tau": 0.0} and o["ego_cov_fun"] == "exp"
    assert P.OPT_EGO_NORM_VI["tol_nr"] == 1e-5 and P.OPT_EGO["tol_nr"] == 1e-4
    assert P.OPT_EGO["grad_tol"] == 1e-1 and math.isinf(P.OPT_EGO_NORM["grad_tol"])
    o = P._merge_opt(P.OPT_EGO, {"TTmax": 12, "no_such_option": 1})
    assert o["TTmax"] == 12 and "no_such_option" not in o and P.OPT_EGO["TTmax"] == 40


def _toy(n=80, d=2, m=4, seed=7):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 10, size=(n, d))
    xu = xy[rng.choice(n, m, replace=False)].copy()
    return xy, xu


def _toy_scorer(xu, fail_on=None):
    calls = {"n": 0}

    def scorer(cand):
        cand = np.asarray(cand).reshape(-1, xu.shape[1])
        out = -50.0 + np.sin(cand).sum(axis=1) - 0.1 * np.abs(cand[:, None, :] - xu[None]).sum(axis=2).min(axis=1)
        for k in range(cand.shape[0]):
            calls["n"] += 1
            if fail_on is not None and calls["n"] == fail_on:
                out[k] = np.nan
        return out
    return scorer, calls


def _fixed_fit(x, vals, start, cov_fun, tau, delta):
    return np.log([vals.max() - vals.min() + 1.0, 2.0])


def _oracle_scan(xy, xu, delta):
    return lambda par, cov_fun, x, vals: E.scan(xy, x, vals, par, cov_fun, delta, excl=xu)["row"]


@pytest.mark.parametrize("meta_fit", [_fixed_fit, None])
def test_product_loop_is_the_oracle_loop(meta_fit):
    """sparsergps_amd.proposals.ego_proposal with the oracle's scan plugged in takes the oracle
    loop's steps: the same scanned rows (the oracle also runs the reference's last, unread
    scan) and the same returned row.  None = the default scipy BFGS fit on both sides."""
    xy, xu = _toy()
    o = P._merge_opt(P.OPT_EGO_NORM_VI, {"TTmin": 4, "TTmax": 8})
    init = [0, 9, 33, 71]
    fit = meta_fit or P.meta_fit_bfgs
    tr_p, tr_o = [], []
    got = P.ego_proposal(xy, xu, _toy_scorer(xu)[0], _oracle_scan(xy, xu, o["delta"]), o,
                         init_rows=init, meta_fit=fit, trace=tr_p)
    ref = E.proposal_loop(xy, xu, _toy_scorer(xu)[0], o, init_rows=init, meta_fit=fit, trace=tr_o)
    assert len(tr_o) == o["TTmax"] - o["TTmin"] + 1 and len(tr_p) == len(tr_o) - 1
    assert [t["row"] for t in tr_p] == [t["row"] for t in tr_o[:-1]]
    assert got.shape == (1, 2) and np.array_equal(got, ref)
    assert any((xy == got).all(axis=1))


def test_failing_meta_fit_takes_the_reference_fallback():
    xy, xu = _toy()
    o = P._merge_opt(P.OPT_EGO_NORM_VI, {"TTmin": 3, "TTmax": 5})

    def boom(*a):
        raise np.linalg.LinAlgError("chol")

    def nan_fit(*a):
        return np.array([np.nan, 0.0])
    for fit in (boom, nan_fit):
        tr = []
        P.ego_proposal(xy, xu, _toy_scorer(xu)[0], _oracle_scan(xy, xu, 1e-6), o,
                       init_rows=[1, 2, 3], meta_fit=fit, trace=tr)
        assert len(tr) == 2
        for t in tr:
            assert t["cov_par"]["tau"] == 0.0
            # (max x - min x) / 1000 over the scored candidates, a subset of xy
            assert 0.0 < t["cov_par"]["l"] <= (xy.max() - xy.min()) / 1000.0


def test_nan_from_the_scorer_resamples_like_the_reference():
    """The scorer fails once, on the first EI-chosen candidate (call 5 after 4 initial rows):
    both loops draw one replacement row plus N(0, 1e-6) jitter from the injected generator."""
    xy, xu = _toy()
    o = P._merge_opt(P.OPT_EGO_NORM_VI, {"TTmin": 4, "TTmax": 7})
    init = [0, 9, 33, 71]
    sp, cp = _toy_scorer(xu, fail_on=5)
    so, co = _toy_scorer(xu, fail_on=5)
    got = P.ego_proposal(xy, xu, sp, _oracle_scan(xy, xu, 1e-6), o, rng=np.random.default_rng(5),
                         init_rows=init, meta_fit=_fixed_fit)
    ref = E.proposal_loop(xy, xu, so, o, rng=np.random.default_rng(5), init_rows=init,
                          meta_fit=_fixed_fit)
    assert cp["n"] == co["n"] == 4 + 3 + 1
    assert np.array_equal(got, ref)
    with pytest.raises(ValueError, match="rng"):
        P.ego_proposal(xy, xu, _toy_scorer(xu, fail_on=5)[0], _oracle_scan(xy, xu, 1e-6), o,
                       init_rows=init, meta_fit=_fixed_fit)


def test_rows_outside_knots():
    xy, xu = _toy()
    near = xu.copy()
    near[:, 1] += 1.0                      # matches a row in coordinate 0 only: excludes nothing
    keep = P.rows_outside_knots(xy, np.vstack([xu, near]))
    assert np.array_equal(keep, np.flatnonzero(~E.excluded_rows(xy, xu)))
    assert keep.size == xy.shape[0] - xu.shape[0]
