"""The OAT knot selection on the GPU against the line-by-line oracle loop of tests/oat_oracle.py
over oracle/drivers.py: VI (sqexp d = 3 with random proposals, ARD with knot_prop_var), FITC
with the EGO proposal (a deterministic meta-model fit, as tests/test_gpu_ego.py pins it), and
Poisson Laplace with knot_prop_error; n = 240 (300 for Poisson), three starting knots,
maxknot = 5, maxit = 4, obj_tol = 0, TTmin = 3, TTmax = 5.  The same seeded numpy Generator
drives both loops.

Bars (tests/test_gpu_drivers.py's): rtol 1e-6, atol 1e-9; atol 1e-7 for posteriors.  The oracle
run asserts that every accept / reject margin is at least 1e-3 away from tol_knot and that every
candidate arg-max is decided by at least 1e-3 (absolute for objective values, relative for scan
keys), so no decision can flip by rounding.
"""
import functools
from collections import OrderedDict

import numpy as np
import pytest

import ego_oracle as E
import oat_oracle as OO
from oracle import sgp_oracle as O

pytestmark = pytest.mark.gpu
RTOL = 1e-6
BASE = {"maxknot": 5, "maxit": 4, "obj_tol": 0.0, "TTmin": 3, "TTmax": 5}
# case -> (kind, cov_fun, proposal, tol_knot, seed)
CASES = {"vi-sqexp-random": ("vi", "sqexp", "random", 1e-3, 7),
         "vi-ard-var": ("vi", "ard", "var", 1e-3, 0),
         "fitc-sqexp-ego": ("fitc", "sqexp", "ego", 1e-3, 11),
         "poisson-error": ("laplace", "sqexp", "error", 1e-1, 0)}


@pytest.fixture(scope="module")
def sgp():
    import sparsergps_amd as S
    from sparsergps_amd import _lib
    _lib.require_gpu()
    return S


def _fixed_fit(x, vals, start, cov_fun, tau, delta):
    """tests/test_gpu_ego.py's deterministic meta fit: smooth in the scores."""
    return np.log([vals.max() - vals.min() + 1.0, 1.5 if x.shape[1] <= 2 else 12.0])


def _close(a, b, atol=1e-9):
    np.testing.assert_allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64),
                               rtol=RTOL, atol=atol)


@functools.lru_cache(maxsize=None)
def _problem(kind, cov_fun):
    if kind == "laplace":
        Pp = O.make_poisson_problem(n=300, m=3)
        return Pp, OrderedDict(Pp["cov_par"]), np.full(3, float(Pp["mu"][0]))
    G = O.make_gaussian_problem("C2", n=240, m=3)
    cp = OrderedDict(G["cov_par"])
    if cov_fun == "ard":
        cp = OrderedDict([("sigma", 1.0), ("l1", 4.0), ("l2", 5.0), ("l3", 3.0), ("tau", 0.5)])
    return G, cp, np.full(3, float(G["y"].mean()))


def _merged(kind, tol_knot):
    from sparsergps_amd import knot_selection as KS
    master = {"vi": KS.OPT_OAT_NORM_VI, "fitc": KS.OPT_OAT_NORM, "laplace": KS.OPT_OAT}[kind]
    return KS.merge_opt(master, {**BASE, "tol_knot": tol_knot})


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The oracle OAT run of a case, with its decision margins checked."""
    from sparsergps_amd import proposals as P
    kind, cov_fun, prop, tol_knot, seed = CASES[name]
    D, cp, muu = _problem(kind, cov_fun)
    o = _merged(kind, tol_knot)
    rng = np.random.default_rng(seed)
    a = D.get("a", 1.0)
    fit = OO.oracle_fit(kind, cov_fun, D["X"], D["y"], D["mu"], o, m=a)
    gaps = []

    def propose(f):
        if prop in ("var", "error"):
            row, res = OO.scan_proposal(f, prop)
            gaps.append(E.top_two_gap(res["key"]))
            return row
        score = OO.make_scorer(kind, f, D["y"], o["delta"], a)
        if prop == "random":
            tr = []
            out = OO.random_proposal(D["X"], f["xu"], score, f["obj_fun"][-1], o["TTmax"],
                                     rng=rng, trace=tr)
            gaps.append(tr[0]["gap"])
            return out
        tr = []
        oe = P._merge_opt(P.OPT_EGO_NORM, o)
        out = E.proposal_loop(D["X"], f["xu"], score, oe, rng=rng, meta_fit=_fixed_fit, trace=tr)
        gaps.extend(t["gap"] for t in tr[:-1])        # the last scan's result is never read
        return out

    margins = []
    ref = OO.oat_loop(fit, propose, cp, D["U"], muu, o, laplace=(kind == "laplace"),
                      ff=D.get("f0"), margins=margins)
    print(f"{name}: margins - tol_knot {margins}, arg-max gaps {gaps}, knots {ref['xu'].shape[0]}")
    assert margins and all(abs(mg) >= 1e-3 for mg in margins), margins
    assert gaps and all(g >= 1e-3 for g in gaps), gaps
    return ref


def _run(sgp, name):
    kind, cov_fun, prop, tol_knot, seed = CASES[name]
    D, cp, muu = _problem(kind, cov_fun)
    opt = {**BASE, "tol_knot": tol_knot}
    rng = np.random.default_rng(seed)
    pkw = {"meta_fit": _fixed_fit} if prop == "ego" else None
    if kind == "laplace":
        pf = {"error": sgp.knot_prop_error, "ego": sgp.knot_prop_ego,
              "random": sgp.knot_prop_random}[prop]
        return sgp.oat_knot_selection(cp, cov_fun, D["U"], pf, D["X"], D["y"], D["f0"], D["mu"],
                                      muu, m=D["a"], opt=opt, rng=rng, proposal_kw=pkw)
    if kind == "vi":
        pf = {"random": sgp.knot_prop_random_norm_vi, "var": sgp.knot_prop_var,
              "ego": sgp.knot_prop_ego_norm_vi}[prop]
        return sgp.oat_knot_selection_norm_vi(cp, cov_fun, D["U"], pf, D["X"], D["y"], D["mu"],
                                              muu, opt=opt, rng=rng, proposal_kw=pkw)
    pf = {"random": sgp.knot_prop_random_norm, "var": sgp.knot_prop_var,
          "ego": sgp.knot_prop_ego_norm}[prop]
    return sgp.oat_knot_selection_norm(cp, cov_fun, D["U"], pf, D["X"], D["y"], D["mu"], muu,
                                       opt=opt, rng=rng, proposal_kw=pkw)


@pytest.mark.parametrize("name", sorted(CASES))
def test_oat_matches_the_oracle_loop(sgp, name):
    ref = _oracle(name)
    got = _run(sgp, name)
    assert ref["shape"] in got and ("upost" in got) != ("u_post" in got)
    assert got["xu"].shape == ref["xu"].shape
    assert list(got["ga_steps"]) == list(ref["ga_steps"])
    _close(got["xu"], ref["xu"])
    _close(got["obj_fun"], ref["obj_fun"])
    _close(got["cov_par_history"], ref["cov_par_history"])
    _close(got["muu"], ref["muu"])
    _close(got["u_mean"], ref["u_mean"], atol=1e-7)
    _close(got["u_var"], ref["u_var"], atol=1e-7)
    if "fmax" in ref:
        _close(got["fmax"], ref["fmax"], atol=1e-7)
        assert got["success"] is ref["success"]


def test_optimize_gp_oat_result_scores_like_the_hand_assembled_mod(sgp):
    G, cp, muu = _problem("vi", "sqexp")
    opt = {**BASE, "tol_knot": 1e-3}
    mod = sgp.optimize_gp(G["y"], G["X"], "sqexp", cp, G["mu"], "gaussian", sparse=True,
                          xu_opt="oat", xu=G["U"], muu=muu, vi=True, opt=opt,
                          rng=np.random.default_rng(3), proposal_kw={"meta_fit": _fixed_fit})
    assert set(mod) == {"results", "sparse", "family", "delta", "xu_init"}
    res = mod["results"]
    assert 3 <= res["xu"].shape[0] <= 5 and np.array_equal(mod["xu_init"], G["U"])
    # optimize_gp's ego_cov_par$tau = 0 reaches the proposal; the same run by hand
    from sparsergps_amd import optimize as Z
    hand = sgp.oat_knot_selection_norm_vi(cp, "sqexp", G["U"], sgp.knot_prop_ego_norm_vi, G["X"],
                                          G["y"], G["mu"], muu,
                                          opt={**Z.OPT_MASTER, **opt}, rng=np.random.default_rng(3),
                                          proposal_kw={"meta_fit": _fixed_fit})
    hand_mod = {"results": hand, "sparse": True, "family": "gaussian", "delta": 1e-6}
    rng = np.random.default_rng(9)
    xt = rng.uniform(0, 10, size=(50, 3))
    yt = np.sin(xt).sum(axis=1)
    s1 = sgp.score_gp(mod, xt, yt, mu_pred=np.full(50, G["y"].mean()), vi=True)
    s2 = sgp.score_gp(hand_mod, xt, yt, mu_pred=np.full(50, G["y"].mean()), vi=True)
    assert np.array_equal(res["xu"], hand["xu"])
    assert np.array_equal(s1["nlp"], s2["nlp"]) and s1["rmse"] == s2["rmse"]
    assert np.isfinite(s1["mean_nlp"])
