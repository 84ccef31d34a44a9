"""The OAT layer without a GPU: the loop core over scripted and oracle fits, each function's
defaults against the reference's numbers, the random proposal's return value, and the
variance / error oracle against a dense restatement."""
import math
from collections import OrderedDict

import numpy as np
import pytest

import oat_oracle as OO
from oracle import sgp_oracle as O


@pytest.fixture(scope="module")
def KS():
    from sparsergps_amd import knot_selection
    return knot_selection


class ScriptedFit:
    """fit(...) returning the next scripted last-objective; records its arguments."""

    def __init__(self, objs, laplace=False, fail_at=()):
        self.objs, self.calls, self.laplace, self.fail_at = list(objs), [], laplace, set(fail_at)

    def __call__(self, cov_par, xu, knot_opt, dknot, muu, ff):
        k = len(self.calls)
        self.calls.append({"cov_par": dict(cov_par), "m": xu.shape[0], "knot_opt": knot_opt,
                           "dknot": dknot, "muu": np.array(muu), "ff": ff})
        if k in self.fail_at:
            from sparsergps_amd import NotPositiveDefinite
            raise NotPositiveDefinite(2, "scripted")
        m = xu.shape[0]
        moved = np.array(xu, dtype=np.float64)
        if knot_opt:
            moved[np.array(knot_opt) - 1] += 0.5          # the ascent moved the appended knot
        out = {"cov_par": OrderedDict(sigma=1.0 + k, l=2.0 + k, tau=0.5), "xu": moved,
               "obj_fun": np.array([-1e9, self.objs[k]]), "iter": 10 + k,
               "u_mean": np.full(m, float(k)), "u_var": np.eye(m) * (k + 1.0), "muu": np.array(muu)}
        if self.laplace:
            out["fmax"] = np.full(4, float(k))
        return out


def _propose_rows(rows):
    it = iter(rows)
    return lambda fit: np.asarray(next(it), dtype=np.float64).reshape(1, -1)


START = OrderedDict(sigma=1.0, l=2.0, tau=0.5)
XU0 = np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]])
MUU0 = np.array([0.7, 0.1, 0.2])


def _opt(KS, **kw):
    return KS.merge_opt(KS.OPT_OAT_NORM_VI, {"maxknot": 5, "tol_knot": 0.5, **kw})


def test_loop_ends_on_maxknot_with_the_upost_shape(KS):
    fit = ScriptedFit([-100.0, -90.0, -80.0])
    out = KS.oat_core(fit, _propose_rows([[5, 5], [6, 6]]), START, XU0, MUU0, _opt(KS))
    assert out["xu"].shape == (5, 2) and "upost" in out and "u_post" not in out
    assert len(out["obj_fun"]) == 3 and len(out["ga_steps"]) == 3
    assert list(out["ga_steps"]) == [10, 11, 12]
    assert out["cov_par_history"].shape == (4, 3)           # start + first fit + two accepted
    assert np.array_equal(out["cov_par_history"][0], [1.0, 2.0, 0.5])
    assert np.array_equal(out["u_mean"], np.full(5, 2.0))   # upost[[iter]]: the last fit's
    assert len(out["upost"]) == 3
    # muu grows by muu[1] (R index), the first fit has the knots fixed, later ones move only
    # the appended knot: knot_opt = m + 1, 1-based
    assert np.array_equal(out["muu"], [0.7, 0.1, 0.2, 0.7, 0.7])
    assert fit.calls[0]["knot_opt"] is None and fit.calls[0]["dknot"] is False
    assert fit.calls[1]["knot_opt"] == [4] and fit.calls[1]["dknot"] is True
    assert fit.calls[2]["knot_opt"] == [5] and fit.calls[2]["m"] == 5
    assert np.array_equal(fit.calls[2]["muu"], [0.7, 0.1, 0.2, 0.7, 0.7])
    assert np.array_equal(out["xu"][3], [5.5, 5.5])          # the moved knot is the one kept
    assert fit.calls[2]["cov_par"] == {"sigma": 2.0, "l": 3.0, "tau": 0.5}   # the accepted fit's


def test_cov_diff_false_keeps_every_knot_fixed(KS):
    fit = ScriptedFit([-100.0, -90.0, -80.0])
    out = KS.oat_core(fit, _propose_rows([[5, 5], [6, 6]]), START, XU0, MUU0,
                      _opt(KS, cov_diff=False))
    assert all(c["knot_opt"] is None and c["dknot"] is False for c in fit.calls)
    assert np.array_equal(out["xu"][3], [5.0, 5.0])


def test_choosek_stops_on_a_knot_that_does_not_pay(KS):
    fit = ScriptedFit([-100.0, -99.8, -50.0])               # +0.2 <= tol_knot = 0.5: rejected
    out = KS.oat_core(fit, _propose_rows([[5, 5], [6, 6]]), START, XU0, MUU0, _opt(KS))
    assert len(fit.calls) == 2 and out["xu"].shape == (3, 2)
    assert "u_post" in out and "upost" not in out
    assert list(out["obj_fun"]) == [-100.0, -99.8] and list(out["ga_steps"]) == [10, 11]
    assert out["cov_par_history"].shape == (2, 3)            # the rejected fit's is not stored
    assert np.array_equal(out["u_mean"], np.zeros(3))        # upost[[iter - 1]]: the first fit's
    assert out["u_post"][1] is None and np.array_equal(out["muu"], MUU0)
    assert out["cov_par"] == OrderedDict(sigma=1.0, l=2.0, tau=0.5)


def test_choosek_false_accepts_a_worsening_knot(KS):
    fit = ScriptedFit([-100.0, -120.0, -130.0])
    out = KS.oat_core(fit, _propose_rows([[5, 5], [6, 6]]), START, XU0, MUU0,
                      _opt(KS, chooseK=False))
    assert out["xu"].shape == (5, 2) and "upost" in out
    assert list(out["obj_fun"]) == [-100.0, -120.0, -130.0]
    assert out["cov_par_history"].shape == (4, 3)


def test_laplace_variant_warm_starts_and_flags_success(KS):
    o = KS.merge_opt(KS.OPT_OAT, {"maxknot": 5, "tol_knot": 0.5})
    fit = ScriptedFit([-100.0, -90.0, -80.0], laplace=True)
    out = KS.oat_core(fit, _propose_rows([[5, 5], [6, 6]]), START, XU0, MUU0, o, laplace=True,
                      ff=np.zeros(4))
    assert np.array_equal(fit.calls[0]["ff"], np.zeros(4))
    assert np.array_equal(fit.calls[1]["ff"], np.zeros(4))       # the first fit's fmax (k = 0)
    assert np.array_equal(fit.calls[2]["ff"], np.ones(4))        # the accepted fmax
    assert out["success"] is True and np.array_equal(out["fmax"], np.full(4, 2.0))
    # a NotPositiveDefinite ascent is the try-error branch: the previous fit stays, its
    # objective repeats, the margin is 0 and chooseK ends the loop
    fit = ScriptedFit([-100.0, -90.0, -80.0], laplace=True, fail_at={1})
    out = KS.oat_core(fit, _propose_rows([[5, 5], [6, 6]]), START, XU0, MUU0, o, laplace=True,
                      ff=np.zeros(4))
    assert out["success"] is False and out["xu"].shape == (3, 2)
    assert list(out["obj_fun"]) == [-100.0, -100.0] and list(out["ga_steps"]) == [10, 10]


def test_core_matches_the_line_by_line_loop_over_the_oracle_drivers(KS):
    G = O.make_gaussian_problem("C2", n=60, m=3)
    o = KS.merge_opt(KS.OPT_OAT_NORM_VI, {"maxknot": 5, "maxit": 3, "obj_tol": 0.0,
                                          "tol_knot": -1e9})
    fit = OO.oracle_fit("vi", G["cov_fun"], G["X"], G["y"], G["mu"], o)
    rows = [G["X"][40], G["X"][50]]
    muu = np.full(3, G["y"].mean())
    got = KS.oat_core(fit, _propose_rows(rows), G["cov_par"], G["U"], muu, o)
    ref = OO.oat_loop(fit, _propose_rows(rows), G["cov_par"], G["U"], muu, o)
    assert ref["shape"] in got and got["xu"].shape == (5, 3)
    for k in ("xu", "obj_fun", "cov_par_history", "ga_steps", "u_mean", "u_var", "muu"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(ref[k])), k
    # OAT's grad_tol = 1 reached the driver: with obj_tol = 0 every fit runs to maxit
    assert list(got["ga_steps"]) == [3, 3, 3]
    assert not np.array_equal(got["xu"][3], rows[0])        # cov_diff: the appended knot moved
    # ... and only it: the others only make the round trip through the bounded transform, whose
    # 1e-4 offsets (covariance_function_derivatives.R:191-197) shift them by that order
    assert np.allclose(got["xu"][:3], G["U"], rtol=0, atol=1e-3)


def test_defaults_are_the_references(KS):
    from sparsergps_amd import proposals as P
    vi, nm, lp = KS.OPT_OAT_NORM_VI, KS.OPT_OAT_NORM, KS.OPT_OAT
    for o in (vi, nm, lp):                                   # vi_functions.R:1383-1393
        assert o["eta"] == 1e3 and o["grad_tol"] == 1 and o["maxit"] == 1000
        assert o["ego_cov_par"] == {"sigma": 3.0, "l": 1.0, "tau": 1e-3}
        assert o["ego_cov_fun"] == "exp" and o["cov_diff"] is True and o["chooseK"] is True
        assert o["maxknot"] == 30 and o["TTmin"] == 10 and o["delta"] == 1e-6
    assert (vi["obj_tol"], vi["tol_knot"], vi["TTmax"]) == (1e-3, 1e-3, 40)
    assert (nm["obj_tol"], nm["tol_knot"], nm["TTmax"]) == (1e-3, 1e-3, 40)   # oat_knot_selection.R:354-362
    assert (lp["obj_tol"], lp["tol_knot"], lp["TTmax"], lp["tol_nr"]) == (1e-2, 1e-1, 30, 1e-5)  # l.67-75
    assert "tol_nr" not in vi and "tol_nr" not in nm
    # the random proposals: vi_functions.R:2132-2135; knot_proposal_functions.R:1200-1203, 1030-1033
    for o in (P.OPT_RANDOM_NORM_VI, P.OPT_RANDOM_NORM, P.OPT_RANDOM):
        assert (o["eta"], o["grad_tol"], o["tol_knot"], o["TTmax"], o["obj_tol"]) == (0.8, 1e-1, 1e-1, 40, 1e-3)
        assert "TTmin" not in o
    assert P.OPT_RANDOM["tol_nr"] == 1e-4 and "tol_nr" not in P.OPT_RANDOM_NORM_VI
    # unknown names are skipped; the merged opt reaches the proposal, which merges by name
    o = KS.merge_opt(vi, {"maxknot": 7, "no_such_name": 1})
    assert o["maxknot"] == 7 and "no_such_name" not in o
    assert P._merge_opt(P.OPT_EGO_NORM_VI, o)["ego_cov_par"]["tau"] == 1e-3
    assert P._merge_opt(P.OPT_RANDOM_NORM_VI, o)["grad_tol"] == 1


def test_random_proposal_returns_the_best_or_the_first_knot():
    from sparsergps_amd import proposals as P
    rng = np.random.default_rng(3)
    xy = rng.uniform(size=(30, 2))
    xu = xy[:3].copy()
    score = lambda c: np.asarray(c)[:, 0] * 10.0            # noqa: E731
    o = {"TTmax": 6}
    tr, tr2 = [], []
    got = P.random_proposal(xy, xu, score, 1.0, o, rng=np.random.default_rng(5), trace=tr)
    ref = OO.random_proposal(xy, xu, score, 1.0, 6, rng=np.random.default_rng(5), trace=tr2)
    assert np.array_equal(got, ref) and got.shape == (1, 2)
    rows = tr[0]["rows"]
    assert len(set(rows)) == 6 and min(rows) >= 3            # outside the knots, no repeats
    assert np.array_equal(got[0], xy[rows[np.argmax(xy[rows, 0])]])
    # no candidate beats the current objective: which.max is 1, the FIRST EXISTING KNOT
    got = P.random_proposal(xy, xu, score, 1e6, o, rng=np.random.default_rng(5))
    assert np.array_equal(got, xu[:1])
    assert np.array_equal(OO.random_proposal(xy, xu, score, 1e6, 6, rng=np.random.default_rng(5)), xu[:1])
    # ... a tie with it too (which.max: first of equals)
    best = float(np.max(score(xy[rows])))
    assert np.array_equal(P.random_proposal(xy, xu, score, best, o, init_rows=rows), xu[:1])
    # a NaN score is resampled: a random row outside the knots plus N(0, 1e-6^2)
    calls = []

    def flaky(c):
        calls.append(len(c))
        v = score(c)
        if len(calls) == 1:
            v[2] = math.nan
        return v
    got = P.random_proposal(xy, xu, flaky, -1e6, o, rng=np.random.default_rng(5))
    assert calls == [6, 1] and got.shape == (1, 2)           # one batched call, one resample


def test_scan_oracle_matches_the_dense_restatement():
    for cov_fun, family, seed in (("sqexp", "gaussian", 0), ("ard", "poisson", 1)):
        Pc = OO.scan_recipe(40, 3, 6, cov_fun, seed)
        for mode in ("var", "error"):
            ref = OO.fit_scan(Pc["X"], Pc["mu"], Pc["cov_par"], cov_fun, Pc["xu"], Pc["u_mean"],
                              Pc["u_var"], Pc["muu"], mode, family, f=Pc["f"])
            dn = OO.fit_scan_dense(Pc["X"], Pc["mu"], Pc["cov_par"], cov_fun, Pc["xu"],
                                   Pc["u_mean"], Pc["u_var"], Pc["muu"], family)
            assert np.max(np.abs(dn["mean"] - ref["mean"])) <= 1e-12 * np.max(np.abs(ref["mean"]))
            assert np.max(np.abs(dn["var"] - ref["var"])) <= 1e-11 * np.max(np.abs(ref["var"]))
            key = np.abs(np.exp(Pc["f"]) - np.exp(dn["mean"])) if mode == "error" else dn["var"]
            assert int(np.argmax(key)) == ref["row"]
    # excluded rows never win and carry NaN keys
    ref = OO.fit_scan(Pc["X"], Pc["mu"], Pc["cov_par"], "ard", Pc["xu"], Pc["u_mean"], Pc["u_var"],
                      Pc["muu"], "var", "poisson", excl=Pc["X"][[ref["row"]]])
    assert np.isnan(ref["key"]).sum() == 1 and not ref["excluded"][ref["row"]]
