"""sgp_ego_scan (the EGO proposals' expected-improvement scan, k_ego.hip) and the three
knot_prop_ego* wrappers on the GPU, against the numpy oracle tests/ego_oracle.py.

Bars (tests/test_gpu_predict_edges.py's): mean and var on EVERY row within 1e-8 s, s the entry's
magnitude budget (|v1| + sum |k_ij| |alpha_j|; sigma^2 + tau^2 + sum |k_ij| |A_jk| |k_ik|), with
cond(K22) <= 4e4 asserted per case (fp64 forward error ~ 4e4 * 2^-53 ~ 5e-12 s).  EI is held to
the bound those two propagate to, Phi(z) 1e-8 s_mean + phi(z) / (2 sqrt var) 1e-8 s_var +
1e-8 max EI_ref, on the rows with var_ref >= 1e-3 sigma^2 (on a meta point var ~ delta and
d EI / d var is unbounded); at most T + n / 50 rows may be left out.  best_row: the oracle's EI
at the returned row is within that bound of the oracle's maximum, and the index is equal where
the oracle's top-two relative gap is >= 1e-6.

Shapes (n, d, T, kernel): one row; T = 1 (alpha = 0: every mean equals v1, a near-tie decided by
var alone); T = 16 / 17 (the padded meta-model's 16-column edge); d = 1; d = 8, T = 40 (the
defaults' last scan); d = 12, T = 65 (A too large for LDS beside the rest: streamed from L2);
d = 32, T = 128 (both limits); n from one 64-row step to 32 of them.

Largest measured on an MI355X over the nine shapes: |d mean| / s 2.6e-16 (d = 1), |d var| / s
6.6e-15 (T = 128), |d EI| / bound 2.4e-7 (T = 65); every winner is the oracle's row.
"""
import functools
import math

import numpy as np
import pytest

import ego_oracle as E

pytestmark = pytest.mark.gpu
RTOL = 1e-8
COND_MAX = 4e4
SIGMA, DELTA = 3.0, 1e-6

# (n, d, T, kernel, l, tau)
SHAPES = [(1, 3, 5, "exp", 1.0, 0.0), (129, 2, 1, "exp", 1.0, 0.0), (257, 3, 16, "exp", 1.0, 0.0),
          (300, 3, 17, "sqexp", 1.5, 0.3), (513, 1, 15, "exp", 2.0, 0.0),
          (1000, 8, 40, "exp", 3.0, 0.0), (640, 12, 65, "exp", 6.0, 0.2),
          (2000, 32, 128, "exp", 16.0, 0.0), (1500, 5, 64, "sqexp", 2.0, 0.5)]


@pytest.fixture(scope="module")
def sgp():
    import sparsergps_amd as S
    from sparsergps_amd import _lib
    _lib.require_gpu()
    return S


@functools.lru_cache(maxsize=None)
def _case(n, d, T, kernel, l, tau, excl_winner=False):
    X, xm, v = E.recipe(n, d, T)
    par = {"sigma": SIGMA, "l": l, "tau": tau}
    excl = None
    if excl_winner:
        excl = X[[_case(n, d, T, kernel, l, tau)[4]["row"]]]
    ref = E.scan(X, xm, v, par, kernel, DELTA, excl)
    for a in (X, xm, v, *[x for x in ref.values() if isinstance(x, np.ndarray)]):
        a.setflags(write=False)
    return X, xm, v, par, ref, excl


def _ctx(sgp, X, **kw):
    n = X.shape[0]
    return sgp.SparseGPContext(X, np.zeros(n), np.zeros(n), m_max=8, **kw)


def _check_against(ref, got, n, T, by_value_only=False):
    """mean / var everywhere, EI and the winner under the propagated bound; returns the figures."""
    assert ref["cond"] <= COND_MAX, ref["cond"]
    e_mean = np.max(np.abs(got["mean"] - ref["mean"]) / ref["s_mean"])
    e_var = np.max(np.abs(got["var"] - ref["var"]) / ref["s_var"])
    bound, on = E.ei_bound(ref, SIGMA, RTOL)
    left_out = int(np.sum(~on & ~ref["excluded"]))
    e_ei = float(np.max((np.abs(got["ei"] - ref["ei"]) / bound)[on])) if on.any() else 0.0
    gap = E.top_two_gap(ref["ei"])
    print(f"n={n} T={T}: cond {ref['cond']:.3g}, max |d mean|/s {e_mean:.2e}, |d var|/s {e_var:.2e}, "
          f"|d EI|/bound {e_ei:.2e}, left out {left_out}, top-two gap {gap:.2e}, "
          f"row {got['row']} (oracle {ref['row']})")
    assert e_mean <= RTOL and e_var <= RTOL
    assert left_out <= T + n / 50
    assert e_ei <= 1.0
    assert np.array_equal(np.isnan(got["ei"]), ref["excluded"])
    r = got["row"]
    assert 0 <= r < n and not ref["excluded"][r]
    # on a left-out row (var ~ delta) EI is within rounding of 0 on both sides
    slack = bound[r] if on[r] else RTOL * np.nanmax(ref["ei"])
    assert ref["ei"][r] >= np.nanmax(ref["ei"]) - slack
    assert abs(got["ei_best"] - got["ei"][r]) == 0.0
    if gap >= 1e-6 and not by_value_only:
        assert r == ref["row"]
    return gap


def _scan(ctx, par, kernel, xm, v, excl=None, delta=DELTA, want=("ei", "mean", "var")):
    out = ctx.ego_scan(par, kernel, xm, v, excl=excl, delta=delta, want=want)
    res = ctx.ego_scan(par, kernel, xm, v, excl=excl, delta=delta, want=())
    # the optional vectors do not change the winner
    assert res["row"] == out["row"] and res["best_ei"] == out["best_ei"] and len(res) == 2
    out["ei_best"] = out["best_ei"]
    return out


@pytest.mark.parametrize("n,d,T,kernel,l,tau", SHAPES)
def test_scan_matches_oracle(sgp, n, d, T, kernel, l, tau):
    X, xm, v, par, ref, _ = _case(n, d, T, kernel, l, tau)
    with _ctx(sgp, X) as ctx:
        got = _scan(ctx, par, kernel, xm, v)
    # (129, 2, 1): v - v1 = 0, so every mean is v1 and the winner is decided by var alone
    # (top-two gap ~ 1e-14): checked by value only
    gap = _check_against(ref, got, n, T, by_value_only=(T == 1))
    if T > 1 and n > 1:
        assert gap >= 1e-6, gap               # the shapes were chosen with gaps >= 2e-3


@pytest.mark.parametrize("n,d,T,kernel,l,tau", [SHAPES[2], SHAPES[5], SHAPES[8]])
def test_excluding_the_winner_returns_the_runner_up(sgp, n, d, T, kernel, l, tau):
    X, xm, v, par, ref0, _ = _case(n, d, T, kernel, l, tau)
    _, _, _, _, ref, excl = _case(n, d, T, kernel, l, tau, True)
    assert ref["row"] != ref0["row"] and ref["excluded"].sum() == 1
    near = X[[ref["row"], 3]].copy()
    if d > 1:
        near[:, 1:] += 0.25       # equal to a row in coordinate 0 only: excludes nothing
        excl = np.vstack([near[:1], excl, near[1:]])
    with _ctx(sgp, X) as ctx:
        got = _scan(ctx, par, kernel, xm, v, excl=excl)
        _check_against(ref, got, n, T)
        none = _scan(ctx, par, kernel, xm, v, excl=None)
        _check_against(ref0, none, n, T)
        if d > 1:
            only0 = _scan(ctx, par, kernel, xm, v, excl=near)
            assert only0["row"] == none["row"] and not np.isnan(only0["ei"]).any()


def test_every_row_excluded_is_einval(sgp):
    X, xm, v, par, ref, _ = _case(*SHAPES[1])
    with _ctx(sgp, X) as ctx:
        with pytest.raises(sgp.SGPError) as ei:
            ctx.ego_scan(par, "exp", xm, v, excl=X[::-1])
        assert ei.value.status == 1 and "no data row outside the knots" in str(ei.value)
        got = _scan(ctx, par, "exp", xm, v, excl=X[1:])     # all but row 0
        assert got["row"] == 0 and np.isnan(got["ei"][1:]).all()


def test_long_exclusion_list(sgp):
    """Most rows excluded (a list of 2105, eleven search steps deep): the winner is among the
    excluded, and five list entries match no row."""
    n, d, T = 2500, 3, 16
    X, xm, v = E.recipe(n, d, T)
    par = {"sigma": SIGMA, "l": 1.0, "tau": 0.0}
    ref0 = E.scan(X, xm, v, par, "exp", DELTA)
    idx = np.random.default_rng(4).permutation(n)[:2100]
    idx[0] = ref0["row"]
    excl = np.vstack([X[idx], X[idx[:5]] + 1e-9])
    ref = E.scan(X, xm, v, par, "exp", DELTA, excl)
    assert ref["excluded"].sum() == np.unique(idx).size >= 2099 and ref["row"] != ref0["row"]
    with _ctx(sgp, X) as ctx:
        _check_against(ref, _scan(ctx, par, "exp", xm, v, excl=excl), n, T)


def test_edges_tmax_notpd_repeat(sgp):
    X, xm, v, par, ref, _ = _case(*SHAPES[3])
    n, d, T = SHAPES[3][:3]
    rng = np.random.default_rng(2)
    with _ctx(sgp, X) as ctx:
        with pytest.raises(sgp.SGPError) as e129:
            ctx.ego_scan(par, "sqexp", rng.uniform(0, 10, (129, d)), np.arange(129.0))
        assert e129.value.status == 1 and "T=129" in str(e129.value)
        with pytest.raises(ValueError, match="ego_cov_fun"):
            ctx.ego_scan({"sigma": 3.0, "l": 1.0, "tau": 0.0}, "ard", xm, v)
        # two identical meta rows, tau = 0, delta_meta = 0: K22 is singular -- with sigma = 3 the
        # first pivot is exactly 9, its factor exactly 3 and the second pivot exactly 0
        dup = np.vstack([xm[:1], xm])
        vd = np.r_[v[0], v]
        with pytest.raises(sgp.NotPositiveDefinite) as enp:
            ctx.ego_scan({"sigma": 3.0, "l": 1.5, "tau": 0.0}, "sqexp", dup, vd, delta=0.0)
        assert "meta-model K22" in str(enp.value)
        a = _scan(ctx, par, "sqexp", xm, v)                  # the next call is right ...
        _check_against(ref, a, n, T)
        b = _scan(ctx, par, "sqexp", xm, v)                  # ... and a repeat is bit-identical
        for k in ("ei", "mean", "var"):
            assert np.array_equal(a[k], b[k], equal_nan=True)
        assert a["row"] == b["row"] and a["ei_best"] == b["ei_best"]


def test_scan_leaves_a_completed_evaluation_alone(sgp):
    from sparsergps_amd.workloads import make_gaussian_problem
    P = make_gaussian_problem("C2", n=700, m=20)
    th = np.array(list(P["cov_par"].values()))
    _, xm, v = E.recipe(700, 3, 9)
    with sgp.SparseGPContext(P["X"], P["y"], P["mu"], m_max=21) as ctx:
        obj, g = ctx.eval_vi(th, "sqexp", P["U"], P["delta"])
        um0, uv0 = ctx.posterior_u(np.zeros(20))
        res = ctx.ego_scan({"sigma": 3.0, "l": 1.0, "tau": 0.0}, "exp", P["X"][:9], v, excl=P["U"])
        ref = E.scan(P["X"], P["X"][:9], v, {"sigma": 3.0, "l": 1.0, "tau": 0.0}, "exp", DELTA, P["U"])
        assert res["row"] == ref["row"] or E.top_two_gap(ref["ei"]) < 1e-6
        um1, uv1 = ctx.posterior_u(np.zeros(20))
        assert np.array_equal(um0, um1) and np.array_equal(uv0, uv1)
        obj2, g2 = ctx.eval_vi(th, "sqexp", P["U"], P["delta"])
        assert obj2 == obj and np.array_equal(g, g2)


def test_three_shards_equal_one_device(sgp):
    n, d, T, kernel, l, tau = SHAPES[5]
    X, xm, v, par, ref, _ = _case(n, d, T, kernel, l, tau)
    excl = X[[5, 400, 999]]
    with _ctx(sgp, X) as one, _ctx(sgp, X, devices=[0, 0, 0]) as tri:
        assert tri.shards() == (3, 1)
        a = one.ego_scan(par, kernel, xm, v, excl=excl)
        b = tri.ego_scan(par, kernel, xm, v, excl=excl)
        assert a["row"] == b["row"] and a["row"] == E.scan(X, xm, v, par, kernel, DELTA, excl)["row"]
        assert abs(a["ei"][a["row"]] - b["ei"][b["row"]]) <= 1e-12 * np.nanmax(ref["ei"])
        assert np.all(np.abs(a["mean"] - b["mean"]) <= 1e-12 * ref["s_mean"])
        assert np.all(np.abs(a["var"] - b["var"]) <= 1e-12 * ref["s_var"])
        assert np.array_equal(np.isnan(a["ei"]), np.isnan(b["ei"]))
        assert np.isnan(b["ei"][[5, 400, 999]]).all()
        ok = ~np.isnan(a["ei"])
        bound, _ = E.ei_bound(ref, SIGMA, 1e-12)
        assert np.all(np.abs(a["ei"] - b["ei"])[ok] <= bound[ok] + 1e-12 * np.nanmax(ref["ei"]))
        with pytest.raises(sgp.SGPError) as e:
            tri.ego_scan(par, kernel, xm, v, excl=X)
        assert "no data row outside the knots" in str(e.value)


# ------------------------------------------------------------------ the proposals
def _fixed_fit(x, vals, start, cov_fun, tau, delta):
    """A deterministic meta fit: smooth in the scores, so last-bit differences between a batched
    and a one-by-one scorer cannot move it.  The length scale grows with d: on [0, 10]^5 the L1
    distances are ~15, and l = 1.5 leaves k ~ e^-10 on most rows with their EI tied to 1e-9."""
    return np.log([vals.max() - vals.min() + 1.0, 1.5 if x.shape[1] <= 2 else 12.0])


def _gauss(n=300, d=2, m=8):
    rng = np.random.default_rng(42)
    X = rng.uniform(0, 10, size=(n, d))
    y = np.sin(X).sum(axis=1) + rng.normal(0, 0.5, n)
    xu = X[rng.choice(n, m, replace=False)].copy()
    from collections import OrderedDict
    return {"xy": X, "xu": xu, "cov_fun": "sqexp", "mu": np.full(n, y.mean()),
            "cov_par": OrderedDict([("sigma", 1.0), ("l", 1.0), ("tau", 0.5)])}, y


def _oracle_run(fit, scorer, o, init, rng=None):
    tr = []
    ref = E.proposal_loop(fit["xy"], fit["xu"], scorer, o, rng=rng, init_rows=init,
                          meta_fit=_fixed_fit, trace=tr)
    for t in tr:
        assert t["gap"] >= 1e-4, tr      # every scan's winner is decided beyond rounding
    return ref, [t["row"] for t in tr]


def test_knot_prop_ego_norm_vi_takes_the_oracle_loops_steps(sgp):
    from sparsergps_amd import proposals as P
    fit, y = _gauss()
    opt = {"TTmin": 4, "TTmax": 7}
    o = P._merge_opt(P.OPT_EGO_NORM_VI, opt)
    init = [3, 77, 150, 299]
    th = np.array(list(fit["cov_par"].values()))
    with sgp.SparseGPContext(fit["xy"], y, fit["mu"], m_max=9) as ctx:
        scorer = lambda c: ctx.vi_candidates(th, "sqexp", fit["xu"], c, o["delta"])   # noqa: E731
        ref, rows = _oracle_run(fit, scorer, o, init)
        tr = []
        got = sgp.knot_prop_ego_norm_vi(fit, opt, ctx=ctx, init_rows=init, meta_fit=_fixed_fit,
                                        trace=tr)
    assert len(rows) == 4 and [t["row"] for t in tr] == rows[:-1]
    assert got.shape == (1, 2) and np.array_equal(got, ref)
    # with y instead of a context, and the default scipy fit: a data row outside the knots
    got2 = sgp.knot_prop_ego_norm_vi(fit, {"TTmin": 3, "TTmax": 4}, y=y,
                                     rng=np.random.default_rng(1))
    hit = (fit["xy"] == got2).all(axis=1)
    assert hit.sum() == 1 and not (fit["xu"][:, None, :] == got2[None]).all(axis=2).any()


def test_knot_prop_ego_norm_fitc(sgp):
    from sparsergps_amd import proposals as P
    fit, y = _gauss()
    opt = {"TTmin": 3, "TTmax": 5}
    o = P._merge_opt(P.OPT_EGO_NORM, opt)
    init = [10, 120, 250]
    th = np.array(list(fit["cov_par"].values()))
    with sgp.SparseGPContext(fit["xy"], y, fit["mu"], m_max=9) as ctx:
        scorer = lambda c: ctx.fitc_candidates(th, "sqexp", fit["xu"], c, o["delta"])   # noqa: E731
        ref, rows = _oracle_run(fit, scorer, o, init)
        tr = []
        got = sgp.knot_prop_ego_norm(fit, opt, ctx=ctx, init_rows=init, meta_fit=_fixed_fit, trace=tr)
    assert [t["row"] for t in tr] == rows[:-1] and np.array_equal(got, ref)


def test_knot_prop_ego_poisson_laplace(sgp):
    from sparsergps_amd import proposals as P
    from sparsergps_amd.workloads import make_poisson_problem
    Q = make_poisson_problem(n=300, m=8)
    xu = Q["X"][np.random.default_rng(8).choice(300, 8, replace=False)].copy()
    th = np.array(list(Q["cov_par"].values()))
    opt = {"TTmin": 3, "TTmax": 5}
    o = P._merge_opt(P.OPT_EGO, opt)
    init = [10, 120, 250]
    with sgp.SparseGPContext(Q["X"], Q["y"], Q["mu"], m_max=9) as ctx:
        ctx.lap_set_f(Q["f0"])
        ctx.lap_nr(th, "sqexp", xu, Q["delta"], 1.0, o["tol_nr"], o["maxit_nr"])
        fit = {"xy": Q["X"], "xu": xu, "cov_fun": "sqexp", "mu": Q["mu"], "cov_par": Q["cov_par"],
               "fmax": ctx.lap_get_f()}
        scorer = lambda c: ctx.lap_candidates(th, "sqexp", xu, c, o["delta"], 1.0,   # noqa: E731
                                              o["tol_nr"], o["maxit_nr"])
        ref, rows = _oracle_run(fit, scorer, o, init)
        tr = []
        got = sgp.knot_prop_ego(fit, opt, ctx=ctx, m=1.0, init_rows=init, meta_fit=_fixed_fit,
                                trace=tr)
        assert np.array_equal(ctx.lap_get_f(), fit["fmax"])     # the scorer restores the mode
    assert [t["row"] for t in tr] == rows[:-1] and np.array_equal(got, ref)


def test_a_failing_scorer_takes_the_resample_branch(sgp):
    """The scorer stub returns NaN once, on the first EI-chosen candidate: the product (device
    scan) and the oracle loop draw the same replacement from the injected generator."""
    from sparsergps_amd import proposals as P
    fit, y = _gauss()
    o = P._merge_opt(P.OPT_EGO_NORM_VI, {"TTmin": 4, "TTmax": 6})
    init = [3, 77, 150, 299]
    th = np.array(list(fit["cov_par"].values()))
    with sgp.SparseGPContext(fit["xy"], y, fit["mu"], m_max=9) as ctx:
        def stub():
            calls = {"n": 0}

            def scorer(c):
                out = ctx.vi_candidates(th, "sqexp", fit["xu"], c, o["delta"]).copy()
                for k in range(out.size):
                    calls["n"] += 1
                    if calls["n"] == 5:
                        out[k] = np.nan
                return out
            return scorer, calls
        so, co = stub()
        ref, rows = _oracle_run(fit, so, o, init, rng=np.random.default_rng(9))
        sp, cp = stub()
        scan = lambda par, cf, x, v: ctx.ego_scan(par, cf, x, v, excl=fit["xu"],   # noqa: E731
                                                  delta=o["delta"], want=())["row"]
        got = P.ego_proposal(fit["xy"], fit["xu"], sp, scan, o, rng=np.random.default_rng(9),
                             init_rows=init, meta_fit=_fixed_fit)
    assert cp["n"] == co["n"] == 4 + 2 + 1
    assert np.array_equal(got, ref)
