"""The batched Laplace path on the GPU against the literal oracle
(O.newtrap_sparseGP / O.dlogq_dcov_par, tests/bern_oracle.py) at the bars
tests/test_gpu_bernoulli.py holds the context route to: exact NR iteration count, NR objectives
rtol 1e-9, mode 1e-8 absolute, objective and gradient 1e-6 relative, posterior_u rtol 1e-6 with
atol 1e-7; prediction within 1e-8 of the largest reference magnitude; and the batch's
independence rules bit for bit.  The cases and their references are tests/batch_laplace_cases.py's
(seeds with both stop margins >= 1e-3, asserted in tests/test_batch_laplace_model.py)."""
from collections import OrderedDict

import numpy as np
import pytest

import batch_laplace_cases as LC
import bern_oracle as BO
from oracle import drivers as OD
from oracle import sgp_oracle as O

pytestmark = pytest.mark.gpu
EVAL_RTOL = 1e-6


@pytest.fixture(scope="module")
def sgp():
    import sparsergps_amd as S
    from sparsergps_amd import _lib
    _lib.require_gpu()
    return S


def _open(sgp, P, f0=None):
    b = sgp.SparseGPBatch(P["X"], P["y"], P["mu"])
    b.lap_init(P["family"], P["expo"])
    b.set_f([P["f0"] if f0 is None else f0])
    return b


def _grad_vec(P, g):
    return np.array([g[k] for k in P["cov_par"]])


def _rel(a, b):
    return np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))


@pytest.mark.parametrize("family,name", LC.all_cases())
def test_matches_oracle(sgp, family, name):
    """Measured on the MI355X (DESIGN.md sec. 0s has the table): see the printed figures."""
    P, nr, g_ref = LC.reference(family, name)
    ov = nr["objective_function_values"]
    with _open(sgp, P) as b:
        obj, grads, st, it = b.eval_laplace([P["cov_par"]], P["cov_fun"], [P["U"]], P["delta"],
                                            tol=LC.TOL, maxit=LC.MAXIT)
        objs, f = b.lap_objective_values(0), b.get_f()[0]
        um, uv = b.posterior_u([np.zeros(P["U"].shape[0])])
    g = _grad_vec(P, grads[0])
    k = min(len(ov), len(objs))
    print(family, name, "iters", int(it[0]), len(ov), "objectives",
          np.max(np.abs(objs[:k] - ov[:k]) / np.abs(ov[:k])), "mode", np.max(np.abs(f - nr["gp"])),
          "objective", abs(obj[0] - ov[-1]) / abs(ov[-1]), "gradient", _rel(g, g_ref),
          "u_mean", np.max(np.abs(um[0] - nr["u_posterior_mean"])),
          "u_var", np.max(np.abs(uv[0] - nr["u_posterior_variance"])))
    assert st[0] == 0 and it[0] == len(ov) < LC.MAXIT
    np.testing.assert_allclose(objs, ov, rtol=1e-9, atol=0.0)
    assert np.max(np.abs(f - nr["gp"])) < 1e-8
    assert obj[0] == objs[-1] and abs(obj[0] - ov[-1]) / abs(ov[-1]) < EVAL_RTOL
    assert _rel(g, g_ref) < EVAL_RTOL
    np.testing.assert_allclose(um[0], nr["u_posterior_mean"], rtol=EVAL_RTOL, atol=1e-7)
    np.testing.assert_allclose(uv[0], nr["u_posterior_variance"], rtol=EVAL_RTOL, atol=1e-7)


# ------------------------------------------------------------------ prediction
PRED_M = [1, 15, 16, 17, 33, 64]
PRED_ROWS = [1, 63, 64, 65, 1100]


def _pred_problem(family, m):
    P = dict(LC.problem(family, "mixed3"))           # 63 rows, d = 3, sqexp
    g = np.random.Generator(np.random.PCG64(4400 + m))
    P["U"] = g.uniform(0.0, 10.0, size=(m, 3))
    return P


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("m", PRED_M)
def test_predict_matches_oracle(sgp, family, m):
    P = _pred_problem(family, m)
    muu = np.zeros(m)
    nr = LC.newtrap(P, muu=muu)
    g = np.random.Generator(np.random.PCG64(4500 + m))
    B = len(PRED_ROWS)
    Xt = g.uniform(0.0, 10.0, size=(sum(PRED_ROWS), 3))
    mut = g.normal(size=Xt.shape[0])
    t0 = np.concatenate([[0], np.cumsum(PRED_ROWS)[:-1]])
    n = P["y"].size
    with sgp.SparseGPBatch(P["X"], P["y"], P["mu"], [0] * B, [n] * B) as b:   # B aliases
        b.lap_init(family, P["expo"])
        b.set_f([P["f0"]] * B)
        _, _, st, it = b.eval_laplace([P["cov_par"]] * B, "sqexp", [P["U"]] * B, P["delta"],
                                      tol=LC.TOL, obj_only=True)
        assert not st.any() and set(it) == {len(nr["objective_function_values"])}
        b.set_test(Xt, None, mut, t0, PRED_ROWS)
        pred = b.predict()
    worst = [0.0, 0.0]
    for q, (r0, nr_) in enumerate(zip(t0, PRED_ROWS)):
        ref = O.predict_laplace(nr["u_posterior_mean"], nr["u_posterior_variance"], P["U"],
                                Xt[r0:r0 + nr_], "sqexp", P["cov_par"], mut[r0:r0 + nr_], muu,
                                family=family, delta=P["delta"])
        for k, key in enumerate(("pred_mean", "pred_var")):
            want = np.asarray(ref[key]).reshape(-1)
            err = np.max(np.abs(pred[q][key].reshape(-1) - want)) / np.max(np.abs(want))
            worst[k] = max(worst[k], err)
            assert err < 1e-8, (q, key, err)
    print(family, m, "pred_mean", worst[0], "pred_var", worst[1])


# ------------------------------------------------------------------ the context route
@pytest.mark.parametrize("family,name", [("poisson", "mixed4"), ("poisson", "mixed9"),
                                         ("bernoulli", "mixed5"), ("bernoulli", "coincident16")])
def test_matches_the_context_route(sgp, family, name):
    P, nr, _ = LC.reference(family, name)
    th = np.array(list(P["cov_par"].values()))
    m = P["U"].shape[0]
    with sgp.SparseGPContext(P["X"], P["y"], P["mu"], m_max=m) as c:
        c.lap_set_family(family)
        c.lap_set_f(P["f0"])
        expo = 1.0
        if family == "poisson":
            c.lap_set_expo(P["expo"])
            expo = sgp._lib.SGP_EXPO_ROWS
        o, g, it = c.eval_laplace(th, P["cov_fun"], P["U"], P["delta"], expo, LC.TOL, LC.MAXIT)
        ov, f, post = c.lap_objective_values(), c.lap_get_f(), c.posterior_u(np.zeros(m))
    with _open(sgp, P) as b:
        obj, grads, st, nit = b.eval_laplace([P["cov_par"]], P["cov_fun"], [P["U"]], P["delta"],
                                             tol=LC.TOL, maxit=LC.MAXIT)
        objs, fb = b.lap_objective_values(0), b.get_f()[0]
        um, uv = b.posterior_u([np.zeros(m)])
    gb = np.array([grads[0][k] for k in sgp.vi.param_names(P["cov_fun"], P["X"].shape[1])])
    assert st[0] == 0 and nit[0] == it
    np.testing.assert_allclose(objs, ov, rtol=1e-9, atol=0.0)
    assert np.max(np.abs(fb - f)) < 1e-8
    assert abs(obj[0] - o) / abs(o) < EVAL_RTOL and _rel(gb, np.asarray(g)) < EVAL_RTOL
    np.testing.assert_allclose(um[0], post[0], rtol=EVAL_RTOL, atol=1e-7)
    np.testing.assert_allclose(uv[0], post[1], rtol=EVAL_RTOL, atol=1e-7)


# ------------------------------------------------------------------ independence, bit for bit
TRIO = ["mixed3", "mixed6", "mixed9"]      # d = 3, sqexp: 63 / 1000 / 1061 rows, 17 / 64 / 30 knots


def _trio(family):
    return [LC.problem(family, n) for n in TRIO]


def _open_many(sgp, Ps, order=None):
    order = list(range(len(Ps))) if order is None else order
    Ps = [Ps[i] for i in order]
    expo = None if Ps[0]["expo"] is None else [P["expo"] for P in Ps]
    b = sgp.SparseGPBatch.from_problems([(P["X"], P["y"], P["mu"]) for P in Ps])
    b.lap_init(Ps[0]["family"], None if expo is None else np.concatenate(expo))
    b.set_f([P["f0"] for P in Ps])
    return b, Ps


def _run(b, Ps, active=None, delta=1e-6, cps=None):
    cps = [P["cov_par"] for P in Ps] if cps is None else cps
    obj, grads, st, it = b.eval_laplace(cps, "sqexp", [P["U"] for P in Ps], delta, active=active,
                                        tol=LC.TOL)
    on = [active is None or bool(active[q]) for q in range(len(Ps))]
    fs = b.get_f()
    out = []
    for q, P in enumerate(Ps):
        if not on[q]:
            out.append(None)
            continue
        out.append(dict(obj=obj[q], grad=np.array(list(grads[q].values())), st=int(st[q]),
                        it=int(it[q]), f=fs[q], objs=b.lap_objective_values(q)))
    ok = [q for q in range(len(Ps)) if on[q] and st[q] == 0]
    if ok:
        um, uv = b.posterior_u([np.zeros(P["U"].shape[0]) for P in Ps])
        for q in ok:
            out[q]["um"], out[q]["uv"] = um[q], uv[q]
    return out


def _same(a, b, keys=("obj", "grad", "it", "f", "objs", "um", "uv")):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_independence_bit_for_bit(sgp, family):
    Ps = _trio(family)
    b, _ = _open_many(sgp, Ps)
    with b:
        full = _run(b, Ps)
        b.set_f([P["f0"] for P in Ps])
        again = _run(b, Ps)                                    # a repeat from the same f
        # under `active`, with sentinels in the inactive slots
        b.set_f([P["f0"] for P in Ps])
        act = np.array([1, 0, 1], dtype=np.uint8)
        th = np.ones((3, 3))
        for q in (0, 2):
            th[q] = list(Ps[q]["cov_par"].values())
        obj, grad = np.full(3, -7.0), np.full((3, 3), -7.0)
        st, it = np.full(3, -7, dtype=np.int32), np.full(3, -7, dtype=np.int32)
        b.eval_laplace_raw("sqexp", th, [Ps[0]["U"], None, Ps[2]["U"]], 1e-6, 0, act, obj, grad,
                           st, LC.TOL, LC.MAXIT, it)
        fa = b.get_f()
    assert obj[1] == -7.0 and np.all(grad[1] == -7.0) and st[1] == -7 and it[1] == -7
    assert np.array_equal(fa[1], Ps[1]["f0"])                  # the inactive problem's f stands
    for q in (0, 2):
        assert obj[q] == full[q]["obj"] and np.array_equal(grad[q], full[q]["grad"])
        assert it[q] == full[q]["it"] and np.array_equal(fa[q], full[q]["f"])
    for q in range(3):
        assert full[q]["st"] == 0
        _same(full[q], again[q])
        with _open(sgp, Ps[q]) as one:                         # alone
            _same(full[q], _run(one, [Ps[q]])[0])
    rb, rPs = _open_many(sgp, Ps, [2, 1, 0])                   # reversed
    with rb:
        rev = _run(rb, rPs)
    for q in range(3):
        _same(full[q], rev[2 - q])


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_aliased_rows_under_different_theta(sgp, family):
    P = LC.problem(family, "mixed9")
    n = P["y"].size
    cps = [P["cov_par"], OrderedDict([("sigma", 0.9), ("l", 2.3), ("tau", 0.7)])]
    with sgp.SparseGPBatch(P["X"], P["y"], P["mu"], [0, 0], [n, n]) as b:
        b.lap_init(family, P["expo"])
        b.set_f([P["f0"], P["f0"]])
        both = _run(b, [P, P], cps=cps)
    for q in range(2):
        with _open(sgp, P) as one:
            _same(both[q], _run(one, [P], cps=[cps[q]])[0])
    assert both[0]["obj"] != both[1]["obj"]


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_neighbours_of_a_failing_problem(sgp, family):
    """Problem 1's knots 0 and 1 coincide and its tau^2 underflows to 0, so with delta = 0 its K22
    has a zero second pivot (exactly: sigma = 1 keeps the sweep's products exact): status +2, NaN
    results, and the neighbours' bits are those they have alone."""
    Ps = [dict(P) for P in _trio(family)]
    Ps[1]["U"] = Ps[1]["U"].copy()
    Ps[1]["U"][1] = Ps[1]["U"][0]
    cps = [P["cov_par"] for P in Ps]
    cps[1] = OrderedDict([("sigma", 1.0), ("l", 1.7), ("tau", 1e-170)])
    b, _ = _open_many(sgp, Ps)
    with b:
        got = _run(b, Ps, delta=0.0, cps=cps)
    assert got[1]["st"] == 2 and np.isnan(got[1]["obj"]) and np.all(np.isnan(got[1]["grad"]))
    for q in (0, 2):
        with _open(sgp, Ps[q]) as one:
            _same(got[q], _run(one, [Ps[q]], delta=0.0)[0])


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_vi_and_fitc_between_two_laplace_evaluations(sgp, family):
    Ps = _trio(family)
    cps, xus = [P["cov_par"] for P in Ps], [P["U"] for P in Ps]
    b, _ = _open_many(sgp, Ps)
    with b:
        first = _run(b, Ps)
        vi = b.eval_vi(cps, "sqexp", xus)
        fitc = b.eval_fitc(cps, "sqexp", xus)
        b.set_f([P["f0"] for P in Ps])
        second = _run(b, Ps)
    with sgp.SparseGPBatch.from_problems([(P["X"], P["y"], P["mu"]) for P in Ps]) as g:
        vi0 = g.eval_vi(cps, "sqexp", xus)                     # a batch that never saw Laplace
        fitc0 = g.eval_fitc(cps, "sqexp", xus)
    for q in range(3):
        _same(first[q], second[q])
        for a, c in ((vi, vi0), (fitc, fitc0)):
            assert a[0][q] == c[0][q] and list(a[1][q].values()) == list(c[1][q].values())


# ------------------------------------------------------------------ other behaviour
@pytest.mark.parametrize("family", LC.FAMILIES)
def test_warm_start(sgp, family):
    """A warm start takes no more iterations than the cold one and gives the same mode to 1e-8.
    Under Bernoulli (quirk Q19's W) the iteration converges linearly: at tol = 1e-6 the mode is
    itself only good to ~1e-6, and the reference's own warm run moves it by 3.6e-7
    (tests/test_batch_laplace_model.py), so both runs are made at tol = 1e-10 there."""
    P = LC.problem(family, "mixed3")
    tol = LC.TOL if family == "poisson" else 1e-10
    with _open(sgp, P) as b:
        _, _, st, cold = b.eval_laplace([P["cov_par"]], "sqexp", [P["U"]], tol=tol)
        f_cold = b.get_f()[0]
        _, _, st2, warm = b.eval_laplace([P["cov_par"]], "sqexp", [P["U"]], tol=tol)
        f_warm = b.get_f()[0]
    assert st[0] == 0 and st2[0] == 0 and 2 <= warm[0] <= cold[0] < LC.MAXIT
    assert np.max(np.abs(f_warm - f_cold)) < 1e-8


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_maxit_zero(sgp, family):
    P, nr, _ = LC.reference(family, "coincident48")
    g_ref = LC.gradient(P, P["f0"])
    with _open(sgp, P) as b:
        obj, grads, st, it = b.eval_laplace([P["cov_par"]], P["cov_fun"], [P["U"]], maxit=0)
        f = b.get_f()[0]
    o0 = nr["objective_function_values"][0]
    assert st[0] == 0 and it[0] == 1 and np.array_equal(f, P["f0"])
    assert abs(obj[0] - o0) / abs(o0) < EVAL_RTOL
    assert _rel(_grad_vec(P, grads[0]), g_ref) < EVAL_RTOL


def _ascent_problems(family):
    out = []
    # seeds whose five warm-started NR runs keep both stop margins >= 1e-3 in the oracle
    for i, (n, m, seed) in enumerate([(150, 6, 8100), (220, 9, 8111), (180, 12, 8102)]):
        g = np.random.Generator(np.random.PCG64(seed))
        X = g.uniform(0.0, 10.0, size=(n, 2))
        lat = 0.8 * np.sin(X).sum(axis=1) / np.sqrt(2.0)
        if family == "poisson":
            expo = g.uniform(0.5, 2.0, size=n)
            y = g.poisson(expo * np.exp(0.7 + lat)).astype(np.float64)
            f0, mu = np.full(n, np.log(y.mean())) - np.log(expo), np.full(n, 0.5)
        else:
            expo = None
            y = (g.uniform(size=n) < 1.0 / (1.0 + np.exp(-2.0 * lat))).astype(np.float64)
            f0, mu = np.zeros(n), np.zeros(n)
        out.append(dict(X=X, y=y, mu=mu, expo=expo, f0=f0, U=g.uniform(0.0, 10.0, size=(m, 2)),
                        cov_par=OrderedDict([("sigma", 1.1 + 0.1 * i), ("l", 1.7), ("tau", 0.5)])))
    return out


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_lockstep_ascent_matches_the_oracles_driver(sgp, family):
    Ps = _ascent_problems(family)
    opt = {"maxit": 5, "obj_tol": 0.0, "tol_nr": 1e-6}
    res = sgp.laplace_grad_ascent_batch(
        [P["cov_par"] for P in Ps], "sqexp", [P["U"] for P in Ps],
        [(P["X"], P["y"], P["mu"]) for P in Ps], [np.zeros(P["U"].shape[0]) for P in Ps], opt,
        family=family, expo=None if family == "bernoulli" else [P["expo"] for P in Ps],
        ff=[P["f0"] for P in Ps])
    for P, got in zip(Ps, res):
        muu = np.zeros(P["U"].shape[0])
        if family == "bernoulli":
            ref = BO.laplace_grad_ascent(P["cov_par"], "sqexp", P["U"], P["X"], P["y"], P["f0"],
                                         P["mu"], muu, opt=opt)
        else:
            ref = OD.laplace_grad_ascent(P["cov_par"], "sqexp", P["U"], P["X"], P["y"], P["f0"],
                                         P["mu"], muu, P["expo"], opt=opt)
        assert got["iter"] == ref["iter"] == 5 and "error" not in got
        print(family, "nr_iter", list(got["nr_iter"]), list(ref["nr_iter"]))
        assert list(got["nr_iter"]) == list(ref["nr_iter"])
        kw = dict(rtol=EVAL_RTOL)
        np.testing.assert_allclose(got["obj_fun"], ref["obj_fun"], atol=1e-9, **kw)
        np.testing.assert_allclose(got["cov_par_history"], ref["cov_par_history"], atol=1e-9, **kw)
        np.testing.assert_allclose(got["grad"], ref["grad"], atol=1e-7, **kw)
        np.testing.assert_allclose(got["fmax"], ref["fmax"], atol=1e-7, **kw)
        np.testing.assert_allclose(got["u_mean"], ref["u_mean"], atol=1e-7, **kw)
        np.testing.assert_allclose(got["u_var"], ref["u_var"], atol=1e-7, **kw)


def test_cross_validation_matches_a_loop_of_fits(sgp):
    """cross_validate_gp(family = "bernoulli", vi = False, folds = 3) against optimize_gp +
    score_gp fold by fold."""
    g = np.random.Generator(np.random.PCG64(8200))
    n = 240
    X = g.uniform(0.0, 10.0, size=(n, 2))
    y = (g.uniform(size=n) < 1.0 / (1.0 + np.exp(-1.6 * np.sin(X).sum(axis=1)))).astype(np.float64)
    U = g.uniform(0.0, 10.0, size=(8, 2))
    cp = OrderedDict([("sigma", 1.2), ("l", 1.7), ("tau", 0.5)])
    opt = {"maxit": 4, "obj_tol": 0.0, "tol_nr": 1e-6}
    mu = np.zeros(n)
    cv = sgp.cross_validate_gp(y, X, "sqexp", cp, U, folds=3, mu=mu, opt=opt, vi=False,
                               family="bernoulli")
    assert len(cv["folds"]) == 3
    nlps = []
    for f in cv["folds"]:
        te = f["test_rows"]
        tr = np.setdiff1d(np.arange(n), te)
        mod = sgp.optimize_gp(y[tr], X[tr], "sqexp", cp, mu[tr], family="bernoulli", sparse=True,
                              xu_opt="fixed", xu=U, opt=opt)
        ref = sgp.score_gp(mod, X[te], y[te], mu[te])
        assert f["model"]["family"] == "bernoulli"
        assert f["model"]["results"]["iter"] == mod["results"]["iter"]
        np.testing.assert_allclose(f["model"]["results"]["obj_fun"], mod["results"]["obj_fun"],
                                   rtol=EVAL_RTOL)
        np.testing.assert_allclose(f["score"]["nlp"], ref["nlp"], rtol=EVAL_RTOL, atol=1e-9)
        for key in ("mean_nlp", "median_nlp", "rmse", "srmse"):
            np.testing.assert_allclose(f["score"][key], ref[key], rtol=EVAL_RTOL)
        assert f["score"]["n_nan"] == ref["n_nan"]
        # the model is what score_gp takes
        again = sgp.score_gp(f["model"], X[te], y[te], mu[te])
        np.testing.assert_allclose(again["nlp"], ref["nlp"], rtol=EVAL_RTOL, atol=1e-9)
        nlps.append(ref["nlp"])
    np.testing.assert_allclose(cv["mean_nlp"], np.concatenate(nlps).mean(), rtol=EVAL_RTOL)
