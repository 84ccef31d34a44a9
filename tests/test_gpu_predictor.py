"""The resident predictor (sgp_predictor_*, sparsergps_amd.Predictor) on the GPU: parity with the
CPU oracle and with mpmath, agreement of its routes, bit-identity over chunking, repeats and the
device-pointer entry, scoring, and errors.

Tolerance: the project's prediction tolerance RTOL = 1e-8 in tests/test_gpu_predict.py's _rel
norm; inputs follow its _pred_inputs (make_gaussian_problem, vi_posterior_u, the first two
prediction rows equal to knots) with a per-row mu_pred.  Shapes and the edge each one reaches:
  m = 20,  np = 150        the register route (route 0 up to 64 knots): three 64-row steps, the
                           last partial; forced onto the tile route: nb = 1
  m = 130, np = 200        nb = 2, knots 130..255 padded, the second row tile partial
  m = 300, np = 129 with chunk_rows = 128    nb = 3, two chunks, the second holding one row
  m = 64 and 65            either side of the crossover between the two routes
  d = 3 sqexp (C2), d = 8 ARD (C3), d = 12 ARD (coordinates beyond one chunk of 8)
"""
from collections import OrderedDict

import numpy as np
import pytest

import full_laplace_oracle as FL
import predict_cases as PC
from oracle import sgp_oracle as O

pytestmark = pytest.mark.gpu
RTOL = 1e-8
MP_RTOL = 1e-8     # tests/test_gpu_predict_edges.py's bar against mpmath, of the entry's budget


@pytest.fixture(scope="module")
def sgp():
    import sparsergps_amd as S
    from sparsergps_amd import _lib
    _lib.require_gpu()
    return S


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


_INPUTS = {}


def _pred_inputs(cfg, m, npred, d=None, n=400, seed=21):
    """tests/test_gpu_predict.py's _pred_inputs with a per-row mu_pred; computed once."""
    key = (cfg, m, npred, d)
    if key not in _INPUTS:
        P = O.make_gaussian_problem(cfg, n=n, m=m, d=d) if d else O.make_gaussian_problem(cfg, n=n, m=m)
        muu = np.full(m, P["y"].mean())
        um, uv = O.vi_posterior_u(P["cov_par"], P["cov_fun"], P["U"], P["X"], P["y"], P["mu"], muu,
                                  P["delta"])
        dd = P["X"].shape[1]
        xp = np.random.default_rng(seed).uniform(0, 10, size=(npred, dd))
        xp[:2] = P["U"][:2]                           # prediction at knots (exact coincidence)
        mup = P["y"].mean() + 0.1 * np.cos(np.arange(npred))
        _INPUTS[key] = (P, muu, um, uv, xp, mup)
    return _INPUTS[key]


_POIS = {}


def _poisson_inputs(m, npred):
    if (m, npred) not in _POIS:
        P = O.make_poisson_problem(n=300, m=m)
        muu = np.full(m, P["mu"][0])
        nr = O.newtrap_sparseGP(P["f0"], P["cov_par"], "sqexp", P["X"], P["U"], P["y"], P["mu"],
                                P["a"], P["delta"], tol=1e-5, muu=muu)
        xp = np.random.default_rng(5).uniform(0, 10, size=(npred, 5))
        xp[:2] = P["U"][:2]
        mup = P["mu"][0] + 0.1 * np.cos(np.arange(npred))
        _POIS[(m, npred)] = (P, muu, nr["u_posterior_mean"], nr["u_posterior_variance"], xp, mup)
    return _POIS[(m, npred)]


def _assert_close(got, ref, what):
    em = _rel(np.asarray(got["pred_mean"]).ravel(), np.asarray(ref["pred_mean"]).ravel())
    ev = _rel(got["pred_var"], ref["pred_var"])
    print(f"{what}: mean {em:.3e} var {ev:.3e}")
    assert got["pred_mean"].shape == (np.asarray(ref["pred_var"]).size, 1)
    assert em < RTOL and ev < RTOL, (what, em, ev)


# (cfg, m, np, d, chunk_rows, routes that apply)
SHAPES = OrderedDict([
    ("c2_m20", ("C2", 20, 150, None, 0, (0, 1, 2, 3))),
    ("c2_m64", ("C2", 64, 150, None, 0, (0, 1, 2, 3))),     # the last register-route m
    ("c2_m65", ("C2", 65, 150, None, 0, (0, 1, 2, 3))),     # the first tile-route m
    ("c2_m130", ("C2", 130, 200, None, 0, (0, 1, 2))),
    ("c3_m300_two_chunks", ("C3", 300, 129, None, 128, (0, 1, 2))),
    ("c3_m130", ("C3", 130, 200, None, 0, (0, 1, 2))),
    ("c3_m20", ("C3", 20, 150, None, 0, (0, 1, 2, 3))),
    ("d12_m40", ("C3", 40, 150, 12, 0, (0, 1, 2, 3))),
    ("d12_m130", ("C3", 130, 150, 12, 128, (0, 1, 2))),
])


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("method", ["vi", "laplace"])
def test_routes_match_the_oracle_and_each_other(sgp, name, method):
    cfg, m, npred, d, chunk, routes = SHAPES[name]
    P, muu, um, uv, xp, mup = _pred_inputs(cfg, m, npred, d)
    ofun = O.predict_vi if method == "vi" else O.predict_laplace
    args = (um, uv, P["U"], xp, P["cov_fun"], P["cov_par"], mup, muu, False)
    ref = ofun(*args, P["delta"]) if method == "vi" else ofun(*args, "gaussian", P["delta"])
    outs = {}
    with sgp.Predictor(method, um, uv, P["U"], P["cov_fun"], P["cov_par"], muu, "gaussian",
                       P["delta"]) as p:
        for route in routes:
            outs[route] = p.predict(xp, mup, chunk_rows=chunk, route=route)
            _assert_close(outs[route], ref, f"{name} {method} route {route}")
        if 3 not in routes:
            with pytest.raises(sgp.SGPError, match="register route") as ei:
                p.predict(xp, mup, route=3)
            assert ei.value.status == 1
    for a in routes:
        for b in routes:
            if a < b:
                assert _rel(outs[a]["pred_mean"], outs[b]["pred_mean"]) < RTOL
                assert _rel(outs[a]["pred_var"], outs[b]["pred_var"]) < RTOL
    # route 0 is one of the others, bit for bit: the register route up to 64 knots
    prod = 3 if m <= 64 else 1
    assert np.array_equal(outs[0]["pred_var"], outs[prod]["pred_var"])
    assert np.array_equal(outs[0]["pred_mean"], outs[prod]["pred_mean"])


def _full_laplace_inputs(n=130, npred=200):
    P = FL.make_problem(n, 2, "sqexp", "poisson")
    nr = FL.newtrapGP(P["f0"], P["cov_par"], P["cov_fun"], P["X"], P["y"], P["mu"], "poisson",
                      P["a"], P["delta"], tol=P["tol"])
    xp = np.random.default_rng(9).uniform(0, 10, size=(npred, 2))
    xp[:2] = P["X"][:2]
    mup = 0.3 + 0.1 * np.cos(np.arange(npred))
    return P, nr, xp, mup


@pytest.mark.parametrize("combo", ["vi", "laplace_gaussian", "laplace_poisson", "full",
                                   "laplace_full"])
def test_every_method_at_130_knots(sgp, combo):
    """All five method / family combinations at m = 130 (nb = 2); the two full methods take
    U = xy with 130 rows.  Predictor.predict against the oracle and against the package's own
    per-call functions."""
    npred = 200
    if combo in ("vi", "laplace_gaussian"):
        P, muu, um, uv, xp, mup = _pred_inputs("C2", 130, npred)
        if combo == "vi":
            ref = O.predict_vi(um, uv, P["U"], xp, "sqexp", P["cov_par"], mup, muu, False, P["delta"])
            own = sgp.predict_vi(um, uv, P["U"], xp, "sqexp", P["cov_par"], mup, muu, False,
                                 delta=P["delta"])
            p = sgp.Predictor("vi", um, uv, P["U"], "sqexp", P["cov_par"], muu, "gaussian", P["delta"])
        else:
            ref = O.predict_laplace(um, uv, P["U"], xp, "sqexp", P["cov_par"], mup, muu, False,
                                    "gaussian", P["delta"])
            own = sgp.predict_laplace(um, uv, P["U"], xp, "sqexp", P["cov_par"], mup, muu, False,
                                      "gaussian", P["delta"])
            p = sgp.Predictor("laplace", um, uv, P["U"], "sqexp", P["cov_par"], muu, "gaussian",
                              P["delta"])
    elif combo == "laplace_poisson":
        P, muu, um, uv, xp, mup = _poisson_inputs(130, npred)
        ref = O.predict_laplace(um, uv, P["U"], xp, "sqexp", P["cov_par"], mup, muu, False,
                                "poisson", P["delta"])
        own = sgp.predict_laplace(um, uv, P["U"], xp, "sqexp", P["cov_par"], mup, muu, False,
                                  "poisson", P["delta"])
        p = sgp.Predictor("laplace", um, uv, P["U"], "sqexp", P["cov_par"], muu, "poisson",
                          P["delta"])
    elif combo == "full":
        P, _, _, _, xp, mup = _pred_inputs("C2", 130, npred)
        xy, y = P["U"], np.sin(P["U"]).sum(axis=1)
        mu = np.full(130, y.mean())
        ref = O.predict_gp_full(xy, y, xp, "sqexp", P["cov_par"], mu, mup, False, P["delta"])
        own = sgp.predict_gp_full(xy, y, xp, "sqexp", P["cov_par"], mu, mup, False, P["delta"])
        p = sgp.Predictor("full", y, None, xy, "sqexp", P["cov_par"], mu, "gaussian", P["delta"])
    else:
        P, nr, xp, mup = _full_laplace_inputs(130, npred)
        ref = FL.predict_laplace_full(P["X"], xp, nr["W"], P["cov_par"], P["cov_fun"],
                                      nr["grad_log_py_ff"], mup, False, P["delta"])
        own = sgp.predict_laplace_full(None, P["X"], xp, nr["W"], P["cov_par"], P["cov_fun"],
                                       nr["grad_log_py_ff"], None, mup, False, P["delta"])
        p = sgp.Predictor("laplace_full", nr["grad_log_py_ff"], None, P["X"], P["cov_fun"],
                          P["cov_par"], nr["W"], "poisson", P["delta"])
    with p:
        got = p.predict(xp, mup)
        alt = p.predict(xp, mup, route=2)
    _assert_close(got, ref, f"{combo} vs oracle")
    _assert_close(alt, ref, f"{combo} route 2 vs oracle")
    _assert_close(got, own, f"{combo} vs the per-call function")


_MP_CALL = {"vi": ("vi", "gauss", "gaussian"), "lap_gauss": ("laplace", "gauss", "gaussian"),
            "lap_nongauss": ("laplace", "nongauss", "poisson")}


@pytest.mark.parametrize("name", list(PC.MP_FIXTURES))
def test_matches_mpmath(sgp, name):
    """The two tests/predict_cases.py fixtures against 50-digit mpmath, every entry within
    1e-8 s (s mpmath's magnitude budget of the entry), on the product's route and the tile
    route."""
    F = PC.mp_fixture(name)
    for method in PC.METHODS:
        ref = PC.mp_predict(name, method, False)
        if method == "gp_full":
            p = sgp.Predictor("full", F["full"]["y"], None, F["U"], F["cov_fun"], F["cov_par"],
                              F["full"]["mu"], "gaussian", F["delta"])
        else:
            meth, key, fam = _MP_CALL[method]
            Q = F[key]
            p = sgp.Predictor(meth, Q["u_mean"], Q["u_var"], F["U"], F["cov_fun"], F["cov_par"],
                              Q["muu"], fam, F["delta"])
        with p:
            for route in (0, 1):
                got = p.predict(F["xp"], F["mu_pred"], route=route)
                em = np.abs(got["pred_mean"].ravel() - ref["pred_mean"]) / ref["s_mean"]
                ev = np.abs(got["pred_var"] - ref["pred_var"]) / ref["s_var"]
                print(f"mpmath {name} {method} route {route}: mean {em.max():.3e} var {ev.max():.3e}")
                assert em.max() <= MP_RTOL and ev.max() <= MP_RTOL, (method, route)


@pytest.mark.parametrize("cfg,m", [("C2", 130), ("C3", 300)])
def test_bit_identity(sgp, cfg, m):
    """A row's result has one summation order: a repeat, every chunking, the device-pointer
    entry with the host's column range as its box and the scoring entry give the same bits."""
    import torch
    npred = 300
    P, muu, um, uv, xp, mup = _pred_inputs(cfg, m, npred)
    with sgp.Predictor("laplace", um, uv, P["U"], P["cov_fun"], P["cov_par"], muu, "gaussian",
                       P["delta"]) as p:
        base = p.predict(xp, mup)
        again = p.predict(xp, mup)
        assert np.array_equal(base["pred_mean"], again["pred_mean"])
        assert np.array_equal(base["pred_var"], again["pred_var"])
        for chunk in (128, 256, 0):
            for route in (1, 2):
                ref = base if route == 1 else p.predict(xp, mup, route=2)
                got = p.predict(xp, mup, chunk_rows=chunk, route=route)
                assert np.array_equal(got["pred_mean"], ref["pred_mean"]), (chunk, route)
                assert np.array_equal(got["pred_var"], ref["pred_var"]), (chunk, route)
        # a batch that starts elsewhere: row i's bits do not depend on its place in a tile
        box = (xp.min(axis=0), xp.max(axis=0))
        tail = p.predict_torch(torch.as_tensor(xp[37:], device="cuda"),
                               torch.as_tensor(mup[37:], device="cuda"), box=box)
        assert np.array_equal(tail["pred_var"].cpu().numpy(), base["pred_var"][37:])
        assert np.array_equal(tail["pred_mean"].cpu().numpy(), base["pred_mean"][37:])
        dev = p.predict_torch(torch.as_tensor(xp, device="cuda"),
                              torch.as_tensor(mup, device="cuda"), box=box)
        torch.cuda.synchronize()
        assert np.array_equal(dev["pred_mean"].cpu().numpy(), base["pred_mean"])
        assert np.array_equal(dev["pred_var"].cpu().numpy(), base["pred_var"])
        # no box: the exact-difference builder, equal to rounding only
        nobox = p.predict_torch(torch.as_tensor(xp, device="cuda"), float(mup[0]))
        assert _rel(nobox["pred_var"].cpu().numpy(), base["pred_var"]) < RTOL
        # scoring: the same mean / variance bits, and sgp_nlp's nlp / stats on those vectors
        from sparsergps_amd.evaluation import _nlp
        rng = np.random.default_rng(3)
        expo = rng.uniform(0.5, 2.0, size=npred)
        cases = [("gaussian", base["pred_mean"].ravel() + rng.normal(0, 0.5, npred), 0.5, None),
                 ("poisson", rng.poisson(2.0, npred).astype(float), 1.0, expo),
                 ("bernoulli", (rng.uniform(size=npred) < 0.5).astype(float), 0.0, None)]
        for family, y, par, ex in cases:
            sc = p.score(xp, y, mup, family, par=par, expo=ex)
            assert np.array_equal(sc["pred_mean"], base["pred_mean"]), family
            assert np.array_equal(sc["pred_var"], base["pred_var"]), family
            nlp, stats = _nlp(family, y, sc["pred_mean"], sc["pred_var"], par, ex)
            assert np.array_equal(sc["nlp"], nlp, equal_nan=True), family
            assert np.array_equal(sc["stats"], stats), family
            assert stats[1] + stats[2] == npred and np.isfinite(stats[0])
            if family != "bernoulli":
                mine = sgp.my_nlp(y, sc["pred_mean"], sc["pred_var"], family,
                                  {"tau": par} if family == "gaussian" else {"m": ex})
                assert np.array_equal(sc["nlp"], mine["nlp"], equal_nan=True)


def test_register_route_bit_identity(sgp):
    """m = 20 (route 0 = the register route): repeat, chunking and the device entry."""
    import torch
    P, muu, um, uv, xp, mup = _pred_inputs("C3", 20, 150)
    with sgp.Predictor("vi", um, uv, P["U"], P["cov_fun"], P["cov_par"], muu, "gaussian",
                       P["delta"]) as p:
        base = p.predict(xp, mup)
        for chunk in (128, 256, 0):
            got = p.predict(xp, mup, chunk_rows=chunk, route=3)
            assert np.array_equal(got["pred_mean"], base["pred_mean"]), chunk
            assert np.array_equal(got["pred_var"], base["pred_var"]), chunk
        dev = p.predict_torch(torch.as_tensor(xp, device="cuda"),
                              torch.as_tensor(mup, device="cuda"))
        assert np.array_equal(dev["pred_var"].cpu().numpy(), base["pred_var"])
        assert np.array_equal(dev["pred_mean"].cpu().numpy(), base["pred_mean"])


def test_not_positive_definite_then_recovers(sgp):
    """tests/test_gpu_predict_edges.py's duplicated-knot construction: Sigma22 = Kuu + delta I with
    delta = -1e-3 is indefinite from the leading minor of order 151 on, so create raises
    NotPositiveDefinite naming that order; a valid predictor made afterwards matches the oracle."""
    g = np.random.Generator(np.random.PCG64(77))
    m, d = 200, 3
    U = g.uniform(0.0, 10.0, size=(m, d))
    U[150] = U[3]
    cp = OrderedDict([("sigma", 1.0), ("l", 0.3), ("tau", 0.5)])
    with pytest.raises(sgp.NotPositiveDefinite, match="Sigma22 is not positive definite.*order 151"):
        sgp.Predictor("vi", np.zeros(m), np.eye(m), U, "sqexp", cp, np.zeros(m), "gaussian", -1e-3)
    P, muu, um, uv, xp, mup = _pred_inputs("C2", 130, 200)
    ref = O.predict_vi(um, uv, P["U"], xp, "sqexp", P["cov_par"], mup, muu, False, P["delta"])
    with sgp.Predictor("vi", um, uv, P["U"], "sqexp", P["cov_par"], muu, "gaussian",
                       P["delta"]) as p:
        _assert_close(p.predict(xp, mup), ref, "after NotPositiveDefinite")


def test_closed_predictor_and_bad_batches(sgp):
    P, muu, um, uv, xp, mup = _pred_inputs("C2", 20, 150)
    p = sgp.Predictor("vi", um, uv, P["U"], "sqexp", P["cov_par"], muu, "gaussian", P["delta"])
    with pytest.raises(ValueError, match="columns"):
        p.predict(xp[:, :2], mup)
    with pytest.raises(sgp.SGPError, match="chunk_rows"):
        p.predict(xp, mup, chunk_rows=100)
    with pytest.raises(sgp.SGPError, match="route"):
        p.predict(xp, mup, route=4)
    with pytest.raises(sgp.SGPError, match="bernoulli y"):
        p.score(xp, np.full(150, 0.5), mup, "bernoulli")
    p.close()
    p.close()
    with pytest.raises(sgp.SGPError, match="closed"):
        p.predict(xp, mup)


def test_predictor_gp_dispatch(sgp):
    """predictor_gp reproduces predict_gp's dispatch: sparse VI / Laplace, the full Gaussian GP,
    a full Poisson fit, and the error string for VI with a non-Gaussian family."""
    P, muu, um, uv, xp, mup = _pred_inputs("C2", 20, 150)
    mod = {"family": "gaussian", "sparse": True, "delta": P["delta"],
           "results": {"u_mean": um, "u_var": uv, "xu": P["U"], "cov_fun": "sqexp",
                       "cov_par": P["cov_par"], "muu": muu}}
    for vi in (True, False):
        want = sgp.predict_gp(mod, xp, mup, full_cov=False, vi=vi)["pred"]
        with sgp.predictor_gp(mod, vi=vi) as p:
            assert p.method == ("vi" if vi else "laplace")
            _assert_close(p.predict(xp, mup), want, f"predictor_gp vi={vi}")
    assert sgp.predictor_gp(dict(mod, family="poisson"), vi=True) == \
        sgp.predict_gp(dict(mod, family="poisson"), xp, mup, vi=True)
    y = np.sin(P["U"]).sum(axis=1)
    full = {"family": "gaussian", "sparse": False, "delta": P["delta"],
            "results": {"xy": P["U"], "y": y, "mu": y.mean(), "cov_fun": "sqexp",
                        "cov_par": P["cov_par"]}}
    want = sgp.predict_gp(full, xp, mup)["pred"]
    with sgp.predictor_gp(full) as p:
        assert p.method == "full"
        _assert_close(p.predict(xp, mup), want, "predictor_gp full gaussian")
    Q, nr, xq, muq = _full_laplace_inputs(60, 70)
    flap = {"family": "poisson", "sparse": False, "delta": Q["delta"],
            "results": {"xy": Q["X"], "fmax": nr["gp"], "W": nr["W"], "mu": Q["mu"],
                        "grad_log_py_ff": nr["grad_log_py_ff"], "cov_fun": Q["cov_fun"],
                        "cov_par": Q["cov_par"]}}
    want = sgp.predict_gp(flap, xq, muq)["pred"]
    with sgp.predictor_gp(flap) as p:
        assert p.method == "laplace_full"
        _assert_close(p.predict(xq, muq), want, "predictor_gp full poisson")
