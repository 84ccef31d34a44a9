"""GPU parity of the Bernoulli (classification) sparse-Laplace path with the CPU restatement
(tests/bern_oracle.py), at the Poisson file's bars: exact NR iteration count, NR objectives
rtol 1e-9, mode 1e-8 absolute, objective and gradient 1e-6 relative.

Bernoulli NR converges linearly, so a run takes 31 to 165 slow steps and
an exact iteration count needs the stop rule's deciding quantity max(|obj_k - obj_k-1|,
max |grad psi|) away from tol_nr = 1e-5.  In the restatement (PCG64 seeds in bern_oracle.CASES)
its relative distance from tol at the stopping test / at the one before is
  sqexp_300_20 4.0 % / 8.7 %,  ard_350_25 2.5 % / 7.9 %,  sqexp_257_1 16.7 % / 23.5 %,
  sqexp_900_130 8.0 % / 1.9 %,  vignette_200_5 1.6 % / 4.2 %
(tests/test_bernoulli_oracle.py::test_stop_rule_margins_of_the_gpu_cases holds them >= 0.1 %).
"""

import numpy as np
import pytest

import bern_oracle as B
from oracle import sgp_oracle as O

pytestmark = pytest.mark.gpu
EVAL_RTOL = 1e-6
TOL = B.TOL_NR


@pytest.fixture(scope="module")
def sgp():
    import sparsergps_amd as S
    from sparsergps_amd import _lib
    _lib.require_gpu()
    return S


_REF = {}


def _ref(name):
    """(problem, restatement NR result, restatement gradient at its mode), computed once."""
    if name not in _REF:
        P = B.problem(name)
        nr = B.newtrap_sparseGP(P["f0"], P["cov_par"], P["cov_fun"], P["X"], P["U"], P["y"],
                                P["mu"], P["delta"], tol=TOL,
                                muu=np.zeros(P["U"].shape[0]))
        g = B.dlogq_dcov_par(P["cov_par"], P["cov_fun"], P["U"], P["X"], P["y"], nr["gp"],
                             P["mu"], P["delta"])["gradient"]
        _REF[name] = (P, nr, g)
    return _REF[name]


def _theta(P):
    return np.array(list(P["cov_par"].values()))


@pytest.mark.parametrize("name", list(B.CASES))
def test_bernoulli_matches_restatement(sgp, name):
    """sqexp_900_130 (d = 2, 130 knots at l = 2: K22 + K12' Z^-1 K12 has condition ~1e7) is the
    case that needs the refined m x m solves: through the explicit inverses
    alone it gave NR objectives 2.8e-8, mode 9.8e-6 and gradient 2.4e-6.  Measured on the
    MI355X with the refinement: objectives 6.8e-10, mode 7.5e-9, objective 2.7e-10, gradient
    2.6e-8; the other four cases are at 1e-12 or better."""
    P, nr, g = _ref(name)
    r = sgp.laplace_eval(P["cov_par"], P["cov_fun"], P["U"], P["X"], P["y"], P["mu"], P["f0"],
                         1.0, P["delta"], tol=TOL, family="bernoulli")
    ov = nr["objective_function_values"]
    k = min(len(ov), len(r["objective_function_values"]))
    gerr = {q: abs(r["gradient"][q] - g[q]) / max(1.0, abs(g[q])) for q in g}
    print(name, "iters", r["nr_iter"], len(ov), "objectives",
          np.max(np.abs(r["objective_function_values"][:k] - ov[:k]) / np.abs(ov[:k])),
          "mode", np.max(np.abs(r["gp"] - nr["gp"])),
          "objective", abs(r["objective"] - ov[-1]) / abs(ov[-1]), "gradient", gerr)
    assert r["nr_iter"] == len(ov) < 1000
    np.testing.assert_allclose(r["objective_function_values"], ov, rtol=1e-9)
    assert np.max(np.abs(r["gp"] - nr["gp"])) < 1e-8
    assert abs(r["objective"] - ov[-1]) / abs(ov[-1]) < EVAL_RTOL
    for q in g:
        assert gerr[q] < EVAL_RTOL, (q, r["gradient"][q], g[q])


def test_objective_and_gradient_at_a_given_f(sgp):
    """maxit = 0: obj_fun_bern and dlogq_dcov_par at a supplied non-mode f with |f| up to 15,
    where log pi and log(1 - pi) need the stable log link (pi itself rounds to within 3e-7 of
    0 or 1 there)."""
    P, _, _ = _ref("sqexp_300_20")
    f = 15.0 * np.sin(0.7 * np.arange(P["y"].size) + 0.3)
    assert np.max(np.abs(f)) > 14.9
    s12, s22, Z = O.laplace_mats(P["cov_par"], "sqexp", P["U"], P["X"], P["delta"])
    ref = B.obj_fun_bern(f, P["mu"], Z, s12, s22, P["y"])
    g = B.dlogq_dcov_par(P["cov_par"], "sqexp", P["U"], P["X"], P["y"], f, P["mu"],
                         P["delta"])["gradient"]
    o = sgp.obj_fun_bern(f, P["cov_par"], "sqexp", P["U"], P["X"], P["y"], P["mu"], P["delta"])
    assert abs(o - ref) / abs(ref) < EVAL_RTOL
    r = sgp.dlogq_dcov_par(P["cov_par"], "sqexp", xu=P["U"], xy=P["X"], y=P["y"], ff=f,
                           mu=P["mu"], delta=P["delta"], family="bernoulli")
    for q in g:
        assert abs(r["gradient"][q] - g[q]) / max(1.0, abs(g[q])) < EVAL_RTOL, (q, r["gradient"][q], g[q])


@pytest.mark.parametrize("maxit", [2, 1000])
def test_newtrap_grad_psi_and_posterior_u(sgp, maxit):
    """newtrap_sparseGP's `gradient` (grad psi of the last NR step) after the first update and
    at convergence, and the u posterior, which uses the last step's W (newtrap_sparseGP.R:
    137-176) -- for this family a W that differs from W3 and from the true Hessian."""
    P, _, _ = _ref("sqexp_300_20")
    muu = np.zeros(P["U"].shape[0])
    nr = B.newtrap_sparseGP(P["f0"], P["cov_par"], "sqexp", P["X"], P["U"], P["y"], P["mu"],
                            P["delta"], maxit=maxit, tol=TOL, muu=muu)
    with sgp.SparseGPContext(P["X"], P["y"], P["mu"], m_max=P["U"].shape[0]) as ctx:
        got = sgp.newtrap_sparseGP(P["f0"], P["cov_par"], "sqexp", P["X"], P["U"], P["y"],
                                   P["mu"], 1.0, P["delta"], maxit=maxit, tol=TOL, ctx=ctx,
                                   family="bernoulli")
        um, uv = ctx.posterior_u(muu)
    assert len(got["objective_function_values"]) == len(nr["objective_function_values"])
    if maxit == 2:
        assert np.max(np.abs(nr["gradient"])) > 0.1
        np.testing.assert_allclose(got["gradient"], nr["gradient"], rtol=1e-9, atol=1e-12)
    else:
        assert np.max(np.abs(got["gradient"] - nr["gradient"])) < 1e-8
    np.testing.assert_allclose(um, nr["u_posterior_mean"], rtol=EVAL_RTOL, atol=1e-7)
    np.testing.assert_allclose(uv, nr["u_posterior_variance"], rtol=EVAL_RTOL, atol=1e-7)


def test_lap_candidates_match_restatement(sgp):
    """OAT scoring: for each of T = 3 candidates, NR at [xu; cand_t] warm-started from the
    fit's mode; the resident mode is restored."""
    P, nr, _ = _ref("sqexp_300_20")
    n, m = P["X"].shape[0], P["U"].shape[0]
    cand = P["X"][np.random.default_rng(5).choice(n, size=3, replace=False)]
    fmax = nr["gp"]
    with sgp.SparseGPContext(P["X"], P["y"], P["mu"], m_max=m + 1) as ctx:
        ctx.lap_set_family("bernoulli")
        ctx.lap_set_f(fmax)
        got = ctx.lap_candidates(_theta(P), "sqexp", P["U"], cand, P["delta"], 1.0, TOL, 1000)
        np.testing.assert_array_equal(ctx.lap_get_f(), fmax)
    for t in range(3):
        ref = B.newtrap_sparseGP(fmax, P["cov_par"], "sqexp", P["X"], np.vstack([P["U"], cand[t]]),
                                 P["y"], P["mu"], P["delta"], tol=TOL)
        o = ref["objective_function_values"][-1]
        assert abs(got[t] - o) / abs(o) < EVAL_RTOL, (t, got[t], o)


def test_grad_ascent_matches_restatement(sgp):
    """Three laplace_grad_ascent iterations (each: warm-started NR, then the gradient) against
    oracle/drivers.py's ascent loop driven by the restatement.  The restatement's NR runs take
    83, 43 and 43 steps, each at least 1.2 % of tol away from the stop rule's threshold."""
    P, _, _ = _ref("sqexp_300_20")
    opt = {"maxit": 3, "obj_tol": 0.0, "tol_nr": TOL}
    muu = np.zeros(P["U"].shape[0])
    ref = B.laplace_grad_ascent(P["cov_par"], "sqexp", P["U"], P["X"], P["y"], P["f0"], P["mu"],
                                muu, opt=opt)
    got = sgp.laplace_grad_ascent(P["cov_par"], "sqexp", True, None, None, P["U"], P["X"],
                                  P["y"], P["f0"], P["mu"], muu, 1.0, opt, family="bernoulli")
    assert got["iter"] == ref["iter"] == 3
    assert list(got["nr_iter"]) == list(ref["nr_iter"])
    kw = dict(rtol=EVAL_RTOL)
    np.testing.assert_allclose(got["obj_fun"], ref["obj_fun"], atol=1e-9, **kw)
    np.testing.assert_allclose(got["cov_par_history"], ref["cov_par_history"], atol=1e-9, **kw)
    np.testing.assert_allclose(got["grad"], ref["grad"], atol=1e-7, **kw)
    np.testing.assert_allclose(got["fmax"], ref["fmax"], atol=1e-7, **kw)
    np.testing.assert_allclose(got["u_mean"], ref["u_mean"], atol=1e-7, **kw)
    np.testing.assert_allclose(got["u_var"], ref["u_var"], atol=1e-7, **kw)


def test_three_shards_match_one_context(sgp):
    """A multi-device context forwards the family to every shard: 3 ragged shards on one GPU
    against the single context.  Sharding reorders the row sums, so the two runs agree as two
    roundings of one computation do: they are held to each other at the bars each is held to
    the restatement (NR count exact, objectives 1e-9, mode and grad psi 1e-8, gradient 1e-6)."""
    P, nr, _ = _ref("sqexp_300_20")
    th, m = _theta(P), P["U"].shape[0]
    res = {}
    for key, dv in (("one", None), ("multi", [0] * 3)):
        with sgp.SparseGPContext(P["X"], P["y"], P["mu"], m_max=m + 1, devices=dv) as c:
            c.lap_set_family("bernoulli")
            c.lap_set_f(P["f0"])
            o, g, it = c.eval_laplace(th, "sqexp", P["U"], P["delta"], 1.0, TOL, 1000)
            res[key] = dict(o=o, g=g, it=it, ov=c.lap_objective_values(), f=c.lap_get_f(),
                            gp=c.lap_get_grad_psi(), post=c.posterior_u(np.zeros(m)),
                            cand=c.lap_candidates(th, "sqexp", P["U"], P["X"][:2], P["delta"],
                                                  1.0, TOL, 1000))
    a, b = res["multi"], res["one"]
    assert a["it"] == b["it"] == len(nr["objective_function_values"])
    np.testing.assert_allclose(a["ov"], b["ov"], rtol=1e-9, atol=0)
    assert abs(a["o"] - b["o"]) / abs(b["o"]) < EVAL_RTOL
    for x, y in zip(a["g"], b["g"]):
        assert abs(x - y) / max(1.0, abs(y)) < EVAL_RTOL
    assert np.max(np.abs(a["f"] - b["f"])) < 1e-8
    assert np.max(np.abs(a["gp"] - b["gp"])) < 1e-8
    np.testing.assert_allclose(a["post"][0], b["post"][0], rtol=EVAL_RTOL, atol=1e-7)
    np.testing.assert_allclose(a["post"][1], b["post"][1], rtol=EVAL_RTOL, atol=1e-7)
    np.testing.assert_allclose(a["cand"], b["cand"], rtol=EVAL_RTOL)


def test_row_sharded_laplace_world_size_one(sgp):
    """RowShardedLaplace(family="bernoulli") on one rank (no collectives) is laplace_eval."""
    from sparsergps_amd.dist import HipRowBackend, RowShardedLaplace
    P, nr, g = _ref("vignette_200_5")
    be = HipRowBackend(P["X"], P["y"], P["mu"], P["U"].shape[0], 0, "sqexp", "laplace")
    try:
        be.ctx.lap_set_f(P["f0"])
        obj, grad, it = RowShardedLaplace(be).eval(_theta(P), P["U"], P["delta"], 1.0, TOL, 1000,
                                                   family="bernoulli")
    finally:
        be.close()
    ov = nr["objective_function_values"]
    assert it == len(ov)
    assert abs(obj - ov[-1]) / abs(ov[-1]) < EVAL_RTOL
    for q, v in zip(g, grad):
        assert abs(v - g[q]) / max(1.0, abs(g[q])) < EVAL_RTOL, q


@pytest.mark.parametrize("bad", [2.0, 0.5])
def test_non_binary_response_is_refused(sgp, bad):
    """A response other than 0 or 1: SGPError when the family is set, and when set_data brings
    such a y under the Bernoulli family; the context stays usable under Poisson."""
    from sparsergps_amd import _lib
    P, _, _ = _ref("sqexp_300_20")
    y = P["y"].copy()
    y[250] = bad          # a row of the third shard: the first two are sent back
    mu = np.full(y.size, np.log(y.mean()))
    th = _theta(P)
    for dv in (None, [0] * 3):
        with sgp.SparseGPContext(P["X"], y, mu, m_max=P["U"].shape[0], devices=dv) as c:
            c.lap_set_f(mu)
            before = c.eval_laplace(th, "sqexp", P["U"], P["delta"], 1.0, TOL, 1000)
            with pytest.raises(sgp.SGPError, match=r"y\[250\]") as e:
                c.lap_set_family("bernoulli")
            assert e.value.status == _lib.SGP_EINVAL
            c.lap_set_f(mu)                     # still Poisson, on every shard
            after = c.eval_laplace(th, "sqexp", P["U"], P["delta"], 1.0, TOL, 1000)
            assert before[0] == after[0] and before[2] == after[2]
            np.testing.assert_array_equal(before[1], after[1])
            c.set_data(P["y"], P["mu"])
            c.lap_set_family("bernoulli")       # binary y: accepted
            with pytest.raises(sgp.SGPError, match=r"y\[250\]"):
                c.set_data(y, mu)               # refused, nothing replaced
            c.lap_set_f(P["f0"])
            o = c.lap_nr(th, "sqexp", P["U"], P["delta"], 1.0, TOL, 1000)
            assert o[1] == len(_ref("sqexp_300_20")[1]["objective_function_values"])
            with pytest.raises(ValueError):
                c.lap_set_family("binomial")
            assert c._lib.sgp_lap_set_family(c.handle, 7) == _lib.SGP_EINVAL


def test_poisson_is_untouched_by_a_bernoulli_run(sgp):
    """Poisson -> Bernoulli -> Poisson on one context from the same start: the two Poisson
    results are bit-identical (y in {0, 1} is a valid Poisson response)."""
    P, nr, _ = _ref("sqexp_300_20")
    th = _theta(P)
    mu = np.full(P["y"].size, np.log(P["y"].mean()))
    with sgp.SparseGPContext(P["X"], P["y"], mu, m_max=P["U"].shape[0]) as c:
        def poisson():
            c.lap_set_family("poisson")
            c.lap_set_f(mu)
            o, g, it = c.eval_laplace(th, "sqexp", P["U"], P["delta"], 1.0, TOL, 1000)
            return o, g, it, c.lap_objective_values(), c.lap_get_f()
        p1 = poisson()
        c.lap_set_family("bernoulli")
        c.lap_set_f(P["f0"])
        ob, gb, itb = c.eval_laplace(th, "sqexp", P["U"], P["delta"], 1.0, TOL, 1000)
        p2 = poisson()
    assert itb != p1[2] and ob != p1[0]           # the middle run was another likelihood
    assert p1[0] == p2[0] and p1[2] == p2[2]
    for a, b in zip(p1[1:], p2[1:]):
        np.testing.assert_array_equal(a, b)


def test_mu_none_is_refused(sgp):
    P, _, _ = _ref("sqexp_300_20")
    with pytest.raises(ValueError, match="Poisson convention"):
        sgp.laplace_eval(P["cov_par"], "sqexp", P["U"], P["X"], P["y"], None, P["f0"],
                         family="bernoulli")
