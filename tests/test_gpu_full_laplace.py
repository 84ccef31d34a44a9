"""GPU parity for the full-GP Laplace path (family = "poisson" / "bernoulli", sparse = FALSE):
sgp_eval_full_laplace (newtrapGP + dlogq_dcov_par_full), sgp_full_laplace_state,
SGP_PRED_LAPLACE_FULL and laplace_grad_ascent_full against tests/full_laplace_oracle.py.

Shapes straddle the Gauss-Jordan chain's 64-wide pivot block and the 128 tile (n = 1, 64, 65,
127, 128, 129, 257), carry a duplicated row (n = 200), take the contraction's chunked coordinate
path (d = 13) and the vignette-like n = 392.  Bars are the project's C5 bars: NR count exact,
every NR objective at rtol 1e-9, the mode at 1e-8 absolute, the gradient at 1e-7 relative to
max(1, |g|); grad psi, W and grad_log_py_ff at 1e-8.  tests/test_full_laplace_oracle.py asserts
that no problem here has its stop-rule quantity within 1 % of tol, so the count is well defined.
"""
from collections import OrderedDict

import numpy as np
import pytest

import full_laplace_oracle as F

pytestmark = pytest.mark.gpu
CASES = [(name, fam) for fam in F.FAMILIES for name in F.SHAPES]


@pytest.fixture(scope="module")
def sgp():
    import sparsergps_amd as S
    from sparsergps_amd import _lib
    _lib.require_gpu()
    return S


def _ctx(sgp, P, m_max=None):
    ctx = sgp.SparseGPContext(P["X"], P["y"], P["mu"], m_max=m_max or P["y"].size)
    ctx.lap_set_family(P["family"])
    ctx.lap_set_f(P["f0"])
    return ctx


def _theta(P):
    return np.array(list(P["cov_par"].values()))


def _check_parity(ctx, P, nr, obj, g, it):
    ov = nr["objective_function_values"]
    got_ov = ctx.lap_objective_values()
    print("NR count", it, len(ov), "max obj rel err",
          np.max(np.abs(got_ov[:len(ov)] - ov[:len(got_ov)]) / np.abs(ov[:len(got_ov)])))
    assert it == len(ov) == len(got_ov)
    np.testing.assert_allclose(got_ov, ov, rtol=1e-9)
    assert obj == got_ov[-1]
    f = ctx.lap_get_f()
    print("mode err", np.max(np.abs(f - nr["gp"])))
    np.testing.assert_allclose(f, nr["gp"], rtol=0, atol=1e-8)
    rg = nr["theta_gradient"]
    gerr = np.abs(g - rg) / np.maximum(1.0, np.abs(rg))
    print("grad", g, rg, gerr)
    assert np.all(gerr <= 1e-7), (g, rg)
    W, d1 = ctx.full_laplace_state()
    gpsi = ctx.lap_get_grad_psi()
    print("state err", np.max(np.abs(W - nr["W"])), np.max(np.abs(d1 - nr["grad_log_py_ff"])),
          np.max(np.abs(gpsi - nr["gradient"])))
    np.testing.assert_allclose(W, nr["W"], rtol=0, atol=1e-8)
    np.testing.assert_allclose(d1, nr["grad_log_py_ff"], rtol=0, atol=1e-8)
    np.testing.assert_allclose(gpsi, nr["gradient"], rtol=0, atol=1e-8)


@pytest.mark.parametrize("name,family", CASES)
def test_eval_matches_restatement(sgp, name, family):
    P, nr = F.reference(name, family)
    with _ctx(sgp, P) as ctx:
        obj, g, it = ctx.eval_full_laplace(_theta(P), P["cov_fun"], P["delta"], P["a"], P["tol"])
        _check_parity(ctx, P, nr, obj, g, it)


def test_row_exposure_is_the_scalar_exposure_bit_for_bit(sgp):
    P = F.problem("sqexp_129", "poisson")
    out = []
    for expo in (1.7, np.full(129, 1.7)):
        with _ctx(sgp, P) as ctx:
            obj, g, it = ctx.eval_full_laplace(_theta(P), P["cov_fun"], P["delta"], expo, P["tol"])
            out.append((obj, g, it, ctx.lap_get_f(), ctx.lap_objective_values()))
    assert out[0][0] == out[1][0] and out[0][2] == out[1][2]
    for k in (1, 3, 4):
        np.testing.assert_array_equal(out[0][k], out[1][k])


def test_warm_start_maxit0_obj_only_and_repeatability(sgp):
    P, nr = F.reference("ard_129", "poisson")
    th = _theta(P)
    with _ctx(sgp, P) as ctx:
        first = ctx.eval_full_laplace(th, P["cov_fun"], P["delta"], P["a"], P["tol"])
        mode = ctx.lap_get_f()
        # a second evaluation at the same theta starts at the mode: one update, two values
        obj2, g2, it2 = ctx.eval_full_laplace(th, P["cov_fun"], P["delta"], P["a"], P["tol"])
        assert it2 == 2 and ctx.lap_objective_values().size == 2
        assert abs(obj2 - first[0]) <= 1e-9 * abs(first[0])
        f2 = ctx.lap_get_f()
        # maxit = 0: objective and gradient at the resident f as given, no step
        obj0, g0, it0 = ctx.eval_full_laplace(th, P["cov_fun"], P["delta"], P["a"], P["tol"], 0)
        assert it0 == 1 and obj0 == obj2
        np.testing.assert_array_equal(g0, g2)
        np.testing.assert_array_equal(ctx.lap_get_f(), f2)
        with pytest.raises(sgp.SGPError):
            ctx.full_laplace_state()                 # no NR step has run in that evaluation
        # SGP_FLAG_OBJ_ONLY: newtrapGP alone, the same objective, no gradient
        ctx.lap_set_f(f2)
        objo, go, ito = ctx.eval_full_laplace(th, P["cov_fun"], P["delta"], P["a"], P["tol"], 0,
                                              obj_only=True)
        assert go is None and objo == obj0
        # repeatability: the same start gives the same bits
        ctx.lap_set_f(P["f0"])
        again = ctx.eval_full_laplace(th, P["cov_fun"], P["delta"], P["a"], P["tol"])
        assert again[0] == first[0] and again[2] == first[2]
        np.testing.assert_array_equal(again[1], first[1])
        np.testing.assert_array_equal(ctx.lap_get_f(), mode)


def test_python_mirror_matches_restatement(sgp):
    """newtrapGP, obj_fun_*_full and dlogq_dcov_par_full by their reference names."""
    for name, family in (("sqexp_127", "poisson"), ("sqexp_127", "bernoulli")):
        P, nr = F.reference(name, family)
        kw = {"m": P["a"]} if family == "poisson" else {}
        got = sgp.newtrapGP(P["f0"], P["cov_par"], P["cov_fun"], P["X"], P["y"], P["mu"],
                            delta=P["delta"], tol=P["tol"], family=family, **kw)
        np.testing.assert_allclose(got["objective_function_values"],
                                   nr["objective_function_values"], rtol=1e-9)
        np.testing.assert_allclose(got["gp"], nr["gp"], rtol=0, atol=1e-8)
        np.testing.assert_allclose(got["W"], nr["W"], rtol=0, atol=1e-8)
        fam = F.family_fns(family, P["a"])
        S = F.O.full_sigma(P["cov_par"], P["cov_fun"], P["X"], P["delta"])
        ro = F.obj_fun_full(P["f0"], P["mu"], S, P["y"], fam)
        if family == "poisson":
            o = sgp.obj_fun_pois_full(P["f0"], P["cov_par"], P["cov_fun"], P["X"], P["y"], P["mu"],
                                      P["a"], P["delta"])
        else:
            o = sgp.obj_fun_bern_full(P["f0"], P["cov_par"], P["cov_fun"], P["X"], P["y"], P["mu"],
                                      P["delta"])
        assert abs(o - ro) <= 1e-9 * abs(ro)
        g = sgp.dlogq_dcov_par_full(P["cov_par"], P["cov_fun"], True, P["X"], P["y"], nr["gp"],
                                    P["mu"], delta=P["delta"], family=family, **kw)["gradient"]
        for k, r in zip(P["cov_par"], nr["theta_gradient"]):
            assert abs(g[k] - r) <= 1e-7 * max(1.0, abs(r)), (k, g[k], r)


@pytest.mark.parametrize("full_cov", [False, True])
@pytest.mark.parametrize("name,family,npred", [("sqexp_129", "poisson", 57),
                                               ("sqexp_200_dup", "bernoulli", 130)])
def test_predict_laplace_full_matches_restatement(sgp, name, family, npred, full_cov):
    """State from a 3-value NR (maxit = 3), so W and grad_log_py_ff are visibly those of the
    previous iterate, not of the returned mode."""
    P = F.problem(name, family)
    nr = F.newtrapGP(P["f0"], P["cov_par"], P["cov_fun"], P["X"], P["y"], P["mu"], family, P["a"],
                     P["delta"], maxit=3, tol=P["tol"])
    assert len(nr["objective_function_values"]) == 3
    W_at_mode = F.family_fns(family, P["a"])[1](nr["gp"], P["y"])
    assert np.max(np.abs(W_at_mode - nr["W"])) > 1e-4      # the quirk is visible
    with _ctx(sgp, P) as ctx:
        obj, _, it = ctx.eval_full_laplace(_theta(P), P["cov_fun"], P["delta"], P["a"], P["tol"], 3,
                                           obj_only=True)
        assert it == 3
        W, d1 = ctx.full_laplace_state()
        fmax = ctx.lap_get_f()
    np.testing.assert_allclose(W, nr["W"], rtol=0, atol=1e-8)
    np.testing.assert_allclose(d1, nr["grad_log_py_ff"], rtol=0, atol=1e-8)
    xp = np.random.default_rng(8).uniform(0, 10, (npred, P["X"].shape[1]))
    mup = np.full(npred, 0.25)
    ref = F.predict_laplace_full(P["X"], xp, nr["W"], P["cov_par"], P["cov_fun"],
                                 nr["grad_log_py_ff"], mup, full_cov, P["delta"])
    got = sgp.predict_laplace_full(fmax, P["X"], xp, W, P["cov_par"], P["cov_fun"], d1, P["mu"],
                                   mup, full_cov, P["delta"])
    np.testing.assert_allclose(got["pred_mean"], ref["pred_mean"], rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose(got["pred_var"], ref["pred_var"], rtol=1e-8, atol=1e-9)
    mod = {"family": family, "sparse": False, "delta": P["delta"],
           "results": {"xy": P["X"], "y": P["y"], "mu": P["mu"], "cov_fun": P["cov_fun"],
                       "cov_par": P["cov_par"], "fmax": fmax, "W": W, "grad_log_py_ff": d1}}
    pg = sgp.predict_gp(mod, xp, mup, full_cov)
    np.testing.assert_allclose(pg["pred"]["pred_mean"], ref["pred_mean"], rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose(pg["pred"]["pred_var"], ref["pred_var"], rtol=1e-8, atol=1e-9)
    assert pg["sparse"] is False and pg["family"] == family


def test_fixture_predictions(sgp):
    """The committed fixture's W and grad_log_py_ff through SGP_PRED_LAPLACE_FULL."""
    import os
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", F.FIXTURE))
    cp = OrderedDict(zip(("sigma", "l", "tau"), fx["theta"]))
    got = sgp.predict_laplace_full(fx["mode"], fx["X"], fx["x_pred"], fx["W"], cp, "sqexp",
                                   fx["grad_log_py_ff"], fx["mu"], np.zeros(fx["x_pred"].shape[0]),
                                   False, float(fx["delta"]))
    np.testing.assert_allclose(got["pred_mean"].reshape(-1), fx["pred_mean"], rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose(got["pred_var"], fx["pred_var"], rtol=1e-8, atol=1e-9)


@pytest.mark.parametrize("family", F.FAMILIES)
def test_laplace_grad_ascent_full_matches_restatement(sgp, family):
    P = F.problem("sqexp_127", family)
    opt = {"maxit": 4, "obj_tol": 0.0, "tol_nr": P["tol"]}
    ref = F.laplace_grad_ascent_full(P["cov_par"], P["cov_fun"], P["X"], P["y"], P["f0"], P["mu"],
                                     family, P["a"], opt)
    got = sgp.laplace_grad_ascent_full(P["cov_par"], P["cov_fun"], True, P["X"], P["y"], P["f0"],
                                       P["mu"], P["a"], opt, family=family)
    assert got["iter"] == ref["iter"] == 4
    np.testing.assert_array_equal(got["nr_iter"], ref["nr_iter"])
    np.testing.assert_allclose(got["obj_fun"], ref["obj_fun"], rtol=1e-6)
    np.testing.assert_allclose(got["cov_par_history"], ref["cov_par_history"], rtol=1e-6)
    np.testing.assert_allclose(got["grad"], ref["grad"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(got["fmax"], ref["fmax"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(got["W"], ref["W"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(got["grad_log_py_ff"], ref["grad_log_py_ff"], rtol=0, atol=1e-6)


def test_refusals_leave_the_context_usable(sgp):
    """m_max < n, a multi-device context, SGP_KERNEL_EXP and a Bernoulli family with a
    non-0/1 y are refused with SGP_EINVAL; after each, a Gaussian sgp_eval_full and a sparse
    sgp_eval_laplace on the same context still return what they returned before."""
    from sparsergps_amd import _lib
    P = F.problem("sqexp_129", "poisson")      # Poisson counts: some y > 1
    assert np.any(P["y"] > 1)
    th = _theta(P)
    U = P["X"][:20].copy()

    def baseline(ctx):
        ctx.lap_set_f(P["f0"])
        lap = ctx.eval_laplace(th, "sqexp", U, P["delta"], P["a"], 1e-6)
        full = ctx.eval_full(th, "sqexp", P["delta"])
        return lap, full

    def same(a, b):
        assert a[0][0] == b[0][0] and a[0][2] == b[0][2] and a[1][0] == b[1][0]
        np.testing.assert_array_equal(a[0][1], b[0][1])
        np.testing.assert_array_equal(a[1][1], b[1][1])

    with _ctx(sgp, P) as ctx:
        base = baseline(ctx)
        with pytest.raises(sgp.SGPError) as e:
            ctx.eval_full_laplace(th, "exp", P["delta"], P["a"], P["tol"])
        assert e.value.status == _lib.SGP_EINVAL
        same(baseline(ctx), base)
        with pytest.raises(sgp.SGPError) as e:
            ctx.lap_set_family("bernoulli")
        assert e.value.status == _lib.SGP_EINVAL and "is not 0 or 1" in str(e.value)
        same(baseline(ctx), base)
        # and the full-Laplace evaluation itself leaves the other paths as they were
        ctx.lap_set_f(P["f0"])
        ctx.eval_full_laplace(th, "sqexp", P["delta"], P["a"], P["tol"])
        same(baseline(ctx), base)
    with _ctx(sgp, P, m_max=64) as small:
        small.lap_set_f(P["f0"])
        lap0 = small.eval_laplace(th, "sqexp", U, P["delta"], P["a"], 1e-6)
        with pytest.raises(sgp.SGPError) as e:
            small.eval_full_laplace(th, "sqexp", P["delta"], P["a"], P["tol"])
        assert e.value.status == _lib.SGP_EINVAL and "m_max >= n" in str(e.value)
        small.lap_set_f(P["f0"])
        lap1 = small.eval_laplace(th, "sqexp", U, P["delta"], P["a"], 1e-6)
        assert lap0[0] == lap1[0] and lap0[2] == lap1[2]
        np.testing.assert_array_equal(lap0[1], lap1[1])
    multi = sgp.SparseGPContext(P["X"], P["y"], P["mu"], m_max=129, devices=[0, 0])
    with multi:
        multi.lap_set_f(P["f0"])
        lap0 = multi.eval_laplace(th, "sqexp", U, P["delta"], 1.3, 1e-6)
        with pytest.raises(sgp.SGPError) as e:
            multi.eval_full_laplace(th, "sqexp", P["delta"], 1.3, P["tol"])
        assert e.value.status == _lib.SGP_EINVAL and "multi-device" in str(e.value)
        multi.lap_set_f(P["f0"])
        lap1 = multi.eval_laplace(th, "sqexp", U, P["delta"], 1.3, 1e-6)
        assert lap0[0] == lap1[0] and lap0[2] == lap1[2]
        np.testing.assert_array_equal(lap0[1], lap1[1])


def test_random_exposure_matches_restatement(sgp):
    """The per-row exposure path against the restatement (every Poisson case above already runs
    with a random exposure vector; this one checks a scalar exposure too)."""
    P = F.problem("sqexp_64", "poisson")
    nr = F.newtrapGP(P["f0"], P["cov_par"], P["cov_fun"], P["X"], P["y"], P["mu"], "poisson", 1.3,
                     P["delta"], tol=P["tol"])
    r = F.stop_ratios(nr["stop_trace"], P["tol"])
    assert not np.any((r >= 0.99) & (r <= 1.01))
    with _ctx(sgp, P) as ctx:
        obj, g, it = ctx.eval_full_laplace(_theta(P), P["cov_fun"], P["delta"], 1.3, P["tol"])
        np.testing.assert_allclose(ctx.lap_objective_values(), nr["objective_function_values"],
                                   rtol=1e-9)
        np.testing.assert_allclose(ctx.lap_get_f(), nr["gp"], rtol=0, atol=1e-8)
