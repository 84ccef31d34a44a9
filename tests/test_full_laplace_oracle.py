"""The full-GP Laplace path without a GPU: the numpy restatement (tests/full_laplace_oracle.py)
against its fixture, the adjoint form of the gradient against the reference's per-parameter
loop, the Poisson gradient against finite differences, the stop-rule condition of every problem
the GPU tests use, and the C ABI's new declarations, exports and argument checks."""
import ctypes as C
import os
import re
from collections import OrderedDict

import numpy as np
import pytest

import full_laplace_oracle as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(name, fam) for fam in F.FAMILIES for name in F.SHAPES]


def test_restatement_reproduces_fixture():
    fx = np.load(os.path.join(ROOT, "tests", "golden", F.FIXTURE))
    rec = F.fixture_record()
    assert sorted(fx.files) == sorted(rec)
    for k in ("X", "y", "mu", "f0", "a", "theta", "x_pred"):
        np.testing.assert_array_equal(fx[k], rec[k], err_msg=k)
    assert fx["objective_function_values"].size == rec["objective_function_values"].size
    for k in ("objective_function_values", "mode", "gradient", "W", "grad_log_py_ff", "grad_psi",
              "pred_mean", "pred_var"):
        np.testing.assert_allclose(rec[k], fx[k], rtol=1e-10, atol=1e-11, err_msg=k)
    assert fx["X"].shape[0] <= 300


@pytest.mark.parametrize("name,family", [("sqexp_129", "poisson"), ("ard_129", "bernoulli"),
                                         ("sqexp_200_dup", "poisson"), ("ard_140_d13", "bernoulli"),
                                         ("sqexp_392", "poisson"), ("sqexp_1", "bernoulli")])
def test_adjoint_form_equals_parameter_loop(name, family):
    """G = 1/2 a a^T - 1/2 R + 1/2 (v d1^T + d1 v^T) contracted with dSigma_p equals
    laplace_approx_gradient.R:650-708's loop."""
    P, nr = F.reference(name, family)
    adj = F.dlogq_dcov_par_full_adjoint(P["cov_par"], P["cov_fun"], P["X"], P["y"], nr["gp"],
                                        P["mu"], family, P["a"], P["delta"])
    ga = np.array([adj[k] for k in P["cov_par"]])
    err = np.max(np.abs(ga - nr["theta_gradient"]) / np.maximum(1.0, np.abs(nr["theta_gradient"])))
    assert err <= 1e-12, err


def _fd_gradient(P, h=1e-5, tol=1e-13):
    """Central differences in log theta of the objective re-converged at each theta +- h."""
    names = list(P["cov_par"])
    out = []
    for k in names:
        vals = []
        for sgn in (1.0, -1.0):
            cp = OrderedDict(P["cov_par"])
            cp[k] = float(np.exp(np.log(cp[k]) + sgn * h))
            nr = F.newtrapGP(P["f0"], cp, P["cov_fun"], P["X"], P["y"], P["mu"], "poisson", P["a"],
                             P["delta"], tol=tol, maxit=200)
            vals.append(nr["objective_function_values"][-1])
        out.append((vals[0] - vals[1]) / (2 * h))
    return np.array(out)


def _analytic_gradient(P, tol=1e-13):
    nr = F.newtrapGP(P["f0"], P["cov_par"], P["cov_fun"], P["X"], P["y"], P["mu"], "poisson",
                     P["a"], P["delta"], tol=tol, maxit=200)
    g = F.dlogq_dcov_par_full(P["cov_par"], P["cov_fun"], P["X"], P["y"], nr["gp"], P["mu"],
                              "poisson", P["a"], P["delta"])["gradient"]
    return np.array([g[k] for k in P["cov_par"]])


def test_poisson_gradient_matches_finite_differences():
    """No duplicate rows (n = 109 <= 110): every parameter, tau included, at the 1e-6 bar."""
    P = F.make_problem(109, 2, "sqexp", "poisson")
    assert np.unique(P["X"], axis=0).shape[0] == 109
    g, fd = _analytic_gradient(P), _fd_gradient(P)
    err = np.abs(g - fd) / np.maximum(1.0, np.abs(fd))
    print("poisson FD", g, fd, err)
    assert np.all(err <= 1e-6), err


def test_poisson_gradient_with_a_duplicated_row():
    """Rows 7 and 100 coincide: sigma and l still agree with finite differences; tau differs
    by the coincidence term (quirk Q5: dSigma/dlog tau = 2 tau^2 on every coincident pair, the
    off-diagonal pair included, while Sigma itself carries tau^2 on the diagonal only)."""
    P = F.problem("sqexp_129", "poisson")
    assert np.array_equal(P["X"][7], P["X"][100])
    g, fd = _analytic_gradient(P), _fd_gradient(P)
    err = np.abs(g - fd) / np.maximum(1.0, np.abs(fd))
    print("poisson FD dup", g, fd, err)
    assert np.all(err[:2] <= 1e-6), err
    nr = F.newtrapGP(P["f0"], P["cov_par"], P["cov_fun"], P["X"], P["y"], P["mu"], "poisson",
                     P["a"], P["delta"], tol=1e-13, maxit=200)
    G = F.dlogq_dcov_par_full_adjoint(P["cov_par"], P["cov_fun"], P["X"], P["y"], nr["gp"],
                                      P["mu"], "poisson", P["a"], P["delta"], return_G=True)
    coinc = 2 * P["cov_par"]["tau"] ** 2 * (G[7, 100] + G[100, 7])
    assert abs(coinc) > 1e-4                       # the term is there ...
    assert abs((g[2] - fd[2]) - coinc) <= 1e-6     # ... and it is the whole difference


@pytest.mark.parametrize("name,family", CASES)
def test_stop_rule_condition(name, family):
    """Every problem the GPU tests use: at every NR loop test the deciding quantity
    max(|obj_k - obj_{k-1}|, max |grad psi|) / tol lies outside [0.99, 1.01], so rounding cannot
    change the iteration count, and cond(Sigma) <= 4e4 (the project's rule)."""
    P, nr = F.reference(name, family)
    r = F.stop_ratios(nr["stop_trace"], P["tol"])
    assert not np.any((r >= 0.99) & (r <= 1.01)), r
    assert nr["cond_sigma"] <= 4e4
    assert len(nr["objective_function_values"]) < 1000


# ------------------------------------------------------------------ ABI, no device
@pytest.fixture(scope="module")
def lib():
    from sparsergps_amd import _lib
    return _lib.lib()


def test_header_declares_the_full_laplace_api():
    text = open(os.path.join(ROOT, "include", "sgp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+sgp_eval_full_laplace\s*\(", code)
    assert re.search(r"\bint\s+sgp_full_laplace_state\s*\(", code)
    assert re.search(r"SGP_PRED_LAPLACE_FULL\s*=\s*3\b", code)
    assert re.search(r"#define\s+SGP_ABI_VERSION\s+1\b", code)


def test_library_exports_the_full_laplace_api(lib):
    from sparsergps_amd import _lib
    for name in ("sgp_eval_full_laplace", "sgp_full_laplace_state"):
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES
    assert _lib.SGP_PRED_LAPLACE_FULL == 3
    assert lib.sgp_abi_version() == 1


def test_argument_checks_need_no_device(lib):
    from sparsergps_amd import _lib
    th = np.array([1.0, 1.5, 0.4])
    obj = C.c_double(0.0)
    g = np.zeros(3)
    it = C.c_int(0)
    st = lib.sgp_eval_full_laplace(None, 0, _lib.dptr(th), 1e-6, 1.0, 1e-6, 10, 0, C.byref(obj),
                                   _lib.dptr(g), C.byref(it))
    assert st == _lib.SGP_EINVAL and b"context is NULL" in lib.sgp_last_error()
    assert lib.sgp_full_laplace_state(None, _lib.dptr(g), _lib.dptr(g)) == _lib.SGP_EINVAL
    X = np.asfortranarray(np.random.default_rng(0).uniform(size=(4, 2)))
    W = -np.ones(4)
    xp = np.asfortranarray(np.random.default_rng(1).uniform(size=(3, 2)))
    mp, pm, pv = np.zeros(3), np.zeros(3), np.zeros(3)

    def predict(u_mean, w):
        return lib.sgp_predict(0, 0, _lib.dptr(th), 1e-6, _lib.SGP_PRED_LAPLACE_FULL, 0,
                               _lib.dptr(X), 4, 4, u_mean, _lib.dptr(w), None, 4, _lib.dptr(xp),
                               3, 3, 2, _lib.dptr(mp), 0, _lib.dptr(pm), _lib.dptr(pv), 3)

    assert predict(None, W) == _lib.SGP_EINVAL
    assert b"invalid sgp_predict arguments" in lib.sgp_last_error()
    # W must be <= 0 (sqrt(-W)): refused on the host, naming the entry
    Wbad = W.copy()
    Wbad[2] = 0.5
    assert predict(_lib.dptr(np.zeros(4)), Wbad) == _lib.SGP_EINVAL
    assert b"SGP_PRED_LAPLACE_FULL: W[2]" in lib.sgp_last_error()


def test_python_exports():
    import sparsergps_amd as S
    for name in ("newtrapGP", "obj_fun_pois_full", "obj_fun_bern_full", "dlogq_dcov_par_full",
                 "full_laplace_eval", "laplace_grad_ascent_full", "predict_laplace_full"):
        assert name in S.__all__ and callable(getattr(S, name)), name
