"""The Bernoulli sparse-Laplace restatement (tests/bern_oracle.py) against closed forms, finite
differences and its committed fixture; and the C ABI's family switch.  No GPU."""
import math
import os
import re
from collections import OrderedDict

import numpy as np
import pytest

import bern_oracle as B
from oracle import sgp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", B.FIXTURE)


def fd_grad(fun, cp, h=1e-5):
    g = OrderedDict()
    for k in cp:
        a, b = OrderedDict(cp), OrderedDict(cp)
        a[k] = cp[k] * math.exp(h)
        b[k] = cp[k] * math.exp(-h)
        g[k] = (fun(a) - fun(b)) / (2 * h)
    return g


def test_restatement_reproduces_fixture():
    """Inputs come from the generator, results from the restatement: both must still give what
    the fixture recorded (1e-10: a different BLAS may round the m x m solves differently; the
    recorded run is well inside its stop-rule margins, so the iteration count is exact)."""
    G = np.load(GOLDEN)
    assert G["X"].shape[0] <= 512
    r = B.fixture_record()
    for k in ("X", "U", "y", "mu", "f0", "theta"):
        np.testing.assert_array_equal(r[k], G[k])
    assert set(np.unique(G["y"])) == {0.0, 1.0}
    assert len(r["objective_function_values"]) == len(G["objective_function_values"])
    np.testing.assert_allclose(r["objective_function_values"], G["objective_function_values"],
                               rtol=1e-10)
    assert np.max(np.abs(r["mode"] - G["mode"])) < 1e-9
    np.testing.assert_allclose(r["gradient"], G["gradient"], rtol=1e-8)


@pytest.mark.parametrize("y", [0.0, 1.0])
def test_d1_and_d3_are_finite_differences(y):
    """d1 = d/df of the log p row term (exact for both y); d3 = d/df of the reference's d2 (for
    y = 1 that d2 is -pi - pi^2, and d3 is ITS derivative: Q19).  Central differences with
    h = 1e-5 on O(1) smooth functions: truncation ~ h^2 = 1e-10, rounding ~ eps / h = 2e-11."""
    f = np.linspace(-6.0, 6.0, 241)
    h = 1e-5
    yy = np.full_like(f, y)
    d1_fd = (B.log_py_rows(f + h, yy) - B.log_py_rows(f - h, yy)) / (2 * h)
    assert np.max(np.abs(B.dlog_py_dff_bern(f, yy) - d1_fd)) < 1e-9
    d3_fd = (B.d2log_py_dff_bern(f + h, yy) - B.d2log_py_dff_bern(f - h, yy)) / (2 * h)
    assert np.max(np.abs(B.d3log_py_dff_bern(f, yy) - d3_fd)) < 1e-9


def test_w_is_exact_for_y0_and_the_quirk_for_y1():
    """Q19: the reference's W is the true -pi (1 - pi) at y = 0 and -pi - pi^2 at y = 1."""
    f = np.linspace(-5.0, 5.0, 101)
    pi = B.my_logistic(f)
    np.testing.assert_allclose(B.d2log_py_dff_bern(f, np.zeros_like(f)), -pi * (1 - pi), atol=1e-15)
    np.testing.assert_allclose(B.d2log_py_dff_bern(f, np.ones_like(f)), -pi - pi ** 2, atol=1e-15)
    assert np.all(B.d2log_py_dff_bern(f, np.ones_like(f)) < 0)


def test_log_link_is_overflow_safe():
    """plogis(., log.p = TRUE) through R's piecewise log1pexp: finite and accurate far out."""
    f = np.array([-800.0, -40.0, -20.0, 0.0, 17.9, 18.1, 33.2, 33.4, 800.0])
    lp = B.plogis_log(f)
    assert np.all(np.isfinite(lp))
    np.testing.assert_allclose(lp[:3], f[:3], rtol=1e-8)          # log pi -> f
    assert lp[3] == -math.log(2.0)
    np.testing.assert_allclose(lp[4:], -np.exp(-f[4:]), rtol=1e-7)  # log pi -> -e^-f


def test_bernoulli_objective_dense():
    """log q = log p(y|f) - 1/2 (f-mu)^T Sig^-1 (f-mu) - 1/2 log|I + Sig (-W)|  (R&W 3.32)."""
    from sparsergps_amd.workloads import make_bernoulli_problem
    P = make_bernoulli_problem(90, 9, cov_par=OrderedDict(sigma=1.0, l=2.0, tau=0.1))
    K12, K22, Z = O.laplace_mats(P["cov_par"], "sqexp", P["U"], P["X"], P["delta"])
    Sig = K12 @ np.linalg.solve(K22, K12.T) + np.diag(Z)
    f = 0.3 + 0.8 * np.sin(np.arange(90))
    mu = np.full(90, 0.1)
    W = B.d2log_py_dff_bern(f, P["y"])
    d = f - mu
    _, ld = np.linalg.slogdet(np.eye(90) + Sig @ np.diag(-W))
    dense = np.sum(B.log_py_rows(f, P["y"])) - 0.5 * d @ np.linalg.solve(Sig, d) - 0.5 * ld
    got = B.obj_fun_bern(f, mu, Z, K12, K22, P["y"])
    assert abs(got - dense) / abs(dense) < 1e-10


def _fd_case(all_zero):
    from sparsergps_amd.workloads import make_bernoulli_problem
    P = make_bernoulli_problem(200, 12, cov_par=OrderedDict(sigma=1.0, l=2.0, tau=0.1))
    y = np.zeros(200) if all_zero else P["y"]
    cp = P["cov_par"]

    def nr(c):
        return B.newtrap_sparseGP(P["f0"], c, "sqexp", P["X"], P["U"], y, P["mu"], tol=1e-11,
                                  maxit=5000)

    g = B.dlogq_dcov_par(cp, "sqexp", P["U"], P["X"], y, nr(cp)["gp"], P["mu"])["gradient"]
    gf = fd_grad(lambda c: nr(c)["objective_function_values"][-1], cp)
    return g, gf


def test_gradient_fd_sigma_tau_when_y_is_zero():
    """With y = 0 everywhere W and W3 are exact, and the gradient is the finite difference of
    the re-converged objective for sigma and tau (not for l: the length-scale discrepancy of
    test_oracle.py::test_laplace_gradient_fd_sigma_tau).  Bound 1e-6, as there: NR stops at
    |d obj| <= 1e-11, which a central difference with h = 1e-5 can turn into 1e-11 / 2h = 5e-7.
    Measured: sigma 5e-9, tau 3e-7, l 8e-3."""
    g, gf = _fd_case(True)
    assert abs(g["sigma"] - gf["sigma"]) / max(1.0, abs(g["sigma"])) < 1e-6
    assert abs(g["tau"] - gf["tau"]) / max(1.0, abs(g["tau"])) < 1e-6
    assert abs(g["l"] - gf["l"]) / abs(gf["l"]) > 1e-3


def test_gradient_is_not_fd_when_y_is_mixed():
    """Q19 on record: with y = 1 rows the reference's W is not the Hessian of log p, so the
    Laplace gradient built on it is not the derivative of the converged objective.  Measured
    relative mismatch: sigma 0.14, l 0.04, tau 0.016."""
    g, gf = _fd_case(False)
    for k in ("sigma", "tau"):
        assert abs(g[k] - gf[k]) / max(1.0, abs(g[k])) > 1e-3, k


def test_stop_rule_margins_of_the_gpu_cases():
    """Every tests/test_gpu_bernoulli.py parity input keeps the stop rule's deciding quantity at
    least 1e-3 tol away from tol at the stopping test and at the one before, and stays under
    1000 iterations -- so a GPU that agrees to 1e-9 takes the same number of steps."""
    for name in B.CASES:
        P = B.problem(name)
        nr = B.newtrap_sparseGP(P["f0"], P["cov_par"], P["cov_fun"], P["X"], P["U"], P["y"],
                                P["mu"], P["delta"], tol=B.TOL_NR, trace=True)
        assert len(nr["objective_function_values"]) < 1000
        assert min(B.stop_margins(nr["stop_trace"], B.TOL_NR)) >= 1e-3, name


def test_family_switch_is_declared_and_exported():
    """include/sgp.h declares sgp_lap_set_family and the family constants; the built library
    exports it and the ctypes table binds it (additive: the ABI version stays 1)."""
    from sparsergps_amd import _lib
    text = open(os.path.join(ROOT, "include", "sgp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+sgp_lap_set_family\s*\(\s*sgp_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", code)
    assert re.search(r"SGP_FAM_POISSON\s*=\s*0\s*,\s*SGP_FAM_BERNOULLI\s*=\s*1", code)
    assert "sgp_lap_set_family" in _lib.PROTOTYPES
    assert _lib.FAMILIES == {"poisson": 0, "bernoulli": 1}
    h = _lib.lib()
    assert hasattr(h, "sgp_lap_set_family")
    assert h.sgp_abi_version() == 1
    # no context: refused with a message, before any device work
    assert h.sgp_lap_set_family(None, 1) == _lib.SGP_EINVAL
    assert b"NULL" in h.sgp_last_error()


def test_python_surface():
    import inspect

    import sparsergps_amd as S
    from sparsergps_amd import dist, laplace
    assert "obj_fun_bern" in S.__all__ and callable(S.obj_fun_bern)
    for fn in (S.laplace_eval, S.newtrap_sparseGP, S.dlogq_dcov_par, S.laplace_grad_ascent,
               dist.RowShardedLaplace.eval):
        assert inspect.signature(fn).parameters["family"].default == "poisson", fn
    assert hasattr(S.SparseGPContext, "lap_set_family")
    y = np.array([0.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="Poisson convention"):
        laplace._mu_vec(None, y, "bernoulli")
    assert laplace._mu_vec(None, y)[0] == math.log(2.0 / 3.0)
    with pytest.raises(ValueError):
        laplace._context(None, y, 0.0, 1, "binomial", None)


def test_make_bernoulli_problem():
    from sparsergps_amd.workloads import make_bernoulli_problem
    P = make_bernoulli_problem(200, 5)
    assert P["X"].shape == (200, 2) and P["U"].shape == (5, 2)
    assert P["X"].min() > 0 and P["X"].max() < 10 and P["U"].min() > 0 and P["U"].max() < 10
    assert set(np.unique(P["y"])) == {0.0, 1.0}
    assert not P["mu"].any() and not P["f0"].any()
    assert list(P["cov_par"].items()) == [("sigma", 5.0), ("l", 2.0), ("tau", 0.1)]
    f = 2.0 * np.sin(P["X"]).sum(axis=1) / math.sqrt(2.0)
    assert np.corrcoef(P["y"], 1 / (1 + np.exp(-f)))[0, 1] > 0.4   # y follows logistic(f)
    Q = make_bernoulli_problem(50, 4, d=3, cov_par=OrderedDict(sigma=1.0, l=2.0, tau=0.1))
    assert Q["X"].shape == (50, 3) and Q["cov_par"]["sigma"] == 1.0
