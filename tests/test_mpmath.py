"""Third independent pin of the oracle: 50-digit mpmath.

``oracle/mp_ref.py`` restates the VI ELBO, the FITC log marginal likelihood and the Poisson
sparse-Laplace objective in dense n x n form at 50 significant digits and differentiates them
with mpmath's own ``diff`` in log(theta) (the Laplace objective with its mode re-found to 50
digits at every theta).  The Laplace gradient adds the reference's comp3 term analytically
(laplace_approx_gradient.R:308-310), so every parameter -- including the length
scales, where the reference formula is not the objective's derivative -- is pinned.

  * CPU: the fp64 oracle (oracle/sgp_oracle.py) against mpmath at 1e-12 relative;
  * GPU: one libsgp evaluation of the same problem against mpmath at 1e-10 relative.

Problems: n = 14 rows, m = 6 knots (one knot equal to a data row, quirk Q5), d = 2,
sqexp and ARD.

Prediction (predict_vi, predict_laplace in both families, predict_gp_full; diagonal and
full_cov) is pinned the same way on the two fixtures of tests/predict_cases.py (m = 24 knots,
8 rows, two of them equal to knots): every entry of the oracle's output within 1e-10 of that
entry's magnitude budget s of the 50-digit value.
"""
import math
from collections import OrderedDict

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

from oracle import mp_ref as M          # noqa: E402
from oracle import sgp_oracle as O      # noqa: E402
import predict_cases as PC              # noqa: E402

PRED_ORACLE_TOL = 1e-10                 # of the entry's magnitude budget s
CASES = [("sqexp", OrderedDict(sigma=1.2, l=1.9, tau=0.6)),
         ("ard", OrderedDict(sigma=1.1, l1=1.6, l2=2.4, tau=0.5))]
LAP_CASES = [("sqexp", OrderedDict(sigma=1.0, l=2.0, tau=0.3)),
             ("ard", OrderedDict(sigma=1.2, l1=1.5, l2=2.5, tau=0.4))]
_CACHE = {}


def _problem(seed=11, n=14, m=5, d=2):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 10, (n, d))
    U = np.vstack([rng.uniform(0, 10, (m, d)), X[3]])          # knot 6 == data row 4 (Q5)
    y = np.sin(X).sum(1) + rng.normal(0, 0.3, n)
    lam = np.exp(0.5 * np.sin(X).sum(1) / math.sqrt(d) + math.log(2))
    yp = rng.poisson(lam).astype(float)
    return X, U, y, np.full(n, y.mean()), yp, np.full(n, math.log(yp.mean()))


def _mp(kind, cf, cp):
    key = (kind, cf)
    if key not in _CACHE:
        X, U, y, mu, yp, mup = _problem()
        if kind == "laplace":
            _CACHE[key] = M.evaluate(kind, cp, cf, X, U, yp, mup)
        else:
            _CACHE[key] = M.evaluate(kind, cp, cf, X, U, y, mu)
    return _CACHE[key]


def _check(obj, grad, ref_obj, ref_grad, tol):
    ro = float(ref_obj)
    assert abs(obj - ro) / abs(ro) < tol, (obj, ro)
    for k, v in ref_grad.items():
        v = float(v)
        assert abs(grad[k] - v) / max(1.0, abs(v)) < tol, (k, grad[k], v)


def _oracle(kind, cf, cp, fhat=None):
    X, U, y, mu, yp, mup = _problem()
    if kind == "vi":
        return (O.elbo_eval(cp, cf, U, X, y, mu),
                O.delbo_dcov_par(cp, cf, U, X, y, mu)["gradient"])
    if kind == "fitc":
        return (O.fitc_obj_eval(cp, cf, U, X, y, mu),
                O.dlogp_dcov_par(cp, cf, U, X, y, mu)["gradient"])
    s12, s22, Z = O.laplace_mats(cp, cf, U, X, 1e-6)
    return (O.obj_fun_pois(fhat, mup, Z, s12, s22, yp, 1.0),
            O.dlogq_dcov_par(cp, cf, U, X, yp, fhat, mup, 1.0)["gradient"])


@pytest.mark.parametrize("cf,cp", CASES)
@pytest.mark.parametrize("kind", ["vi", "fitc"])
def test_oracle_gaussian_matches_mpmath(kind, cf, cp):
    ro, rg = _mp(kind, cf, cp)
    obj, grad = _oracle(kind, cf, cp)
    _check(obj, grad, ro, rg, 1e-12)


@pytest.mark.parametrize("cf,cp", LAP_CASES)
def test_oracle_laplace_matches_mpmath(cf, cp):
    ro, rg, f = _mp("laplace", cf, cp)
    fhat = np.array([float(v) for v in f])
    obj, grad = _oracle("laplace", cf, cp, fhat)
    _check(obj, grad, ro, rg, 1e-12)


def test_laplace_length_scale_quirk_is_nonzero():
    """The comp3 correction is what separates the reference's l gradient from the
    objective's derivative; for sigma it vanishes identically."""
    cf, cp = LAP_CASES[0]
    _, _, f = _mp("laplace", cf, cp)
    X, U, y, mu, yp, mup = _problem()
    with mp.workdps(M.DPS):
        Xm, Um = M._mat(X), M._mat(U)
        th = M._theta(cp)
        coinc = M._coinc(Xm, Um)
        args = (th, cf, Xm, Um, M._vec(yp), mp.mpf(1), mp.mpf(1e-6), f)
        c_l = M.laplace_comp3_correction(*args, "l", coinc)
        c_s = M.laplace_comp3_correction(*args, "sigma", coinc)
    assert abs(float(c_l)) > 1e-3
    assert abs(float(c_s)) < 1e-40


# ----------------------------------------------------------------------------- prediction
@pytest.mark.parametrize("full_cov", [False, True])
@pytest.mark.parametrize("method", PC.METHODS)
@pytest.mark.parametrize("name", list(PC.MP_FIXTURES))
def test_oracle_prediction_matches_mpmath(name, method, full_cov):
    """Every entry of the fp64 oracle's prediction within 1e-10 of its magnitude budget s
    (oracle/mp_ref.py) of the 50-digit value.  Measured maxima of |oracle - mpmath| / s over
    both fixtures and both covariance forms: VI mean 3.0e-15 / variance 7.2e-16,
    predict_laplace gaussian 3.0e-15 / 3.6e-16, other family 3.3e-16 / 3.4e-16,
    predict_gp_full 2.4e-16 / 2.5e-16."""
    ref = PC.mp_predict(name, method, full_cov)
    got = PC.call(O, method, PC.mp_fixture(name), full_cov)
    em = np.abs(np.asarray(got["pred_mean"]).reshape(-1) - ref["pred_mean"]) / ref["s_mean"]
    ev = np.abs(np.asarray(got["pred_var"]) - ref["pred_var"]) / ref["s_var"]
    print(f"{name} {method} full_cov={full_cov}: mean {em.max():.2e} var {ev.max():.2e}")
    assert got["pred_var"].shape == ref["pred_var"].shape
    assert em.max() <= PRED_ORACLE_TOL and ev.max() <= PRED_ORACLE_TOL


def test_prediction_budget_bounds_the_value():
    """s is a sum of absolute values of the terms of its entry: never below |value|, and an
    off-diagonal entry of a full_cov matrix has a budget of its own, below the diagonal's."""
    for method in PC.METHODS:
        r = PC.mp_predict("sqexp_d3", method, True)
        assert np.all(r["s_var"] >= np.abs(r["pred_var"]) * (1 - 1e-15))
        assert np.all(r["s_mean"] >= np.abs(r["pred_mean"]) * (1 - 1e-15))
        off = r["s_var"][~np.eye(8, dtype=bool)]
        assert off.min() < np.diag(r["s_var"]).min()


# ----------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def sgp():
    import sparsergps_amd as S
    from sparsergps_amd import _lib
    _lib.require_gpu()
    return S


@pytest.mark.gpu
@pytest.mark.parametrize("cf,cp", CASES)
@pytest.mark.parametrize("kind", ["vi", "fitc"])
def test_gpu_gaussian_matches_mpmath(sgp, kind, cf, cp):
    ro, rg = _mp(kind, cf, cp)
    X, U, y, mu, _, _ = _problem()
    fn = sgp.vi_eval if kind == "vi" else sgp.fitc_eval
    obj, grad = fn(cp, cf, U, X, y, mu, 1e-6)
    _check(obj, grad, ro, rg, 1e-10)


@pytest.mark.gpu
@pytest.mark.parametrize("cf,cp", LAP_CASES)
def test_gpu_laplace_matches_mpmath(sgp, cf, cp):
    ro, rg, f = _mp("laplace", cf, cp)
    fhat = np.array([float(v) for v in f])
    X, U, _, _, yp, mup = _problem()
    grad = sgp.dlogq_dcov_par(cp, cf, xu=U, xy=X, y=yp, ff=fhat, mu=mup, m=1.0)["gradient"]
    obj = sgp.obj_fun_pois(fhat, cp, cf, U, X, yp, mup, m=1.0)
    _check(obj, grad, ro, rg, 1e-10)
