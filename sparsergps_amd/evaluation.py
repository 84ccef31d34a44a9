"""Held-out scoring: the reference's evaluation functions (R/evaluation_functions.R:5-176).

  my_rmse    l.5-8       host numpy
  my_nlp     l.12-145    mc = FALSE, mv = FALSE on the MI355X (sgp_nlp: one launch over the test
                         rows instead of one integrate() call per row)
  my_kl      l.151-176   the mv = FALSE formula, host numpy, element-wise
  score_gp   predict_gp followed by my_nlp / my_rmse / sd, as exec/boston.R:185-201,
             exec/airfoil.R:181-191 and exec/ccpp.R:168-178 score a fit (sgp_predict_nlp: the
             prediction is scored where it was computed)
  predict_prob  the averaged class probability int sigma(f) N(f; pred_mean, pred_var) df
  joint_nlp  my_nlp(mv = TRUE), l.21-26, 66-80, 120-133     on the MI355X with the library's own
  joint_kl   my_kl(mv = TRUE), l.153-164, as written        counter-based normal stream (a seed and
  mc_nlp     my_nlp(family = "bernoulli", mc = TRUE), l.53-65   a draw count).
             my_nlp / my_kl themselves keep refusing mv / mc: R's signatures have no place for
             either argument

The integrals are taken to fp64 accuracy; R's integrate() misses narrow integrands (it returns 0,
so nlp = Inf) and underflows in linear space.  Neither is reproduced.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib

_MV = ("my_nlp(mv = TRUE) is not ported: the multivariate branches "
       "(R/evaluation_functions.R:21-26 dmvnorm, 66-80 and 120-133 rmvnorm Monte Carlo) "
       "are out of scope")
_MC_BERN = ("my_nlp(family = 'bernoulli', mc = TRUE) draws from R's random stream "
            "(R/evaluation_functions.R:53-65: rnorm) and is not ported")
_MC_POIS = "Error: Monte Carlo estimate of marginal NLP for Poisson data must be fixed."


def my_rmse(pred, actual):
    """R/evaluation_functions.R:5-8."""
    pred = np.asarray(pred, dtype=np.float64)
    actual = np.asarray(actual, dtype=np.float64)
    return float(np.sqrt(np.mean((pred - actual) ** 2)))


def _score_par(family, par):
    """(scalar par, per-row exposure or None) of sgp_nlp from the reference's par list."""
    par = par or {}
    if family == "gaussian":
        if "tau" not in par:
            raise ValueError("family = 'gaussian' needs par = {'tau': ...}")
        return float(par["tau"]), None
    if family == "poisson":
        m = np.asarray(par.get("m", 1.0), dtype=np.float64)
        if m.ndim == 0 or m.size == 1:
            return float(m.reshape(-1)[0]), None
        return 1.0, np.ascontiguousarray(m.reshape(-1))
    return 0.0, None


def _nlp(family, y, pred_mean, pred_var, par, expo):
    if family not in _lib.SCORE_FAMILIES:
        raise ValueError(f"family must be one of {sorted(_lib.SCORE_FAMILIES)}, not {family!r}")
    from .vi import _device
    lib = _lib.lib()
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
    n = y.size
    pm = np.ascontiguousarray(np.broadcast_to(
        np.asarray(pred_mean, dtype=np.float64).reshape(-1), (n,)))
    pv = np.ascontiguousarray(np.broadcast_to(
        np.asarray(pred_var, dtype=np.float64).reshape(-1), (n,)))
    if expo is not None and expo.size != n:
        raise ValueError(f"par['m'] has {expo.size} values for {n} rows")
    nlp, stats = np.zeros(n), np.zeros(4)
    # the argument checks come first and need no device; the scoring itself does
    st = lib.sgp_nlp(_device(), _lib.SCORE_FAMILIES[family], _lib.dptr(y), _lib.dptr(pm),
                     _lib.dptr(pv), n, par, None if expo is None else _lib.dptr(expo),
                     _lib.dptr(nlp), _lib.dptr(stats))
    if st == _lib.SGP_EHIP:
        _lib.require_gpu()
    _lib.check(st)
    return nlp, stats


def my_nlp(y, pred_mean, pred_var, family="gaussian", par=None, mc=False, mv=False):
    """R/evaluation_functions.R:12-145 with mc = FALSE, mv = FALSE: {"nlp": vector}.
    par = {"tau": ...} (gaussian) or {"m": ...} (poisson: a scalar as in the reference, or one
    exposure per row).  Rows whose pred_mean or variance is unusable come back NaN."""
    if mv:
        raise NotImplementedError(_MV)
    if mc:
        if family == "poisson":
            return _MC_POIS   # l.114: the reference returns this string
        raise NotImplementedError(_MC_BERN if family == "bernoulli" else
                                  "my_nlp(mc = TRUE) has no gaussian branch "
                                  "(R/evaluation_functions.R:14-27)")
    p, expo = _score_par(family, par)
    return {"nlp": _nlp(family, y, pred_mean, pred_var, p, expo)[0]}


def my_kl(mean1, mean2, sigma1, sigma2, mv=False):
    """R/evaluation_functions.R:165-173 (mv = FALSE): KL(N(mean1, diag sigma1) || N(mean2, diag
    sigma2)), element-wise (the reference builds the n x n diag(1 / sigma2))."""
    if mv:
        raise NotImplementedError("my_kl(mv = TRUE) is not ported "
                                  "(R/evaluation_functions.R:153-164: chol / solve of full "
                                  "covariance matrices)")
    mean1, mean2, sigma1, sigma2 = (np.asarray(v, dtype=np.float64).reshape(-1)
                                    for v in (mean1, mean2, sigma1, sigma2))
    dm = mean2 - mean1
    return float(0.5 * (np.sum(sigma1 / sigma2) + np.sum(dm * dm / sigma2) - mean1.size
                        + np.sum(np.log(sigma2)) - np.sum(np.log(sigma1))))


def _sym_cov(name, a, n):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape != (n, n):
        raise ValueError(f"{name} must be {n} x {n}, not {a.shape}")
    return np.asfortranarray(a)


def _call(st):
    if st == _lib.SGP_EHIP:
        _lib.require_gpu()
    _lib.check(st)


def _seed(seed):
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must be an integer in [0, 2^64), not {seed}")
    return seed


def joint_nlp(y, pred_mean, pred_cov, family="gaussian", par=None, n_draws=None, seed=0):
    """The reference's my_nlp(mv = TRUE) (R/evaluation_functions.R:21-26, 66-80, 120-133) on the
    MI355X (sgp_joint_nlp): {"nlp", "mcsd", "mcn", "nlp_se"}.  gaussian: -dmvnorm(y, pred_mean,
    pred_cov + tau^2 I) as written (mcsd, nlp_se NaN; mcn None).  bernoulli / poisson: the Monte
    Carlo estimate over n_draws (or par["n"], the reference's place for it) joint draws from the
    library's own counter-based normal stream (include/sgp.h), so the result is a function of
    (inputs, n_draws, seed) alone.  nlp_se is the delta-method standard error of nlp."""
    if family not in _lib.SCORE_FAMILIES:
        raise ValueError(f"family must be one of {sorted(_lib.SCORE_FAMILIES)}, not {family!r}")
    from .vi import _device
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
    n = y.size
    pm = np.ascontiguousarray(np.asarray(pred_mean, dtype=np.float64).reshape(-1))
    if pm.size != n:
        raise ValueError(f"pred_mean has {pm.size} values for {n} rows")
    cov = _sym_cov("pred_cov", pred_cov, n)
    p, expo = _score_par(family, par)
    if expo is not None and expo.size != n:
        raise ValueError(f"par['m'] has {expo.size} values for {n} rows")
    if family == "gaussian":
        S = 1
    else:
        if n_draws is None:
            n_draws = (par or {}).get("n")
        if n_draws is None:
            raise ValueError("a Monte Carlo score needs n_draws (or par['n'])")
        S = int(n_draws)
    out = np.zeros(3)
    _call(_lib.lib().sgp_joint_nlp(_device(), _lib.SCORE_FAMILIES[family], _lib.dptr(y),
                                   _lib.dptr(pm), _lib.dptr(cov), n, max(n, 1), p,
                                   None if expo is None else _lib.dptr(expo), S, _seed(seed),
                                   _lib.dptr(out)))
    return {"nlp": float(out[0]), "mcsd": float(out[1]),
            "mcn": None if family == "gaussian" else S, "nlp_se": float(out[2])}


def joint_kl(mean1, mean2, sigma1, sigma2):
    """The reference's my_kl(mv = TRUE) as written (R/evaluation_functions.R:155-163) on the MI355X
    (sgp_joint_kl).  Its log-determinant term is sum log diag chol2 - sum log diag chol1, half the
    log-determinant difference, so the value is not the KL divergence."""
    from .vi import _device
    m1 = np.ascontiguousarray(np.asarray(mean1, dtype=np.float64).reshape(-1))
    m2 = np.ascontiguousarray(np.asarray(mean2, dtype=np.float64).reshape(-1))
    n = m1.size
    if m2.size != n:
        raise ValueError(f"mean2 has {m2.size} values, mean1 {n}")
    s1, s2 = _sym_cov("sigma1", sigma1, n), _sym_cov("sigma2", sigma2, n)
    kl = np.zeros(1)
    _call(_lib.lib().sgp_joint_kl(_device(), _lib.dptr(m1), _lib.dptr(m2), _lib.dptr(s1),
                                  max(n, 1), _lib.dptr(s2), max(n, 1), n, _lib.dptr(kl)))
    return float(kl[0])


def mc_nlp(y, pred_mean, pred_var, n_draws, seed=0):
    """The reference's my_nlp(family = "bernoulli", mc = TRUE) (R/evaluation_functions.R:53-65) on
    the MI355X (sgp_mc_nlp), with the library's own normal stream: {"nlp", "mcsd", "mcn"}."""
    from .vi import _device
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
    n = y.size
    pm = np.ascontiguousarray(np.asarray(pred_mean, dtype=np.float64).reshape(-1))
    pv = np.ascontiguousarray(np.asarray(pred_var, dtype=np.float64).reshape(-1))
    if pm.size != n or pv.size != n:
        raise ValueError(f"pred_mean / pred_var have {pm.size} / {pv.size} values for {n} rows")
    S = int(n_draws)
    nlp, mcsd = np.zeros(n), np.zeros(n)
    _call(_lib.lib().sgp_mc_nlp(_device(), _lib.dptr(y), _lib.dptr(pm), _lib.dptr(pv), n, S,
                                _seed(seed), _lib.dptr(nlp), _lib.dptr(mcsd)))
    return {"nlp": nlp, "mcsd": mcsd, "mcn": S}


def predict_prob(pred_mean, pred_var):
    """The averaged class probability int sigma(f) N(f; pred_mean, pred_var) df of a bernoulli
    prediction (the vignette approximates it by 1 / (1 + exp(-pred_mean)))."""
    pm = np.asarray(pred_mean, dtype=np.float64).reshape(-1)
    return np.exp(-_nlp("bernoulli", np.ones(pm.size), pm, pred_var, 0.0, None)[0])


def score_gp(mod, x_test, y_test, mu_pred=None, vi=False, par=None, *, joint=False, n_draws=None,
             seed=0):
    """predict_gp(mod, x_test, mu_pred, full_cov = FALSE, vi) scored against y_test as the
    reference's experiment scripts do (exec/boston.R:185-201): {"pred", "nlp", "median_nlp",
    "mean_nlp", "rmse", "srmse" = rmse / sd(y_test) (R's n - 1 sd), "n_nan"}.  par defaults to the
    fit's tau (gaussian) and to m = 1 (poisson).  median and mean are over the finite nlp.
    joint = True also predicts with full_cov = TRUE and adds "joint_nlp" = joint_nlp(y_test, that
    mean, that covariance, family, par, n_draws, seed); every other field is unchanged."""
    from .predict import _predict
    family = mod["family"]
    res = mod["results"]
    delta = mod.get("delta", 1e-6)
    if vi and family != "gaussian":
        return "Error: VI not supported for non-gaussian data."
    x_test = np.asarray(x_test, dtype=np.float64)
    if x_test.ndim == 1:
        x_test = x_test.reshape(-1, 1)
    y_test = np.asarray(y_test, dtype=np.float64).reshape(-1)
    if mu_pred is None or np.any(np.isnan(np.asarray(mu_pred, dtype=np.float64))):
        mu_pred = np.zeros(x_test.shape[0])
    if par is None and family == "gaussian":
        par = {"tau": res["cov_par"]["tau"]}
    p, expo = _score_par(family, par)
    score = (family, y_test, p, expo)
    gaussian = family == "gaussian"
    if not mod.get("sparse", True):
        if not gaussian:
            W = np.asarray(res["W"], dtype=np.float64).reshape(-1)
            xy = np.asarray(res["xy"], dtype=np.float64).reshape(W.size, -1)
            out = _predict(_lib.SGP_PRED_LAPLACE_FULL, False, res["grad_log_py_ff"], None, xy,
                           x_test, res["cov_fun"], res["cov_par"], mu_pred, W, False, delta, score)
        else:
            yt = np.asarray(res["y"], dtype=np.float64).reshape(-1)
            xy = np.asarray(res["xy"], dtype=np.float64).reshape(yt.size, -1)
            mu = np.broadcast_to(np.asarray(res["mu"], dtype=np.float64), yt.shape)
            out = _predict(_lib.SGP_PRED_FULL, True, yt, None, xy, x_test, res["cov_fun"],
                           res["cov_par"], mu_pred, mu, False, delta, score)
    elif vi:
        out = _predict(_lib.SGP_PRED_VI, gaussian, res["u_mean"], res["u_var"], res["xu"], x_test,
                       res["cov_fun"], res["cov_par"], mu_pred, res["muu"], False, delta, score)
    else:
        m = np.asarray(res["xu"]).shape[0]
        out = _predict(_lib.SGP_PRED_LAPLACE, gaussian, np.asarray(res["u_mean"])[:m],
                       res["u_var"], res["xu"], x_test, res["cov_fun"], res["cov_par"], mu_pred,
                       np.asarray(res["muu"])[:m], False, delta, score)
    nlp, stats = out["nlp"], out["stats"]
    n = y_test.size
    rmse = math.sqrt(stats[3] / n)
    sd = float(np.std(y_test, ddof=1)) if n > 1 else float("nan")
    fin = nlp[np.isfinite(nlp)]
    result = {"pred": {"pred_mean": out["pred_mean"], "pred_var": out["pred_var"]},
              "nlp": nlp,
              "median_nlp": float(np.median(fin)) if fin.size else float("nan"),
              "mean_nlp": float(stats[0] / stats[1]) if stats[1] > 0 else float("nan"),
              "rmse": rmse, "srmse": rmse / sd, "n_nan": int(stats[2])}
    if joint:
        from .predict import predict_gp
        full = predict_gp(mod, x_test, mu_pred, full_cov=True, vi=vi)["pred"]
        result["joint_nlp"] = joint_nlp(y_test, full["pred_mean"], full["pred_var"], family, par,
                                        n_draws, seed)
    return result
