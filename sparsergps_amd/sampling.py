"""Draws from a Gaussian process, prior or posterior.

The reference's vignettes and exec/simulated_examples.R:15 begin by drawing a GP sample with
mvtnorm::rmvnorm from a make_cov_matC matrix.  R's stream cannot be reproduced (rmvnorm defaults to
an eigen-decomposition, rnorm inverts Mersenne-Twister output), so the draws come from the
library's own counter-based normal stream (include/sgp.h): f = mean + L z with L the Cholesky
factor taken on the MI355X, a function of (mean, cov, seed) alone that a host can regenerate.

  sample_mvn  n_draws x n draws from N(mean, cov), one per row as rmvnorm returns them
  sample_gp   predict_gp(full_cov = TRUE) followed by sample_mvn on its mean and covariance
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .evaluation import _call, _seed, _sym_cov


def sample_mvn(mean, cov, n_draws, seed=0):
    """n_draws draws from N(mean, cov) (sgp_sample_mvn): an n_draws x n matrix, one draw per row.
    cov is used as given (the caller adds any nugget); one that is not positive definite raises
    NotPositiveDefinite naming the order of the first leading minor that is not."""
    from .vi import _device
    mean = np.ascontiguousarray(np.asarray(mean, dtype=np.float64).reshape(-1))
    n = mean.size
    cov = _sym_cov("cov", cov, n)
    S = int(n_draws)
    out = np.zeros((max(S, 0), n), dtype=np.float64, order="F")
    _call(_lib.lib().sgp_sample_mvn(_device(), _lib.dptr(mean), _lib.dptr(cov), n, max(n, 1), S,
                                    _seed(seed), _lib.dptr(out), max(S, 1)))
    return out


def sample_gp(mod, x_pred, n_draws, seed=0, mu_pred=None, vi=False):
    """Draws of the fitted process at x_pred: predict_gp(mod, x_pred, mu_pred, full_cov = TRUE, vi)
    followed by sample_mvn on its pred_mean and pred_var (n_draws x np)."""
    from .predict import predict_gp
    pred = predict_gp(mod, x_pred, mu_pred, full_cov=True, vi=vi)
    if isinstance(pred, str):
        return pred
    p = pred["pred"]
    return sample_mvn(p["pred_mean"], p["pred_var"], n_draws, seed)
