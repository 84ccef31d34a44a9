"""The joint-score oracle (tests/joint_oracle.py) against independent answers, without a GPU.

With a diagonal covariance the joint probability factorises, so the oracle's Monte Carlo estimate
must agree with the product of the one-dimensional quadratures (tests/nlp_oracle.py) within its own
standard error; the KL as written differs from the true KL by exactly a quarter of the
log-determinant difference; the Gaussian joint score with a diagonal covariance is the sum of the
per-row scores.
"""
import math

import numpy as np
import pytest

import joint_oracle as JO
import nlp_oracle as NO

VAR = np.array([0.5, 1.5, 0.2, 0.8, 1.0])
DIAG_CASES = {
    "bernoulli": dict(mu=np.array([0.3, -0.5, 1.0, 0.2, -1.2]), y=np.array([1.0, 0, 1, 1, 0])),
    "poisson": dict(mu=np.array([0.1, 0.9, 0.0, 1.6, 0.5]), y=np.array([0.0, 3, 1, 7, 2])),
}
SEED, S = 2, 65536


@pytest.mark.parametrize("family", ["bernoulli", "poisson"])
def test_diagonal_covariance_agrees_with_the_quadratures(family):
    c = DIAG_CASES[family]
    r = JO.joint_nlp(family, c["y"], c["mu"], np.diag(VAR), par=1.0, S=S, seed=SEED)
    p_quad = math.exp(-NO.model_nlp(family, c["y"], c["mu"], VAR, par=1.0).sum())
    se = r["mcsd"] / math.sqrt(S)
    print("%s: p = %.8g, quadrature %.8g, %.3g standard errors apart"
          % (family, r["p"], p_quad, abs(r["p"] - p_quad) / se))
    assert abs(r["p"] - p_quad) <= 4.0 * se
    assert abs(r["nlp"] + math.log(r["p"])) <= 1e-12
    # the delta-method standard error of nlp = -log p
    assert abs(r["nlp_se"] - se / r["p"]) <= 1e-12 * r["nlp_se"]


def test_gaussian_joint_with_a_diagonal_covariance_is_the_sum_of_rows():
    rng = np.random.default_rng(5)
    n, tau = 9, 0.4
    y, mu, v = rng.normal(size=n), rng.normal(size=n), rng.uniform(0.2, 2.0, n)
    got = JO.joint_nlp("gaussian", y, mu, np.diag(v), par=tau)["nlp"]
    ref = NO.model_nlp("gaussian", y, mu, v, par=tau).sum()
    assert abs(got - ref) <= 1e-12 * abs(ref)


def test_kl_as_written_is_a_quarter_log_det_off():
    rng = np.random.default_rng(3)
    n = 7
    A, B = rng.normal(size=(n, n)), rng.normal(size=(n, n))
    s1, s2 = A @ A.T + n * np.eye(n), B @ B.T + 0.5 * n * np.eye(n)
    m1, m2 = rng.normal(size=n), rng.normal(size=n)
    lit, true = JO.kl_as_written(m1, m2, s1, s2), JO.kl_true(m1, m2, s1, s2)
    gap = 0.25 * (np.linalg.slogdet(s2)[1] - np.linalg.slogdet(s1)[1])
    assert abs(gap) > 0.05
    assert abs((true - lit) - gap) <= 1e-13 * max(1.0, abs(true))
    assert abs(JO.kl_as_written(m1, m1, s1, s1)) <= 1e-13
    assert JO.kl_true(m1, m2, s1, s2) > 0


def test_single_draw_has_no_spread():
    c = DIAG_CASES["bernoulli"]
    r = JO.joint_nlp("bernoulli", c["y"], c["mu"], np.diag(VAR), S=1, seed=1)
    assert math.isnan(r["mcsd"]) and math.isnan(r["nlp_se"]) and math.isfinite(r["nlp"])
    nlp, mcsd = JO.mc_nlp(c["y"], c["mu"], VAR, 1, 1)
    assert np.all(np.isnan(mcsd)) and np.all(np.isfinite(nlp))


def test_per_row_monte_carlo_agrees_with_the_quadrature():
    c = DIAG_CASES["bernoulli"]
    Sr = 16384
    nlp, mcsd = JO.mc_nlp(c["y"], c["mu"], VAR, Sr, SEED)
    p_quad = np.exp(-NO.model_nlp("bernoulli", c["y"], c["mu"], VAR))
    assert np.all(np.abs(np.exp(-nlp) - p_quad) <= 5.0 * mcsd / math.sqrt(Sr))
