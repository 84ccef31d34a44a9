"""The oracles of the held-out scores against each other, without a GPU (tests/nlp_oracle.py).

* the numpy model of sgp_quad.h against the 50-digit truth frozen in tests/golden/nlp_grid.npz,
  on the whole fixture, at 1e-12 max(1, |nlp|) (oracle against mpmath);
* the frozen truth against a fresh mpmath evaluation on a few rows (the fixture is what
  make_nlp_golden.py writes);
* the gaussian closed form against scipy's norm.logpdf;
* the literal restatement of my_nlp (QUADPACK QAGI with integrate()'s tolerances) against the
  truth where integrate() works: every grid row with s2 >= 0.05 and true nlp <= 4, at
  integrate()'s own absolute-plus-relative tolerance carried through the logarithm;
* the quirk: on a confident bernoulli prediction the literal restatement returns a non-finite
  nlp, the model the true 0.8543552...
"""
import os

import numpy as np
import pytest

import nlp_oracle as NO

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nlp_grid.npz")


@pytest.fixture(scope="module")
def grid():
    return {k: v for k, v in np.load(GOLD).items()}


def _model(g):
    out = np.empty(g["nlp"].size)
    for f, name in ((0, "poisson"), (1, "bernoulli")):
        k = g["fam"] == f
        out[k] = NO.model_nlp(name, g["y"][k], g["mu"][k], g["s2"][k], expo=g["m"][k])
    return out


def test_fixture_is_the_grid(grid):
    fam, y, mu, s2, m = NO.grid_cases()
    assert grid["nlp"].size == 615
    for k, v in (("fam", fam), ("y", y), ("mu", mu), ("s2", s2), ("m", m)):
        assert np.array_equal(grid[k], v), k
    # the named rows
    assert abs(grid["nlp"][612] - 0.854355) < 1e-6
    assert abs(grid["nlp"][613] - 96.516468834) < 1e-8
    assert np.isfinite(grid["nlp"][614])


def test_fixture_rows_recomputed(grid):
    for i in (0, 71, 100, 347, 611, 612, 613):
        v = NO.mp_nlp(NO.FAMILY_NAMES[int(grid["fam"][i])], grid["y"][i], grid["mu"][i],
                      grid["s2"][i], grid["m"][i])
        assert v == grid["nlp"][i], i


def test_model_against_truth(grid):
    got = _model(grid)
    err = np.abs(got - grid["nlp"]) / np.maximum(1.0, np.abs(grid["nlp"]))
    print("model against mpmath: max %.3g at row %d" % (err.max(), err.argmax()))
    assert np.all(np.isfinite(got))
    assert err.max() <= 1e-12


def test_gaussian_closed_form():
    from scipy import stats
    rng = np.random.default_rng(3)
    y, mu = rng.normal(0, 3, 50), rng.normal(0, 3, 50)
    s2 = 10.0 ** rng.uniform(-6, 2, 50)
    for tau in (0.0, 0.4, 7.0):
        ref = -stats.norm.logpdf(y, loc=mu, scale=np.sqrt(s2 + tau ** 2))
        got = NO.model_nlp("gaussian", y, mu, s2, par=tau)
        assert np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))) <= 1e-13
        lit = NO.literal_nlp("gaussian", y, mu, s2, {"tau": tau})
        assert np.array_equal(lit, ref)
        one = NO.mp_nlp("gaussian", y[0], mu[0], s2[0], tau=tau)
        assert abs(one - ref[0]) <= 1e-13 * max(1.0, abs(ref[0]))


def test_literal_restatement_where_integrate_works(grid):
    """The 186 grid rows with s2 >= 0.05 and true nlp <= 4; none left out."""
    sel = (np.arange(615) < 612) & (grid["s2"] >= 0.05) & (grid["nlp"] <= 4.0)
    assert sel.sum() == 186
    worst = 0.0
    for i in np.flatnonzero(sel):
        fam = NO.FAMILY_NAMES[int(grid["fam"][i])]
        lit = NO.literal_nlp(fam, [grid["y"][i]], [grid["mu"][i]], [grid["s2"][i]],
                             {"m": float(grid["m"][i])})[0]
        bound = 2.0 * NO.R_TOL * (1.0 + np.exp(grid["nlp"][i]))
        d = abs(lit - grid["nlp"][i])
        worst = max(worst, d / bound)
        assert d <= bound, (i, fam, lit, grid["nlp"][i], bound)
    print("literal restatement: worst |delta| / bound = %.3g" % worst)


def test_integrate_misses_a_confident_prediction(grid):
    """Quirk Q21: y = 1, pred_mean = -0.3, pred_var = 1e-6."""
    lit = NO.literal_nlp("bernoulli", [1.0], [-0.3], [1e-6])[0]
    assert not np.isfinite(lit)
    got = NO.model_nlp("bernoulli", [1.0], [-0.3], [1e-6])[0]
    assert abs(got - 0.8543552) < 1e-7 and abs(got - grid["nlp"][612]) <= 1e-12


def test_literal_kl_and_rmse():
    rng = np.random.default_rng(5)
    m1, m2 = rng.normal(size=7), rng.normal(size=7)
    s1, s2 = rng.uniform(0.2, 2, 7), rng.uniform(0.2, 2, 7)
    assert NO.literal_kl(m1, m1, s1, s1) == pytest.approx(0.0, abs=1e-14)
    assert NO.literal_kl(m1, m2, s1, s2) > 0.0
    assert NO.literal_rmse(m1, m1 + 2.0) == pytest.approx(2.0, rel=1e-15)
