"""Joint predictive scoring and GP draws on the MI355X: the Cholesky factor (sgp_diag_chol), the
normal stream (sgp_diag_normals), sgp_sample_mvn, sgp_joint_nlp, sgp_joint_kl, sgp_mc_nlp and their
Python wrappers, against the numpy restatement tests/joint_oracle.py on the same stream.

Matrices are A = sqexp K(x, x) + (tau^2 + delta) I with x ~ U(0, 10)^2, sigma = l = 1, tau = 0.5
(condition number <= 60 at n <= 200).  The bars come from the arithmetic, not from the results: a
blocked Cholesky with explicit diagonal-block inverses is within 2e-15 of LAPACK's at these sizes,
so 1e-12 max|L| is a loose cap; the draws and scores carry that factor's error times n.
"""
import math
import os
import re
from collections import OrderedDict

import numpy as np
import pytest

import joint_oracle as JO
from oracle import sgp_oracle as O

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAM = {"poisson": 0, "bernoulli": 1, "gaussian": 2}
TAU, M_EXPO = 0.3, 1.7


@pytest.fixture(scope="module")
def sgp():
    import sparsergps_amd as S
    from sparsergps_amd import _lib
    _lib.require_gpu()
    return S


def _lib():
    from sparsergps_amd import _lib as L
    return L


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


_COV = {}


def _cov(n, seed=0):
    """The test matrix of order n (cached; never modified by a test)."""
    if (n, seed) not in _COV:
        a = JO.sqexp_cov(n, 100 * seed + n)
        a.setflags(write=False)
        _COV[(n, seed)] = a
    return _COV[(n, seed)]


def _order(msg):
    m = re.search(r"leading minor of order (\d+)", msg)
    assert m, msg
    return int(m.group(1))


# ------------------------------------------------------------------ the factor
def _chol(A, n, lda=None, ldl=None):
    L_ = _lib()
    lda, ldl = lda or n, ldl or n
    a = np.full((lda, n), np.nan, order="F")
    a[:n] = np.tril(A)           # only the lower triangle is read: the rest stays NaN
    a[:n][np.triu_indices(n, 1)] = np.nan
    out = np.full((ldl, n), -7.0, order="F")
    ld = np.zeros(1)
    L_.check(L_.lib().sgp_diag_chol(0, L_.dptr(a), n, lda, L_.dptr(out), ldl, L_.dptr(ld)))
    return out, float(ld[0])


@pytest.mark.parametrize("n,lda,ldl", [(1, None, None), (2, None, None), (63, None, None),
                                       (64, None, None), (65, None, None), (128, None, None),
                                       (129, None, None), (200, None, None), (129, 140, 135)])
def test_factor(sgp, n, lda, ldl):
    A = _cov(n)
    out, ld = _chol(A, n, lda, ldl)
    L = out[:n]
    ref = np.linalg.cholesky(A)
    e1 = np.abs(L - ref).max() / np.abs(ref).max()
    e2 = np.abs(L @ L.T - A).max() / np.abs(A).max()
    sld = np.linalg.slogdet(A)[1]
    print("chol n = %d: max|L - L_ref| / max|L| = %.3g, max|L L^T - A| / max|A| = %.3g, "
          "logdet rel %.3g" % (n, e1, e2, abs(ld - sld) / abs(sld)))
    assert e1 <= 1e-12 and e2 <= 1e-13
    assert np.all(L[np.triu_indices(n, 1)] == 0.0)
    assert abs(ld - sld) <= 1e-12 * abs(sld)
    if ldl:   # the rows past n of the strided output are untouched
        assert np.all(out[n:] == -7.0)


@pytest.mark.parametrize("k", [1, 64, 65, 130])
def test_factor_not_pd_order(sgp, k):
    n = 200
    A = _cov(n).copy()
    A[k - 1, k - 1] = -1.0
    with pytest.raises(sgp.NotPositiveDefinite) as ei:
        _chol(A, n)
    # numpy's order: the first leading minor whose factorisation fails
    if k > 1:
        np.linalg.cholesky(A[:k - 1, :k - 1])
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(A[:k, :k])
    assert _order(str(ei.value)) == k and " of A " in str(ei.value)


# ------------------------------------------------------------------ the normals
@pytest.mark.parametrize("stream", [0, 1])
@pytest.mark.parametrize("S,n", [(1, 1), (3, 5), (257, 130)])
def test_normals(sgp, S, n, stream):
    L_ = _lib()
    seed = 0xfedcba9876543210
    out = np.zeros((S, n), order="F")
    L_.check(L_.lib().sgp_diag_normals(0, seed, stream, S, n, L_.dptr(out)))
    err = np.abs(out - JO.normals(seed, stream, S, n)).max()
    print("normals stream %d (S, n) = (%d, %d): max abs error %.3g" % (stream, S, n, err))
    assert err <= 1e-13


# ------------------------------------------------------------------ draws
def _mean(n):
    return np.random.default_rng(7 + n).normal(size=n)


def _diag_sample(mean, cov, S, seed, chunk, blocks=0):
    L_ = _lib()
    n = mean.size
    out = np.zeros((S, n), order="F")
    cov = np.asfortranarray(cov)
    L_.check(L_.lib().sgp_diag_sample_mvn(0, chunk, blocks, L_.dptr(mean), L_.dptr(cov), n, n, S,
                                          seed, L_.dptr(out), S, None))
    return out


@pytest.mark.parametrize("S", [1, 5, 257])
@pytest.mark.parametrize("n", [1, 65, 130])
def test_draws(sgp, n, S):
    mean, cov, seed = _mean(n), _cov(n), 11
    got = sgp.sample_mvn(mean, cov, S, seed)
    assert got.shape == (S, n)
    ref = JO.draws(mean, cov, S, seed)
    err = (np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()
    print("draws n = %d, S = %d: max error / max(1, |f|) = %.3g" % (n, S, err))
    assert err <= 1e-12
    assert np.array_equal(_bits(got), _bits(sgp.sample_mvn(mean, cov, S, seed)))
    for chunk in (0, 64, 100):
        assert np.array_equal(_bits(got), _bits(_diag_sample(mean, cov, S, seed, chunk))), chunk
    assert np.array_equal(_bits(got), _bits(_diag_sample(mean, cov, S, seed, 100, 7)))
    assert not np.array_equal(_bits(got), _bits(sgp.sample_mvn(mean, cov, S, seed + 1)))


# ------------------------------------------------------------------ joint scores
def _joint(family, y, pm, cov, par, S, seed, expo=None, chunk=None, blocks=0):
    L_ = _lib()
    y, pm = (np.ascontiguousarray(v, dtype=np.float64) for v in (y, pm))
    cov = np.asfortranarray(cov)
    ex = None if expo is None else np.ascontiguousarray(expo, dtype=np.float64)
    n, out = y.size, np.zeros(3)
    tail = (L_.dptr(y), L_.dptr(pm), L_.dptr(cov), n, n, float(par),
            None if ex is None else L_.dptr(ex), S, seed, L_.dptr(out))
    if chunk is None:
        L_.check(L_.lib().sgp_joint_nlp(0, FAM[family], *tail))
    else:
        L_.check(L_.lib().sgp_diag_joint_nlp(0, FAM[family], chunk, blocks, *tail, None))
    return out


def _response(family, n):
    rng = np.random.default_rng(31 + n)
    pm = 0.5 * rng.normal(size=n)
    if family == "bernoulli":
        return (rng.uniform(size=n) < 0.5).astype(np.float64), pm
    return rng.poisson(M_EXPO * np.exp(pm)).astype(np.float64), pm


@pytest.mark.parametrize("n", [1, 64, 65, 129])
def test_gaussian_joint_score(sgp, n):
    rng = np.random.default_rng(n)
    y, pm, cov = rng.normal(size=n), 0.3 * rng.normal(size=n), _cov(n)
    got = sgp.joint_nlp(y, pm, cov, family="gaussian", par={"tau": TAU})
    ref = JO.joint_nlp("gaussian", y, pm, cov, par=TAU)["nlp"]
    print("gaussian joint n = %d: nlp %.12g, rel error %.3g" % (n, got["nlp"],
                                                                abs(got["nlp"] - ref) / abs(ref)))
    assert abs(got["nlp"] - ref) <= 1e-11 * abs(ref)
    assert math.isnan(got["mcsd"]) and math.isnan(got["nlp_se"]) and got["mcn"] is None


@pytest.mark.parametrize("S", [1, 257, 4096])
@pytest.mark.parametrize("n", [1, 64, 65, 129])
@pytest.mark.parametrize("family", ["bernoulli", "poisson"])
def test_monte_carlo_joint_score(sgp, family, n, S):
    y, pm = _response(family, n)
    cov, seed = _cov(n), 5
    par = {"m": M_EXPO} if family == "poisson" else None
    got = sgp.joint_nlp(y, pm, cov, family=family, par=par, n_draws=S, seed=seed)
    ref = JO.joint_nlp(family, y, pm, cov, par=M_EXPO, S=S, seed=seed)
    print("%s joint n = %d, S = %d: nlp %.12g (oracle %.12g), mcsd %.6g (%.6g), nlp_se %.6g (%.6g)"
          % (family, n, S, got["nlp"], ref["nlp"], got["mcsd"], ref["mcsd"], got["nlp_se"],
             ref["nlp_se"]))
    assert got["mcn"] == S
    assert abs(got["nlp"] - ref["nlp"]) <= 1e-10 * max(1.0, abs(ref["nlp"]))
    if S == 1:
        assert math.isnan(got["mcsd"]) and math.isnan(got["nlp_se"])
    else:
        assert abs(got["mcsd"] - ref["mcsd"]) <= 1e-9 * ref["mcsd"]
        assert abs(got["nlp_se"] - ref["nlp_se"]) <= 1e-9 * ref["nlp_se"]


@pytest.mark.parametrize("S", [257, 4096])
@pytest.mark.parametrize("family", ["bernoulli", "poisson"])
def test_joint_score_bits_do_not_depend_on_chunks_or_grid(sgp, family, S):
    n = 65
    y, pm = _response(family, n)
    cov = _cov(n)
    base = _joint(family, y, pm, cov, M_EXPO, S, 9)
    assert np.all(np.isfinite(base))
    for chunk, blocks in ((0, 0), (64, 0), (100, 0), (0, 7), (100, 7)):
        got = _joint(family, y, pm, cov, M_EXPO, S, 9, chunk=chunk, blocks=blocks)
        assert np.array_equal(_bits(base), _bits(got)), (chunk, blocks)
    assert np.array_equal(_bits(base), _bits(_joint(family, y, pm, cov, M_EXPO, S, 9)))
    assert not np.array_equal(_bits(base), _bits(_joint(family, y, pm, cov, M_EXPO, S, 10)))


DIAG_VAR = np.array([0.5, 1.5, 0.2, 0.8, 1.0])
DIAG_CASES = {
    "bernoulli": (np.array([1.0, 0, 1, 1, 0]), np.array([0.3, -0.5, 1.0, 0.2, -1.2])),
    "poisson": (np.array([0.0, 3, 1, 7, 2]), np.array([0.1, 0.9, 0.0, 1.6, 0.5])),
}


@pytest.mark.parametrize("family", ["bernoulli", "poisson"])
def test_diagonal_covariance_against_the_row_scores(sgp, family):
    y, pm = DIAG_CASES[family]
    S = 65536
    par = {"m": 1.0} if family == "poisson" else None
    got = sgp.joint_nlp(y, pm, np.diag(DIAG_VAR), family=family, par=par, n_draws=S, seed=2)
    rows = sgp.my_nlp(y, pm, DIAG_VAR, family=family, par=par)["nlp"]
    p, p_quad = math.exp(-got["nlp"]), math.exp(-rows.sum())
    se = got["mcsd"] / math.sqrt(S)
    print("%s diagonal: p = %.8g, row scores %.8g, %.3g standard errors apart"
          % (family, p, p_quad, abs(p - p_quad) / se))
    assert abs(p - p_quad) <= 4.0 * se


def test_constant_exposure_vector_is_the_scalar_call(sgp):
    n, S = 65, 257
    y, pm = _response("poisson", n)
    a = _joint("poisson", y, pm, _cov(n), M_EXPO, S, 3)
    b = _joint("poisson", y, pm, _cov(n), 1.0, S, 3, expo=np.full(n, M_EXPO))
    assert np.array_equal(_bits(a), _bits(b))
    c = sgp.joint_nlp(y, pm, _cov(n), family="poisson", par={"m": np.full(n, M_EXPO)}, n_draws=S,
                      seed=3)
    assert np.array_equal(_bits(a), _bits([c["nlp"], c["mcsd"], c["nlp_se"]]))


# ------------------------------------------------------------------ the KL as written
@pytest.mark.parametrize("n", [1, 65, 129])
def test_joint_kl(sgp, n):
    rng = np.random.default_rng(n)
    m1, m2 = rng.normal(size=n), rng.normal(size=n)
    s1, s2 = _cov(n, 1), _cov(n, 2)
    got = sgp.joint_kl(m1, m2, s1, s2)
    ref = JO.kl_as_written(m1, m2, s1, s2)
    print("kl n = %d: %.12g, rel error %.3g" % (n, got, abs(got - ref) / abs(ref)))
    assert abs(got - ref) <= 1e-11 * abs(ref)
    assert abs(sgp.joint_kl(m1, m1, s1, s1)) <= 1e-10


# ------------------------------------------------------------------ per-row Monte Carlo
def _mc_rows(n):
    rng = np.random.default_rng(77 + n)
    y = (rng.uniform(size=n) < 0.5).astype(np.float64)
    return y, rng.normal(size=n), rng.uniform(0.2, 2.0, n)


@pytest.mark.parametrize("S", [1, 2, 4097])
@pytest.mark.parametrize("n", [1, 130])
def test_mc_nlp(sgp, n, S):
    y, pm, pv = _mc_rows(n)
    got = sgp.mc_nlp(y, pm, pv, S, seed=4)
    nlp, mcsd = JO.mc_nlp(y, pm, pv, S, 4)
    assert got["mcn"] == S
    assert np.all(np.abs(got["nlp"] - nlp) <= 1e-10 * np.abs(nlp))
    if S == 1:
        assert np.all(np.isnan(got["mcsd"]))
    else:
        assert np.all(np.abs(got["mcsd"] - mcsd) <= 1e-10 * mcsd)


def test_mc_nlp_against_the_quadrature(sgp):
    n, S, seed = 130, 16384, 4
    y, pm, pv = _mc_rows(n)
    p_quad = np.exp(-sgp.my_nlp(y, pm, pv, family="bernoulli")["nlp"])
    nlp, mcsd = JO.mc_nlp(y, pm, pv, S, seed)
    z_ref = np.abs(np.exp(-nlp) - p_quad) / (mcsd / math.sqrt(S))
    print("per-row Monte Carlo, oracle: largest distance %.3g standard errors" % z_ref.max())
    assert np.all(z_ref <= 5.0)
    got = sgp.mc_nlp(y, pm, pv, S, seed=seed)
    z = np.abs(np.exp(-got["nlp"]) - p_quad) / (got["mcsd"] / math.sqrt(S))
    print("per-row Monte Carlo, device: largest distance %.3g standard errors" % z.max())
    assert np.all(z <= 5.0)


# ------------------------------------------------------------------ composition
@pytest.fixture(scope="module")
def vi_fit(sgp):
    z = np.load(os.path.join(GOLD, "gauss_c2_small.npz"))
    cp = OrderedDict(zip([str(s) for s in z["names"]], (float(v) for v in z["theta"])))
    cf, dl = str(z["cov_fun"]), float(z["delta"])
    X, y, mu, U = z["X"], z["y"], z["mu"], z["U"]
    tr, te = slice(0, 150), slice(150, 200)
    muu = np.full(U.shape[0], mu[0])
    um, uv = O.vi_posterior_u(cp, cf, U, X[tr], y[tr], mu[tr], muu, dl)
    mod = {"family": "gaussian", "sparse": True, "delta": dl,
           "results": {"u_mean": um, "u_var": uv, "xu": U, "cov_fun": cf, "cov_par": cp,
                       "muu": muu}}
    return mod, X[te], y[te], mu[te], True


@pytest.fixture(scope="module")
def bern_fit(sgp):
    z = np.load(os.path.join(GOLD, "bernoulli_small.npz"))
    cp = OrderedDict(zip(("sigma", "l", "tau"), (float(v) for v in z["theta"])))
    dl, U = float(z["delta"]), z["U"]
    muu = np.zeros(U.shape[0])
    with sgp.SparseGPContext(z["X"], z["y"], z["mu"], m_max=U.shape[0]) as ctx:
        sgp.newtrap_sparseGP(z["f0"], cp, "sqexp", z["X"], U, z["y"], z["mu"], 1.0, dl,
                             tol=float(z["tol"]), ctx=ctx, family="bernoulli")
        um, uv = ctx.posterior_u(muu)
    mod = {"family": "bernoulli", "sparse": True, "delta": dl,
           "results": {"u_mean": um, "u_var": uv, "xu": U, "cov_fun": "sqexp", "cov_par": cp,
                       "muu": muu}}
    return mod, z["X"][:60], z["y"][:60], np.zeros(60), False


@pytest.mark.parametrize("which", ["vi_fit", "bern_fit"])
def test_composition(sgp, request, which):
    mod, x, y, mu_pred, vi = request.getfixturevalue(which)
    family = mod["family"]
    full = sgp.predict_gp(mod, x, mu_pred, full_cov=True, vi=vi)["pred"]
    S, seed = 33, 6
    f = sgp.sample_gp(mod, x, S, seed=seed, mu_pred=mu_pred, vi=vi)
    assert f.shape == (S, y.size)
    assert np.array_equal(_bits(f), _bits(sgp.sample_mvn(full["pred_mean"], full["pred_var"], S,
                                                         seed)))
    plain = sgp.score_gp(mod, x, y, mu_pred=mu_pred, vi=vi)
    sc = sgp.score_gp(mod, x, y, mu_pred=mu_pred, vi=vi, joint=True, n_draws=300, seed=seed)
    assert "joint_nlp" not in plain and set(sc) == set(plain) | {"joint_nlp"}
    par = {"tau": mod["results"]["cov_par"]["tau"]} if family == "gaussian" else None
    ref = sgp.joint_nlp(y, full["pred_mean"], full["pred_var"], family=family, par=par,
                        n_draws=300, seed=seed)
    assert sc["joint_nlp"]["mcn"] == ref["mcn"] and math.isfinite(ref["nlp"])
    for key in ("nlp", "mcsd", "nlp_se"):
        assert np.array_equal(_bits(sc["joint_nlp"][key]), _bits(ref[key])), key
    for key in plain:
        if key == "pred":
            for k2 in ("pred_mean", "pred_var"):
                assert np.array_equal(_bits(sc["pred"][k2]), _bits(plain["pred"][k2]))
        else:
            assert np.array_equal(_bits(sc[key]), _bits(plain[key])), key


# ------------------------------------------------------------------ failure
def test_not_positive_definite_names_the_order(sgp):
    n, k = 70, 66
    bad = _cov(n).copy()
    bad[k - 1, k - 1] = -1.0
    y, pm = _response("bernoulli", n)
    with pytest.raises(sgp.NotPositiveDefinite) as ei:
        sgp.sample_mvn(pm, bad, 4, 1)
    assert _order(str(ei.value)) == k and "sgp_sample_mvn" in str(ei.value)
    with pytest.raises(sgp.NotPositiveDefinite) as ei:
        sgp.joint_nlp(y, pm, bad, family="bernoulli", n_draws=4)
    assert _order(str(ei.value)) == k and "pred_cov" in str(ei.value)
    with pytest.raises(sgp.NotPositiveDefinite) as ei:
        sgp.joint_nlp(y, pm, bad, family="gaussian", par={"tau": 0.1})
    assert _order(str(ei.value)) == k and "pred_cov + tau^2 I" in str(ei.value)
    with pytest.raises(sgp.NotPositiveDefinite) as ei:
        sgp.joint_kl(pm, pm, _cov(n), bad)
    assert _order(str(ei.value)) == k and "sigma2" in str(ei.value)
    with pytest.raises(sgp.NotPositiveDefinite) as ei:
        sgp.joint_kl(pm, pm, bad, _cov(n))
    assert _order(str(ei.value)) == k and "sigma1" in str(ei.value)
